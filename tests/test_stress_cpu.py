"""Stress readout without a GPU: the two derivations of tests/stress_ref.py against each other, and the constitutive header stark_amd/csrc/stress.hpp
compiled with g++ (tests/host_stress/host_stress.cpp, test-only) against the restatement.

Tolerances: stresses like every element quantity of the suite, 1e-11 relative to max|reference| over the potential (or to the reference's own terms
where it has cancelled: stress_ref.rel_to_scale); stretches |error| <= 1e-11 * stretch_max^2 / stretch_i, what a route through the eigenvalues of
C = F^T F can deliver; flags exact, except for elements whose limiting argument lies within relative 1e-9 of zero."""
import ctypes
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import stress_ref as sr  # noqa: E402
from oracle import evaluator as ev  # noqa: E402

TOL = 1e-11


@pytest.fixture(scope="module")
def host_lib():
    out = os.path.join(tempfile.mkdtemp(prefix="mistark_host_stress_"), "host_stress.so")
    subprocess.run(["g++", "-std=c++17", "-O2", "-shared", "-fPIC", os.path.join(ROOT, "tests", "host_stress", "host_stress.cpp"), "-o", out], check=True)
    lib = ctypes.CDLL(out)
    lib.host_stress_eval.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p]
    return lib


def host_records(lib, prob, pot):
    kind, full = sr.KIND[pot.name]
    inp = sr.gathered_flat(prob, pot)
    rec = np.full((len(inp), 16), np.nan)
    assert lib.host_stress_eval(kind, int(full), inp.ctypes.data, inp.shape[1], len(inp), rec.ctypes.data) == 0
    return rec


@pytest.mark.parametrize("name", sr.NAMES)
def test_restatement_equals_oracle_derived_stress(name):
    prob, rec, terms, arg = sr.seeded_problem(name)
    pot = prob.potentials[0]
    sigma, E = sr.stress_from_oracle(prob, pot)
    assert (rec[:, 15] < 2.0).all() and (rec[:, 14] > 0.0).all()
    if sr.KIND[name][1]:
        assert (rec[:, 15] == 1.0).any() and (rec[:, 15] == 0.0).any()   # the limiting branch is taken in some elements and not in others
    for f in range(6):
        err = sr.rel_to_scale(rec[:, f], sigma[:, f], terms.max(), TOL)
        print("%s sigma[%d]: (A) against (B) rel %.3g" % (name, f, err))
        assert err < TOL
    # m * psi is the oracle's element energy (for triangles without their inflation term)
    err = np.abs(rec[:, 13] * rec[:, 14] - E).max() / np.abs(E).max()
    print("%s m psi against the oracle's energies: rel %.3g" % (name, err))
    assert err < TOL
    o = ev.evaluate_potential(prob, pot)
    assert np.abs(rec[:, 13] * rec[:, 14] + sr.inflation_energy(prob, pot) - o.E).max() < TOL * np.abs(o.E).max()


@pytest.mark.parametrize("name", sr.NAMES)
def test_host_build_equals_restatement(host_lib, name):
    prob, rec, terms, arg = sr.seeded_problem(name)
    got = host_records(host_lib, prob, prob.potentials[0])
    sr.check_records(got, rec, terms, arg, name)


def test_homogeneous_and_rest_states_on_the_host(host_lib):
    """The closed-form answers of tests/test_gpu_stress.py, through the g++ build."""
    for name in sr.NAMES:
        for prob, want in sr.homogeneous_cases(name):
            got = host_records(host_lib, prob, prob.potentials[0])
            sr.check_homogeneous(got, want, name)


def test_dry_context_refuses_both_entry_points():
    import ctypes as C

    from stark_amd import capi

    L = capi.lib()
    h = C.c_void_p()
    assert L.mistark_create_dry(C.byref(h)) == 0
    try:
        u = np.zeros(6)
        assert L.mistark_add_dof_set(h, b"u", u.ctypes.data, u.size) >= 0
        ne, kind = C.c_int64(), C.c_int32()
        out = np.zeros(20)
        for call in (lambda: L.mistark_potential_element_stress(h, 0, None, C.byref(ne), C.byref(kind)), lambda: L.mistark_nodal_stress(h, None, 0, out.ctypes.data)):
            assert call() < 0
            msg = L.mistark_last_error(h).decode()
            assert msg and "registration-only" in msg, msg
    finally:
        L.mistark_destroy(h)


def test_degenerate_elements_are_flagged_not_trapped(host_lib):
    for name in sr.NAMES:
        kind = sr.KIND[name][0]
        X, conn = sr.mesh_of(name, 3)
        x0 = X.copy()
        if kind == 0:  # node 3 of element 1 mirrored through the plane of its other three nodes: J < 0
            a, b, c, d = (x0[i] for i in conn[1])
            n = np.cross(b - a, c - a)
            n /= np.linalg.norm(n)
            x0[conn[1, 3]] = d - 2.0 * np.dot(d - a, n) * n
        elif kind == 1:  # two nodes coincide: det C = 0
            x0[conn[1, 2]] = x0[conn[1, 0]]
        else:  # zero length
            x0[conn[1, 1]] = x0[conn[1, 0]]
        prob = sr.make_problem([(name, conn[1:2], sr.PARAMS[name])], X, x0, np.zeros_like(X))
        got = host_records(host_lib, prob, prob.potentials[0])[0]
        assert got[15] >= 2.0, (name, got)
        assert (got[0:8] == 0.0).all() and got[12] == 0.0, (name, got)
        assert np.isfinite(got[[8, 9, 10, 11, 13, 14]]).all(), (name, got)
        rec, _, _ = sr.records(prob, prob.potentials[0])
        assert rec[0, 15] >= 2.0
