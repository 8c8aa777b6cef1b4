"""CPU: the record function of the Hessian spectrum report (stark_amd/csrc/spectrum_report.hpp compiled with g++, tests/host_spectrum/host_spectrum.cpp,
test-only) against the exact spectra of tests/psd_cases.py and the numpy restatement of tests/spectrum_ref.py; the committed tolerances; the C ABI.

The bound (tests/spectrum_ref.py states it): per element b = ||H_in - H_exact||_F + SQRT_OFF_TOL ||H||_F + rounding ||H||_F; here H_in is H_exact rounded
once, so the first term is zero. Every figure is printed before it is asserted."""
import ctypes
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import psd_cases as pc  # noqa: E402
import spectrum_ref as sp  # noqa: E402


@pytest.fixture(scope="module")
def host_lib():
    out = os.path.join(tempfile.mkdtemp(prefix="mistark_host_spectrum_"), "host_spectrum.so")
    subprocess.run(["g++", "-std=c++17", "-O2", "-shared", "-fPIC", os.path.join(ROOT, "tests", "host_spectrum", "host_spectrum.cpp"), "-o", out], check=True)
    lib = ctypes.CDLL(out)
    lib.host_spectrum_eval.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_double, ctypes.c_void_p, ctypes.c_void_p]
    return lib


def host_records(lib, H, eps=pc.EPS):
    H = np.ascontiguousarray(H, dtype=np.float64)
    ne, n, _ = H.shape
    rec, spec = np.full((ne, 10), np.nan), np.full((ne, n), np.nan)
    assert lib.host_spectrum_eval(n // 3, H.ctypes.data, ne, eps, rec.ctypes.data, spec.ctypes.data) == 0
    return rec, spec


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


@pytest.mark.parametrize("nb", pc.NBS)
def test_host_function_against_exact_spectra(host_lib, nb):
    for family in pc.FAMILIES:
        ex = pc.exact(family, nb)
        assert len(ex.H) == pc.n_elem_default(nb)
        rec, spec = host_records(host_lib, ex.H)
        b = sp.bound(sp.rounding(family, nb), ex.fro, 0.0)
        sp.check_records("NB=%d %-18s" % (nb, family), rec, spec, ex.lam, b)
        # fields 5 and 6 from the stored entries
        assert np.abs(rec[:, 5] - ex.fro).max() <= 4 * 2.0 ** -52 * 3 * nb * ex.fro.max()
        tr = np.einsum("eii->e", ex.H)
        assert (np.abs(rec[:, 6] - tr) <= 4 * 2.0 ** -52 * 3 * nb * np.abs(np.einsum("eii->ei", ex.H)).sum(axis=1)).all()
        # field 8 is a certificate: the sorted eigenvalues are within it of the exact ones, up to the rounding term (Weyl)
        err = np.abs(spec - np.sort(ex.lam, axis=1)).max(axis=1)
        assert (err <= rec[:, 8] + sp.rounding(family, nb) * ex.fro).all(), family
        # ... and no smaller than the off-norm the restatement of the same iteration ends with, up to the same rounding
        _, _, A = sp.restatement(ex.H)
        off = np.sqrt(((A * A) * ~np.eye(3 * nb, dtype=bool)).sum(axis=(1, 2)))
        assert (rec[:, 8] >= off - sp.rounding(family, nb) * ex.fro).all(), family


@pytest.mark.parametrize("nb", pc.NBS)
def test_diagonal_families_to_the_bit(host_lib, nb):
    n = 3 * nb
    for family in pc.DIAG:
        d, o = pc.diag_inputs(family, nb, pc.n_elem_default(nb))
        ex = pc.exact(family, nb)
        rec, spec = host_records(host_lib, ex.H)
        plain = (o == 0).all(axis=1)
        assert plain.any() or family in ("s2_big", "tiny_off")
        assert (_bits(spec[plain]) == _bits(sp.sort_by_rank(d[plain]))).all(), family
        assert (rec[plain, 7] == 0).all() and (rec[plain, 8] == 0).all()
        if family == "at_eps":
            assert plain.all() and (rec[:, 2] == 0).all() and (rec[:, 9] == 0).all()
        elif family == "below_eps":
            assert plain.all()
            assert (rec[:, 2] == (d == pc.EPS_BELOW).sum(axis=1)).all() and (rec[:, 2] > 0).any()
            assert (rec[:, 9] == (rec[:, 2] > 0)).all()
        elif family == "zeros_denormal":
            assert plain.all()
            even = np.arange(len(d)) % 2 == 0
            assert (rec[even, 2] == 3).all() and (rec[even, 3] == 1).all() and (rec[~even, 2] == 0).all() and (rec[~even, 3] == 0).all()
    # a matrix of nothing but zeros and the denormal: every eigenvalue is below eps, only -5e-324 is negative
    H = np.zeros((1, n, n))
    H[0, n - 1, n - 1] = pc.DENORMAL
    rec, spec = host_records(host_lib, H)
    assert rec[0, 2] == n and rec[0, 3] == 1 and rec[0, 9] == 1
    assert _bits(spec[0, 0]) == _bits(np.float64(pc.DENORMAL))


@pytest.mark.parametrize("nb", [1, 4, 8])
def test_non_finite_entries_give_flag_two_and_zero_fields(host_lib, nb):
    ex = pc.exact("mixed", nb)
    H = ex.H[:3].copy()
    H[0, 0, 3 * nb - 1] = np.nan
    H[1, 3 * nb - 1, 1 % (3 * nb)] = np.inf
    rec, spec = host_records(host_lib, H)
    ref, rspec, _ = sp.restatement(H)
    for r, s in ((rec, spec), (ref, rspec)):
        assert (r[:2, 9] == 2).all() and (r[:2, :9] == 0).all() and (s[:2] == 0).all()
        assert r[2, 9] in (0, 1) and np.isfinite(r[2]).all()
    good, _ = host_records(host_lib, ex.H[2:3])
    assert (_bits(good[0]) == _bits(rec[2])).all()


@pytest.mark.parametrize("nb", pc.NBS)
def test_restatement_agrees_with_the_host_function(host_lib, nb):
    for family in pc.FAMILIES:
        ex = pc.exact(family, nb)
        rec, spec = host_records(host_lib, ex.H)
        ref, rspec, _ = sp.restatement(ex.H)
        tol = sp.rounding(family, nb) / 8 * ex.fro
        err = np.abs(spec - rspec).max(axis=1)
        print("NB=%d %-18s restatement - host %.3g of %.3g" % (nb, family, (err - tol).max() + tol.max(), tol.max()))
        assert (err <= tol).all(), family
        assert (ref[:, 9] == rec[:, 9]).all(), family        # (every family's decision is either exact or margins away from rounding: psd_cases.margins_hold)
        assert (np.abs(ref[:, 4] - rec[:, 4]) <= np.sqrt(3 * nb) * tol).all(), family
        assert (np.abs(ref[:, 5] - rec[:, 5]) <= 4 * 2.0 ** -52 * ex.fro).all() and (np.abs(ref[:, 7] - rec[:, 7]) <= 1).all(), family


def test_committed_tolerances_are_a_fresh_measurement():
    import json

    with open(sp.TOLERANCES) as f:
        committed = json.load(f)
    fresh = sp.measure_tolerances()
    assert committed == json.loads(json.dumps(fresh)), "tests/spectrum_tolerances.json is stale: regenerate it with spectrum_ref.write_tolerances()"
    for fam in pc.FAMILIES:
        for nb in pc.NBS:
            assert committed[fam][str(nb)] >= sp.floor(nb)


def test_dry_context_refuses_all_three_entry_points():
    import ctypes as C

    from stark_amd import capi

    L = capi.lib()
    h = C.c_void_p()
    assert L.mistark_create_dry(C.byref(h)) == 0
    try:
        u = np.zeros(6)
        assert L.mistark_add_dof_set(h, b"u", u.ctypes.data, u.size) >= 0
        n, nb = C.c_int64(), C.c_int32()
        out = np.zeros(32)
        ids = np.zeros(1, dtype=np.int32)
        for source in (0, 1):
            for call in (lambda: L.mistark_nodal_spectrum(h, ids.ctypes.data, 0, source, 1e-10, out.ctypes.data),
                         lambda: L.mistark_spectrum_potential_report(h, ids.ctypes.data, 0, source, 1e-10, out.ctypes.data)):
                assert call() < 0
                msg = L.mistark_last_error(h).decode()
                assert msg and "registration-only" in msg, msg
        assert L.mistark_potential_spectrum_report(h, 0, 0, 1e-10, None, None, C.byref(n), C.byref(nb)) < 0
        assert "bad potential id" in L.mistark_last_error(h).decode()
        assert L.mistark_nodal_spectrum(h, ids.ctypes.data, 0, 2, 1e-10, out.ctypes.data) < 0
        assert "source" in L.mistark_last_error(h).decode()
    finally:
        L.mistark_destroy(h)


def test_header_declares_and_python_binds_the_new_entry_points():
    from stark_amd import capi
    from stark_amd.engine import Engine

    names = capi.exported_symbols()
    L = capi.lib()
    for s in ("mistark_potential_spectrum_report", "mistark_nodal_spectrum", "mistark_spectrum_potential_report"):
        assert s in names and hasattr(L, s)
    for m in ("spectrum_report", "nodal_spectrum", "spectrum_potential_report"):
        assert callable(getattr(Engine, m))
