"""Bending report without a GPU: the two derivations of tests/bending_ref.py against each other, the per-hinge header
stark_amd/csrc/bending_report.hpp compiled with g++ (tests/host_bending_report/host_bending_report.cpp, test-only) against the restatement, closed forms,
and the refusals that need no device.

Tolerances: bending_ref's docstring. In short 1e-11 relative to the largest reference value of a field over the potential; theta1 within
1e-11 + 16 * 2.2e-16 / sin(theta_ref) per hinge, and what is computed from theta1 within that bound carried linearly through its formula."""
import ctypes
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import bending_ref as br  # noqa: E402
import stress_ref as sr  # noqa: E402

TOL = br.ELEMENT_TOL
THRESHOLDS = (0.05, 0.7, 1e9)   # per group; the third group is declared and empty


@pytest.fixture(scope="module")
def host_lib():
    out = os.path.join(tempfile.mkdtemp(prefix="mistark_host_bending_"), "host_bending_report.so")
    subprocess.run(["g++", "-std=c++17", "-O2", "-shared", "-fPIC", os.path.join(ROOT, "tests", "host_bending_report", "host_bending_report.cpp"), "-o", out], check=True)
    lib = ctypes.CDLL(out)
    lib.host_bending_eval.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    return lib


def host_records(lib, prob, pot, threshold=None):
    inp = sr.gathered_flat(prob, pot)
    group = np.ascontiguousarray(br.groups_of(pot), dtype=np.int32)
    thr = None if threshold is None else np.ascontiguousarray(np.asarray(threshold, dtype=np.float64)[group])
    rec = np.full((len(inp), 16), np.nan)
    assert lib.host_bending_eval(br.KIND[pot.name], inp.ctypes.data, inp.shape[1], len(inp), None if thr is None else thr.ctypes.data, group.ctypes.data, rec.ctypes.data) == 0
    return rec


def _cases(name):
    prob, rec, bound, extra = br.seeded_hinges(name)
    gprob, gpot, grec, gbound = br.golden_problem(name)
    return [("seeded " + name, prob, prob.potentials[0], rec, bound, True), ("golden " + name, gprob, gpot, grec, gbound, False)]


@pytest.mark.parametrize("name", br.NAMES)
def test_records_equal_the_oracle_derived_energy_and_moment(host_lib, name):
    """(A) against (B), and the host build of the header against (B) as well."""
    for what, prob, pot, rec, bound, rigid in _cases(name):
        assert len(rec) >= 96 and not (rec[:, 15].astype(int) & 1).any()
        E, M, mb = br.from_oracle(prob, pot)
        for who, r in (("(A)", rec), ("host build", host_records(host_lib, prob, pot))):
            err = np.abs(r[:, 9] + r[:, 10] - E)
            print("%s: fields 9 + 10 of %s against the oracle's element energies: rel %.3g, worst error / bound %.3g"
                  % (what, who, err.max() / np.abs(E).max(), (err / (bound[:, 9] + bound[:, 10])).max()))
            assert (err <= bound[:, 9] + bound[:, 10]).all()        # (both fields carry theta1's bound: the oracle's acos is another evaluation of it)
            if br.KIND[name] == 1 and not rigid:
                continue    # (the flat moment is dE/dtheta on a rigid fold of the rest stencil only: bending_ref's docstring)
            said = np.isfinite(mb)
            assert said.sum() >= len(rec) // 3, (what, said.sum())
            d = np.abs(r[said, 8] - M[said])
            both = bound[said, 8] + mb[said] * np.abs(rec[:, 8]).max()     # the record's own bound (theta1's, carried through the moment) and (B)'s
            print("%s: moment of %s against (B) on %d hinges: worst error / bound %.3g" % (what, who, said.sum(), (d / both).max()))
            assert (d <= both).all()


@pytest.mark.parametrize("name", br.NAMES)
def test_host_build_equals_restatement(host_lib, name):
    for what, prob, pot, rec, bound, rigid in _cases(name):
        br.check_records(host_records(host_lib, prob, pot), rec, bound, what)


@pytest.mark.parametrize("name", br.NAMES)
def test_thresholds_flag_the_sharp_hinges(host_lib, name):
    """Flag 2 of the host build against the restatement; the thresholds leave the restatement itself undecided on at most 2 % of the rows."""
    prob, rec0, bound0, extra = br.seeded_hinges(name)
    pot = prob.potentials[0]
    rec, bound = br.records(prob, pot, THRESHOLDS)
    out = br.undecided(rec, bound, THRESHOLDS)
    flagged = (rec[:, 15].astype(int) & 2) != 0
    print("%s: %d of %d rows beyond threshold, %d undecided" % (name, flagged.sum(), len(rec), out.sum()))
    assert out.sum() <= 0.02 * len(rec)
    assert flagged.any() and not flagged.all()
    assert np.array_equal(rec[:, :15], rec0[:, :15])     # thresholds change the flags alone
    br.check_records(host_records(host_lib, prob, pot, THRESHOLDS), rec, bound, name, THRESHOLDS)
    grp, _ = br.group_records(rec, 3)
    assert grp[:, 0].sum() == len(rec) and grp[2, 0] == 0 and grp[2, 4] == -1.0
    assert grp[0, 2] == (flagged & (rec[:, 14] == 0)).sum() and grp[1, 2] == (flagged & (rec[:, 14] == 1)).sum()


def test_the_complete_angle_is_blind_to_direction_and_never_below_its_floor(host_lib):
    prob, rec, bound, extra = br.seeded_hinges("EnergyDiscreteShells")
    rec = host_records(host_lib, prob, prob.potentials[0])
    assert (rec[:, 0] >= 1.41e-6).all() and (rec[:, 0] <= np.pi).all()
    flat = np.abs(extra["angle"]) <= 1e-9
    assert flat.any() and np.abs(rec[flat, 0] - np.sqrt(2e-12)).max() < 1e-9
    big = np.abs(extra["angle"]) >= 0.1
    assert np.abs(rec[big, 0] - np.abs(extra["angle"][big])).max() < 1e-5     # (the 1 - 1e-12 factor moves an angle near pi by 1.4e-6)
    inner = big & (np.abs(extra["angle"]) < np.pi)
    assert np.array_equal(np.sign(rec[inner, 1]), np.sign(extra["angle"][inner]))
    assert np.abs(rec[inner, 1] - extra["angle"][inner]).max() < 1e-13


@pytest.mark.parametrize("name", br.NAMES)
def test_a_mirrored_fold_flips_the_sign_of_phi_and_nothing_else(host_lib, name):
    """The mirror image of a fold has the same angle, curvature, moment and energy; only phi1 changes sign. (The hinge normal is a direction in space and
    turns with the mirror: it is not compared.)"""
    prob, rec, bound, extra = br.seeded_hinges(name)
    got = host_records(host_lib, prob, prob.potentials[0])
    m = extra["mirror_of"]
    for r in (rec, got):
        inner = (np.abs(extra["angle"]) >= 1e-5) & (np.abs(extra["angle"]) < np.pi)
        assert np.array_equal(np.sign(r[inner, 1]), -np.sign(r[m[inner], 1]))
        d = np.abs(r[:, 1] + r[m, 1])
        assert np.minimum(d, 2.0 * np.pi - d).max() <= 2.0 * bound[:, 1].max()
        for f in (0, 2, 3, 4, 5, 6, 7, 8, 9, 10, 14, 15):
            assert (np.abs(r[:, f] - r[m, f]) <= bound[:, f] + bound[m, f]).all(), (name, f)


def test_rigid_fold_closed_forms_and_the_flat_models_factor_four(host_lib):
    """|s| = 2 l sin(theta / 2) and M_flat = k l sin(theta) / (2 h_e) on a rigid fold; against the complete model with the same stiffness, no damping and
    a flat rest state, M_complete / M_flat = 4 theta / sin(theta)."""
    prob, rec, bound, extra = br.seeded_hinges("EnergyBendingFlat")
    rec = host_records(host_lib, prob, prob.potentials[0])
    th = np.abs(extra["angle"])
    l, he, k = extra["l"], (extra["h1"] + extra["h2"]) / 6.0, extra["k"]
    a = l * he                                      # (A0 + A1) / 3
    assert np.abs(rec[:, 5] - a).max() <= TOL * a.max()
    s_norm = rec[:, 6] * 3.0 * rec[:, 5]
    assert np.abs(s_norm - 2.0 * l * np.sin(0.5 * th)).max() <= TOL * (2.0 * l).max() + 8 * br.EPS * 4.0   # (s cancels from terms |K| |x| of size 4)
    sel = (th >= 1e-5) & (th < np.pi)               # (at 0 and pi the 1 - 1e-12 factor of theta1 is all there is of cos(theta1 / 2))
    M = k * l * np.sin(th) / (2.0 * he)
    err = np.abs(rec[sel, 8] - M[sel]).max() / np.abs(M).max()
    print("flat: M against k l sin(theta) / (2 h_e): rel %.3g" % err)
    assert err < TOL
    M_complete = 2.0 * k * th * l / he
    ratio = M_complete[sel] / rec[sel, 8]
    assert np.abs(ratio / (4.0 * th[sel] / np.sin(th[sel])) - 1.0).max() < 1e-9
    small = th == 1e-5
    assert np.abs(ratio[small[sel]] - 4.0).max() < 1e-6


def test_the_complete_moment_of_a_flat_rest_hinge_is_two_k_theta_l_over_h(host_lib):
    rng = np.random.default_rng(5)
    n = 40
    l, h1, h2 = rng.uniform(0.05, 0.3, n), rng.uniform(0.03, 0.2, n), rng.uniform(0.03, 0.2, n)
    th = rng.uniform(0.1, 3.0, n)
    x1 = br.fold(l, h1, h2, 0.4 * l, 0.7 * l, th)
    hinges = np.arange(4 * n).reshape(n, 4)
    rest = br.hinge_rest_data(br.fold(l, h1, h2, 0.4 * l, 0.7 * l, np.zeros(n)).reshape(-1, 3), hinges)
    k = 3e-3
    prob = br.make_problem([("EnergyDiscreteShells", hinges, np.zeros(n, dtype=int), rest, dict(scale=[1.0], k=[k], damping=[0.0]))], x1.reshape(-1, 3), np.zeros((4 * n, 3)))
    for rec in (br.records(prob, prob.potentials[0])[0], host_records(host_lib, prob, prob.potentials[0])):
        M = 2.0 * k * (rec[:, 0] - rest["rest_angle"]) * l / ((h1 + h2) / 6.0)
        assert np.abs(rec[:, 8] - M).max() <= TOL * np.abs(M).max()
        assert np.abs(rec[:, 0] - th).max() < 1e-10


@pytest.mark.parametrize("R", [0.5, 2.0, 50.0])
def test_a_strip_inscribed_in_a_cylinder(host_lib, R):
    """Hinges parallel to the axis, facet heights h1 and h2 (chords): theta = asin(h1 / 2R) + asin(h2 / 2R), complete kappa = 2 theta / (h1 + h2), flat
    kappa = 4 sin(theta / 2) / (h1 + h2); both tend to 1 / R."""
    rng = np.random.default_rng(11)
    n = 24
    h1, h2, L = rng.uniform(0.01, 0.08, n), rng.uniform(0.01, 0.08, n), rng.uniform(0.05, 0.2, n)
    z2, z3 = L * rng.uniform(0.0, 1.0, n), L * rng.uniform(0.0, 1.0, n)
    a1, a2 = 2.0 * np.arcsin(h1 / (2.0 * R)), 2.0 * np.arcsin(h2 / (2.0 * R))
    zero = np.zeros(n)
    x1 = np.stack([np.stack([R + zero, zero, zero], axis=1), np.stack([R + zero, zero, L], axis=1), np.stack([R * np.cos(a1), R * np.sin(a1), z2], axis=1),
                   np.stack([R * np.cos(a2), -R * np.sin(a2), z3], axis=1)], axis=1)
    theta = np.arcsin(h1 / (2.0 * R)) + np.arcsin(h2 / (2.0 * R))
    hinges = np.arange(4 * n).reshape(n, 4)
    rest = br.hinge_rest_data(br.fold(L, h1, h2, z2, z3, zero).reshape(-1, 3), hinges)
    want = {"EnergyDiscreteShells": 2.0 * theta / (h1 + h2), "EnergyBendingFlat": 4.0 * np.sin(0.5 * theta) / (h1 + h2)}
    for name in br.NAMES:
        gp = dict(scale=[1.0], k=[1e-3], damping=[0.0]) if br.KIND[name] == 0 else dict(k=[1e-3])
        prob = br.make_problem([(name, hinges, np.zeros(n, dtype=int), rest, gp)], x1.reshape(-1, 3), np.zeros((4 * n, 3)))
        for rec in (br.records(prob, prob.potentials[0])[0], host_records(host_lib, prob, prob.potentials[0])):
            # theta1 within its own bound (the chords make theta about (h1 + h2) / 2R: sin(theta) is small for the large radius), kappa through it
            tb = br.theta_bound(theta) + np.abs(np.sqrt(theta ** 2 + 2e-12) - theta)      # (the 1 - 1e-12 factor: theta1^2 = theta^2 + 2e-12 to first order)
            if br.KIND[name] == 0:
                assert (np.abs(rec[:, 0] - theta) <= 1.01 * tb).all()
                assert (np.abs(rec[:, 6] - want[name]) <= 2.0 * 1.01 * tb / (h1 + h2) + TOL * want[name].max()).all()
            else:
                assert np.abs(rec[:, 6] - want[name]).max() <= TOL * want[name].max() + 8 * br.EPS * 4.0 * R / ((h1 + h2).min() * L.min() / 2.0)
            hmax = max(h1.max(), h2.max())
            # asin(x) = x (1 + x^2 / 6 + ...), x = h / 2R; the complete kind's theta1^2 = theta^2 + 2e-12 shows once theta is small: relative 1e-12 / theta^2
            floor = (1.5e-12 / theta ** 2).max() if br.KIND[name] == 0 else 0.0
            assert np.abs(rec[:, 6] * R - 1.0).max() <= (hmax / R) ** 2 + floor + 1e-8
            assert np.abs(rec[:, 1]).max() > 0.0 and (np.sign(rec[:, 1]) == np.sign(rec[0, 1])).all()


@pytest.mark.parametrize("name", br.NAMES)
def test_collapsed_triangles_are_flagged_not_trapped(host_lib, name):
    """Node 2 on node 0 (a triangle of zero area), and a hinge of zero length: flag 1, zeros where the record needs a normal, nothing that is not finite."""
    prob0, rec0, bound0, extra = br.seeded_hinges(name)
    pot0 = prob0.potentials[0]
    x0, v1 = prob0.arrays[1].copy(), prob0.arrays[0].copy()
    c = pot0.conn
    x0[c[1, 4]], v1[c[1, 4]] = x0[c[1, 2]], v1[c[1, 2]]          # hinge 1: node 2 = node 0 at both states
    x0[c[2, 3]], v1[c[2, 3]] = x0[c[2, 2]], v1[c[2, 2]]          # hinge 2: zero length
    v1[c[3, 5]] = (x0[c[3, 3]] - x0[c[3, 5]]) / br.DT + v1[c[3, 3]]   # hinge 3: node 3 arrives on node 1 at x1 only
    arrays = [v1, x0] + [a.copy() for a in prob0.arrays[2:]]
    prob = br.ev.Problem(dt=prob0.dt, ndofs=prob0.ndofs, dof_offsets=prob0.dof_offsets, dof_sizes=prob0.dof_sizes, arrays=arrays, potentials=prob0.potentials, dof_arrays=prob0.dof_arrays)
    rec, bound = br.records(prob, pot0, THRESHOLDS)
    got = host_records(host_lib, prob, pot0, THRESHOLDS)
    zero = [0, 1, 3, 8, 11, 12, 13] + ([6, 9, 10] if br.KIND[name] == 0 else [])
    for r in (rec, got):
        assert np.isfinite(r).all()
        assert (r[1:4, 15] == 1.0).all(), r[1:4, 15]           # flag 1, never flag 2
        assert (r[1:4][:, zero] == 0.0).all()
        assert (r[0, 15] != 1.0) and (r[4:, 15].astype(int) & 1 == 0).all()
    assert got[2, 4] == 0.0 and got[1, 4] > 0.0
    br.check_records(got, rec, bound, name, THRESHOLDS)


def test_nodal_and_group_sums_of_the_host_rows_add_up(host_lib):
    """The numpy sums the GPU tests compare with, over the host build's rows: the nodal energy shares and the group energies both add up to the rows'
    energy, and that to the oracle's."""
    for name in br.NAMES:
        prob, hinges = br.cloth(name, 6, small_group=10)
        pot = prob.potentials[0]
        rec = host_records(host_lib, prob, pot)
        E = (rec[:, 9] + rec[:, 10]).sum()
        nod, mag = br.nodal(len(prob.arrays[1]), [(br.block_rows(prob, pot), rec)])
        assert abs(nod[:, 2].sum() - E) <= 1e-12 * np.abs(rec[:, 9:11]).sum()
        assert nod[:, 4].sum() == 2 * len(rec) and abs(nod[:, 5].sum() - rec[:, 5].sum()) <= 1e-12 * rec[:, 5].sum()
        grp, _ = br.group_records(rec, 3)
        assert abs(grp[:, 5].sum() + grp[:, 6].sum() - E) <= 1e-12 * np.abs(rec[:, 9:11]).sum()
        assert grp[1, 0] == 10 and grp[2, 4] == -1.0 and grp[0, 3] == br.deviation(rec)[: len(rec) - 10].max()
        o = br.ev.evaluate_potential(prob, pot)
        assert abs(o.E.sum() - E) <= TOL * np.abs(o.E).sum()


def test_dry_context_refuses_all_three_entry_points():
    import ctypes as C

    from stark_amd import capi

    L = capi.lib()
    h = C.c_void_p()
    assert L.mistark_create_dry(C.byref(h)) == 0
    try:
        u = np.zeros(6)
        assert L.mistark_add_dof_set(h, b"u", u.ctypes.data, u.size) >= 0
        n, kind = C.c_int64(), C.c_int32()
        out = np.zeros(32)
        ids = np.zeros(1, dtype=np.int32)
        for call in (lambda: L.mistark_potential_bending_report(h, 0, None, 0, None, C.byref(n), C.byref(kind)),
                     lambda: L.mistark_nodal_bending(h, ids.ctypes.data, 1, out.ctypes.data),
                     lambda: L.mistark_bending_group_report(h, 0, None, 1, out.ctypes.data)):
            assert call() < 0
            msg = L.mistark_last_error(h).decode()
            assert msg and "registration-only" in msg, msg
    finally:
        L.mistark_destroy(h)


def test_header_declares_and_python_binds_the_new_entry_points():
    from stark_amd import capi

    names = capi.exported_symbols()
    for s in ("mistark_potential_bending_report", "mistark_nodal_bending", "mistark_bending_group_report"):
        assert s in names
