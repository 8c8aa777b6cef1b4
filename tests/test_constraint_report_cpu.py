"""Constraint report without a GPU: the per-row arithmetic of stark_amd/csrc/constraint_report.hpp compiled with g++
(tests/host_constraint_report/host_constraint_report.cpp, test-only) against the numpy restatement of tests/constraint_report_ref.py on the seeded
problems of all seventeen kinds, both against the oracle's energies and gradients, and the two families of the group sums in numpy.

Tolerances (tests/constraint_report_ref.py): 1e-11 relative to max |reference| of a field over the table for row quantities (+ 4 * 2^-53 / c rad on the
angle of an angle limit), (n + 8) * 2^-53 * sum |terms| for sums; the exact family uses ==."""
import ctypes
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import constraint_report_ref as cr  # noqa: E402
from oracle import evaluator as ev  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")


@pytest.fixture(scope="module")
def host_lib():
    out = os.path.join(tempfile.mkdtemp(prefix="mistark_host_constraint_report_"), "host_constraint_report.so")
    subprocess.run(["g++", "-std=c++17", "-O2", "-shared", "-fPIC", os.path.join(ROOT, "tests", "host_constraint_report", "host_constraint_report.cpp"), "-o", out], check=True)
    lib = ctypes.CDLL(out)
    p = ctypes.c_void_p
    lib.host_constraint_kind.argtypes = [ctypes.c_int, p, p, ctypes.c_int]
    lib.host_constraint_rows.argtypes = [ctypes.c_int, p, ctypes.c_int, p, p, p]
    return lib


def host_rows(lib, name, inp, tol=None):
    inp = np.ascontiguousarray(inp, dtype=np.float64)
    rec, aux = np.full((len(inp), 16), np.nan), np.full((len(inp), 2), np.nan)
    tol = None if tol is None else np.ascontiguousarray(tol, dtype=np.float64)
    assert lib.host_constraint_rows(cr.KINDS[name][0], inp.ctypes.data, len(inp), None if tol is None else tol.ctypes.data, rec.ctypes.data, aux.ctypes.data) == 0
    return rec, aux


def test_kind_table_of_the_header(host_lib):
    """Kind codes in registry order, group columns, side blocks, direction type and units as the restatement has them; the gathered width of the seeded
    problems is the layout's."""
    units = {0: "m", 1: "deg", 2: "m/s", 3: "deg/s"}
    for code, name in enumerate(cr.NAMES):
        info, buf = (ctypes.c_int * 6)(), ctypes.create_string_buffer(64)
        assert host_lib.host_constraint_kind(code, info, buf, 64) == 0
        assert buf.value.decode() == name
        want = cr.KINDS[name]
        assert (info[1], info[2], info[3], bool(info[4]), units[info[5]]) == (want[1], want[2], want[3], want[4], want[5]), name
        assert cr.gather(cr.seeded_problem(name)[0]).shape == (cr.N_ROWS, info[0]), name
    assert host_lib.host_constraint_kind(17, (ctypes.c_int * 6)(), ctypes.create_string_buffer(64), 64) < 0


def row_tolerances(name):
    prob, tol = cr.seeded_problem(name)
    return tol[prob.potentials[0].conn[:, cr.KINDS[name][1]]]


@pytest.mark.parametrize("name", cr.NAMES)
def test_host_build_against_restatement(host_lib, name):
    prob, _ = cr.seeded_problem(name)
    inp = cr.gather(prob)
    for tol in (None, row_tolerances(name)):
        rec, aux = host_rows(host_lib, name, inp, tol)
        want, want_aux = cr.row_records(name, inp, tol)
        bound = cr.row_bounds(name, inp, want)
        print("%s: worst |difference| / bound %.3g" % (name, float((np.abs(rec - want)[:, :15] / np.maximum(bound[:, :15], 1e-300)).max())))
        assert (np.abs(rec - want) <= bound).all(), np.argwhere(np.abs(rec - want) > bound)[:5]
        assert (np.abs(aux - want_aux) <= cr.ROW_TOL * np.abs(want_aux).max()).all()
    flags = rec[:, 15].astype(int)
    assert ((flags & 2) != 0).any() and ((flags & 2) == 0).any()       # rows on both sides of their tolerance
    assert ((host_rows(host_lib, name, inp)[0][:, 15].astype(int) & 2) == 0).all()   # never without a tolerance
    off = (flags & 1) == 0
    if off.any():   # inactive rows: geometry only
        assert (rec[off][:, 1:8] == 0.0).all() and (rec[off][:, 14] == 0.0).all() and np.abs(rec[off][:, 8:14]).max() > 0.0
    if name == "rb_constraint_damped_spring":
        assert np.abs(aux).min() > 0.0
    else:
        assert (aux == 0.0).all()


@pytest.mark.parametrize("name", cr.NAMES)
def test_energy_and_force_against_the_oracle(host_lib, name):
    """Slot 14 against the oracle's element energies row by row; slots 2..4 against minus the oracle's gradient summed over side a's translational
    blocks, scaled 1 / dt (the DoFs are velocities: dE/dv1 = dt dE/dx); side b's blocks sum to the negative for two-sided kinds."""
    prob, _ = cr.seeded_problem(name)
    pot = prob.potentials[0]
    rec, _ = host_rows(host_lib, name, cr.gather(prob))
    o = ev.evaluate_potential(prob, pot)
    E, g = np.zeros(cr.N_ROWS), np.zeros((cr.N_ROWS, o.g.shape[1]))
    E[o.active], g[o.active] = o.E, o.g
    assert (np.abs(rec[:, 14] - E) <= cr.ROW_TOL * np.abs(E).max()).all()
    assert (rec[~o.active, 14] == 0.0).all()
    blocks_a, blocks_b = cr.KINDS[name][6], cr.KINDS[name][7]
    f_a = -sum((g[:, 3 * k:3 * k + 3] for k in blocks_a), np.zeros((cr.N_ROWS, 3))) / prob.dt
    tol = cr.ROW_TOL * max(np.abs(f_a).max(), np.abs(rec[:, 2:5]).max())
    assert (np.abs(rec[:, 2:5] - f_a) <= tol).all()
    if not blocks_a:
        assert (rec[:, 2:5] == 0.0).all()
    else:
        assert np.abs(f_a).max() > 0.0
    if blocks_b:
        f_b = -sum((g[:, 3 * k:3 * k + 3] for k in blocks_b), np.zeros((cr.N_ROWS, 3))) / prob.dt
        assert (np.abs(rec[:, 2:5] + f_b) <= tol).all()


def test_torque_of_rigid_point_rows_against_the_oracle(host_lib):
    """A rigid side a of a point-type row: slots 5..7 against minus the oracle's gradient by w1 of body a, scaled 1 / dt, to first order in |w1| dt —
    checked on a copy of the seeded problem whose bodies do not rotate (w1 = 0: dE/dw1 = dt dE/dtheta exactly up to the normalisation's second order)."""
    for name in ("rb_constraint_points", "rb_constraint_global_points", "rb_constraint_distances"):
        prob, _ = cr.seeded_problem(name)
        pot = prob.potentials[0]
        arrays = [a.copy() for a in prob.arrays]
        w_arr = prob.dof_arrays[max(prob.dof_arrays)]
        arrays[w_arr][:] = 0.0
        still = ev.Problem(dt=prob.dt, ndofs=prob.ndofs, dof_offsets=prob.dof_offsets, dof_sizes=prob.dof_sizes, arrays=arrays, potentials=prob.potentials,
                           dof_arrays=prob.dof_arrays)
        rec, _ = host_rows(host_lib, name, cr.gather(still))
        o = ev.evaluate_potential(still, pot)
        g = np.zeros((cr.N_ROWS, o.g.shape[1]))
        g[o.active] = o.g
        k_w = 1 if name == "rb_constraint_global_points" else 2   # local block of w1_a
        tau = -g[:, 3 * k_w:3 * k_w + 3] / still.dt
        assert np.abs(tau).max() > 0.0
        assert (np.abs(rec[:, 5:8] - tau) <= 1e-9 * np.abs(tau).max()).all()


GROUP_TABLES = {"small": [1, 255, 256, 0, 257, 1023, 1024, 1025], "single": [1]}


def _table(sizes, seed):
    group = np.concatenate([np.full(s, g, dtype=np.int32) for g, s in enumerate(sizes)])
    np.random.default_rng(seed).shuffle(group)
    return group


@pytest.mark.parametrize("table", sorted(GROUP_TABLES))
def test_group_sums_exact_family(host_lib, table):
    """Dyadic inputs: the host build's records are the restatement's bit for bit, and every group sum is exact in any order."""
    sizes = GROUP_TABLES[table]
    group = _table(sizes, 3)
    n, ng = len(group), len(sizes)
    rng = np.random.default_rng(31)
    fam = cr.dyadic_point_springs(rng, group)
    about = np.array([0.25, -0.5, 0.125])
    x1 = fam["x0a"] + fam["dt"] * fam["v1a"]
    prob = cr.prescribed_problem(fam["x0a"], fam["v1a"], np.arange(n), x1 + fam["d"], np.resize(fam["k"], ng), group, fam["dt"])
    inp = cr.gather(prob)
    want, _ = cr.row_records("EnergyPrescribedPositions", inp)
    rec, _ = host_rows(host_lib, "EnergyPrescribedPositions", inp)
    assert np.array_equal(rec, want)
    assert np.array_equal(want[:, 0] * 64.0, np.rint(want[:, 0] * 64.0))   # |d| is exact
    cr.assert_exact_family(want, group, ng, about)
    grec, _ = cr.group_records(want, group, ng, about, False)
    for g in range(ng):   # another order, another tree: the same bits
        sel = np.flatnonzero(group == g)[::-1]
        terms = cr.group_terms(want[sel], about, False)
        assert [float(np.sum(t)) for t in terms] == list(grec[g, 5:12])
        assert grec[g, 0] == sizes[g] and grec[g, 4] == (-1 if sizes[g] == 0 else np.argmax(np.abs(want[group == g, 0])))


def test_group_sums_rounding_family():
    """Seeded problems: a plain running sum in list order against fsum within (n + 8) 2^-53 sum |terms|."""
    for name in ("EnergyPrescribedPositions", "EnergyAttachments_d_d_p_p", "rb_constraint_directions"):
        prob, tol = cr.seeded_problem(name)
        group = prob.potentials[0].conn[:, cr.KINDS[name][1]]
        rec, _ = cr.row_records(name, cr.gather(prob), tol[group])
        about = np.array([0.3, -0.2, 0.7])
        dir_type = cr.KINDS[name][4]
        grec, mag = cr.group_records(rec, group, len(tol), about, dir_type)
        for g in range(len(tol)):
            sel = group == g
            terms = cr.group_terms(rec[sel], about, dir_type)
            for k, t in enumerate(terms):
                s = 0.0
                for row in t:
                    s += float(row.sum())
                assert abs(s - grec[g, 5 + k]) <= (int(sel.sum()) + 8) * cr.U * mag[g, 5 + k]
        assert grec[:, 0].sum() == cr.N_ROWS and 0 < grec[:, 2].sum() < cr.N_ROWS


def test_fixtures_hold_all_seventeen_kinds():
    names = set()
    for fx in ("rbchain.npz", "attachzoo.npz"):
        prob, man, z = ev.load_fixture(os.path.join(GOLDEN, fx))
        names |= {p.name for p in prob.potentials if len(p.conn) > 0}
    assert set(cr.NAMES) <= names, sorted(set(cr.NAMES) - names)
