"""Contact report without a GPU: the numpy restatement of tests/contact_report_ref.py against the oracle (distances of oracle.contact.detect, element
energies and element forces of the barrier potentials), and the arithmetic header stark_amd/csrc/contact_report.hpp compiled with g++
(tests/host_contact_report/host_contact_report.cpp, test-only) against the restatement.

Tolerances: 64 * 2^-53 relative for one distance or one field (a fixed, small number of operations); the project's element tolerance 1e-11 for energies
against the oracle's potentials (of the table's largest |E|) and for forces (of fn); (n + 8) * 2^-53 * sum |terms| for a sum of n terms against
math.fsum of the same terms."""
import ctypes
import math
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import contact_report_ref as cr  # noqa: E402
import forces_ref as fr  # noqa: E402
from contact_util import state_from_fixture  # noqa: E402
from oracle import contact as oc  # noqa: E402
from oracle import evaluator as ev  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
FIXTURES = ["contactmix_t0", "contactmix_t1", "contactcorners_t0", "contactrods_t0", "contactrods_t1"]
ROWS = {"contactmix_t0": 297, "contactmix_t1": 18, "contactcorners_t0": 65, "contactrods_t0": 47, "contactrods_t1": 17}
U = cr.U
SRC = os.path.join(ROOT, "tests", "host_contact_report", "host_contact_report.cpp")


case = cr.fixture_case


def fixture_rows(c, table):
    """(potential, {connectivity row: element index}) of a barrier table in the fixture."""
    name = cr.TABLE_NAMES[table]
    for pot in c["prob"].potentials:
        if pot.name == name:
            return pot, {tuple(int(v) for v in row): e for e, row in enumerate(pot.conn)}
    raise KeyError(name)


def test_fixture_coverage():
    filled, mollified = set(), {}
    for name in FIXTURES:
        c = case(name)
        assert len(c["keys"]) == ROWS[name], (name, len(c["keys"]))
        filled |= set(int(t) for t in c["ri"][:, 0])
        mollified[name] = c["ri"][(c["ri"][:, 7] & cr.MOLLIFIED) != 0, 0]
        # the key list is the fixture's tables, row for row
        for table in range(21):
            pot, index = fixture_rows(c, table)
            mine = [tuple(cr.table_row(c["scene"], key)) for key in c["keys"] if key[0] == table]
            assert sorted(mine) == sorted(tuple(int(v) for v in row) for row in pot.conn), (name, table)
    assert filled == set(range(21))
    assert {n: len(m) for n, m in mollified.items()} == {"contactmix_t0": 0, "contactmix_t1": 0, "contactcorners_t0": 7, "contactrods_t0": 0, "contactrods_t1": 0}
    assert (mollified["contactcorners_t0"] >= 6).all()  # rigid tables


@pytest.mark.parametrize("name", FIXTURES)
def test_distance_against_the_oracle(name):
    c = case(name)
    err = np.abs(c["rd"][:, 0] - c["d_detect"]) / c["d_detect"]
    print("%s: worst relative distance error %.3g (bound %.3g)" % (name, err.max(), 64 * U))
    assert (err <= 64 * U).all()
    assert (c["rd"][:, 0] < c["rd"][:, 1]).all() and not (c["ri"][:, 7] & (cr.OPEN | cr.DEGENERATE)).any()


@pytest.mark.parametrize("name", FIXTURES)
def test_energy_against_the_oracle(name):
    c = case(name)
    for table in range(21):
        sel = np.nonzero(c["ri"][:, 0] == table)[0]
        if len(sel) == 0:
            continue
        pot, index = fixture_rows(c, table)
        o = ev.evaluate_potential(c["prob"], pot)
        assert o.active.all()
        want = np.array([o.E[index[tuple(cr.table_row(c["scene"], c["keys"][n]))]] for n in sel])
        err = np.abs(c["rd"][sel, 13] - want).max() / np.abs(o.E).max()
        print("%s %s: %d rows, worst energy error %.3g of the largest |E|" % (name, pot.name, len(sel), err))
        assert err <= 1e-11


def test_force_identity_on_the_deformable_tables():
    """Non-mollified rows of the contact_d_d_* tables: the element forces are +w fn n on the nodes of a and -w fn n on the nodes of b. The four fixtures
    together fill all six families."""
    families = set()
    for name in ["contactmix_t0", "contactmix_t1", "contactrods_t0", "contactcorners_t0"]:
        families |= _force_identity(case(name), name)
    assert families == set(range(6))


def _force_identity(c, name):
    L = cr.Layout(c["scene"])
    contrib = cr.contributions(c["scene"], c["ri"], c["rd"])
    worst, n_checked, families = 0.0, 0, set()
    for table in range(6):
        sel = np.nonzero((c["ri"][:, 0] == table) & ((c["ri"][:, 7] & cr.MOLLIFIED) == 0))[0]
        if len(sel) == 0:
            continue
        families.add(table)
        pot, index = fixture_rows(c, table)
        r = fr.potential_forces(c["prob"], pot, 1.0 / c["dt"])
        v1_set = [b.dof_set for b in pot.bindings if b.dof_set >= 0][0]
        row0 = c["prob"].dof_offsets[v1_set] // 3
        for n in sel:
            e = index[tuple(cr.table_row(c["scene"], c["keys"][n]))]
            got = {}
            for blk in range(r["rows"].shape[1]):
                v = int(r["rows"][e, blk] - row0)
                got[v] = got.get(v, np.zeros(3)) + r["f"][e, blk]
            fn, nrm = c["rd"][n, 12], c["rd"][n, 8:11]
            want = {}
            for j, (cv, w) in enumerate(contrib[n]):
                a_side = j < (1 if c["ri"][n, 1] == 0 else 2)
                v = int(L.cv_src[cv])
                want[v] = want.get(v, np.zeros(3)) + (1.0 if a_side else -1.0) * w * fn * nrm
            for v in set(got) | set(want):
                worst = max(worst, np.abs(got.get(v, np.zeros(3)) - want.get(v, np.zeros(3))).max() / fn)
            n_checked += 1
    print("%s: %d rows, worst force deviation %.3g fn" % (name, n_checked, worst))
    assert worst <= 1e-11
    return families


@pytest.fixture(scope="module")
def host_lib():
    out = os.path.join(tempfile.mkdtemp(prefix="mistark_host_contact_report_"), "host_contact_report.so")
    subprocess.run(["g++", "-std=c++17", "-O2", "-shared", "-fPIC", SRC, "-o", out], check=True)
    lib = ctypes.CDLL(out)
    p = ctypes.c_void_p
    lib.host_contact_rows.argtypes = [p, p, p, ctypes.c_double, ctypes.c_int, p, p, p]
    lib.host_contact_triangle_area.argtypes = [p, p, p]
    lib.host_contact_triangle_area.restype = ctypes.c_double
    return lib


def gathered_inputs(c):
    """Per row what the header takes: keys [n, 7], positions [n, 9, 3] (xa0 xa1 xb0 xb1 xb2 ra0 ra1 rb0 rb1), thickness [n, 2]."""
    L = cr.Layout(c["scene"])
    n = len(c["keys"])
    keys = np.zeros((n, 7), dtype=np.int32)
    pos = np.zeros((n, 9, 3))
    thick = np.zeros((n, 2))
    for i, (table, src, ty, a, b) in enumerate(c["keys"]):
        ga, gb = int(c["ri"][i, 3]), int(c["ri"][i, 4])
        keys[i] = [table, src, ty, a, b, ga, gb]
        thick[i] = [L.thick[ga], L.thick[gb]]
        if src == 0:
            pos[i, 0] = pos[i, 1] = c["X"][a]
            pos[i, 2:5] = c["X"][L.tri[b]]
        else:
            pos[i, 0:2], pos[i, 2:4] = c["X"][L.edge[a]], c["X"][L.edge[b]]
            pos[i, 4] = pos[i, 3]
            pos[i, 5:7], pos[i, 7:9] = c["Xrest"][L.edge[a]], c["Xrest"][L.edge[b]]
    return keys, pos, thick


@pytest.mark.parametrize("name", FIXTURES)
def test_header_against_the_restatement(name, host_lib):
    c = case(name)
    keys, pos, thick = gathered_inputs(c)
    n = len(keys)
    ri, rd, w = np.zeros((n, 8), dtype=np.int32), np.zeros((n, 16)), np.zeros((n, 5))
    assert host_lib.host_contact_rows(keys.ctypes.data, pos.ctypes.data, thick.ctypes.data, c["k"], n, ri.ctypes.data, rd.ctypes.data, w.ctypes.data) == 0
    assert (ri == c["ri"]).all()
    err = np.abs(rd - c["rd"]) / cr.field_scales(c["rd"], np.abs(pos[:, :5]).max(axis=(1, 2)), c["k"])
    print("%s: worst field error %.3g (bound %.3g)" % (name, err.max(), 64 * U))
    assert (err <= 64 * U).all()
    for i in range(n):
        wa, wb = cr.weights(int(ri[i, 1]), int(ri[i, 2]), rd[i, 14], rd[i, 15])
        assert list(w[i]) == wa + wb  # the same operations on the same parameters: the same bits
    # exact zeros and ones where a vertex or edge feature does not use a node
    pt_vertex = (ri[:, 1] == 0) & (ri[:, 2] <= oc.P_T2)
    assert set(np.unique(w[pt_vertex, 2:])) <= {0.0, 1.0} and (w[pt_vertex, 2:].sum(axis=1) == 1.0).all()
    pt_edge = (ri[:, 1] == 0) & (ri[:, 2] >= oc.P_E0) & (ri[:, 2] <= oc.P_E2)
    assert ((w[pt_edge, 2:] == 0.0).sum(axis=1) >= 1).all()
    ee_vertex = (ri[:, 1] == 1) & (ri[:, 2] <= oc.EA1_EB1)
    assert set(np.unique(w[ee_vertex, :4])) <= {0.0, 1.0}


def test_header_flags_and_moved_state(host_lib):
    """Rows at a state other than the searched one: pulled past dhat (open), a point put on its partner (degenerate), flattened edges (mollified)."""
    c = case("contactcorners_t0")
    keys, pos, thick = gathered_inputs(c)
    pos = pos.copy()
    n = len(keys)
    pos[:, :2] += np.array([0.0, 0.0, 0.5])  # side a lifted by half a metre: every row open
    ri, rd, w = np.zeros((n, 8), dtype=np.int32), np.zeros((n, 16)), np.zeros((n, 5))
    host_lib.host_contact_rows(keys.ctypes.data, pos.ctypes.data, thick.ctypes.data, c["k"], n, ri.ctypes.data, rd.ctypes.data, w.ctypes.data)
    assert ((ri[:, 7] & cr.OPEN) != 0).all() and (rd[:, 0] >= rd[:, 1]).all()
    assert (ri[:, :7] == c["ri"][:, :7]).all()  # the pair is not classified again
    pp = np.nonzero((ri[:, 1] == 0) & (ri[:, 2] == oc.P_T0))[0]
    assert len(pp) > 0
    pos[pp[0], 0] = pos[pp[0], 2]
    host_lib.host_contact_rows(keys.ctypes.data, pos.ctypes.data, thick.ctypes.data, c["k"], n, ri.ctypes.data, rd.ctypes.data, w.ctypes.data)
    assert ri[pp[0], 7] & cr.DEGENERATE and rd[pp[0], 0] == 0.0 and (rd[pp[0], 8:11] == 0.0).all()
    # an edge-edge row whose edge b is laid nearly parallel to edge a: |u x v|^2 = 1e-6 |u|^4 against eps_x = 1e-3 |ra|^2 |rb|^2
    ee = np.nonzero((ri[:, 1] == 1) & ((c["ri"][:, 7] & cr.MOLLIFIED) == 0))[0]
    assert len(ee) > 0
    i = ee[0]
    u = pos[i, 1] - pos[i, 0]
    perp = np.cross(u, [1.0, 0.0, 0.0] if abs(u[0]) < 0.9 * np.linalg.norm(u) else [0.0, 1.0, 0.0])
    pos[i, 3] = pos[i, 2] + u + 1e-3 * np.linalg.norm(u) * perp / np.linalg.norm(perp)
    pos[i, 4] = pos[i, 3]
    host_lib.host_contact_rows(keys.ctypes.data, pos.ctypes.data, thick.ctypes.data, c["k"], n, ri.ctypes.data, rd.ctypes.data, w.ctypes.data)
    ra, rb = pos[i, 5] - pos[i, 6], pos[i, 7] - pos[i, 8]
    cx = np.cross(u, pos[i, 3] - pos[i, 2])
    r = (cx @ cx) / (1e-3 * (ra @ ra) * (rb @ rb))
    assert r < 1.0 and ri[i, 7] & cr.MOLLIFIED and 0.0 < rd[i, 11] < 1.0
    assert abs(rd[i, 11] - (2.0 - r) * r) <= 64 * U
    g = rd[i, 1] - rd[i, 0]
    assert abs(rd[i, 12] - rd[i, 11] * c["k"] * g * g) <= 64 * U * c["k"] * max(rd[i, 1], abs(g)) ** 2
    assert abs(rd[i, 13] - rd[i, 11] * c["k"] * g ** 3 / 3.0) <= 64 * U * c["k"] * max(rd[i, 1], abs(g)) ** 3


def test_sanitizer_run_of_the_header():
    """The same file as a stand-alone program (its own main, no Python in the process, no preload) under AddressSanitizer and UBSan."""
    exe = os.path.join(tempfile.mkdtemp(prefix="mistark_host_contact_report_"), "host_contact_report_asan")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-DHOST_CONTACT_REPORT_MAIN", SRC, "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout, r.stderr)
    assert r.returncode == 0 and "rows 297" in r.stdout and "ERROR" not in r.stderr and "runtime error" not in r.stderr


@pytest.mark.parametrize("name", FIXTURES)
def test_sums_against_fsum(name, host_lib):
    c = case(name)
    vert, vterms = cr.vertex_report(c["scene"], c["ri"], c["rd"], c["X"])
    for v, xs in enumerate(vterms):
        assert vert[v, 1] == len(xs)
        assert abs(vert[v, 2] - math.fsum(xs)) <= cr.sum_bound(xs)
    assert vert[:, 1].sum() == 4 * len(c["keys"])
    touched = vert[:, 1] > 0
    assert np.isinf(vert[~touched, 0]).all() and (vert[touched, 0] >= c["rd"][:, 0].min()).all()
    pairs, pterms = cr.pair_report(c["scene"], c["ri"], c["rd"])
    for (ga, gb), T in pterms.items():
        for f, xs in T.items():
            assert abs(pairs[ga, gb, f] - math.fsum(xs)) <= cr.sum_bound(xs)
    assert pairs[:, :, 0].sum() == len(c["keys"])
    assert abs(pairs[:, :, 3].sum() - c["rd"][:, 12].sum()) <= cr.sum_bound(list(c["rd"][:, 12]))
    # the weights of a side sum to one: the shares of all vertices add up to twice the sum of fn
    assert abs(vert[:, 2].sum() - 2.0 * c["rd"][:, 12].sum()) <= 64 * U * 4 * len(c["keys"]) * np.abs(c["rd"][:, 12]).max()
    # areas: a third of the triangles' areas per vertex, the header's triangle area against numpy
    L = cr.Layout(c["scene"])
    ta = cr.triangle_areas(c["scene"], c["X"])
    assert abs(vert[:, 3].sum() - ta.sum()) <= (L.n_t + 8) * 4 * U * ta.sum()
    for t in range(min(L.n_t, 16)):
        P = [np.ascontiguousarray(c["X"][v]) for v in L.tri[t]]
        assert abs(host_lib.host_contact_triangle_area(P[0].ctypes.data, P[1].ctypes.data, P[2].ctypes.data) - ta[t]) <= 64 * U * ta[t]
