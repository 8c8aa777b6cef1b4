"""Friction report without a GPU: the numpy restatement of tests/friction_report_ref.py against the oracle (element energies and element gradients of the
14 friction potentials), and the arithmetic header stark_amd/csrc/friction_report.hpp compiled with g++
(tests/host_friction_report/host_friction_report.cpp, test-only) against the restatement.

States: every fixture at its stored DoFs u (every friction row sticks there), at u + 0.1 r and at u + 0.2 r, r = default_rng(7).standard_normal in
Problem.get_dofs() order; the friction tables stay the fixture's (they are lagged). Over the three states every table has sticking and sliding rows, and no
row lies closer to the threshold than | |u| / epsu - 1 | = 0.013, so the sliding flag is compared with == on every row.

Tolerances: the project's element tolerance 1e-11 for energies (relative) and node forces (of mu fn) against the oracle; 64 * 2^-53 of the field's scale
for the header against the restatement, as tests/test_contact_report_cpu.py holds contact_report.hpp (friction_report_ref.field_scales says what a field is
measured against); (n + 8) * 2^-53 * sum |terms| for a sum of n terms against math.fsum of the same terms."""
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
import friction_report_ref as fr  # noqa: E402
from oracle import evaluator as ev  # noqa: E402

U = fr.U
STATES = [(name, s) for name in fr.FIXTURES for s in range(3)]
ROWS = {"contactmix_t0": 292, "contactmix_t1": 212, "contactcorners_t0": 58, "contactrods_t0": 47, "contactrods_t1": 40}
SRC = os.path.join(ROOT, "tests", "host_friction_report", "host_friction_report.cpp")


def potential(c, table):
    name = fr.TABLE_NAMES[table - fr.FIRST_TABLE]
    return [p for p in c["prob"].potentials if p.name == name][0]


def test_fixture_coverage():
    """Every table sticks and slides somewhere; no row near the threshold or without load; at the stored DoFs everything sticks."""
    stick, slide = set(), set()
    margin = np.inf
    for name, s in STATES:
        c = fr.fixture_case(name, s)
        ri, rd = c["ri"], c["rd"]
        assert len(ri) == ROWS[name]
        sliding = (ri[:, 7] & fr.SLIDING) != 0
        if s == 0:
            assert not sliding.any(), name
        stick |= set(int(t) for t in ri[~sliding, 0])
        slide |= set(int(t) for t in ri[sliding, 0])
        margin = min(margin, np.abs(rd[:, 5] / rd[:, 2] - 1.0).min())
        assert not (ri[:, 7] & (fr.NO_LOAD | fr.DEGENERATE)).any() and (rd[:, 0] * rd[:, 1] > 0.0).all()
    print("closest row to the threshold: | |u| / epsu - 1 | = %.3g" % margin)
    assert stick == slide == set(range(21, 35))
    assert margin >= 0.013


@pytest.mark.parametrize("name,s", STATES)
def test_restatement_against_the_oracle(name, s):
    c = fr.fixture_case(name, s)
    prob, ri, rd, contrib, dt = c["prob"], c["ri"], c["rd"], c["contrib"], c["dt"]
    cv_of = fr.vertex_index(c["scene"])
    src_of = {cv: key for key, cv in cv_of.items()}
    M = c["scene"].meshes
    L = fr.Layout(c["scene"])
    from contact_util import roles_from_manifest

    roles = roles_from_manifest(c["man"])
    row0 = {}
    for role in ("v1", "rb_v1", "rb_w1"):
        for sset, a in prob.dof_arrays.items():
            if a == roles.get(role):
                row0[role] = (prob.dof_offsets[sset] // 3, prob.dof_sizes[sset] // 3)
    worst_E = worst_f = 0.0
    n_d = n_rb = 0
    for table in range(21, 35):
        sel = np.nonzero(ri[:, 0] == table)[0]
        if len(sel) == 0:
            continue
        pot = potential(c, table)
        o = ev.evaluate_potential(prob, pot)
        assert o.active.all() and len(o.E) == len(sel) and (ri[sel, 1] == np.arange(len(sel))).all()
        worst_E = max(worst_E, (np.abs(rd[sel, 16] - o.E) / np.abs(o.E)).max())
        sliding = (ri[sel, 7] & fr.SLIDING) != 0
        assert np.array_equal(sliding, ~(rd[sel, 5] < rd[sel, 2]))
        nb = o.block_rows.shape[1]
        f = -o.g.reshape(-1, nb, 3) / dt
        for e, n in enumerate(sel):
            mufn, ft = rd[n, 0] * rd[n, 1], rd[n, 10:13]
            want = {}
            for cv, w in contrib[n]:  # (signed: +w on A, -w on B)
                g = int(L.cv_mesh[cv])
                if M[g].kind == "d":
                    row = row0["v1"][0] + src_of[cv][1]
                    n_d += 1
                else:
                    row = row0["rb_v1"][0] + M[g].idx_in_ps  # (a body's linear block takes its side's node forces: the weights sum to 1)
                    n_rb += 1
                want[row] = want.get(row, np.zeros(3)) + w * ft
            got = {}
            for blk in range(nb):
                row = int(o.block_rows[e, blk])
                if "rb_w1" in row0 and row0["rb_w1"][0] <= row < row0["rb_w1"][0] + row0["rb_w1"][1]:
                    continue  # (torques are not compared: dE/dw goes through the normalised quaternion and is not r x ft)
                got[row] = got.get(row, np.zeros(3)) + f[e, blk]
            assert set(got) == set(want), (table, e)
            for row in got:
                worst_f = max(worst_f, np.abs(got[row] - want[row]).max() / mufn)
    print("%s state %d: worst energy error %.3g relative, worst node force deviation %.3g mu fn (%d deformable, %d rigid contributions)" % (name, s, worst_E, worst_f, n_d, n_rb))
    assert worst_E <= 1e-11 and worst_f <= 1e-11 and n_d + n_rb > 0


@pytest.mark.parametrize("name,s", STATES)
def test_identities(name, s):
    c = fr.fixture_case(name, s)
    ri, rd = c["ri"], c["rd"]
    assert (rd[:, 14] <= 1.0).all() and (rd[:, 14] >= 0.0).all()
    sliding = (ri[:, 7] & fr.SLIDING) != 0
    assert (np.abs(rd[sliding, 14] - 1.0) <= 8 * U).all()
    assert (np.abs(rd[~sliding, 14] - rd[~sliding, 5] / rd[~sliding, 2]) <= 16 * U).all()  # mobilised = min(|u| / epsu, 1)
    assert np.array_equal(rd[:, 15], np.array([float(rd[n, 10:13] @ rd[n, 7:10]) for n in range(len(rd))]))  # dissipation = ft . v
    assert (rd[:, 15] >= 0.0).all() and (rd[:, 16] >= 0.0).all() and (rd[:, 21:] == 0.0).all()
    assert np.array_equal(rd[:, 6], rd[:, 5] / c["dt"])
    # the node weights of a side sum to one (bary as the reference stores it: within a few roundings)
    for n, cs in enumerate(c["contrib"]):
        assert abs(sum(w for _, w in cs)) <= 16 * U
    pairs, terms = fr.pair_report(c["scene"], ri, rd)
    assert pairs[:, :, 0].sum() == len(ri) and pairs[:, :, 1].sum() == sliding.sum()
    for (ga, gb), T in terms.items():
        for f, xs in T.items():
            assert abs(pairs[ga, gb, f] - math.fsum(xs)) <= fr.sum_bound(xs), (ga, gb, f)
    for f, col in ((2, rd[:, 1]), (3, rd[:, 0] * rd[:, 1]), (7, rd[:, 13]), (8, rd[:, 15]), (9, rd[:, 16])):
        assert abs(pairs[:, :, f].sum() - math.fsum(col)) <= fr.sum_bound(list(col)) + 64 * U * abs(math.fsum(col))
    assert (pairs[:, :, 11] <= 1.0 + 1e-12).all() and pairs[:, :, 10].max() == rd[:, 6].max()
    vert, vterms = fr.vertex_report(c["scene"], ri, rd, c["contrib"], c["X"])
    assert vert[:, 0].sum() == sum(len(cs) for cs in c["contrib"])
    for v, vs in enumerate(vterms):
        assert vert[v, 0] == len(vs)
        assert (np.abs(vert[v, 2:5] - fr.fsum3(vs)) <= fr.vector_sum_bound(vs)).all()
    # every row acts on A with ft and on B with -ft: the vertex forces of the whole scene cancel
    allv = [x for vs in vterms for x in vs]
    assert (np.abs(vert[:, 2:5].sum(axis=0)) <= fr.vector_sum_bound(allv) + 16 * U * sum(np.linalg.norm(x) for x in allv)).all()


@pytest.fixture(scope="module")
def host_lib():
    out = os.path.join(tempfile.mkdtemp(prefix="mistark_host_friction_report_"), "host_friction_report.so")
    subprocess.run(["g++", "-std=c++17", "-O2", "-shared", "-fPIC", SRC, "-o", out], check=True)
    lib = ctypes.CDLL(out)
    p = ctypes.c_void_p
    lib.host_friction_rows.argtypes = [p, p, p, p, p, p, ctypes.c_double, ctypes.c_double, ctypes.c_int, p, p, p]
    lib.host_friction_rigid_velocity.argtypes = [p, p, p, p, ctypes.c_double, p]
    return lib


def gathered_inputs(c, lib):
    """Per row what the header takes: meta [n, 6], velocities [n, 5, 3] (A's two, B's three; rigid vertices through the header's own
    fr_rigid_velocity), T [n, 6], mu, fn [n], bary [n, 3]."""
    ri, st, dt = c["ri"], c["st"], c["dt"]
    n = len(ri)
    meta = np.ascontiguousarray(ri[:, [0, 1, 3, 4, 5, 6]]).astype(np.int32)
    vel, T, mu, fn, bary = np.zeros((n, 5, 3)), np.zeros((n, 6)), np.zeros(n), np.zeros(n), np.zeros((n, 3))
    cv_of = fr.vertex_index(c["scene"])
    src_of = {cv: key for key, cv in cv_of.items()}
    worst_rigid = 0.0

    def velocity(cv, body):
        nonlocal worst_rigid
        kind, s = src_of[cv]
        if kind == "d":
            return st["v1"][s]
        out = np.zeros(3)
        args = [np.ascontiguousarray(a, dtype=np.float64) for a in (st["rb_v1"][body], st["rb_w1"][body], st["rb_q0"][body], st["rb_xloc"][s])]
        lib.host_friction_rigid_velocity(args[0].ctypes.data, args[1].ctypes.data, args[2].ctypes.data, args[3].ctypes.data, dt, out.ctypes.data)
        want = fr.rigid_velocity(st, body, st["rb_xloc"][s], dt)
        scale = np.abs(st["rb_v1"][body]).max() + np.linalg.norm(st["rb_w1"][body]) * np.linalg.norm(st["rb_xloc"][s])
        worst_rigid = max(worst_rigid, np.abs(out - want).max() / max(scale, 1e-300))
        return out

    i = 0
    for t, name in enumerate(fr.TABLE_NAMES):
        tb = c["tables"].get(name)
        if tb is None:
            continue
        for r in range(len(tb["conn"])):
            cs = c["contrib"][i]
            na = 2 if ri[i, 2] == 3 else 1
            for j, (cv, _) in enumerate(cs[:na]):
                vel[i, j] = velocity(cv, ri[i, 5])
            for j, (cv, _) in enumerate(cs[na:]):
                vel[i, 2 + j] = velocity(cv, ri[i, 6])
            T[i], mu[i], fn[i] = np.asarray(tb["T"]).reshape(-1, 6)[r], np.asarray(tb["mu"]).reshape(-1)[r], np.asarray(tb["fn"]).reshape(-1)[r]
            if tb.get("bary") is not None:
                b = np.asarray(tb["bary"]).reshape(len(tb["conn"]), -1)[r]
                bary[i, :len(b)] = b
            i += 1
    assert i == n
    return meta, vel, T, mu, fn, bary, worst_rigid


@pytest.mark.parametrize("name,s", STATES)
def test_header_against_the_restatement(name, s, host_lib):
    c = fr.fixture_case(name, s)
    meta, vel, T, mu, fn, bary, worst_rigid = gathered_inputs(c, host_lib)
    n = len(meta)
    ri, rd, w = np.zeros((n, 8), dtype=np.int32), np.zeros((n, 24)), np.zeros((n, 5))
    assert host_lib.host_friction_rows(meta.ctypes.data, vel.ctypes.data, T.ctypes.data, mu.ctypes.data, fn.ctypes.data, bary.ctypes.data, c["dt"], c["epsv"], n, ri.ctypes.data,
                                       rd.ctypes.data, w.ctypes.data) == 0
    assert (ri == c["ri"]).all()  # the sliding flag among them: no row is left out
    err = np.abs(rd - c["rd"]) / fr.field_scales(c["ri"], c["rd"], fr.state_vmax(c["st"]), c["dt"])
    print("%s state %d: worst field error %.3g, worst rigid velocity error %.3g (bound %.3g)" % (name, s, err.max(), worst_rigid, 64 * U))
    assert (err <= 64 * U).all() and worst_rigid <= 64 * U
    assert (rd[:, 14] <= 1.0).all()
    for i, cs in enumerate(c["contrib"]):
        na = 2 if ri[i, 2] == 3 else 1
        want = [x for _, x in cs[:na]] + [0.0] * (2 - na) + [-x for _, x in cs[na:]] + [0.0] * (3 - (len(cs) - na))
        assert list(w[i]) == want  # the same operations on the same parameters: the same bits


def test_header_branches_on_synthetic_rows(host_lib):
    """One pp row pushed through the threshold, and a row without load: the sticking branch never divides by |u|."""
    dt, epsv = 0.01, 1e-3
    meta = np.array([[21, 0, 0, 1, -1, -1]] * 4, dtype=np.int32)
    vel = np.zeros((4, 5, 3))
    speeds = [0.0, 0.5e-3, 2e-3, 2e-3]  # |u| = 1.5e-9 (the offsets alone), 5e-6, 2e-5, 2e-5 beside epsu = 1e-5
    for i, sp in enumerate(speeds):
        vel[i, 2] = [sp, 0.0, 0.0]
    T = np.tile(np.array([1.0, 0.0, 0.0, 0.0, 1.0, 0.0]), (4, 1))
    mu, fn, bary = np.array([0.5, 0.5, 0.5, 0.0]), np.full(4, 10.0), np.zeros((4, 3))
    ri, rd, w = np.zeros((4, 8), dtype=np.int32), np.zeros((4, 24)), np.zeros((4, 5))
    host_lib.host_friction_rows(meta.ctypes.data, vel.ctypes.data, T.ctypes.data, mu.ctypes.data, fn.ctypes.data, bary.ctypes.data, dt, epsv, 4, ri.ctypes.data, rd.ctypes.data,
                                w.ctypes.data)
    assert list(ri[:, 7]) == [0, 0, fr.SLIDING, fr.SLIDING | fr.NO_LOAD]
    assert np.isfinite(rd).all()
    assert abs(rd[0, 5] - math.hypot(1.13e-9, 1.07e-9)) <= 4 * U * 2e-9 and rd[0, 13] > 0.0  # the offsets alone: a force of 1.5e-4 mu fn, not 0 / 0
    assert abs(rd[1, 14] - rd[1, 5] / rd[1, 2]) <= 8 * U and abs(rd[1, 16] - 0.5 * (5.0 / 1e-5) * rd[1, 5] ** 2) <= 64 * U * rd[1, 16]
    assert 1.0 - 8 * U <= rd[2, 14] <= 1.0 and abs(rd[2, 13] - 5.0) <= 8 * U * 5.0 and abs(rd[2, 16] - 5.0 * (rd[2, 5] - 0.5e-5)) <= 64 * U * 5.0 * rd[2, 5]
    assert rd[2, 10] > 0.0 and rd[2, 15] > 0.0  # B moves along +x over A: the force on A points along +x, friction takes power out
    assert (rd[3, 10:17] == 0.0).all() and rd[3, 5] == rd[2, 5]


def test_sanitizer_run_of_the_header():
    """The same file as a stand-alone program (its own main, no Python in the process, no preload) under AddressSanitizer and UBSan."""
    exe = os.path.join(tempfile.mkdtemp(prefix="mistark_host_friction_report_"), "host_friction_report_asan")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-DHOST_FRICTION_REPORT_MAIN", SRC, "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout, r.stderr)
    assert r.returncode == 0 and "rows 292" in r.stdout and "bad 0" in r.stdout and "ERROR" not in r.stderr and "runtime error" not in r.stderr
