"""Rigid-body wrench report on the GPU (include/mistark.h "rigid-body wrench report"): rows and bodies against the numpy restatement of tests/wrench_ref.py
(itself checked against the virtual-work derivative in tests/test_wrench_cpu.py), against the engine's other pipelines, the long-row path, isolation,
empties and refusals.

Tolerances. ids, flags and counts exact; two calls the same bits. Rows against the restatement: F and tau_com within 1e-11 of the largest reference value
of the field over the potential (the project's parity tolerance between the engine's and the oracle's gradients) plus the header's bound
64 * 2^-53 * (1 + |a| + |a|^2) * sum_k |g_k| / dt; arm and couple carry those two linearly through their formulas. Bodies: slots 0..2 and 9..11 equal
Engine.forces bit for bit; 3..8 within the header's bound of the g++ build of the header on the same inputs. Sums: (n + 8) * 2^-53 * sum |terms|.

Where a body record is compared with a sum of body records (test_bodies: the family of all potentials against a partition), the map and the shift to
`about` are applied after the sum on one side and before it on the other. Beside the summation bound on the mapped terms, (n + 8) * 2^-53 *
(1 + |a| + |a|^2) * sum |terms|, the bound therefore takes the header's bound once per record that takes part, 4 * torque_bound for the three parts and
the whole; the torque about `about` takes the same and, for the arm's product, 64 * 2^-53 |t1 - about| sum |F terms| on top of the summation bound
(written (n + 72) * 2^-53 ...). Against the restatement the family of all potentials is allowed PARITY times the largest reference value plus twice
those two bounds, one for each side's own rounding. The long-row test states its bound where it applies it. The host mirror's limits are measured on
the reference's converged state; its test's docstring gives them."""
import ctypes as C
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

import constraint_report_ref as cr  # noqa: E402
import wrench_ref as wr  # noqa: E402
from oracle import evaluator as ev  # noqa: E402

pytestmark = pytest.mark.gpu

FIXTURES = ("rbchain", "contactmix_t0", "contactcorners_t0", "contactrods_t0", "attachzoo")
U = wr.U
PARITY = 1e-11
ABOUT = (0.3, -0.2, 0.5)
_REF = {}


def reference(name, which):
    """(problem, manifest, Rigid, {potential index: (rec, ids, mag)}) of a fixture at its stored state (0) or with rigid.w1 scaled to |a| = 0.5 (1);
    computed once and left unchanged."""
    key = (name, which)
    if key not in _REF:
        prob, man, _ = ev.load_fixture(os.path.join(ROOT, "tests", "golden", name + ".npz"))
        if which:
            prob = wr.scaled_state(prob, 0.5)
        R = wr.Rigid(prob)
        rows = {k: wr.row_records(prob, p, R) for k, p in enumerate(prob.potentials) if len(p.conn)}
        _REF[key] = (prob, man, R, rows)
    return _REF[key]


def is_rigid(prob, R, k):
    return any(b.dof_set in (R.set_v, R.set_w) for b in prob.potentials[k].bindings)


@pytest.fixture(scope="module")
def host_lib():
    out = os.path.join(tempfile.mkdtemp(prefix="mistark_host_wrench_"), "host_wrench.so")
    subprocess.run(["g++", "-std=c++17", "-O2", "-shared", "-fPIC", os.path.join(ROOT, "tests", "host_wrench", "host_wrench.cpp"), "-o", out], check=True)
    lib = C.CDLL(out)
    lib.host_wrench_bodies.argtypes = [C.c_void_p] * 5 + [C.c_double, C.c_void_p, C.c_int, C.c_void_p]
    return lib


def check_rows(name, got, gids, ref, a_of_body):
    rec, ids, mag = ref
    assert np.array_equal(gids, ids), name
    for s in (0, 1):
        on = (ids[:, s] >= 0) & ((ids[:, 3] & 1) == 0)
        assert (got[~on, s] == 0.0).all(), name
        if not on.any():
            continue
        an = a_of_body[ids[on, s]]
        dF = PARITY * np.abs(rec[:, s, 0:3]).max() + 64 * U * mag[on, s, 0]
        dT = PARITY * np.abs(rec[:, s, 3:6]).max() + wr.torque_bound(an, mag[on, s, 1])
        eF, eT = np.abs(got[on, s, 0:3] - rec[on, s, 0:3]).max(axis=1), np.abs(got[on, s, 3:6] - rec[on, s, 3:6]).max(axis=1)
        assert (eF <= dF).all(), (name, s, float((eF / dF).max()))
        assert (eT <= dT).all(), (name, s, float((eT / dT).max()))
        nF, nT = rec[on, s, 10], rec[on, s, 11]
        r3 = np.sqrt(3.0)
        assert (np.abs(got[on, s, 10] - nF) <= r3 * dF + 4 * U * nF).all() and (np.abs(got[on, s, 11] - nT) <= r3 * dT + 4 * U * nT).all(), name
        ok = nF > 4 * r3 * dF    # (where |F| is not resolved, arm and couple are not either)
        arm = np.linalg.norm(rec[on, s, 6:9], axis=1)[ok]
        b_arm = 2 * r3 * (dF[ok] * nT[ok] + nF[ok] * dT[ok]) / nF[ok] ** 2 + 4 * r3 * arm * dF[ok] / nF[ok] + 8 * U * arm
        assert (np.abs(got[on, s, 6:9][ok] - rec[on, s, 6:9][ok]).max(axis=1) <= b_arm).all(), name
        b_c = 2 * r3 * dT[ok] + 4 * r3 * nT[ok] * dF[ok] / nF[ok] + 8 * U * nT[ok]
        assert (np.abs(got[on, s, 9][ok] - rec[on, s, 9][ok]) <= b_c).all(), name


# ---- 1. rows against the restatement --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", [0, 1])
@pytest.mark.parametrize("name", FIXTURES)
def test_rows_match_the_restatement(name, which):
    prob, man, R, rows = reference(name, which)
    eng, ids = wr.engine_of(prob, man, R)
    a_of_body = 0.5 * prob.dt * np.linalg.norm(prob.arrays[R.w1].reshape(-1, 3), axis=1)
    n_rigid = 0
    for k, pid in sorted(eng.pot_ids.items()):
        got, gids = eng.rigid_wrench_rows(pid, **ids)
        again, gids2 = eng.rigid_wrench_rows(pid, **ids)
        assert got.tobytes() == again.tobytes() and np.array_equal(gids, gids2), prob.potentials[k].name
        check_rows(prob.potentials[k].name, got, gids, rows[k], a_of_body)
        if is_rigid(prob, R, k):
            n_rigid += 1
            assert (gids[:, 2] > 0).all()
        else:   # a potential without a rigid block is legal: zeros with bodies -1
            assert (gids == np.array([-1, -1, 0, 0])).all() and (got == 0.0).all()
    assert n_rigid >= 3
    print("%s state %d: %d rigid potentials, |a| up to %.3g" % (name, which, n_rigid, a_of_body.max()))
    eng.close()


# ---- 2. rows against the engine's other pipelines -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", FIXTURES)
def test_row_force_is_the_element_force_of_the_v_block(name):
    prob, man, R, rows = reference(name, 1)
    eng, ids = wr.engine_of(prob, man, R)
    n = n_sum = 0
    for k, pid in sorted(eng.pot_ids.items()):
        if not is_rigid(prob, R, k):
            continue
        got, gids = eng.rigid_wrench_rows(pid, **ids)
        f_el, brow = eng.element_forces(pid, 1.0 / prob.dt)
        for s in (0, 1):
            for e in np.nonzero(gids[:, s] >= 0)[0]:
                blocks = np.nonzero(brow[e] == R.v_row0 + gids[e, s])[0]
                if len(blocks) == 1:   # (one v block of the body in the element: the same product, bit for bit)
                    assert (got[e, s, 0:3] == f_el[e, blocks[0]]).all(), (prob.potentials[k].name, e, s)
                    n += 1
                elif len(blocks) == 0:
                    assert (got[e, s, 0:3] == 0.0).all()
                else:   # (both sides of a contact on one body: the row scales the sum of the blocks, the element forces are scaled one by one)
                    assert (np.abs(got[e, s, 0:3] - f_el[e, blocks].sum(axis=0)) <= 4 * U * np.abs(f_el[e, blocks]).sum(axis=0)).all()
                    n_sum += 1
    print("%s: %d slots compared bit for bit, %d as sums of two blocks" % (name, n, n_sum))
    assert n > 0
    eng.close()


def side_a_torque(name, rep):
    """Engine.constraint_report's torque on side a as the torque of the potential: tests/test_wrench_cpu.py constraint_side_a_torque (the report's slots
    5..7 of rb_constraint_point_on_axis leave the foot-point term (pb - pa) x f out)."""
    tau = rep["torque"].copy()
    if name == "rb_constraint_point_on_axis":
        tau += np.cross(rep["anchor_b"] - rep["anchor_a"], rep["force"])
    return tau


# The two velocity controllers: the constraint report's slots 5..7 are no torque of theirs (zero for rb_constraint_linear_velocity, the generalised force
# on w1 at a held pose for rb_constraint_angular_velocity). Their reference is the torque derived by hand from their energy, wrench_ref.controller_torque,
# formed from the constraint report's own force, torque and anchor slots, under the same 1e-11.
CONTROLLERS = ("rb_constraint_linear_velocity", "rb_constraint_angular_velocity")


@pytest.mark.parametrize("which", [0, 1])
def test_row_torque_is_the_constraint_reports_torque_on_side_a(which):
    """The eleven rigid-body kinds at the stored state and at |a| = 0.5: nine against the report's torque on side a, the two controllers against theirs."""
    prob, man, R, rows = reference("rbchain", which)
    eng, ids = wr.engine_of(prob, man, R)
    kinds = 0
    for k, pid in sorted(eng.pot_ids.items()):
        name = prob.potentials[k].name
        if not name.startswith("rb_constraint_"):
            continue
        got, gids = eng.rigid_wrench_rows(pid, **ids)
        rep = eng.constraint_report(pid)
        side_a = rep["row_a"] - (R.w_row0 if cr.KINDS[name][6] == [] else R.v_row0)
        assert (gids[:, 0] == side_a).all(), name
        if name in CONTROLLERS:
            a = 0.5 * prob.dt * prob.arrays[R.w1].reshape(-1, 3)[side_a]
            ref = wr.controller_torque(name, rep["force"], rep["torque"], rep["anchor_a"], rep["anchor_b"], a, prob.dt)
            ref[~rep["active"]] = 0.0
        else:
            ref = side_a_torque(name, rep)
        scale = max(np.abs(ref).max(), np.abs(got[:, 0, 3:6]).max())
        err = np.abs(got[:, 0, 3:6] - ref).max()
        print("%s: max |tau| %.3g, difference %.3g" % (name, scale, err))
        kinds += 1
        assert err <= PARITY * scale, name
    assert kinds == 11
    eng.close()


def test_contact_row_torque_is_the_normal_force_at_the_contact_reports_closest_point():
    """contact_rb_d_* tables as the detector installs them: tau_com = (c - t1) x (+-fn n), c the contact report's closest point on the rigid side, within
    1e-11 |c - t1| fn. Which of the report's sides a / b is the body is read off a third pipeline: the element forces on the row's deformable blocks
    are -fn n where the body is a and +fn n where it is b. Point-triangle rows are never mollified and are all compared; edge-edge rows are compared
    where the mollified flag is not set (fn of a mollified row is the barrier part only)."""
    import contact_report_ref as crr
    import test_gpu_contact as tc

    eng, prob, man, z, scene, st = tc.build("contactmix_t0")
    dt = float(np.asarray(st["dt"]).ravel()[0])
    assert eng.contact_update(dt) > 0
    R = wr.Rigid(prob)
    ids = dict(v1=eng.array_ids[(R.v1, 3)], w1=eng.array_ids[(R.w1, 3)], t0=eng.array_ids[(R.t0, 3)], q0=eng.array_ids[(R.q0, 4)], n_bodies=R.n)
    t1 = prob.arrays[R.t0].reshape(-1, 3) + dt * prob.arrays[R.v1].reshape(-1, 3)
    rep = eng.contact_report()
    n_pt = n_ee = n_mollified = 0
    for t, tname in enumerate(crr.TABLE_NAMES):
        lo, hi = rep["bounds"][t], rep["bounds"][t + 1]
        if not tname.startswith("contact_rb_d_") or hi == lo:
            continue
        pid = eng.potential_id(tname)
        rec, rids = eng.rigid_wrench_rows(pid, **ids)
        assert len(rec) == hi - lo and (rids[:, 0] >= 0).all() and (rids[:, 1] == -1).all() and (rids[:, 3] == 0).all(), tname
        f_el, brow = eng.element_forces(pid, 1.0 / dt)
        rigid = ((brow >= R.v_row0) & (brow < R.v_row0 + R.n)) | ((brow >= R.w_row0) & (brow < R.w_row0 + R.n))
        f_soft = np.where(rigid[:, :, None], 0.0, f_el).sum(axis=1)
        fn, nrm = rep["fn"][lo:hi], rep["normal"][lo:hi]
        fnn = fn[:, None] * nrm
        mollified = (rep["flags"][lo:hi] & crr.MOLLIFIED) != 0
        if "_pt_" in tname:
            assert not mollified.any(), tname
        use = ~mollified
        body_is_a = np.abs(f_soft + fnn).max(axis=1) < np.abs(f_soft - fnn).max(axis=1)
        assert (np.abs(f_soft - np.where(body_is_a[:, None], -fnn, fnn))[use] <= 1e-9 * fn[use, None]).all(), tname   # (the side is unambiguous)
        c = np.where(body_is_a[:, None], rep["point_a"][lo:hi], rep["point_b"][lo:hi])
        F = np.where(body_is_a[:, None], fnn, -fnn)
        arm = c - t1[rids[:, 0]]
        err = np.abs(rec[:, 0, 3:6] - np.cross(arm, F)).max(axis=1)
        bound = 1e-11 * np.linalg.norm(arm, axis=1) * fn
        print("%s: %d rows, %d compared, worst error / bound %.3g" % (tname, hi - lo, int(use.sum()), float((err[use] / np.maximum(bound[use], 1e-300)).max()) if use.any() else 0.0))
        assert (err[use] <= bound[use]).all(), tname
        if "_pt_" in tname:
            n_pt += int(use.sum())
        else:
            n_ee += int(use.sum())
            n_mollified += int(mollified.sum())
    print("point-triangle rows compared: %d (all); edge-edge rows compared: %d, mollified and left out: %d" % (n_pt, n_ee, n_mollified))
    assert n_pt > 0
    eng.close()


def test_friction_rows_carry_the_friction_reports_force_and_their_own_torque():
    """friction_rb_d_* tables as contact_update_friction installs them on contactmix_t0: F of a row is the friction report's ft on the body (+-ft: the
    side is not fixed by the table), within 1e-11 of the largest ft of the table. The torque is NOT r x ft (include/mistark.h): the potentials take a
    contact point's velocity as v1 + w1 x r1, a function of w1 itself. The friction report carries no contact point, so what is measured here, printed and
    not asserted, is the part no arm can explain: the couple along F (slot 9) over |tau_com|. The full difference to r1 x ft, with r1 restated from the
    tables' weights, and its closed form are in tests/test_wrench_cpu.py test_friction_tables_torque_against_r_cross_ft."""
    import friction_report_ref as frr
    import test_gpu_contact_report as tcr

    eng, c = tcr.build("contactmix_t0")
    assert eng.contact_update_friction() > 0
    prob = c["prob"]
    R = wr.Rigid(prob)
    ids = dict(v1=eng.array_ids[(R.v1, 3)], w1=eng.array_ids[(R.w1, 3)], t0=eng.array_ids[(R.t0, 3)], q0=eng.array_ids[(R.q0, 4)], n_bodies=R.n)
    rep = eng.friction_report()
    n_rows = 0
    for t, tname in enumerate(frr.TABLE_NAMES):
        lo, hi = rep["bounds"][t], rep["bounds"][t + 1]
        if not tname.startswith("friction_rb_d_") or hi == lo:
            continue
        rec, rids = eng.rigid_wrench_rows(eng.potential_id(tname), **ids)
        assert len(rec) == hi - lo and (rids[:, 0] >= 0).all() and (rids[:, 1] == -1).all() and (rids[:, 3] == 0).all(), tname
        F, ft = rec[:, 0, 0:3], rep["ft"][lo:hi]
        err = np.minimum(np.abs(F - ft).max(axis=1), np.abs(F + ft).max(axis=1))
        scale = np.abs(ft).max()
        tau = rec[:, 0, 11]
        share = np.abs(rec[:, 0, 9]) / np.where(tau > 0.0, tau, 1.0)
        print("%s: %d rows, max |ft| %.3g, |F -+ ft| up to %.3g (allowed %.3g); couple along F over |tau_com| up to %.3g"
              % (tname, hi - lo, scale, err.max(), PARITY * scale, share.max()))
        assert (err <= PARITY * scale).all(), tname
        n_rows += hi - lo
    assert n_rows > 0
    eng.close()


# ---- 3. bodies ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", [0, 1])
@pytest.mark.parametrize("name", FIXTURES)
def test_bodies(name, which, host_lib):
    prob, man, R, rows = reference(name, which)
    eng, ids = wr.engine_of(prob, man, R)
    pids = [pid for k, pid in sorted(eng.pot_ids.items())]
    idx = [k for k, pid in sorted(eng.pot_ids.items())]
    # a partition of the potentials into three families, then all
    parts = [pids[0::3], pids[1::3], pids[2::3]]
    fams = parts + [[]]
    out, cnt = eng.rigid_wrench(fams, about=ABOUT, **ids)
    out2, cnt2 = eng.rigid_wrench(fams, about=ABOUT, **ids)
    assert out.tobytes() == out2.tobytes() and np.array_equal(cnt, cnt2)
    t0, v1, w1 = (np.ascontiguousarray(prob.arrays[a].reshape(-1, 3)) for a in (R.t0, R.v1, R.w1))
    ab = np.ascontiguousarray(ABOUT, dtype=np.float64)
    rv, rw = 3 * R.v_row0, 3 * R.w_row0
    for fi, fam in enumerate(fams):
        f = eng.forces(fam if fam else None, 1.0 / prob.dt)
        fv, fw = f[rv:rv + 3 * R.n].reshape(-1, 3), f[rw:rw + 3 * R.n].reshape(-1, 3)
        assert (out[fi, :, 0:3] == fv).all() and (out[fi, :, 9:12] == fw).all(), fi
        host = np.zeros((R.n, 16))
        fvc, fwc = np.ascontiguousarray(fv), np.ascontiguousarray(fw)
        assert host_lib.host_wrench_bodies(fvc.ctypes.data, fwc.ctypes.data, t0.ctypes.data, v1.ctypes.data, w1.ctypes.data, float(prob.dt), ab.ctypes.data, R.n, host.ctypes.data) == 0
        an = host[:, 15]
        bT = wr.torque_bound(an, np.abs(fw).sum(axis=1))[:, None]
        arm = np.abs(host[:, 12:15] - ab).sum(axis=1)[:, None]
        assert (np.abs(out[fi, :, 3:6] - host[:, 3:6]) <= bT).all()
        assert (np.abs(out[fi, :, 6:9] - host[:, 6:9]) <= bT + 64 * U * arm * np.abs(fv).sum(axis=1)[:, None]).all()
        assert (np.abs(out[fi, :, 12:16] - host[:, 12:16]) <= 8 * U * (1.0 + np.abs(host[:, 12:16]))).all()
    # counts: exact, from the restatement's ids
    for fi, fam in enumerate(fams):
        want = np.zeros(R.n, dtype=np.int64)
        for k in (idx if not fam else [idx[pids.index(p)] for p in fam]):
            rids = rows[k][1]
            for s in (0, 1):
                sel = (rids[:, s] >= 0) & ((rids[:, 3] & 1) == 0)
                np.add.at(want, rids[sel, s], 1)
        assert np.array_equal(cnt[fi], want), (fi, cnt[fi], want)
    assert np.array_equal(cnt[3], cnt[0] + cnt[1] + cnt[2])
    # the family of all potentials against the sum of the partition: the summation bound over the element terms
    ref_out, _, mags, nterms = wr.body_records(prob, [[]], ABOUT, R)
    for b in range(R.n):
        n = nterms[0, b].max()
        total = out[0, b] + out[1, b] + out[2, b]
        bF = (n + 8) * U * mags[0, b, 0]
        assert (np.abs(out[3, b, 0:3] - total[0:3]) <= bF).all() and (np.abs(out[3, b, 9:12] - total[9:12]) <= (n + 8) * U * mags[0, b, 1]).all()
        bT = (n + 8) * U * mags[0, b, 1].sum() * (1.0 + out[3, b, 15] + out[3, b, 15] ** 2) + 4 * wr.torque_bound(out[3, b, 15], mags[0, b, 1].sum())
        assert (np.abs(out[3, b, 3:6] - total[3:6]) <= bT).all()
        d = np.abs(out[3, b, 12:15] - ab).sum()
        assert (np.abs(out[3, b, 6:9] - total[6:9]) <= bT + (n + 72) * U * d * mags[0, b, 0].sum()).all()
        # ... and the restatement
        assert (np.abs(out[3, b, 0:6] - ref_out[0, b, 0:6]) <= PARITY * np.abs(ref_out[0, :, 0:6]).max() + 2 * bT + 2 * bF.max()).all()
    assert eng.counter("wrench_reports") == 2
    eng.close()


# ---- 4. the long-row path -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_bodies", [1, 2])
@pytest.mark.parametrize("n_att", [64, 65, 256, 257, 300])
def test_long_rows(n_att, n_bodies):
    prob, R, att = wr.star_problem(n_att, n_bodies)
    eng, ids = wr.engine_of(prob, None, R)
    pid = eng.pot_ids[0]
    rec, rids = eng.rigid_wrench_rows(pid, **ids)
    assert (rids[:, 0] == att).all() and (rids[:, 1] == -1).all() and (rids[:, 2] == 2).all() and (rids[:, 3] == 0).all()
    assert (rec[:, 0, 10] > 0.0).all()   # every attachment pulls
    out, cnt = eng.rigid_wrench([[pid], []], about=ABOUT, **ids)
    # (two families; in each the v row and the w row of body 0, and the inertia potential adds one contribution to the v row of the second)
    assert eng.counter("wrench_long_rows") == 2 * (n_att > 256) + (n_att > 256) + (n_att + 1 > 256)
    out1, cnt1 = eng.rigid_wrench([[pid]], about=ABOUT, **ids)
    assert eng.counter("wrench_long_rows") == (2 if n_att > 256 else 0)
    assert out1.tobytes() == out[:1].tobytes() and np.array_equal(cnt1, cnt[:1])
    assert np.array_equal(cnt[0], np.bincount(att, minlength=n_bodies))
    assert np.array_equal(cnt[1], cnt[0] + 1)   # (the inertia potential has one element per body)
    w1 = prob.arrays[R.w1].reshape(-1, 3)
    for b in range(n_bodies):
        mine = att == b
        n = int(mine.sum())
        an = 0.5 * prob.dt * np.linalg.norm(w1[b])
        for c in range(3):
            F = math.fsum(rec[mine, 0, c])
            assert abs(out[0, b, c] - F) <= (n + 8) * U * np.abs(rec[mine, 0, c]).sum(), (b, c)
            T = math.fsum(rec[mine, 0, 3 + c])
            # the rows map their own gradient, the body maps the sum: the summation bound on the mapped terms and the header's bound on both sides
            mapped = (1.0 + an + an * an) * np.abs(rec[mine, 0, 3:6]).sum()
            assert abs(out[0, b, 3 + c] - T) <= (n + 8) * U * mapped + 2 * wr.torque_bound(an, mapped), (b, c)
    eng.close()


# ---- 5. isolation, empties, refusals ------------------------------------------------------------------------------------------------------
def test_reports_leave_evaluation_matrix_and_solve_alone():
    from stark_amd import capi

    prob, man, R, rows = reference("contactmix_t0", 0)

    def sequence(report):
        eng, ids = wr.engine_of(prob, man, R)
        pids = [pid for k, pid in sorted(eng.pot_ids.items())]

        def reports():
            if report:
                for p in pids:
                    eng.rigid_wrench_rows(p, **ids)
                eng.rigid_wrench([[], pids[:4]], about=ABOUT, **ids)

        reports()
        E, grad = eng.eval(capi.EVAL_P_G_H)
        reports()
        eng.assemble()
        reports()
        bsr = eng.get_bsr()
        x, info = eng.pcg(man["pcg"]["abs_tol"])
        reports()
        E2, grad2 = eng.eval(capi.EVAL_P_G)
        n = eng.counter("wrench_reports")
        assert n == (4 * (len(pids) + 1) if report else 0)
        eng.close()
        return E, grad, bsr, x, info.n_iterations, E2, grad2

    E0, g0, (rp0, c0, v0), x0, it0, F0, h0 = sequence(False)
    E1, g1, (rp1, c1, v1), x1, it1, F1, h1 = sequence(True)
    assert E0 == E1 and np.array_equal(g0, g1) and F0 == F1 and np.array_equal(h0, h1)
    assert np.array_equal(rp0, rp1) and np.array_equal(c0, c1) and np.array_equal(v0, v1)
    assert it0 == it1 and np.array_equal(x0, x1)


def test_reports_leave_the_contact_tables_alone_and_read_them_as_installed():
    import test_gpu_contact as tc

    def sequence(report):
        eng, prob, man, z, scene, st = tc.build("contactmix_t0")
        dt = float(np.asarray(st["dt"]).ravel()[0])
        eng.contact_update_friction()
        n = eng.contact_update(dt)
        names = [p.name for p in prob.potentials if tc.is_contact(p.name)]
        got = {}
        if report:
            R = wr.Rigid(prob)
            ids = dict(v1=eng.array_ids[(R.v1, 3)], w1=eng.array_ids[(R.w1, 3)], t0=eng.array_ids[(R.t0, 3)], q0=eng.array_ids[(R.q0, 4)], n_bodies=R.n)
            for nm in names:
                got[nm] = eng.rigid_wrench_rows(eng.potential_id(nm), **ids)
            got["all"] = eng.rigid_wrench([[]], about=ABOUT, **ids)
        tables = {nm: eng.contact_table(nm) for nm in names}
        E, grad = eng.eval(1)
        eng.close()
        return n, tables, E, grad, got

    n0, t0, E0, g0, _ = sequence(False)
    n1, t1, E1, g1, got = sequence(True)
    assert n0 == n1 and E0 == E1 and np.array_equal(g0, g1)
    touched = 0
    for nm in t0:
        assert np.array_equal(t0[nm], t1[nm]), nm
        rec, ids = got[nm]
        assert len(rec) == len(t1[nm])   # rows line up with the table as installed
        if "_rb_" in nm and len(rec):
            assert (ids[:, 0] >= 0).all(), nm
            touched += len(rec)
    assert touched > 0 and got["all"][1].sum() > 0


def test_empties():
    prob, man, R, rows = reference("contactmix_t0", 0)
    eng, ids = wr.engine_of(prob, man, R)
    k = sorted(kk for kk in eng.pot_ids if "contact_rb" in prob.potentials[kk].name)[0]
    pid = eng.pot_ids[k]
    eng.set_dynamic(pid, True)
    eng.update_connectivity(pid, prob.potentials[k].conn[:0])   # the table runs empty, as a contact table does when its pairs separate
    rec, rids = eng.rigid_wrench_rows(pid, **ids)
    assert rec.shape == (0, 2, 12) and rids.shape == (0, 4)
    out, cnt = eng.rigid_wrench([[pid]], about=ABOUT, **ids)
    assert (out[0, :, 0:12] == 0.0).all() and (cnt == 0).all() and (out[0, :, 15] > 0.0).all()
    n = eng.counter("wrench_reports")
    assert n == 1   # (the body report launched its one kernel; the empty table launched nothing)
    # size queries launch nothing
    m = C.c_int64()
    other = eng.pot_ids[sorted(kk for kk in eng.pot_ids if is_rigid(prob, R, kk) and kk != k)[0]]
    assert eng.L.mistark_potential_rigid_wrench(eng.h, other, ids["v1"], ids["w1"], ids["t0"], ids["q0"], R.n, None, None, C.byref(m)) == 0 and m.value > 0
    ab = (C.c_double * 3)(*ABOUT)
    start = (C.c_int32 * 2)(0, 0)
    assert eng.L.mistark_rigid_wrench(eng.h, None, start, 1, ids["v1"], ids["w1"], ids["t0"], ids["q0"], R.n, ab, None, None) == 0
    out, cnt = eng.rigid_wrench([], about=ABOUT, **ids)
    assert out.shape == (0, R.n, 16)
    assert eng.counter("wrench_reports") == n
    eng.close()


def test_no_bodies():
    """n_bodies = 0: the state arrays are empty, every block is "not rigid"."""
    import stark_amd
    from gpu_util import engine_from_problem

    dof_array = lambda eng, s: eng._ck(eng.L.mistark_dof_array(eng.h, s, 3))
    # a deformable scene: its two rigid DoF sets are registered and empty
    prob, man, _ = ev.load_fixture(os.path.join(ROOT, "tests", "golden", "tetbeam_eo_4x1x1.npz"))
    assert len(prob.dof_sizes) == 3 and prob.dof_sizes[1] == 0 and prob.dof_sizes[2] == 0
    eng = engine_from_problem(prob, man)
    ids = dict(v1=dof_array(eng, 1), w1=dof_array(eng, 2), t0=eng.array(np.zeros((0, 3)), 3), q0=eng.array(np.zeros((0, 4)), 4), n_bodies=0)
    n = 0
    for k, pid in sorted(eng.pot_ids.items()):
        rec, rids = eng.rigid_wrench_rows(pid, **ids)
        assert len(rec) == len(prob.potentials[k].conn) and (rec == 0.0).all() and (rids == np.array([-1, -1, 0, 0])).all()
        n += 1
    out, cnt = eng.rigid_wrench([[]], about=ABOUT, **ids)
    assert out.shape == (1, 0, 16) and cnt.shape == (1, 0)
    assert eng.counter("wrench_reports") == n   # (a body report without bodies launches nothing)
    eng.close()
    # no inertia potential: nothing binds the time step
    prob, _ = cr.seeded_problem("rb_constraint_points")
    eng = engine_from_problem(prob)
    R = wr.Rigid(prob, v1=prob.dof_arrays[0], w1=prob.dof_arrays[1])
    ids = dict(v1=eng.array_ids[(R.v1, 3)], w1=eng.array_ids[(R.w1, 3)], t0=eng.array_ids[(R.t0, 3)], q0=eng.array_ids[(R.q0, 4)], n_bodies=R.n)
    for call in (lambda: eng.rigid_wrench_rows(eng.pot_ids[0], **ids), lambda: eng.rigid_wrench([[]], **ids)):
        with pytest.raises(stark_amd.engine.EngineError, match="no inertia potential"):
            call()
    eng.close()


def test_refusals():
    import stark_amd
    from gpu_util import engine_from_problem
    from stark_amd import capi

    Err = stark_amd.engine.EngineError
    prob, man, R, rows = reference("rbchain", 0)
    eng, ids = wr.engine_of(prob, man, R)
    pids = sorted(eng.pot_ids.values())
    for call in (lambda: eng.rigid_wrench_rows(len(prob.potentials) + 5, **ids), lambda: eng.rigid_wrench([[pids[0], 999]], **ids), lambda: eng.rigid_wrench([[-1]], **ids)):
        with pytest.raises(Err, match="bad potential id"):
            call()
    with pytest.raises(Err, match="listed twice"):
        eng.rigid_wrench([[pids[0]], [pids[1], pids[2], pids[1]]], **ids)
    eng.rigid_wrench([[pids[0]], [pids[0]]], **ids)   # (the same id in two families is legal)
    n0 = eng.counter("wrench_reports")

    def bad(**kw):
        a = dict(ids)
        a.update(kw)
        return a

    for a, what in ((bad(v1=ids["t0"]), "not a DoF array"), (bad(w1=ids["t0"]), "not a DoF array"), (bad(t0=ids["q0"]), "items of 4 doubles"),
                    (bad(q0=ids["t0"]), "items of 3 doubles"), (bad(n_bodies=R.n - 1), "n_bodies is %d" % (R.n - 1)), (bad(n_bodies=R.n + 1), "n_bodies is %d" % (R.n + 1)),
                    (bad(v1=ids["w1"]), "same DoF set"), (bad(v1=-1), "bad array id"), (bad(q0=10 ** 6), "bad array id")):
        for call in (lambda: eng.rigid_wrench_rows(pids[0], **a), lambda: eng.rigid_wrench([[]], **a)):
            with pytest.raises(Err, match=what):
                call()
    # a DoF array of the wrong stride
    nine = eng._ck(eng.L.mistark_dof_array(eng.h, R.set_v, 9))
    with pytest.raises(Err, match="items of 9 doubles"):
        eng.rigid_wrench_rows(pids[0], **bad(v1=nine))
    assert eng.counter("wrench_reports") == n0
    eng.close()
    # user-defined potentials, by name
    p2, m2, z2 = ev.load_fixture(os.path.join(ROOT, "tests", "golden", "tetbeam_eo_4x1x1.npz"))
    eng = engine_from_problem(p2, m2, custom_ops=z2)
    pid = sorted(eng.pot_ids.values())[0]
    for call in (lambda: eng.rigid_wrench_rows(pid, 0, 0, 0, 0, 0), lambda: eng.rigid_wrench([[pid]], 0, 0, 0, 0, 0), lambda: eng.rigid_wrench([[]], 0, 0, 0, 0, 0)):
        with pytest.raises(Err, match="user-defined"):
            call()
    eng.close()
    # sharded and registration-only contexts
    L = capi.lib()
    group = L.mistark_local_group_create(2)
    try:
        eng = stark_amd.Engine(0)
        eng.dist_init_local(group, 0)
        eng.add_dof_set("u", np.zeros(6))
        for call in (lambda: eng.rigid_wrench_rows(0, 0, 0, 0, 0, 0), lambda: eng.rigid_wrench([[]], 0, 0, 0, 0, 0)):
            with pytest.raises(Err, match="single-rank"):
                call()
        eng.close()
    finally:
        L.mistark_local_group_destroy(group)
    h = C.c_void_p()
    assert L.mistark_create_dry(C.byref(h)) == 0
    try:
        n = C.c_int64()
        assert L.mistark_potential_rigid_wrench(h, 0, 0, 0, 0, 0, 0, None, None, C.byref(n)) < 0
        assert "registration-only" in L.mistark_last_error(h).decode()
        ab, start = (C.c_double * 3)(0.0, 0.0, 0.0), (C.c_int32 * 2)(0, 0)
        assert L.mistark_rigid_wrench(h, None, start, 1, 0, 0, 0, 0, 0, ab, None, None) < 0
        assert "registration-only" in L.mistark_last_error(h).decode()
    finally:
        L.mistark_destroy(h)


# ---- 6. the host mirror ---------------------------------------------------------------------------------------------------------------------------
def facade(sim):
    import stark_amd
    from stark_amd import capi

    eng = stark_amd.Engine.__new__(stark_amd.Engine)  # the simulation's own engine context through the facade (not owned: never closed here)
    eng.L, eng.h = capi.lib(), sim.engine_handle()
    return eng


def test_host_mirror_on_the_rbchain_scene():
    """Simulation.record_wrench() / wrench() on the rbchain scene (9 boxes, all 13 rigid-body potentials; the first call of run_one_step ends with "invalid
    converged state" and is redone, tests/test_gpu_scene.py).
    - Recording changes nothing: Newton, solve and CG counts, the time after every call, the bodies' state and the DoFs are the same bits.
    - wrench() of the last step equals, bit for bit, Engine.rigid_wrench on a second, identical simulation taken to the start of that step
      (begin_time_step) with its DoFs set to what the step converged to, the families and array ids from Simulation.wrench_sources().
    - Balance at every accepted step: per body, the unbalanced |F| over the sum of the six source families' |F|, and the same for tau_com. The limit is
      measured, not chosen: on the reference's converged state (tests/golden/traj_rbchain.npz by the oracle restatement, wrench_ref.reference_balance)
      the largest ratio of a body is 5.01e-3 for the force and 0.146 for the torque (body 4, whose loads are 6.5e-3 N m in all: the Newton loop stops on
      the residual of the whole system, not on a body's share). Allowed is 10 times that, as the engine stops on the same tolerance but not at the same
      iterate: 5.01e-2 and 1.46. A ratio cannot exceed 1, so the torque's per-body limit cannot fail; the scene-wide measure therefore stands beside
      it, the largest unbalanced magnitude of a body over the largest load sum of a body: measured 4.68e-5 and 4.46e-3, allowed 4.68e-4 and 4.46e-2.
      Every figure is printed."""
    from stark_amd import sim as S

    CALLS = 4

    def run(record):
        sim = wr.rbchain_scene(S)
        if record:
            sim.record_wrench(True, ABOUT)
        counts, reps, u_steps = [], [], []
        for _ in range(CALLS):
            t_before = sim.info().current_time
            assert sim.run_one_step()
            i = sim.info()
            counts.append((i.total_newton_iterations, i.total_linear_solves, i.total_cg_iterations, i.current_time))
            if record and i.current_time > t_before:
                rep = sim.wrench()
                assert abs(rep["time"] - i.current_time) < 1e-12 and rep["labels"] == ["box%d" % k for k in range(9)]
                assert rep["families"] == sim.WRENCH_FAMILIES and rep["records"].shape == (7, 9, 16) and rep["counts"].shape == (7, 9)
                reps.append(rep)
        assert sim.info().current_time > t_before   # (the last call was accepted: its DoFs are the converged ones)
        eng = facade(sim)
        try:
            u = eng.get_dofs()
            n_reports = eng.counter("wrench_reports")
        finally:
            eng.h = None
        state = np.concatenate([np.concatenate(sim.rb_state(b)) for b in range(9)])
        if not record:
            with pytest.raises(S.SimError, match="recording is off"):
                sim.wrench()
        sim.close()
        return counts, state, u, n_reports, reps

    c_off, s_off, u_off, r_off, _ = run(False)
    c_on, s_on, u_on, r_on, reps = run(True)
    assert r_off == 0 and r_on == len(reps) >= 2
    assert c_on == c_off and s_on.tobytes() == s_off.tobytes() and u_on.tobytes() == u_off.tobytes()

    # the accessors on a second simulation
    sim = wr.rbchain_scene(S)
    for _ in range(CALLS - 1):
        assert sim.run_one_step()
    sim.begin_time_step()
    src = sim.wrench_sources()
    assert src["n_bodies"] == 9 and len(src["families"]["constraints"]) == 11 and src["families"]["all"] == []
    assert src["families"]["contact"] == [] and src["families"]["friction"] == [] and src["families"]["attachments"] == []
    eng = facade(sim)
    try:
        eng.set_dofs(u_on)
        ids = {k: src[k] for k in ("v1", "w1", "t0", "q0", "n_bodies")}
        present = [n for n in sim.WRENCH_FAMILIES if src["families"][n] or n == "all"]
        direct, dcount = eng.rigid_wrench([src["families"][n] for n in present], about=ABOUT, **ids)
    finally:
        eng.h = None
    sim.close()
    rec, cnt = reps[-1]["records"], reps[-1]["counts"]
    for k, name in enumerate(S.Simulation.WRENCH_FAMILIES):
        if name in present:
            assert rec[k].tobytes() == direct[present.index(name)].tobytes() and np.array_equal(cnt[k], dcount[present.index(name)]), name
        else:   # a family without potentials: the zero wrench at the body's place
            assert not rec[k, :, 0:12].any() and not cnt[k].any() and np.array_equal(rec[k, :, 12:16], rec[6, :, 12:16]), name
    assert np.array_equal(cnt[6], cnt[:6].sum(axis=0)) and (cnt[0] == 1).all() and (cnt[1] == 1).all()

    # balance
    ref_body, ref_scene = wr.reference_balance(os.path.join(ROOT, "tests", "golden", "traj_rbchain.npz"))
    lim_body, lim_scene = 10.0 * ref_body.max(axis=0), 10.0 * ref_scene
    print("reference: per body %s, scene %s; allowed: per body %s, scene %s" % (ref_body.max(axis=0), ref_scene, lim_body, lim_scene))
    for rep in reps:
        body, scene = wr.balance(rep["records"])
        print("t = %.4f: per body F %.3e tau %.3e; scene F %.3e tau %.3e" % (rep["time"], body[:, 0].max(), body[:, 1].max(), scene[0], scene[1]))
        assert np.isfinite(rep["records"]).all()
        assert (body.max(axis=0) <= lim_body).all() and (scene <= lim_scene).all(), (rep["time"], body.max(axis=0), scene)


def test_host_mirror_without_bodies():
    """A scene without rigid bodies: recording launches nothing and wrench() gives empty arrays."""
    from stark_amd import capi
    from stark_amd import sim as S

    sim = S.Simulation(S.default_settings())
    beam = sim.add_volume_grid("beam", (0, 0, 0), (0.4, 0.1, 0.1), (4, 1, 1), S.soft_rubber())
    sim.prescribe_inside_aabb(beam, (-0.2, 0, 0), (2e-3, 2, 2), 1e7)
    sim.record_wrench(True)
    with pytest.raises(S.SimError, match="no time step has been accepted"):
        sim.wrench()
    assert sim.run_one_step()
    rep = sim.wrench()
    assert rep["records"].shape == (7, 0, 16) and rep["counts"].shape == (7, 0) and rep["labels"] == [] and abs(rep["time"] - sim.info().current_time) < 1e-12
    v = C.c_int64()
    assert capi.lib().mistark_get_counter(sim.engine_handle(), b"wrench_reports", C.byref(v)) == 0 and v.value == 0
    with pytest.raises(S.SimError, match="not finite"):
        sim.record_wrench(True, (0.0, float("nan"), 0.0))
    sim.close()
