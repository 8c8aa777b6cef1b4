"""Rigid-body wrench report without a GPU: the numpy restatement of tests/wrench_ref.py against the virtual-work derivative of the oracle's energy (a
reference that does not use the map), the header stark_amd/csrc/wrench.hpp compiled with g++ (tests/host_wrench/host_wrench.cpp, test-only) against the
restatement, the same file as a stand-alone program under the address and undefined-behaviour sanitizers, and the torque on side a of the constraint
restatement at non-zero w1.

Tolerances. Virtual work: the estimated error of the central difference per component (wrench_ref's docstring), printed. Header: per torque component
64 * 2^-53 * (1 + |a| + |a|^2) * sum_k |g_k| / dt, per force component 64 * 2^-53 |g| / dt. Constraints: 1e-11 * max |reference| over the potential,
the constraint report's own row tolerance."""
import ctypes
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

FIXTURES = ("rbchain", "contactmix_t0", "contactcorners_t0", "contactrods_t0", "attachzoo")
U = wr.U
SRC = os.path.join(ROOT, "tests", "host_wrench", "host_wrench.cpp")
_STATES = {}


def states(name):
    """(stored state, state with rigid.w1 scaled to max |a| = 0.5) of a fixture, loaded once."""
    if name not in _STATES:
        prob = ev.load_fixture(os.path.join(ROOT, "tests", "golden", name + ".npz"))[0]
        _STATES[name] = (prob, wr.scaled_state(prob, 0.5))
    return _STATES[name]


def rigid_potentials(prob, R):
    """indices of the potentials with rows that touch a rigid DoF set"""
    return [k for k, p in enumerate(prob.potentials) if len(p.conn) and any(b.dof_set in (R.set_v, R.set_w) for b in p.bindings)]


@pytest.fixture(scope="module")
def host_lib():
    out = os.path.join(tempfile.mkdtemp(prefix="mistark_host_wrench_"), "host_wrench.so")
    subprocess.run(["g++", "-std=c++17", "-O2", "-shared", "-fPIC", SRC, "-o", out], check=True)
    lib = ctypes.CDLL(out)
    p = ctypes.c_void_p
    lib.host_wrench_slots.argtypes = [p, p, p, ctypes.c_double, ctypes.c_int, p]
    lib.host_wrench_bodies.argtypes = [p, p, p, p, p, ctypes.c_double, p, ctypes.c_int, p]
    return lib


def host_bodies(lib, fv, fw, t0, v1, w1, dt, about):
    arrs = [np.ascontiguousarray(a, dtype=np.float64).reshape(-1, 3) for a in (fv, fw, t0, v1, w1)]
    ab = np.ascontiguousarray(about, dtype=np.float64)
    rec = np.zeros((len(arrs[0]), 16))
    assert lib.host_wrench_bodies(*[a.ctypes.data for a in arrs], float(dt), ab.ctypes.data, len(rec), rec.ctypes.data) == 0
    return rec


def test_the_scaled_states_reach_half_a_radian_of_cayley_parameter():
    for name in FIXTURES:
        prob, big = states(name)
        R = wr.Rigid(prob)
        a0 = 0.5 * prob.dt * np.linalg.norm(prob.arrays[R.w1].reshape(-1, 3), axis=1).max()
        a1 = 0.5 * big.dt * np.linalg.norm(big.arrays[R.w1].reshape(-1, 3), axis=1).max()
        print("%s: %d bodies, stored |a| %.3g, scaled %.3g" % (name, R.n, a0, a1))
        assert a0 <= 0.03 and abs(a1 - 0.5) < 1e-12


@pytest.mark.parametrize("name", FIXTURES)
def test_restated_wrench_is_the_virtual_work_derivative(name):
    """Per body, the restated F and tau_com of the family of all pose potentials against central differences of the oracle's energy in the body's
    translation and world-frame rotation, at the stored state and at |a| = 0.5. The bound is the estimated error of the difference."""
    worst = 0.0
    for prob in states(name):
        R = wr.Rigid(prob)
        fam = [k for k in rigid_potentials(prob, R) if wr.fd_usable(prob.potentials[k])]
        assert fam
        out, count, _, _ = wr.body_records(prob, [fam], (0.0, 0.0, 0.0), R)
        for b in range(R.n):
            if count[0, b] == 0:
                continue
            F, tau, bF, bT = wr.fd_wrench(prob, [prob.potentials[k] for k in fam], b, R=R)
            eF, eT = np.abs(out[0, b, 0:3] - F), np.abs(out[0, b, 3:6] - tau)
            print("%s body %d |a| %.3g: |F| %.3g err %.2e bound %.2e | |tau| %.3g err %.2e bound %.2e" %
                  (name, b, out[0, b, 15], np.linalg.norm(F), eF.max(), bF.max(), np.linalg.norm(tau), eT.max(), bT.max()))
            assert (eF <= bF).all(), (name, b, eF, bF)
            assert (eT <= bT).all(), (name, b, eT, bT)
            worst = max(worst, float((eT / np.maximum(bT, 1e-300)).max()))
    print("%s: worst torque error / bound %.3g" % (name, worst))


def test_a_wrong_map_fails_the_virtual_work_reference():
    """The check has teeth: with the sign of [a]x flipped, or a a^T dropped, the restatement misses the reference at |a| = 0.5."""
    prob = states("rbchain")[1]
    R = wr.Rigid(prob)
    fam = [k for k in rigid_potentials(prob, R) if wr.fd_usable(prob.potentials[k])]
    f, _, _ = wr.generalised_forces(prob, [prob.potentials[k] for k in fam])
    w1 = prob.arrays[R.w1].reshape(-1, 3)
    b = int(np.argmax(np.linalg.norm(w1, axis=1)))
    fw = f[3 * (R.w_row0 + b):3 * (R.w_row0 + b) + 3]
    a = 0.5 * prob.dt * w1[b]
    _, tau, _, bT = wr.fd_wrench(prob, [prob.potentials[k] for k in fam], b, R=R)
    assert (np.abs(wr.wrench_map(a, fw) - tau) <= bT).all()
    assert not (np.abs(fw - np.cross(a, fw) + a * np.dot(a, fw) - tau) <= bT).all()
    assert not (np.abs(fw + np.cross(a, fw) - tau) <= bT).all()


@pytest.mark.parametrize("name", FIXTURES)
def test_header_against_the_restatement(name, host_lib):
    n_checked = 0
    for prob in states(name):
        R = wr.Rigid(prob)
        w1 = prob.arrays[R.w1].reshape(-1, 3)
        for k in rigid_potentials(prob, R):
            pot = prob.potentials[k]
            rec, ids, mag = wr.row_records(prob, pot, R)
            o = ev.evaluate_potential(prob, pot)
            order = ev.dof_layout(pot)
            g = np.zeros((len(pot.conn), 3 * len(order)))
            g[o.active] = o.g
            rows = np.stack([prob.dof_offsets[pot.bindings[bi].dof_set] // 3 + pot.conn[:, pot.bindings[bi].conn] for bi in order], axis=1)
            for s in (0, 1):
                sel = np.nonzero((ids[:, s] >= 0) & ((ids[:, 3] & 1) == 0))[0]
                if not len(sel):
                    continue
                body = ids[sel, s]
                gv, gw = np.zeros((len(sel), 3)), np.zeros((len(sel), 3))
                for j, e in enumerate(sel):
                    for kk, row in enumerate(rows[e]):
                        if row == R.v_row0 + body[j]:
                            gv[j] += g[e, 3 * kk:3 * kk + 3]
                        if row == R.w_row0 + body[j]:
                            gw[j] += g[e, 3 * kk:3 * kk + 3]
                got = np.zeros((len(sel), 12))
                wb = np.ascontiguousarray(w1[body])
                assert host_lib.host_wrench_slots(gv.ctypes.data, gw.ctypes.data, wb.ctypes.data, float(prob.dt), len(sel), got.ctypes.data) == 0
                an = 0.5 * prob.dt * np.linalg.norm(wb, axis=1)
                bF = 64 * U * np.abs(gv) / prob.dt
                bT = wr.torque_bound(an, mag[sel, s, 1])[:, None] * np.ones(3)
                assert (np.abs(got[:, 0:3] - rec[sel, s, 0:3]) <= bF).all(), pot.name
                assert (np.abs(got[:, 3:6] - rec[sel, s, 3:6]) <= bT).all(), pot.name
                nF, nT = rec[sel, s, 10], rec[sel, s, 11]
                assert (np.abs(got[:, 10] - nF) <= 3 * bF.max(axis=1) + 4 * U * nF).all() and (np.abs(got[:, 11] - nT) <= 3 * bT[:, 0] + 4 * U * nT).all()
                # arm and couple carry the two inputs' bounds linearly: |d arm| <= (|dF| |tau| + |F| |dtau|) / |F|^2 + 2 |arm| |dF| / |F|
                ok = nF > 0
                dF, dT = np.sqrt(3) * bF.max(axis=1)[ok], np.sqrt(3) * bT[ok, 0]
                arm = np.linalg.norm(rec[sel, s, 6:9], axis=1)[ok]
                b_arm = (dF * nT[ok] + nF[ok] * dT) / nF[ok] ** 2 + 2 * arm * dF / nF[ok] + 8 * U * arm
                assert (np.abs(got[ok, 6:9] - rec[sel, s, 6:9][ok]) <= b_arm[:, None]).all(), pot.name
                b_c = dT + 2 * nT[ok] * dF / nF[ok] + 8 * U * nT[ok]
                assert (np.abs(got[ok, 9] - rec[sel, s, 9][ok]) <= b_c).all(), pot.name
                assert (got[~ok, 6:10] == 0.0).all()
                n_checked += len(sel)
        # bodies
        fams = [[], rigid_potentials(prob, R)[:3]]
        about = (0.3, -0.2, 0.5)
        out, _, mags, _ = wr.body_records(prob, fams, about, R)
        t0, v1 = prob.arrays[R.t0].reshape(-1, 3), prob.arrays[R.v1].reshape(-1, 3)
        for fi in range(len(fams)):
            got = host_bodies(host_lib, out[fi, :, 0:3], out[fi, :, 9:12], t0, v1, w1, prob.dt, about)
            an = out[fi, :, 15]
            bT = wr.torque_bound(an, mags[fi, :, 1].sum(axis=1))[:, None]
            assert (got[:, 0:3] == out[fi, :, 0:3]).all() and (got[:, 9:12] == out[fi, :, 9:12]).all()
            assert (np.abs(got[:, 3:6] - out[fi, :, 3:6]) <= bT).all()
            arm = np.abs(out[fi, :, 12:15] - np.asarray(about)).sum(axis=1)[:, None]
            assert (np.abs(got[:, 6:9] - out[fi, :, 6:9]) <= bT + 64 * U * arm * np.abs(out[fi, :, 0:3]).sum(axis=1)[:, None]).all()
            assert (np.abs(got[:, 12:16] - out[fi, :, 12:16]) <= 8 * U * (1.0 + np.abs(out[fi, :, 12:16]))).all()
    print("%s: %d slots checked" % (name, n_checked))
    assert n_checked > 0


def test_header_as_a_stand_alone_program_under_sanitizers():
    exe = os.path.join(tempfile.mkdtemp(prefix="mistark_host_wrench_san_"), "host_wrench_san")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-DHOST_WRENCH_MAIN", SRC, "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, (r.stdout, r.stderr)
    assert "0 mismatches" in r.stdout


POINT_KINDS = [n for n in cr.NAMES if n.startswith("rb_constraint_") and not cr.KINDS[n][4]]


def constraint_side_a_torque(name, want):
    """The constraint restatement's torque on side a (slots 5..7) as a torque of the potential. For every point-type kind but one, side a enters the energy
    through the one material point pa, and the slots are (pa - t1a) x f: the torque. rb_constraint_point_on_axis also reads the axis direction, which turns
    with body a: its force k nv acts on a at the foot of b on the axis, pa + s da, not at pa, and the constraint report's hand-written (pa - t1a) x f leaves
    s da x f out. As f is parallel to nv = (pb - pa) - s da, that term is (pb - pa) x f, formed here from the restatement's own anchors (slots 8..13)."""
    tau = want[:, 5:8].copy()
    if name == "rb_constraint_point_on_axis":
        tau += np.cross(want[:, 11:14] - want[:, 8:11], want[:, 2:5])
    return tau


@pytest.mark.parametrize("name", POINT_KINDS)
def test_tau_com_is_the_constraint_restatements_torque_on_side_a(name):
    """At the seeded problems' own w1 (|w1| dt up to 0.3), not at w1 = 0. For rb_constraint_point_on_axis the constraint report's slots 5..7 are not the
    torque of the potential (constraint_side_a_torque): measured on the seeded problem, max |tau| 5.04e4 and max difference 1.81e5 against the slots as
    they are, 1e-11 relative once the foot-point term is added. The virtual-work test above covers the kind through the rbchain fixture."""
    prob, _ = cr.seeded_problem(name)
    R = wr.Rigid(prob, v1=prob.dof_arrays[0], w1=prob.dof_arrays[1])
    assert 0.5 * prob.dt * np.linalg.norm(prob.arrays[R.w1].reshape(-1, 3), axis=1).max() > 0.1
    rec, ids, _ = wr.row_records(prob, prob.potentials[0], R)
    want, _ = cr.row_records(name, cr.gather(prob))
    side_a = cr.ids_of(prob, name)[:, 2] - R.v_row0
    assert (ids[:, 0] == side_a).all()
    ref = constraint_side_a_torque(name, want)
    scale = np.abs(ref).max()
    err = np.abs(rec[:, 0, 3:6] - ref).max()
    print("%s: max |tau| %.3g, max difference %.3g (allowed %.3g); against slots 5..7 as they are %.3g" %
          (name, scale, err, cr.ROW_TOL * scale, np.abs(rec[:, 0, 3:6] - want[:, 5:8]).max()))
    assert scale > 0.0 and err <= cr.ROW_TOL * scale
    assert np.abs(rec[:, 0, 0:3] - want[:, 2:5]).max() <= cr.ROW_TOL * np.abs(want[:, 2:5]).max()


CONTROLLERS = ("rb_constraint_linear_velocity", "rb_constraint_angular_velocity")


@pytest.mark.parametrize("name", CONTROLLERS)
def test_tau_com_of_the_velocity_controllers_is_their_hand_derived_torque(name):
    """The constraint restatement's slots 5..7 are no torque for these two (zero for the linear one, the generalised force on w1 for the angular one); the
    reference is wrench_ref.controller_torque, within the constraint report's row tolerance, at the seeded problems' own w1."""
    prob, _ = cr.seeded_problem(name)
    R = wr.Rigid(prob, v1=prob.dof_arrays[0], w1=prob.dof_arrays[1], need_pose=False)
    rec, ids, _ = wr.row_records(prob, prob.potentials[0], R)
    want, _ = cr.row_records(name, cr.gather(prob))
    on = (ids[:, 3] & 1) == 0
    assert on.sum() > 0
    a = 0.5 * prob.dt * prob.arrays[R.w1].reshape(-1, 3)[ids[:, 0]]
    assert np.linalg.norm(a, axis=1).max() > 0.1
    ref = wr.controller_torque(name, want[:, 2:5], want[:, 5:8], want[:, 8:11], want[:, 11:14], a, prob.dt)
    scale = np.abs(ref[on]).max()
    err = np.abs(rec[on, 0, 3:6] - ref[on]).max()
    print("%s: max |tau| %.3g, max difference %.3g (allowed %.3g); against slots 5..7 as they are %.3g" %
          (name, scale, err, cr.ROW_TOL * scale, np.abs(rec[on, 0, 3:6] - want[on, 5:8]).max()))
    assert scale > 0.0 and err <= cr.ROW_TOL * scale


# friction_rb_d_*: points of the rigid side (first object) and of the deformable side, number of barycentric weights, weights of the rigid side's points
FRICTION_RB_D = {"pp": (1, 1, 0, lambda w: [1.0]), "pe": (1, 2, 2, lambda w: [1.0]), "pt": (1, 3, 3, lambda w: [1.0]),
                 "ee": (2, 2, 2, lambda w: [1.0 - w[:, 0], w[:, 0]]), "ep": (2, 1, 2, lambda w: [w[:, 0], w[:, 1]]), "tp": (3, 1, 3, lambda w: [w[:, 0], w[:, 1], w[:, 2]])}


def test_friction_tables_torque_against_r_cross_ft():
    """The friction potentials take the velocity of a contact point of a body as v1 + w1 x r1, r1 = R1 r_loc: a function of w1 itself, not of the pose
    alone. Their torque is therefore not r1 x ft. By hand, with F = ft on the body and a = dt w1 / 2: dE/dw1 = -dt (r1 x F + G^T (r1 x (F x w1))), G the
    rotation per variation of w1, and the map gives
        tau_com = (I + [a]x + a a^T) (r1 x F) + 2 r1 x (F x a).
    That closed form is asserted on every row of the friction_rb_d_* tables of the fixtures (restatement against restatement: the constraint report's
    row tolerance, 1e-11 of the largest value). The difference to r1 x F, of first order in |a|, is measured and printed, not asserted."""
    n_rows, worst, worst_a = 0, 0.0, 0.0
    for fx in FIXTURES + ("contactmix_t1",):
        prob, _, _ = ev.load_fixture(os.path.join(ROOT, "tests", "golden", fx + ".npz"))
        R = wr.Rigid(prob)
        for pot in prob.potentials:
            if not pot.name.startswith("friction_rb_d_") or len(pot.conn) == 0:
                continue
            ka, kb, nbary, weights = FRICTION_RB_D[pot.name.split("_")[3]]
            inp = cr.gather(prob, pot)
            dt = inp[:, 0]
            loc = inp[:, 1:1 + 3 * ka].reshape(-1, ka, 3)
            o = 1 + 3 * ka
            w1, q0 = inp[:, o + 3:o + 6], inp[:, o + 9:o + 13]
            bary = inp[:, o + 13 + 3 * kb:o + 13 + 3 * kb + nbary]
            r_loc = sum(np.asarray(wk).reshape(-1, 1) * loc[:, k] for k, wk in enumerate(weights(bary)))
            r1 = cr.mv(cr.rot1(q0, w1, dt), r_loc)
            rec, ids, _ = wr.row_records(prob, pot, R)
            assert (ids[:, 0] >= 0).all() and (ids[:, 1] == -1).all() and (ids[:, 3] == 0).all()
            F, tau = rec[:, 0, 0:3], rec[:, 0, 3:6]
            a = 0.5 * dt[:, None] * w1
            rxF = np.cross(r1, F)
            ref = rxF + np.cross(a, rxF) + a * (a * rxF).sum(axis=1)[:, None] + 2.0 * np.cross(r1, np.cross(F, a))
            scale = max(np.abs(ref).max(), np.abs(rxF).max())
            err, diff = np.abs(tau - ref).max(), np.abs(tau - rxF).max()
            print("%s %s: %d rows, max |r1 x F| %.3g, closed form off by %.3g, tau_com - r1 x F up to %.3g (%.3g of the largest), max |a| %.3g"
                  % (fx, pot.name, len(rec), np.abs(rxF).max(), err, diff, diff / max(np.abs(rxF).max(), 1e-300), np.linalg.norm(a, axis=1).max()))
            if scale > 0.0:
                assert err <= cr.ROW_TOL * scale, (fx, pot.name)
                worst = max(worst, diff / max(np.abs(rxF).max(), 1e-300))
            worst_a = max(worst_a, np.linalg.norm(a, axis=1).max())
            n_rows += len(rec)
    print("friction_rb_d_* rows: %d; largest |tau_com - r1 x F| / max |r1 x F| of a table: %.3g at |a| up to %.3g" % (n_rows, worst, worst_a))
    assert n_rows > 0
