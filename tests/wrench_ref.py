"""Numpy restatement of the rigid-body wrench report (stark_amd/csrc/wrench.hpp, wrench.hip) from the oracle's element gradients, and a reference for
its map that does not use the map: the virtual-work derivative of the oracle's energy under a world-frame rotation of one body.

The map. rb_R1 normalises q0 + dt/2 (0, w1) q0 = (1, a) q0 with a = dt w1 / 2: R1 = C(a) R0, C the Cayley rotation. Then
    F = -(1/dt) dE/dv1,    tau_com = -(1/dt) (I + [a]x + a a^T) dE/dw1.

The reference. Rotating the body by theta about its centre in the world frame multiplies the quaternion (1, a) from the left by
(cos |theta|/2, sin |theta|/2 theta/|theta|); the vector part over the scalar part of the product is the new a (the inverse Cayley map), w1' = 2 a'/dt.
tau_i = -dE/dtheta_i, differentiated centrally at steps h and 2h and extrapolated: D = D(h) - (D(2h) - D(h)) / 3. Its error is estimated per component,
not chosen: the correction |D(2h) - D(h)| / 3 is the whole h^2 term that the extrapolation removed, so it bounds what is left (the h^4 term) as long as
the series converges at this step; the rounding error is 8 * 2^-53 * sum |E_element| / h for the energies that are subtracted. fd_wrench returns value
and bound. Only energies that are functions of the pose (t1, R1) have this reference: the angular inertia and the angular
velocity controller read w1 itself, the friction tables a lagged contact frame; they are left out of it (FD_EXCLUDED)."""
import copy

import numpy as np

import constraint_report_ref as cr
from oracle import evaluator as ev

U = 2.0 ** -53
FD_EXCLUDED = ("EnergyRigidBodyInertia_Angular", "rb_constraint_angular_velocity", "friction_")


class Rigid:
    """Where the bodies' state sits in a Problem: array indices of v1, w1, t0, q0, first block rows of the two DoF sets, body count."""

    def __init__(self, prob, v1=None, w1=None, need_pose=True):
        """v1, w1: array indices of the two DoF arrays; by default those the two rigid-body inertia potentials bind first. need_pose: t0 and q0 must be
        found (the body records need them, the row records do not)."""
        by_name = {p.name: p for p in prob.potentials}
        self.v1 = by_name["EnergyRigidBodyInertia_Linear"].bindings[0].array if v1 is None else v1
        self.w1 = by_name["EnergyRigidBodyInertia_Angular"].bindings[0].array if w1 is None else w1
        set_of = {a: s for s, a in prob.dof_arrays.items()}
        self.set_v, self.set_w = set_of[self.v1], set_of[self.w1]
        self.t0 = self.q0 = None
        for p in prob.potentials:
            bs = p.bindings
            for k in range(len(bs) - 3):
                if (bs[k].array, bs[k + 1].array) == (self.v1, self.w1) and bs[k + 2].stride == 3 and bs[k + 3].stride == 4:
                    self.t0, self.q0 = bs[k + 2].array, bs[k + 3].array
        assert self.t0 is not None or not need_pose, "no potential binds a body block {v1, w1, t0, q0}"
        self.v_row0 = prob.dof_offsets[self.set_v] // 3
        self.w_row0 = prob.dof_offsets[self.set_w] // 3
        self.n = prob.dof_sizes[self.set_v] // 3
        assert prob.dof_sizes[self.set_w] // 3 == self.n


def with_arrays(prob, **changes):
    """A copy of the problem with some arrays replaced ({array index: new array})."""
    q = copy.copy(prob)
    q.arrays = [a.copy() for a in prob.arrays]
    for k, v in changes.items():
        q.arrays[int(k)] = np.asarray(v, dtype=np.float64).reshape(prob.arrays[int(k)].shape).copy()
    return q


def scaled_state(prob, target=0.5):
    """The problem with the rigid.w1 block scaled so that the largest |a| = |dt w1 / 2| is `target`."""
    R = Rigid(prob)
    w = prob.arrays[R.w1].reshape(-1, 3)
    amax = 0.5 * prob.dt * np.linalg.norm(w, axis=1).max()
    assert amax > 0.0
    return with_arrays(prob, **{str(R.w1): w * (target / amax)})


def wrench_map(a, x):
    return x + np.cross(a, x) + a * np.dot(a, x)


def slot_record(gv, gw, w1, dt):
    a = 0.5 * dt * w1
    F = -(1.0 / dt) * gv
    tau = wrench_map(a, -(1.0 / dt) * gw)
    r = np.zeros(12)
    r[0:3], r[3:6] = F, tau
    F2 = float(np.dot(F, F))
    if F2 > 0.0:
        r[6:9] = np.cross(F, tau) / F2
        r[9] = np.dot(tau, F) / np.sqrt(F2)
    r[10], r[11] = np.sqrt(F2), np.linalg.norm(tau)
    return r


def row_records(prob, pot, R=None):
    """(rec [n_elem, 2, 12], ids [n_elem, 4], mag [n_elem, 2, 2]) of one potential; mag: sum_k |g_k| / dt of the v and of the w blocks of a slot (what the
    header's bound is stated in)."""
    R = R or Rigid(prob)
    ne = pot.conn.shape[0]
    rec, ids, mag = np.zeros((ne, 2, 12)), np.zeros((ne, 4), dtype=np.int32), np.zeros((ne, 2, 2))
    ids[:, :2] = -1
    if ne == 0:
        return rec, ids, mag
    o = ev.evaluate_potential(prob, pot)
    order = ev.dof_layout(pot)
    rows = np.stack([prob.dof_offsets[pot.bindings[bi].dof_set] // 3 + pot.conn[:, pot.bindings[bi].conn] for bi in order], axis=1)
    g = np.zeros((ne, 3 * len(order)))
    g[o.active] = o.g
    w1 = prob.arrays[R.w1].reshape(-1, 3)
    for e in range(ne):
        bodies, acc = [], {}
        flags = 0 if o.active[e] else 1
        n_rigid = 0
        for k, row in enumerate(rows[e]):
            bv, bw = row - R.v_row0, row - R.w_row0
            is_v, is_w = 0 <= bv < R.n, 0 <= bw < R.n
            if not (is_v or is_w):
                continue
            b = int(bv if is_v else bw)
            n_rigid += 1
            gk = g[e, 3 * k:3 * k + 3]
            if not np.isfinite(gk).all():
                flags |= 4
            if b not in bodies:
                if len(bodies) == 2:
                    flags |= 2
                    continue
                bodies.append(b)
                acc[b] = np.zeros((2, 3))
            acc[b][0 if is_v else 1] += gk
            mag[e, bodies.index(b), 0 if is_v else 1] += np.abs(gk).sum() / prob.dt
        for s, b in enumerate(bodies):
            ids[e, s] = b
            if o.active[e]:
                rec[e, s] = slot_record(acc[b][0], acc[b][1], w1[b], prob.dt)
        ids[e, 2], ids[e, 3] = n_rigid, flags
    return rec, ids, mag


def generalised_forces(prob, pots):
    """(f [ndofs], mag [ndofs], n [ndofs]) = -sum dE/du / dt over the potentials, the sum of the terms' magnitudes and their number per scalar DoF."""
    f, mag, n = np.zeros(prob.ndofs), np.zeros(prob.ndofs), np.zeros(prob.ndofs)
    for pot in pots:
        o = ev.evaluate_potential(prob, pot)
        if o is None:
            continue
        nb = o.block_rows.shape[1]
        idx = (3 * o.block_rows[:, :, None] + np.arange(3)[None, None, :]).reshape(-1)
        np.add.at(f, idx, -o.g.reshape(-1) / prob.dt)
        np.add.at(mag, idx, np.abs(o.g.reshape(-1)) / prob.dt)
        np.add.at(n, idx, 1.0)
    return f, mag, n


def body_records(prob, families, about, R=None):
    """(out [F, n_bodies, 16], count [F, n_bodies], mag [F, n_bodies, 2, 3], nterms [F, n_bodies, 2]) for families given as lists of potential indices
    (an empty list: every potential)."""
    R = R or Rigid(prob)
    about = np.asarray(about, dtype=np.float64)
    t0, v1, w1 = (prob.arrays[k].reshape(-1, 3) for k in (R.t0, R.v1, R.w1))
    out, count = np.zeros((len(families), R.n, 16)), np.zeros((len(families), R.n), dtype=np.int32)
    mags, nterms = np.zeros((len(families), R.n, 2, 3)), np.zeros((len(families), R.n, 2))
    for fi, fam in enumerate(families):
        pots = [prob.potentials[k] for k in fam] if len(fam) else list(prob.potentials)
        f, mag, n = generalised_forces(prob, pots)
        for pot in pots:
            _, ids, _ = row_records(prob, pot, R)
            for e in range(len(ids)):
                if not ids[e, 3] & 1:
                    for s in (0, 1):
                        if ids[e, s] >= 0:
                            count[fi, ids[e, s]] += 1
        for b in range(R.n):
            rv, rw = 3 * (R.v_row0 + b), 3 * (R.w_row0 + b)
            fv, fw = f[rv:rv + 3], f[rw:rw + 3]
            a = 0.5 * prob.dt * w1[b]
            tau = wrench_map(a, fw)
            t1 = t0[b] + prob.dt * v1[b]
            out[fi, b] = np.r_[fv, tau, tau + np.cross(t1 - about, fv), fw, t1, np.linalg.norm(a)]
            mags[fi, b, 0], mags[fi, b, 1] = mag[rv:rv + 3], mag[rw:rw + 3]
            nterms[fi, b] = n[rv], n[rw]
    return out, count, mags, nterms


def torque_bound(a_norm, mag_w):
    """The header's bound per torque component: 64 * 2^-53 * (1 + |a| + |a|^2) * sum_k |g_k| / dt."""
    return 64 * U * (1.0 + a_norm + a_norm * a_norm) * mag_w


# ---- the virtual-work reference --------------------------------------------------------------------------------------------------------------
def rotated_w1(w1, dt, theta):
    """w1' with R1(w1') = exp([theta]x) R1(w1): the quaternion (1, a) multiplied from the left by the rotation's, then the inverse Cayley map."""
    a = 0.5 * dt * np.asarray(w1, dtype=np.float64)
    ang = np.linalg.norm(theta)
    if ang == 0.0:
        return np.array(w1, dtype=np.float64)
    c, s = np.cos(0.5 * ang), np.sin(0.5 * ang) * np.asarray(theta) / ang
    pw = c - np.dot(s, a)
    pv = c * a + s + np.cross(s, a)
    return 2.0 * (pv / pw) / dt


def fd_usable(pot):
    return not any(pot.name.startswith(x) for x in FD_EXCLUDED)


def energy_of(prob, pots):
    E, mag = 0.0, 0.0
    for pot in pots:
        o = ev.evaluate_potential(prob, pot)
        if o is not None:
            E += float(np.sum(o.E))
            mag += float(np.abs(o.E).sum())
    return E, mag


def fd_wrench(prob, pots, body, h_rot=2e-5, h_pos=2e-6, R=None):
    """(F, tau, bound_F, bound_tau) on one body from the listed potentials by central differences of the oracle's energy in the body's translation and
    world-frame rotation. The bounds are the estimated error of the differences (module docstring)."""
    R = R or Rigid(prob)
    v1, w1 = prob.arrays[R.v1].reshape(-1, 3), prob.arrays[R.w1].reshape(-1, 3)

    def E_at(dx, theta):
        v, w = v1.copy(), w1.copy()
        v[body] = v1[body] + np.asarray(dx) / prob.dt
        w[body] = rotated_w1(w1[body], prob.dt, np.asarray(theta))
        return energy_of(with_arrays(prob, **{str(R.v1): v, str(R.w1): w}), pots)

    def diff(make, h):
        out, bound = np.zeros(3), np.zeros(3)
        for i in range(3):
            d = np.zeros(3)
            d[i] = 1.0
            (Ep, mp), (Em, mm) = E_at(*make(h * d)), E_at(*make(-h * d))
            (Ep2, _), (Em2, _) = E_at(*make(2 * h * d)), E_at(*make(-2 * h * d))
            D1, D2 = (Ep - Em) / (2 * h), (Ep2 - Em2) / (4 * h)
            out[i] = -(D1 - (D2 - D1) / 3.0)
            bound[i] = abs(D2 - D1) / 3.0 + 8 * U * (mp + mm) / h
        return out, bound

    F, bF = diff(lambda d: (d, np.zeros(3)), h_pos)
    tau, bT = diff(lambda d: (np.zeros(3), d), h_rot)
    return F, tau, bF, bT


# ---- shared by the GPU tests and tools/wrench_report_cost.py ---------------------------------------------------------------------------------
def controller_torque(name, f, tau, da, rel, a, dt):
    """The torque on body a of the two velocity controllers, derived by hand from E = dt phi(da1 . rel - target), da1 = R1a da_loc turning with body a. With
    s = phi', a world-frame rotation dtheta of body a at fixed DoFs of the others changes da1 by dtheta x da1: dE = dt s dtheta . (da1 x rel), a torque
    dt rel x (s da1). rb_constraint_linear_velocity (rel = vb1 - va1; the constraint report's force f = s da1, its torque slots zero) has only that.
    rb_constraint_angular_velocity (rel = wb1 - wa1; the report's torque slots T = s da1 are the generalised force on wa1 with the pose held) also reads
    wa1 itself, and the torque the solver balances against that part is the map of it: (I + [a]x + a a^T) T + dt rel x T. Arguments per row; da, rel:
    the report's anchor slots."""
    if name == "rb_constraint_linear_velocity":
        return dt * np.cross(rel, f)
    return tau + np.cross(a, tau) + a * (a * tau).sum(axis=1)[:, None] + dt * np.cross(rel, tau)


def engine_of(prob, man, R):
    """An engine holding the problem and the array ids of the bodies' state as the wrench accessors take them."""
    from gpu_util import engine_from_problem

    eng = engine_from_problem(prob, man)
    ids = dict(v1=eng.array_ids[(R.v1, 3)], w1=eng.array_ids[(R.w1, 3)], t0=eng.array_ids[(R.t0, 3)], q0=eng.array_ids[(R.q0, 4)], n_bodies=R.n)
    return eng, ids


def star_problem(n_att, n_bodies):
    """Body 0 attached to n_att deformable points through EnergyAttachments_rb_d (one row per point), every further body to 37 points, the bodies' rows
    interleaved; with the rigid-body inertia potentials, which bind the time step. DoF sets in the engine's order: soft.v1, rigid.v1, rigid.w1."""
    rng = np.random.default_rng(4000 + n_att + n_bodies)
    dt = 0.01
    att = np.concatenate([np.zeros(n_att, dtype=np.int64)] + [np.full(37, b, dtype=np.int64) for b in range(1, n_bodies)])
    att = att[rng.permutation(len(att))]
    n = len(att)
    B = cr.Builder(dt)
    x0, v1 = rng.random((n, 3)), rng.standard_normal((n, 3))
    bv, bw, bt, bq = cr._bodies(rng, n_bodies, dt)
    s, sv, sw = B.dof_set(v1), B.dof_set(bv), B.dof_set(bw)
    a_x0, a_k = B.array(x0, 3), B.array(10.0 ** (2.0 + 2.0 * rng.random(2)), 1)
    a_t, a_q, a_loc = B.array(bt, 3), B.array(bq, 4), B.array(0.2 * rng.standard_normal((n, 3)), 3)
    B.bind(a_k, 1, 1)
    B.bind_dt()
    B.bind(B.sets[s], 3, 3, s)
    B.bind(a_x0, 3, 3)
    B.bind(a_loc, 3, 0)
    B.bind(B.sets[sv], 3, 2, sv)
    B.bind(B.sets[sw], 3, 2, sw)
    B.bind(a_t, 3, 2)
    B.bind(a_q, 4, 2)
    attach = B.bindings
    conn = np.stack([np.arange(n), rng.integers(0, 2, n), att, np.arange(n)], axis=1)
    B.bindings = []
    nb = n_bodies
    for a in (None, rng.standard_normal((nb, 3)), np.zeros((nb, 3)), rng.standard_normal((nb, 3))):   # v1*, v0, a, force
        if a is None:
            B.bind(B.sets[sv], 3, 0, sv)
        else:
            B.bind(B.array(a, 3), 3, 0)
    for a in (1.0 + rng.random(nb), np.zeros(nb), np.zeros(nb)):   # mass, linear damping, is_quasistatic
        B.bind(B.array(a, 1), 1, 0)
    B.bind_dt()
    B.bind(B.array(np.array([[0.0, 0.0, -9.81]]), 3), 3, -1)
    linear = B.bindings
    prob = B.problem("EnergyAttachments_rb_d", conn, False)
    prob.potentials[0].bindings = attach
    prob.potentials.append(ev.PotentialDesc("EnergyRigidBodyInertia_Linear", np.arange(nb, dtype=np.int32).reshape(-1, 1), linear, False))
    R = Rigid(prob, v1=prob.dof_arrays[sv], w1=prob.dof_arrays[sw])
    return prob, R, att


# ---- the host mirror's scene and its balance measure ---------------------------------------------------------------------------------------------
MIRROR_FAMILIES = ("EnergyRigidBodyInertia_Linear", "EnergyRigidBodyInertia_Angular", "rb_constraint_", "EnergyAttachments_rb_", "contact_rb_", "friction_rb_")


def rbchain_scene(S):
    """The rbchain scene of tests/test_gpu_scene.py (9 boxes, all 13 rigid-body potentials) through the host mirror; the bodies are labelled box0..box8."""
    st = S.default_settings()
    st.init_frictional_contact = 0
    sim = S.Simulation(st)
    sim.rb_set_default_constraint_params(stiffness=1e4)
    axis = np.array([1.0, 0.5, -0.3])
    axis /= np.linalg.norm(axis)
    n = [0]

    def box(x, y, zz):
        b = sim.add_rigid_box("box%d" % n[0], 1.0 + 0.1 * x, (0.1, 0.12, 0.08))
        n[0] += 1
        sim.rb_set_translation(b, (x, y, zz))
        sim.rb_add_rotation(b, 20.0 * x + 5.0, axis)
        return b

    def unit(v):
        v = np.asarray(v, dtype=float)
        return v / np.linalg.norm(v)

    b0 = box(0.0, 0.0, 0.0)
    sim.rb_add_constraint("fix", b0)
    b1 = box(0.15, 0.0, 0.0)
    sim.rb_add_constraint("point", b0, b1, (0.07, 0.02, 0.01))
    b2 = box(0.30, 0.02, 0.0)
    sim.rb_add_constraint("point_on_axis", b1, b2, (0.22, 0.0, 0.01), unit((1.0, 0.2, 0.0)))
    b3 = box(0.45, 0.0, 0.03)
    sim.rb_add_constraint("distance", b2, b3, (0.33, 0.0, 0.0), (0.42, 0.01, 0.02))
    b4 = box(0.60, 0.0, 0.0)
    sim.rb_add_constraint("distance_limits", b3, b4, (0.48, 0.0, 0.0), (0.57, 0.0, 0.0), 0.08995, 0.09005)
    sim.rb_add_constraint("direction", b3, b4, unit((0.0, 1.0, 0.2)))
    b5 = box(0.75, 0.0, 0.0)
    sim.rb_add_constraint("point", b4, b5, (0.67, 0.0, 0.0))
    sim.rb_add_constraint("angle_limit", b4, b5, (1.0, 0.0, 0.0), 0.5)
    b6 = box(0.90, 0.0, 0.0)
    sim.rb_add_constraint("spring", b5, b6, (0.78, 0.0, 0.0), (0.87, 0.01, 0.0), 200.0, 3.0)
    b7 = box(1.05, 0.0, 0.0)
    sim.rb_add_constraint("point_on_axis", b6, b7, (0.97, 0.0, 0.0), (1.0, 0.0, 0.0))
    sim.rb_add_constraint("linear_velocity", b6, b7, (1.0, 0.0, 0.0), 0.3, 5.0, 0.05)
    b8 = box(1.20, 0.0, 0.0)
    sim.rb_add_constraint("hinge", b7, b8, (1.12, 0.0, 0.0), (0.0, 1.0, 0.0))
    sim.rb_add_constraint("angular_velocity", b7, b8, (0.0, 1.0, 0.0), 1.0, 2.0, 0.1)
    return sim


def balance(records):
    """How far the bodies are from balance in a body report [7, n_bodies, 16] of the host mirror's families (six sources, then all): per body the
    unbalanced |F| over the sum of the six families' |F|, likewise for tau_com -> (per_body [n_bodies, 2], scene [2]); scene: the largest unbalanced
    magnitude of a body over the largest load sum of a body."""
    res = np.stack([np.linalg.norm(records[6, :, 0:3], axis=1), np.linalg.norm(records[6, :, 3:6], axis=1)], axis=1)
    load = np.stack([np.linalg.norm(records[:6, :, 0:3], axis=2).sum(axis=0), np.linalg.norm(records[:6, :, 3:6], axis=2).sum(axis=0)], axis=1)
    return res / load, res.max(axis=0) / load.max(axis=0)


def reference_balance(path):
    """balance() of the reference's own converged state: the trajectory fixture's arrays are those of its first call of run_one_step, the state the last
    evaluation point of that call (the reference's Newton loop converged there; the call was then redone with hardened constraints), evaluated by the
    oracle restatement."""
    import json

    prob, _, z = ev.load_fixture(path)
    traj = json.loads(bytes(z["traj_json"]).decode())
    last = np.nonzero(np.array(traj["iter_step"]) == 0)[0][-1]
    prob.set_dofs(z["iterates"][last])
    names = [p.name for p in prob.potentials]
    fams = [[k for k, nm in enumerate(names) if nm.startswith(pre) and len(prob.potentials[k].conn)] for pre in MIRROR_FAMILIES]
    R = Rigid(prob)
    rec = np.zeros((7, R.n, 16))
    for f, fam in enumerate(fams):
        if fam:
            rec[f] = body_records(prob, [fam], (0.0, 0.0, 0.0), R)[0][0]
    rec[6] = body_records(prob, [[]], (0.0, 0.0, 0.0), R)[0][0]
    return balance(rec)
