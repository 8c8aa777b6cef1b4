"""Reference of the bending report (include/mistark.h "bending report"; record layout: stark_amd/csrc/bending_report.hpp), in numpy, and the hinges,
meshes and states its tests share.

Two derivations of the same records:
  (A) `records(prob, pot, threshold)`: a direct restatement of the record's formulas.
  (B) `from_oracle(prob, pot)`: the element energy oracle.evaluator.evaluate_potential has proven against the reference (fields 9 + 10 must add up to it),
      and the moment from its gradient: turning node 3 about the hinge by d alpha moves it by d alpha e0_hat x (x3 - x0) and the signed fold angle phi by
      d alpha, so dE/dphi = g_x3 . (e0_hat x (x3 - x0)) with g_x = g_v / dt.
        complete: E depends on the state through theta1 = acos((1 - 1e-12) cos phi) alone, so M = dE/dtheta1 = dE/dphi * sin(theta1) / ((1 - 1e-12) sin phi)
        flat:     on a rigid fold of the rest stencil M is dE/dtheta with theta = |phi|: M = sign(phi) dE/dphi (only there; a stretched stencil has no such
                  identity, which is why the golden flat fixture is not held to (B) for field 8)
      Both pass through 1 / sin: the oracle's derivative of acos is -1 / sqrt(1 - c^2), whose relative error is 2.2e-16 / sin^2(theta1). `moment_bound`
      carries that, and leaves out hinges where it says nothing (sin^2 < 1e-9: the folds 0, 1e-9, 1e-5 and pi).

Bounds of the comparison with another evaluation of (A)'s formulas (`bounds`), all absolute:
  everything that does not pass through acos: 1e-11 * the largest |reference value| of the field over the potential (the suite's element tolerance). phi1 and
      the hinge normal are formed from unit vectors, quantities of size 1 whatever the fold: their scale is at least 1 (as stress_ref takes the Green strain's).
      phi1 is an angle: +pi and -pi are the same fold, the difference is taken on the circle. The flat kind's s = sum K_i x1_i is what is left of terms of
      the size of the positions: where a field made of it (6, 8, 9) has cancelled below 1e-11 of its own terms over the whole potential (a table of flat
      hinges only), the terms are the scale, as stress_ref.rel_to_scale has it.
  theta1: 1e-11 + 16 * 2.2e-16 / sin(theta_ref) per hinge: the conditioning of acos times a rounding budget of 16 ulp for cross products, normalisation,
      the dot product and the 1 - 1e-12 factor.
  fields computed from theta1 (3; the complete kind's 6, 8, 9, 10; the flat kind's 8, whose formula holds cos(theta1 / 2)): that bound (and theta0's, where
      theta0 enters) propagated linearly through the formula, plus the 1e-11 term.
  hinge normal: (n0_hat + n1_hat) / |n0_hat + n1_hat| divides by 2 cos(phi / 2): 1e-11 + 16 * 2.2e-16 / |n0_hat + n1_hat|_ref. (The record writes zeros
      below 1e-8; the seeded folds have 0.14 at the least or 1e-16 at the most, so the term never reaches 3e-14 here.)
"""
import functools
import os

import numpy as np

import stress_ref as sr
from oracle import evaluator as ev

KIND = {"EnergyDiscreteShells": 0, "EnergyBendingFlat": 1}
NAMES = list(KIND)
EPS = 2.2e-16
ELEMENT_TOL = 1e-11
CLAMP = 1.0 - 1e-12
NO_NORMAL = 1e-8
FOLDS = (0.0, 1e-9, 1e-5, 0.1, 1.0, 3.0, np.pi)
DT = 0.01
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FIXTURES = {"EnergyDiscreteShells": "cloth_shells_6.npz", "EnergyBendingFlat": "cloth_flat_6.npz"}


def _norm(v):
    return np.sqrt((v * v).sum(axis=-1))


def _stencil(x):
    """x [n, 4, 3] -> dict of the hinge geometry; unit vectors are NaN-free zeros where the stencil is degenerate."""
    e0 = x[:, 1] - x[:, 0]
    n0 = np.cross(e0, x[:, 2] - x[:, 0])
    n1 = -np.cross(e0, x[:, 3] - x[:, 0])
    l, nn0, nn1 = _norm(e0), _norm(n0), _norm(n1)
    deg = ~((l > 0.0) & (nn0 > 0.0) & (nn1 > 0.0))
    safe = lambda v, n: v * (1.0 / np.where(deg, 1.0, n))[:, None]
    h0, h1, eh = safe(n0, nn0), safe(n1, nn1), safe(e0, l)
    c = CLAMP * (h0 * h1).sum(axis=1)
    theta = np.where(deg, 0.0, np.arccos(np.clip(c, -1.0, 1.0)))
    phi = np.where(deg, 0.0, np.arctan2((eh * np.cross(h0, h1)).sum(axis=1), (h0 * h1).sum(axis=1)))
    return dict(l=l, deg=deg, h0=h0, h1=h1, eh=eh, theta=theta, phi=phi)


def states(prob, pot):
    """(x0 [n, 4, 3], x1 [n, 4, 3], dt, the gathered bindings)."""
    b = sr.gather(prob, pot)
    dt = float(b[-1][0, 0])
    v1 = np.stack(b[0:4], axis=1)
    x0 = np.stack(b[4:8], axis=1)
    return x0, x0 + dt * v1, dt, b


def groups_of(pot):
    """The group of every row: the connectivity entry the stiffness is read with (0 for a global stiffness)."""
    col = pot.bindings[12 if KIND[pot.name] == 0 else 10].conn
    return pot.conn[:, col].astype(np.int64) if col >= 0 else np.zeros(pot.conn.shape[0], dtype=np.int64)


def theta_bound(theta):
    with np.errstate(divide="ignore"):
        return ELEMENT_TOL + 16.0 * EPS / np.abs(np.sin(theta))


def records(prob, pot, threshold=None):
    """(A): (rec [n, 16], bound [n, 16]: the absolute bound of every entry, see the module's docstring). threshold: per group or None."""
    kind = KIND[pot.name]
    x0, x1, dt, b = states(prob, pot)
    n = len(x0)
    s1, s0 = _stencil(x1), _stencil(x0)
    deg = s1["deg"]
    t1 = s1["theta"]
    t0 = np.where(s0["deg"] | deg, 0.0, s0["theta"])
    tb1 = np.where(deg, 0.0, theta_bound(t1))
    tb0 = np.where(s0["deg"] | deg, 0.0, theta_bound(t0))
    rec, lin = np.zeros((n, 16)), np.zeros((n, 16))   # lin: the part of the bound that comes through theta
    rec[:, 0], lin[:, 0] = t1, tb1
    rec[:, 1] = s1["phi"]
    rec[:, 3] = np.where(s0["deg"] | deg, 0.0, (t1 - t0) / dt)
    lin[:, 3] = (tb1 + tb0) / dt
    rec[:, 4] = s1["l"]
    m = s1["h0"] + s1["h1"]
    nm = _norm(m)
    has_normal = ~deg & (nm >= NO_NORMAL)
    rec[:, 11:14] = np.where(has_normal[:, None], m / np.where(has_normal, nm, 1.0)[:, None], 0.0)
    lin[:, 11:14] = np.where(has_normal, 16.0 * EPS / np.where(has_normal, nm, 1.0), 0.0)[:, None]
    if kind == 0:
        rest, rest_len, rest_h, scale, k, damping = (b[i][:, 0] for i in range(8, 14))
        ratio = (rest_len * scale) / (rest_h * scale)
        dd = t1 - rest
        rec[:, 2] = rest
        rec[:, 5] = scale * scale * rest_len * rest_h
        rec[:, 6] = np.where(deg, 0.0, t1 / (3.0 * scale * rest_h))
        lin[:, 6] = tb1 / (3.0 * scale * rest_h)
        rec[:, 7] = rest / (3.0 * scale * rest_h)
        rec[:, 8] = np.where(deg, 0.0, ratio * (2.0 * k * dd + (damping / dt) * (t1 - t0)))
        lin[:, 8] = ratio * (2.0 * k * tb1 + (damping / dt) * (tb1 + tb0))
        rec[:, 9] = np.where(deg, 0.0, k * (dd * dd) * ratio)
        lin[:, 9] = np.abs(2.0 * k * dd * ratio) * tb1
        rec[:, 10] = np.where(deg, 0.0, (damping / dt) * (0.5 * t1 * t1 - t0 * t1) * ratio)
        lin[:, 10] = (damping / dt) * ratio * (np.abs(t1 - t0) * tb1 + np.abs(t1) * tb0)
    else:
        K, coef, k = b[8], b[9][:, 0], b[10][:, 0]
        s = (K[:, :, None] * x1).sum(axis=1)
        ss = (s * s).sum(axis=1)
        ns = np.sqrt(ss)
        rec[:, 5] = 1.0 / (2.0 * coef)
        rec[:, 6] = ns / (3.0 * rec[:, 5])
        rec[:, 8] = np.where(deg, 0.0, k * coef * ns * s1["l"] * np.cos(0.5 * t1))
        lin[:, 8] = k * coef * ns * s1["l"] * 0.5 * np.abs(np.sin(0.5 * t1)) * tb1
        rec[:, 9] = (0.5 * k * coef) * ss
        # s is what is left of terms K_i x1_i of the size of the positions: where a field has cancelled below the tolerance of its own terms over the
        # whole potential (a table of flat hinges), the terms are the scale (stress_ref.rel_to_scale's rule)
        ts = (np.abs(K)[:, :, None] * np.abs(x1)).sum(axis=1)
        ts = np.sqrt((ts * ts).sum(axis=1))
        terms = {6: ts / (3.0 * rec[:, 5]), 8: k * coef * ts * s1["l"], 9: (0.5 * k * coef) * ts * ts}
    g = groups_of(pot)
    rec[:, 14] = g
    dev = deviation(rec)
    beyond = np.zeros(n, dtype=bool) if threshold is None else (~deg & (dev > np.asarray(threshold, dtype=np.float64)[g]))
    rec[:, 15] = 1.0 * deg + 2.0 * beyond
    scale_f = np.abs(rec).max(axis=0) if n else np.zeros(16)
    scale_f[[1, 11, 12, 13]] = np.maximum(scale_f[[1, 11, 12, 13]], 1.0)
    if kind == 1 and n:
        for f, t in terms.items():
            if scale_f[f] < ELEMENT_TOL * t.max():
                scale_f[f] = t.max()
    bound = lin + ELEMENT_TOL * scale_f[None, :]
    bound[:, 0] = tb1
    bound[deg] = 0.0                                  # what a degenerate hinge writes is exact (zeros, or products of the inputs alone)
    bound[np.ix_(deg, [4, 5, 6, 7, 9])] = ELEMENT_TOL * scale_f[None, [4, 5, 6, 7, 9]]
    bound[:, [14, 15]] = 0.0
    return rec, bound


def deviation(rec):
    """|theta1 - rest| of every row, 0 for a degenerate one."""
    return np.where(rec[:, 15].astype(np.int64) & 1, 0.0, np.abs(rec[:, 0] - rec[:, 2]))


def undecided(rec, bound, threshold):
    """Rows whose |theta1 - rest| lies within the theta1 bound of their group's threshold: the arithmetic does not decide their flag 2."""
    g = rec[:, 14].astype(np.int64)
    return np.abs(deviation(rec) - np.asarray(threshold, dtype=np.float64)[g]) <= bound[:, 0]


def check_records(got, rec, bound, what, threshold=None):
    """The comparison the GPU tests use too: got [n, 16] against (A) within (A)'s bounds."""
    assert got.shape == rec.shape and np.isfinite(got).all(), what
    for f in range(14):
        d = np.abs(got[:, f] - rec[:, f])
        if f == 1:
            d = np.minimum(d, 2.0 * np.pi - d)
        worst = (d / np.maximum(bound[:, f], 1e-300)).max() if len(d) else 0.0
        print("%s field %d: worst error / bound %.3g" % (what, f, worst))
        assert (d <= bound[:, f]).all(), (what, f, worst)
    assert np.array_equal(got[:, 14], rec[:, 14]), what
    gf, rf = got[:, 15].astype(np.int64), rec[:, 15].astype(np.int64)
    assert np.array_equal(gf & 1, rf & 1), what
    if threshold is None:
        assert np.array_equal(gf, rf), what
    else:
        out = undecided(rec, bound, threshold)
        assert out.sum() <= 0.02 * len(rec), (what, out.sum())
        assert np.array_equal(gf[~out], rf[~out]), what


def from_oracle(prob, pot):
    """(B): (E [n] the oracle's element energies, M [n] the moment from its gradient, bound [n] relative to max|M|, NaN where (B) says nothing)."""
    x0, x1, dt, b = states(prob, pot)
    o = ev.evaluate_potential(prob, pot)
    assert o.active.all()
    s1 = _stencil(x1)
    g3 = o.g.reshape(len(x1), 4, 3)[:, 3] / dt
    dE = (g3 * np.cross(s1["eh"], x1[:, 3] - x1[:, 0])).sum(axis=1)
    sin2 = np.sin(s1["theta"]) ** 2
    ok = ~s1["deg"] & (sin2 >= 1e-9)
    with np.errstate(divide="ignore", invalid="ignore"):
        if KIND[pot.name] == 0:
            M = dE * np.sin(s1["theta"]) / (CLAMP * np.sin(s1["phi"]))
        else:
            M = np.sign(s1["phi"]) * dE
        bound = np.where(ok, ELEMENT_TOL + 16.0 * EPS / sin2, np.nan)
    return o.E, np.where(ok, M, np.nan), bound


# ---- nodal and group stages -----------------------------------------------------------------------------------------------------------------
def block_rows(prob, pot):
    """[n, 2]: the block rows of the two edge endpoints."""
    return sr.block_rows(prob, pot)[:, :2]


def nodal(n_rows, parts):
    """(out [n_rows, 6], mag [n_rows, 6]) over parts = [(rows [n, 2], rec [n, 16]), ...] in the order of the device's sorted keys: potential, endpoint, row.
    mag: the sum of |terms| of each entry (divided by the weight sum like the entry itself; the maximum and the count are exact)."""
    num, mag = np.zeros((n_rows, 6)), np.zeros((n_rows, 6))
    for rows, rec in parts:
        w = 0.5 * rec[:, 5]
        val = np.stack([w * rec[:, 6], w * (rec[:, 6] - rec[:, 7]), 0.5 * (rec[:, 9] + rec[:, 10]), np.zeros(len(rec)), np.ones(len(rec)), w], axis=1)
        dev = deviation(rec)
        for k in range(2):
            np.add.at(num, rows[:, k], val)
            np.add.at(mag, rows[:, k], np.abs(val))
            np.maximum.at(num[:, 3], rows[:, k], dev)
    w = num[:, 5].copy()
    ws = np.where(w > 0.0, w, 1.0)
    num[:, :2] /= ws[:, None]
    mag[:, :2] /= ws[:, None]
    mag[:, 3:5] = 0.0
    return num, mag


def group_records(rec, n_groups):
    """(out [n_groups, 10], mag [n_groups, 10]) of rows rec [n, 16]: the sums in table order; maximum, arg-max and counts are exact (mag 0)."""
    out, mag = np.zeros((n_groups, 10)), np.zeros((n_groups, 10))
    g = rec[:, 14].astype(np.int64)
    flags = rec[:, 15].astype(np.int64)
    dev = deviation(rec)
    dk = rec[:, 6] - rec[:, 7]
    for q in range(n_groups):
        sel = np.nonzero(g == q)[0]
        if len(sel) == 0:
            out[q, 4] = -1.0
            continue
        a = rec[sel, 5]
        out[q, 0] = len(sel)
        out[q, 1] = (flags[sel] & 1).sum()
        out[q, 2] = ((flags[sel] >> 1) & 1).sum()
        out[q, 3] = dev[sel].max()
        out[q, 4] = np.argmax(dev[sel])               # (the first position attaining the maximum)
        terms = np.stack([rec[sel, 9], rec[sel, 10], a, a * dk[sel] ** 2, a * np.abs(dk[sel])], axis=1)
        out[q, 5:10] = terms.sum(axis=0)
        mag[q, 5:10] = np.abs(terms).sum(axis=0)
        out[q, 9] /= out[q, 7]
        mag[q, 9] /= out[q, 7]
    return out, mag


# ---- rest data, problems ----------------------------------------------------------------------------------------------------------------------
def hinge_rest_data(X, hinges):
    """What EnergyDiscreteShells::add (stark_amd/csrc/host/sim.cpp) tabulates per hinge from the rest positions: dict(rest_angle, rest_len, rest_h, K
    [n, 4], coef)."""
    x = X[hinges]
    e0, e1, e2 = x[:, 1] - x[:, 0], x[:, 2] - x[:, 0], x[:, 3] - x[:, 0]
    e3, e4 = x[:, 2] - x[:, 1], x[:, 3] - x[:, 1]
    l = _norm(e0)
    n0, n1 = np.cross(e0, e1), -np.cross(e0, e2)
    nn0, nn1 = _norm(n0), _norm(n1)
    rest_angle = np.arccos(CLAMP * ((n0 / nn0[:, None]) * (n1 / nn1[:, None])).sum(axis=1))
    A0, A1 = 0.5 * nn0, 0.5 * nn1
    cot = lambda v, w: (v * w).sum(axis=1) / _norm(np.cross(v, w))
    c01, c02, c03, c04 = cot(e0, e1), cot(e0, e2), cot(-e0, e3), cot(-e0, e4)
    return dict(rest_angle=rest_angle, rest_len=l, rest_h=(2.0 * A0 / l + 2.0 * A1 / l) / 6.0, coef=3.0 / (A0 + A1) * 0.5,
                K=np.stack([c03 + c04, c01 + c02, -c01 - c03, -c02 - c04], axis=1))


def make_problem(parts, x0, v1, dt=DT):
    """An oracle Problem with one DoF set (the nodes' velocities) and one potential per part = (name, hinges [n, 4], group [n], rest data dict, group
    parameters dict of per-group lists). Connectivity rows: hinge index, group, the four nodes, as the host mirror registers them."""
    arrays = [np.array(v1, dtype=np.float64), np.array(x0, dtype=np.float64)]
    pots = []

    def add(values, stride, col):
        arrays.append(np.ascontiguousarray(values, dtype=np.float64).reshape(-1, stride))
        return ev.Binding(len(arrays) - 1, stride, col, -1)

    for name, hinges, group, rest, gp in parts:
        n = len(hinges)
        conn = np.concatenate([np.arange(n)[:, None], np.asarray(group).reshape(n, 1), hinges], axis=1).astype(np.int32)
        bs = [ev.Binding(0, 3, 2 + a, 0) for a in range(4)] + [ev.Binding(1, 3, 2 + a, -1) for a in range(4)]
        if KIND[name] == 0:
            bs += [add(rest["rest_angle"], 1, 0), add(rest["rest_len"], 1, 0), add(rest["rest_h"], 1, 0), add(gp["scale"], 1, 1), add(gp["k"], 1, 1), add(gp["damping"], 1, 1)]
        else:
            bs += [add(rest["K"], 4, 0), add(rest["coef"], 1, 0), add(gp["k"], 1, 1)]
        bs.append(add([dt], 1, -1))
        pots.append(ev.PotentialDesc(name, np.ascontiguousarray(conn), bs))
    nd = 3 * len(x0)
    return ev.Problem(dt=dt, ndofs=nd, dof_offsets=[0], dof_sizes=[nd], arrays=arrays, potentials=pots, dof_arrays={0: 0})


GROUP_PARAMS = {"EnergyDiscreteShells": dict(scale=[1.0, 1.3], k=[2e-3, 5e-4], damping=[1e-4, 3e-5]), "EnergyBendingFlat": dict(k=[2e-3, 5e-4])}


def random_rotations(rng, n):
    q = rng.normal(size=(n, 4))
    q /= _norm(q)[:, None]
    w, x, y, z = q.T
    return np.stack([np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)], axis=1),
                     np.stack([2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)], axis=1),
                     np.stack([2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], axis=1)], axis=1)


def fold(l, h1, h2, a2, a3, angle):
    """[n, 4, 3]: hinge (0,0,0)-(l,0,0), node 2 at height h1 on one side, node 3 at height h2 on the other, turned about the hinge by `angle` (signed)."""
    z = np.zeros_like(l)
    return np.stack([np.stack([z, z, z], axis=1), np.stack([l, z, z], axis=1), np.stack([a2, h1, z], axis=1),
                     np.stack([a3, -h2 * np.cos(angle), -h2 * np.sin(angle)], axis=1)], axis=1)


@functools.lru_cache(maxsize=None)
def seeded_hinges(name, per_fold=20, seed=1):
    """Hinges of their own four nodes each at the fold angles FOLDS, both fold directions, under random rotations and translations: every x1 is a rigid
    fold of its rest stencil. Even hinges rest (x0 = x1), odd ones arrive from a slightly different x0. Two groups. Returns (prob, rec, bound, extra) with
    (A) evaluated once without thresholds; extra: dict(angle [n] signed, l, h1, h2, k [n], mirror_of [n]: the hinge folded the other way)."""
    rng = np.random.default_rng(seed)
    n_half = len(FOLDS) * per_fold
    l, h1, h2 = rng.uniform(0.05, 0.3, n_half), rng.uniform(0.03, 0.2, n_half), rng.uniform(0.03, 0.2, n_half)
    a2, a3 = l * rng.uniform(-0.3, 1.3, n_half), l * rng.uniform(-0.3, 1.3, n_half)
    ang = np.repeat(np.array(FOLDS), per_fold)
    R, t = random_rotations(rng, n_half), rng.uniform(-1.0, 1.0, (n_half, 3))
    noise = 1e-3 * l[:, None, None] * rng.uniform(-1.0, 1.0, (n_half, 4, 3))
    noise[0::2] = 0.0
    rest_fold = np.where(np.arange(n_half) % 3 == 0, 0.0, rng.uniform(0.0, 0.5, n_half))
    dup = lambda a: np.concatenate([a, a])
    l, h1, h2, a2, a3, R, t, rest_fold = (dup(a) for a in (l, h1, h2, a2, a3, R, t, rest_fold))
    angle = np.concatenate([ang, -ang])
    noise = np.concatenate([noise, noise * np.array([1.0, 1.0, -1.0])])   # the second half is the mirror image of the first, at both states
    n = 2 * n_half
    flat = fold(l, h1, h2, a2, a3, np.zeros(n))
    move = lambda x: np.einsum("nij,naj->nai", R, x) + t[:, None, :]
    x1 = move(fold(l, h1, h2, a2, a3, angle))
    x0 = move(fold(l, h1, h2, a2, a3, angle) + noise)
    v1 = (x1 - x0) / DT
    v1[0::2] = 0.0
    x0[0::2] = x1[0::2]
    hinges = np.arange(4 * n).reshape(n, 4)
    rest = hinge_rest_data(flat.reshape(-1, 3), hinges)
    if KIND[name] == 0:   # rest angles: flat for a third, folded for the others (the deviation then has both signs)
        rest["rest_angle"] = np.where(rest_fold == 0.0, rest["rest_angle"], rest_fold)
    group = (np.arange(n) % n_half % 5 == 0).astype(np.int64)
    prob = make_problem([(name, hinges, group, rest, GROUP_PARAMS[name])], x0.reshape(-1, 3), v1.reshape(-1, 3))
    rec, bound = records(prob, prob.potentials[0])
    for a in (rec, bound):
        a.setflags(write=False)
    extra = dict(angle=angle, l=l, h1=h1, h2=h2, k=np.asarray(GROUP_PARAMS[name]["k"])[group], mirror_of=(np.arange(n) + n_half) % n)
    return prob, rec, bound, extra


@functools.lru_cache(maxsize=None)
def golden_problem(name):
    """(prob, pot, rec, bound) of the bending potential of the golden cloth fixture of the kind."""
    prob, man, z = ev.load_fixture(os.path.join(GOLDEN, FIXTURES[name]))
    (pot,) = [p for p in prob.potentials if p.name == name]
    rec, bound = records(prob, pot)
    return prob, pot, rec, bound


def find_hinges(tris):
    """[n, 4]: for every edge two triangles share, (edge node, edge node, opposite node of the first triangle, of the second), in the order the edges are
    first met."""
    seen, out = {}, []
    for t in tris:
        for a in range(3):
            u, v, w = int(t[a]), int(t[(a + 1) % 3]), int(t[(a + 2) % 3])
            key = (min(u, v), max(u, v))
            if key in seen:
                p, q, r = seen[key]
                out.append([p, q, r, w])
            else:
                seen[key] = (u, v, w)
    return np.array(out, dtype=np.int64)


def cloth(name, n, seed=3, small_group=40):
    """An n x n grid cloth (rest: flat, spacing 0.1 / n * 8) bent into a wavy state with noise: (prob, hinges). The last `small_group` hinges are of group
    1, the others of group 0."""
    rng = np.random.default_rng(seed)
    X, tris = sr.tri_grid(n, n, 0.8 / n)
    hinges = find_hinges(tris)
    h = 0.8 / n
    wave = lambda P: np.stack([P[:, 0], P[:, 1], 0.05 * np.sin(7.0 * P[:, 0]) * np.cos(5.0 * P[:, 1])], axis=1)
    x1 = wave(X) + 0.02 * h * rng.uniform(-1.0, 1.0, X.shape)
    x0 = x1 + 0.01 * h * rng.uniform(-1.0, 1.0, X.shape)
    group = np.zeros(len(hinges), dtype=np.int64)
    group[len(hinges) - small_group:] = 1
    prob = make_problem([(name, hinges, group, hinge_rest_data(X, hinges), GROUP_PARAMS[name])], x0, (x1 - x0) / DT)
    return prob, hinges


def fan(n, winding=7):
    """A closed fan of n triangles (0, 1 + i, 1 + (i + 1) % n) about vertex 0, the ring winding `winding` times around it (triangles may overlap in space:
    nothing collides), and the n hinges between neighbours: (X [n + 1, 3], hinges [n, 4]); every hinge has the centre as edge endpoint 0."""
    i = np.arange(n)
    a = 2.0 * np.pi * winding * i / n
    X = np.concatenate([[[0.0, 0.0, 0.0]], np.stack([0.1 * np.cos(a), 0.1 * np.sin(a), 0.01 * np.sin(1.3 * i)], axis=1)])
    hinges = np.stack([np.zeros(n, dtype=np.int64), 1 + i, 1 + (i - 1) % n, 1 + (i + 1) % n], axis=1)
    return X, hinges
