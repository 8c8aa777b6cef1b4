"""numpy restatement of the constraint report (include/mistark.h "constraint report", stark_amd/csrc/constraint_report.hpp): the 16-slot row records of the
seventeen penalty-constraint potentials and the 12-slot group records, written from oracle/energies.py (the energies, whose derivatives by hand are the
forces and torques) and from the record layout; plus the seeded problems the CPU and GPU tests share.

Row record: 0 violation | 1 reaction | 2..4 force on side a | 5..7 torque on side a | 8..10 anchor / direction of a | 11..13 of b, or the target |
14 energy | 15 flags (+1 active, +2 beyond tolerance, +4 out of range); aux[2]: the damped spring's damper (velocity, force).
Group record: 0 rows | 1 active | 2 beyond tolerance | 3 largest |violation| | 4 position in the group's list of the first row attaining it (-1: none) |
5..7 sum of 2..4 | 8..10 moment about `about` | 11 energy sum.

Error bounds (none tuned on the code under test):
  rows   1e-11 relative to max |reference| of the field over the table (the element-quantity tolerance of tests/test_stress_cpu.py); the angle-valued
         slot 0 of the angle limits adds 4 * 2^-53 / c rad: acos(1 - c^2 / 2) amplifies the rounding of its argument by 1 / sin(angle) ~ 1 / c
  sums   (n + 8) * 2^-53 * sum |terms| (tests/budget_ref.py): a sum of n terms in any order and tree, each term carrying a few roundings of its own"""
import math

import numpy as np

from oracle import evaluator as ev

U = 2.0 ** -53
REC, GROUP_REC = 16, 12
ROW_TOL = 1e-11
EPS = 100.0 * 2.220446049250313e-16
N_ROWS = 300
DT = 0.01

# name: (kind code, group column, first block of side a, of side b, direction-type, unit, translational blocks of side a, of side b)
KINDS = {
    "EnergyPrescribedPositions": (0, 2, 0, -1, False, "m", [0], []),
    "rb_constraint_global_points": (1, 0, 0, -1, False, "m", [0], []),
    "rb_constraint_global_directions": (2, 0, 0, -1, True, "deg", [], []),
    "rb_constraint_points": (3, 0, 0, 1, False, "m", [0], [1]),
    "rb_constraint_point_on_axis": (4, 0, 0, 1, False, "m", [0], [1]),
    "rb_constraint_distances": (5, 0, 0, 1, False, "m", [0], [1]),
    "rb_constraint_distance_limits": (6, 0, 0, 1, False, "m", [0], [1]),
    "rb_constraint_directions": (7, 0, 0, 1, True, "deg", [], []),
    "rb_constraint_angle_limits": (8, 0, 0, 1, True, "deg", [], []),
    "rb_constraint_damped_spring": (9, 0, 0, 1, False, "m", [0], [1]),
    "rb_constraint_linear_velocity": (10, 0, 0, 1, True, "m/s", [0], [1]),
    "rb_constraint_angular_velocity": (11, 0, 0, 1, True, "deg/s", [], []),
    "EnergyAttachments_d_d_p_p": (12, 0, 0, 1, False, "m", [0], [1]),
    "EnergyAttachments_d_d_p_e": (13, 1, 0, 1, False, "m", [0], [1, 2]),
    "EnergyAttachments_d_d_p_t": (14, 1, 0, 1, False, "m", [0], [1, 2, 3]),
    "EnergyAttachments_d_d_e_e": (15, 1, 0, 2, False, "m", [0, 1], [2, 3]),
    "EnergyAttachments_rb_d": (16, 1, 1, 0, False, "m", [1], [0]),
}
NAMES = sorted(KINDS, key=lambda n: KINDS[n][0])


# ---- kinematics (oracle/energies.py _R1, _rb_x1, _rb_d1 on arrays of rows) ---------------------------------------------------------------------
def rot1(q0, w, dt):
    """R(q1) [n, 3, 3], q1 = normalize(q0 + dt/2 (0, w) q0), (w, x, y, z) storage."""
    e, f, g, h = q0.T
    wx, wy, wz = w.T
    p = np.stack([-(wx * f) - wy * g - wz * h, wx * e + wy * h - wz * g, -(wx * h) + wy * e + wz * f, wx * g - wy * f + wz * e], axis=1)
    q = q0 + (0.5 * dt)[:, None] * p
    q = q / np.sqrt((q * q).sum(axis=1))[:, None]
    return quat_R(q)


def quat_R(q):
    w, x, y, z = q.T
    R = np.empty((len(q), 3, 3))
    R[:, 0, 0], R[:, 0, 1], R[:, 0, 2] = 1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)
    R[:, 1, 0], R[:, 1, 1], R[:, 1, 2] = 2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)
    R[:, 2, 0], R[:, 2, 1], R[:, 2, 2] = 2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)
    return R


def mv(R, x):
    return np.einsum("nij,nj->ni", R, x)


def nrm(x):
    return np.sqrt((x * x).sum(axis=1))


def body(v1, w1, t0, q0, dt):
    """(t1, R1) of the rows' bodies."""
    return t0 + dt[:, None] * v1, rot1(q0, w1, dt)


def split(inp, strides):
    out, o = [], 0
    for s in strides:
        out.append(inp[:, o] if s == 1 else inp[:, o:o + s])
        o += s
    assert o == inp.shape[1]
    return out


# ---- the row records -------------------------------------------------------------------------------------------------------------------------------
def _blank(n):
    z3 = np.zeros((n, 3))
    return dict(viol=np.zeros(n), react=np.zeros(n), f=z3.copy(), tau=z3.copy(), pa=z3.copy(), pb=z3.copy(), E=np.zeros(n), active=np.ones(n, dtype=bool),
                oor=np.zeros(n, dtype=bool), aux=np.zeros((n, 2)))


def _spring(r, a, b, k):
    d = b - a
    r["viol"] = nrm(d)
    r["react"] = k * r["viol"]
    r["f"] = k[:, None] * d
    r["pa"], r["pb"] = a, b
    r["E"] = 0.5 * k * (d * d).sum(axis=1)


def _axial(r, a, b, length, C, k, t1a):
    with np.errstate(divide="ignore", invalid="ignore"):
        s = np.where(length > 0.0, k * C / length, 0.0)
    r["viol"], r["react"] = C, -k * C
    r["f"] = s[:, None] * (b - a)
    r["tau"] = np.cross(a - t1a, r["f"])
    r["pa"], r["pb"] = a, b


def _direction_deg(r, C):
    r["oor"] = C > 1.0
    with np.errstate(invalid="ignore"):
        r["viol"] = np.where(r["oor"], 90.0, np.degrees(np.arcsin(np.minimum(C, 1.0))))


def _controller(dv, fmax, delay):
    left, mid = dv < -delay, (dv >= -delay) & (dv < delay)
    react = np.where(left, -fmax, np.where(mid, -(fmax / delay) * dv, fmax))
    s = np.where(left, -fmax, np.where(mid, (fmax / delay) * dv, fmax))
    eps = delay / 2.0
    E_over_dt = np.where(left, -fmax * (dv - eps), np.where(mid, 0.5 * (fmax / delay) * dv * dv, fmax * (dv - eps)))
    return react, s, E_over_dt


def row_fields(name, inp):
    """The fields of every row of `inp` [n, gathered inputs of the potential in binding order] before the inactive rows are zeroed."""
    n = len(inp)
    r = _blank(n)
    B13 = (3, 3, 3, 4)
    if name == "EnergyPrescribedPositions":
        v1, x0, target, k, dt = split(inp, (3, 3, 3, 1, 1))
        _spring(r, x0 + dt[:, None] * v1, target, k)
    elif name == "EnergyAttachments_d_d_p_p":
        va, vb, xa, xb, k, dt = split(inp, (3, 3, 3, 3, 1, 1))
        _spring(r, xa + dt[:, None] * va, xb + dt[:, None] * vb, k)
    elif name == "EnergyAttachments_d_d_p_e":
        vp, v0, v1, xp, x0, x1, w, k, dt = split(inp, (3, 3, 3, 3, 3, 3, 2, 1, 1))
        h = dt[:, None]
        _spring(r, xp + h * vp, w[:, :1] * (x0 + h * v0) + w[:, 1:2] * (x1 + h * v1), k)
    elif name == "EnergyAttachments_d_d_p_t":
        vp, v0, v1, v2, xp, x0, x1, x2, w, k, dt = split(inp, (3,) * 8 + (3, 1, 1))
        h = dt[:, None]
        _spring(r, xp + h * vp, w[:, :1] * (x0 + h * v0) + w[:, 1:2] * (x1 + h * v1) + w[:, 2:3] * (x2 + h * v2), k)
    elif name == "EnergyAttachments_d_d_e_e":
        v0, v1, v2, v3, x0, x1, x2, x3, wa, wb, k, dt = split(inp, (3,) * 8 + (2, 2, 1, 1))
        h = dt[:, None]
        _spring(r, wa[:, :1] * (x0 + h * v0) + wa[:, 1:2] * (x1 + h * v1), wb[:, :1] * (x2 + h * v2) + wb[:, 1:2] * (x3 + h * v3), k)
    elif name == "EnergyAttachments_rb_d":
        k, dt, vd, xd, loc, v1, w1, t0, q0 = split(inp, (1, 1, 3, 3, 3) + B13)
        t1, R = body(v1, w1, t0, q0, dt)
        a = t1 + mv(R, loc)
        _spring(r, a, xd + dt[:, None] * vd, k)
        r["tau"] = np.cross(a - t1, r["f"])
    elif name == "rb_constraint_global_points":
        loc, target, k, act, dt, v1, w1, t0, q0 = split(inp, (3, 3, 1, 1, 1) + B13)
        t1, R = body(v1, w1, t0, q0, dt)
        a = t1 + mv(R, loc)
        _spring(r, a, target, k)
        r["tau"] = np.cross(a - t1, r["f"])
        r["active"] = act > 0.5
    elif name == "rb_constraint_points":
        la, lb, k, act, dt, va, wa, ta, qa, vb, wb, tb, qb = split(inp, (3, 3, 1, 1, 1) + B13 + B13)
        t1a, Ra = body(va, wa, ta, qa, dt)
        t1b, Rb = body(vb, wb, tb, qb, dt)
        a = t1a + mv(Ra, la)
        _spring(r, a, t1b + mv(Rb, lb), k)
        r["tau"] = np.cross(a - t1a, r["f"])
        r["active"] = act > 0.5
    elif name == "rb_constraint_point_on_axis":
        la, lda, lb, k, act, dt, va, wa, ta, qa, vb, wb, tb, qb = split(inp, (3, 3, 3, 1, 1, 1) + B13 + B13)
        t1a, Ra = body(va, wa, ta, qa, dt)
        t1b, Rb = body(vb, wb, tb, qb, dt)
        a, da, b = t1a + mv(Ra, la), mv(Ra, lda), t1b + mv(Rb, lb)
        ap = b - a
        s = (ap * da).sum(axis=1) / (da * da).sum(axis=1)
        nv = ap - s[:, None] * da          # the part of b - a across the axis
        e = (ap * da).sum(axis=1)
        D2 = (ap * ap).sum(axis=1) - e * e / (da * da).sum(axis=1)
        r["viol"] = np.sqrt(D2)
        r["react"] = k * r["viol"]
        r["f"] = k[:, None] * nv
        r["tau"] = np.cross(a - t1a, r["f"])
        r["pa"], r["pb"] = a, b
        r["E"] = 0.5 * k * D2
        r["active"] = act > 0.5
    elif name in ("rb_constraint_distances", "rb_constraint_distance_limits", "rb_constraint_damped_spring"):
        ns = {"rb_constraint_distances": 1, "rb_constraint_distance_limits": 2, "rb_constraint_damped_spring": 3}[name]
        parts = split(inp, (3, 3) + (1,) * ns + (1, 1, 1) + B13 + B13) if name != "rb_constraint_damped_spring" else split(inp, (3, 3, 1, 1, 1, 1, 1) + B13 + B13)
        la, lb = parts[0], parts[1]
        va, wa, ta, qa, vb, wb, tb, qb = parts[-8:]
        dt, act = parts[-9], parts[-10]
        t1a, Ra = body(va, wa, ta, qa, dt)
        t1b, Rb = body(vb, wb, tb, qb, dt)
        a, b = t1a + mv(Ra, la), t1b + mv(Rb, lb)
        l = nrm(b - a)
        if name == "rb_constraint_distances":
            target, k = parts[2], parts[3]
            _axial(r, a, b, l, l - target, k, t1a)
            r["E"] = 0.5 * k * (target - l) ** 2
            r["active"] = act > 0.5
        elif name == "rb_constraint_distance_limits":
            dmin, dmax, k = parts[2], parts[3], parts[4]
            C = np.where(l < dmin, l - dmin, np.where(l > dmax, l - dmax, 0.0))
            _axial(r, a, b, l, C, k, t1a)
            r["E"] = 0.5 * k * C * C
            r["active"] = (act > 0.5) & ((l < dmin) | (l > dmax))
        else:
            rest, k, damping = parts[2], parts[3], parts[4]
            l0 = nrm((tb + mv(quat_R(qb), lb)) - (ta + mv(quat_R(qa), la)))
            _axial(r, a, b, l, l - rest, k, t1a)
            u = (b - a) / l[:, None]
            fd = (damping * (l - l0) / (dt * dt))[:, None] * u
            r["f"] = r["f"] + fd
            r["tau"] = r["tau"] + np.cross(a - t1a, fd)
            vel_a, vel_b = va + np.cross(wa, a - t1a), vb + np.cross(wb, b - t1b)
            dv = ((vel_b - vel_a) * u).sum(axis=1)
            r["aux"] = np.stack([dv, -damping * dv], axis=1)
            r["E"] = 0.5 * k * (l - rest) ** 2 + 0.5 * damping * ((l - l0) / dt) ** 2
            r["active"] = act > 0.5
            assert (l > 0.0).all()   # (coincident ends are the out-of-range case the seeded problems do not contain)
    elif name == "rb_constraint_global_directions":
        dl, target, k, act, dt, w1, q0 = split(inp, (3, 3, 1, 1, 1, 3, 4))
        d = mv(rot1(q0, w1, dt), dl)
        u = d - target
        C = nrm(u)
        _direction_deg(r, C)
        r["react"] = nrm(np.cross(target, (-k * C / (C + EPS))[:, None] * u))
        r["tau"] = -np.cross(d, k[:, None] * u)
        r["pa"], r["pb"] = d, target
        r["E"] = 0.5 * k * C * C
        r["active"] = act > 0.5
    elif name in ("rb_constraint_directions", "rb_constraint_angle_limits"):
        if name == "rb_constraint_directions":
            la, lb, k, act, dt, wa, qa, wb, qb = split(inp, (3, 3, 1, 1, 1, 3, 4, 3, 4))
        else:
            la, lb, maxd, k, act, dt, wa, qa, wb, qb = split(inp, (3, 3, 1, 1, 1, 1, 3, 4, 3, 4))
        da, db = mv(rot1(qa, wa, dt), la), mv(rot1(qb, wb, dt), lb)
        u = db - da
        C = nrm(u)
        r["pa"], r["pb"] = da, db
        if name == "rb_constraint_directions":
            _direction_deg(r, C)
            r["react"] = nrm(np.cross(da, (k * C / (C + EPS))[:, None] * u))
            r["tau"] = np.cross(da, k[:, None] * u)
            r["E"] = 0.5 * k * C * C
            r["active"] = act > 0.5
        else:
            engaged = C > maxd
            c = np.where(engaged, C - maxd, 0.0)
            r["viol"] = np.where(engaged, np.degrees(np.arccos((2.0 - c * c) / 2.0)), 0.0)
            r["react"] = np.where(engaged, nrm(np.cross(da, (k * c * c / (C + EPS))[:, None] * u)), 0.0)
            r["tau"] = np.where(engaged[:, None], np.cross(da, (k * c * c / C)[:, None] * u), 0.0)
            r["E"] = k * c ** 3 / 3.0
            r["active"] = (act > 0.5) & engaged
    elif name == "rb_constraint_linear_velocity":
        dl, target, fmax, delay, act, va, vb, wa, qa, dt = split(inp, (3, 1, 1, 1, 1, 3, 3, 3, 4, 1))
        da = mv(rot1(qa, wa, dt), dl)
        rel = vb - va
        r["viol"] = (da * rel).sum(axis=1) - target
        r["react"], s, E_dt = _controller(r["viol"], fmax, delay)
        r["f"] = s[:, None] * da
        r["pa"], r["pb"] = da, rel
        r["E"] = E_dt * dt
        r["active"] = act > 0.5
    elif name == "rb_constraint_angular_velocity":
        dl, target, fmax, delay, act, wa, wb, qa, dt = split(inp, (3, 1, 1, 1, 1, 3, 3, 4, 1))
        da = mv(rot1(qa, wa, dt), dl)
        rel = wb - wa
        dv = (da * rel).sum(axis=1) - target
        r["react"], s, E_dt = _controller(dv, fmax, delay)
        r["viol"] = np.degrees(dv)
        r["tau"] = s[:, None] * da
        r["pa"], r["pb"] = da, rel
        r["E"] = E_dt * dt
        r["active"] = act > 0.5
    else:
        raise KeyError(name)
    return r


def row_records(name, inp, tolerance=None):
    """(rec [n, 16], aux [n, 2]); tolerance: per row, None or negative entries: none."""
    r = row_fields(name, np.asarray(inp, dtype=np.float64))
    n = len(inp)
    on = r["active"]
    rec = np.zeros((n, REC))
    rec[:, 0] = r["viol"]
    rec[:, 1] = np.where(on, r["react"], 0.0)
    rec[:, 2:5] = np.where(on[:, None], r["f"], 0.0)
    rec[:, 5:8] = np.where(on[:, None], r["tau"], 0.0)
    rec[:, 8:11], rec[:, 11:14] = r["pa"], r["pb"]
    rec[:, 14] = np.where(on, r["E"], 0.0)
    tol = np.full(n, -1.0) if tolerance is None else np.asarray(tolerance, dtype=np.float64)
    rec[:, 15] = on + 2.0 * ((tol >= 0.0) & (np.abs(r["viol"]) > tol)) + 4.0 * r["oor"]
    return rec, r["aux"]


def row_bounds(name, inp, rec):
    """The admissible |difference| per entry of the records [n, 16]."""
    b = np.broadcast_to(ROW_TOL * np.abs(rec).max(axis=0), rec.shape).copy()
    if name == "rb_constraint_angle_limits":
        la, lb, maxd, k, act, dt, wa, qa, wb, qb = split(np.asarray(inp), (3, 3, 1, 1, 1, 1, 3, 4, 3, 4))
        C = nrm(mv(rot1(qb, wb, dt), lb) - mv(rot1(qa, wa, dt), la))
        c = np.where(C > maxd, C - maxd, np.inf)
        b[:, 0] += np.degrees(4.0 * U / c)
    b[:, 15] = 0.0
    return b


# ---- the group records ---------------------------------------------------------------------------------------------------------------------------
def sum_terms(terms):
    flat = np.asarray(terms, dtype=np.float64).ravel()
    return math.fsum(flat.tolist()), math.fsum(np.abs(flat).tolist())


def group_terms(rec, about, dir_type):
    """The terms of the summed slots 5..11 of the group record: a list of 7 arrays [n, terms per row]."""
    f = rec[:, 2:5]
    t = [f[:, k][:, None] for k in range(3)]
    if dir_type:
        t += [rec[:, 5 + k][:, None] for k in range(3)]
    else:
        rr = rec[:, 8:11] - np.asarray(about, dtype=np.float64)
        for a, b, c in ((0, 1, 2), (1, 2, 0), (2, 0, 1)):
            t.append(np.stack([rr[:, b] * f[:, c], -(rr[:, c] * f[:, b])], axis=1))
    t.append(rec[:, 14][:, None])
    return t


def group_records(rec, group, n_groups, about, dir_type):
    """(grec [n_groups, 12], S_abs [n_groups, 12]) of row records rec [n, 16], row i in group group[i]; S_abs is 0 for the exact slots 0..4."""
    group = np.asarray(group).reshape(-1)
    terms = group_terms(rec, about, dir_type)
    flags = rec[:, 15].astype(np.int64)
    out, mag = np.zeros((n_groups, GROUP_REC)), np.zeros((n_groups, GROUP_REC))
    for g in range(n_groups):
        sel = np.flatnonzero(group == g)
        out[g, 0], out[g, 1], out[g, 2] = len(sel), (flags[sel] & 1).sum(), ((flags[sel] >> 1) & 1).sum()
        if len(sel):
            v = np.abs(rec[sel, 0])
            out[g, 3], out[g, 4] = v.max(), int(np.argmax(v))   # (argmax: the first occurrence)
        else:
            out[g, 4] = -1.0
        for k in range(7):
            out[g, 5 + k], mag[g, 5 + k] = sum_terms(terms[k][sel])
    return out, mag


def assert_exact_family(rec, group, n_groups, about, dir_type=False):
    """The exact family's claim for the group sums: every term the device forms from the row records is a dyadic rational it represents exactly, and
    every partial sum of a group's terms in any order fits 53 bits. Checked in 64-bit integer arithmetic on the records themselves at the scale 2^20
    (2^40 for products): the lever arm and each product of the moment must equal their exact values, and the terms of a slot, stripped of the trailing
    zero bits they share, must sum in absolute value below 2^53."""
    def ints(a, bits):
        a = np.asarray(a, dtype=np.float64) * 2.0 ** bits   # (a power of two: exact)
        assert (a == np.rint(a)).all() and (np.abs(a) < 2.0 ** 62).all(), "a value is finer than the scale or too large"
        return a.astype(np.int64)

    group = np.asarray(group).reshape(-1)
    terms = group_terms(rec, about, dir_type)
    if not dir_type:
        F = ints(rec[:, 2:5], 20)
        R = ints(rec[:, 8:11], 20) - ints(about, 20)
        assert np.array_equal(ints(rec[:, 8:11] - np.asarray(about, dtype=np.float64), 20), R), "a lever arm is not exact in double"
        assert (np.abs(R) < 2 ** 28).all() and (np.abs(F) < 2 ** 30).all()
        for j, (a, b, c) in enumerate(((0, 1, 2), (1, 2, 0), (2, 0, 1))):
            assert np.array_equal(ints(terms[3 + j][:, 0], 40), R[:, b] * F[:, c]), ("a product is not exact in double", j)
            assert np.array_equal(ints(terms[3 + j][:, 1], 40), -(R[:, c] * F[:, b])), ("a product is not exact in double", j)
    for k, t in enumerate(terms):
        if not (t != 0.0).any():
            continue
        v = ints(t, 40)
        low = int(np.bitwise_or.reduce(np.abs(v).ravel()))
        shift = (low & -low).bit_length() - 1   # trailing zero bits all terms share
        for g in range(n_groups):
            assert int(np.abs(v[group == g] >> shift).sum()) < 2 ** 53, ("partial sums may round", g, k)


# ---- problems ----------------------------------------------------------------------------------------------------------------------------------
class Builder:
    """An oracle Problem with one potential, DoF sets in the engine's registration order (soft.v1, rb.v1, rb.w1)."""
    def __init__(self, dt):
        self.arrays, self.sets, self.dt = [np.array([[float(dt)]])], [], float(dt)
        self.bindings = []

    def array(self, a, stride):
        self.arrays.append(np.ascontiguousarray(a, dtype=np.float64).reshape(-1, stride))
        return len(self.arrays) - 1

    def dof_set(self, a):
        self.sets.append(self.array(a, 3))
        return len(self.sets) - 1

    def bind(self, array, stride, col, dof_set=-1):
        self.bindings.append(ev.Binding(array, stride, col, dof_set))

    def bind_dt(self):
        self.bind(0, 1, -1)

    def problem(self, name, conn, has_condition):
        sizes = [self.arrays[a].size for a in self.sets]
        offsets = [int(sum(sizes[:s])) for s in range(len(sizes))]
        pot = ev.PotentialDesc(name, np.ascontiguousarray(conn, dtype=np.int32), self.bindings, has_condition)
        return ev.Problem(dt=self.dt, ndofs=int(sum(sizes)), dof_offsets=offsets, dof_sizes=sizes, arrays=self.arrays, potentials=[pot],
                          dof_arrays={s: a for s, a in enumerate(self.sets)})


def gather(prob, pot=None):
    """in [n, gathered inputs] of a potential in binding order (what the engine's gather_inputs hands the row function)."""
    pot = prob.potentials[0] if pot is None else pot
    n = len(pot.conn)
    cols = []
    for b in pot.bindings:
        data = prob.arrays[b.array].reshape(-1, b.stride)
        cols.append(data[pot.conn[:, b.conn]] if b.conn >= 0 else np.broadcast_to(data[0], (n, b.stride)))
    return np.ascontiguousarray(np.concatenate(cols, axis=1))


def ids_of(prob, name, pot=None):
    """ids [n, 4]: group, kind code, block row of side a's first DoF block, of side b's or -1."""
    pot = prob.potentials[0] if pot is None else pot
    code, gcol, ba, bb = KINDS[name][:4]
    order = ev.dof_layout(pot)
    row = lambda k: prob.dof_offsets[pot.bindings[order[k]].dof_set] // 3 + pot.conn[:, pot.bindings[order[k]].conn]
    n = len(pot.conn)
    return np.stack([pot.conn[:, gcol], np.full(n, code), row(ba), row(bb) if bb >= 0 else np.full(n, -1)], axis=1).astype(np.int32)


def prescribed_problem(x0, v1, points, target, k, group, dt):
    """EnergyPrescribedPositions: row i prescribes point points[i] to target[i] with the stiffness of group[i]; conn {idx, point, group}."""
    B = Builder(dt)
    s = B.dof_set(v1)
    a_x0, a_t, a_k = B.array(x0, 3), B.array(target, 3), B.array(k, 1)
    B.bind(B.sets[s], 3, 1, s)
    B.bind(a_x0, 3, 1)
    B.bind(a_t, 3, 0)
    B.bind(a_k, 1, 2)
    B.bind_dt()
    n = len(points)
    return B.problem("EnergyPrescribedPositions", np.stack([np.arange(n), points, group], axis=1), False)


def attach_pp_problem(x0, v1, pa, pb, k, group, dt):
    """EnergyAttachments_d_d_p_p: row i ties point pa[i] to point pb[i] with the stiffness of group[i]; conn {group, a, b}."""
    B = Builder(dt)
    s = B.dof_set(v1)
    a_x0, a_k = B.array(x0, 3), B.array(k, 1)
    for col in (1, 2):
        B.bind(B.sets[s], 3, col, s)
    for col in (1, 2):
        B.bind(a_x0, 3, col)
    B.bind(a_k, 1, 0)
    B.bind_dt()
    return B.problem("EnergyAttachments_d_d_p_p", np.stack([group, pa, pb], axis=1), False)


def _unit(v):
    return v / nrm(v)[:, None]


def _rotated(d, rng, max_chord):
    """Unit vectors at a chord distance uniformly in (0.02, max_chord) of the unit vectors d."""
    n = len(d)
    chord = 0.02 + (max_chord - 0.02) * rng.random(n)
    ang = 2.0 * np.arcsin(chord / 2.0)
    p = _unit(np.cross(d, rng.standard_normal((n, 3))))
    return np.cos(ang)[:, None] * d + np.sin(ang)[:, None] * p


def _branches(masks, values_and_thresholds):
    """Every branch is taken by some rows and not by others; no row lies within relative 1e-9 of a branch threshold."""
    for m in masks:
        assert m.any() and not m.all(), "a branch is not exercised"
    for v, t in values_and_thresholds:
        assert (np.abs(v - t) > 1e-9 * np.maximum(np.abs(v), np.abs(t))).all(), "a row lies on a branch threshold"


_CACHE = {}


def seeded_problem(name):
    """The seeded problem of a kind: an oracle Problem with one potential of N_ROWS rows (random anchors, bodies with |w1| dt up to 0.3, random
    stiffness), and the per-group tolerances [n_groups] the tests pass (half of the rows beyond them)."""
    if name in _CACHE:
        return _CACHE[name]
    code = KINDS[name][0]
    rng = np.random.default_rng(1000 + code)
    n, dt = N_ROWS, DT
    B = Builder(dt)
    h = np.full(n, dt)
    if name.startswith("Energy"):   # deformable points (and, for rb_d, bodies)
        npts = 500
        x0, v1 = rng.random((npts, 3)), rng.standard_normal((npts, 3))
        ng = 5
        k = 10.0 ** (2.0 + 3.0 * rng.random(ng))
        group = rng.integers(0, ng, n)
        s = B.dof_set(v1)
        a_x0, a_k = B.array(x0, 3), B.array(k, 1)
        pts = np.stack([rng.permutation(npts)[:4] for _ in range(n)])
        idx = np.arange(n)
        if name == "EnergyPrescribedPositions":
            x1 = x0[pts[:, 0]] + dt * v1[pts[:, 0]]
            target = x1 + 10.0 ** (-4.0 + 3.0 * rng.random((n, 1))) * rng.standard_normal((n, 3))
            prob = prescribed_problem(x0, v1, pts[:, 0], target, k, group, dt)
        elif name == "EnergyAttachments_d_d_p_p":
            prob = attach_pp_problem(x0, v1, pts[:, 0], pts[:, 1], k, group, dt)
        elif name == "EnergyAttachments_rb_d":
            nb = 40
            bv, bw, bt, bq = _bodies(rng, nb, dt)
            sv, sw = B.dof_set(bv), B.dof_set(bw)
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
            prob = B.problem(name, np.stack([idx, group, rng.integers(0, nb, n), pts[:, 0]], axis=1), False)
        else:
            nn = {"EnergyAttachments_d_d_p_e": 3, "EnergyAttachments_d_d_p_t": 4, "EnergyAttachments_d_d_e_e": 4}[name]
            for c in range(nn):
                B.bind(B.sets[s], 3, 2 + c, s)
            for c in range(nn):
                B.bind(a_x0, 3, 2 + c)
            def bary(m):
                w = 0.1 + rng.random((n, m))
                return w / w.sum(axis=1)[:, None]
            if name == "EnergyAttachments_d_d_p_e":
                B.bind(B.array(bary(2), 2), 2, 0)
            elif name == "EnergyAttachments_d_d_p_t":
                B.bind(B.array(bary(3), 3), 3, 0)
            else:
                B.bind(B.array(bary(2), 2), 2, 0)
                B.bind(B.array(bary(2), 2), 2, 0)
            B.bind(a_k, 1, 1)
            B.bind_dt()
            prob = B.problem(name, np.concatenate([idx[:, None], group[:, None], pts[:, :nn]], axis=1), False)
        n_groups = ng
    else:
        nb = 40
        bv, bw, bt, bq = _bodies(rng, nb, dt)
        sv, sw = B.dof_set(bv), B.dof_set(bw)
        a_t, a_q = B.array(bt, 3), B.array(bq, 4)
        ia = rng.integers(0, nb, n)
        ib = (ia + 1 + rng.integers(0, nb - 1, n)) % nb
        idx = np.arange(n)
        k = 10.0 ** (2.0 + 3.0 * rng.random(n))
        act = (rng.random(n) < 0.8).astype(np.float64)
        Ra, Rb = rot1(bq[ia], bw[ia], h), rot1(bq[ib], bw[ib], h)
        t1a, t1b = bt[ia] + dt * bv[ia], bt[ib] + dt * bv[ib]
        vec = lambda a: B.bind(B.array(a, 3), 3, 0)
        sca = lambda a: B.bind(B.array(a, 1), 1, 0)

        def x1(col):
            B.bind(B.sets[sv], 3, col, sv)
            B.bind(B.sets[sw], 3, col, sw)
            B.bind(a_t, 3, col)
            B.bind(a_q, 4, col)

        def d1(col):
            B.bind(B.sets[sw], 3, col, sw)
            B.bind(a_q, 4, col)

        la, lb = 0.2 * rng.standard_normal((n, 3)), 0.2 * rng.standard_normal((n, 3))
        pa, pb = t1a + mv(Ra, la), t1b + mv(Rb, lb)
        l = nrm(pb - pa)
        masks, thresholds = [act > 0.5], []
        two = True
        if name == "rb_constraint_global_points":
            vec(la); vec(pa + 10.0 ** (-4.0 + 3.0 * rng.random((n, 1))) * rng.standard_normal((n, 3))); sca(k); sca(act); B.bind_dt(); x1(1)
            two = False
        elif name == "rb_constraint_global_directions":
            target = _unit(rng.standard_normal((n, 3)))
            d = _rotated(target, rng, 0.9)
            vec(np.einsum("nji,nj->ni", Ra, d)); vec(target); sca(k); sca(act); B.bind_dt(); d1(1)
            two = False
        elif name == "rb_constraint_points":
            vec(la); vec(lb); sca(k); sca(act); B.bind_dt(); x1(1); x1(2)
        elif name == "rb_constraint_point_on_axis":
            vec(la); vec(_unit(rng.standard_normal((n, 3)))); vec(lb); sca(k); sca(act); B.bind_dt(); x1(1); x1(2)
        elif name == "rb_constraint_distances":
            vec(la); vec(lb); sca(l * (0.5 + rng.random(n))); sca(k); sca(act); B.bind_dt(); x1(1); x1(2)
        elif name == "rb_constraint_distance_limits":
            branch = rng.integers(0, 3, n)   # 0: below the minimum, 1: above the maximum, 2: inside
            dmin = np.where(branch == 0, l * (1.05 + rng.random(n)), l * (0.2 + 0.7 * rng.random(n)))
            dmax = np.where(branch == 1, l * (0.95 - 0.04 * rng.random(n)), np.maximum(dmin, l) * (1.05 + rng.random(n)))
            dmin = np.minimum(dmin, np.where(branch == 1, 0.9 * dmax, dmin))
            vec(la); vec(lb); sca(dmin); sca(dmax); sca(k); sca(act); B.bind_dt(); x1(1); x1(2)
            masks += [l < dmin, l > dmax, (l >= dmin) & (l <= dmax)]
            thresholds += [(l, dmin), (l, dmax)]
        elif name in ("rb_constraint_directions", "rb_constraint_angle_limits"):
            da = _unit(rng.standard_normal((n, 3)))
            if name == "rb_constraint_directions":
                db = _rotated(da, rng, 0.9)
                vec(np.einsum("nji,nj->ni", Ra, da)); vec(np.einsum("nji,nj->ni", Rb, db)); sca(k); sca(act); B.bind_dt(); d1(1); d1(2)
            else:
                db = _rotated(da, rng, 1.4)
                C = nrm(db - da)
                engaged = rng.random(n) < 0.6
                c = np.minimum(10.0 ** (-2.0 + 2.0 * rng.random(n)), 0.95 * C)   # opening distances in [1e-2, 1]
                engaged &= c >= 1e-2
                maxd = np.where(engaged, C - c, C * (1.1 + rng.random(n)))
                vec(np.einsum("nji,nj->ni", Ra, da)); vec(np.einsum("nji,nj->ni", Rb, db)); sca(maxd); sca(k); sca(act); B.bind_dt(); d1(1); d1(2)
                masks += [engaged]
                thresholds += [(C, maxd)]
        elif name == "rb_constraint_damped_spring":
            vec(la); vec(lb); sca(l * (0.5 + rng.random(n))); sca(k); sca(10.0 ** (-1.0 + 2.0 * rng.random(n))); sca(act); B.bind_dt(); x1(1); x1(2)
        else:
            lin = name == "rb_constraint_linear_velocity"
            dl = _unit(rng.standard_normal((n, 3)))
            rel = (bv[ib] - bv[ia]) if lin else (bw[ib] - bw[ia])
            v = (mv(Ra, dl) * rel).sum(axis=1)
            delay = 0.05 + 0.2 * rng.random(n)
            regime = rng.integers(0, 3, n)   # 0: below -delay, 1: inside, 2: above +delay
            dv = np.where(regime == 0, -delay * (1.1 + rng.random(n)), np.where(regime == 1, delay * (1.8 * rng.random(n) - 0.9), delay * (1.1 + rng.random(n))))
            vec(dl); sca(v - dv); sca(1.0 + 9.0 * rng.random(n)); sca(delay); sca(act)
            if lin:
                B.bind(B.sets[sv], 3, 1, sv); B.bind(B.sets[sv], 3, 2, sv); B.bind(B.sets[sw], 3, 1, sw); B.bind(a_q, 4, 1)
            else:
                B.bind(B.sets[sw], 3, 1, sw); B.bind(B.sets[sw], 3, 2, sw); B.bind(a_q, 4, 1)
            B.bind_dt()
            masks += [dv < -delay, np.abs(dv) < delay, dv >= delay]
            thresholds += [(dv, -delay), (dv, delay)]
        _branches(masks, thresholds)
        conn = np.stack([idx, ia, ib], axis=1) if two else np.stack([idx, ia], axis=1)
        prob = B.problem(name, conn, True)
        n_groups = n
    # tolerances: per group the median |violation| of the group's rows (about half of the rows beyond it), placed between two distinct violations
    rec, _ = row_records(name, gather(prob))
    g = prob.potentials[0].conn[:, KINDS[name][1]]
    tol = np.zeros(n_groups)
    for q in range(n_groups):
        v = np.sort(np.abs(rec[g == q, 0]))
        tol[q] = 0.5 * v[0] if len(v) == 1 else (0.5 * (v[len(v) // 2 - 1] + v[len(v) // 2]) if len(v) else 1.0)
    if n_groups == n:   # every row its own group: half of them beyond
        tol = np.where(np.arange(n) % 2 == 0, 0.5 * np.abs(rec[:, 0]), 2.0 * np.abs(rec[:, 0]) + 1e-6)
    _CACHE[name] = (prob, tol)
    return _CACHE[name]


def _bodies(rng, nb, dt):
    """v1, w1 (|w1| dt up to 0.3), t0, q0 of nb bodies."""
    q = _unit4(rng.standard_normal((nb, 4)))
    w = _unit(rng.standard_normal((nb, 3))) * (0.3 / dt) * rng.random((nb, 1))
    return rng.standard_normal((nb, 3)), w, 2.0 * rng.random((nb, 3)) - 1.0, q


def _unit4(q):
    return q / np.sqrt((q * q).sum(axis=1))[:, None]


def dyadic_point_springs(rng, group, n_points_extra=0):
    """The exact family for EnergyPrescribedPositions and EnergyAttachments_d_d_p_p: x0 and v1 of point a integer / 64, dt = 1 / 8, offsets d = b - a
    integer multiples of a Pythagorean triple / 64 (so |d| is exact), stiffness a power of two per group. Returns dict(x0a, v1a, d, k, dt)."""
    n = len(group)
    triples = np.array([[3, 4, 0], [0, 3, 4], [4, 0, 3], [1, 2, 2], [2, 1, 2], [2, 3, 6], [6, 2, 3], [0, 0, 1]], dtype=np.float64)
    d = triples[rng.integers(0, len(triples), n)] * rng.integers(1, 4, n)[:, None] * rng.choice([-1.0, 1.0], (n, 3)) / 64.0
    ng = int(np.max(group)) + 1 if n else 1
    return dict(x0a=rng.integers(-31, 32, (n, 3)) / 64.0, v1a=rng.integers(-31, 32, (n, 3)) / 64.0, d=d, k=2.0 ** rng.integers(0, 6, ng), dt=0.125)
