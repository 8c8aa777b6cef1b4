"""numpy restatement of the budget readout (include/mistark.h "budget readout", stark_amd/csrc/budget.hpp): the 13-slot records of point items and of
rigid bodies, and per-potential energy sums. Every sum is math.fsum over explicitly listed terms, and comes with S_abs = sum |terms|: a sum of n terms
taken in ANY order differs from the exact one by at most (n - 1) * 2^-53 * S_abs (to first order), and each listed term carries a few roundings of its
own; the tests' bounds are multiples of 2^-53 * S_abs.

Record: 0 mass | 1..3 first moment | 4..6 momentum | 7..9 angular momentum about `about` | 10 kinetic | 11 gravitational | 12 item count.
Terms per item: one for slots 0..6 and 12; the two products of every cross-product component for 7..9; the three products of the dot product for 10
and 11. A rigid body adds the 27 products R_ia J_ab R_jb w_j to every component of 7..9 and the 81 products 0.5 w_i R_ia J_ab R_jb w_j to slot 10."""
import math

import numpy as np

U = 2.0 ** -53
REC = 13


def quat_advance(q0, w, dt):
    """q1 = normalize(q0 + dt/2 (0, w) q0), (w, x, y, z) storage: the update of every rigid-body potential and of the contact detector's vertices."""
    e, f, g, h = q0
    wx, wy, wz = w
    p = np.array([-(wx * f) - wy * g - wz * h, wx * e + wy * h - wz * g, -(wx * h) + wy * e + wz * f, wx * g - wy * f + wz * e])
    q = np.asarray(q0, dtype=np.float64) + (0.5 * dt) * p
    return q * (1.0 / math.sqrt(float((q * q).sum())))


def quat_to_R(q):
    w, x, y, z = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def point_terms(m, x, v, about, gravity):
    """The terms of every slot for n point masses: a list of 13 arrays [n, terms per item]."""
    m = np.asarray(m, dtype=np.float64).reshape(-1)
    x = np.asarray(x, dtype=np.float64).reshape(-1, 3)
    v = np.asarray(v, dtype=np.float64).reshape(-1, 3)
    about = np.asarray(about, dtype=np.float64)
    g = np.asarray(gravity, dtype=np.float64)
    p = m[:, None] * v
    r = x - about
    t = [m[:, None]]
    t += [(m * x[:, k])[:, None] for k in range(3)]
    t += [p[:, k][:, None] for k in range(3)]
    for a, b, c in ((0, 1, 2), (1, 2, 0), (2, 0, 1)):
        t.append(np.stack([r[:, b] * p[:, c], -(r[:, c] * p[:, b])], axis=1))
    t.append(np.stack([0.5 * p[:, k] * v[:, k] for k in range(3)], axis=1))
    t.append(np.stack([-(m * g[k] * x[:, k]) for k in range(3)], axis=1))
    t.append(np.ones((len(m), 1)))
    return t


def sum_terms(terms):
    """(fsum, S_abs) of one array of terms."""
    flat = np.asarray(terms, dtype=np.float64).ravel()
    return math.fsum(flat.tolist()), math.fsum(np.abs(flat).tolist())


def point_records(m, x, v, group, n_groups, about, gravity):
    """(rec [n_groups, 13], S_abs [n_groups, 13]) of point masses m at x with velocity v, item i in group group[i]."""
    terms = point_terms(m, x, v, about, gravity)
    group = np.asarray(group).reshape(-1)
    rec, mag = np.zeros((n_groups, REC)), np.zeros((n_groups, REC))
    for g in range(n_groups):
        sel = group == g
        for k in range(REC):
            rec[g, k], mag[g, k] = sum_terms(terms[k][sel])
    return rec, mag


def inertia_records(volume, density, x0, v1, dt, group, n_groups, about, gravity):
    """The record of EnergyLumpedInertia's items: m = volume * density[group], x = x0 + dt v1, v = v1."""
    group = np.asarray(group).reshape(-1)
    m = np.asarray(volume, dtype=np.float64).reshape(-1) * np.asarray(density, dtype=np.float64).reshape(-1)[group]
    x = np.asarray(x0, dtype=np.float64) + dt * np.asarray(v1, dtype=np.float64)
    return point_records(m, x, v1, group, n_groups, about, gravity)


def body_record(m, t1, R1, v, w, J_loc, about, gravity):
    """(rec [13], S_abs [13]) of one rigid body at the END-OF-STEP pose (t1, R1): p = m v, L = (t1 - about) x p + J1 w, T = 0.5 m v.v + 0.5 w.J1 w."""
    terms = [a.ravel() for a in point_terms([m], [t1], [v], about, gravity)]
    R1 = np.asarray(R1, dtype=np.float64)
    J = np.asarray(J_loc, dtype=np.float64).reshape(3, 3)
    w = np.asarray(w, dtype=np.float64)
    Jw = np.einsum("ia,ab,jb,j->iabj", R1, J, R1, w)   # the 27 products of every component of J1 w
    for i in range(3):
        terms[7 + i] = np.r_[terms[7 + i], Jw[i].ravel()]
    terms[10] = np.r_[terms[10], (0.5 * w[:, None, None, None] * Jw).ravel()]
    rec, mag = np.zeros(REC), np.zeros(REC)
    for k in range(REC):
        rec[k], mag[k] = sum_terms(terms[k])
    return rec, mag


def rigid_records(t0, q0, v1, w1, mass, J_loc, dt, about, gravity):
    """Records of bodies given at the START-OF-STEP pose, the way the engine holds them: t1 = t0 + dt v1, q1 advanced by quat_advance."""
    out = [body_record(mass[b], np.asarray(t0[b]) + dt * np.asarray(v1[b]), quat_to_R(quat_advance(q0[b], w1[b], dt)), v1[b], w1[b], J_loc[b], about, gravity)
           for b in range(len(mass))]
    return np.array([o[0] for o in out]), np.array([o[1] for o in out])


def energy_sum(element_energies):
    """(fsum, S_abs) of one potential's element energies."""
    return sum_terms(element_energies)


def inertia_tensor_box(mass, size):
    """stark/src/models/rigidbodies/inertia_tensors.cpp:31-47 (the formula of a solid cuboid)."""
    sx, sy, sz = size
    return np.diag([mass / 12.0 * (sy * sy + sz * sz), mass / 12.0 * (sx * sx + sz * sz), mass / 12.0 * (sx * sx + sy * sy)])


def assert_exact_family(volume, density, x0, v1, dt, group, n_groups, about, gravity):
    """The exact family's claim: every term the device forms is a dyadic rational it represents exactly, and every partial sum of a group's terms in any
    order fits 53 bits. Inputs: volumes integer / 8, integer densities and gravity, x0, v1 and `about` integer / 64, dt = 1 / 8. The terms are recomputed
    in 64-bit integer arithmetic at a fixed power-of-two scale per slot; each must equal its double times that scale, and the sum of a group's |terms| at
    that scale must stay below 2^53 (then no partial sum, in whatever order or tree, ever rounds)."""
    def ints(a, scale):
        a = np.asarray(a, dtype=np.float64) * scale
        assert (a == np.rint(a)).all() and (np.abs(a) < 2 ** 20).all()
        return a.astype(np.int64)

    assert dt == 0.125
    group = np.asarray(group).reshape(-1)
    M = ints(volume, 8).reshape(-1) * ints(density, 1).reshape(-1)[group]   # m * 8
    V = ints(v1, 64)                                                         # v * 64
    X = ints(x0, 64) * 8 + V                                                 # x * 512
    R = X - ints(about, 64) * 8                                              # (x - about) * 512
    G = ints(gravity, 1)
    P = M[:, None] * V                                                       # p * 512
    it = [(M[:, None], 8)] + [((M * X[:, k])[:, None], 4096) for k in range(3)] + [(P[:, k][:, None], 512) for k in range(3)]
    for a, b, c in ((0, 1, 2), (1, 2, 0), (2, 0, 1)):
        it.append((np.stack([R[:, b] * P[:, c], -(R[:, c] * P[:, b])], axis=1), 2 ** 18))
    it.append((P * V, 2 ** 16))
    it.append((-(M[:, None] * G[None, :] * X), 4096))
    it.append((np.ones((len(M), 1), dtype=np.int64), 1))
    m = np.asarray(volume, dtype=np.float64).reshape(-1) * np.asarray(density, dtype=np.float64).reshape(-1)[group]
    fl = point_terms(m, np.asarray(x0, dtype=np.float64) + dt * np.asarray(v1, dtype=np.float64), v1, about, gravity)
    for k in range(REC):
        exact, scale = it[k]
        assert (fl[k] * float(scale) == exact.astype(np.float64)).all(), ("a term is not exact in double", k)
        for g in range(n_groups):
            assert int(np.abs(exact[group == g]).sum()) < 2 ** 53, ("partial sums may round", g, k)
