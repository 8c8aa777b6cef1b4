"""Reference of the stress readout (include/mistark.h "stress readout"; record layout: stark_amd/csrc/stress.hpp), in numpy, and the small meshes
and states its tests share.

Two derivations of the same records:
  (A) `records(prob, pot)`: a direct restatement of P, sigma and the scalars from the density formulas of oracle/energies.py; stretches from
      numpy.linalg.svd.
  (B) `stress_from_oracle(prob, pot)`: the same stress obtained LINEARLY from the element gradients oracle.evaluator.evaluate_potential has proven
      against the reference. Tet: dE/dv_a = V dt P w_a and sum_a w_a X_a^T = I, so P = (1 / (V dt)) sum_a g_a X_a^T. Triangle: with the projected
      rest coordinates Y_a about their centroid, F S = (1 / (w dt)) sum_a g_a Y_a^T, and the inflation term drops out (sum_a Y_a = 0). Segment:
      N = g_0 . t / dt with t the unit vector from node 1 to node 0.
"""
import functools

import numpy as np

from oracle import evaluator as ev

KIND = {"EnergyTetStrain": (0, True), "EnergyTetStrain_Elasticity_Only": (0, False), "EnergyTriangleStrain": (1, True),
        "EnergyTriangleStrain_Elasticity_Only": (1, False), "EnergySegmentStrain": (2, True), "EnergySegmentStrain_Elasticity_Only": (2, False)}
NAMES = list(KIND)
NB = {0: 4, 1: 3, 2: 2}
GAM = np.sqrt(2.0 / 3.0)


# ---- gathered inputs ---------------------------------------------------------------------------------------------------------------------
def gather(prob, pot):
    """Per binding the gathered values [n_elem, stride] (what the kernels' gather_inputs reads)."""
    n = pot.conn.shape[0]
    out = []
    for b in pot.bindings:
        data = prob.arrays[b.array]
        out.append(data[pot.conn[:, b.conn]] if b.conn >= 0 else np.broadcast_to(data[0], (n, b.stride)))
    return out


def gathered_flat(prob, pot):
    """[n_elem, NIN]: the in[] array of the device functions."""
    return np.ascontiguousarray(np.concatenate(gather(prob, pot), axis=1))


def _nodes(b, nb):
    v1 = np.stack(b[0:nb], axis=1)
    x0 = np.stack(b[nb:2 * nb], axis=1)
    X = np.stack(b[2 * nb:3 * nb], axis=1)
    return v1, x0, X


def _voigt(s):
    return np.stack([s[:, 0, 0], s[:, 1, 1], s[:, 2, 2], s[:, 0, 1], s[:, 1, 2], s[:, 2, 0]], axis=1)


def _finish(rec, sigma, limiting, degenerate):
    s = _voigt(sigma)
    s[degenerate] = 0.0
    rec[:, 0:6] = s
    rec[:, 6] = np.sqrt(0.5 * ((s[:, 0] - s[:, 1]) ** 2 + (s[:, 1] - s[:, 2]) ** 2 + (s[:, 2] - s[:, 0]) ** 2) + 3.0 * (s[:, 3] ** 2 + s[:, 4] ** 2 + s[:, 5] ** 2))
    rec[:, 7] = (s[:, 0] + s[:, 1] + s[:, 2]) / 3.0
    rec[degenerate, 12] = 0.0
    rec[:, 15] = 1.0 * limiting + 2.0 * degenerate


def _tet_geometry(b):
    v1, x0, X = _nodes(b, 4)
    scale = b[12][:, 0]
    full = len(b) == 19
    dt = b[18 if full else 15][:, 0]
    Xs = scale[:, None, None] * X
    x1 = x0 + dt[:, None, None] * v1
    DX = np.stack([Xs[:, k] - Xs[:, 0] for k in (1, 2, 3)], axis=2)
    Dx1 = np.stack([x1[:, k] - x1[:, 0] for k in (1, 2, 3)], axis=2)
    Dx0 = np.stack([x0[:, k] - x0[:, 0] for k in (1, 2, 3)], axis=2)
    DXi = np.linalg.inv(DX)
    return dict(F=Dx1 @ DXi, F0=Dx0 @ DXi, vol=np.linalg.det(DX) / 6.0, dt=dt, Xs=Xs, x1=x1, Dx1=Dx1, full=full)


def _tet_records(b):
    g = _tet_geometry(b)
    F, F0, full = g["F"], g["F0"], g["full"]
    n = len(F)
    e, nu = b[13][:, 0], b[14][:, 0]
    mu = e / (2.0 * (1.0 + nu))
    lam = (e * nu) / ((1.0 + nu) * (1.0 - 2.0 * nu))
    mu_ = 4.0 / 3.0 * mu
    lam_ = lam + 5.0 / 6.0 * mu
    alpha = 1.0 + mu_ / lam_ - mu_ / (4.0 * lam_)
    J = np.linalg.det(F)
    Ic = (F * F).sum(axis=(1, 2))
    cof = np.stack([np.cross(F[:, :, 1], F[:, :, 2]), np.cross(F[:, :, 2], F[:, :, 0]), np.cross(F[:, :, 0], F[:, :, 1])], axis=2)
    psi = 0.5 * mu_ * (Ic - 3.0) + 0.5 * lam_ * (J - alpha) ** 2 - 0.5 * mu_ * np.log(Ic + 1.0)
    c1 = mu_ * (1.0 - 1.0 / (Ic + 1.0))
    c3 = lam_ * (J - alpha)
    T = np.zeros((n, 3, 3))
    limiting = np.zeros(n, dtype=bool)
    arg = np.full(n, -np.inf)
    if full:
        limit, k, damping = b[15][:, 0], b[16][:, 0], b[17][:, 0]
        I = np.eye(3)
        E1 = 0.5 * (np.swapaxes(F, 1, 2) @ F - I)
        E0 = 0.5 * (np.swapaxes(F0, 1, 2) @ F0 - I)
        dE = (E1 - E0) / g["dt"][:, None, None]
        psi = psi + 0.5 * damping * (dE * dE).sum(axis=(1, 2))
        T = damping[:, None, None] * dE / g["dt"][:, None, None]
        trE = np.trace(E1, axis1=1, axis2=2)
        D = E1 - trE[:, None, None] / 3.0 * I
        nD = np.sqrt((D * D).sum(axis=(1, 2)))
        largest = trE / 3.0 + GAM * nD
        dl = largest - limit
        limiting = dl > 0.0
        arg = dl / np.maximum(np.abs(largest) + np.abs(limit), 1e-300)
        psi = psi + np.where(limiting, k * dl ** 3 / 3.0, 0.0)
        G = I / 3.0 + GAM * D / np.maximum(nD, 1e-300)[:, None, None]
        T = T + np.where(limiting, k * dl ** 2, 0.0)[:, None, None] * G
    t1, t2, t3 = c1[:, None, None] * F, c3[:, None, None] * cof, F @ T
    P = t1 + t2 + t3
    degenerate = ~(J > 0.0)
    Js = np.where(degenerate, 1.0, J)
    sigma = P @ np.swapaxes(F, 1, 2) / Js[:, None, None]
    sigma = 0.5 * (sigma + np.swapaxes(sigma, 1, 2))
    sv = np.linalg.svd(F, compute_uv=False)
    rec = np.zeros((n, 16))
    rec[:, 8] = J
    rec[:, 9:12] = sv
    rec[:, 12] = 0.5 * (sv[:, 0] ** 2 - 1.0)
    rec[:, 13] = psi
    rec[:, 14] = g["vol"]
    _finish(rec, sigma, limiting, degenerate)
    nF = np.abs(F).max(axis=(1, 2))
    terms = (np.abs(t1).max(axis=(1, 2)) + np.abs(t2).max(axis=(1, 2)) + np.abs(t3).max(axis=(1, 2))) * nF / np.abs(Js)
    return rec, terms, arg


def _tri_geometry(b):
    v1, x0, X = _nodes(b, 3)
    full = len(b) == 18
    scale, thickness = b[9][:, 0], b[10][:, 0]
    inflation = b[16 if full else 13][:, 0]
    dt = b[17 if full else 14][:, 0]
    Xs = scale[:, None, None] * X
    x1 = x0 + dt[:, None, None] * v1
    u = Xs[:, 1] - Xs[:, 0]
    u = u / np.linalg.norm(u, axis=1)[:, None]
    nn = np.cross(u, Xs[:, 2] - Xs[:, 0])
    v = np.cross(u, nn)
    v = v / np.linalg.norm(v, axis=1)[:, None]
    Y = np.stack([(Xs * u[:, None, :]).sum(axis=2), (Xs * v[:, None, :]).sum(axis=2)], axis=2)  # [n, node, 2]
    DY = np.stack([Y[:, 1] - Y[:, 0], Y[:, 2] - Y[:, 0]], axis=2)
    DYi = np.linalg.inv(DY)
    Dx1 = np.stack([x1[:, 1] - x1[:, 0], x1[:, 2] - x1[:, 0]], axis=2)
    Dx0 = np.stack([x0[:, 1] - x0[:, 0], x0[:, 2] - x0[:, 0]], axis=2)
    rest_area = 0.5 * np.linalg.norm(np.cross(Xs[:, 0] - Xs[:, 2], Xs[:, 1] - Xs[:, 2]), axis=1)
    n0 = -np.cross(x0[:, 1] - x0[:, 0], x0[:, 2] - x0[:, 0])
    with np.errstate(invalid="ignore", divide="ignore"):  # (a collapsed triangle has no normal; its inflation term is not used)
        n0 = n0 / np.linalg.norm(n0, axis=1)[:, None]
    infl = inflation * (n0 * x1.sum(axis=1)).sum(axis=1) / 3.0
    return dict(F=Dx1 @ DYi, F0=Dx0 @ DYi, w=thickness * rest_area, dt=dt, Y=Y, x1=x1, infl=infl, full=full)


def _tri_records(b):
    g = _tri_geometry(b)
    F, F0, full = g["F"], g["F0"], g["full"]
    n = len(F)
    e, nu = b[11][:, 0], b[12][:, 0]
    mu = e / (2.0 * (1.0 + nu))
    lam = (e * nu) / ((1.0 + nu) * (1.0 - nu))
    C = np.swapaxes(F, 1, 2) @ F
    detC = np.linalg.det(C)
    degenerate = ~(detC > 0.0)
    J = np.sqrt(np.where(degenerate, 0.0, detC))
    Js = np.where(degenerate, 1.0, J)
    logJ = np.log(Js)
    I = np.eye(2)
    psi = 0.5 * mu * (np.trace(C, axis1=1, axis2=2) - 2.0) - mu * logJ + 0.5 * lam * logJ ** 2
    Ci = np.linalg.inv(np.where(degenerate[:, None, None], I, C))
    s1, s2 = mu[:, None, None] * I, (lam * logJ - mu)[:, None, None] * Ci
    S = s1 + s2
    s3 = np.zeros_like(S)
    limiting = np.zeros(n, dtype=bool)
    arg = np.full(n, -np.inf)
    if full:
        damping, limit, k = b[13][:, 0], b[14][:, 0], b[15][:, 0]
        E1 = 0.5 * (C - I)
        E0 = 0.5 * (np.swapaxes(F0, 1, 2) @ F0 - I)
        dE = (E1 - E0) / g["dt"][:, None, None]
        psi = psi + 0.5 * damping * (dE * dE).sum(axis=(1, 2))
        s3 = damping[:, None, None] * dE / g["dt"][:, None, None]
        ew, evec = np.linalg.eigh(E1)
        arg = np.full(n, -np.inf)
        for i in range(2):
            dl = ew[:, i] - limit
            on = dl > 0.0
            limiting |= on
            a = dl / np.maximum(np.abs(ew[:, i]) + np.abs(limit), 1e-300)
            arg = np.where(np.abs(a) < np.abs(arg), a, arg)
            psi = psi + np.where(on, k * dl ** 3 / 3.0, 0.0)
            s3 = s3 + np.where(on, k * dl ** 2, 0.0)[:, None, None] * (evec[:, :, i, None] * evec[:, None, :, i])
        S = S + s3
    psi = np.where(degenerate, 0.0, psi)
    sigma = F @ S @ np.swapaxes(F, 1, 2) / Js[:, None, None]
    sv = np.linalg.svd(F, compute_uv=False)
    rec = np.zeros((n, 16))
    rec[:, 8] = J
    rec[:, 9:11] = sv
    rec[:, 12] = 0.5 * (sv[:, 0] ** 2 - 1.0)
    rec[:, 13] = psi
    rec[:, 14] = g["w"]
    _finish(rec, sigma, limiting, degenerate)
    nF = np.abs(F).max(axis=(1, 2))
    terms = (np.abs(s1).max(axis=(1, 2)) + np.abs(s2).max(axis=(1, 2)) + np.abs(s3).max(axis=(1, 2))) * nF * nF / Js
    return rec, terms, arg


def _seg_geometry(b):
    v1, x0, X = _nodes(b, 2)
    full = len(b) == 13
    scale, radius, youngs = b[6][:, 0], b[7][:, 0], b[8][:, 0]
    dt = b[12 if full else 9][:, 0]
    x1 = x0 + dt[:, None, None] * v1
    l_rest = np.linalg.norm(scale[:, None] * X[:, 0] - scale[:, None] * X[:, 1], axis=1)
    d = x1[:, 0] - x1[:, 1]
    return dict(x0=x0, x1=x1, d=d, l=np.linalg.norm(d, axis=1), l_rest=l_rest, area=np.pi * radius ** 2, youngs=youngs, dt=dt, full=full)


def _seg_records(b):
    g = _seg_geometry(b)
    l, L, A, Y, dt = g["l"], g["l_rest"], g["area"], g["youngs"], g["dt"]
    n = len(l)
    V = A * L
    eps = (l - L) / L
    E = V * Y * eps ** 2 / 2.0
    t1 = V * Y * eps
    dE = t1.copy()
    t2 = np.zeros(n)
    limiting = np.zeros(n, dtype=bool)
    arg = np.full(n, -np.inf)
    if g["full"]:
        damping, limit, k = b[9][:, 0], b[10][:, 0], b[11][:, 0]
        over = eps - limit
        limiting = over > 0.0
        arg = over / np.maximum(np.abs(eps) + np.abs(limit), 1e-300)
        E = E + np.where(limiting, V * k * over ** 3 / 3.0, 0.0)
        e0 = (np.linalg.norm(g["x0"][:, 1] - g["x0"][:, 0], axis=1) - L) / L
        E = E + dt * damping * ((eps - e0) / dt) ** 2 / 2.0
        t2 = np.where(limiting, V * k * over ** 2, 0.0) + damping * (eps - e0) / dt
        dE = dE + t2
    degenerate = ~(l > 0.0)
    ls = np.where(degenerate, 1.0, l)
    t = g["d"] / ls[:, None]
    axial = dE / L / A
    sigma = axial[:, None, None] * (t[:, :, None] * t[:, None, :])
    rec = np.zeros((n, 16))
    rec[:, 8] = l / L
    rec[:, 9] = l / L
    rec[:, 12] = 0.5 * ((l / L) ** 2 - 1.0)
    rec[:, 13] = E / V
    rec[:, 14] = V
    _finish(rec, sigma, limiting, degenerate)
    return rec, (np.abs(t1) + np.abs(t2)) / L / A, arg


def records(prob, pot):
    """(A): (rec [n_elem, 16], terms [n_elem] = the magnitude of the terms each element's stress is the sum of, arg [n_elem] = the strain-limiting
    argument relative to its own terms: the flag of an element with |arg| < 1e-9 is not decided by the arithmetic)."""
    kind, _ = KIND[pot.name]
    return (_tet_records, _tri_records, _seg_records)[kind](gather(prob, pot))


def stress_from_oracle(prob, pot):
    """(B): sigma [n_elem, 6] (xx yy zz xy yz zx) from the oracle's element gradients, and the oracle's element energies without the triangles'
    inflation term."""
    kind, _ = KIND[pot.name]
    b = gather(prob, pot)
    o = ev.evaluate_potential(prob, pot)
    assert o.active.all()
    gr = o.g.reshape(len(o.g), NB[kind], 3)
    if kind == 0:
        g = _tet_geometry(b)
        P = np.einsum("nai,naj->nij", gr, g["Xs"]) / (g["vol"] * g["dt"])[:, None, None]
        sigma = P @ np.swapaxes(g["F"], 1, 2) / np.linalg.det(g["F"])[:, None, None]
        E = o.E
    elif kind == 1:
        g = _tri_geometry(b)
        Yc = g["Y"] - g["Y"].mean(axis=1, keepdims=True)
        FS = np.einsum("nai,naj->nij", gr, Yc) / (g["w"] * g["dt"])[:, None, None]
        C = np.swapaxes(g["F"], 1, 2) @ g["F"]
        sigma = FS @ np.swapaxes(g["F"], 1, 2) / np.sqrt(np.linalg.det(C))[:, None, None]
        E = o.E - g["w"] * g["infl"]
    else:
        g = _seg_geometry(b)
        t = g["d"] / g["l"][:, None]
        N = (gr[:, 0] * t).sum(axis=1) / g["dt"]
        sigma = (N / g["area"])[:, None, None] * (t[:, :, None] * t[:, None, :])
        E = o.E
    return _voigt(0.5 * (sigma + np.swapaxes(sigma, 1, 2))), E


def inflation_energy(prob, pot):
    """w * (inflation / 3) n0 . (x_0 + x_1 + x_2) of a triangle potential's elements (what its energy holds beside m * psi), else zeros."""
    if KIND[pot.name][0] != 1:
        return np.zeros(pot.conn.shape[0])
    g = _tri_geometry(gather(prob, pot))
    return g["w"] * g["infl"]


def rel_to_scale(a, b, scale, tol):
    """forces_ref.rel_to_scale: the error relative to max|b|, or to the terms where b has cancelled below the tolerance of its own terms."""
    bmax = np.abs(b).max()
    return np.abs(a - b).max() / max(bmax if bmax >= tol * scale else scale, 1e-300)


ELEMENT_TOL = 1e-11


def check_records(got, rec, terms, arg, what):
    """The comparison the GPU tests use too: got [n, 16] against (A)."""
    for f in range(8):
        err = rel_to_scale(got[:, f], rec[:, f], terms.max(), ELEMENT_TOL)
        print("%s field %d: rel %.3g" % (what, f, err))
        assert err < ELEMENT_TOL, (what, f, err)
    smax = rec[:, 9]
    for f in (9, 10, 11):
        live = rec[:, f] > 0.0
        assert (got[~live, f] == 0.0).all(), (what, f)
        bound = ELEMENT_TOL * smax[live] ** 2 / rec[live, f]
        err = np.abs(got[live, f] - rec[live, f])
        print("%s stretch %d: worst error / bound %.3g" % (what, f - 9, (err / bound).max() if live.any() else 0.0))
        assert (err <= bound).all(), (what, f)
    for f in (8, 12, 13, 14):
        scale = max(np.abs(rec[:, f]).max(), 1.0 if f == 12 else 0.0)  # (a Green strain is a difference of stretches^2 of size 1)
        err = np.abs(got[:, f] - rec[:, f]).max() / max(scale, 1e-300)
        print("%s field %d: rel %.3g" % (what, f, err))
        assert err < ELEMENT_TOL, (what, f, err)
    decided = np.abs(arg) >= 1e-9
    assert (~decided).sum() <= 1e-3 * len(arg), what
    assert (got[decided, 15] == rec[decided, 15]).all(), what


def nodal_average(n_rows, rows, rec):
    """(avg [n_rows, 10], mag [n_rows, 10]) of records rec [n, 16] at block rows [n, nb]: sum m field / sum m for fields 0..8, then sum m; mag =
    the sum of |terms| of each entry (divided by the weight sum like the entry itself)."""
    num, mag = np.zeros((n_rows, 10)), np.zeros((n_rows, 10))
    m = rec[:, 14]
    val = np.concatenate([m[:, None] * rec[:, 0:9], m[:, None]], axis=1)
    for k in range(rows.shape[1]):
        np.add.at(num, rows[:, k], val)
        np.add.at(mag, rows[:, k], np.abs(val))
    w = num[:, 9].copy()
    ws = np.where(w > 0.0, w, 1.0)
    num[:, :9] /= ws[:, None]
    mag[:, :9] /= ws[:, None]
    return num, mag


# ---- meshes ------------------------------------------------------------------------------------------------------------------------------
KUHN = [(0, 1, 3, 7), (0, 3, 2, 7), (0, 2, 6, 7), (0, 6, 4, 7), (0, 4, 5, 7), (0, 5, 1, 7)]  # corner index = x + 2 y + 4 z; all positively oriented


def tet_grid(nx, ny, nz, h=0.1):
    idx = lambda i, j, k: (k * (ny + 1) + j) * (nx + 1) + i
    X = np.array([[i * h, j * h, k * h] for k in range(nz + 1) for j in range(ny + 1) for i in range(nx + 1)], dtype=np.float64)
    conn = []
    for k in range(nz):
        for j in range(ny):
            for i in range(nx):
                c = [idx(i + (q & 1), j + ((q >> 1) & 1), k + ((q >> 2) & 1)) for q in range(8)]
                conn += [[c[a] for a in t] for t in KUHN]
    return X, np.array(conn, dtype=np.int32)


def tri_grid(nx, ny, h=0.1):
    idx = lambda i, j: j * (nx + 1) + i
    X = np.array([[i * h, j * h, 0.0] for j in range(ny + 1) for i in range(nx + 1)], dtype=np.float64)
    conn = []
    for j in range(ny):
        for i in range(nx):
            conn += [[idx(i, j), idx(i + 1, j), idx(i + 1, j + 1)], [idx(i, j), idx(i + 1, j + 1), idx(i, j + 1)]]
    return X, np.array(conn, dtype=np.int32)


def seg_chain(n, h=0.1):
    X = np.array([[i * h, 0.02 * np.sin(0.7 * i), 0.0] for i in range(n + 1)], dtype=np.float64)
    return X, np.array([[i, i + 1] for i in range(n)], dtype=np.int32)


def tet_fan(n, step=0.3):
    """n tets around the common edge (0, 1); the ring winds around the edge as often as it takes (elements may overlap in space: nothing collides)."""
    ring = [[0.1 * np.cos(step * i), 0.1 * np.sin(step * i), 0.05 + 0.01 * np.sin(1.3 * i)] for i in range(n + 1)]
    X = np.array([[0.0, 0.0, 0.0], [0.0, 0.0, 0.1]] + ring, dtype=np.float64)
    return X, np.array([[0, 1, 2 + i, 3 + i] for i in range(n)], dtype=np.int32)


def tri_fan(n, step=0.3):
    ring = [[0.1 * np.cos(step * i), 0.1 * np.sin(step * i), 0.01 * np.sin(1.3 * i)] for i in range(n + 1)]
    X = np.array([[0.0, 0.0, 0.0]] + ring, dtype=np.float64)
    return X, np.array([[0, 1 + i, 2 + i] for i in range(n)], dtype=np.int32)


PARAMS = {  # scalars in binding order, without dt
    "EnergyTetStrain": dict(scale=1.0, e=1e5, nu=0.3, strain_limit=0.1, sl_k=1e6, damping=0.05),
    "EnergyTetStrain_Elasticity_Only": dict(scale=1.0, e=1e5, nu=0.3),
    "EnergyTriangleStrain": dict(scale=1.0, thickness=1e-3, e=1e4, nu=0.3, damping=0.05, strain_limit=0.1, sl_k=1e5, inflation=30.0),
    "EnergyTriangleStrain_Elasticity_Only": dict(scale=1.0, thickness=1e-3, e=1e4, nu=0.3, inflation=30.0),
    "EnergySegmentStrain": dict(scale=1.0, radius=2e-3, e=1e6, damping=1e-4, strain_limit=0.05, sl_k=1e8),
    "EnergySegmentStrain_Elasticity_Only": dict(scale=1.0, radius=2e-3, e=1e6),
}
DT = 0.01


def make_problem(parts, X, x0, v1, dt=DT):
    """An oracle Problem with one DoF set (the nodes' velocities) and one potential per (name, conn, params) of `parts`; scalars are global values."""
    arrays = [np.array(v1, dtype=np.float64), np.array(x0, dtype=np.float64), np.array(X, dtype=np.float64)]
    pots = []
    for name, conn, params in parts:
        nb = NB[KIND[name][0]]
        bs = [ev.Binding(0, 3, a, 0) for a in range(nb)] + [ev.Binding(1, 3, a, -1) for a in range(nb)] + [ev.Binding(2, 3, a, -1) for a in range(nb)]
        for value in list(params.values()) + [dt]:
            arrays.append(np.array([[value]], dtype=np.float64))
            bs.append(ev.Binding(len(arrays) - 1, 1, -1, -1))
        pots.append(ev.PotentialDesc(name, np.ascontiguousarray(conn, dtype=np.int32), bs))
    n = 3 * len(X)
    return ev.Problem(dt=dt, ndofs=n, dof_offsets=[0], dof_sizes=[n], arrays=arrays, potentials=pots, dof_arrays={0: 0})


def shortest_edge(X, conn):
    nb = conn.shape[1]
    return min(np.linalg.norm(X[conn[:, a]] - X[conn[:, b]], axis=1).min() for a in range(nb) for b in range(a + 1, nb))


def rotation(angle=0.7, axis=(1.0, 2.0, 3.0)):
    a = np.array(axis) / np.linalg.norm(axis)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1.0 - np.cos(angle)) * K @ K


def mesh_of(name, n_elem=None):
    kind = KIND[name][0]
    X, conn = (tet_grid(4, 4, 3), tri_grid(12, 11), seg_chain(264))[kind]
    return X, (conn if n_elem is None else conn[:n_elem])


# A dilation with shear whose stress has six entries of one size (each about a fifth of the terms it is left of): the state of the tests that hold
# nodal SUMS to another evaluation entry by entry
SIZABLE = 1.15 * np.eye(3) + 0.15 * (np.ones((3, 3)) - np.eye(3))


def seeded_state(name, X, conn, seed, limit_to_median=True, affine=None):
    """x0 = a mild affine stretch of the rest mesh plus noise, v1 random with dt |v1| <= 2 % of the shortest rest edge (nothing inverts); for the
    FULL potentials the strain limit is put between the two middle values of the elements' limiting measure, so that the branch is taken in about half of them."""
    rng = np.random.default_rng(seed)
    h = shortest_edge(X, conn)
    A = rotation(0.4, (0.3, -1.0, 0.5)) @ np.diag([1.12, 0.93, 1.05]) if affine is None else affine
    x0 = X @ A.T + 0.02 * h * rng.uniform(-1.0, 1.0, X.shape) + np.array([0.3, -0.2, 0.1])
    v = rng.normal(size=X.shape)
    v1 = v / np.linalg.norm(v, axis=1).max() * (0.02 * h / DT)
    params = dict(PARAMS[name])
    if KIND[name][1] and limit_to_median:
        params["strain_limit"] = 0.0
        prob = make_problem([(name, conn, params)], X, x0, v1)
        b = gather(prob, prob.potentials[0])
        # the measure itself: the limit it is compared with was 0
        kind = KIND[name][0]
        if kind == 0:
            g = _tet_geometry(b)
            E1 = 0.5 * (np.swapaxes(g["F"], 1, 2) @ g["F"] - np.eye(3))
            tr = np.trace(E1, axis1=1, axis2=2)
            D = E1 - tr[:, None, None] / 3.0 * np.eye(3)
            meas = tr / 3.0 + GAM * np.sqrt((D * D).sum(axis=(1, 2)))
        elif kind == 1:
            g = _tri_geometry(b)
            meas = np.linalg.eigvalsh(0.5 * (np.swapaxes(g["F"], 1, 2) @ g["F"] - np.eye(2)))[:, 1]
        else:
            g = _seg_geometry(b)
            meas = (g["l"] - g["l_rest"]) / g["l_rest"]
        # (midway between the two middle values: the median of an odd number of elements IS one element's measure, whose branch rounding would decide)
        ms = np.sort(meas)
        params["strain_limit"] = float(0.5 * (ms[len(ms) // 2 - 1] + ms[len(ms) // 2])) if len(ms) > 1 else float(ms[0] - 1e-3)
    return x0, v1, params


@functools.lru_cache(maxsize=None)
def seeded_problem(name, n_elem=None, seed=1):
    """The shared inhomogeneous state of one potential (a grid of 288 tets / 264 triangles / a chain of 264 segments, or its first n_elem elements):
    (prob, rec, terms, arg) with (A) evaluated once. Left unchanged by its users."""
    X, conn = mesh_of(name, n_elem)
    x0, v1, params = seeded_state(name, X, conn, seed)
    prob = make_problem([(name, conn, params)], X, x0, v1)
    rec, terms, arg = records(prob, prob.potentials[0])
    for a in (rec, terms, arg):
        a.setflags(write=False)
    return prob, rec, terms, arg


def block_rows(prob, pot):
    order = ev.dof_layout(pot)
    return np.stack([prob.dof_offsets[pot.bindings[bi].dof_set] // 3 + pot.conn[:, pot.bindings[bi].conn] for bi in order], axis=1).astype(np.int64)


# ---- homogeneous deformations with closed-form answers -------------------------------------------------------------------------------------
STRETCH = (1.3, 0.9, 0.75)


def _moduli(name):
    """(mu', lambda') of the tets' stable Neo-Hookean density, (mu, lambda_2D) of the membranes, (Y, 0) of the rods."""
    p = PARAMS[name]
    kind = KIND[name][0]
    if kind == 2:
        return p["e"], 0.0
    mu = p["e"] / (2.0 * (1.0 + p["nu"]))
    if kind == 1:
        return mu, p["e"] * p["nu"] / ((1.0 + p["nu"]) * (1.0 - p["nu"]))
    lam = p["e"] * p["nu"] / ((1.0 + p["nu"]) * (1.0 - 2.0 * p["nu"]))
    return 4.0 / 3.0 * mu, lam + 5.0 / 6.0 * mu


def homogeneous_cases(name):
    """[(prob, want)]: x = R diag(stretches) X + t with v1 = 0 (no damping; the strain limit is out of reach) on a cube of 6 Kuhn tets, a square of
    two triangles or one segment, and the same mesh under a rigid motion only. want: sigma [6], stretches [3], J, and `zero` = the absolute bound for
    the undeformed case, 1e-11 * (mu' + lambda'): the size of the terms that cancel there."""
    kind = KIND[name][0]
    X, conn = (tet_grid(1, 1, 1), tri_grid(1, 1), seg_chain(1))[kind]
    R = rotation()
    t = np.array([0.3, -0.2, 0.1])
    a, b = _moduli(name)
    params = dict(PARAMS[name])
    if "strain_limit" in params:
        params["strain_limit"] = 10.0
    out = []
    for deformed in (True, False):
        l = np.array(STRETCH if deformed else (1.0, 1.0, 1.0))
        if kind == 0:
            J = l.prod()
            Ic = (l ** 2).sum()
            alpha = 1.0 + a / b - a / (4.0 * b)
            principal = a * (1.0 - 1.0 / (Ic + 1.0)) * l ** 2 / J + b * (J - alpha)
            stretches = np.sort(l)[::-1]
            A = R @ np.diag(l)
        elif kind == 1:
            l[2] = 1.0
            J = l[0] * l[1]
            principal = np.array([(a * (l[0] ** 2 - 1.0) + b * np.log(J)) / J, (a * (l[1] ** 2 - 1.0) + b * np.log(J)) / J, 0.0])
            stretches = np.array([max(l[0], l[1]), min(l[0], l[1]), 0.0])
            A = R @ np.diag(l)
        else:
            # the rest segment's own direction is stretched: x = R (I + (l0 - 1) d d^T) X
            d = (X[1] - X[0]) / np.linalg.norm(X[1] - X[0])
            J = l[0]
            A = R @ (np.eye(3) + (l[0] - 1.0) * np.outer(d, d))
            tdir = R @ d
            stretches = np.array([l[0], 0.0, 0.0])
        if kind == 2:
            sigma = a * (l[0] - 1.0) * np.outer(tdir, tdir)
        else:
            sigma = R @ np.diag(principal) @ R.T
        x0 = X @ A.T + t
        prob = make_problem([(name, conn, params)], X, x0, np.zeros_like(X))
        s6 = np.array([sigma[0, 0], sigma[1, 1], sigma[2, 2], sigma[0, 1], sigma[1, 2], sigma[2, 0]])
        out.append((prob, dict(sigma=s6, stretches=stretches, J=J, zero=None if deformed else 1e-11 * (a + b))))
    return out


def check_homogeneous(got, want, what):
    """Every element reports the closed-form record. Deformed: the suite's element tolerance, 1e-11 relative to the largest stress entry; stretches by
    the rule of the eigenvalue route; von Mises and mean values as they follow from the tensor. Undeformed: the absolute bound `zero`."""
    s = want["sigma"]
    vm = np.sqrt(0.5 * ((s[0] - s[1]) ** 2 + (s[1] - s[2]) ** 2 + (s[2] - s[0]) ** 2) + 3.0 * (s[3] ** 2 + s[4] ** 2 + s[5] ** 2))
    full = np.r_[s, vm, s[:3].sum() / 3.0]
    bound = want["zero"] if want["zero"] is not None else 1e-11 * np.abs(s).max()
    err = np.abs(got[:, 0:8] - full[None, :]).max()
    print("%s %s: worst |stress error| / bound = %.3g" % (what, "deformed" if want["zero"] is None else "undeformed", err / bound))
    assert err <= bound, (what, err, bound)
    st = want["stretches"]
    for i in range(3):
        if st[i] == 0.0:
            assert (got[:, 9 + i] == 0.0).all(), what
        else:
            assert (np.abs(got[:, 9 + i] - st[i]) <= 1e-11 * st[0] ** 2 / st[i]).all(), (what, i, got[:, 9 + i])
    assert (np.abs(got[:, 8] - want["J"]) <= 1e-11 * want["J"]).all(), what
    assert (np.abs(got[:, 12] - 0.5 * (st[0] ** 2 - 1.0)) <= 1e-11 * st[0] ** 2).all(), what
    assert (got[:, 15] == 0.0).all(), what
