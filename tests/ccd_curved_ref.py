"""Restatement of the curved rigid-body CCD (include/mistark_contact.h mistark_contact_max_step_ex, include/mistark_tmcd.h mistark_cd_run_ccd_padded)
in plain Python floats, on top of tests/ccd_ref.py: the rigid-body update (energies.hpp rb_R1), the deviation bound (stark_amd/csrc/ccd_pad.hpp), the
padded additive CCD, the padded swept-box candidate set and the round loop. The test oracle of tests/test_ccd_curved_cpu.py and
tests/test_gpu_ccd_curved.py."""
import math

import numpy as np

import ccd_ref as R

PAD_CONSTANT = 7.0 / 16.0


# ---- rigid-body kinematics (energies.hpp: q1 = normalize(q0 + dt/2 (0, w) q0), quaternions (w, x, y, z)) ------------------------------------
def rb_R1(q0, w, dt):
    e, f, g, h = (float(c) for c in q0)
    wx, wy, wz = (float(c) for c in w)
    p0 = -(wx * f) - wy * g - wz * h
    p1 = wx * e + wy * h - wz * g
    p2 = -(wx * h) + wy * e + wz * f
    p3 = wx * g - wy * f + wz * e
    q = np.array([e + (0.5 * dt) * p0, f + (0.5 * dt) * p1, g + (0.5 * dt) * p2, h + (0.5 * dt) * p3])
    qw, qx, qy, qz = q / math.sqrt(float(q @ q))
    tx, ty, tz = 2.0 * qx, 2.0 * qy, 2.0 * qz
    twx, twy, twz = tx * qw, ty * qw, tz * qw
    txx, txy, txz = tx * qx, ty * qx, tz * qx
    tyy, tyz, tzz = ty * qy, tz * qy, tz * qz
    return np.array([[1.0 - (tyy + tzz), txy - twz, txz + twy], [txy + twz, 1.0 - (txx + tzz), tyz - twx], [txz - twy, tyz + twx, 1.0 - (txx + tyy)]])


def rigid_point(t0, q0, v, w, dt, x_loc):
    return rb_R1(q0, w, dt) @ np.asarray(x_loc, float) + (np.asarray(t0, float) + dt * np.asarray(v, float))


def rigid_path(t0, q0, v, w, dv, dw, dt, x_loc, ts):
    """rigid_point at w + t dw, v + t dv for every t of ts at once: [len(ts), 3]"""
    ts = np.asarray(ts, float)
    q0, x_loc = np.asarray(q0, float), np.asarray(x_loc, float)
    W = np.asarray(w, float)[None, :] + ts[:, None] * np.asarray(dw, float)[None, :]
    e, f, g, h = q0
    wx, wy, wz = W[:, 0], W[:, 1], W[:, 2]
    q = np.stack([e + (0.5 * dt) * (-(wx * f) - wy * g - wz * h), f + (0.5 * dt) * (wx * e + wy * h - wz * g), g + (0.5 * dt) * (-(wx * h) + wy * e + wz * f),
                  h + (0.5 * dt) * (wx * g - wy * f + wz * e)], axis=1)
    q /= np.sqrt((q * q).sum(axis=1))[:, None]
    qw, qv = q[:, 0:1], q[:, 1:]
    c = np.cross(qv, x_loc[None, :]) + qw * x_loc[None, :]
    r = x_loc[None, :] + 2.0 * np.cross(qv, c)   # R(q) x = x + 2 qv x (qv x x + qw x)
    return r + (np.asarray(t0, float)[None, :] + dt * (np.asarray(v, float)[None, :] + ts[:, None] * np.asarray(dv, float)[None, :]))


# ---- the bound (ccd_pad.hpp) ---------------------------------------------------------------------------------------------------------------
def pad_phi(dt, dw):
    return dt * math.sqrt(dw[0] * dw[0] + dw[1] * dw[1] + dw[2] * dw[2])


def pad_delta(r, phi, tau):
    a = phi * tau
    return min((0.4375 * r) * (a * a), 2.0 * r)


def pad_vertex(x_loc, phi, tau):
    return pad_delta(math.sqrt(x_loc[0] * x_loc[0] + x_loc[1] * x_loc[1] + x_loc[2] * x_loc[2]), phi, tau)


# ---- padded additive CCD of one pair -------------------------------------------------------------------------------------------------------
def accd_padded(ee, xa, xb, pad, eta=0.9, t_c=1.0):
    """ccd_ref.accd on the padded distance d~ = d - pad. Extra status "zero_gap" (0 < d(0) <= pad: toi 0); extra keys pad, bound (the pair survives
    the filter and pad > d(0) / 2). pad == 0.0 gives ccd_ref.accd's values."""
    x, dx, lp = R._prepare(ee, xa, xb)
    d = R.distance(ee, x)
    out = dict(status="none", toi=1.0, t_stop=None, d0=d, pad=pad, bound=False, iterations=0)
    if not d > 0.0:
        out["status"] = "touching"
        return out
    g = d - pad
    if g > 0.0 and not lp > eta * g:
        out["status"] = "filtered"
        return out
    out["bound"] = pad > 0.5 * d
    if not g > 0.0:
        out.update(status="zero_gap", toi=0.0)
        return out
    gap = (1.0 - eta) * g
    t = 0.0
    it = 0
    while True:
        step = eta * g / lp
        x = [R._add(p, R._scale(step, q)) for p, q in zip(x, dx)]
        g = R.distance(ee, x) - pad
        if t > 0.0 and g < gap:
            out.update(status="hit", toi=t, t_stop=t + step, iterations=it + 1)
            return out
        t += step
        if t > t_c:
            out["iterations"] = it + 1
            return out
        it += 1
        if it == R.MAX_ITERATIONS:
            out.update(status="capped", toi=t, iterations=it)
            return out


def last_step_padded(ee, xa, xb, pad, eta, toi):
    """The padded ACCD increment taken at the reported toi (ccd_ref.last_step on d~)."""
    x, dx, lp = R._prepare(ee, xa, xb)
    g = R.distance(ee, x) - pad
    t = 0.0
    while True:
        step = eta * g / lp
        if t >= toi:
            return step
        x = [R._add(p, R._scale(step, q)) for p, q in zip(x, dx)]
        g = R.distance(ee, x) - pad
        t += step


# ---- candidates: swept boxes grown by the primitive's largest pad before the outward rounding ----------------------------------------------
def padded_boxes(xa, xb, pad_v, prims):
    pts = np.concatenate([xa[prims], xb[prims]], axis=1)
    p = pad_v[prims].max(axis=1)[:, None]
    return R._round_down(pts.min(axis=1) - p), R._round_up(pts.max(axis=1) + p)


def candidates_padded(xa, xb, pad_v, tris, edges, mesh_of_v=None, no_self=()):
    """ccd_ref.candidates with padded boxes; mesh_of_v / no_self: meshes whose self collision is off (rigid meshes)."""
    nv = len(xa)
    tris, edges = np.asarray(tris, int).reshape(-1, 3), np.asarray(edges, int).reshape(-1, 2)
    pt, ee = np.zeros((0, 2), int), np.zeros((0, 2), int)
    mesh_of_v = np.zeros(nv, int) if mesh_of_v is None else np.asarray(mesh_of_v)
    off = np.isin(mesh_of_v, list(no_self))
    if len(tris):
        plo, phi = padded_boxes(xa, xb, pad_v, np.arange(nv)[:, None])
        tlo, thi = padded_boxes(xa, xb, pad_v, tris)
        m = R._overlap(plo, phi, tlo, thi)
        m &= ~np.any(np.arange(nv)[:, None, None] == tris[None, :, :], axis=2)
        tm = mesh_of_v[tris[:, 0]]
        m &= ~((mesh_of_v[:, None] == tm[None, :]) & off[:, None])
        pt = np.argwhere(m)
    if len(edges) > 1:
        elo, ehi = padded_boxes(xa, xb, pad_v, edges)
        m = R._overlap(elo, ehi, elo, ehi)
        m &= np.triu(np.ones((len(edges), len(edges)), bool), 1)
        share = np.zeros_like(m)
        for i in range(2):
            for j in range(2):
                share |= edges[:, i][:, None] == edges[:, j][None, :]
        m &= ~share
        em = mesh_of_v[edges[:, 0]]
        m &= ~((em[:, None] == em[None, :]) & off[edges[:, 0]][:, None])
        ee = np.argwhere(m)
    return pt, ee


def pair_pad(ee, pad4):
    return (pad4[0] + max(pad4[1], pad4[2], pad4[3])) if not ee else (max(pad4[0], pad4[1]) + max(pad4[2], pad4[3]))


def padded_query(xa, xb, pad_v, tris, edges, eta=0.9, mesh_of_v=None, no_self=(), cut=False):
    """One pass of the padded chain over a scene: dict(toi, n_candidates, n_pad_bound, max_pad, pairs) — pairs: (ee, vertex ids, result of accd_padded)
    of every candidate. cut: a pair stops at the running minimum, as on the device (large scenes; its own toi is then not known)."""
    tris, edges = np.asarray(tris, int).reshape(-1, 3), np.asarray(edges, int).reshape(-1, 2)
    pt, ee = candidates_padded(xa, xb, pad_v, tris, edges, mesh_of_v, no_self)
    best, n_bound, max_pad, pairs = 1.0, 0, 0.0, []
    for is_ee, lst in ((False, pt), (True, ee)):
        for a, b in lst:
            v = [a, *tris[b]] if not is_ee else [*edges[a], *edges[b]]
            pad = pair_pad(is_ee, pad_v[v])
            max_pad = max(max_pad, pad)
            r = accd_padded(is_ee, xa[v], xb[v], pad, eta, best if cut else 1.0)
            pairs.append((is_ee, v, r))
            n_bound += r["bound"]
            if r["status"] in ("hit", "capped", "zero_gap"):
                best = min(best, r["toi"])
    return dict(toi=best, n_candidates=len(pt) + len(ee), n_pad_bound=n_bound, max_pad=max_pad, pairs=pairs)


# ---- a scene of deformable points and rigid bodies, and the whole query ---------------------------------------------------------------------
class Scene:
    """meshes: list of dict(kind "d" | "rb", body (rb), verts (indices into x0 / x_loc), tris, edges (local)). State: x0, v1 [n, 3] of the deformable
    points, x_loc [m, 3], and per body t0, q0, v, w. A direction: dv1 [n, 3], dv [nb, 3], dw [nb, 3]."""

    def __init__(self, meshes, x0, v1, x_loc, t0, q0, v, w, dt):
        self.meshes, self.dt = meshes, float(dt)
        self.x0, self.v1, self.x_loc = (np.asarray(a, float).reshape(-1, 3) for a in (x0, v1, x_loc))
        self.t0, self.v, self.w = (np.asarray(a, float).reshape(-1, 3) for a in (t0, v, w))
        self.q0 = np.asarray(q0, float).reshape(-1, 4)
        self.tris, self.edges, self.mesh_of_v, self.src, off = [], [], [], [], 0
        for g, m in enumerate(meshes):
            nv = len(m["verts"])
            self.tris += (np.asarray(m["tris"], int).reshape(-1, 3) + off).tolist()
            self.edges += (np.asarray(m["edges"], int).reshape(-1, 2) + off).tolist()
            self.mesh_of_v += [g] * nv
            self.src += [(g, int(s)) for s in m["verts"]]
            off += nv
        self.tris, self.edges = np.asarray(self.tris, int).reshape(-1, 3), np.asarray(self.edges, int).reshape(-1, 2)
        self.mesh_of_v = np.asarray(self.mesh_of_v)
        self.no_self = [g for g, m in enumerate(meshes) if m["kind"] == "rb"]

    def positions(self, dv1, dv, dw, t):
        """collision vertices at the fraction t of the direction: the TRUE motion (rigid vertices through rb_R1 at w + t dw)"""
        out = np.zeros((len(self.src), 3))
        for i, (g, s) in enumerate(self.src):
            m = self.meshes[g]
            if m["kind"] == "d":
                out[i] = self.x0[s] + self.dt * (self.v1[s] + t * dv1[s])
            else:
                b = m["body"]
                out[i] = rigid_point(self.t0[b], self.q0[b], self.v[b] + t * dv[b], self.w[b] + t * dw[b], self.dt, self.x_loc[s])
        return out

    def pads(self, dw, tau):
        out = np.zeros(len(self.src))
        for i, (g, s) in enumerate(self.src):
            m = self.meshes[g]
            if m["kind"] == "rb":
                out[i] = pad_vertex(self.x_loc[s], pad_phi(self.dt, dw[m["body"]]), tau)
        return out

    def all_pairs(self):
        """every (point, triangle) and (edge, edge) pair the detector may pair up (own-triangle points, edges sharing a vertex and rigid self pairs out)"""
        big = np.full(len(self.src), 1e30)
        z = np.zeros((len(self.src), 3))
        pt, ee = candidates_padded(z, z, big, self.tris, self.edges, self.mesh_of_v, self.no_self)
        return [(False, [a, *self.tris[b]]) for a, b in pt] + [(True, [*self.edges[a], *self.edges[b]]) for a, b in ee]


def max_step_linear(sc, dv1, dv, dw, eta=0.9):
    """mistark_contact_max_step / rigid_mode 0: chords between the positions at u and u + du, no pads"""
    xa, xb = sc.positions(dv1, dv, dw, 0.0), sc.positions(dv1, dv, dw, 1.0)
    q = padded_query(xa, xb, np.zeros(len(xa)), sc.tris, sc.edges, eta, sc.mesh_of_v, sc.no_self)
    return dict(max_step=q["toi"], n_candidates=q["n_candidates"], rounds=1, tau=1.0, pad_bound_pairs=0, max_pad=0.0, query=q, xa=xa, xb=xb, pad_v=np.zeros(len(xa)))


def max_step_curved(sc, dv1, dv, dw, eta=0.9, max_rounds=4):
    """rigid_mode 1: the padded chord query, halved while a surviving pair is pad-bound"""
    tau, rnd = 1.0, 1
    xa = sc.positions(dv1, dv, dw, 0.0)
    while True:
        xb = sc.positions(dv1, dv, dw, tau)
        pad_v = sc.pads(dw, tau)
        q = padded_query(xa, xb, pad_v, sc.tris, sc.edges, eta, sc.mesh_of_v, sc.no_self)
        if q["n_pad_bound"] == 0 or rnd == max_rounds:
            break
        tau *= 0.5
        rnd += 1
    return dict(max_step=tau * q["toi"], n_candidates=q["n_candidates"], rounds=rnd, tau=tau, pad_bound_pairs=q["n_pad_bound"], max_pad=q["max_pad"], query=q,
                xa=xa, xb=xb, pad_v=pad_v)


def true_distances(sc, dv1, dv, dw, ts, pairs=None):
    """[len(ts), n_pairs] classified distances of the true motion"""
    pairs = sc.all_pairs() if pairs is None else pairs
    out = np.zeros((len(ts), len(pairs)))
    for k, t in enumerate(ts):
        x = sc.positions(dv1, dv, dw, float(t))
        for j, (ee, v) in enumerate(pairs):
            out[k, j] = R.distance(ee, [tuple(p) for p in x[v]])
    return out


# ---- the discriminating scene: a blade tip sweeping an arc through a small triangle the chord misses ----------------------------------------
def blade_scene(phi=1.2, arm=0.5, radius=0.47, size=0.02, dt=0.1):
    """One rigid body at the origin (q0 identity, w = 0) turning about z by dt |dw| = phi along the direction; its mesh is a thin blade in the plane
    z = 0 with the tip at (arm, 0, 0). A static deformable triangle of the given size, centred at `radius` on the bisector of the swept angle, its
    plane containing the radial direction and z (normal = tangential): the tip's arc crosses it, the tip's chord passes inside of it.
    Returns (scene, dv1, dv, dw)."""
    x_loc = np.array([[arm, 0.0, 0.0], [0.05, 0.004, 0.0], [0.05, -0.004, 0.0]])
    blade = dict(kind="rb", body=0, verts=[0, 1, 2], tris=[[0, 1, 2]], edges=[[0, 1], [1, 2], [2, 0]])
    ang = swept_angle(phi) / 2.0
    rad, zz = np.array([math.cos(ang), math.sin(ang), 0.0]), np.array([0.0, 0.0, 1.0])
    c = radius * rad
    x0 = np.array([c - 0.5 * size * rad - 0.5 * size * zz, c + 0.5 * size * rad - 0.5 * size * zz, c + 0.5 * size * zz])
    tri = dict(kind="d", verts=[0, 1, 2], tris=[[0, 1, 2]], edges=[[0, 1], [1, 2], [2, 0]])
    sc = Scene([blade, tri], x0, np.zeros((3, 3)), x_loc, [[0.0, 0.0, 0.0]], [[1.0, 0.0, 0.0, 0.0]], [[0.0, 0.0, 0.0]], [[0.0, 0.0, 0.0]], dt)
    return sc, np.zeros((3, 3)), np.zeros((1, 3)), np.array([[0.0, 0.0, phi / dt]])


def swept_angle(phi):
    """angle the body has turned at the end of the direction: q = (1, 0, 0, phi / 2) normalised, i.e. 2 atan(phi / 2)"""
    return 2.0 * math.atan(0.5 * phi)
