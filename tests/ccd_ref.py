"""Restatement of the CCD query (include/mistark_contact.h mistark_contact_max_step, include/mistark_tmcd.h mistark_cd_run_ccd) in plain
Python floats: the classified distances of stark_amd/csrc/contact_geom.hpp, the parallel-safe edge-edge distance, additive CCD (Li, Kaufman,
Jiang 2021, Alg. 1, minimum distance 0) and the swept-box candidate set. The test oracle of tests/test_ccd_cpu.py and tests/test_gpu_ccd.py."""
import math

import numpy as np

MAX_ITERATIONS = 10000


def _sub(a, b):
    return (a[0] - b[0], a[1] - b[1], a[2] - b[2])


def _add(a, b):
    return (a[0] + b[0], a[1] + b[1], a[2] + b[2])


def _scale(s, a):
    return (s * a[0], s * a[1], s * a[2])


def _dot(a, b):
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]


def _cross(a, b):
    return (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])


def _sq(a):
    return _dot(a, a)


def point_line_sq(p, e0, e1):
    return _sq(_cross(_sub(e0, p), _sub(e1, p))) / _sq(_sub(e1, e0))


def _edge_param(p, e0, e1, n):
    b0, d = _sub(e1, e0), _sub(p, e0)
    return _dot(b0, d) / _sq(b0), _dot(_cross(b0, n), d)


def point_triangle_sq(p, t0, t1, t2):
    n = _cross(_sub(t1, t0), _sub(t2, t0))
    a0, c0 = _edge_param(p, t0, t1, n)
    if 0.0 < a0 < 1.0 and c0 >= 0.0:
        return point_line_sq(p, t0, t1)
    a1, c1 = _edge_param(p, t1, t2, n)
    if 0.0 < a1 < 1.0 and c1 >= 0.0:
        return point_line_sq(p, t1, t2)
    a2, c2 = _edge_param(p, t2, t0, n)
    if 0.0 < a2 < 1.0 and c2 >= 0.0:
        return point_line_sq(p, t2, t0)
    if a0 <= 0.0 and a2 >= 1.0:
        return _sq(_sub(t0, p))
    if a1 <= 0.0 and a0 >= 1.0:
        return _sq(_sub(t1, p))
    if a2 <= 0.0 and a1 >= 1.0:
        return _sq(_sub(t2, p))
    h = _dot(_sub(p, t0), n)
    return h * h / _sq(n)


def edge_edge_sq(ea0, ea1, eb0, eb1):
    u, v, w = _sub(ea1, ea0), _sub(eb1, eb0), _sub(ea0, eb0)
    a, b, c, d, e = _sq(u), _dot(u, v), _sq(v), _dot(u, w), _dot(v, w)
    D = a * c - b * b
    sN = b * e - c * d
    kind = "ee"
    if sN <= 0.0:
        tN, tD, kind = e, c, "a0"
    elif sN >= D:
        tN, tD, kind = e + b, c, "a1"
    else:
        tN, tD = a * e - b * d, D
    if tN <= 0.0:
        if -d <= 0.0:
            return _sq(_sub(eb0, ea0))
        if -d >= a:
            return _sq(_sub(eb0, ea1))
        return point_line_sq(eb0, ea0, ea1)
    if tN >= tD:
        if (-d + b) <= 0.0:
            return _sq(_sub(eb1, ea0))
        if (-d + b) >= a:
            return _sq(_sub(eb1, ea1))
        return point_line_sq(eb1, ea0, ea1)
    if kind == "a0":
        return point_line_sq(ea0, eb0, eb1)
    if kind == "a1":
        return point_line_sq(ea1, eb0, eb1)
    n = _cross(u, v)
    h = _dot(_sub(eb0, ea0), n)
    return h * h / _sq(n)


def point_segment_sq(p, e0, e1):
    e = _sub(e1, e0)
    ee = _sq(e)
    t = _dot(_sub(p, e0), e) / ee if ee > 0.0 else 0.0
    t = 0.0 if t < 0.0 else (1.0 if t > 1.0 else t)
    return _sq(_sub(p, _add(e0, _scale(t, e))))


def distance(ee, x):
    """Point x[0] - triangle x[1:4] (ee False) or edge x[0:2] - edge x[2:4]; nearly parallel edges: the smallest point-edge distance."""
    if not ee:
        return math.sqrt(point_triangle_sq(*x))
    u, v = _sub(x[1], x[0]), _sub(x[3], x[2])
    uv = _sq(u) * _sq(v)
    if _sq(_cross(u, v)) < 1e-20 * max(uv, 1.0):
        a = min(point_segment_sq(x[0], x[2], x[3]), point_segment_sq(x[1], x[2], x[3]))
        b = min(point_segment_sq(x[2], x[0], x[1]), point_segment_sq(x[3], x[0], x[1]))
        return math.sqrt(min(a, b))
    return math.sqrt(edge_edge_sq(*x))


def _prepare(ee, xa, xb):
    x = [tuple(float(c) for c in p) for p in xa]
    dx = [_sub(tuple(float(c) for c in q), p) for p, q in zip(x, xb)]
    mean = _scale(0.25, _add(_add(_add(dx[0], dx[1]), dx[2]), dx[3]))
    dx = [_sub(d, mean) for d in dx]
    s = [_sq(d) for d in dx]
    lp = math.sqrt(s[0]) + math.sqrt(max(s[1], s[2], s[3])) if not ee else math.sqrt(max(s[0], s[1])) + math.sqrt(max(s[2], s[3]))
    return x, dx, lp


def accd(ee, xa, xb, eta=0.9, t_c=1.0):
    """Additive CCD of one pair moving linearly from xa to xb (4 points each). Returns a dict: status ("hit", "none", "touching", "filtered",
    "capped"), toi (the reported lower bound), t_stop (where the stop test fired: d(t_stop) < (1 - eta) d(0)), d0, iterations."""
    x, dx, lp = _prepare(ee, xa, xb)
    d = distance(ee, x)
    out = dict(status="none", toi=1.0, t_stop=None, d0=d, iterations=0)
    if not d > 0.0:
        out["status"] = "touching"
        return out
    if not lp > eta * d:
        out["status"] = "filtered"
        return out
    gap = (1.0 - eta) * d
    t = 0.0
    it = 0
    while True:
        step = eta * d / lp
        x = [_add(p, _scale(step, q)) for p, q in zip(x, dx)]
        d = distance(ee, x)
        if t > 0.0 and d < gap:
            out.update(status="hit", toi=t, t_stop=t + step, iterations=it + 1)
            return out
        t += step
        if t > t_c:
            out["iterations"] = it + 1
            return out
        it += 1
        if it == MAX_ITERATIONS:
            out.update(status="capped", toi=t, iterations=it)
            return out


def last_step(ee, xa, xb, eta, toi):
    """The ACCD increment taken at the reported toi (the amount a tie in the stop test can move the answer by)."""
    x, dx, lp = _prepare(ee, xa, xb)
    d = distance(ee, x)
    t = 0.0
    while True:
        step = eta * d / lp
        if t >= toi:
            return step
        x = [_add(p, _scale(step, q)) for p, q in zip(x, dx)]
        d = distance(ee, x)
        t += step


# ---- candidate set: swept float boxes rounded outwards, the barrier search's exclusions ----------------------------------------------------
def _round_down(v):
    f = v.astype(np.float32)
    return np.where(f.astype(np.float64) > v, np.nextafter(f, np.float32(-np.inf)), f)


def _round_up(v):
    f = v.astype(np.float32)
    return np.where(f.astype(np.float64) < v, np.nextafter(f, np.float32(np.inf)), f)


def swept_boxes(xa, xb, prims):
    """prims: [n, k] vertex indices -> (lo, hi) float32 [n, 3]"""
    pts = np.concatenate([xa[prims], xb[prims]], axis=1)
    return _round_down(pts.min(axis=1)), _round_up(pts.max(axis=1))


def _overlap(lo_a, hi_a, lo_b, hi_b):
    return np.all((lo_a[:, None, :] <= hi_b[None, :, :]) & (lo_b[None, :, :] <= hi_a[:, None, :]), axis=2)


def candidates(xa, xb, tris, edges, point_triangle=True, edge_edge=True):
    """Brute force: (point, triangle) pairs and (edge a < edge b) pairs whose swept boxes overlap, minus points of their own triangle and
    edges sharing a vertex (one mesh set, no blacklists)."""
    nv = len(xa)
    pt, ee = np.zeros((0, 2), int), np.zeros((0, 2), int)
    if point_triangle and len(tris):
        plo, phi = swept_boxes(xa, xb, np.arange(nv)[:, None])
        tlo, thi = swept_boxes(xa, xb, tris)
        m = _overlap(plo, phi, tlo, thi)
        m &= ~np.any(np.arange(nv)[:, None, None] == tris[None, :, :], axis=2)
        pt = np.argwhere(m)
    if edge_edge and len(edges) > 1:
        elo, ehi = swept_boxes(xa, xb, edges)
        m = _overlap(elo, ehi, elo, ehi)
        m &= np.triu(np.ones((len(edges), len(edges)), bool), 1)
        share = np.zeros_like(m)
        for i in range(2):
            for j in range(2):
                share |= edges[:, i][:, None] == edges[:, j][None, :]
        m &= ~share
        ee = np.argwhere(m)
    return pt, ee


def max_step(xa, xb, tris, edges, eta=0.9):
    """The query over a whole scene: min(1, every candidate's ACCD toi). Returns (toi, n_candidates)."""
    pt, ee = candidates(xa, xb, tris, edges)
    best = 1.0
    for p, t in pt:
        v = [p, *tris[t]]
        r = accd(False, xa[v], xb[v], eta, best)
        if r["status"] in ("hit", "capped"):
            best = min(best, r["toi"])
    for a, b in ee:
        v = [*edges[a], *edges[b]]
        r = accd(True, xa[v], xb[v], eta, best)
        if r["status"] in ("hit", "capped"):
            best = min(best, r["toi"])
    return best, len(pt) + len(ee)
