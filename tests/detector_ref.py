"""Reference of the standalone collision detector (include/mistark_tmcd.h) for synthesised meshes: plain Python and numpy, no GPU.

Two layers:
  * EXACT PREDICATES on `fractions.Fraction`: point-triangle and edge-edge closest feature and squared distance (with the parallel cutoff) and
    the edge-triangle intersection predicate, with the comparisons and the strictness that the header of stark_amd/csrc/contact_geom.hpp and
    include/mistark_tmcd.h document, evaluated in exact rationals. Doubles are rationals with a power-of-two denominator, so the inputs are
    scaled by one common power of two and the polynomials are evaluated on Python integers (exact, and far quicker than Fraction objects);
    quotients are never formed before a comparison (a / b < 1 is decided as a < b), squared distances come back as Fraction.
  * BRUTE-FORCE LISTS over all primitive pairs of a list of meshes, independent of any box broad phase: a float64 bounding-SPHERE bound
    (distance of the centres minus the radii, evaluated for every pair, in chunks) discards the pairs that are certainly farther than
    1.05 enlargement; the float64 restatement of oracle/contact.py classifies the rest; every pair with d < 1.05 enlargement (or without a
    finite float64 distance) is then decided again by the exact predicates, and only the exact decision enters a list.

UNDECIDABLE PAIRS. The device rounds (possibly with fused multiply-adds), so a pair within rounding of a threshold has no single right answer.
Every comparator the decision evaluated — the three along / across values, sN, tN, -d, -d + b against their bounds, d^2 against enl^2, cross^2
against 1e-30, det, t, u, v, u + v — is measured against the magnitude of the terms compared (the sum of the absolute values of the products
that were added up, propagated through the cross and dot products): a comparator within relative UNDECIDABLE_REL = 1e-9 of its threshold makes
the pair undecidable. Such pairs are left out of set comparisons (present, absent or of either type); tests cap their number at
undecidable_cap(): 0.1 % of the reference's hits, never more than 5. Inputs on a binary lattice for which all products are exact in double
(`exact_inputs=True`) have nothing undecidable: an exact tie is then a decision the device has to reproduce.
"""
import math
from fractions import Fraction

import numpy as np

from oracle import contact as oc

LISTS = ("pt_point_point", "pt_point_edge", "pt_point_triangle", "ee_point_point", "ee_point_edge", "ee_edge_edge")
COLS = (8, 9, 7, 10, 9, 8)
UNDECIDABLE_REL = 10 ** 9   # a comparator is near its threshold when |value - threshold| * 1e9 < magnitude
EE_CUTOFF = Fraction(oc.EE_PARALLEL_CUTOFF)   # the double 1e-30, exactly
DET_MIN = Fraction(1e-14)
CHUNK = 2_000_000
P_T0, P_T1, P_T2, P_E0, P_E1, P_E2, P_T = range(7)
EA0_EB0, EA0_EB1, EA1_EB0, EA1_EB1, EA_EB0, EA_EB1, EA0_EB, EA1_EB, EA_EB = range(9)


def undecidable_cap(n_hits):
    return min(5, n_hits // 1000)


# ---- exact integer vectors ---------------------------------------------------------------------------------------------------------------
def _scaled(points):
    """rows of 3 doubles or Fractions -> (rows of 3 Python ints, S) with int / S = the coordinate; S a common denominator (a power of two for doubles)"""
    fr = [tuple(c if isinstance(c, Fraction) else Fraction(float(c)) for c in p) for p in points]
    S = 1
    for p in fr:
        for c in p:
            if c.denominator > S:
                S = S * c.denominator // math.gcd(S, c.denominator)
    return [tuple(int(c * S) for c in p) for p in fr], S


def _sub(a, b):
    return (a[0] - b[0], a[1] - b[1], a[2] - b[2])


def _dot(a, b):
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]


def _adot(a, b):
    return abs(a[0] * b[0]) + abs(a[1] * b[1]) + abs(a[2] * b[2])


def _abs3(a):
    return (abs(a[0]), abs(a[1]), abs(a[2]))


def _cross(a, b):
    return (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])


def _crossmag(am, bm):
    """magnitude of the terms of a cross product from the magnitudes of its factors"""
    return (am[1] * bm[2] + am[2] * bm[1], am[2] * bm[0] + am[0] * bm[2], am[0] * bm[1] + am[1] * bm[0])


class _Near:
    """collects whether any evaluated comparator lay within UNDECIDABLE_REL of its threshold"""
    __slots__ = ("near", "ties")

    def __init__(self):
        self.near = False
        self.ties = set()   # names of the comparators that sat exactly on their threshold

    def __call__(self, value, mag, tag=None):
        # value = (quantity - threshold), mag = magnitude of the terms on both sides
        if abs(value) * UNDECIDABLE_REL < mag or (value == 0 and mag == 0):
            self.near = True
        if value == 0 and tag is not None:
            self.ties.add(tag)
        return value


def _point_line(p, e0, e1):
    """(numerator, magnitude of its terms, denominator) of |(e0 - p) x (e1 - p)|^2 / |e1 - e0|^2"""
    a, b = _sub(e0, p), _sub(e1, p)
    c = _cross(a, b)
    cm = _crossmag(_abs3(a), _abs3(b))
    return _dot(c, c), 2 * _dot(_abs3(c), cm) + _dot(c, c), _dot(_sub(e1, e0), _sub(e1, e0))


def _pt_int(p, t0, t1, t2, near):
    """type, (num, nummag, den) of d^2 on scaled integers"""
    e01, e02 = _sub(t1, t0), _sub(t2, t0)
    n = _cross(e01, e02)
    nm = _crossmag(_abs3(e01), _abs3(e02))

    def edge_param(e0, e1):
        b0, d = _sub(e1, e0), _sub(p, e0)
        num, den, numm = _dot(b0, d), _dot(b0, b0), _adot(b0, d)
        if den == 0:
            raise ValueError("degenerate triangle edge")
        b1 = _cross(b0, n)
        b1m = _crossmag(_abs3(b0), nm)
        return num, den, numm, _dot(b1, d), _dot(b1m, _abs3(d))

    def on_edge(q):
        num, den, numm, acr, acrm = q
        return near(num, numm, "along==0") > 0 and near(num - den, numm + den, "along==1") < 0 and near(acr, acrm, "across==0") >= 0

    def le0(q):   # along <= 0
        return near(q[0], q[2], "along==0") <= 0

    def ge1(q):   # along >= 1
        return near(q[0] - q[1], q[2] + q[1], "along==1") >= 0

    q0 = edge_param(t0, t1)
    if on_edge(q0):
        ty = P_E0
    else:
        q1 = edge_param(t1, t2)
        if on_edge(q1):
            ty = P_E1
        else:
            q2 = edge_param(t2, t0)
            if on_edge(q2):
                ty = P_E2
            elif le0(q0) and ge1(q2):
                ty = P_T0
            elif le0(q1) and ge1(q0):
                ty = P_T1
            elif le0(q2) and ge1(q1):
                ty = P_T2
            else:
                ty = P_T
    if ty <= P_T2:
        v = _sub((t0, t1, t2)[ty], p)
        return ty, (_dot(v, v), _dot(v, v), 1)
    if ty <= P_E2:
        k = ty - P_E0
        return ty, _point_line(p, (t0, t1, t2)[k], (t0, t1, t2)[(k + 1) % 3])
    d = _sub(p, t0)
    h, hm = _dot(d, n), _dot(_abs3(d), nm)
    return ty, (h * h, 2 * abs(h) * hm + h * h, _dot(n, n))


def _ee_int(ea0, ea1, eb0, eb1, near, cutoff_scaled):
    """type (None: dropped by the parallel cutoff), (num, nummag, den) of d^2 on scaled integers"""
    u, v, w = _sub(ea1, ea0), _sub(eb1, eb0), _sub(ea0, eb0)
    n = _cross(u, v)
    nm = _crossmag(_abs3(u), _abs3(v))
    cross2 = _dot(n, n)
    if near(cross2 - cutoff_scaled, 2 * _dot(_abs3(n), nm) + cross2 + cutoff_scaled) <= 0:
        return None, None
    a, b, c, d, e = _dot(u, u), _dot(u, v), _dot(v, v), _dot(u, w), _dot(v, w)
    bm, dm, em = _adot(u, v), _adot(u, w), _adot(v, w)
    D, Dm = a * c - b * b, a * c + bm * bm
    sN, sNm = b * e - c * d, bm * em + c * dm
    if near(sN, sNm, "sN==0") <= 0:
        tN, tNm, tD, tDm, default = e, em, c, c, EA0_EB
    elif near(sN - D, sNm + Dm, "sN==D") >= 0:
        tN, tNm, tD, tDm, default = e + b, em + bm, c, c, EA1_EB
    else:
        tN, tNm, tD, tDm, default = a * e - b * d, a * em + bm * dm, D, Dm, EA_EB
    if near(tN, tNm, "tN==0") <= 0:
        if near(-d, dm, "-d==0") <= 0:
            ty = EA0_EB0
        elif near(-d - a, dm + a, "-d==a") >= 0:
            ty = EA1_EB0
        else:
            ty = EA_EB0
    elif near(tN - tD, tNm + tDm, "tN==tD") >= 0:
        if near(-d + b, dm + bm, "-d+b==0") <= 0:
            ty = EA0_EB1
        elif near(-d + b - a, dm + bm + a, "-d+b==a") >= 0:
            ty = EA1_EB1
        else:
            ty = EA_EB1
    else:
        ty = default
    if ty <= EA1_EB1:
        x = _sub((eb0, eb1)[ty % 2], (ea0, ea1)[ty // 2])
        return ty, (_dot(x, x), _dot(x, x), 1)
    if ty == EA_EB0:
        return ty, _point_line(eb0, ea0, ea1)
    if ty == EA_EB1:
        return ty, _point_line(eb1, ea0, ea1)
    if ty == EA0_EB:
        return ty, _point_line(ea0, eb0, eb1)
    if ty == EA1_EB:
        return ty, _point_line(ea1, eb0, eb1)
    x = _sub(eb0, ea0)
    h, hm = _dot(x, n), _dot(_abs3(x), nm)
    return ty, (h * h, 2 * abs(h) * hm + h * h, cross2)


def _hit(q, enl2_scaled, near):
    """d^2 < enl^2 (strict) on (num, nummag, den), enl^2 already multiplied by the square of the scale"""
    num, numm, den = q
    return near(num - enl2_scaled * den, numm + enl2_scaled * den, "d2==enl2") < 0


def point_triangle_exact(p, t0, t1, t2, ties=None):
    """-> (type, d^2 as Fraction, near): inputs rows of 3 doubles or Fractions; `ties`: a set that receives the names of the comparators that sat
    exactly on their threshold"""
    (p, t0, t1, t2), S = _scaled([p, t0, t1, t2])
    near = _Near()
    ty, (num, _, den) = _pt_int(p, t0, t1, t2, near)
    if ties is not None:
        ties |= near.ties
    return ty, Fraction(num, den * S * S), near.near


def edge_edge_exact(ea0, ea1, eb0, eb1, ties=None):
    """-> (type or None when |u x v|^2 <= 1e-30, d^2 as Fraction or None, near); `ties` as in point_triangle_exact"""
    (ea0, ea1, eb0, eb1), S = _scaled([ea0, ea1, eb0, eb1])
    near = _Near()
    ty, q = _ee_int(ea0, ea1, eb0, eb1, near, EE_CUTOFF * S ** 4)
    if ties is not None:
        ties |= near.ties
    if ty is None:
        return None, None, near.near
    return ty, Fraction(q[0], q[2] * S * S), near.near


def edge_cross2_exact(ea0, ea1, eb0, eb1):
    (ea0, ea1, eb0, eb1), S = _scaled([ea0, ea1, eb0, eb1])
    n = _cross(_sub(ea1, ea0), _sub(eb1, eb0))
    return Fraction(_dot(n, n), S ** 4)


def edge_triangle_exact(q1, q2, a, b, c):
    """-> (intersects, near, det as Fraction): fabs(det) >= 1e-14 && 0 <= t <= 1 && u >= 0 && v >= 0 && u + v <= 1 with t, u, v = numerators / det"""
    (q1, q2, a, b, c), S = _scaled([q1, q2, a, b, c])
    e1, e2 = _sub(b, a), _sub(c, a)
    n = _cross(e1, e2)
    nm = _crossmag(_abs3(e1), _abs3(e2))
    dr = _sub(q2, q1)
    det, detm = -_dot(dr, n), _dot(_abs3(dr), nm)
    det_f = Fraction(det, S ** 3)
    lim = DET_MIN * S ** 3
    clear_fail = False
    nears = []

    def check(value, mag, ok):
        # one conjunct: `ok` its truth; a clearly failing one decides the pair whatever the others do
        nonlocal clear_fail
        is_near = abs(value) * UNDECIDABLE_REL < mag
        nears.append(is_near)
        if not ok and not is_near:
            clear_fail = True
        return ok

    res = check(abs(det) - lim, detm + lim, abs(det) >= lim)
    if det != 0:
        s = 1 if det > 0 else -1
        ao = _sub(q1, a)
        dao = _cross(ao, dr)
        daom = _crossmag(_abs3(ao), _abs3(dr))
        un, unm = _dot(e2, dao) * s, _dot(_abs3(e2), daom)
        vn, vnm = -_dot(e1, dao) * s, _dot(_abs3(e1), daom)
        tn, tnm = _dot(ao, n) * s, _dot(_abs3(ao), nm)
        ad = abs(det)
        res &= check(tn, tnm, tn >= 0)
        res &= check(tn - ad, tnm + detm, tn <= ad)
        res &= check(un, unm, un >= 0)
        res &= check(vn, vnm, vn >= 0)
        res &= check(un + vn - ad, unm + vnm + detm, un + vn <= ad)
    else:
        res = False
    return bool(res), (not clear_fail) and any(nears), det_f


# ---- scenes ---------------------------------------------------------------------------------------------------------------------------------
class Scene:
    """meshes: list of (X [nv, 3] float64, triangles [nt, 3], edges [ne, 2]); blacklists as the detector takes them"""

    def __init__(self, meshes):
        self.meshes = [(np.ascontiguousarray(x, dtype=np.float64), np.asarray(t, dtype=np.int64).reshape(-1, 3), np.asarray(e, dtype=np.int64).reshape(-1, 2)) for x, t, e in meshes]
        self.disabled = set()   # (a, b), both orders
        self.bl_pt = []         # (mesh_a, (a0, a1), mesh_b, (b0, b1)): points x triangles
        self.bl_ee = []         # (mesh_a, (a0, a1), mesh_b, (b0, b1)): lower edges x higher edges

    def blacklist(self, a, b):
        self.disabled.add((a, b))
        self.disabled.add((b, a))

    def X(self):
        return [m[0] for m in self.meshes]

    def counts(self):
        return (sum(len(m[0]) for m in self.meshes), sum(len(m[1]) for m in self.meshes), sum(len(m[2]) for m in self.meshes))

    def register(self, cd):
        """the same scene in a capi.CollisionDetector"""
        for x, t, e in self.meshes:
            cd.add_mesh(x, t, e)
        for a, b in sorted(self.disabled):
            if a <= b:
                cd.add_blacklist(a, b)
        for ma, ia, mb, ib in self.bl_pt:
            cd.add_blacklist_range(False, ma, ia, mb, ib)
        for ma, ia, mb, ib in self.bl_ee:
            cd.add_blacklist_range(True, ma, ia, mb, ib)
        return cd

    def oracle_scene(self):
        sc = oc.ContactScene([oc.Mesh("d", k, np.arange(len(x)), t, e, 1e300) for k, (x, t, e) in enumerate(self.meshes)])
        sc.disabled = {(min(a, b), max(a, b)) for a, b in self.disabled}
        return sc

    def flat(self):
        """global primitive arrays: dict with P [np,3], pm, pi | tri vertex positions T [nt,3,3], tm, ti, tv | E [ne,2,3], em, ei, ev"""
        M = self.meshes
        g = {}
        g["P"] = np.concatenate([m[0] for m in M]).reshape(-1, 3)
        g["pm"] = np.concatenate([np.full(len(m[0]), k, dtype=np.int64) for k, m in enumerate(M)])
        g["pi"] = np.concatenate([np.arange(len(m[0]), dtype=np.int64) for m in M])
        g["T"] = np.concatenate([m[0][m[1]] for m in M]).reshape(-1, 3, 3)
        g["tm"] = np.concatenate([np.full(len(m[1]), k, dtype=np.int64) for k, m in enumerate(M)])
        g["ti"] = np.concatenate([np.arange(len(m[1]), dtype=np.int64) for m in M])
        g["tv"] = np.concatenate([m[1] for m in M]).reshape(-1, 3)
        g["E"] = np.concatenate([m[0][m[2]] for m in M]).reshape(-1, 2, 3)
        g["em"] = np.concatenate([np.full(len(m[2]), k, dtype=np.int64) for k, m in enumerate(M)])
        g["ei"] = np.concatenate([np.arange(len(m[2]), dtype=np.int64) for m in M])
        g["ev"] = np.concatenate([m[2] for m in M]).reshape(-1, 2)
        nm = len(M)
        g["dis"] = np.zeros((nm, nm), dtype=bool)
        for a, b in self.disabled:
            g["dis"][a, b] = True
        return g


def _sphere_pairs(CA, RA, CB, RB, reach, upper):
    """all pairs (i, j) (j > i when `upper`) whose bounding spheres come closer than `reach`: float64, every pair evaluated, chunked"""
    out_i, out_j = [], []
    if len(CA) == 0 or len(CB) == 0:
        return np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64)
    rows = max(1, CHUNK // len(CB))
    for r0 in range(0, len(CA), rows):
        r1 = min(len(CA), r0 + rows)
        dist = np.sqrt(((CA[r0:r1, None, :] - CB[None, :, :]) ** 2).sum(axis=2))
        lim = RA[r0:r1, None] + RB[None, :] + reach
        keep = dist <= lim * (1.0 + 1e-9) + 1e-300
        if upper:
            keep &= np.arange(r0, r1)[:, None] < np.arange(len(CB))[None, :]
        i, j = np.nonzero(keep)
        out_i.append(i + r0)
        out_j.append(j)
    return np.concatenate(out_i), np.concatenate(out_j)


def _sphere(V):
    """[n, k, 3] vertex positions -> centres, radii"""
    c = V.mean(axis=1)
    return c, np.sqrt(((V - c[:, None, :]) ** 2).sum(axis=2)).max(axis=1) * (1.0 + 1e-12)


def _in_ranges(bl, ma, ia, mb, ib):
    for (ra, (a0, a1), rb, (b0, b1)) in bl:
        if ma == ra and a0 <= ia < a1 and mb == rb and b0 <= ib < b1:
            return True
    return False


class Proximity:
    """result of proximity(): rows[name] int64 [n, cols] (lexsorted), dist[name] the exact distances (correctly rounded), span[name] the largest
    coordinate difference among the pair's vertices, und_pt / und_ee the undecidable pairs as (set, idx, set, idx) keys (edge pairs: lower global
    edge first), n_hits the number of rows"""

    def __init__(self, rows, dist, span, und_pt, und_ee):
        self.rows, self.dist, self.span, self.und_pt, self.und_ee = rows, dist, span, und_pt, und_ee
        self.n_hits = sum(len(r) for r in rows.values())


def pt_key(rows):
    return [tuple(r[:4]) for r in np.asarray(rows).tolist()]


def ee_key(rows, name):
    j = 4 if name == "ee_edge_edge" else 5
    out = []
    for r in np.asarray(rows).tolist():
        a, b = (r[0], r[1]), (r[j], r[j + 1])
        out.append(a + b if a < b else b + a)
    return out


def row_keys(rows, name):
    return pt_key(rows) if name.startswith("pt_") else ee_key(rows, name)


def proximity(scene, enl, point_triangle=True, edge_edge=True, exact_inputs=False):
    g = scene.flat()
    reach = 1.05 * enl
    enl2 = Fraction(float(enl)) ** 2
    rows = {n: [] for n in LISTS}
    dist = {n: [] for n in LISTS}
    span = {n: [] for n in LISTS}
    und_pt, und_ee = set(), set()
    if point_triangle and len(g["T"]) and len(g["P"]) and enl > 0:
        ct, rt = _sphere(g["T"])
        ip, it = _sphere_pairs(g["P"], np.zeros(len(g["P"])), ct, rt, reach, False)
        keep = ~((g["pm"][ip] == g["tm"][it]) & (g["pi"][ip][:, None] == g["tv"][it]).any(axis=1)) & ~g["dis"][g["pm"][ip], g["tm"][it]]
        ip, it = ip[keep], it[keep]
        with np.errstate(all="ignore"):
            _, d2 = oc.point_triangle_sq_distance(g["P"][ip], g["T"][it, 0], g["T"][it, 1], g["T"][it, 2])
        sel = ~(d2 >= reach * reach)
        for p, t in zip(ip[sel].tolist(), it[sel].tolist()):
            pm, pi, tm, ti = int(g["pm"][p]), int(g["pi"][p]), int(g["tm"][t]), int(g["ti"][t])
            if _in_ranges(scene.bl_pt, pm, pi, tm, ti):
                continue
            pts, S = _scaled([g["P"][p], g["T"][t, 0], g["T"][t, 1], g["T"][t, 2]])
            near = _Near()
            ty, q = _pt_int(pts[0], pts[1], pts[2], pts[3], near)
            hit = _hit(q, enl2 * S * S, near)
            if near.near and not exact_inputs:
                und_pt.add((pm, pi, tm, ti))
                continue
            if not hit:
                continue
            tv = [int(v) for v in g["tv"][t]]
            head = [pm, pi, tm, ti] + tv
            if ty <= P_T2:
                name, row = LISTS[0], head + [tv[ty]]
            elif ty <= P_E2:
                name, row = LISTS[1], head + [tv[ty - 3], tv[(ty - 2) % 3]]
            else:
                name, row = LISTS[2], head
            rows[name].append(row)
            dist[name].append(math.sqrt(Fraction(q[0], q[2] * S * S)))
            V = np.concatenate([g["P"][p][None], g["T"][t]])
            span[name].append(float((V.max(axis=0) - V.min(axis=0)).max()))
    if edge_edge and len(g["E"]) > 1 and enl > 0:
        ce, re = _sphere(g["E"])
        ia, ib = _sphere_pairs(ce, re, ce, re, reach, True)
        ev = g["ev"]
        share = (ev[ia, 0] == ev[ib, 0]) | (ev[ia, 0] == ev[ib, 1]) | (ev[ia, 1] == ev[ib, 0]) | (ev[ia, 1] == ev[ib, 1])
        keep = ~((g["em"][ia] == g["em"][ib]) & share) & ~g["dis"][g["em"][ia], g["em"][ib]]
        ia, ib = ia[keep], ib[keep]
        with np.errstate(all="ignore"):
            _, d2 = oc.edge_edge_sq_distance(g["E"][ia, 0], g["E"][ia, 1], g["E"][ib, 0], g["E"][ib, 1])
        sel = ~(d2 >= reach * reach)
        for a, b in zip(ia[sel].tolist(), ib[sel].tolist()):
            am, ai, bm, bi = int(g["em"][a]), int(g["ei"][a]), int(g["em"][b]), int(g["ei"][b])
            if _in_ranges(scene.bl_ee, am, ai, bm, bi):
                continue
            pts, S = _scaled([g["E"][a, 0], g["E"][a, 1], g["E"][b, 0], g["E"][b, 1]])
            near = _Near()
            ty, q = _ee_int(pts[0], pts[1], pts[2], pts[3], near, EE_CUTOFF * S ** 4)
            hit = ty is not None and _hit(q, enl2 * S * S, near)
            if near.near and not exact_inputs:
                und_ee.add((am, ai, bm, bi))
                continue
            if not hit:
                continue
            A = [am, ai, int(ev[a, 0]), int(ev[a, 1])]
            B = [bm, bi, int(ev[b, 0]), int(ev[b, 1])]
            if ty <= 3:
                name, row = LISTS[3], A + [A[2 + ty // 2]] + B + [B[2 + ty % 2]]
            elif ty <= 5:   # the point lies on edge b: b comes first
                name, row = LISTS[4], B + [B[2 + ty - 4]] + A
            elif ty <= 7:
                name, row = LISTS[4], A + [A[2 + ty - 6]] + B
            else:
                name, row = LISTS[5], A + B
            rows[name].append(row)
            dist[name].append(math.sqrt(Fraction(q[0], q[2] * S * S)))
            V = np.concatenate([g["E"][a], g["E"][b]])
            span[name].append(float((V.max(axis=0) - V.min(axis=0)).max()))
    out_rows, out_dist, out_span = {}, {}, {}
    for l, n in enumerate(LISTS):
        r = np.array(rows[n], dtype=np.int64).reshape(-1, COLS[l])
        o = np.lexsort(r.T[::-1]) if len(r) else np.zeros(0, dtype=np.int64)
        out_rows[n] = r[o]
        out_dist[n] = np.array(dist[n], dtype=np.float64)[o]
        out_span[n] = np.array(span[n], dtype=np.float64)[o]
    return Proximity(out_rows, out_dist, out_span, und_pt, und_ee)


def only(ref, point_triangle=True, edge_edge=True):
    """a copy of proximity()'s result with one family's three lists emptied (what activate(...) leaves)"""
    rows, dist, span = {}, {}, {}
    for n in LISTS:
        on = point_triangle if n.startswith("pt_") else edge_edge
        rows[n] = ref.rows[n] if on else ref.rows[n][:0]
        dist[n] = ref.dist[n] if on else ref.dist[n][:0]
        span[n] = ref.span[n] if on else ref.span[n][:0]
    return Proximity(rows, dist, span, ref.und_pt, ref.und_ee)


def intersections(scene, exact_inputs=False):
    """-> (rows [n, 9] int64 lexsorted: edge set idx v0 v1 | triangle set idx v0 v1 v2, undecidable {(eset, eidx, tset, tidx)})"""
    g = scene.flat()
    und = set()
    out = []
    if len(g["E"]) and len(g["T"]):
        ce, re = _sphere(g["E"])
        ct, rt = _sphere(g["T"])
        ie, it = _sphere_pairs(ce, re, ct, rt, 0.0, False)
        ev, tv = g["ev"], g["tv"]
        share = (ev[ie, 0][:, None] == tv[it]).any(axis=1) | (ev[ie, 1][:, None] == tv[it]).any(axis=1)
        keep = ~((g["em"][ie] == g["tm"][it]) & share) & ~g["dis"][g["em"][ie], g["tm"][it]]
        ie, it = ie[keep], it[keep]
        # float64 restatement: everything within 1e-6 of the closed parameter domain (or without finite parameters) is decided exactly
        q1, q2, a, b, c = g["E"][ie, 0], g["E"][ie, 1], g["T"][it, 0], g["T"][it, 1], g["T"][it, 2]
        e1, e2 = b - a, c - a
        n = np.cross(e1, e2)
        dr = q2 - q1
        with np.errstate(all="ignore"):
            det = -(dr * n).sum(axis=1)
            inv = 1.0 / det
            ao = q1 - a
            dao = np.cross(ao, dr)
            u = (e2 * dao).sum(axis=1) * inv
            v = -(e1 * dao).sum(axis=1) * inv
            t = (ao * n).sum(axis=1) * inv
            tol = 1e-6
            out_of_reach = (t < -tol) | (t > 1 + tol) | (u < -tol) | (v < -tol) | (u + v > 1 + tol)
            if exact_inputs:   # products are exact in double: det == 0.0 IS coplanar, which never intersects
                out_of_reach |= det == 0.0
        for e, tr in zip(ie[~out_of_reach].tolist(), it[~out_of_reach].tolist()):
            hit, near, _ = edge_triangle_exact(g["E"][e, 0], g["E"][e, 1], g["T"][tr, 0], g["T"][tr, 1], g["T"][tr, 2])
            key = (int(g["em"][e]), int(g["ei"][e]), int(g["tm"][tr]), int(g["ti"][tr]))
            if near and not exact_inputs:
                und.add(key)
            elif hit:
                out.append([key[0], key[1], int(ev[e, 0]), int(ev[e, 1]), key[2], key[3]] + [int(x) for x in tv[tr]])
    r = np.array(out, dtype=np.int64).reshape(-1, 9)
    return (r[np.lexsort(r.T[::-1])] if len(r) else r), und


def et_key(rows):
    return [(r[0], r[1], r[4], r[5]) for r in np.asarray(rows).tolist()]


def broad_phase(scene, enl, point_triangle=True, edge_edge=True):
    """oracle/contact.py broad_phase (boxes as the reference builds them) minus the range blacklists: (point-triangle rows, edge-edge rows), sorted"""
    pt, ee = oc.broad_phase(scene.oracle_scene(), scene.X(), enl)
    if scene.bl_pt:
        pt = np.array([r for r in pt.tolist() if not _in_ranges(scene.bl_pt, *r)], dtype=np.int64).reshape(-1, 4)
    if scene.bl_ee:
        ee = np.array([r for r in ee.tolist() if not _in_ranges(scene.bl_ee, *r)], dtype=np.int64).reshape(-1, 4)
    return (pt if point_triangle else pt[:0]), (ee if edge_edge else ee[:0])


# ---- comparison ---------------------------------------------------------------------------------------------------------------------------
DIST_ROUNDINGS = 32   # |d_dev - d_exact| <= 32 * 2^-53 * L (L = the pair's largest coordinate difference): ~20 operations, one rounding of size L each


def without(rows, keys, und, extra=None):
    """rows (and a parallel array) minus those whose pair key is undecidable"""
    rows = np.asarray(rows, dtype=np.int64)
    m = np.array([k not in und for k in keys], dtype=bool).reshape(-1)
    return (rows[m], None if extra is None else np.asarray(extra)[m])


def sorted_rows(rows, extra=None):
    rows = np.asarray(rows, dtype=np.int64)
    if len(rows) == 0:
        return rows, extra
    o = np.lexsort(rows.T[::-1])
    return rows[o], None if extra is None else np.asarray(extra)[o]


def check_proximity(got, ref, dist_tol=None):
    """`got` = capi.CollisionDetector.run_proximity(), `ref` = proximity(): row sets equal apart from the undecidable pairs, no duplicate rows,
    distances within DIST_ROUNDINGS * 2^-53 * L (or `dist_tol(L)`). Returns the largest distance error in units of 2^-53 L."""
    worst = 0.0
    seen_pt, seen_ee = [], []
    for l, name in enumerate(LISTS):
        rows, d = got[name]
        assert rows.shape == (len(d), COLS[l]), name                      # counts equal the list lengths
        assert len(np.unique(rows, axis=0)) == len(rows), "duplicate rows in " + name
        und = ref.und_pt if name.startswith("pt_") else ref.und_ee
        (seen_pt if name.startswith("pt_") else seen_ee).extend(row_keys(rows, name))
        g_rows, g_d = sorted_rows(*without(rows, row_keys(rows, name), und, d))
        r_rows, r_d = ref.rows[name], ref.dist[name]
        assert g_rows.shape == r_rows.shape, (name, g_rows.shape, r_rows.shape, _diff(g_rows, r_rows))
        assert (g_rows == r_rows).all(), (name, _diff(g_rows, r_rows))
        if len(r_rows):
            L = ref.span[name]
            err = np.abs(g_d - r_d)
            tol = DIST_ROUNDINGS * 2.0 ** -53 * L if dist_tol is None else dist_tol(L)
            worst = max(worst, float((err / (2.0 ** -53 * L)).max()))
            assert (err <= tol).all(), (name, float((err / (2.0 ** -53 * L)).max()))
    # a pair is in one list only (no pair classified twice)
    assert len(set(seen_pt)) == len(seen_pt) and len(set(seen_ee)) == len(seen_ee), "a pair appears in two lists"
    return worst


def _diff(a, b):
    sa, sb = {tuple(r) for r in a.tolist()}, {tuple(r) for r in b.tolist()}
    return {"only_device": sorted(sa - sb)[:5], "only_reference": sorted(sb - sa)[:5]}


def check_intersections(got, ref_rows, und):
    got = np.asarray(got, dtype=np.int64).reshape(-1, 9)
    assert len(np.unique(got, axis=0)) == len(got), "duplicate intersection rows"
    g, _ = sorted_rows(without(got, et_key(got), und)[0])
    assert g.shape == ref_rows.shape and (g == ref_rows).all(), _diff(g, ref_rows)


def check_broad_phase(got, ref):
    for g, r in zip(got, ref):
        g = np.asarray(g, dtype=np.int64)
        assert len(np.unique(g, axis=0)) == len(g)
        assert g.shape == r.shape, (g.shape, r.shape)
        if len(r):
            assert (g[np.lexsort(g.T[::-1])] == r).all()
