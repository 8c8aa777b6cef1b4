"""Numpy restatement of the contact report (include/mistark_contact.h "contact report"), written from the geometry of oracle/contact.py.

A "key" is what the device detector installs per barrier-table row: (table 0..20, source 0 point-triangle / 1 edge-edge, closest-feature type,
primitive a, primitive b) with GLOBAL collision primitive indices (points, triangles and edges numbered mesh after mesh). `keys_from_detection`
derives the sorted key list from oracle.contact.detect, `rows` restates the row records for a key list at any vertex positions, `vertex_report` and
`pair_report` the two sums (terms in row order, plain sequential sums; the tests bound them against math.fsum)."""
import functools
import math
import os

import numpy as np

from oracle import contact as oc
from oracle import evaluator as ev

U = 2.0 ** -53
TABLE_NAMES = [
    "contact_d_d_pt_pp_cubic", "contact_d_d_pt_pe_cubic", "contact_d_d_pt_pt_cubic", "contact_d_d_ee_pp_cubic", "contact_d_d_ee_pe_cubic", "contact_d_d_ee_ee_cubic",
    "contact_rb_rb_pt_pp_cubic", "contact_rb_rb_pt_pe_cubic", "contact_rb_rb_pt_pt_cubic", "contact_rb_rb_ee_pp_cubic", "contact_rb_rb_ee_pe_cubic", "contact_rb_rb_ee_ee_cubic",
    "contact_rb_d_pt_pp_cubic", "contact_rb_d_pt_pe_cubic", "contact_rb_d_pt_pt_cubic", "contact_rb_d_pt_ep_cubic", "contact_rb_d_pt_tp_cubic",
    "contact_rb_d_ee_pp_cubic", "contact_rb_d_ee_pe_cubic", "contact_rb_d_ee_ee_cubic", "contact_rb_d_ee_ep_cubic"]
MOLLIFIED, OPEN, DEGENERATE = 1, 2, 4


class Layout:
    """Global numbering of the collision primitives of a scene."""

    def __init__(self, scene):
        M = scene.meshes
        self.v_off = np.cumsum([0] + [len(m.verts) for m in M])
        self.t_off = np.cumsum([0] + [len(m.tris) for m in M])
        self.e_off = np.cumsum([0] + [len(m.edges) for m in M])
        self.n_v, self.n_t, self.n_e = int(self.v_off[-1]), int(self.t_off[-1]), int(self.e_off[-1])
        self.cv_mesh = np.concatenate([np.full(len(m.verts), k) for k, m in enumerate(M)]).astype(np.int64)
        self.cv_src = np.concatenate([m.verts for m in M]).astype(np.int64)
        self.tri = np.concatenate([m.tris.reshape(-1, 3) + self.v_off[k] for k, m in enumerate(M)]).astype(np.int64).reshape(-1, 3)
        self.tri_mesh = np.concatenate([np.full(len(m.tris), k) for k, m in enumerate(M)]).astype(np.int64)
        self.edge = np.concatenate([m.edges.reshape(-1, 2) + self.v_off[k] for k, m in enumerate(M)]).astype(np.int64).reshape(-1, 2)
        self.edge_mesh = np.concatenate([np.full(len(m.edges), k) for k, m in enumerate(M)]).astype(np.int64)
        self.kind = [m.kind for m in M]
        self.thick = np.array([m.thickness for m in M])


def _family(src, ty):
    if src == 0:
        return 0 if ty <= oc.P_T2 else (1 if ty <= oc.P_E2 else 2)
    return 3 if ty <= oc.EA1_EB1 else (4 if ty <= oc.EA1_EB else 5)


def _table_of(fam, ka, kb):
    """Table of a classified pair; ka / kb: kind of the reference's A / B side (EnergyFrictionalContact.cpp:368-530, as oracle.contact.contact_tables)."""
    if ka == "d" and kb == "d":
        return fam
    if ka == "rb" and kb == "rb":
        return 6 + fam
    if ka == "rb":
        return 12 + fam if fam < 3 else 14 + fam
    return {0: 12, 1: 15, 2: 16, 3: 17, 4: 20, 5: 19}[fam]


def keys_from_detection(scene, prox):
    """Sorted list of (table, src, type, a, b) and, aligned with it, the detector's distance; pairs beyond dhat never reach a table."""
    L = Layout(scene)
    out = []
    if "pt" in prox:
        r = prox["pt"]
        for n in range(len(r["ty"])):
            ga, gb, ty = int(r["pm"][n]), int(r["tm"][n]), int(r["ty"][n])
            if r["d"][n] > L.thick[ga] + L.thick[gb]:
                continue
            out.append(((_table_of(_family(0, ty), L.kind[ga], L.kind[gb]), 0, ty, int(L.v_off[ga] + r["pi"][n]), int(L.t_off[gb] + r["ti"][n])), float(r["d"][n])))
    if "ee" in prox:
        r = prox["ee"]
        for n in range(len(r["ty"])):
            ga, gb, ty = int(r["am"][n]), int(r["bm"][n]), int(r["ty"][n])
            if r["d"][n] > L.thick[ga] + L.thick[gb]:
                continue
            # the reference's A is the point's side: for EA_EB0 / EA_EB1 that is edge b (oracle.contact._classified_pairs)
            ka, kb = (L.kind[gb], L.kind[ga]) if ty in (oc.EA_EB0, oc.EA_EB1) else (L.kind[ga], L.kind[gb])
            out.append(((_table_of(_family(1, ty), ka, kb), 1, ty, int(L.e_off[ga] + r["ai"][n]), int(L.e_off[gb] + r["bi"][n])), float(r["d"][n])))
    out.sort(key=lambda kv: kv[0])
    return [k for k, _ in out], np.array([d for _, d in out])


def table_row(scene, key):
    """The connectivity row mistark_contact_get_table holds for a key (physical vertex indices), as k_route writes it."""
    L = Layout(scene)
    table, src, ty, a, b = key
    fam = _family(src, ty)
    src_of = lambda cvs: [int(L.cv_src[v]) for v in cvs]
    if src == 0:
        A = dict(mesh=int(L.cv_mesh[a]), cols=src_of([a]))
        t = L.tri[b]
        feat = [t[ty]] if fam == 0 else ([t[ty - oc.P_E0], t[(ty - oc.P_E0 + 1) % 3]] if fam == 1 else list(t))
        B = dict(mesh=int(L.tri_mesh[b]), cols=src_of(feat))
    else:
        ea, eb = list(L.edge[a]), list(L.edge[b])
        ma, mb = int(L.edge_mesh[a]), int(L.edge_mesh[b])
        ES = lambda m, e: dict(mesh=m, cols=src_of(e))
        PS = lambda m, e, v: dict(mesh=m, cols=src_of(e + [v]))
        A, B = {
            oc.EA0_EB0: (PS(ma, ea, ea[0]), PS(mb, eb, eb[0])), oc.EA0_EB1: (PS(ma, ea, ea[0]), PS(mb, eb, eb[1])),
            oc.EA1_EB0: (PS(ma, ea, ea[1]), PS(mb, eb, eb[0])), oc.EA1_EB1: (PS(ma, ea, ea[1]), PS(mb, eb, eb[1])),
            oc.EA_EB0: (PS(mb, eb, eb[0]), ES(ma, ea)), oc.EA_EB1: (PS(mb, eb, eb[1]), ES(ma, ea)),
            oc.EA0_EB: (PS(ma, ea, ea[0]), ES(mb, eb)), oc.EA1_EB: (PS(ma, ea, ea[1]), ES(mb, eb)),
            oc.EA_EB: (ES(ma, ea), ES(mb, eb))}[ty]
    M = scene.meshes
    ka, kb = M[A["mesh"]].kind, M[B["mesh"]].kind
    if ka == "d" and kb == "rb":
        return [B["mesh"], A["mesh"], M[B["mesh"]].idx_in_ps] + B["cols"] + A["cols"]
    head = [A["mesh"], B["mesh"]] + ([M[A["mesh"]].idx_in_ps] if ka == "rb" else []) + ([M[B["mesh"]].idx_in_ps] if ka == "rb" and kb == "rb" else [])
    return head + A["cols"] + B["cols"]


def _dot(a, b):
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]


def _cross(a, b):
    return np.array([a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]])


def _point_line_sq(p, e0, e1):
    c = _cross(e0 - p, e1 - p)
    return _dot(c, c) / _dot(e1 - e0, e1 - e0)


def _line_param(p, e0, e1):
    e = e1 - e0
    return _dot(p - e0, e) / _dot(e, e)


def weights(src, ty, p0, p1):
    """(a side [2], b side [3]); exact zeros and ones where the feature does not use a node."""
    if src == 0:
        wb = {oc.P_T0: [1.0, 0.0, 0.0], oc.P_T1: [0.0, 1.0, 0.0], oc.P_T2: [0.0, 0.0, 1.0], oc.P_E0: [1.0 - p0, p0, 0.0], oc.P_E1: [0.0, p0, p1],
              oc.P_E2: [1.0 - p1, 0.0, p1], oc.P_T: [1.0 - p0 - p1, p0, p1]}[ty]
        return [1.0, 0.0], wb
    return [1.0 - p0, p0], [1.0 - p1, p1, 0.0]


def rest_positions(scene, st):
    """Rest position of every collision vertex: X of a deformable mesh, the local vertices of a rigid one."""
    return np.concatenate([(st["X"] if m.kind == "d" else st["rb_xloc"])[m.verts] for m in scene.meshes])


def rows(scene, keys, X, Xrest, k):
    """(ints [n, 8], doubles [n, 16]) of the key list at collision vertex positions X [n_v, 3]."""
    L = Layout(scene)
    ri = np.zeros((len(keys), 8), dtype=np.int32)
    rd = np.zeros((len(keys), 16))
    with np.errstate(divide="ignore", invalid="ignore"):
        for n, (table, src, ty, a, b) in enumerate(keys):
            p0 = p1 = 0.0
            m = 1.0
            if src == 0:
                ga, gb = int(L.cv_mesh[a]), int(L.tri_mesh[b])
                p = X[a]
                t = [X[v] for v in L.tri[b]]
                cA = p
                if ty <= oc.P_T2:
                    cB = t[ty]
                    d2 = _dot(cB - p, cB - p)
                    p0, p1 = (1.0 if ty == oc.P_T1 else 0.0), (1.0 if ty == oc.P_T2 else 0.0)
                elif ty <= oc.P_E2:
                    j = ty - oc.P_E0
                    e0, e1 = t[j], t[(j + 1) % 3]
                    al = _line_param(p, e0, e1)
                    cB = e0 + al * (e1 - e0)
                    d2 = _point_line_sq(p, e0, e1)
                    p0, p1 = [(al, 0.0), (1.0 - al, al), (0.0, 1.0 - al)][j]
                else:
                    nrm = _cross(t[1] - t[0], t[2] - t[0])
                    h, n2 = _dot(p - t[0], nrm), _dot(nrm, nrm)
                    d2 = h * h / n2
                    cB = p - (h / n2) * nrm
                    bc = oc.barycentric_point_triangle(p, t[0], t[1], t[2])
                    p0, p1 = float(bc[1]), float(bc[2])
            else:
                ga, gb = int(L.edge_mesh[a]), int(L.edge_mesh[b])
                ea, eb = [X[v] for v in L.edge[a]], [X[v] for v in L.edge[b]]
                ra, rb = [Xrest[v] for v in L.edge[a]], [Xrest[v] for v in L.edge[b]]
                eps_x = 1e-3 * _dot(ra[0] - ra[1], ra[0] - ra[1]) * _dot(rb[0] - rb[1], rb[0] - rb[1])
                c = _cross(ea[1] - ea[0], eb[1] - eb[0])
                x = _dot(c, c)
                r = x / eps_x
                m = 1.0 if x > eps_x else (-1.0 * r + 2.0) * r
                if ty <= oc.EA1_EB1:
                    ia, ib = ty >> 1, ty & 1
                    cA, cB, p0, p1 = ea[ia], eb[ib], float(ia), float(ib)
                    d2 = _dot(cB - cA, cB - cA)
                elif ty in (oc.EA_EB0, oc.EA_EB1):
                    q = eb[ty - oc.EA_EB0]
                    p0, p1 = _line_param(q, ea[0], ea[1]), float(ty - oc.EA_EB0)
                    cA, cB = ea[0] + p0 * (ea[1] - ea[0]), q
                    d2 = _point_line_sq(q, ea[0], ea[1])
                elif ty in (oc.EA0_EB, oc.EA1_EB):
                    q = ea[ty - oc.EA0_EB]
                    p0, p1 = float(ty - oc.EA0_EB), _line_param(q, eb[0], eb[1])
                    cA, cB = q, eb[0] + p1 * (eb[1] - eb[0])
                    d2 = _point_line_sq(q, eb[0], eb[1])
                else:
                    u, v, w = ea[1] - ea[0], eb[1] - eb[0], ea[0] - eb[0]
                    A, B, C, D, E = _dot(u, u), _dot(u, v), _dot(v, v), _dot(u, w), _dot(v, w)
                    den = A * C - B * B
                    p0, p1 = (B * E - C * D) / den, (A * E - B * D) / den
                    cA, cB = ea[0] + p0 * u, eb[0] + p1 * v
                    h = _dot(eb[0] - ea[0], c)
                    d2 = h * h / _dot(c, c)
            d = math.sqrt(d2) if d2 >= 0.0 else float("nan")
            dhat = L.thick[ga] + L.thick[gb]
            deg = not (d > 0.0) or not math.isfinite(d)
            flags = (MOLLIFIED if (src == 1 and m < 1.0) else 0) | (OPEN if d >= dhat else 0) | (DEGENERATE if deg else 0)
            g = dhat - d
            ri[n] = [table, src, ty, ga, gb, a, b, flags]
            rd[n, 0], rd[n, 1] = d, dhat
            rd[n, 2:5], rd[n, 5:8] = cA, cB
            rd[n, 8:11] = 0.0 if deg else (cA - cB) / d
            rd[n, 11] = m
            rd[n, 12] = m * (k * (g * g))
            rd[n, 13] = m * (k * (g * g * g) / 3.0)
            rd[n, 14], rd[n, 15] = p0, p1
    return ri, rd


def contributions(scene, ri, rd):
    """Per row its four (collision vertex, weight): point + triangle vertices, or the two edges' vertices."""
    L = Layout(scene)
    out = []
    for n in range(len(ri)):
        src, ty, a, b = int(ri[n, 1]), int(ri[n, 2]), int(ri[n, 5]), int(ri[n, 6])
        wa, wb = weights(src, ty, rd[n, 14], rd[n, 15])
        if src == 0:
            out.append(list(zip([a] + list(L.tri[b]), [wa[0]] + wb)))
        else:
            out.append(list(zip(list(L.edge[a]) + list(L.edge[b]), wa + wb[:2])))
    return out


def triangle_areas(scene, X):
    L = Layout(scene)
    if L.n_t == 0:
        return np.zeros(0)
    return 0.5 * np.linalg.norm(np.cross(X[L.tri[:, 1]] - X[L.tri[:, 0]], X[L.tri[:, 2]] - X[L.tri[:, 0]]), axis=1)


def vertex_report(scene, ri, rd, X):
    """(records [n_v, 5], per vertex the list of its w fn terms in row order)."""
    L = Layout(scene)
    out = np.zeros((L.n_v, 5))
    out[:, 0] = np.inf
    terms = [[] for _ in range(L.n_v)]
    for n, cs in enumerate(contributions(scene, ri, rd)):
        for v, w in cs:
            out[v, 0] = min(out[v, 0], rd[n, 0]) if not math.isnan(rd[n, 0]) else out[v, 0]
            out[v, 1] += 1
            terms[v].append(w * rd[n, 12])
    ta = triangle_areas(scene, X)
    area = np.zeros(L.n_v)
    for t in range(L.n_t):
        for v in L.tri[t]:
            area[v] += ta[t]
    for v in range(L.n_v):
        s = 0.0
        for x in terms[v]:
            s += x
        out[v, 2] = s
    out[:, 3] = area / 3.0
    out[:, 4] = [out[v, 2] / out[v, 3] if out[v, 3] > 0.0 else 0.0 for v in range(L.n_v)]
    return out, terms


def pair_report(scene, ri, rd):
    """(records [G, G, 8], terms[(ga, gb)] = per summed field (3 fn, 4..6 fn n, 7 E) the list of terms in row order)."""
    L = Layout(scene)
    G = len(scene.meshes)
    out = np.zeros((G, G, 8))
    terms = {}
    for ga in range(G):
        for gb in range(ga, G):
            out[ga, gb, 1] = np.inf
            out[ga, gb, 2] = L.thick[ga] + L.thick[gb]
            terms[(ga, gb)] = {f: [] for f in (3, 4, 5, 6, 7)}
    for n in range(len(ri)):
        ga, gb = int(ri[n, 3]), int(ri[n, 4])
        lo, hi = min(ga, gb), max(ga, gb)
        sign = 1.0 if ga <= gb else -1.0
        out[lo, hi, 0] += 1
        if not math.isnan(rd[n, 0]):
            out[lo, hi, 1] = min(out[lo, hi, 1], rd[n, 0])
        T = terms[(lo, hi)]
        T[3].append(rd[n, 12])
        for c in range(3):
            T[4 + c].append(sign * (rd[n, 12] * rd[n, 8 + c]))
        T[7].append(rd[n, 13])
    for (ga, gb), T in terms.items():
        for f, xs in T.items():
            s = 0.0
            for x in xs:
                s += x
            out[ga, gb, f] = s
    return out, terms


def sum_bound(xs):
    """(n + 8) 2^-53 sum |terms|: any summation order of n terms against math.fsum of the same terms (the budget tests' bound)."""
    return (len(xs) + 8) * U * math.fsum(abs(x) for x in xs)


def bounds_of(ri):
    """bounds[t], t = 0..21, of the table column of the row ints."""
    return np.searchsorted(ri[:, 0] if len(ri) else np.zeros(0), np.arange(22), side="left")


GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@functools.lru_cache(maxsize=None)
def fixture_case(name):
    """A contact fixture evaluated once per process and shared (read-only): its scene, state, the installed key list with the detector's distances, and
    the restated rows at the detection state."""
    from contact_util import state_from_fixture

    prob, man, z = ev.load_fixture(os.path.join(GOLDEN, name + ".npz"))
    st, _ = state_from_fixture(prob, man)
    scene = oc.scene_from_fixture(man, z)
    dt = float(np.asarray(st["dt"]).ravel()[0])
    k = float(np.asarray(st["k"]).ravel()[0])
    X = np.concatenate(oc.mesh_vertices(scene, st, dt))
    prox = oc.detect(scene, oc.mesh_vertices(scene, st, dt), 2.0 * oc.max_thickness(scene))
    keys, d_detect = keys_from_detection(scene, prox)
    Xrest = rest_positions(scene, st)
    ri, rd = rows(scene, keys, X, Xrest, k)
    for a in (X, Xrest, ri, rd, d_detect):
        a.setflags(write=False)
    return dict(prob=prob, man=man, st=st, scene=scene, dt=dt, k=k, X=X, Xrest=Xrest, keys=keys, d_detect=d_detect, ri=ri, rd=rd)


def field_scales(rd, xmax, k):
    """The magnitude every double field of a row is measured against (xmax: per row or overall, the largest |coordinate| involved)."""
    s = np.ones_like(rd)
    s[:, 0] = s[:, 1] = rd[:, 1]
    s[:, 2:8] = np.reshape(xmax, (-1, 1))
    s[:, 12] = k * rd[:, 1] ** 2
    s[:, 13] = k * rd[:, 1] ** 3 / 3.0
    s[:, 14:16] = np.maximum(1.0, np.abs(rd[:, 14:16]))
    return s
