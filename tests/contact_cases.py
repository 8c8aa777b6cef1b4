"""Synthesised branch states of the 21 barrier and 14 friction potentials (oracle.energies._CONTACT) and their exact derivatives — shared by
tests/test_contact_cases_cpu.py (the states, the two references and the tolerance table are proved there) and tests/test_gpu_contact_synth.py
(k_eval_contact_closed, k_eval_pgh, k_eval_pgh_multi, k_eval_p and the device interpreter against the same numbers).

 * The BINDING LAYOUT of a potential (array order, strides, connectivity columns, DoF sets) and its SymX op arrays are read from the manifest of a
   golden that holds rows of it (contactmix_t0, contactcorners_t0, contactrods_t0); `schema(name)` only names what each binding is, and is
   checked stride by stride against the golden. Arrays and connectivity are synthesised.
 * A STATE is one row, built by construction and finished by solving for the one free scalar (secant on the value measured in mpmath from the
   rounded float64 inputs): the offset along the normal sets d, the rotation of one edge about the common normal sets x = |ea x eb|^2, the scale
   of the tangential velocity sets u. No random search.
 * `exact(name, state)`: the potential restated on second-order Taylor numbers (value, sparse gradient, sparse Hessian) over mpmath at 40 digits,
   `where` branches included; `oracle_rows(table)`: the float64 oracle (oracle.evaluator.evaluate_potential); `oracle_alt(table)`: the float64
   oracle with the plane distance in the closed form's operation order ((u . n)^2 / |n|^2 instead of (u . n / |n|)^2).
 * `measure_tolerances()` / `write_tolerances()` regenerate tests/contact_tolerances.json: per (layout, state label, kind, rigid side present) the largest
   error of the float64 oracle (the larger of the two orders) against `exact`, per quantity, relative to the element's largest exact entry of that
   quantity. `bounds()` is 8 x that, floor 8 * 2^-52, times the element's scale: the margin and floor of custom_cases.bounds.

What the golden layouts fix: dt, the barrier stiffness and epsv are bound globally (connectivity column -1), so they are one value per table;
mu, fn, T, the barycentric weights and the two thicknesses (dhat is their sum) differ from row to row. A rigid edge's rest positions are its x_loc,
so its eps_x follows from x_loc; a deformable edge has rest lengths that differ from the current ones. The point of an `ee` potential that carries
one is the edge's own end vertex (the same index in two connectivity columns), as in the goldens.

Layouts (257 rows; the labelled states first, then the same states again cyclically, input for input):
 * `isolated`: every row has vertices, bodies, objects of its own.
 * `shared`: every rigid side is ONE body for the whole table and the first deformable vertex is ONE vertex for all rows. What is common has one
   state: the bodies carry the `spin` kinematics (|w1| dt = 1.2 rad) in every row, and every row's geometry is laid around the common vertex —
   there `far` is carried by x_loc (rigid sides) or is not translated (no rigid side), and friction's `rest` has the common velocities cancel in
   the tangent plane to rounding instead of being zero. Each labelled state is solved again for this layout: the targets d, x and u hold alike.
 * the tables of 1 and of 7 rows are the first rows of `isolated`.
"""
from __future__ import annotations

import json
import math
import os
import zlib

import mpmath
import numpy as np

from oracle import ad
from oracle import energies as en
from oracle import evaluator as ev

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDENS = ["contactmix_t0", "contactcorners_t0", "contactrods_t0"]
TOLERANCES = os.path.join(HERE, "contact_tolerances.json")
FLOOR = 8.0 * 2.0 ** -52
NE = 257                       # crosses the 256-lane block of the one-lane-per-contact kernel
SMALL = (1, 7)
NAMES = sorted(en._CONTACT)
DT, KSTIFF, EPSV = 0.01, 3.0e5, 1.0e-3
FAR = (1.0e3, -2.0e3, 5.0e2)
SPIN, CALM = 1.2, 0.05         # |w1| dt of a rigid side
U_OFF = (1.13e-9, -1.07e-9)    # the reference's built-in offsets of the tangential displacement

MP = mpmath.mp.clone()
MP.dps = 40
mpf = MP.mpf

BARRIER_STATES = ["mid", "near", "inside", "beyond", "far", "aniso", "spin"]
MOLL_STATES = ["moll_half", "moll_in", "moll_out", "moll_par"]
FRICTION_STATES = ["stick", "slide", "edge_in", "edge_out", "rest", "fast", "corner", "spin"]
D_TARGET = {"near": 1e-3, "inside": 1.0 - 1e-6, "beyond": 1.5}                        # d / dhat (0.6 otherwise)
X_TARGET = {"moll_half": 0.5, "moll_in": 1.0 - 1e-6, "moll_out": 1.0 + 1e-6, "moll_par": 1e-6}   # x / eps_x
U_TARGET = {"stick": 0.3, "slide": 5.0, "edge_in": 1.0 - 1e-6, "edge_out": 1.0 + 1e-6, "fast": 1e4, "corner": 0.6, "spin": 2.0}   # u / epsu


# ======================================================================================================================================
# what each binding is
# ======================================================================================================================================
def parse(name):
    t = name.split("_")
    if t[0] == "contact":
        return {"fam": t[3], "A": t[1], "B": t[2], "kind": t[4]}
    return {"fam": "friction", "A": t[1], "B": t[2], "kind": t[3]}


PT_K = {"pp": (1, 1), "pe": (1, 2), "pt": (1, 3), "ep": (2, 1), "tp": (3, 1)}
FR_K = {"pp": (1, 1), "pe": (1, 2), "pt": (1, 3), "ee": (2, 2), "ep": (2, 1), "tp": (3, 1)}
EE_P = {"pp": (True, True), "pe": (True, False), "ee": (False, False), "ep": (False, True)}
NBARY = {"pp": 0, "pe": 2, "pt": 3, "ee": 2, "ep": 2, "tp": 3}
ROLE_STRIDE = {"v1": 3, "x0": 3, "X": 3, "bv1": 3, "bw1": 3, "t0": 3, "q0": 4, "xloc": 3, "thick": 1, "bary2": 2, "bary3": 3, "T": 6, "mu": 1, "fn": 1, "dt": 1, "k": 1, "epsv": 1}
ROLES = list(ROLE_STRIDE)
ROLE_DOF = {"v1": 0, "bv1": 1, "bw1": 2}
CLASS_OF = {"v1": "soft", "x0": "soft", "X": "soft", "bv1": "body", "bw1": "body", "t0": "body", "q0": "body", "xloc": "rv", "thick": "obj", "bary2": "row", "bary3": "row",
            "T": "row", "mu": "row", "fn": "row"}


def _group(side, rigid, ks, vel, alias=None):
    """The bindings of one getter call: vertices `ks` of a side. Slot = (role, key, entity): key names the value in the energy's terms,
    entity is what holds it (the point of an `ee` potential is the edge's own end vertex: alias)."""
    ent = lambda cls, k: (cls, side, alias if (alias is not None and k == 2) else k)
    if rigid:
        return [("dt", None, None)] + [("xloc", (side, k), ent("rv", k)) for k in ks] + [(r, (side, ks[0]), ("body", side)) for r in ("bv1", "bw1", "t0", "q0")]
    s = [("v1", (side, k), ent("soft", k)) for k in ks]
    if not vel:
        s += [("x0", (side, k), ent("soft", k)) for k in ks] + [("dt", None, None)]
    return s


def schema(name):
    p = parse(name)
    ra, rb = p["A"] == "rb", p["B"] == "rb"
    thick = [("thick", 0, ("obj", 0)), ("thick", 1, ("obj", 1))]
    if p["fam"] == "pt":
        ka, kb = PT_K[p["kind"]]
        return _group(0, ra, list(range(ka)), False) + _group(1, rb, list(range(kb)), False) + thick + [("k", None, None)]
    if p["fam"] == "ee":
        out = []
        for side, rigid, has_p, al in ((0, ra, EE_P[p["kind"]][0], 1), (1, rb, EE_P[p["kind"]][1], 0)):
            out += _group(side, rigid, [0, 1], False)
            out += [("xloc" if rigid else "X", (side, k, "rest"), ("rv" if rigid else "soft", side, k)) for k in (0, 1)]
            if has_p:
                out += _group(side, rigid, [2], False, alias=al)
        return out + [("k", None, None)] + thick
    ka, kb = FR_K[p["kind"]]
    out = _group(0, ra, list(range(ka)), True) + _group(1, rb, list(range(kb)), True)
    nb = NBARY[p["kind"]]
    if nb:
        out.append(("bary%d" % nb, None, ("row",)))
    return out + [(r, None, ("row",)) for r in ("T", "mu", "fn")] + [("epsv", None, None), ("dt", None, None)]


_LAYOUT = {}


def layout(name):
    """(golden file, bindings [(stride, conn column, dof set)], conn stride, op arrays) of the first golden that holds rows of the potential."""
    if not _LAYOUT:
        for g in GOLDENS:
            z = np.load(os.path.join(HERE, "golden", g + ".npz"))
            man = json.loads(bytes(z["manifest_json"]).decode())
            for pi, p in enumerate(man["potentials"]):
                if p["name"] in en._CONTACT and p["name"] not in _LAYOUT and p["n_elem"] > 0 and ("p%d_ops" % pi) in z:
                    ops = {k: np.array(z["p%d_%s" % (pi, k)]) for k in ("ops", "opsc", "cops", "copsc") if ("p%d_%s" % (pi, k)) in z}
                    _LAYOUT[p["name"]] = {"golden": g, "bindings": [(b["stride"], b["conn"], b["dof_set"], b["array"]) for b in p["bindings"]], "conn_stride": p["conn_stride"],
                                          "ops": ops, "n_inputs": p["n_inputs"]}
    return _LAYOUT[name]


_BOUND = {}


def bound_schema(name):
    """The schema laid on the golden's bindings: [(role, key, entity, stride, conn column, dof set)]; asserts that the two describe the same thing."""
    if name in _BOUND:
        return _BOUND[name]
    L, S = layout(name), schema(name)
    assert len(L["bindings"]) == len(S), (name, len(L["bindings"]), len(S))
    out, col_ent, arr_role = [], {}, {}
    for (stride, col, dof, arr), (role, key, ent) in zip(L["bindings"], S):
        assert stride == ROLE_STRIDE[role] and dof == ROLE_DOF.get(role, -1) and (col < 0) == (ent is None), (name, role, stride, col, dof)
        assert arr_role.setdefault(arr, role) == role, (name, arr, role)             # one golden array, one role
        if ent is not None:
            # a column indexes one entity; the aliased point column indexes the end vertex's entity
            assert col_ent.setdefault(col, ent) == ent, (name, col, ent)
        out.append((role, key, ent, stride, col, dof))
    assert sum(s for s, _, _, _ in L["bindings"]) == L["n_inputs"]
    _BOUND[name] = out
    return out


# ======================================================================================================================================
# second-order Taylor numbers over mpmath, sparse in the DoFs (in the manner of custom_cases.T2)
# ======================================================================================================================================
def _lin(ca, A, cb, B):
    r = {k: ca * v for k, v in A.items()}
    for k, v in B.items():
        r[k] = r[k] + cb * v if k in r else cb * v
    return r


class J:
    __slots__ = ("v", "g", "h")

    def __init__(self, v, g=None, h=None):
        self.v, self.g, self.h = v, g or {}, h or {}

    @staticmethod
    def var(v, i):
        return J(v, {i: mpf(1)})

    def __add__(a, b):
        if not isinstance(b, J):
            return J(a.v + b, a.g, a.h)
        return J(a.v + b.v, _lin(1, a.g, 1, b.g), _lin(1, a.h, 1, b.h))

    __radd__ = __add__

    def __neg__(a):
        return J(-a.v, {k: -v for k, v in a.g.items()}, {k: -v for k, v in a.h.items()})

    def __sub__(a, b):
        if not isinstance(b, J):
            return J(a.v - b, a.g, a.h)
        return J(a.v - b.v, _lin(1, a.g, -1, b.g), _lin(1, a.h, -1, b.h))

    def __rsub__(a, b):
        return (-a) + b

    def __mul__(a, b):
        if not isinstance(b, J):
            return J(a.v * b, {k: v * b for k, v in a.g.items()}, {k: v * b for k, v in a.h.items()})
        h = _lin(b.v, a.h, a.v, b.h)
        for i, ai in a.g.items():
            for j, bj in b.g.items():
                p = ai * bj
                if i == j:
                    p, k = p + p, (i, i)
                else:
                    k = (i, j) if i < j else (j, i)
                h[k] = h[k] + p if k in h else p
        return J(a.v * b.v, _lin(b.v, a.g, a.v, b.g), h)

    __rmul__ = __mul__

    def chain(x, f, df, ddf):
        h = {k: df * v for k, v in x.h.items()}
        for i, gi in x.g.items():
            for j, gj in x.g.items():
                if i <= j:
                    p = ddf * gi * gj
                    h[(i, j)] = h[(i, j)] + p if (i, j) in h else p
        return J(f, {k: df * v for k, v in x.g.items()}, h)

    def recip(x):
        r = 1 / x.v
        return x.chain(r, -r * r, 2 * r * r * r)

    def __truediv__(a, b):
        return a * (b.recip() if isinstance(b, J) else 1 / b)

    def __rtruediv__(a, b):
        return a.recip() * b

    def sqrt(x):
        s = MP.sqrt(x.v)
        return x.chain(s, 1 / (2 * s), -1 / (4 * s * x.v))


def _sqrt(x):
    if isinstance(x, J):
        return x.sqrt()
    return math.sqrt(x) if isinstance(x, float) else MP.sqrt(x)


def _val(x):
    return x.v if isinstance(x, J) else x


# ======================================================================================================================================
# the potentials restated (stark/src/models/interactions/EnergyFrictionalContact.cpp, distances.cpp, rigidbody_transformations.cpp), on any
# scalar type: J (exact), mpf (measuring), float
# ======================================================================================================================================
def _sub(a, b): return [a[0] - b[0], a[1] - b[1], a[2] - b[2]]
def _add(a, b): return [a[0] + b[0], a[1] + b[1], a[2] + b[2]]
def _scl(s, a): return [a[0] * s, a[1] * s, a[2] * s]
def _dot(a, b): return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]
def _cross(a, b): return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]


def rotation_after_step(q0, w, dt):
    """R(normalize(q0 + dt/2 (0, w) q0)), q = (w, x, y, z)"""
    a, b, c, d = q0
    p = [-(w[0] * b + w[1] * c + w[2] * d), w[0] * a + w[1] * d - w[2] * c, w[1] * a + w[2] * b - w[0] * d, w[2] * a + w[0] * c - w[1] * b]
    q = [q0[i] + p[i] * (dt / 2) for i in range(4)]
    n = _sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3])
    qw, qx, qy, qz = [c_ / n for c_ in q]
    return [[1 - 2 * (qy * qy + qz * qz), 2 * (qx * qy - qw * qz), 2 * (qx * qz + qw * qy)],
            [2 * (qx * qy + qw * qz), 1 - 2 * (qx * qx + qz * qz), 2 * (qy * qz - qw * qx)],
            [2 * (qx * qz - qw * qy), 2 * (qy * qz + qw * qx), 1 - 2 * (qx * qx + qy * qy)]]


def _mv(R, x): return [_dot(R[0], x), _dot(R[1], x), _dot(R[2], x)]
def _mtv(R, x): return [R[0][i] * x[0] + R[1][i] * x[1] + R[2][i] * x[2] for i in range(3)]


def _line_sq(p, a, b):
    ab, ap = _sub(b, a), _sub(p, a)
    e = _dot(ap, ab)
    return _dot(ap, ap) - e * e / _dot(ab, ab)


def energy(name, x):
    """x: the potential's inputs in binding order (flat). Returns (E, diagnostics)."""
    P = parse(name)
    G, o, dt = {}, 0, None
    for role, key, _, stride, _, _ in bound_schema(name):
        val = x[o:o + stride]
        o += stride
        if role == "dt":
            dt = val[0]
        elif key is not None:
            G[(role, key)] = val
        else:
            G[role] = val
    rigid = {0: P["A"] == "rb", 1: P["B"] == "rb"}
    vel = P["fam"] == "friction"
    Rc = {}

    def point(side, k):
        if not rigid[side]:
            return G[("v1", (side, k))] if vel else _add(G[("x0", (side, k))], _scl(dt, G[("v1", (side, k))]))
        kb = 2 if ("bv1", (side, 2)) in G and k == 2 else 0
        v1, w1, t0, q0 = (G[(r, (side, kb))] for r in ("bv1", "bw1", "t0", "q0"))
        if (side, kb) not in Rc:      # (the point group of an `ee` potential binds the body again: DoF blocks of its own)
            Rc[(side, kb)] = rotation_after_step(q0, w1, dt)
        r = _mv(Rc[(side, kb)], G[("xloc", (side, k))])
        return _add(v1, _cross(w1, r)) if vel else _add(_add(t0, _scl(dt, v1)), r)

    if vel:
        ka, kb = FR_K[P["kind"]]
        a, b = [point(0, k) for k in range(ka)], [point(1, k) for k in range(kb)]
        bary = G.get("bary2", G.get("bary3"))
        comb = lambda pts: _add(_add(_scl(bary[0], pts[0]), _scl(bary[1], pts[1])), _scl(bary[2], pts[2])) if len(pts) == 3 else _add(_scl(bary[0], pts[0]), _scl(bary[1], pts[1]))
        kind = P["kind"]
        if kind == "pp":
            v = _sub(b[0], a[0])
        elif kind in ("pe", "pt"):
            v = _sub(comb(b), a[0])
        elif kind == "ee":
            v = _sub(_add(b[0], _scl(bary[1], _sub(b[1], b[0]))), _add(a[0], _scl(bary[0], _sub(a[1], a[0]))))
        else:
            v = _sub(comb(a), b[0])
        T, mu, fn, epsv = G["T"], G["mu"][0], G["fn"][0], G["epsv"][0]
        ut0 = _dot(T[0:3], v) * dt + U_OFF[0]
        ut1 = _dot(T[3:6], v) * dt + U_OFF[1]
        u = _sqrt(ut0 * ut0 + ut1 * ut1)
        epsu = dt * epsv
        k = mu * fn / epsu
        eps = mu * fn / (2 * k)
        stick = _val(u) < epsu
        E = k * u * u / 2 if stick else mu * fn * (u - eps)
        return E, {"u": _val(u), "epsu": epsu, "stick": stick}

    dhat = G[("thick", 0)][0] + G[("thick", 1)][0]
    k = G["k"][0]
    diag = {}
    if P["fam"] == "pt":
        ka, kb = PT_K[P["kind"]]
        a, b = [point(0, i) for i in range(ka)], [point(1, i) for i in range(kb)]
        if P["kind"] in ("ep", "tp"):      # the point is side b's, the edge / triangle side a's
            a, b = b, a
        pt = a[0]
        if len(b) == 1:
            d = _sqrt(_dot(_sub(pt, b[0]), _sub(pt, b[0])))
        elif len(b) == 2:
            d = _sqrt(_line_sq(pt, b[0], b[1]))
        else:
            n = _cross(_sub(b[0], b[2]), _sub(b[1], b[2]))
            nn = _sqrt(_dot(n, n))
            n = [c / nn for c in n]
            l = _dot(_sub(pt, b[0]), n)
            d = _sqrt(l * l)
        moll = 1
        diag.update(point=pt, prim=b)
    else:
        ea, eb = [point(0, 0), point(0, 1)], [point(1, 0), point(1, 1)]
        ra, rb_ = [G[("xloc" if rigid[0] else "X", (0, i, "rest"))] for i in (0, 1)], [G[("xloc" if rigid[1] else "X", (1, i, "rest"))] for i in (0, 1)]
        has_p, has_q = EE_P[P["kind"]]
        p_ = point(0, 2) if has_p else None
        q_ = point(1, 2) if has_q else None
        if P["kind"] == "pp":
            d = _sqrt(_dot(_sub(p_, q_), _sub(p_, q_)))
        elif P["kind"] == "pe":
            d = _sqrt(_line_sq(p_, eb[0], eb[1]))
        elif P["kind"] == "ep":
            d = _sqrt(_line_sq(q_, ea[0], ea[1]))
        else:
            n = _cross(_sub(ea[1], ea[0]), _sub(eb[1], eb[0]))
            l = _dot(_sub(eb[0], ea[0]), n)
            d = _sqrt(l * l / _dot(n, n))
        la, lb = _sub(ra[0], ra[1]), _sub(rb_[0], rb_[1])
        eps_x = _dot(la, la) * _dot(lb, lb) * 1e-3       # (the reference's double 1e-3, exactly)
        c = _cross(_sub(ea[1], ea[0]), _sub(eb[1], eb[0]))
        xx = _dot(c, c)
        r = xx / eps_x
        mollified = not (_val(xx) > eps_x)
        moll = (2 - r) * r if mollified else 1
        diag.update(x=_val(xx), eps_x=eps_x, mollified=mollified, edges=(ea, eb))
    gap = dhat - d
    E = moll * (gap * gap * gap * k / 3)
    diag.update(d=_val(d), dhat=dhat)
    return E, diag


# ======================================================================================================================================
# states
# ======================================================================================================================================
def _rng(*key):
    return np.random.default_rng(zlib.crc32("|".join(str(k) for k in key).encode()))


def _rotation(rng):
    q = rng.normal(size=4)
    q /= np.linalg.norm(q)
    return np.array(rotation_after_step([float(c) for c in q], [0.0, 0.0, 0.0], 0.0))


def _kin(rng, spin, center=(0.0, 0.0, 0.0), still=False):
    """one body's kinematics: a non-identity q0, |w1| dt about a skew axis"""
    skew = lambda n: rng.choice([-1.0, 1.0], n) * rng.uniform(0.3, 1.0, n)      # no component near zero: neither the identity nor a coordinate axis
    q0 = skew(4)
    q0 /= np.linalg.norm(q0)
    ax = skew(3)
    ax /= np.linalg.norm(ax)
    if still:
        return {"bv1": np.zeros(3), "bw1": np.zeros(3), "t0": np.asarray(center) + rng.normal(size=3) * 0.05, "q0": q0}
    return {"bv1": rng.normal(size=3) * 0.3, "bw1": ax * ((SPIN if spin else CALM) / DT), "t0": np.asarray(center) + rng.normal(size=3) * 0.05, "q0": q0}


def _m(v):
    return [mpf(float(c)) for c in v]


def _f(v):
    return np.array([float(c) for c in v])


def make_pins(name):
    """What the `shared` layout has in common: the bodies of the rigid sides (spin kinematics) and the first deformable vertex."""
    rng = _rng(name, "pins")
    P = parse(name)
    pins = {}
    for side, s in ((0, P["A"]), (1, P["B"])):
        if s == "rb":
            pins[("body", side)] = _kin(rng, True)
    soft = [e for _, _, e, _, _, _ in bound_schema(name) if e is not None and e[0] == "soft"]
    if soft:
        pins["anchor"] = soft[0]
        pins[soft[0]] = {"v1": rng.normal(size=3) * 0.3, "x0": rng.normal(size=3) * 0.2, "X": rng.normal(size=3) * 0.2}
    return pins


def flat(name, state):
    """the row's inputs in binding order, as floats"""
    out = []
    for role, key, ent, stride, _, _ in bound_schema(name):
        v = state["globals"][role] if ent is None else state[ent][role]
        v = np.atleast_1d(np.asarray(v, dtype=np.float64))
        assert v.shape == (stride,), (name, role, v.shape)
        out += [float(c) for c in v]
    return out


def measure(name, state, arith="mp"):
    x = flat(name, state)
    return energy(name, [mpf(c) for c in x] if arith == "mp" else x)[1]


def _solve(build, read, s0, target):
    """secant on the free scalar: build(s) -> state, read(state) -> the measured ratio (mpmath, from the rounded inputs)"""
    s_prev, s = mpf(s0), mpf(s0) * (1 + mpf("1e-4"))
    f_prev = read(build(s_prev)) / target - 1
    best = (abs(f_prev), s_prev)
    for _ in range(8):
        st = build(s)
        f = read(st) / target - 1
        if abs(f) < best[0]:
            best = (abs(f), s)
        if abs(f) < mpf("1e-13") or f == f_prev:
            break
        s_prev, s, f_prev = s, s - f * (s - s_prev) / (f - f_prev), f
    return build(best[1]), best[1]


def _ratio(name, state, a, b):
    m = measure(name, state)
    return m[a] / m[b]


def _place(name, label, pins, rng, pts, rest_len):
    """world points {(side, k): mp vector} -> a state: rounded inputs of every entity. The common vertex stays where it is pinned (the geometry is
    moved to it), a rigid side's x_loc is R1^T (p - t1)."""
    P = parse(name)
    S = bound_schema(name)
    ents = []
    for _, _, e, _, _, _ in S:
        if e is not None and e not in ents:
            ents.append(e)
    st = {"globals": {"dt": DT, "k": KSTIFF, "epsv": EPSV}}
    shift = [mpf(0)] * 3
    if pins and "anchor" in pins:
        a = pins["anchor"]
        st[a] = pins[a]
        shift = _sub(_add(_m(pins[a]["x0"]), _scl(mpf(DT), _m(pins[a]["v1"]))), pts[(a[1], a[2])])
    centre = {side: _f(_add(pts[(side, 0)], shift)) for side in (0, 1)}
    for side, s in ((0, P["A"]), (1, P["B"])):
        if s == "rb":
            st[("body", side)] = pins[("body", side)] if pins else _kin(rng, label == "spin", centre[side] + rng.normal(size=3) * 0.1)
    for e in ents:
        if e[0] == "soft" and e not in st:
            p = _add(pts[(e[1], e[2])], shift)
            v1 = rng.normal(size=3) * 0.3
            st[e] = {"v1": v1, "x0": _f(_sub(p, _scl(mpf(DT), _m(v1))))}
        elif e[0] == "rv":
            b = st[("body", e[1])]
            R = rotation_after_step(_m(b["q0"]), _m(b["bw1"]), mpf(DT))
            t1 = _add(_m(b["t0"]), _scl(mpf(DT), _m(b["bv1"])))
            st[e] = {"xloc": _f(_mtv(R, _sub(_add(pts[(e[1], e[2])], shift), t1)))}
    if P["fam"] == "ee":      # rest edges of deformable sides: lengths that differ from the current ones
        for side in (0, 1):
            e0, e1 = ("soft", side, 0), ("soft", side, 1)
            if e0 in st:
                X0 = np.asarray(st[e0].get("X", rng.normal(size=3) * 0.2))
                d = rng.normal(size=3)
                st[e0] = dict(st[e0], X=X0)
                st[e1] = dict(st[e1], X=X0 + d / np.linalg.norm(d) * rest_len[side])
    return st


def barrier_state(name, label, pins=None):
    P = parse(name)
    rng = _rng(name, label, "shared" if pins else "isolated")
    Q = _rotation(rng)
    e1, e2, n = (_m(Q[:, i]) for i in range(3))
    O = _m(rng.normal(size=3) * 0.3 + (np.array(FAR) if label == "far" else 0.0))
    ta, tb = rng.uniform(0.004, 0.006, 2)
    dhat = mpf(float(ta)) + mpf(float(tb))
    La, Lb = 0.13, 0.08
    if label == "aniso":
        La, Lb = (1e-3, 10.0) if P["fam"] == "ee" else ((1e-3, 1e-3) if P["kind"] in ("pe", "ep") else (10.0, 10.0))
    rest_len = (1.3 * La, 0.8 * Lb)
    at = lambda c1, c2, c3: _add(O, _add(_add(_scl(mpf(c1), e1), _scl(mpf(c2), e2)), _scl(c3 if isinstance(c3, mpf) else mpf(c3), n)))
    theta0, gam = 0.7, 0.4

    def geometry(s, th):
        c, sn = MP.cos(th), MP.sin(th)
        cg, sg = math.cos(gam), math.sin(gam)
        if P["fam"] == "pt":
            L = La
            prim = {1: [at(0, 0, 0)], 2: [at(-0.4 * L, 0.05 * L, 0), at(0.6 * L, -0.075 * L, 0)], 3: [at(-0.3 * L, -0.3 * L, 0), at(0.7 * L, -0.2 * L, 0), at(-0.2 * L, 0.6 * L, 0)]}
            ka, kb = PT_K[P["kind"]]
            pt_side = 0 if ka == 1 and P["kind"] not in ("ep", "tp") else 1
            pts = {(pt_side, 0): at(0, 0, s)}
            for i, p in enumerate(prim[kb if pt_side == 0 else ka]):
                pts[(1 - pt_side, i)] = p
            return pts
        f = e1
        k = P["kind"]
        if k == "ee":      # interior pair: eb turns about the common normal n through its closest point
            g = _add(_scl(c, e1), _scl(sn, e2))
            m0 = at(0, 0, s)
            return {(0, 0): at(-0.4 * La, 0, 0), (0, 1): at(0.6 * La, 0, 0), (1, 0): _sub(m0, _scl(mpf(0.45 * Lb), g)), (1, 1): _add(m0, _scl(mpf(0.55 * Lb), g))}
        if k == "pe":      # p = ea's end 1 against the interior of eb; ea turns about p away from eb
            ua = _add(_scl(c, f), _add(_scl(-sn * cg, n), _scl(sn * sg, e2)))
            return {(0, 1): at(0, 0, 0), (0, 0): _add(at(0, 0, 0), _scl(mpf(La), ua)), (1, 0): at(-0.4 * Lb, 0, s), (1, 1): at(0.6 * Lb, 0, s)}
        if k == "ep":      # q = eb's end 0 against the interior of ea
            ub = _add(_scl(c, f), _add(_scl(sn * cg, n), _scl(sn * sg, e2)))
            return {(0, 0): at(-0.4 * La, 0, 0), (0, 1): at(0.6 * La, 0, 0), (1, 0): at(0, 0, s), (1, 1): _add(at(0, 0, s), _scl(mpf(Lb), ub))}
        # pp: p = ea's end 1, q = eb's end 0, both edges leave the pair; eb = -(ea turned by theta about an axis across it)
        al = 0.5
        ua = _add(_scl(mpf(math.cos(al)), e1), _scl(mpf(-math.sin(al)), n))
        ub = _scl(-1, _add(_scl(c, ua), _scl(sn, e2)))
        return {(0, 1): at(0, 0, 0), (0, 0): _add(at(0, 0, 0), _scl(mpf(La), ua)), (1, 0): at(0, 0, s), (1, 1): _add(at(0, 0, s), _scl(mpf(Lb), ub))}

    def build(s, th):
        r = _rng(name, label, "shared" if pins else "isolated", "place")
        pts = geometry(s, th)
        if P["fam"] == "ee":      # the point of a side is its edge's end vertex
            pts[(0, 2)], pts[(1, 2)] = pts[(0, 1)], pts[(1, 0)]
        st = _place(name, label, pins, r, pts, rest_len)
        st[("obj", 0)], st[("obj", 1)] = {"thick": float(ta)}, {"thick": float(tb)}
        return st

    s0 = dhat * mpf(D_TARGET.get(label, 0.6))
    th = mpf(theta0)
    if label in X_TARGET:     # x = |ea|^2 |eb|^2 sin^2 theta whatever s is: the angle first, then the gap
        m0 = measure(name, build(s0, th))
        th = MP.asin(MP.sqrt(mpf(X_TARGET[label]) * m0["eps_x"] / (m0["x"] / MP.sin(th) ** 2)))
        th = _solve(lambda t: build(s0, t), lambda st_: _ratio(name, st_, "x", "eps_x"), th, mpf(X_TARGET[label]))[1]
    return _solve(lambda s: build(s, th), lambda st_: _ratio(name, st_, "d", "dhat"), s0, mpf(D_TARGET.get(label, 0.6)))[0]


def friction_weights(kind, bary):
    if kind == "pp":
        return [-1.0], [1.0]
    if kind in ("pe", "pt"):
        return [-1.0], list(bary)
    if kind == "ee":
        return [-(1.0 - bary[0]), -bary[0]], [1.0 - bary[1], bary[1]]
    return list(bary), [-1.0]


def friction_state(name, label, pins=None):
    P = parse(name)
    kind = P["kind"]
    rng = _rng(name, label, "shared" if pins else "isolated")
    Q = _rotation(rng)
    T = np.concatenate([Q[0], Q[1]])
    nrm = _m(Q[2])
    nb = NBARY[kind]
    bary = {0: None, 2: np.array([0.35, 0.6]) if kind == "ee" else np.array([0.3, 0.7]), 3: np.array([0.2, 0.5, 0.3])}[nb]
    if label == "corner" and nb:
        bary = np.array([0.0, 0.6]) if kind == "ee" else (np.array([0.0, 1.0]) if nb == 2 else np.array([0.4, 0.0, 0.6]))
    mu, fn = float(rng.uniform(0.2, 0.8)), float(rng.uniform(5.0, 50.0))
    ka, kb = FR_K[kind]
    wa, wb = friction_weights(kind, bary)
    wts = {(0, i): wa[i] for i in range(ka)}
    wts.update({(1, i): wb[i] for i in range(kb)})
    rest_exact = label == "rest" and not pins
    psi = float(rng.uniform(0.3, 1.2))
    S = bound_schema(name)
    ents = []
    for _, _, e, _, _, _ in S:
        if e is not None and e not in ents:
            ents.append(e)

    def build(speed):
        r = _rng(name, label, "shared" if pins else "isolated", "place")
        st = {"globals": {"dt": DT, "k": KSTIFF, "epsv": EPSV}, ("row",): {"T": T, "mu": mu, "fn": fn}}
        if nb:
            st[("row",)]["bary%d" % nb] = bary
        if pins and "anchor" in pins:
            st[pins["anchor"]] = pins[pins["anchor"]]
        for side, s in ((0, P["A"]), (1, P["B"])):
            if s == "rb":
                st[("body", side)] = pins[("body", side)] if pins else _kin(r, label == "spin", still=rest_exact)
        free = None
        for e in ents:
            if e[0] == "soft" and e not in st:
                st[e] = {"v1": np.zeros(3) if rest_exact else r.normal(size=3) * 0.2}
                if free is None and abs(wts[(e[1], e[2])]) > 0.25:
                    free = e
            elif e[0] == "rv":
                st[e] = {"xloc": r.normal(size=3) * 0.1}
        if rest_exact:
            return st
        if free is None:
            free = [e for e in ents if e[0] == "rv" and abs(wts[(e[1], e[2])]) > 0.25][-1]
        # the relative velocity wanted: tangential part of the wanted size and direction, a generic normal part
        t0, t1 = _m(T[0:3]), _m(T[3:6])
        Vt = _add(_scl(speed * mpf(math.cos(psi)), t0), _scl(speed * mpf(math.sin(psi)), t1))
        Rm = {}

        def vel(e):
            if e[0] == "soft":
                return _m(st[e]["v1"])
            b = st[("body", e[1])]
            if e[1] not in Rm:
                Rm[e[1]] = rotation_after_step(_m(b["q0"]), _m(b["bw1"]), mpf(DT))
            return _add(_m(b["bv1"]), _cross(_m(b["bw1"]), _mv(Rm[e[1]], _m(st[e]["xloc"]))))
        others = [mpf(0)] * 3
        for e in ents:
            if e[0] in ("soft", "rv") and e != free:
                others = _add(others, _scl(mpf(wts[(e[1], e[2])]), vel(e)))
        wf = mpf(wts[(free[1], free[2])])
        if free[0] == "soft":
            V = _add(Vt, _scl(mpf(0.05), nrm))
            st[free] = {"v1": _f(_scl(1 / wf, _sub(V, others)))}
        else:                 # a rigid vertex: w x r = Y needs Y . w = 0, which the normal part of the relative velocity provides
            b = st[("body", free[1])]
            vel(free)
            w = _m(b["bw1"])
            Y0 = _sub(_scl(1 / wf, _sub(Vt, others)), _m(b["bv1"]))
            alpha = -wf * _dot(Y0, w) / _dot(nrm, w)
            Y = _add(Y0, _scl(alpha / wf, nrm))
            ww = _dot(w, w)
            rr = _add(_scl(1 / ww, _cross(Y, w)), _scl(mpf(0.08) / MP.sqrt(ww), w))
            st[free] = {"xloc": _f(_mtv(Rm[free[1]], rr))}
        return st

    if rest_exact:
        return build(None)
    epsu = mpf(DT) * mpf(EPSV)
    if label == "rest":       # (shared: the common velocities cancel in the tangent plane)
        return build(mpf(0))
    target = mpf(U_TARGET[label])
    return _solve(build, lambda st_: _ratio(name, st_, "u", "epsu"), target * epsu / mpf(DT), target)[0]


def labels(name):
    P = parse(name)
    rigid = "rb" in (P["A"], P["B"])
    if P["fam"] == "friction":
        return [l for l in FRICTION_STATES if (l != "spin" or rigid) and (l != "corner" or NBARY[P["kind"]])]
    return [l for l in BARRIER_STATES if l != "spin" or rigid] + (MOLL_STATES if P["fam"] == "ee" else [])


_STATES = {}


def states(name, layout_="isolated"):
    """[(label, state)] of a potential; `shared` has its own, built around what the rows have in common"""
    key = (name, layout_)
    if key not in _STATES:
        pins = make_pins(name) if layout_ == "shared" else None
        make = friction_state if parse(name)["fam"] == "friction" else barrier_state
        _STATES[key] = [(l, make(name, l, pins)) for l in labels(name)]
    return _STATES[key]


def kind_of(name):
    P = parse(name)
    return "%s_%s" % (P["fam"], "rigid" if "rb" in (P["A"], P["B"]) else "soft")


# ======================================================================================================================================
# tables: arrays, connectivity, the oracle's Problem
# ======================================================================================================================================
class World:
    """One set of arrays by role for any number of tables (one DoF array per DoF set)."""

    def __init__(self):
        self.n = {"soft": 0, "body": 0, "rv": 0, "obj": 0, "row": 0}
        self.writes = []      # (role, index, value)
        self.tables = []

    def add_table(self, name, layout_="isolated", n_rows=NE):
        S = bound_schema(name)
        L = layout(name)
        sts = states(name, "shared" if layout_ == "shared" else "isolated")
        ents = {}
        for _, _, e, _, _, _ in S:
            if e is not None and e not in ents.setdefault(e[0], []):
                ents[e[0]].append(e)
        base = dict(self.n)
        shared = layout_ == "shared"

        def index(e, row):
            cls, k, m = e[0], ents[e[0]].index(e), len(ents[e[0]])
            if shared and cls == "body":
                return base[cls] + k
            if shared and cls == "soft":
                return base[cls] + (0 if k == 0 else 1 + row * (m - 1) + (k - 1))
            return base[cls] + row * m + k
        for cls, es in ents.items():
            m = len(es)
            self.n[cls] += m if (shared and cls == "body") else (1 + n_rows * (m - 1) if (shared and cls == "soft") else n_rows * m)
        conn = np.zeros((n_rows, L["conn_stride"]), dtype=np.int32)
        state_of_row = np.arange(n_rows) % len(sts)
        for row in range(n_rows):
            st = sts[state_of_row[row]][1]
            for role, _, e, _, col, _ in S:
                if e is None:
                    continue
                i = index(e, row)
                conn[row, col] = i
                self.writes.append((role, i, st[e][role]))
        t = {"name": name, "layout": layout_, "conn": conn, "state_of_row": state_of_row, "states": sts, "index": len(self.tables)}
        self.tables.append(t)
        return t

    def problem(self):
        arrays = {}
        for role in ROLES:
            cls = CLASS_OF.get(role)
            arrays[role] = np.zeros((self.n[cls] if cls else 1, ROLE_STRIDE[role]))
        for role, v in (("dt", DT), ("k", KSTIFF), ("epsv", EPSV)):
            arrays[role][0, 0] = v
        seen = {}
        for role, i, v in self.writes:
            v = np.atleast_1d(np.asarray(v, dtype=np.float64))
            if (role, i) in seen:
                assert (seen[(role, i)].view(np.int64) == v.view(np.int64)).all(), ("what the rows share must have one state", role, i)
            seen[(role, i)] = v
            arrays[role][i] = v
        pots = []
        for t in self.tables:
            bs = [ev.Binding(ROLES.index(role), stride, col, dof) for role, _, _, stride, col, dof in bound_schema(t["name"])]
            for role, _, _, _, col, _ in bound_schema(t["name"]):
                assert col < 0 or (0 <= t["conn"][:, col].min() and t["conn"][:, col].max() < len(arrays[role])), (t["name"], role)   # every index inside its array
            pots.append(ev.PotentialDesc(t["name"], t["conn"], bs, False))
        sizes = [3 * self.n["soft"], 3 * self.n["body"], 3 * self.n["body"]]
        offs = [0, sizes[0], sizes[0] + sizes[1]]
        dof_arrays = {s: ROLES.index(r) for r, s in ROLE_DOF.items() if sizes[s] > 0}
        return ev.Problem(dt=DT, ndofs=sum(sizes), dof_offsets=offs, dof_sizes=sizes, arrays=[np.ascontiguousarray(arrays[r]) for r in ROLES], potentials=pots, dof_arrays=dof_arrays)


class Table:
    """One potential, one layout: the Problem, which state each row holds, and the exact numbers per row."""

    def __init__(self, name, layout_="isolated", n_rows=NE, world=None):
        self.name, self.layout, self.n_rows = name, layout_, n_rows
        w = world or World()
        self.t = w.add_table(name, layout_, n_rows)
        self.world = w
        if world is None:
            self.prob = w.problem()
            self.pot = self.prob.potentials[0]
        self.state_of_row = self.t["state_of_row"]
        self.labels = [l for l, _ in self.t["states"]]

    def bind(self, prob):
        self.prob, self.pot = prob, prob.potentials[self.t["index"]]
        return self

    @property
    def nb(self):
        return len(ev.dof_layout(self.pot))

    def block_rows(self):
        order = ev.dof_layout(self.pot)
        return np.stack([self.prob.dof_offsets[self.pot.bindings[bi].dof_set] // 3 + self.pot.conn[:, self.pot.bindings[bi].conn] for bi in order], axis=1).astype(np.int64)

    def gathered(self):
        """[n_rows, n_inputs]: what the kernels gather per row"""
        cols = []
        for b in self.pot.bindings:
            data = self.prob.arrays[b.array]
            cols.append(data[self.pot.conn[:, b.conn]] if b.conn >= 0 else np.broadcast_to(data[0], (self.n_rows, b.stride)))
        return np.ascontiguousarray(np.concatenate(cols, axis=1))

    def exact_rows(self):
        """(E [n_rows], g [n_rows, n], H [n_rows, n, n]) — every row takes its state's reference"""
        per = [exact(self.name, self.layout if self.layout == "shared" else "isolated", i) for i in range(len(self.labels))]
        s = self.state_of_row
        return np.array([per[i][0] for i in s]), np.stack([per[i][1] for i in s]), np.stack([per[i][2] for i in s])

    def scales(self):
        E, g, H = self.exact_rows()
        return {"energy": np.abs(E), "gradient": np.abs(g).max(axis=1), "hessian": np.abs(H).max(axis=(1, 2))}


def in_dof(name):
    """input index -> local DoF (or -1), in the oracle's local order (oracle.evaluator.dof_layout)"""
    S = bound_schema(name)
    pot = ev.PotentialDesc(name, np.zeros((0, 1), dtype=np.int32), [ev.Binding(0, s, c, d) for _, _, _, s, c, d in S])
    order = ev.dof_layout(pot)
    starts = np.cumsum([0] + [s for _, _, _, s, _, _ in S])
    d = -np.ones(starts[-1], dtype=np.int64)
    for k, bi in enumerate(order):
        d[starts[bi]:starts[bi] + 3] = 3 * k + np.arange(3)
    return d, 3 * len(order)


_EXACT = {}


def exact(name, layout_, i):
    """(E, g [n], H [n, n]) of state i of a potential, rounded from 40 digits"""
    key = (name, layout_, i)
    if key not in _EXACT:
        x = flat(name, states(name, layout_)[i][1])
        d, n = in_dof(name)
        r, _ = energy(name, [J.var(mpf(c), int(d[k])) if d[k] >= 0 else mpf(c) for k, c in enumerate(x)])
        g, H = np.zeros(n), np.zeros((n, n))
        for a, v in r.g.items():
            g[a] = float(v)
        for (a, b), v in r.h.items():
            H[a, b] = H[b, a] = float(v)
        _EXACT[key] = (float(r.v), g, H)
    return _EXACT[key]


def exact_energy_mp(name, x):
    """the mpmath energy alone at inputs x (mpf): for central differences"""
    return energy(name, list(x))[0]


# ---- the float64 oracle, in the reference's operation order and in the closed form's --------------------------------------------------------
def oracle_rows(table):
    o = ev.evaluate_potential(table.prob, table.pot)
    return o.E, o.g, o.H, o.block_rows


def _plane_closed_order(p, a, b_, c):
    n = ad.cross(ad.sub(a, c), ad.sub(b_, c))
    l = ad.dot(ad.sub(p, a), n)
    return (l * l / ad.sqnorm(n)).sqrt()


def oracle_alt(table):
    """The same float64 evaluation with the point-plane distance as contact_closed.hpp orders it: (u . n)^2 / |n|^2 with the unnormalised normal."""
    saved = en._distance_point_plane
    en._distance_point_plane = _plane_closed_order
    try:
        o = ev.evaluate_potential(table.prob, table.pot)
    finally:
        en._distance_point_plane = saved
    return o.E, o.g, o.H, o.block_rows


def row_errors(E, g, H, ex):
    """per row: |. - exact| / the row's largest exact entry of the quantity"""
    Ee, ge, He = ex
    with np.errstate(divide="ignore", invalid="ignore"):
        out = {"energy": np.abs(E - Ee) / np.abs(Ee), "gradient": np.abs(g - ge).max(axis=1) / np.abs(ge).max(axis=1),
               "hessian": np.abs(H - He).max(axis=(1, 2)) / np.abs(He).max(axis=(1, 2))}
    return out


def measure_tolerances(names=None):
    """"<layout>/<label>/<kind>" -> quantity -> the largest error of the float64 oracle (either operation order) against `exact` (the states of
    `shared` are states of their own, so they have entries of their own)"""
    tab = {}
    for name in (NAMES if names is None else names):
        for lay in ("isolated", "shared"):
            n = len(labels(name))
            t = Table(name, lay, n)
            ex = t.exact_rows()
            errs = [row_errors(*oracle_rows(t)[:3], ex), row_errors(*oracle_alt(t)[:3], ex)]
            for i, l in enumerate(t.labels):
                e = tab.setdefault("%s/%s/%s" % (lay, l, kind_of(name)), {"energy": 0.0, "gradient": 0.0, "hessian": 0.0})
                for q in e:
                    e[q] = max(e[q], float(errs[0][q][i]), float(errs[1][q][i]))
    return tab


def write_tolerances(path=TOLERANCES):
    """Regenerates tests/contact_tolerances.json:  python -c "import contact_cases as c; c.write_tolerances()"  from tests/ (repository root on PYTHONPATH)."""
    with open(path, "w") as f:
        json.dump(measure_tolerances(), f, indent=1, sort_keys=True)
        f.write("\n")


_TAB = {}


def bounds(table):
    """Absolute bounds per row of a device result against `exact`: {"energy": [n_rows], "gradient": [n_rows], "hessian": [n_rows]}"""
    if not _TAB:
        with open(TOLERANCES) as f:
            _TAB.update(json.load(f))
    sc = table.scales()
    lay = "shared" if table.layout == "shared" else "isolated"
    rel = {q: np.array([max(8.0 * _TAB["%s/%s/%s" % (lay, table.labels[i], kind_of(table.name))][q], FLOOR) for i in table.state_of_row]) for q in sc}
    return {q: rel[q] * sc[q] for q in sc}


def merged_tables(layout_="isolated", n_rows=NE):
    """All 35 potentials in one Problem (one set of DoF arrays): what the shared launch of the generic kernel needs."""
    w = World()
    ts = [Table(name, layout_, n_rows, world=w) for name in NAMES]
    prob = w.problem()
    return prob, [t.bind(prob) for t in ts]


def custom_ops(tables):
    """the goldens' SymX op arrays keyed as gpu_util.engine_from_problem(custom_ops=...) reads them"""
    z = {}
    for t in tables:
        for k, v in layout(t.name)["ops"].items():
            z["p%d_%s" % (t.t["index"], k)] = v
    return z
