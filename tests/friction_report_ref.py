"""Numpy restatement of the friction report (include/mistark_contact.h "friction report").

The rows are driven by the friction tables themselves: per table 21..34, in table order, the connectivity rows (idx | [rigid bodies] | vertices of the side
listed first | of the side listed second) with their lagged T, mu, fn and bary — the fixture's, or what an engine returns through contact_table /
contact_friction_data — and the velocity state. Roles follow the potential (oracle/energies.py:_friction): v = v_B - v_A; for the kinds pp, pe, pt, ee A
is the side listed first, for ep and tp the single point listed last. Groups and collision vertices come from the physical vertex indices: a vertex of a
physical system belongs to one collision mesh.

`rows` restates the row records, `vertex_report` and `pair_report` the two sums (terms in row order, plain sequential sums; the tests bound them against
math.fsum)."""
import functools
import math
import os

import numpy as np

from oracle import contact as oc
from oracle import evaluator as ev

from contact_report_ref import Layout, triangle_areas

U = 2.0 ** -53
TABLE_NAMES = [
    "friction_d_d_pp_C0", "friction_d_d_pe_C0", "friction_d_d_pt_C0", "friction_d_d_ee_C0",
    "friction_rb_rb_pp_C0", "friction_rb_rb_pe_C0", "friction_rb_rb_pt_C0", "friction_rb_rb_ee_C0",
    "friction_rb_d_pp_C0", "friction_rb_d_pe_C0", "friction_rb_d_pt_C0", "friction_rb_d_ee_C0", "friction_rb_d_ep_C0", "friction_rb_d_tp_C0"]
FIRST_TABLE = 21
SLIDING, NO_LOAD, DEGENERATE = 1, 2, 4
FIXTURES = ["contactmix_t0", "contactmix_t1", "contactcorners_t0", "contactrods_t0", "contactrods_t1"]
STATE_SCALES = [0.0, 0.1, 0.2]
KA = [1, 1, 1, 2, 2, 3]  # vertices of the side listed first, by kind
KB = [1, 2, 3, 2, 1, 1]


def table_shape(t):
    """(kind 0..5, system of the side listed first, of the side listed second, first vertex column) of friction table t = 0..13."""
    fam, kind = (0, t) if t < 4 else ((1, t - 4) if t < 8 else (2, t - 8))
    return kind, ("d" if fam == 0 else "rb"), ("rb" if fam == 1 else "d"), (1 if fam == 0 else (3 if fam == 1 else 2))


def vertex_index(scene):
    """(system, physical vertex index) -> collision vertex."""
    L = Layout(scene)
    out = {}
    for g, m in enumerate(scene.meshes):
        for j, s in enumerate(m.verts):
            key = (m.kind, int(s))
            assert key not in out, key
            out[key] = int(L.v_off[g] + j)
    return out


def rigid_velocity(st, body, xloc, dt):
    """global_point_velocity_in_rigid_body: v1 + w1 x (R1 xloc)."""
    w = st["rb_w1"][body]
    R1 = oc.quat_to_R(oc.quat_time_integration(st["rb_q0"][body], w, dt))
    return st["rb_v1"][body] + np.cross(w, R1 @ xloc)


def rows(scene, tables, st, dt, epsv):
    """tables: name -> dict(conn [n, stride], T [n, 6], mu [n], fn [n], bary [n, nb] or None), the rows of a table in ITS order.
    Returns (ints [n, 8], doubles [n, 24], per row its signed (collision vertex, weight) contributions: A's vertices with +w, then B's with -w)."""
    L = Layout(scene)
    cv_of = vertex_index(scene)
    ri, rd, contrib = [], [], []
    for t, name in enumerate(TABLE_NAMES):
        tb = tables.get(name)
        if tb is None or len(tb["conn"]) == 0:
            continue
        kind, sys1, sys2, base = table_shape(t)
        for r, row in enumerate(np.asarray(tb["conn"])):
            first = [int(v) for v in row[base:base + KA[kind]]]
            second = [int(v) for v in row[base + KA[kind]:base + KA[kind] + KB[kind]]]
            rb1 = int(row[1]) if sys1 == "rb" else -1
            rb2 = int(row[2]) if (sys1 == "rb" and sys2 == "rb") else -1
            sides = [(sys1, rb1, first), (sys2, rb2, second)]
            A, B = (sides[1], sides[0]) if kind >= 4 else (sides[0], sides[1])

            def vel(side):
                s, body, verts = side
                return [st["v1"][v] if s == "d" else rigid_velocity(st, body, st["rb_xloc"][v], dt) for v in verts]

            va, vb = vel(A), vel(B)
            bary = None if tb.get("bary") is None or kind == 0 else np.asarray(tb["bary"]).reshape(len(tb["conn"]), -1)[r]
            if kind == 0:
                wa, wb, pa, pb = [1.0], [1.0], va[0], vb[0]
            elif kind in (1, 4):
                wa, wb, pa, pb = [1.0], [bary[0], bary[1]], va[0], bary[0] * vb[0] + bary[1] * vb[1]
            elif kind in (2, 5):
                wa, wb, pa, pb = [1.0], [bary[0], bary[1], bary[2]], va[0], bary[0] * vb[0] + bary[1] * vb[1] + bary[2] * vb[2]
            else:
                wa, wb = [1.0 - bary[0], bary[0]], [1.0 - bary[1], bary[1]]
                pa, pb = va[0] + bary[0] * (va[1] - va[0]), vb[0] + bary[1] * (vb[1] - vb[0])
            v = pb - pa
            T = np.asarray(tb["T"]).reshape(-1, 6)[r]
            mu, fn = float(np.asarray(tb["mu"]).reshape(-1)[r]), float(np.asarray(tb["fn"]).reshape(-1)[r])
            u0 = float(T[0:3] @ v) * dt + 1.13e-9
            u1 = float(T[3:6] @ v) * dt - 1.07e-9
            un = math.sqrt(u0 * u0 + u1 * u1)
            epsu, mufn = dt * epsv, mu * fn
            stick = un < epsu
            E = 0.5 * (mufn / epsu) * (un * un) if stick else mufn * (un - 0.5 * epsu)
            c = mufn / epsu if stick else (0.0 if mufn == 0.0 else mufn / un)
            ft = c * (u0 * T[0:3] + u1 * T[3:6])
            fmag = math.sqrt(float(ft @ ft))
            mob = 0.0 if mufn == 0.0 else min(fmag / mufn, 1.0)
            cva, cvb = [cv_of[(A[0], x)] for x in A[2]], [cv_of[(B[0], x)] for x in B[2]]
            ga, gb = int(L.cv_mesh[cva[0]]), int(L.cv_mesh[cvb[0]])
            ri.append([FIRST_TABLE + t, r, kind, ga, gb, A[1], B[1], (0 if stick else SLIDING) | (NO_LOAD if mufn == 0.0 else 0)])
            wb3 = list(wb) + [0.0] * (3 - len(wb))
            rd.append([mu, fn, epsu, u0, u1, un, un / dt, v[0], v[1], v[2], ft[0], ft[1], ft[2], fmag, mob, float(ft @ v), E, (bary[0] if kind == 3 else 0.0)] + wb3 + [0.0, 0.0, 0.0])
            contrib.append([(cv, w) for cv, w in zip(cva, wa)] + [(cv, -w) for cv, w in zip(cvb, wb)])
    return np.array(ri, dtype=np.int32).reshape(-1, 8), np.array(rd, dtype=np.float64).reshape(-1, 24), contrib


def vertex_report(scene, ri, rd, contrib, X):
    """(records [n_v, 8], per vertex the list of its s w ft terms (3-vectors) in row order)."""
    L = Layout(scene)
    out = np.zeros((L.n_v, 8))
    terms = [[] for _ in range(L.n_v)]
    for n, cs in enumerate(contrib):
        if ri[n, 7] & DEGENERATE:
            continue
        for v, w in cs:
            out[v, 0] += 1
            out[v, 1] += 1 if ri[n, 7] & SLIDING else 0
            out[v, 5] = max(out[v, 5], rd[n, 6])
            terms[v].append(w * rd[n, 10:13])
    ta = triangle_areas(scene, X)
    area = np.zeros(L.n_v)
    for t in range(L.n_t):
        for v in L.tri[t]:
            area[v] += ta[t]
    out[:, 6] = area / 3.0
    for v in range(L.n_v):
        s = np.zeros(3)
        for x in terms[v]:
            s = s + x
        out[v, 2:5] = s
        out[v, 7] = math.sqrt(float(s @ s)) / out[v, 6] if out[v, 6] > 0.0 else 0.0
    return out, terms


PAIR_SUMS = {2: "fn", 3: "mufn", 4: "ftx", 5: "fty", 6: "ftz", 7: "fmag", 8: "diss", 9: "E"}


def pair_report(scene, ri, rd):
    """(records [G, G, 12], terms[(ga, gb)] = per summed field 2..9 the list of terms in row order)."""
    G = len(scene.meshes)
    out = np.zeros((G, G, 12))
    terms = {(a, b): {f: [] for f in PAIR_SUMS} for a in range(G) for b in range(a, G)}
    for n in range(len(ri)):
        if ri[n, 7] & DEGENERATE:
            continue
        ga, gb = int(ri[n, 3]), int(ri[n, 4])
        lo, hi = min(ga, gb), max(ga, gb)
        sign = 1.0 if ga <= gb else -1.0
        out[lo, hi, 0] += 1
        out[lo, hi, 1] += 1 if ri[n, 7] & SLIDING else 0
        out[lo, hi, 10] = max(out[lo, hi, 10], rd[n, 6])
        T = terms[(lo, hi)]
        T[2].append(rd[n, 1])
        T[3].append(rd[n, 0] * rd[n, 1])
        for c in range(3):
            T[4 + c].append(sign * rd[n, 10 + c])
        T[7].append(rd[n, 13])
        T[8].append(rd[n, 15])
        T[9].append(rd[n, 16])
    for (ga, gb), T in terms.items():
        for f, xs in T.items():
            s = 0.0
            for x in xs:
                s += x
            out[ga, gb, f] = s
        out[ga, gb, 11] = out[ga, gb, 7] / out[ga, gb, 3] if out[ga, gb, 3] != 0.0 else 0.0
    return out, terms


def sum_bound(xs):
    """(n + 8) 2^-53 sum |terms|: any summation order of n scalar terms against math.fsum of the same terms."""
    return (len(xs) + 8) * U * math.fsum(abs(x) for x in xs)


def vector_sum_bound(vs):
    """The same bound for a sum of n vectors, per component, with |term| the VECTOR's magnitude (the components of a term come out of
    products that mix them, so each carries a rounding error relative to the term's norm)."""
    return (len(vs) + 8) * U * math.fsum(math.sqrt(float(np.dot(v, v))) for v in vs)


def fsum3(vs):
    return np.array([math.fsum(v[k] for v in vs) for k in range(3)]) if len(vs) else np.zeros(3)


def bounds_of(ri):
    return np.searchsorted(ri[:, 0] if len(ri) else np.zeros(0), FIRST_TABLE + np.arange(15), side="left")


GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def fixture_tables(prob):
    """The 14 friction tables of a fixture in the shape `rows` takes."""
    out = {}
    for pot in prob.potentials:
        if pot.name not in TABLE_NAMES or len(pot.conn) == 0:
            continue
        rec = oc.RECIPES[pot.name][1]
        tb = dict(conn=pot.conn, bary=None)
        for (role, _, _), b in zip(rec, pot.bindings):
            if role in ("T", "mu", "fn", "bary"):
                tb[role] = np.asarray(prob.arrays[b.array])[pot.conn[:, b.conn]]
        out[pot.name] = tb
    return out


@functools.lru_cache(maxsize=None)
def fixture_case(name, state):
    """A contact fixture at DoFs u + STATE_SCALES[state] r, r = default_rng(7).standard_normal in Problem.get_dofs() order, evaluated once per process and
    shared (read-only). The friction tables stay the fixture's: they are lagged."""
    from contact_util import state_from_fixture

    prob, man, z = ev.load_fixture(os.path.join(GOLDEN, name + ".npz"))
    u = prob.get_dofs()
    r = np.random.default_rng(7).standard_normal(u.shape)
    u = u + STATE_SCALES[state] * r
    prob.set_dofs(u)
    st, _ = state_from_fixture(prob, man)
    scene = oc.scene_from_fixture(man, z)
    dt = float(np.asarray(st["dt"]).ravel()[0])
    epsv = float(np.asarray(st["epsv"]).ravel()[0])
    tables = fixture_tables(prob)
    ri, rd, contrib = rows(scene, tables, st, dt, epsv)
    X = np.concatenate(oc.mesh_vertices(scene, st, dt))
    for a in (ri, rd, X, u):
        a.setflags(write=False)
    return dict(prob=prob, man=man, st=st, scene=scene, dt=dt, epsv=epsv, tables=tables, ri=ri, rd=rd, contrib=contrib, X=X, u=u)


def field_scales(ri, rd, vmax, dt):
    """The magnitude every double field of a row is measured against. vmax: the largest |velocity component| the rows were formed from. The slip is a
    difference of velocities times dt, so its rounding error is relative to vmax dt, not to its own size (a sticking row has |u| < epsu = 1e-5 m beside
    vmax dt of millimetres); force, mobilised share, dissipation and energy inherit that through c = mu fn / epsu (sticking) or mu fn / |u| (sliding)."""
    s = np.ones_like(rd)
    mufn = np.maximum(rd[:, 0] * rd[:, 1], 1e-300)
    ubig = np.maximum(rd[:, 5], vmax * dt)
    stick = (ri[:, 7] & SLIDING) == 0
    c = np.where(stick, mufn / rd[:, 2], mufn / np.maximum(rd[:, 5], 1e-300))
    s[:, 0], s[:, 1], s[:, 2] = np.maximum(rd[:, 0], 1e-300), np.maximum(rd[:, 1], 1e-300), rd[:, 2]
    s[:, 3] = s[:, 4] = s[:, 5] = ubig
    s[:, 6] = ubig / dt
    s[:, 7:10] = vmax
    s[:, 10:13] = np.reshape(c * ubig, (-1, 1))
    s[:, 13] = c * ubig
    s[:, 14] = np.maximum(1.0, c * ubig / mufn)
    s[:, 15] = c * ubig * vmax
    s[:, 16] = np.where(stick, c * ubig * ubig, mufn * ubig)
    s[:, 17:21] = np.maximum(1.0, np.abs(rd[:, 17:21]))
    return s


def state_vmax(st):
    """Largest |velocity component| of any collision vertex's velocity can be formed from: v1, rb_v1 and |rb_w1| |xloc|."""
    m = 0.0
    if "v1" in st and st["v1"].size:
        m = max(m, float(np.abs(st["v1"]).max()))
    if "rb_v1" in st and st["rb_v1"].size:
        m = max(m, float(np.abs(st["rb_v1"]).max()) + float(np.linalg.norm(st["rb_w1"], axis=1).max()) * float(np.linalg.norm(st["rb_xloc"], axis=1).max()))
    return m
