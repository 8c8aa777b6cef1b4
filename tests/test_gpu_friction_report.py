"""GPU tests of the friction report (include/mistark_contact.h "friction report", stark_amd/csrc/friction_report.hip) on the contact fixtures, against the
numpy restatement of tests/friction_report_ref.py, the g++ build of the arithmetic header and the engine's own evaluation and force readout.

States: every fixture at its stored DoFs u, at u + 0.1 r and at u + 0.2 r (r = default_rng(7).standard_normal in Problem.get_dofs() order) with the
friction tables the device search installs at the fixture's state; tests/test_friction_report_cpu.py says why.

Tolerances: ints, flags, counts and maxima exact; row doubles 1e-12 of the field's scale against the header's host build (device FMA contraction may
differ; the CPU test pins the header to the restatement); energies 1e-11 relative against Engine.element_energies and node forces 1e-11 mu fn against
Engine.element_forces (the project's element tolerance); a sum of n terms (n + 8) * 2^-53 * sum |terms| against math.fsum of the same terms, |term| the
vector's magnitude for a sum of vectors."""
import ctypes as C
import math
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import friction_report_ref as fr  # noqa: E402
import test_friction_report_cpu as cpu  # noqa: E402
import test_gpu_contact_report as tcr  # noqa: E402
from oracle import contact as oc  # noqa: E402

pytestmark = pytest.mark.gpu
U = fr.U
_host = []


def host_lib():
    if not _host:
        out = os.path.join(tempfile.mkdtemp(prefix="mistark_host_friction_report_"), "host_friction_report.so")
        subprocess.run(["g++", "-std=c++17", "-O2", "-shared", "-fPIC", cpu.SRC, "-o", out], check=True)
        lib = C.CDLL(out)
        p = C.c_void_p
        lib.host_friction_rows.argtypes = [p, p, p, p, p, p, C.c_double, C.c_double, C.c_int, p, p, p]
        lib.host_friction_rigid_velocity.argtypes = [p, p, p, p, C.c_double, p]
        _host.append(lib)
    return _host[0]


def engine_tables(eng):
    """The 14 friction tables as installed, in the shape friction_report_ref.rows takes."""
    out = {}
    for name in fr.TABLE_NAMES:
        conn = eng.contact_table(name)
        if len(conn):
            tb = eng.contact_friction_data(name, len(conn))
            tb.setdefault("bary", None)
            tb["conn"] = conn
            out[name] = tb
    return out


def installed(name):
    """The fixture with its friction tables installed, and barrier searches run SINCE: the report must not depend on the detector's key buffers."""
    eng, c = tcr.build(name)
    n = eng.contact_update_friction()
    assert n == cpu.ROWS[name]
    eng.contact_update(c["dt"])
    return eng, c, engine_tables(eng)


def restated(c0, tables, name, s):
    """Restatement at state s with the ENGINE's tables (their row order is the device's)."""
    cs = fr.fixture_case(name, s)
    ri, rd, contrib = fr.rows(cs["scene"], tables, cs["st"], cs["dt"], cs["epsv"])
    return cs, ri, rd, contrib


def dof_rows(c):
    return tcr.dof_row0(c, "v1"), tcr.dof_row0(c, "rb_v1"), tcr.dof_row0(c, "rb_w1")


def node_rows(c, contrib_row, v1, rbv):
    """Block row of every contribution of a row: the node of a deformable vertex, the linear block of a rigid vertex's body."""
    L = fr.Layout(c["scene"])
    M = c["scene"].meshes
    out = []
    for cv, w in contrib_row:
        g = int(L.cv_mesh[cv])
        out.append(v1[0] + int(L.cv_src[cv]) if M[g].kind == "d" else rbv[0] + M[g].idx_in_ps)
    return out


# ---- 1. rows ---------------------------------------------------------------------------------------------------------------------------------------
_coverage = {}


@pytest.mark.parametrize("name", fr.FIXTURES)
def test_rows_on_the_fixtures(name):
    from stark_amd import capi

    eng, c, tables = installed(name)
    v1, rbv, rbw = dof_rows(c)
    lib = host_lib()
    stick, slide = set(), set()
    for s in range(3):
        cs, ri, rd, contrib = restated(c, tables, name, s)
        eng.set_dofs(cs["u"])
        rep = eng.friction_report()
        assert rep["ints"].shape == ri.shape and (rep["ints"] == ri).all(), (name, s)  # the sliding flag among them, on every row
        assert (rep["bounds"] == fr.bounds_of(ri)).all()
        sliding = (ri[:, 7] & fr.SLIDING) != 0
        stick |= set(int(t) for t in ri[~sliding, 0])
        slide |= set(int(t) for t in ri[sliding, 0])
        # rows line up with contact_get_table and contact_friction_data row for row
        for t, tname in enumerate(fr.TABLE_NAMES):
            lo, hi = rep["bounds"][t], rep["bounds"][t + 1]
            assert hi - lo == (len(tables[tname]["conn"]) if tname in tables else 0)
            if hi > lo:
                assert (rep["row"][lo:hi] == np.arange(hi - lo)).all() and (tables[tname]["conn"][:, 0] == np.arange(hi - lo)).all()
                assert np.array_equal(rep["mu"][lo:hi], tables[tname]["mu"]) and np.array_equal(rep["fn"][lo:hi], tables[tname]["fn"])
        # the header's host build on the same inputs
        ch = dict(ri=ri, st=cs["st"], dt=cs["dt"], scene=cs["scene"], tables=tables, contrib=contrib)
        meta, vel, T, mu, fn, bary, _ = cpu.gathered_inputs(ch, lib)
        n = len(ri)
        hi_, hd, hw = np.zeros((n, 8), dtype=np.int32), np.zeros((n, 24)), np.zeros((n, 5))
        lib.host_friction_rows(meta.ctypes.data, vel.ctypes.data, T.ctypes.data, mu.ctypes.data, fn.ctypes.data, bary.ctypes.data, cs["dt"], cs["epsv"], n, hi_.ctypes.data,
                               hd.ctypes.data, hw.ctypes.data)
        assert (rep["ints"] == hi_).all()
        err = np.abs(rep["doubles"] - hd) / fr.field_scales(ri, hd, fr.state_vmax(cs["st"]), cs["dt"])
        # energies and node forces against the engine's own evaluation
        eng.eval(capi.EVAL_P)
        worst_E = worst_f = 0.0
        for t, tname in enumerate(fr.TABLE_NAMES):
            lo, hi = rep["bounds"][t], rep["bounds"][t + 1]
            if hi == lo:
                continue
            pid = eng.potential_id(tname)
            E = eng.element_energies(pid, hi - lo)
            worst_E = max(worst_E, (np.abs(rep["E"][lo:hi] - E) / np.abs(E)).max())
            f, rows = eng.element_forces(pid, 1.0 / cs["dt"])
            for k in range(lo, hi):
                mufn, ft = rep["mu"][k] * rep["fn"][k], rep["ft"][k]
                want = {}
                for row, (cv, w) in zip(node_rows(c, contrib[k], v1, rbv), contrib[k]):
                    want[row] = want.get(row, np.zeros(3)) + w * ft
                got = {}
                for blk in range(rows.shape[1]):
                    row = int(rows[k - lo, blk])
                    if rbw is not None and rbw[0] <= row < rbw[0] + rbw[1]:
                        continue  # (torques are not compared: dE/dw goes through the normalised quaternion and is not r x ft)
                    got[row] = got.get(row, np.zeros(3)) + f[k - lo, blk]
                assert set(got) == set(want), (tname, k)
                for row in got:
                    worst_f = max(worst_f, np.abs(got[row] - want[row]).max() / mufn)
        print("%s state %d: %d rows (%d sliding), worst field error %.3g of scale against the header, worst energy error %.3g, worst node force deviation %.3g mu fn"
              % (name, s, n, sliding.sum(), err.max(), worst_E, worst_f))
        assert (err <= 1e-12).all() and worst_E <= 1e-11 and worst_f <= 1e-11
    assert eng.counter("friction_reports") == 3
    _coverage[name] = (stick, slide)
    eng.close()


def test_rows_cover_both_branches_of_every_table():
    """Over the fifteen states every one of the 14 tables has a sticking and a sliding row (a changed fixture cannot silently drop a branch)."""
    stick, slide = set(), set()
    for name in fr.FIXTURES:
        for s in range(3):
            ri = fr.fixture_case(name, s)["ri"]
            sliding = (ri[:, 7] & fr.SLIDING) != 0
            stick |= set(int(t) for t in ri[~sliding, 0])
            slide |= set(int(t) for t in ri[sliding, 0])
    assert stick == slide == set(range(21, 35))
    for name, (st, sl) in _coverage.items():  # (what the device rows of this session showed is part of it)
        assert st <= stick and sl <= slide


# ---- 2. vertex and pair records --------------------------------------------------------------------------------------------------------------------
def check_vertices(scene, rep, vrep, contrib, X):
    """From the device's own rows: counts and maxima exact, the vector sum within the summation bound of its terms."""
    ri, rd = rep["ints"], rep["doubles"]
    want, terms = fr.vertex_report(scene, ri, rd, contrib, X)
    rec = vrep["records"]
    assert np.array_equal(rec[:, 0], want[:, 0]) and np.array_equal(rec[:, 1], want[:, 1]) and np.array_equal(rec[:, 5], want[:, 5])
    worst = 0.0
    for v, vs in enumerate(terms):
        b = fr.vector_sum_bound(vs)
        d = np.abs(rec[v, 2:5] - fr.fsum3(vs))
        assert (d <= b).all(), v
        if b > 0.0:
            worst = max(worst, d.max() / b)
    L = fr.Layout(scene)
    inc = np.zeros(L.n_v)
    np.add.at(inc, L.tri.reshape(-1), 1)
    assert (np.abs(rec[:, 6] - want[:, 6]) <= (inc + 8) * 8 * U * want[:, 6]).all()
    assert (rec[inc == 0, 6] == 0.0).all() and (rec[inc == 0, 7] == 0.0).all()
    norm = np.linalg.norm(rec[:, 2:5], axis=1)
    with np.errstate(divide="ignore", invalid="ignore"):
        traction = np.where(rec[:, 6] > 0.0, norm / rec[:, 6], 0.0)
    assert (np.abs(rec[:, 7] - traction) <= 8 * U * traction).all()
    assert (vrep["group"] == L.cv_mesh).all() and (vrep["source_index"] == L.cv_src).all()
    return worst


def check_pairs(scene, rep, pairs):
    ri, rd = rep["ints"], rep["doubles"]
    want, terms = fr.pair_report(scene, ri, rd)
    assert np.array_equal(pairs[:, :, :2], want[:, :, :2]) and np.array_equal(pairs[:, :, 10], want[:, :, 10])  # counts and the largest slip speed exact
    worst = 0.0
    for (ga, gb), T in terms.items():
        vec = [np.array([T[4][i], T[5][i], T[6][i]]) for i in range(len(T[4]))]
        for f, xs in T.items():
            b = fr.vector_sum_bound(vec) if f in (4, 5, 6) else fr.sum_bound(xs)
            d = abs(pairs[ga, gb, f] - math.fsum(xs))
            assert d <= b, (ga, gb, f)
            if b > 0.0:
                worst = max(worst, d / b)
    with np.errstate(divide="ignore", invalid="ignore"):
        assert np.array_equal(pairs[:, :, 11], np.where(pairs[:, :, 3] != 0.0, pairs[:, :, 7] / pairs[:, :, 3], 0.0))  # the same bits
    assert (pairs[:, :, 11] <= 1.0 + 1e-12).all()
    G = len(scene.meshes)
    assert (pairs[np.tril_indices(G, -1)] == 0.0).all()
    return worst


@pytest.mark.parametrize("name", fr.FIXTURES)
def test_vertex_and_pair_records(name):
    eng, c, tables = installed(name)
    v1, rbv, rbw = dof_rows(c)
    pots = [eng.potential_id(t) for t in fr.TABLE_NAMES]
    L = fr.Layout(c["scene"])
    worst_v = worst_p = worst_r = 0.0
    for s in range(3):
        cs, ri, rd, contrib = restated(c, tables, name, s)
        eng.set_dofs(cs["u"])
        rep = eng.friction_report()
        assert (rep["ints"] == ri).all()
        # the device's own weights: A [1] or [1 - s, s] from rd[17], B rd[18:21] — the restatement's bits (the CPU test pins them)
        for k, row in enumerate(contrib):
            na = 2 if ri[k, 2] == 3 else 1
            wa = [1.0] if na == 1 else [1.0 - rep["param_a"][k], rep["param_a"][k]]
            assert [w for _, w in row] == wa + [-x for x in rep["weights_b"][k][:len(row) - na]]
        vrep = eng.friction_vertex_report()
        pairs = eng.friction_pair_report()
        worst_v = max(worst_v, check_vertices(cs["scene"], rep, vrep, contrib, cs["X"]))
        worst_p = max(worst_p, check_pairs(cs["scene"], rep, pairs))
        # a deformable group's pair vectors against forces_resultant of the 14 friction potentials over the group's rows. The bound is the summation
        # bound of the sum the readout forms: its terms are the node forces w ft on the group's nodes, of every row the group takes part in (both sides
        # of the rows of its own pair, which cancel in the pair vectors' sum), |term| the vector's magnitude |w| |ft|
        elem = {}
        for t, tn in enumerate(fr.TABLE_NAMES):
            if rep["bounds"][t + 1] > rep["bounds"][t]:
                elem[t] = eng.element_forces(eng.potential_id(tn), 1.0 / cs["dt"])
        for g, m in enumerate(cs["scene"].meshes):
            if m.kind != "d":
                continue
            rows = v1[0] + np.unique(m.verts)
            got = eng.forces_resultant(pots, 1.0 / cs["dt"], rows)[:3]
            want = np.zeros(3)
            for h in range(len(cs["scene"].meshes)):
                if h != g:
                    want += (1.0 if g < h else -1.0) * pairs[min(g, h), max(g, h), 4:7]
            node_terms = [w * rep["ft"][k] for k, row in enumerate(contrib) for cv, w in row if int(L.cv_mesh[cv]) == g and w != 0.0]
            if not node_terms:
                assert (got == 0.0).all() and (want == 0.0).all()
                continue
            bound = fr.vector_sum_bound(node_terms)
            ratio = np.abs(got - want) / bound
            own = [[], [], []]
            rowset = set(int(r) for r in rows)
            for t, (f, brow) in elem.items():
                for e in range(len(f)):
                    for blk in range(brow.shape[1]):
                        if int(brow[e, blk]) in rowset:
                            for k in range(3):
                                own[k].append(f[e, blk, k])
            exact_own = np.array([math.fsum(own[k]) for k in range(3)])
            own_bound = np.array([fr.sum_bound(own[k]) for k in range(3)])
            print("%s state %d group %d: %d node terms, |resultant - pair vectors| %s, bound %.3g, ratio %s; |resultant - fsum of its %d element forces| %s, bound %s"
                  % (name, s, g, len(node_terms), np.abs(got - want), bound, ratio, len(own[0]), np.abs(got - exact_own), own_bound))
            assert (np.abs(got - exact_own) <= own_bound).all(), g
            worst_r = max(worst_r, ratio.max())
    print("%s: worst |difference| / bound: vertex sums %.3g, pair sums %.3g, pair vectors against forces_resultant %.3g" % (name, worst_v, worst_p, worst_r))
    assert worst_r <= 1.0, worst_r
    eng.close()


# ---- 3. the wavefront path -------------------------------------------------------------------------------------------------------------------------
def rod_scene(k, n_thickness=2):
    """A rod of k points (group 0) at half of dhat above the interior of one large triangle (group 1); both deformable, in one point set; mu = 0.5.
    The points move sideways at speeds that straddle epsv, so rows stick and slide."""
    import stark_amd

    thick = 0.01
    rod = np.array([[0.1 + 0.005 * i, 0.1, thick] for i in range(k)])
    big = np.array([[-1.0, -1.0, 0.0], [3.0, -1.0, 0.0], [-1.0, 3.0, 0.0]])
    x0 = np.ascontiguousarray(np.concatenate([rod, big]))
    v1 = np.zeros_like(x0)
    v1[:k, 0] = 2e-5 * np.arange(k) * (np.arange(k) % 3 - 0.5)
    v1[:k, 1] = 3e-4
    eng = stark_amd.Engine(0)
    eng.add_dof_set("v1", v1)
    X = x0.copy()
    dt, kk, th, epsv = np.array([0.01]), np.array([1e6]), np.full(n_thickness, thick), np.array([1e-3])
    eng.contact_init(v1=eng.array(v1, 3), x0=eng.array(x0, 3), X=eng.array(X, 3), dt=eng.array(dt, 1), k=eng.array(kk, 1), thickness=eng.array(th, 1), epsv=eng.array(epsv, 1))
    edges = np.array([[i, i + 1] for i in range(k - 1)], dtype=np.int32)
    big_tris, big_edges = np.array([[0, 1, 2]]), np.array([[0, 1], [0, 2], [1, 2]])
    eng.contact_add_mesh("d", 0, np.arange(k), np.zeros((0, 3), dtype=np.int32), edges)
    eng.contact_add_mesh("d", 0, k + np.arange(3), big_tris, big_edges)
    eng.contact_disable_collision(0, 0)
    eng.contact_set_friction(0, 1, 0.5)
    scene = oc.ContactScene([oc.Mesh("d", 0, np.arange(k), np.zeros((0, 3), dtype=np.int64), edges.astype(np.int64), thick),
                             oc.Mesh("d", 0, k + np.arange(3), big_tris.astype(np.int64), big_edges.astype(np.int64), thick)])
    st = dict(v1=v1, x0=x0)
    return eng, scene, st, x0


@pytest.mark.parametrize("k", [64, 65, 200])
def test_long_incidence_lists_take_the_wavefront_path(k):
    """Every point is within dhat of the triangle: k rows of friction_d_d_pt, every vertex of the triangle carries k contributions. A run of 64 is summed by
    one lane, longer ones by a wavefront."""
    eng, scene, st, X = rod_scene(k)
    assert eng.counter("friction_report_long_rows") == 0
    assert eng.contact_update_friction() == k
    tables = engine_tables(eng)
    assert list(tables) == ["friction_d_d_pt_C0"]
    ri, rd, contrib = fr.rows(scene, tables, st, 0.01, 1e-3)
    rep = eng.friction_report()
    assert (rep["ints"] == ri).all() and (rep["kind"] == 2).all() and (rep["group_a"] == 0).all() and (rep["group_b"] == 1).all()
    n_sliding = int(((rep["flags"] & fr.SLIDING) != 0).sum())
    assert 0 < n_sliding < k
    err = np.abs(rep["doubles"] - rd) / fr.field_scales(ri, rd, fr.state_vmax(st), 0.01)
    assert (err <= 1e-12).all()
    for j, row in enumerate(contrib):
        assert [w for _, w in row] == [1.0] + [-x for x in rep["weights_b"][j]]
    vrep = eng.friction_vertex_report()
    assert eng.counter("friction_report_long_rows") == (0 if k <= 64 else 3)
    rec = vrep["records"]
    assert (rec[k:, 0] == k).all() and (rec[:k, 0] == 1).all() and (rec[k:, 1] == n_sliding).all()
    worst = check_vertices(scene, rep, vrep, contrib, X)
    for j, row in enumerate(contrib):  # a rod point carries its row's whole ft (weight exactly 1)
        assert np.array_equal(rec[row[0][0], 2:5], rep["ft"][j])
    area = 0.5 * 4.0 * 4.0 / 3.0
    assert np.abs(rec[k:, 6] - area).max() <= 64 * U * area and (rec[:k, 6] == 0.0).all()
    pairs = eng.friction_pair_report()
    worst_p = check_pairs(scene, rep, pairs)
    assert pairs[0, 1, 0] == k and pairs[0, 0, 0] == 0 and pairs[1, 1, 0] == 0 and pairs[0, 1, 1] == n_sliding
    # the triangle takes what the rod gives: its three vertex forces add up to minus the pair vector (the force on group 0)
    tri_terms = [w * rep["ft"][j] for j, row in enumerate(contrib) for cv, w in row[1:]]
    assert (np.abs(rec[k:, 2:5].sum(axis=0) + pairs[0, 1, 4:7]) <= 2.0 * fr.vector_sum_bound(tri_terms) + 16 * U * np.abs(pairs[0, 1, 4:7]).max()).all()
    print("k = %d: %d sliding rows, worst |difference| / bound: vertex sums %.3g, pair sums %.3g" % (k, n_sliding, worst, worst_p))
    eng.close()


# ---- 4. reproducibility, non-interference, the report's own keys -----------------------------------------------------------------------------------
def all_reports(eng):
    r, v, p = eng.friction_report(), eng.friction_vertex_report(), eng.friction_pair_report()
    return [r["ints"], r["doubles"], v["records"], v["group"], v["source_index"], p]


def test_two_reports_of_one_state_are_bit_identical_and_survive_barrier_searches():
    """The friction search's key buffers are overwritten by every barrier search; the report reads a copy of its own."""
    eng, c = tcr.build("contactmix_t0")
    eng.contact_update_friction()
    eng.set_dofs(fr.fixture_case("contactmix_t0", 1)["u"])
    first = all_reports(eng)  # (no barrier search has run yet)
    assert len(first[0]) == cpu.ROWS["contactmix_t0"]
    assert tcr.same_bits(first, all_reports(eng))
    searches = eng.counter("contact_searches")
    eng.contact_update(c["dt"])
    assert tcr.same_bits(first, all_reports(eng))
    eng.contact_set_broad_phase(True)
    eng.contact_update(0.5 * c["dt"])
    eng.contact_count_intersections(c["dt"])
    assert eng.counter("contact_searches") == searches + 2
    assert tcr.same_bits(first, all_reports(eng))
    eng.close()


def test_reports_between_the_stages_change_nothing():
    from stark_amd import capi

    def sequence(report):
        eng, c = tcr.build("contactmix_t0")
        if report:
            all_reports(eng)  # (before the first friction update)
        eng.contact_update_friction()
        if report:
            all_reports(eng)
        eng.contact_update(c["dt"])
        if report:
            all_reports(eng)
        E, grad = eng.eval(capi.EVAL_P_G_H)
        if report:
            all_reports(eng)
        tables = [eng.contact_table(t) for t in tcr.cr.TABLE_NAMES + fr.TABLE_NAMES]
        data = [eng.contact_friction_data(t, len(eng.contact_table(t))) for t in fr.TABLE_NAMES]
        contact = tcr.all_reports(eng)
        eng.assemble()
        if report:
            all_reports(eng)
        bsr = eng.get_bsr()
        x, info = eng.pcg(c["man"]["pcg"]["abs_tol"])
        assert eng.counter("friction_reports") == (14 if report else 0)  # (five times three; the row report of an empty key list launches nothing)
        eng.close()
        return E, grad, bsr, x, info.n_iterations, tables, data, contact

    E0, g0, (rp0, c0, v0), x0, it0, t0, d0, cr0 = sequence(False)
    E1, g1, (rp1, c1, v1), x1, it1, t1, d1, cr1 = sequence(True)
    assert E0 == E1 and np.array_equal(g0, g1)
    assert np.array_equal(rp0, rp1) and np.array_equal(c0, c1) and np.array_equal(v0, v1)
    assert it0 == it1 and np.array_equal(x0, x1)
    assert all(np.array_equal(a, b) for a, b in zip(t0, t1))
    assert all(set(a) == set(b) and all(np.array_equal(a[k], b[k]) for k in a) for a, b in zip(d0, d1))
    assert tcr.same_bits(cr0, cr1)


# ---- 5. refusals and empties -----------------------------------------------------------------------------------------------------------------------
def test_refusals_name_their_cause():
    import stark_amd
    from stark_amd import capi

    L = capi.lib()
    group = L.mistark_local_group_create(2)
    try:
        eng = stark_amd.Engine(0)
        eng.dist_init_local(group, 0)
        eng.add_dof_set("u", np.zeros(6))
        for call in (eng.friction_report, eng.friction_vertex_report, eng.friction_pair_report):
            with pytest.raises(stark_amd.engine.EngineError, match="single-rank"):
                call()
        eng.close()
    finally:
        L.mistark_local_group_destroy(group)
    h = C.c_void_p()
    assert L.mistark_create_dry(C.byref(h)) == 0
    try:
        n, g = C.c_int64(), C.c_int32()
        for rc in (L.mistark_contact_friction_report(h, None, None, C.byref(n)), L.mistark_contact_friction_vertex_report(h, None, None, None, C.byref(n)),
                   L.mistark_contact_friction_pair_report(h, None, C.byref(g))):
            assert rc < 0 and "registration-only" in L.mistark_last_error(h).decode()
    finally:
        L.mistark_destroy(h)
    eng = stark_amd.Engine(0)
    eng.add_dof_set("u", np.zeros(6))
    for call in (eng.friction_report, eng.friction_vertex_report, eng.friction_pair_report):
        with pytest.raises(stark_amd.engine.EngineError, match="mistark_contact_init"):
            call()
    assert eng.counter("friction_reports") == 0
    eng.close()


def check_empty(eng, scene):
    L = fr.Layout(scene)
    rep, vrep, pairs = eng.friction_report(), eng.friction_vertex_report(), eng.friction_pair_report()
    assert rep["ints"].shape == (0, 8) and rep["doubles"].shape == (0, 24) and (rep["bounds"] == 0).all()
    assert vrep["records"].shape == (L.n_v, 8) and (vrep["records"] == 0.0).all()
    assert (vrep["group"] == L.cv_mesh).all() and (vrep["source_index"] == L.cv_src).all()
    G = len(scene.meshes)
    assert pairs.shape == (G, G, 12) and (pairs == 0.0).all()


def sizes(eng):
    n, nv, g = C.c_int64(-1), C.c_int64(-1), C.c_int32(-1)
    assert eng.L.mistark_contact_friction_report(eng.h, None, None, C.byref(n)) == 0
    assert eng.L.mistark_contact_friction_vertex_report(eng.h, None, None, None, C.byref(nv)) == 0
    assert eng.L.mistark_contact_friction_pair_report(eng.h, None, C.byref(g)) == 0
    return n.value, nv.value, g.value


def test_empties_and_size_queries():
    name = "contactmix_t0"
    eng, c = tcr.build(name)
    scene = c["scene"]
    L = fr.Layout(scene)
    G = len(scene.meshes)
    # before the first friction update
    assert sizes(eng) == (0, L.n_v, G) and eng.counter("friction_reports") == 0
    check_empty(eng, scene)
    assert eng.counter("contact_searches") == 0
    launched = eng.counter("friction_reports")
    # installed: the size queries answer from host counts and launch nothing
    assert eng.contact_update_friction() == cpu.ROWS[name]
    assert sizes(eng) == (cpu.ROWS[name], L.n_v, G) and eng.counter("friction_reports") == launched
    assert len(eng.friction_report()["ints"]) == cpu.ROWS[name] and eng.counter("friction_reports") == launched + 1
    eng.close()
    # a change of the mesh set: zero rows until the next friction update (a scene with a spare thickness value for the group that is added)
    k = 8
    eng, scene, st, X = rod_scene(k, n_thickness=3)
    assert eng.contact_update_friction() == k and sizes(eng) == (k, k + 3, 2)
    assert len(eng.friction_report()["ints"]) == k
    eng.contact_add_mesh("d", 0, k + np.arange(3), np.array([[0, 1, 2]]), np.array([[0, 1], [0, 2], [1, 2]]))  # the large triangle once more
    for g in range(3):
        eng.contact_disable_collision(g, 2)  # (it shares its vertices with group 1: it collides with nothing)
    assert sizes(eng) == (0, k + 6, 3)
    rep, pairs = eng.friction_report(), eng.friction_pair_report()
    assert rep["ints"].shape == (0, 8) and pairs.shape == (3, 3, 12) and (pairs == 0.0).all()
    vrep = eng.friction_vertex_report()
    assert vrep["records"].shape == (k + 6, 8) and (vrep["records"] == 0.0).all() and list(vrep["group"][-3:]) == [2, 2, 2]
    assert eng.contact_update_friction() == k
    rep = eng.friction_report()
    assert len(rep["ints"]) == sizes(eng)[0] == k and (rep["group_b"] == 1).all()
    assert eng.friction_pair_report()[0, 1, 0] == k
    eng.close()


def test_no_rows_without_friction():
    """Friction off (no coefficient set) and every coefficient zero: the friction search routes no row."""
    import copy

    name = "contactrods_t0"
    for zero in (False, True):
        c = tcr.cr.fixture_case(name)
        scene = copy.copy(c["scene"])
        saved = dict(c["scene"].friction)
        try:
            c["scene"].friction.clear()  # (build() reads the scene's coefficients; the cached case is put back below)
            eng, _ = tcr.build(name)
        finally:
            c["scene"].friction.update(saved)
        if zero:
            for (a, b) in saved:
                eng.contact_set_friction(a, b, 0.0)
        assert eng.contact_update_friction() == 0
        eng.contact_update(c["dt"])
        check_empty(eng, scene)
        eng.close()


# ---- 6. host mirror --------------------------------------------------------------------------------------------------------------------------------
def _counter(sim, name):
    from stark_amd import capi

    v = C.c_int64()
    assert capi.lib().mistark_get_counter(sim.engine_handle(), name.encode(), C.byref(v)) == 0
    return v.value


def block_on_box(record):
    """The scene of test_recording_does_not_change_a_trajectory_with_friction (tests/test_gpu_contact_report.py): a soft block on a fixed rigid box,
    mu = 0.5, the block given a sideways velocity."""
    from stark_amd import sim as S

    st = S.default_settings()
    st.max_time_step_size = 0.01
    st.init_frictional_contact = 1
    sim = S.Simulation(st)
    gp = S.contact_global_params()
    gp.default_contact_thickness = 1e-3
    sim.set_contact_global_params(gp)
    block = sim.add_volume_grid("block", (0.0, 0.0, 0.05 + 1.5e-3), (0.12, 0.12, 0.1), (6, 6, 5), S.soft_rubber())
    box = sim.add_rigid_box("box", 1.0, (0.5, 0.5, 0.05))
    sim.rb_add_translation(box, (0.0, 0.0, -0.025))
    sim.rb_add_constraint("fix", box)
    sim.set_friction(sim.contact_group("d", block), sim.contact_group("rb", box), 0.5)
    v = sim.points("v0")
    v[:, 0] = 0.2
    sim.set_points("v0", v)
    if record:
        sim.record_friction(True)
    return sim, box


def facade(sim):
    import stark_amd
    from stark_amd import capi

    eng = stark_amd.Engine.__new__(stark_amd.Engine)  # the simulation's own engine context through the facade (not owned: never closed here)
    eng.L, eng.h = capi.lib(), sim.engine_handle()
    return eng


def test_host_mirror():
    from stark_amd import sim as S

    N = 3

    def run(record):
        sim, box = block_on_box(record)
        counts, reps = [], []
        for _ in range(N):
            assert sim.run_one_step()
            i = sim.info()
            counts.append((i.total_newton_iterations, i.total_linear_solves, i.total_cg_iterations))
            if record:
                rep = sim.friction()
                assert abs(rep["time"] - sim.info().current_time) < 1e-12 and rep["labels"] == ["block", "box"]
                vb = sim.points("v0").mean(axis=0) - sim.rb_state(box)[2]  # the block's mean velocity relative to the box
                reps.append((rep, vb))
        eng = facade(sim)
        try:
            u = eng.get_dofs()  # the converged DoFs of the last step
        finally:
            eng.h = None
        info = sim.contact_info()
        out = sim.points("x0"), sim.points("v0"), counts, info["n_friction_contacts"], _counter(sim, "friction_reports"), reps, u
        if not record:
            with pytest.raises(S.SimError, match="recording is off"):
                sim.friction()
        sim.close()
        return out

    x_off, v_off, c_off, f_off, r_off, _, u_off = run(False)
    x_on, v_on, c_on, f_on, r_on, reps, u_on = run(True)
    assert r_off == 0 and r_on == N and f_on == f_off > 0
    assert c_on == c_off and np.array_equal(x_on, x_off) and np.array_equal(v_on, v_off) and np.array_equal(u_on, u_off)
    n_slid = 0
    for rep, vb in reps:
        rows, pairs = rep["rows"], rep["pairs"]
        assert len(rows["ints"]) > 0 and pairs[0, 1, 0] == len(rows["ints"])
        assert pairs[0, 1, 11] <= 1.0 + 1e-12 and (rows["mobilised"] <= 1.0).all()
        if pairs[0, 1, 1] > 0:  # while rows slide, friction on the block (group 0, the lower one) opposes its motion over the box
            n_slid += 1
            assert float(pairs[0, 1, 4:7] @ vb) < 0.0
        assert pairs[0, 1, 8] >= 0.0
    assert n_slid > 0
    # The report of step N against a direct report of the same state, bit for bit: a second, identical simulation is taken to the start of step N (its
    # x0, rigid-body state and, after begin_time_step, its friction tables are then what step N of the first one saw), its DoFs are set to what step N
    # converged to, and the three accessors are called.
    sim, box = block_on_box(False)
    for _ in range(N - 1):
        assert sim.run_one_step()
    sim.begin_time_step()
    eng = facade(sim)
    try:
        assert eng.ndofs == u_on.size
        eng.set_dofs(u_on)
        direct = all_reports(eng)
        assert eng.counter("friction_reports") == 3
    finally:
        eng.h = None
    rec = reps[-1][0]
    mirror = [rec["rows"]["ints"], rec["rows"]["doubles"], rec["vertices"]["records"], rec["vertices"]["group"], rec["vertices"]["source_index"], rec["pairs"]]
    assert tcr.same_bits(direct, mirror)
    sim.close()
    sim, box = block_on_box(True)
    with pytest.raises(S.SimError, match="no time step has been accepted"):
        sim.friction()
    sim.record_friction(False)
    with pytest.raises(S.SimError, match="recording is off"):
        sim.friction()
    sim.close()
