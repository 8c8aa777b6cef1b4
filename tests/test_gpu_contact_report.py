"""GPU tests of the contact report (include/mistark_contact.h "contact report", stark_amd/csrc/contact_report.hip) on the contact fixtures, against the
numpy restatement of tests/contact_report_ref.py and against the engine's own evaluation and force readout.

Tolerances: ints, flags, counts and minima exact; row doubles 1e-12 of the field's scale (device FMA contraction may differ from numpy; the CPU test pins
the header's bits); energies 1e-11 of the table's largest |E| and forces 1e-11 fn (the project's element tolerance); a sum of n terms (n + 8) * 2^-53 *
sum |terms| against math.fsum of the same terms."""
import ctypes as C
import math
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import contact_report_ref as cr  # noqa: E402
from oracle import contact as oc  # noqa: E402

pytestmark = pytest.mark.gpu
FIXTURES = ["contactmix_t0", "contactmix_t1", "contactcorners_t0", "contactrods_t0", "contactrods_t1"]
U = cr.U


def build(name):
    """The build() of tests/test_gpu_contact.py: the fixture's non-contact potentials registered from the fixture, the 35 contact / friction potentials
    by the device contact module, collision meshes from the fixture's detector inputs."""
    import copy

    from gpu_util import engine_from_problem

    c = cr.fixture_case(name)
    prob, man = c["prob"], c["man"]
    base = copy.copy(prob)
    base.potentials = [copy.copy(p) for p in prob.potentials]
    for p in base.potentials:
        if p.name.startswith("contact_") or p.name.startswith("friction_"):
            p.conn = p.conn[:0]
    eng = engine_from_problem(base, man)
    from contact_util import roles_from_manifest

    ids = {}
    for role, aid in roles_from_manifest(man).items():
        stride = {"rb_q0": 4}.get(role, 3 if role in ("v1", "x0", "X", "rb_xloc", "rb_v1", "rb_w1", "rb_t0") else 1)
        key = (aid, stride)
        if key not in eng.array_ids:
            eng.array_ids[key] = eng.array(eng.host_arrays[aid].reshape(-1, stride), stride)
        ids["thickness" if role == "thick" else role] = eng.array_ids[key]
    eng.contact_init(**ids)
    for m in c["scene"].meshes:
        eng.contact_add_mesh(m.kind, m.idx_in_ps, m.verts, m.tris, m.edges)
    for (a, b), mu in c["scene"].friction.items():
        eng.contact_set_friction(a, b, mu)
    return eng, c


def installed(name):
    eng, c = build(name)
    eng.contact_update_friction()
    assert eng.contact_update(c["dt"]) == len(c["keys"])
    return eng, c


def dof_row0(c, role):
    """First block row of the DoF set behind a state array (v1, rb_v1, rb_w1), or None."""
    from contact_util import roles_from_manifest

    aid = roles_from_manifest(c["man"]).get(role)
    for s, a in c["prob"].dof_arrays.items():
        if a == aid:
            return c["prob"].dof_offsets[s] // 3, c["prob"].dof_sizes[s] // 3
    return None


def check_rows(rep, ri, rd, xmax, k, what):
    assert rep["ints"].shape == ri.shape and (rep["ints"] == ri).all(), what
    err = np.abs(rep["doubles"] - rd) / cr.field_scales(rd, xmax, k)
    print("%s: %d rows, worst field error %.3g of scale" % (what, len(ri), err.max() if err.size else 0.0))
    assert (err <= 1e-12).all(), what


# ---- 1. rows ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", FIXTURES)
def test_rows_on_the_fixtures(name):
    eng, c = installed(name)
    rep = eng.contact_report()
    check_rows(rep, c["ri"], c["rd"], np.abs(c["X"]).max(), c["k"], name)
    assert (rep["bounds"] == cr.bounds_of(c["ri"])).all()
    for t, tname in enumerate(cr.TABLE_NAMES):
        table = eng.contact_table(tname)
        lo, hi = rep["bounds"][t], rep["bounds"][t + 1]
        assert len(table) == hi - lo, tname
        for n in range(lo, hi):
            assert list(table[n - lo]) == cr.table_row(c["scene"], c["keys"][n]), (tname, n)
    assert eng.counter("contact_reports") == 1
    eng.close()


# ---- 2. energies and forces ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", FIXTURES)
def test_energies_and_forces_against_the_engine(name):
    from stark_amd import capi

    eng, c = installed(name)
    L = cr.Layout(c["scene"])
    M = c["scene"].meshes
    rep = eng.contact_report()
    ri, rd = rep["ints"], rep["doubles"]
    contrib = cr.contributions(c["scene"], ri, rd)
    eng.eval(capi.EVAL_P)
    v1, rbv = dof_row0(c, "v1"), dof_row0(c, "rb_v1")
    worst_E = worst_f = 0.0
    n_forces = 0
    for t, tname in enumerate(cr.TABLE_NAMES):
        lo, hi = rep["bounds"][t], rep["bounds"][t + 1]
        if hi == lo:
            continue
        pid = eng.potential_id(tname)
        E = eng.element_energies(pid, hi - lo)
        worst_E = max(worst_E, np.abs(rd[lo:hi, 13] - E).max() / np.abs(E).max())
        f, rows = eng.element_forces(pid, 1.0 / c["dt"])
        for n in range(lo, hi):
            if ri[n, 7] & cr.MOLLIFIED:
                continue
            fn, nrm = rd[n, 12], rd[n, 8:11]
            want = {}
            for j, (cv, w) in enumerate(contrib[n]):
                a_side = j < (1 if ri[n, 1] == 0 else 2)
                g = int(L.cv_mesh[cv])
                row = v1[0] + int(L.cv_src[cv]) if M[g].kind == "d" else rbv[0] + M[g].idx_in_ps  # (a body's linear block takes its side's node forces)
                want[row] = want.get(row, np.zeros(3)) + (1.0 if a_side else -1.0) * w * fn * nrm
            got = {}
            for blk in range(rows.shape[1]):
                row = int(rows[n - lo, blk])
                in_v1 = v1 is not None and v1[0] <= row < v1[0] + v1[1]
                in_rbv = rbv is not None and rbv[0] <= row < rbv[0] + rbv[1]
                if in_v1 or in_rbv:  # (the torque blocks are not compared: the quaternion update is not a pure r x f)
                    got[row] = got.get(row, np.zeros(3)) + f[n - lo, blk]
            for row in set(got) | set(want):  # (nodes of the primitives outside the feature carry weight 0 and are no block of the element)
                worst_f = max(worst_f, np.abs(got.get(row, np.zeros(3)) - want.get(row, np.zeros(3))).max() / fn)
            n_forces += 1
    print("%s: worst energy error %.3g of the table's largest |E|, worst force deviation %.3g fn over %d rows" % (name, worst_E, worst_f, n_forces))
    assert worst_E <= 1e-11 and worst_f <= 1e-11 and n_forces > 0
    eng.close()


# ---- 3. vertex report ------------------------------------------------------------------------------------------------------------------------------
def check_vertices(c, rep, vrep, X):
    want, terms = cr.vertex_report(c["scene"], rep["ints"], rep["doubles"], X)  # (from the device's own rows: gap and count are then exact)
    rec = vrep["records"]
    assert np.array_equal(rec[:, 0], want[:, 0]) and np.array_equal(rec[:, 1], want[:, 1])
    for v, xs in enumerate(terms):
        assert abs(rec[v, 2] - math.fsum(xs)) <= cr.sum_bound(xs), v
    L = cr.Layout(c["scene"])
    ta = cr.triangle_areas(c["scene"], X)
    inc = np.zeros(L.n_v)
    np.add.at(inc, L.tri.reshape(-1), 1)
    assert (np.abs(rec[:, 3] - want[:, 3]) <= (inc + 8) * 8 * U * want[:, 3]).all()
    assert (rec[inc == 0, 3] == 0.0).all()
    with np.errstate(divide="ignore", invalid="ignore"):
        assert np.array_equal(rec[:, 4], np.where(rec[:, 3] > 0.0, rec[:, 2] / rec[:, 3], 0.0))  # the same bits
    assert (vrep["group"] == L.cv_mesh).all() and (vrep["source_index"] == L.cv_src).all()


@pytest.mark.parametrize("name", FIXTURES)
def test_vertex_report(name):
    eng, c = installed(name)
    check_vertices(c, eng.contact_report(), eng.contact_vertex_report(), c["X"])
    eng.close()


# ---- 4. long rows ----------------------------------------------------------------------------------------------------------------------------------
def patch_scene(z):
    """A 12 x 12 grid patch (group 0) parallel over the interior of one large triangle (group 1) at height z; both deformable, in one point set."""
    import stark_amd

    n, h, thick = 12, 0.05, 0.01
    patch = np.array([[0.1 + h * i, 0.1 + h * j, z] for j in range(n) for i in range(n)])
    big = np.array([[-1.0, -1.0, 0.0], [3.0, -1.0, 0.0], [-1.0, 3.0, 0.0]])
    x0 = np.ascontiguousarray(np.concatenate([patch, big]))
    tris = np.array([[j * n + i, j * n + i + 1, (j + 1) * n + i + 1] for j in range(n - 1) for i in range(n - 1)] +
                    [[j * n + i, (j + 1) * n + i + 1, (j + 1) * n + i] for j in range(n - 1) for i in range(n - 1)], dtype=np.int32)
    edges = np.array(sorted({(min(t[k], t[(k + 1) % 3]), max(t[k], t[(k + 1) % 3])) for t in tris for k in range(3)}), dtype=np.int32)
    eng = stark_amd.Engine(0)
    v1 = np.zeros_like(x0)
    eng.add_dof_set("v1", v1)
    X = x0.copy()
    dt, k, th, epsv = np.array([0.01]), np.array([1e6]), np.array([thick, thick]), np.array([1e-3])
    eng.contact_init(v1=eng.array(v1, 3), x0=eng.array(x0, 3), X=eng.array(X, 3), dt=eng.array(dt, 1), k=eng.array(k, 1), thickness=eng.array(th, 1), epsv=eng.array(epsv, 1))
    big_tris, big_edges = np.array([[0, 1, 2]]), np.array([[0, 1], [0, 2], [1, 2]])
    eng.contact_add_mesh("d", 0, np.arange(n * n), tris, edges)
    eng.contact_add_mesh("d", 0, n * n + np.arange(3), big_tris, big_edges)
    eng.contact_disable_collision(0, 0)
    scene = oc.ContactScene([oc.Mesh("d", 0, np.arange(n * n), tris, edges, thick), oc.Mesh("d", 0, n * n + np.arange(3), big_tris, big_edges, thick)])
    return eng, dict(scene=scene, X=x0), n, thick, tris


def test_long_incidence_lists_take_the_wavefront_path():
    """The patch hovers at half of dhat: 144 rows of type P_T, every vertex of the large triangle has 144 incident rows."""
    eng, c, n, thick, tris = patch_scene(0.01)
    assert eng.contact_update(0.01) == n * n
    rep = eng.contact_report()
    assert (rep["source"] == 0).all() and (rep["type"] == oc.P_T).all() and (rep["prim_b"] == len(tris)).all() and sorted(rep["prim_a"]) == list(range(n * n))
    assert np.abs(rep["d"] - thick).max() <= 64 * U * thick and (rep["flags"] == 0).all()
    vrep = eng.contact_vertex_report()
    assert eng.counter("contact_report_long_rows") == 3
    rec = vrep["records"]
    fn = rep["fn"]
    assert (rec[n * n:, 1] == n * n).all() and (rec[:n * n, 1] == 1).all()
    shares = []
    for j in range(3):
        terms = [cr.weights(0, oc.P_T, rep["params"][r, 0], rep["params"][r, 1])[1][j] * fn[r] for r in range(n * n)]
        assert abs(rec[n * n + j, 2] - math.fsum(terms)) <= cr.sum_bound(terms)
        shares += terms
    # the weights of a row sum to one (within three roundings): the three shares add up to the sum of fn
    total = math.fsum(fn)
    assert abs(rec[n * n:, 2].sum() - total) <= cr.sum_bound(shares) + 4 * U * total
    assert np.array_equal(rec[:n * n, 2], fn[np.argsort(rep["prim_a"])])  # a patch vertex carries its row's whole fn (weight exactly 1)
    area = 0.5 * 4.0 * 4.0 / 3.0
    assert np.abs(rec[n * n:, 3] - area).max() <= 64 * U * area
    pairs = eng.contact_pair_report()
    assert pairs[0, 1, 0] == n * n and pairs[0, 0, 0] == 0 and np.isinf(pairs[0, 0, 1]) and abs(pairs[0, 1, 3] - total) <= cr.sum_bound(list(fn))
    assert abs(pairs[0, 1, 6] - total) <= cr.sum_bound(list(fn)) + 64 * U * total  # the patch (group 0) is pushed up
    eng.close()


# ---- 5. pair report --------------------------------------------------------------------------------------------------------------------------------
def check_pairs(c, rep, pairs):
    want, terms = cr.pair_report(c["scene"], rep["ints"], rep["doubles"])
    assert np.array_equal(pairs[:, :, :3], want[:, :, :3])  # counts, minima and dhat exact
    for (ga, gb), T in terms.items():
        for f, xs in T.items():
            assert abs(pairs[ga, gb, f] - math.fsum(xs)) <= cr.sum_bound(xs), (ga, gb, f)
    G = len(c["scene"].meshes)
    assert (pairs[np.tril_indices(G, -1)] == 0.0).all()
    return terms


@pytest.mark.parametrize("name", FIXTURES)
def test_pair_report(name):
    eng, c = installed(name)
    rep = eng.contact_report()
    pairs = eng.contact_pair_report()
    terms = check_pairs(c, rep, pairs)
    if name in ("contactmix_t0", "contactrods_t0"):
        # no mollified rows: the resultant of the 21 barrier potentials on a deformable group is the signed sum of the pair vectors with its partners
        # (the group's own pair is left out: its forces act on the group from both sides and cancel). The bound is the summation bound of the sum the
        # readout forms, (n + 8) * 2^-53 * sum |terms|: its terms are the node forces w fn n on the group's nodes, of every row the group takes part in
        # (both sides of its own pair's rows), and |term| is the VECTOR's magnitude |w| fn, for every component: the components of a term come out of
        # cross products and a normalisation that mix them, so each carries a rounding error relative to the term's norm, not to its own size.
        # Measured on an MI355X: worst |difference| / bound 0.29 (contactrods_t0 group 2, z), 0.19 on contactrods_t0 group 1. With |term| taken per
        # component instead, that group's x and y miss (ratios 3.0 and 44: 18 rows whose normals lie within 1e-2 of z, differences 3.0e-14 and 2.3e-14
        # beside fn of 44 N) while every other component of both fixtures stays below 0.33. The second assertion isolates the summation itself: the
        # resultant against math.fsum of the readout's own element forces on the group's rows, per component (measured: at most 1.4e-14).
        assert not (rep["flags"] & cr.MOLLIFIED).any()
        L = cr.Layout(c["scene"])
        ri, rd = rep["ints"], rep["doubles"]
        contrib = cr.contributions(c["scene"], ri, rd)
        v1 = dof_row0(c, "v1")
        pots = [eng.potential_id(t) for t in cr.TABLE_NAMES]
        elem = {t: eng.element_forces(eng.potential_id(tn), 1.0 / c["dt"]) for t, tn in enumerate(cr.TABLE_NAMES) if rep["bounds"][t + 1] > rep["bounds"][t]}
        checked, worst = 0, 0.0
        for g, m in enumerate(c["scene"].meshes):
            if m.kind != "d":
                continue
            rows = v1[0] + np.unique(m.verts)
            got = eng.forces_resultant(pots, 1.0 / c["dt"], rows)[:3]
            want = np.zeros(3)
            for h in range(len(c["scene"].meshes)):
                if h != g:
                    want += (1.0 if g < h else -1.0) * pairs[min(g, h), max(g, h), 4:7]
            node_terms = []
            for n in range(len(ri)):
                for j, (cv, w) in enumerate(contrib[n]):
                    if int(L.cv_mesh[cv]) == g and w != 0.0:
                        node_terms.append(w * rd[n, 12])
            bound = cr.sum_bound(node_terms)
            own = [[], [], []]
            rowset = set(int(r) for r in rows)
            for t, (f, brow) in elem.items():
                for e in range(len(f)):
                    for blk in range(brow.shape[1]):
                        if int(brow[e, blk]) in rowset:
                            for k in range(3):
                                own[k].append(f[e, blk, k])
            exact_own = np.array([math.fsum(own[k]) for k in range(3)])
            ratio = np.abs(got - want) / bound
            worst = max(worst, ratio.max())
            own_bound = np.array([cr.sum_bound(own[k]) for k in range(3)])
            print("%s group %d: %d node terms, |resultant - pair vectors| %s, bound %.3g, ratio %s; |resultant - fsum of its %d element forces| %s, bound %s"
                  % (name, g, len(node_terms), np.abs(got - want), bound, ratio, len(own[0]), np.abs(got - exact_own), own_bound))
            assert (np.abs(got - exact_own) <= own_bound).all(), g
            checked += 1
        assert checked > 0
        assert worst <= 1.0, worst
    eng.close()


# ---- 6. reproducibility ----------------------------------------------------------------------------------------------------------------------------
def all_reports(eng):
    r, v, p = eng.contact_report(), eng.contact_vertex_report(), eng.contact_pair_report()
    return [r["ints"], r["doubles"], v["records"], v["group"], v["source_index"], p]


def same_bits(a, b):
    return all(x.shape == y.shape and x.tobytes() == y.tobytes() for x, y in zip(a, b))


def test_two_reports_of_one_state_are_bit_identical():
    eng, c = installed("contactmix_t0")
    first = all_reports(eng)
    assert same_bits(first, all_reports(eng))
    eng.contact_set_broad_phase(True)  # the all-pairs broad phase: the same pair set, searched and installed again
    searches = eng.counter("contact_searches")
    assert eng.contact_update(c["dt"]) == len(c["keys"]) and eng.counter("contact_searches") == searches + 1
    assert same_bits(first, all_reports(eng))
    eng.close()


# ---- 7. moved state --------------------------------------------------------------------------------------------------------------------------------
def test_report_follows_the_dofs_with_the_installed_keys():
    eng, c = installed("contactmix_t0")
    man, st, dt = c["man"], c["st"], c["dt"]
    tables = {t: eng.contact_table(t) for t in cr.TABLE_NAMES}
    X_detector = eng.contact_vertices()
    detector_counters = ["contact_searches", "contact_repeated_searches", "ccd_queries", "ccd_skipped_pairs", "ccd_capped_pairs"]
    before = [eng.counter(n) for n in detector_counters]
    soft = man["dof_sets"][0]
    u2 = eng.get_dofs()
    u2[soft["offset"] + 2:soft["offset"] + soft["size"]:3] += 0.004 / dt  # every deformable node 4 mm up within the step
    eng.set_dofs(u2)
    st2 = dict(st)
    st2["v1"] = u2[soft["offset"]:soft["offset"] + soft["size"]].reshape(-1, 3)
    X2 = np.concatenate(oc.mesh_vertices(c["scene"], st2, dt))
    ri, rd = cr.rows(c["scene"], c["keys"], X2, c["Xrest"], c["k"])
    rep = eng.contact_report()
    check_rows(rep, ri, rd, np.abs(X2).max(), c["k"], "moved")
    n_open = int(((rep["flags"] & cr.OPEN) != 0).sum())
    assert 0 < n_open < len(ri) and ((rep["d"] >= rep["dhat"]) == ((rep["flags"] & cr.OPEN) != 0)).all()
    check_vertices(c, rep, eng.contact_vertex_report(), X2)
    check_pairs(c, rep, eng.contact_pair_report())
    # the detector has not moved: no search, its vertices and tables as installed
    assert [eng.counter(n) for n in detector_counters] == before
    assert np.array_equal(eng.contact_vertices(), X_detector)
    for t, rows in tables.items():
        assert np.array_equal(eng.contact_table(t), rows)
    eng.close()


# ---- 8. nothing else moves -------------------------------------------------------------------------------------------------------------------------
def test_reports_between_the_stages_change_nothing():
    from stark_amd import capi

    def sequence(report):
        eng, c = build("contactmix_t0")
        if report:
            all_reports(eng)  # (before the first search)
        eng.contact_update_friction()
        eng.contact_update(c["dt"])
        if report:
            all_reports(eng)
        E, grad = eng.eval(capi.EVAL_P_G_H)
        if report:
            all_reports(eng)
        eng.assemble()
        if report:
            all_reports(eng)
        bsr = eng.get_bsr()
        x, info = eng.pcg(c["man"]["pcg"]["abs_tol"])
        assert eng.counter("contact_reports") == (11 if report else 0)  # (four times three; the row report of an empty key list launches nothing)
        eng.close()
        return E, grad, bsr, x, info.n_iterations

    E0, g0, (rp0, c0, v0), x0, it0 = sequence(False)
    E1, g1, (rp1, c1, v1), x1, it1 = sequence(True)
    assert E0 == E1 and np.array_equal(g0, g1)
    assert np.array_equal(rp0, rp1) and np.array_equal(c0, c1) and np.array_equal(v0, v1)
    assert it0 == it1 and np.array_equal(x0, x1)


def _counter(sim, name):
    from stark_amd import capi

    v = C.c_int64()
    assert capi.lib().mistark_get_counter(sim.engine_handle(), name.encode(), C.byref(v)) == 0
    return v.value


def test_recording_does_not_change_a_trajectory_with_friction():
    from stark_amd import sim as S

    def run(record):
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
            sim.record_contacts(True)
        counts = []
        for _ in range(3):
            assert sim.run_one_step()
            i = sim.info()
            counts.append((i.total_newton_iterations, i.total_linear_solves, i.total_cg_iterations))
        info = sim.contact_info()
        out = sim.points("x0"), sim.points("v0"), counts, info["n_contacts"], info["n_friction_contacts"], _counter(sim, "contact_reports")
        if record:
            rep = sim.contacts()
            assert rep["labels"] == ["block", "box"] and len(rep["rows"]["d"]) == info["n_contacts"] > 0
            assert rep["pairs"][0, 1, 0] == info["n_contacts"] and rep["pairs"][0, 1, 6] > 0.0  # the block (group 0) is pushed up
            assert abs(rep["time"] - sim.info().current_time) < 1e-12
        else:
            with pytest.raises(S.SimError, match="recording is off"):
                sim.contacts()
        sim.close()
        return out

    x_off, v_off, c_off, n_off, f_off, r_off = run(False)
    x_on, v_on, c_on, n_on, f_on, r_on = run(True)
    assert r_off == 0 and r_on == 3
    assert n_on == n_off and f_on == f_off and f_on > 0
    assert c_on == c_off and np.array_equal(x_on, x_off) and np.array_equal(v_on, v_off)


# ---- 9. refusals and empties -----------------------------------------------------------------------------------------------------------------------
def test_refusals_name_their_cause():
    import stark_amd
    from stark_amd import capi

    L = capi.lib()
    group = L.mistark_local_group_create(2)
    try:
        eng = stark_amd.Engine(0)
        eng.dist_init_local(group, 0)
        eng.add_dof_set("u", np.zeros(6))
        for call in (eng.contact_report, eng.contact_vertex_report, eng.contact_pair_report):
            with pytest.raises(stark_amd.engine.EngineError, match="single-rank"):
                call()
        eng.close()
    finally:
        L.mistark_local_group_destroy(group)
    h = C.c_void_p()
    assert L.mistark_create_dry(C.byref(h)) == 0
    try:
        n, g = C.c_int64(), C.c_int32()
        for rc in (L.mistark_contact_report(h, None, None, C.byref(n)), L.mistark_contact_vertex_report(h, None, None, None, C.byref(n)),
                   L.mistark_contact_pair_report(h, None, C.byref(g))):
            assert rc < 0 and "registration-only" in L.mistark_last_error(h).decode()
    finally:
        L.mistark_destroy(h)
    eng = stark_amd.Engine(0)
    eng.add_dof_set("u", np.zeros(6))
    for call in (eng.contact_report, eng.contact_vertex_report, eng.contact_pair_report):
        with pytest.raises(stark_amd.engine.EngineError, match="mistark_contact_init"):
            call()
    assert eng.counter("contact_reports") == 0
    eng.close()


def check_empty(eng, c):
    L = cr.Layout(c["scene"])
    rep, vrep, pairs = eng.contact_report(), eng.contact_vertex_report(), eng.contact_pair_report()
    assert rep["ints"].shape == (0, 8) and rep["doubles"].shape == (0, 16) and (rep["bounds"] == 0).all()
    rec = vrep["records"]
    assert len(rec) == L.n_v and np.isposinf(rec[:, 0]).all() and (rec[:, [1, 2, 4]] == 0.0).all()
    G = len(c["scene"].meshes)
    iu = np.triu_indices(G)
    assert pairs.shape == (G, G, 8) and (pairs[:, :, 0] == 0).all() and np.isposinf(pairs[iu][:, 1]).all() and (pairs[:, :, 3:] == 0.0).all()
    assert np.array_equal(pairs[iu][:, 2], L.thick[iu[0]] + L.thick[iu[1]])
    return rec


def test_no_rows_before_the_first_search_and_far_apart():
    eng, c = build("contactmix_t0")
    rec = check_empty(eng, c)
    ta = cr.triangle_areas(c["scene"], c["X"])
    assert abs(rec[:, 3].sum() - ta.sum()) <= 64 * U * len(ta) * ta.sum()  # areas need no contact
    assert eng.counter("contact_searches") == 0
    eng.close()
    eng, c, n, thick, tris = patch_scene(1.0)  # the patch a metre above the triangle: a search finds nothing
    assert eng.contact_update(0.01) == 0 and eng.counter("contact_searches") == 1
    check_empty(eng, c)
    assert eng.counter("contact_report_long_rows") == 0
    eng.close()


# ---- 10. host mirror -------------------------------------------------------------------------------------------------------------------------------
def test_host_mirror_records_the_end_of_step_state():
    """Two deformable blocks (no rigid body: the whole state is x0 and v1): the step's recorded report against engine-level reports of the same state —
    x0 put back to the start of the step, the DoFs at the converged v1 — bit for bit."""
    import stark_amd
    from stark_amd import capi
    from stark_amd import sim as S

    st = S.default_settings()
    st.max_time_step_size = 0.01
    st.init_frictional_contact = 1
    sim = S.Simulation(st)
    gp = S.contact_global_params()
    gp.default_contact_thickness = 1e-3
    sim.set_contact_global_params(gp)
    sim.add_volume_grid("upper", (0.0, 0.0, 0.1 + 1.5e-3), (0.1, 0.1, 0.1), (3, 3, 3), S.soft_rubber())
    sim.add_volume_grid("lower", (0.0, 0.0, 0.0), (0.2, 0.2, 0.1), (4, 4, 2), S.soft_rubber())
    assert sim.run_one_step()
    assert _counter(sim, "contact_reports") == 0  # recording off: nothing ran
    with pytest.raises(S.SimError, match="recording is off"):
        sim.contacts()
    sim.record_contacts(True)
    with pytest.raises(S.SimError, match="no time step has been accepted"):
        sim.contacts()
    x0_start = sim.points("x0")
    assert sim.run_one_step()
    assert _counter(sim, "contact_reports") == 1
    rec = sim.contacts()
    assert rec["labels"] == ["upper", "lower"] and len(rec["rows"]["d"]) == sim.contact_info()["n_contacts"] > 0
    assert abs(rec["time"] - sim.info().current_time) < 1e-12
    v1 = sim.points("v0")  # (v0 <- v1 when the step was accepted)
    sim.set_points("x0", x0_start)
    eng = stark_amd.Engine.__new__(stark_amd.Engine)  # the simulation's own engine context through the facade (not owned: never closed here)
    eng.L, eng.h = capi.lib(), sim.engine_handle()
    try:
        assert eng.ndofs == v1.size
        eng.set_dofs(v1.reshape(-1))
        direct = all_reports(eng)
    finally:
        eng.h = None
    mirror = [rec["rows"]["ints"], rec["rows"]["doubles"], rec["vertices"]["records"], rec["vertices"]["group"], rec["vertices"]["source_index"], rec["pairs"]]
    assert same_bits(direct, mirror)
    sim.record_contacts(False)
    with pytest.raises(S.SimError, match="recording is off"):
        sim.contacts()
    sim.close()
