"""The curved rigid-body CCD on the device: the padded kernels against the restatement (tests/ccd_curved_ref.py) through mistark_cd_run_ccd_padded,
the whole query through mistark_contact_max_step_ex on synthesised rigid scenes and on the contact fixtures, its reduction to the linear query, the
round loop, non-interference with the evaluation and the solver, the scene API's mode switch and the refusals."""
import json
import math
import os
import sys

import numpy as np
import pytest

import ccd_curved_ref as CR
import ccd_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
ETA = 0.9
TRI_EDGES = [[0, 1], [1, 2], [2, 0]]


def _close(dev, ref, step):
    """equal to 1e-12 relative, or one final ACCD increment (`step`: a callable giving it at a reported value) apart (a tie of the stop test) —
    the rule of tests/test_gpu_ccd.py"""
    if abs(dev - ref) <= 1e-12 * max(abs(dev), abs(ref)):
        return True
    if ref < 1.0 and dev < 1.0:
        return abs(dev - ref) <= step(min(dev, ref)) * (1 + 1e-9)
    return False


def _random_pairs(rng, n):
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from test_ccd_cpu import _random_crossings

    out = [(ee, xa, xb) for ee, xa, xb, _ in _random_crossings(rng, n // 2)]
    for k in range(n - n // 2):
        xa = rng.normal(size=(4, 3))
        out.append((k % 2 == 1, xa, xa + rng.normal(size=(4, 3)) * rng.uniform(0.1, 2.0)))
    return out


# ---- 1. the padded kernels on straight lines ---------------------------------------------------------------------------------------------------
def test_padded_kernels_against_restatement():
    """600 single pairs with pair pads of 0, 5 %, 45 %, 55 %, 105 % and 170 % of d(0), spread over the vertices at random."""
    from stark_amd import capi

    rng = np.random.default_rng(21)
    pairs = _random_pairs(rng, 600)
    pt_x, ee_x = [np.zeros((1, 3)), np.zeros((3, 3))], [np.zeros((2, 3)), np.zeros((2, 3))]
    cd_pt, cd_ee = capi.CollisionDetector(), capi.CollisionDetector()
    cd_pt.add_mesh(pt_x[0], np.zeros((0, 3)), np.zeros((0, 2)))
    cd_pt.add_mesh(pt_x[1], [[0, 1, 2]], TRI_EDGES)
    cd_ee.add_mesh(ee_x[0], np.zeros((0, 3)), [[0, 1]])
    cd_ee.add_mesh(ee_x[1], np.zeros((0, 3)), [[0, 1]])
    n_hit = n_tie = n_zero = n_bound = 0
    for k, (ee, xa, xb) in enumerate(pairs):
        cd, xs, split = (cd_ee, ee_x, 2) if ee else (cd_pt, pt_x, 1)
        xs[0][:] = xa[:split]
        xs[1][:] = xa[split:]
        d0 = R.distance(ee, [tuple(p) for p in xa])
        target = d0 * [0.0, 0.05, 0.45, 0.55, 1.05, 1.7][(k // 2) % 6]
        f = rng.uniform(0.0, 1.0)
        pad_v = np.zeros(4)
        sides = ([0], [1, 2, 3]) if not ee else ([0, 1], [2, 3])
        for side, share in zip(sides, (f * target, (1.0 - f) * target)):
            pad_v[side] = share * rng.uniform(0.0, 1.0, size=len(side))
            pad_v[rng.choice(side)] = share
        pad = CR.pair_pad(ee, pad_v)
        toi, n, nb = cd.run_ccd_padded([xb[:split], xb[split:]], [pad_v[:split], pad_v[split:]], ETA)
        pt_c, ee_c = CR.candidates_padded(xa, xb, pad_v, np.array([[1, 2, 3]]) if not ee else np.zeros((0, 3), int),
                                          np.array([[0, 1], [2, 3]]) if ee else np.array([[1, 2], [2, 3], [3, 1]]))
        assert n == len(pt_c) + len(ee_c), (k, ee, xa, xb, pad_v)
        r = CR.accd_padded(ee, xa, xb, pad, ETA) if n else dict(status="none", bound=False)
        ref = r["toi"] if r["status"] in ("hit", "capped", "zero_gap") else 1.0
        assert _close(toi, ref, lambda t: CR.last_step_padded(ee, xa, xb, pad, ETA, t)), (k, toi, ref, r, pad)
        assert nb == int(r["bound"]), (k, nb, r, pad)
        n_tie += abs(toi - ref) > 1e-12 * max(toi, ref)
        n_hit += 0.0 < toi < 1.0
        n_zero += toi == 0.0
        n_bound += nb
        if target == 0.0:   # every pad 0.0: the unpadded query's bits
            assert (toi, n) == cd.run_ccd([xb[:split], xb[split:]], ETA)
    print("pairs %d, hits %d, no gap %d, pad-bound %d, one-increment ties %d" % (len(pairs), n_hit, n_zero, n_bound, n_tie))
    assert n_hit > 150 and n_zero > 60 and n_bound > n_zero and n_tie <= len(pairs) // 20
    cd_pt.close()
    cd_ee.close()


def test_padded_kernels_scene_candidates_and_minimum():
    """60 small meshes with random pads in one detector: the candidate count is the brute-force count of the inflated swept boxes, the minimum and
    the pad-bound count are the restatement's, two runs give the same bits; with zero pads the unpadded query's bits."""
    from stark_amd import capi

    rng = np.random.default_rng(6)
    cd = capi.CollisionDetector()
    xs, x1s, pads, tris, edges, off = [], [], [], [], [], 0
    for m in range(60):
        if m % 2 == 0:
            x = rng.uniform(0, 1, size=3) + rng.normal(size=(4, 3)) * 0.08
            t, e = np.array([[0, 1, 2], [1, 3, 2]]), np.array([[0, 1], [1, 2], [2, 0], [1, 3], [3, 2]])
        else:
            x = rng.uniform(0, 1, size=3) + np.cumsum(rng.normal(size=(4, 3)) * 0.06, axis=0)
            t, e = np.zeros((0, 3), int), np.array([[0, 1], [1, 2], [2, 3]])
        x = np.ascontiguousarray(x)
        cd.add_mesh(x, t, e)
        xs.append(x)
        x1s.append(x + rng.normal(size=3) * 0.15 + rng.normal(size=(4, 3)) * 0.02)
        pads.append(rng.uniform(0.0, 0.004, size=4) * (m % 3 != 0))   # (a third of the meshes move on their straight lines)
        tris += (t + off).tolist()
        edges += (e + off).tolist()
        off += 4
    xa, xb = np.vstack(xs), np.vstack(x1s)
    n_plain = R.max_step(xa, xb, np.array(tris), np.array(edges), ETA)[1]
    # as drawn, some pair's pad leaves no gap: no step
    toi, n, nb = cd.run_ccd_padded(x1s, pads, ETA)
    q = CR.padded_query(xa, xb, np.concatenate(pads), tris, edges, ETA, cut=True)
    print("scene: %d candidates (%d without pads), %d pad-bound, toi %.17g (restatement %.17g)" % (n, n_plain, nb, toi, q["toi"]))
    assert q["toi"] == 0.0 and (toi, n, nb) == (0.0, q["n_candidates"], q["n_pad_bound"]) and n > n_plain > 100
    # ... and with the pads of the meshes of such pairs taken away: a step limited by a padded pair or an unpadded one
    for _ in range(20):
        if q["toi"] > 0.0:
            break
        for ee, v, r in q["pairs"]:
            if r["status"] == "zero_gap":
                for i in v:
                    pads[i // 4][:] = 0.0
        q = CR.padded_query(xa, xb, np.concatenate(pads), tris, edges, ETA, cut=True)
    toi, n, nb = cd.run_ccd_padded(x1s, pads, ETA)
    print("       %d candidates, %d pad-bound, toi %.17g (restatement %.17g)" % (n, nb, toi, q["toi"]))
    assert 0.0 < q["toi"] < 1.0 and q["n_pad_bound"] > 0 and q["max_pad"] > 0.0
    assert n == q["n_candidates"] and n > n_plain and nb == q["n_pad_bound"]
    ee, v, r = [(ee, v, r) for ee, v, r in q["pairs"] if r["status"] in ("hit", "capped") and r["toi"] == q["toi"]][0]
    assert _close(toi, q["toi"], lambda t: CR.last_step_padded(ee, xa[v], xb[v], r["pad"], ETA, t)), (toi, q["toi"])
    assert (toi, n, nb) == cd.run_ccd_padded(x1s, pads, ETA)
    zero = [np.zeros(4) for _ in pads]
    t0, n0, nb0 = cd.run_ccd_padded(x1s, zero, ETA)
    assert (t0, n0) == cd.run_ccd(x1s, ETA) and nb0 == 0
    cd.close()


# ---- an engine with rigid bodies from a restatement scene --------------------------------------------------------------------------------------
def engine_from_scene(sc):
    """DoF sets v1 | rb_v1 | rb_w1 (a direction is their concatenation); the 35 contact potentials with empty tables are the engine's only potentials"""
    import stark_amd

    eng = stark_amd.Engine(0)
    keep = dict(v1=np.ascontiguousarray(sc.v1), rb_v1=np.ascontiguousarray(sc.v), rb_w1=np.ascontiguousarray(sc.w), x0=np.ascontiguousarray(sc.x0), X=sc.x0.copy(),
                rb_xloc=np.ascontiguousarray(sc.x_loc), rb_t0=np.ascontiguousarray(sc.t0), rb_q0=np.ascontiguousarray(sc.q0), dt=np.array([sc.dt]), k=np.array([1e6]),
                thickness=np.full(len(sc.meshes), 1e-3), epsv=np.array([1e-3]))
    for name in ("v1", "rb_v1", "rb_w1"):
        eng.add_dof_set(name, keep[name])
    eng.contact_init(**{role: eng.array(a, {"rb_q0": 4}.get(role, 3 if a.ndim == 2 else 1)) for role, a in keep.items()})
    for m in sc.meshes:
        eng.contact_add_mesh("d" if m["kind"] == "d" else "rb", m.get("body", 0), m["verts"], m["tris"], m["edges"])
    eng.scene_arrays = keep
    return eng


def _du(dv1, dv, dw):
    return np.concatenate([np.ravel(dv1), np.ravel(dv), np.ravel(dw)])


def _limiting_step(sc_res):
    """the final increment of the pair that limits a restated query, as a function of the reported value (in units of the last round's interval)"""
    q = sc_res["query"]
    lim = [(ee, v, r) for ee, v, r in q["pairs"] if r["status"] in ("hit", "capped") and r["toi"] == q["toi"]]
    if not lim:
        return lambda t: 0.0
    ee, v, r = lim[0]
    return lambda t: sc_res["tau"] * CR.last_step_padded(ee, sc_res["xa"][v], sc_res["xb"][v], r["pad"], ETA, t / sc_res["tau"])


# ---- 2. the discriminating scene ---------------------------------------------------------------------------------------------------------------
def test_blade_scene_curved_against_linear():
    """A blade turning by 1.2 rad along the direction sweeps through a small triangle that the chords of its vertices miss (proved on the CPU:
    tests/test_ccd_curved_cpu.py). The linear query allows the whole step, beyond the contact; the curved one stops before it."""
    from test_ccd_curved_cpu import blade_crossing_time, check_against_true_motion

    phi = 1.2
    sc, dv1, dv, dw = CR.blade_scene(phi)
    eng = engine_from_scene(sc)
    du = _du(dv1, dv, dw)
    lin_ref, cur_ref = CR.max_step_linear(sc, dv1, dv, dw, ETA), CR.max_step_curved(sc, dv1, dv, dw, ETA, 4)
    lin = eng.contact_max_step_ex(sc.dt, ETA, "linear", 4, du)
    print("linear", lin, "\ncurved restated", {k: cur_ref[k] for k in lin})
    assert lin["max_step"] == lin_ref["max_step"] == 1.0 > blade_crossing_time(phi)    # the documented limitation
    assert (lin["n_candidates"], lin["rounds"], lin["tau"], lin["pad_bound_pairs"], lin["max_pad"]) == (lin_ref["n_candidates"], 1, 1.0, 0, 0.0)
    cur = eng.contact_max_step_ex(sc.dt, ETA, "curved", 4, du)
    print("curved", cur)
    assert _close(cur["max_step"], cur_ref["max_step"], _limiting_step(cur_ref))
    assert (cur["n_candidates"], cur["rounds"], cur["tau"], cur["pad_bound_pairs"]) == (cur_ref["n_candidates"], cur_ref["rounds"], cur_ref["tau"], cur_ref["pad_bound_pairs"])
    assert abs(cur["max_pad"] - cur_ref["max_pad"]) <= 8 * 2.0 ** -53 * cur_ref["max_pad"]
    assert 0.0 < cur["max_step"] < blade_crossing_time(phi)
    check_against_true_motion(sc, dv1, dv, dw, dict(cur_ref, max_step=cur["max_step"]), ETA, 2001)
    assert cur == eng.contact_max_step_ex(sc.dt, ETA, "curved", 4, du)    # the same bits from run to run
    assert eng.counter("ccd_rounds") == 1 + 2 * cur["rounds"] and eng.counter("ccd_queries") == 3 and eng.counter("ccd_pad_bound_pairs") == 0
    eng.close()


def test_random_rigid_scenes_against_restatement():
    """The scenes of tests/test_ccd_curved_cpu.py (a spinning, translating rigid triangle with a random start orientation next to a moving deformable
    one; the restated query is checked against the true motion there): both modes on the device equal the restatement, round for round."""
    from test_ccd_curved_cpu import _random_scene

    rng = np.random.default_rng(3)
    rounds, n_limited = [], 0
    for k in range(16):
        sc, dv1, dv, dw = _random_scene(rng)
        eng = engine_from_scene(sc)
        du = _du(dv1, dv, dw)
        for mode, ref in (("linear", CR.max_step_linear(sc, dv1, dv, dw, ETA)), ("curved", CR.max_step_curved(sc, dv1, dv, dw, ETA, 4))):
            got = eng.contact_max_step_ex(sc.dt, ETA, mode, 4, du)
            assert (got["n_candidates"], got["rounds"], got["tau"], got["pad_bound_pairs"]) == (ref["n_candidates"], ref["rounds"], ref["tau"], ref["pad_bound_pairs"]), (k, mode, got)
            assert _close(got["max_step"], ref["max_step"], _limiting_step(ref)), (k, mode, got["max_step"], ref["max_step"])
            assert abs(got["max_pad"] - ref["max_pad"]) <= 16 * 2.0 ** -53 * ref["max_pad"]
        rounds.append(got["rounds"])
        n_limited += 0.0 < got["max_step"] < 1.0
        eng.close()
    print("rounds", rounds, "limited", n_limited)
    assert max(rounds) == 4 and min(rounds) == 1 and n_limited >= 4


# ---- 3. reduction to the present query ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["contactmix_t0", "contactcorners_t0", "contactrods_t0"])
def test_without_rotation_change_curved_is_linear(name):
    from stark_amd import capi

    from contact_util import roles_from_manifest
    from test_gpu_contact import build

    eng, prob, man, z, scene, st = build(name)
    dt = float(np.asarray(st["dt"]).ravel()[0])
    roles = roles_from_manifest(man)
    rng = np.random.default_rng(31)
    du = rng.normal(size=eng.ndofs) * 0.02 / dt    # (velocities: vertices move by about 2 cm along the direction)
    n_rigid = sum(m.kind != "d" for m in scene.meshes)
    if name != "contactrods_t0":
        assert n_rigid > 0 and "rb_w1" in roles
    for s, a in prob.dof_arrays.items():
        if a == roles.get("rb_w1", -2):
            du[prob.dof_offsets[s]:prob.dof_offsets[s] + prob.dof_sizes[s]] = 0.0
    lin = eng.contact_max_step_ex(dt, ETA, "linear", 4, du)
    cur = eng.contact_max_step_ex(dt, ETA, "curved", 4, du)
    print(name, lin)
    assert lin["n_candidates"] > 0 and 0.0 < lin["max_step"] <= 1.0
    assert (cur["max_step"], cur["n_candidates"], cur["rounds"], cur["tau"], cur["pad_bound_pairs"], cur["max_pad"]) == (lin["max_step"], lin["n_candidates"], 1, 1.0, 0, 0.0)
    # du = NULL inside a callback: the query of mistark_contact_max_step
    seen = []

    def max_step(_):
        seen.append((eng.contact_max_step(dt, ETA), eng.contact_max_step_ex(dt, ETA, "linear", 4, None), eng.contact_max_step_ex(dt, ETA, "curved", 1, None)))
        return 1.0

    cb = capi.NewtonCallbacks()
    cb.max_allowed_step = capi.DBLCB(max_step)
    s = eng.default_newton_settings()
    s.max_iterations = 2
    eng.newton_solve(s, cb)
    assert seen
    for (t, n), ex, cu in seen:
        assert (ex["max_step"], ex["n_candidates"], ex["rounds"]) == (t, n, 1)
        assert 0.0 <= cu["max_step"] <= 1.0 and cu["rounds"] == 1
    eng.close()


# ---- 4. rounds ---------------------------------------------------------------------------------------------------------------------------------
def test_rounds_halve_the_interval_until_the_pads_let_go():
    sc, dv1, dv, dw = CR.blade_scene(2.5)
    eng = engine_from_scene(sc)
    du = _du(dv1, dv, dw)
    ref = CR.max_step_curved(sc, dv1, dv, dw, ETA, 4)
    first = CR.max_step_curved(sc, dv1, dv, dw, ETA, 1)
    assert first["pad_bound_pairs"] > 0 and (ref["rounds"], ref["tau"], ref["pad_bound_pairs"]) == (3, 0.25, 0) and 0.0 < ref["max_step"] < 0.25
    got = eng.contact_max_step_ex(sc.dt, ETA, "curved", 4, du)
    print("rounds", got)
    assert (got["rounds"], got["tau"], got["pad_bound_pairs"], got["n_candidates"]) == (3, 0.25, 0, ref["n_candidates"])
    assert _close(got["max_step"], ref["max_step"], _limiting_step(ref))
    assert eng.counter("ccd_rounds") == 3 and eng.counter("ccd_queries") == 1 and eng.counter("ccd_pad_bound_pairs") == 0
    one = eng.contact_max_step_ex(sc.dt, ETA, "curved", 1, du)
    assert (one["rounds"], one["tau"], one["pad_bound_pairs"], one["n_candidates"]) == (1, 1.0, first["pad_bound_pairs"], first["n_candidates"])
    eng.close()
    # still bound when the rounds run out: no step, and the result says why
    sc, dv1, dv, dw = CR.blade_scene(3.0)
    eng = engine_from_scene(sc)
    ref = CR.max_step_curved(sc, dv1, dv, dw, ETA, 2)
    assert ref["max_step"] == 0.0 and ref["rounds"] == 2 and ref["pad_bound_pairs"] > 0
    got = eng.contact_max_step_ex(sc.dt, ETA, "curved", 2, _du(dv1, dv, dw))
    print("out of rounds", got)
    assert (got["max_step"], got["rounds"], got["tau"], got["pad_bound_pairs"], got["n_candidates"]) == (0.0, 2, 0.5, ref["pad_bound_pairs"], ref["n_candidates"])
    assert eng.counter("ccd_pad_bound_pairs") == ref["pad_bound_pairs"]
    eng.close()


# ---- 5. non-interference -----------------------------------------------------------------------------------------------------------------------
def _stages(name, query):
    from stark_amd import capi

    from test_gpu_contact import build, is_contact

    eng, prob, man, z, scene, st = build(name)
    dt = float(np.asarray(st["dt"]).ravel()[0])
    du = np.random.default_rng(41).normal(size=eng.ndofs)
    ask = (lambda: eng.contact_max_step_ex(dt, ETA, "curved", 4, du)) if query else (lambda: None)
    out = {}
    ask()
    out["n"] = (eng.contact_update_friction(), eng.contact_update(dt))
    ask()
    out["tables"] = [eng.contact_table(p["name"]) for p in man["potentials"] if is_contact(p["name"])]
    out["keys"] = eng.contact_report()["ints"]
    out["E"], out["grad"] = eng.eval(capi.EVAL_P_G_H)
    ask()
    eng.assemble()
    out["bsr"] = eng.get_bsr()
    ask()
    out["x"], info = eng.pcg(1e-10, max_iter=5)
    ask()
    out["again"] = (eng.contact_update(dt), eng.eval(capi.EVAL_P)[0])
    rounds = eng.counter("ccd_rounds")
    eng.close()
    return out, rounds


def _same(a, b):
    if isinstance(a, (list, tuple)):
        return len(a) == len(b) and all(_same(p, q) for p, q in zip(a, b))
    return np.array_equal(np.asarray(a), np.asarray(b))


def test_curved_queries_change_nothing():
    plain, r0 = _stages("contactmix_t0", False)
    asked, r1 = _stages("contactmix_t0", True)
    assert r0 == 0 and r1 >= 5
    assert plain["n"][1] > 0 and len(plain["keys"]) == plain["n"][1]
    for k in plain:
        assert _same(plain[k], asked[k]), k


# ---- 6. the scene API --------------------------------------------------------------------------------------------------------------------------
BOX_TRIS = [[0, 1, 3], [0, 3, 2], [4, 6, 7], [4, 7, 5], [0, 4, 5], [0, 5, 1], [2, 3, 7], [2, 7, 6], [0, 2, 6], [0, 6, 4], [1, 5, 7], [1, 7, 3]]


def _edges(T):
    return np.array(sorted({(min(t[k], t[(k + 1) % 3]), max(t[k], t[(k + 1) % 3])) for t in T for k in range(3)}), dtype=np.int32)


def _spinning_box(S, ccd, rigid=None, check=False, n_steps=None):
    """configs[0] as tests/test_gpu_ccd.py runs it; check: edge-triangle intersections of cloth and box at every accepted state"""
    from stark_amd import capi

    z = np.load(os.path.join(GOLDEN, "traj_cfg0_spinning_box_cloth_32.npz"))
    traj = json.loads(bytes(z["traj_json"]).decode())
    sc = traj["scene"]
    st = S.default_settings()
    st.init_frictional_contact = 1
    sim = S.Simulation(st)
    gp = S.contact_global_params()
    gp.default_contact_thickness = sc["thickness"]
    gp.min_contact_stiffness = sc["kmin"]
    sim.set_contact_global_params(gp)
    sim.add_surface_grid("cloth", (sc["size"], sc["size"]), (sc["n"], sc["n"]), S.cotton_fabric())
    box = sim.add_rigid_box("box", 1.0, (sc["box"],) * 3)
    anchor = (0.0, 0.0, -0.5 * sc["box"] - sc["gap"])
    sim.rb_add_translation(box, anchor)
    fix = sim.rb_add_fix(box)
    if ccd:
        sim.set_contact_ccd(True, ETA)
    if rigid:
        sim.set_contact_ccd_rigid(rigid, 4)
    cd = None
    if check:
        _, T = S.generate_triangle_grid((0.0, 0.0), (sc["size"], sc["size"]), (sc["n"], sc["n"]))
        cloth_x, box_x = np.zeros((sim.info().n_points, 3)), np.zeros((8, 3))
        corners = 0.5 * sc["box"] * np.array([[-1.0 if not k & 1 else 1.0, -1.0 if not k & 2 else 1.0, -1.0 if not k & 4 else 1.0] for k in range(8)])
        cd = capi.CollisionDetector()
        cd.add_mesh(cloth_x, T, _edges(T))
        cd.add_mesh(box_x, BOX_TRIS, _edges(BOX_TRIS))
    log, n_ix = [], 0
    for step in range(len(traj["steps"]) if n_steps is None else n_steps):
        sim.rb_fix_set_transformation(fix, anchor, sc["spin"] * sim.info().current_time, (0.0, 0.0, 1.0))
        assert sim.run_one_step()
        i = sim.info()
        assert i.last_newton_result in (0, 8), i.last_newton_result
        s = i.last_stats
        log.append((s.newton_iterations, s.cg_iterations, s.n_linear_solves, s.ls_cap_iterations, s.ls_max_iterations, s.ls_inv_iterations, s.ls_bt_iterations,
                    i.last_newton_result))
        if cd is not None:
            t, q, _, _ = sim.rb_state(box)
            cloth_x[:] = sim.points("x0")
            box_x[:] = corners @ CR.rb_R1(q, (0.0, 0.0, 0.0), 0.0).T + t
            n_ix += len(cd.run_intersection())
    out = dict(log=log, x=sim.points("x0"), state=[np.asarray(v) for v in sim.rb_state(box)], info=sim.ccd_info(), rigid=sim.ccd_rigid_info(), n_ix=n_ix,
               time=sim.info().current_time)
    if cd is not None:
        cd.close()
    sim.close()
    return out


def test_scene_api_rigid_mode():
    from stark_amd import sim as S

    off = _spinning_box(S, False, "curved", n_steps=2)
    assert off["info"]["queries"] == 0 and off["rigid"]["rounds"] == 0 and off["rigid"]["mode"] == "curved"    # CCD off: nothing is registered
    plain = _spinning_box(S, True)
    linear = _spinning_box(S, True, "linear")
    assert linear["log"] == plain["log"] and np.array_equal(linear["x"], plain["x"]) and all(np.array_equal(a, b) for a, b in zip(linear["state"], plain["state"]))
    assert plain["rigid"]["mode"] == "linear" and linear["rigid"]["rounds"] == linear["info"]["queries"] > 0 and linear["rigid"]["max_pad"] == 0.0
    curved = _spinning_box(S, True, "curved", check=True)
    print("configs[0] curved:", curved["info"], curved["rigid"], "linear:", linear["info"])
    assert curved["time"] == plain["time"]    # every step succeeded at the full time step
    assert curved["n_ix"] == 0
    x = curved["x"]
    assert np.isfinite(x).all() and -0.35 < x[:, 2].min() < -0.2 and x[:, 2].max() < -0.02    # draped over the box (the bounds of test_spinning_box_with_ccd)
    assert curved["rigid"]["rounds"] >= curved["info"]["queries"] > 0 and curved["info"]["capped_pairs"] == 0


# ---- 7. refusals -------------------------------------------------------------------------------------------------------------------------------
def test_refusals():
    import stark_amd
    from stark_amd import capi, engine
    from stark_amd import sim as S

    sc, dv1, dv, dw = CR.blade_scene(1.2)
    eng = engine_from_scene(sc)
    du = _du(dv1, dv, dw)
    for eta in (0.0, -0.5, 1.5, float("nan")):
        with pytest.raises(engine.EngineError, match="conservative_rescaling"):
            eng.contact_max_step_ex(sc.dt, eta, "curved", 4, du)
    for rounds in (0, -3):
        with pytest.raises(engine.EngineError, match="max_rounds"):
            eng.contact_max_step_ex(sc.dt, ETA, "curved", rounds, du)
    with pytest.raises(ValueError, match="rigid_mode"):
        eng.contact_max_step_ex(sc.dt, ETA, "spiral", 4, du)
    r = capi.CcdResult()
    assert eng.L.mistark_contact_max_step_ex(eng.h, sc.dt, ETA, 2, 4, None, r) < 0 and b"rigid_mode" in eng.L.mistark_last_error(eng.h)
    for bad in (du[:-1], np.concatenate([du, [0.0]])):
        with pytest.raises(ValueError, match="du has"):
            eng.contact_max_step_ex(sc.dt, ETA, "curved", 4, bad)
    assert eng.counter("ccd_rounds") == 0
    assert eng.contact_max_step_ex(sc.dt, ETA, "curved", 4, du)["max_step"] > 0.0    # (and the engine still answers)
    eng.close()
    # a sharded context
    L = capi.lib()
    group = L.mistark_local_group_create(2)
    try:
        sh = stark_amd.Engine(0)
        sh.dist_init_local(group, 0)
        sh.add_dof_set("u", np.zeros(6))
        for mode in ("linear", "curved"):
            with pytest.raises(engine.EngineError, match="sharded"):
                sh.contact_max_step_ex(sc.dt, ETA, mode, 4, np.zeros(6))
        sh.close()
    finally:
        L.mistark_local_group_destroy(group)
    # the scene API
    st = S.default_settings()
    st.init_frictional_contact = 1
    sim = S.Simulation(st)
    with pytest.raises(ValueError, match="mode"):
        sim.set_contact_ccd_rigid("spiral")
    with pytest.raises(Exception, match="max_rounds"):
        sim.set_contact_ccd_rigid("curved", 0)
    sim.set_contact_ccd_rigid("curved", 2)
    assert sim.ccd_rigid_info() == dict(mode="curved", rounds=0, pad_bound_pairs=0, max_pad=0.0)
    sim.close()
