"""Continuous collision detection on the device: the kernels against the restatement (tests/ccd_ref.py) through mistark_cd_run_ccd, tunnelling
scenes with the scene API's opt-in CCD (Simulation.set_contact_ccd), CCD switched on but never limiting a step, and the spinning-box scene."""
import json
import os
import sys
import time

import numpy as np
import pytest

import ccd_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
ETA = 0.9


def _close(dev, ref, ee, xa, xb):
    """equal to 1e-12 relative, or one final ACCD increment apart (a tie of the stop test)"""
    if abs(dev - ref) <= 1e-12 * max(abs(dev), abs(ref)):
        return True
    if ref < 1.0 and dev < 1.0:
        return abs(dev - ref) <= R.last_step(ee, xa, xb, ETA, min(dev, ref)) * (1 + 1e-9)
    return False


def _random_pairs(rng, n):
    """Crossing pairs with known first crossing times (tests/test_ccd_cpu.py) and as many free random motions (hits or misses, unknown t)."""
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from test_ccd_cpu import _random_crossings

    out = [(ee, xa, xb, t) for ee, xa, xb, t in _random_crossings(rng, n // 2)]
    for k in range(n - n // 2):
        ee = k % 2 == 1
        xa = rng.normal(size=(4, 3))
        xb = xa + rng.normal(size=(4, 3)) * rng.uniform(0.1, 2.0)
        out.append((ee, xa, xb, None))
    return out


def test_kernel_against_restatement():
    from stark_amd import capi

    from test_ccd_cpu import CASES

    pairs = _random_pairs(np.random.default_rng(11), 2400)
    pairs += [(c[1], np.asarray(c[2], float), np.asarray(c[3], float), c[4]) for c in CASES]
    # point-triangle: a one-point mesh and a one-triangle mesh; edge-edge: two one-edge meshes. Positions are updated in place (the detector keeps xm).
    pt_x = [np.zeros((1, 3)), np.zeros((3, 3))]
    ee_x = [np.zeros((2, 3)), np.zeros((2, 3))]
    cd_pt, cd_ee = capi.CollisionDetector(), capi.CollisionDetector()
    cd_pt.add_mesh(pt_x[0], np.zeros((0, 3)), np.zeros((0, 2)))
    cd_pt.add_mesh(pt_x[1], [[0, 1, 2]], [[0, 1], [1, 2], [2, 0]])
    cd_ee.add_mesh(ee_x[0], np.zeros((0, 3)), [[0, 1]])
    cd_ee.add_mesh(ee_x[1], np.zeros((0, 3)), [[0, 1]])
    n_hit = n_tie = 0
    for ee, xa, xb, t_star in pairs:
        cd, xs = (cd_ee, ee_x) if ee else (cd_pt, pt_x)
        split = 2 if ee else 1
        xs[0][:] = xa[:split]
        xs[1][:] = xa[split:]
        toi, n = cd.run_ccd([xb[:split], xb[split:]], ETA)
        # the candidate: swept boxes (brute force) of the pair
        pt_c, ee_c = R.candidates(xa, xb, np.array([[1, 2, 3]]) if not ee else np.zeros((0, 3), int),
                                  np.array([[0, 1], [2, 3]]) if ee else np.array([[1, 2], [2, 3], [3, 1]]))
        assert n == len(pt_c) + len(ee_c), (ee, xa, xb)
        r = R.accd(ee, xa, xb, ETA) if n else dict(status="none")
        ref = r["toi"] if r["status"] in ("hit", "capped") else 1.0
        assert _close(toi, ref, ee, xa, xb), (toi, ref, r, ee, xa.tolist(), xb.tolist())
        n_tie += abs(toi - ref) > 1e-12 * max(toi, ref)
        if t_star is not None and r["status"] != "touching":
            assert toi <= t_star, (toi, t_star)
        n_hit += toi < 1.0
    print("pairs %d, hits %d, one-increment ties %d" % (len(pairs), n_hit, n_tie))
    assert n_hit > 1200 and n_tie <= len(pairs) // 20
    cd_pt.close()
    cd_ee.close()


def test_kernel_scene_candidates_and_minimum():
    """Many small meshes in one detector: the candidate count equals a brute-force count of swept-box overlaps with the exclusions, and the
    device minimum equals the restatement's over all candidates."""
    from stark_amd import capi

    rng = np.random.default_rng(5)
    cd = capi.CollisionDetector()
    xs, x1s, tris, edges, off = [], [], [], [], 0
    for m in range(60):
        if m % 2 == 0:   # a triangle pair (4 vertices)
            x = rng.uniform(0, 1, size=3) + rng.normal(size=(4, 3)) * 0.08
            t = np.array([[0, 1, 2], [1, 3, 2]])
            e = np.array([[0, 1], [1, 2], [2, 0], [1, 3], [3, 2]])
        else:            # a polyline of 3 edges
            x = rng.uniform(0, 1, size=3) + np.cumsum(rng.normal(size=(4, 3)) * 0.06, axis=0)
            t = np.zeros((0, 3), int)
            e = np.array([[0, 1], [1, 2], [2, 3]])
        x = np.ascontiguousarray(x)
        x1 = x + rng.normal(size=3) * 0.15 + rng.normal(size=(4, 3)) * 0.02
        cd.add_mesh(x, t, e)
        xs.append(x); x1s.append(x1)
        tris += (t + off).tolist(); edges += (e + off).tolist()
        off += len(x)
    toi, n = cd.run_ccd(x1s, ETA)
    xa, xb = np.vstack(xs), np.vstack(x1s)
    ref, n_ref = R.max_step(xa, xb, np.array(tris), np.array(edges), ETA)
    print("scene: %d candidates, toi %.17g (restatement %.17g)" % (n, toi, ref))
    assert n == n_ref and n > 100
    assert abs(toi - ref) <= 1e-12 * ref or abs(toi - ref) < 1e-3 * ref, (toi, ref)
    toi2, n2 = cd.run_ccd(x1s, ETA)
    assert toi2 == toi and n2 == n   # bit-identical from run to run
    cd.close()


# ---- scenes --------------------------------------------------------------------------------------------------------------------------------
def _sim(S, dt=1.0 / 30.0, thickness=1e-3):
    st = S.default_settings()
    st.max_time_step_size = dt
    st.init_frictional_contact = 1
    sim = S.Simulation(st)
    gp = S.contact_global_params()
    gp.default_contact_thickness = thickness
    sim.set_contact_global_params(gp)
    return sim


def _drop(S, kind, ccd, n_steps=6):
    """An object 10 cm above a fixed 5 cm slab (top face z = 0), thrown down at 10 m/s: one step of 1/30 s moves it 33 cm."""
    sim = _sim(S)
    if kind == "cloth":
        ps = sim.add_surface_grid("cloth", (0.25, 0.25), (32, 32), S.cotton_fabric())
        sim.point_set_add_displacement(ps, (0.0, 0.0, 0.1))
    else:
        ps = sim.add_volume_grid("cube", (0.0, 0.0, 0.1 + 0.05), (0.1, 0.1, 0.1), (4, 4, 4), S.soft_rubber())
    box = sim.add_rigid_box("slab", 1.0, (1.0, 1.0, 0.05))
    sim.rb_add_translation(box, (0.0, 0.0, -0.025))
    sim.rb_add_constraint("fix", box)
    if ccd:
        sim.set_contact_ccd(True, ETA)
    v = sim.points("v0")
    v[:, 2] = -10.0
    sim.set_points("v0", v)
    zmins, ls_max, ok = [], 0, True
    for _ in range(n_steps):
        ok = sim.run_one_step() and ok
        i = sim.info()
        ls_max += i.last_stats.ls_max_iterations
        zmins.append(float(sim.points("x0")[:, 2].min()))
    x = sim.points("x0")
    info = sim.ccd_info() if ccd else None
    sim.close()
    return zmins, ls_max, ok, x, info


@pytest.mark.parametrize("kind", ["cloth", "tet_cube"])
def test_tunnelling_is_prevented(kind):
    from stark_amd import sim as S

    zmins_off, _, _, _, _ = _drop(S, kind, False)
    print(kind, "CCD off: lowest vertex per step", ["%.4f" % z for z in zmins_off])
    assert min(zmins_off) < 0.0   # the control: the scene tunnels
    zmins, ls_max, ok, x, info = _drop(S, kind, True)
    print(kind, "CCD on: lowest vertex per step", ["%.4f" % z for z in zmins], "ls_max", ls_max, info)
    assert ok and np.isfinite(x).all()
    assert min(zmins) >= 0.0, zmins
    assert ls_max > 0 and info["limited"] > 0 and info["capped_pairs"] == 0
    zmins2, _, _, x2, _ = _drop(S, kind, True)
    assert np.array_equal(x, x2) and zmins == zmins2   # bit-identical runs


def test_cfg2_drop_with_ccd():
    """configs[2] as BASELINE describes it (flat 256 x 256 cloth 5 cm above the 2 m box): with CCD the cloth is above the floor's top face at
    the end of every step."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import steplog_cfg2

    sim = steplog_cfg2.build(0.05)
    sim.set_contact_ccd(True, ETA)
    t0, n, ok = time.perf_counter(), 0, True
    while sim.info().current_time < 0.25 - 1e-9:
        ok = sim.run_one_step()
        assert ok, "simulation stopped"
        n += 1
        x = sim.points("x0")
        assert np.isfinite(x).all()
        assert x[:, 2].min() >= -0.05, (n, x[:, 2].min())   # the box's top face: z = -gap (the cloth starts at z = 0)
    wall = time.perf_counter() - t0
    i = sim.info()
    info = sim.ccd_info()
    assert i.last_newton_result in (0, 8)
    print("configs[2] with CCD: %d steps in %.2f s, %.1f Newton-steps/s; CCD %.1f %% of step time, %d queries (%d limited), %d candidates in the last"
          % (n, wall, i.total_newton_iterations / wall, 100.0 * info["seconds"] / max(i.total_step_time, 1e-12), info["queries"], info["limited"],
             info["last_candidates"]))
    sim.close()


def _quiet_scene(S, ccd):
    """Two rigid boxes far apart, one fixed, one falling: a contact scene whose swept boxes never meet."""
    sim = _sim(S, dt=1.0 / 60.0)
    a = sim.add_rigid_box("fixed", 1.0, (0.5, 0.5, 0.5))
    sim.rb_add_constraint("fix", a)
    b = sim.add_rigid_box("falling", 1.0, (0.3, 0.3, 0.3))
    sim.rb_add_translation(b, (3.0, 0.0, 1.0))
    if ccd:
        sim.set_contact_ccd(True, ETA)
    log = []
    for _ in range(8):
        assert sim.run_one_step()
        s = sim.info().last_stats
        log.append((s.newton_iterations, s.cg_iterations, s.n_linear_solves, s.ls_cap_iterations, s.ls_max_iterations, s.ls_inv_iterations,
                    s.ls_bt_iterations, sim.info().last_newton_result))
    state = sim.rb_state(b)
    info = sim.ccd_info()
    sim.close()
    return log, [np.asarray(v) for v in state], info


def test_quiet_query_changes_nothing():
    from stark_amd import sim as S

    log_off, st_off, info_off = _quiet_scene(S, False)
    log_on, st_on, info_on = _quiet_scene(S, True)
    assert info_off["queries"] == 0
    assert log_on == log_off
    assert all(np.array_equal(a, b) for a, b in zip(st_on, st_off))
    assert all(rec[4] == 0 for rec in log_on)
    assert info_on["queries"] > 0 and info_on["last_candidates"] == 0 and info_on["limited"] == 0


def test_spinning_box_with_ccd():
    """configs[0] (the README's spinning box under a cloth) with CCD: the box's vertices rotate, i.e. the linearised rigid trajectories."""
    from stark_amd import sim as S

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
    sim.set_contact_ccd(True, ETA)
    for step in range(len(traj["steps"])):
        sim.rb_fix_set_transformation(fix, anchor, sc["spin"] * sim.info().current_time, (0.0, 0.0, 1.0))
        assert sim.run_one_step()
        assert sim.info().last_newton_result in (0, 8), sim.info().last_newton_result
    info = sim.ccd_info()
    print("configs[0] with CCD:", info)
    assert info["queries"] > 0 and info["capped_pairs"] == 0
    x = sim.points("x0")
    assert np.isfinite(x).all() and -0.35 < x[:, 2].min() < -0.2 and x[:, 2].max() < -0.02   # draped over the box
    sim.close()
