"""Developer tool: cost of the curved rigid mode of the opt-in CCD (Simulation.set_contact_ccd_rigid) — the configs[0] scene (spinning box under a cloth:
the pads are live) and configs[3] at full size (fixed box: every pad is zero, so this is the overhead of the padded kernels alone), linear against
curved, alternating twice in one process: Newton-steps/s, host time per query, rounds histogram; on configs[0] also max_step(curved) / max_step(linear)
over the queries of a curved run (both asked at every line search through a second callback).
usage: python tools/ccd_curved_cost.py [steps of configs[3]]"""
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, ".")
sys.path.insert(0, "tools")
from bench import build_scene
from stark_amd import capi
from stark_amd import sim as S

ETA = 0.9


def spinning_box():
    z = np.load(os.path.join("tests", "golden", "traj_cfg0_spinning_box_cloth_32.npz"))
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
    return sim, lambda: sim.rb_fix_set_transformation(fix, anchor, sc["spin"] * sim.info().current_time, (0.0, 0.0, 1.0)), len(traj["steps"])


def run(sim, before_step, steps, mode, warmup=1, probe=False):
    sim.set_contact_ccd(True, ETA)
    sim.set_contact_ccd_rigid(mode, 4)
    ratios, hist = [], {}
    if probe:   # both modes at every line search, beside the simulation's own query
        L, r = capi.lib(), capi.CcdResult()

        def ask():
            h = sim.engine_handle()
            step = sim.info().dt
            out = []
            for m in (0, 1):
                assert L.mistark_contact_max_step_ex(h, step, ETA, m, 4, None, C.byref(r)) == 0
                out.append(r.max_step)
                if m == 1:
                    hist[int(r.rounds)] = hist.get(int(r.rounds), 0) + 1
            if out[0] > 0.0:
                ratios.append(out[1] / out[0])
            return 1.0

        sim.add_max_allowed_step(ask)
    for _ in range(warmup):
        before_step()
        assert sim.run_one_step()
    i0, c0, r0 = sim.info(), sim.ccd_info(), sim.ccd_rigid_info()
    t0 = time.perf_counter()
    for _ in range(steps):
        before_step()
        assert sim.run_one_step()
    wall = time.perf_counter() - t0
    i, c, r1 = sim.info(), sim.ccd_info(), sim.ccd_rigid_info()
    q = c["queries"] - c0["queries"]
    return dict(rate=(i.total_newton_iterations - i0.total_newton_iterations) / wall, queries=q, limited=c["limited"] - c0["limited"],
                us_per_query=1e6 * (c["seconds"] - c0["seconds"]) / max(q, 1), rounds=r1["rounds"] - r0["rounds"], pad_bound=r1["pad_bound_pairs"], max_pad=r1["max_pad"],
                candidates=c["last_candidates"], ratios=ratios, hist=hist)


def line(name, mode, k, r):
    print("%s %-6s run %d: %.1f Newton-steps/s, %d queries (%d limited), %d rounds, %.1f us per query, %d candidates in the last, largest pad %.3g, %d pad-bound pairs left"
          % (name, mode, k, r["rate"], r["queries"], r["limited"], r["rounds"], r["us_per_query"], r["candidates"], r["max_pad"], r["pad_bound"]), flush=True)


steps3 = int(sys.argv[1]) if len(sys.argv) > 1 else 4
for k in (1, 2):
    for mode in ("linear", "curved"):
        sim, before, n = spinning_box()
        line("configs[0]", mode, k, run(sim, before, n - 1, mode))
        sim.close()
sim, before, n = spinning_box()
r = run(sim, before, n - 1, "curved", probe=True)
sim.close()
q = np.array(r["ratios"])
print("configs[0] curved, both modes asked at each of its %d line searches: max_step(curved) / max_step(linear) mean %.4f, median %.4f, min %.4f, max %.4f; equal in %d; "
      "rounds histogram %s" % (len(q), q.mean(), np.median(q), q.min(), q.max(), int((q == 1.0).sum()), dict(sorted(r["hist"].items()))), flush=True)
for k in (1, 2):
    for mode in ("linear", "curved"):
        sim = build_scene(S, 44, 44, 43, 0)
        line("configs[3]", mode, k, run(sim, lambda: None, steps3, mode))
        sim.close()
