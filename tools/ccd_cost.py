"""Developer tool: cost of the opt-in CCD (Simulation.set_contact_ccd) — configs[3] at full size (tet block on a box) with CCD off and on in
the same process, and the configs[2] 5 cm cloth drop with CCD on: Newton-steps/s, CCD queries, seconds per query, candidates per query.
usage: python tools/ccd_cost.py [steps]"""
import sys
import time

sys.path.insert(0, ".")
sys.path.insert(0, "tools")
from bench import build_scene
from stark_amd import sim as S


def run(sim, steps, ccd):
    if ccd:
        sim.set_contact_ccd(True, 0.9)
    assert sim.run_one_step()   # (warm-up: first-step allocations)
    i0 = sim.info()
    c0 = sim.ccd_info()
    t0 = time.perf_counter()
    cands = []
    for _ in range(steps):
        assert sim.run_one_step()
        cands.append(sim.ccd_info()["last_candidates"])
    wall = time.perf_counter() - t0
    i, c = sim.info(), sim.ccd_info()
    its = i.total_newton_iterations - i0.total_newton_iterations
    q = c["queries"] - c0["queries"]
    per_q = (c["seconds"] - c0["seconds"]) / q if q else 0.0
    return its / wall, q, per_q, (sum(cands) / len(cands) if ccd else 0), c["limited"] - c0["limited"]


steps = int(sys.argv[1]) if len(sys.argv) > 1 else 4
for name, make in (("configs[3]", lambda: build_scene(S, 44, 44, 43, 0)),):
    for ccd in (False, True):
        sim = make()
        rate, q, per_q, cand, lim = run(sim, steps, ccd)
        print("%s CCD %s: %.1f Newton-steps/s, %d queries (%d limited), %.1f us per query, %.0f candidates per query"
              % (name, "on " if ccd else "off", rate, q, lim, 1e6 * per_q, cand), flush=True)
        sim.close()
import steplog_cfg2

sim = steplog_cfg2.build(0.05)
rate, q, per_q, cand, lim = run(sim, steps, True)
print("configs[2] 5 cm drop CCD on : %.1f Newton-steps/s, %d queries (%d limited), %.1f us per query, %.0f candidates per query" % (rate, q, lim, 1e6 * per_q, cand))
sim.close()
