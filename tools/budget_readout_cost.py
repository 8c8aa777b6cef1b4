"""Developer tool: cost of the opt-in budget recording (Simulation.record_budget) — configs[3] at full size (tet block on a box) with record_budget off
and on in the same process: Newton-steps/s for both, readouts launched, and host microseconds of a direct mistark_energies over all potentials and of a
direct mistark_inertia_budget (launches, download of the results).
The off / on pair is repeated (alternating, fresh scene each time) so that the spread between equal runs stands beside the difference.
Kernel times: run this tool with 4 steps and 1 pair under `rocprofv3 --kernel-trace --stats` (no counters in that run) and read k_budget_inertia_chunks,
k_budget_energy_chunks and k_budget_fold beside k_stress_elements in the same trace: the last `on` run ends with one direct element-stress readout of the
tet potential as that yardstick.
usage: python tools/budget_readout_cost.py [steps] [pairs]"""
import ctypes as C
import json
import sys
import time

import numpy as np

sys.path.insert(0, ".")
sys.path.insert(0, "tools")
from bench import build_scene
from stark_amd import capi
from stark_amd import sim as S


def counter(sim, name):
    v = C.c_int64()
    assert capi.lib().mistark_get_counter(sim.engine_handle(), name.encode(), C.byref(v)) == 0
    return v.value


def run(sim, steps, record):
    if record:
        sim.record_budget(True)
    assert sim.run_one_step()   # (warm-up: first-step allocations)
    i0, r0 = sim.info(), counter(sim, "budget_readouts")
    t0 = time.perf_counter()
    for _ in range(steps):
        assert sim.run_one_step()
    wall = time.perf_counter() - t0
    i = sim.info()
    return (i.total_newton_iterations - i0.total_newton_iterations) / wall, counter(sim, "budget_readouts") - r0, wall / steps


def direct(sim, reps=10):
    """host microseconds of one mistark_energies over all potentials and one mistark_inertia_budget, at the simulation's current state"""
    L, h = capi.lib(), sim.engine_handle()
    n = L.mistark_describe(h, None, 0)
    buf = C.create_string_buffer(int(n))
    L.mistark_describe(h, buf, n)
    pots = json.loads(buf.value.decode())["potentials"]
    (pid,) = [k for k, p in enumerate(pots) if p["name"] == "EnergyLumpedInertia"]
    n_groups = len([o for o in sim.budget()["objects"] if o["kind"] == "deformable"])
    E = np.zeros(len(pots))
    rec = np.zeros((n_groups, 13))
    about = np.zeros(3)
    calls = (("mistark_energies over %d potentials, %d elements" % (len(pots), sum(p["n_elem"] for p in pots)), lambda: L.mistark_energies(h, None, 0, E.ctypes.data)),
             ("mistark_inertia_budget of %d items in %d groups" % (pots[pid]["n_elem"], n_groups), lambda: L.mistark_inertia_budget(h, pid, about.ctypes.data, n_groups, rec.ctypes.data)))
    out = []
    for what, call in calls:
        assert call() == 0
        t0 = time.perf_counter()
        for _ in range(reps):
            assert call() == 0
        out.append((what, 1e6 * (time.perf_counter() - t0) / reps))
    # the kernel trace's yardstick: one element-stress readout of the tet potential
    (tid,) = [k for k, p in enumerate(pots) if p["name"].startswith("EnergyTetStrain") and p["n_elem"] > 0]
    ne, kind = C.c_int64(), C.c_int32()
    srec = np.zeros((pots[tid]["n_elem"], 16))
    assert L.mistark_potential_element_stress(h, tid, srec.ctypes.data, C.byref(ne), C.byref(kind)) == 0
    return out, counter(sim, "budget_chunks")


steps = int(sys.argv[1]) if len(sys.argv) > 1 else 4
pairs = int(sys.argv[2]) if len(sys.argv) > 2 else 2
res = {False: [], True: []}
for k in range(pairs):
    for record in (False, True):
        sim = build_scene(S, 44, 44, 43, 0)
        rate, n_readouts, step_s = run(sim, steps, record)
        res[record].append(step_s)
        print("configs[3] budget recording %s: %.1f Newton-steps/s, %.3f ms per step, %d readouts launched in %d steps"
              % ("on " if record else "off", rate, 1e3 * step_s, n_readouts, steps), flush=True)
        if record and k == pairs - 1:
            lines, chunks = direct(sim)
            for what, us in lines:
                print("  direct readout, %s: %.1f us host time per call, download included" % (what, us), flush=True)
            print("  chunks of the inertia budget: %d" % chunks, flush=True)
        sim.close()
off, on = res[False], res[True]
print("ms per step off: %s; on: %s; mean difference %.1f us; spread of equal runs %.1f us (off), %.1f us (on)"
      % (["%.3f" % (1e3 * x) for x in off], ["%.3f" % (1e3 * x) for x in on], 1e6 * (sum(on) / len(on) - sum(off) / len(off)),
         1e6 * (max(off) - min(off)), 1e6 * (max(on) - min(on))))
