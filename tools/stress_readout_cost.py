"""Developer tool: cost of the opt-in stress recording (Simulation.record_stress) — configs[3] at full size (tet block on a box) with record_stress off
and on in the same process: Newton-steps/s for both, readouts launched, and host microseconds of a direct element readout of the tet potential
(mistark_potential_element_stress: launch, download of the 16-double records, transposition) and of a direct nodal readout (mistark_nodal_stress).
The off / on pair is repeated (alternating, fresh scene each time) so that the spread between equal runs stands beside the difference.
Kernel times: run this tool with 4 steps and 1 pair under `rocprofv3 --kernel-trace --stats` (no counters in that run) and read k_stress_elements
beside k_eval_tet_closed in the same trace.
usage: python tools/stress_readout_cost.py [steps] [pairs]"""
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
        sim.record_stress(True)
    assert sim.run_one_step()   # (warm-up: first-step allocations)
    i0, r0 = sim.info(), counter(sim, "stress_readouts")
    t0 = time.perf_counter()
    for _ in range(steps):
        assert sim.run_one_step()
    wall = time.perf_counter() - t0
    i = sim.info()
    return (i.total_newton_iterations - i0.total_newton_iterations) / wall, counter(sim, "stress_readouts") - r0, wall / steps


def direct(sim, reps=10):
    """host microseconds of one element readout and one nodal readout of the tet potential, at the simulation's current state"""
    L, h = capi.lib(), sim.engine_handle()
    n = L.mistark_describe(h, None, 0)
    buf = C.create_string_buffer(int(n))
    L.mistark_describe(h, buf, n)
    pots = json.loads(buf.value.decode())["potentials"]
    (pid,) = [k for k, p in enumerate(pots) if p["name"].startswith("EnergyTetStrain") and p["n_elem"] > 0]
    ne, kind = C.c_int64(), C.c_int32()
    rec = np.zeros((pots[pid]["n_elem"], 16))
    nodal = np.zeros((int(L.mistark_ndofs(h)) // 3, 10))
    ids = np.array([pid], dtype=np.int32)
    calls = (("element records", lambda: L.mistark_potential_element_stress(h, pid, rec.ctypes.data, C.byref(ne), C.byref(kind))),
             ("nodal averages", lambda: L.mistark_nodal_stress(h, ids.ctypes.data, 1, nodal.ctypes.data)))
    out = []
    for what, call in calls:
        assert call() == 0
        t0 = time.perf_counter()
        for _ in range(reps):
            assert call() == 0
        out.append((what, pots[pid]["name"], pots[pid]["n_elem"], 1e6 * (time.perf_counter() - t0) / reps))
    return out, counter(sim, "stress_long_rows")


steps = int(sys.argv[1]) if len(sys.argv) > 1 else 4
pairs = int(sys.argv[2]) if len(sys.argv) > 2 else 2
res = {False: [], True: []}
for k in range(pairs):
    for record in (False, True):
        sim = build_scene(S, 44, 44, 43, 0)
        rate, n_readouts, step_s = run(sim, steps, record)
        res[record].append(step_s)
        print("configs[3] stress recording %s: %.1f Newton-steps/s, %.3f ms per step, %d readouts launched in %d steps"
              % ("on " if record else "off", rate, 1e3 * step_s, n_readouts, steps), flush=True)
        if record and k == pairs - 1:
            lines, long_rows = direct(sim)
            for what, name, n_elem, us in lines:
                print("  direct readout, %s of '%s' (%d elements): %.1f us host time per call, download included" % (what, name, n_elem, us), flush=True)
            print("  rows of the nodal readout summed by a wavefront: %d" % long_rows, flush=True)
        sim.close()
off, on = res[False], res[True]
print("ms per step off: %s; on: %s; mean difference %.1f us; spread of equal runs %.1f us (off), %.1f us (on)"
      % (["%.3f" % (1e3 * x) for x in off], ["%.3f" % (1e3 * x) for x in on], 1e6 * (sum(on) / len(on) - sum(off) / len(off)),
         1e6 * (max(off) - min(off)), 1e6 * (max(on) - min(on))))
