"""Developer tool: cost of the opt-in force recording (Simulation.record_forces) — configs[3] at full size (tet block on a box) with
record_forces(["contact_", "friction_"]) off and on in the same process: Newton-steps/s for both, readouts launched, and host microseconds of a
readout of the same two groups called directly (mistark_forces: launches, download of the nodal vector and the wait for it).
The off / on pair is repeated (alternating, fresh scene each time) so that the spread between equal runs stands beside the difference.
usage: python tools/force_readout_cost.py [steps] [pairs]"""
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

GROUPS = ["contact_", "friction_"]


def counter(sim, name):
    v = C.c_int64()
    assert capi.lib().mistark_get_counter(sim.engine_handle(), name.encode(), C.byref(v)) == 0
    return v.value


def run(sim, steps, record):
    if record:
        sim.record_forces(GROUPS)
    assert sim.run_one_step()   # (warm-up: first-step allocations)
    i0, r0 = sim.info(), counter(sim, "force_readouts")
    t0 = time.perf_counter()
    for _ in range(steps):
        assert sim.run_one_step()
    wall = time.perf_counter() - t0
    i = sim.info()
    return (i.total_newton_iterations - i0.total_newton_iterations) / wall, counter(sim, "force_readouts") - r0, wall / steps


def direct(sim, reps=20):
    """host microseconds of one mistark_forces call per group, at the simulation's current state"""
    L, h = capi.lib(), sim.engine_handle()
    n = L.mistark_describe(h, None, 0)
    buf = C.create_string_buffer(int(n))
    L.mistark_describe(h, buf, n)
    pots = json.loads(buf.value.decode())["potentials"]
    f = np.zeros(int(L.mistark_ndofs(h)))
    out = []
    for g in GROUPS:
        ids = np.array([k for k, p in enumerate(pots) if p["name"].startswith(g)], dtype=np.int32)
        rows = sum(pots[k]["n_elem"] for k in ids)
        L.mistark_forces(h, ids.ctypes.data, len(ids), 1.0, f.ctypes.data)
        t0 = time.perf_counter()
        for _ in range(reps):
            assert L.mistark_forces(h, ids.ctypes.data, len(ids), 1.0, f.ctypes.data) == 0
        out.append((g, len(ids), rows, 1e6 * (time.perf_counter() - t0) / reps))
    return out


steps = int(sys.argv[1]) if len(sys.argv) > 1 else 4
pairs = int(sys.argv[2]) if len(sys.argv) > 2 else 2
res = {False: [], True: []}
for k in range(pairs):
    for record in (False, True):
        sim = build_scene(S, 44, 44, 43, 0)
        rate, n_readouts, step_s = run(sim, steps, record)
        res[record].append(step_s)
        print("configs[3] force recording %s: %.1f Newton-steps/s, %.3f ms per step, %d readouts launched in %d steps"
              % ("on " if record else "off", rate, 1e3 * step_s, n_readouts, steps), flush=True)
        if record and k == pairs - 1:
            for g, n_pots, rows, us in direct(sim):
                print("  direct readout of '%s' (%d tables, %d rows): %.1f us host time per call, download included" % (g, n_pots, rows, us), flush=True)
        sim.close()
off, on = res[False], res[True]
print("ms per step off: %s; on: %s; mean difference %.1f us for %d groups; spread of equal runs %.1f us (off), %.1f us (on)"
      % (["%.3f" % (1e3 * x) for x in off], ["%.3f" % (1e3 * x) for x in on], 1e6 * (sum(on) / len(on) - sum(off) / len(off)), len(GROUPS),
         1e6 * (max(off) - min(off)), 1e6 * (max(on) - min(on))))
