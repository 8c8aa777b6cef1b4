"""Developer tool: cost of the opt-in constraint recording (Simulation.record_constraints) — the README beam at 52 x 13 x 13 with its clamped face, in ONE
process and one scene: windows of `steps` accepted steps alternate between recording off and on (the scene keeps running, so both modes see the same
drift of the state), and the medians of the per-step wall times of the two modes stand beside the spread of equal windows. run_one_step ends in device
synchronisations (the Newton loop's read-backs), so a host clock around it measures finished work. Then the host microseconds of a direct
mistark_potential_constraint_report and mistark_constraint_group_report of the clamp's potential (launches and download of the results).
Kernel times: run this tool with `2 2` under `rocprofv3 --kernel-trace --stats` (a run of its own, no counters) and read k_constraint_rows,
k_constraint_group_chunks and k_constraint_group_fold in the trace.
The yardstick beside it: the budget readout's recorded 0.75 ms per step on configs[3] (profiles/budget_readout_cost.txt).
usage: python tools/constraint_report_cost.py [steps per window] [windows per mode]"""
import ctypes as C
import json
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, ".")
from stark_amd import capi
from stark_amd import sim as S


def counter(sim, name):
    v = C.c_int64()
    assert capi.lib().mistark_get_counter(sim.engine_handle(), name.encode(), C.byref(v)) == 0
    return v.value


def window(sim, steps):
    """wall seconds of every accepted step of a window"""
    out = []
    while len(out) < steps:
        t_before = sim.info().current_time
        t0 = time.perf_counter()
        assert sim.run_one_step()
        dt = time.perf_counter() - t0
        if sim.info().current_time > t_before:
            out.append(dt)
    return out


def direct(sim, reps=20):
    L, h = capi.lib(), sim.engine_handle()
    n = L.mistark_describe(h, None, 0)
    buf = C.create_string_buffer(int(n))
    L.mistark_describe(h, buf, n)
    pots = json.loads(buf.value.decode())["potentials"]
    (pid,) = [k for k, p in enumerate(pots) if p["name"] == "EnergyPrescribedPositions"]
    rows = pots[pid]["n_elem"]
    rec, aux, ids = np.zeros((rows, 16)), np.zeros((rows, 2)), np.zeros((rows, 4), dtype=np.int32)
    grp, about, tol = np.zeros((1, 12)), np.zeros(3), np.array([1e-3])
    nr, kind = C.c_int64(), C.c_int32()
    calls = (("mistark_potential_constraint_report of %d rows" % rows,
              lambda: L.mistark_potential_constraint_report(h, pid, tol.ctypes.data, 1, rec.ctypes.data, aux.ctypes.data, ids.ctypes.data, C.byref(nr), C.byref(kind))),
             ("mistark_constraint_group_report of %d rows in 1 group" % rows, lambda: L.mistark_constraint_group_report(h, pid, tol.ctypes.data, 1, about.ctypes.data, grp.ctypes.data)))
    out = []
    for what, call in calls:
        assert call() == 0
        t0 = time.perf_counter()
        for _ in range(reps):
            assert call() == 0
        out.append((what, 1e6 * (time.perf_counter() - t0) / reps))
    return out, counter(sim, "constraint_report_chunks"), grp[0]


steps = int(sys.argv[1]) if len(sys.argv) > 1 else 5
windows = int(sys.argv[2]) if len(sys.argv) > 2 else 4
sim = S.Simulation(S.default_settings())
beam = sim.add_volume_grid("beam", (0, 0, 0), (1.0, 0.25, 0.25), (52, 13, 13), S.soft_rubber())
sim.prescribe_inside_aabb(beam, (-0.5, 0, 0), (2e-3, 2, 2), 1e7)
window(sim, 2)   # (warm-up: first-step allocations)
sim.record_constraints(True)
window(sim, 1)   # (... and the report's)
times = {False: [], True: []}
medians = {False: [], True: []}
for k in range(windows):
    for record in (False, True):
        sim.record_constraints(record)
        r0 = counter(sim, "constraint_reports")
        t = window(sim, steps)
        times[record] += t
        medians[record].append(statistics.median(t))
        print("beam 52x13x13 constraint recording %s: median %.3f ms per step over %d steps, %d reports launched"
              % ("on " if record else "off", 1e3 * medians[record][-1], steps, counter(sim, "constraint_reports") - r0), flush=True)
off, on = statistics.median(times[False]), statistics.median(times[True])
print("median ms per step off: %.3f; on: %.3f; difference %.1f us; spread of the window medians %.1f us (off), %.1f us (on)"
      % (1e3 * off, 1e3 * on, 1e6 * (on - off), 1e6 * (max(medians[False]) - min(medians[False])), 1e6 * (max(medians[True]) - min(medians[True]))), flush=True)
sim.record_constraints(True)
window(sim, 1)
lines, chunks, grp = direct(sim)
for what, us in lines:
    print("  direct call, %s: %.1f us host time per call, download included" % (what, us), flush=True)
print("  chunks of the group report: %d; rows %d, largest violation %.3e m, resultant %s N" % (chunks, int(grp[0]), grp[3], np.array2string(grp[5:8], precision=4)), flush=True)
print("yardstick: the budget readout's recorded 0.75 ms per step on configs[3] (profiles/budget_readout_cost.txt)")
sim.close()
