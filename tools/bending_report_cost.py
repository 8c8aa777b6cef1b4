"""Developer tool: cost of the opt-in bending report — a 256 x 256 cloth (196 096 hinges) clamped along one edge and bending under its weight, for both
bending models (flat_rest_angle on: EnergyBendingFlat, the preset's default; off: EnergyDiscreteShells). The sheet is 12.8 m wide, a node spacing of
0.05 m: at 1 m its nodes are so light that every step was seen to converge without a Newton iteration and the sheet stayed flat, which leaves nothing
to compare with. Per model, in one process on one build:
  * ms per time step and per Newton iteration with record_bending off and on, in alternating windows of the same simulation (the recording is the three
    stages on the device, nothing downloaded), so that the spread between equal windows stands beside the difference;
  * host microseconds of the three direct calls at the state reached (mistark_potential_bending_report: rows, download of the 16-double records and
    transposition included; mistark_nodal_bending; mistark_bending_group_report), against one Newton iteration of the same scene.
Kernel times: run this tool with 2 steps and 1 pair under `rocprofv3 --kernel-trace --stats` (no counters in that run) and read the k_bending_* kernels
beside the step's own in the same trace.
usage: python tools/bending_report_cost.py [steps per window] [pairs of windows]"""
import ctypes as C
import json
import sys
import time

import numpy as np

sys.path.insert(0, ".")
from stark_amd import capi
from stark_amd import sim as S

N = 256
SIZE = 12.8


def counter(sim, name):
    v = C.c_int64()
    assert capi.lib().mistark_get_counter(sim.engine_handle(), name.encode(), C.byref(v)) == 0
    return v.value


def build(flat_rest_angle):
    st = S.default_settings()
    st.max_time_step_size = 0.01
    st.mirror_state_to_host = 0
    st.init_frictional_contact = 0
    sim = S.Simulation(st)
    p = S.cotton_fabric()
    p.flat_rest_angle = flat_rest_angle
    cloth = sim.add_surface_grid("cloth", (SIZE, SIZE), (N, N), p)
    sim.prescribe_inside_aabb(cloth, (-0.5 * SIZE, 0.0, 0.0), (2e-3, 2.0 * SIZE, 2.0), 1e7)
    return sim


def window(sim, steps, record):
    sim.record_bending(record)
    i0, r0 = sim.info(), counter(sim, "bending_reports")
    t0 = time.perf_counter()
    for _ in range(steps):
        assert sim.run_one_step()
    wall = time.perf_counter() - t0
    newton = sim.info().total_newton_iterations - i0.total_newton_iterations
    return wall / steps, (wall / newton if newton else float("nan")), newton, counter(sim, "bending_reports") - r0


def direct(sim, name, reps=10):
    """host microseconds of the three direct calls on the bending potential, at the simulation's current state"""
    L, h = capi.lib(), sim.engine_handle()
    n = L.mistark_describe(h, None, 0)
    buf = C.create_string_buffer(int(n))
    L.mistark_describe(h, buf, n)
    pots = json.loads(buf.value.decode())["potentials"]
    (pid,) = [k for k, p in enumerate(pots) if p["name"] == name and p["n_elem"] > 0]
    n_rows = pots[pid]["n_elem"]
    cnt, kind = C.c_int64(), C.c_int32()
    rec, nodal, grp = np.zeros((n_rows, 16)), np.zeros((int(L.mistark_ndofs(h)) // 3, 6)), np.zeros((1, 10))
    ids = np.array([pid], dtype=np.int32)
    thr = np.array([0.05])
    calls = (("rows", lambda: L.mistark_potential_bending_report(h, pid, thr.ctypes.data, 1, rec.ctypes.data, C.byref(cnt), C.byref(kind))),
             ("nodal records", lambda: L.mistark_nodal_bending(h, ids.ctypes.data, 1, nodal.ctypes.data)),
             ("group records", lambda: L.mistark_bending_group_report(h, pid, thr.ctypes.data, 1, grp.ctypes.data)))
    out = []
    for what, call in calls:
        assert call() == 0
        t0 = time.perf_counter()
        for _ in range(reps):
            assert call() == 0
        out.append((what, 1e6 * (time.perf_counter() - t0) / reps))
    return n_rows, out, rec, grp, counter(sim, "bending_report_long_rows"), counter(sim, "bending_report_chunks")


steps = int(sys.argv[1]) if len(sys.argv) > 1 else 6
pairs = int(sys.argv[2]) if len(sys.argv) > 2 else 3
for flat, name in ((1, "EnergyBendingFlat"), (0, "EnergyDiscreteShells")):
    sim = build(flat)
    for _ in range(2):
        assert sim.run_one_step()   # (warm-up: first-step allocations)
    res = {False: [], True: []}
    per_newton = []
    for k in range(pairs):
        for record in (False, True):
            step_s, newton_s, newton, launched = window(sim, steps, record)
            res[record].append(step_s)
            if not record:
                per_newton.append(newton_s)
            print("256 x 256 cloth, %s, bending recording %s: %.3f ms per step, %.3f ms per Newton iteration (%d in %d steps), %d report stages launched"
                  % (name, "on " if record else "off", 1e3 * step_s, 1e3 * newton_s, newton, steps, launched), flush=True)
    off, on = res[False], res[True]
    print("  ms per step off: %s; on: %s; mean difference %.1f us; spread of equal windows %.1f us (off), %.1f us (on)"
          % (["%.3f" % (1e3 * x) for x in off], ["%.3f" % (1e3 * x) for x in on], 1e6 * (sum(on) / len(on) - sum(off) / len(off)), 1e6 * (max(off) - min(off)),
             1e6 * (max(on) - min(on))), flush=True)
    n_rows, lines, rec, grp, long_rows, chunks = direct(sim, name)
    it_us = 1e6 * sum(per_newton) / len(per_newton)
    for what, us in lines:
        print("  direct call, %s of '%s' (%d hinges): %.1f us host time per call, download included = %.3f of one Newton iteration (%.1f us)"
              % (what, name, n_rows, us, us / it_us, it_us), flush=True)
    print("  state: largest |theta1 - rest| %.4f rad, %d hinges beyond 0.05 rad, bending energy %.6g J; rows of the nodal stage summed by a wavefront: %d; chunks of the group stage: %d"
          % (grp[0, 3], int(grp[0, 2]), grp[0, 5] + grp[0, 6], long_rows, chunks), flush=True)
    sim.close()
