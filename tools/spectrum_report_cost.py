"""Developer tool: cost of the opt-in Hessian spectrum report on configs[3] at full size (the 44 x 44 x 43 tet block on a box), at the state reached after
a few time steps, in one process on one build. Option lazy_eval is switched off for the measurement: the report's source 0 reads the double element-Hessian
pool, and mistark_project then projects the same pool in place (on the lazy path it would first recompute the blocks it projects).
  * row stage, source 0: host microseconds of mistark_spectrum_potential_report over every potential with elements (the eigenvalue kernels, the chunked
    potential stage and the download of one 10-double record per potential), and of mistark_potential_spectrum_report on the largest potential with its
    records downloaded;
  * against mistark_project(eps, 0, NULL) over ALL elements of the same pools (the matrix is not assembled: the eigen-decompositions and rebuilds alone),
    each after a fresh mistark_eval(P_G_H) that is not timed;
  * source 1 over the same potentials against one mistark_eval(P_G_H) with force_generic = 1;
  * the nodal stage;
  * ms per time step with record_spectrum off and on, in alternating windows of the same simulation.
Kernel times: run this tool with 1 rep under `rocprofv3 --kernel-trace --stats` (no counters in that run) and read the k_spectrum_* kernels beside
k_project_eig_* in the same trace.
usage: python tools/spectrum_report_cost.py [reps] [steps per window] [pairs of windows]"""
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

EPS = 1e-10


def counter(L, h, name):
    v = C.c_int64()
    assert L.mistark_get_counter(h, name.encode(), C.byref(v)) == 0
    return v.value


def timed(call, reps, before=None):
    out = []
    for _ in range(reps + 1):
        if before:
            before()
        t0 = time.perf_counter()
        assert call() == 0
        out.append(1e6 * (time.perf_counter() - t0))
    return out[1:]          # (the first call allocates)


def window(sim, steps, record):
    sim.record_spectrum(record)
    n0 = sim.info().total_newton_iterations
    t0 = time.perf_counter()
    for _ in range(steps):
        assert sim.run_one_step()
    wall = time.perf_counter() - t0
    return wall / steps, sim.info().total_newton_iterations - n0


reps = int(sys.argv[1]) if len(sys.argv) > 1 else 5
steps = int(sys.argv[2]) if len(sys.argv) > 2 else 3
pairs = int(sys.argv[3]) if len(sys.argv) > 3 else 2
fmt = lambda us: "min %.1f, median %.1f, max %.1f us over %d calls" % (min(us), float(np.median(us)), max(us), len(us))

sim = build_scene(S, 44, 44, 43, 0)
for _ in range(2):
    assert sim.run_one_step()   # (warm-up: first-step allocations)
res = {False: [], True: []}
for k in range(pairs):
    for record in (False, True):
        step_s, newton = window(sim, steps, record)
        res[record].append(step_s)
        print("configs[3] spectrum recording %s: %.3f ms per step (%d Newton iterations in %d steps)" % ("on " if record else "off", 1e3 * step_s, newton, steps), flush=True)
off, on = res[False], res[True]
print("ms per step off: %s; on: %s; mean difference %.1f us; spread of equal windows %.1f us (off), %.1f us (on)"
      % (["%.3f" % (1e3 * x) for x in off], ["%.3f" % (1e3 * x) for x in on], 1e6 * (sum(on) / len(on) - sum(off) / len(off)), 1e6 * (max(off) - min(off)),
         1e6 * (max(on) - min(on))), flush=True)
sim.record_spectrum(False)

L, h = capi.lib(), sim.engine_handle()
n = L.mistark_describe(h, None, 0)
buf = C.create_string_buffer(int(n))
L.mistark_describe(h, buf, n)
pots = json.loads(buf.value.decode())["potentials"]
ids = np.array([k for k, p in enumerate(pots) if p["n_elem"] > 0], dtype=np.int32)
n_elem = sum(pots[k]["n_elem"] for k in ids)
big = int(max(ids, key=lambda k: pots[k]["n_elem"]))
print("%d potentials with elements, %d elements; the largest: '%s', %d elements" % (len(ids), n_elem, pots[big]["name"], pots[big]["n_elem"]), flush=True)
assert L.mistark_set_option(h, b"lazy_eval", 0) == 0
E = C.c_double()
evaluate = lambda: L.mistark_eval(h, capi.EVAL_P_G_H, C.byref(E), None)
out = np.zeros((len(ids), 10))
rec = np.zeros((pots[big]["n_elem"], 10))
cnt, nb = C.c_int64(), C.c_int32()
npj, nch = C.c_int64(), C.c_int64()
nodal = np.zeros((int(L.mistark_ndofs(h)) // 3, 5))
assert evaluate() == 0
us = timed(lambda: L.mistark_spectrum_potential_report(h, ids.ctypes.data, len(ids), 0, EPS, out.ctypes.data), reps)
print("source 0, every potential (rows + potential stage, %d chunks): %s" % (counter(L, h, "spectrum_report_chunks"), fmt(us)), flush=True)
print("  flagged %d of %d elements, %d with lambda_min < 0, smallest lambda_min %.6g, %d not converged, %d non-finite"
      % (out[:, 1].sum(), out[:, 0].sum(), out[:, 2].sum(), out[:, 5].min(), out[:, 4].sum(), out[:, 3].sum()), flush=True)
us = timed(lambda: L.mistark_potential_spectrum_report(h, big, 0, EPS, rec.ctypes.data, None, C.byref(cnt), C.byref(nb)), reps)
print("source 0, '%s' alone, records downloaded (%d x 10 doubles): %s" % (pots[big]["name"], cnt.value, fmt(us)), flush=True)
us = timed(lambda: L.mistark_nodal_spectrum(h, ids.ctypes.data, len(ids), 0, EPS, nodal.ctypes.data), reps)
print("source 0, rows + nodal stage (%d block rows, %d handled by a wavefront), download included: %s" % (len(nodal), counter(L, h, "spectrum_report_long_rows"), fmt(us)), flush=True)
us = timed(lambda: L.mistark_project(h, EPS, 0, None, C.byref(npj), C.byref(nch)), reps, before=evaluate)
print("mistark_project over all elements of the same pools (%d projected, %d changed): %s" % (npj.value, nch.value, fmt(us)), flush=True)
assert L.mistark_set_option(h, b"proj_variant", 8) == 0   # (the full-size kernels for tets and triangles too: the matrices the report diagonalises)
us = timed(lambda: L.mistark_project(h, EPS, 0, None, C.byref(npj), C.byref(nch)), reps, before=evaluate)
print("the same with proj_variant = 8 (no translation-invariant reduction; %d projected, %d changed): %s" % (npj.value, nch.value, fmt(us)), flush=True)
assert L.mistark_set_option(h, b"proj_variant", 0) == 0
us = timed(lambda: L.mistark_spectrum_potential_report(h, ids.ctypes.data, len(ids), 1, EPS, out.ctypes.data), reps)
print("source 1, every potential (evaluation + rows + potential stage): %s" % fmt(us), flush=True)
assert L.mistark_set_option(h, b"force_generic", 1) == 0
us = timed(evaluate, reps)
print("one mistark_eval(P_G_H) with force_generic = 1: %s" % fmt(us), flush=True)
sim.close()
