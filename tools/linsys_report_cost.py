"""Developer tool: cost of the opt-in linear-system report on configs[3] at full size (the 44 x 44 x 43 tet block on a box), on the matrix the last Newton
iteration of a time step left assembled, in one process on one build. For m = 32 and m = 64 and both operators:
  * host microseconds of mistark_linsys_report (the Cholesky of the diagonal blocks, m Lanczos steps with two Gram-Schmidt passes each, one read-back of
    the control block, the tridiagonal eigen solve on the host),
  * the time of m SpMV launches alone (mistark_spmv_bench: HIP events around back-to-back launches on the same matrix),
  * the time of one mistark_pcg solve of the same state at the Newton settings' tolerances, with its iteration count,
  * and of mistark_linsys_modes for the two extreme Ritz vectors with their nodal records (a second run of the same iteration plus two combinations).
usage: python tools/linsys_report_cost.py [reps]"""
import ctypes as C
import sys
import time

import numpy as np

sys.path.insert(0, ".")
sys.path.insert(0, "tools")
from bench import build_scene
from stark_amd import capi
from stark_amd import sim as S


def timed(call, reps):
    out = []
    for _ in range(reps + 1):
        t0 = time.perf_counter()
        assert call() == 0
        out.append(1e6 * (time.perf_counter() - t0))
    return out[1:]          # (the first call allocates)


reps = int(sys.argv[1]) if len(sys.argv) > 1 else 5
fmt = lambda us: "min %.1f, median %.1f, max %.1f us over %d calls" % (min(us), float(np.median(us)), max(us), len(us))

sim = build_scene(S, 44, 44, 43, 0)
for _ in range(3):
    assert sim.run_one_step()
L, h = capi.lib(), sim.engine_handle()
ndofs = int(L.mistark_ndofs(h))
ns = S.default_settings().newton
print("configs[3]: %d unknowns, %d block rows; the matrix of the last Newton iteration of step 3" % (ndofs, ndofs // 3), flush=True)

info = capi.PcgInfo()
du = np.zeros(ndofs)
pcg = lambda: L.mistark_pcg(h, ns.cg_abs_tolerance, ns.cg_rel_tolerance, ns.cg_max_iterations, ns.cg_stop_on_indefiniteness, du.ctypes.data, C.byref(info))
us_pcg = timed(pcg, reps)
print("one mistark_pcg solve (abs %.1e, rel %.1e): %d iterations, converged %d: %s" % (ns.cg_abs_tolerance, ns.cg_rel_tolerance, info.n_iterations, info.converged, fmt(us_pcg)), flush=True)

which = np.array([0, -1], dtype=np.int32)
for m in (32, 64):
    avg = C.c_double()
    assert L.mistark_spmv_bench(h, m, C.byref(avg)) == 0
    print("m = %d: %d SpMV launches alone: %.1f us (%.2f us each)" % (m, m, m * avg.value, avg.value), flush=True)
    for op in (0, 1):
        out, ritz, k = np.zeros(16), np.zeros((m, 2)), C.c_int32()
        us = timed(lambda: L.mistark_linsys_report(h, op, m, None, out.ctypes.data, ritz.ctypes.data, None, C.byref(k)), reps)
        print("m = %d op %d: mistark_linsys_report: %s" % (m, op, fmt(us)), flush=True)
        print("    k %d flags %d theta %.6g (rho %.2e) .. %.6g (rho %.2e) condition %.6g T_norm %.6g, %d Ritz values converged, diagonal blocks not PD %d, smallest pivot %.6g"
              % (out[0], out[1], out[2], out[3], out[4], out[5], out[6], out[7], out[10], out[11], out[13]), flush=True)
        print("    against one PCG solve (median): %.2f x" % (float(np.median(us)) / float(np.median(us_pcg))), flush=True)
        mode, nodal = np.zeros((2, 4)), np.zeros((2, ndofs // 3, 4))
        us = timed(lambda: L.mistark_linsys_modes(h, op, m, None, which.ctypes.data, 2, None, nodal.ctypes.data, mode.ctypes.data), max(reps // 2, 1))
        print("m = %d op %d: mistark_linsys_modes, the two extreme vectors with nodal records: %s" % (m, op, fmt(us)), flush=True)
        print("    measured residuals %.2e, %.2e; largest shares on rows %d (%.3f), %d (%.3f)"
              % (mode[0, 2], mode[1, 2], int(np.argmax(nodal[0, :, 0])), nodal[0, :, 0].max(), int(np.argmax(nodal[1, :, 0])), nodal[1, :, 0].max()), flush=True)
sim.close()
