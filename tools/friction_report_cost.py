"""Developer tool: cost of the opt-in friction recording (Simulation.record_friction) — configs[3] at full size (tet block on a box) with record_friction
off and on in the same process: Newton-steps/s for both, reports launched, and host microseconds of the three direct accessors (launches, download of
the results). The off / on pair is repeated (alternating, fresh scene each time) so that the spread between equal runs stands beside the difference; the
"off" runs are the behaviour without the feature.
Raw lines go to <out>/friction_report_cost.txt. With --kernel-stats the tool then starts `rocprofv3 --kernel-trace --stats` (no counters) on a run of its
own with 4 steps and 1 pair and writes the per-kernel table (profiles/summarize_rocpd.py) to <out>/friction_report_kernel_stats.txt: k_fr_rows,
k_fr_vertex_init, k_fr_vertex_segsum and k_fr_pairs beside the step's own kernels.
usage: python tools/friction_report_cost.py [steps] [pairs] [--out DIR (default: profiles)] [--kernel-stats]"""
import ctypes as C
import glob
import os
import subprocess
import sys
import tempfile
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
        sim.record_friction(True)
    assert sim.run_one_step()   # (warm-up: first-step allocations)
    i0, r0 = sim.info(), counter(sim, "friction_reports")
    t0 = time.perf_counter()
    for _ in range(steps):
        assert sim.run_one_step()
    wall = time.perf_counter() - t0
    i = sim.info()
    return (i.total_newton_iterations - i0.total_newton_iterations) / wall, counter(sim, "friction_reports") - r0, wall / steps


def direct(sim, reps=10):
    """host microseconds of one call of each accessor at the simulation's current state"""
    L, h = capi.lib(), sim.engine_handle()
    n, nv, g = C.c_int64(), C.c_int64(), C.c_int32()
    assert L.mistark_contact_friction_report(h, None, None, C.byref(n)) == 0
    assert L.mistark_contact_friction_vertex_report(h, None, None, None, C.byref(nv)) == 0
    assert L.mistark_contact_friction_pair_report(h, None, C.byref(g)) == 0
    ri, rd = np.zeros((max(n.value, 1), 8), dtype=np.int32), np.zeros((max(n.value, 1), 24))
    vert, pairs = np.zeros((max(nv.value, 1), 8)), np.zeros((max(g.value, 1), max(g.value, 1), 12))
    calls = (("mistark_contact_friction_report of %d rows" % n.value, lambda: L.mistark_contact_friction_report(h, ri.ctypes.data, rd.ctypes.data, C.byref(n))),
             ("mistark_contact_friction_vertex_report of %d collision vertices" % nv.value, lambda: L.mistark_contact_friction_vertex_report(h, vert.ctypes.data, None, None, C.byref(nv))),
             ("mistark_contact_friction_pair_report of %d groups" % g.value, lambda: L.mistark_contact_friction_pair_report(h, pairs.ctypes.data, C.byref(g))))
    out = []
    for what, call in calls:
        assert call() == 0
        t0 = time.perf_counter()
        for _ in range(reps):
            assert call() == 0
        out.append((what, 1e6 * (time.perf_counter() - t0) / reps))
    return out, counter(sim, "friction_report_long_rows")


def main(steps, pairs, say):
    res = {False: [], True: []}
    for k in range(pairs):
        for record in (False, True):
            sim = build_scene(S, 44, 44, 43, 0)
            rate, n_reports, step_s = run(sim, steps, record)
            res[record].append(step_s)
            say("configs[3] friction recording %s: %.1f Newton-steps/s, %.3f ms per step, %d reports launched in %d steps" % ("on " if record else "off", rate, 1e3 * step_s, n_reports, steps))
            if record and k == pairs - 1:
                lines, long_rows = direct(sim)
                for what, us in lines:
                    say("  direct readout, %s: %.1f us host time per call, download included" % (what, us))
                say("  vertices of the last report summed by a wavefront: %d" % long_rows)
            sim.close()
    off, on = res[False], res[True]
    say("ms per step off: %s; on: %s; mean difference %.1f us; spread of equal runs %.1f us (off), %.1f us (on)"
        % (["%.3f" % (1e3 * x) for x in off], ["%.3f" % (1e3 * x) for x in on], 1e6 * (sum(on) / len(on) - sum(off) / len(off)), 1e6 * (max(off) - min(off)),
           1e6 * (max(on) - min(on))))


if __name__ == "__main__":
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    out_dir = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else "profiles"
    args = [a for a in args if a != out_dir]
    steps = int(args[0]) if len(args) > 0 else 4
    pairs = int(args[1]) if len(args) > 1 else 2
    if "--traced" in sys.argv:  # the run under the profiler: no files of its own
        main(steps, pairs, lambda line: print(line, flush=True))
        sys.exit(0)
    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, "friction_report_cost.txt"), "w") as f:
        f.write("# python tools/friction_report_cost.py %d %d\n" % (steps, pairs))

        def say(line):
            print(line, flush=True)
            f.write(line + "\n")
            f.flush()

        main(steps, pairs, say)
    if "--kernel-stats" in sys.argv:
        tmp = tempfile.mkdtemp(prefix="friction_report_trace_")
        subprocess.run(["rocprofv3", "--kernel-trace", "--stats", "-d", tmp, "-o", "r", "--", sys.executable, "tools/friction_report_cost.py", "4", "1", "--traced"], check=True, timeout=600)
        dbs = glob.glob(os.path.join(tmp, "**", "*.db"), recursive=True)
        assert dbs, "the profiler wrote no database under " + tmp
        table = subprocess.run([sys.executable, "profiles/summarize_rocpd.py", dbs[0]], check=True, capture_output=True, text=True).stdout
        with open(os.path.join(out_dir, "friction_report_kernel_stats.txt"), "w") as f:
            f.write("# rocprofv3 --kernel-trace --stats -- python tools/friction_report_cost.py 4 1\n" + table)
        print(table[:4000])
