"""Developer tool: cost of the opt-in wrench recording (Simulation.record_wrench) and of direct calls of the rigid-body wrench report, in ONE process.
1. The rbchain scene (9 boxes, all 13 rigid-body potentials; tests/wrench_ref.py rbchain_scene): windows of `steps` accepted steps alternate between
   recording off and on (the scene keeps running, so both modes see the same drift of the state), and the medians of the per-step wall times of the two
   modes stand beside the spread of equal windows. run_one_step ends in device synchronisations (the Newton loop's read-backs), so a host clock around
   it measures finished work. A recorded step runs one body report of seven families and reads the time step back once (one stream synchronisation).
2. Host time of direct calls (mistark_potential_rigid_wrench, mistark_rigid_wrench), launches and download of the results included: on the contactmix
   fixture (3 bodies, 20 rigid potentials, a few hundred rows) and on a synthesised star of one body attached to N deformable points
   (tests/wrench_ref.py star_problem), whose two rows take the force readout's long-row path. Beside every figure stands the same call repeated in a
   second window, as the spread; mistark_forces of the same selection is timed as the yardstick (the report's nodal stage is that call's).
Kernel times: run this tool under `rocprofv3 --kernel-trace --stats` (a run of its own, no counters) and read k_wrench_rows, k_wrench_bodies,
k_wrench_long_rows and k_force_segsum in the trace.
usage: python tools/wrench_report_cost.py [points of the star] [calls per window] [steps per window] [windows per mode]"""
import ctypes as C
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import wrench_ref as wr  # noqa: E402
from oracle import evaluator as ev  # noqa: E402
from stark_amd import capi  # noqa: E402
from stark_amd import sim as S  # noqa: E402


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


def is_rigid(prob, R, k):
    return any(b.dof_set in (R.set_v, R.set_w) for b in prob.potentials[k].bindings)


def timed(call, reps):
    call()
    out = []
    for _ in range(2):
        t0 = time.perf_counter()
        for _ in range(reps):
            call()
        out.append(1e6 * (time.perf_counter() - t0) / reps)
    return out


def report(what, us):
    print("%s: %.1f us host time per call (second window %.1f us), download included" % (what, us[0], us[1]), flush=True)


n_star = int(sys.argv[1]) if len(sys.argv) > 1 else 20000
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 20
steps = int(sys.argv[3]) if len(sys.argv) > 3 else 10
windows = int(sys.argv[4]) if len(sys.argv) > 4 else 4

sim = wr.rbchain_scene(S)
window(sim, 2)   # (warm-up: first-step allocations)
sim.record_wrench(True)
window(sim, 1)   # (... and the report's)
times = {False: [], True: []}
medians = {False: [], True: []}
for k in range(windows):
    for record in (False, True):
        sim.record_wrench(record)
        r0 = counter(sim, "wrench_reports")
        t = window(sim, steps)
        times[record] += t
        medians[record].append(statistics.median(t))
        print("rbchain wrench recording %s: median %.3f ms per step over %d steps, %d reports launched"
              % ("on " if record else "off", 1e3 * medians[record][-1], steps, counter(sim, "wrench_reports") - r0), flush=True)
off, on = statistics.median(times[False]), statistics.median(times[True])
print("median ms per step off: %.3f; on: %.3f; difference %.1f us; spread of the window medians %.1f us (off), %.1f us (on)"
      % (1e3 * off, 1e3 * on, 1e6 * (on - off), 1e6 * (max(medians[False]) - min(medians[False])), 1e6 * (max(medians[True]) - min(medians[True]))), flush=True)
sim.record_wrench(True)
window(sim, 1)
t0 = time.perf_counter()
for _ in range(reps):
    rep = sim.wrench()
print("  Simulation.wrench() of %d bodies: %.1f us host time per call, download included" % (len(rep["labels"]), 1e6 * (time.perf_counter() - t0) / reps), flush=True)
sim.close()

prob, man, _ = ev.load_fixture(os.path.join(ROOT, "tests", "golden", "contactmix_t0.npz"))
R = wr.Rigid(prob)
eng, ids = wr.engine_of(prob, man, R)
pids = [pid for k, pid in sorted(eng.pot_ids.items())]
rigid = [eng.pot_ids[k] for k in sorted(eng.pot_ids) if is_rigid(prob, R, k)]
rows = sum(len(prob.potentials[k].conn) for k in eng.pot_ids if is_rigid(prob, R, k))
report("contactmix, rows of the %d rigid potentials (%d rows), one call each" % (len(rigid), rows), timed(lambda: [eng.rigid_wrench_rows(p, **ids) for p in rigid], reps))
report("contactmix, bodies, the family of all %d potentials" % len(pids), timed(lambda: eng.rigid_wrench([[]], **ids), reps))
seven = [pids[i::6] for i in range(6)] + [[]]
report("contactmix, bodies, seven families (a partition into six, and all)", timed(lambda: eng.rigid_wrench(seven, **ids), reps))
report("contactmix, yardstick: mistark_forces of all potentials", timed(lambda: eng.forces(None, 1.0 / prob.dt), reps))
eng.close()

prob, R, att = wr.star_problem(n_star, 1)
eng, ids = wr.engine_of(prob, None, R)
pid = eng.pot_ids[0]
report("star of %d attachments, rows" % n_star, timed(lambda: eng.rigid_wrench_rows(pid, **ids), reps))
report("star of %d attachments, bodies, one family" % n_star, timed(lambda: eng.rigid_wrench([[pid]], **ids), reps))
print("  rows a whole wavefront summed: %d" % eng.counter("wrench_long_rows"), flush=True)
report("star of %d attachments, yardstick: mistark_forces of the attachments" % n_star, timed(lambda: eng.forces([pid], 1.0 / prob.dt), reps))
eng.close()
