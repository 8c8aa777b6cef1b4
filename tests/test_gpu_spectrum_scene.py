"""GPU (-m gpu): spectrum recording of the scene mirror (Simulation.record_spectrum): a tet beam at the settings of the recorded trajectory
traj_tetbeam_big_projected (ProjectedNewton on a beam whose first steps hold inverted and indefinite elements) for 3 steps, with and without recording.
The step logs are `==`, the end state is the same bits, and what spectrum() / spectrum_rows() return after the last step is, bit for bit, what the
engine-level source 1 reports give at that state."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_gpu_scene import _load  # noqa: E402

pytestmark = pytest.mark.gpu

FIXTURE = "traj_tetbeam_big_projected"


def _beam(record):
    from stark_amd import capi
    from stark_amd import sim as S

    z, traj, man = _load(FIXTURE)
    sc = traj["scene"]
    args = dict(kv.split("=") for kv in bytes(z["harness_args"]).decode().split()[2:])
    assert args.get("projection") == "ProjectedNewton"
    st = S.default_settings()
    st.init_frictional_contact = 0
    sim = S.Simulation(st)
    p = S.soft_rubber()
    p.elasticity_only = sc["eo"]
    ps = sim.add_volume_grid("beam", (0, 0, 0), (sc["lx"], sc["ly"], sc["lz"]), (sc["nx"], sc["ny"], sc["nz"]), p)
    sim.prescribe_inside_aabb(ps, (-0.5 * sc["lx"], 0, 0), (2e-3, 2 * sc["ly"], 2 * sc["lz"]), 1e7)
    ns = S.default_settings().newton
    ns.projection_mode = capi.PROJ_PROJECTED_NEWTON
    sim.set_newton_settings(ns)
    v = sim.points("v0")
    i = np.arange(v.shape[0])[:, None]
    d = np.arange(3)[None, :]
    sim.set_points("v0", float(args["vamp"]) * np.sin(1.3 * (3.0 * i + d) + 0.7))
    if record is not None:
        sim.record_spectrum(record)
    return sim, traj, ns.projection_eps


def _log(sim):
    i = sim.info()
    out = [i.current_time, i.last_stats.newton_iterations, i.last_stats.n_linear_solves, i.last_stats.cg_iterations]
    for r in sim.newton_iteration_log():
        out.append((int(r.logged), int(r.n_projected_hessians), int(r.cg_iterations_last), int(r.line_search), int(r.ls_cap), int(r.ls_max), int(r.ls_inv), int(r.ls_bt)))
    return out


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def test_recording_changes_no_bit_and_equals_the_engine_level_report():
    from stark_amd import capi
    from stark_amd import sim as S

    start = [None, None]                                       # x0, v0 at the start of the last step

    def run(record):
        sim, traj, eps = _beam(record)
        for call in (sim.spectrum, lambda: sim.spectrum_rows("EnergyTetStrain")):
            with pytest.raises(S.SimError, match="no time step has been accepted" if record else "recording is off"):
                call()
        logs = []
        for ref in traj["steps"][:3]:
            start[:] = [sim.points("x0"), sim.points("v0")]
            sim.run_one_step()
            logs.append(_log(sim))
            assert abs(logs[-1][0] - ref["time"]) < 1e-12 and (logs[-1][1], logs[-1][2]) == (ref["newton"], ref["linear_solves"])   # (the reference's own log)
        return sim, logs, (sim.points("x0"), sim.points("v0")), eps

    sim, logs_off, end_off, _ = run(None)
    sim.close()
    sim, logs_on, end_on, eps = run(True)
    assert len(logs_on) == 3 and logs_on == logs_off
    assert (_bits(end_on[0]) == _bits(end_off[0])).all() and (_bits(end_on[1]) == _bits(end_off[1])).all()
    rep = sim.spectrum()
    n = len(rep["names"])
    assert n > 0 and rep["eps"] == eps and abs(rep["time"] - logs_on[-1][0]) < 1e-12
    assert rep["potentials"].shape == (n, 10) and rep["nodal"].shape == (sim.info().n_points, 5)
    tets = [k for k, name in enumerate(rep["names"]) if name.startswith("EnergyTetStrain")]
    assert tets and rep["potentials"][tets, 0].sum() > 0
    print("recorded: %s; elements %s, flagged %s, lambda_min %s" % (rep["names"], rep["potentials"][:, 0], rep["potentials"][:, 1], rep["potentials"][:, 5]))
    # the engine-level reports at the state the step converged at: the same potentials (every one of the scene is built-in), the same source and eps.
    # Accepting the step moved x0 <- x0 + dt v1 and v0 <- v1 behind the recording; the DoFs v1 and dt are still the step's, so putting x0 and v0 of the
    # step's start back gives the engine the state the Newton solve converged at.
    sim.set_points("x0", start[0])
    sim.set_points("v0", start[1])
    L, h = capi.lib(), sim.engine_handle()
    ids = np.arange(n, dtype=np.int32)
    pots = np.zeros((n, 10))
    assert L.mistark_spectrum_potential_report(h, ids.ctypes.data, n, 1, eps, pots.ctypes.data) == 0, L.mistark_last_error(h)
    ndofs = L.mistark_ndofs(h)
    nodal = np.zeros((ndofs // 3, 5))
    assert L.mistark_nodal_spectrum(h, ids.ctypes.data, n, 1, eps, nodal.ctypes.data) == 0, L.mistark_last_error(h)
    assert (_bits(pots) == _bits(rep["potentials"])).all()
    assert nodal.shape == rep["nodal"].shape                  # (the points are the scene's only DoFs: no rigid body)
    assert (_bits(nodal) == _bits(rep["nodal"])).all()
    for k, name in enumerate(rep["names"]):
        ne, nb = C.c_int64(), C.c_int32()
        assert L.mistark_potential_spectrum_report(h, k, 1, eps, None, None, C.byref(ne), C.byref(nb)) == 0
        rec = np.zeros((ne.value, 10))
        if ne.value:
            assert L.mistark_potential_spectrum_report(h, k, 1, eps, rec.ctypes.data, None, C.byref(ne), C.byref(nb)) == 0
        rows = sim.spectrum_rows(name)
        assert rows["records"].shape == rec.shape and (_bits(rows["records"]) == _bits(rec)).all(), name
        assert pots[k, 0] == ne.value and pots[k, 1] == (rec[:, 9].astype(int) & 1).sum()
    with pytest.raises(S.SimError, match="no recorded potential"):
        sim.spectrum_rows("no_such_potential")
    sim.record_spectrum(False)
    with pytest.raises(S.SimError, match="recording is off"):
        sim.spectrum()
    with pytest.raises(S.SimError, match="not finite"):
        sim.record_spectrum(True, float("nan"))
    sim.close()
