"""Bending report on the GPU (include/mistark.h "bending report", include/mistark_sim.h "bending recording"): the device rows against the g++ build of the
same header (tests/host_bending_report) and the numpy restatement of tests/bending_ref.py, the nodal and group stages against numpy sums in the device's
order, the engine's own energies, reproducibility, isolation from eval(), the host mirror and the refusals.

Tolerances: rows as tests/test_bending_cpu.py holds the host build to the restatement (bending_ref's docstring: 1e-11 relative to the largest reference
value of a field over the potential, theta1 within 1e-11 + 16 * 2.2e-16 / sin(theta_ref) per hinge and carried linearly through what is computed from it);
two evaluations of the header (device, host) are held to each other within twice that. Sums within 1e-12 * the sum of |terms| of the entry; counts, maxima
and the arg-max exactly."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bending_ref as br  # noqa: E402
from test_bending_cpu import THRESHOLDS, host_lib, host_records  # noqa: E402,F401

LONG_ROW = 256   # BEND_LONG_ROW of csrc/bending_report.hip
CHUNK = 2048     # BEND_CHUNK


def _engine(prob, man=None, **kw):
    from gpu_util import engine_from_problem

    return engine_from_problem(prob, man, **kw)


def _pid(eng, prob, name):
    (pid,) = [p for pi, p in eng.pot_ids.items() if prob.potentials[pi].name == name]
    return pid


def _cases(name):
    prob, rec, bound, extra = br.seeded_hinges(name)
    gprob, gpot, grec, gbound = br.golden_problem(name)
    return [("seeded " + name, prob, prob.potentials[0], rec, bound), ("golden " + name, gprob, gpot, grec, gbound)]


# ---- 1. rows ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", br.NAMES)
def test_rows_equal_the_host_build_and_the_restatement(host_lib, name):
    for what, prob, pot, rec, bound in _cases(name):
        eng = _engine(prob)
        pid = _pid(eng, prob, name)
        n, kind = C.c_int64(-1), C.c_int32(-1)
        assert eng.L.mistark_potential_bending_report(eng.h, pid, None, 0, None, C.byref(n), C.byref(kind)) == 0     # the size query
        assert n.value == len(rec) and kind.value == br.KIND[name]
        assert eng.counter("bending_reports") == 0                       # ... launches nothing
        got = eng.bending_report(pid)
        assert got["kind"] == br.KIND[name] and got["name"] == name and got["records"].shape == (len(rec), 16)
        assert eng.counter("bending_reports") == 1
        br.check_records(got["records"], rec, bound, what + " device")
        host = host_records(host_lib, prob, pot)
        d = np.abs(got["records"] - host)
        d[:, 1] = np.minimum(d[:, 1], 2.0 * np.pi - d[:, 1])
        print("%s: device against the host build: worst error / (2 bound) %.3g" % (what, (d[:, :14] / np.maximum(2.0 * bound[:, :14], 1e-300)).max()))
        assert (d[:, :14] <= 2.0 * bound[:, :14]).all() and np.array_equal(got["records"][:, 14:], host[:, 14:])
        eng.close()


@pytest.mark.parametrize("name", br.NAMES)
def test_thresholds_flag_rows_and_groups(host_lib, name):
    prob, rec0, bound0, extra = br.seeded_hinges(name)
    pot = prob.potentials[0]
    rec, bound = br.records(prob, pot, THRESHOLDS)
    out = br.undecided(rec, bound, THRESHOLDS)
    assert out.sum() <= 0.02 * len(rec)
    eng = _engine(prob)
    pid = eng.pot_ids[0]
    got = eng.bending_report(pid, THRESHOLDS)
    br.check_records(got["records"], rec, bound, name, THRESHOLDS)
    assert got["beyond_threshold"].any() and not got["beyond_threshold"].all()
    grp = eng.bending_group_report(pid, 3, THRESHOLDS)
    want, _ = br.group_records(got["records"], 3)          # (counts of the device's own flags: exact)
    assert np.array_equal(grp[:, :3], want[:, :3])
    ref, _ = br.group_records(rec, 3)
    assert (np.abs(grp[:, 2] - ref[:, 2]) <= out.sum()).all()
    assert not eng.bending_report(pid)["beyond_threshold"].any()     # no thresholds: nothing is flagged
    eng.close()


@pytest.mark.parametrize("n", [1, 255, 256, 257])
def test_grid_tails(n):
    """Rows that do not exist are not written: on the host (guard words around the caller's buffer) and on the device, where the two potentials of a
    nodal report share one field-major record buffer and a lane past the end of one would land in the other's columns or in the next field."""
    for name in br.NAMES:
        prob0, rec0, bound0, extra = br.seeded_hinges(name)
        p0 = prob0.potentials[0]
        other = [m for m in br.NAMES if m != name][0]
        pa = br.ev.PotentialDesc(name, np.ascontiguousarray(p0.conn[:n]), p0.bindings)
        qprob, qrec, qbound, _ = br.seeded_hinges(other)
        # the other kind on the remaining hinges: its tables appended to the arrays, the same node arrays
        arrays = list(prob0.arrays)
        bs = []
        for b in qprob.potentials[0].bindings:
            if b.array <= 1:
                bs.append(b)
            else:
                arrays.append(qprob.arrays[b.array])
                bs.append(br.ev.Binding(len(arrays) - 1, b.stride, b.conn, b.dof_set))
        pb = br.ev.PotentialDesc(other, np.ascontiguousarray(p0.conn[n:]), bs)
        prob = br.ev.Problem(dt=prob0.dt, ndofs=prob0.ndofs, dof_offsets=prob0.dof_offsets, dof_sizes=prob0.dof_sizes, arrays=arrays, potentials=[pa, pb], dof_arrays=prob0.dof_arrays)
        eng = _engine(prob)
        guard = 0x7FF8DEADBEEF0001
        buf = np.full(16 * (n + 2), guard, dtype=np.uint64)
        cnt, kind = C.c_int64(), C.c_int32()
        assert eng.L.mistark_potential_bending_report(eng.h, eng.pot_ids[0], None, 0, buf.ctypes.data + 16 * 8, C.byref(cnt), C.byref(kind)) == 0
        assert cnt.value == n and (buf[:16] == guard).all() and (buf[-16:] == guard).all() and not (buf[16:-16] == guard).any()
        ref, bnd = br.records(prob, pa)
        br.check_records(buf[16:-16].view(np.float64).reshape(n, 16), ref, bnd, "%s n=%d" % (name, n))
        rows = [eng.bending_report(eng.pot_ids[i])["records"] for i in (0, 1)]
        br.check_records(rows[1], *br.records(prob, pb), "%s behind %s n=%d" % (other, name, n))
        want, mag = br.nodal(len(arrays[1]), [(br.block_rows(prob, p), r) for p, r in zip(prob.potentials, rows)])   # of the device's own rows
        out = eng.nodal_bending([eng.pot_ids[0], eng.pot_ids[1]])
        assert (np.abs(out - want) <= 1e-12 * mag).all() and out[:, 4].sum() == 2 * len(p0.conn)
        eng.close()


# ---- 2. nodal stage ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [3, 64, 65, LONG_ROW - 1, LONG_ROW, LONG_ROW + 1, 300])
def test_nodal_records_on_fans(n):
    """A closed fan of n triangles about one vertex: n hinges end at the centre node, beyond 256 the long-row path sums them. Both potentials listed
    together: the even hinges are complete, the odd ones flat."""
    X, hinges = br.fan(n)
    X = np.concatenate([X, [[1.0, 1.0, 1.0]]])                      # a point no hinge touches
    rng = np.random.default_rng(n)
    x1 = X + 0.004 * rng.uniform(-1.0, 1.0, X.shape)
    x0 = x1 + 0.0005 * rng.uniform(-1.0, 1.0, X.shape)
    rest = br.hinge_rest_data(X, hinges)
    pick = lambda sel: {k: v[sel] for k, v in rest.items()}
    ev_, od = np.arange(n) % 2 == 0, np.arange(n) % 2 == 1
    parts = [("EnergyDiscreteShells", hinges[ev_], np.zeros(ev_.sum(), dtype=int), pick(ev_), dict(scale=[1.0], k=[2e-3], damping=[1e-4]))]
    if od.any():
        parts.append(("EnergyBendingFlat", hinges[od], np.zeros(od.sum(), dtype=int), pick(od), dict(k=[2e-3])))
    prob = br.make_problem(parts, x0, (x1 - x0) / br.DT)
    eng = _engine(prob)
    pids = [eng.pot_ids[i] for i in range(len(parts))]
    rows = [eng.bending_report(p)["records"] for p in pids]
    for r, p in zip(rows, prob.potentials):
        ref, bound = br.records(prob, p)
        br.check_records(r, ref, bound, "fan %d %s" % (n, p.name))
        assert not (r[:, 15].astype(int) & 1).any()
    before = eng.counter("bending_reports")
    out = eng.nodal_bending(pids)
    assert eng.counter("bending_reports") == before + 1
    assert out.shape == (len(X), 6)
    want, mag = br.nodal(len(X), [(br.block_rows(prob, p), r) for p, r in zip(prob.potentials, rows)])    # of the device's own rows, in the device's order
    worst = (np.abs(out - want) / np.maximum(mag, 1e-300))[:, [0, 1, 2, 5]].max()
    print("fan of %d: worst |difference| / sum|terms| = %.3g" % (n, worst))
    assert (np.abs(out - want) <= 1e-12 * mag).all()
    assert np.array_equal(out[:, 3:5], want[:, 3:5])                 # the maximum and the count: exact
    assert out[0, 4] == n and (out[1:-1, 4] == 1.0).all()
    assert eng.counter("bending_report_long_rows") == (1 if n > LONG_ROW else 0)
    assert (out[-1] == 0.0).all()                                    # untouched rows: six exact zeros
    E_rows = sum((r[:, 9] + r[:, 10]).sum() for r in rows)
    assert abs(out[:, 2].sum() - E_rows) <= 1e-12 * sum(np.abs(r[:, 9:11]).sum() for r in rows)
    assert np.array_equal(out, eng.nodal_bending(pids))
    eng.close()


# ---- 3. group stage ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", br.NAMES)
def test_groups_across_the_chunk_edge(name):
    """A 32 x 32 cloth: 3008 hinges, 2968 of group 0, so its list crosses the 2048-row chunk edge; a second group of 40; a declared empty group. Four
    copies of one sharp hinge (nodes of their own at the same positions: the same bits) sit in the first and in the second chunk of group 0 and twice in
    group 1: the arg-max is the first of them in each list."""
    prob0, hinges0 = br.cloth(name, 32, small_group=40)
    p0 = prob0.potentials[0]
    n0, nn = len(hinges0), len(prob0.arrays[1])
    assert n0 - 40 > CHUNK
    # the sharp hinge: a fold of 2.5 rad, sharper than anything in the wavy cloth; rest data of the flat stencil
    one = lambda v: np.array([v])
    sharp = br.fold(one(0.1), one(0.05), one(0.06), one(0.03), one(0.07), one(2.5))[0]
    flat = br.fold(one(0.1), one(0.05), one(0.06), one(0.03), one(0.07), one(0.0))[0]
    x0 = np.concatenate([prob0.arrays[1]] + [sharp] * 4)
    v1 = np.concatenate([prob0.arrays[0], np.zeros((16, 3))])
    local = np.arange(16).reshape(4, 4)
    # the table: 100 cloth rows, copy A, the rest of group 0, copy B | group 1: 5 cloth rows, copy C, 35 cloth rows, copy D
    order = np.concatenate([np.arange(100), [n0], np.arange(100, n0 - 40), [n0 + 1], np.arange(n0 - 40, n0 - 35), [n0 + 2], np.arange(n0 - 35, n0), [n0 + 3]])
    A, B, Cc, D = 100, n0 - 39, n0 - 33, n0 + 3
    assert (np.nonzero(order >= n0)[0] == np.array([A, B, Cc, D])).all() and B > CHUNK
    hinges = np.concatenate([hinges0, nn + local])[order]
    group = np.concatenate([p0.conn[:, 1], [0, 0, 1, 1]])[order]
    rest0, rest1 = br.hinge_rest_data(_rest_positions(32), hinges0), br.hinge_rest_data(np.concatenate([flat] * 4), local)
    rest = {k: np.concatenate([rest0[k], rest1[k]])[order] for k in rest0}
    prob = br.make_problem([(name, hinges, group, rest, br.GROUP_PARAMS[name])], x0, v1)
    pot = prob.potentials[0]
    eng = _engine(prob)
    pid = eng.pot_ids[0]
    rows = eng.bending_report(pid)["records"]
    ref, bound = br.records(prob, pot)
    br.check_records(rows, ref, bound, "cloth " + name)
    grp = eng.bending_group_report(pid, 3)
    assert eng.counter("bending_report_chunks") == 3               # two of group 0, one of group 1
    want, mag = br.group_records(rows, 3)                          # of the device's own rows, in table order
    assert np.array_equal(grp[:, :5], want[:, :5])                 # counts, the maximum and the arg-max: exact
    assert grp[0, 0] == n0 - 40 + 2 and grp[1, 0] == 42 and grp[2, 4] == -1.0 and (grp[2, [0, 1, 2, 3, 5, 6, 7, 8, 9]] == 0.0).all()
    dev = br.deviation(rows)
    assert dev[A] == dev[B] == dev[Cc] == dev[D] == dev.max()      # the copies tie, bit for bit
    assert grp[0, 4] == A and grp[1, 4] == 5 and grp[0, 3] == dev.max() == grp[1, 3]
    worst = (np.abs(grp - want) / np.maximum(mag, 1e-300))[:, 5:].max()
    print("%s: group sums, worst |difference| / sum|terms| = %.3g" % (name, worst))
    assert (np.abs(grp - want) <= 1e-12 * mag).all()
    E = eng.energies([pid])[0]
    assert abs(grp[:, 5].sum() + grp[:, 6].sum() - E) <= 1e-12 * np.abs(rows[:, 9:11]).sum()
    assert np.array_equal(grp, eng.bending_group_report(pid, 3))
    eng.close()


def _rest_positions(n):
    import stress_ref as sr

    return sr.tri_grid(n, n, 0.8 / n)[0]


# ---- 4. leaves everything else alone -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", br.NAMES)
def test_report_is_reproducible_and_leaves_the_evaluation_alone(name):
    from oracle import evaluator as ev
    from stark_amd import capi

    def sequence(report):
        prob, man, z = ev.load_fixture(os.path.join(br.GOLDEN, br.FIXTURES[name]))
        eng = _engine(prob, man)
        pid = _pid(eng, prob, name)
        ng = int(br.groups_of([p for p in prob.potentials if p.name == name][0]).max()) + 1

        def read():
            return [eng.bending_report(pid, np.full(ng, 0.01))["records"], eng.nodal_bending([pid]), eng.bending_group_report(pid, ng, np.full(ng, 0.01))]

        E0, g0 = eng.eval(capi.EVAL_P_G_H)
        first = read() if report else None
        E1, g1 = eng.eval(capi.EVAL_P_G_H)
        if report:
            for a, b in zip(first, read()):
                assert np.array_equal(a, b)               # two reports of one state: the same bits
            assert eng.counter("bending_reports") == 6
        else:
            assert eng.counter("bending_reports") == 0
        assert E0 == E1 and np.array_equal(g0, g1)        # a report between two eval() calls
        eng.assemble()
        bsr = eng.get_bsr()
        eng.close()
        return E1, g1, bsr

    Ea, ga, (rpa, ca, va) = sequence(False)
    Eb, gb, (rpb, cb, vb) = sequence(True)
    assert Ea == Eb and np.array_equal(ga, gb)
    assert np.array_equal(rpa, rpb) and np.array_equal(ca, cb) and np.array_equal(va, vb)


def _hanging_cloth(record, flat_rest_angle=1):
    from stark_amd import sim as S

    st = S.default_settings()
    st.max_time_step_size = 0.01
    st.init_frictional_contact = 0
    sim = S.Simulation(st)
    params = S.cotton_fabric()
    params.flat_rest_angle = flat_rest_angle
    cloth = sim.add_surface_grid("cloth", (0.4, 0.4), (8, 8), params)
    sim.prescribe_inside_aabb(cloth, (-0.2, 0.0, 0.0), (2e-3, 2.0, 2.0), 1e7)     # one edge clamped: the sheet bends under its weight
    if record is not None:
        sim.record_bending(record, 0.02)
    return sim


def _counter(sim, name):
    from stark_amd import capi

    v = C.c_int64()
    assert capi.lib().mistark_get_counter(sim.engine_handle(), name.encode(), C.byref(v)) == 0
    return v.value


@pytest.mark.parametrize("flat_rest_angle", [1, 0])
def test_recording_does_not_change_the_trajectory(flat_rest_angle):
    from stark_amd import sim as S

    name = br.NAMES[flat_rest_angle]

    def run(record):
        sim = _hanging_cloth(record, flat_rest_angle)
        if record:
            with pytest.raises(S.SimError, match="no time step has been accepted"):
                sim.bending()
        else:
            with pytest.raises(S.SimError, match="recording is off"):
                sim.bending()
        for _ in range(5):
            assert sim.run_one_step()
        out = sim.points("x0"), sim.points("v0"), _counter(sim, "bending_reports")
        rep = sim.bending() if record else None
        sim.close()
        return out, rep

    (x_off, v_off, r_off), _ = run(False)
    (x_on, v_on, r_on), rep = run(True)
    assert r_off == 0 and r_on == 5
    assert np.array_equal(x_on, x_off) and np.array_equal(v_on, v_off)
    assert list(rep["kinds"]) == [name]
    rows, groups, nodal = rep["kinds"][name]["rows"], rep["kinds"][name]["groups"], rep["nodal"]
    n_hinges = 3 * 8 * 8 - 2 * 8
    assert rows["records"].shape == (n_hinges, 16) and groups.shape == (1, 10) and nodal.shape == (81, 6)
    assert rows["kind"] == flat_rest_angle and not rows["degenerate"].any() and (rows["group"] == 0).all()
    assert groups[0, 0] == n_hinges and groups[0, 2] == rows["beyond_threshold"].sum() and groups[0, 3] == br.deviation(rows["records"]).max() > 0.0
    E = (rows["E_elastic"] + rows["E_damping"]).sum()
    assert abs(groups[0, 5] + groups[0, 6] - E) <= 1e-12 * np.abs(rows["records"][:, 9:11]).sum()
    assert abs(nodal[:, 2].sum() - E) <= 1e-12 * np.abs(rows["records"][:, 9:11]).sum()
    assert nodal[:, 4].sum() == 2 * n_hinges and (nodal[:, 5] > 0.0).all()
    assert abs(rep["time"] - 0.05) < 1e-12


def test_switching_recording_off_refuses_the_getter():
    from stark_amd import sim as S

    sim = _hanging_cloth(True)
    assert sim.run_one_step()
    assert sim.bending()["kinds"]
    sim.record_bending(False)
    with pytest.raises(S.SimError, match="recording is off"):
        sim.bending()
    with pytest.raises(S.SimError, match="negative or not finite"):
        sim.record_bending(True, -1.0)
    sim.close()


# ---- 5. refusals -------------------------------------------------------------------------------------------------------------------------------
def test_other_potentials_bad_ids_groups_and_thresholds_are_refused():
    import stark_amd
    from oracle import evaluator as ev

    Err = stark_amd.engine.EngineError
    prob, man, z = ev.load_fixture(os.path.join(br.GOLDEN, br.FIXTURES["EnergyBendingFlat"]))
    eng = _engine(prob, man)
    names = {p: prob.potentials[pi].name for pi, p in eng.pot_ids.items()}
    other = [p for p, n in names.items() if n not in br.KIND]
    assert other
    for p in other:
        for call in (lambda: eng.bending_report(p), lambda: eng.nodal_bending([p]), lambda: eng.bending_group_report(p, 1)):
            with pytest.raises(Err, match=names[p]) as e:
                call()
            assert "has no bending report" in str(e.value)
    pid = [p for p, n in names.items() if n == "EnergyBendingFlat"][0]
    for call in (lambda: eng.bending_report(len(names) + 5), lambda: eng.bending_group_report(-1, 1), lambda: eng.nodal_bending([pid, 99])):
        with pytest.raises(Err, match="bad potential id"):
            call()
    with pytest.raises(Err, match="listed twice"):
        eng.nodal_bending([pid, pid])
    assert eng.counter("bending_reports") == 0
    ng = int(eng.bending_report(pid)["group"].max()) + 1
    for call in (lambda: eng.bending_group_report(pid, ng - 1), lambda: eng.bending_report(pid, np.ones(ng + 1), ng - 1)):
        with pytest.raises(Err, match="names group") as e:
            call()
        assert "n_groups is %d" % (ng - 1) in str(e.value)
    for bad in (-1.0, np.inf, np.nan):
        thr = np.ones(ng)
        thr[ng - 1] = bad
        for call in (lambda: eng.bending_report(pid, thr), lambda: eng.bending_group_report(pid, ng, thr)):
            with pytest.raises(Err, match="negative or not finite"):
                call()
    assert eng.counter("bending_reports") == 1   # (the one report that read the group ids)
    eng.close()
    # user-defined potentials
    eng = _engine(prob, man, custom_ops=z)
    pid = _pid(eng, prob, "EnergyBendingFlat")
    for call in (lambda: eng.bending_report(pid), lambda: eng.nodal_bending([pid]), lambda: eng.bending_group_report(pid, 1)):
        with pytest.raises(Err, match="user-defined"):
            call()
    assert eng.counter("bending_reports") == 0
    eng.close()


def test_sharded_and_registration_only_contexts_are_refused():
    import stark_amd
    from stark_amd import capi

    L = capi.lib()
    group = L.mistark_local_group_create(2)
    try:
        eng = stark_amd.Engine(0)
        eng.dist_init_local(group, 0)
        u = np.zeros(6)
        eng.add_dof_set("u", u)
        for call in (lambda: eng.bending_report(0), lambda: eng.nodal_bending([0]), lambda: eng.bending_group_report(0, 1)):
            with pytest.raises(stark_amd.engine.EngineError, match="single-rank"):
                call()
        eng.close()
    finally:
        L.mistark_local_group_destroy(group)
    h = C.c_void_p()
    assert L.mistark_create_dry(C.byref(h)) == 0
    try:
        n, kind = C.c_int64(), C.c_int32()
        assert L.mistark_potential_bending_report(h, 0, None, 0, None, C.byref(n), C.byref(kind)) < 0
        assert "registration-only" in L.mistark_last_error(h).decode()
    finally:
        L.mistark_destroy(h)
