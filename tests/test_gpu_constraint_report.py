"""Constraint report on the GPU (include/mistark.h "constraint report", include/mistark_sim.h "constraint recording"): the row records of the seventeen
penalty-constraint potentials and their group records against the numpy restatement of tests/constraint_report_ref.py, against the engine's own element
energies and force readout, against the host mirror's constraint handlers, and the refusals.

Tolerances (tests/constraint_report_ref.py): 1e-11 relative to max |reference| of a field over the table for row quantities (+ 4 * 2^-53 / c rad on the
angle of an angle limit), (n + 8) * 2^-53 * sum |terms| for the group sums; the exact family uses ==; the host mirror's handlers reach the same state
through another route of normalised quaternions: 1e-9 relative."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import constraint_report_ref as cr  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
U = cr.U
CHUNK = 2048  # CONSTRAINT_CHUNK of csrc/constraint_report.hip: rows per workgroup
ABOUT = np.array([0.25, -0.5, 0.125])  # (integers / 64)
# group sizes per table; 0: a declared group without rows. Around the wavefront (64 x 4 = 256 threads), around a few strides of 256, around one and two
# chunks; one table with a single row.
TABLES = {
    "small": [1, 255, 256, 0, 257, 1023, 1024, 1025],
    "chunks": [CHUNK - 1, CHUNK, 0, CHUNK + 1, 2 * CHUNK + 1],
    "single": [1],
}
POINT_KINDS = ["EnergyPrescribedPositions", "EnergyAttachments_d_d_p_p"]


def _engine(prob):
    from gpu_util import engine_from_problem

    eng = engine_from_problem(prob)
    return eng, eng.pot_ids[0]


# ---- 1. rows of every kind -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", cr.NAMES)
def test_rows_against_restatement(name):
    prob, tol = cr.seeded_problem(name)
    inp = cr.gather(prob)
    group = prob.potentials[0].conn[:, cr.KINDS[name][1]]
    eng, pid = _engine(prob)
    for t in (None, tol):
        got = eng.constraint_report(pid, t)
        want, want_aux = cr.row_records(name, inp, None if t is None else t[group])
        bound = cr.row_bounds(name, inp, want)
        err = np.abs(got["records"] - want)
        print("%s: worst |difference| / bound %.3g" % (name, float((err[:, :15] / np.maximum(bound[:, :15], 1e-300)).max())))
        assert (err <= bound).all(), np.argwhere(err > bound)[:5]
        assert (np.abs(got["aux"] - want_aux) <= cr.ROW_TOL * np.abs(want_aux).max()).all()
        assert np.array_equal(got["ids"], cr.ids_of(prob, name))
        assert got["kind"] == cr.KINDS[name][0] and got["name"] == name and got["unit"] == cr.KINDS[name][5]
        again = eng.constraint_report(pid, t)   # two reports of one state: the same bits
        assert np.array_equal(again["records"], got["records"]) and np.array_equal(again["aux"], got["aux"]) and np.array_equal(again["ids"], got["ids"])
    assert got["beyond_tolerance"].any() and not got["beyond_tolerance"].all()
    assert eng.counter("constraint_reports") == 4
    eng.close()


# ---- 2. group sums ---------------------------------------------------------------------------------------------------------------------------
def _table(sizes, seed):
    """group[i] of every row: the groups' rows interleaved through the list in a fixed shuffled order."""
    group = np.concatenate([np.full(s, g, dtype=np.int32) for g, s in enumerate(sizes)])
    np.random.default_rng(seed).shuffle(group)
    return group


def _point_problem(name, x0a, v1a, d, k, group, dt, rng, exact):
    """Row i: point a = i at x0a[i] moving with v1a[i]; its partner (the target, or point n + i) sits d[i] away at the end of the step."""
    n = len(group)
    x1 = x0a + dt * v1a
    if name == "EnergyPrescribedPositions":
        return cr.prescribed_problem(x0a, v1a, np.arange(n), x1 + d, k, group, dt)
    v1b = rng.integers(-31, 32, (n, 3)) / 64.0 if exact else rng.standard_normal((n, 3))
    x0b = (x1 + d) - dt * v1b
    return cr.attach_pp_problem(np.concatenate([x0a, x0b]), np.concatenate([v1a, v1b]), np.arange(n), n + np.arange(n), k, group, dt)


def _check_groups(eng, pid, name, group, sizes, tol, rec, exact):
    ng = len(sizes)
    got = eng.constraint_group_report(pid, ng, tol, ABOUT)
    assert eng.counter("constraint_report_chunks") == sum((s + CHUNK - 1) // CHUNK for s in sizes)
    want, mag = cr.group_records(rec, group, ng, ABOUT, False)
    assert np.array_equal(got[:, :5], want[:, :5])   # counts, the maximum and its position: exact by nature
    assert (got[:, 0] == sizes).all()
    for g, s in enumerate(sizes):
        if s == 0:   # a declared group without rows: zeros with -1
            assert (np.delete(got[g], 4) == 0.0).all() and got[g, 4] == -1.0
    if exact:
        assert np.array_equal(got, want), np.argwhere(got != want)
    else:
        bound = (np.asarray(sizes)[:, None] + 8) * U * mag
        print("%s: worst |difference| / bound %.3g" % (name, float((np.abs(got - want)[:, 5:] / np.maximum(bound[:, 5:], 1e-300)).max())))
        assert (np.abs(got - want) <= bound).all()
    assert np.array_equal(eng.constraint_group_report(pid, ng, tol, ABOUT), got)   # two reports of one state: the same bits
    more = eng.constraint_group_report(pid, ng + 2, None if tol is None else np.r_[tol, 1.0, 1.0], ABOUT)   # more declared groups than the table names
    assert np.array_equal(more[:ng], got) and (np.delete(more[ng:], 4, axis=1) == 0.0).all() and (more[ng:, 4] == -1.0).all()
    return got


def _midway_tolerances(rec, group, ng):
    """Per group a tolerance midway between two neighbours of its sorted distinct violations (a group with one value: half of it)."""
    tol = np.ones(ng)
    for g in range(ng):
        v = np.unique(np.abs(rec[group == g, 0]))
        if len(v) >= 2:
            tol[g] = 0.5 * (v[len(v) // 2 - 1] + v[len(v) // 2])
        elif len(v) == 1:
            tol[g] = 0.5 * v[0]
    return tol


@pytest.mark.parametrize("table", sorted(TABLES))
@pytest.mark.parametrize("name", POINT_KINDS)
def test_group_sums_exact_family(name, table):
    sizes = TABLES[table]
    group = _table(sizes, 3)
    ng = len(sizes)
    rng = np.random.default_rng(41)
    fam = cr.dyadic_point_springs(rng, group)
    prob = _point_problem(name, fam["x0a"], fam["v1a"], fam["d"], np.resize(fam["k"], ng), group, fam["dt"], rng, True)
    inp = cr.gather(prob)
    rec0, _ = cr.row_records(name, inp)
    tol = _midway_tolerances(rec0, group, ng)
    rec, _ = cr.row_records(name, inp, tol[group])
    cr.assert_exact_family(rec, group, ng, ABOUT)
    eng, pid = _engine(prob)
    rows = eng.constraint_report(pid, tol)
    assert np.array_equal(rows["records"], rec)   # every operation of a row is exact
    got = _check_groups(eng, pid, name, group, sizes, tol, rec, True)
    # beyond-tolerance counts for tolerances midway between two sorted violations
    assert np.array_equal(got[:, 2], [int((np.abs(rec[group == g, 0]) > tol[g]).sum()) for g in range(ng)])
    assert got[:, 2].sum() > 0 or table == "single"
    eng.close()


@pytest.mark.parametrize("table", sorted(TABLES))
@pytest.mark.parametrize("name", POINT_KINDS)
def test_group_sums_rounding_family(name, table):
    sizes = TABLES[table]
    group = _table(sizes, 4)
    n, ng = len(group), len(sizes)
    rng = np.random.default_rng(42)
    d = 10.0 ** (-4.0 + 3.0 * rng.random((n, 1))) * rng.standard_normal((n, 3))
    prob = _point_problem(name, 1.0 + rng.random((n, 3)), rng.standard_normal((n, 3)), d, 10.0 ** (2.0 + 3.0 * rng.random(ng)), group, 0.01, rng, False)
    eng, pid = _engine(prob)
    dev = eng.constraint_report(pid)["records"]
    tol = _midway_tolerances(dev, group, ng)
    dev = eng.constraint_report(pid, tol)["records"]
    want, _ = cr.row_records(name, cr.gather(prob), tol[group])
    assert (np.abs(dev - want)[:, :15] <= cr.row_bounds(name, None, want)[:, :15]).all()
    # the sums are the device's sums of the device's rows: the restatement sums those
    _check_groups(eng, pid, name, group, sizes, tol, dev, False)
    eng.close()


def test_argmax_ties_resolve_to_the_smaller_list_position():
    """Two equal maxima planted in one group, in different chunks: slot 4 is the position of the first in the group's list."""
    sizes = [5, 2 * CHUNK + 9, 300]
    group = _table(sizes, 5)
    ng = len(sizes)
    rng = np.random.default_rng(43)
    fam = cr.dyadic_point_springs(rng, group)
    members = np.flatnonzero(group == 1)
    first, second = 100, CHUNK + 5   # positions in the list of group 1: chunks 0 and 1
    d = fam["d"].copy()
    d[members[first]] = np.array([30.0, 40.0, 0.0]) / 64.0   # |d| = 50 / 64: beyond every other row's
    d[members[second]] = np.array([0.0, -40.0, 30.0]) / 64.0
    assert np.sqrt((d * d).sum(axis=1)).max() == 50.0 / 64.0 and (np.sqrt((d * d).sum(axis=1)) == 50.0 / 64.0).sum() == 2
    for name in POINT_KINDS:
        prob = _point_problem(name, fam["x0a"], fam["v1a"], d, np.resize(fam["k"], ng), group, fam["dt"], rng, True)
        eng, pid = _engine(prob)
        got = eng.constraint_group_report(pid, ng, None, ABOUT)
        assert got[1, 3] == 50.0 / 64.0 and got[1, 4] == first
        rec = eng.constraint_report(pid)["records"]
        assert rec[members[first], 0] == rec[members[second], 0] == got[1, 3]
        assert (got[:, 2] == 0.0).all()   # no tolerance: nothing is beyond it
        eng.close()


# ---- 3. cross-checks against the engine's own pipelines ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("fixture", ["rbchain", "attachzoo"])
def test_against_element_energies_and_the_force_readout(fixture):
    from gpu_util import engine_from_problem
    from oracle import evaluator as ev
    from stark_amd import capi

    prob, man, z = ev.load_fixture(os.path.join(GOLDEN, fixture + ".npz"))
    eng = engine_from_problem(prob, man)
    eng.eval(capi.EVAL_P)
    seen = set()
    for pi, pot in enumerate(prob.potentials):
        if pot.name not in cr.KINDS or len(pot.conn) == 0:
            continue
        seen.add(pot.name)
        pid = eng.pot_ids[pi]
        got = eng.constraint_report(pid)
        rec = got["records"]
        assert len(rec) == len(pot.conn) and np.array_equal(got["ids"], cr.ids_of(prob, pot.name, pot))
        E = eng.element_energies(pid, len(pot.conn))
        assert (np.abs(rec[:, 14] - E) <= cr.ROW_TOL * np.abs(E).max()).all(), pot.name
        f, rows = eng.element_forces(pid, 1.0 / prob.dt)
        blocks_a, blocks_b = cr.KINDS[pot.name][6], cr.KINDS[pot.name][7]
        f_a = sum((f[:, k] for k in blocks_a), np.zeros((len(rec), 3)))
        tol = cr.ROW_TOL * max(np.abs(f).max(), np.abs(rec[:, 2:5]).max())
        assert (np.abs(rec[:, 2:5] - f_a) <= tol).all(), pot.name
        if blocks_b:   # side b's blocks sum to the negative
            assert (np.abs(rec[:, 2:5] + sum((f[:, k] for k in blocks_b), np.zeros((len(rec), 3)))) <= tol).all(), pot.name
        assert np.array_equal(got["row_a"], rows[:, cr.KINDS[pot.name][2]])
        # the restatement on the fixture's own state
        want, _ = cr.row_records(pot.name, cr.gather(prob, pot))
        assert (np.abs(rec - want) <= cr.row_bounds(pot.name, cr.gather(prob, pot), want) + 1e-300).all(), pot.name
    assert seen == {n for n in cr.KINDS if any(p.name == n and len(p.conn) for p in prob.potentials)} and seen
    eng.close()


# ---- 4. host mirror ---------------------------------------------------------------------------------------------------------------------------
def _sim(S):
    st = S.default_settings()
    st.init_frictional_contact = 0
    st.max_time_step_size = 0.002
    st.newton.residual_tolerance_abs = 1e-6
    st.newton.step_tolerance = 0.0
    st.gravity[0], st.gravity[1], st.gravity[2] = 0.0, 0.0, 0.0
    return S.Simulation(st)


def _box(S, sim, mass, translation=None):
    b = sim.rb_add(mass, S.inertia_tensor_box(mass, (0.1, 0.1, 0.1)))
    if translation is not None:
        sim.rb_set_translation(b, translation)
    return b


def _pair(S, sim, translation, mass=3.5):
    box0 = _box(S, sim, mass)
    sim.rb_add_constraint("fix", box0)
    return box0, _box(S, sim, mass, translation)


# the two-box scenes of tests/test_gpu_rb_constraints.py: base type -> (registry name, scene)
def _scene(S, sim, base):
    pert = 91.0
    if base == "global_point":
        b = _box(S, sim, 3.5)
        c = sim.rb_add_constraint("global_point", b, -1, sim.rb_state(b)[0])
        sim.rb_add_force_at_centroid(b, (pert, 0, 0))
    elif base == "global_direction":
        b = _box(S, sim, 3.5)
        c = sim.rb_add_constraint("global_direction", b, -1, (0.0, 0.0, 1.0))
        sim.rb_add_torque(b, (pert, 0, 0))
    elif base == "point":
        b0, b1 = _pair(S, sim, (0.1, 0.0, 0.0))
        c = sim.rb_add_constraint("point", b0, b1, (0.05, 0.0, 0.0))
        sim.rb_add_force_at_centroid(b1, (pert, 0, 0))
    elif base == "point_on_axis":
        b0, b1 = _pair(S, sim, (0.1, 0.0, 0.0))
        c = sim.rb_add_constraint("point_on_axis", b0, b1, (0.0, 0.0, 0.0), (0.0, 0.0, 1.0))
        sim.rb_add_force_at_centroid(b1, (pert, 0, 0))
    elif base == "distance":
        b0, b1 = _pair(S, sim, (1.0, 0.0, 0.0))
        c = sim.rb_add_constraint("distance", b0, b1, sim.rb_state(b0)[0], sim.rb_state(b1)[0])
        sim.rb_add_force_at_centroid(b1, (pert, 0, 0))
    elif base == "distance_limits":
        b0, b1 = _pair(S, sim, (1.0, 0.0, 0.0))
        c = sim.rb_add_constraint("distance_limits", b0, b1, sim.rb_state(b0)[0], sim.rb_state(b1)[0], 0.9999, 1.0001)
        sim.rb_add_force_at_centroid(b1, (pert, 0, 0))
    elif base == "direction":
        b0, b1 = _pair(S, sim, (0.0, 0.0, 0.1))
        c = sim.rb_add_constraint("direction", b0, b1, (0.0, 0.0, 1.0))
        sim.rb_add_torque(b1, (pert, 0, 0))
    elif base == "angle_limit":
        b0, b1 = _pair(S, sim, (0.0, 0.0, 0.1))
        c = sim.rb_add_constraint("angle_limit", b0, b1, (0.0, 0.0, 1.0), 5.0)
        sim.rb_add_torque(b1, (pert, 0, 0))
    elif base == "spring":
        b0, b1 = _pair(S, sim, (0.2, 0.0, 0.0))
        c = sim.rb_add_constraint("spring", b0, b1, sim.rb_state(b0)[0], sim.rb_state(b1)[0], 1000.0, 1.0)
        sim.rb_add_force_at_centroid(b1, (1.0, 0.5, 0))
    elif base == "linear_velocity":
        b0, b1 = _pair(S, sim, (0.1, 0.0, 0.0))
        sim.rb_add_constraint("point", b0, b1, (0.05, 0.0, 0.0))
        c = sim.rb_add_constraint("linear_velocity", b0, b1, (1.0, 0.0, 0.0), 3.7, 50.0, 0.01)
    else:
        b0, b1 = _pair(S, sim, (0.1, 0.0, 0.0))
        sim.rb_add_constraint("attachment", b0, b1)
        c = sim.rb_add_constraint("angular_velocity", b0, b1, (1.0, 0.0, 0.0), 1.7, 10.0, 0.01)
    return c


HANDLERS = {"global_point": "rb_constraint_global_points", "global_direction": "rb_constraint_global_directions", "point": "rb_constraint_points",
            "point_on_axis": "rb_constraint_point_on_axis", "distance": "rb_constraint_distances", "distance_limits": "rb_constraint_distance_limits",
            "direction": "rb_constraint_directions", "angle_limit": "rb_constraint_angle_limits", "spring": "rb_constraint_damped_spring",
            "linear_velocity": "rb_constraint_linear_velocity", "angular_velocity": "rb_constraint_angular_velocity"}


def _close(a, b, scale, rel=1e-9):
    return abs(a - b) <= rel * max(abs(a), abs(b), scale)


@pytest.mark.parametrize("base", sorted(HANDLERS))
def test_host_mirror_against_the_constraint_handlers(base):
    """After every accepted step constraints() slot 0 is the handler's violation; slot 1 its reaction wherever the violation is within tolerance (soft
    hardening after acceptance changes the stiffness the handler reads otherwise)."""
    from stark_amd import sim as S

    sim = _sim(S)
    c = _scene(S, sim, base)
    sim.record_constraints(True, ABOUT)
    accepted, engaged = 0, 0
    for _ in range(30):
        t_before = sim.info().current_time
        assert sim.run_one_step()
        if sim.info().current_time == t_before:
            continue
        accepted += 1
        rep = sim.constraints()
        assert abs(rep["time"] - sim.info().current_time) < 1e-12
        kind = rep["kinds"][HANDLERS[base]]
        rows = kind["rows"]
        assert kind["unit"] == cr.KINDS[HANDLERS[base]][5] and np.array_equal(kind["groups"][:, 0], np.ones(len(rows["records"])))
        C_, f_, tol = sim.rb_constraint_measure(base, c)
        scale = {"m": 1e-3, "deg": 1e-1, "m/s": 1e-3, "deg/s": 1e-1}[kind["unit"]]   # (a violation near zero is a difference of O(1) lengths / angles)
        slack = 0.0
        if base == "angle_limit" and C_ > 0.0:   # acos(1 - c^2 / 2) amplifies the rounding of its argument by 1 / c on both routes
            slack = np.degrees(8.0 * U / (2.0 * np.sin(0.5 * np.radians(C_))))
        assert abs(rows["violation"][c] - C_) <= slack or _close(rows["violation"][c], C_, scale), (base, rows["violation"][c], C_)
        hardens = base not in ("spring", "linear_velocity", "angular_velocity")
        if not hardens or abs(C_) <= tol:
            assert _close(rows["reaction"][c], f_, 1.0), (base, rows["reaction"][c], f_)   # (1e-9 N absolute for a reaction near zero)
        if hardens:
            assert np.array_equal(kind["tolerance"][c:c + 1], [tol]) and bool(rows["beyond_tolerance"][c]) == (abs(rows["violation"][c]) > tol)
        else:
            assert not rows["beyond_tolerance"].any()
        engaged += int(rows["active"][c])
        if base == "spring":
            dC, df, _ = sim.rb_constraint_measure(base, c, which=1)
            assert _close(rows["damper_velocity"][c], dC, 1e-6) and _close(rows["damper_force"][c], df, 1e-6)
        if accepted >= 6:
            break
    assert accepted >= 3 and engaged >= 1
    sim.close()


def _counter(sim, name):
    from stark_amd import capi

    v = C.c_int64()
    assert capi.lib().mistark_get_counter(sim.engine_handle(), name.encode(), C.byref(v)) == 0
    return v.value


def test_hardened_scene_reports_no_row_beyond_tolerance():
    """The README beam clamped by prescribe_inside_aabb plus one attach_point_point, both with finite tolerances: a step is accepted only once the
    hardening callbacks find every row within tolerance, so every accepted step's report has zero rows beyond tolerance in the kinds that harden."""
    from stark_amd import sim as S

    sim = S.Simulation(S.default_settings())
    beam = sim.add_volume_grid("beam", (0, 0, 0), (1.0, 0.25, 0.25), (12, 3, 3), S.soft_rubber())
    sim.prescribe_inside_aabb(beam, (-0.5, 0, 0), (2e-3, 2, 2), 1e3, 1e-5)
    X = sim.points("X")
    tip = int(np.argmax(X[:, 0] - 10.0 * np.abs(X[:, 1]) - 10.0 * np.abs(X[:, 2] - X[:, 2].min())))
    rod = sim.add_line_as_segments("rod", X[tip], X[tip] + np.array([0.0, 0.0, -0.2]), 3, S.elastic_rubberband())
    sim.attach_point_point(rod, beam, [0], [tip], 10.0, 1e-4)
    sim.record_constraints(True)
    accepted = 0
    for _ in range(60):
        t_before = sim.info().current_time
        assert sim.run_one_step()
        if sim.info().current_time == t_before:
            continue
        accepted += 1
        rep = sim.constraints()
        assert set(rep["kinds"]) == {"EnergyPrescribedPositions", "EnergyAttachments_d_d_p_p"}
        for name, kind in rep["kinds"].items():
            assert np.isfinite(kind["tolerance"]).all() and (kind["groups"][:, 2] == 0.0).all(), name
            assert not kind["rows"]["beyond_tolerance"].any() and (kind["groups"][:, 3] <= kind["tolerance"]).all()
            assert kind["groups"][:, 0].sum() == len(kind["rows"]["records"]) and np.abs(kind["groups"][:, 5:8]).max() > 0.0
        if accepted >= 3:
            break
    assert accepted >= 3 and sim.info().failed_steps >= 1   # (the soft springs did harden on the way)
    sim.close()


# ---- 5. nothing else moves -----------------------------------------------------------------------------------------------------------------------
def test_recording_does_not_change_the_attachzoo_trajectory():
    from stark_amd import sim as S
    from test_gpu_scene import _attachzoo_full, _cloth_triangles, _load

    z, traj, man = _load("traj_attachzoo")

    def run(record):
        sim, box, _ = _attachzoo_full(S, traj["scene"], _cloth_triangles(man, z))
        if record:
            sim.record_constraints(True, ABOUT)
        counts = []
        for _ in range(len(traj["steps"])):
            assert sim.run_one_step()
            i = sim.info()
            counts.append((i.total_newton_iterations, i.total_linear_solves, i.total_cg_iterations))
        out = sim.points("x0"), sim.points("v0"), sim.rb_state(box), counts, _counter(sim, "constraint_reports")
        if record:
            rep = sim.constraints()
            assert {"EnergyPrescribedPositions"} | {n for n in cr.NAMES if n.startswith("EnergyAttachments")} == set(rep["kinds"])
        sim.close()
        return out

    x_off, v_off, rb_off, c_off, r_off = run(False)
    x_on, v_on, rb_on, c_on, r_on = run(True)
    assert r_off == 0 and r_on == 6 * len(traj["steps"])   # six constraint potentials per accepted step
    assert c_on == c_off and np.array_equal(x_on, x_off) and np.array_equal(v_on, v_off)
    assert all(np.array_equal(a, b) for a, b in zip(rb_on, rb_off))


def test_constraints_before_an_accepted_step_is_refused():
    from stark_amd import sim as S

    sim = S.Simulation(S.default_settings())
    cube = sim.add_volume_grid("cube", (0, 0, 0), (0.1, 0.1, 0.1), (2, 2, 2), S.soft_rubber())
    sim.prescribe_inside_aabb(cube, (-0.05, 0, 0), (2e-3, 2, 2), 1e6)
    with pytest.raises(S.SimError, match="recording is off"):
        sim.constraints()
    sim.record_constraints(True)
    with pytest.raises(S.SimError, match="no time step has been accepted"):
        sim.constraints()
    assert sim.run_one_step()
    rep = sim.constraints()
    assert list(rep["kinds"]) == ["EnergyPrescribedPositions"] and np.isinf(rep["kinds"]["EnergyPrescribedPositions"]["tolerance"]).all()
    sim.record_constraints(False)
    with pytest.raises(S.SimError, match="recording is off"):
        sim.constraints()
    sim.close()


# ---- 6. refusals ------------------------------------------------------------------------------------------------------------------------------------
def test_other_custom_and_bad_potentials_groups_and_tolerances_are_refused():
    import stark_amd
    from gpu_util import engine_from_problem
    from oracle import evaluator as ev

    Err = stark_amd.engine.EngineError
    prob, man, z = ev.load_fixture(os.path.join(GOLDEN, "attachzoo.npz"))
    eng = engine_from_problem(prob, man)
    names = {p: prob.potentials[pi].name for pi, p in eng.pot_ids.items()}
    other = [p for p, n in names.items() if n not in cr.KINDS]
    assert other
    for p in other:
        for call in (lambda: eng.constraint_report(p), lambda: eng.constraint_group_report(p, 1)):
            with pytest.raises(Err, match=names[p]) as e:
                call()
            assert "has no constraint report" in str(e.value)
    with pytest.raises(Err, match="bad potential id"):
        eng.constraint_report(len(names) + 5)
    with pytest.raises(Err, match="bad potential id"):
        eng.constraint_group_report(-1, 1)
    pid = [p for p, n in names.items() if n == "EnergyPrescribedPositions"][0]
    ng = int(eng.constraint_report(pid)["group"].max()) + 1
    for call in (lambda: eng.constraint_group_report(pid, ng - 1), lambda: eng.constraint_report(pid, np.ones(ng - 1)), lambda: eng.constraint_report(pid, None, ng - 1)):
        with pytest.raises(Err, match="names group") as e:
            call()
        assert "n_groups is %d" % (ng - 1) in str(e.value)
    for bad in (-1.0, np.inf, np.nan):
        tol = np.ones(ng)
        tol[ng - 1] = bad
        for call in (lambda: eng.constraint_report(pid, tol), lambda: eng.constraint_group_report(pid, ng, tol)):
            with pytest.raises(Err, match="negative or not finite"):
                call()
    with pytest.raises(Err, match="n_groups is 0"):   # (no group count is larger than a group id of a table with rows)
        eng.constraint_group_report(pid, 0)
    assert eng.counter("constraint_reports") == 1   # (the one report that read the group ids)
    eng.close()
    # user-defined potentials
    prob, man, z = ev.load_fixture(os.path.join(GOLDEN, "tetbeam_eo_4x1x1.npz"))
    eng = engine_from_problem(prob, man, custom_ops=z)
    pid = sorted(eng.pot_ids.values())[0]
    for call in (lambda: eng.constraint_report(pid), lambda: eng.constraint_group_report(pid, 1)):
        with pytest.raises(Err, match="user-defined"):
            call()
    assert eng.counter("constraint_reports") == 0
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
        for call in (lambda: eng.constraint_report(0), lambda: eng.constraint_group_report(0, 1)):
            with pytest.raises(stark_amd.engine.EngineError, match="single-rank"):
                call()
        eng.close()
    finally:
        L.mistark_local_group_destroy(group)
    h = C.c_void_p()
    assert L.mistark_create_dry(C.byref(h)) == 0
    try:
        out, about, n, kind = (C.c_double * 16)(), (C.c_double * 3)(), C.c_int64(), C.c_int32()
        for rc in (L.mistark_potential_constraint_report(h, 0, None, 0, out, None, None, C.byref(n), C.byref(kind)), L.mistark_constraint_group_report(h, 0, None, 1, about, out)):
            assert rc < 0
            assert "registration-only" in L.mistark_last_error(h).decode()
    finally:
        L.mistark_destroy(h)


def test_empty_table_reports_zero_rows_without_a_launch():
    prob, _ = cr.seeded_problem("EnergyPrescribedPositions")
    eng, pid = _engine(prob)
    assert len(eng.constraint_report(pid)["records"]) == cr.N_ROWS and eng.counter("constraint_reports") == 1
    eng.set_dynamic(pid, True)
    eng.update_connectivity(pid, prob.potentials[0].conn[:0])
    got = eng.constraint_report(pid, np.ones(3))
    assert got["records"].shape == (0, 16) and got["kind"] == 0
    grp = eng.constraint_group_report(pid, 3, np.ones(3), ABOUT)
    assert (np.delete(grp, 4, axis=1) == 0.0).all() and (grp[:, 4] == -1.0).all()
    assert eng.counter("constraint_reports") == 1 and eng.counter("constraint_report_chunks") == 0
    eng.close()
