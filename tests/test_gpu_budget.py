"""Budget readout on the GPU (include/mistark.h "budget readout", include/mistark_sim.h "budget recording"): energies per potential and the 13-slot
records of inertia groups and rigid bodies, against the numpy restatement of tests/budget_ref.py, the engine's own evaluation, the force and stress
readouts, and identities of the physics.

Tolerances are multiples of 2^-53 * S_abs, S_abs = sum |terms| of the sum in question (tests/budget_ref.py): (n + 8) for a sum of n items or elements
in any order, 64 for the fixed number of operations of one rigid body. The exact family uses ==."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import budget_ref as br  # noqa: E402
from fixture_list import stage_dumps  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
DUMPS = stage_dumps()
IDS = [os.path.basename(p)[:-4] for p in DUMPS]
U = br.U
CHUNK = 2048  # BUDGET_CHUNK of csrc/budget.hip: items per workgroup
ABOUT = np.array([0.25, -0.5, 0.125])  # (integers / 64)
# group sizes per table; 0: a declared group without items. Around the wavefront (64 x 4 = 256 threads), around a few strides of 256, around one and
# two chunks; one table with a single item.
TABLES = {
    "small": [1, 255, 256, 0, 257, 1023, 1024, 1025],
    "chunks": [CHUNK - 1, CHUNK, 0, CHUNK + 1, 4097],
    "single": [1],
}


def _table(sizes, seed):
    """group[i] of every item: the groups' items interleaved through the list in a fixed shuffled order."""
    group = np.concatenate([np.full(s, g, dtype=np.int32) for g, s in enumerate(sizes)])
    np.random.default_rng(seed).shuffle(group)
    return group


def _inertia_engine(volume, density, x0, v1, dt, gravity, group):
    """An EnergyLumpedInertia potential through Engine from plain arrays, bindings in the reference's order; item i is point i."""
    import stark_amd

    n, ng = len(volume), len(density)
    eng = stark_amd.Engine(0)
    v1 = np.ascontiguousarray(v1, dtype=np.float64)
    eng.add_dof_set("soft.v1", v1)
    zeros = np.zeros((n, 3))
    ids = [eng.array(v1, 3), eng.array(np.ascontiguousarray(x0, dtype=np.float64), 3), eng.array(zeros.copy(), 3), eng.array(zeros.copy(), 3), eng.array(zeros.copy(), 3),
           eng.array(np.ascontiguousarray(volume, dtype=np.float64).reshape(n, 1), 1), eng.array(np.ascontiguousarray(density, dtype=np.float64).reshape(ng, 1), 1),
           eng.array(np.zeros((ng, 1)), 1), eng.array(np.zeros((ng, 1)), 1), eng.array(np.array([[float(dt)]]), 1),
           eng.array(np.ascontiguousarray(gravity, dtype=np.float64).reshape(1, 3), 3)]
    cols = [1, 1, 1, 1, 1, 0, 2, 2, 2, -1, -1]
    strides = [3, 3, 3, 3, 3, 1, 1, 1, 1, 1, 3]
    conn = np.stack([np.arange(n), np.arange(n), group], axis=1).astype(np.int32)
    pid = eng.potential("EnergyLumpedInertia", conn, list(zip(ids, strides, cols)))
    return eng, pid


# ---- 1. the exact family ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("table", sorted(TABLES))
def test_exact_family(table):
    sizes = TABLES[table]
    group = _table(sizes, 3)
    n, ng = len(group), len(sizes)
    rng = np.random.default_rng(21)
    volume = rng.integers(1, 32, n) / 8.0
    x0 = rng.integers(-31, 32, (n, 3)) / 64.0
    v1 = rng.integers(-31, 32, (n, 3)) / 64.0
    density, dt, gravity = np.ones(ng), 0.125, np.array([0.0, 0.0, -8.0])
    br.assert_exact_family(volume, density, x0, v1, dt, group, ng, ABOUT, gravity)
    want, _ = br.inertia_records(volume, density, x0, v1, dt, group, ng, ABOUT, gravity)
    eng, pid = _inertia_engine(volume, density, x0, v1, dt, gravity, group)
    got = eng.inertia_budget(pid, ng, ABOUT)
    assert (got == want).all(), np.argwhere(got != want)
    assert (got[:, 12] == sizes).all()
    for g, s in enumerate(sizes):
        if s == 0:
            assert (got[g] == 0.0).all()
    assert eng.counter("budget_readouts") == 1
    assert eng.counter("budget_chunks") == sum((s + CHUNK - 1) // CHUNK for s in sizes)
    assert np.array_equal(eng.inertia_budget(pid, ng, ABOUT), got)   # two readouts of one state: the same bits
    # more declared groups than the list names: zeros behind
    more = eng.inertia_budget(pid, ng + 2, ABOUT)
    assert np.array_equal(more[:ng], got) and (more[ng:] == 0.0).all()
    eng.close()


# ---- 2. the rounding family ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("table", sorted(TABLES))
def test_rounding_family(table):
    sizes = TABLES[table]
    group = _table(sizes, 4)
    n, ng = len(group), len(sizes)
    rng = np.random.default_rng(22)
    volume, density = 1e-4 * (0.1 + rng.random(n)), 500.0 + 1000.0 * rng.random(ng)
    x0, v1, dt, gravity = 1.0 + rng.random((n, 3)), rng.standard_normal((n, 3)), 0.01, np.array([0.3, -0.2, -9.81])
    want, mag = br.inertia_records(volume, density, x0, v1, dt, group, ng, ABOUT, gravity)
    eng, pid = _inertia_engine(volume, density, x0, v1, dt, gravity, group)
    got = eng.inertia_budget(pid, ng, ABOUT)
    bound = (np.asarray(sizes)[:, None] + 8) * U * mag
    print("%s: worst |difference| / bound %.3g" % (table, float((np.abs(got - want) / np.maximum(bound, 1e-300)).max())))
    assert (np.abs(got - want) <= bound).all()
    assert np.array_equal(eng.inertia_budget(pid, ng, ABOUT), got)
    eng.close()


# ---- 3. energies per potential --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", DUMPS, ids=IDS)
def test_energies_match_the_evaluation(path):
    from gpu_util import engine_from_problem
    from oracle import evaluator as ev
    from stark_amd import capi

    prob, man, z = ev.load_fixture(path)
    eng = engine_from_problem(prob, man)
    E, _ = eng.eval(capi.EVAL_P)
    pids = [eng.pot_ids[pi] for pi in sorted(eng.pot_ids)]
    all_el = []
    for pi in sorted(eng.pot_ids):
        pid, pot = eng.pot_ids[pi], prob.potentials[pi]
        el = eng.element_energies(pid, len(pot.conn))
        want, mag = br.energy_sum(el)
        (got,) = eng.energies([pid])
        assert abs(got - want) <= (len(el) + 8) * U * mag, pot.name
        if pot.has_condition:
            o = ev.evaluate_potential(prob, pot)
            active = np.zeros(len(el), dtype=bool) if o is None else o.active
            assert (el[~active] == 0.0).all(), pot.name      # switched-off elements count zero
            if not active.any():
                assert got == 0.0, pot.name
        all_el.append(el)
    every = eng.energies(None)
    assert len(every) == len(pids)
    assert np.array_equal(every, eng.energies(pids)) and np.array_equal(every, eng.energies(None))
    flat = np.concatenate(all_el)
    total, mag = br.energy_sum(flat)
    print("%s: sum of the potentials %.17g, eval %.17g, bound %.3g" % (os.path.basename(path), every.sum(), E, 2 * (len(flat) + 8) * U * mag))
    assert abs(float(np.sum(every)) - E) <= 2 * (len(flat) + 8) * U * mag
    eng.close()


def test_empty_table_reports_zero_without_a_launch():
    from gpu_util import engine_from_problem
    from oracle import evaluator as ev

    prob, man, z = ev.load_fixture(os.path.join(GOLDEN, "contactmix_t0.npz"))
    eng = engine_from_problem(prob, man)
    pi = sorted(k for k in eng.pot_ids if "contact" in prob.potentials[k].name)[0]
    pid = eng.pot_ids[pi]
    eng.set_dynamic(pid, True)
    eng.update_connectivity(pid, prob.potentials[pi].conn[:0])   # the table runs empty, as a contact table does when its pairs separate
    assert (eng.energies([pid]) == 0.0).all()
    assert eng.counter("budget_readouts") == 0
    others = [p for k, p in sorted(eng.pot_ids.items()) if k != pi]
    every = eng.energies(None)
    assert every[pid] == 0.0 and np.array_equal(np.delete(every, pid), eng.energies(others))
    eng.close()


# ---- 4. rigid bodies -------------------------------------------------------------------------------------------------------------------------
def _rb_set_velocity(sim, b, v, w):
    v, w = (C.c_double * 3)(*v), (C.c_double * 3)(*w)
    sim._ck(sim.L.mistark_sim_rb_set_velocity(sim.h, b, v, w))


def _check_bodies(sim, bodies, about, gravity=(0.0, 0.0, -9.81)):
    """budget()'s rigid objects against the restatement at the rb_state() downloads of the accepted state."""
    objs = [o for o in sim.budget()["objects"] if o["kind"] == "rigid"]
    assert len(objs) == len(bodies)
    worst = 0.0
    for b, (o, (mass, size)) in enumerate(zip(objs, bodies)):
        t, q, v, w = sim.rb_state(b)
        want, mag = br.body_record(mass, t, br.quat_to_R(q), v, w, br.inertia_tensor_box(mass, size), about, gravity)
        got = np.r_[o["mass"], o["mass"] * o["com"], o["momentum"], o["angular_momentum"], o["kinetic"], o["gravitational"], o["count"]]
        bound = 64 * U * mag
        bound[1:4] += 2 * U * mag[1:4]   # (the first moment went through a division and a product on the way here)
        worst = max(worst, float((np.abs(got - want) / np.maximum(bound, 1e-300)).max()))
        assert (np.abs(got - want) <= bound).all(), (b, got, want)
    print("bodies: worst |difference| / bound %.3g" % worst)


def test_rigid_budget_of_a_spinning_box():
    from stark_amd import sim as S

    st = S.default_settings()
    st.init_frictional_contact = 0
    sim = S.Simulation(st)
    mass, size = 2.5, (0.3, 0.2, 0.1)
    b = sim.add_rigid_box("spinner", mass, size)
    sim.rb_set_translation(b, (0.4, -0.1, 0.9))
    sim.rb_add_rotation(b, 35.0, (0.3, 1.0, 0.2))
    _rb_set_velocity(sim, b, (0.3, 0.2, -0.5), (2.0, 1.0, -3.0))
    sim.record_budget(True, ABOUT)
    for _ in range(2):
        assert sim.run_one_step()
        assert sim.info().last_newton_result == 0
        _check_bodies(sim, [(mass, size)], ABOUT)
    o = sim.budget()["objects"][0]
    assert o["label"] == "spinner" and o["kinetic"] > 0.0 and np.abs(o["angular_momentum"]).max() > 0.0
    sim.close()


def test_rigid_budget_of_the_rbchain_scene():
    """The rbchain scene of tests/test_gpu_scene.py (9 boxes, all 13 rigid-body potentials)."""
    from stark_amd import sim as S

    st = S.default_settings()
    st.init_frictional_contact = 0
    sim = S.Simulation(st)
    sim.rb_set_default_constraint_params(stiffness=1e4)
    axis = np.array([1.0, 0.5, -0.3])
    axis /= np.linalg.norm(axis)
    size = (0.1, 0.12, 0.08)
    bodies = []

    def box(x, y, zz):
        b = sim.add_rigid_box("box%d" % len(bodies), 1.0 + 0.1 * x, size)
        bodies.append((1.0 + 0.1 * x, size))
        sim.rb_set_translation(b, (x, y, zz))
        sim.rb_add_rotation(b, 20.0 * x + 5.0, axis)
        return b

    def unit(v):
        v = np.asarray(v, dtype=float)
        return v / np.linalg.norm(v)

    b0 = box(0.0, 0.0, 0.0)
    sim.rb_add_constraint("fix", b0)
    b1 = box(0.15, 0.0, 0.0)
    sim.rb_add_constraint("point", b0, b1, (0.07, 0.02, 0.01))
    b2 = box(0.30, 0.02, 0.0)
    sim.rb_add_constraint("point_on_axis", b1, b2, (0.22, 0.0, 0.01), unit((1.0, 0.2, 0.0)))
    b3 = box(0.45, 0.0, 0.03)
    sim.rb_add_constraint("distance", b2, b3, (0.33, 0.0, 0.0), (0.42, 0.01, 0.02))
    b4 = box(0.60, 0.0, 0.0)
    sim.rb_add_constraint("distance_limits", b3, b4, (0.48, 0.0, 0.0), (0.57, 0.0, 0.0), 0.08995, 0.09005)
    sim.rb_add_constraint("direction", b3, b4, unit((0.0, 1.0, 0.2)))
    b5 = box(0.75, 0.0, 0.0)
    sim.rb_add_constraint("point", b4, b5, (0.67, 0.0, 0.0))
    sim.rb_add_constraint("angle_limit", b4, b5, (1.0, 0.0, 0.0), 0.5)
    b6 = box(0.90, 0.0, 0.0)
    sim.rb_add_constraint("spring", b5, b6, (0.78, 0.0, 0.0), (0.87, 0.01, 0.0), 200.0, 3.0)
    b7 = box(1.05, 0.0, 0.0)
    sim.rb_add_constraint("point_on_axis", b6, b7, (0.97, 0.0, 0.0), (1.0, 0.0, 0.0))
    sim.rb_add_constraint("linear_velocity", b6, b7, (1.0, 0.0, 0.0), 0.3, 5.0, 0.05)
    b8 = box(1.20, 0.0, 0.0)
    sim.rb_add_constraint("hinge", b7, b8, (1.12, 0.0, 0.0), (0.0, 1.0, 0.0))
    sim.rb_add_constraint("angular_velocity", b7, b8, (0.0, 1.0, 0.0), 1.0, 2.0, 0.1)
    sim.record_budget(True, ABOUT)
    accepted = 0
    for _ in range(4):   # (the first call ends with "invalid converged state" and is redone: tests/test_gpu_scene.py)
        t_before = sim.info().current_time
        assert sim.run_one_step()
        if sim.info().current_time > t_before:
            accepted += 1
            bud = sim.budget()
            assert abs(bud["time"] - sim.info().current_time) < 1e-12
            assert [o["label"] for o in bud["objects"]] == ["box%d" % k for k in range(9)]
            _check_bodies(sim, bodies, ABOUT)
    assert accepted >= 2
    sim.close()


# ---- 5. the momentum theorem against the force readout ------------------------------------------------------------------------------------------
def _lumped_masses(X, tets, density):
    e = X[tets[:, 1:]] - X[tets[:, :1]]
    vol = np.abs(np.einsum("ij,ij->i", e[:, 0], np.cross(e[:, 1], e[:, 2]))) / 6.0
    m = np.zeros(len(X))
    for k in range(4):
        np.add.at(m, tets[:, k], density * vol / 4.0)
    return m


def test_momentum_theorem_against_the_force_readout():
    """A tet cube thrown with spin under gravity, no damping, no contact: the inertia potential's gradient is m (v1 - v0) - dt m g per node, so
    dt * (M g - sum of the nodal forces of EnergyLumpedInertia) = p(step) - p(step - 1), an identity of the two readouts that no solver tolerance
    enters. Rounding: a nodal force is (m / dt^2) ((x0 + dt v1) - (x0 + dt v0)) + m g evaluated in double, so its terms are of size m |x| / dt^2 and
    m |g|; a momentum's terms are m |v|. The bound is (n + 8) * 2^-53 * the sum of those on both sides, times 8 for the handful of roundings inside a
    term."""
    from stark_amd import sim as S
    from test_gpu_forces import _EngineView, _first_row, _pots

    st = S.default_settings()
    st.init_frictional_contact = 0
    st.max_time_step_size = 0.01
    sim = S.Simulation(st)
    params = S.soft_rubber()
    params.inertia_damping = 0.0
    sim.add_volume_grid("cube", (0.0, 0.0, 1.0), (0.2, 0.2, 0.2), (4, 4, 4), params)
    X = sim.points("X")
    v_init = np.array([0.5, -0.3, 1.0]) + np.cross(np.array([2.0, -1.0, 3.0]), X - X.mean(axis=0))
    sim.set_points("v0", v_init)
    sim.record_forces(["EnergyLumpedInertia"])
    sim.record_budget(True)
    g = np.array([0.0, 0.0, -9.81])
    p_prev, v_prev, m = None, v_init, None
    for step in range(3):
        x_before = sim.points("x0")
        assert sim.run_one_step()
        info = sim.info()
        assert info.last_newton_result == 0
        dt = info.current_time / (step + 1)
        if m is None:
            with _EngineView(sim) as (eng, desc):
                (pid,) = [p for p in _pots(desc, "EnergyTetStrain") if desc["potentials"][p]["n_elem"] > 0]
                _, rows = eng.element_forces(pid, 1.0)
                r0, _ = _first_row(desc, "soft.v1")
            m = _lumped_masses(X, (rows - r0).astype(np.int64), params.density)
            p_prev = np.array([br.sum_terms(m * v_init[:, k])[0] for k in range(3)])
        bud = sim.budget()
        (obj,) = bud["objects"]
        assert obj["label"] == "cube" and obj["kind"] == "deformable" and obj["count"] == len(X)
        assert abs(obj["mass"] - m.sum()) <= 1e-12 * m.sum()   # (two evaluations of the tets' triple products: each cancels by less than 10^2)
        f, _ = sim.forces(0)
        v_now = sim.points("v0")   # (the accepted step has made the converged v1 its v0)
        lhs = dt * (obj["mass"] * g - f.sum(axis=0))
        rhs = obj["momentum"] - p_prev
        mag = np.array([(m * (2.0 * np.abs(x_before[:, k]) / dt + dt * np.abs(g[k]) * 2.0 + np.abs(v_now[:, k]) + np.abs(v_prev[:, k]))).sum() for k in range(3)])
        bound = 8 * (len(X) + 8) * U * mag
        print("step %d: dt (M g - sum f) = %s, p - p_prev = %s, |difference| / bound %s" % (step, lhs, rhs, np.abs(lhs - rhs) / bound))
        assert np.abs(rhs).max() > 1e-3 * np.abs(obj["momentum"]).max()   # gravity has changed the momentum
        assert (np.abs(lhs - rhs) <= bound).all()
        p_prev, v_prev = obj["momentum"], v_now
    sim.close()


# ---- 6. strain energy against the stress readout ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scene", ["tet_beam", "cloth"])
def test_strain_energy_against_the_stress_readout(scene):
    from stark_amd import sim as S

    sim = S.Simulation(S.default_settings())
    if scene == "tet_beam":
        kind, prefix = 0, "EnergyTetStrain"
        beam = sim.add_volume_grid("beam", (0, 0, 0), (1.0, 0.25, 0.25), (12, 3, 3), S.soft_rubber())
        sim.prescribe_inside_aabb(beam, (-0.5, 0, 0), (2e-3, 2, 2), 1e7)
    else:
        kind, prefix = 1, "EnergyTriangleStrain"
        p = S.cotton_fabric()
        assert p.inflation == 0.0   # (the inflation term is in the potential's energy and not in psi)
        cloth = sim.add_surface_grid("cloth", (0.5, 0.5), (10, 10), p)
        sim.prescribe_inside_aabb(cloth, (0.25, 0.25, 0), (0.001, 0.001, 0.001), 1e6)
        sim.prescribe_inside_aabb(cloth, (-0.25, 0.25, 0), (0.001, 0.001, 0.001), 1e6)
    sim.record_stress(True)
    sim.record_budget(True)
    for _ in range(2):
        assert sim.run_one_step()
    rec, _ = sim.stress(kind)
    bud = sim.budget()
    names = [n for n in bud["potentials"] if n.startswith(prefix)]
    assert names and len(rec) > 0
    got = sum(bud["potentials"][n] for n in names)
    m_psi = rec[:, 13] * rec[:, 14]
    print("%s: strain energy %.12g against sum m psi %.12g" % (scene, got, m_psi.sum()))
    assert np.abs(m_psi).sum() > 0.0
    assert abs(got - m_psi.sum()) <= 1e-11 * np.abs(m_psi).sum()
    sim.close()


# ---- 7. nothing else moves ------------------------------------------------------------------------------------------------------------------------
def test_readout_is_reproducible_and_leaves_the_evaluation_alone():
    from gpu_util import engine_from_problem
    from oracle import evaluator as ev
    from stark_amd import capi

    path = os.path.join(GOLDEN, "contactmix_t0.npz")

    def sequence(readout):
        prob, man, z = ev.load_fixture(path)
        eng = engine_from_problem(prob, man)
        E, grad = eng.eval(capi.EVAL_P_G_H)
        if readout:
            pids = [eng.pot_ids[pi] for pi in sorted(eng.pot_ids)]
            first = [eng.energies([p]) for p in pids] + [eng.energies(None)]
            again = [eng.energies([p]) for p in pids] + [eng.energies(None)]
            for a, b in zip(first, again):
                assert np.array_equal(a, b)   # two readouts of one state: the same bits
            for pi, pid in eng.pot_ids.items():
                if prob.potentials[pi].name == "EnergyLumpedInertia":
                    ng = int(prob.potentials[pi].conn[:, 2].max()) + 1
                    assert np.array_equal(eng.inertia_budget(pid, ng, ABOUT), eng.inertia_budget(pid, ng, ABOUT))
            assert eng.counter("budget_readouts") > 0
        else:
            assert eng.counter("budget_readouts") == 0
        eng.assemble()
        bsr = eng.get_bsr()
        x, info = eng.pcg(man["pcg"]["abs_tol"])
        eng.close()
        return E, grad, bsr, x, info.n_iterations

    E0, g0, (rp0, c0, v0), x0, it0 = sequence(False)
    E1, g1, (rp1, c1, v1), x1, it1 = sequence(True)
    assert E0 == E1 and np.array_equal(g0, g1)
    assert np.array_equal(rp0, rp1) and np.array_equal(c0, c1) and np.array_equal(v0, v1)
    assert it0 == it1 and np.array_equal(x0, x1)


def _counter(sim, name):
    from stark_amd import capi

    v = C.c_int64()
    assert capi.lib().mistark_get_counter(sim.engine_handle(), name.encode(), C.byref(v)) == 0
    return v.value


def test_recording_does_not_change_a_trajectory_with_contact():
    from stark_amd import sim as S

    def run(record):
        st = S.default_settings()
        st.max_time_step_size = 0.01
        st.init_frictional_contact = 1
        sim = S.Simulation(st)
        gp = S.contact_global_params()
        gp.default_contact_thickness = 1e-3
        sim.set_contact_global_params(gp)
        sim.add_volume_grid("block", (0.0, 0.0, 0.05 + 1.5e-3), (0.12, 0.12, 0.1), (6, 6, 5), S.soft_rubber())
        box = sim.add_rigid_box("box", 1.0, (0.5, 0.5, 0.05))
        sim.rb_add_translation(box, (0.0, 0.0, -0.025))
        sim.rb_add_constraint("fix", box)
        if record:
            sim.record_budget(True)
        counts = []
        for _ in range(3):
            assert sim.run_one_step()
            i = sim.info()
            counts.append((i.total_newton_iterations, i.total_linear_solves, i.total_cg_iterations))
        out = sim.points("x0"), sim.points("v0"), counts, sim.contact_info()["n_contacts"], _counter(sim, "budget_readouts")
        if record:
            bud = sim.budget()
            assert [o["label"] for o in bud["objects"]] == ["block", "box"]
            assert any(n.startswith("contact_") for n in bud["potentials"])
        sim.close()
        return out

    x_off, v_off, c_off, n_off, r_off = run(False)
    x_on, v_on, c_on, n_on, r_on = run(True)
    assert r_off == 0 and r_on == 9   # three steps of three readouts: energies, the inertia potential, the bodies
    assert n_on > 0 and n_on == n_off
    assert c_on == c_off and np.array_equal(x_on, x_off) and np.array_equal(v_on, v_off)


# ---- 8. refusals ----------------------------------------------------------------------------------------------------------------------------------
def test_custom_other_and_duplicate_potentials_are_refused_by_name():
    import stark_amd
    from gpu_util import engine_from_problem
    from oracle import evaluator as ev

    path = os.path.join(GOLDEN, "tetbeam_eo_4x1x1.npz")
    prob, man, z = ev.load_fixture(path)
    eng = engine_from_problem(prob, man, custom_ops=z)
    pid = sorted(eng.pot_ids.values())[0]
    name = [prob.potentials[pi].name for pi, p in eng.pot_ids.items() if p == pid][0]
    for call in (lambda: eng.energies([pid]), lambda: eng.energies(None), lambda: eng.inertia_budget(pid, 1)):
        with pytest.raises(stark_amd.engine.EngineError, match=name) as e:
            call()
        assert "user-defined" in str(e.value)
    assert eng.counter("budget_readouts") == 0
    eng.close()
    eng = engine_from_problem(prob, man)
    names = {p: prob.potentials[pi].name for pi, p in eng.pot_ids.items()}
    other = [p for p, n in names.items() if n != "EnergyLumpedInertia"]
    assert other
    for p in other:
        with pytest.raises(stark_amd.engine.EngineError, match=names[p]) as e:
            eng.inertia_budget(p, 1)
        assert "not an EnergyLumpedInertia" in str(e.value)
    p = other[0]
    with pytest.raises(stark_amd.engine.EngineError, match=names[p]) as e:
        eng.energies([p, p])
    assert "listed twice" in str(e.value)
    with pytest.raises(stark_amd.engine.EngineError, match="bad potential id"):
        eng.energies([len(names) + 5])
    assert eng.counter("budget_readouts") == 0
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
        for call in (lambda: eng.energies(None), lambda: eng.energies([0]), lambda: eng.inertia_budget(0, 1), lambda: eng.rigid_budget(0, 0, 0, 0, 0, 0, 1)):
            with pytest.raises(stark_amd.engine.EngineError, match="single-rank"):
                call()
        eng.close()
    finally:
        L.mistark_local_group_destroy(group)
    h = C.c_void_p()
    assert L.mistark_create_dry(C.byref(h)) == 0
    try:
        out, about = (C.c_double * 13)(), (C.c_double * 3)()
        for rc in (L.mistark_energies(h, None, 0, out), L.mistark_inertia_budget(h, 0, about, 1, out), L.mistark_rigid_budget(h, 0, 0, 0, 0, 0, 0, 1, about, out)):
            assert rc < 0
            assert "registration-only" in L.mistark_last_error(h).decode()
    finally:
        L.mistark_destroy(h)


def test_budget_before_an_accepted_step_is_refused():
    from stark_amd import sim as S

    sim = S.Simulation(S.default_settings())
    sim.add_volume_grid("cube", (0, 0, 0), (0.1, 0.1, 0.1), (2, 2, 2), S.soft_rubber())
    with pytest.raises(S.SimError, match="recording is off"):
        sim.budget()
    sim.record_budget(True)
    with pytest.raises(S.SimError, match="no time step has been accepted"):
        sim.budget()
    assert sim.run_one_step()
    assert len(sim.budget()["objects"]) == 1
    sim.record_budget(False)
    with pytest.raises(S.SimError, match="recording is off"):
        sim.budget()
    sim.close()


# ---- 9. host mirror --------------------------------------------------------------------------------------------------------------------------------
def test_host_mirror_lists_the_objects_with_their_labels():
    from stark_amd import sim as S

    st = S.default_settings()
    st.init_frictional_contact = 0
    sim = S.Simulation(st)
    rubber, fabric = S.soft_rubber(), S.cotton_fabric()
    sim.add_volume_grid("cube", (0.0, 0.0, 1.0), (0.2, 0.3, 0.1), (3, 4, 2), rubber)
    sim.add_surface_grid("sheet", (0.5, 0.4), (6, 5), fabric)
    sim.add_rigid_box("crate", 3.0, (0.3, 0.2, 0.1))
    assert sim.run_one_step()
    assert _counter(sim, "budget_readouts") == 0   # recording off: nothing ran
    sim.record_budget(True, ABOUT)
    assert sim.run_one_step()
    assert _counter(sim, "budget_readouts") == 3
    bud = sim.budget()
    assert [(o["label"], o["kind"]) for o in bud["objects"]] == [("cube", "deformable"), ("sheet", "deformable"), ("crate", "rigid")]
    cube, sheet, crate = bud["objects"]
    # EnergyLumpedInertia::get_mass is density * the sum of the lumped volumes (areas for a surface): density * the measure of the grid
    assert abs(cube["mass"] - rubber.density * 0.2 * 0.3 * 0.1) <= 1e-12 * cube["mass"] and cube["count"] == 4 * 5 * 3 + 3 * 4 * 2   # (corners and cell centres)
    assert abs(sheet["mass"] - fabric.density * 0.5 * 0.4) <= 1e-12 * sheet["mass"] and sheet["count"] == 7 * 6
    assert crate["mass"] == 3.0 and crate["count"] == 1
    tot = bud["total"]
    assert tot["mass"] == cube["mass"] + sheet["mass"] + crate["mass"]
    assert tot["kinetic"] == cube["kinetic"] + sheet["kinetic"] + crate["kinetic"]
    assert tot["gravitational"] == cube["gravitational"] + sheet["gravitational"] + crate["gravitational"]
    assert np.array_equal(tot["momentum"], cube["momentum"] + sheet["momentum"] + crate["momentum"])
    assert np.array_equal(tot["angular_momentum"], cube["angular_momentum"] + sheet["angular_momentum"] + crate["angular_momentum"])
    # everything falls freely: after the second step of 10 ms every object moves down and its centre of mass is where its points are
    for o in bud["objects"]:
        assert o["momentum"][2] < 0.0 and o["kinetic"] > 0.0 and np.isfinite(o["com"]).all()
    assert "EnergyLumpedInertia" in bud["potentials"] and abs(bud["time"] - sim.info().current_time) < 1e-12
    sim.close()
