"""Stress readout on the GPU (include/mistark.h "stress readout", include/mistark_sim.h "stress recording"): element records and nodal averages of
the six strain potentials against closed-form answers, the numpy restatement of tests/stress_ref.py, the merged force readout and the engine's own
element energies.

Tolerances (stress_ref.check_records): stresses 1e-11 relative to max|reference| of the field over the potential, or to the reference's own terms
where it has cancelled; stretches |error| <= 1e-11 * stretch_max^2 / stretch_i (the route through the eigenvalues of C); flags exact except within
relative 1e-9 of the branch; nodal averages within 1e-12 * the sum of |terms| of the entry, as tests/test_gpu_forces.py sums."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import stress_ref as sr  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
LONG_ROW = 256  # STRESS_LONG_ROW of csrc/stress.hip
TOL = sr.ELEMENT_TOL


def _engine(prob):
    from gpu_util import engine_from_problem

    return engine_from_problem(prob)


# ---- 1. homogeneous deformation with a closed-form answer ---------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sr.NAMES)
def test_homogeneous_deformation(name):
    for prob, want in sr.homogeneous_cases(name):
        eng = _engine(prob)
        rec, kind = eng.element_stress(eng.pot_ids[0])
        assert kind == sr.KIND[name][0] and rec.shape == (prob.potentials[0].conn.shape[0], 16)
        sr.check_homogeneous(rec, want, name)
        eng.close()


# ---- 2. parity with the restatement on seeded inhomogeneous states --------------------------------------------------------------------------
@pytest.mark.parametrize("name", sr.NAMES)
def test_parity_with_restatement(name):
    prob, rec, terms, arg = sr.seeded_problem(name)
    if sr.KIND[name][1]:
        assert (rec[:, 15] == 1.0).any() and (rec[:, 15] == 0.0).any()   # limiting in some elements, not in others
    eng = _engine(prob)
    got, kind = eng.element_stress(eng.pot_ids[0])
    assert kind == sr.KIND[name][0]
    sr.check_records(got, rec, terms, arg, name)
    assert eng.counter("stress_readouts") == 1
    eng.close()


# ---- 3. consistency with the merged force readout and the element energies ---------------------------------------------------------------
@pytest.mark.parametrize("name", sr.NAMES[:2])
def test_stress_gives_the_element_forces(name):
    """f_a = -V_x sigma grad_x N_a, entry by entry, against Engine.element_forces(pid, 1 / dt)."""
    prob, rec, terms, arg = sr.seeded_problem(name)
    pot = prob.potentials[0]
    g = sr._tet_geometry(sr.gather(prob, pot))
    Dx = g["Dx1"]
    Dxi = np.linalg.inv(Dx)                       # rows: grad_x N_1..3
    grads = np.concatenate([-Dxi.sum(axis=1, keepdims=True), Dxi], axis=1)   # [n, node, 3]
    Vx = np.linalg.det(Dx) / 6.0
    cond = np.linalg.cond(Dx)

    def forces_of(records):
        s = records[:, 0:6]
        sig = np.stack([np.stack([s[:, 0], s[:, 3], s[:, 5]], axis=1), np.stack([s[:, 3], s[:, 1], s[:, 4]], axis=1), np.stack([s[:, 5], s[:, 4], s[:, 2]], axis=1)], axis=1)
        return -Vx[:, None, None] * np.einsum("nij,naj->nai", sig, grads)

    eng = _engine(prob)
    pid = eng.pot_ids[0]
    f, rows = eng.element_forces(pid, 1.0 / prob.dt)
    got, _ = eng.element_stress(pid)
    fmax = np.abs(f).max()
    err = np.abs(forces_of(got) - f).max(axis=(1, 2)) / fmax
    own = np.abs(forces_of(rec) - f).max(axis=(1, 2)) / fmax
    print("%s: worst error / (1e-11 cond) = %.3g; the restatement (A) itself leaves %.3g (cond up to %.3g)" % (name, (err / (TOL * cond)).max(), (own / (TOL * cond)).max(), cond.max()))
    assert (err <= TOL * cond).all()
    eng.close()


@pytest.mark.parametrize("name", sr.NAMES)
def test_energy_density_times_measure_is_the_element_energy(name):
    from stark_amd import capi

    prob, rec, terms, arg = sr.seeded_problem(name)
    eng = _engine(prob)
    pid = eng.pot_ids[0]
    eng.eval(capi.EVAL_P_G_H)
    E = eng.element_energies(pid, len(rec))
    got, _ = eng.element_stress(pid)
    err = np.abs(got[:, 13] * got[:, 14] + sr.inflation_energy(prob, prob.potentials[0]) - E).max() / np.abs(E).max()
    print("%s: m psi against the engine's element energies: rel %.3g" % (name, err))
    assert err < TOL
    eng.close()


# ---- 4. grid tails ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_elem", [1, 255, 256, 257])
@pytest.mark.parametrize("name", sr.NAMES)
def test_grid_tails(name, n_elem):
    prob, rec, terms, arg = sr.seeded_problem(name, n_elem)
    eng = _engine(prob)
    pid = eng.pot_ids[0]
    guard = 0x7FF8DEADBEEF0001
    buf = np.full(16 * (n_elem + 2), guard, dtype=np.uint64)
    ne, kind = C.c_int64(), C.c_int32()
    assert eng.L.mistark_potential_element_stress(eng.h, pid, buf.ctypes.data + 16 * 8, C.byref(ne), C.byref(kind)) == 0
    assert ne.value == n_elem
    assert (buf[:16] == guard).all() and (buf[-16:] == guard).all()       # elements that do not exist are not written
    got = buf[16:-16].view(np.float64).reshape(n_elem, 16)
    assert not (buf[16:-16] == guard).any()
    sr.check_records(got, rec, terms, arg, "%s n=%d" % (name, n_elem))
    eng.close()
    # ... nor on the device: the two potentials of a kind (an engine holds one potential per name) share one field-major record buffer, where a lane past
    # the end of one would land in the other's columns or in the next field. The nodal averages over both see every column of fields 0..8 and 14.
    other = [m for m in sr.NAMES if sr.KIND[m][0] == sr.KIND[name][0] and m != name][0]
    X, conn = sr.mesh_of(name)
    x0, v1, params = sr.seeded_state(name, X, conn, 1, affine=sr.SIZABLE)   # (entries that are a sizable part of their terms: see test 5)
    prob2 = sr.make_problem([(name, conn[:n_elem], params), (other, conn[n_elem:], sr.PARAMS[other])], X, x0, v1)
    rec2 = np.concatenate([sr.records(prob2, p)[0] for p in prob2.potentials])
    avg, mag = sr.nodal_average(len(X), np.concatenate([sr.block_rows(prob2, p) for p in prob2.potentials]), rec2)
    eng = _engine(prob2)
    out = eng.nodal_stress([eng.pot_ids[0], eng.pot_ids[1]])
    assert (np.abs(out - avg) <= 1e-12 * mag).all()
    eng.close()


# ---- 5. nodal averages ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 63, 64, 65, LONG_ROW - 1, LONG_ROW, LONG_ROW + 1, 300])
@pytest.mark.parametrize("kind", [0, 1])
def test_nodal_averages_on_fans(kind, n):
    """n tets around a common edge / n triangles around a common vertex: the shared rows collect n contributions each.

    The state: a stress entry is what is left of terms of the size of the moduli (c1 F F^T / J against lambda'(J - alpha) I), so two double
    evaluations of it agree to 1e-16 of THOSE, not of the entry. For the bound below, 1e-12 of the entries themselves against another evaluation
    (A), to test the summation and not the cancellation inside an element, every entry has to be a sizable part of its terms: a dilation with
    shear (stress_ref.SIZABLE: all six components about a fifth of their terms) plus the seeded noise. The same sums are also held to the GPU's
    own element records, where a term is an element value whatever has cancelled inside it."""
    name = ("EnergyTetStrain", "EnergyTriangleStrain")[kind]
    X, conn = (sr.tet_fan, sr.tri_fan)[kind](n)
    X = np.concatenate([X, [[1.0, 1.0, 1.0]]])   # a point no element touches
    x0, v1, params = sr.seeded_state(name, X, conn, 7, affine=sr.SIZABLE)
    prob = sr.make_problem([(name, conn, params)], X, x0, v1)
    pot = prob.potentials[0]
    rec, _, _ = sr.records(prob, pot)
    assert (rec[:, 15] < 2.0).all() and (rec[:, 14] > 0.0).all()
    rows = sr.block_rows(prob, pot)
    avg, mag = sr.nodal_average(len(X), rows, rec)
    eng = _engine(prob)
    out = eng.nodal_stress([eng.pot_ids[0]])
    assert out.shape == (len(X), 10)
    worst = (np.abs(out - avg) / np.maximum(mag, 1e-300)).max()
    print("%s fan of %d: worst |difference| / sum|terms| = %.3g" % (name, n, worst))
    assert (np.abs(out - avg) <= 1e-12 * mag).all()
    own, own_mag = sr.nodal_average(len(X), rows, eng.element_stress(eng.pot_ids[0])[0])
    assert (np.abs(out - own) <= 1e-12 * own_mag).all()
    shared = 2 if kind == 0 else 1
    assert (np.bincount(rows.reshape(-1), minlength=len(X))[:shared] == n).all()
    assert eng.counter("stress_long_rows") == (shared if n > LONG_ROW else 0)
    assert (out[-1] == 0.0).all()                 # untouched rows: ten exact zeros
    assert np.array_equal(out, eng.nodal_stress([eng.pot_ids[0]]))
    eng.close()


# ---- 6. leaves everything else alone ------------------------------------------------------------------------------------------------------
def test_readout_is_reproducible_and_leaves_the_evaluation_alone():
    from gpu_util import engine_from_problem
    from oracle import evaluator as ev
    from stark_amd import capi

    def sequence(readout):
        prob, man, z = ev.load_fixture(os.path.join(GOLDEN, "tetbeam_eo_4x1x1.npz"))
        eng = engine_from_problem(prob, man)
        pids = [pid for pi, pid in eng.pot_ids.items() if prob.potentials[pi].name in sr.KIND]
        assert pids

        def read():
            return [eng.element_stress(p)[0] for p in pids] + [eng.nodal_stress(pids)]

        first = read() if readout else None
        E, grad = eng.eval(capi.EVAL_P_G_H)
        if readout:
            for a, b in zip(first, read()):
                assert np.array_equal(a, b)       # two readouts of one state: the same bits
        eng.assemble()
        if readout:
            read()
        bsr = eng.get_bsr()
        x, info = eng.pcg(man["pcg"]["abs_tol"])
        assert eng.counter("stress_readouts") == (3 * (len(pids) + 1) if readout else 0)
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
            sim.record_stress(True)
        counts = []
        for _ in range(3):
            assert sim.run_one_step()
            i = sim.info()
            counts.append((i.total_newton_iterations, i.total_linear_solves, i.total_cg_iterations))
        out = sim.points("x0"), sim.points("v0"), counts, sim.contact_info()["n_contacts"], _counter(sim, "stress_readouts")
        if record:
            from test_gpu_forces import _EngineView, _pots

            rec, nodal = sim.stress(0)
            with _EngineView(sim) as (eng, desc):
                n_tets = sum(desc["potentials"][p]["n_elem"] for p in _pots(desc, "EnergyTetStrain"))
            assert n_tets > 0 and rec.shape == (n_tets, 16) and (rec[:, 14] > 0.0).all()
        sim.close()
        return out

    x_off, v_off, c_off, n_off, r_off = run(False)
    x_on, v_on, c_on, n_on, r_on = run(True)
    assert r_off == 0 and r_on == 3
    assert n_on > 0 and n_on == n_off
    assert c_on == c_off and np.array_equal(x_on, x_off) and np.array_equal(v_on, v_off)


# ---- 7. refusals --------------------------------------------------------------------------------------------------------------------------
def test_other_potentials_are_refused_by_name():
    import stark_amd
    from gpu_util import engine_from_problem
    from oracle import evaluator as ev

    prob, man, z = ev.load_fixture(os.path.join(GOLDEN, "tetbeam_eo_4x1x1.npz"))
    eng = engine_from_problem(prob, man)
    other = [(prob.potentials[pi].name, pid) for pi, pid in eng.pot_ids.items() if prob.potentials[pi].name not in sr.KIND]
    assert other
    for name, pid in other:
        for call in (lambda: eng.element_stress(pid), lambda: eng.nodal_stress([pid])):
            with pytest.raises(stark_amd.engine.EngineError, match=name) as e:
                call()
            assert "no stress readout" in str(e.value)
    assert eng.counter("stress_readouts") == 0
    eng.close()


def test_mixed_kinds_are_refused():
    import stark_amd

    X, tets = sr.tet_grid(1, 1, 1)
    tris = tets[:, :3]
    prob = sr.make_problem([("EnergyTetStrain_Elasticity_Only", tets, sr.PARAMS["EnergyTetStrain_Elasticity_Only"]),
                            ("EnergyTriangleStrain_Elasticity_Only", tris, sr.PARAMS["EnergyTriangleStrain_Elasticity_Only"])], X, X.copy(), np.zeros_like(X))
    eng = _engine(prob)
    with pytest.raises(stark_amd.engine.EngineError, match="mixes element kinds"):
        eng.nodal_stress([eng.pot_ids[0], eng.pot_ids[1]])
    assert eng.counter("stress_readouts") == 0
    assert eng.element_stress(eng.pot_ids[0])[1] == 0 and eng.element_stress(eng.pot_ids[1])[1] == 1   # one at a time they are served
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
        for call in (lambda: eng.element_stress(0), lambda: eng.nodal_stress([0])):
            with pytest.raises(stark_amd.engine.EngineError, match="single-rank"):
                call()
        eng.close()
    finally:
        L.mistark_local_group_destroy(group)
    h = C.c_void_p()
    assert L.mistark_create_dry(C.byref(h)) == 0
    try:
        ne, kind = C.c_int64(), C.c_int32()
        assert L.mistark_potential_element_stress(h, 0, None, C.byref(ne), C.byref(kind)) < 0
        assert "registration-only" in L.mistark_last_error(h).decode()
    finally:
        L.mistark_destroy(h)


# ---- 8. host mirror -----------------------------------------------------------------------------------------------------------------------
def test_host_mirror_records_the_clamped_beam():
    """The README's clamped beam: one record per tet, the energy sum equals the potential's energy at the recorded state (x0 before the step, the
    converged v1 — which the accepted step has made v0 —, through the restatement (A), which tests/test_stress_cpu.py holds to the oracle's
    energies), a nodal row per point."""
    from stark_amd import sim as S

    params = S.soft_rubber()
    sim = S.Simulation(S.default_settings())
    beam = sim.add_volume_grid("beam", (0, 0, 0), (1.0, 0.25, 0.25), (52, 13, 13), params)
    sim.prescribe_inside_aabb(beam, (-0.5, 0, 0), (2e-3, 2, 2), 1e7)
    assert sim.run_one_step()
    assert _counter(sim, "stress_readouts") == 0          # recording off: nothing ran
    sim.record_stress(True)
    x_before = sim.points("x0")
    dt = sim.info().dt
    assert sim.run_one_step()
    assert _counter(sim, "stress_readouts") == 1          # one launch sequence: the scene has tets only
    from test_gpu_forces import _EngineView, _first_row, _pots

    rec, nodal = sim.stress(0)
    with _EngineView(sim) as (eng, desc):
        n_tets = sum(desc["potentials"][p]["n_elem"] for p in _pots(desc, "EnergyTetStrain"))
    assert n_tets >= 52 * 13 * 13 * 5                      # one record per tet of the grid
    assert rec.shape == (n_tets, 16) and nodal.shape == (sim.info().n_points, 10)
    assert (rec[:, 15] < 2.0).all() and (rec[:, 14] > 0.0).all()
    assert (nodal[:, 9] > 0.0).all()                      # every point of the beam carries weight
    assert abs(nodal[:, 9].sum() - 4.0 * rec[:, 14].sum()) <= 1e-12 * 4.0 * rec[:, 14].sum()
    for k in (1, 2):
        r, nd = sim.stress(k)
        assert r.shape == (0, 16) and (nd == 0.0).all()
    # the same state through the restatement
    v1 = sim.points("v0")
    assert np.abs(sim.points("x0") - (x_before + dt * v1)).max() <= 1e-15
    with _EngineView(sim) as (eng, desc):
        (pid,) = [p for p in _pots(desc, "EnergyTetStrain") if desc["potentials"][p]["n_elem"] > 0]
        name = desc["potentials"][pid]["name"]
        _, rows = eng.element_forces(pid, 1.0)
        r0, _ = _first_row(desc, "soft.v1")
    conn = (rows - r0).astype(np.int32)
    p = dict(scale=params.scale, e=params.youngs_modulus, nu=params.poissons_ratio)
    if name == "EnergyTetStrain":
        p.update(strain_limit=params.strain_limit, sl_k=params.strain_limit_stiffness, damping=params.strain_damping)
    prob = sr.make_problem([(name, conn, p)], sim.points("X"), x_before, v1, dt)
    want, _, _ = sr.records(prob, prob.potentials[0])
    E_want, E_got = (want[:, 13] * want[:, 14]).sum(), (rec[:, 13] * rec[:, 14]).sum()
    print("clamped beam: energy %.12g against %.12g" % (E_got, E_want))
    assert abs(E_got - E_want) <= TOL * np.abs(want[:, 13] * want[:, 14]).sum()
    sim.close()


# ---- 9. frames ------------------------------------------------------------------------------------------------------------------------------
def _read_frame(path):
    """(points [n, 3], cells [n_cells, npc], cell data dict or None) of a legacy binary VTK frame."""
    raw = open(path, "rb").read()

    def section(key, at=0):
        i = raw.index(key, at)
        j = raw.index(b"\n", i)
        return raw[i:j].split(), j + 1

    head, at = section(b"POINTS")
    n = int(head[1])
    pts = np.frombuffer(raw, dtype=">f4", count=3 * n, offset=at).reshape(n, 3)
    head, at = section(b"CELLS", at + 12 * n)
    n_cells, total = int(head[1]), int(head[2])
    cells = np.frombuffer(raw, dtype=">i4", count=total, offset=at).reshape(n_cells, total // n_cells)[:, 1:]
    head, at = section(b"CELL_TYPES", at + 4 * total)
    at += 4 * n_cells + 1
    if at >= len(raw):
        return pts, cells, None
    head, at = section(b"CELL_DATA", at)
    assert int(head[1]) == n_cells
    data = {}
    for name in ("von_mises", "mean_stress", "stretch_max"):
        head, at = section(b"SCALARS", at)
        assert head[1] == name.encode() and head[2] == b"float"
        head, at = section(b"LOOKUP_TABLE", at)
        data[name] = np.frombuffer(raw, dtype=">f4", count=n_cells, offset=at)
        at += 4 * n_cells + 1
    head, at = section(b"TENSORS", at)
    assert head[1] == b"cauchy" and head[2] == b"float"
    data["cauchy"] = np.frombuffer(raw, dtype=">f4", count=9 * n_cells, offset=at).reshape(n_cells, 3, 3)
    assert at + 36 * n_cells + 1 == len(raw)
    return pts, cells, data


def _frame_scene(S, directory, record):
    st = S.default_settings()
    st.max_time_step_size = 0.01
    st.init_frictional_contact = 0
    st.enable_frame_writes = 1
    st.fps = 200                                   # a frame after every step
    st.output_directory = str(directory).encode()
    st.simulation_name = b"s"
    sim = S.Simulation(st)
    vol = sim.add_volume_grid("vol", (0.0, 0.0, 0.0), (0.3, 0.2, 0.2), (3, 2, 2), S.soft_rubber())
    sim.add_surface_grid("cloth", (0.4, 0.4), (4, 3), S.cotton_fabric())
    sim.add_line_as_segments("rod", (0.0, 0.5, 0.0), (0.5, 0.5, 0.1), 7, S.elastic_rubberband())
    sim.add_rigid_box("box", 1.0, (0.1, 0.1, 0.1))
    sim.prescribe_inside_aabb(vol, (-0.15, 0, 0), (2e-3, 2, 2), 1e7)
    if record is not None:
        sim.record_stress(record[0])
    assert sim.run_one_step()
    if record is not None:
        sim.record_stress(record[1])
    return sim


def test_frames_carry_the_recorded_stress(tmp_path):
    from stark_amd import sim as S
    from test_gpu_forces import _EngineView, _first_row, _pots

    sim = _frame_scene(S, tmp_path, (True, True))
    assert sim.run_one_step()
    x = sim.points("x0").astype(np.float32)
    expect = {"cloth": 1, "rod": 2}
    for label, kind in expect.items():
        rec, _ = sim.stress(kind)
        pts, cells, data = _read_frame(os.path.join(tmp_path, "s_%s_2.vtk" % label))
        assert data is not None and len(cells) == len(rec) > 0
        assert np.array_equal(data["von_mises"], rec[:, 6].astype(np.float32))
        assert np.array_equal(data["mean_stress"], rec[:, 7].astype(np.float32))
        assert np.array_equal(data["stretch_max"], rec[:, 9].astype(np.float32))
        s = rec[:, [0, 3, 5, 3, 1, 4, 5, 4, 2]].astype(np.float32).reshape(-1, 3, 3)
        assert np.array_equal(data["cauchy"], s)
        assert np.abs(rec[:, 6]).max() > 0.0
    # the volume's frame is its surface: a triangle shows the tet it is a face of
    rec, _ = sim.stress(0)
    pts, cells, data = _read_frame(os.path.join(tmp_path, "s_vol_2.vtk"))
    with _EngineView(sim) as (eng, desc):
        (pid,) = [p for p in _pots(desc, "EnergyTetStrain") if desc["potentials"][p]["n_elem"] > 0]
        _, rows = eng.element_forces(pid, 1.0)
        r0, _ = _first_row(desc, "soft.v1")
    tets = rows - r0
    assert len(tets) == len(rec)
    face_tet = {}
    for t, tet in enumerate(tets):
        for skip in range(4):
            face_tet.setdefault(tuple(sorted(np.delete(tet, skip))), []).append(t)
    vertex_of = {tuple(p): i for i, p in enumerate(x)}
    assert data is not None and len(cells) > 0
    for c, cell in enumerate(cells):
        owners = face_tet[tuple(sorted(vertex_of[tuple(pts[v])] for v in cell))]
        assert len(owners) == 1
        r = rec[owners[0]]
        assert data["von_mises"][c] == np.float32(r[6]) and data["mean_stress"][c] == np.float32(r[7]) and data["stretch_max"][c] == np.float32(r[9])
        assert np.array_equal(data["cauchy"][c], r[[0, 3, 5, 3, 1, 4, 5, 4, 2]].astype(np.float32).reshape(3, 3))
    # rigid bodies: zeros; the frame at initialisation, before anything was recorded: no cell data
    pts, cells, data = _read_frame(os.path.join(tmp_path, "s_box_2.vtk"))
    assert data is not None and all((v == 0.0).all() for v in data.values()) and len(data["von_mises"]) == len(cells)
    assert _read_frame(os.path.join(tmp_path, "s_cloth_0.vtk"))[2] is None
    sim.close()


def test_frames_with_recording_off_are_byte_identical(tmp_path):
    from stark_amd import sim as S

    a, b = tmp_path / "never", tmp_path / "switched_off"
    a.mkdir()
    b.mkdir()
    for directory, record in ((a, None), (b, (True, False))):
        sim = _frame_scene(S, directory, record)
        assert sim.run_one_step()
        sim.close()
    names = sorted(os.listdir(a))
    assert names == sorted(os.listdir(b)) and any(n.endswith("_2.vtk") for n in names)
    for n in names:
        same = open(a / n, "rb").read() == open(b / n, "rb").read()
        if n.endswith("_1.vtk"):
            assert not same, n     # recorded: the file carries cell data
            assert _read_frame(b / n)[2] is not None and _read_frame(a / n)[2] is None
        else:
            assert same, n
