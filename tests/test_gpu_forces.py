"""Force readout on the GPU (include/mistark.h "force readout", include/mistark_sim.h "force recording"): element, nodal and resultant forces
of any subset of potentials, against the numpy reference of tests/forces_ref.py, the engine's own evaluation, and identities of the physics.

Tolerances: element forces like every element quantity of the suite (1e-11 relative, 1e-8 for EnergyDiscreteShells); sums per row within
1e-12 * the sum of |terms| of that row (double rounding is 1.1e-16 per addition; rows have up to a few thousand terms here)."""
import ctypes as C
import json
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import forces_ref as fr  # noqa: E402
from fixture_list import stage_dumps  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
DUMPS = stage_dumps()
IDS = [os.path.basename(p)[:-4] for p in DUMPS]
LONG_ROW = 256  # FORCE_LONG_ROW of csrc/forces.hip: rows with more contributions are summed by a whole wavefront


def _engine(path):
    from gpu_util import engine_from_problem

    prob, man, z, scale, per, total, mag = fr.reference(path)
    return engine_from_problem(prob, man), prob, man, z, scale, per, total


def _within(a, b, mag, what=""):
    """|a - b| <= 1e-12 * mag, entry by entry (entries nobody contributes to are exactly equal)."""
    err = np.abs(np.asarray(a) - np.asarray(b))
    worst = float((err / np.maximum(mag, 1e-300)).max()) if err.size else 0.0
    print("%s: worst |difference| / sum|terms| = %.3g" % (what, worst))
    assert (err <= 1e-12 * mag).all(), (what, worst)


# ---- 1. parity against the reference ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", DUMPS, ids=IDS)
def test_element_forces_match_reference(path):
    eng, prob, man, z, scale, per, _ = _engine(path)
    assert sorted(eng.pot_ids) == sorted(per)
    for pi, pid in eng.pot_ids.items():
        name = prob.potentials[pi].name
        r = per[pi]
        f, rows = eng.element_forces(pid, scale)
        assert f.shape == r["f"].shape, name
        assert (rows == r["rows"]).all(), name
        assert (rows[r["active"]] == r["rows_active"]).all(), name
        assert (f[~r["active"]] == 0.0).all(), name
        if r["active"].any():
            nb = rows.shape[1]
            got = f[r["active"]].reshape(-1, 3 * nb)
            # (relative to max|reference| — or, where the reference cancels to rounding noise, to its terms: forces_ref.term_scale)
            tol = fr.ELEMENT_TOL.get(name, 1e-11)
            err = fr.rel_to_scale(got, -scale * r["g_active"], scale * r["term_scale"], tol)
            print("%s: element forces rel %.3g (to max|reference| alone: %.3g)" % (name, err, fr.rel(got, -scale * r["g_active"])))
            assert err < tol, name
    assert eng.counter("force_readouts") == len(eng.pot_ids)
    eng.close()


# ---- 2. nodal sums ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", DUMPS, ids=IDS)
def test_nodal_forces(path):
    from stark_amd import capi

    eng, prob, man, z, scale, per, _ = _engine(path)
    ndofs = prob.ndofs
    mag_all = np.zeros(ndofs)
    mag_eval = np.zeros(ndofs)
    own_sum = np.zeros(ndofs)
    for pi, pid in eng.pot_ids.items():
        f_el, rows = eng.element_forces(pid, scale)
        want, mag = fr.scatter(ndofs, rows, f_el)
        # Between two EVALUATIONS of an element (eval()'s closed forms against the generic expression) the terms of a row are those of the element
        # expressions. Where an element force has cancelled to rounding noise (fixtures at rest: forces_ref.term_scale) it does not measure them;
        # such a potential counts with the magnitude of its terms. Everywhere else, and in every comparison of sums of the SAME element
        # forces, a term is an element force.
        if fr.cancelled(per[pi], prob.potentials[pi].name):
            mag_eval += fr.scatter(ndofs, rows, np.full(f_el.shape, scale * per[pi]["term_scale"]))[0]
        else:
            mag_eval += mag
        f = eng.forces([pid], scale)
        _within(f, want, mag, prob.potentials[pi].name)
        assert (f[mag == 0.0] == 0.0).all()
        mag_all += mag
        own_sum += want
    f_all = eng.forces(None, scale)
    err = fr.rel(f_all, -scale * z["grad"])
    print("all potentials against the reference gradient: rel %.3g" % err)
    assert err < fr.gradient_tolerance(man)
    _within(f_all, own_sum, mag_all, "all potentials against the scatter of their element forces")
    # the engine's own evaluation of the same context (closed-form kernels where it has them, its own summation)
    _, grad = eng.eval(capi.EVAL_P_G)
    _within(f_all, -scale * grad, mag_eval, "all potentials against eval(P_G)")
    # disjoint groups add up to their union
    pids = [eng.pot_ids[pi] for pi in sorted(eng.pot_ids)]
    a, b = pids[0::2], pids[1::2]
    if b:
        _within(eng.forces(a, scale) + eng.forces(b, scale), eng.forces(a + b, scale), mag_all, "two groups against their union")
        _within(eng.forces(a + b, scale), f_all, mag_all, "the union against all")
    eng.close()


# ---- 3. row lengths around 64 and around the lane-per-row limit ----------------------------------------------------------------------
class _EngineView:
    """The engine of a Simulation behind stark_amd.Engine's methods (the simulation owns the context)."""

    def __init__(self, sim):
        import stark_amd

        self.e = stark_amd.Engine.__new__(stark_amd.Engine)
        self.e.L = stark_amd.capi.lib()
        self.e.h = sim.engine_handle()
        self.e._keep = []
        n = self.e.L.mistark_describe(self.e.h, None, 0)
        buf = C.create_string_buffer(int(n))
        self.e.L.mistark_describe(self.e.h, buf, n)
        self.desc = json.loads(buf.value.decode())

    def __enter__(self):
        return self.e, self.desc

    def __exit__(self, *a):
        self.e.h = None  # (not ours to destroy)


def _first_row(desc, label):
    at = 0
    for s in desc["dof_sets"]:
        if s["label"] == label:
            return at // 3, s["n"] // 3
        at += s["n"]
    raise KeyError(label)


def _pots(desc, prefix):
    return [i for i, p in enumerate(desc["potentials"]) if p["name"].startswith(prefix)]


@pytest.mark.parametrize("n_att", [1, 63, 64, 65, LONG_ROW - 1, LONG_ROW, LONG_ROW + 1, 4 * LONG_ROW + 1])
def test_row_length_boundaries(n_att):
    """One rigid body attached to N points of a cloth: its two rows (v1, w1) collect N contributions each."""
    from stark_amd import sim as S

    st = S.default_settings()
    st.init_frictional_contact = 0
    sim = S.Simulation(st)
    cloth = sim.add_surface_grid("cloth", (1.0, 1.0), (32, 32), S.cotton_fabric())  # 33 x 33 = 1089 points
    box = sim.add_rigid_box("box", 1.0, (0.3, 0.2, 0.1))
    sim.rb_add_rotation(box, 20.0, (0.3, 1.0, 0.2))
    sim.attach_rigid_body(box, cloth, list(range(n_att)), 1e4, 0.0)
    sim.rb_add_translation(box, (0.01, -0.02, 0.03))  # (after attaching: every attachment is stretched)
    sim.prepare()
    sim.begin_time_step()
    scale = 1.0 / sim.info().dt
    with _EngineView(sim) as (eng, desc):
        (pid,) = _pots(desc, "EnergyAttachments_rb_d")
        assert desc["potentials"][pid]["n_elem"] == n_att
        rv, n_rb = _first_row(desc, "rigid.v1")
        rw, _ = _first_row(desc, "rigid.w1")
        assert n_rb == 1
        f_el, rows = eng.element_forces(pid, scale)
        assert (np.abs(f_el).max(axis=(1, 2)) > 0.0).all()   # every attachment pulls
        assert (rows == rv).sum() == n_att and (rows == rw).sum() == n_att
        want, mag = fr.scatter(eng.ndofs, rows, f_el)
        f = eng.forces([pid], scale)
        body = np.r_[3 * rv:3 * rv + 3, 3 * rw:3 * rw + 3]
        assert (np.abs(want[body]) > 0).all()
        _within(f[body], want[body], mag[body], "the body's rows, N = %d" % n_att)
        _within(f, want, mag, "all rows, N = %d" % n_att)
        # the N-long rows took the path meant for them
        assert eng.counter("force_long_rows") == (2 if n_att > LONG_ROW else 0)
        # ... also beside every other potential of the scene (the body's rows then start anywhere in a wavefront's 64 positions)
        f_all = eng.forces(None, scale)
        mag_all, want_all = np.zeros(eng.ndofs), np.zeros(eng.ndofs)
        for p in range(len(desc["potentials"])):
            fe, r = eng.element_forces(p, scale)
            if len(fe):
                w, m = fr.scatter(eng.ndofs, r, fe)
                want_all += w
                mag_all += m
        _within(f_all, want_all, mag_all, "all potentials, N = %d" % n_att)
        assert eng.counter("force_long_rows") >= (2 if n_att > LONG_ROW else 0)
    sim.close()


# ---- 4. reproducibility and isolation -------------------------------------------------------------------------------------------------
def test_readout_is_reproducible_and_leaves_the_evaluation_alone():
    from stark_amd import capi

    path = os.path.join(GOLDEN, "contactmix_t0.npz")

    def sequence(readout):
        eng, prob, man, z, scale, per, _ = _engine(path)
        E, grad = eng.eval(capi.EVAL_P_G_H)
        if readout:
            pids = [eng.pot_ids[pi] for pi in sorted(eng.pot_ids)]
            first = [eng.forces([p], scale) for p in pids] + [eng.forces(None, scale)]
            again = [eng.forces([p], scale) for p in pids] + [eng.forces(None, scale)]
            for a, b in zip(first, again):
                assert np.array_equal(a, b)   # two readouts of one state: the same bits
            el = [eng.element_forces(p, scale)[0] for p in pids]
            for p, a in zip(pids, el):
                assert np.array_equal(a, eng.element_forces(p, scale)[0])
            rows = np.arange(eng.ndofs // 3, dtype=np.int32)
            assert np.array_equal(eng.forces_resultant(None, scale, rows), eng.forces_resultant(None, scale, rows))
            assert eng.counter("force_readouts") > 0
        else:
            assert eng.counter("force_readouts") == 0
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


def _block_on_box(S, groups, mu=0.0, vx=0.0, n_steps=5):
    """A soft block of 6 x 6 x 5 cells 1.5 mm above a fixed rigid box, dropped (and pushed sideways) for a few steps of 10 ms."""
    st = S.default_settings()
    st.max_time_step_size = 0.01
    st.init_frictional_contact = 1
    sim = S.Simulation(st)
    gp = S.contact_global_params()
    gp.default_contact_thickness = 1e-3
    sim.set_contact_global_params(gp)
    block = sim.add_volume_grid("block", (0.0, 0.0, 0.05 + 1.5e-3), (0.12, 0.12, 0.1), (6, 6, 5), S.soft_rubber())
    box = sim.add_rigid_box("box", 1.0, (0.5, 0.5, 0.05))
    sim.rb_add_translation(box, (0.0, 0.0, -0.025))
    sim.rb_add_constraint("fix", box)
    if mu > 0.0:
        sim.set_friction(sim.contact_group("d", block), sim.contact_group("rb", box), mu)
    if vx != 0.0:
        v = sim.points("v0")
        v[:, 0] = vx
        sim.set_points("v0", v)
    if groups is not None:
        sim.record_forces(groups)
    out = dict(forces=[], info=[], counts=[])
    for _ in range(n_steps):
        assert sim.run_one_step()
        i = sim.info()
        assert i.last_newton_result == 0
        out["counts"].append((i.total_newton_iterations, i.total_linear_solves, i.total_cg_iterations))
        out["info"].append(sim.contact_info())
        if groups is not None:
            out["forces"].append([sim.forces(g) for g in range(len(groups))])
    out["x0"] = sim.points("x0")
    v = C.c_int64()
    from stark_amd import capi

    assert capi.lib().mistark_get_counter(sim.engine_handle(), b"force_readouts", C.byref(v)) == 0
    out["force_readouts"] = v.value
    return sim, out


GROUPS = ["contact_", "friction_", "EnergyTetStrain"]


def test_recording_does_not_change_the_simulation():
    from stark_amd import sim as S

    sim0, off = _block_on_box(S, None, mu=0.5, vx=0.2)
    sim0.close()
    sim1, on = _block_on_box(S, GROUPS, mu=0.5, vx=0.2)
    sim1.close()
    assert off["force_readouts"] == 0
    assert on["force_readouts"] > 0
    assert on["counts"] == off["counts"]
    assert np.array_equal(on["x0"], off["x0"])
    assert on["info"][-1]["n_contacts"] > 0


# ---- 5. Newton's third law through the device-resident tables -------------------------------------------------------------------------
def test_third_law_and_resultants():
    from stark_amd import sim as S

    sim, out = _block_on_box(S, GROUPS, mu=0.5, vx=0.2)
    last = max(k for k, i in enumerate(out["info"]) if i["n_contacts"] > 0 and i["n_friction_contacts"] > 0)
    assert out["info"][last]["n_contacts"] > 0 and out["info"][last]["n_friction_contacts"] > 0
    (pc, rc), (pf, rf), (pt, rt) = out["forces"][last]
    for what, pts, rb in (("contact_", pc, rc), ("friction_", pf, rf)):
        total = pts.sum(axis=0) + rb[0, :3]
        bound = 1e-12 * (np.abs(pts).sum() + np.abs(rb[:, :3]).sum())
        print("%s: sum over block and box %s, sum|f| %.6g" % (what, total, bound / 1e-12))
        assert np.abs(pts).sum() > 0.0, what
        assert (np.abs(total) <= bound).all(), what
    # barrier forces push the block up and the box down; lagged friction opposes the push
    assert pc.sum(axis=0)[2] > 0.0 and rc[0, 2] < 0.0
    assert pf.sum(axis=0)[0] < 0.0
    # internal forces of the block: no resultant, and none on the box
    assert np.abs(pt).sum() > 0.0
    assert (np.abs(pt.sum(axis=0)) <= 1e-12 * np.abs(pt).sum()).all()
    assert (rt == 0.0).all()
    # resultants over the block's rows, at the engine's current state (the step has been accepted: another state than the recorded one, the
    # tables as installed)
    scale = 1.0 / sim.info().dt
    x = sim.points("x0")
    with _EngineView(sim) as (eng, desc):
        r0, n_pts = _first_row(desc, "soft.v1")
        assert n_pts == len(x)
        rows = np.arange(r0, r0 + n_pts, dtype=np.int32)
        about = np.array([0.01, -0.02, 0.03])
        for prefix in GROUPS:
            pids = [p for p in _pots(desc, prefix) if desc["potentials"][p]["n_elem"] > 0]
            if not pids:
                continue
            f = eng.forces(pids, scale).reshape(-1, 3)[rows]
            res = eng.forces_resultant(pids, scale, rows)
            assert (np.abs(res[:3] - f.sum(axis=0)) <= 1e-12 * np.abs(f).sum()).all(), prefix
            assert (res[3:] == 0.0).all()
            res = eng.forces_resultant(pids, scale, rows, x, about)
            arm = x - about
            tq = np.cross(arm, f)
            tq_mag = (np.abs(arm)[:, [1, 2, 0]] * np.abs(f)[:, [2, 0, 1]] + np.abs(arm)[:, [2, 0, 1]] * np.abs(f)[:, [1, 2, 0]]).sum(axis=0)
            assert (np.abs(res[:3] - f.sum(axis=0)) <= 1e-12 * np.abs(f).sum()).all(), prefix
            assert (np.abs(res[3:] - tq.sum(axis=0)) <= 1e-12 * tq_mag).all(), prefix
            # a reversed list: the same sums (another order), an out-of-range row: an error
            res_r = eng.forces_resultant(pids, scale, rows[::-1].copy(), x[::-1].copy(), about)
            assert (np.abs(res_r - res) <= 1e-12 * np.r_[np.abs(f).sum() * np.ones(3), tq_mag]).all()
        import stark_amd

        with pytest.raises(stark_amd.engine.EngineError, match="outside"):
            eng.forces_resultant(None, scale, [eng.ndofs // 3])
    sim.close()


# ---- 6. refusals ------------------------------------------------------------------------------------------------------------------------
def test_custom_potential_is_refused_by_name():
    import stark_amd
    from gpu_util import engine_from_problem

    prob, man, z, scale, per, _, _ = fr.reference(os.path.join(GOLDEN, "tetbeam_eo_4x1x1.npz"))
    eng = engine_from_problem(prob, man, custom_ops=z)
    pid = sorted(eng.pot_ids.values())[0]
    name = [prob.potentials[pi].name for pi, p in eng.pot_ids.items() if p == pid][0]
    for call in (lambda: eng.forces([pid], scale), lambda: eng.forces(None, scale), lambda: eng.element_forces(pid, scale),
                 lambda: eng.forces_resultant([pid], scale, [0])):
        with pytest.raises(stark_amd.engine.EngineError) as e:
            call()
        assert "user-defined" in str(e.value)
    with pytest.raises(stark_amd.engine.EngineError, match=name):
        eng.forces([pid], scale)
    assert eng.counter("force_readouts") == 0
    eng.close()


def test_sharded_context_is_refused():
    import stark_amd
    from stark_amd import capi

    L = capi.lib()
    group = L.mistark_local_group_create(2)
    try:
        eng = stark_amd.Engine(0)
        eng.dist_init_local(group, 0)
        u = np.zeros(6)
        eng.add_dof_set("u", u)
        for call in (lambda: eng.forces(None, 1.0), lambda: eng.element_forces(0, 1.0), lambda: eng.forces_resultant(None, 1.0, [0])):
            with pytest.raises(stark_amd.engine.EngineError, match="single-rank"):
                call()
        eng.close()
    finally:
        L.mistark_local_group_destroy(group)


def test_empty_table_gives_zeros_without_a_launch():
    from gpu_util import engine_from_problem

    prob, man, z, scale, per, _, _ = fr.reference(os.path.join(GOLDEN, "contactmix_t0.npz"))
    eng = engine_from_problem(prob, man)
    pi = sorted(k for k in eng.pot_ids if "contact" in prob.potentials[k].name)[0]
    pot = prob.potentials[pi]
    pid = eng.pot_ids[pi]
    eng.set_dynamic(pid, True)
    eng.update_connectivity(pid, pot.conn[:0])   # the table runs empty, as a contact table does when its pairs separate
    f = eng.forces([pid], scale)
    assert f.shape == (prob.ndofs,) and (f == 0.0).all()
    f_el, rows = eng.element_forces(pid, scale)
    assert f_el.shape[0] == 0 and rows.shape[0] == 0
    assert (eng.forces_resultant([pid], scale, [0, 1]) == 0.0).all()
    assert eng.counter("force_readouts") == 0
    # beside the others it contributes nothing
    others = [p for k, p in eng.pot_ids.items() if k != pi]
    assert np.array_equal(eng.forces(None, scale), eng.forces(others, scale))
    assert eng.counter("force_readouts") == 2
    eng.close()
