"""GPU (-m gpu): the PSD projection kernels of stark_amd/csrc/project.hip on element Hessians whose spectra are KNOWN (tests/psd_cases.py; the
cases and references are proved on the CPU by tests/test_psd_cases_cpu.py), at the list lengths and launch boundaries the kernels branch on.

The bound. The kernels stop at off(A) <= JACOBI_OFF_TOL ||A||_F^2 and return f(V D V^T) for an orthogonal V; clamping to eps (eps I + the projection
onto the PSD cone) and mirroring (the matrix absolute value, away from its jump at eps) are 1-Lipschitz in the Frobenius norm. A correct kernel's
result is therefore within
      ||H_in - H_exact||_F  +  sqrt(JACOBI_OFF_TOL) ||H||_F  +  rounding ||H||_F
of the exact projection of H_exact: the first term measured per element from the unprojected read-back, the second the constant's (1e-12 ||H||),
the third 8 x the error of a float64 restatement of the same Jacobi against the exact projection, per spectrum family and NB (floor
8 * 2^-52 * 3 NB; tests/psd_tolerances.json). The factor 8 is the project's margin for device arithmetic a few ulp from the host's (FMA contraction,
the rcp / rsq estimates with Newton steps); it is a margin over the reference's rounding, never fitted to what the kernels return. Every figure is
printed against its bound.

 a. every spectrum family, NB = 1..8, both rules, proj_variant 0 (registers, batched), 1 (LDS), 2 (stand-alone launch), 4 (IEEE division), 7;
 b. an element's projected bits do not depend on its neighbours: alone, first of a full group, last of a partial group, shifted by one group,
    registered in reversed order; list lengths 1, EPW - 1, EPW, EPW + 1, 4 EPW - 1, 4 EPW, 4 EPW + 1;
 c. selection by active rows over three rounds;
 d. SHORT_LIST against SHORT_LIST + 1 elements, PROJ_BATCH + 5 potentials in one round (second flush, first_wave after it), the ordered matrix
    update behind them (second and third MARK_BATCH flush), the atomic update within float rounding of it;
 e. the translation-invariant (Helmert-reduced) kernels on built-in tets and membrane triangles in synthesised, partly inverted states.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import psd_cases as pc  # noqa: E402

pytestmark = pytest.mark.gpu

ULP = 2.0 ** -52
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _fro(M):
    return np.sqrt((M * M).sum(axis=(1, 2)))


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _same_bits(a, b):
    return bool((_bits(a) == _bits(b)).all())


def _engine(cases, **options):
    """One engine holding the cases as potentials over one DoF set (every element owns its nodes); returns (engine, potential ids, first node of each)."""
    from stark_amd.engine import Engine

    eng = Engine(0)
    x = np.ascontiguousarray(np.concatenate([c.x for c in cases]))
    eng.add_dof_set("x", x)
    a_x = eng.L.mistark_dof_array(eng.h, 0, 3)
    pids, first = [], []
    off = 0
    for k, c in enumerate(cases):
        conn = c.conn.copy()
        conn[:, :c.nb] += off
        ids = [eng.array(a, a.shape[1]) for a in c.arrays]
        bind = [(a_x if isinstance(a, str) else ids[a], s, col) for a, s, col in c.bindings]
        pids.append(eng.potential_custom("%s#%d" % (c.name, k), np.ascontiguousarray(conn), bind, c.ops, c.consts, c.n_inputs))
        first.append(off)
        off += c.x.shape[0]
    eng.set_option("custom_rtc", 0)            # the device interpreter: no compilation inside a test
    for k, v in options.items():
        eng.set_option(k, v)
    eng.n_nodes = off
    return eng, pids, first


def _read(eng, pids, cases):
    return [eng.element_hessians(pid, c.n_elem)[0].copy() for pid, c in zip(pids, cases)]


def _eval(eng):
    from stark_amd import capi

    eng.eval(capi.EVAL_P_G_H)


def _check_against_exact(tag, family, nb, mirroring, H_in, H_out, ne=None):
    """bound, symmetry, untouched elements, smallest eigenvalue; returns the number of elements that count as changed"""
    ex = pc.exact(family, nb, ne)
    n = 3 * nb
    assert np.isfinite(H_out).all()
    if family in pc.DIAG:                       # the interpreter's Hessian is diag(d) + the placed entries to the bit: `l < eps` is decided AT eps
        assert (H_in == ex.H).all(), (tag, family)
    b = pc.bound(family, nb, ex.fro, _fro(H_in - ex.H))
    err = _fro(H_out - ex.P[mirroring])
    worst = int(np.argmax(err - b))
    print("%s %-18s |P - P_exact| %.3g of %.3g (||H|| %.3g, H_in error %.3g, rounding term %.3g ||H||)" % (
        tag, family, err[worst], b[worst], ex.fro[worst], _fro(H_in - ex.H)[worst], pc.rounding_tolerance(family, nb)))
    assert (err <= b).all(), (tag, family, worst, err[worst], b[worst])
    assert _same_bits(H_out, np.transpose(H_out, (0, 2, 1)))                         # symmetric to the bit
    assert _same_bits(H_out[~ex.changed], H_in[~ex.changed])                         # untouched, to the bit
    fl = np.where(ex.lam < pc.EPS, -ex.lam if mirroring else pc.EPS, ex.lam).min(axis=1)
    if not mirroring:
        assert (fl >= pc.EPS).all()
    lo = np.linalg.eigvalsh(H_out).min(axis=1)
    slack = b + 4 * ULP * n * _fro(H_out)                                             # (+ eigvalsh's own backward error)
    k = int(np.argmin(lo - fl + slack))
    print("%s %-18s smallest eigenvalue %.6g, at least %.6g - %.3g" % (tag, family, lo[k], fl[k], slack[k]))
    assert (lo >= fl - slack).all(), (tag, family, k, lo[k], fl[k], slack[k])
    return int(ex.changed.sum())


# ---- a. spectra, every path ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mirroring", [0, 1], ids=["clamp", "mirror"])
@pytest.mark.parametrize("variant", [0, 1, 2, 4, 7])
@pytest.mark.parametrize("nb", pc.NBS)
def test_spectra_on_every_path(nb, variant, mirroring):
    """Every family on 4 EPW + 1 elements, one potential each, in one round. NB = 7, 8 reach only the LDS kernel whatever the variant."""
    cases = [pc.make_case(f, nb) for f in pc.FAMILIES]
    eng, pids, _ = _engine(cases, proj_variant=variant)
    _eval(eng)
    H_in = _read(eng, pids, cases)
    n_proj, n_changed = eng.project(pc.EPS, bool(mirroring), None)
    H_out = _read(eng, pids, cases)
    again = eng.project(pc.EPS, bool(mirroring), None)
    H_again = _read(eng, pids, cases)
    eng.close()
    tag = "NB=%d v=%d %s" % (nb, variant, "mirror" if mirroring else "clamp")
    expect_changed = 0
    for f, hi, ho, ha in zip(pc.FAMILIES, H_in, H_out, H_again):
        assert len(hi) == 4 * pc.epw(nb) + 1
        expect_changed += _check_against_exact(tag, f, nb, mirroring, hi, ho)
        assert _same_bits(ho, ha), f                                                  # a second project() changes no bit
    assert n_proj == sum(c.n_elem for c in cases)
    assert n_changed == expect_changed, (n_changed, expect_changed)
    assert again == (0, 0)


# ---- b. neighbours do not matter -------------------------------------------------------------------------------------------------------------
def _mask(n_nodes, nb, elems, first=0):
    m = np.zeros(n_nodes, dtype=np.uint8)
    for e in elems:
        m[first + e * nb:first + (e + 1) * nb] = 1
    return m


@pytest.mark.parametrize("family", ["mixed", "repeated"])
@pytest.mark.parametrize("nb", [2, 3, 4, 5])
def test_an_elements_result_does_not_depend_on_its_neighbours(nb, family):
    """NB = 2, 3, 4 leave idle tail lanes in the wavefront (64 is no multiple of even(3 NB)), NB = 5 none. `repeated` needs the most sweeps and its
    elements converge at different ones: a converged group has to apply identity rotations while its neighbours go on."""
    E = pc.epw(nb)
    case = pc.make_case(family, nb)
    ne = case.n_elem
    assert ne == 4 * E + 1 and ne <= 64                      # one wavefront of the selection kernel: the list is in element order
    ex = pc.exact(family, nb)
    eng, (pid,), _ = _engine([case])
    _eval(eng)
    H0 = _read(eng, [pid], [case])[0]

    def round_of(elems):
        _eval(eng)
        n_proj, n_changed = eng.project(pc.EPS, False, _mask(eng.n_nodes, nb, elems))
        assert n_proj == len(elems) and n_changed == int(ex.changed[list(elems)].sum())
        return _read(eng, [pid], [case])[0]

    alone = H0.copy()
    for e in range(ne):
        H = round_of([e])
        rest = np.arange(ne) != e
        assert _same_bits(H[rest], H0[rest])
        alone[e] = H[e]
    _check_against_exact("NB=%d alone" % nb, family, nb, 0, H0, alone)
    for L in (1, E - 1, E, E + 1, 4 * E - 1, 4 * E, 4 * E + 1):
        H = round_of(range(L))
        assert _same_bits(H[:L], alone[:L]), L               # element 0: first of a full group; element L - 1: last of a partial one
        assert _same_bits(H[L:], H0[L:]), L                  # not in the list: untouched
    H = round_of(range(1, ne))                               # every element one group earlier than in the full list
    assert _same_bits(H[1:], alone[1:]) and _same_bits(H[:1], H0[:1])
    H = round_of(range(E - 1, ne, 2))                        # only changed or only unchanged elements share the wavefronts
    sel = np.zeros(ne, dtype=bool)
    sel[E - 1::2] = True
    assert _same_bits(H[sel], alone[sel]) and _same_bits(H[~sel], H0[~sel])
    eng.close()
    # the same elements registered in reversed order: every element in another lane group, beside other neighbours
    rev = pc.make_case(family, nb, reverse=True)
    eng, (pid,), _ = _engine([rev])
    _eval(eng)
    R0 = _read(eng, [pid], [rev])[0]
    assert _same_bits(R0[::-1], H0)
    assert eng.project(pc.EPS, False, None) == (ne, int(ex.changed.sum()))
    R = _read(eng, [pid], [rev])[0]
    eng.close()
    assert _same_bits(R[::-1], alone)


# ---- c. selection by active rows -------------------------------------------------------------------------------------------------------------
def test_selection_by_active_rows_over_three_rounds():
    """549 elements of two nodes: three workgroups of the selection kernel, the last one partial; wavefronts with none, some and all lanes selected."""
    nb, ne, family = 2, 2 * 256 + 37, "mixed"
    case = pc.make_case(family, nb, ne=ne)
    changed = (pc.spectrum(family, nb, ne) < pc.EPS).any(axis=1)
    rng = np.random.default_rng(11)
    s1 = rng.random(ne) < 0.4
    s1[64:128] = False                                        # a wavefront with no lane selected
    s1[128:192] = True                                        # ... and one with all
    s2 = rng.random(ne) < 0.5
    s2[64:128] = True
    eng, (pid,), _ = _engine([case])
    _eval(eng)
    H_prev = _read(eng, [pid], [case])[0]
    done = np.zeros(ne, dtype=bool)
    total = 0
    for rnd, s in enumerate((s1, s2, None)):
        if s is None:
            mask, want = None, ~done
        else:
            mask = np.zeros(eng.n_nodes, dtype=np.uint8)       # ONE node of the element is enough; which one varies
            el = np.flatnonzero(s)
            mask[el * nb + (el % nb)] = 1
            both = el[el % 3 == 0]
            mask[both * nb] = mask[both * nb + 1] = 1
            want = s & ~done
        n_proj, n_changed = eng.project(pc.EPS, False, mask)
        H = _read(eng, [pid], [case])[0]
        moved = (_bits(H) != _bits(H_prev)).any(axis=(1, 2))
        print("round %d: projected %d of %d, changed %d" % (rnd, n_proj, ne, n_changed))
        assert n_proj == int(want.sum()) and n_changed == int((want & changed).sum())
        assert (moved == (want & changed)).all()
        done |= want
        total += n_proj
        H_prev = H
    assert total == ne and done.all()
    assert eng.project(pc.EPS, False, None) == (0, 0)
    eng.close()


# ---- d. launch boundaries --------------------------------------------------------------------------------------------------------------------
def test_short_list_threshold_batched_against_stand_alone_launch():
    """NB = 1: SHORT_LIST elements go through the batched launch, SHORT_LIST + 1 through k_project_eig_cols: the shared elements have the same bits."""
    nb, family = 1, "mixed"
    ne = pc.SHORT_LIST + 1
    case = pc.make_case(family, nb, ne=ne)
    changed = (pc.spectrum(family, nb, ne) < pc.EPS).any(axis=1)
    eng, (pid,), _ = _engine([case])
    _eval(eng)
    H0 = _read(eng, [pid], [case])[0]
    assert eng.project(pc.EPS, False, None) == (ne, int(changed.sum()))                    # stand-alone
    Hs = _read(eng, [pid], [case])[0]
    _eval(eng)
    assert _same_bits(_read(eng, [pid], [case])[0], H0)
    assert eng.project(pc.EPS, False, _mask(eng.n_nodes, nb, range(pc.SHORT_LIST))) == (pc.SHORT_LIST, int(changed[:-1].sum()))   # batched
    Hb = _read(eng, [pid], [case])[0]
    eng.close()
    assert _same_bits(Hb[:-1], Hs[:-1]) and _same_bits(Hb[-1:], H0[-1:])
    assert ((_bits(Hs) != _bits(H0)).any(axis=(1, 2)) == changed).all()
    head = 4 * pc.epw(nb) + 1                                  # the first elements are those of the default case: against the exact projection
    _check_against_exact("NB=1 stand-alone", family, nb, 0, H0[:head], Hs[:head])


def _many_potentials():
    n_pot = pc.PROJ_BATCH + 5
    return [pc.make_case(pc.FAMILIES[k % len(pc.FAMILIES)], k % 6 + 1, ne=pc.epw(k % 6 + 1) + 1) for k in range(n_pot)]


def _rows_of(cases, first):
    return [np.arange(f, f + c.x.shape[0]) for c, f in zip(cases, first)]


def test_more_potentials_than_one_batch_holds():
    """PROJ_BATCH + 5 potentials of EPW + 1 elements, NB = 1..6 mixed: the batch is flushed once in the middle of the round and first_wave starts
    again at 0. Every element is within the bound and has the bits it gets in an engine that holds its potential alone."""
    cases = _many_potentials()
    assert len(cases) > pc.PROJ_BATCH and len(cases) > 2 * pc.MARK_BATCH and {c.nb for c in cases} == {1, 2, 3, 4, 5, 6}
    eng, pids, _ = _engine(cases)
    _eval(eng)
    H_in = _read(eng, pids, cases)
    n_proj, n_changed = eng.project(pc.EPS, False, None)
    H_out = _read(eng, pids, cases)
    eng.close()
    expect = 0
    for k, c in enumerate(cases):
        expect += _check_against_exact("potential %d NB=%d" % (k, c.nb), c.family, c.nb, 0, H_in[k], H_out[k], ne=c.n_elem)
        one, (pid,), _ = _engine([c])
        _eval(one)
        assert _same_bits(_read(one, [pid], [c])[0], H_in[k])
        one.project(pc.EPS, False, None)
        assert _same_bits(_read(one, [pid], [c])[0], H_out[k]), (k, c.name)
        one.close()
    assert n_proj == sum(c.n_elem for c in cases) and n_changed == expect


def test_ordered_matrix_update_behind_more_marks_than_one_batch_holds():
    """After assemble() the round patches the matrix: ordered (default) the result equals assemble() from the projected pools BIT FOR BIT — the
    marks of PROJ_BATCH + 5 potentials take three launches of MARK_BATCH —, atomic_projection = 1 within float rounding of it (64 float epsilons,
    as test_projection_updates_the_matrix_in_order, here of each potential's own largest entry: the potentials share no block)."""
    cases = _many_potentials()

    def run(atomic):
        eng, pids, first = _engine(cases, atomic_projection=atomic)
        _eval(eng)
        eng.assemble()
        v0 = eng.get_bsr()[2].copy()
        eng.project(pc.EPS, False, None)
        row_ptr, cols, v1 = eng.get_bsr()
        v1 = v1.copy()
        eng.assemble()
        v2 = eng.get_bsr()[2].copy()
        eng.close()
        return row_ptr, v0, v1, v2, first

    row_ptr, v0, v1, v2, first = run(0)
    assert (v1.view(np.int32) == v2.view(np.int32)).all()
    assert (v0 != v1).any()
    _, a0, a1, a2, _ = run(1)
    assert (a0.view(np.int32) == v0.view(np.int32)).all() and (a2.view(np.int32) == v2.view(np.int32)).all()
    for k, (c, rows) in enumerate(zip(cases, _rows_of(cases, first))):
        blk = np.arange(row_ptr[rows[0]], row_ptr[rows[-1] + 1])
        scale = max(np.abs(v2[blk]).max(), np.abs(v0[blk]).max())
        d = np.abs(a1[blk] - v1[blk]).max()
        print("potential %d %-18s NB=%d atomic - ordered %.3g of %.3g" % (k, c.family, c.nb, d, 64 * np.finfo(np.float32).eps * scale))
        assert d <= 64 * np.finfo(np.float32).eps * scale, (k, c.name)


# ---- e. translation-invariant kernels on synthesised states -----------------------------------------------------------------------------------
TI_NAMES = ("EnergyTetStrain", "EnergyTetStrain_Elasticity_Only", "EnergyTriangleStrain", "EnergyTriangleStrain_Elasticity_Only")
TI_MAX = 48          # elements per potential compared against mpmath.eigsy (0.05 s per 12 x 12)
_STATE, _TI_REF = {}, {}


def _synth_state(name):
    """(problem, manifest, u): DoFs = amplitude x a seeded pattern; the amplitude is the first of a geometric ladder at which, by the float64 oracle,
    at least a quarter of the elements of every translation-invariant potential have an eigenvalue below -1e-6 ||H|| and (tets) one is inverted."""
    if name in _STATE:
        return _STATE[name]
    from oracle import evaluator as ev

    prob, man, z = ev.load_fixture(os.path.join(GOLDEN, name + ".npz"))
    pattern = np.random.default_rng(2024).standard_normal(prob.ndofs)
    ti = [p for p in prob.potentials if p.name in TI_NAMES and p.conn.shape[0] > 0]
    assert ti
    for amp in 0.25 * 1.5 ** np.arange(24):
        prob.set_dofs(amp * pattern)
        ok = True
        for pot in ti:
            H = ev.evaluate_potential(prob, pot).H
            if not np.isfinite(H).all():
                ok = False
                break
            lo = np.linalg.eigvalsh(H).min(axis=1)
            ok = ok and (lo < -1e-6 * _fro(H)).sum() * 4 >= len(H)
            if "Tet" in pot.name:
                b = pot.bindings
                x1 = prob.arrays[b[4].array] + prob.dt * prob.arrays[b[0].array]
                X = prob.arrays[b[8].array]
                nodes = pot.conn[:, [b[k].conn for k in range(4)]]
                vol = lambda P: np.linalg.det(P[nodes[:, 1:]] - P[nodes[:, :1]])
                ok = ok and bool((vol(x1) * vol(X) < 0).any())
        if ok:
            print("%s: amplitude %.4g" % (name, amp))
            _STATE[name] = (prob, man, amp * pattern)
            return _STATE[name]
    raise AssertionError("%s: no amplitude of the ladder gives the state the test needs" % name)


@pytest.mark.parametrize("mirroring", [0, 1], ids=["clamp", "mirror"])
@pytest.mark.parametrize("variant", [2, 10], ids=["reduced", "full_size"])
@pytest.mark.parametrize("name", ["tetbeam_eo_4x1x1", "tetbeam_full_4x1x1", "cloth_shells_6"])
def test_translation_invariant_kernels_on_synthesised_states(name, variant, mirroring):
    """Built-in tets and membrane triangles, DoFs synthesised (a quarter of the elements indefinite, a tet inverted): the Helmert-reduced kernel
    (proj_variant 2) and the full-size one (10) against mpmath.eigsy on the unprojected read-back. Allowance: the bound of this module with the
    rounding term measured on this very read-back (8 x the float64 restatement's error against eigsy, floor 8 * 2^-52 * 3 NB), plus sqrt(3) eps for
    the three null directions, which the reduced kernel clamps as exact zeros, plus ||H_in (1 x I3)||_F, the read-back's own translational defect, plus
    the norm of its skew part (both measured from the read-back, never from the projected output)."""
    from gpu_util import engine_from_problem

    prob, man, u = _synth_state(name)
    eng = engine_from_problem(prob, man)
    eng.set_option("proj_variant", variant)
    eng.set_option("lazy_eval", 0)                             # the double pool: what is read back is what is projected
    eng.set_dofs(u)
    _eval(eng)
    counts = {pi: prob.potentials[pi].conn.shape[0] for pi in eng.pot_ids}
    H_in = {pi: eng.element_hessians(pid, counts[pi])[0].copy() for pi, pid in eng.pot_ids.items()}
    n_proj, n_changed = eng.project(pc.EPS, bool(mirroring), None)
    H_out = {pi: eng.element_hessians(pid, counts[pi])[0].copy() for pi, pid in eng.pot_ids.items()}
    assert eng.project(pc.EPS, bool(mirroring), None) == (0, 0)
    eng.close()
    assert n_proj == sum(counts.values())
    lo_count = hi_count = 0
    checked = 0
    for pi, H in H_in.items():
        pname = prob.potentials[pi].name
        n = H.shape[1]
        if pname not in TI_NAMES:
            lo = np.linalg.eigvalsh(H).min(axis=1)
            unsure = np.abs(lo - pc.EPS) <= 1e3 * 4 * ULP * n * _fro(H)
            lo_count += int(((lo < pc.EPS) & ~unsure).sum())
            hi_count += int(((lo < pc.EPS) | unsure).sum())
            continue
        lo_count += len(H)                                      # three eigenvalues of size rounding: below eps whatever their sign
        hi_count += len(H)
        m = min(len(H), TI_MAX)
        # (the closed-form kernels write both triangles: the read-back is symmetric to rounding, not to the bit. The reference projects its symmetric
        # part; the skew part joins the read-back's defects below.)
        Hs = 0.5 * (H[:m] + np.transpose(H[:m], (0, 2, 1)))
        asym = _fro(H[:m] - Hs)
        key = (name, pi)
        if key not in _TI_REF or not _same_bits(_TI_REF[key][0], H[:m]):
            ref, changed = pc.project_readback(Hs, pc.EPS, None)
            Pr, _, sweeps, converged = pc.restatement(Hs, pc.EPS)
            assert converged.all() and changed.all()
            fro = _fro(H[:m])
            rounding = {mir: np.maximum(8 * _fro(Pr[mir] - ref[mir]), 8 * ULP * n * fro) for mir in (0, 1)}
            _TI_REF[key] = (H[:m].copy(), ref, rounding, int(sweeps.max()))
        _, ref, rounding, sweeps = _TI_REF[key]
        fro = _fro(H[:m])
        defect = _fro(H[:m] @ np.kron(np.ones((n // 3, 1)), np.eye(3)))
        b = pc.SQRT_OFF_TOL * fro + rounding[mirroring] + np.sqrt(3.0) * pc.EPS + defect + asym
        err = _fro(H_out[pi][:m] - ref[mirroring])
        k = int(np.argmax(err - b))
        print("%s %-36s v=%d %s |P - P_eigsy| %.3g of %.3g (||H|| %.3g, rounding %.3g, defect %.3g, skew part %.3g, restatement sweeps %d)" % (
            name, pname, variant, "mirror" if mirroring else "clamp", err[k], b[k], fro[k], rounding[mirroring][k], defect[k], asym[k], sweeps))
        assert (err <= b).all(), (pname, k, err[k], b[k])
        assert _same_bits(H_out[pi], np.transpose(H_out[pi], (0, 2, 1)))
        if not mirroring:
            lam = np.linalg.eigvalsh(H_out[pi][:m]).min(axis=1)
            assert (lam >= pc.EPS - b - 4 * ULP * n * _fro(H_out[pi][:m])).all()
        checked += m
    assert checked > 0
    assert lo_count <= n_changed <= hi_count, (lo_count, n_changed, hi_count)
