"""GPU (-m gpu): the Hessian spectrum report (stark_amd/csrc/spectrum_report.hip) on element Hessians whose spectra are KNOWN (tests/psd_cases.py,
interpreter potentials, custom_rtc = 0) and on built-in potentials, against the bound of tests/spectrum_ref.py:
      b = ||H_in - H_exact||_F + SQRT_OFF_TOL ||H||_F + rounding ||H||_F      per element,
H_in the read-back element Hessian, rounding from tests/spectrum_tolerances.json (8 x the CPU restatement's error, measured on the CPU). Counts lie
between #(lam < eps - b) and #(lam < eps + b); |deficit - exact| <= sqrt(n) b. Every figure is printed before it is asserted.

 a. source 0 on every family x NB 1..8 at 4 EPW + 1 elements; ne = 1, EPW, EPW + 1 for NB 2 and 4; the DIAG identities to the bit
 b. decision consistency with mistark_project on the margin families (count, deficit, a second report after a mirroring projection)
 c. read-only and reproducible; an element's record does not depend on its neighbours
 d. built-in potentials: source 1 against source 0 (force_generic) and mpmath.eigsy; the refusals
 e. nodal and potential stages against numpy folds, with a hub row of more than 64 contributions
 f. non-finite entries
"""
import dataclasses
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import custom_cases as cc  # noqa: E402
import psd_cases as pc  # noqa: E402
import spectrum_ref as sp  # noqa: E402
from test_gpu_psd_synth import _engine, _eval, _read  # noqa: E402

pytestmark = pytest.mark.gpu

ULP = 2.0 ** -52
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and bool((_bits(a) == _bits(b)).all())


def _check_family(tag, family, nb, H_in, rep, ne=None):
    """a report of one synthesised potential against its exact spectrum; returns the bound"""
    ex = pc.exact(family, nb, ne)
    n = 3 * nb
    rec, spec = rep["records"], rep["spectrum"]
    assert rec.shape == (len(ex.H), 10) and spec.shape == (len(ex.H), n) and rep["nb"] == nb
    if family in pc.DIAG:
        assert (H_in == ex.H).all(), (tag, family)
    b = sp.bound(sp.rounding(family, nb), ex.fro, sp.fro(H_in - ex.H))
    sp.check_records("%s %-18s" % (tag, family), rec, spec, ex.lam, b)
    # fields 5 and 6 against the read-back, 4 ulp n
    fr = sp.fro(H_in)
    assert (np.abs(rec[:, 5] - fr) <= 4 * ULP * n * fr).all(), (tag, family)
    dg = np.einsum("eii->ei", H_in)
    assert (np.abs(rec[:, 6] - dg.sum(axis=1)) <= 4 * ULP * n * np.abs(dg).sum(axis=1)).all(), (tag, family)
    if family in pc.DIAG:                               # no rotation touches a diagonal matrix: the eigenvalues are the input diagonal to the bit
        d, o = pc.diag_inputs(family, nb, len(ex.H))
        plain = (o == 0).all(axis=1)
        assert (dg == d).all()
        assert _same_bits(spec[plain], sp.sort_by_rank(dg[plain])), (tag, family)   # (the stored diagonal: the interpreter's d_i * 1 + 0 turns -0.0 into +0.0)
        assert (rec[plain, 7] == 0).all() and (rec[plain, 8] == 0).all()
        if family == "at_eps":
            assert plain.all() and (rec[:, 2] == 0).all() and (rec[:, 9] == 0).all()
        elif family == "below_eps":
            assert plain.all() and (rec[:, 2] == (d == pc.EPS_BELOW).sum(axis=1)).all() and (rec[:, 9] == (rec[:, 2] > 0)).all()
        elif family == "zeros_denormal":
            assert plain.all()
            assert (rec[:, 2] == (d < pc.EPS).sum(axis=1)).all() and (rec[:, 3] == (_bits(d) == _bits(np.float64(pc.DENORMAL))).sum(axis=1)).all()
            assert (rec[::2, 2] == 3).all() and (rec[::2, 3] == 1).all()
    return b


# ---- a. spectra ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nb", pc.NBS)
def test_source0_on_every_family(nb):
    cases = [pc.make_case(f, nb) for f in pc.FAMILIES]
    eng, pids, _ = _engine(cases)
    _eval(eng)
    H_in = _read(eng, pids, cases)
    reps = [eng.spectrum_report(pid, 0, pc.EPS, spectrum=True) for pid in pids]
    again = eng.spectrum_report(pids[1], 0, pc.EPS, spectrum=True)
    only = eng.spectrum_report(pids[1], 0, pc.EPS)
    assert eng.counter("spectrum_reports") == len(pids) + 2
    eng.close()
    for f, hi, rep in zip(pc.FAMILIES, H_in, reps):
        assert len(hi) == 4 * pc.epw(nb) + 1
        _check_family("NB=%d" % nb, f, nb, hi, rep)
    assert _same_bits(again["records"], reps[1]["records"]) and _same_bits(again["spectrum"], reps[1]["spectrum"])
    assert _same_bits(only["records"], reps[1]["records"]) and only["spectrum"] is None


@pytest.mark.parametrize("which", ["one", "epw", "epw_plus_one"])
@pytest.mark.parametrize("nb", [2, 4])
def test_source0_at_the_wavefront_boundaries(nb, which):
    ne = {"one": 1, "epw": pc.epw(nb), "epw_plus_one": pc.epw(nb) + 1}[which]
    cases = [pc.make_case(f, nb, ne=ne) for f in pc.FAMILIES]
    eng, pids, _ = _engine(cases)
    _eval(eng)
    H_in = _read(eng, pids, cases)
    reps = [eng.spectrum_report(pid, 0, pc.EPS, spectrum=True) for pid in pids]
    eng.close()
    for f, hi, rep in zip(pc.FAMILIES, H_in, reps):
        _check_family("NB=%d ne=%d" % (nb, ne), f, nb, hi, rep, ne=ne)


# ---- b. the projection's decisions -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nb", pc.NBS)
def test_decisions_agree_with_the_projection(nb):
    """The rows flagged +1 are the elements mistark_project changes; the deficit is the Frobenius norm of what the clamping projection adds, within
    the projection's own bound (pc.bound) + sqrt(n) b. After a MIRRORING projection the spectrum is |lam|: lambda_min is min |lam| within b (b measured
    from the mirrored read-back against the exact mirrored matrix), and the count of eigenvalues below eps obeys the count bound of the module docstring
    on |lam| — no element flagged wherever every |lam| >= eps + b. (Exact zeros stay zeros under mirroring and -eps becomes eps to rounding: the
    elements of `zero`, `rank_one_negative` and `near_eps` are the ones whose count the bound leaves open or puts above zero.)"""
    n = 3 * nb
    fams = pc.MARGIN_FAMILIES
    cases = [pc.make_case(f, nb) for f in fams]
    eng, pids, _ = _engine(cases)
    _eval(eng)
    H_in = _read(eng, pids, cases)
    reps = [eng.spectrum_report(pid, 0, pc.EPS, spectrum=True) for pid in pids]
    _, n_changed = eng.project(pc.EPS, False, None)
    H_out = _read(eng, pids, cases)
    flagged = sum(int(r["projected"].sum()) for r in reps)
    print("NB=%d flagged %d, n_changed_now %d" % (nb, flagged, n_changed))
    assert flagged == n_changed
    for f, hi, ho, rep in zip(fams, H_in, H_out, reps):
        ex = pc.exact(f, nb)
        assert (rep["projected"] == ex.changed).all(), f
        h_err = sp.fro(hi - ex.H)
        tol = pc.bound(f, nb, ex.fro, h_err) + np.sqrt(n) * sp.bound(sp.rounding(f, nb), ex.fro, h_err)
        tol = tol + (n + 2) * ULP * rep["deficit"]                # (+ the rounding of the two norms themselves, as spectrum_ref.check_records)
        diff = np.abs(sp.fro(ho - hi) - rep["deficit"])
        k = int(np.argmax(diff - tol))
        print("NB=%d %-18s | ||H_out - H_in|| - deficit | %.3g of %.3g" % (nb, f, diff[k], tol[k]))
        assert (diff <= tol).all(), (f, k, diff[k], tol[k])
    _eval(eng)
    eng.project(pc.EPS, True, None)
    H_mir = _read(eng, pids, cases)
    reps2 = [eng.spectrum_report(pid, 0, pc.EPS, spectrum=True) for pid in pids]
    eng.close()
    for f, hm, rep in zip(fams, H_mir, reps2):
        ex = pc.exact(f, nb)
        b = sp.bound(sp.rounding(f, nb), ex.fro, sp.fro(hm - ex.P[1]))
        am = np.sort(np.abs(ex.lam), axis=1)
        err = np.abs(rep["lambda_min"] - am[:, 0])
        k = int(np.argmax(err - b))
        print("NB=%d %-18s mirrored: |lambda_min - min|lam|| %.3g of %.3g, flagged %d" % (nb, f, err[k], b[k], int(rep["projected"].sum())))
        assert (err <= b).all(), (f, k, err[k], b[k])
        lo, hi = (am < (pc.EPS - b)[:, None]).sum(axis=1), (am < (pc.EPS + b)[:, None]).sum(axis=1)
        assert ((rep["n_below_eps"] >= lo) & (rep["n_below_eps"] <= hi)).all(), f
        assert not rep["projected"][hi == 0].any(), f
        if f in ("positive", "mixed", "one_negative", "repeated", "s2_big", "tiny_off"):
            assert (hi == 0).all() and not rep["projected"].any(), f      # (every |lam| of these is far above eps: the report flags nothing)


# ---- c. read-only, reproducible, independent of neighbours -----------------------------------------------------------------------------------
def test_a_report_writes_nothing_the_engine_owns():
    nb = 3
    cases = [pc.make_case(f, nb) for f in ("mixed", "positive", "s2_big")]

    def run(report):
        eng, pids, _ = _engine(cases)
        _, g = eng.eval()
        if report:
            H0 = _read(eng, pids, cases)
            reps = [eng.spectrum_report(pid, 0, pc.EPS, spectrum=True) for pid in pids]
            nod = eng.nodal_spectrum(pids, 0, pc.EPS)
            pot = eng.spectrum_potential_report(pids, 0, pc.EPS)
            H1 = _read(eng, pids, cases)
            assert all(_same_bits(a, b) for a, b in zip(H0, H1))
        eng.assemble()
        vals0 = eng.get_bsr()[2].copy()
        if report:
            reps2 = [eng.spectrum_report(pid, 0, pc.EPS, spectrum=True) for pid in pids]
            assert all(_same_bits(a["records"], b["records"]) and _same_bits(a["spectrum"], b["spectrum"]) for a, b in zip(reps, reps2))
            assert _same_bits(nod, eng.nodal_spectrum(pids, 0, pc.EPS)) and _same_bits(pot, eng.spectrum_potential_report(pids, 0, pc.EPS))
            assert (eng.get_bsr()[2].view(np.int32) == vals0.view(np.int32)).all()
            assert all(_same_bits(a, b) for a, b in zip(H0, _read(eng, pids, cases)))
        # the gradient and the matrix as a solve sees them: the product and the preconditioned right-hand side
        y = eng.spmv(np.linspace(-1.0, 1.0, eng.ndofs))
        E2, g2 = eng.eval()
        eng.close()
        return g, vals0, y, E2, g2

    a, b = run(False), run(True)
    assert _same_bits(a[0], b[0]) and (a[1].view(np.int32) == b[1].view(np.int32)).all() and _same_bits(a[2], b[2])
    assert a[3] == b[3] and _same_bits(a[4], b[4])


@pytest.mark.parametrize("family", ["mixed", "repeated"])
@pytest.mark.parametrize("nb", [2, 3, 4, 5])
def test_a_record_does_not_depend_on_the_neighbours(nb, family):
    """forwards, reversed (every element in another lane group, beside other neighbours) and alone (a potential of one element): the same bits"""
    case = pc.make_case(family, nb)
    ne = case.n_elem
    eng, (pid,), _ = _engine([case])
    _eval(eng)
    fwd = eng.spectrum_report(pid, 0, pc.EPS, spectrum=True)
    eng.close()
    eng, (pid,), _ = _engine([pc.make_case(family, nb, reverse=True)])
    _eval(eng)
    rev = eng.spectrum_report(pid, 0, pc.EPS, spectrum=True)
    eng.close()
    assert _same_bits(rev["records"][::-1], fwd["records"]) and _same_bits(rev["spectrum"][::-1], fwd["spectrum"])
    singles = [cc.single(case, e) for e in range(ne)]
    eng, pids, _ = _engine(singles)
    _eval(eng)
    for e, p in enumerate(pids):
        one = eng.spectrum_report(p, 0, pc.EPS, spectrum=True)
        assert _same_bits(one["records"][0], fwd["records"][e]) and _same_bits(one["spectrum"][0], fwd["spectrum"][e]), e
    eng.close()
    assert len({int(s) for s in fwd["sweeps"]}) > 1 or family == "mixed"      # (elements converge at different sweeps: identity rotations are applied)


# ---- d. built-in potentials ------------------------------------------------------------------------------------------------------------------
MP_MAX = 16                                  # elements per potential checked through mpmath.eigsy (the first ones and the flagged ones)


def _builtin_engine(name, **options):
    from stark_amd import capi  # noqa: F401

    if name.startswith("contactmix"):
        from test_gpu_contact import build

        eng, prob, man, z, scene, st = build(name)
        dt = float(np.asarray(st["dt"]).ravel()[0])
        for k, v in options.items():
            eng.set_option(k, v)
        eng.contact_update_friction()
        eng.contact_update(dt)
    else:
        from gpu_util import engine_from_problem
        from oracle import evaluator as ev

        prob, man, z = ev.load_fixture(os.path.join(GOLDEN, name + ".npz"))
        eng = engine_from_problem(prob, man)
        for k, v in options.items():
            eng.set_option(k, v)
    return eng


@pytest.mark.parametrize("name", ["tetbeam_eo_4x1x1_big", "cloth_shells_6", "contactmix_t0"])
def test_builtin_potentials_source1(name):
    """force_generic = 1: eval() and source 1 run the same kernel, the records are the same bits. Without the option the evaluation takes its closed-form
    kernels and source 1 still gives those bits; they are within b of mpmath.eigsy of the generic Hessians (rounding: the largest entry of that NB in
    the JSON; H_in error 0: the read-back IS the matrix; mpmath on the first MP_MAX and the flagged elements, numpy.linalg.eigvalsh with its backward
    error 4 ulp n ||H|| on all of them)."""
    eng = _builtin_engine(name, force_generic=1, lazy_eval=0)
    n_pots = len(eng.describe_potentials())
    eng.eval()
    src0, src1, Hs = {}, {}, {}
    for p in range(n_pots):
        r0 = eng.spectrum_report(p, 0, pc.EPS, spectrum=True)
        if len(r0["records"]) == 0:
            continue
        src0[p], src1[p] = r0, eng.spectrum_report(p, 1, pc.EPS, spectrum=True)
        Hs[p] = eng.element_hessians(p, len(r0["records"]))[0].copy()
    ids = sorted(src0)
    pot0, pot1 = eng.spectrum_potential_report(ids, 0, pc.EPS), eng.spectrum_potential_report(ids, 1, pc.EPS)
    nod0, nod1 = eng.nodal_spectrum(ids, 0, pc.EPS), eng.nodal_spectrum(ids, 1, pc.EPS)
    eng.close()
    assert ids
    for p in ids:
        assert _same_bits(src0[p]["records"], src1[p]["records"]) and _same_bits(src0[p]["spectrum"], src1[p]["spectrum"]), p
    assert _same_bits(pot0, pot1) and _same_bits(nod0, nod1)
    flagged = int(pot0[:, 1].sum())
    print("%s: %d potentials with elements, %d elements, %d flagged, lambda_min %.6g" % (name, len(ids), int(pot0[:, 0].sum()), flagged, pot0[:, 5].min()))
    if name.startswith("tetbeam"):
        assert flagged >= 1                                   # the fixture was built for indefinite elements
    # the engine as it runs by default: closed-form evaluation, the report's source 1 beside it
    eng = _builtin_engine(name, lazy_eval=0)
    eng.eval()
    for p in ids:
        r = eng.spectrum_report(p, 1, pc.EPS, spectrum=True)
        assert _same_bits(r["records"], src1[p]["records"]) and _same_bits(r["spectrum"], src1[p]["spectrum"]), p
    eng.close()
    for p in ids:
        H, rep = Hs[p], src1[p]
        n = H.shape[1]
        assert _same_bits(H, np.transpose(H, (0, 2, 1)))     # the generic kernel writes both triangles from one value
        fr = sp.fro(H)
        b = sp.bound(sp.rounding_largest(n // 3), fr, 0.0)
        assert (rep["flags"] & 6 == 0).all(), p
        ev_np = np.linalg.eigvalsh(H)
        err = np.abs(rep["spectrum"] - ev_np).max(axis=1)
        assert (err <= b + 4 * ULP * n * fr).all(), (p, err.max())
        pick = sorted(set(range(min(len(H), MP_MAX))) | set(np.flatnonzero(rep["projected"])[:MP_MAX].tolist()))
        worst = 0.0
        for e in pick:
            E, _ = pc._eig_block(np.array([[pc.MP.mpf(float(v)) for v in row] for row in H[e]], dtype=object), pc.EPS)
            lam = np.sort(np.array([float(v) for v in E]))
            d = np.abs(rep["spectrum"][e] - lam).max()
            worst = max(worst, d / b[e] if b[e] > 0 else (0.0 if d == 0 else np.inf))
            assert d <= b[e], (p, e, d, b[e])
            lo, hi = (lam < pc.EPS - b[e]).sum(), (lam < pc.EPS + b[e]).sum()
            assert lo <= rep["n_below_eps"][e] <= hi, (p, e)
        print("%s potential %d (n = %d): %d elements, %d through mpmath, worst |lambda - eigsy| / b %.3g" % (name, p, n, len(H), len(pick), worst))


def test_refusals():
    from stark_amd.engine import EngineError

    eng = _builtin_engine("tetbeam_eo_4x1x1_big", lazy_eval=1)
    n_pots = len(eng.describe_potentials())
    with pytest.raises(EngineError, match="no element Hessians"):
        eng.spectrum_report(0, 0, pc.EPS)
    eng.eval()
    msgs = []
    for p in range(n_pots):
        try:
            eng.spectrum_report(p, 0, pc.EPS)
        except EngineError as e:
            msgs.append(str(e))
    assert msgs and all("lazy path" in m for m in msgs), msgs
    for p in range(n_pots):
        eng.spectrum_report(p, 1, pc.EPS)                     # (a fresh evaluation does not depend on how eval() stored its Hessians)
    with pytest.raises(EngineError, match="source"):
        eng.spectrum_report(0, 2, pc.EPS)
    with pytest.raises(EngineError, match="listed twice"):
        eng.nodal_spectrum([0, 0], 1, pc.EPS)
    with pytest.raises(EngineError, match="bad potential id"):
        eng.spectrum_potential_report([n_pots], 1, pc.EPS)
    eng.close()
    eng, (pid,), _ = _engine([pc.make_case("mixed", 2)])
    _eval(eng)
    with pytest.raises(EngineError, match="user-defined"):
        eng.spectrum_report(pid, 1, pc.EPS)
    with pytest.raises(EngineError, match="user-defined"):
        eng.nodal_spectrum([pid], 1, pc.EPS)
    assert len(eng.spectrum_report(pid, 0, pc.EPS)["records"]) == pc.n_elem_default(2)
    eng.close()


# ---- e. nodal and potential stages -----------------------------------------------------------------------------------------------------------
def _hub_case(ne=70):
    """SynthDiag NB = 2 on a star (linsys_cases._star): node 0 is touched by every element, more than SPEC_LONG_ROW = 64 contributions"""
    import linsys_cases as lc

    base = pc.make_case("s2_big", 2, ne=ne)
    star = lc._star(ne)
    conn = np.ascontiguousarray(np.concatenate([star, np.arange(ne)[:, None]], axis=1).astype(np.int32))
    rng = np.random.default_rng(5)
    return dataclasses.replace(base, name="psd_hub", x=rng.uniform(-0.8, 0.8, (ne + 1, 3)), conn=conn)


def test_nodal_and_potential_stages_against_numpy_folds():
    cases = [_hub_case(), pc.make_case("mixed", 3), pc.make_case("near_eps", 1), pc.make_case("positive", 4, ne=1)]
    eng, pids, _ = _engine(cases)
    _eval(eng)
    nbr = eng.ndofs // 3
    recs, rows = [], []
    for pid, c in zip(pids, cases):
        recs.append(eng.spectrum_report(pid, 0, pc.EPS)["records"])
        rows.append(eng.element_hessians(pid, c.n_elem)[1])
    order = [2, 0, 3, 1]                                       # (the list's order, not the ids', is the contribution order)
    sel = [pids[k] for k in order]
    nod = eng.nodal_spectrum(sel, 0, pc.EPS)
    long_rows = eng.counter("spectrum_report_long_rows")
    pot = eng.spectrum_potential_report(sel, 0, pc.EPS)
    chunks = eng.counter("spectrum_report_chunks")
    eng.close()
    ref, asum = sp.nodal_fold(nbr, [(pids[k], recs[k], rows[k]) for k in order])
    print("nodal: %d rows, %d long, largest count %d, flagged %d" % (nbr, long_rows, int(nod[:, 0].max()), int(nod[:, 1].sum())))
    assert long_rows == 1 and nod[:, 0].max() == 70 and chunks == len(sel)
    assert (nod[:, [0, 1, 2, 4]] == ref[:, [0, 1, 2, 4]]).all()
    assert (np.abs(nod[:, 3] - ref[:, 3]) <= 1e-12 * asum).all()
    for j, k in enumerate(order):
        r, d2 = sp.potential_fold(recs[k])
        assert (pot[j, [0, 1, 2, 3, 4, 5, 6, 7, 9]] == r[[0, 1, 2, 3, 4, 5, 6, 7, 9]]).all(), (k, pot[j], r)
        assert abs(pot[j, 8] ** 2 - d2) <= 1e-12 * d2 + 0.0 and abs(pot[j, 8] - r[8]) <= 1e-12 * r[8], (k, pot[j, 8], r[8])


def test_potential_stage_over_several_chunks():
    """5000 elements of one node: three chunks of 2048, the last one partial; the first of several elements attaining the minimum is named"""
    ne = 2 * 2048 + 904
    case = pc.make_case("one_negative", 1, ne=ne)
    eng, (pid,), _ = _engine([case])
    _eval(eng)
    rec = eng.spectrum_report(pid, 0, pc.EPS)["records"]
    pot = eng.spectrum_potential_report([pid], 0, pc.EPS)[0]
    assert eng.counter("spectrum_report_chunks") == 3
    eng.close()
    r, d2 = sp.potential_fold(rec)
    assert (rec[:, 0] == rec[:, 0].min()).sum() > 1 and r[6] == int(np.argmin(rec[:, 0]))
    assert (pot[[0, 1, 2, 3, 4, 5, 6, 7, 9]] == r[[0, 1, 2, 3, 4, 5, 6, 7, 9]]).all(), (pot, r)
    assert abs(pot[8] - r[8]) <= 1e-12 * r[8]


# ---- f. non-finite entries -------------------------------------------------------------------------------------------------------------------
def test_non_finite_elements_are_named_and_leave_the_rest_alone():
    nb = 3
    base = pc.make_case("s2_big", nb)
    d = base.arrays[0].copy()
    d[5, 2] = np.nan
    d[2, 0] = np.inf
    bad = dataclasses.replace(base, name="psd_nonfinite", arrays=[d, base.arrays[1]])
    eng, (p_ok, p_bad), _ = _engine([base, bad])
    _eval(eng)
    ok = eng.spectrum_report(p_ok, 0, pc.EPS, spectrum=True)
    rep = eng.spectrum_report(p_bad, 0, pc.EPS, spectrum=True)
    pot = eng.spectrum_potential_report([p_bad, p_ok], 0, pc.EPS)
    nod = eng.nodal_spectrum([p_bad], 0, pc.EPS)
    rows = eng.element_hessians(p_bad, bad.n_elem)[1]
    eng.close()
    hit = np.zeros(bad.n_elem, dtype=bool)
    hit[[2, 5]] = True
    assert (rep["flags"][hit] == 2).all() and (rep["records"][hit, :9] == 0).all() and (rep["spectrum"][hit] == 0).all()
    assert _same_bits(rep["records"][~hit], ok["records"][~hit]) and _same_bits(rep["spectrum"][~hit], ok["spectrum"][~hit])
    assert pot[0, 3] == 2 and pot[0, 9] == 2 and pot[1, 3] == 0 and pot[1, 9] == -1
    r, _ = sp.potential_fold(rep["records"])
    assert (pot[0, [0, 1, 2, 4, 5, 6, 7]] == r[[0, 1, 2, 4, 5, 6, 7]]).all()
    assert (nod[rows[2], 0] == 1).all() and (nod[rows[2], 4] == -1).all() and (nod[rows[2], 2] == 0).all()
