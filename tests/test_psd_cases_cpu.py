"""CPU: the synthesised spectra of tests/psd_cases.py and their exact projections are proved here, before any kernel is blamed
(tests/test_gpu_psd_synth.py).

 * every program, run through oracle.symx_ops in float64, has the Hessian H_exact to 8 * 2^-52 ||H||_F, symmetric to the bit; the SynthDiag
   programs give diag(d) (+ the two placed entries) BIT FOR BIT, eps, nextafter(eps, 0) and the negative denormal included;
 * Q is orthogonal in mpmath (exactly: Z Z^T = D^2 I in integers);
 * the exact projection Q diag(f(lambda)) Q^T equals mpmath.eigsy on H_exact (project_readback), and the changed flags agree;
 * the float64 restatement of the kernels' Jacobi converges inside 30 sweeps on every spectrum, decides changed / unchanged as the exact
   spectrum does, and its error is what tests/psd_tolerances.json records;
 * the conditions on the cases: decision margins (psd_cases.margins_hold), changed and unchanged elements alternating inside the first
   wavefront, the special values where the families promise them, the thresholds read from the sources.
"""
import json
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import custom_cases as cc  # noqa: E402
import psd_cases as pc  # noqa: E402

ULP = 2.0 ** -52


def _fro(M):
    return np.sqrt((M * M).sum(axis=(1, 2)))


def test_thresholds_are_read_from_the_sources():
    assert [pc.epw(nb) for nb in pc.NBS] == [16, 10, 6, 5, 4, 3, 2, 2]
    assert pc.SHORT_LIST > 0 and pc.PROJ_BATCH > 0 and pc.MARK_BATCH > 0 and 0 < pc.JACOBI_OFF_TOL < 1e-20
    assert pc.SQRT_OFF_TOL ** 2 == pytest.approx(pc.JACOBI_OFF_TOL, rel=1e-15)
    # idle tail lanes at NB = 2, 3, 4 (64 is no multiple of even(3 NB)), none at NB = 5
    assert [64 - pc.epw(nb) * ((3 * nb + 1) & ~1) for nb in (2, 3, 4, 5)] == [4, 4, 4, 0]


@pytest.mark.parametrize("nb", pc.NBS)
def test_q_is_orthogonal_and_dense(nb):
    n = 3 * nb
    Z, D = pc.q_exact(n)
    G = Z @ Z.T
    assert all(G[i, j] == (D * D if i == j else 0) for i in range(n) for j in range(n))
    assert all(Z[i, j] != 0 for i in range(n) for j in range(n))
    ops, cst = pc.spectral_program(nb)
    assert len(ops) <= 600 and 2 * n <= cc.MAX_IN and 2 * n + 2 <= cc.MAX_IN


@pytest.mark.parametrize("nb", pc.NBS)
@pytest.mark.parametrize("family", pc.FAMILIES)
def test_programs_have_the_exact_hessian(family, nb):
    case = pc.make_case(family, nb)
    ex = pc.exact(family, nb)
    assert case.n_elem == 4 * pc.epw(nb) + 1
    E, g, H, active = cc.oracle(case)
    assert active.all() and (H == np.transpose(H, (0, 2, 1))).all()
    err = _fro(H - ex.H)
    print(family, nb, "oracle %.3g ulp of ||H||" % (pc._rel(err, ex.fro).max() / ULP))
    assert (err <= 8 * ULP * ex.fro).all()
    if family in pc.DIAG:                                   # to the bit (signed zeros compare equal: the kernels do not tell them apart either)
        assert (H == ex.H).all()
        d, o = pc.diag_inputs(family, nb, case.n_elem)
        assert (np.einsum("eii->ei", H) == d).all() and (H[:, 0, 1] == o[:, 0]).all() and (H[:, 1, 2] == o[:, 1]).all()
    # the reversed registration holds the same elements
    rev = pc.make_case(family, nb, reverse=True)
    assert (rev.gathered()[::-1, 3 * nb:] == case.gathered()[:, 3 * nb:]).all()


# (SynthDiag is diagonal beyond the leading 3 x 3 block: NB <= 4 says all there is to say)
@pytest.mark.parametrize("family,nb", [(f, nb) for f in pc.FAMILIES for nb in pc.NBS if f in pc.SPECTRAL or nb <= 4])
def test_exact_projection_equals_mpmath_eigsy(family, nb):
    """eigsy sees H_exact rounded to float64, so the two differ by the perturbation of that rounding: 2^-53 ||H|| in the matrix, carried through the
    1-Lipschitz rule. Checked on a changed and an unchanged element (NB <= 4: two of each); eigsy on 24 x 24 costs 0.3 s."""
    ex = pc.exact(family, nb)
    ne = len(ex.H)
    sel = [0, 1] if nb >= 5 else [0, 1, 2, ne - 1]
    Pb, changed = pc.project_readback(ex.H[sel], pc.EPS, None)
    assert (changed == ex.changed[sel]).all()
    for mir in (0, 1):
        P = Pb[mir]
        err = _fro(P - ex.P[mir][sel])
        assert (err <= 2 * ULP * (ex.fro[sel] + _fro(ex.P[mir][sel]))).all(), (family, nb, mir, err, ex.fro[sel])   # 2^-53: H rounded, P rounded twice
    if family in ("at_eps", "below_eps", "zeros_denormal"):
        P, changed = pc.project_readback(ex.H[sel], pc.EPS, 0)
        assert (changed == ex.changed[sel]).all() and (P == ex.P[0][sel]).all()


@pytest.fixture(scope="module")
def table():
    with open(pc.TOLERANCES) as f:
        return json.load(f)


@pytest.mark.parametrize("family", pc.FAMILIES)
def test_restatement_converges_and_the_table_is_its_measurement(family, table):
    worst = 0
    for nb in pc.NBS:
        ex = pc.exact(family, nb)
        v, changed, sweeps, converged, P = pc.restatement_figures(family, nb)
        assert converged.all() and sweeps.max() < pc.MAX_SWEEPS, (family, nb, sweeps.max())
        assert (changed == ex.changed).all()
        assert (P[0][~changed] == ex.H[~changed]).all() and (P[1][~changed] == ex.H[~changed]).all()
        worst = max(worst, int(sweeps.max()))
        t = table[family][str(nb)]
        print(family, nb, "restatement error %.3g ||H|| (table %.3g), bound's rounding term %.3g" % (v, t, pc.rounding_tolerance(family, nb)))
        # the committed table is this measurement (a BLAS that sums a 24-term dot product in another order moves the last sweep's landing point:
        # a factor 2 either way, or both under the floor)
        floor = ULP * 3 * nb
        assert (v <= 2 * t and t <= 2 * v) or max(v, t) <= floor, (family, nb, v, t)
    print(family, "sweeps at most", worst)
    if family in ("at_eps", "below_eps", "zeros_denormal"):
        assert worst == 0                                     # diagonal to the bit: no sweep


def test_the_table_has_every_family_and_nb(table):
    assert set(table) == set(pc.FAMILIES)
    assert all(set(table[f]) == {str(nb) for nb in pc.NBS} for f in table)
    assert all(0 <= table[f][k] < 1e-11 for f in table for k in table[f])


@pytest.mark.parametrize("nb", pc.NBS)
@pytest.mark.parametrize("family", pc.FAMILIES)
def test_conditions_on_the_cases(family, nb):
    ex = pc.exact(family, nb)
    n = 3 * nb
    ne = len(ex.H)
    if family in pc.MARGIN_FAMILIES:
        ok, (lo, b) = pc.margins_hold(family, nb)
        assert ok.all(), (family, nb, lo[~ok], b[~ok])
    # changed and unchanged elements alternate inside the first wavefront (families that have both kinds)
    if family in ("positive", "at_eps"):
        assert not ex.changed.any()
    else:
        first = ex.changed[:pc.epw(nb)]
        assert first.any() and not first.all() and (first[::2]).all() and not first[1::2].any()
        assert ex.changed[-1] == (ne % 2 == 1)              # the lone element of the last wavefront is a changed one
    lam = ex.lam
    if family == "rank_one_negative":
        assert ((lam[::2] == 0).sum(axis=1) == n - 1).all() and (lam[::2].min(axis=1) < 0).all()
    if family == "zero":
        assert (ex.H[::2] == 0).all()
    if family == "repeated":
        assert all(np.unique(l, return_counts=True)[1].max() >= (2 if n == 3 else 3) for l in lam)
    if family == "range":
        assert lam.max() == 2.0 ** 39 and lam.min() == -2.0 ** 13 and np.abs(lam[::2]).min() == 2.0 ** -10
    if family == "near_eps":
        assert all((l == 3 * pc.EPS).any() for l in lam) and all((l == -pc.EPS).any() for l in lam[::2]) and lam.max() / pc.EPS > 1e8
    d, o = (None, None) if family in pc.SPECTRAL else pc.diag_inputs(family, nb, ne)
    if family == "s2_big":
        theta = (d[:, 1] - d[:, 0]) / (2.0 * o[:, 0])
        with np.errstate(over="ignore"):
            assert (np.abs(o[:, 0]) > 1e-300).all() and (theta * theta + 1.0 >= 1e300).all() and (o[:, 1] != 0).any()
    if family == "tiny_off":
        assert (np.abs(o[:, 0]) == 1e-305).all() and (o[:, 1] != 0).any() and (o[:, 1] == 0).any()
    if family == "at_eps":
        assert all((l == pc.EPS).any() for l in d) and (d >= pc.EPS).all()
    if family == "below_eps":
        assert pc.EPS_BELOW < pc.EPS and np.nextafter(pc.EPS_BELOW, 1.0) == pc.EPS
        assert all((l == pc.EPS_BELOW).any() for l in d[::2]) and all((l == pc.EPS).any() and (l >= pc.EPS).all() for l in d[1::2])
    if family == "zeros_denormal":
        for l in d[::2]:
            z = l[l == 0]
            assert len(z) == 2 and np.signbit(z).sum() == 1 and (l == pc.DENORMAL).sum() == 1 and pc.DENORMAL < 0


def test_pair_schedule_visits_every_pair_once_per_sweep():
    for n in (3, 6, 9, 12, 15, 18, 21, 24):
        m = (n + 1) & ~1
        seen = []
        for r in range(m - 1):
            pairs = pc.round_pairs(n, r)
            flat = [i for p in pairs for i in p]
            assert len(set(flat)) == len(flat)                # disjoint within a round
            seen += pairs
        assert sorted(seen) == [(p, q) for p in range(n) for q in range(p + 1, n)]


def test_clamp_and_mirror_are_1_lipschitz_away_from_the_jump():
    """the step the bound rests on: ||f(A) - f(B)||_F <= ||A - B||_F for symmetric A, B whose eigenvalues stay clear of eps"""
    rng = np.random.default_rng(7)
    worst = 0.0
    for _ in range(300):
        n = int(rng.choice([3, 6, 12]))
        A = rng.standard_normal((n, n))
        A = A + A.T
        w, V = np.linalg.eigh(A)
        w = np.where(np.abs(w - pc.EPS) < 0.05, w + 0.2, w)
        A = (V * w) @ V.T
        E = rng.standard_normal((n, n)) * 1e-4
        B = A + E + E.T
        for mir in (False, True):
            fa, fb = (_project_np(M, mir) for M in (A, B))
            worst = max(worst, np.linalg.norm(fa - fb) / np.linalg.norm(A - B))
    print("Lipschitz ratio %.10f" % worst)
    assert worst <= 1.0 + 1e-6


def _project_np(M, mirroring):
    w, V = np.linalg.eigh(M)
    w = np.where(w < pc.EPS, -w if mirroring else pc.EPS, w)
    return (V * w) @ V.T
