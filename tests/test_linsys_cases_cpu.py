"""CPU: the references of tests/linsys_cases.py are proved here, before any kernel is blamed (tests/test_gpu_linsys_synth.py).

 * each op program, run through oracle.symx_ops, equals its closed form bit for bit;
 * the exactness claim: the contributions of every block summed in three shuffled orders, in float32 and in float64, give identical bits, and
   the per-case bit bounds (24 bits per block entry, 53 per row sum / energy) hold;
 * every SPD case factors (Cholesky / LU with positive pivots), with kappa_2 <= 1e6 wherever a forward error is asserted;
 * every indefinite_* case has a negative eigenvalue and the oracle's PCG reports found_indefiniteness on the case's right-hand side;
 * the threshold arithmetic each case's name promises is read off the graph.
"""
import os
import sys

import numpy as np
import pytest
import scipy.sparse.linalg as spla

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import linsys_cases as lc  # noqa: E402

from oracle import evaluator as ev  # noqa: E402
from oracle import symx_ops  # noqa: E402

IDS = [c.name for c in lc.CASES]


@pytest.mark.parametrize("case", lc.EXACT, ids=[c.name for c in lc.EXACT])
def test_op_programs_equal_the_closed_forms_bit_for_bit(case):
    prob, progs = lc.oracle_problem(case)
    U = case.u.reshape(-1, 3)
    E_sum = 0.0
    for p, pot, (ops, cst, n_in) in zip(case.pots, prob.potentials, progs):
        assert n_in == sum(b.stride for b in pot.bindings)
        o = symx_ops.evaluate(prob, pot, ops, cst)
        rows = case.rows_of(p)
        if p.kind == "spring":
            E, g, H = lc.spring_closed_form(p.k, p.c, p.w, U[rows[:, 0]], U[rows[:, 1]])
        else:
            E, g, H = lc.anchor_closed_form(p.k, p.c, p.w, U[rows[:, 0]])
        assert (o.block_rows == rows).all()
        assert (o.E == E).all() and (o.g == g).all() and (o.H == H).all(), p.kind
        E_sum += float(o.E.sum())
    E_ref, g_ref = lc.energy_grad(case)
    A = lc.exact_matrix(case)
    assert E_sum == E_ref == 0.5 * float(case.u @ (A @ case.u))
    assert (g_ref == A @ case.u).all()


@pytest.mark.parametrize("case", lc.EXACT, ids=[c.name for c in lc.EXACT])
def test_sums_do_not_depend_on_order_or_precision(case):
    block_bits, row_bits, e_bits = lc.check_exact(case)
    R, C, B = lc.contributions(case)
    keys, inv = np.unique(R * case.nbr + C, return_inverse=True)
    ref = np.zeros((len(keys), 3, 3))
    np.add.at(ref, inv, B)
    assert (ref.astype(np.float32).astype(np.float64) == ref).all()      # representable in the engine's float storage
    rng = np.random.default_rng(5)
    for dtype in (np.float32, np.float64):
        for _ in range(3):
            perm = rng.permutation(len(inv))
            acc = np.zeros((len(keys), 3, 3), dtype=dtype)
            np.add.at(acc, inv[perm], B[perm].astype(dtype))              # sequential, in the shuffled order, in dtype
            assert (acc.astype(np.float64) == ref).all(), dtype
    # and the assembled matrix is those sums
    bsr = lc.to_bsr(case)
    A = lc.exact_matrix(case)
    assert abs(bsr.to_scipy() - A).max() == 0.0
    for v in (case.u, case.x):
        y = A @ v
        if case.n <= 300:
            assert (A.toarray().astype(np.longdouble) @ v.astype(np.longdouble) == y).all()
        assert (y * 4096 == np.round(y * 4096)).all()


@pytest.mark.parametrize("case", lc.SPD, ids=[c.name for c in lc.SPD])
def test_spd_cases_factor_and_are_well_conditioned(case):
    A = lc.exact_matrix(case)
    assert abs(A - A.T).max() <= (0.0 if case.family == "exact" else 1e-13 * abs(A).max())      # (random family: the two triangles are summed in two orders)
    if case.n <= 4000:
        np.linalg.cholesky(A.toarray())
    else:   # symmetric fill-reducing order, pivots taken from the diagonal: P A P^T = L U with the diagonal of U positive
        lu = spla.splu(A.tocsc(), permc_spec="MMD_AT_PLUS_A", diag_pivot_thresh=0.0, options=dict(SymmetricMode=True))
        assert (lu.perm_r == lu.perm_c).all() and (lu.U.diagonal() > 0).all()
    kappa = lc.kappa2(case)
    assert kappa <= 1e6, kappa                                            # every SPD case is used in a forward-error assertion
    x = lc.reference_solution(case)
    eta, _ = lc.backward_error(A, x, case.b)
    print("%s: n %d kappa_2 %.3g eta_ref %.2e (refined %.2e)" % (case.name, case.n, kappa, case.eta_ref, eta))
    assert case.eta_ref <= case.n * 2.0 ** -53 and eta <= case.eta_ref + 2.0 ** -60


@pytest.mark.parametrize("case", lc.INDEFINITE, ids=[c.name for c in lc.INDEFINITE])
def test_indefinite_cases_are_indefinite_and_the_oracle_pcg_says_so(case):
    assert case.name.startswith("indefinite_")
    lc.check_exact(case)
    A = lc.exact_matrix(case)
    lo = np.linalg.eigvalsh(A.toarray())[0] if case.n <= 600 else spla.eigsh(A, k=1, which="SA", return_eigenvectors=False)[0]
    assert lo < -1.0, lo
    _, info = ev.solve_pcg(lc.to_bsr(case), case.b, 1e-10)
    assert info.found_indefiniteness and not info.converged


def _len(case, r, c, dynamic=()):
    static, dyn = lc.slot_lengths(case, dynamic)
    return static.get(r * case.nbr + c, 0), dyn.get(r * case.nbr + c, 0)


def test_threshold_counts_are_what_the_names_promise():
    # multi_L: the off-diagonal block (0, 1) has exactly L contributions; the diagonal blocks of rows 0 and 1 L (+ 1 path spring) + anchor,
    # and in the static part one structural key more
    for L in lc.MULTI_L:
        c = lc.BY_NAME["multi_%d" % L]
        assert _len(c, 0, 1) == (L, 0) and _len(c, 1, 0) == (L, 0)
        assert _len(c, 0, 0) == (L + 2, 0) and _len(c, 1, 1) == (L + 3, 0)
        assert _len(c, 0, 1, ("spring",)) == (0, L) and _len(c, 0, 0, ("spring",)) == (2, L)
        assert _len(c, 0, 0, ("spring", "anchor")) == (1, L + 1)
        n = lc.expected_counters(c)
        assert n["asm_vlong_slots_0"] == (4 if L > lc.VERY_LONG_SLOT else (2 if L + 3 > lc.VERY_LONG_SLOT else 0)), (L, n)
        assert n["asm_long_slots_0"] + n["asm_vlong_slots_0"] == (4 if L > lc.LONG_SLOT else (2 if L + 2 > lc.LONG_SLOT else 0)), (L, n)
        assert n["asm_short_slots_0"] + n["asm_long_slots_0"] + n["asm_vlong_slots_0"] == len(lc.block_pattern(c)) == 3 * 5 - 2
    S, V = lc.LONG_SLOT, lc.VERY_LONG_SLOT          # (48 and 4096 in the engine as it stands)
    assert lc.MULTI_L == (1, lc.SPLIT_LEN, lc.SPLIT_LEN + 1, S, S + 1, V, V + 1, V + lc.VLONG_SPLIT + 1)
    cnt = lambda L, dyn=(): lc.expected_counters(lc.BY_NAME["multi_%d" % L], dyn)  # noqa: E731
    assert cnt(S)["asm_long_slots_0"] == 2 and cnt(S + 1)["asm_long_slots_0"] == 4
    assert cnt(V)["asm_vlong_slots_0"] == 2 and cnt(V + 1)["asm_vlong_slots_0"] == 4
    # with the springs dynamic the lists of part 1 carry no structural key: blocks (0, 1), (1, 0), (0, 0) are exactly L long, (1, 1) L + 1 (the
    # path's first spring): at the threshold only that one is long, one above all four; the same at the very long threshold
    for L, key, want in ((S, "asm_long_slots_1", 1), (S + 1, "asm_long_slots_1", 4), (V, "asm_vlong_slots_1", 1), (V, "asm_long_slots_1", 3), (V + 1, "asm_vlong_slots_1", 4)):
        assert cnt(L, ("spring",))[key] == want, (L, key)
    # the very long lists are split into VLONG_SPLIT ranges: one above the threshold the last ranges are short or empty, VLONG_SPLIT + 1 above it
    # every range is one longer with a tail
    for L in (V + 1, V + lc.VLONG_SPLIT + 1):
        chunk = -(-L // lc.VLONG_SPLIT)
        assert chunk * (lc.VLONG_SPLIT - 1) < L + chunk and L % lc.VLONG_SPLIT != 0
    # star_N: the hub row holds N + 1 blocks, its diagonal block N contributions (+ anchor + structural key), N + 1 gradient incidences
    for N in lc.STAR_N:
        c = lc.BY_NAME["star_%d" % N]
        keys = lc.block_pattern(c)
        assert (keys // c.nbr == 0).sum() == N + 1 and len(keys) == 3 * N + 1
        assert _len(c, 0, 0) == (N + 2, 0)
        assert sum(int((c.rows_of(p) == 0).sum()) for p in c.pots) == N + 1      # gradient incidences of the hub: N springs + its anchor
    assert any(N + 1 <= lc.GRAD_LONG_ROW for N in lc.STAR_N) and any(N + 1 > lc.GRAD_LONG_ROW for N in lc.STAR_N) and 256 in lc.STAR_N
    # path_n: nnzb = 3 n - 2 one below, on and one above a multiple of the 64-block tile and of the 256-block chunk
    got = []
    for n in lc.PATH_N:
        c = lc.BY_NAME["path_%d" % n]
        nnzb = len(lc.block_pattern(c))
        assert nnzb == 3 * n - 2
        got.append(nnzb)
    assert [g % 64 for g in got[:3]] == [63, 0, 1] and [g % 256 for g in got[3:]] == [255, 0, 1], got
    assert lc.BY_NAME["sets_1024_1025"].set_rows == [lc.HOT_SET_ROWS, lc.HOT_SET_ROWS + 1]
    # DirectLLT: 1024 block rows are the last dense size, 1025 the first band size; the chain's band is LLT_MIN_BLOCK wide: 5 panels, one row left
    assert lc.BY_NAME["dense_1024_chain"].n == lc.MAX_DIRECT_DOFS and lc.llt_paths(lc.BY_NAME["dense_1024_star"]) == ["dense"]
    assert lc.BY_NAME["band_1025_chain"].n == lc.MAX_DIRECT_DOFS + 3 and lc.llt_paths(lc.BY_NAME["band_1025_star"]) == ["band", "mf"]
    assert -(-1025 // lc.LLT_MIN_BLOCK) == 5 and 1025 - 4 * lc.LLT_MIN_BLOCK == 1
    c = lc.BY_NAME["two_components_plus_isolated"]
    import scipy.sparse.csgraph as csg
    ncomp, lab = csg.connected_components(lc.exact_matrix(c).tocsr()[::3, ::3])      # (K has a positive diagonal: entry (0, 0) of a block is never zero)
    assert ncomp == 7 and sorted(np.bincount(lab).tolist()) == [1] * 5 + [400, 700]
    pw2 = lc.BY_NAME["path_pow2_diag_100"]
    d = lc.exact_matrix(pw2).diagonal()
    assert pw2.diag_exact and (np.log2(d) % 1 == 0).all() and abs(lc.exact_matrix(pw2) - lc.exact_matrix(pw2).T).max() == 0
