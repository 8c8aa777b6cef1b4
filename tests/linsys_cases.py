"""Synthesised SPD (and deliberately indefinite) linear systems for the solver layer (solve.hip, direct.hip), with references that are EXACT.

Pure numpy / scipy: nothing here touches the device. tests/test_linsys_cases_cpu.py proves the references, tests/test_gpu_linsys_synth.py
holds the engine to them.

Two user potentials, written as op sequences for the device interpreter (mistark_potential_custom with custom_rtc = 0):

  SynthSpring(a, b):  E = 1/2 k |u_a - u_b|^2 + 1/2 c (w . (u_a - u_b))^2      element Hessian [[K, -K], [-K, K]],  K = k I + c w w^T
  SynthAnchor(a):     E = 1/2 d |u_a|^2       + 1/2 c (w . u_a)^2              element Hessian K = d I + c w w^T

Both Hessians do not depend on the state. In the "exact" family every k, c, d, w_i, u_i, x_i, b_i is an integer / 8 of small magnitude, so every
block entry is an integer / 512 and every sum of them that fits in 24 bits (asserted per case: check_exact) has the same bits in ANY summation
order, in float or double, fused or not. The numpy matrix is then the matrix the engine must produce bit for bit, and A x, the gradient A u and
the energy 1/2 u^T A u likewise (53 bits, asserted). The "random" family keeps the graphs and draws non-dyadic values: the project's rounding
tolerances apply there (tests/test_gpu_parity.py), with the contribution count of each block.

Which kernel sums a BSR block is decided by the length of its contribution list (kernels_common.hpp, solve.hip); the thresholds are restated here
and the lists are counted from the graph (slot_lengths), so a case's name says what it straddles and expected_counters says what the engine's
counters must then read.
"""
from __future__ import annotations

import os
import re
from dataclasses import dataclass, field

import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla

# thresholds of the engine, read from its sources (no device, no library: the text of the constexpr lines), so that the cases straddle the constants
# the kernels were built with and a moved threshold moves the cases with it
_CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "stark_amd", "csrc")


def _constants(fname, *names):
    with open(os.path.join(_CSRC, fname)) as f:
        text = f.read()
    out = []
    for n in names:
        m = re.search(r"constexpr\s+\w+\s+%s\s*=\s*(\d+)\s*;" % n, text)
        assert m, "%s: no constexpr %s" % (fname, n)
        out.append(int(m.group(1)))
    return out


LONG_SLOT, VERY_LONG_SLOT, VLONG_SPLIT, GRAD_LONG_ROW, CHUNK_BLOCKS = _constants("kernels_common.hpp", "LONG_SLOT", "VERY_LONG_SLOT", "VLONG_SPLIT", "GRAD_LONG_ROW", "CHUNK_BLOCKS")
SPLIT_LEN, = _constants("solve.hip", "SPLIT_LEN")
HOT_SET_ROWS, = _constants("engine.hpp", "HOT_SET_ROWS")
MAX_DIRECT_DOFS, MF_LEAF = _constants("direct.hip", "MAX_DIRECT_DOFS", "MF_LEAF")
TILE_BLOCKS, LLT_MIN_BLOCK, LLT_TILE, LLT_PANEL = 64, 256, 64, 256   # tile of the BSR storage; DirectLLT: smallest band block, tile and panel widths
BAND_LIMIT_GB = 2.0   # the engine's own switch from the band to the multifrontal path

# symx::ExprType codes used by the two programs (oracle/symx_ops.py)
CONST, SYMBOL, ADD, SUB, MUL = 4, 5, 6, 7, 8


def _program(n_inputs, r, kk, cc, w):
    """1/2 (kk * |r|^2 + cc * (w . r)^2) over input / temporary indices; r and w are index triples."""
    ops, cst = [], []
    t = [n_inputs]

    def op(typ, a, b, c=0.0):
        ops.append((typ, t[0], a, b, -1))
        cst.append(c)
        t[0] += 1
        return t[0] - 1

    sq = [op(MUL, r[d], r[d]) for d in range(3)]
    rr = op(ADD, op(ADD, sq[0], sq[1]), sq[2])
    wr = [op(MUL, w[d], r[d]) for d in range(3)]
    s = op(ADD, op(ADD, wr[0], wr[1]), wr[2])
    ss = op(MUL, s, s)
    half = op(CONST, -1, -1, 0.5)
    e = op(MUL, half, op(ADD, op(MUL, kk, rr), op(MUL, cc, ss)))
    ops.append((SYMBOL, 0, e, -1, -1))
    cst.append(0.0)
    return np.array(ops, dtype=np.int32), np.array(cst), n_inputs


def spring_program():
    """inputs: u_a 0..2, u_b 3..5 (DoFs), k 6, c 7, w 8..10."""
    ops, cst = [], []
    n_in = 11
    for d in range(3):
        ops.append((SUB, n_in + d, d, 3 + d, -1))
        cst.append(0.0)
    o, c, _ = _program(n_in + 3, [n_in, n_in + 1, n_in + 2], 6, 7, [8, 9, 10])
    return np.concatenate([np.array(ops, dtype=np.int32), o]), np.concatenate([np.array(cst), c]), n_in


def anchor_program():
    """inputs: u 0..2 (DoF), d 3, c 4, w 5..7."""
    return _program(8, [0, 1, 2], 3, 4, [5, 6, 7])


def block_K(k, c, w):
    """K = k I + c w w^T per element: [n, 3, 3]."""
    return k[:, None, None] * np.eye(3)[None] + c[:, None, None] * w[:, :, None] * w[:, None, :]


def spring_closed_form(k, c, w, ua, ub):
    """(E [n], g [n, 6], H [n, 6, 6]) of SynthSpring."""
    K = block_K(k, c, w)
    r = ua - ub
    Kr = np.einsum("eij,ej->ei", K, r)
    H = np.zeros((len(k), 6, 6))
    H[:, :3, :3] = K
    H[:, 3:, 3:] = K
    H[:, :3, 3:] = -K
    H[:, 3:, :3] = -K
    return 0.5 * (r * Kr).sum(1), np.concatenate([Kr, -Kr], axis=1), H


def anchor_closed_form(d, c, w, u):
    K = block_K(d, c, w)
    Ku = np.einsum("eij,ej->ei", K, u)
    return 0.5 * (u * Ku).sum(1), Ku, K


@dataclass
class Pot:
    kind: str            # "spring" | "anchor"
    sets: tuple          # DoF set of each node column
    conn: np.ndarray     # int32 [n, 2 | 1]: row within its set
    k: np.ndarray        # k of a spring, d of an anchor
    c: np.ndarray
    w: np.ndarray        # [n, 3]

    @property
    def n(self):
        return len(self.k)

    def engine_conn(self):
        """node columns + the element's own index (the column its per-element data is bound through)."""
        return np.concatenate([self.conn, np.arange(self.n, dtype=np.int32)[:, None]], axis=1).astype(np.int32)


@dataclass
class Case:
    name: str
    set_rows: list
    pots: list
    family: str = "exact"       # "exact" | "random"
    spd: bool = True
    coords: np.ndarray | None = None
    diag_exact: bool = False    # c = 0 everywhere and every diagonal entry a power of two: the block-Jacobi inverse is exact as well
    u: np.ndarray = None
    x: np.ndarray = None
    b: np.ndarray = None
    hub: int = -1               # block row of the hub / of the long lists (-1: none)
    eta_ref: float = field(default=float("nan"))   # backward error of the float64 reference solve (reference_solution), filled when first computed

    @property
    def set_off(self):
        return np.concatenate([[0], np.cumsum(self.set_rows)]).astype(np.int64)

    @property
    def nbr(self):
        return int(sum(self.set_rows))

    @property
    def n(self):
        return 3 * self.nbr

    def rows_of(self, pot):
        """global block rows of every node column: [n, ncols]."""
        off = self.set_off
        return np.stack([off[s] + pot.conn[:, j] for j, s in enumerate(pot.sets)], axis=1).astype(np.int64)


# ----------------------------------------------------------------------------------------------------------------------
# references
# ----------------------------------------------------------------------------------------------------------------------
def contributions(case, kinds=("spring", "anchor")):
    """(block row, block col, 3x3 block) of every element-block contribution of the potentials of the given kinds, in registration order."""
    R, C, B = [], [], []
    for p in case.pots:
        if p.kind not in kinds or p.n == 0:
            continue
        rows = case.rows_of(p)
        K = block_K(p.k, p.c, p.w)
        if p.kind == "anchor":
            R.append(rows[:, 0]); C.append(rows[:, 0]); B.append(K)
        else:
            for a, b, sgn in ((0, 0, 1.0), (0, 1, -1.0), (1, 0, -1.0), (1, 1, 1.0)):
                R.append(rows[:, a]); C.append(rows[:, b]); B.append(sgn * K)
    if not R:
        return np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros((0, 3, 3))
    return np.concatenate(R), np.concatenate(C), np.concatenate(B)


def _scatter(case, R, C, B):
    n = case.n
    i = np.broadcast_to(3 * R[:, None, None] + np.arange(3)[None, :, None], B.shape)
    j = np.broadcast_to(3 * C[:, None, None] + np.arange(3)[None, None, :], B.shape)
    return sp.coo_matrix((B.reshape(-1), (i.reshape(-1), j.reshape(-1))), shape=(n, n)).tocsr()


def exact_matrix(case, kinds=("spring", "anchor")):
    """The global matrix in float64 (exact family: THE matrix, no rounding anywhere)."""
    return _scatter(case, *contributions(case, kinds))


def block_pattern(case):
    """Sorted (row, col) block keys of the matrix: every contribution and every diagonal block."""
    R, C, _ = contributions(case)
    nbr = case.nbr
    return np.unique(np.concatenate([R * nbr + C, np.arange(nbr, dtype=np.int64) * (nbr + 1)]))


def block_counts(case, kinds=("spring", "anchor")):
    """dict key -> number of element contributions into that block."""
    R, C, _ = contributions(case, kinds)
    k, n = np.unique(R * case.nbr + C, return_counts=True)
    return dict(zip(k.tolist(), n.tolist()))


def slot_lengths(case, dynamic=()):
    """Contribution-list lengths of the two matrix parts (0 static, 1 dynamic) as the pattern build counts them: part 0 holds every diagonal
    block with one structural (data-free) key each, part 1 only what its potentials touch."""
    nbr = case.nbr
    static = block_counts(case, tuple(k for k in ("spring", "anchor") if k not in dynamic))
    for r in range(nbr):
        static[r * (nbr + 1)] = static.get(r * (nbr + 1), 0) + 1
    dyn = block_counts(case, tuple(dynamic)) if dynamic else {}
    return static, dyn


def expected_counters(case, dynamic=()):
    out = {}
    for part, lens in enumerate(slot_lengths(case, dynamic)):
        v = np.array(list(lens.values()), dtype=np.int64)
        out["asm_vlong_slots_%d" % part] = int((v > VERY_LONG_SLOT).sum())
        out["asm_long_slots_%d" % part] = int(((v > LONG_SLOT) & (v <= VERY_LONG_SLOT)).sum())
        out["asm_short_slots_%d" % part] = int((v <= LONG_SLOT).sum())
    return out


def check_exact(case):
    """The bit bounds behind `==` (exact family): every value an integer / 8, every partial sum of a block entry within 24 bits at 2^-9, every
    SpMV row sum, gradient entry and the energy within 53 bits. Returns the largest bit counts met."""
    assert case.family == "exact"
    for p in case.pots:
        for a in (p.k, p.c, p.w):
            assert (a * 8 == np.round(a * 8)).all(), case.name
    for v in (case.u, case.x, case.b):
        assert (v * 8 == np.round(v * 8)).all(), case.name
    R, C, B = contributions(case)
    assert (B * 512 == np.round(B * 512)).all()
    absA = _scatter(case, R, C, np.abs(B))          # bounds every partial sum, whatever the order
    block_bits = np.log2(absA.max() * 512 + 1)
    assert block_bits < 24, (case.name, block_bits)
    row_bits = 0.0
    for v in (case.u, case.x):
        row_bits = max(row_bits, np.log2((absA @ np.abs(v)).max() * 4096 + 1))   # A at 2^-9, v at 2^-3
    e_bits = np.log2(np.abs(case.u) @ (absA @ np.abs(case.u)) * 32768 * 2 + 1)
    assert row_bits < 53 and e_bits < 53, (case.name, row_bits, e_bits)
    return block_bits, row_bits, e_bits


def energy_grad(case, absolute=False):
    """(E, grad) of the whole system at case.u from the closed forms (exact family: exact). absolute: the sums of the terms' magnitudes instead
    (the scale of a rounding tolerance)."""
    E, g = 0.0, np.zeros(case.n)
    off = case.set_off
    U = case.u.reshape(-1, 3)
    for p in case.pots:
        rows = case.rows_of(p)
        if p.kind == "spring":
            e, ge, _ = spring_closed_form(p.k, p.c, p.w, U[rows[:, 0]], U[rows[:, 1]])
        else:
            e, ge, _ = anchor_closed_form(p.k, p.c, p.w, U[rows[:, 0]])
        if absolute:
            e, ge = np.abs(e), np.abs(ge)
        E += float(e.sum())
        idx = (3 * rows[:, :, None] + np.arange(3)[None, None, :]).reshape(p.n, -1)
        np.add.at(g, idx.reshape(-1), ge.reshape(-1))
    return E, g


def to_bsr(case, A=None, dtype=np.float32):
    """oracle.evaluator.BSR of the matrix on the case's block pattern (structural diagonal blocks included)."""
    from oracle import evaluator as ev

    A = exact_matrix(case) if A is None else A
    nbr = case.nbr
    keys = block_pattern(case)
    rows, cols = keys // nbr, (keys % nbr).astype(np.int32)
    row_ptr = np.zeros(nbr + 1, dtype=np.int64)
    np.add.at(row_ptr, rows + 1, 1)
    A = A.tocsr()
    i = np.broadcast_to(3 * rows[:, None, None] + np.arange(3)[None, :, None], (len(rows), 3, 3))
    j = np.broadcast_to(3 * cols[:, None, None].astype(np.int64) + np.arange(3)[None, None, :], (len(rows), 3, 3))
    vals = np.asarray(A[i.reshape(-1), j.reshape(-1)]).reshape(-1, 3, 3)
    return ev.BSR(nbr, np.cumsum(row_ptr), cols, vals.astype(dtype))


def oracle_problem(case):
    """The case as oracle.evaluator.Problem + the op sequences per potential (for oracle.symx_ops.evaluate)."""
    from oracle import evaluator as ev

    off = case.set_off
    arrays, dof_arrays = [], {}
    for s, nr in enumerate(case.set_rows):
        dof_arrays[s] = len(arrays)
        arrays.append(case.u[3 * off[s]:3 * off[s + 1]].reshape(-1, 3).copy())
    pots, progs = [], []
    for p in case.pots:
        base = len(arrays)
        arrays += [p.k.reshape(-1, 1).copy(), p.c.reshape(-1, 1).copy(), p.w.copy()]
        ncol = len(p.sets)
        bs = [ev.Binding(dof_arrays[s], 3, j, s) for j, s in enumerate(p.sets)]
        bs += [ev.Binding(base, 1, ncol, -1), ev.Binding(base + 1, 1, ncol, -1), ev.Binding(base + 2, 3, ncol, -1)]
        pots.append(ev.PotentialDesc("SynthSpring" if p.kind == "spring" else "SynthAnchor", p.engine_conn(), bs))
        progs.append(spring_program() if p.kind == "spring" else anchor_program())
    prob = ev.Problem(dt=0.0, ndofs=case.n, dof_offsets=[int(3 * o) for o in off[:-1]], dof_sizes=[3 * r for r in case.set_rows], arrays=arrays, potentials=pots,
                      dof_arrays=dof_arrays)
    return prob, progs


def backward_error(A, x, b):
    """eta = |b - A x|_inf / (|A|_inf |x|_inf + |b|_inf), the residual in long double."""
    A = A.tocsr()
    xl, bl = x.astype(np.longdouble), b.astype(np.longdouble)
    r = bl.copy()
    np.subtract.at(r, np.repeat(np.arange(A.shape[0]), np.diff(A.indptr)), A.data.astype(np.longdouble) * xl[A.indices])
    return float(np.abs(r).max() / (abs(A).sum(axis=1).max() * np.abs(xl).max() + np.abs(bl).max())), r


_SOLUTIONS = {}


def reference_solution(case):
    """x* = A^-1 b: scipy splu in float64, refined with long-double residuals until the correction stalls. Also records case.eta_ref, the
    backward error of the unrefined float64 solve (what a good double solver achieves on this system). Computed once per case."""
    if case.name not in _SOLUTIONS:
        A = exact_matrix(case).tocsc()
        lu = spla.splu(A)
        x = lu.solve(case.b)
        case.eta_ref, r = backward_error(A, x, case.b)
        last = np.inf
        for _ in range(20):
            dx = lu.solve(np.asarray(r, dtype=np.float64))
            step = float(np.abs(dx).max())
            if not step < 0.5 * last:
                break
            x = x + dx
            last = step
            _, r = backward_error(A, x, case.b)
        _SOLUTIONS[case.name] = x
    return _SOLUTIONS[case.name]


_KAPPA = {}


def kappa2(case):
    """Spectral condition number of an SPD case: eigvalsh up to 4000 unknowns, eigsh (extreme pairs, shift-invert at 0 for the smallest) beyond."""
    if case.name not in _KAPPA:
        A = exact_matrix(case)
        if case.n <= 4000:
            w = np.linalg.eigvalsh(A.toarray())
            lo, hi = w[0], w[-1]
        else:
            hi = spla.eigsh(A, k=1, which="LA", return_eigenvectors=False, tol=1e-6)[0]
            lo = spla.eigsh(A.tocsc(), k=1, sigma=0.0, which="LM", return_eigenvectors=False, tol=1e-6)[0]
        _KAPPA[case.name] = float(hi / lo)
    return _KAPPA[case.name]


# ----------------------------------------------------------------------------------------------------------------------
# the cases
# ----------------------------------------------------------------------------------------------------------------------
def _eighths(rng, lo, hi, size):
    return rng.integers(lo, hi + 1, size=size).astype(np.float64) / 8.0


def _make(name, set_rows, pairs, seed, family="exact", coords=None, hub=-1, negative=(), diag_pow2=False):
    """pairs: int [m, 2] global block rows (a < b is arranged here); one anchor on every row. negative: rows whose anchor is made strongly
    negative (the diagonal block becomes negative definite: indefinite_*)."""
    rng = np.random.default_rng(seed)
    set_rows = list(set_rows)
    off = np.concatenate([[0], np.cumsum(set_rows)])
    nbr = int(off[-1])
    pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    pairs = np.sort(pairs, axis=1)
    assert (pairs[:, 0] != pairs[:, 1]).all() and pairs.min(initial=0) >= 0 and pairs.max(initial=0) < nbr
    m = len(pairs)
    if family == "exact":
        k, c, w = _eighths(rng, 1, 8, m), _eighths(rng, 0, 8, m), _eighths(rng, -8, 8, (m, 3))
        d, ca, wa = _eighths(rng, 4, 16, nbr), _eighths(rng, 0, 8, nbr), _eighths(rng, -8, 8, (nbr, 3))
    else:
        k, c, w = rng.uniform(0.1, 1.0, m), rng.uniform(0.0, 1.0, m), rng.uniform(-1.0, 1.0, (m, 3))
        d, ca, wa = rng.uniform(0.5, 2.0, nbr), rng.uniform(0.0, 1.0, nbr), rng.uniform(-1.0, 1.0, (nbr, 3))
    if diag_pow2:   # K = k I, and every diagonal entry (degree + d) a power of two
        k[:] = 1.0
        c[:] = 0.0
        ca[:] = 0.0
        deg = np.bincount(pairs.reshape(-1), minlength=nbr).astype(np.float64)
        d = 2.0 ** np.ceil(np.log2(deg + 1.0)) - deg
        d[d == 0] = 1.0
        assert (np.log2(deg + d) % 1 == 0).all()
    for r in negative:    # far below what its springs add (each K's eigenvalues are <= 1 + 3 = 4)
        deg = int((pairs == r).sum())
        d[r] = -(4.0 * deg + 8.0)
    sid = np.searchsorted(off, np.arange(nbr), side="right") - 1
    pots = []
    sa, sb = sid[pairs[:, 0]], sid[pairs[:, 1]]
    for s0 in range(len(set_rows)):
        for s1 in range(s0, len(set_rows)):
            sel = np.nonzero((sa == s0) & (sb == s1))[0]
            if len(sel):
                conn = np.stack([pairs[sel, 0] - off[s0], pairs[sel, 1] - off[s1]], axis=1).astype(np.int32)
                pots.append(Pot("spring", (s0, s1), conn, k[sel], c[sel], w[sel]))
    for s0, nr in enumerate(set_rows):
        sel = np.arange(off[s0], off[s0 + 1])
        pots.append(Pot("anchor", (s0,), (sel - off[s0]).astype(np.int32)[:, None], d[sel], ca[sel], wa[sel]))
    case = Case(name, set_rows, pots, family=family, spd=not negative, coords=coords, diag_exact=diag_pow2, hub=hub)
    if family == "exact":
        case.u, case.x, case.b = _eighths(rng, -16, 16, 3 * nbr), _eighths(rng, -32, 32, 3 * nbr), _eighths(rng, -32, 32, 3 * nbr)
    else:
        case.u, case.x, case.b = rng.uniform(-2, 2, 3 * nbr), rng.uniform(-4, 4, 3 * nbr), rng.uniform(-4, 4, 3 * nbr)
    if negative:   # a right-hand side on which the first PCG direction already has negative curvature: only the negative row is loaded
        case.b = np.zeros(3 * nbr)
        case.b[3 * negative[0]:3 * negative[0] + 3] = [1.0, -0.5, 0.25]
    return case


def _chain(n, first=0):
    return np.stack([np.arange(first, first + n - 1), np.arange(first + 1, first + n)], axis=1).reshape(-1, 2)


def _star(n_spokes):
    return np.stack([np.zeros(n_spokes, dtype=np.int64), np.arange(1, n_spokes + 1)], axis=1)


def _grid(nx, ny, first=0):
    idx = first + np.arange(nx * ny).reshape(nx, ny)
    e = [np.stack([idx[:-1, :].ravel(), idx[1:, :].ravel()], 1), np.stack([idx[:, :-1].ravel(), idx[:, 1:].ravel()], 1),
         np.stack([idx[:-1, :-1].ravel(), idx[1:, 1:].ravel()], 1)]   # + one diagonal: valence 6, like a triangle mesh
    return np.concatenate(e)


def _multi(L):
    # rows 0 and 1 joined by L parallel springs, then a path 1-2-3-4
    return np.concatenate([np.tile([[0, 1]], (L, 1)), _chain(4, 1)])


def path_rows_for(nnzb_mod, residue):
    """smallest n >= 4 whose chain has nnzb = 3 n - 2 = residue (mod nnzb_mod)."""
    n = 4
    while (3 * n - 2) % nnzb_mod != residue % nnzb_mod:
        n += 1
    return n


MULTI_L = (1, SPLIT_LEN, SPLIT_LEN + 1, LONG_SLOT, LONG_SLOT + 1, VERY_LONG_SLOT, VERY_LONG_SLOT + 1, VERY_LONG_SLOT + VLONG_SPLIT + 1)
STAR_N = (31, 32, 33, 63, 64, 65, 255, 256, 257, 5000)
PATH_N = tuple(path_rows_for(m, r) for m in (TILE_BLOCKS, CHUNK_BLOCKS) for r in (-1, 0, 1))


def _build_cases():
    cases = []
    seed = [1000]

    def add(*a, **kw):
        seed[0] += 1
        cases.append(_make(*a, seed=seed[0], **kw))

    add("tiny_1", [1], np.zeros((0, 2)))
    add("tiny_2", [2], [[0, 1]])
    for L in MULTI_L:
        add("multi_%d" % L, [5], _multi(L), hub=0)
    for N in STAR_N:
        add("star_%d" % N, [N + 1], _star(N), hub=0)
    for n in PATH_N:
        add("path_%d" % n, [n], _chain(n))
    add("path_pow2_diag_100", [100], _chain(100), diag_pow2=True)
    a, b = HOT_SET_ROWS, HOT_SET_ROWS + 1
    cross = np.stack([np.arange(0, a, 8), a + np.arange(0, a, 8)], axis=1)
    add("sets_1024_1025", [a, b], np.concatenate([_chain(a), _chain(b, a), cross]))
    gx = np.stack(np.meshgrid(np.arange(40.0), np.arange(40.0), indexing="ij"), -1).reshape(-1, 2)
    add("grid2d_40x40", [1600], _grid(40, 40), coords=np.concatenate([gx, np.zeros((1600, 1))], axis=1))
    from scipy.spatial import cKDTree
    pts = np.random.default_rng(77).uniform(0.0, 1.0, (1500, 2))
    add("random_geometric_1500", [1500], cKDTree(pts).query_pairs(np.sqrt(8.0 / (np.pi * 1500.0)), output_type="ndarray"),
        coords=np.concatenate([pts, np.zeros((1500, 1))], axis=1))
    rb = np.random.default_rng(78)
    i = rb.integers(0, 1200, 4000)
    j = np.clip(i + rb.integers(1, 301, 4000), 0, 1199)
    band = np.stack([i, j], 1)[i != j]
    add("banded_300", [1200], np.concatenate([band, _chain(1200), np.stack([np.arange(900), np.arange(900) + 300], 1)]))
    add("two_components_plus_isolated", [700 + 400 + 5], np.concatenate([_chain(700), _grid(20, 20, 700)]))
    add("dense_1024_chain", [1024], _chain(1024))
    add("dense_1024_star", [1024], _star(1023), hub=0)
    add("band_1025_chain", [1025], _chain(1025))
    add("band_1025_star", [1025], _star(1024), hub=0)
    # the same graphs with one anchor so negative that the exact matrix has a negative eigenvalue
    add("indefinite_tiny_2", [2], [[0, 1]], negative=(1,))
    add("indefinite_path_43", [43], _chain(43), negative=(20,))
    add("indefinite_star_65", [66], _star(65), negative=(0,), hub=0)
    add("indefinite_multi_%d" % (LONG_SLOT + 1), [5], _multi(LONG_SLOT + 1), negative=(1,), hub=0)
    add("indefinite_dense_1024_chain", [1024], _chain(1024), negative=(3,))
    add("indefinite_band_1025_chain", [1025], _chain(1025), negative=(1000,))
    add("indefinite_grid2d_40x40", [1600], _grid(40, 40), negative=(820,), coords=np.concatenate([gx, np.zeros((1600, 1))], axis=1))
    # non-dyadic values on graphs that reach every assembly kernel: rounding applies, the project's tolerances hold
    add("random_values_multi_%d" % (VERY_LONG_SLOT + 1), [5], _multi(VERY_LONG_SLOT + 1), family="random", hub=0)
    add("random_values_star_257", [258], _star(257), family="random", hub=0)
    add("random_values_grid2d_40x40", [1600], _grid(40, 40), family="random", coords=np.concatenate([gx, np.zeros((1600, 1))], axis=1))
    return cases


CASES = _build_cases()
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)
EXACT = [c for c in CASES if c.family == "exact"]
SPD = [c for c in CASES if c.spd]
INDEFINITE = [c for c in CASES if not c.spd]


def llt_paths(case):
    """DirectLLT paths the engine can run on the case: the dense one-workgroup Cholesky up to MAX_DIRECT_DOFS unknowns (the options do not
    matter there); beyond, the band (llt_multifrontal = -1) and the multifrontal path (= 1, breadth-first ordering; with row coordinates too
    where the case has them). The band of a star is the whole matrix as one dense panel: it is run where that panel stays under the engine's
    own band limit (BAND_LIMIT_GB)."""
    if case.n <= MAX_DIRECT_DOFS:
        return ["dense"]
    paths = []
    worst_rows = case.nbr if case.hub >= 0 else None    # a hub couples every row: bandwidth >= size / 2, one panel
    if worst_rows is None or 2.0 * (3.0 * worst_rows) ** 2 * 8.0 / 1e9 <= BAND_LIMIT_GB:
        paths.append("band")
    paths.append("mf")
    if case.coords is not None:
        paths.append("mf_coords")
    return paths
