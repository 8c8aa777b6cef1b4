"""GPU (-m gpu): assembly, SpMV, block-Jacobi, PCG (solve.hip) and DirectLLT (direct.hip) on the synthesised systems of tests/linsys_cases.py.

The inputs are chosen, not found in a mesh: every case straddles one constant of the solver layer (the contribution-list thresholds, the tile /
chunk / hot-set granules, the DirectLLT switches), and the engine's counters (asm_*_slots_P, llt_*) prove that the kernel a case names ran. In
the exact family every sum is exact in any order and precision (proved on the CPU by tests/test_linsys_cases_cpu.py), so the energy, the
gradient, the element Hessians, the assembled blocks and A x are compared with `==`: one dropped or doubled contribution out of thousands
fails. The random family (non-dyadic values on the same graphs) keeps the rounding paths honest with the project's tolerances
(tests/test_gpu_parity.py), the assembly tolerance with the contribution count of each block.

DirectLLT is held to the exact matrix in long double, not to the engine's own SpMV: normwise backward error eta <= n 2^-53 and forward error
<= kappa_2 n 2^-53 against a refined float64 solution (the textbook Cholesky bounds with the constant dropped), every path the size allows.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import linsys_cases as lc  # noqa: E402

from oracle import evaluator as ev  # noqa: E402

pytestmark = pytest.mark.gpu

EPS32 = float(np.finfo(np.float32).eps)
ALL = lc.CASES
IDS = [c.name for c in ALL]
PLACEMENTS = {"static": (), "springs_dynamic": ("spring",), "both_dynamic": ("spring", "anchor")}


def _engine(case, dynamic=(), options=None, pots=None):
    """The case registered through the C ABI: one DoF set per set, every potential as an interpreted op sequence."""
    from stark_amd.engine import Engine

    eng = Engine(0)
    off = case.set_off
    dof = []
    for s in range(len(case.set_rows)):
        eng.add_dof_set("set%d" % s, np.ascontiguousarray(case.u[3 * off[s]:3 * off[s + 1]].reshape(-1, 3)).copy())
        dof.append(eng.L.mistark_dof_array(eng.h, s, 3))
    eng.set_option("custom_rtc", 0)
    for k, v in (options or {}).items():
        eng.set_option(k, v)
    pids = []
    for i, p in enumerate(case.pots if pots is None else pots):
        ops, cst, n_in = lc.spring_program() if p.kind == "spring" else lc.anchor_program()
        ncol = len(p.sets)
        data = [eng.array(p.k.reshape(-1, 1).copy(), 1), eng.array(p.c.reshape(-1, 1).copy(), 1), eng.array(np.ascontiguousarray(p.w).copy(), 3)]
        bs = [(dof[s], 3, j) for j, s in enumerate(p.sets)] + [(data[0], 1, ncol), (data[1], 1, ncol), (data[2], 3, ncol)]
        pid = eng.potential_custom("Synth%s_%d" % (p.kind.capitalize(), i), p.engine_conn(), bs, ops, cst, n_in)
        if p.kind in dynamic:
            eng.set_dynamic(pid, True)
        pids.append(pid)
    if case.coords is not None and (options or {}).get("llt_no_coords", 1) == 0:
        xyz = np.ascontiguousarray(case.coords, dtype=np.float64)
        eng._keep.append(xyz)
        eng._ck(eng.L.mistark_dist_set_row_coords(eng.h, xyz.ctypes.data, case.nbr))
    return eng, pids


def _assembled(case, dynamic=(), options=None):
    from stark_amd import capi

    eng, pids = _engine(case, dynamic, options)
    eng.eval(capi.EVAL_P_G_H)
    eng.assemble()
    return eng, pids


def _check_counters(eng, case, dynamic=()):
    want = lc.expected_counters(case, dynamic)
    got = {k: eng.counter(k) for k in want}
    assert got == want, (case.name, got, want)
    assert eng.counter("rtc_launches") == 0
    return got


def _check_matrix(eng, case, A=None, counts=None):
    """pattern == the graph's, values == the exact matrix (exact family) or within eps32 * contributions * max|A| per block (random family)."""
    A = lc.exact_matrix(case) if A is None else A
    row_ptr, cols, vals = eng.get_bsr()
    nbr = case.nbr
    keys = np.repeat(np.arange(nbr, dtype=np.int64), np.diff(row_ptr)) * nbr + cols
    want = lc.block_pattern(case)
    assert len(keys) == len(want) and (keys == want).all(), "pattern: %d blocks, the graph has %d" % (len(keys), len(want))
    ref = lc.to_bsr(case, A, dtype=np.float64).vals
    if case.family == "exact":
        bad = np.nonzero((vals.astype(np.float64) != ref).any(axis=(1, 2)))[0]
        assert len(bad) == 0, "blocks (row, col) %s differ: got %s want %s" % ([(int(k // nbr), int(k % nbr)) for k in keys[bad[:4]]], vals[bad[:1]], ref[bad[:1]])
    else:
        counts = lc.block_counts(case) if counts is None else counts
        n = np.array([counts.get(int(k), 0) for k in keys], dtype=np.float64)
        err = np.abs(vals.astype(np.float64) - ref).max(axis=(1, 2))
        tol = EPS32 * np.maximum(n, 1.0) * np.abs(ref).max()
        assert (err <= tol).all(), (err / tol).max()


# ----------------------------------------------------------------------------------------------------------------------
# evaluation
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ALL, ids=IDS)
def test_energy_gradient_and_element_hessians(case):
    from stark_amd import capi

    E_ref, g_ref = lc.energy_grad(case)
    U = case.u.reshape(-1, 3)
    for placement, no_grad_gather, no_dyn_pool in (("static", 0, 0), ("static", 1, 0), ("springs_dynamic", 0, 0), ("springs_dynamic", 0, 1), ("both_dynamic", 1, 1)):
        eng, pids = _engine(case, PLACEMENTS[placement], {"no_grad_gather": no_grad_gather, "no_dyn_pool": no_dyn_pool})
        E, g = eng.eval(capi.EVAL_P_G_H)
        Ep, _ = eng.eval(capi.EVAL_P)
        Eg, gg = eng.eval(capi.EVAL_P_G)
        tag = (case.name, placement, no_grad_gather, no_dyn_pool)
        if case.family == "exact":
            assert E == E_ref and Ep == E_ref and Eg == E_ref, tag
            assert (g == g_ref).all() and (gg == g_ref).all(), (tag, np.nonzero(g != g_ref)[0][:6])
        else:
            assert abs(E - E_ref) <= 1e-12 * abs(E_ref) and abs(Ep - E_ref) <= 1e-12 * abs(E_ref), tag
            _, g_abs = lc.energy_grad(case, absolute=True)
            assert (np.abs(g - g_ref) <= 1e-12 * g_abs).all() and (np.abs(gg - g_ref) <= 1e-12 * g_abs).all(), tag
        for p, pid in zip(case.pots, pids):
            H, rows = eng.element_hessians(pid, p.n)
            R = case.rows_of(p)
            H_ref = lc.spring_closed_form(p.k, p.c, p.w, U[R[:, 0]], U[R[:, 1]])[2] if p.kind == "spring" else lc.anchor_closed_form(p.k, p.c, p.w, U[R[:, 0]])[2]
            assert (rows == R).all()
            if case.family == "exact":
                assert (H == H_ref).all(), tag
            else:
                assert np.abs(H - H_ref).max() <= 1e-11 * np.abs(H_ref).max(), tag
        assert eng.counter("rtc_launches") == 0
        eng.close()


# ----------------------------------------------------------------------------------------------------------------------
# assembly
# ----------------------------------------------------------------------------------------------------------------------
ASSEMBLY_VARIANTS = [("default", {}), ("atomic_assembly", {"atomic_assembly": 1}), ("no_sym_gather", {"no_sym_gather": 1}), ("no_split_gather", {"no_split_gather": 1}),
                     ("no_row_order", {"no_row_order": 1}), ("chunk_tiles_1", {"spmv_chunk_tiles": 1}), ("chunk_tiles_8", {"spmv_chunk_tiles": 8}),
                     ("chunk_tiles_64", {"spmv_chunk_tiles": 64})]


@pytest.mark.parametrize("case", ALL, ids=IDS)
def test_assembly_pattern_and_values(case):
    A = lc.exact_matrix(case)
    counts = lc.block_counts(case)
    for name, options in ASSEMBLY_VARIANTS:
        eng, _ = _assembled(case, (), options)
        _check_counters(eng, case)
        _check_matrix(eng, case, A, counts)
        eng.close()
    for placement in ("springs_dynamic", "both_dynamic"):
        for options in ({}, {"atomic_assembly": 1}, {"no_split_gather": 1}):
            eng, _ = _assembled(case, PLACEMENTS[placement], options)
            _check_counters(eng, case, PLACEMENTS[placement])
            _check_matrix(eng, case, A, counts)
            eng.close()


def _sub(case, pot_index, keep):
    """the case with elements `keep` of one potential only (data and element indices unchanged): (case', engine connectivity)."""
    import copy

    c2 = copy.copy(case)
    p = case.pots[pot_index]
    c2.pots = list(case.pots)
    c2.pots[pot_index] = lc.Pot(p.kind, p.sets, p.conn[keep], p.k[keep], p.c[keep], p.w[keep])
    conn = np.concatenate([p.conn[keep], np.asarray(keep, dtype=np.int32)[:, None]], axis=1).astype(np.int32)
    return c2, conn


UPDATES = [("multi_%d" % (lc.LONG_SLOT + 1), 1), ("multi_%d" % (lc.VERY_LONG_SLOT + 1), 1), ("multi_%d" % (lc.VERY_LONG_SLOT + lc.VLONG_SPLIT + 1), lc.VLONG_SPLIT + 6),
           ("multi_%d" % (lc.SPLIT_LEN + 1), 1), ("star_257", 2), ("path_86", 1)]


@pytest.mark.parametrize("name,drop", UPDATES)
@pytest.mark.parametrize("placement", ["static", "springs_dynamic"])
def test_update_connectivity_shrinks_and_grows_across_the_thresholds(name, drop, placement):
    """LONG_SLOT + 1 <-> LONG_SLOT (49 <-> 48), VERY_LONG_SLOT + 1 <-> VERY_LONG_SLOT (4097 <-> 4096), ...: after update_connectivity the matrix is the one a fresh build of the new connectivity gives (here: the exact
    matrix of the new graph), pattern, values and kernel counters, shrinking and growing back."""
    from stark_amd import capi

    case = lc.BY_NAME[name]
    dyn = PLACEMENTS[placement]
    p = case.pots[0]
    assert p.kind == "spring"
    keep = np.arange(drop, p.n, dtype=np.int32)
    small, conn_small = _sub(case, 0, keep)
    eng, pids = _assembled(case, dyn)
    _check_counters(eng, case, dyn)
    _check_matrix(eng, case)
    for target, conn in ((small, conn_small), (case, p.engine_conn()), (small, conn_small)):
        eng.update_connectivity(pids[0], conn)
        eng.eval(capi.EVAL_P_G_H)
        eng.assemble()
        _check_counters(eng, target, dyn)
        _check_matrix(eng, target)
        E_ref, g_ref = lc.energy_grad(target)
        E, g = eng.eval(capi.EVAL_P_G)
        assert E == E_ref and (g == g_ref).all()
        y = eng.spmv(case.x)
        assert (y == lc.exact_matrix(target) @ case.x).all()
    if (name, drop) in UPDATES[:3]:     # these updates move blocks from one assembly kernel to another (the SPLIT_LEN one stays inside k_assemble_gather_split)
        assert lc.expected_counters(small, dyn) != lc.expected_counters(case, dyn)
    eng.close()


# ----------------------------------------------------------------------------------------------------------------------
# SpMV
# ----------------------------------------------------------------------------------------------------------------------
def _probe_vectors(case):
    """the case's dyadic vector and unit-ish vectors that isolate the hub column, the last row and the first row."""
    out = [("x", case.x)]
    for label, r in (("hub", max(case.hub, 0)), ("last", case.nbr - 1)):
        v = np.zeros(case.n)
        v[3 * r:3 * r + 3] = [1.0, -2.0, 0.5]
        out.append((label, v))
    return out


@pytest.mark.parametrize("case", ALL, ids=IDS)
def test_spmv(case):
    A = lc.exact_matrix(case)
    absA = abs(A)
    variants = [("static", {}), ("static", {"spmv_chunk_tiles": 1}), ("static", {"spmv_chunk_tiles": 8}), ("static", {"spmv_chunk_tiles": 64}), ("springs_dynamic", {}),
                ("both_dynamic", {})]
    for placement, options in variants:
        eng, _ = _assembled(case, PLACEMENTS[placement], options)
        for cap in (0, 1):
            for nt in (0, 1):
                eng.set_option("spmv_grid_cap", cap)
                eng.set_option("spmv_nt", nt)
                for label, v in _probe_vectors(case):
                    y = eng.spmv(v)
                    tag = (case.name, placement, options, cap, nt, label)
                    if case.family == "exact":
                        bad = np.nonzero(y != A @ v)[0]
                        assert len(bad) == 0, (tag, bad[:6] // 3)
                    else:   # float storage of A: one rounding per entry, products and sums in double
                        assert (np.abs(y - A @ v) <= 2.0 * EPS32 * (absA @ np.abs(v)) + 1e-300).all(), tag
        eng.close()


# ----------------------------------------------------------------------------------------------------------------------
# block-Jacobi preconditioner
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ALL, ids=IDS)
def test_block_jacobi(case):
    dinv = ev.block_diag_inverse(lc.to_bsr(case))
    z_ref = ev.apply_preconditioner(dinv, case.x)
    for placement in PLACEMENTS:
        eng, _ = _assembled(case, PLACEMENTS[placement])
        z = eng.apply_preconditioner(case.x)
        assert np.abs(z - z_ref).max() <= 1e-4 * np.abs(z_ref).max(), (case.name, placement)
        if case.diag_exact:   # diagonal blocks 2^k I: determinant, reciprocal and cofactors are exact in float
            d = lc.exact_matrix(case).diagonal()
            assert (z == case.x / d).all(), (case.name, placement)
        eng.close()


# ----------------------------------------------------------------------------------------------------------------------
# PCG
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ALL, ids=IDS)
def test_pcg(case):
    A = lc.exact_matrix(case)
    bsr = lc.to_bsr(case)
    abs_tol = 1e-8
    rhs = [case.b] if not case.spd else [case.b, case.x]
    refs = [ev.solve_pcg(bsr, b, abs_tol) for b in rhs]
    for options in ({}, {"cg_variant": 1}, {"pcg_batch": 1}, {"pcg_batch": 4}, {"pcg_batch": 8}):
        eng, _ = _assembled(case, (), options)
        for b, (x_ref, i_ref) in zip(rhs, refs):       # two solves back to back, different right-hand sides
            x, info = eng.pcg(abs_tol, rhs=b)
            tag = (case.name, options, info.n_iterations, i_ref.n_iterations)
            assert np.isfinite(x).all(), tag
            assert bool(info.found_indefiniteness) == i_ref.found_indefiniteness, tag
            assert bool(info.converged) == i_ref.converged, tag
            assert abs(info.n_iterations - i_ref.n_iterations) <= 1, tag
            if not case.spd:
                assert info.found_indefiniteness and not info.converged, tag
            elif info.converged and info.n_iterations == i_ref.n_iterations:
                res = np.linalg.norm(b - A @ x) / np.linalg.norm(b)
                res_ref = np.linalg.norm(b - A @ x_ref) / np.linalg.norm(b)
                assert res <= 3.0 * res_ref + 1e-6, (tag, res, res_ref)
        eng.close()


# ----------------------------------------------------------------------------------------------------------------------
# DirectLLT
# ----------------------------------------------------------------------------------------------------------------------
LLT_OPTIONS = {"dense": {}, "band": {"llt_multifrontal": -1}, "mf": {"llt_multifrontal": 1, "llt_no_coords": 1}, "mf_coords": {"llt_multifrontal": 1, "llt_no_coords": 0}}
LLT_PATH_ID = {"dense": 0, "band": 1, "mf": 2, "mf_coords": 2}


def _check_llt_counters(eng, case, path):
    got = {k: eng.counter(k) for k in ("llt_path", "llt_panel_rows", "llt_panels", "llt_fronts")}
    assert got["llt_path"] == LLT_PATH_ID[path], (case.name, path, got)
    if path == "dense":
        assert got["llt_panel_rows"] == case.nbr and got["llt_panels"] == 1 and got["llt_fronts"] == 0
    elif path == "band":
        mb = got["llt_panel_rows"]
        assert lc.LLT_MIN_BLOCK <= mb <= case.nbr and got["llt_panels"] == -(-case.nbr // mb) and got["llt_fronts"] == 0, got
        if case.name.endswith("band_1025_chain"):     # band 1 -> 256-row panels, the last one a single block row
            assert mb == lc.LLT_MIN_BLOCK and got["llt_panels"] == 5 and case.nbr - 4 * mb == 1, got
        if case.name.endswith("_star"):               # the hub couples every row: the band is (nearly) the whole matrix, two panels at the most
            assert 2 * mb >= case.nbr and got["llt_panels"] <= 2, got
        if case.name == "banded_300":                 # a block size that is a multiple of neither the 64-wide tile nor the 256-wide panel
            assert mb > lc.LLT_MIN_BLOCK and (3 * mb) % lc.LLT_TILE != 0 and (3 * mb) % lc.LLT_PANEL != 0, got
    else:
        assert got["llt_fronts"] == got["llt_panels"] >= 1 and 1 <= got["llt_panel_rows"] <= case.nbr, got
        if case.name.split("indefinite_")[-1] in ("band_1025_chain", "grid2d_40x40", "sets_1024_1025", "random_geometric_1500"):
            assert got["llt_fronts"] >= 3, got        # more than MF_LEAF rows in one component, many breadth-first levels: dissected at least once
        if case.name == "two_components_plus_isolated":
            assert got["llt_fronts"] >= 2 + 5, got    # the components and the five isolated rows are separate trees
        if case.name == "star_5000":
            assert got["llt_fronts"] >= 2, got        # the hub row leaves the graph first and forms the root
    return got


@pytest.mark.parametrize("case", ALL, ids=IDS)
def test_direct_llt(case):
    A = lc.exact_matrix(case)
    n = case.n
    bound = n * 2.0 ** -53
    sols = {}
    for path in lc.llt_paths(case):
        eng, _ = _assembled(case, (), LLT_OPTIONS[path])
        x, ok = eng.direct_llt(case.b)
        got = _check_llt_counters(eng, case, path)
        if not case.spd:
            assert ok is False, (case.name, path)
            eng.close()
            continue
        assert ok is True and np.isfinite(x).all(), (case.name, path)
        if case.family == "random":                    # the engine factors its float matrix: hold it to that matrix
            row_ptr, cols, vals = eng.get_bsr()
            A = ev.BSR(case.nbr, row_ptr, cols, vals).to_scipy().tocsr()
        eta, _ = lc.backward_error(A, x, case.b)
        if case.family == "exact":
            x_star = lc.reference_solution(case)
            fwd = np.abs(x - x_star).max() / np.abs(x_star).max()
            kappa = lc.kappa2(case)
            print("%s %s: eta %.2e (eta_ref %.2e, bound %.2e) forward %.2e (bound %.2e) %s" % (case.name, path, eta, case.eta_ref, bound, fwd, kappa * bound, got))
            assert fwd <= kappa * bound, (case.name, path, fwd, kappa * bound)
        else:
            print("%s %s: eta %.2e (bound %.2e) %s" % (case.name, path, eta, bound, got))
        assert eta <= bound, (case.name, path, eta, bound)
        # a second right-hand side on the same path (not at the dense limit: one workgroup factors 3072 unknowns in 3.4 s, once is enough)
        if case.n < lc.MAX_DIRECT_DOFS:
            x2, ok2 = eng.direct_llt(case.x)
            assert ok2 and lc.backward_error(A, x2, case.x)[0] <= bound
        sols[path] = x
        eng.close()
    if case.spd and case.family == "exact" and len(sols) > 1:
        kb = lc.kappa2(case) * bound
        ref = next(iter(sols.values()))
        for path, x in sols.items():
            assert np.abs(x - ref).max() <= kb * np.abs(ref).max(), (case.name, path)
