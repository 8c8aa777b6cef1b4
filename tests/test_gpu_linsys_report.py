"""GPU (-m gpu): the linear-system report (mistark_linsys_report / _modes / _potential_shares, stark_amd/csrc/linsys_report.hip) on the synthesised systems of
tests/linsys_cases.py, whose assembled float matrix is known bit for bit, against reference spectra computed once per case (tests/linsys_report_ref.py:
dense eigh up to 800 unknowns, eigsh for the two ends beyond) and against the numpy restatement's definitions.

tol of a case is its entry c of tests/linsys_report_tolerances.json times eps T_norm: four times what the numpy restatement itself misses the reference by.
Every figure is printed before it is asserted. The mode tests run m = 256: there the extreme Ritz pairs have converged on every case, which the
comparison of |A x - theta D x| with twice the measured |B u - theta u| needs (the two differ by the factor ||L||, which exceeds 2 on the cases with long
rows; at m = 64 the numpy restatement itself misses that comparison on grid2d_40x40 and two_components_plus_isolated, by that factor)."""
import ctypes as C
import math
import os
import sys

import numpy as np
import pytest
import scipy.sparse as sp

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import linsys_cases as lc  # noqa: E402
import linsys_report_ref as lr  # noqa: E402

pytestmark = pytest.mark.gpu

EPS = lr.EPS
EPS32 = lr.EPS32
CASES = [lc.BY_NAME[n] for n in lr.GPU_CASES]
IDS = lr.GPU_CASES
SPD = [c for c in CASES if c.spd]
INDEF = [c for c in CASES if not c.spd]
EXACT_SPD = [c for c in SPD if c.family == "exact"]
PLACEMENTS = {"static": (), "springs_dynamic": ("spring",)}
M_MODES = 256


def _engine(case, dynamic=(), options=None, pots=None):
    """The case registered through the C ABI: one DoF set per set, every potential as an interpreted op sequence (as tests/test_gpu_linsys_synth.py)."""
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
    return eng, pids


def _assembled(case, dynamic=(), options=None):
    from stark_amd import capi

    eng, pids = _engine(case, dynamic, options)
    eng.eval(capi.EVAL_P_G_H)
    eng.assemble()
    return eng, pids


_ENGINES = {}


@pytest.fixture(scope="module", autouse=True)
def _close_engines():
    yield
    for eng, _ in _ENGINES.values():
        eng.close()
    _ENGINES.clear()


def shared(case):
    """one assembled engine per case for the read-only tests of this module"""
    if case.name not in _ENGINES:
        _ENGINES[case.name] = _assembled(case)
    return _ENGINES[case.name]


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _tol(case, t_norm):
    return lr.tolerance(case.name) * EPS * t_norm


def _D(case):
    A = lr.case_matrix(case)
    return A, lr.diag_blocks(A, case.nbr)


# ---- 1. certificate ---------------------------------------------------------------------------------------------------------------
def test_no_tolerance_exceeds_the_stop_threshold():
    doc = lr.load_tolerances()
    assert sorted(doc["c"]) == sorted(IDS)
    assert max(doc["c"].values()) <= 1e-10 / EPS


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_certificate_and_containment(case):
    eng, _ = shared(case)
    c = lr.tolerance(case.name)
    for op in (0, 1):
        eigs, full = lr.reference_eigs(case, op)
        if eigs is None:
            continue                                          # (operator 1 on a diagonal that is not PD: test_indefiniteness)
        for m in lr.MS:
            rep = eng.linsys_report(op, m)
            assert rep.k == len(rep.ritz) == len(rep.tri) and 1 <= rep.k <= min(m, case.n) and rep.n == case.n and not rep.non_finite
            tol = c * EPS * rep.t_norm
            excess, n_held = lr.certificate_excess(rep.ritz, rep.t_norm, eigs, full)
            print("%s op %d m %d: k %d flags %d, %d Ritz values held, excess %.2f eps T_norm (c = %.2f); theta %.9g .. %.9g lambda %.9g .. %.9g; kappa %.6g" %
                  (case.name, op, m, rep.k, rep.flags, n_held, excess, c, rep.theta_min, rep.theta_max, eigs[0], eigs[-1], rep.condition))
            assert excess <= c                                                           # 1. every (theta_i, rho_i) has a reference eigenvalue within rho_i + tol
            assert (np.diff(rep.ritz[:, 0]) >= 0).all() and (rep.ritz[:, 1] >= 0).all()
            assert rep.theta_min == rep.ritz[0, 0] and rep.theta_max == rep.ritz[-1, 0] and rep.rho_min == rep.ritz[0, 1] and rep.rho_max == rep.ritz[-1, 1]
            assert rep.beta_last == rep.tri[-1, 1] and rep.n_converged == (rep.ritz[:, 1] <= 1e-8 * rep.t_norm).sum() and rep.n_negative == (rep.ritz[:, 0] < 0).sum()
            t = np.abs(rep.tri[:, 0]) + rep.tri[:, 1] + np.concatenate([[0.0], rep.tri[:-1, 1]])
            assert rep.t_norm == t.max()
            assert eigs[0] - tol <= rep.theta_min and rep.theta_max <= eigs[-1] + tol   # 2. containment
            if case.spd:
                assert rep.condition == rep.theta_max / rep.theta_min
                assert rep.condition <= (eigs[-1] + tol) / (eigs[0] - tol)               # ... so slot 6 <= kappa_true (1 + small)
                assert rep.n_negative == 0 and rep.n_diag_not_pd == 0 and rep.first_diag_not_pd == -1 and rep.min_pivot > 0 and not rep.indefinite
    if case.name == "grid2d_40x40":
        eigs, _ = lr.reference_eigs(case, 1)
        rep = eng.linsys_report(1, 256)
        kappa = eigs[-1] / eigs[0]
        print("grid2d_40x40 op 1 m 256: kappa %.15g, true %.15g, relative %.2e" % (rep.condition, kappa, abs(rep.condition / kappa - 1)))
        assert abs(rep.condition / kappa - 1) <= 1e-6


@pytest.mark.parametrize("case", SPD, ids=[c.name for c in SPD])
def test_diagonal_slots(case):
    eng, _ = shared(case)
    A, D = _D(case)
    _, piv, ok = lr.chol_blocks(D)
    assert ok.all()
    for op in (0, 1):
        rep = eng.linsys_report(op, 8)
        assert rep.n_diag_not_pd == 0 and rep.first_diag_not_pd == -1
        assert rep.min_pivot == piv.min() and rep.min_pivot_row == int(np.argmin(piv))   # (the same formulas on the same float blocks: the same bits)


# ---- 3. exhaustion ----------------------------------------------------------------------------------------------------------------
def _clusters(eigs, tol):
    out = [[eigs[0]]]
    for e in eigs[1:]:
        if e - out[-1][-1] <= 2 * tol:
            out[-1].append(e)
        else:
            out.append([e])
    return out


@pytest.mark.parametrize("name", ["tiny_1", "tiny_2", "multi_1"])
def test_exhaustion_on_tiny_systems(name):
    case = lc.BY_NAME[name]
    eng, _ = shared(case)
    for op in (0, 1):
        eigs, full = lr.reference_eigs(case, op)
        rep = eng.linsys_report(op, 256)
        tol = _tol(case, rep.t_norm)
        cl = _clusters(eigs, tol)
        print("%s op %d: n %d k %d flags %d beta_last %.3e T_norm %.6g; %d distinct eigenvalues; theta %s" % (name, op, case.n, rep.k, rep.flags, rep.beta_last, rep.t_norm, len(cl), rep.ritz[:, 0]))
        assert full and rep.k <= case.n
        assert rep.exhausted                                 # flag +1
        hit = set()
        for theta, rho in rep.ritz:
            d = [min(abs(theta - e) for e in g) for g in cl]
            j = int(np.argmin(d))
            assert d[j] <= rho + tol
            hit.add(j)
        assert hit == set(range(len(cl))) and rep.k == len(cl)      # the distinct Ritz values are exactly the distinct eigenvalues


def test_star_stops_after_a_handful_of_steps():
    case = lc.BY_NAME["star_65"]
    eng, _ = shared(case)
    rep = eng.linsys_report(1, 256)
    print("star_65 op 1: k %d flags %d" % (rep.k, rep.flags))
    assert rep.exhausted and rep.k < 20


# ---- 4. indefiniteness ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", INDEF, ids=[c.name for c in INDEF])
def test_indefiniteness(case):
    eng, _ = shared(case)
    row = lr.NEGATIVE_ROW[case.name]
    eigs, full = lr.reference_eigs(case, 0)
    A, D = _D(case)
    _, piv, ok = lr.chol_blocks(D)
    for m in (64, 256):
        rep = eng.linsys_report(0, m)
        tol = _tol(case, rep.t_norm)
        print("%s op 0 m %d: k %d flags %d theta_min %.12g (rho %.2e) lambda_min %.12g, %d negative Ritz values" % (case.name, m, rep.k, rep.flags, rep.theta_min, rep.rho_min, eigs[0], rep.n_negative))
        assert rep.indefinite and rep.n_negative >= 1
        assert abs(rep.theta_min - eigs[0]) <= rep.rho_min + tol
        assert rep.condition == 0.0
        assert rep.n_diag_not_pd == (~ok).sum() >= 1 and rep.first_diag_not_pd == row and rep.min_pivot == piv.min() and rep.min_pivot_row == row   # slots 11..14 for both operators
    rep = eng.linsys_report(1, 64)
    assert rep.flags == 8 and rep.diag_not_pd and rep.n_diag_not_pd >= 1 and rep.first_diag_not_pd == row and rep.k == 0
    assert (rep.record[2:11] == 0).all() and rep.record[0] == 0 and len(rep.ritz) == 0 and rep.min_pivot == piv.min() < 0 and rep.min_pivot_row == row
    from stark_amd.engine import EngineError
    with pytest.raises(EngineError, match="no Ritz pairs"):
        eng.linsys_modes((0,), 1, 64)


# ---- 5. the first step ------------------------------------------------------------------------------------------------------------
def _unit(v):
    return v / math.sqrt(math.fsum(v * v))


def _alpha0(A, L, op, v0):
    """v0^T B v0 and the sum of the magnitudes of its terms"""
    x = lr.solve_Lt(L, v0) if op == 1 else v0
    return float(x @ (A @ x)), float(np.abs(x) @ (abs(A) @ np.abs(x)))


@pytest.mark.parametrize("case", EXACT_SPD + [c for c in INDEF], ids=[c.name for c in EXACT_SPD + INDEF])
def test_first_step_pins_the_dof_order(case):
    from stark_amd import capi

    eng, _ = shared(case)
    A = lc.exact_matrix(case).tocsr()
    L, _, ok = lr.chol_blocks(lr.diag_blocks(A, case.nbr))
    _, g = eng.eval(capi.EVAL_P_G)
    rng = np.random.default_rng(3)
    given = rng.uniform(-1, 1, case.n) * (1.0 + np.arange(case.n) % 7)      # not invariant under any permutation of the rows
    ops = (0, 1) if case.diag_exact else (0,)
    for op in ops:
        for label, start, v in (("built-in", None, lr.start_vector(case.n)), ("rhs", "rhs", -g), ("array", given, given)):
            rep = eng.linsys_report(op, 1, start=start)
            want, scale = _alpha0(A, L, op, _unit(v))
            print("%s op %d %s: alpha_0 %.17g numpy %.17g, difference %.2e, 8 eps sum|terms| %.2e" % (case.name, op, label, rep.tri[0, 0], want, abs(rep.tri[0, 0] - want), 8 * EPS * scale))
            assert abs(rep.tri[0, 0] - want) <= 8 * EPS * scale
            if case.n > 3:
                perm = np.roll(np.arange(case.n), 3)
                other, _ = _alpha0(A, L, op, _unit(v)[perm])
                assert abs(other - want) > 8 * EPS * scale      # (the check can tell the order: the neighbouring row order gives another number)


# ---- 6. modes ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_modes(case):
    eng, _ = shared(case)
    A, D = _D(case)
    Dsp = sp.block_diag(list(D)).tocsr()
    for op in (0, 1):
        if op == 1 and not case.spd:
            continue
        rep = eng.linsys_report(op, M_MODES)
        tol = _tol(case, rep.t_norm)
        md = eng.linsys_modes((0, -1), op, M_MODES)
        assert (md["index"] == [0, rep.k - 1]).all()
        assert (md["theta"] == [rep.theta_min, rep.theta_max]).all() and (md["rho"] == [rep.rho_min, rep.rho_max]).all()   # the same run, the same bits
        for i in range(2):
            x, nodal, theta, rho, res = md["x"][i], md["nodal"][i], md["theta"][i], md["rho"][i], md["residual"][i]
            norm = float(x @ (Dsp @ x)) if op == 1 else float(x @ x)
            gen = float(np.linalg.norm(A @ x - theta * (Dsp @ x if op == 1 else x)))
            u_rows = x.reshape(-1, 3)
            if op == 1:
                Lb, _, _ = lr.chol_blocks(D)
                u_rows = np.einsum("rji,rj->ri", Lb, x.reshape(-1, 3))        # u = L^T x
            share = (u_rows ** 2).sum(axis=1)
            print("%s op %d mode %d: theta %.12g rho %.2e measured residual %.2e; norm - 1 %.2e; |A x - theta D x| %.2e (limit %.2e); shares sum - 1 %.2e, |share - numpy| %.2e; top row %d (%.3f)" %
                  (case.name, op, i, theta, rho, res, norm - 1, gen, 2 * res + tol, nodal[:, 0].sum() - 1, np.abs(nodal[:, 0] - share).max(), int(np.argmax(nodal[:, 0])), nodal[:, 0].max()))
            assert abs(norm - 1) <= 1e-12
            assert gen <= 2 * res + tol
            assert res <= rho + tol
            assert abs(nodal[:, 0].sum() - 1) <= 1e-12 and np.abs(nodal[:, 0] - share).max() <= 1e-12
            assert np.abs(nodal[:, 1] - np.linalg.norm(x.reshape(-1, 3), axis=1)).max() <= 1e-14
            assert (nodal[:, 2] == np.einsum("rii->r", D)).all()
            assert (_bits(nodal[:, 3]) == _bits(lr.chol_blocks(D)[1])).all()
        if case.name == "star_65" and op == 0:
            assert int(np.argmax(md["nodal"][1][:, 0])) == case.hub            # the highest mode sits on the hub row
        if not case.spd:
            assert int(np.argmax(md["nodal"][0][:, 0])) == lr.NEGATIVE_ROW[case.name]   # the lowest mode sits on the negative row


# ---- 7. potential shares ------------------------------------------------------------------------------------------------------------
def _q_ref(case, x):
    """per potential q_e = x_e^T H_e x_e from the closed forms, evaluated in long double and rounded once (an extreme mode is smooth across a soft spring, the
    36 terms then cancel to a q_e far below them, and a reference evaluated in double would itself be off by more than 8 eps |q_e|), and the sum of the
    magnitudes of the terms, the scale of the long-double evaluation's own rounding"""
    X = x.reshape(-1, 3).astype(np.longdouble)
    out = []
    for p in case.pots:
        R = case.rows_of(p)
        if p.kind == "spring":
            H = lc.spring_closed_form(p.k, p.c, p.w, X[R[:, 0]], X[R[:, 1]])[2]
            xe = np.concatenate([X[R[:, 0]], X[R[:, 1]]], axis=1)
        else:
            H = lc.anchor_closed_form(p.k, p.c, p.w, X[R[:, 0]])[2]
            xe = X[R[:, 0]]
        H = H.astype(np.longdouble)
        out.append((np.einsum("ei,eij,ej->e", xe, H, xe).astype(np.float64), float(np.einsum("ei,eij,ej->", np.abs(xe), np.abs(H), np.abs(xe)))))
    return [q for q, _ in out], [t for _, t in out]


def _fsum(v):
    return math.fsum(float(t) for t in v)


# A potential's record is held to 8 eps sum|q_e| of THAT potential plus the reference's own rounding, REF_EPS times the sum of the magnitudes of the terms:
# the closed forms are evaluated in long double (64-bit significand, 2^-64 per operation; 36 terms and two products each leave 2^-60 with room). Without
# that term no reference of finite precision would do: on path_pow2_diag_100 the lowest mode of operator 1 is constant across every spring in exact
# arithmetic, the springs' exact sum is 0, and long double gives -2.8e-21 there where the device, adding its terms in double-double, gives 1.8e-28.
# The total over all potentials is held to theta within 8 eps sum|q_e| over all of them plus tol.
REF_EPS = 2.0 ** -60
SHARE_CASES = [c for c in CASES if c.family == "exact"] + [lc.BY_NAME["random_values_star_257"]]


@pytest.mark.parametrize("case", SHARE_CASES, ids=[c.name for c in SHARE_CASES])
def test_potential_shares(case):
    eng, pids = shared(case)
    for op in (0, 1):
        if op == 1 and not case.spd:
            continue
        rep = eng.linsys_report(op, M_MODES)
        tol = _tol(case, rep.t_norm)
        for which in (0, -1):
            md = eng.linsys_modes((which,), op, M_MODES, nodal=False)
            x, theta = md["x"][0], md["theta"][0]
            got = eng.linsys_potential_shares(pids, which, op, M_MODES)
            q, terms = _q_ref(case, x)
            qabs = sum(_fsum(np.abs(v)) for v in q)
            extra = EPS32 * qabs if case.family == "random" else 0.0
            for k, (p, v) in enumerate(zip(case.pots, q)):
                own = _fsum(np.abs(v))
                lim = 8 * EPS * own + REF_EPS * terms[k] + (EPS32 * own if case.family == "random" else 0.0)
                print("%s op %d which %d %s: sum q %.15g (numpy %.15g, difference %.2e, limit %.2e) sum|q| %.6g elements %d first largest %d" %
                      (case.name, op, which, p.kind, got[k, 0], _fsum(v), abs(got[k, 0] - _fsum(v)), lim, got[k, 1], got[k, 2], got[k, 3]))
                assert abs(got[k, 0] - _fsum(v)) <= lim and abs(got[k, 1] - _fsum(np.abs(v))) <= lim
                assert got[k, 2] == p.n
                if p.n:
                    e = int(got[k, 3])
                    assert 0 <= e < p.n and abs(v[e]) >= np.abs(v).max() - lim
                else:
                    assert got[k, 3] == -1
            print("%s op %d which %d: sum over all potentials %.15g theta %.15g, difference %.2e, limit %.2e" % (case.name, op, which, got[:, 0].sum(), theta, abs(got[:, 0].sum() - theta), 8 * EPS * qabs + tol + extra))
            assert abs(got[:, 0].sum() - theta) <= 8 * EPS * qabs + tol + extra


# ---- 8. nothing else moves, and the bits repeat -------------------------------------------------------------------------------------
@pytest.mark.parametrize("placement", list(PLACEMENTS))
@pytest.mark.parametrize("options", [{}, {"cg_variant": 1}], ids=["default", "cg_variant_1"])
@pytest.mark.parametrize("name", ["multi_%d" % (lc.LONG_SLOT + 1), "grid2d_40x40"])
def test_nothing_else_moves_and_the_bits_repeat(name, options, placement):
    from stark_amd import capi

    case = lc.BY_NAME[name]

    def state(eng, pids):
        """what the solver owns, read as it stands: nothing is evaluated or assembled again, so a report that wrote into the gradient, the element-Hessian
        pool, the matrix, the preconditioner or a PCG vector would show"""
        bsr = eng.get_bsr()
        g = np.zeros(eng.ndofs)
        eng._ck(eng.L.mistark_linsys_rhs(eng.h, g.ctypes.data))             # minus the gradient on the device, fetched
        H = [eng.element_hessians(pid, p.n)[0] for pid, p in zip(pids, case.pots)]
        z = eng.apply_preconditioner(case.x)
        x, info = eng.pcg(1e-8, rhs=case.b)
        x2, info2 = eng.pcg(1e-8)                                           # ... and the solve for the gradient on the device
        return [bsr[0], bsr[1], bsr[2], g] + H + [z, x, np.array([info.n_iterations, info.converged], dtype=np.float64), np.array([info.error]),
                                                  x2, np.array([info2.n_iterations, info2.converged], dtype=np.float64), np.array([info2.error])]

    def reports(eng, pids):
        out = []
        for op in (0, 1):
            rep = eng.linsys_report(op, 64)
            md = eng.linsys_modes((0, -1), op, 64)
            sh = eng.linsys_potential_shares(pids, -1, op, 64)
            out += [rep.record, rep.ritz, rep.tri, md["mode"], md["x"], md["nodal"], sh]
        return out

    eng, pids = _assembled(case, PLACEMENTS[placement], options)
    plain = state(eng, pids)
    eng.close()
    eng, pids = _assembled(case, PLACEMENTS[placement], options)
    n0 = eng.counter("linsys_reports")
    first = reports(eng, pids)
    second = reports(eng, pids)
    assert eng.counter("linsys_reports") == n0 + 12
    for a, b in zip(first, second):
        assert a.shape == b.shape and a.tobytes() == b.tobytes()          # two consecutive calls: identical bytes for every output
    after = state(eng, pids)
    assert (after[3] != 0).any() and all((h != 0).any() for h, p in zip(after[4:], case.pots) if p.n)   # (the snapshot holds the gradient and the Hessians)
    third = reports(eng, pids)                                            # ... and again after a solve has run in between
    for a, b in zip(first, third):
        assert a.tobytes() == b.tobytes()
    eng.close()
    for k, (a, b) in enumerate(zip(plain, after)):
        assert a.shape == b.shape and a.tobytes() == b.tobytes(), k       # matrix, gradient, element Hessians, PCG result: as without the report


# ---- 9. refusals --------------------------------------------------------------------------------------------------------------------
def test_refusals_and_null_outputs():
    import stark_amd
    from stark_amd import capi
    from stark_amd.engine import EngineError

    case = lc.BY_NAME["path_43"]
    eng, pids = _engine(case)
    for call in (lambda: eng.linsys_report(1, 64), lambda: eng.linsys_modes((0,), 1, 64), lambda: eng.linsys_potential_shares(pids, 0, 1, 64)):
        with pytest.raises(EngineError, match="matrix not assembled"):
            call()
    eng.eval(capi.EVAL_P_G_H)
    eng.assemble()
    n0 = eng.counter("linsys_reports")
    for m in (0, -1, 257):
        with pytest.raises(EngineError, match="out of range"):
            eng.linsys_report(1, m)
        with pytest.raises(EngineError, match="out of range"):
            eng.linsys_modes((0,), 0, m)
    for op in (-1, 2):
        with pytest.raises(EngineError, match="operator is 0"):
            eng.linsys_report(op, 8)
        with pytest.raises(EngineError, match="operator is 0"):
            eng.linsys_potential_shares(pids, 0, op, 8)
    with pytest.raises(EngineError, match="listed twice"):
        eng.linsys_potential_shares([pids[0], pids[0]], 0, 1, 8)
    with pytest.raises(EngineError, match="bad potential id"):
        eng.linsys_potential_shares([len(pids)], 0, 1, 8)
    with pytest.raises(EngineError, match="bad potential id"):
        eng.linsys_potential_shares([-1], 0, 1, 8)
    for start in (np.zeros(case.n), np.full(case.n, np.nan), np.concatenate([[np.inf], np.ones(case.n - 1)])):
        with pytest.raises(EngineError, match="zero or not finite"):
            eng.linsys_report(1, 8, start=start)
    assert eng.counter("linsys_reports") == n0                      # none of the refusals launched anything
    for which in (8, -9, 1000):
        with pytest.raises(EngineError, match="bad which"):
            eng.linsys_modes((which,), 1, 8)
        with pytest.raises(EngineError, match="bad which"):
            eng.linsys_potential_shares(pids, which, 1, 8)
    # every output NULL: nothing is launched, as the counter shows
    n0 = eng.counter("linsys_reports")
    L, h = eng.L, eng.h
    w = np.array([0], dtype=np.int32)
    ids = np.array(pids, dtype=np.int32)
    assert L.mistark_linsys_report(h, 1, 64, None, None, None, None, None) == 0
    assert L.mistark_linsys_modes(h, 1, 64, None, w.ctypes.data, 1, None, None, None) == 0
    assert L.mistark_linsys_potential_shares(h, 1, 64, None, 0, ids.ctypes.data, len(ids), None) == 0
    assert eng.counter("linsys_reports") == n0
    k = C.c_int32()
    assert L.mistark_linsys_report(h, 1, 64, None, None, None, None, C.byref(k)) == 0 and k.value == 64
    assert eng.counter("linsys_reports") == n0 + 1
    eng.close()
    # no element Hessians: the shares are refused, the report itself is not asked (no matrix either)
    eng, pids = _engine(case)
    eng.eval(capi.EVAL_P_G)
    with pytest.raises(EngineError, match="matrix not assembled"):
        eng.linsys_potential_shares(pids, 0, 1, 8)
    eng.close()
    # sharded and registration-only contexts
    L = capi.lib()
    group = L.mistark_local_group_create(2)
    try:
        eng = stark_amd.Engine(0)
        eng.dist_init_local(group, 0)
        eng.add_dof_set("u", np.zeros(6))
        for call in (lambda: eng.linsys_report(1, 8), lambda: eng.linsys_modes((0,), 1, 8), lambda: eng.linsys_potential_shares([], 0, 1, 8)):
            with pytest.raises(EngineError, match="single-rank"):
                call()
        eng.close()
    finally:
        L.mistark_local_group_destroy(group)
    h = C.c_void_p()
    assert L.mistark_create_dry(C.byref(h)) == 0
    try:
        out = np.zeros(16)
        assert L.mistark_linsys_report(h, 1, 8, None, out.ctypes.data, None, None, None) < 0
        assert "registration-only" in L.mistark_last_error(h).decode()
        assert L.mistark_linsys_modes(h, 1, 8, None, w.ctypes.data, 1, None, None, out.ctypes.data) < 0
        assert "registration-only" in L.mistark_last_error(h).decode()
        assert L.mistark_linsys_potential_shares(h, 1, 8, None, 0, None, 0, out.ctypes.data) < 0
        assert "registration-only" in L.mistark_last_error(h).decode()
    finally:
        L.mistark_destroy(h)


def test_lazy_float_blocks_are_refused_by_the_shares():
    from gpu_util import engine_from_problem
    from oracle import evaluator as ev
    from stark_amd.engine import EngineError

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    prob, man, z = ev.load_fixture(os.path.join(root, "tests", "golden", "tetbeam_eo_4x1x1_big.npz"))
    eng = engine_from_problem(prob, man)
    eng.set_option("lazy_eval", 1)
    n_pots = len(eng.describe_potentials())
    eng.eval()
    eng.assemble()
    rep = eng.linsys_report(1, 32)                                   # (the report itself reads the matrix only)
    assert rep.k >= 1 and rep.theta_min > 0
    msgs = []
    for p in range(n_pots):
        try:
            eng.linsys_potential_shares([p], 0, 1, 32)
        except EngineError as e:
            msgs.append(str(e))
    assert msgs and all("lazy path" in m for m in msgs), msgs
    eng.close()


# ---- 10. the scene mirror -------------------------------------------------------------------------------------------------------------
def _beam(record):
    from stark_amd import capi
    from stark_amd import sim as S
    from test_gpu_scene import _load

    z, traj, man = _load("traj_tetbeam_big_projected")
    sc = traj["scene"]
    args = dict(kv.split("=") for kv in bytes(z["harness_args"]).decode().split()[2:])
    st = S.default_settings()
    st.init_frictional_contact = 0
    sim = S.Simulation(st)
    p = S.soft_rubber()
    p.elasticity_only = sc["eo"]
    ps = sim.add_volume_grid("beam", (0, 0, 0), (sc["lx"], sc["ly"], sc["lz"]), (sc["nx"], sc["ny"], sc["nz"]), p)
    sim.prescribe_inside_aabb(ps, (-0.5 * sc["lx"], 0, 0), (2e-3, 2 * sc["ly"], 2 * sc["lz"]), 1e7)
    ns = S.default_settings().newton
    ns.projection_mode = capi.PROJ_PROJECTED_NEWTON
    sim.set_newton_settings(ns)
    v = sim.points("v0")
    i = np.arange(v.shape[0])[:, None]
    d = np.arange(3)[None, :]
    sim.set_points("v0", float(args["vamp"]) * np.sin(1.3 * (3.0 * i + d) + 0.7))
    if record:
        sim.record_linsys(True, 1, 64)
    return sim


def _log(sim):
    i = sim.info()
    out = [i.current_time, i.last_stats.newton_iterations, i.last_stats.n_linear_solves, i.last_stats.cg_iterations]
    for r in sim.newton_iteration_log():
        out.append((int(r.logged), int(r.n_projected_hessians), int(r.cg_iterations_last), int(r.line_search)))
    return out


def test_scene_recording():
    from stark_amd import sim as S

    def run(record):
        sim = _beam(record)
        with pytest.raises(S.SimError, match="no time step has been accepted" if record else "recording is off"):
            sim.linsys()
        logs, recs = [], []
        for _ in range(3):
            sim.run_one_step()
            logs.append(_log(sim))
            if record:
                recs.append(sim.linsys())
        return sim, logs, (sim.points("x0"), sim.points("v0")), recs

    sim, logs_off, end_off, _ = run(False)
    sim.close()
    sim, logs_on, end_on, recs = run(True)
    assert len(recs) == 3 and logs_on == logs_off                                 # the Newton / CG counts: as without recording
    assert (_bits(end_on[0]) == _bits(end_off[0])).all() and (_bits(end_on[1]) == _bits(end_off[1])).all()
    nbr = sim.info().n_points
    for s, r in enumerate(recs):
        rep = r["report"]
        print("step %d: time %.6g k %d flags %d kappa %.6g theta %.6g .. %.6g; lowest mode on row %d (%.3f), highest on row %d (%.3f)" %
              (s, r["time"], rep.k, rep.flags, rep.condition, rep.theta_min, rep.theta_max, r["low_row"], r["low_share"], r["high_row"], r["high_share"]))
        assert abs(r["time"] - logs_on[s][0]) < 1e-12 and r["op"] == 1 and r["m"] == 64
        assert np.isfinite(rep.condition) and rep.condition >= 1                   # slot 6
        assert rep.n_diag_not_pd == 0                                              # slot 11
        assert rep.k >= 1 and rep.n == 3 * nbr and 0 <= r["low_row"] < nbr and 0 <= r["high_row"] < nbr and 0 < r["low_share"] <= 1 and 0 < r["high_share"] <= 1
    sim.record_linsys(False)
    with pytest.raises(S.SimError, match="recording is off"):
        sim.linsys()
    with pytest.raises(S.SimError, match="out of range"):
        sim.record_linsys(True, 1, 0)
    with pytest.raises(S.SimError, match="operator"):
        sim.record_linsys(True, 2, 8)
    sim.close()
