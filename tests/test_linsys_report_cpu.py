"""CPU: the shared arithmetic of the linear-system report (stark_amd/csrc/linsys_report.hpp compiled with g++, tests/host_linsys_report, test-only) against
numpy, and the numpy restatement of the whole report (tests/linsys_report_ref.py) against the exact spectra of tests/linsys_cases.py; the committed
tolerances. Every figure is printed before it is asserted."""
import ctypes
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import linsys_cases as lc  # noqa: E402
import linsys_report_ref as lr  # noqa: E402

SRC = os.path.join(ROOT, "tests", "host_linsys_report", "host_linsys_report.cpp")
EPS = lr.EPS


@pytest.fixture(scope="module")
def host_lib():
    out = os.path.join(tempfile.mkdtemp(prefix="mistark_host_linsys_"), "host_linsys_report.so")
    subprocess.run(["g++", "-std=c++17", "-O2", "-shared", "-fPIC", SRC, "-o", out], check=True)
    lib = ctypes.CDLL(out)
    p, i, d = ctypes.c_void_p, ctypes.c_int, ctypes.c_double
    lib.host_linsys_hash.argtypes = [p, i, p]
    lib.host_linsys_chol.argtypes = [p, i, p, p, p]
    lib.host_linsys_solves.argtypes = [p, p, i, p, p]
    lib.host_linsys_tridiag.argtypes = [i, p, p, p, p]
    lib.host_linsys_tridiag_last.argtypes = [i, p, p, p, p]
    lib.host_linsys_record.argtypes = [i, i, p, p, d, i, ctypes.c_longlong, p, ctypes.c_longlong, p, p]
    return lib


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


# ----------------------------------------------------------------------------------------------------------------------
# the start vector
# ----------------------------------------------------------------------------------------------------------------------
def test_hash_equals_numpy_bit_for_bit_and_the_pinned_values(host_lib):
    idx = np.concatenate([np.arange(0, 5000, dtype=np.uint64), np.array([2 ** 32 - 1, 2 ** 32, 2 ** 32 + 1, 2 ** 63, 2 ** 64 - 2, 2 ** 64 - 1], dtype=np.uint64)])
    out = np.zeros(len(idx))
    host_lib.host_linsys_hash(idx.ctypes.data, len(idx), out.ctypes.data)
    assert (_bits(out[:5000]) == _bits(lr.start_vector(5000))).all()
    assert (_bits(out) == _bits([lr.hash_value(int(i)) for i in idx])).all()
    assert ((out >= -1.0) & (out < 1.0)).all()
    pinned = {0: 0.7666216164272852, 1: -0.13694400590298006, 2: -0.9471324568148045, 2 ** 32: -0.45284307304587834}
    for i, v in pinned.items():
        got = np.zeros(1)
        one = np.array([i], dtype=np.uint64)
        host_lib.host_linsys_hash(one.ctypes.data, 1, got.ctypes.data)
        assert got[0] == v and lr.hash_value(i) == v, (i, got[0], v)


# ----------------------------------------------------------------------------------------------------------------------
# the tridiagonal solver
# ----------------------------------------------------------------------------------------------------------------------
def _tridiagonals():
    rng = np.random.default_rng(5)
    out = []
    for k in (1, 2, 3, 64, 256):
        out.append(("random_%d" % k, rng.uniform(-2, 2, k), rng.uniform(0.1, 1.0, k)))
    d, e = rng.uniform(-2, 2, 40), rng.uniform(0.1, 1.0, 40)
    e[19] = 0.0
    out.append(("zero_beta_in_the_middle", d, e))
    # two identical decoupled 2 x 2 blocks and a triple on the diagonal: repeated eigenvalues
    out.append(("repeated", np.array([1.0, 2.0, 1.0, 2.0, 3.0, 3.0, 3.0]), np.array([0.5, 0.0, 0.5, 0.0, 0.0, 0.0, 0.0])))
    k = 33
    out.append(("graded_1e-8_1e8", 10.0 ** np.linspace(-8, 8, k), 10.0 ** np.linspace(-8, 7.5, k) * 0.3))
    out.append(("laplacian_256", np.full(256, 2.0), np.full(256, -1.0)))
    return out


@pytest.mark.parametrize("name,d,e", _tridiagonals(), ids=[t[0] for t in _tridiagonals()])
def test_tridiagonal_solver_against_eigh(host_lib, name, d, e):
    k = len(d)
    d, e = np.ascontiguousarray(d), np.ascontiguousarray(e)
    T = np.diag(d) + np.diag(e[:k - 1], 1) + np.diag(e[:k - 1], -1)
    theta, S, last = np.zeros(k), np.zeros((k, k)), np.zeros(k)
    its = host_lib.host_linsys_tridiag(k, d.ctypes.data, e.ctypes.data, theta.ctypes.data, S.ctypes.data)
    assert its >= 0
    ref = np.linalg.eigvalsh(T)
    norm = np.linalg.norm(T, 2)
    bound = 8 * k * EPS * norm
    err = np.abs(theta - ref).max()
    res = np.linalg.norm(T @ S.T - S.T * theta[None, :], axis=0).max()
    unit = np.abs(np.linalg.norm(S, axis=1) - 1.0).max()
    print("%s: k %d iterations %d |theta - eigh| %.2e residual %.2e bound %.2e | |s| - 1 %.2e" % (name, k, its, err, res, bound, unit))
    assert (np.diff(theta) >= 0).all()
    assert err <= bound and res <= bound
    assert unit <= 8 * k * EPS
    # the last components alone: the same values and the same last components, to the bit (the same rotations)
    theta2 = np.zeros(k)
    assert host_lib.host_linsys_tridiag_last(k, d.ctypes.data, e.ctypes.data, theta2.ctypes.data, last.ctypes.data) >= 0
    assert (_bits(theta2) == _bits(theta)).all() and (_bits(last) == _bits(S[:, k - 1])).all()


# ----------------------------------------------------------------------------------------------------------------------
# Cholesky of the diagonal blocks and the two solves
# ----------------------------------------------------------------------------------------------------------------------
def _upper(D):
    return np.ascontiguousarray(np.stack([D[:, 0, 0], D[:, 0, 1], D[:, 0, 2], D[:, 1, 1], D[:, 1, 2], D[:, 2, 2]], axis=1))


def _host_chol(lib, D):
    a = _upper(D)
    n = len(a)
    L6, piv, ok = np.zeros((n, 6)), np.zeros(n), np.zeros(n, dtype=np.int32)
    lib.host_linsys_chol(a.ctypes.data, n, L6.ctypes.data, piv.ctypes.data, ok.ctypes.data)
    L = np.zeros((n, 3, 3))
    L[:, 0, 0], L[:, 1, 0], L[:, 1, 1], L[:, 2, 0], L[:, 2, 1], L[:, 2, 2] = L6.T
    return L6, L, piv, ok


def test_cholesky_and_solves_against_numpy(host_lib):
    blocks = []
    for name in ("path_43", "star_65", "random_values_star_257", "grid2d_40x40"):
        case = lc.BY_NAME[name]
        blocks.append(lr.diag_blocks(lr.case_matrix(case), case.nbr))
    D = np.concatenate(blocks)
    L6, L, piv, ok = _host_chol(host_lib, D)
    assert ok.all()
    ref = np.linalg.cholesky(D)
    scale = np.abs(D).max(axis=(1, 2))
    err = (np.abs(L - ref).max(axis=(1, 2)) / np.sqrt(scale)).max()
    back = (np.abs(L @ np.transpose(L, (0, 2, 1)) - D).max(axis=(1, 2)) / scale).max()
    print("cholesky: %d blocks, |L - numpy| / sqrt|D| %.2e, |L L^T - D| / |D| %.2e" % (len(D), err, back))
    kappa = np.linalg.cond(D).max()
    assert back <= 8 * EPS and err <= 8 * EPS * kappa
    assert (piv > 0).all() and np.abs(piv - np.minimum.reduce([ref[:, 0, 0] ** 2, ref[:, 1, 1] ** 2, ref[:, 2, 2] ** 2])).max() <= 8 * EPS * scale.max()
    # ... and the numpy restatement of the same formulas agrees to the bit
    L_ref, piv_ref, ok_ref = lr.chol_blocks(D)
    assert ok_ref.all() and (_bits(L_ref) == _bits(L)).all() and (_bits(piv_ref) == _bits(piv)).all()
    rng = np.random.default_rng(9)
    y = rng.uniform(-1, 1, (len(D), 3))
    w, x = np.zeros_like(y), np.zeros_like(y)
    host_lib.host_linsys_solves(L6.ctypes.data, y.ctypes.data, len(D), w.ctypes.data, x.ctypes.data)
    rw = np.abs(np.einsum("rij,rj->ri", L, w) - y).max()
    rx = np.abs(np.einsum("rji,rj->ri", L, x) - y).max()
    print("solves: |L w - y| %.2e |L^T x - y| %.2e" % (rw, rx))
    assert rw <= 16 * EPS * kappa and rx <= 16 * EPS * kappa


def test_cholesky_of_power_of_two_blocks_is_exact(host_lib):
    case = lc.BY_NAME["path_pow2_diag_100"]
    D = lr.diag_blocks(lr.case_matrix(case), case.nbr)
    d = D[:, 0, 0]
    assert (np.log2(d) % 1 == 0).all() and (D == d[:, None, None] * np.eye(3)).all()
    even = np.log2(d) % 2 == 0      # 4^k: the square root is exact as well
    assert even.any()
    L6, L, piv, ok = _host_chol(host_lib, D)
    assert ok.all() and (piv == d).all()
    assert (L[even] == np.sqrt(d[even])[:, None, None] * np.eye(3)).all()
    assert (L == np.sqrt(d)[:, None, None] * np.eye(3)).all()      # (sqrt is correctly rounded: the same double either way)


def test_negative_and_zero_pivots_are_reported_not_factored(host_lib):
    D = np.array([np.diag([-2.0, 1.0, 1.0]), np.diag([0.0, 1.0, 1.0]), [[1.0, 1.0, 0.0], [1.0, 1.0, 0.0], [0.0, 0.0, 1.0]], [[1.0, 0.0, 2.0], [0.0, 1.0, 0.0], [2.0, 0.0, 1.0]],
                  np.diag([1.0, np.nan, 1.0]), np.eye(3)])
    L6, L, piv, ok = _host_chol(host_lib, D)
    assert list(ok) == [0, 0, 0, 0, 0, 1]
    assert piv[0] == -2.0 and piv[1] == 0.0 and piv[2] == 0.0 and piv[3] == -3.0 and np.isnan(piv[4]) and piv[5] == 1.0
    _, piv_ref, ok_ref = lr.chol_blocks(D[[0, 1, 2, 3, 5]])
    assert list(ok_ref) == [False, False, False, False, True] and (piv_ref == piv[[0, 1, 2, 3, 5]]).all()
    # folded: two rows made negative, the first and the smallest are reported
    rec, ritz = np.zeros(16), np.zeros((4, 2))
    pivots = np.array([1.0, 0.5, -1.0, 2.0, -3.0, 0.25])
    a, b = np.array([1.0, 2.0]), np.array([0.5, 0.1])
    assert host_lib.host_linsys_record(2, 4, a.ctypes.data, b.ctypes.data, 3.0, 8, 18, pivots.ctypes.data, 6, rec.ctypes.data, ritz.ctypes.data) == 0
    assert rec[0] == 0 and rec[1] == 8 and (rec[2:11] == 0).all() and list(rec[11:16]) == [2.0, 2.0, -3.0, 4.0, 18.0] and (ritz == 0).all()


# ----------------------------------------------------------------------------------------------------------------------
# the record builder against the numpy restatement
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["tiny_2", "path_43", "indefinite_star_65"])
def test_record_builder_against_the_restatement(host_lib, name):
    case = lc.BY_NAME[name]
    A = lr.case_matrix(case)
    for m in (8, 64):
        r = lr.run(A, 0, m)
        k = len(r["alpha"])
        _, piv, _ = lr.chol_blocks(lr.diag_blocks(A, case.nbr))
        rec, ritz = np.zeros(16), np.full((m, 2), np.nan)
        a, b = np.ascontiguousarray(r["alpha"]), np.ascontiguousarray(r["beta"])
        flags_in = int(r["record"][1]) & 1
        assert host_lib.host_linsys_record(k, m, a.ctypes.data, b.ctypes.data, r["record"][7], flags_in, case.n, piv.ctypes.data, case.nbr, rec.ctypes.data, ritz.ctypes.data) == 0
        t_norm = r["record"][7]
        tol = 8 * k * EPS * t_norm
        print("%s m %d: k %d |record - numpy| %.2e (tol %.2e)" % (name, m, k, np.abs(rec - r["record"])[[2, 3, 4, 5, 7, 8]].max(), tol))
        assert (rec[[0, 1, 7, 8, 9, 11, 12, 13, 14, 15]] == r["record"][[0, 1, 7, 8, 9, 11, 12, 13, 14, 15]]).all()
        assert np.abs(rec[[2, 4]] - r["record"][[2, 4]]).max() <= tol and np.abs(rec[[3, 5]] - r["record"][[3, 5]]).max() <= tol
        if rec[2] > 0:
            assert abs(rec[6] - r["record"][6]) <= 4 * tol / rec[2] * rec[6]
        else:
            assert rec[6] == 0.0
        assert np.abs(ritz[:k] - r["ritz"]).max() <= tol and (ritz[k:] == 0).all()


# ----------------------------------------------------------------------------------------------------------------------
# the restatement against the exact spectra; the committed tolerances
# ----------------------------------------------------------------------------------------------------------------------
def test_tolerance_file_is_what_the_restatement_measures():
    doc = lr.load_tolerances()
    assert sorted(doc["c"]) == sorted(lr.GPU_CASES) and "_how" in doc
    for name, c in doc["c"].items():
        assert 0.0 < c <= lr.TOLERANCE_CAP, (name, c)
        assert c == max(4.0 * doc["measured"][name], 4.0), name


@pytest.mark.parametrize("name", lr.GPU_CASES)
def test_restatement_against_the_exact_spectrum(name):
    case = lc.BY_NAME[name]
    A = lr.case_matrix(case)
    c = lr.tolerance(name)
    for op in (0, 1):
        eigs, full = lr.reference_eigs(case, op)
        for m in lr.MS:
            r = lr.run(A, op, m)
            rec = r["record"]
            if eigs is None:
                assert not case.spd and int(rec[1]) == lr.FLAG_DIAG_NOT_PD and rec[0] == 0 and rec[11] >= 1 and rec[12] == lr.NEGATIVE_ROW[name]
                continue
            excess, n_held = lr.certificate_excess(r["ritz"], rec[7], eigs, full)
            tol = c * EPS * rec[7]
            print("%s op %d m %d: k %d flags %d excess %.2f eps T_norm over %d values (c = %.2f) theta %.6g .. %.6g, lambda %.6g .. %.6g" %
                  (name, op, m, rec[0], rec[1], excess, n_held, c, rec[2], rec[4], eigs[0], eigs[-1]))
            assert excess <= c
            assert eigs[0] - tol <= rec[2] and rec[4] <= eigs[-1] + tol          # Ritz values lie inside the spectrum's range
            if case.spd:
                assert rec[9] == 0 and rec[11] == 0 and rec[13] > 0 and not int(rec[1]) & lr.FLAG_INDEFINITE
                assert rec[6] <= eigs[-1] / eigs[0] * (1 + 4 * tol / eigs[0])
            elif op == 0 and m >= 64:
                assert int(rec[1]) & lr.FLAG_INDEFINITE and rec[9] >= 1


def test_header_as_a_stand_alone_program_under_sanitizers():
    exe = os.path.join(tempfile.mkdtemp(prefix="mistark_host_linsys_san_"), "host_linsys_san")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-DHOST_LINSYS_REPORT_MAIN", SRC, "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, (r.stdout, r.stderr)
    assert "0 mismatches" in r.stdout


def test_dry_context_refuses_every_entry_point():
    import ctypes as C

    from stark_amd import capi

    L = capi.lib()
    h = C.c_void_p()
    assert L.mistark_create_dry(C.byref(h)) == 0
    try:
        u = np.zeros(6)
        assert L.mistark_add_dof_set(h, b"u", u.ctypes.data, u.size) >= 0
        out = np.zeros(16)
        w = np.zeros(1, dtype=np.int32)
        for call in (lambda: L.mistark_linsys_report(h, 1, 8, None, out.ctypes.data, None, None, None),
                     lambda: L.mistark_linsys_modes(h, 1, 8, None, w.ctypes.data, 1, None, None, out.ctypes.data),
                     lambda: L.mistark_linsys_potential_shares(h, 1, 8, None, 0, None, 0, out.ctypes.data),
                     lambda: L.mistark_linsys_rhs(h, out.ctypes.data)):
            assert call() < 0
            msg = L.mistark_last_error(h).decode()
            assert msg and "registration-only" in msg, msg
    finally:
        L.mistark_destroy(h)


def test_header_declares_and_python_binds_the_new_entry_points():
    from stark_amd import capi
    from stark_amd import sim as S
    from stark_amd.engine import Engine, LinsysReport

    names = capi.exported_symbols()
    L = capi.lib()
    for s in ("mistark_linsys_report", "mistark_linsys_modes", "mistark_linsys_potential_shares", "mistark_linsys_rhs", "mistark_sim_record_linsys", "mistark_sim_get_linsys"):
        assert s in names and hasattr(L, s)
    for m in ("linsys_report", "linsys_modes", "linsys_potential_shares"):
        assert callable(getattr(Engine, m))
    for m in ("record_linsys", "linsys"):
        assert callable(getattr(S.Simulation, m))
    rep = LinsysReport(np.array([3, 1 + 2, -1.0, 0.5, 2.0, 0.0, 0.0, 4.0, 1e-12, 1, 2, 0, -1, 0.25, 7, 9.0]))
    assert rep.k == 3 and rep.exhausted and rep.indefinite and not rep.non_finite and not rep.diag_not_pd and rep.theta_min == -1.0 and rep.min_pivot_row == 7 and rep.n == 9
