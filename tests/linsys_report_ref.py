"""numpy restatement of the linear-system report (stark_amd/csrc/linsys_report.hpp / .hip) and its reference spectra, for tests/test_linsys_report_cpu.py
and tests/test_gpu_linsys_report.py. Pure numpy / scipy: nothing here touches the device.

The same start vector (splitmix64 of i + 1 in uint64), the same iteration (w = B v_j, alpha_j, the three-term update, classical Gram-Schmidt applied
twice, beta_j, T_norm), the same stop rule (beta_j <= 1e-10 T_norm, j + 1 == m, j + 1 == n) and the records built by the same definitions. The Ritz pairs
come from numpy.linalg.eigh of the dense tridiagonal matrix.

Reference spectra: the cases of tests/linsys_cases.py give the assembled float matrix bit for bit (exact family) or to one float rounding (random family:
the float-rounded exact matrix). Up to DENSE_LIMIT unknowns every eigenvalue is computed (scipy.linalg.eigh(A, D) for operator 1, eigvalsh(A) for operator
0); beyond, scipy.sparse.linalg.eigsh gives END_K eigenvalues at either end of B = L^-1 A L^-T (operator 1) or A (operator 0), and only Ritz values that
have converged there (rho_i <= 1e-8 T_norm) are held to them.
"""
import json
import os

import numpy as np
import scipy.linalg as sla
import scipy.sparse as sp
import scipy.sparse.linalg as spla

import linsys_cases as lc

EPS = float(np.finfo(np.float64).eps)
EPS32 = float(np.finfo(np.float32).eps)
BREAKDOWN = 1e-10
CONVERGED = 1e-8
MAX_M = 256
DENSE_LIMIT = 800
END_K = 12
FLAG_EXHAUSTED, FLAG_INDEFINITE, FLAG_NONFINITE, FLAG_DIAG_NOT_PD = 1, 2, 4, 8
TOLERANCE_FILE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "linsys_report_tolerances.json")
TOLERANCE_CAP = BREAKDOWN / EPS     # a condition, not a measurement: the tolerance stays below the stop threshold
MS = (8, 64, 256)

GPU_CASES = ["tiny_1", "tiny_2", "multi_1", "multi_%d" % (lc.LONG_SLOT + 1), "path_43", "path_pow2_diag_100", "star_65", "random_values_star_257",
             "two_components_plus_isolated", "grid2d_40x40", "indefinite_tiny_2", "indefinite_path_43", "indefinite_star_65", "indefinite_grid2d_40x40"]
NEGATIVE_ROW = {"indefinite_tiny_2": 1, "indefinite_path_43": 20, "indefinite_star_65": 0, "indefinite_grid2d_40x40": 820}


def start_vector(n):
    """the built-in start vector before normalisation: entry i in [-1, 1)."""
    with np.errstate(over="ignore"):
        z = (np.arange(n, dtype=np.uint64) + np.uint64(1)) * np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z = z ^ (z >> np.uint64(31))
    return (z >> np.uint64(11)).astype(np.float64) * 2.0 ** -52 - 1.0


def hash_value(i):
    """one entry, in Python integers (no numpy): the definition itself."""
    M = (1 << 64) - 1
    z = ((i + 1) * 0x9E3779B97F4A7C15) & M
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M
    z ^= z >> 31
    return float(z >> 11) * 2.0 ** -52 - 1.0


def case_matrix(case):
    """the assembled matrix as the engine stores it: the exact matrix rounded to float (exact family: unchanged), as float64 CSR."""
    A = lc.exact_matrix(case).tocsr()
    A.sum_duplicates()
    A.data = A.data.astype(np.float32).astype(np.float64)
    return A


def diag_blocks(A, nbr):
    """[nbr, 3, 3] diagonal blocks of a CSR matrix."""
    A = A.tocsr()
    i = 3 * np.arange(nbr)[:, None, None] + np.arange(3)[None, :, None]
    j = 3 * np.arange(nbr)[:, None, None] + np.arange(3)[None, None, :]
    i, j = np.broadcast_arrays(i, j)
    return np.asarray(A[i.reshape(-1), j.reshape(-1)]).reshape(nbr, 3, 3)


def chol_blocks(D):
    """(L [nbr, 3, 3] lower, smallest squared pivot [nbr], ok [nbr]) by the header's formulas from the upper entries; L is the identity where not ok."""
    a00, a01, a02, a11, a12, a22 = D[:, 0, 0], D[:, 0, 1], D[:, 0, 2], D[:, 1, 1], D[:, 1, 2], D[:, 2, 2]
    n = len(D)
    L = np.zeros((n, 3, 3))
    piv = a00.copy()
    ok = a00 > 0
    with np.errstate(all="ignore"):
        l00 = np.sqrt(np.where(ok, a00, 1.0))
        l10, l20 = a01 / l00, a02 / l00
        p1 = a11 - l10 * l10
        piv = np.where(ok & (p1 < piv), p1, piv)
        ok1 = ok & (p1 > 0)
        l11 = np.sqrt(np.where(ok1, p1, 1.0))
        l21 = (a12 - l20 * l10) / l11
        p2 = a22 - l20 * l20 - l21 * l21
        piv = np.where(ok1 & (p2 < piv), p2, piv)
        ok2 = ok1 & (p2 > 0)
        l22 = np.sqrt(np.where(ok2, p2, 1.0))
    L[:, 0, 0], L[:, 1, 0], L[:, 1, 1], L[:, 2, 0], L[:, 2, 1], L[:, 2, 2] = l00, l10, l11, l20, l21, l22
    L[~ok2] = np.eye(3)
    return L, piv, ok2


def solve_L(L, y):
    return np.linalg.solve(L, y.reshape(-1, 3, 1)).reshape(-1)


def solve_Lt(L, v):
    return np.linalg.solve(np.transpose(L, (0, 2, 1)), v.reshape(-1, 3, 1)).reshape(-1)


def operator(A, op, L=None):
    if op == 0:
        return lambda v: A @ v
    return lambda v: solve_L(L, A @ solve_Lt(L, v))


def lanczos(apply, v0, m):
    """(alpha, beta, T_norm, flags, V [k, n])"""
    n = len(v0)
    V = [v0 / np.linalg.norm(v0)]
    alpha, beta = [], []
    t_norm, flags = 0.0, 0
    for j in range(min(m, n)):
        w = apply(V[j])
        a = float(V[j] @ w)
        w = w - a * V[j] - (beta[j - 1] * V[j - 1] if j > 0 else 0.0)
        Vm = np.array(V)
        for _ in range(2):
            w = w - Vm.T @ (Vm @ w)
        b = float(np.linalg.norm(w))
        alpha.append(a)
        beta.append(b)
        if not (np.isfinite(a) and np.isfinite(b)):
            flags |= FLAG_NONFINITE
            break
        t_norm = max(t_norm, abs(a) + b + (beta[j - 1] if j > 0 else 0.0))
        if b <= BREAKDOWN * t_norm:
            flags |= FLAG_EXHAUSTED
            break
        if j + 1 == m or j + 1 == n:
            break
        V.append(w / b)
    return np.array(alpha), np.array(beta), t_norm, flags, np.array(V)


def ritz_pairs(alpha, beta):
    """(theta ascending [k], S [k, k] with COLUMN i the eigenvector of theta_i, rho [k])"""
    k = len(alpha)
    T = np.diag(alpha) + np.diag(beta[:k - 1], 1) + np.diag(beta[:k - 1], -1)
    theta, S = np.linalg.eigh(T)
    return theta, S, beta[k - 1] * np.abs(S[k - 1, :])


def fold_pivots(piv):
    bad = np.nonzero(~(piv > 0))[0]
    r = int(np.argmin(piv))
    return float(len(bad)), float(bad[0]) if len(bad) else -1.0, float(piv[r]), float(r)


def build_record(alpha, beta, t_norm, flags, n, piv):
    """(record [16], ritz [k, 2])"""
    out = np.zeros(16)
    out[11:15] = fold_pivots(piv)
    out[15] = n
    if flags & FLAG_DIAG_NOT_PD:
        out[1] = flags
        return out, np.zeros((0, 2))
    k = len(alpha)
    out[0] = k
    if flags & FLAG_NONFINITE:
        out[1] = flags
        return out, np.zeros((0, 2))
    theta, S, rho = ritz_pairs(alpha, beta)
    if theta[0] < -64 * EPS * t_norm:
        flags |= FLAG_INDEFINITE
    out[1] = flags
    out[2], out[3], out[4], out[5] = theta[0], rho[0], theta[-1], rho[-1]
    out[6] = theta[-1] / theta[0] if theta[0] > 0 else 0.0
    out[7], out[8] = t_norm, beta[-1]
    out[9] = (theta < 0).sum()
    out[10] = (rho <= CONVERGED * t_norm).sum()
    return out, np.stack([theta, rho], axis=1)


def run(A, op, m, start=None):
    """The report of a CSR matrix: dict(record, ritz, alpha, beta, V, L). start: None (built-in) or a vector."""
    n = A.shape[0]
    L, piv, ok = chol_blocks(diag_blocks(A, n // 3))
    if op == 1 and not ok.all():
        rec, ritz = build_record(np.zeros(0), np.zeros(0), 0.0, FLAG_DIAG_NOT_PD, n, piv)
        return dict(record=rec, ritz=ritz, alpha=np.zeros(0), beta=np.zeros(0), V=None, L=L)
    v0 = start_vector(n) if start is None else np.asarray(start, dtype=np.float64)
    alpha, beta, t_norm, flags, V = lanczos(operator(A, op, L), v0, m)
    rec, ritz = build_record(alpha, beta, t_norm, flags, n, piv)
    return dict(record=rec, ritz=ritz, alpha=alpha, beta=beta, V=V, L=L)


# ----------------------------------------------------------------------------------------------------------------------
# reference spectra
# ----------------------------------------------------------------------------------------------------------------------
_EIGS = {}


def reference_eigs(case, op):
    """(eigenvalues ascending, full): every eigenvalue (full) or END_K at either end. Operator 1 on a case whose diagonal is not PD has none: (None, False).
    Computed once per (case, operator)."""
    key = (case.name, op)
    if key not in _EIGS:
        A = case_matrix(case)
        n = case.n
        D = diag_blocks(A, case.nbr)
        L, piv, ok = chol_blocks(D)
        if op == 1 and not ok.all():
            _EIGS[key] = (None, False)
        elif n <= DENSE_LIMIT:
            Ad = A.toarray()
            if op == 1:
                w = sla.eigh(Ad, sla.block_diag(*D), eigvals_only=True)
            else:
                w = np.linalg.eigvalsh(Ad)
            _EIGS[key] = (np.sort(w), True)
        else:
            B = A
            if op == 1:
                Linv = sp.block_diag([np.linalg.inv(l) for l in L], format="csr")
                B = (Linv @ A @ Linv.T).tocsr()
                B = ((B + B.T) * 0.5).tocsr()
            k = min(END_K, n // 2 - 1)
            hi = spla.eigsh(B, k=k, which="LA", return_eigenvectors=False, tol=0, ncv=8 * k)
            if case.spd:
                lo = spla.eigsh(B.tocsc(), k=k, sigma=0.0, which="LM", return_eigenvectors=False, tol=0, ncv=8 * k)
            else:
                lo = spla.eigsh(B, k=k, which="SA", return_eigenvectors=False, tol=0, ncv=8 * k)
            _EIGS[key] = (np.sort(np.concatenate([lo, hi])), False)
    return _EIGS[key]


def certificate_excess(ritz, t_norm, eigs, full):
    """max over the Ritz values held to the reference of (distance to the nearest reference eigenvalue - rho) / (eps T_norm); with the ends alone, the
    values converged there (rho <= 1e-8 T_norm, inside END_K / 2 of an end of the Ritz list: the ends' own neighbours are then in the reference)."""
    theta, rho = ritz[:, 0], ritz[:, 1]
    sel = np.ones(len(theta), dtype=bool)
    if not full:
        sel = rho <= CONVERGED * t_norm
        pos = np.arange(len(theta))
        sel &= (pos < END_K // 2) | (pos >= len(theta) - END_K // 2)
    if not sel.any():
        return 0.0, 0
    dist = np.abs(theta[sel, None] - eigs[None, :]).min(axis=1)
    return float(((dist - rho[sel]) / (EPS * t_norm)).max()), int(sel.sum())


def load_tolerances():
    with open(TOLERANCE_FILE) as f:
        return json.load(f)


def tolerance(name):
    """c of the case: the Ritz values of a report lie within rho_i + c eps T_norm of an eigenvalue."""
    return float(load_tolerances()["c"][name])


def measure(names=None):
    """per case the largest certificate excess of the numpy run over both operators and m in MS; what the tolerance file holds is 4 x this."""
    out = {}
    for name in names or GPU_CASES:
        case = lc.BY_NAME[name]
        A = case_matrix(case)
        worst = 0.0
        for op in (0, 1):
            eigs, full = reference_eigs(case, op)
            if eigs is None:
                continue
            for m in MS:
                r = run(A, op, m)
                c, _ = certificate_excess(r["ritz"], r["record"][7], eigs, full)
                worst = max(worst, c)
            worst = max(worst, mode_excess(A, op, r))       # (r: the run of the largest m)
        out[name] = worst
    return out


def mode_excess(A, op, r):
    """what the two extreme Ritz vectors of a run miss the mode checks by, in units of eps T_norm: the measured residual |B u - theta u| against rho, and
    |A x - theta D x| against twice the measured residual (x = L^-T u for operator 1, u for operator 0)."""
    t_norm = r["record"][7]
    theta, S, rho = ritz_pairs(r["alpha"], r["beta"])
    B = operator(A, op, r["L"])
    D = sp.block_diag(list(diag_blocks(A, A.shape[0] // 3))).tocsr()
    worst = 0.0
    for i in (0, -1):
        u = r["V"].T @ S[:, i]
        x = solve_Lt(r["L"], u) if op == 1 else u
        res = np.linalg.norm(B(u) - theta[i] * u)
        gen = np.linalg.norm(A @ x - theta[i] * (D @ x if op == 1 else x))
        worst = max(worst, (res - rho[i]) / (EPS * t_norm), (gen - 2.0 * res) / (EPS * t_norm))
    return float(worst)


if __name__ == "__main__":   # python tests/linsys_report_ref.py: measure and write the tolerance file
    got = measure()
    doc = {"_how": "python tests/linsys_report_ref.py: per case the largest figure, in units of eps T_norm, by which the numpy restatement "
                   "(tests/linsys_report_ref.py: built-in start vector, both operators) misses a check that is held to the tolerance: over m in (8, 64, 256) "
                   "the distance of a Ritz value to the nearest reference eigenvalue (scipy.linalg.eigh / eigsh as reference_eigs states) minus rho_i; at "
                   "m = 256 for the two extreme Ritz vectors the measured residual |B u - theta u| minus rho, and |A x - theta D x| minus twice the measured "
                   "residual. The entry is 4 times that maximum, and never below 4: on the systems of 3 and 6 unknowns the restatement's own miss is a fraction of "
                   "one rounding (0.12 eps T_norm on tiny_1), and 4 times that is less than one ulp of the Ritz value itself, which no computation in double "
                   "can promise. No entry may exceed 1e-10 / eps.",
           "measured": got, "c": {k: max(4.0 * v, 4.0) for k, v in got.items()}}
    with open(TOLERANCE_FILE, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
    for k, v in got.items():
        print("%-32s measured %8.2f -> c = %8.2f" % (k, v, doc["c"][k]))
