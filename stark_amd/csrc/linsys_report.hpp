// linsys_report.hpp — linear-system report: what Lanczos with full reorthogonalisation sees of the assembled matrix (linsys_report.hip). Host and device
// code without HIP dependencies: tests/host_linsys_report compiles it with g++.
//
// Operators: LINSYS_A (0) B = A; LINSYS_JACOBI (1) B = L^-1 A L^-T with L block diagonal, L_r L_r^T = D_r the 3x3 Cholesky IN DOUBLE of the row's stored
// float diagonal block (what load_diag_block yields). The eigenvalues of B are those of A x = lambda D x, the spectrum the block-Jacobi PCG works on.
// PCG ITSELF applies sym3_inverse in FLOAT (solve.hip): its preconditioner is the float-rounded inverse of D_r, the report's the double Cholesky of the same
// stored block; the two spectra differ by the rounding of that inverse (relative 2^-24 times the block's condition number).
//
// Iteration j = 0 .. m-1 (1 <= m <= LINSYS_MAX_M): w = B v_j; alpha_j = v_j . w; w -= alpha_j v_j + beta_{j-1} v_{j-1}; twice classical Gram-Schmidt
// against v_0 .. v_j (c = V^T w, w -= V c); beta_j = |w|; T_norm = max_j (|alpha_j| + beta_j + beta_{j-1}). Stop after step j when
// beta_j <= LINSYS_BREAKDOWN * T_norm (flag +1), j + 1 == m or j + 1 == n; else v_{j+1} = w / beta_j. With k steps run, T is the k x k tridiagonal
// matrix; (theta_i, s_i) its eigenpairs (linsys_tridiag_eig), rho_i = beta_{k-1} |s_i[k-1]| the residual bound of Ritz value i.
//
// Summary record, LINSYS_REC = 16 doubles:
//   0 steps run k | 1 flags | 2 theta_min | 3 its rho | 4 theta_max | 5 its rho | 6 theta_max / theta_min, 0 where theta_min <= 0 | 7 T_norm | 8 beta_{k-1}
//   9 Ritz values < 0 | 10 Ritz values with rho_i <= 1e-8 T_norm | 11 diagonal blocks that are not positive definite | 12 the first such block row, -1: none
//   13 smallest squared Cholesky pivot over all rows | 14 its row | 15 n
//   flags: +1 Krylov space exhausted | +2 theta_min < -64 eps T_norm (Ritz values lie inside the spectrum's range: the matrix is proved indefinite)
//          +4 a non-finite value was met, slots 2..10 are zeros | +8 operator 1 refused for a diagonal block that is not PD, slots 0 and 2..10 are zeros
//   Slots 11..14 are filled for both operators.
// Mode record, LINSYS_MODE = 4: 0 theta | 1 rho | 2 |B u - theta u| measured by one more operator application | 3 index in the ascending list
// Nodal record, LINSYS_NODAL = 4 per block row: 0 |u_r|^2, the row's share of the unit Ritz vector u = V s | 1 |x_r| | 2 trace of D_r | 3 smallest squared
//   pivot of D_r
// Potential record, LINSYS_POT = 4: 0 sum q_e in element order | 1 sum |q_e| | 2 elements counted | 3 first element attaining the largest |q_e|, -1: none;
//   q_e = x_e^T H_e x_e with x the Ritz vector in DoF space.
#pragma once
#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#define LINSYS_HD __host__ __device__ __forceinline__
#else
#define LINSYS_HD inline
#endif
// The 3x3 factorisation and solves round every product and sum on its own (no fused multiply-add), so that the device, the host build of the tests and
// their numpy restatement give the same bits for the same block.
#if defined(__clang__)
#define LINSYS_NO_CONTRACT _Pragma("clang fp contract(off)")
#else
#define LINSYS_NO_CONTRACT
#endif

namespace mistark {

constexpr int LINSYS_A = 0, LINSYS_JACOBI = 1;
constexpr int LINSYS_MAX_M = 256;
constexpr int LINSYS_REC = 16, LINSYS_MODE = 4, LINSYS_NODAL = 4, LINSYS_POT = 4;
constexpr double LINSYS_BREAKDOWN = 1e-10;   // beta_j <= this * T_norm: the Krylov space is exhausted
constexpr double LINSYS_CONVERGED = 1e-8;    // rho_i <= this * T_norm counts in slot 10
constexpr double LINSYS_EPS = 2.220446049250313e-16;
constexpr int LINSYS_FLAG_EXHAUSTED = 1, LINSYS_FLAG_INDEFINITE = 2, LINSYS_FLAG_NONFINITE = 4, LINSYS_FLAG_DIAG_NOT_PD = 8;

// entry i of the built-in start vector before normalisation, in [-1, 1): splitmix64 of i + 1, all arithmetic in uint64
LINSYS_HD double linsys_start_value(uint64_t i)
{
    uint64_t z = (i + 1ull) * 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    z ^= z >> 31;
    return (double)(z >> 11) * 2.220446049250313e-16 - 1.0;  // 2^-52
}

// Cholesky of the symmetric 3x3 block with upper entries a00 a01 a02 a11 a12 a22 (the entries sym3_inverse reads): L = [l00; l10 l11; l20 l21 l22] in
// L[0..5] = l00 l10 l11 l20 l21 l22. Returns false at the first pivot that is not > 0 (or not finite); min_pivot is the smallest squared pivot met, the
// failing one included. Nothing of L is valid then.
LINSYS_HD bool linsys_chol3(const double a[6], double L[6], double& min_pivot)
{
    LINSYS_NO_CONTRACT
    const double p0 = a[0];
    min_pivot = p0;
    if (!(p0 > 0.0) || !(p0 < INFINITY)) return false;
    const double l00 = sqrt(p0), l10 = a[1] / l00, l20 = a[2] / l00;
    const double p1 = a[3] - l10 * l10;
    min_pivot = p1 < min_pivot || !(p1 == p1) ? p1 : min_pivot;
    if (!(p1 > 0.0) || !(p1 < INFINITY)) return false;
    const double l11 = sqrt(p1), l21 = (a[4] - l20 * l10) / l11;
    const double p2 = a[5] - l20 * l20 - l21 * l21;
    min_pivot = p2 < min_pivot || !(p2 == p2) ? p2 : min_pivot;
    if (!(p2 > 0.0) || !(p2 < INFINITY)) return false;
    L[0] = l00; L[1] = l10; L[2] = l11; L[3] = l20; L[4] = l21; L[5] = sqrt(p2);
    return true;
}
// w = L^-1 y
LINSYS_HD void linsys_solve_L(const double L[6], const double y[3], double w[3])
{
    LINSYS_NO_CONTRACT
    w[0] = y[0] / L[0];
    w[1] = (y[1] - L[1] * w[0]) / L[2];
    w[2] = (y[2] - L[3] * w[0] - L[4] * w[1]) / L[5];
}
// x = L^-T v
LINSYS_HD void linsys_solve_Lt(const double L[6], const double v[3], double x[3])
{
    LINSYS_NO_CONTRACT
    x[2] = v[2] / L[5];
    x[1] = (v[1] - L[4] * x[2]) / L[2];
    x[0] = (v[0] - L[1] * x[1] - L[3] * x[2]) / L[0];
}

// Eigenpairs of the symmetric tridiagonal k x k matrix with diagonal d[0..k) and off-diagonal e[0..k-1) (e[i] couples i and i + 1): implicit QL with
// Wilkinson shifts. On exit d holds the eigenvalues ASCENDING (ties in the order the iteration left them) and Z, [k][nz] row-major, row i = components
// first .. first + nz - 1 of the unit eigenvector of d[i] (first = 0, nz = k: the whole vector; first = k - 1, nz = 1: its last component, all a residual
// bound needs). e is destroyed (k entries of work space; e[k-1] need not be set). Returns the largest iteration count of an eigenvalue, -1 when one did
// not converge in 60.
inline int linsys_tridiag_eig(int k, double* d, double* e, double* Z, int first, int nz)
{
    for (int i = 0; i < k; i++)
        for (int c = 0; c < nz; c++) Z[(size_t)i * nz + c] = (i == first + c) ? 1.0 : 0.0;
    if (k > 0) e[k - 1] = 0.0;
    int worst = 0;
    for (int l = 0; l < k; l++) {
        int iter = 0, m;
        do {
            for (m = l; m < k - 1; m++) {
                const double dd = fabs(d[m]) + fabs(d[m + 1]);
                if (fabs(e[m]) <= 0.5 * LINSYS_EPS * dd) break;
            }
            if (m != l) {
                if (iter++ == 60) return -1;
                double g = (d[l + 1] - d[l]) / (2.0 * e[l]);
                double r = hypot(g, 1.0);
                g = d[m] - d[l] + e[l] / (g + (g >= 0.0 ? fabs(r) : -fabs(r)));
                double s = 1.0, c = 1.0, p = 0.0;
                int i;
                for (i = m - 1; i >= l; i--) {
                    double f = s * e[i];
                    const double b = c * e[i];
                    e[i + 1] = r = hypot(f, g);
                    if (r == 0.0) {
                        d[i + 1] -= p;
                        e[m] = 0.0;
                        break;
                    }
                    s = f / r;
                    c = g / r;
                    g = d[i + 1] - p;
                    r = (d[i] - g) * s + 2.0 * c * b;
                    p = s * r;
                    d[i + 1] = g + p;
                    g = c * r - b;
                    double* z0 = Z + (size_t)i * nz;
                    double* z1 = Z + (size_t)(i + 1) * nz;
                    for (int q = 0; q < nz; q++) {
                        f = z1[q];
                        z1[q] = s * z0[q] + c * f;
                        z0[q] = c * z0[q] - s * f;
                    }
                }
                if (r == 0.0 && i >= l) continue;
                d[l] -= p;
                e[l] = g;
                e[m] = 0.0;
            }
        } while (m != l);
        worst = iter > worst ? iter : worst;
    }
    // ascending by selection: k <= 256
    for (int i = 0; i + 1 < k; i++) {
        int best = i;
        for (int j = i + 1; j < k; j++)
            if (d[j] < d[best]) best = j;
        if (best != i) {
            const double t = d[i];
            d[i] = d[best];
            d[best] = t;
            for (int q = 0; q < nz; q++) {
                const double u = Z[(size_t)i * nz + q];
                Z[(size_t)i * nz + q] = Z[(size_t)best * nz + q];
                Z[(size_t)best * nz + q] = u;
            }
        }
    }
    return worst;
}

struct LinsysDiag  // what the Cholesky stage found, block rows in the caller's numbering
{
    double not_pd = 0.0, first_not_pd = -1.0, min_pivot = 0.0, min_pivot_row = -1.0;
};
// pivots[r]: smallest squared pivot of block row r (linsys_chol3). The first row attaining the minimum is reported; a NaN pivot counts as not PD and as
// smaller than any number.
inline LinsysDiag linsys_fold_pivots(const double* pivots, int64_t nbr)
{
    LinsysDiag D;
    bool have = false, nan_seen = false;
    for (int64_t r = 0; r < nbr; r++) {
        const double p = pivots[r];
        if (!(p > 0.0) || !(p < INFINITY)) {
            if (D.not_pd == 0.0) D.first_not_pd = (double)r;
            D.not_pd += 1.0;
        }
        const bool is_nan = !(p == p);
        if (!have || (is_nan && !nan_seen) || (!nan_seen && p < D.min_pivot)) {
            D.min_pivot = p;
            D.min_pivot_row = (double)r;
            have = true;
            nan_seen = nan_seen || is_nan;
        }
    }
    return D;
}

// The summary record and the Ritz list from the recurrence's coefficients. alpha, beta: k entries (beta[k-1] the last norm); ritz: [m][2] theta ascending,
// rho (rows >= k zero) or null; S: null, or [k][k] receiving the eigenvectors of T (row i belongs to theta_i); work: 3 k doubles (+ nothing when S given).
// flags_in: LINSYS_FLAG_EXHAUSTED / _NONFINITE / _DIAG_NOT_PD as the iteration set them. Returns false when the tridiagonal solver did not converge (the
// record is then flagged non-finite).
inline bool linsys_build_record(int k, int m, const double* alpha, const double* beta, double t_norm, int flags_in, int64_t n, const LinsysDiag& D, double* out, double* ritz,
                                double* S, double* work)
{
    for (int i = 0; i < LINSYS_REC; i++) out[i] = 0.0;
    if (ritz)
        for (int i = 0; i < 2 * m; i++) ritz[i] = 0.0;
    out[11] = D.not_pd;
    out[12] = D.first_not_pd;
    out[13] = D.min_pivot;
    out[14] = D.min_pivot_row;
    out[15] = (double)n;
    int flags = flags_in;
    if (flags & LINSYS_FLAG_DIAG_NOT_PD) {
        out[1] = (double)flags;
        return true;
    }
    out[0] = (double)k;
    bool ok = true;
    double* d = work;
    double* e = work + k;
    double* last = work + 2 * k;
    if (!(flags & LINSYS_FLAG_NONFINITE)) {
        for (int i = 0; i < k; i++) {
            d[i] = alpha[i];
            e[i] = beta[i];
        }
        ok = linsys_tridiag_eig(k, d, e, S ? S : last, S ? 0 : k - 1, S ? k : 1) >= 0;
        if (!ok) flags |= LINSYS_FLAG_NONFINITE;
    }
    if (flags & LINSYS_FLAG_NONFINITE) {
        out[1] = (double)flags;
        return ok;
    }
    const double bk = beta[k - 1];
    double n_neg = 0.0, n_conv = 0.0, rho_min = 0.0, rho_max = 0.0;
    for (int i = 0; i < k; i++) {
        const double rho = bk * fabs(S ? S[(size_t)i * k + (k - 1)] : last[i]);
        if (ritz) {
            ritz[2 * i] = d[i];
            ritz[2 * i + 1] = rho;
        }
        if (d[i] < 0.0) n_neg += 1.0;
        if (rho <= LINSYS_CONVERGED * t_norm) n_conv += 1.0;
        if (i == 0) rho_min = rho;
        if (i == k - 1) rho_max = rho;
    }
    if (d[0] < -64.0 * LINSYS_EPS * t_norm) flags |= LINSYS_FLAG_INDEFINITE;
    out[1] = (double)flags;
    out[2] = d[0];
    out[3] = rho_min;
    out[4] = d[k - 1];
    out[5] = rho_max;
    out[6] = d[0] > 0.0 ? d[k - 1] / d[0] : 0.0;
    out[7] = t_norm;
    out[8] = bk;
    out[9] = n_neg;
    out[10] = n_conv;
    return true;
}

}  // namespace mistark
