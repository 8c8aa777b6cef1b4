// spectrum_report.hpp — Hessian spectrum report: the eigenvalues of one element Hessian and what the PSD projection (project.hip) would make of them,
// without eigenvectors and without writing the matrix. Host and device code: tests/host_spectrum compiles it with g++.
//
//   spectrum_record<n>(H, eps, rec, spectrum)   H: n x n row-major as stored (n = 3 NB, NB = 1..8), spectrum: n doubles or null
//
// Cyclic-by-round Jacobi on a copy of H: the round-robin pair schedule of k_project_eig (spectrum_partner = project.hip's rr_partner; the rotations of a
// round are disjoint, so applying them one after the other is the parallel round), its stop rule off <= SPEC_OFF_TOL * fro (off, fro: squared Frobenius
// norms of the off-diagonal part and of the matrix), at most SPEC_MAX_SWEEPS sweeps, and its `fabs(apq) > 1e-300` guard. The eigenvalues are the diagonal
// at the stop: by Weyl every sorted one is within sqrt(off) of a true eigenvalue of the matrix the rotations produced, which is the certificate the
// projection's clamping decisions rest on.
//
// One record of SPEC_REC = 10 doubles:
//   0  lambda_min                      1  lambda_max
//   2  eigenvalues < eps (the projection's own test, `l < eps`)            3  eigenvalues < 0
//   4  deficit sqrt(sum_{l < eps} (eps - l)^2): the Frobenius norm of what a clamping projection adds
//   5  ||H||_F of the stored entries (column by column, columns in order)   6  trace of the stored diagonal
//   7  sweeps run                      8  sqrt(off) at the stop
//   9  flags as a double: +1 field 2 > 0 (mistark_project would change the element), +2 a stored entry is not finite (fields 0..8 and the spectrum are
//      zeros then), +4 not converged in SPEC_MAX_SWEEPS sweeps
// spectrum: the n eigenvalues ascending, placed by rank counting (rank of l_c = #{k: l_k < l_c or (l_k == l_c and k < c)}): deterministic, -0.0 and +0.0
// keep their index order.
// Nodal record (SPEC_NODAL = 5, per block row): elements touching the row, of them flagged +1, smallest lambda_min among the finite ones (0 where none),
//   sum of deficit^2, potential id holding the smallest (-1 where none).
// Potential record (SPEC_POT = 10): elements, flagged +1, with lambda_min < 0, non-finite, not converged, smallest lambda_min, first element attaining it
//   (-1: none), largest lambda_max, sqrt(sum deficit^2), first non-finite element (-1: none). Minimum and maximum run over the finite elements.
#pragma once
#include <cmath>

#include "hdual.hpp"

namespace mistark {

constexpr int SPEC_REC = 10;
constexpr int SPEC_NODAL = 5;
constexpr int SPEC_POT = 10;
constexpr int SPEC_MAX_SWEEPS = 30;
constexpr double SPEC_OFF_TOL = 1e-24;  // = JACOBI_OFF_TOL (kernels_common.hpp; spectrum_report.hip asserts it)
constexpr double SPEC_APQ_GUARD = 1e-300;

// partner of player i in round r of the round-robin schedule of m players (m even): pairs (m-1, r), ((r+k) % (m-1), (r-k) % (m-1))
MS_HD int spectrum_partner(int m, int r, int i) { return i == m - 1 ? r : (i == r ? m - 1 : (2 * r - i + 2 * (m - 1)) % (m - 1)); }

// new[p] = cs old[p] - sn old[q];  new[q] = sn old[p] + cs old[q]   (p < q; IEEE division and square root: k_project_eig's formula)
MS_HD void spectrum_rotation(double app, double aqq, double apq, double& cs, double& sn)
{
    const double theta = (aqq - app) / (2.0 * apq);
    const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
    cs = 1.0 / sqrt(t * t + 1.0);
    sn = t * cs;
}

// rank of lam[c] in ascending order, ties by index
template <int n>
MS_HD int spectrum_rank(const double* lam, int c)
{
    int rank = 0;
    for (int k = 0; k < n; k++) rank += (lam[k] < lam[c] || (lam[k] == lam[c] && k < c)) ? 1 : 0;
    return rank;
}

// the record from the eigenvalues (index order) and the figures of the iteration; fro2, off: squared norms
template <int n>
MS_HD void spectrum_finish(const double* lam, double eps, double fro2, double trace, int sweeps, double off, bool converged, bool finite, double* rec)
{
    if (!finite) {
        for (int f = 0; f < SPEC_REC - 1; f++) rec[f] = 0.0;
        rec[9] = 2.0;
        return;
    }
    double lo = lam[0], hi = lam[0], def2 = 0.0;
    int below = 0, neg = 0;
    for (int k = 0; k < n; k++) {
        const double l = lam[k];
        lo = l < lo ? l : lo;
        hi = l > hi ? l : hi;
        if (l < eps) {
            below++;
            def2 += (eps - l) * (eps - l);
        }
        if (l < 0.0) neg++;
    }
    rec[0] = lo;
    rec[1] = hi;
    rec[2] = (double)below;
    rec[3] = (double)neg;
    rec[4] = sqrt(def2);
    rec[5] = sqrt(fro2);
    rec[6] = trace;
    rec[7] = (double)sweeps;
    rec[8] = sqrt(off);
    rec[9] = (double)((below > 0 ? 1 : 0) + (converged ? 0 : 4));
}

template <int n>
MS_HD void spectrum_record(const double* H, double eps, double* rec, double* spectrum)
{
    constexpr int m = (n + 1) & ~1;
    double A[n * n];
    bool finite = true;
    double fro2 = 0.0, trace = 0.0;
    for (int c = 0; c < n; c++) {  // column by column, as the kernel's lanes hold them
        double s = 0.0;
        for (int i = 0; i < n; i++) {
            const double v = H[i * n + c];
            A[i * n + c] = v;
            finite = finite && std::isfinite(v);
            s += v * v;
        }
        fro2 += s;
        trace += H[c * n + c];
    }
    double lam[n];
    for (int k = 0; k < n; k++) lam[k] = 0.0;
    int sweeps = 0;
    double off = 0.0;
    bool converged = false;
    if (finite) {
        for (;;) {
            off = 0.0;
            for (int c = 0; c < n; c++) {
                double s = 0.0;
                for (int i = 0; i < n; i++) s += i == c ? 0.0 : A[i * n + c] * A[i * n + c];
                off += s;
            }
            if (off <= SPEC_OFF_TOL * fro2) {
                converged = true;
                break;
            }
            if (sweeps == SPEC_MAX_SWEEPS) break;
            for (int r = 0; r < m - 1; r++)
                for (int p = 0; p < n; p++) {
                    const int q = spectrum_partner(m, r, p);
                    if (q <= p || q >= n) continue;
                    const double apq = A[p * n + q];
                    if (!(fabs(apq) > SPEC_APQ_GUARD)) continue;
                    double cs, sn;
                    spectrum_rotation(A[p * n + p], A[q * n + q], apq, cs, sn);
                    for (int i = 0; i < n; i++) {  // columns: A <- A J
                        const double x = A[i * n + p], y = A[i * n + q];
                        A[i * n + p] = cs * x - sn * y;
                        A[i * n + q] = sn * x + cs * y;
                    }
                    for (int j = 0; j < n; j++) {  // rows: A <- J^T A
                        const double x = A[p * n + j], y = A[q * n + j];
                        A[p * n + j] = cs * x - sn * y;
                        A[q * n + j] = sn * x + cs * y;
                    }
                }
            sweeps++;
        }
        for (int k = 0; k < n; k++) lam[k] = A[k * n + k];
    }
    spectrum_finish<n>(lam, eps, fro2, trace, sweeps, off, converged, finite, rec);
    if (spectrum) {
        if (finite)
            for (int c = 0; c < n; c++) spectrum[spectrum_rank<n>(lam, c)] = lam[c];
        else
            for (int c = 0; c < n; c++) spectrum[c] = 0.0;
    }
}

}  // namespace mistark
