// TEST-ONLY host build of the linear-system report's shared arithmetic (stark_amd/csrc/linsys_report.hpp compiled with g++): the start vector's hash, the
// 3x3 Cholesky and its two solves, the tridiagonal eigen solver and the record builder, for tests/test_linsys_report_cpu.py. Not part of the product.
// With -DHOST_LINSYS_REPORT_MAIN: a stand-alone program that drives the same functions (built with -fsanitize=address,undefined by the test).
#include "../../stark_amd/csrc/linsys_report.hpp"

#include <cstddef>
#include <vector>

using namespace mistark;

extern "C" void host_linsys_hash(const uint64_t* idx, int n, double* out)
{
    for (int i = 0; i < n; i++) out[i] = linsys_start_value(idx[i]);
}
// a: [n][6] upper entries a00 a01 a02 a11 a12 a22; L [n][6], pivot [n], ok [n]
extern "C" void host_linsys_chol(const double* a, int n, double* L, double* pivot, int* ok)
{
    for (int i = 0; i < n; i++) {
        double l[6] = {0, 0, 0, 0, 0, 0};
        ok[i] = linsys_chol3(a + 6 * (size_t)i, l, pivot[i]) ? 1 : 0;
        for (int k = 0; k < 6; k++) L[6 * (size_t)i + k] = l[k];
    }
}
// w = L^-1 y, x = L^-T y per block
extern "C" void host_linsys_solves(const double* L, const double* y, int n, double* w, double* x)
{
    for (int i = 0; i < n; i++) {
        linsys_solve_L(L + 6 * (size_t)i, y + 3 * (size_t)i, w + 3 * (size_t)i);
        linsys_solve_Lt(L + 6 * (size_t)i, y + 3 * (size_t)i, x + 3 * (size_t)i);
    }
}
// d [k], e [k] (e[k-1] ignored) -> theta [k] ascending, S [k][k] (row i: the eigenvector of theta[i]); returns the solver's iteration count or -1
extern "C" int host_linsys_tridiag(int k, const double* d, const double* e, double* theta, double* S)
{
    std::vector<double> ee(e, e + k);
    for (int i = 0; i < k; i++) theta[i] = d[i];
    return linsys_tridiag_eig(k, theta, ee.data(), S, 0, k);
}
// the same with the last components alone: last [k]
extern "C" int host_linsys_tridiag_last(int k, const double* d, const double* e, double* theta, double* last)
{
    std::vector<double> ee(e, e + k);
    for (int i = 0; i < k; i++) theta[i] = d[i];
    return linsys_tridiag_eig(k, theta, ee.data(), last, k - 1, 1);
}
// pivots [nbr] -> diag4: not PD, first such row, smallest pivot, its row; then the record and the Ritz list
extern "C" int host_linsys_record(int k, int m, const double* alpha, const double* beta, double t_norm, int flags, long long n, const double* pivots, long long nbr, double* out,
                                  double* ritz)
{
    const LinsysDiag D = linsys_fold_pivots(pivots, nbr);
    std::vector<double> work(3 * (size_t)(k > 0 ? k : 1));
    return linsys_build_record(k, m, alpha, beta, t_norm, flags, n, D, out, ritz, nullptr, work.data()) ? 0 : -1;
}

#ifdef HOST_LINSYS_REPORT_MAIN
#include <cstdio>
int main()
{
    int bad = 0;
    // hash: in [-1, 1), and the pinned first value
    for (uint64_t i : {0ull, 1ull, 2ull, 1ull << 32}) {
        const double v = linsys_start_value(i);
        if (!(v >= -1.0 && v < 1.0)) bad++;
    }
    // Cholesky and solves on an SPD block, a zero and a negative pivot
    const double a[6] = {4.0, 2.0, -1.0, 5.0, 0.5, 3.0};
    double L[6], piv;
    if (!linsys_chol3(a, L, piv)) bad++;
    const double y[3] = {1.0, -2.0, 0.5};
    double w[3], x[3], back[3];
    linsys_solve_L(L, y, w);
    back[0] = L[0] * w[0];
    back[1] = L[1] * w[0] + L[2] * w[1];
    back[2] = L[3] * w[0] + L[4] * w[1] + L[5] * w[2];
    for (int i = 0; i < 3; i++)
        if (std::fabs(back[i] - y[i]) > 1e-14) bad++;
    linsys_solve_Lt(L, y, x);
    back[0] = L[0] * x[0] + L[1] * x[1] + L[3] * x[2];
    back[1] = L[2] * x[1] + L[4] * x[2];
    back[2] = L[5] * x[2];
    for (int i = 0; i < 3; i++)
        if (std::fabs(back[i] - y[i]) > 1e-14) bad++;
    const double z[6] = {1.0, 1.0, 0.0, 1.0, 0.0, 1.0}, ng[6] = {-2.0, 0.0, 0.0, 1.0, 0.0, 1.0};
    if (linsys_chol3(z, L, piv) || piv != 0.0) bad++;
    if (linsys_chol3(ng, L, piv) || piv != -2.0) bad++;
    // the tridiagonal solver at every size 1..256 on the (-1, 2, -1) matrix, whose eigenvalues are 2 - 2 cos(i pi / (k + 1)); the record builder
    for (int k : {1, 2, 3, 64, 256}) {
        std::vector<double> d((size_t)k, 2.0), e((size_t)k, -1.0), S((size_t)k * k), beta((size_t)k, 1.0), ritz(2 * (size_t)k), work(3 * (size_t)k);
        std::vector<double> alpha = d;
        if (linsys_tridiag_eig(k, d.data(), e.data(), S.data(), 0, k) < 0) bad++;
        for (int i = 0; i < k; i++)
            if (std::fabs(d[(size_t)i] - (2.0 - 2.0 * std::cos((i + 1) * 3.141592653589793 / (k + 1)))) > 8.0 * k * LINSYS_EPS * 4.0) bad++;
        double out[LINSYS_REC];
        std::vector<double> piv2(5, 1.0);
        piv2[3] = -1.0;
        const LinsysDiag D = linsys_fold_pivots(piv2.data(), 5);
        if (D.first_not_pd != 3.0 || D.min_pivot_row != 3.0) bad++;
        if (!linsys_build_record(k, k, alpha.data(), beta.data(), 4.0, 0, 3 * k, D, out, ritz.data(), nullptr, work.data())) bad++;
        if (out[0] != (double)k || out[9] != 0.0) bad++;
        if (!linsys_build_record(k, k, alpha.data(), beta.data(), 4.0, LINSYS_FLAG_DIAG_NOT_PD, 3 * k, D, out, ritz.data(), nullptr, work.data())) bad++;
        if (out[0] != 0.0 || out[1] != 8.0 || out[12] != 3.0) bad++;
    }
    std::printf("%d mismatches\n", bad);
    return bad ? 1 : 0;
}
#endif
