// TEST-ONLY host build of the friction report's arithmetic (stark_amd/csrc/friction_report.hpp compiled with g++): lets the CPU test suite check the exact
// device arithmetic against the numpy restatement of tests/friction_report_ref.py without a GPU. Not part of the product library.
// With -DHOST_FRICTION_REPORT_MAIN the file is a stand-alone program (no Python in the process): it runs the header over a fixture-sized input of every
// table, sticking and sliding, so that a sanitizer build can watch it.
#include "../../stark_amd/csrc/friction_report.hpp"

using namespace mistark;

// meta [n][6]: table, row, ga, gb, rba, rbb; vel [n][5][3]: va0 va1 vb0 vb1 vb2; T [n][6]; mu, fn [n]; bary [n][3] (unused places 0); ri [n][8];
// rd [n][24]; w [n][5]: the node weights wa[2], wb[3]
extern "C" int host_friction_rows(const int* meta, const double* vel, const double* T, const double* mu, const double* fn, const double* bary, double dt, double epsv, int n,
                                  int32_t* ri, double* rd, double* w)
{
    for (int i = 0; i < n; i++) {
        const int* M = meta + 6 * (size_t)i;
        D3 v[5];
        for (int j = 0; j < 5; j++) v[j] = d3(vel[(5 * (size_t)i + j) * 3], vel[(5 * (size_t)i + j) * 3 + 1], vel[(5 * (size_t)i + j) * 3 + 2]);
        friction_report_row(M[0], M[1], M[2], M[3], M[4], M[5], v, v + 2, T + 6 * (size_t)i, mu[i], fn[i], bary + 3 * (size_t)i, dt, epsv, ri + FR_NI * (size_t)i,
                            rd + FR_ND * (size_t)i, w + 5 * (size_t)i, w + 5 * (size_t)i + 2);
    }
    return 0;
}
// velocity of the point xloc of a rigid body (v1, w1, q0) into out[3]
extern "C" void host_friction_rigid_velocity(const double* v, const double* w, const double* q0, const double* xloc, double dt, double* out)
{
    const D3 r = fr_rigid_velocity(v, w, q0, xloc, dt);
    out[0] = r.x; out[1] = r.y; out[2] = r.z;
}

#ifdef HOST_FRICTION_REPORT_MAIN
#include <cmath>
#include <cstdio>
#include <vector>

int main()
{
    // 292 rows (the largest fixture's count) cycling through the 14 tables; velocities of alternating size, so that rows stick and slide; an orthonormal
    // tangent basis per row; rigid vertices through fr_rigid_velocity; one row without load (mu = 0)
    const int n = 292;
    const double dt = 0.01, epsv = 1e-3;
    std::vector<int> meta(6 * (size_t)n);
    std::vector<double> vel(15 * (size_t)n), T(6 * (size_t)n), mu(n), fn(n), bary(3 * (size_t)n), rd(FR_ND * (size_t)n), w(5 * (size_t)n);
    std::vector<int32_t> ri(FR_NI * (size_t)n);
    unsigned long long s = 88172645463325252ull;
    auto rnd = [&]() {
        s ^= s << 13;
        s ^= s >> 7;
        s ^= s << 17;
        return (double)(s >> 11) / 9007199254740992.0;
    };
    for (int i = 0; i < n; i++) {
        int* M = &meta[6 * (size_t)i];
        M[0] = FR_FIRST_TABLE + i % FR_N_TABLES; M[1] = i / FR_N_TABLES; M[2] = i % 3; M[3] = (i + 1) % 3; M[4] = M[0] >= 25 ? i % 2 : -1; M[5] = (M[0] >= 25 && M[0] < 29) ? (i + 1) % 2 : -1;
        const double size = (i / FR_N_TABLES) % 2 ? 1.0 : 1e-4;  // |u| = |v| dt: 1e-2 (sliding) or 1e-6 (sticking) beside epsu = 1e-5
        for (int j = 0; j < 5; j++) {
            const double q0[4] = {0.8, 0.2 * rnd(), 0.4, 0.4}, xl[3] = {rnd(), rnd(), rnd()}, v0[3] = {size * rnd(), size * rnd(), size * rnd()},
                         w0[3] = {size * rnd(), size * rnd(), size * rnd()};
            host_friction_rigid_velocity(v0, w0, q0, xl, dt, &vel[(5 * (size_t)i + j) * 3]);
        }
        double a[3] = {rnd() - 0.5, rnd() - 0.5, rnd() + 0.5}, b[3] = {rnd() + 0.5, rnd() - 0.5, rnd() - 0.5};
        const double na = std::sqrt(a[0] * a[0] + a[1] * a[1] + a[2] * a[2]);
        for (int c = 0; c < 3; c++) a[c] /= na;
        const double ab = a[0] * b[0] + a[1] * b[1] + a[2] * b[2];
        for (int c = 0; c < 3; c++) b[c] -= ab * a[c];
        const double nb = std::sqrt(b[0] * b[0] + b[1] * b[1] + b[2] * b[2]);
        for (int c = 0; c < 3; c++) {
            T[6 * (size_t)i + c] = a[c];
            T[6 * (size_t)i + 3 + c] = b[c] / nb;
        }
        mu[i] = i == 7 ? 0.0 : 0.3 + 0.4 * rnd();
        fn[i] = 1.0 + 10.0 * rnd();
        const double b0 = rnd(), b1 = (1.0 - b0) * rnd();
        bary[3 * (size_t)i] = b0; bary[3 * (size_t)i + 1] = b1; bary[3 * (size_t)i + 2] = 1.0 - b0 - b1;
    }
    host_friction_rows(meta.data(), vel.data(), T.data(), mu.data(), fn.data(), bary.data(), dt, epsv, n, ri.data(), rd.data(), w.data());
    int n_sliding = 0, n_noload = 0, n_bad = 0;
    double sum = 0.0;
    for (int i = 0; i < n; i++) {
        const int f = ri[FR_NI * (size_t)i + 7];
        const double* r = &rd[FR_ND * (size_t)i];
        n_sliding += (f & FR_SLIDING) != 0;
        n_noload += (f & FR_NO_LOAD) != 0;
        bool ok = ((f & FR_SLIDING) != 0) == !(r[5] < r[2]) && r[14] <= 1.0 && r[14] >= 0.0 && r[16] >= 0.0 && r[15] >= -1e-12 * r[13];
        for (int j = 0; j < FR_ND; j++) ok = ok && std::isfinite(r[j]);
        if ((f & FR_SLIDING) && !(f & FR_NO_LOAD)) ok = ok && std::fabs(r[13] - r[0] * r[1]) <= 1e-12 * r[0] * r[1];
        if (f & FR_NO_LOAD) ok = ok && r[13] == 0.0 && r[14] == 0.0 && r[16] == 0.0;
        n_bad += !ok;
        sum += r[16];
    }
    std::printf("rows %d sliding %d noload %d bad %d sum_E %.17g\n", n, n_sliding, n_noload, n_bad, sum);
    return (n_bad == 0 && n_noload == 1 && n_sliding > 0 && n_sliding < n) ? 0 : 1;
}
#endif
