// TEST-ONLY host build of the wrench report's per-record header (stark_amd/csrc/wrench.hpp compiled with g++): lets the CPU test suite check the exact
// device arithmetic against the numpy reference of tests/wrench_ref.py without a GPU. Not part of the product library. With HOST_WRENCH_MAIN it is a
// stand-alone program (for a sanitizer build) that runs both records on a few fixed inputs and checks them against the map written out by hand.
#include "../../stark_amd/csrc/wrench.hpp"

using namespace mistark;

// gv, gw, w1: [n][3]; rec: [n][12]
extern "C" int host_wrench_slots(const double* gv, const double* gw, const double* w1, double dt, int n, double* rec)
{
    for (int e = 0; e < n; e++) wrench_slot_record(gv + 3 * (size_t)e, gw + 3 * (size_t)e, w1 + 3 * (size_t)e, dt, 1.0 / dt, rec + (size_t)WRENCH_REC * e);
    return 0;
}
// fv, fw, t0, v1, w1: [n][3]; rec: [n][16]
extern "C" int host_wrench_bodies(const double* fv, const double* fw, const double* t0, const double* v1, const double* w1, double dt, const double* about, int n, double* rec)
{
    for (int b = 0; b < n; b++)
        wrench_body_record(fv + 3 * (size_t)b, fw + 3 * (size_t)b, t0 + 3 * (size_t)b, v1 + 3 * (size_t)b, w1 + 3 * (size_t)b, dt, about, rec + (size_t)WRENCH_BODY_REC * b);
    return 0;
}

#ifdef HOST_WRENCH_MAIN
#include <cstdio>
#include <vector>
int main()
{
    const int n = 5;
    const double dt = 1.0 / 30.0;
    std::vector<double> gv(3 * n), gw(3 * n), w1(3 * n), t0(3 * n), v1(3 * n), rs((size_t)WRENCH_REC * n), rb((size_t)WRENCH_BODY_REC * n);
    for (int i = 0; i < 3 * n; i++) {
        gv[i] = i < 3 ? 0.0 : 0.37 * (i % 7) - 1.1;  // (the first record has |F| == 0)
        gw[i] = 0.21 * (i % 5) - 0.4;
        w1[i] = 9.0 * ((i * 3) % 4) - 13.0;
        t0[i] = 0.1 * i;
        v1[i] = 0.5 - 0.05 * i;
    }
    const double about[3] = {0.2, -0.1, 0.4};
    host_wrench_slots(gv.data(), gw.data(), w1.data(), dt, n, rs.data());
    host_wrench_bodies(gv.data(), gw.data(), t0.data(), v1.data(), w1.data(), dt, about, n, rb.data());
    int bad = 0;
    for (int e = 0; e < n; e++) {
        const double* a3 = &w1[3 * e];
        const double a[3] = {0.5 * dt * a3[0], 0.5 * dt * a3[1], 0.5 * dt * a3[2]};
        const double* x = &gw[3 * e];
        const double d = a[0] * x[0] + a[1] * x[1] + a[2] * x[2];
        const double y[3] = {x[0] + a[1] * x[2] - a[2] * x[1] + a[0] * d, x[1] + a[2] * x[0] - a[0] * x[2] + a[1] * d, x[2] + a[0] * x[1] - a[1] * x[0] + a[2] * d};
        for (int i = 0; i < 3; i++) {
            if (fabs(rb[(size_t)WRENCH_BODY_REC * e + 3 + i] - y[i]) > 1e-13 * (1.0 + fabs(y[i]))) bad++;
            if (fabs(rs[(size_t)WRENCH_REC * e + 3 + i] + y[i] / dt) > 1e-13 * (1.0 + fabs(y[i] / dt))) bad++;
        }
    }
    for (int i = 6; i < 10; i++)
        if (rs[i] != 0.0) bad++;
    std::printf("host_wrench: %d records, %d mismatches\n", n, bad);
    return bad ? 1 : 0;
}
#endif
