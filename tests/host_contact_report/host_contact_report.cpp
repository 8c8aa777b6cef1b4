// TEST-ONLY host build of the contact report's arithmetic (stark_amd/csrc/contact_report.hpp compiled with g++): lets the CPU test suite check the exact
// device arithmetic against the numpy restatement of tests/contact_report_ref.py without a GPU. Not part of the product library.
// With -DHOST_CONTACT_REPORT_MAIN the file is a stand-alone program (no Python in the process): it runs the header over a fixture-sized input of every
// feature type, so that a sanitizer build can watch it.
#include "../../stark_amd/csrc/contact_report.hpp"

using namespace mistark;

// keys [n][7]: table, src, type, a, b, ga, gb; pos [n][9][3]: xa0 xa1 xb0 xb1 xb2 ra0 ra1 rb0 rb1; thick [n][2]; ri [n][8]; rd [n][16]; w [n][5]: the node
// weights wa[2], wb[3]
extern "C" int host_contact_rows(const int* keys, const double* pos, const double* thick, double k, int n, int32_t* ri, double* rd, double* w)
{
    for (int i = 0; i < n; i++) {
        const int* K = keys + 7 * (size_t)i;
        D3 x[9];
        for (int j = 0; j < 9; j++) x[j] = d3(pos[(9 * (size_t)i + j) * 3], pos[(9 * (size_t)i + j) * 3 + 1], pos[(9 * (size_t)i + j) * 3 + 2]);
        contact_report_row(K[0], K[1], K[2], K[3], K[4], K[5], K[6], x, x + 2, x + 5, x + 7, thick[2 * (size_t)i], thick[2 * (size_t)i + 1], k, ri + CR_NI * (size_t)i,
                           rd + CR_ND * (size_t)i);
        cr_weights(K[1], K[2], rd[CR_ND * (size_t)i + 14], rd[CR_ND * (size_t)i + 15], w + 5 * (size_t)i, w + 5 * (size_t)i + 2);
    }
    return 0;
}
extern "C" double host_contact_triangle_area(const double* a, const double* b, const double* c)
{
    return cr_triangle_area(d3(a[0], a[1], a[2]), d3(b[0], b[1], b[2]), d3(c[0], c[1], c[2]));
}

#ifdef HOST_CONTACT_REPORT_MAIN
#include <cmath>
#include <cstdio>
#include <vector>

int main()
{
    // 297 rows (the largest fixture's count) cycling through the 7 point-triangle and 9 edge-edge feature types over pseudo-random primitives; every
    // 16th edge-edge row has nearly parallel edges (a mollified row), one row has a point on its partner (a degenerate row)
    const int n = 297;
    std::vector<int> keys(7 * (size_t)n);
    std::vector<double> pos(27 * (size_t)n), thick(2 * (size_t)n), rd(CR_ND * (size_t)n), w(5 * (size_t)n);
    std::vector<int32_t> ri(CR_NI * (size_t)n);
    unsigned long long s = 88172645463325252ull;
    auto rnd = [&]() {
        s ^= s << 13;
        s ^= s >> 7;
        s ^= s << 17;
        return (double)(s >> 11) / 9007199254740992.0;
    };
    for (int i = 0; i < n; i++) {
        const int src = i & 1, type = src == 0 ? (i / 2) % 7 : (i / 2) % 9;
        int* K = &keys[7 * (size_t)i];
        K[0] = i % 21; K[1] = src; K[2] = type; K[3] = i; K[4] = n - i; K[5] = i % 3; K[6] = (i + 1) % 3;
        double* x = &pos[27 * (size_t)i];
        for (int j = 0; j < 27; j++) x[j] = rnd();
        if (src == 1 && (i / 2) % 16 == 5)
            for (int c = 0; c < 3; c++) x[9 + c] = x[6 + c] + (x[3 + c] - x[c]) * (1.0 + 1e-2 * c);  // edge b nearly parallel to edge a
        thick[2 * (size_t)i] = 0.3 + 0.2 * rnd();
        thick[2 * (size_t)i + 1] = 0.3 + 0.2 * rnd();
    }
    for (int c = 0; c < 3; c++) pos[6 + c] = pos[c];  // row 0 (P_T0): the point on the vertex
    host_contact_rows(keys.data(), pos.data(), thick.data(), 1e4, n, ri.data(), rd.data(), w.data());
    int n_mollified = 0, n_degenerate = 0, n_bad = 0;
    double sum = 0.0;
    for (int i = 0; i < n; i++) {
        const int f = ri[CR_NI * (size_t)i + 7];
        n_mollified += (f & CR_MOLLIFIED) != 0;
        n_degenerate += (f & CR_DEGENERATE) != 0;
        if (f & CR_DEGENERATE) continue;
        const double* r = &rd[CR_ND * (size_t)i];
        const double nn = r[8] * r[8] + r[9] * r[9] + r[10] * r[10];
        if (!(std::fabs(nn - 1.0) < 1e-9) || !std::isfinite(r[12]) || !std::isfinite(r[13])) n_bad++;
        sum += r[0];
    }
    std::printf("rows %d mollified %d degenerate %d bad %d sum_d %.17g\n", n, n_mollified, n_degenerate, n_bad, sum);
    return (n_bad == 0 && n_degenerate == 1 && n_mollified > 0) ? 0 : 1;
}
#endif
