// TEST-ONLY host build of the curved CCD's deviation bound (stark_amd/csrc/ccd_pad.hpp compiled with g++): lets the CPU test suite check the exact device
// arithmetic against the numpy restatement of tests/ccd_curved_ref.py without a GPU. Not part of the product library.
// With -DHOST_CCD_PAD_MAIN: a stand-alone program (for a sanitizer build) that drives the same functions over heap arrays and checks the bound against
// the rigid-body update itself.
#include "../../stark_amd/csrc/ccd_pad.hpp"

using namespace mistark;

// x_loc [n][3], dw [n][3], dt [n], tau [n] -> pad [n]
extern "C" int host_ccd_pad(const double* x_loc, const double* dw, const double* dt, const double* tau, int n, double* pad)
{
    for (int i = 0; i < n; i++) pad[i] = ccd_pad_vertex(x_loc + 3 * i, ccd_pad_phi(dt[i], dw[3 * i], dw[3 * i + 1], dw[3 * i + 2]), tau[i]);
    return 0;
}
// the vertex of one body at the fraction t of the direction: t0 + dt (v + t dv) + R1(q0, w + t dw, dt) x_loc
extern "C" int host_ccd_true_point(const double* t0, const double* q0, const double* v, const double* w, const double* dv, const double* dw, double dt, const double* x_loc,
                                   double t, double* out)
{
    const V3<double> W(w[0] + t * dw[0], w[1] + t * dw[1], w[2] + t * dw[2]);
    const V3<double> r = rb_R1(q0, W, dt) * V3<double>(x_loc[0], x_loc[1], x_loc[2]);
    out[0] = r.x + (t0[0] + dt * (v[0] + t * dv[0]));
    out[1] = r.y + (t0[1] + dt * (v[1] + t * dv[1]));
    out[2] = r.z + (t0[2] + dt * (v[2] + t * dv[2]));
    return 0;
}

#ifdef HOST_CCD_PAD_MAIN
#include <cstdio>
#include <vector>
int main()
{
    // a deterministic family of motions (an LCG, no library state): the sampled path never leaves the chord by more than the pad
    unsigned long long s = 88172645463325252ull;
    auto uni = [&]() {
        s = s * 6364136223846793005ull + 1442695040888963407ull;
        return (double)(s >> 11) / 9007199254740992.0;
    };
    const int n = 400, samples = 101;
    std::vector<double> x_loc(3 * n), dw(3 * n), dt(n), tau(n), pad(n);
    std::vector<double> q0(4 * n), w(3 * n);
    for (int i = 0; i < n; i++) {
        for (int k = 0; k < 3; k++) x_loc[3 * i + k] = 2.0 * uni() - 1.0, dw[3 * i + k] = (2.0 * uni() - 1.0) * 60.0 * uni(), w[3 * i + k] = (2.0 * uni() - 1.0) * 20.0;
        double nq = 0.0;
        for (int k = 0; k < 4; k++) q0[4 * i + k] = 2.0 * uni() - 1.0, nq += q0[4 * i + k] * q0[4 * i + k];
        for (int k = 0; k < 4; k++) q0[4 * i + k] /= ::sqrt(nq);
        dt[i] = 0.01 + 0.09 * uni();
        tau[i] = i % 3 == 0 ? 1.0 : (i % 3 == 1 ? 0.5 : 0.25);
    }
    host_ccd_pad(x_loc.data(), dw.data(), dt.data(), tau.data(), n, pad.data());
    const double zero[3] = {0.0, 0.0, 0.0};
    int bad = 0;
    double worst = 0.0;
    for (int i = 0; i < n; i++) {
        double a[3], b[3], p[3];
        host_ccd_true_point(zero, &q0[4 * i], zero, &w[3 * i], zero, &dw[3 * i], dt[i], &x_loc[3 * i], 0.0, a);
        host_ccd_true_point(zero, &q0[4 * i], zero, &w[3 * i], zero, &dw[3 * i], dt[i], &x_loc[3 * i], tau[i], b);
        for (int k = 0; k < samples; k++) {
            const double u = (double)k / (samples - 1);
            host_ccd_true_point(zero, &q0[4 * i], zero, &w[3 * i], zero, &dw[3 * i], dt[i], &x_loc[3 * i], u * tau[i], p);
            double dev = 0.0;
            for (int c = 0; c < 3; c++) {
                const double e = p[c] - (a[c] + u * (b[c] - a[c]));
                dev += e * e;
            }
            dev = ::sqrt(dev);
            if (dev > pad[i] * (1.0 + 1e-12) + 1e-15) bad++;
            if (pad[i] > 0.0 && dev / pad[i] > worst) worst = dev / pad[i];
        }
    }
    std::printf("motions %d bad %d worst ratio %.6f\n", n, bad, worst);
    return bad == 0 ? 0 : 1;
}
#endif
