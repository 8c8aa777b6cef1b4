// stress.hpp — stress and strain readout of the strain potentials: what the closed forms compute on the way to the gradient and throw away.
//   EnergyTetStrain / _Elasticity_Only       (tet_closed.hpp)   tet_stress<FULL>
//   EnergyTriangleStrain / _Elasticity_Only  (tri_closed.hpp)   tri_stress<FULL>
//   EnergySegmentStrain / _Elasticity_Only   (energies.hpp)     seg_stress<FULL>
// in[]: the gathered inputs of one element in the reference's binding order, the same array the evaluation kernels read. The state is the
// end-of-step state x1 = x0 + dt v1. Host and device code: tests/host_stress compiles it with g++.
//
// One record of STRESS_REC = 16 doubles, the same for the three kinds:
//   0..5   Cauchy stress in the world frame, xx yy zz xy yz zx [Pa]
//   6      von Mises stress of that tensor (3-D formula)
//   7      mean stress tr(sigma) / 3
//   8      J: volume ratio (tet), area ratio (triangle), length ratio (segment)
//   9..11  principal stretches, descending (triangle: two, then 0; segment: one, then 0, 0)
//   12     largest principal Green strain (stretch_max^2 - 1) / 2
//   13     energy density psi [J/m^3] exactly as the potential evaluates it: elastic + damping + strain limiting (not the triangle's inflation term)
//   14     rest measure m, element energy = m psi: det(DX) / 6 (tet), thickness * rest area (triangle), pi r^2 l_rest (segment)
//   15     flags as a double: +1 a strain-limiting branch is active, +2 degenerate
// Degenerate elements (J <= 0 for a tet, det C <= 0 for a triangle, zero length for a segment) set flag 2 and report zeros in 0..7 and 12; 8..11,
// 13 and 14 are still reported where they are finite (a triangle's psi holds log J: it is reported as 0 there).
//   tet      sigma = P F^T / J,  P = dpsi/dF = c1 F + lambda'(J - alpha) cof F + F T  =>  sigma = (c1 F F^T + F T F^T) / J + lambda'(J - alpha) I
//   triangle sigma = F S F^T / J,  S = 2 dpsi/dC, J = sqrt(det C): a symmetric world-frame tensor tangent to the deformed triangle. The inflation term is
//            a load, not a stress: it is in neither sigma nor psi.
//   segment  sigma = (N / (pi r^2)) t t^T,  N = dE/dl of the whole element energy (the reference's oddly scaled damping term included), t the unit tangent
// The nodal readout (stress.hip: k_stress_nodal) averages fields 0..8 with the weights m. Its entry 6 is the AVERAGE OF THE ELEMENTS' von Mises values,
// not the von Mises value of the averaged tensor.
#pragma once
#include "tri_closed.hpp"

#ifndef M_PI
#define M_PI 3.14159265358979323846
#endif

namespace mistark {

constexpr int STRESS_REC = 16;
constexpr int STRESS_NODAL = 10;       // nodal record: the weighted averages of fields 0..8, then the weight sum
constexpr int STRESS_JACOBI_SWEEPS = 6;  // cyclic Jacobi on a symmetric 3 x 3 converges quadratically: off/|A| 1e-1 -> 1e-2 -> 1e-4 -> 1e-8 -> 1e-16, one to spare

// von Mises, mean stress and flags into a record whose tensor is set; a degenerate element reports zeros in 0..7 and 12
MS_HD void stress_finish(double* rec, bool limiting, bool degenerate)
{
    if (degenerate) {
        rec[0] = rec[1] = rec[2] = rec[3] = rec[4] = rec[5] = 0.0;
        rec[12] = 0.0;
    }
    const double dxy = rec[0] - rec[1], dyz = rec[1] - rec[2], dzx = rec[2] - rec[0];
    rec[6] = ::sqrt(0.5 * (dxy * dxy + dyz * dyz + dzx * dzx) + 3.0 * (rec[3] * rec[3] + rec[4] * rec[4] + rec[5] * rec[5]));
    rec[7] = (rec[0] + rec[1] + rec[2]) / 3.0;
    rec[15] = (limiting ? 1.0 : 0.0) + (degenerate ? 2.0 : 0.0);
}

// one Jacobi rotation that annihilates apq; arp / arq are the two other off-diagonal entries of rows p and q
MS_HD void stress_jacobi_rotate(double& app, double& aqq, double& apq, double& arp, double& arq)
{
    if (apq == 0.0) return;
    const double theta = (aqq - app) / (2.0 * apq);
    const double t = (theta >= 0.0 ? 1.0 : -1.0) / (::fabs(theta) + ::sqrt(theta * theta + 1.0));  // (|theta| beyond 1e154: t = 0, nothing left to do)
    const double c = 1.0 / ::sqrt(t * t + 1.0), s = t * c;
    app -= t * apq;
    aqq += t * apq;
    apq = 0.0;
    const double rp = c * arp - s * arq, rq = s * arp + c * arq;
    arp = rp;
    arq = rq;
}
// eigenvalues of the symmetric 3 x 3 (a00 a11 a22 a01 a12 a02), descending: a fixed number of cyclic sweeps on named scalars (no runtime-indexed array)
MS_HD void stress_eig_sym3(double a00, double a11, double a22, double a01, double a12, double a02, double& l0, double& l1, double& l2)
{
    for (int sweep = 0; sweep < STRESS_JACOBI_SWEEPS; sweep++) {
        stress_jacobi_rotate(a00, a11, a01, a02, a12);  // (0,1): third index 2
        stress_jacobi_rotate(a00, a22, a02, a01, a12);  // (0,2): third index 1
        stress_jacobi_rotate(a11, a22, a12, a01, a02);  // (1,2): third index 0
    }
    double t;
    if (a00 < a11) { t = a00; a00 = a11; a11 = t; }
    if (a11 < a22) { t = a11; a11 = a22; a22 = t; }
    if (a00 < a11) { t = a00; a00 = a11; a11 = t; }
    l0 = a00;
    l1 = a11;
    l2 = a22;
}

// in[]: v1[4] (0..11), x0[4] (12..23), X[4] (24..35), then EO: scale, e, nu, dt | FULL: scale, e, nu, strain_limit, strain_limit_stiffness, damping, dt
template <bool FULL>
MS_HD void tet_stress(const double* in, double* rec)
{
    const double scale = in[36], e = in[37], nu = in[38];
    const double strain_limit = FULL ? in[39] : 0.0, sl_k = FULL ? in[40] : 0.0, damping = FULL ? in[41] : 0.0;
    const double dt = FULL ? in[42] : in[39];

    // rest shape and deformation gradient(s): as tet_closed_eval_to
    double DX[3][3];
    for (int k = 0; k < 3; k++)
        for (int i = 0; i < 3; i++) DX[i][k] = scale * (in[24 + 3 * (k + 1) + i] - in[24 + i]);
    const double c00 = DX[1][1] * DX[2][2] - DX[1][2] * DX[2][1];
    const double c01 = DX[1][2] * DX[2][0] - DX[1][0] * DX[2][2];
    const double c02 = DX[1][0] * DX[2][1] - DX[1][1] * DX[2][0];
    const double detDX = DX[0][0] * c00 + DX[0][1] * c01 + DX[0][2] * c02;
    const double idet = 1.0 / detDX;
    double w[4][3];
    w[1][0] = c00 * idet;
    w[1][1] = (DX[0][2] * DX[2][1] - DX[0][1] * DX[2][2]) * idet;
    w[1][2] = (DX[0][1] * DX[1][2] - DX[0][2] * DX[1][1]) * idet;
    w[2][0] = c01 * idet;
    w[2][1] = (DX[0][0] * DX[2][2] - DX[0][2] * DX[2][0]) * idet;
    w[2][2] = (DX[0][2] * DX[1][0] - DX[0][0] * DX[1][2]) * idet;
    w[3][0] = c02 * idet;
    w[3][1] = (DX[0][1] * DX[2][0] - DX[0][0] * DX[2][1]) * idet;
    w[3][2] = (DX[0][0] * DX[1][1] - DX[0][1] * DX[1][0]) * idet;
    for (int j = 0; j < 3; j++) w[0][j] = -(w[1][j] + w[2][j] + w[3][j]);
    const double vol = detDX / 6.0;
    double F[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}}, F0[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}};
    for (int a = 0; a < 4; a++)
        for (int i = 0; i < 3; i++) {
            const double x0 = in[12 + 3 * a + i];
            const double x1 = x0 + dt * in[3 * a + i];
            for (int j = 0; j < 3; j++) {
                F[i][j] += x1 * w[a][j];
                if (FULL) F0[i][j] += x0 * w[a][j];
            }
        }
    const double J = F[0][0] * (F[1][1] * F[2][2] - F[2][1] * F[1][2]) + F[1][0] * (F[2][1] * F[0][2] - F[0][1] * F[2][2]) + F[2][0] * (F[0][1] * F[1][2] - F[1][1] * F[0][2]);
    double Ic = 0.0;
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) Ic += F[i][j] * F[i][j];
    double Cg[3][3];  // right Cauchy-Green tensor F^T F
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) Cg[i][j] = F[0][i] * F[0][j] + F[1][i] * F[1][j] + F[2][i] * F[2][j];

    const double mu = e / (2.0 * (1.0 + nu));
    const double lambda = (e * nu) / ((1.0 + nu) * (1.0 - 2.0 * nu));
    const double mu_ = 4.0 / 3.0 * mu;
    const double lambda_ = lambda + 5.0 / 6.0 * mu;
    const double alpha = 1.0 + mu_ / lambda_ - mu_ / (4.0 * lambda_);
    const double Jm = J - alpha;
    double psi = 0.5 * mu_ * (Ic - 3.0) + 0.5 * lambda_ * Jm * Jm - 0.5 * mu_ * ::log(Ic + 1.0);
    const double c1 = mu_ * (1.0 - 1.0 / (Ic + 1.0));
    const double c3 = lambda_ * Jm;

    double T[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}};  // dphi/dE
    bool limiting = false;
    if (FULL) {
        double E1[3][3], D[3][3];
        const double cd = damping / (dt * dt);
        double ss = 0.0;
        for (int i = 0; i < 3; i++)
            for (int j = 0; j < 3; j++) {
                const double s0 = F0[0][i] * F0[0][j] + F0[1][i] * F0[1][j] + F0[2][i] * F0[2][j];
                E1[i][j] = 0.5 * (Cg[i][j] - (i == j ? 1.0 : 0.0));
                const double s = E1[i][j] - 0.5 * (s0 - (i == j ? 1.0 : 0.0));
                ss += s * s;
                T[i][j] = cd * s;
            }
        psi += 0.5 * cd * ss;
        const double trE = E1[0][0] + E1[1][1] + E1[2][2];
        double n2 = 0.0;
        for (int i = 0; i < 3; i++)
            for (int j = 0; j < 3; j++) {
                D[i][j] = E1[i][j] - (i == j ? trE / 3.0 : 0.0);
                n2 += D[i][j] * D[i][j];
            }
        const double gam = 0.81649658092772603;  // sqrt(2/3)
        const double n = ::sqrt(n2);
        const double dl = trE / 3.0 + gam * n - strain_limit;
        if (dl > 0.0) {
            limiting = true;
            psi += sl_k * dl * dl * dl / 3.0;
            const double gn = n > 0.0 ? gam / n : 0.0;  // (a purely volumetric strain has no deviatoric direction)
            for (int i = 0; i < 3; i++)
                for (int j = 0; j < 3; j++) T[i][j] += sl_k * dl * dl * ((i == j ? 1.0 / 3.0 : 0.0) + gn * D[i][j]);
        }
    }
    // sigma J = F (c1 I + T) F^T + c3 J I   (cof F F^T = J I)
    double A[3][3];
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) A[i][j] = c1 * F[i][j] + (FULL ? F[i][0] * T[0][j] + F[i][1] * T[1][j] + F[i][2] * T[2][j] : 0.0);
    const bool degenerate = !(J > 0.0);
    const double iJ = degenerate ? 0.0 : 1.0 / J;
    rec[0] = (A[0][0] * F[0][0] + A[0][1] * F[0][1] + A[0][2] * F[0][2]) * iJ + c3;
    rec[1] = (A[1][0] * F[1][0] + A[1][1] * F[1][1] + A[1][2] * F[1][2]) * iJ + c3;
    rec[2] = (A[2][0] * F[2][0] + A[2][1] * F[2][1] + A[2][2] * F[2][2]) * iJ + c3;
    rec[3] = (A[0][0] * F[1][0] + A[0][1] * F[1][1] + A[0][2] * F[1][2]) * iJ;
    rec[4] = (A[1][0] * F[2][0] + A[1][1] * F[2][1] + A[1][2] * F[2][2]) * iJ;
    rec[5] = (A[2][0] * F[0][0] + A[2][1] * F[0][1] + A[2][2] * F[0][2]) * iJ;
    double l0, l1, l2;
    stress_eig_sym3(Cg[0][0], Cg[1][1], Cg[2][2], Cg[0][1], Cg[1][2], Cg[0][2], l0, l1, l2);
    rec[8] = J;
    rec[9] = ::sqrt(::fmax(l0, 0.0));
    rec[10] = ::sqrt(::fmax(l1, 0.0));
    rec[11] = ::sqrt(::fmax(l2, 0.0));
    rec[12] = 0.5 * (l0 - 1.0);
    rec[13] = psi;
    rec[14] = vol;
    stress_finish(rec, limiting, degenerate);
}

// in[]: v1[3] (0..8), x0[3] (9..17), X[3] (18..26), scale, thickness, e, nu, then FULL: strain_damping, strain_limit, strain_limit_stiffness, inflation, dt
// | EO: inflation, dt
template <bool FULL>
MS_HD void tri_stress(const double* in, double* rec)
{
    const int p = 27;
    const double scale = in[p], thickness = in[p + 1], e = in[p + 2], nu = in[p + 3];
    const double damping = FULL ? in[p + 4] : 0.0, strain_limit = FULL ? in[p + 5] : 0.0, sl_k = FULL ? in[p + 6] : 0.0;
    const double dt = in[FULL ? p + 8 : p + 5];
    V3<double> x1[3], x0[3], Xs[3];
    for (int i = 0; i < 3; i++) {
        x0[i] = V3<double>(in[9 + 3 * i], in[10 + 3 * i], in[11 + 3 * i]);
        x1[i] = V3<double>(x0[i].x + dt * in[3 * i], x0[i].y + dt * in[3 * i + 1], x0[i].z + dt * in[3 * i + 2]);
        Xs[i] = V3<double>(scale * in[18 + 3 * i], scale * in[19 + 3 * i], scale * in[20 + 3 * i]);
    }
    // rest triangle in its own plane, F = [f0 | f1]: as tri_closed_eval
    const double rest_area = 0.5 * norm(cross(Xs[0] - Xs[2], Xs[1] - Xs[2]));
    const V3<double> u = normalized(Xs[1] - Xs[0]);
    const V3<double> n = cross(u, Xs[2] - Xs[0]);
    const V3<double> v = normalized(cross(u, n));
    const double a00 = dot(u, Xs[1]) - dot(u, Xs[0]), a01 = dot(u, Xs[2]) - dot(u, Xs[0]);
    const double a10 = dot(v, Xs[1]) - dot(v, Xs[0]), a11 = dot(v, Xs[2]) - dot(v, Xs[0]);
    const double idet = 1.0 / (a00 * a11 - a01 * a10);
    const double i00 = a11 * idet, i01 = -a01 * idet, i10 = -a10 * idet, i11 = a00 * idet;
    const V3<double> d1 = x1[1] - x1[0], d2 = x1[2] - x1[0];
    const V3<double> f0 = i00 * d1 + i10 * d2, f1 = i01 * d1 + i11 * d2;
    const double C00 = dot(f0, f0), C01 = dot(f0, f1), C11 = dot(f1, f1);
    TriParams P{};
    P.mu = e / (2.0 * (1.0 + nu));
    P.lambda = (e * nu) / ((1.0 + nu) * (1.0 - nu));  // 2D
    P.damping = damping;
    P.strain_limit = strain_limit;
    P.sl_k = sl_k;
    bool limiting = false;
    if (FULL) {
        const V3<double> e1 = x0[1] - x0[0], e2 = x0[2] - x0[0];
        const V3<double> g0 = i00 * e1 + i10 * e2, g1 = i01 * e1 + i11 * e2;
        P.P00 = 0.5 * (dot(g0, g0) - 1.0);
        P.P01 = 0.5 * dot(g0, g1);
        P.P11 = 0.5 * (dot(g1, g1) - 1.0);
        P.idt = 1.0 / dt;
        // the larger eigenvalue of E, as tri_density branches on it (the smaller one exceeds the limit only if this one does)
        const double E00 = 0.5 * (C00 - 1.0), E01 = 0.5 * C01, E11 = 0.5 * (C11 - 1.0);
        const double sq = ::sqrt(4.0 * pow2(E01) + pow2(E00 - E11));
        limiting = 0.5 * (E00 + E11 + sq) - strain_limit > 0.0;
    }
    const double detC = C00 * C11 - C01 * C01;
    const bool degenerate = !(detC > 0.0);
    double psi = 0.0, dpsi[3] = {0.0, 0.0, 0.0};
    if (!degenerate)
        for (int i = 0; i < 3; i++) {
            const HDual c0(C00, i == 0 ? 1.0 : 0.0, 0.0, 0.0), c1(C01, i == 1 ? 1.0 : 0.0, 0.0, 0.0), c2(C11, i == 2 ? 1.0 : 0.0, 0.0, 0.0);
            const HDual r = tri_density<FULL>(c0, c1, c2, P);
            psi = r.v;
            dpsi[i] = r.a;
        }
    const double J = degenerate ? 0.0 : ::sqrt(detC);
    const double iJ = degenerate ? 0.0 : 1.0 / J;
    // S = 2 dpsi/dC with C01 = C10 one variable of tri_density: S00 = 2 psi_0, S01 = psi_1, S11 = 2 psi_2
    const double S00 = 2.0 * dpsi[0] * iJ, S01 = dpsi[1] * iJ, S11 = 2.0 * dpsi[2] * iJ;
    const V3<double> p0 = S00 * f0 + S01 * f1, p1 = S01 * f0 + S11 * f1;  // (F S) / J
    rec[0] = p0.x * f0.x + p1.x * f1.x;
    rec[1] = p0.y * f0.y + p1.y * f1.y;
    rec[2] = p0.z * f0.z + p1.z * f1.z;
    rec[3] = 0.5 * (p0.x * f0.y + p1.x * f1.y + p0.y * f0.x + p1.y * f1.x);
    rec[4] = 0.5 * (p0.y * f0.z + p1.y * f1.z + p0.z * f0.y + p1.z * f1.y);
    rec[5] = 0.5 * (p0.z * f0.x + p1.z * f1.x + p0.x * f0.z + p1.x * f1.z);
    const double tr = C00 + C11, disc = ::sqrt(4.0 * C01 * C01 + (C00 - C11) * (C00 - C11));
    const double l0 = 0.5 * (tr + disc), l1 = 0.5 * (tr - disc);
    rec[8] = J;
    rec[9] = ::sqrt(::fmax(l0, 0.0));
    rec[10] = ::sqrt(::fmax(l1, 0.0));
    rec[11] = 0.0;
    rec[12] = 0.5 * (l0 - 1.0);
    rec[13] = psi;
    rec[14] = thickness * rest_area;
    stress_finish(rec, limiting, degenerate);
}

// in[]: v1[2] (0..5), x0[2] (6..11), X[2] (12..17), scale, section_radius, youngs_modulus, then FULL: strain_damping, strain_limit,
// strain_limit_stiffness, dt | EO: dt
template <bool FULL>
MS_HD void seg_stress(const double* in, double* rec)
{
    const double scale = in[18], radius = in[19], youngs_modulus = in[20];
    const double damping = FULL ? in[21] : 0.0, strain_limit = FULL ? in[22] : 0.0, sl_k = FULL ? in[23] : 0.0;
    const double dt = in[FULL ? 24 : 21];
    const V3<double> x00(in[6], in[7], in[8]), x01(in[9], in[10], in[11]);
    const V3<double> x10 = x00 + dt * V3<double>(in[0], in[1], in[2]), x11 = x01 + dt * V3<double>(in[3], in[4], in[5]);
    const double l_rest = norm(scale * V3<double>(in[12], in[13], in[14]) - scale * V3<double>(in[15], in[16], in[17]));
    const V3<double> d = x10 - x11;
    const double l = norm(d);
    const double eps = (l - l_rest) * (1.0 / l_rest);
    const double area = M_PI * radius * radius;
    const double volume = area * l_rest;
    // E = V Y eps^2 / 2 + [over > 0] V k over^3 / 3 + dt c ((eps - eps0) / dt)^2 / 2,  N = dE/dl = (dE/deps) / l_rest
    double E = (0.5 * volume * youngs_modulus) * pow2(eps);
    double dE = volume * youngs_modulus * eps;
    bool limiting = false;
    if (FULL) {
        const double over = eps - strain_limit;
        if (over > 0.0) {
            limiting = true;
            E += (volume * sl_k / 3.0) * pow3(over);
            dE += volume * sl_k * pow2(over);
        }
        const double e0 = (norm(x01 - x00) - l_rest) / l_rest;
        E += (0.5 * dt * damping) * pow2((eps - e0) * (1.0 / dt));
        dE += damping * (eps - e0) * (1.0 / dt);
    }
    const bool degenerate = !(l > 0.0);
    const double s = degenerate ? 0.0 : dE / (l_rest * area) / (l * l);  // axial stress / l^2: sigma = s d d^T
    rec[0] = s * d.x * d.x;
    rec[1] = s * d.y * d.y;
    rec[2] = s * d.z * d.z;
    rec[3] = s * d.x * d.y;
    rec[4] = s * d.y * d.z;
    rec[5] = s * d.z * d.x;
    const double stretch = l / l_rest;
    rec[8] = stretch;
    rec[9] = stretch;
    rec[10] = 0.0;
    rec[11] = 0.0;
    rec[12] = 0.5 * (stretch * stretch - 1.0);
    rec[13] = E / volume;
    rec[14] = volume;
    stress_finish(rec, limiting, degenerate);
}

}  // namespace mistark
