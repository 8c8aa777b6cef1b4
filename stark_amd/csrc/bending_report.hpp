// bending_report.hpp — bending report of the two cloth bending potentials: what their evaluation computes on the way to the gradient and throws away.
//   EnergyDiscreteShells  (energies.hpp, "complete")  shells_bending_record
//   EnergyBendingFlat     (energies.hpp, "flat")      flat_bending_record
// in[]: the gathered inputs of one hinge in the reference's binding order, the same array the evaluation kernels read:
//   complete  v1[4] x0[4] rest angle, rest length, rest height, scale, k, damping, dt     (31)
//   flat      v1[4] x0[4] K[4] coef, k, dt                                                (31)
// Local nodes 0 and 1 are the hinge edge, 2 and 3 the opposite vertices. The state is the end-of-step state x1 = x0 + dt v1. Host and device code:
// tests/host_bending_report compiles it with g++.
//
// One record of BEND_REC = 16 doubles, the same for both kinds:
//   0      theta1: the angle exactly as the potential's dihedral_angle() computes it at x1, acos((1 - 1e-12) n0_hat . n1_hat): in [1.41e-6, pi], blind to
//          the fold direction
//   1      phi1: signed fold angle atan2(e0_hat . (n0_hat x n1_hat), n0_hat . n1_hat), well conditioned near flat; its sign is the fold direction
//          (+pi and -pi are the same fold)
//   2      rest angle (complete: the bound rest_dihedral_angle; flat: 0)
//   3      angle rate (theta1 - theta0) / dt, theta0 the same function at x0 (0 where the stencil at x0 has no normals)
//   4      current hinge length |x1[1] - x1[0]|
//   5      rest hinge area a = (A0 + A1) / 3 from the potential's own data: complete scale^2 rest_len rest_height; flat 1 / (2 coef)
//   6      normal curvature across the hinge kappa: complete theta1 / (3 scale rest_height); flat |s| / (3 a), s = sum_i K_i x1_i. Under a rigid fold the two
//          agree to O(theta^2); on a mesh inscribed in a cylinder of radius R both tend to 1 / R
//   7      rest curvature: complete rest_angle / (3 scale rest_height); flat 0
//   8      bending moment M [J/rad]. complete: dE/dtheta1 = ratio (2 k (theta1 - rest) + (damping / dt) (theta1 - theta0)), ratio as the potential forms
//          it. flat: k coef |s| l1 cos(theta1 / 2), which is dE/dtheta for a fold that leaves both triangles rigid (|s| = 2 l sin(theta / 2) there, so
//          M = k l sin(theta) / (2 h_e): for one stiffness a quarter of the complete model's 2 k theta l / h_e at small angles)
//   9      elastic energy: complete k (theta1 - rest)^2 ratio; flat the whole element energy (k coef / 2) |s|^2
//   10     damping energy: complete (damping / dt) (theta1^2 / 2 - theta0 theta1) ratio, as the potential writes it; flat 0. 9 + 10 = the element energy
//   11..13 unit hinge normal (n0_hat + n1_hat) / |n0_hat + n1_hat|; zeros for a hinge folded onto itself (|n0_hat + n1_hat| < 1e-8: no direction is left)
//   14     group: the connectivity entry the row reads its stiffness with (filled in by the caller, who holds the connectivity)
//   15     flags as a double: +1 degenerate, +2 |theta1 - rest| beyond the threshold of the row's group
// A hinge is degenerate when a triangle of its stencil has zero area at x1 or the hinge has zero length. It sets flag 1, never flag 2, and writes zeros into
// every field that needs a normal: 0, 1, 3, 8, 11..13, and for the complete kind 6, 9 and 10 as well.
#pragma once
#include "energies.hpp"

namespace mistark {

constexpr int BEND_REC = 16;
constexpr int BEND_NODAL = 6;   // nodal record: weighted mean kappa, weighted mean kappa - kappa_rest, energy share, largest |theta1 - rest|, hinges, weight sum
constexpr int BEND_GROUP = 10;  // group record: hinges, degenerate, beyond threshold, largest |theta1 - rest|, where, sums of 9, 10, a, a (kappa - kappa_rest)^2, mean |kappa - kappa_rest|
constexpr double BEND_NO_NORMAL = 1e-8;

// the stencil of one hinge at one state
struct BendStencil
{
    V3<double> e0, n0, n1;  // hinge edge, the two (unnormalised) triangle normals as dihedral_angle() forms them
    double l, nn0, nn1;
    bool degenerate;
};
MS_HD BendStencil bend_stencil(const V3<double>* x)
{
    BendStencil s;
    s.e0 = x[1] - x[0];
    s.n0 = cross(s.e0, x[2] - x[0]);
    s.n1 = -cross(s.e0, x[3] - x[0]);
    s.l = norm(s.e0);
    s.nn0 = norm(s.n0);
    s.nn1 = norm(s.n1);
    s.degenerate = !(s.l > 0.0 && s.nn0 > 0.0 && s.nn1 > 0.0);
    return s;
}
// x0 and x1 of the four nodes from the first 24 inputs
MS_HD void bend_states(const double* in, double dt, V3<double>* x0, V3<double>* x1)
{
    for (int i = 0; i < 4; i++) {
        x0[i] = V3<double>(in[12 + 3 * i], in[13 + 3 * i], in[14 + 3 * i]);
        x1[i] = x0[i] + dt * V3<double>(in[3 * i], in[3 * i + 1], in[3 * i + 2]);
    }
}
// fields 0, 1, 3, 4, 11..13 and the degenerate flag: what both kinds share. Returns theta0 (0 where x0 has no normals) through t0.
MS_HD bool bend_angles(const V3<double>* x0, const V3<double>* x1, double dt, double* r, double& t0)
{
    const BendStencil s1 = bend_stencil(x1), s0 = bend_stencil(x0);
    r[4] = s1.l;
    r[0] = r[1] = r[3] = r[11] = r[12] = r[13] = 0.0;
    t0 = 0.0;
    if (s1.degenerate) return true;
    r[0] = dihedral_angle(x1);
    const V3<double> h0 = (1.0 / s1.nn0) * s1.n0, h1 = (1.0 / s1.nn1) * s1.n1, eh = (1.0 / s1.l) * s1.e0;
    r[1] = ::atan2(dot(eh, cross(h0, h1)), dot(h0, h1));
    if (!s0.degenerate) {
        t0 = dihedral_angle(x0);
        r[3] = (r[0] - t0) / dt;
    }
    const V3<double> m = h0 + h1;
    const double nm = norm(m);
    if (nm >= BEND_NO_NORMAL) {
        r[11] = m.x / nm;
        r[12] = m.y / nm;
        r[13] = m.z / nm;
    }
    return false;
}
// flags from the degenerate state and the threshold of the row's group (negative: none)
MS_HD double bend_flags(bool degenerate, double theta1, double rest, double threshold)
{
    if (degenerate) return 1.0;
    return threshold >= 0.0 && ::fabs(theta1 - rest) > threshold ? 2.0 : 0.0;
}

// EnergyDiscreteShells. r[14] is left to the caller.
MS_HD void shells_bending_record(const double* in, double threshold, double* r)
{
    const double rest = in[24], rest_len = in[25], rest_h = in[26], scale = in[27], k = in[28], damping = in[29], dt = in[30];
    V3<double> x0[4], x1[4];
    bend_states(in, dt, x0, x1);
    double t0;
    const bool deg = bend_angles(x0, x1, dt, r, t0);
    const double ratio = (rest_len * scale) / (rest_h * scale);
    const double t1 = r[0], dd = t1 - rest;
    r[2] = rest;
    r[5] = scale * scale * rest_len * rest_h;
    r[7] = rest / (3.0 * scale * rest_h);
    if (deg) {
        r[6] = r[8] = r[9] = r[10] = 0.0;
    } else {
        r[6] = t1 / (3.0 * scale * rest_h);
        r[8] = ratio * (2.0 * k * dd + (damping / dt) * (t1 - t0));
        r[9] = k * (dd * dd) * ratio;
        r[10] = (damping / dt) * (0.5 * pow2(t1) - t0 * t1) * ratio;
    }
    r[15] = bend_flags(deg, t1, rest, threshold);
}

// EnergyBendingFlat. r[14] is left to the caller.
MS_HD void flat_bending_record(const double* in, double threshold, double* r)
{
    const double coef = in[28], k = in[29], dt = in[30];
    V3<double> x0[4], x1[4];
    bend_states(in, dt, x0, x1);
    double t0;
    const bool deg = bend_angles(x0, x1, dt, r, t0);
    V3<double> s(0.0, 0.0, 0.0);
    for (int i = 0; i < 4; i++) s = s + in[24 + i] * x1[i];
    const double ss = sqnorm(s), ns = ::sqrt(ss);
    r[2] = 0.0;
    r[5] = 1.0 / (2.0 * coef);
    r[6] = ns / (3.0 * r[5]);
    r[7] = 0.0;
    r[8] = deg ? 0.0 : k * coef * ns * r[4] * ::cos(0.5 * r[0]);
    r[9] = (0.5 * k * coef) * ss;
    r[10] = 0.0;
    r[15] = bend_flags(deg, r[0], 0.0, threshold);
}

// |theta1 - rest| of a stored record for the maxima of the nodal and group stages: 0 for a degenerate hinge
MS_HD double bend_deviation(double theta1, double rest, double flags) { return ((int)flags & 1) ? 0.0 : ::fabs(theta1 - rest); }

}  // namespace mistark
