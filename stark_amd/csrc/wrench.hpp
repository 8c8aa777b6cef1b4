// wrench.hpp — per-record arithmetic of the rigid-body wrench report (wrench.hip): force and torque on a rigid body from the gradient of any energy
// that sees the body through t1 = t0 + dt v1 and R1 = rb_R1(q0, w1, dt) (energies.hpp). Host and device: compiles with g++ and with hipcc.
//
// rb_R1 normalises q0 + dt/2 (0, w1) q0, which is R1 = C(a) R0 with C the Cayley rotation of a = dt w1 / 2 in the world frame. A variation of w1 rotates
// the body by dtheta = dt / (1 + |a|^2) (dw + a x dw), so the virtual work dE = dE/dw1 . dw = -tau . dtheta gives, with
// (I - [a]x)^-1 = (I + [a]x + a a^T) / (1 + |a|^2),
//     F       = -(1/dt) dE/dv1
//     tau_com = -(1/dt) (I + [a]x + a a^T) dE/dw1          (torque about t1, world frame)
// At w1 = 0 the map is the identity. It is linear: it applies to one element's gradient, to a family's sum or to the whole residual alike.
//
// The report is the torque the solver balances: exact virtual work of the potential as the engine evaluates it. For a potential whose contact-point
// velocity is no pure function of the pose (the lagged friction tables) this need not equal r x f of a force read off the potential's own terms.
#pragma once
#include "hdual.hpp"

namespace mistark {

constexpr int WRENCH_REC = 12;       // doubles per (row, slot)
constexpr int WRENCH_SLOTS = 2;      // bodies per row
constexpr int WRENCH_BODY_REC = 16;  // doubles per (family, body)
constexpr int WRENCH_FLAG_OFF = 1, WRENCH_FLAG_BODIES = 2, WRENCH_FLAG_NONFINITE = 4;

// y = (I + [a]x + a a^T) x
MS_HD void wrench_map(const double a[3], const double x[3], double y[3])
{
    const double d = a[0] * x[0] + a[1] * x[1] + a[2] * x[2];
    y[0] = x[0] + (a[1] * x[2] - a[2] * x[1]) + a[0] * d;
    y[1] = x[1] + (a[2] * x[0] - a[0] * x[2]) + a[1] * d;
    y[2] = x[2] + (a[0] * x[1] - a[1] * x[0]) + a[2] * d;
}

// One slot of a row record from the summed gradient blocks of one body inside one element: gv = dE/dv1, gw = dE/dw1.
//   0..2 F, 3..5 tau_com, 6..8 arm F x tau / |F|^2 (the point of the line of action nearest to the centre of mass, relative to t1), 9 couple along F,
//   10 |F|, 11 |tau_com|; arm and couple are zero where |F| == 0
MS_HD void wrench_slot_record(const double gv[3], const double gw[3], const double w1[3], double dt, double inv_dt, double r[WRENCH_REC])
{
    const double a[3] = {0.5 * dt * w1[0], 0.5 * dt * w1[1], 0.5 * dt * w1[2]};
    const double F[3] = {-inv_dt * gv[0], -inv_dt * gv[1], -inv_dt * gv[2]};
    const double raw[3] = {-inv_dt * gw[0], -inv_dt * gw[1], -inv_dt * gw[2]};
    double tau[3];
    wrench_map(a, raw, tau);
    const double F2 = F[0] * F[0] + F[1] * F[1] + F[2] * F[2];
    const double nF = sqrt(F2), nT = sqrt(tau[0] * tau[0] + tau[1] * tau[1] + tau[2] * tau[2]);
    const bool any = F2 > 0.0;
    const double s = any ? 1.0 / F2 : 0.0;
    r[0] = F[0];
    r[1] = F[1];
    r[2] = F[2];
    r[3] = tau[0];
    r[4] = tau[1];
    r[5] = tau[2];
    r[6] = any ? (F[1] * tau[2] - F[2] * tau[1]) * s : 0.0;
    r[7] = any ? (F[2] * tau[0] - F[0] * tau[2]) * s : 0.0;
    r[8] = any ? (F[0] * tau[1] - F[1] * tau[0]) * s : 0.0;
    r[9] = any ? (tau[0] * F[0] + tau[1] * F[1] + tau[2] * F[2]) / nF : 0.0;
    r[10] = nF;
    r[11] = nT;
}

// The record of one (family, body) from the family's generalised forces fv = -dE/dv1 / dt and fw = -dE/dw1 / dt on the body's two block rows.
//   0..2 F, 3..5 tau_com, 6..8 torque about `about` = tau_com + (t1 - about) x F, 9..11 fw as it came, 12..14 t1, 15 |a|
MS_HD void wrench_body_record(const double fv[3], const double fw[3], const double t0[3], const double v1[3], const double w1[3], double dt, const double about[3],
                              double r[WRENCH_BODY_REC])
{
    const double a[3] = {0.5 * dt * w1[0], 0.5 * dt * w1[1], 0.5 * dt * w1[2]};
    double tau[3];
    wrench_map(a, fw, tau);
    const double t1[3] = {t0[0] + dt * v1[0], t0[1] + dt * v1[1], t0[2] + dt * v1[2]};
    const double d[3] = {t1[0] - about[0], t1[1] - about[1], t1[2] - about[2]};
    r[0] = fv[0];
    r[1] = fv[1];
    r[2] = fv[2];
    r[3] = tau[0];
    r[4] = tau[1];
    r[5] = tau[2];
    r[6] = tau[0] + (d[1] * fv[2] - d[2] * fv[1]);
    r[7] = tau[1] + (d[2] * fv[0] - d[0] * fv[2]);
    r[8] = tau[2] + (d[0] * fv[1] - d[1] * fv[0]);
    r[9] = fw[0];
    r[10] = fw[1];
    r[11] = fw[2];
    r[12] = t1[0];
    r[13] = t1[1];
    r[14] = t1[2];
    r[15] = sqrt(a[0] * a[0] + a[1] * a[1] + a[2] * a[2]);
}

}  // namespace mistark
