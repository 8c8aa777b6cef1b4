// budget.hpp — energy and momentum budget readout: what one item (a lumped point mass, a rigid body) adds to the record of its object. Host and
// device code without device-only intrinsics: tests/host_budget compiles it with g++.
//
// One record of BUDGET_REC = 13 doubles per object (an inertia group or a rigid body), at the end-of-step state of the current DoFs:
//   0       mass                        sum m
//   1..3    first moment                sum m x            (centre of mass = first moment / mass)
//   4..6    linear momentum             sum m v
//   7..9    angular momentum            sum (x - about) x (m v)    (+ J1 w1 for a rigid body)
//   10      kinetic energy              0.5 sum m v.v              (+ 0.5 w1.J1 w1)
//   11      gravitational energy        -sum m gravity.x
//   12      item count
//   point   m = lumped volume * density, x = x0 + dt v1, v = v1    (the mass rule and end-of-step position of EnergyLumpedInertia)
//   body    x = t1 = t0 + dt v1, v = v1, J1 = R(q1) J_loc R(q1)^T, q1 = normalize(q0 + dt/2 (0, w1) q0): rb_R1, the update every rigid-body
//           potential and the contact detector's vertices use
// A BudgetAcc holds the 13 sums in named scalars: nothing here is indexed at run time, so the accumulators stay in registers.
#pragma once
#include "energies.hpp"

namespace mistark {

constexpr int BUDGET_REC = 13;

struct BudgetAcc
{
    double m = 0.0, mx = 0.0, my = 0.0, mz = 0.0, px = 0.0, py = 0.0, pz = 0.0, lx = 0.0, ly = 0.0, lz = 0.0, T = 0.0, U = 0.0, n = 0.0;
};

// a point mass m at x with velocity v; `about` is the reference point of the angular momentum
MS_HD void budget_add_point(BudgetAcc& a, double m, const V3<double>& x, const V3<double>& v, const V3<double>& about, const V3<double>& gravity)
{
    const double px = m * v.x, py = m * v.y, pz = m * v.z;
    const double rx = x.x - about.x, ry = x.y - about.y, rz = x.z - about.z;
    a.m += m;
    a.mx += m * x.x;
    a.my += m * x.y;
    a.mz += m * x.z;
    a.px += px;
    a.py += py;
    a.pz += pz;
    a.lx += ry * pz - rz * py;
    a.ly += rz * px - rx * pz;
    a.lz += rx * py - ry * px;
    a.T += 0.5 * (px * v.x + py * v.y + pz * v.z);
    a.U -= m * (gravity.x * x.x + gravity.y * x.y + gravity.z * x.z);
    a.n += 1.0;
}

// in[]: the gathered inputs of one element of EnergyLumpedInertia in binding order (E_LumpedInertia::Layout)
MS_HD void budget_add_inertia_item(BudgetAcc& a, const double* in, const V3<double>& about)
{
    const V3<double> v1(in[0], in[1], in[2]), x0(in[3], in[4], in[5]), gravity(in[20], in[21], in[22]);
    const double volume = in[15], density = in[16], dt = in[19];
    const V3<double> x(x0.x + dt * v1.x, x0.y + dt * v1.y, x0.z + dt * v1.z);
    budget_add_point(a, volume * density, x, v1, about, gravity);
}

// one rigid body; J_loc row-major 3 x 3 in the body frame
MS_HD void budget_add_body(BudgetAcc& a, const double* t0, const double* q0, const double* v1, const double* w1, double mass, const double* J_loc, double dt, const V3<double>& about,
                           const V3<double>& gravity)
{
    const V3<double> v(v1[0], v1[1], v1[2]), w(w1[0], w1[1], w1[2]);
    const V3<double> t1(t0[0] + dt * v.x, t0[1] + dt * v.y, t0[2] + dt * v.z);
    const M3<double> R = rb_R1(q0, w, dt);
    // J1 w = R (J_loc (R^T w))
    const V3<double> wl(R.m[0][0] * w.x + R.m[1][0] * w.y + R.m[2][0] * w.z, R.m[0][1] * w.x + R.m[1][1] * w.y + R.m[2][1] * w.z, R.m[0][2] * w.x + R.m[1][2] * w.y + R.m[2][2] * w.z);
    const V3<double> jl(J_loc[0] * wl.x + J_loc[1] * wl.y + J_loc[2] * wl.z, J_loc[3] * wl.x + J_loc[4] * wl.y + J_loc[5] * wl.z, J_loc[6] * wl.x + J_loc[7] * wl.y + J_loc[8] * wl.z);
    const V3<double> Jw = R * jl;
    budget_add_point(a, mass, t1, v, about, gravity);
    a.lx += Jw.x;
    a.ly += Jw.y;
    a.lz += Jw.z;
    a.T += 0.5 * (w.x * Jw.x + w.y * Jw.y + w.z * Jw.z);
}

MS_HD void budget_store(const BudgetAcc& a, double* rec)
{
    rec[0] = a.m;
    rec[1] = a.mx; rec[2] = a.my; rec[3] = a.mz;
    rec[4] = a.px; rec[5] = a.py; rec[6] = a.pz;
    rec[7] = a.lx; rec[8] = a.ly; rec[9] = a.lz;
    rec[10] = a.T;
    rec[11] = a.U;
    rec[12] = a.n;
}

}  // namespace mistark
