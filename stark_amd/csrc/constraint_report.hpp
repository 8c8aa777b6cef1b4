// constraint_report.hpp — constraint report: what one row of a penalty-constraint potential (prescribed positions, the five attachments, the eleven
// rigid-body constraints) reports about itself. Host and device code without device-only intrinsics: tests/host_constraint_report compiles it with g++.
//
// One function per potential takes the gathered inputs in[] of one row in the binding order energies.hpp documents and fills a ConstraintRow; the state is
// the end-of-step state of the current DoFs (x1 = x0 + dt v1, bodies through rb_point / rb_dir, velocities v1, w1). The arithmetic is written from the
// energies of energies.hpp (forces and torques are their derivatives by hand) and from the handlers host/rigid.cpp: measure() restates.
//
// One record of CONSTRAINT_REC = 16 doubles per row:
//   0       violation as the handler defines it: m, deg, m/s or deg/s by potential; signed for distances, distance limits, the damped spring and the two
//           velocity controllers; prescribed positions and attachments: the distance |d| between the two material points
//   1       reaction as the handler defines it (N or N m, the sign convention of measure()); prescribed positions and attachments: k |d|
//   2..4    force on side a in the world frame, -dE/dx of side a's anchor (side a: the first party in the potential's name; the rigid body of rb_d);
//           zero for direction-type rows (global directions, directions, angle limits, angular velocity)
//   5..7    torque on side a about its centre of mass at x1: (anchor_a - t1_a) x f for a rigid side a of a point-type row, -d_a x dE/dd_a for a
//           direction-type row, the controller's torque along the axis for the angular velocity controller; zero when side a is deformable and for
//           the linear velocity controller (its force acts on the centre of mass)
//   8..10   anchor of side a at x1 (point-type), unit direction of side a (direction-type), the axis of body a (velocity controllers)
//   11..13  anchor or direction of side b, or the global target; velocity controllers: the relative velocity v_b - v_a (w_b - w_a)
//   14      energy of the row exactly as the potential evaluates it (En::energy)
//   15      flags as a double: +1 active (is_active > 0.5 where the potential has the input and, for the limit kinds, the limit engaged),
//           +2 |violation| > the tolerance of the row's group (never without a tolerance), +4 out of range (a damped spring with coincident ends reports
//           a damper value of 0; a direction difference C > 1 reports 90 deg where asin would be NaN)
//   inactive rows report their geometry (0, 8..13) and zeros in 1..7 and 14
//   aux[2]  the damped spring's damper: relative velocity of the ends along the axis (m/s) and -damping * that (N); zeros for every other kind
// One record of CONSTRAINT_GROUP_REC = 12 doubles per group (constraint_report.hip sums it):
//   0 rows, 1 active rows, 2 rows beyond tolerance, 3 largest |violation|, 4 position in the group's list of the first row attaining it (-1: no row),
//   5..7 sum of 2..4, 8..10 moment about `about`: sum of (anchor_a - about) x f, direction-type kinds: sum of 5..7 (the linear velocity controller, whose
//   potential reads no anchor, counts as one: its force enters 5..7 and not the moment), 11 energy sum
#pragma once
#include "energies.hpp"

namespace mistark {

constexpr int CONSTRAINT_REC = 16;
constexpr int CONSTRAINT_GROUP_REC = 12;
constexpr int CONSTRAINT_KINDS = 17;

struct ConstraintRow
{
    double viol = 0.0, react = 0.0;
    V3<double> f = V3<double>(0.0, 0.0, 0.0), tau = V3<double>(0.0, 0.0, 0.0), pa = V3<double>(0.0, 0.0, 0.0), pb = V3<double>(0.0, 0.0, 0.0);
    bool active = true, out_of_range = false;
    double aux0 = 0.0, aux1 = 0.0;
};

// Properties of the potentials, by kind code (registry order of the seventeen): the connectivity column the row reads its stiffness with (its group),
// the local DoF blocks that are the first block of side a and of side b (-1: none), whether the row is direction-type (its moment is 5..7), the unit
// of slot 0 (0 m, 1 deg, 2 m/s, 3 deg/s).
template <class En>
struct ConstraintKind;
#define MISTARK_CONSTRAINT_KIND(En, CODE, GCOL, BA, BB, DIR, UNIT) \
    template <>                                                    \
    struct ConstraintKind<En>                                      \
    {                                                              \
        static constexpr int code = CODE, group_col = GCOL, block_a = BA, block_b = BB, unit = UNIT; \
        static constexpr bool dir_type = DIR;                      \
    };
MISTARK_CONSTRAINT_KIND(E_PrescribedPositions, 0, 2, 0, -1, false, 0)
MISTARK_CONSTRAINT_KIND(E_RBGlobalPoints, 1, 0, 0, -1, false, 0)
MISTARK_CONSTRAINT_KIND(E_RBGlobalDirections, 2, 0, 0, -1, true, 1)
MISTARK_CONSTRAINT_KIND(E_RBPoints, 3, 0, 0, 1, false, 0)
MISTARK_CONSTRAINT_KIND(E_RBPointOnAxis, 4, 0, 0, 1, false, 0)
MISTARK_CONSTRAINT_KIND(E_RBDistances, 5, 0, 0, 1, false, 0)
MISTARK_CONSTRAINT_KIND(E_RBDistanceLimits, 6, 0, 0, 1, false, 0)
MISTARK_CONSTRAINT_KIND(E_RBDirections, 7, 0, 0, 1, true, 1)
MISTARK_CONSTRAINT_KIND(E_RBAngleLimits, 8, 0, 0, 1, true, 1)
MISTARK_CONSTRAINT_KIND(E_RBDampedSpring, 9, 0, 0, 1, false, 0)
MISTARK_CONSTRAINT_KIND(E_RBLinearVelocity, 10, 0, 0, 1, true, 2)
MISTARK_CONSTRAINT_KIND(E_RBAngularVelocity, 11, 0, 0, 1, true, 3)
MISTARK_CONSTRAINT_KIND(E_AttachPP, 12, 0, 0, 1, false, 0)
MISTARK_CONSTRAINT_KIND(E_AttachPE, 13, 1, 0, 1, false, 0)
MISTARK_CONSTRAINT_KIND(E_AttachPT, 14, 1, 0, 1, false, 0)
MISTARK_CONSTRAINT_KIND(E_AttachEE, 15, 1, 0, 2, false, 0)
MISTARK_CONSTRAINT_KIND(E_AttachRBD, 16, 1, 1, 0, false, 0)
#undef MISTARK_CONSTRAINT_KIND
#define MISTARK_FOR_EACH_CONSTRAINT(X) \
    X(E_PrescribedPositions)           \
    X(E_RBGlobalPoints)                \
    X(E_RBGlobalDirections)            \
    X(E_RBPoints)                      \
    X(E_RBPointOnAxis)                 \
    X(E_RBDistances)                   \
    X(E_RBDistanceLimits)              \
    X(E_RBDirections)                  \
    X(E_RBAngleLimits)                 \
    X(E_RBDampedSpring)                \
    X(E_RBLinearVelocity)              \
    X(E_RBAngularVelocity)             \
    X(E_AttachPP)                      \
    X(E_AttachPE)                      \
    X(E_AttachPT)                      \
    X(E_AttachEE)                      \
    X(E_AttachRBD)

MS_HD double cr_rad2deg(double x) { return x * (180.0 / M_PI); }
constexpr double CR_EPS = 100.0 * 2.220446049250313e-16;  // the handlers' guard against a zero direction difference
MS_HD V3<double> cr_x1(const double* in, int ov, int ox, double dt) { return V3<double>(in[ox] + dt * in[ov], in[ox + 1] + dt * in[ov + 1], in[ox + 2] + dt * in[ov + 2]); }
// body block {v1, w1, t0, q0_} at offset o
MS_HD V3<double> cr_body_point(const double* in, int o, const V3<double>& loc, double dt) { return rb_point(Loader<double>{in}, o, 0, 0, loc, dt); }
MS_HD V3<double> cr_body_t1(const double* in, int o, double dt) { return cr_x1(in, o, o + 6, dt); }
MS_HD V3<double> cr_body_dir(const double* in, int ow, int oq, const V3<double>& loc, double dt) { return rb_dir(Loader<double>{in}, ow, oq, 0, loc, dt); }
MS_HD V3<double> cr_v(const double* in, int o) { return V3<double>(in[o], in[o + 1], in[o + 2]); }
// violation of a direction difference of length C in degrees
MS_HD double cr_direction_deg(double C, bool& out_of_range)
{
    if (C > 1.0) {
        out_of_range = true;
        return 90.0;
    }
    return cr_rad2deg(::asin(C));
}

// a spring k/2 |b - a|^2 between two material points (prescribed positions, the attachments, global points, points)
MS_HD void cr_point_spring(ConstraintRow& r, const V3<double>& a, const V3<double>& b, double k)
{
    const V3<double> d = b - a;
    r.viol = norm(d);
    r.react = k * r.viol;
    r.f = k * d;
    r.pa = a;
    r.pb = b;
}

template <class En>
MS_HD ConstraintRow constraint_row(const double* in);

template <>
MS_HD ConstraintRow constraint_row<E_PrescribedPositions>(const double* in)
{
    ConstraintRow r;
    cr_point_spring(r, cr_x1(in, 0, 3, in[10]), cr_v(in, 6), in[9]);
    return r;
}
template <>
MS_HD ConstraintRow constraint_row<E_AttachPP>(const double* in)
{
    ConstraintRow r;
    const double dt = in[13];
    cr_point_spring(r, cr_x1(in, 0, 6, dt), cr_x1(in, 3, 9, dt), in[12]);
    return r;
}
template <>
MS_HD ConstraintRow constraint_row<E_AttachPE>(const double* in)
{
    ConstraintRow r;
    const double dt = in[21];
    cr_point_spring(r, cr_x1(in, 0, 9, dt), in[18] * cr_x1(in, 3, 12, dt) + in[19] * cr_x1(in, 6, 15, dt), in[20]);
    return r;
}
template <>
MS_HD ConstraintRow constraint_row<E_AttachPT>(const double* in)
{
    ConstraintRow r;
    const double dt = in[28];
    cr_point_spring(r, cr_x1(in, 0, 12, dt), in[24] * cr_x1(in, 3, 15, dt) + in[25] * cr_x1(in, 6, 18, dt) + in[26] * cr_x1(in, 9, 21, dt), in[27]);
    return r;
}
template <>
MS_HD ConstraintRow constraint_row<E_AttachEE>(const double* in)
{
    ConstraintRow r;
    const double dt = in[29];
    cr_point_spring(r, in[24] * cr_x1(in, 0, 12, dt) + in[25] * cr_x1(in, 3, 15, dt), in[26] * cr_x1(in, 6, 18, dt) + in[27] * cr_x1(in, 9, 21, dt), in[28]);
    return r;
}
template <>
MS_HD ConstraintRow constraint_row<E_AttachRBD>(const double* in)
{
    ConstraintRow r;
    const double dt = in[1];
    const V3<double> a = cr_body_point(in, 11, cr_v(in, 8), dt);
    cr_point_spring(r, a, cr_x1(in, 2, 5, dt), in[0]);
    r.tau = cross(a - cr_body_t1(in, 11, dt), r.f);
    return r;
}
template <>
MS_HD ConstraintRow constraint_row<E_RBGlobalPoints>(const double* in)
{
    ConstraintRow r;
    const double dt = in[8];
    const V3<double> a = cr_body_point(in, 9, cr_v(in, 0), dt);
    cr_point_spring(r, a, cr_v(in, 3), in[6]);
    r.tau = cross(a - cr_body_t1(in, 9, dt), r.f);
    r.active = in[7] > 0.5;
    return r;
}
template <>
MS_HD ConstraintRow constraint_row<E_RBPoints>(const double* in)
{
    ConstraintRow r;
    const double dt = in[8];
    const V3<double> a = cr_body_point(in, 9, cr_v(in, 0), dt);
    cr_point_spring(r, a, cr_body_point(in, 22, cr_v(in, 3), dt), in[6]);
    r.tau = cross(a - cr_body_t1(in, 9, dt), r.f);
    r.active = in[7] > 0.5;
    return r;
}
template <>
MS_HD ConstraintRow constraint_row<E_RBPointOnAxis>(const double* in)
{
    ConstraintRow r;
    const double k = in[9], dt = in[11];
    const V3<double> a = cr_body_point(in, 12, cr_v(in, 0), dt), da = cr_body_dir(in, 15, 21, cr_v(in, 3), dt), b = cr_body_point(in, 25, cr_v(in, 6), dt);
    // E = k/2 |n|^2, n the part of b - a across the axis: dE/da = -k n with the axis held
    const V3<double> ap = b - a;
    const double s = dot(ap, da) / dot(da, da);
    const V3<double> n = ap - s * da;
    r.viol = ::sqrt(sq_distance_point_line(b, a, a + da));
    r.react = k * r.viol;
    r.f = k * n;
    r.tau = cross(a - cr_body_t1(in, 12, dt), r.f);
    r.pa = a;
    r.pb = b;
    r.active = in[10] > 0.5;
    return r;
}
// a spring along the line of two anchors whose signed extension is C: E = k/2 C^2, f_a = k C u, u the unit vector from a to b
MS_HD void cr_axial(ConstraintRow& r, const V3<double>& a, const V3<double>& b, double length, double C, double k, const V3<double>& t1_a)
{
    const V3<double> d = b - a;
    const double s = length > 0.0 ? k * C / length : 0.0;
    r.viol = C;
    r.react = -k * C;
    r.f = s * d;
    r.tau = cross(a - t1_a, r.f);
    r.pa = a;
    r.pb = b;
}
template <>
MS_HD ConstraintRow constraint_row<E_RBDistances>(const double* in)
{
    ConstraintRow r;
    const double dt = in[9];
    const V3<double> a = cr_body_point(in, 10, cr_v(in, 0), dt), b = cr_body_point(in, 23, cr_v(in, 3), dt);
    const double l = norm(b - a);
    cr_axial(r, a, b, l, l - in[6], in[7], cr_body_t1(in, 10, dt));
    r.active = in[8] > 0.5;
    return r;
}
template <>
MS_HD ConstraintRow constraint_row<E_RBDistanceLimits>(const double* in)
{
    ConstraintRow r;
    const double dmin = in[6], dmax = in[7], dt = in[10];
    const V3<double> a = cr_body_point(in, 11, cr_v(in, 0), dt), b = cr_body_point(in, 24, cr_v(in, 3), dt);
    const double l = norm(b - a);
    const double C = l < dmin ? l - dmin : (l > dmax ? l - dmax : 0.0);
    cr_axial(r, a, b, l, C, in[8], cr_body_t1(in, 11, dt));
    r.active = in[9] > 0.5 && (l < dmin || l > dmax);
    return r;
}
template <>
MS_HD ConstraintRow constraint_row<E_RBDampedSpring>(const double* in)
{
    ConstraintRow r;
    const double rest = in[6], k = in[7], damping = in[8], dt = in[10];
    const V3<double> la = cr_v(in, 0), lb = cr_v(in, 3);
    const V3<double> a = cr_body_point(in, 11, la, dt), b = cr_body_point(in, 24, lb, dt), ta = cr_body_t1(in, 11, dt), tb = cr_body_t1(in, 24, dt);
    const double l1 = norm(b - a), l0 = norm(rb_point0(in, 24, lb) - rb_point0(in, 11, la));
    cr_axial(r, a, b, l1, l1 - rest, k, ta);
    r.active = in[9] > 0.5;
    if (l1 > 0.0) {
        const V3<double> u = (1.0 / l1) * (b - a);
        // the damper of the energy, damping/2 ((l1 - l0) / dt)^2, pulls a along the axis with damping (l1 - l0) / dt^2
        const V3<double> fd = (damping * (l1 - l0) / (dt * dt)) * u;
        r.f = r.f + fd;
        r.tau = r.tau + cross(a - ta, fd);
        // the handler's damper: velocity of b relative to a along the axis, v = v1 + w1 x (x1 - t1)
        const V3<double> va = cr_v(in, 11) + cross(cr_v(in, 14), a - ta), vb = cr_v(in, 24) + cross(cr_v(in, 27), b - tb);
        r.aux0 = dot(vb - va, u);
        r.aux1 = -damping * r.aux0;
    } else {
        r.out_of_range = true;
    }
    return r;
}
template <>
MS_HD ConstraintRow constraint_row<E_RBGlobalDirections>(const double* in)
{
    ConstraintRow r;
    const double k = in[6], dt = in[8];
    const V3<double> d = cr_body_dir(in, 9, 12, cr_v(in, 0), dt), target = cr_v(in, 3);
    const V3<double> u = d - target;
    const double C = norm(u);
    r.viol = cr_direction_deg(C, r.out_of_range);
    r.react = norm(cross(target, (-k * C / (C + CR_EPS)) * u));
    r.tau = -cross(d, k * u);  // dE/dd = k (d - target)
    r.pa = d;
    r.pb = target;
    r.active = in[7] > 0.5;
    return r;
}
template <>
MS_HD ConstraintRow constraint_row<E_RBDirections>(const double* in)
{
    ConstraintRow r;
    const double k = in[6], dt = in[8];
    const V3<double> da = cr_body_dir(in, 9, 12, cr_v(in, 0), dt), db = cr_body_dir(in, 16, 19, cr_v(in, 3), dt);
    const V3<double> u = db - da;
    const double C = norm(u);
    r.viol = cr_direction_deg(C, r.out_of_range);
    r.react = norm(cross(da, (k * C / (C + CR_EPS)) * u));
    r.tau = cross(da, k * u);  // dE/dda = -k (db - da)
    r.pa = da;
    r.pb = db;
    r.active = in[7] > 0.5;
    return r;
}
template <>
MS_HD ConstraintRow constraint_row<E_RBAngleLimits>(const double* in)
{
    ConstraintRow r;
    const double maxd = in[6], k = in[7], dt = in[9];
    const V3<double> da = cr_body_dir(in, 10, 13, cr_v(in, 0), dt), db = cr_body_dir(in, 17, 20, cr_v(in, 3), dt);
    const V3<double> u = db - da;
    const double d = norm(u);
    const bool engaged = d > maxd;
    if (engaged) {
        const double C = d - maxd;
        r.viol = cr_rad2deg(::acos((2.0 - C * C) / 2.0));  // angle of an opening distance
        r.react = norm(cross(da, (k * C * C / (d + CR_EPS)) * u));
        r.tau = cross(da, (k * C * C / d) * u);  // E = k/3 C^3: dE/dda = -k C^2 u / d
    }
    r.pa = da;
    r.pb = db;
    r.active = in[8] > 0.5 && engaged;
    return r;
}
// the C1 controller on dv = axis . (vb - va) - target: its reaction as the handler reports it, and s = (dE/ddv) / dt, the strength with which it pushes
// side a along the axis
MS_HD void cr_controller(double dv, double max_force, double delay, double& react, double& s)
{
    if (dv < -delay) react = -max_force, s = -max_force;
    else if (dv < delay) react = -(max_force / delay) * dv, s = (max_force / delay) * dv;
    else react = max_force, s = max_force;
}
template <>
MS_HD ConstraintRow constraint_row<E_RBLinearVelocity>(const double* in)
{
    ConstraintRow r;
    const V3<double> da = cr_body_dir(in, 13, 16, cr_v(in, 0), in[20]);
    const V3<double> rel = cr_v(in, 10) - cr_v(in, 7);
    double s;
    r.viol = dot(da, rel) - in[3];
    cr_controller(r.viol, in[4], in[5], r.react, s);
    r.f = s * da;
    r.pa = da;
    r.pb = rel;
    r.active = in[6] > 0.5;
    return r;
}
template <>
MS_HD ConstraintRow constraint_row<E_RBAngularVelocity>(const double* in)
{
    ConstraintRow r;
    const V3<double> da = cr_body_dir(in, 7, 13, cr_v(in, 0), in[17]);
    const V3<double> rel = cr_v(in, 10) - cr_v(in, 7);
    const double dv = dot(da, rel) - in[3];
    double s;
    cr_controller(dv, in[4], in[5], r.react, s);
    r.viol = cr_rad2deg(dv);
    r.tau = s * da;
    r.pa = da;
    r.pb = rel;
    r.active = in[6] > 0.5;
    return r;
}

// the record of one row; tolerance < 0: none
template <class En>
MS_HD void constraint_record(const double* in, double tolerance, double* rec, double* aux)
{
    ConstraintRow r = constraint_row<En>(in);
    const bool on = r.active;
    rec[0] = r.viol;
    rec[1] = on ? r.react : 0.0;
    rec[2] = on ? r.f.x : 0.0; rec[3] = on ? r.f.y : 0.0; rec[4] = on ? r.f.z : 0.0;
    rec[5] = on ? r.tau.x : 0.0; rec[6] = on ? r.tau.y : 0.0; rec[7] = on ? r.tau.z : 0.0;
    rec[8] = r.pa.x; rec[9] = r.pa.y; rec[10] = r.pa.z;
    rec[11] = r.pb.x; rec[12] = r.pb.y; rec[13] = r.pb.z;
    rec[14] = r.active ? En::energy(Loader<double>{in}) : 0.0;
    rec[15] = (on ? 1.0 : 0.0) + (tolerance >= 0.0 && ::fabs(r.viol) > tolerance ? 2.0 : 0.0) + (r.out_of_range ? 4.0 : 0.0);
    aux[0] = r.aux0;
    aux[1] = r.aux1;
}

}  // namespace mistark
