// ccd_pad.hpp — the deviation bound of the curved rigid-body CCD (contact.hip, k_ccd_vertices_curved). Host and device code without device-only
// intrinsics: tests/host_ccd_pad compiles it with g++.
//
// A vertex of a rigid body at body-frame position x_loc moves, along the fraction t of a Newton direction (dv, dw), on
//     p(t) = t0 + dt (v + t dv) + R(n(t)) x_loc,   n = q / |q|,   q(t) = q0 + (dt / 2) (0, w + t dw) q0     (rb_R1, energies.hpp).
// q is affine in t and (0, w) q0 is orthogonal to q0, so |q(t)| >= |q0| and beta = |q'| / |q| <= dt |dw| / 2. With |n'| <= beta, |n''| <= 6 beta^2 and
// f = n x_loc conj(n): |f''| <= (2 * 6 + 2) beta^2 r, r = |x_loc|. Linear interpolation over [0, tau] is off by at most tau^2 / 8 max |f''|, the translation is
// affine, hence
//     | p(t) - chord over [0, tau] (t) |  <=  delta(tau) = min( (7 / 16) r (phi tau)^2, 2 r ),   phi = dt |dw|
// (2 r: both lie in the ball of radius r about the moving centre). Written so that halving tau quarters the result exactly where the cap is inactive
// (a power of two scales phi tau and its square without rounding) and so that phi == 0 gives +0.0.
#pragma once
#include "energies.hpp"

namespace mistark {

constexpr double CCD_PAD_CONSTANT = 0.4375;  // 7 / 16

// phi of one body: dt |dw|
MS_HD double ccd_pad_phi(double dt, double dwx, double dwy, double dwz) { return dt * ::sqrt(dwx * dwx + dwy * dwy + dwz * dwz); }

// delta(tau) of a vertex at arm r
MS_HD double ccd_pad_delta(double r, double phi, double tau)
{
    const double a = phi * tau;
    const double bound = (CCD_PAD_CONSTANT * r) * (a * a);
    const double cap = 2.0 * r;
    return bound < cap ? bound : cap;
}

// ... from the body-frame position itself
MS_HD double ccd_pad_vertex(const double* x_loc, double phi, double tau)
{
    return ccd_pad_delta(::sqrt(x_loc[0] * x_loc[0] + x_loc[1] * x_loc[1] + x_loc[2] * x_loc[2]), phi, tau);
}

}  // namespace mistark
