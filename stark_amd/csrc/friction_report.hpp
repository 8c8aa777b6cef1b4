// friction_report.hpp — arithmetic of the friction report, host/device: one row record per installed friction-table row.
//
// Everything is as the table's potential evaluates it (oracle/energies.py:_friction, EnergyFrictionalContact.cpp:1260-1278): the lagged T, mu, fn and bary
// of the table, the velocities of the current DoFs; nothing is classified or recomputed from positions. The roles follow the potential: B is the side
// whose contact-point velocity it takes positive, A the side it subtracts, v = v_B - v_A. That is the detected (A, B) of the search, except in the rows of
// friction_rb_d_pp and friction_rb_d_ee whose detected A is the deformable side: the reference lists the rigid side first there AND evaluates
// v = v_deformable - v_rigid (for edge-edge rows with bary[0] on the rigid edge), so the rigid side is A in such a row.
//   kinds           0 pp | 1 pe | 2 pt | 3 ee | 4 ep | 5 tp (the table's; ep / tp are pe / pt with the rigid multi-vertex side as B)
//   contact points  pp: the vertices; pe, pt, ep, tp: sum bary_i vB_i on B, the vertex on A; ee: a0 + bary[0] (a1 - a0), b0 + bary[1] (b1 - b0)
//   slip            u0 = T[0:3].v dt + 1.13e-9, u1 = T[3:6].v dt - 1.07e-9 (the reference's offsets), |u|, epsu = dt epsv; sticking iff |u| < epsu
//   energy          E = 0.5 (mu fn / epsu) |u|^2 sticking, mu fn (|u| - epsu / 2) sliding
//   force on A      ft = c (u0 T[0:3] + u1 T[3:6]), c = mu fn / epsu sticking (no division by |u|), mu fn / |u| sliding; on B: -ft
//   node weights    A: [1] or [1 - s, s]; B: [1], [b0, b1], [b0, b1, b2] or [1 - t, t]. Node force of a deformable node: +w ft on A, -w ft on B; the
//                   linear force on a rigid body is +-ft (its weights sum to 1). Torques are not reported.
// ints [FR_NI]:    0 table (21..34) | 1 row in that table | 2 kind | 3 group of A | 4 group of B | 5 rigid body of A or -1 | 6 rigid body of B or -1 |
//                  7 flags: +1 sliding, +2 mu fn == 0, +4 degenerate (a key outside the meshes: a row of zeros)
// doubles [FR_ND]: 0 mu | 1 lagged fn | 2 epsu | 3 u0 | 4 u1 | 5 |u| | 6 slip speed |u| / dt | 7..9 v | 10..12 ft | 13 |ft| | 14 mobilised = |ft| / (mu fn),
//                  never above 1, 0 where mu fn == 0 | 15 dissipation ft.v [W] | 16 E | 17 A-side parameter s (ee rows, else 0) | 18..20 B-side weights |
//                  21..23 zero
#pragma once
#include "contact_geom.hpp"
#include "energies.hpp"

namespace mistark {

constexpr int FR_NI = 8, FR_ND = 24;
constexpr int FR_SLIDING = 1, FR_NO_LOAD = 2, FR_DEGENERATE = 4;
constexpr int FR_VERTEX_REC = 8;  // rows | sliding rows | sum s w ft (3) | largest slip speed | area | shear traction
constexpr int FR_PAIR_REC = 12;   // rows | sliding rows | sum fn | sum mu fn | sum ft (3) | sum |ft| | sum dissipation | sum E | largest slip speed | sum |ft| / sum mu fn
constexpr int FR_FIRST_TABLE = 21, FR_N_TABLES = 14;
constexpr int FR_SLOTS = 5;       // signed (vertex, weight) contributions of a row: two on A, three on B

MS_HD int fr_kind_of_table(int table)
{
    const int f = table - FR_FIRST_TABLE;
    return f < 4 ? f : (f < 8 ? f - 4 : f - 8);
}

// global_point_velocity_in_rigid_body: v1 + w1 x (R1 xloc), R1 the rotation of the integrated quaternion (rb_R1)
MS_HD D3 fr_rigid_velocity(const double* v, const double* w, const double* q0, const double* xloc, double dt)
{
    const V3<double> W(w[0], w[1], w[2]);
    const V3<double> r = rb_R1(q0, W, dt) * V3<double>(xloc[0], xloc[1], xloc[2]);
    return d3(v[0], v[1], v[2]) + cross3(d3(w[0], w[1], w[2]), d3(r.x, r.y, r.z));
}

// One row. va: velocities of A's vertices (1, or 2 for an ee row), vb: of B's (1, 2 or 3); T [6], bary [0, 2 or 3] (null for pp). wa [2], wb [3]: the
// node weights, zeros in the places the kind does not use.
MS_HD void friction_report_row(int table, int row, int ga, int gb, int rba, int rbb, const D3* va, const D3* vb, const double* T, double mu, double fn, const double* bary, double dt,
                               double epsv, int32_t* ri, double* rd, double* wa, double* wb)
{
    const int kind = fr_kind_of_table(table);
    D3 pa = va[0], pb = vb[0];
    wa[0] = 1.0; wa[1] = 0.0;
    wb[0] = 1.0; wb[1] = 0.0; wb[2] = 0.0;
    if (kind == 1 || kind == 4) {
        pb = bary[0] * vb[0] + bary[1] * vb[1];
        wb[0] = bary[0]; wb[1] = bary[1];
    } else if (kind == 2 || kind == 5) {
        pb = bary[0] * vb[0] + bary[1] * vb[1] + bary[2] * vb[2];
        wb[0] = bary[0]; wb[1] = bary[1]; wb[2] = bary[2];
    } else if (kind == 3) {
        pa = va[0] + bary[0] * (va[1] - va[0]);
        pb = vb[0] + bary[1] * (vb[1] - vb[0]);
        wa[0] = 1.0 - bary[0]; wa[1] = bary[0];
        wb[0] = 1.0 - bary[1]; wb[1] = bary[1];
    }
    const D3 v = pb - pa;
    const D3 T0 = d3(T[0], T[1], T[2]), T1 = d3(T[3], T[4], T[5]);
    const double u0 = dot3(T0, v) * dt + 1.13e-9, u1 = dot3(T1, v) * dt - 1.07e-9;
    const double un = ::sqrt(u0 * u0 + u1 * u1), epsu = dt * epsv, mufn = mu * fn;
    const bool stick = un < epsu;
    const double E = stick ? 0.5 * (mufn / epsu) * (un * un) : mufn * (un - 0.5 * epsu);
    const double c = stick ? mufn / epsu : (mufn == 0.0 ? 0.0 : mufn / un);
    const D3 ft = c * (u0 * T0 + u1 * T1);
    const double fmag = ::sqrt(sq3(ft));
    double mob = mufn == 0.0 ? 0.0 : fmag / mufn;
    mob = mob > 1.0 ? 1.0 : mob;
    ri[0] = table; ri[1] = row; ri[2] = kind; ri[3] = ga; ri[4] = gb; ri[5] = rba; ri[6] = rbb;
    ri[7] = (stick ? 0 : FR_SLIDING) | (mufn == 0.0 ? FR_NO_LOAD : 0);
    rd[0] = mu; rd[1] = fn; rd[2] = epsu; rd[3] = u0; rd[4] = u1; rd[5] = un; rd[6] = un / dt;
    rd[7] = v.x; rd[8] = v.y; rd[9] = v.z;
    rd[10] = ft.x; rd[11] = ft.y; rd[12] = ft.z;
    rd[13] = fmag;
    rd[14] = mob;
    rd[15] = dot3(ft, v);
    rd[16] = E;
    rd[17] = kind == 3 ? bary[0] : 0.0;
    rd[18] = wb[0]; rd[19] = wb[1]; rd[20] = wb[2];
    rd[21] = 0.0; rd[22] = 0.0; rd[23] = 0.0;
}

}  // namespace mistark
