// contact_report.hpp — arithmetic of the contact report, host/device: one row record per installed barrier-table key.
//
// A key names a table, a source (0 point-triangle, 1 edge-edge), the closest feature the search classified (PtType / EeType) and the two
// primitives: a = the point or the first edge, b = the triangle or the second edge (the KEY's roles, not the A / B of the reference's tables,
// which swap sides for some features). The row reports the distance of exactly that feature — point-point, point-line, point-plane or line-line,
// line and plane parameters unclamped, as the table's potential evaluates it — and never classifies the pair again: at a state other than the
// one searched, the row follows the feature it was installed with.
//
// ints [CR_NI]:    0 table | 1 source | 2 feature type | 3 group of a | 4 group of b | 5 primitive a | 6 primitive b | 7 flags
// flags:           +1 mollified (edge-edge row with mollifier < 1) | +2 open (d >= dhat) | +4 degenerate (d zero or not finite: the normal is zeros)
// doubles [CR_ND]: 0 d | 1 dhat = thickness[ga] + thickness[gb] | 2..4 closest point on a | 5..7 closest point on b | 8..10 unit normal
//                  (cA - cB) / d, from b to a | 11 mollifier m (1 for point-triangle rows) | 12 fn = m k (dhat - d)^2 [N] | 13 E = m k (dhat - d)^3 / 3 [J],
//                  unclamped as the potential has it | 14, 15 parameters of the closest points: point-triangle beta1, beta2 of cB (beta0 = 1 - beta1 -
//                  beta2), edge-edge s along a and t along b
// fn of a mollified row is the barrier part only: the force of that row also has a b grad(m) term.
#pragma once
#include "contact_geom.hpp"

namespace mistark {

constexpr int CR_NI = 8, CR_ND = 16;
constexpr int CR_MOLLIFIED = 1, CR_OPEN = 2, CR_DEGENERATE = 4;
constexpr int CR_VERTEX_REC = 5;  // gap | incident rows | sum w fn | area | pressure
constexpr int CR_PAIR_REC = 8;    // rows | min d | dhat | sum fn | sum fn n (3) | sum E

// unclamped parameter of the foot of p on the line (e0, e1)
MS_HD double cr_line_param(const D3& p, const D3& e0, const D3& e1)
{
    const D3 e = e1 - e0;
    return dot3(p - e0, e) / sq3(e);
}
MS_HD D3 cr_lerp(const D3& e0, const D3& e1, double s) { return e0 + s * (e1 - e0); }

// EnergyFrictionalContact's edge-edge mollifier (oracle/energies.py:_mollifier): rest lengths from the rest positions ra, rb of the two edges
MS_HD double cr_mollifier(const D3* ea, const D3* eb, const D3* ra, const D3* rb)
{
    const double eps_x = 1e-3 * sq3(ra[0] - ra[1]) * sq3(rb[0] - rb[1]);
    const double x = sq3(cross3(ea[1] - ea[0], eb[1] - eb[0]));
    const double r = x / eps_x;
    return x > eps_x ? 1.0 : (-1.0 * r + 2.0) * r;
}

// Node weights of a row from its type and parameters: a side [1] (point) or [1 - s, s] (edge), b side [beta0, beta1, beta2] (triangle) or
// [1 - t, t] (edge). Vertex and edge features carry exact zeros and ones in the places they do not use.
MS_HD void cr_weights(int src, int type, double p0, double p1, double* wa /*[2]*/, double* wb /*[3]*/)
{
    if (src == 0) {
        wa[0] = 1.0; wa[1] = 0.0;
        switch (type) {
            case P_T0: wb[0] = 1.0; wb[1] = 0.0; wb[2] = 0.0; break;
            case P_T1: wb[0] = 0.0; wb[1] = 1.0; wb[2] = 0.0; break;
            case P_T2: wb[0] = 0.0; wb[1] = 0.0; wb[2] = 1.0; break;
            case P_E0: wb[0] = 1.0 - p0; wb[1] = p0; wb[2] = 0.0; break;   // (t0, t1): beta1 = alpha
            case P_E1: wb[0] = 0.0; wb[1] = p0; wb[2] = p1; break;         // (t1, t2): beta1 = 1 - alpha, beta2 = alpha
            case P_E2: wb[0] = 1.0 - p1; wb[1] = 0.0; wb[2] = p1; break;   // (t2, t0): beta2 = 1 - alpha
            default: wb[0] = 1.0 - p0 - p1; wb[1] = p0; wb[2] = p1; break;
        }
        return;
    }
    wa[0] = 1.0 - p0; wa[1] = p0;
    wb[0] = 1.0 - p1; wb[1] = p1; wb[2] = 0.0;
}

// One row. xa: the point (1) or the vertices of edge a (2); xb: the vertices of the triangle (3) or of edge b (2); ra, rb: rest positions of the
// two edges (edge-edge rows only, else unused); ta, tb: contact thickness of the two groups; k: contact stiffness.
MS_HD void contact_report_row(int table, int src, int type, int a, int b, int ga, int gb, const D3* xa, const D3* xb, const D3* ra, const D3* rb, double ta, double tb, double k,
                              int32_t* ri, double* rd)
{
    double d2, p0 = 0.0, p1 = 0.0, m = 1.0;
    D3 cA, cB;
    if (src == 0) {
        const D3 p = xa[0];
        cA = p;
        switch (type) {
            case P_T0: cB = xb[0]; d2 = sq3(xb[0] - p); break;
            case P_T1: cB = xb[1]; d2 = sq3(xb[1] - p); p0 = 1.0; break;
            case P_T2: cB = xb[2]; d2 = sq3(xb[2] - p); p1 = 1.0; break;
            case P_E0: {
                const double al = cr_line_param(p, xb[0], xb[1]);
                cB = cr_lerp(xb[0], xb[1], al);
                d2 = point_line_sq(p, xb[0], xb[1]);
                p0 = al;
                break;
            }
            case P_E1: {
                const double al = cr_line_param(p, xb[1], xb[2]);
                cB = cr_lerp(xb[1], xb[2], al);
                d2 = point_line_sq(p, xb[1], xb[2]);
                p0 = 1.0 - al;
                p1 = al;
                break;
            }
            case P_E2: {
                const double al = cr_line_param(p, xb[2], xb[0]);
                cB = cr_lerp(xb[2], xb[0], al);
                d2 = point_line_sq(p, xb[2], xb[0]);
                p1 = 1.0 - al;
                break;
            }
            default: {
                const D3 n = cross3(xb[1] - xb[0], xb[2] - xb[0]);
                const double h = dot3(p - xb[0], n), n2 = sq3(n);
                d2 = h * h / n2;
                cB = p - (h / n2) * n;
                double bc[3];
                bary_point_triangle(p, xb[0], xb[1], xb[2], bc);
                p0 = bc[1];
                p1 = bc[2];
                break;
            }
        }
    } else {
        m = cr_mollifier(xa, xb, ra, rb);
        switch (type) {
            case EA0_EB0: cA = xa[0]; cB = xb[0]; break;
            case EA0_EB1: cA = xa[0]; cB = xb[1]; p1 = 1.0; break;
            case EA1_EB0: cA = xa[1]; cB = xb[0]; p0 = 1.0; break;
            case EA1_EB1: cA = xa[1]; cB = xb[1]; p0 = 1.0; p1 = 1.0; break;
            case EA_EB0: p0 = cr_line_param(xb[0], xa[0], xa[1]); cA = cr_lerp(xa[0], xa[1], p0); cB = xb[0]; break;
            case EA_EB1: p0 = cr_line_param(xb[1], xa[0], xa[1]); cA = cr_lerp(xa[0], xa[1], p0); cB = xb[1]; p1 = 1.0; break;
            case EA0_EB: p1 = cr_line_param(xa[0], xb[0], xb[1]); cA = xa[0]; cB = cr_lerp(xb[0], xb[1], p1); break;
            case EA1_EB: p1 = cr_line_param(xa[1], xb[0], xb[1]); cA = xa[1]; cB = cr_lerp(xb[0], xb[1], p1); p0 = 1.0; break;
            default: {
                const D3 u = xa[1] - xa[0], v = xb[1] - xb[0], w = xa[0] - xb[0];
                const double A = sq3(u), B = dot3(u, v), C = sq3(v), D = dot3(u, w), E = dot3(v, w);
                const double den = A * C - B * B;
                p0 = (B * E - C * D) / den;
                p1 = (A * E - B * D) / den;
                cA = cr_lerp(xa[0], xa[1], p0);
                cB = cr_lerp(xb[0], xb[1], p1);
                break;
            }
        }
        switch (type) {  // the distances of edge_edge_sq_distance, by the classified feature
            case EA0_EB0: d2 = sq3(xb[0] - xa[0]); break;
            case EA0_EB1: d2 = sq3(xb[1] - xa[0]); break;
            case EA1_EB0: d2 = sq3(xb[0] - xa[1]); break;
            case EA1_EB1: d2 = sq3(xb[1] - xa[1]); break;
            case EA_EB0: d2 = point_line_sq(xb[0], xa[0], xa[1]); break;
            case EA_EB1: d2 = point_line_sq(xb[1], xa[0], xa[1]); break;
            case EA0_EB: d2 = point_line_sq(xa[0], xb[0], xb[1]); break;
            case EA1_EB: d2 = point_line_sq(xa[1], xb[0], xb[1]); break;
            default: {
                const D3 n = cross3(xa[1] - xa[0], xb[1] - xb[0]);
                const double h = dot3(xb[0] - xa[0], n);
                d2 = h * h / sq3(n);
                break;
            }
        }
    }
    const double d = ::sqrt(d2), dhat = ta + tb;
    const bool degenerate = !(d > 0.0) || !(d < 1.7976931348623157e308);  // zero, NaN or infinite
    int flags = 0;
    if (src == 1 && m < 1.0) flags |= CR_MOLLIFIED;
    if (d >= dhat) flags |= CR_OPEN;
    if (degenerate) flags |= CR_DEGENERATE;
    const double g = dhat - d;
    ri[0] = table; ri[1] = src; ri[2] = type; ri[3] = ga; ri[4] = gb; ri[5] = a; ri[6] = b; ri[7] = flags;
    rd[0] = d;
    rd[1] = dhat;
    rd[2] = cA.x; rd[3] = cA.y; rd[4] = cA.z;
    rd[5] = cB.x; rd[6] = cB.y; rd[7] = cB.z;
    const D3 nrm = cA - cB;
    rd[8] = degenerate ? 0.0 : nrm.x / d;
    rd[9] = degenerate ? 0.0 : nrm.y / d;
    rd[10] = degenerate ? 0.0 : nrm.z / d;
    rd[11] = m;
    rd[12] = m * (k * (g * g));
    rd[13] = m * (k * (g * g * g) / 3.0);
    rd[14] = p0;
    rd[15] = p1;
}

// half the norm of the cross product: the area of one collision triangle
MS_HD double cr_triangle_area(const D3& a, const D3& b, const D3& c) { return 0.5 * ::sqrt(sq3(cross3(b - a, c - a))); }

}  // namespace mistark
