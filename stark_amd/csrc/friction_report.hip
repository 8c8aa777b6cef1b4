// friction_report.hip — opt-in friction report: one row per installed friction-table row (slip, stick or slide, friction force, dissipation, energy), one
// record per collision vertex (rows, sliding rows, friction force on the vertex, largest slip speed, area, shear traction) and one per pair of groups
// (rows, sliding rows, sums of fn, mu fn, ft, |ft|, dissipation and E, largest slip speed, mobilised share), at the velocities of the engine's current DoFs.
//
// A pipeline of its own beside eval(), like the contact report (contact_report.hip) whose scheme it follows: it reads the friction tables as the last
// friction search installed them (lagged T, mu, fn, bary), that search's sorted key list (ContactSystem::fr_keys: row order = key order; a friction row
// does not carry its groups, the key does) and the bound velocity arrays, and writes only the Context::frr_* buffers.
//   rows      : one lane per key (k_fr_rows, arithmetic: friction_report.hpp): the key is decoded into the sides with their collision vertices
//               (fr_sides), the row's table data is read through a table view of the report's own; every row also emits up to five signed
//               (collision vertex, weight) contributions (two on A, three on B; unused slots are keyed behind every vertex) and the key of its group pair
//   vertices  : contributions sorted by collision vertex (stable radix sort), one segmented pass in sorted order (k_fr_vertex_segsum): a run up to
//               FR_LONG_ROW contributions is summed by the lane at its head, a longer one by the wavefront its head lies in (lanes stride over the run,
//               then wave_sum's fixed tree); areas as the contact report has them (k_fr_vertex_init)
//   pairs     : rows sorted by group pair (stable), one workgroup per pair: thread t takes the rows t, t + 256, ... of the pair's list in order, then
//               block_sum's fixed tree (k_fr_pairs)
// A result depends on the row order alone, never on a grid size or the run. No floating-point atomics; one integer atomic counts the long runs.
#include "kernels_common.hpp"
#include "friction_report.hpp"

namespace mistark {

constexpr int FR_LONG_ROW = 64;  // contributions of one collision vertex beyond which a whole wavefront sums them

namespace {
struct FrTableDev
{
    const int32_t* conn;
    const double *T, *mu, *fn, *bary;
    int stride, nbary, start, n;
};
struct FrMesh
{
    const int32_t *cv_src, *cv_mesh, *tri, *tri_mesh, *edge, *edge_mesh, *mesh_kind, *mesh_idx;
    int n_mesh, n_v, n_t, n_e, prim_bits;
};
struct FrDev
{
    FrMesh mesh;
    const double *v1, *rb_v1, *rb_w1, *rb_q0, *rb_xloc, *X;
    double dt, epsv;
};
// The detected sides A and B of a key with their collision vertices: what decode() of contact.hip gives k_route (ProximityDetection.cpp:117-119,
// 166-176), restated with selects. decode()'s Side carries its vertices in arrays, and with the branches of this kernel merged the compiler indexes them
// at run time, which puts them into scratch; named scalars stay in registers. a0 / a1: vertices of A (na of them), b0..b2: of B (nb).
struct FrSides
{
    int ga, gb, na, nb, a0, a1, b0, b1, b2;
};
__device__ __forceinline__ FrSides fr_sides(const FrMesh& d, int src, int type, int a, int b)
{
    FrSides S;
    if (src == 0) {
        const int32_t* t = d.tri + 3 * (size_t)b;
        const int t0 = t[0], t1 = t[1], t2 = t[2];
        S.ga = d.cv_mesh[a]; S.na = 1; S.a0 = a; S.a1 = a;
        S.gb = d.tri_mesh[b];
        if (type <= P_T2) {
            S.nb = 1;
            S.b0 = type == P_T0 ? t0 : (type == P_T1 ? t1 : t2);
            S.b1 = S.b0; S.b2 = S.b0;
        } else if (type <= P_E2) {  // P_E0: (t0,t1), P_E1: (t1,t2), P_E2: (t2,t0)
            S.nb = 2;
            S.b0 = type == P_E0 ? t0 : (type == P_E1 ? t1 : t2);
            S.b1 = type == P_E0 ? t1 : (type == P_E1 ? t2 : t0);
            S.b2 = S.b0;
        } else {
            S.nb = 3;
            S.b0 = t0; S.b1 = t1; S.b2 = t2;
        }
        return S;
    }
    const int ea0 = d.edge[2 * (size_t)a], ea1 = d.edge[2 * (size_t)a + 1], eb0 = d.edge[2 * (size_t)b], eb1 = d.edge[2 * (size_t)b + 1];
    const int ma = d.edge_mesh[a], mb = d.edge_mesh[b];
    if (type <= EA1_EB1) {  // EA0_EB0, EA0_EB1, EA1_EB0, EA1_EB1: a point of edge a, a point of edge b
        S.ga = ma; S.gb = mb; S.na = 1; S.nb = 1;
        S.a0 = (type == EA0_EB0 || type == EA0_EB1) ? ea0 : ea1;
        S.b0 = (type == EA0_EB0 || type == EA1_EB0) ? eb0 : eb1;
        S.a1 = S.a0; S.b1 = S.b0;
    } else if (type == EA_EB0 || type == EA_EB1) {  // the point is on edge b: A = that point, B = edge a
        S.ga = mb; S.gb = ma; S.na = 1; S.nb = 2;
        S.a0 = type == EA_EB0 ? eb0 : eb1;
        S.a1 = S.a0;
        S.b0 = ea0; S.b1 = ea1;
    } else if (type == EA0_EB || type == EA1_EB) {
        S.ga = ma; S.gb = mb; S.na = 1; S.nb = 2;
        S.a0 = type == EA0_EB ? ea0 : ea1;
        S.a1 = S.a0;
        S.b0 = eb0; S.b1 = eb1;
    } else {
        S.ga = ma; S.gb = mb; S.na = 2; S.nb = 2;
        S.a0 = ea0; S.a1 = ea1; S.b0 = eb0; S.b1 = eb1;
    }
    S.b2 = S.b0;
    return S;
}
__device__ __forceinline__ D3 fr_ld(const double* X, int i) { return d3(X[3 * (size_t)i], X[3 * (size_t)i + 1], X[3 * (size_t)i + 2]); }
// velocity of collision vertex cv of a mesh of kind `kind` (0 deformable, 1 rigid body number `body`)
__device__ __forceinline__ D3 fr_vertex_velocity(const FrDev& d, int cv, int kind, int body)
{
    const int s = d.mesh.cv_src[cv];
    if (kind == 0) return fr_ld(d.v1, s);
    return fr_rigid_velocity(d.rb_v1 + 3 * (size_t)body, d.rb_w1 + 3 * (size_t)body, d.rb_q0 + 4 * (size_t)body, d.rb_xloc + 3 * (size_t)s, d.dt);
}
}  // namespace

__global__ __launch_bounds__(BLOCK) void k_fr_rows(FrDev d, const uint64_t* __restrict__ keys, int n, const FrTableDev* __restrict__ tables, int32_t* __restrict__ rows_i,
                                                  double* __restrict__ rows_d, uint32_t* __restrict__ ckey, uint32_t* __restrict__ cval, double* __restrict__ cw,
                                                  uint32_t* __restrict__ pkey, uint32_t* __restrict__ pval)
{
    const int i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    const uint64_t key = keys[i];
    const uint32_t mask = (1u << d.mesh.prim_bits) - 1u;
    const int table = (int)(key >> 58), src = (int)((key >> 57) & 1), type = (int)((key >> 53) & 15);
    const int a = (int)((key >> d.mesh.prim_bits) & mask), b = (int)(key & mask);
    int32_t ri[FR_NI];
    double rd[FR_ND];
    // contributions: slots 0, 1 on A, 2..4 on B (named scalars: nothing here is indexed at run time)
    int c0 = 0, c1 = 0, c2 = 0, c3 = 0, c4 = 0, used = 0;
    double w0 = 0.0, w1 = 0.0, w2 = 0.0, w3 = 0.0, w4 = 0.0;
    int ga = 0, gb = 0, row = 0;
    // (keys are the detector's own; a primitive or a table outside what is installed would be a bug there — such a row is reported degenerate, nothing is read)
    bool ok = table >= FR_FIRST_TABLE && table < FR_FIRST_TABLE + FR_N_TABLES;
    ok = ok && (src == 0 ? (a < d.mesh.n_v && b < d.mesh.n_t && type <= P_T) : (a < d.mesh.n_e && b < d.mesh.n_e && type <= EA_EB));
    FrTableDev T{};
    if (ok) {
        T = tables[table - FR_FIRST_TABLE];
        row = i - T.start;
        ok = row >= 0 && row < T.n;
    }
    if (ok) {
        const FrSides S = fr_sides(d.mesh, src, type, a, b);
        const int kA = d.mesh.mesh_kind[S.ga], kB = d.mesh.mesh_kind[S.gb];
        // friction_rb_d_pp (29) and friction_rb_d_ee (32) with the deformable side detected first: the potential subtracts the rigid side (friction_report.hpp)
        const bool swap = (table == 29 || table == 32) && kA == 0 && kB == 1;
        const int na = S.na, nb = S.nb;  // (equal in the swapped rows)
        const int ka = swap ? kB : kA, kb = swap ? kA : kB;
        ga = swap ? S.gb : S.ga;
        gb = swap ? S.ga : S.gb;
        const int ba = d.mesh.mesh_idx[ga], bb = d.mesh.mesh_idx[gb];
        c0 = swap ? S.b0 : S.a0;
        c1 = swap ? S.b1 : S.a1;
        c2 = swap ? S.a0 : S.b0;
        c3 = swap ? S.a1 : S.b1;
        c4 = S.b2;
        D3 va[2], vb[3];
        va[0] = fr_vertex_velocity(d, c0, ka, ba);
        va[1] = na > 1 ? fr_vertex_velocity(d, c1, ka, ba) : va[0];
        vb[0] = fr_vertex_velocity(d, c2, kb, bb);
        vb[1] = nb > 1 ? fr_vertex_velocity(d, c3, kb, bb) : vb[0];
        vb[2] = nb > 2 ? fr_vertex_velocity(d, c4, kb, bb) : vb[0];
        double Tm[6], bary[3] = {0.0, 0.0, 0.0};
#pragma unroll
        for (int j = 0; j < 6; j++) Tm[j] = T.T[6 * (size_t)row + j];
        if (T.nbary >= 2) {
            bary[0] = T.bary[(size_t)T.nbary * row];
            bary[1] = T.bary[(size_t)T.nbary * row + 1];
        }
        if (T.nbary == 3) bary[2] = T.bary[3 * (size_t)row + 2];
        double wa[2], wb[3];
        friction_report_row(table, row, ga, gb, ka == 1 ? ba : -1, kb == 1 ? bb : -1, va, vb, Tm, T.mu[row], T.fn[row], bary, d.dt, d.epsv, ri, rd, wa, wb);
        w0 = wa[0]; w1 = wa[1]; w2 = -wb[0]; w3 = -wb[1]; w4 = -wb[2];
        used = 1 | (na > 1 ? 2 : 0) | 4 | (nb > 1 ? 8 : 0) | (nb > 2 ? 16 : 0);
    } else {  // reported as a degenerate row of zeros; it takes no part in the vertex and pair records (keys behind every vertex and every pair)
        ri[0] = table; ri[1] = row; ri[2] = 0; ri[3] = 0; ri[4] = 0; ri[5] = -1; ri[6] = -1; ri[7] = FR_DEGENERATE;
#pragma unroll
        for (int j = 0; j < FR_ND; j++) rd[j] = 0.0;
    }
#pragma unroll
    for (int j = 0; j < FR_NI; j++) rows_i[(size_t)FR_NI * i + j] = ri[j];
#pragma unroll
    for (int j = 0; j < FR_ND; j++) rows_d[(size_t)FR_ND * i + j] = rd[j];
    const size_t at = (size_t)FR_SLOTS * i;
    const uint32_t behind = (uint32_t)d.mesh.n_v;
    ckey[at] = (used & 1) ? (uint32_t)c0 : behind;
    ckey[at + 1] = (used & 2) ? (uint32_t)c1 : behind;
    ckey[at + 2] = (used & 4) ? (uint32_t)c2 : behind;
    ckey[at + 3] = (used & 8) ? (uint32_t)c3 : behind;
    ckey[at + 4] = (used & 16) ? (uint32_t)c4 : behind;
    cw[at] = w0; cw[at + 1] = w1; cw[at + 2] = w2; cw[at + 3] = w3; cw[at + 4] = w4;
#pragma unroll
    for (int j = 0; j < FR_SLOTS; j++) cval[at + j] = (uint32_t)at + (uint32_t)j;
    const int lo = ga < gb ? ga : gb, hi = ga < gb ? gb : ga;
    pkey[i] = ok ? (uint32_t)lo * (uint32_t)d.mesh.n_mesh + (uint32_t)hi : (uint32_t)d.mesh.n_mesh * (uint32_t)d.mesh.n_mesh;
    pval[i] = (uint32_t)i;
}

// per collision vertex: no rows, no force; area = a third of the current areas of its collision triangles, in the order of the incidence list (the scheme
// of k_cr_vertex_init)
__global__ __launch_bounds__(BLOCK) void k_fr_vertex_init(FrDev d, const int32_t* __restrict__ inc_start, const int32_t* __restrict__ inc_tri, double* __restrict__ vert)
{
    const int v = blockIdx.x * BLOCK + threadIdx.x;
    if (v >= d.mesh.n_v) return;
    double s = 0.0;
    for (int j = inc_start[v]; j < inc_start[v + 1]; j++) {
        const int32_t* t = d.mesh.tri + 3 * (size_t)inc_tri[j];
        const D3 p = fr_ld(d.X, t[0]), q = fr_ld(d.X, t[1]), r = fr_ld(d.X, t[2]);
        s += 0.5 * ::sqrt(sq3(cross3(q - p, r - p)));
    }
    double* o = vert + (size_t)FR_VERTEX_REC * v;
#pragma unroll
    for (int j = 0; j < FR_VERTEX_REC; j++) o[j] = 0.0;
    o[6] = s / 3.0;
}

namespace {
struct FrVertexAcc
{
    double fx = 0.0, fy = 0.0, fz = 0.0, sliding = 0.0, speed = 0.0;
};
__device__ __forceinline__ void fr_vertex_add(FrVertexAcc& a, uint32_t c, const int32_t* __restrict__ rows_i, const double* __restrict__ rows_d, const double* __restrict__ cw)
{
    const uint32_t r = c / (uint32_t)FR_SLOTS;
    const double* rd = rows_d + (size_t)FR_ND * r;
    const double w = cw[c];
    a.fx += w * rd[10];
    a.fy += w * rd[11];
    a.fz += w * rd[12];
    a.sliding += (rows_i[(size_t)FR_NI * r + 7] & FR_SLIDING) ? 1.0 : 0.0;
    a.speed = fmax(a.speed, rd[6]);
}
__device__ __forceinline__ void fr_vertex_store(double* __restrict__ vert, uint32_t v, double count, const FrVertexAcc& a)
{
    double* o = vert + (size_t)FR_VERTEX_REC * v;
    const double area = o[6];
    o[0] = count;
    o[1] = a.sliding;
    o[2] = a.fx;
    o[3] = a.fy;
    o[4] = a.fz;
    o[5] = a.speed;
    o[7] = area > 0.0 ? ::sqrt(a.fx * a.fx + a.fy * a.fy + a.fz * a.fz) / area : 0.0;
}
}  // namespace
// Segmented pass over the sorted contributions (the scheme of k_cr_vertex_segsum): one lane per sorted position, the lane at the head of a vertex's run owns
// the vertex. No lane leaves early: the cross-lane steps need all 64.
__global__ __launch_bounds__(BLOCK) void k_fr_vertex_segsum(const uint32_t* __restrict__ key, const uint32_t* __restrict__ val, int64_t total, const int32_t* __restrict__ rows_i,
                                                           const double* __restrict__ rows_d, const double* __restrict__ cw, int n_v, double* __restrict__ vert,
                                                           uint32_t* __restrict__ stat)
{
    const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    const int lane = threadIdx.x & 63;
    uint32_t row = 0;
    int64_t end = 0;
    bool head = false;
    if (i < total) {
        row = key[i];
        head = (i == 0 || key[i - 1] != row) && row < (uint32_t)n_v;  // (key n_v: unused slots and the rows that take no part, sorted last)
        if (head) {
            int64_t lo = i, hi = total;  // first position behind the run
            while (hi - lo > 1) {
                const int64_t mid = (lo + hi) >> 1;
                if (key[mid] == row) lo = mid;
                else hi = mid;
            }
            end = hi;
        }
    }
    const bool is_long = head && end - i > FR_LONG_ROW;
    if (head && !is_long) {
        FrVertexAcc acc;
        for (int64_t j = i; j < end; j++) fr_vertex_add(acc, val[j], rows_i, rows_d, cw);
        fr_vertex_store(vert, row, (double)(end - i), acc);
    }
    const unsigned long long any_long = __ballot(is_long);
    unsigned long long m = ((unsigned long long)(uint32_t)__builtin_amdgcn_readfirstlane((int)(any_long >> 32)) << 32) | (uint32_t)__builtin_amdgcn_readfirstlane((int)any_long);
    if (lane == 0 && m) atomicAdd(&stat[0], (uint32_t)__popcll(m));  // (an integer count for the tests; no sum depends on it)
    const int64_t wave_first = i - lane;
    while (m) {
        const int src = __ffsll((long long)m) - 1;
        m &= m - 1;
        const int64_t first = wave_first + src;
        const int64_t last = (int64_t)(uint32_t)__shfl((int)(uint32_t)end, src, 64);  // (total < 2^31)
        const uint32_t r = (uint32_t)__shfl((int)row, src, 64);
        FrVertexAcc acc;
        for (int64_t j = first + lane; j < last; j += 64) fr_vertex_add(acc, val[j], rows_i, rows_d, cw);
        acc.fx = wave_sum(acc.fx);
        acc.fy = wave_sum(acc.fy);
        acc.fz = wave_sum(acc.fz);
        acc.sliding = wave_sum(acc.sliding);
        acc.speed = wave_max(acc.speed);
        if (lane == 0) fr_vertex_store(vert, r, (double)(last - first), acc);
    }
}

// one workgroup per ordered pair (ga, gb) of groups; ga <= gb: the pair's rows [lo, hi) of the list sorted by pair, else zeros
__global__ __launch_bounds__(BLOCK) void k_fr_pairs(const uint32_t* __restrict__ pkey, const uint32_t* __restrict__ pval, int n, int n_mesh, const int32_t* __restrict__ rows_i,
                                                   const double* __restrict__ rows_d, double* __restrict__ out)
{
    __shared__ double sm[4];
    const int ga = blockIdx.x / n_mesh, gb = blockIdx.x % n_mesh;
    double* o = out + (size_t)FR_PAIR_REC * blockIdx.x;
    if (ga > gb) {
        if (threadIdx.x < FR_PAIR_REC) o[threadIdx.x] = 0.0;
        return;
    }
    const uint32_t want = (uint32_t)blockIdx.x;
    int lo = 0, hi = n;  // first position with pkey >= want
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (pkey[mid] < want) lo = mid + 1;
        else hi = mid;
    }
    const int first = lo;
    hi = n;  // first position with pkey > want
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (pkey[mid] <= want) lo = mid + 1;
        else hi = mid;
    }
    const int last = lo;
    double s[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, speed = 0.0;
    for (int t = first + (int)threadIdx.x; t < last; t += BLOCK) {
        const uint32_t r = pval[t];
        const double* rd = rows_d + (size_t)FR_ND * r;
        const int32_t* ri = rows_i + (size_t)FR_NI * r;
        const double sign = ri[3] <= ri[4] ? 1.0 : -1.0;  // the force on the lower-numbered group; on A inside one group
        s[0] += (ri[7] & FR_SLIDING) ? 1.0 : 0.0;
        s[1] += rd[1];
        s[2] += rd[0] * rd[1];
        s[3] += sign * rd[10];
        s[4] += sign * rd[11];
        s[5] += sign * rd[12];
        s[6] += rd[13];
        s[7] += rd[15];
        s[8] += rd[16];
        speed = fmax(speed, rd[6]);
    }
    speed = block_max(speed, sm);
    double v[9];
#pragma unroll
    for (int k = 0; k < 9; k++) v[k] = block_sum(s[k], sm);
    if (threadIdx.x == 0) {
        o[0] = (double)(last - first);
#pragma unroll
        for (int k = 0; k < 9; k++) o[1 + k] = v[k];
        o[10] = speed;
        o[11] = v[2] != 0.0 ? v[6] / v[2] : 0.0;
    }
}

namespace {
const char* const WHO = "friction report";
void refuse(Context& c)
{
    if (c.dry) throw Error(std::string(WHO) + ": registration-only context (mistark_create_dry): nothing can be evaluated");
    if (c.world > 1) throw Error(std::string(WHO) + ": single-rank accessor (a sharded context holds the elements touching its rows)");
}
int bits_for(int64_t n)
{
    int bits = 1;
    while (bits < 32 && (1ll << bits) <= n) bits++;
    return bits;
}
const uint32_t* sort_pairs(Context& c, uint32_t* key, uint32_t* key_alt, uint32_t* val, uint32_t* val_alt, int64_t n, int bits, const uint32_t** sorted_val)
{
    hipcub::DoubleBuffer<uint32_t> dk(key, key_alt), dv(val, val_alt);
    size_t tmp = 0;
    MS_CHECK(hipcub::DeviceRadixSort::SortPairs(nullptr, tmp, dk, dv, (int)n, 0, bits, c.stream));
    c.frr_cub_tmp.ensure(tmp);
    MS_CHECK(hipcub::DeviceRadixSort::SortPairs(c.frr_cub_tmp.p, tmp, dk, dv, (int)n, 0, bits, c.stream));  // (stable: equal keys keep the row order)
    *sorted_val = dv.Current();
    return dk.Current();
}
}  // namespace

void friction_report_sizes(Context& c, int64_t* n_rows, int64_t* n_vertices, int32_t* n_groups)
{
    refuse(c);
    FrictionReportView V;
    friction_report_view(c, V, true);
    if (n_rows) *n_rows = V.n_keys;
    if (n_vertices) *n_vertices = V.n_v;
    if (n_groups) *n_groups = V.n_mesh;
}

void friction_report_run(Context& c, int set)
{
    refuse(c);
    FrictionReportView V;
    friction_report_view(c, V, false);
    Context::FrictionReportSet& S = c.frr_set[set];
    const int64_t n = V.n_keys;
    S.n_rows = -1;
    if ((int64_t)FR_SLOTS * n >= (1ll << 31)) throw Error(std::string(WHO) + ": too many rows");
    if ((int64_t)V.n_mesh * V.n_mesh >= (1ll << 31)) throw Error(std::string(WHO) + ": too many groups");
    S.n_v = V.n_v;
    S.n_groups = V.n_mesh;
    if (V.n_v == 0) {  // no collision mesh: nothing to launch
        S.n_rows = 0;
        return;
    }
    S.rows_i.ensure((size_t)FR_NI * std::max<int64_t>(n, 1));
    S.rows_d.ensure((size_t)FR_ND * std::max<int64_t>(n, 1));
    S.vert.ensure((size_t)FR_VERTEX_REC * V.n_v);
    S.pair.ensure((size_t)FR_PAIR_REC * V.n_mesh * V.n_mesh);
    c.n_friction_reports++;
    c.frr_stat.ensure(2);
    fill_async(c.stream, c.frr_stat.p, 0, 2 * sizeof(uint32_t));
    c.frr_stat_valid = true;
    if (n == 0) {  // no friction rows (no friction search on this mesh set yet, friction off, every mu zero): records of zeros, no kernel
        fill_async(c.stream, S.vert.p, 0, (size_t)FR_VERTEX_REC * V.n_v * sizeof(double));
        fill_async(c.stream, S.pair.p, 0, (size_t)FR_PAIR_REC * V.n_mesh * V.n_mesh * sizeof(double));
        S.n_rows = 0;
        return;
    }
    c.frr_X.ensure(3 * (size_t)V.n_v);
    contact_report_positions(c, c.frr_X.p);
    if (c.frr_inc_meshes != V.n_mesh) {
        // the triangles of every collision vertex, in triangle order (counting sort); meshes are only ever added
        std::vector<int32_t> table((size_t)V.n_v + 1 + 3 * (size_t)V.n_t, 0);
        for (int32_t v : *V.h_tri) table[(size_t)v + 1]++;
        for (int v = 0; v < V.n_v; v++) table[(size_t)v + 1] += table[(size_t)v];
        std::vector<int32_t> at(table.begin(), table.begin() + V.n_v);
        for (int t = 0; t < V.n_t; t++)
            for (int j = 0; j < 3; j++) table[(size_t)V.n_v + 1 + (size_t)at[(size_t)(*V.h_tri)[3 * (size_t)t + j]]++] = t;
        c.frr_inc.ensure(table.size());
        h2d_staged(c, c.frr_inc.p, table.data(), table.size() * sizeof(int32_t));
        MS_CHECK(hipStreamSynchronize(c.stream));  // (the list is a temporary)
        c.frr_inc_meshes = V.n_mesh;
    }
    FrTableDev tables[FR_N_TABLES];
    for (int t = 0; t < FR_N_TABLES; t++) {
        const FrictionReportView::Table& T = V.tables[t];
        tables[t] = FrTableDev{T.conn, T.T, T.mu, T.fn, T.bary, T.stride, T.nbary, T.start, T.n};
    }
    c.frr_tables.ensure(sizeof(tables));
    h2d_staged(c, c.frr_tables.p, tables, sizeof(tables));
    MS_CHECK(hipStreamSynchronize(c.stream));  // (the views are a temporary)
    FrDev d{};
    d.mesh.prim_bits = V.prim_bits;
    d.mesh.cv_src = V.cv_src; d.mesh.cv_mesh = V.cv_mesh; d.mesh.tri = V.tri; d.mesh.tri_mesh = V.tri_mesh; d.mesh.edge = V.edge; d.mesh.edge_mesh = V.edge_mesh;
    d.mesh.mesh_kind = V.mesh_kind; d.mesh.mesh_idx = V.mesh_idx;
    d.mesh.n_mesh = V.n_mesh; d.mesh.n_v = V.n_v; d.mesh.n_t = V.n_t; d.mesh.n_e = V.n_e;
    d.v1 = V.v1; d.rb_v1 = V.rb_v1; d.rb_w1 = V.rb_w1; d.rb_q0 = V.rb_q0; d.rb_xloc = V.rb_xloc; d.X = c.frr_X.p;
    d.dt = V.dt; d.epsv = V.epsv;
    const size_t nc = (size_t)FR_SLOTS * (size_t)n;
    c.frr_key.ensure(nc + (size_t)n);  // contributions, then the rows' pair keys
    c.frr_key_alt.ensure(nc + (size_t)n);
    c.frr_val.ensure(nc + (size_t)n);
    c.frr_val_alt.ensure(nc + (size_t)n);
    c.frr_w.ensure(nc);
    hipLaunchKernelGGL(k_fr_rows, dim3(grid_for(n)), dim3(BLOCK), 0, c.stream, d, V.keys, (int)n, (const FrTableDev*)c.frr_tables.p, S.rows_i.p, S.rows_d.p, c.frr_key.p, c.frr_val.p,
                       c.frr_w.p, c.frr_key.p + nc, c.frr_val.p + nc);
    hipLaunchKernelGGL(k_fr_vertex_init, dim3(grid_for(V.n_v)), dim3(BLOCK), 0, c.stream, d, (const int32_t*)c.frr_inc.p, (const int32_t*)c.frr_inc.p + V.n_v + 1, S.vert.p);
    const uint32_t* sv = nullptr;
    const uint32_t* sk = sort_pairs(c, c.frr_key.p, c.frr_key_alt.p, c.frr_val.p, c.frr_val_alt.p, (int64_t)nc, bits_for(V.n_v), &sv);
    hipLaunchKernelGGL(k_fr_vertex_segsum, dim3(grid_for((int64_t)nc)), dim3(BLOCK), 0, c.stream, sk, sv, (int64_t)nc, (const int32_t*)S.rows_i.p, (const double*)S.rows_d.p,
                       (const double*)c.frr_w.p, V.n_v, S.vert.p, c.frr_stat.p);
    const uint32_t* pv = nullptr;
    const uint32_t* pk = sort_pairs(c, c.frr_key.p + nc, c.frr_key_alt.p + nc, c.frr_val.p + nc, c.frr_val_alt.p + nc, n, bits_for((int64_t)V.n_mesh * V.n_mesh), &pv);
    hipLaunchKernelGGL(k_fr_pairs, dim3((unsigned)(V.n_mesh * V.n_mesh)), dim3(BLOCK), 0, c.stream, pk, pv, (int)n, V.n_mesh, (const int32_t*)S.rows_i.p, (const double*)S.rows_d.p,
                       S.pair.p);
    MS_CHECK(hipGetLastError());
    S.n_rows = n;
}

namespace {
const Context::FrictionReportSet& recorded(Context& c, int set)
{
    const Context::FrictionReportSet& S = c.frr_set[set];
    if (S.n_rows < 0) throw Error(std::string(WHO) + ": nothing recorded");
    return S;
}
template <class T>
void download(Context& c, T* dst, const T* src, size_t n)
{
    if (!dst || n == 0) return;
    MS_CHECK(hipMemcpyAsync(dst, src, n * sizeof(T), hipMemcpyDeviceToHost, c.stream));
    MS_CHECK(hipStreamSynchronize(c.stream));
}
}  // namespace

void friction_report_rows(Context& c, int set, int32_t* rows_i, double* rows_d, int64_t* n_rows)
{
    const Context::FrictionReportSet& S = recorded(c, set);
    if (n_rows) *n_rows = S.n_rows;
    download(c, rows_i, (const int32_t*)S.rows_i.p, (size_t)FR_NI * S.n_rows);
    download(c, rows_d, (const double*)S.rows_d.p, (size_t)FR_ND * S.n_rows);
}
void friction_report_vertices(Context& c, int set, double* out, int32_t* group, int32_t* source_index, int64_t* n_vertices)
{
    const Context::FrictionReportSet& S = recorded(c, set);
    if (n_vertices) *n_vertices = S.n_v;
    download(c, out, (const double*)S.vert.p, (size_t)FR_VERTEX_REC * S.n_v);
    if (group || source_index) {
        FrictionReportView V;
        friction_report_view(c, V, true);
        for (int64_t v = 0; v < S.n_v; v++) {
            if (group) group[v] = (*V.h_cv_mesh)[(size_t)v];
            if (source_index) source_index[v] = (*V.h_cv_src)[(size_t)v];
        }
    }
}
void friction_report_pairs(Context& c, int set, double* out, int32_t* n_groups)
{
    const Context::FrictionReportSet& S = recorded(c, set);
    if (n_groups) *n_groups = S.n_groups;
    if (S.n_v == 0) return;
    download(c, out, (const double*)S.pair.p, (size_t)FR_PAIR_REC * S.n_groups * S.n_groups);
}
int64_t friction_report_long_rows(Context& c)
{
    if (!c.frr_stat_valid) return 0;
    uint32_t v[2] = {0, 0};
    fetch(c, v, c.frr_stat.p, sizeof(v));
    return (int64_t)v[0];
}

}  // namespace mistark
