// contact_report.hip — opt-in contact report: one row per installed barrier-table key (pair, gap, closest points, normal, normal force, energy), one
// record per collision vertex (gap, incident rows, normal force share, area, pressure) and one per pair of groups (rows, smallest gap, normal force
// resultant, energy), at the engine's current DoFs.
//
// A pipeline of its own beside eval(), like the force, stress and budget readouts: it reads the detector's installed key list and meshes (no search
// runs) and the state arrays, and writes only the Context::cr_* buffers. One exception: before the first search of a mesh set the collision meshes are not
// on the device yet, and the report uploads them as that search would (contact_report_view).
//   positions : k_contact_vertices (contact.hip) at the current DoFs into cr_X — the detector's own X, tables, caches and counters are not written
//   rows      : one lane per key, in key order = the order of the installed tables (k_cr_rows, arithmetic: contact_report.hpp); every row also emits
//               its four (primitive vertex, weight) contributions and the key of its group pair
//   vertices  : contributions sorted by collision vertex (stable radix sort), one segmented pass in sorted order (k_cr_vertex_segsum): a run up to
//               CR_LONG_ROW contributions is summed by the lane at its head, a longer one by the wavefront its head lies in (lanes stride over the run,
//               then wave_sum's fixed tree); areas from a triangle-incidence list built once per mesh set (k_cr_vertex_init)
//   pairs     : rows sorted by group pair (stable), one workgroup per pair: thread t takes the rows t, t + 256, ... of the pair's list in order, then
//               block_sum's fixed tree (k_cr_pairs)
// A result depends on the row order alone, never on a grid size or the run. No floating-point atomics; one integer atomic counts the long runs.
#include "kernels_common.hpp"
#include "contact_report.hpp"

namespace mistark {

constexpr int CR_LONG_ROW = 64;  // contributions of one collision vertex beyond which a whole wavefront sums them

namespace {
struct CrDev
{
    const int32_t *cv_src, *cv_mesh, *tri, *tri_mesh, *edge, *edge_mesh, *mesh_kind;
    const double *thick, *k, *X_rest, *rb_xloc, *X;
    int n_mesh, n_v, n_t, n_e, prim_bits;
};
__device__ __forceinline__ D3 cr_ld(const double* X, int i) { return d3(X[3 * (size_t)i], X[3 * (size_t)i + 1], X[3 * (size_t)i + 2]); }
__device__ __forceinline__ double wave_min(double v)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v = fmin(v, __shfl_down(v, d, 64));
    return v;
}
}  // namespace

__global__ __launch_bounds__(BLOCK) void k_cr_rows(CrDev d, const uint64_t* __restrict__ keys, int n, int32_t* __restrict__ rows_i, double* __restrict__ rows_d,
                                                  uint32_t* __restrict__ ckey, uint32_t* __restrict__ cval, double* __restrict__ cw, uint32_t* __restrict__ pkey,
                                                  uint32_t* __restrict__ pval)
{
    const int i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    const uint64_t key = keys[i];
    const uint32_t mask = (1u << d.prim_bits) - 1u;
    const int table = (int)(key >> 58), src = (int)((key >> 57) & 1), type = (int)((key >> 53) & 15);
    const int a = (int)((key >> d.prim_bits) & mask), b = (int)(key & mask);
    int32_t ri[CR_NI];
    double rd[CR_ND];
    int cv[4] = {0, 0, 0, 0};
    double w[4] = {0.0, 0.0, 0.0, 0.0};
    int ga = 0, gb = 0;
    // (keys are the detector's own; a primitive outside the meshes would be a bug there — such a row is reported degenerate, nothing is read)
    const bool ok = src == 0 ? (a < d.n_v && b < d.n_t && type <= P_T) : (a < d.n_e && b < d.n_e && type <= EA_EB);
    if (ok) {
        D3 xa[2], xb[3], ra[2], rb[2];
        if (src == 0) {
            ga = d.cv_mesh[a];
            gb = d.tri_mesh[b];
            cv[0] = a;
            xa[0] = cr_ld(d.X, a);
            xa[1] = xa[0];
#pragma unroll
            for (int j = 0; j < 3; j++) {
                cv[1 + j] = d.tri[3 * (size_t)b + j];
                xb[j] = cr_ld(d.X, cv[1 + j]);
            }
            ra[0] = ra[1] = rb[0] = rb[1] = d3(0.0, 0.0, 0.0);
        } else {
            ga = d.edge_mesh[a];
            gb = d.edge_mesh[b];
            const double* rest_a = d.mesh_kind[ga] == 0 ? d.X_rest : d.rb_xloc;
            const double* rest_b = d.mesh_kind[gb] == 0 ? d.X_rest : d.rb_xloc;
#pragma unroll
            for (int j = 0; j < 2; j++) {
                cv[j] = d.edge[2 * (size_t)a + j];
                cv[2 + j] = d.edge[2 * (size_t)b + j];
                xa[j] = cr_ld(d.X, cv[j]);
                xb[j] = cr_ld(d.X, cv[2 + j]);
                ra[j] = cr_ld(rest_a, d.cv_src[cv[j]]);
                rb[j] = cr_ld(rest_b, d.cv_src[cv[2 + j]]);
            }
            xb[2] = xb[1];
        }
        contact_report_row(table, src, type, a, b, ga, gb, xa, xb, ra, rb, d.thick[ga], d.thick[gb], d.k[0], ri, rd);
        double wa[2], wb[3];
        cr_weights(src, type, rd[14], rd[15], wa, wb);
        if (src == 0) {
            w[0] = wa[0]; w[1] = wb[0]; w[2] = wb[1]; w[3] = wb[2];
        } else {
            w[0] = wa[0]; w[1] = wa[1]; w[2] = wb[0]; w[3] = wb[1];
        }
    } else {  // reported as a degenerate row of zeros; it takes no part in the vertex and pair records (keys behind every vertex and every pair)
        ri[0] = table; ri[1] = src; ri[2] = type; ri[3] = 0; ri[4] = 0; ri[5] = a; ri[6] = b; ri[7] = CR_DEGENERATE;
#pragma unroll
        for (int j = 0; j < CR_ND; j++) rd[j] = 0.0;
    }
#pragma unroll
    for (int j = 0; j < CR_NI; j++) rows_i[(size_t)CR_NI * i + j] = ri[j];
#pragma unroll
    for (int j = 0; j < CR_ND; j++) rows_d[(size_t)CR_ND * i + j] = rd[j];
#pragma unroll
    for (int j = 0; j < 4; j++) {
        ckey[4 * (size_t)i + j] = ok ? (uint32_t)cv[j] : (uint32_t)d.n_v;
        cval[4 * (size_t)i + j] = 4u * (uint32_t)i + (uint32_t)j;
        cw[4 * (size_t)i + j] = w[j];
    }
    const int lo = ga < gb ? ga : gb, hi = ga < gb ? gb : ga;
    pkey[i] = ok ? (uint32_t)lo * (uint32_t)d.n_mesh + (uint32_t)hi : (uint32_t)d.n_mesh * (uint32_t)d.n_mesh;
    pval[i] = (uint32_t)i;
}

// per collision vertex: gap +inf, no rows, no force; area = a third of the current areas of its collision triangles, in the order of the incidence list
__global__ __launch_bounds__(BLOCK) void k_cr_vertex_init(CrDev d, const int32_t* __restrict__ inc_start, const int32_t* __restrict__ inc_tri, double* __restrict__ vert)
{
    const int v = blockIdx.x * BLOCK + threadIdx.x;
    if (v >= d.n_v) return;
    double s = 0.0;
    for (int j = inc_start[v]; j < inc_start[v + 1]; j++) {
        const int32_t* t = d.tri + 3 * (size_t)inc_tri[j];
        s += cr_triangle_area(cr_ld(d.X, t[0]), cr_ld(d.X, t[1]), cr_ld(d.X, t[2]));
    }
    double* o = vert + (size_t)CR_VERTEX_REC * v;
    o[0] = __builtin_huge_val();
    o[1] = 0.0;
    o[2] = 0.0;
    o[3] = s / 3.0;
    o[4] = 0.0;
}

__device__ __forceinline__ void cr_vertex_store(double* __restrict__ vert, uint32_t v, double gap, double count, double share)
{
    double* o = vert + (size_t)CR_VERTEX_REC * v;
    const double area = o[3];
    o[0] = gap;
    o[1] = count;
    o[2] = share;
    o[4] = area > 0.0 ? share / area : 0.0;
}
// Segmented pass over the sorted contributions (the scheme of k_force_segsum): one lane per sorted position, the lane at the head of a vertex's run owns
// the vertex. No lane leaves early: the cross-lane steps need all 64.
__global__ __launch_bounds__(BLOCK) void k_cr_vertex_segsum(const uint32_t* __restrict__ key, const uint32_t* __restrict__ val, int64_t total, const double* __restrict__ rows_d,
                                                           const double* __restrict__ cw, int n_v, double* __restrict__ vert, uint32_t* __restrict__ stat)
{
    const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    const int lane = threadIdx.x & 63;
    uint32_t row = 0;
    int64_t end = 0;
    bool head = false;
    if (i < total) {
        row = key[i];
        head = (i == 0 || key[i - 1] != row) && row < (uint32_t)n_v;  // (key n_v: the contributions of rows that take no part, sorted last)
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
    const bool is_long = head && end - i > CR_LONG_ROW;
    if (head && !is_long) {
        double gap = __builtin_huge_val(), share = 0.0;
        for (int64_t j = i; j < end; j++) {
            const uint32_t c = val[j];
            const double* r = rows_d + (size_t)CR_ND * (c >> 2);
            gap = fmin(gap, r[0]);
            share += cw[c] * r[12];
        }
        cr_vertex_store(vert, row, gap, (double)(end - i), share);
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
        double gap = __builtin_huge_val(), share = 0.0;
        for (int64_t j = first + lane; j < last; j += 64) {
            const uint32_t c = val[j];
            const double* rr = rows_d + (size_t)CR_ND * (c >> 2);
            gap = fmin(gap, rr[0]);
            share += cw[c] * rr[12];
        }
        gap = wave_min(gap);
        share = wave_sum(share);
        if (lane == 0) cr_vertex_store(vert, r, gap, (double)(last - first), share);
    }
}

// one workgroup per ordered pair (ga, gb) of groups; ga <= gb: the pair's rows [lo, hi) of the list sorted by pair, else zeros
__global__ __launch_bounds__(BLOCK) void k_cr_pairs(const uint32_t* __restrict__ pkey, const uint32_t* __restrict__ pval, int n, int n_mesh, const double* __restrict__ thick,
                                                   const int32_t* __restrict__ rows_i, const double* __restrict__ rows_d, double* __restrict__ out)
{
    __shared__ double sm[4];
    const int ga = blockIdx.x / n_mesh, gb = blockIdx.x % n_mesh;
    double* o = out + (size_t)CR_PAIR_REC * blockIdx.x;
    if (ga > gb) {
        if (threadIdx.x < CR_PAIR_REC) o[threadIdx.x] = 0.0;
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
    double s[5] = {0.0, 0.0, 0.0, 0.0, 0.0}, gap = __builtin_huge_val();
    for (int t = first + (int)threadIdx.x; t < last; t += BLOCK) {
        const uint32_t r = pval[t];
        const double* rd = rows_d + (size_t)CR_ND * r;
        const int32_t* ri = rows_i + (size_t)CR_NI * r;
        const double fn = rd[12], sign = ri[3] <= ri[4] ? 1.0 : -1.0;  // the force on the lower-numbered group; a <- b inside one group
        gap = fmin(gap, rd[0]);
        s[0] += fn;
        s[1] += sign * (fn * rd[8]);
        s[2] += sign * (fn * rd[9]);
        s[3] += sign * (fn * rd[10]);
        s[4] += rd[13];
    }
    gap = wave_min(gap);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = gap;
    __syncthreads();
    gap = fmin(fmin(sm[0], sm[1]), fmin(sm[2], sm[3]));
    double v[5];
#pragma unroll
    for (int k = 0; k < 5; k++) v[k] = block_sum(s[k], sm);
    if (threadIdx.x == 0) {
        o[0] = (double)(last - first);
        o[1] = gap;
        o[2] = thick[ga] + thick[gb];
        o[3] = v[0];
        o[4] = v[1];
        o[5] = v[2];
        o[6] = v[3];
        o[7] = v[4];
    }
}

namespace {
const char* const WHO = "contact report";
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
    c.cr_cub_tmp.ensure(tmp);
    MS_CHECK(hipcub::DeviceRadixSort::SortPairs(c.cr_cub_tmp.p, tmp, dk, dv, (int)n, 0, bits, c.stream));  // (stable: equal keys keep the row order)
    *sorted_val = dv.Current();
    return dk.Current();
}
}  // namespace

void contact_report_sizes(Context& c, int64_t* n_rows, int64_t* n_vertices, int32_t* n_groups)
{
    refuse(c);
    ContactReportView V;
    contact_report_view(c, V, true);
    if (n_rows) *n_rows = V.n_keys;
    if (n_vertices) *n_vertices = V.n_v;
    if (n_groups) *n_groups = V.n_mesh;
}

void contact_report_run(Context& c, int set)
{
    refuse(c);
    ContactReportView V;
    contact_report_view(c, V, false);
    Context::ContactReportSet& S = c.cr_set[set];
    const int64_t n = V.n_keys;
    S.n_rows = -1;
    if (4 * n >= (1ll << 31)) throw Error(std::string(WHO) + ": too many rows");
    if ((int64_t)V.n_mesh * V.n_mesh >= (1ll << 31)) throw Error(std::string(WHO) + ": too many groups");
    S.n_v = V.n_v;
    S.n_groups = V.n_mesh;
    if (V.n_v == 0) {  // no collision mesh: nothing to launch
        S.n_rows = 0;
        return;
    }
    c.cr_X.ensure(3 * (size_t)V.n_v);
    contact_report_positions(c, c.cr_X.p);
    if (c.cr_inc_meshes != V.n_mesh) {
        // the triangles of every collision vertex, in triangle order (counting sort); meshes are only ever added
        std::vector<int32_t> table((size_t)V.n_v + 1 + 3 * (size_t)V.n_t, 0);
        for (int32_t v : *V.h_tri) table[(size_t)v + 1]++;
        for (int v = 0; v < V.n_v; v++) table[(size_t)v + 1] += table[(size_t)v];
        std::vector<int32_t> at(table.begin(), table.begin() + V.n_v);
        for (int t = 0; t < V.n_t; t++)
            for (int j = 0; j < 3; j++) table[(size_t)V.n_v + 1 + (size_t)at[(size_t)(*V.h_tri)[3 * (size_t)t + j]]++] = t;
        c.cr_inc.ensure(table.size());
        h2d_staged(c, c.cr_inc.p, table.data(), table.size() * sizeof(int32_t));
        MS_CHECK(hipStreamSynchronize(c.stream));  // (the list is a temporary)
        c.cr_inc_meshes = V.n_mesh;
    }
    CrDev d{V.cv_src, V.cv_mesh, V.tri, V.tri_mesh, V.edge, V.edge_mesh, V.mesh_kind, V.thick, V.k, V.X_rest, V.rb_xloc, c.cr_X.p, V.n_mesh, V.n_v, V.n_t, V.n_e, V.prim_bits};
    S.rows_i.ensure((size_t)CR_NI * std::max<int64_t>(n, 1));
    S.rows_d.ensure((size_t)CR_ND * std::max<int64_t>(n, 1));
    S.vert.ensure((size_t)CR_VERTEX_REC * V.n_v);
    S.pair.ensure((size_t)CR_PAIR_REC * V.n_mesh * V.n_mesh);
    c.cr_stat.ensure(2);
    fill_async(c.stream, c.cr_stat.p, 0, 2 * sizeof(uint32_t));
    const size_t nc = 4 * (size_t)std::max<int64_t>(n, 1);
    c.cr_key.ensure(nc + (size_t)n);  // contributions, then the rows' pair keys
    c.cr_key_alt.ensure(nc + (size_t)n);
    c.cr_val.ensure(nc + (size_t)n);
    c.cr_val_alt.ensure(nc + (size_t)n);
    c.cr_w.ensure(nc);
    if (n > 0)
        hipLaunchKernelGGL(k_cr_rows, dim3(grid_for(n)), dim3(BLOCK), 0, c.stream, d, V.keys, (int)n, S.rows_i.p, S.rows_d.p, c.cr_key.p, c.cr_val.p, c.cr_w.p, c.cr_key.p + nc,
                           c.cr_val.p + nc);
    hipLaunchKernelGGL(k_cr_vertex_init, dim3(grid_for(V.n_v)), dim3(BLOCK), 0, c.stream, d, (const int32_t*)c.cr_inc.p, (const int32_t*)c.cr_inc.p + V.n_v + 1, S.vert.p);
    const uint32_t *pk = c.cr_key.p + nc, *pv = c.cr_val.p + nc;
    if (n > 0) {
        const uint32_t* sv = nullptr;
        const uint32_t* sk = sort_pairs(c, c.cr_key.p, c.cr_key_alt.p, c.cr_val.p, c.cr_val_alt.p, 4 * n, bits_for(V.n_v), &sv);
        hipLaunchKernelGGL(k_cr_vertex_segsum, dim3(grid_for(4 * n)), dim3(BLOCK), 0, c.stream, sk, sv, 4 * n, (const double*)S.rows_d.p, (const double*)c.cr_w.p, V.n_v, S.vert.p, c.cr_stat.p);
        pk = sort_pairs(c, c.cr_key.p + nc, c.cr_key_alt.p + nc, c.cr_val.p + nc, c.cr_val_alt.p + nc, n, bits_for((int64_t)V.n_mesh * V.n_mesh), &pv);
    }
    hipLaunchKernelGGL(k_cr_pairs, dim3((unsigned)(V.n_mesh * V.n_mesh)), dim3(BLOCK), 0, c.stream, pk, pv, (int)n, V.n_mesh, V.thick, (const int32_t*)S.rows_i.p,
                       (const double*)S.rows_d.p, S.pair.p);
    MS_CHECK(hipGetLastError());
    c.cr_stat_valid = true;
    c.n_contact_reports++;
    S.n_rows = n;
}

namespace {
const Context::ContactReportSet& recorded(Context& c, int set)
{
    const Context::ContactReportSet& S = c.cr_set[set];
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

void contact_report_rows(Context& c, int set, int32_t* rows_i, double* rows_d, int64_t* n_rows)
{
    const Context::ContactReportSet& S = recorded(c, set);
    if (n_rows) *n_rows = S.n_rows;
    download(c, rows_i, (const int32_t*)S.rows_i.p, (size_t)CR_NI * S.n_rows);
    download(c, rows_d, (const double*)S.rows_d.p, (size_t)CR_ND * S.n_rows);
}
void contact_report_vertices(Context& c, int set, double* out, int32_t* group, int32_t* source_index, int64_t* n_vertices)
{
    const Context::ContactReportSet& S = recorded(c, set);
    if (n_vertices) *n_vertices = S.n_v;
    download(c, out, (const double*)S.vert.p, (size_t)CR_VERTEX_REC * S.n_v);
    if (group || source_index) {
        ContactReportView V;
        contact_report_view(c, V, true);
        for (int64_t v = 0; v < S.n_v; v++) {
            if (group) group[v] = (*V.h_cv_mesh)[(size_t)v];
            if (source_index) source_index[v] = (*V.h_cv_src)[(size_t)v];
        }
    }
}
void contact_report_pairs(Context& c, int set, double* out, int32_t* n_groups)
{
    const Context::ContactReportSet& S = recorded(c, set);
    if (n_groups) *n_groups = S.n_groups;
    if (S.n_v == 0) return;
    download(c, out, (const double*)S.pair.p, (size_t)CR_PAIR_REC * S.n_groups * S.n_groups);
}
int64_t contact_report_long_rows(Context& c)
{
    if (!c.cr_stat_valid) return 0;
    uint32_t v[2] = {0, 0};
    fetch(c, v, c.cr_stat.p, sizeof(v));
    return (int64_t)v[0];
}

}  // namespace mistark
