// bending_report.hip — opt-in bending report of the two cloth bending potentials (EnergyDiscreteShells, EnergyBendingFlat): per hinge the angles, curvature,
// moment and energy, per node area-weighted curvature and the energy share, per group counts, the sharpest hinge and the energy, at the engine's current
// DoFs. The per-hinge arithmetic and the record layouts are in bending_report.hpp.
//
// A pipeline of its own beside eval(), like the stress readout (stress.hip) and the constraint report (constraint_report.hip): it reads potentials and state
// and writes only the Context::bdr_* buffers (and the set the host mirror keeps).
//   rows   : one lane per hinge, gather_inputs on the potential's own argument block, the record stored field-major (k_bending_rows)
//   nodal  : one key per (hinge, edge endpoint) = its block row, stable radix sort, one sum per row in sorted order; rows beyond BEND_LONG_ROW by the wavefront
//            that holds their head, through wave_sum's fixed tree (k_bending_nodal)
//   groups : the host lists the rows group by group (stable) and cuts every group's list into chunks of BEND_CHUNK rows, whenever the table changes; one
//            workgroup per chunk (k_bending_group_chunks: thread t of 256 takes the rows t, t + 256, ... of the chunk in list order, then block_sum's fixed
//            tree), one workgroup per group folds its chunks in chunk order (k_bending_group_fold)
// A result depends on the order of the lists, on BEND_CHUNK and on BLOCK, never on a grid size, the device or the run. Maxima are exact; the arg-max is the
// smallest list position attaining the maximum. No floating-point atomics anywhere: two reports of one state give the same bits.
#include "kernels_common.hpp"
#include "force_keys.hpp"
#include "energies.hpp"
#include "bending_report.hpp"

namespace mistark {

constexpr int BEND_CHUNK = 2048;    // rows per workgroup: eight per thread
constexpr int BEND_LONG_ROW = 256;  // contributions of a block row beyond which a wavefront sums the row
void cut_chunks(std::vector<int32_t>& chunks, int64_t first, int64_t count, int chunk);  // budget.hip

template <class En>
struct BendKind;
template <>
struct BendKind<E_DiscreteShells>
{
    static constexpr int code = 0, k_binding = 12;  // (the binding the stiffness is read with: its connectivity column is the row's group)
};
template <>
struct BendKind<E_BendingFlat>
{
    static constexpr int code = 1, k_binding = 10;
};

// rec[field][N]: the 16 stores of a wavefront are one coalesced request each; col0 = first column of this potential in a selection of both. thr: per
// group, null: none (the host has checked that every group id of the table is below its length). gcol: connectivity column of the group, -1: one group
template <class En>
__global__ __launch_bounds__(BLOCK) void k_bending_rows(PotArgs a, const double* __restrict__ thr, int gcol, double* __restrict__ rec, int64_t N, int64_t col0)
{
    const int e = blockIdx.x * BLOCK + threadIdx.x;
    if (e >= a.n_elem) return;
    double in[En::Layout::NIN];
    gather_inputs<En>(a, e, in);
    const int g = gcol < 0 ? 0 : a.conn[(size_t)e * a.conn_stride + gcol];
    double r[BEND_REC];
    if constexpr (BendKind<En>::code == 0) shells_bending_record(in, thr ? thr[g] : -1.0, r);
    else flat_bending_record(in, thr ? thr[g] : -1.0, r);
    r[14] = (double)g;
#pragma unroll
    for (int f = 0; f < BEND_REC; f++) rec[(size_t)f * N + col0 + e] = r[f];
}

// column of contribution g in the record buffer: every potential of the selection has two contributing blocks, so the potential whose contributions start
// at g_off has its hinges from column g_off / 2 on
__device__ __forceinline__ int64_t bend_column(const ForceDesc* __restrict__ D, int n_desc, uint32_t g)
{
    int k = 0;
    while (k + 1 < n_desc && g >= D[k + 1].g_off) k++;
    const uint32_t l = g - D[k].g_off;
    return (int64_t)(D[k].g_off / 2u) + (int64_t)(l % (uint32_t)D[k].n_elem);
}
// a[]: sum w kappa, sum w (kappa - kappa_rest), sum E / 2, max |theta1 - rest|, count, sum w; w = a / 2
__device__ __forceinline__ void bend_accumulate(double (&a)[BEND_NODAL], const double* __restrict__ rec, int64_t N, int64_t col)
{
    const double w = 0.5 * rec[5 * N + col], kap = rec[6 * N + col];
    a[0] += w * kap;
    a[1] += w * (kap - rec[7 * N + col]);
    a[2] += 0.5 * (rec[9 * N + col] + rec[10 * N + col]);
    a[3] = fmax(a[3], bend_deviation(rec[col], rec[2 * N + col], rec[15 * N + col]));
    a[4] += 1.0;
    a[5] += w;
}
__device__ __forceinline__ void bend_write_row(double* __restrict__ out, uint32_t row, const double (&a)[BEND_NODAL])
{
    double* o = out + (size_t)BEND_NODAL * row;
    const double w = a[5];
    o[0] = w > 0.0 ? a[0] / w : 0.0;
    o[1] = w > 0.0 ? a[1] / w : 0.0;
    o[2] = a[2];
    o[3] = a[3];
    o[4] = a[4];
    o[5] = w;
}
// Sums over the sorted contributions: one lane per sorted position; the lane at the head of a row's run sums the run in order. Runs beyond BEND_LONG_ROW
// are summed by the whole wavefront their head lies in: lanes stride over the run from its head, then wave_sum's fixed tree (the rule of k_stress_nodal). A
// run belongs to the one wavefront that holds its head, so every row is written once, by one lane. No lane leaves early: the cross-lane steps need all 64.
__global__ __launch_bounds__(BLOCK) void k_bending_nodal(const uint32_t* __restrict__ key, const uint32_t* __restrict__ val, int64_t total, const ForceDesc* __restrict__ D, int n_desc,
                                                        const double* __restrict__ rec, int64_t N, double* __restrict__ out, uint32_t* __restrict__ stat)
{
    const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    const int lane = threadIdx.x & 63;
    uint32_t row = 0;
    int64_t end = 0;
    bool head = false;
    if (i < total) {
        row = key[i];
        head = i == 0 || key[i - 1] != row;
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
    const bool is_long = head && end - i > BEND_LONG_ROW;
    if (head && !is_long) {
        double a[BEND_NODAL] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        for (int64_t j = i; j < end; j++) bend_accumulate(a, rec, N, bend_column(D, n_desc, val[j]));
        bend_write_row(out, row, a);
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
        double a[BEND_NODAL] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        for (int64_t j = first + lane; j < last; j += 64) bend_accumulate(a, rec, N, bend_column(D, n_desc, val[j]));
#pragma unroll
        for (int f = 0; f < BEND_NODAL; f++) a[f] = f == 3 ? wave_max(a[f]) : wave_sum(a[f]);
        if (lane == 0) bend_write_row(out, r, a);
    }
}

// both of a block's (maximum, smallest position attaining it); a thread without a value passes m = -1
__device__ __forceinline__ void bend_block_argmax(double& m, double& pos, double* sm)
{
    const double M = block_max(m, sm);
    const double P = -block_max(m == M && M >= 0.0 ? -pos : -1e300, sm);
    m = M;
    pos = P;
}

// one workgroup per chunk of one group's rows. partial[chunk][10]: the group record's sums over the chunk; 3: the chunk's largest |theta1 - rest| (-1:
// none), 4: the position in `items` of the first row attaining it; 9: sum of a |kappa - kappa_rest|
__global__ __launch_bounds__(BLOCK) void k_bending_group_chunks(const double* __restrict__ rec, int64_t N, int64_t col0, const uint32_t* __restrict__ items,
                                                               const int32_t* __restrict__ chunks, double* __restrict__ partial)
{
    __shared__ double sm[4];
    const int first = chunks[2 * blockIdx.x], count = chunks[2 * blockIdx.x + 1];
    double n = 0.0, deg = 0.0, bey = 0.0, Ee = 0.0, Ed = 0.0, A = 0.0, q2 = 0.0, q1 = 0.0, vmax = -1.0, pos = 0.0;
    for (int t = threadIdx.x; t < count; t += BLOCK) {
        const size_t e = (size_t)col0 + items[(size_t)first + t];
        const double fl = rec[15 * N + e];
        const int flags = (int)fl;
        const double v = bend_deviation(rec[e], rec[2 * N + e], fl);
        const double a = rec[5 * N + e], dk = rec[6 * N + e] - rec[7 * N + e];
        n += 1.0;
        deg += (double)(flags & 1);
        bey += (double)((flags >> 1) & 1);
        Ee += rec[9 * N + e];
        Ed += rec[10 * N + e];
        A += a;
        q2 += a * dk * dk;
        q1 += a * fabs(dk);
        if (v > vmax) {  // (positions ascend: the first row attaining the maximum stays)
            vmax = v;
            pos = (double)(first + t);
        }
    }
    double* o = partial + (size_t)blockIdx.x * BEND_GROUP;
#define MISTARK_BEND_SUM(field, k)              \
    {                                           \
        const double s = block_sum(field, sm);  \
        if (threadIdx.x == 0) o[k] = s;         \
    }
    MISTARK_BEND_SUM(n, 0)
    MISTARK_BEND_SUM(deg, 1)
    MISTARK_BEND_SUM(bey, 2)
    MISTARK_BEND_SUM(Ee, 5)
    MISTARK_BEND_SUM(Ed, 6)
    MISTARK_BEND_SUM(A, 7)
    MISTARK_BEND_SUM(q2, 8)
    MISTARK_BEND_SUM(q1, 9)
#undef MISTARK_BEND_SUM
    bend_block_argmax(vmax, pos, sm);
    if (threadIdx.x == 0) {
        o[3] = vmax;
        o[4] = pos;
    }
}

// out[group][10] = the group's partials [chunk0[group], chunk0[group + 1]) folded in chunk order; a group without chunks: zeros with -1 in slot 4
__global__ __launch_bounds__(BLOCK) void k_bending_group_fold(const double* __restrict__ partial, const int32_t* __restrict__ chunks, const int32_t* __restrict__ chunk0,
                                                             double* __restrict__ out)
{
    __shared__ double sm[4];
    const int c0 = chunk0[blockIdx.x], c1 = chunk0[blockIdx.x + 1];
    double* o = out + (size_t)blockIdx.x * BEND_GROUP;
    double area = 0.0;
#pragma unroll
    for (int k = 0; k < BEND_GROUP; k++) {
        if (k == 3 || k == 4) continue;
        double v = sum_partials(partial + (size_t)c0 * BEND_GROUP + k, c1 - c0, sm, BEND_GROUP);
        if (k == 7) area = v;
        if (k == 9) v = area > 0.0 ? v / area : 0.0;
        if (threadIdx.x == 0) o[k] = v;
    }
    double vmax = -1.0, pos = 0.0;
    for (int i = threadIdx.x; i < c1 - c0; i += BLOCK) {
        const double* p = partial + (size_t)(c0 + i) * BEND_GROUP;
        if (p[3] > vmax) {  // (chunks ascend in list order)
            vmax = p[3];
            pos = p[4];
        }
    }
    bend_block_argmax(vmax, pos, sm);
    if (threadIdx.x == 0) {
        const bool any = c1 > c0 && vmax >= 0.0;
        o[3] = any ? vmax : 0.0;
        o[4] = any ? pos - (double)chunks[2 * c0] : -1.0;  // position in the group's own list
    }
}

namespace {
struct KindInfo
{
    int code = -1, k_binding = 0;
};
bool kind_of(const Potential& P, KindInfo& k)
{
    if (P.kind == KIND_CUSTOM) return false;
    if (P.name == E_DiscreteShells::name) k = {BendKind<E_DiscreteShells>::code, BendKind<E_DiscreteShells>::k_binding};
    else if (P.name == E_BendingFlat::name) k = {BendKind<E_BendingFlat>::code, BendKind<E_BendingFlat>::k_binding};
    else return false;
    return true;
}
// connectivity column of the group: the one the stiffness is read with (-1: a global stiffness, every row is of group 0)
int group_col(const Potential& P, const KindInfo& K) { return P.args.conn_col[K.k_binding]; }

struct Selection
{
    std::vector<int> pots;  // selected potentials with rows, in the caller's order
    std::vector<ForceDesc> descs;
    std::vector<int64_t> col0;
    int64_t N = 0, total = 0;  // rows, contributions (row, edge endpoint)
};
// refusals, prepare(), the selection and its layout in the record buffer
Selection select(Context& c, const int32_t* pots, int32_t n, const char* who)
{
    if (n < 0) throw Error(std::string(who) + ": bad potential list");
    const std::vector<int> ids = select_potentials(c, pots, n, false, who);
    Selection S;
    for (int p : ids) {
        const Potential& P = c.pots[(size_t)p];
        KindInfo K;
        if (!kind_of(P, K))
            throw Error(std::string(who) + ": potential '" + P.name + "' has no bending report (only EnergyDiscreteShells and EnergyBendingFlat have one)");
        if (P.n_elem <= 0) continue;
        if (P.args.elem_list || P.args.e_count != P.n_elem) throw Error(std::string(who) + ": single-rank accessor");
        ForceDesc d{};
        d.conn = P.args.conn;
        d.stride = P.conn_stride;
        d.n_elem = P.n_elem;
        d.NB = 2;  // (the two edge endpoints: local blocks 0 and 1)
        d.g_off = (uint32_t)S.total;
        for (int b = 0; b < 2; b++) {
            d.dof_col[b] = P.args.dof_col[b];
            d.dof_row_off[b] = P.args.dof_row_off[b];
        }
        S.pots.push_back(p);
        S.descs.push_back(d);
        S.col0.push_back(S.N);
        S.N += P.n_elem;
        S.total += 2 * (int64_t)P.n_elem;
    }
    if (S.total >= (1ll << 31)) throw Error(std::string(who) + ": too many contributions");
    return S;
}
// n_groups must exceed every group id of the table; thresholds are finite and not negative
void check_groups(const Potential& P, const KindInfo& K, const double* threshold, int32_t n_groups, const char* who)
{
    if (n_groups < 0) throw Error(std::string(who) + ": negative group count");
    const int gc = group_col(P, K);
    if (P.n_elem > 0 && gc >= 0) {
        if (P.conn_ext || P.conn_stride <= gc || P.conn_host.size() != (size_t)P.n_elem * P.conn_stride)
            throw Error(std::string(who) + ": the table of '" + P.name + "' has no host connectivity with a group column");
        for (int e = 0; e < P.n_elem; e++) {
            const int g = P.conn_host[(size_t)e * P.conn_stride + gc];
            if (g < 0 || g >= n_groups)
                throw Error(std::string(who) + ": row " + std::to_string(e) + " of '" + P.name + "' names group " + std::to_string(g) + ", n_groups is " + std::to_string(n_groups));
        }
    } else if (P.n_elem > 0 && n_groups < 1) {
        throw Error(std::string(who) + ": the rows of '" + P.name + "' are of group 0, n_groups is " + std::to_string(n_groups));
    }
    if (threshold)
        for (int32_t g = 0; g < n_groups; g++)
            if (!(threshold[g] >= 0.0) || !std::isfinite(threshold[g]))
                throw Error(std::string(who) + ": the threshold of group " + std::to_string(g) + " is negative or not finite");
}
int group_of(const Potential& P, int gc, int e) { return gc < 0 ? 0 : P.conn_host[(size_t)e * P.conn_stride + gc]; }

template <class En>
void launch_rows(Context& c, const Potential& P, const double* thr, int gcol, double* rec, int64_t N, int64_t col0)
{
    hipLaunchKernelGGL((k_bending_rows<En>), dim3(grid_for(P.n_elem)), dim3(BLOCK), 0, c.stream, P.args, thr, gcol, rec, N, col0);
}
// stage 1: rec[16][S.N]. threshold: [n_groups] or null, shared by the potentials of the selection
void rows_stage(Context& c, const Selection& S, const double* threshold, int32_t n_groups, double* rec)
{
    const double* thr = nullptr;
    if (threshold && n_groups > 0) {
        c.bdr_thr.ensure((size_t)n_groups);
        h2d_small(c, c.bdr_thr.p, threshold, (size_t)n_groups * sizeof(double));  // (the caller's thresholds may be a temporary)
        thr = c.bdr_thr.p;
    }
    for (size_t k = 0; k < S.pots.size(); k++) {
        const Potential& P = c.pots[(size_t)S.pots[k]];
        KindInfo K;
        kind_of(P, K);
        if (K.code == 0) launch_rows<E_DiscreteShells>(c, P, thr, group_col(P, K), rec, S.N, S.col0[k]);
        else launch_rows<E_BendingFlat>(c, P, thr, group_col(P, K), rec, S.N, S.col0[k]);
    }
    MS_CHECK(hipGetLastError());
    c.n_bending_reports++;
}
// stage 2: out[nbr][6] from the records of stage 1
void nodal_stage(Context& c, const Selection& S, const double* rec, double* out)
{
    const int64_t n = S.total;
    c.bdr_key.ensure((size_t)n);
    c.bdr_key_alt.ensure((size_t)n);
    c.bdr_val.ensure((size_t)n);
    c.bdr_val_alt.ensure((size_t)n);
    c.bdr_stat.ensure(2);
    c.bdr_desc.ensure(S.descs.size() * sizeof(ForceDesc));
    h2d_small(c, c.bdr_desc.p, S.descs.data(), S.descs.size() * sizeof(ForceDesc));
    hipLaunchKernelGGL(k_force_keys, dim3(grid_for(n)), dim3(BLOCK), 0, c.stream, (const ForceDesc*)c.bdr_desc.p, (int)S.descs.size(), n, c.bdr_key.p, c.bdr_val.p);
    int bits = 1;
    while (bits < 32 && (1ll << bits) <= c.nbr) bits++;
    size_t tmp = 0;
    hipcub::DoubleBuffer<uint32_t> dk(c.bdr_key.p, c.bdr_key_alt.p), dv(c.bdr_val.p, c.bdr_val_alt.p);
    MS_CHECK(hipcub::DeviceRadixSort::SortPairs(nullptr, tmp, dk, dv, (int)n, 0, bits, c.stream));
    c.bdr_cub_tmp.ensure(tmp);
    MS_CHECK(hipcub::DeviceRadixSort::SortPairs(c.bdr_cub_tmp.p, tmp, dk, dv, (int)n, 0, bits, c.stream));  // (stable: equal rows keep the contribution order)
    {
        FillQueue fills(c.stream);
        fills.add(out, 0, (size_t)BEND_NODAL * c.nbr * sizeof(double));  // (rows nobody touches are six zeros)
        fills.add(c.bdr_stat.p, 0, 2 * sizeof(uint32_t));
    }
    hipLaunchKernelGGL(k_bending_nodal, dim3(grid_for(n)), dim3(BLOCK), 0, c.stream, (const uint32_t*)dk.Current(), (const uint32_t*)dv.Current(), n, (const ForceDesc*)c.bdr_desc.p,
                       (int)S.descs.size(), rec, S.N, out, c.bdr_stat.p);
    MS_CHECK(hipGetLastError());
    c.bdr_stat_valid = true;
}
// stage 3: groups[n_groups][10] of the rows of potential `pot` (which has rows) in columns col0.. of rec
void groups_stage(Context& c, int pot, const Potential& P, const KindInfo& K, int32_t n_groups, const double* rec, int64_t N, int64_t col0, double* groups)
{
    Context::BendingPlan& plan = c.bdr_plans[pot];
    if (plan.conn_version != P.conn_version || plan.n_elem != P.n_elem || plan.n_groups != n_groups) {
        // the rows group by group, list order kept inside a group (counting sort), every group's list cut into chunks
        plan.n_elem = -1;
        const int gc = group_col(P, K);
        std::vector<int64_t> start((size_t)n_groups + 1, 0);
        for (int e = 0; e < P.n_elem; e++) start[(size_t)group_of(P, gc, e) + 1]++;
        for (int g = 0; g < n_groups; g++) start[(size_t)g + 1] += start[(size_t)g];
        std::vector<uint32_t> items((size_t)P.n_elem);
        std::vector<int64_t> at(start.begin(), start.end() - 1);
        for (int e = 0; e < P.n_elem; e++) items[(size_t)at[(size_t)group_of(P, gc, e)]++] = (uint32_t)e;
        std::vector<int32_t> table, chunk0;
        for (int g = 0; g < n_groups; g++) {
            chunk0.push_back((int32_t)(table.size() / 2));
            cut_chunks(table, start[(size_t)g], start[(size_t)g + 1] - start[(size_t)g], BEND_CHUNK);
        }
        const int64_t n_chunks = (int64_t)table.size() / 2;
        chunk0.push_back((int32_t)n_chunks);
        table.insert(table.end(), chunk0.begin(), chunk0.end());
        plan.items.ensure(items.size());
        plan.chunks.ensure(table.size());
        h2d_staged(c, plan.items.p, items.data(), items.size() * sizeof(uint32_t));
        h2d_staged(c, plan.chunks.p, table.data(), table.size() * sizeof(int32_t));
        MS_CHECK(hipStreamSynchronize(c.stream));  // (the two lists are temporaries)
        plan.conn_version = P.conn_version;
        plan.n_elem = P.n_elem;
        plan.n_groups = n_groups;
        plan.n_chunks = n_chunks;
    }
    c.bdr_partial.ensure((size_t)BEND_GROUP * plan.n_chunks);
    hipLaunchKernelGGL(k_bending_group_chunks, dim3((unsigned)plan.n_chunks), dim3(BLOCK), 0, c.stream, rec, N, col0, (const uint32_t*)plan.items.p, (const int32_t*)plan.chunks.p,
                       c.bdr_partial.p);
    hipLaunchKernelGGL(k_bending_group_fold, dim3((unsigned)n_groups), dim3(BLOCK), 0, c.stream, (const double*)c.bdr_partial.p, (const int32_t*)plan.chunks.p,
                       (const int32_t*)plan.chunks.p + 2 * plan.n_chunks, groups);
    MS_CHECK(hipGetLastError());
    c.n_bending_chunks = plan.n_chunks;
}
// columns [col0, col0 + n) of the field-major records -> row-major for the caller
void download_rows(Context& c, const double* rec, int64_t N, int64_t col0, int64_t n, double* out)
{
    if (!out || n <= 0) return;
    std::vector<double> tmp((size_t)BEND_REC * N);
    MS_CHECK(hipMemcpyAsync(tmp.data(), rec, tmp.size() * sizeof(double), hipMemcpyDeviceToHost, c.stream));
    MS_CHECK(hipStreamSynchronize(c.stream));
    for (int64_t e = 0; e < n; e++)
        for (int f = 0; f < BEND_REC; f++) out[(size_t)e * BEND_REC + f] = tmp[(size_t)f * N + col0 + e];
}
// the group records of a potential with n_rows rows (0: nothing was launched, every declared group is empty)
void download_groups(Context& c, const double* groups, int64_t n_rows, int32_t n_groups, double* out)
{
    if (!out || n_groups <= 0) return;
    const size_t n = (size_t)BEND_GROUP * n_groups;
    if (n_rows == 0) {
        std::fill(out, out + n, 0.0);
        for (int g = 0; g < n_groups; g++) out[(size_t)g * BEND_GROUP + 4] = -1.0;
        return;
    }
    MS_CHECK(hipMemcpyAsync(out, groups, n * sizeof(double), hipMemcpyDeviceToHost, c.stream));
    MS_CHECK(hipStreamSynchronize(c.stream));
}
}  // namespace

void bending_rows_host(Context& c, int pot, const double* threshold, int32_t n_groups, double* out, int64_t* n_rows, int32_t* kind)
{
    const char* who = "mistark_potential_bending_report";
    const int32_t id = pot;
    const Selection S = select(c, &id, 1, who);
    const Potential& P = c.pots[(size_t)pot];
    KindInfo K;
    kind_of(P, K);
    if (threshold || n_groups != 0) check_groups(P, K, threshold, n_groups, who);
    if (n_rows) *n_rows = P.n_elem;
    if (kind) *kind = K.code;
    if (!out || S.N == 0) return;  // (an empty table launches nothing; a null output: a size query)
    c.bdr_rec.ensure((size_t)BEND_REC * S.N);
    rows_stage(c, S, threshold, n_groups, c.bdr_rec.p);
    download_rows(c, c.bdr_rec.p, S.N, 0, S.N, out);
}

void bending_nodal_host(Context& c, const int32_t* pots, int32_t n, double* out_host)
{
    if (!out_host) throw Error("mistark_nodal_bending: null output");
    const Selection S = select(c, pots, n, "mistark_nodal_bending");
    if (S.total == 0) {
        std::fill(out_host, out_host + (size_t)BEND_NODAL * c.nbr, 0.0);
        return;
    }
    c.bdr_rec.ensure((size_t)BEND_REC * S.N);
    c.bdr_out.ensure((size_t)BEND_NODAL * c.nbr);
    rows_stage(c, S, nullptr, 0, c.bdr_rec.p);
    nodal_stage(c, S, c.bdr_rec.p, c.bdr_out.p);
    MS_CHECK(hipMemcpyAsync(out_host, c.bdr_out.p, (size_t)BEND_NODAL * c.nbr * sizeof(double), hipMemcpyDeviceToHost, c.stream));
    MS_CHECK(hipStreamSynchronize(c.stream));
}

void bending_groups_host(Context& c, int pot, const double* threshold, int32_t n_groups, double* out)
{
    const char* who = "mistark_bending_group_report";
    const int32_t id = pot;
    const Selection S = select(c, &id, 1, who);
    const Potential& P = c.pots[(size_t)pot];
    KindInfo K;
    kind_of(P, K);
    check_groups(P, K, threshold, n_groups, who);
    if (n_groups == 0 || !out) return;
    if (S.N > 0) {
        c.bdr_rec.ensure((size_t)BEND_REC * S.N);
        c.bdr_groups.ensure((size_t)BEND_GROUP * n_groups);
        rows_stage(c, S, threshold, n_groups, c.bdr_rec.p);
        groups_stage(c, pot, P, K, n_groups, c.bdr_rec.p, S.N, 0, c.bdr_groups.p);
    }
    download_groups(c, c.bdr_groups.p, S.N, n_groups, out);
}

int64_t bending_long_rows(Context& c)
{
    if (!c.bdr_stat_valid) return 0;
    uint32_t v[2] = {0, 0};
    fetch(c, v, c.bdr_stat.p, sizeof(v));
    return (int64_t)v[0];
}

// the host mirror's recording inside a time step: rows, nodal records and groups of the registered bending potentials (ids, -1: not registered) into
// Context::bdr_slot, kept on the device until they are asked for
void bending_record_step(Context& c, int pot_complete, int pot_flat, const double* threshold, int32_t n_groups)
{
    const char* who = "bending report";
    Context::BendingSlot& s = c.bdr_slot;
    s.N = -1;
    std::vector<int32_t> ids;
    if (pot_complete >= 0) ids.push_back(pot_complete);
    if (pot_flat >= 0) ids.push_back(pot_flat);
    const Selection S = select(c, ids.data(), (int32_t)ids.size(), who);
    for (int k = 0; k < 2; k++) s.n_rows[k] = s.col0[k] = 0;
    for (int p : ids) {
        KindInfo K;
        kind_of(c.pots[(size_t)p], K);
        check_groups(c.pots[(size_t)p], K, threshold, n_groups, who);
    }
    s.nbr = c.nbr;
    s.n_groups = n_groups;
    if (S.N > 0) {
        s.rec.ensure((size_t)BEND_REC * S.N);
        s.nodal.ensure((size_t)BEND_NODAL * c.nbr);
        rows_stage(c, S, threshold, n_groups, s.rec.p);
        nodal_stage(c, S, s.rec.p, s.nodal.p);
        for (size_t k = 0; k < S.pots.size(); k++) {
            const Potential& P = c.pots[(size_t)S.pots[k]];
            KindInfo K;
            kind_of(P, K);
            s.n_rows[K.code] = P.n_elem;
            s.col0[K.code] = S.col0[k];
            if (n_groups > 0) {
                s.groups[K.code].ensure((size_t)BEND_GROUP * n_groups);
                groups_stage(c, S.pots[k], P, K, n_groups, s.rec.p, S.N, S.col0[k], s.groups[K.code].p);
            }
        }
    }
    s.N = S.N;
}
void bending_fetch_kind(Context& c, int kind, double* rows, double* groups, int64_t* n_rows, int32_t* n_groups)
{
    const Context::BendingSlot& s = c.bdr_slot;
    if (kind < 0 || kind > 1 || s.N < 0) throw Error("bending report: nothing recorded for kind " + std::to_string(kind));
    if (n_rows) *n_rows = s.n_rows[kind];
    if (n_groups) *n_groups = s.n_groups;
    download_rows(c, s.rec.p, s.N, s.col0[kind], s.n_rows[kind], rows);
    download_groups(c, s.groups[kind].p, s.n_rows[kind], s.n_groups, groups);
}
void bending_fetch_nodal(Context& c, double* out, int64_t n_rows)
{
    const Context::BendingSlot& s = c.bdr_slot;
    if (s.N < 0) throw Error("bending report: nothing recorded");
    if (n_rows != s.nbr) throw Error("bending report: the recorded array has " + std::to_string(s.nbr) + " rows, the caller asks for " + std::to_string(n_rows));
    if (s.N == 0) {
        std::fill(out, out + (size_t)BEND_NODAL * n_rows, 0.0);
        return;
    }
    MS_CHECK(hipMemcpyAsync(out, s.nodal.p, (size_t)BEND_NODAL * n_rows * sizeof(double), hipMemcpyDeviceToHost, c.stream));
    MS_CHECK(hipStreamSynchronize(c.stream));
}

}  // namespace mistark
