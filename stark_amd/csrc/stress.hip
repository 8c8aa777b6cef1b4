// stress.hip — opt-in stress and strain readout of the strain potentials (tets, membranes, rods): per-element records and rest-measure-weighted nodal
// averages at the engine's current DoFs. The constitutive arithmetic and the record layout are in stress.hpp.
//
// A pipeline of its own beside eval(), like the force readout (forces.hip): it reads potentials and state and writes only the Context::sr_* buffers (and
// the slots the host mirror keeps).
//   1. element records : one lane per element, gather_inputs on the potential's own argument block, the record stored field-major (k_stress_elements)
//   2. nodal averages  : one key per (element, local block) = its block row, stable radix sort, one weighted sum per row in sorted order (k_stress_nodal)
// No floating-point atomics anywhere: two readouts of one state give the same bits.
#include "kernels_common.hpp"
#include "force_keys.hpp"
#include "energies.hpp"
#include "stress.hpp"

namespace mistark {

// rec[field][N]: the 16 stores of a wavefront are one coalesced request each; col0 = first column of this potential in a selection of several
template <class En, int KIND, bool FULL>
__global__ __launch_bounds__(BLOCK) void k_stress_elements(PotArgs a, double* __restrict__ rec, int64_t N, int64_t col0)
{
    const int e = blockIdx.x * BLOCK + threadIdx.x;
    if (e >= a.n_elem) return;
    double in[En::Layout::NIN];
    gather_inputs<En>(a, e, in);
    double r[STRESS_REC];
    if constexpr (KIND == 0) tet_stress<FULL>(in, r);
    else if constexpr (KIND == 1) tri_stress<FULL>(in, r);
    else seg_stress<FULL>(in, r);
#pragma unroll
    for (int f = 0; f < STRESS_REC; f++) rec[(size_t)f * N + col0 + e] = r[f];
}

// column of contribution g in the record buffer: the potentials of one nodal readout are of one kind, so all have NB blocks and the potential whose
// contributions start at g_off has its elements from column g_off / NB on
__device__ __forceinline__ int64_t stress_column(const ForceDesc* __restrict__ D, int n_desc, uint32_t g)
{
    int k = 0;
    while (k + 1 < n_desc && g >= D[k + 1].g_off) k++;
    const uint32_t l = g - D[k].g_off;
    return (int64_t)(D[k].g_off / (uint32_t)D[k].NB) + (int64_t)(l % (uint32_t)D[k].n_elem);
}
__device__ __forceinline__ void stress_accumulate(double (&a)[STRESS_NODAL], const double* __restrict__ rec, int64_t N, int64_t col)
{
    const double m = rec[14 * N + col];
#pragma unroll
    for (int f = 0; f < STRESS_NODAL - 1; f++) a[f] += m * rec[f * N + col];
    a[STRESS_NODAL - 1] += m;
}
__device__ __forceinline__ void stress_write_row(double* __restrict__ out, uint32_t row, const double (&a)[STRESS_NODAL])
{
    double* o = out + (size_t)STRESS_NODAL * row;
    const double w = a[STRESS_NODAL - 1];
#pragma unroll
    for (int f = 0; f < STRESS_NODAL - 1; f++) o[f] = w > 0.0 ? a[f] / w : 0.0;
    o[STRESS_NODAL - 1] = w;
}
// Weighted sums over the sorted contributions: one lane per sorted position; the lane at the head of a row's run sums the run in order,
// out[row] = (sum m field_f / sum m for f = 0..8, sum m). Runs beyond STRESS_LONG_ROW are summed by the whole wavefront their head lies in: lanes stride
// over the run from its head, then wave_sum's fixed tree (the rule of k_force_segsum). A run belongs to the one wavefront that holds its head, so every
// row is written once, by one lane. No lane leaves early: the cross-lane steps need all 64.
constexpr int STRESS_LONG_ROW = 256;
__global__ __launch_bounds__(BLOCK) void k_stress_nodal(const uint32_t* __restrict__ key, const uint32_t* __restrict__ val, int64_t total, const ForceDesc* __restrict__ D, int n_desc,
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
    const bool is_long = head && end - i > STRESS_LONG_ROW;
    if (head && !is_long) {
        double a[STRESS_NODAL] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        for (int64_t j = i; j < end; j++) stress_accumulate(a, rec, N, stress_column(D, n_desc, val[j]));
        stress_write_row(out, row, a);
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
        double a[STRESS_NODAL] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        for (int64_t j = first + lane; j < last; j += 64) stress_accumulate(a, rec, N, stress_column(D, n_desc, val[j]));
#pragma unroll
        for (int f = 0; f < STRESS_NODAL; f++) a[f] = wave_sum(a[f]);
        if (lane == 0) stress_write_row(out, r, a);
    }
}

namespace {
struct StressKind
{
    int kind;  // 0 tet, 1 triangle, 2 segment
    bool full;
};
bool stress_kind_of(const Potential& P, StressKind& k)
{
    if (P.kind == KIND_CUSTOM) return false;
    if (P.name == E_TetStrain::name) k = {0, true};
    else if (P.name == E_TetStrainEO::name) k = {0, false};
    else if (P.name == E_TriangleStrain::name) k = {1, true};
    else if (P.name == E_TriangleStrainEO::name) k = {1, false};
    else if (P.name == E_SegmentStrain::name) k = {2, true};
    else if (P.name == E_SegmentStrainEO::name) k = {2, false};
    else return false;
    return true;
}
struct Selection
{
    std::vector<int> pots;  // selected potentials with elements, in the caller's order
    std::vector<ForceDesc> descs;
    std::vector<int64_t> col0;
    int64_t n_elem = 0, total = 0;  // elements, contributions (element, block)
    int kind = -1;
};
// refusals, prepare(), the selection and its layout in the record buffer
Selection select(Context& c, const int32_t* pots, int32_t n, const char* who)
{
    if (c.dry) throw Error(std::string(who) + ": registration-only context (mistark_create_dry): nothing can be evaluated");
    if (c.world > 1) throw Error(std::string(who) + ": single-rank accessor (a sharded context holds the elements touching its rows)");
    if (n < 0 || (n > 0 && !pots)) throw Error(std::string(who) + ": bad potential list");
    std::vector<char> seen(c.pots.size(), 0);
    Selection S;
    for (int32_t k = 0; k < n; k++) {
        const int p = pots[k];
        if (p < 0 || p >= (int)c.pots.size()) throw Error(std::string(who) + ": bad potential id " + std::to_string(p));
        const Potential& P = c.pots[(size_t)p];
        if (seen[(size_t)p]) throw Error(std::string(who) + ": potential '" + P.name + "' is listed twice");
        seen[(size_t)p] = 1;
        StressKind sk{};
        if (!stress_kind_of(P, sk))
            throw Error(std::string(who) + ": potential '" + P.name + "' has no stress readout (only the tet, triangle and segment strain potentials have one)");
        if (S.kind >= 0 && sk.kind != S.kind)
            throw Error(std::string(who) + ": the list mixes element kinds ('" + P.name + "' beside '" + c.pots[(size_t)pots[0]].name +
                        "'): the weights of a nodal average would have different units");
        S.kind = sk.kind;
    }
    prepare(c);
    for (int32_t k = 0; k < n; k++) {
        const Potential& P = c.pots[(size_t)pots[k]];
        if (P.n_elem <= 0) continue;
        if (P.args.elem_list || P.args.e_count != P.n_elem) throw Error(std::string(who) + ": single-rank accessor");
        ForceDesc d{};
        d.conn = P.args.conn;
        d.stride = P.conn_stride;
        d.n_elem = P.n_elem;
        d.NB = P.NB;
        d.g_off = (uint32_t)S.total;
        for (int b = 0; b < P.NB; b++) {
            d.dof_col[b] = P.args.dof_col[b];
            d.dof_row_off[b] = P.args.dof_row_off[b];
        }
        S.pots.push_back(pots[k]);
        S.descs.push_back(d);
        S.col0.push_back(S.n_elem);
        S.n_elem += P.n_elem;
        S.total += (int64_t)P.NB * P.n_elem;
    }
    if (S.total >= (1ll << 31)) throw Error(std::string(who) + ": too many contributions");
    return S;
}
template <class En, int KIND, bool FULL>
void launch_elements(Context& c, const Potential& P, double* rec, int64_t N, int64_t col0)
{
    hipLaunchKernelGGL((k_stress_elements<En, KIND, FULL>), dim3(grid_for(P.n_elem)), dim3(BLOCK), 0, c.stream, P.args, rec, N, col0);
}
// stage 1: rec[16][S.n_elem]
void element_stage(Context& c, const Selection& S, double* rec)
{
    for (size_t k = 0; k < S.pots.size(); k++) {
        const Potential& P = c.pots[(size_t)S.pots[k]];
        StressKind sk{};
        stress_kind_of(P, sk);
        const int64_t N = S.n_elem, c0 = S.col0[k];
        if (sk.kind == 0 && sk.full) launch_elements<E_TetStrain, 0, true>(c, P, rec, N, c0);
        else if (sk.kind == 0) launch_elements<E_TetStrainEO, 0, false>(c, P, rec, N, c0);
        else if (sk.kind == 1 && sk.full) launch_elements<E_TriangleStrain, 1, true>(c, P, rec, N, c0);
        else if (sk.kind == 1) launch_elements<E_TriangleStrainEO, 1, false>(c, P, rec, N, c0);
        else if (sk.full) launch_elements<E_SegmentStrain, 2, true>(c, P, rec, N, c0);
        else launch_elements<E_SegmentStrainEO, 2, false>(c, P, rec, N, c0);
    }
    MS_CHECK(hipGetLastError());
    c.n_stress_readouts++;
}
// stage 2: out[nbr][10] from the records of stage 1
void nodal_stage(Context& c, const Selection& S, const double* rec, double* out)
{
    const int64_t n = S.total;
    c.sr_key.ensure((size_t)n);
    c.sr_key_alt.ensure((size_t)n);
    c.sr_val.ensure((size_t)n);
    c.sr_val_alt.ensure((size_t)n);
    c.sr_stat.ensure(2);
    c.sr_desc.ensure(S.descs.size() * sizeof(ForceDesc));
    h2d_small(c, c.sr_desc.p, S.descs.data(), S.descs.size() * sizeof(ForceDesc));
    hipLaunchKernelGGL(k_force_keys, dim3(grid_for(n)), dim3(BLOCK), 0, c.stream, (const ForceDesc*)c.sr_desc.p, (int)S.descs.size(), n, c.sr_key.p, c.sr_val.p);
    int bits = 1;
    while (bits < 32 && (1ll << bits) <= c.nbr) bits++;
    size_t tmp = 0;
    hipcub::DoubleBuffer<uint32_t> dk(c.sr_key.p, c.sr_key_alt.p), dv(c.sr_val.p, c.sr_val_alt.p);
    MS_CHECK(hipcub::DeviceRadixSort::SortPairs(nullptr, tmp, dk, dv, (int)n, 0, bits, c.stream));
    c.sr_cub_tmp.ensure(tmp);
    MS_CHECK(hipcub::DeviceRadixSort::SortPairs(c.sr_cub_tmp.p, tmp, dk, dv, (int)n, 0, bits, c.stream));  // (stable: equal rows keep the contribution order)
    {
        FillQueue fills(c.stream);
        fills.add(out, 0, (size_t)STRESS_NODAL * c.nbr * sizeof(double));  // (rows nobody touches are ten zeros)
        fills.add(c.sr_stat.p, 0, 2 * sizeof(uint32_t));
    }
    hipLaunchKernelGGL(k_stress_nodal, dim3(grid_for(n)), dim3(BLOCK), 0, c.stream, (const uint32_t*)dk.Current(), (const uint32_t*)dv.Current(), n, (const ForceDesc*)c.sr_desc.p,
                       (int)S.descs.size(), rec, S.n_elem, out, c.sr_stat.p);
    MS_CHECK(hipGetLastError());
    c.sr_stat_valid = true;
}
// field-major on the device -> element-major for the caller
void download_records(Context& c, const double* rec, int64_t N, double* out)
{
    std::vector<double> tmp((size_t)STRESS_REC * N);
    MS_CHECK(hipMemcpyAsync(tmp.data(), rec, tmp.size() * sizeof(double), hipMemcpyDeviceToHost, c.stream));
    MS_CHECK(hipStreamSynchronize(c.stream));
    for (int64_t e = 0; e < N; e++)
        for (int f = 0; f < STRESS_REC; f++) out[(size_t)e * STRESS_REC + f] = tmp[(size_t)f * N + e];
}
}  // namespace

void stress_elements_host(Context& c, int pot, double* out, int64_t* n_elem, int32_t* kind)
{
    const int32_t id = pot;
    const Selection S = select(c, &id, 1, "mistark_potential_element_stress");
    if (n_elem) *n_elem = c.pots[(size_t)pot].n_elem;
    if (kind) *kind = S.kind;
    if (!out || S.n_elem == 0) return;
    c.sr_rec.ensure((size_t)STRESS_REC * S.n_elem);
    element_stage(c, S, c.sr_rec.p);
    download_records(c, c.sr_rec.p, S.n_elem, out);
}

void stress_nodal_host(Context& c, const int32_t* pots, int32_t n, double* out_host)
{
    if (!out_host) throw Error("mistark_nodal_stress: null output");
    const Selection S = select(c, pots, n, "mistark_nodal_stress");
    if (S.total == 0) {
        std::fill(out_host, out_host + (size_t)STRESS_NODAL * c.nbr, 0.0);
        return;
    }
    c.sr_rec.ensure((size_t)STRESS_REC * S.n_elem);
    c.sr_out.ensure((size_t)STRESS_NODAL * c.nbr);
    element_stage(c, S, c.sr_rec.p);
    nodal_stage(c, S, c.sr_rec.p, c.sr_out.p);
    MS_CHECK(hipMemcpyAsync(out_host, c.sr_out.p, (size_t)STRESS_NODAL * c.nbr * sizeof(double), hipMemcpyDeviceToHost, c.stream));
    MS_CHECK(hipStreamSynchronize(c.stream));
}

int64_t stress_long_rows(Context& c)
{
    if (!c.sr_stat_valid) return 0;
    uint32_t v[2] = {0, 0};
    fetch(c, v, c.sr_stat.p, sizeof(v));
    return (int64_t)v[0];
}

// the host mirror's recording inside a time step: results stay on the device until they are asked for
void stress_record_kind(Context& c, int kind)
{
    if (kind < 0 || kind > 2) throw Error("stress readout: bad kind " + std::to_string(kind));
    Context::StressSlot& s = c.stress_slots[kind];
    s.n_elem = -1;
    std::vector<int32_t> ids;
    for (int p = 0; p < (int)c.pots.size(); p++) {
        StressKind sk{};
        if (stress_kind_of(c.pots[(size_t)p], sk) && sk.kind == kind) ids.push_back(p);
    }
    const Selection S = select(c, ids.data(), (int32_t)ids.size(), "stress readout");
    s.nbr = c.nbr;
    if (S.total > 0) {
        s.rec.ensure((size_t)STRESS_REC * S.n_elem);
        s.nodal.ensure((size_t)STRESS_NODAL * c.nbr);
        element_stage(c, S, s.rec.p);
        nodal_stage(c, S, s.rec.p, s.nodal.p);
    }
    s.n_elem = S.n_elem;
}
void stress_fetch_elements(Context& c, int kind, double* out, int64_t* n_elem)
{
    if (kind < 0 || kind > 2 || c.stress_slots[kind].n_elem < 0) throw Error("stress readout: nothing recorded for kind " + std::to_string(kind));
    const Context::StressSlot& s = c.stress_slots[kind];
    if (n_elem) *n_elem = s.n_elem;
    if (out && s.n_elem > 0) download_records(c, s.rec.p, s.n_elem, out);
}
void stress_fetch_nodal(Context& c, int kind, double* out, int64_t n_rows)
{
    if (kind < 0 || kind > 2 || c.stress_slots[kind].n_elem < 0) throw Error("stress readout: nothing recorded for kind " + std::to_string(kind));
    const Context::StressSlot& s = c.stress_slots[kind];
    if (n_rows != s.nbr) throw Error("stress readout: the recorded array has " + std::to_string(s.nbr) + " rows, the caller asks for " + std::to_string(n_rows));
    if (s.n_elem == 0) {
        std::fill(out, out + (size_t)STRESS_NODAL * n_rows, 0.0);
        return;
    }
    MS_CHECK(hipMemcpyAsync(out, s.nodal.p, (size_t)STRESS_NODAL * n_rows * sizeof(double), hipMemcpyDeviceToHost, c.stream));
    MS_CHECK(hipStreamSynchronize(c.stream));
}

}  // namespace mistark
