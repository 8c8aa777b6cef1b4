// forces.hip — per-potential force readout: element, nodal and resultant forces of any subset of the registered potentials.
//
//   f = -scale * sum over the selected potentials of dE/du at the engine's current DoFs (scale = 1/dt: Newtons, with STARK's velocity DoFs)
//
// A pipeline of its own beside eval(): it reads potentials and state and writes only the Context::fr_* buffers (and the slots the host mirror keeps).
//   1. element forces : the generic hyper-dual kernel of every selected potential, node gradients to the readout pool (launch_force_elements)
//   2. nodal forces   : one key per (element, local block) = its block row, stable radix sort, segmented sum in sorted order (k_force_segsum)
//   3. resultants     : sum of force and moment over a caller's list of block rows, in list order (k_force_resultant)
// No floating-point atomics anywhere: two readouts of one state give the same bits.
#include "kernels_common.hpp"
#include "force_keys.hpp"
#include "force_stage.hpp"

namespace mistark {

// Segmented sum over the sorted contributions: one lane per sorted position; the lane at the head of a row's run sums the run in order and writes
// f[row] = -scale * sum. Runs beyond FORCE_LONG_ROW (a rigid body attached to hundreds of points, or under thousands of contacts) are summed by the
// whole wavefront their head lies in: lanes stride over the run from its head, then a fixed-order tree. A run belongs to the one wavefront that holds
// its head, wherever it ends, so every row is written once, by one lane. No lane leaves early: the cross-lane steps need all 64.
constexpr int FORCE_LONG_ROW = 256;
__global__ __launch_bounds__(BLOCK) void k_force_segsum(const uint32_t* __restrict__ key, const uint32_t* __restrict__ val, int64_t total, const double* __restrict__ pool, double scale,
                                                       double* __restrict__ f, uint32_t* __restrict__ stat)
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
    const bool is_long = head && end - i > FORCE_LONG_ROW;
    if (head && !is_long) {
        double a0 = 0.0, a1 = 0.0, a2 = 0.0;
        for (int64_t j = i; j < end; j++) {
            const double* g = pool + 3 * (size_t)val[j];
            a0 += g[0];
            a1 += g[1];
            a2 += g[2];
        }
        double* o = f + 3 * (size_t)row;
        o[0] = -scale * a0;
        o[1] = -scale * a1;
        o[2] = -scale * a2;
    }
    const unsigned long long any_long = __ballot(is_long);
    // (the mask as two scalars: the loop below is uniform over the wavefront by construction)
    unsigned long long m = ((unsigned long long)(uint32_t)__builtin_amdgcn_readfirstlane((int)(any_long >> 32)) << 32) | (uint32_t)__builtin_amdgcn_readfirstlane((int)any_long);
    if (lane == 0 && m) atomicAdd(&stat[0], (uint32_t)__popcll(m));  // (an integer count for the tests; no sum depends on it)
    const int64_t wave_first = i - lane;
    while (m) {
        const int src = __ffsll((long long)m) - 1;
        m &= m - 1;
        const int64_t first = wave_first + src;
        const int64_t last = (int64_t)(uint32_t)__shfl((int)(uint32_t)end, src, 64);  // (total < 2^31)
        const uint32_t r = (uint32_t)__shfl((int)row, src, 64);
        double a0 = 0.0, a1 = 0.0, a2 = 0.0;
        for (int64_t j = first + lane; j < last; j += 64) {
            const double* g = pool + 3 * (size_t)val[j];
            a0 += g[0];
            a1 += g[1];
            a2 += g[2];
        }
        a0 = wave_sum(a0);
        a1 = wave_sum(a1);
        a2 = wave_sum(a2);
        if (lane == 0) {
            double* o = f + 3 * (size_t)r;
            o[0] = -scale * a0;
            o[1] = -scale * a1;
            o[2] = -scale * a2;
        }
    }
}

// out[0..3) = sum of f over the listed block rows, out[3..6) = sum of (pos - about) x f when positions are given, else 0. One workgroup: thread t
// takes the list entries t, t + 256, ... in order, then the fixed tree of block_sum.
__global__ __launch_bounds__(BLOCK) void k_force_resultant(const double* __restrict__ f, const int32_t* __restrict__ rows, int64_t n_rows, const double* __restrict__ pos, double ax,
                                                          double ay, double az, double* __restrict__ out)
{
    __shared__ double sm[4];
    double s[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int64_t t = threadIdx.x; t < n_rows; t += BLOCK) {
        const double* fr = f + 3 * (size_t)rows[t];
        const double fx = fr[0], fy = fr[1], fz = fr[2];
        s[0] += fx;
        s[1] += fy;
        s[2] += fz;
        if (pos) {
            const double rx = pos[3 * t] - ax, ry = pos[3 * t + 1] - ay, rz = pos[3 * t + 2] - az;
            s[3] += ry * fz - rz * fy;
            s[4] += rz * fx - rx * fz;
            s[5] += rx * fy - ry * fx;
        }
    }
#pragma unroll
    for (int k = 0; k < 6; k++) {
        const double v = block_sum(s[k], sm);
        if (threadIdx.x == 0) out[k] = v;
    }
}

// refusals and prepare() of every readout that takes a list of potentials (this one and budget.hip): the ids in the caller's order, all of them when
// `all` is set
std::vector<int> select_potentials(Context& c, const int32_t* pots, int32_t n, bool all, const char* who)
{
    if (c.dry) throw Error(std::string(who) + ": registration-only context (mistark_create_dry): nothing can be evaluated");
    if (c.world > 1) throw Error(std::string(who) + ": single-rank accessor (a sharded context holds the elements touching its rows)");
    if (!all && n > 0 && !pots) throw Error(std::string(who) + ": null potential list");
    std::vector<int> ids;
    if (all) {
        for (int p = 0; p < (int)c.pots.size(); p++) ids.push_back(p);
    } else {
        std::vector<char> seen(c.pots.size(), 0);
        for (int32_t k = 0; k < n; k++) {
            const int p = pots[k];
            if (p < 0 || p >= (int)c.pots.size()) throw Error(std::string(who) + ": bad potential id " + std::to_string(p));
            if (seen[(size_t)p]) throw Error(std::string(who) + ": potential '" + c.pots[(size_t)p].name + "' is listed twice");
            seen[(size_t)p] = 1;
            ids.push_back(p);
        }
    }
    for (int p : ids)
        if (c.pots[(size_t)p].kind == KIND_CUSTOM)
            throw Error(std::string(who) + ": potential '" + c.pots[(size_t)p].name + "' is user-defined (mistark_potential_custom): its kernels have no pool path");
    prepare(c);  // (as eval(): contact tables then have their device connectivity and current row counts; no search runs)
    return ids;
}

// the selection and its layout in a readout pool
ForceSelection force_select(Context& c, const int32_t* pots, int32_t n, bool all, const char* who)
{
    const std::vector<int> ids = select_potentials(c, pots, n, all, who);
    ForceSelection S;
    for (int p : ids) {
        const Potential& P = c.pots[(size_t)p];
        if (P.n_elem <= 0) continue;  // (empty tables launch nothing)
        ForceDesc d{};
        d.conn = P.args.conn;
        d.stride = P.conn_stride;
        d.n_elem = P.n_elem;
        d.NB = P.NB;
        d.g_off = (uint32_t)S.total;
        for (int k = 0; k < P.NB; k++) {
            d.dof_col[k] = P.args.dof_col[k];
            d.dof_row_off[k] = P.args.dof_row_off[k];
        }
        S.pots.push_back(p);
        S.descs.push_back(d);
        S.g_off.push_back(S.total);
        S.total += (int64_t)P.NB * P.n_elem;
    }
    if (S.total >= (1ll << 31)) throw Error(std::string(who) + ": too many contributions");
    return S;
}
// stage 1: node gradients of every selected element into W.pool
void force_element_stage(Context& c, const ForceSelection& S, const ForceWork& W)
{
    int n_max = 0;
    for (int p : S.pots) n_max = std::max(n_max, c.pots[(size_t)p].n_elem);
    W.pool.ensure(3 * (size_t)S.total);
    W.elemE.ensure((size_t)n_max);
    for (size_t k = 0; k < S.pots.size(); k++) launch_force_elements(c, c.pots[(size_t)S.pots[k]], W.pool.p + 3 * (size_t)S.g_off[k], W.elemE.p);
    MS_CHECK(hipGetLastError());
}
// stage 2: f_dev[ndofs] = -scale * row sums of the pool; stat[0] = rows a whole wavefront summed. Returns the sorted keys (one of W.key / W.key_alt).
const uint32_t* force_nodal_stage(Context& c, const ForceSelection& S, const ForceWork& W, double scale, double* f_dev, uint32_t* stat)
{
    const int64_t n = S.total;
    W.key.ensure((size_t)n);
    W.key_alt.ensure((size_t)n);
    W.val.ensure((size_t)n);
    W.val_alt.ensure((size_t)n);
    W.desc.ensure(S.descs.size() * sizeof(ForceDesc));
    h2d_small(c, W.desc.p, S.descs.data(), S.descs.size() * sizeof(ForceDesc));
    hipLaunchKernelGGL(k_force_keys, dim3(grid_for(n)), dim3(BLOCK), 0, c.stream, (const ForceDesc*)W.desc.p, (int)S.descs.size(), n, W.key.p, W.val.p);
    int bits = 1;
    while (bits < 32 && (1ll << bits) <= c.nbr) bits++;
    size_t tmp = 0;
    hipcub::DoubleBuffer<uint32_t> dk(W.key.p, W.key_alt.p), dv(W.val.p, W.val_alt.p);
    MS_CHECK(hipcub::DeviceRadixSort::SortPairs(nullptr, tmp, dk, dv, (int)n, 0, bits, c.stream));
    W.cub_tmp.ensure(tmp);
    MS_CHECK(hipcub::DeviceRadixSort::SortPairs(W.cub_tmp.p, tmp, dk, dv, (int)n, 0, bits, c.stream));  // (stable: equal rows keep the contribution order)
    {
        FillQueue fills(c.stream);
        fills.add(f_dev, 0, (size_t)c.ndofs * sizeof(double));  // (rows with nobody contributing are zero)
        fills.add(stat, 0, 2 * sizeof(uint32_t));
    }
    hipLaunchKernelGGL(k_force_segsum, dim3(grid_for(n)), dim3(BLOCK), 0, c.stream, (const uint32_t*)dk.Current(), (const uint32_t*)dv.Current(), n, (const double*)W.pool.p, scale,
                       f_dev, stat);
    MS_CHECK(hipGetLastError());
    return dk.Current();
}

namespace {
using Selection = ForceSelection;
Selection select(Context& c, const int32_t* pots, int32_t n, bool all, const char* who) { return force_select(c, pots, n, all, who); }
ForceWork own_work(Context& c) { return ForceWork{c.fr_pool, c.fr_elemE, c.fr_key, c.fr_key_alt, c.fr_val, c.fr_val_alt, c.fr_desc, c.fr_cub_tmp}; }
void element_stage(Context& c, const Selection& S)
{
    force_element_stage(c, S, own_work(c));
    c.n_force_readouts++;
}
void nodal_stage(Context& c, const Selection& S, double scale, double* f_dev)
{
    c.fr_stat.ensure(2);
    force_nodal_stage(c, S, own_work(c), scale, f_dev, c.fr_stat.p);
    c.fr_stat_valid = true;
}
}  // namespace

bool force_readout(Context& c, const int32_t* pots, int32_t n, bool all, double scale, double* f_dev)
{
    const Selection S = select(c, pots, n, all, "mistark_forces");
    if (S.total == 0) return false;
    element_stage(c, S);
    nodal_stage(c, S, scale, f_dev);
    return true;
}

void force_elements_host(Context& c, int pot, double scale, double* out, int32_t* block_rows, int64_t* n_elem, int32_t* nb)
{
    const int32_t id = pot;
    const Selection S = select(c, &id, 1, false, "mistark_potential_element_forces");
    const Potential& P = c.pots[(size_t)pot];
    const int NB = P.NB, ne = P.n_elem;
    if (n_elem) *n_elem = ne;
    if (nb) *nb = NB;
    if (ne <= 0) return;
    if (out) {
        element_stage(c, S);
        std::vector<double> tmp(3 * (size_t)S.total);
        MS_CHECK(hipMemcpyAsync(tmp.data(), c.fr_pool.p, tmp.size() * sizeof(double), hipMemcpyDeviceToHost, c.stream));
        MS_CHECK(hipStreamSynchronize(c.stream));
        for (int e = 0; e < ne; e++)
            for (int k = 0; k < NB; k++)
                for (int i = 0; i < 3; i++) out[((size_t)e * NB + k) * 3 + i] = -scale * tmp[((size_t)k * ne + e) * 3 + i];
    }
    if (block_rows) {
        std::vector<int32_t> dev_conn;  // (tables of the device-side contact detector have no host copy)
        const int32_t* conn = P.conn_host.data();
        if (P.conn_ext) {
            dev_conn.resize((size_t)ne * P.conn_stride);
            MS_CHECK(hipMemcpyAsync(dev_conn.data(), P.conn_ext, dev_conn.size() * sizeof(int32_t), hipMemcpyDeviceToHost, c.stream));
            MS_CHECK(hipStreamSynchronize(c.stream));
            conn = dev_conn.data();
        }
        for (int e = 0; e < ne; e++)
            for (int k = 0; k < NB; k++) block_rows[(size_t)e * NB + k] = P.args.dof_row_off[k] + conn[(size_t)e * P.conn_stride + P.args.dof_col[k]];
    }
}

void force_nodal_host(Context& c, const int32_t* pots, int32_t n, double scale, double* f_host)
{
    if (!f_host) throw Error("mistark_forces: null output");
    if (n < 0) throw Error("mistark_forces: negative count");
    const Selection S = select(c, pots, n, n == 0, "mistark_forces");
    if (S.total == 0) {
        std::fill(f_host, f_host + c.ndofs, 0.0);
        return;
    }
    element_stage(c, S);
    c.fr_out.ensure((size_t)c.ndofs);
    nodal_stage(c, S, scale, c.fr_out.p);
    MS_CHECK(hipMemcpyAsync(f_host, c.fr_out.p, (size_t)c.ndofs * sizeof(double), hipMemcpyDeviceToHost, c.stream));
    MS_CHECK(hipStreamSynchronize(c.stream));
}

void force_resultant_host(Context& c, const int32_t* pots, int32_t n, double scale, const int32_t* rows, int64_t n_rows, const double* pos_host, const double* about, double* out)
{
    const char* who = "mistark_forces_resultant";
    if (!out) throw Error(std::string(who) + ": null output");
    if (n < 0 || n_rows < 0 || (n_rows > 0 && !rows)) throw Error(std::string(who) + ": bad row list");
    if (pos_host && !about) throw Error(std::string(who) + ": positions without a reference point");
    const Selection S = select(c, pots, n, n == 0, who);
    for (int64_t t = 0; t < n_rows; t++)
        if (rows[t] < 0 || rows[t] >= c.nbr) throw Error(std::string(who) + ": block row " + std::to_string(rows[t]) + " is outside the " + std::to_string(c.nbr) + " rows of the DoF vector");
    for (int k = 0; k < 6; k++) out[k] = 0.0;
    if (S.total == 0 || n_rows == 0) return;
    element_stage(c, S);
    c.fr_out.ensure((size_t)c.ndofs);
    nodal_stage(c, S, scale, c.fr_out.p);
    c.fr_rows.ensure((size_t)n_rows);
    c.fr_res.ensure(6);
    h2d_staged(c, c.fr_rows.p, rows, (size_t)n_rows * sizeof(int32_t));
    if (pos_host) {
        c.fr_pos.ensure(3 * (size_t)n_rows);
        h2d_staged(c, c.fr_pos.p, pos_host, 3 * (size_t)n_rows * sizeof(double));
    }
    hipLaunchKernelGGL(k_force_resultant, dim3(1), dim3(BLOCK), 0, c.stream, (const double*)c.fr_out.p, (const int32_t*)c.fr_rows.p, n_rows, pos_host ? (const double*)c.fr_pos.p : nullptr,
                       pos_host ? about[0] : 0.0, pos_host ? about[1] : 0.0, pos_host ? about[2] : 0.0, c.fr_res.p);
    MS_CHECK(hipGetLastError());
    MS_CHECK(hipMemcpyAsync(out, c.fr_res.p, 6 * sizeof(double), hipMemcpyDeviceToHost, c.stream));
    MS_CHECK(hipStreamSynchronize(c.stream));  // (also: the caller's row and position arrays have been read)
}

int64_t force_long_rows(Context& c)
{
    if (!c.fr_stat_valid) return 0;
    uint32_t v[2] = {0, 0};
    fetch(c, v, c.fr_stat.p, sizeof(v));
    return (int64_t)v[0];
}

// nodal vectors the host mirror records inside a time step and keeps on the device
void force_record_slot(Context& c, int slot, const int32_t* pots, int32_t n, bool all, double scale)
{
    if (slot < 0 || slot >= 4096) throw Error("force readout: bad slot");
    if ((size_t)slot >= c.force_slots.size()) c.force_slots.resize((size_t)slot + 1);
    Context::ForceSlot& s = c.force_slots[(size_t)slot];
    if (!all && n == 0) {  // (a group that matches no potential)
        if (c.dry) throw Error("force readout: registration-only context (mistark_create_dry): nothing can be evaluated");
        prepare(c);
        s.n = c.ndofs;
        s.zero = true;
        return;
    }
    s.n = -1;
    prepare(c);
    s.f.ensure((size_t)c.ndofs);
    s.zero = !force_readout(c, pots, n, all, scale, s.f.p);
    s.n = c.ndofs;
}
void force_fetch_slot(Context& c, int slot, double* f_host, int64_t n)
{
    if (slot < 0 || (size_t)slot >= c.force_slots.size() || c.force_slots[(size_t)slot].n < 0) throw Error("force readout: nothing recorded for group " + std::to_string(slot));
    Context::ForceSlot& s = c.force_slots[(size_t)slot];
    if (n != s.n) throw Error("force readout: the recorded vector has " + std::to_string(s.n) + " entries, the caller asks for " + std::to_string(n));
    if (s.zero) {
        std::fill(f_host, f_host + n, 0.0);
        return;
    }
    MS_CHECK(hipMemcpyAsync(f_host, s.f.p, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, c.stream));
    MS_CHECK(hipStreamSynchronize(c.stream));
}

}  // namespace mistark
