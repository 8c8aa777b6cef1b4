// wrench.hip — opt-in rigid-body wrench report: force and torque on every rigid body from any potential (rows) and from any family of potentials
// (bodies), at the engine's current DoFs. The map from the gradient to the wrench and the record layouts are in wrench.hpp.
//
// A pipeline of its own beside eval(), like the force readout whose two stages it reuses on buffers of its own (force_stage.hpp): it reads potentials,
// state and the contact and friction tables as installed, and writes only the Context::wr_* buffers.
//   rows   : the generic hyper-dual gradient of every element of one potential -> wr_pool; one lane per element classifies the element's block rows as
//            "v of body b", "w of body b" or "not rigid" from the row ranges of the two DoF sets, adds up the blocks of one body in block order, applies
//            the map and stores up to two slots field-major (k_wrench_rows)
//   bodies : per family the same element stage, the key sort and k_force_segsum -> wr_f[family] (the bits mistark_forces returns with scale 1/dt);
//            k_wrench_rows in counting mode adds every active element to the integer count of the bodies it touches; one lane per (family, body) applies
//            the map and the shift to the reference point (k_wrench_bodies)
// No floating-point atomics anywhere: two reports of one state give the same bits. The counts are integer atomics, exact in any order.
#include "kernels_common.hpp"
#include "energies.hpp"
#include "registry.hpp"
#include "force_stage.hpp"
#include "wrench.hpp"

namespace mistark {

constexpr int WRENCH_LONG_ROW = 256;  // (k_force_segsum's FORCE_LONG_ROW)

// active[e] = whether the condition of element e is on
template <class En>
__global__ __launch_bounds__(BLOCK) void k_wrench_active(PotArgs a, uint8_t* __restrict__ active)
{
    const int e = blockIdx.x * BLOCK + threadIdx.x;
    if (e >= a.n_elem) return;
    double in[En::Layout::NIN];
    gather_inputs<En>(a, e, in);
    active[e] = En::active(in) ? 1 : 0;
}

struct WrenchBodies  // the rigid bodies' state on the device and where their rows lie in the DoF vector
{
    const double *v1, *w1, *t0;
    int v_row0, w_row0, n_bodies;
    double dt, inv_dt;
};

// One lane per element of one potential. pool: the potential's node gradients [block][element][3]; active: null for a potential without a condition.
// rec [2 * 12][N] and ids [N][4] are written when given; count [n_bodies] (integers) takes one per active element and body it touches when given.
__global__ __launch_bounds__(BLOCK) void k_wrench_rows(ForceDesc d, const double* __restrict__ pool, const uint8_t* __restrict__ active, WrenchBodies B, double* __restrict__ rec,
                                                      int64_t N, int32_t* __restrict__ ids, int32_t* __restrict__ count)
{
    const int e = blockIdx.x * BLOCK + threadIdx.x;
    if (e >= d.n_elem) return;
    const int32_t* ce = d.conn + (size_t)e * d.stride;
    int b0 = -1, b1 = -1, n_rigid = 0, flags = 0;
    double v0x = 0.0, v0y = 0.0, v0z = 0.0, w0x = 0.0, w0y = 0.0, w0z = 0.0;
    double v1x = 0.0, v1y = 0.0, v1z = 0.0, w1x = 0.0, w1y = 0.0, w1z = 0.0;
#pragma unroll
    for (int k = 0; k < MAX_NB; k++) {
        if (k >= d.NB) continue;
        const int row = d.dof_row_off[k] + ce[d.dof_col[k]];
        const int bv = row - B.v_row0, bw = row - B.w_row0;
        const bool is_v = bv >= 0 && bv < B.n_bodies, is_w = bw >= 0 && bw < B.n_bodies;
        if (!is_v && !is_w) continue;
        const int b = is_v ? bv : bw;
        const double* g = pool + 3 * ((size_t)k * d.n_elem + e);
        const double gx = g[0], gy = g[1], gz = g[2];
        n_rigid++;
        if (!(isfinite(gx) && isfinite(gy) && isfinite(gz))) flags |= WRENCH_FLAG_NONFINITE;
        if (b0 < 0) b0 = b;
        else if (b != b0 && b1 < 0) b1 = b;
        const bool s0 = b == b0, s1 = !s0 && b == b1;
        if (!s0 && !s1) flags |= WRENCH_FLAG_BODIES;
        if (s0 && is_v) v0x += gx, v0y += gy, v0z += gz;
        if (s0 && is_w) w0x += gx, w0y += gy, w0z += gz;
        if (s1 && is_v) v1x += gx, v1y += gy, v1z += gz;
        if (s1 && is_w) w1x += gx, w1y += gy, w1z += gz;
    }
    const bool on = !active || active[e] != 0;
    if (!on) flags |= WRENCH_FLAG_OFF;
    if (count && on) {
        if (b0 >= 0) atomicAdd(&count[b0], 1);
        if (b1 >= 0) atomicAdd(&count[b1], 1);
    }
    if (ids) reinterpret_cast<int4*>(ids)[e] = make_int4(b0, b1, n_rigid, flags);
    if (!rec) return;
#pragma unroll
    for (int s = 0; s < WRENCH_SLOTS; s++) {
        const int b = s == 0 ? b0 : b1;
        double r[WRENCH_REC];
#pragma unroll
        for (int f = 0; f < WRENCH_REC; f++) r[f] = 0.0;
        if (b >= 0 && on) {
            const double gv[3] = {s == 0 ? v0x : v1x, s == 0 ? v0y : v1y, s == 0 ? v0z : v1z};
            const double gw[3] = {s == 0 ? w0x : w1x, s == 0 ? w0y : w1y, s == 0 ? w0z : w1z};
            const double* w = B.w1 + 3 * (size_t)b;
            const double wb[3] = {w[0], w[1], w[2]};
            wrench_slot_record(gv, gw, wb, B.dt, B.inv_dt, r);
        }
#pragma unroll
        for (int f = 0; f < WRENCH_REC; f++) rec[(size_t)(s * WRENCH_REC + f) * N + e] = r[f];
    }
}

// stat[0] += the runs of the sorted keys that lie in the bodies' rows and that k_force_segsum gave to a whole wavefront (an integer count for the
// tests; no sum depends on it)
__global__ __launch_bounds__(BLOCK) void k_wrench_long_rows(const uint32_t* __restrict__ key, int64_t total, WrenchBodies B, uint32_t* __restrict__ stat)
{
    const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= total) return;
    const uint32_t row = key[i];
    if (i > 0 && key[i - 1] == row) return;
    const int bv = (int)row - B.v_row0, bw = (int)row - B.w_row0;
    if (!((bv >= 0 && bv < B.n_bodies) || (bw >= 0 && bw < B.n_bodies))) return;
    int64_t lo = i, hi = total;  // first position behind the run
    while (hi - lo > 1) {
        const int64_t mid = (lo + hi) >> 1;
        if (key[mid] == row) lo = mid;
        else hi = mid;
    }
    if (hi - i > WRENCH_LONG_ROW) atomicAdd(&stat[0], 1u);
}

// one lane per (family, body): f [n_families][ndofs] -> out [n_families][n_bodies][16]
__global__ __launch_bounds__(BLOCK) void k_wrench_bodies(const double* __restrict__ f, int64_t ndofs, int n_families, WrenchBodies B, double ax, double ay, double az,
                                                        double* __restrict__ out)
{
    const int t = blockIdx.x * BLOCK + threadIdx.x;
    if (t >= n_families * B.n_bodies) return;
    const int fam = t / B.n_bodies, b = t - fam * B.n_bodies;
    const double* fv = f + (size_t)fam * ndofs + 3 * (size_t)(B.v_row0 + b);
    const double* fw = f + (size_t)fam * ndofs + 3 * (size_t)(B.w_row0 + b);
    const double Fv[3] = {fv[0], fv[1], fv[2]}, Fw[3] = {fw[0], fw[1], fw[2]};
    const double t0[3] = {B.t0[3 * (size_t)b], B.t0[3 * (size_t)b + 1], B.t0[3 * (size_t)b + 2]};
    const double v1[3] = {B.v1[3 * (size_t)b], B.v1[3 * (size_t)b + 1], B.v1[3 * (size_t)b + 2]};
    const double w1[3] = {B.w1[3 * (size_t)b], B.w1[3 * (size_t)b + 1], B.w1[3 * (size_t)b + 2]};
    const double about[3] = {ax, ay, az};
    double r[WRENCH_BODY_REC];
    wrench_body_record(Fv, Fw, t0, v1, w1, B.dt, about, r);
    double* o = out + (size_t)t * WRENCH_BODY_REC;
#pragma unroll
    for (int k = 0; k < WRENCH_BODY_REC; k++) o[k] = r[k];
}

namespace {
ForceWork own_work(Context& c) { return ForceWork{c.wr_pool, c.wr_elemE, c.wr_key, c.wr_key_alt, c.wr_val, c.wr_val_alt, c.wr_desc, c.wr_cub_tmp}; }

const Array& state_array(Context& c, int id, int stride, int64_t n_bodies, bool dof, const char* role, const char* who)
{
    if (id < 0 || id >= (int)c.arrays.size()) throw Error(std::string(who) + ": bad array id " + std::to_string(id) + " for " + role);
    const Array& A = c.arrays[(size_t)id];
    if (dof && A.dof_set < 0) throw Error(std::string(who) + ": array " + std::to_string(id) + " (" + role + ") is not a DoF array: the bodies' rows are read off its DoF set");
    if (A.stride != stride)
        throw Error(std::string(who) + ": array " + std::to_string(id) + " (" + role + ") has items of " + std::to_string(A.stride) + " doubles, " + std::to_string(stride) + " are needed");
    if (A.n_items != n_bodies)
        throw Error(std::string(who) + ": array " + std::to_string(id) + " (" + role + ") has " + std::to_string(A.n_items) + " items, n_bodies is " + std::to_string(n_bodies));
    return A;
}
// the bodies' state arrays (after prepare()); refuses where no inertia potential is bound (inertia_bindings: EnergyRigidBodyInertia_linear's, else
// EnergyLumpedInertia's, which serves a scene without bodies); the time step itself comes with fetch_dt()
WrenchBodies resolve_bodies(Context& c, int v1, int w1, int t0, int q0, int32_t n_bodies, const char* who)
{
    if (n_bodies < 0) throw Error(std::string(who) + ": negative body count");
    const Array& Av = state_array(c, v1, 3, n_bodies, true, "v1", who);
    const Array& Aw = state_array(c, w1, 3, n_bodies, true, "w1", who);
    const Array& At = state_array(c, t0, 3, n_bodies, false, "t0", who);
    state_array(c, q0, 4, n_bodies, false, "q0", who);
    if (Av.dof_set == Aw.dof_set) throw Error(std::string(who) + ": v1 and w1 name the same DoF set");
    if (!inertia_bindings(c).dt) throw Error(std::string(who) + ": no inertia potential is registered: the time step is taken from its bindings");
    WrenchBodies B{};
    B.v1 = Av.dev;
    B.w1 = Aw.dev;
    B.t0 = At.dev;
    B.v_row0 = (int)(c.dof_sets[(size_t)Av.dof_set].offset / 3);
    B.w_row0 = (int)(c.dof_sets[(size_t)Aw.dof_set].offset / 3);
    B.n_bodies = n_bodies;
    return B;
}
// the time step, read back from the device (a stream synchronisation: only the calls that launch pay it)
void fetch_dt(Context& c, WrenchBodies& B, const char* who)
{
    fetch(c, &B.dt, inertia_bindings(c).dt, sizeof(double));
    if (!(B.dt > 0.0) || !std::isfinite(B.dt)) throw Error(std::string(who) + ": the bound time step is " + std::to_string(B.dt));
    B.inv_dt = 1.0 / B.dt;
}
template <class En>
bool try_active(Context& c, const Potential& P, uint8_t* active)
{
    if constexpr (HasCond<En>::value) {
        if (P.name != En::name) return false;
        hipLaunchKernelGGL((k_wrench_active<En>), dim3(grid_for(P.n_elem)), dim3(BLOCK), 0, c.stream, P.args, active);
        return true;
    } else {
        return false;
    }
}
// the rows kernel of one potential on its part of the pool (P has elements)
void launch_rows(Context& c, const Potential& P, const ForceDesc& d, const double* pool, const WrenchBodies& B, double* rec, int32_t* ids, int32_t* count)
{
    bool cond = false;
    c.wr_active.ensure((size_t)P.n_elem);
#define X(En) cond = cond || try_active<En>(c, P, c.wr_active.p);
    MISTARK_FOR_EACH_ENERGY(X)
#undef X
    hipLaunchKernelGGL(k_wrench_rows, dim3(grid_for(P.n_elem)), dim3(BLOCK), 0, c.stream, d, pool, cond ? (const uint8_t*)c.wr_active.p : nullptr, B, rec, (int64_t)P.n_elem, ids, count);
    MS_CHECK(hipGetLastError());
}
}  // namespace

void wrench_rows_host(Context& c, int pot, int v1, int w1, int t0, int q0, int32_t n_bodies, double* out, int32_t* ids, int64_t* n_rows)
{
    const char* who = "mistark_potential_rigid_wrench";
    const int32_t id = pot;
    const ForceSelection S = force_select(c, &id, 1, false, who);
    WrenchBodies B = resolve_bodies(c, v1, w1, t0, q0, n_bodies, who);
    const Potential& P = c.pots[(size_t)pot];
    if (n_rows) *n_rows = P.n_elem;
    if (P.n_elem <= 0 || (!out && !ids)) return;  // (an empty table launches nothing; all outputs null: a size query)
    fetch_dt(c, B, who);
    const size_t N = (size_t)P.n_elem;
    force_element_stage(c, S, own_work(c));
    c.wr_rec.ensure((size_t)WRENCH_SLOTS * WRENCH_REC * N);
    c.wr_ids.ensure(4 * N);
    launch_rows(c, P, S.descs[0], c.wr_pool.p, B, c.wr_rec.p, c.wr_ids.p, nullptr);
    c.n_wrench_reports++;
    std::vector<double> tmp;
    constexpr int NF = WRENCH_SLOTS * WRENCH_REC;
    if (out) {
        tmp.resize((size_t)NF * N);
        MS_CHECK(hipMemcpyAsync(tmp.data(), c.wr_rec.p, tmp.size() * sizeof(double), hipMemcpyDeviceToHost, c.stream));
    }
    if (ids) MS_CHECK(hipMemcpyAsync(ids, c.wr_ids.p, 4 * N * sizeof(int32_t), hipMemcpyDeviceToHost, c.stream));
    MS_CHECK(hipStreamSynchronize(c.stream));
    if (out)
        for (size_t e = 0; e < N; e++)
            for (int f = 0; f < NF; f++) out[e * NF + f] = tmp[(size_t)f * N + e];
}

namespace {
// the body report of the selected families into wr_out / wr_count; nothing is downloaded
void run_bodies(Context& c, const std::vector<ForceSelection>& sel, WrenchBodies B, const double* about, const char* who)
{
    const int32_t n_families = (int32_t)sel.size(), n_bodies = B.n_bodies;
    fetch_dt(c, B, who);
    const size_t nf = (size_t)n_families, nb = (size_t)n_bodies, nd = (size_t)c.ndofs;
    c.wr_f.ensure(nf * nd);
    c.wr_out.ensure(nf * nb * WRENCH_BODY_REC);
    c.wr_count.ensure(nf * nb);
    c.wr_stat.ensure(2 * nf);
    c.wr_stat_families = 0;
    fill_async(c.stream, c.wr_count.p, 0, nf * nb * sizeof(int32_t));
    const ForceWork W = own_work(c);
    for (size_t f = 0; f < nf; f++) {
        const ForceSelection& S = sel[f];
        double* fd = c.wr_f.p + f * nd;
        uint32_t* stat = c.wr_stat.p + 2 * f;
        if (S.total == 0) {  // (nothing contributes: the zero vector)
            fill_async(c.stream, fd, 0, nd * sizeof(double));
            fill_async(c.stream, stat, 0, 2 * sizeof(uint32_t));
            continue;
        }
        force_element_stage(c, S, W);
        const uint32_t* keys = force_nodal_stage(c, S, W, B.inv_dt, fd, stat);
        hipLaunchKernelGGL(k_wrench_long_rows, dim3(grid_for(S.total)), dim3(BLOCK), 0, c.stream, keys, S.total, B, stat + 1);
        for (size_t k = 0; k < S.pots.size(); k++)
            launch_rows(c, c.pots[(size_t)S.pots[k]], S.descs[k], c.wr_pool.p + 3 * (size_t)S.g_off[k], B, nullptr, nullptr, c.wr_count.p + f * nb);
    }
    hipLaunchKernelGGL(k_wrench_bodies, dim3(grid_for((int64_t)(nf * nb))), dim3(BLOCK), 0, c.stream, (const double*)c.wr_f.p, (int64_t)c.ndofs, (int)n_families, B, about[0], about[1],
                       about[2], c.wr_out.p);
    MS_CHECK(hipGetLastError());
    c.n_wrench_reports++;
    c.wr_stat_families = n_families;
    c.wr_out_families = n_families;
    c.wr_out_bodies = n_bodies;
}
void download_bodies(Context& c, double* out, int32_t* count)
{
    const size_t n = (size_t)c.wr_out_families * (size_t)c.wr_out_bodies;
    if (out) MS_CHECK(hipMemcpyAsync(out, c.wr_out.p, n * WRENCH_BODY_REC * sizeof(double), hipMemcpyDeviceToHost, c.stream));
    if (count) MS_CHECK(hipMemcpyAsync(count, c.wr_count.p, n * sizeof(int32_t), hipMemcpyDeviceToHost, c.stream));
    MS_CHECK(hipStreamSynchronize(c.stream));
}
}  // namespace

void wrench_bodies_host(Context& c, const int32_t* families, const int32_t* family_start, int32_t n_families, int v1, int w1, int t0, int q0, int32_t n_bodies, const double* about,
                        double* out, int32_t* count)
{
    const char* who = "mistark_rigid_wrench";
    if (n_families < 0) throw Error(std::string(who) + ": negative family count");
    if (n_families > 0 && !family_start) throw Error(std::string(who) + ": null family table");
    if (!about) throw Error(std::string(who) + ": null reference point");
    select_potentials(c, nullptr, 0, false, who);  // (the refusals that need no list, and prepare())
    std::vector<ForceSelection> sel;
    for (int32_t f = 0; f < n_families; f++) {
        const int32_t a = family_start[f], b = family_start[f + 1];
        if (a < 0 || b < a) throw Error(std::string(who) + ": the family table does not ascend at family " + std::to_string(f));
        if (b > a && !families) throw Error(std::string(who) + ": null potential list");
        sel.push_back(force_select(c, b > a ? families + a : nullptr, b - a, b == a, who));  // (an empty list: every potential)
    }
    const WrenchBodies B = resolve_bodies(c, v1, w1, t0, q0, n_bodies, who);
    if (n_families == 0 || n_bodies == 0 || (!out && !count)) return;
    run_bodies(c, sel, B, about, who);
    download_bodies(c, out, count);
}

// The host mirror's step: the body report of the given families (a list may be empty: the zero wrench; all[f]: every potential), kept on the device.
void wrench_record_step(Context& c, const std::vector<std::vector<int32_t>>& families, const std::vector<char>& all, int v1, int w1, int t0, int q0, int32_t n_bodies,
                        const double* about)
{
    const char* who = "wrench recording";
    select_potentials(c, nullptr, 0, false, who);
    std::vector<ForceSelection> sel;
    for (size_t f = 0; f < families.size(); f++) sel.push_back(force_select(c, families[f].empty() ? nullptr : families[f].data(), (int32_t)families[f].size(), all[f] != 0, who));
    const WrenchBodies B = resolve_bodies(c, v1, w1, t0, q0, n_bodies, who);
    c.wr_out_families = c.wr_out_bodies = 0;
    if (sel.empty() || n_bodies == 0) return;
    run_bodies(c, sel, B, about, who);
}
void wrench_fetch_step(Context& c, int32_t n_families, int32_t n_bodies, double* out, int32_t* count)
{
    if (n_families != c.wr_out_families || n_bodies != c.wr_out_bodies)
        throw Error("wrench recording: " + std::to_string(c.wr_out_families) + " x " + std::to_string(c.wr_out_bodies) + " records are held, the caller asks for " +
                    std::to_string(n_families) + " x " + std::to_string(n_bodies));
    download_bodies(c, out, count);
}

int64_t wrench_long_rows(Context& c)
{
    if (c.wr_stat_families <= 0) return 0;
    std::vector<uint32_t> v(2 * (size_t)c.wr_stat_families);
    MS_CHECK(hipMemcpyAsync(v.data(), c.wr_stat.p, v.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, c.stream));
    MS_CHECK(hipStreamSynchronize(c.stream));
    int64_t n = 0;
    for (int f = 0; f < c.wr_stat_families; f++) n += v[2 * (size_t)f + 1];
    return n;
}

}  // namespace mistark
