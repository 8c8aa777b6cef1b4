// budget.hip — opt-in energy and momentum budget readout: the energy of every potential, the 13-slot record (budget.hpp) of every inertia group and of
// every rigid body, at the engine's current DoFs.
//
// A pipeline of its own beside eval(), like the force and stress readouts: it reads potentials and state and writes only the Context::bg_* buffers (and
// the slots the host mirror keeps).
//   energies : the energy-only kernel of every selected potential on a copy of its argument block, element energies to bg_elemE (launch_energy_elements),
//              one workgroup per chunk of BUDGET_CHUNK elements (k_budget_energy_chunks), one workgroup per potential folds its chunks (k_budget_fold)
//   inertia  : the host lists the elements group by group (stable) and cuts every group's list into chunks of BUDGET_CHUNK items, whenever the table
//              changes; one workgroup per chunk gathers its items' inputs from the potential's own block and sums the 13 slots (k_budget_inertia_chunks);
//              one workgroup per group folds its chunks in chunk order (k_budget_fold)
//   bodies   : one lane per body (k_budget_rigid)
// Every sum is: thread t of 256 takes the terms t, t + 256, ... of its list in order, then block_sum's fixed tree. A result depends on the order of the
// element list, on BUDGET_CHUNK and on BLOCK, never on a grid size, the device or the run. No floating-point atomics anywhere.
#include "kernels_common.hpp"
#include "energies.hpp"
#include "budget.hpp"

namespace mistark {

constexpr int BUDGET_CHUNK = 2048;  // items per workgroup: eight per thread

// chunks[2 c], chunks[2 c + 1]: first term and number of terms of chunk c
__global__ __launch_bounds__(BLOCK) void k_budget_energy_chunks(const double* __restrict__ E, const int32_t* __restrict__ chunks, double* __restrict__ partial)
{
    __shared__ double sm[4];
    const int first = chunks[2 * blockIdx.x], count = chunks[2 * blockIdx.x + 1];
    double s = 0.0;
    for (int t = threadIdx.x; t < count; t += BLOCK) s += E[(size_t)first + t];
    s = block_sum(s, sm);
    if (threadIdx.x == 0) partial[blockIdx.x] = s;
}

// out[segment][NF] = the segment's partials [chunk0[segment], chunk0[segment + 1]) summed field by field in chunk order; a segment without chunks: zeros
template <int NF>
__global__ __launch_bounds__(BLOCK) void k_budget_fold(const double* __restrict__ partial, const int32_t* __restrict__ chunk0, double* __restrict__ out)
{
    __shared__ double sm[4];
    const int c0 = chunk0[blockIdx.x], c1 = chunk0[blockIdx.x + 1];
#pragma unroll
    for (int k = 0; k < NF; k++) {
        const double v = sum_partials(partial + (size_t)c0 * NF + k, c1 - c0, sm, NF);
        if (threadIdx.x == 0) out[(size_t)blockIdx.x * NF + k] = v;
    }
}

// one workgroup per chunk of one group's items; a: the argument block of the EnergyLumpedInertia potential
__global__ __launch_bounds__(BLOCK) void k_budget_inertia_chunks(PotArgs a, const uint32_t* __restrict__ items, const int32_t* __restrict__ chunks, double ax, double ay, double az,
                                                                double* __restrict__ partial)
{
    using En = E_LumpedInertia;
    __shared__ double sm[4];
    const int first = chunks[2 * blockIdx.x], count = chunks[2 * blockIdx.x + 1];
    const V3<double> about(ax, ay, az);
    BudgetAcc acc;
    for (int t = threadIdx.x; t < count; t += BLOCK) {
        double in[En::Layout::NIN];
        gather_inputs<En>(a, (int)items[(size_t)first + t], in);
        budget_add_inertia_item(acc, in, about);
    }
    double* o = partial + (size_t)blockIdx.x * BUDGET_REC;
#define MISTARK_BUDGET_SUM(field, k)                  \
    {                                                 \
        const double v = block_sum(acc.field, sm);    \
        if (threadIdx.x == 0) o[k] = v;               \
    }
    MISTARK_BUDGET_SUM(m, 0)
    MISTARK_BUDGET_SUM(mx, 1)
    MISTARK_BUDGET_SUM(my, 2)
    MISTARK_BUDGET_SUM(mz, 3)
    MISTARK_BUDGET_SUM(px, 4)
    MISTARK_BUDGET_SUM(py, 5)
    MISTARK_BUDGET_SUM(pz, 6)
    MISTARK_BUDGET_SUM(lx, 7)
    MISTARK_BUDGET_SUM(ly, 8)
    MISTARK_BUDGET_SUM(lz, 9)
    MISTARK_BUDGET_SUM(T, 10)
    MISTARK_BUDGET_SUM(U, 11)
    MISTARK_BUDGET_SUM(n, 12)
#undef MISTARK_BUDGET_SUM
}

__global__ __launch_bounds__(BLOCK) void k_budget_rigid(const double* __restrict__ t0, const double* __restrict__ q0, const double* __restrict__ v1, const double* __restrict__ w1,
                                                       const double* __restrict__ mass, const double* __restrict__ J_loc, const double* __restrict__ dt,
                                                       const double* __restrict__ gravity, int n_bodies, double ax, double ay, double az, double* __restrict__ out)
{
    const int b = blockIdx.x * BLOCK + threadIdx.x;
    if (b >= n_bodies) return;
    BudgetAcc acc;
    budget_add_body(acc, t0 + 3 * (size_t)b, q0 + 4 * (size_t)b, v1 + 3 * (size_t)b, w1 + 3 * (size_t)b, mass[b], J_loc + 9 * (size_t)b, dt[0], V3<double>(ax, ay, az),
                    V3<double>(gravity[0], gravity[1], gravity[2]));
    budget_store(acc, out + (size_t)BUDGET_REC * b);
}

// chunks of at most `chunk` terms over [first, first + count): (first term, number of terms) per chunk (shared with constraint_report.hip)
void cut_chunks(std::vector<int32_t>& chunks, int64_t first, int64_t count, int chunk)
{
    for (int64_t at = 0; at < count; at += chunk) {
        chunks.push_back((int32_t)(first + at));
        chunks.push_back((int32_t)std::min<int64_t>(chunk, count - at));
    }
}

namespace {
// where a readout leaves its n doubles: the context's own buffer, or the host mirror's slot
double* budget_target(Context& c, int slot, DevBuf<double>& own, size_t n)
{
    if (slot < 0) {
        own.ensure(n);
        return own.p;
    }
    if (slot >= 4096) throw Error("budget readout: bad slot");
    if ((size_t)slot >= c.budget_slots.size()) c.budget_slots.resize((size_t)slot + 1);
    Context::BudgetSlot& s = c.budget_slots[(size_t)slot];
    s.n = -1;
    s.v.ensure(n);
    return s.v.p;
}
void budget_finish(Context& c, int slot, const double* dev, bool launched, size_t n, double* out_host)
{
    if (slot >= 0) {
        Context::BudgetSlot& s = c.budget_slots[(size_t)slot];
        s.n = (int64_t)n;
        s.zero = !launched;
    }
    if (!out_host) return;
    if (!launched) {
        std::fill(out_host, out_host + n, 0.0);
        return;
    }
    MS_CHECK(hipMemcpyAsync(out_host, dev, n * sizeof(double), hipMemcpyDeviceToHost, c.stream));
    MS_CHECK(hipStreamSynchronize(c.stream));
}
// device pointer of an engine array with the stride and length a budget needs
const double* budget_array(Context& c, int id, int stride, int64_t n_items, const char* role, const char* who)
{
    if (id < 0 || id >= (int)c.arrays.size()) throw Error(std::string(who) + ": bad array id " + std::to_string(id) + " for " + role);
    const Array& A = c.arrays[(size_t)id];
    if (A.stride != stride || A.n_items < n_items)
        throw Error(std::string(who) + ": array " + std::to_string(id) + " (" + role + ") has " + std::to_string(A.n_items) + " items of " + std::to_string(A.stride) + " doubles, " +
                    std::to_string(n_items) + " of " + std::to_string(stride) + " are needed");
    return A.dev;
}
}  // namespace

void budget_energies(Context& c, const int32_t* pots, int32_t n, double* out_host, int slot)
{
    const char* who = "mistark_energies";
    if (n < 0) throw Error(std::string(who) + ": negative count");
    const std::vector<int> ids = select_potentials(c, pots, n, n == 0, who);
    if (ids.empty()) return;
    if (slot < 0 && !out_host) throw Error(std::string(who) + ": null output");
    // layout: the potentials' element energies one behind the other in bg_elemE; table = (first, count) per chunk, then the first chunk per potential (+1)
    std::vector<int32_t> table, chunk0;
    std::vector<int64_t> e_off;
    int64_t total = 0;
    for (int p : ids) {
        const Potential& P = c.pots[(size_t)p];
        chunk0.push_back((int32_t)(table.size() / 2));
        e_off.push_back(total);
        if (P.n_elem <= 0) continue;  // (empty tables launch nothing and report 0)
        cut_chunks(table, total, P.n_elem, BUDGET_CHUNK);
        total += P.n_elem;
    }
    if (total >= (1ll << 31)) throw Error(std::string(who) + ": too many elements");
    const int64_t n_chunks = (int64_t)table.size() / 2;
    chunk0.push_back((int32_t)n_chunks);
    double* dst = budget_target(c, slot, c.bg_E, ids.size());
    if (n_chunks > 0) {
        table.insert(table.end(), chunk0.begin(), chunk0.end());
        c.bg_echunks.ensure(table.size());
        if (table != c.bg_echunks_host) {
            h2d_small(c, c.bg_echunks.p, table.data(), table.size() * sizeof(int32_t));
            c.bg_echunks_host = table;
        }
        c.bg_elemE.ensure((size_t)total);
        c.bg_partial.ensure((size_t)n_chunks);
        for (size_t k = 0; k < ids.size(); k++) launch_energy_elements(c, c.pots[(size_t)ids[k]], c.bg_elemE.p + e_off[k]);
        hipLaunchKernelGGL(k_budget_energy_chunks, dim3((unsigned)n_chunks), dim3(BLOCK), 0, c.stream, (const double*)c.bg_elemE.p, (const int32_t*)c.bg_echunks.p, c.bg_partial.p);
        hipLaunchKernelGGL(k_budget_fold<1>, dim3((unsigned)ids.size()), dim3(BLOCK), 0, c.stream, (const double*)c.bg_partial.p, (const int32_t*)c.bg_echunks.p + 2 * n_chunks, dst);
        MS_CHECK(hipGetLastError());
        c.n_budget_readouts++;
    }
    budget_finish(c, slot, dst, n_chunks > 0, ids.size(), out_host);
}

void budget_inertia(Context& c, int pot, const double* about, int32_t n_groups, double* out_host, int slot)
{
    const char* who = "mistark_inertia_budget";
    if (n_groups < 0) throw Error(std::string(who) + ": negative group count");
    if (!about) throw Error(std::string(who) + ": null reference point");
    const int32_t id = pot;
    select_potentials(c, &id, 1, false, who);
    if (slot < 0 && n_groups > 0 && !out_host) throw Error(std::string(who) + ": null output");
    const Potential& P = c.pots[(size_t)pot];
    if (P.name != E_LumpedInertia::name) throw Error(std::string(who) + ": potential '" + P.name + "' is not an " + E_LumpedInertia::name + " potential");
    if (n_groups == 0) return;
    if (P.n_elem > 0 && (P.conn_ext || P.conn_stride < 3 || P.conn_host.size() != (size_t)P.n_elem * P.conn_stride || P.args.elem_list || P.args.e_count != P.n_elem))
        throw Error(std::string(who) + ": the table of '" + P.name + "' has no host connectivity with a group column");
    Context::BudgetPlan& plan = c.bg_plan;
    if (P.n_elem > 0 && (plan.pot != pot || plan.conn_version != P.conn_version || plan.n_elem != P.n_elem || plan.n_groups != n_groups)) {
        // the elements group by group, list order kept inside a group (counting sort), every group's list cut into chunks
        plan.pot = -1;
        std::vector<int64_t> start((size_t)n_groups + 1, 0);
        for (int e = 0; e < P.n_elem; e++) {
            const int g = P.conn_host[(size_t)e * P.conn_stride + 2];
            if (g < 0 || g >= n_groups) throw Error(std::string(who) + ": element " + std::to_string(e) + " names group " + std::to_string(g) + " of " + std::to_string(n_groups));
            start[(size_t)g + 1]++;
        }
        for (int g = 0; g < n_groups; g++) start[(size_t)g + 1] += start[(size_t)g];
        std::vector<uint32_t> items((size_t)P.n_elem);
        std::vector<int64_t> at(start.begin(), start.end() - 1);
        for (int e = 0; e < P.n_elem; e++) items[(size_t)at[(size_t)P.conn_host[(size_t)e * P.conn_stride + 2]]++] = (uint32_t)e;
        std::vector<int32_t> table, chunk0;
        for (int g = 0; g < n_groups; g++) {
            chunk0.push_back((int32_t)(table.size() / 2));
            cut_chunks(table, start[(size_t)g], start[(size_t)g + 1] - start[(size_t)g], BUDGET_CHUNK);
        }
        const int64_t n_chunks = (int64_t)table.size() / 2;
        chunk0.push_back((int32_t)n_chunks);
        table.insert(table.end(), chunk0.begin(), chunk0.end());
        c.bg_items.ensure(items.size());
        c.bg_chunks.ensure(table.size());
        h2d_staged(c, c.bg_items.p, items.data(), items.size() * sizeof(uint32_t));
        h2d_staged(c, c.bg_chunks.p, table.data(), table.size() * sizeof(int32_t));
        MS_CHECK(hipStreamSynchronize(c.stream));  // (the two lists are temporaries)
        plan.pot = pot;
        plan.conn_version = P.conn_version;
        plan.n_elem = P.n_elem;
        plan.n_groups = n_groups;
        plan.n_chunks = n_chunks;
    }
    const size_t n_out = (size_t)BUDGET_REC * n_groups;
    double* dst = budget_target(c, slot, c.bg_out, n_out);
    const bool launch = P.n_elem > 0;
    if (launch) {
        c.bg_partial.ensure((size_t)BUDGET_REC * plan.n_chunks);
        hipLaunchKernelGGL(k_budget_inertia_chunks, dim3((unsigned)plan.n_chunks), dim3(BLOCK), 0, c.stream, P.args, (const uint32_t*)c.bg_items.p, (const int32_t*)c.bg_chunks.p, about[0],
                           about[1], about[2], c.bg_partial.p);
        hipLaunchKernelGGL(k_budget_fold<BUDGET_REC>, dim3((unsigned)n_groups), dim3(BLOCK), 0, c.stream, (const double*)c.bg_partial.p, (const int32_t*)c.bg_chunks.p + 2 * plan.n_chunks,
                           dst);
        MS_CHECK(hipGetLastError());
        c.n_budget_readouts++;
        c.n_budget_chunks = plan.n_chunks;
    }
    budget_finish(c, slot, dst, launch, n_out, out_host);
}

// dt and gravity as the first registered inertia potential has them bound: EnergyRigidBodyInertia_linear's bindings 7 and 8, EnergyLumpedInertia's 9 and 10
InertiaBindings inertia_bindings(const Context& c)
{
    for (const Potential& P : c.pots) {
        if (P.kind == KIND_CUSTOM) continue;
        if (P.name == E_RBInertiaLinear::name) return {P.args.arr[7], P.args.arr[8]};
        if (P.name == E_LumpedInertia::name) return {P.args.arr[9], P.args.arr[10]};
    }
    return {};
}

void budget_rigid(Context& c, int t0, int q0, int v1, int w1, int mass, int J_loc, int32_t n_bodies, const double* about, double* out_host, int slot)
{
    const char* who = "mistark_rigid_budget";
    if (c.dry) throw Error(std::string(who) + ": registration-only context (mistark_create_dry): nothing can be evaluated");
    if (c.world > 1) throw Error(std::string(who) + ": single-rank accessor (a sharded context holds the elements touching its rows)");
    if (n_bodies < 0) throw Error(std::string(who) + ": negative body count");
    if (!about) throw Error(std::string(who) + ": null reference point");
    if (slot < 0 && n_bodies > 0 && !out_host) throw Error(std::string(who) + ": null output");
    prepare(c);
    if (n_bodies == 0) return;
    const double* d_t0 = budget_array(c, t0, 3, n_bodies, "t0", who);
    const double* d_q0 = budget_array(c, q0, 4, n_bodies, "q0", who);
    const double* d_v1 = budget_array(c, v1, 3, n_bodies, "v1", who);
    const double* d_w1 = budget_array(c, w1, 3, n_bodies, "w1", who);
    const double* d_m = budget_array(c, mass, 1, n_bodies, "mass", who);
    const double* d_J = budget_array(c, J_loc, 9, n_bodies, "J_loc", who);
    // dt and gravity as the inertia potentials have them bound
    const InertiaBindings ib = inertia_bindings(c);
    const double *d_dt = ib.dt, *d_g = ib.gravity;
    if (!d_dt || !d_g) throw Error(std::string(who) + ": no inertia potential is registered: the time step and gravity are taken from its bindings");
    const size_t n_out = (size_t)BUDGET_REC * n_bodies;
    double* dst = budget_target(c, slot, c.bg_out, n_out);
    hipLaunchKernelGGL(k_budget_rigid, dim3(grid_for(n_bodies)), dim3(BLOCK), 0, c.stream, d_t0, d_q0, d_v1, d_w1, d_m, d_J, d_dt, d_g, (int)n_bodies, about[0], about[1], about[2], dst);
    MS_CHECK(hipGetLastError());
    c.n_budget_readouts++;
    budget_finish(c, slot, dst, true, n_out, out_host);
}

void budget_fetch_slot(Context& c, int slot, double* out_host, int64_t n)
{
    if (slot < 0 || (size_t)slot >= c.budget_slots.size() || c.budget_slots[(size_t)slot].n < 0) throw Error("budget readout: nothing recorded in slot " + std::to_string(slot));
    const Context::BudgetSlot& s = c.budget_slots[(size_t)slot];
    if (n != s.n) throw Error("budget readout: the recorded array has " + std::to_string(s.n) + " entries, the caller asks for " + std::to_string(n));
    if (n == 0) return;
    if (s.zero) {
        std::fill(out_host, out_host + n, 0.0);
        return;
    }
    MS_CHECK(hipMemcpyAsync(out_host, s.v.p, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, c.stream));
    MS_CHECK(hipStreamSynchronize(c.stream));
}

}  // namespace mistark
