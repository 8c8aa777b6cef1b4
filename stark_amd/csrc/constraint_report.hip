// constraint_report.hip — opt-in constraint report of the seventeen penalty-constraint potentials (prescribed positions, the five attachments, the eleven
// rigid-body constraints): per-row violation, reaction, force, torque, anchors, energy and tolerance flags, and per-group counts, worst row, resultant,
// moment and energy, at the engine's current DoFs. The per-row arithmetic and the record layouts are in constraint_report.hpp.
//
// A pipeline of its own beside eval(), like the budget readout (budget.hip): it reads potentials and state and writes only the Context::cnr_* buffers (and
// the sets the host mirror keeps).
//   rows   : one lane per row gathers the row's inputs from the potential's own argument block and stores the record field-major, ids and aux
//            (k_constraint_rows)
//   groups : the host lists the rows group by group (stable) and cuts every group's list into chunks of CONSTRAINT_CHUNK rows, whenever the table changes;
//            one workgroup per chunk sums its rows' records (k_constraint_group_chunks): thread t of 256 takes the rows t, t + 256, ... of the chunk in list
//            order, then block_sum's fixed tree; one workgroup per group folds its chunks in chunk order (k_constraint_group_fold)
// A result depends on the order of the list, on CONSTRAINT_CHUNK and on BLOCK, never on a grid size, the device or the run. Maxima are exact; the arg-max is
// the smallest list position attaining the maximum. No floating-point atomics anywhere.
#include "kernels_common.hpp"
#include "energies.hpp"
#include "constraint_report.hpp"

namespace mistark {

constexpr int CONSTRAINT_CHUNK = 2048;  // rows per workgroup: eight per thread
void cut_chunks(std::vector<int32_t>& chunks, int64_t first, int64_t count, int chunk);  // budget.hip

// rec[field][N]: the 16 stores of a wavefront are one coalesced request each. tol: per group, null: no tolerance (the host has checked that every group
// id of the table is below the length of tol)
template <class En>
__global__ __launch_bounds__(BLOCK) void k_constraint_rows(PotArgs a, const double* __restrict__ tol, double* __restrict__ rec, int64_t N, double* __restrict__ aux,
                                                          int32_t* __restrict__ ids)
{
    using K = ConstraintKind<En>;
    const int e = blockIdx.x * BLOCK + threadIdx.x;
    if (e >= a.n_elem) return;
    double in[En::Layout::NIN];
    gather_inputs<En>(a, e, in);
    const int32_t* ce = a.conn + (size_t)e * a.conn_stride;
    const int g = ce[K::group_col];
    double r[CONSTRAINT_REC], x[2];
    constraint_record<En>(in, tol ? tol[g] : -1.0, r, x);
#pragma unroll
    for (int f = 0; f < CONSTRAINT_REC; f++) rec[(size_t)f * N + e] = r[f];
    reinterpret_cast<double2*>(aux)[e] = make_double2(x[0], x[1]);
    const int row_a = a.dof_row_off[K::block_a] + ce[a.dof_col[K::block_a]];
    int row_b = -1;
    if constexpr (K::block_b >= 0) row_b = a.dof_row_off[K::block_b] + ce[a.dof_col[K::block_b]];
    reinterpret_cast<int4*>(ids)[e] = make_int4(g, K::code, row_a, row_b);
}

// both of a block's (maximum, smallest position attaining it); a thread without a value passes m = -1
__device__ __forceinline__ void block_argmax(double& m, double& pos, double* sm)
{
    const double M = block_max(m, sm);
    const double P = -block_max(m == M && M >= 0.0 ? -pos : -1e300, sm);
    m = M;
    pos = P;
}

// one workgroup per chunk of one group's rows. partial[chunk][12]: the group record's sums over the chunk; 3: the chunk's largest |violation| (-1: none),
// 4: the position in `items` of the first row attaining it
template <bool DIR>
__global__ __launch_bounds__(BLOCK) void k_constraint_group_chunks(const double* __restrict__ rec, int64_t N, const uint32_t* __restrict__ items, const int32_t* __restrict__ chunks,
                                                                  double ax, double ay, double az, double* __restrict__ partial)
{
    __shared__ double sm[4];
    const int first = chunks[2 * blockIdx.x], count = chunks[2 * blockIdx.x + 1];
    double n = 0.0, act = 0.0, bey = 0.0, fx = 0.0, fy = 0.0, fz = 0.0, mx = 0.0, my = 0.0, mz = 0.0, E = 0.0, vmax = -1.0, pos = 0.0;
    for (int t = threadIdx.x; t < count; t += BLOCK) {
        const size_t e = items[(size_t)first + t];
        const int flags = (int)rec[15 * N + e];
        const double v = fabs(rec[e]);
        const double gx = rec[2 * N + e], gy = rec[3 * N + e], gz = rec[4 * N + e];
        n += 1.0;
        act += (double)(flags & 1);
        bey += (double)((flags >> 1) & 1);
        fx += gx;
        fy += gy;
        fz += gz;
        if constexpr (DIR) {
            mx += rec[5 * N + e];
            my += rec[6 * N + e];
            mz += rec[7 * N + e];
        } else {
            const double rx = rec[8 * N + e] - ax, ry = rec[9 * N + e] - ay, rz = rec[10 * N + e] - az;
            mx += ry * gz - rz * gy;
            my += rz * gx - rx * gz;
            mz += rx * gy - ry * gx;
        }
        E += rec[14 * N + e];
        if (v > vmax) {  // (positions ascend: the first row attaining the maximum stays)
            vmax = v;
            pos = (double)(first + t);
        }
    }
    double* o = partial + (size_t)blockIdx.x * CONSTRAINT_GROUP_REC;
#define MISTARK_CONSTRAINT_SUM(field, k)        \
    {                                           \
        const double s = block_sum(field, sm);  \
        if (threadIdx.x == 0) o[k] = s;         \
    }
    MISTARK_CONSTRAINT_SUM(n, 0)
    MISTARK_CONSTRAINT_SUM(act, 1)
    MISTARK_CONSTRAINT_SUM(bey, 2)
    MISTARK_CONSTRAINT_SUM(fx, 5)
    MISTARK_CONSTRAINT_SUM(fy, 6)
    MISTARK_CONSTRAINT_SUM(fz, 7)
    MISTARK_CONSTRAINT_SUM(mx, 8)
    MISTARK_CONSTRAINT_SUM(my, 9)
    MISTARK_CONSTRAINT_SUM(mz, 10)
    MISTARK_CONSTRAINT_SUM(E, 11)
#undef MISTARK_CONSTRAINT_SUM
    block_argmax(vmax, pos, sm);
    if (threadIdx.x == 0) {
        o[3] = vmax;
        o[4] = pos;
    }
}

// out[group][12] = the group's partials [chunk0[group], chunk0[group + 1]) folded in chunk order; a group without chunks: zeros with -1 in slot 4
__global__ __launch_bounds__(BLOCK) void k_constraint_group_fold(const double* __restrict__ partial, const int32_t* __restrict__ chunks, const int32_t* __restrict__ chunk0,
                                                                double* __restrict__ out)
{
    __shared__ double sm[4];
    const int c0 = chunk0[blockIdx.x], c1 = chunk0[blockIdx.x + 1];
    double* o = out + (size_t)blockIdx.x * CONSTRAINT_GROUP_REC;
#pragma unroll
    for (int k = 0; k < CONSTRAINT_GROUP_REC; k++) {
        if (k == 3 || k == 4) continue;
        const double v = sum_partials(partial + (size_t)c0 * CONSTRAINT_GROUP_REC + k, c1 - c0, sm, CONSTRAINT_GROUP_REC);
        if (threadIdx.x == 0) o[k] = v;
    }
    double vmax = -1.0, pos = 0.0;
    for (int i = threadIdx.x; i < c1 - c0; i += BLOCK) {
        const double* p = partial + (size_t)(c0 + i) * CONSTRAINT_GROUP_REC;
        if (p[3] > vmax) {  // (chunks ascend in list order)
            vmax = p[3];
            pos = p[4];
        }
    }
    block_argmax(vmax, pos, sm);
    if (threadIdx.x == 0) {
        const bool any = c1 > c0 && vmax >= 0.0;
        o[3] = any ? vmax : 0.0;
        o[4] = any ? pos - (double)chunks[2 * c0] : -1.0;  // position in the group's own list
    }
}

namespace {
struct KindInfo
{
    int code = -1, group_col = 0;
    bool dir = false;
};
bool kind_of(const Potential& P, KindInfo& k)
{
    if (P.kind == KIND_CUSTOM) return false;
#define X(En)                                                                                         \
    if (P.name == En::name) {                                                                         \
        k = {ConstraintKind<En>::code, ConstraintKind<En>::group_col, ConstraintKind<En>::dir_type}; \
        return true;                                                                                  \
    }
    MISTARK_FOR_EACH_CONSTRAINT(X)
#undef X
    return false;
}
// refusals, prepare(), the potential's kind; returns the potential
const Potential& select(Context& c, int pot, KindInfo& K, const char* who)
{
    const int32_t id = pot;
    select_potentials(c, &id, 1, false, who);
    const Potential& P = c.pots[(size_t)pot];
    if (!kind_of(P, K))
        throw Error(std::string(who) + ": potential '" + P.name +
                    "' has no constraint report (only EnergyPrescribedPositions, the EnergyAttachments_* and the rb_constraint_* potentials have one)");
    if (P.n_elem > 0 && (P.conn_ext || P.conn_stride <= K.group_col || P.conn_host.size() != (size_t)P.n_elem * P.conn_stride || P.args.elem_list || P.args.e_count != P.n_elem))
        throw Error(std::string(who) + ": the table of '" + P.name + "' has no host connectivity with a group column");
    return P;
}
// n_groups must exceed every group id of the table; tolerances are finite and not negative
void check_groups(const Potential& P, const KindInfo& K, const double* tolerance, int32_t n_groups, const char* who)
{
    if (n_groups < 0) throw Error(std::string(who) + ": negative group count");
    for (int e = 0; e < P.n_elem; e++) {
        const int g = P.conn_host[(size_t)e * P.conn_stride + K.group_col];
        if (g < 0 || g >= n_groups)
            throw Error(std::string(who) + ": row " + std::to_string(e) + " of '" + P.name + "' names group " + std::to_string(g) + ", n_groups is " + std::to_string(n_groups));
    }
    if (tolerance)
        for (int32_t g = 0; g < n_groups; g++)
            if (!(tolerance[g] >= 0.0) || !std::isfinite(tolerance[g]))
                throw Error(std::string(who) + ": the tolerance of group " + std::to_string(g) + " is negative or not finite");
}
template <class En>
void launch_rows(Context& c, const Potential& P, const double* tol, Context::ConstraintReportSet& S)
{
    hipLaunchKernelGGL((k_constraint_rows<En>), dim3(grid_for(P.n_elem)), dim3(BLOCK), 0, c.stream, P.args, tol, S.rec.p, (int64_t)P.n_elem, S.aux.p, S.ids.p);
}
// the row records of P into S (P has rows)
void rows_stage(Context& c, const Potential& P, const double* tolerance, int32_t n_groups, Context::ConstraintReportSet& S)
{
    const size_t N = (size_t)P.n_elem;
    S.rec.ensure((size_t)CONSTRAINT_REC * N);
    S.aux.ensure(2 * N);
    S.ids.ensure(4 * N);
    const double* tol = nullptr;
    if (tolerance && n_groups > 0) {
        c.cnr_tol.ensure((size_t)n_groups);
        h2d_staged(c, c.cnr_tol.p, tolerance, (size_t)n_groups * sizeof(double));
        tol = c.cnr_tol.p;
    }
#define X(En) \
    if (P.name == En::name) launch_rows<En>(c, P, tol, S);
    MISTARK_FOR_EACH_CONSTRAINT(X)
#undef X
    MS_CHECK(hipGetLastError());
}
// the group records of the rows in S.rec into S.groups (P has rows)
void groups_stage(Context& c, int pot, const Potential& P, const KindInfo& K, int32_t n_groups, const double* about, Context::ConstraintReportSet& S)
{
    Context::ConstraintPlan& plan = c.cnr_plans[pot];
    if (plan.conn_version != P.conn_version || plan.n_elem != P.n_elem || plan.n_groups != n_groups) {
        // the rows group by group, list order kept inside a group (counting sort), every group's list cut into chunks
        plan.n_elem = -1;
        std::vector<int64_t> start((size_t)n_groups + 1, 0);
        for (int e = 0; e < P.n_elem; e++) start[(size_t)P.conn_host[(size_t)e * P.conn_stride + K.group_col] + 1]++;
        for (int g = 0; g < n_groups; g++) start[(size_t)g + 1] += start[(size_t)g];
        std::vector<uint32_t> items((size_t)P.n_elem);
        std::vector<int64_t> at(start.begin(), start.end() - 1);
        for (int e = 0; e < P.n_elem; e++) items[(size_t)at[(size_t)P.conn_host[(size_t)e * P.conn_stride + K.group_col]]++] = (uint32_t)e;
        std::vector<int32_t> table, chunk0;
        for (int g = 0; g < n_groups; g++) {
            chunk0.push_back((int32_t)(table.size() / 2));
            cut_chunks(table, start[(size_t)g], start[(size_t)g + 1] - start[(size_t)g], CONSTRAINT_CHUNK);
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
    S.groups.ensure((size_t)CONSTRAINT_GROUP_REC * n_groups);
    c.cnr_partial.ensure((size_t)CONSTRAINT_GROUP_REC * plan.n_chunks);
    const int64_t N = P.n_elem;
    if (K.dir)
        hipLaunchKernelGGL(k_constraint_group_chunks<true>, dim3((unsigned)plan.n_chunks), dim3(BLOCK), 0, c.stream, (const double*)S.rec.p, N, (const uint32_t*)plan.items.p,
                           (const int32_t*)plan.chunks.p, about[0], about[1], about[2], c.cnr_partial.p);
    else
        hipLaunchKernelGGL(k_constraint_group_chunks<false>, dim3((unsigned)plan.n_chunks), dim3(BLOCK), 0, c.stream, (const double*)S.rec.p, N, (const uint32_t*)plan.items.p,
                           (const int32_t*)plan.chunks.p, about[0], about[1], about[2], c.cnr_partial.p);
    hipLaunchKernelGGL(k_constraint_group_fold, dim3((unsigned)n_groups), dim3(BLOCK), 0, c.stream, (const double*)c.cnr_partial.p, (const int32_t*)plan.chunks.p,
                       (const int32_t*)plan.chunks.p + 2 * plan.n_chunks, S.groups.p);
    MS_CHECK(hipGetLastError());
    c.n_constraint_chunks = plan.n_chunks;
}
// field-major records, aux and ids of a set -> the caller's row-major arrays (null outputs are skipped)
void download_rows(Context& c, const Context::ConstraintReportSet& S, double* out, double* aux, int32_t* ids)
{
    const size_t N = (size_t)S.n_rows;
    if (N == 0) return;
    std::vector<double> tmp;
    if (out) {
        tmp.resize((size_t)CONSTRAINT_REC * N);
        MS_CHECK(hipMemcpyAsync(tmp.data(), S.rec.p, tmp.size() * sizeof(double), hipMemcpyDeviceToHost, c.stream));
    }
    if (aux) MS_CHECK(hipMemcpyAsync(aux, S.aux.p, 2 * N * sizeof(double), hipMemcpyDeviceToHost, c.stream));
    if (ids) MS_CHECK(hipMemcpyAsync(ids, S.ids.p, 4 * N * sizeof(int32_t), hipMemcpyDeviceToHost, c.stream));
    MS_CHECK(hipStreamSynchronize(c.stream));
    if (out)
        for (size_t e = 0; e < N; e++)
            for (int f = 0; f < CONSTRAINT_REC; f++) out[e * CONSTRAINT_REC + f] = tmp[(size_t)f * N + e];
}
void download_groups(Context& c, const Context::ConstraintReportSet& S, double* out)
{
    if (!out || S.n_groups <= 0) return;
    const size_t n = (size_t)CONSTRAINT_GROUP_REC * S.n_groups;
    if (S.n_rows == 0) {  // nothing was launched: every declared group is empty
        std::fill(out, out + n, 0.0);
        for (int g = 0; g < S.n_groups; g++) out[(size_t)g * CONSTRAINT_GROUP_REC + 4] = -1.0;
        return;
    }
    MS_CHECK(hipMemcpyAsync(out, S.groups.p, n * sizeof(double), hipMemcpyDeviceToHost, c.stream));
    MS_CHECK(hipStreamSynchronize(c.stream));
}
}  // namespace

void constraint_rows_host(Context& c, int pot, const double* tolerance, int32_t n_groups, double* out, double* aux, int32_t* ids, int64_t* n_rows, int32_t* kind)
{
    const char* who = "mistark_potential_constraint_report";
    KindInfo K;
    const Potential& P = select(c, pot, K, who);
    if (tolerance || n_groups != 0) check_groups(P, K, tolerance, n_groups, who);
    if (n_rows) *n_rows = P.n_elem;
    if (kind) *kind = K.code;
    if (P.n_elem <= 0 || (!out && !aux && !ids)) return;  // (an empty table launches nothing; all outputs null: a size query)
    Context::ConstraintReportSet& S = c.cnr_set;
    S.n_rows = -1;
    rows_stage(c, P, tolerance, n_groups, S);
    c.n_constraint_reports++;
    S.n_rows = P.n_elem;
    S.n_groups = 0;
    download_rows(c, S, out, aux, ids);
}

void constraint_groups_host(Context& c, int pot, const double* tolerance, int32_t n_groups, const double* about, double* out)
{
    const char* who = "mistark_constraint_group_report";
    KindInfo K;
    const Potential& P = select(c, pot, K, who);
    if (!about) throw Error(std::string(who) + ": null reference point");
    check_groups(P, K, tolerance, n_groups, who);
    if (n_groups == 0 || !out) {
        if (P.n_elem <= 0) c.n_constraint_chunks = 0;
        return;
    }
    Context::ConstraintReportSet& S = c.cnr_set;
    S.n_rows = -1;
    if (P.n_elem > 0) {
        rows_stage(c, P, tolerance, n_groups, S);
        groups_stage(c, pot, P, K, n_groups, about, S);
        c.n_constraint_reports++;
    } else {
        c.n_constraint_chunks = 0;
    }
    S.n_rows = P.n_elem;
    S.n_groups = n_groups;
    download_groups(c, S, out);
}

// the host mirror's recording inside a time step: rows and groups of one potential into the set of its kind, kept on the device until they are asked for
void constraint_record_kind(Context& c, int pot, const double* tolerance, int32_t n_groups, const double* about, int32_t* kind)
{
    const char* who = "constraint report";
    KindInfo K;
    const Potential& P = select(c, pot, K, who);
    check_groups(P, K, tolerance, n_groups, who);
    if (c.cnr_slots.size() < (size_t)CONSTRAINT_KINDS) c.cnr_slots.resize((size_t)CONSTRAINT_KINDS);
    Context::ConstraintReportSet& S = c.cnr_slots[(size_t)K.code];
    S.n_rows = -1;
    if (P.n_elem > 0) {
        rows_stage(c, P, tolerance, n_groups, S);
        if (n_groups > 0) groups_stage(c, pot, P, K, n_groups, about, S);
        c.n_constraint_reports++;
    }
    S.n_rows = P.n_elem;
    S.n_groups = n_groups;
    if (kind) *kind = K.code;
}
void constraint_fetch_kind(Context& c, int kind, double* out, double* aux, int32_t* ids, double* groups, int64_t* n_rows, int32_t* n_groups)
{
    if (kind < 0 || (size_t)kind >= c.cnr_slots.size() || c.cnr_slots[(size_t)kind].n_rows < 0) throw Error("constraint report: nothing recorded for kind " + std::to_string(kind));
    const Context::ConstraintReportSet& S = c.cnr_slots[(size_t)kind];
    if (n_rows) *n_rows = S.n_rows;
    if (n_groups) *n_groups = S.n_groups;
    download_rows(c, S, out, aux, ids);
    download_groups(c, S, groups);
}

}  // namespace mistark
