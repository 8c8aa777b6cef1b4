// spectrum_report.hip — opt-in Hessian spectrum report: per element the eigenvalues of its Hessian and what the PSD projection would make of them
// (record layouts and the host restatement: spectrum_report.hpp), per block row and per potential where the indefiniteness sits.
//
// A pipeline of its own beside eval(), like the bending report: it READS element Hessians and writes only the Context::spr_* buffers.
//   source 0 : the engine's element-Hessian pool as it stands (after eval(P_G_H), before or after project()); any potential, user-defined ones included
//   source 1 : a fresh evaluation at the current DoFs into a pool of the report's own (launch_hessian_elements, kernels.hip): one potential at a time, so the
//              pool is sized by the largest, 72 NB^2 bytes per element (+ 24 NB for the node gradients the kernel also emits, + 8 for the energy)
//   rows     : k_spectrum_cols<NB>, NB = 1..8: one group of m = even(3 NB) lanes per element, 64 / m elements per wavefront (project_cols_body's ownership),
//              lane c keeps COLUMN c of A in registers, partner columns come over ds_bpermute, the rotations (c, s) of a round go through LDS once and the
//              row rotations address the lane's own registers. No V: 2 n + O(1) registers of matrix per lane instead of 4 n, and only CS / L / R in LDS.
//              A converged group applies identity rotations: an element's record does not depend on its wavefront neighbours.
//   nodal    : one key per (element, block) = its block row, stable radix sort, one pass per row in sorted order; rows beyond SPEC_LONG_ROW by the wavefront
//              that holds their head (k_spectrum_nodal)
//   potential: every potential's elements cut into chunks of SPEC_CHUNK, one workgroup per chunk (thread t takes elements t, t + 256, ..., then block_sum's
//              fixed tree), one workgroup per potential folds its chunks in chunk order
// No floating-point atomics: two reports of one state give the same bits. Minima are exact; the arg-min is the smallest position attaining the minimum.
#include "kernels_common.hpp"
#include "force_keys.hpp"
#include "spectrum_report.hpp"

namespace mistark {

static_assert(SPEC_OFF_TOL == JACOBI_OFF_TOL, "the report's stop rule is the projection's");
constexpr int SPEC_CHUNK = 2048;    // elements per workgroup of the potential stage: eight per thread
constexpr int SPEC_LONG_ROW = 64;   // contributions of a block row beyond which a wavefront handles the row
constexpr int SPEC_PART = 11;       // partial record of a chunk
void cut_chunks(std::vector<int32_t>& chunks, int64_t first, int64_t count, int chunk);  // budget.hip

template <int n>
__device__ __forceinline__ double spec_pick(const double (&x)[n], int idx)
{
    double r = 0.0;
#pragma unroll
    for (int i = 0; i < n; i++) r = i == idx ? x[i] : r;
    return r;
}
template <int NB>
struct SpecWaveShared  // LDS of ONE wavefront
{
    static constexpr int n = 3 * NB, m = (n + 1) & ~1, W = m, EPW = 64 / W;
    double2 CS[EPW + 1][m];  // (c, s) of the current round by player (+1: idle tail lanes)
    double L[EPW + 1][m];    // eigenvalues in index order
    double R[64 + W];        // group sums
};

// rec[field][N] at column col0 + e; spectrum[e][n] or null. H: pool H[(a*NB+b) * n_pool + e][3][3]
template <int NB>
__global__ __launch_bounds__(BLOCK) void k_spectrum_cols(const double* __restrict__ H, int n_elem, int n_pool, double eps, double* __restrict__ rec, int64_t N, int64_t col0,
                                                         double* __restrict__ spectrum)
{
    constexpr int n = 3 * NB, m = (n + 1) & ~1, W = m, EPW = 64 / W;
    __shared__ SpecWaveShared<NB> SS[4];
    SpecWaveShared<NB>& S = SS[threadIdx.x >> 6];
    const int w = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    const int g = lane / W, c = lane - g * W;
    if ((int64_t)w * EPW >= n_elem) return;  // (whole wavefront)
    const int e = w * EPW + g;
    const bool elem_ok = g < EPW && e < n_elem;
    const bool valid = elem_ok && c < n;  // this lane holds a column
    const size_t hs = (size_t)n_pool * 9;
    const int bb = c / 3, jj = c - 3 * bb;
    double a[n];
    bool bad = false;
#pragma unroll
    for (int i = 0; i < n; i++) {
        const int ba = i / 3, ii = i - 3 * ba;
        a[i] = valid ? H[(size_t)(ba * NB + bb) * hs + (size_t)e * 9 + ii * 3 + jj] : 0.0;
        bad = bad || !isfinite(a[i]);
    }
    auto group_sum = [&](double x) {
        __builtin_amdgcn_wave_barrier();
        S.R[lane] = x;
        __builtin_amdgcn_wave_barrier();
        double sum = 0.0;
#pragma unroll
        for (int k = 0; k < W; k++) sum += S.R[g * W + k];
        return sum;
    };
    double fro = 0.0;
#pragma unroll
    for (int i = 0; i < n; i++) fro += a[i] * a[i];
    fro = group_sum(fro);
    const double trace = group_sum(spec_pick<n>(a, c));
    const bool finite = group_sum(bad ? 1.0 : 0.0) == 0.0;
    if (!finite) {  // (no rotation may see the entries: a NaN never converges)
#pragma unroll
        for (int i = 0; i < n; i++) a[i] = 0.0;
    }
    bool active = elem_ok && finite;
    bool converged = false;
    int sweeps = 0;
    double off_stop = 0.0;
    // 1 / sqrt(x) and 1 / x to double precision from the hardware estimates and Newton steps, as project_cols_body: a rotation only has to be
    // orthogonal to rounding, its angle may be a few ulps off the ideal one
    auto rsqrt_nr = [](double x) {
        double y = __builtin_amdgcn_rsq(x);
        y = y * (1.5 - 0.5 * x * y * y);
        return y * (1.5 - 0.5 * x * y * y);
    };
    auto rcp_nr = [](double x) {
        const double y = __builtin_amdgcn_rcp(x);
        return fma(y, fma(-x, y, 1.0), y);
    };
    auto shfl64 = [](double x, int addr) {  // addr = 4 * source lane
        const int lo = __builtin_amdgcn_ds_bpermute(addr, __double2loint(x)), hi = __builtin_amdgcn_ds_bpermute(addr, __double2hiint(x));
        return __hiloint2double(hi, lo);
    };
    for (int sweep = 0; sweep <= SPEC_MAX_SWEEPS; sweep++) {
        double off = 0.0;
#pragma unroll
        for (int i = 0; i < n; i++) off += i == c ? 0.0 : a[i] * a[i];
        off = group_sum(off);
        if (active) {
            off_stop = off;
            if (off <= SPEC_OFF_TOL * fro) {
                active = false;
                converged = true;
            } else if (sweep == SPEC_MAX_SWEEPS) {
                active = false;
            }
        }
        if (__ballot(active) == 0ull) break;
        if (active) sweeps++;
#pragma unroll
        for (int r = 0; r < m - 1; r++) {
            const int partner = spectrum_partner(m, r, c);
            const int src = ((g * W + partner) & 63) << 2;
            const bool is_lo = c < partner;
            // the three numbers of my pair's rotation: A[lo][lo], A[hi][hi], A[hi][lo] (the entry the lower lane holds)
            const double d_own = spec_pick<n>(a, c), x_own = spec_pick<n>(a, partner);
            const double d_oth = shfl64(d_own, src), x_oth = shfl64(x_own, src);
            double cs = 1.0, sg = 0.0;  // my column <- cs * mine + sg * partner's
            if (active && c < n && partner < n) {
                const double app = is_lo ? d_own : d_oth, aqq = is_lo ? d_oth : d_own, apq = is_lo ? x_own : x_oth;
                if (fabs(apq) > SPEC_APQ_GUARD) {
                    const double theta = (aqq - app) * rcp_nr(2.0 * apq);
                    const double s2 = fma(theta, theta, 1.0);
                    double y = __builtin_amdgcn_rsq(s2);
                    y = y * (1.5 - 0.5 * s2 * y * y);
                    const double root = s2 < 1e300 ? s2 * y : fabs(theta);
                    const double t = copysign(rcp_nr(fabs(theta) + root), theta);
                    cs = rsqrt_nr(t * t + 1.0);
                    const double sn = t * cs;
                    sg = is_lo ? -sn : sn;  // new[lo] = cs old[lo] - sn old[hi];  new[hi] = sn old[lo] + cs old[hi]
                }
            }
            __builtin_amdgcn_wave_barrier();
            S.CS[g][c] = make_double2(cs, sg);
            __builtin_amdgcn_wave_barrier();
            // columns: A <- A J
#pragma unroll
            for (int i = 0; i < n; i++) a[i] = cs * a[i] + sg * shfl64(a[i], src);
            // rows: A <- J^T A, pair by pair (indices are constants after unrolling)
#pragma unroll
            for (int i = 0; i < n; i++) {
                const int pi = spectrum_partner(m, r, i);
                if (pi > i && pi < n) {
                    const double2 ri = S.CS[g][i], rp = S.CS[g][pi];
                    const double ai = a[i], ap_ = a[pi];
                    a[i] = ri.x * ai + ri.y * ap_;
                    a[pi] = rp.x * ap_ + rp.y * ai;
                }
            }
        }
    }
    // eigenvalues = diag(A)
    __builtin_amdgcn_wave_barrier();
    S.L[g][c] = spec_pick<n>(a, c);
    __builtin_amdgcn_wave_barrier();
    if (!elem_ok) return;
    const double* lam = S.L[g];
    if (valid && spectrum) spectrum[(size_t)e * n + (finite ? spectrum_rank<n>(lam, c) : c)] = finite ? lam[c] : 0.0;
    if (c == 0) {
        double r[SPEC_REC];
        spectrum_finish<n>(lam, eps, fro, trace, sweeps, off_stop, converged, finite, r);
#pragma unroll
        for (int f = 0; f < SPEC_REC; f++) rec[(size_t)f * N + col0 + e] = r[f];
    }
}

// ---- nodal stage ---------------------------------------------------------------------------------------------------------------------------
struct SpecDesc  // per selected potential, beside its ForceDesc
{
    int64_t col0;  // first column of its elements in the record buffer
    uint32_t g_off;
    int n_elem, pot, pad;
};
struct SpecAcc
{
    double cnt = 0.0, flg = 0.0, def2 = 0.0, mn = __builtin_huge_val();
    int64_t pos = -1;  // sorted position of the first contribution attaining mn
};
__device__ __forceinline__ int spec_desc_of(const SpecDesc* __restrict__ D, int n_desc, uint32_t g)
{
    int k = 0;
    while (k + 1 < n_desc && g >= D[k + 1].g_off) k++;
    return k;
}
__device__ __forceinline__ void spec_accumulate(SpecAcc& a, const SpecDesc* __restrict__ D, int n_desc, const double* __restrict__ rec, int64_t N, uint32_t g, int64_t j)
{
    const SpecDesc& d = D[spec_desc_of(D, n_desc, g)];
    const int64_t col = d.col0 + (int64_t)((g - d.g_off) % (uint32_t)d.n_elem);
    const int flags = (int)rec[9 * N + col];
    const double dfc = rec[4 * N + col], lo = rec[col];
    a.cnt += 1.0;
    a.flg += (double)(flags & 1);
    a.def2 += dfc * dfc;
    if (!(flags & 2) && lo < a.mn) {  // (positions ascend: the first contribution attaining the minimum stays)
        a.mn = lo;
        a.pos = j;
    }
}
__device__ __forceinline__ void spec_write_row(double* __restrict__ out, uint32_t row, const SpecAcc& a, const SpecDesc* __restrict__ D, int n_desc, const uint32_t* __restrict__ val)
{
    double* o = out + (size_t)SPEC_NODAL * row;
    const bool has = a.pos >= 0;
    o[0] = a.cnt;
    o[1] = a.flg;
    o[2] = has ? a.mn : 0.0;
    o[3] = a.def2;
    o[4] = has ? (double)D[spec_desc_of(D, n_desc, val[a.pos])].pot : -1.0;
}
__global__ __launch_bounds__(BLOCK) void k_spectrum_nodal_init(double* __restrict__ out, int64_t nbr)
{
    const int64_t r = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (r >= nbr) return;
    double* o = out + (size_t)SPEC_NODAL * r;
    o[0] = o[1] = o[2] = o[3] = 0.0;
    o[4] = -1.0;
}
// One lane per sorted position; the lane at the head of a row's run walks the run in order. Runs beyond SPEC_LONG_ROW are handled by the whole wavefront
// their head lies in: lanes stride over the run from its head, then wave_sum's fixed tree (the rule of k_force_segsum). No lane leaves early.
__global__ __launch_bounds__(BLOCK) void k_spectrum_nodal(const uint32_t* __restrict__ key, const uint32_t* __restrict__ val, int64_t total, const SpecDesc* __restrict__ D, int n_desc,
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
    const bool is_long = head && end - i > SPEC_LONG_ROW;
    if (head && !is_long) {
        SpecAcc a;
        for (int64_t j = i; j < end; j++) spec_accumulate(a, D, n_desc, rec, N, val[j], j);
        spec_write_row(out, row, a, D, n_desc, val);
    }
    const unsigned long long any_long = __ballot(is_long);
    unsigned long long m = ((unsigned long long)(uint32_t)__builtin_amdgcn_readfirstlane((int)(any_long >> 32)) << 32) | (uint32_t)__builtin_amdgcn_readfirstlane((int)any_long);
    if (lane == 0 && m) atomicAdd(&stat[0], (uint32_t)__popcll(m));  // (an integer count for the tests; no result depends on it)
    const int64_t wave_first = i - lane;
    while (m) {
        const int src = __ffsll((long long)m) - 1;
        m &= m - 1;
        const int64_t first = wave_first + src;
        const int64_t last = (int64_t)(uint32_t)__shfl((int)(uint32_t)end, src, 64);  // (total < 2^31)
        const uint32_t r = (uint32_t)__shfl((int)row, src, 64);
        SpecAcc a;
        for (int64_t j = first + lane; j < last; j += 64) spec_accumulate(a, D, n_desc, rec, N, val[j], j);
        SpecAcc t;
        t.cnt = wave_sum(a.cnt);
        t.flg = wave_sum(a.flg);
        t.def2 = wave_sum(a.def2);
        const double M = read_lane(-wave_max(-a.mn), 0);
        const double P = -wave_max(a.pos >= 0 && a.mn == M ? -(double)a.pos : -1e300);  // (positions < 2^31: exact)
        if (lane == 0) {
            t.mn = M;
            t.pos = P < 1e299 ? (int64_t)P : -1;
            spec_write_row(out, r, t, D, n_desc, val);
        }
    }
}

// ---- potential stage -----------------------------------------------------------------------------------------------------------------------
// partial[chunk][11]: 0 elements, 1 flagged, 2 lambda_min < 0, 3 non-finite, 4 not converged, 5 smallest lambda_min (+inf: none), 6 column of the first
// element attaining it, 7 largest lambda_max (-inf: none), 8 sum deficit^2, 9 column of the first non-finite element (1e300: none), 10 finite elements
__device__ __forceinline__ void spec_block_argmin(double& v, double& pos, double* sm)
{
    const double M = -block_max(-v, sm);
    const double P = -block_max(v == M && pos < 1e299 ? -pos : -1e300, sm);
    v = M;
    pos = P;
}
__global__ __launch_bounds__(BLOCK) void k_spectrum_pot_chunks(const double* __restrict__ rec, int64_t N, const int32_t* __restrict__ chunks, double* __restrict__ partial)
{
    __shared__ double sm[4];
    const int first = chunks[2 * blockIdx.x], count = chunks[2 * blockIdx.x + 1];
    double cnt = 0.0, flg = 0.0, neg = 0.0, nf = 0.0, nc = 0.0, def2 = 0.0, fin = 0.0;
    double mn = __builtin_huge_val(), mnpos = 1e300, mx = -__builtin_huge_val(), nfpos = 1e300;
    for (int t = threadIdx.x; t < count; t += BLOCK) {
        const size_t e = (size_t)first + t;
        const int flags = (int)rec[9 * N + e];
        const double lo = rec[e], hi = rec[N + e], dfc = rec[4 * N + e];
        cnt += 1.0;
        flg += (double)(flags & 1);
        nc += (double)((flags >> 2) & 1);
        def2 += dfc * dfc;
        if (flags & 2) {
            nf += 1.0;
            if (nfpos > 1e299) nfpos = (double)e;  // (columns ascend)
        } else {
            fin += 1.0;
            neg += lo < 0.0 ? 1.0 : 0.0;
            mx = fmax(mx, hi);
            if (lo < mn) {
                mn = lo;
                mnpos = (double)e;
            }
        }
    }
    double* o = partial + (size_t)blockIdx.x * SPEC_PART;
#define MISTARK_SPEC_SUM(field, k)              \
    {                                           \
        const double s = block_sum(field, sm);  \
        if (threadIdx.x == 0) o[k] = s;         \
    }
    MISTARK_SPEC_SUM(cnt, 0)
    MISTARK_SPEC_SUM(flg, 1)
    MISTARK_SPEC_SUM(neg, 2)
    MISTARK_SPEC_SUM(nf, 3)
    MISTARK_SPEC_SUM(nc, 4)
    MISTARK_SPEC_SUM(def2, 8)
    MISTARK_SPEC_SUM(fin, 10)
#undef MISTARK_SPEC_SUM
    spec_block_argmin(mn, mnpos, sm);
    mx = block_max(mx, sm);
    nfpos = -block_max(-nfpos, sm);
    if (threadIdx.x == 0) {
        o[5] = mn;
        o[6] = mnpos;
        o[7] = mx;
        o[9] = nfpos;
    }
}
// out[p][10] = the partials [chunk0[p], chunk0[p + 1]) of potential p folded in chunk order (every listed potential has at least one chunk)
__global__ __launch_bounds__(BLOCK) void k_spectrum_pot_fold(const double* __restrict__ partial, const int32_t* __restrict__ chunks, const int32_t* __restrict__ chunk0,
                                                            double* __restrict__ out)
{
    __shared__ double sm[4];
    const int c0 = chunk0[blockIdx.x], c1 = chunk0[blockIdx.x + 1];
    double* o = out + (size_t)blockIdx.x * SPEC_POT;
    double sums[SPEC_PART];
#pragma unroll
    for (int k = 0; k < SPEC_PART; k++) {
        if (k == 5 || k == 6 || k == 7 || k == 9) continue;
        sums[k] = sum_partials(partial + (size_t)c0 * SPEC_PART + k, c1 - c0, sm, SPEC_PART);
    }
    double mn = __builtin_huge_val(), mnpos = 1e300, mx = -__builtin_huge_val(), nfpos = 1e300;
    for (int i = threadIdx.x; i < c1 - c0; i += BLOCK) {
        const double* p = partial + (size_t)(c0 + i) * SPEC_PART;
        if (p[5] < mn) {  // (chunks ascend in element order)
            mn = p[5];
            mnpos = p[6];
        }
        mx = fmax(mx, p[7]);
        nfpos = fmin(nfpos, p[9]);
    }
    spec_block_argmin(mn, mnpos, sm);
    mx = block_max(mx, sm);
    nfpos = -block_max(-nfpos, sm);
    if (threadIdx.x == 0) {
        const double base = (double)chunks[2 * c0];  // first column of the potential
        const bool any = sums[10] > 0.0;
        o[0] = sums[0];
        o[1] = sums[1];
        o[2] = sums[2];
        o[3] = sums[3];
        o[4] = sums[4];
        o[5] = any ? mn : 0.0;
        o[6] = any ? mnpos - base : -1.0;
        o[7] = any ? mx : 0.0;
        o[8] = sqrt(sums[8]);
        o[9] = sums[3] > 0.0 ? nfpos - base : -1.0;
    }
}

namespace {
struct Selection
{
    std::vector<int> pots;      // selected potentials with elements, in the caller's order
    std::vector<int> slot_of;   // per entry of the caller's list: index into pots, -1: a potential without elements
    std::vector<ForceDesc> descs;
    std::vector<SpecDesc> sdescs;
    std::vector<int64_t> col0;
    int64_t N = 0, total = 0;   // elements, contributions (element, block)
};
// refusals, prepare() (source 1), the selection and its layout in the record buffer
Selection select(Context& c, const int32_t* pots, int32_t n, int source, const char* who)
{
    if (n < 0) throw Error(std::string(who) + ": bad potential list");
    if (source != 0 && source != 1) throw Error(std::string(who) + ": source is 0 (the element-Hessian pool as it stands) or 1 (a fresh evaluation)");
    std::vector<int> ids;
    if (source == 1) {
        ids = select_potentials(c, pots, n, false, who);
    } else {  // the pool as it stands: any potential, nothing is prepared or evaluated
        if (c.dry) throw Error(std::string(who) + ": registration-only context (mistark_create_dry): nothing can be evaluated");
        if (c.world > 1) throw Error(std::string(who) + ": single-rank accessor (a sharded context holds the elements touching its rows)");
        if (n > 0 && !pots) throw Error(std::string(who) + ": null potential list");
        std::vector<char> seen(c.pots.size(), 0);
        for (int32_t k = 0; k < n; k++) {
            const int p = pots[k];
            if (p < 0 || p >= (int)c.pots.size()) throw Error(std::string(who) + ": bad potential id " + std::to_string(p));
            if (seen[(size_t)p]) throw Error(std::string(who) + ": potential '" + c.pots[(size_t)p].name + "' is listed twice");
            seen[(size_t)p] = 1;
            ids.push_back(p);
        }
        if (!c.have_hessians) throw Error(std::string(who) + ": no element Hessians (call eval with MISTARK_EVAL_P_G_H first, or ask for source 1)");
        for (int p : ids)
            if (c.lazy_active && c.pots[(size_t)p].lazy_capable)
                throw Error(std::string(who) + ": element Hessians of '" + c.pots[(size_t)p].name +
                            "' were evaluated on the lazy path (float blocks only); evaluate without lazy_eval, or ask for source 1");
    }
    Selection S;
    for (int p : ids) {
        const Potential& P = c.pots[(size_t)p];
        if (P.NB < 1 || P.NB > 8) throw Error(std::string(who) + ": unsupported block count");
        if (P.n_elem <= 0) {
            S.slot_of.push_back(-1);
            continue;
        }
        if (P.args.elem_list || P.args.e_count != P.n_elem) throw Error(std::string(who) + ": single-rank accessor");
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
        S.slot_of.push_back((int)S.pots.size());
        S.pots.push_back(p);
        S.descs.push_back(d);
        S.sdescs.push_back(SpecDesc{S.N, (uint32_t)S.total, P.n_elem, p, 0});
        S.col0.push_back(S.N);
        S.N += P.n_elem;
        S.total += (int64_t)P.NB * P.n_elem;
    }
    if (S.total >= (1ll << 31)) throw Error(std::string(who) + ": too many contributions");
    return S;
}

template <int NB>
void launch_cols(Context& c, const double* H, int n_elem, int n_pool, double eps, double* rec, int64_t N, int64_t col0, double* spectrum)
{
    constexpr int EPW = 64 / ((3 * NB + 1) & ~1);
    const int waves = (n_elem + EPW - 1) / EPW;
    hipLaunchKernelGGL((k_spectrum_cols<NB>), dim3((waves + 3) / 4), dim3(BLOCK), 0, c.stream, H, n_elem, n_pool, eps, rec, N, col0, spectrum);
}
// stage 1: rec[10][S.N]; spectrum (device, [n_elem][3 NB]) only for a selection of one potential
void rows_stage(Context& c, const Selection& S, int source, double eps, double* rec, double* spectrum)
{
    if (source == 1) {  // the private pool holds one potential at a time: sized by the largest
        size_t h = 0, g = 0, e = 0;
        for (int p : S.pots) {
            const Potential& P = c.pots[(size_t)p];
            h = std::max(h, (size_t)9 * P.NB * P.NB * P.n_elem);
            g = std::max(g, (size_t)3 * P.NB * P.n_elem);
            e = std::max(e, (size_t)P.n_elem);
        }
        c.spr_H.ensure(h);
        c.spr_gpool.ensure(g);
        c.spr_elemE.ensure(e);
    }
    for (size_t k = 0; k < S.pots.size(); k++) {
        const Potential& P = c.pots[(size_t)S.pots[k]];
        const double* H = c.elemH.p + P.h_off;
        int n_pool = P.n_key;
        if (source == 1) {
            launch_hessian_elements(c, P, c.spr_H.p, c.spr_elemE.p, c.spr_gpool.p);
            H = c.spr_H.p;
            n_pool = P.n_elem;
        }
        switch (P.NB) {
            case 1: launch_cols<1>(c, H, P.n_elem, n_pool, eps, rec, S.N, S.col0[k], spectrum); break;
            case 2: launch_cols<2>(c, H, P.n_elem, n_pool, eps, rec, S.N, S.col0[k], spectrum); break;
            case 3: launch_cols<3>(c, H, P.n_elem, n_pool, eps, rec, S.N, S.col0[k], spectrum); break;
            case 4: launch_cols<4>(c, H, P.n_elem, n_pool, eps, rec, S.N, S.col0[k], spectrum); break;
            case 5: launch_cols<5>(c, H, P.n_elem, n_pool, eps, rec, S.N, S.col0[k], spectrum); break;
            case 6: launch_cols<6>(c, H, P.n_elem, n_pool, eps, rec, S.N, S.col0[k], spectrum); break;
            case 7: launch_cols<7>(c, H, P.n_elem, n_pool, eps, rec, S.N, S.col0[k], spectrum); break;
            default: launch_cols<8>(c, H, P.n_elem, n_pool, eps, rec, S.N, S.col0[k], spectrum); break;
        }
    }
    MS_CHECK(hipGetLastError());
    c.n_spectrum_reports++;
}
// stage 2: out[nbr][5] from the records of stage 1
void nodal_stage(Context& c, const Selection& S, const double* rec, double* out)
{
    const int64_t n = S.total;
    c.spr_key.ensure((size_t)n);
    c.spr_key_alt.ensure((size_t)n);
    c.spr_val.ensure((size_t)n);
    c.spr_val_alt.ensure((size_t)n);
    c.spr_stat.ensure(2);
    c.spr_desc.ensure(S.descs.size() * sizeof(ForceDesc));
    c.spr_sdesc.ensure(S.sdescs.size() * sizeof(SpecDesc));
    h2d_small(c, c.spr_desc.p, S.descs.data(), S.descs.size() * sizeof(ForceDesc));
    h2d_small(c, c.spr_sdesc.p, S.sdescs.data(), S.sdescs.size() * sizeof(SpecDesc));
    hipLaunchKernelGGL(k_force_keys, dim3(grid_for(n)), dim3(BLOCK), 0, c.stream, (const ForceDesc*)c.spr_desc.p, (int)S.descs.size(), n, c.spr_key.p, c.spr_val.p);
    int bits = 1;
    while (bits < 32 && (1ll << bits) <= c.nbr) bits++;
    size_t tmp = 0;
    hipcub::DoubleBuffer<uint32_t> dk(c.spr_key.p, c.spr_key_alt.p), dv(c.spr_val.p, c.spr_val_alt.p);
    MS_CHECK(hipcub::DeviceRadixSort::SortPairs(nullptr, tmp, dk, dv, (int)n, 0, bits, c.stream));
    c.spr_cub_tmp.ensure(tmp);
    MS_CHECK(hipcub::DeviceRadixSort::SortPairs(c.spr_cub_tmp.p, tmp, dk, dv, (int)n, 0, bits, c.stream));  // (stable: equal rows keep the contribution order)
    fill_async(c.stream, c.spr_stat.p, 0, 2 * sizeof(uint32_t));
    hipLaunchKernelGGL(k_spectrum_nodal_init, dim3(grid_for(c.nbr)), dim3(BLOCK), 0, c.stream, out, (int64_t)c.nbr);  // (rows nobody touches: zeros, potential -1)
    hipLaunchKernelGGL(k_spectrum_nodal, dim3(grid_for(n)), dim3(BLOCK), 0, c.stream, (const uint32_t*)dk.Current(), (const uint32_t*)dv.Current(), n, (const SpecDesc*)c.spr_sdesc.p,
                       (int)S.sdescs.size(), rec, S.N, out, c.spr_stat.p);
    MS_CHECK(hipGetLastError());
    c.spr_stat_valid = true;
}
// stage 3: out[S.pots.size()][10] (device) from the records of stage 1
void pots_stage(Context& c, const Selection& S, const double* rec, double* out)
{
    std::vector<int32_t> table, chunk0;
    for (size_t k = 0; k < S.pots.size(); k++) {
        chunk0.push_back((int32_t)(table.size() / 2));
        cut_chunks(table, S.col0[k], c.pots[(size_t)S.pots[k]].n_elem, SPEC_CHUNK);
    }
    const int64_t n_chunks = (int64_t)table.size() / 2;
    chunk0.push_back((int32_t)n_chunks);
    table.insert(table.end(), chunk0.begin(), chunk0.end());
    c.spr_chunks.ensure(table.size());
    c.spr_partial.ensure((size_t)SPEC_PART * n_chunks);
    h2d_staged(c, c.spr_chunks.p, table.data(), table.size() * sizeof(int32_t));
    hipLaunchKernelGGL(k_spectrum_pot_chunks, dim3((unsigned)n_chunks), dim3(BLOCK), 0, c.stream, rec, S.N, (const int32_t*)c.spr_chunks.p, c.spr_partial.p);
    hipLaunchKernelGGL(k_spectrum_pot_fold, dim3((unsigned)S.pots.size()), dim3(BLOCK), 0, c.stream, (const double*)c.spr_partial.p, (const int32_t*)c.spr_chunks.p,
                       (const int32_t*)c.spr_chunks.p + 2 * n_chunks, out);
    MS_CHECK(hipGetLastError());
    MS_CHECK(hipStreamSynchronize(c.stream));  // (the table is a temporary)
    c.n_spectrum_chunks = n_chunks;
}
}  // namespace

void spectrum_rows_host(Context& c, int pot, int source, double eps, double* out, double* spectrum, int64_t* n_elem, int32_t* nb)
{
    const int32_t id = pot;
    const Selection S = select(c, &id, 1, source, "mistark_potential_spectrum_report");
    const Potential& P = c.pots[(size_t)pot];
    const int n = 3 * P.NB;
    if (n_elem) *n_elem = P.n_elem;
    if (nb) *nb = P.NB;
    if ((!out && !spectrum) || S.N == 0) return;  // (an empty table launches nothing; null outputs: a size query)
    c.spr_rec.ensure((size_t)SPEC_REC * S.N);
    if (spectrum) c.spr_spec.ensure((size_t)n * S.N);
    rows_stage(c, S, source, eps, c.spr_rec.p, spectrum ? c.spr_spec.p : nullptr);
    std::vector<double> tmp((size_t)SPEC_REC * S.N);
    MS_CHECK(hipMemcpyAsync(tmp.data(), c.spr_rec.p, tmp.size() * sizeof(double), hipMemcpyDeviceToHost, c.stream));
    if (spectrum) MS_CHECK(hipMemcpyAsync(spectrum, c.spr_spec.p, (size_t)n * S.N * sizeof(double), hipMemcpyDeviceToHost, c.stream));
    MS_CHECK(hipStreamSynchronize(c.stream));
    if (out)
        for (int64_t e = 0; e < S.N; e++)
            for (int f = 0; f < SPEC_REC; f++) out[(size_t)e * SPEC_REC + f] = tmp[(size_t)f * S.N + e];
}

void spectrum_nodal_host(Context& c, const int32_t* pots, int32_t n, int source, double eps, double* out_host)
{
    if (!out_host) throw Error("mistark_nodal_spectrum: null output");
    const Selection S = select(c, pots, n, source, "mistark_nodal_spectrum");
    if (S.total == 0) {
        for (int64_t r = 0; r < c.nbr; r++) {
            double* o = out_host + (size_t)SPEC_NODAL * r;
            o[0] = o[1] = o[2] = o[3] = 0.0;
            o[4] = -1.0;
        }
        return;
    }
    c.spr_rec.ensure((size_t)SPEC_REC * S.N);
    c.spr_nodal.ensure((size_t)SPEC_NODAL * c.nbr);
    rows_stage(c, S, source, eps, c.spr_rec.p, nullptr);
    nodal_stage(c, S, c.spr_rec.p, c.spr_nodal.p);
    MS_CHECK(hipMemcpyAsync(out_host, c.spr_nodal.p, (size_t)SPEC_NODAL * c.nbr * sizeof(double), hipMemcpyDeviceToHost, c.stream));
    MS_CHECK(hipStreamSynchronize(c.stream));
}

void spectrum_pots_host(Context& c, const int32_t* pots, int32_t n, int source, double eps, double* out)
{
    const Selection S = select(c, pots, n, source, "mistark_spectrum_potential_report");
    if (n == 0) return;
    if (!out) throw Error("mistark_spectrum_potential_report: null output");
    std::vector<double> tmp((size_t)SPEC_POT * std::max<size_t>(S.pots.size(), 1));
    if (S.N > 0) {
        c.spr_rec.ensure((size_t)SPEC_REC * S.N);
        c.spr_pot.ensure((size_t)SPEC_POT * S.pots.size());
        rows_stage(c, S, source, eps, c.spr_rec.p, nullptr);
        pots_stage(c, S, c.spr_rec.p, c.spr_pot.p);
        MS_CHECK(hipMemcpyAsync(tmp.data(), c.spr_pot.p, (size_t)SPEC_POT * S.pots.size() * sizeof(double), hipMemcpyDeviceToHost, c.stream));
        MS_CHECK(hipStreamSynchronize(c.stream));
    }
    for (int32_t k = 0; k < n; k++) {
        double* o = out + (size_t)k * SPEC_POT;
        const int s = S.slot_of[(size_t)k];
        if (s < 0) {  // a potential without elements
            std::fill(o, o + SPEC_POT, 0.0);
            o[6] = o[9] = -1.0;
        } else {
            std::copy(tmp.begin() + (size_t)s * SPEC_POT, tmp.begin() + (size_t)(s + 1) * SPEC_POT, o);
        }
    }
}

void spectrum_record_step(Context& c, const int32_t* pots, int32_t n, double eps)
{
    Context::SpectrumSlot& s = c.spr_slot;
    s.N = -1;
    const Selection S = select(c, pots, n, 1, "spectrum report");
    s.slot_of = S.slot_of;
    s.col0 = S.col0;
    s.n_elem.clear();
    for (int p : S.pots) s.n_elem.push_back(c.pots[(size_t)p].n_elem);
    s.nbr = c.nbr;
    if (S.N > 0) {
        s.rec.ensure((size_t)SPEC_REC * S.N);
        s.nodal.ensure((size_t)SPEC_NODAL * c.nbr);
        s.pot.ensure((size_t)SPEC_POT * S.pots.size());
        rows_stage(c, S, 1, eps, s.rec.p, nullptr);
        nodal_stage(c, S, s.rec.p, s.nodal.p);
        pots_stage(c, S, s.rec.p, s.pot.p);
    }
    s.N = S.N;
}
void spectrum_fetch_summary(Context& c, int32_t n, double* pots_out, double* nodal_out, int64_t n_rows)
{
    const Context::SpectrumSlot& s = c.spr_slot;
    if (s.N < 0) throw Error("spectrum report: nothing recorded");
    if (pots_out) {
        if (n != (int32_t)s.slot_of.size()) throw Error("spectrum report: " + std::to_string(s.slot_of.size()) + " potentials were recorded, the caller asks for " + std::to_string(n));
        std::vector<double> tmp((size_t)SPEC_POT * std::max<size_t>(s.n_elem.size(), 1));
        if (s.N > 0) {
            MS_CHECK(hipMemcpyAsync(tmp.data(), s.pot.p, (size_t)SPEC_POT * s.n_elem.size() * sizeof(double), hipMemcpyDeviceToHost, c.stream));
            MS_CHECK(hipStreamSynchronize(c.stream));
        }
        for (int32_t k = 0; k < n; k++) {
            double* o = pots_out + (size_t)k * SPEC_POT;
            const int i = s.slot_of[(size_t)k];
            if (i < 0) {
                std::fill(o, o + SPEC_POT, 0.0);
                o[6] = o[9] = -1.0;
            } else {
                std::copy(tmp.begin() + (size_t)i * SPEC_POT, tmp.begin() + (size_t)(i + 1) * SPEC_POT, o);
            }
        }
    }
    if (nodal_out) {
        if (n_rows != s.nbr) throw Error("spectrum report: the recorded array has " + std::to_string(s.nbr) + " rows, the caller asks for " + std::to_string(n_rows));
        if (s.N == 0) {
            for (int64_t r = 0; r < n_rows; r++) {
                double* o = nodal_out + (size_t)SPEC_NODAL * r;
                o[0] = o[1] = o[2] = o[3] = 0.0;
                o[4] = -1.0;
            }
        } else {
            MS_CHECK(hipMemcpyAsync(nodal_out, s.nodal.p, (size_t)SPEC_NODAL * n_rows * sizeof(double), hipMemcpyDeviceToHost, c.stream));
            MS_CHECK(hipStreamSynchronize(c.stream));
        }
    }
}
void spectrum_fetch_rows(Context& c, int32_t index, double* rows, int64_t* n_rows)
{
    const Context::SpectrumSlot& s = c.spr_slot;
    if (s.N < 0) throw Error("spectrum report: nothing recorded");
    if (index < 0 || index >= (int32_t)s.slot_of.size()) throw Error("spectrum report: no recorded potential " + std::to_string(index));
    const int i = s.slot_of[(size_t)index];
    const int64_t ne = i < 0 ? 0 : s.n_elem[(size_t)i];
    if (n_rows) *n_rows = ne;
    if (!rows || ne == 0) return;
    std::vector<double> tmp((size_t)SPEC_REC * s.N);
    MS_CHECK(hipMemcpyAsync(tmp.data(), s.rec.p, tmp.size() * sizeof(double), hipMemcpyDeviceToHost, c.stream));
    MS_CHECK(hipStreamSynchronize(c.stream));
    for (int64_t e = 0; e < ne; e++)
        for (int f = 0; f < SPEC_REC; f++) rows[(size_t)e * SPEC_REC + f] = tmp[(size_t)f * s.N + s.col0[(size_t)i] + e];
}

int64_t spectrum_long_rows(Context& c)
{
    if (!c.spr_stat_valid) return 0;
    uint32_t v[2] = {0, 0};
    fetch(c, v, c.spr_stat.p, sizeof(v));
    return (int64_t)v[0];
}

}  // namespace mistark
