// linsys_report.hip — opt-in linear-system report: Lanczos with full reorthogonalisation on the assembled matrix as it stands (the static and the dynamic
// part together, the state after mistark_assemble), its Ritz values with residual bounds, the extreme Ritz vectors and who carries them (record layouts,
// the shared arithmetic and the method: linsys_report.hpp).
//
// A pipeline of its own beside eval() and pcg(): it READS the matrix, the permutation and the element-Hessian pool and writes only the Context::lsr_*
// buffers (and, through spmv_device, the SpMV's own scratch of the contact part, as mistark_spmv does). No buffer of PCG is touched.
//   diagonal : k_lsr_chol, one lane per block row: the stored float diagonal block (load_diag_block's sum of the two parts, restated here because that
//              helper is local to solve.hip) promoted to double, its 3x3 Cholesky, trace and smallest squared pivot; folded on the host in row order
//   operator : op 0 w = A v by spmv_device; op 1 k_lsr_solve_Lt (x = L^-T v), spmv_device, k_lsr_solve_L (w = L^-1 y), one lane per block row.
//              Every vector of the iteration lives in the SOLVER's row numbering (Context::perm_active); only the start vector and the outputs are permuted
//   basis    : (m + 1) rows of ld = even(n) doubles in lsr_V, so that every row starts 16-byte aligned
//   multi-dot: c = V^T w. Workgroup g owns the slab [LSR_SLAB g, LSR_SLAB (g + 1)) of the rows; each of its four wavefronts keeps the slab of w in
//              registers (eight double2 per lane) and streams the basis slabs i = wave, wave + 4, ... past it with 16-byte loads, once each; a wavefront's
//              sum goes to part[i][g]. k_lsr_fold sums part[i][0 .. G) in a fixed order (lane l of one wavefront takes the workgroups l, l + 64, ...
//              in ascending order, then the wavefront's fixed tree). G depends on n alone: two runs give the same bits.
//   update   : w -= V c, every basis slab read once, coefficients from the device
//   control  : alpha, beta, T_norm, the step count and the stop flag live in LsrCtrl on the device (as PcgCtrl does for PCG); after the stop flag is set the
//              remaining launches of the report's own kernels do nothing; the host reads the block back after the last step and looks at the stop
//              flag every LSR_STOP_CHECK steps in between, to leave the loop early.
// No floating-point atomics anywhere. The Ritz pairs, the records and the folds over rows and elements are host code (linsys_report.hpp).
#include "kernels_common.hpp"
#include "linsys_report.hpp"

namespace mistark {

constexpr int LSR_STOP_CHECK = 32;  // steps between two looks of the host at the stop flag
constexpr int LSR_SLAB = 1024;  // doubles of a vector per workgroup: 64 lanes x 8 double2 per wavefront, 256 threads x 2 double2 in the update

struct LsrCtrl
{
    int stop, flags, k, pad_;
    double t_norm;
    double alpha[LINSYS_MAX_M], beta[LINSYS_MAX_M];
};
constexpr size_t LSR_CTRL_DOUBLES = (sizeof(LsrCtrl) + 7) / 8;

// elements i, i + 1 (i even) of a vector of n doubles whose base is 16-byte aligned; zeros beyond n
__device__ __forceinline__ double2 lsr_load2(const double* __restrict__ v, int64_t i, int64_t n)
{
    if (i + 1 < n) return *reinterpret_cast<const double2*>(v + i);
    return make_double2(i < n ? v[i] : 0.0, 0.0);
}
__device__ __forceinline__ void lsr_store2(double* __restrict__ v, int64_t i, int64_t n, double2 a)
{
    if (i + 1 < n) *reinterpret_cast<double2*>(v + i) = a;
    else if (i < n) v[i] = a.x;
}

// diag[row'][0..1] = trace, smallest squared pivot with row' the caller's block row; L[row][6] by solver row
__global__ __launch_bounds__(BLOCK) void k_lsr_chol(const float* __restrict__ vals, const int32_t* __restrict__ diag_slot, const float* __restrict__ vals_dyn,
                                                    const int32_t* __restrict__ diag_slot_dyn, const int32_t* __restrict__ caller_row, int64_t nbr, double* __restrict__ L,
                                                    double* __restrict__ diag)
{
    const int64_t r = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (r >= nbr) return;
    float m[9];
    const uint32_t s = (uint32_t)diag_slot[r];
#pragma unroll
    for (int k = 0; k < 9; k++) m[k] = vals[tile_val_index(s, k)];
    if (vals_dyn) {
        const int32_t sd = diag_slot_dyn[r];
        if (sd >= 0) {
#pragma unroll
            for (int k = 0; k < 9; k++) m[k] += vals_dyn[tile_val_index((uint32_t)sd, k)];
        }
    }
    const double a[6] = {(double)m[0], (double)m[1], (double)m[2], (double)m[4], (double)m[5], (double)m[8]};
    double l[6] = {1.0, 0.0, 1.0, 0.0, 0.0, 1.0}, piv;
    if (!linsys_chol3(a, l, piv)) {
        l[0] = l[2] = l[5] = 1.0;
        l[1] = l[3] = l[4] = 0.0;
    }
#pragma unroll
    for (int k = 0; k < 6; k++) L[6 * r + k] = l[k];
    const int64_t cr = caller_row ? (int64_t)caller_row[r] : r;
    diag[2 * cr] = a[0] + a[3] + a[5];
    diag[2 * cr + 1] = piv;
}
// out = L^-T in (TRANSPOSED) or L^-1 in, block row by block row; in == out is allowed
template <bool TRANSPOSED>
__global__ __launch_bounds__(BLOCK) void k_lsr_solve(const double* __restrict__ L, const double* in, double* out, int64_t nbr, const LsrCtrl* __restrict__ ctrl)
{
    if (ctrl && ctrl->stop) return;
    const int64_t r = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (r >= nbr) return;
    double l[6];
#pragma unroll
    for (int k = 0; k < 6; k++) l[k] = L[6 * r + k];
    const double v[3] = {in[3 * r], in[3 * r + 1], in[3 * r + 2]};
    double x[3];
    if (TRANSPOSED) linsys_solve_Lt(l, v, x);
    else linsys_solve_L(l, v, x);
    out[3 * r] = x[0];
    out[3 * r + 1] = x[1];
    out[3 * r + 2] = x[2];
}

// part[(i - first) * G + g] = sum over workgroup g's slab of V[i][.] * w[.], i = first .. first + count - 1 (V rows ld apart)
__global__ __launch_bounds__(BLOCK) void k_lsr_multidot(const double* __restrict__ V, int64_t ld, int first, int count, const double* __restrict__ w, int64_t n,
                                                        double* __restrict__ part, const LsrCtrl* __restrict__ ctrl)
{
    if (ctrl && ctrl->stop) return;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t base = (int64_t)blockIdx.x * LSR_SLAB + 2 * lane;
    double2 wr[8];
#pragma unroll
    for (int q = 0; q < 8; q++) wr[q] = lsr_load2(w, base + 128 * q, n);
    for (int i = wave; i < count; i += 4) {
        const double* __restrict__ v = V + (size_t)(first + i) * (size_t)ld;
        double2 a[8];
#pragma unroll
        for (int q = 0; q < 8; q++) a[q] = lsr_load2(v, base + 128 * q, n);
        double s = 0.0;
#pragma unroll
        for (int q = 0; q < 8; q++) s = fma(a[q].y, wr[q].y, fma(a[q].x, wr[q].x, s));
        s = wave_sum(s);
        if (lane == 0) part[(size_t)i * gridDim.x + blockIdx.x] = s;
    }
}
enum { LSR_FOLD_COEF = 0, LSR_FOLD_ALPHA = 1, LSR_FOLD_BETA = 2 };
// c[i] = sum_g part[i][g] in a fixed order, one wavefront per i: lane l adds the workgroups l, l + 64, ... in ascending order, then the wavefront's fixed
// tree. (One lane adding all G partials one after the other is a chain of dependent latencies: ~90 us per fold at configs[3], 32.5 ms instead of 14.1 ms
// for m = 64.) ALPHA (count 1, step j): alpha_j and the coefficients of w -= beta_{j-1} v_{j-1} + alpha_j v_j;
// BETA (count 1, step j): beta_j = sqrt(sum), T_norm, the step count and the stop rule.
__global__ __launch_bounds__(BLOCK) void k_lsr_fold(const double* __restrict__ part, int G, int count, int mode, int j, double* __restrict__ c, LsrCtrl* __restrict__ ctrl)
{
    if (ctrl && ctrl->stop) return;
    const int i = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (i >= count) return;  // (whole wavefront)
    const double* __restrict__ p = part + (size_t)i * G;
    double s = 0.0;
    for (int g = lane; g < G; g += 64) s += p[g];
    s = wave_sum(s);
    if (lane != 0) return;
    if (mode == LSR_FOLD_COEF) {
        c[i] = s;
    } else if (mode == LSR_FOLD_ALPHA) {
        ctrl->alpha[j] = s;
        if (j > 0) {
            c[0] = ctrl->beta[j - 1];
            c[1] = s;
        } else {
            c[0] = s;
        }
    } else {
        const double beta = sqrt(s), alpha = ctrl->alpha[j];
        ctrl->beta[j] = beta;
        ctrl->k = j + 1;
        const double t = fabs(alpha) + beta + (j > 0 ? ctrl->beta[j - 1] : 0.0);
        const double tn = t > ctrl->t_norm ? t : ctrl->t_norm;
        if (!isfinite(alpha) || !isfinite(beta)) {
            ctrl->flags |= LINSYS_FLAG_NONFINITE;
            ctrl->stop = 1;
        } else {
            ctrl->t_norm = tn;
            if (beta <= LINSYS_BREAKDOWN * tn) {
                ctrl->flags |= LINSYS_FLAG_EXHAUSTED;
                ctrl->stop = 1;
            }
        }
    }
}
// w -= sum_i c[i] V[first + i][.] (sign = -1), the terms added in the order of i
__global__ __launch_bounds__(BLOCK) void k_lsr_update(const double* __restrict__ V, int64_t ld, int first, int count, const double* __restrict__ c, double* __restrict__ w, int64_t n,
                                                      const LsrCtrl* __restrict__ ctrl)
{
    if (ctrl && ctrl->stop) return;
    const int64_t i0 = (int64_t)blockIdx.x * LSR_SLAB + 2 * threadIdx.x, i1 = i0 + 2 * BLOCK;
    double2 s0 = make_double2(0.0, 0.0), s1 = s0;
#pragma unroll 4
    for (int i = 0; i < count; i++) {
        const double ci = c[i];
        const double* __restrict__ v = V + (size_t)(first + i) * (size_t)ld;
        const double2 a0 = lsr_load2(v, i0, n), a1 = lsr_load2(v, i1, n);
        s0.x = fma(ci, a0.x, s0.x);
        s0.y = fma(ci, a0.y, s0.y);
        s1.x = fma(ci, a1.x, s1.x);
        s1.y = fma(ci, a1.y, s1.y);
    }
    double2 w0 = lsr_load2(w, i0, n), w1 = lsr_load2(w, i1, n);
    w0.x -= s0.x; w0.y -= s0.y; w1.x -= s1.x; w1.y -= s1.y;
    lsr_store2(w, i0, n, w0);
    lsr_store2(w, i1, n, w1);
}
// v_{j+1} = w / beta_j
__global__ __launch_bounds__(BLOCK) void k_lsr_normalise(const double* __restrict__ w, double* __restrict__ v, int64_t n, int j, const LsrCtrl* __restrict__ ctrl)
{
    if (ctrl->stop) return;
    const double beta = ctrl->beta[j];
    const int64_t i0 = (int64_t)blockIdx.x * LSR_SLAB + 2 * threadIdx.x, i1 = i0 + 2 * BLOCK;
    double2 a = lsr_load2(w, i0, n), b = lsr_load2(w, i1, n);
    a.x /= beta; a.y /= beta; b.x /= beta; b.y /= beta;
    lsr_store2(v, i0, n, a);
    lsr_store2(v, i1, n, b);
}
// the per-row shares of one Ritz vector: out[row'][4] = |u_r|^2, |x_r|, trace of D_r, smallest squared pivot of D_r; u, x by solver row, row' the caller's
__global__ __launch_bounds__(BLOCK) void k_lsr_nodal(const double* __restrict__ u, const double* __restrict__ x, const double* __restrict__ diag,
                                                     const int32_t* __restrict__ caller_row, int64_t nbr, double* __restrict__ out)
{
    const int64_t r = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (r >= nbr) return;
    const int64_t cr = caller_row ? (int64_t)caller_row[r] : r;
    const double u0 = u[3 * r], u1 = u[3 * r + 1], u2 = u[3 * r + 2], x0 = x[3 * r], x1 = x[3 * r + 1], x2 = x[3 * r + 2];
    out[4 * cr] = u0 * u0 + u1 * u1 + u2 * u2;
    out[4 * cr + 1] = sqrt(x0 * x0 + x1 * x1 + x2 * x2);
    out[4 * cr + 2] = diag[2 * cr];
    out[4 * cr + 3] = diag[2 * cr + 1];
}
// s += a in double-double: (hi, lo) with the rounding error of the sum kept in lo
__device__ __forceinline__ void lsr_dd_add(double& hi, double& lo, double a_hi, double a_lo)
{
#pragma clang fp contract(off)
    const double s = hi + a_hi;
    const double bb = s - hi;
    lo += ((hi - (s - bb)) + (a_hi - bb)) + a_lo;
    hi = s;
}
// the per-element quadratic forms q[e] = x_e^T H_e x_e and whether any stored entry of H_e is non-zero; x in DoF order; pool H[(a NB + b) n_pool + e][3][3].
// An extreme mode is smooth where its potential is soft: x_a ~ x_b across a spring and the 36 terms cancel to a small q_e. The terms are therefore formed
// and added in double-double (exact products by fma, two-sum), so that q_e is the rounded value of the exact form of the stored entries.
__global__ __launch_bounds__(BLOCK) void k_lsr_quad(const double* __restrict__ H, int n_elem, int n_pool, int NB, const int32_t* __restrict__ conn, int stride,
                                                    const int* __restrict__ dof_col, const int* __restrict__ dof_row_off, const double* __restrict__ x, double* __restrict__ q,
                                                    uint8_t* __restrict__ nonzero)
{
#pragma clang fp contract(off)
    const int e = blockIdx.x * BLOCK + threadIdx.x;
    if (e >= n_elem) return;
    const size_t hs = (size_t)n_pool * 9;
    double hi = 0.0, lo = 0.0;
    bool nz = false;
    for (int a = 0; a < NB; a++) {  // (the node vectors are read again per block pair: they stay in cache, and no indexed array goes to scratch)
        const double* __restrict__ xa = x + 3 * ((int64_t)dof_row_off[a] + conn[(size_t)e * stride + dof_col[a]]);
        const double xa3[3] = {xa[0], xa[1], xa[2]};
        for (int b = 0; b < NB; b++) {
            const double* __restrict__ xb = x + 3 * ((int64_t)dof_row_off[b] + conn[(size_t)e * stride + dof_col[b]]);
            const double xb3[3] = {xb[0], xb[1], xb[2]};
            const double* __restrict__ h = H + (size_t)(a * NB + b) * hs + (size_t)e * 9;
#pragma unroll
            for (int i = 0; i < 3; i++)
#pragma unroll
                for (int jj = 0; jj < 3; jj++) {
                    const double v = h[3 * i + jj];
                    nz = nz || v != 0.0;
                    const double p_hi = xa3[i] * v, p_lo = __builtin_fma(xa3[i], v, -p_hi);       // xa v, exactly
                    const double t_hi = p_hi * xb3[jj];
                    const double t_lo = __builtin_fma(p_hi, xb3[jj], -t_hi) + p_lo * xb3[jj];     // (xa v) xb to about 2^-104
                    lsr_dd_add(hi, lo, t_hi, t_lo);
                }
        }
    }
    q[e] = hi + lo;
    nonzero[e] = nz ? 1 : 0;
}

namespace {
struct Run  // one Lanczos run and what the host made of it
{
    int op = 0, m = 0, k = 0, flags = 0;
    int64_t n = 0, ld = 0;
    int G = 1;
    double t_norm = 0.0;
    std::vector<double> alpha, beta;
    LinsysDiag D;
};

void refuse(Context& c, int op, int m, const char* who)
{
    if (c.dry) throw Error(std::string(who) + ": registration-only context (mistark_create_dry): nothing can be evaluated");
    if (c.world > 1) throw Error(std::string(who) + ": single-rank accessor (a sharded context holds its own block rows in local numbering)");
    if (!c.have_matrix) throw Error(std::string(who) + ": matrix not assembled (call mistark_assemble first)");
    if (op != LINSYS_A && op != LINSYS_JACOBI) throw Error(std::string(who) + ": operator is 0 (A) or 1 (L^-1 A L^-T, the block-Jacobi preconditioned matrix)");
    if (m < 1 || m > LINSYS_MAX_M) throw Error(std::string(who) + ": m = " + std::to_string(m) + " is out of range (1.." + std::to_string(LINSYS_MAX_M) + ")");
}
const LsrCtrl* ctrl_of(Context& c) { return reinterpret_cast<const LsrCtrl*>(c.lsr_ctrl.p); }
LsrCtrl* ctrl_mut(Context& c) { return reinterpret_cast<LsrCtrl*>(c.lsr_ctrl.p); }
const int32_t* caller_rows(Context& c) { return c.perm_active ? (const int32_t*)c.iperm.p : nullptr; }

// w = B v in solver numbering (t, y: scratch of one vector each); ctrl may be null
void apply_operator(Context& c, int op, const double* v, double* w, const LsrCtrl* ctrl)
{
    if (op == LINSYS_A) {
        spmv_device(c, v, w, nullptr, nullptr);
        return;
    }
    hipLaunchKernelGGL((k_lsr_solve<true>), dim3(grid_for(c.nbr)), dim3(BLOCK), 0, c.stream, (const double*)c.lsr_L.p, v, c.lsr_t.p, c.nbr, ctrl);
    spmv_device(c, c.lsr_t.p, c.lsr_y.p, nullptr, nullptr);
    hipLaunchKernelGGL((k_lsr_solve<false>), dim3(grid_for(c.nbr)), dim3(BLOCK), 0, c.stream, (const double*)c.lsr_L.p, (const double*)c.lsr_y.p, w, c.nbr, ctrl);
}

// the diagonal stage and, unless it refuses operator 1, the iteration; one read-back of the control block at the end
Run lanczos(Context& c, int op, int m, const double* start_host, const char* who)
{
    Run R;
    R.op = op;
    R.m = m;
    R.n = c.ndofs;
    const int64_t n = c.ndofs, nbr = c.nbr;
    if (n != 3 * nbr || n < 1) throw Error(std::string(who) + ": the matrix has no rows");
    R.ld = (n + 1) & ~(int64_t)1;
    R.G = grid_for(n, LSR_SLAB);
    // start vector in DoF order, normalised on the host
    std::vector<double> v0((size_t)n);
    double nrm2 = 0.0, comp = 0.0;  // (compensated: the norm is the correctly rounded one up to an ulp whatever n is, so that a caller can restate v_0)
    for (int64_t i = 0; i < n; i++) {
        v0[(size_t)i] = start_host ? start_host[i] : linsys_start_value((uint64_t)i);
        const volatile double y = v0[(size_t)i] * v0[(size_t)i] - comp;
        const volatile double t = nrm2 + y;
        comp = (t - nrm2) - y;
        nrm2 = t;
    }
    const double nrm = std::sqrt(nrm2);
    if (!(nrm > 0.0) || !std::isfinite(nrm)) throw Error(std::string(who) + ": the start vector is zero or not finite");
    for (double& x : v0) x /= nrm;

    const int kmax = (int)std::min<int64_t>(m, n);
    c.lsr_V.ensure((size_t)(m + 1) * (size_t)R.ld);
    c.lsr_w.ensure((size_t)R.ld);
    c.lsr_t.ensure((size_t)R.ld);
    c.lsr_y.ensure((size_t)R.ld);
    c.lsr_part.ensure((size_t)(m + 1) * (size_t)R.G);
    c.lsr_c.ensure((size_t)m + 2);
    c.lsr_ctrl.ensure(LSR_CTRL_DOUBLES);
    c.lsr_L.ensure((size_t)6 * nbr);
    c.lsr_diag.ensure((size_t)2 * nbr);
    c.n_linsys_reports++;

    const BsrPart& d = c.part[1];
    hipLaunchKernelGGL(k_lsr_chol, dim3(grid_for(nbr)), dim3(BLOCK), 0, c.stream, (const float*)c.part[0].vals.p, (const int32_t*)c.diag_slot[0].p,
                       d.nnzb ? (const float*)d.vals.p : (const float*)nullptr, (const int32_t*)c.diag_slot[1].p, caller_rows(c), nbr, c.lsr_L.p, c.lsr_diag.p);
    MS_CHECK(hipGetLastError());
    std::vector<double> diag((size_t)2 * nbr), piv((size_t)nbr);
    fetch(c, diag.data(), c.lsr_diag.p, diag.size() * sizeof(double));
    for (int64_t r = 0; r < nbr; r++) piv[(size_t)r] = diag[(size_t)(2 * r + 1)];
    R.D = linsys_fold_pivots(piv.data(), nbr);
    if (op == LINSYS_JACOBI && R.D.not_pd > 0.0) {  // nothing is iterated: a finding in itself
        R.flags = LINSYS_FLAG_DIAG_NOT_PD;
        return R;
    }

    double* V = c.lsr_V.p;
    double* w = c.lsr_w.p;
    h2d_staged(c, c.lsr_t.p, v0.data(), (size_t)n * sizeof(double));
    if (c.perm_active) rows_to_solver(c, c.lsr_t.p, V);
    else copy_async(c.stream, V, c.lsr_t.p, (size_t)n * sizeof(double));
    fill_async(c.stream, c.lsr_ctrl.p, 0, LSR_CTRL_DOUBLES * sizeof(double));
    const LsrCtrl* ctrl = ctrl_of(c);
    const dim3 grid((unsigned)R.G), block(BLOCK);
    for (int j = 0; j < kmax; j++) {
        const double* vj = V + (size_t)j * (size_t)R.ld;
        apply_operator(c, op, vj, w, ctrl);
        hipLaunchKernelGGL(k_lsr_multidot, grid, block, 0, c.stream, (const double*)V, R.ld, j, 1, (const double*)w, n, c.lsr_part.p, ctrl);
        hipLaunchKernelGGL(k_lsr_fold, dim3(1), block, 0, c.stream, (const double*)c.lsr_part.p, R.G, 1, (int)LSR_FOLD_ALPHA, j, c.lsr_c.p, ctrl_mut(c));
        hipLaunchKernelGGL(k_lsr_update, grid, block, 0, c.stream, (const double*)V, R.ld, j > 0 ? j - 1 : 0, j > 0 ? 2 : 1, (const double*)c.lsr_c.p, w, n, ctrl);
        for (int pass = 0; pass < 2; pass++) {
            hipLaunchKernelGGL(k_lsr_multidot, grid, block, 0, c.stream, (const double*)V, R.ld, 0, j + 1, (const double*)w, n, c.lsr_part.p, ctrl);
            hipLaunchKernelGGL(k_lsr_fold, dim3((unsigned)((j + 4) / 4)), block, 0, c.stream, (const double*)c.lsr_part.p, R.G, j + 1, (int)LSR_FOLD_COEF, j, c.lsr_c.p, ctrl_mut(c));
            hipLaunchKernelGGL(k_lsr_update, grid, block, 0, c.stream, (const double*)V, R.ld, 0, j + 1, (const double*)c.lsr_c.p, w, n, ctrl);
        }
        hipLaunchKernelGGL(k_lsr_multidot, grid, block, 0, c.stream, (const double*)w, R.ld, 0, 1, (const double*)w, n, c.lsr_part.p, ctrl);
        hipLaunchKernelGGL(k_lsr_fold, dim3(1), block, 0, c.stream, (const double*)c.lsr_part.p, R.G, 1, (int)LSR_FOLD_BETA, j, c.lsr_c.p, ctrl_mut(c));
        if (j + 1 < kmax) hipLaunchKernelGGL(k_lsr_normalise, grid, block, 0, c.stream, (const double*)w, V + (size_t)(j + 1) * (size_t)R.ld, n, j, ctrl);
        // every LSR_STOP_CHECK steps the host looks at the stop flag, so that an exhausted Krylov space (a star stops after 7 steps) does not cost the
        // remaining SpMV launches; what is computed does not depend on it
        if ((j + 1) % LSR_STOP_CHECK == 0 && j + 1 < kmax) {
            int stop = 0;
            fetch(c, &stop, c.lsr_ctrl.p, sizeof(int));
            if (stop) break;
        }
    }
    MS_CHECK(hipGetLastError());
    std::vector<double> raw(LSR_CTRL_DOUBLES);
    fetch(c, raw.data(), c.lsr_ctrl.p, raw.size() * sizeof(double));
    LsrCtrl h;
    std::memcpy(&h, raw.data(), sizeof(LsrCtrl));
    R.k = h.k;
    R.flags = h.flags;
    R.t_norm = h.t_norm;
    R.alpha.assign(h.alpha, h.alpha + R.k);
    R.beta.assign(h.beta, h.beta + R.k);
    return R;
}

// the record, the Ritz list and (S non-null) the eigenvectors of T
void records(const Run& R, double* out, double* ritz, std::vector<double>* S)
{
    const int k = std::max(R.k, 1);
    std::vector<double> work((size_t)3 * k), rz((size_t)2 * R.m);
    if (S) S->assign((size_t)k * k, 0.0);
    double rec[LINSYS_REC];
    linsys_build_record(R.k, R.m, R.alpha.data(), R.beta.data(), R.t_norm, R.flags, R.n, R.D, rec, rz.data(), S && R.k > 0 ? S->data() : nullptr, work.data());
    if (out) std::copy(rec, rec + LINSYS_REC, out);
    if (ritz) std::copy(rz.begin(), rz.end(), ritz);
}

struct Mode
{
    int index = 0;
    double theta = 0.0, rho = 0.0, resid = 0.0;
};
// u = V s_i into lsr_w, x = L^-T u (op 1) or u (op 0) into lsr_t, both by solver row; the residual |B u - theta u| from one more operator application
Mode ritz_vector(Context& c, const Run& R, const std::vector<double>& S, const std::vector<double>& ritz, int which, const char* who)
{
    const int k = R.k;
    if (R.flags & (LINSYS_FLAG_DIAG_NOT_PD | LINSYS_FLAG_NONFINITE) || k < 1)
        throw Error(std::string(who) + ": no Ritz pairs (the run was refused or met a non-finite value; see mistark_linsys_report)");
    const int idx = which >= 0 ? which : k + which;
    if (idx < 0 || idx >= k) throw Error(std::string(who) + ": bad which " + std::to_string(which) + " (" + std::to_string(k) + " Ritz values)");
    Mode M;
    M.index = idx;
    M.theta = ritz[(size_t)2 * idx];
    M.rho = ritz[(size_t)2 * idx + 1];
    std::vector<double> coef((size_t)k);
    for (int i = 0; i < k; i++) coef[(size_t)i] = -S[(size_t)idx * k + i];
    const int64_t n = R.n;
    h2d_small(c, c.lsr_c.p, coef.data(), coef.size() * sizeof(double));
    fill_async(c.stream, c.lsr_w.p, 0, (size_t)R.ld * sizeof(double));
    hipLaunchKernelGGL(k_lsr_update, dim3((unsigned)R.G), dim3(BLOCK), 0, c.stream, (const double*)c.lsr_V.p, R.ld, 0, k, (const double*)c.lsr_c.p, c.lsr_w.p, n, (const LsrCtrl*)nullptr);
    // B u into row k of the basis buffer (rows beyond the k basis vectors are free: k <= m)
    double* Bu = c.lsr_V.p + (size_t)k * (size_t)R.ld;
    apply_operator(c, R.op, c.lsr_w.p, Bu, nullptr);  // (op 1 leaves x = L^-T u in lsr_t)
    if (R.op == LINSYS_A) copy_async(c.stream, c.lsr_t.p, c.lsr_w.p, (size_t)n * sizeof(double));
    MS_CHECK(hipGetLastError());
    std::vector<double> u((size_t)n), bu((size_t)n);
    MS_CHECK(hipMemcpyAsync(u.data(), c.lsr_w.p, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, c.stream));
    MS_CHECK(hipMemcpyAsync(bu.data(), Bu, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, c.stream));
    MS_CHECK(hipStreamSynchronize(c.stream));
    double r2 = 0.0;
    for (int64_t i = 0; i < n; i++) {
        const double r = bu[(size_t)i] - M.theta * u[(size_t)i];
        r2 += r * r;
    }
    M.resid = std::sqrt(r2);
    return M;
}
// x of the last ritz_vector() in DoF order into lsr_y
void x_to_caller(Context& c, const Run& R)
{
    if (c.perm_active) rows_from_solver(c, c.lsr_t.p, c.lsr_y.p);
    else copy_async(c.stream, c.lsr_y.p, c.lsr_t.p, (size_t)R.n * sizeof(double));
}
}  // namespace

void linsys_report_host(Context& c, int op, int m, const double* start_host, double* out, double* ritz, double* tri, int32_t* k_out)
{
    const char* who = "mistark_linsys_report";
    refuse(c, op, m, who);
    if (!out && !ritz && !tri && !k_out) return;  // nothing is launched
    const Run R = lanczos(c, op, m, start_host, who);
    records(R, out, ritz, nullptr);
    if (tri) {
        std::fill(tri, tri + 2 * (size_t)m, 0.0);
        for (int j = 0; j < R.k; j++) {
            tri[2 * j] = R.alpha[(size_t)j];
            tri[2 * j + 1] = R.beta[(size_t)j];
        }
    }
    if (k_out) *k_out = R.k;
}

void linsys_modes_host(Context& c, int op, int m, const double* start_host, const int32_t* which, int32_t n_which, double* x_host, double* nodal, double* mode)
{
    const char* who = "mistark_linsys_modes";
    refuse(c, op, m, who);
    if (n_which < 0 || (n_which > 0 && !which)) throw Error(std::string(who) + ": bad which list");
    for (int32_t w = 0; w < n_which; w++)
        if (which[w] >= m || which[w] < -m) throw Error(std::string(who) + ": bad which " + std::to_string(which[w]) + " (at most " + std::to_string(m) + " Ritz values)");
    if ((!x_host && !nodal && !mode) || n_which == 0) return;  // nothing is launched
    const Run R = lanczos(c, op, m, start_host, who);
    std::vector<double> S, ritz((size_t)2 * m);
    records(R, nullptr, ritz.data(), &S);
    c.lsr_nodal.ensure((size_t)LINSYS_NODAL * c.nbr);
    for (int32_t w = 0; w < n_which; w++) {
        const Mode M = ritz_vector(c, R, S, ritz, which[w], who);
        if (mode) {
            double* o = mode + (size_t)LINSYS_MODE * w;
            o[0] = M.theta;
            o[1] = M.rho;
            o[2] = M.resid;
            o[3] = (double)M.index;
        }
        if (nodal) {
            hipLaunchKernelGGL(k_lsr_nodal, dim3(grid_for(c.nbr)), dim3(BLOCK), 0, c.stream, (const double*)c.lsr_w.p, (const double*)c.lsr_t.p, (const double*)c.lsr_diag.p,
                               caller_rows(c), c.nbr, c.lsr_nodal.p);
            MS_CHECK(hipGetLastError());
            MS_CHECK(hipMemcpyAsync(nodal + (size_t)LINSYS_NODAL * c.nbr * w, c.lsr_nodal.p, (size_t)LINSYS_NODAL * c.nbr * sizeof(double), hipMemcpyDeviceToHost, c.stream));
        }
        if (x_host) {
            x_to_caller(c, R);
            MS_CHECK(hipMemcpyAsync(x_host + (size_t)R.n * w, c.lsr_y.p, (size_t)R.n * sizeof(double), hipMemcpyDeviceToHost, c.stream));
        }
        MS_CHECK(hipStreamSynchronize(c.stream));
    }
}

void linsys_potential_shares_host(Context& c, int op, int m, const double* start_host, int32_t which, const int32_t* pots, int32_t n, double* out)
{
    const char* who = "mistark_linsys_potential_shares";
    refuse(c, op, m, who);
    if (n < 0 || (n > 0 && !pots)) throw Error(std::string(who) + ": bad potential list");
    std::vector<char> seen(c.pots.size(), 0);
    for (int32_t k = 0; k < n; k++) {
        const int p = pots[k];
        if (p < 0 || p >= (int)c.pots.size()) throw Error(std::string(who) + ": bad potential id " + std::to_string(p));
        if (seen[(size_t)p]) throw Error(std::string(who) + ": potential '" + c.pots[(size_t)p].name + "' is listed twice");
        seen[(size_t)p] = 1;
    }
    if (which >= m || which < -m) throw Error(std::string(who) + ": bad which " + std::to_string(which) + " (at most " + std::to_string(m) + " Ritz values)");
    // (reached only with a stale matrix: a registration after mistark_assemble makes the next prepare() drop the Hessians and keeps the matrix)
    if (!c.have_hessians) throw Error(std::string(who) + ": no element Hessians (call eval with MISTARK_EVAL_P_G_H first)");
    for (int32_t k = 0; k < n; k++) {
        const Potential& P = c.pots[(size_t)pots[k]];
        if (c.lazy_active && P.lazy_capable)
            throw Error(std::string(who) + ": element Hessians of '" + P.name + "' were evaluated on the lazy path (float blocks only); evaluate without lazy_eval");
        if (P.NB < 1 || P.NB > MAX_NB) throw Error(std::string(who) + ": unsupported block count");
        if (P.n_elem > 0 && (P.args.elem_list || P.args.e_count != P.n_elem)) throw Error(std::string(who) + ": single-rank accessor");
    }
    if (!out || n == 0) return;  // nothing is launched
    const Run R = lanczos(c, op, m, start_host, who);
    std::vector<double> S, ritz((size_t)2 * m);
    records(R, nullptr, ritz.data(), &S);
    ritz_vector(c, R, S, ritz, which, who);
    x_to_caller(c, R);
    int64_t ne_max = 0;
    for (int32_t k = 0; k < n; k++) ne_max = std::max<int64_t>(ne_max, c.pots[(size_t)pots[k]].n_elem);
    c.lsr_q.ensure((size_t)ne_max);
    c.lsr_nz.ensure((size_t)ne_max);
    c.lsr_cols.ensure(2 * MAX_NB);
    std::vector<double> q;
    std::vector<uint8_t> nz;
    for (int32_t k = 0; k < n; k++) {
        const Potential& P = c.pots[(size_t)pots[k]];
        double* o = out + (size_t)LINSYS_POT * k;
        o[0] = o[1] = o[2] = 0.0;
        o[3] = -1.0;
        if (P.n_elem <= 0) continue;
        int cols[2 * MAX_NB];
        for (int b = 0; b < MAX_NB; b++) {
            cols[b] = P.args.dof_col[b];
            cols[MAX_NB + b] = P.args.dof_row_off[b];
        }
        h2d_small(c, c.lsr_cols.p, cols, sizeof(cols));
        hipLaunchKernelGGL(k_lsr_quad, dim3(grid_for(P.n_elem)), dim3(BLOCK), 0, c.stream, (const double*)(c.elemH.p + P.h_off), P.n_elem, P.n_key, P.NB, P.args.conn, P.conn_stride,
                           (const int*)c.lsr_cols.p, (const int*)c.lsr_cols.p + MAX_NB, (const double*)c.lsr_y.p, c.lsr_q.p, c.lsr_nz.p);
        MS_CHECK(hipGetLastError());
        q.resize((size_t)P.n_elem);
        nz.resize((size_t)P.n_elem);
        MS_CHECK(hipMemcpyAsync(q.data(), c.lsr_q.p, q.size() * sizeof(double), hipMemcpyDeviceToHost, c.stream));
        MS_CHECK(hipMemcpyAsync(nz.data(), c.lsr_nz.p, nz.size(), hipMemcpyDeviceToHost, c.stream));
        MS_CHECK(hipStreamSynchronize(c.stream));
        double big = -1.0, c0 = 0.0, c1 = 0.0;
        auto add = [](double& sum, double& comp, double v) {  // compensated (Neumaier), in element order: the sum is good to an ulp of sum |q_e| whatever the count
            const volatile double t = sum + v;
            comp += std::fabs(sum) >= std::fabs(v) ? (sum - t) + v : (v - t) + sum;
            sum = t;
        };
        for (int e = 0; e < P.n_elem; e++) {  // fixed order: the element's
            add(o[0], c0, q[(size_t)e]);
            add(o[1], c1, std::fabs(q[(size_t)e]));
            o[2] += nz[(size_t)e] ? 1.0 : 0.0;
            if (std::fabs(q[(size_t)e]) > big) {
                big = std::fabs(q[(size_t)e]);
                o[3] = (double)e;
            }
        }
        o[0] += c0;
        o[1] += c1;
    }
}

// the host mirror's recording: one run from the built-in start vector; the summary record and, from the nodal records of the lowest and the highest
// Ritz vector, the first block row attaining the largest share of each
void linsys_record_step(Context& c, int op, int m)
{
    const char* who = "linear-system report";
    Context::LinsysSlot& s = c.lsr_slot;
    s = Context::LinsysSlot{};
    refuse(c, op, m, who);
    const Run R = lanczos(c, op, m, nullptr, who);
    std::vector<double> S, ritz((size_t)2 * m);
    records(R, s.rec, ritz.data(), &S);
    if (!(R.flags & (LINSYS_FLAG_DIAG_NOT_PD | LINSYS_FLAG_NONFINITE)) && R.k >= 1) {
        c.lsr_nodal.ensure((size_t)LINSYS_NODAL * c.nbr);
        std::vector<double> nodal((size_t)LINSYS_NODAL * c.nbr);
        for (int end = 0; end < 2; end++) {
            ritz_vector(c, R, S, ritz, end == 0 ? 0 : -1, who);
            hipLaunchKernelGGL(k_lsr_nodal, dim3(grid_for(c.nbr)), dim3(BLOCK), 0, c.stream, (const double*)c.lsr_w.p, (const double*)c.lsr_t.p, (const double*)c.lsr_diag.p,
                               caller_rows(c), c.nbr, c.lsr_nodal.p);
            MS_CHECK(hipGetLastError());
            fetch(c, nodal.data(), c.lsr_nodal.p, nodal.size() * sizeof(double));
            double best = -1.0, row = -1.0;
            for (int64_t r = 0; r < c.nbr; r++)
                if (nodal[(size_t)(LINSYS_NODAL * r)] > best) {
                    best = nodal[(size_t)(LINSYS_NODAL * r)];
                    row = (double)r;
                }
            (end == 0 ? s.low_row : s.high_row) = row;
            (end == 0 ? s.low_share : s.high_share) = best;
        }
    }
    s.valid = true;
}
void linsys_fetch(Context& c, double* rec16, double* rows4)
{
    const Context::LinsysSlot& s = c.lsr_slot;
    if (!s.valid) throw Error("linear-system report: nothing recorded");
    if (rec16) std::copy(s.rec, s.rec + LINSYS_REC, rec16);
    if (rows4) {
        rows4[0] = s.low_row;
        rows4[1] = s.low_share;
        rows4[2] = s.high_row;
        rows4[3] = s.high_share;
    }
}

}  // namespace mistark
