// force_keys.hpp — the sort keys of the readouts that sum element contributions per block row without atomics (forces.hip, stress.hip): one key per
// (element, local DoF block) = its block row; a stable radix sort by it keeps equal rows in contribution order.
#pragma once
#include "kernels_common.hpp"

namespace mistark {

struct ForceDesc
{
    const int32_t* conn;
    int stride, n_elem, NB;
    uint32_t g_off;  // first contribution of the potential: g = g_off + block * n_elem + element, the pool holds 3 doubles per contribution
    int dof_col[MAX_NB], dof_row_off[MAX_NB];
};
// contribution g -> (block row, g)
static __global__ __launch_bounds__(BLOCK) void k_force_keys(const ForceDesc* __restrict__ D, int n_desc, int64_t total, uint32_t* __restrict__ key, uint32_t* __restrict__ val)
{
    const int64_t g = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (g >= total) return;
    int k = 0;
    while (k + 1 < n_desc && g >= (int64_t)D[k + 1].g_off) k++;
    const ForceDesc& d = D[k];
    const uint32_t l = (uint32_t)g - d.g_off;
    const int b = (int)(l / (uint32_t)d.n_elem), e = (int)(l - (uint32_t)b * (uint32_t)d.n_elem);
    key[g] = (uint32_t)(d.dof_row_off[b] + d.conn[(size_t)e * d.stride + d.dof_col[b]]);
    val[g] = (uint32_t)g;
}

}  // namespace mistark
