// force_stage.hpp — the two stages of the force readout (forces.hip) for the pipelines that reuse them on buffers of their own (wrench.hip): the generic
// hyper-dual gradient of every selected element into a pool, then the key sort and k_force_segsum into a nodal vector.
#pragma once
#include "force_keys.hpp"

namespace mistark {

struct ForceSelection
{
    std::vector<int> pots;           // selected potentials with elements, in the caller's order
    std::vector<ForceDesc> descs;
    std::vector<int64_t> g_off;
    int64_t total = 0;               // contributions (element, block)
};
struct ForceWork                     // the buffers a readout works in
{
    DevBuf<double>&pool, &elemE;
    DevBuf<uint32_t>&key, &key_alt, &val, &val_alt;
    DevBuf<unsigned char>& desc;
    DevBuf<uint8_t>& cub_tmp;
};
// refusals (select_potentials), prepare(), and the layout of the selection in a pool: contribution g = g_off + block * n_elem + element
ForceSelection force_select(Context& c, const int32_t* pots, int32_t n, bool all, const char* who);
void force_element_stage(Context& c, const ForceSelection& S, const ForceWork& W);
// f_dev[ndofs] = -scale * row sums of W.pool, one lane per row, a run of more than 256 contributions by the wavefront that holds its head; stat[0..1] is
// zeroed and stat[0] counts those runs. Returns the sorted keys (total of them, in W.key or W.key_alt).
const uint32_t* force_nodal_stage(Context& c, const ForceSelection& S, const ForceWork& W, double scale, double* f_dev, uint32_t* stat);

}  // namespace mistark
