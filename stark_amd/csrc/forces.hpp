// forces.hpp — what the host mirror (host/sim.cpp) uses of the force readout beyond the C ABI of include/mistark.h: nodal vectors recorded inside a
// time step stay on the device until somebody asks for them. Status returns as in the C ABI (0 = ok, otherwise mistark_last_error()).
#pragma once
#include <string>
#include <vector>

#include "../../include/mistark.h"

namespace mistark {

// ids of the potentials whose registry name starts with `prefix` (an empty prefix: every potential), in registration order
int force_potentials_by_prefix(mistark_ctx* ctx, const std::string& prefix, std::vector<int32_t>& out);
// readout of the listed potentials into device slot `slot` (an empty list: the zero vector, no launch)
int force_record(mistark_ctx* ctx, int slot, const std::vector<int32_t>& pots, double scale);
// f_host[ndofs] of slot `slot`
int force_fetch(mistark_ctx* ctx, int slot, double* f_host, int64_t ndofs);

}  // namespace mistark
