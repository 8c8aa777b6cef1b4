// forces.hpp — what the host mirror (host/sim.cpp) uses of the force and stress readouts beyond the C ABI of include/mistark.h: what is recorded inside a
// time step stays on the device until somebody asks for it. Status returns as in the C ABI (0 = ok, otherwise mistark_last_error()).
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
// stress readout (stress.hip) of every potential of one kind (0 tet, 1 triangle, 2 segment; potential id ascending, then element): element records
// and nodal averages into the device slot of the kind
int stress_record(mistark_ctx* ctx, int kind);
// out[n_elem][16] of the kind's slot (out nullable: the count alone)
int stress_fetch(mistark_ctx* ctx, int kind, double* out, int64_t* n_elem);
// out[n_rows][10] of the kind's slot, n_rows = block rows of the DoF vector
int stress_fetch_nodal(mistark_ctx* ctx, int kind, double* out, int64_t n_rows);

}  // namespace mistark
