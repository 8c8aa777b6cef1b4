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
// budget readout (budget.hip) into device slot `slot`: the energies of the listed potentials (one double each), the 13-double records of an
// EnergyLumpedInertia potential's groups, of the rigid bodies (array ids as mistark_rigid_budget takes them)
int budget_record_energies(mistark_ctx* ctx, int slot, const std::vector<int32_t>& pots);
int budget_record_inertia(mistark_ctx* ctx, int slot, int potential, const double about[3], int32_t n_groups);
int budget_record_rigid(mistark_ctx* ctx, int slot, int t0, int q0, int v1, int w1, int mass, int J_loc, int32_t n_bodies, const double about[3]);
// out[n] of slot `slot`
int budget_fetch(mistark_ctx* ctx, int slot, double* out, int64_t n);
// constraint report (constraint_report.hip): rows and groups of one potential into the set of its kind (0..16), kept on the device until fetched
int constraint_record(mistark_ctx* ctx, int potential, const double* tolerance, int32_t n_groups, const double about[3], int32_t* kind);
int constraint_fetch(mistark_ctx* ctx, int kind, double* out, double* aux, int32_t* ids, double* groups, int64_t* n_rows, int32_t* n_groups);
// bending report (bending_report.hip): rows, nodal records and groups of the registered bending potentials (-1: not registered) into the device set of the
// host mirror; kind 0 complete, 1 flat; nodal out[n_rows][6], n_rows = block rows of the DoF vector
int bending_record(mistark_ctx* ctx, int pot_complete, int pot_flat, const double* threshold, int32_t n_groups);
int bending_fetch(mistark_ctx* ctx, int kind, double* rows, double* groups, int64_t* n_rows, int32_t* n_groups);
int bending_fetch_nodal(mistark_ctx* ctx, double* out, int64_t n_rows);
// Hessian spectrum report (spectrum_report.hip), source 1 over the listed potentials: element, nodal and potential records into the device set of the host
// mirror. Fetch: pots_out [n][10] for the n listed potentials, nodal_out [n_rows][5], n_rows = block rows of the DoF vector (both nullable); rows
// [n_rows][10] of the index-th listed potential (rows nullable: the count alone)
int spectrum_record(mistark_ctx* ctx, const std::vector<int32_t>& pots, double eps);
int spectrum_fetch(mistark_ctx* ctx, int32_t n, double* pots_out, double* nodal_out, int64_t n_rows);
int spectrum_fetch_rows(mistark_ctx* ctx, int32_t index, double* rows, int64_t* n_rows);
// linear-system report (linsys_report.hip) of the matrix as the step's last assembly left it: the summary record and the block rows with the largest share
// of the lowest and of the highest mode, kept in the context until fetched. rec16 [16]; rows4: low row, its share, high row, its share
int linsys_record(mistark_ctx* ctx, int op, int m);
int linsys_fetch(mistark_ctx* ctx, double* rec16, double* rows4);
// rigid-body wrench report (wrench.hip): the body report of the given families of potentials (an empty list: the zero wrench, unless all[f]: every
// potential) kept on the device; out [n_families][n_bodies][16], count [n_families][n_bodies]
int wrench_record(mistark_ctx* ctx, const std::vector<std::vector<int32_t>>& families, const std::vector<char>& all, int v1, int w1, int t0, int q0, int32_t n_bodies,
                  const double about[3]);
int wrench_fetch(mistark_ctx* ctx, int32_t n_families, int32_t n_bodies, double* out, int32_t* count);
// contact report (contact_report.hip) of the current state into the device set of the host mirror; its three parts (null outputs are skipped, the counts
// always come back)
int contact_report_record(mistark_ctx* ctx);
int contact_report_fetch(mistark_ctx* ctx, int32_t* rows_i, double* rows_d, int64_t* n_rows, double* vert, int32_t* group, int32_t* source_index, int64_t* n_vertices, double* pairs,
                         int32_t* n_groups);
// friction report (friction_report.hip), likewise
int friction_report_record(mistark_ctx* ctx);
int friction_report_fetch(mistark_ctx* ctx, int32_t* rows_i, double* rows_d, int64_t* n_rows, double* vert, int32_t* group, int32_t* source_index, int64_t* n_vertices, double* pairs,
                          int32_t* n_groups);
// registry name of every potential in id order, and whether it is user-defined
int potential_names(mistark_ctx* ctx, std::vector<std::string>& names, std::vector<char>& custom);

}  // namespace mistark
