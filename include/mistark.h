/* mistark.h — C ABI of libmistark.so, the MI355X-native engine behind STARK's per-Newton-step hot path.
 *
 * This is the drop-in boundary (SURVEY.md §8b "New C ABI"): plain pointers and sizes, int status returns
 * (0 = ok, otherwise mistark_last_error()), no exceptions / exit() across the boundary, one host thread per context.
 * Host buffers are caller-owned (the reference's DataMap lambdas, symx/src/compile/data_maps.h:97-105); device buffers
 * are library-owned. Each entry point cites the reference interface it replaces.
 *
 * Mapping to the reference's registration API (symx/src/solver/GlobalPotential.h:37-70):
 *   GlobalPotential::add_dof(arr, label)                 -> mistark_add_dof_set
 *   mws.make_scalar / make_vector / make_matrix(arr,..)  -> mistark_array + one mistark_binding per call, in call order
 *   GlobalPotential::add_potential(name, conn, lambda)   -> mistark_potential (name selects the hand-written kernel;
 *                                                           the symbolic lambda is not needed)
 *   GlobalPotential::get_dofs / set_dofs                 -> mistark_get_dofs / mistark_set_dofs
 *   SecondOrderCompiledGlobal::evaluate_*                -> mistark_eval
 *   NewtonsMethod::_project_and_assemble                 -> mistark_assemble / mistark_project
 *   NewtonsMethod::_solve_linear_system (bsm::solve_pcg) -> mistark_pcg
 *   NewtonsMethod::solve                                 -> mistark_newton_solve
 */
#ifndef MISTARK_H
#define MISTARK_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct mistark_ctx mistark_ctx;

/* ---- context -------------------------------------------------------------------------------------------------- */
int mistark_create(int device, mistark_ctx** out);
void mistark_destroy(mistark_ctx* ctx);
/* A registration-only context: no GPU is touched (process-wide from the first call on), DoF sets / arrays / potentials are recorded,
 * every evaluation entry point fails. For checking on a machine without a GPU what a caller registers (mistark_describe). */
int mistark_create_dry(mistark_ctx** out);
/* The registration as JSON (DoF sets; per potential: name, connectivity stride, element count, bindings as [array, stride, connectivity
 * column, items] with arrays named "dof:<label>" or "a<k>" in order of first use). Returns the length needed including the terminator;
 * writes at most cap bytes. */
int64_t mistark_describe(mistark_ctx* ctx, char* buf, int64_t cap);
const char* mistark_last_error(mistark_ctx* ctx);
/* Version / build info string (static storage). */
const char* mistark_version(void);

/* ---- DoF sets and bound arrays ---------------------------------------------------------------------------------- */
/* GlobalPotential::add_dof (GlobalPotential.h:55-61): `host` holds n_scalars doubles (3 per DoF block, AoS as
 * PointDynamics::v1, stark/src/models/deformables/PointDynamics.h:16-23). Sets are concatenated in registration order.
 * Returns the set index (>= 0) or < 0 on error. The size may be changed later with mistark_resize_dof_set. */
int mistark_add_dof_set(mistark_ctx* ctx, const char* label, double* host, int64_t n_scalars);
int mistark_resize_dof_set(mistark_ctx* ctx, int set, double* host, int64_t n_scalars);

/* A bound input array (DataMap, data_maps.h:97-121): n_items x stride doubles, row-major, caller-owned.
 * Arrays are identified by (host pointer, stride); binding the host pointer of a DoF set yields a view of the DoF
 * vector. Returns the array id (>= 0). Re-binding an existing (pointer, stride) updates n_items. */
int mistark_array(mistark_ctx* ctx, const double* host, int64_t n_items, int stride);
/* The view of DoF set `set` as an array of the given stride, by set index instead of by host address (an EMPTY set has no address to be
 * recognised by: SymX identifies DoF maps by container identity, DataMap::id, data_maps.h:97-105). Returns the array id. */
int mistark_dof_array(mistark_ctx* ctx, int set, int stride);
/* Re-point an array id at a (possibly reallocated / resized) host buffer. */
int mistark_array_rebind(mistark_ctx* ctx, int array, const double* host, int64_t n_items);
/* host -> device / device -> host copies of one array (all arrays if array < 0). */
int mistark_upload(mistark_ctx* ctx, int array);
int mistark_download(mistark_ctx* ctx, int array);
/* Device-side vector helpers used by the state containers (PointDynamics.cpp:58-78): dst = a*x + b*y (x,y,dst array
 * ids of equal size; y may be -1), fill. */
int mistark_array_axpby(mistark_ctx* ctx, int dst, double a, int x, double b, int y);
int mistark_array_fill(mistark_ctx* ctx, int dst, double value);

/* ---- potentials ----------------------------------------------------------------------------------------------------- */
typedef struct mistark_binding
{
    int32_t array;     /* id from mistark_array */
    int32_t stride;    /* doubles per item (must match the kernel's expectation) */
    int32_t conn_col;  /* connectivity column that indexes the array, -1 = global value (item 0) */
} mistark_binding;

/* GlobalPotential::add_potential(name, LabelledConnectivity<N>&, ...) (GlobalPotential.h:37-52). `name` is the
 * reference's registry key (e.g. "EnergyTetStrain"); bindings are given in the order of the reference's mws.make_*
 * calls for that potential. conn: n_elem x conn_stride int32, row-major, copied at call time.
 * Returns the potential id (>= 0). Calling again with an existing name replaces connectivity and bindings. */
int mistark_potential(mistark_ctx* ctx, const char* name, const int32_t* conn, int32_t n_elem, int32_t conn_stride,
                      const mistark_binding* bindings, int32_t n_bindings);

/* A potential WITHOUT a hand-written kernel (user-defined energies, README.md:109-126 of the reference): the energy is handed over as
 * SymX's own straight-line op sequence and interpreted on the device (slow path; see csrc/custom.hip). The reference-side shim builds
 * it with `symx::Sequence seq({potential.get_expression()})` (symx/src/compile/Sequence.h:24-41) and copies `seq.ops`:
 *   ops       n_ops rows {type, dst, a, b, cond} with symx::ExprType codes (symx/src/symbol/Expr.h:12-43) and the value numbering of
 *             symx/src/compile/Compilation.cpp:381-469: values < n_inputs are the gathered inputs (the bindings flattened in order),
 *             a Symbol op binds output 0 (the energy), Branch ops are the if (value > 0) / else / endif markers
 *   constants one double per op (used by ConstantFloat ops)
 *   cond_*    optional second sequence: the element is active iff its value is > 0 (Potential::get_condition, conditional potentials)
 * Bindings on DoF arrays define the local DoF blocks exactly as for mistark_potential. Limits: 96 inputs, 256 live temporaries, Branch
 * markers nested at most 32 deep. The markers of either sequence must nest (no else / endif without an open if, one else per if, none left
 * open): anything else is refused here with the potential's name and the op index. */
int mistark_potential_custom(mistark_ctx* ctx, const char* name, const int32_t* conn, int32_t n_elem, int32_t conn_stride, const mistark_binding* bindings, int32_t n_bindings,
                             const int32_t* ops, const double* constants, int32_t n_ops, int32_t n_inputs, const int32_t* cond_ops, const double* cond_constants,
                             int32_t n_cond_ops);
/* A custom potential does not stay interpreted: at its first evaluation the op sequence is EMITTED as HIP source (one statement per op, the
 * temporaries local variables, Branch markers real branches, the gather unrolled — the mirror of the reference's scalar emitter,
 * symx/src/compile/Compilation.cpp:381-469), compiled for gfx950 by hipRTC and cached on disk by a hash of the source (MISTARK_RTC_CACHE,
 * default /tmp/mistark_rtc_cache_<uid>). The interpreter remains the fallback (no libhiprtc, a failed build, sequences of more than
 * MISTARK_RTC_MAX_OPS = 3000 ops, option "custom_rtc" = 0). mistark_custom_emit returns what the emitter writes for a sequence — the source
 * in `out` (truncated to cap) and its length — and, with compile != 0, runs hipRTC on it and returns the size of the code object; < 0 with the
 * message in `out` on failure. in_dof[k]: the local DoF component (3 * block + c) input k seeds, -1 for inputs that are not DoFs. Needs no
 * context and no GPU. */
int64_t mistark_custom_emit(const char* name, const int32_t* strides, int32_t n_bindings, const int32_t* in_dof, const int32_t* ops, const double* constants, int32_t n_ops,
                            int32_t n_inputs, const int32_t* cond_ops, const double* cond_constants, int32_t n_cond_ops, int32_t n_blocks, int32_t compile, char* out, int64_t cap);
/* Summation loop of a custom potential (MappedWorkspace::add_for_each, symx/src/compile/MappedWorkspace.h:123-130; used by SymX's fem
 * integrators for quadrature rules): inputs [first_input, first_input + stride) — covered by a binding like any other input — take the
 * n_iterations rows of `data` (copied) one after the other, and the element's energy, gradient and Hessian are the sums over the rows in
 * that order (CompiledInLoop_run.h:375-400). One summation per potential, as in the reference (MappedWorkspace.h:525-530). */
int mistark_potential_custom_set_summation(mistark_ctx* ctx, int potential, int32_t first_input, int32_t stride, int32_t n_iterations, const double* data);
/* Marks a potential whose connectivity changes inside the Newton loop (the reference's contact tables are refilled in
 * before_energy_evaluation, EnergyFrictionalContact.cpp:117-119). Its Hessian blocks go to a second, small block-CSR part
 * (A = A_static + A_dynamic) so that a connectivity update only re-patterns that part, not the whole matrix. */
/* Introspection of a registration (what MappedWorkspace holds for a potential, MappedWorkspace.h:329-333): the connectivity table as
 * registered (conn may be NULL to query the sizes; device-side contact tables: mistark_contact_get_table), and the caller's array behind
 * binding `binding` (pointer, items, stride). */
int mistark_potential_table(mistark_ctx* ctx, int potential, int32_t* conn, int64_t* n_elem, int32_t* conn_stride);
int mistark_potential_binding_data(mistark_ctx* ctx, int potential, int binding, const double** host, int64_t* n_items, int32_t* stride);
int mistark_potential_set_dynamic(mistark_ctx* ctx, int potential, int dynamic);
/* Id of the first potential registered under `name` (the ids mistark_potential returned, in registration order), -1 if there is none. */
int mistark_find_potential(mistark_ctx* ctx, const char* name);
/* LabelledConnectivity::clear() + push_back() (symx/src/compile/LabelledConnectivity.h): replaces the rows of a potential. */
int mistark_potential_update_connectivity(mistark_ctx* ctx, int potential, const int32_t* conn, int32_t n_elem);
/* Number of potentials known to the engine and their registry names (for the shim's "unknown name" error path). */
int mistark_n_supported_potentials(void);
const char* mistark_supported_potential(int i);

/* ---- DoF vector --------------------------------------------------------------------------------------------------- */
int64_t mistark_ndofs(mistark_ctx* ctx);
int mistark_get_dofs(mistark_ctx* ctx, double* u_host);        /* GlobalPotential::get_dofs (GlobalPotential.cpp:111-121) */
int mistark_set_dofs(mistark_ctx* ctx, const double* u_host);  /* GlobalPotential::set_dofs (GlobalPotential.cpp:134-144) */
/* device DoFs -> the host arrays registered with mistark_add_dof_set, and back */
int mistark_dofs_to_host_arrays(mistark_ctx* ctx);
/* The same, skipped when the DoF vector on the device has not changed since the last transfer to the caller's arrays (a drop-in's Newton
 * callbacks all read the DoFs from the caller's arrays; several of them run at the same iterate: intersection check, contact update,
 * convergence test). The caller must not have written its DoF arrays in between (mistark_dofs_from_host_arrays / mistark_set_dofs say so). */
int mistark_dofs_to_host_arrays_if_changed(mistark_ctx* ctx);
int mistark_dofs_from_host_arrays(mistark_ctx* ctx);

/* ---- evaluation ----------------------------------------------------------------------------------------------------- */
enum { MISTARK_EVAL_P = 0, MISTARK_EVAL_P_G = 1, MISTARK_EVAL_P_G_H = 2 };
/* SecondOrderCompiledGlobal::evaluate_P / _P__dP_du / _P__dP_du__local_d2P_du2 (SecondOrderCompiledGlobal.cpp:72-142).
 * E: total energy; grad_host (may be NULL): ndofs doubles. Element Hessians stay on the device. */
int mistark_eval(mistark_ctx* ctx, int mode, double* E, double* grad_host);
/* Parity access: element Hessians of one potential, n_elem x (3 NB) x (3 NB) row-major doubles, and the global block
 * rows n_elem x NB (ElementHessians::HessianView, ElementHessians.h:33-39). Either pointer may be NULL. */
int mistark_get_element_hessians(mistark_ctx* ctx, int potential, double* values, int32_t* block_rows, int32_t* nb_out);
int mistark_get_element_energies(mistark_ctx* ctx, int potential, double* values);

/* ---- force readout --------------------------------------------------------------------------------------------------------
 * The generalised force of a set S of potentials at the current DoFs u: f = -scale * sum over S of dE_P/du (with STARK's velocity DoFs,
 * x1 = x0 + dt v1, scale = 1/dt gives Newtons). A pipeline of its own beside mistark_eval: every selected potential is evaluated through its generic
 * hyper-dual expression, node gradients go to a pool of the readout's own, are sorted by block row (stable) and summed row by row in that order.
 * No floating-point atomics: two readouts of one state give the same bits. Nothing mistark_eval, the matrix or the contact detector own is written;
 * contact and friction tables are read as installed (no search runs). May be called between solves and from any Newton callback. Refused: sharded
 * contexts (single-rank accessor), user-defined potentials (mistark_potential_custom) in the set, registration-only contexts. */
/* Node forces of every element of one potential at the current DoFs: out[e][k][3] = -scale * dE_e/du_(block k), e < n_elem, k < NB
 * (zeros for elements whose condition is off); block_rows[e][k] as mistark_get_element_hessians reports them. Pointers nullable
 * (query sizes with both NULL). */
int mistark_potential_element_forces(mistark_ctx* ctx, int potential, double scale, double* out, int32_t* block_rows, int64_t* n_elem, int32_t* nb);
/* f_host[ndofs] = -scale * sum over the listed potentials of dE/du, rows summed in a fixed order (bit-reproducible). n = 0: all potentials. */
int mistark_forces(mistark_ctx* ctx, const int32_t* potentials, int32_t n, double scale, double* f_host);
/* Resultant of the same forces over `rows` (block rows, list order): out[0..3) = sum f; out[3..6) = sum (pos_r - about) x f_r when
 * pos_host (3 doubles per listed row) is given, else 0. */
int mistark_forces_resultant(mistark_ctx* ctx, const int32_t* potentials, int32_t n, double scale, const int32_t* rows, int64_t n_rows,
                             const double* pos_host, const double about[3], double out[6]);

/* ---- stress readout -------------------------------------------------------------------------------------------------------
 * Stress and strain of the elements of the six strain potentials (EnergyTetStrain, EnergyTriangleStrain, EnergySegmentStrain and their
 * _Elasticity_Only variants) at the end-of-step state x1 = x0 + dt v1 of the current DoFs. A pipeline of its own beside mistark_eval, like the force
 * readout: it writes only buffers of its own, uses no floating-point atomics (two readouts of one state give the same bits) and costs nothing unless it
 * is called. One record is 16 doubles, the same for the three kinds:
 *   0..5 Cauchy stress in the world frame (xx yy zz xy yz zx, Pa) | 6 von Mises stress | 7 mean stress tr(sigma)/3 | 8 J (volume, area or length ratio)
 *   9..11 principal stretches, descending (a triangle has two, a segment one; the rest are 0) | 12 largest principal Green strain (stretch_max^2 - 1)/2
 *   13 energy density psi (J/m^3) as the potential evaluates it: elastic + damping + strain limiting, without the triangle's inflation term
 *   14 rest measure m, element energy = m * psi: det(DX)/6, thickness * rest area, pi r^2 l_rest | 15 flags: +1 strain limiting active, +2 degenerate
 * A triangle's stress is F S F^T / J, a symmetric world-frame tensor tangent to the deformed triangle; a segment's is (N / (pi r^2)) t t^T. Degenerate
 * elements (J <= 0, det C <= 0, zero length) set flag 2 and report zeros in 0..7 and 12. Refused, with the cause in the message: sharded contexts
 * (single-rank accessor), registration-only contexts, any other potential (by name), and a nodal list that mixes kinds. */
/* out[e][16], e < n_elem (nullable: query n_elem and kind = 0 tet, 1 triangle, 2 segment). */
int mistark_potential_element_stress(mistark_ctx* ctx, int potential, double* out, int64_t* n_elem, int32_t* kind);
/* out_host[block row][10]: the averages of fields 0..8 over the listed potentials' elements at the row, weighted with the rest measure m, then the weight
 * sum; summed in a fixed order (bit-reproducible). Entry 6 is the AVERAGE OF THE ELEMENTS' von Mises values, not the von Mises value of the averaged
 * tensor. Rows nobody touches are ten zeros. The listed potentials must be of one kind (the weights of different kinds have different units). */
int mistark_nodal_stress(mistark_ctx* ctx, const int32_t* potentials, int32_t n, double* out_host);

/* ---- budget readout -------------------------------------------------------------------------------------------------------
 * Energies per potential and the mass, momentum and energy record of every object at the current DoFs. A pipeline of its own beside mistark_eval, like
 * the force and stress readouts: it writes only buffers of its own, uses no floating-point atomics and costs nothing unless it is called. Every sum runs
 * over fixed chunks of the element list in list order and through a fixed tree: a result depends on the order of the list alone, never on a grid size,
 * the device or the run (two readouts of one state give the same bits). Contact and friction tables are read as installed (no search runs). Refused,
 * with the cause in the message: sharded contexts (single-rank accessor), registration-only contexts, user-defined potentials, bad and duplicate ids.
 * One record is 13 doubles, at the end-of-step state x = x0 + dt v1, v = v1:
 *   0 mass sum m | 1..3 first moment sum m x | 4..6 linear momentum sum m v | 7..9 angular momentum sum (x - about) x (m v) (+ J1 w1 for a rigid body)
 *   10 kinetic energy 0.5 sum m v.v (+ 0.5 w1.J1 w1) | 11 gravitational energy -sum m gravity.x | 12 item count */
/* out[k] = the energy of potential potentials[k] (n = 0: of every potential, out[number of potentials]): the sum of the element energies mistark_eval
 * would compute, elements whose condition is off counting zero, empty tables 0. */
int mistark_energies(mistark_ctx* ctx, const int32_t* potentials, int32_t n, double* out);
/* out[g][13], g < n_groups: the record of every group of an EnergyLumpedInertia potential (any other is refused by name). An element's mass is
 * lumped volume * density as the potential has them bound; its group is connectivity column 2. Group ids may come in any order; a group without elements
 * reports 13 zeros; quasistatic groups are reported like any other (the record describes the state, not the integrator). */
int mistark_inertia_budget(mistark_ctx* ctx, int potential, const double about[3], int32_t n_groups, double* out);
/* out[b][13], b < n_bodies: the record of every rigid body. Arguments: array ids of t0 [3], q0 [4], v1 [3], w1 [3], mass [1] and J_loc [9, row-major, body
 * frame] per body; the time step and gravity are those the inertia potentials have bound. t1 = t0 + dt v1, q1 = normalize(q0 + dt/2 (0, w1) q0) as in every
 * rigid-body potential, J1 = R(q1) J_loc R(q1)^T; the item count is 1. */
int mistark_rigid_budget(mistark_ctx* ctx, int t0, int q0, int v1, int w1, int mass, int J_loc, int32_t n_bodies, const double about[3], double* out);

/* ---- constraint report -----------------------------------------------------------------------------------------------------
 * What the seventeen penalty-constraint potentials (EnergyPrescribedPositions, the five EnergyAttachments_*, the eleven rb_constraint_*) hold and carry at
 * the current DoFs: per row the violation, the reaction, force and torque on side a, the two anchors, the energy and tolerance flags; per group counts, the
 * worst row, the resultant, the moment and the energy. A pipeline of its own beside mistark_eval, like the readouts above: it writes only buffers of its
 * own, uses no floating-point atomics and launches nothing unless it is called. The group sums run over fixed chunks of each group's row list in list order
 * and through a fixed tree: two reports of one state give the same bits. Refused, with the cause in the message: sharded contexts (single-rank accessor),
 * registration-only contexts, any other potential (by name), user-defined potentials, bad ids, n_groups not larger than the largest group id of the table,
 * a negative or non-finite tolerance. The group of a row is the connectivity entry it reads its stiffness with: column 2 for prescribed positions, column 0
 * for EnergyAttachments_d_d_p_p, column 1 for the other attachments, column 0 (the constraint itself) for every rigid-body kind. State: x1 = x0 + dt v1,
 * bodies at t1 = t0 + dt v1, q1 = normalize(q0 + dt/2 (0, w1) q0), velocities v1, w1.
 * Row record, 16 doubles:
 *   0 violation (m, deg, m/s or deg/s by potential; signed for distances, distance limits, the damped spring and the velocity controllers; prescribed
 *     positions and attachments: the distance |d| of the two material points) | 1 reaction (N or N m; prescribed positions and attachments: k |d|)
 *   2..4 force on side a (the first party in the potential's name; the rigid body of rb_d), -dE/dx of its anchor; zero for direction-type rows
 *   5..7 torque on side a about its centre of mass; zero when side a is deformable | 8..10 anchor (point-type) or unit direction of side a
 *   11..13 anchor or direction of side b, or the global target (velocity controllers: 8..10 the axis, 11..13 the relative velocity of b)
 *   14 energy of the row as the potential evaluates it | 15 flags: +1 active, +2 |violation| > tolerance of the row's group, +4 out of range
 *   Inactive rows (is_active off, a limit not engaged) report 0 and 8..13 and zeros elsewhere.
 * aux[row][2]: the damped spring's damper (relative velocity along the axis, -damping * that); zeros for every other kind.
 * ids[row][4]: group, kind code 0..16 (the seventeen in registry order), block row of side a's first DoF block, of side b's or -1.
 * Group record, 12 doubles: 0 rows | 1 active rows | 2 rows beyond tolerance | 3 largest |violation| | 4 position in the group's list (table order) of the
 *   first row attaining it, -1 for a group without rows | 5..7 sum of 2..4 | 8..10 moment about `about`: sum of (anchor_a - about) x f, direction-type kinds
 *   and the linear velocity controller: sum of 5..7 | 11 energy sum */
/* tolerance: [n_groups] or NULL (then n_groups may be 0 and no row is flagged beyond tolerance). All output pointers may be NULL (n_rows and kind alone: a
 * size query, nothing is launched). An empty table launches nothing and reports zero rows. */
int mistark_potential_constraint_report(mistark_ctx* ctx, int potential, const double* tolerance, int32_t n_groups, double* out, double* aux, int32_t* ids, int64_t* n_rows,
                                        int32_t* kind);
/* out[g][12], g < n_groups; a declared group without rows reports zeros with -1 in slot 4. */
int mistark_constraint_group_report(mistark_ctx* ctx, int potential, const double* tolerance, int32_t n_groups, const double about[3], double* out);

/* ---- bending report ---------------------------------------------------------------------------------------------------------
 * Where a sheet creases, how sharply it curves, what moment its hinges carry and how much energy bending holds: the two cloth bending potentials,
 * EnergyDiscreteShells (kind 0, "complete") and EnergyBendingFlat (kind 1, "flat"), at the current DoFs (x1 = x0 + dt v1). A pipeline of its own beside
 * mistark_eval, like the readouts above: it writes only buffers of its own, uses no floating-point atomics and launches nothing unless it is called; two
 * reports of one state give the same bits. Refused, with the cause in the message: sharded contexts (single-rank accessor), registration-only contexts, any
 * other potential (by name), user-defined potentials, bad or duplicate ids, n_groups not larger than the largest group id of the table, a negative or
 * non-finite threshold. The group of a row is the connectivity entry it reads its stiffness with (column 1 of the tables the host mirror registers; group 0
 * for a potential bound to one global stiffness). Local nodes 0 and 1 of a row are the hinge edge, 2 and 3 the opposite vertices.
 * Row record, 16 doubles, the same for both kinds:
 *   0 theta1: the angle as the potential's own dihedral_angle() computes it, acos((1 - 1e-12) n0.n1): in [1.41e-6, pi], blind to the fold direction
 *   1 phi1: signed fold angle atan2(e0 . (n0 x n1), n0 . n1) of the unit vectors, well conditioned near flat; its sign is the fold direction
 *   2 rest angle (complete: the bound rest angle; flat: 0) | 3 angle rate (theta1 - theta0) / dt, theta0 the same function at x0
 *   4 current hinge length | 5 rest hinge area a = (A0 + A1) / 3 from the potential's own data (complete scale^2 rest_len rest_height; flat 1 / (2 coef))
 *   6 normal curvature across the hinge kappa (complete theta1 / (3 scale rest_height); flat |s| / (3 a), s = sum K_i x1_i; both tend to 1 / R on a mesh
 *     inscribed in a cylinder of radius R) | 7 rest curvature (complete rest / (3 scale rest_height); flat 0)
 *   8 bending moment [J/rad]: complete dE/dtheta1 = ratio (2 k (theta1 - rest) + (damping / dt) (theta1 - theta0)); flat k coef |s| l1 cos(theta1 / 2),
 *     which is dE/dtheta for a fold that leaves both triangles rigid: k l sin(theta) / (2 h_e), for one stiffness a quarter of the complete model's
 *     2 k theta l / h_e at small angles
 *   9 elastic energy (complete k (theta1 - rest)^2 ratio; flat the whole element energy) | 10 damping energy (complete: the potential's damping term;
 *     flat 0); 9 + 10 is the element energy mistark_eval computes
 *   11..13 unit hinge normal (n0 + n1) / |n0 + n1| (zeros for a hinge folded onto itself) | 14 group | 15 flags: +1 degenerate, +2 |theta1 - rest| beyond
 *     the threshold of the row's group
 *   A hinge is degenerate when a triangle of its stencil has zero area at x1 or the hinge has zero length: flag 1 (never flag 2), and zeros in every field
 *   that needs a normal: 0, 1, 3, 8, 11..13, and for the complete kind 6, 9 and 10. Finite inputs give finite records.
 * Nodal record, 6 doubles per block row: only the two edge endpoints of a hinge contribute, each with weight a / 2.
 *   0 weighted mean kappa | 1 weighted mean kappa - kappa_rest | 2 energy share, sum of (9 + 10) / 2 (the nodal sum is the total) | 3 largest
 *   |theta1 - rest| | 4 hinges ending at the node | 5 weight sum. Rows no hinge ends at are six zeros.
 * Group record, 10 doubles: 0 hinges | 1 degenerate hinges | 2 hinges beyond threshold | 3 largest |theta1 - rest| | 4 position in the group's list (table
 *   order) of the first row attaining it, -1 for a group without rows | 5 sum of 9 | 6 sum of 10 | 7 sum of a | 8 sum of a (kappa - kappa_rest)^2 |
 *   9 a-weighted mean |kappa - kappa_rest| */
/* threshold: [n_groups] in rad, or NULL (then n_groups may be 0 and no row is flagged). out: [row][16] or NULL (n_rows and kind alone: a size query,
 * nothing is launched). An empty table launches nothing and reports zero rows. */
int mistark_potential_bending_report(mistark_ctx* ctx, int potential, const double* threshold, int32_t n_groups, double* out, int64_t* n_rows, int32_t* kind);
/* out_host[block row][6] over the listed potentials; both kinds may be listed together (their units agree). */
int mistark_nodal_bending(mistark_ctx* ctx, const int32_t* potentials, int32_t n, double* out_host);
/* out[g][10], g < n_groups; a declared group without rows reports zeros with -1 in slot 4. */
int mistark_bending_group_report(mistark_ctx* ctx, int potential, const double* threshold, int32_t n_groups, double* out);

/* ---- Hessian spectrum report ---------------------------------------------------------------------------------------------------
 * Where indefiniteness sits: the eigenvalues of every element Hessian of a potential and what mistark_project would make of them, per element, per block
 * row and per potential, without eigenvectors and without changing a bit of the Hessians, the gradient, the matrix or anything a solver owns. A pipeline
 * of its own beside mistark_eval, like the readouts above: it writes only buffers of its own, uses no floating-point atomics and launches nothing unless
 * it is called; two reports of one state give the same bits.
 * source 0: the element-Hessian pool as it stands, that is the state after mistark_eval(MISTARK_EVAL_P_G_H), before or after mistark_project. Any
 *   potential qualifies, user-defined ones included. Refused when no Hessians have been evaluated, and for a potential whose current Hessians are the
 *   float blocks of the lazy path (option lazy_eval).
 * source 1: a fresh evaluation at the current DoFs with the generic kernel of the potential's kind, into a pool of the report's own (one potential at a
 *   time: 72 NB^2 bytes per element of the largest). Refuses user-defined potentials and sharded contexts with the force readout's messages. With option
 *   force_generic = 1 the evaluation's own Hessians come from the same kernel, and source 1 equals source 0 to the bit.
 * Also refused: registration-only contexts, bad or duplicate ids, any other source.
 * The eigenvalues come from the projection's own iteration (cyclic-by-round Jacobi, the same pair schedule, stop rule off <= 1e-24 ||H||_F^2, at most 30
 * sweeps, the same guard on tiny off-diagonal entries), so the test `l < eps` is decided as mistark_project decides it, up to rounding.
 * Element record, 10 doubles: 0 lambda_min | 1 lambda_max | 2 eigenvalues < eps | 3 eigenvalues < 0 | 4 deficit sqrt(sum_{l < eps} (eps - l)^2), the
 *   Frobenius norm of what a clamping projection adds | 5 ||H||_F of the stored entries | 6 trace of the stored diagonal | 7 sweeps run | 8 sqrt(off) at
 *   the stop: by Weyl every sorted eigenvalue is within this of a true one, up to rounding | 9 flags: +1 field 2 > 0 (mistark_project would change the
 *   element), +2 a stored entry is not finite (fields 0..8 and the spectrum are zeros), +4 not converged in 30 sweeps.
 * Nodal record, 5 doubles per block row: 0 elements touching the row | 1 of them flagged +1 | 2 smallest lambda_min among the finite ones (0 where none)
 *   | 3 sum of deficit^2 | 4 potential id holding the smallest (-1 where none; the first in the order of the list, then of the elements).
 * Potential record, 10 doubles: 0 elements | 1 flagged +1 | 2 with lambda_min < 0 | 3 non-finite | 4 not converged | 5 smallest lambda_min | 6 first
 *   element attaining it (-1: none) | 7 largest lambda_max | 8 sqrt(sum deficit^2) | 9 first non-finite element (-1: none). 5..7 run over the finite ones. */
/* out: [element][10] or NULL; spectrum: [element][3 NB] ascending (ties in index order) or NULL; both NULL: n_elem and nb alone, nothing is launched. */
int mistark_potential_spectrum_report(mistark_ctx* ctx, int potential, int source, double eps, double* out, double* spectrum, int64_t* n_elem, int32_t* nb);
/* out_host[block row][5] over the listed potentials. */
int mistark_nodal_spectrum(mistark_ctx* ctx, const int32_t* potentials, int32_t n, int source, double eps, double* out_host);
/* out[k][10] for the k-th listed potential; one without elements reports zeros with -1 in slots 6 and 9. */
int mistark_spectrum_potential_report(mistark_ctx* ctx, const int32_t* potentials, int32_t n, int source, double eps, double* out);

/* ---- linear-system report ---------------------------------------------------------------------------------------------------------
 * What the linear solver is given: the spectrum of the assembled matrix as it stands (the state after mistark_assemble, the static and the dynamic part
 * together), its conditioning, the extreme modes and who carries them. Lanczos with full reorthogonalisation (two passes of classical Gram-Schmidt per
 * step) in double on the device; a pipeline of its own beside mistark_eval and mistark_pcg, read-only on what the solver owns, without floating-point
 * atomics, bit-reproducible, and nothing is launched unless it is called. Each call is a fresh, deterministic run; no state is kept between calls.
 * Operators: MISTARK_LINSYS_A, B = A; MISTARK_LINSYS_JACOBI, B = L^-1 A L^-T with L block diagonal and L_r L_r^T = D_r the 3x3 Cholesky in double of the
 *   row's stored float diagonal block. The eigenvalues of B are those of A x = lambda D x, the spectrum the block-Jacobi PCG works on. PCG itself applies
 *   the inverse of D_r computed and stored in float; the two differ by the rounding of that inverse. If any D_r has a pivot <= 0 nothing is iterated and the
 *   record says so (flag +8, slots 11..14): a finding in itself.
 * Iteration j = 0 .. m-1, 1 <= m <= 256: w = B v_j; alpha_j = v_j . w; w -= alpha_j v_j + beta_{j-1} v_{j-1}; two Gram-Schmidt passes against v_0 .. v_j;
 *   beta_j = |w|; T_norm = max_j (|alpha_j| + beta_j + beta_{j-1}). It stops after step j when beta_j <= 1e-10 T_norm (flag +1), j + 1 == m or j + 1 == n;
 *   otherwise v_{j+1} = w / beta_j. With k steps run, T is the k x k tridiagonal matrix, (theta_i, s_i) its eigenpairs (a symmetric QL solver of the
 *   library's own, in double on the host) and rho_i = beta_{k-1} |s_i[k-1]| the residual bound of Ritz value i: in exact arithmetic some eigenvalue of B
 *   lies within rho_i of theta_i.
 * start_host NULL: the built-in vector, in DoF order (the order mistark_spmv takes its host vectors in) entry i from z = (i+1) * 0x9E3779B97F4A7C15,
 *   z = (z ^ z>>30) * 0xBF58476D1CE4E5B9, z = (z ^ z>>27) * 0x94D049BB133111EB, z ^= z>>31 in uint64, value (z >> 11) * 2^-52 - 1, then normalised.
 *   Otherwise the caller's ndofs doubles (minus the gradient of the last evaluation gives the Ritz values PCG from x0 = 0 meets). A zero or non-finite
 *   start vector is refused.
 * Summary record, 16 doubles: 0 steps run k | 1 flags | 2 theta_min | 3 its rho | 4 theta_max | 5 its rho | 6 theta_max / theta_min, 0 where theta_min <= 0
 *   | 7 T_norm | 8 beta_{k-1} | 9 Ritz values < 0 | 10 Ritz values with rho_i <= 1e-8 T_norm | 11 diagonal blocks that are not positive definite | 12 the
 *   first such block row, or -1 | 13 smallest squared Cholesky pivot over all rows | 14 its row | 15 n. Slots 11..14 are filled for both operators.
 *   Flags: +1 Krylov space exhausted | +2 theta_min < -64 eps T_norm (Ritz values lie inside the spectrum's range, so the matrix is proved indefinite) | +4 a
 *   non-finite value was met, slots 2..10 are zeros | +8 operator 1 refused for a diagonal block that is not PD, slots 0 and 2..10 are zeros.
 * Mode record, 4 doubles: 0 theta | 1 rho | 2 |B u - theta u| measured by one more operator application, a true a-posteriori residual, not the recurrence's
 *   | 3 the index in the ascending list.
 * Nodal record, 4 doubles per block row: 0 |u_r|^2, the row's share of the unit Ritz vector u = V s (the shares sum to 1) | 1 |x_r| | 2 trace of D_r | 3
 *   smallest squared pivot of D_r.
 * Potential record, 4 doubles: 0 sum q_e, summed in element order | 1 sum |q_e| | 2 elements that contribute: a stored entry of H_e is not zero (an element
 *   whose condition is off stores zeros) | 3 first element attaining the largest |q_e|, or -1; q_e = x_e^T H_e x_e over the element-Hessian pool as it
 *   stands, x the Ritz vector in DoF space. Over all potentials slot 0 adds up to x^T A x, which is theta under the normalisation below. Refused as source 0
 *   of the spectrum report is: no Hessians evaluated, the float blocks of the lazy path. User-defined potentials are allowed.
 * Refused with an error: registration-only contexts, sharded contexts, no assembled matrix, m out of range, a bad operator, a bad which, bad or duplicate
 *   potential ids. When every output pointer is NULL nothing is launched. */
enum { MISTARK_LINSYS_A = 0, MISTARK_LINSYS_JACOBI = 1 };
/* out[16]; ritz[m][2] = theta ascending, rho (rows >= k zero) or NULL; tri[m][2] = alpha_j, beta_j or NULL; k_out: steps run */
int mistark_linsys_report(mistark_ctx* ctx, int op, int m, const double* start_host, double* out, double* ritz, double* tri, int32_t* k_out);
/* which[i] >= 0: i-th smallest Ritz value; < 0: counted from the largest (-1 = largest).
   x_host[n_which][ndofs] or NULL: x with x^T D x = 1 (op 1) or |x| = 1 (op 0), DoF order.
   nodal[n_which][block rows][4] or NULL.  mode[n_which][4]. */
int mistark_linsys_modes(mistark_ctx* ctx, int op, int m, const double* start_host, const int32_t* which, int32_t n_which, double* x_host, double* nodal, double* mode);
/* rhs_host[ndofs]: minus the gradient of the last evaluation in DoF order, the right-hand side mistark_pcg solves for; as start_host it gives the Ritz
   values PCG from x0 = 0 meets. Single-rank accessor. */
int mistark_linsys_rhs(mistark_ctx* ctx, double* rhs_host);
/* out[n][4] for the n listed potentials, for one Ritz vector */
int mistark_linsys_potential_shares(mistark_ctx* ctx, int op, int m, const double* start_host, int32_t which, const int32_t* potentials, int32_t n, double* out);

/* ---- rigid-body wrench report -------------------------------------------------------------------------------------------------
 * The free-body diagram of a rigid body: force and torque on it from any potential (rows) and from any family of potentials (bodies), at the current
 * DoFs. Every rigid potential places a body through t1 = t0 + dt v1 and the normalised quaternion q0 + dt/2 (0, w1) q0, that is R1 = C(a) R0 with C the
 * Cayley rotation of a = dt w1 / 2 in the world frame, so for any of them
 *     F       = -(1/dt) dE/dv1
 *     tau_com = -(1/dt) (I + [a]x + a a^T) dE/dw1          (torque about t1, world frame; N and N m with STARK's velocity DoFs)
 * without a derivation per kind. mistark_forces returns -dE/dw1 / dt for a body's angular block: a generalised force on the angular-velocity DoF, which is
 * the torque only while w1 dt is small. The report is the torque the solver balances, the exact virtual work of the potential as evaluated: for the lagged
 * friction tables it need not equal r x ft of the friction report (mistark_contact.h): their contact-point velocity v1 + w1 x r1 reads w1 itself and is no
 * pure function of the pose. The force is the report's ft; the torque is (I + [a]x + a a^T) (r1 x ft) + 2 r1 x (ft x a), off r1 x ft in first order of
 * |a| (measured on the recorded scenes: up to 0.75 % of a table's largest r1 x ft at |a| = 5e-3).
 * v1, w1, t0, q0: array ids of the bodies' state as mistark_rigid_budget takes them (v1, w1 DoF arrays of stride 3; all four with n_bodies items); dt is
 * the one the first registered inertia potential has bound (EnergyRigidBodyInertia_Linear's, else EnergyLumpedInertia's, which serves a scene without
 * bodies), read back once per call that launches. A pipeline of its own beside mistark_eval: nothing the evaluation, the solver or the contact detector
 * owns is written, contact and friction tables are read as installed, no floating-point atomics (two reports of one state give the same bits), nothing is
 * launched unless called. Single-rank accessor; refuses registration-only contexts, user-defined potentials, bad and duplicate ids.
 *
 * Rows. out[e][2][12], ids[e][4], rows as mistark_potential_element_forces has them. An element's DoF blocks are classed by block row as "v of body b",
 * "w of body b" or "not rigid"; the blocks of one body are added in block order. Slot 0 is the body that appears first; a third body sets a flag and is
 * dropped (no built-in potential has one). Per slot:
 *   0..2 F | 3..5 tau_com | 6..8 arm F x tau_com / |F|^2: the point of the line of action nearest to the centre of mass, relative to t1 | 9 couple along F,
 *   tau_com . F / |F| | 10 |F| | 11 |tau_com|   (6..9 are zero where |F| == 0)
 * ids: 0 body of slot 0 or -1 | 1 body of slot 1 or -1 | 2 number of rigid blocks | 3 flags: +1 the element's condition is off (the record is zeros),
 *   +2 more than two bodies, +4 a gradient block of a body is not finite
 * A potential without a rigid block is legal: zeros with bodies -1. out and ids both NULL: n_rows alone, nothing is launched. */
int mistark_potential_rigid_wrench(mistark_ctx* ctx, int potential, int v1, int w1, int t0, int q0, int32_t n_bodies, double* out, int32_t* ids, int64_t* n_rows);
/* Bodies. Family f lists the potential ids families[family_start[f] .. family_start[f + 1]); an empty list means every potential: the unbalanced wrench,
 * the body's Newton residual in N and N m. The generalised force of a family is formed by the force readout's nodal stage, so slots 0..2 and 9..11 are the
 * bits mistark_forces returns with scale 1/dt for the body's v and w block. out[f][b][16]:
 *   0..2 F | 3..5 tau_com | 6..8 torque about `about`, tau_com + (t1 - about) x F | 9..11 -dE/dw1 / dt as it came | 12..14 t1 | 15 |a|
 * count[f][b]: the elements of the family whose condition is on and that touch the body (integers). Either output may be NULL. */
int mistark_rigid_wrench(mistark_ctx* ctx, const int32_t* families, const int32_t* family_start, int32_t n_families, int v1, int w1, int t0, int q0, int32_t n_bodies,
                         const double about[3], double* out, int32_t* count);

/* ---- projection + assembly ------------------------------------------------------------------------------------------ */
/* ElementHessians::project_to_PD_inplace__all / project_to_PD_for_update__selectively (ElementHessians.cpp:48-67,79-182;
 * project_to_PD.cpp:12-32). active_blocks: NULL = all elements, else ndofs/3 flags; only not-yet-projected elements
 * touching an active block are projected. Returns counts through the out-pointers (may be NULL). */
int mistark_project(mistark_ctx* ctx, double eps, int mirroring, const uint8_t* active_blocks, int64_t* n_projected_now,
                    int64_t* n_changed_now);
/* Same selection rule evaluated on the device from the current gradient: block active iff max|grad_block| >= threshold
 * (NewtonsMethod.cpp:314-323). all_active_out: 1 if every block was active. */
int mistark_project_by_gradient(mistark_ctx* ctx, double eps, int mirroring, double threshold, int* all_active_out,
                                int64_t* n_projected_now);
/* ElementHessians::assemble_global (ElementHessians.cpp:224-256): element blocks -> float 3x3-block CSR. */
int mistark_assemble(mistark_ctx* ctx);
/* Parity access to the assembled matrix (BlockedSparseMatrix::to_triplets): block CSR, vals row-major 3x3 floats. */
int mistark_get_bsr(mistark_ctx* ctx, int64_t* n_block_rows, int64_t* nnzb, int64_t* row_ptr, int32_t* cols, float* vals);
/* Probes: y = A x (BlockedSparseMatrix::spmxv_from_ptr), z = M^-1 x (prepare/apply_preconditioning). Host vectors. */
int mistark_spmv(mistark_ctx* ctx, const double* x_host, double* y_host);
int mistark_apply_preconditioner(mistark_ctx* ctx, const double* x_host, double* z_host);

/* ---- linear solve --------------------------------------------------------------------------------------------------- */
typedef struct mistark_pcg_info
{
    int32_t converged;
    int32_t n_iterations;
    int32_t found_indefiniteness;
    int32_t reserved;
    double error;
} mistark_pcg_info;
/* bsm::solve_pcg (BlockedSparseMatrix/solve_pcg.h:83-232) with x0 = 0 and rhs = -grad of the last evaluation
 * (NewtonsMethod.cpp:392,431-446). The solution stays on the device as the Newton step `du`; du_host may be NULL. */
int mistark_pcg(mistark_ctx* ctx, double abs_tol, double rel_tol, int max_iter, int stop_on_indefiniteness, double* du_host,
                mistark_pcg_info* info);
/* Same with an explicit host rhs (parity tests). */
int mistark_pcg_rhs(mistark_ctx* ctx, const double* rhs_host, double abs_tol, double rel_tol, int max_iter,
                    int stop_on_indefiniteness, double* x_host, mistark_pcg_info* info);
/* symx::LinearSolver::DirectLLT as a staged call (NewtonsMethod.cpp:395-418: Eigen::SimplicialLLT of the assembled matrix): x = A^-1 rhs by a
 * Cholesky factorisation in double on the device — dense up to 3072 unknowns, block-tridiagonal on a reverse Cuthill-McKee ordering while the
 * band is cheap, multifrontal on a nested-dissection ordering beyond (option "llt_multifrontal": 1 = always, -1 = never). *success = 0 when a
 * pivot is not positive (the reference's "solve failed"). */
int mistark_direct_llt_rhs(mistark_ctx* ctx, const double* rhs_host, double* x_host, int* success);

/* ---- Newton's method -------------------------------------------------------------------------------------------------- */
/* symx::SolverReturn (symx/src/solver/solver_utils.h:15-26) */
enum
{
    MISTARK_SUCCESSFUL = 0,
    MISTARK_RUNNING = 1,
    MISTARK_INVALID_INITIAL_STATE = 2,
    MISTARK_TOO_MANY_ITERATIONS = 3,
    MISTARK_TOO_MANY_ARMIJO_ITERATIONS = 4,
    MISTARK_LINEAR_SYSTEM_SOLVE_FAILURE = 5,
    MISTARK_TOO_MANY_INVALID_INTERMEDIATE_ITERATIONS = 6,
    MISTARK_STEP_DOES_NOT_DESCEND = 7,
    MISTARK_INVALID_CONVERGED_STATE = 8
};
/* symx::ProjectionToPD (solver_utils.h:137-143) */
enum { MISTARK_PROJ_NEWTON = 0, MISTARK_PROJ_PROJECTED_NEWTON = 1, MISTARK_PROJ_ON_DEMAND = 2, MISTARK_PROJ_PROGRESSIVE = 3 };

/* symx::NewtonSettings (solver_utils.h:173-259) with STARK's overrides as defaults (stark/src/core/Settings.cpp:43-50) */
/* symx::LinearSolver. DirectLLT (NewtonsMethod.cpp:395-418) is a dense Cholesky for small systems (<= 3072 unknowns); larger ones are an error. */
enum
{
    MISTARK_SOLVER_BDPCG = 0,
    MISTARK_SOLVER_DIRECT_LLT = 1
};
typedef struct mistark_newton_settings
{
    int32_t max_iterations;
    int32_t min_iterations;
    double residual_tolerance_abs;
    double residual_tolerance_rel;
    double step_tolerance;
    int32_t max_iterations_as_success;
    double step_cap;
    int32_t enable_armijo_backtracking;
    double line_search_armijo_beta;
    int32_t max_backtracking_armijo_iterations;
    int32_t max_backtracking_invalid_state_iterations;
    int32_t projection_mode;
    double projection_eps;
    int32_t project_to_pd_use_mirroring;
    int32_t project_on_demand_countdown;
    double ppn_tightening_factor;
    double ppn_release_factor;
    int32_t cg_max_iterations;
    double cg_abs_tolerance;
    double cg_rel_tolerance;
    int32_t cg_stop_on_indefiniteness;
    double bailout_residual;
    int32_t linear_solver; /* symx::LinearSolver (solver_utils.h): MISTARK_SOLVER_BDPCG (default) or MISTARK_SOLVER_DIRECT_LLT */
} mistark_newton_settings;
void mistark_newton_default_settings(mistark_newton_settings* s);

/* NewtonsMethod::SolveStats (NewtonsMethod.h:32-43) + wall-clock per stage (the reference's Logger timers) */
typedef struct mistark_newton_stats
{
    int32_t newton_iterations;
    int32_t cg_iterations;
    int32_t ls_cap_iterations;
    int32_t ls_max_iterations;
    int32_t ls_inv_iterations;
    int32_t ls_bt_iterations;
    int64_t n_hessians;
    int64_t n_projected_hessians;
    double projected_hessians_ratio;
    int32_t n_linear_solves;
    int32_t n_evaluations;
    double t_eval_pgh;
    double t_eval_p;
    double t_project;
    double t_assembly;
    double t_linear_solve;
    double t_callbacks;
    double t_total;
} mistark_newton_stats;

/* One record per Newton iteration of the last mistark_newton_solve: what the reference appends to its Logger series inside the loop
 * (NewtonsMethod.cpp:198-207 "n_hessians", "n_projected_hessians", "cg_iterations" = the iterations of the LAST linear solve of the
 * iteration, :488-594 "ls_cap", "ls_max", "ls_inv", "ls_bt") and prints at Verbosity::Full (r0, du). `logged` = the iteration got past
 * its linear solves (the first group of series has an entry), `line_search` = its line search ran (the ls_* series have one). */
typedef struct mistark_newton_iteration
{
    double residual;             /* r0 at the iteration's evaluation */
    double du_max;               /* max |du| of the accepted solve */
    int32_t linear_solves;       /* solves of this iteration (progressive projection retries included) */
    int32_t cg_iterations_last;  /* the reference's per-iteration "cg_iterations" */
    int32_t cg_iterations_all;   /* over all solves of the iteration */
    int32_t logged;
    int64_t n_hessians;
    int64_t n_projected_hessians;
    int32_t line_search;
    int32_t ls_cap, ls_max, ls_inv, ls_bt;
    int32_t reserved;
} mistark_newton_iteration;
/* Copies up to `cap` records into `out`; *n = number of records the last solve produced. */
int mistark_newton_iteration_log(mistark_ctx* ctx, mistark_newton_iteration* out, int32_t cap, int32_t* n);

/* symx::SolverCallbacks (solver_utils.h:29-117). Any pointer may be NULL. Callbacks run on the calling thread; they may
 * call mistark_* functions on the same context (e.g. download positions, update contact connectivity). */
typedef struct mistark_newton_callbacks
{
    void* user;
    void (*before_energy_evaluation)(void* user);
    int (*is_initial_state_valid)(void* user);
    int (*is_intermediate_state_valid)(void* user);
    void (*on_intermediate_state_invalid)(void* user);
    void (*on_armijo_fail)(void* user);
    int (*is_converged)(void* user);
    int (*is_converged_state_valid)(void* user);
    double (*max_allowed_step)(void* user);
} mistark_newton_callbacks;

/* NewtonsMethod::solve (NewtonsMethod.cpp:28-252). Returns a MISTARK_* SolverReturn code (>= 0) or < 0 on engine error. */
int mistark_newton_solve(mistark_ctx* ctx, const mistark_newton_settings* settings, const mistark_newton_callbacks* callbacks,
                         mistark_newton_stats* stats);

/* ---- options --------------------------------------------------------------------------------------------------------- */
/* Engine switches (all default 0): "force_generic" = evaluate every potential through the generic hyper-dual kernels (the
 * closed-form kernels are then cross-checked against them; "generic_contact" = the same for the contact and friction potentials only;
 * "contact_closed_min_lanes" = N: closed-form contact kernels for tables with at least N (contact, DoF pair) lanes, 0 = always, default
 * -1 = by potential, see launch_eval);
 * "generic_inertia" = EnergyLumpedInertia through the generic kernel (six lanes per node; default: one lane per node, the same bits);
 * "atomic_assembly" = scatter assembly with float atomics
 * instead of the deterministic gather; "proj_variant" = PSD projection cross-checks, bits: 1 = eigen-decomposition with the
 * matrix in LDS instead of registers, 2 = one launch per potential instead of one for all short lists, 4 = IEEE division /
 * square root for the rotation angles, 8 = the full-size matrix for translation-invariant elements too (default: their reduced
 * matrix); "spmv_chunk_tiles" = tiles per SpMV chunk (0 = by matrix size); "no_contact_cache" = run every contact search in full
 * (no answer from the installed tables, no shared box list, count read back before the sort); "lazy_hessians" = 0: the Newton loop
 * keeps the double element-Hessian pool (default 1: float upper triangles, doubles recomputed for projected elements);
 * "lazy_eval" = staged mistark_eval calls take the lazy path too; "no_grad_gather" = gradient by atomics in arrival order instead of
 * the per-potential pools summed in list order;
 * "no_multi_eval_p" = one launch per potential in energy-only evaluations (default: the small potentials share one launch);
 * "no_eval_prelaunch" = do not start the large potentials' kernels ahead of the callback that precedes an evaluation;
 * "no_pattern_overlap" / "no_eval_overlap" / "no_bounded_pattern" = switch off, one by one, the side stream for the contact part's
 * pattern, the auxiliary stream for small potentials, the device-side counts of the pattern build.
 * Returns 0, or < 0 for an unknown name. The environment variable
 * MISTARK_OPTIONS="name=value,name=value" applies the same switches inside mistark_create (for a process that cannot be
 * edited: a test suite, a profiler run); a bad entry makes mistark_create fail with -6. MISTARK_POISON=1 fills every fresh
 * device allocation with a NaN pattern (finds reads of memory nobody wrote; the GPU test suite passes with it).
 * MISTARK_NEWTON_TRACE=1 prints one line per Newton iteration and linear solve on stderr (residual, CG iterations, tolerance,
 * converged / indefinite, projection threshold, max |du|): what the reference prints at symx::Verbosity::Full. */
int mistark_set_option(mistark_ctx* ctx, const char* name, int value);

/* ---- timers ------------------------------------------------------------------------------------------------------- */
/* Average duration in ms of the SpMV kernel over the launches since the last reset, measured with HIP events on the
 * engine's stream; n = number of launches measured. Used by bench.py for the roofline figure. */
int mistark_spmv_timing(mistark_ctx* ctx, int reset, double* avg_ms, int64_t* n, double* bytes_per_launch);
/* Average duration in ms of the EMPTY event brackets recorded right behind the timed launches: what a pair of event records costs the
 * stream by itself (call before the reset of mistark_spmv_timing). */
int mistark_spmv_event_overhead(mistark_ctx* ctx, double* avg_ms);
/* The same sampled launches on the device's constant clock: every workgroup records when it started and finished, the host takes
 * max(end) - min(start) — the launch's execution time inside the solver loop, which is what rocprofv3's kernel trace reports, without
 * the dispatch latency and marker packets an event bracket contains (call before the reset of mistark_spmv_timing). */
int mistark_spmv_device_clock(mistark_ctx* ctx, double* avg_ms, int64_t* n);
/* Micro-benchmark: n back-to-back SpMV launches on the currently assembled matrix, average duration in microseconds. */
int mistark_spmv_bench(mistark_ctx* ctx, int n_launches, double* avg_us);
/* Waits until everything queued on the engine's stream has finished (entry points that return values already do; assemble / project /
 * axpby only enqueue). For timing from the host. */
int mistark_sync(mistark_ctx* ctx);
/* Event counters of the context, by name (tests assert that a feature under test actually ran): "dof_skips_verified" (MISTARK_VERIFY_DOF_SKIP=1: DoF
 * transfers skipped at an unchanged iterate and checked against a real transfer), "fused_solves" / "unfused_solves" (sharded PCG),
 * "rtc_builds" / "rtc_launches" / "rtc_build_ms" (user-defined potentials: kernels emitted and compiled by hipRTC, their launches, build time),
 * "multi_pgh_launches" (evaluations whose contact / friction tables shared one launch; option no_multi_eval_pgh = 1: one launch per table),
 * "contact_searches" / "contact_repeated_searches" (barrier-table searches that ran on the device / that ran at the state the previous one had
 * searched: 0 unless the option no_contact_cache is set), "eval_pgh_issue_us" / "eval_pgh_wait_us" (host microseconds of the P+g+H evaluations:
 * issuing their launches / waiting for their read-backs), "ccd_queries" / "ccd_skipped_pairs" / "ccd_capped_pairs" (mistark_contact_max_step: queries,
 * candidate pairs skipped because they touch at the line search's start, pairs whose additive CCD stopped at its iteration cap), "ccd_rounds" /
 * "ccd_pad_bound_pairs" (mistark_contact_max_step_ex: passes of the CCD chain its queries made, pairs still pad-bound when a query's rounds ran out),
 * "asm_short_slots_P" / "asm_long_slots_P" / "asm_vlong_slots_P" (P = 0 static, 1 dynamic matrix part: BSR blocks of the current pattern summed by
 * the one-lane / one-wavefront / 64-wavefront gather kernel, by the length of their contribution lists), "llt_path" / "llt_panel_rows" /
 * "llt_panels" / "llt_fronts" (the last DirectLLT solve: 0 dense, 1 band, 2 multifrontal, -1 none yet; block rows per panel — multifrontal: of the
 * largest front —, panels, fronts), "force_readouts" (force readout calls that launched) / "force_long_rows" (block rows of the last readout
 * that were summed by a whole wavefront: more than 256 contributions), "stress_readouts" / "stress_long_rows" (the same two for the stress readout:
 * calls that launched, rows of the last nodal readout summed by a whole wavefront), "budget_readouts" / "budget_chunks" (budget readout calls that
 * launched, chunks of the element list the last inertia budget was summed in), "contact_reports" / "contact_report_long_rows" (contact report calls
 * that launched, mistark_contact.h; collision vertices of the last report summed by a whole wavefront), "friction_reports" / "friction_report_long_rows"
 * (the same two for the friction report), "constraint_reports" / "constraint_report_chunks" (constraint report calls that launched, chunks the last group
 * report was summed in), "bending_reports" / "bending_report_long_rows" / "bending_report_chunks" (bending report calls that launched, block rows of the
 * last nodal stage summed by a whole wavefront, chunks the last group stage was summed in), "wrench_reports" / "wrench_long_rows" (wrench report calls
 * that launched, rigid-body block rows of the last body report summed by a whole wavefront, over all its families), "spectrum_reports" /
 * "spectrum_report_long_rows" / "spectrum_report_chunks" (spectrum report calls that launched, block rows of the last nodal stage handled by a whole
 * wavefront: more than 64 contributions, chunks the last potential stage was summed in), "linsys_reports" (linear-system report calls that launched). */
int mistark_get_counter(mistark_ctx* ctx, const char* name, int64_t* out);

/* ---- multi-GPU: one problem sharded over `world` ranks, one engine context (and one process) per GPU ------------------------
 * Block rows are partitioned over the ranks (owner map: mistark_dist_set_row_owner, or a graph partition of the potentials' connectivity).
 * A rank evaluates every element that touches one of its rows (interface elements are evaluated by both sides: no gradient / Hessian
 * traffic), assembles and solves ITS rows of the system (block-Jacobi PCG on a row-sharded matrix: the ghosts of the search direction
 * from their owners and the three dot products of solve_pcg.h:180,201,217 are exchanged in every iteration, (r.r, r.z) fused), and
 * holds the whole state (DoFs, bound arrays, contact tables), so every rank runs the same host code and takes the same decisions.
 * All exchanges are all-gathers on the engine's stream: stores into IPC windows of the peers (below), ncclAllGather over xGMI (RCCL), or a copy
 * kernel for ranks inside one process.
 * Reductions are done by every rank in rank order: identical bits everywhere. Call right after mistark_create, before the first
 * evaluation. With N ranks mistark_get_bsr / mistark_apply_preconditioner are not available (single-rank accessors). */
int mistark_shard_range(int64_t n, int rank, int world, int64_t* begin, int64_t* end); /* [n*rank/world, n*(rank+1)/world) */
/* The built-in graph partition as a host function (no GPU, no context): tables of elements given by their block rows (rows[t][e * nb[t] + k]),
 * hub[r] != 0 marks rows kept out of the graph (given to the last rank; NULL: none). Breadth-first order from a pseudo-peripheral row, cut
 * into `world` pieces of equal element incidence. */
int mistark_partition_rows(int64_t n_block_rows, int world, int n_tables, const int32_t* const* rows, const int64_t* n_elem, const int32_t* nb, const uint8_t* hub,
                           int32_t* owner_out);
int mistark_dist_unique_id(char out[128]);  /* rank 0: ncclGetUniqueId, to be broadcast by the launcher (e.g. torch.distributed) */
int mistark_dist_init_rccl(mistark_ctx* ctx, int rank, int world, const char unique_id[128]);
/* Moves the communicator (rank, world, transport) of `from` to `ctx`; `from` becomes a single-rank context (a scene that registers
 * again keeps its communicator: an RCCL unique id is single-use). */
int mistark_dist_move(mistark_ctx* ctx, mistark_ctx* from);
/* one-rank RCCL round trip (all-gather of `inout`) through the dlopen'ed entry points the N-rank path uses */
int mistark_dist_rccl_selftest(mistark_ctx* ctx, double* inout, int64_t n);
/* Explicit partition: owner[r] in [0, world) for every block row r of the flat DoF vector (e.g. slabs along the longest axis from the
 * scene's positions). owner == NULL returns to the built-in graph partition. */
int mistark_dist_set_row_owner(mistark_ctx* ctx, const int32_t* owner, int64_t n_block_rows);
int64_t mistark_dof_set_first_row(mistark_ctx* ctx, int set);  /* first block row of a DoF set in the flat DoF vector (< 0: no such set) */
/* A position per block row (xyz[3 r ..], NaN for rows without one: rigid bodies keep the last rank): the rows are partitioned by recursive
 * coordinate bisection, weighted by element incidences — box-like parts with few interface rows. The host mirror passes the rest positions
 * of its point sets. An explicit owner map takes precedence; without either the built-in graph partition is used. */
int mistark_dist_set_row_coords(mistark_ctx* ctx, const double* xyz, int64_t n_block_rows);
/* Block rows that potentials with device-side connectivity may reference on any rank; every rank keeps them as ghosts. The contact system
 * registers the collision vertices of its deformable meshes itself; small DoF sets (rigid bodies) are always shared. */
int mistark_dist_add_shared_rows(mistark_ctx* ctx, const int32_t* rows, int64_t n);
/* out[0..15): block rows owned by this rank, ghosts, rows it sends, elements it evaluates, blocks of its static / contact matrix part, linear
 * solves that took the fused iteration (one exposed exchange, ranks exchanging through windows) and the five-launch one; [8] world and [9] rank
 * of the context, [10] transport (0 none, 1 in-process group, 2 RCCL, 3 IPC windows), [11] ranks the transport itself counts (RCCL:
 * ncclCommCount of the communicator), [12] contact searches whose sweep was dealt out to the ranks (keys all-gathered and merged), [13] elements
 * of all potentials with fixed connectivity as registered (the unsharded problem) and [14] those of them this rank evaluates */
int mistark_dist_info(mistark_ctx* ctx, int64_t* out, int n);
int mistark_dist_get_row_owner(mistark_ctx* ctx, int32_t* owner);
/* ---- IPC windows: one process per rank, no library in the data path -----------------------------------------------------------------
 * Every rank owns a window of device memory that the other ranks map with hipIpcOpenMemHandle (the peers' GPUs through the xGMI aperture,
 * or the same GPU when several ranks share one device — how a one-GPU box runs the real multi-process launch path). An exchange is: the
 * producing kernel stores its values into every rank's window as 8-byte {sequence tag, 32 data bits} granules (system-scope write-through
 * stores), the consuming kernel polls its own window until the granules carry the tag. No host involvement, no library launch, no separate
 * flag: one exchange costs the one-way store latency. Waits are bounded (MISTARK_IPC_TIMEOUT_S, default 30 s): a peer that never delivers
 * turns into an error at the host's next synchronisation point instead of a hung GPU.
 *   create (allocates and zeroes the window; `handle_out` = its 64-byte hipIpcMemHandle_t)  ->  the launcher all-gathers the handles (bench.py:
 *   torch.distributed / gloo)  ->  connect (handles of all ranks in rank order, n_bytes = world * 64)  ->  mistark_dist_init_ipc(ctx, comm).
 * window_bytes: at least 48 bytes per DoF of the largest problem (smaller messages than a slot travel in one piece, longer ones in several);
 * 0 = the minimum. The communicator must outlive the contexts using it. */
typedef struct mistark_ipc_comm mistark_ipc_comm;
mistark_ipc_comm* mistark_ipc_comm_create(int device, int rank, int world, int64_t window_bytes, char handle_out[64]);
int mistark_ipc_comm_connect(mistark_ipc_comm* comm, const char* handles, int64_t n_bytes);
const char* mistark_ipc_comm_last_error(mistark_ipc_comm* comm);
void mistark_ipc_comm_destroy(mistark_ipc_comm* comm);
int mistark_dist_init_ipc(mistark_ctx* ctx, mistark_ipc_comm* comm);
/* `iters` all-gathers of n doubles with predictable values, every received value checked; avg_us[0] = wall time of one exchange + stream
 * synchronisation, avg_us[1] = of one exchange in a train enqueued back to back. Collective: every rank calls it with the same arguments. */
int mistark_ipc_comm_selftest(mistark_ipc_comm* comm, int64_t n, int iters, double avg_us[2]);
/* Pre-flight of the windows: one tagged granule over every ordered pair of ranks (ping-pong, `iters` >= 2 exchanges per pair, the first of a
 * pair discarded), every wait bounded by timeout_s (clamped to 2 s). half_rtt_us[p] = half the best round trip with peer p in microseconds
 * (0 for the own rank, < 0 where no granule came back). Returns the number of peers that answered (world - 1 = the windows deliver), < 0 on
 * error. Collective: every rank calls it with the same arguments, a host barrier in front (the kernels must start within the time-out of each
 * other). A launcher that sees fewer than world - 1 on any rank falls back to RCCL and says so (bench.py). */
int mistark_ipc_comm_preflight(mistark_ipc_comm* comm, int iters, double timeout_s, double* half_rtt_us /* world */);
/* The two all-reduces the reference's parallel reductions turn into on N GPUs, on RCCL whatever transport the engine runs on: ncclAllReduce
 * (f64, sum) of n_big doubles (the gradient of the shared DoFs: symx SecondOrderCompiledGlobal.cpp:72-142) and of 3 doubles (the dot products of
 * a CG iteration: BlockedSparseMatrix/solve_pcg.h:180,201,217), `reps` launches each back to back between HIP events, results checked.
 * out[0] = ncclCommCount, out[1] = microseconds per all-reduce of n_big doubles, out[2] = of 3 doubles, out[3] = seconds in ncclCommInitRank.
 * Collective; one rank per device (RCCL refuses two ranks on one device: the error text lands in err). No engine context involved. */
int mistark_rccl_allreduce_bench(int device, int rank, int world, const char unique_id[128], int64_t n_big, int reps, double* out /* 4 */, char* err, int err_len);
/* Measurement: solo durations (microseconds) of the two kernels of the fused PCG iteration on THIS rank's rows — out[0] = the SpMV with its
 * halo polls, out[1] = the vector kernel (whose workgroup 0 reduces and pushes the rank's three sums) — replayed from the rank's
 * last converged solve on the messages still in its window (every poll answered at once). Not a collective: the caller lets the ranks take
 * turns (a host barrier between them), so the figures are kernels running alone even when all ranks share one GPU; no rank may start a solve
 * in between. Needs ranks that exchange through windows and a converged solve on the current matrix. */
int mistark_dist_fused_bench(mistark_ctx* ctx, int n_launches, double* out);
/* the same sharded path with several contexts inside one process (one host thread per context, one device, one shared stream), used by
 * the single-GPU tests */
typedef struct mistark_local_group mistark_local_group;
mistark_local_group* mistark_local_group_create(int world);
void mistark_local_group_destroy(mistark_local_group* group);
int mistark_dist_init_local(mistark_ctx* ctx, mistark_local_group* group, int rank);

#ifdef __cplusplus
}
#endif
#endif
