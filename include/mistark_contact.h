/* mistark_contact.h — C ABI of the device contact detector (IPC proximity + intersection detection, contact and friction
 * table construction). Drop-in for the part of stark::EnergyFrictionalContact that runs inside the Newton loop:
 *
 *   EnergyFrictionalContact::add_triangles / add_edges           (EnergyFrictionalContact.cpp:54-91)   -> mistark_contact_add_mesh
 *   EnergyFrictionalContact::set_friction / disable_collision    (:102-119)                            -> mistark_contact_set_friction / _disable_collision
 *   _before_energy_evaluation__update_contacts                   (:368-530)                            -> mistark_contact_update
 *   _before_time_step__update_friction_contacts                  (:531-773)                            -> mistark_contact_update_friction
 *   _is_intermediate_state_valid (tmcd::IntersectionDetection)   (:774-799)                            -> mistark_contact_count_intersections
 *   the 21 barrier + 14 friction add_potential calls             (:829-1218)                           -> mistark_contact_init
 *
 * The reference keeps the collision meshes, the tmcd broad/narrow phase and the LabelledConnectivity tables on the host
 * and refills them at every energy evaluation. Here the meshes live in HBM, detection/classification/routing run as HIP
 * kernels, and the tables are written where the potentials' kernels read them; only the row counts cross PCIe.
 * Row CONTENT is the reference's (same columns, same A/B roles); row ORDER is deterministic (sorted by pair id) instead of
 * the reference's thread-dependent order.
 */
#ifndef MISTARK_CONTACT_H
#define MISTARK_CONTACT_H
#include "mistark.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Engine array ids (mistark_array) of the state the contact potentials bind, named after the reference's members.
 * -1 for a physical system the scene does not have. */
typedef struct mistark_contact_arrays
{
    int32_t v1;        /* PointDynamics::v1   (DoF)                       stride 3 */
    int32_t x0;        /* PointDynamics::x0                               stride 3 */
    int32_t X;         /* PointDynamics::X    (rest)                      stride 3 */
    int32_t dt;        /* Stark::dt                                       stride 1, 1 item */
    int32_t k;         /* EnergyFrictionalContact::contact_stiffness      stride 1, 1 item */
    int32_t thickness; /* EnergyFrictionalContact::contact_thicknesses    stride 1, one item per collision mesh (group) */
    int32_t epsv;      /* GlobalParams::friction_stick_slide_threshold    stride 1, 1 item */
    int32_t rb_xloc;   /* EnergyFrictionalContact::rigidbody_local_vertices  stride 3 */
    int32_t rb_v1;     /* RigidBodyDynamics::v1 (DoF)                     stride 3 */
    int32_t rb_w1;     /* RigidBodyDynamics::w1 (DoF)                     stride 3 */
    int32_t rb_t0;     /* RigidBodyDynamics::t0                           stride 3 */
    int32_t rb_q0;     /* RigidBodyDynamics::q0_                          stride 4 */
} mistark_contact_arrays;

enum { MISTARK_CONTACT_DEFORMABLE = 0, MISTARK_CONTACT_RIGIDBODY = 1 };

/* Creates the detector and registers the 35 contact/friction potentials (empty tables) in the dynamic matrix part. */
int mistark_contact_init(mistark_ctx* ctx, const mistark_contact_arrays* arrays);

/* One collision mesh (EnergyFrictionalContact::Handler group). vertex_index[i]: index of collision vertex i in the physical
 * system's vertex array (PointDynamics global index, or rigidbody_local_vertices global index). triangles / edges: local
 * connectivity. Returns the group id. Rigid meshes get their self collision disabled (EnergyFrictionalContact.cpp:208-209). */
int mistark_contact_add_mesh(mistark_ctx* ctx, int kind, int idx_in_ps, const int32_t* vertex_index, int32_t n_vertices, const int32_t* triangles,
                             int32_t n_triangles, const int32_t* edges, int32_t n_edges);
int mistark_contact_set_friction(mistark_ctx* ctx, int group_a, int group_b, double mu);
int mistark_contact_disable_collision(mistark_ctx* ctx, int group_a, int group_b);
int mistark_contact_enable(mistark_ctx* ctx, int point_triangle, int edge_edge);
/* Candidate search: 0 (default) = sweep and prune over sorted boxes, 1 = LDS-tiled all-pairs (ablation / cross-check). Same pair set. */
int mistark_contact_set_broad_phase(mistark_ctx* ctx, int brute_force);

/* Barrier tables for the positions x0 + dt v1 (v1 = the engine's current DoFs). n_contacts: total rows (nullable). */
int mistark_contact_update(mistark_ctx* ctx, double dt, int64_t* n_contacts);
/* Friction tables (connectivity, T, mu, fn, barycentric coordinates) at x0. */
int mistark_contact_update_friction(mistark_ctx* ctx, int64_t* n_contacts);
/* Number of intersecting edge-triangle pairs at x0 + dt v1. */
int mistark_contact_count_intersections(mistark_ctx* ctx, double dt, int64_t* n_found);

/* Continuous collision detection: largest fraction t in (0, 1] of the current Newton direction along which no collision pair's distance falls
 * below (1 - conservative_rescaling) of its distance at the line search's start (additive CCD on linear vertex trajectories: positions x0 + dt v1
 * at the engine's DoFs u and at u + du; rigid-body rotation is linearised between the two — mistark_contact_max_step_ex below has a mode that is sound
 * for the true rotation). Meaningful inside a max_allowed_step callback.
 * Returns 1 when collisions are disabled or nothing moves. A sharded context returns an error. n_candidates: pairs whose swept boxes overlap
 * (nullable). Leaves the installed tables and the detection caches alone. */
int mistark_contact_max_step(mistark_ctx* ctx, double dt, double conservative_rescaling, double* max_step, int64_t* n_candidates);

/* The same query with the choice of how rigid bodies move, and along a direction of the caller's.
 *   rigid_mode 0 (linear): mistark_contact_max_step itself — rigid vertices on the chord between their positions at u and at u + du.
 *   rigid_mode 1 (curved): sound for the true motion. A rigid vertex follows t -> t0 + dt (v + t dv) + R1(q0, w + t dw, dt) x_loc, which leaves the chord
 *     over [0, tau] by at most  delta(tau) = min((7/16) r (phi tau)^2, 2 r),  r = |x_loc|, phi = dt |dw|  (derivation: DESIGN.md section 4). The chord query
 *     runs on the padded distance d~ = d - pad, pad = largest delta on one side of the pair + largest on the other (0.0 for deformable vertices and for
 *     dw == 0): additive CCD with per-pair minimum separation pad. While a surviving pair is pad-bound (pad > d(0) / 2: the pad, not the motion, would stop
 *     the step) the query is repeated on [0, tau / 2] with the end point placed anew at u + (tau / 2) du, which quarters every pad; at most max_rounds
 *     rounds (>= 1), each one more pass of the kernels and one more read-back. max_step = tau * (the last round's result).
 *     Guarantee: for every t in [0, max_step] the true rigid and deformable motion keeps every candidate pair apart (d > 0), and at max_step the pair
 *     that limits it keeps a gap of (1 - conservative_rescaling) (d(0) - pad). A pair that after the last round still has d(0) <= pad gives max_step = 0: the line search
 *     then fails and the caller is expected to shorten dt (which shrinks phi) — conservative, never unsound. With no rotation change (dw == 0 for every body,
 *     or no rigid mesh) max_step, n_candidates and rounds == 1 are rigid_mode 0's bit for bit.
 * du: NULL = the engine's current Newton direction (meaningful inside a max_allowed_step callback); else a host array of mistark_ndofs doubles in the
 * layout of the DoF vector, which makes the query usable outside a Newton solve. The engine's own direction is not touched.
 * Errors: sharded context, conservative_rescaling outside (0, 1], rigid_mode not 0 or 1, max_rounds < 1. Counters: "ccd_rounds", "ccd_pad_bound_pairs". */
typedef struct mistark_ccd_result
{
    double max_step;          /* in [0, 1] */
    double tau;               /* length of the last round's interval: 2^-(rounds - 1) */
    double max_pad;           /* largest pad over the last round's candidates */
    int64_t n_candidates;     /* pairs whose (padded) swept boxes overlap, last round */
    int64_t rounds;           /* passes made (0: no collision mesh) */
    int64_t pad_bound_pairs;  /* surviving pairs of the last round with pad > d(0) / 2 (0 unless the rounds ran out) */
} mistark_ccd_result;
int mistark_contact_max_step_ex(mistark_ctx* ctx, double dt, double conservative_rescaling, int rigid_mode, int max_rounds, const double* du, mistark_ccd_result* out);

/* Parity access: rows of one table (by potential name, e.g. "contact_d_d_pt_pt_cubic"); conn == NULL queries n_rows/stride. */
int mistark_contact_get_table(mistark_ctx* ctx, const char* potential, int32_t* conn, int32_t* n_rows, int32_t* stride);
/* Parity access: friction data of one friction table: T [n x 6], mu [n], fn [n], bary [n x nbary] (nullable outputs). */
int mistark_contact_get_friction_data(mistark_ctx* ctx, const char* potential, double* T, double* mu, double* fn, double* bary, int32_t* nbary);
/* Parity access: collision vertex positions used by the last update [n_collision_vertices x 3]. */
int mistark_contact_get_vertices(mistark_ctx* ctx, double* x, int64_t* n_vertices);

/* ---- contact report (opt-in, not in the reference) -------------------------------------------------------------------------
 * What the contact itself looks like at the current DoFs: which primitives are in contact, how close, where the closest points and the normal lie, how
 * much normal force each pair carries and what pressure that puts on a surface. A pipeline of its own beside mistark_eval, like the force, stress and
 * budget readouts of mistark.h: it reads the key list of the barrier tables as installed (no search runs), recomputes the collision vertices at the
 * current DoFs (x0 + dt v1, rigid bodies as the detector moves them; dt = the bound dt array) into a buffer of its own, and writes nothing the
 * evaluation or the solver own, and nothing of the detector's once a search has run. (Before the first search of a mesh set the collision meshes are not on
 * the device yet: a report then uploads them as that search would — mesh arrays uploaded, the detector's position and box buffers allocated, its box cache
 * marked stale. The size queries below do not even do that.) No floating-point atomics; every sum runs in a fixed order over the row list and through a fixed tree, so a result
 * depends on the row order alone and two reports of one state give the same bits. It costs nothing unless it is called. All three may be called between
 * solves and from any Newton callback. Refused, with the cause in the message: sharded contexts (single-rank accessor), registration-only contexts
 * (mistark_create_dry), contexts without mistark_contact_init. Before the first search, after a change of the mesh set or of the collision switches
 * that has not been searched yet, or with no pair in range: zero rows, gaps +inf, counts 0 — not an error.
 *
 * Rows come in key order, the order of the installed tables: the rows of table t (0..20, the order of the potentials' registration:
 * contact_d_d_pt_pp .. contact_rb_d_ee_ep) are contiguous and correspond one to one to mistark_contact_get_table's. Roles are the key's primitives,
 * not the A / B of the reference's tables: a = the point or the first edge, b = the triangle or the second edge. The distance is that of the closest
 * feature the search classified (point-point, point-line, point-plane, line-line, parameters unclamped), as the table's potential evaluates it; the pair
 * is never classified again.
 *   rows_i [n][8]:  0 table | 1 source (0 point-triangle, 1 edge-edge) | 2 closest-feature type | 3 group of a | 4 group of b | 5 primitive a (global
 *                   collision point / edge) | 6 primitive b (global collision triangle / edge) | 7 flags: +1 mollified (edge-edge row, mollifier < 1),
 *                   +2 open (d >= dhat), +4 degenerate (d zero or not finite: the normal is zeros)
 *   rows_d [n][16]: 0 d | 1 dhat = thickness[ga] + thickness[gb] | 2..4 closest point on a | 5..7 closest point on b | 8..10 unit normal (cA - cB) / d,
 *                   from b to a | 11 mollifier m (1 for point-triangle rows) | 12 fn = m k (dhat - d)^2 [N] | 13 E = m k (dhat - d)^3 / 3 [J], unclamped
 *                   as the potential has it | 14, 15 point-triangle: barycentrics beta1, beta2 of cB (beta0 = 1 - beta1 - beta2); edge-edge: s along a,
 *                   t along b. Node weights: a side [1] or [1 - s, s], b side [beta0, beta1, beta2] or [1 - t, t]; vertex and edge features have
 *                   exact 0 / 1 in the places they do not use.
 * fn of a mollified row is the barrier part only: the force of such a row also has a b grad(m) term.
 * Outputs are nullable: a first call with rows_i = rows_d = NULL gives n_rows from host counts alone: nothing is launched, uploaded or allocated (so do the
 * size queries of the two calls below).
 * Each of the three calls with an output runs the whole pipeline — positions, rows, two radix sorts, the vertex pass, the pair pass — and downloads its own
 * part: a caller who wants all three pays for the pipeline three times (tens of microseconds of kernels each, profiles/contact_report_cost.txt). Nothing is
 * cached between calls, because nothing the engine tracks says that DoFs, state arrays and key list are all unchanged; the host mirror's recording
 * (mistark_sim_record_contacts) runs the pipeline once per step for all three parts.
 * A key that names a primitive outside the meshes (a detector bug, never seen) gives a row of zeros with flag 4 that takes no part in the vertex and pair
 * records. */
int mistark_contact_report(mistark_ctx* ctx, int32_t* rows_i, double* rows_d, int64_t* n_rows);
/* out [n_collision_vertices][5]: 0 gap = the smallest d over the rows whose primitive a or b contains the vertex (+inf: none) | 1 number of such rows |
 * 2 normal force share = sum of w fn over them, w the vertex's node weight in the row (as it is: outside the feature a weight is 0, at a moved state it
 * may leave [0, 1]) | 3 area = a third of the current areas of the vertex's collision triangles (0 for a rod vertex) | 4 pressure = [2] / [3] where
 * [3] > 0, else 0. group [n], source_index [n]: the vertex's group and its index in the physical system's vertex array (mistark_contact_add_mesh's
 * vertex_index), so that a caller can map collision vertices to his own. Every output is nullable. */
int mistark_contact_vertex_report(mistark_ctx* ctx, double* out, int32_t* group, int32_t* source_index, int64_t* n_vertices);
/* out [n_groups][n_groups][8], entries ga <= gb filled, the rest zero: 0 rows | 1 smallest d (+inf: none) | 2 dhat | 3 sum fn | 4..6 sum fn n, oriented as
 * the force on the lower-numbered group (ga == gb: in role order, on a from b) | 7 sum E. out nullable: n_groups alone. */
int mistark_contact_pair_report(mistark_ctx* ctx, double* out, int32_t* n_groups);

/* ---- friction report (opt-in, not in the reference) ------------------------------------------------------------------------
 * What friction does at the current DoFs: which contacts stick and which slide, how fast, how much of mu fn is mobilised, which way the friction force
 * points and how much power it takes out. A pipeline of its own beside mistark_eval, shaped like the contact report above: it reads the friction tables
 * as the last mistark_contact_update_friction installed them (the lagged T, mu, fn and bary; nothing is classified or recomputed from positions), that
 * search's key list (a copy the detector keeps for this report alone: a friction row does not carry its groups) and the velocities of the current DoFs
 * (v1, rb_v1, rb_w1; rb_q0, rb_xloc, dt and epsv as bound), and writes only buffers of its own. No floating-point atomics; every sum runs in a fixed
 * order over the row list and through a fixed tree, so two reports of one state give the same bits. It costs nothing unless it is called. Refused, with
 * the cause in the message: sharded contexts, registration-only contexts, contexts without mistark_contact_init. Zero rows (vertex and pair records of
 * zeros), not an error: before the first friction update, after a mesh was added and friction has not been updated since, with friction off or every mu
 * zero (the friction search then routes no row).
 *
 * Everything is as the table's potential evaluates it. Roles follow the potential: v = v_B - v_A with B the side whose contact-point velocity the
 * potential takes positive. That is the search's detected (A, B) — in friction_rb_d_ep / _tp the deformable point is A although the row lists it last —
 * except in rows of friction_rb_d_pp and friction_rb_d_ee whose detected A is deformable: the reference lists and subtracts the rigid side there, so
 * the rigid side is A. Contact-point velocity of a side: the bary combination of its vertices' velocities (a rigid vertex: rb_v1 + rb_w1 x (R1 xloc));
 * u0 = T[0:3].v dt + 1.13e-9, u1 = T[3:6].v dt - 1.07e-9 (the reference's offsets), epsu = dt epsv; sticking iff |u| < epsu;
 * E = 0.5 (mu fn / epsu) |u|^2 sticking, mu fn (|u| - epsu / 2) sliding; force on A: ft = c (u0 T[0:3] + u1 T[3:6]), c = mu fn / epsu sticking,
 * mu fn / |u| sliding; on B: -ft. Torques on rigid bodies are not reported here: the wrench report (mistark.h, "rigid-body wrench
 * report") gives the torque of every friction table on a body, as the exact virtual work of the lagged potential, which need not equal r x ft.
 * Rows come in key order = table order: the rows of table t (21..34, friction_d_d_pp_C0 .. friction_rb_d_tp_C0) are contiguous and line up with
 * mistark_contact_get_table's and mistark_contact_get_friction_data's.
 *   rows_i [n][8]:  0 table | 1 row in that table | 2 kind (0 pp, 1 pe, 2 pt, 3 ee, 4 ep, 5 tp) | 3 group of A | 4 group of B | 5 rigid body of A or -1 |
 *                   6 rigid body of B or -1 | 7 flags: +1 sliding, +2 mu fn == 0, +4 degenerate (a key outside the meshes — a detector bug, never seen —:
 *                   a row of zeros that takes no part in the vertex and pair records)
 *   rows_d [n][24]: 0 mu | 1 lagged fn | 2 epsu | 3 u0 | 4 u1 | 5 |u| | 6 slip speed |u| / dt | 7..9 v | 10..12 ft | 13 |ft| | 14 mobilised = |ft| / (mu fn),
 *                   never above 1, 0 where mu fn == 0 | 15 dissipation = ft.v [W] | 16 E | 17 A-side parameter s (ee rows, else 0) | 18..20 B-side weights |
 *                   21..23 zero. Node weights: A [1] or [1 - s, s]; B [1], [b0, b1], [b0, b1, b2] or [1 - t, t]; the force on a deformable node is +w ft
 *                   on A and -w ft on B, the linear force on a rigid body +ft / -ft.
 * Outputs are nullable; a call with every output NULL answers the size from host counts: nothing is launched, uploaded or allocated. Each call with an
 * output runs the whole pipeline and downloads its own part; nothing is cached between calls (mistark_sim_record_friction runs it once per step). */
int mistark_contact_friction_report(mistark_ctx* ctx, int32_t* rows_i, double* rows_d, int64_t* n_rows);
/* out [n_collision_vertices][8]: 0 rows the vertex takes part in | 1 sliding ones among them | 2..4 friction force on the vertex = sum of s w ft over them
 * (s = +1 on A, -1 on B, w the vertex's node weight) | 5 largest slip speed over them (0: none) | 6 area = a third of the current areas of the vertex's
 * collision triangles (computed only while the report has rows, else 0) | 7 shear traction = |[2..4]| / [6] where [6] > 0, else 0. group, source_index as
 * mistark_contact_vertex_report. */
int mistark_contact_friction_vertex_report(mistark_ctx* ctx, double* out, int32_t* group, int32_t* source_index, int64_t* n_vertices);
/* out [n_groups][n_groups][12], entries ga <= gb filled, the rest zero: 0 rows | 1 sliding rows | 2 sum fn | 3 sum mu fn | 4..6 sum ft oriented as the force
 * on the lower-numbered group (ga == gb: in role order, on A) | 7 sum |ft| | 8 sum dissipation | 9 sum E | 10 largest slip speed | 11 [7] / [3] (0 where
 * [3] is 0). out nullable: n_groups alone. */
int mistark_contact_friction_pair_report(mistark_ctx* ctx, double* out, int32_t* n_groups);

/* Binding recipe of one of the 35 potentials: (role, stride, connectivity column) per binding in the reference's order;
 * roles index the members of mistark_contact_arrays (0..11), 12 = T, 13 = mu, 14 = fn, 15 = bary. Returns n_bindings. */
int mistark_contact_recipe(const char* potential, int32_t* conn_stride, int32_t* roles, int32_t* strides, int32_t* conn_cols);

#ifdef __cplusplus
}
#endif
#endif
