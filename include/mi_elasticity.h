/*
 * mi_elasticity.h -- C-ABI of the MI355X-native structural-elasticity hot path.
 *
 * This is the drop-in boundary for the hot path of precice/dealii-adapter's nonlinear solver
 * (source/nonlinear_elasticity/nonlinear_elasticity.cc): one Newmark step =
 * Newton iterations x (cell tangent/residual assembly + CG) + Newmark vector updates.
 * The host-side Solid<dim>/Adapter (dealii-adapter_amd/host/) call exactly these entry points at the
 * sites cited below; nothing else crosses the boundary.  All device memory is owned by the opaque
 * context; the host only passes interface-sized buffers and scalars (plain pointers + sizes).
 *
 * Conventions: every function returns MI_OK (0) or a negative MI_E* code; mi_last_error() gives text.
 * One host thread per context; a context is not re-entrant.  DoF numbering is node-major:
 * dof = dim*node + component; nodes are lexicographic (x fastest) on the (p*reps+1)^dim lattice.
 */
#ifndef MI_ELASTICITY_H
#define MI_ELASTICITY_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MI_OK 0
#define MI_EINVAL (-1)      /* bad argument / unsupported (dim, degree)            */
#define MI_EHIP (-2)        /* HIP runtime error                                   */
#define MI_ENOCONV_LIN (-3) /* CG hit max iterations (SolverControl::NoConvergence) */
#define MI_ENOCONV_NR (-4)  /* "No convergence in nonlinear solver!" (nonlinear_elasticity.cc:497) */
#define MI_ECOMM (-5)       /* RCCL error                                          */

/* role of each side of the box, order x-,x+,y-,y+,z-,z+ (deal.II colorize ids 0..5,
 * nonlinear_elasticity.cc:237-241), values = the ids the reference relabels to (:255-278, .h:256-257) */
#define MI_FACE_FREE 0
#define MI_FACE_CLAMPED 1   /* clamped_boundary_id: u = 0                     */
#define MI_FACE_INTERFACE 7 /* boundary_interface_id: coupling traction       */
#define MI_FACE_ZCLAMP 8    /* out_of_plane_clamped_mesh_id: u_z = 0 (3D)     */

typedef struct mi_ctx mi_ctx;

/* replaces make_grid (nonlinear_elasticity.cc:171-301) + system_setup (:305-380) inputs */
typedef struct
{
  int32_t       dim;       /* 2 or 3 (the reference's -DDIM, CMakeLists.txt:15-18)        */
  int32_t       degree;    /* FE_Q degree ("Polynomial degree", parameters.cc:110-113)    */
  int32_t       reps[3];   /* subdivided_hyper_rectangle repetitions                      */
  double        lo[3], hi[3];
  int32_t       face_role[6];
  const double *vertex_perturbation; /* optional nverts*dim offsets (tests), else NULL    */
} mi_mesh_desc;

/* parameters.cc:35-50 */
typedef struct
{
  double mu, nu, rho;
  double body_force[3];
} mi_material_desc;

/* parameters.cc:120-125, parameters.cc:12-15; alpha_1..6 derived as nonlinear_elasticity.h:242-250 */
typedef struct
{
  double beta, gamma, delta_t;
} mi_newmark_desc;

/* domain decomposition into `size` slabs along one box direction (`cut_axis`), one slab per process/GPU with ghost planes
 * exchanged by ncclSend/ncclRecv and scalars by ncclAllReduce (RCCL over xGMI).  size==1 (or a NULL descriptor):
 * single GPU.  rank == -1: all `size` slabs are created inside this process on one device and advance in
 * lockstep (test mode: lets the decomposition be checked on a single-GPU box).  All entry points keep speaking
 * GLOBAL arrays in every mode.  The reference has no counterpart (adapter.h:152-154 hard-codes one rank). */
typedef struct
{
  int32_t     rank, size;
  const void *nccl_unique_id; /* 128-byte ncclUniqueId from mi_comm_unique_id(), the same on all ranks */
  int32_t     cut_axis;       /* direction the slabs are cut along: 0 = automatic (the one with most cell layers; ties: the
                                 last, i.e. z-slabs of a cube), 1 / 2 / 3 = x / y / z.  The reference's flap is 18 x 3 (x 1)
                                 cells (nonlinear_elasticity.cc:189-205): only x can be cut into more than 3 parts */
} mi_comm_desc;

/* host-only description of one slab (no device needed; used by the multi-process CPU tests) */
typedef struct
{
  int32_t z0, z1, local_layers;      /* owned cell layers [z0,z1); layers of the local box (incl. ghost layer) */
  int64_t plane_nodes, node_offset;  /* nodes per lattice plane; global id of local node 0                    */
  int64_t nnodes_global, nnodes_local;
  int64_t own_begin, own_end;        /* owned LOCAL node range                                                */
  int64_t up_send, up_send_n, up_recv, up_recv_n;         /* LOCAL node ranges exchanged with rank+1          */
  int64_t down_send, down_send_n, down_recv, down_recv_n; /* ... and with rank-1                              */
  int32_t local_reps[3];
  double  local_lo[3], local_hi[3];
  int32_t local_face_role[6];
} mi_partition_info;
int mi_partition_describe(const mi_mesh_desc *mesh, int rank, int size, mi_partition_info *out);
/* host-only: the row order of the slab's SpMV (sliced-ELL, 64 rows per slice).  rows[] receives the LOCAL node of
 * every slot (-1 = padding) if it is not NULL and capacity suffices; slots [0, 64*n_interior_slices) hold the rows
 * without ghost columns (computed while the halo exchange is in flight), the rest the rows that wait for it. */
int mi_partition_spmv_rows(const mi_mesh_desc *mesh, int rank, int size, int64_t *n_slices, int64_t *n_interior_slices,
                           int32_t *rows, int64_t capacity);
int mi_comm_unique_id(void *out128); /* ncclGetUniqueId */
/* slabs of the decomposition this context belongs to, and ncclCommCount of its RCCL communicator (0: none) */
int mi_comm_info(const mi_ctx *ctx, int *team_size, int *rccl_ranks);
/* values[0..n) of rank 0 to every rank of the decomposition (collective; no-op in one process).  The reference couples
 * through ONE process (adapter.h:152-154, 213-225): with several GPUs only rank 0 owns the precice::Participant and what
 * it reads -- coupling data (:346-361), isCouplingOngoing, getMaxTimeStepSize, the checkpoint requests (:447-489) --
 * travels to the other ranks through this call (host/include/adapter/rank_zero_participant.h). */
int mi_comm_broadcast(mi_ctx *ctx, double *values, int32_t n);

/* parameters.cc:61-99 ("Solver" subsection) */
typedef struct
{
  double  tol_lin;            /* "Residual": CG stops at ||r|| <= tol_lin*||rhs||  (:1171-1172) */
  double  max_iterations_lin; /* "Max iteration multiplier" (x n_dofs)             (:1169-1170) */
  int32_t max_iterations_NR;  /* :436 */
  double  tol_f, tol_u;       /* :459-463 */
} mi_solver_desc;

typedef struct
{
  int32_t newton_iterations; /* linear solves done                          */
  int32_t assemblies;        /* = newton_iterations + 1 when converged      */
  int32_t lin_its_total;
  int32_t converged;
  double  res_norm, res_abs, upd_norm, upd_abs; /* last Newton table row (:489-494) */
  int32_t lin_its[16];       /* per Newton iteration (first 16)             */
  double  lin_res[16];
} mi_step_info;

/* ---- lifetime ---------------------------------------------------------------------------- */
int         mi_ctx_create(const mi_mesh_desc *mesh, const mi_material_desc *mat, const mi_newmark_desc *nm,
                          int device_id, const mi_comm_desc *comm, mi_ctx **out);
void        mi_ctx_destroy(mi_ctx *ctx);
const char *mi_last_error(const mi_ctx *ctx); /* ctx may be NULL: error of the last failed create */

/* ---- sizes / topology (global numbers, identical on every rank) --------------------------- */
int64_t mi_n_dofs(const mi_ctx *ctx);
int64_t mi_n_nodes(const mi_ctx *ctx);
int64_t mi_n_cells(const mi_ctx *ctx);
int64_t mi_nnz(const mi_ctx *ctx);   /* scalar non-zeros of the tangent (= dim^2 * stored blocks) */
int     mi_n_colours(const mi_ctx *ctx);
int     mi_get_node_coords(const mi_ctx *ctx, double *xyz /* n_nodes*dim */);
int     mi_get_constrained(const mi_ctx *ctx, uint8_t *flags /* n_dofs */);

/* ---- coupling interface: replaces Adapter::format_* (adapter.h:389-443) ------------------- */
/* interface nodes = nodes on MI_FACE_INTERFACE sides in ascending node (= x-dof) order (adapter.h:313-321);
 * coords interleaved [x0,y0,(z0),x1,...] exactly as passed to precice::setMeshVertices (adapter.h:305-326) */
int mi_n_interface_nodes(const mi_ctx *ctx);
int mi_get_interface_nodes(const mi_ctx *ctx, int32_t *node_ids, double *coords);
/* external_stress[interface dofs] = vals (format_precice_to_deal, adapter.h:421-443); vals [x0,y0,(z0),...] */
int mi_set_interface_traction(mi_ctx *ctx, int n, const double *vals);
/* vals = total_displacement[interface dofs] (format_deal_to_precice, adapter.h:389-417) */
int mi_get_interface_displacement(mi_ctx *ctx, int n, double *vals);

/* ---- the hot path, piecewise (call sites in solve_nonlinear_timestep, :410-499) ----------- */
int mi_newton_begin_step(mi_ctx *ctx);              /* solution_delta = 0 (:121); newton_update = 0 (:419) */
int mi_update_acceleration(mi_ctx *ctx);            /* :444 -> :592-599                                   */
int mi_assemble(mi_ctx *ctx, double *res_norm);     /* :446 -> :1044-1087 incl. Neumann :791-859, scatter
                                                       :760-774; *res_norm = get_error_residual :549-560  */
/* the same system_rhs and norm WITHOUT the tangent (bit-identical residual; tangent, Jacobi diagonal and multigrid
 * hierarchy keep the state of the last mi_assemble): for the assembly that only feeds the convergence test of
 * :459-463 -- callers use it when the update criterion already holds and fall back to mi_assemble if the residual
 * criterion fails.  No reference counterpart (the reference always builds both, :1078-1084). */
int mi_assemble_residual(mi_ctx *ctx, double *res_norm);
int mi_cg_solve(mi_ctx *ctx, double rel_tol, int64_t max_it, int *its, double *res);
                                                    /* :472 -> :1153-1191 (Jacobi-PCG, warm start) + :1208 */
/* "Solver type = Direct" (SparseDirectUMFPACK re-factorised in every Newton iteration, :1192-1200; the reference's shipped
 * default, parameters.prm:43): banded Cholesky factorisation of the current tangent + substitution on the device (one
 * workgroup; nodes renumbered with the shortest lattice direction fastest), then :1208.  *res = 0 as in :1199.  Meant for
 * the sizes of the reference's own geometries: MI_EINVAL ("too large ...") beyond ~3e8 flops of factorisation or on a
 * decomposed mesh -- callers then use mi_cg_solve at a tolerance of 1e-12.  MI_ENOCONV_LIN: non-positive pivot.
 * mi_set_tuning("solver_type", 1) makes mi_newmark_step and mi_linear_step solve this way (with that fallback); the
 * linear model factorises its constant matrix once (linear_elasticity.cc:553-559). */
int mi_direct_solve(mi_ctx *ctx, double *res);
int mi_apply_newton_update(mi_ctx *ctx, double *upd_norm); /* get_error_update :564-576; delta += update :487; then
                                                       the consumed update is cleared, so that the next solve of the
                                                       step starts from zero -- unless mi_set_tuning("cg_warm_start", 1)
                                                       asks for the reference's start vector, the previous update
                                                       (:419, :472-473: 28 instead of 22 CG iterations per step), or
                                                       "cg_warm_start" 2 for the solution of the same solve of the
                                                       previous time step (what the executable sets: 19-20) */
int mi_newmark_finish_step(mi_ctx *ctx);            /* :139-144: u += delta; a, v updates; old := new      */
/* the whole of solve_nonlinear_timestep + :139-144 with the reference's convergence logic */
int mi_newmark_step(mi_ctx *ctx, const mi_solver_desc *s, mi_step_info *info);

/* implicit-coupling checkpoint of the 6 state vectors (adapter.h:447-489), device-to-device */
int mi_state_save(mi_ctx *ctx);
int mi_state_restore(mi_ctx *ctx);

/* ---- energy diagnostics ------------------------------------------------------------------ */
/* What the structure holds, summed on the device.  The reference has the stored-energy function (get_Psi) but never
 * integrates it; a caller logs these per step to watch drift, an unstable coupling, or whether a run has settled.
 * NOT a term: the work of the interface traction.  With the reference's pull-back at the cell point (nonlinear_elasticity.cc:
 * 825-827) that load has no potential; a caller who wants a balance accumulates f_ext . delta u itself. */
typedef struct
{
  double strain;   /* nonlinear: sum over cells and points of Psi(F(u)) JxW, Psi = get_Psi = kappa/4 (J^2 - 1 - 2 ln J) +
                      mu/2 (J^(-2/dim) tr(F F^T) - dim) (compressible_neo_hook_material.h:30-35, 62-72), rule qf_cell =
                      QGauss(p+2) (nonlinear_elasticity.cc:74); linear: 1/2 u^T K u                                     */
  double kinetic;  /* 1/2 rho int |v_h|^2 on the model's own rule = 1/2 v^T M v with the consistent mass the model
                      itself uses (nonlinear: QGauss(p+2); linear: the M of linear_elasticity.cc:248-374, QGauss(p+1))  */
  double body;     /* potential of the body force: -rho int b . u_h  (linear: -u . body-force vector of :358-373)       */
  double reserved; /* 0 */
} mi_energy_info;
/* Nonlinear model, COMMITTED state: reads MI_V_TOTAL_DISPLACEMENT and MI_V_VELOCITY alone -- not + MI_V_SOLUTION_DELTA:
 * after mi_newmark_finish_step the delta is already folded into u; inside a step the numbers are those of the last
 * finished step.  Modifies no vector, record, matrix, hierarchy, counter or timing, and needs no matrix: every (dim, degree)
 * an assembly supports, "fine_level" 0 and 1, after a "linear_operator" 1 set-up has released the tangent array, single,
 * emulated and RCCL teams (collective: every rank calls and receives the same numbers; each slab sums the cells it owns).
 * Bitwise repeatable (per-cell sums, then a fixed-order reduction; no floating-point atomics).  A point with det F <= 0:
 * MI_EINVAL "inverted element" as from mi_assemble, since ln J has no value there. */
int mi_energy(mi_ctx *ctx, mi_energy_info *out);

/* Nodal stress field: what the stress is and where it is largest.  The reference's post-processor stops at the symmetric
 * gradient (postprocessor.h:61-75); the Kirchhoff stress tau of every residual pass is dropped after its contraction with
 * grad N.  This is the lumped L2 projection of the stress onto the nodes, in the reference configuration, with N_i the scalar
 * shape function of node i and the model's own quadrature rule:
 *     W_i       = sum_cells sum_q N_i(q) JxW(q)                          (lumped weight; sum_i W_i = volume)
 *     sigma_i   = ( sum_cells sum_q N_i(q) sigma(q) JxW(q) ) / W_i
 * MI_STRESS_NEOHOOKE: sigma(q) = tau(F)/J, the Cauchy stress of the compressible neo-Hookean material at F = I + grad u
 *   (compressible_neo_hook_material.h:62-138), u = MI_V_TOTAL_DISPLACEMENT, the COMMITTED state as for mi_energy, on
 *   qf_cell = QGauss(p+2) (nonlinear_elasticity.cc:74).  A point with det F <= 0: MI_EINVAL "inverted element" as from
 *   mi_assemble / mi_energy; the context works afterwards (the arrays then hold no result).
 * MI_STRESS_LINEAR: sigma(q) = lambda tr(eps) I + 2 mu eps, eps = sym grad u, lambda = 2 mu nu / (1 - 2 nu) (parameters.cc:189),
 *   u = MI_L_DISPLACEMENT (the same slot), on the linear model's QGauss(p+1) (linear_elasticity.cc:61).  Needs no mi_linear_setup.
 * sigma [n_nodes][ncomp] (required), ncomp = dim (dim + 1) / 2, in the order xx, yy, zz, xy, xz, yz (3D) or xx, yy, xy (2D);
 * von_mises [n_nodes] and weight [n_nodes] each optional (NULL = not wanted); global arrays in the reference's node order.
 * All nodes, constrained ones too.  von_mises is formed from the projected NODAL tensor, not projected itself: 3D
 * sqrt(3/2 s : s), s = sigma - tr(sigma)/3 I; 2D the in-plane form sqrt(sxx^2 - sxx syy + syy^2 + 3 sxy^2), because the
 * reference's 2D formulation has no sigma_zz.  W_i > 0 on the meshes the library builds (smallest at Q3 / Q4 corner nodes).
 * Modifies no state vector, record, matrix, hierarchy, counter or timing (scratch of its own is allocated on first use) and
 * needs no matrix: every (dim, degree) an assembly supports, "fine_level" 0 and 1, after a "linear_operator" 1 set-up has
 * released the tangent array.  Bitwise repeatable: the cells add to the nodes colour by colour, the colours in order; no
 * floating-point atomics.  Single contexts and emulated slabs (each slab computes the cells it holds and hands over the
 * nodes it owns); on an RCCL team MI_EINVAL "one process only", as mi_get_diagonal_blocks.  A bad model, a NULL sigma or a
 * NULL ctx: MI_EINVAL. */
#define MI_STRESS_NEOHOOKE 0
#define MI_STRESS_LINEAR   1
int mi_stress_field(mi_ctx *ctx, int model, double *sigma, double *von_mises, double *weight);

/* A posteriori stress error indicator: how far to trust that stress on this mesh.  The Zienkiewicz-Zhu distance between the
 * recovered field sigma* of mi_stress_field(model) and the raw stress sigma_h of the elements, same state, same rule,
 * reference configuration.  With sigma*(q) = sum_i N_i(q) sigma*_i and e(q) = sigma*(q) - sigma_h(q):
 *     m(s)    = ( s:s - c tr(s)^2 ) / (2 mu)      s:s counts each off-diagonal entry twice; c = nu / (1 + nu) in 3D and
 *                                                 c = nu in 2D (the plane-strain compliance of the reference's 2 x 2
 *                                                 formulation, which has no sigma_zz)
 *     eta_K^2 = sum_{q in K} m(e(q)) JxW(q)       n_K^2 = sum_{q in K} m(sigma_h(q)) JxW(q)
 *     eta = sqrt(sum_K eta_K^2)    n = sqrt(sum_K n_K^2)    relative = eta / sqrt(n^2 + eta^2)   (0 where n = eta = 0)
 * m is the complementary energy density of isotropic linear elasticity, s : C^-1 : s, positive definite for nu < 1/2.  For
 * MI_STRESS_LINEAR n^2 = u^T K u exactly on the model's rule; for MI_STRESS_NEOHOOKE the same metric is applied to the Cauchy
 * stress tau(F)/J: a scaling, not the material's own energy.  sigma_h(q) is what mi_stress_field projects (model 0 on
 * QGauss(p+2), model 1 on QGauss(p+1)).
 * AN INDICATOR, NOT A GUARANTEED BOUND: on smooth fields eta falls like h^p or faster and eta / true error was measured
 * between 0.45 and 1.3, but nothing bounds the error from above by eta.
 * eta_cell, norm_cell [n_cells], each optional (NULL = not wanted): eta_K and n_K (not their squares) in lexicographic cell
 * order with x fastest, cell (i, j, k) at i + reps[0] (j + reps[1] k).  max_cell is the lexicographic id of the largest
 * eta_K, the smallest id on ties.
 * The contract of mi_stress_field: every (dim, degree) an assembly supports, "fine_level" 0 and 1, after a "linear_operator" 1
 * set-up has released the tangent array, model 1 without mi_linear_setup.  Modifies no state vector, record, matrix,
 * hierarchy, counter or timing (scratch of its own is allocated on first use).  Bitwise repeatable: fixed-order sums, no
 * floating-point atomics.  Model 0 with a point of det F <= 0: MI_EINVAL "inverted element"; the context works afterwards.
 * Undecomposed contexts only: on an emulated or RCCL team MI_EINVAL "one slab only", as mi_linear_modes (a slab's first
 * node plane holds a partial sigma*, and the exchange of a six-component nodal field is not provided).  A bad model, a NULL
 * out or a NULL ctx: MI_EINVAL. */
typedef struct
{
  double  error, norm, relative; /* eta, n, eta / sqrt(n^2 + eta^2) */
  double  max_cell_error;        /* largest eta_K */
  int64_t max_cell;              /* its lexicographic cell id; the smallest id on ties */
  int64_t reserved;              /* 0 */
} mi_stress_error_info;
int mi_stress_error(mi_ctx *ctx, int model, mi_stress_error_info *out, double *eta_cell /* [n_cells] or NULL */,
                    double *norm_cell /* [n_cells] or NULL */);

/* Support reactions and load resultants: what the supports carry, and whether the structure is in balance with its loads.
 * Every residual path of the library masks the constrained dofs; this forms the UNMASKED nodal forces, term by term, on every
 * dof (node and dof order of the reference, as every array of this interface), with N_i the scalar shape function of node i:
 * MI_STRESS_NEOHOOKE (0): the Newmark model's COMMITTED state as mi_energy reads it -- u = MI_V_TOTAL_DISPLACEMENT alone (not
 *   + MI_V_SOLUTION_DELTA), a = MI_V_ACCELERATION and MI_V_EXTERNAL_STRESS as they are -- on qf_cell = QGauss(p+2):
 *     internal_i = sum_cells sum_q tau(F) F^-T grad_X N_i JxW      the force the body exerts on the node
 *     inertia_i  = rho sum N_i a_h JxW
 *     body_i     = rho b W_i,  W_i = sum N_i JxW                   the lumped weight of mi_stress_field
 *     load_i     = the interface faces' contribution exactly as the assembly forms it (nonlinear_elasticity.cc:791-859): the
 *                  pull-back at the cell point whose index is the face-point counter, or at the face point with
 *                  "correct_face_F" 1, at the committed displacement
 * MI_STRESS_LINEAR (1), no mi_linear_setup needed for the internal term, on QGauss(p+1):
 *     internal   = K d, formed element by element as the integral of (lambda tr eps I + 2 mu eps) grad N, d = MI_L_DISPLACEMENT
 *     inertia_i  = rho sum N_i a_h JxW,  a = (MI_L_VELOCITY - MI_L_OLD_VELOCITY) / delta_t
 *     load       = MI_L_OLD_STRESS, the load vector F of the last step as assemble_rhs left it (body force and either coupling
 *                  form are in it);  body = 0
 *   THESE ARE THE TERMS OF THE THETA SCHEME, NOT AN EQUILIBRIUM AT ONE TIME.  On the free dofs the scheme's identity is
 *     inertia_{n+1} + theta (internal - load)_{n+1} + (1 - theta) (internal - load)_n = (A v - rhs) / delta_t,
 *   so a single call balances (to the solver's residual) only for theta = 1; for another theta combine the terms of two calls.
 * forces = internal + inertia - body - load, the out-of-balance force r.  Reaction: r on the dofs mi_get_constrained flags, zero
 * elsewhere; unbalanced: r on the free dofs.  Resultant of a nodal vector f over a dof set: sum f_i; moment about x0:
 * sum (x_i - x0) x f_i with x_i = X_i + u_i, the CURRENT positions, for model 0 and x_i = X_i for model 1.  2D: the moment is
 * the z entry alone; entries [0], [1] and the force's [2] are 0.  For any state sum_all internal = 0 and
 * sum_all (x_i - x0) x internal_i = 0 at round-off of internal_abs (translation and rotation invariance), so
 * reaction + unbalanced = inertia - body - load for force and moment.
 * about [dim] or NULL (the origin); forces [n_dofs] or NULL; terms [4][n_dofs] = internal, inertia, body, load, or NULL.
 * The contract of mi_stress_error: every (dim, degree) an assembly supports, "fine_level" 0 and 1, after a "linear_operator" 1
 * set-up has released the tangent array.  Modifies no state vector, record, matrix, hierarchy, tuning key, counter or timing
 * (scratch of its own is allocated on first use).  Bitwise repeatable: the cells add to the nodes colour by colour, the colours
 * in order; the resultants in chunks of 1,024 nodes, then the chunks; no floating-point atomics.  Model 0 with a point of
 * det F <= 0: MI_EINVAL "inverted element"; the context works afterwards.  Undecomposed contexts only: on an emulated or RCCL
 * team MI_EINVAL "one slab only".  A bad model, a NULL out or a NULL ctx: MI_EINVAL. */
typedef struct
{
  double  about[3];                            /* x0 as used */
  double  reaction[3], reaction_moment[3];     /* r over constrained dofs */
  double  unbalanced[3], unbalanced_moment[3]; /* r over free dofs */
  double  inertia[3], inertia_moment[3];       /* all dofs */
  double  body[3], body_moment[3];
  double  load[3], load_moment[3];
  double  internal_abs;                        /* sum |internal_i|: the scale of the round-off identities */
  double  max_unbalanced;                      /* max |r_i| over free dofs */
  double  max_reaction;                        /* largest |R_node|_2 ... */
  int64_t max_reaction_node;                   /* ... and its node, the smallest id on ties */
} mi_reaction_info;
int mi_reactions(mi_ctx *ctx, int model, const double *about /* [dim] or NULL = origin */, mi_reaction_info *out,
                 double *forces /* [n_dofs] r, or NULL */, double *terms /* [4][n_dofs] internal, inertia, body, load, or NULL */);

/* Fields at arbitrary points: u_h(X) = sum_a N_a(xi) u_a at npts points X of the REFERENCE configuration, for n_which state
 * vectors at once (which[]: MI_V_* / MI_L_* ids, 1 <= n_which <= MI_V_COUNT; the vectors as they are, nothing is committed or
 * combined).  xi is the pre-image of X under the d-linear (Q1) map of the cell's (perturbed) vertices, the map the support
 * points of mi_get_node_coords are placed with; N_a the element's Lagrange basis, evaluated at that xi without clamping.
 *   xyz [npts][dim]; values [n_which][npts][dim]; gradients [n_which][npts][dim][dim] = d u_c / d X_d, or NULL; cell [npts] the
 *   lexicographic id of the cell that answered (x fastest, as mi_stress_error), -1 = outside, or NULL; n_outside or NULL.
 * INSIDE is a definition, not a measurement: a point is in a cell when xi lies in [-1e-10, 1 + 1e-10]^dim.  On a shared face, edge
 *   or corner any one of the containing cells may answer: the values are continuous, the gradient and `cell` are those of the
 *   cell chosen, and the choice is deterministic -- two calls return the same bits.
 * OUTSIDE: a point in no cell, NaN coordinates included, gets cell -1 and zeros in values / gradients and is counted in
 *   *n_outside; the call still returns MI_OK.
 * FOUND are all points of the mesh on meshes whose vertex offsets stay below a quarter of the smallest cell edge (every mesh the
 *   suite builds; boxes are the closed-form case): the first guess is the cell of the unperturbed lattice, refined by a walk of at
 *   most three cells along the directions xi leaves through and then by the 3^dim cells around the first guess; xi by Newton
 *   on the Q1 map.  One thread per point (field_at_points), plain stores, the count by a fixed-order sum; no atomics.
 * Modifies no state vector, record, matrix, hierarchy, counter or timing: a following mi_newmark_step / mi_linear_step returns
 *   the bits it would have returned without the call.  Needs no matrix: every (dim, degree) an assembly supports, "fine_level"
 *   0 and 1, after a "linear_operator" 1 set-up.  Scratch of its own, allocated on first use and grown on demand.
 * npts = 0: MI_OK, no array is written (*n_outside = 0).  Undecomposed contexts only: an emulated or RCCL team gives MI_EINVAL
 *   "one slab only", as mi_stress_error.  A NULL ctx, which, xyz or values, a bad vector id, npts < 0 or n_which out of range:
 *   MI_EINVAL. */
int mi_evaluate_points(mi_ctx *ctx, int n_which, const int *which, int64_t npts, const double *xyz, double *values,
                       double *gradients, int64_t *cell, int64_t *n_outside);
/* Stress at arbitrary points: the stress gauge.  npts points X of the REFERENCE configuration, located exactly as
 * mi_evaluate_points locates them -- INSIDE, OUTSIDE, FOUND, the choice on shared faces and the NaN rule are its definitions,
 * the same device functions.  model as mi_stress_field (MI_STRESS_NEOHOOKE / MI_STRESS_LINEAR), the COMMITTED state.
 * MI_STRESS_AT_RAW: sigma_h(X), the stress of the element that answers, from grad u_h at X itself.  Model 0 sigma = tau(F)/J of
 *   the compressible neo-Hookean material at F = I + d u / d X, u = MI_V_TOTAL_DISPLACEMENT; model 1 sigma = lambda tr(eps) I +
 *   2 mu eps, u = MI_L_DISPLACEMENT (the same slot).  Discontinuous across cells: on a shared face the value is the answering
 *   cell's, and `cell` says which.  A requested point with det F <= 0 (model 0): MI_EINVAL "inverted element", the arrays hold no
 *   result, the context works afterwards.  No mesh pass, no scratch beyond the point buffers.
 * MI_STRESS_AT_RECOVERED: sigma*(X) = sum_a N_a(xi(X)) sigma*_a, the nodal field mi_stress_field(model) returns (under tuning
 *   "stress_projection" 0 or 1), interpolated with the element's basis.  Runs that whole-mesh pass first, with its folded-cell
 *   error; continuous across cells; at a node it is the nodal value.
 * sigma [npts][ncomp] (required) in mi_stress_field's component order; von_mises [npts] or NULL, formed from the POINT's tensor by
 * mi_stress_field's formulas; principal [npts][dim] or NULL: the eigenvalues of that tensor in DESCENDING order; directions
 * [npts][dim][dim] or NULL: row k the unit eigenvector of principal[k] (see mi_principal_stress); cell [npts] or NULL;
 * n_outside or NULL.  An outside point gets cell -1 and zeros (its directions: the coordinate axes), is counted, and the call
 * returns MI_OK.  npts = 0: MI_OK, no array is written.
 * The contract of mi_evaluate_points: modifies no state vector, record, matrix, hierarchy, counter or timing -- a following
 * mi_newmark_step / mi_linear_step returns the bits it would have returned without the call; needs no matrix ("fine_level" 0
 * and 1, after a "linear_operator" 1 or 2 set-up); 2D and 3D, degrees 1 to 4; two calls return the same bits.  Undecomposed
 * contexts only: MI_EINVAL "one slab only".  A NULL ctx, xyz or sigma, a bad model or kind, npts < 0: MI_EINVAL. */
#define MI_STRESS_AT_RAW       0
#define MI_STRESS_AT_RECOVERED 1
int mi_evaluate_stress(mi_ctx *ctx, int model, int kind, int64_t npts, const double *xyz /* [npts][dim] */,
                       double *sigma /* [npts][ncomp] */, double *von_mises /* [npts] or NULL */,
                       double *principal /* [npts][dim] descending, or NULL */, double *directions /* [npts][dim][dim] or NULL */,
                       int64_t *cell /* or NULL */, int64_t *n_outside /* or NULL */);
/* Principal stresses of n symmetric tensors, host arrays in and out (as mi_block_gram): sigma [n][ncomp] in mi_stress_field's
 * component order, principal [n][dim] in descending order, directions [n][dim][dim] or NULL with row k the unit eigenvector of
 * principal[k].  The kernel mi_evaluate_stress runs on its points' tensors, one thread per tensor: 3D the cyclic Jacobi method
 * on the 3 x 3 matrix with a fixed count of 8 sweeps; 2D the closed form m +- hypot(d, xy), m = (xx + yy) / 2, d = (xx - yy) / 2.
 * Sign: the component of largest magnitude of each eigenvector is positive, the first such on ties.  Equal eigenvalues keep the
 * order their diagonal entries had, and a degenerate tensor (hydrostatic, zero) gets an orthonormal basis -- a definition, always
 * the same one, not a property of the tensor.  Two calls return the same bits.  Measured against the tensor (not against another
 * solver's vectors, which depend on the gaps): |sigma v - lambda v|_2 and |V^T V - I| are a few units of round-off times
 * |sigma|_F.  Reads and modifies no state; any context of the tensors' dimension, teams included.
 * n = 0: MI_OK.  A NULL ctx, sigma or principal, n < 0: MI_EINVAL. */
int mi_principal_stress(mi_ctx *ctx, int64_t n, const double *sigma /* [n][ncomp] */, double *principal /* [n][dim] */,
                        double *directions /* [n][dim][dim] or NULL */);
/* State transfer between meshes: dst's six state vectors MI_V_TOTAL_DISPLACEMENT .. MI_V_ACCELERATION_OLD := src's fields at
 * dst's nodes, device to device.  BY DEFINITION mi_evaluate_points of src at mi_get_node_coords(dst) for the six vectors, written
 * into dst's vectors with every dof that dst flags constrained (mi_get_constrained) set to exactly 0 -- the same kernel, the same
 * bits as that host route, without the fields passing through the host.
 *   Both contexts: the same dim, the same device, undecomposed; else MI_EINVAL.  A node of dst outside src's mesh: MI_EINVAL naming
 *   the first such node, dst unchanged.
 *   Nodal interpolation, not a projection: exact when dst's space contains src's (box meshes, dst's cells nested in src's, degree
 *   not lower); any other pair is allowed (a coarser or lower-order dst samples src).
 *   Writes nothing else in dst (external stress, delta, update, rhs keep their values) and nothing in src.  Meant for a fresh dst
 *   before its first step; on a stepped dst it has the consequences mi_vec_set of those vectors has. */
int mi_state_transfer(mi_ctx *dst, mi_ctx *src);

/* ---- consistent mass and L2 projection of a state onto another mesh --------------------------------------- */
/* M is the unit-density vector mass of the context's space on the assembly's rule QGauss(p + 2):
 *   M_(i,c)(j,d) = delta_cd sum_cells sum_q N_i N_j JxW,
 * so rho M is the mass the Newmark model integrates its inertia with (1/2 rho v^T M v = mi_energy's kinetic).  On box meshes it
 * equals the linear model's M / rho to rounding; on perturbed cells the linear model's rule QGauss(p + 1) differs (2e-5
 * relative at a 5 % vertex perturbation).  No matrix is formed: the product runs cell by cell, colour by colour, with plain
 * loads and stores in an order the mesh alone fixes -- no atomics, two calls return the same bits.
 * Blocks are [nrhs][n_dofs], 0 <= nrhs <= MI_MASS_MAX_RHS (nrhs = 0: MI_OK, nothing is read or written).
 * masked = 1: x is read as 0 on the dofs mi_get_constrained flags, y and the solution are written exactly 0 there, b is ignored
 *   there; masked = 0: all dofs take part.
 * The calls of this section modify no state vector (but the six target vectors of mi_state_project), record, matrix, hierarchy,
 *   counter or timing, need no matrix ("fine_level" 0 and 1, after a "linear_operator" 1 set-up), and allocate their scratch per
 *   call and free it before they return (mi_mass_solve: 3 nrhs + 1 work vectors).  Undecomposed contexts only, else MI_EINVAL
 *   "one slab only"; a NULL argument or nrhs / masked out of range: MI_EINVAL. */
#define MI_MASS_MAX_RHS 6
int mi_mass_apply(mi_ctx *ctx, int nrhs, int masked, const double *x, double *y); /* y = M x, [nrhs][n_dofs] */
/* x = M^-1 b by a Jacobi-preconditioned CG on all columns at once, start vector 0; the diagonal of M comes from the product
 * kernel's own sums, once per solve.  Column j is converged when |r_j|_2 <= tol |b_j|_2 (the recurrence's residual); a zero
 * column gives x = 0 at once.  A converged column is not updated any more, and every column's dot products are its own: solving
 * columns together returns, column by column, the bits of solving each alone.  The scalars and done-flags stay on the device;
 * the host reads one word per iteration.
 *   res[j] (or NULL) = |b_j - M x_j| / |b_j| on a freshly formed M x_j (0 for a zero column); *its (or NULL) the iteration
 *   count of the slowest column.  Not converged in max_it iterations: MI_ENOCONV_LIN with x, res and its still written. */
int mi_mass_solve(mi_ctx *ctx, int nrhs, int masked, const double *b, double *x, double tol, int max_it, int *its, double *res);
/* Load of src's fields against dst's test functions, b [n_which][n_dofs(dst)] (every dof, nothing masked):
 *   b_(i,c) = sum_{dst cells} sum_q N_i^dst(xi_q) w_c^src(X_q) JxW(q)
 * on a COMPOSITE rule: every dst cell is cut into sub^dim equal boxes in xi (1 <= sub <= 4) with QGauss(p_dst + 2) on each;
 * X_q is the point's image under dst's Q1 map and w^src(X_q) exactly what mi_evaluate_points(src, ...) returns there.
 * When src.reps = sub * dst.reps on the same box the integrand is a polynomial of degree p_dst + p_src <= 2 p_dst + 3 per
 * direction on each sub-box and b is exact; the same holds for sub = 1 on equal cells with any pair of degrees.  Otherwise b is
 * the discrete load of this rule: a definition, not a measurement.  which[]: MI_V_* ids, 0 <= n_which <= 6 (0: MI_OK).
 *   Conditions as mi_state_transfer (same dim, same device, both undecomposed).  A quadrature point outside src's mesh:
 *   MI_EINVAL naming the first dst cell (lexicographic id) and its point.  The points go through the evaluation in chunks of
 *   whole cells of one colour (point scratch <= 256 MiB; tuning key "project_chunk_cells", 0 = automatic, forces a size for
 *   tests): the result does not depend on the chunk size bit for bit. */
int mi_project_load(mi_ctx *dst, mi_ctx *src, int n_which, const int *which, int sub, double *b);
typedef struct
{
  int32_t its, sub;
  int64_t n_points;  /* points of the composite rule over dst */
  double  res;       /* worst column's |b - M w| / |b| */
  double  src_sq[6]; /* sum_q |w_src(X_q)|^2 JxW on the composite rule */
  double  dst_sq[6]; /* w_dst^T M w_dst */
} mi_project_info;
/* L2 projection of src's state onto dst's space: for each of the six vectors MI_V_TOTAL_DISPLACEMENT .. MI_V_ACCELERATION_OLD,
 * w_dst = 0 on dst's constrained dofs and M_ff w_f = b_f on the free ones.  BY DEFINITION mi_project_load for the six vectors,
 * then mi_mass_solve with masked = 1, then the result into dst's six vectors, device to device -- the same bits as that host
 * route.  The best approximation of src's fields in dst's (constrained) space on the exact pairs above: orthogonal to dst's test
 * functions, never increasing the integral of |w|^2 -- where mi_state_transfer samples.
 *   Writes nothing else in dst and nothing in src.  On any error -- a point outside src's mesh (MI_EINVAL), no convergence
 *   (MI_ENOCONV_LIN; *out is still written), a refusal -- dst is unchanged.  out or NULL. */
int mi_state_project(mi_ctx *dst, mi_ctx *src, int sub, double tol, int max_it, mi_project_info *out);

/* ---- linear model: ElastoDynamics (source/linear_elasticity/linear_elasticity.cc) -------------------------- */
/* state vectors of the linear model live in the same slots as the nonlinear ones */
enum
{
  MI_L_DISPLACEMENT     = 0, /* MI_V_TOTAL_DISPLACEMENT      */
  MI_L_OLD_DISPLACEMENT = 1, /* MI_V_TOTAL_DISPLACEMENT_OLD  */
  MI_L_VELOCITY         = 2,
  MI_L_OLD_VELOCITY     = 3,
  MI_L_OLD_STRESS       = 4, /* load vector F_n (assemble_rhs :402-409) */
  MI_L_STRESS           = 6, /* MI_V_EXTERNAL_STRESS: coupling data at the interface dofs */
  MI_L_SYSTEM_RHS       = 9
};
/* assemble_system (:248-374): K, M (QGauss(p+1)) once; stepping matrix M + theta^2 dt^2 K with the zero
 * boundary values of :426-451 eliminated; consistent-load operator of :458-521; body-force vector (:358-373) */
int mi_linear_setup(mi_ctx *ctx, double theta);
/* one pass of the time loop body (:676-684): assemble_rhs (:378-454, data_consistent: 1 "Stress" face integral,
 * 0 "Force" nodal forces), solve (:525-575; Jacobi-PCG -- multigrid-PCG with "linear_precond" 1 --, absolute tolerance, warm
 * start from the previous velocity), update_displacement (:579-586) */
int mi_linear_step(mi_ctx *ctx, int data_consistent, double abs_tol, int64_t max_it, int *its, double *res);
/* energies of the linear model after mi_linear_setup (MI_EINVAL without one): 1/2 u . (K u), 1/2 v . (M v) and -u . f_body with
 * u = MI_L_DISPLACEMENT, v = MI_L_VELOCITY, through the products the current set-up runs -- the sliced-ELL product on the
 * assembled K and M, or mf_linear_q3 / mf_linear_q2 + the slot gather ("linear_operator" 1 / 2), each with the dot product fused.  Runs
 * wherever mi_linear_step runs, teams included (collective).  Overwrites the solver's work vectors, no state vector. */
int mi_linear_energy(mi_ctx *ctx, mi_energy_info *out);
/* K (0), M (1) or the constrained stepping matrix (2) as scalar CSR, for parity tests */
int mi_linear_matrix_get_csr(mi_ctx *ctx, int which, int64_t *rowptr, int32_t *col, double *val);
/* y = K x (0), M x (1) or A x (2) through the device kernels the current set-up runs, in every mode of "linear_operator"
 * (host arrays of n_dofs; undecomposed mesh).  A: constrained columns dropped, row of a constrained dof = diag(A) x.  K, M:
 * unconstrained, as assembled.  With profiling on, the product alone is timed under MI_T_SPMV.
 * 3: y = B x, one multigrid V-cycle of the current set-up ("linear_precond" 1) as the solve applies it to its residual;
 * MI_EINVAL where the set-up has no hierarchy. */
int mi_linear_apply(mi_ctx *ctx, int which, const double *x_host, double *y_host);
/* the Jacobi diagonal of the stepping matrix the PCG of mi_linear_step uses (n_dofs; undecomposed mesh) */
int mi_linear_get_diagonal(mi_ctx *ctx, double *diag_host);
/* the dim x dim node blocks of the stepping matrix in use (host array [n_nodes][dim * dim], row-major; undecomposed mesh):
 * with "linear_precond" 1 the D whose inverse the block-Jacobi smoother multiplies with, in either mode of "linear_operator",
 * under the model's constraint rule (row and column of a constrained dof zero inside the block, its diagonal entry kept).
 * On a borrowed level context (mi_linear_mg_level_context) the level's.  A matrix-free set-up with "linear_precond" 0 forms
 * the diagonal entries alone. */
int mi_linear_get_diagonal_blocks(mi_ctx *ctx, double *blocks);
/* Modal analysis: the n_modes smallest eigenpairs of  K phi = lambda M phi  on the free dofs of the linear model (phi = 0 on the
 * dofs mi_get_constrained flags), lambda = omega^2, ascending; frequency f = sqrt(lambda) / 2 pi.
 *   Needs mi_linear_setup (MI_EINVAL without one) on an undecomposed context: an emulated or RCCL team gives MI_EINVAL, "one slab
 *   only".  1 <= n_modes <= 16, n_modes + guard <= number of free dofs, tol > 0, max_it >= 1, else MI_EINVAL.  Runs in both forms of
 *   "linear_operator" and with both values of "linear_precond", 2D and 3D, degrees 1-4.
 *   Method: LOBPCG on a block of m = n_modes + max(2, n_modes / 4) vectors (the surplus are guard vectors), so 3 m <= 60.  The
 *   products K x and M x go one vector at a time through the products of the current set-up (the sliced-ELL product or
 *   mf_linear_q3 / mf_linear_q2 + the slot gather), their output zeroed on the constrained dofs.  The preconditioner is what the set-up has for
 *   the stepping matrix A = M + theta^2 dt^2 K = (theta dt)^2 (K + sigma M), sigma = 1 / (theta dt)^2: the reciprocal diagonal,
 *   or one multigrid V-cycle with "linear_precond" 1.  The images K S and M S of the search space S = [X W P] are kept, so an
 *   iteration costs 2 m products and m preconditioner applications; all 9 m^2 scalar products of an iteration are two
 *   launches of block_gram, the updates six of block_combine.  The Rayleigh-Ritz problem is solved on the host from the device's
 *   Gram matrices (mi_dense_sym_eig's method); if the Cholesky factor of S^T M S breaks down the iteration is repeated without
 *   P, and if it breaks down again X is re-orthonormalised in the M-inner product and P restarted.
 *   Start block: a fixed integer hash of (dof, column), zero on constrained dofs.  There is no random state and no atomic sum:
 *   two calls return the same bits.
 *   Stopping: converged when every wanted j has |K x_j - lambda_j M x_j|_2 <= tol max_{k < n_modes} |lambda_k| |M x_j|_2;
 *   residual[j] is that ratio, evaluated on freshly formed products of the returned pairs.  The scale max |lambda_k| keeps
 *   rigid-body modes (lambda = 0) meaningful.  Not converged within max_it iterations: MI_ENOCONV_LIN, with the best pairs,
 *   residual and its still written.
 *   modes ([n_modes][n_dofs], or NULL): M-orthonormal, exactly zero on constrained dofs, global dof order.
 *   Convergence speed depends on sigma against the wanted lambda: the preconditioner approximates (K + sigma M)^-1, which is
 *   the better the smaller sigma is beside lambda.  A context made for modal analysis takes a large time step.  The result
 *   does not depend on the time step or theta.
 *   Block storage of 9 m n_dofs doubles (+ the Gram partials) is allocated per call and freed before return.  The call
 *   overwrites the solver's work vectors, as mi_linear_energy does; it changes no state vector, matrix, hierarchy, tuning key or
 *   "count_cg_*" counter, and a following mi_linear_step returns the bits it would have returned without the call. */
int mi_linear_modes(mi_ctx *ctx, int n_modes, double tol, int max_it, double *lambda /* n_modes */,
                    double *modes /* [n_modes][n_dofs] or NULL */, double *residual /* n_modes or NULL */, int *its /* or NULL */);
/* Vibration modes of the loaded structure: the n_modes algebraically smallest eigenpairs of  K_T(u) phi = lambda rho M phi  on the
 * free dofs of the NONLINEAR model (phi = 0 on the dofs mi_get_constrained flags), lambda ascending.  K_T is the tangent
 * stiffness of the committed state u = MI_V_TOTAL_DISPLACEMENT -- the tangent as mi_assemble forms it, without its mass term
 * alpha_1 rho M, alpha_1 = 1 / (beta dt^2) -- and rho M the mass of mi_mass_apply times the density.  lambda = omega^2 while the
 * state is stable; lambda_min -> 0 announces buckling, and a negative lambda is returned as such (a buckled state).
 *   The call (1) zeroes MI_V_SOLUTION_DELTA and MI_V_NEWTON_UPDATE as mi_newton_begin_step does (after a finished step the delta is
 *   folded into u already), (2) runs the assembly of mi_assemble -- with "fine_level" 1 the point pass and the diagonal blocks,
 *   formed afresh under "mf_diag_lag" too --, (3) with "precond" 1 refreshes the multigrid hierarchy for this tangent by the route
 *   a linear solve takes, whatever "mg_refresh_every" says, and (4) iterates: the LOBPCG of mi_linear_modes with the same block
 *   size, guard vectors, hashed start block, Rayleigh-Ritz with its fall-backs, final polish and residual ratios on fresh
 *   products.  One difference: every Rayleigh-Ritz step leaves out the columns of [X W P] that depend on those before them and
 *   is solved in two passes (basis M-orthonormalised on the device by the factor of its Gram matrix, Gram matrices formed again),
 *   because with sigma = alpha_1 far above lambda the search directions run close to X; three more block_combine triples and
 *   two more block_gram launches per iteration.  The eigenvalue estimates of the hierarchy are taken from scratch in (3), so two
 *   calls return the same bits.
 *   Products: the context holds A = K_T + alpha_1 rho M in whichever form it runs (the sliced-ELL product, or mf_spmv /
 *   mf_spmv_q3 and their gathers with "fine_level" 1), output zeroed on constrained dofs -- three columns per launch through the
 *   block kernel sell_spmm where the context is eligible (see mi_spmm; "modes_block_product" 0: one column at a time, same bits); K_T x = A x -
 *   alpha_1 rho (M x) with M x from the matrix-free mass, six columns per launch group.  The preconditioner is the context's own
 *   for A: the tangent's V-cycle with "precond" 1, else the Jacobi diagonal of the assembly.
 *   Stopping: converged when every wanted j has |K_T x_j - lambda_j rho M x_j|_2 <= tol max_{k < n_modes} |lambda_k| |rho M x_j|_2;
 *   residual[j] is that ratio on freshly formed products.  FLOOR: forming K_T x as a difference leaves a rounding error of order
 *   eps alpha_1 / max_k |lambda_k| in that ratio (about 1e-11 where dt = 0.005 meets lambda of order 1..10); tol must stay above
 *   it, and a context made for this analysis takes a large time step, which also helps the preconditioner (mi_linear_modes).
 *   The method needs A positive definite, lambda_min > -alpha_1: the condition under which a Newmark step's CG works at all.
 *   Not converged within max_it iterations: MI_ENOCONV_LIN, with the best pairs, residual and its still written.
 *   modes ([n_modes][n_dofs], or NULL): rho M-orthonormal, exactly zero on constrained dofs, global dof order.
 *   Undecomposed contexts only (a team: MI_EINVAL "one slab only"); 2D and 3D, degrees 1-4, "fine_level" 0 and 1.  MI_EINVAL with
 *   nothing changed: a context whose tangent array a "linear_operator" 1 set-up has released, and the argument errors of
 *   mi_linear_modes.  A folded cell is NOT among them: it is found by the assembly itself, which reports MI_EINVAL "inverted
 *   element" as mi_assemble does.  By then MI_V_SOLUTION_DELTA and MI_V_NEWTON_UPDATE are zero and tangent, diagonal, records and
 *   MI_V_SYSTEM_RHS are what that assembly wrote (the hierarchy is untouched and marked stale); the six state vectors and
 *   MI_V_EXTERNAL_STRESS are unchanged, and the context is usable once the state is.
 *   Effects: none on the six state vectors or MI_V_EXTERNAL_STRESS, on the stored start vectors of "cg_warm_start" or on the
 *   "count_cg_*" counters.  Tangent, diagonal, point records and hierarchy are left as an assembly plus a preconditioner refresh
 *   at the committed state leave them; the solver's work vectors and MI_V_SYSTEM_RHS are overwritten.  With "precond" 0 a
 *   following mi_newmark_step returns the bits of an undisturbed run; with the V-cycle it is a run whose hierarchy was refreshed
 *   one step early (same answers to the solver's tolerance, iteration counts may differ; "count_mg_refresh" grows by one).
 *   Block storage of 10 m n_dofs doubles (+ the Gram partials), m = n_modes + max(2, n_modes / 4), is allocated per call and
 *   freed before return. */
int mi_tangent_modes(mi_ctx *ctx, int n_modes, double tol, int max_it, double *lambda /* n_modes */,
                     double *modes /* [n_modes][n_dofs] or NULL */, double *residual /* n_modes or NULL */, int *its /* or NULL */);

/* ---- explicit dynamics of the NONLINEAR model: central differences in velocity-Verlet form with a lumped mass ----------------
 * For short transients far below the structure's period: a step is one residual-only pass and one streaming kernel -- no tangent,
 * no solve, no Newton loop.  The lumped mass is m_i = rho W_i on every component of node i, W_i = sum_q N_i JxW on the assembly's
 * rule QGauss(p + 2): the row sum of the consistent mass of mi_mass_apply (positive for FE_Q of degrees 1-4).  minv_i = 1 / m_i on
 * free dofs and 0 on the dofs mi_get_constrained flags.  Given the committed u, v, a (MI_V_TOTAL_DISPLACEMENT, MI_V_VELOCITY,
 * MI_V_ACCELERATION) and the step dt:
 *     du = dt v + dt^2 / 2 a
 *     F  = -f_int(u + du) + rho b W + Neumann(u + du, MI_V_EXTERNAL_STRESS), masked: what mi_assemble_residual leaves in
 *          MI_V_SYSTEM_RHS when MI_V_ACCELERATION is zero and MI_V_SOLUTION_DELTA = du (the pass reads a zero vector of the
 *          call's own in place of the acceleration; MI_V_ACCELERATION itself is not zeroed)
 *     a' = minv F;   v <- v + dt / 2 (a + a');   u <- u + du;   a <- a'
 * The traction is held over the steps of one call.  The force pass is whichever pass the context's keys select ("fine_level" 0 / 1,
 * "point_pass_q3" 0 / 1); 2D and 3D, degrees 1-4.  Undecomposed contexts only: an emulated or RCCL team gets MI_EINVAL "one slab
 * only".  The calls touch no tangent, record, hierarchy or hierarchy flag, no "count_cg_*" counter and no stored start vector of
 * "cg_warm_start" (mi_explicit_stable_dt excepted, see there).  One timing slot moves: with mi_set_profiling on, every force pass
 * is stamped in MI_T_ASSEMBLE_RESIDUAL, as the pass of mi_assemble_residual is.  After mi_linear_setup the calls still step the
 * NONLINEAR model on the shared state vectors; they select the tangent's side of the context first, as mi_tangent_modes does.
 *   Tuning key "explicit_force_only" (1 default | 0; read back by mi_get_tuning): 1, the force passes of the two one-launch point
 * passes -- the 3D Q2 matrix-free level's (assemble_q2sf) and the 3D Q3 level's under "point_pass_q3" 1 (mf_point_pass_q3) -- run
 * instances that do not read the acceleration (a template flag: Q2 without the gather and the interpolation N a, Q3 without the
 * gather; the value pass stays there because the body force rides on it); 0, every pass reads the call's zero vector through the
 * parent's instances.  Both forms return the same bits (==, the sign of a zero aside); every other element family reads the zero
 * vector whatever the key says.  Not provided: teams, the linear model, mass scaling, an
 * element-wise step estimate, damping, releasing the tangent array of a context that only steps explicitly. */
typedef struct mi_explicit_info
{
  int32_t steps_done;     /* steps committed by the call                                                      */
  int32_t inverted_step;  /* the 1-based step whose force pass found det F <= 0, -1: none                     */
  double  dt;             /* the step of the last mi_explicit_setup                                           */
  double  kinetic_lumped; /* 1/2 sum_i m_i v_i^2 of the state the call leaves, summed in a fixed order        */
} mi_explicit_info;
/* Forms the lumped masses on the device (first call: M 1 through the mass kernels of mi_mass_apply; 3 n_dofs doubles are kept
 * with the context: masses, inverses, a zero vector) and sets the step dt > 0 of the following mi_explicit_run calls.
 * init_acceleration 1: MI_V_SOLUTION_DELTA := 0, then MI_V_ACCELERATION and MI_V_ACCELERATION_OLD := minv F(u) of the committed
 * state -- the one change to the six state vectors; MI_V_SYSTEM_RHS holds that F.  A committed state with det F <= 0: MI_EINVAL
 * "inverted element", the acceleration untouched.  init_acceleration 0: the state stays as it is (continuing an explicit run with
 * another dt, or after mi_state_restore).  May be called again; cheap apart from the optional force pass.  dt <= 0 or not finite,
 * another init_acceleration, a team: MI_EINVAL with nothing changed. */
int mi_explicit_setup(mi_ctx *ctx, double dt, int init_acceleration);
/* n_steps steps of the scheme above, enqueued on the context's stream as plain launches: per step the force pass and
 * explicit_advance (commits the step and predicts the next du), one explicit_start before and one explicit_finish after them;
 * no host synchronisation between steps, one read-back at the end.  The device takes the one decision of a step: if the pass of
 * step k reports det F <= 0, step k and all later steps of the call commit nothing (their passes still run), a device word keeps
 * k, and the call returns MI_EINVAL "inverted element ... at explicit step k" with info->steps_done = k - 1, info->inverted_step =
 * k and the six state vectors those after step k - 1 bit for bit (what a call with n_steps = k - 1 leaves).
 *   Afterwards the *_OLD vectors equal the new ones, as mi_newmark_finish_step leaves them, MI_V_SOLUTION_DELTA is 0 and
 * MI_V_SYSTEM_RHS holds the force of the last pass.  A run of n steps equals n runs of one step bit for bit, and two runs from the
 * same state return the same bytes: every sum of the update is written with its rounding, the kinetic sum goes through
 * fixed-order partials, nothing is added atomically.  n_steps = 0: no vector is written, info is filled.
 *   MI_EINVAL with nothing changed: no mi_explicit_setup yet, n_steps < 0, a NULL argument, a team, a context whose tangent array a
 * "linear_operator" 1 set-up has released.  A force pass that cannot be enqueued (no kernel, a HIP error) ends the run after the
 * steps before it: those stay committed, the *_OLD vectors and the delta are finished as after any run, info is filled with the
 * steps done, and the pass's error code is returned. */
int mi_explicit_run(mi_ctx *ctx, int n_steps, mi_explicit_info *info);
/* the lumped masses m [n_dofs] (global dof order, constrained dofs included): a test hook; forms them if no set-up has */
int mi_explicit_get_mass(mi_ctx *ctx, double *m /* n_dofs */);
/* Stability limit of the scheme at the committed state: *lambda_max = the largest Ritz value theta of krylov_steps >= 1 Lanczos
 * steps (40 is a good default; at most the number of free dofs are taken) for K_T phi = lambda M_L phi on the free dofs, in the
 * inner product of the lumped mass M_L, and *dt_crit = 2 / sqrt(theta).  theta is a LOWER bound of lambda_max, so dt_crit lies
 * above the true limit by that much: a caller multiplies it by a safety factor (the executable: 0.8).
 *   The call zeroes MI_V_SOLUTION_DELTA and MI_V_NEWTON_UPDATE and runs the assembly of mi_assemble at the committed state, as
 * mi_tangent_modes does, without the refresh of the hierarchy (which is left marked stale).  Products go through the context's own
 * operator A (assembled, or matrix-free with "fine_level" 1) minus alpha_1 rho M x from the matrix-free mass, as mi_tangent_modes
 * forms them.  The start vector is the eigensolvers' fixed hashed one and every sum has a fixed order: two calls return the same
 * bits.  No reorthogonalisation: the largest Ritz value does not need it.
 *   Effects: none on the six state vectors or MI_V_EXTERNAL_STRESS; tangent, diagonal, records and MI_V_SYSTEM_RHS are what the
 * assembly wrote; 5 n_dofs doubles are allocated for the call and freed.  Forms the lumped masses if no set-up has.  A folded
 * state: MI_EINVAL "inverted element" from the assembly.  A NULL argument, krylov_steps < 1, a team: MI_EINVAL. */
int mi_explicit_stable_dt(mi_ctx *ctx, int krylov_steps, double *lambda_max, double *dt_crit);

/* per-vector device snapshots: what `old_state_data[i] = *state_variables[i]` (adapter.h:457-460) and its
 * inverse (:481-482) become when VectorType is a handle to a device-resident vector */
typedef struct mi_snapshot mi_snapshot;
int  mi_snapshot_create(mi_ctx *ctx, mi_snapshot **out);
void mi_snapshot_destroy(mi_ctx *ctx, mi_snapshot *s);
int  mi_snapshot_store(mi_ctx *ctx, mi_snapshot *s, int which); /* snapshot := vector `which` (MI_V_*) */
int  mi_snapshot_load(mi_ctx *ctx, const mi_snapshot *s, int which); /* vector `which` := snapshot   */

/* ---- inspection hooks (tests, bench) ------------------------------------------------------ */
enum
{
  MI_V_TOTAL_DISPLACEMENT = 0,
  MI_V_TOTAL_DISPLACEMENT_OLD,
  MI_V_VELOCITY,
  MI_V_VELOCITY_OLD,
  MI_V_ACCELERATION,
  MI_V_ACCELERATION_OLD,
  MI_V_EXTERNAL_STRESS,
  MI_V_SOLUTION_DELTA,
  MI_V_NEWTON_UPDATE,
  MI_V_SYSTEM_RHS,
  MI_V_COUNT
};
int mi_vec_get(mi_ctx *ctx, int which, double *host, int64_t n);
int mi_vec_set(mi_ctx *ctx, int which, const double *host, int64_t n);
/* tangent as scalar CSR (host arrays: rowptr n_dofs+1 (int64), col nnz (int32), val nnz) */
int mi_matrix_get_csr(mi_ctx *ctx, int64_t *rowptr, int32_t *col, double *val);
int mi_spmv(mi_ctx *ctx, const double *x_host, double *y_host); /* y = K x through the device kernel */
/* y_j = K x_j for nv columns (host arrays [nv][n_dofs], 1 <= nv <= 64) on the current tangent, undecomposed contexts.  Where every
 * sliced-ELL launch of the context is an LDS-staged one (3D, assembled fp64 tangent, more than 160 slices) the columns go three at
 * a time through the block kernel sell_spmm -- the matrix read once per group; column j bit for bit what mi_spmv returns for it --,
 * else one by one through the product mi_spmv runs.  y_host is copied in first: a row nobody computes keeps the caller's value.
 * Tuning read-back "spmm_launches": launches of sell_spmm so far.  "modes_block_product" 0 makes mi_tangent_modes go column by
 * column (same bits); the key has no effect here. */
int mi_spmm(mi_ctx *ctx, int nv, const double *x_host, double *y_host);
/* the block product against nv single products on the same matrix (1 <= nv <= 20): `rounds` alternated measurements of each, device
 * events around `reps` products of the block; ms per block into ms_block / ms_single [rounds].  Undecomposed contexts */
int mi_bench_spmm(mi_ctx *ctx, int nv, int reps, int rounds, double *ms_block, double *ms_single);
/* the dim x dim diagonal block of every node of the current tangent (host array [n_nodes][dim * dim], row-major, node order of
 * the reference) under the constraint rule of the assembly (nonlinear_elasticity.cc:760-774): out of the assembled tangent or,
 * with "fine_level" 1, as formed from the point records.  One process only (single or emulated slabs). */
int mi_get_diagonal_blocks(mi_ctx *ctx, double *blocks);
/* the block-vector kernels of mi_linear_modes on host arrays (any context; blocks column-major: column j of a at a + j n):
 * c [ma][mb] = a^T b (block_gram; ma, mb <= 60) and y = s coef with coef [ks][my] row-major (block_combine; ks <= 60, my <= 20).
 * Per-workgroup partials summed in index order, no atomics: bitwise repeatable */
int mi_block_gram(mi_ctx *ctx, int64_t n, const double *a, int ma, const double *b, int mb, double *c /* [ma][mb] */);
int mi_block_combine(mi_ctx *ctx, int64_t n, const double *s, int ks, const double *coef /* [ks][my] */, int my, double *y);
/* host only, no device: A v = w B v for dense symmetric A and symmetric positive definite B, n <= 64 (Cholesky of B + cyclic
 * Jacobi; the library links no LAPACK).  w ascending, eigenvector j at V + j n, V^T B V = I.  MI_EINVAL where B is not
 * positive definite */
int mi_dense_sym_eig(int n, const double *A, const double *B, double *w, double *V);

/* ---- the multigrid hierarchy, read-only (tests) --------------------------------------------
 * What the V-cycle of "spmv_as_smoother" 2 applies: the levels as the last linear solve left them.  Level 0 is the fine
 * problem, the last level the coarsest.  Nothing here changes a level, a kernel or a tuning key. */
typedef struct
{
  int32_t degree;          /* element degree of the level                                                        */
  int32_t reps[3];         /* cells of the level's undecomposed box, in the directions of mi_mesh_desc           */
  int64_t n_dofs;          /* dofs of the undecomposed level                                                     */
  double  lmax;            /* the smoother's estimate of lambda_max(D^-1 A) incl. its safety factor; 0 on an
                              exactly solved level                                                               */
  double  interval_ratio;  /* the polynomial targets [lmax / interval_ratio, lmax]; 0 on an exactly solved level */
  int32_t smoother_degree; /* Chebyshev steps before and after the coarse correction; on the coarsest level the
                              degree of its polynomial, 0 where it is solved exactly                             */
  int32_t exact_solve;     /* 1: the coarsest level, multiplied by its dense inverse                             */
  int32_t distributed;     /* 1: the level is cut into the slabs of the team, 0: whole (replicated on a team)    */
  int32_t reserved;
} mi_mg_level_desc;
/* levels of the hierarchy; 0 without one ("precond" 0, or no hierarchy built yet) */
int mi_mg_n_levels(const mi_ctx *ctx);
/* Works on teams; the values are those of slab 0.  MI_EINVAL without a hierarchy, for a level outside it, and while the
 * hierarchy waits for its first operators (from its creation or a change of its shape -- "precond", "fine_level",
 * "mg_coarsest", "mg_dense", "mg_dist_nodes" -- until a linear solve has built them): the description would be of operators
 * that were never built.  Under "mg_lag" 1 the operators of an earlier tangent stay in use over later assemblies of a time
 * step; the view then describes those, as the V-cycle applies them. */
int mi_mg_level_describe(mi_ctx *ctx, int level, mi_mg_level_desc *out);
/* The level's own context, for the read-only entry points: mi_n_dofs, mi_n_nodes, mi_nnz, mi_get_constrained, mi_vec_get
 * (MI_V_TOTAL_DISPLACEMENT: on levels >= 1 the state the level was assembled at, u + du interpolated down; level 0 is `ctx`
 * and holds u alone there, its tangent belongs to u + du), mi_matrix_get_csr, mi_get_diagonal_blocks.  Level 0 is
 * `ctx` itself.  Undecomposed contexts only (MI_EINVAL on a team), and MI_EINVAL under the conditions of
 * mi_mg_level_describe.
 * LIFETIME: *borrowed belongs to the hierarchy.  It must not be destroyed, stepped, assembled, solved on or given to
 * mi_set_tuning / mi_vec_set, and it dies with the next rebuild of the hierarchy ("precond", "fine_level", "mg_coarsest",
 * "mg_dense", "mg_dist_nodes") and with mi_ctx_destroy(ctx). */
int mi_mg_level_context(mi_ctx *ctx, int level, mi_ctx **borrowed);
/* The linear model's own multigrid hierarchy ("linear_precond" 1), read-only, with the contracts of mi_mg_n_levels,
 * mi_mg_level_describe and mi_mg_level_context (which keep describing the tangent's hierarchy alone).  It is built by
 * mi_linear_setup and complete when that returns: 0 levels / MI_EINVAL without one.  A borrowed level context answers
 * mi_n_dofs, mi_n_nodes, mi_nnz, mi_get_constrained, mi_linear_matrix_get_csr (2: the level's stepping matrix) and
 * mi_linear_get_diagonal_blocks; level 0 is `ctx` itself.  It dies with the next mi_linear_setup and with mi_ctx_destroy(ctx). */
int mi_linear_mg_n_levels(const mi_ctx *ctx);
int mi_linear_mg_level_describe(mi_ctx *ctx, int level, mi_mg_level_desc *out);
int mi_linear_mg_level_context(mi_ctx *ctx, int level, mi_ctx **borrowed);

/* per-kernel-class device timings from HIP events on the context's stream */
enum
{
  MI_T_ASSEMBLE_CELLS = 0, /* all colours of one assembly                     */
  MI_T_ASSEMBLE_TOTAL,     /* memset + cells + faces + diag + norm            */
  MI_T_SPMV,
  MI_T_CG_VECTOR,          /* the two fused vector kernels of a CG iteration  */
  MI_T_CG_TOTAL,
  MI_T_NEWMARK,
  MI_T_STEP,               /* whole mi_newmark_step                           */
  MI_T_ASSEMBLE_DIAG,      /* matrix-free fine level ("fine_level" 1): diagonal blocks from the point records, per tangent
                              (this slot was the block-CSR -> sliced-ELL copy until round 2; no such copy exists)  */
  MI_T_ASSEMBLE_RESIDUAL,  /* all colours of one residual-only pass (mi_assemble_residual)              */
  MI_T_SPMV_PRECOND,       /* fine-level products of the multigrid preconditioner, per product                */
  MI_T_EBE_LAUNCH,         /* single launches of ebe_spmv (one colour of one element-tangent product), timed from
                              the dispatch itself on a sample of the products (every 6th)                      */
  MI_T_COUNT
};
typedef struct
{
  double  ms[MI_T_COUNT];    /* accumulated milliseconds   */
  int64_t count[MI_T_COUNT]; /* launches / calls           */
} mi_timings;
int mi_set_profiling(mi_ctx *ctx, int enable);
/* Run-time switches of a context (all its slabs).  None is needed for production use: the defaults are what bench.py and
 * the executables run, except "cg_warm_start", which both set to 2.  Unknown key or value out of range: MI_EINVAL.
 * The library reads NO environment variable (round 6): the column "env" names the hook of the EXPERIMENTS build only
 * (-DMI_EXPERIMENTS, make EXPERIMENTS=1 -> libmi_elasticity_exp.so: A/B runs of tools/), read once at context creation there.
 *
 *  key                  values (default first)     meaning                                                            env
 *  -------------------  -------------------------  -----------------------------------------------------------------  ----------------
 *  SOLVER POLICIES
 *  precond              1 | 0                      CG preconditioner: multigrid V-cycle (default from 75 k dofs) |      MI_PRECOND
 *                                                  Jacobi (default below)
 *  solver_type          0 | 1                      mi_newmark_step / mi_linear_step solve by PCG | banded Cholesky      -
 *                                                  ("Solver type = Direct", nonlinear_elasticity.cc:1192-1200)
 *  cg_warm_start        0 | 1 | 2 | 3              start vector of a solve: zero | the previous Newton update (the      MI_CG_WARM_START
 *                                                  reference, :419,472) | the same solve of the previous time step |
 *                                                  ... extrapolated over two steps; see mi_apply_newton_update
 *  cg_speculate         1 | 0                      multigrid-PCG: iterations up to (count of the same solve one step    -
 *                                                  earlier) - 2 are enqueued without polling the convergence flag, the
 *                                                  device decides; same iterates bit by bit | poll every iteration
 *  mg_lag               1 | 0                      coarse operators kept over the Newton iterations of a step | rebuilt  -
 *                                                  after every assembly
 *  mg_refresh_every     8 (1..1000)                coarse operators rebuilt at the first solve of every k-th step, or   MI_MG_REFRESH_EVERY
 *                                                  earlier when a solve needs 25 % (>= 2) more iterations than the
 *                                                  first one after a rebuild
 *  correct_face_F       0 | 1                      Neumann pull-back with F of CELL point fq (the reference's quirk,    MI_CORRECT_FACE_F
 *                                                  :825-827) | with F at the face point
 *  OPERATOR FORMS
 *  fine_level           0 | 1                      3D Q2 and Q3 (Q3: one slab): the fine level assembled (global        -
 *                                                  tangent + sell_spmv: the north-star path) | matrix-free end to end: a
 *                                                  tangent assembly writes point records, residual and the nodes'
 *                                                  diagonal blocks only; the CG's product, residual / start-vector
 *                                                  products and the smoother run on mf_spmv (Q3: mf_spmv_q3, 125 points;
 *                                                  the smoother's rule there is "smoother_quadrature_q3";
 *                                                  "smoother_quadrature", "smoother_precision" 32 and
 *                                                  "mf_slots_cell_major" have no effect there); the assembled tangent's
 *                                                  memory is released.  Same results (nonlinear_elasticity.cc:1044-1087,
 *                                                  1153-1191); excludes "solver_type" 1, "precond_storage" 32 and matrix
 *                                                  export
 *  linear_operator      0 | 1 | 2                  linear model (mi_linear_setup / mi_linear_step): K, M and the stepping  -
 *                                                  matrix assembled in the tangent's sliced-ELL layout | matrix-free on 3D
 *                                                  Q3 meshes of one slab (elsewhere: MI_EINVAL, the key stays 0): one
 *                                                  kernel, mf_linear_q3, applies (c_K K + c_M M) x on the model's own
 *                                                  4 x 4 x 4 rule (linear_elasticity.cc:61), one wave per cell, no point
 *                                                  record; the diagonal of the stepping matrix comes from mf_linear_diag_q3,
 *                                                  the body force as M (b, b, ...) | matrix-free on the kernel of the mesh's
 *                                                  element family: 3D Q2 of one slab: mf_linear_q2 on the model's own
 *                                                  3 x 3 x 3 rule, two cells per wave, no point record, the diagonal from
 *                                                  mf_linear_diag_q2, in whichever slot layout the context has; 3D Q3 of one
 *                                                  slab: exactly what 1 does; elsewhere (2D, degrees 1 and 4, teams):
 *                                                  MI_EINVAL, the key keeps its value.  Read by the next mi_linear_setup, which
 *                                                  then keeps no assembled array: the nonlinear tangent array is released
 *                                                  too, and mi_assemble, mi_newmark_step, mi_cg_solve, mi_spmv and the matrix
 *                                                  exports return MI_EINVAL until a set-up with 0.  "solver_type" 1 takes
 *                                                  the PCG route there; "fine_level" cannot change meanwhile.  Same
 *                                                  operators up to rounding.  Read-back "linear_operator": the value set;
 *                                                  "linear_operator_active": what the current linear set-up runs -- 0
 *                                                  assembled (or no set-up), 1 mf_linear_q3, 2 mf_linear_q2
 *  linear_precond       0 | 1                      linear model: the solve of mi_linear_step is the Jacobi-PCG | the PCG   -
 *                                                  preconditioned by a geometric multigrid V-cycle on a hierarchy of the
 *                                                  (constant) stepping matrix that the model owns: the shape rules of the
 *                                                  tangent's ("mg_coarsest", "mg_dense"; nu 3 / 2 over ratio 20), every level
 *                                                  >= 1 the assembled linear model of its own unperturbed mesh, level 0 the
 *                                                  context in either mode of "linear_operator" (matrix-free: the smoother
 *                                                  steps and the residual in the slot gathers, D from the block form of
 *                                                  mf_linear_diag_q3 / mf_linear_diag_q2).  Built once by the next mi_linear_setup, never refreshed;
 *                                                  independent of "precond" and of the tangent's hierarchy.  Undecomposed
 *                                                  contexts only (a team: MI_EINVAL, the key stays 0).  "solver_type" 1
 *                                                  keeps precedence where the band solver applies.  Read-back
 *                                                  "linear_precond_active": what the current linear set-up runs
 *  mf_diag_lag          0 | 1                      "fine_level" 1: diagonal blocks (smoother's D, Jacobi diagonal) at     -
 *                                                  every tangent | at the first tangent of a time step, kept over its
 *                                                  Newton iterations (what bench.py and the executable set)
 *  face_slots           1 | 0                      Neumann term: all interface cells in one launch, contributions into    -
 *                                                  slots, summed per node in entry order | eight colour launches
 *  asm_box_geometry     1 | 0                      assemble_q2sf on meshes of axis-parallel boxes: 1/h and the volume     -
 *                                                  (as mf_spmv) | the trilinear map inverted at every point
 *  mf_point_slots       1 | 0                      "fine_level" 1: the point pass (records + residual) over all cells in  -
 *                                                  one launch, residual through the product's slots | eight colour launches
 *  point_pass_q3        0 | 1                      3D Q3 matrix-free level ("fine_level" 1): an assembly forms the         MI_POINT_PASS_Q3
 *                                                  residual with the generic element kernel colour by colour and then the
 *                                                  records (mf_records_q3) | records and residual of all cells in ONE
 *                                                  sum-factorised launch (mf_point_pass_q3, the shape of mf_spmv_q3) into
 *                                                  the product's slots + residual_gather; mi_assemble_residual runs the
 *                                                  same kernel without the record stores.  Same residual up to rounding.
 *                                                  Elsewhere accepted, remembered, no effect; either order with
 *                                                  "fine_level".  Read-back "point_pass_q3_active": 1 = the next assembly
 *                                                  of this context runs that kernel, else 0
 *  smoother_operator    2 | 1 | 0                  fine-level products of the smoother on 3D Q2 slabs > 100 k nodes:    MI_EBE
 *                                                  matrix-free from the assembly's point records | stored element
 *                                                  tangents | assembled matrix
 *  cg_operator          0 | 1                      the CG's own product on the assembled matrix (north star) | in the   -
 *                                                  smoother's unassembled form (A/B)
 *  cg_r0_operator       1 | 0                      A h of a predicted start vector h ("cg_warm_start" 2 / 3) by the     -
 *                                                  matrix-free product where the point records exist | assembled
 *  precond_storage      64 | 32                    smoother multiplies with the fp64 matrices | an fp32-rounded copy    -
 *                                                  (opt-in; arithmetic, the CG's product and residual stay fp64; every
 *                                                  product of a V-cycle -- smoother steps, the cycle's residual, the
 *                                                  eigenvalue estimates -- reads the copy, D^-1 and the coarsest level's
 *                                                  inverse come from the fp64 values).  Levels built later -- "precond" 1
 *                                                  after the key, a hierarchy rebuilt by a shape key -- take the setting.
 *                                                  Read-backs, no setters: "precond_storage" = the setting of the context
 *                                                  asked (a borrowed multigrid level context answers for itself);
 *                                                  "precond_storage_levels" = how many levels of the hierarchy, level 0
 *                                                  included, multiply their cycle products with the fp32 copy (0 without
 *                                                  a hierarchy or with 64; on a team: slab 0's)
 *  mf_single_launch    1 | 0                      matrix-free product: one launch + gather | eight colour launches     MI_MF_SINGLE_LAUNCH
 *  cell_lattice         1 | 0                      mf_spmv: node ids of a cell by lattice arithmetic | from conn        MI_CELL_LATTICE
 *  element_tangents     2 | 1                      tests: keep point records / element tangents whatever the size       -
 *  DECOMPOSITION
 *  halo_overlap         1 | 0                      ghost planes exchanged on the communication stream next to the       MI_HALO_OVERLAP
 *                                                  interior rows | in line (same bits)
 *  mf_halo_overlap      1 | 0                      a slab's matrix-free product in launches over cell layers: the       -
 *                                                  layers away from the ghost planes while the halo travels | one
 *                                                  launch after the exchange (same bits)
 *  halo_skip            1 | 0                      no exchange before a product whose operand's ghost planes are        -
 *                                                  current (first post-smoothing step) | always exchange (same bits)
 *  smoother_quadrature  3 | 4                      Gauss points per direction of the multigrid smoother's fine-level       -
 *                                                  operator (3D Q2, where it multiplies matrix-free): the full-order
 *                                                  3 x 3 x 3 rule (mf_spmv27, two cells per wave, records of its own; the
 *                                                  V-cycle's residual and eigenvalue estimate use it too) | the assembly's
 *                                                  4 x 4 x 4 (nonlinear_elasticity.cc:74).  Preconditioner side only, fp64:
 *                                                  the CG's operator, residuals and the assembly always integrate with 4
 *  smoother_quadrature_q3  5 | 4                   ... on a 3D Q3 matrix-free level ("fine_level" 1): the assembly's          MI_SMOOTHER_QUADRATURE_Q3
 *                                                  5 x 5 x 5 rule (mf_spmv_q3 on the assembly's records) | the full-order
 *                                                  4 x 4 x 4 rule (mf_spmv_q3s, one wave per cell, records of its own with
 *                                                  the fold rule; the V-cycle's residual and the eigenvalue estimates use
 *                                                  it too).  Preconditioner side only: the CG's operator, residuals,
 *                                                  mi_spmv and the block-Jacobi D keep 5.  Elsewhere accepted, remembered,
 *                                                  no effect.  Read-back "smoother_quadrature_q3_active": 4 | 5 = the rule
 *                                                  of the next smoother product on such a level, 0 elsewhere
 *  smoother_precision   64 | 32                    the smoother's matrix-free fine-level products in fp64 | in fp32      -
 *                                                  arithmetic on fp32 point records (opt-in; everything else stays fp64;
 *                                                  takes effect with the next tangent assembly).  Read-back, no setter:
 *                                                  "smoother_precision_active" = 32 if the next smoother product of level 0
 *                                                  runs the float instantiation of mf_spmv (fp32 records of the current
 *                                                  tangent; one launch, box cells, lattice ids, cell-major slots), else 64
 *  cg_single_reduction  -1 | 0 | 1                multigrid-PCG with ONE all-reduce per iteration (r.z, z.Az, ||r||^2;      MI_CG_SINGLE_REDUCTION
 *                                                  Chronopoulos-Gear form): on teams of several slabs | never | always
 *  cg_speculate_margin  0 | 1..16                  expected iterations of a solve left to polled ones (0: two)          -
 *  mg_dist_nodes        -1 | n                     node count from which the first coarsened multigrid level of a team   MI_MG_DIST_NODES
 *                                                  is cut into slabs of its own (default 65,536); an existing hierarchy
 *                                                  is rebuilt
 *  mg_coarsest          4 | 1..64                  cells per direction at which the multigrid coarsening stops            MI_MG_COARSEST
 *  mg_dense             1 | 0                      exact dense solve on the coarsest level (<= 384 dofs) | polynomial     MI_MG_DENSE
 *                                                  (both keys rebuild an existing hierarchy)
 *  mg_restrict_fuse     1 | 0                      the restriction takes the coarse level's first smoother step | a     MI_MG_RESTRICT_FUSE
 *                                                  launch of its own (same bits)
 *  KERNEL A/B (timing, tests)
 *  spmv_variant         3 | 1 | 4 | 11..14         sliced-ELL LDS-DMA product | row-per-wave cross-check | mi_spmv      MI_SPMV_VARIANT
 *                                                  through the unassembled form | streaming calibration kernels
 *  sell_icol            1 | 0                      column indices generated from the rows' column boxes | read          MI_SELL_ICOL
 *  sell_unroll, spmv_grid, xcd_remap               launch shape of the sliced-ELL product (MI_SELL_SPLIT=0: never the   MI_SELL_UNROLL
 *                                                  one-workgroup-per-slice kernel on short launches).  Read-backs
 *                                                  "spmv_lds_launches" / "spmv_split_launches": how many launches of one
 *                                                  sliced-ELL product of the context (interior and boundary rows of every
 *                                                  slab, those with a slice) run sell_spmv / sell_spmv_split; no setter;
 *                                                  answered on a borrowed multigrid level context too
 *  cg_fused_dot         1 | 0                      p.q partials in the product's epilogue | separate reduction          MI_CG_FUSED_DOT
 *  small_cg             1 | 0                      matrices <= 1 MiB: whole Jacobi-PCG in one launch | three launches   MI_SMALL_CG
 *                                                  per iteration
 *  asm_variant          0 | 9 | 1,2                3D Q2 element kernel: sum factorised | node-pair form | its chunk    -
 *                                                  sizes (3-8, the A/B forms of rounds 4-5, were removed: DESIGN.md C.1)
 *  mg_fuse              1 | 0 | 2                  smoother update fused into the product on small levels | never |     MI_MG_FUSE
 *                                                  always
 *  mf_slots_cell_major  -1 | 0 | 1 | 2             result slots of the matrix-free kernels: follows smoother_quadrature     -
 *                                                  (3: cell-major, a cell's 81 results one contiguous run, the gathers read
 *                                                  through an index; 4: node-major) | forced (A/B; 2: line-major within an
 *                                                  x-row of cells, lattice meshes -- measured slower)
 *  spmv_as_smoother     0 | 1 | 2                  tests: mi_spmv / mi_bench_spmv apply the smoother's form of the operator -
 *                                                  | 2: mi_spmv applies M^-1, one V-cycle of the last solve's hierarchy
 *  mg_scale_lmax_percent 10..400                   tests: spoil the eigenvalue estimates once                           -
 *  stress_projection    0 | 1                      nodal stress sigma*: 0 the lumped projection b_i / W_i, every bit as without -
 *                                                  the key | 1 the CONSISTENT one, the L2 best approximation: the colour passes
 *                                                  leave b_k(i) = sum N_i sigma_k JxW and W_i, then M sigma*_k = b_k is solved
 *                                                  with the unit-density consistent mass of mi_mass_apply, unmasked, the ncomp
 *                                                  scalar fields packed as components of two vector columns (3D xx yy zz |
 *                                                  xy xz yz, 2D xx yy | xy 0), by mi_mass_solve's device solve to the fixed
 *                                                  tolerance 1e-13 in at most 1,000 iterations; von Mises from the solved
 *                                                  tensor, weight stays W_i.  Governs mi_stress_field, mi_stress_error,
 *                                                  mi_evaluate_stress (RECOVERED) and the VTK stress output alike (one nodal
 *                                                  array).  Not converged: MI_ENOCONV_LIN from the entry point that asked.
 *                                                  A DEFINITION for model 1: b is integrated on QGauss(p+1), M on QGauss(p+2)
 *                                                  (model 0: both on QGauss(p+2), where sigma* minimises mi_stress_error's eta
 *                                                  over all nodal fields).  On a team the setter returns MI_EINVAL and the key
 *                                                  stays 0.  Read-backs "stress_projection" and "stress_projection_its"
 *                                                  (iterations of the last solve; 0 under key 0)
 *
 * Further switches of the experiments build only (read at creation; diagnostics): MI_MG_NU, MI_MG_NU_COARSE, MI_MG_RATIO, MI_MG_KIND,
 * MI_MG_BLOCK, MI_MG_COARSEST, MI_MG_DENSE, MI_MG_FACTOR, MI_MG_SAFETY, MI_MG_POWER_ITS,
 * MI_MG_COARSE_DEGREE, MI_MG_COARSE_RATIO, MI_MG_FUSE_MAX_NODES, MI_MG_VERBOSE (multigrid parameters);
 * MI_MF_XCD (XCD-aware cell order of mf_spmv), MI_ASM_CELL_LATTICE, MI_ASM_STAMPS / MI_MF_STAMPS / MI_MF_DBG (phase stamps
 * and timing-only ablations of the two element kernels), MI_ENERGY_GENERIC (mi_energy through the generic kernel on 3D Q2 / Q3
 * too: the cross-check of tools/energy_generic_check.py), MI_STRESS_GENERIC (mi_stress_field likewise:
 * tools/stress_generic_check.py), MI_STRESS_ERROR_GENERIC (the second pass of mi_stress_error likewise:
 * tools/stress_error_generic_check.py), MI_REACTIONS_GENERIC (mi_reactions likewise: tools/reactions_time.py). */
int mi_set_tuning(mi_ctx *ctx, const char *key, int value);
/* Read back.  Counters since the last mi_reset_timings (what a solve costs in latency-bound events; counted on one slab
 * as well, where the collectives themselves are no-ops): "count_scalar_allreduce", "count_scalar_allreduce_cg" (those inside
 * the linear solves), "count_vector_allreduce", "count_halo_exchange", "count_cg_host_sync", "count_cg_iterations", "count_cg_solves", "count_mg_refresh" (rebuilds of
 * the preconditioner's coarse operators).  State: "smoother_operator_active" (2 / 1: the smoother's fine-level products
 * are matrix-free / use the stored element tangents, 0: the assembled matrix), "precond", "spmv_variant",
 * "mf_single_launch", "cell_lattice", "mg_refresh_every", "cg_speculate", "halo_skip", "cut_axis" (1 / 2 / 3: the slabs
 * are cut along x / y / z, 0: not decomposed), "cg_single_reduction_active", "mg_distributed_levels" (multigrid levels cut
 * into slabs; 0 on one slab), "spmv_lds_launches" / "spmv_split_launches" (launches of one sliced-ELL product on
 * sell_spmv / sell_spmv_split; read-only), "precond_storage", "precond_storage_levels" and "smoother_precision_active"
 * (what the fp32 opt-ins of the preconditioner do now; read-only, described with their keys above). */
int mi_get_tuning(mi_ctx *ctx, const char *key, int *value);
int mi_reset_timings(mi_ctx *ctx);
int mi_get_timings(mi_ctx *ctx, mi_timings *out);
/* isolated kernel benches on the current matrix/state: average ms per launch over reps */
int mi_bench_spmv(mi_ctx *ctx, int reps, double *ms_per_launch);
int mi_bench_assemble(mi_ctx *ctx, int reps, double *ms_per_assembly);

#ifdef __cplusplus
}
#endif
#endif /* MI_ELASTICITY_H */
