// mi_kernels.h -- kernel argument blocks and launchers shared by mi_kernels.hip and mi_ctx.cpp
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <stdlib.h>

namespace mi
{
  // Environment switches are EXPERIMENT hooks (A/B runs, diagnostics of tools/): the release library reads none -- its
  // numerics and solver path do not change with the caller's environment; every supported switch is a mi_set_tuning key.
  // -DMI_EXPERIMENTS (make EXPERIMENTS=1 -> libmi_elasticity_exp.so, what tools/profile_round.sh builds) compiles the hooks
  // and the extra kernel instantiations they select.
#ifdef MI_EXPERIMENTS
  inline const char *exp_env(const char *name) { return getenv(name); }
#else
  inline const char *exp_env(const char *) { return nullptr; }
#endif

  // Node ids of a cell WITHOUT reading the connectivity (round 4).  The mesh is a lattice: the cell at colour-sorted
  // position pos belongs to colour col (begin[col] <= pos < begin[col+1]), is the r-th cell (x fastest) of that colour's
  // sub-lattice of mx x my x mz cells, and its first node is  base + rx sx + ry sy + rz sz;  local node (i, j, k) of a
  // 3D cell then is  node0 + i + nn0 j + nn01 k.  The two divisions of r are multiplications by floor(2^42 / d) + 1
  // (exact for r < 2^22, d < 2^20: r e < 2^42 with e = M d - 2^42 <= d), so a workgroup knows its nodes after a handful
  // of scalar instructions and ONE scalar load of its colour's row (32 bytes of a 256-byte table every workgroup reads:
  // scalar-cache resident) instead of after a round trip to memory for the connectivity (conn -> values was a chain of
  // two dependent vector loads at the head of mf_spmv and assemble_q2sf).  Built and checked against conn by
  // build_cell_lattice (mi_ctx.cpp); ncol == 0: not available (the kernels then read conn).  The per-colour rows live in
  // device memory, not in the argument block: a by-value table indexed by the colour made the compiler copy the whole
  // block to scratch at the head of every wave (0.72 instead of 0.40 ms per product, measured).
  struct CellLatticeRow
  {
    int32_t  mx, mxy, base, pz; // pz: parity of the colour's cells along the last lattice direction
    uint64_t magic_mx, magic_mxy;
  };
  struct CellLattice
  {
    int32_t               ncol = 0;
    int32_t               begin[9] = {};
    int32_t               sx = 0, sy = 0, sz = 0, nn0 = 0, nn01 = 0;
    const CellLatticeRow *rows = nullptr; // [8] device
  };

  // The other direction (slot gathers): the cells of a NODE and where their contributions lie, without reading slot_base /
  // slot_src.  Cell-major slots (dst[cell][a] = cell * 27 + a) on a lattice of Q2 cells: node (i, j, k) = n = i + nn0 j + nn01 k
  // with an odd coordinate lies inside one cell along that direction (local index 1), with an even one it is the last node
  // (2) of cell h - 1 and the first (0) of cell h = i / 2, where those exist.  The colours are the parity triples of the
  // cells in ascending order of  v = px | py << 1 | pz << 2  (those that occur), so "ascending colour-sorted position" --
  // the processing order the slot tables hold -- is ascending v, and the cell of parity triple v sits at position
  //   begin[v] + rz mxy[v] + ry mx[v] + rx,   r = (cell index - parity) / 2  per direction
  // (the inverse of lattice_row_node0).  Tables by PARITY TRIPLE, in the kernel's argument block: every index is a
  // compile-time constant after unrolling, so they are scalar registers.  n -> (i, j, k) by multiplications with
  // floor(2^64 / d) + 1, upper half of the product (exact for n, d < 2^32: n e < 2^64 with e = M d - 2^64 <= d).
  // Built by build_slot_lattice and checked node by node against the tables by build_slot_tables (mi_ctx.cpp): any
  // difference leaves ncol = 0 and the gathers keep reading the tables.
  struct SlotLattice
  {
    int32_t  ncol = 0;                 // 0: not available
    int32_t  nc[3] = {};               // cells per direction
    int32_t  nn0 = 0, nn01 = 0;        // nodes per line, per plane
    uint64_t magic_nn0 = 0, magic_nn01 = 0;
    int32_t  begin[8] = {}, mx[8] = {}, mxy[8] = {}; // by parity triple; begin -1: no cell has it
  };
  __host__ __device__ inline uint32_t slot_lattice_div(const uint32_t n, const uint64_t magic)
  {
#if defined(__HIP_DEVICE_COMPILE__)
    return uint32_t(__umul64hi(uint64_t(n), magic));
#else
    return uint32_t((static_cast<unsigned __int128>(n) * magic) >> 64);
#endif
  }
  __host__ __device__ inline void slot_lattice_ijk(const SlotLattice &L, const uint32_t n, int32_t &i, int32_t &j, int32_t &k)
  {
    const uint32_t kk = slot_lattice_div(n, L.magic_nn01), rem = n - kk * uint32_t(L.nn01);
    const uint32_t jj = slot_lattice_div(rem, L.magic_nn0);
    i = int32_t(rem - jj * uint32_t(L.nn0)), j = int32_t(jj), k = int32_t(kk);
  }
  // one direction: the cell of parity P that holds node coordinate i -- its index within the colour's sub-lattice, the
  // node's local index there, whether that cell exists (mesh faces and slab ends: it does not)
  template <int P>
  __host__ __device__ inline void slot_lattice_axis(const int32_t i, const int32_t ncells, int32_t &r, int32_t &l, bool &ok)
  {
    const int32_t h = i >> 1, odd = i & 1;
    const bool    at_h = (h & 1) == P; // cell h has the parity (else cell h - 1 has)
    r  = (h - (at_h ? 0 : 1)) >> 1;
    l  = at_h ? odd : 2;
    ok = at_h ? h < ncells : (odd == 0 && h >= 1);
  }
  // slot positions (cell position * 27 + local node) of the contributions to node (i, j, k), by parity triple = in
  // processing order; -1: no contribution (never an address)
  __host__ __device__ inline void slot_lattice_slots(const SlotLattice &L, const int32_t i, const int32_t j, const int32_t k,
                                                     int32_t slot[8])
  {
    int32_t rx[2], lx[2], ry[2], ly[2], rz[2], lz[2];
    bool    okx[2], oky[2], okz[2];
    slot_lattice_axis<0>(i, L.nc[0], rx[0], lx[0], okx[0]);
    slot_lattice_axis<1>(i, L.nc[0], rx[1], lx[1], okx[1]);
    slot_lattice_axis<0>(j, L.nc[1], ry[0], ly[0], oky[0]);
    slot_lattice_axis<1>(j, L.nc[1], ry[1], ly[1], oky[1]);
    slot_lattice_axis<0>(k, L.nc[2], rz[0], lz[0], okz[0]);
    slot_lattice_axis<1>(k, L.nc[2], rz[1], lz[1], okz[1]);
#pragma unroll
    for (int v = 0; v < 8; ++v)
      {
        const int  px = v & 1, py = (v >> 1) & 1, pz = v >> 2;
        const bool ok = okx[px] && oky[py] && okz[pz] && L.begin[v] >= 0;
        const int32_t pos = L.begin[v] + rz[pz] * L.mxy[v] + ry[py] * L.mx[v] + rx[px];
        // (all ones over the position instead of a select of it: the eight positions stay straight-line code)
        slot[v] = (pos * 27 + lx[px] + 3 * ly[py] + 9 * lz[pz]) | (ok ? 0 : -1);
      }
  }
  // ... of node n as a list: the number of contributing cells, their positions in processing order (what slot_src holds in
  // [slot_base[n], slot_base[n + 1]) with cell-major slots) -- the form build_slot_tables compares with the tables
  __host__ __device__ inline int slot_lattice_list(const SlotLattice &L, const uint32_t n, int32_t list[8])
  {
    int32_t i, j, k, slot[8];
    slot_lattice_ijk(L, n, i, j, k);
    slot_lattice_slots(L, i, j, k, slot);
    int cnt = 0;
#pragma unroll
    for (int v = 0; v < 8; ++v)
      if (slot[v] >= 0)
        list[cnt++] = slot[v];
    return cnt;
  }

  // arguments of assemble_cells / neumann_faces (device pointers unless noted)
  struct AsmParams
  {
    const int32_t  *conn;   // [ncells][npc]       colour-sorted
    const double   *cverts; // [ncells][2^dim][dim]
    const uint16_t *off;    // [ncells][npc][npc]
    const int2     *rowinfo; // [nnodes] {base, gstride}: block (g, kx) of the node's row sits at base + g * gstride + kx of
                             // `vals` (mi::HostMesh::rowinfo; off[] holds g << 4 | kx); base -1: no row here (ghost
                             // node of a slab) -> nothing stored
    const uint8_t  *cmask;  // [nnodes]
    const double   *tab1d;  // N1[nq1][np1], dN1[nq1][np1], qw[nq1], qx[nq1]
    const double   *u, *du, *acc, *stress;
    double         *rhs;
    double         *vals;   // tangent, slice-interleaved block rows (mi_mesh.hpp) -- the layout the SpMV reads
    uint32_t        zero_blk, trash_blk; // two blocks behind the matrix: one that stays zero (what a first touch "reads"), one that
                                         // takes the stores of nodes without a row here (assemble_q2sf's branch-free scatter)
    double          mu, kappa, rho, alpha1;
    double          body[3];
    int64_t         cell_begin;
    int32_t         cell_count;
    int32_t         variant; // kernel variant for A/B timing
    int32_t         residual_only; // 1: residual without the tangent (Newton convergence check), same numbers
    double         *qrec;   // optional (3D Q2): the quadrature-point records the tangent is made of, [cell][MF_NREC][64] (see mf_spmv)
    float          *qrec32; // optional: the same records rounded to fp32 (opt-in fp32 smoother product)
    int32_t         axmap;    // how the lattice lies over the box (mi::AxisMap): bits 2d..2d+1 the physical coordinate lattice
                              // direction d runs along, bit 6+d set if backwards; 0x24 = aligned.  Only the Neumann term needs it
                              // (the reference pairs face and cell quadrature points by their index in PHYSICAL order)
    double         *inverted; // set to 1.0 by any quadrature point with det F <= 0 (the reference asserts det F > 0 there,
                              // nonlinear_elasticity.cc:935); sits next to the residual norm in the context's scalar block
    unsigned long long *stamps; // diagnostic (null in production): [cells of the launch][8] shader-clock stamps of one
                                // tangent wave at the phase boundaries of assemble_q2sf (mi_bench_assemble, MI_ASM_STAMPS)
    double         *ke;     // optional (3D Q2): the cell's masked element tangent, lower-triangle node-pair blocks, stored
                            // [cell][e = 0..8][block = a(a+1)/2 + b] -- the multigrid smoother's operator (see ebe_spmv)
    CellLattice     lat;    // 3D Q2: node ids by arithmetic (ncol == 0: read conn)
    double         *face_slots; // Neumann faces in one launch: [entries][npc * dim] (see neumann_faces); null: colour by colour
    double         *res_slots; // matrix-free fine level, point pass in one launch: [nslots][3] the cells' residual entries ...
    const int32_t  *slot_dst;  // ... at slot_dst[cell][27] (MfParams::dst); xcd_chunk: cells per XCD of that launch
    int32_t         xcd_chunk;
    const double   *cellbox;  // [ncells][4] = 1/hx, 1/hy, 1/hz, hx hy hz when every local cell is an axis-parallel box, else null
    int32_t         box_geometry; // assemble_q2sf: take 1/h and the volume from cellbox where present (tuning "asm_box_geometry")
    int32_t         correct_face_F; // Neumann term: 0 (default) = the reference's pull-back with the deformation gradient of CELL
                                    // quadrature point fq (nonlinear_elasticity.cc:825-827), 1 = F at the
                                    // face quadrature point itself (the physically consistent pull-back; the oracle's switch)
  };

  // product with the unassembled element tangents (see ebe_spmv in mi_kernels.hip)
  struct EbeParams
  {
    const double  *ke;
    const int32_t  *conn;  // [ncells][27] colour-sorted
    const uint32_t *first; // [ncells] bit a: first cell (in processing order) that contains its local node a -> store
    const double   *x;
    double         *y;     // complete after all colours (no zero fill needed: first touches store)
  };

  // matrix-free product from the quadrature-point records of the last tangent assembly (see mf_spmv in mi_kernels.hip)
  constexpr int MF_NREC = 11; // per point: F[9], J^(-2/3), 1/J -- the state the tangent is linearised at
  struct MfParams
  {
    const double   *qrec;    // [ncells][MF_NREC][64]
    const float    *qrec32;  // the same records rounded to fp32 (opt-in fp32 smoother product), or null
    const double   *qrec27;  // [ncells][MF_NREC][27] the records at the 27 points of the 3-point rule (smoother quadrature 3), or null
    const double   *tab27;   // N1[3][3], dN1[3][3], qw[3], qx[3] of that rule
    const double   *qrec_q3s; // 3D Q3: [ncells][MF_NREC][64] the records at the 64 points of the 4-point rule ("smoother_quadrature_q3" 4), or null
    const double   *tab_q3s;  // N1[4][4], dN1[4][4], qw[4], qx[4] of that rule
    const int32_t  *conn;    // [ncells][27] colour-sorted
    const uint32_t *first;   // as EbeParams
    const uint8_t  *cmask;   // [nnodes]
    const double   *vals;    // assembled tangent: diagonal entries of constrained dofs
    const int32_t  *diagpos; // [nnodes] position of block (node,node) in vals (in blocks), -1: no row here
    const double   *tab1d;   // N1[4][3], dN1[4][3], qw[4], qx[4] (the assembly's tables)
    const double   *cverts;  // [ncells][8][3]
    double          mu, kappa;
    const double   *cellbox; // [ncells][4] = 1/hx, 1/hy, 1/hz, hx hy hz when every cell is an axis-parallel box, else null
    const double   *x;
    double         *y;
    double          mass;    // alpha_1 rho
    int32_t         count, xcd_chunk; // set by the launcher: cells of this launch, cells per XCD (0: plain order)
    // single-launch form (null: colour-by-colour update of y): every cell stores its results in its own slots
    double         *yc;        // [nslots][3] contributions
    const int32_t  *dst;       // [ncells][27] slot of (cell, local node)
    const int32_t  *slot_base; // [nnodes+1] first slot of every node (slots of a node in processing order of its cells)
    const int32_t  *slot_src;  // cell-major slots (dst[cell][a] = cell * 27 + a: a cell's 81 results are ONE contiguous run): position
                               // of the k-th contribution of a node, k in [slot_base[n], slot_base[n+1]); null: node-major (dst = k)
    int32_t         slot_inline; // 1: dst[cell][a] = cell * 27 + a, no need to read it (0: another order of the slots behind slot_src)
    CellLattice     lat;       // node ids by arithmetic (ncol == 0: read conn)
    unsigned long long *stamps; // diagnostic (null in production): [cells][8] shader-clock stamps at the stage boundaries
    // slabs, lattice ids only: a launch over the cells of the layers [z_a, z_b) of the last lattice direction alone (the
    // layers that touch no ghost plane of x run while the halo is in flight, the others after it).  Cells are sorted by
    // colour with z slowest, so the layers' cells are ONE contiguous range of positions per colour: workgroup `local` of the
    // launch takes position sel_pos0[c] + (local - sel_begin[c]) of colour c, sel_begin[c] <= local < sel_begin[c + 1].
    // sel_n == 0: all cells, position = local.
    int32_t         sel_n, sel_begin[9], sel_pos0[8];
  };

  // what the Q3 level's point pass (mf_point_pass_q3) takes beside MfParams: the state, the mass term's constants, its outputs
  struct MfPointPass
  {
    const double *u, *du, *acc; // total displacement, solution delta, acceleration
    double        body[3], rho;
    double       *rec;          // [ncells][MF_NREC][MF_Q3_QS] the records to write; null: the residual-only pass, which touches none
    double       *inverted;     // as AsmParams::inverted
  };

  // energy diagnostics (see energy_q3 / energy_q2 / energy_cells): the state, the material, where the cells' three numbers go.
  // The two sum-factorised forms take mesh tables, 1D tables and geometry from MfParams; energy_cells from here
  struct EnergyParams
  {
    const int32_t *conn;   // [ncells][npc] colour-sorted
    const double  *cverts; // [ncells][2^dim][dim]
    const double  *tab;    // the assembly's tables (AsmParams::tab1d), as StressParams::tab
    const double  *u, *v;  // total displacement (committed state), velocity
    double         mu, kappa, rho;
    double         body[3];
    double        *cell_e;   // [ncells][3] strain, kinetic, body-force potential of every cell
    double        *inverted; // as AsmParams::inverted (a slot of its own)
    int32_t        own_node_end; // a cell whose first node is this or a later one belongs to the slab's ghost layer: zeros
  };

  // nodal stress recovery (see stress_q2 / stress_q3 / stress_cells): the state, the material, the accumulator, the colour's cells.
  // The two sum-factorised forms take mesh tables, 1D tables and geometry from MfParams; stress_cells from here
  struct StressParams
  {
    const int32_t *conn;   // [ncells][npc] colour-sorted
    const double  *cverts; // [ncells][2^dim][dim]
    const double  *tab;    // the 1D tables of the model's rule: the assembly's (AsmParams::tab1d) or the linear model's (LinAsmParams::tab)
    const double  *u;      // total displacement (the committed state)
    double         mu, kappa, lambda;
    double        *acc;      // [nnodes][8]: sum of N_i w sigma in the order xx yy zz xy xz yz, sum of N_i w, one spare; zeroed by the caller
    double        *inverted; // as AsmParams::inverted (a slot of its own)
    int64_t        cell_begin; // the cells of ONE colour: no two of them share a node
    int32_t        cell_count;
  };

  // stress error indicator (see stress_error_q2 / stress_error_q3 / stress_error_cells): the state, the recovered nodal stress,
  // the material, the metric and where the cells' numbers go.  Mesh tables, 1D tables and geometry as StressParams
  struct StressErrorParams
  {
    const int32_t *conn;   // [ncells][npc] colour-sorted
    const double  *cverts; // [ncells][2^dim][dim]
    const double  *tab;    // the 1D tables of the model's rule, as StressParams::tab
    const double  *u;      // total displacement (the committed state)
    const double  *sigma;  // [nnodes][dim (dim + 1) / 2]: the nodal field of stress_finish (xx yy zz xy xz yz; 2D xx yy xy)
    double         mu, kappa, lambda;
    double         c, inv2mu; // m(s) = (s:s - c tr(s)^2) inv2mu: c = nu / (1 + nu) in 3D, nu in 2D; inv2mu = 1 / (2 mu)
    double        *cell_e;    // [ncells][3]: eta_K^2, n_K^2, 0 (the layout launch_energy_sum adds up)
    double        *inverted;  // as StressParams::inverted
  };

  // nodal forces (see nodal_force_cells): the state, the acceleration field, the material, the accumulator, the colour's cells.
  // Mesh tables, 1D tables and geometry as StressParams
  struct ReactionParams
  {
    const int32_t *conn;   // [ncells][npc] colour-sorted
    const double  *cverts; // [ncells][2^dim][dim]
    const double  *tab;    // the 1D tables of the model's rule, as StressParams::tab
    const double  *u;      // total displacement (the committed state)
    const double  *a0, *a1; // the nodal acceleration: a0 (a1 null: MI_V_ACCELERATION) or (a0 - a1) / dt (the linear model's velocities)
    double         dt;
    double         mu, kappa, lambda, rho;
    double        *acc;      // [nnodes][8]: internal force (3), inertia force (3), sum of N_i w, one spare; zeroed by the caller
    double        *inverted; // as StressParams::inverted
    int64_t        cell_begin; // the cells of ONE colour: no two of them share a node
    int32_t        cell_count;
  };
  // resultants of the nodal forces (see reaction_sums).  A workgroup's result: REACT_NSUMS sums -- force and moment (6 each) of
  // reaction, unbalanced, inertia, body, load, then sum |internal| -- the largest unbalanced entry, the largest nodal reaction and
  // its node
  constexpr int REACT_NSUMS = 31, REACT_NOUT = 34;
  struct ReactionSumParams
  {
    const double  *forces, *terms; // [n], [4][n] of nodal_force_finish
    const double  *xyz, *u;        // node coordinates [nnodes][dim]; the displacement added to them, or null (linear model)
    const uint8_t *cmask;          // [nnodes] bit c: dof (node, c) is constrained
    int64_t        n;              // dofs
    double         about[3];
  };

  // fields at arbitrary points (see field_at_points): the points, the mesh they are looked up in, the state vectors wanted and
  // where the answers go.  All pointers are device memory
  constexpr int PE_MAX_VECTORS = 10; // MI_V_COUNT
  struct PointEvalParams
  {
    const double  *xyz;      // [npts][dim] reference configuration
    int64_t        npts;
    const double  *cverts;   // [ncells][2^dim][dim], colour-sorted cells
    const int32_t *cell_pos; // [ncells] lexicographic cell id -> colour-sorted position (the inverse of HostMesh::cell_orig)
    const double  *vecs;     // the state vectors: vector w at vecs + w * n
    int64_t        n;        // dofs
    int32_t        n_which, which[PE_MAX_VECTORS];
    int32_t        reps[3];
    double         lo[3], inv_h[3];      // the unperturbed lattice: first guess of a point's cell
    double         nodes[5], rdenom[5];  // 1D support points of the element and 1 / prod_{m != a} (x_a - x_m)
    double        *values;    // [n_which][npts][dim]
    double        *gradients; // [n_which][npts][dim][dim] = d u_c / d X_d, or null
    int64_t       *cell;      // [npts] lexicographic cell id, -1 = in no cell; or null
    double        *part;      // [field_at_points_partials(npts)] points in no cell, per workgroup
  };

  // stress at arbitrary points (see stress_at_points): pe's points, mesh and lattice (its vecs, which, values and gradients are
  // not read), what to evaluate and where the answers go
  struct StressPointParams
  {
    PointEvalParams pe;
    const double   *u;     // kind 0: the displacement [nnodes][dim]
    const double   *nodal; // kind 1: the recovered nodal stress [nnodes][ncomp] (enqueue_stress)
    int32_t         kind, model; // MI_STRESS_AT_*, MI_STRESS_*
    double          mu, kappa, lambda;
    double         *sigma;     // [npts][ncomp]
    double         *von_mises; // [npts]
    double         *inverted;  // raised by a point with det F <= 0 (kind 0, model 0)
  };

  // consistent mass (see mass_apply_cells): y += M x for nrhs columns over the cells of one colour, or the diagonal of M
  constexpr int MASS_MAX_RHS = 6;    // MI_MASS_MAX_RHS
  constexpr int MASS_CHUNK   = 1024; // entries of a column per workgroup of the column algebra
  struct MassParams
  {
    const int32_t *conn;   // [ncells][npc] colour-sorted
    const double  *cverts; // [ncells][2^dim][dim]
    const double  *tab;    // the assembly's tables (AsmParams::tab1d)
    const uint8_t *cmask;  // [nnodes] bit c: dof (node, c) is constrained
    const double  *x;      // [nrhs][n]
    double        *y;      // [nrhs][n] (diag: [n]); zeroed by the caller
    int64_t        n;      // dofs
    int32_t        nrhs, masked, diag;
    int64_t        cell_begin; // the cells of ONE colour: no two of them share a node
    int32_t        cell_count;
  };
  // the columns' scalars and flags of the mass solve, on the device (see mass_cg_scalars)
  struct MassCgState
  {
    double  bb[MASS_MAX_RHS], rz[MASS_MAX_RHS], pq[MASS_MAX_RHS], rr[MASS_MAX_RHS], beta[MASS_MAX_RHS], fresh[MASS_MAX_RHS];
    int32_t done[MASS_MAX_RHS], its[MASS_MAX_RHS];
    int32_t nactive, reserved; // columns still running: the word the host reads once per iteration
  };
  // load pass of the L2 projection (see project_load_cells): a chunk of dst's cells inside one colour and src's fields at its points
  constexpr int PROJ_FIELDS = 6, PROJ_MAX_SUB = 4, PROJ_TILE = 64;
  struct ProjectParams
  {
    const int32_t *conn;   // dst: [ncells][npc] colour-sorted
    const double  *cverts; // dst: [ncells][2^dim][dim]
    const double  *tab;    // dst: the assembly's tables (weights and points of QGauss(p + 2))
    const double  *ntab;   // [sub (p + 2)][p + 1]: dst's 1D basis at the composite rule's points
    const double  *values; // [n_which][npts][dim]: src's fields at the chunk's points (field_at_points)
    int64_t        npts;   // points of the chunk
    double        *b;      // [n_which][n]; zeroed by the caller
    double        *cell_sq; // [PROJ_FIELDS][ncells]: sum_q |w_src|^2 JxW of every cell
    int64_t        n, ncells;
    int32_t        n_which, sub;
    int64_t        chunk_begin; // the chunk's first cell (its points start there)
    int64_t        cell_begin;  // the cells of this launch
    int32_t        cell_count;
  };

  // matrix-free operator of the linear model on 3D Q3 and Q2 cells (see mf_linear_q3, mf_linear_q2): y = (c_K K + c_M M) x
  struct MfLinearOp
  {
    double  lambda, mu, rho; // Lame parameters, density
    double  c_K, c_M;        // K: 1, 0   M: 0, 1   stepping matrix: theta^2 dt^2, 1
    int32_t masked;          // 1: x is read as zero at constrained dofs (the stepping matrix: its columns are dropped)
  };

  // constant operators of the linear model (linear_elasticity.cc:248-374), one launch per colour
  struct LinAsmParams
  {
    const int32_t  *conn;    // [ncells][npc] colour-sorted
    const double   *cverts;  // [ncells][2^dim][dim]
    const uint16_t *off;     // as AsmParams::off
    const int2     *rowinfo; // as AsmParams::rowinfo
    const uint8_t  *cmask;   // [nnodes]
    const double   *tab;     // N1[nq1][np1], dN1[nq1][np1], qw[nq1], qx[nq1] of the LINEAR model's rule (nq1 = p + 1, :61)
    int32_t         np1, nq1;
    double          lambda, mu, rho, ctheta; // Lame parameters, density, theta^2 dt^2
    double          body[3];
    double         *K, *M, *A; // block values in the tangent's layout, zeroed by the caller
    double         *bodyvec;   // [ndofs] rho b integrated against the shape functions (:358-373), or null
    int64_t         cell_begin;
    int32_t         cell_count;
  };

  // row-per-wave cross-check product (tests) and the streaming calibration kernels
  struct SpmvParams
  {
    const int32_t *rowptr;  // [nnodes+1] block pattern
    const int32_t *col;
    const int2    *rowinfo; // [nnodes] as AsmParams::rowinfo
    const uint8_t *rowwx;   // [nnodes] x-width of the row's column box
    const double  *vals;
    const double  *x;
    double        *y;
    const double  *dotv;     // optional: partials of y . dotv
    double        *partials; // [grid]
    const int32_t *done;     // optional early-exit flag
    int64_t        row0, nrows;
    int64_t        nvalblocks; // number of stored blocks (timing-only stream kernels)
  };

  // sliced-ELL SpMV (see mi_kernels.hip)
  struct SellParams
  {
    const int32_t *perm; // [nslices*64]
    const int32_t *len;  // [nslices]
    const int64_t *off;  // [nslices+1]
    const int32_t *col;  // [nblk64*64]
    const int32_t *rowbox; // optional [nslices*64][2]: first column and box widths of every row; when set the kernel
                           // generates the column indices instead of reading `col` (lattice meshes: columns form a box)
    int32_t        nn0, nn1; // lattice points along x and y (column = x + nn0 * (y + nn1 * z))
    const double  *vals; // x-line-interleaved block rows (mi_mesh.hpp)
    const int32_t *wx;   // [nslices] x-width of the rows' column boxes
    const float   *vals32; // same layout, rounded to fp32: the smoother's copy (null: use vals)
    // fused Chebyshev-Jacobi epilogue (multigrid smoother; cheb_d == null: plain product).  Per owned row i:
    //   res = cheb_b - (K x); d = c1 d + c2 dinv res; cheb_xout = x + d   (x itself stays: other rows still gather it)
    // cheb_b set but cheb_d null: residual mode, y = cheb_b - K x
    const double  *cheb_b, *cheb_dinv;
    double        *cheb_d, *cheb_xout;
    double         cheb_c1, cheb_c2;
    int32_t        cheb_blk; // 1: cheb_dinv holds DxD inverse diagonal blocks per node (block-Jacobi)
    const double  *x;
    double        *y;
    const double  *dotv;
    double        *partials;
    const int32_t *done;
    int32_t        nslices;            // slices this launch works on ...
    int32_t        slice0;             // ... starting here (interior / boundary launches of a slab)
    int32_t        part0;              // first slot of `partials` this launch writes (one per workgroup)
    int32_t        own_begin, own_end; // rows (nodes) that contribute to the fused dot product
    int32_t        xcd_remap; // 1: workgroups of one XCD take a contiguous eighth of the slices (measured slower)
    int32_t        split;     // 1: small launch -- one workgroup of SELL_SPLIT_W wavefronts per slice (sell_spmv_split; the
                              // dot partials then count one per SLICE); set from the launch's slice count alone
  };

  struct CgParams
  {
    double       *x, *r, *p, *q;
    double       *s;     // single-reduction form: s = A p by recurrence (q then holds w = A z)
    const double *dinv;
    double       *part_rr, *part_rz, *part_pq;
    double       *sc;    // [8] device scalars
    int32_t      *flags; // [2] done, iterations
    int64_t       n;
    int32_t       npart, npart_pq;
    const double *z;      // preconditioned residual (general preconditioner); null -> Jacobi fused in the kernels
    double       *hist;   // optional [2*it] alpha, [2*it+1] beta of every iteration (Lanczos eigenvalue estimates)
    const double *totals; // distributed: all-reduced [rr, rz, pq, bb]; null -> consumers reduce the partials
  };

  struct NewmarkParams
  {
    double *u, *u_old, *v, *v_old, *a, *a_old;
    const double *du;
    double  alpha1, alpha2, alpha3, alpha4, alpha5, alpha6;
    int64_t n;
  };

  // explicit central differences (explicit_start, explicit_advance): the state and the force of one slab, the inverted word
  // of the force pass and the word that keeps the first folded step of a run (0: none), both doubles on the device
  struct ExplicitParams
  {
    double       *u, *v, *a, *du;
    const double *F, *minv, *inverted;
    double       *stop;
    double        dt;
    int64_t       n;
    int           step; // 1-based step of the run (explicit_advance)
  };

  // index-space transfer between two lattices (see lattice_interp / lattice_restrict)
  struct LatticeParams
  {
    int64_t        n_tgt;    // nodes of the target (interp) or coarse (restrict) lattice
    int32_t        nt[3];    // its extents
    int32_t        ns[3];    // extents of the source (interp) / fine (restrict) lattice
    const int32_t *i0[3];    // interp: source index per target index
    const double  *w[3];     //         weight of i0+1
    const int32_t *rstart[3]; // restrict: per coarse index, range into ri/rw
    const int32_t *ri[3];
    const double  *rw[3];
    int32_t        rmax;      // restrict: longest list of any coarse index in any direction (<= 4: the unrolled kernel)
  };

  struct LinearParams
  {
    const double *load, *body;
    double       *f_old, *v, *d, *v_old, *d_old, *rhs, *w;
    double        theta, dt;
    int64_t       n;
  };

  void launch_linear_rhs_prepare(const LinearParams &p, hipStream_t s);
  void launch_linear_rhs_finish(int dim, const LinearParams &p, const double *mv, const double *kw,
                                const uint8_t *cmask, hipStream_t s);
  void launch_linear_update_displacement(const LinearParams &p, hipStream_t s);
  int  launch_assemble_cells(int dim, int degree, const AsmParams &p, hipStream_t s);
  int  launch_neumann_faces(int dim, int degree, const AsmParams &p, const int32_t *faces, int face_begin,
                            int face_count, hipStream_t s);
  void launch_neumann_gather(int dim, const double *slots, const int32_t *node_ids, const int32_t *start, const int32_t *src,
                             const uint8_t *cmask, double *rhs, int nnodes_if, hipStream_t s);
  void launch_spmv(int dim, const SpmvParams &p, int grid, hipStream_t s, int variant, int maxrow);
  void launch_sell_spmv(int dim, const SellParams &p, int grid, hipStream_t s, int unroll);
  // columns per launch of the block product sell_spmm: 3 columns take 249 VGPRs at the occupancy of sell_spmv (2 waves per SIMD,
  // set by the 69 KB of staging buffers); 4 spill into 44 AGPRs and halve it (profiles/tangent_modes/resources.tsv)
  constexpr int SELL_SPMM_NV = 3;
  int  launch_sell_spmm(const SellParams &p, int nv, int64_t ldx, int64_t ldy, int grid, hipStream_t s, int unroll);
  void set_next_sell_launch_events(hipEvent_t start, hipEvent_t stop); // profiling: bracket exactly the next launch
  // ev_start / ev_stop (optional): bracket exactly this launch (dispatch-level events, profiling)
  void launch_ebe_spmv(const EbeParams &p, int64_t cell_begin, int32_t cell_count, hipStream_t s,
                       hipEvent_t ev_start = nullptr, hipEvent_t ev_stop = nullptr);
  // (f32: the fp32 form -- production shape with p.qrec32 only, otherwise the fp64 kernel runs)
  void launch_mf_spmv(const MfParams &p, int64_t cell_begin, int32_t cell_count, hipStream_t s,
                      hipEvent_t ev_start = nullptr, hipEvent_t ev_stop = nullptr);
  // smoother quadrature 3 (see mf_spmv27): the product with two cells per wave from the 27-point records, and the kernel that
  // writes those records from u + du
  void launch_mf_spmv27(const MfParams &p, int32_t cell_count, hipStream_t s, hipEvent_t ev_start = nullptr, hipEvent_t ev_stop = nullptr);
  void launch_mf_records27(const MfParams &p, const double *u, const double *du, double *rec27, int32_t cell_count, hipStream_t s);
  // (sl with ncol > 0, all four gathers: the lattice source -- slot positions by arithmetic, see SlotLattice)
  void launch_mf_gather(const MfParams &p, int64_t ndofs, hipStream_t s, const SlotLattice *sl = nullptr);
  // ... with the partials of dotv . y over the owned dofs (fixed grid): the CG's product on the matrix-free fine level
  void launch_mf_gather_dot(const MfParams &p, int64_t ndofs, const double *dotv, double *partials, int grid, int64_t own0,
                            int64_t own_n, hipStream_t s, const SlotLattice *sl = nullptr);
  // matrix-free fine level (round 6): the nodes' diagonal blocks from the point records -- every cell into its own slots
  // [nslots][6] (MfParams::dst), then summed per node under the assembled matrix's constraint rule (see mf_diag)
  void launch_mf_diag(const MfParams &p, double *slots6, int32_t cell_count, hipStream_t s);
  // matrix-free fine level of 3D Q3 meshes (see mf_spmv_q3): records [ncells][MF_NREC][MF_Q3_QS] at the 125 points of the
  // assembly's rule from u + du, the product into the cells' slots [nslots][3] (64 per cell), the diagonal blocks into
  // [nslots][6].  One workgroup per cell; the records' pointer is MfParams::qrec, the 1D tables MfParams::tab1d (Q3, 5 points)
  constexpr int MF_Q3_QS = 128; // points per record field (125 used)
  void launch_mf_records_q3(const MfParams &p, const double *u, const double *du, double *rec, int32_t cell_count, hipStream_t s);
  void launch_mf_spmv_q3(const MfParams &p, int32_t cell_count, hipStream_t s, hipEvent_t ev_start = nullptr, hipEvent_t ev_stop = nullptr);
  void launch_mf_diag_q3(const MfParams &p, double *slots6, int32_t cell_count, hipStream_t s);
  // ... the level's point pass in one launch ("point_pass_q3" 1; see mf_point_pass_q3): the residual of every cell into its slots
  // (MfParams::yc / dst / slot_inline, the product's), from u + du and the acceleration; with pp.rec set, the records of
  // launch_mf_records_q3 into it as well (null: the residual-only pass).  launch_residual_gather then sums the slots into system_rhs
  void launch_mf_point_pass_q3(const MfParams &p, const MfPointPass &pp, int32_t cell_count, hipStream_t s, bool force_only = false);
  // energy diagnostics: every cell's strain energy, kinetic energy and body-force potential into e.cell_e, by the kernel of
  // (dim, degree) -- energy_q3, energy_q2 (p.conn, p.tab1d, p.cverts / p.cellbox) or energy_cells; generic: energy_cells on
  // 3D Q2 / Q3 too (cross-check).  -1: no kernel for the element.  launch_energy_sum: the cells' numbers in a fixed order into
  // out[3]; scratch holds 3 doubles per 1024 cells
  int  launch_energy(int dim, int degree, const MfParams &p, const EnergyParams &e, int32_t cell_count, bool generic, hipStream_t s);
  void launch_energy_sum(const double *cell_e, int64_t ncells, double *scratch, double *out, hipStream_t s);
  // nodal stress recovery: the cells [sp.cell_begin, + sp.cell_count) of one colour add their seven numbers per node to sp.acc,
  // by the kernel of (dim, degree, model) -- stress_q3, stress_q2 (model 0; p.conn, p.tab1d, p.cverts / p.cellbox) or
  // stress_cells; generic: stress_cells on 3D Q2 / Q3 too (cross-check).  -1: no kernel for the element.  launch_stress_finish:
  // sigma[nnodes][dim (dim + 1) / 2] = acc / W, von_mises[nnodes] of that tensor, weight[nnodes] = W
  int  launch_stress(int dim, int degree, int model, const MfParams &p, const StressParams &sp, bool generic, hipStream_t s);
  void launch_stress_finish(int dim, const double *acc, int64_t nnodes, double *sigma, double *von_mises, double *weight, hipStream_t s);
  // the consistent projection's columns: b [2][nnodes][dim] := the accumulator's sums as components of two vector columns
  // (stress_pack); sigma, von_mises and weight from the solved columns x and the accumulator's W (stress_unpack)
  void launch_stress_pack(int dim, const double *acc, int64_t nnodes, double *b, hipStream_t s);
  void launch_stress_unpack(int dim, const double *x, const double *acc, int64_t nnodes, double *sigma, double *von_mises, double *weight,
                            hipStream_t s);
  // mi_reactions.  launch_nodal_force: one colour of cells into rp.acc by nodal_force_cells (every element, both models); -1: no
  // kernel for the element.  launch_nodal_force_gather: the face slots of neumann_faces into `load` on every dof of the interface
  // nodes.  launch_nodal_force_finish: terms [4][n] and forces [n] from the accumulator and the load (rho_body: rho b, or zeros).
  // launch_reaction_sums: the resultants into out[REACT_NOUT], chunks of 1,024 nodes into scratch [(nnodes / 1024 + 1)][REACT_NOUT]
  // first
  int  launch_nodal_force(int dim, int degree, int model, const MfParams &p, const ReactionParams &rp, bool generic, hipStream_t s);
  void launch_nodal_force_gather(int dim, const double *slots, const int32_t *node_ids, const int32_t *start, const int32_t *src,
                                 double *load, int nnodes_if, hipStream_t s);
  void launch_nodal_force_finish(int dim, const double *acc, const double *load, int64_t nnodes, const double rho_body[3], double *terms,
                                 double *forces, hipStream_t s);
  void launch_reaction_sums(int dim, const ReactionSumParams &p, int64_t nnodes, double *scratch, double *out, hipStream_t s);
  // stress error indicator: all cells in one launch store their two sums into ep.cell_e, by the kernel of (dim, degree, model)
  // -- stress_error_q3, stress_error_q2 (model 0; p.conn, p.tab1d, p.cverts / p.cellbox) or stress_error_cells; generic:
  // stress_error_cells on 3D Q2 / Q3 too (cross-check).  -1: no kernel for the element.  launch_stress_error_finish:
  // eta_cell[cell_orig[i]] = sqrt(cell_e[i][0]), norm_cell likewise; max_out[0] the largest eta_K, max_out[1] the smallest
  // lexicographic id that has it (as a double); scratch holds 2 doubles per 1024 cells (launch_energy_sum's, once that is through)
  int  launch_stress_error(int dim, int degree, int model, const MfParams &p, const StressErrorParams &ep, int32_t cell_count, bool generic,
                           hipStream_t s);
  void launch_stress_error_finish(const double *cell_e, const int32_t *cell_orig, int64_t ncells, double *eta_cell, double *norm_cell,
                                  double *scratch, double *max_out, hipStream_t s);
  // fields at points: one thread per point of p.xyz, field_at_points<dim, degree, box> (box: every cell an axis-parallel box, xi
  // in closed form; else Newton on the Q1 map); then *n_outside = sum of p.part (finish_sum).  -1: no kernel for the element
  int64_t field_at_points_partials(int64_t npts);
  int     launch_field_at_points(int dim, int degree, bool box, const PointEvalParams &p, double *n_outside, hipStream_t s);
  // stress at points: stress_at_points<dim, degree, box> over p.pe's points with field_at_points' location, then *n_outside as
  // above (p.pe.part holds field_at_points_partials(npts) doubles).  launch_sym_eig_batch: principal values [n][dim], descending,
  // and unit eigenvectors [n][dim][dim] (or null) of n tensors [n][ncomp], sym_eig_batch<dim>.  -1: no kernel / too many for one launch
  int launch_stress_at_points(int dim, int degree, bool box, const StressPointParams &p, double *n_outside, hipStream_t s);
  int launch_sym_eig_batch(int dim, int64_t n, const double *sigma, double *principal, double *directions, hipStream_t s);
  // consistent mass and L2 projection.  launch_mass_apply: the cells of one colour by the kernel of (dim, degree) -- mass_apply_q3,
  // mass_apply_q2 (p.conn, p.tab1d, p.cverts / p.cellbox) or mass_apply_cells; generic: mass_apply_cells on 3D Q2 / Q3 too
  // (cross-check); the diagonal is always mass_apply_cells' (-1: no kernel for the element).  Column algebra: mass_chunks(n) workgroups per column; part arrays hold [nrhs][mass_chunks(n)] doubles.
  // launch_mass_col_dots: out[j] = a_j . b_j.  The solve's two fused updates and its scalars: see the kernels
  int  launch_mass_apply(int dim, int degree, const MfParams &p, const MassParams &mp, bool generic, hipStream_t s);
  int  mass_chunks(int64_t n);
  void launch_mass_col_dots(const double *a, const double *b, int64_t n, int nrhs, double *part, double *out, hipStream_t s);
  void launch_mass_cg_update_xr(bool first, double *x, double *r, const double *p, const double *q, const double *dinv, int64_t n,
                                int nrhs, const MassCgState *st, double *part_rr, double *part_rz, hipStream_t s);
  void launch_mass_cg_scalars(const double *part_rr, const double *part_rz, int64_t n, int nrhs, int it, double tol, MassCgState *st,
                              hipStream_t s);
  void launch_mass_cg_update_p(bool first, double *p, const double *r, const double *dinv, int64_t n, int nrhs, const MassCgState *st,
                               hipStream_t s);
  void launch_mass_diag_invert(int dim, double *d, const uint8_t *cmask, int masked, int64_t n, hipStream_t s);
  void launch_mass_fresh_residual(int dim, const double *b, const double *q, const uint8_t *cmask, int masked, int64_t n, int nrhs,
                                  double *r, hipStream_t s);
  // load pass: the points of a chunk of cells (qx: the nq1 Gauss points on [0, 1]), the chunk's cells of one colour into b and
  // cell_sq (-1: no kernel, or sub / n_which out of range), the fields' sums over the cells
  void launch_project_points(int dim, const double *cverts, const double *qx, int64_t cell_begin, int64_t npts, int nq1, int sub,
                             double *xyz, hipStream_t s);
  int  launch_project_load(int dim, int degree, const ProjectParams &pp, hipStream_t s);
  void launch_project_sq_sum(const double *cell_sq, int ncells, double *out, hipStream_t s);
  // ... the multigrid smoother's operator on the element's full-order rule, 4 x 4 x 4 points (see mf_spmv_q3s): records
  // [ncells][MF_NREC][64] of its own (MfParams::qrec_q3s, written by mf_records_q3s from u + du with the fold rule of
  // mf_records27), the rule's 1D tables MfParams::tab_q3s; one wave per cell, the results into the same cell-major slots
  void launch_mf_records_q3s(const MfParams &p, const double *u, const double *du, double *rec, int32_t cell_count, hipStream_t s);
  void launch_mf_spmv_q3s(const MfParams &p, int32_t cell_count, hipStream_t s, hipEvent_t ev_start = nullptr, hipEvent_t ev_stop = nullptr);
  // linear model, "linear_operator" 1 (3D Q3; see mf_linear_q3): the product (c_K K + c_M M) x into the cells' slots (MfParams::yc;
  // the rule's 1D tables MfParams::tab_q3s), and the diagonal of that operator: every cell into the same slots, then summed per
  // node into the diagonal entries of blk[nnodes][9] and inverted into dinv[ndofs]
  void launch_mf_linear_q3(const MfParams &p, const MfLinearOp &op, int32_t cell_count, hipStream_t s, hipEvent_t ev_start = nullptr,
                           hipEvent_t ev_stop = nullptr);
  void launch_mf_linear_diag_q3(const MfParams &p, const MfLinearOp &op, int32_t cell_count, double *blk, double *dinv, int64_t ndofs,
                                hipStream_t s);
  // "linear_precond" 1: the nodes' whole 3 x 3 blocks of that operator, every cell's symmetric halves into slots6 [ncells * 64][6]
  // (slot = the product's); launch_mf_diag_gather sums them, applies the constraint rule and inverts
  void launch_mf_linear_diag_blk_q3(const MfParams &p, const MfLinearOp &op, int32_t cell_count, double *slots6, hipStream_t s);
  // linear model, "linear_operator" 2 on 3D Q2 (see mf_linear_q2): the same three on the 3 x 3 x 3 rule, two cells per wave as
  // mf_spmv27 (the rule's 1D tables MfParams::tab27; x masked by MfParams::cmask whatever op.masked says; any slot layout;
  // slots6 [ncells * 27][6])
  void launch_mf_linear_q2(const MfParams &p, const MfLinearOp &op, int32_t cell_count, hipStream_t s, hipEvent_t ev_start = nullptr,
                           hipEvent_t ev_stop = nullptr);
  void launch_mf_linear_diag_q2(const MfParams &p, const MfLinearOp &op, int32_t cell_count, double *blk, double *dinv, int64_t ndofs,
                                hipStream_t s);
  void launch_mf_linear_diag_blk_q2(const MfParams &p, const MfLinearOp &op, int32_t cell_count, double *slots6, hipStream_t s);
  // the matrix-free fine level's point pass over ALL cells in one launch (assemble_q2sf<true> with the residual into slots:
  // AsmParams::res_slots / slot_dst; cell_begin = 0, cell_count = all) and the sum of the slots into system_rhs
  void launch_point_pass_slots(const AsmParams &p, hipStream_t s, bool force_only = false); // force_only: the acceleration is zero and not read
  void launch_residual_gather(const double *slots3, const int32_t *slot_base, const int32_t *slot_src, const uint8_t *cmask, double *rhs,
                              int64_t ndofs, hipStream_t s);
  void launch_mf_diag_gather(const double *slots6, const int32_t *slot_base, const int32_t *slot_src, const uint8_t *cmask,
                             const int32_t *diagpos, double *blk, double *dinv, double *dinv_blk, double *sym6, int64_t nnodes, hipStream_t s);
  // gather fused with the smoother's three-term Chebyshev step (xnext = x'' on the owned nodes), or with the residual
  // (yres = b - K x on the owned nodes); tiles: the lattice source in node tiles (the node range is whole planes)
  void launch_mf_gather_cheb3(const MfParams &p, const double *b, const double *dinv6, const double *xprev, const double *xcur,
                              double *xnext, double c1, double c2, int64_t node0, int64_t nnodes, hipStream_t s,
                              const SlotLattice *sl = nullptr, bool tiles = false);
  void launch_mf_gather_residual(const MfParams &p, const double *b, double *yres, int64_t node0, int64_t nnodes, hipStream_t s,
                                 const SlotLattice *sl = nullptr, bool tiles = false);
  // coarsest multigrid level: dense inverse of the level's sliced-ELL matrix (n <= 96, -1 otherwise) and its application
  int  launch_dense_inverse_from_sell(int dim, const SellParams &p, int n, double *out, hipStream_t s);
  void launch_dense_apply(const double *inv, const double *b, double *x, int n, hipStream_t s);
  // banded Cholesky of a small tangent (direct solver): see band_cholesky_solve in mi_kernels.hip
  constexpr int BAND_NB = 16, BAND_MAXH = 512; // block-column width; the half bandwidth (in dofs) stays below BAND_MAXH
  void launch_band_extract(int dim, const SellParams &p, const int32_t *bperm, double *band, int hbw, hipStream_t s);
  int  launch_band_cholesky_solve(int dim, double *band, int n, int hbw, const int32_t *bperm, int nnodes, const double *b,
                                  double *x, double *work, int32_t *flag, bool factor, bool solve, hipStream_t s); // -1: band too wide
  constexpr int SELL_SPLIT_MAX_SLICES = 160; // launches up to this many slices take the k-split kernel (sell_spmv_split)
  constexpr int SELL_WPB = 3;   // wavefronts (= slices in flight) per workgroup of sell_spmv: launch grids and dot partials count in these
  constexpr int EBE_NBLK = 378; // 27 * 28 / 2 node-pair blocks of a 3D Q2 cell
  void launch_vals_to_f32(const double *vals, float *vals32, int64_t n, hipStream_t s); // the smoother's fp32-rounded copy (opt-in)
  void launch_sell_build_cols(const SellParams &p, const int32_t *rowptr, const int32_t *bsr_col, int32_t *sell_col,
                              hipStream_t s);
  void launch_dot_partials(const double *a, const double *b, int64_t n, double *part, int grid, hipStream_t s);
  void launch_finish_sum(const double *part, int n, double *out, hipStream_t s); // out[0] = sum of part[0..n)
  void launch_cheb4_start(double *x, double *d, double *r, const double *b, const double *q, const double *dinv,
                          double s0, int64_t n, hipStream_t s);
  void launch_cheb4_step(double *x, double *d, double *r, const double *q, const double *dinv, double beta, double ca,
                         double cb, int64_t n, hipStream_t s);
  void launch_extract_dinv_blk(int dim, const double *vals, const int32_t *diagpos, double *dinv, double *sym6, int64_t nnodes,
                               hipStream_t s);
  void launch_gather_diag_blocks(int dim, const double *vals, const int32_t *diagpos, double *out, int64_t nnodes, hipStream_t s);
  void launch_blk_apply(int dim, double *out, const double *a, const double *dinv, int64_t nnodes, hipStream_t s);
  void launch_cheb_step_blk(int dim, double *x, double *d, const double *b, const double *q, const double *dinv,
                            double c1, double c2, int64_t node0, int64_t nnodes, hipStream_t s);
  void launch_cheb_step(double *x, double *d, const double *b, const double *q, const double *dinv, double c1, double c2,
                        int64_t n, hipStream_t s);
  void launch_vec_scale_mul(double *dst, const double *a, const double *b, double s, int64_t n, hipStream_t st);
  void launch_vec_residual(double *res, const double *b, const double *q, int64_t n, hipStream_t s);
  void launch_vec_lincomb2(double *x, double a, const double *h1, double b, const double *h2, int64_t n, hipStream_t s);
  void launch_scale_start(double *x, double *q, const double *sc, int64_t n, hipStream_t s);
  void launch_tangent_images(int dim, double *ks, const double *mx, double *ms, const uint8_t *cmask, double shift, double rho, int64_t n,
                             int cols, hipStream_t s);
  void launch_copy_owned(double *y, const double *x, int64_t n, int64_t own0, int64_t own_n, hipStream_t s);
  void launch_lattice_interp(int dim, bool add, const LatticeParams &p, double *tgt, const double *src,
                             const uint8_t *cmask_tgt, hipStream_t s);
  bool launch_lattice_restrict_first_step(int dim, const LatticeParams &p, double *coarse, const double *fine,
                                          const uint8_t *cmask_coarse, double *x, double *d, const double *dinv_blk, double c2,
                                          int64_t node0, int64_t nnodes, hipStream_t s);
  void launch_lattice_restrict(int dim, const LatticeParams &p, double *coarse, const double *fine,
                               const uint8_t *cmask_coarse, hipStream_t s);
  void launch_cg_update_p(const CgParams &c, int it, int grid, hipStream_t s);
  void launch_cg_update_xr(const CgParams &c, int it, int grid, hipStream_t s);
  void launch_cg_update_single(const CgParams &c, int it, int grid, hipStream_t s);
  void launch_cg_init_residual(const CgParams &c, const double *b, double *part_bb, int grid, hipStream_t s);
  void launch_cg_set_tolerance(const CgParams &c, const double *part_bb, double rel_tol, hipStream_t s);
  void launch_cg_final_check(const CgParams &c, int it, hipStream_t s);
  // whole Jacobi-PCG in one single-workgroup launch (small problems, one slab)
  void launch_cg_small(int dim, const SellParams &p, const CgParams &c, const double *b, double rel_tol, int max_it,
                       hipStream_t s);
  void launch_assemble_linear(int dim, const LinAsmParams &p, hipStream_t s);
  void launch_extract_dinv(int dim, const double *vals, const int32_t *diagpos, double *dinv, int64_t nnodes,
                           hipStream_t s);
  void launch_masked_norm(int dim, const double *v, const uint8_t *cmask, int64_t n, double *part, int grid,
                          double *out, hipStream_t s);
  void launch_reduce_to_totals(const double *pa, int na, double *oa, const double *pb, int nb, double *ob,
                               const int32_t *done, hipStream_t s);
  void launch_team_sum(double *const *bufs, int nranks, int off, int cnt, hipStream_t s);
  void launch_gather_to_slots(int dim, const double *v, const int32_t *nodes, const int32_t *slots, int n, double *out,
                              hipStream_t s);
  void launch_zero_constrained(int dim, double *x, const uint8_t *cmask, int64_t n, hipStream_t s);
  void launch_newmark_acceleration(const NewmarkParams &p, hipStream_t s);
  void launch_newmark_finish(const NewmarkParams &p, hipStream_t s);
  void launch_vec_add(double *y, const double *x, int64_t n, hipStream_t s);
  // explicit central differences: lumped masses from w = M 1; the first du of a run; one committed step + the next du; the sum of
  // m v^2 into *out through `grid` fixed-order partials (commit: *_OLD := new, du := 0 as well); the Lanczos update
  // y := minv y - alpha q - beta qprev (qprev may be null)
  void launch_explicit_masses(int dim, const double *w, const uint8_t *cmask, double rho, double *mass, double *minv, int64_t n, hipStream_t s);
  void launch_explicit_start(const ExplicitParams &p, hipStream_t s);
  void launch_explicit_advance(const ExplicitParams &p, hipStream_t s);
  void launch_explicit_finish(bool commit, const NewmarkParams &p, const double *mass, double *du, double *part, int grid, double *out,
                              hipStream_t s);
  void launch_weighted_sq(const double *mass, const double *x, int64_t n, double *part, int grid, double *out, hipStream_t s); // *out = sum m x^2
  void launch_lanczos_update(double *y, const double *minv, const double *q, const double *qprev, double alpha, double beta, int64_t n,
                             hipStream_t s);
  void launch_gather_nodes(int dim, const double *v, const int32_t *nodes, int n, double *out, hipStream_t s);
  void launch_scatter_nodes(int dim, double *v, const int32_t *nodes, int n, const double *in, hipStream_t s);
  // ---- block-vector algebra of the eigensolver (mi_linear_modes): column-major blocks, column j at base + j * ld
  constexpr int     BLOCK_TILE     = 8;    // block_gram: a workgroup's tile of C, kept in the threads' registers
  constexpr int64_t BLOCK_CHUNK    = 8192; // rows per workgroup of block_gram and block_residual (= rows per partial)
  constexpr int     BLOCK_MAX_COLS = 60, BLOCK_MAX_OUT = 20; // widest block; widest output of block_combine
  inline int64_t    block_chunks(int64_t n) { return (n + BLOCK_CHUNK - 1) / BLOCK_CHUNK; }
  struct BlockLambda
  {
    double v[BLOCK_MAX_OUT];
  };
  // c [ma][mb] = a^T b, ma, mb <= BLOCK_MAX_COLS; part: block_chunks(n) * ma * mb doubles.  The grid depends on n, ma, mb alone and
  // the partials are summed in chunk order: bitwise repeatable
  void launch_block_gram(const double *a, int ma, int64_t lda, const double *b, int mb, int64_t ldb, int64_t n, double *part,
                         double *c, hipStream_t s);
  // y = S coef; coef [ks][my] on the device, ks <= BLOCK_MAX_COLS, my <= BLOCK_MAX_OUT.  y may be columns of S (row-wise in place)
  void launch_block_combine(const double *S, int ks, int64_t lds, const double *coef, int my, double *y, int64_t ldy, int64_t n,
                            hipStream_t s);
  // r_j = kx_j - lam_j mx_j masked, j < m <= BLOCK_MAX_OUT; out [2][m] = |r_j|^2, |mx_j|^2; part: 2 * m * block_chunks(n) doubles
  void launch_block_residual(int dim, const double *kx, const double *mx, int64_t ld, const BlockLambda &lam, int m,
                             const uint8_t *cmask, int64_t n, double *r, int64_t ldr, double *part, double *out, hipStream_t s);
  void launch_block_hash_init(int dim, double *x, int64_t ld, int m, const uint8_t *cmask, int64_t n, hipStream_t s);
} // namespace mi
