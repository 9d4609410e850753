// mi_linear.cpp -- the linear elastodynamics model (ElastoDynamics, source/linear_elasticity/linear_elasticity.cc)
// on the device context.
//
// Stiffness K, mass M and the stepping matrix are constant: they are assembled ONCE, on the device
// (assemble_linear_cells, colour by colour like the tangent; linear_elasticity.cc:248-374) straight into the device
// layout of the tangent (x-line-interleaved block rows, mi_mesh.hpp); only the consistent-load operator of the interface
// (interface-sized) is put together on the host.  The per-step path (assemble_rhs :378-454, solve :525-575, update_displacement :579-586) runs on the
// device: fused vector kernels, 2 SpMVs (M v - K (theta(1-theta)dt^2 v + dt d)) and the warm-started PCG.
//
// Tuning "linear_operator" 1 (3D Q3, one slab): nothing is assembled.  K, M and the stepping matrix are one kernel
// (mf_linear_q3: (c_K K + c_M M) x on the model's own 4 x 4 x 4 rule, one wave per cell) + the slot gathers; the set-up forms
// the diagonal of the stepping matrix (mf_linear_diag_q3) and the body-force vector as M (b, b, ...), and releases the
// nonlinear tangent array.  The per-step path is the same; the solve is the PCG whatever "solver_type" says.
// "linear_operator" 2: the same on the kernel of the mesh's element family -- 3D Q2: mf_linear_q2 on the 3 x 3 x 3 rule, two
// cells per wave, and mf_linear_diag_q2; 3D Q3: exactly what 1 does.
//
// Tuning "linear_precond" 1 (one slab): the PCG is preconditioned by a geometric multigrid V-cycle on a hierarchy of the
// stepping matrix that the model owns (mg_setup_linear): built once per set-up, never refreshed, independent of "precond" and
// of the tangent's hierarchy.  Level 0 is the context with the stepping matrix selected, in either operator form; its
// block-Jacobi D is the model's (the node blocks of d_A, or mf_linear_diag_q3 / _q2 <., true> + mf_diag_gather without a matrix).
#include <cmath>
#include <cstring>
#include <map>

#include "mi_internal.h"

namespace mi_detail
{
  struct LinearModel
  {
    double  theta = 0.5;
    double *d_K = nullptr, *d_M = nullptr, *d_A = nullptr, *d_dinvA = nullptr, *d_body = nullptr;
    bool    body_force_enabled = false;
    bool    factored = false; // the banded Cholesky factor of the (constant) system matrix is in the context's band
    // "linear_operator" 1 / 2: no d_K / d_M / d_A; the three operators as mf_linear_q3 / mf_linear_q2 runs them, the diagonal of the stepping
    // matrix in the layout the slot gathers read (mi_ctx::d_diag_blk's), the rule's tables -- all the model's own, so that
    // no key of the nonlinear path can take them away
    bool     mf = false;
    LinearMf op[3]; // K, M, stepping matrix
    double  *d_diag = nullptr, *d_tab_mf = nullptr; // (the tables of QGauss(p + 1): Tables1D(3, 4) | Tables1D(2, 3), tab27's layout)
    int32_t *d_diagpos_mf = nullptr;
    uint8_t *d_nomask = nullptr; // [nnodes] zeros: the constraint mask of K and M (no row replaced)
    // "linear_precond" 1: the hierarchy of the stepping matrix, the inverse node blocks of level 0 (full, and in 3D their
    // symmetric halves), the iterations of the previous step's solve (what cg_run may enqueue without polling)
    Multigrid *mg = nullptr;
    double    *d_dinv_blk = nullptr, *d_dinv_sym6 = nullptr;
    int        last_its = 0;
    // consistent-load operator on the interface nodes (scalar CSR over interface slots), :458-521
    std::vector<int32_t> B_rowptr, B_col;
    std::vector<double>  B_val;
  };

  void linear_destroy(mi_ctx *c)
  {
    if (!c->linear)
      return;
    mg_free(c->linear->mg);
    c->mg_linear = nullptr;
    for (double *p : {c->linear->d_K, c->linear->d_M, c->linear->d_A, c->linear->d_dinvA, c->linear->d_body, c->linear->d_diag,
                      c->linear->d_tab_mf, c->linear->d_dinv_blk, c->linear->d_dinv_sym6})
      if (p)
        hipFree(p);
    if (c->linear->d_diagpos_mf)
      hipFree(c->linear->d_diagpos_mf);
    if (c->linear->d_nomask)
      hipFree(c->linear->d_nomask);
    c->active_linear_mf = nullptr;
    delete c->linear;
    c->linear = nullptr;
  }

  namespace
  {
    // Jm[i][j] = dX_i/dxi_j of the d-linear cell map
    void jacobian(int dim, const double *verts, const double *xi, double Jm[3][3])
    {
      for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j)
          Jm[i][j] = (i == j && i >= dim) ? 1.0 : 0.0;
      for (int v = 0; v < (1 << dim); ++v)
        for (int j = 0; j < dim; ++j)
          {
            double g = ((v >> j) & 1) ? 1.0 : -1.0;
            for (int d = 0; d < dim; ++d)
              if (d != j)
                g *= ((v >> d) & 1) ? xi[d] : 1.0 - xi[d];
            for (int i = 0; i < dim; ++i)
              Jm[i][j] += verts[v * dim + i] * g;
          }
    }
  } // namespace
} // namespace mi_detail

using namespace mi_detail;

extern "C" {

// "linear_operator" 1 / 2: nothing is assembled.  Slot tables, slots and cell boxes where absent; the rule's tables; the three
// operators; the diagonal of the stepping matrix and its inverse; body = M (b, b, ...).  Tables and kernels by the degree
static int linear_setup_matrix_free(mi_ctx *c, LinearModel &L, const mi::Tables1D &t, double lambda, double theta)
{
  const mi::HostMesh &m  = c->mesh;
  const size_t        nn = size_t(m.nnodes);
  const double        mu = c->mat.mu, rho = c->mat.rho, dt = c->nm.delta_t;
  if (int rc = linear_mf_prepare(c))
    return rc;
  const bool q2 = c->degree == 2;
  if (int rc = upload(c, &L.d_tab_mf, t.packed()))
    return rc;
  std::vector<int32_t> dp(nn);
  for (size_t n = 0; n < nn; ++n)
    dp[n] = int32_t(n);
  if (int rc = upload(c, &L.d_diagpos_mf, dp))
    return rc;
  HIPCHK(c, hipMalloc((void **)&L.d_nomask, nn));
  HIPCHK(c, hipMemsetAsync(L.d_nomask, 0, nn, c->stream));
  HIPCHK(c, hipMalloc((void **)&L.d_diag, nn * 9 * sizeof(double)));
  HIPCHK(c, hipMalloc((void **)&L.d_dinvA, size_t(c->n) * sizeof(double)));
  // K and M are unconstrained (assemble_linear_cells drops entries in A only): x unmasked, no row replaced
  const double cK[3] = {1.0, 0.0, dt * dt * theta * theta}, cM[3] = {0.0, 1.0, 1.0};
  for (int w = 0; w < 3; ++w)
    L.op[w] = LinearMf{mi::MfLinearOp{lambda, mu, rho, cK[w], cM[w], w == 2 ? 1 : 0}, c->degree, L.d_tab_mf, L.d_diag, L.d_diagpos_mf,
                       w == 2 ? c->d_cmask : L.d_nomask};
  mi::MfParams f = mf_params(c);
  (q2 ? f.tab27 : f.tab_q3s) = L.d_tab_mf;
  f.yc = c->d_mf_yc, f.dst = c->d_mf_dst, f.slot_base = c->d_mf_slot_base, f.slot_src = c->d_mf_src;
  f.slot_inline = c->slots_layout == 1;
  if (c->linear_precond == 1)
    {
      // the nodes' whole blocks of the stepping matrix, cell by cell into slots of six, summed in slot order.  The gather's
      // constraint rule (row and column of a constrained dof dropped, |diagonal contribution| kept) is the model's: the
      // diagonal contributions are sums of squares, so nothing changes sign.  Out: the blocks, 1 / diagonal, D^-1 in both forms
      double *d_slots6 = nullptr;
      HIPCHK(c, hipMalloc((void **)&d_slots6, size_t(m.ncells) * m.npc * 6 * sizeof(double)));
      HIPCHK(c, hipMalloc((void **)&L.d_dinv_blk, nn * 9 * sizeof(double)));
      HIPCHK(c, hipMalloc((void **)&L.d_dinv_sym6, nn * 6 * sizeof(double)));
      (q2 ? mi::launch_mf_linear_diag_blk_q2 : mi::launch_mf_linear_diag_blk_q3)(f, L.op[2].op, int32_t(m.ncells), d_slots6, c->stream);
      mi::launch_mf_diag_gather(d_slots6, c->d_mf_slot_base, c->d_mf_src, c->d_cmask, L.d_diagpos_mf, L.d_diag, L.d_dinvA, L.d_dinv_blk,
                                L.d_dinv_sym6, m.nnodes, c->stream);
      const hipError_t e1 = hipGetLastError(), e2 = hipStreamSynchronize(c->stream);
      hipFree(d_slots6);
      HIPCHK(c, e1);
      HIPCHK(c, e2);
    }
  else
    (q2 ? mi::launch_mf_linear_diag_q2 : mi::launch_mf_linear_diag_q3)(f, L.op[2].op, int32_t(m.ncells), L.d_diag, L.d_dinvA, c->n, c->stream);
  HIPCHK(c, hipGetLastError());
  if (L.body_force_enabled)
    {
      // rho b int N_a = sum_b M_ab b: the shape functions sum to one (create_right_hand_side :358-373)
      HIPCHK(c, hipMalloc((void **)&L.d_body, size_t(c->n) * sizeof(double)));
      std::vector<double> b(size_t(c->n));
      for (size_t g = 0; g < b.size(); ++g)
        b[g] = c->mat.body_force[g % 3];
      HIPCHK(c, hipMemcpy(c->work(W_P), b.data(), b.size() * sizeof(double), hipMemcpyHostToDevice));
      c->active_linear_mf = &L.op[1];
      enqueue_spmv(c, c->work(W_P), L.d_body, nullptr, nullptr, nullptr);
      c->active_linear_mf = nullptr;
      HIPCHK(c, hipGetLastError());
    }
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return MI_OK;
}

// K, M, A assembled (tuning "linear_operator" 0) and the body-force vector
static int linear_assemble_operators(mi_ctx *c, LinearModel &L, const mi::Tables1D &t, double lambda, double theta)
{
  const mi::HostMesh &m   = c->mesh;
  const int           dim = c->dim, DD = dim * dim;
  const double        mu = c->mat.mu, rho = c->mat.rho, dt = c->nm.delta_t;
  if (int rc = linear_mf_leave(c))
    return rc;
  // K, M, A = M + theta^2 dt^2 K with zero boundary values applied, and the body-force vector: on the device
  const size_t nval = std::max<size_t>(1, size_t(m.nvalblocks()) * DD);
  double      *d_tab = nullptr;
  {
    const std::vector<double> tab = t.packed();
    HIPCHK(c, hipMalloc((void **)&d_tab, tab.size() * sizeof(double)));
    HIPCHK(c, hipMemcpy(d_tab, tab.data(), tab.size() * sizeof(double), hipMemcpyHostToDevice));
  }
  for (double **pp : {&L.d_K, &L.d_M, &L.d_A})
    {
      HIPCHK(c, hipMalloc((void **)pp, nval * sizeof(double)));
      HIPCHK(c, hipMemsetAsync(*pp, 0, nval * sizeof(double), c->stream));
    }
  if (L.body_force_enabled)
    {
      HIPCHK(c, hipMalloc((void **)&L.d_body, size_t(c->n) * sizeof(double)));
      HIPCHK(c, hipMemsetAsync(L.d_body, 0, size_t(c->n) * sizeof(double), c->stream));
    }
  {
    mi::LinAsmParams p{};
    p.conn    = c->d_conn;
    p.cverts  = c->d_cverts;
    p.off     = c->d_off;
    p.rowinfo = reinterpret_cast<const int2 *>(c->d_rowinfo);
    p.cmask   = c->d_cmask;
    p.tab     = d_tab;
    p.np1     = t.np1;
    p.nq1     = t.nq1;
    p.lambda  = lambda;
    p.mu      = mu;
    p.rho     = rho;
    p.ctheta  = dt * dt * theta * theta;
    for (int d = 0; d < 3; ++d)
      p.body[d] = c->mat.body_force[d];
    p.K       = L.d_K;
    p.M       = L.d_M;
    p.A       = L.d_A;
    p.bodyvec = L.d_body;
    for (int col = 0; col < m.ncolours; ++col)
      {
        p.cell_begin = m.colour_begin[size_t(col)];
        p.cell_count = int32_t(m.colour_begin[size_t(col) + 1] - m.colour_begin[size_t(col)]);
        mi::launch_assemble_linear(dim, p, c->stream);
      }
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipStreamSynchronize(c->stream));
    hipFree(d_tab);
  }
  return MI_OK;
}

// K, M, stepping matrix, load operator and body force of ONE slab: the launches run over the slab's local cells
// (ghost layer included), which completes every owned row exactly as the tangent's assembly does
static int linear_setup_member(mi_ctx *c, double theta)
{
  linear_destroy(c);
  c->linear      = new LinearModel;
  LinearModel &L = *c->linear;
  L.theta        = theta;

  const mi::HostMesh &m   = c->mesh;
  const int           dim = c->dim, npc = m.npc;
  const double        mu = c->mat.mu, nu = c->mat.nu;
  const double        lambda = 2 * mu * nu / (1 - 2 * nu); // parameters.cc:189

  mi::Tables1D t;
  t.build(c->degree, c->degree + 1); // quad_order = p+1 (linear_elasticity.cc:61)
  int nqf = 1;
  for (int d = 0; d < dim - 1; ++d)
    nqf *= t.nq1;

  double bn = 0;
  for (int d = 0; d < 3; ++d)
    bn += c->mat.body_force[d] * c->mat.body_force[d];
  L.body_force_enabled = std::sqrt(bn) > 1e-15; // :62

  L.mf = c->linear_operator != 0; // (1 and 2: set_tuning has checked the mesh)
  if (int rc = L.mf ? linear_setup_matrix_free(c, L, t, lambda, theta) : linear_assemble_operators(c, L, t, lambda, theta))
    return rc;

  // consistent-load operator B_ab = int_interface N_a N_b dA (assemble_consistent_loading :458-521, no pull-back)
  {
    std::map<int32_t, int32_t> slot;
    for (size_t i = 0; i < m.iface_nodes.size(); ++i)
      slot[m.iface_nodes[i]] = int32_t(i);
    std::vector<std::map<int32_t, double>> rows(m.iface_nodes.size());
    const int np1 = t.np1, nq1 = t.nq1;
    for (const auto &fc : m.iface_faces)
      for (int f = 0; f < 2 * dim; ++f)
        {
          if (!((fc.face >> f) & 1))
            continue;
          const int     nd = f / 2, side = f & 1;
          const double *verts = &m.cverts[size_t(fc.cell) * m.nv * dim];
          int           tang[2] = {0, 0}, nt = 0;
          for (int d = 0; d < dim; ++d)
            if (d != nd)
              tang[nt++] = d;
          for (int fq = 0; fq < nqf; ++fq)
            {
              const int f1 = fq % nq1, f2 = fq / nq1;
              double    xi[3] = {0, 0, 0}, w = t.qw[f1];
              xi[nd]          = side ? 1.0 : 0.0;
              xi[tang[0]]     = t.qx[f1];
              if (dim == 3)
                {
                  xi[tang[1]] = t.qx[f2];
                  w *= t.qw[f2];
                }
              double Jm[3][3];
              jacobian(dim, verts, xi, Jm);
              double area;
              if (dim == 2)
                area = std::hypot(Jm[0][tang[0]], Jm[1][tang[0]]);
              else
                {
                  const double a0 = Jm[0][tang[0]], a1 = Jm[1][tang[0]], a2 = Jm[2][tang[0]];
                  const double b0 = Jm[0][tang[1]], b1 = Jm[1][tang[1]], b2 = Jm[2][tang[1]];
                  area = std::sqrt((a1 * b2 - a2 * b1) * (a1 * b2 - a2 * b1) + (a2 * b0 - a0 * b2) * (a2 * b0 - a0 * b2) +
                                   (a0 * b1 - a1 * b0) * (a0 * b1 - a1 * b0));
                }
              const double JxW = area * w;
              // shape values on the face: product of 1D values along the tangential axes
              std::vector<std::pair<int32_t, double>> nodes;
              for (int a = 0; a < npc; ++a)
                {
                  const int ai[3] = {a % np1, (a / np1) % np1, dim == 3 ? a / (np1 * np1) : 0};
                  if (ai[nd] != (side ? c->degree : 0))
                    continue;
                  double n = t.N[size_t(f1) * np1 + ai[tang[0]]];
                  if (dim == 3)
                    n *= t.N[size_t(f2) * np1 + ai[tang[1]]];
                  nodes.push_back({m.conn[size_t(fc.cell) * npc + a], n});
                }
              for (const auto &na : nodes)
                for (const auto &nb : nodes)
                  rows[size_t(slot[na.first])][slot[nb.first]] += na.second * nb.second * JxW;
            }
        }
    L.B_rowptr.assign(1, 0);
    for (const auto &r : rows)
      {
        for (const auto &kv : r)
          {
            L.B_col.push_back(kv.first);
            L.B_val.push_back(kv.second);
          }
        L.B_rowptr.push_back(int32_t(L.B_col.size()));
      }
  }

  // Jacobi diagonal of A (matrix-free: formed above)
  if (!L.mf)
    {
      HIPCHK(c, hipMalloc((void **)&L.d_dinvA, size_t(c->n) * sizeof(double)));
      mi::launch_extract_dinv(c->dim, L.d_A, c->d_diagpos, L.d_dinvA, m.nnodes, c->stream);
      HIPCHK(c, hipGetLastError());
    }
  HIPCHK(c, hipMemsetAsync(c->d_vecs, 0, size_t(MI_V_COUNT) * size_t(c->n) * sizeof(double), c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return MI_OK;
}

// the model's multigrid ("linear_precond" 1, one slab): the inverse node blocks of level 0 where a matrix is assembled (the
// matrix-free set-up has formed them), then the hierarchy
static int linear_setup_multigrid(mi_ctx *c, double theta)
{
  LinearModel &L = *c->linear;
  if (!L.mf)
    {
      const size_t nn = size_t(c->mesh.nnodes), DD = size_t(c->dim) * c->dim;
      HIPCHK(c, hipMalloc((void **)&L.d_dinv_blk, nn * DD * sizeof(double)));
      if (c->dim == 3)
        HIPCHK(c, hipMalloc((void **)&L.d_dinv_sym6, nn * 6 * sizeof(double)));
      mi::launch_extract_dinv_blk(c->dim, L.d_A, c->d_diagpos, L.d_dinv_blk, L.d_dinv_sym6, c->mesh.nnodes, c->stream);
      HIPCHK(c, hipGetLastError());
    }
  return mg_setup_linear(c, theta, L.d_dinv_blk, L.d_dinv_sym6, &L.mg);
}

int mi_linear_setup(mi_ctx *c, double theta)
{
  HIPCHK(c, hipSetDevice(c->device));
  if (!(theta >= 0.0 && theta <= 1.0))
    return fail(c, MI_EINVAL, "theta must be in [0,1]");
  for (mi_ctx *m : c->team->members)
    {
      const int rc = linear_setup_member(m, theta);
      if (rc)
        return m == c ? rc : fail(c, rc, "%s", m->err.c_str());
    }
  if (c->linear_precond == 1 && c->team->size == 1)
    return linear_setup_multigrid(c, theta);
  return MI_OK;
}

int mi_linear_step(mi_ctx *c, int data_consistent, double abs_tol, int64_t max_it, int *its, double *res)
{
  if (!c->linear)
    return fail(c, MI_EINVAL, "mi_linear_setup has not been called");
  if (!(abs_tol > 0))
    return fail(c, MI_EINVAL, "absolute tolerance must be positive");
  HIPCHK(c, hipSetDevice(c->device));
  Team      &T  = *c->team;
  mi_ctx    *c0 = T.members[0];
  const int  dim = c->dim;
  std::vector<mi::LinearParams> ps;
  for (mi_ctx *m : T.members)
    {
      LinearModel &L   = *m->linear;
      const int    nif = int(m->mesh.iface_nodes.size());
      // load at the interface dofs: face integral of the traction ("Stress", :383-384) or the nodal forces as
      // they come ("Force", :385-388); interface sized, computed on the host from the last coupling data
      // (c0->h_iface holds the GLOBAL interface array, iface_slot maps the slab's nodes into it)
      double *load = m->vec(MI_V_NEWTON_UPDATE);
      if (nif > 0)
        {
          if (c0->h_iface.size() != T.iface_global.size() * size_t(dim))
            c0->h_iface.assign(T.iface_global.size() * size_t(dim), 0.0);
          auto coupling = [&](int i, int k) { return c0->h_iface[size_t(m->iface_slot[size_t(i)]) * dim + k]; };
          double *stage = m->h_pinned + 64;
          for (int i = 0; i < nif; ++i)
            for (int k = 0; k < dim; ++k)
              {
                double s = 0;
                if (data_consistent)
                  for (int32_t e = L.B_rowptr[size_t(i)]; e < L.B_rowptr[size_t(i) + 1]; ++e)
                    s += L.B_val[size_t(e)] * coupling(L.B_col[size_t(e)], k);
                else
                  s = coupling(i, k);
                stage[i * dim + k] = s;
              }
          HIPCHK(m, hipMemcpyAsync(m->d_iface_buf, stage, size_t(nif) * dim * sizeof(double), hipMemcpyHostToDevice,
                                   m->stream));
          mi::launch_scatter_nodes(dim, load, m->d_iface_nodes, nif, m->d_iface_buf, m->stream);
        }
      mi::LinearParams p{};
      p.load  = load;
      p.body  = L.body_force_enabled ? L.d_body : nullptr;
      p.f_old = m->vec(MI_L_OLD_STRESS);
      p.v     = m->vec(MI_L_VELOCITY);
      p.d     = m->vec(MI_L_DISPLACEMENT);
      p.v_old = m->vec(MI_L_OLD_VELOCITY);
      p.d_old = m->vec(MI_L_OLD_DISPLACEMENT);
      p.rhs   = m->vec(MI_L_SYSTEM_RHS);
      p.w     = m->vec(MI_V_SOLUTION_DELTA);
      p.theta = L.theta;
      p.dt    = m->nm.delta_t;
      p.n     = m->n; // pointwise on all local dofs: the ghost copies stay consistent
      mi::launch_linear_rhs_prepare(p, m->stream);
      ps.push_back(p);
    }
  // M v_old and K w  (:411-420 with the two K products merged); ghost planes of both operands are consistent
  auto self = [](mi_ctx *m) { return m; };
  int  rc;
  for (mi_ctx *m : T.members)
    linear_select(m, 1);
  int t = tic(c0, MI_T_SPMV);
  rc    = team_spmv(
    T, self, [](mi_ctx *m) { return m->vec(MI_L_OLD_VELOCITY); }, [](mi_ctx *m) { return m->work(W_R); }, nullptr);
  toc(c0, t);
  for (mi_ctx *m : T.members)
    linear_select(m, 0);
  t = tic(c0, MI_T_SPMV);
  if (!rc)
    rc = team_spmv(
      T, self, [](mi_ctx *m) { return m->vec(MI_V_SOLUTION_DELTA); }, [](mi_ctx *m) { return m->work(W_Q); }, nullptr);
  toc(c0, t);
  for (size_t k = 0; k < T.members.size() && !rc; ++k)
    {
      mi_ctx *m = T.members[k];
      mi::launch_linear_rhs_finish(dim, ps[k], m->work(W_R), m->work(W_Q), m->d_cmask, m->stream);
    }
  HIPCHK(c, hipGetLastError());
  // solve (:531-551): absolute tolerance, start vector = previous velocity
  for (mi_ctx *m : T.members)
    linear_select(m, 2);
  // (matrix-free: there is no matrix to factorise -- the PCG route, as for a system too large for the band solver)
  bool direct = false;
  if (!rc && c0->solver_direct && T.size == 1 && !c0->linear->mf && direct_prepare(c0) == MI_OK)
    {
      // "Solver type = Direct" (:553-559): the system matrix is constant, so it is factorised ONCE and a step is one
      // forward and one backward substitution
      direct          = true;
      LinearModel &Lm = *c0->linear;
      rc = direct_factor_solve(c0, Lm.d_A, c0->vec(MI_L_SYSTEM_RHS), c0->vec(MI_L_VELOCITY), !Lm.factored, true);
      Lm.factored = Lm.factored || rc == MI_OK;
      if (its)
        *its = 1;
      if (res)
        *res = 0.0;
    }
  if (!rc && !direct)
    {
      // (multigrid: the iterations of the previous step's solve may be enqueued without polling -- the same iterates)
      LinearModel &Lm = *c0->linear;
      int          n_its = 0;
      rc = cg_run(c0, MI_L_VELOCITY, MI_L_SYSTEM_RHS, -abs_tol, max_it, &n_its, res, false, false, Lm.mg ? Lm.last_its : 0);
      Lm.last_its = rc == MI_OK ? n_its : 0;
      if (its)
        *its = n_its;
    }
  for (mi_ctx *m : T.members)
    linear_select(m, -1);
  if (rc)
    return rc;
  for (size_t k = 0; k < T.members.size(); ++k)
    mi::launch_linear_update_displacement(ps[k], T.members[k]->stream); // :579-586
  HIPCHK(c, hipGetLastError());
  return sync(c0);
}

// 1/2 u . (K u), 1/2 v . (M v), -u . f_body: two products of the current set-up with the dot product fused (their partials
// count per workgroup of the product: the slot gather's or the sliced-ELL launch's, as in cg_run), one reduction of the
// body-force vector, the three sums in one all-reduce.  No new point kernel
int mi_linear_energy(mi_ctx *c, mi_energy_info *out)
{
  if (!c || !out)
    return c ? fail(c, MI_EINVAL, "mi_linear_energy: null argument") : MI_EINVAL;
  if (!c->linear)
    return fail(c, MI_EINVAL, "mi_linear_setup has not been called");
  HIPCHK(c, hipSetDevice(c->device));
  Team &T    = *c->team;
  auto  self = [](mi_ctx *m) { return m; };
  int   rc   = MI_OK;
  for (int w = 0; w < 2 && !rc; ++w) // K on the displacement, M on the velocity
    {
      const int               vid = w == 0 ? MI_L_DISPLACEMENT : MI_L_VELOCITY;
      std::vector<SpmvFusion> fu;
      for (mi_ctx *m : T.members)
        {
          linear_select(m, w);
          fu.push_back(SpmvFusion{m->vec(vid), m->part(5 + w), nullptr});
        }
      rc = team_spmv(T, self, [vid](mi_ctx *m) { return m->vec(vid); }, [](mi_ctx *m) { return m->work(W_Q); }, fu.data());
      for (mi_ctx *m : T.members)
        {
          const int np = m->linear->mf ? m->grid_gdot : m->grid_spmv;
          mi::launch_finish_sum(m->part(5 + w), np, energy_scalars(m) + w, m->stream);
          linear_select(m, -1);
        }
    }
  if (rc)
    return rc;
  for (mi_ctx *m : T.members)
    {
      double *sc = energy_scalars(m);
      HIPCHK(m, hipMemsetAsync(sc + 2, 0, 2 * sizeof(double), m->stream));
      if (m->linear->body_force_enabled)
        {
          mi::launch_dot_partials(m->vec(MI_L_DISPLACEMENT) + m->own0, m->linear->d_body + m->own0, m->own_n, m->part(7), m->grid_vec,
                                  m->stream);
          mi::launch_finish_sum(m->part(7), m->grid_vec, sc + 2, m->stream);
        }
    }
  HIPCHK(c, hipGetLastError());
  if ((rc = energy_finish(T, out, nullptr)))
    return rc;
  out->strain *= 0.5, out->kinetic *= 0.5, out->body = -out->body;
  return MI_OK;
}

int mi_linear_matrix_get_csr(mi_ctx *c, int which, int64_t *rowptr, int32_t *col, double *val)
{
  if (!c->linear || which < 0 || which > 2)
    return fail(c, MI_EINVAL, "linear model not set up or bad matrix id");
  if (team_size(c) != 1)
    return fail(c, MI_EINVAL, "matrix export is only available on an undecomposed mesh");
  if (c->linear->mf)
    return fail(c, MI_EINVAL, "matrix export: the matrix-free linear model keeps no assembled operator (\"linear_operator\" 0)");
  const int           D = c->dim, DD = D * D;
  const mi::HostMesh &m = c->mesh;
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  std::vector<double> bv(size_t(m.nvalblocks()) * DD);
  HIPCHK(c, hipMemcpy(bv.data(), which == 0 ? c->linear->d_K : which == 1 ? c->linear->d_M : c->linear->d_A,
                      bv.size() * sizeof(double), hipMemcpyDeviceToHost));
  int64_t k = 0;
  for (int64_t nd = 0; nd < m.nnodes; ++nd)
    for (int i = 0; i < D; ++i)
      {
        rowptr[nd * D + i] = k;
        for (int32_t b = m.rowptr[size_t(nd)]; b < m.rowptr[size_t(nd) + 1]; ++b)
          for (int j = 0; j < D; ++j)
            {
              col[k] = m.colidx[size_t(b)] * D + j;
              val[k] = bv[size_t(m.valpos(nd, int(b - m.rowptr[size_t(nd)]))) * DD + i * D + j];
              ++k;
            }
      }
  rowptr[m.nnodes * D] = k;
  return MI_OK;
}

// y = K x (0), M x (1) or A x (2) through the device kernels of the current mode: the sliced-ELL product on the assembled
// arrays or mf_linear_q3 / mf_linear_q2 + mf_gather.  The product is timed as MI_T_SPMV (device stamps) when profiling is on.
int mi_linear_apply(mi_ctx *c, int which, const double *x_host, double *y_host)
{
  if (!c->linear || which < 0 || which > 3 || !x_host || !y_host)
    return fail(c, MI_EINVAL, "linear model not set up, bad operator id or null argument");
  if (team_size(c) != 1)
    return fail(c, MI_EINVAL, "mi_linear_apply is only available on an undecomposed mesh");
  if (which == 3 && !c->linear->mg)
    return fail(c, MI_EINVAL, "mi_linear_apply: the linear set-up has no multigrid hierarchy (\"linear_precond\" 1 and mi_linear_setup)");
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (which == 3) // y = B x: one V-cycle, as the solve applies it to its residual
    {
      HIPCHK(c, hipMemcpy(c->work(W_R), x_host, size_t(c->n) * sizeof(double), hipMemcpyHostToDevice));
      linear_select(c, 2);
      const int rc = mg_apply(*c->team);
      linear_select(c, -1);
      if (rc)
        return rc;
      HIPCHK(c, hipStreamSynchronize(c->stream));
      HIPCHK(c, hipMemcpy(y_host, c->work(W_Z), size_t(c->n) * sizeof(double), hipMemcpyDeviceToHost));
      return MI_OK;
    }
  HIPCHK(c, hipMemcpy(c->work(W_P), x_host, size_t(c->n) * sizeof(double), hipMemcpyHostToDevice));
  const bool level = c->active_sell_vals && c->active_sell_vals == c->linear->d_A; // a borrowed multigrid level keeps its selection
  linear_select(c, which);
  const int t = tic(c, MI_T_SPMV);
  enqueue_spmv(c, c->work(W_P), c->work(W_Q), nullptr, nullptr, nullptr);
  toc(c, t);
  linear_select(c, level ? 2 : -1);
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipStreamSynchronize(c->stream));
  HIPCHK(c, hipMemcpy(y_host, c->work(W_Q), size_t(c->n) * sizeof(double), hipMemcpyDeviceToHost));
  return MI_OK;
}

// the Jacobi diagonal of the stepping matrix in use: the diagonal entries whose reciprocals the PCG multiplies with -- out of
// the assembled array, or as mf_linear_diag_q3 / mf_linear_diag_q2 formed them
int mi_linear_get_diagonal(mi_ctx *c, double *diag_host)
{
  if (!c->linear || !diag_host)
    return fail(c, MI_EINVAL, "linear model not set up or null argument");
  if (team_size(c) != 1)
    return fail(c, MI_EINVAL, "mi_linear_get_diagonal is only available on an undecomposed mesh");
  const LinearModel &L = *c->linear;
  const int          D = c->dim, DD = D * D;
  const size_t       cnt = size_t(c->mesh.nnodes) * DD;
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  std::vector<double> blk(cnt);
  if (L.mf)
    HIPCHK(c, hipMemcpy(blk.data(), L.d_diag, cnt * sizeof(double), hipMemcpyDeviceToHost));
  else
    {
      double *tmp = nullptr;
      HIPCHK(c, hipMalloc((void **)&tmp, cnt * sizeof(double)));
      mi::launch_gather_diag_blocks(D, L.d_A, c->d_diagpos, tmp, c->mesh.nnodes, c->stream);
      const hipError_t e1 = hipStreamSynchronize(c->stream);
      const hipError_t e2 = hipMemcpy(blk.data(), tmp, cnt * sizeof(double), hipMemcpyDeviceToHost);
      hipFree(tmp);
      HIPCHK(c, e1);
      HIPCHK(c, e2);
    }
  for (int64_t n = 0; n < c->mesh.nnodes; ++n)
    for (int k = 0; k < D; ++k)
      diag_host[n * D + k] = blk[size_t(n) * DD + k * D + k];
  return MI_OK;
}

// the node blocks of the stepping matrix in use, [nnodes][dim][dim]: what the block-Jacobi smoother of "linear_precond" 1 inverts
// -- out of the assembled array, or as mf_linear_diag_q3 / _q2 + the gather formed them (diagonal entries alone with the key at 0)
int mi_linear_get_diagonal_blocks(mi_ctx *c, double *blocks)
{
  if (!c->linear || !blocks)
    return fail(c, MI_EINVAL, "linear model not set up or null argument");
  if (team_size(c) != 1)
    return fail(c, MI_EINVAL, "mi_linear_get_diagonal_blocks is only available on an undecomposed mesh");
  const LinearModel &L   = *c->linear;
  const size_t       cnt = size_t(c->mesh.nnodes) * c->dim * c->dim;
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (L.mf)
    {
      HIPCHK(c, hipMemcpy(blocks, L.d_diag, cnt * sizeof(double), hipMemcpyDeviceToHost));
      return MI_OK;
    }
  double *tmp = nullptr;
  HIPCHK(c, hipMalloc((void **)&tmp, cnt * sizeof(double)));
  mi::launch_gather_diag_blocks(c->dim, L.d_A, c->d_diagpos, tmp, c->mesh.nnodes, c->stream);
  const hipError_t e1 = hipStreamSynchronize(c->stream);
  const hipError_t e2 = hipMemcpy(blocks, tmp, cnt * sizeof(double), hipMemcpyDeviceToHost);
  hipFree(tmp);
  HIPCHK(c, e1);
  HIPCHK(c, e2);
  return MI_OK;
}

// ---- read-only view of the model's hierarchy (the contracts of mi_mg_n_levels, mi_mg_level_describe, mi_mg_level_context)
int mi_linear_mg_n_levels(const mi_ctx *c)
{
  return c->linear ? mg_n_levels(c->linear->mg) : 0;
}

int mi_linear_mg_level_describe(mi_ctx *c, int level, mi_mg_level_desc *out)
{
  if (!out)
    return fail(c, MI_EINVAL, "mi_linear_mg_level_describe: null argument");
  const int nl = mi_linear_mg_n_levels(c);
  if (level < 0 || level >= nl)
    return fail(c, MI_EINVAL, "mi_linear_mg_level_describe: level %d of %d (\"linear_precond\" 1 and mi_linear_setup)", level, nl);
  return mg_describe(c, *c->linear->mg, level, out);
}

int mi_linear_mg_level_context(mi_ctx *c, int level, mi_ctx **borrowed)
{
  if (!borrowed)
    return fail(c, MI_EINVAL, "mi_linear_mg_level_context: null argument");
  *borrowed    = nullptr;
  const int nl = mi_linear_mg_n_levels(c);
  if (level < 0 || level >= nl)
    return fail(c, MI_EINVAL, "mi_linear_mg_level_context: level %d of %d (\"linear_precond\" 1 and mi_linear_setup)", level, nl);
  *borrowed = mg_level_ctx(*c->linear->mg, level);
  return MI_OK;
}

} // extern "C"

// which operator the next products of a slab apply: 0 K, 1 M, 2 the stepping matrix; -1 none (back to the tangent).  With the
// stepping matrix its hierarchy becomes the active one, where the model has one
void mi_detail::linear_select(mi_ctx *m, int which)
{
  LinearModel &L      = *m->linear;
  m->active_sell_vals = (which < 0 || L.mf) ? nullptr : which == 0 ? L.d_K : which == 1 ? L.d_M : L.d_A;
  m->active_linear_mf = (which < 0 || !L.mf) ? nullptr : &L.op[which];
  m->active_dinv      = which == 2 ? L.d_dinvA : nullptr;
  m->mg_linear        = which == 2 ? L.mg : nullptr;
}

// a level >= 1 of the model's hierarchy: the assembled linear model of the level's own mesh, the stepping matrix selected for
// good, its inverse node blocks where the level context keeps those of its tangent (it never assembles one)
int mi_detail::linear_setup_level(mi_ctx *lc, double theta)
{
  lc->linear_operator = 0;
  if (const int rc = linear_setup_member(lc, theta))
    return rc;
  linear_select(lc, 2);
  const size_t nn = size_t(lc->mesh.nnodes), DD = size_t(lc->dim) * lc->dim;
  if (!lc->d_dinv_blk)
    HIPCHK(lc, hipMalloc((void **)&lc->d_dinv_blk, nn * DD * sizeof(double)));
  if (!lc->d_dinv_sym6 && lc->dim == 3)
    HIPCHK(lc, hipMalloc((void **)&lc->d_dinv_sym6, nn * 6 * sizeof(double)));
  mi::launch_extract_dinv_blk(lc->dim, lc->linear->d_A, lc->d_diagpos, lc->d_dinv_blk, lc->d_dinv_sym6, lc->mesh.nnodes, lc->stream);
  HIPCHK(lc, hipGetLastError());
  return MI_OK;
}

// The modal analysis of the linear model (mi_linear_modes and the block-vector hooks) is compiled with this translation unit:
// the library is linked from a fixed list of objects in more than one place (the test builds against the RCCL double among
// them), and the eigensolver is the linear model's.
#include "mi_modes.cpp"
