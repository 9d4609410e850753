// Consistent mass on the device and the L2 projection of a state onto another mesh: mi_mass_apply, mi_mass_solve,
// mi_project_load, mi_state_project.  Part of mi_ctx.cpp's translation unit (included at its end).
//
// M is the unit-density vector mass on the assembly's rule QGauss(p + 2), applied cell by cell without a matrix
// (mass_apply_q2 / mass_apply_q3 on 3D Q2 / Q3, mass_apply_cells elsewhere; colour by colour).  The solve is a Jacobi-preconditioned CG on all columns at once whose scalars and
// done-flags stay on the device; the load of a source field is integrated on a composite rule over dst's cells with src's
// fields from field_at_points.  Scratch is allocated per call and freed before return; the calls touch no state vector (but the
// six target vectors of mi_state_project), record, matrix, hierarchy, counter or timing.

namespace mi_detail
{
  struct DevBuf // device scratch of one call
  {
    void *p = nullptr;
    ~DevBuf()
    {
      if (p)
        hipFree(p);
    }
    double *d() const { return static_cast<double *>(p); }
  };
  static const int project_six[6] = {MI_V_TOTAL_DISPLACEMENT, MI_V_TOTAL_DISPLACEMENT_OLD, MI_V_VELOCITY,
                                     MI_V_VELOCITY_OLD,       MI_V_ACCELERATION,           MI_V_ACCELERATION_OLD};

  // y = M x for the device blocks x, y [nrhs][n] (diag: y [n] = the diagonal of M), enqueued on c's stream
  int enqueue_mass_apply(mi_ctx *c, int nrhs, int masked, bool diag, const double *x, double *y)
  {
    if (int rc = energy_box_prepare(c)) // (the cells' boxes for the sum-factorised forms, where the context keeps none)
      return rc;
    HIPCHK(c, hipMemsetAsync(y, 0, size_t(diag ? 1 : nrhs) * size_t(c->n) * sizeof(double), c->stream));
    mi::MfParams f = mf_params(c);
    if (!f.cellbox)
      f.cellbox = c->d_energy_box;
    static const bool generic = post_generic("MI_MASS_GENERIC");
    mi::MassParams    mp{};
    mp.conn = c->d_conn, mp.cverts = c->d_cverts, mp.tab = c->d_tab, mp.cmask = c->d_cmask;
    mp.x = x, mp.y = y, mp.n = c->n, mp.nrhs = nrhs, mp.masked = masked, mp.diag = diag ? 1 : 0;
    for (int col = 0; col < c->mesh.ncolours; ++col)
      {
        mp.cell_begin = c->mesh.colour_begin[col];
        mp.cell_count = int32_t(c->mesh.colour_begin[col + 1] - c->mesh.colour_begin[col]);
        if (mi::launch_mass_apply(c->dim, c->degree, f, mp, generic, c->stream))
          return fail(c, MI_EINVAL, "no mass kernel for dim=%d degree=%d", c->dim, c->degree);
      }
    HIPCHK(c, hipGetLastError());
    return MI_OK;
  }

  // the solve on device blocks: d_b is read (masked: ignored on constrained dofs), d_x written.  its, res [nrhs], bb [nrhs]
  // (the columns' |b|^2) on the host, each or NULL.  MI_ENOCONV_LIN with everything written when max_it does not suffice
  static int mass_solve_device(mi_ctx *c, int nrhs, int masked, const double *d_b, double *d_x, double tol, int max_it, int *its,
                               double *res, double *bb)
  {
    const size_t n = size_t(c->n), blk = size_t(nrhs) * n, nblk = size_t(mi::mass_chunks(c->n));
    const size_t npart = size_t(nrhs) * nblk, nstate = (sizeof(mi::MassCgState) + sizeof(double) - 1) / sizeof(double);
    DevBuf       w;
    HIPCHK(c, hipMalloc(&w.p, (3 * blk + n + 2 * npart + nstate) * sizeof(double)));
    double *r = w.d(), *p = r + blk, *q = p + blk, *dinv = q + blk, *part_rr = dinv + n, *part_rz = part_rr + npart;
    auto   *st = reinterpret_cast<mi::MassCgState *>(part_rz + npart);
    hipStream_t s = c->stream;
    HIPCHK(c, hipMemcpyAsync(r, d_b, blk * sizeof(double), hipMemcpyDeviceToDevice, s));
    if (masked)
      for (int j = 0; j < nrhs; ++j)
        mi::launch_zero_constrained(c->dim, r + size_t(j) * n, c->d_cmask, c->n, s);
    HIPCHK(c, hipMemsetAsync(d_x, 0, blk * sizeof(double), s));
    HIPCHK(c, hipMemsetAsync(st, 0, sizeof(mi::MassCgState), s));
    if (int rc = enqueue_mass_apply(c, 1, 0, true, nullptr, dinv))
      return rc;
    mi::launch_mass_diag_invert(c->dim, dinv, c->d_cmask, masked, c->n, s);
    mi::launch_mass_cg_update_xr(true, d_x, r, p, q, dinv, c->n, nrhs, st, part_rr, part_rz, s);
    mi::launch_mass_cg_scalars(part_rr, part_rz, c->n, nrhs, 0, tol, st, s);
    int32_t nactive = 0;
    HIPCHK(c, hipMemcpyAsync(&nactive, &st->nactive, sizeof(int32_t), hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));
    int it = 0;
    while (nactive > 0 && it < max_it)
      {
        ++it;
        mi::launch_mass_cg_update_p(it == 1, p, r, dinv, c->n, nrhs, st, s);
        if (int rc = enqueue_mass_apply(c, nrhs, masked, false, p, q))
          return rc;
        mi::launch_mass_col_dots(p, q, c->n, nrhs, part_rr, st->pq, s);
        mi::launch_mass_cg_update_xr(false, d_x, r, p, q, dinv, c->n, nrhs, st, part_rr, part_rz, s);
        mi::launch_mass_cg_scalars(part_rr, part_rz, c->n, nrhs, it, tol, st, s);
        HIPCHK(c, hipMemcpyAsync(&nactive, &st->nactive, sizeof(int32_t), hipMemcpyDeviceToHost, s));
        HIPCHK(c, hipStreamSynchronize(s));
      }
    // the residual of what is returned, freshly formed: |b - M x| / |b|
    if (int rc = enqueue_mass_apply(c, nrhs, masked, false, d_x, q))
      return rc;
    mi::launch_mass_fresh_residual(c->dim, d_b, q, c->d_cmask, masked, c->n, nrhs, r, s);
    mi::launch_mass_col_dots(r, r, c->n, nrhs, part_rr, st->fresh, s);
    HIPCHK(c, hipGetLastError());
    mi::MassCgState h;
    HIPCHK(c, hipMemcpyAsync(&h, st, sizeof(h), hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));
    int    slowest = 0;
    double worst   = 0.0;
    for (int j = 0; j < nrhs; ++j)
      {
        const double rj = h.bb[j] > 0.0 ? std::sqrt(h.fresh[j] / h.bb[j]) : 0.0;
        if (res)
          res[j] = rj;
        if (bb)
          bb[j] = h.bb[j];
        slowest = std::max(slowest, int(h.its[j]));
        worst   = std::max(worst, rj);
      }
    if (its)
      *its = slowest;
    if (nactive > 0)
      return fail(c, MI_ENOCONV_LIN, "mass solve: %d of %d columns not converged in %d iterations (worst |b - M x| / |b| = %.3e)", int(nactive),
                  nrhs, max_it, worst);
    return MI_OK;
  }

  // The consistent stress recovery (tuning "stress_projection" 1), the end of enqueue_stress: the accumulator's sums b_k(i) =
  // sum N_i sigma_k JxW are packed into two vector columns, M x = b is solved unmasked by the solve above to
  // STRESS_PROJECTION_TOL within STRESS_PROJECTION_MAX_IT iterations, and the columns are unpacked into sigma, von Mises (of the
  // solved tensor) and W behind the accumulator, where stress_finish leaves the lumped field.  Scratch of the call, freed on return
  constexpr double STRESS_PROJECTION_TOL    = 1e-13;
  constexpr int    STRESS_PROJECTION_MAX_IT = 1000;
  static int stress_consistent_solve(mi_ctx *c)
  {
    const size_t nn = size_t(c->mesh.nnodes), n = size_t(c->n), ncomp = size_t(c->dim * (c->dim + 1) / 2);
    DevBuf       w;
    HIPCHK(c, hipMalloc(&w.p, 4 * n * sizeof(double)));
    double *b = w.d(), *x = b + 2 * n, *out = c->d_stress + nn * 8;
    mi::launch_stress_pack(c->dim, c->d_stress, int64_t(nn), b, c->stream);
    HIPCHK(c, hipGetLastError());
    int       its = 0;
    const int rc  = mass_solve_device(c, 2, 0, b, x, STRESS_PROJECTION_TOL, STRESS_PROJECTION_MAX_IT, &its, nullptr, nullptr);
    c->stress_projection_its = its;
    if (rc)
      return rc;
    mi::launch_stress_unpack(c->dim, x, c->d_stress, int64_t(nn), out, out + nn * ncomp, out + nn * (ncomp + 1), c->stream);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipStreamSynchronize(c->stream)); // (the columns are freed on return)
    return MI_OK;
  }

  // b [n_which][n(dst)] on the device := the load of src's vectors which[] on the composite rule; src_sq [n_which] and the count of
  // points on the host.  dst's stream carries dst's kernels, src's stream the point evaluation, as mi_state_transfer
  static int project_load_device(mi_ctx *dst, mi_ctx *src, int n_which, const int *which, int sub, double *d_b, double *src_sq,
                                 int64_t *n_points)
  {
    const mi::HostMesh &m = dst->mesh;
    const int           dim = dst->dim, nq1 = dst->tab.nq1, np1 = dst->degree + 1, ns1 = sub * nq1;
    const int64_t       pc = dim == 3 ? int64_t(ns1) * ns1 * ns1 : int64_t(ns1) * ns1;
    // dst's 1D basis at the composite rule's points, xi = (box + x_g) / sub as the kernels form it
    std::vector<double> ntab(size_t(ns1) * size_t(np1)), der(np1, 0.0);
    for (int k = 0; k < ns1; ++k)
      mi::lagrange_eval(dst->tab.nodes, (double(k / nq1) + dst->tab.qx[size_t(k % nq1)]) / double(sub), &ntab[size_t(k) * np1], der.data());
    // chunks: whole groups of cells inside one colour, the point scratch at or below 256 MiB
    const size_t per_point = size_t(dim) * 8 + size_t(n_which) * dim * 8 + 8 + 1;
    int64_t      chunk     = dst->project_chunk_cells > 0 ? dst->project_chunk_cells :
                                                            std::max<int64_t>(1, int64_t((size_t(256) << 20) / (size_t(pc) * per_point)));
    int64_t      largest   = 0;
    for (int col = 0; col < m.ncolours; ++col)
      largest = std::max(largest, m.colour_begin[col + 1] - m.colour_begin[col]);
    chunk            = std::min(chunk, std::max<int64_t>(largest, 1));
    const int64_t np = chunk * pc; // points of a full chunk
    const size_t  nx = size_t(np) * dim, nv = size_t(n_which) * nx, npart = size_t(mi::field_at_points_partials(np));
    const size_t  nsq = size_t(mi::PROJ_FIELDS) * size_t(m.ncells);
    DevBuf        w;
    HIPCHK(dst, hipMalloc(&w.p, (nx + nv + size_t(np) + npart + 1 + ntab.size() + nsq + mi::PROJ_FIELDS) * sizeof(double)));
    PeBuffers pb{};
    pb.xyz = w.d(), pb.values = pb.xyz + nx, pb.gradients = nullptr;
    pb.cell = reinterpret_cast<int64_t *>(pb.values + nv), pb.part = pb.values + nv + size_t(np), pb.count = pb.part + npart;
    double *d_ntab = pb.count + 1, *d_sq = d_ntab + ntab.size(), *d_sums = d_sq + nsq;
    HIPCHK(dst, hipMemcpyAsync(d_ntab, ntab.data(), ntab.size() * sizeof(double), hipMemcpyHostToDevice, dst->stream));
    HIPCHK(dst, hipMemsetAsync(d_b, 0, size_t(n_which) * size_t(dst->n) * sizeof(double), dst->stream));
    mi::ProjectParams pp{};
    pp.conn = dst->d_conn, pp.cverts = dst->d_cverts, pp.tab = dst->d_tab, pp.ntab = d_ntab, pp.values = pb.values;
    pp.b = d_b, pp.cell_sq = d_sq, pp.n = dst->n, pp.ncells = m.ncells, pp.n_which = n_which, pp.sub = sub;
    const double *d_qx = dst->d_tab + 2 * size_t(nq1) * np1 + nq1;
    for (int col = 0; col < m.ncolours; ++col)
      for (int64_t c0 = m.colour_begin[col]; c0 < m.colour_begin[col + 1]; c0 += chunk)
        {
          const int64_t nc = std::min(chunk, m.colour_begin[col + 1] - c0), npc = nc * pc;
          mi::launch_project_points(dim, dst->d_cverts, d_qx, c0, npc, nq1, sub, pb.xyz, dst->stream);
          HIPCHK(dst, hipGetLastError());
          HIPCHK(dst, hipStreamSynchronize(dst->stream)); // (the scratch is dst's stream's; the evaluation runs on src's)
          if (const int rc = enqueue_point_eval(src, n_which, which, npc, pb.xyz, pb, src->stream))
            return fail(dst, rc, "%s", src->err.c_str());
          HIPCHK(dst, hipStreamSynchronize(src->stream));
          double cnt = 0.0;
          HIPCHK(dst, hipMemcpy(&cnt, pb.count, sizeof(double), hipMemcpyDeviceToHost));
          if (cnt > 0.0)
            {
              std::vector<int64_t> cells(size_t(npc), 0);
              HIPCHK(dst, hipMemcpy(cells.data(), pb.cell, size_t(npc) * sizeof(int64_t), hipMemcpyDeviceToHost));
              int64_t first = 0;
              while (first < npc - 1 && cells[size_t(first)] >= 0)
                ++first;
              return fail(dst, MI_EINVAL, "projection: quadrature point %lld of dst's cell %lld lies outside src's mesh; dst is unchanged",
                          (long long)(first % pc), (long long)m.cell_orig[size_t(c0 + first / pc)]);
            }
          pp.npts = npc, pp.chunk_begin = c0, pp.cell_begin = c0, pp.cell_count = int32_t(nc);
          if (mi::launch_project_load(dim, dst->degree, pp, dst->stream))
            return fail(dst, MI_EINVAL, "no projection kernel for dim=%d degree=%d", dim, dst->degree);
        }
    mi::launch_project_sq_sum(d_sq, int(m.ncells), d_sums, dst->stream);
    HIPCHK(dst, hipGetLastError());
    double h[mi::PROJ_FIELDS];
    HIPCHK(dst, hipMemcpyAsync(h, d_sums, sizeof(h), hipMemcpyDeviceToHost, dst->stream));
    HIPCHK(dst, hipStreamSynchronize(dst->stream));
    for (int k = 0; k < n_which && src_sq; ++k)
      src_sq[k] = h[k];
    if (n_points)
      *n_points = m.ncells * pc;
    return MI_OK;
  }

  // the conditions the calls share: one slab that is its own team's
  static int mass_check(mi_ctx *c, const char *what, int nrhs, int masked)
  {
    if (nrhs < 0 || nrhs > mi::MASS_MAX_RHS)
      return fail(c, MI_EINVAL, "%s: nrhs %d (0..%d)", what, nrhs, mi::MASS_MAX_RHS);
    if (masked != 0 && masked != 1)
      return fail(c, MI_EINVAL, "%s: masked %d (0 or 1)", what, masked);
    if (!pe_undecomposed(c))
      return fail(c, MI_EINVAL, "%s: one slab only (an undecomposed mesh)", what);
    return MI_OK;
  }
  static int project_check(mi_ctx *dst, mi_ctx *src, const char *what, int sub)
  {
    if (dst->dim != src->dim)
      return fail(dst, MI_EINVAL, "%s: dst is %dD, src %dD", what, dst->dim, src->dim);
    if (dst->device != src->device)
      return fail(dst, MI_EINVAL, "%s: dst is on device %d, src on %d", what, dst->device, src->device);
    if (!pe_undecomposed(dst) || !pe_undecomposed(src))
      return fail(dst, MI_EINVAL, "%s: one slab only (undecomposed meshes)", what);
    if (sub < 1 || sub > mi::PROJ_MAX_SUB)
      return fail(dst, MI_EINVAL, "%s: sub %d (1..%d)", what, sub, mi::PROJ_MAX_SUB);
    return MI_OK;
  }
} // namespace mi_detail

extern "C" {

static_assert(MI_MASS_MAX_RHS == mi::MASS_MAX_RHS && mi::PROJ_FIELDS == 6, "the kernels' column count is the header's");

int mi_mass_apply(mi_ctx *c, int nrhs, int masked, const double *x, double *y)
{
  if (!c)
    return MI_EINVAL;
  if (int rc = mass_check(c, "mi_mass_apply", nrhs, masked))
    return rc;
  if (nrhs == 0)
    return MI_OK;
  if (!x || !y)
    return fail(c, MI_EINVAL, "mi_mass_apply: null argument");
  HIPCHK(c, hipSetDevice(c->device));
  const size_t blk = size_t(nrhs) * size_t(c->n);
  DevBuf       w;
  HIPCHK(c, hipMalloc(&w.p, 2 * blk * sizeof(double)));
  HIPCHK(c, hipMemcpyAsync(w.d(), x, blk * sizeof(double), hipMemcpyHostToDevice, c->stream));
  if (int rc = enqueue_mass_apply(c, nrhs, masked, false, w.d(), w.d() + blk))
    return rc;
  HIPCHK(c, hipMemcpyAsync(y, w.d() + blk, blk * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return MI_OK;
}

int mi_mass_solve(mi_ctx *c, int nrhs, int masked, const double *b, double *x, double tol, int max_it, int *its, double *res)
{
  if (!c)
    return MI_EINVAL;
  if (int rc = mass_check(c, "mi_mass_solve", nrhs, masked))
    return rc;
  if (!(tol >= 0.0) || max_it < 0)
    return fail(c, MI_EINVAL, "mi_mass_solve: tol %g, max_it %d", tol, max_it);
  if (its)
    *its = 0;
  if (nrhs == 0)
    return MI_OK;
  if (!b || !x)
    return fail(c, MI_EINVAL, "mi_mass_solve: null argument");
  HIPCHK(c, hipSetDevice(c->device));
  const size_t blk = size_t(nrhs) * size_t(c->n);
  DevBuf       w;
  HIPCHK(c, hipMalloc(&w.p, 2 * blk * sizeof(double)));
  HIPCHK(c, hipMemcpyAsync(w.d(), b, blk * sizeof(double), hipMemcpyHostToDevice, c->stream));
  const int rc = mass_solve_device(c, nrhs, masked, w.d(), w.d() + blk, tol, max_it, its, res, nullptr);
  if (rc != MI_OK && rc != MI_ENOCONV_LIN)
    return rc;
  HIPCHK(c, hipMemcpyAsync(x, w.d() + blk, blk * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return rc;
}

int mi_project_load(mi_ctx *dst, mi_ctx *src, int n_which, const int *which, int sub, double *b)
{
  if (!dst || !src)
    return dst ? fail(dst, MI_EINVAL, "mi_project_load: null argument") : MI_EINVAL;
  if (int rc = project_check(dst, src, "mi_project_load", sub))
    return rc;
  if (n_which < 0 || n_which > mi::PROJ_FIELDS)
    return fail(dst, MI_EINVAL, "mi_project_load: n_which %d (0..%d)", n_which, mi::PROJ_FIELDS);
  if (n_which == 0)
    return MI_OK;
  if (!which || !b)
    return fail(dst, MI_EINVAL, "mi_project_load: null argument");
  for (int w = 0; w < n_which; ++w)
    if (which[w] < 0 || which[w] >= MI_V_COUNT)
      return fail(dst, MI_EINVAL, "mi_project_load: bad vector id %d", which[w]);
  HIPCHK(dst, hipSetDevice(dst->device));
  const size_t blk = size_t(n_which) * size_t(dst->n);
  DevBuf       w;
  HIPCHK(dst, hipMalloc(&w.p, blk * sizeof(double)));
  if (int rc = project_load_device(dst, src, n_which, which, sub, w.d(), nullptr, nullptr))
    return rc;
  HIPCHK(dst, hipMemcpy(b, w.d(), blk * sizeof(double), hipMemcpyDeviceToHost));
  return MI_OK;
}

int mi_state_project(mi_ctx *dst, mi_ctx *src, int sub, double tol, int max_it, mi_project_info *out)
{
  if (!dst || !src)
    return dst ? fail(dst, MI_EINVAL, "mi_state_project: null argument") : MI_EINVAL;
  if (int rc = project_check(dst, src, "mi_state_project", sub))
    return rc;
  if (!(tol >= 0.0) || max_it < 0)
    return fail(dst, MI_EINVAL, "mi_state_project: tol %g, max_it %d", tol, max_it);
  HIPCHK(dst, hipSetDevice(dst->device));
  const size_t n = size_t(dst->n), blk = 6 * n, nblk = size_t(mi::mass_chunks(dst->n));
  DevBuf       w;
  HIPCHK(dst, hipMalloc(&w.p, (2 * blk + 6 * nblk + 6) * sizeof(double)));
  double *B = w.d(), *X = B + blk, *part = X + blk, *sums = part + 6 * nblk;
  mi_project_info info{};
  info.sub = sub;
  int rc = project_load_device(dst, src, 6, project_six, sub, B, info.src_sq, &info.n_points);
  if (rc)
    return rc;
  int    its = 0;
  double res[6];
  rc       = mass_solve_device(dst, 6, 1, B, X, tol, max_it, &its, res, nullptr);
  info.its = its;
  if (rc == MI_OK || rc == MI_ENOCONV_LIN)
    for (int j = 0; j < 6; ++j)
      info.res = std::max(info.res, res[j]);
  if (rc == MI_OK)
    {
      // w^T M w of what was found (B is free), then the six vectors: the first six of d_vecs in the order of project_six
      if (int r2 = enqueue_mass_apply(dst, 6, 1, false, X, B))
        return r2;
      mi::launch_mass_col_dots(X, B, dst->n, 6, part, sums, dst->stream);
      HIPCHK(dst, hipGetLastError());
      HIPCHK(dst, hipMemcpyAsync(info.dst_sq, sums, 6 * sizeof(double), hipMemcpyDeviceToHost, dst->stream));
      HIPCHK(dst, hipMemcpyAsync(dst->d_vecs, X, blk * sizeof(double), hipMemcpyDeviceToDevice, dst->stream));
      HIPCHK(dst, hipStreamSynchronize(dst->stream));
    }
  if (out)
    *out = info;
  return rc;
}

} // extern "C"
