// Explicit central differences for the neo-Hookean solid: mi_explicit_setup, mi_explicit_run, mi_explicit_get_mass,
// mi_explicit_stable_dt.  Part of mi_ctx.cpp's translation unit (included at its end, after mi_project.cpp).
//
// Velocity-Verlet form with the lumped mass m_i = rho W_i, W = M 1 the row sums of the unit-density consistent mass of
// mi_mass_apply (rule QGauss(p + 2)).  A step is the residual-only pass of the context (whichever pass its keys select) at
// u + du with a zero acceleration field, then explicit_advance: no tangent, no solve, no host synchronisation; the one decision
// of a step (a folded cell) is taken on the device.  One slab only.

namespace mi_detail
{
  struct ExplicitBufs
  {
    double *mass, *minv, *zero, *part, *words; // words: [0] first folded step of a run (0: none), [1] sum m v^2, [2], [3] Lanczos scalars
  };
  static ExplicitBufs explicit_bufs(mi_ctx *c)
  {
    const size_t n2 = (size_t(c->n) + 1) & ~size_t(1); // every array on a 16-byte boundary
    double      *d  = c->d_explicit;
    return ExplicitBufs{d, d + n2, d + 2 * n2, d + 3 * n2, d + 3 * n2 + MAX_PART};
  }
  static const char *explicit_refusal(mi_ctx *c, const char *name)
  {
    static thread_local char buf[128];
    if (!c->team || team_size(c) != 1 || c->team->members[0] != c)
      {
        snprintf(buf, sizeof(buf), "%s: one slab only (an undecomposed mesh)", name);
        return buf;
      }
    return nullptr;
  }
  // the lumped masses and the zero vector, formed by the first call that needs them (they depend on the mesh and the density alone)
  static int explicit_ensure_masses(mi_ctx *c)
  {
    if (c->d_explicit)
      return MI_OK;
    const size_t n2 = (size_t(c->n) + 1) & ~size_t(1);
    DevBuf       w; // ones | M 1
    HIPCHK(c, hipMalloc(&w.p, 2 * n2 * sizeof(double)));
    std::vector<double> ones(size_t(c->n), 1.0);
    HIPCHK(c, hipMemcpy(w.d(), ones.data(), ones.size() * sizeof(double), hipMemcpyHostToDevice));
    double *d = nullptr;
    HIPCHK(c, hipMalloc((void **)&d, (3 * n2 + MAX_PART + 4) * sizeof(double)));
    hipError_t e = hipMemsetAsync(d, 0, (3 * n2 + MAX_PART + 4) * sizeof(double), c->stream);
    int        rc = e == hipSuccess ? enqueue_mass_apply(c, 1, 0, false, w.d(), w.d() + n2) : fail(c, MI_EHIP, "hipMemsetAsync failed");
    if (!rc)
      {
        mi::launch_explicit_masses(c->dim, w.d() + n2, c->d_cmask, c->mat.rho, d, d + n2, c->n, c->stream);
        e = hipGetLastError();
        if (e == hipSuccess)
          e = hipStreamSynchronize(c->stream);
        if (e != hipSuccess)
          rc = fail(c, MI_EHIP, "explicit_masses failed: %s", hipGetErrorString(e));
      }
    if (rc)
      {
        hipFree(d);
        return rc;
      }
    c->d_explicit = d;
    return MI_OK;
  }
  static mi::ExplicitParams explicit_params(mi_ctx *c, const ExplicitBufs &b)
  {
    mi::ExplicitParams p{};
    p.u = c->vec(MI_V_TOTAL_DISPLACEMENT), p.v = c->vec(MI_V_VELOCITY), p.a = c->vec(MI_V_ACCELERATION);
    p.du = c->vec(MI_V_SOLUTION_DELTA), p.F = c->vec(MI_V_SYSTEM_RHS), p.minv = b.minv;
    p.inverted = c->d_sc + SC_INVERTED, p.stop = b.words;
    p.dt = c->explicit_dt, p.n = c->n;
    return p;
  }
  static const char *INVERTED_TEXT = "inverted element: det F <= 0 at a quadrature point";

  // the largest eigenvalue of the symmetric tridiagonal matrix (alpha, beta) by bisection on its Sturm sequence
  static double tridiagonal_largest(const std::vector<double> &alpha, const std::vector<double> &beta)
  {
    const size_t k = alpha.size();
    double       lo = alpha[0], hi = alpha[0];
    for (size_t j = 0; j < k; ++j)
      {
        const double r = (j > 0 ? std::fabs(beta[j - 1]) : 0.0) + (j + 1 < k ? std::fabs(beta[j]) : 0.0);
        lo = std::min(lo, alpha[j] - r), hi = std::max(hi, alpha[j] + r);
      }
    auto below = [&](double x) { // eigenvalues < x
      size_t cnt = 0;
      double d   = 1.0;
      for (size_t j = 0; j < k; ++j)
        {
          const double b2 = j > 0 ? beta[j - 1] * beta[j - 1] : 0.0;
          d               = alpha[j] - x - (j > 0 ? b2 / d : 0.0);
          if (d == 0.0)
            d = -1e-300;
          cnt += d < 0.0;
        }
      return cnt;
    };
    for (int it = 0; it < 200; ++it)
      {
        const double mid = 0.5 * (lo + hi);
        if (!(mid > lo && mid < hi))
          break;
        if (below(mid) >= k)
          hi = mid;
        else
          lo = mid;
      }
    return hi;
  }
} // namespace mi_detail

extern "C" {

int mi_explicit_setup(mi_ctx *c, double dt, int init_acceleration)
{
  if (!c)
    return MI_EINVAL;
  if (const char *why = explicit_refusal(c, "mi_explicit_setup"))
    return fail(c, MI_EINVAL, "%s", why);
  if (!(dt > 0.0) || !std::isfinite(dt) || (init_acceleration != 0 && init_acceleration != 1))
    return fail(c, MI_EINVAL, "mi_explicit_setup: dt > 0 and init_acceleration 0 or 1 are required");
  if (int e = check_tangent_array(c, "mi_explicit_setup"))
    return e;
  HIPCHK(c, hipSetDevice(c->device));
  if (int rc = explicit_ensure_masses(c))
    return rc;
  const ExplicitBufs b = explicit_bufs(c);
  if (c->linear) // after mi_linear_setup: the tangent's side of the context, as mi_tangent_modes selects it
    linear_select(c, -1);
  if (init_acceleration)
    {
      HIPCHK(c, hipMemsetAsync(c->vec(MI_V_SOLUTION_DELTA), 0, size_t(c->n) * sizeof(double), c->stream));
      if (int rc = enqueue_assembly(c, true, b.zero, c->explicit_force_only != 0))
        return rc;
      HIPCHK(c, hipMemcpyAsync(c->h_pinned, c->d_sc + SC_INVERTED, sizeof(double), hipMemcpyDeviceToHost, c->stream));
      if (int rc = sync(c))
        return rc;
      if (c->h_pinned[0] > 0.0)
        return fail(c, MI_EINVAL, "%s (mi_explicit_setup: the committed state has folded a cell; no acceleration was written)", INVERTED_TEXT);
      mi::launch_vec_scale_mul(c->vec(MI_V_ACCELERATION), b.minv, c->vec(MI_V_SYSTEM_RHS), 1.0, c->n, c->stream);
      HIPCHK(c, hipGetLastError());
      HIPCHK(c, hipMemcpyAsync(c->vec(MI_V_ACCELERATION_OLD), c->vec(MI_V_ACCELERATION), size_t(c->n) * sizeof(double),
                               hipMemcpyDeviceToDevice, c->stream));
      if (int rc = sync(c))
        return rc;
    }
  c->explicit_dt = dt;
  return MI_OK;
}

int mi_explicit_run(mi_ctx *c, int n_steps, mi_explicit_info *info)
{
  if (!c)
    return MI_EINVAL;
  if (const char *why = explicit_refusal(c, "mi_explicit_run"))
    return fail(c, MI_EINVAL, "%s", why);
  if (!info || n_steps < 0)
    return fail(c, MI_EINVAL, "mi_explicit_run: null info or n_steps < 0");
  if (!(c->explicit_dt > 0.0) || !c->d_explicit)
    return fail(c, MI_EINVAL, "mi_explicit_run: mi_explicit_setup has not been called");
  if (int e = check_tangent_array(c, "mi_explicit_run"))
    return e;
  HIPCHK(c, hipSetDevice(c->device));
  const ExplicitBufs b = explicit_bufs(c);
  mi::ExplicitParams p = explicit_params(c, b);
  int                enqueued = 0, rc_pass = MI_OK; // a pass that cannot be enqueued ends the run after the steps before it
  if (n_steps > 0)
    {
      mi::launch_explicit_start(p, c->stream);
      for (int k = 1; k <= n_steps && !rc_pass; ++k)
        {
          if ((rc_pass = enqueue_assembly(c, true, b.zero, c->explicit_force_only != 0)))
            break;
          p.step = k;
          mi::launch_explicit_advance(p, c->stream);
          enqueued = k;
        }
    }
  else
    HIPCHK(c, hipMemsetAsync(b.words, 0, sizeof(double), c->stream));
  mi::launch_explicit_finish(n_steps > 0, newmark_params(c), b.mass, c->vec(MI_V_SOLUTION_DELTA), b.part, c->grid_vec, b.words + 1, c->stream);
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipMemcpyAsync(c->h_pinned, b.words, 2 * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  if (int rc = sync(c))
    return rc;
  const int folded     = int(c->h_pinned[0]);
  info->steps_done     = folded ? folded - 1 : enqueued;
  info->inverted_step  = folded ? folded : -1;
  info->dt             = c->explicit_dt;
  info->kinetic_lumped = 0.5 * c->h_pinned[1];
  if (rc_pass) // (the state is the committed one after info->steps_done steps, *_OLD and the delta as after any run; c->err is the pass's)
    return rc_pass;
  if (folded)
    return fail(c, MI_EINVAL, "%s at explicit step %d (the state is that after step %d; the reference asserts det F > 0, "
                              "nonlinear_elasticity.cc:935)", INVERTED_TEXT, folded, folded - 1);
  return MI_OK;
}

int mi_explicit_get_mass(mi_ctx *c, double *m)
{
  if (!c)
    return MI_EINVAL;
  if (const char *why = explicit_refusal(c, "mi_explicit_get_mass"))
    return fail(c, MI_EINVAL, "%s", why);
  if (!m)
    return fail(c, MI_EINVAL, "mi_explicit_get_mass: null argument");
  HIPCHK(c, hipSetDevice(c->device));
  if (int rc = explicit_ensure_masses(c))
    return rc;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  HIPCHK(c, hipMemcpy(m, explicit_bufs(c).mass, size_t(c->n) * sizeof(double), hipMemcpyDeviceToHost));
  return MI_OK;
}

int mi_explicit_stable_dt(mi_ctx *c, int krylov_steps, double *lambda_max, double *dt_crit)
{
  if (!c)
    return MI_EINVAL;
  if (const char *why = explicit_refusal(c, "mi_explicit_stable_dt"))
    return fail(c, MI_EINVAL, "%s", why);
  if (!lambda_max || !dt_crit || krylov_steps < 1)
    return fail(c, MI_EINVAL, "mi_explicit_stable_dt: null argument or krylov_steps < 1");
  if (int e = check_tangent_array(c, "mi_explicit_stable_dt"))
    return e;
  HIPCHK(c, hipSetDevice(c->device));
  if (int rc = explicit_ensure_masses(c))
    return rc;
  // the tangent at the committed state, as tangent_prepare forms it; the hierarchy is left alone (and marked stale)
  if (c->linear)
    linear_select(c, -1);
  c->active_sell_vals = nullptr;
  c->active_dinv      = nullptr;
  HIPCHK(c, hipMemsetAsync(c->vec(MI_V_SOLUTION_DELTA), 0, size_t(c->n) * sizeof(double), c->stream));
  HIPCHK(c, hipMemsetAsync(c->vec(MI_V_NEWTON_UPDATE), 0, size_t(c->n) * sizeof(double), c->stream));
  c->newton_update_is_zero = true;
  c->mf_diag_fresh         = false;
  if (int rc = assemble_impl(c, false, nullptr))
    return rc;
  if (int rc = check_mf_tangent(c))
    return rc;
  int64_t n_free = 0;
  for (int64_t nd = 0; nd < c->mesh.nnodes; ++nd)
    for (int k = 0; k < c->dim; ++k)
      n_free += !((c->mesh.cmask[size_t(nd)] >> k) & 1);
  if (n_free < 1)
    return fail(c, MI_EINVAL, "mi_explicit_stable_dt: no free dof");
  const int          steps = int(std::min<int64_t>(krylov_steps, n_free));
  const ExplicitBufs b     = explicit_bufs(c);
  const size_t       n     = size_t(c->n);
  DevBuf             w; // q | q_prev | y | M q | rho M q
  HIPCHK(c, hipMalloc(&w.p, 5 * n * sizeof(double)));
  double *q = w.d(), *qp = q + n, *y = qp + n, *mx = y + n, *ms = mx + n;
  const double rho = c->mat.rho, shift = c->alpha[1] * rho;
  // sum m x^2 of a vector that is zero on constrained dofs: its squared norm in the lumped-mass inner product
  auto mnorm2 = [&](const double *x, double *out) -> int {
    mi::launch_weighted_sq(b.mass, x, c->n, b.part, c->grid_vec, b.words + 2, c->stream);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(c->h_pinned, b.words + 2, sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    *out = c->h_pinned[0];
    return MI_OK;
  };
  mi::launch_block_hash_init(c->dim, y, c->n, 1, c->d_cmask, c->n, c->stream); // the fixed start vector of the eigensolvers
  double nrm2 = 0;
  if (int rc = mnorm2(y, &nrm2))
    return rc;
  if (!(nrm2 > 0.0))
    return fail(c, MI_EINVAL, "mi_explicit_stable_dt: the start vector vanished");
  mi::launch_vec_scale_mul(q, y, nullptr, 1.0 / std::sqrt(nrm2), c->n, c->stream);
  std::vector<double> alpha, beta;
  for (int j = 0; j < steps; ++j)
    {
      // y = K_T q = A q - alpha_1 rho M q on the free dofs (tangent_images), A the context's own operator
      if (int rc = enqueue_mass_apply(c, 1, 1, false, q, mx))
        return rc;
      enqueue_spmv(c, q, y, nullptr, nullptr, nullptr);
      mi::launch_tangent_images(c->dim, y, mx, ms, c->d_cmask, shift, rho, c->n, 1, c->stream);
      mi::launch_dot_partials(q, y, c->n, b.part, c->grid_vec, c->stream);
      mi::launch_finish_sum(b.part, c->grid_vec, b.words + 3, c->stream);
      HIPCHK(c, hipGetLastError());
      HIPCHK(c, hipMemcpyAsync(c->h_pinned, b.words + 3, sizeof(double), hipMemcpyDeviceToHost, c->stream));
      HIPCHK(c, hipStreamSynchronize(c->stream));
      alpha.push_back(c->h_pinned[0]);
      if (j + 1 == steps)
        break;
      mi::launch_lanczos_update(y, b.minv, q, j > 0 ? qp : nullptr, alpha.back(), j > 0 ? beta.back() : 0.0, c->n, c->stream);
      if (int rc = mnorm2(y, &nrm2))
        return rc;
      if (!(nrm2 > 0.0) || !std::isfinite(nrm2)) // an invariant subspace: the Ritz values so far are eigenvalues
        break;
      beta.push_back(std::sqrt(nrm2));
      std::swap(q, qp);
      mi::launch_vec_scale_mul(q, y, nullptr, 1.0 / beta.back(), c->n, c->stream);
    }
  HIPCHK(c, hipStreamSynchronize(c->stream));
  beta.resize(alpha.size() - 1);
  const double theta = tridiagonal_largest(alpha, beta);
  *lambda_max        = theta;
  if (!(theta > 0.0) || !std::isfinite(theta))
    return fail(c, MI_EINVAL, "mi_explicit_stable_dt: the largest Ritz value %g is not positive", theta);
  *dt_crit = 2.0 / std::sqrt(theta);
  return MI_OK;
}

} // extern "C"
