// mi_modes.cpp -- the lowest vibration modes of the linear model:  K phi = lambda M phi  on the free dofs (mi_linear_modes), and of
// the nonlinear model's tangent at the committed state:  K_T(u) phi = lambda rho M phi  (mi_tangent_modes).  One eigensolver over
// an operator pair: the two entry points differ in products() and in where the preconditioner comes from.
// Compiled as part of mi_linear.cpp's translation unit (included at its end), not as an object of its own.
//
// The tangent's pair.  The context holds A = K_T + alpha_1 rho M (what mi_assemble forms and the Newmark step's CG solves with), in
// whichever form it runs: assembled (sell_spmv / sell_spmv_split) or matrix-free (mf_spmv, mf_spmv_q3 + their gathers).  K_T x is
// formed as A x - alpha_1 rho (M x), M x from enqueue_mass_apply (masked, six columns per launch group); that difference carries
// a rounding floor of order eps alpha_1 / |lambda| relative to |lambda| |rho M x| (1e-11 at worst in the tested cases), which
// the stopping tolerance must stay above.  The preconditioner is the context's own for A -- the tangent's V-cycle or the
// Jacobi diagonal of the assembly -- and needs A positive definite, lambda_min > -alpha_1: the condition of the step's CG.
//
// LOBPCG (Knyazev 2001) on a block of m = n_modes + guard vectors.  The device holds S = [X W P] and its images KS, MS
// (9 m n doubles, allocated per call; the tangent's pair one block more for M x); the host sees only Gram matrices.  One iteration:
//
//   R = KX - MX diag(lambda), masked, with |R_j| and |MX_j| of the same pass        block_residual            (1 launch + finish)
//   W_j = T R_j, masked; T = the preconditioner the current set-up has for the stepping matrix A = M + theta^2 dt^2 K
//       = (theta dt)^2 (K + sigma M): 1 / diag(A), or one multigrid V-cycle                                   (m applications)
//   W -= X (MX^T W): the search directions M-orthogonal to the iterates                block_gram + block_combine
//   KW, MW                                                                              (2 m products, one vector at a time)
//   S^T K S, S^T M S                                                                     block_gram              (2 launches + finish)
//   Rayleigh-Ritz on the host: columns scaled to unit M-norm, Cholesky of the scaled S^T M S, cyclic Jacobi
//   X <- S C, P <- [W P] C_WP, the same for KS and MS                                   block_combine           (6 launches)
//
// block_combine works row-wise in place (a thread holds its row of S before it writes), which is what lets the three blocks
// live in 9 m n doubles.  KX and MX follow by recurrence; before the call returns they are formed afresh and X is
// Rayleigh-Ritz'ed on its own, so that the returned pairs, their residuals and their orthonormality do not carry the
// recurrence's rounding.
//
// If the Cholesky factor meets a pivot below CHOL_MIN (the scaled Gram matrix is numerically singular: P has run into the span
// of X and W) the iteration is repeated without P; if it fails again X is re-orthonormalised and P restarted.
//
// The tangent's pair runs every Rayleigh-Ritz step of the iteration in another form (rayleigh_ritz with drop): the columns that
// depend on those before them are left out, and the problem is solved in two passes.  mi_linear_modes never takes that form.  Its preconditioner approximates (K_T + sigma
// rho M)^-1 with sigma = alpha_1 far above the wanted lambda, so T R_j lies almost inside span X and what is left after the
// projection is small and noisy: W and P run close to X and to each other long before convergence.  Dropping all of P at a
// pivot of 1e-8 then happens in most iterations and leaves block steepest descent at a rate of 1 - gap / sigma (2400 iterations
// on the 3 x 1 x 1 Q2 beam at u = 0 with the V-cycle, or none at all), and a one-pass solve at smaller pivots returns spurious
// Ritz values.  With the second pass that case takes 45 iterations, as its neighbours do.
#include <algorithm>
#include <cmath>

#include "mi_internal.h"

using namespace mi_detail;

namespace
{
  constexpr double CHOL_MIN = 1e-8; // smallest pivot (squared distance of a unit column from the span of those before it)

  // A v = w B v, dense symmetric A, SPD B, row-major n x n (symmetric: the order is immaterial).  Cholesky B = L L^T,
  // C = L^-1 A L^-T, cyclic Jacobi on C, V = L^-T Q; w ascending, V column-major (eigenvector j at V + j n), V^T B V = I.
  // Returns 1 where a pivot of the factor is not above min_pivot
  int dense_sym_eig(int n, const double *A, const double *B, double *w, double *V, double min_pivot)
  {
    const size_t        N = size_t(n);
    std::vector<double> L(N * N, 0.0), C(N * N), Q(N * N, 0.0);
    for (int i = 0; i < n; ++i)
      for (int j = 0; j <= i; ++j)
        {
          double s = 0.5 * (B[i * N + j] + B[j * N + i]);
          for (int k = 0; k < j; ++k)
            s -= L[i * N + k] * L[j * N + k];
          if (i == j)
            {
              if (!(s > min_pivot))
                return 1;
              L[i * N + i] = std::sqrt(s);
            }
          else
            L[i * N + j] = s / L[j * N + j];
        }
    // Y = L^-1 A (column by column), C = Y L^-T = (L^-1 Y^T)^T
    for (int c = 0; c < n; ++c)
      for (int i = 0; i < n; ++i)
        {
          double s = 0.5 * (A[i * N + c] + A[c * N + i]);
          for (int k = 0; k < i; ++k)
            s -= L[i * N + k] * C[k * N + c];
          C[i * N + c] = s / L[i * N + i];
        }
    for (int r = 0; r < n; ++r) // row r of Y := L^-1 (row r of Y)^T
      for (int i = 0; i < n; ++i)
        {
          double s = C[r * N + i];
          for (int k = 0; k < i; ++k)
            s -= L[i * N + k] * C[r * N + k];
          C[r * N + i] = s / L[i * N + i];
        }
    for (int i = 0; i < n; ++i)
      for (int j = 0; j < i; ++j)
        C[i * N + j] = C[j * N + i] = 0.5 * (C[i * N + j] + C[j * N + i]);
    for (int i = 0; i < n; ++i)
      Q[i * N + i] = 1.0;
    // cyclic Jacobi (Rutishauser's rotations): Q^T C Q -> diagonal, Q row-major with the eigenvectors in its columns
    for (int sweep = 0; sweep < 64; ++sweep)
      {
        double off = 0.0, all = 0.0;
        for (int i = 0; i < n; ++i)
          for (int j = 0; j < n; ++j)
            (i == j ? all : off) += C[i * N + j] * C[i * N + j];
        all += off;
        if (off <= 1e-33 * all || off == 0.0)
          break;
        for (int p = 0; p < n - 1; ++p)
          for (int q = p + 1; q < n; ++q)
            {
              const double apq = C[p * N + q];
              if (apq == 0.0)
                continue;
              const double th = (C[q * N + q] - C[p * N + p]) / (2.0 * apq);
              const double t  = (th >= 0 ? 1.0 : -1.0) / (std::fabs(th) + std::sqrt(th * th + 1.0));
              const double cs = 1.0 / std::sqrt(t * t + 1.0), sn = t * cs;
              for (int k = 0; k < n; ++k)
                {
                  const double kp = C[k * N + p], kq = C[k * N + q];
                  C[k * N + p] = cs * kp - sn * kq;
                  C[k * N + q] = sn * kp + cs * kq;
                }
              for (int k = 0; k < n; ++k)
                {
                  const double pk = C[p * N + k], qk = C[q * N + k];
                  C[p * N + k] = cs * pk - sn * qk;
                  C[q * N + k] = sn * pk + cs * qk;
                }
              C[p * N + q] = C[q * N + p] = 0.0;
              for (int k = 0; k < n; ++k)
                {
                  const double kp = Q[k * N + p], kq = Q[k * N + q];
                  Q[k * N + p] = cs * kp - sn * kq;
                  Q[k * N + q] = sn * kp + cs * kq;
                }
            }
      }
    std::vector<int> order(N);
    for (int i = 0; i < n; ++i)
      order[size_t(i)] = i;
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return C[a * N + a] < C[b * N + b]; });
    for (int j = 0; j < n; ++j)
      {
        const int src = order[size_t(j)];
        w[j]          = C[src * N + src];
        double *v     = V + size_t(j) * N;
        for (int i = n - 1; i >= 0; --i) // L^T v = q
          {
            double s = Q[i * N + src];
            for (int k = i + 1; k < n; ++k)
              s -= L[k * N + i] * v[k];
            v[i] = s / L[i * N + i];
          }
      }
    return 0;
  }

  // The columns of the symmetric n x n matrix B that a Cholesky factorisation accepts, taken in order: a column whose pivot against
  // the accepted ones before it is not above min_pivot is left out
  std::vector<int> independent_columns(int n, const double *B, double min_pivot)
  {
    const size_t                     N = size_t(n);
    std::vector<int>                 keep;
    std::vector<std::vector<double>> L; // row k: the factor's row of keep[k]
    for (int i = 0; i < n; ++i)
      {
        std::vector<double> row(keep.size() + 1);
        double              s = B[i * N + i];
        for (size_t k = 0; k < keep.size(); ++k)
          {
            double t = 0.5 * (B[i * N + size_t(keep[k])] + B[size_t(keep[k]) * N + i]);
            for (size_t q = 0; q < k; ++q)
              t -= row[q] * L[k][q];
            row[k] = t / L[k][k];
            s -= row[k] * row[k];
          }
        if (!(s > min_pivot))
          continue;
        row[keep.size()] = std::sqrt(s);
        L.push_back(row);
        keep.push_back(i);
      }
    return keep;
  }

  // what a call of mi_linear_modes / mi_tangent_modes holds on the device
  struct Blocks
  {
    mi_ctx     *c = nullptr;
    int64_t     n = 0;
    int         m = 0;
    const char *name    = "mi_linear_modes";
    bool        tangent = false; // the pair (K_T, rho M) of the nonlinear model, else (K, M) of the linear model
    double      rho = 1.0, shift = 0.0; // tangent: density; alpha_1 rho, the mass term inside the context's tangent
    double *S = nullptr, *KS = nullptr, *MS = nullptr; // [X W P], each block m columns of n
    double *MX = nullptr;                              // tangent: M x of the m columns of one products() call (unit density)
    double *part = nullptr, *gram = nullptr, *coef = nullptr, *sums = nullptr;
    ~Blocks()
    {
      for (double *p : {S, part, gram, coef, sums})
        if (p)
          hipFree(p);
    }
    double *W(double *b) const { return b + size_t(m) * size_t(n); }
  };

  // y = K x (0) or M x (1), zero on the constrained dofs; one vector through the product of the current set-up
  void product(mi_ctx *c, int which, const double *x, double *y)
  {
    linear_select(c, which);
    enqueue_spmv(c, x, y, nullptr, nullptr, nullptr);
    mi::launch_zero_constrained(c->dim, y, c->d_cmask, c->n, c->stream);
  }
  // the images of the m columns from col0 on.  Tangent: M x six columns at a time; A x_j through enqueue_spmm; K_T x_j = A x_j -
  // alpha_1 rho M x_j, zeroed on the constrained dofs, and rho M x_j (tangent_images)
  int products(const Blocks &b, size_t col0)
  {
    mi_ctx      *c = b.c;
    const size_t n = size_t(b.n);
    if (!b.tangent)
      {
        for (int j = 0; j < b.m; ++j)
          for (int w = 0; w < 2; ++w)
            product(c, w, b.S + (col0 + size_t(j)) * n, (w ? b.MS : b.KS) + (col0 + size_t(j)) * n);
        return MI_OK;
      }
    for (int j0 = 0; j0 < b.m; j0 += mi::MASS_MAX_RHS)
      if (int rc = enqueue_mass_apply(c, std::min(mi::MASS_MAX_RHS, b.m - j0), 1, false, b.S + (col0 + size_t(j0)) * n, b.MX + size_t(j0) * n))
        return rc;
    // A x of the block: sell_spmm where the context is eligible and "modes_block_product" allows it, else column by column (the
    // same bits either way); then both images of all columns in one pass
    enqueue_spmm(c, b.m, b.S + col0 * n, b.n, b.KS + col0 * n, b.n, c->modes_block_product != 0);
    mi::launch_tangent_images(c->dim, b.KS + col0 * n, b.MX, b.MS + col0 * n, c->d_cmask, b.shift, b.rho, c->n, b.m, c->stream);
    HIPCHK(c, hipGetLastError());
    return MI_OK;
  }

  // host <- a^T b of the first ka / kb columns
  int gram(const Blocks &b, const double *a, int ka, const double *bb, int kb, std::vector<double> &out)
  {
    mi_ctx *c = b.c;
    mi::launch_block_gram(a, ka, b.n, bb, kb, b.n, b.n, b.part, b.gram, c->stream);
    HIPCHK(c, hipGetLastError());
    out.resize(size_t(ka) * size_t(kb));
    HIPCHK(c, hipMemcpyAsync(out.data(), b.gram, out.size() * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return MI_OK;
  }

  // y <- src coef for the three images; coef [ks][my] row-major on the host
  int combine3(const Blocks &b, size_t src_col, int ks, const std::vector<double> &coef, int my, size_t dst_col)
  {
    mi_ctx *c = b.c;
    HIPCHK(c, hipMemcpyAsync(b.coef, coef.data(), size_t(ks) * my * sizeof(double), hipMemcpyHostToDevice, c->stream));
    for (double *base : {b.S, b.KS, b.MS})
      mi::launch_block_combine(base + src_col * size_t(b.n), ks, b.n, b.coef, my, base + dst_col * size_t(b.n), b.n, b.n, c->stream);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipStreamSynchronize(c->stream)); // (the host vector behind the copy may go away)
    return MI_OK;
  }

  // Rayleigh-Ritz on the leading ks columns: the m lowest pairs of (S^T K S, S^T M S) after scaling the columns to unit
  // M-norm.  C [ks][m] row-major.  1: the scaled Gram matrix is numerically singular.
  // drop: columns that depend on those before them (independent_columns) are left out of the problem, their rows of C zero (1
  // where fewer than m remain), and the problem is solved in two passes: a Gram matrix formed once on an ill-conditioned basis
  // carries an error of eps |K|_S / pivot into the Ritz values, so the kept columns are first M-orthonormalised on the device by
  // the factor of their Gram matrix, and the Gram matrices formed again on that basis (the CholeskyQR2 idea)
  int rayleigh_ritz(const Blocks &b, int ks, double min_pivot, std::vector<double> &lam, std::vector<double> &C, int *status,
                    bool drop = false)
  {
    std::vector<double> gk, gm;
    if (int rc = gram(b, b.S, ks, b.KS, ks, gk))
      return rc;
    if (int rc = gram(b, b.S, ks, b.MS, ks, gm))
      return rc;
    const size_t        K = size_t(ks);
    std::vector<double> d(K), w(K), V(K * K);
    *status = 1;
    for (size_t i = 0; i < K; ++i)
      {
        if (!(gm[i * K + i] > 0.0) || !std::isfinite(gm[i * K + i]))
          return MI_OK;
        d[i] = 1.0 / std::sqrt(gm[i * K + i]);
      }
    for (size_t i = 0; i < K; ++i)
      for (size_t j = 0; j < K; ++j)
        {
          gk[i * K + j] *= d[i] * d[j];
          gm[i * K + j] *= d[i] * d[j];
        }
    std::vector<int> keep(K);
    for (size_t i = 0; i < K; ++i)
      keep[i] = int(i);
    if (drop)
      {
        keep = independent_columns(ks, gm.data(), min_pivot);
        if (int(keep.size()) < b.m)
          return MI_OK;
        const size_t        R = keep.size();
        std::vector<double> rk(R * R), rm(R * R);
        for (size_t i = 0; i < R; ++i)
          for (size_t j = 0; j < R; ++j)
            {
              rk[i * R + j] = gk[size_t(keep[i]) * K + size_t(keep[j])];
              rm[i * R + j] = gm[size_t(keep[i]) * K + size_t(keep[j])];
            }
        gk.swap(rk), gm.swap(rm);
      }
    const size_t R = keep.size();
    if (drop)
      {
        // second pass: the kept columns M-orthonormalised on the device by the factor of their scaled Gram matrix (q_i = sum_{j <= i}
        // s_j d_j (L^-T)_ji, all three images), the Gram matrices formed again on that basis
        std::vector<double> L(R * R, 0.0), Li(R * R, 0.0);
        for (size_t i = 0; i < R; ++i)
          for (size_t j = 0; j <= i; ++j)
            {
              double t = gm[i * R + j];
              for (size_t q = 0; q < j; ++q)
                t -= L[i * R + q] * L[j * R + q];
              L[i * R + j] = i == j ? std::sqrt(t) : t / L[j * R + j];
            }
        for (size_t c0 = 0; c0 < R; ++c0) // Li = L^-1, column by column
          for (size_t i = c0; i < R; ++i)
            {
              double t = i == c0 ? 1.0 : 0.0;
              for (size_t q = c0; q < i; ++q)
                t -= L[i * R + q] * Li[q * R + c0];
              Li[i * R + c0] = t / L[i * R + i];
            }
        std::vector<double> T(K * K, 0.0);
        for (size_t i = 0; i < K; ++i)
          T[i * K + i] = 1.0; // (a column that was left out stays what it is)
        for (size_t i = 0; i < R; ++i)
          {
            T[size_t(keep[i]) * K + size_t(keep[i])] = 0.0;
            for (size_t j = 0; j <= i; ++j)
              T[size_t(keep[j]) * K + size_t(keep[i])] = d[size_t(keep[j])] * Li[i * R + j];
          }
        const size_t m = size_t(b.m);
        for (int blk = ks / b.m - 1; blk >= 0; --blk) // last block first: column i reads the columns <= i
          {
            std::vector<double> coef(K * m);
            for (size_t r = 0; r < K; ++r)
              for (size_t cc = 0; cc < m; ++cc)
                coef[r * m + cc] = T[r * K + size_t(blk) * m + cc];
            if (int rc = combine3(b, 0, ks, coef, b.m, size_t(blk) * m))
              return rc;
          }
        std::vector<double> fk, fm;
        if (int rc = gram(b, b.S, ks, b.KS, ks, fk))
          return rc;
        if (int rc = gram(b, b.S, ks, b.MS, ks, fm))
          return rc;
        for (size_t i = 0; i < R; ++i)
          for (size_t j = 0; j < R; ++j)
            {
              gk[i * R + j] = fk[size_t(keep[i]) * K + size_t(keep[j])];
              gm[i * R + j] = fm[size_t(keep[i]) * K + size_t(keep[j])];
            }
        for (size_t i = 0; i < K; ++i)
          d[i] = 1.0;
        min_pivot = 0.25;
      }
    if (dense_sym_eig(int(R), gk.data(), gm.data(), w.data(), V.data(), min_pivot))
      return MI_OK;
    *status = 0;
    lam.assign(w.begin(), w.begin() + b.m);
    C.assign(K * size_t(b.m), 0.0);
    for (size_t i = 0; i < R; ++i)
      for (int j = 0; j < b.m; ++j)
        C[size_t(keep[i]) * size_t(b.m) + size_t(j)] = d[size_t(keep[i])] * V[size_t(j) * R + i];
    return MI_OK;
  }

  // KX, MX afresh, X Rayleigh-Ritz'ed on its own (a well-conditioned m x m problem): M-orthonormal X, Ritz values
  int polish(const Blocks &b, std::vector<double> &lam)
  {
    if (int rc = products(b, 0))
      return rc;
    std::vector<double> C;
    int                 st = 0;
    if (int rc = rayleigh_ritz(b, b.m, 0.0, lam, C, &st))
      return rc;
    if (st)
      return fail(b.c, MI_ENOCONV_LIN, "%s: the iterates have become linearly dependent", b.name);
    return combine3(b, 0, b.m, C, b.m, 0);
  }

  // R into the W block of S; ratio_j = |R_j| / (max_k<n_modes |lambda_k| |MX_j|)
  int residual(const Blocks &b, const std::vector<double> &lam, int n_modes, std::vector<double> &ratio)
  {
    mi_ctx         *c = b.c;
    mi::BlockLambda l{};
    for (int j = 0; j < b.m; ++j)
      l.v[j] = lam[size_t(j)];
    mi::launch_block_residual(c->dim, b.KS, b.MS, b.n, l, b.m, c->d_cmask, b.n, b.W(b.S), b.n, b.part, b.sums, c->stream);
    HIPCHK(c, hipGetLastError());
    std::vector<double> s(2 * size_t(b.m));
    HIPCHK(c, hipMemcpyAsync(s.data(), b.sums, s.size() * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    double scale = 0.0;
    for (int k = 0; k < n_modes; ++k)
      scale = std::max(scale, std::fabs(lam[size_t(k)]));
    ratio.resize(size_t(b.m));
    for (int j = 0; j < b.m; ++j)
      ratio[size_t(j)] = std::sqrt(s[size_t(j)]) / (scale * std::sqrt(s[size_t(b.m + j)]));
    return MI_OK;
  }

  bool converged(const std::vector<double> &ratio, int n_modes, double tol)
  {
    for (int j = 0; j < n_modes; ++j)
      if (!(ratio[size_t(j)] <= tol))
        return false;
    return true;
  }

  int modes_run(mi_ctx *c, bool tangent, int n_modes, int m, double tol, int max_it, double *lambda, double *modes, double *residual_out,
                int *its)
  {
    Blocks b;
    b.c = c, b.n = c->n, b.m = m;
    b.tangent = tangent;
    if (tangent)
      b.name = "mi_tangent_modes", b.rho = c->mat.rho, b.shift = c->alpha[1] * c->mat.rho;
    const size_t n = size_t(c->n), blk = size_t(m) * n;
    const size_t npart = size_t(mi::block_chunks(c->n)) * size_t(9 * m * m);
    HIPCHK(c, hipMalloc((void **)&b.S, (tangent ? 10 : 9) * blk * sizeof(double)));
    b.KS = b.S + 3 * blk, b.MS = b.S + 6 * blk, b.MX = tangent ? b.S + 9 * blk : nullptr;
    HIPCHK(c, hipMalloc((void **)&b.part, npart * sizeof(double)));
    HIPCHK(c, hipMalloc((void **)&b.gram, size_t(9 * m * m) * sizeof(double)));
    HIPCHK(c, hipMalloc((void **)&b.coef, size_t(3 * m * m) * sizeof(double)));
    HIPCHK(c, hipMalloc((void **)&b.sums, size_t(2 * m) * sizeof(double)));
    HIPCHK(c, hipMemsetAsync(b.S, 0, 9 * blk * sizeof(double), c->stream));
    mi::launch_block_hash_init(c->dim, b.S, b.n, m, c->d_cmask, b.n, c->stream);
    HIPCHK(c, hipGetLastError());

    std::vector<double> lam, ratio, C, G;
    int                 rc = polish(b, lam);
    bool                have_p = false;
    int                 it = 0, status = MI_OK;
    while (!rc)
      {
        if ((rc = residual(b, lam, n_modes, ratio)))
          break;
        if (converged(ratio, n_modes, tol) || it == max_it)
          {
            // the pairs that are returned: products afresh, X orthonormalised, the stopping rule evaluated on them
            if ((rc = polish(b, lam)) || (rc = residual(b, lam, n_modes, ratio)))
              break;
            if (converged(ratio, n_modes, tol))
              break;
            if (it == max_it)
              {
                status = MI_ENOCONV_LIN;
                break;
              }
          }
        ++it;
        // W = T R (R lies in the W block), one vector at a time through the solver's residual vector
        if (!tangent)
          linear_select(c, 2);
        const bool    cycle = mg_active(c);
        const double *dinv  = tangent ? c->work(W_DINV) : c->active_dinv;
        for (int j = 0; j < m && !rc; ++j)
          {
            double *wj = b.W(b.S) + size_t(j) * n;
            HIPCHK(c, hipMemcpyAsync(c->work(W_R), wj, n * sizeof(double), hipMemcpyDeviceToDevice, c->stream));
            if (cycle)
              {
                if ((rc = mg_apply(*c->team)))
                  break;
                HIPCHK(c, hipMemcpyAsync(wj, c->work(W_Z), n * sizeof(double), hipMemcpyDeviceToDevice, c->stream));
              }
            else
              mi::launch_vec_scale_mul(wj, dinv, c->work(W_R), 1.0, c->n, c->stream);
            mi::launch_zero_constrained(c->dim, wj, c->d_cmask, c->n, c->stream);
          }
        if (rc)
          break;
        // W -= X (MX^T W): [X W] <- [X W] [[0], [-G; I]] written to W
        if ((rc = gram(b, b.MS, m, b.W(b.S), m, G)))
          break;
        C.assign(size_t(2 * m) * size_t(m), 0.0);
        for (int i = 0; i < m; ++i)
          for (int j = 0; j < m; ++j)
            C[size_t(i) * m + j] = -G[size_t(i) * m + j];
        for (int j = 0; j < m; ++j)
          C[size_t(m + j) * m + j] = 1.0;
        HIPCHK(c, hipMemcpyAsync(b.coef, C.data(), C.size() * sizeof(double), hipMemcpyHostToDevice, c->stream));
        mi::launch_block_combine(b.S, 2 * m, b.n, b.coef, m, b.W(b.S), b.n, b.n, c->stream);
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, hipStreamSynchronize(c->stream));
        if ((rc = products(b, size_t(m))))
          break;
        // Rayleigh-Ritz on [X W P]; without P, then with X re-orthonormalised, where the Gram matrix is singular
        int st = 1, ks = 0;
        for (int attempt = 0; attempt < 3 && st && !rc; ++attempt)
          {
            ks = (have_p ? 3 : 2) * m;
            if ((rc = rayleigh_ritz(b, ks, CHOL_MIN, lam, C, &st, tangent)) || !st)
              break;
            if (have_p)
              have_p = false;
            else
              rc = polish(b, lam);
          }
        // still singular with X orthonormal and no P: columns of W depend on X and on each other (with a preconditioner as good
        // as a V-cycle the residuals of a late iteration can all point at the same slow mode).  Those columns are left out
        if (st && !rc && tangent)
          rc = rayleigh_ritz(b, ks, CHOL_MIN, lam, C, &st, true);
        if (rc)
          break;
        if (st) // (not seen: the pairs of the last residual evaluation are returned as not converged)
          {
            status = MI_ENOCONV_LIN;
            break;
          }
        // X <- S C first (in place, row-wise), then P <- [W P] C_WP, which does not read X
        std::vector<double> Cwp(C.begin() + size_t(m) * m, C.end());
        if ((rc = combine3(b, 0, ks, C, m, 0)) || (rc = combine3(b, size_t(m), ks - m, Cwp, m, 2 * size_t(m))))
          break;
        have_p = true;
      }
    if (!tangent)
      linear_select(c, -1);
    if (rc)
      return rc;
    for (int j = 0; j < n_modes; ++j)
      {
        lambda[j] = lam[size_t(j)];
        if (residual_out)
          residual_out[j] = ratio[size_t(j)];
      }
    if (its)
      *its = it;
    if (modes)
      HIPCHK(c, hipMemcpy(modes, b.S, size_t(n_modes) * n * sizeof(double), hipMemcpyDeviceToHost));
    if (status)
      return fail(c, status, "%s: not converged within %d iterations", b.name, max_it);
    return MI_OK;
  }

  // the arguments the two entry points share; *m = block size, the wanted modes and their guard vectors
  int modes_arguments(mi_ctx *c, const char *name, int n_modes, double tol, int max_it, int *m)
  {
    if (n_modes < 1 || n_modes > 16 || !(tol > 0) || max_it < 1)
      return fail(c, MI_EINVAL, "%s: 1 <= n_modes <= 16, tol > 0 and max_it >= 1 are required", name);
    *m             = n_modes + std::max(2, n_modes / 4);
    int64_t n_free = 0;
    for (int64_t nd = 0; nd < c->mesh.nnodes; ++nd)
      for (int k = 0; k < c->dim; ++k)
        n_free += !((c->mesh.cmask[size_t(nd)] >> k) & 1);
    if (*m > n_free)
      return fail(c, MI_EINVAL, "%s: %d modes and %d guard vectors on %lld free dofs", name, n_modes, *m - n_modes, (long long)n_free);
    return MI_OK;
  }
} // namespace

extern "C" {

int mi_linear_modes(mi_ctx *c, int n_modes, double tol, int max_it, double *lambda, double *modes, double *residual, int *its)
{
  if (!c || !lambda)
    return c ? fail(c, MI_EINVAL, "mi_linear_modes: null argument") : MI_EINVAL;
  if (!c->linear)
    return fail(c, MI_EINVAL, "mi_linear_setup has not been called");
  if (team_size(c) != 1)
    return fail(c, MI_EINVAL, "mi_linear_modes: one slab only (an undecomposed mesh)");
  int m = 0;
  if (int rc = modes_arguments(c, "mi_linear_modes", n_modes, tol, max_it, &m))
    return rc;
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  const int rc = modes_run(c, false, n_modes, m, tol, max_it, lambda, modes, residual, its);
  linear_select(c, -1);
  hipStreamSynchronize(c->stream);
  return rc;
}

int mi_tangent_modes(mi_ctx *c, int n_modes, double tol, int max_it, double *lambda, double *modes, double *residual, int *its)
{
  if (!c || !lambda)
    return c ? fail(c, MI_EINVAL, "mi_tangent_modes: null argument") : MI_EINVAL;
  if (team_size(c) != 1 || !c->team || c->team->members[0] != c)
    return fail(c, MI_EINVAL, "mi_tangent_modes: one slab only (an undecomposed mesh)");
  if (c->linear_mf)
    return fail(c, MI_EINVAL, "mi_tangent_modes: the matrix-free linear model keeps no assembled tangent (\"linear_operator\" 0 and mi_linear_setup)");
  int m = 0;
  if (int rc = modes_arguments(c, "mi_tangent_modes", n_modes, tol, max_it, &m))
    return rc;
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  int rc = tangent_prepare(c);
  if (!rc)
    rc = modes_run(c, true, n_modes, m, tol, max_it, lambda, modes, residual, its);
  hipStreamSynchronize(c->stream);
  return rc;
}

// ---- inspection hooks: the block kernels on host arrays (column-major), and the host's dense eigensolver
int mi_block_gram(mi_ctx *c, int64_t n, const double *a, int ma, const double *b, int mb, double *out)
{
  if (!c || !a || !b || !out || n < 1 || ma < 1 || mb < 1 || ma > mi::BLOCK_MAX_COLS || mb > mi::BLOCK_MAX_COLS)
    return c ? fail(c, MI_EINVAL, "mi_block_gram: null argument, n < 1 or a column count outside 1 .. %d", mi::BLOCK_MAX_COLS) : MI_EINVAL;
  HIPCHK(c, hipSetDevice(c->device));
  const size_t na = size_t(n) * ma, nb = size_t(n) * mb, np = size_t(mi::block_chunks(n)) * ma * mb;
  double      *d = nullptr;
  HIPCHK(c, hipMalloc((void **)&d, (na + nb + np + size_t(ma) * mb) * sizeof(double)));
  hipError_t e = hipMemcpy(d, a, na * sizeof(double), hipMemcpyHostToDevice);
  if (e == hipSuccess)
    e = hipMemcpy(d + na, b, nb * sizeof(double), hipMemcpyHostToDevice);
  if (e == hipSuccess)
    {
      mi::launch_block_gram(d, ma, n, d + na, mb, n, n, d + na + nb, d + na + nb + np, c->stream);
      e = hipGetLastError();
    }
  if (e == hipSuccess)
    e = hipStreamSynchronize(c->stream);
  if (e == hipSuccess)
    e = hipMemcpy(out, d + na + nb + np, size_t(ma) * mb * sizeof(double), hipMemcpyDeviceToHost);
  hipFree(d);
  HIPCHK(c, e);
  return MI_OK;
}

int mi_block_combine(mi_ctx *c, int64_t n, const double *s, int ks, const double *coef, int my, double *y)
{
  if (!c || !s || !coef || !y || n < 1 || ks < 1 || my < 1 || ks > mi::BLOCK_MAX_COLS || my > mi::BLOCK_MAX_OUT)
    return c ? fail(c, MI_EINVAL, "mi_block_combine: null argument, n < 1, ks outside 1 .. %d or my outside 1 .. %d", mi::BLOCK_MAX_COLS,
                    mi::BLOCK_MAX_OUT) :
               MI_EINVAL;
  HIPCHK(c, hipSetDevice(c->device));
  const size_t ns = size_t(n) * ks, ny = size_t(n) * my, nc = size_t(ks) * my;
  double      *d = nullptr;
  HIPCHK(c, hipMalloc((void **)&d, (ns + ny + nc) * sizeof(double)));
  hipError_t e = hipMemcpy(d, s, ns * sizeof(double), hipMemcpyHostToDevice);
  if (e == hipSuccess)
    e = hipMemcpy(d + ns + ny, coef, nc * sizeof(double), hipMemcpyHostToDevice);
  if (e == hipSuccess)
    {
      mi::launch_block_combine(d, ks, n, d + ns + ny, my, d + ns, n, n, c->stream);
      e = hipGetLastError();
    }
  if (e == hipSuccess)
    e = hipStreamSynchronize(c->stream);
  if (e == hipSuccess)
    e = hipMemcpy(y, d + ns, ny * sizeof(double), hipMemcpyDeviceToHost);
  hipFree(d);
  HIPCHK(c, e);
  return MI_OK;
}

int mi_dense_sym_eig(int n, const double *A, const double *B, double *w, double *V)
{
  if (n < 1 || n > 64 || !A || !B || !w || !V)
    return fail(nullptr, MI_EINVAL, "mi_dense_sym_eig: null argument or n outside 1 .. 64");
  if (dense_sym_eig(n, A, B, w, V, 0.0))
    return fail(nullptr, MI_EINVAL, "mi_dense_sym_eig: B is not positive definite");
  return MI_OK;
}

} // extern "C"
