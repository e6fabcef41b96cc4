// lgn-autoencoder_amd/csrc/sinkhorn.hip -- the entropic optimal-transport loss (Sinkhorn iterations in the log domain) and its debiased
// form, the Sinkhorn divergence, for aligned pairs of events and for Cartesian jets on their relative-polar frames.
// Entry points: lgn_sinkhorn_f64, lgn_sinkhorn_relative_f64, lgn_sinkhorn_lds_bytes.  include/lgn_amd.h is the specification.
//
// The extended problem is the EMD's (emd.hip, emd_grad_opts.hip): rows are the first event's particles, columns the second's, row n and
// column m the fictitious particles of which at most one has weight (none under norm).  With a, b the extended weights, S their sum,
// C the option cost (EmdOptCost, the EMD's statements and bits) the kernel iterates on F = f / eps, G = g / eps and Cs = C / eps:
//     F_i <- -LSE_j(log(b_j / S) + G_j - Cs_ij)        G_j <- -LSE_i(log(a_i / S) + F_i - Cs_ij)         LSE max-shifted, G = 0 at the start
// One wavefront per pair, up to four per workgroup; no workgroup barrier anywhere (a wave whose pair number is past B leaves at once).
// Everything a pair needs sits in its wave's slice of LDS (SinkhornLds).  The two half-steps walk the cost matrix in the two directions:
// in the F half-step lane l owns the rows l + 64 k and sums over the columns in index order, in the G half-step it owns the columns
// l + 64 k and sums over the rows in index order.  A sum is therefore one lane's serial sum -- no cross-lane reduction inside a
// half-step -- and only the marginal error, the value and the weighted mean potentials of the norm form go through the fixed butterfly
// (wave_sum).  Cs is kept in LDS as [R][ld] with an odd leading dimension ld, so that the row-owner walk (lane stride ld doubles) and
// the column-owner walk (lane stride 1) are both free of bank conflicts; when the slice with it would pass 64 KiB (max(n, m) >= 82) the
// cost is recomputed from the staged coordinates in every sweep instead.  There is no global workspace.
//
// The gradient is the envelope formula at the returned state: the EMD's closed form (emd_dev.hpp: emd_opt_gradients) with the flow
// replaced by the plan P_ij = (a_i b_j / S) exp(F_i + G_j - Cs_ij), formed on the fly in one row-owner and one column-owner sweep, and
// (u, v) by (f, g).  debias runs the same routine on each event against itself (no fictitious particle) and subtracts half of each.
//
// Floating-point contraction is OFF for this file (pragma below and the Makefile), as for the EMD files: the costs are the EMD's bits.
#pragma clang fp contract(off)

#include <math.h>

#include "lds.hpp"
#include "../../include/lgn_amd.h"
#include "emd_dev.hpp"

namespace lgn {
namespace {

constexpr int SK_LDS_BUDGET = 64 * 1024;       // of one wave's slice with the cost matrix, and of a whole workgroup (no opt-in attribute)
constexpr int SK_MAX_WAVES = 4;                // pairs per workgroup

// One wave's slice: R = max(n, m) + 1 entries per array (the self problems of debias are n x n and m x m), ld = R | 1.
struct SinkhornLds {
  size_t wa, wb, la, lb, ya, pa, yb, pb, F, G, h0, h1, gy0, gp0, gy1, gp1, jet, cs;
  int R, ld;
  size_t bytes;
  __host__ __device__ SinkhornLds(int n, int m, bool cache) {
    R = (n > m ? n : m) + 1, ld = R | 1;
    LdsCarve c;
    wa = c.take<double>(R), wb = c.take<double>(R);          // extended weights (normalised under norm)
    la = c.take<double>(R), lb = c.take<double>(R);          // log(w / S) of the problem being solved
    ya = c.take<double>(R), pa = c.take<double>(R);          // (y, phi) of the rows
    yb = c.take<double>(R), pb = c.take<double>(R);          // ... of the columns
    F = c.take<double>(R), G = c.take<double>(R);            // potentials / eps of the problem being solved
    h0 = c.take<double>(R), h1 = c.take<double>(R);          // potentials that enter the weight gradients
    gy0 = c.take<double>(R), gp0 = c.take<double>(R);        // position gradients
    gy1 = c.take<double>(R), gp1 = c.take<double>(R);
    jet = c.take<double>(8);                                 // [2][4] jet 4-vectors (REL)
    cs = c.take<double>(cache ? (size_t)R * ld : 0);         // C / eps
    bytes = c.off;
  }
};
inline bool sinkhorn_cached(int n, int m) { return SinkhornLds(n, m, true).bytes <= (size_t)SK_LDS_BUDGET; }
inline int sinkhorn_waves(size_t slice) {
  const int w = (int)((size_t)SK_LDS_BUDGET / slice);
  return w < 1 ? 1 : (w > SK_MAX_WAVES ? SK_MAX_WAVES : w);
}

// One problem: rows x cols, weights and coordinates of either side (LDS), the fictitious indices (-1: none), the sum S.
struct SkProb {
  int rows, cols, fr, fc;
  const double *wr, *wc, *yr, *pr, *yc, *pc;
  double S;
};

// C / eps of (row i, column j): from LDS, or EmdOptCost's statements on the staged coordinates.
template <bool CACHE>
struct SkCost {
  EmdOptCost<1> c;
  const double *yc, *pc, *cs;
  int ld;
  double eps;
  __device__ __forceinline__ void problem(const SkProb& p) {
    c.y = p.yr, c.phi = p.pr, c.n = p.fr, c.m = p.fc;
    yc = p.yc, pc = p.pc;
  }
  __device__ __forceinline__ double raw(int i, int j) {
    c.lane = j, c.qy[0] = yc[j], c.qphi[0] = pc[j];
    return c(i, 0);
  }
  __device__ __forceinline__ double operator()(int i, int j) { return CACHE ? cs[(size_t)i * ld + j] : raw(i, j) / eps; }
};

// The iterations of one problem.  F, G, lr, lc: [rows], [cols] of LDS, written here.  Returns the number of applied iterations; err
// is the row-marginal violation of the returned (F, G), value = eps (<wr, F> + <wc, G>).  The same on every lane.
template <int K, bool CACHE>
__device__ __forceinline__ int sk_solve(SkCost<CACHE>& C, const SkProb& p, double* F, double* G, double* lr, double* lc, double* cs,
                                        int lane, double eps, int max_iter, double tol, double& value, double& err) {
  const int rows = p.rows, cols = p.cols;
  C.problem(p);
  for (int i = lane; i < rows; i += 64) lr[i] = p.wr[i] > 0.0 ? log(p.wr[i] / p.S) : 0.0;
  for (int j = lane; j < cols; j += 64) lc[j] = p.wc[j] > 0.0 ? log(p.wc[j] / p.S) : 0.0, G[j] = 0.0;
  if (CACHE) {
    for (int i = 0; i < rows; ++i)
      for (int j = lane; j < cols; j += 64) cs[(size_t)i * C.ld + j] = C.raw(i, j) / eps;
  }
  wave_sync();
  int it = 0;
  err = 0.0;
  for (;;) {
    double fn[K];
#pragma unroll
    for (int k = 0; k < K; ++k) {
      const int i = lane + 64 * k;
      fn[k] = 0.0;
      if (i < rows) {
        double M = -INFINITY, s = 0.0;
        for (int j = 0; j < cols; ++j)
          if (p.wc[j] > 0.0) {
            const double t = (lc[j] + G[j]) - C(i, j);
            M = t > M ? t : M;
          }
        for (int j = 0; j < cols; ++j)
          if (p.wc[j] > 0.0) s = s + exp(((lc[j] + G[j]) - C(i, j)) - M);
        fn[k] = -(M + log(s));
      }
    }
    if (it >= 1) {
      double part = 0.0;
#pragma unroll
      for (int k = 0; k < K; ++k) {
        const int i = lane + 64 * k;
        if (i < rows && p.wr[i] > 0.0) part = part + p.wr[i] * fabs(1.0 - exp(F[i] - fn[k]));
      }
      err = wave_sum(part);
      if (it >= max_iter || (tol > 0.0 && err <= tol * p.S)) break;
    }
#pragma unroll
    for (int k = 0; k < K; ++k)
      if (lane + 64 * k < rows) F[lane + 64 * k] = fn[k];
    wave_sync();
#pragma unroll
    for (int k = 0; k < K; ++k) {
      const int j = lane + 64 * k;
      if (j < cols) {
        double M = -INFINITY, s = 0.0;
        for (int i = 0; i < rows; ++i)
          if (p.wr[i] > 0.0) {
            const double t = (lr[i] + F[i]) - C(i, j);
            M = t > M ? t : M;
          }
        for (int i = 0; i < rows; ++i)
          if (p.wr[i] > 0.0) s = s + exp(((lr[i] + F[i]) - C(i, j)) - M);
        G[j] = -(M + log(s));
      }
    }
    wave_sync();
    ++it;
  }
  double part = 0.0;
  for (int i = lane; i < rows; i += 64) part = part + p.wr[i] * F[i];
  for (int j = lane; j < cols; j += 64) part = part + p.wc[j] * G[j];
  value = eps * wave_sum(part);
  return it;
}

// P_ij of the returned state; 0 where either particle is weightless
template <bool CACHE>
__device__ __forceinline__ double sk_plan(SkCost<CACHE>& C, const SkProb& p, const double* F, const double* G, int i, int j) {
  const double w = p.wr[i] * p.wc[j];
  if (!(w > 0.0)) return 0.0;
  return (w / p.S) * exp((F[i] + G[j]) - C(i, j));
}

// The position terms of one arc that carries P: k_ij dy and k_ij dphi s_ij (the statements of emd_opt_gradients, dy = row - column)
__device__ __forceinline__ void sk_arc(const EmdOptCost<1>& cf, double P, double yi, double pi, double yj, double pj, double& ty, double& tp) {
  ty = 0.0, tp = 0.0;
  const double dy = yi - yj;
  double dp = pi - pj, sgn = 1.0;
  if (cf.periodic) {
    const double a = M_PI - fabs(dp);
    sgn = (dp > 0.0 ? 1.0 : (dp < 0.0 ? -1.0 : 0.0)) * (a > 0.0 ? 1.0 : (a < 0.0 ? -1.0 : 0.0));
    dp = M_PI - fabs(a);
  }
  const double d = sqrt(dy * dy + dp * dp);
  if (P > 0.0 && d > 0.0) {
    double t;
    if (cf.beta_mode == BETA_TWO) {
      t = P * (2.0 / (cf.R * cf.R));
    } else {
      t = P / (cf.R * d);
      if (cf.beta_mode == BETA_POW) t = t * (cf.beta * pow(cf.R == 1.0 ? d : d / cf.R, cf.beta - 1.0));
    }
    ty = t * dy, tp = (t * dp) * sgn;
  }
}

// The position gradients of a solved problem, times `scale`: the rows' into (gyr, gpr) by the row owners, then the columns' into
// (gyc, gpc) by the column owners.  SET: the arrays are written, else added to (the self problems, whose two sides are one event:
// index i belongs to lane i & 63 in both sweeps, so the two updates of an entry are one lane's, in program order).
template <int K, bool CACHE, bool SET>
__device__ __forceinline__ void sk_position_gradients(SkCost<CACHE>& C, const SkProb& p, const double* F, const double* G, int lane,
                                                      double scale, double* gyr, double* gpr, double* gyc, double* gpc) {
  const int nr = p.fr >= 0 ? p.rows - 1 : p.rows, nc = p.fc >= 0 ? p.cols - 1 : p.cols;      // the real particles
#pragma unroll
  for (int k = 0; k < K; ++k) {
    const int i = lane + 64 * k;
    if (i < nr) {
      double sy = 0.0, sp = 0.0;
      for (int j = 0; j < nc; ++j) {
        double ty, tp;
        sk_arc(C.c, sk_plan(C, p, F, G, i, j), p.yr[i], p.pr[i], p.yc[j], p.pc[j], ty, tp);
        sy = sy + ty, sp = sp + tp;
      }
      gyr[i] = SET ? scale * sy : gyr[i] + scale * sy;
      gpr[i] = SET ? scale * sp : gpr[i] + scale * sp;
    }
  }
#pragma unroll
  for (int k = 0; k < K; ++k) {
    const int j = lane + 64 * k;
    if (j < nc) {
      double sy = 0.0, sp = 0.0;
      for (int i = 0; i < nr; ++i) {
        double ty, tp;
        sk_arc(C.c, sk_plan(C, p, F, G, i, j), p.yr[i], p.pr[i], p.yc[j], p.pc[j], ty, tp);
        sy = sy - ty, sp = sp - tp;
      }
      gyc[j] = SET ? scale * sy : gyc[j] + scale * sy;
      gpc[j] = SET ? scale * sp : gpc[j] + scale * sp;
    }
  }
}

struct SinkhornArgs {
  const double *a0, *a1;
  int B, n, m;
  lgn_sinkhorn_opts opt;
  double *value, *g0, *g1, *f, *g, *plan;
  int* iters;
  double* err;
  int* status;
};

// REL: a0 = recons, a1 = target [B][n][4] Cartesian jets (n == m), staged as emd_kernel<REL> stages them; otherwise events [B][n][3],
// [B][m][3] of (pT, y, phi).  g0, g1 [B][n][W], [B][m][W], W = 3 or (REL) 4, each nullable.
template <int K, bool CACHE, bool REL>
__global__ __launch_bounds__(64 * SK_MAX_WAVES) void sinkhorn_kernel(SinkhornArgs A) {
  extern __shared__ __align__(16) unsigned char smem_raw[];
  const int n = A.n, m = A.m, rows = n + 1, cols = m + 1, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long b = (long)blockIdx.x * (blockDim.x >> 6) + wave;
  if (b >= A.B) return;                    // (no workgroup barrier below)
  constexpr int W = REL ? 4 : 3;
  const SinkhornLds L(n, m, CACHE);
  unsigned char* smem = smem_raw + (size_t)wave * L.bytes;
  double *wa = lds_at<double>(smem, L.wa), *wb = lds_at<double>(smem, L.wb), *la = lds_at<double>(smem, L.la);
  double *lb = lds_at<double>(smem, L.lb), *ya = lds_at<double>(smem, L.ya), *pa = lds_at<double>(smem, L.pa);
  double *yb = lds_at<double>(smem, L.yb), *pb = lds_at<double>(smem, L.pb), *F = lds_at<double>(smem, L.F);
  double *G = lds_at<double>(smem, L.G), *h0 = lds_at<double>(smem, L.h0), *h1 = lds_at<double>(smem, L.h1);
  double *gy0 = lds_at<double>(smem, L.gy0), *gp0 = lds_at<double>(smem, L.gp0), *gy1 = lds_at<double>(smem, L.gy1);
  double *gp1 = lds_at<double>(smem, L.gp1), *jet = lds_at<double>(smem, L.jet), *cs = lds_at<double>(smem, L.cs);

  const double* __restrict__ x0 = A.a0 + (size_t)b * n * W;
  const double* __restrict__ x1 = A.a1 + (size_t)b * m * W;
  double* g0 = A.g0 ? A.g0 + (size_t)b * n * W : nullptr;
  double* g1 = A.g1 ? A.g1 + (size_t)b * m * W : nullptr;
  const bool grad = g0 || g1, norm = A.opt.base.norm != 0;
  const double eps = A.opt.epsilon, tol = A.opt.tol;
  const int max_iter = A.opt.max_iter;

  // ---- staging: the statements of emd_grad_opts_kernel, the columns then stored to LDS as well --------------------------------------
  bool bad = false;
  double p0 = 0.0, p1 = 0.0;
  {
    double dem[K], qy[K], qphi[K];
    if (REL) {
      emd_stage_rel<K>(x0, x1, n, m, lane, wa, ya, pa, jet, dem, qy, qphi, bad, p0, p1);
    } else {
      for (int i = lane; i < rows; i += 64) {
        double w = 0.0, y = 0.0, ph = 0.0;
        if (i < n) {
          const double* x = x0 + (size_t)i * 3;
          w = x[0], y = x[1], ph = x[2];
          bad |= !emd_finite(w) || !emd_finite(y) || !emd_finite(ph) || w < 0.0;
        }
        wa[i] = w, ya[i] = y, pa[i] = ph;
        p0 = p0 + w;
      }
#pragma unroll
      for (int k = 0; k < K; ++k) {
        const int j = lane + 64 * k;
        double w = 0.0, y = 0.0, ph = 0.0;
        if (j < m) {
          const double* x = x1 + (size_t)j * 3;
          w = x[0], y = x[1], ph = x[2];
          bad |= !emd_finite(w) || !emd_finite(y) || !emd_finite(ph) || w < 0.0;
        }
        dem[k] = w, qy[k] = y, qphi[k] = ph;
        p1 = p1 + w;
      }
    }
#pragma unroll
    for (int k = 0; k < K; ++k) {
      const int j = lane + 64 * k;
      if (j < cols) wb[j] = dem[k], yb[j] = qy[k], pb[j] = qphi[k];
    }
  }
  // ---- sums, empty test, norm, the fictitious particle: the statements of emd_solve_opts ----------------------------------------------
  int st = __ballot(bad) ? LGN_EMD_INVALID : 0;
  double S0 = wave_sum(p0), S1 = wave_sum(p1);
  const double T0 = S0, T1 = S1;           // the sums as given: what norm divides by
  if (!st && (norm ? (!(S0 > 0.0) || !(S1 > 0.0)) : (!(S0 > 0.0) && !(S1 > 0.0)))) st = LGN_EMD_EMPTY;
  if (norm && !st) {
    p0 = 0.0, p1 = 0.0;
    for (int i = lane; i < n; i += 64) {
      const double w = wa[i] / S0;
      wa[i] = w;
      p0 = p0 + w;
    }
#pragma unroll
    for (int k = 0; k < K; ++k) {
      const int j = lane + 64 * k;
      double w = 0.0;
      if (j < m) w = wb[j] / S1, wb[j] = w;
      p1 = p1 + w;
    }
    S0 = wave_sum(p0), S1 = wave_sum(p1);
  }
  double value = NAN, err = NAN;
  int iters = 0;
  if (!st) {
    if (lane == 0) {
      wa[n] = (!norm && S1 > S0) ? S1 - S0 : 0.0;
      wb[m] = (!norm && S0 > S1) ? S0 - S1 : 0.0;
    }
    wave_sync();
    SkCost<CACHE> C;
    C.c.options(A.opt.base);
    C.cs = cs, C.ld = L.ld, C.eps = eps;
    // ---- the cross problem ---------------------------------------------------------------------------------------------------------
    const SkProb cross{rows, cols, n, m, wa, wb, ya, pa, yb, pb, S0 > S1 ? S0 : S1};
    iters = sk_solve<K, CACHE>(C, cross, F, G, la, lb, cs, lane, eps, max_iter, tol, value, err);
    if (tol > 0.0 && err > tol * cross.S) st |= LGN_SINKHORN_ITER;
    if (A.f)
      for (int i = lane; i < rows; i += 64) A.f[(size_t)b * rows + i] = eps * F[i];
    if (A.g)
      for (int j = lane; j < cols; j += 64) A.g[(size_t)b * cols + j] = eps * G[j];
    if (A.plan) {
      double* po = A.plan + (size_t)b * rows * cols;
      for (int i = 0; i < rows; ++i)
        for (int j = lane; j < cols; j += 64) po[(size_t)i * cols + j] = sk_plan(C, cross, F, G, i, j);
    }
    if (grad) {                            // (h0[n] and h1[m]: the fictitious particles' potentials)
      for (int i = lane; i < rows; i += 64) h0[i] = eps * F[i];
      for (int j = lane; j < cols; j += 64) h1[j] = eps * G[j];
      sk_position_gradients<K, CACHE, true>(C, cross, F, G, lane, 1.0, gy0, gp0, gy1, gp1);
    }
    // ---- debias: each event against itself, no fictitious particle; a weightless event's self term is 0 -----------------------------
    if (A.opt.debias) {
#pragma unroll 1
      for (int side = 0; side < 2; ++side) {
        const int q = side ? m : n;
        const double Ss = side ? S1 : S0;
        if (!(Ss > 0.0)) continue;
        const double *w = side ? wb : wa, *y = side ? yb : ya, *ph = side ? pb : pa;
        double *h = side ? h1 : h0, *gy = side ? gy1 : gy0, *gp = side ? gp1 : gp0;
        const SkProb self{q, q, -1, -1, w, w, y, ph, y, ph, Ss};
        wave_sync();
        double vs, es;
        sk_solve<K, CACHE>(C, self, F, G, la, lb, cs, lane, eps, max_iter, tol, vs, es);
        if (tol > 0.0 && es > tol * Ss) st |= LGN_SINKHORN_ITER;
        value = value - 0.5 * vs;
        if (side ? g1 != nullptr : g0 != nullptr) {
          for (int i = lane; i < q; i += 64) h[i] = h[i] - 0.5 * (eps * (F[i] + G[i]));
          sk_position_gradients<K, CACHE, false>(C, self, F, G, lane, -0.5, gy, gp, gy, gp);
        }
      }
    }
    wave_sync();
  } else {
    if (A.f)
      for (int i = lane; i < rows; i += 64) A.f[(size_t)b * rows + i] = NAN;
    if (A.g)
      for (int j = lane; j < cols; j += 64) A.g[(size_t)b * cols + j] = NAN;
    if (A.plan)
      for (int t = lane; t < rows * cols; t += 64) A.plan[(size_t)b * rows * cols + t] = NAN;
  }
  if (lane == 0) {
    A.value[b] = value;
    A.status[b] = st;
    if (A.iters) A.iters[b] = iters;
    if (A.err) A.err[b] = err;
  }
  if (!grad) return;
  if (st & (LGN_EMD_INVALID | LGN_EMD_EMPTY)) {
    if (g0)
      for (int t = lane; t < n * W; t += 64) g0[t] = NAN;
    if (g1)
      for (int t = lane; t < m * W; t += 64) g1[t] = NAN;
    return;
  }
  // ---- weight gradients: the forms of emd_opt_gradients on h = f (- (f_self + g_self) / 2), then the way out -------------------------
  double c0, c1, q0 = 1.0, q1 = 1.0;
  if (norm) {
    double au = 0.0, bv = 0.0;
    if (g0)
      for (int i = lane; i < n; i += 64) au = au + wa[i] * h0[i];
    if (g1)
      for (int j = lane; j < m; j += 64) bv = bv + wb[j] * h1[j];
    c0 = -wave_sum(au), c1 = -wave_sum(bv), q0 = T0, q1 = T1;
  } else {
    const double un = h0[n], vm = h1[m];
    c0 = T1 > T0 ? -un : (T0 > T1 ? vm : 0.0), c1 = T0 > T1 ? -vm : (T1 > T0 ? un : 0.0);
  }
  auto w0 = [&](int i) { return norm ? (h0[i] + c0) / q0 : h0[i] + c0; };
  auto w1 = [&](int j) { return norm ? (h1[j] + c1) / q1 : h1[j] + c1; };
  if (REL) {
    if (g0)
      emd_rel_to_cartesian<K>(x0, jet, n, lane, [&](int k) { return w0(lane + 64 * k); }, [&](int k) { return gy0[lane + 64 * k]; },
                              [&](int k) { return gp0[lane + 64 * k]; }, g0);
    if (g1)
      emd_rel_to_cartesian<K>(x1, jet + 4, m, lane, [&](int k) { return w1(lane + 64 * k); }, [&](int k) { return gy1[lane + 64 * k]; },
                              [&](int k) { return gp1[lane + 64 * k]; }, g1);
  } else {
    if (g0)
      for (int i = lane; i < n; i += 64) g0[3 * i] = w0(i), g0[3 * i + 1] = gy0[i], g0[3 * i + 2] = gp0[i];
    if (g1)
      for (int j = lane; j < m; j += 64) g1[3 * j] = w1(j), g1[3 * j + 1] = gy1[j], g1[3 * j + 2] = gp1[j];
  }
}

template <int K, bool CACHE, bool REL>
int launch_sinkhorn_kc(const SinkhornArgs& a, hipStream_t st) {
  const SinkhornLds L(a.n, a.m, CACHE);
  const int waves = sinkhorn_waves(L.bytes);
  return lds_launch(sinkhorn_kernel<K, CACHE, REL>, "sinkhorn", dim3((a.B + waves - 1) / waves), dim3(64 * waves), L.bytes * waves, st, a);
}

template <bool REL>
int launch_sinkhorn(const SinkhornArgs& a, hipStream_t st) {
  const bool cache = sinkhorn_cached(a.n, a.m);
  const int K = ((a.n > a.m ? a.n : a.m) + 1 + 63) / 64;
#define LGN_SK_CASE(KK) \
  if (K == KK) return cache ? launch_sinkhorn_kc<KK, true, REL>(a, st) : launch_sinkhorn_kc<KK, false, REL>(a, st);
  LGN_SK_CASE(1)
  LGN_SK_CASE(2)
  LGN_SK_CASE(3)
#undef LGN_SK_CASE
  set_error("sinkhorn: n = %d, m = %d need more than three rows per lane", a.n, a.m);
  return -1;
}

int read_sinkhorn_opts(const char* who, const lgn_sinkhorn_opts* opts, lgn_sinkhorn_opts& o) {
  LGN_CHECK_ARG(opts, "%s: null pointer (opts)", who);
  o = *opts;
  LGN_CHECK_ARG(o.base.R > 0.0 && o.base.R < INFINITY, "%s: R = %g (need a finite R > 0)", who, o.base.R);
  LGN_CHECK_ARG(o.base.beta > 0.0 && o.base.beta < INFINITY, "%s: beta = %g (need a finite beta > 0)", who, o.base.beta);
  LGN_CHECK_ARG(o.epsilon > 0.0 && o.epsilon < INFINITY, "%s: epsilon = %g (need a finite epsilon > 0)", who, o.epsilon);
  LGN_CHECK_ARG(o.tol >= 0.0 && o.tol < INFINITY, "%s: tol = %g (need a finite tol >= 0)", who, o.tol);
  LGN_CHECK_ARG(o.max_iter >= 1, "%s: max_iter = %d (need max_iter >= 1)", who, o.max_iter);
  o.base.norm = o.base.norm != 0, o.base.periodic_phi = o.base.periodic_phi != 0, o.debias = o.debias != 0;
  return 0;
}

}  // namespace
}  // namespace lgn

using namespace lgn;

extern "C" {

long long lgn_sinkhorn_lds_bytes(int n, int m) {
  if (n < 1 || n > LGN_EMD_NMAX || m < 1 || m > LGN_EMD_NMAX) {
    set_error("sinkhorn_lds_bytes: n = %d, m = %d outside 1 .. %d", n, m, LGN_EMD_NMAX);
    return -1;
  }
  return (long long)SinkhornLds(n, m, sinkhorn_cached(n, m)).bytes;
}

int lgn_sinkhorn_f64(const double* ev0, const double* ev1, int B, int n, int m, const lgn_sinkhorn_opts* opts, double* value, double* g0,
                     double* g1, double* f, double* g, double* plan, int* iters, double* err, int* status, void* stream) {
  LGN_CHECK_ARG(B >= 1, "sinkhorn: B = %d (need B >= 1)", B);
  LGN_CHECK_ARG(n >= 1 && n <= LGN_EMD_NMAX && m >= 1 && m <= LGN_EMD_NMAX, "sinkhorn: n = %d, m = %d outside 1 .. %d", n, m, LGN_EMD_NMAX);
  LGN_CHECK_ARG(ev0 && ev1 && value && status, "sinkhorn: null pointer (ev0, ev1, value, status)");
  lgn_sinkhorn_opts o;
  if (read_sinkhorn_opts("sinkhorn", opts, o) != 0) return -1;
  const SinkhornArgs a{ev0, ev1, B, n, m, o, value, g0, g1, f, g, plan, iters, err, status};
  return launch_sinkhorn<false>(a, (hipStream_t)stream);
}

int lgn_sinkhorn_relative_f64(const double* recons, const double* target, int B, int N, const lgn_sinkhorn_opts* opts, double* value,
                              double* g_recons, double* g_target, int* iters, double* err, int* status, void* stream) {
  LGN_CHECK_ARG(B >= 1, "sinkhorn_relative: B = %d (need B >= 1)", B);
  LGN_CHECK_ARG(N >= 1 && N <= LGN_EMD_NMAX, "sinkhorn_relative: N = %d outside 1 .. %d", N, LGN_EMD_NMAX);
  LGN_CHECK_ARG(recons && target && value && status, "sinkhorn_relative: null pointer (recons, target, value, status)");
  LGN_CHECK_ARG(g_recons || !g_target, "sinkhorn_relative: g_target without g_recons");
  lgn_sinkhorn_opts o;
  if (read_sinkhorn_opts("sinkhorn_relative", opts, o) != 0) return -1;
  const SinkhornArgs a{recons, target, B, N, N, o, value, g_recons, g_target, nullptr, nullptr, nullptr, iters, err, status};
  return launch_sinkhorn<true>(a, (hipStream_t)stream);
}

}  // extern "C"
