// lgn-autoencoder_amd/csrc/emd_pairs_grad.hip -- the gradient of a matrix of energy mover's distances (energyflow.emd.emds with autograd):
// every pair of a range of whole rows of the FULL or UPPER matrix is solved once, by one wavefront that also writes that pair's
// gradients, and a second kernel sums the pairs' gradients, weighted by the upstream matrix, in a fixed order.
// Entry points: lgn_emd_pairs_grad_f64, lgn_emd_pairs_grad_reduce_f64, lgn_emd_pairs_grad_slab_bytes (include/lgn_amd.h).
//
// emd_pairs_grad_kernel<K, Flow, OPT>: the persistent grid of emd_pairs_kernel over the pair numbers of the row range.  A wave stages
// ev0[i] and ev1[j] where they lie, solves and writes the value exactly as emd_pairs_kernel<K, Flow, OPT> does (its statements in its
// order: the value has the bits of lgn_emd_pairs_f64), then runs the gradient epilogue into this pair's rows of the two slabs
// s0 [pairs][n][3] and s1 [pairs][m][3].  OPT = true: the epilogue of emd_grad_opts.hip (emd_opt_gradients, its generic form); OPT =
// false: emd.hip's cost and emd_gradients, which is the same epilogue with every option branch taken out.  The slabs therefore have
// the bits lgn_emd_grad_opts_f64 (at default options lgn_emd_grad_f64) gives for the same ordered pair.  The statements are repeated
// here, not shared: the kernels of emd.hip, emd_pairs.hip and emd_grad_opts.hip keep their instructions.
//
// emd_pairs_grad_reduce_kernel: one thread per output element, a rounded multiply and a rounded add per pair, partners ascending; no
// FMA (contraction is off), no atomics, no tree.  A range that starts at row 0 starts every sum at +0.0, a later range continues from
// what is stored, so ranges processed in ascending order give bits that do not depend on where they were cut.
//
// Floating-point contraction is OFF for this file (pragma below and the Makefile), as for emd.hip, emd_pairs.hip and emd_grad_opts.hip.
#pragma clang fp contract(off)

#include <limits.h>
#include <math.h>

#include <type_traits>

#include "lds.hpp"
#include "../../include/lgn_amd.h"
#include "emd_plan.hpp"
#include "emd_wave.hpp"

namespace lgn {
namespace {

// emd_pairs.hip's grids (DESIGN 8.1c has the measurements): one workgroup per pair up to EMD_PAIRS_GRID with the flow in LDS, resident
// waves only on the workspace path.
constexpr int EMD_PAIRS_GRID = 1048573;
constexpr int EMD_PAIRS_GLOBAL_WAVES = 2039;
constexpr int EMD_AUG_PER_NODE = 16;           // emd.hip's cap of the augmentations of one problem per node
constexpr int REDUCE_BLOCK = 256;
enum { BETA_ONE = 0, BETA_TWO = 1, BETA_POW = 2 };

static_assert(EMD_NMAX == LGN_EMD_NMAX, "include/lgn_amd.h and emd_wave.hpp agree on the largest event");
static_assert(EMD_PAIRS_GLOBAL_WAVES <= EMD_GLOBAL_WAVES, "lgn_emd_workspace_bytes holds a slice for every wave");

// c[i][j] = theta_ij^beta, 1 to or from the fictitious node; rows from LDS, columns in registers: emd_pairs.hip's EmdPairCost.
// OPT = false is emd.hip's EmdCost.
template <int K, bool OPT>
struct EmdPairGradCost {
  const double *y, *phi;       // [n + 1]
  int n, m, lane;
  double R, beta;
  int beta_mode, periodic;
  double qy[K], qphi[K];
  __device__ __forceinline__ double operator()(int i, int k) const {
    const int j = lane + 64 * k;
    if (i == n || j == m) return (i == n && j == m) ? 0.0 : 1.0;
    const double dy = y[i] - qy[k];
    double dp = phi[i] - qphi[k];
    if (OPT && periodic) {                     // pi - |pi - |dphi||, one rounded operation each
      const double a = M_PI - fabs(dp);
      dp = M_PI - fabs(a);
    }
    const double d = sqrt(dy * dy + dp * dp);
    const double t = R == 1.0 ? d : d / R;
    if (!OPT || beta_mode == BETA_ONE) return t;
    return beta_mode == BETA_TWO ? t * t : pow(t, beta);
  }
};

__device__ __forceinline__ bool finite(double x) { return fabs(x) < INFINITY; }      // false for NaN and +-inf

// The gradient epilogue of one solved pair: emd_opt_gradients of emd_grad_opts.hip in its generic (not relative) form; with OPT =
// false every option branch is gone and what is left is emd_gradients of emd.hip.  F the optimal flow, rs.u and v the finished
// potentials, S0 and S1 the sums of the weights as staged (before norm), x0 and x1 this pair's events, g0 and g1 its rows of the
// slabs.  Overwrites rs.dist and rs.sup.
template <int K, class Flow, bool OPT>
__device__ __forceinline__ void emd_pair_gradients(const EmdPairGradCost<K, OPT>& cf, const EmdRows& rs, const Flow& F, const double (&v)[K],
                                                   int st, bool norm, double S0, double S1, const double* __restrict__ x0,
                                                   const double* __restrict__ x1, double* __restrict__ g0, double* __restrict__ g1) {
  const int n = cf.n, m = cf.m, lane = cf.lane;
  if (st) {
    for (int t = lane; t < n * 3; t += 64) g0[t] = NAN;
    for (int t = lane; t < m * 3; t += 64) g1[t] = NAN;
    return;
  }
  const double two_over_R2 = 2.0 / (cf.R * cf.R), bm1 = cf.beta - 1.0;
  double cy[K], cp[K];
#pragma unroll
  for (int k = 0; k < K; ++k) cy[k] = cp[k] = 0.0;
  for (int i = 0; i < n; ++i) {
    const double yi = cf.y[i], pi = cf.phi[i];
    double ry = 0.0, rp = 0.0;
#pragma unroll
    for (int k = 0; k < K; ++k) {
      const int j = lane + 64 * k;
      if (j < m) {
        const double f = F.get(i, j);
        const double dy = yi - cf.qy[k];
        double dp = pi - cf.qphi[k], sgn = 1.0;
        if (OPT && cf.periodic) {
          const double a = M_PI - fabs(dp);
          sgn = (dp > 0.0 ? 1.0 : (dp < 0.0 ? -1.0 : 0.0)) * (a > 0.0 ? 1.0 : (a < 0.0 ? -1.0 : 0.0));
          dp = M_PI - fabs(a);
        }
        const double d = sqrt(dy * dy + dp * dp);
        if (f > 0.0 && d > 0.0) {
          double t;
          if (OPT && cf.beta_mode == BETA_TWO) {
            t = f * two_over_R2;
          } else {
            t = f / (cf.R * d);                                // f / (R^2 theta)
            if (OPT && cf.beta_mode == BETA_POW) t = t * (cf.beta * pow(cf.R == 1.0 ? d : d / cf.R, bm1));
          }
          const double ty = t * dy, tp = OPT ? (t * dp) * sgn : t * dp;
          ry = ry + ty, rp = rp + tp;
          cy[k] = cy[k] - ty, cp[k] = cp[k] - tp;
        }
      }
    }
    ry = wave_sum(ry), rp = wave_sum(rp);
    if (lane == 0) rs.dist[i] = ry, rs.sup[i] = rp;
  }
  wave_sync();
  // norm off: the fictitious particle's weight is the difference of the sums, its potential joins every weight gradient on both sides.
  // norm on: no fictitious weight; a_k = pT_k / S0 moves with every pT of its event, which subtracts the weighted mean potential.
  double c0, c1, q0 = 1.0, q1 = 1.0;
  if (OPT && norm) {
    double au = 0.0, bv = 0.0;
    for (int i = lane; i < n; i += 64) au = au + (x0[3 * i] / S0) * rs.u[i];
#pragma unroll
    for (int k = 0; k < K; ++k)
      if (lane + 64 * k < m) bv = bv + (x1[3 * (lane + 64 * k)] / S1) * v[k];
    c0 = -wave_sum(au), c1 = -wave_sum(bv), q0 = S0, q1 = S1;
  } else {
    const double un = rs.u[n], vm = lane_slot<K>(v, m);
    c0 = S1 > S0 ? -un : (S0 > S1 ? vm : 0.0), c1 = S0 > S1 ? -vm : (S1 > S0 ? un : 0.0);
  }
  auto w0 = [&](int i) { return (OPT && norm) ? (rs.u[i] + c0) / q0 : rs.u[i] + c0; };
  auto w1 = [&](int k) { return (OPT && norm) ? (v[k] + c1) / q1 : v[k] + c1; };
  for (int i = lane; i < n; i += 64) g0[3 * i] = w0(i), g0[3 * i + 1] = rs.dist[i], g0[3 * i + 2] = rs.sup[i];
#pragma unroll
  for (int k = 0; k < K; ++k) {
    const int j = lane + 64 * k;
    if (j < m) g1[3 * j] = w1(k), g1[3 * j + 1] = cy[k], g1[3 * j + 2] = cp[k];
  }
}

// ev0 [B0][n][3], ev1 [B1][m][3] (ev0 itself in UPPER mode).  The pairs of the rows [row_begin, row_begin + row_count) of the matrix
// are the pair numbers [p_begin, p_begin + P) of emd_plan.hpp; pair p_begin + q writes row q of s0 [P][n][3] and s1 [P][m][3], and
// its value and status into emd and status [B0][B1] (each nullable), mirrored in UPPER.  One wave per workgroup, with emd_kernel's LDS
// (emd_plan.hpp) and, on the workspace path, its own slice of `work`.
template <int K, class Flow, bool OPT>
__global__ __launch_bounds__(64) void emd_pairs_grad_kernel(const double* __restrict__ ev0, const double* __restrict__ ev1, int mode,
                                                            long long p_begin, long long P, int B0, int B1, int n, int m, lgn_emd_opts opt,
                                                            int row_begin, int row_count, double* __restrict__ emd,
                                                            double* __restrict__ s0, double* __restrict__ s1, int* __restrict__ status,
                                                            double* __restrict__ work) {
  extern __shared__ __align__(16) double lds[];
  const int rows = n + 1, cols = m + 1, lane = threadIdx.x & 63;
  const long long slot = blockIdx.x, slots = gridDim.x;
  constexpr bool LDS_FLOW = std::is_same<Flow, FlowLds>::value;
  EmdRows rs;
  rs.u = lds;
  rs.sup = rs.u + rows;
  rs.dist = rs.sup + rows;
  double* ry = rs.dist + rows;
  double* rphi = ry + rows;
  double* fl = rphi + rows + 8;            // [cols][rows] (LDS_FLOW); the 8 doubles before it are emd_kernel's jet sums (unused here)
  rs.pred = reinterpret_cast<int*>(fl + (LDS_FLOW ? rows * cols : 0));
  rs.vis = rs.pred + rows;
  Flow F;
  F.f = LDS_FLOW ? fl : work + (size_t)slot * rows * cols;
  F.ld = rows;

  if (mode == LGN_EMD_PAIRS_UPPER)         // the diagonal of the rows of this call: +0.0 with status 0, whatever the event holds
    for (long long d = slot * 64 + lane; d < row_count; d += slots * 64) {
      const size_t dd = (size_t)(row_begin + d) * B0 + (row_begin + d);
      if (emd) emd[dd] = 0.0;
      if (status) status[dd] = 0;
    }

  for (long long q = slot; q < P; q += slots) {
    const long long p = p_begin + q;
    int pi, pj;
    emd_pairs_decode(mode, p, B0, B1, pi, pj);
    const double* __restrict__ a0 = ev0 + (size_t)pi * n * 3;
    const double* __restrict__ a1 = ev1 + (size_t)pj * m * 3;
    wave_sync();                           // the LDS of the previous pair is free
    EmdPairGradCost<K, OPT> cf;
    cf.y = ry, cf.phi = rphi, cf.n = n, cf.m = m, cf.lane = lane, cf.R = opt.R, cf.beta = opt.beta, cf.periodic = opt.periodic_phi;
    cf.beta_mode = opt.beta == 1.0 ? BETA_ONE : (opt.beta == 2.0 ? BETA_TWO : BETA_POW);
    double dem[K], v[K];
    bool bad = false;
    double p0 = 0.0, p1 = 0.0;
    for (int i = lane; i < rows; i += 64) {
      double w = 0.0, y = 0.0, ph = 0.0;
      if (i < n) {
        const double* x = a0 + (size_t)i * 3;
        w = x[0], y = x[1], ph = x[2];
        bad |= !finite(w) || !finite(y) || !finite(ph) || w < 0.0;
      }
      rs.sup[i] = w, ry[i] = y, rphi[i] = ph;
      p0 = p0 + w;
    }
#pragma unroll
    for (int k = 0; k < K; ++k) {
      const int j = lane + 64 * k;
      double w = 0.0, y = 0.0, ph = 0.0;
      if (j < m) {
        const double* x = a1 + (size_t)j * 3;
        w = x[0], y = x[1], ph = x[2];
        bad |= !finite(w) || !finite(y) || !finite(ph) || w < 0.0;
      }
      dem[k] = w, cf.qy[k] = y, cf.qphi[k] = ph;
      p1 = p1 + w;
    }
    int st = __ballot(bad) ? LGN_EMD_INVALID : 0;
    double S0 = wave_sum(p0), S1 = wave_sum(p1);
    const double T0 = S0, T1 = S1;         // the sums as given: what norm divides by
    const bool norm = OPT && opt.norm;
    if (!st && (norm ? (!(S0 > 0.0) || !(S1 > 0.0)) : (!(S0 > 0.0) && !(S1 > 0.0)))) st = LGN_EMD_EMPTY;
    if (norm && !st) {                     // each event's weights over that event's sum; the sums of what the solver will see
      p0 = 0.0, p1 = 0.0;
      for (int i = lane; i < n; i += 64) {   // (a lane's own rows: no other lane has touched them)
        const double w = rs.sup[i] / S0;
        rs.sup[i] = w;
        p0 = p0 + w;
      }
#pragma unroll
      for (int k = 0; k < K; ++k) {
        if (lane + 64 * k < m) dem[k] = dem[k] / S1;
        p1 = p1 + dem[k];
      }
      S0 = wave_sum(p0), S1 = wave_sum(p1);
    }
    double score = NAN;
    int n_aug = 0;
    bool had[K];
#pragma unroll
    for (int k = 0; k < K; ++k) had[k] = false;
    if (!st) {
      // the fictitious particle of the lighter event carries the difference; none under norm (the two sums differ by rounding only)
      if (lane == 0) rs.sup[n] = (!norm && S1 > S0) ? S1 - S0 : 0.0;
#pragma unroll
      for (int k = 0; k < K; ++k) {
        if (lane + 64 * k == m) dem[k] = (!norm && S0 > S1) ? S0 - S1 : 0.0;
        had[k] = lane + 64 * k < cols && dem[k] > 0.0;
      }
      wave_sync();
      const double tol = (double)(n + m) * 0x1p-52 * (S0 > S1 ? S0 : S1);      // the rounding bound of the two sums
      st = emd_wave<K>(cf, rows, cols, rs, dem, v, F, EMD_AUG_PER_NODE * (rows + cols), tol, n_aug);
      wave_sync();
    }
    if (!st) {
      double part = 0.0;
#pragma unroll
      for (int k = 0; k < K; ++k) {
        if (had[k]) {
          for (int i = 0; i < rows; ++i) {
            const double f = F.get(i, lane + 64 * k);
            if (f > 0.0) part = part + f * cf(i, k);
          }
        }
      }
      score = wave_sum(part);
      finish_duals<K>(cf, rows, cols, rs, had, v);
    }
    if (lane == 0) {
      const size_t ij = (size_t)pi * B1 + pj, ji = (size_t)pj * B1 + pi;     // (UPPER: B1 == B0)
      if (emd) {
        emd[ij] = score;
        if (mode == LGN_EMD_PAIRS_UPPER) emd[ji] = score;
      }
      if (status) {
        status[ij] = st;
        if (mode == LGN_EMD_PAIRS_UPPER) status[ji] = st;
      }
    }
    emd_pair_gradients<K, Flow, OPT>(cf, rs, F, v, st, norm, T0, T1, a0, a1, s0 + (size_t)q * n * 3, s1 + (size_t)q * m * 3);
  }
}

// The weighted sum of the slabs of one row range (the header of this file; include/lgn_amd.h states the order).  Thread t owns one
// double of g0 or of g1: element c of an event e.  G [B0][B1] is nullable (every weight 1).
//   FULL   g0[i] of the rows of the range: over j ascending, complete in this call.  g1[j]: over the rows i of the range ascending,
//          from +0.0 when the range starts at row 0, else from what g1 holds.
//   UPPER  g0[e] of every event: the pairs (k, e) of the rows k < e of the range, k ascending, with s1; then, when row e is in the
//          range, the pairs (e, k), k > e ascending, with s0.  From +0.0 when the range starts at row 0, else from what g0 holds.
__global__ __launch_bounds__(REDUCE_BLOCK) void emd_pairs_grad_reduce_kernel(const double* __restrict__ s0, const double* __restrict__ s1,
                                                                             const double* __restrict__ G, int B0, int B1, int n, int m,
                                                                             int mode, int row_begin, int row_count, double* g0,
                                                                             double* g1, long long count0, long long count1) {
  const long long t = (long long)blockIdx.x * REDUCE_BLOCK + threadIdx.x;
  if (t >= count0 + count1) return;
  const int row_end = row_begin + row_count;
  if (mode == LGN_EMD_PAIRS_FULL) {
    if (t < count0) {                      // g0: the rows of the range
      const int w3 = n * 3, r = (int)(t / w3), c = (int)(t % w3), i = row_begin + r;
      const double* s = s0 + (size_t)r * B1 * w3 + c;
      double acc = 0.0;
#pragma unroll 8
      for (int j = 0; j < B1; ++j) {
        const double w = G ? G[(size_t)i * B1 + j] : 1.0;
        const double term = w * s[(size_t)j * w3];
        acc = acc + term;
      }
      g0[(size_t)i * w3 + c] = acc;
    } else {                               // g1: every column event
      const long long u = t - count0;
      const int w3 = m * 3, j = (int)(u / w3), c = (int)(u % w3);
      const double* s = s1 + (size_t)j * w3 + c;
      double acc = row_begin == 0 ? 0.0 : g1[(size_t)j * w3 + c];
#pragma unroll 8
      for (int i = row_begin; i < row_end; ++i) {
        const double w = G ? G[(size_t)i * B1 + j] : 1.0;
        const double term = w * s[(size_t)(i - row_begin) * B1 * w3];
        acc = acc + term;
      }
      g1[(size_t)j * w3 + c] = acc;
    }
    return;
  }
  // UPPER (count1 == 0; n == m; B1 == B0)
  const int w3 = n * 3, e = (int)(t / w3), c = (int)(t % w3);
  const unsigned long long B = (unsigned long long)B0, base = emd_upper_row_start((unsigned long long)row_begin, B);
  double acc = row_begin == 0 ? 0.0 : g0[(size_t)e * w3 + c];
  const int kend = e < row_end ? e : row_end;
#pragma unroll 8
  for (int k = row_begin; k < kend; ++k) {                     // pairs (k, e), k < e: the event is the column
    const double w = G ? G[(size_t)k * B0 + e] + G[(size_t)e * B0 + k] : 1.0 + 1.0;
    const size_t q = (size_t)(emd_upper_row_start((unsigned long long)k, B) - base) + (size_t)(e - k - 1);
    const double term = w * s1[q * w3 + c];
    acc = acc + term;
  }
  if (e >= row_begin && e < row_end) {                         // pairs (e, k), k > e: the event is the row
    const size_t q0 = (size_t)(emd_upper_row_start((unsigned long long)e, B) - base);
#pragma unroll 8
    for (int k = e + 1; k < B0; ++k) {
      const double w = G ? G[(size_t)e * B0 + k] + G[(size_t)k * B0 + e] : 1.0 + 1.0;
      const double term = w * s0[(q0 + (size_t)(k - e - 1)) * w3 + c];
      acc = acc + term;
    }
  }
  g0[(size_t)e * w3 + c] = acc;
}

struct PairsGradArgs {
  const double *ev0, *ev1;
  int mode;
  long long p_begin, P;
  int B0, B1, n, m;
  lgn_emd_opts opt;
  int row_begin, row_count;
  double *emd, *s0, *s1;
  int* status;
  double* work;
};

template <int K, class Flow, bool OPT>
int launch_pairs_grad_kfo(const PairsGradArgs& a, int grid, size_t smem, hipStream_t st) {
  return lds_launch(emd_pairs_grad_kernel<K, Flow, OPT>, "emd_pairs_grad", dim3(grid), dim3(64), smem, st, a.ev0, a.ev1, a.mode, a.p_begin,
                    a.P, a.B0, a.B1, a.n, a.m, a.opt, a.row_begin, a.row_count, a.emd, a.s0, a.s1, a.status, a.work);
}

template <int K, class Flow>
int launch_pairs_grad_kf(const PairsGradArgs& a, int grid, size_t smem, hipStream_t st) {
  const bool optioned = a.opt.beta != 1.0 || a.opt.norm || a.opt.periodic_phi;
  return optioned ? launch_pairs_grad_kfo<K, Flow, true>(a, grid, smem, st) : launch_pairs_grad_kfo<K, Flow, false>(a, grid, smem, st);
}

int launch_pairs_grad(const PairsGradArgs& a, hipStream_t st) {
  const int N = a.n > a.m ? a.n : a.m;
  const bool in_lds = emd_flow_in_lds(N);
  const size_t smem = (size_t)emd_lds_total(a.n, a.m, in_lds);
  // P == 0 (UPPER, the last row alone): one workgroup writes the diagonal
  const long long waves_max = in_lds ? EMD_PAIRS_GRID : EMD_PAIRS_GLOBAL_WAVES;
  const int grid = (int)(a.P < 1 ? 1 : (a.P < waves_max ? a.P : waves_max));
  const int K = (a.m + 1 + 63) / 64;
#define LGN_EMD_CASE(KK) \
  if (K == KK) return in_lds ? launch_pairs_grad_kf<KK, FlowLds>(a, grid, smem, st) : launch_pairs_grad_kf<KK, FlowGlobal>(a, grid, smem, st);
  LGN_EMD_CASE(1)
  LGN_EMD_CASE(2)
  LGN_EMD_CASE(3)
#undef LGN_EMD_CASE
  set_error("emd_pairs_grad: m = %d needs more than three columns per lane", a.m);
  return -1;
}

// what both calls refuse about the shape of the matrix and the row range; ev1_is_other: ev1 is neither NULL nor ev0
int check_shape(const char* who, int mode, int B0, int B1, int n, int m, int row_begin, int row_count, bool ev1_is_other) {
  LGN_CHECK_ARG(mode == LGN_EMD_PAIRS_FULL || mode == LGN_EMD_PAIRS_UPPER, "%s: mode %d (the matrix modes are FULL and UPPER)", who, mode);
  LGN_CHECK_ARG(B0 >= 1 && B1 >= 1, "%s: B0 = %d, B1 = %d (need both >= 1)", who, B0, B1);
  LGN_CHECK_ARG(n >= 1 && n <= LGN_EMD_NMAX && m >= 1 && m <= LGN_EMD_NMAX, "%s: n = %d, m = %d outside 1 .. %d", who, n, m, LGN_EMD_NMAX);
  if (mode == LGN_EMD_PAIRS_UPPER) {
    LGN_CHECK_ARG(n == m && B0 == B1, "%s: UPPER is one set against itself: n = %d, m = %d, B0 = %d, B1 = %d", who, n, m, B0, B1);
    LGN_CHECK_ARG(!ev1_is_other, "%s: UPPER takes ev1 NULL or ev0 itself", who);
  }
  LGN_CHECK_ARG(row_begin >= 0 && row_count >= 1 && row_begin <= B0 - row_count, "%s: rows %d .. %d + %d outside the %d rows of the matrix",
                who, row_begin, row_begin, row_count, B0);
  return 0;
}

// the pair numbers [p_begin, p_begin + P) of the rows [row_begin, row_begin + row_count)
void range_pairs(int mode, int B0, int B1, int row_begin, int row_count, long long& p_begin, long long& P) {
  if (mode == LGN_EMD_PAIRS_FULL) {
    p_begin = (long long)row_begin * B1, P = (long long)row_count * B1;
  } else {
    p_begin = (long long)emd_upper_row_start((unsigned long long)row_begin, (unsigned long long)B0);
    P = (long long)emd_upper_row_start((unsigned long long)(row_begin + row_count), (unsigned long long)B0) - p_begin;
  }
}

}  // namespace
}  // namespace lgn

using namespace lgn;

extern "C" {

long long lgn_emd_pairs_grad_slab_bytes(int mode, int B0, int B1, int n, int m, int row_begin, int row_count) {
  if (check_shape("emd_pairs_grad_slab_bytes", mode, B0, B1, n, m, row_begin, row_count, false) != 0) return -1;
  long long p_begin, P;
  range_pairs(mode, B0, B1, row_begin, row_count, p_begin, P);
  return P * (long long)(n + m) * 3 * 8;
}

int lgn_emd_pairs_grad_f64(const double* ev0, const double* ev1, int B0, int B1, int n, int m, int mode, const lgn_emd_opts* opts,
                           int row_begin, int row_count, double* emd, double* s0, double* s1, int* status, void* work,
                           long long work_bytes, void* stream) {
  if (check_shape("emd_pairs_grad", mode, B0, B1, n, m, row_begin, row_count, mode == LGN_EMD_PAIRS_UPPER && ev1 && ev1 != ev0) != 0) return -1;
  LGN_CHECK_ARG(ev0 && s0 && s1, "emd_pairs_grad: null pointer (ev0, s0, s1)");
  if (mode == LGN_EMD_PAIRS_UPPER) ev1 = ev0;
  LGN_CHECK_ARG(ev1, "emd_pairs_grad: null pointer (ev1)");
  lgn_emd_opts o{1.0, 1.0, 0, 0};
  if (opts) o = *opts;
  LGN_CHECK_ARG(o.R > 0.0 && o.R < INFINITY, "emd_pairs_grad: R = %g (need a finite R > 0)", o.R);
  LGN_CHECK_ARG(o.beta > 0.0 && o.beta < INFINITY, "emd_pairs_grad: beta = %g (need a finite beta > 0)", o.beta);
  o.norm = o.norm != 0, o.periodic_phi = o.periodic_phi != 0;
  long long p_begin, P;
  range_pairs(mode, B0, B1, row_begin, row_count, p_begin, P);
  if (emd_check_work("emd_pairs_grad", P < 1 ? 1 : P, n > m ? n : m, work, work_bytes) != 0) return -1;
  const PairsGradArgs a{ev0, ev1, mode, p_begin, P, B0, B1, n, m, o, row_begin, row_count, emd, s0, s1, status, static_cast<double*>(work)};
  return launch_pairs_grad(a, (hipStream_t)stream);
}

int lgn_emd_pairs_grad_reduce_f64(const double* s0, const double* s1, const double* G, int B0, int B1, int n, int m, int mode, int row_begin,
                                  int row_count, double* g0, double* g1, void* stream) {
  if (check_shape("emd_pairs_grad_reduce", mode, B0, B1, n, m, row_begin, row_count, false) != 0) return -1;
  LGN_CHECK_ARG(s0 && s1, "emd_pairs_grad_reduce: null pointer (s0, s1)");
  LGN_CHECK_ARG(g0 || g1, "emd_pairs_grad_reduce: no output (g0 and g1 are both null)");
  LGN_CHECK_ARG(mode != LGN_EMD_PAIRS_UPPER || !g1, "emd_pairs_grad_reduce: UPPER sums both roles of an event into g0; g1 must be null");
  const long long count0 = !g0 ? 0 : (mode == LGN_EMD_PAIRS_UPPER ? (long long)B0 : (long long)row_count) * n * 3;
  const long long count1 = g1 ? (long long)B1 * m * 3 : 0;
  const long long blocks = (count0 + count1 + REDUCE_BLOCK - 1) / REDUCE_BLOCK;
  hipLaunchKernelGGL(emd_pairs_grad_reduce_kernel, dim3((unsigned)blocks), dim3(REDUCE_BLOCK), 0, (hipStream_t)stream, s0, s1, G, B0, B1, n, m,
                     mode, row_begin, row_count, g0, g1, count0, count1);
  LGN_CHECK_LAUNCH();
  return 0;
}

}  // extern "C"
