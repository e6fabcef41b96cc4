// lgn-autoencoder_amd/csrc/emd_grad_opts.hip -- the gradient of the energy mover's distance under energyflow's options (R, beta, norm,
// periodic_phi of include/lgn_amd.h), for aligned pairs of events and for Cartesian jets on their relative-polar frames.
// Entry points: lgn_emd_grad_opts_f64, lgn_emd_relative_opts_f64.  At default options both hand the call to emd.hip's entry points
// (lgn_emd_grad_f64, lgn_emd_relative_grad_f64, lgn_emd_relative_f64), whose bits they therefore give; the kernels here run otherwise.
//
// One wavefront per pair (emd_wave.hpp).  The staging, the sums, the tolerance, the solve, the objective and finish_duals are the
// statements of emd_pairs_kernel<K, Flow, OPT = true> in its order (REL: the frame staging of emd_kernel<REL> in front of them), so that
// the value has the bits of lgn_emd_pairs_f64 in its ALIGNED mode.  They are repeated here, not shared: the kernels of emd.hip and
// emd_pairs.hip keep their instructions.  The epilogue is emd_gradients of emd.hip generalised.  With dy = y_i - y'_j,
// D = phi_i - phi'_j, dphi = D or its minimum image pi - |pi - |D||, theta_ij = sqrt(dy^2 + dphi^2) / R, f the optimal flow in the
// units of the staged weights, u and v the finished potentials, S0 = sum pT and S1 = sum pT' as given:
//   s_ij      = 1 without periodic_phi, sign(D) sign(pi - |D|) with it (0 at D = 0 and at |D| = pi)
//   k_ij      = f_ij beta theta_ij^(beta - 2) / R^2 where theta_ij > 0, else 0
//   dE/dy_i   =  sum_j k_ij dy            dE/dy'_j   = -sum_i k_ij dy
//   dE/dphi_i =  sum_j k_ij dphi s_ij     dE/dphi'_j = -sum_i k_ij dphi s_ij
//   norm off:  dE/dpT_i = u_i - [S1 > S0] u_n + [S0 > S1] v_m             (dE/dpT'_j alike: emd.hip's formula)
//   norm on :  dE/dpT_i = (u_i - sum_k a_k u_k) / S0, a = pT / S0          dE/dpT'_j = (v_j - sum_k b_k v_k) / S1, b = pT' / S1
// k_ij is f / (R d) at beta = 1 (d = R theta: emd.hip's term), f (2 / R^2) at beta = 2, and f / (R d) times beta pow(theta, beta - 1)
// otherwise.  Column gradients accumulate per lane over the rows, a row's gradient is one wave reduction; rs.dist and rs.sup, free
// after the solve, hold the rows' position gradients.  The solver consumes the staged weights, so the epilogue stages a and b of the
// norm form once more from the inputs (the same operations, the same bits).
//
// Floating-point contraction is OFF for this file (pragma below and the Makefile), as for emd.hip and emd_pairs.hip.
#pragma clang fp contract(off)

#include <math.h>

#include <type_traits>

#include "lds.hpp"
#include "../../include/lgn_amd.h"
#include "emd_plan.hpp"
#include "emd_wave.hpp"
#include "polar_dev.hpp"

namespace lgn {
namespace {

constexpr int EMD_AUG_PER_NODE = 16;           // emd.hip's cap of the augmentations of one problem per node
enum { BETA_ONE = 0, BETA_TWO = 1, BETA_POW = 2 };

static_assert(EMD_NMAX == LGN_EMD_NMAX, "include/lgn_amd.h and emd_wave.hpp agree on the largest event");

// c[i][j] = theta_ij^beta, 1 to or from the fictitious node; rows from LDS, columns in registers: emd_pairs.hip's EmdPairCost<K, true>.
template <int K>
struct EmdOptCost {
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
    if (periodic) {                            // pi - |pi - |dphi||, one rounded operation each
      const double a = M_PI - fabs(dp);
      dp = M_PI - fabs(a);
    }
    const double d = sqrt(dy * dy + dp * dp);
    const double t = R == 1.0 ? d : d / R;
    if (beta_mode == BETA_ONE) return t;
    return beta_mode == BETA_TWO ? t * t : pow(t, beta);
  }
};

__device__ __forceinline__ bool finite(double x) { return fabs(x) < INFINITY; }      // false for NaN and +-inf

// emd.hip's p4_polar_bwd: the gradient of p4_polar (polar_dev.hpp), (g_pt, g_eta, g_phi) -> (g_px, g_py, g_pz).  At pt == 0 the 0/0
// of the root and of atan2 reads as 0.
__device__ __forceinline__ void p4_polar_bwd(double px, double py, double pz, double g_pt, double g_eta, double g_phi, double& gx,
                                             double& gy, double& gz) {
  gx = gy = gz = 0.0;
  const double pt = sqrt(px * px + py * py);
  if (!(pt > 0.0)) return;
  const double q = pt + POLAR_EPS, z = pz / q;
  const double s = 1.0 / sqrt(1.0 + z * z);                    // d asinh(z) / dz
  const double gt = g_pt - (g_eta * s) * (z / q);              // dz / dpt = -pz / q^2
  const double X = px + POLAR_EPS, Y = py + POLAR_EPS, r2 = X * X + Y * Y;
  gx = gt * (px / pt) - g_phi * (Y / r2);
  gy = gt * (py / pt) + g_phi * (X / r2);
  gz = (g_eta * s) / q;
}

// emd.hip's emd_rel_to_cartesian: the gradients (gw, gy, gp)(k) with respect to the relative-polar frame of particle lane + 64 k of
// the jet x [n][4], whose sum is J [4], become out [n][4].  Every particle, weightless ones included, receives the jet-sum term.
template <int K, class GW, class GY, class GP>
__device__ __forceinline__ void emd_rel_to_cartesian(const double* __restrict__ x, const double* J, int n, int lane, GW gw, GY gy, GP gp,
                                                     double* __restrict__ out) {
  double jpT, jeta, jphi;
  p4_polar(J[1], J[2], J[3], jpT, jeta, jphi);
  const double q = jpT + POLAR_EPS;
  double sw = 0.0, sy = 0.0, sp = 0.0;
#pragma unroll
  for (int k = 0; k < K; ++k) {
    const int i = lane + 64 * k;
    if (i < n) {
      const double* p = x + 4 * i;
      sw = sw + gw(k) * sqrt(p[1] * p[1] + p[2] * p[2]);
      sy = sy + gy(k);
      sp = sp + gp(k);
    }
  }
  sw = wave_sum(sw), sy = wave_sum(sy), sp = wave_sum(sp);
  double jx, jy, jz;
  p4_polar_bwd(J[1], J[2], J[3], -(sw / (q * q)), -sy, -sp, jx, jy, jz);
#pragma unroll
  for (int k = 0; k < K; ++k) {
    const int i = lane + 64 * k;
    if (i < n) {
      const double* p = x + 4 * i;
      double dx, dy, dz;
      p4_polar_bwd(p[1], p[2], p[3], gw(k) / q, gy(k), gp(k), dx, dy, dz);
      out[4 * i] = 0.0, out[4 * i + 1] = dx + jx, out[4 * i + 2] = dy + jy, out[4 * i + 3] = dz + jz;
    }
  }
}

// The weight of particle i of one event as the kernel stages it, before norm: column 0 of an event [n][3], or pT / (jet pT + 1e-16)
// of a Cartesian jet [n][4] whose sum is J [4] (REL).
template <bool REL>
__device__ __forceinline__ double staged_weight(const double* __restrict__ x, const double* J, int i) {
  if (!REL) return x[3 * i];
  const double px = x[4 * i + 1], py = x[4 * i + 2];               // (the pt of p4_polar, polar_dev.hpp)
  return sqrt(px * px + py * py) / (sqrt(J[1] * J[1] + J[2] * J[2]) + POLAR_EPS);
}

// The gradient epilogue of one solved pair (the header of this file): F the optimal flow, rs.u and v the finished potentials, S0 and
// S1 the sums of the weights as staged (before norm).  x0, x1: this pair's inputs (events, REL: Cartesian jets, J their sums [2][4]).
// g0, g1: this pair's outputs, each nullable.  Overwrites rs.dist and rs.sup.
template <int K, class Flow, bool REL>
__device__ __forceinline__ void emd_opt_gradients(const EmdOptCost<K>& cf, const EmdRows& rs, const Flow& F, const double (&v)[K], int st,
                                                  bool norm, double S0, double S1, const double* __restrict__ x0,
                                                  const double* __restrict__ x1, const double* J, double* __restrict__ g0,
                                                  double* __restrict__ g1) {
  const int n = cf.n, m = cf.m, lane = cf.lane;
  constexpr int W = REL ? 4 : 3;
  if (st) {
    if (g0)
      for (int t = lane; t < n * W; t += 64) g0[t] = NAN;
    if (g1)
      for (int t = lane; t < m * W; t += 64) g1[t] = NAN;
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
        if (cf.periodic) {
          const double a = M_PI - fabs(dp);
          sgn = (dp > 0.0 ? 1.0 : (dp < 0.0 ? -1.0 : 0.0)) * (a > 0.0 ? 1.0 : (a < 0.0 ? -1.0 : 0.0));
          dp = M_PI - fabs(a);
        }
        const double d = sqrt(dy * dy + dp * dp);
        if (f > 0.0 && d > 0.0) {
          double t;
          if (cf.beta_mode == BETA_TWO) {
            t = f * two_over_R2;
          } else {
            t = f / (cf.R * d);                                // f / (R^2 theta)
            if (cf.beta_mode == BETA_POW) t = t * (cf.beta * pow(cf.R == 1.0 ? d : d / cf.R, bm1));
          }
          const double ty = t * dy, tp = (t * dp) * sgn;
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
  if (norm) {
    double au = 0.0, bv = 0.0;
    if (g0)
      for (int i = lane; i < n; i += 64) au = au + (staged_weight<REL>(x0, J, i) / S0) * rs.u[i];
    if (g1) {
#pragma unroll
      for (int k = 0; k < K; ++k)
        if (lane + 64 * k < m) bv = bv + (staged_weight<REL>(x1, J + 4, lane + 64 * k) / S1) * v[k];
    }
    c0 = -wave_sum(au), c1 = -wave_sum(bv), q0 = S0, q1 = S1;
  } else {
    const double un = rs.u[n], vm = lane_slot<K>(v, m);
    c0 = S1 > S0 ? -un : (S0 > S1 ? vm : 0.0), c1 = S0 > S1 ? -vm : (S1 > S0 ? un : 0.0);
  }
  auto w0 = [&](int i) { return norm ? (rs.u[i] + c0) / q0 : rs.u[i] + c0; };
  auto w1 = [&](int k) { return norm ? (v[k] + c1) / q1 : v[k] + c1; };
  if (REL) {
    // (n == m: a lane's rows are lane + 64 k, k < K, like its columns)
    if (g0)
      emd_rel_to_cartesian<K>(x0, J, n, lane, [&](int k) { return w0(lane + 64 * k); }, [&](int k) { return rs.dist[lane + 64 * k]; },
                              [&](int k) { return rs.sup[lane + 64 * k]; }, g0);
    if (g1)
      emd_rel_to_cartesian<K>(x1, J + 4, m, lane, w1, [&](int k) { return cy[k]; }, [&](int k) { return cp[k]; }, g1);
  } else {
    if (g0)
      for (int i = lane; i < n; i += 64) g0[3 * i] = w0(i), g0[3 * i + 1] = rs.dist[i], g0[3 * i + 2] = rs.sup[i];
    if (g1) {
#pragma unroll
      for (int k = 0; k < K; ++k) {
        const int j = lane + 64 * k;
        if (j < m) g1[3 * j] = w1(k), g1[3 * j + 1] = cy[k], g1[3 * j + 2] = cp[k];
      }
    }
  }
}

// REL: a0 = recons, a1 = target [B][n][4] Cartesian jets (n == m), staged into the relative-polar frame as emd_kernel<REL> stages
// them.  Otherwise a0 [B][n][3], a1 [B][m][3] events of (pT, y, phi).  g0, g1 (each nullable; both null: the value only) are
// [B][n][W], [B][m][W] with W = 3 (pT, y, phi), REL: 4 Cartesian.  One wave per workgroup with emd_kernel's LDS (emd_plan.hpp) and, on
// the workspace path, its own slice of `work`.  Two waves per SIMD are asked for: the workspace path keeps 8 waves per CU resident
// (EMD_GLOBAL_WAVES), which REL at K = 3 would otherwise miss by a few registers (DESIGN 8.1c has the figures).
template <int K, class Flow, bool REL>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(2))) void emd_grad_opts_kernel(const double* __restrict__ a0, const double* __restrict__ a1, int B, int n, int m,
                                                           lgn_emd_opts opt, double* __restrict__ emd, double* __restrict__ flow,
                                                           double* __restrict__ dual0, double* __restrict__ dual1,
                                                           int* __restrict__ status, double* __restrict__ work, double* __restrict__ g0,
                                                           double* __restrict__ g1) {
  extern __shared__ __align__(16) double lds[];
  const int rows = n + 1, cols = m + 1, lane = threadIdx.x & 63;
  constexpr bool LDS_FLOW = std::is_same<Flow, FlowLds>::value;
  constexpr int W = REL ? 4 : 3;
  EmdRows rs;
  rs.u = lds;
  rs.sup = rs.u + rows;
  rs.dist = rs.sup + rows;
  double* ry = rs.dist + rows;
  double* rphi = ry + rows;
  double* jet = rphi + rows;               // [2][4] jet 4-vectors (REL)
  double* fl = jet + 8;                    // [cols][rows] (LDS_FLOW)
  rs.pred = reinterpret_cast<int*>(fl + (LDS_FLOW ? rows * cols : 0));
  rs.vis = rs.pred + rows;
  Flow F;
  F.f = LDS_FLOW ? fl : work + (size_t)blockIdx.x * rows * cols;
  F.ld = rows;
  const bool grad = g0 || g1;

  for (long b = blockIdx.x; b < B; b += gridDim.x) {
    const double* __restrict__ x0 = a0 + (size_t)b * n * W;
    const double* __restrict__ x1 = a1 + (size_t)b * m * W;
    wave_sync();                           // the LDS of the previous pair is free
    EmdOptCost<K> cf;
    cf.y = ry, cf.phi = rphi, cf.n = n, cf.m = m, cf.lane = lane, cf.R = opt.R, cf.beta = opt.beta, cf.periodic = opt.periodic_phi;
    cf.beta_mode = opt.beta == 1.0 ? BETA_ONE : (opt.beta == 2.0 ? BETA_TWO : BETA_POW);
    double dem[K], v[K];
    bool bad = false;
    double p0 = 0.0, p1 = 0.0;
    if (REL) {
      if (lane < 8) {                      // jet sums, rows in order 0 .. N-1
        const double* x = (lane < 4 ? x0 : x1) + (lane & 3);
        double s = 0.0;
        for (int r = 0; r < n; ++r) s = s + x[4 * r];
        jet[lane] = s;
      }
      wave_sync();
      double jpT0, jeta0, jphi0, jpT1, jeta1, jphi1;
      p4_polar(jet[1], jet[2], jet[3], jpT0, jeta0, jphi0);
      p4_polar(jet[5], jet[6], jet[7], jpT1, jeta1, jphi1);
      for (int i = lane; i < rows; i += 64) {
        double w = 0.0, y = 0.0, ph = 0.0;
        if (i < n) {
          const double* x = x0 + 4 * i;
          double pT, eta, phi;
          p4_polar(x[1], x[2], x[3], pT, eta, phi);
          w = pT / (jpT0 + POLAR_EPS);
          y = eta - jeta0;
          ph = wrap_phi(phi - jphi0);
          bad |= !finite(w) || !finite(y) || !finite(ph) || !finite(x[0]) || w < 0.0;
        }
        rs.sup[i] = w, ry[i] = y, rphi[i] = ph;
        p0 = p0 + w;
      }
#pragma unroll
      for (int k = 0; k < K; ++k) {
        const int j = lane + 64 * k;
        double w = 0.0, y = 0.0, ph = 0.0;
        if (j < m) {
          const double* x = x1 + 4 * j;
          double pT, eta, phi;
          p4_polar(x[1], x[2], x[3], pT, eta, phi);
          w = pT / (jpT1 + POLAR_EPS);
          y = eta - jeta1;
          ph = wrap_phi(phi - jphi1);
          bad |= !finite(w) || !finite(y) || !finite(ph) || !finite(x[0]) || w < 0.0;
        }
        dem[k] = w, cf.qy[k] = y, cf.qphi[k] = ph;
        p1 = p1 + w;
      }
    } else {
      for (int i = lane; i < rows; i += 64) {
        double w = 0.0, y = 0.0, ph = 0.0;
        if (i < n) {
          const double* x = x0 + (size_t)i * 3;
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
          const double* x = x1 + (size_t)j * 3;
          w = x[0], y = x[1], ph = x[2];
          bad |= !finite(w) || !finite(y) || !finite(ph) || w < 0.0;
        }
        dem[k] = w, cf.qy[k] = y, cf.qphi[k] = ph;
        p1 = p1 + w;
      }
    }
    int st = __ballot(bad) ? LGN_EMD_INVALID : 0;
    double S0 = wave_sum(p0), S1 = wave_sum(p1);
    const double T0 = S0, T1 = S1;         // the sums as given: what norm divides by
    const bool norm = opt.norm;
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
      if (grad || dual1) finish_duals<K>(cf, rows, cols, rs, had, v);
    }
    if (lane == 0) {
      emd[b] = score;
      status[b] = st;
    }
    if (grad)
      emd_opt_gradients<K, Flow, REL>(cf, rs, F, v, st, norm, T0, T1, x0, x1, jet, g0 ? g0 + (size_t)b * n * W : nullptr,
                                      g1 ? g1 + (size_t)b * m * W : nullptr);
    if (flow) {
      double* fo = flow + (size_t)b * rows * cols;
      for (int i = 0; i < rows; ++i) {
#pragma unroll
        for (int k = 0; k < K; ++k) {
          const int j = lane + 64 * k;
          if (j < cols) fo[(size_t)i * cols + j] = st ? NAN : F.get(i, j);
        }
      }
    }
    if (dual0)
      for (int i = lane; i < rows; i += 64) dual0[(size_t)b * rows + i] = st ? NAN : rs.u[i];
    if (dual1) {
#pragma unroll
      for (int k = 0; k < K; ++k)
        if (lane + 64 * k < cols) dual1[(size_t)b * cols + lane + 64 * k] = st ? NAN : v[k];
    }
  }
}

struct GradOptsArgs {
  const double *a0, *a1;
  int B, n, m;
  lgn_emd_opts opt;
  double *emd, *flow, *dual0, *dual1;
  int* status;
  double *work, *g0, *g1;
};

template <int K, class Flow, bool REL>
int launch_grad_opts_kf(const GradOptsArgs& a, int grid, size_t smem, hipStream_t st) {
  return lds_launch(emd_grad_opts_kernel<K, Flow, REL>, "emd_grad_opts", dim3(grid), dim3(64), smem, st, a.a0, a.a1, a.B, a.n, a.m, a.opt,
                    a.emd, a.flow, a.dual0, a.dual1, a.status, a.work, a.g0, a.g1);
}

// (the grid of emd.hip's launch_emd: one workgroup per pair in LDS, EMD_GLOBAL_WAVES resident waves on the workspace)
template <bool REL>
int launch_grad_opts(const GradOptsArgs& a, hipStream_t st) {
  const int N = a.n > a.m ? a.n : a.m;
  const bool in_lds = emd_flow_in_lds(N);
  const size_t smem = (size_t)emd_lds_total(a.n, a.m, in_lds);
  const int grid = in_lds ? a.B : (a.B < EMD_GLOBAL_WAVES ? a.B : EMD_GLOBAL_WAVES);
  const int K = (a.m + 1 + 63) / 64;
#define LGN_EMD_CASE(KK) \
  if (K == KK) return in_lds ? launch_grad_opts_kf<KK, FlowLds, REL>(a, grid, smem, st) : launch_grad_opts_kf<KK, FlowGlobal, REL>(a, grid, smem, st);
  LGN_EMD_CASE(1)
  LGN_EMD_CASE(2)
  LGN_EMD_CASE(3)
#undef LGN_EMD_CASE
  set_error("emd_grad_opts: m = %d needs more than three columns per lane", a.m);
  return -1;
}

// opts (nullable) checked and normalised into o; returns whether every option is at its default (R aside)
int read_opts(const char* who, const lgn_emd_opts* opts, lgn_emd_opts& o, bool& optioned) {
  o = lgn_emd_opts{1.0, 1.0, 0, 0};
  if (opts) o = *opts;
  LGN_CHECK_ARG(o.R > 0.0 && o.R < INFINITY, "%s: R = %g (need a finite R > 0)", who, o.R);
  LGN_CHECK_ARG(o.beta > 0.0 && o.beta < INFINITY, "%s: beta = %g (need a finite beta > 0)", who, o.beta);
  o.norm = o.norm != 0, o.periodic_phi = o.periodic_phi != 0;
  optioned = o.beta != 1.0 || o.norm || o.periodic_phi;
  return 0;
}

}  // namespace
}  // namespace lgn

using namespace lgn;

extern "C" {

int lgn_emd_grad_opts_f64(const double* ev0, const double* ev1, int B, int n, int m, const lgn_emd_opts* opts, double* emd, double* g0,
                          double* g1, double* flow, double* dual0, double* dual1, int* status, void* work, long long work_bytes,
                          void* stream) {
  LGN_CHECK_ARG(B >= 1, "emd_grad_opts: B = %d (need B >= 1)", B);
  LGN_CHECK_ARG(n >= 1 && n <= LGN_EMD_NMAX && m >= 1 && m <= LGN_EMD_NMAX, "emd_grad_opts: n = %d, m = %d outside 1 .. %d", n, m,
                LGN_EMD_NMAX);
  LGN_CHECK_ARG(g0 || g1, "emd_grad_opts: no gradient output (g0 and g1 are both null; lgn_emd_pairs_f64 is the call without gradients)");
  LGN_CHECK_ARG(ev0 && ev1 && emd && status, "emd_grad_opts: null pointer (ev0, ev1, emd, status)");
  lgn_emd_opts o;
  bool optioned;
  if (read_opts("emd_grad_opts", opts, o, optioned) != 0) return -1;
  if (emd_check_work("emd_grad_opts", B, n > m ? n : m, work, work_bytes) != 0) return -1;
  if (!optioned) return lgn_emd_grad_f64(ev0, ev1, B, n, m, o.R, emd, g0, g1, flow, dual0, dual1, status, work, work_bytes, stream);
  const GradOptsArgs a{ev0, ev1, B, n, m, o, emd, flow, dual0, dual1, status, static_cast<double*>(work), g0, g1};
  return launch_grad_opts<false>(a, (hipStream_t)stream);
}

int lgn_emd_relative_opts_f64(const double* recons, const double* target, int B, int N, const lgn_emd_opts* opts, double* emd,
                              double* g_recons, double* g_target, int* status, void* work, long long work_bytes, void* stream) {
  LGN_CHECK_ARG(B >= 1, "emd_relative_opts: B = %d (need B >= 1)", B);
  LGN_CHECK_ARG(N >= 1 && N <= LGN_EMD_NMAX, "emd_relative_opts: N = %d outside 1 .. %d", N, LGN_EMD_NMAX);
  LGN_CHECK_ARG(recons && target && emd && status, "emd_relative_opts: null pointer (recons, target, emd, status)");
  LGN_CHECK_ARG(g_recons || !g_target, "emd_relative_opts: g_target without g_recons");
  lgn_emd_opts o;
  bool optioned;
  if (read_opts("emd_relative_opts", opts, o, optioned) != 0) return -1;
  if (emd_check_work("emd_relative_opts", B, N, work, work_bytes) != 0) return -1;
  if (!optioned && o.R == 1.0)
    return g_recons ? lgn_emd_relative_grad_f64(recons, target, B, N, emd, g_recons, g_target, status, work, work_bytes, stream)
                    : lgn_emd_relative_f64(recons, target, B, N, emd, status, work, work_bytes, stream);
  const GradOptsArgs a{recons, target, B, N, N, o, emd, nullptr, nullptr, nullptr, status, static_cast<double*>(work), g_recons, g_target};
  return launch_grad_opts<true>(a, (hipStream_t)stream);
}

}  // extern "C"
