// lgn-autoencoder_amd/csrc/emd_dev.hpp -- what one wavefront does for one EMD problem, as device functions: the relative-polar staging of a
// pair of Cartesian jets, the cost under energyflow's options, the solve with its sums, tolerance, objective and finished duals, the
// gradient epilogue, and the way back from the relative-polar frame to the Cartesian jets.  ONE copy, shared by the kernels of
// emd.hip (staging, p4_polar_bwd, emd_rel_to_cartesian), of emd_grad_opts.hip (all of it) and by the loss stage of the whole-step
// calls (emd_loss.hip: all of it, on jets that sit in LDS).  The pointers are plain: global memory or LDS.
//
// The formulas are in the headers of emd.hip (the problem, the LP sensitivities) and emd_grad_opts.hip (the options).  Every statement
// rounds one operation at a time: contraction is OFF from here on in an including file, so a file whose other code contracts (the
// output mix of net_dev.hpp) includes that code first, as assign_loss.hip does with lsap_wave.hpp.
#pragma once
#pragma clang fp contract(off)

#include <math.h>

#include "../../include/lgn_amd.h"
#include "emd_wave.hpp"
#include "polar_dev.hpp"

namespace lgn {

constexpr int EMD_AUG_PER_NODE = 16;           // cap of the augmentations of one problem per node
enum { BETA_ONE = 0, BETA_TWO = 1, BETA_POW = 2 };

static_assert(EMD_NMAX == LGN_EMD_NMAX, "include/lgn_amd.h and emd_wave.hpp agree on the largest event");

__device__ __forceinline__ bool emd_finite(double x) { return fabs(x) < INFINITY; }      // false for NaN and +-inf

// The relative-polar frames of the Cartesian jets x0 [n][4] (rows) and x1 [m][4] (columns), staged as anomaly_scores_kernel stages
// its components 16..18: w = pT / (J_pT + 1e-16), y = eta - J_eta, phi = wrap(phi - J_phi), J the jet's own sum (rows in order).
// Rows go to sup / ry / rphi [n + 1] (the fictitious row n gets zeros), columns to this lane's dem / qy / qphi; jet [2][4] receives
// the two sums.  bad, p0, p1 accumulate the lane's validity flag and weight sums.
template <int K>
__device__ __forceinline__ void emd_stage_rel(const double* x0, const double* x1, int n, int m, int lane, double* sup, double* ry,
                                              double* rphi, double* jet, double (&dem)[K], double (&qy)[K], double (&qphi)[K],
                                              bool& bad, double& p0, double& p1) {
  const int rows = n + 1;
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
      bad |= !emd_finite(w) || !emd_finite(y) || !emd_finite(ph) || !emd_finite(x[0]) || w < 0.0;
    }
    sup[i] = w, ry[i] = y, rphi[i] = ph;
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
      bad |= !emd_finite(w) || !emd_finite(y) || !emd_finite(ph) || !emd_finite(x[0]) || w < 0.0;
    }
    dem[k] = w, qy[k] = y, qphi[k] = ph;
    p1 = p1 + w;
  }
}

// The gradient of p4_polar (polar_dev.hpp): (g_pt, g_eta, g_phi) -> (g_px, g_py, g_pz).  At pt == 0 the 0/0 of the root and of atan2
// reads as 0: such a particle gets no direct term.
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

// One side of the REL form: the gradients (gw, gy, gp)(k) with respect to the relative-polar frame of particle lane + 64 k of the
// jet x [n][4], whose sum is J [4], become out [n][4].  Every particle, weightless ones included, receives the jet-sum term.
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

// c[i][j] = theta_ij^beta, 1 to or from the fictitious node; rows from LDS, columns in registers: emd_pairs.hip's EmdPairCost<K, true>.
template <int K>
struct EmdOptCost {
  const double *y, *phi;       // [n + 1]
  int n, m, lane;
  double R, beta;
  int beta_mode, periodic;
  double qy[K], qphi[K];
  __device__ __forceinline__ void options(const lgn_emd_opts& opt) {
    R = opt.R, beta = opt.beta, periodic = opt.periodic_phi;
    beta_mode = opt.beta == 1.0 ? BETA_ONE : (opt.beta == 2.0 ? BETA_TWO : BETA_POW);
  }
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

// One staged problem, solved: rs.sup [n + 1] and dem hold the weights as staged, (bad, p0, p1) this lane's flag and partial sums.
// The statements of emd_pairs_kernel<K, Flow, OPT = true> in its order: the sums, the empty test, norm, the fictitious particle, the
// tolerance, emd_wave, the objective and (duals) finish_duals.  Returns the status (LGN_EMD_* bits, the same on every lane); T0, T1
// are the sums as staged (what norm divides by), score the objective (NaN when flagged), v the column potentials.
template <int K, class Flow>
__device__ __forceinline__ int emd_solve_opts(const EmdOptCost<K>& cf, const EmdRows& rs, const Flow& F, bool norm, bool duals, bool bad,
                                              double p0, double p1, double (&dem)[K], double (&v)[K], double& T0, double& T1,
                                              double& score) {
  const int n = cf.n, m = cf.m, lane = cf.lane, rows = n + 1, cols = m + 1;
  int st = __ballot(bad) ? LGN_EMD_INVALID : 0;
  double S0 = wave_sum(p0), S1 = wave_sum(p1);
  T0 = S0, T1 = S1;                      // the sums as given: what norm divides by
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
  score = NAN;
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
    if (duals) finish_duals<K>(cf, rows, cols, rs, had, v);
  }
  return st;
}

// The weight of particle i of one event as the kernel stages it, before norm: column 0 of an event [n][3], or pT / (jet pT + 1e-16)
// of a Cartesian jet [n][4] whose sum is J [4] (REL).
template <bool REL>
__device__ __forceinline__ double staged_weight(const double* __restrict__ x, const double* J, int i) {
  if (!REL) return x[3 * i];
  const double px = x[4 * i + 1], py = x[4 * i + 2];               // (the pt of p4_polar, polar_dev.hpp)
  return sqrt(px * px + py * py) / (sqrt(J[1] * J[1] + J[2] * J[2]) + POLAR_EPS);
}

// The gradient epilogue of one solved pair (the header of emd_grad_opts.hip): F the optimal flow, rs.u and v the finished potentials,
// S0 and S1 the sums of the weights as staged (before norm).  x0, x1: this pair's inputs (events, REL: Cartesian jets, J their sums
// [2][4]).  g0, g1: this pair's outputs, each nullable; a flagged pair gets NaN.  Overwrites rs.dist and rs.sup.
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

}  // namespace lgn
