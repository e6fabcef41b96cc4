// lgn-autoencoder_amd/csrc/emd_grad_opts.hip -- the gradient of the energy mover's distance under energyflow's options (R, beta, norm,
// periodic_phi of include/lgn_amd.h), for aligned pairs of events and for Cartesian jets on their relative-polar frames.
// Entry points: lgn_emd_grad_opts_f64, lgn_emd_relative_opts_f64.  At default options both hand the call to emd.hip's entry points
// (lgn_emd_grad_f64, lgn_emd_relative_grad_f64, lgn_emd_relative_f64), whose bits they therefore give; the kernels here run otherwise.
//
// One wavefront per pair (emd_wave.hpp).  What the wave does for its pair is emd_dev.hpp, shared with the loss stage of the whole-step
// calls (emd_loss.hip): the staging, the sums, the tolerance, the solve, the objective and finish_duals are the statements of
// emd_pairs_kernel<K, Flow, OPT = true> in its order (REL: the frame staging of emd_kernel<REL> in front of them), so that the value
// has the bits of lgn_emd_pairs_f64 in its ALIGNED mode.  The epilogue is emd_gradients of emd.hip generalised.  With dy = y_i - y'_j,
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
#include "emd_dev.hpp"

namespace lgn {
namespace {

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
    cf.y = ry, cf.phi = rphi, cf.n = n, cf.m = m, cf.lane = lane;
    cf.options(opt);
    double dem[K], v[K];
    bool bad = false;
    double p0 = 0.0, p1 = 0.0;
    if (REL) {
      emd_stage_rel<K>(x0, x1, n, m, lane, rs.sup, ry, rphi, jet, dem, cf.qy, cf.qphi, bad, p0, p1);
    } else {
      for (int i = lane; i < rows; i += 64) {
        double w = 0.0, y = 0.0, ph = 0.0;
        if (i < n) {
          const double* x = x0 + (size_t)i * 3;
          w = x[0], y = x[1], ph = x[2];
          bad |= !emd_finite(w) || !emd_finite(y) || !emd_finite(ph) || w < 0.0;
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
          bad |= !emd_finite(w) || !emd_finite(y) || !emd_finite(ph) || w < 0.0;
        }
        dem[k] = w, cf.qy[k] = y, cf.qphi[k] = ph;
        p1 = p1 + w;
      }
    }
    const bool norm = opt.norm;
    double T0, T1, score;
    const int st = emd_solve_opts<K>(cf, rs, F, norm, grad || dual1, bad, p0, p1, dem, v, T0, T1, score);
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
