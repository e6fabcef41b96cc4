// lgn-autoencoder_amd/csrc/emd_pairs.hip -- matrices of energy mover's distances and energyflow's options: energyflow.emd.emds (every
// event of one set against every event of another, or of one set against itself) and the R, beta, norm and periodic_phi arguments of
// energyflow.emd.emd, around the solver of emd.hip (emd_wave.hpp: one wavefront per pair, successive shortest paths).
// Entry points: lgn_emd_pairs_f64, lgn_emd_pairs_decode.  include/lgn_amd.h states the definition of every option.
//
// A persistent grid strides over the pair numbers p in [0, P); emd_plan.hpp decodes p into the events (i, j) of the three pair modes.
// A wave stages rows and columns, solves and writes exactly as emd_kernel does; the staging, the sums, the fictitious particle and the
// objective are emd.hip's statements in emd.hip's order, so that at default options every output has emd_kernel's bits.  They are
// repeated here, not shared: emd.hip's kernels keep their instructions.
//
// The options are a second instantiation (OPT): its cost functor applies the periodic minimum image, beta, and the staging divides
// each event's weights by that event's sum (norm).  At default options the OPT = false kernels run, whose cost is emd.hip's EmdCost.
//
// Floating-point contraction is OFF for this file (pragma below and the Makefile), as for emd.hip.
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

// The waves the pairs are dealt to, one per workgroup (DESIGN 8.1c has the measurements).  A pair takes as long as its events make it,
// so workgroups are handed out finest when each solves one pair: up to EMD_PAIRS_GRID pairs that is what happens, and the kernel then
// keeps step with emd_kernel on the gathered pairs; fewer, longer-lived workgroups lose to the tail and, at a stride that divides B1,
// to waves that meet the same column event in every pair.  Both counts are primes, so that beyond them the stride is coprime to B1.
constexpr int EMD_PAIRS_GRID = 1048573;        // flow in LDS
constexpr int EMD_PAIRS_GLOBAL_WAVES = 2039;   // flow in the workspace: resident waves only, below EMD_GLOBAL_WAVES slices
constexpr int EMD_AUG_PER_NODE = 16;           // emd.hip's cap of the augmentations of one problem per node
enum { BETA_ONE = 0, BETA_TWO = 1, BETA_POW = 2 };

static_assert(EMD_NMAX == LGN_EMD_NMAX, "include/lgn_amd.h and emd_wave.hpp agree on the largest event");
static_assert(EMD_PAIRS_GLOBAL_WAVES <= EMD_GLOBAL_WAVES, "lgn_emd_workspace_bytes holds a slice for every wave");

// c[i][j] = theta_ij^beta, 1 to or from the fictitious node; rows from LDS, columns in registers.  OPT = false is emd.hip's EmdCost.
template <int K, bool OPT>
struct EmdPairCost {
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

// ev0 [B0][n][3], ev1 [B1][m][3] (ev0 itself in UPPER mode); the outputs in the layouts of include/lgn_amd.h.  One wave per
// workgroup, with emd_kernel's LDS (emd_plan.hpp) and, on the workspace path, its own slice of `work`.
template <int K, class Flow, bool OPT>
__global__ __launch_bounds__(64) void emd_pairs_kernel(const double* __restrict__ ev0, const double* __restrict__ ev1, int mode, long long P,
                                                       int B0, int B1, int n, int m, lgn_emd_opts opt, double* __restrict__ emd,
                                                       double* __restrict__ flow, double* __restrict__ dual0, double* __restrict__ dual1,
                                                       int* __restrict__ status, double* __restrict__ work) {
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

  if (mode == LGN_EMD_PAIRS_UPPER)         // the diagonal: +0.0 with status 0, whatever the event holds
    for (long long d = slot * 64 + lane; d < B0; d += slots * 64) emd[d * B0 + d] = 0.0, status[d * B0 + d] = 0;

  for (long long p = slot; p < P; p += slots) {
    int pi, pj;
    emd_pairs_decode(mode, p, B0, B1, pi, pj);
    const double* __restrict__ a0 = ev0 + (size_t)pi * n * 3;
    const double* __restrict__ a1 = ev1 + (size_t)pj * m * 3;
    wave_sync();                           // the LDS of the previous pair is free
    EmdPairCost<K, OPT> cf;
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
      if (dual1) finish_duals<K>(cf, rows, cols, rs, had, v);
    }
    if (lane == 0) {
      if (mode == LGN_EMD_PAIRS_UPPER) {
        const size_t ij = (size_t)pi * B0 + pj, ji = (size_t)pj * B0 + pi;
        emd[ij] = score, emd[ji] = score;
        status[ij] = st, status[ji] = st;
      } else {
        emd[p] = score;
        status[p] = st;
      }
    }
    // (ALIGNED only: the host refuses these outputs in the other modes)
    if (flow) {
      double* fo = flow + (size_t)p * rows * cols;
      for (int i = 0; i < rows; ++i) {
#pragma unroll
        for (int k = 0; k < K; ++k) {
          const int j = lane + 64 * k;
          if (j < cols) fo[(size_t)i * cols + j] = st ? NAN : F.get(i, j);
        }
      }
    }
    if (dual0)
      for (int i = lane; i < rows; i += 64) dual0[(size_t)p * rows + i] = st ? NAN : rs.u[i];
    if (dual1) {
#pragma unroll
      for (int k = 0; k < K; ++k)
        if (lane + 64 * k < cols) dual1[(size_t)p * cols + lane + 64 * k] = st ? NAN : v[k];
    }
  }
}

struct PairsArgs {
  const double *ev0, *ev1;
  int mode;
  long long P;
  int B0, B1, n, m;
  lgn_emd_opts opt;
  double *emd, *flow, *dual0, *dual1;
  int* status;
  double* work;
};

template <int K, class Flow, bool OPT>
int launch_pairs_kfo(const PairsArgs& a, int grid, size_t smem, hipStream_t st) {
  return lds_launch(emd_pairs_kernel<K, Flow, OPT>, "emd_pairs", dim3(grid), dim3(64), smem, st, a.ev0, a.ev1, a.mode, a.P, a.B0, a.B1, a.n,
                    a.m, a.opt, a.emd, a.flow, a.dual0, a.dual1, a.status, a.work);
}

template <int K, class Flow>
int launch_pairs_kf(const PairsArgs& a, int grid, size_t smem, hipStream_t st) {
  const bool optioned = a.opt.beta != 1.0 || a.opt.norm || a.opt.periodic_phi;
  return optioned ? launch_pairs_kfo<K, Flow, true>(a, grid, smem, st) : launch_pairs_kfo<K, Flow, false>(a, grid, smem, st);
}

int launch_pairs(const PairsArgs& a, hipStream_t st) {
  const int N = a.n > a.m ? a.n : a.m;
  const bool in_lds = emd_flow_in_lds(N);
  const size_t smem = (size_t)emd_lds_total(a.n, a.m, in_lds);
  // P == 0 (UPPER, one event): one workgroup writes the diagonal
  const long long waves_max = in_lds ? EMD_PAIRS_GRID : EMD_PAIRS_GLOBAL_WAVES;
  const int grid = (int)(a.P < 1 ? 1 : (a.P < waves_max ? a.P : waves_max));
  const int K = (a.m + 1 + 63) / 64;
#define LGN_EMD_CASE(KK) \
  if (K == KK) return in_lds ? launch_pairs_kf<KK, FlowLds>(a, grid, smem, st) : launch_pairs_kf<KK, FlowGlobal>(a, grid, smem, st);
  LGN_EMD_CASE(1)
  LGN_EMD_CASE(2)
  LGN_EMD_CASE(3)
#undef LGN_EMD_CASE
  set_error("emd_pairs: m = %d needs more than three columns per lane", a.m);
  return -1;
}

}  // namespace
}  // namespace lgn

using namespace lgn;

extern "C" {

int lgn_emd_pairs_decode(int mode, long long p, int B0, int B1, int* i, int* j) {
  LGN_CHECK_ARG(mode == LGN_EMD_PAIRS_FULL || mode == LGN_EMD_PAIRS_UPPER || mode == LGN_EMD_PAIRS_ALIGNED, "emd_pairs_decode: unknown mode %d",
                mode);
  LGN_CHECK_ARG(B0 >= 1 && B1 >= 1, "emd_pairs_decode: B0 = %d, B1 = %d (need both >= 1)", B0, B1);
  LGN_CHECK_ARG(mode == LGN_EMD_PAIRS_FULL || B0 == B1, "emd_pairs_decode: B0 = %d != B1 = %d outside the FULL mode", B0, B1);
  LGN_CHECK_ARG(i && j, "emd_pairs_decode: null pointer (i, j)");
  const long long P = emd_pairs_count(mode, B0, B1);
  LGN_CHECK_ARG(p >= 0 && p < P, "emd_pairs_decode: p = %lld outside 0 .. %lld", p, P - 1);
  emd_pairs_decode(mode, p, B0, B1, *i, *j);
  return 0;
}

int lgn_emd_pairs_f64(const double* ev0, const double* ev1, int B0, int B1, int n, int m, int mode, const lgn_emd_opts* opts, double* emd,
                      double* flow, double* dual0, double* dual1, int* status, void* work, long long work_bytes, void* stream) {
  LGN_CHECK_ARG(mode == LGN_EMD_PAIRS_FULL || mode == LGN_EMD_PAIRS_UPPER || mode == LGN_EMD_PAIRS_ALIGNED, "emd_pairs: unknown mode %d", mode);
  LGN_CHECK_ARG(B0 >= 1 && B1 >= 1, "emd_pairs: B0 = %d, B1 = %d (need both >= 1)", B0, B1);
  LGN_CHECK_ARG(n >= 1 && n <= LGN_EMD_NMAX && m >= 1 && m <= LGN_EMD_NMAX, "emd_pairs: n = %d, m = %d outside 1 .. %d", n, m, LGN_EMD_NMAX);
  LGN_CHECK_ARG(ev0 && emd && status, "emd_pairs: null pointer (ev0, emd, status)");
  if (mode == LGN_EMD_PAIRS_UPPER) {
    LGN_CHECK_ARG(n == m && B0 == B1, "emd_pairs: UPPER is one set against itself: n = %d, m = %d, B0 = %d, B1 = %d", n, m, B0, B1);
    LGN_CHECK_ARG(!ev1 || ev1 == ev0, "emd_pairs: UPPER takes ev1 NULL or ev0 itself");
    ev1 = ev0;
  } else {
    LGN_CHECK_ARG(ev1, "emd_pairs: null pointer (ev1)");
  }
  LGN_CHECK_ARG(mode != LGN_EMD_PAIRS_ALIGNED || B0 == B1, "emd_pairs: ALIGNED needs B0 == B1; got %d and %d", B0, B1);
  lgn_emd_opts o{1.0, 1.0, 0, 0};
  if (opts) o = *opts;
  LGN_CHECK_ARG(o.R > 0.0 && o.R < INFINITY, "emd_pairs: R = %g (need a finite R > 0)", o.R);
  LGN_CHECK_ARG(o.beta > 0.0 && o.beta < INFINITY, "emd_pairs: beta = %g (need a finite beta > 0)", o.beta);
  o.norm = o.norm != 0, o.periodic_phi = o.periodic_phi != 0;
  LGN_CHECK_ARG(mode == LGN_EMD_PAIRS_ALIGNED || (!flow && !dual0 && !dual1), "emd_pairs: flow and duals are outputs of the ALIGNED mode only");
  const long long P = emd_pairs_count(mode, B0, B1);
  if (emd_check_work("emd_pairs", P < 1 ? 1 : P, n > m ? n : m, work, work_bytes) != 0) return -1;
  const PairsArgs a{ev0, ev1, mode, P, B0, B1, n, m, o, emd, flow, dual0, dual1, status, static_cast<double*>(work)};
  return launch_pairs(a, (hipStream_t)stream);
}

}  // extern "C"
