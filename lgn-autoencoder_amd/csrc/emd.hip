// lgn-autoencoder_amd/csrc/emd.hip -- the energy mover's distance of two events of (pT, y, phi) particles, exactly: the reference's 22nd
// anomaly score "emd (relative coordinates)" (emd_loss() of utils/jet_analysis/anomaly_detection.py, which calls energyflow.emd.emd per
// jet with its defaults R = 1, beta = 1, norm = False, Euclidean ground distance, no periodic phi) and the generic batched solver behind it.
// Entry points: lgn_emd_f64, lgn_emd_relative_f64, lgn_emd_workspace_bytes, lgn_emd_lds_bytes, lgn_emd_debug_max_augmentations.
//
//   theta_ij = sqrt((y_i - y'_j)^2 + (phi_i - phi'_j)^2) / R
//   EMD      = min over f >= 0 of sum f_ij theta_ij + |sum pT - sum pT'|,  sum_j f_ij <= pT_i, sum_i f_ij <= pT'_j, sum f = min of the sums
// solved as the balanced transportation problem with one fictitious particle on the lighter side (it carries the weight difference
// at cost 1 to every particle of the other event).  One wavefront per pair of events (emd_wave.hpp); the first event's particles are
// the rows (LDS), the second's the columns (registers); row n and column m are the fictitious ones, of which at most one has weight.
// The flow matrix lives in LDS when it fits EMD_LDS_BUDGET together with the row state, else in the caller's workspace, where a fixed
// number of resident waves share the pairs.
//
// Floating-point contraction is OFF for this file (pragma below and the Makefile): costs and frames round one operation at a time, as
// the host restatement computes them, and the relative-polar frame is anomaly.hip's bit for bit.
#pragma clang fp contract(off)

#include <math.h>

#include <type_traits>

#include "common.hpp"
#include "../../include/lgn_amd.h"
#include "emd_wave.hpp"
#include "polar_dev.hpp"

namespace lgn {
namespace {

constexpr int EMD_LDS_BUDGET = 64 * 1024;      // plan-time budget of one wave's LDS (no opt-in launch attribute below it)
constexpr int EMD_GLOBAL_WAVES = 2048;         // resident waves of the workspace path: 8 per CU
constexpr int EMD_AUG_PER_NODE = 16;           // cap of the augmentations of one problem per node

static_assert(EMD_NMAX == LGN_EMD_NMAX, "include/lgn_amd.h and emd_wave.hpp agree on the largest event");
static_assert(EMD_ITER == LGN_EMD_ITER && EMD_INFEASIBLE == LGN_EMD_INFEASIBLE, "status bits of include/lgn_amd.h");

__device__ int g_emd_max_aug;                  // the largest augmentation count of any problem since the last reset (tools/emd_bench.py)

template <int K>
struct EmdCost {               // c[i][j] = theta_ij, 1 to or from the fictitious node; rows from LDS, columns in registers
  const double *y, *phi;       // [n + 1]
  int n, m, lane;
  double R;
  double qy[K], qphi[K];
  __device__ __forceinline__ double operator()(int i, int k) const {
    const int j = lane + 64 * k;
    if (i == n || j == m) return (i == n && j == m) ? 0.0 : 1.0;
    const double dy = y[i] - qy[k], dp = phi[i] - qphi[k];
    const double d = sqrt(dy * dy + dp * dp);
    return R == 1.0 ? d : d / R;
  }
};

__device__ __forceinline__ bool finite(double x) { return fabs(x) < INFINITY; }      // false for NaN and +-inf

__host__ __device__ constexpr long long emd_lds_doubles(int n, int m, bool lds_flow) {
  return 5ll * (n + 1) + 8 + (lds_flow ? (long long)(n + 1) * (m + 1) : 0);
}
__host__ __device__ constexpr long long emd_lds_total(int n, int m, bool lds_flow) {
  return 8 * emd_lds_doubles(n, m, lds_flow) + 8ll * (n + 1);
}
inline bool emd_flow_in_lds(int N) { return emd_lds_total(N, N, true) <= EMD_LDS_BUDGET; }
inline long long emd_workspace(long long B, int N) {
  if (emd_flow_in_lds(N)) return 0;
  return (B < EMD_GLOBAL_WAVES ? B : EMD_GLOBAL_WAVES) * (long long)(N + 1) * (N + 1) * 8;
}

// REL: a0 = recons, a1 = target [B][n][4] Cartesian jets (n == m), staged into the relative-polar frame as anomaly_scores_kernel
// stages its components 16..18.  Otherwise a0 [B][n][3], a1 [B][m][3] events of (pT, y, phi).
template <int K, class Flow, bool REL>
__global__ __launch_bounds__(64) void emd_kernel(const double* __restrict__ a0, const double* __restrict__ a1, int B, int n, int m, double R,
                                                 double* __restrict__ emd, double* __restrict__ flow, double* __restrict__ dual0,
                                                 double* __restrict__ dual1, int* __restrict__ status, double* __restrict__ work) {
  extern __shared__ __align__(16) double lds[];
  const int rows = n + 1, cols = m + 1, lane = threadIdx.x & 63;
  constexpr bool LDS_FLOW = std::is_same<Flow, FlowLds>::value;
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

  for (long b = blockIdx.x; b < B; b += gridDim.x) {
    wave_sync();                           // the LDS of the previous pair is free
    EmdCost<K> cf;
    cf.y = ry, cf.phi = rphi, cf.n = n, cf.m = m, cf.lane = lane, cf.R = R;
    double dem[K], v[K];
    bool bad = false;
    double p0 = 0.0, p1 = 0.0;
    if (REL) {
      const size_t base = (size_t)b * n * 4;
      if (lane < 8) {                      // jet sums, rows in order 0 .. N-1
        const double* x = (lane < 4 ? a0 : a1) + base + (lane & 3);
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
          const double* x = a0 + base + 4 * i;
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
          const double* x = a1 + base + 4 * j;
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
          const double* x = a0 + ((size_t)b * n + i) * 3;
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
          const double* x = a1 + ((size_t)b * m + j) * 3;
          w = x[0], y = x[1], ph = x[2];
          bad |= !finite(w) || !finite(y) || !finite(ph) || w < 0.0;
        }
        dem[k] = w, cf.qy[k] = y, cf.qphi[k] = ph;
        p1 = p1 + w;
      }
    }
    int st = __ballot(bad) ? LGN_EMD_INVALID : 0;
    const double S0 = wave_sum(p0), S1 = wave_sum(p1);
    if (!st && !(S0 > 0.0) && !(S1 > 0.0)) st = LGN_EMD_EMPTY;
    double score = NAN;
    int n_aug = 0;
    bool had[K];
#pragma unroll
    for (int k = 0; k < K; ++k) had[k] = false;
    if (!st) {
      // the fictitious particle of the lighter event carries the difference
      if (lane == 0) rs.sup[n] = S1 > S0 ? S1 - S0 : 0.0;
#pragma unroll
      for (int k = 0; k < K; ++k) {
        if (lane + 64 * k == m) dem[k] = S0 > S1 ? S0 - S1 : 0.0;
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
      emd[b] = score;
      status[b] = st;
      if (n_aug > 0) atomicMax(&g_emd_max_aug, n_aug);
    }
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

template <int K, class Flow, bool REL>
int launch_emd_kf(const double* a0, const double* a1, int B, int n, int m, double R, double* emd, double* flow, double* dual0, double* dual1,
                  int* status, double* work, int grid, size_t smem, hipStream_t st) {
  emd_kernel<K, Flow, REL><<<grid, 64, smem, st>>>(a0, a1, B, n, m, R, emd, flow, dual0, dual1, status, work);
  LGN_CHECK_LAUNCH();
  return 0;
}

template <bool REL>
int launch_emd(const double* a0, const double* a1, int B, int n, int m, double R, double* emd, double* flow, double* dual0, double* dual1,
               int* status, double* work, hipStream_t st) {
  const int N = n > m ? n : m;
  const bool in_lds = emd_flow_in_lds(N);
  const size_t smem = (size_t)emd_lds_total(n, m, in_lds);
  const int grid = in_lds ? B : (B < EMD_GLOBAL_WAVES ? B : EMD_GLOBAL_WAVES);
  const int K = (m + 1 + 63) / 64;
#define LGN_EMD_CASE(KK)                                                                                                               \
  if (K == KK)                                                                                                                         \
    return in_lds ? launch_emd_kf<KK, FlowLds, REL>(a0, a1, B, n, m, R, emd, flow, dual0, dual1, status, work, grid, smem, st)          \
                  : launch_emd_kf<KK, FlowGlobal, REL>(a0, a1, B, n, m, R, emd, flow, dual0, dual1, status, work, grid, smem, st);
  LGN_EMD_CASE(1)
  LGN_EMD_CASE(2)
  LGN_EMD_CASE(3)
#undef LGN_EMD_CASE
  set_error("emd: m = %d needs more than three columns per lane", m);
  return -1;
}

int check_work(const char* who, int B, int N, const void* work, long long work_bytes) {
  const long long need = emd_workspace(B, N);
  if (need == 0) return 0;
  LGN_CHECK_ARG(work, "%s: N = %d keeps the flow in a workspace: null work (lgn_emd_workspace_bytes: %lld bytes)", who, N, need);
  LGN_CHECK_ARG(work_bytes >= need, "%s: workspace of %lld bytes is too short (%lld needed)", who, work_bytes, need);
  LGN_CHECK_ARG((reinterpret_cast<uintptr_t>(work) & 7) == 0, "%s: the workspace must be 8-byte aligned", who);
  return 0;
}

}  // namespace
}  // namespace lgn

using namespace lgn;

extern "C" {

long long lgn_emd_workspace_bytes(int B, int N) {
  if (B < 1 || N < 1 || N > LGN_EMD_NMAX) {
    set_error("emd_workspace_bytes: B = %d, N = %d (B >= 1, 1 <= N <= %d)", B, N, LGN_EMD_NMAX);
    return -1;
  }
  return emd_workspace(B, N);
}

long long lgn_emd_lds_bytes(int N) {
  if (N < 1 || N > LGN_EMD_NMAX) {
    set_error("emd_lds_bytes: N = %d outside 1 .. %d", N, LGN_EMD_NMAX);
    return -1;
  }
  return emd_lds_total(N, N, emd_flow_in_lds(N));
}

int lgn_emd_f64(const double* ev0, const double* ev1, int B, int n, int m, double R, double* emd, double* flow, double* dual0, double* dual1,
                int* status, void* work, long long work_bytes, void* stream) {
  LGN_CHECK_ARG(B >= 1, "emd: B = %d (need B >= 1)", B);
  LGN_CHECK_ARG(n >= 1 && n <= LGN_EMD_NMAX && m >= 1 && m <= LGN_EMD_NMAX, "emd: n = %d, m = %d outside 1 .. %d", n, m, LGN_EMD_NMAX);
  LGN_CHECK_ARG(ev0 && ev1 && emd && status, "emd: null pointer (ev0, ev1, emd, status)");
  LGN_CHECK_ARG(R > 0.0 && R < INFINITY, "emd: R = %g (need a finite R > 0)", R);
  if (check_work("emd", B, n > m ? n : m, work, work_bytes) != 0) return -1;
  return launch_emd<false>(ev0, ev1, B, n, m, R, emd, flow, dual0, dual1, status, static_cast<double*>(work), (hipStream_t)stream);
}

int lgn_emd_relative_f64(const double* recons, const double* target, int B, int N, double* emd, int* status, void* work, long long work_bytes,
                         void* stream) {
  LGN_CHECK_ARG(B >= 1, "emd_relative: B = %d (need B >= 1)", B);
  LGN_CHECK_ARG(N >= 1 && N <= LGN_EMD_NMAX, "emd_relative: N = %d outside 1 .. %d", N, LGN_EMD_NMAX);
  LGN_CHECK_ARG(recons && target && emd && status, "emd_relative: null pointer (recons, target, emd, status)");
  if (check_work("emd_relative", B, N, work, work_bytes) != 0) return -1;
  return launch_emd<true>(recons, target, B, N, N, 1.0, emd, nullptr, nullptr, nullptr, status, static_cast<double*>(work),
                          (hipStream_t)stream);
}

int lgn_emd_debug_max_augmentations(int* out, int reset) {
  int v = 0;
  hipError_t e = hipMemcpyFromSymbol(&v, HIP_SYMBOL(g_emd_max_aug), sizeof(int));
  if (e == hipSuccess && reset) {
    const int zero = 0;
    e = hipMemcpyToSymbol(HIP_SYMBOL(g_emd_max_aug), &zero, sizeof(int));
  }
  if (e != hipSuccess) {
    set_error("emd_debug_max_augmentations: %s", hipGetErrorString(e));
    return (int)e;
  }
  if (out) *out = v;
  return 0;
}

}  // extern "C"
