// lgn-autoencoder_amd/csrc/anomaly.hip -- per-jet anomaly scores (the reference's anomaly_scores(),
// utils/jet_analysis/anomaly_detection.py) and a batched exact linear-sum-assignment solver.
//
// lsap_wave: one wavefront solves one n x n assignment problem with the shortest-augmenting-path algorithm (Crouse 2016) exactly
// as scipy.optimize.linear_sum_assignment runs it, so that col_ind is scipy's bit for bit, ties included:
//   - rows are augmented in order 0 .. n-1; the `remaining` column list starts as n-1, n-2, .., 0 and shrinks by swap-remove;
//   - reduced cost r = ((minVal + C[i][j]) - u[i]) - v[j], a column's shortest-path cost (spc) and path row change when r < spc;
//   - among the remaining columns at the minimal spc: the LAST one in `remaining` order that has no row yet, else the FIRST one;
//   - duals: u[cur] += minVal; u[i] += minVal - spc[col4row[i]] for the other visited rows; v[j] -= minVal - spc[j] for the
//     visited columns.
// Lanes own columns j = lane + 64 k (k < K): spc, v, row4col, path, visited and the position in `remaining` live in VGPRs.  The
// per-row state (u, col4row) lives in LDS.  A Dijkstra step is one wave-wide fp64 min, then the tie rule as a wave-wide max of a
// key (free flag | position | column).  The cost is a functor: read from memory, or computed from staged rows on the fly.
//
// Floating-point contraction is OFF for this file (pragma below): an FMA in the reduced cost changes which column wins an exact
// tie, and the frames / distances must round as the host computes them.
#pragma clang fp contract(off)

#include <math.h>

#include "common.hpp"
#include "../../include/lgn_amd.h"

namespace lgn {
namespace {

constexpr int NMAX = LGN_ANOMALY_NMAX;
constexpr int NSC = LGN_ANOMALY_NSCORES;
constexpr int LSAP_INFEASIBLE = 2;
constexpr double EPS = 1e-16;          // EPS_DEFAULT of the reference

__device__ __forceinline__ void wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}
__device__ __forceinline__ double wave_min(double x) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const double y = __shfl_xor(x, o);
    x = y < x ? y : x;
  }
  return x;
}
__device__ __forceinline__ int wave_max(int x) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) x = max(x, __shfl_xor(x, o));
  return x;
}
__device__ __forceinline__ double wave_sum(double x) {     // fixed butterfly order: every lane gets the same total
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) x = x + __shfl_xor(x, o);
  return x;
}
__device__ __forceinline__ bool bad_cost(double c) { return c != c || c == -INFINITY; }

// Solves the n x n problem whose cost cost(i, k) is C[i][lane + 64 k]; leaves col4row[0..n) in LDS.  Returns 0, or
// LSAP_INFEASIBLE (every remaining reduced cost infinite: scipy's "cost matrix is infeasible").  The caller has checked that no
// cost is NaN or -inf.  All control flow is wave-uniform.
template <int K, class Cost>
__device__ int lsap_wave(const Cost& cost, const int n, double* u, int* col4row) {
  const int lane = threadIdx.x & 63;
  double v[K], spc[K];
  int row4col[K], path[K], pos[K];
  bool sc[K];
#pragma unroll
  for (int k = 0; k < K; ++k) {
    v[k] = 0.0;
    row4col[k] = -1;
    path[k] = -1;
  }
  for (int i = lane; i < n; i += 64) {
    u[i] = 0.0;
    col4row[i] = -1;
  }
  wave_sync();
  for (int cur = 0; cur < n; ++cur) {
#pragma unroll
    for (int k = 0; k < K; ++k) {
      const int j = lane + 64 * k;
      pos[k] = j < n ? n - 1 - j : -1;
      spc[k] = INFINITY;
      sc[k] = false;
    }
    double minVal = 0.0;
    int i = cur, nrem = n, sink;
    while (true) {
      const double ui = u[i];
      double lm = INFINITY;
#pragma unroll
      for (int k = 0; k < K; ++k) {
        if (pos[k] >= 0) {
          const double r = ((minVal + cost(i, k)) - ui) - v[k];
          if (r < spc[k]) {
            path[k] = i;
            spc[k] = r;
          }
          lm = spc[k] < lm ? spc[k] : lm;
        }
      }
      const double lowest = wave_min(lm);
      if (!(lowest < INFINITY)) return LSAP_INFEASIBLE;
      // tie rule: a free column beats any assigned one; among free ones the highest position wins, among assigned the lowest
      int key = -1;
#pragma unroll
      for (int k = 0; k < K; ++k) {
        if (pos[k] >= 0 && spc[k] == lowest) {
          const int j = lane + 64 * k;
          const int kk = row4col[k] < 0 ? ((1 << 20) | (pos[k] << 8) | j) : (((1023 - pos[k]) << 8) | j);
          key = kk > key ? kk : key;
        }
      }
      key = wave_max(key);
      if (key < 0) return LSAP_INFEASIBLE;        // unreachable with finite duals; keeps every index below in range
      const int j = key & 255;
      const int p = (key >> 20) ? ((key >> 8) & 1023) : 1023 - ((key >> 8) & 1023);
      minVal = lowest;
      --nrem;
      int r4c = -1;
#pragma unroll
      for (int k = 0; k < K; ++k) {
        if (pos[k] == nrem) pos[k] = p;      // swap-remove: the last remaining column takes the freed position
        if (lane + 64 * k == j) {
          sc[k] = true;
          pos[k] = -1;
        }
        if (k == (j >> 6)) r4c = row4col[k];
      }
      r4c = __shfl(r4c, j & 63);
      if (r4c < 0) {
        sink = j;
        break;
      }
      i = r4c;
    }
    // duals (every visited row other than cur was reached through the column it holds: distinct LDS slots)
    if (lane == 0) u[cur] = u[cur] + minVal;
#pragma unroll
    for (int k = 0; k < K; ++k) {
      if (sc[k]) {
        if (row4col[k] >= 0) u[row4col[k]] = u[row4col[k]] + (minVal - spc[k]);
        v[k] = v[k] - (minVal - spc[k]);
      }
    }
    wave_sync();
    // augment along the path back to cur
    int j = sink;
    for (int step = 0; step < n; ++step) {     // a path visits each row at most once
      int pth = -1;
#pragma unroll
      for (int k = 0; k < K; ++k)
        if (k == (j >> 6)) pth = path[k];
      const int pi = __shfl(pth, j & 63);
      if (pi < 0) return LSAP_INFEASIBLE;
#pragma unroll
      for (int k = 0; k < K; ++k)
        if (lane + 64 * k == j) row4col[k] = pi;
      const int old = col4row[pi];
      wave_sync();
      col4row[pi] = j;           // every lane writes the same value
      wave_sync();
      j = old;
      if (pi == cur) break;
    }
  }
  return 0;
}

// ---- standalone batched solver: cost[B][n][n] -> col4row[B][n] -----------------------------------------------------------
struct GlobalCost {
  const double* c;
  int n, lane;
  __device__ double operator()(int i, int k) const { return c[(size_t)i * n + lane + 64 * k]; }
};

constexpr int LSA_WAVES = 4;

template <int K>
__global__ __launch_bounds__(64 * LSA_WAVES) void lsap_batched_kernel(const double* __restrict__ cost, int B, int n,
                                                                      int* __restrict__ col4row, int* __restrict__ status) {
  __shared__ double u_s[LSA_WAVES][NMAX];
  __shared__ int c_s[LSA_WAVES][NMAX];
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const long b = (long)blockIdx.x * LSA_WAVES + w;
  if (b >= B) return;                  // whole waves leave; nothing below waits on the workgroup
  const double* C = cost + (size_t)b * n * n;
  bool bad = false;
  for (int e = lane; e < n * n; e += 64) bad |= bad_cost(C[e]);
  int st = __ballot(bad) ? 1 : 0;
  if (!st) {
    const GlobalCost cf{C, n, lane};
    if (lsap_wave<K>(cf, n, u_s[w], c_s[w]) != 0) st = 1 << 8;
  }
  wave_sync();
  for (int i = lane; i < n; i += 64) col4row[(size_t)b * n + i] = st ? -1 : c_s[w][i];
  if (lane == 0) status[b] = st;
}

// ---- fused scores: one workgroup of 8 waves per jet --------------------------------------------------------------------------
// Staged frames, per side (0 = recons: assignment rows, 1 = target: columns), component-major F[side][20][N]:
//   0..3 Cartesian, 4..7 polar (E, pT, eta, phi), 8..11 normalized Cartesian, 12..15 normalized polar,
//   16..18 relative polar (pT / jet pT, eta - jet eta, wrapped phi - jet phi), 19 zero (so every frame has 4 components).
// Score variants f = 0..4 are those frames (offset 4 f), f = 5 the Lorentz scores on the Cartesian frame.
constexpr int SC_WAVES = 8;
constexpr int NCOMP = 20;

__host__ __device__ constexpr int hung_bit(int f) { return f < 5 ? 5 + f : 18; }
__host__ __device__ constexpr int cham_bit(int f) { return f < 5 ? f : 17; }
__host__ __device__ constexpr int mse_bit(int f) { return f < 5 ? 10 + f : 19; }

__device__ __forceinline__ double sq4(double a, double b, double c, double d) { return ((a * a + b * b) + c * c) + d * d; }
__device__ __forceinline__ double mink4(double a, double b, double c, double d) { return ((a * a - b * b) - c * c) - d * d; }

// the reference's torch.remainder(x + pi, 2 pi) - pi (float remainder: the sign follows the divisor)
__device__ __forceinline__ double wrap_phi(double x) {
  const double b = 2.0 * M_PI;
  double m = fmod(x + M_PI, b);
  if (m != 0.0 && ((m < 0.0) != (b < 0.0))) m += b;
  return m - M_PI;
}
__device__ __forceinline__ void polar(double px, double py, double pz, double& pT, double& eta, double& phi) {
  pT = sqrt(px * px + py * py);
  eta = asinh(pz / (pT + EPS));
  phi = atan2(py + EPS, px + EPS);
}

template <int K>
struct StagedCost {            // C[i][j] = |p_i - q_j| (Euclidean) or the signed Minkowski square, p from LDS, q in registers
  const double* P;             // F[0] + 4 f N: component c of row i at P[c N + i]
  int N;
  bool lorentz;
  double q[K][4];
  __device__ double operator()(int i, int k) const {
    const double d0 = P[i] - q[k][0], d1 = P[N + i] - q[k][1], d2 = P[2 * N + i] - q[k][2], d3 = P[3 * N + i] - q[k][3];
    return lorentz ? mink4(d0, d1, d2, d3) : sqrt(sq4(d0, d1, d2, d3));
  }
};

template <int K>
__global__ __launch_bounds__(64 * SC_WAVES) void anomaly_scores_kernel(const double* __restrict__ rec, const double* __restrict__ tgt,
                                                                      const double* __restrict__ rec_n, const double* __restrict__ tgt_n,
                                                                      int N, int mask, double* __restrict__ scores,
                                                                      int* __restrict__ col4row_out, int* __restrict__ status, int B) {
  extern __shared__ __align__(16) double lds[];
  double* F = lds;                       // [2][20][N]
  double* cham = F + 2 * NCOMP * N;      // [6][2][N] row minima
  double* msr = cham + 12 * N;           // [6][N] per-row squared differences
  double* uu = msr + 6 * N;              // [6][N] row duals of the six solvers
  double* jet = uu + 6 * N;              // [2][4] jet 4-vectors
  int* c4r = reinterpret_cast<int*>(jet + 8);    // [6][N]
  __shared__ int st_s;
  const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63;
  const size_t b = blockIdx.x;
  const size_t base = b * (size_t)N * 4;

  // jet sums, rows in order 0 .. N-1
  if (tid < 8) {
    const double* x = (tid < 4 ? rec : tgt) + base + (tid & 3);
    double s = 0.0;
    for (int r = 0; r < N; ++r) s = s + x[4 * r];
    jet[tid] = s;
  }
  if (tid == 0) st_s = 0;
  __syncthreads();

  for (int t = tid; t < 2 * N; t += 64 * SC_WAVES) {
    const int side = t >= N, r = t - side * N;
    const double* x = (side ? tgt : rec) + base + 4 * r;
    const double* xn = (side ? tgt_n : rec_n) + base + 4 * r;
    double* f = F + side * NCOMP * N + r;
    const double E = x[0], px = x[1], py = x[2], pz = x[3];
    double pT, eta, phi;
    polar(px, py, pz, pT, eta, phi);
    f[0] = E, f[N] = px, f[2 * N] = py, f[3 * N] = pz;
    f[4 * N] = E, f[5 * N] = pT, f[6 * N] = eta, f[7 * N] = phi;
    const double En = xn[0], pxn = xn[1], pyn = xn[2], pzn = xn[3];
    double pTn, etan, phin;
    polar(pxn, pyn, pzn, pTn, etan, phin);
    f[8 * N] = En, f[9 * N] = pxn, f[10 * N] = pyn, f[11 * N] = pzn;
    f[12 * N] = En, f[13 * N] = pTn, f[14 * N] = etan, f[15 * N] = phin;
    const double* J = jet + 4 * side;
    double jpT, jeta, jphi;
    polar(J[1], J[2], J[3], jpT, jeta, jphi);
    f[16 * N] = pT / (jpT + EPS);
    f[17 * N] = eta - jeta;
    f[18 * N] = wrap_phi(phi - jphi);
    f[19 * N] = 0.0;
  }
  __syncthreads();

  // waves 0..5 solve the Hungarian variant of their index when asked; every other wave shares the O(N^2) work
  const bool solver = w < 6 && ((mask >> hung_bit(w)) & 1);
  if (solver) {
    const int off = 4 * w * (w < 5);    // Lorentz: Cartesian frame
    StagedCost<K> cf;
    cf.P = F + off * N;
    cf.N = N;
    cf.lorentz = w == 5;
#pragma unroll
    for (int k = 0; k < K; ++k) {
      const int j = lane + 64 * k;
#pragma unroll
      for (int c = 0; c < 4; ++c) cf.q[k][c] = j < N ? F[(NCOMP + off + c) * N + j] : 0.0;
    }
    bool bad = false;
    for (int i = 0; i < N; ++i) {
#pragma unroll
      for (int k = 0; k < K; ++k)
        if (lane + 64 * k < N) bad |= bad_cost(cf(i, k));
    }
    int st = __ballot(bad) ? (1 << w) : 0;
    int* c4 = c4r + w * N;
    if (!st && lsap_wave<K>(cf, N, uu + w * N, c4) != 0) st = 1 << (8 + w);
    wave_sync();
    double score = NAN;
    if (!st) {
      // the reference's pairing: p[col_ind[r]] against q[r] (Euclidean, on the variant's frame; Lorentz: Cartesian)
      const int fo = 4 * w * (w < 5);
      double part = 0.0;
      for (int r = lane; r < N; r += 64) {
        const int s = c4[r];
        const double* p = F + fo * N;
        const double* q = F + (NCOMP + fo) * N;
        part = part + sq4(p[s] - q[r], p[N + s] - q[N + r], p[2 * N + s] - q[2 * N + r], p[3 * N + s] - q[3 * N + r]);
      }
      score = wave_sum(part) / N;
    }
    if (lane == 0) {
      scores[b * NSC + (w < 5 ? 5 + w : 18)] = score;
      if (st) atomicOr(&st_s, st);
    }
    if (col4row_out)
      for (int r = lane; r < N; r += 64) col4row_out[((size_t)w * B + b) * N + r] = st ? -1 : c4[r];
  } else {
    if (w < 6 && col4row_out)
      for (int r = lane; r < N; r += 64) col4row_out[((size_t)w * B + b) * N + r] = -1;
    int h = 0, nh = 0;
    for (int x = 0; x < SC_WAVES; ++x) {
      const bool hx = !(x < 6 && ((mask >> hung_bit(x)) & 1));
      h += hx && x < w;
      nh += hx;
    }
    const int n_cham = 12 * N, n_all = 18 * N;
    for (int t = h * 64 + lane; t < n_all; t += nh * 64) {
      if (t < n_cham) {          // Chamfer row minimum: (variant f, direction d, row k)
        const int fd = t / N, k = t - fd * N, f = fd >> 1, d = fd & 1;
        if (!((mask >> cham_bit(f)) & 1)) continue;
        const int off = 4 * f * (f < 5);
        const double* P = F + off * N;
        const double* Q = F + (NCOMP + off) * N;
        double m = 0.0;
        for (int jj = 0; jj < N; ++jj) {
          const int i = d ? jj : k, j = d ? k : jj;     // dist[i][j] = |p_i - q_j|; d = 0: min over j, d = 1: min over i
          const double d0 = P[i] - Q[j], d1 = P[N + i] - Q[N + j], d2 = P[2 * N + i] - Q[2 * N + j], d3 = P[3 * N + i] - Q[3 * N + j];
          const double c = f == 5 ? mink4(d0, d1, d2, d3) : sqrt(sq4(d0, d1, d2, d3));
          m = (jj == 0 || c < m || c != c) ? c : m;     // torch.min propagates NaN
          if (m != m) break;
        }
        cham[fd * N + k] = m;
      } else {                   // MSE row term (variant f, row r)
        const int u = t - n_cham, f = u / N, r = u - f * N;
        if (!((mask >> mse_bit(f)) & 1)) continue;
        const int off = 4 * f * (f < 5);
        const double* P = F + off * N;
        const double* Q = F + (NCOMP + off) * N;
        const double d0 = P[r] - Q[r], d1 = P[N + r] - Q[N + r], d2 = P[2 * N + r] - Q[2 * N + r], d3 = P[3 * N + r] - Q[3 * N + r];
        msr[f * N + r] = f == 5 ? mink4(d0, d1, d2, d3) : sq4(d0, d1, d2, d3);
      }
    }
  }
  __syncthreads();

  // the remaining 15 scores, each summed in row order by one thread
  if (tid < NSC) {
    const int s = tid;
    const bool hung = (s >= 5 && s < 10) || s == 18;
    if (!hung) {
      double val = NAN;
      if ((mask >> s) & 1) {
        if (s < 5 || s == 17) {
          const int f = s < 5 ? s : 5;
          double acc = 0.0;
          for (int k = 0; k < N; ++k) acc = acc + (cham[2 * f * N + k] + cham[(2 * f + 1) * N + k]);
          val = acc / N;
        } else if ((s >= 10 && s < 15) || s == 19) {
          const int f = s < 15 ? s - 10 : 5;
          double acc = 0.0;
          for (int k = 0; k < N; ++k) acc = acc + msr[f * N + k];
          val = acc / N;
        } else {                 // 15, 16: jet Cartesian (the reference scores "jet, polar" on the Cartesian jets too); 20: Lorentz
          const double d0 = jet[0] - jet[4], d1 = jet[1] - jet[5], d2 = jet[2] - jet[6], d3 = jet[3] - jet[7];
          val = s == 20 ? mink4(d0, d1, d2, d3) : sq4(d0, d1, d2, d3);
        }
      }
      scores[b * NSC + s] = val;
    } else if (!((mask >> s) & 1)) {
      scores[b * NSC + s] = NAN;
    }
    if (s == 0) status[b] = st_s;
  }
}

inline size_t scores_lds_bytes(int N) { return (size_t)(40 + 12 + 6 + 6) * N * 8 + 64 + (size_t)6 * N * 4; }

template <int K>
int launch_scores(const double* rec, const double* tgt, const double* rec_n, const double* tgt_n, int B, int N, int mask, double* scores,
                  int* col4row, int* status, hipStream_t st) {
  const size_t smem = scores_lds_bytes(N);
  if (smem > 64 * 1024)
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(anomaly_scores_kernel<K>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem);
  anomaly_scores_kernel<K><<<B, 64 * SC_WAVES, smem, st>>>(rec, tgt, rec_n, tgt_n, N, mask, scores, col4row, status, B);
  LGN_CHECK_LAUNCH();
  return 0;
}

template <int K>
int launch_lsap(const double* cost, int B, int n, int* col4row, int* status, hipStream_t st) {
  lsap_batched_kernel<K><<<(B + LSA_WAVES - 1) / LSA_WAVES, 64 * LSA_WAVES, 0, st>>>(cost, B, n, col4row, status);
  LGN_CHECK_LAUNCH();
  return 0;
}

static_assert(NMAX <= 192 && NMAX <= 255, "three columns per lane and 8-bit column indices in the tie key");

}  // namespace

int anomaly_scores(const double* rec, const double* tgt, const double* rec_n, const double* tgt_n, int B, int N, int mask, double* scores,
                   int* col4row, int* status, hipStream_t st) {
  if (N <= 64) return launch_scores<1>(rec, tgt, rec_n, tgt_n, B, N, mask, scores, col4row, status, st);
  if (N <= 128) return launch_scores<2>(rec, tgt, rec_n, tgt_n, B, N, mask, scores, col4row, status, st);
  return launch_scores<3>(rec, tgt, rec_n, tgt_n, B, N, mask, scores, col4row, status, st);
}

int linear_sum_assignment(const double* cost, int B, int n, int* col4row, int* status, hipStream_t st) {
  if (n <= 64) return launch_lsap<1>(cost, B, n, col4row, status, st);
  if (n <= 128) return launch_lsap<2>(cost, B, n, col4row, status, st);
  return launch_lsap<3>(cost, B, n, col4row, status, st);
}

}  // namespace lgn
