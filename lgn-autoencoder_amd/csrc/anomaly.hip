// lgn-autoencoder_amd/csrc/anomaly.hip -- per-jet anomaly scores (the reference's anomaly_scores(),
// utils/jet_analysis/anomaly_detection.py) and a batched exact linear-sum-assignment solver.
//
// The solver itself (lsap_wave, one wavefront per problem) and its cost functors live in lsap_wave.hpp, shared with the Hungarian-MSE
// training loss (assign_loss.hip).
//
// Floating-point contraction is OFF for this file (pragma below): an FMA in the reduced cost changes which column wins an exact
// tie, and the frames / distances must round as the host computes them.
#pragma clang fp contract(off)

#include <math.h>

#include "lds.hpp"
#include "../../include/lgn_amd.h"
#include "lsap_wave.hpp"
#include "polar_dev.hpp"     // p4_polar, wrap_phi: shared with emd.hip

namespace lgn {
namespace {

constexpr int NMAX = LGN_ANOMALY_NMAX;
constexpr int NSC = LGN_ANOMALY_NSCORES;
constexpr double EPS = POLAR_EPS;      // EPS_DEFAULT of the reference

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
    p4_polar(px, py, pz, pT, eta, phi);
    f[0] = E, f[N] = px, f[2 * N] = py, f[3 * N] = pz;
    f[4 * N] = E, f[5 * N] = pT, f[6 * N] = eta, f[7 * N] = phi;
    const double En = xn[0], pxn = xn[1], pyn = xn[2], pzn = xn[3];
    double pTn, etan, phin;
    p4_polar(pxn, pyn, pzn, pTn, etan, phin);
    f[8 * N] = En, f[9 * N] = pxn, f[10 * N] = pyn, f[11 * N] = pzn;
    f[12 * N] = En, f[13 * N] = pTn, f[14 * N] = etan, f[15 * N] = phin;
    const double* J = jet + 4 * side;
    double jpT, jeta, jphi;
    p4_polar(J[1], J[2], J[3], jpT, jeta, jphi);
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
  return lds_launch(anomaly_scores_kernel<K>, "anomaly_scores", dim3(B), dim3(64 * SC_WAVES), smem, st, rec, tgt, rec_n, tgt_n, N, mask, scores, col4row,
                    status, B);
}

template <int K>
int launch_lsap(const double* cost, int B, int n, int* col4row, int* status, hipStream_t st) {
  lsap_batched_kernel<K><<<(B + LSA_WAVES - 1) / LSA_WAVES, 64 * LSA_WAVES, 0, st>>>(cost, B, n, col4row, status);
  LGN_CHECK_LAUNCH();
  return 0;
}

static_assert(NMAX <= LSAP_NMAX, "lsap_wave holds three columns per lane");

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
