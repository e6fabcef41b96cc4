// lgn-autoencoder_amd/csrc/lsap_wave.hpp -- the exact linear-sum-assignment solver of one wavefront and its cost functors, shared by
// the anomaly scores (anomaly.hip) and the Hungarian-MSE training loss (assign_loss.hip).
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
// Floating-point contraction is OFF from here on (pragma below; a translation unit includes this header after the ones whose code
// may contract): an FMA in the reduced cost changes which column wins an exact tie, and the frames / distances must round as the
// host computes them.
#pragma once
#pragma clang fp contract(off)

#include <math.h>

#include "common.hpp"

namespace lgn {

constexpr int LSAP_NMAX = 192;         // three columns per lane (LGN_ANOMALY_NMAX of include/lgn_amd.h)
constexpr int LSAP_INFEASIBLE = 2;

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

static_assert(LSAP_NMAX <= 192 && LSAP_NMAX <= 255, "three columns per lane and 8-bit column indices in the tie key");

__device__ __forceinline__ double sq4(double a, double b, double c, double d) { return ((a * a + b * b) + c * c) + d * d; }
__device__ __forceinline__ double mink4(double a, double b, double c, double d) { return ((a * a - b * b) - c * c) - d * d; }

template <int K>
struct StagedCost {            // C[i][j] = |p_i - q_j| (Euclidean) or the signed Minkowski square, p from LDS, q in registers
  const double* P;             // component-major frame of the rows: component c of row i at P[c N + i]
  int N;
  bool lorentz;
  double q[K][4];
  __device__ double operator()(int i, int k) const {
    const double d0 = P[i] - q[k][0], d1 = P[N + i] - q[k][1], d2 = P[2 * N + i] - q[k][2], d3 = P[3 * N + i] - q[k][3];
    return lorentz ? mink4(d0, d1, d2, d3) : sqrt(sq4(d0, d1, d2, d3));
  }
};

}  // namespace lgn
