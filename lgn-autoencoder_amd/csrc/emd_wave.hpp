// lgn-autoencoder_amd/csrc/emd_wave.hpp -- the exact transportation solver of one wavefront: the weighted generalisation of lsap_wave
// (lsap_wave.hpp), used by the EMD score (emd.hip).
//
// emd_wave: one wavefront solves one balanced transportation problem, min sum f_ij c_ij with row sums = supplies, column sums =
// demands, f >= 0, by successive shortest paths on the residual graph with node potentials (u rows, v columns; every reduced cost
// c_ij - u_i - v_j stays >= 0 and is 0 on an arc that carries flow):
//   - sources are the rows in order 0 .. rows-1; a source is repeated until its supply is exactly 0;
//   - lanes own columns j = lane + 64 k (k < K): v, the shortest-path cost (spc), the predecessor row (path), the visited flag and the
//     remaining demand live in VGPRs.  The row state (u, remaining supply, distance, predecessor column, visited flag) lives in LDS;
//   - a Dijkstra step is one wave-wide fp64 min, then a wave-wide max of a key: a column with remaining demand (a sink) first, else
//     the lowest column index;
//   - backward arcs: a column may hold flow from several rows.  When a column without remaining demand is finalised at distance d,
//     every unvisited row with flow into it is reached at d as well (flow arcs are tight) and relaxes all columns: a wave-uniform loop
//     over the __ballot of that column's flows.  A row is scanned at most once per Dijkstra run;
//   - an augmentation pushes delta = min(remaining supply, remaining demand, the flows on the path's backward arcs), found by one walk
//     and applied by a second.  delta IS one of those values, so what it came from becomes exactly 0 (x - x), and every other value
//     stays > 0: each augmentation empties a supply, a demand or an arc.
// Columns without any demand (zero-weight particles) can neither end a path nor carry flow; they take no part in the search, and
// their potential is set at the end (finish_duals) so that the certificate covers them.
//
// Every loop is bounded: a Dijkstra run makes at most `cols` selections and scans each row at most once, a path walk takes at most
// rows + cols steps, and the augmentations of one problem are capped by the caller (EMD_ITER when the cap is hit).  A Dijkstra run
// that finds no column with remaining demand ends its source: the two weight sums agree to rounding only.  A supply left over of at
// most `leftover_tol` is dropped, a larger one is EMD_INFEASIBLE.
//
// The cost is a functor computed from staged rows (no cost matrix is stored); the flow sits behind an accessor, column-major, in
// LDS (FlowLds) or in a global workspace (FlowGlobal).  All control flow is wave-uniform.  Contraction is OFF (lsap_wave.hpp).
#pragma once
#pragma clang fp contract(off)

#include "lsap_wave.hpp"

namespace lgn {

constexpr int EMD_NMAX = 191;          // particles per event: with the fictitious node 192 rows / columns, three columns per lane
constexpr int EMD_ITER = 4;            // LGN_EMD_ITER of include/lgn_amd.h
constexpr int EMD_INFEASIBLE = 8;      // LGN_EMD_INFEASIBLE

struct EmdRows {                       // the row state of one problem (LDS), [rows] each
  double *u, *sup, *dist;
  int *pred, *vis;
};

// flow accessors: f_ij of row i into column j at [j ld + i], so that one column's flows are contiguous (the backward-arc ballot)
struct FlowLds {
  double* f;                           // LDS
  int ld;
  __device__ __forceinline__ double get(int i, int j) const { return f[j * ld + i]; }
  __device__ __forceinline__ void set(int i, int j, double x) const { f[j * ld + i] = x; }
};
struct FlowGlobal {
  double* f;                           // this wave's slice of the caller's workspace
  int ld;
  __device__ __forceinline__ double get(int i, int j) const { return f[(size_t)j * ld + i]; }
  __device__ __forceinline__ void set(int i, int j, double x) const { f[(size_t)j * ld + i] = x; }
};

template <int K, class T>
__device__ __forceinline__ T lane_slot(const T (&x)[K], int j) {       // x of column j, from the lane that owns it
  T r = x[0];
#pragma unroll
  for (int k = 1; k < K; ++k)
    if (k == (j >> 6)) r = x[k];
  return __shfl(r, j & 63);
}

// Solves the rows x cols problem with cost(i, k) = c[i][lane + 64 k].  In: rs.sup[0..rows) the supplies (LDS), dem[k] the demands of
// this lane's columns (0 beyond cols).  Out: the flow in F, rs.u and v the potentials, dem / rs.sup what could not be shipped (rounding),
// n_aug the number of augmentations.  Returns 0, EMD_ITER or EMD_INFEASIBLE.  1 <= rows, cols <= 64 K.
template <int K, class Cost, class Flow>
__device__ int emd_wave(const Cost& cost, const int rows, const int cols, const EmdRows& rs, double (&dem)[K], double (&v)[K], const Flow& F,
                        const int max_aug, const double leftover_tol, int& n_aug) {
  const int lane = threadIdx.x & 63;
  double spc[K];
  int path[K];
  bool live[K], vis[K];
#pragma unroll
  for (int k = 0; k < K; ++k) {
    v[k] = 0.0;
    path[k] = -1;
    live[k] = lane + 64 * k < cols && dem[k] > 0.0;
  }
  for (int i = lane; i < rows; i += 64) rs.u[i] = 0.0;
  for (int j = 0; j < cols; ++j)
    for (int i = lane; i < rows; i += 64) F.set(i, j, 0.0);
  wave_sync();
  n_aug = 0;

  for (int s = 0; s < rows; ++s) {
    while (true) {
      const double sup = rs.sup[s];
      if (!(sup > 0.0)) break;
      if (n_aug >= max_aug) return EMD_ITER;

      // ---- shortest paths from row s until a column with remaining demand is finalised
#pragma unroll
      for (int k = 0; k < K; ++k) {
        spc[k] = INFINITY;
        vis[k] = false;
        path[k] = -1;
      }
      for (int i = lane; i < rows; i += 64) {
        rs.vis[i] = i == s;
        rs.pred[i] = -1;
        rs.dist[i] = 0.0;
      }
      wave_sync();
      auto scan = [&](const int i, const double di) {       // row i, reached at distance di, relaxes every open column
        const double ui = rs.u[i];
#pragma unroll
        for (int k = 0; k < K; ++k) {
          if (live[k] && !vis[k]) {
            const double r = ((di + cost(i, k)) - ui) - v[k];
            if (r < spc[k]) {
              spc[k] = r;
              path[k] = i;
            }
          }
        }
      };
      scan(s, 0.0);
      double D = 0.0;
      int sink = -1;
      for (int sel = 0; sel < cols; ++sel) {
        double lm = INFINITY;
#pragma unroll
        for (int k = 0; k < K; ++k)
          if (live[k] && !vis[k]) lm = spc[k] < lm ? spc[k] : lm;
        const double lowest = wave_min(lm);
        if (!(lowest < INFINITY)) break;                      // no open column is left
        int key = -1;
#pragma unroll
        for (int k = 0; k < K; ++k) {
          if (live[k] && !vis[k] && spc[k] == lowest) {
            const int kk = (dem[k] > 0.0 ? 256 : 0) | (255 - (lane + 64 * k));
            key = kk > key ? kk : key;
          }
        }
        key = wave_max(key);
        if (key < 0) break;                                   // unreachable; keeps every index below in range
        const int j = 255 - (key & 255);
        D = lowest;
#pragma unroll
        for (int k = 0; k < K; ++k)
          if (lane + 64 * k == j) vis[k] = true;
        if (key & 256) {
          sink = j;
          break;
        }
        for (int t = 0; t < rows; t += 64) {                  // backward arcs: the unvisited rows with flow into column j
          const int i = t + lane;
          const bool reach = i < rows && rs.vis[i] == 0 && F.get(i, j) > 0.0;
          unsigned long long todo = __ballot(reach);
          if (!todo) continue;
          if (reach) {
            rs.vis[i] = 1;
            rs.pred[i] = j;
            rs.dist[i] = D;
          }
          wave_sync();
          while (todo) {
            const int b = __ffsll((long long)todo) - 1;
            todo &= todo - 1;
            scan(t + b, D);
          }
        }
      }
      // leftover_tol bounds the rounding of the two weight sums only, not that of the sup - delta / dem - delta steps on the way
      // here; those are exact whenever delta is the value subtracted from, and otherwise round by half an ulp of a remaining weight
      if (sink < 0) {                                         // the sums agree to rounding only: nothing can take what is left
        if (sup > leftover_tol) return EMD_INFEASIBLE;
        break;                                                // dropped (rs.sup[s] keeps it for the caller to see)
      }

      // ---- potentials of the visited nodes
      for (int i = lane; i < rows; i += 64)
        if (rs.vis[i]) rs.u[i] = rs.u[i] + (D - rs.dist[i]);
#pragma unroll
      for (int k = 0; k < K; ++k)
        if (vis[k]) v[k] = v[k] - (D - spc[k]);

      // ---- augment: the bottleneck along the path back to s, then the update
      const double dsink = lane_slot<K>(dem, sink);
      double delta = sup < dsink ? sup : dsink;
      const int max_steps = rows + cols;
      bool closed = false;
      int j = sink;
      for (int step = 0; step < max_steps; ++step) {
        const int i = lane_slot<K>(path, j);
        if (i < 0 || i >= rows) return EMD_INFEASIBLE;        // unreachable; keeps every index in range
        const int pj = rs.pred[i];
        if (pj < 0) {
          closed = i == s;
          break;
        }
        const double f = F.get(i, pj);
        delta = f < delta ? f : delta;
        j = pj;
      }
      if (!closed || !(delta > 0.0)) return EMD_INFEASIBLE;   // unreachable: every candidate is > 0
      j = sink;
      for (int step = 0; step < max_steps; ++step) {
        const int i = lane_slot<K>(path, j);
        const int pj = rs.pred[i];
        if (lane == 0) {
          F.set(i, j, F.get(i, j) + delta);
          if (pj >= 0) F.set(i, pj, F.get(i, pj) - delta);
        }
        if (pj < 0) break;
        j = pj;
      }
      if (lane == 0) rs.sup[s] = sup - delta;
#pragma unroll
      for (int k = 0; k < K; ++k)
        if (lane + 64 * k == sink) dem[k] = dem[k] - delta;
      ++n_aug;
      wave_sync();
    }
  }
  return 0;
}

// The potential of a column that had no demand (it took no part above): the largest feasible one, min_i (c_ij - u_i).  `had_demand`
// is the caller's record of dem > 0 before emd_wave.
template <int K, class Cost>
__device__ void finish_duals(const Cost& cost, const int rows, const int cols, const EmdRows& rs, const bool (&had_demand)[K], double (&v)[K]) {
  const int lane = threadIdx.x & 63;
  for (int i = 0; i < rows; ++i) {
    const double ui = rs.u[i];
#pragma unroll
    for (int k = 0; k < K; ++k) {
      if (lane + 64 * k < cols && !had_demand[k]) {
        const double r = cost(i, k) - ui;
        v[k] = (i == 0 || r < v[k]) ? r : v[k];
      }
    }
  }
}

static_assert(EMD_NMAX + 1 <= 192 && EMD_NMAX + 1 <= 255, "three columns per lane and 8-bit column indices in the selection key");

}  // namespace lgn
