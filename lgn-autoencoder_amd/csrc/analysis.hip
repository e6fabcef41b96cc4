// lgn-autoencoder_amd/csrc/analysis.hip -- the numeric half of the reference's plot_p (utils/jet_analysis/utils.py,
// particle_recon_err.py, jet_recon_err.py): per jet the particle features in polar and relative-polar coordinates, the jet features,
// the matched relative errors of get_rel_err_find_match (two exact assignments per jet) and the jet relative errors; and a batched
// histogram over explicit edges with numpy's semantics.
//
// recon_analysis_kernel: one wavefront per jet.  The jet's rows are staged in LDS once, per side (0 = target: assignment rows,
// 1 = recons: columns) component-major F[side][10][N]: 0 E, 1..3 (px, py, pz), 4..6 polar (pt, eta, phi), 7..9 relative polar.  Both
// assignments (lsap_wave of lsap_wave.hpp, cost = exact Euclidean distance computed from the staged rows) and every feature read them
// from there.  LDS of a workgroup of 4 waves: 4 ((21 N + 8) 8 + 8 N) bytes = 135,424 at N = LGN_ANOMALY_NMAX = 192, under the
// 160 KiB of a CU: every admitted N fits, so there is no plan-time query.
//
// Floating-point contraction is OFF for this file (pragma below and in lsap_wave.hpp, -ffp-contract=off in the Makefile): the
// frames, costs and relative errors round one operation at a time, as the host computes them, and an FMA in a cost changes which
// column wins an exact tie.
#pragma clang fp contract(off)

#include <math.h>

#include <type_traits>

#include "lds.hpp"
#include "../../include/lgn_amd.h"
#include "lsap_wave.hpp"
#include "polar_dev.hpp"     // p_polar_tensor, wrap_phi

namespace lgn {
namespace {

constexpr int NMAX = LGN_ANOMALY_NMAX;
constexpr double EPS = 1e-16;          // EPS of particle_recon_err.py and the eps defaults of utils.py / jet_recon_err.py
constexpr int RA_WAVES = 4;
constexpr int NFR = 10;                // staged rows per side

__host__ __device__ constexpr size_t ra_wave_doubles(int N) { return (size_t)(2 * NFR + 1) * N + 8; }   // frames, row duals, jet sums
inline size_t ra_lds_bytes(int N) { return RA_WAVES * (ra_wave_doubles(N) * sizeof(double) + (size_t)2 * N * sizeof(int)); }

__device__ __forceinline__ bool is_inf(double x) { return fabs(x) == INFINITY; }

template <int K>
struct Cost3 {                 // C[i][j] = |t_i - r_j| on three components: rows from LDS, the lane's columns in registers
  const double* P;
  int N;
  double q[K][3];
  __device__ double operator()(int i, int k) const {
    const double d0 = P[i] - q[k][0], d1 = P[N + i] - q[k][1], d2 = P[2 * N + i] - q[k][2];
    return sqrt((d0 * d0 + d1 * d1) + d2 * d2);
  }
};

// Does some cost |t_i - r_j| come out NaN?  (It is never -inf.)  A difference is NaN when either side is, or when both are the
// same infinity; squares and their sum then stay non-NaN, overflow included.  Every row meets every column, so per component it is
// enough to know which special values each side holds.  Wave uniform.
__device__ bool frame_is_bad(const double* T, const double* R, int N, int lane) {
  int f = 0;
  for (int r = lane; r < N; r += 64) {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const double t = T[c * N + r], x = R[c * N + r];
      if (t != t || x != x) f |= 1;
      if (t == INFINITY) f |= 2 << (4 * c);
      if (t == -INFINITY) f |= 4 << (4 * c);
      if (x == INFINITY) f |= 8 << (4 * c);
      if (x == -INFINITY) f |= 16 << (4 * c);
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) f |= __shfl_xor(f, o);
  bool bad = f & 1;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const int g = f >> (4 * c);
    bad |= ((g & 2) && (g & 8)) || ((g & 4) && (g & 16));
  }
  return bad;
}

struct RaArgs {
  const double *target, *recons;
  int B, N, abs_coord, find_match;
  double *part_polar, *part_polarrel, *jet_cart, *jet_polar, *jet_rel_err;
  uint8_t* jet_keep;
  double* rel_err;
  int* col4row;
  uint8_t* is_padded;
  int* status;
};

// The matched (or identity-paired) relative errors of one jet from its staged frames: rows 1..3, 4..6 and relrow..relrow+2 of both
// sides.  The wave has synchronised after staging.
template <int K>
__device__ void residuals(const RaArgs& a, const double* F, double* u, int* c4r, const int N, const size_t B, const size_t b,
                          const int lane, const int relrow) {

  const int rows[3] = {1, 4, relrow};
  if (!a.find_match) {         // get_rel_err: identity pairing, no eps in any frame
    for (int r = lane; r < N; r += 64) {
      bool pad = false;
#pragma unroll
      for (int f = 0; f < 3; ++f) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          const double t = F[(rows[f] + c) * N + r], x = F[(NFR + rows[f] + c) * N + r];
          const double e = (x - t) / t;
          a.rel_err[((f * B + b) * N + r) * 3 + c] = e;
          if (f == 0) pad |= is_inf(e);
        }
      }
      a.is_padded[b * N + r] = pad;
      if (a.col4row) a.col4row[b * N + r] = r, a.col4row[(B + b) * N + r] = r;
    }
    if (lane == 0) a.status[b] = 0;
    return;
  }

  int st = 0;
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    const int row0 = k ? relrow : 1;
    const double* T = F + row0 * N;
    const double* R = F + (NFR + row0) * N;
    if (frame_is_bad(T, R, N, lane)) {
      st |= 1;
    } else {
      Cost3<K> cf;
      cf.P = T;
      cf.N = N;
#pragma unroll
      for (int kk = 0; kk < K; ++kk) {
        const int j = lane + 64 * kk;
#pragma unroll
        for (int c = 0; c < 3; ++c) cf.q[kk][c] = j < N ? R[c * N + j] : 0.0;
      }
      if (lsap_wave<K>(cf, N, u, c4r + k * N) != 0) st |= 1 << 8;
    }
    wave_sync();
  }
  for (int r = lane; r < N; r += 64) {
    const int c0 = st ? 0 : c4r[r], c1 = st ? 0 : c4r[N + r];
    bool pad = false;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const double t0 = F[(1 + c) * N + r], t1 = F[(4 + c) * N + r], t2 = F[(relrow + c) * N + r];
      double e0 = (F[(NFR + 1 + c) * N + c0] - t0) / t0;               // no eps: padded rows give +-inf or NaN
      double e1 = (F[(NFR + 4 + c) * N + c0] - t1) / (t1 + EPS);       // the polar frame keeps the Cartesian matching
      double e2 = (F[(NFR + relrow + c) * N + c1] - t2) / (t2 + EPS);
      if (st) e0 = e1 = e2 = NAN;
      a.rel_err[(b * N + r) * 3 + c] = e0;
      a.rel_err[((B + b) * N + r) * 3 + c] = e1;
      a.rel_err[((2 * B + b) * N + r) * 3 + c] = e2;
      pad |= is_inf(e0);
    }
    a.is_padded[b * N + r] = pad;
    if (a.col4row) a.col4row[b * N + r] = st ? -1 : c0, a.col4row[(B + b) * N + r] = st ? -1 : c1;
  }
  if (lane == 0) a.status[b] = st;
}

template <int K>
__global__ __launch_bounds__(64 * RA_WAVES) void recon_analysis_kernel(const RaArgs a) {
  extern __shared__ __align__(16) double lds[];
  const int N = a.N;
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const size_t B = a.B, b = (size_t)blockIdx.x * RA_WAVES + w;
  if (b >= B) return;                    // whole waves leave; nothing below waits on the workgroup
  double* F = lds + w * ra_wave_doubles(N);       // [2][NFR][N]
  double* u = F + 2 * NFR * N;                    // [N] row duals of the solver
  double* jet = u + N;                            // [2][4] summed 4-vectors
  int* c4r = reinterpret_cast<int*>(lds + RA_WAVES * ra_wave_doubles(N)) + (size_t)w * 2 * N;    // [2][N]

  for (int r = lane; r < N; r += 64) {
#pragma unroll
    for (int side = 0; side < 2; ++side) {
      const double* x = (side ? a.recons : a.target) + (b * N + r) * 4;
#pragma unroll
      for (int c = 0; c < 4; ++c) F[(side * NFR + c) * N + r] = x[c];
    }
  }
  wave_sync();
  if (lane < 8) {                        // jet sums, rows in order 0 .. N-1
    const double* x = F + ((lane >> 2) * NFR + (lane & 3)) * N;
    double s = 0.0;
    for (int r = 0; r < N; ++r) s = s + x[r];
    jet[lane] = s;
  }
  wave_sync();

  // particle frames
  const int relrow = a.abs_coord ? 7 : 4;        // without abs_coord the relative-polar frame IS the polar one
#pragma unroll
  for (int side = 0; side < 2; ++side) {
    double* f = F + side * NFR * N;
    double Pt, Eta, Phi;
    p_polar_tensor(jet[4 * side + 1], jet[4 * side + 2], jet[4 * side + 3], Pt, Eta, Phi);
    for (int r = lane; r < N; r += 64) {
      double pt, eta, phi;
      p_polar_tensor(f[N + r], f[2 * N + r], f[3 * N + r], pt, eta, phi);
      f[4 * N + r] = pt, f[5 * N + r] = eta, f[6 * N + r] = phi;
      const size_t o = ((side * B + b) * N + r) * 3;
      if (a.part_polar) a.part_polar[o] = pt, a.part_polar[o + 1] = eta, a.part_polar[o + 2] = phi;
      if (a.abs_coord) {
        const double q0 = pt / (Pt + EPS), q1 = Eta - eta, q2 = wrap_phi(Phi - phi);
        f[7 * N + r] = q0, f[8 * N + r] = q1, f[9 * N + r] = q2;
        if (a.part_polarrel) a.part_polarrel[o] = q0, a.part_polarrel[o + 1] = q1, a.part_polarrel[o + 2] = q2;
      }
    }
  }

  // jet features: lane 0 the target's, lane 1 the reconstruction's (the other lanes repeat them)
  {
    const int side = lane & 1;
    const double E = jet[4 * side], px = jet[4 * side + 1], py = jet[4 * side + 2], pz = jet[4 * side + 3];
    const double msq = ((E * E - px * px) - py * py) - pz * pz;
    const double m = sqrt(fabs(msq)) * (double)((msq > 0.0) - (msq < 0.0));
    const double pt = sqrt(px * px + py * py);
    const double fc[4] = {m, px, py, pz};
    const double fp[4] = {m, pt, asinh(pz / (pt + EPS)), atan2(py, px)};      // get_jet_feature_polar: no eps in phi
    double tc[4], tp[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) tc[c] = __shfl(fc[c], 0), tp[c] = __shfl(fp[c], 0);
    if (lane < 2) {
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        a.jet_cart[(side * B + b) * 4 + c] = fc[c];
        a.jet_polar[(side * B + b) * 4 + c] = fp[c];
      }
    }
    if (lane == 1) {           // the reference's call hands (recons, target) to a lambda written for (target, recons)
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        a.jet_rel_err[b * 4 + c] = (fc[c] - tc[c]) / (fc[c] + EPS);
        a.jet_rel_err[(B + b) * 4 + c] = (fp[c] - tp[c]) / (fp[c] + EPS);
      }
    }
    if (lane == 0) {           // filter_out_zeros
      a.jet_keep[b] = tc[0] != 0.0 && tc[1] != 0.0 && tc[2] != 0.0 && tc[3] != 0.0;
      a.jet_keep[B + b] = tp[0] != 0.0 && tp[1] != 0.0 && tp[2] != 0.0 && tp[3] != 0.0;
    }
  }
  if (!a.rel_err) return;
  wave_sync();
  residuals<K>(a, F, u, c4r, N, B, b, lane, relrow);
}

// get_rel_err_find_match on frames the caller computed: fr[0..5] = target / recons Cartesian, polar, relative polar, each [B][N][3]
template <int K>
__global__ __launch_bounds__(64 * RA_WAVES) void match_rel_err_kernel(const RaArgs a, const double* t3, const double* r3, const double* tp,
                                                                      const double* rp, const double* tq, const double* rq) {
  extern __shared__ __align__(16) double lds[];
  const int N = a.N;
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const size_t B = a.B, b = (size_t)blockIdx.x * RA_WAVES + w;
  if (b >= B) return;
  double* F = lds + w * ra_wave_doubles(N);
  double* u = F + 2 * NFR * N;
  int* c4r = reinterpret_cast<int*>(lds + RA_WAVES * ra_wave_doubles(N)) + (size_t)w * 2 * N;
  const double* src[2][3] = {{t3, tp, tq}, {r3, rp, rq}};
  for (int r = lane; r < N; r += 64) {
#pragma unroll
    for (int side = 0; side < 2; ++side) {
#pragma unroll
      for (int f = 0; f < 3; ++f) {
#pragma unroll
        for (int c = 0; c < 3; ++c) F[(side * NFR + 1 + 3 * f + c) * N + r] = src[side][f][(b * N + r) * 3 + c];
      }
    }
  }
  wave_sync();
  residuals<K>(a, F, u, c4r, N, B, b, lane, 7);
}

template <int K>
int launch_analysis(const RaArgs& a, hipStream_t st) {
  const size_t smem = ra_lds_bytes(a.N);
  return lds_launch(recon_analysis_kernel<K>, "recon_analysis", dim3((a.B + RA_WAVES - 1) / RA_WAVES), dim3(64 * RA_WAVES), smem, st, a);
}

template <int K>
int launch_match(const RaArgs& a, const double* const* fr, hipStream_t st) {
  const size_t smem = ra_lds_bytes(a.N);
  return lds_launch(match_rel_err_kernel<K>, "match_rel_err", dim3((a.B + RA_WAVES - 1) / RA_WAVES), dim3(64 * RA_WAVES), smem, st, a, fr[0], fr[1], fr[2],
                    fr[3], fr[4], fr[5]);
}

static_assert(NMAX <= LSAP_NMAX, "lsap_wave holds three columns per lane");

// ---- histogram over explicit edges ---------------------------------------------------------------------------------------------
constexpr int HIST_THREADS = 256;
struct HistCols {
  int n_edges[LGN_HIST_MAX_COLS];
};

__global__ void hist_clear_kernel(long long* counts, double* wcounts, size_t n) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    if (counts) counts[i] = 0;
    if (wcounts) wcounts[i] = 0.0;
  }
}

// Workgroup (x, c) counts column c of its rows into LDS, then adds every non-empty bin to the output with one global atomic.
// Membership compares with the edge values themselves (upper bound by bisection): bin i holds edges[i] <= v < edges[i + 1], the last
// bin also v == edges[-1]; NaN compares false with every edge and lands nowhere.
template <bool W>
__global__ __launch_bounds__(HIST_THREADS) void histogram_kernel(const double* __restrict__ x, long long rows, int ld,
                                                                 const double* __restrict__ edges, const HistCols nc, int max_edges,
                                                                 const uint8_t* __restrict__ keep, const double* __restrict__ weights,
                                                                 unsigned long long* __restrict__ counts, double* __restrict__ wcounts,
                                                                 int max_bins) {
  using cnt_t = typename std::conditional<W, double, unsigned int>::type;
  __shared__ double e_s[LGN_HIST_MAX_EDGES];
  __shared__ cnt_t c_s[LGN_HIST_MAX_EDGES - 1];
  const int c = blockIdx.y, tid = threadIdx.x;
  const int ne = nc.n_edges[c], nb = ne - 1;
  for (int i = tid; i < ne; i += HIST_THREADS) e_s[i] = edges[(size_t)c * max_edges + i];
  for (int i = tid; i < nb; i += HIST_THREADS) c_s[i] = 0;
  __syncthreads();
  const double last = e_s[nb];
  for (long long r = (long long)blockIdx.x * HIST_THREADS + tid; r < rows; r += (long long)gridDim.x * HIST_THREADS) {
    if (keep && !keep[r]) continue;
    const double v = x[(size_t)r * ld + c];
    int lo = 0, hi = ne;                 // edges[< lo] <= v, and not edges[>= hi] <= v
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (e_s[mid] <= v) lo = mid + 1;
      else hi = mid;
    }
    int bin = lo - 1;
    if (bin == nb) bin = v == last ? nb - 1 : -1;
    if (bin < 0) continue;
    if constexpr (W) atomicAdd(&c_s[bin], weights[r]);
    else atomicAdd(&c_s[bin], 1u);
  }
  __syncthreads();
  for (int i = tid; i < nb; i += HIST_THREADS) {
    const cnt_t n = c_s[i];
    if (n != 0) {
      if constexpr (W) atomicAdd(&wcounts[(size_t)c * max_bins + i], n);
      else atomicAdd(&counts[(size_t)c * max_bins + i], (unsigned long long)n);
    }
  }
}

}  // namespace

int recon_analysis(const double* target, const double* recons, int B, int N, int abs_coord, int find_match, double* part_polar,
                   double* part_polarrel, double* jet_cart, double* jet_polar, double* jet_rel_err, uint8_t* jet_keep, double* rel_err,
                   int* col4row, uint8_t* is_padded, int* status, hipStream_t st) {
  const RaArgs a{target, recons, B, N, abs_coord, find_match, part_polar, part_polarrel, jet_cart, jet_polar, jet_rel_err, jet_keep,
                 rel_err, col4row, is_padded, status};
  if (N <= 64) return launch_analysis<1>(a, st);
  if (N <= 128) return launch_analysis<2>(a, st);
  return launch_analysis<3>(a, st);
}

int match_rel_err(const double* const* frames, int B, int N, double* rel_err, int* col4row, uint8_t* is_padded, int* status,
                  hipStream_t st) {
  RaArgs a{};
  a.B = B, a.N = N, a.abs_coord = 1, a.find_match = 1;
  a.rel_err = rel_err, a.col4row = col4row, a.is_padded = is_padded, a.status = status;
  if (N <= 64) return launch_match<1>(a, frames, st);
  if (N <= 128) return launch_match<2>(a, frames, st);
  return launch_match<3>(a, frames, st);
}

int histogram(const double* x, long long rows, int ld, int cols, const double* edges, const int* n_edges, int max_edges,
              const uint8_t* keep, const double* weights, long long* counts, double* wcounts, int max_bins, hipStream_t st) {
  HistCols nc{};
  for (int c = 0; c < cols; ++c) nc.n_edges[c] = n_edges[c];
  const size_t n = (size_t)cols * max_bins;
  hist_clear_kernel<<<(unsigned)((n + 255) / 256), 256, 0, st>>>(counts, wcounts, n);
  LGN_CHECK_LAUNCH();
  if (rows == 0) return 0;
  // a workgroup's 32-bit LDS counters hold its share of the rows: at most rows / 2048 + 256 < 2^32 (rows <= 2^40, checked by the caller)
  long long gx = (rows + HIST_THREADS * 16 - 1) / (HIST_THREADS * 16);
  gx = gx < 1 ? 1 : gx > 2048 ? 2048 : gx;
  const dim3 grid((unsigned)gx, (unsigned)cols);
  if (weights)
    histogram_kernel<true><<<grid, HIST_THREADS, 0, st>>>(x, rows, ld, edges, nc, max_edges, keep, weights, nullptr, wcounts, max_bins);
  else
    histogram_kernel<false><<<grid, HIST_THREADS, 0, st>>>(x, rows, ld, edges, nc, max_edges, keep, nullptr,
                                                           reinterpret_cast<unsigned long long*>(counts), nullptr, max_bins);
  LGN_CHECK_LAUNCH();
  return 0;
}

}  // namespace lgn
