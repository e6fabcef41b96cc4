// lgn-autoencoder_amd/csrc/stats.hip -- the statistics half of the reference's plot_p: get_stats() and find_fwhm() of
// utils/jet_analysis/utils.py per column of a device matrix, the histogram edges linspace(median -+ alpha IQR) it draws over, and the
// jet images of utils/jet_analysis/jet_images.py.  Entry points: lgn_column_stats_workspace_bytes, lgn_column_stats_f64,
// lgn_hist_fwhm_f64, lgn_jet_images_workspace_bytes, lgn_jet_images_f64.  The header holds the specification.
//
// lgn_column_stats_f64, all on the caller's stream, nothing allocated, no host wait; the kept count n lives on the device, so every
// grid is sized by `rows` and a workgroup past n leaves at once:
//   1. compaction   the mask is one per row, so one count | scan | scatter serves every column; the scatter writes order-preserving
//                   64-bit keys of the kept doubles and the column's NONFINITE bit (an integer atomic).
//   2. sort         a bitonic sort of LGN_STATS_TILE keys in LDS, then ceil(log2(rows / tile)) merge passes between two buffers, a
//                   workgroup per output tile located by a merge-path search: sort_dev.hpp, shared with roc.hip, keys only.
//   3. selection    one thread per column: quantiles, median, min, max, abs_min by index; the MAD as a k-th-of-two-sorted-runs
//                   selection (left of the median the deviations fall, right of it they rise, rounding is monotone); the runs
//                   |a| < IQR and |a| < IDR by bisection; the edges.
//   4. moments      two passes over the SORTED column (sum, sum |a|, the two filtered sums | central m2, m3, m4), each a partial per
//                   tile -- thread-serial over consecutive values, a fixed shuffle tree, the four waves in order -- and a final sum
//                   of the ceil(n / tile) partials in a fixed order.  The order depends on the multiset of kept values alone: not on
//                   the grid, the row order, the mask or the number of columns.  No floating-point atomics.
// lgn_jet_images_f64: one wavefront per jet, image in LDS, part q of P = min(B, LGN_JET_IMAGE_PARTS) takes jets q, q + P, ..;
// the parts' sums are added in order by a second kernel.
// Contraction is off: linspace rounds i * step and + start separately, as numpy does, and the lerp of a quantile likewise.
#pragma clang fp contract(off)
#include <math.h>

#include "lds.hpp"
#include "../../include/lgn_amd.h"
#include "polar_dev.hpp"     // wrap_phi
#include "sort_dev.hpp"

namespace lgn {
namespace {

constexpr int ST = LGN_STATS_TILE;      // keys per sort tile, merge chunk and moment partial
constexpr int SB = 256;                 // threads per workgroup
constexpr int SI = ST / SB;             // consecutive items of a thread
constexpr int NSTAT = LGN_STATS_COUNT;
static_assert(ST == SB * SI && (ST & (ST - 1)) == 0, "the tile is a power of two and a multiple of the workgroup");
static_assert(LGN_STATS_MAX_COLS <= SB, "the init kernel clears one status word per thread");

struct StatsCtx {
  const double* x;
  const uint8_t* mask;
  long long rows;
  int ld, cols, mask_keep, nb, num_edges;
  double alpha;
  u64 *key_a, *key_b;      // [cols][rows]
  u64* sorted;             // whichever of the two holds the sorted columns
  int* blk;                // [nb] kept rows of a tile, then their exclusive scan
  long long* count;        // [1] n
  double* part;            // [cols][nb][4]
  long long* runs;         // [cols][4] the runs |a| < IQR and |a| < IDR: lo, hi, lo, hi
  double *stats, *edges;
  long long* kept;
  int* status;
};

__device__ __forceinline__ bool row_kept(const StatsCtx& c, long long r) {
  return !c.mask || (c.mask[r] != 0) == (c.mask_keep != 0);
}

// ---- 1. compaction -------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(SB) void stats_count(StatsCtx c) {
  const long long r0 = (long long)blockIdx.x * ST + threadIdx.x * SI;
  int s = 0;
#pragma unroll
  for (int e = 0; e < SI; ++e)
    if (r0 + e < c.rows) s += row_kept(c, r0 + e);
  int total;
  block_excl_scan<SB>(s, total);
  if (threadIdx.x == 0) c.blk[blockIdx.x] = total;
  if (blockIdx.x == 0 && threadIdx.x < c.cols) c.status[threadIdx.x] = 0;
}

__global__ __launch_bounds__(SB) void stats_scan(StatsCtx c) {
  long long carry = 0;
  for (int base = 0; base < c.nb; base += SB) {
    const int q = base + threadIdx.x;
    const int v = q < c.nb ? c.blk[q] : 0;
    int total;
    const int ex = block_excl_scan<SB>(v, total);
    if (q < c.nb) c.blk[q] = (int)(carry + ex);        // < rows < 2^31
    carry += total;
  }
  if (threadIdx.x == 0) *c.count = carry;
}

__global__ __launch_bounds__(SB) void stats_scatter(StatsCtx c) {
  __shared__ int s_bad;
  const int k = blockIdx.y;
  const long long r0 = (long long)blockIdx.x * ST + threadIdx.x * SI;
  if (threadIdx.x == 0) s_bad = 0;
  int f[SI], s = 0;
#pragma unroll
  for (int e = 0; e < SI; ++e) {
    f[e] = r0 + e < c.rows ? row_kept(c, r0 + e) : 0;
    s += f[e];
  }
  int total;
  long long o = (long long)k * c.rows + c.blk[blockIdx.x] + block_excl_scan<SB>(s, total);     // the scan's barriers order s_bad = 0
  int bad = 0;
#pragma unroll
  for (int e = 0; e < SI; ++e) {
    if (!f[e]) continue;
    const double v = c.x[(r0 + e) * c.ld + k];
    if (nonfinite_bits((u64)__double_as_longlong(v))) bad = 1;
    c.key_a[o++] = key_of(v);              // o - k rows < n <= rows
  }
  if (bad) atomicOr(&s_bad, LGN_STATS_NONFINITE);
  __syncthreads();
  if (threadIdx.x == 0 && s_bad) atomicOr(&c.status[k], s_bad);
}

// ---- 2. sort ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(SB) void stats_tile_sort(StatsCtx c) {
  __shared__ u64 sk[ST];
  const int tid = threadIdx.x;
  const long long M = *c.count, base = (long long)blockIdx.x * ST;
  if (base >= M) return;
  const int n = (int)(M - base < ST ? M - base : ST);
  const int p2 = bitonic_size(n);
  u64* col = c.key_a + (long long)blockIdx.y * c.rows + base;
  for (int j = tid; j < p2; j += SB) sk[j] = j < n ? col[j] : ~0ull;
  bitonic_sort_lds<SB>(sk, (NoPayload*)nullptr, p2);
  for (int j = tid; j < n; j += SB) col[j] = sk[j];
}

// runs of W sorted keys -> runs of 2 W; an unpaired run (and a whole column shorter than W) is copied
__global__ __launch_bounds__(SB) void stats_merge_pass(const u64* __restrict__ kin, u64* __restrict__ kout, long long rows,
                                                       const long long* __restrict__ count, long long W) {
  const long long M = *count;
  if ((long long)blockIdx.x * ST >= M) return;
  merge_chunk<ST, SB>(kin, (const NoPayload*)nullptr, kout, (NoPayload*)nullptr, (long long)blockIdx.y * rows, M, W);
}

// ---- 3. selection ----------------------------------------------------------------------------------------------------------------
// np.quantile(a, q), method "linear": numpy's _lerp of the two neighbours of the virtual index (n - 1) q
__device__ double quantile_linear(const u64* a, long long n, double q) {
  const double idx = (double)(n - 1) * q;
  const double fl = floor(idx);
  const long long lo = (long long)fl, hi = lo + 1 < n ? lo + 1 : n - 1;
  const double g = idx - fl, x = value_of(a[lo]), y = value_of(a[hi]), d = y - x;
  return g >= 0.5 ? y - d * (1.0 - g) : x + d * g;
}
// first index whose value is not below v (strict = false) or above v (strict = true)
__device__ long long lower_index(const u64* a, long long n, double v, bool strict) {
  long long lo = 0, hi = n;
  while (lo < hi) {
    const long long mid = lo + ((hi - lo) >> 1);
    const double x = value_of(a[mid]);
    if (strict ? x <= v : x < v) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}
// the k-th smallest (from 0) of |a_i - med|: L[j] = med - a[s - 1 - j] (j < s) and R[j] = a[s + j] - med (j < n - s) both rise
__device__ double kth_deviation(const u64* a, long long n, long long s, double med, long long k) {
  const long long nl = s, nr = n - s;
  long long lo = k > nr ? k - nr : 0, hi = k < nl ? k : nl;       // lo = how many of the k smallest come from L
  while (lo < hi) {
    const long long mid = lo + ((hi - lo) >> 1);
    const double l = fabs(value_of(a[s - 1 - mid]) - med), r = fabs(value_of(a[s + (k - 1 - mid)]) - med);
    if (l <= r) lo = mid + 1;
    else hi = mid;
  }
  const long long i = lo, j = k - lo;
  const double l = i < nl ? fabs(value_of(a[s - 1 - i]) - med) : INFINITY;
  const double r = j < nr ? fabs(value_of(a[s + j]) - med) : INFINITY;
  return l < r ? l : r;
}

__global__ __launch_bounds__(SB) void stats_select(StatsCtx c) {
  __shared__ double s_edge[2];
  const int k = blockIdx.x;
  const long long n = *c.count;
  const u64* a = c.sorted + (long long)k * c.rows;
  double* out = c.stats + (long long)k * NSTAT;
  if (threadIdx.x == 0) {
    int st = c.status[k];
    if (n == 0) st |= LGN_STATS_EMPTY;
    c.status[k] = st;
    c.kept[k] = n;
    long long* run = c.runs + k * 4;
    if (st) {
      for (int i = 0; i < NSTAT; ++i) out[i] = qnan();
      run[0] = run[1] = run[2] = run[3] = 0;
      s_edge[0] = s_edge[1] = qnan();
    } else {
      const double q10 = quantile_linear(a, n, 0.1), q25 = quantile_linear(a, n, 0.25), q75 = quantile_linear(a, n, 0.75),
                   q90 = quantile_linear(a, n, 0.9);
      const double med = (n & 1) ? value_of(a[n / 2]) : (value_of(a[n / 2 - 1]) + value_of(a[n / 2])) / 2.0;
      const double iqr = q75 - q25, idr = q90 - q10;
      const long long s = lower_index(a, n, med, false);
      const double mad = (n & 1) ? kth_deviation(a, n, s, med, n / 2)
                                 : (kth_deviation(a, n, s, med, n / 2 - 1) + kth_deviation(a, n, s, med, n / 2)) / 2.0;
      const long long z = lower_index(a, n, 0.0, false);       // a[z - 1] < 0 <= a[z]
      double amin = INFINITY;
      if (z < n) amin = fabs(value_of(a[z]));
      if (z > 0) amin = fmin(amin, fabs(value_of(a[z - 1])));
      out[LGN_STAT_MEDIAN] = med;
      out[LGN_STAT_IQR] = iqr;
      out[LGN_STAT_FIRST_QUARTILE] = q25;
      out[LGN_STAT_THIRD_QUARTILE] = q75;
      out[LGN_STAT_IDR] = idr;
      out[LGN_STAT_MAD] = mad;
      out[LGN_STAT_MAX] = value_of(a[n - 1]);
      out[LGN_STAT_MIN] = value_of(a[0]);
      out[LGN_STAT_ABS_MIN] = amin;
      out[LGN_STAT_FWHM] = qnan();                            // lgn_hist_fwhm_f64's
      out[LGN_STAT_Q10] = q10;
      out[LGN_STAT_Q90] = q90;
      run[0] = lower_index(a, n, -iqr, true);                  // |a| < IQR  <=>  -IQR < a < IQR
      run[1] = lower_index(a, n, iqr, false);
      run[2] = lower_index(a, n, -idr, true);
      run[3] = lower_index(a, n, idr, false);
      if (run[1] < run[0]) run[1] = run[0];                    // IQR = 0: an empty run
      if (run[3] < run[2]) run[3] = run[2];
      s_edge[0] = med - c.alpha * iqr;
      s_edge[1] = med + c.alpha * iqr;
    }
  }
  __syncthreads();
  if (c.num_edges) {           // np.linspace(start, stop, num): arange(num) * step + start, the last element stop itself
    const double start = s_edge[0], stop = s_edge[1], step = (stop - start) / (double)(c.num_edges - 1);
    double* e = c.edges + (long long)k * c.num_edges;
    for (int i = threadIdx.x; i < c.num_edges; i += SB) e[i] = i == c.num_edges - 1 ? stop : (double)i * step + start;
  }
}

// ---- 4. moments ------------------------------------------------------------------------------------------------------------------
template <int PASS>
__global__ __launch_bounds__(SB) void stats_partial(StatsCtx c) {
  __shared__ double ws[SB / 64];
  const int k = blockIdx.y;
  const long long n = *c.count, i0 = (long long)blockIdx.x * ST + threadIdx.x * SI;
  if ((long long)blockIdx.x * ST >= n || c.status[k]) return;
  const u64* a = c.sorted + (long long)k * c.rows;
  const long long* run = c.runs + k * 4;
  const double mean = c.stats[(long long)k * NSTAT + LGN_STAT_MEAN];
  double s[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
  for (int e = 0; e < SI; ++e) {
    const long long i = i0 + e;
    if (i >= n) break;
    const double v = value_of(a[i]);
    if constexpr (PASS == 0) {
      const double av = fabs(v);
      s[0] += v;
      s[1] += av;
      if (i >= run[0] && i < run[1]) s[2] += av;
      if (i >= run[2] && i < run[3]) s[3] += av;
    } else {
      const double d = v - mean, d2 = d * d;
      s[0] += d2;
      s[1] += d2 * d;
      s[2] += d2 * d2;
    }
  }
  double* p = c.part + ((long long)k * c.nb + blockIdx.x) * 4;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const double t = block_sum_fixed<SB>(s[q], ws);
    if (threadIdx.x == 0) p[q] = t;
  }
}

template <int PASS>
__global__ __launch_bounds__(SB) void stats_final(StatsCtx c) {
  __shared__ double ws[SB / 64];
  const int k = blockIdx.x;
  if (c.status[k]) return;
  const long long n = *c.count;
  const int nbn = (int)((n + ST - 1) / ST);                   // the partials of this call's n: the rest were not written
  const double* p = c.part + (long long)k * c.nb * 4;
  double s[4] = {0.0, 0.0, 0.0, 0.0};
  for (int q = threadIdx.x; q < nbn; q += SB) {
#pragma unroll
    for (int j = 0; j < 4; ++j) s[j] += p[4 * q + j];
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) s[j] = block_sum_fixed<SB>(s[j], ws);
  if (threadIdx.x) return;
  double* out = c.stats + (long long)k * NSTAT;
  const double dn = (double)n;
  if constexpr (PASS == 0) {
    const long long* run = c.runs + k * 4;
    out[LGN_STAT_MEAN] = s[0] / dn;
    out[LGN_STAT_ABS_MEAN] = s[1] / dn;
    out[LGN_STAT_ABS_MEAN_WITHIN_IQR] = run[1] > run[0] ? s[2] / (double)(run[1] - run[0]) : 1e32;
    out[LGN_STAT_ABS_MEAN_WITHIN_IDR] = run[3] > run[2] ? s[3] / (double)(run[3] - run[2]) : 1e32;
  } else {
    const double m2 = s[0] / dn, m3 = s[1] / dn, m4 = s[2] / dn;
    out[LGN_STAT_STD_DEV] = sqrt(m2);
    out[LGN_STAT_SKEW] = m3 / pow(m2, 1.5);
    out[LGN_STAT_KURTOSIS] = m4 / (m2 * m2) - 3.0;
  }
}

struct StatsLayout {
  long long key_a, key_b, blk, count, part, runs, total;
  int nb;
};
inline StatsLayout stats_layout(long long rows, int cols) {
  StatsLayout l;
  l.nb = (int)((rows + ST - 1) / ST);
  if (l.nb < 1) l.nb = 1;
  long long o = 0;
  l.key_a = o; o += up256(8 * rows * cols);
  l.key_b = o; o += up256(8 * rows * cols);
  l.blk = o; o += up256(4ll * l.nb);
  l.count = o; o += 256;
  l.part = o; o += up256(32ll * l.nb * cols);
  l.runs = o; o += up256(32ll * cols);
  l.total = o;
  return l;
}

// ---- find_fwhm on the output of lgn_histogram_f64 -----------------------------------------------------------------------------
struct FwhmCols {
  int n_edges[LGN_HIST_MAX_COLS];
};
// the first lane holding the best value wins, as np.argmax / np.argmin take the first
template <typename T, bool MAX>
__device__ __forceinline__ void wave_arg(T& v, int& i) {
#pragma unroll
  for (int m = 32; m > 0; m >>= 1) {
    const T ov = __shfl_xor(v, m, 64);
    const int oi = __shfl_xor(i, m, 64);
    const bool better = MAX ? ov > v : ov < v;
    if (better || (ov == v && oi < i)) { v = ov; i = oi; }
  }
}
__global__ __launch_bounds__(64) void hist_fwhm_kernel(const long long* __restrict__ counts, int max_bins,
                                                       const double* __restrict__ edges, int max_edges, const FwhmCols nc,
                                                       double* __restrict__ fwhm) {
  const int k = blockIdx.x, lane = threadIdx.x, nb = nc.n_edges[k] - 1;
  const long long* h = counts + (long long)k * max_bins;
  long long best = -0x7FFFFFFFFFFFFFFFll - 1;
  int bi = 0x7FFFFFFF;
  for (int b = lane; b < nb; b += 64)
    if (h[b] > best) { best = h[b]; bi = b; }
  wave_arg<long long, true>(best, bi);
  const double half = (double)best / 2.0;
  double dist = INFINITY;
  int di = 0x7FFFFFFF;
  for (int b = lane; b < nb; b += 64) {
    const double d = fabs((double)h[b] - half);
    if (d < dist) { dist = d; di = b; }
  }
  wave_arg<double, false>(dist, di);
  if (lane == 0) {
    const double* e = edges + (long long)k * max_edges;
    fwhm[k] = 2.0 * fabs(e[bi] - e[di]);
  }
}

// ---- jet images ----------------------------------------------------------------------------------------------------------------
constexpr int JW = 2;                          // waves per workgroup: each holds an image and a running sum of npix^2 doubles
constexpr int JP = LGN_JET_IMAGE_PARTS;

__host__ __device__ constexpr size_t ji_wave_bytes(int N, int npix) {
  return (size_t)(2 * npix * npix + N) * sizeof(double) + (size_t)N * sizeof(int);
}
inline size_t ji_lds_bytes(int N, int npix) { return (size_t)(npix + 1) * sizeof(double) + JW * ((ji_wave_bytes(N, npix) + 7) / 8 * 8); }

// frame [B][3] = (Pt, Eta, Phi) of the summed massless particles, summed in particle order; *any_far != 0 once some |Pt| > 1e-8
// (np.isclose(Pt, 0) with its defaults fails), NaN and inf included
__global__ __launch_bounds__(64 * JW) void jet_frame_kernel(const double* __restrict__ jets, int B, int N, double* __restrict__ frame,
                                                            int* any_far) {
  extern __shared__ __align__(16) double lds[];
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const long long b = (long long)blockIdx.x * JW + w;
  if (b >= B) return;
  double* P = lds + (size_t)w * 3 * N;
  for (int i = lane; i < N; i += 64) {
    const double* p = jets + (b * N + i) * 3;
    P[i] = p[0] * cos(p[2]);
    P[N + i] = p[0] * sin(p[2]);
    P[2 * N + i] = p[0] * sinh(p[1]);
  }
  wave_sync();
  double s = 0.0;
  if (lane < 3)
    for (int i = 0; i < N; ++i) s = s + P[lane * N + i];
  const double px = __shfl(s, 0, 64), py = __shfl(s, 1, 64), pz = __shfl(s, 2, 64);
  if (lane == 0) {
    const double pt = hypot(px, py);
    frame[b * 3] = pt;
    frame[b * 3 + 1] = asinh(pz / pt);
    frame[b * 3 + 2] = atan2(py, px);
    if (!(fabs(pt) <= 1e-8)) atomicOr(any_far, 1);
  }
}

__global__ void jet_clear_kernel(int* any_far) { *any_far = 0; }

__global__ __launch_bounds__(64 * JW) void jet_image_kernel(const double* __restrict__ jets, const double* __restrict__ frame,
                                                            const int* __restrict__ any_far, int B, int N, int npix, double maxR,
                                                            int first_n, int parts, double* __restrict__ images,
                                                            double* __restrict__ part) {
  extern __shared__ __align__(16) double lds[];
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63, np2 = npix * npix;
  const int q = blockIdx.x * JW + w;
  double* bins = lds;                                                       // [npix + 1], the workgroup's
  char* mine = reinterpret_cast<char*>(lds + npix + 1) + (size_t)w * ((ji_wave_bytes(N, npix) + 7) / 8 * 8);
  double* img = reinterpret_cast<double*>(mine);                            // [npix][npix] the current jet's image
  double* acc = img + np2;                                                  // [npix][npix] the sum over this part's jets
  double* pv = acc + np2;                                                   // [N] pt of a particle (in the frame, if any)
  int* pix = reinterpret_cast<int*>(pv + N);                                // [N] pixel of a particle, -1: none
  {
    const double start = -maxR, step = (maxR - start) / (double)npix;       // np.linspace(-maxR, maxR, npix + 1)
    for (int i = threadIdx.x; i <= npix; i += 64 * JW) bins[i] = i == npix ? maxR : (double)i * step + start;
  }
  __syncthreads();
  if (q >= parts) return;                  // whole waves leave; nothing below waits on the workgroup
  for (int i = lane; i < np2; i += 64) img[i] = 0.0, acc[i] = 0.0;
  const bool norm = frame && *any_far;
  for (long long b = q; b < B; b += parts) {
    wave_sync();
    for (int i = lane; i < N; i += 64) {
      const double* p = jets + (b * N + i) * 3;
      double pt = p[0], eta = p[1], phi = p[2];
      if (norm) {
        pt = pt / frame[b * 3];
        eta = eta - frame[b * 3 + 1];
        phi = wrap_phi(phi - frame[b * 3 + 2]);
      }
      int bin[2];
#pragma unroll
      for (int a = 0; a < 2; ++a) {        // np.digitize(v, bins) - 1: the i with bins[i] <= v < bins[i + 1]; NaN compares false
        const double v = a ? phi : eta;
        int lo = 0, hi = npix + 1;
        while (lo < hi) {
          const int mid = (lo + hi) >> 1;
          if (bins[mid] <= v) lo = mid + 1;
          else hi = mid;
        }
        bin[a] = lo - 1;
      }
      pv[i] = pt;
      pix[i] = (bin[0] >= 0 && bin[0] < npix && bin[1] >= 0 && bin[1] < npix)
                   ? bin[1] * npix + bin[0] : -1;
    }
    wave_sync();
    if (lane == 0)
      for (int i = 0; i < N; ++i)
        if (pix[i] >= 0) img[pix[i]] += pv[i];
    wave_sync();
    if (b < first_n)
      for (int i = lane; i < np2; i += 64) images[b * np2 + i] = img[i];
    wave_sync();
    if (lane == 0)
      for (int i = 0; i < N; ++i)
        if (pix[i] >= 0) {
          acc[pix[i]] += img[pix[i]];      // a pixel met twice adds 0 the second time
          img[pix[i]] = 0.0;
        }
  }
  wave_sync();
  for (int i = lane; i < np2; i += 64) part[(long long)q * np2 + i] = acc[i];
}

__global__ void jet_average_kernel(const double* __restrict__ part, int parts, int np2, int B, double* __restrict__ average) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= np2) return;
  double s = 0.0;
  for (int q = 0; q < parts; ++q) s = s + part[(long long)q * np2 + i];
  average[i] = s / (double)B;
}

struct JetLayout {
  long long frame, any_far, part, total;
  int parts;
};
inline JetLayout jet_layout(int B, int npix) {
  JetLayout l;
  l.parts = B < JP ? B : JP;
  long long o = 0;
  l.frame = o; o += up256(24ll * B);
  l.any_far = o; o += 256;
  l.part = o; o += up256(8ll * l.parts * npix * npix);
  l.total = o;
  return l;
}

}  // namespace
}  // namespace lgn

using namespace lgn;

extern "C" {

long long lgn_column_stats_workspace_bytes(long long rows, int cols) {
  if (rows < 0 || rows >= (1ll << 31) || cols < 1 || cols > LGN_STATS_MAX_COLS) {
    set_error("column_stats_workspace_bytes: rows = %lld, cols = %d (0 <= rows < 2^31, 1 <= cols <= %d)", rows, cols,
              LGN_STATS_MAX_COLS);
    return -1;
  }
  return stats_layout(rows, cols).total;
}

int lgn_column_stats_f64(const double* x, long long rows, int ld, int cols, const uint8_t* mask, int mask_keep, double alpha,
                         int num_edges, double* stats, double* edges, long long* kept, int* status, void* workspace,
                         long long workspace_bytes, void* stream) {
  LGN_CHECK_ARG(rows >= 0 && rows < (1ll << 31), "column_stats: rows = %lld (0 <= rows < 2^31)", rows);
  LGN_CHECK_ARG(cols >= 1 && cols <= LGN_STATS_MAX_COLS, "column_stats: cols = %d (1 <= cols <= %d)", cols, LGN_STATS_MAX_COLS);
  LGN_CHECK_ARG(ld >= cols, "column_stats: ld = %d < cols = %d", ld, cols);
  LGN_CHECK_ARG(num_edges == 0 || (num_edges >= 2 && num_edges <= LGN_HIST_MAX_EDGES),
                "column_stats: num_edges = %d (0, or 2 .. %d)", num_edges, LGN_HIST_MAX_EDGES);
  LGN_CHECK_ARG(alpha - alpha == 0.0, "column_stats: alpha is not finite");
  LGN_CHECK_ARG((x || rows == 0) && stats && kept && status && workspace && (edges || num_edges == 0), "column_stats: null pointer");
  const StatsLayout l = stats_layout(rows, cols);
  LGN_CHECK_ARG(workspace_bytes >= l.total, "column_stats: workspace of %lld bytes is too short (%lld needed)", workspace_bytes,
                l.total);
  LGN_CHECK_ARG((reinterpret_cast<uintptr_t>(workspace) & 7) == 0, "column_stats: the workspace must be 8-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  char* w = static_cast<char*>(workspace);
  StatsCtx c;
  c.x = x; c.mask = mask; c.rows = rows; c.ld = ld; c.cols = cols; c.mask_keep = mask_keep; c.nb = l.nb; c.num_edges = num_edges;
  c.alpha = alpha;
  c.key_a = reinterpret_cast<u64*>(w + l.key_a);
  c.key_b = reinterpret_cast<u64*>(w + l.key_b);
  c.blk = reinterpret_cast<int*>(w + l.blk);
  c.count = reinterpret_cast<long long*>(w + l.count);
  c.part = reinterpret_cast<double*>(w + l.part);
  c.runs = reinterpret_cast<long long*>(w + l.runs);
  c.stats = stats; c.edges = edges; c.kept = kept; c.status = status;
  c.sorted = c.key_a;
  const dim3 grid(l.nb, cols), percol(cols);

  stats_count<<<l.nb, SB, 0, s>>>(c);
  stats_scan<<<1, SB, 0, s>>>(c);
  stats_scatter<<<grid, SB, 0, s>>>(c);
  stats_tile_sort<<<grid, SB, 0, s>>>(c);
  u64* key[2] = {c.key_a, c.key_b};
  int cur = 0;
  for (long long W = ST; W < rows; W *= 2, cur ^= 1)
    stats_merge_pass<<<grid, SB, 0, s>>>(key[cur], key[cur ^ 1], rows, c.count, W);
  c.sorted = key[cur];
  stats_select<<<percol, SB, 0, s>>>(c);
  stats_partial<0><<<grid, SB, 0, s>>>(c);
  stats_final<0><<<percol, SB, 0, s>>>(c);
  stats_partial<1><<<grid, SB, 0, s>>>(c);
  stats_final<1><<<percol, SB, 0, s>>>(c);
  LGN_CHECK_LAUNCH();
  return 0;
}

int lgn_hist_fwhm_f64(const long long* counts, int max_bins, const double* edges, int max_edges, const int* n_edges, int cols,
                      double* fwhm, void* stream) {
  LGN_CHECK_ARG(counts && edges && n_edges && fwhm, "hist_fwhm: null pointer");
  LGN_CHECK_ARG(cols >= 1 && cols <= LGN_HIST_MAX_COLS, "hist_fwhm: cols = %d (1 <= cols <= %d)", cols, LGN_HIST_MAX_COLS);
  LGN_CHECK_ARG(max_edges >= 2 && max_edges <= LGN_HIST_MAX_EDGES && max_bins >= max_edges - 1,
                "hist_fwhm: max_edges = %d, max_bins = %d (2 <= max_edges <= %d, max_bins >= max_edges - 1)", max_edges, max_bins,
                LGN_HIST_MAX_EDGES);
  FwhmCols nc{};
  for (int k = 0; k < cols; ++k) {
    LGN_CHECK_ARG(n_edges[k] >= 2 && n_edges[k] <= max_edges, "hist_fwhm: n_edges[%d] = %d (2 .. max_edges = %d)", k, n_edges[k],
                  max_edges);
    nc.n_edges[k] = n_edges[k];
  }
  hist_fwhm_kernel<<<cols, 64, 0, (hipStream_t)stream>>>(counts, max_bins, edges, max_edges, nc, fwhm);
  LGN_CHECK_LAUNCH();
  return 0;
}

long long lgn_jet_images_workspace_bytes(int B, int npix) {
  if (B < 1 || npix < 1 || npix > LGN_JET_IMAGE_MAX_NPIX) {
    set_error("jet_images_workspace_bytes: B = %d, npix = %d (B >= 1, 1 <= npix <= %d)", B, npix, LGN_JET_IMAGE_MAX_NPIX);
    return -1;
  }
  return jet_layout(B, npix).total;
}

int lgn_jet_images_f64(const double* jets, const double* frame_jets, int B, int N, int mode, int npix, double maxR, int first_n,
                       double* images, double* average, void* workspace, long long workspace_bytes, void* stream) {
  LGN_CHECK_ARG(B >= 1, "jet_images: B = %d (need B >= 1)", B);
  LGN_CHECK_ARG(N >= 1 && N <= LGN_ANOMALY_NMAX, "jet_images: N = %d outside 1 .. %d", N, LGN_ANOMALY_NMAX);
  LGN_CHECK_ARG(npix >= 1 && npix <= LGN_JET_IMAGE_MAX_NPIX, "jet_images: npix = %d outside 1 .. %d", npix, LGN_JET_IMAGE_MAX_NPIX);
  LGN_CHECK_ARG(maxR - maxR == 0.0 && maxR > 0.0, "jet_images: maxR must be a finite positive number");
  LGN_CHECK_ARG(mode >= 0 && mode <= 2, "jet_images: mode = %d (0, 1 or 2)", mode);
  LGN_CHECK_ARG(first_n >= 0, "jet_images: first_n = %d < 0", first_n);
  LGN_CHECK_ARG(jets && average && workspace && (images || first_n == 0) && (frame_jets || mode != 2), "jet_images: null pointer");
  const JetLayout l = jet_layout(B, npix);
  LGN_CHECK_ARG(workspace_bytes >= l.total, "jet_images: workspace of %lld bytes is too short (%lld needed)", workspace_bytes, l.total);
  LGN_CHECK_ARG((reinterpret_cast<uintptr_t>(workspace) & 7) == 0, "jet_images: the workspace must be 8-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  char* w = static_cast<char*>(workspace);
  double* frame = reinterpret_cast<double*>(w + l.frame);
  int* any_far = reinterpret_cast<int*>(w + l.any_far);
  double* part = reinterpret_cast<double*>(w + l.part);
  if (mode) {
    jet_clear_kernel<<<1, 1, 0, s>>>(any_far);
    jet_frame_kernel<<<(B + JW - 1) / JW, 64 * JW, (size_t)JW * 3 * N * sizeof(double), s>>>(mode == 2 ? frame_jets : jets, B, N, frame,
                                                                                              any_far);
  }
  const size_t smem = ji_lds_bytes(N, npix);
  if (const int rc = lds_launch(jet_image_kernel, "jet_images", dim3((l.parts + JW - 1) / JW), dim3(64 * JW), smem, s, jets, mode ? frame : nullptr,
                                any_far, B, N, npix, maxR, first_n < B ? first_n : B, l.parts, images, part))
    return rc;
  jet_average_kernel<<<(npix * npix + 255) / 256, 256, 0, s>>>(part, l.parts, npix * npix, B, average);
  LGN_CHECK_LAUNCH();
  return 0;
}

}  // extern "C"
