// lgn-autoencoder_amd/csrc/roc.hip -- ROC curves and AUCs of the anomaly scores (the reference's get_ROC_AUC(),
// utils/jet_analysis/anomaly_detection.py): per score column sklearn.metrics.roc_curve(labels, scores[:, k]) with its defaults, then
// sklearn.metrics.auc, then the reference's flip when the AUC is below 0.5.  Entry points: lgn_roc_workspace_bytes, lgn_roc_auc_f64.
//
// Stages, all batched over the K columns (blockIdx.y), all on the caller's stream, nothing allocated, no host wait:
//   1. keys + tile sort   score -> 64-bit key whose unsigned order is the descending order of the doubles (-0.0 == +0.0), one label
//                         bit per row; a bitonic sort of LGN_ROC_TILE pairs in LDS.  Also the status bits of the column.
//   2. merge passes       ceil(log2(M / tile)) passes between two buffers; a workgroup writes one tile of the output, located by a
//                         merge-path search in global memory, and merges it in LDS (a second merge-path search per thread).
//   3. three scans        (block sums | scan of the block sums | apply) x (cumulative positives, tie-group ends, kept points); the
//                         third apply writes fpr, tpr and thresholds.
//   4. AUC                trapezoid terms summed in a fixed order (thread-serial, fixed shuffle tree, block partials in order) for the
//                         curve and for the curve with fpr and tpr exchanged; the flip is decided on the device, then a swap pass.
// The order inside a group of equal keys is free: every later stage reads the last row of a tie group only.
// Rates are single IEEE divisions and the trapezoid terms are rounded one operation at a time: no contraction into FMAs.
#pragma clang fp contract(off)
#include "common.hpp"
#include "../../include/lgn_amd.h"
#include "sort_dev.hpp"

namespace lgn {
namespace {

constexpr int RT = LGN_ROC_TILE;        // pairs per sort tile, per merge chunk and per scan block
constexpr int RB = 256;                 // threads per workgroup
constexpr int RI = RT / RB;             // consecutive items of a thread
static_assert(RT == RB * RI && (RT & (RT - 1)) == 0, "the tile is a power of two and a multiple of the workgroup");

// label classes met (one word for the call: the labels are the same for every column)
constexpr int LAB_POS = 1, LAB_ZERO = 2, LAB_NEG = 4, LAB_OTHER = 8;

struct RocCtx {
  const u64* keys;      // [K][M] sorted
  const uint8_t* bits;  // [K][M] label bit of the sorted rows
  int* cum;             // [K][M] positives in sorted rows 0 .. i
  int* gidx;            // [K][M] sorted row of the last member of tie group g
  int* sums;            // [K][nb] block sums, then their exclusive scan
  int* totals;          // [K][4]: positives, tie groups, kept points
  double* part;         // [K][nb][2] AUC partials: the curve, the exchanged curve
  int* labstat;         // [1]
  long long M;
  int nb;
  double *fpr, *tpr, *thr;   // [K][M + 1]
  int *length, *flipped, *status;
  double* auc;
};

// unsigned order of the keys = descending order of the doubles
__device__ __forceinline__ u64 roc_key(double x) {
  if (x == 0.0) x = 0.0;                                   // -0.0 ties with +0.0
  return ~key_of(x);
}
__device__ __forceinline__ double roc_value(u64 key) { return value_of(~key); }

// ---- 1. keys, status, tile sort --------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(RB) void roc_init(int* status, int* labstat, int K) {
  const int t = blockIdx.x * RB + threadIdx.x;
  if (t < K) status[t] = 0;
  if (t == 0) *labstat = 0;
}

__global__ __launch_bounds__(RB) void roc_tile_sort(const double* __restrict__ scores, long long M, int ld,
                                                    const double* __restrict__ labels, u64* __restrict__ keys,
                                                    uint8_t* __restrict__ bits, int* status, int* labstat) {
  __shared__ u64 sk[RT];
  __shared__ uint8_t sb[RT];
  __shared__ int s_lab, s_bad;
  const int tid = threadIdx.x, k = blockIdx.y;
  const long long base = (long long)blockIdx.x * RT;
  const int n = (int)(M - base < RT ? M - base : RT);       // 1 .. RT rows of this tile
  const int p2 = bitonic_size(n);
  if (tid == 0) { s_lab = 0; s_bad = 0; }
  __syncthreads();
  int lab = 0, bad = 0;
  for (int j = tid; j < p2; j += RB) {
    u64 key = ~0ull;
    uint8_t b = 0;
    if (j < n) {
      const double x = scores[(base + j) * ld + k];
      const double l = labels[base + j];
      const u64 u = (u64)__double_as_longlong(x);
      if (nonfinite_bits(u)) bad |= LGN_ROC_NONFINITE | ((u & ~(F64_SIGN | F64_EXPO)) ? LGN_ROC_NAN : 0);
      lab |= l == 1.0 ? LAB_POS : l == 0.0 ? LAB_ZERO : l == -1.0 ? LAB_NEG : LAB_OTHER;
      key = roc_key(x);
      b = l == 1.0;
    }
    sk[j] = key;
    sb[j] = b;
  }
  if (bad) atomicOr(&s_bad, bad);
  if (k == 0) atomicOr(&s_lab, lab);
  bitonic_sort_lds<RB>(sk, sb, p2);
  const long long col = (long long)k * M + base;
  for (int j = tid; j < n; j += RB) {
    keys[col + j] = sk[j];
    bits[col + j] = sb[j];
  }
  if (tid == 0) {
    if (s_bad) atomicOr(&status[k], s_bad);
    if (k == 0) atomicOr(labstat, s_lab);
  }
}

// ---- 2. one merge pass: runs of W sorted rows -> runs of 2 W -------------------------------------------------------------------
__global__ __launch_bounds__(RB) void roc_merge_pass(const u64* __restrict__ kin, const uint8_t* __restrict__ bin,
                                                     u64* __restrict__ kout, uint8_t* __restrict__ bout, long long M, long long W) {
  merge_chunk<RT, RB>(kin, bin, kout, bout, (long long)blockIdx.y * M, M, W);
}

// ---- 3. batched exclusive int32 scan: block sums, scan of the block sums, apply ----------------------------------------------
// the value scanned at position i < M of column k.  0: the label bit; 1: row i ends a tie group; 2: point i of the tie-group
// sequence is kept by roc_curve's drop_intermediate (first, last, or a nonzero second difference of fps or tps)
template <int STAGE>
__device__ __forceinline__ int roc_flag(const RocCtx& c, int k, long long i) {
  const long long col = (long long)k * c.M;
  if constexpr (STAGE == 0) return c.bits[col + i];
  if constexpr (STAGE == 1) return i == c.M - 1 || c.keys[col + i] != c.keys[col + i + 1];
  if constexpr (STAGE == 2) {
    const long long G = c.totals[k * 4 + 1];
    if (i >= G) return 0;
    if (G <= 2 || i == 0 || i == G - 1) return 1;
    const long long r0 = c.gidx[col + i - 1], r1 = c.gidx[col + i], r2 = c.gidx[col + i + 1];
    const long long t0 = c.cum[col + r0], t1 = c.cum[col + r1], t2 = c.cum[col + r2];
    const long long f0 = r0 + 1 - t0, f1 = r1 + 1 - t1, f2 = r2 + 1 - t2;
    return (f2 - 2 * f1 + f0) != 0 || (t2 - 2 * t1 + t0) != 0;
  }
  return 0;
}

template <int STAGE>
__global__ __launch_bounds__(RB) void roc_block_sums(RocCtx c) {
  const int k = blockIdx.y;
  const long long i0 = (long long)blockIdx.x * RT + threadIdx.x * RI;
  int s = 0;
#pragma unroll
  for (int e = 0; e < RI; ++e)
    if (i0 + e < c.M) s += roc_flag<STAGE>(c, k, i0 + e);
  int total;
  block_excl_scan<RB>(s, total);
  if (threadIdx.x == 0) c.sums[(long long)k * c.nb + blockIdx.x] = total;
}

template <int STAGE>
__global__ __launch_bounds__(RB) void roc_scan_sums(RocCtx c) {
  const int k = blockIdx.x;
  int* s = c.sums + (long long)k * c.nb;
  int carry = 0;
  for (int base = 0; base < c.nb; base += RB) {
    const int q = base + threadIdx.x;
    const int v = q < c.nb ? s[q] : 0;
    int total;
    const int ex = block_excl_scan<RB>(v, total);
    if (q < c.nb) s[q] = carry + ex;
    carry += total;
  }
  if (threadIdx.x == 0) c.totals[k * 4 + STAGE] = carry;
}

template <int STAGE>
__global__ __launch_bounds__(RB) void roc_apply(RocCtx c) {
  const int k = blockIdx.y;
  const long long col = (long long)k * c.M, i0 = (long long)blockIdx.x * RT + threadIdx.x * RI;
  int f[RI], s = 0;
#pragma unroll
  for (int e = 0; e < RI; ++e) {
    f[e] = i0 + e < c.M ? roc_flag<STAGE>(c, k, i0 + e) : 0;
    s += f[e];
  }
  int total;
  int ex = c.sums[(long long)k * c.nb + blockIdx.x] + block_excl_scan<RB>(s, total);
  const long long out = (long long)k * (c.M + 1);
  if (STAGE == 2 && blockIdx.x == 0 && threadIdx.x == 0) {   // roc_curve's extra first point
    c.fpr[out] = 0.0;
    c.tpr[out] = 0.0;
    c.thr[out] = __longlong_as_double(0x7FF0000000000000ll);
  }
#pragma unroll
  for (int e = 0; e < RI; ++e) {
    const long long i = i0 + e;
    if (i >= c.M) break;
    if constexpr (STAGE == 0) {
      ex += f[e];
      c.cum[col + i] = ex;
    } else if (f[e]) {
      if constexpr (STAGE == 1) {
        c.gidx[col + ex] = (int)i;
      } else {
        const long long r = c.gidx[col + i];
        const int tps = c.cum[col + r], pos = c.totals[k * 4 + 0];
        const long long fps = r + 1 - tps, neg = c.M - pos;
        c.fpr[out + 1 + ex] = (double)fps / (double)neg;
        c.tpr[out + 1 + ex] = (double)tps / (double)pos;
        c.thr[out + 1 + ex] = roc_value(c.keys[col + r]);
      }
      ex += 1;
    }
  }
}

// ---- 4. AUC in a fixed order, flip --------------------------------------------------------------------------------------------
__global__ __launch_bounds__(RB) void roc_auc_partial(RocCtx c) {
  __shared__ double ws[RB / 64];
  const int k = blockIdx.y;
  const long long segs = c.totals[k * 4 + 2];                // points - 1
  const long long out = (long long)k * (c.M + 1), s0 = (long long)blockIdx.x * RT + threadIdx.x * RI;
  double a = 0.0, b = 0.0;
  if (s0 < segs) {
    double x0 = c.fpr[out + s0], y0 = c.tpr[out + s0];
#pragma unroll
    for (int e = 0; e < RI; ++e) {
      if (s0 + e >= segs) break;
      const double x1 = c.fpr[out + s0 + e + 1], y1 = c.tpr[out + s0 + e + 1];
      a += (x1 - x0) * (y1 + y0) / 2.0;
      b += (y1 - y0) * (x1 + x0) / 2.0;
      x0 = x1;
      y0 = y1;
    }
  }
  a = block_sum_fixed<RB>(a, ws);
  b = block_sum_fixed<RB>(b, ws);
  if (threadIdx.x == 0) {
    double* p = c.part + ((long long)k * c.nb + blockIdx.x) * 2;
    p[0] = a;
    p[1] = b;
  }
}

__global__ __launch_bounds__(RB) void roc_auc_final(RocCtx c) {
  __shared__ double ws[RB / 64];
  const int k = blockIdx.x;
  const double* p = c.part + (long long)k * c.nb * 2;
  double a = 0.0, b = 0.0;
  for (int q = threadIdx.x; q < c.nb; q += RB) {
    a += p[2 * q];
    b += p[2 * q + 1];
  }
  a = block_sum_fixed<RB>(a, ws);
  b = block_sum_fixed<RB>(b, ws);
  if (threadIdx.x == 0) {
    const int lab = *c.labstat;
    int st = c.status[k];
    if ((lab & LAB_OTHER) || ((lab & LAB_ZERO) && (lab & LAB_NEG))) st |= LGN_ROC_BAD_LABEL;
    else if (!(lab & LAB_POS) || !(lab & (LAB_ZERO | LAB_NEG))) st |= LGN_ROC_SINGLE_CLASS;
    const bool flip = st == 0 && a < 0.5;
    c.status[k] = st;
    c.length[k] = st ? 0 : c.totals[k * 4 + 2] + 1;
    c.flipped[k] = flip;
    c.auc[k] = st ? qnan() : flip ? b : a;
  }
}

__global__ __launch_bounds__(RB) void roc_swap(RocCtx c) {
  const int k = blockIdx.y;
  if (!c.flipped[k]) return;
  const long long L = c.length[k], out = (long long)k * (c.M + 1);
  const long long i0 = (long long)blockIdx.x * RT;
  for (long long i = i0 + threadIdx.x; i < i0 + RT && i < L; i += RB) {
    const double x = c.fpr[out + i];
    c.fpr[out + i] = c.tpr[out + i];
    c.tpr[out + i] = x;
  }
}

// ---- workspace -----------------------------------------------------------------------------------------------------------------
struct RocLayout {
  long long key_a, key_b, bit_a, bit_b, sums, totals, part, labstat, total;
  int nb;
};
inline RocLayout roc_layout(long long M, int K) {
  RocLayout l;
  l.nb = (int)((M + RT - 1) / RT);
  long long o = 0;
  l.key_a = o; o += up256(8 * M * K);
  l.key_b = o; o += up256(8 * M * K);      // after the sort the spare key buffer holds cum and gidx (2 x int32 per row)
  l.bit_a = o; o += up256(M * K);
  l.bit_b = o; o += up256(M * K);
  l.sums = o; o += up256(4ll * l.nb * K);
  l.totals = o; o += up256(16ll * K);
  l.part = o; o += up256(16ll * l.nb * K);
  l.labstat = o; o += 256;
  l.total = o;
  return l;
}

}  // namespace
}  // namespace lgn

using namespace lgn;

extern "C" {

long long lgn_roc_workspace_bytes(long long M, int K) {
  if (M < 1 || M >= (1ll << 31) || K < 1 || K > LGN_ROC_MAX_COLS) {
    set_error("roc_workspace_bytes: M = %lld, K = %d (1 <= M < 2^31, 1 <= K <= %d)", M, K, LGN_ROC_MAX_COLS);
    return -1;
  }
  return roc_layout(M, K).total;
}

int lgn_roc_auc_f64(const double* scores, long long M, int ld, int K, const double* labels, double* fpr, double* tpr,
                    double* thresholds, int* length, double* auc, int* flipped, int* status, void* workspace,
                    long long workspace_bytes, void* stream) {
  LGN_CHECK_ARG(scores && labels && fpr && tpr && thresholds && length && auc && flipped && status && workspace,
                "roc_auc: null pointer");
  LGN_CHECK_ARG(M >= 1 && M < (1ll << 31), "roc_auc: M = %lld (1 <= M < 2^31)", M);
  LGN_CHECK_ARG(K >= 1 && K <= LGN_ROC_MAX_COLS, "roc_auc: K = %d (1 <= K <= %d)", K, LGN_ROC_MAX_COLS);
  LGN_CHECK_ARG(ld >= K, "roc_auc: ld = %d < K = %d", ld, K);
  const RocLayout l = roc_layout(M, K);
  LGN_CHECK_ARG(workspace_bytes >= l.total, "roc_auc: workspace of %lld bytes is too short (%lld needed)", workspace_bytes, l.total);
  LGN_CHECK_ARG((reinterpret_cast<uintptr_t>(workspace) & 7) == 0, "roc_auc: the workspace must be 8-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  char* w = static_cast<char*>(workspace);
  u64* key[2] = {reinterpret_cast<u64*>(w + l.key_a), reinterpret_cast<u64*>(w + l.key_b)};
  uint8_t* bit[2] = {reinterpret_cast<uint8_t*>(w + l.bit_a), reinterpret_cast<uint8_t*>(w + l.bit_b)};
  int* labstat = reinterpret_cast<int*>(w + l.labstat);
  const dim3 grid(l.nb, K), cols(K);

  roc_init<<<dim3((K + RB - 1) / RB), RB, 0, s>>>(status, labstat, K);
  roc_tile_sort<<<grid, RB, 0, s>>>(scores, M, ld, labels, key[0], bit[0], status, labstat);
  int cur = 0;
  for (long long W = RT; W < M; W *= 2, cur ^= 1)
    roc_merge_pass<<<grid, RB, 0, s>>>(key[cur], bit[cur], key[cur ^ 1], bit[cur ^ 1], M, W);

  RocCtx c;
  c.keys = key[cur];
  c.bits = bit[cur];
  c.cum = reinterpret_cast<int*>(key[cur ^ 1]);
  c.gidx = c.cum + M * K;
  c.sums = reinterpret_cast<int*>(w + l.sums);
  c.totals = reinterpret_cast<int*>(w + l.totals);
  c.part = reinterpret_cast<double*>(w + l.part);
  c.labstat = labstat;
  c.M = M;
  c.nb = l.nb;
  c.fpr = fpr; c.tpr = tpr; c.thr = thresholds;
  c.length = length; c.flipped = flipped; c.status = status; c.auc = auc;
  roc_block_sums<0><<<grid, RB, 0, s>>>(c);
  roc_scan_sums<0><<<cols, RB, 0, s>>>(c);
  roc_apply<0><<<grid, RB, 0, s>>>(c);
  roc_block_sums<1><<<grid, RB, 0, s>>>(c);
  roc_scan_sums<1><<<cols, RB, 0, s>>>(c);
  roc_apply<1><<<grid, RB, 0, s>>>(c);
  roc_block_sums<2><<<grid, RB, 0, s>>>(c);
  roc_scan_sums<2><<<cols, RB, 0, s>>>(c);
  roc_apply<2><<<grid, RB, 0, s>>>(c);
  roc_auc_partial<<<grid, RB, 0, s>>>(c);
  roc_auc_final<<<cols, RB, 0, s>>>(c);
  roc_swap<<<dim3((unsigned)((M + 1 + RT - 1) / RT), K), RB, 0, s>>>(c);
  LGN_CHECK_LAUNCH();
  return 0;
}

}  // extern "C"
