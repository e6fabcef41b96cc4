// lgn-autoencoder_amd/csrc/sort_dev.hpp -- the device sort of double columns and the deterministic block scan and sum around it,
// shared by the ROC curves (roc.hip: keys with one payload byte per row) and the column statistics (stats.hip: keys only).
//
//   key map           double <-> 64-bit key whose unsigned order is the ascending order of the doubles (-0.0 below +0.0, NaNs at the
//                     two ends); the masks, the non-finite test on the bit pattern and the quiet NaN that go with it
//   block_excl_scan   exclusive int prefix over a workgroup's threads, and the workgroup's sum
//   block_sum_fixed   fp64 sum over a workgroup in a fixed order: xor butterfly from 32 down to 1, then the waves left to right
//   bitonic_sort_lds  sort of a power-of-two tile of keys (and their payloads) in LDS
//   merge_chunk       one workgroup's chunk of a merge pass: runs of W sorted rows -> runs of 2 W, located by merge-path searches
//   up256             workspace rounding (host)
// A sort is: a tile sort per TILE rows, then ceil(log2(M / TILE)) merge passes between two buffers, a workgroup per output chunk.
// The order inside a group of equal keys is not stable across the tile sort; the merge keeps the order of its runs.
//
// Integer code and plain additions only: nothing here can contract, so the header leaves the contraction mode of its includer alone.
#pragma once
#include <type_traits>

#include "common.hpp"

namespace lgn {

typedef unsigned long long u64;
constexpr u64 F64_SIGN = 0x8000000000000000ull;
constexpr u64 F64_EXPO = 0x7FF0000000000000ull;

__device__ __forceinline__ bool nonfinite_bits(u64 u) { return (u & F64_EXPO) == F64_EXPO; }      // inf or NaN
__device__ __forceinline__ double qnan() { return __longlong_as_double(0x7FF8000000000000ll); }

__device__ __forceinline__ u64 key_of(double x) {     // unsigned order of the keys = ascending order of the doubles
  const u64 u = (u64)__double_as_longlong(x);
  return (u & F64_SIGN) ? ~u : (u | F64_SIGN);
}
__device__ __forceinline__ double value_of(u64 a) {   // its inverse
  return __longlong_as_double((long long)((a & F64_SIGN) ? (a ^ F64_SIGN) : ~a));
}

// exclusive prefix of v over the workgroup's THREADS threads, and the workgroup's sum
template <int THREADS>
__device__ __forceinline__ int block_excl_scan(int v, int& total) {
  static_assert(THREADS % 64 == 0 && THREADS >= 64 && THREADS <= 1024, "whole waves of 64");
  __shared__ int ws[THREADS / 64];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  int inc = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int t = __shfl_up(inc, o, 64);
    if (lane >= o) inc += t;
  }
  __syncthreads();                       // the previous call's readers are done with ws
  if (lane == 63) ws[w] = inc;
  __syncthreads();
  int off = 0, tot = 0;
#pragma unroll
  for (int q = 0; q < THREADS / 64; ++q) {
    if (q < w) off += ws[q];
    tot += ws[q];
  }
  total = tot;
  return off + inc - v;
}

// the sum of v over the workgroup, the same bits on every thread and every run; ws holds THREADS / 64 doubles of LDS
template <int THREADS>
__device__ __forceinline__ double block_sum_fixed(double v, double* ws) {
  static_assert(THREADS % 64 == 0 && THREADS >= 64 && THREADS <= 1024, "whole waves of 64");
#pragma unroll
  for (int m = 32; m > 0; m >>= 1) v += __shfl_xor(v, m, 64);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) ws[threadIdx.x >> 6] = v;
  __syncthreads();
  double s = ws[0];
#pragma unroll
  for (int q = 1; q < THREADS / 64; ++q) s += ws[q];         // ((w0 + w1) + w2) + ..
  return s;
}

// rows of a taken before equal rows of b, everywhere: the splits of neighbouring chunks and threads then agree
template <typename I>
__device__ __forceinline__ I merge_path(const u64* a, I na, const u64* b, I nb, I diag) {
  I lo = diag > nb ? diag - nb : 0, hi = diag < na ? diag : na;
  while (lo < hi) {
    const I mid = lo + ((hi - lo) >> 1);
    if (a[mid] <= b[diag - 1 - mid]) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

struct NoPayload {};           // keys only: pass (NoPayload*)nullptr for every payload pointer

// the sort of n <= TILE rows runs on the next power of two (at least 2), the rows past n padded with the largest key ~0
__device__ __forceinline__ int bitonic_size(int n) {
  int p2 = 2;
  while (p2 < n) p2 <<= 1;
  return p2;
}

// sorts keys[0 .. p2) in LDS ascending, payload[] moving with its key; the caller has written both (no barrier needed before the
// call), and every thread may read them on return
template <int THREADS, typename Payload>
__device__ __forceinline__ void bitonic_sort_lds(u64* keys, Payload* payload, int p2) {
  for (int size = 2; size <= p2; size <<= 1) {
    for (int stride = size >> 1; stride > 0; stride >>= 1) {
      __syncthreads();
      for (int t = threadIdx.x; t < (p2 >> 1); t += THREADS) {
        const int lo = 2 * t - (t & (stride - 1)), hi = lo + stride;
        const bool up = (lo & size) == 0;
        const u64 a = keys[lo], c = keys[hi];
        if ((a > c) == up) {
          keys[lo] = c; keys[hi] = a;
          if constexpr (!std::is_same_v<Payload, NoPayload>) {
            const Payload pa = payload[lo]; payload[lo] = payload[hi]; payload[hi] = pa;
          }
        }
      }
    }
  }
  __syncthreads();
}

// One merge pass, the part of workgroup blockIdx.x: rows [blockIdx.x TILE, + TILE) of the output column at offset col, whose M rows
// are runs of W sorted rows in (kin, pin) and become runs of 2 W in (kout, pout).  An unpaired run is copied.  Every thread of the
// workgroup calls it, with blockIdx.x TILE < M.
template <int TILE, int THREADS, typename Payload>
__device__ __forceinline__ void merge_chunk(const u64* __restrict__ kin, const Payload* __restrict__ pin, u64* __restrict__ kout,
                                            Payload* __restrict__ pout, long long col, long long M, long long W) {
  constexpr bool PAY = !std::is_same_v<Payload, NoPayload>;
  constexpr int ITEMS = TILE / THREADS;                     // consecutive output rows of a thread
  static_assert(TILE == THREADS * ITEMS, "the chunk is a multiple of the workgroup");
  __shared__ u64 sk[TILE], ok[TILE];
  __shared__ Payload sp[TILE], op[TILE];                    // never referenced without a payload: no LDS then
  __shared__ long long s_split[2];
  const int tid = threadIdx.x;
  const long long o0 = (long long)blockIdx.x * TILE, o1 = o0 + TILE < M ? o0 + TILE : M;
  const long long pair0 = o0 / (2 * W) * (2 * W);           // W is a multiple of the chunk: a chunk lies inside one pair of runs
  const long long a_end = pair0 + W < M ? pair0 + W : M, b_end = pair0 + 2 * W < M ? pair0 + 2 * W : M;
  const long long na = a_end - pair0, nbb = b_end - a_end;  // an unpaired run has nbb = 0
  const u64* A = kin + col + pair0;
  const u64* B = kin + col + a_end;
  if (tid < 2) s_split[tid] = merge_path<long long>(A, na, B, nbb, (tid ? o1 : o0) - pair0);
  __syncthreads();
  const long long a0 = s_split[0], a1 = s_split[1], b0 = (o0 - pair0) - a0, b1 = (o1 - pair0) - a1;
  const int ca = (int)(a1 - a0), cb = (int)(b1 - b0), n = ca + cb;       // ca + cb = o1 - o0 <= TILE
  for (int j = tid; j < n; j += THREADS) {
    const long long src = j < ca ? pair0 + a0 + j : a_end + b0 + (j - ca);
    sk[j] = kin[col + src];
    if constexpr (PAY) sp[j] = pin[col + src];
  }
  __syncthreads();
  const int d = tid * ITEMS < n ? tid * ITEMS : n;
  int i = merge_path<int>(sk, ca, sk + ca, cb, d), j = d - i;
#pragma unroll
  for (int e = 0; e < ITEMS; ++e) {
    if (d + e < n) {
      const bool take_a = j >= cb || (i < ca && sk[i] <= sk[ca + j]);
      const int s = take_a ? i : ca + j;
      ok[d + e] = sk[s];
      if constexpr (PAY) op[d + e] = sp[s];
      i += take_a;
      j += !take_a;
    }
  }
  __syncthreads();
  for (int q = tid; q < n; q += THREADS) {
    kout[col + o0 + q] = ok[q];
    if constexpr (PAY) pout[col + o0 + q] = op[q];
  }
}

inline long long up256(long long b) { return (b + 255) / 256 * 256; }

}  // namespace lgn
