// lgn-autoencoder_amd/csrc/equivariance.hip -- the Lorentz-group equivariance test (lgn/models/autotest/lgn_tests.py of the
// reference: covariance_test, permutation_invariance_test, rotate_rep of g_lib/rotations.py and get_node_dev of autotest/utils.py)
// as two calls: the transformed copies of a batch, and the deviation statistics of every (irrep, layer, transformation) of one kind.
//
//   lgn_transform_jets_f64   out[t][b][n][:] = p4[b][perm ? perm[b][n] : n][:] @ R[t]: one thread per (t, b, n) row, the four
//                            components ((p0 R0a + p1 R1a) + p2 R2a) + p3 R3a as the reference's einsum("...b,ba->...a") sums them;
//                            R[t] is wave-uniform (scalar loads).  The optional scalars are gathered by the same permutation.
//   lgn_rep_deviation_f64    one workgroup per (part, tile of LGN_EQUI_TILE rows, transformation t).  A row is the d complex numbers
//                            of one (jet, particle, channel); a lane owns one ELEMENT (row, j) at a time, so consecutive lanes read
//                            consecutive doubles of a (both planes) whatever d is -- rows of 1, 3, 4 or 9 doubles have no vector
//                            width in common.  The tile's rows of b are read once, the same way, into LDS; the lane forms
//                            b'[j] = sum_k b[k] conj(D)[k][j] from its row there and D[t] (LDS too) and never stores it.  Five
//                            running values per lane, a 64-lane xor butterfly, the four waves through LDS in wave order, one
//                            partial row per workgroup; a second kernel adds the partial rows of each (part, t) in a fixed
//                            order.  No atomics: the same bits on every run.
//
// The maxima keep a NaN (torch.max does): a plain fmax would drop it.  A perm entry outside [0, N) forms no address: that row of b
// counts as NaN (transform_jets writes NaN rows), so a bad permutation shows in the result instead of reading out of bounds.
#include <math.h>

#include "common.hpp"
#include "../../include/lgn_amd.h"

namespace lgn {
namespace {

constexpr int EQ_BLOCK = 256;
constexpr int EQ_WAVES = EQ_BLOCK / 64;
constexpr int EQ_NSTAT = 5;
constexpr int EQ_MAX_D = 9;

struct EquiParts {           // by value in the kernel arguments (2.6 KB): nothing to upload, nothing to keep alive
  const double* a[LGN_EQUI_MAX_PARTS];
  const double* b[LGN_EQUI_MAX_PARTS];
  const double* D[LGN_EQUI_MAX_PARTS];
  int N[LGN_EQUI_MAX_PARTS], C[LGN_EQUI_MAX_PARTS], d[LGN_EQUI_MAX_PARTS];
  int tile0[LGN_EQUI_MAX_PARTS + 1];      // first tile of each part in the flattened grid; tile0[parts] = all tiles
};

__global__ void __launch_bounds__(EQ_BLOCK) transform_jets_kernel(const double* __restrict__ p4, const double* __restrict__ R,
                                                                  const int* __restrict__ perm, const double* __restrict__ scalars,
                                                                  int B, int N, int K, double* __restrict__ out,
                                                                  double* __restrict__ scalars_out) {
  const long long rows = (long long)B * N;
  const long long row = (long long)blockIdx.x * EQ_BLOCK + threadIdx.x;
  const int t = blockIdx.y;
  if (row >= rows) return;
  long long src = row;
  bool bad = false;
  if (perm) {
    const int n = (int)(row % N), pn = perm[row];
    bad = (unsigned)pn >= (unsigned)N;
    src = bad ? row : row - n + pn;
  }
  const double* r = R + (long long)t * 16;
  const double* p = p4 + src * 4;
  const double nan = __builtin_nan("");
  const double p0 = bad ? nan : p[0], p1 = bad ? nan : p[1], p2 = bad ? nan : p[2], p3 = bad ? nan : p[3];
  double* o = out + ((long long)t * rows + row) * 4;
#pragma unroll
  for (int c = 0; c < 4; ++c) o[c] = ((p0 * r[c] + p1 * r[4 + c]) + p2 * r[8 + c]) + p3 * r[12 + c];
  if (K > 0) {
    const double* s = scalars + src * K;
    double* so = scalars_out + ((long long)t * rows + row) * K;
    for (int k = 0; k < K; ++k) so[k] = bad ? nan : s[k];
  }
}

template <int d>
__device__ __forceinline__ void rep_deviation_tile(const EquiParts& P, int part, int tile, int t, int T, int B,
                                                   const int* __restrict__ perm, double* sD, double* sB, double (*red)[EQ_NSTAT],
                                                   double* __restrict__ partial_row) {
  const int N = P.N[part], C = P.C[part];
  const long long rows = (long long)B * N * C;                 // rows of one (part, t) block
  const double* a_r = P.a[part] + (long long)t * rows * d;
  const double* a_i = a_r + (long long)T * rows * d;
  const double* b_r = P.b[part];
  const double* b_i = b_r + rows * d;
  const double* Dt = P.D[part] + (long long)t * 2 * d * d;
  const int tid = threadIdx.x;
  if (tid < 2 * d * d) sD[tid] = Dt[tid];
  const double* Dr = sD;
  const double* Di = sD + d * d;

  const long long row0 = (long long)tile * LGN_EQUI_TILE;
  const int nrows = (int)(rows - row0 < LGN_EQUI_TILE ? rows - row0 : LGN_EQUI_TILE);
  const int nel = nrows * d;
  // the tile's rows of b, both planes, read once: consecutive lanes take consecutive doubles (without perm the tile is one
  // contiguous run of each plane; with it whole rows move)
  double* sBr = sB;
  double* sBi = sB + LGN_EQUI_TILE * d;
  for (int e = tid; e < nel; e += EQ_BLOCK) {
    const int r = e / d, j = e - r * d;
    const long long row = row0 + r;
    long long brow = row;
    bool bad = false;
    if (perm) {
      const long long bn = row / C;
      const int c = (int)(row - bn * C), n = (int)(bn % N), pn = perm[bn];
      bad = (unsigned)pn >= (unsigned)N;
      brow = bad ? row : (bn - n + pn) * C + c;
    }
    sBr[e] = bad ? __builtin_nan("") : b_r[brow * d + j];
    sBi[e] = bad ? __builtin_nan("") : b_i[brow * d + j];
  }
  __syncthreads();

  double s_diff = 0.0, s_b = 0.0, m_diff = 0.0, m_b = 0.0, m_rel = 0.0;
  for (int e = tid; e < nel; e += EQ_BLOCK) {
    const int r = e / d, j = e - r * d;
    const long long row = row0 + r;
    const double ar = a_r[row * d + j], ai = a_i[row * d + j];
    double pr = 0.0, pi = 0.0;                                   // b' = b conj(D): (b_r D_r + b_i D_i, -b_r D_i + b_i D_r)
#pragma unroll
    for (int k = 0; k < d; ++k) {
      const double x = sBr[r * d + k], y = sBi[r * d + k];
      const double dr = Dr[k * d + j], di = Di[k * d + j];
      pr = __builtin_fma(x, dr, pr);
      pr = __builtin_fma(y, di, pr);
      pi = __builtin_fma(-x, di, pi);
      pi = __builtin_fma(y, dr, pi);
    }
    const double er = ar - pr, ei = ai - pi;
    s_diff += er;
    s_diff += ei;
    s_b += pr;
    s_b += pi;
    m_diff = nan_max(nan_max(m_diff, fabs(er)), fabs(ei));
    m_b = nan_max(nan_max(m_b, fabs(pr)), fabs(pi));
    m_rel = nan_max(nan_max(m_rel, fabs(er / (pr + 1e-16))), fabs(ei / (pi + 1e-16)));
  }
#pragma unroll
  for (int m = 1; m < 64; m <<= 1) {
    s_diff += shfl_xor(s_diff, m);
    s_b += shfl_xor(s_b, m);
    m_diff = nan_max(m_diff, shfl_xor(m_diff, m));
    m_b = nan_max(m_b, shfl_xor(m_b, m));
    m_rel = nan_max(m_rel, shfl_xor(m_rel, m));
  }
  // (nan_max(x, y) and nan_max(y, x) agree: both NaN if either is, else the larger -- every lane holds the same bits)
  if ((tid & 63) == 0) {
    double* w = red[tid >> 6];
    w[0] = s_diff, w[1] = s_b, w[2] = m_diff, w[3] = m_b, w[4] = m_rel;
  }
  __syncthreads();
  if (tid == 0) {
    double v[EQ_NSTAT];
#pragma unroll
    for (int k = 0; k < EQ_NSTAT; ++k) v[k] = red[0][k];
#pragma unroll
    for (int w = 1; w < EQ_WAVES; ++w) {
      v[0] += red[w][0];
      v[1] += red[w][1];
#pragma unroll
      for (int k = 2; k < EQ_NSTAT; ++k) v[k] = nan_max(v[k], red[w][k]);
    }
#pragma unroll
    for (int k = 0; k < EQ_NSTAT; ++k) partial_row[k] = v[k];
  }
}

// partial [all tiles][T][5]
__global__ void __launch_bounds__(EQ_BLOCK) rep_deviation_kernel(const EquiParts P, int parts, int T, int B,
                                                                 const int* __restrict__ perm, double* __restrict__ partial) {
  __shared__ double sD[2 * EQ_MAX_D * EQ_MAX_D];
  __shared__ double sB[2 * LGN_EQUI_TILE * EQ_MAX_D];
  __shared__ double red[EQ_WAVES][EQ_NSTAT];
  const int bx = blockIdx.x, t = blockIdx.y;
  int part = 0;
  while (part + 1 < parts && P.tile0[part + 1] <= bx) ++part;
  const int tile = bx - P.tile0[part];
  double* row = partial + ((long long)bx * T + t) * EQ_NSTAT;
  switch (P.d[part]) {
    case 1: rep_deviation_tile<1>(P, part, tile, t, T, B, perm, sD, sB, red, row); break;
    case 3: rep_deviation_tile<3>(P, part, tile, t, T, B, perm, sD, sB, red, row); break;
    case 4: rep_deviation_tile<4>(P, part, tile, t, T, B, perm, sD, sB, red, row); break;
    default: rep_deviation_tile<9>(P, part, tile, t, T, B, perm, sD, sB, red, row); break;
  }
}

// one wavefront per (part, t): lane l takes the partial rows of tiles l, l + 64, ... in order, then the butterfly
__global__ void __launch_bounds__(64) rep_deviation_final_kernel(const EquiParts P, int T, const double* __restrict__ partial,
                                                                 double* __restrict__ stats) {
  const int part = blockIdx.x, t = blockIdx.y, lane = threadIdx.x;
  const int first = P.tile0[part], last = P.tile0[part + 1];
  double v[EQ_NSTAT] = {0.0, 0.0, 0.0, 0.0, 0.0};
  for (int tile = first + lane; tile < last; tile += 64) {
    const double* row = partial + ((long long)tile * T + t) * EQ_NSTAT;
    v[0] += row[0];
    v[1] += row[1];
#pragma unroll
    for (int k = 2; k < EQ_NSTAT; ++k) v[k] = nan_max(v[k], row[k]);
  }
#pragma unroll
  for (int m = 1; m < 64; m <<= 1) {
    v[0] += shfl_xor(v[0], m);
    v[1] += shfl_xor(v[1], m);
#pragma unroll
    for (int k = 2; k < EQ_NSTAT; ++k) v[k] = nan_max(v[k], shfl_xor(v[k], m));
  }
  if (lane == 0) {
    double* o = stats + ((long long)part * T + t) * EQ_NSTAT;
#pragma unroll
    for (int k = 0; k < EQ_NSTAT; ++k) o[k] = v[k];
  }
}

// shapes -> tiles; < 0 with the error set when they are refused
long long equi_layout(const char* who, int parts, int T, int B, const int* N, const int* C, const int* d, int* tile0 /*nullable*/) {
  LGN_CHECK_ARG(parts >= 1 && parts <= LGN_EQUI_MAX_PARTS, "%s: parts = %d (1 <= parts <= %d)", who, parts, LGN_EQUI_MAX_PARTS);
  LGN_CHECK_ARG(N && C && d, "%s: null pointer", who);
  LGN_CHECK_ARG(T >= 1 && T <= 65535, "%s: T = %d (1 <= T <= 65535)", who, T);
  LGN_CHECK_ARG(B >= 1, "%s: B = %d (need B >= 1)", who, B);
  long long tiles = 0;
  for (int p = 0; p < parts; ++p) {
    LGN_CHECK_ARG(N[p] >= 1 && C[p] >= 1, "%s: part %d has N = %d, C = %d (need N, C >= 1)", who, p, N[p], C[p]);
    LGN_CHECK_ARG(d[p] == 1 || d[p] == 3 || d[p] == 4 || d[p] == 9, "%s: part %d has d = %d (1, 3, 4 or 9)", who, p, d[p]);
    const long long rows = (long long)B * N[p] * C[p];
    LGN_CHECK_ARG(rows < (1ll << 31) / EQ_MAX_D, "%s: part %d has B * N * C = %lld rows (< 2^31 / 9)", who, p, rows);
    if (tile0) tile0[p] = (int)tiles;
    tiles += (rows + LGN_EQUI_TILE - 1) / LGN_EQUI_TILE;
  }
  LGN_CHECK_ARG(tiles < (1ll << 31) / T, "%s: %lld tiles x T = %d do not fit one grid", who, tiles, T);
  if (tile0) tile0[parts] = (int)tiles;
  return tiles;
}

}  // namespace
}  // namespace lgn

using namespace lgn;

extern "C" {

int lgn_transform_jets_f64(const double* p4, const double* R, const int* perm, const double* scalars, int T, int B, int N, int K,
                           double* out, double* scalars_out, void* stream) {
  LGN_CHECK_ARG(T >= 1 && T <= 65535, "transform_jets: T = %d (1 <= T <= 65535)", T);
  LGN_CHECK_ARG(B >= 1 && N >= 1, "transform_jets: B = %d, N = %d (need B, N >= 1)", B, N);
  LGN_CHECK_ARG(K >= 0, "transform_jets: K = %d < 0", K);
  LGN_CHECK_ARG((long long)B * N < (1ll << 31), "transform_jets: B * N = %lld rows (< 2^31)", (long long)B * N);
  LGN_CHECK_ARG(p4 && R && out && (K == 0 || (scalars && scalars_out)), "transform_jets: null pointer");
  const long long rows = (long long)B * N;
  const dim3 grid((unsigned)((rows + EQ_BLOCK - 1) / EQ_BLOCK), (unsigned)T);
  transform_jets_kernel<<<grid, EQ_BLOCK, 0, (hipStream_t)stream>>>(p4, R, perm, scalars, B, N, K, out, scalars_out);
  LGN_CHECK_LAUNCH();
  return 0;
}

long long lgn_rep_deviation_workspace_bytes(int parts, int T, int B, const int* N, const int* C, const int* d) {
  const long long tiles = equi_layout("rep_deviation_workspace_bytes", parts, T, B, N, C, d, nullptr);
  return tiles < 0 ? -1 : tiles * T * EQ_NSTAT * (long long)sizeof(double);
}

int lgn_rep_deviation_f64(int parts, int T, int B, const double* const* a, const double* const* b, const double* const* D,
                          const int* N, const int* C, const int* d, const int* perm, double* stats, void* workspace,
                          long long workspace_bytes, void* stream) {
  EquiParts P;
  const long long tiles = equi_layout("rep_deviation", parts, T, B, N, C, d, P.tile0);
  if (tiles < 0) return -1;
  LGN_CHECK_ARG(a && b && D && stats && workspace, "rep_deviation: null pointer");
  for (int p = 0; p < parts; ++p) {
    LGN_CHECK_ARG(a[p] && b[p] && D[p], "rep_deviation: null pointer in part %d", p);
    LGN_CHECK_ARG(!perm || N[p] == N[0], "rep_deviation: with perm every part has the same N (part %d: %d, part 0: %d)", p, N[p], N[0]);
    P.a[p] = a[p], P.b[p] = b[p], P.D[p] = D[p];
    P.N[p] = N[p], P.C[p] = C[p], P.d[p] = d[p];
  }
  for (int p = parts; p < LGN_EQUI_MAX_PARTS; ++p) {
    P.a[p] = P.b[p] = P.D[p] = nullptr;
    P.N[p] = P.C[p] = P.d[p] = 0;
    P.tile0[p + 1] = (int)tiles;
  }
  const long long need = tiles * T * EQ_NSTAT * (long long)sizeof(double);
  LGN_CHECK_ARG(workspace_bytes >= need, "rep_deviation: workspace of %lld bytes is too short (%lld needed)", workspace_bytes, need);
  LGN_CHECK_ARG((reinterpret_cast<uintptr_t>(workspace) & 7) == 0, "rep_deviation: the workspace must be 8-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  double* partial = reinterpret_cast<double*>(workspace);
  rep_deviation_kernel<<<dim3((unsigned)tiles, (unsigned)T), EQ_BLOCK, 0, s>>>(P, parts, T, B, perm, partial);
  LGN_CHECK_LAUNCH();
  rep_deviation_final_kernel<<<dim3((unsigned)parts, (unsigned)T), 64, 0, s>>>(P, T, partial, stats);
  LGN_CHECK_LAUNCH();
  return 0;
}

}  // extern "C"
