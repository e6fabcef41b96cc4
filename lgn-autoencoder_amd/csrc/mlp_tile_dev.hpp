// lgn-autoencoder_amd/csrc/mlp_tile_dev.hpp -- what the tiled matrix-core CGMLP kernels share: mlp_mfma.hip (H <= 48) and
// mlp_mfma_wide.hip (48 < H <= 96).  Every Linear is a [rows x Hin] x [Hin x Hout] GEMM on v_mfma_f64_16x16x4_f64
// (D(16x16) += A(16x4) B(4x16)):
//   A: lane l holds A[i = l&15][k = l>>4]      B: lane l holds B[k = l>>4][j = l&15]
//   D: lane l, register r holds D[i = (l>>4) + 4r][j = l&15]          (probed: csrc/probes/mfma_probe.hip)
// and wave (m, nt) of a workgroup owns output tile nt of Q M-tiles (m, m + 2 when Q = 2) of every layer.
//
// The kernels keep their control flow (barriers, single or double buffered weight images, tile ping-pong, passes, the copy of the
// activations the forward may leave, stamps) and their LDS budgets; what a tile, a layer or a layer step computes is here:
//
//   pad4, lds_stride, TileGeo         sizes and strides of images and tiles, the staging split
//   prefetch_* / commit_*             a layer's weights: global -> registers, registers -> LDS image
//   load_input_tiles                  the MLP's input rows -> 16-column tiles
//   dense, activate, store_tile, load_tile, output_layer
//                                     one forward layer of Q M-tiles that share each weight fragment
//   load_rows, store_rows             a tile of g_out / g_in / s_out with its row and column guards
//   layer_part, publish, gin_product, dw_tiles, part_store, bias_sum, slope_mul
//                                     one layer step of the backward; the store kind (PartStore) and the order of the bias
//                                     reduction (TileSum) are template arguments each kernel sets
//   launch_tile_kernel                LeakyReLU / general instantiation, dynamic LDS, launch
//
// Everything a piece branches on is a template argument or a value the unrolled layer loops make a constant; none of them stamps.
#pragma once
#include "lds.hpp"
#include "ops.hpp"

namespace lgn {
namespace tile {

__host__ __device__ constexpr int pad4(int x) { return (x + 3) & ~3; }
// smallest stride >= x with stride == 2 (mod 4): 16 rows x 2 k's of a ds_read_b64 group hit 32 distinct bank pairs
__host__ __device__ constexpr int lds_stride(int x) { return x + ((6 - (x & 3)) & 3); }

// NT N-tiles (16 neurons each) of the padded hidden width, MT M-tiles (16 rows each) of waves: MT x NT waves per workgroup
template <int NT, int MT>
struct TileGeo {
  static constexpr int HP = NT * 16;                  // padded hidden width
  static constexpr int S = lds_stride(HP);            // row stride of weight image and activation tiles
  static constexpr int S0 = 18;                       // row stride of the 16-column MLP input tiles
  static constexpr int WSIZE = HP * S;                // one weight image
  static constexpr int TSIZE = 16 * S;                // one 16-row activation tile
  static constexpr int T0SIZE = 16 * S0;              // one 16-row input tile
  static constexpr int THREADS = 64 * MT * NT;
  static constexpr int NW = MT * NT;                  // waves
  static constexpr int RPP = THREADS / HP;            // rows of a hidden-layer image staged per pass (4 MT)
  static constexpr int NPH = HP / RPP;                // ... and its passes (4 NT / MT)
  static constexpr int RPF = THREADS / 16;            // rows of the first-layer image (16 columns) staged per pass (4 MT NT)
  static constexpr int NPF = HP / RPF;                // ... and its passes (4 / MT)
  static_assert(MT == 1 || MT == 2 || MT == 4, "M-tiles of waves per workgroup");
  static_assert(RPP * HP == THREADS && NPH * RPP == HP && NPF * RPF == HP && NPF <= NPH, "staging passes; prefetch registers");
};

// ---- weight staging ------------------------------------------------------------------------------
// Image of one Linear layer in LDS: W[o][k] at Wl[o*S + k] (zero padded to 16-multiples both ways; the k padding
// feeds the MFMAs zeros, padded neurons produce exact zeros) and its bias at Wl[o*S + HP] (S >= HP + 2).
// Hidden / output layers (HP input columns): thread tid stages column k = tid % HP of rows tid / HP + RPP i, so every
// address is a thread-constant base plus a compile-time (LDS) or wave-uniform (global) multiple of i.
template <class G>
__device__ __forceinline__ void prefetch_hidden(const double* __restrict__ W, const double* __restrict__ bias, int Hout, int Hin,
                                                double (&regs)[G::NPH], double& breg) {
  const int o0 = (int)threadIdx.x / G::HP, k = (int)threadIdx.x - o0 * G::HP;
  const double* src = W + (o0 * Hin + k);
#pragma unroll
  for (int i = 0; i < G::NPH; ++i) regs[i] = (k < Hin && o0 + G::RPP * i < Hout) ? src[G::RPP * i * Hin] : 0.0;
  breg = ((int)threadIdx.x < Hout) ? bias[threadIdx.x] : 0.0;
}
template <class G>
__device__ __forceinline__ void commit_hidden(double* Wl, const double (&regs)[G::NPH], double breg) {
  const int o0 = (int)threadIdx.x / G::HP, k = (int)threadIdx.x - o0 * G::HP;
  double* dst = Wl + (o0 * G::S + k);
#pragma unroll
  for (int i = 0; i < G::NPH; ++i) dst[G::RPP * i * G::S] = regs[i];
  if ((int)threadIdx.x < G::HP) Wl[threadIdx.x * G::S + G::HP] = breg;
}
// First layer (2C <= 16 input columns): thread -> column tid % 16 of rows tid / 16 + RPF i.
template <class G>
__device__ __forceinline__ void prefetch_first(const double* __restrict__ W, const double* __restrict__ bias, int Hout, int Hin,
                                               double (&regs)[G::NPH], double& breg) {
  const int o0 = (int)threadIdx.x >> 4, k = (int)threadIdx.x & 15;
#pragma unroll
  for (int i = 0; i < G::NPF; ++i) {
    const int o = o0 + G::RPF * i;
    regs[i] = (o < Hout && k < Hin) ? W[o * Hin + k] : 0.0;
  }
  breg = ((int)threadIdx.x < Hout) ? bias[threadIdx.x] : 0.0;
}
template <class G>
__device__ __forceinline__ void commit_first(double* Wl, const double (&regs)[G::NPH], double breg) {
  const int o0 = (int)threadIdx.x >> 4, k = (int)threadIdx.x & 15;
#pragma unroll
  for (int i = 0; i < G::NPF; ++i) Wl[(o0 + G::RPF * i) * G::S + k] = regs[i];      // (NPF RPF == HP: every row is one of the image's)
  if ((int)threadIdx.x < G::HP) Wl[threadIdx.x * G::S + G::HP] = breg;
}

// rows of the scalar irrep [2][M][C] from row0 on -> MTILES input tiles, feature k = 2c + z, zero padded to 16 columns
template <class G, int MTILES>
__device__ __forceinline__ void load_input_tiles(const double* __restrict__ s, int M, int C, int row0, double* X0) {
  const int D = 2 * C;
  for (int e = threadIdx.x; e < 16 * MTILES * 16; e += G::THREADS) {
    const int r = e >> 4, k = e & 15, row = row0 + r;
    X0[(r >> 4) * G::T0SIZE + (r & 15) * G::S0 + k] = (row < M && k < D) ? s[(size_t)(k & 1) * M * C + (size_t)row * C + (k >> 1)] : 0.0;
  }
}

// ---- a forward layer ---------------------------------------------------------------------------------
// acc[q] (D layout) += A_q B over 4 KS columns of A_q, every B fragment used by all Q chains, acc[0] before acc[1] within a k-step.
// xa -> A fragment base of tile 0, tile q is xq doubles further; wb -> B fragment base, k-step s is 4 s BS doubles further (BS = 1:
// the image read row-major = X W^T; BS = S: read transposed = G W).  KS compile-time k-steps, or the run-time count ks when KS == 0.
template <int Q, int BS>
__device__ __forceinline__ void mma_step(const double* xa, int xq, const double* wb, int s, v4d (&acc)[Q]) {
  const double w = wb[4 * s * BS];
#pragma unroll
  for (int q = 0; q < Q; ++q) acc[q] = __builtin_amdgcn_mfma_f64_16x16x4f64(xa[q * xq + 4 * s], w, acc[q], 0, 0, 0);
}
template <int Q, int KS, int BS>
__device__ __forceinline__ void mma_shared_b(const double* xa, int xq, const double* wb, int ks, v4d (&acc)[Q]) {
  if (KS > 0) {
#pragma unroll
    for (int s = 0; s < KS; ++s) mma_step<Q, BS>(xa, xq, wb, s, acc);
  } else {
    for (int s = 0; s < ks; ++s) mma_step<Q, BS>(xa, xq, wb, s, acc);
  }
}
// pre-activations of output tile nt of the wave's Q M-tiles m0 + 2q: bias + X W^T.  first: the 16-column MLP input tiles X0
// (four k-steps); otherwise the activation tiles X (KSH k-steps, or ksh at run time when KSH == 0).
template <class G, int Q, int KSH>
__device__ __forceinline__ void dense(bool first, const double* Wl, const double* X0, const double* X, int m0, int nt, int lane, int ksh,
                                      v4d (&acc)[Q]) {
  static_assert(Q == 1 || Q == 2, "M-tiles of a wave");
  const int c = lane & 15, g = lane >> 4;
  const double bias = Wl[(16 * nt + c) * G::S + G::HP];
#pragma unroll
  for (int q = 0; q < Q; ++q) acc[q] = v4d{bias, bias, bias, bias};
  const double* wb = Wl + (16 * nt + c) * G::S + g;
  if (first) mma_shared_b<Q, 4, 1>(X0 + m0 * G::T0SIZE + c * G::S0 + g, 2 * G::T0SIZE, wb, 4, acc);
  else mma_shared_b<Q, KSH, 1>(X + m0 * G::TSIZE + c * G::S + g, 2 * G::TSIZE, wb, ksh, acc);
}
template <bool GEN, int Q>
__device__ __forceinline__ void activate(v4d (&acc)[Q], int act) {
#pragma unroll
  for (int q = 0; q < Q; ++q)
#pragma unroll
    for (int r = 0; r < 4; ++r) acc[q][r] = act_apply_t<GEN>(acc[q][r], act);
}
// a wave's tile (D layout) <-> tile mt, columns of N-tile nt, of the tiles at T
template <class G>
__device__ __forceinline__ void store_tile(double* T, int mt, int nt, int lane, const v4d& v) {
  double* o = T + mt * G::TSIZE + (lane >> 4) * G::S + 16 * nt + (lane & 15);
#pragma unroll
  for (int r = 0; r < 4; ++r) o[4 * r * G::S] = v[r];
}
template <class G>
__device__ __forceinline__ v4d load_tile(const double* T, int mt, int nt, int lane) {
  const double* o = T + mt * G::TSIZE + (lane >> 4) * G::S + 16 * nt + (lane & 15);
  v4d v;
#pragma unroll
  for (int r = 0; r < 4; ++r) v[r] = o[4 * r * G::S];
  return v;
}

// the 16 rows from row0 on of a strided MLP operand (ops.hpp mlp_out_index), feature c = 2 ch + z in column c: one tile in D layout,
// guarded at the last row and the last feature
template <typename Args>
__device__ __forceinline__ v4d load_rows(const Args& a, const double* src, int row0, int lane) {
  const int c = lane & 15, g = lane >> 4;
  v4d v;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int row = row0 + g + 4 * r;
    v[r] = (c < 2 * a.C && row < a.M) ? src[mlp_out_index(a, c & 1, row, c >> 1)] : 0.0;
  }
  return v;
}
template <typename Args>
__device__ __forceinline__ void store_rows(const Args& a, double* dst, int row0, int lane, const v4d& v) {
  const int c = lane & 15, g = lane >> 4;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int row = row0 + g + 4 * r;
    if (c < 2 * a.C && row < a.M) dst[mlp_out_index(a, c & 1, row, c >> 1)] = v[r];
  }
}
// output layer of M-tile mt (its 16 rows start at row0): one N-tile (2C <= 16 neurons), no activation; the waves with nt == 0 call
template <class G, int KSH, typename Args>
__device__ __forceinline__ void output_layer(const Args& a, const double* Wl, const double* X, int mt, int lane, int ksh, int row0) {
  v4d acc[1];
  dense<G, 1, KSH>(false, Wl, nullptr, X, mt, 0, lane, ksh, acc);
  store_rows(a, a.s_out, row0, lane, acc[0]);
}

// ---- a layer step of the backward -----------------------------------------------------------------------
// Layer l of NH + 1 (first: l == 0, last: l == NH) has g_pre (gradient of its pre-activations) in the waves' registers and:
//   g_in  = g_pre W        A = g_pre tile,            B = W[o][k] read "transposed" from the layer's LDS image
//   dW    = g_pre^T h_in   A = g_pre tile^T, B = h_in tile, K = the rows of the pass; output tile (o-tile, k-tile) number w is computed
//                          by wave w and stored into this workgroup's partial row (reduced deterministically by reduce_partials)
//   db    = column sums of g_pre (two wave shuffles + a sum over the M-tiles through LDS)
// sizes of layer l and its block (W_l, b_l) in a partial row = concat_l (W_l, b_l), walked from the end: poff_end is where the block
// of the layer above begins
struct LayerPart {
  int Hin, Hout;
  double *pW, *pB;
};
__device__ __forceinline__ LayerPart layer_part(bool first, bool last, int D, int H, double* part, int& poff_end) {
  const int Hin = first ? D : H, Hout = last ? D : H;
  poff_end -= Hout * Hin + Hout;
  return LayerPart{Hin, Hout, part + poff_end, part + poff_end + Hout * Hin};
}
// operands of the step to LDS: the wave's g_pre tile into the tiles at Gt and (with_x) its tile of the layer input into the tiles at
// Xt; the tile's column sums (bias gradient over its 16 rows) into row `tile` of dbw
template <class G>
__device__ __forceinline__ void publish(double* Gt, double* Xt, bool with_x, double* dbw, int tile, int nt, int lane, const v4d& gpre,
                                        const v4d& hin) {
  store_tile<G>(Gt, tile, nt, lane, gpre);
  if (with_x) store_tile<G>(Xt, tile, nt, lane, hin);
  double v = (gpre[0] + gpre[1]) + (gpre[2] + gpre[3]);
  v += shfl_xor(v, 16);
  v += shfl_xor(v, 32);
  if ((lane >> 4) == 0) dbw[tile * G::HP + 16 * nt + (lane & 15)] = v;
}
// g_in tiles (m0 + 2q, nt) = g_pre W over 4 KS output neurons of the layer (ks at run time when KS == 0); zero where not live (the
// first layer has a single 16-column input tile: nt == 0)
template <class G, int Q, int KS>
__device__ __forceinline__ void gin_product(bool live, const double* Gt, const double* Wl, int m0, int nt, int lane, int ks, v4d (&gin)[Q]) {
  const int c = lane & 15, g = lane >> 4;
#pragma unroll
  for (int q = 0; q < Q; ++q) gin[q] = v4d{0, 0, 0, 0};
  if (live) mma_shared_b<Q, KS, G::S>(Gt + m0 * G::TSIZE + c * G::S + g, 2 * G::TSIZE, Wl + g * G::S + 16 * nt + c, ks, gin);
}
// dW tiles over the 16 T rows of the pass, dealt round robin to the waves; two accumulation chains: M-tiles (w, w + T/2) for w < T/2,
// with one M-tile its k-steps (s, s + 2).  The layer input is in the T tiles at Xt, for the first layer in the input tiles X0.
// An element of the partial row is written once and read once, by the reduction at the end of the step (Stream: non-temporal
// store), or a later pass of the same workgroup adds to what an earlier one wrote (Update; add: this is a later pass).
enum class PartStore { Stream, Update };
template <PartStore ST>
__device__ __forceinline__ void part_store(double v, double* dst, bool add) {
  if constexpr (ST == PartStore::Stream) __builtin_nontemporal_store(v, dst);
  else *dst = add ? *dst + v : v;
}
template <class G, int T, PartStore ST>
__device__ __forceinline__ void dw_tiles(bool first, bool last, const double* Gt, const double* Xt, const double* X0, int wave, int lane,
                                         const LayerPart& p, bool add) {
  static_assert(T == 1 || T == 2 || T == 4, "M-tiles of a pass");
  constexpr int S = G::S;
  const int c = lane & 15, g = lane >> 4;
  const int nti = first ? 1 : G::HP / 16, ntiles = (last ? 1 : G::HP / 16) * nti;
  for (int tile = wave; tile < ntiles; tile += G::NW) {
    const int t = tile / nti, u = tile - t * nti;
    const double* ga = Gt + g * S + 16 * t + c;
    const double* xb = first ? X0 + g * G::S0 + c : Xt + g * S + 16 * u + c;
    const int xts = first ? G::T0SIZE : G::TSIZE, xss = first ? G::S0 : S;
    v4d acc0 = v4d{0, 0, 0, 0}, acc1 = v4d{0, 0, 0, 0};
    if (T >= 2) {
#pragma unroll
      for (int w = 0; w < T / 2; ++w)
#pragma unroll
        for (int s = 0; s < 4; ++s) {
          acc0 = __builtin_amdgcn_mfma_f64_16x16x4f64(ga[w * G::TSIZE + 4 * s * S], xb[w * xts + 4 * s * xss], acc0, 0, 0, 0);
          acc1 = __builtin_amdgcn_mfma_f64_16x16x4f64(ga[(w + T / 2) * G::TSIZE + 4 * s * S], xb[(w + T / 2) * xts + 4 * s * xss], acc1, 0, 0, 0);
        }
    } else {
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        acc0 = __builtin_amdgcn_mfma_f64_16x16x4f64(ga[4 * s * S], xb[4 * s * xss], acc0, 0, 0, 0);
        acc1 = __builtin_amdgcn_mfma_f64_16x16x4f64(ga[4 * (s + 2) * S], xb[4 * (s + 2) * xss], acc1, 0, 0, 0);
      }
    }
    const int k = 16 * u + c;                              // D[i = o][j = k]
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int o = 16 * t + g + 4 * r;
      if (o < p.Hout && k < p.Hin) part_store<ST>(acc0[r] + acc1[r], &p.pW[o * p.Hin + k], add);
    }
  }
}
// bias gradient of neuron tid: the T M-tiles' column sums in the order its kernel has always summed them
//   Sequential   ((t0 + t1) + t2) + t3          Pairwise   (t0 + t1) + (t2 + t3), t0 + t1
enum class TileSum { Sequential, Pairwise };
template <class G, int T, TileSum FORM>
__device__ __forceinline__ double bias_sum(const double* dq, int tid) {
  if constexpr (FORM == TileSum::Sequential) {
    double v = dq[tid];
#pragma unroll
    for (int w = 1; w < T; ++w) v += dq[w * G::HP + tid];
    return v;
  } else {
    static_assert(T == 2 || T == 4, "pairs of M-tiles");
    if constexpr (T == 2) return dq[tid] + dq[G::HP + tid];
    else return (dq[tid] + dq[G::HP + tid]) + (dq[2 * G::HP + tid] + dq[3 * G::HP + tid]);
  }
}
// g_pre of the layer below: g_in times the activation's slope at that layer's output h
template <bool GEN>
__device__ __forceinline__ v4d slope_mul(const v4d& gin, const v4d& h, int act) {
  v4d gpre;
#pragma unroll
  for (int r = 0; r < 4; ++r) gpre[r] = gin[r] * act_slope_t<GEN>(h[r], act);
  return gpre;
}

// ---- launch ----------------------------------------------------------------------------------------------
// LeakyReLU, the reference default, has its own instantiation (common.hpp act_apply_t) at the reference depth; every other
// activation and depth runs the one with the activation switch: callers pass kernel<.., GEN = NH != 6> as `leaky`.
using MlpKernel = void (*)(MlpArgs<double>);
inline int launch_tile_kernel(MlpKernel leaky, MlpKernel gen, const MlpArgs<double>& a, int nblk, int threads, size_t smem,
                              hipStream_t stream) {
  return lds_launch(a.act == 0 ? leaky : gen, "cgmlp (tile)", dim3(nblk), dim3(threads), smem, stream, a);
}

}  // namespace tile
}  // namespace lgn
