// lgn-autoencoder_amd/csrc/mlp_mfma_wide.hip -- CGMLP forward / backward on the fp64 matrix cores for hidden widths
// 48 < H <= 96 (C = 5..8 at mlp_width 6; cfg5 has C = 6 -> H = 72).  Same operator and the same pieces as mlp_mfma.hip
// (mlp_tile_dev.hpp; reference: CGMLP.forward, lgn/models/lgn_levels.py:191-227); what changes is the budget:
//   * NT = 4..6 N-tiles: a weight image is 34..75 KB, so it is single buffered and a layer costs two barriers
//     (operands visible / all reads done) instead of one; the tiles need no ping-pong then either;
//   * a workgroup runs 2 M-tiles x NT N-tiles = 8..12 waves (one 16x16 output tile per wave);
//   * the backward covers its workgroup's 64 rows in ONE pass: a wave owns the tiles (mp, nt) and (mp + 2, nt) of the four
//     16-row M-tiles (two accumulation chains that share every weight fragment).  Round 2 made two 32-row passes, the second
//     adding into the partial row the first had written: 450 MB of HBM traffic per launch at cfg5 (PMC, profiles/
//     r03_pmc_cfg5.json) for 54 MB of partial rows, and every weight image staged twice.  The hidden activations of the
//     recompute stay in registers (2 tiles x 6 layers; the LDS is taken by the 4 + 4 operand tiles of the weight gradient).
#include "mlp_tile_dev.hpp"

namespace lgn {
namespace wide {

using namespace tile;

constexpr int MT = 2;

template <int NT>
struct Geo : TileGeo<NT, MT> {
  using T = TileGeo<NT, MT>;
  static constexpr size_t fwd_doubles() { return T::WSIZE + MT * T::TSIZE + MT * T::T0SIZE; }
  static constexpr int MTB = 4;                         // M-tiles of a backward workgroup (64 rows)
  //                                          image   X, G tiles       input tiles    column sums
  static constexpr size_t bwd_doubles() { return T::WSIZE + 2 * MTB * T::TSIZE + MTB * T::T0SIZE + MTB * T::HP; }
  static constexpr bool ONE_PASS = sizeof(double) * (T::WSIZE + 2 * MTB * T::TSIZE + MTB * T::T0SIZE + MTB * T::HP) <= LGN_LDS_LIMIT;
  // two-pass backward (NT = 6): the activations of the first NHL hidden layers stay in LDS tiles of their own
  static constexpr int BWD_BASE = T::WSIZE + 2 * MT * T::TSIZE + MT * T::T0SIZE + MT * T::HP;
  static constexpr int NHL_FIT = (LGN_LDS_LIMIT / 8 - BWD_BASE) / (MT * T::TSIZE);
  static constexpr int NHL = NHL_FIT > 5 ? 5 : NHL_FIT;
  static constexpr size_t bwd2p_doubles() { return BWD_BASE + NHL * MT * T::TSIZE; }
};

template <int NT, int NH, bool GEN>
__global__ __launch_bounds__(64 * MT * NT) void mlp_fwd_wide_kernel(MlpArgs<double> a) {
  using G = Geo<NT>;
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int mt = wave % MT, nt = wave / MT;
  const int D = 2 * a.C, H = a.H, M = a.M;
  const int ksh = pad4(H) >> 2;
  const int row0 = blockIdx.x * 16 * MT;
  extern __shared__ __align__(16) unsigned char smem_raw[];
  double* Wl = reinterpret_cast<double*>(smem_raw);
  double* X = Wl + G::WSIZE;
  double* X0 = X + MT * G::TSIZE;

  double regs[G::NPH], breg;
  prefetch_first<G>(a.w[0], a.b[0], H, D, regs, breg);
  load_input_tiles<G, MT>(a.s_in, M, a.C, row0, X0);
  commit_first<G>(Wl, regs, breg);
  __syncthreads();
#pragma unroll
  for (int l = 0; l < NH; ++l) {
    prefetch_hidden<G>(a.w[l + 1], a.b[l + 1], l + 1 == NH ? D : H, H, regs, breg);
    v4d acc[1];
    dense<G, 1, 0>(l == 0, Wl, X0, X, mt, nt, lane, ksh, acc);
    activate<GEN>(acc, a.act);
    __syncthreads();                                       // every read of the weight image and of the layer input is done
    store_tile<G>(X, mt, nt, lane, acc[0]);
    commit_hidden<G>(Wl, regs, breg);
    __syncthreads();
  }
  if (nt == 0) output_layer<G, 0>(a, Wl, X, mt, lane, ksh, row0 + mt * 16);
}

template <int NT, int NH, bool GEN>
__global__ __launch_bounds__(64 * MT * NT) void mlp_bwd_wide_kernel(MlpArgs<double> a) {
  using G = Geo<NT>;
  constexpr int MTB = G::MTB;
  static_assert(MT == 2 && MTB == 4, "a wave owns M-tiles mp and mp + 2");
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int mp = wave % MT, nt = wave / MT;
  const int D = 2 * a.C, H = a.H, M = a.M;
  const int ksh = pad4(H) >> 2;
  extern __shared__ __align__(16) unsigned char smem_raw[];
  double* Wl = reinterpret_cast<double*>(smem_raw);
  double* X = Wl + G::WSIZE;                               // MTB layer-input tiles
  double* Gt = X + MTB * G::TSIZE;                         // MTB g_pre tiles
  double* X0 = Gt + MTB * G::TSIZE;                        // MTB MLP input tiles
  double* dbw = X0 + MTB * G::T0SIZE;                      // MTB x HP column sums
  double* part = a.part + (size_t)blockIdx.x * a.psize;
  const int row0 = blockIdx.x * 16 * MTB;

  // ---- forward recompute; h[l][q] = post-activation of hidden layer l, tile (mp + 2 q, nt), D layout ------------------------
  double regs[G::NPH], breg;
  prefetch_first<G>(a.w[0], a.b[0], H, D, regs, breg);
  load_input_tiles<G, MTB>(a.s_in, M, a.C, row0, X0);
  commit_first<G>(Wl, regs, breg);
  __syncthreads();
  v4d h[NH][2];
#pragma unroll
  for (int l = 0; l < NH; ++l) {
    prefetch_hidden<G>(a.w[l + 1], a.b[l + 1], l + 1 == NH ? D : H, H, regs, breg);   // after the last hidden layer: the output layer
    dense<G, 2, 0>(l == 0, Wl, X0, X, mp, nt, lane, ksh, h[l]);
    activate<GEN>(h[l], a.act);
    __syncthreads();                                       // every read of the input tiles and of the weight image is done
    if (l + 1 < NH) {
      store_tile<G>(X, mp, nt, lane, h[l][0]);
      store_tile<G>(X, mp + 2, nt, lane, h[l][1]);
    }
    commit_hidden<G>(Wl, regs, breg);
    __syncthreads();
  }

  // ---- backward sweep ---------------------------------------------------------------------------------------
  v4d gpre[2] = {v4d{0, 0, 0, 0}, v4d{0, 0, 0, 0}};
  if (nt == 0) {
#pragma unroll
    for (int q = 0; q < 2; ++q) gpre[q] = load_rows(a, a.g_out, row0 + (mp + 2 * q) * 16, lane);
  }
  int poff_end = a.psize;
#pragma unroll
  for (int l = NH; l >= 0; --l) {
    const LayerPart p = layer_part(l == 0, l == NH, D, H, part, poff_end);
    if (l == 1) prefetch_first<G>(a.w[0], a.b[0], H, D, regs, breg);
    else if (l > 1) prefetch_hidden<G>(a.w[l - 1], a.b[l - 1], H, H, regs, breg);

#pragma unroll
    for (int q = 0; q < 2; ++q) publish<G>(Gt, X, l > 0, dbw, mp + 2 * q, nt, lane, gpre[q], h[l > 0 ? l - 1 : 0][q]);
    __syncthreads();

    // (a) g_in tiles (mp, nt), (mp + 2, nt) = g_pre W; K = output neurons of this layer
    v4d gin[2];
    gin_product<G, 2, 0>(l > 0 || nt == 0, Gt, Wl, mp, nt, lane, l == NH ? 4 : ksh, gin);
    // (b) dW tiles over the workgroup's 64 rows; the bias gradient
    dw_tiles<G, MTB, PartStore::Stream>(l == 0, l == NH, Gt, X, X0, wave, lane, p, false);
    if (tid < p.Hout) p.pB[tid] = bias_sum<G, MTB, TileSum::Pairwise>(dbw, tid);
    if (l > 0) {
#pragma unroll
      for (int q = 0; q < 2; ++q) gpre[q] = slope_mul<GEN>(gin[q], h[l > 0 ? l - 1 : 0][q], a.act);
      __syncthreads();                                     // every read of the weight image and of the tiles is done
      if (l == 1) commit_first<G>(Wl, regs, breg);
      else commit_hidden<G>(Wl, regs, breg);
    } else if (nt == 0) {
#pragma unroll
      for (int q = 0; q < 2; ++q) store_rows(a, a.g_in, row0 + (mp + 2 * q) * 16, lane, gin[q]);
    }
  }
}

// H > 80 (NT = 6: C = 7, 8): the 4 + 4 operand tiles of the one-pass kernel do not fit the LDS beside a 75 KB weight image.
// Round-2 kernel: two 32-row passes per workgroup, the second adding into the partial row the first one wrote; the
// activations of the first NHL hidden layers stay in LDS tiles of their own.
template <int NT, int NH, bool GEN>
__global__ __launch_bounds__(64 * MT * NT) void mlp_bwd_wide_2pass_kernel(MlpArgs<double> a) {
  using G = Geo<NT>;
  constexpr int HP = G::HP, NHL = G::NHL;
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int mt = wave % MT, nt = wave / MT;
  const int D = 2 * a.C, H = a.H, M = a.M;
  const int ksh = pad4(H) >> 2;
  extern __shared__ __align__(16) unsigned char smem_raw[];
  double* Wl = reinterpret_cast<double*>(smem_raw);
  double* X = Wl + G::WSIZE;                               // MT layer-input tiles
  double* Gt = X + MT * G::TSIZE;                          // MT g_pre tiles
  double* X0 = Gt + MT * G::TSIZE;                         // MT MLP input tiles
  double* dbw = X0 + MT * G::T0SIZE;                       // MT x HP column sums
  double* Hl = dbw + MT * HP;                              // NHL x MT tiles: post-activations of hidden layers 0 .. NHL - 1
  double* part = a.part + (size_t)blockIdx.x * a.psize;

  for (int pass = 0; pass < 64 / (16 * MT); ++pass) {      // 32-row passes of this workgroup's 64 rows
    const int row0 = blockIdx.x * 64 + pass * 16 * MT;
    if (pass) __syncthreads();
    // ---- forward recompute; h[l][0] = post-activation of hidden layer l, this wave's tile, D layout ------------------------
    double regs[G::NPH], breg;
    prefetch_first<G>(a.w[0], a.b[0], H, D, regs, breg);
    load_input_tiles<G, MT>(a.s_in, M, a.C, row0, X0);
    commit_first<G>(Wl, regs, breg);
    __syncthreads();
    v4d h[NH][1];
#pragma unroll
    for (int l = 0; l < NH; ++l) {
      prefetch_hidden<G>(a.w[l + 1], a.b[l + 1], l + 1 == NH ? D : H, H, regs, breg);   // after the last hidden layer: the output layer
      dense<G, 1, 0>(l == 0, Wl, X0, (l >= 1 && l - 1 < NHL) ? Hl + (l - 1) * MT * G::TSIZE : X, mt, nt, lane, ksh, h[l]);
      activate<GEN>(h[l], a.act);
      __syncthreads();
      if (l < NHL) store_tile<G>(Hl + l * MT * G::TSIZE, mt, nt, lane, h[l][0]);
      else if (l + 1 < NH) store_tile<G>(X, mt, nt, lane, h[l][0]);
      commit_hidden<G>(Wl, regs, breg);
      __syncthreads();
    }

    // ---- backward sweep ---------------------------------------------------------------------------------------
    v4d gpre = v4d{0, 0, 0, 0};
    if (nt == 0) gpre = load_rows(a, a.g_out, row0 + mt * 16, lane);
    int poff_end = a.psize;
#pragma unroll
    for (int l = NH; l >= 0; --l) {
      const LayerPart p = layer_part(l == 0, l == NH, D, H, part, poff_end);
      if (l == 1) prefetch_first<G>(a.w[0], a.b[0], H, D, regs, breg);
      else if (l > 1) prefetch_hidden<G>(a.w[l - 1], a.b[l - 1], H, H, regs, breg);

      const bool in_lds = l > 0 && l - 1 < NHL;            // layer input: already in its own tiles / from registers
      double* Xl = in_lds ? Hl + (l > 0 ? l - 1 : 0) * MT * G::TSIZE : X;
      publish<G>(Gt, X, l > 0 && !in_lds, dbw, mt, nt, lane, gpre, h[l > 0 ? l - 1 : 0][0]);
      __syncthreads();

      // (a) g_in tile (mt, nt) = g_pre W; K = output neurons of this layer
      v4d gin[1];
      gin_product<G, 1, 0>(l > 0 || nt == 0, Gt, Wl, mt, nt, lane, l == NH ? 4 : ksh, gin);
      // (b) dW tiles over this pass's 32 rows, one accumulation chain per M-tile; the bias gradient
      dw_tiles<G, MT, PartStore::Update>(l == 0, l == NH, Gt, Xl, X0, wave, lane, p, pass != 0);
      if (tid < p.Hout) part_store<PartStore::Update>(bias_sum<G, MT, TileSum::Pairwise>(dbw, tid), &p.pB[tid], pass != 0);
      if (l > 0) {
        // (in_lds: this wave's tile of the layer input read back in D layout)
        gpre = slope_mul<GEN>(gin[0], in_lds ? load_tile<G>(Xl, mt, nt, lane) : h[l > 0 ? l - 1 : 0][0], a.act);
        __syncthreads();                                     // every read of the weight image and of the tiles is done
        if (l == 1) commit_first<G>(Wl, regs, breg);
        else commit_hidden<G>(Wl, regs, breg);
      } else if (nt == 0) {
        store_rows(a, a.g_in, row0 + mt * 16, lane, gin[0]);
      }
    }
  }
}

template <int NT, int NH = 6>
static int launch(const MlpArgs<double>& a, bool backward, hipStream_t stream) {
  using G = Geo<NT>;
  static_assert(sizeof(double) * G::bwd2p_doubles() <= LGN_LDS_LIMIT && sizeof(double) * G::fwd_doubles() <= LGN_LDS_LIMIT, "LDS budget");
  // (mlp_depth 3 .. 5 share the instantiation with the activation switch)
  constexpr bool GEN = NH != 6;
  if (!backward)
    return launch_tile_kernel(mlp_fwd_wide_kernel<NT, NH, GEN>, mlp_fwd_wide_kernel<NT, NH, true>, a, cdiv(a.M, 16 * MT), G::THREADS,
                              sizeof(double) * G::fwd_doubles(), stream);
  if constexpr (G::ONE_PASS)
    return launch_tile_kernel(mlp_bwd_wide_kernel<NT, NH, GEN>, mlp_bwd_wide_kernel<NT, NH, true>, a, cdiv(a.M, 64), G::THREADS,
                              sizeof(double) * G::bwd_doubles(), stream);
  else
    return launch_tile_kernel(mlp_bwd_wide_2pass_kernel<NT, NH, GEN>, mlp_bwd_wide_2pass_kernel<NT, NH, true>, a, cdiv(a.M, 64), G::THREADS,
                              sizeof(double) * G::bwd2p_doubles(), stream);
}

}  // namespace wide

template <int NH>
static int wide_launch_depth(const MlpArgs<double>& a, bool backward, hipStream_t stream) {
  const int nt = (a.H + 15) / 16;
  if (nt == 4) return wide::launch<4, NH>(a, backward, stream);
  if (nt == 5) return wide::launch<5, NH>(a, backward, stream);
  return wide::launch<6, NH>(a, backward, stream);
}
// 48 < H <= 96, 2C <= 16, 4 .. 7 Linear layers (mlp_depth 3 .. 6).  Returns -2 if the shape is outside this kernel's range.
int mlp_mfma_wide_dispatch(const MlpArgs<double>& a, bool backward, hipStream_t stream) {
  if (a.nlin < 4 || a.nlin > 7 || a.H <= 48 || a.H > 96 || 2 * a.C > 16 || a.H < 2 * a.C) return -2;
  if (a.nlin == 4) return wide_launch_depth<3>(a, backward, stream);
  if (a.nlin == 5) return wide_launch_depth<4>(a, backward, stream);
  if (a.nlin == 6) return wide_launch_depth<5>(a, backward, stream);
  return wide_launch_depth<6>(a, backward, stream);
}

}  // namespace lgn
