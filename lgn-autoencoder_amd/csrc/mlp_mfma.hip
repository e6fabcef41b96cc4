// lgn-autoencoder_amd/csrc/mlp_mfma.hip -- CGMLP forward / backward on the fp64 matrix cores.
//
// Same operator as csrc/mlp.hip (reference: CGMLP.forward, lgn/models/lgn_levels.py:191-227), for hidden
// widths H <= 48 (all BASELINE maxdim=2 configs: H = 6 * 2C, C <= 4).  Each Linear is a
// [rows x Hin] x [Hin x Hout] GEMM executed with v_mfma_f64_16x16x4_f64; fragment layouts, weight staging, the layer and the pieces
// of the backward's layer step are in mlp_tile_dev.hpp, shared with mlp_mfma_wide.hip.
//
// Work split: a workgroup owns 64 rows = 4 M-tiles of 16 rows and runs 4 * NT waves (NT = ceil(H/16) N-tiles);
// wave (mt, nt) owns ONE 16x16 output tile of every layer.  B*N rows give only ~one M-tile per SIMD of the
// chip, so splitting N over waves is what puts several waves on a SIMD: a layer is 12 dependent MFMAs per wave,
// and the other waves' MFMAs fill the gaps left by its LDS reads, LeakyReLU and stores.  It also keeps the
// backward's register footprint small (one tile of each hidden activation instead of NT).
//
// LDS: activations as padded [row][neuron] tiles per M-tile (row stride == 2 mod 4 scalars -> conflict-free
// ds_read_b64 of A fragments), ping-ponged between layers so that one barrier per layer suffices; layer weights
// row-major [out][in] with the same stride (bias in column HP), double buffered, the next layer's weights
// prefetched into registers while the current layer's MFMAs run.
//
// Backward (recompute; the hidden activations of the wave's own tile stay in registers in D layout): the layer step of
// mlp_tile_dev.hpp over the workgroup's 16 MT rows.
#include "mlp_tile_dev.hpp"

namespace lgn {

namespace { LGN_STAMP_DECL }
LGN_STAMP_READER(lgn_debug_stamps_mlp)

using namespace tile;

// MT = M-tiles (16 rows each) per workgroup: 4 (64 rows) in general; 1 when the batch has too few rows to give every CU a
// 64-row workgroup (mlp_rows_per_workgroup): 4x the workgroups, each with a quarter of the MFMAs per layer -- at 64 jets the
// layer time is the matrix-pipe time of ONE CU's 64 rows while 200 CUs idle.
template <int NT, int MT = 4>
struct Geo : TileGeo<NT, MT> {
  using T = TileGeo<NT, MT>;
  static constexpr size_t fwd_doubles() { return 2 * T::WSIZE + 2 * MT * T::TSIZE + MT * T::T0SIZE; }
  static constexpr size_t bwd_doubles() { return 2 * T::WSIZE + 4 * MT * T::TSIZE + MT * T::T0SIZE + 2 * MT * T::HP; }
};

template <int NT, int NH, int KSH, int MT, bool GEN>
__global__ __launch_bounds__(64 * MT * NT) void mlp_fwd_mfma_kernel(MlpArgs<double> a) {
  using G = Geo<NT, MT>;
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int mt = wave % MT, nt = wave / MT;
  const int D = 2 * a.C, H = a.H, M = a.M;
  const int ksh = pad4(H) >> 2;
  const int wg_row0 = blockIdx.x * 16 * MT;
  extern __shared__ __align__(16) unsigned char smem_raw[];
  double* Wl = reinterpret_cast<double*>(smem_raw);          // 2 weight images
  double* Xb = Wl + 2 * G::WSIZE;                            // 2 x MT activation tiles
  double* X0 = Xb + 2 * MT * G::TSIZE;                       // MT input tiles

  double regs[G::NPH], breg;
  STAMP(0);
  prefetch_first<G>(a.w[0], a.b[0], H, D, regs, breg);
  load_input_tiles<G, MT>(a.s_in, M, a.C, wg_row0, X0);
  commit_first<G>(Wl, regs, breg);
  __syncthreads();
#pragma unroll
  for (int l = 0; l < NH; ++l) {
    // hidden layers read the activation tiles of parity l & 1 and write LeakyReLU(pre) into those of parity (l + 1) & 1
    prefetch_hidden<G>(a.w[l + 1], a.b[l + 1], l + 1 == NH ? D : H, H, regs, breg);
    v4d hv[1];
    dense<G, 1, KSH>(l == 0, Wl + (l & 1) * G::WSIZE, X0, Xb + (l & 1) * MT * G::TSIZE, mt, nt, lane, ksh, hv);
    activate<GEN>(hv, a.act);
    store_tile<G>(Xb + ((l + 1) & 1) * MT * G::TSIZE, mt, nt, lane, hv[0]);
    if (a.h_saved) {                                           // kept for the backward (rows beyond M: finite values of zero inputs)
      double* hs = a.h_saved + ((size_t)l * a.h_rows + wg_row0 + mt * 16 + (lane >> 4)) * G::HP + 16 * nt + (lane & 15);
#pragma unroll
      for (int r = 0; r < 4; ++r) hs[(size_t)4 * r * G::HP] = hv[0][r];
    }
    commit_hidden<G>(Wl + ((l + 1) & 1) * G::WSIZE, regs, breg);
    __syncthreads();
  }
  if (nt == 0) output_layer<G, KSH>(a, Wl + (NH & 1) * G::WSIZE, Xb + (NH & 1) * MT * G::TSIZE, mt, lane, ksh, wg_row0 + mt * 16);
  STAMP(1);
}

template <int NT, int NH, int KSH, int MT, bool GEN>
__global__ __launch_bounds__(64 * MT * NT) void mlp_bwd_mfma_kernel(MlpArgs<double> a) {
  using G = Geo<NT, MT>;
  constexpr int HP = G::HP;
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int mt = wave % MT, nt = wave / MT;
  const int c = lane & 15, g = lane >> 4;
  const int D = 2 * a.C, H = a.H, M = a.M;
  const int ksh = pad4(H) >> 2;
  const int wg_row0 = blockIdx.x * 16 * MT;
  extern __shared__ __align__(16) unsigned char smem_raw[];
  double* Wl = reinterpret_cast<double*>(smem_raw);          // 2 weight images
  double* Xb = Wl + 2 * G::WSIZE;                            // 2 x MT layer-input tiles
  double* Gb = Xb + 2 * MT * G::TSIZE;                       // 2 x MT g_pre tiles
  double* X0 = Gb + 2 * MT * G::TSIZE;                       // MT MLP input tiles
  double* dbw = X0 + MT * G::T0SIZE;                         // 2 x MT x HP column sums
  double* part = a.part + (size_t)blockIdx.x * a.psize;

  // ---- h[l] = post-activation of hidden layer l, this wave's tile, D layout: read back from the forward's copy, or recomputed
  STAMP(2);
  double regs[G::NPH], breg;
  v4d h[NH][1];
  if (a.h_saved) {
    prefetch_hidden<G>(a.w[NH], a.b[NH], D, H, regs, breg);        // the output layer: first layer of the backward sweep
    load_input_tiles<G, MT>(a.s_in, M, a.C, wg_row0, X0);
    const double* hs = a.h_saved + ((size_t)wg_row0 + mt * 16 + g) * HP + 16 * nt + c;
#pragma unroll
    for (int l = 0; l < NH; ++l)
#pragma unroll
      for (int r = 0; r < 4; ++r) h[l][0][r] = hs[((size_t)l * a.h_rows + 4 * r) * HP];
    commit_hidden<G>(Wl + (NH & 1) * G::WSIZE, regs, breg);
    __syncthreads();
  } else {
    prefetch_first<G>(a.w[0], a.b[0], H, D, regs, breg);
    load_input_tiles<G, MT>(a.s_in, M, a.C, wg_row0, X0);
    commit_first<G>(Wl, regs, breg);
    __syncthreads();
#pragma unroll
    for (int l = 0; l < NH; ++l) {
      // the weights of the next forward layer; after the last hidden layer: the output layer (first backward layer)
      prefetch_hidden<G>(a.w[l + 1], a.b[l + 1], l + 1 == NH ? D : H, H, regs, breg);
      dense<G, 1, KSH>(l == 0, Wl + (l & 1) * G::WSIZE, X0, Xb + (l & 1) * MT * G::TSIZE, mt, nt, lane, ksh, h[l]);
      activate<GEN>(h[l], a.act);
      if (l + 1 < NH) store_tile<G>(Xb + ((l + 1) & 1) * MT * G::TSIZE, mt, nt, lane, h[l][0]);
      commit_hidden<G>(Wl + ((l + 1) & 1) * G::WSIZE, regs, breg);
      __syncthreads();
    }
  }

  // ---- backward sweep; tile buffers of parity q alternate per layer -> one barrier per layer ------------
  v4d gpre = v4d{0, 0, 0, 0};
  if (nt == 0) gpre = load_rows(a, a.g_out, wg_row0 + mt * 16, lane);
  int poff_end = a.psize;
#pragma unroll
  for (int l = NH; l >= 0; --l) {
    const int q = (NH - l) & 1;
    const LayerPart p = layer_part(l == 0, l == NH, D, H, part, poff_end);
    const double* Wcur = Wl + (l & 1) * G::WSIZE;            // image of W_l (staged by the previous iteration)
    if (l == 1) prefetch_first<G>(a.w[0], a.b[0], H, D, regs, breg);
    else if (l > 1) prefetch_hidden<G>(a.w[l - 1], a.b[l - 1], H, H, regs, breg);

    // operands of this layer to LDS: g_pre tile and layer-input tile (h[l-1]; the MLP input tiles serve l == 0)
    double* Gq = Gb + q * MT * G::TSIZE;
    double* Xq = Xb + q * MT * G::TSIZE;
    double* dq = dbw + q * MT * HP;
    publish<G>(Gq, Xq, l > 0, dq, mt, nt, lane, gpre, h[l > 0 ? l - 1 : 0][0]);
    __syncthreads();

    // (a) g_in tile (mt, nt) = g_pre W; the last layer has K = 2C <= 16 output neurons
    v4d gin[1];
    if (l == NH) gin_product<G, 1, 4>(true, Gq, Wcur, mt, nt, lane, 4, gin);
    else gin_product<G, 1, KSH>(l > 0 || nt == 0, Gq, Wcur, mt, nt, lane, ksh, gin);
    // (b) dW tiles over the workgroup's 16 MT rows (MT = 4: 9 tiles on 12 waves, one each)
    dw_tiles<G, MT, PartStore::Stream>(l == 0, l == NH, Gq, Xq, X0, wave, lane, p, false);
    if (tid < p.Hout) part_store<PartStore::Stream>(bias_sum<G, MT, TileSum::Sequential>(dq, tid), &p.pB[tid], false);
    // next layer down
    if (l > 0) {
      gpre = slope_mul<GEN>(gin[0], h[l > 0 ? l - 1 : 0][0], a.act);
      // W_{l-1} goes into the image buffer last read two layers up; every wave is past that layer's barrier
      if (l == 1) commit_first<G>(Wl, regs, breg);
      else commit_hidden<G>(Wl + ((l - 1) & 1) * G::WSIZE, regs, breg);
    } else if (nt == 0) {
      store_rows(a, a.g_in, wg_row0 + mt * 16, lane, gin[0]);
    }
  }
  STAMP(3);
}

template <int NT, int KSH, int MT, int NH>
static int launch_mlp_mfma_mt(const MlpArgs<double>& a, bool backward, hipStream_t stream) {
  using G = Geo<NT, MT>;
  const size_t smem = sizeof(double) * (backward ? G::bwd_doubles() : G::fwd_doubles());
  static_assert(sizeof(double) * G::bwd_doubles() <= LGN_LDS_LIMIT, "LDS budget");
  // (the other depths -- mlp_depth 3 .. 5, round 5 -- share the instantiation with the activation switch)
  constexpr bool GEN = NH != 6;
  return backward ? launch_tile_kernel(mlp_bwd_mfma_kernel<NT, NH, KSH, MT, GEN>, mlp_bwd_mfma_kernel<NT, NH, KSH, MT, true>, a,
                                       cdiv(a.M, 16 * MT), G::THREADS, smem, stream)
                  : launch_tile_kernel(mlp_fwd_mfma_kernel<NT, NH, KSH, MT, GEN>, mlp_fwd_mfma_kernel<NT, NH, KSH, MT, true>, a,
                                       cdiv(a.M, 16 * MT), G::THREADS, smem, stream);
}
template <int NT, int KSH, int NH = 6>
static int launch_mlp_mfma(const MlpArgs<double>& a, bool backward, hipStream_t stream) {
  // (measured again in round 4 with today's staging: 32-row forward workgroups, two per CU with independent barrier domains --
  // MT = 2, 68 KB of LDS -- take the cfg2 step from 0.568 to 0.584 ms)
  return mlp_rows_per_workgroup(a.M, a.H) == 16 ? launch_mlp_mfma_mt<NT, KSH, 1, NH>(a, backward, stream)
                                                 : launch_mlp_mfma_mt<NT, KSH, 4, NH>(a, backward, stream);
}

// the depths besides the reference default (mlp_depth 3 .. 5 = 4 .. 6 Linear layers): run-time k-loops
template <int NH>
static int launch_mlp_mfma_depth(const MlpArgs<double>& a, bool backward, hipStream_t stream) {
  const int nt = (a.H + 15) / 16;
  if (nt == 1) return launch_mlp_mfma<1, 0, NH>(a, backward, stream);
  if (nt == 2) return launch_mlp_mfma<2, 0, NH>(a, backward, stream);
  return launch_mlp_mfma<3, 0, NH>(a, backward, stream);
}

// H <= 48, 2C <= 16, 4 .. 7 Linear layers (mlp_depth 3 .. 6).  Returns -2 if the shape is outside this kernel's range.
int mlp_mfma_dispatch(const MlpArgs<double>& a, bool backward, hipStream_t stream) {
  if (a.nlin < 4 || a.nlin > 7 || a.H > 48 || 2 * a.C > 16 || a.H < 2 * a.C) return -2;
  LGN_CHECK_ARG(!a.h_saved || a.h_rows >= mlp_saved_rows(a.M), "CGMLP: the saved-activation buffer has %d rows per layer, %d rows need %d",
                a.h_rows, a.M, mlp_saved_rows(a.M));
  if (a.nlin == 4) return launch_mlp_mfma_depth<3>(a, backward, stream);
  if (a.nlin == 5) return launch_mlp_mfma_depth<4>(a, backward, stream);
  if (a.nlin == 6) return launch_mlp_mfma_depth<5>(a, backward, stream);
  const int nt = (a.H + 15) / 16;
  // fully unrolled k-loops for the widths of the reference configs (H = 6 * 2C); anything else keeps the run-time loop
  if (a.H == 48) return launch_mlp_mfma<3, 12>(a, backward, stream);
  if (a.H == 36) return launch_mlp_mfma<3, 9>(a, backward, stream);
  if (a.H == 24) return launch_mlp_mfma<2, 6>(a, backward, stream);
  if (a.H == 12) return launch_mlp_mfma<1, 3>(a, backward, stream);
  if (nt == 1) return launch_mlp_mfma<1, 0>(a, backward, stream);
  if (nt == 2) return launch_mlp_mfma<2, 0>(a, backward, stream);
  return launch_mlp_mfma<3, 0>(a, backward, stream);
}

}  // namespace lgn
