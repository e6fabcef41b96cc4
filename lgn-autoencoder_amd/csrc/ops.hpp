// lgn-autoencoder_amd/csrc/ops.hpp -- argument blocks and host entry points shared between translation units.
#pragma once
#include <cstdlib>
#include <vector>
#include "level.hpp"

namespace lgn {

// ---- level (level_fwd.hip / level_bwd.hip) ---------------------------------------------------------
template <typename T> int level_fwd_dispatch(const LevelArgs<T>&, int decoder, hipStream_t);
// the same level forward without the aggregate stores and with the forward-only loss tail (evaluation step)
int level_fwd_eval(const LevelArgs<double>&, int decoder, hipStream_t);
template <typename T> int level_bwd_dispatch(const LevelBwdArgs<T>&, int decoder, hipStream_t);
template <typename T> int reduce_partials(const T* part, int rows, int n, T* out, int accumulate, hipStream_t);
template <typename T> int reduce_partials_strided(const T* part, int rows, int stride, int col0, int n, T* out, hipStream_t);
// one launch reducing up to RED_MAX_SEG column ranges (a whole cfg2 step has ~30):  seg.out[c] = sum_r seg.part[r*stride + col0 + c]
constexpr int RED_MAX_SEG = 64;
template <typename T> struct RedSeg { const T* part; int rows, stride, col0, n; T* out; };
template <typename T> struct RedJob {
  int nseg;
  RedSeg<T> seg[RED_MAX_SEG];
  int tile0[RED_MAX_SEG + 1];
  void add(const T* part, int rows, int stride, int col0, int n, T* out) { seg[nseg++] = RedSeg<T>{part, rows, stride, col0, n, out}; }
};
template <typename T> int reduce_segments(RedJob<T>& job, hipStream_t);
template <typename T>
int rad_finalize(const T* tot, int C, const T* ra, const T* rb, const T* rc, const T* w0, const T* w1, T* g_a, T* g_b, T* g_c,
                 T* g_w0, T* g_b0, T* g_w1, T* g_b1, hipStream_t);
// several levels in one launch (one workgroup per level)
struct RadFinJob {
  int n;
  struct Item { const double* tot; int C; const double *ra, *rb, *rc, *w0, *w1; double *g_a, *g_b, *g_c, *g_w0, *g_b0, *g_w1, *g_b1; } it[4];
};
int rad_finalize_batch(const RadFinJob& job, hipStream_t);
// the tail of a single-process training step -- deferred reductions, radial finalisation, L1 + Adam, loss assembly -- in ONE launch
// (step_tail.hip); -2 = this step does not fit the fused form, take reduce_segments + rad_finalize_batch + finalize_step
struct StepTailArgs {
  double *w, *g;
  long n;
  double *m, *v;
  long* step_dev;
  double lambda, lr, beta1, beta2, eps;
  int do_adam;
  const double* loss_part;
  int nB;
  double* loss_out;             // 3 results + LGN_FINALIZE_SCRATCH doubles (include/lgn_amd.h)
  // reduce_only: the reductions and the radial finalisation only (the data-parallel step: the gradient all-reduce follows) -- w / g / n
  // describe the gradient buffer, `counters` are 4 64-bit words that are zero before the first launch (the kernel leaves them zero)
  int reduce_only;
  unsigned long long* counters;
  // the lgn_optim_desc calls (lgn_step_train_opt_f64 / lgn_step_finalize_opt_f64): kind = LGN_OPT_*, the L2 weight, RMSprop's alpha and
  // momentum (m carries the momentum buffer, v square_avg; beta1 / beta2 are Adam's), and loss_out = 4 results +
  // LGN_FINALIZE_OPT_SCRATCH doubles.  opt_form == 0: the calls without a descriptor -- L1 + Adam on the 3-result block.
  int opt_form = 0;
  int kind = 0;
  double l2 = 0.0, alpha = 0.0, mu = 0.0;
};
int step_tail(const std::vector<RedSeg<double>>& segs, const RadFinJob& fin, const StepTailArgs& ta, hipStream_t st);
void level_bwd_partial_rows(int B, int N, int decoder, int flags, int* rows_mix, int* rows_rad);
bool level_bwd_carries_input(int N, int flags);   // the encoder's first level may take LevelBwdArgs::part_in0 (one-kernel backward, N <= 40)
bool level_dec_rebuilds(int N, int flags);        // a sequencer's decoder level keeps its jet sums, not the aggregate (LevelArgs::sep_sums)
bool level_fwd_carries_loss(int N, int flags);    // the decoder's last level may take LevelArgs::loss_* (separable one-workgroup-per-jet forward)
// does the level's CGMLP ride on the level kernel (LevelArgs::mlp / LevelBwdArgs::mlp)?  The forward and the backward decide
// independently (the forward always leaves the scalars before AND after the MLP)

// ---- CGMLP (mlp.hip / mlp_mfma.hip) ------------------------------------------------------------------
constexpr int MLP_MAX_LIN = 8;
template <typename T>
struct MlpArgs {
  int M;        // rows = B*N
  int C;        // channels; in/out features D = 2C (index 2c+z)
  int H;        // hidden width
  int nlin;     // number of Linear layers = hidden layers + 1
  const T* w[MLP_MAX_LIN];   // [out][in] row-major (nn.Linear.weight)
  const T* b[MLP_MAX_LIN];
  const T* s_in;    // [2][M][C]  scalars before the MLP
  T* s_out;         // [2][M][C]  scalars after the MLP
  // backward only
  const T* g_out;   // [2][M][C]
  T* g_in;          // [2][M][C]
  T* part;          // [nblk][psize] partial parameter gradients, layout = concat_l (W_l, b_l)
  int psize;
  // element stride of s_out / g_out / g_in (s_in is always dense): 1 = [2][M][C]; Q = the scalar column of a packed
  // feature tensor [2][M][C][Q] (pointer already offset to that column) -- the table-driven levels apply the MLP in place
  int ld = 1;
  // tbQ > 0: s_out / g_out / g_in are the scalar column of a tile-blocked tensor [tile][C][tbQ][2][64] (pointer offset to the
  // column: + q_s * 128); element (plane z, row, channel ch) at (((row >> 6) * C + ch) * tbQ) * 128 + z * 64 + (row & 63)
  int tbQ = 0;
  // optional [nlin - 1][h_rows][HP] (HP = H rounded up to 16, h_rows = M rounded up to 64; mlp_saved_doubles): the forward
  // stores the post-activation of every hidden layer here and the backward reads it back instead of recomputing the forward
  // chain (the backward is a chain of barrier-separated layer steps: six of its thirteen go away).  H <= 48 kernels only.
  T* h_saved = nullptr;
  int h_rows = 0;
  int act = 0;      // LGN_ACT_* (include/lgn_amd.h): activation after all but the last Linear
  int flags = 0;    // LVL_* (level.hpp): LVL_MLP_V1 keeps the 12-wave kernels
};
inline int mlp_saved_rows(int M) { return (M + 63) & ~63; }
inline size_t mlp_saved_doubles(int M, int H, int nlin) {
  return H <= 48 && nlin >= 4 && nlin <= 7 ? (size_t)(nlin - 1) * mlp_saved_rows(M) * ((H + 15) & ~15) : 0;
}
// The copy is 6 x M x 48 doubles per CGMLP (35 MB at 512 x 30 rows; at 64 x 30 rows, 4.4 MB, the backward drops from 24 to 17 us).
// The step always keeps it when the batch has at most this many rows -- the 16-row regime:
// (Round 6, 16-row chain kernels with the layers split over three waves: the copy pays up to the last batch size that runs them --
// 256 jets x 30 rows: 0.439 -> 0.422 ms per step, 200 jets 0.431 -> 0.408 -- so the threshold is the 16-row regime itself.)
// Beyond it the copy is the descriptor's choice (LGN_NET_MLP_KEEP, set by default; step.hip: carve_net):
// (Round 5, ONE-role 64-row kernels at 512 x 30 rows, the copy as every other 16 bytes of a 2 KB run, i.e. half of every 128-byte
// line per store, re-read two steps ahead of its use: backward 33.5 -> 27.7 us, forward 11.5 -> 19.2 us, the step 26 us slower.)
// (Two-role 64-row kernels, the copy as whole lines -- 1 KB per store of a wave: the six recompute steps were steps in which the
// four dW waves only staged images.  512 x 30 rows: backward 26.5 -> 22.4 us (H = 48) and 19.5 -> 16.3 us (H = 36), forward
// 10.5 -> 11.8 us and 7.8 -> 9.4 us, the step 0.451 -> 0.443 ms; DESIGN.md section 5.2 has the traces and the A/B.)
constexpr int MLP_SAVE_MAX_ROWS = 8128;
inline size_t mlp_save_max_rows() {          // LGN_AMD_MLP_SAVE_ROWS overrides the threshold (tuning; read once)
  static const long v = [] { const char* e = getenv("LGN_AMD_MLP_SAVE_ROWS"); return e ? atol(e) : (long)MLP_SAVE_MAX_ROWS; }();
  return (size_t)(v < 0 ? 0 : v);
}
// address of (z, row, ch) in the MLP's strided operands
template <typename T>
__host__ __device__ inline size_t mlp_out_index(const MlpArgs<T>& a, int z, int row, int ch) {
  if (a.tbQ > 0) return ((size_t)((row >> 6) * a.C + ch) * a.tbQ) * 128 + z * 64 + (row & 63);
  return ((size_t)z * a.M * a.C + (size_t)row * a.C + ch) * a.ld;
}
// parameters of a CGMLP = doubles of a partial row of its gradients, concat_l (W_l, b_l): Linear(2C -> H), nlin - 2 x Linear(H -> H), Linear(H -> 2C)
constexpr int mlp_param_count(int C, int H, int nlin) {
  return nlin == 1 ? 2 * C * 2 * C + 2 * C : (H * 2 * C + H) + (nlin - 2) * (H * H + H) + (2 * C * H + 2 * C);
}
template <typename T> int mlp_dispatch(const MlpArgs<T>&, bool backward, hipStream_t);
// standalone Clebsch-Gordan product (cg_product.hip)
int cg_product_fwd(int R, int N, int C, int D1, int D2, int DO, int mode, int nnz, const int* row_ptr, const int* col, const double* coef,
                   const double* x1, const double* x2, double* out, hipStream_t st);
int cg_product_bwd(int R, int N, int C, int D1, int D2, int DO, int mode, int nnz, const int* row_ptr, const int* col, const double* coef,
                   const double* x1, const double* x2, const double* g_out, double* g_x1, double* g_x2, hipStream_t st);
int mlp_mfma_dispatch(const MlpArgs<double>&, bool backward, hipStream_t);
int mlp_chain_dispatch(const MlpArgs<double>&, bool backward, hipStream_t);   // H = 6 * 2C <= 48, 64-row workgroups (mlp_chain.hip)
int mlp_mfma_wide_dispatch(const MlpArgs<double>&, bool backward, hipStream_t);   // 48 < H <= 96 (mlp_mfma_wide.hip)
// rows a CGMLP workgroup (= a partial row of its weight gradients) covers: 64, or 16 for H <= 48 when the batch would give
// fewer than 128 64-row workgroups (small batches: more, shorter workgroups; mlp_mfma.hip)
inline int mlp_rows_per_workgroup(int M, int H) { return (H <= 48 && (M + 63) / 64 < 128) ? 16 : 64; }
inline int mlp_partial_rows(int M, int H) { const int r = mlp_rows_per_workgroup(M, H); return (M + r - 1) / r; }

// ---- MixReps (mixreps.hip) -----------------------------------------------------------------------------
template <typename T>
struct MixArgs {
  int rows, Cin, Cout, d;
  const T* w;     // [2][Cout][Cin]
  const T* x;     // [2][rows][Cin][d]
  T* y;           // [2][rows][Cout][d]
  const T* g_y;   // backward
  T* g_x;         // [2][rows][Cin][d]  (may be null)
  T* part;        // [nblk][2*Cout*Cin]
};
template <typename T> int mix_fwd(const MixArgs<T>&, hipStream_t);
template <typename T> int mix_bwd(const MixArgs<T>&, hipStream_t);
int mix_partial_rows(int rows);

// ---- generic irreps (generic_moments.hip / generic_local.hip) -----------------------------------------------
struct GenArgs {
  int B, N, C, Q;
  const double* X;          // packed node features [2][B][N][C][Q]
  const double* p;          // encoder [B][N][4] real; decoder [2][B][N][4] complex canonical
  const uint8_t* mask;
  const double *ra, *rb, *rc, *w0, *b0, *w1, *b1;
  double* U;                // moments [B][N][C][Q][5][2]
  const double* gU;
  double* gX;               // [2][B][N][C][Q], accumulated into
  double* g_p;              // decoder, accumulated into
  double* part_rad;         // [B][rad_partial_size]
  double* gbuf;             // encoder i-centric backward, N <= 32: pair-gradient scratch, moments2_gbuf_doubles(B, N, C) doubles (optional:
                            // without it the v1 kernel of generic_moments.hip runs)
  int flags;                // LVL_* (level.hpp)
  int tb;                   // 1: X / gX are [tile][C][Q][2][64] and U / gU [tile][C][5 Q][2][64] (node n = b N + j = 64 tile + lane),
                            // the layouts of generic_local_static.hip (channel-outermost kernels of generic_moments2.hip only)
};
// element (node n, channel c, component q, plane z) of a feature tensor in either layout; Qx = components per channel
__host__ __device__ inline size_t feat_index(bool tb, size_t plane, int C, int Qx, int n, int c, int q, int z) {
  return tb ? ((size_t)((n >> 6) * C + c) * Qx + q) * 128 + z * 64 + (n & 63) : (size_t)z * plane + ((size_t)n * C + c) * Qx + q;
}
size_t moments2_gbuf_doubles(int B, int N, int C);
int moments_dispatch(const GenArgs& a, int decoder, int which, hipStream_t st);

// sparse description of (aggregate CG, power CG, concatenation) of one level, see lgn/plan.py:build_local_tables
struct LocalTables {
  int n_rows, n_out, n_w;                 // cat rows (irrep, block, m); output irreps; total complex CatMix weights
  const int *row_ptr, *t_type, *t_a, *t_b;
  const double* t_coef;
  const int *out_dim, *out_nblk, *out_row0, *out_q0, *out_w0;
  const int *u_ptr, *u_row;
  const double* u_coef;
  const int *x_ptr, *x_row, *x_other;
  const double* x_coef;
};
struct LocalArgs {
  int nodes, C, CO, Q, Qout;
  int n_terms, n_u, n_x;    // lengths of the CSR term lists (row_ptr[n_rows], u_ptr[5Q], x_ptr[Q])
  int n_units;              // forward walk units (irrep, chunk of <= 4 rows, block)
  LocalTables t;
  const double* X;          // [2][nodes][C][Q]
  const double* U;          // [nodes][C][Q][5][2]
  const double* wcat;       // concatenated CatMix weights, irrep l at t.out_w0[l]: [2][CO][nblk_l*C]
  double* out;              // [2][nodes][CO][Qout]
  const double* g_out;
  double* gU;               // [nodes][C][Q][5][2]
  double* gX;               // [2][nodes][C][Q]  (overwritten)
  double* part;             // [nblk][2*n_w]  layout per irrep like wcat (irrep l at t.out_w0[l])
  double* s_copy;           // optional [2][nodes][CO]: copy of output component q_s (the pre-MLP scalars)
  int q_s;
};
int local_fwd(const LocalArgs& a, hipStream_t st);
int local_bwd(const LocalArgs& a, hipStream_t st);
int local_partial_rows(int nodes);
// compile-time-table kernels for the two maxdim = 3 level kinds (generic_local_static.hip), node-innermost layouts
size_t local_static_packed_doubles(int kind, int C, int CO);
int local_bwd_static(int kind, int M, int C, int CO, const double* XT, const double* UT, const double* w, const int* w0, double* wp,
                     const double* goT, double* gUT, double* gXT, double* part, hipStream_t st, bool packed = false,
                     bool param_layout = false);
int local_static_unpack_grads(int kind, int C, int CO, const int* w0, const double* gpacked, double* gw, hipStream_t st);
int local_fwd_static(int kind, int M, int C, int CO, const double* XT, const double* UT, const double* w, const int* w0, double* wp,
                     double* outT, double* s_copy, int q_s, hipStream_t st, bool packed = false);
// packed = true: wp already holds the level's packed weight image.  Batched (un)packing, one launch for up to 8 levels:
// pack: dst = packed image of the CatMix weights src;  unpack: dst (CatMix parameter layout) += unpacked packed gradients src
// decoder levels with the separable moments kept on chip (generic_local_sep.hip, generic_moments_sep.hip: dec_sep_tab; round 6)
constexpr int SEP_TBL_STRIDE = 24;        // doubles per (jet, channel, component) of the jet table
int dec_sep_tab(const GenArgs& a, double* tbl, double* pc, hipStream_t st);
int local_sep_part_rows(int B);
int local_fwd_sep(int kind, int B, int N, int C, int CO, const double* XT, const double* tbl, const double* pc, const double* wp,
                  double* outT, double* s_copy, int q_s, hipStream_t st);
int local_bwd_sep(int kind, int B, int N, int C, int CO, const double* XT, const double* tbl, const double* pc, const double* b0,
                  const double* b1, const double* wp, const int* w0p, const double* goT, double* gXT, double* part, double* gpb,
                  double* part_rad, hipStream_t st);
int local_sep_gp_reduce(const double* const* gpb, const int* C, int n, int M, double* g_p, hipStream_t st);
struct StaticPackJob { int kind, C, CO; int w0[5]; const double* src; double* dst; };
int local_static_pack_batch(const StaticPackJob* jobs, int n, bool unpack, hipStream_t st);
// packed X [2][nodes][C][Q] <-> s [2][nodes][C] (component q_s) + v [2][nodes][C][4] (components q_v..q_v+3); pack zero-fills the rest
// anomaly scores and the batched assignment solver (anomaly.hip)
int anomaly_scores(const double* rec, const double* tgt, const double* rec_n, const double* tgt_n, int B, int N, int mask, double* scores,
                   int* col4row, int* status, hipStream_t st);
int linear_sum_assignment(const double* cost, int B, int n, int* col4row, int* status, hipStream_t st);
// reconstruction analysis (per-jet frames, jet features, matched relative errors) and the histogram over explicit edges (analysis.hip)
int recon_analysis(const double* target, const double* recons, int B, int N, int abs_coord, int find_match, double* part_polar,
                   double* part_polarrel, double* jet_cart, double* jet_polar, double* jet_rel_err, uint8_t* jet_keep, double* rel_err,
                   int* col4row, uint8_t* is_padded, int* status, hipStream_t st);
int match_rel_err(const double* const* frames, int B, int N, double* rel_err, int* col4row, uint8_t* is_padded, int* status,
                  hipStream_t st);
int histogram(const double* x, long long rows, int ld, int cols, const double* edges, const int* n_edges, int max_edges,
              const uint8_t* keep, const double* weights, long long* counts, double* wcounts, int max_bins, hipStream_t st);
// staging of a batch with the per-jet --normalize, and the de-normalisation of reconstruction and target (stage.hip)
int stage_batch(const double* p4, const uint8_t* labels, const double* scalars, int B, int B_pad, int N, int method, double scale,
                int jet_features, int K, double* p4_in, double* target, uint8_t* mask, double* in_scalars, double* factor,
                hipStream_t st);
int denormalize(const double* x0, const double* x1, const double* factor, int B, int N, double* out0, double* out1, hipStream_t st);
// device-resident epochs (csrc/stage.hip): staging by index at a device cursor, the bookkeeping behind a step, the state's clear
int stage_gather(const double* p4, const uint8_t* labels, const double* scalars, long long M, const int* index, long long count,
                 const long long* cursor, int B_pad, int N, int method, double scale, int jet_features, int K, double* p4_in,
                 double* target, uint8_t* mask, double* in_scalars, double* factor, int* status, hipStream_t st);
int epoch_collect(const double* loss, double* epoch, long long* cursor, long long count, int B, int n, const double* const* src,
                  double* const* dst, const int* row_doubles, hipStream_t st);
int epoch_reset(long long* cursor, double* epoch, int* status, hipStream_t st);
// the same two for a second plan behind the first (rows from `base` on) and for tensors of several planes, [planes][B][rd]
int stage_gather_at(const double* p4, const uint8_t* labels, const double* scalars, long long M, const int* index, long long count,
                    long long base, const long long* cursor, int B_pad, int N, int method, double scale, int jet_features, int K,
                    double* p4_in, double* target, uint8_t* mask, double* in_scalars, double* factor, int* status, hipStream_t st);
int epoch_collect_planes(const double* loss, double* epoch, long long* cursor, long long count, long long base, int B, int n,
                         const double* const* src, double* const* dst, const int* row_doubles, const int* planes, hipStream_t st);
int gen_pack(size_t nodes_x_C, int Q, int q_s, int q_v, const double* s, const double* v, double* X, hipStream_t st);
int gen_unpack(size_t nodes_x_C, int Q, int q_s, int q_v, const double* X, double* s, double* v, hipStream_t st);
// the same with the packed tensor tile-blocked: XT [tile][C][Q][2][64]  (M nodes; whole tiles are written, padding lanes zero)
int gen_pack_tb(int M, int C, int Q, int q_s, int q_v, const double* s, const double* v, double* XT, hipStream_t st);
int gen_unpack_tb(int M, int C, int Q, int q_s, int q_v, const double* XT, double* s, double* v, hipStream_t st);

}  // namespace lgn
