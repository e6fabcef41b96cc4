/*
 * include/lgn_amd.h -- C ABI of liblgn_amd.so, the MI355X (gfx950) implementation of the LGN
 * message-passing hot path of zichunhao/lgn-autoencoder.
 *
 * The reference has no FFI layer: the path sits behind the Python nn.Module API of
 * lgn.models.LGNEncoder / LGNDecoder (lgn/models/__init__.py:1-5).  This header is the boundary the
 * build introduces *below* that API; each entry point names the reference code it replaces.
 *
 * Conventions
 *  - All pointers are DEVICE pointers owned by the caller (PyTorch); the library never allocates,
 *    frees or retains device memory.  Tensors are contiguous in the reference's planar-complex
 *    layouts:  scalar irrep (0,0): T[2][B][N][C];  vector irrep (1,1): T[2][B][N][C][4];
 *    MixReps weight: T[2][C_out][C_in]  (lgn/g_lib/g_vec.py:30-48, g_weight.py:38-40).
 *  - `stream` is a hipStream_t (0 = default stream).  Calls only enqueue work; no host sync.
 *  - Return value: 0 success; < 0 argument/shape error detected on the host before any launch;
 *    > 0 a hipError_t from a launch.  lgn_last_error() gives the message (thread-local).
 *  - Suffix _f64: IEEE double arithmetic (the reference is fp64-only, lgn/cg_lib/cg_module.py:62-73).
 *  - Parameter-gradient reductions over the batch are deterministic: kernels write per-workgroup
 *    partial rows into caller-provided workspaces which lgn_reduce_partials_f64 sums in a fixed order.
 */
#ifndef LGN_AMD_H
#define LGN_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LGN_AMD_ABI_VERSION 19   /* bump on ANY struct or signature change (lgn/_native.py: ABI_VERSION) */

int lgn_abi_version(void);
const char* lgn_last_error(void);

/* ---- message-passing level, maxdim = 2 ------------------------------------------------------
 * Replaces, fused: RadPolyTrig.forward (lgn/nn/position_levels.py:118-209), edge = rad * zonal
 * (lgn/models/lgn_cg.py:167; zonal functions lgn/cg_lib/zonal_functions.py:123-248),
 * CGProduct aggregate + power (lgn/cg_lib/cg_ops.py:135-298; LGNNodeLevel.forward
 * lgn/models/lgn_levels.py:96-121) and CatMixReps (lgn/nn/g_nn.py:260-278).
 *
 *  decoder = 0: p = real Cartesian momenta [B][N][4], mask = node mask [B][N] (uint8);
 *               ra,rb,rc [20]; w0,w1 [2C][20]; b0,b1 [2C]   (Linear feature index 2c+z)
 *  decoder = 1: p = complex canonical momenta [2][B][N][4], mask ignored (all edges masked:
 *               lgn/models/lgn_decoder.py:335-340); only the Linear biases b0,b1 [C] are used.
 *  wm0, wm1: CatMix weights [2][CO][5C] of irreps (0,0) and (1,1); cat order [aggregate, node, power].
 *  outputs: ag0 [2][B][N][2C], ag1 [2][B][N][2C][4] (the aggregate CG product, kept for backward),
 *           s_out [2][B][N][CO], v_out [2][B][N][CO][4].
 */
int lgn_level_fwd_f64(int B, int N, int C, int CO, int decoder,
                      const double* s_in, const double* v_in, const double* p, const uint8_t* mask,
                      const double* ra, const double* rb, const double* rc,
                      const double* w0, const double* b0, const double* w1, const double* b1,
                      const double* wm0, const double* wm1,
                      double* ag0, double* ag1, double* s_out, double* v_out, void* stream);

/* Workspace sizing for lgn_level_bwd_f64: number of partial rows written for the CatMix weights
 * (row length 4*CO*5C) and for the radial network (row length lgn_level_rad_partial_len). */
int lgn_level_bwd_partial_rows(int B, int N, int decoder, int* rows_mix, int* rows_rad);
int lgn_level_rad_partial_len(int C, int decoder);
/* Workgroups per jet of the pair-sweep level kernels at this batch (jets of <= 40 particles; small batches split a jet's row groups
 * over several workgroups; 1 otherwise): what decides the partial-row counts above and which backward instantiation runs. */
int lgn_level_jet_split(int B, int N);

/* Backward of lgn_level_fwd_f64 (autograd of the same reference functions).  Edges are recomputed.
 *  in : forward inputs + ag0/ag1 + g_s_out [2][B][N][CO], g_v_out [2][B][N][CO][4]
 *  out: g_s_in [2][B][N][C], g_v_in [2][B][N][C][4] (overwritten);
 *       g_p [2][B][N][4] (decoder only; ACCUMULATED into, caller zero-initialises);
 *       g_ag scratch [B][N][20C]; part_mix [rows_mix][4*CO*5C]; part_rad [rows_rad][rad_partial_len].
 *  The caller then reduces the partial rows (lgn_reduce_partials_f64) and, for the encoder, converts
 *  the reduced radial sums into parameter gradients with lgn_radial_finalize_f64.
 */
int lgn_level_bwd_f64(int B, int N, int C, int CO, int decoder,
                      const double* s_in, const double* v_in, const double* p, const uint8_t* mask,
                      const double* ra, const double* rb, const double* rc,
                      const double* w0, const double* b0, const double* w1, const double* b1,
                      const double* wm0, const double* wm1, const double* ag0, const double* ag1,
                      const double* g_s_out, const double* g_v_out,
                      double* g_ag, double* g_s_in, double* g_v_in, double* g_p,
                      double* part_mix, double* part_rad, void* stream);

/* ---- Clebsch-Gordan product of two irreps, standalone (lgn/cg_lib/cg_ops.py:135-218: cg_product; :221-297: complex_kron_product) --
 * Per channel: out = H (x1 (x) x2), H = the stacked Clebsch-Gordan matrix [DO][D1 * D2] of the irrep pair in CSR form (device arrays
 * row_ptr [DO + 1], col [nnz] = m1 * D2 + m2, coef [nnz]).  mode 0: x1 [2][R][C][D1], x2 [2][R][C][D2].  Aggregate (sum over the
 * neighbour index before H, cg_ops.py:281-291), rows R = B * N: mode 1: x1 [2][B][N][N][C][D1] edge-like, x2 [2][B][N][C][D2];
 * mode 2: the operands the other way round.  out [2][R][C][DO].  Backward: g_x1 / g_x2 are ACCUMULATED into (zero-filled by the
 * caller); either may be NULL (that operand is data: its gradient is not computed).  What lgn.cg_lib.cg_product / CGProduct bind, one call per pair of irreps; inside the networks the product is fused into
 * the level kernels and never materialised. */
int lgn_cg_product_fwd_f64(int R, int N, int C, int D1, int D2, int DO, int mode, int nnz, const int* row_ptr, const int* col,
                           const double* coef, const double* x1, const double* x2, double* out, void* stream);
int lgn_cg_product_bwd_f64(int R, int N, int C, int D1, int D2, int DO, int mode, int nnz, const int* row_ptr, const int* col,
                           const double* coef, const double* x1, const double* x2, const double* g_out, double* g_x1, double* g_x2,
                           void* stream);

/* out[n] = (accumulate ? out[n] : 0) + sum_r part[r][n], fixed summation order. */
int lgn_reduce_partials_f64(const double* part, int rows, int n, double* out, int accumulate, void* stream);

/* Encoder radial network: reduced pair sums (T1|T2|S|dB, see csrc/level_bwd.hip) -> gradients of
 * RadPolyTrig's a, b, c [20], linear.{0,1}.weight [2C][20] and .bias [2C]
 * (parameters of lgn/nn/position_levels.py:67-97). */
int lgn_radial_finalize_f64(const double* tot, int C, const double* ra, const double* rb, const double* rc,
                            const double* w0, const double* w1,
                            double* g_a, double* g_b, double* g_c,
                            double* g_w0, double* g_b0, double* g_w1, double* g_b1, void* stream);

/* ---- CGMLP (lgn/models/lgn_levels.py:191-227) ------------------------------------------------
 * rows M = B*N, features 2C (index 2c+z) taken from / written to the scalar irrep [2][M][C];
 * nlin Linear layers (nn.Linear weight [out][in], bias [out]) of hidden width H, the activation
 * (LGN_ACT_*: get_activation_fn, lgn/nn/generic_levels.py:119-135) after all but the last.
 * w / b: host arrays of nlin device pointers. */
#define LGN_ACT_LEAKYRELU 0   /* nn.LeakyReLU() (slope 0.01): the reference default */
#define LGN_ACT_RELU 1
#define LGN_ACT_ELU 2         /* alpha = 1 */
#define LGN_ACT_SIGMOID 3
#define LGN_ACT_LOGSIGMOID 4
#define LGN_ACT_ATAN 5
#define LGN_ACT_COUNT 6
int lgn_cgmlp_fwd_f64(int M, int C, int H, int nlin, int activation, const double* const* w, const double* const* b,
                      const double* s_in, double* s_out, void* stream);
/* rows of the partial weight-gradient buffer for M rows at hidden width H: one per workgroup of the backward (64 rows; 16 rows
 * for H <= 48 when M is small enough that 64-row workgroups would leave most CUs idle). */
int lgn_cgmlp_partial_rows(int M, int H);
/* part [lgn_cgmlp_partial_rows(M, H)][psize], psize = sum_l (out_l*in_l + out_l), layout concat_l (W_l, b_l). */
int lgn_cgmlp_bwd_f64(int M, int C, int H, int nlin, int activation, const double* const* w, const double* const* b,
                      const double* s_in, const double* g_out, double* g_in, double* part, int psize, void* stream);

/* ---- MixReps (lgn/nn/g_nn.py:95-117, lgn/g_lib/cplx_lib.py:7-25) -------------------------------
 * y[z][row][o][m] = sum_i W[o][i] x[row][i][m]   complex, d = irrep dimension. */
int lgn_mixreps_fwd_f64(int rows, int Cin, int Cout, int d, const double* w, const double* x, double* y, void* stream);
int lgn_mixreps_partial_rows(int rows);
/* g_x may be NULL (input is data).  part [rows][2*Cout*Cin]. */
int lgn_mixreps_bwd_f64(int rows, int Cin, int Cout, int d, const double* w, const double* x, const double* g_y,
                        double* g_x, double* part, void* stream);

/* ---- arbitrary irreps (maxdim = 3): table-driven level --------------------------------------------------
 * Same operator as lgn_level_fwd/bwd for node features carrying any set of irreps with k, n < maxdim, packed as
 * X [2][B][N][C][Q] (Q = sum of irrep dimensions, irreps in the level's GVec order).  Split in two stages:
 *  (1) "moments" (O(N^2), no CG tables):  U[b][i][c][q][0] = sum_j X_j[c][q] e0_ij[c],  U[..][1+m] = sum_j X_j[c][q] e1_ij[c][m]
 *      -- the neighbour sum of the Kronecker products of lgn/cg_lib/cg_ops.py:281-297 before the CG matrix is applied;
 *  (2) per node: sparse CG contraction of U (aggregate) and of X (x) X (power), concatenation with X, CatMix
 *      (cg_ops.py:195-215, lgn/nn/g_nn.py:160-190,260-278), driven by the CSR tables of lgn_local_tables.
 * U / gU layout: [B][N][C][Q][5][2] (re, im innermost).  Radial parameters as for lgn_level_fwd_f64. */
int lgn_moments_fwd_f64(int B, int N, int C, int Q, int decoder, const double* X, const double* p, const uint8_t* mask,
                        const double* ra, const double* rb, const double* rc, const double* w0, const double* b0,
                        const double* w1, const double* b1, double* U, void* stream);
/* gX [2][B][N][C][Q] and g_p (decoder) are ACCUMULATED into; part_rad [B][lgn_level_rad_partial_len(C, decoder)];
 * scratch: lgn_moments_scratch_doubles(B, N, C, decoder) doubles (0 = none needed, NULL allowed: jets of up to 32 particles
 * run channel-outermost kernels whose encoder radial backward parks the per-pair gradients there). */
long long lgn_moments_scratch_doubles(int B, int N, int C, int decoder);
int lgn_moments_bwd_f64(int B, int N, int C, int Q, int decoder, const double* X, const double* p, const uint8_t* mask,
                        const double* ra, const double* rb, const double* rc, const double* w0, const double* b0,
                        const double* w1, const double* b1, const double* gU, double* gX, double* g_p,
                        double* part_rad, double* scratch, void* stream);

typedef struct lgn_local_tables {
  int n_rows, n_out, n_w;          /* concatenated rows (irrep, block, m); output irreps; complex CatMix weights */
  int n_terms, n_u, n_x;           /* lengths of the three CSR term lists (= row_ptr[n_rows], u_ptr[5 Q], x_ptr[Q]); the backward keeps
                                      the U list in LDS and the host sizes it from n_u */
  int n_units, static_kind;        /* n_units: reserved (0).  static_kind: 1 / 2 when these tables are exactly the ones compiled into
                                      the library for the first / later levels of maxdim = 3 networks (csrc/cg_static_tables.hpp,
                                      lgn/plan.py: static_kind), else 0: whole-network calls then run the compile-time-table kernels */
  const int *row_ptr, *t_type, *t_a, *t_b;      /* CSR terms per row: type (t_type & 3) 0: U[a = q*5+k], 1: X[a], 2: X[a]*X[b];
                                                   t_type & 4 marks the last term of a row (every row has >= 1 term) */
  const double* t_coef;
  const int *out_dim, *out_nblk, *out_row0, *out_q0, *out_w0;   /* per output irrep */
  const int *u_ptr, *u_row;                     /* transposed lists for the backward */
  const double* u_coef;
  const int *x_ptr, *x_row, *x_other;
  const double* x_coef;
  int h_out_w0[8];                 /* host copy of out_w0 (first n_out entries): the compile-time-table kernels take the offsets by value */
} lgn_local_tables;

/* X [2][nodes][C][Q], U [nodes][C][Q][5][2], wcat = CatMix weights of all irreps ([2][CO][nblk*C] each, at out_w0),
 * out [2][nodes][CO][Qout]. */
int lgn_local_fwd_f64(int nodes, int C, int CO, int Q, int Qout, const lgn_local_tables* t, const double* X, const double* U,
                      const double* wcat, double* out, void* stream);
int lgn_local_partial_rows(int nodes);
/* gU, gX overwritten; part [lgn_local_partial_rows][2*n_w] (layout like wcat). */
int lgn_local_bwd_f64(int nodes, int C, int CO, int Q, int Qout, const lgn_local_tables* t, const double* X, const double* U,
                      const double* wcat, const double* g_out, double* gU, double* gX, double* part, void* stream);

/* The two level kinds of maxdim = 3 networks (kind 1: first level, node irreps (1,1), (0,0); kind 2: later levels, all five
 * irreps) have their tables compiled in (csrc/cg_static_tables.hpp): same operator as lgn_local_fwd_f64 on tile-blocked,
 * node-innermost layouts (node n = 64 tile + lane; buffers cover ceil(nodes / 64) whole tiles):
 *   XT [tile][C][Q][2][64], UT [tile][C][5 Q][2][64], outT [tile][CO][Qout][2][64];
 * w0[5] = offset of each output irrep's weights in wcat (host array); wpacked: scratch of
 * lgn_local_static_packed_doubles(kind, C, CO) doubles (the call repacks the weights into it);
 * s_copy optional [2][nodes][CO] copy of output component q_s (dense). */
long long lgn_local_static_packed_doubles(int kind, int C, int CO);
/* Backward of lgn_local_fwd_static_f64: goT [tile][CO][Qout][2][64] -> gUT [tile][C][5 Q][2][64], gXT [tile][C][Q][2][64]
 * (both overwritten) and g_wcat += CatMix weight gradient (wcat layout; caller zero-initialises).  Scratch: wpacked and
 * gpacked (lgn_local_static_packed_doubles doubles each), part (ceil(nodes / 64) rows of that length). */
int lgn_local_bwd_static_f64(int kind, int nodes, int C, int CO, const double* XT, const double* UT, const double* wcat,
                             const int* w0, double* wpacked, const double* goT, double* gUT, double* gXT, double* part,
                             double* gpacked, double* g_wcat, void* stream);
int lgn_local_fwd_static_f64(int kind, int nodes, int C, int CO, const double* XT, const double* UT, const double* wcat,
                             const int* w0, double* wpacked, double* outT, double* s_copy, int q_s, void* stream);

/* ---- whole training step (utils/train.py:283-343 inner loop); fused maxdim = 2 or table-driven networks -------
 * One call enqueues encoder -> decoder -> get_real(., d->get_real) -> Chamfer [+ jet-feature MSE, d->jet_loss_scale]
 * -> full backward (~80 launches, no host
 * sync, all buffers caller-owned and static => capturable in a HIP graph).  Parameters of both networks
 * live in ONE flat buffer `params`; gradients are written into `grads` at the same offsets (the call zero-
 * fills `grads` first; parameters that cannot receive gradient keep an exact 0).
 * Offsets (in elements) are given per slot, in this order (L = n_levels, nlin = mlp_nlin):
 *   encoder: input_func_node (0,0),(1,1) | per level: a,b,c,linear.0.weight,.bias,linear.1.weight,.bias |
 *            per level: cat_mix (0,0),(1,1) | per level: linear.0.weight,.bias ... linear.{nlin-1} | mix_reps (0,0),(1,1)
 *   decoder: latent_to_graph (0,0),(1,1) | input_func_node (0,0),(1,1) | radial | cat_mix | mlp | mix_to_output (0,0),(1,1)
 * Pooling is 'min&max' (lgn/models/lgn_encoder.py:419-583); the decoder consumes 2*tau_v latent vectors.
 */
typedef struct lgn_net_desc {
  int B, N;
  int n_levels;            /* message-passing levels per network (<= 4) */
  int enc_channels[5];     /* n_levels + 1 entries */
  int dec_channels[5];
  int tau_s, tau_v;        /* encoder latent multiplicities before the min&max concatenation */
  int mlp_hidden_mul;      /* CGMLP hidden width = mlp_hidden_mul * 2C  (reference: mlp_width) */
  int mlp_nlin;            /* Linear layers per CGMLP (mlp_depth + 1) */
  int tau_v_in;            /* decoder: latent vectors it consumes; 0 = 2 * tau_v (the 'min&max' concatenation) */
  /* Table-driven networks (any level with maxdim = 3): set enc_tables[l] / dec_tables[l] for EVERY level of that network
   * (host structs holding device pointers, as for lgn_local_fwd_f64; all NULL = the fused maxdim = 2 kernels).  The level
   * features are then the packed tensors X_l [2][B][N][C_l][Q_l] of lgn_moments_fwd_f64 / lgn_local_fwd_f64 with
   * Q_l = *_Q[l] components per channel, the scalar irrep (0,0) at component *_qs[l] and the vector irrep (1,1) at
   * components *_qv[l] .. +3 (l = 0 .. n_levels).  The CatMix parameter slot (.., 0) of level l is the lowest offset of the
   * level's CatMix weights in the flat block; tables[l]->out_w0 are offsets from there (slot (.., 1) is ignored). */
  const lgn_local_tables* enc_tables[4];
  const lgn_local_tables* dec_tables[4];
  int enc_Q[5], enc_qs[5], enc_qv[5];
  int dec_Q[5], dec_qs[5], dec_qv[5];
  /* LGN_NET_* bits.  Switches that change the LAYOUT of buffers living across calls (the activations a forward leaves for
   * its backward) are part of the descriptor, fixed when the caller creates it -- not read from the environment per call, so
   * a forward and its backward can never disagree. */
  int flags;
  int activation;          /* LGN_ACT_* of every CGMLP of both networks (the reference builds them from one --activation) */
  int n_in_scalars;        /* encoder: input scalars per node, K (0 or 1: the mass alone).  K > 1 -- jet_features and / or
                              data['scalars'], lgn/models/lgn_encoder.py:372-411: the mass, then K - 1 values per node the caller
                              passes as in_scalars [B][N][K - 1] -- to the per-network calls and (ABI 17) the whole-step calls, on
                              maxdim = 2 and table-driven networks alike; K <= 8 */
  int latent_pool;         /* encoder: how the latent channels are pooled over the particles (aggregate(), lgn/models/
                              lgn_encoder.py:419-496): 0 = 'min&max' (the reference default), else LGN_POOL(...).  With P output
                              blocks (one per pooling under '&', one in all under '+') the latent space is lat_s [2][B][P tau_s],
                              lat_v [2][B][P tau_v][4], and the decoder of a whole step takes Tin = P tau_v vectors */
  int dec_N;               /* whole-step call only: particles the decoder reconstructs when that differs from the encoder's node count N
                              (jet_features: the encoder works on N = particles + 1 nodes, lgn_encoder.py:372-411); 0 = N.  With
                              dec_N != N or n_in_scalars > 1 the step runs its four end stages as launches of their own, each on
                              its network's node count -- maxdim = 2 and table-driven networks alike (both kinds take dec_N and
                              n_in_scalars; a table-driven network's layout and kernels are chosen per network on that network's
                              node count).  Checked at plan time: >= 0, and the decoder's end stages at dec_N particles fit
                              LGN_LDS_LIMIT */
  /* Loss options of the whole-step call (ABI 18; a zero-initialised descriptor is the 'sum' / no-jet-term step of ABI 17): */
  int get_real;            /* LGN_REAL_*: how the real reconstruction x is taken from the two planes (utils/utils.py:194-207) */
  double jet_loss_scale;   /* >= 0; adds jet_loss_scale * sum_mu (sum_i x_i - sum_j t_j)_mu^2 per jet, sums over all N rows, padding
                              included (--chamfer-jet-features: nn.MSELoss over (B, 4) is 1 / (4 B) with B the global batch); 0 = off */
} lgn_net_desc;
#define LGN_REAL_SUM 0        /* re + im */
#define LGN_REAL_REAL 1       /* re (the reference's default --get-real-method) */
#define LGN_REAL_IMAG 2       /* im */
#define LGN_REAL_MEAN 3       /* (re + im) / 2 */
#define LGN_REAL_NORM 4       /* sqrt(re^2 + im^2 + 1e-16) */
/* The loss of the whole-step calls (--loss-choice, utils/train.py:416-480: get_loss): their `loss` argument.  NULL or kind ==
 * LGN_LOSS_CHAMFER: Chamfer [+ the jet-feature term of d->jet_loss_scale] inside the decoder's last kernel; assignment and status are
 * then not touched.  Otherwise, with x = get_real(reconstruction) and t = target:
 *   LGN_LOSS_MSE        nn.MSELoss()(x, t) (utils/train.py:460-462): the identity assignment on the (E, px, py, pz) columns;
 *   LGN_LOSS_HUNGARIAN  HungarianMSELoss (utils/losses/hungarian_mse/hungarian_mse.py:46-84 and utils.py next to it) in the frame
 *                       abs_coord / polar_coord select (main.py:324-334: --hungarian-abs-coord True, --hungarian-polar-coord False):
 *       abs Cartesian (E, px, py, pz), D = 4;  abs polar (pt, eta, phi) of get_p_polar, D = 3;  relative polar (pt / Jpt, eta - Jeta,
 *       phi - Jphi) with J the polar form of the TARGET's summed momenta for both sides;  relative Cartesian (pt cos phi, pt cos phi,
 *       pt sinh eta) of the relative polar frame, as get_p_cartesian has it.
 *     col = scipy.optimize.linear_sum_assignment of the Euclidean distances |p_i - q_j| (ties as scipy breaks them; no gradient
 *     through it), solved by one wavefront per jet on the device instead of the reference's copy to the host and Python loop.
 *   loss_part[b] = scale * sum_r sum_c (p[col[r]][c] - q[r][c])^2 -- the reference pairs p[col[r]] with q[r] -- and the gradient
 *   goes through the frame, get_real and the output mix like the Chamfer gradient.  scale = 1 / (global batch * N * D): the mean of
 *   nn.MSELoss.  Nothing is masked.  d->jet_loss_scale must be 0 (--chamfer-jet-features is a Chamfer option).  The loss stage is a
 *   launch of its own (csrc/assign_loss.hip); 1 <= Nd <= LGN_ANOMALY_NMAX and its LDS must fit LGN_LDS_LIMIT: refused before any launch.
 *   assignment [B][Nd] int32 (nullable): col; status [B] int32 (nullable): 1 -- a cost is NaN or -inf, 256 -- infeasible matrix;
 *   loss_part[b] is then NaN, its assignment row is -1, and the stage hands on exact zeros for the jet (d loss / d x, the gradient
 *   into the last level's vectors and its dWo1 partial row); where the jet's activations themselves are NaN, the level backwards
 *   after the stage still turn 0 * NaN into NaN parameter gradients.
 *   LGN_LOSS_EMD        the energy mover's distance of (x, t) on their relative-polar frames (lgn/losses.py: EMDLoss, HybridLoss): the
 *                       `loss` argument then points at the first member of an lgn_emd_loss_desc, which is defined with the EMD
 *                       calls below, where its stage is described.
 * Workspace sizes do not depend on the loss. */
#define LGN_LOSS_CHAMFER 0
#define LGN_LOSS_MSE 1
#define LGN_LOSS_HUNGARIAN 2
#define LGN_LOSS_EMD 3
typedef struct lgn_loss_desc {
  int kind;                /* LGN_LOSS_* */
  int abs_coord;           /* Hungarian: --hungarian-abs-coord */
  int polar_coord;         /* Hungarian: --hungarian-polar-coord */
  double scale;            /* 1 / (global batch * N * D), D = 4 (MSE, abs Cartesian) or 3 */
} lgn_loss_desc;
/* latent pooling code: n = 1..4 poolings o0..o3 (LGN_POOL_MIN / MAX / MEAN), avg = 0: concatenated ('a&b'), 1: averaged ('a+b').
 * min / max pick ONE particle per (plane, channel) -- by the value itself (min) / its square (max) for scalars, by the Minkowski
 * square of the Cartesian vector for vectors (get_min_features / get_max_features, lgn_encoder.py:538-583); mean = torch.mean over
 * the particle axis, padded particles included.  ('sum' returns an extra axis in the reference: per-operator path only.) */
#define LGN_POOL_MIN 0
#define LGN_POOL_MAX 1
#define LGN_POOL_MEAN 2
#define LGN_POOL_MIX 3        /* only as LGN_POOL(1, 0, LGN_POOL_MIX, 0, 0, 0): map_to_latent = 'mix' -- no pooling, the latent MixReps
                                 weights (encoder output slots) are [2][tau][N C] and act on all (particle, channel) pairs of a jet
                                 (lgn_encoder.py:226-232,313-319); one output block */
#define LGN_POOL(n, avg, o0, o1, o2, o3) ((n) | ((avg) << 3) | ((o0) << 4) | ((o1) << 6) | ((o2) << 8) | ((o3) << 10))
#define LGN_NET_NO_STATIC 1   /* table-driven levels: run-time-table kernels + node-major features (cross-check of the
                                 compile-time-table kernels; lgn/_native.py sets it from LGN_AMD_NO_STATIC at creation) */
/* kernel-selecting cross-check switches, frozen the same way (lgn/_native.py: net_flags; the partial-row counts, whether the loss
 * rides on the last decoder level all follow from them -- a forward, its backward
 * and the workspace sizing can never disagree): */
#define LGN_NET_DEC_PAIRWISE 2   /* LGN_AMD_DEC_PAIRWISE=1: decoder levels as O(N^2) pair sweeps instead of the separable form */
#define LGN_NET_LEVEL_V2 4       /* LGN_AMD_LEVEL_V2=1: three-kernel level backward also for N <= 40 */
#define LGN_NET_MLP_V1 8         /* LGN_AMD_MLP_V1=1: the CGMLP keeps the 12-wave kernels (csrc/mlp_mfma.hip) where the chain kernels
                                    (csrc/mlp_chain.hip: large batches, H = 6 x 2C <= 48) would run; cross-check */
/* (bit 32, and bit 8 before ABI 14: round 4's CGMLP-inside-the-level-kernels switches; measured slower in every regime, removed) */
#define LGN_NET_MOMENTS_V1 16    /* LGN_AMD_MOMENTS_V1=1: component-chunked moments kernels (with LGN_NET_NO_STATIC) */
#define LGN_NET_BWD_ORDERED 64   /* LGN_AMD_BWD_ORDERED=1: the encoder level backward runs its radial-gradient GEMM per ordered pair tile
                                    (the form before round 4's symmetric sweep; cross-check) */
#define LGN_NET_DEC_UNFUSED 256  /* LGN_AMD_DEC_UNFUSED=1: table-driven decoder levels as moments tensor + per-node kernels (the round-5
                                    sequence) instead of the fused separable form of csrc/generic_local_sep.hip; cross-check.  Changes
                                    the activation / scratch layouts: fixed in the descriptor like the others */
#define LGN_NET_MOMENTS_SPLIT 512 /* LGN_AMD_MOMENTS_SPLIT=1: the encoder's table-driven level backward runs its two pair sweeps as two
                                    kernels (moments_bwd_nodes2 + moments_bwd_G2: the round-5 form) instead of the merged one; cross-check */
#define LGN_NET_MLP_BWD1 1024    /* LGN_AMD_MLP_BWD1=1: the chain CGMLP backward as ONE role per wave (four waves per workgroup: chain, weight
                                    gradients and image staging on the same wave -- the round-5 kernel) instead of the two-role kernel
                                    (eight waves: four carry the chain, four the weight gradients and the staging); below 8 129 rows: one chain
                                    wave per 16-row workgroup instead of a layer split over three; cross-check */
#define LGN_NET_MLP_FULLTILE 2048 /* LGN_AMD_MLP_FULLTILE=1: the chain CGMLP kernels on 64-row workgroups compute the padded last tile of a hidden
                                    layer (H = 36: neurons 32 .. 47, four of them real) as a full 16 x 16 x 4 tile, as before the four-neuron
                                    block instructions (csrc/mlp_chain.hip: Items); cross-check */
#define LGN_NET_LIVE_SCALARS 4096 /* LGN_AMD_LIVE_SCALARS=1: the last level of either network, whose scalar output nobody reads and whose scalars carry
                                    no gradient, runs the level kernels with live scalars -- on the zero block, as before those kernels had a
                                    form without them; cross-check (bit-identical) */
#define LGN_NET_MLP_KEEP 8192    /* not a cross-check but a workspace request, SET by default (lgn/_native.py: net_flags; LGN_AMD_MLP_RECOMPUTE=1
                                    clears it): the training step and the per-network calls keep the six hidden activations of a CGMLP
                                    of H <= 48 for its backward also beyond 8 128 rows, where the 64-row two-role kernels of
                                    csrc/mlp_chain.hip then store and re-read them instead of recomputing them at the head of the backward --
                                    6 x rows (rounded up to 64) x 48 doubles per CGMLP with a backward, 141.6 MB at 512 jets of 30 particles.
                                    Without the bit the workspace is the one of before (tests/golden/workspace_doubles.json) and those batches
                                    recompute; bit-identical results either way.  The evaluation step keeps nothing.  A new bit of `flags`
                                    changes no struct or signature: LGN_AMD_ABI_VERSION stays 19 */
#define LGN_NET_SPLIT_TAIL 128  /* LGN_AMD_SPLIT_TAIL=1: the tail of a step (deferred reductions, radial finalisation, L1 + Adam) as the
                                    three separate launches instead of csrc/step_tail.hip's one (cross-check; bit-identical) */

/* Plan-time fit queries: bytes of LDS the largest per-jet end stage needs (one workgroup per jet; the limit is LGN_LDS_LIMIT).
 * encoder: input-stage backward (K input scalars, C0 = first channel count) and the latent stage (CL = last channel count,
 * Ts / Tv latent multiplicities, pool = LGN_POOL code); decoder: its input stage (Tin latent vectors) and output / loss stage;
 * junction: the fused encoder-latent + decoder-input kernels of the whole-step call.  -1: bad pooling code.  A caller whose
 * shape does not fit takes the per-operator path instead (_fused_ok of lgn/models/encoder.py and decoder.py, NativeTrainStep of lgn/step.py). */
#define LGN_LDS_LIMIT (160 * 1024)
long long lgn_encoder_end_lds_bytes(int N, int C0, int K, int CL, int Ts, int Tv, int pool);
long long lgn_decoder_end_lds_bytes(int N, int C0, int Tin, int CL);
long long lgn_junction_lds_bytes(int N, int CL, int Ts, int Tv, int pool, int C0);

int lgn_step_param_slots(const lgn_net_desc* d, int decoder);
long long lgn_step_workspace_doubles(const lgn_net_desc* d);
/* p4 [B][N][4] real Cartesian encoder input (already multiplied by the encoder's `scale`, lgn_encoder.py:376; with jet_features its
 * last node is the jet); target [B][Nd][4] the UNscaled batch the reconstruction is compared with (utils/train.py:285-292; may alias
 * p4 when scale == 1 and Nd == N), Nd = d->dec_N or N; mask [B][N]; in_scalars [B][N][K - 1] or NULL (d->n_in_scalars <= 1);
 * recon [2][B][Nd][4]; loss_part [B].  workspace_doubles = capacity of `workspace`: the call
 * fails before enqueuing anything if the current configuration needs more (lgn_step_workspace_doubles).
 * loss, assignment [B][Nd], status [B]: the lgn_loss_desc above and what its stage writes; all three NULL = Chamfer.
 * (ABI 16: the side_stream argument of the forked gradient reductions is gone with that path -- measured slower in every regime.)
 * (ABI 19: the three whole-step calls take (loss, assignment, status) themselves; their *_loss_f64 twins are gone.) */
int lgn_step_fwd_bwd_f64(const lgn_net_desc* d, const double* params, double* grads, long long n_params,
                         const int64_t* enc_off, const int64_t* dec_off, const double* p4, const double* target,
                         const uint8_t* mask, const double* in_scalars, double* workspace, long long workspace_doubles,
                         double* recon, double* loss_part, const lgn_loss_desc* loss, int* assignment /* nullable */,
                         int* status /* nullable */, void* stream);
/* grads += l1_lambda*sign(params) (utils/train.py:484-487); loss_out[0..2] = total, chamfer, sum|w|; optional Adam
 * (torch.optim.Adam defaults; the step counter lives on the device so that graph replays stay correct).
 * loss_out must hold 3 + LGN_FINALIZE_SCRATCH doubles: the results, then scratch -- the per-workgroup |w| partials, the cached
 * bias-correction powers {t, beta1^t, beta2^t} of the next odd / even step (checked against the step counter before use: a
 * restored counter or changed betas just recompute them) and, in the last slot, the finished-workgroup counter of the single
 * launch.  The caller zero-fills the block ONCE, at allocation; every kernel that uses it (this call's, lgn_step_train_f64's fused
 * tail) leaves the counters AND the |w| partial slots at zero -- the fused tail reads "zero = not yet written in this launch", so
 * the two calls may be mixed on one block.  A launch that died
 * part-way (device fault) leaves it dirty: zero the block again before reusing it -- with a non-zero counter no workgroup
 * recognises itself as the last one, loss_out[0..2] stay stale and the step counter is not advanced. */
#define LGN_FINALIZE_SCRATCH 2048
int lgn_step_finalize_f64(double* params, double* grads, long long n_params, const double* loss_part, int n_loss,
                          double l1_lambda, double* adam_m, double* adam_v, long long* step_dev,
                          double lr, double beta1, double beta2, double eps, int do_adam, double* loss_out, void* stream);
/* The whole training step of ONE process in one call: lgn_step_fwd_bwd_f64 followed by lgn_step_finalize_f64 (same arguments, same
 * results: gradients incl. the L1 sub-gradient in `grads`, loss terms in loss_out[0..2], Adam applied when do_adam).  With nothing
 * to do between the gradients and the optimiser (no all-reduce) the tail of the step -- the deferred reductions of all partial
 * rows, the radial-gradient finalisation, L1 + Adam, the loss assembly: three dependent launches above -- is ONE launch
 * (csrc/step_tail.hip; bit-identical results; LGN_NET_SPLIT_TAIL in d->flags keeps the three launches).  The table-driven (maxdim 3) step
 * and steps that do not fit the fused form take the three launches by themselves.  loss_out as for lgn_step_finalize_f64; the
 * scratch slots -11 .. -8 of the block are the per-level counters of the fused launch (zero between calls, like the last slot).
 * Data-parallel training keeps the two calls above: the gradient all-reduce sits between them. */
int lgn_step_train_f64(const lgn_net_desc* d, double* params, double* grads, long long n_params, const int64_t* enc_off,
                       const int64_t* dec_off, const double* p4, const double* target, const uint8_t* mask, const double* in_scalars,
                       double* workspace, long long workspace_doubles, double* recon, double* loss_part, int n_loss, double l1_lambda,
                       double* adam_m, double* adam_v, long long* step_dev, double lr, double beta1, double beta2, double eps,
                       int do_adam, double* loss_out, const lgn_loss_desc* loss, int* assignment /* nullable */,
                       int* status /* nullable */, void* stream);

/* ---- the same two calls with an optimiser descriptor in place of the scalar hyper-parameter list: --optimizer rmsprop
 * (utils/initialize.py:153-173: torch.optim.RMSprop(params, lr, eps=get_eps(dtype), momentum=0.9)) and --l2-lambda
 * (utils/train.py:489-492: + l2_lambda * (encoder.l2_norm() + decoder.l2_norm()), l2_norm = sum w^2).  Per parameter, with g the
 * reduced loss gradient and w the weight BEFORE the update:
 *     g += l1_lambda * sign(w) + 2 * l2_lambda * w                  (a lambda of 0 switches its term off)
 *     LGN_OPT_ADAM:    lgn_step_finalize_f64's update on that g (l2_lambda == 0: its bits -- weights, moments, gradients, counter)
 *     LGN_OPT_RMSPROP: v = alpha v + (1 - alpha) g^2;  avg = sqrt(v) + eps;
 *                      momentum > 0:  buf = momentum buf + g / avg,  w -= lr buf;      momentum == 0:  w -= lr g / avg
 *                      (torch.optim.RMSprop, centered=False, weight_decay=0; torch's default alpha is 0.99, the reference passes
 *                      momentum 0.9 and eps 1e-16).  state_v carries square_avg, state_m the momentum buffer (untouched when
 *                      momentum == 0); no bias-correction powers; the device step counter advances by one per applied step.
 * do_step == 0: gradients and loss only, for both kinds.
 * loss_out must hold 4 + LGN_FINALIZE_OPT_SCRATCH doubles: loss_out[0..3] = total (= data + l1_lambda sum|w| + l2_lambda sum w^2),
 * data loss, sum|w|, sum w^2 (both norms of the weights before the update), then scratch of these calls' own -- NOT the block of the
 * calls above: TWO arrays of (LGN_FINALIZE_OPT_SCRATCH - 12) / 2 partial sums (|w|, then w^2; the fused tail of
 * lgn_step_train_opt_f64 needs a slot per tile in each, and a step with more tiles than that takes the separate launches), then, as
 * in the block above, four per-level counters (slots -11 .. -8), the cached powers of LGN_OPT_ADAM (-7 .. -2) and the
 * finished-workgroup counter (-1).  The same rule holds: the caller zero-fills the block ONCE, at allocation; every launch leaves
 * counters and partial-sum slots at zero (the fused tail reads "zero = not yet written in this launch": both sums are
 * non-negative and travel with the sign bit set), so the two calls -- and both kinds -- may be mixed on one block; after a launch
 * that died part-way, zero the block again before reusing it.
 * Both calls only enqueue (capturable) and refuse before the first launch with a negative code and lgn_last_error(). */
#define LGN_OPT_ADAM 0
#define LGN_OPT_RMSPROP 1
typedef struct {
  int kind;               /* LGN_OPT_ADAM | LGN_OPT_RMSPROP */
  double l1_lambda, l2_lambda, lr, eps;
  double beta1, beta2;    /* LGN_OPT_ADAM */
  double alpha, momentum; /* LGN_OPT_RMSPROP */
} lgn_optim_desc;
#define LGN_FINALIZE_OPT_SCRATCH 4096
/* lgn_step_finalize_f64 with a descriptor: the data-parallel and module-step form, called after the all-reduce */
int lgn_step_finalize_opt_f64(double* params, double* grads, long long n_params, const double* loss_part, int n_loss,
                              const lgn_optim_desc* opt, double* state_m, double* state_v, long long* step_dev, int do_step,
                              double* loss_out, void* stream);
/* lgn_step_train_f64 with a descriptor: the single-process form, ONE fused tail launch where lgn_step_train_f64 has one (same
 * gradients, state and weights as lgn_step_fwd_bwd_f64 + lgn_step_finalize_opt_f64 bit for bit, the loss value to rounding) */
int lgn_step_train_opt_f64(const lgn_net_desc* d, double* params, double* grads, long long n_params, const int64_t* enc_off,
                           const int64_t* dec_off, const double* p4, const double* target, const uint8_t* mask,
                           const double* in_scalars, double* workspace, long long workspace_doubles, double* recon,
                           double* loss_part, int n_loss, const lgn_optim_desc* opt, double* state_m, double* state_v,
                           long long* step_dev, int do_step, double* loss_out, const lgn_loss_desc* loss,
                           int* assignment /* nullable */, int* status /* nullable */, void* stream);

/* ---- guarded finalize: gradient-norm clipping, skip on a non-finite or exploding step, a learning rate that lives on the device.
 * The reference meets a diverging run on the host (utils/train.py: BLOW_UP_THRESHOLD = 1e32 on every batch_loss.item()); a
 * device-resident epoch has no host in the loop, so the decision is taken where the gradient is finished.  The call sits where the
 * descriptor finalize sits -- behind lgn_step_fwd_bwd_f64 and, under data parallelism, behind the all-reduce (every rank sees the
 * same reduced buffer and takes the same decision) -- and takes its arguments plus a host descriptor, read when the call is made,
 * and a device control block of LGN_CTL_DOUBLES doubles (caller-owned, zero-filled once).  These only ADD a struct, constants and
 * functions: LGN_AMD_ABI_VERSION stays 19.  Per call, with w the weights before the update and g the reduced loss gradient:
 *   G     = g + l1_lambda sign(w) + 2 l2_lambda w, written to `grads` (ALWAYS the unclipped regularised gradient);
 *   norm  = sqrt(sum G^2) over all n_params, summed in a fixed order (per-workgroup partials, then in index order);
 *   total = data + l1_lambda sum|w| + l2_lambda sum w^2;  loss_out[0..3] as the descriptor finalize writes them;
 *   bad_nf = skip_nonfinite && !(isfinite(norm) && isfinite(total));   bad_bu = threshold on && fabs(total) > blow_up_threshold;
 *   coef  = min(1, max_grad_norm / (norm + 1e-6)) with clipping on (torch.nn.utils.clip_grad_norm_; a NaN norm gives a NaN
 *           coefficient, as there), else exactly 1.0;
 *   t     = *step_dev + 1 (the number Adam uses);  lr of this step by lr_kind:
 *     LGN_LR_HOST           opt->lr
 *     LGN_LR_DEVICE         ctl[LGN_CTL_LR] (an 8-byte device write between two replays changes it; no re-capture)
 *     LGN_LR_WARMUP_COSINE  t <= W: base t / W;  else min + (base - min) 1/2 (1 + cos(pi min(t - W, T - W) / (T - W)))
 *     LGN_LR_WARMUP_STEP    t <= W: base t / W;  else base gamma^floor((t - W - 1) / step_size)
 *     (W = warmup_steps, T = total_steps; the closed form is also a host function, below)
 *   apply: only when do_step and neither bad_nf nor bad_bu -- the optimiser's update (LGN_OPT_ADAM / LGN_OPT_RMSPROP as above) on
 *     G coef with that lr: new weights, both state tensors, *step_dev + 1.  A skipped step writes none of them, so t does not
 *     advance.  With every control off and LGN_LR_HOST the weights, state, gradients and counter are the descriptor finalize's
 *     bit for bit (G * 1.0 is exact; Adam's powers are cached in this call's own block under the same protocol).
 * Control block: per-step fields LGN_CTL_LR_USED, LGN_CTL_GRAD_NORM, LGN_CTL_CLIP_COEF, LGN_CTL_FLAGS (bits LGN_CTL_CLIPPED,
 * LGN_CTL_SKIP_NONFINITE, LGN_CTL_SKIP_BLOWUP, as a double) are written by every call; the running fields -- LGN_CTL_APPLIED,
 * LGN_CTL_CLIPPED_STEPS, LGN_CTL_SKIPPED (counts), LGN_CTL_FIRST_SKIPPED (t of the first skipped step since the last reset, 0: none),
 * LGN_CTL_GRAD_NORM_MAX (largest finite norm), LGN_CTL_APPLIED_LOSS_SUM (sum of total over applied steps, one fp64 add per step in
 * step order) -- only with do_step (a capture's warm-up leaves no trace).  LGN_CTL_APPLY / LGN_CTL_BC1 / LGN_CTL_BC2_SQRT hand the
 * decision from the first launch to the second.  The reset call clears the running fields in a kernel (no memset node) and keeps
 * LGN_CTL_LR.
 * Two launches behind the reductions: gradient + partial sums + decision (the last workgroup to arrive assembles, as in the
 * finalize calls above: atomic exchange -> counter, no fence), then the update, which reads the decision across the launch
 * boundary (one launch with do_step == 0).  No workgroup waits for another.  loss_out must hold 4 + LGN_FINALIZE_CTL_SCRATCH
 * doubles: the 4 results, then scratch of this call's own -- THREE arrays of (LGN_FINALIZE_CTL_SCRATCH - 12) / 3 partial sums
 * (|w|, w^2, G^2), slots -7 .. -2 the cached powers of LGN_OPT_ADAM, slot -1 the finished-workgroup counter; zero-filled once by
 * the caller, partial sums and counter are zero again after every call.  Only enqueues (capturable); refuses before the first
 * launch with a negative code and the last-error message: null pointers, an unknown lr_kind, warmup_steps < 0, total_steps <=
 * warmup_steps under the cosine, step_size < 1 or gamma <= 0 under the step schedule, a negative base_lr or min_lr, missing state
 * with do_step, and whatever the descriptor finalize refuses. */
#define LGN_LR_HOST 0
#define LGN_LR_DEVICE 1
#define LGN_LR_WARMUP_COSINE 2
#define LGN_LR_WARMUP_STEP 3
typedef struct {
  double max_grad_norm;       /* <= 0 or +inf: no clipping */
  double blow_up_threshold;   /* <= 0 or +inf: off */
  int skip_nonfinite;
  int lr_kind;                /* LGN_LR_* */
  double base_lr, min_lr;
  long long warmup_steps, total_steps;
  double gamma;
  long long step_size;
} lgn_train_ctl;
#define LGN_CTL_LR 0
#define LGN_CTL_LR_USED 1
#define LGN_CTL_GRAD_NORM 2
#define LGN_CTL_CLIP_COEF 3
#define LGN_CTL_FLAGS 4
#define LGN_CTL_APPLIED 5
#define LGN_CTL_CLIPPED_STEPS 6
#define LGN_CTL_SKIPPED 7
#define LGN_CTL_FIRST_SKIPPED 8
#define LGN_CTL_GRAD_NORM_MAX 9
#define LGN_CTL_APPLIED_LOSS_SUM 10
#define LGN_CTL_APPLY 11
#define LGN_CTL_BC1 12
#define LGN_CTL_BC2_SQRT 13
#define LGN_CTL_DOUBLES 16
#define LGN_CTL_CLIPPED 1
#define LGN_CTL_SKIP_NONFINITE 2
#define LGN_CTL_SKIP_BLOWUP 4
#define LGN_FINALIZE_CTL_SCRATCH 4096
int lgn_step_finalize_ctl_f64(double* params, double* grads, long long n_params, const double* loss_part, int n_loss,
                              const lgn_optim_desc* opt, double* state_m, double* state_v, long long* step_dev, int do_step,
                              double* loss_out, const lgn_train_ctl* tc, double* ctl, void* stream);
int lgn_train_ctl_reset(double* ctl, void* stream);
/* the learning rate of step t >= 1 under *tc (device_lr: what LGN_LR_DEVICE returns; LGN_LR_HOST has no descriptor here and returns
 * device_lr as well); NaN for a null or refused descriptor.  Pure host arithmetic: the same inline function the kernel runs. */
double lgn_lr_schedule_value(const lgn_train_ctl* tc, long long t, double device_lr);

/* ---- evaluation step (the reference's validate() / test.py loop under torch.no_grad(), utils/train.py:390): encoder -> decoder ->
 * get_real(., d->get_real) -> Chamfer [+ d->jet_loss_scale * jet-feature term] or the assignment loss of `loss`, forward only and without L1 (regularization =
 * is_train, utils/train.py:308-314).  Takes every descriptor lgn_step_fwd_bwd_f64 takes and the same inputs; nothing is kept for a
 * backward, so the workspace (lgn_eval_workspace_doubles) is smaller than the training step's.  Only enqueues work (no allocation,
 * no host sync): capturable into a graph.  Refusals come before the first launch.
 *   recon_real [B][Nd][4] = get_real(reconstruction): the training step's reconstruction through the same get_real, bit for bit;
 *   lat_s [2][B][P tau_s], lat_v [2][B][P tau_v][4] (both or neither; NULL: not written) the pooled latent as lgn_encoder_fwd_f64
 *   writes it; loss_part [B] the per-jet terms (a data-parallel caller reduces them); loss_out[0] = sum of loss_part over the jets
 *   with at least one unmasked particle (a short last batch is padded with all-masked jets), in a fixed order. */
long long lgn_eval_workspace_doubles(const lgn_net_desc* d);
int lgn_step_eval_f64(const lgn_net_desc* d, const double* params, const int64_t* enc_off, const int64_t* dec_off,
                      const double* p4_scaled, const double* p4_target, const uint8_t* mask, const double* in_scalars,
                      double* workspace, long long workspace_doubles, double* recon_real, double* lat_s /*nullable*/,
                      double* lat_v /*nullable*/, double* loss_part, double* loss_out, const lgn_loss_desc* loss,
                      int* assignment /* [B][Nd], nullable */, int* status /* [B], nullable */, void* stream);

/* ---- one network at a time, maxdim = 2: what LGNEncoder.forward / LGNDecoder.forward (lgn/models/lgn_encoder.py:255-336,
 * lgn_decoder.py:218-303) and autograd's backward of them become under the module API.  Same parameter-slot layout as
 * above, but `params` / `grads` / `off` refer to ONE network's flat parameter block.  *_fwd writes the activations the
 * backward needs into `act` (lgn_net_workspace_doubles(d, decoder, 0) doubles, owned by the caller between the two
 * calls); *_bwd zero-fills `grads`, then writes every parameter gradient (dead parameters keep an exact 0) and uses
 * `scratch` (lgn_net_workspace_doubles(d, decoder, 1) doubles).
 *   encoder: p4 [B][N][4] (already scaled), mask [B][N], in_scalars [B][N][K - 1] (NULL when d->n_in_scalars <= 1: the input
 *            MixReps (0,0) weight is [2][C][K], slot 0) -> lat_s [2][B][P tau_s], lat_v [2][B][P tau_v][4] Cartesian
 *            (P = 2 for the default 'min&max' pooling, see lgn_net_desc.latent_pool); g_lat_s may be NULL (no gradient on the latent scalars: the last level's scalar
 *            branch is then skipped, like autograd would).
 *   decoder: lat_v [2][B][Tin][4] (Tin = tau_v_in, or 2 tau_v when 0) -> recon [2][B][N][4] complex Cartesian;
 *            backward from g_recon [2][B][N][4] to g_lat_v (the latent scalars never reach the output). */
long long lgn_net_workspace_doubles(const lgn_net_desc* d, int decoder, int which);
int lgn_encoder_fwd_f64(const lgn_net_desc* d, const double* params, const int64_t* off, const double* p4, const uint8_t* mask,
                        const double* in_scalars, double* act, long long act_doubles, double* lat_s, double* lat_v, void* stream);
int lgn_encoder_bwd_f64(const lgn_net_desc* d, const double* params, double* grads, long long n_params, const int64_t* off,
                        const double* p4, const uint8_t* mask, const double* in_scalars, const double* act, long long act_doubles,
                        const double* g_lat_s, const double* g_lat_v, double* scratch, long long scratch_doubles, void* stream);
int lgn_decoder_fwd_f64(const lgn_net_desc* d, const double* params, const int64_t* off, const double* lat_v, double* act,
                        long long act_doubles, double* recon, void* stream);
int lgn_decoder_bwd_f64(const lgn_net_desc* d, const double* params, double* grads, long long n_params, const int64_t* off,
                        const double* lat_v, const double* act, long long act_doubles, const double* g_recon, double* g_lat_v,
                        double* scratch, long long scratch_doubles, void* stream);

/* ---- Chamfer loss on its own (module API: lgn/losses.py ChamferLoss, the drop-in of utils/losses/chamfer_loss/chamfer_loss.py:7-31;
 * the whole-step call has the loss inside the decoder's last kernel).  x [B][N][4], y [B][M][4] real 4-vectors, cdist = sum of
 * squared component differences (distance_sq.py:263-304, even p: no eps).
 *   loss_part[b] = (sum_i min_j d_ij + sum_j min_i d_ij) / 2  [+ sum_mu (sum_i x - sum_j y)_mu^2 / (4 B) with jet_features: the
 *                  nn.MSELoss() of the jet momenta, chamfer_loss.py:25-29];  the loss is the sum of loss_part over the batch
 *   gx [B][N][4], gy [B][M][4] = d loss / d x, d loss / d y (first minimum on ties, as torch.min; gy may be needed for a target that
 *                  requires grad -- always written) */
int lgn_chamfer_f64(int B, int N, int M, const double* x, const double* y, int jet_features, double* loss_part, double* gx, double* gy,
                    void* stream);

/* ---- anomaly scores (the reference's anomaly_scores(), utils/jet_analysis/anomaly_detection.py, with include_emd=False) ---------
 * recons, target, recons_n, target_n [B][N][4] real Cartesian (E, px, py, pz) 4-vectors (recons_n / target_n: the normalized
 * jets).  One workgroup per jet; nothing is allocated, nothing waits on the host: capturable into a graph.  1 <= N <= LGN_ANOMALY_NMAX.
 *   scores [B][LGN_ANOMALY_NSCORES] in the reference's key order (lgn/anomaly.py: SCORE_KEYS):
 *      0..4 Chamfer, 5..9 Hungarian, 10..14 MSE in the Cartesian, polar, normalized Cartesian, normalized polar and relative polar
 *      frames; 15 jet Cartesian; 16 jet "polar" (the reference scores it on the Cartesian jets: equal to 15); 17 Chamfer, 18 Hungarian,
 *      19 MSE and 20 jet with the Minkowski square diag(+,-,-,-).  Nothing is masked: zero-padded rows take part, as in the reference.
 *      Hungarian: col_ind = scipy's linear_sum_assignment of C[i][j] = |p_i - q_j| (Lorentz: the signed Minkowski square), and the
 *      score is the reference's mean_r sum_c (p[col_ind[r]]_c - q[r]_c)^2 (Lorentz: on the Cartesian frame).
 *   score_mask: bit k asks for score k (LGN_ANOMALY_ALL: every score); a score not asked for is written as NaN, and a Hungarian
 *      variant not asked for is not solved (its col4row row is -1).  LGN_ANOMALY_NO_HUNGARIAN skips the six assignments.
 *   col4row [6][B][N] (nullable) int32: col_ind of the Hungarian variants in score order (5..9, 18).
 *   status [B] int32: bit v (v = 0..5) -- variant v has a NaN or -inf cost (scipy: "matrix contains invalid numeric entries");
 *      bit 8 + v -- variant v is infeasible.  Either way its score is NaN and its col4row row -1.
 * Replaces: anomaly_scores() and its helpers chamfer / hungarian / mse / *_lorentz / get_p4_polar / get_polar_rel. */
#define LGN_ANOMALY_NMAX 192
#define LGN_ANOMALY_NSCORES 21
#define LGN_ANOMALY_ALL 0x1FFFFF
#define LGN_ANOMALY_HUNGARIAN 0x403E0        /* bits 5..9 and 18 */
#define LGN_ANOMALY_NO_HUNGARIAN (LGN_ANOMALY_ALL & ~LGN_ANOMALY_HUNGARIAN)
int lgn_anomaly_scores_f64(const double* recons, const double* target, const double* recons_n, const double* target_n, int B, int N,
                           int score_mask, double* scores, int* col4row /*nullable*/, int* status, void* stream);

/* ---- ROC curves and AUCs of score columns (the reference's get_ROC_AUC(), utils/jet_analysis/anomaly_detection.py; csrc/roc.hip) ----
 * For every column k < K of scores (M rows, column k at scores + k, row stride ld >= K: a [B][21] score tensor is read in place):
 * sklearn.metrics.roc_curve(labels, scores[:, k]) with its defaults (drop_intermediate=True, pos_label inferred: 1), then
 * sklearn.metrics.auc(fpr, tpr), then the reference's flip: with an AUC < 0.5 the curve and AUC are those of the negated labels --
 * fpr and tpr exchanged, thresholds unchanged, the AUC summed again from the exchanged curve -- and flipped[k] = 1.
 * Sorted on the device (bitonic tiles of LGN_ROC_TILE pairs in LDS, then merge passes between two workspace buffers); counts are
 * int32, each rate is one IEEE division, the AUC is summed in a fixed order (the same input gives the same bits), no floating-point
 * atomics.  On the caller's stream; nothing is allocated, nothing waits on the host: capturable into a graph.
 *   labels      [M] fp64: 1 is the positive class; the other class is 0 or -1 (not both)
 *   fpr, tpr, thresholds [K][M + 1]: the first length[k] entries of row k are the curve; thresholds[k][0] = +inf; a threshold
 *               that is a zero is +0.0 (sklearn keeps the sign of one of the tied zeros)
 *   length, flipped, status [K] int32;  auc [K]
 *   status      LGN_ROC_NONFINITE -- the column holds NaN or +-inf (with LGN_ROC_NAN: a NaN); LGN_ROC_SINGLE_CLASS -- only one class
 *               among the labels; LGN_ROC_BAD_LABEL -- a label outside {-1, 0, 1}, or both -1 and 0.  Such a column has length 0 and
 *               auc NaN (its curve rows are unspecified); the other columns are unaffected.
 *   workspace   8-byte aligned device memory of at least the bytes the workspace query returns (< 0: bad arguments)
 * Refused before any launch: null pointers, M < 1 or M >= 2^31, K < 1 or K > LGN_ROC_MAX_COLS, ld < K, a short workspace. */
#define LGN_ROC_TILE 2048
#define LGN_ROC_MAX_COLS 65535
#define LGN_ROC_NONFINITE 1
#define LGN_ROC_SINGLE_CLASS 2
#define LGN_ROC_BAD_LABEL 4
#define LGN_ROC_NAN 8
long long lgn_roc_workspace_bytes(long long M, int K);
int lgn_roc_auc_f64(const double* scores, long long M, int ld, int K, const double* labels, double* fpr, double* tpr,
                    double* thresholds, int* length, double* auc, int* flipped, int* status, void* workspace,
                    long long workspace_bytes, void* stream);

/* ---- energy mover's distance (csrc/emd.hip, csrc/emd_wave.hpp): the reference's 22nd anomaly score "emd (relative coordinates)",
 * emd_loss() of utils/jet_analysis/anomaly_detection.py, which calls energyflow.emd.emd(p, q) per jet with its defaults (R = 1, beta = 1,
 * norm = False, Euclidean ground distance, no periodic phi).  energyflow was not available when this was written: the definition
 * below, taken from its documentation, is the specification.  For events (pT_i, y_i, phi_i), i < n, and (pT'_j, y'_j, phi'_j), j < m:
 *      theta_ij = sqrt((y_i - y'_j)^2 + (phi_i - phi'_j)^2) / R
 *      EMD      = min over f >= 0 of sum f_ij theta_ij + |sum pT - sum pT'|
 *                 with sum_j f_ij <= pT_i, sum_i f_ij <= pT'_j, sum f_ij = min(sum pT, sum pT')
 * solved exactly as a balanced transportation problem: one fictitious particle on the lighter side carries the weight difference at
 * cost 1 to every particle of the other event.  Successive shortest paths, one wavefront per pair of events; the order of the two
 * arguments does not change the cost.  Nothing is allocated, nothing waits on the host: capturable into a graph.
 *   lgn_emd_f64: ev0 [B][n][3], ev1 [B][m][3] events of (pT, y, phi); n != m allowed; 1 <= n, m <= LGN_EMD_NMAX; R > 0.
 *      emd    [B]
 *      flow   [B][n + 1][m + 1] (nullable): the optimal flow; row n and column m are the fictitious particles (at most one has weight)
 *      dual0  [B][n + 1], dual1 [B][m + 1] (nullable): potentials with dual0_i + dual1_j <= theta_ij (1 on a fictitious arc), equality
 *             where flow_ij > 0, so that sum f theta = sum dual0 w + sum dual1 w' certifies the optimum
 *      status [B] int32: LGN_EMD_INVALID -- NaN or +-inf anywhere, or a negative weight; LGN_EMD_EMPTY -- both events weightless (what
 *             energyflow returns there is not known); LGN_EMD_ITER -- the cap of 16 (n + m + 2) augmentations was hit;
 *             LGN_EMD_INFEASIBLE -- more weight was left over than the rounding of the two sums, (n + m) 2^-52 max(sum pT, sum pT'),
 *             explains.  With a status bit emd (and flow, dual0, dual1) of that pair is NaN; the other pairs are unaffected.
 *             One event weightless is well defined: the other event's sum pT.
 *      work   the flow matrices when they do not fit LDS: at least lgn_emd_workspace_bytes(B, max(n, m)) bytes of 8-byte aligned device
 *             memory (0 bytes: work may be NULL).  lgn_emd_lds_bytes(N): the LDS of one wavefront at N particles per event; the flow
 *             is in LDS when that is at least 8 (N + 1)^2.
 *   lgn_emd_relative_f64: recons, target [B][N][4] real Cartesian (E, px, py, pz) jets; each is staged into its relative-polar frame
 *      (pT / (jet pT + 1e-16), eta - jet eta, wrapped phi - jet phi) exactly as lgn_anomaly_scores_f64 stages it, then solved with
 *      R = 1: the reference's score.  Zero-padded particles have no weight.
 *   Refused before any launch (negative return): null pointers, B < 1, n, m or N outside 1 .. LGN_EMD_NMAX, R not a finite positive
 *   number, a missing, short or misaligned workspace.
 *   lgn_emd_grad_f64, lgn_emd_relative_grad_f64: the same distances (bit for bit) with their gradients, computed in the same launch by
 *   the wavefront that solved the pair (LP sensitivity: the optimal flow weighs d theta / d position, the potentials are d EMD / d
 *   weight).  These two only ADD functions: LGN_AMD_ABI_VERSION stays 19 (the rule above lgn_column_stats_f64).  With S0 = sum pT,
 *   S1 = sum pT', u = dual0, v = dual1, row n and column m the fictitious particles:
 *      dE/dy_i   =  sum_j f_ij (y_i - y'_j) / (R^2 theta_ij)       dE/dy'_j  = -sum_i (the same term)        (phi alike)
 *      dE/dpT_i  =  u_i - [S1 > S0] u_n + [S0 > S1] v_m            dE/dpT'_j =  v_j - [S0 > S1] v_m + [S1 > S0] u_n
 *   An arc with theta_ij = 0 contributes 0; at S0 == S1 neither fictitious term is added; a weightless particle gets a zero position
 *   gradient and the weight gradient above: every output of a pair without a status bit is finite.  With a status bit every gradient
 *   of that pair is NaN, like its value; the other pairs are unaffected.
 *      g0 [B][n][3], g1 [B][m][3] (each nullable, not both): columns (d/dpT, d/dy, d/dphi), like the events
 *      g_recons [B][N][4], g_target [B][N][4] (nullable): the gradient carried back to the Cartesian jets through w = pT / (jet pT +
 *             1e-16), y = eta - jet eta, phi = wrap(phi - jet phi) (wrap has derivative 1) and the frame's (pT, eta, phi), with the
 *             term every particle receives through the jet sum.  The E column is 0.  A particle with pT == 0 gets no direct term (the
 *             0/0 of the root and of atan2 reads as 0), only the jet-sum term.
 *   The workspace, the LDS and the refusals are those of lgn_emd_f64 / lgn_emd_relative_f64 (g_recons is required), and one more:
 *   lgn_emd_grad_f64 with g0 and g1 both null.  Nothing is allocated, nothing waits on the host: capturable.
 *   lgn_emd_debug_max_augmentations: DEBUG ONLY, not part of the stable surface (it may change or go without an ABI bump): the
 *   largest number of augmentations of any pair since the last reset, on the current device only (one counter per device, fed by one
 *   integer atomic max per pair), read with a blocking copy: it waits on the host and is not capturable.  For tools/emd_bench.py. */
#define LGN_EMD_NMAX 191
#define LGN_EMD_INVALID 1
#define LGN_EMD_EMPTY 2
#define LGN_EMD_ITER 4
#define LGN_EMD_INFEASIBLE 8
long long lgn_emd_workspace_bytes(int B, int N);
long long lgn_emd_lds_bytes(int N);
int lgn_emd_f64(const double* ev0, const double* ev1, int B, int n, int m, double R, double* emd, double* flow /*nullable*/,
                double* dual0 /*nullable*/, double* dual1 /*nullable*/, int* status, void* work, long long work_bytes, void* stream);
int lgn_emd_relative_f64(const double* recons, const double* target, int B, int N, double* emd, int* status, void* work,
                         long long work_bytes, void* stream);
int lgn_emd_grad_f64(const double* ev0, const double* ev1, int B, int n, int m, double R, double* emd, double* g0 /*nullable*/,
                     double* g1 /*nullable*/, double* flow /*nullable*/, double* dual0 /*nullable*/, double* dual1 /*nullable*/,
                     int* status, void* work, long long work_bytes, void* stream);
int lgn_emd_relative_grad_f64(const double* recons, const double* target, int B, int N, double* emd, double* g_recons,
                              double* g_target /*nullable*/, int* status, void* work, long long work_bytes, void* stream);
int lgn_emd_debug_max_augmentations(int* out, int reset);

/* ---- matrices of EMDs and energyflow's options (csrc/emd_pairs.hip, csrc/emd_plan.hpp): energyflow.emd.emds and the R, beta, norm and
 * periodic_phi arguments of energyflow.emd.emd, around the solver above (one wavefront per pair; a persistent grid strides over the
 * pair numbers p in [0, P), 64-bit).  These only ADD functions: LGN_AMD_ABI_VERSION stays 19.
 *   mode   LGN_EMD_PAIRS_FULL     p = i B1 + j: ev0[i] against ev1[j], P = B0 B1; emd, status [B0][B1]
 *          LGN_EMD_PAIRS_UPPER    one set against itself (ev1 NULL or ev0, n == m, B1 == B0 = B): only i < j is solved, row-major over
 *                                 the upper triangle, P = B (B - 1) / 2; emd, status [B][B], [i][j] and [j][i] get the same value, the
 *                                 diagonal is +0.0 with status 0 whatever the event holds.  B == 1 solves nothing and writes the one zero.
 *          LGN_EMD_PAIRS_ALIGNED  B1 == B0, p = i: ev0[i] against ev1[i] as lgn_emd_f64 pairs them; emd, status [B0]; flow, dual0, dual1
 *                                 (each nullable) in the layouts of lgn_emd_f64.  In the other modes a non-null one is refused.
 *   lgn_emd_pairs_decode: the pair (i, j) of pair number p, on the host (the kernel decodes with the same function): integer-exact.
 *   opts   NULL: R = 1, beta = 1, norm = 0, periodic_phi = 0, at which every result has the bits lgn_emd_f64 gives for the same pair.
 *          energyflow is not available to this project: the definition here is the specification.  Every step is one rounded operation:
 *            dphi   = phi_i - phi'_j;  periodic_phi: dphi = pi - |pi - |phi_i - phi'_j|| with pi the double M_PI (the minimum image
 *                     for |phi_i - phi'_j| <= 2 pi; applied as written outside that)
 *            theta  = sqrt(dy^2 + dphi^2), divided by R unless R == 1
 *            cost   = theta for beta == 1, theta * theta for beta == 2, pow(theta, beta) otherwise.  The fictitious particle's cost
 *                     stays 1: the term |sum pT - sum pT'| is not raised to beta.
 *            norm   each event's weights are divided by that event's sum (summed as staged); the fictitious particle gets no weight;
 *                     the rounding difference of the two normalised sums is dropped under the leftover tolerance of lgn_emd_f64,
 *                     computed from the normalised sums; flow, dual0 and dual1 refer to the normalised weights.  With norm an event
 *                     without weight on either side of a pair is LGN_EMD_EMPTY (without: only both sides weightless, as above).
 *   status is per pair: an invalid event (NaN, +-inf, a negative weight) marks every pair it takes part in and no other.
 *   work   at least lgn_emd_workspace_bytes(min(P, INT_MAX), max(n, m)) bytes, 8-byte aligned (0 bytes: may be NULL).
 *   Refused before any launch (negative return): null ev0, emd or status (ev1 outside UPPER); B0 or B1 < 1; n or m outside
 *   1 .. LGN_EMD_NMAX; an unknown mode; UPPER with n != m, B0 != B1 or an ev1 that is neither NULL nor ev0; ALIGNED with B0 != B1; R or
 *   beta not a finite positive number; flow or duals outside ALIGNED; a short, missing or misaligned workspace.  Nothing is allocated,
 *   nothing waits on the host, no buffer is cleared by a memset: capturable.  Gradients under the options: the section below. */
#define LGN_EMD_PAIRS_FULL 0
#define LGN_EMD_PAIRS_UPPER 1
#define LGN_EMD_PAIRS_ALIGNED 2
typedef struct lgn_emd_opts {
  double R, beta;
  int norm, periodic_phi;
} lgn_emd_opts;
int lgn_emd_pairs_decode(int mode, long long p, int B0, int B1, int* i, int* j);
int lgn_emd_pairs_f64(const double* ev0, const double* ev1 /*NULL: UPPER*/, int B0, int B1, int n, int m, int mode,
                      const lgn_emd_opts* opts /*nullable*/, double* emd, double* flow /*nullable*/, double* dual0 /*nullable*/,
                      double* dual1 /*nullable*/, int* status, void* work, long long work_bytes, void* stream);

/* ---- gradients of the EMD under the options (csrc/emd_grad_opts.hip): the GRAD calls above with an lgn_emd_opts, computed like them by
 * the wavefront that solved the pair.  These only ADD functions: LGN_AMD_ABI_VERSION stays 19.  The value (and flow, dual0, dual1) is the
 * ALIGNED mode's of the pairs call above under the same options, bit for bit.  With dy = y_i - y'_j, D = phi_i - phi'_j, dphi and
 * theta_ij as defined above, f the optimal flow in the units of the staged weights (normalised under norm), u = dual0, v = dual1,
 * S0 = sum pT, S1 = sum pT' as given, row n and column m the fictitious particles:
 *      s_ij      = 1 without periodic_phi;  sign(D) sign(pi - |D|) with it (0 at D = 0 and at |D| = pi)
 *      k_ij      = f_ij beta theta_ij^(beta - 2) / R^2   where theta_ij > 0, else 0 (at every beta)
 *      dE/dy_i   =  sum_j k_ij dy             dE/dy'_j   = -sum_i k_ij dy
 *      dE/dphi_i =  sum_j k_ij dphi s_ij      dE/dphi'_j = -sum_i k_ij dphi s_ij
 *      norm off:  dE/dpT_i = u_i - [S1 > S0] u_n + [S0 > S1] v_m          dE/dpT'_j = v_j - [S0 > S1] v_m + [S1 > S0] u_n
 *      norm on :  dE/dpT_i = (u_i - sum_k a_k u_k) / S0, a = pT / S0      dE/dpT'_j = (v_j - sum_k b_k v_k) / S1, b = pT' / S1
 *   The norm form does not change under the shift (u + c, v - c) a balanced problem leaves free.  An arc with theta_ij = 0 contributes 0
 *   at every beta (for beta < 1 the true derivative is unbounded there: a convention); a weightless particle gets a zero position
 *   gradient and the weight gradient above with its finished potential: every output of a pair without a status bit is finite.  With a
 *   status bit (with norm: LGN_EMD_EMPTY when either event is weightless) value and gradients of that pair are NaN, the other pairs
 *   are unaffected.
 *   lgn_emd_grad_opts_f64: the arguments of lgn_emd_grad_f64 with opts (nullable) in the place of R.
 *   lgn_emd_relative_opts_f64: recons, target [B][N][4] Cartesian jets staged into their relative-polar frames as lgn_emd_relative_f64
 *      stages them, solved under opts, the gradients (g_w, g_y, g_phi) carried back to the Cartesian jets as lgn_emd_relative_grad_f64
 *      carries them.  g_recons NULL: the value only, the score under the options (g_target must then be NULL too).
 *   opts NULL, or R = 1, beta = 1, norm = 0, periodic_phi = 0: every output has the bits of lgn_emd_grad_f64, lgn_emd_relative_grad_f64
 *   or (g_recons NULL) lgn_emd_relative_f64, which then run.  Workspace and LDS are those of lgn_emd_f64.
 *   Refused before any launch (negative return): null ev0, ev1, recons, target, emd or status; B < 1; n, m or N outside
 *   1 .. LGN_EMD_NMAX; R or beta not a finite positive number; g0 and g1 both null; g_target without g_recons; a short, missing or
 *   misaligned workspace.  Nothing is allocated, nothing waits on the host, no buffer is cleared by a memset: capturable.
 *   Not offered: energyflow's gdim, spherical measure, coords and mask.  Gradients of the FULL and UPPER matrices: the section after
 *   this one.  The EMD as the loss of the whole-step calls: LGN_LOSS_EMD, after that. */
int lgn_emd_grad_opts_f64(const double* ev0, const double* ev1, int B, int n, int m, const lgn_emd_opts* opts /*nullable*/, double* emd,
                          double* g0 /*nullable*/, double* g1 /*nullable, not both*/, double* flow /*nullable*/,
                          double* dual0 /*nullable*/, double* dual1 /*nullable*/, int* status, void* work, long long work_bytes,
                          void* stream);
int lgn_emd_relative_opts_f64(const double* recons, const double* target, int B, int N, const lgn_emd_opts* opts /*nullable*/,
                              double* emd, double* g_recons /*nullable: value only*/, double* g_target /*nullable*/, int* status,
                              void* work, long long work_bytes, void* stream);

/* ---- the EMD as the loss stage of the whole-step calls (csrc/emd_loss.hip): lgn/losses.py's EMDLoss and HybridLoss inside
 * lgn_step_fwd_bwd_f64, lgn_step_train_f64, lgn_step_train_opt_f64 and lgn_step_eval_f64.  This only ADDS a kind, a struct and a
 * function: LGN_AMD_ABI_VERSION stays 19 and no existing struct or signature changes.  A `loss` whose kind is LGN_LOSS_EMD is read as
 * an lgn_emd_loss_desc, whose first member it is (pass &desc.base).  With x = get_real(reconstruction) and t = target, per jet b:
 *      E_b          = the value of lgn_emd_relative_opts_f64(x, t) under opts, bit for bit (at default options: lgn_emd_relative_f64's)
 *      loss_part[b] = base.scale * E_b                                   chamfer_weight == 0 (EMDLoss)
 *                   = chamfer_weight * Chamfer_b + base.scale * E_b      chamfer_weight  > 0 (HybridLoss), each product rounded
 *   and the gradient is that call's g_recons (times base.scale) carried through get_real and the output mix like every other loss
 *   gradient.  The loss is a SUM over the jets, like Chamfer.  One launch of its own after the decoder's last level, one workgroup per
 *   jet; one wavefront of it solves the jet with the device functions of the calls above (csrc/emd_dev.hpp).  Under the hybrid loss the
 *   step's Chamfer stage runs first, exactly as without a `loss` (riding on the decoder's last level where it does), with
 *   chamfer_weight as its gradient scale; the EMD stage then recomputes x (the same bits) and adds its gradient into the last level's
 *   vectors, its dWo1 partial row and its term of loss_part[b] to what that stage wrote -- the owning thread's read-modify-write, in a
 *   fixed order, no atomics.  The reconstruction is the Chamfer step's bit for bit.
 *   base.abs_coord = base.polar_coord = 0.  `assignment` is ignored; status [B] int32 (nullable) receives the LGN_EMD_* bits.  A
 *   flagged jet follows the contract of lgn_loss_desc: loss_part[b] is NaN and the stage hands on exact zeros for the jet (under the
 *   hybrid loss: it adds nothing, the jet's Chamfer gradient stays).  Without norm "both events weightless" (LGN_EMD_EMPTY) needs a
 *   reconstruction without any pT; with norm a target without weight -- an all-padded jet -- is LGN_EMD_EMPTY.  lgn_step_eval_f64 sums
 *   loss_part over the jets that have an unmasked particle: it selects, so the NaN of an all-masked pad jet does not reach loss_out.
 *   The flow matrix lives in LDS only, so the workspace sizes still do not depend on the loss.
 *   lgn_emd_loss_lds_bytes(N, C): the dynamic LDS of the stage at N decoder particles and C channels of the decoder's last level, the one
 *   place that counts it (-1 for N < 1 or C < 1):
 *      8 * (20 N + 10 N C + 2 C)              the output stage's block (that of lgn_assign_loss_lds_bytes without the assignment's own)
 *      + 8 * (5 (N + 1) + 8 + (N + 1)^2)      one wavefront's rows, jets and flow: lgn_emd_lds_bytes' count with the flow in LDS
 *      + 8 * (N + 1)                          its two int arrays
 *   Refused before any launch (negative return): R or beta not a finite positive number; chamfer_weight negative or not finite;
 *   base.scale not positive and finite; d->jet_loss_scale != 0; Nd outside 1 .. LGN_EMD_NMAX; lgn_emd_loss_lds_bytes(Nd, C) above
 *   LGN_LDS_LIMIT (a flow in a global workspace is not offered here).
 *   Layout: sizeof(lgn_emd_loss_desc) = 56; offsets base 0 (kind 0, abs_coord 4, polar_coord 8, scale 16), opts 24 (R 24, beta 32,
 *   norm 40, periodic_phi 44), chamfer_weight 48. */
typedef struct lgn_emd_loss_desc {
  lgn_loss_desc base;      /* kind = LGN_LOSS_EMD, abs_coord = polar_coord = 0, scale = weight of the EMD term (1) */
  lgn_emd_opts opts;
  double chamfer_weight;   /* 0: the EMD alone; > 0: chamfer_weight * Chamfer + EMD (HybridLoss) */
} lgn_emd_loss_desc;
long long lgn_emd_loss_lds_bytes(int N, int C);

/* ---- gradients of a matrix of EMDs (csrc/emd_pairs_grad.hip): d sum_ij G[i][j] E[i][j] / d events for the FULL and UPPER matrices of
 * lgn_emd_pairs_f64, each pair solved once.  These only ADD functions: LGN_AMD_ABI_VERSION stays 19.  Two calls work on a range of
 * whole rows [row_begin, row_begin + row_count) of the matrix: its pairs are the pair numbers p_begin .. p_begin + P - 1 of the mode
 * (FULL: P = row_count B1; UPPER: the rows' pairs i < j, row i holds B - 1 - i), and pair p_begin + q is row q of the two slabs.
 *   lgn_emd_pairs_grad_f64: one wavefront per pair on the persistent grid of lgn_emd_pairs_f64 stages ev0[i] and ev1[j] where they lie
 *      (no gathered copies), solves the pair and writes
 *        emd, status [B0][B1] (each nullable): the value and the status of the pair, with the bits of lgn_emd_pairs_f64 under the same
 *               opts; UPPER mirrors them to [j][i] and writes +0.0 / 0 on the diagonal of the rows of the range.
 *        s0 [P][n][3], s1 [P][m][3]: d E[i][j] / d ev0[i] and d E[i][j] / d ev1[j] as (d/dpT, d/dy, d/dphi), with the bits
 *               lgn_emd_grad_opts_f64 gives g0 and g1 for the aligned pair (ev0[i], ev1[j]) under the same opts (the formulas of the
 *               section above).  A pair with a status bit has value NaN and NaN in both of its slab rows.
 *      work: at least lgn_emd_workspace_bytes(min(max(P, 1), INT_MAX), max(n, m)) bytes, 8-byte aligned (0 bytes: may be NULL); what
 *      the whole matrix needs is enough for every range.
 *   lgn_emd_pairs_grad_slab_bytes: the bytes of s0 and s1 together for a row range, P (n + m) 24 (s0 takes P n 24 of them); negative
 *      for a shape or a range the calls refuse.
 *   lgn_emd_pairs_grad_reduce_f64: the slabs of a row range, weighted by G [B0][B1] (nullable: every weight 1), summed into
 *      g0 [B0][n][3] and g1 [B1][m][3] (each nullable, not both).  One thread owns one output double and sums sequentially, one rounded
 *      product then one rounded sum per pair -- no FMA, no atomics, no tree -- in this order:
 *        FULL   g0[i], i in the range:  acc = +0.0, then acc = acc + G[i][j] s0[i, j] for j ascending (complete in one call; other rows
 *               of g0 are not touched).  g1[j]: acc = acc + G[i][j] s1[i, j] for the rows i of the range ascending.
 *        UPPER  (g1 must be NULL) g0[e], every e: the weight of pair i < j is w = G[i][j] + G[j][i] (one rounded sum; 2 without G);
 *               partners ascending: first the rows k < e of the range with w s1[k, e], then, if row e is in the range, k > e with
 *               w s0[e, k].  The diagonal gives nothing.
 *      g1 (UPPER: g0) starts at +0.0 in a call with row_begin == 0 and continues from what is stored otherwise: ranges that cover the
 *      matrix, processed in ascending order, give bits that do not depend on where they were cut, on the grid or on the run.  NaN
 *      propagates: a pair with a status bit makes the gradients of both its events NaN whatever G holds there.
 *   Refused before any launch (negative return): null ev0, s0 or s1 (ev1 in FULL); B0 or B1 < 1; n or m outside 1 .. LGN_EMD_NMAX;
 *   ALIGNED or an unknown mode; UPPER with n != m, B0 != B1, an ev1 that is neither NULL nor ev0, or a non-null g1; a row range
 *   outside the matrix (row_count < 1 included); R or beta not a finite positive number; a short, missing or misaligned workspace; g0
 *   and g1 both null.  Nothing is allocated, nothing waits on the host, no buffer is cleared by a memset: capturable.
 *   Not offered: the matrix of the relative (Cartesian jet) form. */
long long lgn_emd_pairs_grad_slab_bytes(int mode, int B0, int B1, int n, int m, int row_begin, int row_count);
int lgn_emd_pairs_grad_f64(const double* ev0, const double* ev1 /*NULL: UPPER*/, int B0, int B1, int n, int m, int mode,
                           const lgn_emd_opts* opts /*nullable*/, int row_begin, int row_count, double* emd /*nullable*/, double* s0,
                           double* s1, int* status /*nullable*/, void* work, long long work_bytes, void* stream);
int lgn_emd_pairs_grad_reduce_f64(const double* s0, const double* s1, const double* G /*nullable*/, int B0, int B1, int n, int m, int mode,
                                  int row_begin, int row_count, double* g0 /*nullable*/, double* g1 /*nullable*/, void* stream);

/* ---- entropic optimal transport and the Sinkhorn divergence (csrc/sinkhorn.hip): the regularised, smooth relative of the EMD above,
 * solved by Sinkhorn iterations in the log domain, one wavefront per pair.  These only ADD functions, a struct and a status bit:
 * LGN_AMD_ABI_VERSION stays 19.  energyflow, POT and geomloss are not available to this project: the definition here is the
 * specification (tests/_sinkhorn_ref.py restates it in numpy).
 *   Inputs   ev0 [B][n][3], ev1 [B][m][3], columns (pT, y, phi); opts.base gives cost and staging exactly as lgn_emd_pairs_f64 defines
 *            them (R, beta, norm, periodic_phi); epsilon > 0, max_iter >= 1, tol >= 0, debias 0 or 1.
 *   Extended problem: the EMD's.  Without norm the lighter event gets a fictitious particle (row n or column m) of weight |S0 - S1| at
 *            cost 1 to every particle of the other event (0 to the other fictitious one); with norm each event's weights are divided
 *            by that event's sum and there is none.  a [n + 1], b [m + 1] are the extended weights, S = max(sum a, sum b) (the two sums
 *            agree to rounding), C [n + 1][m + 1] the cost.
 *   Objective  OT_eps(a, b) = min over P of <P, C> + eps KL(P | a (x) b / S).
 *   Iteration k = 1, 2, ..., from g = 0:
 *            f_i <- -eps log sum_j (b_j / S) exp((g_j - C_ij) / eps)
 *            g_j <- -eps log sum_i (a_i / S) exp((f_i - C_ij) / eps)
 *            evaluated on F = f / eps, G = g / eps, Cs = C / eps as F_i = -(M + log sum_j exp(t_j - M)), t_j = (log(b_j / S) + G_j) - Cs_ij,
 *            M = max_j t_j.  Terms of weightless particles are skipped; a weightless particle still gets its potential.  Every sum runs
 *            in index order in one lane; err, the value and the mean potentials of the norm form are per-lane sums in index order
 *            (indices l, l + 64, ...) reduced by a fixed butterfly: the same bits run to run, whatever B and the pair's place in it.
 *   Stopping, at no extra pass: when iteration k + 1 has computed f_new, err = sum_i a_i |1 - exp((f_i - f_new_i) / eps)|, the
 *            row-marginal violation of the current (f, g) (its column marginals are exact after a g-update).  With tol > 0 and
 *            err <= tol S the iteration stops and keeps (f, g): f_new is not applied.  After max_iter iterations one more f evaluation
 *            gives the final err and is not applied either.  tol > 0 and a final err > tol S set LGN_SINKHORN_ITER; value and gradients
 *            are delivered all the same (the value is a valid lower bound of OT_eps).  tol = 0 always runs max_iter iterations and never
 *            sets the bit.  LGN_EMD_INVALID and LGN_EMD_EMPTY as in lgn_emd_pairs_f64: such a pair's outputs are NaN (iters 0).
 *   Outputs per pair: value E = <a, f> + <b, g>; f [n + 1], g [m + 1]; plan [n + 1][m + 1], P_ij = (a_i b_j / S) exp(F_i + G_j - Cs_ij)
 *            (0 where a_i b_j = 0); iters, the iterations applied; err.  Each but value and status is nullable.
 *   Gradients (g0 [B][n][3], g1 [B][m][3], each nullable; both null: the value only, the same bits): the envelope theorem at the
 *            returned state, which is the closed form of lgn_emd_grad_opts_f64 above with the flow replaced by P and (u, v) by (f, g):
 *            k_ij = P_ij beta theta_ij^(beta - 2) / R^2 where theta_ij > 0, else 0; the same position sums, the same s_ij under
 *            periodic_phi, the same fictitious-particle and norm forms of the weight terms.  P is never stored for this.
 *   debias   value = OT_eps(ev0, ev1) - OT_eps(ev0, ev0) / 2 - OT_eps(ev1, ev1) / 2: zero for equal events.  A self term is the same
 *            routine on the event's own staged (under norm: normalised) weights, without a fictitious particle, its reference
 *            measure a (x) a / S0; d / d a_i = f_i + g_i, its position terms count as row and as column, and its weight terms take the
 *            norm form like the cross term's.  The self term of a weightless event is 0.  status, iters, err, f, g and plan refer to
 *            the cross term; a self term that misses tol sets LGN_SINKHORN_ITER as well.
 *   lgn_sinkhorn_relative_f64: recons, target [B][N][4] Cartesian jets, staged into their relative-polar frames and the gradients
 *            carried back exactly as lgn_emd_relative_opts_f64 does it.  g_recons NULL: the value only (g_target must be NULL too).
 *   lgn_sinkhorn_lds_bytes(n, m): the dynamic LDS of ONE wavefront, the one place that counts it (-1 outside 1 .. LGN_EMD_NMAX): with
 *            R = max(n, m) + 1 and ld = R | 1 (odd: both walks of the matrix are free of bank conflicts)
 *               8 * (16 R + 8)      sixteen arrays of R doubles (weights, their logs, coordinates, potentials, gradients), two jets
 *               + 8 * R * ld        C / eps, when the sum stays within 64 KiB (max(n, m) <= 81); else the cost is recomputed from the
 *                                   staged coordinates in every sweep.  There is no global workspace.
 *            A workgroup holds min(4, 64 KiB / that) wavefronts, one pair each.
 *   Refused before any launch (negative return): null ev0, ev1, recons, target, opts, value or status; B < 1; n, m or N outside
 *   1 .. LGN_EMD_NMAX; R, beta or epsilon not a finite positive number; tol negative or not finite; max_iter < 1; g_target without
 *   g_recons.  Nothing is allocated, nothing waits on the host, no buffer is cleared by a memset, no atomics: capturable.
 *   Not offered: a LGN_LOSS_SINKHORN stage inside the whole-step calls; epsilon scaling (annealing); an all-pairs matrix form;
 *   unbalanced (KL-relaxed) marginals.
 *   Layout: sizeof(lgn_sinkhorn_opts) = 48; offsets base 0 (R 0, beta 8, norm 16, periodic_phi 20), epsilon 24, tol 32, max_iter 40,
 *   debias 44. */
#define LGN_SINKHORN_ITER 16
typedef struct lgn_sinkhorn_opts {
  lgn_emd_opts base;
  double epsilon, tol;
  int max_iter, debias;
} lgn_sinkhorn_opts;
long long lgn_sinkhorn_lds_bytes(int n, int m);
int lgn_sinkhorn_f64(const double* ev0, const double* ev1, int B, int n, int m, const lgn_sinkhorn_opts* opts, double* value,
                     double* g0 /*nullable*/, double* g1 /*nullable*/, double* f /*nullable*/, double* g /*nullable*/,
                     double* plan /*nullable*/, int* iters /*nullable*/, double* err /*nullable*/, int* status, void* stream);
int lgn_sinkhorn_relative_f64(const double* recons, const double* target, int B, int N, const lgn_sinkhorn_opts* opts, double* value,
                              double* g_recons /*nullable: value only*/, double* g_target /*nullable*/, int* iters /*nullable*/,
                              double* err /*nullable*/, int* status, void* stream);

/* ---- batched linear sum assignment: cost [B][n][n] -> col4row [B][n] int32, scipy.optimize.linear_sum_assignment(cost[b])[1] for
 * every b, ties broken as scipy breaks them (csrc/anomaly.hip).  One wavefront per problem; 1 <= n <= LGN_ANOMALY_NMAX.
 *   status [B] int32: 1 -- the matrix holds NaN or -inf; 256 -- infeasible (+inf entries); col4row is then -1. */
int lgn_linear_sum_assignment_f64(const double* cost, int B, int n, int* col4row, int* status, void* stream);

/* ---- reconstruction analysis: the numeric half of the reference's plot_p (utils/jet_analysis/utils.py, particle_recon_err.py,
 * jet_recon_err.py; csrc/analysis.hip).  target, recons [B][N][4] real Cartesian (E, px, py, pz), 1 <= N <= LGN_ANOMALY_NMAX.  One
 * wavefront per jet; nothing is allocated, nothing waits on the host: capturable into a graph.  B = 0 is no work.  Every output is the
 * caller's device memory; index 0 of a leading [2] is the target, 1 the reconstruction.
 *   part_polar    [2][B][N][3] (nullable) get_p_polar_tensor(p, eps = 1e-16): pt = sqrt(px^2 + py^2), eta = asinh(pz / (pt + eps)),
 *                 phi = atan2(py + eps, px)
 *   part_polarrel [2][B][N][3] (nullable) get_p_polarrel_tensor: with (Pt, Eta, Phi) the same formulas on the summed jet,
 *                 (pt / (Pt + eps), Eta - eta, ((Phi - phi + pi) mod 2 pi) - pi), the mod Python's.  Written only with abs_coord:
 *                 without it the relative-polar frame IS part_polar (plot_particle_recon_err).
 *   jet_cart      [2][B][4] (m, px, py, pz) of the summed jet (rows in order), m = sqrt|m^2| sign(m^2), m^2 = E^2 - px^2 - py^2 - pz^2
 *   jet_polar     [2][B][4] (m, pt, eta, phi) with phi = atan2(py, px): get_jet_feature_polar has no eps there
 *   jet_rel_err   [2][B][4] Cartesian then polar, as plot_jet_recon_err's call computes it: it hands (recons, target) to a lambda
 *                 written for (target, recons), so the value is (recons - target) / (recons + 1e-16)
 *   jet_keep      [2][B] uint8, filter_out_zeros' mask per coordinate system: all four target features non-zero
 *   rel_err       [3][B][N][3] (nullable; needs is_padded and status): Cartesian, polar, relative polar.
 *                 find_match: col0 = scipy's linear_sum_assignment(cost)[1] of cost[i][j] = |target3[i] - recons3[j]| on (px, py, pz),
 *                 col1 the same on the relative-polar frame; costs are exact Euclidean distances (a square root of an ordered sum of
 *                 squares), ties broken as scipy breaks them.
 *                    Cartesian       (recons3[col0] - target3) / target3: NO eps -- padded rows give +-inf or NaN, and is_padded is
 *                                    derived from those infinities
 *                    polar           (polar_r[col0] - polar_t) / (polar_t + 1e-16), on the Cartesian matching
 *                    relative polar  (polrel_r[col1] - polrel_t) / (polrel_t + 1e-16)
 *                 without find_match: the identity pairing and get_rel_err's (recons - target) / target, no eps, in all three frames.
 *   col4row       [2][B][N] int32 (nullable; only with rel_err): col0, col1 (the identity without find_match)
 *   is_padded     [B][N] uint8: any infinity among the row's three Cartesian relative errors
 *   status        [B] int32, as lgn_linear_sum_assignment_f64: 1 -- a cost of one of the two assignments is NaN (or -inf);
 *                 256 -- one is infeasible.  The jet's col4row is then -1, its rel_err NaN and its is_padded 0.
 * Replaces: get_p_polar_tensor, get_p_polarrel_tensor, get_jet_feature_cartesian / _polar, get_rel_err, get_rel_err_find_match,
 * filter_out_zeros and the jet relative errors of plot_jet_recon_err. */
int lgn_recon_analysis_f64(const double* target, const double* recons, int B, int N, int abs_coord, int find_match,
                           double* part_polar /*nullable*/, double* part_polarrel /*nullable*/, double* jet_cart, double* jet_polar,
                           double* jet_rel_err, uint8_t* jet_keep, double* rel_err /*nullable*/, int* col4row /*nullable*/,
                           uint8_t* is_padded, int* status, void* stream);

/* get_rel_err_find_match of particle_recon_err.py on frames the caller computed (each [B][N][3]): the same two assignments and three
 * gathers as above -- rel_err [3][B][N][3], col4row [2][B][N] (nullable), is_padded [B][N], status [B] -- and nothing else. */
int lgn_match_rel_err_f64(const double* target3, const double* recons3, const double* target_polar, const double* recons_polar,
                          const double* target_polarrel, const double* recons_polarrel, int B, int N, double* rel_err,
                          int* col4row /*nullable*/, uint8_t* is_padded, int* status, void* stream);

/* ---- batched histogram over explicit edges: counts[c][:] = np.histogram(x[keep, c], bins = edges[c][:n_edges[c]])[0] for the
 * columns c < cols <= ld of the device matrix x [rows][ld] (csrc/analysis.hip).  numpy's semantics exactly: bin i holds
 * edges[i] <= v < edges[i + 1], the last bin also v == edges[-1]; values outside the range, NaN and +-inf are counted nowhere.
 * Membership compares with the edge values themselves (bisection), never a scale-and-floor.  Per-workgroup LDS counters, one global
 * atomic per non-empty bin; the output is cleared by a kernel of the library: capturable, nothing allocated, no host wait.
 *   edges    [cols][max_edges] device, non-decreasing per column (not checked);  n_edges [cols] HOST ints, read during the call and
 *            checked before any launch: 2 <= n_edges[c] <= max_edges <= LGN_HIST_MAX_EDGES;  1 <= cols <= LGN_HIST_MAX_COLS
 *   keep     [rows] uint8, nullable: rows with keep == 0 are left out
 *   weights  [rows] fp64, nullable.  Without: counts [cols][max_bins] int64 (wcounts NULL), integer atomics -- exact and independent
 *            of the grid.  With: wcounts [cols][max_bins] fp64 (counts NULL), the sum of the weights per bin in no fixed order:
 *            within n 2^-52 sum|w| of any other order for a bin of n values.
 *   bins n_edges[c] - 1 .. max_bins - 1 of a column are written as 0.  rows = 0 clears the output. */
#define LGN_HIST_MAX_EDGES 1025
#define LGN_HIST_MAX_COLS 16
int lgn_histogram_f64(const double* x, long long rows, int ld, int cols, const double* edges, const int* n_edges /*host*/, int max_edges,
                      const uint8_t* keep /*nullable*/, const double* weights /*nullable*/, long long* counts, double* wcounts,
                      int max_bins, void* stream);

/* ---- reconstruction statistics: get_stats() and find_fwhm() of utils/jet_analysis/utils.py, the histogram edges plot_p draws over,
 * and the jet images of utils/jet_analysis/jet_images.py (csrc/stats.hip).  This block only ADDS functions: no struct and no
 * signature changed, so LGN_AMD_ABI_VERSION stays 19 (the rule above is about changes to what a caller already links against).
 *
 * lgn_column_stats_f64: for every column c < cols <= ld of the device matrix x [rows][ld], over the rows the mask keeps -- those
 * with (mask[r] != 0) == (mask_keep != 0); mask NULL keeps all.  With a_0 <= .. <= a_{n-1} the sorted kept values, stats[c][LGN_STAT_*]:
 *   quantiles q in {0.1, 0.25, 0.5, 0.75, 0.9} as np.quantile(a, q) (method "linear"): idx = (n - 1) q in fp64, lo = floor(idx),
 *       g = idx - lo, numpy's _lerp of a[lo], a[min(lo + 1, n - 1)]: a + (b - a) g, or b - (b - a) (1 - g) where g >= 0.5
 *   MEDIAN as np.median (the middle element or the mean of the two middle ones), FIRST_QUARTILE, THIRD_QUARTILE, Q10, Q90,
 *   IQR = q.75 - q.25, IDR = q.9 - q.1, MIN, MAX, ABS_MIN = min |a|,
 *   MAD = scipy.stats.median_abs_deviation(a): the median of |a - median| (selected on the sorted column, no second sort)
 *   MEAN, STD_DEV (np.std, ddof 0), SKEW = m3 / m2^1.5 and KURTOSIS = m4 / m2^2 - 3 (scipy.stats.skew / kurtosis defaults: biased,
 *       Fisher) from the two-pass central moments about MEAN, ABS_MEAN = mean |a|
 *   ABS_MEAN_WITHIN_IQR = mean of |a| over the values with |a| < IQR (this call's own IQR), 1e32 when there is none; _IDR likewise
 *   FWHM is written as NaN: it is lgn_hist_fwhm_f64's, whose slot it keeps so that the positions are the reference's dict order.
 * edges[c][:] = np.linspace(median - alpha IQR, median + alpha IQR, num_edges): start + i step with step = (stop - start) /
 * (num_edges - 1), rounded one operation at a time, the last element stop itself.  kept[c] = n.  status[c]: LGN_STATS_EMPTY (n = 0)
 * or LGN_STATS_NONFINITE (a kept value is NaN or +-inf): the column's statistics and edges are then NaN, the other columns
 * unaffected.  A constant column is no error: IQR = 0, m2 = 0, SKEW and KURTOSIS the NaN of 0 / 0.  +-0.0 sort in either order.
 * Every sum is taken in one fixed order that depends on the multiset of kept values alone: the same bits on every run, for every
 * grid, row order and column count; no floating-point atomics.  Nothing is allocated, nothing waits on the host: capturable.
 * Refused before any launch (negative return): null pointers (x may be NULL with rows = 0, edges with num_edges = 0), rows < 0 or
 * >= 2^31, cols outside 1 .. LGN_STATS_MAX_COLS, ld < cols, num_edges = 1 or > LGN_HIST_MAX_EDGES, alpha not finite, a workspace
 * shorter than lgn_column_stats_workspace_bytes(rows, cols) or not 8-byte aligned.  rows = 0: every column EMPTY. */
#define LGN_STATS_TILE 2048
#define LGN_STATS_MAX_COLS 16
#define LGN_STATS_EMPTY 1
#define LGN_STATS_NONFINITE 2
#define LGN_STAT_MEDIAN 0
#define LGN_STAT_IQR 1
#define LGN_STAT_FIRST_QUARTILE 2
#define LGN_STAT_THIRD_QUARTILE 3
#define LGN_STAT_IDR 4
#define LGN_STAT_MAD 5
#define LGN_STAT_MEAN 6
#define LGN_STAT_MAX 7
#define LGN_STAT_MIN 8
#define LGN_STAT_ABS_MIN 9
#define LGN_STAT_STD_DEV 10
#define LGN_STAT_SKEW 11
#define LGN_STAT_KURTOSIS 12
#define LGN_STAT_FWHM 13
#define LGN_STAT_ABS_MEAN 14
#define LGN_STAT_ABS_MEAN_WITHIN_IQR 15
#define LGN_STAT_ABS_MEAN_WITHIN_IDR 16
#define LGN_STAT_Q10 17
#define LGN_STAT_Q90 18
#define LGN_STATS_COUNT 19
long long lgn_column_stats_workspace_bytes(long long rows, int cols);
int lgn_column_stats_f64(const double* x, long long rows, int ld, int cols, const uint8_t* mask /*nullable*/, int mask_keep,
                         double alpha, int num_edges, double* stats /* [cols][LGN_STATS_COUNT] */,
                         double* edges /* [cols][num_edges], nullable with num_edges = 0 */, long long* kept /* [cols] */,
                         int* status /* [cols] */, void* workspace, long long workspace_bytes, void* stream);

/* find_fwhm (utils.py:352-362) on the output layout of lgn_histogram_f64: i = argmax(counts) (the first maximum), h = counts[i] / 2,
 * j = argmin |counts - h| (the first minimum), fwhm[c] = 2 |edges[i] - edges[j]|: integer logic and one subtraction, bitwise the
 * reference's given the same counts and edges.  n_edges [cols] HOST ints as lgn_histogram_f64 takes them; 1 <= cols <=
 * LGN_HIST_MAX_COLS.  get_stats is then lgn_column_stats_f64 -> lgn_histogram_f64 -> lgn_hist_fwhm_f64 with no host round trip. */
int lgn_hist_fwhm_f64(const long long* counts, int max_bins, const double* edges, int max_edges, const int* n_edges /*host*/, int cols,
                      double* fwhm /* [cols] */, void* stream);

/* pixelate (jet_images.py:193-226) of every jet, the first first_n images (get_n_jet_images) and the mean image over all B jets
 * (get_average_jet_image).  jets [B][N][3] (pt, eta, phi); bins = np.linspace(-maxR, maxR, npix + 1); a particle goes to the pixel
 * [phi_bin][eta_bin] with bins[i] <= v < bins[i + 1] (np.digitize - 1: a value equal to maxR, outside the range or NaN goes nowhere,
 * unlike np.histogram), decided by comparing with the edge values themselves; image[phi_bin][eta_bin] += pt in particle order.
 *   mode 0  jets are relative already (abs_coord = False)
 *   mode 1  each jet is first taken into its own frame (get_jet_rel + normalize)
 *   mode 2  into the frame of frame_jets [B][N][3] (the *_same_norm pair: once target with itself, once recons with the target)
 * The frame is that of the summed massless particles: Px = sum pt cos(phi), Py = sum pt sin(phi), Pz = sum pt sinh(eta) in particle
 * order, Pt = hypot(Px, Py), Eta = asinh(Pz / Pt), Phi = atan2(Py, Px); then pt / Pt, eta - Eta, ((phi - Phi + pi) mod 2 pi) - pi with
 * Python's mod.  normalize's escape is kept: when np.isclose(Pt, 0) (|Pt| <= 1e-8) holds for EVERY jet of the call nothing is
 * normalised (a device-side reduction, no host read).  The reference does this sum with awkward / coffea; the formula written here
 * is the specification of modes 1 and 2, and no test value of theirs was produced by those packages.
 * images [min(first_n, B)][npix][npix] (nullable with first_n = 0), average [npix][npix].  One wavefront per jet, image in LDS; the
 * average is a fixed-order two-stage sum (LGN_JET_IMAGE_PARTS partial images in the workspace, added in order): no floating-point
 * atomics, the same bits on every run.  Refused: null pointers, B < 1, N outside 1 .. LGN_ANOMALY_NMAX, npix outside
 * 1 .. LGN_JET_IMAGE_MAX_NPIX, maxR not finite and positive, mode outside 0 .. 2, first_n < 0, a workspace shorter than
 * lgn_jet_images_workspace_bytes(B, npix) or not 8-byte aligned. */
#define LGN_JET_IMAGE_MAX_NPIX 64
#define LGN_JET_IMAGE_PARTS 512
long long lgn_jet_images_workspace_bytes(int B, int npix);
int lgn_jet_images_f64(const double* jets, const double* frame_jets /*nullable*/, int B, int N, int mode, int npix, double maxR,
                       int first_n, double* images /*nullable*/, double* average, void* workspace, long long workspace_bytes,
                       void* stream);

/* ---- the equivariance test (lgn/models/autotest/lgn_tests.py:82-269 with rotate_rep of lgn/g_lib/rotations.py:7-51 and get_node_dev
 * of autotest/utils.py:22-45; host side lgn/equivariance.py) -------------------------------------------------------------------------
 * lgn_transform_jets_f64: the T transformed copies of a batch, out[t][b][n][a] = sum_b p4[b][m][b] R[t][b][a] with m = perm[b][n] (n
 * without perm), each component the four-term sum ((p0 R0a + p1 R1a) + p2 R2a) + p3 R3a of the reference's einsum("...b,ba->...a").
 *   p4 [B][N][4], R [T][4][4], out [T][B][N][4]; perm [B][N] int32, nullable; scalars [B][N][K] -> scalars_out [T][B][N][K] gathered by
 *   the same permutation, no matrix (both NULL with K = 0).  Boosts, rotations, and with T = 1, R = identity the permuted batch of
 *   permutation_invariance_test (then the gathered input, bit for bit).  Refused: null pointers, T outside 1 .. 65535, B or N < 1,
 *   K < 0, B * N >= 2^31.
 *
 * lgn_rep_deviation_f64: every transformation, layer and irrep of one kind in one call.  Part p (one irrep of one GVec, parts <=
 * LGN_EQUI_MAX_PARTS) is
 *   a[p] [2][T * B][N][C][d]  features of the transformed input, jet t * B + b (plane 0 real, plane 1 imaginary: the entries of
 *                             `nodes_all`)
 *   b[p] [2][B][N][C][d]      features of the untransformed input
 *   D[p] [T][2][d][d]         planar representation matrix of the irrep per transformation (lorentz_D), d in {1, 3, 4, 9}
 * with N[p], C[p], d[p]; a, b, D, N, C, d are HOST arrays of `parts` entries read during the call, T and B are common.  Per row of d
 * complex numbers b' = (b_r D_r + b_i D_i, -b_r D_i + b_i D_r) -- rotate_rep's convention, z times conj(D) -- is formed on the fly (D[t]
 * in LDS, b' never stored), and over the whole (2, B, N, C, d) block of each (p, t)
 *   stats[p][t] = { sum(a - b'), sum(b'), max|a - b'|, max|b'|, max|(a - b') / (b' + 1e-16)| }
 * from which the host forms get_node_dev's metrics: mean |s0 / n / (s1 / n + eps)|, max s4, and the max-norm s2 / (s3 + eps).
 * perm [B][N] int32 (nullable; then every part has the same N) reads b at particle perm[b][n]: with D the identity the permutation
 * "equivariance" column.  An entry of perm outside [0, N) forms no address; its rows count as NaN (lgn_transform_jets_f64 writes NaN
 * rows).  A workgroup reduces LGN_EQUI_TILE rows of one (p, t); its partial row goes to the workspace and a second kernel adds the
 * partial rows in a fixed order: no floating-point atomics, the same bits on every run.  The maxima keep a NaN as torch.max does, so
 * a NaN anywhere in a block makes its five numbers NaN.  Nothing is allocated and nothing waits on the host.  Refused: null pointers,
 * parts outside 1 .. LGN_EQUI_MAX_PARTS, d outside {1, 3, 4, 9}, T outside 1 .. 65535, B, N or C < 1, B * N * C >= 2^31 / 9, a
 * workspace shorter than lgn_rep_deviation_workspace_bytes says or not 8-byte aligned. */
#define LGN_EQUI_TILE 256
#define LGN_EQUI_MAX_PARTS 64
int lgn_transform_jets_f64(const double* p4, const double* R, const int* perm /*nullable*/, const double* scalars /*nullable*/, int T,
                           int B, int N, int K, double* out, double* scalars_out /*nullable*/, void* stream);
long long lgn_rep_deviation_workspace_bytes(int parts, int T, int B, const int* N /*host*/, const int* C /*host*/,
                                            const int* d /*host*/);
int lgn_rep_deviation_f64(int parts, int T, int B, const double* const* a /*host*/, const double* const* b /*host*/,
                          const double* const* D /*host*/, const int* N /*host*/, const int* C /*host*/, const int* d /*host*/,
                          const int* perm /*nullable*/, double* stats /* [parts][T][5] */, void* workspace, long long workspace_bytes,
                          void* stream);

/* ---- the assignment loss on its own (module API: lgn/losses.py HungarianMSELoss, the drop-in of the reference's class; the device
 * code of the whole-step calls' loss stage -- lgn_loss_desc above -- without the output mix): x, y [B][N][4] real 4-vectors ->
 * loss_part [B], gx [B][N][4] = d (sum of loss_part) / d x. */
int lgn_hungarian_mse_f64(int B, int N, const double* x, const double* y, int kind, int abs_coord, int polar_coord, double scale,
                          double* loss_part, double* gx, int* assignment /* [B][N], nullable */, int* status /* [B], nullable */,
                          void* stream);
/* Plan-time fit query: bytes of LDS of the step's assignment-loss stage at N particles and C channels of the last decoder level. */
long long lgn_assign_loss_lds_bytes(int N, int C);

/* ---- staging of a batch with the reference's --normalize / --normalize-method (utils/train.py:281-297, utils/normalize_p4.py) ------
 * One launch does what a step's load_batch does: per jet the factor, target = p4 / factor (the UNscaled normalised batch the loss
 * compares with), p4_in = target * scale (the encoder's input), the node mask, and with jet_features the jet node and the input
 * scalars of Encoder._prepare_input.  One wavefront per jet; nothing is allocated, nothing waits on the host.  Any N >= 1.
 *   method       LGN_NORM_NONE (factor 1), COMPONENT_MAX (max_i |p_i^mu| + 1e-16 per component), OVERALL_MAX (max over (i, mu) + 1e-16),
 *                JET_E (sum_i E_i + 1e-16, summed in a fixed order).  The max keeps a NaN, as torch.amax does: a NaN or inf poisons
 *                its own jet only.  The 1e-16 is added, not clamped: an all-zero jet has factor 1e-16 and stays zero.
 *   p4           [B][N][4], 16-byte aligned;  labels [B][N] uint8, nullable: without it mask = target[..][0] != 0 (after the division)
 *   scalars      [B][N + jet_features][K] data['scalars'], NULL when K = 0
 *   p4_in        [B_pad][N + jet_features][4]; with jet_features row N is the jet node sum_i p4_in[i] (row order), its mask 1
 *   target       [B_pad][N][4]; may BE p4_in when scale = 1 and there is no jet node
 *   mask         [B_pad][N + jet_features] uint8
 *   in_scalars   [B_pad][N + jet_features][jet_features + K], required when jet_features or K > 0: column 0 = normsq4(sum over all
 *                N + 1 nodes) for every node (lgn_encoder.py:377-390), then the K columns of `scalars`
 *   factor       [B_pad][4]: always four doubles per jet (the scalar methods write theirs four times)
 * Jets B .. B_pad - 1 (the all-masked padding jets of a short batch) are written as zeros in every output. */
#define LGN_NORM_NONE 0
#define LGN_NORM_COMPONENT_MAX 1
#define LGN_NORM_OVERALL_MAX 2
#define LGN_NORM_JET_E 3
int lgn_stage_batch_f64(const double* p4, const uint8_t* labels /*nullable*/, const double* scalars /*nullable*/, int B, int B_pad, int N,
                        int method, double scale, int jet_features, int K, double* p4_in, double* target, uint8_t* mask,
                        double* in_scalars /*nullable*/, double* factor, void* stream);
/* out0[b][i][mu] = x0[b][i][mu] * factor[b][mu], and the same for x1 -> out1 (both NULL: one tensor only) in the same launch: what
 * validate() collects under --normalize (p4_recons * norm_factor, p4_target * norm_factor).  x, out [B][N][4]; factor [B][4] as
 * lgn_stage_batch_f64 writes it; all 16-byte aligned.  Static pointers: capturable behind lgn_step_eval_f64. */
int lgn_denormalize_f64(const double* x0, const double* x1 /*nullable*/, const double* factor, int B, int N, double* out0,
                        double* out1 /*nullable*/, void* stream);

/* ---- device-resident epochs: an epoch as ceil(count / B) replays of ONE linear graph [gather staging | step | collect] -------------
 * The dataset stays on the device, the epoch's order is one int32 index tensor, and what tells one step from the next -- the batch
 * cursor, the loss sum, the step count -- lives in device memory the kernels read and write: no argument changes between replays.
 *   cursor  [2] long long: [0] batches done in this epoch, [1] the collect kernel's arrival ticket (0 between launches)
 *   epoch   [2] double:    [0] sum of the steps' losses, one fp64 add per step in step order (the sum a host loop makes of
 *                          loss.item()), [1] steps counted
 *   status  [1] int:       LGN_EPOCH_BAD_INDEX once an index outside [0, M) was met (plain store)
 * lgn_epoch_reset clears all three (one single-thread kernel: capturable, no memset node).
 *
 * lgn_stage_gather_f64 is lgn_stage_batch_f64 with the jet of batch row b taken from a resident dataset: jet
 * index[cursor * B_pad + b] of p4 [M][N][4], labels [M][N] (nullable), scalars [M][N + jet_features][K] (NULL when K = 0).  Row b is a
 * real jet when cursor * B_pad + b < count, else a padding jet (zeros in every output); an index outside [0, M) forms no address, its
 * row is a padding jet and status says so.  Everything else -- the four methods, scale, the aliased target, jet node, in_scalars,
 * factor, alignment -- as lgn_stage_batch_f64, and the outputs are bit for bit what that call writes for p4[index[...]].
 *
 * lgn_epoch_collect_f64 runs once behind the step: with n_valid = min(B, count - cursor * B) it copies rows b < n_valid of each of the
 * n <= LGN_EPOCH_MAX_COLLECT sources src[k] [B][row_doubles[k]] to dst[k] [count][row_doubles[k]] at jet cursor * B + b, adds *loss to
 * epoch[0], counts the step and -- its last act, one thread -- advances the cursor.  src / dst / row_doubles are HOST arrays read during
 * the call (n = 0: all three may be NULL).  Only tensors whose batch axis leads can be collected (the latent: lgn_epoch_collect_planes_f64
 * below). */
#define LGN_EPOCH_MAX_COLLECT 4
#define LGN_EPOCH_BAD_INDEX 1
int lgn_stage_gather_f64(const double* p4, const uint8_t* labels /*nullable*/, const double* scalars /*nullable*/, long long M,
                         const int* index, long long count, const long long* cursor, int B_pad, int N, int method, double scale,
                         int jet_features, int K, double* p4_in, double* target, uint8_t* mask, double* in_scalars /*nullable*/,
                         double* factor, int* status, void* stream);
int lgn_epoch_collect_f64(const double* loss, double* epoch, long long* cursor, long long count, int B, int n,
                          const double* const* src /*host*/, double* const* dst /*host*/, const int* row_doubles /*host*/, void* stream);
int lgn_epoch_reset(long long* cursor, double* epoch, int* status, void* stream);
/* The same two calls for a SECOND plan of another batch size replayed behind the first in the same epoch -- the short last batch of a
 * training epoch: B jets per replay of the first plan, then r = count mod B jets in one replay of a plan built for r -- and for
 * tensors whose batch axis is the second one (the latent, [2][B][...]).  Both add functions only (ABI 19 stands).
 *
 * lgn_stage_gather_at_f64 is lgn_stage_gather_f64 with row b taken from index[base + cursor * B_pad + b], 0 <= base <= count.  With
 * `full` batches of B done, the cursor holds `full`, and a plan of B_pad = r jets reads from position full * B with
 * base = full * (B - r).  base = 0 writes the bits of lgn_stage_gather_f64.
 *
 * lgn_epoch_collect_planes_f64 is lgn_epoch_collect_f64 with a per-tensor planes[k] >= 1 and the same base: source k is
 * [planes[k]][B][row_doubles[k]], its destination [planes[k]][count][row_doubles[k]]; with row0 = base + cursor * B and
 * n_valid = min(B, count - row0), every plane is one contiguous run of n_valid * row_doubles[k] doubles written at row row0 of its
 * plane (16-byte vectors where both ends are aligned).  Loss sum, step count, ticket and cursor as lgn_epoch_collect_f64; planes is
 * a HOST array like the other three.  planes = 1 everywhere and base = 0 write the bits of lgn_epoch_collect_f64. */
int lgn_stage_gather_at_f64(const double* p4, const uint8_t* labels /*nullable*/, const double* scalars /*nullable*/, long long M,
                            const int* index, long long count, long long base, const long long* cursor, int B_pad, int N, int method,
                            double scale, int jet_features, int K, double* p4_in, double* target, uint8_t* mask,
                            double* in_scalars /*nullable*/, double* factor, int* status, void* stream);
int lgn_epoch_collect_planes_f64(const double* loss, double* epoch, long long* cursor, long long count, long long base, int B, int n,
                                 const double* const* src /*host*/, double* const* dst /*host*/, const int* row_doubles /*host*/,
                                 const int* planes /*host*/, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* LGN_AMD_H */
