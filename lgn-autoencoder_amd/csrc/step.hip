// lgn-autoencoder_amd/csrc/step.hip -- one training step of the LGN autoencoder as a single native call.
//
// Counterpart of the inner loop of the reference's utils/train.py:283-343 (encoder -> decoder ->
// get_real -> Chamfer [+ jet-feature MSE] -> backward) for the maxdim=2 path: ~80 kernel launches enqueued back to back
// on the caller's stream, no host synchronisation, every buffer caller-owned and static -> the call can be
// captured into a HIP graph (the Python harness does so) and replayed.  Parameter gradients are written
// straight into the caller's flat gradient buffer at the same offsets as the parameters.
//
// The file, top to bottom: shared plumbing -- one maxdim-2 network (levels_fwd / levels_bwd, encoder_fwd / encoder_bwd, decoder_fwd /
// decoder_bwd) -- one table-driven network (the gen_* counterparts) -- the per-network carves -- the training steps -- the evaluation
// step; then the C calls in the same order.  Each workspace layout is one carve, each end-stage sequence one function.
#include <stdlib.h>

#include <algorithm>
#include <vector>

#include "net.hpp"
#include "../../include/lgn_amd.h"

namespace lgn {
namespace {

// ---------------------------------------------------------------------------------------------------------
// shared plumbing
// ---------------------------------------------------------------------------------------------------------
inline size_t r16(size_t n) { return (n + 15) & ~size_t(15); }     // 128-byte granules: what a take of n doubles occupies

struct Bump {                       // workspace carving (also used for the size query with base == nullptr)
  double* base;
  size_t off = 0;
  double* here() const { return base ? base + off : nullptr; }       // where the next take starts
  double* take(size_t n) {
    double* p = here();
    off += r16(n);
    return p;
  }
};

// deferred reductions: producers register their column ranges, one or two launches at the end reduce everything
struct Deferred {
  std::vector<RedSeg<double>> segs;
  double* parts;
  size_t off = 0, cap;
  Deferred(double* rows, size_t doubles) : parts(rows), cap(doubles) {}       // opened on a carve's partial-row region
  // nullptr when the slice does not fit: callers test it (DQ_TAKE) BEFORE enqueuing the kernel that would write there --
  // the capacity mirrors the take sequence (net_parts / gen_net_parts), a disagreement must not reach the device
  double* take(size_t n) {
    n = r16(n);
    if (off + n > cap) return nullptr;
    double* p = parts + off;
    off += n;
    return p;
  }
  void add(const double* part, int rows, int stride, int col0, int n, double* out) {
    if (n > 0) segs.push_back(RedSeg<double>{part, rows, stride, col0, n, out});
  }
  int flush(hipStream_t st) {
    for (size_t i = 0; i < segs.size(); i += RED_MAX_SEG) {
      RedJob<double> job{};
      for (size_t k = i; k < segs.size() && k < i + RED_MAX_SEG; ++k) job.seg[job.nseg++] = segs[k];
      if (int rc = reduce_segments<double>(job, st)) return rc;
    }
    segs.clear();
    return 0;
  }
};

#define DQ_NEW(var, n) double* var = nullptr; DQ_TAKE(var, n)
#define DQ_TAKE(lhs, n)                                                                                           \
  lhs = dq.take(n);                                                                                             \
  LGN_CHECK_ARG((lhs) != nullptr, "partial-row workspace overflow: %zu + %zu doubles > capacity %zu (carve / take mismatch)", \
                dq.off, (size_t)(n), dq.cap)
#define LGN_TRY(expr)            \
  do {                           \
    int rc_ = (expr);            \
    if (rc_ != 0) return rc_;    \
  } while (0)

// The end of a backward whose gradients go on to somebody else (the all-reduce of a data-parallel step, autograd under the module
// API): every deferred reduction and the radial finalisation as ONE launch (step_tail.hip, reduce_only) -- `counters`: 4 words of the
// caller's zero block -- or, when that form does not fit (or with LGN_NET_SPLIT_TAIL), as reduce_segments + rad_finalize_batch.
int finish_reductions(Deferred& dq, const RadFinJob& fin, double* grads, long long n_params, double* counters, int flags, hipStream_t st) {
  if (counters && !(flags & LGN_NET_SPLIT_TAIL)) {
    StepTailArgs ro{};
    ro.g = grads;
    ro.n = (long)n_params;
    ro.reduce_only = 1;
    ro.counters = reinterpret_cast<unsigned long long*>(counters);
    const int rc = step_tail(dq.segs, fin, ro, st);
    if (rc == 0) { dq.segs.clear(); return 0; }
    if (rc != -2) return rc;
  }
  if (int rc = dq.flush(st)) return rc;
  return rad_finalize_batch(fin, st);
}

// L1 [+ L2] + optimiser + loss assembly as a launch of its own: l1_adam_kernel of the tail's form (net_kernels.hip)
int finalize_tail(const StepTailArgs& t, hipStream_t st) {
  if (t.opt_form) return finalize_step_opt(t, st);
  return finalize_step(t.w, t.g, t.n, t.loss_part, t.nB, t.lambda, t.m, t.v, t.step_dev, t.lr, t.beta1, t.beta2, t.eps, t.do_adam,
                       t.loss_out, st);
}

// The end of a whole step.  With `tail` (single process: nothing sits between the gradients and the optimiser) the deferred
// reductions, the radial finalisation, L1 + Adam and the loss assembly are ONE launch (step_tail.hip); where that form does not fit
// (-2), or with LGN_NET_SPLIT_TAIL, finish_reductions and then finalize_step.  Without `tail` (data-parallel step: the all-reduce
// follows) finish_reductions alone, in one launch on `counters` where the caller has them.
int end_step(Deferred& dq, const RadFinJob& fin, double* grads, long long n_params, double* counters, int flags, const StepTailArgs* tail,
             hipStream_t st) {
  if (tail && !(flags & LGN_NET_SPLIT_TAIL)) {
    const int rc = step_tail(dq.segs, fin, *tail, st);
    if (rc != -2) return rc;
  }
  if (int rc = finish_reductions(dq, fin, grads, n_params, tail ? nullptr : counters, flags, st)) return rc;
  if (!tail) return 0;
  return finalize_tail(*tail, st);
}

inline int in_K(const lgn_net_desc& d) { return d.n_in_scalars > 1 ? d.n_in_scalars : 1; }      // encoder input scalars per node

// decoder node count of a whole step: its own (jet_features gives the encoder one node more than the decoder reconstructs), or N
inline int dec_nodes(const lgn_net_desc& d) { return d.dec_N > 0 ? d.dec_N : d.N; }
// the step takes the two-kernel junction and the riding input stage only when both networks work on the same nodes and the mass is
// the only input scalar; otherwise the four end stages are launches of their own
inline bool step_is_split(const lgn_net_desc& d) { return dec_nodes(d) != d.N || d.n_in_scalars > 1; }
// the decoder's view of a whole step's descriptor: the level sequencers, the carves and the layout predicates of a network read B, N,
// flags and the MLP shape off the descriptor they are given -- the decoder's carries its own node count
inline lgn_net_desc dec_view(const lgn_net_desc& d) {
  lgn_net_desc dd = d;
  dd.N = dec_nodes(d);
  return dd;
}
// latent vectors per jet the decoder's input stage reads: its own tau_v_in, or the encoder's pooled ones
inline int dec_tin(const lgn_net_desc& d) { return d.tau_v_in > 0 ? d.tau_v_in : pool_blocks(d.latent_pool) * d.tau_v; }

// buffer sizes every carve states through these: the encoder's pooled latent scalars [2][B][P Ts] and vectors [2][B][P Tv][4], and
// the pooling indices of its latent stage (ints, two to a double)
inline size_t lat_s_doubles(const lgn_net_desc& d) { return (size_t)2 * d.B * pool_blocks(d.latent_pool) * d.tau_s; }
inline size_t lat_v_doubles(const lgn_net_desc& d) { return (size_t)2 * d.B * pool_blocks(d.latent_pool) * d.tau_v * 4; }
inline size_t pool_idx_doubles(const lgn_net_desc& d) { return ((size_t)d.B * 2 * (d.tau_s + d.tau_v) * 2 + 1) / 2 + 8; }

struct Slots {                      // canonical parameter slot order shared with lgn/step.py
  int L, nlin;
  int in0(bool dec) const { return dec ? 2 : 0; }
  int rad(bool dec, int l, int k) const { return in0(dec) + 2 + 7 * l + k; }
  int mix(bool dec, int l, int k) const { return in0(dec) + 2 + 7 * L + 2 * l + k; }
  int mlp(bool dec, int l, int k) const { return in0(dec) + 2 + 9 * L + 2 * nlin * l + k; }
  int out0(bool dec) const { return in0(dec) + 2 + 9 * L + 2 * nlin * L; }
  int count(bool dec) const { return out0(dec) + 2; }
};

// Partial-row layout of an end stage: its launch writes one row of `width` doubles per workgroup; columns [col, col + n) of the rows
// reduce into the gradient of parameter slot `slot`.  Each layout below is stated here only: the sequencers register their
// reductions with add(), the workspace carves size the rows with width.
struct RowLayout {
  int width, nseg, col[3], n[3], slot[3];
  void add(Deferred& dq, const double* part, int rows, double* G, const int64_t* off) const {
    for (int i = 0; i < nseg; ++i) dq.add(part, rows, width, col[i], n[i], G + off[slot[i]]);
  }
};
// encoder latent stage (enc_latent_bwd / junction_bwd): dWl0 [2][Ts][KL] | dWl1 [2][Tv][KL]
RowLayout enc_latent_rows(const lgn_net_desc& d, int N, int CL) {
  const int KL = pool_mix_in(d.latent_pool, N, CL), o = Slots{d.n_levels, d.mlp_nlin}.out0(false);
  return {2 * (d.tau_s + d.tau_v) * KL, 2, {0, 2 * d.tau_s * KL}, {2 * d.tau_s * KL, 2 * d.tau_v * KL}, {o, o + 1}};
}
// encoder input stage with K scalars (enc_input_bwd, or riding on the first level's backward with K = 1): dW00 [2][C0][K] | dW11 [2][C0]
RowLayout enc_input_rows(int K, int C0) { return {(2 * K + 2) * C0, 2, {0, 2 * C0 * K}, {2 * C0 * K, 2 * C0}, {0, 1}}; }
// decoder input stage (dec_input_bwd / junction_bwd): dW00 [2][C0] | dW11 [2][C0] | dWg1 [2][N][Tin]
RowLayout dec_input_rows(int C0, int N, int Tin) {
  return {4 * C0 + 2 * N * Tin, 3, {0, 2 * C0, 4 * C0}, {2 * C0, 2 * C0, 2 * N * Tin}, {2, 3, 1}};
}
// decoder output stage (dec_output_bwd / dec_output_loss): dWo1 [2][CL]
RowLayout dec_output_rows(const lgn_net_desc& d, int CL) {
  return {2 * CL, 1, {0}, {2 * CL}, {Slots{d.n_levels, d.mlp_nlin}.out0(true) + 1}};
}

// partial rows of a network's two end stages on N nodes; in_rows: rows of the encoder's input stage
size_t end_parts(const lgn_net_desc& d, bool dec, int N, int in_rows) {
  const int* ch = dec ? d.dec_channels : d.enc_channels;
  const int L = d.n_levels;
  if (dec) return r16((size_t)d.B * dec_output_rows(d, ch[L]).width) + r16((size_t)d.B * dec_input_rows(ch[0], N, dec_tin(d)).width);
  return r16((size_t)d.B * enc_latent_rows(d, N, ch[L]).width) + r16((size_t)in_rows * enc_input_rows(in_K(d), ch[0]).width);
}

// Zero-fill of up to three ranges in ONE launch of our own.  NOT hipMemsetAsync: under stream capture (ROCm 7.2, torch 2.10) the
// memset node of a replayed graph fills its range with a stale 16-byte pattern -- two pointer-like words, i.e. denormals ~7e-310 --
// from the second replay on (tools/graph_memset_check.py).  As gradients of dead parameters and "zero" upstream gradients that
// went unnoticed numerically; as counters it does not.
struct ZeroJob { double* p[3]; size_t n[3]; };
__global__ __launch_bounds__(BLOCK) void zero_ranges_kernel(ZeroJob job) {
  const size_t stride = (size_t)gridDim.x * BLOCK;
#pragma unroll
  for (int q = 0; q < 3; ++q)
    for (size_t i = (size_t)blockIdx.x * BLOCK + threadIdx.x; i < job.n[q]; i += stride) job.p[q][i] = 0.0;
}
int zero_ranges(double* a, size_t na, double* b, size_t nb, double* c, size_t nc, hipStream_t st) {
  const ZeroJob job{{a, b, c}, {a ? na : 0, b ? nb : 0, c ? nc : 0}};
  const size_t most = std::max(job.n[0], std::max(job.n[1], job.n[2]));
  if (!most) return 0;
  const int blocks = (int)std::min<size_t>((most + BLOCK - 1) / BLOCK, 1024);
  hipLaunchKernelGGL(zero_ranges_kernel, dim3(blocks), dim3(BLOCK), 0, st, job);
  LGN_CHECK_LAUNCH();
  return 0;
}
// grads [n] and the zero block [nz]: one range when the caller laid them out back to back (lgn/ops.py does)
int zero_grads_and_block(double* grads, size_t n, double* zeros, size_t nz, hipStream_t st) {
  if (zeros >= grads + n && zeros <= grads + n + 16) return zero_ranges(grads, (size_t)((zeros + nz) - grads), nullptr, 0, nullptr, 0, st);
  return zero_ranges(grads, n, zeros, nz, nullptr, 0, st);
}

int check_desc(const lgn_net_desc* d) {
  LGN_CHECK_ARG(d, "step: null descriptor");
  LGN_CHECK_ARG(d->B > 0 && d->N > 0, "step: empty batch (B=%d N=%d)", d->B, d->N);
  LGN_CHECK_ARG(d->n_levels >= 1 && d->n_levels <= 4, "step: n_levels=%d unsupported (1..4)", d->n_levels);
  LGN_CHECK_ARG(d->mlp_nlin >= 4 && d->mlp_nlin <= 7, "step: mlp_depth must be 3 .. 6 (4 .. 7 Linear layers), got %d layers", d->mlp_nlin);
  LGN_CHECK_ARG(d->tau_s >= 1 && d->tau_v >= 1 && d->tau_v_in >= 0, "step: latent multiplicities must be positive");
  LGN_CHECK_ARG(d->n_in_scalars >= 0 && d->n_in_scalars <= 8, "step: n_in_scalars=%d unsupported (0..8)", d->n_in_scalars);
  LGN_CHECK_ARG(pool_valid(d->latent_pool), "step: latent_pool=%d is not an LGN_POOL(...) code", d->latent_pool);
  for (int l = 0; l <= d->n_levels; ++l)
    LGN_CHECK_ARG(d->enc_channels[l] >= 1 && d->enc_channels[l] <= 8 && d->dec_channels[l] >= 1 && d->dec_channels[l] <= 8,
                  "step: channel counts must be in 1..8");
  LGN_CHECK_ARG(d->get_real >= LGN_REAL_SUM && d->get_real <= LGN_REAL_NORM, "step: get_real=%d is not an LGN_REAL_* code", d->get_real);
  LGN_CHECK_ARG(d->jet_loss_scale >= 0.0, "step: jet_loss_scale=%g must be >= 0", d->jet_loss_scale);
  LGN_CHECK_ARG(d->dec_N >= 0, "step: dec_N=%d must be >= 0", d->dec_N);
  if (d->dec_N > 0) {        // the whole step's decoder end stages are one workgroup per jet of dec_N particles
    const size_t need = decoder_end_lds_bytes(d->dec_N, d->dec_channels[0], dec_tin(*d), d->dec_channels[d->n_levels]);
    LGN_CHECK_ARG(need <= LGN_LDS_LIMIT, "step: dec_N=%d: the decoder end stages need %zu B of LDS (> %d)", d->dec_N, need, LGN_LDS_LIMIT);
  }
  return 0;
}

// a whole step's decoder consumes the encoder's pooled latent vectors
int check_latent_match(const lgn_net_desc& d) {
  const int Tin = pool_blocks(d.latent_pool) * d.tau_v;
  LGN_CHECK_ARG(d.tau_v_in == 0 || d.tau_v_in == Tin, "step: the decoder must consume the encoder's %d pooled latent vectors", Tin);
  return 0;
}

int check_mlp_contiguous(const lgn_net_desc& d, bool dec, const int64_t* off) {
  const Slots S{d.n_levels, d.mlp_nlin};
  const int* ch = dec ? d.dec_channels : d.enc_channels;
  for (int l = 0; l < d.n_levels; ++l) {
    const int D = 2 * ch[l + 1], H = d.mlp_hidden_mul * D;
    int64_t expect = off[S.mlp(dec, l, 0)];
    for (int q = 0; q < d.mlp_nlin; ++q) {
      const int hin = q == 0 ? D : H, hout = q == d.mlp_nlin - 1 ? D : H;
      LGN_CHECK_ARG(off[S.mlp(dec, l, 2 * q)] == expect, "MLP weights are not contiguous in the flat parameter buffer");
      expect += (int64_t)hin * hout;
      LGN_CHECK_ARG(off[S.mlp(dec, l, 2 * q + 1)] == expect, "MLP biases are not contiguous in the flat parameter buffer");
      expect += hout;
    }
  }
  return 0;
}

// the arguments of level l's CGMLP every caller shares: shape (M = B N), activation, weights and biases
MlpArgs<double> level_mlp_args(const lgn_net_desc& d, bool dec, int l, const double* P, const int64_t* off) {
  const Slots S{d.n_levels, d.mlp_nlin};
  const int CO = (dec ? d.dec_channels : d.enc_channels)[l + 1];
  MlpArgs<double> m{};
  m.M = d.B * d.N; m.C = CO; m.H = d.mlp_hidden_mul * 2 * CO; m.nlin = d.mlp_nlin; m.act = d.activation; m.flags = d.flags;
  for (int q = 0; q < d.mlp_nlin; ++q) { m.w[q] = P + off[S.mlp(dec, l, 2 * q)]; m.b[q] = P + off[S.mlp(dec, l, 2 * q + 1)]; }
  return m;
}

// decoder-side operands of junction_bwd (whole step): the decoder's input stage backward and the encoder's latent stage backward of
// a jet are then ONE launch, made by the encoder's backward
struct JunctionBwd {
  int C0, Tin;
  const double *lat_v, *wg1, *w1, *pdec, *g_p, *g_s0, *g_v0;
  double* part_dec;
};

// The loss argument of the whole-step calls: nullptr for Chamfer, else the loss stage that is a launch of its own after the
// decoder's last level (net.hpp: StageLoss) -- an assignment loss, or the EMD, whose descriptor is an lgn_emd_loss_desc read through
// its first member.  The one planner of any non-Chamfer stage: every refusal is made here, before anything is enqueued.
int plan_assign_loss(const lgn_net_desc* d, const lgn_loss_desc* loss, int* assignment, int* status, StageLoss& al, const StageLoss** out) {
  *out = nullptr;
  if (!loss || loss->kind == LGN_LOSS_CHAMFER) return 0;
  if (int rc = check_desc(d)) return rc;
  const int Nd = dec_nodes(*d), CL = d->dec_channels[d->n_levels];
  al = StageLoss{};
  al.kind = loss->kind;
  if (loss->kind == LGN_LOSS_EMD) {
    const lgn_emd_loss_desc* e = reinterpret_cast<const lgn_emd_loss_desc*>(loss);
    al.emd = EmdLoss{e->opts, loss->scale, e->chamfer_weight, status};
    al.emd.opts.norm = e->opts.norm != 0, al.emd.opts.periodic_phi = e->opts.periodic_phi != 0;
    if (int rc = check_emd_loss(al.emd, Nd)) return rc;
    LGN_CHECK_ARG(loss->abs_coord == 0 && loss->polar_coord == 0, "step: LGN_LOSS_EMD takes abs_coord = polar_coord = 0 (the frame is "
                  "the relative polar one)");
  } else {
    al.al = AssignLoss{loss->kind, loss->abs_coord, loss->polar_coord, loss->scale, assignment, status};
    if (int rc = check_assign_loss(al.al, Nd)) return rc;
  }
  LGN_CHECK_ARG(d->jet_loss_scale == 0.0, "step: jet_loss_scale=%g with loss kind %d: the jet-feature term is a Chamfer option "
                "(--chamfer-jet-features)", d->jet_loss_scale, loss->kind);
  if (loss->kind == LGN_LOSS_EMD) {
    const long long need = emd_loss_lds_bytes(Nd, CL);
    LGN_CHECK_ARG(need <= LGN_LDS_LIMIT, "step: the EMD loss stage at N=%d needs %lld B of LDS (lgn_emd_loss_lds_bytes; > %d)", Nd, need,
                  LGN_LDS_LIMIT);
  } else {
    const size_t need = assign_loss_lds_bytes(Nd, CL);
    LGN_CHECK_ARG(need <= LGN_LDS_LIMIT, "step: the assignment-loss stage at N=%d needs %zu B of LDS (> %d)", Nd, need, LGN_LDS_LIMIT);
  }
  *out = &al;
  return 0;
}

// What the step's Chamfer stage does next to a StageLoss: nothing beside an assignment loss or the EMD alone; under the hybrid loss
// (LGN_LOSS_EMD with chamfer_weight > 0) it runs exactly as without one, its gradient scale times chamfer_weight, and the EMD stage
// after it accumulates.
bool stage_keeps_chamfer(const StageLoss* al) { return !al || (al->kind == LGN_LOSS_EMD && al->emd.chamfer_weight > 0.0); }
double chamfer_scale(const StageLoss* al) { return al ? al->emd.chamfer_weight : 1.0; }

// the training / evaluation launch of a StageLoss, by kind
int stage_loss_train(const StageLoss& L, int B, int N, int C, const double* v, const double* wo1, const double* target, int method,
                     double* recon, double* loss_part, double* g_v, double* part, hipStream_t st) {
  if (L.kind == LGN_LOSS_EMD) return dec_output_emd_loss(B, N, C, v, wo1, target, method, L.emd, recon, loss_part, g_v, part, st);
  return dec_output_assign_loss(B, N, C, v, wo1, target, method, L.al, recon, loss_part, g_v, part, st);
}
int stage_loss_eval(const StageLoss& L, int B, int N, int C, const double* v, const double* wo1, const double* target, int method,
                    double* recon_real, double* loss_part, hipStream_t st) {
  if (L.kind == LGN_LOSS_EMD) return dec_output_emd_eval(B, N, C, v, wo1, target, method, L.emd, recon_real, loss_part, st);
  return dec_output_assign_eval(B, N, C, v, wo1, target, method, L.al, recon_real, loss_part, st);
}

// ---------------------------------------------------------------------------------------------------------
// one maxdim-2 network: level stack, encoder, decoder (shared by the per-network calls, the training step and the evaluation step)
// ---------------------------------------------------------------------------------------------------------
struct NetBuf {                     // per-network activations kept for the backward pass
  double *s[5], *v[5], *smix[4], *ag0[4], *ag1[4];
  double* hsave[4];                 // hidden activations of the level's CGMLP, kept for its backward (null: recomputed)
  double* sep[4];                   // decoder: jet sums of a separable level, kept instead of ag0 / ag1 (LevelArgs::sep_sums)
};
// The activations a network keeps on BN = B N nodes.  last_mlp_bwd: does the last level's CGMLP have a backward?  The step never runs
// it (the last level's scalars never reach the loss), so nothing is kept for it there; a per-network caller's
// upstream gradient may reach every level.  (A CGMLP that rides on the level kernels recomputes: nothing kept.)
// The copy is kept in the 16-row regime (BN <= mlp_save_max_rows()) and, beyond it, where the descriptor asks for it
// (LGN_NET_MLP_KEEP: the 64-row two-role kernels of mlp_chain.hip); levels_fwd / levels_bwd hand on whatever is carved here.
void carve_net(Bump& b, const lgn_net_desc& d, bool dec, size_t BN, bool last_mlp_bwd, NetBuf& n) {
  const int* ch = dec ? d.dec_channels : d.enc_channels;
  const int L = d.n_levels;
  for (int l = 0; l <= L; ++l) {
    n.s[l] = b.take(2 * BN * ch[l]);
    n.v[l] = b.take(8 * BN * ch[l]);
  }
  for (int l = 0; l < L; ++l) {
    n.smix[l] = b.take(2 * BN * ch[l + 1]);
    n.ag0[l] = b.take(4 * BN * ch[l]);
    n.ag1[l] = b.take(16 * BN * ch[l]);
    n.sep[l] = dec ? b.take((size_t)d.B * sep_sums_doubles(ch[l])) : nullptr;
    const size_t hs = (last_mlp_bwd || l + 1 < L) && (BN <= mlp_save_max_rows() || (d.flags & LGN_NET_MLP_KEEP))
                          ? mlp_saved_doubles((int)BN, d.mlp_hidden_mul * 2 * ch[l + 1], d.mlp_nlin) : 0;
    n.hsave[l] = hs ? b.take(hs) : nullptr;
  }
}

// What a backward through level stacks works in -- levels_bwd reads and writes nothing else.  The step has one for both networks.
struct BwdScratch {
  double *gs[2], *gv[2];       // gradient w.r.t. a level's features, two buffers used in turn
  double *gsmix, *g_ag;
  // the zero block: zeros_s (the scalar gradient nobody produced), g_p (decoder: d p, accumulated), g_lat_s (the latent scalars'
  // gradient nobody produced), tail_cnt (4 counters of the fused reduction: step_tail.hip, reduce_only) -- contiguous, one clear;
  // first in the per-network scratch (tail_cnt leading), behind the gradient buffers in the step (tail_cnt closing): carve_scratch / carve
  double *zeros_s, *g_p, *g_lat_s, *tail_cnt;
  size_t zero_doubles;
  double* zero0() const { return tail_cnt < zeros_s ? tail_cnt : zeros_s; }     // start of the zero block
  double* tot[4];              // encoder: reduced radial sums per level
  double* parts;               // bump region: every producer of partial rows gets its own slice (reduced at the end)
  size_t parts_size;
};
void carve_level_grads(Bump& b, size_t BN, int cmax, BwdScratch& k) {
  for (int q = 0; q < 2; ++q) {
    k.gs[q] = b.take(2 * BN * cmax);
    k.gv[q] = b.take(8 * BN * cmax);
  }
  k.gsmix = b.take(2 * BN * cmax);
  k.g_ag = b.take(20 * BN * cmax);
}
inline size_t tot_doubles(int C, bool dec) { return rad_partial_size(C, dec) + 16; }

// partial-row capacity of one maxdim-2 network on N nodes: its level stack (levels_bwd) and its end stages.  (The decoder's CGMLP rows
// are counted on dec_nodes(d) even for a per-network call, where the descriptor's dec_N is 0 -- as the layout has always been sized.)
size_t net_parts(const lgn_net_desc& d, bool dec, int N) {
  const int* ch = dec ? d.dec_channels : d.enc_channels;
  int rm, rr;
  level_bwd_partial_rows(d.B, N, dec, d.flags, &rm, &rr);
  size_t sum = 0;
  for (int l = 0; l < d.n_levels; ++l) {
    const int H = d.mlp_hidden_mul * 2 * ch[l + 1];
    sum += r16((size_t)rm * 4 * ch[l + 1] * 5 * ch[l]) + r16((size_t)rr * rad_partial_size(ch[l], dec)) +
           r16((size_t)mlp_partial_rows(d.B * (dec ? dec_nodes(d) : N), H) * mlp_param_count(ch[l + 1], H, d.mlp_nlin));
  }
  // the encoder's input-stage rows: one per jet, or one per workgroup of the first level's backward when they ride on it
  return sum + end_parts(d, dec, N, rm > d.B ? rm : d.B);
}

// The encoder's input stage (input_func_node on mass and canonical momenta) rides on the first level's kernel, which then
// is the first kernel of the call and also clears z1 / z2 (LevelArgs::in_w0).
struct InputStage {
  const double *w0, *w1;
  double* z1 = nullptr;
  size_t z1n = 0;
  double* z2 = nullptr;
  size_t z2n = 0;
};
// The decoder output + Chamfer loss (forward and backward) rides on the decoder's last level forward (LevelArgs::loss_wo1).
struct LossStage {
  const double *wo1, *target;
  double scale;
  int method;      // get_real code
  double jscale;   // jet-feature term weight (0: off)
  double *recon, *loss_part, *g_v, *wpart;
};

// forward of one network's level stack; returns via buffers
// eval (evaluation step): the level kernels without the aggregate stores (level_fwd_eval; n.ag0 / ag1 unused), a riding loss
// tail in its forward-only form, and no CGMLP after the decoder's last level (its scalars never reach the output)
// last_scalars = false: the caller consumes no output of the last level's CGMLP (the last level's scalars n.s[L]), which is then
// not launched and leaves n.s[L] unwritten -- a step that returns no latent scalars, for either network (the decoder's output
// and loss read only its last level's vectors; the latent vectors only the encoder's, and the latent scalars, which then mean
// nothing, carry no gradient: LatentStage).  The last level's kernel then runs without live scalars (LevelArgs::dead_scalars: no
// scalar aggregates, no scalar CatMix rows, n.smix / n.ag0 of that level unwritten); LVL_LIVE_SCALARS keeps the full kernel (cross-check).
int levels_fwd(const lgn_net_desc& d, bool dec, const double* P, const int64_t* off, NetBuf& n, const double* pos, const uint8_t* mask,
               hipStream_t st, const InputStage* in0, const LossStage* loss, bool eval, bool last_scalars) {
  const Slots S{d.n_levels, d.mlp_nlin};
  const int* ch = dec ? d.dec_channels : d.enc_channels;
  for (int l = 0; l < d.n_levels; ++l) {
    auto p = [&](int slot) { return P + off[slot]; };
    LevelArgs<double> a{d.B, d.N, ch[l], ch[l + 1], n.s[l], n.v[l], pos, mask,
                        p(S.rad(dec, l, 0)), p(S.rad(dec, l, 1)), p(S.rad(dec, l, 2)), p(S.rad(dec, l, 3)), p(S.rad(dec, l, 4)),
                        p(S.rad(dec, l, 5)), p(S.rad(dec, l, 6)), p(S.mix(dec, l, 0)), p(S.mix(dec, l, 1)),
                        n.ag0[l], n.ag1[l], n.smix[l], n.v[l + 1]};
    if (l == 0 && !dec && in0) {
      a.in_w0 = in0->w0; a.in_w1 = in0->w1; a.in_s = n.s[0]; a.in_v = n.v[0];
      a.z1 = in0->z1; a.z1n = in0->z1n; a.z2 = in0->z2; a.z2n = in0->z2n;
    }
    if (l + 1 == d.n_levels && dec && loss) {
      a.loss_wo1 = loss->wo1; a.loss_target = loss->target; a.loss_scale = loss->scale; a.loss_real = loss->method;
      a.loss_jscale = loss->jscale; a.loss_recon = loss->recon;
      a.loss_part = loss->loss_part; a.loss_gv = loss->g_v; a.loss_wpart = loss->wpart;
    }
    a.flags = d.flags;
    if (dec && !eval && level_dec_rebuilds(d.N, d.flags)) a.sep_sums = n.sep[l];     // (levels_bwd makes the same choice)
    const bool no_mlp = l + 1 == d.n_levels && (!last_scalars || (eval && dec));
    a.dead_scalars = no_mlp && !(d.flags & LVL_LIVE_SCALARS);
    LGN_TRY(eval ? level_fwd_eval(a, dec, st) : level_fwd_dispatch<double>(a, dec, st));
    if (no_mlp) break;
    MlpArgs<double> m = level_mlp_args(d, dec, l, P, off);
    m.s_in = n.smix[l]; m.s_out = n.s[l + 1];
    m.h_saved = n.hsave[l]; m.h_rows = mlp_saved_rows(m.M);
    LGN_TRY(mlp_dispatch<double>(m, false, st));
  }
  return 0;
}

// backward of one network's level stack.  On entry gs[cur]/gv[cur] hold the gradient w.r.t. (s[L], v[L]);
// has_s_grad says whether gs is non-zero (false for both networks of the autoencoder: the last level's
// scalars never reach the loss).  On exit gs[cur]/gv[cur] hold the gradient w.r.t. level 0.
// in0_done (encoder only, optional): the input stage's backward (mass only) may ride on the first level's.  When that level's
// backward is the one-kernel form, it does (LevelBwdArgs::part_in0) and *in0_done is set; otherwise the caller launches enc_input_bwd.
int levels_bwd(const lgn_net_desc& d, bool dec, const double* P, double* G, const int64_t* off, const NetBuf& n, const double* pos,
               const uint8_t* mask, BwdScratch& w, Deferred& dq, RadFinJob& fin, int& cur, bool has_s_grad, hipStream_t st,
               bool* in0_done = nullptr) {
  const Slots S{d.n_levels, d.mlp_nlin};
  const int* ch = dec ? d.dec_channels : d.enc_channels;
  const int BN = d.B * d.N;
  for (int l = d.n_levels - 1; l >= 0; --l) {
    auto p = [&](int slot) { return P + off[slot]; };
    auto g = [&](int slot) { return G + off[slot]; };
    const int C = ch[l], CO = ch[l + 1];
    const double* g_smix = w.zeros_s;
    if (has_s_grad) {
      MlpArgs<double> m = level_mlp_args(d, dec, l, P, off);
      m.s_in = n.smix[l]; m.g_out = w.gs[cur]; m.g_in = w.gsmix;
      m.h_saved = n.hsave[l];
      m.h_rows = mlp_saved_rows(BN);
      m.psize = mlp_param_count(CO, m.H, m.nlin);
      DQ_TAKE(m.part, (size_t)mlp_partial_rows(BN, m.H) * m.psize);
      LGN_TRY(mlp_dispatch<double>(m, true, st));
      // the MLP's parameters are contiguous in the flat buffer in (W_0, b_0, W_1, ...) order (checked at plan time)
      dq.add(m.part, mlp_partial_rows(BN, m.H), m.psize, 0, m.psize, g(S.mlp(dec, l, 0)));
      g_smix = w.gsmix;
    }
    int rm, rr;
    level_bwd_partial_rows(d.B, d.N, dec, d.flags, &rm, &rr);
    const int nmix = 4 * CO * 5 * C, nrad = rad_partial_size(C, dec);
    DQ_NEW(part_mix, (size_t)rm * nmix);
    DQ_NEW(part_rad, (size_t)rr * nrad);
    const int nxt = cur ^ 1;
    LevelBwdArgs<double> a{d.B, d.N, C, CO, n.s[l], n.v[l], pos, mask,
                           p(S.rad(dec, l, 0)), p(S.rad(dec, l, 1)), p(S.rad(dec, l, 2)), p(S.rad(dec, l, 3)), p(S.rad(dec, l, 4)),
                           p(S.rad(dec, l, 5)), p(S.rad(dec, l, 6)), p(S.mix(dec, l, 0)), p(S.mix(dec, l, 1)), n.ag0[l], n.ag1[l],
                           g_smix, w.gv[cur], w.g_ag, w.gs[nxt], w.gv[nxt], dec ? w.g_p : nullptr, part_mix, part_rad};
    // No gradient on this level's scalars (the first level this loop runs): the one-kernel backward leaves out every term it zeroes
    // (LevelBwdArgs::dead_scalars).  The N > 40 kernels (level_bwd.hip, level_bwd2.hip) have no such form and keep reading the zero
    // block; what they write into the wm0 half of their partial rows is not reduced either (the forward has not stored ag0).
    const bool dead_s = !has_s_grad && !(d.flags & LVL_LIVE_SCALARS);
    a.dead_scalars = dead_s;
    const bool carry_in0 = !dec && l == 0 && in0_done && level_bwd_carries_input(d.N, d.flags);
    const RowLayout rin = enc_input_rows(1, C);
    if (carry_in0) { DQ_TAKE(a.part_in0, (size_t)rm * rin.width); }
    a.flags = d.flags;
    if (dec && level_dec_rebuilds(d.N, d.flags)) a.sep_sums = n.sep[l];
    LGN_TRY(level_bwd_dispatch<double>(a, dec, st));
    if (carry_in0) {
      rin.add(dq, a.part_in0, rm, G, off);
      *in0_done = true;
    }
    // deferred reductions: CatMix weights (partial row = [wm0 | wm1]) + radial sums
    // (dead scalars: the wm0 gradient is exactly zero -- a row-less segment, like every parameter nothing produces a gradient for)
    if (dead_s) dq.add(nullptr, 0, 0, 0, nmix / 2, g(S.mix(dec, l, 0)));
    else dq.add(part_mix, rm, nmix, 0, nmix / 2, g(S.mix(dec, l, 0)));
    dq.add(part_mix, rm, nmix, nmix / 2, nmix / 2, g(S.mix(dec, l, 1)));
    if (dec) {   // only the Linear biases receive gradient (all edges are "masked")
      dq.add(part_rad, rr, nrad, 0, C, g(S.rad(dec, l, 4)));
      dq.add(part_rad, rr, nrad, C, C, g(S.rad(dec, l, 6)));
    } else {
      double* tot = w.tot[l];
      dq.add(part_rad, rr, nrad, 0, nrad, tot);
      fin.it[fin.n++] = RadFinJob::Item{tot, C, p(S.rad(dec, l, 0)), p(S.rad(dec, l, 1)), p(S.rad(dec, l, 2)), p(S.rad(dec, l, 3)),
                                        p(S.rad(dec, l, 5)), g(S.rad(dec, l, 0)), g(S.rad(dec, l, 1)), g(S.rad(dec, l, 2)),
                                        g(S.rad(dec, l, 3)), g(S.rad(dec, l, 4)), g(S.rad(dec, l, 5)), g(S.rad(dec, l, 6))};
    }
    cur = nxt;
    has_s_grad = true;       // the level input scalars do carry gradient
  }
  return 0;
}

// ---- one maxdim-2 network, forward / backward, in the shape of gen_encoder_fwd ... gen_decoder_bwd below --------------
// ride: the input stage rides on the first level's kernel, which then also makes ride's two clears (the mass as the only input scalar);
//   nullptr: enc_input_fwd as a launch of its own on the K scalars xs
// with_latent = false (fused whole step): the latent stage runs in the junction kernel together with the decoder's input stage
// last_scalars = false: nobody reads the latent scalars -- no last CGMLP, the latent stage takes the last level's scalars as zero
int encoder_fwd(const lgn_net_desc& d, const double* P, const int64_t* off, const double* p4, const uint8_t* mask, const double* xs,
                NetBuf& n, double* lat_s, double* lat_v, int* idx, hipStream_t st, const InputStage* ride, bool with_latent = true,
                bool eval = false, bool last_scalars = true) {
  const Slots S{d.n_levels, d.mlp_nlin};
  const int L = d.n_levels;
  const int* ce = d.enc_channels;
  if (!ride) LGN_TRY(enc_input_fwd(d.B, d.N, ce[0], in_K(d), p4, xs, P + off[0], P + off[1], n.s[0], n.v[0], st));
  LGN_TRY(levels_fwd(d, false, P, off, n, p4, mask, st, ride, nullptr, eval, last_scalars));
  if (with_latent)
    LGN_TRY(enc_latent_fwd(d.B, d.N, ce[L], d.tau_s, d.tau_v, d.latent_pool, last_scalars ? n.s[L] : nullptr, n.v[L], P + off[S.out0(false)],
                           P + off[S.out0(false) + 1], lat_s, lat_v, idx, st));
  return 0;
}

// The caller has zero-filled G and k's zero block; dq / fin are the caller's and are run by the caller.  The latent stage's backward
// writes k.gs[cur] / k.gv[cur].  g_lat_s = nullptr: no gradient on the latent scalars (the zero block's g_lat_s stands in), and then
// none on the last level's scalars and its CGMLP.  last_scalars: as in encoder_fwd.
// ride_in0: the input stage's backward rides on the first level's where that is the one-kernel form (levels_bwd); else, and where it
//   is not, enc_input_bwd is a launch of its own.
// jb (fused whole step): the decoder's input stage backward and this latent stage backward of a jet in one launch
int encoder_bwd(const lgn_net_desc& d, const double* P, double* G, const int64_t* off, const double* p4, const uint8_t* mask,
                const double* xs, const NetBuf& n, const int* idx, const double* g_lat_s, const double* g_lat_v, BwdScratch& k, int cur,
                Deferred& dq, RadFinJob& fin, hipStream_t st, bool ride_in0, bool last_scalars = true, const JunctionBwd* jb = nullptr) {
  const Slots S{d.n_levels, d.mlp_nlin};
  const int L = d.n_levels, B = d.B, N = d.N, K = in_K(d);
  const int* ce = d.enc_channels;
  {
    const RowLayout rl = enc_latent_rows(d, N, ce[L]);
    const double *sL = last_scalars ? n.s[L] : nullptr, *wl0 = P + off[S.out0(false)], *wl1 = P + off[S.out0(false) + 1];
    DQ_NEW(parte, (size_t)B * rl.width);
    if (jb)
      LGN_TRY(junction_bwd(B, N, jb->C0, jb->Tin, jb->lat_v, jb->wg1, jb->w1, jb->pdec, jb->g_p, jb->g_s0, jb->g_v0, const_cast<double*>(g_lat_v),
                           jb->part_dec, ce[L], d.tau_s, d.tau_v, d.latent_pool, sL, n.v[L], wl0, wl1, g_lat_s ? g_lat_s : k.g_lat_s, idx,
                           k.gs[cur], k.gv[cur], parte, st));
    else
      LGN_TRY(enc_latent_bwd(B, N, ce[L], d.tau_s, d.tau_v, d.latent_pool, sL, n.v[L], wl0, wl1, g_lat_s ? g_lat_s : k.g_lat_s, g_lat_v, idx,
                             k.gs[cur], k.gv[cur], parte, st));
    rl.add(dq, parte, B, G, off);
  }
  bool in0_done = false;
  LGN_TRY(levels_bwd(d, false, P, G, off, n, p4, mask, k, dq, fin, cur, /*has_s_grad=*/g_lat_s != nullptr, st, ride_in0 ? &in0_done : nullptr));
  if (!in0_done) {      // (several input scalars, a split step, or the three-kernel level backward: N > 40, LGN_AMD_LEVEL_V2)
    const RowLayout ri = enc_input_rows(K, ce[0]);
    DQ_NEW(part, (size_t)B * ri.width);
    LGN_TRY(enc_input_bwd(B, N, ce[0], K, p4, xs, k.gs[cur], k.gv[cur], part, st));
    ri.add(dq, part, B, G, off);
  }
  return 0;
}

// forward up to the last level's features (the caller applies dec_output_fwd, or a loss kernel where the loss does not ride)
// with_input = false (fused whole step): the junction kernel has run the input stage
// loss: output + loss ride on the last level's kernel;  eval, last_scalars: as in levels_fwd
int decoder_fwd(const lgn_net_desc& d, const double* P, const int64_t* off, const double* lat_v, NetBuf& n, double* pdec, hipStream_t st,
                bool with_input = true, const LossStage* loss = nullptr, bool eval = false, bool last_scalars = true) {
  if (with_input)
    LGN_TRY(dec_input_fwd(d.B, d.N, d.dec_channels[0], dec_tin(d), lat_v, P + off[1], P + off[2], P + off[3], pdec, n.s[0], n.v[0], st));
  return levels_fwd(d, true, P, off, n, pdec, nullptr, st, nullptr, loss, eval, last_scalars);
}

// k.gv[cur] holds the gradient w.r.t. the last level's vectors (from dec_output_bwd or a loss kernel); on exit `cur` is the buffer
// pair with the gradient w.r.t. the level-0 features.  dq / fin are the caller's and are run by the caller.
// part_in (fused whole step): the input stage's backward is the caller's (junction kernel) -- its partial rows are allocated and their
// reductions registered here, *part_in tells the caller where they go
int decoder_bwd(const lgn_net_desc& d, const double* P, double* G, const int64_t* off, const double* lat_v, const NetBuf& n,
                const double* pdec, double* g_lat_v, BwdScratch& k, int& cur, Deferred& dq, RadFinJob& fin, hipStream_t st,
                double** part_in = nullptr) {
  const int B = d.B, N = d.N, C0 = d.dec_channels[0], Tin = dec_tin(d);
  LGN_TRY(levels_bwd(d, true, P, G, off, n, pdec, nullptr, k, dq, fin, cur, /*has_s_grad=*/false, st));
  const RowLayout ri = dec_input_rows(C0, N, Tin);
  DQ_NEW(part, (size_t)B * ri.width);
  if (part_in) *part_in = part;
  else LGN_TRY(dec_input_bwd(B, N, C0, Tin, lat_v, P + off[1], P + off[3], pdec, k.g_p, k.gs[cur], k.gv[cur], g_lat_v, part, st));
  ri.add(dq, part, B, G, off);
  return 0;
}

// ---------------------------------------------------------------------------------------------------------
// one table-driven network (maxdim = 3): same structure as above on packed features X_l [2][B][N][C_l][Q_l]
//   level forward : moments (generic_moments.hip) -> sparse CG + CatMix (generic_local.hip) -> CGMLP in place on the
//                   scalar column; backward in reverse.  Reference: LGNCG.forward lgn/models/lgn_cg.py:164-172.
// ---------------------------------------------------------------------------------------------------------
inline bool is_generic(const lgn_net_desc& d, bool dec) { return (dec ? d.dec_tables[0] : d.enc_tables[0]) != nullptr; }

struct GenGeom {                   // per-network view of the descriptor
  const int *ch, *Q, *qs, *qv;
  const lgn_local_tables* const* tab;
};
inline GenGeom geom(const lgn_net_desc& d, bool dec) {
  return dec ? GenGeom{d.dec_channels, d.dec_Q, d.dec_qs, d.dec_qv, d.dec_tables}
             : GenGeom{d.enc_channels, d.enc_Q, d.enc_qs, d.enc_qv, d.enc_tables};
}

// every level has compile-time tables and the jets fit the channel-outermost moments kernels: tile-blocked feature layouts
// [tile][C][Q][2][64] end to end, generic_local_static.hip for the per-node part
inline bool is_static(const lgn_net_desc& d, bool dec) {
  const GenGeom g = geom(d, dec);
  if (d.N > 32) return false;
  for (int l = 0; l < d.n_levels; ++l)
    if (!g.tab[l] || g.tab[l]->static_kind == 0) return false;
  return !(d.flags & LGN_NET_NO_STATIC);                // run-time-table kernels (cross-check): fixed at descriptor creation
}
// decoder levels on the static kernels keep their separable moments on chip (generic_local_sep.hip, round 6): no U / dU tensors,
// one launch per level backward.  LGN_NET_DEC_UNFUSED: the round-5 sequence (dec_sep_fwd/bwd_tb + local_fwd/bwd_static), cross-check
inline bool is_sep_fused(const lgn_net_desc& d, bool dec) {
  return dec && is_static(d, dec) && !(d.flags & (LGN_NET_DEC_PAIRWISE | LGN_NET_DEC_UNFUSED));
}
inline size_t tb_doubles(const lgn_net_desc& d, int C, int Qx) { return (size_t)(((size_t)d.B * d.N + 63) / 64) * C * Qx * 128; }

int check_generic(const lgn_net_desc& d, bool dec) {
  const GenGeom g = geom(d, dec);
  for (int l = 0; l < d.n_levels; ++l) {
    LGN_CHECK_ARG(g.tab[l], "table-driven network: level %d has no tables (every level needs one)", l);
    LGN_CHECK_ARG(g.tab[l]->n_w > 0 && g.tab[l]->n_rows > 0, "table-driven network: empty tables at level %d", l);
  }
  for (int l = 0; l <= d.n_levels; ++l)
    LGN_CHECK_ARG(g.Q[l] >= 5 && g.Q[l] <= 64 && g.qs[l] >= 0 && g.qs[l] < g.Q[l] && g.qv[l] >= 0 && g.qv[l] + 4 <= g.Q[l],
                  "table-driven network: bad component layout at level %d (Q=%d qs=%d qv=%d)", l, g.Q[l], g.qs[l], g.qv[l]);
  LGN_CHECK_ARG(g.Q[0] == 5, "table-driven network: the input level carries (1,1) and (0,0) only (Q=5), got %d", g.Q[0]);
  return 0;
}

struct GenAct {                     // written by the forward, read by the backward
  double *s0, *v0;                  // input-kernel outputs [2][BN][C0], [2][BN][C0][4]
  double *X[5], *U[4], *smix[4];
  double* wp[4];                    // static path: packed CatMix weights of each level (written by the forward, reused by the backward)
  double* tbl[4];                   // fused decoder levels: jet table of each level (dec_sep_tab), instead of U
  double* pc;                       // ... and the nodes' centred momenta [B N][8]
  double *sL, *vL;                  // (0,0) / (1,1) of the last level, unpacked for the end kernels
  double* pdec;
  int* idx;
  size_t total;
};
GenAct carve_gen_act(const lgn_net_desc& d, bool dec, double* base) {
  GenAct a{};
  Bump b{base};
  const GenGeom g = geom(d, dec);
  const size_t BN = (size_t)d.B * d.N;
  const int L = d.n_levels;
  a.s0 = b.take(2 * BN * g.ch[0]);
  a.v0 = b.take(8 * BN * g.ch[0]);
  const bool tb = is_static(d, dec);                  // whole tiles of 64 nodes
  const bool sep = is_sep_fused(d, dec);
  for (int l = 0; l <= L; ++l) a.X[l] = b.take(tb ? tb_doubles(d, g.ch[l], g.Q[l]) : 2 * BN * g.ch[l] * g.Q[l]);
  a.pc = sep ? b.take(8 * BN) : nullptr;
  for (int l = 0; l < L; ++l) {
    a.U[l] = sep ? nullptr : b.take(tb ? tb_doubles(d, g.ch[l], 5 * g.Q[l]) : 10 * BN * g.ch[l] * g.Q[l]);
    a.tbl[l] = sep ? b.take((size_t)d.B * g.ch[l] * g.Q[l] * SEP_TBL_STRIDE) : nullptr;
    a.smix[l] = b.take(2 * BN * g.ch[l + 1]);
    a.wp[l] = tb ? b.take(local_static_packed_doubles(g.tab[l]->static_kind, g.ch[l], g.ch[l + 1])) : nullptr;
  }
  a.sL = b.take(2 * BN * g.ch[L]);
  a.vL = b.take(8 * BN * g.ch[L]);
  if (dec) a.pdec = b.take(8 * BN);
  else a.idx = reinterpret_cast<int*>(b.take(pool_idx_doubles(d)));
  a.total = b.off;
  return a;
}

struct GenScratch {
  double *zero0, *g_p, *g_lat_s;    // zero block (first): zeros for a missing scalar gradient | decoder d p | encoder g_lat_s stand-in
  size_t zero_doubles;
  double *gs, *gv;                  // unpacked gradients at the two ends
  double *gX[2], *gU;
  double* gbuf;                     // encoder: pair-gradient scratch of the channel-outermost radial backward (generic_moments2.hip)
  double* gpk[4];                   // static path: reduced packed CatMix weight gradients per level
  double* gpb[4];                   // fused decoder levels: per-channel d p of each level [C_l][B N][8]
  double* tot[4];
  double* parts;
  size_t parts_size, total;
};
// partial-row capacity of one table-driven network: its level stack (gen_levels_bwd) and its end stages
size_t gen_net_parts(const lgn_net_desc& d, bool dec) {
  const GenGeom g = geom(d, dec);
  const size_t BN = (size_t)d.B * d.N, tiles = (BN + 63) / 64;
  const bool tb = is_static(d, dec), sep = is_sep_fused(d, dec);
  size_t sum = 0;
  for (int l = 0; l < d.n_levels; ++l) {
    const int H = d.mlp_hidden_mul * 2 * g.ch[l + 1];
    const size_t lrows = tb ? (sep ? (size_t)local_sep_part_rows(d.B) : tiles) * local_static_packed_doubles(g.tab[l]->static_kind, g.ch[l], g.ch[l + 1])
                            : (size_t)local_partial_rows((int)BN) * 2 * g.tab[l]->n_w;
    sum += r16(lrows) + r16((size_t)d.B * rad_partial_size(g.ch[l], dec)) +
           r16((size_t)mlp_partial_rows((int)BN, H) * mlp_param_count(g.ch[l + 1], H, d.mlp_nlin));
  }
  return sum + end_parts(d, dec, d.N, d.B);
}

GenScratch carve_gen_scratch(const lgn_net_desc& d, bool dec, double* base) {
  GenScratch s{};
  Bump b{base};
  const GenGeom g = geom(d, dec);
  const size_t BN = (size_t)d.B * d.N;
  const int L = d.n_levels;
  size_t cq = 0, cmax = 0;
  for (int l = 0; l <= L; ++l) {
    cq = cq > (size_t)g.ch[l] * g.Q[l] ? cq : (size_t)g.ch[l] * g.Q[l];
    cmax = cmax > (size_t)g.ch[l] ? cmax : (size_t)g.ch[l];
  }
  {
    const size_t z0 = b.off;
    s.zero0 = b.take(2 * BN * cmax);
    s.g_p = b.take(dec ? 8 * BN : 0);
    s.g_lat_s = b.take(dec ? 0 : lat_s_doubles(d));
    s.zero_doubles = b.off - z0;
  }
  s.gs = b.take(2 * BN * cmax);
  s.gv = b.take(8 * BN * cmax);
  const bool tb = is_static(d, dec), sep = is_sep_fused(d, dec);
  const size_t tiles = (BN + 63) / 64;
  s.gX[0] = b.take(tb ? tiles * cq * 128 : 2 * BN * cq);
  s.gX[1] = b.take(tb ? tiles * cq * 128 : 2 * BN * cq);
  s.gU = sep ? nullptr : b.take(tb ? tiles * cq * 640 : 10 * BN * cq);
  for (int l = 0; l < L; ++l) {
    s.gpk[l] = tb ? b.take(local_static_packed_doubles(g.tab[l]->static_kind, g.ch[l], g.ch[l + 1])) : nullptr;
    s.gpb[l] = sep ? b.take((size_t)g.ch[l] * BN * 8) : nullptr;
  }
  s.gbuf = (!dec && d.N <= 32) ? b.take(moments2_gbuf_doubles(d.B, d.N, (int)cmax)) : nullptr;
  for (int l = 0; l < L; ++l) s.tot[l] = b.take(tot_doubles(g.ch[l], dec));
  const size_t psum = gen_net_parts(d, dec);
  s.parts = b.take(psum);
  s.parts_size = psum;
  s.total = b.off;
  return s;
}

GenArgs gen_level_args(const lgn_net_desc& d, bool dec, int l, const double* P, const int64_t* off, const double* X, const double* pos,
                       const uint8_t* mask) {
  const Slots S{d.n_levels, d.mlp_nlin};
  const GenGeom g = geom(d, dec);
  GenArgs a{};
  a.B = d.B; a.N = d.N; a.C = g.ch[l]; a.Q = g.Q[l]; a.X = X; a.p = pos; a.mask = mask;
  a.flags = d.flags;
  a.ra = P + off[S.rad(dec, l, 0)]; a.rb = P + off[S.rad(dec, l, 1)]; a.rc = P + off[S.rad(dec, l, 2)];
  a.w0 = P + off[S.rad(dec, l, 3)]; a.b0 = P + off[S.rad(dec, l, 4)]; a.w1 = P + off[S.rad(dec, l, 5)]; a.b1 = P + off[S.rad(dec, l, 6)];
  return a;
}

// X[0] (packed input features) must be in place; fills X[1..L], U, smix
int gen_levels_fwd(const lgn_net_desc& d, bool dec, const double* P, const int64_t* off, GenAct& a, const double* pos,
                   const uint8_t* mask, hipStream_t st) {
  const Slots S{d.n_levels, d.mlp_nlin};
  const GenGeom g = geom(d, dec);
  const int BN = d.B * d.N;
  const bool tb = is_static(d, dec);
  if (tb) {       // the packed CatMix weight images of all levels, one launch (the backward reuses them)
    StaticPackJob jobs[8];
    for (int l = 0; l < d.n_levels; ++l) {
      jobs[l] = StaticPackJob{g.tab[l]->static_kind, g.ch[l], g.ch[l + 1], {0, 0, 0, 0, 0}, P + off[S.mix(dec, l, 0)], a.wp[l]};
      for (int k = 0; k < 5; ++k) jobs[l].w0[k] = g.tab[l]->h_out_w0[k];
    }
    LGN_TRY(local_static_pack_batch(jobs, d.n_levels, false, st));
  }
  const bool sep = is_sep_fused(d, dec);
  for (int l = 0; l < d.n_levels; ++l) {
    GenArgs m = gen_level_args(d, dec, l, P, off, a.X[l], pos, mask);
    m.U = a.U[l];
    m.tb = tb;
    if (sep) {      // jet table instead of the moments tensor; the per-node kernel forms U where a term reads it
      LGN_TRY(dec_sep_tab(m, a.tbl[l], a.pc, st));
      LGN_TRY(local_fwd_sep(g.tab[l]->static_kind, d.B, d.N, g.ch[l], g.ch[l + 1], a.X[l], a.tbl[l], a.pc, a.wp[l], a.X[l + 1], a.smix[l],
                            g.qs[l + 1], st));
    } else if (tb) {
      LGN_TRY(moments_dispatch(m, dec, 0, st));
      int w0[8];
      for (int k = 0; k < 5; ++k) w0[k] = g.tab[l]->h_out_w0[k];
      LGN_TRY(local_fwd_static(g.tab[l]->static_kind, BN, g.ch[l], g.ch[l + 1], a.X[l], a.U[l], P + off[S.mix(dec, l, 0)], w0, a.wp[l],
                               a.X[l + 1], a.smix[l], g.qs[l + 1], st, /*packed=*/true));
    } else {
      LGN_TRY(moments_dispatch(m, dec, 0, st));
      LocalArgs la{};
      LGN_TRY(local_args(la, BN, g.ch[l], g.ch[l + 1], g.Q[l], g.Q[l + 1], g.tab[l]));
      la.X = a.X[l]; la.U = a.U[l]; la.wcat = P + off[S.mix(dec, l, 0)]; la.out = a.X[l + 1];
      la.s_copy = a.smix[l]; la.q_s = g.qs[l + 1];
      LGN_TRY(local_fwd(la, st));
    }
    MlpArgs<double> mm = level_mlp_args(d, dec, l, P, off);
    mm.s_in = a.smix[l];
    if (tb) { mm.s_out = a.X[l + 1] + (size_t)g.qs[l + 1] * 128; mm.tbQ = g.Q[l + 1]; }
    else { mm.s_out = a.X[l + 1] + g.qs[l + 1]; mm.ld = g.Q[l + 1]; }
    LGN_TRY(mlp_dispatch<double>(mm, false, st));
  }
  return 0;
}

// packed CatMix weight gradients (static path) are unpacked into the flat gradient AFTER the deferred reductions ran
typedef StaticPackJob UnpackJob;      // src = reduced packed gradients, dst = the CatMix slot of the flat gradient
int run_unpack_jobs(const std::vector<UnpackJob>& post, hipStream_t st) {
  if (post.empty()) return 0;
  return local_static_pack_batch(post.data(), (int)post.size(), true, st);
}

// On entry sc.gX[cur] holds the gradient w.r.t. X[L] (scalar column = 0 when !has_s_grad); on exit sc.gX[cur] the one w.r.t. X[0].
int gen_levels_bwd(const lgn_net_desc& d, bool dec, const double* P, double* G, const int64_t* off, const GenAct& a, const double* pos,
                   const uint8_t* mask, GenScratch& sc, Deferred& dq, RadFinJob& fin, std::vector<UnpackJob>& post, int& cur,
                   bool has_s_grad, hipStream_t st) {
  const Slots S{d.n_levels, d.mlp_nlin};
  const GenGeom g = geom(d, dec);
  const int BN = d.B * d.N;
  const bool tb = is_static(d, dec);
  for (int l = d.n_levels - 1; l >= 0; --l) {
    const int C = g.ch[l], CO = g.ch[l + 1];
    if (has_s_grad) {     // CGMLP backward, in place on the scalar column of the gradient
      MlpArgs<double> m = level_mlp_args(d, dec, l, P, off);
      m.s_in = a.smix[l];
      if (tb) { m.g_out = sc.gX[cur] + (size_t)g.qs[l + 1] * 128; m.g_in = sc.gX[cur] + (size_t)g.qs[l + 1] * 128; m.tbQ = g.Q[l + 1]; }
      else { m.g_out = sc.gX[cur] + g.qs[l + 1]; m.g_in = sc.gX[cur] + g.qs[l + 1]; m.ld = g.Q[l + 1]; }
      m.psize = mlp_param_count(CO, m.H, m.nlin);
      DQ_TAKE(m.part, (size_t)mlp_partial_rows(BN, m.H) * m.psize);
      LGN_TRY(mlp_dispatch<double>(m, true, st));
      dq.add(m.part, mlp_partial_rows(BN, m.H), m.psize, 0, m.psize, G + off[S.mlp(dec, l, 0)]);
    }
    const int nxt = cur ^ 1;
    if (is_sep_fused(d, dec)) {      // per-node part + separable moments of the level in ONE launch; d p per channel, reduced after the stack
      int w0[8];
      for (int k = 0; k < 5; ++k) w0[k] = g.tab[l]->h_out_w0[k];
      const int kind = g.tab[l]->static_kind, np = (int)local_static_packed_doubles(kind, C, CO), rows = local_sep_part_rows(d.B);
      const int nrad = rad_partial_size(C, true);
      DQ_NEW(part, (size_t)rows * np);
      DQ_NEW(part_rad, (size_t)d.B * nrad);
      // (partial rows in the layout of the CatMix parameters themselves, np apart: the reduction writes the gradient, nothing to unpack)
      LGN_TRY(local_bwd_sep(kind, d.B, d.N, C, CO, a.X[l], a.tbl[l], a.pc, P + off[S.rad(dec, l, 4)], P + off[S.rad(dec, l, 6)], a.wp[l], w0,
                            sc.gX[cur], sc.gX[nxt], part, sc.gpb[l], part_rad, st));
      dq.add(part, rows, np, 0, 2 * g.tab[l]->n_w, G + off[S.mix(dec, l, 0)]);
      dq.add(part_rad, d.B, nrad, 0, C, G + off[S.rad(dec, l, 4)]);
      dq.add(part_rad, d.B, nrad, C, C, G + off[S.rad(dec, l, 6)]);
      cur = nxt;
      has_s_grad = true;
      continue;
    }
    if (tb) {       // compile-time-table kernel; its packed partial rows are reduced with everything else, then unpacked (post)
      int w0[8];
      for (int k = 0; k < 5; ++k) w0[k] = g.tab[l]->h_out_w0[k];
      const int kind = g.tab[l]->static_kind, np = (int)local_static_packed_doubles(kind, C, CO), tiles = (BN + 63) / 64;
      DQ_NEW(part, (size_t)tiles * np);
      LGN_TRY(local_bwd_static(kind, BN, C, CO, a.X[l], a.U[l], P + off[S.mix(dec, l, 0)], w0, a.wp[l], sc.gX[cur], sc.gU, sc.gX[nxt], part, st,
                               /*packed=*/true, /*param_layout=*/true));
      dq.add(part, tiles, np, 0, 2 * g.tab[l]->n_w, G + off[S.mix(dec, l, 0)]);
    } else {
      LocalArgs la{};
      LGN_TRY(local_args(la, BN, C, CO, g.Q[l], g.Q[l + 1], g.tab[l]));
      const int rows = local_partial_rows(BN), nw2 = 2 * g.tab[l]->n_w;
      la.X = a.X[l]; la.U = a.U[l]; la.wcat = P + off[S.mix(dec, l, 0)]; la.g_out = sc.gX[cur];
      la.gU = sc.gU; la.gX = sc.gX[nxt]; DQ_TAKE(la.part, (size_t)rows * nw2);
      LGN_TRY(local_bwd(la, st));
      dq.add(la.part, rows, nw2, 0, nw2, G + off[S.mix(dec, l, 0)]);
    }
    GenArgs m = gen_level_args(d, dec, l, P, off, a.X[l], pos, mask);
    m.tb = tb;
    const int nrad = rad_partial_size(C, dec);
    m.gU = sc.gU; m.gX = sc.gX[nxt]; m.g_p = dec ? sc.g_p : nullptr; DQ_TAKE(m.part_rad, (size_t)d.B * nrad);
    m.gbuf = sc.gbuf;
    LGN_TRY(moments_dispatch(m, dec, 1, st));
    LGN_TRY(moments_dispatch(m, dec, 2, st));
    if (dec) {
      dq.add(m.part_rad, d.B, nrad, 0, C, G + off[S.rad(dec, l, 4)]);
      dq.add(m.part_rad, d.B, nrad, C, C, G + off[S.rad(dec, l, 6)]);
    } else {
      dq.add(m.part_rad, d.B, nrad, 0, nrad, sc.tot[l]);
      fin.it[fin.n++] = RadFinJob::Item{sc.tot[l], C, m.ra, m.rb, m.rc, m.w0, m.w1, G + off[S.rad(dec, l, 0)], G + off[S.rad(dec, l, 1)],
                                        G + off[S.rad(dec, l, 2)], G + off[S.rad(dec, l, 3)], G + off[S.rad(dec, l, 4)],
                                        G + off[S.rad(dec, l, 5)], G + off[S.rad(dec, l, 6)]};
    }
    cur = nxt;
    has_s_grad = true;
  }
  return 0;
}

// packed <-> separate (0,0) / (1,1) features at the ends of the level stack, in the layout the network runs on
int net_pack(const lgn_net_desc& d, bool dec, int l, const double* s, const double* v, double* X, hipStream_t st) {
  const GenGeom g = geom(d, dec);
  if (is_static(d, dec)) return gen_pack_tb(d.B * d.N, g.ch[l], g.Q[l], g.qs[l], g.qv[l], s, v, X, st);
  return gen_pack((size_t)d.B * d.N * g.ch[l], g.Q[l], g.qs[l], g.qv[l], s, v, X, st);
}
int net_unpack(const lgn_net_desc& d, bool dec, int l, const double* X, double* s, double* v, hipStream_t st) {
  const GenGeom g = geom(d, dec);
  if (is_static(d, dec)) return gen_unpack_tb(d.B * d.N, g.ch[l], g.Q[l], g.qs[l], g.qv[l], X, s, v, st);
  return gen_unpack((size_t)d.B * d.N * g.ch[l], g.Q[l], g.qs[l], g.qv[l], X, s, v, st);
}


// ---- one table-driven network, forward / backward (shared by the per-network API and the whole step) ----------------
// with_latent = false (whole step): the latent stage runs in the junction kernel together with the decoder's input stage
int gen_encoder_fwd(const lgn_net_desc& d, const double* P, const int64_t* off, const double* p4, const uint8_t* mask, GenAct& a,
                    double* lat_s, double* lat_v, hipStream_t st, const double* xs = nullptr, bool with_latent = true) {
  const Slots S{d.n_levels, d.mlp_nlin};
  const GenGeom g = geom(d, false);
  const int L = d.n_levels;
  LGN_TRY(enc_input_fwd(d.B, d.N, g.ch[0], in_K(d), p4, xs, P + off[0], P + off[1], a.s0, a.v0, st));
  LGN_TRY(net_pack(d, false, 0, a.s0, a.v0, a.X[0], st));
  LGN_TRY(gen_levels_fwd(d, false, P, off, a, p4, mask, st));
  LGN_TRY(net_unpack(d, false, L, a.X[L], a.sL, a.vL, st));
  if (with_latent)
    LGN_TRY(enc_latent_fwd(d.B, d.N, g.ch[L], d.tau_s, d.tau_v, d.latent_pool, a.sL, a.vL, P + off[S.out0(false)], P + off[S.out0(false) + 1],
                           lat_s, lat_v, a.idx, st));
  return 0;
}

// the caller has zero-filled G and sc's zero block
// hand_dq / hand_fin (whole step): the pending reductions and radial finalisations are handed to the caller instead of being run here
int gen_encoder_bwd(const lgn_net_desc& d, const double* P, double* G, const int64_t* off, const double* p4, const uint8_t* mask,
                    const GenAct& a, const double* g_lat_s, const double* g_lat_v, GenScratch& sc, hipStream_t st,
                    const double* xs = nullptr, Deferred* hand_dq = nullptr, RadFinJob* hand_fin = nullptr, const JunctionBwd* jb = nullptr) {
  const Slots S{d.n_levels, d.mlp_nlin};
  const GenGeom g = geom(d, false);
  const int L = d.n_levels, B = d.B, N = d.N, Ts = d.tau_s, Tv = d.tau_v;
  Deferred dq(sc.parts, sc.parts_size);
  RadFinJob fin{};
  int cur = 0;
  {
    const int CL = g.ch[L];
    const RowLayout rl = enc_latent_rows(d, N, CL);
    DQ_NEW(parte, (size_t)B * rl.width);
    if (jb)       // whole step: the decoder's input stage backward and this latent stage backward of a jet in one launch
      LGN_TRY(junction_bwd(B, N, jb->C0, jb->Tin, jb->lat_v, jb->wg1, jb->w1, jb->pdec, jb->g_p, jb->g_s0, jb->g_v0, const_cast<double*>(g_lat_v),
                           jb->part_dec, CL, Ts, Tv, d.latent_pool, a.sL, a.vL, P + off[S.out0(false)], P + off[S.out0(false) + 1],
                           g_lat_s ? g_lat_s : sc.g_lat_s, a.idx, sc.gs, sc.gv, parte, st));
    else
      LGN_TRY(enc_latent_bwd(B, N, CL, Ts, Tv, d.latent_pool, a.sL, a.vL, P + off[S.out0(false)], P + off[S.out0(false) + 1],
                             g_lat_s ? g_lat_s : sc.g_lat_s, g_lat_v, a.idx, sc.gs, sc.gv, parte, st));
    rl.add(dq, parte, B, G, off);
    LGN_TRY(net_pack(d, false, L, g_lat_s ? sc.gs : sc.zero0, sc.gv, sc.gX[cur], st));
  }
  std::vector<UnpackJob> post;
  LGN_TRY(gen_levels_bwd(d, false, P, G, off, a, p4, mask, sc, dq, fin, post, cur, g_lat_s != nullptr, st));
  {
    const int C0 = g.ch[0];
    LGN_TRY(net_unpack(d, false, 0, sc.gX[cur], sc.gs, sc.gv, st));
    const RowLayout ri = enc_input_rows(in_K(d), C0);
    DQ_NEW(part, (size_t)B * ri.width);
    LGN_TRY(enc_input_bwd(B, N, C0, in_K(d), p4, xs, sc.gs, sc.gv, part, st));
    ri.add(dq, part, B, G, off);
  }
  if (hand_dq) {
    LGN_CHECK_ARG(post.empty() && hand_fin && hand_fin->n + fin.n <= (int)(sizeof(fin.it) / sizeof(fin.it[0])), "encoder_bwd: hand-over");
    hand_dq->segs.insert(hand_dq->segs.end(), dq.segs.begin(), dq.segs.end());
    for (int i = 0; i < fin.n; ++i) hand_fin->it[hand_fin->n++] = fin.it[i];
    return 0;
  }
  LGN_TRY(dq.flush(st));
  LGN_TRY(run_unpack_jobs(post, st));
  LGN_TRY(rad_finalize_batch(fin, st));
  return 0;
}

// forward up to the unpacked last-level features (the caller applies dec_output_fwd or the fused output + loss kernel)
int gen_decoder_fwd(const lgn_net_desc& d, const double* P, const int64_t* off, const double* lat_v, GenAct& a, hipStream_t st,
                    bool with_input = true) {
  const GenGeom g = geom(d, true);
  const int L = d.n_levels;
  if (with_input) LGN_TRY(dec_input_fwd(d.B, d.N, g.ch[0], dec_tin(d), lat_v, P + off[1], P + off[2], P + off[3], a.pdec, a.s0, a.v0, st));
  LGN_TRY(net_pack(d, true, 0, a.s0, a.v0, a.X[0], st));
  LGN_TRY(gen_levels_fwd(d, true, P, off, a, a.pdec, nullptr, st));
  LGN_TRY(net_unpack(d, true, L, a.X[L], a.sL, a.vL, st));
  return 0;
}

// sc.gv holds the gradient w.r.t. the last level's (1,1) features (from dec_output_bwd / dec_output_loss); dq carries the
// caller's pending reductions and is flushed by the caller
// part_in (whole step): the input stage's backward is the caller's (junction kernel) -- its partial rows are allocated and their
// reductions registered here, *part_in tells the caller where they go
int gen_decoder_bwd(const lgn_net_desc& d, const double* P, double* G, const int64_t* off, const double* lat_v, const GenAct& a,
                    double* g_lat_v, GenScratch& sc, Deferred& dq, RadFinJob& fin, std::vector<UnpackJob>& post, hipStream_t st,
                    double** part_in = nullptr) {
  const GenGeom g = geom(d, true);
  const int L = d.n_levels, B = d.B, N = d.N, Tin = dec_tin(d);
  int cur = 0;
  LGN_TRY(net_pack(d, true, L, sc.zero0, sc.gv, sc.gX[cur], st));
  LGN_TRY(gen_levels_bwd(d, true, P, G, off, a, a.pdec, nullptr, sc, dq, fin, post, cur, /*has_s_grad=*/false, st));
  if (is_sep_fused(d, true)) {     // d p of the levels: per-channel parts -> sc.g_p (zero on entry), in level and channel order
    const double* gpb[4];
    int cl[4];
    for (int l = 0; l < L; ++l) { gpb[l] = sc.gpb[L - 1 - l]; cl[l] = g.ch[L - 1 - l]; }      // (the order the levels ran in)
    LGN_TRY(local_sep_gp_reduce(gpb, cl, L, B * N, sc.g_p, st));
  }
  const int C0 = g.ch[0];
  const RowLayout ri = dec_input_rows(C0, N, Tin);
  LGN_TRY(net_unpack(d, true, 0, sc.gX[cur], sc.gs, sc.gv, st));
  DQ_NEW(part, (size_t)B * ri.width);
  if (part_in) *part_in = part;
  else LGN_TRY(dec_input_bwd(B, N, C0, Tin, lat_v, P + off[1], P + off[3], a.pdec, sc.g_p, sc.gs, sc.gv, g_lat_v, part, st));
  ri.add(dq, part, B, G, off);
  return 0;
}

// ---------------------------------------------------------------------------------------------------------
// one network at a time (module API: LGNEncoder.forward / LGNDecoder.forward and their autograd backward): the two buffers of a
// maxdim-2 network (the table-driven ones are carve_gen_act / carve_gen_scratch above)
// ---------------------------------------------------------------------------------------------------------
struct NetAct {                     // written by *_fwd, read by *_bwd
  NetBuf n;
  double* pdec;                     // decoder: complex canonical positions [2][B][N][4]
  int* idx;                         // encoder: pooling indices
  size_t total;
};
NetAct carve_act(const lgn_net_desc& d, bool dec, double* base) {
  NetAct a{};
  Bump b{base};
  const size_t BN = (size_t)d.B * d.N;
  carve_net(b, d, dec, BN, /*last_mlp_bwd=*/true, a.n);
  if (dec) a.pdec = b.take(8 * BN);
  else a.idx = reinterpret_cast<int*>(b.take(pool_idx_doubles(d)));
  a.total = b.off;
  return a;
}

struct NetScratch : BwdScratch {    // backward only
  size_t total;
};
NetScratch carve_scratch(const lgn_net_desc& d, bool dec, double* base) {
  NetScratch s{};
  Bump b{base};
  const size_t BN = (size_t)d.B * d.N;
  const int L = d.n_levels;
  const int* ch = dec ? d.dec_channels : d.enc_channels;
  const int cmax = *std::max_element(ch, ch + L + 1);
  {  // zero-initialised block FIRST: a caller that places `grads` right in front of the scratch gets one memset for both
    const size_t z0 = b.off;
    s.tail_cnt = b.take(8);
    s.zeros_s = b.take(2 * BN * cmax);
    s.g_p = b.take(dec ? 8 * BN : 0);
    s.g_lat_s = b.take(dec ? 0 : lat_s_doubles(d));
    s.zero_doubles = b.off - z0;
  }
  carve_level_grads(b, BN, cmax, s);
  for (int l = 0; l < L; ++l) s.tot[l] = b.take(tot_doubles(ch[l], dec));      // (the decoder's: nothing reads them)
  s.parts_size = net_parts(d, dec, d.N);
  s.parts = b.take(s.parts_size);
  s.total = b.off;
  return s;
}

// ---------------------------------------------------------------------------------------------------------
// training steps
// ---------------------------------------------------------------------------------------------------------
struct StepNets {                   // what the forward of a whole maxdim-2 step runs on, training and evaluation alike
  NetBuf enc, dec;
  double *lat_s, *lat_v, *pdec;
  int* idx;
};
struct Work : StepNets {
  double* g_lat_v;
  BwdScratch k;                     // one for both networks
  size_t total;
};
Work carve(const lgn_net_desc& d, double* base) {
  Work w{};
  Bump b{base};
  const int Nd = dec_nodes(d), Nmax = d.N > Nd ? d.N : Nd;
  const size_t BN = (size_t)d.B * Nmax;
  const int L = d.n_levels;
  const int cmax = std::max(*std::max_element(d.enc_channels, d.enc_channels + L + 1), *std::max_element(d.dec_channels, d.dec_channels + L + 1));
  carve_net(b, d, false, (size_t)d.B * d.N, /*last_mlp_bwd=*/false, w.enc);
  carve_net(b, d, true, (size_t)d.B * Nd, /*last_mlp_bwd=*/false, w.dec);
  w.lat_s = b.take(lat_s_doubles(d));
  w.lat_v = b.take(lat_v_doubles(d));
  w.g_lat_v = b.take(lat_v_doubles(d));
  w.pdec = b.take(8 * BN);
  BwdScratch& k = w.k;
  carve_level_grads(b, BN, cmax, k);
  {  // contiguous zero-initialised region
    const size_t z0 = b.off;
    k.zeros_s = b.take(2 * BN * cmax);
    k.g_p = b.take(8 * BN);
    k.g_lat_s = b.take(lat_s_doubles(d));
    k.tail_cnt = b.take(8);
    k.zero_doubles = b.off - z0;
  }
  w.idx = reinterpret_cast<int*>(b.take(pool_idx_doubles(d)));
  for (int l = 0; l < L; ++l) k.tot[l] = b.take(tot_doubles(d.enc_channels[l], false));
  for (int l = 0; l < L; ++l) b.take(tot_doubles(d.dec_channels[l], true));      // (nothing reads these: kept so that no buffer moves)
  // partial rows: every producer keeps its own slice until the deferred reduction at the end of the step
  k.parts_size = net_parts(d, false, d.N) + net_parts(d, true, Nd);
  k.parts = b.take(k.parts_size);
  w.total = b.off;
  return w;
}

// Forward of a whole maxdim-2 step up to the decoder's last level, training and evaluation alike.  Two forms of the same level stacks:
//   fused: both networks on the same N nodes, the mass the only input scalar -- the encoder's input stage (and ride's clears) rides on
//          its first level's kernel, the latent stage and the decoder's input stage are one junction kernel;
//   split (step_is_split: jet_features gives the encoder N + 1 nodes, lgn/models/lgn_encoder.py:372-411; data['scalars'] more input
//          scalars): the four end stages are launches of their own, each on its network's node count, and nothing rides on the encoder.
// dd: the decoder's view of the descriptor (N = dec_nodes).  keep_s: the latent scalars are returned -- otherwise nobody reads them
// (the decoder never does): the encoder's last CGMLP does not run and the latent stage takes its scalars as zero
// (LatentStage).  The decoder's last CGMLP never runs.
int autoencoder_fwd(const lgn_net_desc& d, const lgn_net_desc& dd, const double* params, const int64_t* enc_off, const int64_t* dec_off,
                    const double* p4, const uint8_t* mask, const double* in_scalars, StepNets& w, const InputStage& ride,
                    const LossStage* loss, bool eval, bool keep_s, hipStream_t st) {
  const Slots S{d.n_levels, d.mlp_nlin};
  const int L = d.n_levels;
  const bool split = step_is_split(d);
  LGN_TRY(encoder_fwd(d, params, enc_off, p4, mask, in_scalars, w.enc, w.lat_s, w.lat_v, w.idx, st, split ? nullptr : &ride,
                      /*with_latent=*/split, eval, keep_s));
  if (!split)
    LGN_TRY(junction_fwd(d.B, d.N, d.enc_channels[L], d.tau_s, d.tau_v, d.latent_pool, keep_s ? w.enc.s[L] : nullptr, w.enc.v[L],
                         params + enc_off[S.out0(false)], params + enc_off[S.out0(false) + 1], w.lat_s, w.lat_v, w.idx, d.dec_channels[0],
                         params + dec_off[1], params + dec_off[2], params + dec_off[3], w.pdec, w.dec.s[0], w.dec.v[0], st));
  return decoder_fwd(dd, params, dec_off, w.lat_v, w.dec, w.pdec, st, /*with_input=*/split, loss, eval, /*last_scalars=*/false);
}

// ---- whole training step on table-driven networks -------------------------------------------------------------------
struct GenStep {
  GenAct ea, da;
  GenScratch es, ds;
  double *lat_s, *lat_v, *g_lat_v;
  size_t total;
};
// (each network's activations, scratch and partial rows on its own node count: the decoder's through dd = dec_view(d))
GenStep carve_gen_step(const lgn_net_desc& d, double* base) {
  GenStep g{};
  Bump b{base};
  const lgn_net_desc dd = dec_view(d);
  g.ea = carve_gen_act(d, false, b.here()); b.take(g.ea.total);
  g.da = carve_gen_act(dd, true, b.here()); b.take(g.da.total);
  g.es = carve_gen_scratch(d, false, b.here()); b.take(g.es.total);
  g.ds = carve_gen_scratch(dd, true, b.here()); b.take(g.ds.total);
  g.lat_s = b.take(lat_s_doubles(d));
  g.lat_v = b.take(lat_v_doubles(d));        // (= the dec_tin(d) vectors the decoder reads: check_latent_match)
  g.g_lat_v = b.take(lat_v_doubles(d));
  g.total = b.off;
  return g;
}

// forward of a whole table-driven step up to the decoder's unpacked last-level features, training and evaluation alike.  Two forms,
// as autoencoder_fwd has them: the encoder's latent stage + the decoder's input stage of a jet as ONE launch (the junction kernel of
// the maxdim-2 step), or, split (step_is_split: two node counts, several input scalars), as launches of their own, each on its
// network's node count.  dd: the decoder's view of the descriptor (dec_view)
int gen_autoencoder_fwd(const lgn_net_desc& d, const lgn_net_desc& dd, const double* params, const int64_t* enc_off, const int64_t* dec_off,
                        const double* p4, const uint8_t* mask, const double* in_scalars, GenAct& ea, GenAct& da, double* lat_s,
                        double* lat_v, hipStream_t st) {
  const Slots S{d.n_levels, d.mlp_nlin};
  if (step_is_split(d)) {
    LGN_TRY(gen_encoder_fwd(d, params, enc_off, p4, mask, ea, lat_s, lat_v, st, in_scalars, /*with_latent=*/true));
    return gen_decoder_fwd(dd, params, dec_off, lat_v, da, st, /*with_input=*/true);
  }
  LGN_TRY(gen_encoder_fwd(d, params, enc_off, p4, mask, ea, lat_s, lat_v, st, nullptr, /*with_latent=*/false));
  LGN_TRY(junction_fwd(d.B, d.N, d.enc_channels[d.n_levels], d.tau_s, d.tau_v, d.latent_pool, ea.sL, ea.vL, params + enc_off[S.out0(false)],
                       params + enc_off[S.out0(false) + 1], lat_s, lat_v, ea.idx, d.dec_channels[0], params + dec_off[1], params + dec_off[2],
                       params + dec_off[3], da.pdec, da.s0, da.v0, st));
  return gen_decoder_fwd(d, params, dec_off, lat_v, da, st, /*with_input=*/false);
}

int gen_step_fwd_bwd(const lgn_net_desc& d, const double* params, double* grads, long long n_params, const int64_t* enc_off,
                     const int64_t* dec_off, const double* p4, const double* target, const uint8_t* mask, const double* in_scalars,
                     double* workspace, long long workspace_doubles, double* recon, double* loss_part, hipStream_t st,
                     const StepTailArgs* tail, const StageLoss* al) {
  LGN_CHECK_ARG(is_generic(d, false) && is_generic(d, true), "step: encoder and decoder must both be table-driven (or both fused)");
  if (int rc = check_generic(d, false)) return rc;
  if (int rc = check_generic(d, true)) return rc;
  GenStep g = carve_gen_step(d, workspace);
  LGN_CHECK_ARG((long long)g.total <= workspace_doubles, "step: workspace holds %lld doubles, this configuration needs %zu",
                workspace_doubles, g.total);
  if (int rc = check_mlp_contiguous(d, false, enc_off)) return rc;
  if (int rc = check_mlp_contiguous(d, true, dec_off)) return rc;
  const Slots S{d.n_levels, d.mlp_nlin};
  const lgn_net_desc dd = dec_view(d);       // (the carve made the same one)
  const bool split = step_is_split(d);
  const int L = d.n_levels, B = d.B, N = dd.N, CL = d.dec_channels[L];       // N: the decoder's nodes -- what the loss stages run on
  LGN_TRY(zero_ranges(grads, (size_t)n_params, g.es.zero0, g.es.zero_doubles, g.ds.zero0, g.ds.zero_doubles, st));
  LGN_TRY(gen_autoencoder_fwd(d, dd, params, enc_off, dec_off, p4, mask, in_scalars, g.ea, g.da, g.lat_s, g.lat_v, st));
  Deferred dq(g.ds.parts, g.ds.parts_size);
  RadFinJob fin{};
  {
    const RowLayout ro = dec_output_rows(d, CL);
    DQ_NEW(part, (size_t)B * ro.width);
    if (stage_keeps_chamfer(al))
      LGN_TRY(dec_output_loss(B, N, CL, g.da.vL, params + dec_off[S.out0(true) + 1], target, chamfer_scale(al), d.get_real,
                              d.jet_loss_scale, recon, loss_part, g.ds.gv, part, st));
    if (al)
      LGN_TRY(stage_loss_train(*al, B, N, CL, g.da.vL, params + dec_off[S.out0(true) + 1], target, d.get_real, recon, loss_part, g.ds.gv,
                               part, st));
    ro.add(dq, part, B, grads, dec_off);
  }
  std::vector<UnpackJob> post;
  double* part_in = nullptr;
  // split: the decoder's input stage backward is gen_decoder_bwd's own launch (part_in stays null), the latent stage's the encoder's
  LGN_TRY(gen_decoder_bwd(dd, params, grads, dec_off, g.lat_v, g.da, g.g_lat_v, g.ds, dq, fin, post, st, split ? nullptr : &part_in));
  const int Tin = dec_tin(d), C0d = d.dec_channels[0];
  const JunctionBwd jb{C0d, Tin, g.lat_v, params + dec_off[1], params + dec_off[3], g.da.pdec, g.ds.g_p, g.ds.gs, g.ds.gv, part_in};
  // Round 6: the static levels leave their CatMix partial rows in PARAMETER layout (nothing to unpack after the reduction), so the
  // two networks' reductions wait for ONE launch at the end of the step -- with `tail` (single process) the fused tail of the
  // maxdim-2 step (step_tail.hip: reductions + radial finalisation + L1 + Adam + loss), else reduce_segments + rad_finalize_batch.
  // Run-time-table levels (LGN_NET_NO_STATIC) keep packed rows and the round-5 sequence.
  // (split: either network alone may be on run-time tables -- the encoder's one node more crosses N = 32 first)
  if (!post.empty() || !is_static(d, false) || !is_static(dd, true)) {
    // (the decoder's reductions run now: its input stage's backward must have written its partial rows -- no junction kernel here)
    if (!split)
      LGN_TRY(dec_input_bwd(B, N, C0d, Tin, g.lat_v, params + dec_off[1], params + dec_off[3], g.da.pdec, g.ds.g_p, g.ds.gs, g.ds.gv, g.g_lat_v,
                            part_in, st));
    LGN_TRY(dq.flush(st));
    LGN_TRY(run_unpack_jobs(post, st));
    // the decoder never reads the latent scalars: no gradient on them
    LGN_TRY(gen_encoder_bwd(d, params, grads, enc_off, p4, mask, g.ea, nullptr, g.g_lat_v, g.es, st, split ? in_scalars : nullptr));
    if (tail) LGN_TRY(finalize_tail(*tail, st));
    return 0;
  }
  LGN_TRY(gen_encoder_bwd(d, params, grads, enc_off, p4, mask, g.ea, nullptr, g.g_lat_v, g.es, st, split ? in_scalars : nullptr, &dq, &fin,
                          split ? nullptr : &jb));
  return end_step(dq, fin, grads, n_params, /*counters=*/nullptr, d.flags, tail, st);
}

// forward + backward of a training step, ended by end_step: argument checks, a carve, autoencoder_fwd, the loss, decoder_bwd and
// encoder_bwd on one BwdScratch.  In the fused form the first kernel also clears the gradients and the zero block, the loss rides on
// the decoder's last level where that is one workgroup per jet, and the two stages between the networks are one junction kernel
// in each direction; in the split form (autoencoder_fwd) every end stage is a launch of its own.
int step_fwd_bwd(const lgn_net_desc* dp, const double* params, double* grads, long long n_params, const int64_t* enc_off,
                 const int64_t* dec_off, const double* p4, const double* target, const uint8_t* mask, const double* in_scalars,
                 double* workspace, long long workspace_doubles, double* recon, double* loss_part, void* stream,
                 const StepTailArgs* tail, const StageLoss* al = nullptr) {
  if (int rc = check_desc(dp)) return rc;
  const lgn_net_desc& d = *dp;
  LGN_CHECK_ARG(params && grads && enc_off && dec_off && p4 && target && mask && workspace && recon && loss_part && n_params > 0,
                "step_fwd_bwd: null pointer");
  LGN_CHECK_ARG(d.n_in_scalars <= 1 || in_scalars, "step_fwd_bwd: %d input scalars per node, but in_scalars is NULL", d.n_in_scalars);
  if (int rc = check_latent_match(d)) return rc;
  hipStream_t st = (hipStream_t)stream;
  const bool split = step_is_split(d);
  if (is_generic(d, false) || is_generic(d, true)) {
    return gen_step_fwd_bwd(d, params, grads, n_params, enc_off, dec_off, p4, target, mask, in_scalars, workspace, workspace_doubles,
                            recon, loss_part, st, tail, al);
  }
  Work w = carve(d, workspace);
  // the layout depends on run-time switches (LGN_AMD_DEC_PAIRWISE / LGN_AMD_LEVEL_V2 change the partial-row counts):
  // refuse before anything is enqueued if the caller sized the workspace under different settings
  LGN_CHECK_ARG((long long)w.total <= workspace_doubles, "step: workspace holds %lld doubles, this configuration needs %zu",
                workspace_doubles, w.total);
  // MLP parameter blocks must be contiguous (W_0, b_0, W_1, b_1, ...) for the single-reduce path
  if (int rc = check_mlp_contiguous(d, false, enc_off)) return rc;
  if (int rc = check_mlp_contiguous(d, true, dec_off)) return rc;
  const lgn_net_desc dd = dec_view(d);
  const Slots S{d.n_levels, d.mlp_nlin};
  const int B = d.B, Nd = dd.N, CL = d.dec_channels[d.n_levels];
  BwdScratch& k = w.k;
  Deferred dq(k.parts, k.parts_size);
  RadFinJob fin{};
  int cur = 0;

  // ---------------- forward, loss (and its backward) ----------------
  const RowLayout ro = dec_output_rows(d, CL);
  DQ_NEW(part, (size_t)B * ro.width);
  const bool chamfer = stage_keeps_chamfer(al);
  const LossStage ls{params + dec_off[S.out0(true) + 1], target, chamfer_scale(al), d.get_real, d.jet_loss_scale, recon, loss_part, k.gv[cur], part};
  const bool rides = chamfer && level_fwd_carries_loss(Nd, d.flags);  // (a StageLoss is a launch of its own in every regime)
  // fused: the first kernel also zeroes the gradient buffer (dead parameters keep an exact zero) and zeros_s | g_p | g_lat_s | tail_cnt
  const InputStage in0{params + enc_off[0], params + enc_off[1], grads, (size_t)n_params, k.zeros_s, k.zero_doubles};
  if (split) LGN_TRY(zero_ranges(grads, (size_t)n_params, k.zero0(), k.zero_doubles, nullptr, 0, st));
  LGN_TRY(autoencoder_fwd(d, dd, params, enc_off, dec_off, p4, mask, in_scalars, w, in0, rides ? &ls : nullptr, /*eval=*/false,
                          /*keep_s=*/false, st));
  if (chamfer && !rides)
    LGN_TRY(dec_output_loss(B, Nd, CL, w.dec.v[d.n_levels], ls.wo1, target, chamfer_scale(al), ls.method, ls.jscale, recon, loss_part,
                            k.gv[cur], part, st));
  if (al)
    LGN_TRY(stage_loss_train(*al, B, Nd, CL, w.dec.v[d.n_levels], ls.wo1, target, ls.method, recon, loss_part, k.gv[cur], part, st));
  ro.add(dq, part, B, grads, dec_off);

  // ---------------- backward ----------------
  // fused: the junction kernel reads the gradient w.r.t. the decoder's level-0 features and writes the one w.r.t. the encoder's last
  // level into the other buffer pair (jets do not occupy the same slices when the two channel counts differ); the split form's two
  // launches do the same.  The decoder never reads the latent scalars: their gradient is the zero block's g_lat_s.
  double* part_in = nullptr;
  LGN_TRY(decoder_bwd(dd, params, grads, dec_off, w.lat_v, w.dec, w.pdec, w.g_lat_v, k, cur, dq, fin, st, split ? nullptr : &part_in));
  const JunctionBwd jb{d.dec_channels[0], dec_tin(d), w.lat_v, params + dec_off[1], params + dec_off[3], w.pdec, k.g_p, k.gs[cur], k.gv[cur], part_in};
  // the input stage's backward rides on the first level's where it can -- fused form only (split: its own launch, even with K = 1)
  LGN_TRY(encoder_bwd(d, params, grads, enc_off, p4, mask, split ? in_scalars : nullptr, w.enc, w.idx, nullptr, w.g_lat_v, k, cur ^ 1, dq, fin,
                      st, /*ride_in0=*/!split, /*last_scalars=*/false, split ? nullptr : &jb));
  return end_step(dq, fin, grads, n_params, k.tail_cnt, d.flags, tail, st);
}

// the tail of a call with an optimiser descriptor; refuses what no kernel implements before anything is enqueued
int optim_tail(const lgn_optim_desc* o, double* params, double* grads, long long n_params, double* state_m, double* state_v,
               long long* step_dev, int do_step, const double* loss_part, int n_loss, double* loss_out, StepTailArgs& t) {
  LGN_CHECK_ARG(o, "optimiser descriptor: null pointer");
  LGN_CHECK_ARG(o->kind == LGN_OPT_ADAM || o->kind == LGN_OPT_RMSPROP, "optimiser descriptor: kind %d is neither LGN_OPT_ADAM nor "
                "LGN_OPT_RMSPROP", o->kind);
  LGN_CHECK_ARG(!do_step || (state_m && state_v && step_dev), "optimiser state missing");
  LGN_CHECK_ARG(o->l2_lambda >= 0.0 && o->eps >= 0.0, "optimiser descriptor: negative l2_lambda or eps");
  LGN_CHECK_ARG(o->kind != LGN_OPT_RMSPROP || (o->alpha >= 0.0 && o->alpha <= 1.0 && o->momentum >= 0.0),
                "optimiser descriptor: RMSprop takes 0 <= alpha <= 1 and momentum >= 0");
  t = StepTailArgs{params, grads, (long)n_params, state_m, state_v, reinterpret_cast<long*>(step_dev), o->l1_lambda, o->lr, o->beta1,
                   o->beta2, o->eps, do_step, loss_part, n_loss, loss_out, 0, nullptr};
  t.opt_form = 1;
  t.kind = o->kind;
  t.l2 = o->l2_lambda;
  t.alpha = o->alpha;
  t.mu = o->momentum;
  return 0;
}

// ---------------------------------------------------------------------------------------------------------
// evaluation step (the reference's validate() / test.py loop under torch.no_grad(), utils/train.py:390): encoder -> decoder ->
// get_real -> Chamfer [+ jet-feature term] forward only, no L1 (regularization = is_train, utils/train.py:308-314).  Nothing is
// kept for a backward: two feature buffers per network used in turn, level kernels without the aggregate stores, the CGMLPs on
// their no-save path, no CGMLP after the decoder's last level, a loss tail that writes no gradient.
// ---------------------------------------------------------------------------------------------------------
struct EvalWork : StepNets {        // s / v of level l point to feature buffer l & 1 of the network; smix one buffer for all levels
  size_t total;
};
EvalWork carve_eval(const lgn_net_desc& d, double* base) {
  EvalWork w{};
  Bump b{base};
  const int L = d.n_levels, Nd = dec_nodes(d);
  const size_t BNe = (size_t)d.B * d.N, BNd = (size_t)d.B * Nd;
  size_t smix = 0;
  auto net = [&](NetBuf& n, const int* ch, size_t BN) {
    const int cmax = *std::max_element(ch, ch + L + 1);
    double *s[2], *v[2];
    for (int q = 0; q < 2; ++q) {
      s[q] = b.take(2 * BN * cmax);
      v[q] = b.take(8 * BN * cmax);
    }
    for (int l = 0; l <= L; ++l) {
      n.s[l] = s[l & 1];
      n.v[l] = v[l & 1];
    }
    smix = std::max(smix, 2 * BN * cmax);
  };
  net(w.enc, d.enc_channels, BNe);
  net(w.dec, d.dec_channels, BNd);
  double* sm = b.take(smix);
  for (int l = 0; l < L; ++l) w.enc.smix[l] = w.dec.smix[l] = sm;
  w.lat_s = b.take(lat_s_doubles(d));
  w.lat_v = b.take(lat_v_doubles(d));
  w.pdec = b.take(8 * BNd);
  w.idx = reinterpret_cast<int*>(b.take(pool_idx_doubles(d)));
  w.total = b.off;
  return w;
}

// table-driven networks: the training forward (gen_autoencoder_fwd) on activations of their own -- those kernels
// store what their backward would read; no-keep forms of them are not part of the evaluation step yet
struct GenEval {
  GenAct ea, da;
  double *lat_s, *lat_v;
  size_t total;
};
GenEval carve_gen_eval(const lgn_net_desc& d, double* base) {
  GenEval g{};
  Bump b{base};
  g.ea = carve_gen_act(d, false, b.here()); b.take(g.ea.total);
  g.da = carve_gen_act(dec_view(d), true, b.here()); b.take(g.da.total);
  g.lat_s = b.take(lat_s_doubles(d));
  g.lat_v = b.take(lat_v_doubles(d));
  g.total = b.off;
  return g;
}

long long eval_workspace(const lgn_net_desc& d) {
  if (is_generic(d, false) || is_generic(d, true)) {
    if (check_generic(d, false) || check_generic(d, true)) return -1;
    return (long long)carve_gen_eval(d, nullptr).total;
  }
  return (long long)carve_eval(d, nullptr).total;
}

int step_eval(const lgn_net_desc* dp, const double* params, const int64_t* enc_off, const int64_t* dec_off, const double* p4,
              const double* target, const uint8_t* mask, const double* in_scalars, double* workspace, long long workspace_doubles,
              double* recon_real, double* lat_s_out, double* lat_v_out, double* loss_part, double* loss_out, hipStream_t st,
              const StageLoss* al) {
  // every refusal comes before the first launch
  if (int rc = check_desc(dp)) return rc;
  const lgn_net_desc& d = *dp;
  LGN_CHECK_ARG(params && enc_off && dec_off && p4 && target && mask && workspace && recon_real && loss_part && loss_out,
                "step_eval: null pointer");
  LGN_CHECK_ARG(d.n_in_scalars <= 1 || in_scalars, "step_eval: %d input scalars per node, but in_scalars is NULL", d.n_in_scalars);
  LGN_CHECK_ARG(!lat_s_out == !lat_v_out, "step_eval: give both latent outputs or neither");
  if (int rc = check_latent_match(d)) return rc;
  const long long need = eval_workspace(d);
  if (need < 0) return -1;
  LGN_CHECK_ARG(need <= workspace_doubles, "step_eval: workspace holds %lld doubles, this configuration needs %lld", workspace_doubles, need);
  if (int rc = check_mlp_contiguous(d, false, enc_off)) return rc;
  if (int rc = check_mlp_contiguous(d, true, dec_off)) return rc;
  const int B = d.B, Ne = d.N, Nd = dec_nodes(d), CL = d.dec_channels[d.n_levels];
  const double* wo1 = params + dec_off[Slots{d.n_levels, d.mlp_nlin}.out0(true) + 1];
  const double* vL;                  // the decoder's last-level vectors
  bool rides = false;                // output + loss rode on the decoder's last level
  const bool chamfer = stage_keeps_chamfer(al);
  if (is_generic(d, false) || is_generic(d, true)) {
    LGN_CHECK_ARG(is_generic(d, false) && is_generic(d, true), "step_eval: encoder and decoder must both be table-driven (or both fused)");
    GenEval g = carve_gen_eval(d, workspace);
    LGN_TRY(gen_autoencoder_fwd(d, dec_view(d), params, enc_off, dec_off, p4, mask, in_scalars, g.ea, g.da, lat_s_out ? lat_s_out : g.lat_s,
                                lat_v_out ? lat_v_out : g.lat_v, st));
    vL = g.da.vL;
  } else {
    EvalWork w = carve_eval(d, workspace);
    if (lat_s_out) { w.lat_s = lat_s_out; w.lat_v = lat_v_out; }
    const lgn_net_desc dd = dec_view(d);
    const LossStage loss{wo1, target, 1.0, d.get_real, d.jet_loss_scale, recon_real, loss_part, nullptr, nullptr};
    rides = chamfer && level_fwd_carries_loss(Nd, d.flags);
    const InputStage in0{params + enc_off[0], params + enc_off[1]};
    // the latent scalars (the encoder's last CGMLP and what the latent stage makes of its output) only when they are returned
    LGN_TRY(autoencoder_fwd(d, dd, params, enc_off, dec_off, p4, mask, in_scalars, w, in0, rides ? &loss : nullptr, /*eval=*/true,
                            /*keep_s=*/lat_s_out != nullptr, st));
    vL = w.dec.v[d.n_levels];
  }
  if (chamfer && !rides) LGN_TRY(dec_output_eval(B, Nd, CL, vL, wo1, target, d.get_real, d.jet_loss_scale, recon_real, loss_part, st));
  if (al) LGN_TRY(stage_loss_eval(*al, B, Nd, CL, vL, wo1, target, d.get_real, recon_real, loss_part, st));
  return eval_loss_sum(B, Ne, mask, loss_part, loss_out, st);
}

}  // namespace
}  // namespace lgn

using namespace lgn;

extern "C" {

// ---- one network at a time ----------------------------------------------------------------------------------------------
long long lgn_net_workspace_doubles(const lgn_net_desc* d, int decoder, int which) {
  if (check_desc(d)) return -1;
  if (is_generic(*d, decoder != 0)) {
    if (check_generic(*d, decoder != 0)) return -1;
    return which == 0 ? (long long)carve_gen_act(*d, decoder != 0, nullptr).total : (long long)carve_gen_scratch(*d, decoder != 0, nullptr).total;
  }
  return which == 0 ? (long long)carve_act(*d, decoder != 0, nullptr).total : (long long)carve_scratch(*d, decoder != 0, nullptr).total;
}

int lgn_encoder_fwd_f64(const lgn_net_desc* d, const double* params, const int64_t* off, const double* p4, const uint8_t* mask,
                        const double* in_scalars, double* act, long long act_doubles, double* lat_s, double* lat_v, void* stream) {
  if (int rc = check_desc(d)) return rc;
  LGN_CHECK_ARG(params && off && p4 && mask && act && lat_s && lat_v, "encoder_fwd: null pointer");
  LGN_CHECK_ARG(d->n_in_scalars <= 1 || in_scalars, "encoder_fwd: %d input scalars per node, but in_scalars is NULL", d->n_in_scalars);
  if (is_generic(*d, false)) {
    if (int rc = check_generic(*d, false)) return rc;
    GenAct ga = carve_gen_act(*d, false, act);
    LGN_CHECK_ARG((long long)ga.total <= act_doubles, "encoder_fwd: activation buffer holds %lld doubles, needs %zu", act_doubles, ga.total);
    return gen_encoder_fwd(*d, params, off, p4, mask, ga, lat_s, lat_v, (hipStream_t)stream, in_scalars);
  }
  NetAct a = carve_act(*d, false, act);
  LGN_CHECK_ARG((long long)a.total <= act_doubles, "encoder_fwd: activation buffer holds %lld doubles, needs %zu", act_doubles, a.total);
  // the input stage rides on the first level's kernel; several input scalars: it is a launch of its own
  const InputStage in0{params + off[0], params + off[1]};
  return encoder_fwd(*d, params, off, p4, mask, in_scalars, a.n, lat_s, lat_v, a.idx, (hipStream_t)stream, in_K(*d) > 1 ? nullptr : &in0);
}

int lgn_encoder_bwd_f64(const lgn_net_desc* d, const double* params, double* grads, long long n_params, const int64_t* off,
                        const double* p4, const uint8_t* mask, const double* in_scalars, const double* act, long long act_doubles,
                        const double* g_lat_s, const double* g_lat_v, double* scratch, long long scratch_doubles, void* stream) {
  if (int rc = check_desc(d)) return rc;
  LGN_CHECK_ARG(params && grads && off && p4 && mask && act && g_lat_v && scratch && n_params > 0, "encoder_bwd: null pointer");
  LGN_CHECK_ARG(d->n_in_scalars <= 1 || in_scalars, "encoder_bwd: %d input scalars per node, but in_scalars is NULL", d->n_in_scalars);
  hipStream_t st = (hipStream_t)stream;
  if (is_generic(*d, false)) {
    if (int rc = check_generic(*d, false)) return rc;
    GenAct ga = carve_gen_act(*d, false, const_cast<double*>(act));
    GenScratch gs = carve_gen_scratch(*d, false, scratch);
    LGN_CHECK_ARG((long long)ga.total <= act_doubles && (long long)gs.total <= scratch_doubles,
                  "encoder_bwd: buffers hold %lld / %lld doubles, need %zu / %zu", act_doubles, scratch_doubles, ga.total, gs.total);
    if (int rc = check_mlp_contiguous(*d, false, off)) return rc;
    LGN_TRY(zero_grads_and_block(grads, (size_t)n_params, gs.zero0, gs.zero_doubles, st));
    return gen_encoder_bwd(*d, params, grads, off, p4, mask, ga, g_lat_s, g_lat_v, gs, st, in_scalars);
  }
  NetAct a = carve_act(*d, false, const_cast<double*>(act));
  NetScratch sc = carve_scratch(*d, false, scratch);
  LGN_CHECK_ARG((long long)a.total <= act_doubles && (long long)sc.total <= scratch_doubles,
                "encoder_bwd: buffers hold %lld / %lld doubles, need %zu / %zu", act_doubles, scratch_doubles, a.total, sc.total);
  if (int rc = check_mlp_contiguous(*d, false, off)) return rc;
  LGN_TRY(zero_grads_and_block(grads, (size_t)n_params, sc.zero0(), sc.zero_doubles, st));
  Deferred dq(sc.parts, sc.parts_size);
  RadFinJob fin{};
  // (several input scalars: the input stage's backward is its own launch, nothing rides)
  LGN_TRY(encoder_bwd(*d, params, grads, off, p4, mask, in_scalars, a.n, a.idx, g_lat_s, g_lat_v, sc, /*cur=*/0, dq, fin, st,
                      /*ride_in0=*/in_K(*d) == 1));
  // (measured at cfg2, captured module step: the one-launch form is 3 us SLOWER for the encoder alone -- 0.5966 against 0.5937 ms)
  return finish_reductions(dq, fin, grads, n_params, nullptr, d->flags, st);
}

int lgn_decoder_fwd_f64(const lgn_net_desc* d, const double* params, const int64_t* off, const double* lat_v, double* act,
                        long long act_doubles, double* recon, void* stream) {
  if (int rc = check_desc(d)) return rc;
  LGN_CHECK_ARG(params && off && lat_v && act && recon, "decoder_fwd: null pointer");
  hipStream_t st = (hipStream_t)stream;
  const int CL = d->dec_channels[d->n_levels];
  const double* wo1 = params + off[Slots{d->n_levels, d->mlp_nlin}.out0(true) + 1];
  if (is_generic(*d, true)) {
    if (int rc = check_generic(*d, true)) return rc;
    GenAct ga = carve_gen_act(*d, true, act);
    LGN_CHECK_ARG((long long)ga.total <= act_doubles, "decoder_fwd: activation buffer holds %lld doubles, needs %zu", act_doubles, ga.total);
    LGN_TRY(gen_decoder_fwd(*d, params, off, lat_v, ga, st));
    return dec_output_fwd(d->B, d->N, CL, ga.vL, wo1, recon, st);
  }
  NetAct a = carve_act(*d, true, act);
  LGN_CHECK_ARG((long long)a.total <= act_doubles, "decoder_fwd: activation buffer holds %lld doubles, needs %zu", act_doubles, a.total);
  LGN_TRY(decoder_fwd(*d, params, off, lat_v, a.n, a.pdec, st));
  return dec_output_fwd(d->B, d->N, CL, a.n.v[d->n_levels], wo1, recon, st);
}

int lgn_decoder_bwd_f64(const lgn_net_desc* d, const double* params, double* grads, long long n_params, const int64_t* off,
                        const double* lat_v, const double* act, long long act_doubles, const double* g_recon, double* g_lat_v,
                        double* scratch, long long scratch_doubles, void* stream) {
  if (int rc = check_desc(d)) return rc;
  LGN_CHECK_ARG(params && grads && off && lat_v && act && g_recon && g_lat_v && scratch && n_params > 0, "decoder_bwd: null pointer");
  hipStream_t st = (hipStream_t)stream;
  const int B = d->B, N = d->N, CL = d->dec_channels[d->n_levels];
  const double* wo1 = params + off[Slots{d->n_levels, d->mlp_nlin}.out0(true) + 1];
  const RowLayout ro = dec_output_rows(*d, CL);
  RadFinJob fin{};
  if (is_generic(*d, true)) {
    if (int rc = check_generic(*d, true)) return rc;
    GenAct ga = carve_gen_act(*d, true, const_cast<double*>(act));
    GenScratch gs = carve_gen_scratch(*d, true, scratch);
    LGN_CHECK_ARG((long long)ga.total <= act_doubles && (long long)gs.total <= scratch_doubles,
                  "decoder_bwd: buffers hold %lld / %lld doubles, need %zu / %zu", act_doubles, scratch_doubles, ga.total, gs.total);
    if (int rc = check_mlp_contiguous(*d, true, off)) return rc;
    LGN_TRY(zero_grads_and_block(grads, (size_t)n_params, gs.zero0, gs.zero_doubles, st));
    Deferred dq(gs.parts, gs.parts_size);
    DQ_NEW(part, (size_t)B * ro.width);
    LGN_TRY(dec_output_bwd(B, N, CL, ga.vL, wo1, g_recon, gs.gv, part, st));
    ro.add(dq, part, B, grads, off);
    std::vector<UnpackJob> post;
    LGN_TRY(gen_decoder_bwd(*d, params, grads, off, lat_v, ga, g_lat_v, gs, dq, fin, post, st));
    LGN_TRY(dq.flush(st));
    return run_unpack_jobs(post, st);
  }
  NetAct a = carve_act(*d, true, const_cast<double*>(act));
  NetScratch sc = carve_scratch(*d, true, scratch);
  LGN_CHECK_ARG((long long)a.total <= act_doubles && (long long)sc.total <= scratch_doubles,
                "decoder_bwd: buffers hold %lld / %lld doubles, need %zu / %zu", act_doubles, scratch_doubles, a.total, sc.total);
  if (int rc = check_mlp_contiguous(*d, true, off)) return rc;
  LGN_TRY(zero_grads_and_block(grads, (size_t)n_params, sc.zero0(), sc.zero_doubles, st));
  Deferred dq(sc.parts, sc.parts_size);
  int cur = 0;
  DQ_NEW(part, (size_t)B * ro.width);
  LGN_TRY(dec_output_bwd(B, N, CL, a.n.v[d->n_levels], wo1, g_recon, sc.gv[cur], part, st));
  ro.add(dq, part, B, grads, off);
  LGN_TRY(decoder_bwd(*d, params, grads, off, lat_v, a.n, a.pdec, g_lat_v, sc, cur, dq, fin, st));
  return finish_reductions(dq, fin, grads, n_params, /*counters=*/nullptr, d->flags, st);
}

// ---- training steps -------------------------------------------------------------------------------------------------------
int lgn_step_param_slots(const lgn_net_desc* d, int decoder) {
  if (check_desc(d)) return -1;
  return Slots{d->n_levels, d->mlp_nlin}.count(decoder != 0);
}

long long lgn_encoder_end_lds_bytes(int N, int C0, int K, int CL, int Ts, int Tv, int pool) {
  return pool_valid(pool) ? (long long)encoder_end_lds_bytes(N, C0, K < 1 ? 1 : K, CL, Ts, Tv, pool) : -1;
}
long long lgn_decoder_end_lds_bytes(int N, int C0, int Tin, int CL) { return (long long)decoder_end_lds_bytes(N, C0, Tin, CL); }
long long lgn_junction_lds_bytes(int N, int CL, int Ts, int Tv, int pool, int C0) {
  return pool_valid(pool) ? (long long)junction_lds_bytes(N, CL, Ts, Tv, pool, C0) : -1;
}

long long lgn_step_workspace_doubles(const lgn_net_desc* d) {
  if (check_desc(d) || check_latent_match(*d)) return -1;
  if (is_generic(*d, false) || is_generic(*d, true)) {
    if (check_generic(*d, false) || check_generic(*d, true)) return -1;
    return (long long)carve_gen_step(*d, nullptr).total;
  }
  return (long long)carve(*d, nullptr).total;
}

int lgn_step_fwd_bwd_f64(const lgn_net_desc* d, const double* params, double* grads, long long n_params, const int64_t* enc_off,
                         const int64_t* dec_off, const double* p4, const double* target, const uint8_t* mask, const double* in_scalars,
                         double* workspace, long long workspace_doubles, double* recon, double* loss_part, const lgn_loss_desc* loss,
                         int* assignment, int* status, void* stream) {
  StageLoss al;
  const StageLoss* alp;
  if (int rc = plan_assign_loss(d, loss, assignment, status, al, &alp)) return rc;
  return step_fwd_bwd(d, params, grads, n_params, enc_off, dec_off, p4, target, mask, in_scalars, workspace, workspace_doubles, recon,
                      loss_part, stream, nullptr, alp);
}

int lgn_step_train_f64(const lgn_net_desc* d, double* params, double* grads, long long n_params, const int64_t* enc_off,
                       const int64_t* dec_off, const double* p4, const double* target, const uint8_t* mask, const double* in_scalars,
                       double* workspace, long long workspace_doubles, double* recon, double* loss_part, int n_loss, double l1_lambda,
                       double* adam_m, double* adam_v, long long* step_dev, double lr, double beta1, double beta2, double eps,
                       int do_adam, double* loss_out, const lgn_loss_desc* loss, int* assignment, int* status, void* stream) {
  StageLoss al;
  const StageLoss* alp;
  if (int rc = plan_assign_loss(d, loss, assignment, status, al, &alp)) return rc;
  LGN_CHECK_ARG(loss_out && n_loss > 0, "step_train: null pointer");
  LGN_CHECK_ARG(!do_adam || (adam_m && adam_v && step_dev), "step_train: Adam state missing");
  const StepTailArgs tail{params, grads, (long)n_params, adam_m, adam_v, reinterpret_cast<long*>(step_dev), l1_lambda, lr, beta1, beta2,
                          eps, do_adam, loss_part, n_loss, loss_out, 0, nullptr};
  // LGN_NET_SPLIT_TAIL (frozen into the descriptor): the three separate launches (reduce_segments, rad_finalize_batch, l1_adam) -- the
  // A/B switch of the fused tail
  return step_fwd_bwd(d, params, grads, n_params, enc_off, dec_off, p4, target, mask, in_scalars, workspace, workspace_doubles, recon,
                      loss_part, stream, &tail, alp);
}

int lgn_step_finalize_f64(double* params, double* grads, long long n_params, const double* loss_part, int n_loss, double l1_lambda,
                          double* adam_m, double* adam_v, long long* step_dev, double lr, double beta1, double beta2, double eps,
                          int do_adam, double* loss_out, void* stream) {
  LGN_CHECK_ARG(params && grads && loss_part && loss_out && n_params > 0 && n_loss > 0, "step_finalize: null pointer");
  LGN_CHECK_ARG(!do_adam || (adam_m && adam_v && step_dev), "step_finalize: Adam state missing");
  hipStream_t st = (hipStream_t)stream;
  LGN_TRY(finalize_step(params, grads, (long)n_params, loss_part, n_loss, l1_lambda, adam_m, adam_v, reinterpret_cast<long*>(step_dev),
                        lr, beta1, beta2, eps, do_adam, loss_out, st));
  return 0;
}

int lgn_step_train_opt_f64(const lgn_net_desc* d, double* params, double* grads, long long n_params, const int64_t* enc_off,
                           const int64_t* dec_off, const double* p4, const double* target, const uint8_t* mask, const double* in_scalars,
                           double* workspace, long long workspace_doubles, double* recon, double* loss_part, int n_loss,
                           const lgn_optim_desc* opt, double* state_m, double* state_v, long long* step_dev, int do_step,
                           double* loss_out, const lgn_loss_desc* loss, int* assignment, int* status, void* stream) {
  StageLoss al;
  const StageLoss* alp;
  if (int rc = plan_assign_loss(d, loss, assignment, status, al, &alp)) return rc;
  LGN_CHECK_ARG(loss_out && n_loss > 0, "step_train_opt: null pointer");
  StepTailArgs tail{};
  if (int rc = optim_tail(opt, params, grads, n_params, state_m, state_v, step_dev, do_step, loss_part, n_loss, loss_out, tail))
    return rc;
  return step_fwd_bwd(d, params, grads, n_params, enc_off, dec_off, p4, target, mask, in_scalars, workspace, workspace_doubles,
                      recon, loss_part, stream, &tail, alp);
}

int lgn_step_finalize_opt_f64(double* params, double* grads, long long n_params, const double* loss_part, int n_loss,
                              const lgn_optim_desc* opt, double* state_m, double* state_v, long long* step_dev, int do_step,
                              double* loss_out, void* stream) {
  LGN_CHECK_ARG(params && grads && loss_part && loss_out && n_params > 0 && n_loss > 0, "step_finalize_opt: null pointer");
  StepTailArgs tail{};
  if (int rc = optim_tail(opt, params, grads, n_params, state_m, state_v, step_dev, do_step, loss_part, n_loss, loss_out, tail))
    return rc;
  return finalize_step_opt(tail, (hipStream_t)stream);
}

// ---- evaluation step ------------------------------------------------------------------------------------------------------
long long lgn_eval_workspace_doubles(const lgn_net_desc* d) {
  if (check_desc(d)) return -1;
  return eval_workspace(*d);
}

int lgn_step_eval_f64(const lgn_net_desc* d, const double* params, const int64_t* enc_off, const int64_t* dec_off,
                      const double* p4_scaled, const double* p4_target, const uint8_t* mask, const double* in_scalars,
                      double* workspace, long long workspace_doubles, double* recon_real, double* lat_s, double* lat_v,
                      double* loss_part, double* loss_out, const lgn_loss_desc* loss, int* assignment, int* status, void* stream) {
  StageLoss al;
  const StageLoss* alp;
  if (int rc = plan_assign_loss(d, loss, assignment, status, al, &alp)) return rc;
  return step_eval(d, params, enc_off, dec_off, p4_scaled, p4_target, mask, in_scalars, workspace, workspace_doubles, recon_real, lat_s,
                   lat_v, loss_part, loss_out, (hipStream_t)stream, alp);
}

}  // extern "C"
