// lgn-autoencoder_amd/csrc/step_ctl.hip -- the guarded finalize of a training step (lgn_step_finalize_ctl_f64 of include/lgn_amd.h):
// gradient-norm clipping (torch.nn.utils.clip_grad_norm_), "leave the state alone if this step is non-finite or blew up" (the
// reference's BLOW_UP_THRESHOLD of utils/train.py, decided on the device because a device-resident epoch has no host in the loop)
// and a learning rate that is read from the device or from a closed-form schedule per step, so that a captured graph follows it.
//
// The update cannot start before the norm of the WHOLE regularised gradient is known, so there are two launches with the launch
// boundary as the only grid-wide wait:
//   ctl_grad_kernel   G = g + l1 sign(w) + 2 l2 w -> grads; per-workgroup partials of |w|, w^2, G^2.  The last workgroup to arrive
//                     (l1_adam_kernel's hand-off: atomic exchange, awaited -> counter; atomic loads on the reading side; no
//                     __threadfence(), for the reason given in step_tail.hip) sums them in index order, assembles the loss, takes
//                     the decision, works out the step's learning rate and Adam's bias corrections, advances the step counter and
//                     keeps the books of the control block.  It leaves the partial slots and the counter at zero.
//   ctl_apply_kernel  reads {apply, coef, lr, bc1, bc2_sqrt} from the control block (plain loads: another launch wrote them) and,
//                     if the step is applied, runs the optimiser's rule on G * coef.  No cross-workgroup traffic at all.
// No workgroup waits for another one in either kernel.  With every control off the arithmetic per parameter is the descriptor
// finalize's, operation for operation (tail_dev.hpp), and Adam's powers are cached in this call's own block under l1_adam_kernel's
// protocol (slot t & 1 = {t, beta1^t, beta2^t}, written by the step before): same bits.
#include "net_dev.hpp"
#include "tail_dev.hpp"
#include "../../include/lgn_amd.h"
#include <math.h>

namespace lgn {
namespace {

constexpr int CTL_PER_THREAD = 4;                                  // as ADAM_PER_THREAD of net_kernels.hip: a quarter of the workgroups at the counter
constexpr int CTL_THIRD = (LGN_FINALIZE_CTL_SCRATCH - 12) / 3;     // partial-sum slots per array

static_assert(LR_COSINE == LGN_LR_WARMUP_COSINE && LR_STEP == LGN_LR_WARMUP_STEP, "tail_dev.hpp names the schedule kinds of lgn_amd.h");

struct CtlArgs {
  long n;
  double *w, *g, *m, *v;
  long* step_dev;
  int opt, do_step;
  double l1, l2, lr, beta1, beta2, eps, alpha, mu;
  const double* loss_part;
  int nB;
  double* loss_out;                                               // 4 results, then LGN_FINALIZE_CTL_SCRATCH doubles
  double* ctl;
  // lgn_train_ctl, with the switches resolved on the host
  int clip_on, thr_on, skip_nf, lr_kind;
  double max_norm, threshold, base_lr, min_lr, gamma;
  long long W, T, step_size;
};

__device__ __forceinline__ unsigned long long* as_bits(double* p) { return reinterpret_cast<unsigned long long*>(p); }
__device__ __forceinline__ unsigned long long exchange(double* slot, double x) {   // issued; awaited() makes it performed
  return __hip_atomic_exchange(as_bits(slot), (unsigned long long)__double_as_longlong(x), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// One wait for all three exchanges of a workgroup, as l1_adam_kernel waits once for its two: their returns are awaited, so they are
// performed at the coherent level before the count is issued, and thread 0 pays one memory round trip instead of three dependent ones.
__device__ __forceinline__ void awaited(unsigned long long& a, unsigned long long& b, unsigned long long& c) {
  asm volatile("s_waitcnt vmcnt(0)" : "+v"(a), "+v"(b), "+v"(c) : : "memory");
}
__device__ __forceinline__ double collect(double* slot) {                     // read a published partial and leave the slot zero
  const double x = __longlong_as_double((long long)__hip_atomic_load(as_bits(slot), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
  __hip_atomic_store(as_bits(slot), 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  return x;
}

__global__ __launch_bounds__(BLOCK) void ctl_grad_kernel(CtlArgs a) {
  __shared__ double red[4];
  __shared__ int last;
  double* scratch = a.loss_out + 4;
  double* l1_part = scratch;
  double* l2_part = scratch + CTL_THIRD;
  double* gg_part = scratch + 2 * CTL_THIRD;
  double* powers = scratch + LGN_FINALIZE_CTL_SCRATCH - 7;
  unsigned long long* done = as_bits(scratch + LGN_FINALIZE_CTL_SCRATCH - 1);
  double s1 = 0.0, s2 = 0.0, sg = 0.0;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < a.n; i += (long)gridDim.x * blockDim.x) {
    const double wi = a.w[i];
    const double G = reg_grad(wi, a.g[i], a.l1, a.l2);
    a.g[i] = G;
    s1 += fabs(wi);
    s2 = __builtin_fma(wi, wi, s2);
    sg = __builtin_fma(G, G, sg);
  }
  s1 = block_sum(s1, red);
  s2 = block_sum(s2, red);
  sg = block_sum(sg, red);
  if (threadIdx.x == 0) {
    unsigned long long o1 = exchange(l1_part + blockIdx.x, s1);
    unsigned long long o2 = exchange(l2_part + blockIdx.x, s2);
    unsigned long long o3 = exchange(gg_part + blockIdx.x, sg);
    awaited(o1, o2, o3);
    last = __hip_atomic_fetch_add(done, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == (unsigned long long)gridDim.x - 1;
  }
  __syncthreads();
  if (!last) return;
  // ---- the last workgroup: sums in index order (whichever workgroup this is), loss, decision, books ----
  double p1 = 0.0, p2 = 0.0, pg = 0.0, l = 0.0;
  for (int i = threadIdx.x; i < (int)gridDim.x; i += BLOCK) {
    p1 += collect(l1_part + i);
    p2 += collect(l2_part + i);
    pg += collect(gg_part + i);
  }
  for (int i = threadIdx.x; i < a.nB; i += BLOCK) l += a.loss_part[i];
  p1 = block_sum(p1, red);
  p2 = block_sum(p2, red);
  pg = block_sum(pg, red);
  l = block_sum(l, red);
  if (threadIdx.x != 0) return;
  const double total = __builtin_fma(a.l2, p2, l + a.l1 * p1);
  a.loss_out[0] = total;
  a.loss_out[1] = l;
  a.loss_out[2] = p1;
  a.loss_out[3] = p2;
  const double norm = sqrt(pg);
  const bool bad_nf = a.skip_nf && !(isfinite(norm) && isfinite(total));
  const bool bad_bu = a.thr_on && fabs(total) > a.threshold;
  double coef = 1.0;
  if (a.clip_on) {
    const double c = a.max_norm / (norm + 1e-6);
    coef = c >= 1.0 ? 1.0 : c;                                    // (a NaN norm gives a NaN coefficient, as torch's clamp does)
  }
  const long t = (a.step_dev ? *a.step_dev : 0) + 1;
  double lr = a.lr;
  if (a.lr_kind == LGN_LR_DEVICE) lr = a.ctl[LGN_CTL_LR];
  else if (a.lr_kind != LGN_LR_HOST) lr = lr_schedule(a.lr_kind, a.base_lr, a.min_lr, a.W, a.T, a.gamma, a.step_size, t);
  const bool apply = a.do_step && !bad_nf && !bad_bu;
  const bool clipped = coef != 1.0;
  double bc1 = 1.0, bc2_sqrt = 1.0;
  if (apply) {
    if (a.opt == LGN_OPT_ADAM) {
      const double tt = (double)t;
      const double* slot = powers + 3 * (t & 1);
      double q1, q2;
      if (slot[0] == tt) { q1 = slot[1]; q2 = slot[2]; }
      else { q1 = pow(a.beta1, tt); q2 = pow(a.beta2, tt); }
      bc1 = 1.0 - q1;
      bc2_sqrt = sqrt(1.0 - q2);
      double* next = powers + 3 * ((t + 1) & 1);                  // the NEXT step's number and powers, into the slot it will read
      next[1] = q1 * a.beta1;
      next[2] = q2 * a.beta2;
      next[0] = (double)(t + 1);
    }
    *a.step_dev += 1;
  }
  double* c = a.ctl;
  c[LGN_CTL_LR_USED] = lr;
  c[LGN_CTL_GRAD_NORM] = norm;
  c[LGN_CTL_CLIP_COEF] = coef;
  c[LGN_CTL_FLAGS] = (double)((clipped ? LGN_CTL_CLIPPED : 0) | (bad_nf ? LGN_CTL_SKIP_NONFINITE : 0) | (bad_bu ? LGN_CTL_SKIP_BLOWUP : 0));
  c[LGN_CTL_APPLY] = apply ? 1.0 : 0.0;
  c[LGN_CTL_BC1] = bc1;
  c[LGN_CTL_BC2_SQRT] = bc2_sqrt;
  if (a.do_step) {
    if (apply) {
      c[LGN_CTL_APPLIED] += 1.0;
      if (clipped) c[LGN_CTL_CLIPPED_STEPS] += 1.0;
      c[LGN_CTL_APPLIED_LOSS_SUM] += total;
    } else {
      c[LGN_CTL_SKIPPED] += 1.0;
      if (c[LGN_CTL_FIRST_SKIPPED] == 0.0) c[LGN_CTL_FIRST_SKIPPED] = (double)t;
    }
    if (isfinite(norm) && norm > c[LGN_CTL_GRAD_NORM_MAX]) c[LGN_CTL_GRAD_NORM_MAX] = norm;
  }
  *done = 0ull;
}

template <int OPT>
__global__ __launch_bounds__(BLOCK) void ctl_apply_kernel(long n, double* w, const double* __restrict__ g, double* m, double* v,
                                                         double beta1, double beta2, double eps, double alpha, double mu,
                                                         const double* __restrict__ ctl) {
  if (ctl[LGN_CTL_APPLY] == 0.0) return;                          // a skipped step writes nothing (uniform over the grid)
  const double coef = ctl[LGN_CTL_CLIP_COEF], lr = ctl[LGN_CTL_LR_USED];
  [[maybe_unused]] const double bc1 = ctl[LGN_CTL_BC1], bc2_sqrt = ctl[LGN_CTL_BC2_SQRT];
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    const double gc = g[i] * coef;                                // coef == 1.0: the gradient's bits
    AdamOut o;
    if constexpr (OPT == TAIL_ADAM) o = adam_update_one(w[i], gc, m[i], v[i], lr, beta1, beta2, eps, bc1, bc2_sqrt);
    else o = rmsprop_update_one(w[i], gc, m[i], v[i], lr, alpha, mu, eps);
    m[i] = o.m;
    v[i] = o.v;
    w[i] = o.w;
  }
}

__global__ void ctl_reset_kernel(double* ctl) {
  const int i = threadIdx.x;
  if (i >= LGN_CTL_APPLIED && i <= LGN_CTL_APPLIED_LOSS_SUM) ctl[i] = 0.0;
}

int ctl_grid(long n) {
  long g = ((n + CTL_PER_THREAD - 1) / CTL_PER_THREAD + BLOCK - 1) / BLOCK;
  if (g < 1) g = 1;
  return (int)(g < CTL_THIRD ? g : CTL_THIRD);
}

bool switch_on(double x) { return x > 0.0 && x < INFINITY; }      // <= 0, +inf (and NaN): off

// the refusals of the descriptor: message set, -1
int check_train_ctl(const lgn_train_ctl* tc) {
  LGN_CHECK_ARG(tc, "training control descriptor: null pointer");
  LGN_CHECK_ARG(tc->lr_kind >= LGN_LR_HOST && tc->lr_kind <= LGN_LR_WARMUP_STEP, "training control descriptor: unknown lr_kind %d", tc->lr_kind);
  // under every lr_kind, as lgn_amd.h lists them, although LGN_LR_HOST / LGN_LR_DEVICE read none of the three (zero passes)
  LGN_CHECK_ARG(tc->warmup_steps >= 0, "training control descriptor: warmup_steps %lld < 0", tc->warmup_steps);
  LGN_CHECK_ARG(tc->base_lr >= 0.0 && tc->min_lr >= 0.0, "training control descriptor: negative base_lr or min_lr");
  if (tc->lr_kind == LGN_LR_WARMUP_COSINE)
    LGN_CHECK_ARG(tc->total_steps > tc->warmup_steps, "training control descriptor: the cosine needs total_steps %lld > warmup_steps %lld",
                  tc->total_steps, tc->warmup_steps);
  if (tc->lr_kind == LGN_LR_WARMUP_STEP) {
    LGN_CHECK_ARG(tc->step_size >= 1, "training control descriptor: step_size %lld < 1", tc->step_size);
    LGN_CHECK_ARG(tc->gamma > 0.0, "training control descriptor: gamma must be > 0");
  }
  return 0;
}

}  // namespace
}  // namespace lgn

using namespace lgn;

extern "C" {

int lgn_step_finalize_ctl_f64(double* params, double* grads, long long n_params, const double* loss_part, int n_loss,
                              const lgn_optim_desc* opt, double* state_m, double* state_v, long long* step_dev, int do_step,
                              double* loss_out, const lgn_train_ctl* tc, double* ctl, void* stream) {
  LGN_CHECK_ARG(params && grads && loss_part && loss_out && n_params > 0 && n_loss > 0, "step_finalize_ctl: null pointer");
  LGN_CHECK_ARG(opt, "optimiser descriptor: null pointer");
  LGN_CHECK_ARG(opt->kind == LGN_OPT_ADAM || opt->kind == LGN_OPT_RMSPROP, "optimiser descriptor: kind %d is neither LGN_OPT_ADAM nor "
                "LGN_OPT_RMSPROP", opt->kind);
  LGN_CHECK_ARG(!do_step || (state_m && state_v && step_dev), "optimiser state missing");
  LGN_CHECK_ARG(opt->l2_lambda >= 0.0 && opt->eps >= 0.0, "optimiser descriptor: negative l2_lambda or eps");
  LGN_CHECK_ARG(opt->kind != LGN_OPT_RMSPROP || (opt->alpha >= 0.0 && opt->alpha <= 1.0 && opt->momentum >= 0.0),
                "optimiser descriptor: RMSprop takes 0 <= alpha <= 1 and momentum >= 0");
  if (int rc = check_train_ctl(tc)) return rc;
  LGN_CHECK_ARG(ctl, "training control block: null pointer");
  hipStream_t st = (hipStream_t)stream;
  CtlArgs a{};
  a.n = (long)n_params;
  a.w = params; a.g = grads; a.m = state_m; a.v = state_v;
  a.step_dev = reinterpret_cast<long*>(step_dev);
  a.opt = opt->kind; a.do_step = do_step ? 1 : 0;
  a.l1 = opt->l1_lambda; a.l2 = opt->l2_lambda; a.lr = opt->lr; a.beta1 = opt->beta1; a.beta2 = opt->beta2; a.eps = opt->eps;
  a.alpha = opt->alpha; a.mu = opt->momentum;
  a.loss_part = loss_part; a.nB = n_loss; a.loss_out = loss_out; a.ctl = ctl;
  a.clip_on = switch_on(tc->max_grad_norm); a.thr_on = switch_on(tc->blow_up_threshold); a.skip_nf = tc->skip_nonfinite != 0;
  a.lr_kind = tc->lr_kind;
  a.max_norm = tc->max_grad_norm; a.threshold = tc->blow_up_threshold;
  a.base_lr = tc->base_lr; a.min_lr = tc->min_lr; a.gamma = tc->gamma;
  a.W = tc->warmup_steps; a.T = tc->total_steps; a.step_size = tc->step_size;
  const int nblk = ctl_grid(a.n);
  hipLaunchKernelGGL(ctl_grad_kernel, dim3(nblk), dim3(BLOCK), 0, st, a);
  LGN_CHECK_LAUNCH();
  if (!do_step) return 0;
  if (opt->kind == LGN_OPT_ADAM)
    hipLaunchKernelGGL(ctl_apply_kernel<TAIL_ADAM>, dim3(nblk), dim3(BLOCK), 0, st, a.n, a.w, a.g, a.m, a.v, a.beta1, a.beta2, a.eps, a.alpha,
                       a.mu, ctl);
  else
    hipLaunchKernelGGL(ctl_apply_kernel<TAIL_RMSPROP>, dim3(nblk), dim3(BLOCK), 0, st, a.n, a.w, a.g, a.m, a.v, a.beta1, a.beta2, a.eps,
                       a.alpha, a.mu, ctl);
  LGN_CHECK_LAUNCH();
  return 0;
}

int lgn_train_ctl_reset(double* ctl, void* stream) {
  LGN_CHECK_ARG(ctl, "train_ctl_reset: null pointer");
  hipLaunchKernelGGL(ctl_reset_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, ctl);
  LGN_CHECK_LAUNCH();
  return 0;
}

double lgn_lr_schedule_value(const lgn_train_ctl* tc, long long t, double device_lr) {
  if (check_train_ctl(tc)) return NAN;
  if (tc->lr_kind == LGN_LR_HOST || tc->lr_kind == LGN_LR_DEVICE) return device_lr;
  return lr_schedule(tc->lr_kind, tc->base_lr, tc->min_lr, tc->warmup_steps, tc->total_steps, tc->gamma, tc->step_size, t);
}

}  // extern "C"
