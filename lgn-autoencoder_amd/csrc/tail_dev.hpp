// lgn-autoencoder_amd/csrc/tail_dev.hpp -- the arithmetic of a step's tail with every multiply-add spelled out, shared by the
// kernels that run it as separate launches (rad_finalize_batch_kernel in level_bwd.hip, l1_adam_kernel in net_kernels.hip) and
// by the fused launch (step_tail.hip): which products the compiler contracts into fused multiply-adds may differ from one kernel to
// the next, and the two routes are tested to agree bit for bit.  The same holds for the update rules of the lgn_optim_desc calls below.
#pragma once
#include "common.hpp"

namespace lgn {

// radial-parameter gradients from a level's reduced sums (RadPolyTrig: lgn/nn/position_levels.py:118-209; sums T1 | T2 | S | dB)
__device__ __forceinline__ double radfin_weight(double rb, double t1, double ra, double s) { return __builtin_fma(rb, t1, ra * s); }
// sum_r w[r ws] x[r xs], r ascending
__device__ __forceinline__ double radfin_dot(const double* w, int ws, const double* x, int xs, int R) {
  double d = 0.0;
  for (int r = 0; r < R; ++r) d = __builtin_fma(w[r * ws], x[r * xs], d);
  return d;
}
__device__ __forceinline__ double radfin_c(double rb, double rc, double dc) { return ((-2.0 * rb) * rc) * dc; }

// L1 sub-gradient + Adam of one parameter (torch.optim.Adam defaults; utils/train.py:484-492): gradient incl. the L1 term, new
// moments, new weight
struct AdamOut { double g, m, v, w; };
__device__ __forceinline__ AdamOut l1_adam_one(double w, double gsum, double m, double v, double lambda, double lr, double beta1,
                                               double beta2, double eps, double bc1, double bc2_sqrt) {
  AdamOut o;
  o.g = gsum + lambda * (double)((w > 0.0) - (w < 0.0));       // (lambda * +-1 is exact: no contraction can change this)
  o.m = __builtin_fma(o.g - m, 1.0 - beta1, m);
  o.v = __builtin_fma((1.0 - beta2) * o.g, o.g, v * beta2);
  const double denom = sqrt(o.v) / bc2_sqrt + eps;
  o.w = w - (lr / bc1) * (o.m / denom);
  return o;
}

// The optimiser kinds of the lgn_optim_desc calls (LGN_OPT_* of include/lgn_amd.h) as template arguments of the tail kernels.  The
// second template argument of those kernels, L2, is "the lgn_optim_desc form": the L2 term, the w^2 partial sums and the fourth
// result.  <TAIL_ADAM, false> is the kernel of the calls without a descriptor and stays the code it was.
constexpr int TAIL_ADAM = 0, TAIL_RMSPROP = 1;

// loss gradient + the L2 term 2 l2 w, from the weight BEFORE the update; l2 == 0 switches the term off (no "+ 0 w": the gradient
// keeps its bits).  The L1 term is added to this sum, by l1_adam_one for Adam and in its words for RMSprop.
__device__ __forceinline__ double l2_grad(double w, double gsum, double l2) {
  return l2 != 0.0 ? __builtin_fma(2.0 * l2, w, gsum) : gsum;
}
// Adam with both regularisers: l1_adam_one on the gradient that holds the L2 term (l2 == 0: l1_adam_one's bits)
__device__ __forceinline__ AdamOut l1_l2_adam_one(double w, double gsum, double m, double v, double l1, double l2, double lr, double beta1,
                                                  double beta2, double eps, double bc1, double bc2_sqrt) {
  return l1_adam_one(w, l2_grad(w, gsum, l2), m, v, l1, lr, beta1, beta2, eps, bc1, bc2_sqrt);
}
// RMSprop of one parameter in the arithmetic of torch.optim.RMSprop(centered=False, weight_decay=0) (utils/initialize.py:153-173):
// v = alpha v + (1 - alpha) g^2;  avg = sqrt(v) + eps (eps OUTSIDE the root);  mu > 0: buf = mu buf + g / avg, w -= lr buf (lr on
// the buffer);  mu == 0: w -= lr g / avg and the buffer is left alone.  AdamOut::m carries the momentum buffer, ::v square_avg.
__device__ __forceinline__ AdamOut l1_l2_rmsprop_one(double w, double gsum, double buf, double v, double l1, double l2, double lr,
                                                     double alpha, double mu, double eps) {
  AdamOut o;
  o.g = l2_grad(w, gsum, l2) + l1 * (double)((w > 0.0) - (w < 0.0));
  o.v = __builtin_fma((1.0 - alpha) * o.g, o.g, v * alpha);
  const double q = o.g / (sqrt(o.v) + eps);
  o.m = mu > 0.0 ? __builtin_fma(mu, buf, q) : buf;
  o.w = __builtin_fma(-lr, mu > 0.0 ? o.m : q, w);
  return o;
}

// ---- the guarded finalize (step_ctl.hip): the same rules in two halves, because the update waits for the norm of the WHOLE
// regularised gradient.  reg_grad is the gradient both rules above form (their words: l2_grad, then + l1 sign(w));
// adam_update_one / rmsprop_update_one are l1_adam_one / l1_l2_rmsprop_one from that point on, on a gradient that is already
// regularised (and clipped: G * coef, coef == 1.0 keeps the bits).  AdamOut::g is the gradient handed in.
__device__ __forceinline__ double reg_grad(double w, double gsum, double l1, double l2) {
  return l2_grad(w, gsum, l2) + l1 * (double)((w > 0.0) - (w < 0.0));
}
__device__ __forceinline__ AdamOut adam_update_one(double w, double g, double m, double v, double lr, double beta1, double beta2,
                                                   double eps, double bc1, double bc2_sqrt) {
  AdamOut o;
  o.g = g;
  o.m = __builtin_fma(o.g - m, 1.0 - beta1, m);
  o.v = __builtin_fma((1.0 - beta2) * o.g, o.g, v * beta2);
  const double denom = sqrt(o.v) / bc2_sqrt + eps;
  o.w = w - (lr / bc1) * (o.m / denom);
  return o;
}
__device__ __forceinline__ AdamOut rmsprop_update_one(double w, double g, double buf, double v, double lr, double alpha, double mu,
                                                      double eps) {
  AdamOut o;
  o.g = g;
  o.v = __builtin_fma((1.0 - alpha) * o.g, o.g, v * alpha);
  const double q = o.g / (sqrt(o.v) + eps);
  o.m = mu > 0.0 ? __builtin_fma(mu, buf, q) : buf;
  o.w = __builtin_fma(-lr, mu > 0.0 ? o.m : q, w);
  return o;
}

// The learning rate of step t >= 1 under a schedule (LGN_LR_WARMUP_COSINE / LGN_LR_WARMUP_STEP of include/lgn_amd.h), one closed
// form for the kernel and for the host (lgn_lr_schedule_value): linear warm-up base t / W over the first W steps, then half a
// cosine from base down to min_lr at step T (held there), or base gamma^floor((t - W - 1) / step_size).
constexpr int LR_COSINE = 2, LR_STEP = 3;
__host__ __device__ inline double lr_schedule(int kind, double base, double min_lr, long long W, long long T, double gamma,
                                              long long step_size, long long t) {
  if (t <= W) return base * (double)t / (double)W;
  if (kind == LR_COSINE) {
    const long long span = T - W, at = t - W < span ? t - W : span;
    const double x = 3.14159265358979323846 * (double)at / (double)span;
    return min_lr + (base - min_lr) * 0.5 * (1.0 + cos(x));
  }
  return base * pow(gamma, (double)((t - W - 1) / step_size));
}

}  // namespace lgn
