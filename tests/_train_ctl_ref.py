"""Plain numpy restatement of the guarded finalize of a training step (csrc/step_ctl.hip, lgn_step_finalize_ctl_f64), built on
tests/_optim_ref.py: the clipping coefficient of torch.nn.utils.clip_grad_norm_, the rule that decides whether a step is applied,
the closed-form learning-rate schedules, and one whole controlled step on a flat parameter vector.  It pins what the kernels
implement and is itself checked against torch on the CPU (tests/test_host_train_ctl.py)."""
import math

import numpy as np

import _optim_ref as R

LR_HOST, LR_DEVICE, LR_WARMUP_COSINE, LR_WARMUP_STEP = 0, 1, 2, 3
CLIPPED, SKIP_NONFINITE, SKIP_BLOWUP = 1, 2, 4


def _on(x):
    """max_grad_norm / blow_up_threshold: None, <= 0 or +inf is off."""
    return x is not None and 0.0 < x < math.inf


def grad_norm(G):
    return float(np.sqrt(np.sum(np.square(np.asarray(G, dtype=np.float64)))))


def clip_coef(G, max_norm):
    """min(1, max_norm / (norm + 1e-6)) (torch.nn.utils.clip_grad_norm_); exactly 1.0 with clipping off; NaN for a NaN norm."""
    if not _on(max_norm):
        return 1.0
    c = max_norm / (grad_norm(G) + 1e-6)
    return 1.0 if c >= 1.0 else c


def decide(norm, total, skip_nonfinite=False, blow_up_threshold=None):
    """(bad_nf, bad_bu): the step is applied only when both are False."""
    bad_nf = bool(skip_nonfinite) and not (math.isfinite(norm) and math.isfinite(total))
    bad_bu = _on(blow_up_threshold) and abs(total) > blow_up_threshold
    return bad_nf, bool(bad_bu)


def lr_value(schedule, t):
    """The learning rate of step t >= 1.  schedule: dict(kind, base_lr, min_lr, warmup_steps, total_steps, gamma, step_size) with
    kind LR_WARMUP_COSINE or LR_WARMUP_STEP."""
    W, base = schedule.get("warmup_steps", 0), schedule["base_lr"]
    if t <= W:
        return base * t / W
    if schedule["kind"] == LR_WARMUP_COSINE:
        span, lo = schedule["total_steps"] - W, schedule.get("min_lr", 0.0)
        return lo + (base - lo) * 0.5 * (1.0 + math.cos(math.pi * min(t - W, span) / span))
    return base * schedule.get("gamma", 1.0) ** ((t - W - 1) // schedule.get("step_size", 1))


def controlled_step(w, g, m, v, t_prev, data, kind="adam", lr=5e-4, l1=0.0, l2=0.0, max_grad_norm=None, skip_nonfinite=False,
                    blow_up_threshold=None, beta1=0.9, beta2=0.999, eps=None, alpha=0.99, momentum=0.9):
    """One guarded step on the raw loss gradient g from the weights w, state (m, v) and t_prev applied steps, `data` the data loss
    and `lr` this step's learning rate.  Returns dict(w, m, v, t, G, norm, coef, total, flags, applied): G is the unclipped
    regularised gradient; a skipped step returns w, m, v and t_prev unchanged."""
    w, g, m, v = (np.asarray(x, dtype=np.float64) for x in (w, g, m, v))
    G = R.regularised_grad(w, g, l1, l2)
    norm = grad_norm(G)
    total = float(R.loss_total(data, w, l1, l2))
    coef = clip_coef(G, max_grad_norm)
    bad_nf, bad_bu = decide(norm, total, skip_nonfinite, blow_up_threshold)
    flags = (CLIPPED if coef != 1.0 else 0) | (SKIP_NONFINITE if bad_nf else 0) | (SKIP_BLOWUP if bad_bu else 0)
    out = dict(w=w, m=m, v=v, t=t_prev, G=G, norm=norm, coef=coef, total=total, flags=flags, applied=False)
    if bad_nf or bad_bu:
        return out
    gc = G * coef
    if kind == "adam":
        w2, m2, v2 = R.adam_step(w, gc, m, v, t_prev + 1, lr, beta1, beta2, 1e-8 if eps is None else eps)
    else:
        w2, v2, m2 = R.rmsprop_step(w, gc, v, m, lr, alpha, 1e-16 if eps is None else eps, momentum)
    out.update(w=w2, m=m2, v=v2, t=t_prev + 1, applied=True)
    return out
