"""Host-side checks of the guarded training step (gradient clipping, skip on a non-finite or exploding step, live learning rate):
the three new entry points are exported under ABI 19 and mirror the header; lgn_step_finalize_ctl_f64 refuses bad descriptors
before any launch; the closed-form schedule the kernel runs (exported as lgn_lr_schedule_value) agrees with its numpy restatement
and with torch's schedulers; and the numpy restatement of the guarded step (tests/_train_ctl_ref.py) agrees with
clip_grad_norm_ + torch.optim on the CPU.  No GPU needed."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest
import torch

import _train_ctl_ref as T
from lgn import _native as N
from lgn import step as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("lgn_step_finalize_ctl_f64", "lgn_train_ctl_reset", "lgn_lr_schedule_value")


def _header():
    return open(os.path.join(ROOT, "include", "lgn_amd.h")).read()


def test_new_entry_points_are_exported_under_abi_19_and_mirror_the_header():
    lib, header = N.lib(), _header()
    assert N.ABI_VERSION == 19 and lib.lgn_abi_version() == 19 and re.search(r"#define LGN_AMD_ABI_VERSION 19\b", header)
    for name in NEW:
        assert hasattr(lib, name) and name in N.EXPORTED_SYMBOLS
    assert lib.lgn_lr_schedule_value.restype is C.c_double and lib.lgn_step_finalize_ctl_f64.restype is C.c_int
    # the descriptor finalize's arguments with the control descriptor and the control block ahead of the stream
    assert N._SIGNATURES["lgn_step_finalize_ctl_f64"][:-3] == N._SIGNATURES["lgn_step_finalize_opt_f64"][:-1]
    assert len(N._SIGNATURES["lgn_step_finalize_ctl_f64"]) == len(N._SIGNATURES["lgn_step_finalize_opt_f64"]) + 2
    # every LGN_CTL_* / LGN_LR_* / LGN_FINALIZE_CTL_SCRATCH constant of the header has its twin in lgn/_native.py, same value
    defines = dict(re.findall(r"#define (LGN_(?:CTL|LR)_[A-Z0-9_]+|LGN_FINALIZE_CTL_SCRATCH) (\d+)", header))
    assert len(defines) >= 23
    for name, value in defines.items():
        twin = name[4:]
        assert getattr(N, twin) == int(value), name
    for twin in ("CTL_LR", "CTL_LR_USED", "CTL_GRAD_NORM", "CTL_CLIP_COEF", "CTL_FLAGS", "CTL_APPLIED", "CTL_CLIPPED_STEPS", "CTL_SKIPPED",
                 "CTL_FIRST_SKIPPED", "CTL_GRAD_NORM_MAX", "CTL_APPLIED_LOSS_SUM", "CTL_DOUBLES", "CTL_CLIPPED", "CTL_SKIP_NONFINITE",
                 "CTL_SKIP_BLOWUP", "LR_HOST", "LR_DEVICE", "LR_WARMUP_COSINE", "LR_WARMUP_STEP", "FINALIZE_CTL_SCRATCH"):
        assert "LGN_" + twin in defines, twin
    assert (T.LR_HOST, T.LR_DEVICE, T.LR_WARMUP_COSINE, T.LR_WARMUP_STEP) == (N.LR_HOST, N.LR_DEVICE, N.LR_WARMUP_COSINE, N.LR_WARMUP_STEP)
    assert (T.CLIPPED, T.SKIP_NONFINITE, T.SKIP_BLOWUP) == (N.CTL_CLIPPED, N.CTL_SKIP_NONFINITE, N.CTL_SKIP_BLOWUP)
    # the struct, field by field, as the header declares it
    body = re.search(r"typedef struct \{([^}]*)\} lgn_train_ctl;", header).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    ctype = {"double": C.c_double, "int": C.c_int, "long long": C.c_longlong}
    declared = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            ty, names = re.match(r"(long long|double|int)\s+(.*)", decl).groups()
            declared += [(n.strip(), ctype[ty]) for n in names.split(",")]
    assert declared == list(N.TrainCtl._fields_)
    assert C.sizeof(N.TrainCtl) == 72


def _call(lib, tc, ctl="buf", opt="adam", do_step=1, state="buf"):
    """lgn_step_finalize_ctl_f64 on host pointers that are never dereferenced: every refusal comes before the first launch."""
    buf = (C.c_double * 8)()
    p = C.addressof(buf)
    d = N.OptimDesc()
    d.kind, d.lr, d.eps, d.beta1, d.beta2, d.alpha, d.momentum = N.OPT_ADAM, 1e-3, 1e-8, 0.9, 0.999, 0.99, 0.9
    st = p if state == "buf" else None
    return lib.lgn_step_finalize_ctl_f64(p, p, 4, p, 1, C.byref(d) if opt else None, st, st, st, do_step, p,
                                         C.byref(tc) if tc is not None else None, p if ctl == "buf" else None, None)


def _good(kind):
    tc = N.TrainCtl()
    tc.lr_kind, tc.base_lr, tc.min_lr, tc.warmup_steps, tc.total_steps, tc.gamma, tc.step_size = kind, 1e-3, 0.0, 2, 10, 0.5, 3
    return tc


def test_every_refusal_arrives_before_any_launch():
    lib = N.lib()
    assert _call(lib, None) < 0 and b"control descriptor" in lib.lgn_last_error()
    assert _call(lib, _good(N.LR_HOST), ctl=None) < 0 and b"control block" in lib.lgn_last_error()
    assert _call(lib, _good(N.LR_HOST), opt=None) < 0 and b"descriptor" in lib.lgn_last_error()
    tc = _good(N.LR_HOST)
    tc.lr_kind = 9
    assert _call(lib, tc) < 0 and b"lr_kind" in lib.lgn_last_error()
    tc.lr_kind = -1
    assert _call(lib, tc) < 0 and b"lr_kind" in lib.lgn_last_error()
    for kind in (N.LR_HOST, N.LR_DEVICE, N.LR_WARMUP_COSINE, N.LR_WARMUP_STEP):      # under every lr_kind, used there or not
        tc = _good(kind)
        tc.warmup_steps = -1
        assert _call(lib, tc) < 0 and b"warmup_steps" in lib.lgn_last_error()
        tc = _good(kind)
        tc.base_lr = -1e-3
        assert _call(lib, tc) < 0 and b"base_lr" in lib.lgn_last_error()
        tc = _good(kind)
        tc.min_lr = -1e-9
        assert _call(lib, tc) < 0 and b"min_lr" in lib.lgn_last_error()
    tc = _good(N.LR_WARMUP_COSINE)
    tc.total_steps = tc.warmup_steps
    assert _call(lib, tc) < 0 and b"total_steps" in lib.lgn_last_error()
    tc = _good(N.LR_WARMUP_STEP)
    tc.step_size = 0
    assert _call(lib, tc) < 0 and b"step_size" in lib.lgn_last_error()
    tc = _good(N.LR_WARMUP_STEP)
    tc.gamma = 0.0
    assert _call(lib, tc) < 0 and b"gamma" in lib.lgn_last_error()
    assert _call(lib, _good(N.LR_HOST), state=None) < 0 and b"state" in lib.lgn_last_error()
    assert lib.lgn_train_ctl_reset(None, None) < 0 and b"null" in lib.lgn_last_error()
    assert math.isnan(lib.lgn_lr_schedule_value(None, 1, 0.0))
    tc = _good(N.LR_WARMUP_STEP)
    tc.gamma = -1.0
    assert math.isnan(lib.lgn_lr_schedule_value(C.byref(tc), 1, 0.0))


def _points(W, Tt):
    return sorted({t for t in (1, W - 1, W, W + 1, Tt - 1, Tt, Tt + 5) if t >= 1})


@pytest.mark.parametrize("W", [0, 1, 5])
@pytest.mark.parametrize("step_size", [1, 7])
def test_closed_form_of_the_library_matches_the_numpy_restatement(W, step_size):
    """The formula is a handful of fp64 roundings around one cos or pow of libm: relative 1e-14."""
    lib, Tt = N.lib(), 40
    for kind, extra in ((N.LR_WARMUP_COSINE, dict(min_lr=1e-5)), (N.LR_WARMUP_COSINE, dict(min_lr=0.0)),
                        (N.LR_WARMUP_STEP, dict(gamma=0.7, step_size=step_size))):
        sched = dict(kind=kind, base_lr=3e-3, warmup_steps=W, total_steps=Tt, min_lr=0.0, gamma=1.0, step_size=1)
        sched.update(extra)
        tc = N.TrainCtl()
        tc.lr_kind, tc.base_lr, tc.min_lr, tc.gamma = kind, sched["base_lr"], sched["min_lr"], sched["gamma"]
        tc.warmup_steps, tc.total_steps, tc.step_size = W, Tt, sched["step_size"]
        for t in _points(W, Tt):
            got, want = lib.lgn_lr_schedule_value(C.byref(tc), t, -1.0), T.lr_value(sched, t)
            print(f"kind {kind} W {W} step_size {sched['step_size']} t {t}: library {got!r} numpy {want!r}")
            assert abs(got - want) <= 1e-14 * abs(want), (kind, W, t, got, want)
        # the Python class of lgn.step computes the same numbers
        s = S.LRSchedule("cosine" if kind == N.LR_WARMUP_COSINE else "step", sched["base_lr"], W, Tt, sched["min_lr"], sched["gamma"],
                         sched["step_size"])
        assert s.code == kind and all(s.value(t) == T.lr_value(sched, t) for t in range(1, Tt + 6))
    tc = N.TrainCtl()
    tc.lr_kind = N.LR_DEVICE
    assert lib.lgn_lr_schedule_value(C.byref(tc), 3, 0.125) == 0.125


def _torch_lrs(make, steps=50, base=3e-3):
    """param_group['lr'] in force at optimiser step t = 1 .. steps when scheduler.step() follows every optimizer.step()."""
    p = torch.nn.Parameter(torch.zeros(1))
    opt = torch.optim.SGD([p], lr=base)
    sched = make(opt)
    out = []
    for _ in range(steps):
        out.append(opt.param_groups[0]["lr"])
        opt.step()
        sched.step()
    return out


@pytest.mark.parametrize("step_size", [1, 7])
def test_step_schedule_is_torchs_step_lr_and_exponential_lr(step_size):
    """Without warm-up, base gamma^floor((t - 1) / step_size) is StepLR stepped once per optimiser step (step_size 1:
    ExponentialLR).  Torch multiplies by gamma recursively, about one rounding per step: 50 * 2^-53 = 6e-15, held at 1e-12."""
    from torch.optim import lr_scheduler as L
    base, gamma = 3e-3, 0.9
    sched = dict(kind=T.LR_WARMUP_STEP, base_lr=base, warmup_steps=0, gamma=gamma, step_size=step_size)
    makes = [lambda o: L.StepLR(o, step_size=step_size, gamma=gamma)]
    if step_size == 1:
        makes.append(lambda o: L.ExponentialLR(o, gamma=gamma))
    for make in makes:
        for t, lr in enumerate(_torch_lrs(make, base=base), start=1):
            assert abs(T.lr_value(sched, t) - lr) <= 1e-12 * lr, (t, lr)


@pytest.mark.parametrize("W", [2, 5])
def test_warmup_cosine_is_linear_lr_then_cosine_annealing_under_sequential_lr(W):
    """lr(t) = base t / W for t <= W is LinearLR(start_factor=1/W, total_iters=W-1) read at optimiser step t (its epoch t - 1); the
    cosine part, with its phase counted from step W, is CosineAnnealingLR(T_max=T-W, eta_min=min_lr) switched in by SequentialLR at
    milestone W - 1, i.e. at step W, where both give base.  Torch's cosine goes on (it is periodic) past T_max while the definition
    here holds min_lr from step T on: the comparison covers t = 1 .. T, the whole range where the two definitions coincide."""
    from torch.optim import lr_scheduler as L
    import warnings
    base, lo, Tt = 3e-3, 1e-5, 40
    sched = dict(kind=T.LR_WARMUP_COSINE, base_lr=base, min_lr=lo, warmup_steps=W, total_steps=Tt)

    def make(o):
        return L.SequentialLR(o, [L.LinearLR(o, start_factor=1.0 / W, end_factor=1.0, total_iters=W - 1),
                                  L.CosineAnnealingLR(o, T_max=Tt - W, eta_min=lo)], milestones=[W - 1])

    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        lrs = _torch_lrs(make, steps=50, base=base)
    for t in range(1, Tt + 1):
        want = T.lr_value(sched, t)
        print(f"W {W} t {t}: torch {lrs[t - 1]!r} closed form {want!r}")
        assert abs(want - lrs[t - 1]) <= 1e-12 * abs(lrs[t - 1]), (t, want, lrs[t - 1])
    assert T.lr_value(sched, Tt) == lo == T.lr_value(sched, Tt + 5)


# ---- the numpy restatement of the guarded step against clip_grad_norm_ + torch.optim on the CPU ---------------------------------

# as tests/test_host_optimizer_options.py holds _optim_ref to torch (the reasoning is given there)
RTOL, ATOL = 1e-13, 1e-300


@pytest.mark.parametrize("n", [1, 257, 5000])
@pytest.mark.parametrize("kind", ["adam", "rmsprop"])
def test_controlled_step_matches_clip_grad_norm_and_torch_optim(kind, n):
    rng = np.random.default_rng(100 + n)
    w = rng.standard_normal(n)
    m, v, t = np.zeros(n), np.zeros(n), 0
    p = torch.nn.Parameter(torch.tensor(w))
    lr, l1, l2 = 5e-4, 1e-8, 1e-6
    opt = S.torch_optimizer([p], kind, lr)
    # The tolerance is relative to each result, so it presumes results that are not the small difference of two large operands: a
    # first moment 0.9 m + 0.1 g with m and g of opposite sign may cancel, and both sides then carry the operands' rounding.  Every
    # element therefore keeps its gradient's sign over the steps (random magnitudes), as a parameter far from its optimum does.
    sign = np.where(rng.standard_normal(n) >= 0, 1.0, -1.0)
    norm0 = T.grad_norm(0.05 + np.abs(rng.standard_normal(n)))
    for it in range(4):
        g = sign * (0.05 + np.abs(rng.standard_normal(n)))
        factor = (0.5, 2.0, 0.25, None)[it]                   # clipped, not clipped, clipped, clipping off
        max_norm = None if factor is None else factor * norm0
        step_lr = lr * (1.0 + it)
        out = T.controlled_step(w, g, m, v, t, data=1.0, kind=kind, lr=step_lr, l1=l1, l2=l2, max_grad_norm=max_norm)
        with torch.no_grad():
            p.grad = torch.tensor(g) + l1 * torch.sign(p) + 2.0 * l2 * p
        G = p.grad.clone().numpy()
        np.testing.assert_allclose(out["G"], G, rtol=RTOL, atol=ATOL)
        if max_norm is not None:
            tn = float(torch.nn.utils.clip_grad_norm_([p], max_norm))
            assert abs(out["norm"] - tn) <= n * 2.0 ** -52 * tn
            np.testing.assert_allclose(out["G"] * out["coef"], p.grad.numpy(), rtol=RTOL, atol=ATOL)
            assert (out["flags"] & T.CLIPPED) == (T.CLIPPED if out["norm"] + 1e-6 > max_norm else 0)
        else:
            assert out["coef"] == 1.0 and out["flags"] == 0
        for group in opt.param_groups:
            group["lr"] = step_lr
        opt.step()
        w, m, v, t = out["w"], out["m"], out["v"], out["t"]
        st = opt.state[p]
        np.testing.assert_allclose(w, p.detach().numpy(), rtol=RTOL, atol=ATOL)
        np.testing.assert_allclose(v, st["square_avg" if kind == "rmsprop" else "exp_avg_sq"].numpy(), rtol=RTOL, atol=ATOL)
        np.testing.assert_allclose(m, st["momentum_buffer" if kind == "rmsprop" else "exp_avg"].numpy(), rtol=RTOL, atol=ATOL)
        assert out["applied"] and t == it + 1


def test_decision_rule_and_skipped_steps_of_the_restatement():
    w, z = np.array([1.0, -2.0, 0.5]), np.zeros(3)
    for bad, kw, bit in ((np.array([0.1, np.nan, 0.2]), dict(skip_nonfinite=True), T.SKIP_NONFINITE),
                         (np.array([0.1, np.inf, 0.2]), dict(skip_nonfinite=True), T.SKIP_NONFINITE),
                         (np.array([0.1, 0.3, 0.2]), dict(blow_up_threshold=1e-30), T.SKIP_BLOWUP)):
        out = T.controlled_step(w, bad, z, z, 4, data=2.0, **kw)
        assert not out["applied"] and out["flags"] & bit and out["t"] == 4
        assert out["w"] is not None and np.array_equal(out["w"], w) and not out["m"].any() and not out["v"].any()
    out = T.controlled_step(w, np.array([0.1, 0.3, 0.2]), z, z, 4, data=float("nan"), skip_nonfinite=True)
    assert not out["applied"] and out["flags"] == T.SKIP_NONFINITE
    out = T.controlled_step(w, np.array([0.1, np.nan, 0.2]), z, z, 4, data=2.0)          # guard off: the NaN goes through
    assert out["applied"] and np.isnan(out["w"][1]) and not np.isnan(out["w"][0])
    assert T.decide(1.0, 1e33, blow_up_threshold=1e32) == (False, True) and T.decide(1.0, 1e33, blow_up_threshold=math.inf) == (False, False)
    assert T.clip_coef(np.ones(4), None) == 1.0 == T.clip_coef(np.ones(4), 0.0) == T.clip_coef(np.ones(4), math.inf)
    assert math.isnan(T.clip_coef(np.array([1.0, np.nan]), 1.0))


def test_step_classes_take_the_control_keywords_with_everything_off_by_default():
    import inspect
    for cls in (S.NativeTrainStep, S.CapturedModuleStep, S.TrainStep, S.ReferenceLoopStep):
        sig = inspect.signature(cls.__init__).parameters
        assert sig["max_grad_norm"].default is None and sig["blow_up_threshold"].default is None
        assert sig["skip_nonfinite"].default is False and sig["lr_schedule"].default is None
    for cls in (S.NativeTrainStep, S.CapturedModuleStep):
        assert {"max_grad_norm", "skip_nonfinite", "blow_up_threshold", "lr_schedule"} <= S._STEP_KEYWORDS[cls]
    assert not S._controlled(None, False, None, None) and S._controlled(None, False, None, "device") and S._controlled(1.0, False, None, None)
    with pytest.raises(ValueError):
        S.LRSchedule("cosine", 1e-3, warmup_steps=5, total_steps=5)
    with pytest.raises(ValueError):
        S.LRSchedule("step", 1e-3, gamma=0.0)
    with pytest.raises(ValueError):
        S.LRSchedule("linear", 1e-3)


def test_torch_side_guard_clips_skips_and_schedules_on_the_cpu():
    """The comparator's guard (what TrainStep / ReferenceLoopStep run) against the numpy restatement on one flat parameter."""
    n = 64
    rng = np.random.default_rng(3)
    w = rng.standard_normal(n)
    p = torch.nn.Parameter(torch.tensor(w))
    opt = torch.optim.Adam([p], 1e-3)
    sched = S.LRSchedule("cosine", 1e-3, warmup_steps=2, total_steps=6)
    guard = S._TorchGuard(1e-3, max_grad_norm=1.0, skip_nonfinite=True, blow_up_threshold=1e32, lr_schedule=sched)
    m, v, t = np.zeros(n), np.zeros(n), 0
    for it in range(5):
        g = rng.standard_normal(n)
        if it == 2:
            g[7] = np.nan
        p.grad = torch.tensor(g)
        ok = guard.admit([p], torch.tensor(1.0), [opt])
        out = T.controlled_step(w, g, m, v, t, data=1.0, lr=sched.value(t + 1), max_grad_norm=1.0, skip_nonfinite=True,
                                blow_up_threshold=1e32)
        assert ok == out["applied"] == (it != 2) and guard.flags == out["flags"]
        if ok:
            opt.step()
            assert guard.lr_used == sched.value(t + 1) == opt.param_groups[0]["lr"]
        w, m, v, t = out["w"], out["m"], out["v"], out["t"]
        np.testing.assert_allclose(w, p.detach().numpy(), rtol=RTOL, atol=ATOL)
    assert guard.stats["applied"] == 4 and guard.stats["skipped"] == 1 and guard.stats["first_skipped"] == 3 and guard.t == 4
