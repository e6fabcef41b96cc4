"""GPU tests of the guarded training step (csrc/step_ctl.hip): gradient-norm clipping, skip on a non-finite or exploding step, and a
learning rate that lives on the device.  First the finalize alone on hand-made vectors (no network kernel runs there: NaN and Inf
inputs are plain arithmetic), then whole steps on the smallest networks of the suite against the default step, the module-API
loop, the numpy restatement (tests/_train_ctl_ref.py) and torch.optim."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import _train_ctl_ref as T
import _util as U
from test_gpu_optimizer_options import LR, UPDATE_TOL, _setup

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SHARE = 1024                     # parameters per workgroup of the two kernels: 256 threads x 4
SIZES = [1, SHARE - 1, SHARE + 1, 66001]        # 66 001: 65 workgroups, the last one ragged
NB = 5                           # per-jet loss terms
L1, L2 = 1e-6, 1e-5


def _inputs(n, seed=0):
    g = torch.Generator().manual_seed(1000 + n + seed)
    w = torch.randn(n, generator=g, dtype=torch.float64)
    if n > 4:
        w[3] = 0.0               # sign(0) = 0
    grads = [torch.randn(n, generator=g, dtype=torch.float64) * (1.0 + k) for k in range(3)]
    lp = torch.rand(NB, generator=g, dtype=torch.float64) + 0.5
    return w.to(DEV), [x.to(DEV) for x in grads], lp.to(DEV)


class Fin:
    """One parameter vector with its optimiser state and the blocks of a finalize call."""

    def __init__(self, w, kind, ctl: bool, lr=LR):
        from lgn import _native as N
        self.N, self.ctl_form, self.kind, n = N, ctl, kind, w.numel()
        self.w, self.g = w.clone(), torch.zeros(n, device=DEV, dtype=torch.float64)
        self.m, self.v = torch.zeros_like(self.w), torch.zeros_like(self.w)
        self.step = torch.zeros(1, device=DEV, dtype=torch.int64)
        self.loss = torch.zeros(4 + (N.FINALIZE_CTL_SCRATCH if ctl else N.FINALIZE_OPT_SCRATCH), device=DEV, dtype=torch.float64)
        self.ctl = torch.zeros(N.CTL_DOUBLES, device=DEV, dtype=torch.float64)
        self.d = d = N.OptimDesc()
        d.kind = N.OPT_ADAM if kind == "adam" else N.OPT_RMSPROP
        d.l1_lambda, d.l2_lambda, d.lr, d.eps = L1, L2, lr, 1e-8 if kind == "adam" else 1e-16
        d.beta1, d.beta2, d.alpha, d.momentum = 0.9, 0.999, 0.99, 0.9

    def call(self, g, lp, do_step=1, lr_kind=0, **controls):
        N = self.N
        self.g.copy_(g)
        head = (N.ptr(self.w), N.ptr(self.g), self.w.numel(), N.ptr(lp), lp.numel(), C.byref(self.d), N.ptr(self.m), N.ptr(self.v),
                N.ptr(self.step), int(do_step), N.ptr(self.loss))
        if self.ctl_form:
            tc = N.TrainCtl()
            tc.lr_kind = lr_kind
            for k, val in controls.items():
                setattr(tc, k, val)
            N._check(N.lib().lgn_step_finalize_ctl_f64(*head, C.byref(tc), N.ptr(self.ctl), N.stream_ptr()), "lgn_step_finalize_ctl_f64")
        else:
            N._check(N.lib().lgn_step_finalize_opt_f64(*head, N.stream_ptr()), "lgn_step_finalize_opt_f64")
        torch.cuda.synchronize()
        # the scratch is zero again after every call: partial sums and the counter (slots -7 .. -2 cache Adam's powers, as documented)
        scratch = self.loss[4:]
        assert float(scratch[:-7].abs().sum()) == 0.0 and float(scratch[-1]) == 0.0, "scratch slots left non-zero"
        return self.ctl.cpu().numpy().copy()

    def state(self):
        return self.w.clone(), self.m.clone(), self.v.clone(), self.step.clone()

    def same_state(self, other, what):
        for name, a, b in zip(("weights", "state m", "state v", "step counter"), self.state(), other if isinstance(other, tuple) else other.state()):
            assert torch.equal(a, b), f"{what}: {name} differ"


def _assert_update_close(upd, upd_ref, w0, tol, what):
    """The update as tests/test_gpu_optimizer_options.py measures it: relative to the largest update of the step, and per element
    -- tol of the element's OWN update plus 2 ulp of |w0| (the update is read off as a difference of weights, and the two sides
    may round the weight in opposite directions) -- so that an error confined to parameters with small updates cannot hide behind
    the largest one.  Returns the max-norm figure."""
    upd, upd_ref = upd.detach().cpu(), upd_ref.detach().cpu()
    e = U.assert_close(upd, upd_ref, tol, f"{what}: update")
    ulp = torch.from_numpy(np.spacing(w0.detach().abs().cpu().numpy()))
    excess = (upd - upd_ref).abs() - (tol * upd_ref.abs() + 2.0 * ulp)
    assert float(excess.max()) <= 0.0, f"{what}: element {int(excess.argmax())} is off by more than its own update allows"
    return e


def _flags(c):
    from lgn import _native as N
    return int(c[N.CTL_FLAGS])


@pytest.mark.parametrize("do_step", [0, 1])
@pytest.mark.parametrize("kind", ["adam", "rmsprop"])
@pytest.mark.parametrize("n", SIZES)
def test_controls_off_gives_the_bits_of_the_descriptor_finalize_and_the_norm_of_the_gradient(n, kind, do_step):
    """Clipping off, threshold off, LGN_LR_HOST, three consecutive calls, the two finalize calls taking turns on blocks of their
    own (neither disturbs the other): weights, both states, grads and the counter are torch.equal; loss_out agrees to 1e-10; and
    GRAD_NORM is the norm of the returned gradient to n 2^-52, the bound for re-ordering a sum of n non-negative terms plus the root."""
    from lgn import _native as N
    w, grads, lp = _inputs(n)
    a, b = Fin(w, kind, ctl=True), Fin(w, kind, ctl=False)
    for k in range(3):
        c = a.call(grads[k], lp, do_step)
        b.call(grads[k], lp, do_step)
        a.same_state(b, f"call {k}")
        assert torch.equal(a.g, b.g), f"call {k}: grads differ"
        U.assert_close(a.loss[:4], b.loss[:4], 1e-10, f"call {k}: loss_out")
        want = float(torch.linalg.vector_norm(a.g.cpu()))
        print(f"n {n} {kind} call {k}: GRAD_NORM {c[N.CTL_GRAD_NORM]!r} torch {want!r}")
        assert abs(c[N.CTL_GRAD_NORM] - want) <= n * 2.0 ** -52 * want
        assert c[N.CTL_CLIP_COEF] == 1.0 and _flags(c) == 0 and c[N.CTL_LR_USED] == LR
        assert c[N.CTL_APPLIED] == (k + 1) * do_step and c[N.CTL_SKIPPED] == 0 and c[N.CTL_FIRST_SKIPPED] == 0
    assert int(a.step.item()) == 3 * do_step
    if not do_step:              # gradients and loss only: the running fields are left alone, the state too
        assert not c[N.CTL_APPLIED:N.CTL_APPLIED_LOSS_SUM + 1].any() and torch.equal(a.w, w) and not a.m.any() and not a.v.any()
    else:
        assert c[N.CTL_GRAD_NORM_MAX] > 0 and c[N.CTL_APPLIED_LOSS_SUM] > 0
        N._check(N.lib().lgn_train_ctl_reset(N.ptr(a.ctl), N.stream_ptr()), "lgn_train_ctl_reset")
        r = a.ctl.cpu().numpy()
        assert not r[N.CTL_APPLIED:N.CTL_APPLIED_LOSS_SUM + 1].any() and r[N.CTL_LR_USED] == LR and r[N.CTL_GRAD_NORM] == c[N.CTL_GRAD_NORM]


def _torch_update(w0, G, coef_max_norm, kind, lr, m0, v0, t):
    """clip_grad_norm_ + the torch optimiser on the gradient G from the state (m0, v0, t applied steps)."""
    from lgn.step import torch_optimizer
    p = torch.nn.Parameter(w0.detach().cpu().clone())
    opt = torch_optimizer([p], kind, lr, None)
    p.grad = G.detach().cpu().clone()
    if t > 0:                    # torch's state = the state before this step
        p.grad.zero_()
        opt.step()
        st = opt.state[p]
        with torch.no_grad():
            p.copy_(w0.cpu())
        st["square_avg" if kind == "rmsprop" else "exp_avg_sq"].copy_(v0.cpu())
        st["momentum_buffer" if kind == "rmsprop" else "exp_avg"].copy_(m0.cpu())
        st["step"] = torch.tensor(float(t)) if torch.is_tensor(st["step"]) else t
        p.grad = G.detach().cpu().clone()
    if coef_max_norm is not None:
        torch.nn.utils.clip_grad_norm_([p], coef_max_norm)
    opt.step()
    st = opt.state[p]
    return p.detach(), st["momentum_buffer" if kind == "rmsprop" else "exp_avg"], st["square_avg" if kind == "rmsprop" else "exp_avg_sq"]


@pytest.mark.parametrize("kind", ["adam", "rmsprop"])
@pytest.mark.parametrize("n", SIZES)
def test_clipping(n, kind):
    """norm0 is measured with clipping off.  max_grad_norm = 2 norm0: CLIP_COEF is exactly 1.0 and the bits are the unclipped
    call's.  max_grad_norm = 0.5 norm0: the CLIPPED bit, grads stay unclipped, weights and states agree with the numpy restatement
    and with clip_grad_norm_ + the torch optimiser on the same G at UPDATE_TOL + n 2^-52 (the norm's own re-ordering bound),
    measured as tests/test_gpu_optimizer_options.py measures it: the update w_after - w_before relative to the largest update, and
    per element against its own update plus 2 ulp of |w0| (_assert_update_close)."""
    from lgn import _native as N
    w, grads, lp = _inputs(n)
    tol = UPDATE_TOL + n * 2.0 ** -52
    plain = Fin(w, kind, ctl=True)
    norm0 = plain.call(grads[0], lp)[N.CTL_GRAD_NORM]
    loose = Fin(w, kind, ctl=True)
    c = loose.call(grads[0], lp, max_grad_norm=2.0 * norm0)
    assert c[N.CTL_CLIP_COEF] == 1.0 and _flags(c) == 0 and c[N.CTL_CLIPPED_STEPS] == 0
    loose.same_state(plain, "max_grad_norm = 2 norm0")
    assert torch.equal(loose.g, plain.g)
    # a second step from a non-trivial state, clipped
    tight = Fin(w, kind, ctl=True)
    tight.call(grads[0], lp)
    w0, m0, v0, _ = tight.state()
    c = tight.call(grads[1], lp, max_grad_norm=0.5 * norm0)
    unclipped = Fin(w, kind, ctl=True)
    unclipped.call(grads[0], lp)
    unclipped.call(grads[1], lp)
    assert _flags(c) == N.CTL_CLIPPED and c[N.CTL_CLIPPED_STEPS] == 1 and c[N.CTL_APPLIED] == 2 and int(tight.step.item()) == 2
    assert torch.equal(tight.g, unclipped.g), "grads must hold the unclipped regularised gradient"
    norm1 = float(torch.linalg.vector_norm(tight.g.cpu()))
    want = 0.5 * norm0 / (norm1 + 1e-6)
    assert want < 1.0 and abs(c[N.CTL_CLIP_COEF] - want) <= (n * 2.0 ** -52 + 4 * 2.0 ** -52) * want
    ref = T.controlled_step(w0.cpu().numpy(), grads[1].cpu().numpy(), m0.cpu().numpy(), v0.cpu().numpy(), 1, data=float(lp.sum()),
                            kind=kind, lr=LR, l1=L1, l2=L2, max_grad_norm=0.5 * norm0)
    assert ref["applied"] and ref["flags"] == T.CLIPPED
    tw, tm, tv = _torch_update(w0, tight.g, 0.5 * norm0, kind, LR, m0, v0, 1)
    upd = (tight.w - w0).cpu()
    for who, rw, rm, rv in (("numpy", torch.from_numpy(ref["w"]), torch.from_numpy(ref["m"]), torch.from_numpy(ref["v"])), ("torch", tw, tm, tv)):
        e = _assert_update_close(upd, rw - w0.cpu(), w0, tol, who)
        U.assert_close(tight.w, rw, tol, f"{who}: weights")
        U.assert_close(tight.m, rm, tol, f"{who}: state m")
        U.assert_close(tight.v, rv, tol, f"{who}: state v")
        print(f"n {n} {kind}: clipped update against {who}: {e:.3e} (bound {tol:.3e})")
    assert not torch.equal(tight.w, unclipped.w)


BAD = {"nan_in_g": ("g", float("nan"), {"skip_nonfinite": 1}, "nonfinite"),
       "inf_in_g": ("g", float("inf"), {"skip_nonfinite": 1}, "nonfinite"),
       "nan_in_loss_part": ("lp", float("nan"), {"skip_nonfinite": 1}, "nonfinite"),
       "blow_up": (None, None, {"blow_up_threshold": 1e-30}, "blowup")}


@pytest.mark.parametrize("kind", ["adam", "rmsprop"])
@pytest.mark.parametrize("case", sorted(BAD))
@pytest.mark.parametrize("n", SIZES)
def test_a_bad_step_is_skipped_and_leaves_no_trace(n, case, kind):
    """One clean step, the bad one, one clean step: the bad call changes neither weights nor states nor the counter, sets its flag,
    counts in SKIPPED and names its t in FIRST_SKIPPED; the clean call behind it gives the bits of a run that never saw the bad
    step."""
    from lgn import _native as N
    where, value, controls, why = BAD[case]
    w, grads, lp = _inputs(n)
    g_bad, lp_bad = grads[1].clone(), lp.clone()
    if where == "g":
        g_bad[n // 2] = value
    elif where == "lp":
        lp_bad[2] = value
    a, clean = Fin(w, kind, ctl=True), Fin(w, kind, ctl=True)
    a.call(grads[0], lp, **controls) if case != "blow_up" else a.call(grads[0], lp)
    clean.call(grads[0], lp)
    a.same_state(clean, "first step")
    before = a.state()
    c = a.call(g_bad, lp_bad, **controls)
    a.same_state(before, case)
    bit = N.CTL_SKIP_NONFINITE if why == "nonfinite" else N.CTL_SKIP_BLOWUP
    assert _flags(c) & bit and not _flags(c) & (N.CTL_SKIP_NONFINITE | N.CTL_SKIP_BLOWUP) & ~bit
    assert c[N.CTL_SKIPPED] == 1 and c[N.CTL_FIRST_SKIPPED] == 2 and c[N.CTL_APPLIED] == 1 and c[N.CTL_APPLY] == 0
    assert math.isfinite(c[N.CTL_GRAD_NORM_MAX]) and math.isfinite(c[N.CTL_APPLIED_LOSS_SUM])
    c = a.call(grads[2], lp, **({} if case == "blow_up" else controls))
    clean.call(grads[2], lp)
    a.same_state(clean, "the clean step behind the skipped one")
    assert torch.equal(a.g, clean.g) and int(a.step.item()) == 2
    assert c[N.CTL_SKIPPED] == 1 and c[N.CTL_FIRST_SKIPPED] == 2 and c[N.CTL_APPLIED] == 2 and _flags(c) == 0


@pytest.mark.parametrize("kind", ["adam", "rmsprop"])
def test_without_skip_nonfinite_the_nan_propagates_as_in_torch(kind):
    """skip_nonfinite off, no clipping: the NaN reaches exactly the element it sits in (elementwise rules), as torch.optim does it;
    with clipping on, the NaN norm makes the coefficient NaN and every weight NaN, as clip_grad_norm_ does it."""
    from lgn import _native as N
    n = SHARE + 1
    w, grads, lp = _inputs(n)
    g_bad = grads[0].clone()
    g_bad[7] = float("nan")
    a, clean = Fin(w, kind, ctl=True), Fin(w, kind, ctl=True)
    c = a.call(g_bad, lp, blow_up_threshold=1e32)
    clean.call(grads[0], lp)
    keep = torch.ones(n, dtype=torch.bool, device=DEV)
    keep[7] = False
    assert _flags(c) == 0 and c[N.CTL_APPLIED] == 1 and math.isnan(c[N.CTL_GRAD_NORM]) and c[N.CTL_GRAD_NORM_MAX] == 0
    assert torch.isnan(a.w[7]) and torch.equal(a.w[keep], clean.w[keep]) and torch.equal(a.v[keep], clean.v[keep])
    tw, _, _ = _torch_update(w, a.g, None, kind, LR, None, None, 0)
    assert torch.isnan(tw[7]) and int(torch.isnan(tw).sum()) == 1
    b = Fin(w, kind, ctl=True)
    c = b.call(g_bad, lp, max_grad_norm=1.0)
    assert math.isnan(c[N.CTL_CLIP_COEF]) and bool(torch.isnan(b.w).all())
    tw, _, _ = _torch_update(w, a.g, 1.0, kind, LR, None, None, 0)
    assert bool(torch.isnan(tw).all())


def test_device_lr_and_schedules_in_the_finalize_alone():
    """LGN_LR_DEVICE reads ctl[LGN_CTL_LR]; the schedules follow t = *step_dev + 1, which a skipped step does not advance."""
    from lgn import _native as N
    n = SHARE + 1
    w, grads, lp = _inputs(n)
    a, b = Fin(w, "adam", ctl=True), Fin(w, "adam", ctl=True, lr=2e-4)
    a.ctl[N.CTL_LR] = 2e-4
    c = a.call(grads[0], lp, lr_kind=N.LR_DEVICE)
    b.call(grads[0], lp)
    assert c[N.CTL_LR_USED] == 2e-4
    a.same_state(b, "device lr against the same host lr")
    sched = dict(kind=T.LR_WARMUP_STEP, base_lr=1e-3, warmup_steps=1, gamma=0.5, step_size=2)
    kw = dict(lr_kind=N.LR_WARMUP_STEP, base_lr=1e-3, warmup_steps=1, gamma=0.5, step_size=2)
    s = Fin(w, "rmsprop", ctl=True)
    for t in range(1, 6):
        c = s.call(grads[t % 3], lp, **kw)
        want = T.lr_value(sched, t)
        assert abs(c[N.CTL_LR_USED] - want) <= 1e-13 * want, (t, c[N.CTL_LR_USED], want)
        if t == 3:
            c = s.call(grads[0], lp, blow_up_threshold=1e-30, **kw)
            assert _flags(c) == N.CTL_SKIP_BLOWUP and int(s.step.item()) == 3 and c[N.CTL_FIRST_SKIPPED] == 4


# ---- whole steps ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("use_graph", [False, True], ids=["eager", "graph"])
@pytest.mark.parametrize("name", ["g1_e2e_maxdim2.npz", "g2_e2e_maxdim3.npz"])
def test_all_controls_off_forced_into_the_controlled_form_is_the_default_step(name, use_graph, monkeypatch):
    """_OptimState._force_ctl: three steps through lgn_step_fwd_bwd_f64 + lgn_step_finalize_ctl_f64 against the default
    NativeTrainStep -- parameters, states, counter and flat.grad torch.equal, the loss to 1e-10."""
    from lgn import step as S
    runs = []
    for force in (False, True):
        monkeypatch.setattr(S._OptimState, "_force_ctl", force)
        m, enc, dec, batch = _setup(name)
        st = S.NativeTrainStep(enc, dec, batch_size=m["B"], lr=1e-3, l1_lambda=1e-6, use_graph=use_graph)
        assert st.opt_state.ctl_form == force
        losses = torch.stack([st.step(batch)[0].clone() for _ in range(3)])
        torch.cuda.synchronize()
        runs.append((losses, st.flat.flat.clone(), st.adam_m.clone(), st.adam_v.clone(), st.flat.grad.clone(), st.step_dev.clone()))
        if force:
            assert st.control_stats()["applied"] == 3 and float(st.clip_coef) == 1.0 and float(st.lr_used) == 1e-3
    for what, x, y in zip(("losses", "weights", "Adam m", "Adam v", "gradients", "step counter"), *runs):
        if what == "losses":
            U.assert_close(y, x, 1e-10, what)
        else:
            assert torch.equal(x, y), f"{what}: the controlled form differs from the default step"
    assert int(runs[1][5].item()) == 3


def test_the_default_step_refuses_the_control_methods():
    from lgn.step import NativeTrainStep
    m, enc, dec, batch = _setup()
    st = NativeTrainStep(enc, dec, batch_size=m["B"], use_graph=False)
    assert not st.opt_state.ctl_form and st.ctl is None
    for call in (st.control_stats, st.reset_control, lambda: st.set_lr(1e-3), st.lr_handle):
        with pytest.raises(ValueError):
            call()


def _norm0(opts):
    """The gradient norm of the first step, from a probe that only looks (the controlled form, optimiser off)."""
    from lgn.step import NativeTrainStep
    m, enc, dec, batch = _setup()
    probe = NativeTrainStep(enc, dec, batch_size=m["B"], optimizer=False, use_graph=False, skip_nonfinite=True, **opts)
    probe.step(batch)
    return float(probe.grad_norm)


@pytest.mark.parametrize("use_graph", [False, True], ids=["eager", "graph"])
@pytest.mark.parametrize("choice", ["adam", "rmsprop"])
def test_clipped_step_matches_the_reference_loop(choice, use_graph):
    """max_grad_norm = 0.5 norm0 against ReferenceLoopStep with the same keywords (clip_grad_norm_ over both networks, two torch
    optimisers) over 3 steps: the loss per step at 1e-10, the parameters at 1e-9 -- the tolerances of
    test_rmsprop_l2_step_matches_the_reference_loop_on_the_module_api (l1_lambda > 0 for the reason given there)."""
    from lgn.step import NativeTrainStep, ReferenceLoopStep
    opts = dict(optimizer_choice=choice, l1_lambda=1e-6, lr=LR)
    norm0 = _norm0(opts)
    opts["max_grad_norm"] = 0.5 * norm0
    m, enc, dec, batch = _setup()
    _, enc2, dec2, _ = _setup()
    nat = NativeTrainStep(enc2, dec2, batch_size=m["B"], use_graph=use_graph, **opts)
    loop = ReferenceLoopStep(enc, dec, **opts)
    for it in range(3):
        lb, _ = loop.step(batch)
        la, _ = nat.step(batch)
        U.assert_close(la, lb, 1e-10, f"loss at step {it}")
        assert int(nat.ctl_flags) == loop.guard.flags and (it > 0 or loop.guard.flags == 1), "both clip the same steps, the first for sure"
        # the two gradients come from different kernels (whole-step call / autograd over the per-network calls); the suite holds them
        # to 1e-9 of the largest entry (test_gpu_step_loss_options.py: "flat gradient"), so the norms of n entries may differ by
        # sqrt(n) 1e-9 max|G| <= sqrt(n) 1e-9 norm
        e = U.assert_close(nat.grad_norm, torch.tensor(loop.guard.grad_norm), math.sqrt(nat.flat.flat.numel()) * 1e-9, f"gradient norm at step {it}")
        print(f"{choice} step {it}: gradient norm, native against the loop: {e:.3e}")
    U.assert_close(torch.cat([enc.flat_params.detach(), dec.flat_params.detach()]), nat.flat.flat, 1e-9, "parameters after 3 steps")
    assert nat.control_stats() == dict(nat.control_stats(), applied=3, clipped=loop.guard.stats["clipped"], skipped=0, first_skipped=0)


def _reference_update(step, w0, m0, v0, t, lr, l1, kind="adam", **controls):
    """The numpy restatement fed with the native step's own raw gradient and loss, and the given learning rate."""
    raw = (step.flat.grad - l1 * torch.sign(w0)).cpu().numpy()
    return T.controlled_step(w0.cpu().numpy(), raw, m0.cpu().numpy(), v0.cpu().numpy(), t, data=float(step.loss_out[1]), kind=kind,
                             lr=lr, l1=l1, **controls)


def test_live_learning_rate_changes_between_replays_without_a_new_capture():
    """lr_schedule='device' with a captured graph: set_lr between replays changes lr_used and the update, the graph object stays the
    same; weights agree with the numpy restatement fed with lr_used read back per step, at UPDATE_TOL.  lr_handle() drives the same
    write from a torch scheduler."""
    from lgn.step import NativeTrainStep
    m, enc, dec, batch = _setup()
    l1 = 1e-8
    step = NativeTrainStep(enc, dec, batch_size=m["B"], lr=LR, l1_lambda=l1, use_graph=True, lr_schedule="device")
    step.step(batch)
    graph = step._g1
    assert graph is not None and float(step.lr_used) == LR
    handle = step.lr_handle()
    sched = torch.optim.lr_scheduler.ReduceLROnPlateau(handle, factor=0.5, patience=0)
    updates = []
    for it, lr in enumerate((2e-4, 1e-3, None)):
        if lr is None:           # two "epochs" without improvement: ReduceLROnPlateau halves the handle's rate
            sched.step(1.0)
            sched.step(1.0)
            handle.sync_lr()
            lr = 5e-4
            assert handle.param_groups[0]["lr"] == lr
        else:
            step.set_lr(lr)
            handle.param_groups[0]["lr"] = lr
        w0, m0, v0, t = step.flat.flat.clone(), step.adam_m.clone(), step.adam_v.clone(), int(step.step_dev.item())
        step.step(batch)
        torch.cuda.synchronize()
        assert step._g1 is graph, "set_lr must not capture again"
        used = float(step.lr_used)
        assert used == lr
        ref = _reference_update(step, w0, m0, v0, t, used, l1)
        upd = (step.flat.flat - w0).cpu()
        _assert_update_close(upd, torch.from_numpy(ref["w"]) - w0.cpu(), w0, UPDATE_TOL, f"lr {lr}")
        updates.append(float(upd.abs().max()))
    assert updates[0] < 0.5 * updates[1], "a five times larger rate must show in the update"
    assert int(step.step_dev.item()) == 4
    _, enc2, dec2, _ = _setup()
    for kw in (dict(max_grad_norm=1.0), dict()):
        other = NativeTrainStep(enc2, dec2, batch_size=m["B"], use_graph=False, **kw)
        with pytest.raises(ValueError):
            other.set_lr(1e-3)


def test_warmup_cosine_schedule_follows_the_applied_steps():
    """LGN_LR_WARMUP_COSINE with W = 2, T = 6 over 8 steps: lr_used per step against lr_value (relative 1e-13), weights against the
    restatement fed with the device's lr_used (UPDATE_TOL); a step skipped in the middle -- blow_up_threshold = 1e-30 on a second
    step object that shares the state -- does not advance t."""
    from lgn.step import LRSchedule, NativeTrainStep
    m, enc, dec, batch = _setup()
    l1 = 1e-8
    sched = LRSchedule("cosine", LR, warmup_steps=2, total_steps=6, min_lr=1e-5)
    ref_sched = dict(kind=T.LR_WARMUP_COSINE, base_lr=LR, min_lr=1e-5, warmup_steps=2, total_steps=6)
    step = NativeTrainStep(enc, dec, batch_size=m["B"], lr=LR, l1_lambda=l1, use_graph=True, lr_schedule=sched)
    skipper = NativeTrainStep(enc, dec, batch_size=m["B"], lr=LR, l1_lambda=l1, use_graph=False, lr_schedule=sched,
                              blow_up_threshold=1e-30, _share=step)
    assert skipper.ctl is step.ctl and skipper.step_dev is step.step_dev
    for t in range(1, 9):
        w0, m0, v0 = step.flat.flat.clone(), step.adam_m.clone(), step.adam_v.clone()
        step.step(batch)
        torch.cuda.synchronize()
        used, want = float(step.lr_used), T.lr_value(ref_sched, t)
        print(f"step {t}: lr_used {used!r} closed form {want!r}")
        assert abs(used - want) <= 1e-13 * want and int(step.step_dev.item()) == t and int(step.ctl_flags) == 0
        ref = _reference_update(step, w0, m0, v0, t - 1, used, l1)
        _assert_update_close(step.flat.flat - w0, torch.from_numpy(ref["w"]) - w0.cpu(), w0, UPDATE_TOL, f"step {t}")
        if t == 4:
            before = step.opt_state.snapshot()
            skipper.step(batch)
            torch.cuda.synchronize()
            for x, y in zip(before[:4], (step.flat.flat, step.adam_m, step.adam_v, step.step_dev)):
                assert torch.equal(x, y), "a skipped step changed the state"
            want5 = T.lr_value(ref_sched, 5)         # the skipped call evaluated the schedule at t = 5, which stays the next t
            assert int(skipper.ctl_flags) == 4 and abs(float(skipper.lr_used) - want5) <= 1e-13 * want5
    assert float(step.lr_used) == 1e-5          # t = 7, 8 > T: held at min_lr
    assert step.control_stats() == dict(step.control_stats(), applied=8, skipped=1, first_skipped=5, clipped=0)
    step.reset_control()
    assert step.control_stats() == dict(applied=0, clipped=0, skipped=0, first_skipped=0, grad_norm_max=0.0, applied_loss_sum=0.0)


def test_single_rank_all_reduce_branch_gives_the_single_process_bits(monkeypatch):
    """force_collective=True on one rank (fwd_bwd | all-reduce | guarded finalize, eager and as graph | all-reduce | graph) against
    the single-process guarded step: torch.equal."""
    import socket
    import torch.distributed as dist
    from lgn.step import LRSchedule, NativeTrainStep
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    monkeypatch.setenv("MASTER_ADDR", "127.0.0.1")
    monkeypatch.setenv("MASTER_PORT", str(port))
    opts = dict(lr=LR, l1_lambda=1e-6, skip_nonfinite=True, blow_up_threshold=1e32,
                lr_schedule=LRSchedule("cosine", LR, warmup_steps=1, total_steps=5))
    opts["max_grad_norm"] = 0.5 * _norm0(dict(lr=LR, l1_lambda=1e-6))
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
    try:
        forms = {"single": dict(use_graph=True), "collective_eager": dict(use_graph=False, force_collective=True),
                 "collective_two_graphs": dict(use_graph=True, force_collective=True, graph_collective=False)}
        runs = {}
        for form, kw in forms.items():
            m, enc, dec, batch = _setup()
            st = NativeTrainStep(enc, dec, batch_size=m["B"], **opts, **kw)
            for _ in range(3):
                st.step(batch)
            torch.cuda.synchronize()
            assert st.control_stats()["applied"] == 3 and st.control_stats()["clipped"] >= 1
            if form == "collective_two_graphs":
                assert st.launches_per_step == 3
            runs[form] = (st.flat.flat.clone(), st.flat.grad.clone(), st.adam_m.clone(), st.adam_v.clone(), st.step_dev.clone(),
                          st.ctl[:11].clone())
        for form, r in runs.items():
            for what, x, y in zip(("weights", "gradients", "Adam m", "Adam v", "step counter", "control block"), runs["single"], r):
                assert torch.equal(x, y), f"{form}: {what} differ from the single-process step"
    finally:
        dist.destroy_process_group()


def test_captured_module_step_takes_the_controls():
    """CapturedModuleStep with the same keywords against NativeTrainStep on g1, three steps: the loss per step and the parameters
    at 1e-9, as the existing module-versus-native step tests hold them (test_chooser_takes_the_native_step_for_loss_options)."""
    from lgn.step import CapturedModuleStep, LRSchedule, NativeTrainStep
    opts = dict(lr=LR, l1_lambda=1e-6, skip_nonfinite=True, lr_schedule=LRSchedule("step", LR, warmup_steps=1, gamma=0.5, step_size=1))
    opts["max_grad_norm"] = 0.5 * _norm0(dict(lr=LR, l1_lambda=1e-6))
    m, enc, dec, batch = _setup()
    _, enc2, dec2, _ = _setup()
    a = NativeTrainStep(enc, dec, batch_size=m["B"], use_graph=True, **opts)
    b = CapturedModuleStep(enc2, dec2, batch_size=m["B"], use_graph=True, **opts)
    assert b.opt_state.ctl_form
    for it in range(3):
        la, _ = a.step(batch)
        lb, _ = b.step(batch)
        U.assert_close(lb, la, 1e-9, f"loss at step {it}")
        assert float(a.lr_used) == float(b.lr_used) == LR * 0.5 ** max(0, it - 1) and int(a.ctl_flags) == int(b.ctl_flags)
    U.assert_close(b.flat.flat, a.flat.flat, 1e-9, "parameters after 3 steps")
    assert a.control_stats()["applied"] == b.control_stats()["applied"] == 3
