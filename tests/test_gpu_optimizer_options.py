"""GPU tests of the optimiser options of the training steps: ``optimizer_choice='rmsprop'`` and ``l2_lambda`` run in the native tail
(lgn_step_train_opt_f64 / lgn_step_finalize_opt_f64: csrc/step_tail.hip, l1_adam_kernel of csrc/net_kernels.hip, the update rules of
csrc/tail_dev.hpp) and are held to torch.optim on the same gradients, to the module-API loop, and to each other across the forms a
step can take.  Defaults (Adam, no L2) keep the old entry points; their bits are pinned by the existing suites."""
import numpy as np
import pytest
import torch

import _util as U

pytestmark = pytest.mark.gpu

LR = 5e-4
# Largest deviation of the update w_after - w_before between the native tail and torch.optim on the same gradient, relative to the
# largest update of the step (U.relerr).  Both sides do the same ten or so fp64 operations per element (<= 1 ulp each where a
# product is fused differently); the update itself is read off as a difference of weights of size <= 4, which costs up to an ulp
# of the weight, 4.4e-16, against updates of lr / sqrt(1 - alpha) = 5e-3 (RMSprop) or lr = 5e-4 (Adam): 1e-13 .. 1e-12 expected.
# Measured on the first GPU run: 2.22e-13 at most (Adam + L2 on g2; RMSprop 1.1e-14 .. 4.4e-14); the bound
# is that with a margin of 100 for ordering differences in torch's kernels, and stays below the 1e-9 the existing Adam test holds
# parameters to.
UPDATE_TOL = 2.2e-11
# The figure above is a maximum norm.  Element by element, an update read off as w_after - w_before carries the rounding of both
# weights, up to an ulp of |w| in all, whatever its own size: the per-element check below allows that ulp (2 np.spacing(|w0|): the
# two sides may round the weight in opposite directions) plus UPDATE_TOL of the element's OWN update, so an error confined to
# parameters with small updates does not hide behind the largest one.

CASES = {"rmsprop": dict(optimizer_choice="rmsprop", l1_lambda=1e-8),
         "rmsprop_mu0": dict(optimizer_choice="rmsprop", momentum=0.0, l1_lambda=1e-8),
         "rmsprop_l2": dict(optimizer_choice="rmsprop", l1_lambda=1e-8, l2_lambda=1e-6),
         "adam_l2": dict(optimizer_choice="adam", l1_lambda=1e-8, l2_lambda=1e-6)}


def _setup(name="g1_e2e_maxdim2.npz"):
    import __graft_entry__ as G
    dev = torch.device("cuda:0")
    z = U.load(name)
    m = U.meta(z)
    enc, dec = G._models(m["N"], m["ch_enc"], m["ch_dec"], dev, seed=m["seed"], maxdim=m.get("maxdim", 2))
    batch = {"p4": torch.from_numpy(z["p4"]).to(dev), "labels": torch.from_numpy(z["labels"]).to(dev)}
    return m, enc, dec, batch


def _torch_twin(w, kw):
    from lgn.step import torch_optimizer
    p = torch.nn.Parameter(w.clone())
    opt = torch_optimizer([p], kw["optimizer_choice"], LR, None, momentum=kw.get("momentum", 0.9), rms_alpha=kw.get("rms_alpha", 0.99))
    return p, opt


@pytest.mark.parametrize("use_graph", [False, True])
@pytest.mark.parametrize("name", ["g1_e2e_maxdim2.npz", "g2_e2e_maxdim3.npz"])
@pytest.mark.parametrize("case", sorted(CASES))
def test_native_update_matches_torch_optimizer_on_the_same_gradients(case, name, use_graph):
    """Three steps.  After each native step a torch optimiser, started from the native step's weights and state BEFORE the step, is
    fed the native raw gradient (step.flat.grad minus the regulariser terms of the pre-step weights) plus the L1 and L2 terms
    formed in torch: weights, square_avg / momentum buffer (or Adam's moments), the update itself and the step counter agree."""
    from lgn.step import NativeTrainStep
    kw = CASES[case]
    m, enc, dec, batch = _setup(name)
    step = NativeTrainStep(enc, dec, batch_size=m["B"], lr=LR, use_graph=use_graph, **kw)
    l1, l2 = kw.get("l1_lambda", 0.0), kw.get("l2_lambda", 0.0)
    rms = kw["optimizer_choice"] == "rmsprop"
    assert step.opt_state.opt_form and step.eps == (1e-16 if rms else 1e-8)
    p, opt = _torch_twin(step.flat.flat, kw)
    worst = 0.0
    for it in range(3):
        w0, m0, v0 = step.flat.flat.clone(), step.adam_m.clone(), step.adam_v.clone()
        step.step(batch)
        torch.cuda.synchronize()
        raw = step.flat.grad - l1 * torch.sign(w0) - 2.0 * l2 * w0
        with torch.no_grad():
            p.copy_(w0)
            if it > 0:          # torch's state = the native state before this step: the comparison holds ONE tail, not their history
                st = opt.state[p]
                st["square_avg" if rms else "exp_avg_sq"].copy_(v0)
                if rms and kw.get("momentum", 0.9) > 0:
                    st["momentum_buffer"].copy_(m0)
                elif not rms:
                    st["exp_avg"].copy_(m0)
            p.grad = raw + l1 * torch.sign(p) + 2.0 * l2 * p
        opt.step()
        st = opt.state[p]
        upd, upd_t = step.flat.flat - w0, p.detach() - w0
        e = U.assert_close(upd, upd_t, UPDATE_TOL, f"{case} step {it}: update")
        worst = max(worst, e)
        ulp = torch.from_numpy(np.spacing(w0.abs().cpu().numpy())).to(w0.device)
        excess = (upd - upd_t).abs() - (UPDATE_TOL * upd_t.abs() + 2.0 * ulp)
        assert float(excess.max()) <= 0.0, f"{case} step {it}: element {int(excess.argmax())} is off by more than its own update allows"
        U.assert_close(step.flat.flat, p.detach(), UPDATE_TOL, f"{case} step {it}: weights")
        U.assert_close(step.square_avg, st["square_avg" if rms else "exp_avg_sq"], UPDATE_TOL, f"{case} step {it}: second-moment state")
        if rms and kw.get("momentum", 0.9) > 0:
            U.assert_close(step.momentum_buf, st["momentum_buffer"], UPDATE_TOL, f"{case} step {it}: momentum buffer")
        elif rms:
            assert not step.momentum_buf.any(), "momentum == 0 must leave the buffer alone"
        else:
            U.assert_close(step.adam_m, st["exp_avg"], UPDATE_TOL, f"{case} step {it}: first moment")
        assert int(step.step_dev.item()) == it + 1 == int(st["step"])
    print(f"largest relative deviation of the update, {case} {name} graph={use_graph}: {worst:.3e}")


@pytest.mark.parametrize("momentum", [0.9, 0.0])
def test_dead_parameters_do_not_move_without_regularisers(momentum):
    """A parameter whose loss gradient is exactly zero, under RMSprop with both lambdas 0: g / (sqrt(v) + eps) = 0 / eps = 0, the
    weight keeps its bits."""
    from lgn.step import NativeTrainStep
    m, enc, dec, batch = _setup()
    probe = NativeTrainStep(enc, dec, batch_size=m["B"], lr=LR, l1_lambda=0.0, optimizer=False, use_graph=False)
    probe.step(batch)
    dead = probe.flat.grad == 0
    assert dead.any() and not dead.all()
    m, enc, dec, batch = _setup()
    step = NativeTrainStep(enc, dec, batch_size=m["B"], lr=LR, l1_lambda=0.0, l2_lambda=0.0, optimizer_choice="rmsprop", momentum=momentum)
    w0 = step.flat.flat.clone()
    for _ in range(3):
        step.step(batch)
    torch.cuda.synchronize()
    assert torch.equal(step.flat.flat[dead], w0[dead])
    assert not torch.equal(step.flat.flat[~dead], w0[~dead])
    assert not step.square_avg[dead].any() and not step.momentum_buf[dead].any()


def test_rmsprop_l2_step_matches_the_reference_loop_on_the_module_api():
    """NativeTrainStep(optimizer_choice='rmsprop', l2_lambda=1e-6) against ReferenceLoopStep with the same options (two
    torch.optim.RMSprop, + l2_lambda * l2_norm() on the loss), 3 steps on g1: the loss per step at the tolerance of
    test_reference_loop_step_matches_native_step (1e-10), the parameters after step 3 at its 1e-9.

    l1_lambda > 0 on purpose.  The first RMSprop update is +-lr / sqrt(1 - alpha) whatever |g| is, so a parameter whose gradient
    is rounding noise on one path and an exact zero on the other would differ by a whole step; the L1 term gives both paths the
    same non-zero gradient there."""
    from lgn.step import NativeTrainStep, ReferenceLoopStep
    m, enc, dec, batch = _setup()
    _, enc2, dec2, _ = _setup()
    opts = dict(optimizer_choice="rmsprop", l2_lambda=1e-6, l1_lambda=1e-6, lr=LR)
    ref = NativeTrainStep(enc2, dec2, batch_size=m["B"], use_graph=True, **opts)
    loop = ReferenceLoopStep(enc, dec, **opts)
    assert type(loop.opt_enc).__name__ == "RMSprop" and loop.opt_enc.defaults["eps"] == 1e-16 == ref.eps
    for it in range(3):
        loss, _ = loop.step(batch)
        lr, _ = ref.step(batch)
        U.assert_close(loss, lr, 1e-10, f"loss at step {it}")
    U.assert_close(torch.cat([enc.flat_params.detach(), dec.flat_params.detach()]), ref.flat.flat, 1e-9, "parameters after 3 steps")


@pytest.mark.parametrize("split", [False, True])
@pytest.mark.parametrize("choice", ["adam", "rmsprop"])
def test_loss_terms(choice, split, monkeypatch):
    """loss_out[0] = loss_out[1] + l1 loss_out[2] + l2 l2_out; the two norms are those of the weights BEFORE the step."""
    from lgn.step import NativeTrainStep
    if split:
        monkeypatch.setenv("LGN_AMD_SPLIT_TAIL", "1")
    m, enc, dec, batch = _setup()
    l1, l2 = 1e-3, 1e-2
    step = NativeTrainStep(enc, dec, batch_size=m["B"], lr=LR, l1_lambda=l1, l2_lambda=l2, optimizer_choice=choice, use_graph=False)
    for it in range(2):
        with torch.no_grad():
            l1n, l2n = (enc.l1_norm() + dec.l1_norm()).double().cpu(), (enc.l2_norm() + dec.l2_norm()).double().cpu()
        step.step(batch)
        torch.cuda.synchronize()
        out, l2o = step.loss_out.cpu(), float(step.l2_out)
        U.assert_close(out[2], l1n, 1e-12, "sum |w| before the step")
        U.assert_close(step.l2_out.cpu()[0], l2n, 1e-12, "sum w^2 before the step")
        want = float(out[1]) + l1 * float(out[2]) + l2 * l2o
        assert abs(float(out[0]) - want) <= 4 * 2.2e-16 * abs(want), (float(out[0]), want)     # three roundings of the assembly
        assert l2 * l2o > 1e-6 * want                 # (the L2 term is visible in the total at this lambda)


@pytest.mark.parametrize("split", [False, True])
@pytest.mark.parametrize("name", ["g1_e2e_maxdim2.npz", "g2_e2e_maxdim3.npz"])
def test_adam_without_l2_through_the_new_entry_points_gives_the_old_bits(name, split, monkeypatch):
    """Adam with l2_lambda = 0 forced through lgn_step_train_opt_f64 (a private switch of _OptimState) against lgn_step_train_f64:
    weights, moments, gradients and counter are torch.equal after 3 steps, with the fused tail and with LGN_AMD_SPLIT_TAIL=1."""
    from lgn import step as S
    if split:
        monkeypatch.setenv("LGN_AMD_SPLIT_TAIL", "1")
    runs = []
    for force in (False, True):
        monkeypatch.setattr(S._OptimState, "_force_opt", force)
        m, enc, dec, batch = _setup(name)
        st = S.NativeTrainStep(enc, dec, batch_size=m["B"], lr=1e-3, l1_lambda=1e-6, use_graph=True)
        assert st.opt_state.opt_form == force
        losses = torch.stack([st.step(batch)[0].clone() for _ in range(3)])
        torch.cuda.synchronize()
        runs.append((losses, st.loss_out.clone(), st.flat.flat.clone(), st.adam_m.clone(), st.adam_v.clone(), st.flat.grad.clone(),
                     st.step_dev.clone()))
    for what, x, y in zip(("losses", "loss terms", "weights", "Adam m", "Adam v", "gradients", "step counter"), *runs):
        if what.startswith("loss"):
            U.assert_close(x, y, 1e-13, what)
        else:
            assert torch.equal(x, y), f"{what}: the descriptor call differs from the old one"
    assert int(runs[1][6].item()) == 3


def test_all_four_forms_of_the_rmsprop_l2_step_agree(monkeypatch):
    """single call | LGN_AMD_SPLIT_TAIL=1 | fwd_bwd + all-reduce on one rank + finalize, eager | the same, captured: the same
    weights after 3 steps; gradients and state bit for bit, the loss to rounding (its sums run over other partitions)."""
    import socket
    import torch.distributed as dist
    from lgn.step import NativeTrainStep
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    monkeypatch.setenv("MASTER_ADDR", "127.0.0.1")
    monkeypatch.setenv("MASTER_PORT", str(port))
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
    try:
        opts = dict(lr=LR, l1_lambda=1e-6, l2_lambda=1e-5, optimizer_choice="rmsprop")
        forms = {"single": dict(use_graph=True), "split": dict(use_graph=True),
                 "collective_eager": dict(use_graph=False, force_collective=True),
                 "collective_captured": dict(use_graph=True, force_collective=True)}
        runs = {}
        for form, kw in forms.items():
            if form == "split":
                monkeypatch.setenv("LGN_AMD_SPLIT_TAIL", "1")
            m, enc, dec, batch = _setup()
            st = NativeTrainStep(enc, dec, batch_size=m["B"], **opts, **kw)
            losses = torch.stack([st.step(batch)[0].clone() for _ in range(3)])
            if form == "split":
                monkeypatch.delenv("LGN_AMD_SPLIT_TAIL")
            torch.cuda.synchronize()
            assert int(st.step_dev.item()) == 3
            runs[form] = (losses, torch.cat([st.loss_out, st.l2_out]).clone(), st.flat.flat.clone(), st.flat.grad.clone(),
                          st.square_avg.clone(), st.momentum_buf.clone())
            scratch = st._loss_buf[4:]
            assert float(scratch[:-7].abs().sum()) == 0.0 and float(scratch[-1]) == 0.0, f"{form}: scratch slots left non-zero"
        base = runs["single"]
        for form, r in runs.items():
            for what, x, y in zip(("losses", "loss terms", "weights", "gradients", "square_avg", "momentum buffer"), base, r):
                if what.startswith("loss"):
                    U.assert_close(y, x, 1e-13, f"{form}: {what}")
                else:
                    assert torch.equal(x, y), f"{form}: {what} differ from the single call"
    finally:
        dist.destroy_process_group()


def test_fallback_step_takes_the_options_too():
    """A configuration the whole step refuses (map_to_latent='sum'): native_train_step(..., optimizer_choice='rmsprop') returns a
    CapturedModuleStep whose tail is lgn_step_finalize_opt_f64; its weights after 3 steps match ReferenceLoopStep's at 1e-9.
    (l1_lambda > 0 for the reason given in test_rmsprop_l2_step_matches_the_reference_loop_on_the_module_api.)"""
    import __graft_entry__ as G
    from lgn.step import CapturedModuleStep, ReferenceLoopStep, native_train_step
    from oracle import lgn_oracle as O
    dev = torch.device("cuda:0")
    N, B, chans = 12, 4, ((2, 3, 3, 4), (4, 3, 3, 2))
    build = lambda: G._models(N, chans[0], chans[1], dev, seed=7, map_to_latent="sum")      # noqa: E731
    p4, labels = O.synthetic_jets(B, N, seed=11, pad=True)
    batch = {"p4": p4.to(dev), "labels": labels.to(dev)}
    opts = dict(optimizer_choice="rmsprop", l2_lambda=1e-6, l1_lambda=1e-6, lr=LR)
    a = native_train_step(*build(), B, use_graph=True, **opts)
    assert isinstance(a, CapturedModuleStep) and a.opt_state.opt_form and a.optimizer_choice == "rmsprop"
    enc, dec = build()
    b = ReferenceLoopStep(enc, dec, **opts)
    for it in range(3):
        la, _ = a.step(batch)
        lb, _ = b.step(batch)
        U.assert_close(la, lb, 1e-10, f"loss at step {it}")
    U.assert_close(a.flat.flat, torch.cat([enc.flat_params.detach(), dec.flat_params.detach()]), 1e-9, "parameters after 3 steps")
    assert int(a.step_dev.item()) == 3


def test_eval_step_next_to_an_rmsprop_step_sees_the_updated_weights():
    from lgn.step import NativeEvalStep, NativeTrainStep
    m, enc, dec, batch = _setup()
    train = NativeTrainStep(enc, dec, batch_size=m["B"], lr=LR, optimizer_choice="rmsprop", l2_lambda=1e-6)
    ev = NativeEvalStep(enc, dec, m["B"], get_real_method="sum")
    before = float(ev.run(batch)["loss"])
    train.step(batch)
    after = float(ev.run(batch)["loss"])
    assert after != before
    _, enc2, dec2, _ = _setup()
    n = enc.flat_params.numel()
    with torch.no_grad():
        enc2.flat_params.copy_(train.flat.flat[:n])
        dec2.flat_params.copy_(train.flat.flat[n:])
    fresh = float(NativeEvalStep(enc2, dec2, m["B"], get_real_method="sum", use_graph=False).run(batch)["loss"])
    assert after == fresh
