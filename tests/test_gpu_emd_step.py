"""GPU tests of the EMD and hybrid losses as the loss stage of the native steps (csrc/emd_loss.hip, LGN_LOSS_EMD;
NativeTrainStep / NativeEvalStep / native_train_step / native_eval_step with ``native_emd=True``): the per-jet value is the EMD
score bit for bit, the gradients are the module-API step's and the oracle's, the hybrid loss accumulates on the step's Chamfer stage,
graph / eager / two-call forms and an EpochRunner epoch agree, flagged jets follow the step's contract, and a decoder that does not
fit is refused at plan time.  Tiny networks (two channels, two levels, live weights)."""
import numpy as np
import pytest
import torch

import _emd_grad_ref as G           # noqa: F401  (the restatements below build on it)
import _emd_opts_grad_ref as GO
import _emd_pairs_ref as P
import _emd_ref as E
import _normalize_ref as R
import _util as U

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
B = 4
CH = ((2, 2, 2), (2, 2, 2))
OPTS = {"default": {}, "beta2": dict(beta=2.0), "all": dict(R=0.8, beta=2.0, norm=True, periodic_phi=True)}
N_REAL = {6: 4}                     # N = 6 holds 4 real particles, the other sizes are full
# Batch seeds for which every jet's optimum is non-degenerate (_assert_nondegenerate asserts it, from the module-API step's
# reconstruction).  At 64 particles an optimum has 128 basic among 4160 arcs and a second optimum within 1e-6 is common: of the
# seeds 106 .. 110, 108 is the one whose four jets all have a unique basis.
SEEDS = {64: 108}


def _nets(N, n=1, maxdim=2, ch=CH):
    """n pairs of equal networks at live weights, and the CPU dicts the oracle gets"""
    import __graft_entry__ as GE
    out = []
    for _ in range(n):
        enc, dec = GE._models(N, ch[0], ch[1], torch.device(DEV), seed=23, maxdim=maxdim)
        out.append((enc, dec) + U.live_weights(enc, dec))
    return out


def _jets(N, seed=None, n_jets=B):
    seed = SEEDS.get(N, 106) if seed is None else seed
    p4 = R.jets(n_jets, N, seed=seed + N, n_real=N_REAL.get(N))
    return (p4 / (p4.abs().amax(dim=(1, 2), keepdim=True) + 1e-16)).contiguous()


def _batch(N, seed=None, n_jets=B):
    p4 = _jets(N, seed, n_jets)
    return {"p4": p4.to(DEV), "labels": (p4[..., 0] != 0).to(torch.uint8).to(DEV)}


def _module(loss):
    from lgn.losses import EMDLoss, HybridLoss
    kind, args = loss[0], loss[1:]
    return EMDLoss(**args[0]) if kind == "emd" else HybridLoss(args[0], **args[1])


def _native(enc, dec, loss, **kw):
    from lgn.step import NativeTrainStep
    kw = dict(dict(batch_size=B, l1_lambda=0.0, optimizer=False, use_graph=False), **kw)
    return NativeTrainStep(enc, dec, loss_choice=_module(loss), native_emd=True, **kw)


def _module_step(enc, dec, loss, **kw):
    from lgn.step import TrainStep
    return TrainStep(enc, dec, l1_lambda=0.0, optimizer=False, loss_choice=_module(loss), **kw)


def _grads(enc, dec):
    return {n: (None if g is None else g.detach().clone()) for n, g in U.named_grads(enc, dec)}


def _assert_nondegenerate(x, t, opts, what):
    """Decided on the CPU from the module-API step's x = get_real(reconstruction): every jet's optimum is non-degenerate both ways --
    the arcs among weighted particles whose reduced cost c_ij - u_i - v_j is below 1e-6 x the largest cost number exactly (weighted
    rows + weighted columns - 1), and every one of them carries flow above 1e-9 x the total weight.  Then the optimal basis, and with
    it the closed-form gradient, is the same for every reconstruction within 1e-10 of x."""
    p, q = E.relative_events(x.detach().cpu().numpy()), E.relative_events(t.detach().cpu().numpy())
    for b in range(len(p)):
        _, flow, u, v = GO.solve(p[b], q[b], **opts)
        c, a, d = P.balanced(p[b], q[b], opts.get("R", 1.0), opts.get("beta", 1.0), opts.get("norm", False),
                             opts.get("periodic_phi", False))
        ri, ci = np.flatnonzero(a > 0), np.flatnonzero(d > 0)
        sel = np.ix_(ri, ci)
        tight = (c - u[:, None] - v[None, :])[sel] < 1e-6 * c[sel].max()
        assert tight.sum() == len(ri) + len(ci) - 1, f"{what}: jet {b}: {tight.sum()} tight arcs, basis {len(ri) + len(ci) - 1}"
        assert (flow[sel][tight] > 1e-9 * max(a.sum(), d.sum())).all(), f"{what}: jet {b}: a basic arc without flow"


def _compare_with_module_step(N, loss, maxdim=2, method="sum", what=""):
    """NativeTrainStep(native_emd=True) against TrainStep with the same module on equal weights: loss and reconstruction to 1e-10,
    every gradient tensor to 1e-9 (the tolerances of the project's native-vs-module tests).  Returns the native step."""
    from lgn.step import get_real
    (ea, da, _, _), (eb, db, _, _) = _nets(N, 2, maxdim)
    batch = _batch(N)
    ref = _module_step(eb, db, loss, get_real_method=method)
    loss_m, rec_m = ref.step(batch)
    emd_opts = loss[1] if loss[0] == "emd" else loss[2]
    _assert_nondegenerate(get_real(rec_m.detach(), method), batch["p4"], emd_opts, what)
    nat = _native(ea, da, loss, get_real_method=method)
    loss_n, rec_n = nat.step(batch)
    torch.cuda.synchronize()
    assert int(nat.status.abs().max()) == 0 and int(ref.loss_fn.status.abs().max()) == 0
    print(f"{what}: loss native {float(loss_n):.15e}, module {float(loss_m):.15e}")
    U.assert_close(loss_n, loss_m, 1e-10, f"{what}: loss")
    U.assert_close(rec_n, rec_m, 1e-10, f"{what}: reconstruction")
    worst = U.assert_named_grads_close(U.named_grads(ea, da), _grads(eb, db), 1e-9, what)
    print(f"{what}: worst gradient tensor {worst}")
    return nat


# ---- 1. the value is the score, bit for bit ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("N", [6, 30, 63, 64])       # 63: the last shape with one solver column per lane (64 nodes), 64: the first with two
@pytest.mark.parametrize("opt", list(OPTS))
def test_the_value_is_the_score_bit_for_bit(opt, N):
    from lgn import emd as M
    from lgn.step import NativeEvalStep, NativeTrainStep
    loss = ("emd", OPTS[opt])
    batch = _batch(N)
    for method in ("real", "sum"):
        (ea, da, _, _), (ec, dc, _, _) = _nets(N, 2)
        train = _native(ea, da, loss, get_real_method=method)
        _, rec_t = train.step(batch)
        ev = NativeEvalStep(ea, da, batch_size=B, get_real_method=method, use_graph=False, loss_choice=_module(loss), native_emd=True)
        out = ev.run(batch)
        score, status = M.emd_relative_tensor(out["recon"], batch["p4"], return_status=True, **OPTS[opt])
        torch.cuda.synchronize()
        assert torch.isfinite(ev.loss_part).all() and int(status.abs().max()) == 0
        assert torch.equal(ev.loss_part, score), (opt, N, method, (ev.loss_part - score).abs().max().item())
        assert torch.equal(ev.status, status) and ev.status is ev.inputs.status
        U.assert_close(out["loss"], score.sum(), 1e-14, "the evaluation loss is the sum of the scores")
        # the training step: the same per-jet bits and flags
        assert torch.equal(train.loss_part, ev.loss_part) and torch.equal(train.status, ev.status), (opt, N, method)
        # ... and the Chamfer step's reconstruction
        chamfer = NativeTrainStep(ec, dc, batch_size=B, l1_lambda=0.0, optimizer=False, use_graph=False, get_real_method=method)
        _, rec_c = chamfer.step(batch)
        torch.cuda.synchronize()
        assert torch.equal(rec_t, rec_c), (opt, N, method)


# ---- 2. gradients against the module-API step -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("opt,N,maxdim", [("default", 6, 2), ("beta2", 6, 2), ("all", 6, 2), ("default", 30, 2), ("default", 64, 2),
                                          ("default", 6, 3)])
def test_gradients_against_the_module_step(opt, N, maxdim):
    nat = _compare_with_module_step(N, ("emd", OPTS[opt]), maxdim, what=f"emd {opt} N={N} maxdim={maxdim}")
    assert nat.loss_kind == nat.N.LOSS_EMD and nat.loss_desc.chamfer_weight == 0.0


# ---- 3. against the oracle ------------------------------------------------------------------------------------------------------------

class _RefEMD(torch.autograd.Function):
    """the restatement's EMD of (x, target) per jet, with its closed-form gradient"""

    @staticmethod
    def forward(ctx, x, t, opts):
        with torch.enable_grad():       # (the restatement carries the frame gradient back with autograd of its own)
            val, gr, _ = GO.emd_relative_grad(x.detach().numpy(), t.detach().numpy(), **dict(opts))
        ctx.save_for_backward(torch.from_numpy(gr))
        return torch.from_numpy(val)

    @staticmethod
    def backward(ctx, g):
        (gr,) = ctx.saved_tensors
        return gr * g.reshape(-1, 1, 1), None, None


@pytest.mark.parametrize("opt", ["default", "beta2"])
def test_against_the_oracle(opt):
    """The oracle networks on the CPU with the restatement's EMD as their loss.  No tolerance is fixed: the parent's route -- TrainStep
    with the module -- is compared with the same oracle, and the native step may show at most 10 x that discrepancy per tensor
    (floor 1e-12), relative to the tensor's own largest entry."""
    from oracle import lgn_oracle as O
    N = 6
    loss = ("emd", OPTS[opt])
    (ea, da, Pe, Pd), (eb, db, _, _) = _nets(N, 2)
    batch = _batch(N)
    p4 = batch["p4"].cpu()
    cfg = [O.NetConfig(num_particles=N, maxdim=2, num_channels=c) for c in CH]
    frozen = tuple(sorted(OPTS[opt].items()))
    loss_o, rec_o, grads_o = U.oracle_step(O, Pe, Pd, cfg[0], cfg[1], p4, batch["labels"].cpu(), get_real="sum",
                                           loss_fn=lambda x, t: _RefEMD.apply(x, t, frozen))
    got = {}
    for name, (enc, dec, make) in {"module": (eb, db, _module_step), "native": (ea, da, _native)}.items():
        step = make(enc, dec, loss)
        l, rec = step.step(batch)
        torch.cuda.synchronize()
        got[name] = (float(l), rec.detach().cpu(), _grads(enc, dec))

    def rel(a, b):
        return float((a.cpu() - b).abs().max() / b.abs().max())

    for what, pick in (("loss", lambda r: torch.tensor([r[0]])), ("reconstruction", lambda r: r[1])):
        ref = pick((float(loss_o), rec_o, None))
        dm, dn = rel(pick(got["module"]), ref), rel(pick(got["native"]), ref)
        print(f"{opt} {what}: module vs oracle {dm:.3e}, native vs oracle {dn:.3e}")
        assert dn <= max(10 * dm, 1e-12), what
    checked = 0
    for name, g in grads_o.items():
        if g is None or float(g.abs().max()) == 0:
            continue
        dm, dn = rel(got["module"][2][name], g), rel(got["native"][2][name], g)
        print(f"{opt} grad {name}: module vs oracle {dm:.3e}, native vs oracle {dn:.3e}")
        assert dn <= max(10 * dm, 1e-12), name
        checked += 1
    assert checked >= 10


# ---- 4. hybrid --------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("N", [6, 30])
@pytest.mark.parametrize("weight,opts", [(0.5, {}), (2.0, dict(beta=2.0))])
def test_the_hybrid_loss_against_the_module_step(weight, opts, N):
    nat = _compare_with_module_step(N, ("hybrid", weight, opts), what=f"hybrid {weight} {opts} N={N}")
    assert nat.loss_desc.chamfer_weight == weight


def test_a_hybrid_loss_without_chamfer_weight_is_the_emd_step():
    (ea, da, _, _), (eb, db, _, _) = _nets(6, 2)
    batch = _batch(6)
    a, b = _native(ea, da, ("hybrid", 0.0, {})), _native(eb, db, ("emd", {}))
    la, ra = a.step(batch)
    lb, rb = b.step(batch)
    torch.cuda.synchronize()
    assert torch.equal(a.loss_part, b.loss_part) and torch.equal(la, lb) and torch.equal(ra, rb)
    assert torch.equal(a.flat.grad, b.flat.grad) and float(a.flat.grad.abs().max()) > 0


def test_the_hybrid_evaluation_step():
    from lgn import emd as M
    from lgn.losses import ChamferLoss
    from lgn.step import NativeEvalStep
    for N in (6, 64):               # (the Chamfer loss rides on the decoder's last level up to 40 particles, and is a launch of its own above)
        ((enc, dec, _, _),) = _nets(N, 1)
        batch = _batch(N)
        ev = NativeEvalStep(enc, dec, batch_size=B, use_graph=False, loss_choice=_module(("hybrid", 0.5, dict(beta=2.0))), native_emd=True)
        out = ev.run(batch)
        score = M.emd_relative_tensor(out["recon"], batch["p4"], beta=2.0)
        chamfer = torch.stack([ChamferLoss()(out["recon"][b:b + 1], batch["p4"][b:b + 1]) for b in range(B)])
        U.assert_close(ev.loss_part, 0.5 * chamfer + score, 1e-13, f"N={N}: per-jet hybrid terms")
        U.assert_close(out["loss"], (0.5 * chamfer + score).sum(), 1e-13, f"N={N}: hybrid evaluation loss")


# ---- 5. whole step and plumbing ---------------------------------------------------------------------------------------------------------

def test_graph_eager_and_the_two_call_form_give_equal_bits():
    loss = ("emd", dict(beta=2.0))
    (ea, da, _, _), (eb, db, _, _), (ec, dc, _, _) = _nets(6, 3)
    batch = _batch(6)
    kw = dict(l1_lambda=1e-8, optimizer=True, lr=1e-3)
    eager, graph, two = _native(ea, da, loss, **kw), _native(eb, db, loss, use_graph=True, **kw), _native(ec, dc, loss, **kw)
    before = eager.flat.flat.clone()
    for _ in range(2):
        le, re_ = eager.step(batch)
        lg, rg = graph.step(batch)
        two.load_batch(batch)       # the two-call form: lgn_step_fwd_bwd_f64, then the finalize call
        two._fwd_bwd()
        two._finalize(True)
    torch.cuda.synchronize()
    assert graph.launches_per_step == 1
    assert not torch.equal(eager.flat.flat, before)
    for other, what in ((graph, "graph"), (two, "two-call")):
        assert torch.equal(other.flat.flat, eager.flat.flat), what
        assert torch.equal(other.loss_part, eager.loss_part) and torch.equal(other.loss_out[:3], eager.loss_out[:3]), what
        assert torch.equal(other.recon, eager.recon) and torch.equal(other.status, eager.status), what


def test_one_adam_step_against_the_captured_module_step():
    from lgn.step import CapturedModuleStep, NativeTrainStep, native_train_step
    loss = ("hybrid", 0.5, dict(norm=True))
    (ea, da, _, _), (eb, db, _, _) = _nets(6, 2)
    batch = _batch(6)
    mod_n = _module(loss)
    nat = native_train_step(ea, da, B, lr=1e-3, l1_lambda=1e-8, loss_choice=mod_n, native_emd=True)
    assert isinstance(nat, NativeTrainStep)
    ref = CapturedModuleStep(eb, db, batch_size=B, lr=1e-3, l1_lambda=1e-8, use_graph=True, loss_choice=_module(loss))
    assert torch.equal(nat.flat.flat, ref.flat.flat)
    ln, rn = nat.step(batch)
    lr_, rr = ref.step(batch)
    torch.cuda.synchronize()
    assert mod_n.status is nat.status and int(nat.status.abs().max()) == 0
    U.assert_close(ln, lr_, 1e-10, "loss")
    U.assert_close(rn, rr, 1e-10, "reconstruction")
    U.assert_close(nat.flat.flat, ref.flat.flat, 1e-9, "parameters after one Adam step")


def test_an_epoch_reproduces_three_steps():
    from lgn.epoch import DeviceDataset, EpochRunner
    loss = ("emd", {})
    (ea, da, _, _), (eb, db, _, _) = _nets(6, 2)
    data = _batch(6, seed=300, n_jets=3 * B)
    kw = dict(l1_lambda=1e-8, optimizer=True, lr=1e-3, use_graph=True)
    a, b = _native(ea, da, loss, **kw), _native(eb, db, loss, **kw)
    runner = EpochRunner(a, DeviceDataset(data, shuffle=False), shuffle=False)
    res = runner.run_epoch()
    losses = [b.step({k: v[i * B:(i + 1) * B] for k, v in data.items()})[0].item() for i in range(3)]
    torch.cuda.synchronize()
    print(f"epoch loss sum {res['loss_sum']!r}, three steps {losses!r} = {sum(losses)!r}")
    assert res["steps"] == 3 and res["status"] == 0
    assert torch.equal(a.flat.flat, b.flat.flat) and torch.equal(a.loss_part, b.loss_part)
    assert res["loss_sum"] == sum(losses)


# ---- 6. flags -----------------------------------------------------------------------------------------------------------------------

def test_an_all_padded_jet_under_norm_is_flagged_and_hands_on_nothing():
    from lgn import _native as Nat
    loss = ("emd", dict(norm=True))
    (ea, da, _, _), (eb, db, _, _), (ec, dc, _, _) = _nets(6, 3)
    clean = _batch(6)
    bad = 2
    holed = {k: v.clone() for k, v in clean.items()}
    holed["p4"][bad] = 0.0
    holed["labels"][bad] = 0
    rest = {k: torch.cat((v[:bad], v[bad + 1:])) for k, v in clean.items()}
    nat = _native(ea, da, loss)
    nat.step(holed)
    torch.cuda.synchronize()
    status = nat.status.cpu()
    assert int(status[bad]) == Nat.EMD_EMPTY and int(status.abs().sum()) == Nat.EMD_EMPTY
    assert bool(torch.isnan(nat.loss_part[bad])) and bool(torch.isfinite(torch.cat((nat.loss_part[:bad], nat.loss_part[bad + 1:]))).all())
    assert bool(torch.isfinite(nat.flat.grad).all())
    # the loss is a sum over the jets: the module-API step on the batch without that jet
    ref = _module_step(eb, db, loss)
    ref.step(rest)
    torch.cuda.synchronize()
    U.assert_named_grads_close(U.named_grads(ea, da), _grads(eb, db), 1e-9, "the other jets' gradients")
    # the next clean step is unaffected
    fresh = _native(ec, dc, loss)
    l1, r1 = nat.step(clean)
    l2, r2 = fresh.step(clean)
    torch.cuda.synchronize()
    assert int(nat.status.abs().max()) == 0
    assert torch.equal(l1, l2) and torch.equal(r1, r2) and torch.equal(nat.flat.grad, fresh.flat.grad)
    assert torch.equal(nat.loss_part, fresh.loss_part)


@pytest.mark.parametrize("use_graph", [False, True])
def test_a_short_evaluation_batch_gives_the_loss_of_its_real_jets(use_graph):
    from lgn import _native as Nat
    from lgn import emd as M
    from lgn.step import NativeEvalStep
    ((enc, dec, _, _),) = _nets(6, 1)
    batch = {k: v[:B - 1] for k, v in _batch(6).items()}
    ev = NativeEvalStep(enc, dec, batch_size=B, use_graph=use_graph, loss_choice=_module(("emd", dict(norm=True))), native_emd=True)
    out = ev.run(batch)
    score = M.emd_relative_tensor(out["recon"], batch["p4"], norm=True)
    torch.cuda.synchronize()
    assert out["recon"].shape[0] == B - 1 and bool(torch.isfinite(out["loss"]))
    assert torch.equal(ev.loss_part[:B - 1], score)
    U.assert_close(out["loss"], score.sum(), 1e-14, "the loss of the real jets")
    assert int(ev.status[B - 1]) == Nat.EMD_EMPTY and bool(torch.isnan(ev.loss_part[B - 1])) and int(ev.status[:B - 1].abs().max()) == 0


# ---- 7. refusal ---------------------------------------------------------------------------------------------------------------------

def test_a_decoder_that_does_not_fit_is_refused_at_plan_time():
    import __graft_entry__ as GE
    from lgn import _native as Nat
    from lgn.losses import EMDLoss
    from lgn.step import CapturedModuleStep, NativeEvalStep, NativeTrainStep, native_train_step
    enc, dec = GE._models(150, (2, 2, 4), (4, 2, 4), torch.device(DEV), seed=23)
    assert dec.num_channels[-1] == 4 and Nat.lib().lgn_emd_loss_lds_bytes(150, 4) > Nat.LDS_LIMIT
    for cls in (NativeTrainStep, NativeEvalStep):
        with pytest.raises(NotImplementedError, match=rf"lgn_emd_loss_lds_bytes.*{Nat.LDS_LIMIT}"):
            cls(enc, dec, batch_size=2, loss_choice=EMDLoss(), native_emd=True)
    step = native_train_step(enc, dec, 2, loss_choice=EMDLoss(), native_emd=True)
    assert isinstance(step, CapturedModuleStep)


def test_the_native_call_refuses_bad_descriptors_before_any_launch():
    from lgn.step import NativeEvalStep
    ((enc, dec, _, _),) = _nets(6, 1)
    ev = NativeEvalStep(enc, dec, batch_size=B, use_graph=False, loss_choice=_module(("emd", {})), native_emd=True)
    ev.load_batch(_batch(6))
    ev.loss_part.fill_(-7.0)
    good = type(ev.loss_desc).from_buffer_copy(ev.loss_desc)

    def refused(words, **change):
        d = type(good).from_buffer_copy(good)
        for k, v in change.items():
            obj, _, field = k.rpartition("__")
            setattr(getattr(d, obj) if obj else d, field, v)
        with pytest.raises(RuntimeError, match=words):
            ev._eval(None, d)

    refused("R = ", opts__R=0.0)
    refused("R = ", opts__R=float("inf"))
    refused("beta = ", opts__beta=-1.0)
    refused("beta = ", opts__beta=float("nan"))
    refused("chamfer_weight", chamfer_weight=-0.5)
    refused("chamfer_weight", chamfer_weight=float("inf"))
    refused("scale", base__scale=0.0)
    refused("scale", base__scale=float("nan"))
    d = type(ev.desc).from_buffer_copy(ev.desc)
    d.jet_loss_scale = 0.25
    with pytest.raises(RuntimeError, match="jet_loss_scale"):
        ev._eval(d)
    torch.cuda.synchronize()
    assert bool((ev.loss_part == -7.0).all()), "a refused call launched something"
    ev._eval()
    torch.cuda.synchronize()
    assert bool(torch.isfinite(ev.loss_part).all())
