"""GPU tests of the split form of the whole-step calls on table-driven (maxdim 3) networks (``table_split=True``): jet_features gives
the encoder one node more than the decoder reconstructs, data['scalars'] more input scalars per node; each network then runs on its
own node count -- its own tile count, and its own choice between the static and the run-time-table kernels.

Against the oracle at live weights (FWD_TOL / GRAD_TOL of test_gpu_step_oracle.py, per gradient tensor, the graph replay): CASES
below, the smallest shape that enters each regime.  sigma and wseed of U.live_weights were chosen on the CPU so that U.assert_live
holds on the oracle's outputs alone; measured there (sigma: max |recon|; live gradient tensors under 1e-4 of the largest, of 65 --
112 in the wide network):

    jet_b3_n12   0.03: 1.7e-2; 2     jet_b9_n7    0.05: 1.4e-2; 1     K3  0.13: 1.1e-2; 0     K8  0.1: 4.8e-3; 2
    jet_b2_n31   0.1:  3.2e-1; 2     jet_b2_n32   0.1:  1.7e+1; 3     jet_b2_n33  0.1: 2.3e+1; 2     jet_K4_wide  0.1: 3.5e-1; 0

The second row runs with the encoder's ``scale`` = 0.1 (--scale, lgn_encoder.py:376).  The jet node carries the sum of 31 and more
momenta (and the wide network seven and eight channels of it), and at scale 1 no sigma between 0.007 and 0.16 with any of five seeds
is live: from 0.02 down 10 .. 25 of the 65 tensors (the CGMLP biases, the (0, 2) / (2, 0) mixing weights) fall under 1e-4 of the
largest, from 0.02 up the reconstruction passes 1e3 and reaches 1e28.  The target stays the unscaled batch.

Against the module route (TrainStep / CapturedModuleStep / ReferenceLoopStep / ModuleEvalStep on equal weights) and against itself
(graph, eager and two-call forms, an EpochRunner epoch) on the same shapes."""
import functools

import pytest
import torch

import _util as U
from test_gpu_step_options_oracle import Net, _batch, _forward, _nets, _to_dev
from test_gpu_step_oracle import FWD_TOL, GRAD_TOL

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SMALL = ((2, 3, 4), (4, 3, 2))
MID = ((3, 4, 4), (4, 4, 3))
WIDE = ((2, 4, 7, 8), (8, 6, 5, 3))

# tau_input_scalars is the constructor's: jet_features adds the jet-mass scalar (and the jet node) by itself
CASES = {
    "jet_b3_n12": Net(3, 12, 3, chans=SMALL, jet_features=True, sigma=0.03),      # smallest: 39 encoder nodes, 36 decoder nodes
    "jet_b9_n7": Net(3, 7, 9, chans=SMALL, jet_features=True, sigma=0.05),        # 72 encoder nodes (two tiles), 63 decoder nodes (one)
    "jet_b2_n31": Net(3, 31, 2, chans=MID, jet_features=True, scale=0.1),        # encoder at 32 nodes: the last N of the static kernels
    "jet_b2_n32": Net(3, 32, 2, chans=MID, jet_features=True, scale=0.1),        # encoder at 33: run-time tables; decoder static, separable
    "jet_b2_n33": Net(3, 33, 2, chans=MID, jet_features=True, scale=0.1),        # both on run-time tables
    "jet_K4_wide": Net(3, 13, 4, chans=WIDE, jet_features=True, tau_input_scalars=3, scale=0.1),      # K = 4, both table kinds
    "K3": Net(3, 12, 3, chans=SMALL, tau_input_scalars=3, sigma=0.13),                        # one node count: split by K alone
    "K8": Net(3, 12, 3, chans=SMALL, tau_input_scalars=8),
}
MODULE_CASES = ["jet_b3_n12", "jet_b9_n7", "jet_b2_n32", "jet_K4_wide", "K3"]


def _K(net):
    return net.tau_input_scalars + int(net.jet_features)


def _native(net, enc, dec, **kw):
    from lgn.step import NativeTrainStep
    step = NativeTrainStep(enc, dec, batch_size=net.B, table_split=True, **kw)
    assert step.split and step.desc.N == net.N + int(net.jet_features) and step.desc.dec_N == net.N and step.desc.n_in_scalars == _K(net)
    assert bool(step.desc.enc_tables[0]) and bool(step.desc.dec_tables[0])
    return step


# ---- 1. the oracle --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(CASES))
def test_split_step_matches_oracle(case):
    """The graph-replayed whole-step call the chooser takes with table_split: total loss, Chamfer part, reconstruction and every
    named gradient (+ the L1 sub-gradient) against the oracle; U.assert_live on the oracle's outputs decides the inputs first."""
    from lgn.step import NativeTrainStep, native_train_step
    from oracle import lgn_oracle as O
    net = CASES[case]
    F = _forward(net)
    enc, dec, _, _ = _nets(net, DEV)
    lam = 1e-8
    step = native_train_step(enc, dec, net.B, extra_scalars=net.tau_input_scalars - 1, l1_lambda=lam, optimizer=False, use_graph=True,
                             table_split=True)
    assert isinstance(step, NativeTrainStep) and step.split, "the chooser must take the whole-step call with table_split"
    batch = _to_dev(_batch(net)[0])
    first = None
    for it in range(3):                      # capture + replay, then replays on the same buffers
        total, recon = step.step(batch)
        if first is None:
            first = (total.clone(), recon.clone(), step.flat.grad.clone())
    torch.cuda.synchronize()
    assert step.launches_per_step == 1
    assert torch.equal(total, first[0]) and torch.equal(recon, first[1]) and torch.equal(step.flat.grad, first[2]), "replays differ"
    x_o = O.get_real(F.rec.detach(), "sum")
    chamfer_o = U.oracle_loss(O, F.Pe, F.Pd, F.rec, F.target)
    grads_o = U.oracle_backward(chamfer_o, F.Pe, F.Pd, retain_graph=True)
    floor = U.assert_live(O, F.rec.detach(), grads_o, F.target, x_o, pooled=F.pooled, latent_map=net.latent)
    chamfer_o, rec_o = chamfer_o.detach(), F.rec.detach()
    l1_o = O.l1_norm(F.Pe).detach() + O.l1_norm(F.Pd).detach()
    errs = {"recon": U.relerr(recon.cpu(), rec_o), "chamfer": U.relerr(step.loss_out[1].cpu(), chamfer_o),
            "loss": U.relerr(total.cpu(), chamfer_o + lam * l1_o)}
    print(f"[{case}] recon abs max {float(rec_o.abs().max()):.3e}, floor tensors {floor}, rel errs "
          + ", ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    U.assert_close(total, chamfer_o + lam * l1_o, FWD_TOL, "total loss")
    U.assert_close(step.loss_out[1], chamfer_o, FWD_TOL, "chamfer")
    U.assert_close(recon, rec_o, FWD_TOL, "recon")
    l1 = {f"{pre}.{k}": lam * torch.sign(v.detach()) for pre, P in (("enc", F.Pe), ("dec", F.Pd)) for k, v in P.items()}
    worst, name = U.assert_named_grads_close(U.named_grads(enc, dec), grads_o, GRAD_TOL, case, add=l1, max_floor_routed=floor)
    print(f"[{case}] worst gradient tensor: {name}: rel err {worst:.2e}")


# ---- 2. the module route --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", MODULE_CASES)
def test_split_step_matches_module_path(case):
    """Against the module / autograd path (per-network native calls) on the same weights: 1e-12 / 1e-9, as the maxdim-2 split form."""
    from lgn.step import TrainStep
    net = CASES[case]
    enc, dec, _, _ = _nets(net, DEV)
    enc2, dec2, _, _ = _nets(net, DEV)
    batch = _to_dev(_batch(net)[0])
    a = _native(net, enc, dec, optimizer=False, use_graph=True)
    b = TrainStep(enc2, dec2, optimizer=False)
    for _ in range(2):
        la, ra = a.step(batch)
    lb, rb = b.forward_backward(batch)
    print(f"[{case}] loss {float(la):.15e} / {float(lb):.15e}: rel err {U.relerr(la.cpu(), lb.cpu()):.2e}, recon {U.relerr(ra.cpu(), rb.cpu()):.2e}")
    U.assert_close(la, lb, 1e-12, "loss")
    U.assert_close(ra, rb, 1e-12, "recon")
    U.assert_named_grads_close(U.named_grads(enc, dec), dict(U.named_grads(enc2, dec2)), 1e-9, case)
    assert torch.isfinite(a.flat.grad).all()


@pytest.mark.parametrize("case", ["jet_b3_n12", "jet_b2_n32", "jet_K4_wide"])
def test_eval_step_matches_module_eval_step_and_oracle(case):
    """NativeEvalStep(table_split, keep_latent): loss, get_real(reconstruction) and the pooled latent against ModuleEvalStep (1e-12)
    and the oracle (FWD_TOL), replayed; then a short last batch against ModuleEvalStep on the same jets."""
    from lgn.step import ModuleEvalStep, NativeEvalStep
    from oracle import lgn_oracle as O
    net = CASES[case]
    F = _forward(net)
    enc, dec, _, _ = _nets(net, DEV)
    ev = NativeEvalStep(enc, dec, net.B, get_real_method="real", keep_latent=True, use_graph=True, table_split=True)
    assert ev.split
    mod = ModuleEvalStep(enc, dec, net.B, get_real_method="real", keep_latent=True)
    batch = _to_dev(_batch(net)[0])
    for _ in range(2):
        out = ev.run(batch)
    ref = mod.run(batch)
    torch.cuda.synchronize()
    x_o = O.get_real(F.rec.detach(), "real")
    with torch.no_grad():
        loss_o = U.oracle_loss(O, F.Pe, F.Pd, F.rec.detach(), F.target, get_real="real")
    U.assert_live(O, F.rec.detach(), None, F.target, x_o, pooled=F.pooled, latent_map=net.latent)
    errs = {"loss": U.relerr(out["loss"].cpu(), loss_o), "recon": U.relerr(out["recon"].cpu(), x_o)}
    errs.update({f"latent {k}": U.relerr(out["latent"][k].cpu(), F.latent[k]) for k in F.latent})
    print(f"[eval {case}] rel errs " + ", ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    U.assert_close(out["loss"], loss_o, FWD_TOL, "loss against the oracle")
    U.assert_close(out["recon"], x_o, FWD_TOL, "recon against the oracle")
    U.assert_close(out["loss"], ref["loss"], 1e-12, "loss against ModuleEvalStep")
    U.assert_close(out["recon"], ref["recon"], 1e-12, "recon against ModuleEvalStep")
    for k in F.latent:
        U.assert_close(out["latent"][k], F.latent[k], FWD_TOL, f"latent {k} against the oracle")
        U.assert_close(out["latent"][k], ref["latent"][k], 1e-12, f"latent {k} against ModuleEvalStep")
    n = net.B - 1
    short = {k: v[:n].contiguous() for k, v in batch.items()}
    out, ref = ev.run(short), mod.run(short)
    assert out["recon"].shape[0] == n and out["latent"][(1, 1)].shape[1] == n
    U.assert_close(out["loss"], ref["loss"], 1e-12, "short batch: loss")
    U.assert_close(out["recon"], ref["recon"], 1e-12, "short batch: recon")
    U.assert_close(out["latent"][(1, 1)], ref["latent"][(1, 1)], 1e-12, "short batch: latent vectors")
    assert bool((ev.p4[n:] == 0).all()) and bool((ev.mask[n:] == 0).all())


# ---- 3. the optimiser tail: graph, eager and two-call forms ----------------------------------------------------------------------
@pytest.mark.parametrize("case", ["jet_b3_n12", "jet_b2_n32"])
def test_three_adam_steps_agree_in_every_form(case):
    """The tail is the code every step runs: three Adam steps replayed from the graph, three eager ones and three in the two-call
    form (lgn_step_fwd_bwd_f64, then the finalize call) leave the same bits -- parameters, both moments, the step counter."""
    net = CASES[case]
    batch = _to_dev(_batch(net)[0])
    steps = []
    for kw in (dict(use_graph=True), dict(use_graph=False), dict(use_graph=False)):
        enc, dec, _, _ = _nets(net, DEV)
        steps.append(_native(net, enc, dec, lr=1e-3, l1_lambda=1e-8, **kw))
    graph, eager, two = steps
    before = eager.flat.flat.clone()
    for _ in range(3):
        graph.step(batch)
        eager.step(batch)
        two.load_batch(batch)
        two._fwd_bwd()
        two._finalize(True)
    torch.cuda.synchronize()
    assert graph.launches_per_step == 1 and not torch.equal(eager.flat.flat, before)
    for other, what in ((graph, "graph"), (two, "two-call")):
        assert torch.equal(other.flat.flat, eager.flat.flat), f"{what}: parameters"
        assert torch.equal(other.adam_m, eager.adam_m) and torch.equal(other.adam_v, eager.adam_v), f"{what}: optimiser state"
        assert torch.equal(other.step_dev, eager.step_dev) and int(other.step_dev.item()) == 3, f"{what}: step counter"
        assert torch.equal(other.recon, eager.recon) and torch.equal(other.loss_out[:3], eager.loss_out[:3]), f"{what}: outputs"


# ---- 4. one case per option, against the module route ------------------------------------------------------------------------------
OPTION_NET = CASES["jet_b3_n12"]


def _pair():
    return [_nets(OPTION_NET, DEV)[:2] for _ in range(2)]


def test_option_get_real_and_jet_feature_term():
    """get_real 'real' + chamfer_jet_features against CapturedModuleStep (lgn.losses.ChamferLoss under autograd): the tolerances of
    test_gpu_step_loss_options.test_split_step_with_jet_loss_matches_captured_module_step."""
    from lgn.step import CapturedModuleStep
    net = OPTION_NET
    (ea, da), (eb, db) = _pair()
    batch = _to_dev(_batch(net)[0])
    kw = dict(l1_lambda=0.0, optimizer=False, get_real_method="real", chamfer_jet_features=True)
    a = _native(net, ea, da, use_graph=True, **kw)
    b = CapturedModuleStep(eb, db, batch_size=net.B, use_graph=False, **kw)
    for _ in range(2):
        la, ra = a.step(batch)
    lb, rb = b.step(batch)
    U.assert_close(la, lb, 1e-11, "loss")
    U.assert_close(ra, rb, 1e-11, "recon")
    U.assert_close(a.flat.grad, b.flat.grad, 1e-9, "flat gradient")


def test_option_hungarian_loss():
    """loss_choice 'hungarian' against CapturedModuleStep: the tolerances of test_gpu_hungarian_loss.test_split_step_matches_captured_module_step."""
    from lgn.step import CapturedModuleStep
    net = OPTION_NET
    (ea, da), (eb, db) = _pair()
    batch = _to_dev(_batch(net)[0])
    kw = dict(l1_lambda=0.0, optimizer=False, get_real_method="real", loss_choice="hungarian", hungarian_abs_coord=True,
              hungarian_polar_coord=False)
    a = _native(net, ea, da, use_graph=True, **kw)
    b = CapturedModuleStep(eb, db, batch_size=net.B, use_graph=False, **kw)
    for _ in range(2):
        a.assignment.fill_(-7)
        la, ra = a.step(batch)
    lb, rb = b.step(batch)
    torch.cuda.synchronize()
    assert int(a.status.abs().max()) == 0 and tuple(a.assignment.shape) == (net.B, net.N) and int(a.assignment.min()) >= 0
    U.assert_close(la, lb, 1e-10, "loss")
    U.assert_close(ra, rb, 1e-10, "recon")
    U.assert_close(a.flat.grad, b.flat.grad, 1e-9, "flat gradient")


def test_option_native_emd_loss():
    """EMDLoss() as the step's loss stage (native_emd) against TrainStep with the same module: the tolerances and the non-degeneracy
    condition on the inputs of test_gpu_emd_step._compare_with_module_step."""
    from lgn.losses import EMDLoss
    from lgn.step import TrainStep, get_real
    from test_gpu_emd_step import _assert_nondegenerate
    net = OPTION_NET
    (ea, da), (eb, db) = _pair()
    batch = _to_dev(_batch(net)[0])
    ref = TrainStep(eb, db, l1_lambda=0.0, optimizer=False, loss_choice=EMDLoss())
    loss_m, rec_m = ref.step(batch)
    _assert_nondegenerate(get_real(rec_m.detach(), "sum"), batch["p4"], {}, "table split EMD")
    grads_m = {n: (None if g is None else g.detach().clone()) for n, g in U.named_grads(eb, db)}
    nat = _native(net, ea, da, l1_lambda=0.0, optimizer=False, use_graph=True, loss_choice=EMDLoss(), native_emd=True)
    for _ in range(2):
        loss_n, rec_n = nat.step(batch)
    torch.cuda.synchronize()
    assert int(nat.status.abs().max()) == 0 and int(ref.loss_fn.status.abs().max()) == 0
    U.assert_close(loss_n, loss_m, 1e-10, "loss")
    U.assert_close(rec_n, rec_m, 1e-10, "reconstruction")
    U.assert_named_grads_close(U.named_grads(ea, da), grads_m, 1e-9, "table split EMD")


def test_option_normalize():
    """normalize=True (jet node and jet-mass scalar from lgn_stage_batch_f64) against ReferenceLoopStep, whose encoder prepares its own
    input from the normalised batch: the tolerances of test_gpu_normalize.test_split_step_with_normalize_matches_the_reference_loop_step."""
    import _normalize_ref as R
    from lgn.step import ReferenceLoopStep
    net = OPTION_NET
    (ea, da), (eb, db) = _pair()
    batch = {"p4": R.jets(net.B, net.N, seed=60, n_real=net.N - net.N // 4).to(DEV)}
    a = _native(net, ea, da, optimizer=False, normalize=True, normalize_method="overall_max")
    b = ReferenceLoopStep(eb, db, optimizer=False, normalize=True, normalize_method="overall_max")
    for _ in range(2):
        la, ra = a.step(batch)
    lb, rb = b.step(batch)
    U.assert_close(la, lb, 1e-12, "loss")
    U.assert_close(ra, rb, 1e-12, "recon")
    U.assert_close(a.flat.grad, torch.cat([eb.flat_params.grad, db.flat_params.grad]), 1e-9, "flat gradient")
    assert torch.equal(a.norm_factor, b.norm_factor)


def test_option_rmsprop_with_l2():
    """optimizer_choice 'rmsprop' with l2_lambda > 0 against ReferenceLoopStep, three steps: the tolerances of
    test_gpu_optimizer_options.test_rmsprop_l2_step_matches_the_reference_loop_on_the_module_api, and like it at the networks'
    initial weights with l1_lambda > 0 (the first RMSprop update is +-lr / sqrt(1 - alpha) whatever |g| is: a gradient that is
    rounding noise on one path and an exact zero on the other would differ by a whole step)."""
    import __graft_entry__ as G
    from lgn.step import ReferenceLoopStep
    net = OPTION_NET
    nets = [G._models(net.N, net.ch[0], net.ch[1], torch.device(DEV), seed=net.seed, maxdim=3, jet_features=True) for _ in range(2)]
    batch = _to_dev(_batch(net)[0])
    opts = dict(optimizer_choice="rmsprop", l2_lambda=1e-6, l1_lambda=1e-6, lr=5e-4)
    a = _native(net, *nets[0], use_graph=True, **opts)
    b = ReferenceLoopStep(*nets[1], **opts)
    for it in range(3):
        lb, _ = b.step(batch)
        la, _ = a.step(batch)
        U.assert_close(la, lb, 1e-10, f"loss at step {it}")
    U.assert_close(torch.cat([nets[1][0].flat_params.detach(), nets[1][1].flat_params.detach()]), a.flat.flat, 1e-9, "parameters after 3 steps")


# ---- 5. a device-resident epoch -----------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _epoch_data(M, N):
    import _normalize_ref as R
    p4 = R.jets(M, N, seed=100 + N, n_real=N - N // 3).contiguous()      # raw jets: the steps normalise them
    g = torch.Generator().manual_seed(200 + N)
    return {"p4": p4.to(DEV), "labels": (p4[..., 0] != 0).to(torch.uint8).to(DEV),
            "scalars": torch.randn(M, N + 1, 1, generator=g, dtype=torch.float64).to(DEV)}


def test_training_epoch_is_the_host_loop():
    """One EpochRunner epoch (M = 10 jets, B = 4, N = 6, jet_features plus one extra scalar from the DeviceDataset, the short batch
    dropped) against the host loop over the same batches: the same kernels on the same inputs in the same order -- torch.equal.
    With normalize, as test_gpu_epoch's second training case: the host loop then stages through lgn_stage_batch_f64, whose outputs
    the epoch's gather kernel reproduces bit for bit.  (Without it the host loop's jet node and jet-mass scalar come from the
    encoder's torch operators, which sum the momenta in another order -- measured here: p4 4.4e-16, in_scalars 1.1e-14 apart, for
    maxdim-2 pairs alike -- so the two would not run on the same inputs.)"""
    import __graft_entry__ as G
    from lgn.epoch import DeviceDataset, EpochRunner
    from lgn.step import NativeTrainStep
    M, B, N = 10, 4, 6
    data = _epoch_data(M, N)
    nets = [G._models(N, SMALL[0], SMALL[1], torch.device(DEV), seed=23, maxdim=3, jet_features=True, tau_input_scalars=2) for _ in range(2)]
    a = NativeTrainStep(*nets[0], batch_size=B, lr=1e-3, use_graph=True, table_split=True, normalize=True)
    b = NativeTrainStep(*nets[1], batch_size=B, lr=1e-3, table_split=True, normalize=True)
    assert a.split and a.desc.n_in_scalars == 3 and bool(a.desc.enc_tables[0])
    runner = EpochRunner(a, DeviceDataset(data, shuffle=False), shuffle=True, generator=torch.Generator().manual_seed(5), remainder="drop")
    out = runner.run_epoch()
    assert out["steps"] == 2 and out["status"] == 0 and runner.single_graph
    index = runner.index.clone()
    assert torch.equal(index.cpu(), torch.randperm(M, generator=torch.Generator().manual_seed(5)).to(torch.int32))
    losses = []
    for i in range(2):
        rows = index[i * B:(i + 1) * B].long()
        loss, _ = b.step({k: v[rows] for k, v in data.items()})
        losses.append(loss.item())
    print(f"epoch loss sum {out['loss_sum']!r}, host loop {sum(losses)!r}")
    assert out["loss_sum"] == sum(losses)
    assert torch.equal(a.in_scalars, b.in_scalars) and torch.equal(a.p4, b.p4) and torch.equal(a.norm_factor, b.norm_factor)
    assert torch.equal(a.flat.flat, b.flat.flat), "parameters"
    assert torch.equal(a.adam_m, b.adam_m) and torch.equal(a.adam_v, b.adam_v), "optimiser state"
    assert torch.equal(a.step_dev, b.step_dev) and int(a.step_dev.item()) == 2


# ---- 6. the choosers ------------------------------------------------------------------------------------------------------------------
def test_choosers_take_the_native_steps_with_the_keyword_only():
    from lgn import step as S
    net = OPTION_NET
    enc, dec, _, _ = _nets(net, DEV)
    assert type(S.native_train_step(enc, dec, net.B, table_split=True)) is S.NativeTrainStep
    assert type(S.native_eval_step(enc, dec, net.B, table_split=True)) is S.NativeEvalStep
    enc, dec, _, _ = _nets(net, DEV)
    assert type(S.native_train_step(enc, dec, net.B)) is S.CapturedModuleStep
    assert type(S.native_train_step(enc, dec, net.B, table_split=False)) is S.CapturedModuleStep
    assert type(S.native_eval_step(enc, dec, net.B)) is S.ModuleEvalStep
    assert type(S.native_eval_step(enc, dec, net.B, table_split=False)) is S.ModuleEvalStep
