"""Every option of the training and evaluation steps at LIVE weights against the oracle, per gradient tensor.

The option tests next to this file build their networks at the reference's initial weights, where the reconstruction is ~1e-9: the
'norm' of get_real is all eps, every Hungarian assignment is as good as any other, every activation sees its linear piece around 0.
Here every case moves the weights with U.live_weights (sigma per net, below), runs ONE option away from the defaults through the
graph-replayed native step (two steps: the second is a replay), and holds loss and reconstruction to FWD_TOL and every gradient
tensor to GRAD_TOL of its own largest entry (U.assert_named_grads_close) against the oracle on the CPU.  U.assert_live decides on the
oracle's outputs alone that the case is live -- reconstruction in 1e-3 .. 1e3, at most 10 % of the gradient tensors under 1e-4 of the
largest (that count is the case's max_floor_routed), no Chamfer partner and no min / max pooling score within 1e-8 of its runner-up.

Nets (G._models seed 21 unless noted, U.live_weights seed 77), sigma, and what the oracle alone gives there (max |recon| of the
default options; gradient tensors under 1e-4 of the largest / tensors with a gradient):

    net / section                          sigma                           max |recon|        under 1e-4 / with a gradient
    md2_n12 (C1, C2, C3, C5, C9)           0.1                             7.2e-3             2 .. 5 / 100 over all loss options
    md2_n50 (C1, C2, C3)                   0.1                             1.1e+1             1 .. 5 / 100
    md3_n12 (C1, C2, C3, C5, C9)           0.1                             1.9e-2             1 .. 4 / 65
    C4 latent maps, maxdim 2 (seed 7)      0.1                             6.1e-2 .. 3.1e-1   2 .. 6 / 100
    C4 latent maps, maxdim 3 (seed 7)      0.1                             1.7e-2 .. 6.5e-1   3 .. 9 / 112
    C5 relu / elu / logsigmoid / atan      0.1                             4.1e-3 .. 7.1e-2   1 .. 6 / 100, 3 .. 4 / 65
    C5 sigmoid md2_n12 | md3_n12           0.1, CGMLP tensors 1.2          3.4e+1 | 5.3e-1    1 / 100 | 2 / 65
    C6 depth 3 | 4 | 5                     0.13 | 0.13 | 0.1               1.2e-1 | 3.9e-2 | 9.1e-3    1 / 76 | 1 / 84 | 2 / 92
    C6 width 4 | 5 | 7                     0.1                             1.3e-2 | 2.4e-2 | 1.4e-2    4 | 5 | 4 / 100
    C6 2 bells | 10 bells | maxdim 3       0.1                             5.7e-1 | 1.6e-1 | 3.9e-3    5 / 100 | 9 / 100 | 3 / 53
    C7 jet_K2 (seed 2, live seed 9)        0.03                            2.7e-2             7 / 100
    C7 K3 | jet_md3                        0.13 | 0.03                     2.7e-2 | 2.4e-3    0 / 100 | 4 / 65
    C8 component_max | overall_max | jet_E 0.1 | 0.1 | 0.16                1.8e-3 | 1.6e-3 | 9.4e-2    1 | 2 | 0 / 100
    C8 md3_n12 overall_max                 0.1                             1.6e-2             2 / 65
    C9 maxdim 2, B 8, N 30 (seed 3)        0.1                             1.6e+2             2 / 100

Sigma matters: with jet_features the reconstruction goes from 7e-4 (sigma 0.02) to 5e10 (0.05); with sigmoid no uniform sigma and none
of 96 seeds brings fewer than 15 of 100 tensors above 1e-4 (six layers of slope <= 1/4), so there the CGMLP tensors alone move by 1.2
(live_weights takes a sigma per name part) -- which also takes the pre-activations off the sigmoid's linear piece.

The oracle's forward is computed once per net (functools.lru_cache) and never modified; every case attaches its own loss to it.

Tolerances measured with the oracle against itself (particles of every jet reversed), held to 100 x that figure: none needed.
Measured on the MI355X: worst gradient tensor of any case here 8.5e-14 (C4, maxdim 3; 5e-14 in another run), worst evaluation loss /
reconstruction / latent 6.4e-15 (the assignment losses included), worst parameter tensor after three optimiser steps 2.0e-11
(RMSprop, maxdim 2, B = 8, N = 30)."""
import dataclasses
import functools

import pytest
import torch

import _hungarian_ref as H
import _normalize_ref as R
import _util as U

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
FWD_TOL = 1e-11
GRAD_TOL = 1e-9
ASSIGN_LOSS_TOL = 1e-10       # mse / hungarian losses: what test_gpu_hungarian_loss.py states (device asinh / atan2 in the polar frames)
METHODS = ["real", "imag", "sum", "mean", "norm"]
CH = {2: ((3, 3, 4, 4), (4, 4, 3, 3)), 3: ((2, 3, 4), (4, 3, 2))}
LATENT_CH = ((2, 3, 3, 4), (4, 3, 3, 2))
CFG2 = CH[2]


@dataclasses.dataclass(frozen=True)
class Net:
    """One configuration: the networks' constructor arguments, the batch, and how far live_weights moves the weights."""
    maxdim: int
    N: int
    B: int
    sigma: float = 0.1
    chans: tuple = None
    seed: int = 21
    wseed: int = 77               # U.live_weights' seed
    latent: str = "min&max"
    activation: str = "leakyrelu"
    jet_features: bool = False
    tau_input_scalars: int = 1
    mlp_depth: int = 6
    mlp_width: int = 6
    num_basis_fn: int = 10
    scale: float = 1.0
    normalize: str = None          # a --normalize-method: the batch is raw jets, normalised per jet by the step

    @property
    def ch(self):
        return self.chans or CH[self.maxdim]

    def but(self, **kw):
        return dataclasses.replace(self, **kw)


# sigma of the cases that are not live at 0.1 (the table at the head of the file)
# sigmoid: six layers of slope <= 1/4 leave 15 .. 35 of 100 tensors under 1e-4 at every uniform sigma; the CGMLP tensors move further
ACT_SIGMA = {"sigmoid": (("", 0.1), ("mlp_levels", 1.2))}
SHAPE_SIGMA = {"depth3": 0.13, "depth4": 0.13}
NORM_SIGMA = {("md2_n12", "jet_E"): 0.16}

SPINE = {"md2_n12": Net(2, 12, 3), "md2_n50": Net(2, 50, 2), "md3_n12": Net(3, 12, 2)}


def _nets(net, dev):
    """(encoder, decoder, CPU state dicts of both) at the net's live weights: the weights are drawn on the CPU, so the networks of a
    test (on the GPU) and those the cached oracle forward was built from hold the same numbers."""
    import __graft_entry__ as G
    enc, dec = G._models(net.N, net.ch[0], net.ch[1], torch.device(dev), seed=net.seed, maxdim=net.maxdim, map_to_latent=net.latent,
                         activation=net.activation, jet_features=net.jet_features, tau_input_scalars=net.tau_input_scalars,
                         mlp_depth=net.mlp_depth, num_basis_fn=net.num_basis_fn, mlp_width=net.mlp_width)
    enc.scale = net.scale
    Pe, Pd = U.live_weights(enc, dec, sigma=net.sigma, seed=net.wseed)
    return enc, dec, Pe, Pd


def _cfgs(net):
    from oracle import lgn_oracle as O
    common = dict(num_particles=net.N, maxdim=net.maxdim, map_to_latent=net.latent, activation=net.activation, mlp_depth=net.mlp_depth,
                  num_basis_fn=net.num_basis_fn, mlp_width=net.mlp_width)
    return (O.NetConfig(num_channels=tuple(net.ch[0]), jet_features=net.jet_features, tau_input_scalars=net.tau_input_scalars,
                        scale=net.scale, **common), O.NetConfig(num_channels=tuple(net.ch[1]), **common))


@functools.lru_cache(maxsize=None)
def _batch(net):
    """({the step's batch, on the CPU}, what the oracle's encoder gets = the loss's target, labels or None, data['scalars'] or None)."""
    from oracle import lgn_oracle as O
    if net.normalize:
        raw = R.jets(net.B, net.N, seed=net.N + net.B, n_real=net.N - net.N // 4)
        return {"p4": raw}, R.normalize_p4(raw, net.normalize)[0], None, None
    p4, labels = O.synthetic_jets(net.B, net.N, seed=net.N + net.B, pad=True)
    batch, scalars = {"p4": p4, "labels": labels}, None
    if net.tau_input_scalars > 1:
        g = torch.Generator().manual_seed(net.B + net.tau_input_scalars)
        scalars = torch.randn(net.B, net.N + int(net.jet_features), net.tau_input_scalars - 1, dtype=torch.float64, generator=g)
        batch["scalars"] = scalars
    return batch, p4, labels, scalars


@dataclasses.dataclass
class Forward:
    Pe: dict
    Pd: dict
    rec: torch.Tensor          # with its graph: every case attaches a loss of its own
    latent: dict
    pooled: dict
    target: torch.Tensor


@functools.lru_cache(maxsize=None)
def _forward(net):
    from oracle import lgn_oracle as O
    _, _, Pe, Pd = _nets(net, "cpu")
    _, p4, labels, scalars = _batch(net)
    rec, lat, pooled = U.oracle_forward(O, Pe, Pd, *_cfgs(net), p4, labels, extra_scalars=scalars)
    return Forward(Pe, Pd, rec, {k: v.detach() for k, v in lat.items()}, pooled, p4)


def _to_dev(batch):
    return {k: v.to(DEV) for k, v in batch.items()}


def _train_case(net, what, step_kw=None, get_real="sum", jet_term=False, loss=None, tol_loss=FWD_TOL, chooser=None):
    """Two graph-replayed steps of the native step on `net` against the oracle with the same options; loss = (choice, abs, polar)
    of an assignment loss, scored on the step's own assignment."""
    from lgn import step as S
    from oracle import lgn_oracle as O
    F = _forward(net)
    enc, dec, _, _ = _nets(net, DEV)
    kw = dict(l1_lambda=0.0, optimizer=False, use_graph=True, get_real_method=get_real, chamfer_jet_features=jet_term)
    kw.update(step_kw or {})
    if net.normalize:
        kw.update(normalize=True, normalize_method=net.normalize)
    if loss is not None:
        kw.update(loss_choice=loss[0], hungarian_abs_coord=loss[1], hungarian_polar_coord=loss[2])
    if chooser is not None:
        step = S.native_train_step(enc, dec, net.B, extra_scalars=net.tau_input_scalars - 1, **kw)
        assert type(step).__name__ == chooser, f"the chooser took {type(step).__name__}"
    else:
        step = S.NativeTrainStep(enc, dec, batch_size=net.B, **kw)
        assert step.split == (net.jet_features or net.tau_input_scalars > 1)
    batch = _to_dev(_batch(net)[0])
    for _ in range(2):
        if loss is not None:
            step.assignment.fill_(-7)             # (a replay that left a stale assignment must not pass)
        got, recon = step.step(batch)
    torch.cuda.synchronize()
    x_o, loss_fn = O.get_real(F.rec.detach(), get_real), None
    if loss is not None:
        from test_gpu_hungarian_loss import _check_optimal
        choice, a, p = loss
        col = step.assignment.cpu().long()
        assert int(step.status.abs().max()) == 0
        if choice == "hungarian":       # optimal on the step's OWN reconstruction (see test_gpu_hungarian_loss.test_native_step_matches_oracle)
            _check_optimal(S.get_real(recon.detach(), get_real).cpu(), F.target, col, a, p, True, what, pool=False,
                           identical=bool(a and not p and get_real == "real"))
            loss_fn = lambda x, t: H.per_jet(x, t, col, a, p)                      # noqa: E731
        else:
            assert bool((col == torch.arange(col.shape[1])).all())
            loss_fn = H.mse_per_jet
    loss_o = U.oracle_loss(O, F.Pe, F.Pd, F.rec, F.target, get_real=get_real, jet_term=jet_term, loss_fn=loss_fn)
    grads_o = U.oracle_backward(loss_o, F.Pe, F.Pd, retain_graph=True)
    floor = U.assert_live(O, F.rec.detach(), grads_o, F.target, x_o, chamfer=loss is None, pooled=F.pooled, latent_map=net.latent)
    errs = {"loss": U.relerr(got.cpu(), loss_o.detach()), "recon": U.relerr(recon.cpu(), F.rec.detach())}
    print(f"[{what}] recon abs max {float(F.rec.detach().abs().max()):.3e}, floor tensors {floor}, rel errs "
          + ", ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    U.assert_close(got, loss_o.detach(), tol_loss, "loss")
    U.assert_close(recon, F.rec.detach(), FWD_TOL, "recon")
    worst, name = U.assert_named_grads_close(U.named_grads(enc, dec), grads_o, GRAD_TOL, what, max_floor_routed=floor)
    print(f"[{what}] worst gradient tensor: {name}: rel err {worst:.2e}")
    return step


# ---- C1: get_real and the jet-feature term ------------------------------------------------------------------------------------
@pytest.mark.parametrize("net", list(SPINE))
@pytest.mark.parametrize("jet", [False, True], ids=["nojet", "jet"])
@pytest.mark.parametrize("method", METHODS)
def test_get_real_and_jet_term(method, jet, net):
    _train_case(SPINE[net], f"{net} get_real {method} jet {jet}", get_real=method, jet_term=jet)


# ---- C2: assignment losses ----------------------------------------------------------------------------------------------------
LOSSES = [("mse", True, False)] + [("hungarian",) + H.FRAMES[f] for f in H.FRAMES]
LOSS_IDS = ["mse"] + list(H.FRAMES)


@pytest.mark.parametrize("net", list(SPINE))
@pytest.mark.parametrize("method", ["real", "norm"])
@pytest.mark.parametrize("loss", LOSSES, ids=LOSS_IDS)
def test_assignment_losses(loss, method, net):
    _train_case(SPINE[net], f"{net} {loss[0]} abs {loss[1]} polar {loss[2]} get_real {method}", get_real=method, loss=loss,
                tol_loss=ASSIGN_LOSS_TOL)


# ---- C3: the evaluation step ---------------------------------------------------------------------------------------------------
EVAL_CASES = [(m, j, None) for m in ("real", "norm") for j in (False, True)] + \
             [("real", False, LOSSES[0]), ("real", False, ("hungarian",) + H.FRAMES["abs_cart"]), ("real", False, ("hungarian",) + H.FRAMES["rel_polar"])]
EVAL_IDS = ["real", "real-jet", "norm", "norm-jet", "mse", "abs_cart", "rel_polar"]


@pytest.mark.parametrize("net", list(SPINE))
@pytest.mark.parametrize("method,jet,loss", EVAL_CASES, ids=EVAL_IDS)
def test_eval_step_with_latent(method, jet, loss, net):
    """NativeEvalStep(keep_latent=True): loss, get_real(reconstruction) and the pooled latent against the oracle at FWD_TOL (the
    assignment losses scored on the step's own assignment)."""
    from lgn.step import NativeEvalStep
    from oracle import lgn_oracle as O
    from test_gpu_hungarian_loss import _check_optimal
    net, what = SPINE[net], f"eval {net} {method} jet {jet} loss {loss}"
    F = _forward(net)
    enc, dec, _, _ = _nets(net, DEV)
    kw = {} if loss is None else dict(loss_choice=loss[0], hungarian_abs_coord=loss[1], hungarian_polar_coord=loss[2])
    ev = NativeEvalStep(enc, dec, net.B, get_real_method=method, chamfer_jet_features=jet, keep_latent=True, use_graph=True, **kw)
    batch = _to_dev(_batch(net)[0])
    for _ in range(2):
        if loss is not None:
            ev.assignment.fill_(-7)
        out = ev.run(batch)
    torch.cuda.synchronize()
    x_o, loss_fn = O.get_real(F.rec.detach(), method), None
    if loss is not None:
        choice, a, p = loss
        col = ev.assignment.cpu().long()
        assert int(ev.status.abs().max()) == 0
        if choice == "hungarian":
            _check_optimal(out["recon"].cpu(), F.target, col, a, p, True, what, pool=False, identical=bool(a and not p))
            loss_fn = lambda x, t: H.per_jet(x, t, col, a, p)                      # noqa: E731
        else:
            loss_fn = H.mse_per_jet
    with torch.no_grad():
        loss_o = U.oracle_loss(O, F.Pe, F.Pd, F.rec.detach(), F.target, get_real=method, jet_term=jet, loss_fn=loss_fn)
    U.assert_live(O, F.rec.detach(), None, F.target, x_o, chamfer=loss is None, pooled=F.pooled, latent_map=net.latent)
    errs = {"loss": U.relerr(out["loss"].cpu(), loss_o), "recon": U.relerr(out["recon"].cpu(), x_o)}
    errs.update({f"latent {k}": U.relerr(out["latent"][k].cpu(), F.latent[k]) for k in F.latent})
    print(f"[{what}] rel errs " + ", ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    U.assert_close(out["loss"], loss_o, FWD_TOL, "loss")
    U.assert_close(out["recon"], x_o, FWD_TOL, "recon")
    for k in F.latent:
        U.assert_close(out["latent"][k], F.latent[k], FWD_TOL, f"latent {k}")


# ---- C4: latent maps -----------------------------------------------------------------------------------------------------------
LATENT_MAPS = ["mean", "max", "min", "mean&max", "max&min", "min+max", "mean&min&max", "mean+min+max", "Mean&Max&Min&Mean", "mix"]


@pytest.mark.parametrize("maxdim", [2, 3])
@pytest.mark.parametrize("latent", LATENT_MAPS)
def test_latent_maps(latent, maxdim):
    net = Net(maxdim, 12, 5, chans=LATENT_CH, seed=7, latent=latent, sigma=0.1)
    _train_case(net, f"maxdim {maxdim} map_to_latent {latent}")


# ---- C5: activations -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("net", ["md2_n12", "md3_n12"])
@pytest.mark.parametrize("activation", ["leakyrelu", "relu", "elu", "sigmoid", "logsigmoid", "atan"])
def test_activations(activation, net):
    _train_case(SPINE[net].but(activation=activation, sigma=ACT_SIGMA.get(activation, 0.1)), f"{net} activation {activation}")


# ---- C6: CGMLP and radial shapes -----------------------------------------------------------------------------------------------
SHAPES = {"depth3": dict(mlp_depth=3), "depth4": dict(mlp_depth=4), "depth5": dict(mlp_depth=5), "width4": dict(mlp_width=4),
          "width5": dict(mlp_width=5), "width7": dict(mlp_width=7), "bells2": dict(num_basis_fn=1), "bells10": dict(num_basis_fn=5)}


@pytest.mark.parametrize("shape", list(SHAPES))
def test_cgmlp_and_radial_shapes(shape):
    _train_case(SPINE["md2_n12"].but(sigma=SHAPE_SIGMA.get(shape, 0.1), **SHAPES[shape]), f"md2_n12 {shape}")


def test_cgmlp_and_radial_shapes_maxdim3():
    _train_case(SPINE["md3_n12"].but(mlp_depth=3, mlp_width=5, num_basis_fn=5, sigma=SHAPE_SIGMA.get("md3", 0.1)),
                "md3_n12 depth 3 width 5 bells 10")


# ---- C7: input scalars and jet features ----------------------------------------------------------------------------------------
SCALAR_NETS = {"jet_K2": SPINE["md2_n12"].but(jet_features=True, tau_input_scalars=2, sigma=0.03, seed=2, wseed=9),
               "K3": SPINE["md2_n12"].but(tau_input_scalars=3, sigma=0.13),
               "jet_md3": SPINE["md3_n12"].but(jet_features=True, sigma=0.03)}


@pytest.mark.parametrize("case", ["jet_K2", "K3"])
def test_split_step_with_input_scalars(case):
    step = _train_case(SCALAR_NETS[case], f"split step {case}")
    assert step.split


def test_jet_features_maxdim3_through_the_captured_module_step():
    _train_case(SCALAR_NETS["jet_md3"], "maxdim 3 jet_features", chooser="CapturedModuleStep")


# ---- C8: --normalize -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("net,method", [("md2_n12", m) for m in R.METHODS] + [("md3_n12", "overall_max")])
def test_normalize(net, method):
    """Raw jets of very different scales, normalised per jet by the step's staging kernel; the encoder's scale of 0.25 reaches its
    input alone, the loss compares with the normalised, unscaled batch."""
    _train_case(SPINE[net].but(normalize=method, scale=0.25 if net == "md2_n12" else 1.0, sigma=NORM_SIGMA.get((net, method), 0.1)),
                f"{net} normalize {method}")


# ---- C9: optimisers -------------------------------------------------------------------------------------------------------------
OPTIMS = {"rmsprop": dict(optimizer_choice="rmsprop"), "rmsprop_mu0": dict(optimizer_choice="rmsprop", momentum=0.0),
          "adam_l2": dict(optimizer_choice="adam", l2_lambda=1e-4), "rmsprop_l2": dict(optimizer_choice="rmsprop", l2_lambda=1e-4)}
OPTIM_NETS = {"md2_b8_n30": Net(2, 30, 8, chans=CFG2, seed=3), "md3_n12": SPINE["md3_n12"]}
# {(net, optimiser): {parameter tensor: the oracle's disagreement with itself after three steps}}: none measured
_OPTIM_CONDITIONING = {}


@pytest.mark.parametrize("net", list(OPTIM_NETS))
@pytest.mark.parametrize("case", list(OPTIMS))
def test_optimisers_follow_oracle(case, net):
    """Three graph-replayed steps from live weights against three oracle steps with the torch optimiser lgn.step.torch_optimizer
    builds on the CPU leaves (L1 and L2 terms on the loss, as the reference's loop adds them): the loss of every step at FWD_TOL,
    l2_out against sum w^2 of the weights before the step, every parameter tensor at 1e-9 after the three."""
    from lgn.step import NativeTrainStep, torch_optimizer
    from oracle import lgn_oracle as O
    spec, kw = OPTIM_NETS[net], OPTIMS[case]
    enc, dec, Pe, Pd = _nets(spec, DEV)
    ce, cd = _cfgs(spec)
    _, p4, labels, _ = _batch(spec)
    lr, lam, l2 = 5e-4, 1e-8, kw.get("l2_lambda", 0.0)
    step = NativeTrainStep(enc, dec, batch_size=spec.B, lr=lr, l1_lambda=lam, use_graph=True, **kw)
    batch = _to_dev(_batch(spec)[0])
    for P in (Pe, Pd):
        for v in P.values():
            v.requires_grad_(True)
    opt = torch_optimizer(list(Pe.values()) + list(Pd.values()), kw["optimizer_choice"], lr, None, momentum=kw.get("momentum", 0.9))
    what = f"{net} {case}"
    # live on the data term alone: the regularisers give every tensor a gradient, the dead ones (exactly zero otherwise) included
    _, rec_o, grads_o, _, pooled = U.oracle_step(O, Pe, Pd, ce, cd, p4, labels, with_latent=True)
    U.assert_live(O, rec_o, grads_o, p4, O.get_real(rec_o, "sum"), pooled=pooled, latent_map=spec.latent)
    for it in range(3):
        with torch.no_grad():
            l2_o = sum((v * v).sum() for P in (Pe, Pd) for v in P.values())
        loss, _ = step.step(batch)
        loss_o, _, _ = U.oracle_step(O, Pe, Pd, ce, cd, p4, labels, l1_lambda=lam, l2_lambda=l2)
        opt.step()
        print(f"[{what}] step {it}: loss {float(loss_o):.6e}, rel err {U.relerr(loss.cpu(), loss_o):.2e}")
        U.assert_close(loss, loss_o, FWD_TOL, f"loss at step {it}")
        if l2:
            U.assert_close(step.l2_out.cpu()[0], l2_o, 1e-12, f"sum w^2 before step {it}")
    assert int(step.step_dev.item()) == 3
    measured = _OPTIM_CONDITIONING.get((net, case), {})
    errs = {f"{pre}.{k}": U.relerr(v.cpu(), P[k].detach()) for pre, mod, P in (("enc", enc, Pe), ("dec", dec, Pd)) for k, v in mod.state_dict().items()}
    strict = {k: e for k, e in errs.items() if k not in measured}
    name = max(strict, key=strict.get)
    print(f"[{what}] worst parameter tensor after 3 steps: {name}: rel err {strict[name]:.2e}")
    for k, e in errs.items():
        tol = 100 * measured[k] if k in measured else 1e-9
        assert e <= tol, f"{k} after 3 steps: rel err {e:.3e} > {tol:.1e}"
