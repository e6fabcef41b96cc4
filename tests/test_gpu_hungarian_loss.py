"""GPU tests of the native Hungarian-MSE and MSE training losses (csrc/assign_loss.hip): lgn.losses.HungarianMSELoss against the
CPU restatement and the reference's g19 vectors, the whole training / evaluation step with ``loss_choice`` against the oracle
networks and g19, the split step, unchanged Chamfer behaviour, a poisoned jet, and a short training run.

The device's asinh / atan2 / cos / sinh differ from the host's in the last bits, so among TIED columns (zero-padded target rows) the
device may find another optimal assignment: every comparison scores the NATIVE assignment with the restatement, and checks
separately that it is an optimum (same total exact cost)."""
import functools
import os

import numpy as np
import pytest
import torch

import _hungarian_ref as H
import _util as U

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
LOSSES = [("mse", True, False)] + [("hungarian",) + H.FRAMES[f] for f in H.FRAMES]
LOSS_IDS = ["mse"] + list(H.FRAMES)


def _check_optimal(x, t, col, a, p, padded, what, pool=True, identical=None):
    """col (B, N) is a permutation whose total exact cost on (x, t) is the restatement's optimum to 1e-12 relative; x is what the
    kernel saw.  Unpadded jets, and the abs Cartesian frame on every jet (exact IEEE costs on both sides): the two assignments are
    identical.  Other frames: at most 10 % of the padded jets may hold another optimum (device asinh / atan2 / cos / sinh last bits
    among tied columns).  pool = False -- a step's batch of two or three jets, where a share is not a rate: there the count is
    printed and the total-cost bound alone decides.  identical: overrides whether identity is asserted (a caller whose x is not
    bit for bit the kernel's).  Returns the share of jets that differ."""
    col = col.cpu().long()
    N = col.shape[1]
    assert bool((col.sort(-1).values == torch.arange(N)).all()), f"{what}: not a permutation"
    ref = H.assignment(x, t, a, p)
    np.testing.assert_allclose(H.total_cost(x, t, col, a, p).numpy(), H.total_cost(x, t, ref, a, p).numpy(), rtol=1e-12, atol=0,
                               err_msg=f"{what}: total cost")
    differ = (col != ref).any(-1).double().mean().item()
    print(f"{what}: native assignment differs from the restatement's on {100 * differ:.2f} % of the jets")
    if identical if identical is not None else (not padded or (a and not p)):
        assert differ == 0.0, what
    elif pool:
        assert differ <= 0.10, what
    return differ


@pytest.mark.parametrize("frame", list(H.FRAMES))
@pytest.mark.parametrize("N,n_real,B", [(1, None, 3), (12, None, 8), (12, 7, 20), (30, None, 16), (30, 20, 40), (64, None, 8), (64, 40, 20), (65, None, 4),
                                        (65, 50, 20), (150, None, 4), (150, 100, 10)])
def test_module_loss_matches_restatement(N, n_real, B, frame):
    from lgn.losses import HungarianMSELoss
    a, p = H.FRAMES[frame]
    x, t = H.jets(B, N, n_real, seed=N + B)
    xd = x.to(DEV).requires_grad_(True)
    fn = HungarianMSELoss()
    loss = fn(xd, t.to(DEV), abs_coord=a, polar_coord=p)
    (3.0 * loss).backward()
    assert fn.assignment.dtype == torch.int64 and int(fn.status.abs().max()) == 0
    _check_optimal(x, t, fn.assignment, a, p, n_real is not None, f"N={N} {frame}")
    xr = x.clone().requires_grad_(True)
    lr = H.loss(xr, t, fn.assignment.cpu(), a, p)
    (3.0 * lr).backward()
    U.assert_close(loss, lr, 1e-10, "loss")
    U.assert_close(xd.grad, xr.grad, 1e-10, "d loss / d x")


@pytest.mark.parametrize("frame", list(H.FRAMES))
@pytest.mark.parametrize("name,padded", [("g19_loss_n30.npz", False), ("g19_loss_n150.npz", False), ("g19_loss_n30_pad.npz", True)])
def test_module_loss_matches_reference_golden(name, padded, frame):
    from lgn.losses import HungarianMSELoss
    z = U.load(name)
    a, p = H.FRAMES[frame]
    x, t = torch.from_numpy(z["x"]), torch.from_numpy(z["t"])
    col_ref = torch.from_numpy(z[f"col.{frame}"].astype(np.int64))
    xd = x.to(DEV).requires_grad_(True)
    fn = HungarianMSELoss()
    loss = fn(xd, t.to(DEV), abs_coord=a, polar_coord=p)
    loss.backward()
    col = fn.assignment.cpu()
    same = (col == col_ref).all(-1)
    share = 1.0 - same.double().mean().item()
    print(f"{name} {frame}: native col differs from the reference's on {100 * share:.2f} % of the jets")
    g_ref = torch.from_numpy(z[f"grad.{frame}"])
    if not padded:
        assert bool(same.all())
        U.assert_close(loss, z[f"loss.{frame}"], 1e-10, "loss")
        U.assert_close(xd.grad, g_ref, 1e-10, "gradient")
    else:
        assert share <= 0.10
        _check_optimal(x, t, col, a, p, True, f"{name} {frame}")
        xr = x.clone().requires_grad_(True)
        lr = H.loss(xr, t, col, a, p)
        lr.backward()
        U.assert_close(loss, lr, 1e-10, "loss on the native assignment")
        U.assert_close(xd.grad, xr.grad, 1e-10, "gradient on the native assignment")
        U.assert_close(xd.grad[same.to(DEV)], g_ref[same], 1e-10, "gradient on the jets with the reference's col")


def test_mse_kind_matches_reference_golden():
    from lgn import _native as N
    z = U.load("g19_loss_n30_pad.npz")
    x, t = torch.from_numpy(z["x"]).to(DEV), torch.from_numpy(z["t"]).to(DEV)
    part, gx, col, status = N.hungarian_mse(x, t, kind=N.LOSS_MSE)
    U.assert_close(part.sum(), z["loss.mse"], 1e-12, "mse loss")
    U.assert_close(gx, z["grad.mse"], 1e-12, "mse gradient")
    assert bool((col.cpu() == torch.arange(30, dtype=torch.int32)).all()) and int(status.abs().max()) == 0


# ---- the whole step -----------------------------------------------------------------------------------------------------------
NETS = {"md2_n12": (2, 12, 3), "md2_n50": (2, 50, 2), "md3_n12": (3, 12, 2)}
CH = {2: ((3, 3, 4, 4), (4, 4, 3, 3)), 3: ((2, 3, 4), (4, 3, 2))}


def _models(net, seed=21, **kw):
    import __graft_entry__ as G
    maxdim, N, _ = NETS[net]
    return G._models(N, CH[maxdim][0], CH[maxdim][1], torch.device(DEV), seed=seed, maxdim=maxdim, **kw)


def _batch(net):
    from oracle import lgn_oracle as O
    _, N, B = NETS[net]
    return O.synthetic_jets(B, N, seed=N + B, pad=True)


@functools.lru_cache(maxsize=None)
def _oracle_forward(net, method):
    """The oracle networks' reconstruction and parameter leaves (CPU); the loss is attached per test (it needs step.assignment)."""
    from oracle import lgn_oracle as O
    maxdim, N, _ = NETS[net]
    enc, dec = _models(net)
    p4, labels = _batch(net)
    Pe = {k: v.detach().cpu().clone().requires_grad_(True) for k, v in enc.state_dict().items()}
    Pd = {k: v.detach().cpu().clone().requires_grad_(True) for k, v in dec.state_dict().items()}
    ce = O.NetConfig(num_particles=N, maxdim=maxdim, num_channels=CH[maxdim][0])
    cd = O.NetConfig(num_particles=N, maxdim=maxdim, num_channels=CH[maxdim][1])
    rec = O.decoder_forward(Pd, cd, O.encoder_forward(Pe, ce, p4, labels))
    return rec, O.get_real(rec, method), {f"{pre}.{k}": q for pre, P in (("enc", Pe), ("dec", Pd)) for k, q in P.items()}


def _oracle_grads(loss, leaves):
    """{name: gradient or None} of the oracle's named leaves."""
    return dict(zip(leaves, torch.autograd.grad(loss, list(leaves.values()), retain_graph=True, allow_unused=True)))


def _oracle_grad(loss, leaves):
    return torch.cat([(g if g is not None else torch.zeros_like(leaves[k])).reshape(-1) for k, g in _oracle_grads(loss, leaves).items()])


def _flat_grad(enc, dec):
    return torch.cat([g.detach().reshape(-1).cpu() for _, g in list(enc.named_grads()) + list(dec.named_grads())])


def _ref_loss(choice, x, t, col, a, p, n_jets=None):
    return H.mse_per_jet(x, t, n_jets).sum() if choice == "mse" else H.loss(x, t, col, a, p, n_jets)


@pytest.mark.parametrize("use_graph", [False, True])
@pytest.mark.parametrize("method", ["real", "norm"])
@pytest.mark.parametrize("loss", LOSSES, ids=LOSS_IDS)
@pytest.mark.parametrize("net", list(NETS))
def test_native_step_matches_oracle(net, loss, method, use_graph):
    from lgn.step import NativeTrainStep, get_real
    choice, a, p = loss
    enc, dec = _models(net)
    p4, labels = _batch(net)
    _, _, B = NETS[net]
    step = NativeTrainStep(enc, dec, batch_size=B, l1_lambda=0.0, optimizer=False, use_graph=use_graph, get_real_method=method,
                           loss_choice=choice, hungarian_abs_coord=a, hungarian_polar_coord=p)
    batch = {"p4": p4.to(DEV), "labels": labels.to(DEV)}
    for _ in range(2):
        step.assignment.fill_(-7)
        got, recon = step.step(batch)
    torch.cuda.synchronize()
    rec_o, x_o, leaves = _oracle_forward(net, method)
    col = step.assignment.cpu().long()
    assert int(step.status.abs().max()) == 0
    if choice == "hungarian":
        # optimality on the step's OWN reconstruction -- what the kernel solved on: bit for bit with 'real'; with 'norm' the kernel's
        # sqrt(re^2 + im^2 + eps) is contracted, torch's is not (last bits of x: far inside the 1e-12 of the total cost, but enough to
        # choose among tied columns, so identity is asserted with 'real' only)
        x_own = get_real(recon.detach(), method).cpu()
        _check_optimal(x_own, p4, col, a, p, True, f"{net} {choice} {a} {p} {method}", pool=False,
                       identical=bool(a and not p and method == "real"))
    else:
        assert bool((col == torch.arange(col.shape[1])).all())
    loss_o = _ref_loss(choice, x_o, p4, col, a, p)
    U.assert_close(got, loss_o.detach(), 1e-10, "loss")
    U.assert_close(recon, rec_o.detach(), 1e-10, "recon")
    U.assert_named_grads_close(U.named_grads(enc, dec), _oracle_grads(loss_o, leaves), 1e-10, f"{net} {choice} {a} {p} {method}")


@pytest.mark.parametrize("method", ["real", "norm"])
@pytest.mark.parametrize("net", list(NETS))
def test_reconstruction_is_the_chamfer_steps_bit_for_bit(net, method):
    from lgn.step import NativeTrainStep
    p4, labels = _batch(net)
    batch = {"p4": p4.to(DEV), "labels": labels.to(DEV)}
    recs = []
    for choice in ("chamfer", "hungarian"):
        enc, dec = _models(net)
        step = NativeTrainStep(enc, dec, batch_size=NETS[net][2], l1_lambda=0.0, optimizer=False, use_graph=False, get_real_method=method,
                               loss_choice=choice)
        recs.append(step.step(batch)[1].clone())
    assert torch.equal(recs[0], recs[1])


STEP_GOLDEN = [f"g19_step_{tag}_maxdim{m}.npz" for m in (2, 3) for tag in ("hungarian", "relpolar", "mse")]


def _golden_step(name, kind, use_graph=True):
    """The reference's loss, reconstruction, assignment and every parameter gradient through a step.  The fixtures' optimum is
    decidable (one zero row: no tied columns; stable under 1e-8 perturbations of x, tests/golden/gen_golden_g19.py), so the step
    must find the reference's assignment on every jet, and every comparison always runs."""
    import __graft_entry__ as G
    from lgn.step import CapturedModuleStep, NativeTrainStep, ReferenceLoopStep
    dev = torch.device(DEV)
    z = U.load(name)
    m = U.meta(z)
    enc, dec = G._models(m["N"], m["ch_enc"], m["ch_dec"], dev, seed=m["seed"], maxdim=m["maxdim"])
    batch = {"p4": torch.from_numpy(z["p4"]).to(dev), "labels": torch.from_numpy(z["labels"]).to(dev)}
    opts = dict(l1_lambda=0.0, optimizer=False, get_real_method="real", loss_choice=m["loss_choice"],
                hungarian_abs_coord=m["hungarian_abs_coord"], hungarian_polar_coord=m["hungarian_polar_coord"])
    if kind == "native":
        step = NativeTrainStep(enc, dec, m["B"], use_graph=use_graph, **opts)
    elif kind == "captured":
        step = CapturedModuleStep(enc, dec, m["B"], use_graph=use_graph, **opts)
    else:
        step = ReferenceLoopStep(enc, dec, native_loss=True, **opts)
    for _ in range(2):
        loss, recon = step.step(batch)
    U.assert_close(recon, z["recon"], 1e-9, "recon")
    a, p, choice = m["hungarian_abs_coord"], m["hungarian_polar_coord"], m["loss_choice"]
    col_ref = torch.from_numpy(z["col"].astype(np.int64))
    if kind == "native":
        col = step.assignment.cpu().long()
    elif choice == "mse":
        col = col_ref
    else:
        col = step.loss_fn.module.assignment.cpu()
    assert torch.equal(col, col_ref), f"{name} {kind}: assignment differs from the reference's on jets {(col != col_ref).any(-1).nonzero().flatten().tolist()}"
    U.assert_close(loss, z["loss"], 1e-9, "loss")
    scale = max(float(abs(z[k]).max()) for k in z.files if k.startswith("grad."))
    for pre, mod in (("enc", enc), ("dec", dec)):
        for k, g in mod.named_grads():
            U.assert_close_scaled(g, torch.from_numpy(z[f"grad.{pre}.{k}"]), 1e-9, scale, f"grad {pre}.{k}")


@pytest.mark.parametrize("use_graph", [False, True])
@pytest.mark.parametrize("name", STEP_GOLDEN)
def test_native_step_matches_reference_golden(name, use_graph):
    _golden_step(name, "native", use_graph)


@pytest.mark.parametrize("name", STEP_GOLDEN)
def test_captured_module_step_matches_reference_golden(name):
    _golden_step(name, "captured")


@pytest.mark.parametrize("name", STEP_GOLDEN)
def test_reference_loop_step_matches_reference_golden(name):
    _golden_step(name, "loop")


@pytest.mark.parametrize("loss", LOSSES, ids=LOSS_IDS)
@pytest.mark.parametrize("net", list(NETS))
def test_eval_step_is_the_training_steps_forward(net, loss):
    """Loss = the training step's without L1, recon = its get_real reconstruction bit for bit; a short last batch takes the mean
    over its real jets; ModuleEvalStep agrees."""
    from lgn.step import ModuleEvalStep, NativeEvalStep, NativeTrainStep, get_real
    choice, a, p = loss
    opts = dict(get_real_method="real", loss_choice=choice, hungarian_abs_coord=a, hungarian_polar_coord=p)
    enc, dec = _models(net)
    p4, labels = _batch(net)
    B = NETS[net][2]
    batch = {"p4": p4.to(DEV), "labels": labels.to(DEV)}
    train = NativeTrainStep(enc, dec, batch_size=B, l1_lambda=1e-3, optimizer=False, use_graph=False, **opts)
    train.step(batch)
    ev = NativeEvalStep(enc, dec, batch_size=B, use_graph=True, **opts)
    for _ in range(2):
        out = ev.run(batch)
    assert torch.equal(out["recon"], get_real(train.recon, "real"))
    assert torch.equal(out["loss"], train.loss_part.sum()) or abs(out["loss"].item() - train.loss_part.sum().item()) <= 1e-14 * abs(out["loss"].item())
    assert torch.equal(ev.loss_part, train.loss_part)
    assert torch.equal(ev.assignment, train.assignment)
    ms = ModuleEvalStep(enc, dec, batch_size=B, **opts)
    mod = ms.run(batch)
    U.assert_close(out["recon"], mod["recon"], 1e-10, "ModuleEvalStep recon")
    # the module route's loss is the restatement's on ITS assignment (among tied columns it may hold another optimum than the step's);
    # where the two routes found the same assignment the two losses agree
    mcol = ev.assignment.cpu().long() if choice == "mse" else ms.loss_fn.module.assignment.cpu()
    U.assert_close(mod["loss"], _ref_loss(choice, mod["recon"].cpu(), p4, mcol, a, p), 1e-10, "ModuleEvalStep loss")
    if choice != "mse":
        _check_optimal(mod["recon"].cpu(), p4, mcol, a, p, padded=not (a and not p), what=f"ModuleEvalStep {net} {a} {p}", pool=False)
    if torch.equal(mcol, ev.assignment.cpu().long()):
        U.assert_close(out["loss"], mod["loss"], 1e-10, "ModuleEvalStep loss against the native step's")
    # short last batch: B' = B - 1 real jets, the mean runs over them
    short = {k: v[:B - 1] for k, v in batch.items()}
    out = ev.run(short)
    x = out["recon"].cpu()
    want = _ref_loss(choice, x, p4[:B - 1], ev.assignment[:B - 1].cpu().long(), a, p)
    U.assert_close(out["loss"], want, 1e-10, "short batch loss")


@pytest.mark.parametrize("loss", [LOSSES[0], LOSSES[1], LOSSES[3]], ids=["mse", "abs_cart", "rel_polar"])
def test_split_step_matches_captured_module_step(loss):
    """jet_features encoder (the split form of the step) against the module-API step under autograd on the same weights."""
    import __graft_entry__ as G
    from lgn.step import CapturedModuleStep, NativeTrainStep
    from oracle import lgn_oracle as O
    choice, a, p = loss
    dev = torch.device(DEV)
    N, B = 12, 3
    nets = [G._models(N, (3, 3, 4, 4), (4, 4, 3, 3), dev, seed=9, jet_features=True) for _ in range(2)]
    p4, labels = O.synthetic_jets(B, N, seed=4, pad=False)
    batch = {"p4": p4.to(dev), "labels": labels.to(dev)}
    opts = dict(batch_size=B, l1_lambda=0.0, optimizer=False, get_real_method="real", loss_choice=choice, hungarian_abs_coord=a,
                hungarian_polar_coord=p)
    s1 = NativeTrainStep(*nets[0], use_graph=True, **opts)
    assert s1.split
    s2 = CapturedModuleStep(*nets[1], use_graph=False, **opts)
    for _ in range(2):
        la, ra = s1.step(batch)
    lb, rb = s2.step(batch)
    U.assert_close(la, lb, 1e-10, "loss")
    U.assert_close(ra, rb, 1e-10, "recon")
    U.assert_close(s1.flat.grad, s2.flat.grad, 1e-9, "flat gradient")


def test_two_call_form_equals_the_single_call():
    """lgn_step_fwd_bwd_f64 + lgn_step_finalize_f64 (the data-parallel form: the all-reduce sits between them) against the
    single call lgn_step_train_f64, both with a loss descriptor."""
    from lgn.step import NativeTrainStep
    p4, labels = _batch("md2_n12")
    batch = {"p4": p4.to(DEV), "labels": labels.to(DEV)}
    out = []
    for two in (False, True):
        enc, dec = _models("md2_n12")
        step = NativeTrainStep(enc, dec, batch_size=3, optimizer=True, use_graph=False, get_real_method="real", loss_choice="hungarian")
        step.load_batch(batch)
        for _ in range(2):
            if two:
                step._fwd_bwd()
                step._finalize(True)
            else:
                step._train(True)
        torch.cuda.synchronize()
        out.append((step.loss_out.clone(), step.flat.flat.clone(), step.flat.grad.clone(), step.assignment.clone()))
    for x, y in zip(*out):
        assert torch.equal(x, y)


@pytest.mark.parametrize("kind,choice", [("native", "hungarian"), ("native", "mse"), ("native", "hungarian_rel_polar"),
                                         ("captured", "hungarian"), ("captured", "mse"), ("loop", "hungarian"), ("loop", "mse")])
def test_two_ranks_match_single_process(kind, choice, tmp_path):
    """2 ranks x 8 jets equal one process x 16 jets after three Adam steps: the mse / hungarian losses are means over the GLOBAL
    batch, so each rank scales by 1 / (8 x 2 x N x D) (NativeTrainStep) or weighs its local mean by 1 / 2 (CapturedModuleStep,
    ReferenceLoopStep) before the SUM all-reduce.  Unpadded jets: a unique optimum, whichever process solves it."""
    import socket
    import subprocess
    import sys as _sys
    import _dist_hungarian_worker as W
    per_rank, world, steps = 8, 2, 3
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    procs = [subprocess.Popen([_sys.executable, W.__file__, str(r), str(world), str(port), str(tmp_path), str(per_rank), str(steps), kind,
                               choice], stdout=subprocess.PIPE, stderr=subprocess.STDOUT) for r in range(world)]
    outs = [p.communicate(timeout=600)[0].decode(errors="replace") for p in procs]
    for r, (p, o) in enumerate(zip(procs, outs)):
        assert p.returncode == 0, f"rank {r} failed:\n{o[-3000:]}"
    step, enc, dec = W.build(kind, choice, per_rank * world)
    batch = W.batch(per_rank * world, slice(None))
    ref_losses = [float(step.step(batch)[0]) for _ in range(steps)]
    ref_params = W.params(enc, dec)
    for r in range(world):
        z = torch.load(os.path.join(str(tmp_path), f"rank{r}.pt"))
        U.assert_close(z["params"], ref_params, 1e-9, f"rank {r} parameters after {steps} steps")
        if kind != "loop":          # (ReferenceLoopStep returns the rank's own loss; the other two the all-reduced one)
            for x, y in zip(z["losses"], ref_losses):
                assert abs(x - y) <= 1e-10 * max(1.0, abs(y)), (z["losses"], ref_losses)
    if kind == "loop":              # the two ranks' own means average to the whole batch's
        both = [torch.load(os.path.join(str(tmp_path), f"rank{r}.pt"))["losses"] for r in range(world)]
        for x0, x1, y in zip(both[0], both[1], ref_losses):
            assert abs((x0 + x1) / 2 - y) <= 1e-10 * max(1.0, abs(y)), (both, ref_losses)


def test_chamfer_by_name_is_the_step_without_the_argument():
    from lgn.step import NativeTrainStep
    p4, labels = _batch("md2_n12")
    batch = {"p4": p4.to(DEV), "labels": labels.to(DEV)}
    out = []
    for kw in ({}, {"loss_choice": "chamfer"}):
        enc, dec = _models("md2_n12")
        step = NativeTrainStep(enc, dec, batch_size=3, optimizer=True, use_graph=True, get_real_method="real", **kw)
        assert step.loss_desc is None and step.assignment is None
        for _ in range(3):
            loss, _ = step.step(batch)
        out.append((loss.clone(), step.flat.grad.clone(), step.flat.flat.clone(), step.adam_m.clone(), step.adam_v.clone()))
    for x, y in zip(*out):
        assert torch.equal(x, y)


def test_poisoned_jet_sets_its_status_and_the_next_step_is_clean():
    """A NaN in one target row: that jet's cost matrix holds NaN -> status bit, NaN loss, the call returns; a clean step follows."""
    from lgn import _native as N
    from lgn.step import NativeTrainStep
    x, t = H.jets(6, 30, 20, seed=5)
    bad = t.clone()
    bad[2, 3, 1] = float("nan")
    part, gx, col, status = N.hungarian_mse(x.to(DEV), bad.to(DEV))
    assert status.cpu().tolist() == [0, 0, 1, 0, 0, 0]
    assert bool(torch.isnan(part[2])) and bool(torch.isfinite(part[[0, 1, 3, 4, 5]]).all())
    assert bool((gx[2] == 0).all()) and bool((col[2] == -1).all()) and bool(torch.isfinite(gx).all())
    enc, dec = _models("md2_n12")
    p4, labels = _batch("md2_n12")
    step = NativeTrainStep(enc, dec, batch_size=3, l1_lambda=0.0, optimizer=False, use_graph=False, get_real_method="real",
                           loss_choice="hungarian")
    poisoned = p4.clone()
    poisoned[1, 2, 2] = float("nan")
    loss, _ = step.step({"p4": poisoned.to(DEV), "labels": labels.to(DEV)})
    torch.cuda.synchronize()
    assert step.status.cpu().tolist() == [0, 1, 0] and bool(torch.isnan(loss)) and bool((step.assignment[1] == -1).all())
    loss, _ = step.step({"p4": p4.to(DEV), "labels": labels.to(DEV)})
    rec_o, x_o, leaves = _oracle_forward("md2_n12", "real")
    assert step.status.cpu().tolist() == [0, 0, 0]
    loss_o = H.loss(x_o, p4, step.assignment.cpu().long())
    U.assert_close(loss, loss_o.detach(), 1e-10, "loss after the poisoned step")
    U.assert_close(_flat_grad(enc, dec), _oracle_grad(loss_o, leaves), 1e-10, "gradient after the poisoned step")


def test_hungarian_step_trains():
    import __graft_entry__ as G
    from lgn.step import NativeTrainStep
    from oracle import lgn_oracle as O
    enc, dec = G._models(30, (3, 3, 4, 4), (4, 4, 3, 3), torch.device(DEV), seed=3)
    p4, labels = O.synthetic_jets(32, 30, seed=11, pad=True)
    batch = {"p4": p4.to(DEV), "labels": labels.to(DEV)}
    step = NativeTrainStep(enc, dec, batch_size=32, lr=5e-4, use_graph=True, get_real_method="real", loss_choice="hungarian")
    losses = [step.step(batch)[0].item() for _ in range(30)]
    print("hungarian training losses", losses[0], losses[-1])
    assert all(np.isfinite(losses)) and losses[-1] < losses[0], f"loss did not fall: {losses[0]} -> {losses[-1]}"
