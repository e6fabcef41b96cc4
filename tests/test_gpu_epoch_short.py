"""GPU tests of remainder='short' (the short last batch of a training epoch as a step of a second plan) and of the latent's
collection: the two entry points csrc/stage.hip gained against the first two and against torch on the same rows (bit for bit), the
short step against a fresh NativeTrainStep of that batch size, the runner against the host loop (torch.equal: the same kernels on
the same inputs in the same order) and against the reference's loop on the module API (to the tolerances of the existing
native-versus-ReferenceLoopStep comparisons), and the collected latent against step.run's per batch."""
import ctypes as C

import pytest
import torch

import _util as U
import test_gpu_epoch as E          # its shared inputs and helpers: _data, _pairs, _train_data, _buffers, _staged, _same, CODES

pytestmark = pytest.mark.gpu

DEV = E.DEV
M, B = E.M, E.B                     # 10 jets in batches of 4: two whole batches and a short one of r = 2


def _ptr_array(ts):
    from lgn import _native as N_
    return (C.c_void_p * len(ts))(*[N_.ptr(t) for t in ts])


def _collect(new, srcs, rds, planes, count, Bc, cursor, base=0):
    """One raw collect call at a cursor written from the host into NaN-filled destinations.  Returns (dsts, epoch, cursor)."""
    from lgn import _native as N_
    dsts = [torch.full((p * count * rd,), float("nan"), device=DEV, dtype=torch.float64) for rd, p in zip(rds, planes)]
    cur = torch.tensor([cursor, 0], device=DEV, dtype=torch.int64)
    epoch = torch.tensor([1.5, 3.0], device=DEV, dtype=torch.float64)
    loss = torch.tensor([0.1], device=DEV, dtype=torch.float64)
    head = (N_.ptr(loss), N_.ptr(epoch), N_.ptr(cur), count)
    arrays = (_ptr_array(srcs), _ptr_array(dsts), (C.c_int * len(rds))(*rds))
    if new:
        rc = N_.lib().lgn_epoch_collect_planes_f64(*head, base, Bc, len(srcs), *arrays, (C.c_int * len(planes))(*planes), N_.stream_ptr())
    else:
        rc = N_.lib().lgn_epoch_collect_f64(*head, Bc, len(srcs), *arrays, N_.stream_ptr())
    N_._check(rc, "collect")
    torch.cuda.synchronize()
    return dsts, epoch, cur


def _bits(t):
    return t.view(torch.int64)


@pytest.mark.parametrize("N", [1, 6, 70])
def test_planes_1_base_0_is_the_first_collect_call(N):
    """On the staged tensors of the existing gather test's inputs -- target (rd = 4 N), factor (4), a mask-wide odd row (N + 1 doubles:
    unaligned rows for even N) and a one-double row -- at every cursor of the epoch and one behind it: the bits of lgn_epoch_collect_f64
    in every destination (NaN where nothing is written), the same loss sum, step count, ticket and cursor."""
    p4, labels, _ = E._data(N)
    out = E._staged(p4, labels, None, torch.arange(B, device=DEV), E.CODES["overall_max"], 1.0, False, 0, False)
    g = torch.Generator().manual_seed(N)
    odd = torch.randn(B, N + 1, generator=g, dtype=torch.float64).to(DEV)
    one = torch.randn(B, 1, generator=g, dtype=torch.float64).to(DEV)
    srcs, rds = [out[1], out[4], odd, one], [4 * N, 4, N + 1, 1]
    # batches of 4, and of 3 (the first three rows of each source): odd runs, destinations off the 16-byte grid
    for Bc, cursors in ((B, (0, 1, 2, 3)), (3, (0, 1, 3, 4))):
        for cursor in cursors:
            old = _collect(False, srcs, rds, [1] * 4, M, Bc, cursor)
            new = _collect(True, srcs, rds, [1] * 4, M, Bc, cursor)
            for k, (a, b) in enumerate(zip(old[0], new[0])):
                assert torch.equal(_bits(a), _bits(b)), f"B {Bc}, cursor {cursor}: destination {k}"
            assert torch.equal(old[1], new[1]) and torch.equal(old[2], new[2])
            assert new[2].tolist() == [cursor + 1, 0] and new[1].tolist() == [1.5 + 0.1, 4.0]
            written = int((~new[0][3].isnan()).sum().item())
            assert written == max(0, min(Bc, M - cursor * Bc)), "rows written"


@pytest.mark.parametrize("rd", [1, 3, 8])
def test_collect_planes_with_a_base_row(rd):
    """Source [2][r][rd] at base row 8 of [2][10][rd] (the short plan behind two batches of 4: cursor 2, base = 2 (4 - 2)), next to a
    one-plane tensor: each plane's rows land at row 8 of its plane, everything else stays untouched."""
    r, full = 2, 2
    g = torch.Generator().manual_seed(rd)
    two = torch.randn(2, r, rd, generator=g, dtype=torch.float64).to(DEV)
    flat = torch.randn(r, 5, generator=g, dtype=torch.float64).to(DEV)
    (d2, d1), epoch, cur = _collect(True, [two, flat], [rd, 5], [2, 1], M, r, full, base=full * (B - r))
    d2, d1 = d2.view(2, M, rd), d1.view(M, 5)
    assert torch.equal(d2[:, 8:], two) and torch.equal(d1[8:], flat)
    assert bool(d2[:, :8].isnan().all()) and bool(d1[:8].isnan().all())
    assert cur.tolist() == [full + 1, 0] and epoch.tolist()[1] == 4.0
    # a cursor behind the epoch copies nothing and still books the step
    (d2, d1), epoch, cur = _collect(True, [two, flat], [rd, 5], [2, 1], M, r, full + 1, base=full * (B - r))
    assert bool(d2.isnan().all()) and bool(d1.isnan().all()) and cur.tolist() == [full + 2, 0]


@pytest.mark.parametrize("variant", ["plain", "jet_scalars", "aliased"])
@pytest.mark.parametrize("method", ["none", "component_max", "jet_E"])
def test_gather_at_is_the_batch_staging_of_the_rows_behind_the_base(method, variant):
    """lgn_stage_gather_at_f64 for a plan of r = 2 jets at cursor 2 with base = 2 (4 - 2): rows index[8], index[9], bit for bit what
    lgn_stage_batch_f64 stages for them; with base = 0 it is lgn_stage_gather_f64."""
    from lgn import _native as N_
    v = E.VARIANTS[variant]
    jet, K, scale, alias = v.get("jet", False), v.get("K", 0), v.get("scale", 1.0), v.get("alias", False)
    N, r, full = 6, 2, 2
    p4, labels, scalars = E._data(N)
    labels, scalars = (labels if v.get("labels") else None), (scalars if K else None)
    index = torch.randperm(M, generator=torch.Generator().manual_seed(3)).to(torch.int32).to(DEV)

    def gather_at(Bp, cursor, base):
        nan = lambda *s: torch.full(s, float("nan"), device=DEV, dtype=torch.float64)      # noqa: E731
        Nn = N + int(jet)
        target = nan(Bp, N, 4)
        out = (target if alias else nan(Bp, Nn, 4), target, torch.full((Bp, Nn), 255, device=DEV, dtype=torch.uint8),
               nan(Bp, Nn, int(jet) + K) if jet or K else None, nan(Bp, 4))
        cur = torch.tensor([cursor, 0], device=DEV, dtype=torch.int64)
        status = torch.zeros(1, device=DEV, dtype=torch.int32)
        N_._check(N_.lib().lgn_stage_gather_at_f64(N_.ptr(p4), N_.ptr(labels), N_.ptr(scalars), M, N_.ptr(index), M, base, N_.ptr(cur), Bp,
                                                   N, E.CODES[method], scale, int(jet), K, *[N_.ptr(t) for t in out], N_.ptr(status),
                                                   N_.stream_ptr()), "lgn_stage_gather_at_f64")
        torch.cuda.synchronize()
        assert status.item() == 0 and cur.tolist() == [cursor, 0]
        return out

    got = gather_at(r, full, full * (B - r))
    want = E._staged(p4, labels, scalars, index[8:], E.CODES[method], scale, jet, K, alias)
    for name, g, w in zip(("p4_in", "target", "mask", "in_scalars", "factor"), got, want):
        if g is not None:
            assert torch.equal(g, w[:r]), f"{name} differs from lgn_stage_batch_f64 on index[8:]"
    for cursor in (0, 2):
        first, _ = E._gather(p4, labels, scalars, index, cursor, E.CODES[method], scale, jet, K, alias)
        E._same(gather_at(B, cursor, 0), first, f"base 0, cursor {cursor}")


# ---- the short step ------------------------------------------------------------------------------------------------------------
SHORT_CASES = {
    "adam_chamfer_jet_features": dict(chamfer_jet_features=True),
    "rmsprop_hungarian_normalize_l2": dict(optimizer_choice="rmsprop", loss_choice="hungarian", normalize=True, l2_lambda=1e-4),
    "mse_norm": dict(loss_choice="mse", get_real_method="norm"),
}


def _data_of(kw):
    p4, labels = E._train_data(kw.get("normalize", False))
    return {"p4": p4, "labels": labels} if kw.get("normalize") else {"p4": p4}


def _same_state(a, b, steps, what):
    assert torch.equal(a.flat.flat, b.flat.flat), f"{what}: parameters"
    assert torch.equal(a.adam_m, b.adam_m) and torch.equal(a.adam_v, b.adam_v), f"{what}: optimiser state"
    assert torch.equal(a.step_dev, b.step_dev) and int(a.step_dev.item()) == steps, f"{what}: step counter"


@pytest.mark.parametrize("case", list(SHORT_CASES))
def test_the_short_step_is_a_step_of_r_jets(case):
    """M = 3 jets in batches of 4: the epoch is ONE short step from fresh state, and it is the step a fresh NativeTrainStep(batch_size=3)
    takes on those rows -- parameters, both optimiser tensors, counter and loss, bit for bit."""
    from lgn.epoch import DeviceDataset, EpochRunner
    from lgn.step import NativeTrainStep
    kw = SHORT_CASES[case]
    data = {k: v[:3].contiguous() for k, v in _data_of(kw).items()}
    (ea, da), (eb, db) = E._pairs()
    a = NativeTrainStep(ea, da, batch_size=B, lr=1e-3, **kw)
    b = NativeTrainStep(eb, db, batch_size=3, lr=1e-3, **kw)
    runner = EpochRunner(a, DeviceDataset(data, shuffle=False), shuffle=False, remainder="short")
    assert (runner.steps, runner.count, runner.short) == (1, 3, 3)
    out = runner.run_epoch()
    loss, _ = b.step(data)
    print(f"{case}: short step loss {out['loss_sum']!r}, a step of 3 jets {loss.item()!r}")
    assert out["steps"] == 1 and out["status"] == 0 and runner.launches_per_epoch == 1
    assert out["loss_sum"] == loss.item() and out["avg_loss"] == loss.item()
    _same_state(a, b, 1, case)
    short = a.short_step(3)
    assert short is a.short_step(3) and short.desc.B == 3 and tuple(short.recon.shape) == (2, 3, E.N_STEP, 4)
    assert short.flat.flat is a.flat.flat and short.adam_m is a.adam_m and short.step_dev is a.step_dev
    assert torch.equal(short.recon, b.recon)


def test_the_short_step_of_one_jet():
    """r = 1 (M = 5, B = 4), the single-jet regime, behind one whole batch: against a NativeTrainStep(batch_size=1) that takes over the
    state the whole batch's step left (parameters through its modules, the optimiser tensors and the counter copied)."""
    from lgn.epoch import DeviceDataset, EpochRunner
    from lgn.step import NativeTrainStep
    kw = SHORT_CASES["adam_chamfer_jet_features"]
    data = {k: v[:5].contiguous() for k, v in _data_of(kw).items()}
    (ea, da), (eb, db) = E._pairs()
    a = NativeTrainStep(ea, da, batch_size=B, lr=1e-3, **kw)
    b = NativeTrainStep(eb, db, batch_size=B, lr=1e-3, **kw)
    runner = EpochRunner(a, DeviceDataset(data, shuffle=False), shuffle=False, remainder="short")
    out = runner.run_epoch()
    assert out["steps"] == 2 and runner.launches_per_epoch == 2 and runner.short == 1
    l0, _ = b.step({k: v[:4] for k, v in data.items()})
    l0 = l0.item()
    c = NativeTrainStep(eb, db, batch_size=1, lr=1e-3, **kw)          # (re-homes b's parameters as they are now)
    for dst, src in ((c.adam_m, b.adam_m), (c.adam_v, b.adam_v), (c.step_dev, b.step_dev)):
        dst.copy_(src)
    l1, _ = c.step({k: v[4:5] for k, v in data.items()})
    assert out["loss_sum"] == l0 + l1.item()
    _same_state(a, c, 2, "r = 1")


@pytest.mark.parametrize("use_graph", [True, False], ids=["graph", "eager"])
@pytest.mark.parametrize("case", list(E.TRAIN_CASES))
def test_short_epochs_are_the_host_loop(case, use_graph):
    """Two shuffled epochs of M = 10 in batches of 4 with remainder='short': step.step x 2, then step.short_step(2).step on the rows
    behind them -- parameters, optimiser state, counter, the collected target / norm_factor of all 10 jets and the loss sum (the
    Python sum of the three .item() values) are the host loop's.  An epoch with remainder='drop' still covers 8 jets."""
    from lgn.epoch import DeviceDataset, EpochRunner
    from lgn.step import NativeTrainStep
    kw = E.TRAIN_CASES[case]
    p4, labels = E._train_data(kw.get("normalize", False))
    data = {"p4": p4, "labels": labels} if kw else {"p4": p4}
    (ea, da), (eb, db) = E._pairs()
    a = NativeTrainStep(ea, da, batch_size=B, lr=1e-3, use_graph=use_graph, **kw)
    b = NativeTrainStep(eb, db, batch_size=B, lr=1e-3, **kw)
    ds = DeviceDataset(data, shuffle=False)
    runner = EpochRunner(a, ds, shuffle=True, generator=torch.Generator().manual_seed(5), collect=("target", "norm_factor"),
                         remainder="short")
    assert (runner.steps, runner.count, runner.short) == (3, M, 2)
    epochs = []
    for _ in range(2):
        out = runner.run_epoch()
        assert out["steps"] == 3 and out["status"] == 0 and out["avg_loss"] == out["loss_sum"] / 3
        assert runner.launches_per_epoch == (3 if use_graph else 9)
        epochs.append((runner.index.clone(), out["loss_sum"], {k: v.clone() for k, v in out["collected"].items()}))
    g = torch.Generator().manual_seed(5)
    for index, loss_sum, collected in epochs:
        assert torch.equal(index.cpu(), torch.randperm(M, generator=g).to(torch.int32))
        losses, targets, factors = [], [], []
        for i in range(3):
            rows = index[i * B:(i + 1) * B].long()
            s = b if i < 2 else b.short_step(2)
            loss, _ = s.step({k: v[rows] for k, v in data.items()})
            losses.append(loss.item())
            targets.append(s.target.clone())
            factors.append(s.norm_factor.clone())
        print(f"{case}: epoch loss sum {loss_sum!r}, host loop {sum(losses)!r}")
        assert loss_sum == sum(losses)
        assert tuple(collected["target"].shape) == (M, E.N_STEP, 4)
        assert torch.equal(collected["target"], torch.cat(targets)) and torch.equal(collected["norm_factor"], torch.cat(factors))
    _same_state(a, b, 6, case)
    dropped = EpochRunner(a, ds, shuffle=False, remainder="drop")
    out = dropped.run_epoch()
    assert (dropped.steps, dropped.count, dropped.short, out["steps"]) == (2, 8, 0, 2)


class _JetChamfer(torch.nn.Module):
    """lgn.losses.ChamferLoss with the jet-feature term (--chamfer-jet-features) as a loss module for ReferenceLoopStep."""

    def __init__(self):
        super().__init__()
        from lgn.losses import ChamferLoss
        self.fn = ChamferLoss(device=torch.device(DEV))

    def forward(self, x, t):
        return self.fn(x, t, jet_features=True)


@pytest.mark.parametrize("case", ["hungarian", "chamfer_jet_features"])
def test_a_short_epoch_is_the_reference_loop(case):
    """The three batches (4, 4, 2) through lgn.step.ReferenceLoopStep -- the module API, torch autograd and torch.optim, which takes
    any batch size -- against one epoch of the runner: the loss of every step and the parameters after the epoch.  Tolerances: those of
    the native step against ReferenceLoopStep over three optimiser steps, test_gpu_step.py::test_reference_loop_step_matches_native_step
    and test_gpu_optimizer_options.py (loss 1e-10 per step, parameters 1e-9; test_gpu_normalize.py holds a single step's loss to
    1e-12 and its gradient to 1e-9).  A 1 / B left where 1 / r belongs doubles the short step's mean at these shapes: no tolerance
    hides it.
    Measured on an MI355X: every step's loss, the short one included, equals the loop's to the last bit in both cases; the parameters
    after the epoch differ by 1.0e-17 of their largest entry."""
    from lgn.epoch import DeviceDataset, EpochRunner
    from lgn.step import NativeTrainStep, ReferenceLoopStep
    native = dict(loss_choice="hungarian") if case == "hungarian" else dict(chamfer_jet_features=True)
    p4, _ = E._train_data(False)
    (ea, da), (eb, db) = E._pairs()
    a = NativeTrainStep(ea, da, batch_size=B, lr=1e-3, **native)
    loop = ReferenceLoopStep(eb, db, lr=1e-3, loss_choice="hungarian" if case == "hungarian" else _JetChamfer())
    # the runner returns the epoch's loss SUM: the loss of each step comes from the native host loop on a third pair of networks
    # (step x 2, short_step(2)), which ends the epoch on the runner's parameters bit for bit
    runner = EpochRunner(a, DeviceDataset({"p4": p4}, shuffle=False), shuffle=False, remainder="short")
    (ec, dc), = E._pairs(1)
    host = NativeTrainStep(ec, dc, batch_size=B, lr=1e-3, **native)
    ref_losses = []
    for i in range(3):
        batch = {"p4": p4[i * B:(i + 1) * B]}
        lr_, _ = loop.step(batch)
        ln, _ = (host if i < 2 else host.short_step(2)).step(batch)
        e = U.assert_close(ln, lr_, 1e-10, f"loss of step {i} ({batch['p4'].shape[0]} jets)")
        print(f"{case}: step {i} ({batch['p4'].shape[0]} jets) loss {ln.item()!r}, reference loop {lr_.item()!r}, rel {e:.2e}")
        ref_losses.append(lr_.item())
    out = runner.run_epoch()
    ref_params = torch.cat([eb.flat_params.detach(), db.flat_params.detach()])
    e = U.assert_close(a.flat.flat, ref_params, 1e-9, "parameters after the epoch")
    print(f"{case}: parameters after the epoch, rel {e:.2e}")
    U.assert_close(torch.tensor(out["loss_sum"]), torch.tensor(sum(ref_losses)), 1e-10, "the epoch's loss sum")
    assert torch.equal(a.flat.flat, host.flat.flat)


# ---- the latent ----------------------------------------------------------------------------------------------------------------
LATENT_CASES = {"min&max": dict(N=6, Bc=4), "mix_odd_rows": dict(N=6, Bc=3, map_to_latent="mix"), "one_particle": dict(N=1, Bc=4)}


@pytest.mark.parametrize("case", list(LATENT_CASES))
def test_the_collected_latent_is_the_batches_latents(case):
    """collect=('latent', 'recon') over M = 10 jets, run twice: {(0, 0): (2, M, ...), (1, 1): (2, M, ...)} is step.run(batch)['latent']
    of every batch concatenated on dim 1 (the reference's latent_dict), the padded rows of the short batch left out.  'mix' in batches
    of 3 has rows of another width whose destinations are not 16-byte aligned; N = 1 is the smallest jet."""
    import __graft_entry__ as G
    from lgn.epoch import DeviceDataset, EpochRunner
    from lgn.step import NativeEvalStep
    c = LATENT_CASES[case]
    N, Bc = c["N"], c["Bc"]
    p4, labels, _ = E._data(N)
    p4 = (p4 / (p4.abs().amax(dim=(1, 2), keepdim=True) + 1e-16)).contiguous()
    data = {"p4": p4, "labels": labels} if N > 1 else {"p4": p4}
    nets = [G._models(N, E.CH[0], E.CH[1], torch.device(DEV), seed=23, maxdim=2, map_to_latent=c.get("map_to_latent", "min&max"))
            for _ in range(2)]
    a = NativeEvalStep(*nets[0], batch_size=Bc, keep_latent=True)
    b = NativeEvalStep(*nets[1], batch_size=Bc, keep_latent=True)
    runner = EpochRunner(a, DeviceDataset(data, shuffle=False), shuffle=False, collect=("latent", "recon"))
    want = {(0, 0): [], (1, 1): [], "recon": []}
    for i in range(-(-M // Bc)):
        out = b.run({k: v[i * Bc:(i + 1) * Bc] for k, v in data.items()})
        for key in ((0, 0), (1, 1)):
            want[key].append(out["latent"][key].clone())
        want["recon"].append(out["recon"].clone())
    for run in range(2):
        out = runner.run_epoch()
        lat = out["collected"]["latent"]
        assert set(lat) == {(0, 0), (1, 1)} and out["steps"] == -(-M // Bc)
        for key in ((0, 0), (1, 1)):
            assert tuple(lat[key].shape) == (2, M) + tuple(a.lat_s.shape[2:] if key == (0, 0) else a.lat_v.shape[2:])
            assert torch.equal(lat[key], torch.cat(want[key], dim=1)), f"run {run}: latent {key}"
            lat[key].fill_(float("nan"))         # the second epoch has to write every row again
        assert torch.equal(out["collected"]["recon"], torch.cat(want["recon"]))
        out["collected"]["recon"].fill_(float("nan"))


def test_latent_refusals():
    from lgn.epoch import DeviceDataset, EpochRunner
    from lgn.step import NativeEvalStep, NativeTrainStep
    p4, _ = E._train_data(False)
    ds = DeviceDataset({"p4": p4}, shuffle=False)
    (ea, da), (eb, db) = E._pairs()
    with pytest.raises(ValueError, match="keep_latent=True"):
        EpochRunner(NativeEvalStep(ea, da, batch_size=B), ds, collect=("latent",))
    step = NativeTrainStep(eb, db, batch_size=B)
    with pytest.raises(ValueError, match="a training step keeps no latent"):
        EpochRunner(step, ds, collect=("latent",))
    with pytest.raises(ValueError, match="batch axis does not lead"):
        EpochRunner(step, ds, collect=("recon",), remainder="short")
    ev = NativeEvalStep(ea, da, batch_size=B, keep_latent=True, normalize=True)
    with pytest.raises(ValueError, match="'latent' counts as two"):
        EpochRunner(ev, ds, collect=("latent", "recon", "target", "norm_factor"))
    with pytest.raises(ValueError, match="'pad'"):
        EpochRunner(ev, ds, remainder="short")
