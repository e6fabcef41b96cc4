"""GPU tests of the device-resident epochs: lgn_stage_gather_f64 against lgn_stage_batch_f64 on the indexed jets (every output, bit
for bit), the out-of-range index, and lgn.epoch.EpochRunner against the host loop over the same batches -- parameters, optimiser
state, loss sum and collected tensors with torch.equal: the epoch runs the kernels the loop runs, on the same inputs, in the same
order, and sums the losses in the same order, so nothing is left to a tolerance."""
import functools

import pytest
import torch

import _normalize_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
M, B = 10, 4                      # three batches: 4, 4 and a short one of 2
CODES = {"none": 0, "component_max": 1, "overall_max": 2, "jet_E": 3}
VARIANTS = {"plain": {}, "labels": dict(labels=True), "jet_scalars": dict(jet=True, K=2, labels=True, scale=0.5),
            "scaled": dict(scale=0.25), "aliased": dict(alias=True)}


@functools.lru_cache(maxsize=None)
def _data(N):
    """(p4 (M, N, 4), labels (M, N), scalars (M, N + 1, 2)) on the device, shared and never modified."""
    p4 = R.jets(M, N, seed=100 + N, n_real=N - N // 3 if N > 2 else None)
    g = torch.Generator().manual_seed(200 + N)
    labels = (torch.rand(M, N, generator=g) < 0.7).to(torch.uint8)
    scalars = torch.randn(M, N + 1, 2, generator=g, dtype=torch.float64)
    return p4.to(DEV), labels.to(DEV), scalars.to(DEV)


def _buffers(N, jet, K, alias):
    """NaN-filled (mask: 255) outputs of a staging call: p4_in, target, mask, in_scalars, factor."""
    nan = lambda *s: torch.full(s, float("nan"), device=DEV, dtype=torch.float64)      # noqa: E731
    Nn = N + int(jet)
    target = nan(B, N, 4)
    return (target if alias else nan(B, Nn, 4), target, torch.full((B, Nn), 255, device=DEV, dtype=torch.uint8),
            nan(B, Nn, int(jet) + K) if jet or K else None, nan(B, 4))


def _gather(p4, labels, scalars, index, cursor, code, scale, jet, K, alias, count=None):
    """The raw native call at a cursor written from the host.  Returns (outputs, status)."""
    from lgn import _native as N_
    out = _buffers(p4.shape[1], jet, K, alias)
    cur = torch.tensor([cursor, 0], device=DEV, dtype=torch.int64)
    status = torch.zeros(1, device=DEV, dtype=torch.int32)
    count = index.numel() if count is None else count
    N_._check(N_.lib().lgn_stage_gather_f64(N_.ptr(p4), N_.ptr(labels), N_.ptr(scalars), p4.shape[0], N_.ptr(index), count, N_.ptr(cur),
                                            B, p4.shape[1], code, scale, int(jet), K, *[N_.ptr(t) for t in out], N_.ptr(status),
                                            N_.stream_ptr()), "lgn_stage_gather_f64")
    torch.cuda.synchronize()
    assert cur.tolist() == [cursor, 0], "the staging reads the cursor, it does not move it"
    return out, int(status.item())


def _staged(p4, labels, scalars, rows, code, scale, jet, K, alias):
    """lgn_stage_batch_f64 on the jets `rows` (a short batch is padded to B)."""
    from lgn import ops
    out = _buffers(p4.shape[1], jet, K, alias)
    rows = rows.long()
    ops.stage_batch(p4[rows], code, out[0], out[1], out[2], out[4], out[3], labels=None if labels is None else labels[rows],
                    scalars=None if scalars is None else scalars[rows], scale=scale, jet_features=jet)
    torch.cuda.synchronize()
    return out


def _same(got, want, what):
    for name, g, w in zip(("p4_in", "target", "mask", "in_scalars", "factor"), got, want):
        assert (g is None) == (w is None)
        if g is not None:
            assert torch.equal(g, w), f"{what}: {name} differs from lgn_stage_batch_f64 on the indexed jets"


@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("method", list(CODES))
@pytest.mark.parametrize("N", [1, 6, 70])
def test_gather_staging_is_the_batch_staging_of_the_indexed_jets(N, method, variant):
    v = VARIANTS[variant]
    jet, K, scale, alias = v.get("jet", False), v.get("K", 0), v.get("scale", 1.0), v.get("alias", False)
    p4, labels, scalars = _data(N)
    labels = labels if v.get("labels") else None
    scalars = scalars if K else None
    g = torch.Generator().manual_seed(N)
    shuffled = torch.randperm(M, generator=g).to(torch.int32).to(DEV)
    repeated = torch.tensor([7, 7, 0, 3, 3, 3, 9, 0, 7, 1], dtype=torch.int32, device=DEV)
    for kind, index in (("shuffled", shuffled), ("repeated", repeated)):
        for cursor in (0, 1, 2):
            rows = index[cursor * B:(cursor + 1) * B]
            got, status = _gather(p4, labels, scalars, index, cursor, CODES[method], scale, jet, K, alias)
            _same(got, _staged(p4, labels, scalars, rows, CODES[method], scale, jet, K, alias), f"{kind} index, cursor {cursor}")
            assert status == 0
            if cursor == 2:              # the short batch: rows 2 and 3 are padding jets
                assert rows.numel() == 2
                for t in got:
                    assert t is None or bool((t[2:] == 0).all()), "padding jets must be written as exact zeros"
    got, status = _gather(p4, labels, scalars, shuffled, 3, CODES[method], scale, jet, K, alias)       # behind the epoch: padding only
    assert status == 0 and all(t is None or bool((t == 0).all()) for t in got)


@pytest.mark.parametrize("method", ["none", "overall_max"])
def test_an_index_outside_the_dataset_is_a_padding_jet_and_sets_status(method):
    p4, labels, _ = _data(6)
    index = torch.tensor([0, -1, 2, M, 4, 5, 6, 7, 8, 9], dtype=torch.int32, device=DEV)
    got, status = _gather(p4, labels, None, index, 0, CODES[method], 1.0, False, 0, False)
    assert status == 1
    want = _staged(p4, labels, None, torch.tensor([0, 2], device=DEV), CODES[method], 1.0, False, 0, False)
    for g, w in zip(got, want):
        if g is not None:
            assert torch.equal(g[0], w[0]) and torch.equal(g[2], w[1]), "the rows beside a bad index are unaffected"
            assert bool((g[1] == 0).all()) and bool((g[3] == 0).all()), "a row with a bad index is a padding jet"
    got, status = _gather(p4, labels, None, index, 1, CODES[method], 1.0, False, 0, False)
    assert status == 0
    _same(got, _staged(p4, labels, None, index[4:8], CODES[method], 1.0, False, 0, False), "the batch behind the bad indices")


# ---- the runner ---------------------------------------------------------------------------------------------------------------
N_STEP = 6
CH = ((2, 2, 2), (2, 2, 2))        # maxdim 2, two channels, two levels


def _pairs(n=2, seed=23):
    """n pairs of networks on identical initial weights."""
    import __graft_entry__ as G
    return [G._models(N_STEP, CH[0], CH[1], torch.device(DEV), seed=seed, maxdim=2) for _ in range(n)]


def _train_data(normalize):
    p4, labels, _ = _data(N_STEP)
    if not normalize:              # (a plain step is fed normalised jets, as bench.py feeds them)
        p4 = p4 / (p4.abs().amax(dim=(1, 2), keepdim=True) + 1e-16)
    return p4.contiguous(), labels


TRAIN_CASES = {"adam_chamfer": dict(), "rmsprop_hungarian_normalize": dict(normalize=True, loss_choice="hungarian",
                                                                           optimizer_choice="rmsprop")}


@pytest.mark.parametrize("use_graph", [True, False], ids=["graph", "eager"])
@pytest.mark.parametrize("case", list(TRAIN_CASES))
def test_training_epochs_are_the_host_loop(case, use_graph):
    """Two epochs, reshuffled from a seeded generator, the short batch dropped: parameters, both optimiser state tensors, the step
    counter and each epoch's loss sum are the host loop's over p4[idx[i B:(i + 1) B]].  use_graph=False: the eager fallback (gather
    and collect launched around step.step(None)) gives the same."""
    from lgn.epoch import DeviceDataset, EpochRunner
    from lgn.step import NativeTrainStep
    kw = TRAIN_CASES[case]
    p4, labels = _train_data(kw.get("normalize", False))
    data = {"p4": p4, "labels": labels} if kw else {"p4": p4}
    (ea, da), (eb, db) = _pairs()
    a = NativeTrainStep(ea, da, batch_size=B, lr=1e-3, use_graph=use_graph, **kw)
    b = NativeTrainStep(eb, db, batch_size=B, lr=1e-3, **kw)
    runner = EpochRunner(a, DeviceDataset(data, shuffle=False), shuffle=True, generator=torch.Generator().manual_seed(5),
                         collect=("target", "norm_factor"), remainder="drop")
    assert runner.single_graph == use_graph
    epochs = []
    for _ in range(2):
        out = runner.run_epoch()
        assert out["steps"] == 2 and out["status"] == 0 and out["avg_loss"] == out["loss_sum"] / 2
        assert runner.launches_per_epoch == (2 if use_graph else 6)
        epochs.append((runner.index.clone(), out["loss_sum"], {k: v.clone() for k, v in out["collected"].items()}))
    g = torch.Generator().manual_seed(5)
    for index, loss_sum, collected in epochs:
        assert torch.equal(index.cpu(), torch.randperm(M, generator=g).to(torch.int32))
        losses, targets, factors = [], [], []
        for i in range(2):
            rows = index[i * B:(i + 1) * B].long()
            loss, _ = b.step({k: v[rows] for k, v in data.items()})
            losses.append(loss.item())
            targets.append(b.target.clone())
            factors.append(b.norm_factor.clone())
        print(f"{case}: epoch loss sum {loss_sum!r}, host loop {sum(losses)!r}")
        assert loss_sum == sum(losses)
        assert tuple(collected["target"].shape) == (8, N_STEP, 4)
        assert torch.equal(collected["target"], torch.cat(targets)) and torch.equal(collected["norm_factor"], torch.cat(factors))
    assert torch.equal(a.flat.flat, b.flat.flat), "parameters"
    assert torch.equal(a.adam_m, b.adam_m) and torch.equal(a.adam_v, b.adam_v), "optimiser state"
    assert torch.equal(a.step_dev, b.step_dev) and int(a.step_dev.item()) == 4


def test_training_runner_refusals():
    from lgn.epoch import DeviceDataset, EpochRunner
    from lgn.step import NativeTrainStep
    p4, _ = _train_data(False)
    ((enc, dec),) = _pairs(1)
    step = NativeTrainStep(enc, dec, batch_size=B)
    ds = DeviceDataset({"p4": p4}, shuffle=False)
    with pytest.raises(ValueError, match="2 left over"):
        EpochRunner(step, ds, remainder="error")
    with pytest.raises(ValueError, match="whole batches only"):
        EpochRunner(step, ds, remainder="pad")
    with pytest.raises(ValueError, match="batch axis does not lead"):
        EpochRunner(step, ds, collect=("recon",))
    with pytest.raises(ValueError, match="need normalize"):
        EpochRunner(step, ds, collect=("target_denorm",))
    with pytest.raises(ValueError, match=r"outside \[0, 10\)"):
        EpochRunner(step, ds, index=torch.arange(1, 11))
    with pytest.raises(ValueError, match="the dataset holds"):
        EpochRunner(step, DeviceDataset({"p4": _data(70)[0]}, shuffle=False))


EVAL_CASES = {"chamfer": dict(), "chamfer_normalize": dict(normalize=True, normalize_method="component_max"),
              "hungarian_normalize": dict(normalize=True, loss_choice="hungarian")}


@pytest.mark.parametrize("case", list(EVAL_CASES))
def test_evaluation_epoch_is_the_host_loop_and_runs_twice(case):
    """M = 10 in batches of 4: the short batch is padded, the collected rows cover all 10 jets and are the concatenation of
    step.run(batch) outputs cut to each batch's real jets; a second run_epoch() reproduces the first (cursor and sums are reset).
    With a mean-reduced loss the short batch is a call of its own descriptors around eager gather and collect launches."""
    from lgn.epoch import DeviceDataset, EpochRunner
    from lgn.step import NativeEvalStep
    kw = EVAL_CASES[case]
    normalize = kw.get("normalize", False)
    p4, labels = _train_data(normalize)
    (ea, da), (eb, db) = _pairs()
    a = NativeEvalStep(ea, da, batch_size=B, **kw)
    b = NativeEvalStep(eb, db, batch_size=B, **kw)
    names = ("recon", "target", "norm_factor") + (("recon_denorm",) if normalize else ())
    runner = EpochRunner(a, DeviceDataset({"p4": p4, "labels": labels}, shuffle=False), shuffle=False, collect=names)
    want, losses = {k: [] for k in names}, []
    for i in range(3):
        out = b.run({"p4": p4[i * B:(i + 1) * B], "labels": labels[i * B:(i + 1) * B]})
        n = out["recon"].shape[0]
        losses.append(out["loss"].item())
        want["recon"].append(out["recon"].clone())
        want["target"].append(b.target[:n].clone())
        want["norm_factor"].append(b.norm_factor[:n].clone())
        if normalize:
            want["recon_denorm"].append(out["recon_denorm"].clone())
    assert [w.shape[0] for w in want["recon"]] == [4, 4, 2]
    for run in range(2):
        out = runner.run_epoch()
        print(f"{case} run {run}: epoch loss sum {out['loss_sum']!r}, host loop {sum(losses)!r}")
        assert out["steps"] == 3 and out["status"] == 0
        assert out["loss_sum"] == sum(losses) and out["avg_loss"] == sum(losses) / 3
        assert runner.launches_per_epoch == (5 if "hungarian" in case else 3)
        for k in names:
            assert out["collected"][k].shape[0] == M
            assert torch.equal(out["collected"][k], torch.cat(want[k])), f"run {run}: collected {k}"
        for v in out["collected"].values():
            v.fill_(float("nan"))            # the second epoch has to write every row again
    assert a.n_real == 2
