"""GPU tests of device-resident epochs of a guarded training step (lgn.epoch.EpochRunner on a NativeTrainStep built with
max_grad_norm / skip_nonfinite / lr_schedule): the epoch is the same steps driven one by one, bit for bit, and an epoch with one
poisoned jet loses exactly that step -- where the default step ends with non-finite parameters.  The poisoned jet's values overflow
in plain arithmetic (Chamfer loss only: no kernel with a data-dependent loop sees them); nothing here touches an illegal address."""
import functools
import math

import pytest
import torch

from test_gpu_optimizer_options import LR, _setup

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
B, N_PART = 4, 30                # the g1 shape
FULL, SHORT = 5, 2


@functools.lru_cache(maxsize=None)
def _jets(M):
    """M padded jets of the g1 shape, normalised per jet as the fixture's are; shared, never modified."""
    from oracle import lgn_oracle as O
    p4, labels = O.synthetic_jets(M, N_PART, seed=41, pad=True)
    p4 = p4 / (p4.abs().amax(dim=(1, 2), keepdim=True) + 1e-16)
    return p4.contiguous().to(DEV), labels.to(torch.uint8).to(DEV)


def _models():
    m, enc, dec, _ = _setup()
    assert (m["B"], m["N"]) == (B, N_PART)
    return enc, dec


def test_controlled_epoch_is_the_same_steps_driven_one_by_one():
    """5 batches and a short last one (remainder='short') with clipping and the cosine schedule: parameters, optimiser state, the
    counter and the control block's running fields are torch.equal to step.step(batch) / short_step(2).step(batch) in a loop;
    control['applied'] is 6 and applied_loss_sum is loss_sum to the bit (both are one fp64 add per step, in step order)."""
    from lgn.epoch import DeviceDataset, EpochRunner
    from lgn.step import LRSchedule, NativeTrainStep
    p4, labels = _jets(FULL * B + SHORT)
    data = {"p4": p4, "labels": labels}
    probe = NativeTrainStep(*_models(), batch_size=B, lr=LR, optimizer=False, use_graph=False, skip_nonfinite=True)
    probe.step({k: v[:B] for k, v in data.items()})
    opts = dict(lr=LR, l1_lambda=1e-6, max_grad_norm=0.5 * float(probe.grad_norm),
                lr_schedule=LRSchedule("cosine", LR, warmup_steps=2, total_steps=5, min_lr=1e-5))
    a = NativeTrainStep(*_models(), batch_size=B, **opts)
    b = NativeTrainStep(*_models(), batch_size=B, **opts)
    runner = EpochRunner(a, DeviceDataset(data, shuffle=False), shuffle=False, remainder="short")
    out = runner.run_epoch()
    assert out["steps"] == FULL + 1 and out["status"] == 0 and runner.launches_per_epoch == FULL + 1
    losses = []
    for i in range(FULL):
        losses.append(b.step({k: v[i * B:(i + 1) * B] for k, v in data.items()})[0].item())
    losses.append(b.short_step(SHORT).step({k: v[FULL * B:] for k, v in data.items()})[0].item())
    torch.cuda.synchronize()
    assert torch.equal(a.flat.flat, b.flat.flat), "parameters"
    assert torch.equal(a.adam_m, b.adam_m) and torch.equal(a.adam_v, b.adam_v), "optimiser state"
    assert torch.equal(a.step_dev, b.step_dev) and int(a.step_dev.item()) == FULL + 1
    ctl = out["control"]
    assert ctl == b.control_stats(), (ctl, b.control_stats())
    assert ctl["applied"] == 6 and ctl["skipped"] == 0 and ctl["first_skipped"] == 0 and ctl["clipped"] >= 1
    assert out["loss_sum"] == sum(losses) and ctl["applied_loss_sum"] == out["loss_sum"]
    assert float(a.lr_used) == 1e-5              # step 6 > total_steps: held at min_lr
    out2 = runner.run_epoch()                    # the running fields start over with every epoch; the schedule goes on
    assert out2["control"]["applied"] == 6 and int(a.step_dev.item()) == 2 * (FULL + 1)
    assert set(out) - {"control"} == {"loss_sum", "steps", "avg_loss", "status", "collected"}


def test_an_epoch_with_one_poisoned_jet_skips_exactly_that_step():
    """One jet's p4 is multiplied by 1e200 (its squares overflow to Inf; Chamfer loss).  With skip_nonfinite=True exactly one step
    is skipped, first_skipped names it, and the final parameters are finite and torch.equal to an epoch over the dataset without
    that batch.  The same epoch on the default step ends with non-finite parameters."""
    from lgn.epoch import DeviceDataset, EpochRunner
    from lgn.step import NativeTrainStep
    p4, labels = _jets(FULL * B)
    bad_batch, bad_jet = 2, 2 * B + 1
    poisoned = p4.clone()
    poisoned[bad_jet] *= 1e200
    keep = torch.ones(FULL * B, dtype=torch.bool, device=DEV)
    keep[bad_batch * B:(bad_batch + 1) * B] = False
    opts = dict(lr=LR, l1_lambda=1e-6)
    guarded = NativeTrainStep(*_models(), batch_size=B, skip_nonfinite=True, **opts)
    out = EpochRunner(guarded, DeviceDataset({"p4": poisoned, "labels": labels}, shuffle=False), shuffle=False).run_epoch()
    ctl = out["control"]
    assert out["steps"] == FULL and ctl["skipped"] == 1 and ctl["applied"] == FULL - 1
    assert ctl["first_skipped"] == bad_batch + 1          # two steps were applied before it: it would have been step t = 3
    assert not math.isfinite(out["loss_sum"]) and math.isfinite(ctl["applied_loss_sum"]) and math.isfinite(ctl["grad_norm_max"])
    assert bool(torch.isfinite(guarded.flat.flat).all()) and int(guarded.step_dev.item()) == FULL - 1
    clean = NativeTrainStep(*_models(), batch_size=B, skip_nonfinite=True, **opts)
    out_c = EpochRunner(clean, DeviceDataset({"p4": p4[keep].contiguous(), "labels": labels[keep].contiguous()}, shuffle=False),
                        shuffle=False).run_epoch()
    assert out_c["control"]["skipped"] == 0 and out_c["control"]["applied"] == FULL - 1
    assert torch.equal(guarded.flat.flat, clean.flat.flat), "the skipped step left a trace in the parameters"
    assert torch.equal(guarded.adam_m, clean.adam_m) and torch.equal(guarded.adam_v, clean.adam_v)
    assert ctl["applied_loss_sum"] == out_c["control"]["applied_loss_sum"] == out_c["loss_sum"]
    default = NativeTrainStep(*_models(), batch_size=B, **opts)
    out_d = EpochRunner(default, DeviceDataset({"p4": poisoned, "labels": labels}, shuffle=False), shuffle=False).run_epoch()
    assert "control" not in out_d and not bool(torch.isfinite(default.flat.flat).all()), "the default step has no guard"
