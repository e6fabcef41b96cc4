"""Bit-for-bit pins of the step classes' plumbing (lgn/step.py): the paths tests/golden/dead_cgmlp_step_bits.json does not reach --
the loss descriptor of the whole-step calls (mse / Hungarian), the eager step, the two-call data-parallel form between two graphs,
the split staging of a jet_features encoder, CapturedModuleStep under autograd, and the evaluation step on a short last batch.
tests/golden/step_plumbing_bits.json holds the sha256 hashes these runs gave while every whole-step call still had a `_loss` twin
and each step class staged, snapshotted and finalised with code of its own; each case gave the same hashes in two runs."""
import hashlib
import json
import os

import pytest
import torch

import _util as U

# The hashes of the cases that run the encoder's input stage were recorded again when its mass stopped being contracted into fused
# multiply-adds (minkowski_sq_unfused, csrc/common.hpp: the reference's arithmetic); each case gave the same hashes in two runs.
# In the two mse cases only `recon` got a new hash: `grad`, the moments and the weights gave their recorded hashes again, in both runs.
pytestmark = pytest.mark.gpu

DEV = "cuda:0"
CH = ((3, 3, 4, 4), (4, 4, 3, 3))
REL_POLAR = dict(hungarian_abs_coord=False, hungarian_polar_coord=True)
# id -> (jets, particles, step options)
TRAIN_CASES = {
    "64x30:mse:graph": (64, 30, dict(loss_choice="mse", use_graph=True)),
    "64x30:mse:eager": (64, 30, dict(loss_choice="mse", use_graph=False)),
    "64x30:hungarian:abs_cart": (64, 30, dict(loss_choice="hungarian", use_graph=True)),
    "7x30:hungarian:rel_polar": (7, 30, dict(loss_choice="hungarian", use_graph=True, **REL_POLAR)),
    "64x30:two_call": (64, 30, dict(force_collective=True, graph_collective=False, use_graph=True)),
    "7x30:split": (7, 30, dict(chamfer_jet_features=True, get_real_method="real", use_graph=True)),
    "7x30:captured_sum": (7, 30, dict(use_graph=True)),
}
# id -> (batch size of the step, jets of the short batch, step options)
EVAL_CASES = {
    "eval:5of7x30:jet_features": (7, 5, dict(chamfer_jet_features=True)),
    "eval:5of7x30:hungarian": (7, 5, dict(loss_choice="hungarian")),
}


def _batch(B, N):
    from oracle import lgn_oracle as O
    p4, labels = O.synthetic_jets(B, N, seed=B + N, pad=True)
    return {"p4": p4.to(DEV), "labels": labels.to(DEV)}


def _sha(bufs):
    import numpy as np
    torch.cuda.synchronize()
    return {k: hashlib.sha256(np.ascontiguousarray(v.detach().cpu().numpy()).tobytes()).hexdigest() for k, v in bufs.items()}


def _one_rank_group():
    import socket
    import torch.distributed as dist
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))


def train_bits(case):
    """sha256 of every buffer a training step leaves behind after four Adam steps (as step_bits() of test_gpu_dead_cgmlp.py), with the
    assignment and its status where the loss has them."""
    import torch.distributed as dist
    import __graft_entry__ as G
    from lgn.step import CapturedModuleStep, NativeTrainStep
    B, N, opts = TRAIN_CASES[case]
    kind = case.split(":")[1]
    cls, net = NativeTrainStep, {}
    if kind == "split":
        net = dict(jet_features=True)
    elif kind == "captured_sum":
        cls, net = CapturedModuleStep, dict(map_to_latent="sum")
    enc, dec = G._models(N, *CH, torch.device(DEV), seed=11, **net)
    batch = _batch(B, N)
    if kind == "two_call":
        _one_rank_group()
    try:
        st = cls(enc, dec, batch_size=B, lr=1e-3, l1_lambda=1e-6, **opts)
        losses = torch.stack([st.step(batch)[0].clone() for _ in range(4)])
        torch.cuda.synchronize()
        if kind == "two_call":
            assert st._g2 is not None and st.launches_per_step == 3
        if kind == "split":
            assert st.split
        bufs = {"losses": losses, "loss_out": st.loss_out, "grad": st.flat.grad, "adam_m": st.adam_m, "adam_v": st.adam_v,
                "weights": st.flat.flat, "step": st.step_dev, "recon": st.recon, "loss_part": st.loss_part}
        if getattr(st, "assignment", None) is not None:
            bufs.update(assignment=st.assignment, status=st.status)
        return _sha(bufs)
    finally:
        if kind == "two_call":
            dist.destroy_process_group()


def eval_bits(case):
    """sha256 of what the evaluation step returns for a full batch (the captured graph) and then for a short one (the call of its
    own with the mean over the B' real jets)."""
    import __graft_entry__ as G
    from lgn.step import NativeEvalStep
    B, n, opts = EVAL_CASES[case]
    enc, dec = G._models(30, *CH, torch.device(DEV), seed=11)
    batch = _batch(B, 30)
    ev = NativeEvalStep(enc, dec, B, get_real_method="real", **opts)
    bufs = {"loss_full": ev.run(batch)["loss"].clone()}
    out = ev.run({k: v[:n] for k, v in batch.items()})
    assert ev.n_real == n and out["recon"].shape[0] == n
    bufs.update(loss=out["loss"], recon=out["recon"])
    if ev.assignment is not None:
        bufs.update(assignment=ev.assignment[:n], status=ev.status[:n])
    return _sha(bufs)


def _golden(case):
    with open(os.path.join(U.GOLDEN, "step_plumbing_bits.json")) as f:
        return json.load(f)[case]


@pytest.mark.parametrize("case", list(TRAIN_CASES))
def test_training_steps_keep_their_bits(case):
    ref, got = _golden(case), train_bits(case)
    assert set(ref) == set(got)
    bad = [k for k in ref if got[k] != ref[k]]
    assert not bad, f"differ bit for bit from the recorded step: {bad}"


@pytest.mark.parametrize("case", list(EVAL_CASES))
def test_short_batch_evaluation_keeps_its_bits(case):
    ref, got = _golden(case), eval_bits(case)
    assert set(ref) == set(got)
    bad = [k for k in ref if got[k] != ref[k]]
    assert not bad, f"differ bit for bit from the recorded evaluation step: {bad}"
