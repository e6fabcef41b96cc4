"""Bit-for-bit pins of the host sequencer (csrc/step.hip) on the paths tests/golden/dead_cgmlp_step_bits.json and
tests/golden/step_plumbing_bits.json do not reach, in the manner of test_gpu_step_plumbing_bits.py: the table-driven (maxdim 3)
step with its static kernels, with run-time tables (the branch of the step that hands nothing over to one closing launch) and with
the unfused decoder levels, the per-network table-driven calls under CapturedModuleStep, the table-driven evaluation step; the
maxdim-2 step past 40 particles (three-kernel level backward: the encoder's input stage backward as a launch of its own, no riding
loss), its per-network calls and its evaluation step with the latent kept; the per-network calls with two input scalars
(jet_features); and the step that closes with three launches (LGN_AMD_SPLIT_TAIL).  tests/golden/sequencer_bits.json holds the
sha256 hashes these runs gave while the maxdim-2 end-stage sequences were still written out per caller; each case gave the same
hashes in two runs."""
import hashlib
import json
import os

import pytest
import torch

import _util as U

# The hashes of the cases that run the encoder's input stage were recorded again when its mass stopped being contracted into fused
# multiply-adds (minkowski_sq_unfused, csrc/common.hpp: the reference's arithmetic); each case gave the same hashes in two runs.
pytestmark = pytest.mark.gpu

DEV = "cuda:0"
CH2 = ((3, 3, 4, 4), (4, 4, 3, 3))
CH3 = ((3, 4, 4), (4, 4, 3))       # (a channel set of test_gpu_step.py's maxdim-3 steps on the static kernels)
# id -> (maxdim, jets, particles, step class, model options, switches set while the step is built and run)
TRAIN_CASES = {
    "md3:7x13:native": (3, 7, 13, "NativeTrainStep", {}, ()),
    "md3:7x13:no_static": (3, 7, 13, "NativeTrainStep", {}, ("LGN_AMD_NO_STATIC",)),
    "md3:7x13:dec_unfused": (3, 7, 13, "NativeTrainStep", {}, ("LGN_AMD_DEC_UNFUSED",)),
    "md3:7x13:captured": (3, 7, 13, "CapturedModuleStep", {}, ()),
    "md2:3x41:native": (2, 3, 41, "NativeTrainStep", {}, ()),
    "md2:3x41:captured": (2, 3, 41, "CapturedModuleStep", {}, ()),
    "md2:7x30:jet_features:captured": (2, 7, 30, "CapturedModuleStep", dict(jet_features=True), ()),
    "md2:64x30:split_tail": (2, 64, 30, "NativeTrainStep", {}, ("LGN_AMD_SPLIT_TAIL",)),
}
# id -> (maxdim, batch size of the step, jets of the short batch, particles, step options)
EVAL_CASES = {
    "md3:eval:5of7x13": (3, 7, 5, 13, {}),
    "md2:eval:2of3x41:keep_latent": (2, 3, 2, 41, dict(keep_latent=True)),
}


def _models(maxdim, N, **net):
    import __graft_entry__ as G
    return G._models(N, *(CH3 if maxdim == 3 else CH2), torch.device(DEV), seed=11, maxdim=maxdim, **net)


def _batch(B, N):
    from oracle import lgn_oracle as O
    p4, labels = O.synthetic_jets(B, N, seed=B + N, pad=True)
    return {"p4": p4.to(DEV), "labels": labels.to(DEV)}


def _sha(bufs):
    import numpy as np
    torch.cuda.synchronize()
    return {k: hashlib.sha256(np.ascontiguousarray(v.detach().cpu().numpy()).tobytes()).hexdigest() for k, v in bufs.items()}


def train_bits(case, setenv):
    """sha256 of every buffer a training step leaves behind after four Adam steps (as train_bits() of
    test_gpu_step_plumbing_bits.py).  setenv(name, value) sets a switch for the rest of the test."""
    import lgn.step as S
    maxdim, B, N, cls, net, switches = TRAIN_CASES[case]
    for name in switches:
        setenv(name, "1")
    enc, dec = _models(maxdim, N, **net)
    batch = _batch(B, N)
    st = getattr(S, cls)(enc, dec, batch_size=B, lr=1e-3, l1_lambda=1e-6, use_graph=True)
    losses = torch.stack([st.step(batch)[0].clone() for _ in range(4)])
    torch.cuda.synchronize()
    return _sha({"losses": losses, "loss_out": st.loss_out, "grad": st.flat.grad, "adam_m": st.adam_m, "adam_v": st.adam_v,
                 "weights": st.flat.flat, "step": st.step_dev, "recon": st.recon, "loss_part": st.loss_part})


def eval_bits(case):
    """sha256 of what the evaluation step returns for a full batch (the captured graph) and then for a short one."""
    from lgn.step import NativeEvalStep
    maxdim, B, n, N, opts = EVAL_CASES[case]
    enc, dec = _models(maxdim, N)
    batch = _batch(B, N)
    ev = NativeEvalStep(enc, dec, B, get_real_method="real", **opts)
    full = ev.run(batch)
    bufs = {"loss_full": full["loss"].clone(), "recon_full": full["recon"].clone()}
    if opts.get("keep_latent"):
        bufs.update(lat_s_full=full["latent"][(0, 0)].clone(), lat_v_full=full["latent"][(1, 1)].clone())
    out = ev.run({k: v[:n] for k, v in batch.items()})
    assert ev.n_real == n and out["recon"].shape[0] == n
    bufs.update(loss=out["loss"], recon=out["recon"])
    if opts.get("keep_latent"):
        bufs.update(lat_s=out["latent"][(0, 0)], lat_v=out["latent"][(1, 1)])
    return _sha(bufs)


def _golden(case):
    with open(os.path.join(U.GOLDEN, "sequencer_bits.json")) as f:
        return json.load(f)[case]


@pytest.mark.parametrize("case", list(TRAIN_CASES))
def test_training_steps_keep_their_bits(case, monkeypatch):
    ref, got = _golden(case), train_bits(case, monkeypatch.setenv)
    assert set(ref) == set(got)
    bad = [k for k in ref if got[k] != ref[k]]
    assert not bad, f"differ bit for bit from the recorded step: {bad}"


@pytest.mark.parametrize("case", list(EVAL_CASES))
def test_evaluation_steps_keep_their_bits(case):
    ref, got = _golden(case), eval_bits(case)
    assert set(ref) == set(got)
    bad = [k for k in ref if got[k] != ref[k]]
    assert not bad, f"differ bit for bit from the recorded evaluation step: {bad}"
