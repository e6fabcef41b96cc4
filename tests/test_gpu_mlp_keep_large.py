"""GPU tests of the kept CGMLP activations at large batches.  From 8 129 rows on the CGMLP runs 64-row workgroups; a training step
whose descriptor carries LGN_NET_MLP_KEEP (the default) has the two-role forward store the six hidden activations of every CGMLP
and the two-role backward read them back instead of recomputing them at its head.  LGN_AMD_MLP_RECOMPUTE=1 clears the bit: the
step of before, which recomputes.  The kept value is the register the forward computed and the recomputed one comes from the same
layer function on the same inputs, so every buffer a training step leaves behind must be the same bits either way.

Shape: cfg2's networks (enc 3-3-4-4, dec 4-4-3-3: CGMLPs of H = 36, thin last tile, and H = 48) on jets of 30 particles.  271 jets
are 8 130 rows = 128 tiles of 64, the smallest batch that runs the 64-row kernels, with 2 live rows in the last tile; 300 jets
leave 40 live rows (three waves of the last workgroup with rows, the third half full, the fourth without).  Further cases: the
full-tile form of H = 36 (LGN_AMD_MLP_FULLTILE=1) and a non-default activation (the kernels that derive the slope from the kept
value through the activation switch).  The 16-row kernels and their copy are untouched."""
import hashlib

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
CH = ((3, 3, 4, 4), (4, 4, 3, 3))
N = 30
SWITCH = "LGN_AMD_MLP_RECOMPUTE"
BIT = 8192                               # LGN_NET_MLP_KEEP (include/lgn_amd.h)

# id -> (jets, activation, further environment switches)
CASES = {
    "271": (271, "leakyrelu", {}),
    "300": (300, "leakyrelu", {}),
    "271:fulltile": (271, "leakyrelu", {"LGN_AMD_MLP_FULLTILE": "1"}),
    "271:elu": (271, "elu", {}),
}


def _batch(B):
    from oracle import lgn_oracle as O
    p4, labels = O.synthetic_jets(B, N, seed=B + N, pad=True)
    return {"p4": p4.to(DEV), "labels": labels.to(DEV)}


def _bits(monkeypatch, recompute, B, act, env):
    """sha256 of what two optimiser steps leave behind.  The switches are frozen into the descriptor when the step is built."""
    import __graft_entry__ as G
    from lgn.step import NativeTrainStep
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    if recompute:
        monkeypatch.setenv(SWITCH, "1")
    else:
        monkeypatch.delenv(SWITCH, raising=False)
    enc, dec = G._models(N, *CH, torch.device(DEV), seed=11, activation=act)
    st = NativeTrainStep(enc, dec, batch_size=B, lr=1e-3, l1_lambda=1e-6, use_graph=False)
    assert bool(st.desc.flags & BIT) == (not recompute)
    for k in env:
        assert st.desc.flags & {"LGN_AMD_MLP_FULLTILE": 2048}[k]
    batch = _batch(B)
    losses = torch.stack([st.step(batch)[0].clone() for _ in range(2)])
    torch.cuda.synchronize()
    bufs = {"losses": losses, "loss_out": st.loss_out, "grad": st.flat.grad, "adam_m": st.adam_m, "adam_v": st.adam_v,
            "weights": st.flat.flat, "recon": st.recon}
    for k, v in bufs.items():
        assert torch.isfinite(v).all(), k
    assert torch.count_nonzero(st.flat.grad) > 0
    return {k: hashlib.sha256(np.ascontiguousarray(v.detach().cpu().numpy()).tobytes()).hexdigest() for k, v in bufs.items()}


@pytest.mark.parametrize("case", list(CASES))
def test_kept_activations_give_the_bits_of_the_recomputed_ones(monkeypatch, case):
    B, act, env = CASES[case]
    assert (B * N + 63) // 64 >= 128, "the 64-row regime"
    kept = _bits(monkeypatch, False, B, act, env)
    recomputed = _bits(monkeypatch, True, B, act, env)
    bad = [k for k in kept if kept[k] != recomputed[k]]
    assert not bad, f"differ bit for bit from the step that recomputes the activations: {bad}"
