"""GPU tests of the separable decoder levels that keep their jet sums instead of the aggregate.  In the sequencers (whole step, whole
network) a decoder level of jets of <= 40 particles stores the 20 C sums and eight means of each jet; its backward rebuilds the rows
of the aggregate from them with the forward's own row function instead of reading ag0 / ag1 back.  LGN_AMD_DEC_STORE_AG=1 keeps the
stored aggregate -- the step the pinned hashes of test_gpu_dead_cgmlp.py and test_gpu_pair_sweep_bits.py hold in place: every buffer
a training step leaves behind must be the same bits either way.

Shapes: 9 particles (a padded last group of four), 30, and 40 (N * 2C exceeds one workgroup's staging items: the remainder loops);
2 and 257 jets.  (launch_level_fwd2 gives a jet eight waves only for N >= 64, outside the range that rebuilds: every case here runs
the four-wave launch, at a grid below and above one workgroup per CU.)  41 particles take the kernels that read the stored aggregate
whatever the switch says."""
import hashlib

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
CH = ((3, 3, 4, 4), (4, 4, 3, 3))        # decoder levels with C = 4, 4, 3; the last one without live scalars
SWITCH = "LGN_AMD_DEC_STORE_AG"
BIT = 16384                              # LVL_DEC_STORE_AG (csrc/level.hpp)

# (jets, particles, map_to_latent, get_real method, graph)
CASES = [(B, N, "min&max", "sum", B == 257) for N in (9, 30, 40) for B in (2, 257)] + [(7, 30, "mix", "real", False)]


def _batch(B, N):
    from oracle import lgn_oracle as O
    p4, labels = O.synthetic_jets(B, N, seed=B + N, pad=True)
    return {"p4": p4.to(DEV), "labels": labels.to(DEV)}


def _bits(monkeypatch, stored, B, N, pool, method, graph):
    """sha256 of what two optimiser steps leave behind (the buffers step_bits of test_gpu_dead_cgmlp.py hashes).  The switch is
    frozen into the descriptor when the step is built."""
    import __graft_entry__ as G
    from lgn.step import NativeEvalStep, NativeTrainStep
    if stored:
        monkeypatch.setenv(SWITCH, "1")
    else:
        monkeypatch.delenv(SWITCH, raising=False)
    enc, dec = G._models(N, *CH, torch.device(DEV), seed=11, map_to_latent=pool)
    st = NativeTrainStep(enc, dec, batch_size=B, lr=1e-3, l1_lambda=1e-6, use_graph=graph, get_real_method=method)
    assert bool(st.desc.flags & BIT) == stored
    batch = _batch(B, N)
    losses = torch.stack([st.step(batch)[0].clone() for _ in range(2)])
    lat = NativeEvalStep(enc, dec, B, get_real_method=method, keep_latent=True).run(batch)["latent"]
    torch.cuda.synchronize()
    bufs = {"losses": losses, "loss_out": st.loss_out, "grad": st.flat.grad, "adam_m": st.adam_m, "adam_v": st.adam_v,
            "weights": st.flat.flat, "recon": st.recon, "latent_s": lat[(0, 0)], "latent_v": lat[(1, 1)]}
    for k, v in bufs.items():
        assert torch.isfinite(v).all(), k
    assert torch.count_nonzero(st.flat.grad) > 0
    return {k: hashlib.sha256(np.ascontiguousarray(v.detach().cpu().numpy()).tobytes()).hexdigest() for k, v in bufs.items()}


@pytest.mark.parametrize("B,N,pool,method,graph", CASES)
def test_rebuilt_aggregate_gives_the_bits_of_the_stored_one(monkeypatch, B, N, pool, method, graph):
    new = _bits(monkeypatch, False, B, N, pool, method, graph)
    old = _bits(monkeypatch, True, B, N, pool, method, graph)
    bad = [k for k in old if new[k] != old[k]]
    assert not bad, f"differ bit for bit from the step that stores the aggregate: {bad}"


def test_jets_of_41_particles_keep_the_stored_aggregate(monkeypatch):
    """N > 40: the three-kernel backward reads ag0 / ag1; the sequencer leaves sep_sums null and the switch changes nothing."""
    new = _bits(monkeypatch, False, 3, 41, "min&max", "sum", False)
    old = _bits(monkeypatch, True, 3, 41, "min&max", "sum", False)
    assert new == old
