"""GPU tests of the whole-network steps that skip the last CGMLP of each network when nothing reads its output: the training step
(which returns no latent scalars, and whose decoder never reads them) and the evaluation step without the latent.  The latent
vectors, their arg-indices, the loss, the reconstruction and every gradient must stay what the per-operator module path computes,
which runs both CGMLPs; the evaluation step that returns the latent must still return the encoder's latent scalars."""
import json
import os

import pytest
import torch

import _util as U

# The hashes of the cases that run the encoder's input stage were recorded again when its mass stopped being contracted into fused
# multiply-adds (minkowski_sq_unfused, csrc/common.hpp: the reference's arithmetic); each case gave the same hashes in two runs.
pytestmark = pytest.mark.gpu

DEV = "cuda:0"
CH = ((3, 3, 4, 4), (4, 4, 3, 3))
POOLS = ["min&max", "mean&max", "min+mean", "mix"]
# cfg2's 512 jets, the 64-jet launch geometry, a handful of jets, and the jet sizes that take the other level kernels
SIZES = [(512, 30), (64, 30), (7, 30), (5, 70), (3, 150)]
CASES = [(B, N, pool) for B, N in SIZES for pool in POOLS if not (pool == "mix" and N > 70)]


def _pair(N, pool, seed):
    import __graft_entry__ as G
    return [G._models(N, *CH, torch.device(DEV), seed=seed, map_to_latent=pool) for _ in range(2)]


def _batch(B, N):
    from oracle import lgn_oracle as O
    p4, labels = O.synthetic_jets(B, N, seed=B + N, pad=True)
    return {"p4": p4.to(DEV), "labels": labels.to(DEV)}


@pytest.mark.parametrize("B,N,pool", CASES)
def test_training_step_without_the_dead_cgmlps_matches_the_module_path(B, N, pool):
    """The native step (graph-replayed) against the module API with one native call per operator, both CGMLPs included."""
    from lgn.step import NativeTrainStep, TrainStep
    (enc, dec), (enc2, dec2) = _pair(N, pool, seed=7)
    for m in (enc2, dec2):
        m.use_fused = False
    method = "real" if B % 2 else "sum"
    batch = _batch(B, N)
    a = NativeTrainStep(enc, dec, batch_size=B, optimizer=False, use_graph=True, get_real_method=method)
    b = TrainStep(enc2, dec2, optimizer=False, get_real_method=method)
    a.step(batch)
    la, ra = a.step(batch)                  # (the replay)
    lb, rb = b.forward_backward(batch)
    U.assert_close(la, lb, 1e-12, "loss")
    U.assert_close(ra, rb, 1e-12, "recon")
    assert torch.isfinite(a.flat.grad).all()
    U.assert_close(a.flat.grad, b.flat.grad, 1e-9, "flat gradient")


@pytest.mark.parametrize("pool", POOLS)
@pytest.mark.parametrize("B,N", [(512, 30), (5, 70)])
def test_eval_step_latent_scalars_and_results_with_and_without_the_latent(B, N, pool):
    """With the latent requested the encoder's last CGMLP runs and the latent scalars are the module encoder's; without it the
    reconstruction and the loss are the same bits."""
    from lgn.step import NativeEvalStep
    (enc, dec), _ = _pair(N, pool, seed=3)
    batch = _batch(B, N)
    keep = NativeEvalStep(enc, dec, B, get_real_method="norm", keep_latent=True).run(batch)
    keep = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in keep.items()}
    bare = NativeEvalStep(enc, dec, B, get_real_method="norm").run(batch)
    assert torch.equal(keep["recon"], bare["recon"]) and torch.equal(keep["loss"], bare["loss"])
    with torch.no_grad():
        lat = enc(batch)
    for key in ((0, 0), (1, 1)):
        assert keep["latent"][key].shape == lat[key].shape
        U.assert_close(keep["latent"][key], lat[key], 1e-12, f"latent {key}")
        assert torch.count_nonzero(keep["latent"][key]) > 0


# Four Adam steps of the graph-replayed training step, hashed bit for bit: tests/golden/dead_cgmlp_step_bits.json holds the hashes
# the same runs gave while both networks still launched their last CGMLP (and the latent stage read the encoder's last-level
# scalars).  Cases: (jets, particles, map_to_latent, get_real method).
BITS_CASES = [(512, 30, "min&max", "sum"), (64, 30, "mix", "real"), (7, 30, "mean&max", "norm"), (5, 70, "min+mean", "real")]


def _case_id(B, N, pool, method):
    return f"{B}x{N}:{pool}:{method}"


def step_bits(B, N, pool, method):
    """sha256 of every buffer the training step leaves behind after four Adam steps, and of the latent the evaluation step
    returns on the trained weights."""
    import hashlib
    import numpy as np
    from lgn.step import NativeEvalStep, NativeTrainStep
    (enc, dec), _ = _pair(N, pool, seed=11)
    batch = _batch(B, N)
    st = NativeTrainStep(enc, dec, batch_size=B, lr=1e-3, l1_lambda=1e-6, use_graph=True, get_real_method=method)
    losses = torch.stack([st.step(batch)[0].clone() for _ in range(4)])
    lat = NativeEvalStep(enc, dec, B, get_real_method=method, keep_latent=True).run(batch)["latent"]
    torch.cuda.synchronize()
    bufs = {"losses": losses, "loss_out": st.loss_out, "grad": st.flat.grad, "adam_m": st.adam_m, "adam_v": st.adam_v,
            "weights": st.flat.flat, "step": st.step_dev, "recon": st.recon, "latent_s": lat[(0, 0)], "latent_v": lat[(1, 1)]}
    return {k: hashlib.sha256(np.ascontiguousarray(v.detach().cpu().numpy()).tobytes()).hexdigest() for k, v in bufs.items()}


@pytest.mark.parametrize("B,N,pool,method", BITS_CASES)
def test_training_step_is_bit_identical_to_the_one_that_ran_the_last_cgmlps(B, N, pool, method):
    with open(os.path.join(U.GOLDEN, "dead_cgmlp_step_bits.json")) as f:
        ref = json.load(f)[_case_id(B, N, pool, method)]
    got = step_bits(B, N, pool, method)
    bad = [k for k in ref if got[k] != ref[k]]
    assert not bad, f"differ bit for bit from the step that ran both last CGMLPs: {bad}"


def test_the_training_step_launches_no_cgmlp_forward_after_a_last_level():
    """Kernel launches of one eager step: one CGMLP forward per level but the last, in each network (3 levels: 2 + 2)."""
    from torch.profiler import DeviceType, ProfilerActivity, profile
    from lgn.step import NativeTrainStep
    (enc, dec), _ = _pair(30, "min&max", seed=11)
    batch = _batch(64, 30)
    st = NativeTrainStep(enc, dec, batch_size=64, use_graph=False)
    st.step(batch)
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        st.step(batch)
        torch.cuda.synchronize()
    names = [e.name for e in prof.events() if e.device_type == DeviceType.CUDA]
    assert any("level_fwd2_kernel" in n for n in names), f"the profiler saw no level kernel: {sorted(set(names))}"
    fwd = [n for n in names if "mlp_chain_fwd" in n]
    assert len(fwd) == 4, f"{len(fwd)} CGMLP forwards per step, expected 4: {fwd}"
