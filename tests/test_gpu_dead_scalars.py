"""GPU tests of the last levels without live scalars.  The scalar output of either network's last level reaches neither the loss nor
anything a step returns, and its upstream gradient is identically zero: the level kernels of those launches leave out the scalar
aggregates, the scalar CatMix rows and every backward term the zero gradient multiplies.  LGN_AMD_LIVE_SCALARS=1 runs the same
launches on the kernels with live scalars (on the zero block, as before): every result must be the same bits."""
import os

import pytest
import torch

import _util as U

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
CH = ((3, 3, 4, 4), (4, 4, 3, 3))        # cfg2: the encoder's last level has C = 4, the decoder's C = 3
SWITCH = "LGN_AMD_LIVE_SCALARS"

# (jets, particles, map_to_latent, get_real method, further switches, fwd_bwd | finalize form)
#   257 x 6, 257 x 30   level_jet_split = 1: whole-jet symmetric sweep (6 particles: two row groups, one partly padded)
#   64 x 30             eight workgroups per jet, partner / source-group split
#   3 x 70              N > 40: the forward without live scalars, the three-kernel backward on the zero block
#   2 x 150             chunked rows
TRAIN_CASES = [
    (257, 6, "min&max", "sum", (), False),
    (257, 30, "min&max", "sum", (), True),
    (257, 30, "mix", "real", ("LGN_AMD_BWD_ORDERED",), False),
    (64, 30, "mix", "real", (), False),
    (64, 30, "min&max", "sum", ("LGN_AMD_DEC_PAIRWISE",), True),
    (3, 70, "min&max", "real", (), False),
    (2, 150, "min&max", "sum", (), False),
]


def _models(N, pool, seed, **kw):
    import __graft_entry__ as G
    return G._models(N, *CH, torch.device(DEV), seed=seed, map_to_latent=pool, **kw)


def _batch(B, N):
    from oracle import lgn_oracle as O
    p4, labels = O.synthetic_jets(B, N, seed=B + N, pad=True)
    return {"p4": p4.to(DEV), "labels": labels.to(DEV)}


@pytest.fixture
def one_rank_group():
    """The fwd_bwd | all-reduce | finalize form of the step needs a process group: one rank, here."""
    import socket
    import torch.distributed as dist
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
    yield
    dist.destroy_process_group()


def _last_wm0(net, flat):
    """(offset, size) of the last level's scalar CatMix weight in the flat parameter / gradient buffers."""
    w = net.lgn_cg.node_levels[-1].cat_mix.mix_reps.weight((0, 0))
    return (w.data_ptr() - flat.flat.data_ptr()) // 8, w.numel()


def _train(monkeypatch, live, B, N, pool, method, flags, two_calls, jet_features=False):
    """Four Adam steps; the buffers the step leaves behind.  The switches are frozen into the descriptor when the step is built."""
    from lgn.step import NativeTrainStep
    for f in flags:
        monkeypatch.setenv(f, "1")
    if live:
        monkeypatch.setenv(SWITCH, "1")
    else:
        monkeypatch.delenv(SWITCH, raising=False)
    enc, dec = _models(N, pool, seed=11, jet_features=jet_features)
    st = NativeTrainStep(enc, dec, batch_size=B, lr=1e-3, l1_lambda=1e-6, use_graph=False, get_real_method=method,
                         force_collective=two_calls, graph_collective=False if two_calls else None)
    assert bool(st.desc.flags & 4096) == live
    batch = _batch(B, N)
    losses = torch.stack([st.step(batch)[0].clone() for _ in range(4)])
    torch.cuda.synchronize()
    out = {"losses": losses, "grad": st.flat.grad.clone(), "adam_m": st.adam_m.clone(), "adam_v": st.adam_v.clone(),
           "weights": st.flat.flat.clone(), "recon": st.recon.clone()}
    dead = [_last_wm0(enc, st.flat), _last_wm0(dec, st.flat)]
    return out, dead, st.l1_lambda


def _assert_same_bits(a, b):
    for k in a:
        assert torch.isfinite(a[k]).all(), k
        assert torch.equal(a[k], b[k]), f"{k} differs from the step with live scalars"


@pytest.mark.parametrize("B,N,pool,method,flags,two_calls", TRAIN_CASES)
def test_training_step_without_live_scalars_is_the_step_with_them_bit_for_bit(monkeypatch, request, B, N, pool, method, flags, two_calls):
    if two_calls:
        request.getfixturevalue("one_rank_group")
    new, dead, lam = _train(monkeypatch, False, B, N, pool, method, flags, two_calls)
    old, _, _ = _train(monkeypatch, True, B, N, pool, method, flags, two_calls)
    _assert_same_bits(new, old)
    # the last levels' scalar CatMix weights see the L1 term only: gradient = lambda * sign(w), in both
    for off, n in dead:
        for r in (new, old):
            g = r["grad"][off:off + n]
            assert torch.equal(g.abs(), torch.full_like(g, lam)), "the last level's wm0 has a loss gradient"


def test_split_training_step_with_jet_features_is_the_same_bits(monkeypatch):
    """jet_features gives the encoder one node more than the decoder: the four end stages are launches of their own."""
    new, _, _ = _train(monkeypatch, False, 7, 30, "min&max", "sum", (), False, jet_features=True)
    old, _, _ = _train(monkeypatch, True, 7, 30, "min&max", "sum", (), False, jet_features=True)
    _assert_same_bits(new, old)


@pytest.mark.parametrize("B,N,pool", [(257, 30, "min&max"), (64, 30, "mix"), (3, 70, "min&max")])
def test_last_level_wm0_gradient_is_exactly_zero_native_and_module(B, N, pool):
    """No optimiser, no L1 term: the gradient slice of each network's last-level wm0 holds no non-zero, on the native step and on the
    module path (one native call per operator, autograd in between)."""
    from lgn.step import NativeTrainStep, TrainStep
    enc, dec = _models(N, pool, seed=7)
    enc2, dec2 = _models(N, pool, seed=7)
    for m in (enc2, dec2):
        m.use_fused = False
    batch = _batch(B, N)
    a = NativeTrainStep(enc, dec, batch_size=B, optimizer=False, use_graph=False, l1_lambda=0.0)
    b = TrainStep(enc2, dec2, optimizer=False, l1_lambda=0.0)
    a.step(batch)
    a.step(batch)
    b.forward_backward(batch)
    torch.cuda.synchronize()
    for step, nets in ((a, (enc, dec)), (b, (enc2, dec2))):
        assert torch.count_nonzero(step.flat.grad) > 0
        for net in nets:
            off, n = _last_wm0(net, step.flat)
            assert n > 0 and torch.count_nonzero(step.flat.grad[off:off + n]) == 0
    U.assert_close(a.flat.grad, b.flat.grad, 1e-9, "flat gradient")


@pytest.mark.parametrize("B,N,pool", [(257, 30, "min&max"), (64, 30, "mix"), (3, 70, "min&max"), (2, 150, "min&max")])
def test_eval_step_is_the_same_bits_and_the_kept_latent_has_live_scalars(monkeypatch, B, N, pool):
    from lgn.step import NativeEvalStep
    enc, dec = _models(N, pool, seed=3)
    batch = _batch(B, N)
    res = {}
    for live in (False, True):
        if live:
            monkeypatch.setenv(SWITCH, "1")
        else:
            monkeypatch.delenv(SWITCH, raising=False)
        for keep in (False, True):
            r = NativeEvalStep(enc, dec, B, get_real_method="real", keep_latent=keep, use_graph=False).run(batch)
            res[live, keep] = {"recon": r["recon"].clone(), "loss": r["loss"].clone()}
            if keep:
                res[live, keep]["latent"] = {q: r["latent"][q].clone() for q in ((0, 0), (1, 1))}
    torch.cuda.synchronize()
    ref = res[True, True]
    for key, r in res.items():
        assert torch.isfinite(r["recon"]).all()
        assert torch.equal(r["recon"], ref["recon"]) and torch.equal(r["loss"], ref["loss"]), key
    with torch.no_grad():
        lat = enc(batch)
    for live in (False, True):
        for key in ((0, 0), (1, 1)):
            got = res[live, True]["latent"][key]
            assert torch.equal(got, ref["latent"][key])
            U.assert_close(got, lat[key], 1e-12, f"latent {key}")
            assert torch.count_nonzero(got) > 0
