"""The chain CGMLP kernels on 64-row workgroups (>= 8 129 rows) with the padded last hidden tile as four-neuron block instructions
(csrc/mlp_chain.hip: Items; H = 36 / 24, and the H = 72 forward): against the oracle, against the full-tile instantiations
(LGN_AMD_MLP_FULLTILE=1), run to run, through the one-role kernels (LGN_AMD_MLP_BWD1=1), and inside one whole training step.
Shapes: 8 130 rows (271 jets x 30: the last workgroup holds 2 real rows) and 8 192 rows (256 x 32: no ragged tail)."""
import functools

import pytest
import torch

import _util as U

pytestmark = pytest.mark.gpu

FWD_TOL = 1e-11          # test_gpu_parity.test_cgmlp's bounds against the oracle
GRAD_TOL = 1e-9
AB_OUT_TOL = 1e-13       # thin against full tiles: test_level_mlp_full_batch_matches_small_batches_and_v1's bounds against the 12-wave kernels
AB_GRAD_TOL = 1e-11

SHAPES = [(271, 30), (256, 32)]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the GPU box"
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def _case(C, B, N, act, backward=True):
    """Inputs, parameters and the oracle's output and gradients (computed once per shape, never modified)."""
    from oracle import lgn_oracle as O
    g = torch.Generator().manual_seed(C * 7 + N)
    cfg = O.NetConfig(num_channels=(C, C), activation=act)
    P = {}
    torch.manual_seed(C)
    plans = O.build_level_plans(cfg, {(0, 0): C, (1, 1): C})
    O._init_levels(P, cfg, plans)
    P = {k: v.requires_grad_(True) for k, v in P.items() if "mlp" in k}
    s = torch.randn(2, B, N, C, 1, dtype=torch.float64, generator=g).requires_grad_(True)
    node = {(1, 1): torch.zeros(2, B, N, C, 4, dtype=torch.float64), (0, 0): s}
    out = O.cg_mlp(P, cfg, 0, node)[(0, 0)]
    cot = torch.randn(out.shape, dtype=torch.float64, generator=g)
    ref = {"out": out.detach()}
    if backward:
        (out * cot).sum().backward()
        ref["g_in"] = s.grad
        for i in range(7):
            ref[f"g_w{i}"] = P[f"lgn_cg.mlp_levels.0.linear.{i}.weight"].grad
            ref[f"g_b{i}"] = P[f"lgn_cg.mlp_levels.0.linear.{i}.bias"].grad
    W = [P[f"lgn_cg.mlp_levels.0.linear.{i}.{k}"].detach() for i in range(7) for k in ("weight", "bias")]
    return s.detach().squeeze(-1), W, cot, ref


def _native(dev, C, B, N, act, backward=True):
    """Output and gradients of the native operator under the switches in the environment NOW (the per-operator entry points read them per call)."""
    from lgn import ops, _native as Nn
    s, W, cot, _ = _case(C, B, N, act, backward)
    sd = s.to(dev).requires_grad_(backward)
    flat = [w.to(dev).requires_grad_(backward) for w in W]
    y = ops.CGMLPFn.apply(Nn.activation_id(act), sd, *flat)
    got = {"out": y.detach().unsqueeze(-1)}
    if backward:
        (y.unsqueeze(-1) * cot.to(dev)).sum().backward()
        got["g_in"] = sd.grad.unsqueeze(-1)
        for i in range(7):
            got[f"g_w{i}"], got[f"g_b{i}"] = flat[2 * i].grad, flat[2 * i + 1].grad
    return got


def _assert_vs_oracle(got, ref, what):
    for k, r in ref.items():
        U.assert_close(got[k], r, FWD_TOL if k == "out" else GRAD_TOL, f"{what}{k}")


CASES = [(C, B, N, "leakyrelu") for C in (2, 3, 4) for B, N in SHAPES] + [(3, 271, 30, "elu")]


@pytest.mark.parametrize("C,B,N,act", CASES)
def test_thin_tiles_vs_oracle_and_full_tiles(dev, C, B, N, act, monkeypatch):
    """Output, g_in and EVERY weight and bias gradient (rows and columns 32 .. 35 of the H = 36 hidden matrices and their 4 x 4 corner
    included: whole tensors are compared) against the oracle; the same against the full-tile kernels; two runs bit for bit.
    (C = 4, H = 48 has no padded tile: the switch must change nothing there.)"""
    _, _, _, ref = _case(C, B, N, act)
    thin = _native(dev, C, B, N, act)
    _assert_vs_oracle(thin, ref, "thin: ")
    again = _native(dev, C, B, N, act)
    for k in thin:
        assert torch.equal(thin[k], again[k]), f"two runs differ: {k}"
    monkeypatch.setenv("LGN_AMD_MLP_FULLTILE", "1")
    full = _native(dev, C, B, N, act)
    monkeypatch.delenv("LGN_AMD_MLP_FULLTILE")
    _assert_vs_oracle(full, ref, "full: ")
    for k in thin:
        U.assert_close(thin[k], full[k], AB_OUT_TOL if k == "out" else AB_GRAD_TOL, f"thin vs full tiles: {k}")
        if C == 4:
            assert torch.equal(thin[k], full[k]), f"H = 48 has no padded tile: {k}"


@pytest.mark.parametrize("C,B,N,act", [(2, 271, 30, "leakyrelu"), (3, 271, 30, "leakyrelu"), (3, 256, 32, "leakyrelu"), (3, 271, 30, "elu")])
def test_thin_tiles_one_role_kernels_vs_oracle(dev, C, B, N, act, monkeypatch):
    """LGN_AMD_MLP_BWD1=1: the four-wave forward and backward with thin chain layers meet the same oracle bounds."""
    _, _, _, ref = _case(C, B, N, act)
    monkeypatch.setenv("LGN_AMD_MLP_BWD1", "1")
    got = _native(dev, C, B, N, act)
    monkeypatch.delenv("LGN_AMD_MLP_BWD1")
    _assert_vs_oracle(got, ref, "one role: ")


def test_thin_tiles_h72_forward_vs_oracle(dev, monkeypatch):
    """C = 6, H = 72 (five tiles, eight real neurons in the last: two blocks): the chain forward against the oracle and the full tiles."""
    _, _, _, ref = _case(6, 271, 30, "leakyrelu", False)
    thin = _native(dev, 6, 271, 30, "leakyrelu", False)
    U.assert_close(thin["out"], ref["out"], FWD_TOL, "H = 72 forward")
    monkeypatch.setenv("LGN_AMD_MLP_FULLTILE", "1")
    full = _native(dev, 6, 271, 30, "leakyrelu", False)
    monkeypatch.delenv("LGN_AMD_MLP_FULLTILE")
    U.assert_close(thin["out"], full["out"], AB_OUT_TOL, "H = 72 forward, thin vs full tiles")


def test_thin_tiles_whole_step_vs_full_tiles(monkeypatch):
    """One training step of cfg2's networks at 280 jets x 30 (8 400 rows: 64-row CGMLP workgroups), graph-replayed: loss and all
    gradients, thin against LGN_AMD_MLP_FULLTILE=1 (frozen into the descriptor), within the bounds test_native_step_batch_regimes
    holds the chain kernels to against LGN_AMD_MLP_V1 (1e-13 / 1e-10); the reconstruction within that test's 1e-12."""
    import __graft_entry__ as G
    from lgn.step import NativeTrainStep
    from oracle import lgn_oracle as O
    dev = torch.device("cuda:0")
    B, N, che, chd = 280, 30, (3, 3, 4, 4), (4, 4, 3, 3)
    p4, labels = O.synthetic_jets(B, N, seed=B, pad=True)
    batch = {"p4": p4.to(dev), "labels": labels.to(dev)}
    enc, dec = G._models(N, che, chd, dev, seed=5)
    a = NativeTrainStep(enc, dec, batch_size=B, optimizer=False, use_graph=True)
    la, ra = a.step(batch)
    la, ra = a.step(batch)                  # (the replay)
    enc2, dec2 = G._models(N, che, chd, dev, seed=5)
    monkeypatch.setenv("LGN_AMD_MLP_FULLTILE", "1")
    b = NativeTrainStep(enc2, dec2, batch_size=B, optimizer=False, use_graph=True)
    monkeypatch.delenv("LGN_AMD_MLP_FULLTILE")
    lb, rb = b.step(batch)
    U.assert_close(la, lb, 1e-13, "loss, thin vs full tiles")
    U.assert_close(ra, rb, 1e-12, "recon, thin vs full tiles")
    U.assert_close(a.flat.grad, b.flat.grad, 1e-10, "flat gradient, thin vs full tiles")
