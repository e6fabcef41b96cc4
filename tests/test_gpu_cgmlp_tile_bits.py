"""Bit-for-bit pins of the tiled matrix-core CGMLP (csrc/mlp_tile_dev.hpp and the five kernels of mlp_mfma.hip / mlp_mfma_wide.hip
that call it), through lgn/_native.py cgmlp_fwd / cgmlp_bwd.  tests/golden/cgmlp_tile_bits.json holds the sha256 hashes of y, g_in
and every g_w, g_b as the library gave them while each of these kernels still carried its own copy of the geometry, the staging, the
forward layer and the backward's layer step (recorded with that library selected by LGN_AMD_LIB, on this module's code; each case
gave the same hashes in two runs and none was left out: profiles/r12_mlp_tile.txt, section 3).  Inputs come from CPU generators
with fixed seeds, the parameters O(1) from the oracle's _init_levels as test_gpu_parity.py test_cgmlp_widths builds them.
Rows (B, N): (2, 9) = 18 for the 16-row narrow kernels: two workgroups, the second with 2 real rows; (2, 37) = 74 for the wide
kernels: the backward's second 64-row workgroup has 10 rows, the forward's third 32-row workgroup 10; (271, 30) = 8130 for the
64-row narrow kernels: the first row count past the mlp_rows_per_workgroup threshold, the last workgroup with 2 rows."""
import json
import os

import pytest
import torch

import _util as U
import test_gpu_pair_sweep_bits as PS

# The hashes of the cases that run the encoder's input stage were recorded again when its mass stopped being contracted into fused
# multiply-adds (minkowski_sq_unfused, csrc/common.hpp: the reference's arithmetic); each case gave the same hashes in two runs.
pytestmark = pytest.mark.gpu

DEV = "cuda:0"
V1 = {"LGN_AMD_MLP_V1": "1"}
# id -> (C, mlp_width, mlp_depth, activation, B, N, environment switches)                     what it reaches
CASES = {
    "4,5,6,leakyrelu,18": (4, 5, 6, "leakyrelu", 2, 9, {}),                                  # narrow MT = 1: NT = 3, run-time k
    "4,5,6,elu,18": (4, 5, 6, "elu", 2, 9, {}),                                              # the activation switch
    "3,5,6,leakyrelu,18": (3, 5, 6, "leakyrelu", 2, 9, {}),                                  # H = 30: pad4, NT = 2
    "3,8,6,leakyrelu,18": (3, 8, 6, "leakyrelu", 2, 9, {}),                                  # H = 48 unrolled, not a chain kernel
    "4,5,3,leakyrelu,18": (4, 5, 3, "leakyrelu", 2, 9, {}),                                  # NH = 3
    "2,6,6,leakyrelu,18:v1": (2, 6, 6, "leakyrelu", 2, 9, V1),                               # KSH = 6
    "1,6,6,leakyrelu,18:v1": (1, 6, 6, "leakyrelu", 2, 9, V1),                               # NT = 1, KSH = 3
    "4,5,6,leakyrelu,8130": (4, 5, 6, "leakyrelu", 271, 30, {}),                             # narrow MT = 4
    "4,6,6,leakyrelu,8130:v1": (4, 6, 6, "leakyrelu", 271, 30, V1),                          # KSH = 12
    "3,6,6,leakyrelu,8130:v1": (3, 6, 6, "leakyrelu", 271, 30, V1),                          # KSH = 9
    "6,5,6,leakyrelu,74": (6, 5, 6, "leakyrelu", 2, 37, {}),                                 # wide, one pass: NT = 4, wide forward too
    "6,6,6,leakyrelu,74": (6, 6, 6, "leakyrelu", 2, 37, {}),                                 # chain forward + mlp_bwd_wide<5, 6>
    "6,6,6,leakyrelu,74:v1": (6, 6, 6, "leakyrelu", 2, 37, V1),                              # wide forward NT = 5
    "6,6,4,atan,74": (6, 6, 4, "atan", 2, 37, {}),                                           # NH = 4, the activation switch
    "8,6,6,leakyrelu,74:v1": (8, 6, 6, "leakyrelu", 2, 37, V1),                              # wide, two passes: NT = 6
    "7,6,6,elu,74": (7, 6, 6, "elu", 2, 37, {}),                                             # H = 84, partial last tile
    # the narrow backward reading the forward's copy of the activations back: reached only inside a training step
    "step:2x9:v1": (0, 0, 0, "", 2, 9, V1),
}


def mlp_bits(C, width, depth, act, B, N):
    from lgn import _native as Nn
    from oracle import lgn_oracle as O
    cfg = O.NetConfig(num_channels=(C, C), mlp_width=width, mlp_depth=depth)
    P = {}
    torch.manual_seed(100 * C + 10 * width + depth)
    O._init_levels(P, cfg, O.build_level_plans(cfg, {(0, 0): C, (1, 1): C}))
    ws = [P[f"lgn_cg.mlp_levels.0.linear.{i}.weight"].detach().contiguous().to(DEV) for i in range(depth + 1)]
    bs = [P[f"lgn_cg.mlp_levels.0.linear.{i}.bias"].detach().contiguous().to(DEV) for i in range(depth + 1)]
    assert tuple(ws[0].shape) == (width * 2 * C, 2 * C)
    g = torch.Generator().manual_seed(1000 * C + 100 * width + 10 * depth + N)
    s_in = torch.randn(2, B, N, C, dtype=torch.float64, generator=g).to(DEV)
    g_out = torch.randn(2, B, N, C, dtype=torch.float64, generator=g).to(DEV)
    act = Nn.activation_id(act)
    y = Nn.cgmlp_fwd(s_in, ws, bs, act)
    g_in, g_ws, g_bs = Nn.cgmlp_bwd(s_in, ws, bs, g_out, act)
    bufs = dict(y=y, g_in=g_in)
    bufs.update({f"g_w{i}": t for i, t in enumerate(g_ws)})
    bufs.update({f"g_b{i}": t for i, t in enumerate(g_bs)})
    return U.sha(bufs)


def case_bits(case):
    C, width, depth, act, B, N, _ = CASES[case]
    return PS.step_bits(N, B) if case.startswith("step") else mlp_bits(C, width, depth, act, B, N)


@pytest.mark.parametrize("case", list(CASES))
def test_cgmlp_tile_kernels_keep_their_bits(monkeypatch, case):
    for k, v in CASES[case][6].items():
        monkeypatch.setenv(k, v)
    with open(os.path.join(U.GOLDEN, "cgmlp_tile_bits.json")) as f:
        ref = json.load(f)[case]
    got = case_bits(case)
    assert set(ref) == set(got)
    bad = [k for k in ref if got[k] != ref[k]]
    assert not bad, f"differ bit for bit from the recorded tile kernels: {bad}"
