"""Bit-for-bit pins of the pair sweep (csrc/pair_dev.hpp and the kernels that call it): geometry of a pair, the radial network on the
matrix cores, the edge gradients and the radial-parameter GEMM, through the per-operator calls of lgn/_native.py.
tests/golden/pair_sweep_bits.json holds the sha256 hashes of every output buffer as the library gave them while each of these
kernels still carried its own copy of that arithmetic (recorded with that library selected by LGN_AMD_LIB, on this module's code;
each case gave the same hashes in two runs and none was left out: profiles/r11_pair_dev.txt, section 3).  Inputs come from CPU
generators with fixed seeds.  Shapes (C, CO, N, B) are the smallest that reach each instantiation: 257 jets of 9 particles = whole
jets per workgroup with a padded third group (symmetric backward: tiles above, on and below the diagonal); 2 jets of 9 =
level_jet_split with the rs = 2 and rs = 4 receiver split; N = 41 = level_bwd_mix + level_bwd_sweep_enc with four waves; N = 150,
one jet = eight waves and several receiver chunks; N = 33 at maxdim 3 = the moments kernels of generic_moments.hip by size; five packed
components (":q5") = the two-components-per-thread instantiations of generic_moments2.hip; N = 150 at maxdim 3 = the smallest round
shape whose features exceed the LDS, read from global memory by generic_moments.hip.  (The q5 and N = 150 moments cases were
recorded from the library as it was before the kernels' launches went through csrc/lds.hpp, each the same in two runs.)"""
import json
import os

import pytest
import torch

import _util as U

# The hashes of the cases that run the encoder's input stage were recorded again when its mass stopped being contracted into fused
# multiply-adds (minkowski_sq_unfused, csrc/common.hpp: the reference's arithmetic); each case gave the same hashes in two runs.
pytestmark = pytest.mark.gpu

DEV = "cuda:0"
ORDERED = {"LGN_AMD_BWD_ORDERED": "1"}
# id -> (kind, decoder, C, CO, N, B, environment switches); moments cases: CO = packed components per node (0: Q3, maxdim = 3)
CASES = {
    "enc:4,4,9,257": ("level", False, 4, 4, 9, 257, {}),
    "enc:4,4,9,257:ordered": ("level", False, 4, 4, 9, 257, ORDERED),
    "enc:3,4,9,257": ("level", False, 3, 4, 9, 257, {}),
    "enc:5,5,9,257": ("level", False, 5, 5, 9, 257, {}),
    "enc:4,4,9,2": ("level", False, 4, 4, 9, 2, {}),
    "enc:4,3,41,2": ("level", False, 4, 3, 41, 2, {}),
    "enc:4,3,41,2:ordered": ("level", False, 4, 3, 41, 2, ORDERED),
    "enc:5,5,41,1": ("level", False, 5, 5, 41, 1, {}),
    "enc:4,4,150,1": ("level", False, 4, 4, 150, 1, {}),
    "enc:4,4,150,1:ordered": ("level", False, 4, 4, 150, 1, ORDERED),
    "enc:4,4,9,2:v2": ("level", False, 4, 4, 9, 2, {"LGN_AMD_LEVEL_V2": "1"}),
    "dec:4,4,9,2:v2": ("level", True, 4, 4, 9, 2, {"LGN_AMD_LEVEL_V2": "1"}),
    "dec:4,4,9,2:pairwise": ("level", True, 4, 4, 9, 2, {"LGN_AMD_DEC_PAIRWISE": "1"}),
    "m3:enc:4,9,2": ("moments", False, 4, 0, 9, 2, {}),
    "m3:dec:4,9,2": ("moments", True, 4, 0, 9, 2, {}),
    "m3:enc:4,9,2:split": ("moments", False, 4, 0, 9, 2, {"LGN_AMD_MOMENTS_SPLIT": "1"}),
    "m3:dec:4,9,2:split": ("moments", True, 4, 0, 9, 2, {"LGN_AMD_MOMENTS_SPLIT": "1"}),
    "m3:enc:4,9,2:v1": ("moments", False, 4, 0, 9, 2, {"LGN_AMD_MOMENTS_V1": "1"}),
    "m3:dec:4,9,2:v1": ("moments", True, 4, 0, 9, 2, {"LGN_AMD_MOMENTS_V1": "1"}),
    "m3:dec:4,9,2:pairwise": ("moments", True, 4, 0, 9, 2, {"LGN_AMD_DEC_PAIRWISE": "1"}),
    "m3:enc:4,33,1": ("moments", False, 4, 0, 33, 1, {}),
    "m3:dec:4,33,1": ("moments", True, 4, 0, 33, 1, {}),
    "m3:enc:4,9,2:q5": ("moments", False, 4, 5, 9, 2, {}),
    "m3:enc:4,9,2:q5:split": ("moments", False, 4, 5, 9, 2, {"LGN_AMD_MOMENTS_SPLIT": "1"}),
    "m3:dec:4,9,2:q5:pairwise": ("moments", True, 4, 5, 9, 2, {"LGN_AMD_DEC_PAIRWISE": "1"}),
    "m3:enc:4,150,1": ("moments", False, 4, 0, 150, 1, {}),
    "m3:dec:4,150,1": ("moments", True, 4, 0, 150, 1, {}),
    # the dead-scalar (NOS) form of the symmetric backward: the last encoder level of a training step on whole-jet workgroups
    "step:257x9": ("step", False, 0, 0, 9, 257, {}),
}
Q3 = 4 + 3 + 3 + 9 + 1          # packed components of a maxdim = 3 node: (1,1), (2,0), (0,2), (2,2), (0,0)
CH = ((3, 3, 4, 4), (4, 4, 3, 3))   # channels of the training step, as tests/test_gpu_step_plumbing_bits.py


def _radial(decoder, C, g):
    """the seven radial parameters of one level, O(1) so that every gradient path carries digits; on the device"""
    from oracle import lgn_oracle as O
    P = {}
    torch.manual_seed(int(torch.randint(0, 10000, (1,), generator=g)))
    O._init_radial(P, O.NetConfig(num_channels=(C, C)), decoder)
    names = ["a", "b", "c", "linear.0.weight", "linear.0.bias", "linear.1.weight", "linear.1.bias"]
    rad = tuple(P["rad_funcs.rad_funcs.0." + n].detach().contiguous().to(DEV) for n in names)
    return (None, None, None, None, rad[4], None, rad[6]) if decoder else rad


def _momenta(decoder, N, B, C, g):
    from oracle import lgn_oracle as O
    if decoder:
        return torch.randn(2, B, N, 4, dtype=torch.float64, generator=g).to(DEV), None
    p4, labels = O.synthetic_jets(B, N, seed=N + C, pad=True)
    return p4.to(DEV), labels.to(DEV)


def level_bits(decoder, C, CO, N, B):
    from lgn import _native as Nn
    g = torch.Generator().manual_seed(100 * C + 10 * CO + N + int(decoder))
    rn = lambda *shape: torch.randn(*shape, dtype=torch.float64, generator=g)      # noqa: E731
    rad = _radial(decoder, C, g)
    s_in, v_in = rn(2, B, N, C).to(DEV), rn(2, B, N, C, 4).to(DEV)
    wm0, wm1 = (rn(2, CO, 5 * C) * 0.3).to(DEV), (rn(2, CO, 5 * C) * 0.3).to(DEV)
    g_s, g_v = rn(2, B, N, CO).to(DEV), rn(2, B, N, CO, 4).to(DEV)
    p, mask = _momenta(decoder, N, B, C, g)
    ag0, ag1, s_out, v_out = Nn.level_fwd(decoder, s_in, v_in, p, mask, rad, wm0, wm1)
    g_p = torch.zeros_like(p) if decoder else None
    g_s_in, g_v_in, g_wm0, g_wm1, rg = Nn.level_bwd(decoder, s_in, v_in, p, mask, rad, wm0, wm1, ag0, ag1, g_s, g_v, g_p)
    bufs = dict(ag0=ag0, ag1=ag1, s_out=s_out, v_out=v_out, g_s_in=g_s_in, g_v_in=g_v_in, g_wm0=g_wm0, g_wm1=g_wm1)
    bufs.update({f"g_rad{k}": t for k, t in enumerate(rg)})
    if decoder:
        bufs["g_p"] = g_p
    return U.sha(bufs)


def moments_bits(decoder, C, N, B, Q=0):
    from lgn import _native as Nn
    g = torch.Generator().manual_seed(3000 + 10 * C + N + int(decoder) + 100 * Q)
    Q = Q or Q3
    rn = lambda *shape: torch.randn(*shape, dtype=torch.float64, generator=g)      # noqa: E731
    rad = _radial(decoder, C, g)
    X = rn(2, B, N, C, Q).to(DEV)
    gU, gX = rn(B, N, C, Q, 5, 2).to(DEV), rn(2, B, N, C, Q).to(DEV)
    p, mask = _momenta(decoder, N, B, C, g)
    Um = Nn.moments_fwd(decoder, X, p, mask, rad)
    g_p = torch.zeros_like(p) if decoder else None
    rg = Nn.moments_bwd(decoder, X, p, mask, rad, gU, gX, g_p)
    bufs = dict(U=Um, gX=gX)
    bufs.update({f"g_rad{k}": t for k, t in enumerate(rg)})
    if decoder:
        bufs["g_p"] = g_p
    return U.sha(bufs)


def step_bits(N, B):
    """every buffer a training step leaves behind after two Adam steps, hashed like train_bits() of test_gpu_step_plumbing_bits.py"""
    import __graft_entry__ as G
    from oracle import lgn_oracle as O
    from lgn.step import NativeTrainStep
    enc, dec = G._models(N, *CH, torch.device(DEV), seed=11)
    p4, labels = O.synthetic_jets(B, N, seed=B + N, pad=True)
    batch = {"p4": p4.to(DEV), "labels": labels.to(DEV)}
    st = NativeTrainStep(enc, dec, batch_size=B, lr=1e-3, l1_lambda=1e-6, use_graph=True)
    losses = torch.stack([st.step(batch)[0].clone() for _ in range(2)])
    torch.cuda.synchronize()
    return U.sha({"losses": losses, "loss_out": st.loss_out, "grad": st.flat.grad, "adam_m": st.adam_m, "adam_v": st.adam_v,
                  "weights": st.flat.flat, "step": st.step_dev, "recon": st.recon, "loss_part": st.loss_part})


def case_bits(case):
    kind, decoder, C, CO, N, B, _ = CASES[case]
    if kind == "level":
        return level_bits(decoder, C, CO, N, B)
    if kind == "moments":
        return moments_bits(decoder, C, N, B, CO)
    return step_bits(N, B)


@pytest.mark.parametrize("case", list(CASES))
def test_pair_sweep_keeps_its_bits(monkeypatch, case):
    for k, v in CASES[case][6].items():
        monkeypatch.setenv(k, v)
    with open(os.path.join(U.GOLDEN, "pair_sweep_bits.json")) as f:
        ref = json.load(f)[case]
    got = case_bits(case)
    assert set(ref) == set(got)
    bad = [k for k in ref if got[k] != ref[k]]
    assert not bad, f"differ bit for bit from the recorded pair sweep: {bad}"
