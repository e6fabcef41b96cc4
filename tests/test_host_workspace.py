"""Workspace totals of csrc/step.hip, pinned: what lgn_step_workspace_doubles, lgn_eval_workspace_doubles and
lgn_net_workspace_doubles (encoder and decoder, activations and backward scratch) return for the benchmark configurations, for
maxdim-2 shapes that take the other level kernels, for map_to_latent='mix', for a jet_features pair, and for cfg2 / cfg5 under each
descriptor flag that changes a carve.  Every carve takes its sizes in a fixed order, so an unchanged total per descriptor is the
host-side sign that no buffer moved.  tests/golden/workspace_doubles.json holds the totals the library gave before the sequencer
was written once per path (one network sequencer and one workspace carve per path).  The descriptors are filled from models built
on the CPU, as in test_host_eval_step.py.  No GPU needed."""
import ctypes as C
import json
import os

import pytest
import torch

import _util as U
from lgn import _native as N

CH2 = ((3, 3, 4, 4), (4, 4, 3, 3))
CH3 = ((4, 4, 6, 6), (6, 6, 4, 4))
# id -> (jets, particles the decoder reconstructs, channels, maxdim, model options)
SHAPES = {
    "cfg1": (32, 30, CH2, 2, {}),
    "cfg2": (512, 30, CH2, 2, {}),
    "cfg4": (256, 150, CH2, 2, {}),
    "cfg5": (512, 30, CH3, 3, {}),
    "3x41": (3, 41, CH2, 2, {}),
    "5x70": (5, 70, CH2, 2, {}),
    "7x30:mix": (7, 30, CH2, 2, dict(map_to_latent="mix")),
    "7x30:jet_features": (7, 30, CH2, 2, dict(jet_features=True)),
}
# LGN_NET_* bits of include/lgn_amd.h that change a carve
FLAGS = {"dec_pairwise": 2, "level_v2": 4, "no_static": 1, "dec_unfused": 256}
CASES = list(SHAPES) + [f"{cfg}:{flag}" for cfg in ("cfg2", "cfg5") for flag in FLAGS]


def _desc(case):
    """The descriptor of a whole step on the case's two networks (lgn/step.py: _step_desc), flags from the case and not from the
    environment."""
    import __graft_entry__ as G
    from lgn.ops import describe_network
    shape, _, flag = case.partition(":")
    if flag in FLAGS:
        case = shape
    B, n, (ce, cd), maxdim, opts = SHAPES[case]
    enc, dec = G._models(n, ce, cd, torch.device("cpu"), maxdim=maxdim, **opts)
    d = N.NetDesc()
    d.B, d.N, d.n_levels = B, enc.num_input_particles, enc.num_cg_levels
    keep = describe_network(d, enc, False) + describe_network(d, dec, True)
    d.mlp_hidden_mul, d.mlp_nlin = enc.mlp_width, enc.mlp_depth + 1
    d.dec_N = dec.num_output_particles if opts.get("jet_features") else 0
    d.flags = FLAGS.get(flag, 0)
    return d, (enc, dec, keep)


def totals(case):
    d, _keep = _desc(case)
    lib, ref = N.lib(), C.byref(d)
    if case == "7x30:jet_features":
        assert d.N == 31 and d.dec_N == 30 and d.n_in_scalars == 2
    out = {"step": lib.lgn_step_workspace_doubles(ref), "eval": lib.lgn_eval_workspace_doubles(ref)}
    for net, decoder in (("enc", 0), ("dec", 1)):
        for name, which in (("act", 0), ("scratch", 1)):
            out[f"{net}_{name}"] = lib.lgn_net_workspace_doubles(ref, decoder, which)
    return out


def _golden():
    with open(os.path.join(U.GOLDEN, "workspace_doubles.json")) as f:
        return json.load(f)


def test_every_case_is_recorded():
    assert sorted(_golden()) == sorted(CASES)


@pytest.mark.parametrize("case", CASES)
def test_workspace_totals_are_the_recorded_ones(case):
    ref, got = _golden()[case], totals(case)
    assert all(v > 0 for v in got.values()), (case, got, N.last_error())
    assert got == ref, (case, {k: (got[k], ref[k]) for k in ref if got.get(k) != ref[k]})
