"""Host-side checks of LGN_NET_MLP_KEEP (include/lgn_amd.h): the descriptor bit that asks the training step to keep the hidden
activations of its CGMLPs beyond the 16-row regime (more than 8 128 rows).  With the bit the step workspace of cfg2 and cfg4 grows
by exactly the four kept copies -- the CGMLPs of levels 0 and 1 of either network; the last level's has no backward in the step --
and by no alignment: a copy is 6 layers x rows (a multiple of 64) x 48 doubles, a multiple of the carve's 16-double granule.  The
evaluation workspace and a maxdim-3 (table-driven, H = 72) descriptor do not move.  The flags = 0 totals themselves are the ones
tests/golden/workspace_doubles.json holds (test_host_workspace.py).  No GPU needed."""
import ctypes as C
import json
import os

import pytest
import torch

import _util as U
from lgn import _native as N

KEEP = 8192                               # LGN_NET_MLP_KEEP
CH2 = ((3, 3, 4, 4), (4, 4, 3, 3))
CH3 = ((4, 4, 6, 6), (6, 6, 4, 4))
# id -> (jets, particles, channels, maxdim)
SHAPES = {"cfg1": (32, 30, CH2, 2), "cfg2": (512, 30, CH2, 2), "cfg4": (256, 150, CH2, 2), "cfg5": (512, 30, CH3, 3)}
# doubles of one kept copy: 6 hidden layers x rows rounded up to 64 x the hidden width rounded up to 16 (H = 36 and H = 48: 48)
COPY = {"cfg2": 6 * 15360 * 48, "cfg4": 6 * 38400 * 48}


def _totals(cfg, flags):
    import __graft_entry__ as G
    from lgn.ops import describe_network
    B, n, (ce, cd), maxdim = SHAPES[cfg]
    enc, dec = G._models(n, ce, cd, torch.device("cpu"), maxdim=maxdim)
    d = N.NetDesc()
    d.B, d.N, d.n_levels = B, n, enc.num_cg_levels
    keep = describe_network(d, enc, False) + describe_network(d, dec, True)
    d.mlp_hidden_mul, d.mlp_nlin = enc.mlp_width, enc.mlp_depth + 1
    d.flags = flags
    lib, ref = N.lib(), C.byref(d)
    out = {"step": lib.lgn_step_workspace_doubles(ref), "eval": lib.lgn_eval_workspace_doubles(ref)}
    del keep
    assert all(v > 0 for v in out.values()), (cfg, flags, out, N.last_error())
    return out


def _golden(cfg):
    with open(os.path.join(U.GOLDEN, "workspace_doubles.json")) as f:
        return json.load(f)[cfg]


def test_the_figures_of_the_documents():
    assert COPY["cfg2"] == 4423680 and 4 * COPY["cfg2"] * 8 == 141557760       # 141.6 MB
    assert COPY["cfg4"] == 11059200 and 4 * COPY["cfg4"] * 8 == 353894400      # 353.9 MB


@pytest.mark.parametrize("cfg", ["cfg2", "cfg4"])
def test_the_bit_adds_the_four_kept_copies_and_nothing_else(cfg):
    plain, kept, ref = _totals(cfg, 0), _totals(cfg, KEEP), _golden(cfg)
    assert plain["step"] == ref["step"] and plain["eval"] == ref["eval"]
    assert kept["step"] - plain["step"] == 4 * COPY[cfg]
    assert kept["eval"] == plain["eval"]


def test_a_small_batch_keeps_its_copies_with_or_without_the_bit():
    """cfg1: 960 rows, the 16-row regime, whose copies the step has always kept."""
    assert _totals("cfg1", KEEP) == _totals("cfg1", 0) == {k: _golden("cfg1")[k] for k in ("step", "eval")}


def test_a_maxdim3_descriptor_is_unchanged():
    assert _totals("cfg5", KEEP) == _totals("cfg5", 0) == {k: _golden("cfg5")[k] for k in ("step", "eval")}


def test_net_flags_sets_the_bit_unless_asked_to_recompute(monkeypatch):
    monkeypatch.delenv("LGN_AMD_MLP_RECOMPUTE", raising=False)
    assert N.net_flags() & KEEP and N.NetDesc().flags & KEEP
    monkeypatch.setenv("LGN_AMD_MLP_RECOMPUTE", "1")
    assert not N.net_flags() & KEEP and not N.NetDesc().flags & KEEP
