"""Host-side checks of the evaluation step's C ABI (lgn_eval_workspace_doubles / lgn_step_eval_f64): the symbols, the workspace
size next to the training step's at the benchmark configurations, and the refusals that come before anything is enqueued.  The
descriptors are filled from models built on the CPU.  No GPU needed."""
import ctypes as C

import pytest
import torch

from lgn import _native as N

CONFIGS = {"cfg1": (32, 30, (3, 3, 4, 4), (4, 4, 3, 3), 2), "cfg2": (512, 30, (3, 3, 4, 4), (4, 4, 3, 3), 2),
           "cfg4": (256, 150, (3, 3, 4, 4), (4, 4, 3, 3), 2), "cfg5": (512, 30, (4, 4, 6, 6), (6, 6, 4, 4), 3)}


def _desc(cfg, **kw):
    import __graft_entry__ as G
    from lgn.ops import describe_network
    B, n, ce, cd, maxdim = CONFIGS[cfg]
    enc, dec = G._models(n, ce, cd, torch.device("cpu"), maxdim=maxdim)
    d = N.NetDesc()
    d.B, d.N, d.n_levels = B, n, enc.num_cg_levels
    keep = describe_network(d, enc, False) + describe_network(d, dec, True)
    d.mlp_hidden_mul, d.mlp_nlin = enc.mlp_width, enc.mlp_depth + 1
    for k, v in kw.items():
        setattr(d, k, v)
    return d, (enc, dec, keep)


def test_eval_symbols_are_exported():
    lib = N.lib()
    for name in ("lgn_eval_workspace_doubles", "lgn_step_eval_f64"):
        assert name in N.EXPORTED_SYMBOLS
        assert hasattr(lib, name)
    assert N.lib().lgn_abi_version() == 19


@pytest.mark.parametrize("cfg", sorted(CONFIGS))
def test_eval_workspace_is_smaller_than_the_step_workspace(cfg):
    d, _keep = _desc(cfg)
    step = N.lib().lgn_step_workspace_doubles(C.byref(d))
    ev = N.lib().lgn_eval_workspace_doubles(C.byref(d))
    assert 0 < ev < step, (cfg, ev, step)


def test_eval_workspace_refuses_a_bad_descriptor():
    d, _keep = _desc("cfg1", get_real=7)
    assert N.lib().lgn_eval_workspace_doubles(C.byref(d)) == -1
    assert "get_real" in N.last_error()


def _call(d, target=8, workspace_doubles=None):
    """lgn_step_eval_f64 with placeholder device pointers: every call here must be refused before a launch."""
    lib = N.lib()
    off = (C.c_int64 * 64)()
    ws = lib.lgn_eval_workspace_doubles(C.byref(d)) if workspace_doubles is None else workspace_doubles
    p = 8
    return lib.lgn_step_eval_f64(C.byref(d), p, off, off, p, target, p, None, p, ws, p, None, None, p, p, None, None, None, None)


def test_eval_refuses_a_null_target():
    d, _keep = _desc("cfg1")
    assert _call(d, target=None) != 0
    assert "null pointer" in N.last_error()


def test_eval_refuses_a_short_workspace():
    d, _keep = _desc("cfg1")
    need = N.lib().lgn_eval_workspace_doubles(C.byref(d))
    assert _call(d, workspace_doubles=need - 1) != 0
    assert "workspace" in N.last_error()


@pytest.mark.parametrize("code", [5, -1])
def test_eval_refuses_an_unknown_get_real_code(code):
    d, _keep = _desc("cfg1", get_real=code)
    assert _call(d) != 0
    assert "get_real" in N.last_error()


@pytest.mark.parametrize("tau_v_in", [5, 32])
def test_training_step_refuses_a_decoder_that_does_not_take_the_pooled_latent(tau_v_in):
    """The fused maxdim-2 training step (one node count, the mass the only input scalar) refuses a decoder whose tau_v_in is not the
    encoder's pool_blocks * tau_v, before any launch (placeholder pointers), as the split, table-driven and evaluation steps do; the
    workspace query refuses it too."""
    d, _keep = _desc("cfg1", tau_v_in=tau_v_in)
    lib = N.lib()
    assert lib.lgn_step_workspace_doubles(C.byref(d)) == -1
    assert "pooled latent" in N.last_error()
    off = (C.c_int64 * 64)()
    p = 8
    assert lib.lgn_step_fwd_bwd_f64(C.byref(d), p, p, 1000, off, off, p, p, p, None, p, 1 << 40, p, p, None, None, None, None) != 0
    assert "pooled latent" in N.last_error()
