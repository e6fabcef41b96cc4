"""Host-side tests of the native --normalize path (no GPU): the torch restatement tests/_normalize_ref.py against the reference's
own outputs (g21), the C ABI (symbols, version, argument refusals before any launch) and the method-name matching."""
import json
import logging

import numpy as np
import pytest
import torch

import _normalize_ref as R
import _util as U
from lgn import _native as N


def _g21():
    z = U.load("g21_normalize.npz")
    return z, torch.from_numpy(z["p4"]), json.loads(str(z["names"]))


def test_restatement_equals_the_reference_bit_for_bit():
    """Factors and quotients of every method and spelling; NaN where the reference has NaN.  The reference's jet_E quotient is the
    (B, B, N, 4) table p4[b] / factor[a] (its factor is (B, 1, 1, 1)): the restatement is its diagonal."""
    z, p4, names = _g21()
    assert names == ["component_max", "overall_max", "jet_E", "Overall-Max", "jet e", "bogus"]
    for name in names:
        out, f = R.normalize_p4(p4, name)
        f_ref, out_ref = z[f"factor.{name}"], z[f"out.{name}"]
        if out_ref.ndim == 4:
            assert f_ref.shape == (6, 1, 1, 1)
            f_ref, out_ref = f_ref.reshape(6, 1, 1), np.stack([out_ref[b, b] for b in range(6)])
        assert tuple(f.shape) == f_ref.shape == ((6, 1, 4) if name == "component_max" else (6, 1, 1))
        assert np.array_equal(f.numpy(), f_ref, equal_nan=True), name
        assert np.array_equal(out.numpy(), out_ref, equal_nan=True), name
    # the quirks the fixture pins: EPS is added (all-zero jet: factor 1e-16, stays zero), a NaN poisons its own jet only
    f = R.factor(p4, "overall_max").flatten()
    assert f[3].item() == 1e-16 and bool((R.normalize_p4(p4, "overall_max")[0][3] == 0).all())
    assert bool(torch.isnan(f[5])) and bool(torch.isfinite(f[:5]).all())
    assert torch.equal(R.factor(p4, "bogus")[:5], R.factor(p4, "overall_max")[:5])


def test_normalize_symbols_are_exported():
    lib = N.lib()
    for name in ("lgn_stage_batch_f64", "lgn_denormalize_f64"):
        assert name in N.EXPORTED_SYMBOLS
        assert hasattr(lib, name)
    assert lib.lgn_abi_version() == 19
    assert (N.NORM_NONE, N.NORM_COMPONENT_MAX, N.NORM_OVERALL_MAX, N.NORM_JET_E) == (0, 1, 2, 3)


@pytest.mark.parametrize("name,code", [("component_max", 1), ("overall_max", 2), ("jet_E", 3), ("Overall-Max", 2), ("jet e", 3),
                                       ("COMPONENT MAX", 1), ("Jet-E", 3)])
def test_method_names_match_as_the_reference_matches_them(name, code, caplog):
    from lgn.ops import normalize_code
    from lgn.step import normalize_code as step_code
    with caplog.at_level(logging.WARNING):
        assert normalize_code(name) == code and step_code(name) == code
    assert not caplog.records
    assert R.method_key(name) == {1: "component_max", 2: "overall_max", 3: "jet_e"}[code]


def test_unknown_method_warns_and_takes_overall_max(caplog):
    from lgn.ops import normalize_code
    with caplog.at_level(logging.WARNING):
        assert normalize_code("bogus") == N.NORM_OVERALL_MAX
    assert any("bogus not recognized" in r.getMessage() for r in caplog.records)


def test_step_classes_take_the_normalize_arguments():
    import inspect
    import lgn.step as S
    for cls in (S.NativeTrainStep, S.CapturedModuleStep, S.TrainStep, S.ReferenceLoopStep, S.NativeEvalStep, S.ModuleEvalStep):
        p = inspect.signature(cls.__init__).parameters
        assert p["normalize"].default is False and p["normalize_method"].default == "overall_max", cls.__name__
    assert list(inspect.signature(S.normalize_p4).parameters) == ["p4"]


P = 16         # placeholder device pointer (16-byte aligned): every call below must be refused before anything touches it
OUT = (P, P, P, P, P)          # p4_in, target, mask, in_scalars, factor


@pytest.mark.parametrize("src,dims,method,opts,out,what", [
    ((P, None, None), (4, 4, 30), 4, (1.0, 0, 0), OUT, "unknown method code 4"),
    ((P, None, None), (4, 4, 30), -1, (1.0, 0, 0), OUT, "unknown method code -1"),
    ((P, None, None), (0, 4, 30), 2, (1.0, 0, 0), OUT, "B = 0"),
    ((P, None, None), (4, 3, 30), 2, (1.0, 0, 0), OUT, "B_pad = 3 < B = 4"),
    ((P, None, None), (4, 4, 0), 2, (1.0, 0, 0), OUT, "N = 0"),
    ((P, None, None), (4, 4, 30), 2, (1.0, 0, -1), OUT, "K = -1"),
    ((None, None, None), (4, 4, 30), 2, (1.0, 0, 0), OUT, "null p4"),
    ((P, None, None), (4, 4, 30), 2, (1.0, 0, 0), (None, P, P, P, P), "null output"),
    ((P, None, None), (4, 4, 30), 2, (1.0, 0, 0), (P, None, P, P, P), "null output"),
    ((P, None, None), (4, 4, 30), 2, (1.0, 0, 0), (P, P, None, P, P), "null output"),
    ((P, None, None), (4, 4, 30), 2, (1.0, 0, 0), (P, P, P, P, None), "null output"),
    ((P, None, None), (4, 4, 30), 2, (1.0, 1, 0), (P, 32, P, None, P), "in_scalars missing"),
    ((P, None, P), (4, 4, 30), 2, (1.0, 0, 2), (P, 32, P, None, P), "in_scalars missing"),
    ((P, None, None), (4, 4, 30), 2, (1.0, 0, 2), (P, 32, P, P, P), "null scalars"),
    ((P, None, None), (4, 4, 30), 2, (0.5, 0, 0), OUT, "target may be p4_in only"),
    ((P, None, None), (4, 4, 30), 2, (1.0, 1, 0), OUT, "target may be p4_in only"),
    ((8, None, None), (4, 4, 30), 2, (1.0, 0, 0), OUT, "16-byte aligned"),
])
def test_stage_batch_refusals(src, dims, method, opts, out, what):
    p4, labels, scalars = src
    (B, B_pad, n), (scale, jet, K) = dims, opts
    p4_in, target, mask, in_scalars, factor = out
    assert N.lib().lgn_stage_batch_f64(p4, labels, scalars, B, B_pad, n, method, scale, jet, K, p4_in, target, mask, in_scalars, factor,
                                       None) < 0
    assert what in N.last_error()


@pytest.mark.parametrize("B,n,ptrs,what", [
    (0, 30, (P, P, P, P, P), "B = 0"),
    (4, 0, (P, P, P, P, P), "N = 0"),
    (4, 30, (None, P, P, P, P), "null pointer"),
    (4, 30, (P, P, None, P, P), "null pointer"),
    (4, 30, (P, P, P, None, P), "null pointer"),
    (4, 30, (P, None, P, P, P), "go together"),
    (4, 30, (P, P, P, P, None), "go together"),
    (4, 30, (P, P, P, 8, P), "16-byte aligned"),
])
def test_denormalize_refusals(B, n, ptrs, what):
    x0, x1, factor, out0, out1 = ptrs
    assert N.lib().lgn_denormalize_f64(x0, x1, factor, B, n, out0, out1, None) < 0
    assert what in N.last_error()
