"""Host-side checks of the optimiser options of the training steps (--optimizer rmsprop, --l2-lambda): the lgn_optim_desc entry points
are exported next to the old ones under ABI 19 and refuse bad arguments without a GPU; the option matching of lgn/step.py follows
utils/initialize.py:153-173 as recorded in g20_optimizer_defaults.json (tests/golden/gen_golden_g20.py); and the numpy restatement
of the update (tests/_optim_ref.py), which pins what the kernels implement, agrees with torch.optim on the CPU.  No GPU needed."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

import _optim_ref as R
from lgn import _native as N
from lgn import step as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("lgn_step_finalize_opt_f64", "lgn_step_train_opt_f64")


def _fixture():
    with open(os.path.join(ROOT, "tests", "golden", "g20_optimizer_defaults.json")) as fh:
        return json.load(fh)


def test_new_entry_points_are_exported_next_to_the_old_ones_under_abi_19():
    lib = N.lib()
    assert N.ABI_VERSION == 19 and lib.lgn_abi_version() == 19
    for name in NEW + ("lgn_step_finalize_f64", "lgn_step_train_f64"):
        assert hasattr(lib, name) and name in N.EXPORTED_SYMBOLS and name in N._SIGNATURES
        assert getattr(lib, name).argtypes == N._SIGNATURES[name]
    # the descriptor takes the place of five scalars (l1_lambda, lr, beta1, beta2, eps): four arguments fewer
    for new, old in zip(NEW, ("lgn_step_finalize_f64", "lgn_step_train_f64")):
        assert len(N._SIGNATURES[new]) == len(N._SIGNATURES[old]) - 4
        assert N._op in N._SIGNATURES[new]
    header = open(os.path.join(ROOT, "include", "lgn_amd.h")).read()
    assert "#define LGN_FINALIZE_OPT_SCRATCH %d" % N.FINALIZE_OPT_SCRATCH in header
    assert "#define LGN_OPT_ADAM %d" % N.OPT_ADAM in header and "#define LGN_OPT_RMSPROP %d" % N.OPT_RMSPROP in header
    assert [f[0] for f in N.OptimDesc._fields_] == ["kind", "l1_lambda", "l2_lambda", "lr", "eps", "beta1", "beta2", "alpha", "momentum"]
    assert C.sizeof(N.OptimDesc) == 72          # int (padded to 8) + 8 doubles


def test_null_pointer_calls_are_refused_without_a_gpu():
    lib = N.lib()
    rc = lib.lgn_step_finalize_opt_f64(None, None, 0, None, 0, None, None, None, None, 1, None, None)
    assert rc < 0 and b"null" in lib.lgn_last_error()
    rc = lib.lgn_step_train_opt_f64(*([None] * 3), 0, *([None] * 7), 0, None, None, 0, None, None, None, None, 1, None, None, None, None,
                                    None)
    assert rc < 0 and lib.lgn_last_error()


def test_descriptor_is_checked_before_anything_is_enqueued():
    """Host pointers that are never dereferenced: every refusal below comes before the first launch."""
    lib = N.lib()
    buf = (C.c_double * 8)()
    p = C.addressof(buf)

    def call(d, do_step=1, state=p):
        return lib.lgn_step_finalize_opt_f64(p, p, 4, p, 1, C.byref(d) if d is not None else None, state, state, state, do_step, p, None)

    assert call(None) < 0 and b"descriptor" in lib.lgn_last_error()
    d = N.OptimDesc()
    d.kind = 7
    assert call(d) < 0 and b"kind" in lib.lgn_last_error()
    d.kind = N.OPT_RMSPROP
    d.alpha, d.momentum = 0.99, 0.9
    assert call(d, state=None) < 0 and b"state" in lib.lgn_last_error()
    d.l2_lambda = -1.0
    assert call(d) < 0 and b"l2_lambda" in lib.lgn_last_error()
    d.l2_lambda, d.alpha = 0.0, 1.5
    assert call(d) < 0 and b"alpha" in lib.lgn_last_error()


# ---- option matching ------------------------------------------------------------------------------------

def test_optimizer_choice_is_matched_as_the_reference_matches_it():
    fx = _fixture()
    assert S.optimizer_kind("Adam") == "adam" and S.optimizer_kind("RMSprop") == "rmsprop" and S.optimizer_kind("RMSPROP") == "rmsprop"
    assert fx["unknown_raises"] == "NotImplementedError"
    for bad in ("sgd", "adamw", "", None):
        with pytest.raises(NotImplementedError, match="Adam.*RMSprop"):
            S.optimizer_kind(bad)


def test_l2_lambda_none_or_non_positive_is_off():
    assert S.l2_weight(None) == 0.0 and S.l2_weight(0) == 0.0 and S.l2_weight(-1e-3) == 0.0 and S.l2_weight(1e-6) == 1e-6


def test_eps_defaults_follow_the_choice_and_equal_the_fixture():
    fx = _fixture()["choices"]
    assert S.optimizer_eps("adam") == fx["adam"][0]["defaults"]["eps"] == 1e-8
    assert S.optimizer_eps("rmsprop", None, torch.float64) == fx["rmsprop"][0]["defaults"]["eps"] == 1e-16
    assert S.optimizer_eps("rmsprop", None, torch.float32) == 1e-12
    assert S.optimizer_eps("rmsprop", 1e-10) == 1e-10 and S.optimizer_eps("adam", 1e-6) == 1e-6       # an explicit eps wins


def test_step_classes_take_the_options_and_refuse_an_unknown_optimizer_before_touching_the_gpu():
    import inspect
    for cls in (S.NativeTrainStep, S.CapturedModuleStep, S.TrainStep, S.ReferenceLoopStep):
        sig = inspect.signature(cls.__init__).parameters
        assert sig["optimizer_choice"].default == "adam" and sig["l2_lambda"].default == 0.0
        assert sig["rms_alpha"].default == 0.99 and sig["momentum"].default == 0.9
        assert sig["eps"].default is None
    for cls in (S.NativeTrainStep, S.CapturedModuleStep):
        assert {"optimizer_choice", "l2_lambda", "rms_alpha", "momentum"} <= S._STEP_KEYWORDS[cls]
        with pytest.raises(NotImplementedError, match="Adam.*RMSprop"):
            cls(None, None, 4, optimizer_choice="sgd")


def _cpu_models():
    import __graft_entry__ as G
    return G._models(8, (2, 2, 2, 2), (2, 2, 2, 2), torch.device("cpu"))


@pytest.mark.parametrize("choice", ["adam", "rmsprop"])
def test_reference_loop_step_hands_torch_the_reference_hyper_parameters(choice):
    fx = _fixture()
    enc, dec = _cpu_models()
    step = S.ReferenceLoopStep(enc, dec, lr=fx["args"]["lr"], native_loss=False, optimizer_choice=choice, l2_lambda=None)
    assert step.l2_lambda == 0.0
    for opt, rec in zip((step.opt_enc, step.opt_dec), fx["choices"][choice]):
        assert type(opt).__name__ == rec["type"]
        keys = ("lr", "eps", "momentum", "alpha", "centered", "weight_decay") if choice == "rmsprop" else ("lr", "eps", "betas", "weight_decay", "amsgrad")
        for k in keys:
            got = opt.defaults[k]
            assert (list(got) if isinstance(got, tuple) else got) == rec["defaults"][k], k
    with pytest.raises(NotImplementedError):
        S.ReferenceLoopStep(enc, dec, native_loss=False, optimizer_choice="sgd")


# ---- the numpy restatement against torch.optim on the CPU -----------------------------------------------------

def _gradients(n, steps, seed):
    """Random gradients whose magnitudes run from 1e-300 to 1e3, with exact zeros (dead parameters) in every step."""
    rng = np.random.default_rng(seed)
    g = rng.standard_normal((steps, n)) * 10.0 ** rng.uniform(-300, 3, size=(steps, n))
    g[:, ::7] = 0.0                      # never a gradient
    g[1::2, 3::11] = 0.0                 # a gradient in some steps only
    g[:, 1] = 1e-300 * np.array([1, -1, 1, 1, -1])[:steps]
    g[:, 2] = 1e3
    return g


# Both sides do the same handful of fp64 operations per element; they differ in where a product is fused into the addition that
# follows it (<= 1 ulp each, ~1.1e-16) and in rounding of sqrt / division inputs that differ by those ulps.  Five steps of at most
# ten such operations: 1e-13 relative is two orders above that and nine below an error in the rule itself (eps under the root, lr
# outside the buffer, a missing regulariser term all change results at the 1e-3 .. 1 level).
RTOL = 1e-13
ATOL = 1e-300                            # sums of squares of 1e-160-sized gradients are subnormal: no relative accuracy there


def _close(a, b):
    np.testing.assert_allclose(a, b, rtol=RTOL, atol=ATOL)


@pytest.mark.parametrize("momentum", [0.9, 0.0])
@pytest.mark.parametrize("l1,l2", [(0.0, 0.0), (1e-8, 0.0), (1e-8, 1e-6), (0.0, 1e-3)])
def test_numpy_rmsprop_matches_torch(momentum, l1, l2):
    n, steps, lr, alpha, eps = 257, 5, 5e-4, 0.99, 1e-16
    g = _gradients(n, steps, seed=11)
    rng = np.random.default_rng(5)
    w = rng.standard_normal(n)
    w[5] = 0.0                           # sign(0) = 0
    p = torch.nn.Parameter(torch.tensor(w))
    opt = torch.optim.RMSprop([p], lr=lr, eps=eps, momentum=momentum, alpha=alpha)
    v, buf = np.zeros(n), np.zeros(n)
    for t in range(steps):
        w0 = w.copy()
        gr = R.regularised_grad(w, g[t], l1, l2)
        w, v, buf = R.rmsprop_step(w, gr, v, buf, lr, alpha, eps, momentum)
        with torch.no_grad():
            p.grad = torch.tensor(g[t]) + l1 * torch.sign(p) + 2.0 * l2 * p
        opt.step()
        st = opt.state[p]
        _close(w, p.detach().numpy())
        # the update itself, not only the weight it is added to: w - w0 carries the rounding of w (half an ulp of |w| per side)
        upd, upd_t = w - w0, p.detach().numpy() - w0
        assert np.all(np.abs(upd - upd_t) <= RTOL * np.abs(upd_t) + 2.0 * np.spacing(np.abs(w0)))
        _close(v, st["square_avg"].numpy())
        if momentum > 0:
            _close(buf, st["momentum_buffer"].numpy())
        else:
            assert "momentum_buffer" not in st or st["momentum_buffer"] is None or not torch.is_tensor(st["momentum_buffer"]) \
                or float(st["momentum_buffer"].abs().sum()) == 0.0
            assert not buf.any()
        if l1 == 0.0 and l2 == 0.0:
            dead = np.arange(n)[::7]
            assert np.array_equal(w[dead], w0[dead])                # never a gradient, no regulariser: does not move at all


@pytest.mark.parametrize("l1,l2", [(1e-8, 0.0), (1e-8, 1e-6)])
def test_numpy_adam_matches_torch(l1, l2):
    n, steps, lr = 257, 5, 5e-4
    g = _gradients(n, steps, seed=13)
    w = np.random.default_rng(6).standard_normal(n)
    p = torch.nn.Parameter(torch.tensor(w))
    opt = torch.optim.Adam([p], lr)
    m, v = np.zeros(n), np.zeros(n)
    for t in range(steps):
        gr = R.regularised_grad(w, g[t], l1, l2)
        w, m, v = R.adam_step(w, gr, m, v, t + 1, lr)
        with torch.no_grad():
            p.grad = torch.tensor(g[t]) + l1 * torch.sign(p) + 2.0 * l2 * p
        opt.step()
        _close(w, p.detach().numpy())
        _close(m, opt.state[p]["exp_avg"].numpy())
        _close(v, opt.state[p]["exp_avg_sq"].numpy())


def test_loss_total_is_data_plus_both_norms():
    w = np.array([1.0, -2.0, 0.0, 0.5])
    assert R.loss_total(3.0, w, 0.1, 0.01) == pytest.approx(3.0 + 0.1 * 3.5 + 0.01 * 5.25, rel=1e-15)
    assert R.loss_total(3.0, w, 0.1, None) == pytest.approx(3.35, rel=1e-15)
