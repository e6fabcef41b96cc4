"""Host tests of the Sinkhorn entry points (csrc/sinkhorn.hip, lgn/sinkhorn.py, lgn.losses.SinkhornLoss): the symbols are declared,
exported and bound, the ABI is still 19, the option struct and the LDS count are the documented ones, every refusal happens before
any launch, and the Python layer checks its options and refuses CPU tensors.  No GPU."""
import ctypes
import os
import re

import pytest
import torch

import _util as U

SYMBOLS = ("lgn_sinkhorn_f64", "lgn_sinkhorn_relative_f64")


def _opts(R=1.0, beta=1.0, norm=0, periodic=0, epsilon=0.1, tol=1e-6, max_iter=10, debias=0):
    from lgn import _native as N
    return N.SinkhornOpts(N.EmdOpts(R, beta, norm, periodic), epsilon, tol, max_iter, debias)


def test_the_entry_points_are_declared_and_the_abi_is_19():
    from lgn import _native as N
    with open(os.path.join(U.ROOT, "include", "lgn_amd.h")) as f:
        header = f.read()
    lib = N.lib()
    for s in SYMBOLS:
        assert re.search(r"\bint " + s + r"\(", header), s
        assert s in N.EXPORTED_SYMBOLS and s in N._SIGNATURES and hasattr(lib, s), s
        assert list(getattr(lib, s).argtypes) == list(N._SIGNATURES[s])
    assert re.search(r"\blong long lgn_sinkhorn_lds_bytes\(", header)
    assert "lgn_sinkhorn_lds_bytes" in N.EXPORTED_SYMBOLS and "lgn_sinkhorn_lds_bytes" in N._LL_SIGNATURES
    assert len(N._SIGNATURES["lgn_sinkhorn_f64"]) == 16 and len(N._SIGNATURES["lgn_sinkhorn_relative_f64"]) == 12
    assert N.ABI_VERSION == 19 and re.search(r"#define LGN_AMD_ABI_VERSION 19\b", header) and lib.lgn_abi_version() == 19
    assert re.search(r"#define LGN_SINKHORN_ITER 16\b", header) and N.SINKHORN_ITER == 16
    assert N.SINKHORN_ITER & (N.EMD_INVALID | N.EMD_EMPTY | N.EMD_ITER | N.EMD_INFEASIBLE) == 0


def test_the_option_struct_has_the_documented_layout():
    from lgn import _native as N
    with open(os.path.join(U.ROOT, "include", "lgn_amd.h")) as f:
        header = f.read()
    assert "sizeof(lgn_sinkhorn_opts) = 48" in header and "epsilon 24, tol 32, max_iter 40," in header and "debias 44" in header
    S = N.SinkhornOpts
    assert ctypes.sizeof(S) == 48
    assert (S.base.offset, S.epsilon.offset, S.tol.offset, S.max_iter.offset, S.debias.offset) == (0, 24, 32, 40, 44)
    E = N.EmdOpts
    assert (E.R.offset, E.beta.offset, E.norm.offset, E.periodic_phi.offset) == (0, 8, 16, 20)


@pytest.mark.parametrize("n,m", [(1, 1), (1, 5), (30, 30), (63, 64), (64, 65), (81, 81), (81, 40), (82, 82), (5, 82), (191, 191)])
def test_the_lds_count_is_the_documented_sum(n, m):
    from lgn import _native as N
    from lgn import sinkhorn as K
    R = max(n, m) + 1
    ld = R | 1
    fixed, cached = 8 * (16 * R + 8), 8 * (16 * R + 8) + 8 * R * ld
    want = cached if cached <= 64 * 1024 else fixed
    assert N.lib().lgn_sinkhorn_lds_bytes(n, m) == want
    assert K.cost_in_lds(n, m) == (max(n, m) <= 81)


def test_the_lds_query_refuses_sizes_outside_the_range():
    from lgn import _native as N
    lib = N.lib()
    for n, m in ((0, 5), (5, 0), (N.EMD_NMAX + 1, 5), (5, N.EMD_NMAX + 1)):
        assert lib.lgn_sinkhorn_lds_bytes(n, m) < 0 and "outside" in N.last_error()


def test_arguments_are_refused_before_any_launch():
    """Every call below is refused by the check under test or by one before it: none can reach a launch.  A host buffer stands in
    for the device pointers past the null checks."""
    from lgn import _native as N
    lib = N.lib()
    big = N.EMD_NMAX + 1
    host = (ctypes.c_double * 8)()
    h = ctypes.cast(host, ctypes.c_void_p)

    def g(ev0=None, ev1=None, B=2, n=5, m=5, opts=None, value=None, g0=None, g1=None, status=None):
        return lib.lgn_sinkhorn_f64(ev0, ev1, B, n, m, opts, value, g0, g1, None, None, None, None, None, status, None)

    def r(recons=None, target=None, B=2, N_=30, opts=None, value=None, g_r=None, g_t=None, status=None):
        return lib.lgn_sinkhorn_relative_f64(recons, target, B, N_, opts, value, g_r, g_t, None, None, status, None)

    for kw in (dict(n=big), dict(m=big), dict(n=0), dict(m=0)):
        assert g(**kw) < 0 and "outside" in N.last_error(), kw
    assert g(B=0) < 0 and "B = 0" in N.last_error()
    assert r(N_=big) < 0 and "outside" in N.last_error()
    assert r(N_=0) < 0 and "outside" in N.last_error()
    assert r(B=0) < 0 and "B = 0" in N.last_error()
    assert g() < 0 and "null pointer" in N.last_error()
    assert r() < 0 and "null pointer" in N.last_error()
    ok = ctypes.byref(_opts())
    for missing in ("ev0", "ev1", "value", "status"):
        kw = dict(ev0=h, ev1=h, value=h, status=h, opts=ok)
        kw[missing] = None
        assert g(**kw) < 0 and "null pointer" in N.last_error(), missing
    for missing in ("recons", "target", "value", "status"):
        kw = dict(recons=h, target=h, value=h, status=h, opts=ok)
        kw[missing] = None
        assert r(**kw) < 0 and "null pointer" in N.last_error(), missing
    gok = dict(ev0=h, ev1=h, value=h, status=h)
    rok = dict(recons=h, target=h, value=h, status=h)
    assert g(**gok) < 0 and "null pointer (opts)" in N.last_error()
    assert r(**rok) < 0 and "null pointer (opts)" in N.last_error()
    assert r(**rok, g_t=h, opts=ok) < 0 and "g_target without g_recons" in N.last_error()
    inf, nan = float("inf"), float("nan")
    for what, values in (("R", (0.0, -1.0, inf, nan)), ("beta", (0.0, -2.0, inf, nan)), ("epsilon", (0.0, -0.1, inf, nan)),
                         ("tol", (-1e-9, inf, nan)), ("max_iter", (0, -3))):
        for v in values:
            o = ctypes.byref(_opts(**{what: v}))
            assert g(**gok, opts=o) < 0 and f"{what} = " in N.last_error(), (what, v)
            assert r(**rok, opts=o) < 0 and f"{what} = " in N.last_error(), (what, v)
            assert r(**rok, g_r=h, opts=o) < 0 and f"{what} = " in N.last_error(), (what, v)


def test_python_options_are_checked_on_the_host():
    from lgn import sinkhorn as K
    from lgn.losses import SinkhornLoss
    a, b = torch.rand(2, 5, 3, dtype=torch.float64), torch.rand(2, 6, 3, dtype=torch.float64)
    x, t = torch.rand(2, 5, 4, dtype=torch.float64), torch.rand(2, 5, 4, dtype=torch.float64)
    for fn in (K.sinkhorn, K.sinkhorn_grad, K.sinkhorn_differentiable):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            fn(a, b, 0.1)
    for fn in (K.sinkhorn_relative_tensor, K.sinkhorn_relative_grad):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            fn(x, t, 0.1)
    bad = (dict(epsilon=0.0), dict(epsilon=float("nan")), dict(epsilon=float("inf")), dict(tol=-1.0), dict(tol=float("inf")),
           dict(max_iter=0), dict(max_iter=2.5), dict(R=0.0), dict(beta=float("nan")))
    for kw in bad:
        full = dict(dict(epsilon=0.1), **kw)
        eps = full.pop("epsilon")
        with pytest.raises(ValueError, match="finite|integer"):
            K.sinkhorn(a, b, eps, **full)
        with pytest.raises(ValueError, match="finite|integer"):
            K.sinkhorn_relative_tensor(x, t, eps, **full)
        with pytest.raises(ValueError, match="finite|integer"):
            SinkhornLoss(**kw)
    with pytest.raises(ValueError, match="events"):
        K.sinkhorn(a, x, 0.1)
    with pytest.raises(ValueError, match="particles per event"):
        K.sinkhorn(torch.zeros(1, 192, 3), torch.zeros(1, 5, 3), 0.1)
    loss = SinkhornLoss(num_particles=30, device="cuda")
    assert (loss.epsilon, loss.max_iter, loss.tol, loss.debias) == (0.02, 200, 1e-6, True)
    assert (loss.R, loss.beta, loss.norm, loss.periodic_phi) == (1.0, 1.0, False, False) and list(loss.parameters()) == []
    assert loss.status is None and loss.iters is None and loss.err is None
    tuned = SinkhornLoss(30, "cuda", epsilon=0.5, max_iter=7, tol=0.0, debias=False, R=0.8, beta=2.0, norm=True, periodic_phi=True)
    assert (tuned.epsilon, tuned.max_iter, tuned.tol, tuned.debias, tuned.R, tuned.beta, tuned.norm, tuned.periodic_phi) == \
        (0.5, 7, 0.0, False, 0.8, 2.0, True, True)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        loss(x, t)
    with pytest.raises(ValueError, match="4-vector"):
        loss(a, a)
    assert "not a measured optimum" in " ".join(SinkhornLoss.__doc__.split())
    assert K.status_message(K.ITER).startswith("the Sinkhorn iteration") and "NaN" in K.status_message(K.INVALID | K.ITER)


def test_the_steps_take_the_module_and_the_native_calls_refuse_it():
    from lgn import step as S
    from lgn.losses import SinkhornLoss
    module = SinkhornLoss()
    assert S._module_loss(module, True, False, torch.device("cpu")) is module
    for native_emd in (False, True):
        with pytest.raises(NotImplementedError, match="loss module"):
            S._loss_desc(module, True, False, False, 4, None, native_emd=native_emd)
