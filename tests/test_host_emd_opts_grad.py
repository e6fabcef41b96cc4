"""Host tests of the EMD gradients under energyflow's options: the restatement tests/_emd_opts_grad_ref.py (LP sensitivity on scipy's
HiGHS solution of the option LP) is pinned to central differences of tests/_emd_pairs_ref.emd, to closed forms and to the identities
the distance obeys (homogeneity in the weights, translation); it reproduces the g27 fixture; the two entry points are declared,
exported and refuse bad arguments before any launch, the ABI is still 19; the Python keywords are checked on the host.  No GPU."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import _emd_grad_ref as G
import _emd_opts_grad_ref as GO
import _emd_pairs_ref as P
import _util as U

SYMBOLS = ("lgn_emd_grad_opts_f64", "lgn_emd_relative_opts_f64")
# Central differences at h = 1e-6 are known to h^2 |E'''| ~ 1e-12 .. 1e-10 plus 2^-52 E / h ~ 2e-10 of rounding, ~1e-9 of the largest
# entry over the grid below (measured: <= 1.6e-9); a wrong formula is off by O(1) of it.
FD_REL_BOUND = 1e-7
# The identities hold exactly for the exact LP solution; HiGHS returns a vertex to its feasibility tolerances (1e-10 of the scaled
# weights), which enters each term once.
IDENTITY_BOUND = 1e-9


def _events(seed, n, m, periodic):
    rng = np.random.default_rng(seed)
    return GO.events(rng, 1, n, periodic)[0], GO.events(rng, 1, m, periodic)[0]


# ---- 1. the restatement against central differences of the option LP -------------------------------------------------------------------

@pytest.mark.parametrize("beta", [0.5, 1.0, 1.5, 2.0])
@pytest.mark.parametrize("n,m", [(5, 8), (6, 6), (1, 7)])
def test_the_gradient_is_the_central_difference_of_the_option_lp(n, m, beta):
    worst = 0.0
    for R in (1.0, 0.8):
        for norm in (False, True):
            for periodic in (False, True):
                o = dict(R=R, beta=beta, norm=norm, periodic_phi=periodic)
                a, b = _events(100 * n + m, n, m, periodic)
                value, g0, g1 = GO.emd_grad(a, b, **o)
                f0, f1 = GO.fd_events(a, b, h=1e-6, **o)
                top = max(np.abs(g0).max(), np.abs(g1).max())
                err = max(np.abs(g0 - f0).max(), np.abs(g1 - f1).max())
                worst = max(worst, err / top)
                assert err <= FD_REL_BOUND * top, (o, err, top)
                assert abs(value - P.emd(a, b, **o)) <= 1e-12 * value
    print(f"{n}x{m}, beta = {beta}: worst |formula - central difference| / max |g| = {worst:.3e}")


# ---- 2. closed forms -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("beta", [0.5, 1.0, 1.5, 2.0])
def test_two_particles_under_norm(beta):
    """One particle each: the normalised weights are 1 and 1, E = theta^beta, dE/dy_0 = beta theta^(beta - 2) dy / R^2, and no weight
    moves the distance."""
    R = 0.8
    a, b = np.array([[3.0, 0.3, -0.2]]), np.array([[0.7, -0.4, 0.5]])
    dy, dp = a[0, 1] - b[0, 1], a[0, 2] - b[0, 2]
    theta = np.sqrt(dy * dy + dp * dp) / R
    value, g0, g1 = GO.emd_grad(a, b, R=R, beta=beta, norm=True)
    k = beta * theta ** (beta - 2.0) / (R * R)
    np.testing.assert_allclose(value, theta ** beta, rtol=1e-13)
    np.testing.assert_allclose(g0[0], [0.0, k * dy, k * dp], rtol=1e-13, atol=1e-15)
    np.testing.assert_allclose(g1[0], [0.0, -k * dy, -k * dp], rtol=1e-13, atol=1e-15)


def test_the_periodic_sign_across_the_seam():
    """phi = 0.1 against 2 pi - 0.1: the minimum image is 0.2 across the seam, so raising phi_0 lengthens it"""
    a, b = np.array([[1.0, 0.0, 0.1]]), np.array([[1.0, 0.0, 2.0 * np.pi - 0.1]])
    value, g0, g1 = GO.emd_grad(a, b, periodic_phi=True)
    np.testing.assert_allclose(value, 0.2, rtol=1e-12)
    np.testing.assert_allclose([g0[0, 2], g1[0, 2]], [1.0, -1.0], rtol=1e-13)
    assert g0[0, 1] == 0.0 and g1[0, 1] == 0.0


# ---- 3. identities ----------------------------------------------------------------------------------------------------------------------

def _clear_of_the_seam(a, b):
    D = np.abs(a[:, None, 2] - b[None, :, 2])
    return np.abs(D - np.pi).min() > 1e-3


@pytest.mark.parametrize("opt", list(GO.OPTIONS))
@pytest.mark.parametrize("n,m", [(5, 8), (12, 12)])
def test_homogeneity_and_translation(n, m, opt):
    """norm: the distance has degree 0 in each event's weights, sum pT dE/dpT = 0 per event.  Without: degree 1 in all the weights
    jointly (the costs do not move), sum pT dE/dpT + sum pT' dE/dpT' = E at every beta.  A common shift of y, or of phi, moves
    nothing: the position gradients of the two events cancel (periodic_phi: away from |D| = pi, where the image has a kink)."""
    o = GO.OPTIONS[opt]
    seed = 1000 * n + m
    a, b = _events(seed, n, m, o.get("periodic_phi", False))
    while o.get("periodic_phi") and not _clear_of_the_seam(a, b):
        seed += 1
        a, b = _events(seed, n, m, True)
    value, g0, g1 = GO.emd_grad(a, b, **o)
    t0, t1 = a[:, 0] * g0[:, 0], b[:, 0] * g1[:, 0]
    if o.get("norm"):
        assert abs(t0.sum()) <= IDENTITY_BOUND * np.abs(t0).sum() and abs(t1.sum()) <= IDENTITY_BOUND * np.abs(t1).sum()
    else:
        assert abs(t0.sum() + t1.sum() - value) <= IDENTITY_BOUND * (np.abs(t0).sum() + np.abs(t1).sum())
    for c in (1, 2):
        assert abs(g0[:, c].sum() + g1[:, c].sum()) <= IDENTITY_BOUND * (np.abs(g0[:, c]).sum() + np.abs(g1[:, c]).sum()), c


# ---- 4. the fixture ---------------------------------------------------------------------------------------------------------------------

def test_the_restatement_reproduces_the_fixture():
    z = U.load("g27_emd_opts_grad.npz")
    assert len(GO.GENERIC) == 28 and len(GO.REL) == 9
    for tag, opt in GO.GENERIC:
        a, b, o = GO.generic_case(tag, opt)
        pre = f"gen_{tag}_{opt}_"
        assert np.array_equal(a, z[pre + "ev0"]) and np.array_equal(b, z[pre + "ev1"])
        top = max(np.abs(z[pre + "g0"]).max(), np.abs(z[pre + "g1"]).max())
        assert 0 < float(z[pre + "fd_err"]) <= FD_REL_BOUND * top, (tag, opt)
        value, g0, g1 = GO.emd_grad(a[0], b[0], **o)                                 # (the first pair: the others are the generator's)
        assert abs(value - z[pre + "emd"][0]) <= 1e-12 * value
        assert np.abs(g0 - z[pre + "g0"][0]).max() <= 1e-11 * top and np.abs(g1 - z[pre + "g1"][0]).max() <= 1e-11 * top, (tag, opt)
    for tag, opt in GO.REL:
        r, t = G.rel_case(tag)
        pre = f"rel_{tag}_{opt}_"
        assert np.array_equal(r, z[pre + "recons"]) and np.array_equal(t, z[pre + "target"])
        top = max(np.abs(z[pre + "g_recons"]).max(), np.abs(z[pre + "g_target"]).max())
        assert 0 < float(z[pre + "fd_err"]) <= FD_REL_BOUND * top, (tag, opt)
        assert (z[pre + "g_recons"][..., 0] == 0).all() and (z[pre + "g_target"][..., 0] == 0).all()
        if tag == "n5":
            value, gr, gt = GO.emd_relative_grad(r, t, **GO.OPTIONS[opt])
            np.testing.assert_allclose(value, z[pre + "emd"], rtol=1e-12)
            assert np.abs(gr - z[pre + "g_recons"]).max() <= 1e-11 * top and np.abs(gt - z[pre + "g_target"]).max() <= 1e-11 * top


# ---- 5. ABI and refusals ----------------------------------------------------------------------------------------------------------------

def test_the_entry_points_are_declared_and_the_abi_is_19():
    from lgn import _native as N
    with open(os.path.join(U.ROOT, "include", "lgn_amd.h")) as f:
        header = f.read()
    lib = N.lib()
    for s in SYMBOLS:
        assert re.search(r"\bint " + s + r"\(", header), s
        assert s in N.EXPORTED_SYMBOLS and s in N._SIGNATURES and hasattr(lib, s), s
        assert list(getattr(lib, s).argtypes) == list(N._SIGNATURES[s])
    assert len(N._SIGNATURES["lgn_emd_grad_opts_f64"]) == 16 and len(N._SIGNATURES["lgn_emd_relative_opts_f64"]) == 12
    assert N.ABI_VERSION == 19 and re.search(r"#define LGN_AMD_ABI_VERSION 19\b", header) and lib.lgn_abi_version() == 19
    assert ctypes.sizeof(N.EmdOpts) == 24
    assert "Gradients under the options are not offered" not in header


def test_arguments_are_refused_before_any_launch():
    """As tests/test_host_emd_pairs.py, calls that cannot reach a launch whatever the check under test does: up to the null check every
    pointer is null; the checks after it are given a host buffer with n = 150 and no workspace, which the last check refuses.  Only the
    workspace checks themselves stand alone."""
    from lgn import _native as N
    lib = N.lib()
    big = N.EMD_NMAX + 1

    def g(ev0=None, ev1=None, B=2, n=5, m=5, opts=None, emd=None, g0=None, g1=None, flow=None, d0=None, d1=None, status=None, work=None,
          work_bytes=0):
        return lib.lgn_emd_grad_opts_f64(ev0, ev1, B, n, m, opts, emd, g0, g1, flow, d0, d1, status, work, work_bytes, None)

    def r(recons=None, target=None, B=2, N_=30, opts=None, emd=None, g_r=None, g_t=None, status=None, work=None, work_bytes=0):
        return lib.lgn_emd_relative_opts_f64(recons, target, B, N_, opts, emd, g_r, g_t, status, work, work_bytes, None)

    for kw in (dict(n=big), dict(m=big), dict(n=0), dict(m=0)):
        assert g(**kw) < 0 and "outside" in N.last_error(), kw
    assert g(B=0) < 0 and "B = 0" in N.last_error()
    assert g() < 0 and "no gradient output" in N.last_error()
    assert r(N_=big) < 0 and "outside" in N.last_error()
    assert r(N_=0) < 0 and "outside" in N.last_error()
    assert r(B=0) < 0 and "B = 0" in N.last_error()
    assert r() < 0 and "null pointer" in N.last_error()
    # past the null checks: a host buffer stands in for the device pointers; every call below is refused before it would be used
    host = (ctypes.c_double * 8)()
    h = ctypes.cast(host, ctypes.c_void_p)
    assert g(g0=h) < 0 and "null pointer" in N.last_error()
    for missing in ("ev0", "ev1", "emd", "status"):
        kw = dict(ev0=h, ev1=h, emd=h, status=h, g1=h)
        kw[missing] = None
        assert g(**kw) < 0 and "null pointer" in N.last_error(), missing
    for missing in ("recons", "target", "emd", "status"):
        kw = dict(recons=h, target=h, emd=h, status=h)
        kw[missing] = None
        assert r(**kw) < 0 and "null pointer" in N.last_error(), missing
    gok = dict(ev0=h, ev1=h, emd=h, status=h, g0=h, n=150, m=150)
    rok = dict(recons=h, target=h, emd=h, status=h, N_=150)
    assert g(**dict(gok, g0=None)) < 0 and "no gradient output" in N.last_error()
    assert r(**rok, g_t=h) < 0 and "g_target without g_recons" in N.last_error()
    for R in (0.0, -1.0, float("inf"), float("nan")):
        o = ctypes.byref(N.EmdOpts(R, 1.0, 0, 0))
        assert g(**gok, opts=o) < 0 and "R = " in N.last_error(), R
        assert r(**rok, opts=o) < 0 and "R = " in N.last_error(), R
    for beta in (0.0, -2.0, float("inf"), float("nan")):
        o = ctypes.byref(N.EmdOpts(1.0, beta, 0, 0))
        assert g(**gok, opts=o) < 0 and "beta = " in N.last_error(), beta
        assert r(**rok, g_r=h, opts=o) < 0 and "beta = " in N.last_error(), beta
    # n = 150 keeps the flow in a workspace: missing, short, misaligned -- with options, without, and on the value-only form
    need = lib.lgn_emd_workspace_bytes(2, 150)
    assert need == 2 * 151 * 151 * 8
    for o in (None, ctypes.byref(N.EmdOpts(1.0, 1.0, 0, 0)), ctypes.byref(N.EmdOpts(0.8, 2.0, 1, 1))):
        assert g(**gok, opts=o) < 0 and "null work" in N.last_error()
        assert r(**rok, opts=o) < 0 and "null work" in N.last_error()
        assert r(**rok, g_r=h, opts=o) < 0 and "null work" in N.last_error()
        assert g(**gok, opts=o, work=h, work_bytes=need - 8) < 0 and "too short" in N.last_error()
        assert r(**rok, opts=o, work=h, work_bytes=need - 8) < 0 and "too short" in N.last_error()
        odd = ctypes.c_void_p(h.value + 4)
        assert g(**gok, opts=o, work=odd, work_bytes=need) < 0 and "aligned" in N.last_error()
        assert r(**rok, opts=o, work=odd, work_bytes=need) < 0 and "aligned" in N.last_error()


# ---- 6. Python ----------------------------------------------------------------------------------------------------------------------------

def test_python_keywords_are_checked_on_the_host():
    from lgn import emd as M
    from lgn.losses import EMDLoss, HybridLoss
    a, b = torch.rand(2, 5, 3, dtype=torch.float64), torch.rand(2, 6, 3, dtype=torch.float64)
    x, t = torch.rand(2, 5, 4, dtype=torch.float64), torch.rand(2, 5, 4, dtype=torch.float64)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        M.emd_grad(a, b, beta=2.0, norm=True)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        M.emd_differentiable(a, b, beta=2.0, periodic_phi=True)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        M.emd_relative_grad(x, t, beta=2.0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        M.emd_relative_tensor(x, t, norm=True)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        M.emds_differentiable(a, b, beta=2.0)
    for kw in (dict(beta=0.0), dict(beta=float("nan")), dict(beta=float("inf")), dict(R=0.0, norm=True), dict(R=-1.0, beta=2.0)):
        with pytest.raises(ValueError, match="finite"):
            M.emd_grad(a, b, **kw)
        with pytest.raises(ValueError, match="finite"):
            M.emd_differentiable(a, b, **kw)
        with pytest.raises(ValueError, match="finite"):
            M.emd_relative_grad(x, t, **kw)
        with pytest.raises(ValueError, match="finite"):
            M.emd_relative_tensor(x, t, **kw)
        with pytest.raises(ValueError, match="finite"):
            EMDLoss(**kw)
    loss = EMDLoss(num_particles=30, device="cuda", beta=2.0)
    assert (loss.R, loss.beta, loss.norm, loss.periodic_phi) == (1.0, 2.0, False, False) and list(loss.parameters()) == []
    plain = EMDLoss(30, "cuda")
    assert (plain.R, plain.beta, plain.norm, plain.periodic_phi) == (1.0, 1.0, False, False)
    h = HybridLoss(2.5, norm=True)
    assert h.chamfer_loss_weight == 2.5 and h.emd.norm is True and h.emd.beta == 1.0
    for fn in (loss, h):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            fn(x, t)


def test_the_loss_names_and_the_whole_step_calls_keep_refusing():
    from lgn import step as S
    from lgn.losses import EMDLoss, HybridLoss, loss_kind
    for name in ("emd", "hybrid"):
        with pytest.raises(NotImplementedError, match="not implemented in this build"):
            loss_kind(name)
    for module in (EMDLoss(beta=2.0), HybridLoss(norm=True)):
        assert S._module_loss(module, True, False, torch.device("cpu")) is module
        with pytest.raises(NotImplementedError, match="module API"):
            S._loss_desc(module, True, False, False, 4, None)
