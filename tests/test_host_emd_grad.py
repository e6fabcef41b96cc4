"""Host tests of the differentiable EMD's yardstick, ABI and refusals: the gradient restatement tests/_emd_grad_ref.py (LP sensitivity
on scipy's HiGHS solution) is pinned to central differences of the LP restatement tests/_emd_ref.py and reproduces the g26 fixture;
the two new entry points are declared, exported and refuse bad arguments before any launch, the ABI is still 19; CPU tensors are
refused by emd_grad, EMDLoss and HybridLoss; the loss names 'emd' and 'hybrid' and the whole-step native calls keep refusing.  No GPU."""
import os
import re

import numpy as np
import pytest
import torch

import _emd_grad_ref as G
import _util as U

SYMBOLS = ("lgn_emd_grad_f64", "lgn_emd_relative_grad_f64")
FD_BOUND = 1e-8           # measured: 4e-10 (events, h = 1e-6), 1e-9 (jets, h = 1e-5); the gradients are 1e-2 .. 1 in size


# ---- 1. the restatement against central differences of the LP ------------------------------------------------------------------------

@pytest.mark.parametrize("tag", [c[0] for c in G.GENERIC])
def test_the_event_gradient_is_the_central_difference_of_the_lp(tag):
    a, b, R = G.generic_case(tag)
    value, g0, g1 = G.emd_grad(a[0], b[0], R)
    f0, f1 = G.fd_events(a[0], b[0], R, h=1e-6)
    err = max(np.abs(g0 - f0).max(), np.abs(g1 - f1).max())
    print(f"{tag}: |formula - central difference| = {err:.3e}, max |g| = {max(np.abs(g0).max(), np.abs(g1).max()):.3e}")
    assert err <= FD_BOUND
    assert abs(value - G.E.emd(a[0], b[0], R)) <= 1e-13 * value


@pytest.mark.parametrize("N,padded", [(6, 0), (12, 3), (5, 0)])
def test_the_jet_gradient_is_the_central_difference_of_the_relative_lp(N, padded):
    r, t = G.jets(np.random.default_rng(N), 1, N, padded)
    if padded:
        assert (t[:, N - padded:] == 0).all() and (r[:, N - padded:] == 0).all()
    value, gr, gt = G.emd_relative_grad(r, t)
    fr, ft, mask = G.fd_relative(r[0], t[0], h=1e-5)
    assert mask.sum() == 2 * (N - padded)
    err = max(np.abs(gr[0] - fr)[mask[0]].max(), np.abs(gt[0] - ft)[mask[1]].max())
    print(f"N = {N}: |formula - central difference| = {err:.3e}, max |g| = {max(np.abs(gr).max(), np.abs(gt).max()):.3e}")
    assert err <= FD_BOUND
    assert (gr[..., 0] == 0).all() and (gt[..., 0] == 0).all()                      # E does not enter the frame
    for g, m in ((gr[0], mask[0]), (gt[0], mask[1])):                               # pT == 0: the jet-sum term only, one vector for all
        if (~m).any():
            assert np.abs(g[~m]).max() > 0 and (g[~m] == g[~m][0]).all()
    assert abs(value[0] - G.E.emd_relative(r, t)[0]) <= 1e-13 * value[0]


def test_the_restatement_reproduces_the_fixture():
    z = U.load("g26_emd_grad.npz")
    for tag, n, m, R in G.GENERIC:
        a, b, R_ = G.generic_case(tag)
        pre = f"gen_{tag}_"
        assert np.array_equal(a, z[pre + "ev0"]) and np.array_equal(b, z[pre + "ev1"]) and R_ == float(z[pre + "R"]) == R
        assert a.shape == (G.GENERIC_PAIRS, n, 3) and b.shape == (G.GENERIC_PAIRS, m, 3)
        assert 0 < float(z[pre + "fd_err"]) <= FD_BOUND, tag
        for i in range(len(a)):
            value, g0, g1 = G.emd_grad(a[i], b[i], R)
            scale = max(np.abs(z[pre + "g0"][i]).max(), np.abs(z[pre + "g1"][i]).max())
            assert abs(value - z[pre + "emd"][i]) <= 1e-12 * value
            assert np.abs(g0 - z[pre + "g0"][i]).max() <= 1e-11 * scale and np.abs(g1 - z[pre + "g1"][i]).max() <= 1e-11 * scale, tag
    S0, S1 = z["gen_7x7_balanced_ev0"][..., 0].sum(-1), z["gen_7x7_balanced_ev1"][..., 0].sum(-1)
    np.testing.assert_allclose(S1 - S0, 1e-3, rtol=1e-9)
    for tag, N, padded in G.REL:
        r, t = G.rel_case(tag)
        pre = f"rel_{tag}_"
        assert np.array_equal(r, z[pre + "recons"]) and np.array_equal(t, z[pre + "target"]) and r.shape == (G.REL_JETS, N, 4)
        assert 0 < float(z[pre + "fd_err"]) <= FD_BOUND, tag
        if tag == "n30":
            continue                                                                # (the largest: its numbers are the generator's)
        value, gr, gt = G.emd_relative_grad(r, t)
        scale = max(np.abs(z[pre + "g_recons"]).max(), np.abs(z[pre + "g_target"]).max())
        np.testing.assert_allclose(value, z[pre + "emd"], rtol=1e-12)
        assert np.abs(gr - z[pre + "g_recons"]).max() <= 1e-11 * scale and np.abs(gt - z[pre + "g_target"]).max() <= 1e-11 * scale, tag


# ---- 2. ABI and refusals ----------------------------------------------------------------------------------------------------------------

def test_the_entry_points_are_declared_and_the_abi_is_19():
    from lgn import _native as N
    with open(os.path.join(U.ROOT, "include", "lgn_amd.h")) as f:
        header = f.read()
    lib = N.lib()
    for s in SYMBOLS:
        assert re.search(r"\bint " + s + r"\(", header), s
        assert s in N.EXPORTED_SYMBOLS and s in N._SIGNATURES and hasattr(lib, s), s
    assert N.ABI_VERSION == 19 and re.search(r"#define LGN_AMD_ABI_VERSION 19\b", header) and lib.lgn_abi_version() == 19
    assert len(N._SIGNATURES["lgn_emd_grad_f64"]) == 16 and len(N._SIGNATURES["lgn_emd_relative_grad_f64"]) == 11
    assert len(N._SIGNATURES["lgn_emd_f64"]) == 14 and len(N._SIGNATURES["lgn_emd_relative_f64"]) == 9          # untouched


def test_arguments_are_refused_before_any_launch():
    """Only calls that cannot reach a launch whatever the other checks do: every pointer is null, so even if the check under test
    regressed the null-pointer check would still refuse the call."""
    from lgn import _native as N
    lib = N.lib()
    big = N.EMD_NMAX + 1
    g = lambda B, n, m, R=1.0: lib.lgn_emd_grad_f64(None, None, B, n, m, R, *([None] * 8), 0, None)             # noqa: E731
    r = lambda B, n: lib.lgn_emd_relative_grad_f64(None, None, B, n, *([None] * 5), 0, None)                     # noqa: E731
    assert g(2, big, 5) < 0 and "outside" in N.last_error()
    assert g(2, 5, big) < 0 and "outside" in N.last_error()
    assert g(2, 0, 5) < 0 and "outside" in N.last_error()
    assert g(0, 5, 5) < 0 and "B = 0" in N.last_error()
    assert g(2, 5, 5) < 0 and "no gradient output" in N.last_error()              # checked before the other pointers
    assert r(2, big) < 0 and "outside" in N.last_error()
    assert r(0, 30) < 0 and "B = 0" in N.last_error()
    assert r(2, 30) < 0 and "null pointer" in N.last_error()
    assert lib.lgn_emd_workspace_bytes(2, 150) == 2 * 151 * 151 * 8               # the GRAD kernels need no more than the forward ones


def test_cpu_tensors_and_wrong_shapes_are_refused():
    from lgn import emd as M
    from lgn.losses import EMDLoss, HybridLoss
    a, b = torch.rand(2, 5, 3, dtype=torch.float64), torch.rand(2, 6, 3, dtype=torch.float64)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        M.emd_grad(a, b)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        M.emd_differentiable(a, b)
    with pytest.raises(ValueError, match=r"\(B, n, 3\)"):
        M.emd_grad(a, torch.rand(2, 6, 4, dtype=torch.float64))
    with pytest.raises(ValueError, match="191"):
        M.emd_grad(torch.rand(1, 192, 3, dtype=torch.float64), b[:1])
    with pytest.raises(ValueError, match="finite R"):
        M.emd_grad(a, b, R=0.0)
    with pytest.raises(ValueError, match="at least one"):
        M.emd_grad(a, b, need_g0=False, need_g1=False)
    x, t = torch.rand(2, 5, 4, dtype=torch.float64), torch.rand(2, 5, 4, dtype=torch.float64)
    loss = EMDLoss(num_particles=5, device="cpu")                                   # as get_loss() writes it: taken and ignored
    assert loss.status is None and list(loss.parameters()) == []
    for fn in (loss, EMDLoss(), HybridLoss(chamfer_loss_weight=0.5), HybridLoss()):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            fn(x, t)
    with pytest.raises(ValueError, match="p4_recons must be a 4-vector. Got: p4_recons.shape="):
        loss(x[..., :3], t)
    with pytest.raises(ValueError, match="p4_target must be a 4-vector. Got: p4_target.shape="):
        loss(x, t[..., :3])


def test_the_loss_names_and_the_whole_step_calls_keep_refusing():
    from lgn import step as S
    from lgn.losses import ChamferLoss, EMDLoss, HybridLoss, loss_kind
    for name in ("emd", "EMD", "hybrid", "combined", "mix"):
        with pytest.raises(NotImplementedError, match="not implemented in this build"):
            loss_kind(name)
    for module in (EMDLoss(), HybridLoss()):
        assert S._module_loss(module, True, False, torch.device("cpu")) is module      # used as it is
        assert S._loss_weight(module, 1) == 1.0 and S._loss_weight(module, 8) == 1.0    # sums over the jets, like Chamfer
        with pytest.raises(NotImplementedError, match="module API"):
            S._loss_desc(module, True, False, False, 4, None)
        with pytest.raises(ValueError, match="chamfer_jet_features"):
            S._module_loss(module, True, False, torch.device("cpu"), jet_features=True)
    assert isinstance(S._module_loss("chamfer", True, False, torch.device("cpu")), ChamferLoss)       # strings: as before
    assert S._loss_weight("chamfer", 4) == 1.0 and S._loss_weight("mse", 4) == 0.25
    h = HybridLoss(chamfer_loss_weight=2.5)
    assert h.chamfer_loss_weight == 2.5 and isinstance(h.chamfer, ChamferLoss) and isinstance(h.emd, EMDLoss)
