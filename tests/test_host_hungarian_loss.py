"""Host-side checks of the Hungarian-MSE / MSE training losses: the torch restatement (tests/_hungarian_ref.py) against the
reference-pinned g19 fixtures, the new C entry points' symbols and their refusals before any launch, and the --loss-choice name
matching.  No GPU needed."""
import ctypes as C

import numpy as np
import pytest
import torch

import _hungarian_ref as H
from _util import load
from lgn import _native as N

LOSS_FIXTURES = {"g19_loss_n30.npz": False, "g19_loss_n150.npz": False, "g19_loss_n30_pad.npz": True}


@pytest.mark.parametrize("frame", list(H.FRAMES))
@pytest.mark.parametrize("name", list(LOSS_FIXTURES))
def test_restatement_matches_the_reference_fixture(name, frame):
    """Where the restatement's assignment (exact costs) is the reference's (torch.cdist), per-jet loss and gradient agree to 1e-12;
    without padding that is every jet; with padded (tied) target rows at most 5 % of the jets may hold another optimum of the same
    total cost."""
    z = load(name)
    a, p = H.FRAMES[frame]
    x, t = torch.from_numpy(z["x"]), torch.from_numpy(z["t"])
    col_ref = torch.from_numpy(z[f"col.{frame}"].astype(np.int64))
    col = H.assignment(x, t, a, p)
    same = (col == col_ref).all(-1)
    share = 1.0 - same.double().mean().item()
    print(f"{name} {frame}: assignment differs on {100 * share:.2f} % of the jets")
    if LOSS_FIXTURES[name]:
        assert share <= 0.05
    else:
        assert bool(same.all())
    ca, cb = H.total_cost(x, t, col, a, p), H.total_cost(x, t, col_ref, a, p)
    np.testing.assert_allclose(ca.numpy(), cb.numpy(), rtol=1e-12, atol=0)
    # the loss scored on the REFERENCE's assignment is the reference's loss; gradients on the jets both agree on
    xx = x.clone().requires_grad_(True)
    loss = H.loss(xx, t, col_ref, a, p)
    loss.backward()
    np.testing.assert_allclose(loss.item(), float(z[f"loss.{frame}"]), rtol=1e-12)
    g_ref = torch.from_numpy(z[f"grad.{frame}"])
    scale = g_ref.abs().max().item()
    assert (xx.grad - g_ref).abs().max().item() <= 1e-12 * scale
    per_a, per_b = H.per_jet(x, t, col, a, p), H.per_jet(x, t, col_ref, a, p)
    np.testing.assert_allclose(per_a[same].numpy(), per_b[same].numpy(), rtol=1e-12, atol=0)


def test_mse_fixture_is_the_identity_assignment():
    z = load("g19_loss_n30_pad.npz")
    x, t = torch.from_numpy(z["x"]).requires_grad_(True), torch.from_numpy(z["t"])
    loss = H.mse_per_jet(x, t).sum()
    loss.backward()
    np.testing.assert_allclose(loss.item(), float(z["loss.mse"]), rtol=1e-12)
    np.testing.assert_allclose(x.grad.numpy(), z["grad.mse"], rtol=1e-12, atol=1e-300)
    ident = torch.arange(30).expand(x.shape[0], 30)
    np.testing.assert_allclose(H.loss(x.detach(), t, ident).item(), loss.item(), rtol=1e-13)


def test_new_symbols_and_unchanged_abi():
    lib = N.lib()
    assert lib.lgn_abi_version() == 19
    for name in ("lgn_step_fwd_bwd_f64", "lgn_step_train_f64", "lgn_step_eval_f64", "lgn_hungarian_mse_f64",
                 "lgn_assign_loss_lds_bytes"):
        assert hasattr(lib, name) and name in N.EXPORTED_SYMBOLS
    for name in ("lgn_step_fwd_bwd_loss_f64", "lgn_step_train_loss_f64", "lgn_step_eval_loss_f64"):     # merged into the calls above
        assert not hasattr(lib, name) and name not in N.EXPORTED_SYMBOLS
    assert 0 < lib.lgn_assign_loss_lds_bytes(30, 4) < lib.lgn_assign_loss_lds_bytes(150, 4) <= N.LDS_LIMIT
    assert lib.lgn_assign_loss_lds_bytes(192, 8) > N.LDS_LIMIT
    assert lib.lgn_assign_loss_lds_bytes(0, 4) < 0


def _desc(N_=12, jet_loss_scale=0.0, ch=4):
    d = N.NetDesc()
    d.B, d.N, d.n_levels = 2, N_, 3
    for l in range(4):
        d.enc_channels[l] = d.dec_channels[l] = ch
    d.tau_s, d.tau_v, d.mlp_hidden_mul, d.mlp_nlin = 1, 8, 6, 7
    d.get_real, d.jet_loss_scale = 1, jet_loss_scale
    return d


def _call(d, ld, which="train"):
    lib = N.lib()
    ldp = C.byref(ld) if ld is not None else None
    if which == "eval":
        return lib.lgn_step_eval_f64(C.byref(d), *([None] * 8), 0, *([None] * 5), ldp, None, None, None)
    return lib.lgn_step_fwd_bwd_f64(C.byref(d), None, None, 0, *([None] * 7), 0, None, None, ldp, None, None, None)


def _loss(kind, scale=1e-3, a=1, p=0):
    ld = N.LossDesc()
    ld.kind, ld.abs_coord, ld.polar_coord, ld.scale = kind, a, p, scale
    return ld


@pytest.mark.parametrize("which", ["train", "eval"])
def test_plan_time_refusals_come_with_a_message(which):
    lib = N.lib()
    # loss = NULL and kind = Chamfer are the plain call: they get as far as its own null-pointer check
    for ld in (None, _loss(N.LOSS_CHAMFER)):
        assert _call(_desc(), ld, which) < 0 and b"null pointer" in lib.lgn_last_error()
    assert _call(_desc(), _loss(7), which) < 0 and b"kind=7" in lib.lgn_last_error()
    assert _call(_desc(jet_loss_scale=0.25), _loss(N.LOSS_HUNGARIAN), which) < 0 and b"jet_loss_scale" in lib.lgn_last_error()
    assert _call(_desc(), _loss(N.LOSS_MSE, scale=0.0), which) < 0 and b"scale" in lib.lgn_last_error()
    assert _call(_desc(N_=200), _loss(N.LOSS_HUNGARIAN), which) < 0 and b"N = 200" in lib.lgn_last_error()
    assert _call(_desc(N_=190, ch=8), _loss(N.LOSS_HUNGARIAN), which) < 0 and b"LDS" in lib.lgn_last_error()
    # a good descriptor passes the loss checks and stops at the plain call's null-pointer check
    assert _call(_desc(), _loss(N.LOSS_HUNGARIAN, a=0, p=1), which) < 0 and b"null pointer" in lib.lgn_last_error()


def test_standalone_loss_refuses_bad_arguments():
    lib = N.lib()
    assert lib.lgn_hungarian_mse_f64(0, 4, None, None, 2, 1, 0, 1.0, None, None, None, None, None) < 0
    assert lib.lgn_hungarian_mse_f64(1, 4, None, None, 2, 1, 0, 1.0, None, None, None, None, None) < 0
    assert b"null" in lib.lgn_last_error()


def test_loss_choice_names_match_as_get_loss_does():
    from lgn.losses import loss_columns, loss_kind
    assert loss_kind("ChamferLoss") == N.LOSS_CHAMFER and loss_kind("chamfer") == N.LOSS_CHAMFER
    assert loss_kind("hungarian") == N.LOSS_HUNGARIAN and loss_kind("jet") == N.LOSS_HUNGARIAN
    assert loss_kind("MSE") == N.LOSS_MSE
    assert loss_kind("hungarian_mse") == N.LOSS_MSE            # the reference tests 'mse' before 'hungarian'
    assert loss_kind("chamfer+mse") == N.LOSS_CHAMFER           # ... and 'chamfer' first
    for name in ("emd", "hybrid", "combined", "mix", "EMD", "bogus"):
        with pytest.raises(NotImplementedError, match="chamfer.*mse.*hungarian"):
            loss_kind(name)
    assert loss_columns(N.LOSS_MSE) == 4 and loss_columns(N.LOSS_HUNGARIAN, True, False) == 4
    assert loss_columns(N.LOSS_HUNGARIAN, True, True) == 3 and loss_columns(N.LOSS_HUNGARIAN, False, False) == 3


def test_module_loss_refuses_cpu_tensors():
    from lgn.losses import HungarianMSELoss
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        HungarianMSELoss()(torch.zeros(1, 3, 4, dtype=torch.float64), torch.zeros(1, 3, 4, dtype=torch.float64))
