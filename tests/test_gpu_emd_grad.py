"""GPU tests of the differentiable EMD (csrc/emd.hip, the GRAD kernels; lgn.emd.emd_grad / EMDFn / EMDRelativeFn, lgn.losses.EMDLoss /
HybridLoss, a loss module in the module-API steps): the gradients against a solver-free identity (the header's formulas evaluated in
numpy from the flow and the potentials the same launch returns, which are certified optimal), against the g26 fixture (LP sensitivity
on scipy's solution, known to its own finite-difference error), against closed forms, through the relative-polar frame down to
Cartesian jets, through autograd, and end to end through a training step with a directional derivative in weight space."""
import functools

import numpy as np
import pytest
import torch

import _emd_grad_ref as G
import _emd_ref as E
import _util as U

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CERT = 1e-12              # the project's certificate tolerance (tests/test_gpu_emd.py)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def host(*xs):
    return [None if x is None else x.cpu().numpy() for x in xs]


@functools.lru_cache(maxsize=None)
def fixture():
    return U.load("g26_emd_grad.npz")


def certify(ev0, ev1, val, flow, d0, d1, R):
    """The optimality certificate of tests/test_gpu_emd.py (its `certify`, on arrays already fetched): the flow is feasible, the
    potentials are feasible and the two objectives agree -- together that IS optimality (LP duality).  Bounds: 1e-12 of the total
    weight for the marginals, 1e-12 absolute for the dual constraints (costs are O(1)), 1e-12 relative for the objectives."""
    for b in range(len(ev0)):
        c, a, w = E.balanced(ev0[b], ev1[b], R)
        total = max(a.sum(), w.sum())
        f = flow[b]
        assert f.shape == c.shape and (f >= 0).all()
        assert np.abs(f.sum(1) - a).max() <= CERT * total and np.abs(f.sum(0) - w).max() <= CERT * total, b
        assert (d0[b][:, None] + d1[b][None, :] <= c + CERT).all(), (b, (d0[b][:, None] + d1[b][None, :] - c).max())
        primal, dual = (f * c).sum(), (d0[b] * a).sum() + (d1[b] * w).sum()
        assert abs(primal - dual) <= CERT * abs(primal), (b, primal, dual)
        assert abs(val[b] - primal) <= CERT * abs(primal), (b, val[b], primal)


# ---- 1. the solver-free identity -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n,m", [(1, 1), (1, 7), (5, 8), (8, 5), (12, 12), (63, 63), (64, 64), (65, 65), (86, 86), (87, 87),
                                 (191, 191)])
def test_the_gradients_are_the_formula_on_the_returned_flow_and_potentials(n, m):
    """Both flow placements (the flow fits LDS up to 86 particles, 87 is the first size in the workspace) and all three
    column-per-lane counts (the fictitious column makes 64 the first size with two, 128 with three).  The flow and the potentials of
    the GRAD launch are certified, the gradients are the header's formulas on them to 1e-12 of the largest gradient entry, and the
    value is emd()'s bit for bit."""
    from lgn import emd as M
    rng = np.random.default_rng(1000 * n + m)
    for B, R in ((6 if n < 60 else 2, 1.0), (3 if n < 60 else 2, 0.4)):
        a, b = G.events(rng, B, n), G.events(rng, B, m)
        out = M.emd_grad(dev(a), dev(b), R=R, return_flow=True, return_duals=True, return_status=True)
        val, g0, g1, flow, d0, d1, st = host(*out)
        assert (st == 0).all(), st
        assert torch.equal(out[0], M.emd(dev(a), dev(b), R=R))
        certify(a, b, val, flow, d0, d1, R)
        for k in range(B):
            w0, w1 = G.formula(a[k], b[k], flow[k], d0[k], d1[k], R)
            top = max(np.abs(w0).max(), np.abs(w1).max())
            err = max(np.abs(g0[k] - w0).max(), np.abs(g1[k] - w1).max())
            assert np.isfinite(g0[k]).all() and np.isfinite(g1[k]).all() and top > 0
            assert err <= CERT * top, (n, m, R, k, err, top)
    # one gradient alone is the same gradient, and flow and potentials are the forward call's
    only0, only1 = M.emd_grad(dev(a), dev(b), R=R, need_g1=False), M.emd_grad(dev(a), dev(b), R=R, need_g0=False)
    assert only0[2] is None and only1[1] is None and torch.equal(only0[1], out[1]) and torch.equal(only1[2], out[2])
    fwd = M.emd(dev(a), dev(b), R=R, return_flow=True, return_duals=True)
    assert all(torch.equal(x, y) for x, y in zip(fwd, (out[0], out[3], out[4], out[5])))
    assert M.flow_in_lds(max(n, m)) == (max(n, m) <= 86)


# ---- 2. the fixture ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("tag", [c[0] for c in G.GENERIC])
def test_generic_gradients_match_the_fixture(tag):
    """|gpu - g26| <= 10 fd_err of that case + 1e-12 max |g|: the oracle itself is only known to fd_err (the identity above is the
    tight check)."""
    from lgn import emd as M
    z, pre = fixture(), f"gen_{tag}_"
    val, g0, g1, st = host(*M.emd_grad(dev(z[pre + "ev0"]), dev(z[pre + "ev1"]), R=float(z[pre + "R"]), return_status=True))
    assert (st == 0).all()
    np.testing.assert_allclose(val, z[pre + "emd"], rtol=1e-12, atol=1e-300)
    top = max(np.abs(z[pre + "g0"]).max(), np.abs(z[pre + "g1"]).max())
    bound = 10 * float(z[pre + "fd_err"]) + 1e-12 * top
    err = max(np.abs(g0 - z[pre + "g0"]).max(), np.abs(g1 - z[pre + "g1"]).max())
    print(f"{tag}: |gpu - g26| = {err:.3e}, bound {bound:.3e}, max |g| {top:.3e}")
    assert err <= bound


@pytest.mark.parametrize("tag", [c[0] for c in G.REL])
def test_relative_gradients_match_the_fixture(tag):
    """N = 5, 12 with 3 zero-padded rows in both jets, 30: Cartesian gradients against g26 with the same bound; the E column is 0; the
    target's gradient is produced only when asked for; the value is emd_relative_tensor()'s bit for bit."""
    from lgn import emd as M
    z, pre = fixture(), f"rel_{tag}_"
    r, t = dev(z[pre + "recons"]), dev(z[pre + "target"])
    out = M.emd_relative_grad(r, t, need_g_target=True)
    val, gr, gt, st = host(*out)
    assert (st == 0).all()
    assert torch.equal(out[0], M.emd_relative_tensor(r, t))
    np.testing.assert_allclose(val, z[pre + "emd"], rtol=1e-11, atol=1e-300)
    top = max(np.abs(z[pre + "g_recons"]).max(), np.abs(z[pre + "g_target"]).max())
    bound = 10 * float(z[pre + "fd_err"]) + 1e-12 * top
    err = max(np.abs(gr - z[pre + "g_recons"]).max(), np.abs(gt - z[pre + "g_target"]).max())
    print(f"{tag}: |gpu - g26| = {err:.3e}, bound {bound:.3e}, max |g| {top:.3e}")
    assert err <= bound
    assert (gr[..., 0] == 0).all() and (gt[..., 0] == 0).all()
    alone = M.emd_relative_grad(r, t)
    assert alone[2] is None and torch.equal(alone[1], out[1]) and torch.equal(alone[0], out[0])
    if tag == "n12":                                                                # pT == 0: the jet-sum term only, the same for all
        assert (gr[:, 9:] == gr[:, 9:10]).all() and np.abs(gr[:, 9:]).max() > 0


def test_the_relative_gradient_on_the_workspace_path():
    """N = 100 (the flow in the workspace, two columns per lane) with 10 zero-padded rows: the REL kernel's Cartesian gradient against
    the generic GRAD kernel on the frames staged on the host, chained back by CPU autograd (tests/_emd_grad_ref.py).  Bound
    1e-10 max |g|: the host's and the device's asinh / atan2 differ by a few ulp of O(1) coordinates (the values agree to 1e-11,
    tests/test_gpu_emd.py), which moves a unit vector (y_i - y'_j) / theta_ij by ~1e-16 / theta_ij, theta_ij >~ 1e-3 here."""
    from lgn import emd as M
    r, t = G.jets(np.random.default_rng(100), 2, 100, padded=10)
    assert not M.flow_in_lds(100)
    val, gr, gt, st = host(*M.emd_relative_grad(dev(r), dev(t), need_g_target=True))
    assert (st == 0).all()
    p, q = E.relative_events(r), E.relative_events(t)
    v2, g0, g1 = host(*M.emd_grad(dev(p), dev(q)))
    np.testing.assert_allclose(val, v2, rtol=1e-11)
    for b in range(2):
        wr, wt = G._frame_backward(r[b], g0[b]), G._frame_backward(t[b], g1[b])
        top = max(np.abs(wr).max(), np.abs(wt).max())
        err = max(np.abs(gr[b] - wr).max(), np.abs(gt[b] - wt).max())
        print(f"N = 100, jet {b}: |REL - generic chained on the host| = {err:.3e}, max |g| {top:.3e}")
        assert err <= 1e-10 * top


# ---- 3. closed forms -------------------------------------------------------------------------------------------------------------------

def test_one_event_weightless():
    """The value is the other event's sum pT, its weight gradients are all 1 and every position gradient is 0."""
    from lgn import emd as M
    rng = np.random.default_rng(3)
    a, b = G.events(rng, 2, 9), G.events(rng, 2, 11)
    a[0, :, 0] = 0.0
    b[1, :, 0] = 0.0
    val, g0, g1 = host(*M.emd_grad(dev(a), dev(b)))
    np.testing.assert_allclose(val, [b[0, :, 0].sum(), a[1, :, 0].sum()], rtol=1e-12)
    assert np.abs(g1[0, :, 0] - 1.0).max() <= 1e-12 and np.abs(g0[1, :, 0] - 1.0).max() <= 1e-12
    assert (g0[..., 1:] == 0).all() and (g1[..., 1:] == 0).all()
    assert np.isfinite(g0).all() and np.isfinite(g1).all()


@pytest.mark.parametrize("n", [30, 70, 100])
def test_equal_weights_pull_along_the_assignment(n):
    """Equal weights 1 / n (100: the workspace path): the optimal flow is scipy's assignment, so a particle's position gradient is 1 / n
    times the unit vector between it and its partner."""
    from scipy.optimize import linear_sum_assignment
    from lgn import emd as M
    rng = np.random.default_rng(n)
    a, b = G.events(rng, 3, n, spread=1.0), G.events(rng, 3, n, spread=1.0)
    a[..., 0] = b[..., 0] = 1.0 / n
    val, g0, g1 = host(*M.emd_grad(dev(a), dev(b)))
    for k in range(3):
        rows, col = linear_sum_assignment(E.thetas(a[k], b[k]))
        d = a[k][rows, 1:] - b[k][col, 1:]
        unit = d / np.sqrt((d * d).sum(-1, keepdims=True)) / n
        assert np.abs(g0[k][rows, 1:] - unit).max() <= 1e-12 and np.abs(g1[k][col, 1:] + unit).max() <= 1e-12, k


def test_identical_events_and_a_nan_pair():
    from lgn import _native as N
    from lgn import emd as M
    rng = np.random.default_rng(8)
    a, b = G.events(rng, 4, 13), G.events(rng, 4, 13)
    b[1] = a[1]                                                                      # identical events: 0, every arc has theta = 0
    clean = M.emd_grad(dev(a), dev(b), return_status=True)
    val, g0, g1, st = host(*clean)
    assert (st == 0).all() and val[1] == 0.0 and np.isfinite(g0).all() and np.isfinite(g1).all()
    assert (g0[1, :, 1:] == 0).all() and (g1[1, :, 1:] == 0).all()
    bad = a.copy()
    bad[2, 4, 1] = np.nan
    out = M.emd_grad(dev(bad), dev(b), return_status=True)
    val2, h0, h1, st2 = host(*out)
    assert st2.tolist() == [0, 0, N.EMD_INVALID, 0]
    assert np.isnan(val2[2]) and np.isnan(h0[2]).all() and np.isnan(h1[2]).all()
    keep = [0, 1, 3]
    for x, y in zip(out[:3], clean[:3]):                                             # the neighbours: bit-equal to the run without it
        assert torch.equal(x[keep], y[keep])
    with pytest.raises(ValueError, match="NaN, infinity or a negative weight"):
        M.emd_grad(dev(bad), dev(b))
    rj, tj = G.jets(rng, 3, 8)
    rj[1, 2, 3] = np.inf
    v, gr, gt, s = host(*M.emd_relative_grad(dev(rj), dev(tj), need_g_target=True))
    assert s.tolist() == [0, N.EMD_INVALID, 0] and np.isnan(gr[1]).all() and np.isnan(gt[1]).all() and np.isnan(v[1])
    assert np.isfinite(gr[[0, 2]]).all() and np.isfinite(gt[[0, 2]]).all()


# ---- 4. autograd ------------------------------------------------------------------------------------------------------------------------

def test_autograd_gives_the_kernels_gradients():
    from lgn import emd as M
    from lgn.losses import ChamferLoss, EMDLoss, HybridLoss
    z = fixture()
    r, t = dev(z["rel_n12_recons"]), dev(z["rel_n12_target"])
    val, gr, gt, _ = M.emd_relative_grad(r, t, need_g_target=True)
    loss = EMDLoss(num_particles=12, device="cuda")
    x = r.clone().requires_grad_(True)
    out = loss(x, t)
    assert torch.equal(out, M.emd_relative_tensor(r, t).sum()) and (loss.status.cpu() == 0).all() and loss.status.dtype == torch.int32
    out.backward()
    assert torch.equal(x.grad, gr)
    x2, t2 = r.clone().requires_grad_(True), t.clone().requires_grad_(True)
    (3.0 * loss(x2, t2)).backward()
    assert torch.equal(x2.grad, 3.0 * gr) and torch.equal(t2.grad, 3.0 * gt)
    # per-pair upstream gradients through emd_differentiable
    a, b = dev(z["gen_5x8_ev0"]).requires_grad_(True), dev(z["gen_5x8_ev1"]).requires_grad_(True)
    w = torch.tensor([1.0, -2.0, 0.5], device=DEV, dtype=torch.float64)
    d = M.emd_differentiable(a, b)
    (d * w).sum().backward()
    v0, g0, g1 = M.emd_grad(a.detach(), b.detach())
    assert torch.equal(d.detach(), v0) and torch.equal(a.grad, g0 * w.view(3, 1, 1)) and torch.equal(b.grad, g1 * w.view(3, 1, 1))
    # the hybrid loss: the weighted sum of the two modules, values and gradients
    hybrid, chamfer = HybridLoss(chamfer_loss_weight=0.25), ChamferLoss()
    xs = [r.clone().requires_grad_(True) for _ in range(3)]
    h = hybrid(xs[0], t, jet_features=True)
    c, e = chamfer(xs[1], t, jet_features=True), loss(xs[2], t)
    assert torch.equal(h, 0.25 * c + e) and (hybrid.status.cpu() == 0).all()
    h.backward(), c.backward(), e.backward()
    U.assert_close(xs[0].grad, 0.25 * xs[1].grad + xs[2].grad, 1e-15, "hybrid gradient")


# ---- 5. end to end ----------------------------------------------------------------------------------------------------------------------

N_STEP, B_STEP = 6, 4
CH = ((2, 2, 2), (2, 2, 2))        # the tiny network of tests/test_gpu_epoch.py: maxdim 2, two channels, two levels


def _nets(n):
    import __graft_entry__ as GE
    nets = [GE._models(N_STEP, CH[0], CH[1], torch.device(DEV), seed=23, maxdim=2) for _ in range(n)]
    for enc, dec in nets:
        U.live_weights(enc, dec)                 # off the initial weights, where the reconstruction is ~1e-9
    return nets


def _batch():
    import _normalize_ref as R
    p4 = R.jets(B_STEP, N_STEP, seed=106, n_real=4)
    p4 = p4 / (p4.abs().amax(dim=(1, 2), keepdim=True) + 1e-16)
    return {"p4": p4.contiguous().to(DEV), "labels": (p4[..., 0] != 0).to(torch.uint8).to(DEV)}


def test_a_captured_step_with_the_emd_loss_trains_like_the_eager_step():
    from lgn.losses import EMDLoss
    from lgn.step import CapturedModuleStep, NativeTrainStep, TrainStep, native_train_step
    (ea, da), (eb, db) = _nets(2)
    batch = _batch()
    la_mod, lb_mod = EMDLoss(), EMDLoss()
    a = CapturedModuleStep(ea, da, batch_size=B_STEP, lr=1e-3, l1_lambda=1e-8, use_graph=True, loss_choice=la_mod)
    b = TrainStep(eb, db, lr=1e-3, l1_lambda=1e-8, loss_choice=lb_mod)
    before = a.flat.flat.clone()
    assert torch.equal(before, b.flat.flat)
    la, ra = a.step(batch)
    lb, rb = b.step(batch)
    assert (la_mod.status.cpu() == 0).all() and (lb_mod.status.cpu() == 0).all()
    assert torch.isfinite(la).all() and not torch.equal(a.flat.flat, before)
    U.assert_close(la, lb, 1e-11, "loss")
    U.assert_close(ra, rb, 1e-11, "reconstruction")
    U.assert_close(a.flat.flat, b.flat.flat, 1e-9, "parameters after one Adam step")
    with pytest.raises(NotImplementedError):
        NativeTrainStep(eb, db, batch_size=B_STEP, loss_choice=EMDLoss())
    assert isinstance(native_train_step(eb, db, B_STEP, loss_choice=EMDLoss()), CapturedModuleStep)


DIRECTIONS, H = 4, 1e-5


def _directional(module):
    """[(central difference of the loss along d, <gradient, d>)] of the eager step for DIRECTIONS random unit vectors d in weight
    space, and the loss.  H = 1e-5, near eps^(1/3): the truncation error of the central difference (~H^2) and the rounding of the two
    loss values (~2^-52 L / H) are then both ~1e-10 of the derivative's scale, for either loss."""
    from lgn.step import TrainStep
    ((enc, dec),) = _nets(1)
    batch = _batch()
    step = TrainStep(enc, dec, l1_lambda=0.0, optimizer=False, loss_choice=module)
    loss0, _ = step.forward_backward(batch)
    grad, theta = step.flat.grad.clone(), step.flat.flat.clone()
    gen = torch.Generator().manual_seed(11)
    out = []
    for _ in range(DIRECTIONS):
        delta = torch.randn(theta.shape, generator=gen, dtype=theta.dtype)
        delta = (delta / delta.norm()).to(DEV)
        vals = []
        for sign in (1.0, -1.0):
            step.flat.flat.copy_(theta + sign * H * delta)
            vals.append(step.forward_backward(batch)[0].item())
        out.append(((vals[0] - vals[1]) / (2 * H), float((grad * delta).sum())))
    step.flat.flat.copy_(theta)
    return out, loss0.item()


def test_the_directional_derivative_in_weight_space():
    """(L(theta + h d) - L(theta - h d)) / 2h against <grad, d> with the EMD loss, and with ChamferLoss as the control, on the same
    directions: the EMD's relative discrepancy (the largest over the directions, relative to the largest |<grad, d>|) may be at most
    10 x the control's."""
    from lgn.losses import ChamferLoss, EMDLoss
    rel = {}
    for name, module in (("chamfer", ChamferLoss()), ("emd", EMDLoss())):
        pairs, loss = _directional(module)
        scale = max(abs(an) for _, an in pairs)
        rel[name] = max(abs(fd - an) for fd, an in pairs) / scale
        for fd, an in pairs:
            print(f"{name}: loss {loss:.6e}, central difference {fd:.12e}, <grad, d> {an:.12e}, |difference| {abs(fd - an):.3e}")
        print(f"{name}: relative discrepancy {rel[name]:.3e}")
        assert scale > 0 and np.isfinite(rel[name])
    assert rel["emd"] <= 10 * rel["chamfer"]
