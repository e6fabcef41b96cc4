"""GPU tests of the EMD gradients under energyflow's options (csrc/emd_grad_opts.hip; the beta, norm and periodic_phi keywords of
lgn.emd.emd_grad / emd_differentiable / emd_relative_grad / emd_relative_tensor, lgn.emd.emds_differentiable, lgn.losses.EMDLoss /
HybridLoss): the gradients against a solver-free identity (the header's formulas evaluated in numpy from the flow and the potentials
the same launch returns, which are certified optimal under the options), against the g27 fixture (LP sensitivity on scipy's solution,
known to its own finite-difference error), the default options against the calls without options bit for bit, the relative form
against the generic one, the identities the distance obeys, statuses, autograd, a captured training step, graph capture, and the
matrix form."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import _emd_grad_ref as G
import _emd_opts_grad_ref as GO
import _emd_pairs_ref as P
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
    return U.load("g27_emd_opts_grad.npz")


def _pair(rng, B, n, m, o):
    periodic = bool(o.get("periodic_phi"))
    return GO.events(rng, B, n, periodic), GO.events(rng, B, m, periodic)


# ---- 1. the solver-free identity -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("opt", list(GO.OPTIONS))
@pytest.mark.parametrize("n,m", [(1, 1), (1, 7), (5, 8), (8, 5), (12, 12), (64, 64), (87, 87), (128, 128), (191, 191)])
def test_the_gradients_are_the_formula_on_the_returned_flow_and_potentials(n, m, opt):
    """Both flow placements (LDS up to 86 particles) and all three column-per-lane counts (64 is the first size with two, 128 with
    three).  The flow and the potentials of the launch are certified under the options, the gradients are the header's formulas on
    them to 1e-12 of the largest gradient entry, the value is emd(..., options) bit for bit, and one gradient alone is the same
    gradient."""
    from lgn import emd as M
    o = GO.OPTIONS[opt]
    rng = np.random.default_rng(1000 * n + m)
    B = 6 if n < 60 else 2
    a, b = _pair(rng, B, n, m, o)
    out = M.emd_grad(dev(a), dev(b), return_flow=True, return_duals=True, return_status=True, **o)
    val, g0, g1, flow, d0, d1, st = host(*out)
    assert (st == 0).all(), st
    assert torch.equal(out[0], M.emd(dev(a), dev(b), **o))
    for k in range(B):
        P.certify(val[k], flow[k], d0[k], d1[k], a[k], b[k], **o)
        w0, w1 = GO.formula(a[k], b[k], flow[k], d0[k], d1[k], **o)
        top = max(np.abs(w0).max(), np.abs(w1).max())
        err = max(np.abs(g0[k] - w0).max(), np.abs(g1[k] - w1).max())
        assert np.isfinite(g0[k]).all() and np.isfinite(g1[k]).all() and top > 0
        assert err <= CERT * top, (n, m, opt, k, err, top)
    only0, only1 = M.emd_grad(dev(a), dev(b), need_g1=False, **o), M.emd_grad(dev(a), dev(b), need_g0=False, **o)
    assert only0[2] is None and only1[1] is None and torch.equal(only0[1], out[1]) and torch.equal(only1[2], out[2])
    assert torch.equal(only0[0], out[0]) and torch.equal(only1[0], out[0])
    fwd = M.emd(dev(a), dev(b), return_flow=True, return_duals=True, **o)
    assert all(torch.equal(x, y) for x, y in zip(fwd, (out[0], out[3], out[4], out[5])))


# ---- 2. the fixture ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("tag,opt", GO.GENERIC)
def test_generic_gradients_match_the_fixture(tag, opt):
    """|gpu - g27| <= 10 fd_err of that case + 1e-12 max |g|: the oracle itself is only known to fd_err (the identity above is the
    tight check)."""
    from lgn import emd as M
    z, pre = fixture(), f"gen_{tag}_{opt}_"
    o = GO.case_options(tag, opt)
    val, g0, g1, st = host(*M.emd_grad(dev(z[pre + "ev0"]), dev(z[pre + "ev1"]), return_status=True, **o))
    assert (st == 0).all()
    np.testing.assert_allclose(val, z[pre + "emd"], rtol=1e-12, atol=1e-300)
    top = max(np.abs(z[pre + "g0"]).max(), np.abs(z[pre + "g1"]).max())
    bound = 10 * float(z[pre + "fd_err"]) + 1e-12 * top
    err = max(np.abs(g0 - z[pre + "g0"]).max(), np.abs(g1 - z[pre + "g1"]).max())
    print(f"{tag} {opt}: |gpu - g27| = {err:.3e}, bound {bound:.3e}, max |g| {top:.3e}")
    assert err <= bound


@pytest.mark.parametrize("tag,opt", GO.REL)
def test_relative_gradients_match_the_fixture(tag, opt):
    """N = 5, 12 with 3 zero-padded rows in both jets, 30: Cartesian gradients against g27 with the same bound; the E column is 0; the
    target's gradient is produced only when asked for; the value is emd_relative_tensor(..., options) bit for bit."""
    from lgn import emd as M
    z, pre = fixture(), f"rel_{tag}_{opt}_"
    o = GO.OPTIONS[opt]
    r, t = dev(z[pre + "recons"]), dev(z[pre + "target"])
    out = M.emd_relative_grad(r, t, need_g_target=True, **o)
    val, gr, gt, st = host(*out)
    assert (st == 0).all()
    assert torch.equal(out[0], M.emd_relative_tensor(r, t, **o))
    np.testing.assert_allclose(val, z[pre + "emd"], rtol=1e-11, atol=1e-300)
    top = max(np.abs(z[pre + "g_recons"]).max(), np.abs(z[pre + "g_target"]).max())
    bound = 10 * float(z[pre + "fd_err"]) + 1e-12 * top
    err = max(np.abs(gr - z[pre + "g_recons"]).max(), np.abs(gt - z[pre + "g_target"]).max())
    print(f"{tag} {opt}: |gpu - g27| = {err:.3e}, bound {bound:.3e}, max |g| {top:.3e}")
    assert err <= bound
    assert (gr[..., 0] == 0).all() and (gt[..., 0] == 0).all()
    alone = M.emd_relative_grad(r, t, **o)
    assert alone[2] is None and torch.equal(alone[1], out[1]) and torch.equal(alone[0], out[0])


# ---- 3. the default options are the calls without options ---------------------------------------------------------------------------------

def _c_grad_opts(a, b, opts, flow_too=True):
    from lgn import _native as N
    B, n, m = a.shape[0], a.shape[1], b.shape[1]
    f64 = dict(device=DEV, dtype=torch.float64)
    out = [torch.full((B,), -1.0, **f64), torch.full((B, n, 3), -1.0, **f64), torch.full((B, m, 3), -1.0, **f64),
           torch.full((B, n + 1, m + 1), -1.0, **f64), torch.full((B, n + 1), -1.0, **f64), torch.full((B, m + 1), -1.0, **f64)]
    st = torch.full((B,), -1, device=DEV, dtype=torch.int32)
    nbytes = N.lib().lgn_emd_workspace_bytes(B, max(n, m))
    work = torch.empty(max(nbytes, 8), device=DEV, dtype=torch.uint8)
    rc = N.lib().lgn_emd_grad_opts_f64(N.ptr(a), N.ptr(b), B, n, m, opts, *[N.ptr(x) for x in out], N.ptr(st), N.ptr(work), work.numel(),
                                       N.stream_ptr())
    assert rc == 0, N.last_error()
    return out + [st]


def _c_relative_opts(r, t, opts, grads=True):
    from lgn import _native as N
    B, n = r.shape[0], r.shape[1]
    f64 = dict(device=DEV, dtype=torch.float64)
    val, st = torch.full((B,), -1.0, **f64), torch.full((B,), -1, device=DEV, dtype=torch.int32)
    gr, gt = (torch.full((B, n, 4), -1.0, **f64), torch.full((B, n, 4), -1.0, **f64)) if grads else (None, None)
    nbytes = N.lib().lgn_emd_workspace_bytes(B, n)
    work = torch.empty(max(nbytes, 8), device=DEV, dtype=torch.uint8)
    rc = N.lib().lgn_emd_relative_opts_f64(N.ptr(r), N.ptr(t), B, n, opts, N.ptr(val), N.ptr(gr), N.ptr(gt), N.ptr(st), N.ptr(work),
                                           work.numel(), N.stream_ptr())
    assert rc == 0, N.last_error()
    return val, gr, gt, st


@pytest.mark.parametrize("n,m", [(5, 8), (100, 100)])
def test_default_options_give_the_bits_of_the_calls_without_options(n, m):
    from lgn import _native as N
    from lgn import emd as M
    rng = np.random.default_rng(n)
    a, b = dev(G.events(rng, 3, n)), dev(G.events(rng, 3, m))
    for R in (1.0, 0.4):
        old = M.emd_grad(a, b, R=R, return_flow=True, return_duals=True, return_status=True)
        kw = M.emd_grad(a, b, R=R, return_flow=True, return_duals=True, return_status=True, beta=1.0, norm=False, periodic_phi=False)
        assert all(torch.equal(x, y) for x, y in zip(old, kw))
        for opts in ([None] if R == 1.0 else []) + [ctypes.byref(N.EmdOpts(R, 1.0, 0, 0))]:
            assert all(torch.equal(x, y) for x, y in zip(old, _c_grad_opts(a, b, opts))), R
    N_ = min(n, m) if n < 50 else 100
    r, t = (dev(x) for x in G.jets(rng, 3, N_, padded=2))
    old = M.emd_relative_grad(r, t, need_g_target=True)
    kw = M.emd_relative_grad(r, t, need_g_target=True, R=1.0, beta=1.0, norm=False, periodic_phi=False)
    assert all(torch.equal(x, y) for x, y in zip(old, kw))
    score = M.emd_relative_tensor(r, t, return_status=True)
    for opts in (None, ctypes.byref(N.EmdOpts(1.0, 1.0, 0, 0))):
        assert all(torch.equal(x, y) for x, y in zip(old, _c_relative_opts(r, t, opts)))
        val, _, _, st = _c_relative_opts(r, t, opts, grads=False)
        assert torch.equal(val, score[0]) and torch.equal(st, score[1])
    x = r.clone().requires_grad_(True)
    from lgn.losses import EMDLoss
    EMDLoss()(x, t).backward()
    assert torch.equal(x.grad, old[1])


# ---- 4. the relative form against the generic one -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("opt", ["all", "norm"])
@pytest.mark.parametrize("N_,padded", [(12, 3), (100, 10)])
def test_the_relative_form_is_the_generic_one_on_the_frames(N_, padded, opt):
    """The frames staged on the host, the generic kernel under the same options, the chain back by CPU autograd
    (tests/_emd_grad_ref.py); N = 100 is the workspace path.  Bound 1e-10 max |g|, as tests/test_gpu_emd_grad.py argues it: the host's
    and the device's asinh / atan2 differ by a few ulp of O(1) coordinates, which moves a unit vector by ~1e-16 / theta_ij."""
    from lgn import emd as M
    o = GO.OPTIONS[opt]
    r, t = G.jets(np.random.default_rng(N_), 2, N_, padded=padded)
    assert M.flow_in_lds(N_) == (N_ <= 86)
    val, gr, gt, st = host(*M.emd_relative_grad(dev(r), dev(t), need_g_target=True, **o))
    assert (st == 0).all()
    p, q = E.relative_events(r), E.relative_events(t)
    v2, g0, g1 = host(*M.emd_grad(dev(p), dev(q), **o))
    np.testing.assert_allclose(val, v2, rtol=1e-11)
    for b in range(2):
        wr, wt = G._frame_backward(r[b], g0[b]), G._frame_backward(t[b], g1[b])
        top = max(np.abs(wr).max(), np.abs(wt).max())
        err = max(np.abs(gr[b] - wr).max(), np.abs(gt[b] - wt).max())
        print(f"N = {N_} {opt}, jet {b}: |REL - generic chained on the host| = {err:.3e}, max |g| {top:.3e}")
        assert err <= 1e-10 * top
        assert (gr[b][:, 0] == 0).all() and (gt[b][:, 0] == 0).all()


# ---- 5. identities ----------------------------------------------------------------------------------------------------------------------

def _seam_free(rng, B, n, m):
    """periodic events whose phi differences stay 0.1 pi clear of |D| = pi, on both sides of it: the first event within
    [0, 0.45 pi], the second there or within [1.55 pi, 2 pi)"""
    a, b = G.events(rng, B, n), G.events(rng, B, m)
    a[..., 2] = rng.random((B, n)) * 0.45 * np.pi
    b[..., 2] = rng.random((B, m)) * 0.45 * np.pi + np.where(rng.random((B, m)) < 0.5, 1.55 * np.pi, 0.0)
    return a, b


@pytest.mark.parametrize("opt", list(GO.OPTIONS))
@pytest.mark.parametrize("n", [12, 87])
def test_homogeneity_and_translation(n, opt):
    """The identities of tests/test_host_emd_opts_grad.py on the device's outputs, to 1e-12 of the sum of the absolute terms: degree 0
    in each event's weights under norm, degree 1 in all the weights without it, and no change under a common shift of y or of phi."""
    from lgn import emd as M
    o = GO.OPTIONS[opt]
    rng = np.random.default_rng(n)
    a, b = _seam_free(rng, 2, n, n) if o.get("periodic_phi") else (G.events(rng, 2, n), G.events(rng, 2, n))
    val, g0, g1 = host(*M.emd_grad(dev(a), dev(b), **o))
    for k in range(2):
        t0, t1 = a[k, :, 0] * g0[k, :, 0], b[k, :, 0] * g1[k, :, 0]
        if o.get("norm"):
            assert abs(t0.sum()) <= CERT * np.abs(t0).sum() and abs(t1.sum()) <= CERT * np.abs(t1).sum(), (t0.sum(), t1.sum())
        else:
            assert abs(t0.sum() + t1.sum() - val[k]) <= CERT * (np.abs(t0).sum() + np.abs(t1).sum()), (t0.sum() + t1.sum(), val[k])
        for c in (1, 2):
            assert abs(g0[k, :, c].sum() + g1[k, :, c].sum()) <= CERT * (np.abs(g0[k, :, c]).sum() + np.abs(g1[k, :, c]).sum()), c


# ---- 6. statuses ------------------------------------------------------------------------------------------------------------------------

def test_a_flagged_pair_is_nan_and_leaves_its_neighbours_alone():
    from lgn import _native as N
    from lgn import emd as M
    rng = np.random.default_rng(8)
    a, b = G.events(rng, 4, 13), G.events(rng, 4, 13)
    o = GO.OPTIONS["all"]
    clean = M.emd_grad(dev(a), dev(b), return_status=True, **o)
    assert (clean[3] == 0).all()
    bad = a.copy()
    bad[2, 4, 1] = np.nan                                                            # LGN_EMD_INVALID
    light = b.copy()
    light[0, :, 0] = 0.0                                                             # under norm: LGN_EMD_EMPTY
    out = M.emd_grad(dev(bad), dev(light), return_status=True, **o)
    val, h0, h1, st = host(*out)
    assert st.tolist() == [N.EMD_EMPTY, 0, N.EMD_INVALID, 0]
    for k in (0, 2):
        assert np.isnan(val[k]) and np.isnan(h0[k]).all() and np.isnan(h1[k]).all()
    for x, y in zip(out[:3], clean[:3]):                                             # the neighbours: bit-equal to the run without them
        assert torch.equal(x[[1, 3]], y[[1, 3]])
    with pytest.raises(ValueError, match="weightless and cannot be normalised"):
        M.emd_grad(dev(a), dev(light), **o)
    # without norm one weightless event is well defined, also at beta = 2
    val, g0, g1, st = host(*M.emd_grad(dev(a), dev(light), return_status=True, beta=2.0))
    assert (st == 0).all() and np.isfinite(g0).all() and np.isfinite(g1).all()
    np.testing.assert_allclose(val[0], a[0, :, 0].sum(), rtol=1e-12)
    rj, tj = G.jets(rng, 3, 8)
    rj[1, 2, 3] = np.inf
    tj[2, :, 1:3] = 0.0                                                              # no pT: weightless under norm
    v, gr, gt, s = host(*M.emd_relative_grad(dev(rj), dev(tj), need_g_target=True, **o))
    assert s.tolist() == [0, N.EMD_INVALID, N.EMD_EMPTY]
    assert np.isnan(v[1:]).all() and np.isnan(gr[1:]).all() and np.isnan(gt[1:]).all()
    assert np.isfinite(v[0]) and np.isfinite(gr[0]).all() and np.isfinite(gt[0]).all()


# ---- 7. autograd ------------------------------------------------------------------------------------------------------------------------

def test_autograd_gives_the_kernels_gradients():
    from lgn import emd as M
    from lgn.losses import EMDLoss, HybridLoss
    z = fixture()
    o = dict(beta=2.0, norm=True)
    a, b = dev(z["gen_5x8_beta2_ev0"]).requires_grad_(True), dev(z["gen_5x8_beta2_ev1"]).requires_grad_(True)
    w = torch.tensor([1.0, -2.0, 0.5], device=DEV, dtype=torch.float64)
    d = M.emd_differentiable(a, b, **o)
    (d * w).sum().backward()
    v0, g0, g1 = M.emd_grad(a.detach(), b.detach(), **o)
    assert torch.equal(d.detach(), v0) and torch.equal(a.grad, g0 * w.view(3, 1, 1)) and torch.equal(b.grad, g1 * w.view(3, 1, 1))
    r, t = dev(z["rel_n12_beta2_recons"]), dev(z["rel_n12_beta2_target"])
    val, gr, gt, _ = M.emd_relative_grad(r, t, need_g_target=True, **o)
    loss = EMDLoss(num_particles=12, device="cuda", **o)
    x = r.clone().requires_grad_(True)
    out = loss(x, t)
    assert torch.equal(out, M.emd_relative_tensor(r, t, **o).sum()) and torch.equal(out, val.sum()) and (loss.status.cpu() == 0).all()
    out.backward()
    assert torch.equal(x.grad, gr)
    x2, t2 = r.clone().requires_grad_(True), t.clone().requires_grad_(True)
    (3.0 * loss(x2, t2)).backward()
    assert torch.equal(x2.grad, 3.0 * gr) and torch.equal(t2.grad, 3.0 * gt)
    assert not torch.equal(gr, M.emd_relative_grad(r, t)[1])                         # (the options do change the gradient)
    hybrid = HybridLoss(0.25, **o)
    x3 = r.clone().requires_grad_(True)
    hybrid(x3, t).backward()
    x4 = r.clone().requires_grad_(True)
    (0.25 * hybrid.chamfer(x4, t) + loss(x4, t)).backward()
    U.assert_close(x3.grad, x4.grad, 1e-15, "hybrid gradient")


# ---- 8. a captured step -----------------------------------------------------------------------------------------------------------------

N_STEP, B_STEP = 6, 4
CH = ((2, 2, 2), (2, 2, 2))        # the tiny network of tests/test_gpu_emd_grad.py


def _nets(n):
    import __graft_entry__ as GE
    nets = [GE._models(N_STEP, CH[0], CH[1], torch.device(DEV), seed=23, maxdim=2) for _ in range(n)]
    for enc, dec in nets:
        U.live_weights(enc, dec)
    return nets


def _batch():
    import _normalize_ref as R
    p4 = R.jets(B_STEP, N_STEP, seed=106, n_real=4)
    p4 = p4 / (p4.abs().amax(dim=(1, 2), keepdim=True) + 1e-16)
    return {"p4": p4.contiguous().to(DEV), "labels": (p4[..., 0] != 0).to(torch.uint8).to(DEV)}


def test_a_captured_step_with_the_option_loss_trains_like_the_eager_step():
    from lgn.losses import EMDLoss
    from lgn.step import CapturedModuleStep, NativeTrainStep, TrainStep
    (ea, da), (eb, db) = _nets(2)
    batch = _batch()
    la_mod, lb_mod = EMDLoss(beta=2.0, norm=True), EMDLoss(beta=2.0, norm=True)
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
        NativeTrainStep(eb, db, batch_size=B_STEP, loss_choice=EMDLoss(beta=2.0))


# ---- 9. capture -----------------------------------------------------------------------------------------------------------------------

def test_a_captured_call_replays_the_eager_bits():
    from lgn import emd as M
    rng = np.random.default_rng(11)
    o = GO.OPTIONS["all"]
    a, b = (dev(x) for x in _pair(rng, 5, 10, 14, o))
    eager = M.emd_grad(a, b, return_status=True, **o)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        M.emd_grad(a, b, return_status=True, **o)            # warm-up outside the capture
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            out = M.emd_grad(a, b, return_status=True, **o)  # (return_status: no host sync, which a capture does not admit)
    torch.cuda.current_stream().wait_stream(side)
    for _ in range(2):
        for x in out:
            x.fill_(-1)
        graph.replay()
        torch.cuda.synchronize()
        assert all(torch.equal(x, y) for x, y in zip(out, eager))


# ---- 10. the matrix form ------------------------------------------------------------------------------------------------------------------

def _pairwise(X0, X1, W, sym, o):
    """(g of X0, g of X1) of sum_ij W_ij emd(X0[i], X1[j]) from one emd_grad call per pair, the terms summed on the host: over the
    columns for X0, over the rows for X1 (sym: both roles of X0 added, the diagonal left out), and the sums of the absolute terms"""
    from lgn import emd as M
    B0, B1 = len(X0), len(X1)
    t0, t1 = np.zeros((B0, B1) + X0.shape[1:]), np.zeros((B0, B1) + X1.shape[1:])
    for i in range(B0):
        for j in range(B1):
            if sym and i == j:
                continue
            _, g0, g1 = host(*M.emd_grad(dev(X0[i]), dev(X1[j]), **o))
            t0[i, j], t1[i, j] = g0 * W[i, j], g1 * W[i, j]
    s0, s1, a0, a1 = t0.sum(1), t1.sum(0), np.abs(t0).sum(1), np.abs(t1).sum(0)
    return (s0 + s1, None, a0 + a1, None) if sym else (s0, s1, a0, a1)


@pytest.mark.parametrize("B0,B1", [(3, 4), (1, 4), (3, 1), (4, None)])
def test_the_matrix_form_sums_the_pair_gradients(B0, B1):
    """emds_differentiable: forward is emds() bit for bit; backward under a random upstream matrix is the weighted sum of the per-pair
    emd_grad results -- to the bit for a side whose sums have one term (the other side has a single event), else within
    (T + 1) 2^-52 of the sum of the absolute terms (T terms, whose order in the sum is the device's here and numpy's there, each
    order good to (T - 1) 2^-53 of that sum) -- and two runs are bit-equal.  B1 = None is the symmetric form."""
    from lgn import emd as M
    o = dict(R=0.8, beta=2.0, norm=True)
    sym = B1 is None
    rng = np.random.default_rng(10 * B0 + (B1 or 0))
    X0 = G.events(rng, B0, 5)
    X1 = X0 if sym else G.events(rng, B1, 8)
    W = rng.normal(size=(B0, len(X1)))
    runs = []
    for _ in range(2):
        x0, x1 = dev(X0).requires_grad_(True), (None if sym else dev(X1).requires_grad_(True))
        out = M.emds_differentiable(x0, x1, chunk_pairs=2 * len(X1), **o)            # (two rows of the matrix per chunk)
        assert torch.equal(out.detach(), M.emds(dev(X0), None if sym else dev(X1), **o))
        (out * dev(W)).sum().backward()
        runs.append((x0.grad.clone(), None if sym else x1.grad.clone()))
    assert torch.equal(runs[0][0], runs[1][0]) and (sym or torch.equal(runs[0][1], runs[1][1]))
    s0, s1, a0, a1 = _pairwise(X0, X1, W, sym, o)
    got = [runs[0][0].cpu().numpy()] + ([] if sym else [runs[0][1].cpu().numpy()])
    for g, s, a, terms in zip(got, (s0, s1), (a0, a1), (2 * (B0 - 1) if sym else B1, B0)):
        if terms == 1:                                                               # (one term per sum: nothing to reorder)
            assert np.array_equal(g, s)
        else:
            assert (np.abs(g - s) <= (terms + 1) * 2.0 ** -52 * a).all(), np.abs(g - s).max()
