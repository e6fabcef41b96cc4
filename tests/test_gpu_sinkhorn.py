"""GPU tests of the Sinkhorn calls (csrc/sinkhorn.hip, lgn/sinkhorn.py, lgn.losses.SinkhornLoss) against the numpy restatement
tests/_sinkhorn_ref.py: value, potentials, plan, marginal error, both gradient forms and the Cartesian gradients at EQUAL iteration
counts; the bits (run to run, batch size and position, value-only call, graph replay); the exact EMD of the device as the lower
bound; the status bits; the loss module in the module-API steps.

Every case that stops by tol is chosen (on the CPU, seeds fixed below) so that on the restatement every problem of every pair stops
at an err below tol S / 4 after errs above 4 tol S only: a last-bit difference cannot move the count.  That asks for a contraction
of more than 16 per iteration, hence the large epsilon of these cases (4 .. 256 against costs of order 1 .. 15); the cases at
tol = 0 cover a small epsilon over a fixed count.

Tolerance per quantity: 64 x the spread between the two float64 variants of the restatement on the same input, plus
8 (n + m + 2) 2^-53 x the quantity's scale (S max C for the value, S for plan and err, max C for potentials and event gradients, the
restatement's own largest entry for the Cartesian gradients)."""
import numpy as np
import pytest
import torch

import _emd_grad_ref as G
import _sinkhorn_ref as S

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
B = 5
OPTS = {"default": {}, "beta2": dict(beta=2.0), "all": dict(R=0.8, beta=2.0, norm=True, periodic_phi=True)}
REAL = {(6, 6): 4}
# (n, m, option set, debias) -> (seed of _sinkhorn_ref.batch, epsilon, tol); 81 | 82: the last size with the cost in LDS | the first
# without; 63 x 64 | 64 x 65: one | two rows per lane; 191: three, and the recompute path
CASES = {
    (1, 1, "default", False): (1010, 4.0, 1e-3), (1, 1, "default", True): (1010, 4.0, 1e-3),
    (1, 1, "beta2", False): (1010, 4.0, 1e-3), (1, 1, "beta2", True): (1010, 4.0, 1e-3),
    (1, 1, "all", False): (1010, 4.0, 1e-3), (1, 1, "all", True): (1010, 4.0, 1e-3),
    (1, 5, "default", False): (1050, 4.0, 3.981e-11), (1, 5, "default", True): (1051, 16.0, 5.623e-10),
    (1, 5, "beta2", False): (1050, 8.0, 2.818e-08), (1, 5, "beta2", True): (1051, 16.0, 1.585e-06),
    (1, 5, "all", False): (1050, 4.0, 1e-3), (1, 5, "all", True): (1050, 64.0, 8.913e-10),
    (6, 6, "default", False): (6060, 4.0, 5.623e-10), (6, 6, "default", True): (6060, 16.0, 1.413e-11),
    (6, 6, "beta2", False): (6060, 4.0, 5.623e-09), (6, 6, "beta2", True): (6082, 16.0, 7.079e-07),
    (6, 6, "all", False): (6071, 16.0, 2.239e-10), (6, 6, "all", True): (6060, 256.0, 1.995e-10),
    (30, 30, "default", False): (30300, 4.0, 1.122e-07), (30, 30, "default", True): (30300, 16.0, 4.467e-10),
    (30, 30, "beta2", False): (30300, 4.0, 3.548e-11), (30, 30, "beta2", True): (30302, 8.0, 5.623e-11),
    (30, 30, "all", False): (30300, 64.0, 3.548e-10), (30, 30, "all", True): (30300, 64.0, 7.079e-08),
    (63, 64, "default", False): (63640, 4.0, 1.585e-10), (63, 64, "default", True): (63640, 4.0, 7.943e-08),
    (63, 64, "beta2", False): (63640, 4.0, 7.943e-07), (63, 64, "beta2", True): (63640, 16.0, 5.012e-10),
    (63, 64, "all", False): (63647, 16.0, 3.548e-05), (63, 64, "all", True): (63640, 64.0, 1.122e-10),
    (64, 65, "default", False): (64650, 4.0, 1.122e-10), (64, 65, "default", True): (64650, 4.0, 1e-07),
    (64, 65, "beta2", False): (64650, 8.0, 1.778e-08), (64, 65, "beta2", True): (64650, 16.0, 1.122e-09),
    (64, 65, "all", False): (64653, 16.0, 3.981e-05), (64, 65, "all", True): (64650, 64.0, 1.778e-10),
    (81, 81, "default", False): (81810, 4.0, 1e-10), (81, 81, "default", True): (81810, 4.0, 8.913e-08),
    (81, 81, "beta2", False): (81810, 8.0, 3.548e-08), (81, 81, "beta2", True): (81810, 16.0, 1.413e-09),
    (81, 81, "all", False): (81822, 16.0, 1.995e-05), (81, 81, "all", True): (81810, 64.0, 3.162e-10),
    (82, 82, "default", False): (82820, 4.0, 1.413e-10), (82, 82, "default", True): (82820, 4.0, 1.259e-07),
    (82, 82, "beta2", False): (82820, 4.0, 2.512e-09), (82, 82, "beta2", True): (82820, 8.0, 4.467e-08),
    (82, 82, "all", False): (82830, 16.0, 1.122e-06), (82, 82, "all", True): (82820, 64.0, 1.122e-10),
    (191, 191, "default", False): (192910, 4.0, 3.981e-11), (191, 191, "default", True): (192910, 4.0, 7.079e-08),
    (191, 191, "beta2", False): (192910, 4.0, 1.122e-09), (191, 191, "beta2", True): (192910, 8.0, 2.239e-11),
    (191, 191, "all", False): (192910, 64.0, 1e-10), (191, 191, "all", True): (192910, 64.0, 1e-10),
}
MAX_ITER = 8
QUANTITIES = ("value", "f", "g", "plan", "err", "g0", "g1")
WORST = {}


def _dev(x):
    return torch.tensor(np.asarray(x), device=DEV)


def _cpu(t):
    return t.detach().cpu().numpy()


def _scales(a, b, o):
    import _emd_pairs_ref as P
    C, wa, wb = P.balanced(a, b, **o)
    Ssum = max(wa.sum(), wb.sum())
    return dict(value=Ssum * C.max(), plan=Ssum, err=Ssum, f=C.max(), g=C.max(), g0=C.max(), g1=C.max())


def _compare(what, a, b, eps, kw, o, got):
    """one batch against both variants of the restatement; got: the dict of device results"""
    n, m = a.shape[1], b.shape[1]
    for i in range(len(a)):
        r0 = S.sinkhorn(a[i], b[i], eps, variant=0, **kw, **o)
        r1 = S.sinkhorn(a[i], b[i], eps, variant=1, **kw, **o)
        assert r0["iters"] == r1["iters"], (what, i, "the two restatements disagree on the count")
        assert int(got["iters"][i]) == r0["iters"], (what, i, int(got["iters"][i]), r0["iters"])
        assert int(got["status"][i]) == r0["status"], (what, i, int(got["status"][i]), r0["status"])
        scale = _scales(a[i], b[i], o)
        for q in QUANTITIES:
            spread = float(np.abs(np.asarray(r0[q]) - np.asarray(r1[q])).max())
            bound = 64 * spread + 8 * (n + m + 2) * 2.0 ** -53 * scale[q]
            dev = float(np.abs(_cpu(got[q][i]) - np.asarray(r0[q])).max())
            WORST[q] = max(WORST.get(q, 0.0), dev / bound)
            assert dev <= bound, f"{what}, pair {i}, {q}: |device - restatement| = {dev:.3e} > {bound:.3e} (spread {spread:.3e})"


def _run(a, b, eps, kw, o):
    from lgn import sinkhorn as K
    keys = ("value", "g0", "g1", "f", "g", "plan", "iters", "err", "status")
    out = K.sinkhorn_grad(_dev(a), _dev(b), eps, return_potentials=True, return_plan=True, return_info=True, return_status=True, **kw, **o)
    torch.cuda.synchronize()
    return dict(zip(keys, out))


@pytest.mark.parametrize("case", list(CASES), ids=["{}x{}-{}-{}".format(n, m, o, "debias" if d else "plain") for n, m, o, d in CASES])
def test_the_call_is_the_restatement_at_equal_iteration_counts(case):
    n, m, opt, debias = case
    seed, eps, tol = CASES[case]
    o = OPTS[opt]
    a, b = S.batch(seed, B, n, m, REAL.get((n, m)), o.get("periodic_phi", False))
    hist = S.histories(a, b, eps, MAX_ITER, debias, **o)
    assert S.tol_is_safe(hist, tol), "the case does not keep its distance from tol on the restatement"
    kw = dict(max_iter=MAX_ITER, tol=tol, debias=debias)
    got = _run(a, b, eps, kw, o)
    assert int(got["status"].abs().max()) == 0
    _compare(str(case), a, b, eps, kw, o, got)
    print(f"{case}: iterations {got['iters'].tolist()}; worst |device - restatement| / bound so far "
          + ", ".join(f"{q} {v:.3f}" for q, v in WORST.items()))


@pytest.mark.parametrize("opt", list(OPTS))
@pytest.mark.parametrize("n,m,real", [(6, 6, 4), (30, 30, 17), (64, 65, None), (82, 82, None)])
def test_a_small_epsilon_over_a_fixed_count(n, m, real, opt):
    """tol = 0: the count is max_iter whatever the last bits are; epsilon = 0.1 times the largest cost, 25 iterations, debias"""
    o = OPTS[opt]
    a, b = S.batch(7000 + n, B, n, m, real, o.get("periodic_phi", False))
    eps = 0.1 * (1.0 if opt == "default" else (2.0 if opt == "beta2" else 15.0))
    kw = dict(max_iter=25, tol=0.0, debias=True)
    got = _run(a, b, eps, kw, o)
    assert int(got["status"].abs().max()) == 0 and (got["iters"] == 25).all()
    _compare(f"{n}x{m} {opt} fixed count", a, b, eps, kw, o, got)


@pytest.mark.parametrize("opt", list(OPTS))
@pytest.mark.parametrize("N,pad", [(6, 2), (30, 0), (64, 0)])
def test_the_relative_call_carries_the_gradients_back_to_the_jets(N, pad, opt):
    """lgn_sinkhorn_relative_f64 against the restatement on host-staged frames, and against lgn_sinkhorn_f64 on those frames.  No
    device call stages the frames alone with the kernel's own bits (the host's asinh and atan2 differ from the device's in the last
    bits), so the second comparison is held to the tolerance of the first, not to torch.equal."""
    import _emd_ref as E
    from lgn import sinkhorn as K
    o = OPTS[opt]
    rec, tgt = G.jets(np.random.default_rng(300 + N), B, N, pad)
    eps = 1.0 if opt == "default" else (2.0 if opt == "beta2" else 15.0)
    kw = dict(max_iter=6, tol=0.0, debias=True)
    value, g_r, g_t, iters, err, status = K.sinkhorn_relative_grad(_dev(rec), _dev(tgt), eps, need_g_target=True, **kw, **o)
    only = K.sinkhorn_relative_tensor(_dev(rec), _dev(tgt), eps, **kw, **o)
    p, q = E.relative_events(rec), E.relative_events(tgt)
    frames = K.sinkhorn(_dev(p), _dev(q), eps, **kw, **o)
    torch.cuda.synchronize()
    assert int(status.abs().max()) == 0 and (iters == 6).all() and torch.equal(only, value)
    assert (g_r[..., 0] == 0).all() and (g_t[..., 0] == 0).all()
    for i in range(B):
        r0 = S.sinkhorn_relative(rec[i], tgt[i], eps, variant=0, **kw, **o)
        r1 = S.sinkhorn_relative(rec[i], tgt[i], eps, variant=1, **kw, **o)
        scale = _scales(p[i], q[i], o)["value"]
        bound = 64 * abs(r0["value"] - r1["value"]) + 8 * (2 * N + 2) * 2.0 ** -53 * scale
        assert abs(float(value[i]) - r0["value"]) <= bound and abs(float(frames[i]) - float(value[i])) <= bound, (i, bound)
        assert abs(float(err[i]) - r0["err"]) <= 64 * abs(r0["err"] - r1["err"]) + 8 * (2 * N + 2) * 2.0 ** -53 * r0["S"]
        for got, key in ((g_r[i], "g_recons"), (g_t[i], "g_target")):
            top = np.abs(r0[key]).max()
            bound = 64 * np.abs(r0[key] - r1[key]).max() + 8 * (2 * N + 2) * 2.0 ** -53 * top
            dev = np.abs(_cpu(got) - r0[key]).max()
            assert dev <= bound, f"N = {N}, {opt}, jet {i}, {key}: {dev:.3e} > {bound:.3e}"


# ---- bits ---------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n,m", [(30, 30), (64, 65), (82, 82)])
def test_the_bits_depend_on_nothing_but_the_pair(n, m):
    """run to run; the batch size and the pair's place in it (B = 5 leaves the last workgroup partly filled, 1 and 7 change every
    pair's workgroup and wave); the value-only call; a captured graph"""
    from lgn import sinkhorn as K
    a, b = S.batch(900 + n, 7, n, m, None)
    o = dict(max_iter=12, tol=1e-7, debias=True, beta=2.0)
    A_, B_ = _dev(a), _dev(b)
    keys = ("value", "g0", "g1", "f", "g", "plan", "iters", "err", "status")
    full = K.sinkhorn_grad(A_, B_, 0.5, return_potentials=True, return_plan=True, return_info=True, return_status=True, **o)
    again = K.sinkhorn_grad(A_, B_, 0.5, return_potentials=True, return_plan=True, return_info=True, return_status=True, **o)
    for k, x, y in zip(keys, full, again):
        assert torch.equal(x, y), ("run to run", k)
    perm = [4, 0, 6, 2, 5]
    part = K.sinkhorn_grad(A_[perm].contiguous(), B_[perm].contiguous(), 0.5, return_potentials=True, return_plan=True, return_info=True,
                           return_status=True, **o)
    for k, x, y in zip(keys, full, part):
        assert torch.equal(x[perm], y), ("batch of 5, permuted", k)
    one = K.sinkhorn_grad(A_[3:4].contiguous(), B_[3:4].contiguous(), 0.5, return_potentials=True, return_plan=True, return_info=True,
                          return_status=True, **o)
    for k, x, y in zip(keys, full, one):
        assert torch.equal(x[3:4], y), ("batch of 1", k)
    value, pot_f, pot_g, _ = K.sinkhorn(A_, B_, 0.5, return_potentials=True, return_status=True, **o)
    assert torch.equal(value, full[0]) and torch.equal(pot_f, full[3]) and torch.equal(pot_g, full[4])
    only0 = K.sinkhorn_grad(A_, B_, 0.5, need_g1=False, return_status=True, **o)
    assert torch.equal(only0[0], full[0]) and torch.equal(only0[1], full[1]) and only0[2] is None
    # graph replay: the same launch captured, on fresh inputs copied into the captured buffers
    sa, sb = torch.zeros_like(A_), torch.zeros_like(B_)
    sa.copy_(A_), sb.copy_(B_)
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        K.sinkhorn_grad(sa, sb, 0.5, return_status=True, **o)
    torch.cuda.current_stream().wait_stream(stream)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = K.sinkhorn_grad(sa, sb, 0.5, return_info=True, return_status=True, **o)
    sa.copy_(A_.flip(0)), sb.copy_(B_.flip(0))
    graph.replay()
    torch.cuda.synchronize()
    for k, idx in (("value", 0), ("g0", 1), ("g1", 2), ("iters", 6), ("err", 7), ("status", 8)):
        pos = {0: 0, 1: 1, 2: 2, 6: 3, 7: 4, 8: 5}[idx]
        assert torch.equal(captured[pos], full[idx].flip(0)), ("graph replay", k)


def test_autograd_is_the_one_launch_gradient():
    from lgn import sinkhorn as K
    a, b = S.batch(41, B, 9, 12, None)
    o = dict(max_iter=20, tol=1e-8, debias=True)
    x, y = _dev(a).requires_grad_(True), _dev(b).requires_grad_(True)
    w = torch.linspace(0.5, 2.0, B, device=DEV, dtype=torch.float64)
    out = K.sinkhorn_differentiable(x, y, 0.5, **o)
    (out * w).sum().backward()
    value, g0, g1, _ = K.sinkhorn_grad(_dev(a), _dev(b), 0.5, return_status=True, **o)
    assert torch.equal(out.detach(), value)
    assert torch.equal(x.grad, g0 * w.view(-1, 1, 1)) and torch.equal(y.grad, g1 * w.view(-1, 1, 1))


# ---- against the exact EMD on the device --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n,m,real,eps,o", [(6, 6, 4, 0.05, {}), (30, 30, None, 0.1, {}), (12, 17, None, 0.1, dict(beta=2.0, norm=True))],
                         ids=["6x6", "30x30", "12x17-beta2-norm"])
def test_the_converged_value_lies_above_the_exact_emd_of_the_device(n, m, real, eps, o):
    import _emd_pairs_ref as P
    from lgn import emd as M
    from lgn import sinkhorn as K
    a, b = S.batch(500 + n, B, n, m, real)
    exact = M.emd(_dev(a), _dev(b), **o)
    value, iters, err, status = K.sinkhorn(_dev(a), _dev(b), eps, max_iter=20000, tol=1e-10, return_info=True, return_status=True, **o)
    torch.cuda.synchronize()
    assert int(status.abs().max()) == 0, (status.tolist(), iters.tolist())
    for i in range(B):
        _, wa, wb = P.balanced(a[i], b[i], **o)
        Ssum = max(wa.sum(), wb.sum())
        w_min = min(wa[wa > 0].min(), wb[wb > 0].min())
        lo, hi = float(exact[i]) - 1e-9 * Ssum, float(exact[i]) + eps * Ssum * np.log(Ssum / w_min)
        print(f"pair {i}: {int(iters[i])} iterations, EMD {float(exact[i]):.6f} <= {float(value[i]):.6f} <= {hi:.6f}")
        assert lo <= float(value[i]) <= hi, (i, lo, float(value[i]), hi)


# ---- status -------------------------------------------------------------------------------------------------------------------------------

def test_the_status_bits():
    from lgn import sinkhorn as K
    a, b = S.batch(77, B, 8, 9, 6)
    A_, B_ = _dev(a), _dev(b)
    value, g0, g1, iters, err, status = K.sinkhorn_grad(A_, B_, 0.05, max_iter=3, tol=1e-12, debias=True, return_info=True, return_status=True)
    assert (status == K.ITER).all() and (iters == 3).all()
    assert torch.isfinite(value).all() and torch.isfinite(g0).all() and torch.isfinite(g1).all() and (err > 1e-12 * 10).all()
    with pytest.raises(ValueError, match="max_iter"):
        K.sinkhorn(A_, B_, 0.05, max_iter=3, tol=1e-12)
    value0, iters0, _, status0 = K.sinkhorn(A_, B_, 0.05, max_iter=3, tol=0.0, debias=True, return_info=True, return_status=True)
    assert (status0 == 0).all() and (iters0 == 3).all() and torch.equal(value0, value)
    free = K.sinkhorn(A_, B_, 4.0, max_iter=40, tol=0.0, return_info=True, return_status=True)
    assert (free[3] == 0).all() and (free[1] == 40).all()
    # a NaN event flags only its own pair
    bad = A_.clone()
    bad[2, 1, 1] = float("nan")
    v, h0, h1, it, er, st = K.sinkhorn_grad(bad, B_, 0.5, max_iter=10, tol=0.0, return_info=True, return_status=True)
    ref = K.sinkhorn_grad(A_, B_, 0.5, max_iter=10, tol=0.0, return_info=True, return_status=True)
    keep = [0, 1, 3, 4]
    assert st.tolist() == [0, 0, K.INVALID, 0, 0] and int(it[2]) == 0
    assert torch.isnan(v[2]) and torch.isnan(h0[2]).all() and torch.isnan(h1[2]).all() and torch.isnan(er[2])
    for x, y in zip((v, h0, h1, it, er), ref):
        assert torch.equal(x[keep], y[keep])
    neg = B_.clone()
    neg[0, 0, 0] = -1.0
    assert (K.sinkhorn(A_, neg, 0.5, return_status=True)[1] & 3).tolist() == [K.INVALID, 0, 0, 0, 0]
    # an all-padded event: EMPTY under norm, a problem against the fictitious particle without
    empty = A_.clone()
    empty[1] = 0.0
    v, st = K.sinkhorn(empty, B_, 0.5, norm=True, return_status=True)
    assert (st & 3).tolist() == [0, K.EMPTY, 0, 0, 0] and torch.isnan(v[1]) and torch.isfinite(v[[0, 2, 3, 4]]).all()
    v, st = K.sinkhorn(empty, B_, 0.5, debias=True, return_status=True)
    assert int((st & 3).max()) == 0 and torch.isfinite(v).all()
    both = B_.clone()
    both[1] = 0.0
    assert (K.sinkhorn(empty, both, 0.5, return_status=True)[1] & 3).tolist() == [0, K.EMPTY, 0, 0, 0]


# ---- the loss module ----------------------------------------------------------------------------------------------------------------------

CH = ((2, 2, 2), (2, 2, 2))
N_REAL = {6: 4}


def _nets(N, n=1):
    import __graft_entry__ as GE
    import _util as U
    out = []
    for _ in range(n):
        enc, dec = GE._models(N, CH[0], CH[1], torch.device(DEV), seed=23)
        U.live_weights(enc, dec)
        out.append((enc, dec))
    return out


def _batch(N, n_jets=4):
    import _normalize_ref as R
    p4 = R.jets(n_jets, N, seed=106 + N, n_real=N_REAL.get(N))
    p4 = (p4 / (p4.abs().amax(dim=(1, 2), keepdim=True) + 1e-16)).contiguous()
    return {"p4": p4.to(DEV), "labels": (p4[..., 0] != 0).to(torch.uint8).to(DEV)}


@pytest.mark.parametrize("N", [6, 30])
def test_the_loss_module_is_the_relative_call(N):
    from lgn import sinkhorn as K
    from lgn.losses import SinkhornLoss
    rec, tgt = G.jets(np.random.default_rng(60 + N), 4, N, N - N_REAL.get(N, N))
    x, t = _dev(rec).requires_grad_(True), _dev(tgt)
    for kw in (dict(), dict(epsilon=0.5, max_iter=30, tol=1e-8, debias=False, beta=2.0, norm=True)):
        loss = SinkhornLoss(num_particles=N, device=DEV, **kw)
        conf = dict(epsilon=loss.epsilon, max_iter=loss.max_iter, tol=loss.tol, debias=loss.debias, R=loss.R, beta=loss.beta,
                    norm=loss.norm, periodic_phi=loss.periodic_phi)
        eps = conf.pop("epsilon")
        out = loss(x, t)
        value, g_r, _, iters, err, status = K.sinkhorn_relative_grad(_dev(rec), t, eps, **conf)
        assert torch.equal(out.detach(), K.sinkhorn_relative_tensor(_dev(rec), t, eps, **conf).sum()) and torch.equal(out.detach(), value.sum())
        assert torch.equal(loss.status, status) and torch.equal(loss.iters, iters) and torch.equal(loss.err, err)
        (g,) = torch.autograd.grad(out, x)
        assert torch.equal(g, g_r) and torch.isfinite(g).all()


@pytest.mark.parametrize("N", [6, 30])
def test_one_adam_step_of_the_captured_module_step_is_the_eager_step(N):
    """CapturedModuleStep replays the kernels TrainStep launches, but its optimiser and L1 term run in another form: the two steps
    are held to the tolerances of the EMD tests (1e-10 loss and reconstruction, 1e-9 parameters), not to torch.equal."""
    import _util as U
    from lgn.losses import SinkhornLoss
    from lgn.step import CapturedModuleStep, NativeTrainStep, TrainStep, native_train_step
    (ea, da), (eb, db) = _nets(N, 2)
    batch = _batch(N)
    kw = dict(epsilon=0.05, max_iter=60, tol=1e-7)
    la_mod, lb_mod = SinkhornLoss(**kw), SinkhornLoss(**kw)
    a = CapturedModuleStep(ea, da, batch_size=4, lr=1e-3, l1_lambda=1e-8, use_graph=True, loss_choice=la_mod)
    b = TrainStep(eb, db, lr=1e-3, l1_lambda=1e-8, loss_choice=lb_mod)
    before = a.flat.flat.clone()
    assert torch.equal(before, b.flat.flat)
    la, ra = a.step(batch)
    lb, rb = b.step(batch)
    torch.cuda.synchronize()
    assert (la_mod.status.cpu() & ~16 == 0).all() and torch.equal(la_mod.iters, lb_mod.iters)
    assert torch.isfinite(la).all() and not torch.equal(a.flat.flat, before)
    U.assert_close(la, lb, 1e-10, "loss")
    U.assert_close(ra, rb, 1e-10, "reconstruction")
    U.assert_close(a.flat.flat, b.flat.flat, 1e-9, "parameters after one Adam step")
    with pytest.raises(NotImplementedError):
        NativeTrainStep(eb, db, batch_size=4, loss_choice=SinkhornLoss())
    with pytest.raises(NotImplementedError):
        NativeTrainStep(eb, db, batch_size=4, loss_choice=SinkhornLoss(), native_emd=True)
    assert isinstance(native_train_step(eb, db, 4, loss_choice=SinkhornLoss()), CapturedModuleStep)


def test_the_evaluation_and_reference_loop_steps_take_the_module():
    from lgn.losses import SinkhornLoss
    from lgn.step import ModuleEvalStep, ReferenceLoopStep
    ((enc, dec),) = _nets(6, 1)
    batch = _batch(6)
    mod = SinkhornLoss(epsilon=0.5, max_iter=20)
    ev = ModuleEvalStep(enc, dec, batch_size=4, loss_choice=mod)
    out = ev.run(batch)
    torch.cuda.synchronize()
    assert torch.isfinite(out["loss"]).all() and mod.status is not None and int((mod.status & 3).abs().max()) == 0
    loop = ReferenceLoopStep(enc, dec, lr=1e-3, l1_lambda=0.0, loss_choice=SinkhornLoss(epsilon=0.5, max_iter=20))
    loss, _ = loop.step(batch)
    assert torch.isfinite(loss).all()
