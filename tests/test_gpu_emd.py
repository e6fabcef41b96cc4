"""GPU tests of the native EMD score (csrc/emd.hip, csrc/emd_wave.hpp; lgn.emd, lgn.anomaly include_emd="native"): against the g24
fixture (values of the LP restatement tests/_emd_ref.py), against an optimality certificate that needs no solver (primal and dual
feasibility and equal objectives), against the exact assignment optimum on equal weights, at the edges of the wave layout and of the
two flow placements (LDS / workspace), on degenerate input, and through the Python interface up to the ROC curves."""
import numpy as np
import pytest
import torch

import _emd_ref as E
import _util as U

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def events(rng, B, n, spread=0.4):
    """[B][n][3] events of (pT, y, phi) with random positive weights"""
    return np.stack([rng.random((B, n)) + 0.05, rng.normal(size=(B, n)) * spread, rng.normal(size=(B, n)) * spread], axis=-1)


def certify(ev0, ev1, R=1.0):
    """Runs lgn.emd.emd with the flow and the potentials returned and checks, pair by pair and without any other solver, that the flow
    is feasible, the potentials are feasible and the two objectives agree: together that IS optimality (LP duality).  Bounds: 1e-12 of
    the total weight for the marginals, 1e-12 absolute for the dual constraints (costs are O(1)), 1e-12 relative for the objectives.
    Returns the (B,) distances."""
    from lgn import emd as M
    val, flow, d0, d1, st = M.emd(dev(ev0), dev(ev1), R=R, return_flow=True, return_duals=True, return_status=True)
    val, flow, d0, d1, st = (x.cpu().numpy() for x in (val, flow, d0, d1, st))
    assert (st == 0).all(), st
    for b in range(len(ev0)):
        c, a, w = E.balanced(ev0[b], ev1[b], R)
        total = max(a.sum(), w.sum())
        f = flow[b]
        assert f.shape == c.shape and (f >= 0).all()
        assert np.abs(f.sum(1) - a).max() <= 1e-12 * total and np.abs(f.sum(0) - w).max() <= 1e-12 * total, b
        assert (d0[b][:, None] + d1[b][None, :] <= c + 1e-12).all(), (b, (d0[b][:, None] + d1[b][None, :] - c).max())
        primal, dual = (f * c).sum(), (d0[b] * a).sum() + (d1[b] * w).sum()
        assert abs(primal - dual) <= 1e-12 * abs(primal), (b, primal, dual)
        assert abs(val[b] - primal) <= 1e-12 * abs(primal), (b, val[b], primal)
    return val


# ---- 1. values ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("tag", ["5x8", "1x7", "64x65"])
def test_generic_events_match_the_fixture(tag):
    from lgn import emd as M
    z = U.load("g24_emd.npz")
    got, st = M.emd(dev(z[f"gen_{tag}_ev0"]), dev(z[f"gen_{tag}_ev1"]), return_status=True)
    assert (st.cpu() == 0).all()
    np.testing.assert_allclose(got.cpu().numpy(), z[f"gen_{tag}_emd"], rtol=1e-12, atol=1e-300)


@pytest.mark.parametrize("tag", ["n12", "n30", "n150"])
def test_the_relative_score_matches_the_fixture(tag):
    from lgn import emd as M
    z = U.load("g24_emd.npz")
    got, st = M.emd_relative_tensor(dev(z[f"rel_{tag}_recons"]), dev(z[f"rel_{tag}_target"]), return_status=True)
    assert (st.cpu() == 0).all()
    np.testing.assert_allclose(got.cpu().numpy(), z[f"rel_{tag}_emd"], rtol=1e-11, atol=1e-300)


# ---- 2. optimality certificate --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n,m", [(12, 12), (30, 30), (5, 8)])
def test_the_flow_and_the_potentials_certify_the_optimum(n, m):
    rng = np.random.default_rng(100 * n + m)
    certify(events(rng, 6, n), events(rng, 6, m))
    certify(events(rng, 3, n), events(rng, 3, m), R=0.4)            # theta / R against the constant cost 1 of the fictitious particle


# ---- 3. exact cross-check ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [30, 70])
def test_equal_weights_give_the_assignment_optimum(n):
    from scipy.optimize import linear_sum_assignment
    from lgn import emd as M
    rng = np.random.default_rng(n)
    a, b = events(rng, 4, n, spread=1.0), events(rng, 4, n, spread=1.0)
    a[..., 0] = b[..., 0] = 1.0 / n
    got = M.emd(dev(a), dev(b)).cpu().numpy()
    for k in range(4):
        c = E.thetas(a[k], b[k])
        r, col = linear_sum_assignment(c)
        want = c[r, col].sum()
        assert abs(n * got[k] - want) <= 1e-12 * want, (k, n * got[k], want)


# ---- 4. edges of the wave layout ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [1, 63, 64, 65, 191])
def test_sizes_at_the_edges_of_the_wave_layout(n):
    from lgn import _native as N
    from lgn import emd as M
    assert N.EMD_NMAX == 191
    rng = np.random.default_rng(n)
    a, b = events(rng, 2, n), events(rng, 2, n)
    val = certify(a, b)
    swapped = M.emd(dev(b), dev(a)).cpu().numpy()
    np.testing.assert_allclose(swapped, val, rtol=1e-12)
    pa, pb = rng.permutation(n), rng.permutation(n)
    permuted = M.emd(dev(a[:, pa]), dev(b[:, pb])).cpu().numpy()
    np.testing.assert_allclose(permuted, val, rtol=1e-12)
    assert M.flow_in_lds(n) == (n <= 65)                            # 191: the workspace path


def test_the_largest_jet_takes_the_workspace_path():
    """N = 150 with 100 real particles, 4 jets: the flow does not fit LDS.  The relative score equals the generic solver's on the frames
    staged on the host (rtol 1e-11: device asinh / atan2), and that one is certified."""
    from lgn import _native as N
    from lgn import emd as M
    assert not M.flow_in_lds(150) and M.flow_in_lds(30)
    assert N.lib().lgn_emd_lds_bytes(150) < 8 * 151 * 151 and N.lib().lgn_emd_workspace_bytes(4, 150) == 4 * 151 * 151 * 8
    rng = np.random.default_rng(150)
    t = rng.normal(size=(4, 150, 4))
    t[..., 0] = np.sqrt((t[..., 1:] ** 2).sum(-1)) + 0.1
    t[:, 100:] = 0.0
    r = t + 0.2 * rng.normal(size=t.shape)
    r[:, 120:] = 0.0
    got, st = M.emd_relative_tensor(dev(r), dev(t), return_status=True)
    assert (st.cpu() == 0).all()
    want = certify(E.relative_events(r), E.relative_events(t))
    np.testing.assert_allclose(got.cpu().numpy(), want, rtol=1e-11)


# ---- 5. degenerate input ---------------------------------------------------------------------------------------------------------------

def test_weightless_invalid_and_tied_events():
    from lgn import _native as N
    from lgn import emd as M
    rng = np.random.default_rng(5)
    a, b = events(rng, 6, 9), events(rng, 6, 11)
    a[0, :, 0] = 0.0                                   # all-zero-padded against real: the other event's sum pT
    b[1, :, 0] = 0.0
    a[2, :, 0] = 0.0                                   # both sides empty
    b[2, :, 0] = 0.0
    a[3, 4, 1] = np.nan                                # a NaN coordinate: that pair only
    b[4, 2, 0] = -0.5                                  # a negative weight
    val, st = M.emd(dev(a), dev(b), return_status=True)
    val, st = val.cpu().numpy(), st.cpu().numpy()
    assert st.tolist() == [0, 0, N.EMD_EMPTY, N.EMD_INVALID, N.EMD_INVALID, 0]
    assert np.isnan(val[2:5]).all()
    np.testing.assert_allclose(val[0], b[0, :, 0].sum(), rtol=1e-12)
    np.testing.assert_allclose(val[1], a[1, :, 0].sum(), rtol=1e-12)
    np.testing.assert_allclose(val[5], certify(a[5:], b[5:])[0], rtol=1e-12)
    with pytest.raises(ValueError, match="weightless"):
        M.emd(dev(a[2]), dev(b[2]))
    with pytest.raises(ValueError, match="NaN, infinity or a negative weight"):
        M.emd(dev(a[3:5]), dev(b[3:5]))
    for bad in (np.inf, -np.inf):
        c = a[5:].copy()
        c[0, 1, 2] = bad
        assert M.emd(dev(c), dev(b[5:]), return_status=True)[1].item() == N.EMD_INVALID

    # exact ties: many equal weights and duplicate positions (a degenerate LP), some particles weightless
    t0, t1 = events(rng, 3, 20), events(rng, 3, 20)
    t0[..., 0] = t1[..., 0] = 0.25
    t0[:, ::2, 1:] = t0[:, :1, 1:]
    t1[:, ::3, 1:] = t0[:, :1, 1:]
    t0[:, 5:9, 0] = 0.0
    t1[2] = t0[2]                                       # identical events: 0
    val = certify(t0, t1)
    want = np.array([E.emd(t0[k], t1[k]) for k in range(3)])
    np.testing.assert_allclose(val, want, rtol=1e-12, atol=1e-300)
    assert val[2] == 0.0


def test_arguments_are_refused_before_any_launch():
    from lgn import _native as N
    from lgn import emd as M
    lib = N.lib()
    a, b = torch.rand(2, 150, 3, device=DEV, dtype=torch.float64), torch.rand(2, 20, 3, device=DEV, dtype=torch.float64)
    out, st = torch.full((2,), -7.0, device=DEV, dtype=torch.float64), torch.full((2,), -7, device=DEV, dtype=torch.int32)
    need = lib.lgn_emd_workspace_bytes(2, 150)
    work = torch.empty(need, device=DEV, dtype=torch.uint8)
    args = (N.ptr(a), N.ptr(b), 2, 150, 20, 1.0, N.ptr(out), None, None, None, N.ptr(st))
    assert lib.lgn_emd_f64(*args, N.ptr(work), need - 8, N.stream_ptr()) < 0 and "too short" in N.last_error()
    assert lib.lgn_emd_f64(*args, None, 0, N.stream_ptr()) < 0
    assert lib.lgn_emd_f64(N.ptr(a), N.ptr(b), 2, N.EMD_NMAX + 1, 20, 1.0, N.ptr(out), None, None, None, N.ptr(st), N.ptr(work), need,
                           N.stream_ptr()) < 0
    torch.cuda.synchronize()
    assert (out.cpu() == -7.0).all() and (st.cpu() == -7).all()          # nothing ran
    assert lib.lgn_emd_f64(*args, N.ptr(work), need, N.stream_ptr()) == 0
    assert (st.cpu() == 0).all() and torch.isfinite(out).all()
    with pytest.raises(ValueError, match="191"):
        M.emd(torch.rand(1, 192, 3, device=DEV, dtype=torch.float64), b[:1])
    with pytest.raises(ValueError, match="191"):
        M.emd_relative_tensor(torch.rand(1, 192, 4, device=DEV, dtype=torch.float64), torch.rand(1, 192, 4, device=DEV, dtype=torch.float64))


# ---- 6. interface ------------------------------------------------------------------------------------------------------------------------

def _jets(B, N, seed, real=20):
    g = torch.Generator().manual_seed(seed)
    t = torch.randn(B, N, 4, generator=g, dtype=torch.float64)
    t[..., 0] = t[..., 1:].norm(dim=-1) + 0.1
    t[:, real:] = 0.0
    r = t + 0.2 * torch.randn(B, N, 4, generator=g, dtype=torch.float64)
    norm = lambda x: x / (x.abs().amax(-2, keepdim=True) + 1e-16)
    return [r, t, norm(r), norm(t)]


def test_anomaly_scores_with_the_native_emd():
    from lgn import anomaly as A
    from lgn import emd as M
    xs = _jets(23, 30, 6)
    on_dev = [x.to(DEV) for x in xs]
    base = A.anomaly_scores(*on_dev, include_emd=False)
    ref = A.anomaly_scores(*on_dev, include_emd="native")
    assert tuple(ref) == A.SCORE_KEYS_EMD == A.SCORE_KEYS + (E.KEY,) and len(ref) == 22
    for k in A.SCORE_KEYS:
        assert np.array_equal(ref[k], base[k]), k                   # the first 21: bit-identical
    direct = M.emd_relative_tensor(on_dev[0], on_dev[1]).cpu().numpy()
    assert ref[E.KEY].shape == (23,) and ref[E.KEY].dtype == np.float64 and np.array_equal(ref[E.KEY], direct)
    np.testing.assert_allclose(direct[:4], E.emd_relative(xs[0][:4].numpy(), xs[1][:4].numpy()), rtol=1e-11)
    for chunk in (1, 7, 23):
        for ins in (xs, on_dev):
            out = A.anomaly_scores(*ins, include_emd="native", batch_size=chunk)
            assert list(out) == list(ref)
            for k in ref:
                assert np.array_equal(out[k], ref[k]), (chunk, k)
    with pytest.raises(NotImplementedError, match="energyflow"):
        A.anomaly_scores(*on_dev, include_emd=True)
    sc, st = A.score_tensor(*on_dev, emd=True, return_status=True)
    assert sc.shape == (23, 22) and (st.cpu() == 0).all()
    assert np.array_equal(sc.cpu().numpy(), np.stack(list(ref.values()), -1))
    scores, labels, sig, bkg = A.anomaly_scores_sig_bkg(*[x[:10] for x in on_dev], *[x[10:] for x in on_dev], include_emd="native")
    assert list(scores) == list(ref) and np.array_equal(scores[E.KEY], ref[E.KEY]) and labels.tolist() == [1.0] * 10 + [-1.0] * 13
    curves, aucs = A.get_ROC_AUC(scores, labels, plot_rocs=False)
    assert list(aucs) == list(ref) and 0.5 <= aucs[E.KEY] <= 1.0 and len(curves[E.KEY]) == 3
    empty = [torch.zeros_like(x) for x in on_dev]
    with pytest.raises(ValueError, match="EMD score: both events are weightless"):
        A.anomaly_scores(*[torch.cat([x, e[:1]]) for x, e in zip(on_dev, empty)], include_emd="native")


def test_eval_step_then_22_scores_then_roc_without_a_sync():
    """NativeEvalStep.run(), then score_tensor(emd=True) and roc_auc_tensor captured into one graph (a capture admits no host sync),
    replayed and compared with the eager calls."""
    import __graft_entry__ as G
    from lgn import anomaly as A
    from lgn.step import NativeEvalStep
    z = U.load("g17_real_maxdim2.npz")
    m = U.meta(z)
    enc, dec = G._models(m["N"], m["ch_enc"], m["ch_dec"], torch.device(DEV), seed=m["seed"], maxdim=2)
    batch = {"p4": torch.from_numpy(z["p4"]).to(DEV), "labels": torch.from_numpy(z["labels"]).to(DEV)}
    out = NativeEvalStep(enc, dec, m["B"], get_real_method="real").run(batch)
    recon, target = out["recon"].clone(), batch["p4"].clone()
    norm = lambda x: x / (x.abs().amax(-2, keepdim=True) + 1e-16)
    static = [recon, target, norm(recon), norm(target)]
    labels = torch.from_numpy(np.where(np.arange(m["B"]) % 2 == 0, 1.0, -1.0)).to(DEV)
    eager_scores = A.score_tensor(*static, emd=True)
    eager = A.roc_auc_tensor(eager_scores, labels)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        A.roc_auc_tensor(A.score_tensor(*static, emd=True), labels)      # warm-up outside the capture
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            scores = A.score_tensor(*static, emd=True)
            roc = A.roc_auc_tensor(scores, labels)
    torch.cuda.current_stream().wait_stream(side)
    graph.replay()
    torch.cuda.synchronize()
    assert scores.shape == (m["B"], 22) and torch.equal(scores, eager_scores)
    want = E.emd_relative(recon.cpu().numpy(), target.cpu().numpy())
    np.testing.assert_allclose(scores[:, 21].cpu().numpy(), want, rtol=1e-11)
    assert roc["auc"].shape == (22,) and (roc["status"].cpu() == 0).all()
    for k in ("length", "flipped", "status", "auc"):
        assert torch.equal(roc[k], eager[k]), k
