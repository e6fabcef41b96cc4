"""GPU tests of the native anomaly scores (lgn_anomaly_scores_f64, lgn.anomaly) and the batched assignment solver
(lgn_linear_sum_assignment_f64): against the reference's g18 fixtures, against the numpy restatement in tests/_anomaly_ref.py
(scipy's col_ind, ties included), across chunkings and input placements, on invalid input, and after NativeEvalStep."""
import numpy as np
import pytest
import torch

import _anomaly_ref as R
import _util as U

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
G18 = ("g18_anomaly_n12.npz", "g18_anomaly_n30.npz", "g18_anomaly_n150.npz")
POLAR = (1, 3, 4, 6, 8, 9, 11, 13, 14)       # device asinh / atan2 are not the host's: rtol 1e-11 there


def _inputs(z, dev=DEV):
    return [torch.from_numpy(np.ascontiguousarray(z[k])).to(dev) for k in ("recons", "target", "recons_n", "target_n")]


def _assert_scores(got, want, what="", skip=()):
    for s in range(21):
        if s not in skip:
            np.testing.assert_allclose(got[:, s], want[:, s], rtol=1e-11 if s in POLAR else 1e-12, atol=1e-300,
                                       err_msg=f"{what} {R.SCORE_KEYS[s]}")


POLAR_VARIANTS = (1, 3, 4)      # Hungarian variants on polar frames: their costs differ from the host's in the last bit


def _check_against_restatement(arrs, got, col, what=""):
    """Device scores and assignments against the restatement on the same float64 arrays.  Cartesian, normalized Cartesian and
    Lorentz costs are bit-identical to the host's, so their col_ind must be the restatement's.  The polar-frame costs go through
    device asinh / atan2, which may round differently in the last bit; with tied (zero-padded) target rows that can pick another
    optimal assignment among identical columns, and the reference's sigma pairing then scores it differently.  There the device's
    col_ind must be an optimal assignment of the host's costs and its score must be the reference's score of that col_ind."""
    want, wcol = R.anomaly_scores(*arrs)
    hung = [R.HUNGARIAN_INDEX[f] for f in POLAR_VARIANTS]
    _assert_scores(got, want, what, skip=hung)
    for f, (p, q, lor) in enumerate(R.frames(*arrs)):
        if f not in POLAR_VARIANTS:
            assert np.array_equal(col[f], wcol[f]), (what, f)
            continue
        c = R.costs(p, q, lor)
        for b in range(c.shape[0]):
            if np.array_equal(col[f, b], wcol[f, b]):
                mine = want[b, R.HUNGARIAN_INDEX[f]]
            else:
                rows = np.arange(c.shape[1])
                tot, best = c[b, rows, col[f, b]].sum(), c[b, rows, wcol[f, b]].sum()
                assert abs(tot - best) <= 1e-12 * abs(best), (what, f, b, tot, best)
                dd = p[b, col[f, b]] - q[b]
                mine = (dd * dd).sum(-1).mean()
            np.testing.assert_allclose(got[b, R.HUNGARIAN_INDEX[f]], mine, rtol=1e-11, err_msg=f"{what} variant {f} jet {b}")


@pytest.mark.parametrize("name", G18)
def test_scores_match_the_reference_fixture(name):
    from lgn import anomaly as A
    z = U.load(name)
    xs = _inputs(z)
    B, N = xs[0].shape[:2]
    col = torch.full((6, B, N), -7, device=DEV, dtype=torch.int32)
    sc, st = A.score_tensor(*xs, return_status=True, col4row=col)
    assert (st.cpu() == 0).all()
    col = col.cpu().numpy()
    for f in range(6):
        if f not in POLAR_VARIANTS:
            assert np.array_equal(col[f], z["col4row"][f]), f
    same = [(f, b) for f in POLAR_VARIANTS for b in range(B) if np.array_equal(col[f, b], z["col4row"][f, b])]
    assert len(same) >= 0.9 * len(POLAR_VARIANTS) * B
    got = sc.cpu().numpy()
    _assert_scores(got, z["scores"], name, skip=[R.HUNGARIAN_INDEX[f] for f in POLAR_VARIANTS])
    for f, b in same:
        s = R.HUNGARIAN_INDEX[f]
        np.testing.assert_allclose(got[b, s], z["scores"][b, s], rtol=1e-11, err_msg=f"{name} {R.SCORE_KEYS[s]} jet {b}")
    _check_against_restatement([z[k] for k in ("recons", "target", "recons_n", "target_n")], got, col, name)
    out = A.anomaly_scores(*xs)
    assert tuple(out) == A.SCORE_KEYS == tuple(str(k) for k in z["keys"])
    assert all(v.shape == (B,) and v.dtype == np.float64 for v in out.values())
    assert np.array_equal(np.stack(list(out.values()), -1), sc.cpu().numpy())


def _cases(n, seed):
    rng = np.random.default_rng(seed)
    yield "normal", rng.normal(size=(5, n, n))
    yield "negative", -rng.random(size=(5, n, n)) * 10
    yield "int012", rng.integers(0, 3, size=(5, n, n)).astype(np.float64)
    yield "constant", np.full((3, n, n), 1.5)
    c = rng.integers(0, 2, size=(4, n, n)).astype(np.float64)
    c[:, :, rng.integers(0, n, size=max(1, n // 4))] = 0.0           # zero columns
    c[:, rng.integers(0, n, size=max(1, n // 4))] = c[:, :1]          # duplicated rows
    yield "zerocols_duprows", c


@pytest.mark.parametrize("n", [1, 2, 7, 30, 63, 64, 65, 150, 192])
def test_linear_sum_assignment_is_the_restatement(n):
    from lgn import anomaly as A
    for kind, c in _cases(n, n):
        got = A.linear_sum_assignment(torch.from_numpy(c).to(DEV)).cpu().numpy()
        want = np.stack([R.lsap(m) for m in c])
        assert got.dtype == np.int64 and np.array_equal(got, want), (n, kind)
    one = A.linear_sum_assignment(torch.from_numpy(c[0]).to(DEV))
    assert one.shape == (n,) and np.array_equal(one.cpu().numpy(), R.lsap(c[0]))


def _degenerate(N=30, seed=3):
    rng = np.random.default_rng(seed)
    t = rng.normal(size=(6, N, 4))
    t[:, :, 0] = np.abs(t[:, :, 0]) + 2
    for b, n in enumerate((8, 12, 20, 29, N, 1)):
        t[b, n:] = 0.0
    r = t.copy()                                   # recons == target, padding included: massive ties
    r[3] = 0.0                                     # an all-zero reconstruction
    r[4, ::3] = t[4, 0]                            # duplicated rows
    t = np.concatenate([t, np.zeros((1, N, 4))])  # an all-zero jet on both sides
    r = np.concatenate([r, np.zeros((1, N, 4))])
    norm = lambda x: x / (np.abs(x).max(-2, keepdims=True) + 1e-16)
    return r, t, norm(r), norm(t)


def test_degenerate_jets_match_the_restatement():
    from lgn import anomaly as A
    arrs = _degenerate()
    xs = [torch.from_numpy(a).to(DEV) for a in arrs]
    col = torch.empty((6,) + xs[0].shape[:2], device=DEV, dtype=torch.int32)
    sc, st = A.score_tensor(*xs, return_status=True, col4row=col)
    assert (st.cpu() == 0).all()
    _check_against_restatement(arrs, sc.cpu().numpy(), col.cpu().numpy(), "degenerate")


def _restated(xs, what):
    from lgn import anomaly as A
    dev = [x.to(DEV) for x in xs]
    col = torch.empty((6,) + tuple(dev[0].shape[:2]), device=DEV, dtype=torch.int32)
    sc = A.score_tensor(*dev, col4row=col).cpu().numpy()
    _check_against_restatement([x.detach().cpu().numpy() for x in xs], sc, col.cpu().numpy(), what)
    return sc


def _random(B, N, seed, real=20):
    g = torch.Generator().manual_seed(seed)
    t = torch.randn(B, N, 4, generator=g, dtype=torch.float64)
    t[..., 0] = t[..., 1:].norm(dim=-1) + 0.1
    t[:, real:] = 0.0
    r = t + 0.2 * torch.randn(B, N, 4, generator=g, dtype=torch.float64)
    norm = lambda x: x / (x.abs().amax(-2, keepdim=True) + 1e-16)
    return [r, t, norm(r), norm(t)]


def test_chunking_and_placement_do_not_change_the_scores():
    from lgn import anomaly as A
    xs = _random(37, 30, 11)
    dev = [x.to(DEV) for x in xs]
    ref = A.anomaly_scores(*dev, batch_size=-1)
    for kw in ({"batch_size": 4}, {"batch_size": 1}, {"batch_size": 36}, {}):
        for ins in (xs, dev):
            out = A.anomaly_scores(*ins, **kw)
            assert list(out) == list(ref)
            for k in ref:
                assert np.array_equal(out[k], ref[k]), (kw, k)
    one = A.anomaly_scores(*[x[:1] for x in xs])
    for k in ref:
        assert np.array_equal(one[k], ref[k][:1])
    again = A.anomaly_scores(*dev)
    assert all(np.array_equal(again[k], ref[k]) for k in ref)
    assert np.array_equal(_restated(xs, "random 37 x 30"), np.stack(list(ref.values()), -1))
    no_h = A.score_tensor(*dev, hungarian=False).cpu().numpy()
    full = np.stack(list(ref.values()), -1)
    assert np.isnan(no_h[:, list(R.HUNGARIAN_INDEX)]).all()
    keep = [s for s in range(21) if s not in R.HUNGARIAN_INDEX]
    assert np.array_equal(no_h[:, keep], full[:, keep])


def test_a_chunk_boundary_past_65536_jets():
    from lgn import anomaly as A
    xs = _random(65537, 8, 12, real=6)
    dev = [x.to(DEV) for x in xs]
    whole = A.score_tensor(*dev).cpu().numpy()
    out = A.anomaly_scores(*xs)                  # CPU inputs: two chunks of the default 65,536
    assert np.array_equal(np.stack(list(out.values()), -1), whole)
    tail = A.score_tensor(*[x[-3:] for x in dev]).cpu().numpy()
    assert np.array_equal(tail, whole[-3:])


def test_nan_input_raises_and_the_next_call_succeeds():
    from lgn import anomaly as A
    xs = [x.to(DEV) for x in _random(5, 12, 13, real=10)]
    bad = [x.clone() for x in xs]
    bad[0][2, 3, 1] = float("nan")
    with pytest.raises(ValueError, match="invalid numeric entries"):
        A.anomaly_scores(*bad)
    sc, st = A.score_tensor(*bad, return_status=True)
    st = st.cpu().numpy()
    assert st[2] != 0 and (np.delete(st, 2) == 0).all()
    h = sc[2, list(R.HUNGARIAN_INDEX)].cpu().numpy()
    assert np.isnan(h[[0, 1, 4, 5]]).all() and np.isfinite(h[[2, 3]]).all()    # the NaN is in recons, not in recons_n
    assert st[2] == (1 << 0) | (1 << 1) | (1 << 4) | (1 << 5)
    c = torch.randn(3, 6, 6, device=DEV, dtype=torch.float64)
    c[1, 2, 2] = float("-inf")
    with pytest.raises(ValueError, match="invalid numeric entries"):
        A.linear_sum_assignment(c)
    out = A.anomaly_scores(*xs)
    assert np.array_equal(_restated(xs, "after NaN"), np.stack(list(out.values()), -1))


def test_include_emd_is_refused():
    from lgn import anomaly as A
    xs = [x.to(DEV) for x in _random(2, 6, 14, real=6)]
    with pytest.raises(NotImplementedError, match="energyflow"):
        A.anomaly_scores(*xs, include_emd=True)


def test_scores_after_the_native_eval_step():
    """The test.py path: NativeEvalStep's get_real(recon) and its target through anomaly_scores, against the restatement."""
    import __graft_entry__ as G
    from lgn import anomaly as A
    from lgn.step import NativeEvalStep
    z = U.load("g17_real_maxdim2.npz")
    m = U.meta(z)
    enc, dec = G._models(m["N"], m["ch_enc"], m["ch_dec"], torch.device(DEV), seed=m["seed"], maxdim=2)
    batch = {"p4": torch.from_numpy(z["p4"]).to(DEV), "labels": torch.from_numpy(z["labels"]).to(DEV)}
    out = NativeEvalStep(enc, dec, m["B"], get_real_method="real").run(batch)
    recon, target = out["recon"], batch["p4"]
    norm = lambda x: x / (x.abs().amax(-2, keepdim=True) + 1e-16)
    xs = [recon, target, norm(recon), norm(target)]
    got = A.anomaly_scores(*xs)
    assert np.array_equal(_restated(xs, "eval step"), np.stack(list(got.values()), -1))
