"""GPU tests of the native reconstruction analysis (lgn_recon_analysis_f64, lgn_match_rel_err_f64, lgn_histogram_f64, lgn.analysis):
against the reference's g22 fixtures, against the numpy / scipy restatement in tests/_analysis_ref.py at the shapes where the kernel
takes another path, on invalid input, under graph capture, as the reference's drop-in and behind NativeEvalStep."""
import numpy as np
import pytest
import torch

import _analysis_ref as R
import _util as U

pytestmark = pytest.mark.gpu
assert_same, assert_mass = R.assert_same, R.assert_mass
DEV = "cuda:0"
G22 = ("g22_analysis_n12.npz", "g22_analysis_n30.npz", "g22_analysis_n150.npz")
ARITH, TRANS = 1e-12, 1e-11        # only arithmetic / device asinh, atan2 enter (the tolerances of tests/test_gpu_anomaly.py)


def _run(target, recons, **kw):
    from lgn import analysis as A
    out = A.recon_analysis(torch.from_numpy(np.ascontiguousarray(target)).to(DEV), torch.from_numpy(np.ascontiguousarray(recons)).to(DEV), **kw)
    return {k: v.cpu().numpy() for k, v in out.items()}


def _check(got, want, target, recons, padded, what, floors=None):
    """Device arrays against host ones (fixture or restatement).  `padded`: jets whose relative-polar costs tie exactly (zero rows):
    device asinh / atan2 may differ from the host's in the last bit and pick another optimal assignment among them.
    floors: {quantity: (B,) absolute term per jet} of a case whose restatement misses the relative tolerance against itself on named
    jets (measured on the CPU; "rel_err.1", "rel_err.2", "part_polar", "part_polarrel"); None: the relative tolerances alone."""
    B = target.shape[0]
    fl = (lambda q, shape, idx=slice(None): None) if floors is None else \
        (lambda q, shape, idx=slice(None): np.reshape(floors[q][idx], shape))                           # noqa: E731
    assert (got["status"] == 0).all(), what
    assert np.array_equal(got["col4row"][0], want["col4row"][0]), f"{what}: Cartesian assignment"
    firm = np.setdiff1d(np.arange(B), padded)
    assert np.array_equal(got["col4row"][1, firm], want["col4row"][1, firm]), f"{what}: relative-polar assignment"
    loose = [b for b in padded if not np.array_equal(got["col4row"][1, b], want["col4row"][1, b])]
    for b in loose:
        R.assert_tied_assignment(want["part_polarrel"][0, b], want["part_polarrel"][1, b], got["col4row"][1, b], want["col4row"][1, b],
                                 got["rel_err"][2, b], f"{what} jet {b}", floor=None if floors is None else floors["rel_err.2"][b])
    same = np.setdiff1d(np.arange(B), loose)
    assert_same(got["rel_err"][0], want["rel_err"][0], ARITH, f"{what} rel_err Cartesian")
    assert_same(got["rel_err"][1], want["rel_err"][1], TRANS, f"{what} rel_err polar", fl("rel_err.1", (-1, 1, 1)))
    assert_same(got["rel_err"][2, same], want["rel_err"][2, same], TRANS, f"{what} rel_err polarrel", fl("rel_err.2", (-1, 1, 1), same))
    for k in ("part_polar", "part_polarrel"):
        assert_same(got[k], want[k], TRANS, f"{what} {k}", fl(k, (1, -1, 1, 1)))
    assert_same(got["jet_cart"][..., 1:], want["jet_cart"][..., 1:], ARITH, f"{what} jet_cart")
    assert_same(got["jet_polar"][..., 1:], want["jet_polar"][..., 1:], TRANS, f"{what} jet_polar")
    assert_same(got["jet_rel_err"][..., 1:], want["jet_rel_err"][..., 1:], TRANS, f"{what} jet_rel_err")
    # its mass component: the definition (recons - target) / (recons + 1e-16) on the device's own masses, where it is exact (the masses
    # themselves are compared through m^2 below)
    for k, f in (("jet_cart", 0), ("jet_polar", 1)):
        with np.errstate(all="ignore"):
            mine = (got[k][1][:, 0] - got[k][0][:, 0]) / (got[k][1][:, 0] + 1e-16)
        assert np.array_equal(got["jet_rel_err"][f][:, 0], mine, equal_nan=True), f"{what} jet_rel_err mass"
    for side, p in enumerate((target, recons)):
        assert_mass(got["jet_cart"][side, :, 0], p, f"{what} mass")
        assert np.array_equal(got["jet_polar"][side, :, 0], got["jet_cart"][side, :, 0])
    assert np.array_equal(got["is_padded"], want["is_padded"]) and np.array_equal(got["jet_keep"], want["jet_keep"]), what


@pytest.mark.parametrize("name", G22)
def test_analysis_matches_the_reference_fixture(name):
    z = U.load(name)
    got = _run(z["target"], z["recons"])
    _check(got, z, z["target"], z["recons"], U.meta(z)["padded_kept"], name)


def _jets(B, N, seed, pad=()):
    rng = np.random.default_rng(seed)
    p3 = rng.normal(size=(B, N, 3)) * np.array([1.0, 1.0, 2.0])
    t = np.concatenate([(np.sqrt((p3 ** 2).sum(-1)) + 0.1)[..., None], p3], -1)
    r = t + rng.normal(scale=0.3, size=t.shape)
    for b, n in pad:
        t[b, n:] = 0.0
        r[b, n:] = rng.normal(scale=1e-3, size=(N - n, 4))
    return t, r


@pytest.mark.parametrize("B,N", [(3, 1), (5, 63), (5, 64), (5, 65), (3, 129), (3, 192), (1, 30), (257, 9)])
def test_analysis_matches_the_restatement(B, N):
    pad = [(0, max(1, N // 2))] if N > 1 else []
    if B > 2:
        pad.append((2, 0))                   # an all-zero target jet: status 0, every row padded
    t, r = _jets(B, N, 100 * N + B, pad)
    got = _run(t, r)
    _check(got, R.recon_analysis(t, r), t, r, [b for b, _ in pad], f"B {B} N {N}")
    if B > 2:
        assert got["is_padded"][2].all() and got["status"][2] == 0 and not got["jet_keep"][:, 2].any()


def test_invalid_jets_get_a_status_and_leave_the_others_alone():
    t, r = _jets(6, 20, 7, [(4, 12)])
    bad_t, bad_r = t.copy(), r.copy()
    bad_r[1, 3, 2] = np.nan                  # a NaN cost: status 1
    bad_t[3, 5, 1] = np.inf                  # a row of infinite Cartesian costs: infeasible, 256; its relative-polar frame holds NaN: | 1
    got, want, clean = _run(bad_t, bad_r), R.recon_analysis(bad_t, bad_r), _run(t, r)
    assert np.array_equal(got["status"], want["status"]) and list(got["status"]) == [0, 1, 0, 257, 0, 0]
    for b in (1, 3):
        assert (got["col4row"][:, b] == -1).all() and np.isnan(got["rel_err"][:, b]).all() and not got["is_padded"][b].any()
    ok = [0, 2, 4, 5]
    for k in ("rel_err", "col4row", "part_polar", "part_polarrel", "jet_cart", "jet_polar", "jet_rel_err", "jet_keep"):
        assert np.array_equal(got[k][:, ok], clean[k][:, ok], equal_nan=True), k
    assert np.array_equal(got["is_padded"][ok], clean["is_padded"][ok])


def test_identity_pairing_and_relative_coordinates():
    t, r = _jets(9, 30, 8, [(1, 17)])
    for kw in (dict(find_match=False), dict(abs_coord=False), dict(find_match=False, abs_coord=False)):
        got, want = _run(t, r, **kw), R.recon_analysis(t, r, **kw)
        if kw.get("find_match", True):
            # the polar frame stands in for the relative-polar one: the padded jet's rows tie there too, so its second assignment
            # goes by the rule of _check
            _check(got, want, t, r, [1], f"{kw}")
        else:
            assert np.array_equal(got["col4row"], want["col4row"]), kw
            assert_same(got["rel_err"][0], want["rel_err"][0], ARITH, f"{kw} Cartesian")
            assert_same(got["rel_err"][1:], want["rel_err"][1:], TRANS, f"{kw} polar")
            assert np.array_equal(got["is_padded"], want["is_padded"]) and (got["status"] == 0).all()
        if not kw.get("abs_coord", True):
            assert np.array_equal(got["part_polarrel"], got["part_polar"])
            assert_same(got["part_polar"], want["part_polar"], TRANS, f"{kw} part_polar")


def test_optional_outputs_may_be_null():
    from lgn import analysis as A
    t, r = (torch.from_numpy(x).to(DEV) for x in _jets(7, 30, 9, [(2, 11)]))
    full = A.recon_analysis(t, r)
    jets = A.recon_analysis(t, r, residuals=False, particles=False)
    assert set(jets) == {"target", "recons", "jet_cart", "jet_polar", "jet_rel_err", "jet_keep"}
    res = A.recon_analysis(t, r, particles=False)
    assert "part_polar" not in res and "part_polarrel" not in res
    for out in (jets, res):
        for k, v in out.items():
            assert torch.equal(v, full[k]) or (v.is_floating_point() and np.array_equal(v.cpu().numpy(), full[k].cpu().numpy(), equal_nan=True)), k
    host = A.recon_analysis(t.cpu(), r.cpu(), batch_size=3)         # CPU inputs, three chunks
    for k, v in full.items():
        assert np.array_equal(v.cpu().numpy(), host[k].cpu().numpy(), equal_nan=True), k
    f32, f64 = A.recon_analysis(t.float(), r.float()), A.recon_analysis(t.float().double(), r.float().double())
    assert all(np.array_equal(f32[k].cpu().numpy(), f64[k].cpu().numpy(), equal_nan=True) for k in f64) and f32["rel_err"].dtype == torch.float64
    empty = A.recon_analysis(t[:0], r[:0])
    assert empty["rel_err"].shape == (3, 0, 30, 3) and empty["status"].shape == (0,)


def _hist_case(rows, seed):
    rng = np.random.default_rng(seed)
    edges = [np.array([-0.5, 0.25]), np.linspace(-2.0, 3.0, 82), np.linspace(-1.0, 1.0, 1025)]
    x = rng.normal(size=(rows, 3))
    for c, e in enumerate(edges):            # edge values, their neighbours, NaN and infinities, where the rows allow
        special = np.concatenate([e, np.nextafter(e, np.inf), np.nextafter(e, -np.inf), [np.nan, np.inf, -np.inf]])
        n = min(rows, len(special))
        x[rng.permutation(rows)[:n], c] = special[rng.permutation(len(special))[:n]]
    return x, edges, rng.random(rows) < 0.6, rng.normal(size=rows)


@pytest.mark.parametrize("rows", [1, 63, 64, 65, 100003])
def test_histogram_is_numpys(rows):
    from lgn import analysis as A
    x, edges, keep, w = _hist_case(rows, rows)
    xd, kd, wd = torch.from_numpy(x).to(DEV), torch.from_numpy(keep).to(DEV), torch.from_numpy(w).to(DEV)
    for k, kdev in ((None, None), (keep, kd)):
        got = A.histogram(xd, edges, keep=kdev)
        assert got.dtype == torch.int64 and got.shape == (3, 1024)
        assert torch.equal(got, A.histogram(xd, edges, keep=kdev))
        got, gw = got.cpu().numpy(), A.histogram(xd, edges, keep=kdev, weights=wd).cpu().numpy()
        for c, e in enumerate(edges):
            v, ww = (x[:, c], w) if k is None else (x[k, c], w[k])
            want = np.histogram(v, bins=e)[0]
            assert np.array_equal(got[c, :len(e) - 1], want) and not got[c, len(e) - 1:].any(), (rows, c)
            wantw = np.histogram(v, bins=e, weights=ww)[0]
            # np.histogram takes a weighted bin as a difference of the cumulative sum over ALL sorted values, so its own error in
            # every bin is that of an n-term sum of all the weights: n 2^-52 sum|w| with n = len(v)
            assert (np.abs(gw[c, :len(e) - 1] - wantw) <= len(v) * 2.0 ** -52 * np.abs(ww).sum()).all(), (rows, c)
            assert not gw[c, len(e) - 1:].any(), (rows, c)
            # against each bin summed on its own (np.bincount), the kernel's error is that of the bin's own n_i-term sum
            bins = R.bin_index(v, e)
            direct = np.bincount(bins[bins >= 0], weights=ww[bins >= 0], minlength=len(e) - 1)
            bound = np.array([(bins == i).sum() * 2.0 ** -52 * np.abs(ww[bins == i]).sum() for i in range(len(e) - 1)])
            assert (np.abs(gw[c, :len(e) - 1] - direct) <= bound).all(), (rows, c)
    view = torch.from_numpy(np.concatenate([np.zeros((rows, 1)), x], -1)).to(DEV)[:, 1:]     # columns 1..3 of a 4-wide matrix
    assert torch.equal(A.histogram(view, edges), A.histogram(xd, edges))
    wide = torch.from_numpy(np.repeat(x, 2, axis=1)).to(DEV)                                   # non-adjacent columns, one row included
    assert torch.equal(A.histogram(wide[:, ::2], edges), A.histogram(xd, edges))
    assert torch.equal(A.histogram(wide[:1, ::2], edges), A.histogram(xd[:1], edges))


def test_particle_histograms_are_numpys():
    from lgn import analysis as A
    t, r = _jets(40, 30, 10, [(b, 10 + b) for b in range(12)])
    out = A.recon_analysis(torch.from_numpy(t).to(DEV), torch.from_numpy(r).to(DEV))
    e3 = lambda lo, hi: [np.linspace(lo, hi, 81)] * 3
    ranges = {"p_cartesian": e3(-3, 3), "p_polar": [np.linspace(0, 4, 81), np.linspace(-3, 3, 41), np.linspace(-np.pi, np.pi, 81)],
              "rel_err_cartesian": e3(-2, 2), "rel_err_polar": e3(-2, 2), "rel_err_polarrel": e3(-2, 2),
              "padded_cartesian": e3(-4e-3, 4e-3), "padded_polar": e3(-2, 2), "padded_polarrel": e3(-2, 2)}
    got = A.particle_histograms(out, ranges)
    h = {k: v.cpu().numpy() for k, v in out.items()}
    pad = h["is_padded"].reshape(-1)
    want = {}
    for s, p in enumerate((t, r)):
        big = np.linalg.norm(p[..., 1:], axis=-1).reshape(-1) > 1e-6
        want.setdefault("p_cartesian", []).append([np.histogram(p.reshape(-1, 4)[big, 1 + c], bins=ranges["p_cartesian"][c])[0] for c in range(3)])
        want.setdefault("p_polar", []).append([np.histogram(h["part_polar"][s].reshape(-1, 3)[big, c], bins=ranges["p_polar"][c])[0] for c in range(3)])
    feats = (r[..., 1:].reshape(-1, 3), h["part_polar"][1].reshape(-1, 3), h["part_polarrel"][1].reshape(-1, 3))
    for f, frame in enumerate(A.FRAMES):
        want[f"rel_err_{frame}"] = [np.histogram(h["rel_err"][f].reshape(-1, 3)[~pad, c], bins=ranges[f"rel_err_{frame}"][c])[0] for c in range(3)]
        want[f"padded_{frame}"] = [np.histogram(feats[f][pad, c], bins=ranges[f"padded_{frame}"][c])[0] for c in range(3)]
    assert set(got) == set(want)
    for k in want:
        flat = lambda v: [a for x in v for a in (x if isinstance(x, list) else [x])]
        assert all(np.array_equal(a, b) for a, b in zip(flat(got[k]), flat(want[k]))), k
    assert sum(a.sum() for a in got["padded_cartesian"]) > 0 and sum(a.sum() for a in got["rel_err_cartesian"]) > 0


def test_analysis_and_histogram_replay_from_a_graph():
    from lgn import analysis as A
    ins = [tuple(torch.from_numpy(x).to(DEV) for x in _jets(33, 30, s, [(1, 12), (20, 25)])) for s in (21, 22, 23)]
    edges = A.pack_edges([np.linspace(-2, 2, 82), np.linspace(-1, 1, 11), np.linspace(-3, 3, 1025)])
    t, r = ins[0][0].clone(), ins[0][1].clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        out = A.recon_analysis(t, r)
        A.histogram(out["rel_err"][0].view(-1, 3), edges, keep=~out["is_padded"].view(-1))
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = A.recon_analysis(t, r)
        hist = A.histogram(out["rel_err"][0].view(-1, 3), edges, keep=~out["is_padded"].view(-1))
    for x, y in ins[1:]:
        t.copy_(x), r.copy_(y)
        g.replay()
        torch.cuda.synchronize()
        eager = A.recon_analysis(x, y)
        for k in eager:
            assert np.array_equal(out[k].cpu().numpy(), eager[k].cpu().numpy(), equal_nan=True), k
        assert torch.equal(hist, A.histogram(eager["rel_err"][0].view(-1, 3), edges, keep=~eager["is_padded"].view(-1)))


def test_get_rel_err_find_match_drop_in():
    from lgn import analysis as A
    z = U.load("g22_analysis_n12.npz")
    B, N = z["target"].shape[:2]
    t, r = torch.from_numpy(z["target"]), torch.from_numpy(z["recons"])
    fr = [t[..., 1:], r[..., 1:]] + [torch.from_numpy(z[k][s]) for k in ("part_polar", "part_polarrel") for s in (0, 1)]
    out = A.get_rel_err_find_match(*fr)
    assert len(out) == 3 and all(o.shape == (B * N, 3) and o.device.type == "cpu" and o.dtype == torch.float64 for o in out)
    for f in range(3):          # given the fixture's own frames the costs are the host's, bit for bit: so are the matchings
        assert_same(out[f].numpy().reshape(B, N, 3), z["rel_err"][f], ARITH, f"drop-in frame {f}")
    assert_same(A.get_p_polar_tensor(t).numpy(), z["part_polar"][0], TRANS, "get_p_polar_tensor")
    flat = A.get_p_polar_tensor(t[..., 1:].reshape(-1, 3))            # element-wise on any shape: B * N = 192 rows here, 3-vectors
    assert flat.shape == (B * N, 3)
    twice = A.get_p_polar_tensor(torch.cat([t.reshape(-1, 4)] * 2))    # 384 rows: more than a jet may hold
    assert torch.equal(twice[:B * N], flat) and torch.equal(twice[B * N:], flat)
    assert_same(flat.numpy().reshape(B, N, 3), z["part_polar"][0], TRANS, "get_p_polar_tensor, flattened")
    assert_same(A.get_p_polarrel_tensor(r).numpy(), z["part_polarrel"][1], TRANS, "get_p_polarrel_tensor")
    jc = A.get_jet_feature_cartesian(t, return_arr=True)
    assert isinstance(jc, torch.Tensor) and jc.shape == (B, 4) and len(A.get_jet_feature_cartesian(t)) == 4
    assert_same(jc.numpy()[:, 1:], z["jet_cart"][0][:, 1:], ARITH, "get_jet_feature_cartesian")
    jp = A.get_jet_feature_polar(r, return_arr=True)
    assert isinstance(jp, np.ndarray) and isinstance(A.get_jet_feature_polar(r)[0], np.ndarray)
    assert_same(jp[:, 1:], z["jet_polar"][1][:, 1:], TRANS, "get_jet_feature_polar")
    bad = [x.clone() for x in fr]
    bad[1][2, 1, 0] = float("nan")
    with pytest.raises(ValueError, match="invalid numeric entries"):
        A.get_rel_err_find_match(*bad)


def test_analysis_after_the_native_eval_step():
    """The per-epoch path: NativeEvalStep.run()'s reconstruction and its target go into recon_analysis as device tensors; the result
    is that of the same tensors copied to the host and back."""
    import __graft_entry__ as G
    from lgn import analysis as A
    from lgn.step import NativeEvalStep
    B, N = 8, 30
    enc, dec = G._models(N, (3, 3, 4, 4), (4, 4, 3, 3), torch.device(DEV))
    from oracle import lgn_oracle as O
    p4, labels = O.synthetic_jets(B, N, seed=3, pad=True)
    batch = {"p4": p4.to(DEV), "labels": labels.to(DEV)}
    out = NativeEvalStep(enc, dec, B, get_real_method="real").run(batch)
    recon, target = out["recon"], batch["p4"]
    assert recon.is_cuda and recon.shape == (B, N, 4)
    dev = A.recon_analysis(target, recon)
    host = A.recon_analysis(target.cpu(), recon.cpu())
    assert set(dev) == set(host)
    for k in dev:
        assert dev[k].is_cuda and np.array_equal(dev[k].cpu().numpy(), host[k].cpu().numpy(), equal_nan=True), k
    assert dev["is_padded"].any() and (dev["status"] == 0).all()
