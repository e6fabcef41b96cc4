"""GPU tests of the matrix gradients of the EMD (csrc/emd_pairs_grad.hip; lgn.emd.emds_pair_grads, emds_grad and
emds_differentiable(backward="native")): every pair's value against emds() and its gradients against emd_grad() bit for bit, the
weighted sum against its numpy restatement (tests/_emd_pairs_grad_ref.py) bit for bit, independence of the row chunks, of kept slabs
and of the run, the composition emds_differentiable(backward="rows"), central differences through emds(), statuses, and capture.
The events are random and continuous (tests/_emd_opts_grad_ref.events), so that every optimum is unique."""
import numpy as np
import pytest
import torch

import _emd_opts_grad_ref as GO
import _emd_pairs_grad_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
OPTION_SETS = {
    "defaults": dict(),
    "beta2": dict(beta=2.0),
    "norm": dict(norm=True),
    "R_beta15_periodic": dict(R=0.8, beta=1.5, periodic_phi=True),
    "all": dict(R=0.8, beta=1.5, norm=True, periodic_phi=True),
}
# both flow placements (LDS up to 86 particles), every count of columns per lane (m + 1 <= 64, 128, 192) and the 86 | 87 boundary
SHAPES = [(1, 1), (5, 8), (30, 30), (63, 64), (86, 86), (87, 87), (127, 128), (191, 191)]


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _sets(seed, B0, B1, n, m, o):
    rng = np.random.default_rng(seed)
    periodic = bool(o.get("periodic_phi"))
    return GO.events(rng, B0, n, periodic), GO.events(rng, B1, m, periodic)


def _upstream(rng, B0, B1):
    """a random upstream matrix with zeros and negative entries"""
    G = rng.normal(size=(B0, B1))
    G[rng.random((B0, B1)) < 0.25] = 0.0
    G.flat[0] = -abs(G.flat[0]) - 0.5
    return G


# ---- 1. every pair: the bits of emds() and of emd_grad() ----------------------------------------------------------------------------------

@pytest.mark.parametrize("opt", list(OPTION_SETS))
@pytest.mark.parametrize("n,m", SHAPES)
def test_every_pair_has_the_bits_of_emds_and_of_emd_grad(n, m, opt):
    from lgn import emd as M
    o = OPTION_SETS[opt]
    X0, X1 = _sets(1000 * n + m, 3, 2, n, m, o)
    forms = [(dev(X0), dev(X1), [(i, j) for i in range(3) for j in range(2)])]
    if n == m:
        forms.append((dev(X0), None, R.upper_pairs(3)))
    for x0, x1, pairs in forms:
        E, s0, s1, st = M.emds_pair_grads(x0, x1, **o)
        assert (st == 0).all(), st
        assert torch.equal(E, M.emds(x0, x1, **o))
        ii, jj = [p[0] for p in pairs], [p[1] for p in pairs]
        _, g0, g1 = M.emd_grad(x0[ii], (x0 if x1 is None else x1)[jj], **o)         # the ordered pairs, as aligned pairs
        assert s0.shape == g0.shape and s1.shape == g1.shape
        assert torch.equal(s0, g0) and torch.equal(s1, g1), (n, m, opt, x1 is None)
        assert torch.isfinite(s0).all() and torch.isfinite(s1).all() and float(s0.abs().max()) > 0


# ---- 2. the weighted sum: the bits of the restatement -----------------------------------------------------------------------------------

@pytest.mark.parametrize("opt", ["defaults", "all"])
@pytest.mark.parametrize("B0,B1", [(3, 4), (1, 4), (3, 1), (4, None), (2, None)])
def test_the_weighted_sum_has_the_bits_of_the_restatement(B0, B1, opt):
    """B1 = None is the symmetric form.  G = None is G = ones; a one-hot G returns that pair's emd_grad() gradients and zeros."""
    from lgn import emd as M
    o = OPTION_SETS[opt]
    sym = B1 is None
    n, m = (6, 6) if sym else (5, 8)
    X0, X1 = _sets(50 * B0 + (B1 or 0), B0, B1 or B0, n, m, o)
    x0, x1 = dev(X0), (None if sym else dev(X1))
    cols = B0 if sym else B1
    G = _upstream(np.random.default_rng(7 + B0), B0, cols)
    E, s0, s1, _ = M.emds_pair_grads(x0, x1, **o)
    s0, s1 = s0.cpu().numpy(), s1.cpu().numpy()

    def want(W):
        return (R.reduce_upper(s0, s1, W, B0), None) if sym else R.reduce_full(s0, s1, W, B0, B1)

    def got(W):
        E2, g0, g1 = M.emds_grad(x0, x1, None if W is None else dev(W), **o)
        assert torch.equal(E2, E) and (g1 is None) == sym
        return g0.cpu().numpy(), (None if sym else g1.cpu().numpy())

    for W in (G, None, np.ones((B0, cols))):
        for g, w in zip(got(W), want(W)):
            assert (g is None and w is None) or np.array_equal(g, w), (B0, B1, opt)
    ones, none = got(np.ones((B0, cols))), got(None)
    assert np.array_equal(ones[0], none[0]) and (sym or np.array_equal(ones[1], none[1]))
    if B0 * cols > 1:
        i, j = B0 - 1, 0                                                             # (symmetric: below the diagonal, the pair (0, B0 - 1))
        hot = np.zeros((B0, cols))
        hot[i, j] = 1.0
        g0, g1 = got(hot)
        if sym:
            _, p0, p1 = M.emd_grad(x0[0:1], x0[B0 - 1:B0], **o)
            expect = np.zeros_like(g0)
            expect[0], expect[B0 - 1] = p0[0].cpu().numpy(), p1[0].cpu().numpy()
            assert (g0 == expect).all()
        else:
            _, p0, p1 = M.emd_grad(x0[i:i + 1], x1[j:j + 1], **o)
            e0, e1 = np.zeros_like(g0), np.zeros_like(g1)
            e0[i], e1[j] = p0[0].cpu().numpy(), p1[0].cpu().numpy()
            assert (g0 == e0).all() and (g1 == e1).all()


# ---- 3. chunks, kept slabs and runs ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("sym", [False, True])
def test_the_bits_do_not_depend_on_chunks_kept_slabs_or_the_run(sym):
    from lgn import emd as M
    o = OPTION_SETS["all"]
    B0, B1, n, m = (5, 5, 7, 7) if sym else (5, 3, 7, 9)
    X0, X1 = _sets(77 + sym, B0, B1, n, m, o)
    x0, x1 = dev(X0), (None if sym else dev(X1))
    G = dev(_upstream(np.random.default_rng(5), B0, B1))
    one_row = (B0 - 1 if sym else B1) * (n + m) * 24                                 # (symmetric: the longest row)
    whole = M.emds_grad(x0, x1, G, **o)
    for limit in (one_row, 2 * one_row, 0):
        part = M.emds_grad(x0, x1, G, max_slab_bytes=limit, **o)
        assert all((a is None and b is None) or torch.equal(a, b) for a, b in zip(whole, part)), limit
    again = M.emds_grad(x0, x1, G, **o)
    assert all((a is None and b is None) or torch.equal(a, b) for a, b in zip(whole, again))

    def autograd(**kw):
        a, b = x0.clone().requires_grad_(True), (None if sym else x1.clone().requires_grad_(True))
        out = M.emds_differentiable(a, b, backward="native", **kw, **o)
        assert torch.equal(out.detach(), whole[0])
        (out * G).sum().backward()
        return a.grad, (None if sym else b.grad)

    for kw in (dict(), dict(keep_bytes=0), dict(keep_bytes=0, chunk_pairs=1), dict()):
        g0, g1 = autograd(**kw)
        assert torch.equal(g0, whole[1]) and (sym or torch.equal(g1, whole[2])), kw
    # one side alone is the same gradient
    if not sym:
        a = x0.clone().requires_grad_(True)
        (M.emds_differentiable(a, x1, backward="native", **o) * G).sum().backward()
        b = x1.clone().requires_grad_(True)
        (M.emds_differentiable(x0, b, backward="native", keep_bytes=0, **o) * G).sum().backward()
        assert torch.equal(a.grad, whole[1]) and torch.equal(b.grad, whole[2])


# ---- 4. the composition -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("opt", ["defaults", "all"])
@pytest.mark.parametrize("sym", [False, True])
def test_native_backward_against_the_composition(sym, opt):
    """Forward: the same bits.  FULL: both sum the same terms G[i, j] s[i, j], in their own orders: within (T + 1) 2^-52 of the sum of
    the absolute terms (T terms per sum; taken from the slabs).  UPPER: the composition solves every pair in both orders, whose
    gradients agree as solutions do, not to the bit: 1e-12 of the largest entry, the tolerance of the project's formula checks."""
    from lgn import emd as M
    o = OPTION_SETS[opt]
    B0, B1, n, m = (4, 4, 6, 6) if sym else (3, 4, 5, 8)
    X0, X1 = _sets(31 + sym, B0, B1, n, m, o)
    W = _upstream(np.random.default_rng(3), B0, B1)
    grads = {}
    for how in ("rows", "native"):
        a, b = dev(X0).requires_grad_(True), (None if sym else dev(X1).requires_grad_(True))
        out = M.emds_differentiable(a, b, backward=how, **o)
        assert torch.equal(out.detach(), M.emds(dev(X0), None if sym else dev(X1), **o))
        (out * dev(W)).sum().backward()
        grads[how] = (a.grad.cpu().numpy(), None if sym else b.grad.cpu().numpy())
    if sym:
        top = np.abs(grads["rows"][0]).max()
        err = np.abs(grads["native"][0] - grads["rows"][0]).max()
        print(f"UPPER {opt}: |native - rows| = {err:.3e}, largest entry {top:.3e}")
        assert top > 0 and err <= 1e-12 * top
    else:
        _, s0, s1, _ = M.emds_pair_grads(dev(X0), dev(X1), **o)
        a0, a1 = R.abs_terms_full(s0.cpu().numpy(), s1.cpu().numpy(), W, B0, B1)
        for k, (a, T) in enumerate(((a0, B1), (a1, B0))):
            err = np.abs(grads["native"][k] - grads["rows"][k])
            print(f"FULL {opt} side {k}: max |native - rows| = {err.max():.3e}, T = {T}")
            assert (err <= (T + 1) * 2.0 ** -52 * a).all()


# ---- 5. central differences through emds() -----------------------------------------------------------------------------------------------

def test_the_gradient_is_the_central_difference_of_the_weighted_matrix():
    """sum(G * emds(X0, X1)) at B0 = 3, B1 = 2, n = 5, m = 4 under beta = 2, norm; 1e-7 of the largest entry, what the host tests hold
    the restatement to against central differences (step 1e-6)."""
    from lgn import emd as M
    o = dict(beta=2.0, norm=True)
    X0, X1 = _sets(99, 3, 2, 5, 4, o)
    G = _upstream(np.random.default_rng(1), 3, 2)
    Gd = dev(G)
    _, g0, g1 = M.emds_grad(dev(X0), dev(X1), Gd, **o)

    def value(A, B):
        E, st = M.emds(dev(A), dev(B), return_status=True, **o)
        return float((E * Gd).sum())

    h = 1e-6
    fd = [np.zeros_like(X0), np.zeros_like(X1)]
    for side in (0, 1):
        base = [X0.copy(), X1.copy()]
        for idx in np.ndindex(*base[side].shape):
            x = base[side][idx]
            base[side][idx] = x + h
            up = value(*base)
            base[side][idx] = x - h
            dn = value(*base)
            base[side][idx] = x
            fd[side][idx] = (up - dn) / (2 * h)
    top = max(np.abs(fd[0]).max(), np.abs(fd[1]).max())
    err = max(np.abs(g0.cpu().numpy() - fd[0]).max(), np.abs(g1.cpu().numpy() - fd[1]).max())
    print(f"|native - central differences| = {err:.3e}, largest entry {top:.3e}")
    assert top > 0 and err <= 1e-7 * top


# ---- 6. statuses ----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("sym", [False, True])
def test_a_weightless_event_under_norm_marks_its_row_as_the_composition_does(sym):
    from lgn import emd as M
    o = dict(norm=True)
    B0, B1, n, m = (4, 4, 5, 5) if sym else (3, 2, 5, 4)
    X0, X1 = _sets(13 + sym, B0, B1, n, m, o)
    X0[1, :, 0] = 0.0
    W = dev(_upstream(np.random.default_rng(2), B0, B1))
    x0, x1 = dev(X0), (None if sym else dev(X1))
    E, g0, g1, st = M.emds_grad(x0, x1, W, return_status=True, **o)
    want = torch.zeros(B0, B1, dtype=torch.int32, device=DEV)
    want[1, :] = M.EMPTY
    if sym:
        want[:, 1] = M.EMPTY
        want[1, 1] = 0
    assert torch.equal(st, want)
    assert torch.equal(st, M.emds(x0, x1, return_status=True, **o)[1])
    a, b = x0.clone().requires_grad_(True), (None if sym else x1.clone().requires_grad_(True))
    out = M.emds_differentiable(a, b, **o)                                          # the composition
    (out * W).sum().backward()
    assert torch.equal(torch.isnan(E), torch.isnan(out.detach())) and torch.equal(torch.isnan(E), st != 0)
    assert torch.equal(torch.isnan(g0), torch.isnan(a.grad)) and torch.isnan(g0[1]).all()
    if sym:
        assert torch.isnan(g0).all()                                                  # every event meets the weightless one
    else:
        assert torch.equal(torch.isnan(g1), torch.isnan(b.grad)) and torch.isnan(g1).all() and not torch.isnan(g0[[0, 2]]).any()
    # a zero weight on the flagged pairs does not hide them
    W0 = W.clone()
    W0[1, :] = 0.0
    W0[:, 1] = 0.0 if sym else W0[:, 1]
    _, h0, h1, _ = M.emds_grad(x0, x1, W0, return_status=True, **o)
    assert torch.equal(torch.isnan(h0), torch.isnan(g0)) and (sym or torch.equal(torch.isnan(h1), torch.isnan(g1)))
    _, s0, s1, _ = M.emds_pair_grads(x0, x1, **o)
    pairs = R.upper_pairs(B0) if sym else [(i, j) for i in range(B0) for j in range(B1)]
    flagged = [p for p, (i, j) in enumerate(pairs) if i == 1 or (sym and j == 1)]
    assert torch.isnan(s0[flagged]).all() and torch.isnan(s1[flagged]).all()
    rest = [p for p in range(s0.shape[0]) if p not in flagged]
    assert torch.isfinite(s0[rest]).all() and torch.isfinite(s1[rest]).all()
    with pytest.raises(ValueError, match=r"cannot be normalised \(pair \(0, 1\)" if sym else r"cannot be normalised \(pair \(1, 0\)"):
        M.emds_grad(x0, x1, W, **o)


# ---- 7. capture -------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("sym", [False, True])
def test_a_captured_call_replays_the_eager_bits(sym):
    """One stream, no branches; three pairs per row chunk, so that the continued sums are captured too."""
    from lgn import emd as M
    o = OPTION_SETS["all"]
    B0, B1, n, m = (4, 4, 6, 6) if sym else (4, 3, 6, 9)
    X0, X1 = _sets(21 + sym, B0, B1, n, m, o)
    x0, x1 = dev(X0), (None if sym else dev(X1))
    G = dev(_upstream(np.random.default_rng(4), B0, B1))
    kw = dict(return_status=True, max_slab_bytes=3 * (n + m) * 24, **o)
    eager = M.emds_grad(x0, x1, G, **kw)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        M.emds_grad(x0, x1, G, **kw)                                                  # warm-up outside the capture
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            out = M.emds_grad(x0, x1, G, **kw)                                        # (return_status: no host sync)
    torch.cuda.current_stream().wait_stream(side)
    for _ in range(2):
        for x in out:
            if x is not None:
                x.fill_(-1)
        graph.replay()
        torch.cuda.synchronize()
        assert all((x is None and y is None) or torch.equal(x, y) for x, y in zip(out, eager))
