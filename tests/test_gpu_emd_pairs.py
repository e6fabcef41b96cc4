"""GPU tests of the EMD matrices and energyflow's options (csrc/emd_pairs.hip; lgn.emd.emds, lgn.emd.emd(beta, norm, periodic_phi)):
the bits of the existing solver at default options in every pair mode and on both flow placements, the optimality certificate and the
LP restatement (tests/_emd_pairs_ref.py) under the options, statuses that stay with their pair, refusals, and graph capture."""
import numpy as np
import pytest
import torch

import _emd_pairs_ref as P

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FULL, UPPER, ALIGNED = 0, 1, 2


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def events(rng, B, n, spread=0.4, periodic=False):
    """[B][n][3] events of (pT, y, phi) with random positive weights; periodic: phi uniform in [0, 2 pi)"""
    phi = rng.uniform(0, 2 * np.pi, (B, n)) if periodic else rng.normal(size=(B, n)) * spread
    return np.stack([rng.random((B, n)) + 0.05, rng.normal(size=(B, n)) * spread, phi], axis=-1)


def same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int64), b.contiguous().view(torch.int64))


def pairs_call(ev0, ev1, mode, opts=None, want_flow=False):
    """lgn_emd_pairs_f64 directly: (emd, status[, flow, dual0, dual1])"""
    from lgn import _native as N
    B0, n = ev0.shape[:2]
    B1, m = (B0, n) if ev1 is None else ev1.shape[:2]
    shape = (B0,) if mode == ALIGNED else (B0, B1)
    out = torch.empty(shape, device=DEV, dtype=torch.float64)
    st = torch.empty(shape, device=DEV, dtype=torch.int32)
    extra = [torch.empty(B0, n + 1, m + 1, device=DEV, dtype=torch.float64), torch.empty(B0, n + 1, device=DEV, dtype=torch.float64),
             torch.empty(B0, m + 1, device=DEV, dtype=torch.float64)] if want_flow else [None] * 3
    npairs = {FULL: B0 * B1, UPPER: max(B0 * (B0 - 1) // 2, 1), ALIGNED: B0}[mode]
    need = N.lib().lgn_emd_workspace_bytes(npairs, max(n, m))
    work = torch.empty(need, device=DEV, dtype=torch.uint8) if need else None
    rc = N.lib().lgn_emd_pairs_f64(N.ptr(ev0), N.ptr(ev1), B0, B1, n, m, mode, opts, N.ptr(out), *[N.ptr(x) for x in extra], N.ptr(st),
                                   N.ptr(work), need, N.stream_ptr())
    assert rc == 0, N.last_error()
    return (out, st, *extra) if want_flow else (out, st)


# ---- 1. the bits of the existing solver at default options -----------------------------------------------------------------------------

@pytest.mark.parametrize("R", [1.0, 0.4])
def test_full_matrix_has_the_bits_of_emd_pair_by_pair(R):
    from lgn import emd as M
    rng = np.random.default_rng(35)
    X0, X1 = dev(events(rng, 3, 7)), dev(events(rng, 5, 12))
    got, st = M.emds(X0, X1, R=R, return_status=True)
    assert got.shape == (3, 5) and got.dtype == torch.float64 and st.dtype == torch.int32 and (st.cpu() == 0).all()
    for i in range(3):
        for j in range(5):
            assert same_bits(got[i, j], M.emd(X0[i], X1[j], R=R)), (i, j)


@pytest.mark.parametrize("n,m", [(1, 64), (63, 64), (64, 63), (127, 30)])
def test_aligned_mode_has_the_bits_of_lgn_emd_f64(n, m):
    """The edges of the columns-per-lane layout (m + 1 = 65, 65, 64, 31 columns: 2, 2, 1, 1 per lane) and both flow placements."""
    from lgn import emd as M
    rng = np.random.default_rng(1000 * n + m)
    a, b = dev(events(rng, 3, n)), dev(events(rng, 3, m))
    want = M.emd(a, b, return_flow=True, return_duals=True, return_status=True)
    val, st, flow, d0, d1 = pairs_call(a, b, ALIGNED, None, want_flow=True)
    assert (st.cpu() == 0).all() and torch.equal(st, want[4])
    for got, ref, what in ((val, want[0], "value"), (flow, want[1], "flow"), (d0, want[2], "dual0"), (d1, want[3], "dual1")):
        assert same_bits(got, ref), what


def test_upper_mode_is_symmetric_with_a_zero_diagonal():
    from lgn import emd as M
    rng = np.random.default_rng(59)
    x = events(rng, 5, 9)
    x[2, 3, 1] = np.nan                                # the diagonal is +0.0 with status 0 whatever the event holds
    X = dev(x)
    got, st = M.emds(X, return_status=True)
    assert got.shape == (5, 5) and same_bits(got, got.t())
    assert same_bits(got.diagonal(), torch.zeros(5, device=DEV, dtype=torch.float64)) and (st.diagonal().cpu() == 0).all()
    assert torch.equal(st, st.t())
    for i in range(5):
        for j in range(i + 1, 5):
            val, s = M.emd(X[i], X[j], return_status=True)
            assert same_bits(got[i, j], val) and int(st[i, j]) == int(s) == (M.INVALID if 2 in (i, j) else 0), (i, j)
    one, st1 = M.emds(X[:1], return_status=True)
    assert one.shape == (1, 1) and same_bits(one, torch.zeros(1, 1, device=DEV, dtype=torch.float64)) and int(st1[0, 0]) == 0
    # ev1 == ev0 is the other spelling of the symmetric form
    again, st2 = pairs_call(X, X, UPPER)
    assert same_bits(again, got) and torch.equal(st2, st)


def test_upper_mode_at_two_million_pairs():
    """B = 2049 events of 2 particles: 2,098,176 pairs, more than the persistent grid holds at once: grid striding and the decode at
    scale, every i < j entry against emd() on the gathered pairs."""
    from lgn import emd as M
    rng = np.random.default_rng(2049)
    X = dev(events(rng, 2049, 2))
    got, st = M.emds(X, return_status=True)
    assert (st == 0).all()
    iu = torch.triu_indices(2049, 2049, offset=1, device=DEV)
    assert iu.shape[1] == 2098176
    want = M.emd(X[iu[0]], X[iu[1]])
    assert same_bits(got[iu[0], iu[1]], want)
    assert same_bits(got, got.t()) and same_bits(got.diagonal(), torch.zeros(2049, device=DEV, dtype=torch.float64))


def test_the_workspace_path_and_its_refusal():
    from lgn import _native as N
    from lgn import emd as M
    assert not M.flow_in_lds(87)
    rng = np.random.default_rng(87)
    X0, X1 = dev(events(rng, 3, 87)), dev(events(rng, 2, 87))
    got, st = M.emds(X0, X1, return_status=True)
    assert (st.cpu() == 0).all()
    i, j = torch.arange(3, device=DEV).repeat_interleave(2), torch.arange(2, device=DEV).repeat(3)
    assert same_bits(got.reshape(-1), M.emd(X0[i], X1[j]))
    lib = N.lib()
    need = lib.lgn_emd_workspace_bytes(6, 87)
    assert need == 6 * 88 * 88 * 8
    work = torch.empty(need, device=DEV, dtype=torch.uint8)
    out, flag = torch.full((3, 2), -7.0, device=DEV, dtype=torch.float64), torch.full((3, 2), -7, device=DEV, dtype=torch.int32)
    args = (N.ptr(X0), N.ptr(X1), 3, 2, 87, 87, FULL, None, N.ptr(out), None, None, None, N.ptr(flag))
    assert lib.lgn_emd_pairs_f64(*args, N.ptr(work), need - 8, N.stream_ptr()) < 0 and "too short" in N.last_error()
    assert lib.lgn_emd_pairs_f64(*args, None, 0, N.stream_ptr()) < 0 and "null work" in N.last_error()
    flow = torch.empty(6 * 88 * 88, device=DEV, dtype=torch.float64)
    assert lib.lgn_emd_pairs_f64(*args[:9], N.ptr(flow), None, None, N.ptr(flag), N.ptr(work), need, N.stream_ptr()) < 0
    assert "ALIGNED mode only" in N.last_error()
    torch.cuda.synchronize()
    assert (out.cpu() == -7.0).all() and (flag.cpu() == -7).all()          # nothing ran
    assert lib.lgn_emd_pairs_f64(*args, N.ptr(work), need, N.stream_ptr()) == 0
    assert (flag.cpu() == 0).all() and same_bits(out, got)


# ---- 2. the options -----------------------------------------------------------------------------------------------------------------

OPTIONS = {"beta2": dict(beta=2.0), "beta05": dict(beta=0.5), "periodic": dict(periodic_phi=True), "norm": dict(norm=True),
           "all": dict(R=0.8, beta=2.0, norm=True, periodic_phi=True)}


@pytest.mark.parametrize("n,m", [(12, 12), (30, 17)])
@pytest.mark.parametrize("name", list(OPTIONS))
def test_the_options_are_optimal(name, n, m):
    """ALIGNED with flow and duals: the project's certificate under the option cost matrix and weights of the restatement."""
    from lgn import emd as M
    opts = OPTIONS[name]
    rng = np.random.default_rng(100 * n + m)
    periodic = bool(opts.get("periodic_phi"))
    a, b = events(rng, 4, n, periodic=periodic), events(rng, 4, m, periodic=periodic)
    val, flow, d0, d1, st = (x.cpu().numpy() for x in M.emd(dev(a), dev(b), return_flow=True, return_duals=True, return_status=True, **opts))
    assert (st == 0).all(), st
    for k in range(4):
        P.certify(val[k], flow[k], d0[k], d1[k], a[k], b[k], **opts)


@pytest.fixture(scope="module")
def option_events():
    rng = np.random.default_rng(34)
    return events(rng, 3, 10, spread=1.0, periodic=True), events(rng, 4, 10, spread=1.0, periodic=True)


@pytest.mark.parametrize("name", list(OPTIONS))
def test_the_options_have_the_value_of_the_restatement(name, option_events):
    """rtol 1e-11: the bound of the existing EMD tests wherever a device transcendental is involved (here pow)."""
    from lgn import emd as M
    x0, x1 = option_events
    opts = OPTIONS[name]
    got = M.emds(dev(x0), dev(x1), **opts).cpu().numpy()
    np.testing.assert_allclose(got, P.emds(x0, x1, **opts), rtol=1e-11, atol=1e-300)
    if name == "norm":                                   # the same LP as the existing solver on events normalised on the host
        h0, h1 = x0.copy(), x1.copy()
        h0[..., 0] /= h0[..., 0].sum(-1, keepdims=True)
        h1[..., 0] /= h1[..., 0].sum(-1, keepdims=True)
        i, j = np.repeat(np.arange(3), 4), np.tile(np.arange(4), 3)
        want = M.emd(dev(h0[i]), dev(h1[j])).cpu().numpy().reshape(3, 4)
        np.testing.assert_allclose(got, want, rtol=1e-12, atol=1e-300)
    if name == "periodic":                               # symmetric form under an option
        sym = M.emds(dev(x0), **opts).cpu().numpy()
        np.testing.assert_allclose(sym, P.emds(x0, **opts), rtol=1e-11, atol=1e-300)


# ---- 3. statuses ----------------------------------------------------------------------------------------------------------------------

def test_statuses_stay_with_their_pair():
    from lgn import emd as M
    rng = np.random.default_rng(7)
    x0, x1 = events(rng, 4, 8), events(rng, 3, 11)
    clean0, clean1 = dev(x0), dev(x1)
    x0, x1 = x0.copy(), x1.copy()
    x0[1, 5, 2] = np.nan
    x0[2, :, 0] = 0.0
    x1[0, :, 0] = 0.0
    X0, X1 = dev(x0), dev(x1)
    for norm in (False, True):
        ref = M.emds(clean0, clean1, norm=norm)
        got, st = M.emds(X0, X1, norm=norm, return_status=True)
        st = st.cpu().numpy()
        assert (st[1] == M.INVALID).all() and torch.isnan(got[1]).all()
        assert st[2, 0] == M.EMPTY and torch.isnan(got[2, 0])
        if norm:
            assert (st[2] == M.EMPTY).all() and (st[[0, 2, 3], 0] == M.EMPTY).all()
            assert torch.isnan(got[2]).all() and torch.isnan(got[[0, 2, 3], 0]).all()
            good = [(i, j) for i in (0, 3) for j in (1, 2)]
        else:
            assert (st[2, 1:] == 0).all() and (st[[0, 3], 0] == 0).all()
            np.testing.assert_allclose(got[2, 1:].cpu().numpy(), x1[1:, :, 0].sum(-1), rtol=1e-12)      # the other event's sum pT
            np.testing.assert_allclose(got[[0, 3], 0].cpu().numpy(), x0[[0, 3], :, 0].sum(-1), rtol=1e-12)
            good = [(i, j) for i in (0, 3) for j in (1, 2)]
        for i, j in good:
            assert st[i, j] == 0 and same_bits(got[i, j], ref[i, j]), (norm, i, j)
        with pytest.raises(ValueError, match=r"pair \(\d+, \d+\)"):
            M.emds(X0, X1, norm=norm)


# ---- 4. capture -----------------------------------------------------------------------------------------------------------------------

def test_a_captured_call_replays_the_eager_bits():
    from lgn import emd as M
    rng = np.random.default_rng(11)
    X0, X1 = dev(events(rng, 6, 10)), dev(events(rng, 5, 14))
    eager, eager_st = M.emds(X0, X1, return_status=True)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        M.emds(X0, X1, return_status=True)               # warm-up outside the capture
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            out, st = M.emds(X0, X1, return_status=True)     # (return_status: no host sync, which a capture does not admit)
    torch.cuda.current_stream().wait_stream(side)
    for _ in range(2):
        out.fill_(-1.0)
        st.fill_(-1)
        graph.replay()
        torch.cuda.synchronize()
        assert same_bits(out, eager) and torch.equal(st, eager_st)
