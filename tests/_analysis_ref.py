"""numpy / scipy restatement of the numeric half of the reference's plot_p (utils/jet_analysis/utils.py, particle_recon_err.py,
jet_recon_err.py) as lgn_recon_analysis_f64 computes it, and of np.histogram's membership rule over explicit edges as
lgn_histogram_f64 applies it.  Costs are exact Euclidean distances, the assignment is scipy's linear_sum_assignment (its restatement
in _anomaly_ref.py where scipy is absent).  Not a test module."""
import numpy as np

import _anomaly_ref as A

try:
    from scipy.optimize import linear_sum_assignment as _scipy_lsa
except ImportError:          # pragma: no cover
    _scipy_lsa = None

EPS = 1e-16


def lsap(cost):
    """col_ind of scipy.optimize.linear_sum_assignment(cost); ValueError as scipy raises it."""
    if _scipy_lsa is not None:
        return _scipy_lsa(cost)[1]
    return A.lsap(cost)


def p_polar(p):
    """get_p_polar_tensor(p, eps=1e-16): (.., 3 or 4) -> (pt, eta, phi)."""
    px, py, pz = p[..., -3], p[..., -2], p[..., -1]
    pt = np.sqrt(px * px + py * py)
    with np.errstate(all="ignore"):
        return np.stack((pt, np.arcsinh(pz / (pt + EPS)), np.arctan2(py + EPS, px)), axis=-1)


def p_polarrel(p):
    """get_p_polarrel_tensor(p, eps=1e-16)."""
    pt, eta, phi = np.moveaxis(p_polar(p), -1, 0)
    Pt, Eta, Phi = np.moveaxis(p_polar(p.sum(-2, keepdims=True)), -1, 0)
    with np.errstate(all="ignore"):
        return np.stack((pt / (Pt + EPS), Eta - eta, np.remainder((Phi - phi) + np.pi, 2 * np.pi) - np.pi), axis=-1)


def jet_cartesian(p):
    """get_jet_feature_cartesian(p, return_arr=True): (B, N, 4) -> (B, 4) (m, px, py, pz)."""
    E, px, py, pz = np.moveaxis(p.sum(-2), -1, 0)
    msq = ((E * E - px * px) - py * py) - pz * pz
    return np.stack((np.sqrt(np.abs(msq)) * np.sign(msq), px, py, pz), axis=-1)


def jet_polar(p):
    """get_jet_feature_polar(p, return_arr=True): (m, pt, eta, phi), phi without eps."""
    m, px, py, pz = np.moveaxis(jet_cartesian(p), -1, 0)
    pt = np.sqrt(px * px + py * py)
    with np.errstate(all="ignore"):
        return np.stack((m, pt, np.arcsinh(pz / (pt + EPS)), np.arctan2(py, px)), axis=-1)


def jet_msq(p):
    """(m^2, E^2 + |p|^2) of the summed jet: the tests compare masses through m^2 with the cancellation bound of the sum."""
    E, px, py, pz = np.moveaxis(p.sum(-2), -1, 0)
    return ((E * E - px * px) - py * py) - pz * pz, E * E + px * px + py * py + pz * pz


def cost3(t, r):
    """|t_i - r_j| on three components: a square root of an ordered sum of squares."""
    d = t[..., :, None, :] - r[..., None, :, :]
    with np.errstate(all="ignore"):
        return np.sqrt((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2])


def matched_rel_err(t3, r3, tp, rp, tq, rq):
    """get_rel_err_find_match on given frames (B, N, 3) -> (rel_err [3][B][N][3], col4row [2][B][N], status [B])."""
    B, N, _ = t3.shape
    out = np.full((3, B, N, 3), np.nan)
    col = np.full((2, B, N), -1, dtype=np.int64)
    status = np.zeros(B, dtype=np.int32)
    c0, c1 = cost3(t3, r3), cost3(tq, rq)
    for b in range(B):
        got = []
        for c in (c0[b], c1[b]):
            try:
                got.append(lsap(c))
            except ValueError as e:
                status[b] |= 256 if "infeasible" in str(e) else 1
        if status[b]:
            continue
        col[0, b], col[1, b] = got
        with np.errstate(all="ignore"):
            out[0, b] = (r3[b][got[0]] - t3[b]) / t3[b]
            out[1, b] = (rp[b][got[0]] - tp[b]) / (tp[b] + EPS)
            out[2, b] = (rq[b][got[1]] - tq[b]) / (tq[b] + EPS)
    return out, col, status


def recon_analysis(target, recons, abs_coord=True, find_match=True):
    """Every array of lgn_recon_analysis_f64, named as lgn.analysis.recon_analysis names them."""
    target, recons = np.asarray(target, dtype=np.float64), np.asarray(recons, dtype=np.float64)
    B, N, _ = target.shape
    t3, r3 = target[..., 1:], recons[..., 1:]
    tp, rp = p_polar(target), p_polar(recons)
    tq, rq = (p_polarrel(target), p_polarrel(recons)) if abs_coord else (tp, rp)
    jc, jp = np.stack((jet_cartesian(target), jet_cartesian(recons))), np.stack((jet_polar(target), jet_polar(recons)))
    with np.errstate(all="ignore"):
        jre = np.stack(((jc[1] - jc[0]) / (jc[1] + EPS), (jp[1] - jp[0]) / (jp[1] + EPS)))
    out = dict(part_polar=np.stack((tp, rp)), part_polarrel=np.stack((tq, rq)), jet_cart=jc, jet_polar=jp, jet_rel_err=jre,
               jet_keep=np.stack(((jc[0] != 0).all(-1), (jp[0] != 0).all(-1))))
    if find_match:
        rel, col, status = matched_rel_err(t3, r3, tp, rp, tq, rq)
    else:
        with np.errstate(all="ignore"):
            rel = np.stack(((r3 - t3) / t3, (rp - tp) / tp, (rq - tq) / tq))
        col = np.broadcast_to(np.arange(N), (2, B, N)).copy()
        status = np.zeros(B, dtype=np.int32)
    out.update(rel_err=rel, col4row=col, status=status, is_padded=np.isinf(rel[0]).any(-1))
    return out


def assert_same(got, want, rtol, what, floor=None):
    """allclose with identical NaN / +-inf positions.  floor: an absolute term per entry (broadcast against want) for the named
    cases whose restatement misses rtol against itself (a measured tolerance); None: rtol alone."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, what
    assert np.array_equal(np.isnan(got), np.isnan(want)), f"{what}: NaN positions"
    assert np.array_equal(np.isinf(got), np.isinf(want)) and np.array_equal(got[np.isinf(got)], want[np.isinf(want)]), f"{what}: inf positions"
    f = np.isfinite(want)
    if floor is None:
        np.testing.assert_allclose(got[f], want[f], rtol=rtol, atol=0, err_msg=what)
        return
    err, allowed = np.abs(got[f] - want[f]), rtol * np.abs(want[f]) + np.broadcast_to(np.asarray(floor, dtype=np.float64), want.shape)[f]
    bad = ~(err <= allowed)
    assert not bad.any(), f"{what}: {int(bad.sum())} entries, worst |got - want| {err[bad].max():.3e} where {allowed[bad][err[bad].argmax()]:.3e} is allowed"


def assert_mass(got_m, p, what):
    """Jet masses through m^2, within the cancellation bound of an N-term sum: 4 N 2^-52 (E^2 + |p|^2)."""
    msq, scale = jet_msq(p)
    np.testing.assert_array_less(np.abs(np.sign(got_m) * got_m * got_m - msq), 4 * p.shape[-2] * 2.0 ** -52 * scale + 1e-300, err_msg=what)


def assert_tied_assignment(tq, rq, col, want_col, rel, what="", floor=None):
    """The rule for a padded jet's relative-polar assignment, whose exactly tied costs a last-bit difference in asinh / atan2 can
    order differently: col is a permutation, its total cost on the given frames (N, 3) is within 1e-12 relative of scipy's optimum
    want_col, and rel (N, 3) is the relative error of THAT assignment at rtol 1e-11 (plus `floor`, a measured absolute term, if given)."""
    n = len(want_col)
    assert sorted(int(c) for c in col) == list(range(n)), (what, col)
    c = cost3(tq, rq)
    tot, best = c[np.arange(n), col].sum(), c[np.arange(n), want_col].sum()
    assert abs(tot - best) <= 1e-12 * abs(best), (what, tot, best)
    with np.errstate(all="ignore"):
        mine = (rq[col] - tq) / (tq + EPS)
    assert np.array_equal(np.isfinite(rel), np.isfinite(mine)), what
    f = np.isfinite(mine)
    if floor is None:
        np.testing.assert_allclose(rel[f], mine[f], rtol=1e-11, atol=0, err_msg=what)
    else:                                          # (a measured absolute term of this jet: see assert_same)
        assert (np.abs(rel[f] - mine[f]) <= 1e-11 * np.abs(mine[f]) + floor).all(), what


def bin_index(v, edges):
    """The bin of every value under np.histogram's rule for explicit edges, -1 for none: edges[i] <= v < edges[i + 1], the last bin
    also v == edges[-1]; decided by comparing with the edges themselves (the count of edges <= v)."""
    v, edges = np.asarray(v, dtype=np.float64), np.asarray(edges, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        i = (edges[None, :] <= v.reshape(-1, 1)).sum(-1) - 1
        nb = len(edges) - 1
        return np.where(i == nb, np.where(v.reshape(-1) == edges[-1], nb - 1, -1), i)


def histogram(x, edges, keep=None, weights=None):
    """Counts of column c of x (rows, cols) over edges[c], by bin_index: a list of arrays (int64, or float64 with weights)."""
    out = []
    for c, e in enumerate(edges):
        v = x[:, c] if keep is None else x[keep, c]
        w = None if weights is None else (weights if keep is None else weights[keep])
        b = bin_index(v, e)
        ok = b >= 0
        out.append(np.bincount(b[ok], weights=None if w is None else w[ok], minlength=len(e) - 1))
    return out
