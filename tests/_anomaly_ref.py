"""numpy restatement of the reference's anomaly_scores() (utils/jet_analysis/anomaly_detection.py, include_emd=False, unbatched)
and of scipy.optimize.linear_sum_assignment's shortest-augmenting-path solver, with no scipy dependency: the tests check the native
kernels against it on machines where scipy is absent.  Not a test module."""
import numpy as np

EPS = 1e-16

SCORE_KEYS = (
    "particle, Cartesian, Chamfer distance",
    "particle, polar, Chamfer distance",
    "particle, normalized Cartesian, Chamfer distance",
    "particle, normalized polar, Chamfer distance",
    "particle, relative polar, Chamfer distance",
    "particle, Cartesian, Hungarian distance",
    "particle, polar, Hungarian distance",
    "particle, normalized Cartesian, Hungarian distance",
    "particle, normalized polar, Hungarian distance",
    "particle, relative polar, Hungarian distance",
    "particle, Cartesian, MSE",
    "particle, polar, MSE",
    "particle, normalized Cartesian, MSE",
    "particle, normalized polar, MSE",
    "particle, relative polar, MSE",
    "jet, Cartesian",
    "jet, polar",
    "particle, Lorentz norms, Chamfer distance",
    "particle, Lorentz norms, Hungarian distance",
    "particle, Lorentz norms, MSE",
    "jet, Lorentz norms",
)
HUNGARIAN_INDEX = (5, 6, 7, 8, 9, 18)       # score slots of the six assignment variants, in the order of col4row


def lsap(cost):
    """col_ind of scipy.optimize.linear_sum_assignment(cost) for a square cost, ties included (Crouse's shortest augmenting path
    as scipy implements it).  Each Dijkstra step is vectorised over the `remaining` list, in its order; the selection
    "first strict minimum, then any later tie with a free column" of the sequential scan is: the last free column at the minimum
    if there is one, else the first column at the minimum."""
    cost = np.asarray(cost, dtype=np.float64)
    n = cost.shape[0]
    if not np.all(np.isfinite(cost) | (cost == np.inf)):
        raise ValueError("matrix contains invalid numeric entries")
    u, v = np.zeros(n), np.zeros(n)
    col4row, row4col, path = np.full(n, -1), np.full(n, -1), np.full(n, -1)
    for cur in range(n):
        remaining = list(range(n - 1, -1, -1))
        spc = np.full(n, np.inf)
        sc, sr = np.zeros(n, bool), np.zeros(n, bool)
        min_val, i, sink = 0.0, cur, -1
        while sink == -1:
            sr[i] = True
            rem = np.array(remaining)
            r = ((min_val + cost[i, rem]) - u[i]) - v[rem]
            better = r < spc[rem]
            path[rem[better]] = i
            spc[rem[better]] = r[better]
            s = spc[rem]
            lowest = s.min()
            if lowest == np.inf:
                raise ValueError("cost matrix is infeasible")
            at_min = np.flatnonzero(s == lowest)
            free = at_min[row4col[rem[at_min]] == -1]
            index = free[-1] if len(free) else at_min[0]
            min_val = lowest
            j = remaining[index]
            if row4col[j] == -1:
                sink = j
            else:
                i = row4col[j]
            sc[j] = True
            remaining[index] = remaining[-1]
            remaining.pop()
        u[cur] += min_val
        for i in np.flatnonzero(sr):
            if i != cur:
                u[i] += min_val - spc[col4row[i]]
        v[sc] -= min_val - spc[sc]
        j = sink
        while True:
            i = path[j]
            row4col[j] = i
            col4row[i], j = j, col4row[i]
            if i == cur:
                break
    return col4row


def p4_polar(x):
    """(E, px, py, pz) -> (E, pT, eta, phi) as get_p4_polar."""
    E, px, py, pz = np.moveaxis(x, -1, 0)
    pT = np.sqrt(px * px + py * py)
    return np.stack((E, pT, np.arcsinh(pz / (pT + EPS)), np.arctan2(py + EPS, px + EPS)), axis=-1)


def polar_rel(xp, jp):
    """get_polar_rel: (pT / (jet pT + eps), eta - jet eta, remainder(phi - jet phi + pi, 2 pi) - pi), padded with a zero 4th column."""
    pt = xp[..., 1] / (jp[..., None, 1] + EPS)
    eta = xp[..., 2] - jp[..., None, 2]
    phi = np.remainder((xp[..., 3] - jp[..., None, 3]) + np.pi, 2 * np.pi) - np.pi
    return np.stack((pt, eta, phi, np.zeros_like(pt)), axis=-1)


def mink(d):
    return ((d[..., 0] * d[..., 0] - d[..., 1] * d[..., 1]) - d[..., 2] * d[..., 2]) - d[..., 3] * d[..., 3]


def euclid(d):
    return np.sqrt(((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]) + d[..., 3] * d[..., 3])


def frames(recons, target, recons_n, target_n):
    """The six (p, q, lorentz) pairs of the score variants: Cartesian, polar, normalized Cartesian, normalized polar, relative polar,
    Lorentz (Cartesian with the Minkowski square)."""
    rp, tp = p4_polar(recons), p4_polar(target)
    rj, tj = recons.sum(-2), target.sum(-2)
    return [(recons, target, False), (rp, tp, False), (recons_n, target_n, False), (p4_polar(recons_n), p4_polar(target_n), False),
            (polar_rel(rp, p4_polar(rj)), polar_rel(tp, p4_polar(tj)), False), (recons, target, True)]


def costs(p, q, lorentz):
    d = p[..., :, None, :] - q[..., None, :, :]
    return mink(d) if lorentz else euclid(d)


def anomaly_scores(recons, target, recons_n, target_n, hungarian=True):
    """(scores [B][21] in SCORE_KEYS order, col4row [6][B][N]) of float64 arrays [B][N][4]."""
    recons, target, recons_n, target_n = (np.asarray(a, dtype=np.float64) for a in (recons, target, recons_n, target_n))
    B, N, _ = recons.shape
    out = np.full((B, 21), np.nan)
    col = np.full((6, B, N), -1, dtype=np.int64)
    for f, (p, q, lor) in enumerate(frames(recons, target, recons_n, target_n)):
        c = costs(p, q, lor)
        cham = (c.min(-1) + c.min(-2)).mean(-1)
        d = p - q
        mse = (mink(d) if lor else (d * d).sum(-1)).mean(-1)
        out[:, 17 if lor else f] = cham
        out[:, 19 if lor else 10 + f] = mse
        if hungarian:
            pe = recons if lor else p          # the Lorentz variant scores the Euclidean Cartesian MSE of its pairing
            qe = target if lor else q
            for b in range(B):
                col[f, b] = lsap(c[b])
                dd = pe[b, col[f, b]] - qe[b]   # the reference pairs p[col_ind[r]] with q[r]
                out[b, HUNGARIAN_INDEX[f]] = (dd * dd).sum(-1).mean()
    dj = recons.sum(-2) - target.sum(-2)
    out[:, 15] = (dj * dj).sum(-1)
    out[:, 16] = out[:, 15]
    out[:, 20] = mink(dj)
    return out, col
