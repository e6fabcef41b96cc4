"""numpy / scipy restatement of the EMD under energyflow's options and of the matrix of EMDs, as include/lgn_amd.h defines them
(csrc/emd_pairs.hip computes them), on top of the balanced LP of tests/_emd_ref.py (linprog, HiGHS, tolerances 1e-10):

    dphi   = phi_i - phi'_j;  periodic_phi: dphi = pi - |pi - |phi_i - phi'_j||
    theta  = sqrt(dy^2 + dphi^2) / R
    cost   = theta^beta between particles, 1 to or from the fictitious particle (the term |sum pT - sum pT'| is not raised to beta)
    norm   each event's weights over that event's sum; no fictitious weight

and the project's optimality certificate for a flow and potentials returned under these options.  Not a test module."""
import numpy as np

import _emd_ref as E


def thetas(ev0, ev1, R=1.0, beta=1.0, periodic_phi=False):
    """The option cost matrix [n][m] between the particles of two events."""
    dy = ev0[:, None, 1] - ev1[None, :, 1]
    dp = ev0[:, None, 2] - ev1[None, :, 2]
    if periodic_phi:
        dp = np.pi - np.abs(np.pi - np.abs(dp))
    t = np.sqrt(dy * dy + dp * dp)
    if R != 1.0:
        t = t / R
    return t if beta == 1.0 else (t * t if beta == 2.0 else np.power(t, beta))


def weights(ev, norm=False):
    w = np.asarray(ev, dtype=np.float64)[:, 0]
    return w / w.sum() if norm else w


def balanced(ev0, ev1, R=1.0, beta=1.0, norm=False, periodic_phi=False):
    """(cost [n + 1][m + 1], supplies [n + 1], demands [m + 1]) as tests/_emd_ref.py's balanced(), under the options."""
    ev0, ev1 = np.asarray(ev0, dtype=np.float64), np.asarray(ev1, dtype=np.float64)
    n, m = len(ev0), len(ev1)
    c = np.ones((n + 1, m + 1))
    c[:n, :m] = thetas(ev0, ev1, R, beta, periodic_phi)
    c[n, m] = 0.0
    a, b = weights(ev0, norm), weights(ev1, norm)
    s0, s1 = a.sum(), b.sum()
    fict = (0.0, 0.0) if norm else (max(s1 - s0, 0.0), max(s0 - s1, 0.0))
    return c, np.append(a, fict[0]), np.append(b, fict[1])


def emd(ev0, ev1, R=1.0, beta=1.0, norm=False, periodic_phi=False):
    """EMD of two events [n][3], [m][3] under the options.  NaN where the native code reports LGN_EMD_EMPTY: both events weightless,
    or with norm either one."""
    from scipy.optimize import linprog
    ev0, ev1 = np.asarray(ev0, dtype=np.float64), np.asarray(ev1, dtype=np.float64)
    s0, s1 = ev0[:, 0].sum(), ev1[:, 0].sum()
    if (norm and not (s0 > 0 and s1 > 0)) or not (s0 > 0 or s1 > 0):
        return np.nan
    c, a, b = balanced(ev0, ev1, R, beta, norm, periodic_phi)
    if not (np.isfinite(c).all() and np.isfinite(a).all() and np.isfinite(b).all()) or (a < 0).any() or (b < 0).any():
        raise ValueError("emd: NaN, infinity or a negative weight")
    scale = max(a.sum(), b.sum())
    ri, ci = np.flatnonzero(a > 0), np.flatnonzero(b > 0)
    nr, nc = len(ri), len(ci)
    cc = c[np.ix_(ri, ci)]
    A_eq = np.zeros((nr + nc, nr * nc))
    for r in range(nr):
        A_eq[r, r * nc:(r + 1) * nc] = 1.0
    for k in range(nc):
        A_eq[nr + k, k::nc] = 1.0
    b_eq = np.concatenate([a[ri], b[ci]]) / scale
    res = linprog(cc.ravel(), A_eq=A_eq, b_eq=b_eq, bounds=(0, None), method="highs",
                  options={"primal_feasibility_tolerance": 1e-10, "dual_feasibility_tolerance": 1e-10})
    if res.status != 0:
        raise RuntimeError(f"emd: linprog failed: {res.message}")
    return float((res.x.reshape(nr, nc) * scale * cc).sum())


def emds(X0, X1=None, **opts):
    """The matrix [B0][B1] of emd(X0[i], X1[j]); X1=None: X0 against itself, i < j solved and mirrored, a zero diagonal."""
    if X1 is None:
        B = len(X0)
        out = np.zeros((B, B))
        for i in range(B):
            for j in range(i + 1, B):
                out[i, j] = out[j, i] = emd(X0[i], X0[j], **opts)
        return out
    return np.array([[emd(x, y, **opts) for y in X1] for x in X0])


def certify(val, flow, d0, d1, ev0, ev1, **opts):
    """One pair: the flow is feasible (1e-12 of the total weight), the potentials are feasible (1e-12 absolute; costs are O(1)), and
    the two objectives and the returned value agree (1e-12 relative): together that IS optimality (LP duality), under the option cost
    matrix and weights of balanced()."""
    c, a, w = balanced(ev0, ev1, **opts)
    total = max(a.sum(), w.sum())
    assert flow.shape == c.shape and (flow >= 0).all()
    assert np.abs(flow.sum(1) - a).max() <= 1e-12 * total and np.abs(flow.sum(0) - w).max() <= 1e-12 * total
    assert (d0[:, None] + d1[None, :] <= c + 1e-12).all(), (d0[:, None] + d1[None, :] - c).max()
    primal, dual = (flow * c).sum(), (d0 * a).sum() + (d1 * w).sum()
    assert abs(primal - dual) <= 1e-12 * abs(primal), (primal, dual)
    assert abs(val - primal) <= 1e-12 * abs(primal), (val, primal)


def upper_pairs(B):
    """[(i, j)] in the order of LGN_EMD_PAIRS_UPPER: i < j, row-major over the upper triangle."""
    return [(i, j) for i in range(B) for j in range(i + 1, B)]
