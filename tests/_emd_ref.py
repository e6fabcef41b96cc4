"""numpy / scipy restatement of the energy mover's distance the native EMD score computes (csrc/emd.hip; include/lgn_amd.h states the
definition): energyflow.emd.emd(ev0, ev1) with its defaults R = 1, beta = 1, norm = False, Euclidean ground distance, no periodic phi,
as energyflow's documentation defines it.  energyflow itself was not available when this was written, so this file follows the
definition, not the package:

    theta_ij = sqrt((y_i - y'_j)^2 + (phi_i - phi'_j)^2) / R
    EMD      = min over f >= 0 of sum f_ij theta_ij + |sum pT - sum pT'|
               with sum_j f_ij <= pT_i, sum_i f_ij <= pT'_j, sum f_ij = min(sum pT, sum pT')

solved as the balanced transportation LP (one fictitious particle on the lighter side carries the weight difference at cost 1 to every
particle of the other event) with scipy.optimize.linprog(method="highs"), feasibility tolerances 1e-10, the weights divided by
max(sum pT, sum pT') as energyflow divides them.  Also the relative-polar staging of the reference's score (the frames of
tests/_anomaly_ref.py).  Not a test module."""
import numpy as np

import _anomaly_ref as A

KEY = "emd (relative coordinates)"


def thetas(ev0, ev1, R=1.0):
    dy = ev0[:, None, 1] - ev1[None, :, 1]
    dp = ev0[:, None, 2] - ev1[None, :, 2]
    return np.sqrt(dy * dy + dp * dp) / R


def balanced(ev0, ev1, R=1.0):
    """(cost [n + 1][m + 1], supplies [n + 1], demands [m + 1]): row n and column m are the fictitious particles, of which at most
    one has weight; their costs are 1 (0 between the two, which never carries flow)."""
    ev0, ev1 = np.asarray(ev0, dtype=np.float64), np.asarray(ev1, dtype=np.float64)
    n, m = len(ev0), len(ev1)
    c = np.ones((n + 1, m + 1))
    c[:n, :m] = thetas(ev0, ev1, R)
    c[n, m] = 0.0
    s0, s1 = ev0[:, 0].sum(), ev1[:, 0].sum()
    a = np.append(ev0[:, 0], max(s1 - s0, 0.0))
    b = np.append(ev1[:, 0], max(s0 - s1, 0.0))
    return c, a, b


def emd(ev0, ev1, R=1.0, return_flow=False):
    """EMD of two events [n][3], [m][3] of (pT, y, phi); with return_flow also the flow [n + 1][m + 1].  NaN when both events are
    weightless.  Particles without weight are left out of the LP (they can carry no flow)."""
    from scipy.optimize import linprog
    c, a, b = balanced(ev0, ev1, R)
    if not (np.isfinite(c).all() and np.isfinite(a).all() and np.isfinite(b).all()) or (a < 0).any() or (b < 0).any():
        raise ValueError("emd: NaN, infinity or a negative weight")
    scale = max(a.sum(), b.sum())
    flow = np.zeros_like(c)
    if not scale > 0:
        return (np.nan, flow) if return_flow else np.nan
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
    f = res.x.reshape(nr, nc) * scale
    flow[np.ix_(ri, ci)] = f
    value = float((f * cc).sum())
    return (value, flow) if return_flow else value


def relative_events(jets):
    """[B][N][4] Cartesian jets -> [B][N][3] events (pT / (jet pT + eps), eta - jet eta, wrapped phi - jet phi): get_polar_rel."""
    jets = np.asarray(jets, dtype=np.float64)
    return A.polar_rel(A.p4_polar(jets), A.p4_polar(jets.sum(-2)))[..., :3]


def emd_relative(recons, target):
    """The reference's 22nd score of [B][N][4] jets: one EMD per jet on the relative-polar frames."""
    p, q = relative_events(recons), relative_events(target)
    return np.array([emd(p[b], q[b]) for b in range(len(p))])
