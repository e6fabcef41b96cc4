"""numpy / scipy restatement of the gradient of the energy mover's distance that the native GRAD kernels compute (csrc/emd.hip;
include/lgn_amd.h states the formulas), on top of the LP of tests/_emd_ref.py: by LP sensitivity the optimal flow weighs
d theta_ij / d position and the equality marginals are d EMD / d weight.  With S0 = sum pT, S1 = sum pT', u the row and v the column
marginals of the balanced problem, row n and column m the fictitious particles:

    dE/dy_i   =  sum_j f_ij (y_i - y'_j) / (R^2 theta_ij)      dE/dy'_j  = -sum_i (the same term)        (phi alike; 0 where theta = 0)
    dE/dpT_i  =  u_i - [S1 > S0] u_n + [S0 > S1] v_m           dE/dpT'_j =  v_j - [S0 > S1] v_m + [S1 > S0] u_n

The flow and the marginals come from scipy.optimize.linprog (HiGHS), solved here once more because _emd_ref.emd does not return the
marginals.  The chain from the relative-polar frame back to the Cartesian jets is CPU torch autograd on the frame's own formulas (the
wrap has derivative 1; a particle with pT == 0 is masked out of the direct path -- the 0/0 of the root and of atan2 reads as 0 -- and
still receives the term through the jet sum).  tests/test_host_emd_grad.py pins all of it to central differences of _emd_ref.emd and
_emd_ref.emd_relative.  Not a test module."""
import numpy as np

import _emd_ref as E

EPS = 1e-16


def events(rng, B, n, spread=0.4):
    """[B][n][3] events of (pT, y, phi) with random positive weights: the recipe of tests/test_gpu_emd.py"""
    return np.stack([rng.random((B, n)) + 0.05, rng.normal(size=(B, n)) * spread, rng.normal(size=(B, n)) * spread], axis=-1)


def jets(rng, B, N, padded=0):
    """(recons, target) [B][N][4] Cartesian jets: pt in [1, 51], eta and phi spread 0.3, the reconstruction perturbed by 10 %, the last
    `padded` rows of both exact zeros."""
    pt, eta, phi = 1.0 + 50.0 * rng.random((B, N)), 0.3 * rng.normal(size=(B, N)), 0.3 * rng.normal(size=(B, N))
    target = np.stack([pt * np.cosh(eta), pt * np.cos(phi), pt * np.sin(phi), pt * np.sinh(eta)], axis=-1)
    recons = target * (1.0 + 0.1 * rng.normal(size=target.shape))
    if padded:
        target[:, N - padded:] = 0.0
        recons[:, N - padded:] = 0.0
    return recons, target


def solve(ev0, ev1, R=1.0):
    """(value, flow [n + 1][m + 1], u [n + 1], v [m + 1]) of the balanced LP.  Particles without weight are left out of the LP as in
    _emd_ref.emd; their marginal is the largest feasible one (it multiplies no weight, and no test reads it)."""
    from scipy.optimize import linprog
    c, a, b = E.balanced(ev0, ev1, R)
    scale = max(a.sum(), b.sum())
    if not scale > 0:
        raise ValueError("both events are weightless")
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
    flow = np.zeros_like(c)
    flow[np.ix_(ri, ci)] = res.x.reshape(nr, nc) * scale
    # the objective and the right-hand side are both in units of `scale`: the marginals are d EMD / d weight as they stand
    mar = np.asarray(res.eqlin.marginals, dtype=np.float64)
    u, v = np.full(len(a), np.nan), np.full(len(b), np.nan)
    u[ri], v[ci] = mar[:nr], mar[nr:]
    for j in np.flatnonzero(np.isnan(v)):
        v[j] = (c[ri, j] - u[ri]).min()
    for i in np.flatnonzero(np.isnan(u)):
        u[i] = (c[i, :] - v).min()
    return float((flow * c).sum()), flow, u, v


def formula(ev0, ev1, flow, u, v, R=1.0):
    """(g0 [n][3], g1 [m][3]) in the events' column order (pT, y, phi) from a flow [n + 1][m + 1] and potentials [n + 1], [m + 1]:
    the formulas of the header, evaluated as they are written."""
    ev0, ev1 = np.asarray(ev0, dtype=np.float64), np.asarray(ev1, dtype=np.float64)
    n, m = len(ev0), len(ev1)
    dy = ev0[:, None, 1] - ev1[None, :, 1]
    dp = ev0[:, None, 2] - ev1[None, :, 2]
    theta = np.sqrt(dy * dy + dp * dp) / R
    f = flow[:n, :m]
    with np.errstate(divide="ignore", invalid="ignore"):
        k = np.where(theta > 0, f / (R * R * theta), 0.0)
    S0, S1 = ev0[:, 0].sum(), ev1[:, 0].sum()
    g0, g1 = np.zeros((n, 3)), np.zeros((m, 3))
    g0[:, 1], g0[:, 2] = (k * dy).sum(1), (k * dp).sum(1)
    g1[:, 1], g1[:, 2] = -(k * dy).sum(0), -(k * dp).sum(0)
    g0[:, 0] = u[:n] - (u[n] if S1 > S0 else 0.0) + (v[m] if S0 > S1 else 0.0)
    g1[:, 0] = v[:m] - (v[m] if S0 > S1 else 0.0) + (u[n] if S1 > S0 else 0.0)
    return g0, g1


def emd_grad(ev0, ev1, R=1.0):
    """(value, g0 [n][3], g1 [m][3]) of two events [n][3], [m][3] of (pT, y, phi)"""
    value, flow, u, v = solve(ev0, ev1, R)
    return (value,) + formula(ev0, ev1, flow, u, v, R)


def _frame_backward(jets_, g_frame):
    """d (sum of g_frame * frame(jets)) / d jets for [N][4] jets and [N][3] frame gradients (w, y, phi): torch autograd on the CPU"""
    import torch
    p = torch.tensor(np.asarray(jets_, dtype=np.float64), requires_grad=True)
    g = torch.tensor(np.asarray(g_frame, dtype=np.float64))
    px, py, pz = p[:, 1], p[:, 2], p[:, 3]
    real = (px * px + py * py) > 0
    one = torch.ones_like(px)
    sx, sy = torch.where(real, px, one), torch.where(real, py, one)      # a stand-in where pT == 0: no gradient reaches px, py there
    pT = torch.sqrt(sx * sx + sy * sy)
    eta = torch.asinh(pz / (pT + EPS))
    phi = torch.atan2(sy + EPS, sx + EPS)
    J = p.sum(0)
    jpT = torch.sqrt(J[1] * J[1] + J[2] * J[2])
    jeta = torch.asinh(J[3] / (jpT + EPS))
    jphi = torch.atan2(J[2] + EPS, J[1] + EPS)
    zero = torch.zeros_like(px)
    w = torch.where(real, pT, zero) / (jpT + EPS)
    y = eta - jeta
    ph = phi - jphi                                                       # (the wrap adds a constant: derivative 1)
    obj = (g[:, 0] * w).sum() + torch.where(real, g[:, 1] * y + g[:, 2] * ph, zero).sum()
    obj.backward()
    return p.grad.numpy()


def emd_relative_grad(recons, target):
    """(values [B], g_recons [B][N][4], g_target [B][N][4]) of [B][N][4] Cartesian jets: the gradient of _emd_ref.emd_relative"""
    recons, target = np.asarray(recons, dtype=np.float64), np.asarray(target, dtype=np.float64)
    p, q = E.relative_events(recons), E.relative_events(target)
    val, gr, gt = np.zeros(len(p)), np.zeros_like(recons), np.zeros_like(target)
    for b in range(len(p)):
        val[b], g0, g1 = emd_grad(p[b], q[b])
        # a weightless particle's weight gradient multiplies d pT / d p = 0/0, read as 0: it never reaches the jets
        gr[b], gt[b] = _frame_backward(recons[b], g0), _frame_backward(target[b], g1)
    return val, gr, gt


def fd_events(ev0, ev1, R=1.0, h=1e-6):
    """central differences of _emd_ref.emd in every coordinate of both events: (g0 [n][3], g1 [m][3])"""
    out = []
    for side in (0, 1):
        base = [np.array(ev0, dtype=np.float64), np.array(ev1, dtype=np.float64)]
        g = np.zeros_like(base[side])
        for idx in np.ndindex(*g.shape):
            x = base[side][idx]
            base[side][idx] = x + h
            up = E.emd(base[0], base[1], R)
            base[side][idx] = x - h
            dn = E.emd(base[0], base[1], R)
            base[side][idx] = x
            g[idx] = (up - dn) / (2 * h)
        out.append(g)
    return out


def fd_relative(recons, target, h=1e-5):
    """central differences of _emd_ref.emd_relative of ONE jet pair [N][4] in the momentum columns of every particle with pT > 0
    (at pT == 0 the distance has a kink in px, py: |h| enters as the weight): (g_recons, g_target, mask [2][N] of the rows taken)"""
    base = [np.array(recons, dtype=np.float64), np.array(target, dtype=np.float64)]
    out, masks = [], []
    for side in (0, 1):
        g = np.zeros_like(base[side])
        real = (base[side][:, 1] ** 2 + base[side][:, 2] ** 2) > 0
        for i in np.flatnonzero(real):
            for c in (0, 1, 2, 3):
                x = base[side][i, c]
                base[side][i, c] = x + h
                up = E.emd_relative(base[0][None], base[1][None])[0]
                base[side][i, c] = x - h
                dn = E.emd_relative(base[0][None], base[1][None])[0]
                base[side][i, c] = x
                g[i, c] = (up - dn) / (2 * h)
        out.append(g)
        masks.append(real)
    return out[0], out[1], np.stack(masks)


# ---- the cases of the g26 fixture (tests/golden/gen_golden_g26.py writes them, the host and GPU tests read them) ----------------------
GENERIC = (("5x8", 5, 8, 1.0), ("8x5", 8, 5, 1.0), ("6x6_R0.4", 6, 6, 0.4), ("1x7", 1, 7, 1.0), ("12x12", 12, 12, 1.0),
           ("7x7_balanced", 7, 7, 1.0))                  # (tag, n, m, R); the last: sum pT' = sum pT + 1e-3
REL = (("n5", 5, 0), ("n12", 12, 3), ("n30", 30, 0))     # (tag, N, zero-padded rows of both jets)
GENERIC_PAIRS, REL_JETS = 3, 2


def generic_case(tag):
    """(ev0 [B][n][3], ev1 [B][m][3], R) of a GENERIC tag"""
    k, (_, n, m, R) = next((k, c) for k, c in enumerate(GENERIC) if c[0] == tag)
    rng = np.random.default_rng(26000 + k)
    a, b = events(rng, GENERIC_PAIRS, n), events(rng, GENERIC_PAIRS, m)
    if tag.endswith("balanced"):
        b[..., 0] *= ((a[..., 0].sum(-1) + 1e-3) / b[..., 0].sum(-1))[:, None]
    return a, b, R


def rel_case(tag):
    """(recons, target) [B][N][4] of a REL tag"""
    k, (_, N, padded) = next((k, c) for k, c in enumerate(REL) if c[0] == tag)
    return jets(np.random.default_rng(26100 + k), REL_JETS, N, padded)
