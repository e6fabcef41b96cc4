"""numpy / scipy restatement of the gradient of the energy mover's distance under energyflow's options (csrc/emd_grad_opts.hip computes
it; include/lgn_amd.h states the formulas), on top of the option LP of tests/_emd_pairs_ref.py.  With dy = y_i - y'_j,
D = phi_i - phi'_j, dphi = D (periodic_phi: pi - |pi - |D||), theta = sqrt(dy^2 + dphi^2) / R, f the optimal flow in the units of the
LP's weights (normalised under norm), u and v the equality marginals, S0 = sum pT, S1 = sum pT', row n and column m fictitious:

    s_ij      = 1 without periodic_phi;  sign(D) sign(pi - |D|) with it
    k_ij      = f_ij beta theta_ij^(beta - 2) / R^2   where theta_ij > 0, else 0
    dE/dy_i   =  sum_j k_ij dy             dE/dy'_j   = -sum_i k_ij dy
    dE/dphi_i =  sum_j k_ij dphi s_ij      dE/dphi'_j = -sum_i k_ij dphi s_ij
    norm off:  dE/dpT_i = u_i - [S1 > S0] u_n + [S0 > S1] v_m           (dE/dpT'_j alike)
    norm on :  dE/dpT_i = (u_i - sum_k a_k u_k) / S0,  a = pT / S0       dE/dpT'_j = (v_j - sum_k b_k v_k) / S1,  b = pT' / S1

tests/test_host_emd_opts_grad.py pins the restatement to central differences of _emd_pairs_ref.emd.  Not a test module."""
import numpy as np

import _emd_grad_ref as G
import _emd_pairs_ref as P

OPTIONS = {                    # the named option sets of the tests and of the g27 fixture (R comes on top where a case has one)
    "beta2": dict(beta=2.0),
    "beta05": dict(beta=0.5),
    "beta15": dict(beta=1.5),
    "periodic": dict(periodic_phi=True),
    "norm": dict(norm=True),
    "all": dict(R=0.8, beta=2.0, norm=True, periodic_phi=True),
}


def solve(ev0, ev1, R=1.0, beta=1.0, norm=False, periodic_phi=False):
    """(value, flow [n + 1][m + 1], u [n + 1], v [m + 1]) of the balanced LP of _emd_pairs_ref.balanced: _emd_grad_ref.solve under the
    options.  Particles without weight are left out of the LP; their marginal is the largest feasible one."""
    from scipy.optimize import linprog
    c, a, b = P.balanced(ev0, ev1, R, beta, norm, periodic_phi)
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
    mar = np.asarray(res.eqlin.marginals, dtype=np.float64)
    u, v = np.full(len(a), np.nan), np.full(len(b), np.nan)
    u[ri], v[ci] = mar[:nr], mar[nr:]
    for j in np.flatnonzero(np.isnan(v)):
        v[j] = (c[ri, j] - u[ri]).min()
    for i in np.flatnonzero(np.isnan(u)):
        u[i] = (c[i, :] - v).min()
    return float((flow * c).sum()), flow, u, v


def formula(ev0, ev1, flow, u, v, R=1.0, beta=1.0, norm=False, periodic_phi=False):
    """(g0 [n][3], g1 [m][3]) in the events' column order (pT, y, phi) from a flow [n + 1][m + 1] and potentials [n + 1], [m + 1]:
    the formulas of the header, evaluated as they are written."""
    ev0, ev1 = np.asarray(ev0, dtype=np.float64), np.asarray(ev1, dtype=np.float64)
    n, m = len(ev0), len(ev1)
    dy = ev0[:, None, 1] - ev1[None, :, 1]
    D = ev0[:, None, 2] - ev1[None, :, 2]
    dp, s = D, np.ones_like(D)
    if periodic_phi:
        dp = np.pi - np.abs(np.pi - np.abs(D))
        s = np.sign(D) * np.sign(np.pi - np.abs(D))
    theta = np.sqrt(dy * dy + dp * dp) / R
    f = flow[:n, :m]
    with np.errstate(divide="ignore", invalid="ignore"):
        k = np.where(theta > 0, f * beta * np.power(theta, beta - 2.0) / (R * R), 0.0)
    g0, g1 = np.zeros((n, 3)), np.zeros((m, 3))
    g0[:, 1], g0[:, 2] = (k * dy).sum(1), (k * dp * s).sum(1)
    g1[:, 1], g1[:, 2] = -(k * dy).sum(0), -(k * dp * s).sum(0)
    S0, S1 = ev0[:, 0].sum(), ev1[:, 0].sum()
    if norm:
        a, b = ev0[:, 0] / S0, ev1[:, 0] / S1
        g0[:, 0] = (u[:n] - (a * u[:n]).sum()) / S0
        g1[:, 0] = (v[:m] - (b * v[:m]).sum()) / S1
    else:
        g0[:, 0] = u[:n] - (u[n] if S1 > S0 else 0.0) + (v[m] if S0 > S1 else 0.0)
        g1[:, 0] = v[:m] - (v[m] if S0 > S1 else 0.0) + (u[n] if S1 > S0 else 0.0)
    return g0, g1


def emd_grad(ev0, ev1, **opts):
    """(value, g0 [n][3], g1 [m][3]) of two events [n][3], [m][3] of (pT, y, phi) under the options"""
    value, flow, u, v = solve(ev0, ev1, **opts)
    return (value,) + formula(ev0, ev1, flow, u, v, **opts)


def emd_relative_grad(recons, target, **opts):
    """(values [B], g_recons [B][N][4], g_target [B][N][4]) of [B][N][4] Cartesian jets: the options on the relative-polar frames,
    carried back by _emd_grad_ref._frame_backward"""
    import _emd_ref as E
    recons, target = np.asarray(recons, dtype=np.float64), np.asarray(target, dtype=np.float64)
    p, q = E.relative_events(recons), E.relative_events(target)
    val, gr, gt = np.zeros(len(p)), np.zeros_like(recons), np.zeros_like(target)
    for b in range(len(p)):
        val[b], g0, g1 = emd_grad(p[b], q[b], **opts)
        gr[b], gt[b] = G._frame_backward(recons[b], g0), G._frame_backward(target[b], g1)
    return val, gr, gt


def fd_events(ev0, ev1, h=1e-6, **opts):
    """central differences of _emd_pairs_ref.emd in every coordinate of both events: (g0 [n][3], g1 [m][3])"""
    out = []
    for side in (0, 1):
        base = [np.array(ev0, dtype=np.float64), np.array(ev1, dtype=np.float64)]
        g = np.zeros_like(base[side])
        for idx in np.ndindex(*g.shape):
            x = base[side][idx]
            base[side][idx] = x + h
            up = P.emd(base[0], base[1], **opts)
            base[side][idx] = x - h
            dn = P.emd(base[0], base[1], **opts)
            base[side][idx] = x
            g[idx] = (up - dn) / (2 * h)
        out.append(g)
    return out


def fd_relative(recons, target, h=1e-5, **opts):
    """central differences of the option EMD of ONE jet pair [N][4] on its relative-polar frames, in the momentum columns of every
    particle with pT > 0 (as _emd_grad_ref.fd_relative): (g_recons, g_target, mask [2][N] of the rows taken)"""
    import _emd_ref as E

    def value(r, t):
        return P.emd(E.relative_events(r[None])[0], E.relative_events(t[None])[0], **opts)
    base = [np.array(recons, dtype=np.float64), np.array(target, dtype=np.float64)]
    out, masks = [], []
    for side in (0, 1):
        g = np.zeros_like(base[side])
        real = (base[side][:, 1] ** 2 + base[side][:, 2] ** 2) > 0
        for i in np.flatnonzero(real):
            for c in (0, 1, 2, 3):
                x = base[side][i, c]
                base[side][i, c] = x + h
                up = value(base[0], base[1])
                base[side][i, c] = x - h
                dn = value(base[0], base[1])
                base[side][i, c] = x
                g[i, c] = (up - dn) / (2 * h)
        out.append(g)
        masks.append(real)
    return out[0], out[1], np.stack(masks)


def events(rng, B, n, periodic=False, spread=0.4):
    """_emd_grad_ref.events; periodic: phi uniform in [0, 2 pi)"""
    ev = G.events(rng, B, n, spread)
    if periodic:
        ev[..., 2] = rng.random((B, n)) * 2.0 * np.pi
    return ev


# ---- the cases of the g27 fixture (tests/golden/gen_golden_g27.py writes them, the GPU tests read them) --------------------------------
# generic: (tag of _emd_grad_ref.GENERIC, option name); the case's own R applies unless the option set brings one ("all": 0.8)
GENERIC = tuple((c[0], o) for o in ("beta2", "beta05", "norm", "all") for c in G.GENERIC) + \
    tuple((t, o) for o in ("beta15", "periodic") for t in ("5x8", "12x12"))
REL = tuple((c[0], o) for o in ("beta2", "norm", "all") for c in G.REL)


def case_options(tag, opt):
    """the keyword options of a generic case"""
    R = next(c[3] for c in G.GENERIC if c[0] == tag)
    return {"R": R, **OPTIONS[opt]}


def generic_case(tag, opt):
    """(ev0 [B][n][3], ev1 [B][m][3], options) of a GENERIC case: the events of _emd_grad_ref.generic_case, phi redrawn uniform in
    [0, 2 pi) under periodic_phi"""
    a, b, _ = G.generic_case(tag)
    o = case_options(tag, opt)
    if o.get("periodic_phi"):
        rng = np.random.default_rng(27000 + [c[0] for c in G.GENERIC].index(tag))
        a[..., 2], b[..., 2] = rng.random(a.shape[:2]) * 2.0 * np.pi, rng.random(b.shape[:2]) * 2.0 * np.pi
    return a, b, o
