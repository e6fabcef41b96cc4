"""numpy restatement of the entropic optimal-transport loss and the Sinkhorn divergence that csrc/sinkhorn.hip computes, written from
the section of include/lgn_amd.h that defines them -- never by calling the library.  Not a test module.

    extended problem   the EMD's (tests/_emd_pairs_ref.balanced): a [n + 1], b [m + 1], C [n + 1][m + 1]; without norm the lighter
                       event's fictitious particle carries |S0 - S1| at cost 1; S = max(sum a, sum b)
    objective          OT_eps(a, b) = min_P <P, C> + eps KL(P | a (x) b / S)
    iteration, g = 0   f_i <- -eps log sum_j (b_j / S) exp((g_j - C_ij) / eps);   g_j <- -eps log sum_i (a_i / S) exp((f_i - C_ij) / eps)
    stopping           err = sum_i a_i |1 - exp((f_i - f_new_i) / eps)| when the next f has been computed; tol > 0 and err <= tol S
                       stops without applying f_new; after max_iter iterations one more f evaluation gives err
    value              E = <a, f> + <b, g>;  plan P_ij = (a_i b_j / S) exp((f_i + g_j - C_ij) / eps)
    gradients          tests/_emd_opts_grad_ref.formula with the flow replaced by P and (u, v) by (f, g)
    debias             E(ev0, ev1) - E(ev0, ev0) / 2 - E(ev1, ev1) / 2, a self term without a fictitious particle, its position terms
                       counted as row and as column, d / d a_i = f_i + g_i

Two float64 variants of the same definition: variant 0 iterates on f / eps, g / eps and C / eps with a max-shifted log-sum-exp
whose sums run in index order (what the header writes down); variant 1 iterates on f and g themselves with
scipy.special.logsumexp(b=weights) over the REVERSED index order.  Their spread on one input is the definition's own sensitivity to
rounding order, which the GPU tests use as the unit of their tolerance."""
import numpy as np

import _emd_grad_ref as G
import _emd_opts_grad_ref as GO
import _emd_pairs_ref as P
import _emd_ref as E

INVALID, EMPTY, ITER = 1, 2, 16            # LGN_EMD_INVALID, LGN_EMD_EMPTY, LGN_SINKHORN_ITER


def _ordered_sum(x, axis):
    """the sum along axis in index order, one rounded addition per term"""
    return np.take(np.cumsum(x, axis=axis), -1, axis=axis)


def _update(logw, w, pot, C, eps, pos, variant):
    """-eps log sum_{j in pos} (w_j / S) exp((pot_j - C[:, j]) / eps) for every row of C; variant 0 returns it divided by eps and takes
    pot and C divided by eps"""
    if variant == 0:
        t = (logw[pos] + pot[pos])[None, :] - C[:, pos]
        M = t.max(axis=1)
        return -(M + np.log(_ordered_sum(np.exp(t - M[:, None]), 1)))
    from scipy.special import logsumexp
    rev = pos[::-1]
    return -eps * logsumexp((pot[rev][None, :] - C[:, rev]) / eps, b=w[rev][None, :], axis=1)


def solve(C, a, b, S, epsilon, max_iter, tol, variant=0):
    """The iterations on one extended problem.  Returns a dict: f, g, value, plan, iters, err, missed (tol > 0 and err > tol S) and
    history, the err measured after 1, 2, ... iters applied iterations (the last entry is the returned err)."""
    C, a, b = np.asarray(C, dtype=np.float64), np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    ra, cb = np.flatnonzero(a > 0), np.flatnonzero(b > 0)
    with np.errstate(divide="ignore"):
        la, lb = np.log(a / S), np.log(b / S)
    if variant == 0:
        Cx, wa, wb, unit = C / epsilon, la, lb, 1.0
    else:
        Cx, wa, wb, unit = C, la, lb, epsilon
    f, g = np.zeros(len(a)), np.zeros(len(b))
    iters, err, history = 0, 0.0, []
    while True:
        f_new = _update(wb, b / S, g, Cx, epsilon, cb, variant)
        if iters >= 1:
            d = (f - f_new) / unit
            terms = a[ra] * np.abs(1.0 - np.exp(d[ra]))
            err = float(_ordered_sum(terms, 0)) if variant == 0 else float(terms[::-1].sum())
            history.append(err)
            if iters >= max_iter or (tol > 0 and err <= tol * S):
                break
        f = f_new
        g = _update(wa, a / S, f, Cx.T, epsilon, ra, variant)
        iters += 1
    if variant == 0:
        F, Gs = f, g
        f, g = epsilon * f, epsilon * g
        value = epsilon * float((a * F).sum() + (b * Gs).sum())
        expo = (F[:, None] + Gs[None, :]) - Cx
    else:
        value = float((a * f).sum() + (b * g).sum())
        expo = (f[:, None] + g[None, :] - C) / epsilon
    w = a[:, None] * b[None, :]
    plan = np.where(w > 0, (w / S) * np.exp(expo), 0.0)
    return dict(f=f, g=g, value=value, plan=plan, iters=iters, err=err, missed=bool(tol > 0 and err > tol * S), history=history)


def _status(ev0, ev1, norm):
    x = np.concatenate([np.asarray(ev0, dtype=np.float64).ravel(), np.asarray(ev1, dtype=np.float64).ravel()])
    if not np.isfinite(x).all() or (np.asarray(ev0)[:, 0] < 0).any() or (np.asarray(ev1)[:, 0] < 0).any():
        return INVALID
    s0, s1 = np.asarray(ev0)[:, 0].sum(), np.asarray(ev1)[:, 0].sum()
    if (norm and not (s0 > 0 and s1 > 0)) or not (s0 > 0 or s1 > 0):
        return EMPTY
    return 0


def _self_term(ev, epsilon, max_iter, tol, variant, R, beta, norm, periodic_phi):
    """OT_eps of an event with itself: (solution or None for a weightless event, gradient [n][3] of the term)"""
    ev = np.asarray(ev, dtype=np.float64)
    n = len(ev)
    w = P.weights(ev, norm)
    S = w.sum()
    if not S > 0:
        return None, np.zeros((n, 3))
    C = P.thetas(ev, ev, R, beta, periodic_phi)
    s = solve(C, w, w, S, epsilon, max_iter, tol, variant)
    pad = np.zeros((n + 1, n + 1))
    pad[:n, :n] = s["plan"]
    g_row, g_col = GO.formula(ev, ev, pad, np.append(s["f"], 0.0), np.append(s["g"], 0.0), R=R, beta=beta, norm=norm,
                              periodic_phi=periodic_phi)
    return s, g_row + g_col


def sinkhorn(ev0, ev1, epsilon, max_iter=200, tol=1e-6, debias=False, R=1.0, beta=1.0, norm=False, periodic_phi=False, variant=0,
             grad=True):
    """One pair of events [n][3], [m][3] of (pT, y, phi).  Returns a dict: value, f [n + 1], g [m + 1], plan [n + 1][m + 1], iters,
    err, status, S, history (of the cross term), g0 [n][3], g1 [m][3] (grad), self_iters and self_history (debias).  A pair with
    INVALID or EMPTY is NaN throughout with iters 0."""
    ev0, ev1 = np.asarray(ev0, dtype=np.float64), np.asarray(ev1, dtype=np.float64)
    n, m = len(ev0), len(ev1)
    st = _status(ev0, ev1, norm)
    if st:
        nan = np.nan
        return dict(value=nan, f=np.full(n + 1, nan), g=np.full(m + 1, nan), plan=np.full((n + 1, m + 1), nan), iters=0, err=nan,
                    status=st, S=nan, history=[], g0=np.full((n, 3), nan), g1=np.full((m, 3), nan), self_iters=[], self_history=[])
    C, a, b = P.balanced(ev0, ev1, R, beta, norm, periodic_phi)
    S = max(a.sum(), b.sum())
    s = solve(C, a, b, S, epsilon, max_iter, tol, variant)
    out = dict(value=s["value"], f=s["f"], g=s["g"], plan=s["plan"], iters=s["iters"], err=s["err"], status=ITER if s["missed"] else 0,
               S=S, history=s["history"], self_iters=[], self_history=[])
    opts = dict(R=R, beta=beta, norm=norm, periodic_phi=periodic_phi)
    if grad:
        out["g0"], out["g1"] = GO.formula(ev0, ev1, s["plan"], s["f"], s["g"], **opts)
    if debias:
        for side, ev in ((0, ev0), (1, ev1)):
            t, gs = _self_term(ev, epsilon, max_iter, tol, variant, **opts)
            if t is None:
                continue
            out["value"] = out["value"] - 0.5 * t["value"]
            out["status"] |= ITER if t["missed"] else 0
            out["self_iters"].append(t["iters"])
            out["self_history"].append((t["history"], P.weights(ev, norm).sum()))
            if grad:
                out["g1" if side else "g0"] = out["g1" if side else "g0"] - 0.5 * gs
    return out


def sinkhorn_relative(recons, target, epsilon, **kw):
    """ONE pair of Cartesian jets [N][4] on their relative-polar frames: sinkhorn()'s dict with g_recons, g_target [N][4] in addition,
    carried back by _emd_grad_ref._frame_backward"""
    recons, target = np.asarray(recons, dtype=np.float64), np.asarray(target, dtype=np.float64)
    p, q = E.relative_events(recons[None])[0], E.relative_events(target[None])[0]
    out = sinkhorn(p, q, epsilon, **kw)
    if "g0" in out and not out["status"] & (INVALID | EMPTY):
        out["g_recons"], out["g_target"] = G._frame_backward(recons, out["g0"]), G._frame_backward(target, out["g1"])
    return out


def fd_events(ev0, ev1, epsilon, h=1e-6, **kw):
    """central differences of the value in every coordinate of both events (weights: only those that are positive): (g0, g1)"""
    out = []
    for side in (0, 1):
        base = [np.array(ev0, dtype=np.float64), np.array(ev1, dtype=np.float64)]
        g = np.full(base[side].shape, np.nan)
        for idx in np.ndindex(*g.shape):
            x = base[side][idx]
            if idx[1] == 0 and not x > 0:
                continue
            base[side][idx] = x + h
            up = sinkhorn(base[0], base[1], epsilon, grad=False, **kw)["value"]
            base[side][idx] = x - h
            dn = sinkhorn(base[0], base[1], epsilon, grad=False, **kw)["value"]
            base[side][idx] = x
            g[idx] = (up - dn) / (2 * h)
        out.append(g)
    return out


def jet_events(rng, n, real=None, scale=1.0, spread=0.4):
    """a jet-like event [n][3] of (pT, y, phi): falling pT spectrum, positions around the axis; rows from `real` on are zero padding"""
    pT = scale * rng.exponential(1.0, n) + 0.05
    ev = np.stack([pT, rng.normal(size=n) * spread, rng.normal(size=n) * spread], axis=-1)
    if real is not None:
        ev[real:] = 0.0
    return ev


def stopping_margin(history, S, tol):
    """(err at the stop / (tol S), smallest err before it / (tol S)) of a run that stopped by tol: a case is safe against a last-bit
    flip of the count when the first is below 1/4 and the second above 4"""
    if len(history) < 2:
        return history[-1] / (tol * S), np.inf
    return history[-1] / (tol * S), min(history[:-1]) / (tol * S)


def batch(seed, B, n, m, real=None, periodic=False):
    """(ev0 [B][n][3], ev1 [B][m][3]): jet_events per pair, the second event heavier in the even pairs and lighter in the odd ones;
    periodic: the phi of the real particles uniform in [0, 2 pi)"""
    rng = np.random.default_rng(seed)
    a = np.stack([jet_events(rng, n, real) for _ in range(B)])
    b = np.stack([jet_events(rng, m, real, scale=0.7 if i % 2 else 1.3) for i in range(B)])
    if periodic:
        for ev in (a, b):
            ev[..., 2] = np.where(ev[..., 0] > 0, rng.random(ev.shape[:2]) * 2.0 * np.pi, 0.0)
    return a, b


def histories(ev0, ev1, epsilon, max_iter, debias, **opts):
    """[(err history, S)] of every problem of every pair of a batch run with tol = 0: what a choice of tol is judged on"""
    out = []
    for x, y in zip(ev0, ev1):
        r = sinkhorn(x, y, epsilon, max_iter=max_iter, tol=0.0, debias=debias, grad=False, **opts)
        out.append((r["history"], r["S"]))
        out.extend(r["self_history"])
    return out


def tol_is_safe(hist, tol):
    """every problem stops at an err below tol S / 4 after errs above 4 tol S only (or at its first test): a last-bit difference
    cannot move the count"""
    for h, S_ in hist:
        stop = next((k for k, e in enumerate(h) if e <= tol * S_), None)
        if stop is None or h[stop] >= tol * S_ / 4 or any(e <= 4 * tol * S_ for e in h[:stop]):
            return False
    return True
