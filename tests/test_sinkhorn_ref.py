"""Pins the specification of the Sinkhorn calls itself: the numpy restatement tests/_sinkhorn_ref.py, converged, lies between the exact
EMD (tests/_emd_pairs_ref.py) and EMD + eps S log(S / w_min), grows with eps, has the plan marginals the stopping rule promises, has
envelope gradients that are the central differences of its value, and its debiased form vanishes for equal events.  No GPU."""
import numpy as np
import pytest

import _emd_pairs_ref as P
import _sinkhorn_ref as S

TOL = 1e-12
MAX_ITER = 200000
# (tag, n, m, real particles (None: all), scale of the second event's pT, options)
CASES = (("6x6_4real", 6, 6, 4, 1.0, {}), ("30x30", 30, 30, None, 1.0, {}), ("30x30_17real", 30, 30, 17, 1.0, {}),
         ("heavier_second", 8, 11, None, 1.6, {}), ("heavier_first", 11, 8, None, 0.6, {}), ("norm", 9, 7, None, 1.3, dict(norm=True)),
         ("beta2", 8, 8, None, 1.2, dict(beta=2.0)))


def _events(tag, n, m, real, scale):
    rng = np.random.default_rng(sum(map(ord, tag)))
    return S.jet_events(rng, n, real), S.jet_events(rng, m, real, scale=scale)


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
@pytest.mark.parametrize("eps", [0.03, 0.1])
def test_the_converged_value_lies_between_the_emd_and_its_entropic_bound(case, eps):
    """The lower bound is weak duality (1e-9 S for the finite tol); the upper one evaluates the objective at the LP's optimal plan,
    whose entropy term is at most eps S log(S / w_min), w_min the smallest positive extended weight."""
    tag, n, m, real, scale, o = case
    a, b = _events(tag, n, m, real, scale)
    r = S.sinkhorn(a, b, eps, max_iter=MAX_ITER, tol=TOL, grad=False, **o)
    assert r["status"] == 0 and r["err"] <= TOL * r["S"], (r["status"], r["iters"], r["err"])
    emd = P.emd(a, b, **o)
    _, wa, wb = P.balanced(a, b, **o)
    w_min = min(wa[wa > 0].min(), wb[wb > 0].min())
    bound = eps * r["S"] * np.log(r["S"] / w_min)
    print(f"{tag}, eps = {eps}: {r['iters']} iterations, E - EMD = {r['value'] - emd:.4e}, bound {bound:.4e}")
    assert emd - 1e-9 * r["S"] <= r["value"] <= emd + bound, (emd, r["value"], bound)


@pytest.mark.parametrize("case", CASES[:1] + CASES[3:], ids=[c[0] for c in CASES[:1] + CASES[3:]])
def test_the_value_does_not_decrease_with_epsilon(case):
    tag, n, m, real, scale, o = case
    a, b = _events(tag, n, m, real, scale)
    values = [S.sinkhorn(a, b, eps, max_iter=MAX_ITER, tol=TOL, grad=False, **o)["value"] for eps in (0.03, 0.06, 0.12, 0.5, 2.0)]
    assert all(y >= x - 1e-9 for x, y in zip(values, values[1:])), values


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_the_plan_has_the_marginals_the_stopping_rule_promises(case):
    """columns to rounding (the state ends on a g-update), rows within tol S in the l1 norm -- for a loose and for a tight tol"""
    tag, n, m, real, scale, o = case
    a, b = _events(tag, n, m, real, scale)
    _, wa, wb = P.balanced(a, b, **o)
    for tol in (1e-4, TOL):
        r = S.sinkhorn(a, b, 0.1, max_iter=MAX_ITER, tol=tol, grad=False, **o)
        assert r["status"] == 0
        assert np.abs(r["plan"].sum(0) - wb).max() <= 64 * 2.0 ** -53 * r["S"]
        rows = np.abs(r["plan"].sum(1) - wa).sum()
        assert rows <= tol * r["S"] * (1 + 1e-6) + 64 * 2.0 ** -53 * r["S"], (tol, rows)
        assert abs(rows - r["err"]) <= 1e-9 * r["S"] + 1e-3 * r["err"], (rows, r["err"])     # err IS the row violation, to first order
        assert np.all(r["plan"][wa == 0] == 0) and np.all(r["plan"][:, wb == 0] == 0)
        assert abs(r["plan"].sum() - r["S"]) <= 64 * 2.0 ** -53 * r["S"]


def test_the_stopping_rule_counts_as_the_header_says():
    a, b = _events("rule", 6, 7, None, 1.3)
    free = S.sinkhorn(a, b, 0.5, max_iter=9, tol=0.0, grad=False)
    assert free["iters"] == 9 and free["status"] == 0 and len(free["history"]) == 9
    h, Ssum = free["history"], free["S"]
    tol = np.sqrt(h[3] * h[4]) / Ssum                        # between the errors after 4 and after 5 iterations
    r = S.sinkhorn(a, b, 0.5, max_iter=9, tol=tol, grad=False)
    assert r["iters"] == 5 and r["status"] == 0 and r["err"] == h[4]
    short = S.sinkhorn(a, b, 0.5, max_iter=3, tol=1e-12, grad=False)
    assert short["iters"] == 3 and short["status"] == S.ITER and np.isfinite(short["value"]) and short["err"] == h[2]
    assert short["value"] <= r["value"] + 1e-12             # every iterate is a lower bound that the iteration raises


GRAD_CASES = (("6x6_4real", 6, 6, 4, 1.0, 0.05, dict()), ("heavier_second", 7, 9, None, 1.6, 0.05, dict()),
              ("heavier_first", 9, 7, None, 0.6, 0.05, dict(beta=2.0)), ("all", 7, 8, None, 1.3, 0.05, dict(R=0.8, beta=2.0, norm=True)),
              ("debias", 6, 7, None, 1.3, 0.5, dict(debias=True)), ("debias_norm", 7, 6, 5, 0.7, 0.5, dict(debias=True, norm=True)))


@pytest.mark.parametrize("case", GRAD_CASES, ids=[c[0] for c in GRAD_CASES])
def test_the_envelope_gradients_are_the_central_differences_of_the_value(case):
    """h = 1e-6 against the formula, within 100 x the deviation between the differences at h and at 2 h (which measures the
    truncation and rounding error of the difference itself); at least as many entries as particles are compared"""
    tag, n, m, real, scale, eps, o = case
    a, b = _events(tag, n, m, real, scale)
    kw = dict(max_iter=MAX_ITER, tol=TOL, **o)
    r = S.sinkhorn(a, b, eps, **kw)
    assert r["status"] == 0
    f1, f2 = S.fd_events(a, b, eps, h=1e-6, **kw), S.fd_events(a, b, eps, h=2e-6, **kw)
    for side, (g, d1, d2) in enumerate(zip((r["g0"], r["g1"]), f1, f2)):
        taken = ~np.isnan(d1)
        assert taken.sum() >= 2 * len(g)
        unit = np.abs(d1 - d2)[taken].max()
        err = np.abs(g - d1)[taken].max()
        print(f"{tag}, side {side}: |formula - difference| = {err:.3e}, |difference(h) - difference(2h)| = {unit:.3e}, max |g| = "
              f"{np.abs(g).max():.3e}")
        assert unit < 1e-6 * np.abs(g).max(), "the differences themselves are not settled"
        assert err <= 100 * unit, (tag, side, err, unit)
        if real is not None:                               # a weightless particle: no position gradient
            assert np.all(g[real:, 1:] == 0)


@pytest.mark.parametrize("o", [dict(), dict(norm=True), dict(R=0.8, beta=2.0, norm=True, periodic_phi=True)], ids=["default", "norm", "all"])
def test_the_debiased_value_is_zero_for_equal_events_and_not_negative_elsewhere(o):
    a, b = _events("debias0", 9, 9, 7, 1.2)
    for eps in (0.1, 1.0):
        kw = dict(max_iter=400, tol=1e-9, debias=True, **o)
        same = S.sinkhorn(a, a.copy(), eps, **kw)
        rounding = 64 * 2.0 ** -53 * same["S"] * max(1.0, eps * same["iters"])
        assert abs(same["value"]) <= rounding, same["value"]
        assert np.abs(same["g0"] + same["g1"])[:, 1:].max() <= 1e-9        # the position gradients of the two copies cancel
        other = S.sinkhorn(a, b, eps, **kw)
        assert other["value"] >= -rounding and other["value"] > 1e-3, other["value"]
