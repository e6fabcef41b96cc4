"""Host-side checks of the anomaly scores: the numpy restatement (tests/_anomaly_ref.py) against the reference-pinned g18 fixtures and
against scipy's linear_sum_assignment, the new C entry points' symbols, and their refusals before any launch.  No GPU needed."""
import numpy as np
import pytest

import _anomaly_ref as R
from _util import load, meta
from lgn import _native as N

G18 = ("g18_anomaly_n12.npz", "g18_anomaly_n30.npz", "g18_anomaly_n150.npz")
POLAR = (1, 3, 4, 6, 8, 9, 11, 13, 14)          # score slots in the polar frames (host asinh / atan2 differ from torch's in ulps)


@pytest.mark.parametrize("name", G18)
def test_restatement_matches_the_reference_fixture(name):
    z = load(name)
    assert tuple(str(k) for k in z["keys"]) == R.SCORE_KEYS
    scores, col = R.anomaly_scores(z["recons"], z["target"], z["recons_n"], z["target_n"])
    assert np.array_equal(col, z["col4row"])
    for s in range(21):
        np.testing.assert_allclose(scores[:, s], z["scores"][:, s], rtol=1e-11 if s in POLAR else 1e-12, atol=0, err_msg=R.SCORE_KEYS[s])
    assert meta(z)["B"] == z["recons"].shape[0]


def test_fixtures_hold_the_degenerate_jet():
    z = load("g18_anomaly_n30.npz")
    m = meta(z)
    assert m["same"] and all(b not in m["dropped"] for b in m["same"])
    b = m["same"][0] - sum(d < m["same"][0] for d in m["dropped"])
    assert np.array_equal(z["recons"][b], z["target"][b]) and (z["target"][b] == 0).all(-1).any()


def _matrices(seed):
    rng = np.random.default_rng(seed)
    for it in range(600):
        n = int(rng.integers(1, 24))
        kind = it % 5
        if kind == 0:
            yield rng.normal(size=(n, n))
        elif kind == 1:
            yield rng.integers(0, 3, size=(n, n)).astype(np.float64)
        elif kind == 2:
            yield -rng.random(size=(n, n))
        elif kind == 3:
            yield np.full((n, n), 2.5)
        else:
            c = rng.integers(0, 2, size=(n, n)).astype(np.float64)
            c[:, rng.integers(0, n)] = 0.0
            c[rng.integers(0, n)] = c[0]
            yield c


def test_restated_assignment_is_scipys():
    scipy_opt = pytest.importorskip("scipy.optimize")
    for c in _matrices(7):
        assert np.array_equal(R.lsap(c), scipy_opt.linear_sum_assignment(c)[1]), c


def test_restated_assignment_refuses_what_scipy_refuses():
    with pytest.raises(ValueError, match="invalid numeric entries"):
        R.lsap(np.array([[0.0, np.nan], [1.0, 2.0]]))
    with pytest.raises(ValueError, match="infeasible"):
        R.lsap(np.array([[np.inf, np.inf], [1.0, 2.0]]))


def test_anomaly_symbols_are_exported():
    lib = N.lib()
    for name in ("lgn_anomaly_scores_f64", "lgn_linear_sum_assignment_f64"):
        assert name in N.EXPORTED_SYMBOLS
        assert hasattr(lib, name)
    assert lib.lgn_abi_version() == 19


ALL = (1 << 21) - 1
P = 8          # placeholder device pointer: every call below must be refused before anything touches it


@pytest.mark.parametrize("B,n,mask,ptrs,what", [
    (0, 30, ALL, (P, P, P, P, P, P), "B = 0"),
    (4, 0, ALL, (P, P, P, P, P, P), "N = 0"),
    (4, 193, ALL, (P, P, P, P, P, P), "N = 193"),
    (4, 30, ALL, (P, None, P, P, P, P), "null input"),
    (4, 30, ALL, (P, P, P, None, P, P), "null input"),
    (4, 30, ALL, (P, P, P, P, None, P), "null scores"),
    (4, 30, ALL, (P, P, P, P, P, None), "null status"),
    (4, 30, 1 << 21, (P, P, P, P, P, P), "unknown score_mask"),
    (4, 30, -1, (P, P, P, P, P, P), "unknown score_mask"),
])
def test_anomaly_scores_refusals(B, n, mask, ptrs, what):
    r, t, rn, tn, sc, st = ptrs
    assert N.lib().lgn_anomaly_scores_f64(r, t, rn, tn, B, n, mask, sc, None, st, None) < 0
    assert what in N.last_error()


@pytest.mark.parametrize("B,n,ptrs,what", [
    (0, 5, (P, P, P), "B = 0"),
    (2, 0, (P, P, P), "n = 0"),
    (2, 193, (P, P, P), "n = 193"),
    (2, 5, (None, P, P), "null cost"),
    (2, 5, (P, None, P), "null col4row"),
    (2, 5, (P, P, None), "null status"),
])
def test_linear_sum_assignment_refusals(B, n, ptrs, what):
    c, col, st = ptrs
    assert N.lib().lgn_linear_sum_assignment_f64(c, B, n, col, st, None) < 0
    assert what in N.last_error()
