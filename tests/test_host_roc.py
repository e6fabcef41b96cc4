"""Host-side tests of the native ROC curves and AUCs (no GPU): the numpy restatement tests/_roc_ref.py against the reference's g23
fixture and against scikit-learn where it is present, the C ABI of csrc/roc.hip (symbols, version, every argument refusal before any
launch) and lgn.anomaly's refusal to run without a GPU."""
import numpy as np
import pytest
import torch

import _roc_ref as R
import _util as U
from lgn import _native as N

P = 16          # placeholder device pointer: every call below must be refused before anything touches it
PTRS = (P,) * 10          # scores, labels, fpr, tpr, thresholds, length, auc, flipped, status, workspace
BIG = 1 << 40


@pytest.mark.parametrize("prefix", ["a_", "b_"])
def test_restatement_reproduces_the_reference_fixture(prefix):
    g = U.load("g23_roc.npz")
    scores, labels = g[prefix + "scores"], g[prefix + "labels"]
    for k in range(scores.shape[1]):
        fpr, tpr, thr, auc, flipped = R.roc_auc(labels, scores[:, k])
        n = int(g[prefix + "length"][k])
        assert len(fpr) == n and flipped == bool(g[prefix + "flipped"][k])
        assert np.array_equal(fpr, g[prefix + "fpr"][k, :n]) and np.array_equal(tpr, g[prefix + "tpr"][k, :n])
        assert np.array_equal(thr, g[prefix + "thresholds"][k, :n])
        assert np.isnan(g[prefix + "fpr"][k, n:]).all()
        assert abs(auc - g[prefix + "auc"][k]) <= R.auc_tolerance(n)
    if prefix == "b_":
        keys = list(g["b_keys"])
        assert list(g["b_flipped"]) == [0, 1, 0, 0, 0] and keys[1] == "inverted"
        assert g["b_auc"][keys.index("equal")] == 0.5 and g["b_length"][keys.index("equal")] == 2
        assert g["b_auc"][keys.index("perfect")] == 1.0


def test_restatement_equals_sklearn():
    metrics = pytest.importorskip("sklearn.metrics")
    rng = np.random.default_rng(5)
    for case in range(40):
        M = int(rng.integers(2, 400))
        labels = np.where(rng.random(M) < 0.5, 1.0, -1.0 if case % 2 else 0.0)
        labels[:2] = (1.0, labels[labels != 1].max(initial=-1.0 if case % 2 else 0.0))
        scores = rng.normal(size=M) + (0.5 if case % 3 else -0.5) * (labels == 1)
        if case % 4 == 0:
            scores = np.round(scores * 2) / 2
        ref = metrics.roc_curve(labels, scores)
        mine = R.roc_curve(labels, scores)
        for a, b in zip(ref, mine):
            assert np.array_equal(a, b)
        assert metrics.auc(ref[0], ref[1]) == R.auc(mine[0], mine[1])
        if case % 2:                 # the reference's flip: the curve of the negated labels is the exchanged curve
            neg = metrics.roc_curve(-labels, scores)
            assert np.array_equal(neg[0], mine[1]) and np.array_equal(neg[1], mine[0]) and np.array_equal(neg[2], mine[2])


def test_roc_symbols_are_exported():
    lib = N.lib()
    for name in ("lgn_roc_workspace_bytes", "lgn_roc_auc_f64"):
        assert name in N.EXPORTED_SYMBOLS
        assert hasattr(lib, name)
    assert lib.lgn_abi_version() == 19 and N.ABI_VERSION == 19
    header = open(U.ROOT + "/include/lgn_amd.h").read()
    for name, value in (("TILE", N.ROC_TILE), ("MAX_COLS", N.ROC_MAX_COLS), ("NONFINITE", N.ROC_NONFINITE),
                        ("SINGLE_CLASS", N.ROC_SINGLE_CLASS), ("BAD_LABEL", N.ROC_BAD_LABEL), ("NAN", N.ROC_NAN)):
        assert f"#define LGN_ROC_{name} {value}\n" in header
    from lgn import anomaly
    assert anomaly.ROC_TILE == N.ROC_TILE


@pytest.mark.parametrize("M,K", [(0, 1), (-1, 1), (1 << 31, 1), (10, 0), (10, -3), (10, 65536)])
def test_workspace_query_refuses_bad_sizes(M, K):
    assert N.lib().lgn_roc_workspace_bytes(M, K) < 0
    assert f"M = {M}, K = {K}" in N.last_error()


def test_workspace_query_grows_with_the_problem():
    L = N.lib()
    small, big = L.lgn_roc_workspace_bytes(1, 1), L.lgn_roc_workspace_bytes(200000, 21)
    assert 0 < small < big
    assert big >= 2 * 9 * 200000 * 21          # two buffers of 64-bit keys and label bits
    assert L.lgn_roc_workspace_bytes((1 << 31) - 1, 21) > (1 << 31) * 18 * 21 - (1 << 20)     # no 32-bit overflow


@pytest.mark.parametrize("ptrs,M,ld,K,nbytes,what", [
    *[(PTRS[:i] + (None,) + PTRS[i + 1:], 10, 3, 3, BIG, "null pointer") for i in range(10)],
    (PTRS, 0, 3, 3, BIG, "M = 0"),
    (PTRS, -5, 3, 3, BIG, "M = -5"),
    (PTRS, 1 << 31, 3, 3, BIG, "M = 2147483648"),
    (PTRS, 10, 3, 0, BIG, "K = 0"),
    (PTRS, 10, 3, -1, BIG, "K = -1"),
    (PTRS, 10, 2, 3, BIG, "ld = 2 < K = 3"),
    (PTRS, 10, 3, 3, 0, "too short"),
    (PTRS, 10, 3, 3, -1, "too short"),
])
def test_roc_auc_refusals(ptrs, M, ld, K, nbytes, what):
    scores, labels, fpr, tpr, thr, length, auc, flipped, status, work = ptrs
    assert N.lib().lgn_roc_auc_f64(scores, M, ld, K, labels, fpr, tpr, thr, length, auc, flipped, status, work, nbytes, None) < 0
    assert what in N.last_error()


def test_a_workspace_one_byte_short_is_refused():
    L = N.lib()
    need = L.lgn_roc_workspace_bytes(5000, 3)
    assert L.lgn_roc_auc_f64(P, 5000, 3, 3, P, P, P, P, P, P, P, P, P, need - 1, None) < 0
    assert f"{need} needed" in N.last_error()


def test_roc_needs_a_gpu(monkeypatch):
    from lgn import anomaly
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    scores = {"a": np.array([0.1, 0.7, 0.3]), "b": np.array([0.2, 0.1, 0.9])}
    with pytest.raises(RuntimeError, match="needs a GPU"):
        anomaly.get_ROC_AUC(scores, np.array([1.0, -1.0, 1.0]), plot_rocs=False)
    with pytest.raises(RuntimeError, match="needs a GPU"):
        anomaly.roc_auc_tensor(torch.zeros(3, 2, dtype=torch.float64), torch.ones(3))
