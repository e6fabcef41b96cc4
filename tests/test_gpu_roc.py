"""Native ROC curves and AUCs (csrc/roc.hip, lgn.anomaly.roc_auc_tensor / get_ROC_AUC) against the numpy restatement of sklearn in
tests/_roc_ref.py and the reference's g23 fixture.  fpr, tpr, thresholds, length and flipped must be exactly equal (counts are
integers, each rate is one IEEE division); the AUC within _roc_ref.auc_tolerance(length).  Every random case keeps its reference AUC
1e-6 away from 0.5 (asserted), so that no flip hinges on the last bit of a sum."""
import numpy as np
import pytest
import torch

import _roc_ref as R
import _util as U
from lgn import _native as N
from lgn import anomaly as A

pytestmark = pytest.mark.gpu
T = A.ROC_TILE
DEV = "cuda:0"


def labels_for(rng, M, neg=-1.0):
    lab = np.where(rng.random(M) < 0.45, 1.0, neg)
    if M >= 2:
        lab[rng.integers(M)] = 1.0
        lab[(np.flatnonzero(lab == 1)[0] + 1) % M] = neg          # both classes present
    return lab


def three_columns(rng, M, labels):
    """continuous, rounded to 1/4 (long tie groups), all equal"""
    x = rng.normal(size=M) + 0.8 * (labels == 1)
    return np.stack([x, np.round(4 * (rng.normal(size=M) - 0.9 * (labels == 1))) / 4, np.full(M, -2.5)], axis=1)


def check(out, scores, labels, cols=None):
    """out: roc_auc_tensor's dict; scores (M, K) numpy: every column against the restatement"""
    o = {k: v.cpu().numpy() for k, v in out.items()}
    for k in range(scores.shape[1]) if cols is None else cols:
        fpr, tpr, thr, auc, flipped = R.roc_auc(labels, scores[:, k])
        n = len(fpr)
        if len(np.unique(scores[:, k])) > 1:          # (a constant column is exactly 0.5 on both sides and does not flip)
            assert abs(auc - 0.5) >= 1e-6 and abs(R.auc(*R.roc_curve(labels, scores[:, k])[:2]) - 0.5) >= 1e-6, "choose another seed"
        assert o["status"][k] == 0 and o["length"][k] == n and bool(o["flipped"][k]) == flipped, (k, o["length"][k], n)
        assert np.array_equal(o["fpr"][k, :n], fpr), k
        assert np.array_equal(o["tpr"][k, :n], tpr), k
        assert np.array_equal(o["thresholds"][k, :n], thr), k
        print(f"column {k}: length {n}, auc {o['auc'][k]!r} (ref {auc!r}), |diff| {abs(o['auc'][k] - auc):.3e}, "
              f"bound {R.auc_tolerance(n):.3e}")
        assert abs(o["auc"][k] - auc) <= R.auc_tolerance(n), k
    return o


def run(scores, labels):
    return A.roc_auc_tensor(torch.from_numpy(scores).to(DEV), torch.from_numpy(labels).to(DEV))


@pytest.mark.parametrize("prefix", ["a_", "b_"])
def test_fixture_through_get_ROC_AUC(prefix):
    g = U.load("g23_roc.npz")
    keys = [str(k) for k in g[prefix + "keys"]]
    scores = g[prefix + "scores"]
    given = {k: (scores[:, i] if i % 3 == 0 else torch.from_numpy(scores[:, i].copy()) if i % 3 == 1
                 else torch.from_numpy(scores[:, i].copy()).to(DEV)) for i, k in enumerate(keys)}
    curves, aucs = A.get_ROC_AUC(given, g[prefix + "labels"], plot_rocs=(prefix == "b_"))
    assert list(curves) == keys and list(aucs) == keys
    if prefix == "a_":
        assert tuple(keys) == A.SCORE_KEYS
    for i, k in enumerate(keys):
        n = int(g[prefix + "length"][i])
        for j, name in enumerate(("fpr", "tpr", "thresholds")):
            assert isinstance(curves[k][j], np.ndarray) and np.array_equal(curves[k][j], g[prefix + name][i, :n]), (k, name)
        assert isinstance(aucs[k], float) and abs(aucs[k] - g[prefix + "auc"][i]) <= R.auc_tolerance(n)
    flipped = A.roc_auc_tensor(torch.from_numpy(scores).to(DEV), torch.from_numpy(g[prefix + "labels"]).to(DEV))["flipped"]
    assert flipped.cpu().tolist() == g[prefix + "flipped"].tolist()


def test_get_ROC_AUC_in_groups_of_columns(monkeypatch):
    """a budget that holds 4 columns at a time: 21 kinds go in six groups, the last one short"""
    g = U.load("g23_roc.npz")
    keys = [str(k) for k in g["a_keys"]]
    M = g["a_scores"].shape[0]
    per_col = 3 * 8 * (M + 1) + N.lib().lgn_roc_workspace_bytes(M, 1)
    monkeypatch.setattr(A, "ROC_GROUP_BYTES", 4 * per_col + per_col // 2)
    launches = []
    native = A.roc_auc_tensor
    monkeypatch.setattr(A, "roc_auc_tensor", lambda s, l: launches.append(s.shape[1]) or native(s, l))
    curves, aucs = A.get_ROC_AUC({k: g["a_scores"][:, i] for i, k in enumerate(keys)}, g["a_labels"], plot_rocs=False)
    assert launches == [4, 4, 4, 4, 4, 1] and list(curves) == keys and list(aucs) == keys
    for i, k in enumerate(keys):
        n = int(g["a_length"][i])
        for j, name in enumerate(("fpr", "tpr", "thresholds")):
            assert np.array_equal(curves[k][j], g["a_" + name][i, :n]), (k, name)
        assert abs(aucs[k] - g["a_auc"][i]) <= R.auc_tolerance(n)


def test_get_ROC_AUC_saves_what_the_reference_saves(tmp_path):
    g = U.load("g23_roc.npz")
    keys = [str(k) for k in g["b_keys"]]
    given = {k: g["b_scores"][:, i] for i, k in enumerate(keys)}
    curves, aucs = A.get_ROC_AUC(given, g["b_labels"], save_path=tmp_path / "roc", plot_rocs=True, rocs_hlines=[0.1])
    assert sorted(p.name for p in (tmp_path / "roc").iterdir()) == ["aucs.pt", "roc_curves.pt", "scores.pt", "true_labels.pt"]
    saved = torch.load(tmp_path / "roc" / "aucs.pt", weights_only=False)
    assert saved == aucs and list(saved) == keys


@pytest.mark.parametrize("M", [2, 3, 63, 64, 65, T - 1, T, T + 1, 2 * T + 1, 3 * T + 17, 200003])
def test_sizes_at_the_seams_of_the_sort(M):
    rng = np.random.default_rng({3: 1024}.get(M, 1000 + M))     # (three rows have an AUC of 0, 1/2 or 1: a seed without the 1/2)
    labels = labels_for(rng, M)
    scores = three_columns(rng, M, labels)
    o = check(run(scores, labels), scores, labels)
    assert o["length"][2] == 2 and o["auc"][2] == 0.5 and o["flipped"][2] == 0          # the all-equal column


def test_one_row_is_a_single_class():
    with pytest.raises(ValueError, match="Only one class"):
        A.get_ROC_AUC({"a": np.array([0.3]), "b": np.array([0.1]), "c": np.array([0.2])}, np.array([1.0]), plot_rocs=False)
    out = run(np.array([[0.3, 0.1, 0.2]]), np.array([1.0]))
    assert out["status"].cpu().tolist() == [N.ROC_SINGLE_CLASS] * 3 and out["length"].cpu().tolist() == [0, 0, 0]


def test_key_map_orders_every_kind_of_double():
    rng = np.random.default_rng(7)
    tiny = np.float64(5e-324)
    special = np.array([0.0, -0.0, 0.0, -0.0, tiny, -tiny, 3 * tiny, 2.2250738585072014e-308, -2.2250738585072014e-308, 1e300, -1e300,
                        1.0, np.nextafter(1.0, 2.0), np.nextafter(1.0, 0.0), -1.0, np.nextafter(-1.0, 0.0), np.nextafter(-1.0, -2.0),
                        1e-300, -1e-300, 0.5, -0.5, np.finfo(np.float64).max, -np.finfo(np.float64).max])
    col = np.concatenate([special, special, rng.normal(size=40), -rng.random(30) * 1e-310])
    rng.shuffle(col)
    M = len(col)
    labels = np.where(np.argsort(np.argsort(col)) + rng.integers(-20, 20, size=M) > M // 2, 1.0, 0.0)
    labels[:2] = (1.0, 0.0)
    scores = np.stack([col, -col], axis=1)
    check(run(scores, labels), scores, labels)


def test_degenerate_curves():
    rng = np.random.default_rng(11)
    M = 777
    labels = labels_for(rng, M)
    perfect = rng.random(M) + 2.0 * (labels == 1)
    two = np.where(rng.random(M) < 0.5 + 0.3 * (labels == 1), 1.0, -1.0)
    scores = np.stack([perfect, -perfect, two], axis=1)
    o = check(run(scores, labels), scores, labels)
    assert o["auc"][0] == 1.0 and o["flipped"][0] == 0
    assert o["auc"][1] == 1.0 and o["flipped"][1] == 1
    assert o["length"][2] <= 3


@pytest.mark.parametrize("neg", [-1.0, 0.0])
def test_layout_in_place_and_column_views(neg):
    rng = np.random.default_rng(21 + int(neg))
    M = T + 300
    labels = labels_for(rng, M, neg)
    scores = rng.normal(size=(M, 21)) + np.linspace(-1.0, 1.0, 21) * (labels == 1)[:, None]
    scores[:, 10] += 0.3 * (labels == 1)           # (the middle column would otherwise sit at an AUC of 0.5)
    scores[:, 3] = np.round(scores[:, 3] * 2) / 2
    dev = torch.from_numpy(scores).to(DEV)
    for lab in (torch.from_numpy(labels).to(DEV), torch.from_numpy(labels).to(DEV).to(torch.int32), torch.from_numpy(labels)):
        check(A.roc_auc_tensor(dev, lab), scores, labels)
    view = dev[:, 7:12]
    assert view.stride() == (21, 1)
    out = A.roc_auc_tensor(view, torch.from_numpy(labels).to(DEV))
    assert out["auc"].shape == (5,) and out["fpr"].shape == (5, M + 1)
    check(out, scores[:, 7:12], labels)


def test_refusals_by_status():
    rng = np.random.default_rng(31)
    M = T + 9
    labels = labels_for(rng, M)
    scores = three_columns(rng, M, labels)
    names = ("a", "b", "c")
    for bad, bits, message in ((np.nan, N.ROC_NONFINITE | N.ROC_NAN, r"^Input contains NaN\.$"),
                               (np.inf, N.ROC_NONFINITE, r"^Input contains infinity or a value too large for dtype\('float64'\)\.$"),
                               (-np.inf, N.ROC_NONFINITE, r"^Input contains infinity")):
        s = scores.copy()
        s[T + 3, 1] = bad
        out = run(s, labels)
        o = check(out, s, labels, cols=(0, 2))
        assert o["status"].tolist() == [0, bits, 0] and o["length"][1] == 0 and np.isnan(o["auc"][1]) and o["flipped"][1] == 0
        with pytest.raises(ValueError, match=message):
            A.get_ROC_AUC({k: s[:, i] for i, k in enumerate(names)}, labels, plot_rocs=False)
    for lab, bit in ((np.where(np.arange(M) == 5, 2.0, labels), N.ROC_BAD_LABEL),
                     (np.where(np.arange(M) == M - 1, 0.0, np.where(np.arange(M) == 0, -1.0, labels)), N.ROC_BAD_LABEL),
                     (np.ones(M), N.ROC_SINGLE_CLASS), (-np.ones(M), N.ROC_SINGLE_CLASS), (np.zeros(M), N.ROC_SINGLE_CLASS)):
        o = {k: v.cpu().numpy() for k, v in run(scores, lab).items()}
        assert o["status"].tolist() == [bit] * 3 and o["length"].tolist() == [0] * 3 and np.isnan(o["auc"]).all()
        with pytest.raises(ValueError):
            A.get_ROC_AUC({k: scores[:, i] for i, k in enumerate(names)}, lab, plot_rocs=False)


def test_scores_then_roc_in_one_graph_without_a_sync():
    B = 2 * T + 5                                  # jets; a merge pass runs
    def inputs(seed):
        r = np.random.default_rng(seed)
        t = AR_jets(r, B, 6)
        rec = t + r.normal(scale=0.3, size=t.shape) * np.where(np.arange(B) < B // 2, 1.0, 1.6)[:, None, None]
        norm = lambda x: x / (np.abs(x).max(-2, keepdims=True) + 1e-16)
        return [torch.from_numpy(a).to(DEV) for a in (rec, t, norm(rec), norm(t))]

    labels = torch.from_numpy(np.where(np.arange(B) < B // 2, -1.0, 1.0)).to(DEV)
    # seeds 1 and 3: every one of the 21 score kinds is at least 0.025 from an AUC of 0.5 (Hungarian Lorentz is the closest), three flip
    first, second = inputs(1), inputs(3)
    static = [x.clone() for x in first]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        A.roc_auc_tensor(A.score_tensor(*static), labels)      # warm-up outside the capture
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            out = A.roc_auc_tensor(A.score_tensor(*static), labels)
    torch.cuda.current_stream().wait_stream(side)
    for given in (second, first):
        for dst, src in zip(static, given):
            dst.copy_(src)
        graph.replay()
        torch.cuda.synchronize()
        replayed = {k: v.clone() for k, v in out.items()}
        eager_scores = A.score_tensor(*given)
        eager = A.roc_auc_tensor(eager_scores, labels)
        again = A.roc_auc_tensor(eager_scores, labels)
        for k in ("length", "flipped", "status", "auc"):
            assert torch.equal(replayed[k], eager[k]) and torch.equal(again[k], eager[k]), k
        assert eager["status"].abs().sum().item() == 0
        for k in ("fpr", "tpr", "thresholds"):
            for c, n in enumerate(eager["length"].tolist()):
                assert torch.equal(replayed[k][c, :n], eager[k][c, :n]) and torch.equal(again[k][c, :n], eager[k][c, :n]), (k, c)
        o = check(eager, eager_scores.cpu().numpy(), labels.cpu().numpy())
        assert o["flipped"].sum() == 3


def AR_jets(rng, B, n):
    p3 = rng.normal(size=(B, n, 3)) * np.array([1.0, 1.0, 2.0])
    E = np.sqrt((p3 ** 2).sum(-1)) + np.abs(rng.normal(scale=0.1, size=(B, n)))
    return np.concatenate([E[..., None], p3], -1)
