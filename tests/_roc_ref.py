"""
numpy-only restatement of what the reference's get_ROC_AUC() (utils/jet_analysis/anomaly_detection.py) computes per score kind:
sklearn.metrics.roc_curve(labels, scores) with its defaults, sklearn.metrics.auc(fpr, tpr), and the reference's flip.  No sklearn
import: the tests that use it run where sklearn may be absent (tests/test_host_roc.py compares it with sklearn where it is present).

1. roc_curve.  The positive class is label 1 (sklearn infers pos_label = 1 from labels in {0, 1} or {-1, 1}).
2. auc.        The trapezoid rule as numpy sums it: sum(diff(x) * (y[1:] + y[:-1]) / 2.0).
3. The algorithm, stage by stage (what csrc/roc.hip implements):
     a. sort the rows by descending score with a stable sort (mergesort argsort, reversed); -0.0 and +0.0 tie
     b. a tie group ends at row i when score[i] != score[i + 1], and at the last row
     c. at the last row i of each tie group: tps = positives in sorted rows 0 .. i, fps = i + 1 - tps, threshold = score[i]
     d. drop rule, when there are more than 2 groups: keep group j if it is the first, the last, or the second difference of fps or
        of tps at j is nonzero
     e. prepend the point (fps, tps, threshold) = (0, 0, +inf)
     f. fpr = fps / fps[-1], tpr = tps / tps[-1]
     g. auc; if auc < 0.5 the curve is that of the negated labels: fpr and tpr exchanged, thresholds unchanged (the drop rule is
        symmetric in fps and tps), and the auc is summed again from the exchanged curve
   The order inside a tie group does not matter: only its last row is read, and tps there counts the whole group.
"""
import numpy as np

SINGLE_CLASS = "Only one class present in y_true"


def roc_curve(labels, scores):
    """(fpr, tpr, thresholds) of sklearn.metrics.roc_curve(labels, scores) for labels in {0, 1} or {-1, 1} and finite scores."""
    y_score = np.asarray(scores, dtype=np.float64)
    y_true = np.asarray(labels) == 1
    order = np.argsort(y_score, kind="mergesort")[::-1]
    y_score, y_true = y_score[order], y_true[order]
    idx = np.r_[np.where(np.diff(y_score))[0], y_true.size - 1]
    tps = np.cumsum(y_true * 1.0, dtype=np.float64)[idx]
    fps = 1 + idx - tps
    thresholds = y_score[idx]
    if len(fps) > 2:
        keep = np.where(np.r_[True, np.logical_or(np.diff(fps, 2), np.diff(tps, 2)), True])[0]
        fps, tps, thresholds = fps[keep], tps[keep], thresholds[keep]
    tps, fps, thresholds = np.r_[0, tps], np.r_[0, fps], np.r_[np.inf, thresholds]
    if fps[-1] <= 0 or tps[-1] <= 0:
        raise ValueError(SINGLE_CLASS)          # sklearn returns NaN rates, on which metrics.auc raises
    return fps / fps[-1], tps / tps[-1], thresholds


def auc(x, y):
    return float((np.diff(x) * (y[1:] + y[:-1]) / 2.0).sum())


def roc_auc(labels, scores):
    """One score kind of get_ROC_AUC: (fpr, tpr, thresholds, auc, flipped)."""
    fpr, tpr, thr = roc_curve(labels, scores)
    a = auc(fpr, tpr)
    if a < 0.5:
        fpr, tpr = tpr, fpr
        return fpr, tpr, thr, auc(fpr, tpr), True
    return fpr, tpr, thr, a, False


def auc_tolerance(length):
    """|native - ref| allowed on an AUC whose curve has `length` points: length - 1 non-negative terms that total at most 1, three
    roundings per term, and at most (length - 2) 2^-53 from the order of the sum."""
    return (length + 2) * 2.0 ** -52
