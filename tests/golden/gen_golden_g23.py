#!/usr/bin/env python3
"""
Generate the g23 golden vectors under tests/golden/: the ROC curves and AUCs of the *reference's* get_ROC_AUC()
(utils/jet_analysis/anomaly_detection.py, save_path=None, plot_rocs=False; scikit-learn underneath).  Run it as gen_golden_g18.py
is run:

    cd "$(mktemp -d)" && PYTHONDONTWRITEBYTECODE=1 PYTHONPATH=<reference checkout> \
        python3 <this repo>/tests/golden/gen_golden_g23.py

anomaly_detection.py is loaded by file path under stub `utils` / `utils.jet_analysis` packages with a stub `energyflow`, exactly
as gen_golden_g18.py loads it.

Fixture g23_roc.npz, two sets (prefix a_ and b_), each with scores [M][K], labels [M], keys [K], fpr / tpr / thresholds [K][M + 1]
(the first length[k] entries of row k are the curve, the rest NaN), length [K], auc [K] and flipped [K] (the reference took its
"opposite labels" branch):
  a_  the 21 reference score columns of g18_anomaly_n30.npz under the reference's key strings; the first half of the jets is
      labelled +1, the rest -1
  b_  M = 300 synthetic scores, labels +-1 at random: "separated" (positives score higher), "inverted" (flips), "quarters" (quantised
      to 1/4: long tie groups), "equal" (all scores equal: AUC exactly 0.5, two points), "perfect" (AUC 1)
"""
import os
import sys

sys.dont_write_bytecode = True
import numpy as np  # noqa: E402

OUT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, OUT)
from gen_golden_g18 import load_reference  # noqa: E402


def run(AD, prefix, keys, scores, labels, out):
    M, K = scores.shape
    curves, aucs = AD.get_ROC_AUC({k: scores[:, i].copy() for i, k in enumerate(keys)}, labels, save_path=None, plot_rocs=False)
    assert list(curves) == list(keys) and list(aucs) == list(keys)
    pad = np.full((3, K, M + 1), np.nan)
    length = np.zeros(K, dtype=np.int64)
    flipped = np.zeros(K, dtype=np.int64)
    for i, k in enumerate(keys):
        length[i] = len(curves[k][0])
        for j in range(3):
            pad[j, i, :length[i]] = curves[k][j]
        first = AD.metrics.roc_curve(labels, scores[:, i])
        flipped[i] = AD.metrics.auc(first[0], first[1]) < 0.5
    out.update({prefix + "scores": scores, prefix + "labels": labels, prefix + "keys": np.array(list(keys)),
                prefix + "fpr": pad[0], prefix + "tpr": pad[1], prefix + "thresholds": pad[2], prefix + "length": length,
                prefix + "auc": np.array([aucs[k] for k in keys]), prefix + "flipped": flipped})
    print(prefix, "lengths", length.tolist(), "flipped", flipped.tolist(), "auc", np.round(out[prefix + "auc"], 4).tolist())


if __name__ == "__main__":
    AD = load_reference()
    out = {}

    g18 = np.load(os.path.join(OUT, "g18_anomaly_n30.npz"))
    scores = np.ascontiguousarray(g18["scores"], dtype=np.float64)
    B = scores.shape[0]
    labels = np.where(np.arange(B) < B // 2, 1.0, -1.0)
    run(AD, "a_", [str(k) for k in g18["keys"]], scores, labels, out)

    rng = np.random.default_rng(23)
    M = 300
    labels = np.where(rng.random(M) < 0.4, 1.0, -1.0)
    sep = rng.normal(size=M) + 1.5 * (labels == 1)
    cols = {"separated": sep, "inverted": -sep + 0.25 * rng.normal(size=M), "quarters": np.round(sep * 4) / 4,
            "equal": np.full(M, 0.75), "perfect": rng.random(M) + 2.0 * (labels == 1)}
    run(AD, "b_", list(cols), np.stack(list(cols.values()), axis=1), labels, out)

    np.savez_compressed(os.path.join(OUT, "g23_roc.npz"), **out)
    print("g23_roc.npz", os.path.getsize(os.path.join(OUT, "g23_roc.npz")), "bytes")
