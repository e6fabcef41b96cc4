#!/usr/bin/env python3
"""
Generate the g18 golden vectors under tests/golden/: the per-jet anomaly scores of the *reference's* anomaly_scores()
(utils/jet_analysis/anomaly_detection.py, include_emd=False, batch_size=-1).  Run it as gen_golden.py is run:

    cd "$(mktemp -d)" && PYTHONDONTWRITEBYTECODE=1 PYTHONPATH=<reference checkout> \
        python3 <this repo>/tests/golden/gen_golden_g18.py

utils/jet_analysis/__init__.py imports coffea, which the scores do not need: anomaly_detection.py (and the utils.py it imports) are
loaded by file path under stub `utils` / `utils.jet_analysis` packages, and a stub `energyflow` stands in (EMD stays off).

Fixtures:
  g18_anomaly_n30.npz   N = 30, B = 64: twenty jets zero padded to 8 .. 29 real particles, one jet with recons == target
  g18_anomaly_n12.npz   N = 12, B = 16
  g18_anomaly_n150.npz  N = 150, B = 4
Each holds recons, target, recons_n, target_n [B][N][4], scores [B][21] (the reference's, in its key order; keys: the key strings),
col4row [6][B][N] (scipy.optimize.linear_sum_assignment(cost)[1] of the six Hungarian variants, in score order) and meta.

torch.cdist switches to a matrix-product formula past 25 points, so the reference's Euclidean costs are not the exact distances in
the last bits.  For every jet and variant the generator checks that scipy's col_ind on the exact costs equals the one on the
reference's costs, and that the reference's Hungarian score is the score of that pairing; a jet where either fails is left out of
the fixture (meta.dropped).  The tie behaviour of such jets is pinned against the restatement in tests/_anomaly_ref.py instead.
"""
import importlib.util
import json
import os
import sys
import types

sys.dont_write_bytecode = True
import numpy as np  # noqa: E402
import torch  # noqa: E402
from scipy.optimize import linear_sum_assignment  # noqa: E402

OUT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(OUT))
import _anomaly_ref as R  # noqa: E402


def load_reference():
    root = next(p for p in sys.path if p and os.path.isfile(os.path.join(p, "utils", "jet_analysis", "anomaly_detection.py")))
    ja = os.path.join(root, "utils", "jet_analysis")
    for name, path in (("utils", os.path.join(root, "utils")), ("utils.jet_analysis", ja)):
        pkg = types.ModuleType(name)
        pkg.__path__ = [path]
        sys.modules[name] = pkg
    sys.modules["energyflow"] = types.ModuleType("energyflow")
    mods = {}
    for sub in ("utils", "anomaly_detection"):
        spec = importlib.util.spec_from_file_location(f"utils.jet_analysis.{sub}", os.path.join(ja, f"{sub}.py"))
        m = importlib.util.module_from_spec(spec)
        sys.modules[spec.name] = m
        spec.loader.exec_module(m)
        mods[sub] = m
    return mods["anomaly_detection"]


def jets(rng, B, N, pad=()):
    """Massless-ish random particles; rows pad[b] .. N-1 of jet b zeroed (target and recons alike)."""
    p3 = rng.normal(size=(B, N, 3)) * np.array([1.0, 1.0, 2.0])
    E = np.sqrt((p3 ** 2).sum(-1)) + np.abs(rng.normal(scale=0.1, size=(B, N)))
    x = np.concatenate([E[..., None], p3], -1)
    for b, n in pad:
        x[b, n:] = 0.0
    return x


def normalize(x):          # normalize_particle_features: per jet and component, divided by the largest |value|
    return x / (np.abs(x).max(-2, keepdims=True) + 1e-16)


def case(AD, name, B, N, seed, pad=(), same=()):
    rng = np.random.default_rng(seed)
    target = jets(rng, B, N, pad)
    recons = target + rng.normal(scale=0.3, size=target.shape)
    for b, n in pad:
        recons[b, n:] = rng.normal(scale=1e-3, size=(N - n, 4))     # the decoder does not reproduce exact zeros
    for b in same:
        recons[b] = target[b]
    recons_n, target_n = normalize(recons), normalize(target)
    t = [torch.from_numpy(a) for a in (recons, target, recons_n, target_n)]
    ref = AD.anomaly_scores(*t, include_emd=False, batch_size=-1)
    keys = list(ref)
    assert tuple(keys) == R.SCORE_KEYS, keys
    scores = np.stack([ref[k] for k in keys], -1)

    # the reference's cost matrices, and the exact ones
    fr = R.frames(recons, target, recons_n, target_n)
    col = np.zeros((6, B, N), dtype=np.int64)
    keep = np.ones(B, bool)
    for f, (p, q, lor) in enumerate(fr):
        pt, qt = torch.from_numpy(np.ascontiguousarray(p[..., :3] if f == 4 else p)), torch.from_numpy(np.ascontiguousarray(q[..., :3] if f == 4 else q))
        if lor:
            ref_cost = AD.norm_sq_Lorentz(pt.unsqueeze(-2) - qt.unsqueeze(-3)).numpy()
            exact = ref_cost
        else:
            ref_cost = torch.cdist(pt, qt).numpy()
            exact = torch.cdist(pt, qt, compute_mode="donot_use_mm_for_euclid_dist").numpy()
        for b in range(B):
            c_ref = linear_sum_assignment(ref_cost[b])[1]
            c_ex = linear_sum_assignment(exact[b])[1]
            col[f, b] = c_ex
            pe, qe = (recons[b], target[b]) if lor else (p[b], q[b])
            d = pe[c_ex] - qe
            mine = (d * d).sum(-1).mean()
            if not np.array_equal(c_ref, c_ex) or abs(mine - scores[b, R.HUNGARIAN_INDEX[f]]) > 1e-12 * max(abs(mine), 1e-300):
                keep[b] = False
    dropped = [int(b) for b in np.flatnonzero(~keep)]
    k = keep
    meta = dict(B=int(k.sum()), N=N, seed=seed, pad=[list(map(int, x)) for x in pad], same=list(map(int, same)), dropped=dropped,
                source="utils/jet_analysis/anomaly_detection.py: anomaly_scores(include_emd=False, batch_size=-1)")
    np.savez_compressed(os.path.join(OUT, name), recons=recons[k], target=target[k], recons_n=recons_n[k], target_n=target_n[k],
                        scores=scores[k], col4row=col[:, k], keys=np.array(keys), meta=np.array(json.dumps(meta)))
    print(name, "jets", int(k.sum()), "dropped", dropped)


if __name__ == "__main__":
    torch.set_num_threads(8)
    AD = load_reference()
    rng = np.random.default_rng(18)
    pad30 = tuple((b, int(rng.integers(8, 30))) for b in range(20))
    case(AD, "g18_anomaly_n30.npz", 64, 30, 1830, pad=pad30, same=(5,))
    case(AD, "g18_anomaly_n12.npz", 16, 12, 1812)
    case(AD, "g18_anomaly_n150.npz", 4, 150, 18150)
