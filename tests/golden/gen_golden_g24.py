"""Writes tests/golden/g24_emd.npz: inputs and expected values of the native EMD score (csrc/emd.hip).

This is the project's own script: it imports nothing from the reference.  The expected values come from tests/_emd_ref.py, the LP
restatement of energyflow's documented definition of the EMD (R = 1, beta = 1, norm = False); the energyflow package itself was not
available, so no value in the fixture was produced by it.

    python tests/golden/gen_golden_g24.py

  rel_<tag>_recons / _target [B][N][4], rel_<tag>_emd [B]   the first (at most 16) jets of the three g18 anomaly fixtures: the
                                                             reference's 22nd score, EMD of the relative-polar frames
  gen_<n>x<m>_ev0 [B][n][3], _ev1 [B][m][3], _emd [B]        generic events of (pT, y, phi) with random positive weights, n != m
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import _emd_ref as E  # noqa: E402

REL = (("n12", "g18_anomaly_n12.npz"), ("n30", "g18_anomaly_n30.npz"), ("n150", "g18_anomaly_n150.npz"))
GENERIC = ((5, 8, 4), (1, 7, 4), (64, 65, 3))          # (n, m, pairs)
MAX_JETS = 16


def generic_events(n, m, B, seed):
    rng = np.random.default_rng(seed)

    def ev(k):
        return np.stack([rng.random((B, k)) + 0.05, rng.normal(size=(B, k)) * 0.4, rng.normal(size=(B, k)) * 0.4], axis=-1)
    return ev(n), ev(m)


def main():
    out = {}
    for tag, name in REL:
        z = np.load(os.path.join(HERE, name), allow_pickle=False)
        r, t = z["recons"][:MAX_JETS].astype(np.float64), z["target"][:MAX_JETS].astype(np.float64)
        out[f"rel_{tag}_recons"], out[f"rel_{tag}_target"] = r, t
        out[f"rel_{tag}_emd"] = E.emd_relative(r, t)
    for n, m, B in GENERIC:
        a, b = generic_events(n, m, B, seed=24000 + 100 * n + m)
        out[f"gen_{n}x{m}_ev0"], out[f"gen_{n}x{m}_ev1"] = a, b
        out[f"gen_{n}x{m}_emd"] = np.array([E.emd(a[i], b[i]) for i in range(B)])
    np.savez(os.path.join(HERE, "g24_emd.npz"), **out)
    for k, v in out.items():
        if k.endswith("_emd"):
            print(k, v)


if __name__ == "__main__":
    main()
