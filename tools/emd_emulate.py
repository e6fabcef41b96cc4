#!/usr/bin/env python3
"""numpy emulation of emd_wave (csrc/emd_wave.hpp), step for step -- row sources in order, the sink-first / lowest-index selection,
backward arcs through a finalised column's flows, the two-walk augmentation -- on random events: checks the value against the LP
restatement tests/_emd_ref.py, the potentials and the marginals, and counts the augmentations per node (rows + cols), the figure the
solver's cap of 16 per node is set against.  Host only.
    python tools/emd_emulate.py"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _emd_ref as E  # noqa: E402


def solve(c, a, b, max_aug=10**9):
    rows, cols = c.shape
    sup, dem = a.copy(), b.copy()
    live = dem > 0
    u, v = np.zeros(rows), np.zeros(cols)
    F = np.zeros((rows, cols))
    n_aug = 0
    for s in range(rows):
        while sup[s] > 0:
            spc = np.full(cols, np.inf); vis = np.zeros(cols, bool); path = np.full(cols, -1)
            rvis = np.zeros(rows, bool); rvis[s] = True; pred = np.full(rows, -1); dist = np.zeros(rows)

            def scan(i, di):
                o = live & ~vis
                r = ((di + c[i]) - u[i]) - v
                better = o & (r < spc)
                spc[better] = r[better]; path[better] = i
            scan(s, 0.0)
            D, sink = 0.0, -1
            for sel in range(cols):
                o = live & ~vis
                if not o.any():
                    break
                lowest = spc[o].min()
                if not lowest < np.inf:
                    break
                cand = np.flatnonzero(o & (spc == lowest))
                sinks = cand[dem[cand] > 0]
                j = sinks[0] if len(sinks) else cand[0]
                D = lowest; vis[j] = True
                if dem[j] > 0:
                    sink = j; break
                reach = np.flatnonzero(~rvis & (F[:, j] > 0))
                rvis[reach] = True; pred[reach] = j; dist[reach] = D
                for i in reach:
                    scan(i, D)
            if sink < 0:                      # the sums agree to rounding only: what is left is dropped (the kernel checks its size)
                break
            u[rvis] += D - dist[rvis]
            v[vis] -= D - spc[vis]
            delta = min(sup[s], dem[sink]); j = sink
            while True:
                i = path[j]; pj = pred[i]
                if pj < 0:
                    assert i == s; break
                delta = min(delta, F[i, pj]); j = pj
            assert delta > 0
            j = sink
            while True:
                i = path[j]; pj = pred[i]
                F[i, j] += delta
                if pj < 0: break
                F[i, pj] -= delta; j = pj
            sup[s] -= delta; dem[sink] -= delta; n_aug += 1
    dead = ~live
    if dead.any():
        v[dead] = (c[:, dead] - u[:, None]).min(0)
    return (F, u, v), 0.0, n_aug


rng = np.random.default_rng(0)
worst = 0
for (n, m, ties) in [(5, 8, 0), (1, 7, 0), (12, 12, 0), (30, 30, 0), (30, 30, 1), (64, 65, 0), (20, 20, 2), (100, 100, 0), (150, 150, 0), (100, 100, 1)]:
    for rep in range(3):
        ev0 = np.stack([rng.random(n) + 0.01, rng.normal(size=n), rng.normal(size=n)], -1)
        ev1 = np.stack([rng.random(m) + 0.01, rng.normal(size=m), rng.normal(size=m)], -1)
        if ties == 1:
            ev0[:, 0] = 1.0 / n; ev1[:, 0] = 1.0 / m
        if ties == 2:
            ev0[:, 0] = 0.25; ev1[:, 0] = 0.25; ev0[::2, 1:] = ev0[0, 1:]; ev1[::3, 1:] = ev0[0, 1:]; ev0[5:9, 0] = 0
        c, a, b = E.balanced(ev0, ev1)
        t = time.time()
        out, left, na = solve(c, a, b)
        t1 = time.time() - t
        F, u, v = out
        val = (F * c).sum()
        t = time.time()
        ref = E.emd(ev0, ev1)
        t2 = time.time() - t
        slack = (c - u[:, None] - v[None, :]).min()
        dual = (u * a).sum() + (v * b).sum()
        worst = max(worst, na / (n + m + 2))
        print(n, m, ties, "aug", na, "ratio %.2f" % (na / (n + m + 2)), "rel err %.1e" % (abs(val - ref) / ref), "slack %.1e" % slack,
              "gap %.1e" % (abs(dual - val) / val), "rowerr %.1e" % np.abs(F.sum(1) - a).max(), "colerr %.1e" % np.abs(F.sum(0) - b).max(),
              "t %.2f %.2f" % (t1, t2))
print("worst aug ratio", worst)
