#!/usr/bin/env python3
"""Native reconstruction analysis in jets/s: lgn.analysis.recon_analysis at B = 65,536, N = 30 (20 real particles; with and without
the two assignments) and lgn.analysis.particle_histograms of its output over 81 edges, next to (a) a Hungarian anomaly-score pass
with two variants at the same shape (lgn_anomaly_scores_f64, Cartesian and relative polar) and (b) the reference's path on the host:
the scipy loop of tests/_analysis_ref.py on a 4,096-jet slice, split over the host's worker processes and scaled linearly.  The
workers are started and have imported numpy / scipy and run a few jets before anything is timed; the slice is then run `runs` times on
the warm pool: the median wall time of a run and the longest worker's own time (taken inside the worker) are printed.
Device times are events around `steps` calls after a warm-up, repeated `runs` times: the median and the spread (min .. max) are
printed.  One JSON line.
    python tools/analysis_bench.py [--steps K] [--warmup W] [--runs R] [--host-jets 4096] [--workers 16]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "lgn-autoencoder_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

import numpy as np  # noqa: E402


def _host_slice(args):
    import _analysis_ref as R
    t, r = args
    t0 = time.perf_counter()
    R.recon_analysis(t, r)
    return time.perf_counter() - t0


def timed(fn, steps, warmup, runs):
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(runs):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(steps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1) / steps)
    return {"ms": round(float(np.median(ms)), 4), "min": round(min(ms), 4), "max": round(max(ms), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--jets", type=int, default=65536)
    ap.add_argument("--host-jets", type=int, default=4096)
    ap.add_argument("--workers", type=int, default=int(os.environ.get("OMP_NUM_THREADS", "16")))
    args = ap.parse_args()
    # the reference's path on the host first, before this process opens the GPU: the scipy loop on a slice of jets made as the
    # device's are, over fresh worker processes, scaled linearly
    import multiprocessing as mp
    from concurrent.futures import ProcessPoolExecutor
    hj, w = args.host_jets, max(1, args.workers)
    rng = np.random.default_rng(1)
    th = rng.normal(size=(hj, 30, 4))
    th[..., 0] = np.linalg.norm(th[..., 1:], axis=-1) + 0.1
    th[:, 20:] = 0.0
    rh = th + 0.2 * rng.normal(size=th.shape)
    parts = [(th[i::w], rh[i::w]) for i in range(w)]
    walls, inside = [], []
    with ProcessPoolExecutor(w, mp_context=mp.get_context("spawn")) as ex:
        list(ex.map(_host_slice, [(th[:8], rh[:8])] * (4 * w)))      # start every worker: imports, first calls
        for _ in range(args.runs):
            t0 = time.perf_counter()
            own = list(ex.map(_host_slice, parts))
            walls.append(time.perf_counter() - t0)
            inside.append(max(own))
    wall = float(np.median(walls))
    host = {"jets": hj, "workers": w, "runs": args.runs, "seconds": round(wall, 4), "seconds_min": round(min(walls), 4),
            "seconds_max": round(max(walls), 4), "longest_worker_seconds": round(float(np.median(inside)), 4),
            "jets_per_s": round(hj / wall)}

    import torch
    from lgn import analysis as A
    from lgn import anomaly as AN
    if not torch.cuda.is_available():
        sys.exit("analysis_bench: no GPU; a device time is never estimated on the host")
    dev = torch.device("cuda:0")
    B, n, real = args.jets, 30, 20
    g = torch.Generator(device=dev).manual_seed(1)
    t = torch.randn(B, n, 4, device=dev, dtype=torch.float64, generator=g)
    t[..., 0] = t[..., 1:].norm(dim=-1) + 0.1
    t[:, real:] = 0.0
    r = t + 0.2 * torch.randn(B, n, 4, device=dev, dtype=torch.float64, generator=g)
    res = {"B": B, "N": n, "real_particles": real, "steps": args.steps, "runs": args.runs}
    res["recon_analysis"] = timed(lambda: A.recon_analysis(t, r), args.steps, args.warmup, args.runs)
    res["recon_analysis_no_match"] = timed(lambda: A.recon_analysis(t, r, residuals=False), args.steps, args.warmup, args.runs)
    out = A.recon_analysis(t, r)
    e = [np.linspace(-2.0, 2.0, 81)] * 3
    ranges = {k: e for k in ("p_cartesian", "p_polar", "rel_err_cartesian", "rel_err_polar", "rel_err_polarrel", "padded_cartesian",
                             "padded_polar", "padded_polarrel")}
    res["particle_histograms"] = timed(lambda: A.particle_histograms(out, ranges), args.steps, args.warmup, args.runs)
    norm = lambda x: x / (x.abs().amax(-2, keepdim=True) + 1e-16)
    xs = [r, t, norm(r), norm(t)]
    sc, st = torch.empty(B, 21, device=dev, dtype=torch.float64), torch.empty(B, device=dev, dtype=torch.int32)
    two = (1 << 5) | (1 << 9)              # Hungarian, Cartesian and relative polar
    res["anomaly_two_hungarian"] = timed(lambda: AN._launch(xs, two, sc, st), args.steps, args.warmup, args.runs)
    for k in ("recon_analysis", "recon_analysis_no_match", "anomaly_two_hungarian"):
        res[k]["jets_per_s"] = round(B / (res[k]["ms"] * 1e-3))

    host["scaled_to_B_seconds"] = round(wall * B / hj, 3)
    res["host_scipy_loop"] = host
    res["speedup_vs_host"] = round(host["scaled_to_B_seconds"] / (res["recon_analysis"]["ms"] * 1e-3), 1)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
