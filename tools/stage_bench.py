#!/usr/bin/env python3
"""Staging of a batch under --normalize: the one native launch (lgn_stage_batch_f64, _StaticInputs.stage with normalize=True) next
to the torch sequence a caller needed before it -- normalize_p4 in torch, then _StaticInputs.stage -- at 512 x 30, 64 x 30 and
512 x 150, non-split and split (jet_features), host and device time per call; and NativeEvalStep with and without normalize (the
de-normalise kernel inside the graph).  One JSON line per configuration.    python tools/stage_bench.py [--iters K] [--warmup W]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "lgn-autoencoder_amd"))
import torch  # noqa: E402

SHAPES = [(512, 30), (64, 30), (512, 150)]
EPS = 1e-16


def torch_normalize(p4, method):
    """utils/normalize_p4.py in eager torch."""
    if method == "component_max":
        f = torch.abs(p4).amax(dim=-2, keepdim=True) + EPS
    elif method == "overall_max":
        f = torch.abs(p4).amax(dim=-1, keepdim=True).amax(dim=-2, keepdim=True) + EPS
    else:
        f = p4.sum(dim=-2, keepdim=True)[..., 0].unsqueeze(-1) + EPS
    return p4 / f, f


def timed(fn, iters, warmup):
    """(host ms per call: time to enqueue; device ms per call: event time over the back-to-back calls)."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    host = (time.perf_counter() - t0) / iters * 1e3
    torch.cuda.synchronize()
    return host, e0.elapsed_time(e1) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--method", default="overall_max")
    args = ap.parse_args()
    import bench
    import __graft_entry__ as G
    from lgn.step import NativeEvalStep, _StaticInputs
    dev = torch.device("cuda:0")
    r4 = lambda d: {k: (round(v, 4) if isinstance(v, float) else v) for k, v in d.items()}      # noqa: E731
    for B, N in SHAPES:
        p4, _ = bench.synthetic_jets(B, N, seed=5)
        raw = (p4 * 37.0).to(dev)
        for split in (False, True):
            enc, dec = G._models(N, (3, 3, 4, 4), (4, 4, 3, 3), dev, seed=0, jet_features=split)
            enc.scale = 0.5
            native = _StaticInputs(enc, dec, B, split, False, normalize=True, normalize_method=args.method)
            plain = _StaticInputs(enc, dec, B, split, False)

            def torch_path():
                norm, f = torch_normalize(raw, args.method)
                plain.stage({"p4": norm})
                return f

            res = {"what": "stage", "B": B, "N": N, "split": split, "method": args.method}
            res["native_host_ms"], res["native_dev_ms"] = timed(lambda: native.stage({"p4": raw}), args.iters, args.warmup)
            res["torch_host_ms"], res["torch_dev_ms"] = timed(torch_path, args.iters, args.warmup)
            res["speedup_dev"] = res["torch_dev_ms"] / res["native_dev_ms"]
            print(json.dumps(r4(res)), flush=True)
        enc, dec = G._models(N, (3, 3, 4, 4), (4, 4, 3, 3), dev, seed=0)
        res = {"what": "eval_step", "B": B, "N": N}
        for key, kw in (("plain", {}), ("normalize", dict(normalize=True, normalize_method=args.method))):
            ev = NativeEvalStep(enc, dec, B, **kw)
            ev.load_batch({"p4": raw})
            res[f"{key}_host_ms"], res[f"{key}_dev_ms"] = timed(ev.run, args.iters, args.warmup)
        print(json.dumps(r4(res)), flush=True)


if __name__ == "__main__":
    main()
