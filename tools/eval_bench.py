#!/usr/bin/env python3
"""Evaluation step (lgn_step_eval_f64 / NativeEvalStep, HIP graph) next to the training step (NativeTrainStep) and the module-API
evaluation loop under no_grad (ModuleEvalStep): jets/s at cfg2 (512 x 30, maxdim 2), cfg5 (512 x 30, maxdim 3) and cfg2's network
at 64 jets.  One JSON line per configuration.      python tools/eval_bench.py [--steps K] [--warmup W] [--configs cfg2,cfg5,cfg2_b64]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "lgn-autoencoder_amd"))
import torch  # noqa: E402

CONFIGS = {"cfg2": (512, 30, (3, 3, 4, 4), (4, 4, 3, 3), 2), "cfg5": (512, 30, (4, 4, 6, 6), (6, 6, 4, 4), 3),
           "cfg2_b64": (64, 30, (3, 3, 4, 4), (4, 4, 3, 3), 2)}


def per_call_ms(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--configs", default="cfg2,cfg5,cfg2_b64")
    args = ap.parse_args()
    import bench
    import __graft_entry__ as G
    from lgn.step import ModuleEvalStep, NativeEvalStep, NativeTrainStep
    dev = torch.device("cuda:0")
    for name in args.configs.split(","):
        B, N, ce, cd, maxdim = CONFIGS[name]
        p4, labels = bench.synthetic_jets(B, N, seed=5)
        batch = {"p4": p4.to(dev), "labels": labels.to(dev)}
        opts = dict(get_real_method="real", chamfer_jet_features=False)
        res = {"config": name, "B": B, "N": N, "maxdim": maxdim}
        enc, dec = G._models(N, ce, cd, dev, seed=0, maxdim=maxdim)
        ev = NativeEvalStep(enc, dec, B, **opts)
        ev.load_batch(batch)
        res["eval_ms"] = per_call_ms(ev.run, args.steps, args.warmup)
        mod = ModuleEvalStep(enc, dec, B, **opts)
        res["module_eval_ms"] = per_call_ms(lambda: mod.run(batch), max(5, args.steps // 5), 3)
        tr = NativeTrainStep(enc, dec, B, **opts)
        tr.load_batch(batch)
        res["train_ms"] = per_call_ms(tr.step, args.steps, args.warmup)
        for k in ("eval", "module_eval", "train"):
            res[f"{k}_jets_per_s"] = B / (res[f"{k}_ms"] * 1e-3)
        res["eval_over_train"] = res["eval_ms"] / res["train_ms"]
        res["eval_workspace_mb"] = ev.workspace.numel() * 8 / 2**20
        res["train_workspace_mb"] = tr.workspace.numel() * 8 / 2**20
        print(json.dumps({k: (round(v, 4) if isinstance(v, float) else v) for k, v in res.items()}), flush=True)


if __name__ == "__main__":
    main()
