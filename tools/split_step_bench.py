#!/usr/bin/env python3
"""The split whole-step calls on table-driven networks next to the route such a configuration had before them: cfg5's networks
(maxdim 3, (4,4,6,6)/(6,6,4,4)) with jet_features -- NativeTrainStep(table_split=True) (twice: the second run gives the spread of
repeated runs of the same code) against CapturedModuleStep, and NativeEvalStep(table_split=True) (twice) against ModuleEvalStep.
One process, the variants interleaved over several rounds; ms per step and kernel launches per step (the device kernels of one step,
counted by torch.profiler; null where the profiler gives none), one JSON line per configuration.
    python tools/split_step_bench.py [--steps K] [--warmup W] [--rounds R] [--configs cfg5_jet,cfg5_jet_b64]
                                     [--out profiles/table_split_bench.jsonl] [--commit ID]"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "lgn-autoencoder_amd"))
import torch  # noqa: E402

CONFIGS = {"cfg5_jet": (512, 30, (4, 4, 6, 6), (6, 6, 4, 4), 3), "cfg5_jet_b64": (64, 30, (4, 4, 6, 6), (6, 6, 4, 4), 3)}


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


def kernel_launches(fn):
    """Device kernels of one call of fn (a graph replay reports the kernels of its nodes); None where the profiler reports none."""
    try:
        from torch.profiler import ProfilerActivity, profile
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        n = sum(1 for e in prof.events() if str(getattr(e, "device_type", "")).endswith("CUDA") and "memcpy" not in e.name.lower()
                and "memset" not in e.name.lower())
        return n or None
    except Exception:      # noqa: BLE001
        return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--configs", default="cfg5_jet,cfg5_jet_b64")
    ap.add_argument("--out", default=None)
    ap.add_argument("--commit", default=os.environ.get("LGN_BENCH_COMMIT"), help="commit the numbers are taken on, where git cannot tell")
    args = ap.parse_args()
    import bench
    import __graft_entry__ as G
    from lgn.step import CapturedModuleStep, ModuleEvalStep, NativeEvalStep, NativeTrainStep
    dev = torch.device("cuda:0")
    commit = args.commit
    try:
        commit = commit or subprocess.check_output(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], stderr=subprocess.DEVNULL).decode().strip()
    except Exception:      # noqa: BLE001
        commit = commit or "unknown"
    for name in args.configs.split(","):
        B, N, ce, cd, maxdim = CONFIGS[name]
        p4, labels = bench.synthetic_jets(B, N, seed=5)
        batch = {"p4": p4.to(dev), "labels": labels.to(dev)}

        def nets():
            return G._models(N, ce, cd, dev, seed=0, maxdim=maxdim, jet_features=True)

        train = {"native_split": NativeTrainStep(*nets(), B, get_real_method="real", table_split=True),
                 "native_split_again": NativeTrainStep(*nets(), B, get_real_method="real", table_split=True),
                 "captured_module": CapturedModuleStep(*nets(), B, get_real_method="real")}
        calls = {}
        for v, s in train.items():
            s.load_batch(batch)
            s.step()                                           # (captures)
            calls[f"train_{v}"] = s.step
        evals = {"native_split": NativeEvalStep(*nets(), B, table_split=True), "native_split_again": NativeEvalStep(*nets(), B, table_split=True)}
        for v, s in evals.items():
            s.load_batch(batch)
            s.run()
            calls[f"eval_{v}"] = s.run
        module_eval = ModuleEvalStep(*nets(), B)
        calls["eval_module"] = lambda: module_eval.run(batch)
        ms = {v: [] for v in calls}
        for _ in range(args.rounds):                       # interleaved: drift of the clocks hits every variant alike
            for v, fn in calls.items():
                ms[v].append(per_call_ms(fn, args.steps, args.warmup))
        res = {"config": name, "B": B, "N": N, "jet_features": True, "commit": commit, "steps": args.steps, "rounds": args.rounds}
        for v, fn in calls.items():
            res[f"{v}_ms"] = min(ms[v])
            res[f"{v}_ms_rounds"] = [round(x, 4) for x in ms[v]]
            res[f"{v}_launches"] = kernel_launches(fn)
        res["train_spread_ms"] = abs(res["train_native_split_ms"] - res["train_native_split_again_ms"])
        res["train_captured_over_native"] = res["train_captured_module_ms"] / res["train_native_split_ms"]
        res["eval_module_over_native"] = res["eval_module_ms"] / res["eval_native_split_ms"]
        line = json.dumps({k: (round(v, 4) if isinstance(v, float) else v) for k, v in res.items()})
        print(line, flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
