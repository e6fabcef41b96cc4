#!/usr/bin/env python3
"""An epoch of cfg2's training step over a device-resident dataset, three ways, wall-clock per step (the epoch ends synchronised):
  (a) loop_item   the loop a user writes around the step: index the resident tensors per batch, step.step(batch), loss.item()
  (b) loop        the same loop without .item() (one synchronisation at the end)
  (c) runner      lgn.epoch.EpochRunner: one graph replay per batch (gather staging | step | collect), one synchronisation
next to (s) the bare step on a staged batch -- what bench.py times.  512 and 64 jets per batch at 30 particles, with and without
normalize; every epoch uses a fresh shuffle.  One JSON line per configuration, the median over the timed epochs.
    python tools/epoch_bench.py [--steps K] [--epochs E] [--warmup W]"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "lgn-autoencoder_amd"))
import torch  # noqa: E402

N_PART, CH_ENC, CH_DEC = 30, (3, 3, 4, 4), (4, 4, 3, 3)        # cfg2


def timed_epochs(variants, epochs, warmup):
    """{name: median wall-clock seconds of fn()} -- every fn returns synchronised -- over `epochs` rounds after `warmup` rounds; a
    round runs every variant once, so that they alternate and share whatever else the machine is doing."""
    ts = {name: [] for name, _ in variants}
    for r in range(warmup + epochs):
        for name, fn in variants:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            if r >= warmup:
                ts[name].append(time.perf_counter() - t0)
    return {name: statistics.median(v) for name, v in ts.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=64, help="batches per epoch")
    ap.add_argument("--epochs", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    import bench
    import __graft_entry__ as G
    from lgn.epoch import DeviceDataset, EpochRunner
    from lgn.step import NativeTrainStep
    dev = torch.device("cuda:0")
    for B in (512, 64):
        for normalize in (False, True):
            M = B * args.steps
            p4, labels = bench.synthetic_jets(M, N_PART, seed=5)
            if normalize:
                p4 = p4 * 37.0
            p4, labels = p4.to(dev), labels.to(dev)
            enc, dec = G._models(N_PART, CH_ENC, CH_DEC, dev, seed=0)
            step = NativeTrainStep(enc, dec, batch_size=B, lr=5e-4, l1_lambda=1e-8, normalize=normalize)
            gen = torch.Generator().manual_seed(1)

            def loop(item):
                idx = torch.randperm(M, generator=gen).to(dev)
                total = 0.0
                for i in range(args.steps):
                    rows = idx[i * B:(i + 1) * B]
                    loss, _ = step.step({"p4": p4[rows], "labels": labels[rows]})
                    if item:
                        total += loss.item()
                torch.cuda.synchronize()
                return total

            runner = EpochRunner(step, DeviceDataset({"p4": p4, "labels": labels}, shuffle=False), shuffle=True, generator=gen)

            def bare():
                for _ in range(args.steps):
                    step.step()
                torch.cuda.synchronize()

            res = {"what": "train_epoch", "B": B, "N": N_PART, "normalize": normalize, "steps": args.steps, "epochs": args.epochs}
            variants = (("loop_item", lambda: loop(True)), ("loop", lambda: loop(False)), ("runner", runner.run_epoch), ("bare_step", bare))
            for key, t in timed_epochs(variants, args.epochs, args.warmup).items():
                res[f"{key}_ms_per_step"] = t / args.steps * 1e3
            res["launches_per_epoch"] = runner.launches_per_epoch
            res["runner_over_loop_item"] = res["runner_ms_per_step"] / res["loop_item_ms_per_step"]
            res["runner_over_loop"] = res["runner_ms_per_step"] / res["loop_ms_per_step"]
            res["runner_minus_bare_ms"] = res["runner_ms_per_step"] - res["bare_step_ms_per_step"]
            print(json.dumps({k: (round(v, 4) if isinstance(v, float) else v) for k, v in res.items()}), flush=True)


if __name__ == "__main__":
    main()
