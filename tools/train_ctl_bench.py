#!/usr/bin/env python3
"""What the guarded training step costs, timed on the GPU.

Workloads: cfg2 (512 jets x 30 particles, (3,3,4,4) / (4,4,3,3) channels) and 64 x 30.  Variants, each built TWICE (the spread of a
repeated variant is the noise floor the differences are read against):
  default        NativeTrainStep as it is without the new keywords: one fused tail launch
  ctl_off        the guarded form with every control off (forced): reduce-only tail + gradient/decision launch + update launch
  ctl_on         max_grad_norm + skip_nonfinite + blow_up_threshold + warm-up/cosine schedule
One process, the variants taking turns within each of ROUNDS rounds of STEPS graph-replayed steps; the best round per variant.

python tools/train_ctl_bench.py [--rounds 3] [--steps 200] [--jsonl profiles/train_ctl_bench.jsonl]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "lgn-autoencoder_amd"))

import torch  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--steps", type=int, default=200)
ap.add_argument("--jsonl", default=os.path.join(ROOT, "profiles", "train_ctl_bench.jsonl"))
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("train_ctl_bench: no GPU (a time measured anywhere else says nothing)")
dev = torch.device("cuda:0")

import __graft_entry__ as G  # noqa: E402
from lgn import step as S  # noqa: E402
from oracle import lgn_oracle as O  # noqa: E402


def timed(replay, count):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(count):
        replay()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / count          # us per replay


def build(B, N, variant):
    enc, dec = G._models(N, (3, 3, 4, 4), (4, 4, 3, 3), dev)
    kw = {}
    if variant == "ctl_on":
        # a threshold far above the gradient norm of this workload would never clip: 1.0 does, on most steps
        kw = dict(max_grad_norm=1.0, skip_nonfinite=True, blow_up_threshold=1e32,
                  lr_schedule=S.LRSchedule("cosine", 5e-4, warmup_steps=100, total_steps=100000, min_lr=1e-5))
    S._OptimState._force_ctl = variant == "ctl_off"
    try:
        st = S.NativeTrainStep(enc, dec, batch_size=B, use_graph=True, **kw)
    finally:
        S._OptimState._force_ctl = False
    assert st.opt_state.ctl_form == (variant != "default")
    p4, labels = O.synthetic_jets(B, N, seed=3, pad=True)
    st.load_batch({"p4": p4.to(dev), "labels": labels.to(dev)})
    for _ in range(5):
        st.step()
    torch.cuda.synchronize()
    assert st.launches_per_step == 1
    return st


records = []
for name, (B, N) in (("cfg2", (512, 30)), ("64x30", (64, 30))):
    steps = {f"{v}#{k}": build(B, N, v) for k in (1, 2) for v in ("default", "ctl_off", "ctl_on")}
    times = {k: [] for k in steps}
    for _ in range(args.rounds):
        for k, st in steps.items():
            times[k].append(timed(st._g1.replay, args.steps))
    best = {k: min(v) for k, v in times.items()}
    print(f"{name} ({B} x {N}): us per graph-replayed step, best of {args.rounds} rounds of {args.steps} steps (all rounds)")
    for k in steps:
        print(f"  {k:12s} {best[k]:9.2f}   ({', '.join(f'{t:.2f}' for t in times[k])})")
    for v in ("default", "ctl_off", "ctl_on"):
        a, b = best[f"{v}#1"], best[f"{v}#2"]
        rec = {"workload": name, "B": B, "N": N, "variant": v, "best_us": [round(a, 3), round(b, 3)], "repeat_spread_us": round(abs(a - b), 3),
               "rounds_us": {k: [round(t, 3) for t in times[f"{v}#{k}"]] for k in (1, 2)}, "rounds": args.rounds, "steps": args.steps}
        if v != "default":
            rec["over_default_us"] = round(min(a, b) - min(best["default#1"], best["default#2"]), 3)
            stats = steps[f"{v}#1"].control_stats()
            rec["applied"], rec["clipped"], rec["skipped"] = stats["applied"], stats["clipped"], stats["skipped"]
        records.append(rec)
    del steps
    torch.cuda.empty_cache()

os.makedirs(os.path.dirname(os.path.abspath(args.jsonl)), exist_ok=True)
with open(args.jsonl, "a") as fh:
    for rec in records:
        fh.write(json.dumps(rec) + "\n")
        print(json.dumps(rec))
