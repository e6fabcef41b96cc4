#!/usr/bin/env python3
"""Training step per --loss-choice: NativeTrainStep (HIP graph) with chamfer (twice: the second run gives the spread of repeated
runs of the same code), mse and hungarian in its four frames, next to the route a user had before the native loss stage -- the
module API with the assignment solved on the host (encoder -> decoder -> costs copied to the host -> linear_sum_assignment per jet ->
gather -> MSE -> backward -> two Adam optimisers), with scipy if importable, else the restatement of tests/_anomaly_ref.py.  One
process, the variants interleaved over several rounds; ms per step, one JSON line per configuration.
    python tools/loss_bench.py [--steps K] [--warmup W] [--rounds R] [--configs cfg2,cfg2_b64] [--out profiles/loss_bench.jsonl] [--commit ID]"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "lgn-autoencoder_amd")); sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402

CONFIGS = {"cfg2": (512, 30, (3, 3, 4, 4), (4, 4, 3, 3), 2), "cfg2_b64": (64, 30, (3, 3, 4, 4), (4, 4, 3, 3), 2)}
FRAMES = {"abs_cart": (True, False), "abs_polar": (True, True), "rel_polar": (False, True), "rel_cart": (False, False)}


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


class HostAssignmentStep:
    """The reference's loop with its HungarianMSELoss (absolute Cartesian frame): cdist on the device, assignment on the host."""

    def __init__(self, enc, dec, lr=5e-4):
        try:
            from scipy.optimize import linear_sum_assignment
            self.solver, self.lsa = "scipy", lambda c: linear_sum_assignment(c)[1]
        except ImportError:
            import _anomaly_ref
            self.solver, self.lsa = "_anomaly_ref.lsap", _anomaly_ref.lsap
        self.enc, self.dec = enc, dec
        self.opts = [torch.optim.Adam(enc.parameters(), lr), torch.optim.Adam(dec.parameters(), lr)]

    def step(self, batch):
        x = self.dec(self.enc(batch))[0]
        t = batch["p4"]
        cost = torch.cdist(x, t).cpu().detach().numpy()
        col = torch.as_tensor([list(self.lsa(c)) for c in cost], device=x.device)
        loss = torch.nn.functional.mse_loss(torch.gather(x, 1, col.unsqueeze(-1).expand_as(x)), t)
        for o in self.opts:
            o.zero_grad()
        loss.backward()
        for o in self.opts:
            o.step()
        return loss


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--configs", default="cfg2,cfg2_b64")
    ap.add_argument("--out", default=None)
    ap.add_argument("--commit", default=os.environ.get("LGN_BENCH_COMMIT"), help="commit the numbers are taken on, where git cannot tell")
    args = ap.parse_args()
    import bench
    import __graft_entry__ as G
    from lgn.step import NativeTrainStep
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
        variants = {"chamfer": {}, "chamfer_again": {}, "mse": dict(loss_choice="mse")}
        for f, (a, p) in FRAMES.items():
            variants[f"hungarian_{f}"] = dict(loss_choice="hungarian", hungarian_abs_coord=a, hungarian_polar_coord=p)
        steps = {}
        for v, kw in variants.items():
            enc, dec = G._models(N, ce, cd, dev, seed=0, maxdim=maxdim)
            steps[v] = NativeTrainStep(enc, dec, B, get_real_method="real", **kw)
            steps[v].load_batch(batch)
        ms = {v: [] for v in steps}
        for _ in range(args.rounds):                       # interleaved: drift of the clocks hits every variant alike
            for v, s in steps.items():
                ms[v].append(per_call_ms(s.step, args.steps, args.warmup))
        enc, dec = G._models(N, ce, cd, dev, seed=0, maxdim=maxdim)
        host = HostAssignmentStep(enc, dec)
        host_ms = per_call_ms(lambda: host.step(batch), max(5, args.steps // 20), 2)
        res = {"config": name, "B": B, "N": N, "commit": commit, "steps": args.steps, "rounds": args.rounds}
        for v in steps:
            res[f"{v}_ms"] = min(ms[v])
            res[f"{v}_ms_rounds"] = [round(x, 4) for x in ms[v]]
        res["module_host_assignment_ms"], res["host_solver"] = host_ms, host.solver
        res["host_over_native_hungarian"] = host_ms / res["hungarian_abs_cart_ms"]
        line = json.dumps({k: (round(v, 4) if isinstance(v, float) else v) for k, v in res.items()})
        print(line, flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
