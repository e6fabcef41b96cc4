#!/usr/bin/env python3
"""Native anomaly scores (lgn.anomaly.score_tensor, one launch) in jets/s: N = 30 (65,536 jets, 20 real particles) and N = 150
(8,192 jets, 100 real), with all 21 scores and with the six Hungarian variants masked off; and the standalone batched assignment
(lgn.anomaly.linear_sum_assignment's kernel) on random normal costs.  Each case runs in a child process of its own under
`timeout -k 10`; the first failure ends the run.  One JSON line per case.
    python tools/anomaly_bench.py [--steps K] [--warmup W] [--cases n30,n30_noh,n150,n150_noh,lsa30,lsa150]"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "lgn-autoencoder_amd"))

CASES = {"n30": (65536, 30, 20, True), "n30_noh": (65536, 30, 20, False), "n150": (8192, 150, 100, True),
         "n150_noh": (8192, 150, 100, False), "lsa30": (65536, 30, 0, None), "lsa150": (8192, 150, 0, None)}


def per_call_ms(fn, steps, warmup):
    import torch
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


def one(name, steps, warmup):
    import torch
    from lgn import _native as N
    from lgn import anomaly as A
    B, n, real, hung = CASES[name]
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(1)
    res = {"case": name, "B": B, "N": n}
    if hung is None:
        cost = torch.randn(B, n, n, device=dev, dtype=torch.float64, generator=g)
        col = torch.empty(B, n, device=dev, dtype=torch.int32)
        st = torch.empty(B, device=dev, dtype=torch.int32)

        def fn():
            N._check(N.lib().lgn_linear_sum_assignment_f64(N.ptr(cost), B, n, N.ptr(col), N.ptr(st), N.stream_ptr()), "lsa")
        res["kind"] = "linear_sum_assignment"
    else:
        t = torch.randn(B, n, 4, device=dev, dtype=torch.float64, generator=g)
        t[..., 0] = t[..., 1:].norm(dim=-1) + 0.1
        t[:, real:] = 0.0
        r = t + 0.2 * torch.randn(B, n, 4, device=dev, dtype=torch.float64, generator=g)
        norm = lambda x: x / (x.abs().amax(-2, keepdim=True) + 1e-16)
        xs = [r, t, norm(r), norm(t)]
        fn = lambda: A.score_tensor(*xs, hungarian=hung)
        res["kind"] = "scores" if hung else "scores, no Hungarian"
        res["real_particles"] = real
    res["ms"] = per_call_ms(fn, steps, warmup)
    res["jets_per_s"] = B / (res["ms"] * 1e-3)
    print(json.dumps({k: (round(v, 4) if isinstance(v, float) else v) for k, v in res.items()}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--cases", default=",".join(CASES))
    ap.add_argument("--timeout", type=int, default=180, help="seconds per case")
    ap.add_argument("--one", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.one:
        return one(args.one, args.steps, args.warmup)
    for name in args.cases.split(","):
        cmd = ["timeout", "-k", "10", str(args.timeout), sys.executable, os.path.abspath(__file__), "--one", name,
               "--steps", str(args.steps), "--warmup", str(args.warmup)]
        rc = subprocess.run(cmd).returncode
        if rc != 0:
            print(json.dumps({"case": name, "error": f"exit status {rc}"}), flush=True)
            sys.exit(rc)


if __name__ == "__main__":
    main()
