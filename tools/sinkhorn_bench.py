#!/usr/bin/env python3
"""The Sinkhorn loss call next to the exact EMD call at cfg2 (512 jets x 30 particles), modelled on tools/emd_bench.py.  The batch is
a live reconstruction: the output of the cfg2 networks on bench.py's synthetic jets, against those jets.  Cases, each in a child
process of its own under `timeout -k 10` (the first failure ends the run), one JSON line each, printed and appended to
profiles/sinkhorn_bench.jsonl:
  call  lgn_emd_relative_opts_f64 with gradient (lgn.emd.emd_relative_grad: unchanged code, the baseline) against
        lgn_sinkhorn_relative_f64 with gradient at SinkhornLoss's defaults and at tol = 0 with max_iter 50 / 100 / 200, debias off and
        on; interleaved over three rounds, the fastest round, every round and the baseline's spread are reported, with the
        microseconds per iteration from the tol = 0 runs and the distribution of the iteration counts at the defaults
  step  one graph-replayed CapturedModuleStep with SinkhornLoss() next to the same step with EMDLoss()
    python tools/sinkhorn_bench.py [--steps K] [--warmup W] [--cases call,step] [--timeout S]"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "lgn-autoencoder_amd"))

ROUNDS = 3
OUT = os.path.join(ROOT, "profiles", "sinkhorn_bench.jsonl")
B, N, CE, CD = 512, 30, (3, 3, 4, 4), (4, 4, 3, 3)


def _emit(res):
    line = json.dumps({k: (float(f"{v:.5g}") if isinstance(v, float) else v) for k, v in res.items()})
    print(line, flush=True)
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with open(OUT, "a") as f:
        f.write(line + "\n")


def _ms(fn, steps, warmup):
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


def _live_batch(dev):
    import torch
    import bench
    import __graft_entry__ as G
    from lgn.step import get_real
    p4, labels = bench.synthetic_jets(B, N, seed=5)
    batch = {"p4": p4.to(dev), "labels": labels.to(dev)}
    enc, dec = G._models(N, CE, CD, dev, seed=0, maxdim=2)
    with torch.no_grad():
        recon = get_real(dec(enc(batch)), "real").contiguous()
    return batch, recon, batch["p4"].to(torch.float64).contiguous()


def one_call(steps, warmup):
    import torch
    from lgn import emd as M
    from lgn import sinkhorn as K
    from lgn.losses import SinkhornLoss
    dev = torch.device("cuda:0")
    _, recon, target = _live_batch(dev)
    d = SinkhornLoss()
    defaults = dict(max_iter=d.max_iter, tol=d.tol, debias=d.debias)
    variants = {"emd_exact": lambda: M.emd_relative_grad(recon, target),
                "sinkhorn_default": lambda: K.sinkhorn_relative_grad(recon, target, d.epsilon, **defaults)}
    for debias in (False, True):
        for it in (50, 100, 200):
            variants[f"tol0_{it}_{'debias' if debias else 'plain'}"] = \
                (lambda it=it, debias=debias: K.sinkhorn_relative_grad(recon, target, d.epsilon, max_iter=it, tol=0.0, debias=debias))
    ms = {k: [] for k in variants}
    for _ in range(ROUNDS):
        for k, fn in variants.items():
            ms[k].append(_ms(fn, steps, warmup))
    _, _, _, iters, err, status = K.sinkhorn_relative_grad(recon, target, d.epsilon, **defaults)
    it = iters.cpu().numpy()
    res = {"case": "call", "B": B, "N": N, "steps": steps, "rounds": ROUNDS, "epsilon": d.epsilon, **defaults,
           "iters_min": int(it.min()), "iters_median": float(sorted(it)[len(it) // 2]), "iters_max": int(it.max()),
           "iters_at_cap": int((it >= d.max_iter).sum()), "status_iter": int(((status & K.ITER) != 0).sum().item()),
           "status_other": int(((status & 3) != 0).sum().item()), "err_max_over_S": float(err.max().item()),
           "cost_in_lds": K.cost_in_lds(N, N)}
    for k in variants:
        res[f"{k}_ms"] = min(ms[k])
        res[f"{k}_ms_rounds"] = [round(x, 4) for x in ms[k]]
    res["emd_exact_spread_ms"] = max(ms["emd_exact"]) - min(ms["emd_exact"])
    for tag in ("plain", "debias"):
        res[f"us_per_iteration_{tag}"] = 1e3 * (res[f"tol0_200_{tag}_ms"] - res[f"tol0_50_{tag}_ms"]) / 150.0
    _emit(res)


def one_step(steps, warmup):
    import torch
    import __graft_entry__ as G
    from lgn.losses import EMDLoss, SinkhornLoss
    from lgn.step import CapturedModuleStep
    dev = torch.device("cuda:0")
    batch, _, _ = _live_batch(dev)
    losses = {"emd": EMDLoss(), "sinkhorn": SinkhornLoss()}
    runs = {}
    for k, loss in losses.items():
        enc, dec = G._models(N, CE, CD, dev, seed=0, maxdim=2)
        runs[k] = CapturedModuleStep(enc, dec, B, get_real_method="real", loss_choice=loss)
        runs[k].load_batch(batch)
    ms = {k: [] for k in runs}
    for _ in range(ROUNDS):
        for k, s in runs.items():
            ms[k].append(_ms(s.step, steps, warmup))
    res = {"case": "step", "kind": "CapturedModuleStep, graph replay", "B": B, "N": N, "steps": steps, "rounds": ROUNDS}
    for k in runs:
        res[f"{k}_ms"] = min(ms[k])
        res[f"{k}_ms_rounds"] = [round(x, 4) for x in ms[k]]
        res[f"{k}_loss"] = float(runs[k].loss_out[0].item())
    _emit(res)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--cases", default="call,step")
    ap.add_argument("--timeout", type=int, default=180, help="seconds per case")
    ap.add_argument("--one", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.one:
        {"call": one_call, "step": one_step}[a.one](a.steps, a.warmup)
        return 0
    for case in a.cases.split(","):
        rc = subprocess.run(["timeout", "-k", "10", str(a.timeout), sys.executable, os.path.abspath(__file__), "--one", case,
                             "--steps", str(a.steps), "--warmup", str(a.warmup)]).returncode
        if rc != 0:
            print(f"case {case} failed (exit status {rc}); nothing more is started", file=sys.stderr)
            return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())
