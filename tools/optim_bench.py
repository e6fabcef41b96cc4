#!/usr/bin/env python3
"""The optimiser variants of a step's tail, timed on the GPU.

  1. lgn_step_finalize_opt_f64 in isolation (n parameters, nB per-jet loss terms) for Adam / RMSprop, each without and with L2,
     against lgn_step_finalize_f64 on the same sizes: calls replayed from a HIP graph, ROUNDS rounds of REPS calls, the variants
     taking turns within every round; median and spread (min .. max) over the rounds.
  2. the cfg2 NativeTrainStep (512 jets x 30 particles, (3,3,4,4) / (4,4,3,3) channels) per option, graph-replayed, the variants
     again alternating within every round.

python tools/optim_bench.py [n] [nB] [--rounds R] [--reps K] [--steps S] [--json PATH]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "lgn-autoencoder_amd"))
import ctypes as C  # noqa: E402

import torch  # noqa: E402

from lgn import _native as Nn  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("n", nargs="?", type=int, default=63510)
ap.add_argument("nB", nargs="?", type=int, default=512)
ap.add_argument("--rounds", type=int, default=9)
ap.add_argument("--reps", type=int, default=2000)
ap.add_argument("--steps", type=int, default=300)
ap.add_argument("--json", default=None)
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("optim_bench: no GPU (a time measured anywhere else says nothing)")
dev = torch.device("cuda:0")
L, P = Nn.lib(), Nn.ptr


def timed(replay, count):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(count):
        replay()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / count          # us per replay


def rounds(variants, count):
    """{name: [us per call, one figure per round]}: in every round each variant is timed once, in turn."""
    out = {k: [] for k in variants}
    for _ in range(args.rounds):
        for k, replay in variants.items():
            out[k].append(timed(replay, count))
    return out


def summary(ts):
    return {"median_us": round(statistics.median(ts), 3), "min_us": round(min(ts), 3), "max_us": round(max(ts), 3)}


def captured(fn, inner=1):
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(3):
            fn()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(inner):
            fn()
    return g


KEEP = []          # the buffers the captured graphs point into


# ---- 1. the finalize call in isolation -------------------------------------------------------------------
def finalize_variant(kind, l2):
    n, nB = args.n, args.nB
    gen = torch.Generator(device=dev).manual_seed(1)
    w = torch.randn(n, device=dev, dtype=torch.float64, generator=gen)
    g = torch.randn(n, device=dev, dtype=torch.float64, generator=gen)
    m, v = torch.zeros_like(w), torch.zeros_like(w)
    lp = torch.rand(nB, device=dev, dtype=torch.float64, generator=gen)
    step = torch.zeros(1, device=dev, dtype=torch.int64)
    keep = [w, g, m, v, lp, step]
    if kind is None:
        out = torch.zeros(3 + Nn.FINALIZE_SCRATCH, device=dev, dtype=torch.float64)

        def fn():
            Nn._check(L.lgn_step_finalize_f64(P(w), P(g), n, P(lp), nB, 1e-8, P(m), P(v), P(step), 5e-4, 0.9, 0.999, 1e-8, 1, P(out),
                                              Nn.stream_ptr()), "finalize")
    else:
        out = torch.zeros(4 + Nn.FINALIZE_OPT_SCRATCH, device=dev, dtype=torch.float64)
        d = Nn.OptimDesc()
        d.kind, d.l1_lambda, d.l2_lambda, d.lr = kind, 1e-8, l2, 5e-4
        d.eps = 1e-8 if kind == Nn.OPT_ADAM else 1e-16
        d.beta1, d.beta2, d.alpha, d.momentum = 0.9, 0.999, 0.99, 0.9
        keep.append(d)

        def fn():
            Nn._check(L.lgn_step_finalize_opt_f64(P(w), P(g), n, P(lp), nB, C.byref(d), P(m), P(v), P(step), 1, P(out), Nn.stream_ptr()),
                      "finalize_opt")
    INNER = 20                                          # calls per graph: the graph launch itself is not what is compared
    graph = captured(fn, INNER)
    KEEP.append(keep + [out])
    return graph, INNER


result = {"n": args.n, "nB": args.nB, "rounds": args.rounds}
fin = {"adam (lgn_step_finalize_f64)": finalize_variant(None, 0.0), "adam, descriptor": finalize_variant(Nn.OPT_ADAM, 0.0),
       "adam + L2": finalize_variant(Nn.OPT_ADAM, 1e-6), "rmsprop": finalize_variant(Nn.OPT_RMSPROP, 0.0),
       "rmsprop + L2": finalize_variant(Nn.OPT_RMSPROP, 1e-6)}
inner = next(iter(fin.values()))[1]
ts = rounds({k: g.replay for k, (g, _) in fin.items()}, max(1, args.reps // inner))
result["finalize"] = {k: summary([t / inner for t in v]) for k, v in ts.items()}
print(f"finalize call, n={args.n} nB={args.nB}, us per call: median (min .. max) over {args.rounds} rounds")
for k, s in result["finalize"].items():
    print(f"  {k:32s} {s['median_us']:8.2f}  ({s['min_us']:.2f} .. {s['max_us']:.2f})")

# ---- 2. the cfg2 training step per option --------------------------------------------------------------------
import __graft_entry__ as G  # noqa: E402
from lgn.step import NativeTrainStep  # noqa: E402
from oracle import lgn_oracle as O  # noqa: E402

B, N = 512, 30
p4, labels = O.synthetic_jets(B, N, seed=3, pad=True)
batch = {"p4": p4.to(dev), "labels": labels.to(dev)}
options = {"adam (default)": {}, "adam + L2": dict(l2_lambda=1e-6), "rmsprop": dict(optimizer_choice="rmsprop"),
           "rmsprop + L2": dict(optimizer_choice="rmsprop", l2_lambda=1e-6), "rmsprop, momentum 0": dict(optimizer_choice="rmsprop", momentum=0.0)}
steps = {}
for k, kw in options.items():
    enc, dec = G._models(N, (3, 3, 4, 4), (4, 4, 3, 3), dev)
    st = NativeTrainStep(enc, dec, batch_size=B, use_graph=True, **kw)
    st.load_batch(batch)
    for _ in range(5):
        st.step()
    torch.cuda.synchronize()
    assert st.launches_per_step == 1
    steps[k] = st
ts = rounds({k: st._g1.replay for k, st in steps.items()}, args.steps)
result["cfg2_step"] = {k: summary(v) for k, v in ts.items()}
print(f"cfg2 NativeTrainStep ({B} x {N}), us per graph-replayed step: median (min .. max) over {args.rounds} rounds of {args.steps} steps")
for k, s in result["cfg2_step"].items():
    print(f"  {k:32s} {s['median_us']:8.2f}  ({s['min_us']:.2f} .. {s['max_us']:.2f})")
print(json.dumps(result))
if args.json:
    os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
    with open(args.json, "w") as fh:
        json.dump(result, fh, indent=1)
