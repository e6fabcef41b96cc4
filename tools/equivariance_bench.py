#!/usr/bin/env python3
"""Wall time of the equivariance test: the Python harness (lgn.models.autotest.lgn_tests: one forward per angle, torch operations and
two .item() per irrep and layer) against the native one (lgn.equivariance.lgn_tests: batched transforms, one forward and one
reduction per chunk of angles), on the same modules and jets in the same process.  Models: the g1 (maxdim 2) and g2 (maxdim 3)
fixtures; one batch of the 6 jets of g8_harness.npz, or of B synthetic jets (oracle.synthetic_jets, padded).  Both calls end in a
device-to-host copy, so a host clock around them measures the whole test (26 boosts, 26 rotations, the permutation test).  After
`--warmup` runs of each, `--repeats` runs in alternation; median with minimum and maximum.  One JSON line per (model, batch).
    python tools/equivariance_bench.py [--tags g1 g2] [--batches 6 64] [--repeats 5] [--warmup 1] [--max-jets 512] [--native-only]
(--native-only: for a kernel trace, e.g. rocprofv3 --kernel-trace --stats -- python tools/equivariance_bench.py --native-only)"""
import argparse
import contextlib
import io
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "lgn-autoencoder_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

CASES = {"g1": ("g1_e2e_maxdim2.npz", 2), "g2": ("g2_e2e_maxdim3.npz", 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tags", nargs="+", default=["g1", "g2"], choices=list(CASES))
    ap.add_argument("--batches", nargs="+", type=int, default=[6, 64])
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--max-jets", type=int, default=512)
    ap.add_argument("--native-only", action="store_true")
    args = ap.parse_args()

    import torch
    import __graft_entry__ as G
    import _util as U
    from oracle import lgn_oracle as O
    from lgn.models.autotest import lgn_tests, lgn_tests_native
    if not torch.cuda.is_available():
        raise RuntimeError("equivariance_bench needs a GPU: a time taken elsewhere says nothing about it")
    dev = torch.device("cuda:0")
    h = U.load("g8_harness.npz")

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        with contextlib.redirect_stdout(io.StringIO()):
            res = fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0, res

    for tag in args.tags:
        name, maxdim = CASES[tag]
        z = U.load(name)
        m = U.meta(z)
        enc, dec = G._models(m["N"], m["ch_enc"], m["ch_dec"], dev, seed=m["seed"], maxdim=maxdim)
        enc.load_state_dict(U.params_from(z, "enc")); dec.load_state_dict(U.params_from(z, "dec"))
        for B in args.batches:
            if B == 6:
                p4, labels = torch.from_numpy(h[f"{tag}.p4"]), torch.from_numpy(h[f"{tag}.labels"])
            else:
                p4, labels = O.synthetic_jets(B, m["N"], seed=3, pad=True)
            loader = [{"p4": p4.clone(), "labels": labels.clone()}]
            ways = {"python": lambda: lgn_tests(None, enc, dec, loader, unit="TeV", irreps="all"),
                    "native": lambda: lgn_tests_native(None, enc, dec, loader, unit="TeV", irreps="all", max_jets=args.max_jets)}
            if args.native_only:
                del ways["python"]
            times = {k: [] for k in ways}
            for i in range(args.warmup + args.repeats):
                for k, fn in ways.items():
                    t, res = timed(fn)
                    if i >= args.warmup:
                        times[k].append(t)
            worst = max(max(d.values()) for d in res["rot_dev_output"])
            row = {"bench": "equivariance", "model": tag, "maxdim": maxdim, "B": B, "N": m["N"], "max_jets": args.max_jets,
                   "repeats": args.repeats, "warmup": args.warmup, "native_max_rot_dev_output": worst}
            for k, ts in times.items():
                row[f"{k}_s"] = {"median": statistics.median(ts), "min": min(ts), "max": max(ts)}
            if not args.native_only:
                row["python_over_native"] = row["python_s"]["median"] / row["native_s"]["median"]
            print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
