#!/usr/bin/env python3
"""The native EMD score (lgn.emd.emd_relative_tensor, one launch) in jets/s at the shapes of tools/anomaly_bench.py: N = 30 (65,536
jets, 20 real particles: the flow in LDS) and N = 150 (8,192 jets, 100 real: the flow in a workspace), timed with stream events; also
the largest number of augmentations any jet needed (the solver's cap is 16 per node).  Each case runs in a child process of its own
under `timeout -k 10`; the first failure ends the run.  One JSON line per case, printed and appended to profiles/emd_bench.jsonl.
The gradient cases (not run by default): n30_grad / n150_grad -- 4,096 jets, the forward-only launch (emd_relative_tensor) against
the GRAD launch (emd_relative_grad, reconstruction's gradient alone and with the target's), interleaved over three rounds, the
fastest round of each; step_cfg2 -- one graph-replayed CapturedModuleStep at cfg2 (512 x 30, maxdim 2) with lgn.losses.EMDLoss()
against the same step with the Chamfer loss; step_cfg2_native -- the same shape through NativeTrainStep(native_emd=True), whose loss
stage is the EMD (csrc/emd_loss.hip), against CapturedModuleStep with the same loss and against the Chamfer native step, with the
stage's LDS (--one step_cfg2_trace:<route>: that route's steps alone, eager, for a kernel trace of its launches).
The option-gradient cases (not run by default): n30_grad_opts / n150_grad_opts -- the same 4,096 jets under beta = 2, under norm and
under R = 0.8, beta = 2, norm, periodic phi: the gradient launch against the value-only launch under the same options, for the generic
form on the jets' (pT, eta, phi) events and for the relative form, with the default options timed in the same rounds as the control.
The pairs cases (not run by default): pairs_full -- lgn.emd.emds of 512 x 512 events of 30 particles (20 real; the jets of the cases
above as (pT, eta, phi) events), 262,144 pairs in one launch, against what there was before it for the same job: index_select the
pairs into two (P, 30, 3) tensors, then one emd() call, the gather and the solve timed apart; pairs_upper -- the symmetric form on
the same 512 events (130,816 pairs); pairs_full_n150 -- 64 x 64 events of 150 particles (100 real), the flow in the workspace.  Interleaved over five rounds; the fastest round, every round and the spread are reported, and
the results of the two ways are compared bit for bit.
The matrix-gradient cases (not run by default): pairs_grad_full -- forward + backward of lgn.emd.emds_differentiable on 64 x 64 events
of 30 particles (4,096 pairs, as the gradient cases) under a random upstream matrix: backward="rows" (the composition over emd_grad,
the control) against backward="native" with kept slabs and with keep_bytes=0; pairs_grad_upper -- the symmetric form on 91 events
(4,095 pairs); pairs_grad_full_n150 -- 64 x 64 events of 150 particles, the flow in the workspace.  Interleaved over three rounds;
the fastest round, every round and the spread are reported.
    python tools/emd_bench.py [--steps K] [--warmup W] [--cases n30,n150[,n30_grad,n150_grad,n30_grad_opts,n150_grad_opts,step_cfg2,step_cfg2_native,pairs_full,pairs_upper,pairs_full_n150,pairs_grad_full,pairs_grad_upper,pairs_grad_full_n150]]"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "lgn-autoencoder_amd"))

CASES = {"n30": (65536, 30, 20), "n150": (8192, 150, 100)}
GRAD_CASES = {"n30_grad": (4096, 30, 20), "n150_grad": (4096, 150, 100)}
GRAD_OPTS_CASES = {"n30_grad_opts": (4096, 30, 20), "n150_grad_opts": (4096, 150, 100)}
PAIRS_CASES = {"pairs_full": (512, 30, 20), "pairs_upper": (512, 30, 20), "pairs_full_n150": (64, 150, 100)}
PAIRS_GRAD_CASES = {"pairs_grad_full": (64, 30, 20), "pairs_grad_upper": (91, 30, 20), "pairs_grad_full_n150": (64, 150, 100)}
ROUNDS = 3
PAIRS_ROUNDS = 5
OUT = os.path.join(ROOT, "profiles", "emd_bench.jsonl")


def one(name, steps, warmup):
    import torch
    from lgn import emd as M
    B, n, real = CASES[name]
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(1)
    t = torch.randn(B, n, 4, device=dev, dtype=torch.float64, generator=g)
    t[..., 0] = t[..., 1:].norm(dim=-1) + 0.1
    t[:, real:] = 0.0
    r = t + 0.2 * torch.randn(B, n, 4, device=dev, dtype=torch.float64, generator=g)
    M.max_augmentations(reset=True)
    for _ in range(warmup):
        out, st = M.emd_relative_tensor(r, t, return_status=True)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        out, st = M.emd_relative_tensor(r, t, return_status=True)
    e1.record()
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1) / steps
    res = {"case": name, "kind": "emd (relative coordinates)", "B": B, "N": n, "real_particles": real, "flow_in_lds": M.flow_in_lds(n),
           "ms": ms, "jets_per_s": B / (ms * 1e-3), "max_augmentations": M.max_augmentations(), "aug_cap": 16 * (2 * n + 2),
           "status_nonzero": int((st != 0).sum().item()), "mean_emd": float(out.mean().item())}
    line = json.dumps({k: (round(v, 4) if isinstance(v, float) else v) for k, v in res.items()})
    print(line, flush=True)
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with open(OUT, "a") as f:
        f.write(line + "\n")


def _emit(res):
    line = json.dumps({k: (round(v, 4) if isinstance(v, float) else v) for k, v in res.items()})
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


def one_grad(name, steps, warmup):
    import torch
    from lgn import emd as M
    B, n, real = GRAD_CASES[name]
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(1)
    t = torch.randn(B, n, 4, device=dev, dtype=torch.float64, generator=g)
    t[..., 0] = t[..., 1:].norm(dim=-1) + 0.1
    t[:, real:] = 0.0
    r = t + 0.2 * torch.randn(B, n, 4, device=dev, dtype=torch.float64, generator=g)
    variants = {"forward": lambda: M.emd_relative_tensor(r, t, return_status=True), "grad": lambda: M.emd_relative_grad(r, t),
                "grad_both": lambda: M.emd_relative_grad(r, t, need_g_target=True)}
    ms = {k: [] for k in variants}
    for _ in range(ROUNDS):                                # interleaved: drift of the clocks hits every variant alike
        for k, fn in variants.items():
            ms[k].append(_ms(fn, steps, warmup))
    st = M.emd_relative_grad(r, t)[3]
    res = {"case": name, "kind": "emd gradient epilogue", "B": B, "N": n, "real_particles": real, "flow_in_lds": M.flow_in_lds(n),
           "steps": steps, "rounds": ROUNDS, "status_nonzero": int((st != 0).sum().item())}
    for k in variants:
        res[f"{k}_ms"] = min(ms[k])
        res[f"{k}_ms_rounds"] = [round(x, 4) for x in ms[k]]
    res["grad_over_forward"] = res["grad_ms"] / res["forward_ms"]
    res["grad_both_over_forward"] = res["grad_both_ms"] / res["forward_ms"]
    _emit(res)


OPTIONS = {"beta2": dict(beta=2.0), "norm": dict(norm=True), "all": dict(R=0.8, beta=2.0, norm=True, periodic_phi=True)}


def one_grad_opts(name, steps, warmup):
    """The gradients under the options against the value-only calls under the same options, on the jets of one_grad: the generic
    form on their (pT, eta, phi) events (emd_grad with the first event's gradient against emd(), whose pairs kernel is the value-only
    launch) and the relative form (emd_relative_grad against emd_relative_tensor), with the default options as the control."""
    import torch
    from lgn import emd as M
    B, n, real = GRAD_OPTS_CASES[name]
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(1)
    t = torch.randn(B, n, 4, device=dev, dtype=torch.float64, generator=g)
    t[..., 0] = t[..., 1:].norm(dim=-1) + 0.1
    t[:, real:] = 0.0
    r = t + 0.2 * torch.randn(B, n, 4, device=dev, dtype=torch.float64, generator=g)

    def events(x):
        pt = x[..., 1:3].norm(dim=-1)
        ev = torch.stack([pt, torch.asinh(x[..., 3] / pt), torch.atan2(x[..., 2], x[..., 1])], -1)
        ev[pt == 0] = 0.0                                  # (the target's zero padding)
        return ev.contiguous()
    er, et = events(r), events(t)
    variants = {"control_forward": lambda: M.emd_relative_tensor(r, t, return_status=True), "control_grad": lambda: M.emd_relative_grad(r, t)}
    for k, o in OPTIONS.items():
        variants[f"{k}_value"] = lambda o=o: M.emd(er, et, return_status=True, **o)
        variants[f"{k}_grad"] = lambda o=o: M.emd_grad(er, et, return_status=True, need_g1=False, **o)
        variants[f"{k}_rel_value"] = lambda o=o: M.emd_relative_tensor(r, t, return_status=True, **o)
        variants[f"{k}_rel_grad"] = lambda o=o: M.emd_relative_grad(r, t, **o)
    ms = {k: [] for k in variants}
    for _ in range(ROUNDS):                                # interleaved: drift of the clocks hits every variant alike
        for k, fn in variants.items():
            ms[k].append(_ms(fn, steps, warmup))
    bad = sum(int((M.emd_grad(er, et, return_status=True, **o)[3] != 0).sum().item()) +
              int((M.emd_relative_grad(r, t, **o)[3] != 0).sum().item()) for o in OPTIONS.values())
    res = {"case": name, "kind": "emd gradient epilogue under options", "B": B, "N": n, "real_particles": real,
           "flow_in_lds": M.flow_in_lds(n), "steps": steps, "rounds": ROUNDS, "status_nonzero": bad}
    for k in variants:
        res[f"{k}_ms"] = min(ms[k])
        res[f"{k}_spread"] = (max(ms[k]) - min(ms[k])) / min(ms[k])
    res["control_grad_over_forward"] = res["control_grad_ms"] / res["control_forward_ms"]
    for k in OPTIONS:
        res[f"{k}_grad_over_value"] = res[f"{k}_grad_ms"] / res[f"{k}_value_ms"]
        res[f"{k}_rel_grad_over_value"] = res[f"{k}_rel_grad_ms"] / res[f"{k}_rel_value_ms"]
    _emit(res)


def _events(B, n, real, seed, dev):
    """(B, n, 3) events of (pT, eta, phi) from the jet-like 4-vectors of the cases above, zero padded"""
    import torch
    g = torch.Generator(device=dev).manual_seed(seed)
    t = torch.randn(B, n, 4, device=dev, dtype=torch.float64, generator=g)
    pt = t[..., 1:3].norm(dim=-1)
    ev = torch.stack([pt, torch.asinh(t[..., 3] / pt), torch.atan2(t[..., 2], t[..., 1])], -1)
    ev[:, real:] = 0.0
    return ev


def one_pairs(name, steps, warmup):
    import torch
    from lgn import emd as M
    B, n, real = PAIRS_CASES[name]
    dev = torch.device("cuda:0")
    X0, X1 = _events(B, n, real, 1, dev), _events(B, n, real, 2, dev)
    upper = name == "pairs_upper"
    if upper:
        iu = torch.triu_indices(B, B, offset=1, device=dev)
        i, j, X1 = iu[0].contiguous(), iu[1].contiguous(), X0
    else:
        i, j = torch.arange(B, device=dev).repeat_interleave(B), torch.arange(B, device=dev).repeat(B)
    npairs = int(i.numel())
    gathered = [X0.index_select(0, i), X1.index_select(0, j)]

    def gather():
        gathered[0], gathered[1] = X0.index_select(0, i), X1.index_select(0, j)

    variants = {"emds": lambda: M.emds(X0, None if upper else X1, return_status=True), "gather": gather,
                "solve": lambda: M.emd(gathered[0], gathered[1], return_status=True)}
    ms = {k: [] for k in variants}
    for _ in range(PAIRS_ROUNDS):                          # interleaved: drift of the clocks hits every variant alike
        for k, fn in variants.items():
            ms[k].append(_ms(fn, steps, warmup))
    out, st = M.emds(X0, None if upper else X1, return_status=True)
    ref, ref_st = M.emd(gathered[0], gathered[1], return_status=True)
    same = bool(torch.equal(out[i, j].view(torch.int64), ref.view(torch.int64)) and torch.equal(st[i, j], ref_st))
    res = {"case": name, "kind": "emds, one launch, against gather + emd", "B0": B, "B1": B, "N": n, "real_particles": real, "pairs": npairs,
           "flow_in_lds": M.flow_in_lds(n), "steps": steps, "rounds": PAIRS_ROUNDS, "status_nonzero": int((st != 0).sum().item()),
           "same_bits_as_gather_and_emd": same}
    for k in variants:
        res[f"{k}_ms"] = min(ms[k])
        res[f"{k}_ms_rounds"] = [round(x, 4) for x in ms[k]]
        res[f"{k}_spread"] = (max(ms[k]) - min(ms[k])) / min(ms[k])
    res["emds_pairs_per_s"] = npairs / (res["emds_ms"] * 1e-3)
    res["solve_pairs_per_s"] = npairs / (res["solve_ms"] * 1e-3)
    res["emds_over_solve"] = res["emds_ms"] / res["solve_ms"]
    res["emds_over_gather_plus_solve"] = res["emds_ms"] / (res["gather_ms"] + res["solve_ms"])
    if os.environ.get("LGN_AMD_LIB"):
        res["library"] = os.path.basename(os.environ["LGN_AMD_LIB"])
    _emit(res)


def one_pairs_grad(name, steps, warmup):
    """Forward + backward of emds_differentiable under a random upstream matrix: the composition (backward="rows", the parent's code,
    unchanged) as the control against backward="native" with kept slabs and with keep_bytes=0.  The gradients of the variants are
    compared: native kept against native keep_bytes=0 bit for bit, native against the composition by the largest relative deviation."""
    import torch
    from lgn import emd as M
    B, n, real = PAIRS_GRAD_CASES[name]
    dev = torch.device("cuda:0")
    upper = name == "pairs_grad_upper"
    X0 = _events(B, n, real, 1, dev).requires_grad_(True)
    X1 = None if upper else _events(B, n, real, 2, dev).requires_grad_(True)
    npairs = B * (B - 1) // 2 if upper else B * B
    W = torch.randn(B, B, device=dev, dtype=torch.float64, generator=torch.Generator(device=dev).manual_seed(3))
    grads = {}

    def run(key, **kw):
        def fn():
            X0.grad = None
            if X1 is not None:
                X1.grad = None
            out = M.emds_differentiable(X0, X1, **kw)
            out.backward(W)
            grads[key] = (X0.grad, None if upper else X1.grad)
        return fn

    variants = {"rows": run("rows", backward="rows"), "native_kept": run("native_kept", backward="native"),
                "native_nokeep": run("native_nokeep", backward="native", keep_bytes=0)}
    ms = {k: [] for k in variants}
    for _ in range(ROUNDS):                                # interleaved: drift of the clocks hits every variant alike
        for k, fn in variants.items():
            ms[k].append(_ms(fn, steps, warmup))
    st = M.emds(X0.detach(), None if upper else X1.detach(), return_status=True)[1]
    same = all(b is None or bool(torch.equal(a, b)) for a, b in zip(grads["native_kept"], grads["native_nokeep"]))
    # (the particles with weight: at zero weight the distance has a kink in that weight, and the two orders of a pair, which the
    # composition's symmetric form solves, may return different subgradients there)
    dev_rows = max(float((a[:, :real] - b[:, :real]).abs().max() / b[:, :real].abs().max())
                   for a, b in zip(grads["native_kept"], grads["rows"]) if b is not None)
    res = {"case": name, "kind": "emds_differentiable forward + backward", "B0": B, "B1": B, "N": n, "real_particles": real,
           "pairs": npairs, "flow_in_lds": M.flow_in_lds(n), "steps": steps, "rounds": ROUNDS,
           "status_nonzero": int((st != 0).sum().item()), "kept_and_nokeep_same_bits": same, "native_against_rows_max_rel_weighted_particles": dev_rows}
    for k in variants:
        res[f"{k}_ms"] = min(ms[k])
        res[f"{k}_ms_rounds"] = [round(x, 4) for x in ms[k]]
        res[f"{k}_spread"] = (max(ms[k]) - min(ms[k])) / min(ms[k])
    res["native_kept_over_rows"] = res["native_kept_ms"] / res["rows_ms"]
    res["native_nokeep_over_rows"] = res["native_nokeep_ms"] / res["rows_ms"]
    _emit(res)


def one_step(steps, warmup):
    import torch
    import bench
    import __graft_entry__ as G
    from lgn.losses import EMDLoss
    from lgn.step import CapturedModuleStep
    B, N, ce, cd = 512, 30, (3, 3, 4, 4), (4, 4, 3, 3)
    dev = torch.device("cuda:0")
    p4, labels = bench.synthetic_jets(B, N, seed=5)
    batch = {"p4": p4.to(dev), "labels": labels.to(dev)}
    emd_loss = EMDLoss()
    runs = {}
    for k, loss in (("chamfer", "chamfer"), ("emd", emd_loss)):
        enc, dec = G._models(N, ce, cd, dev, seed=0, maxdim=2)
        runs[k] = CapturedModuleStep(enc, dec, B, get_real_method="real", loss_choice=loss)
        runs[k].load_batch(batch)
    ms = {k: [] for k in runs}
    for _ in range(ROUNDS):
        for k, s in runs.items():
            ms[k].append(_ms(s.step, steps, warmup))
    res = {"case": "step_cfg2", "kind": "CapturedModuleStep, graph replay", "B": B, "N": N, "steps": steps, "rounds": ROUNDS,
           "status_nonzero": int((emd_loss.status != 0).sum().item()), "emd_loss": float(runs["emd"].loss_out[0].item())}
    for k in runs:
        res[f"{k}_ms"] = min(ms[k])
        res[f"{k}_ms_rounds"] = [round(x, 4) for x in ms[k]]
    _emit(res)


def _native_routes(B, Np, cd):
    """the three routes of step_cfg2_native: name -> (encoder, decoder) -> step, and the loss modules by name"""
    from lgn.losses import EMDLoss
    from lgn.step import CapturedModuleStep, NativeTrainStep
    mods = {"native_emd": EMDLoss(), "captured_module_emd": EMDLoss()}
    make = {"native_emd": lambda e, d, **kw: NativeTrainStep(e, d, B, get_real_method="real", loss_choice=mods["native_emd"],
                                                              native_emd=True, **kw),
            "captured_module_emd": lambda e, d, **kw: CapturedModuleStep(e, d, B, get_real_method="real",
                                                                         loss_choice=mods["captured_module_emd"], **kw),
            "native_chamfer": lambda e, d, **kw: NativeTrainStep(e, d, B, get_real_method="real", **kw)}
    return make, mods


def one_step_trace(route, steps):
    """step_cfg2_trace:<route>: `steps` eager (uncaptured) steps of one route of step_cfg2_native on a staged batch and nothing else on
    the device, for a kernel trace of its launches:  rocprofv3 --kernel-trace --stats -d DIR -- python tools/emd_bench.py --one
    step_cfg2_trace:native_emd --steps 10  (the calls per kernel over `steps` are the launches per step)."""
    import torch
    import bench
    import __graft_entry__ as G
    B, Np, ce, cd = 512, 30, (3, 3, 4, 4), (4, 4, 3, 3)
    dev = torch.device("cuda:0")
    p4, labels = bench.synthetic_jets(B, Np, seed=5)
    enc, dec = G._models(Np, ce, cd, dev, seed=0, maxdim=2)
    step = _native_routes(B, Np, cd)[0][route](enc, dec, use_graph=False)
    step.load_batch({"p4": p4.to(dev), "labels": labels.to(dev)})
    torch.cuda.synchronize()
    for _ in range(steps):
        step.step()
    torch.cuda.synchronize()
    print(json.dumps({"case": f"step_cfg2_trace:{route}", "steps": steps, "loss": float(step.loss_out[0].item())}), flush=True)


def one_step_native(steps, warmup):
    """step_cfg2_native: the EMD loss as the loss stage of the native step (NativeTrainStep(native_emd=True)) against the module-API
    step captured into one graph (CapturedModuleStep) with the same loss, and the Chamfer native step, at cfg2 (512 x 30, fp64):
    interleaved over three rounds, every round reported."""
    import torch
    import bench
    import __graft_entry__ as G
    from lgn import _native as N
    B, Np, ce, cd = 512, 30, (3, 3, 4, 4), (4, 4, 3, 3)
    dev = torch.device("cuda:0")
    p4, labels = bench.synthetic_jets(B, Np, seed=5)
    batch = {"p4": p4.to(dev), "labels": labels.to(dev)}
    make, mods = _native_routes(B, Np, cd)
    runs = {}
    for k, fn in make.items():
        enc, dec = G._models(Np, ce, cd, dev, seed=0, maxdim=2)
        runs[k] = fn(enc, dec)
        runs[k].load_batch(batch)
    ms = {k: [] for k in runs}
    for _ in range(ROUNDS):
        for k, s in runs.items():
            ms[k].append(_ms(s.step, steps, warmup))
    res = {"case": "step_cfg2_native", "kind": "one training step, graph replay", "B": B, "N": Np, "steps": steps, "rounds": ROUNDS,
           "status_nonzero": {k: int((m.status != 0).sum().item()) for k, m in mods.items()},
           "loss": {k: float(s.loss_out[0].item()) for k, s in runs.items()},
           "stage_lds_bytes": int(N.lib().lgn_emd_loss_lds_bytes(Np, cd[-1]))}
    for k in runs:
        res[f"{k}_ms"] = min(ms[k])
        res[f"{k}_ms_rounds"] = [round(x, 4) for x in ms[k]]
        res[f"{k}_spread_ms"] = max(ms[k]) - min(ms[k])
    res["native_over_captured"] = res["native_emd_ms"] / res["captured_module_emd_ms"]
    _emit(res)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--cases", default=",".join(CASES))
    ap.add_argument("--timeout", type=int, default=180, help="seconds per case")
    ap.add_argument("--one", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.one == "step_cfg2":
        return one_step(args.steps, args.warmup)
    if args.one == "step_cfg2_native":
        return one_step_native(args.steps, args.warmup)
    if args.one and args.one.startswith("step_cfg2_trace:"):
        return one_step_trace(args.one.split(":", 1)[1], args.steps)
    if args.one in GRAD_CASES:
        return one_grad(args.one, args.steps, args.warmup)
    if args.one in GRAD_OPTS_CASES:
        return one_grad_opts(args.one, args.steps, args.warmup)
    if args.one in PAIRS_CASES:
        return one_pairs(args.one, args.steps, args.warmup)
    if args.one in PAIRS_GRAD_CASES:
        return one_pairs_grad(args.one, args.steps, args.warmup)
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
