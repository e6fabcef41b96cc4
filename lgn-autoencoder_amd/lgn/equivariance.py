"""
lgn.equivariance -- the Lorentz-group equivariance test (lgn/models/autotest/lgn_tests.py of the reference) on the native path:
the same call shapes, result keys and nesting as lgn.models.autotest.lgn_tests, which stays the restatement the reference pins.

Where that harness runs one forward per angle and a handful of torch operations and two ``.item()`` per irrep and layer, this one
  * builds the 26 Lorentz matrices R and every representation matrix D with the harness's own ``lorentz_D`` / ``cartesian_lorentz``
    on the host (26 x at most 5 matrices of at most 9 x 9) and uploads them in ONE copy per kind,
  * transforms the batch for a chunk of Tc angles at once (lgn_transform_jets_f64) and runs ONE forward of Tc * B jets
    (Tc * B <= max_jets) with ``covariance_test=True``,
  * reduces f(R x) - D(R) f(x) for the output GVec and every internal GVec, all irreps, all Tc angles in ONE call
    (lgn_rep_deviation_f64: b' = z conj(D) formed on chip, five numbers per (part, angle)) and copies them to the host once per chunk.
The three metrics of ``node_dev`` come from those five numbers on the host.  CPU tensors and a missing library raise; no fallback.
"""
import ctypes as C
import logging
import time
from math import cosh
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _native as N
from .models.autotest.lgn_tests import (REFERENCE_IRREPS, SEPARATOR, _angles, _avg, cartesian_lorentz, get_output, lorentz_D)

EQUI_TILE, EQUI_MAX_PARTS = N.EQUI_TILE, N.EQUI_MAX_PARTS
SUM_DIFF, SUM_B, MAX_DIFF, MAX_B, MAX_REL = range(5)        # the columns of rep_deviation's result
_EPS = 1e-16


def _need_cuda(*ts):
    for t in ts:
        if isinstance(t, torch.Tensor) and not t.is_cuda:
            raise RuntimeError("liblgn_amd.so operates on GPU tensors only (got a CPU tensor); there is no CPU fallback")


def _gpu_of(module) -> torch.device:
    dev = torch.device(module.device)
    if dev.type != "cuda":
        raise RuntimeError(f"the native equivariance test runs on GPU modules only (got one on {dev}); there is no CPU fallback")
    return dev


def _perm32(perm, B, n_particles, dev):
    if perm is None:
        return None
    _need_cuda(perm)
    if tuple(perm.shape) != (B, n_particles):
        raise ValueError(f"perm must have shape ({B}, {n_particles}); got {tuple(perm.shape)}")
    return perm.to(device=dev, dtype=torch.int32).contiguous()


def angle_chunks(B: int, T: int, max_jets: int) -> List[Tuple[int, int]]:
    """[t0, t1) ranges of the T transformations, Tc = max_jets // B of them per forward of Tc * B jets."""
    if B < 1 or T < 1:
        raise ValueError(f"angle_chunks: B = {B}, T = {T} (need both >= 1)")
    if max_jets < B:
        raise ValueError(f"max_jets = {max_jets} is smaller than the batch of {B} jets: not even one transformation fits a forward")
    tc = min(T, max_jets // B)
    return [(t0, min(T, t0 + tc)) for t0 in range(0, T, tc)]


def transform_jets(p4: torch.Tensor, R: torch.Tensor, perm: Optional[torch.Tensor] = None, scalars: Optional[torch.Tensor] = None):
    """lgn_transform_jets_f64 (include/lgn_amd.h): (T, B, N, 4) = p4[b, perm[b, n]] @ R[t] for p4 (B, N, 4) and R (T, 4, 4) or (4, 4).
    With ``scalars`` (B, N, K) returns (momenta, scalars gathered the same way as (T, B, N, K))."""
    _need_cuda(p4, R, perm, scalars)
    p4, R = N.f64(p4), N.f64(R)
    if R.dim() == 2:
        R = R.unsqueeze(0)
    if p4.dim() != 3 or p4.shape[-1] != 4 or R.dim() != 3 or tuple(R.shape[1:]) != (4, 4):
        raise ValueError(f"transform_jets takes p4 (B, N, 4) and R (T, 4, 4); got {tuple(p4.shape)} and {tuple(R.shape)}")
    T, (B, n) = int(R.shape[0]), (int(p4.shape[0]), int(p4.shape[1]))
    perm = _perm32(perm, B, n, p4.device)
    out = torch.empty(T, B, n, 4, device=p4.device, dtype=torch.float64)
    K, s_out = 0, None
    if scalars is not None:
        scalars = N.f64(scalars)
        if scalars.dim() != 3 or tuple(scalars.shape[:2]) != (B, n):
            raise ValueError(f"scalars must have shape ({B}, {n}, K); got {tuple(scalars.shape)}")
        K = int(scalars.shape[2])
        s_out = torch.empty(T, B, n, K, device=p4.device, dtype=torch.float64)
    rc = N.lib().lgn_transform_jets_f64(N.ptr(p4), N.ptr(R), N.ptr(perm), N.ptr(scalars) if K else None, T, B, n, K, N.ptr(out),
                                        N.ptr(s_out) if K else None, N.stream_ptr())
    if rc < 0:
        raise ValueError(N.last_error())
    N._check(rc, "lgn_transform_jets_f64")
    return out if scalars is None else (out, s_out)


def _int_array(xs):
    return (C.c_int * len(xs))(*xs)


def _ptr_array(ts):
    return (C.c_void_p * len(ts))(*[t.data_ptr() for t in ts])


def rep_deviation(a_parts: Sequence[torch.Tensor], b_parts: Sequence[torch.Tensor], D_parts: Sequence[torch.Tensor],
                  perm: Optional[torch.Tensor] = None) -> torch.Tensor:
    """lgn_rep_deviation_f64 (include/lgn_amd.h).  Part p: a (2, T * B, N, C, d) features of the transformed input (jet t * B + b),
    b (2, B, N, C, d) of the untransformed one, D (T, 2, d, d).  Returns the (parts, T, 5) device tensor of
    [sum(a - b'), sum(b'), max|a - b'|, max|b'|, max|(a - b') / (b' + 1e-16)|] with b' = rotate_rep(b); no host sync.  More than
    EQUI_MAX_PARTS parts go in several calls."""
    if not (len(a_parts) == len(b_parts) == len(D_parts)) or not a_parts:
        raise ValueError("rep_deviation takes three equally long, non-empty lists of parts")
    _need_cuda(perm, *a_parts, *b_parts, *D_parts)
    a_parts, b_parts, D_parts = ([N.f64(x) for x in xs] for xs in (a_parts, b_parts, D_parts))
    T, B = int(D_parts[0].shape[0]), int(b_parts[0].shape[1])
    ns, cs, ds = [], [], []
    for p, (a, b, D) in enumerate(zip(a_parts, b_parts, D_parts)):
        if b.dim() != 5 or b.shape[0] != 2 or b.shape[1] != B:
            raise ValueError(f"part {p}: b must be (2, {B}, N, C, d); got {tuple(b.shape)}")
        n, c, d = (int(x) for x in b.shape[2:])
        if d not in (1, 3, 4, 9):
            raise ValueError(f"part {p}: d = {d} is not the dimension of an irrep up to maxdim 3 (1, 3, 4 or 9)")
        if tuple(a.shape) != (2, T * B, n, c, d):
            raise ValueError(f"part {p}: a must be (2, T * B = {T * B}, {n}, {c}, {d}); got {tuple(a.shape)}")
        if tuple(D.shape) != (T, 2, d, d):
            raise ValueError(f"part {p}: D must be ({T}, 2, {d}, {d}); got {tuple(D.shape)}")
        ns.append(n), cs.append(c), ds.append(d)
    dev = b_parts[0].device
    if perm is not None:
        perm = _perm32(perm, B, ns[0], dev)
    lib = N.lib()
    stats = torch.empty(len(a_parts), T, 5, device=dev, dtype=torch.float64)
    for p0 in range(0, len(a_parts), EQUI_MAX_PARTS):
        p1 = min(len(a_parts), p0 + EQUI_MAX_PARTS)
        n_, c_, d_ = _int_array(ns[p0:p1]), _int_array(cs[p0:p1]), _int_array(ds[p0:p1])
        nbytes = lib.lgn_rep_deviation_workspace_bytes(p1 - p0, T, B, n_, c_, d_)
        if nbytes < 0:
            raise ValueError(N.last_error())
        work = torch.empty(nbytes // 8, device=dev, dtype=torch.float64)
        rc = lib.lgn_rep_deviation_f64(p1 - p0, T, B, _ptr_array(a_parts[p0:p1]), _ptr_array(b_parts[p0:p1]), _ptr_array(D_parts[p0:p1]),
                                       n_, c_, d_, N.ptr(perm), N.ptr(stats[p0:p1]), N.ptr(work), nbytes, N.stream_ptr())
        if rc < 0:
            raise ValueError(N.last_error())
        N._check(rc, "lgn_rep_deviation_f64")
    return stats


def _metric(row, numel: int, mode: str) -> float:
    """node_dev's three metrics from one (5,) row of rep_deviation over a block of `numel` numbers."""
    if mode == "max":
        return float(row[MAX_REL])
    if mode == "maxnorm":
        return float(row[MAX_DIFF] / (row[MAX_B] + _EPS))
    return float(abs((row[SUM_DIFF] / numel) / (row[SUM_B] / numel + _EPS)))


def _kind(test_type: str) -> str:
    kind = "boost" if test_type.lower().startswith("boost") else "rot"
    if kind == "rot" and not test_type.lower().startswith("rot"):
        raise ValueError(f"test_type must be one of 'boost' or 'rotation': {test_type}")
    return kind


@torch.no_grad()
def covariance_test(encoder, decoder, data, test_type, axis="z", alpha_max=None, cg_dict=None, unit="GeV", irreps=REFERENCE_IRREPS,
                    max_jets=512):
    """lgn.models.autotest.covariance_test with every angle of a chunk in one forward and one reduction (module docstring)."""
    kind = _kind(test_type)
    cg_dict = encoder.cg_dict if cg_dict is None else cg_dict
    dev, dtype = _gpu_of(encoder), encoder.dtype
    data = dict(data)
    data["p4"] = data["p4"].to(dev, dtype)
    if unit.lower() == "gev":
        data["p4"] = data["p4"] / 1e3
    if alpha_max is None:
        alpha_max = 10.0 if kind == "boost" else 2 * np.pi
    grid = np.arange(0, alpha_max + 0.01, step=alpha_max / 25.0)
    T, B = len(grid), int(data["p4"].shape[0])
    chunks = angle_chunks(B, T, int(max_jets))

    ref_out, ref_nodes = get_output(encoder, decoder, data)
    gvecs = [ref_out] + list(ref_nodes)
    # the parts of one reduction: (GVec, irrep); the output and the reference-shaped tables take the reference's two irreps
    every = irreps == "all"
    parts = [(g, w) for g, vec in enumerate(gvecs) for w in (list(vec.keys()) if every and g > 0 else REFERENCE_IRREPS)]
    b_parts = [gvecs[g][w].contiguous() for g, w in parts]
    numel = [b.numel() for b in b_parts]

    # every matrix of the kind on the host, one upload
    angs = [_angles(kind, value, axis) for value in grid]
    keys = sorted({w for _, w in parts})
    # (lorentz_D takes the coupling matrix of (k, 0) x (0, n) -> (k, n) to the host at every call: fetch each one once)
    cg_host = {((k, 0), (0, n)): {(k, n): cg_dict[((k, 0), (0, n))][(k, n)].detach().cpu()} for k, n in set(keys) | {(1, 1)}}
    host = [torch.stack([cartesian_lorentz(lorentz_D((1, 1), *ang, cg_host)) for ang in angs])]
    host += [torch.stack([lorentz_D(w, *ang, cg_host) for ang in angs]) for w in keys]
    flat = torch.cat([h.reshape(-1) for h in host]).to(dev)
    views, at = [], 0
    for h in host:
        views.append(flat[at:at + h.numel()].view(h.shape))
        at += h.numel()
    R, D = views[0], dict(zip(keys, views[1:]))

    batch_keys = [k for k in ("labels", "masks", "mask") if k in data]
    rows = []
    for t0, t1 in chunks:
        moved = {k: v for k, v in data.items() if k != "scalars"}
        if "scalars" in data:
            p4t, sct = transform_jets(data["p4"], R[t0:t1], scalars=data["scalars"].to(dev, dtype))
            moved["scalars"] = sct.view(-1, *sct.shape[2:])
        else:
            p4t = transform_jets(data["p4"], R[t0:t1])
        moved["p4"] = p4t.view(-1, *p4t.shape[2:])
        for k in batch_keys:
            moved[k] = data[k].repeat(t1 - t0, *([1] * (data[k].dim() - 1)))
        out_in, nodes_in = get_output(encoder, decoder, moved)
        moved_vecs = [out_in] + list(nodes_in)
        stats = rep_deviation([moved_vecs[g][w] for g, w in parts], b_parts, [D[w][t0:t1] for _, w in parts])
        rows.append(stats.cpu())                                               # the chunk's one device-to-host copy
    stats = torch.cat(rows, 1).numpy()                                         # (parts, T, 5)

    index = {gw: p for p, gw in enumerate(parts)}

    def table(t, g, ws, mode):
        return {w: _metric(stats[index[g, w], t], numel[index[g, w]], mode) for w in ws}

    layers = range(1, len(gvecs))
    dev_output = [table(t, 0, REFERENCE_IRREPS, "mean") for t in range(T)]
    dev_internal = [[table(t, g, REFERENCE_IRREPS, "mean") for g in layers] for t in range(T)]
    dev_all = [[table(t, g, list(gvecs[g].keys()), "maxnorm") for g in layers] for t in range(T)] if every else []
    extra = {f"{kind}_dev_internal_all": dev_all} if every else {}
    if kind == "boost":
        return {"gammas": [cosh(x) for x in grid], "boost_dev_output": dev_output, "boost_dev_internal": dev_internal, **extra}
    return {"thetas": grid, "rot_dev_output": dev_output, "rot_dev_internal": dev_internal, **extra}


@torch.no_grad()
def permutation_invariance_test(encoder, decoder, data, *ignore, generator=None):
    """lgn.models.autotest.permutation_invariance_test: the same permutation draw, the permuted batch from transform_jets, both
    deviations (invariance, 'equivariance') from rep_deviation with D the identity."""
    dev, dtype = _gpu_of(encoder), encoder.dtype
    mask = data["labels"] if "labels" in data else (data["p4"][..., 0] != 0).to(torch.uint8)
    B, n = mask.shape
    perm = torch.arange(n).expand(B, -1).clone()
    for b in range(B):
        k = int(mask[b].long().sum())
        perm[b, :k] = torch.randperm(k, generator=generator)
    assert (mask.cpu() == torch.gather(mask.cpu(), 1, perm)).all(), "the permutation must stay inside the real particles"
    perm_d = perm.to(device=dev, dtype=torch.int32)
    eye = torch.eye(4, device=dev, dtype=torch.float64)
    permuted = dict(data)
    if "scalars" in data:
        p4p, scp = transform_jets(data["p4"].to(dev, dtype), eye, perm_d, data["scalars"].to(dev, dtype))
        permuted["scalars"] = scp[0]
    else:
        p4p = transform_jets(data["p4"].to(dev, dtype), eye, perm_d)
    permuted["p4"] = p4p[0]
    out_p, _ = get_output(encoder, decoder, permuted)
    out_n, _ = get_output(encoder, decoder, dict(data))
    a_parts = [out_p[w].contiguous() for w in REFERENCE_IRREPS]
    b_parts = [out_n[w].contiguous() for w in REFERENCE_IRREPS]
    ident = []
    for b in b_parts:
        d = int(b.shape[-1])
        ident.append(torch.stack([torch.eye(d, device=dev, dtype=torch.float64), torch.zeros(d, d, device=dev, dtype=torch.float64)])[None])
    stats = torch.stack([rep_deviation(a_parts, b_parts, ident)[:, 0, MAX_REL],
                         rep_deviation(a_parts, b_parts, ident, perm=perm_d)[:, 0, MAX_REL]]).cpu().numpy()
    return ({w: float(stats[0, i]) for i, w in enumerate(REFERENCE_IRREPS)},
            {w: float(stats[1, i]) for i, w in enumerate(REFERENCE_IRREPS)})


@torch.no_grad()
def lgn_tests(args, encoder, decoder, dataloader, axis="z", alpha_max=None, theta_max=None, cg_dict=None, unit="GeV",
              irreps=REFERENCE_IRREPS, max_jets=512):
    """lgn.models.autotest.lgn_tests on the native path: the same averaging over batches, printed tables and returned dict (plain
    floats, dicts keyed by irrep tuples, the same list nesting), so ``plot_all_dev`` and ``check_equivariance`` take it unchanged."""
    t0 = time.time()
    logging.info("Covariance test begins...")
    encoder.eval(); decoder.eval()
    boosts, rots, pinv, pequi = [], [], [], []
    max_batches = getattr(args, "num_test_batch", -1) if args is not None else -1
    for idx, data in enumerate(dataloader):
        boosts.append(covariance_test(encoder, decoder, data, "boost", axis, alpha_max, cg_dict, unit, irreps, max_jets))
        rots.append(covariance_test(encoder, decoder, data, "rotation", axis, theta_max, cg_dict, unit, irreps, max_jets))
        a, b = permutation_invariance_test(encoder, decoder, data)
        pinv.append(a); pequi.append(b)
        if max_batches and max_batches > 0 and idx + 1 >= max_batches:
            break
    res = {"gammas": boosts[0]["gammas"], "thetas": rots[0]["thetas"]}
    for name, runs in (("boost", boosts), ("rot", rots)):
        n_alpha = len(runs[0][f"{name}_dev_output"])
        res[f"{name}_dev_output"] = [_avg([r[f"{name}_dev_output"][i] for r in runs]) for i in range(n_alpha)]
        n_layers = len(runs[0][f"{name}_dev_internal"][0])
        for table in (f"{name}_dev_internal", f"{name}_dev_internal_all"):
            if table in runs[0]:
                res[table] = [[_avg([r[table][i][l] for r in runs]) for l in range(n_layers)] for i in range(n_alpha)]
    res["perm_invariance_dev_output"] = _avg(pinv)
    res["perm_equivariance_dev_output"] = _avg(pequi)
    print(f"Covariance test completed! Time taken: {round((time.time() - t0) / 60, 2)} min")
    for title, xs, devs, xname in (("Boost", res["gammas"], res["boost_dev_output"], "gamma"),
                                   ("Rotation", res["thetas"], res["rot_dev_output"], "theta")):
        print(SEPARATOR)
        print(f"{title} equivariance test result (output relative error)")
        print(f"{xname:>12s} {'(0,0)':>12s} {'(1,1)':>12s}")
        for x, d in zip(xs, devs):
            print(f"{x:12.4g} {d[(0, 0)]:12.3e} {d[(1, 1)]:12.3e}")
    print(SEPARATOR)
    print(f"Permutation invariance test result: {res['perm_invariance_dev_output']}")
    print(f"Permutation equivariance test result: {res['perm_equivariance_dev_output']}")
    print(SEPARATOR)
    return res
