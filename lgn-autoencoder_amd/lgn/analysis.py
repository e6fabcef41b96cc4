"""
Reconstruction analysis on the GPU: the numeric half of the reference's ``plot_p`` (utils/jet_analysis/utils.py,
particle_recon_err.py, jet_recon_err.py) -- particle features in polar and relative-polar coordinates, jet features, the matched
relative errors of ``get_rel_err_find_match`` (two scipy-exact assignments per jet), the jet relative errors, the histograms the
plots are drawn from, ``get_stats`` with the ``err_dict`` JSON the plots dump, the median +- 4 IQR histogram ranges and the jet
images (csrc/stats.hip).  Only the drawing itself (matplotlib) stays with the reference.

One HIP kernel launch per chunk of jets (csrc/analysis.hip, C ABI ``lgn_recon_analysis_f64``) and one clear + one count launch per
histogram call (``lgn_histogram_f64``).  There is no CPU fallback.  Deliberate differences from the reference: the
assignment costs are the exact Euclidean distances (torch.cdist's matrix-product formula past 25 points is not), and everything is
computed in fp64 whatever the input dtype.
"""
import ctypes as C
from typing import Dict, Optional, Sequence

import numpy as np
import torch

from . import _native as N

NMAX = N.ASSIGN_NMAX
DEFAULT_CHUNK = 65536
FRAMES = ("cartesian", "polar", "polarrel")


def _device() -> torch.device:
    if not torch.cuda.is_available():
        raise RuntimeError("lgn.analysis needs a GPU (liblgn_amd.so); there is no CPU fallback")
    return torch.device("cuda", torch.cuda.current_device())


def _launch(target, recons, abs_coord, find_match, out):
    B, n = int(target.shape[0]), int(target.shape[1])
    if B == 0:
        return
    g = lambda k: N.ptr(out[k]) if k in out else None
    rc = N.lib().lgn_recon_analysis_f64(N.ptr(target), N.ptr(recons), B, n, int(bool(abs_coord)), int(bool(find_match)),
                                        g("part_polar"), g("part_polarrel") if abs_coord else None, g("jet_cart"), g("jet_polar"),
                                        g("jet_rel_err"), g("jet_keep"), g("rel_err"), g("col4row"), g("is_padded"), g("status"),
                                        N.stream_ptr())
    N._check(rc, "lgn_recon_analysis_f64")


def _alloc(B, n, dev, abs_coord, residuals, particles):
    f64 = dict(device=dev, dtype=torch.float64)
    out = {"jet_cart": torch.empty(2, B, 4, **f64), "jet_polar": torch.empty(2, B, 4, **f64), "jet_rel_err": torch.empty(2, B, 4, **f64),
           "jet_keep": torch.empty(2, B, device=dev, dtype=torch.uint8)}
    if particles:
        out["part_polar"] = torch.empty(2, B, n, 3, **f64)
        if abs_coord:
            out["part_polarrel"] = torch.empty(2, B, n, 3, **f64)
    if residuals:
        out["rel_err"] = torch.empty(3, B, n, 3, **f64)
        out["col4row"] = torch.empty(2, B, n, device=dev, dtype=torch.int32)
        out["is_padded"] = torch.empty(B, n, device=dev, dtype=torch.uint8)
        out["status"] = torch.empty(B, device=dev, dtype=torch.int32)
    return out


_JET_AXIS = {"target": 0, "recons": 0, "jet_cart": 1, "jet_polar": 1, "jet_rel_err": 1, "jet_keep": 1, "part_polar": 1, "part_polarrel": 1, "rel_err": 1,
             "col4row": 1, "is_padded": 0, "status": 0}


def recon_analysis(target: torch.Tensor, recons: torch.Tensor, abs_coord: bool = True, find_match: bool = True,
                   batch_size: int = DEFAULT_CHUNK, residuals: bool = True, particles: bool = True) -> Dict[str, torch.Tensor]:
    """Every array of lgn_recon_analysis_f64 (include/lgn_amd.h) as device tensors, named as the header names them; index 0 of a
    leading 2 is the target, 1 the reconstruction:
      part_polar (2, B, N, 3), part_polarrel (2, B, N, 3) (part_polar itself without abs_coord), jet_cart, jet_polar, jet_rel_err
      (2, B, 4), jet_keep (2, B) bool, rel_err (3, B, N, 3), col4row (2, B, N) int32, is_padded (B, N) bool, status (B,) int32,
      and the fp64 device inputs themselves as target, recons (B, N, 4) (particle_histograms reads them).
    target, recons: (B, N, 4) Cartesian (E, px, py, pz), CPU or device tensors of any float dtype (computed in fp64).  CPU inputs
    travel in chunks of batch_size jets through pinned buffers; device inputs cause no host sync, so the call chains after
    NativeEvalStep.run().  A jet whose assignment cost holds NaN gets status 1 (256: infeasible), col4row -1 and NaN rel_err; nothing
    is raised.  residuals=False skips the two assignments and rel_err / col4row / is_padded / status, particles=False the
    per-particle frames."""
    if target.dim() != 3 or target.shape[-1] != 4 or recons.shape != target.shape:
        raise ValueError(f"recon_analysis takes two (B, N, 4) Cartesian 4-vector tensors; got {tuple(target.shape)} and {tuple(recons.shape)}")
    B, n = int(target.shape[0]), int(target.shape[1])
    if not 1 <= n <= NMAX:
        raise ValueError(f"recon_analysis supports 1 <= N <= {NMAX} particles per jet; got N = {n}")
    dev = _device()
    chunk = int(batch_size) if batch_size is not None and batch_size > 0 else DEFAULT_CHUNK
    chunk = max(1, min(chunk, max(B, 1)))
    xs = (target, recons)
    on_host = [not x.is_cuda for x in xs]
    pinned = [torch.empty(chunk, n, 4, dtype=torch.float64).pin_memory() if h else None for h in on_host]
    staged = [torch.empty(chunk, n, 4, device=dev, dtype=torch.float64) if h else None for h in on_host]
    parts, copied = [], None
    for b0 in range(0, max(B, 1), chunk):
        m = min(chunk, B - b0)
        if copied is not None:
            copied.synchronize()           # the pinned buffers are free again
        part = []
        for x, h, pin, st in zip(xs, on_host, pinned, staged):
            if h:
                pin[:m].copy_(x[b0:b0 + m])
                st[:m].copy_(pin[:m], non_blocking=True)
                part.append(st[:m])
            else:
                part.append(N.f64(x[b0:b0 + m].detach().to(device=dev, dtype=torch.float64)))
        if any(on_host):
            copied = torch.cuda.Event()
            copied.record()
        out = _alloc(m, n, dev, abs_coord, residuals, particles)
        _launch(part[0], part[1], abs_coord, find_match, out)
        out["target"], out["recons"] = (x.clone() if h and B > chunk else x for x, h in zip(part, on_host))
        parts.append(out)
    out = parts[0] if len(parts) == 1 else {k: torch.cat([p[k] for p in parts], dim=_JET_AXIS[k]) for k in parts[0]}
    if particles and not abs_coord:
        out["part_polarrel"] = out["part_polar"]
    for k in ("jet_keep", "is_padded"):
        if k in out:
            out[k] = out[k].view(torch.bool)
    return out


class PackedEdges:
    """Edge arrays of a histogram call on the device: .device (cols, max_edges) fp64, .n_edges the host list of their lengths."""

    def __init__(self, device: torch.Tensor, n_edges):
        self.device, self.n_edges = device, [int(n) for n in n_edges]


def pack_edges(edges, cols: Optional[int] = None) -> PackedEdges:
    """Copy edge arrays to the device once (histogram() does it per call otherwise; under graph capture it must be done before).
    edges: one 1-d array shared by `cols` columns, or a sequence of 1-d arrays, one per column."""
    dev = _device()
    if isinstance(edges, (np.ndarray, torch.Tensor)) and edges.ndim == 1:
        edges = [edges] * (cols or 1)
    es = [np.ascontiguousarray(e.detach().cpu().numpy() if isinstance(e, torch.Tensor) else e, dtype=np.float64) for e in edges]
    if any(e.ndim != 1 for e in es):
        raise ValueError("histogram needs one 1-d edge array per column")
    max_edges = max(2, max(len(e) for e in es))
    packed = np.zeros((len(es), max_edges))
    for c, e in enumerate(es):
        packed[c, :len(e)] = e
    return PackedEdges(torch.from_numpy(packed).to(dev), [len(e) for e in es])


def histogram(x: torch.Tensor, edges, keep: Optional[torch.Tensor] = None, weights: Optional[torch.Tensor] = None) -> torch.Tensor:
    """np.histogram(x[keep, c], bins=edges[c], weights=weights[keep])[0] for every column c of the device matrix x (rows, cols), in
    one call: a (cols, max_bins) device tensor, int64 (exact, reproducible) or with weights fp64 (summed in no fixed order); bins past
    a column's own are 0.  edges: one array of edges (shared by every column), a sequence of cols arrays of 2 .. 1025 non-decreasing
    edges each, or what pack_edges() made of either.  x may be a strided view whose rows are a fixed number of doubles apart and whose columns are adjacent, e.g.
    p4.view(-1, 4)[:, 1:]; nothing is copied then.  numpy's semantics exactly (bin i: edges[i] <= v < edges[i + 1], the last bin
    closed; NaN, +-inf and out-of-range values nowhere).  keep: (rows,) bool / uint8 device tensor."""
    dev = _device()
    if x.dim() == 1:
        x = x.unsqueeze(-1)
    if x.dim() != 2:
        raise ValueError(f"histogram takes a (rows, cols) matrix; got {tuple(x.shape)}")
    if x.dtype != torch.float64 or not x.is_cuda:
        x = x.detach().to(device=dev, dtype=torch.float64)
    rows, cols = int(x.shape[0]), int(x.shape[1])
    if not 1 <= cols <= N.HIST_MAX_COLS:
        raise ValueError(f"histogram takes 1 .. {N.HIST_MAX_COLS} columns per call; got {cols}")
    if (cols > 1 and x.stride(1) != 1) or (rows > 1 and x.stride(0) < cols):
        x = x.contiguous()
    ld = int(x.stride(0)) if rows > 1 else cols
    if not isinstance(edges, PackedEdges):
        edges = pack_edges(edges, cols)
    if len(edges.n_edges) != cols:
        raise ValueError(f"histogram needs one edge array per column ({cols}); got {len(edges.n_edges)}")
    n_edges = (C.c_int * cols)(*edges.n_edges)
    e_dev, max_edges = edges.device, int(edges.device.shape[1])
    if keep is not None:
        keep = keep.to(dev)
        keep = (keep.view(torch.uint8) if keep.dtype == torch.bool else keep.to(torch.uint8)).contiguous()
        if keep.shape != (rows,):
            raise ValueError(f"keep must have shape ({rows},); got {tuple(keep.shape)}")
    if weights is not None:
        weights = N.f64(weights.detach().to(device=dev, dtype=torch.float64))
        if weights.shape != (rows,):
            raise ValueError(f"weights must have shape ({rows},); got {tuple(weights.shape)}")
    out = torch.empty(cols, max_edges - 1, device=dev, dtype=torch.int64 if weights is None else torch.float64)
    rc = N.lib().lgn_histogram_f64(x.data_ptr() if rows else None, rows, ld, cols, N.ptr(e_dev), n_edges, max_edges, N.ptr(keep),
                                   N.ptr(weights), N.ptr(out) if weights is None else None, None if weights is None else N.ptr(out),
                                   max_edges - 1, N.stream_ptr())
    N._check(rc, "lgn_histogram_f64")
    return out


def particle_histograms(analysis: Dict[str, torch.Tensor], ranges: Dict[str, Sequence], cutoff: float = 1e-6) -> Dict[str, list]:
    """The histograms plot_p draws, over caller-given edges, from recon_analysis' output.  ranges maps a name to
    three edge arrays (one per component); names left out are not counted:
      "p_cartesian", "p_polar"            particle (px, py, pz) / (pt, eta, phi) of target and reconstruction, rows with |p3| > cutoff
                                          (get_p_cartesian / get_p_polar): -> [target counts, recons counts]
      "rel_err_cartesian" / "_polar" / "_polarrel"   the matched relative errors of the non-padded rows
      "padded_cartesian" / "_polar" / "_polarrel"    the reconstructed features of the padded rows
    Each count entry is a list of three int64 numpy arrays (len(edges) - 1 each).  recon_stats() chooses the edges from median +- 4 IQR
    on the device.  The keep masks are element-wise torch expressions on the device; the counting is native."""
    t, r = analysis["target"].reshape(-1, 4), analysis["recons"].reshape(-1, 4)

    def count(x, edges, keep):
        h = histogram(x, [np.asarray(e) for e in edges], keep=keep).cpu().numpy()
        return [h[c, :len(e) - 1].copy() for c, e in enumerate(edges)]

    out = {}
    sides = (t, r)
    if "p_cartesian" in ranges or "p_polar" in ranges:
        big = [torch.linalg.vector_norm(x[:, 1:], dim=-1) > cutoff for x in sides]
        if "p_cartesian" in ranges:
            out["p_cartesian"] = [count(x[:, 1:], ranges["p_cartesian"], k) for x, k in zip(sides, big)]
        if "p_polar" in ranges:
            out["p_polar"] = [count(analysis["part_polar"][s].reshape(-1, 3), ranges["p_polar"], big[s]) for s in range(2)]
    pad = analysis["is_padded"].reshape(-1) if "is_padded" in analysis else None
    feats = {"cartesian": lambda: r[:, 1:], "polar": lambda: analysis["part_polar"][1].reshape(-1, 3),
             "polarrel": lambda: analysis["part_polarrel"][1].reshape(-1, 3)}
    for f, frame in enumerate(FRAMES):
        if f"rel_err_{frame}" in ranges:
            out[f"rel_err_{frame}"] = count(analysis["rel_err"][f].reshape(-1, 3), ranges[f"rel_err_{frame}"], ~pad)
        if f"padded_{frame}" in ranges:
            out[f"padded_{frame}"] = count(feats[frame](), ranges[f"padded_{frame}"], pad)
    return out


# ---- drop-ins with the reference's signatures (utils/jet_analysis/utils.py, particle_recon_err.py) --------------------------------

def _as4(p: torch.Tensor) -> torch.Tensor:
    """(.., N, 3 or 4) -> (B, N, 4) with a zero energy column for 3-vectors (the frames never read it)."""
    if p.shape[-1] not in (3, 4):
        raise ValueError(f"Invalid error. p.shape[-1] should be either 3 or 4. Found: {p.shape[-1]}.")
    x = p.detach().to(torch.float64)
    if p.shape[-1] == 3:
        x = torch.cat((torch.zeros_like(x[..., :1]), x), dim=-1)
    return x.reshape((-1,) + tuple(x.shape[-2:])) if x.dim() != 3 else x


def _jets_only(p: torch.Tensor, key: str, side_shape):
    x = _as4(p if p.dim() >= 2 else p.unsqueeze(0))
    out = recon_analysis(x, x, residuals=False, particles=key.startswith("part"))[key][0]
    return out.reshape(side_shape).to(device=p.device, dtype=p.dtype if p.dtype.is_floating_point else torch.float64)


def get_p_polar_tensor(p: torch.Tensor, eps: float = 1e-16) -> torch.Tensor:
    """(E, px, py, pz) or (px, py, pz) -> (pt, eta, phi), get_p_polar_tensor of the reference (eps is its default 1e-16 only).
    Element-wise on the last axis, for any leading shape, a flattened (B * N, 3) included: every row goes as a jet of its own."""
    if eps != 1e-16:
        raise NotImplementedError("the native frames use the reference's default eps = 1e-16")
    if p.shape[-1] not in (3, 4):
        raise ValueError(f"Invalid error. p.shape[-1] should be either 3 or 4. Found: {p.shape[-1]}.")
    return _jets_only(p.reshape(-1, 1, p.shape[-1]), "part_polar", tuple(p.shape[:-1]) + (3,))


def get_p_polarrel_tensor(p: torch.Tensor, eps: float = 1e-16) -> torch.Tensor:
    """(E, px, py, pz) -> (pt / Pt, Eta - eta, wrapped Phi - phi) relative to the summed jet: the sum runs over axis -2, as in the
    reference, so the input is (.., N, 3 or 4) with N <= 192 particles per jet (a 2-d input is ONE jet)."""
    if eps != 1e-16:
        raise NotImplementedError("the native frames use the reference's default eps = 1e-16")
    return _jets_only(p, "part_polarrel", tuple(p.shape[:-1]) + (3,))


def get_jet_feature_cartesian(p4: torch.Tensor, gpu: bool = True, return_arr: bool = False):
    """Jet (m, px, py, pz) as CPU tensors (stacked on the last axis with return_arr), get_jet_feature_cartesian of the reference."""
    f = _jets_only(p4, "jet_cart", tuple(p4.shape[:-2]) + (4,)).cpu()
    return f if return_arr else tuple(f.unbind(-1))


def get_jet_feature_polar(p4: torch.Tensor, gpu: bool = True, eps: float = 1e-16, return_arr: bool = False):
    """Jet (m, pt, eta, phi) as numpy arrays (stacked with return_arr), get_jet_feature_polar of the reference for torch input."""
    if eps != 1e-16:
        raise NotImplementedError("the native frames use the reference's default eps = 1e-16")
    f = _jets_only(p4, "jet_polar", tuple(p4.shape[:-2]) + (4,)).cpu().numpy()
    return f if return_arr else tuple(f[..., i] for i in range(4))


def get_rel_err_find_match(p_target_cartesian, p_recons_cartesian, p_target_polar, p_recons_polar, p_target_polarrel,
                           p_recons_polarrel, gpu: bool = True):
    """get_rel_err_find_match of particle_recon_err.py on given frames (B, N, 3): the two assignments and the three gathers run
    natively (lgn_match_rel_err_f64 is the same kernel fed with frames).  Returns three (B * N, 3) CPU tensors.  Raises ValueError,
    worded as scipy words it, when a cost holds NaN or is infeasible."""
    frames = [x.detach().to(device=_device(), dtype=torch.float64).contiguous() for x in
              (p_target_cartesian, p_recons_cartesian, p_target_polar, p_recons_polar, p_target_polarrel, p_recons_polarrel)]
    B, n = int(frames[0].shape[0]), int(frames[0].shape[1])
    if any(f.shape != (B, n, 3) for f in frames):
        raise ValueError("get_rel_err_find_match takes six (B, N, 3) tensors")
    if not 1 <= n <= NMAX:
        raise ValueError(f"get_rel_err_find_match supports 1 <= N <= {NMAX} particles per jet; got N = {n}")
    dev = frames[0].device
    rel = torch.empty(3, B, n, 3, device=dev, dtype=torch.float64)
    pad = torch.empty(B, n, device=dev, dtype=torch.uint8)
    status = torch.empty(B, device=dev, dtype=torch.int32)
    rc = N.lib().lgn_match_rel_err_f64(*(N.ptr(f) for f in frames), B, n, N.ptr(rel), None, N.ptr(pad), N.ptr(status), N.stream_ptr())
    N._check(rc, "lgn_match_rel_err_f64")
    st = status.cpu().numpy()
    bad = np.flatnonzero(st)
    if len(bad):
        what = "matrix contains invalid numeric entries" if int(st[bad[0]]) & 0xFF else "cost matrix is infeasible"
        raise ValueError(f"{what} (jet {int(bad[0])}, {len(bad)} jet(s) in all)")
    dt = p_target_cartesian.dtype
    return tuple(rel[f].reshape(-1, 3).cpu().to(dt) for f in range(3))


# ---- reconstruction statistics: get_stats, the err_dict JSON of plot_p, jet images (csrc/stats.hip) ---------------------------------

STAT_NAMES = N.STAT_NAMES
REFERENCE_STAT_KEYS = STAT_NAMES[:17]       # the keys of the reference's get_stats dict, in its order
NUM_BINS = 81                               # utils/jet_analysis/utils.py
_NONE_IF_NAN = ("mean", "std_dev", "skew", "kurtosis")
_NONE_IF_EMPTY = ("max", "min", "abs_min")


def _need_cuda(*ts):
    for t in ts:
        if isinstance(t, torch.Tensor) and not t.is_cuda:
            raise RuntimeError("liblgn_amd.so operates on GPU tensors only (got a CPU tensor); there is no CPU fallback")


def _as_mask(mask, rows, dev):
    if mask is None:
        return None
    _need_cuda(mask)
    mask = (mask.view(torch.uint8) if mask.dtype == torch.bool else mask.to(torch.uint8)).contiguous()
    if mask.shape != (rows,):
        raise ValueError(f"mask must have shape ({rows},); got {tuple(mask.shape)}")
    return mask


def _matrix(x):
    """(rows, cols) fp64 device view with adjacent columns, and its leading dimension."""
    _need_cuda(x)
    if x.dim() == 1:
        x = x.unsqueeze(-1)
    if x.dim() != 2:
        raise ValueError(f"a (rows, cols) matrix is needed; got {tuple(x.shape)}")
    if x.dtype != torch.float64:
        x = x.detach().to(torch.float64)
    rows, cols = int(x.shape[0]), int(x.shape[1])
    if (cols > 1 and x.stride(1) != 1) or (rows > 1 and x.stride(0) < cols):
        x = x.contiguous()
    return x, (int(x.stride(0)) if rows > 1 else cols)


def column_stats(x: torch.Tensor, mask: Optional[torch.Tensor] = None, mask_keep: bool = True, alpha: float = 4.0,
                 num_edges: int = 0) -> Dict[str, torch.Tensor]:
    """lgn_column_stats_f64 (include/lgn_amd.h) on the columns of the device matrix x (rows, cols <= 16), over the rows with
    bool(mask[r]) == mask_keep: {"stats": (cols, len(STAT_NAMES)) fp64, "edges": (cols, num_edges) fp64 =
    linspace(median - alpha IQR, median + alpha IQR, num_edges), "kept": (cols,) int64, "status": (cols,) int32}, all on the device;
    no host sync.  x may be a strided view with adjacent columns, as histogram() takes it."""
    x, ld = _matrix(x)
    dev = x.device
    rows, cols = int(x.shape[0]), int(x.shape[1])
    mask = _as_mask(mask, rows, dev)
    lib = N.lib()
    nbytes = lib.lgn_column_stats_workspace_bytes(rows, cols)
    if nbytes < 0:
        raise ValueError(N.last_error())
    out = {"stats": torch.empty(cols, N.STATS_COUNT, device=dev, dtype=torch.float64),
           "edges": torch.empty(cols, int(num_edges), device=dev, dtype=torch.float64),
           "kept": torch.empty(cols, device=dev, dtype=torch.int64), "status": torch.empty(cols, device=dev, dtype=torch.int32)}
    work = torch.empty(nbytes // 8, device=dev, dtype=torch.int64)
    rc = lib.lgn_column_stats_f64(x.data_ptr() if rows else None, rows, ld, cols, N.ptr(mask), int(bool(mask_keep)), float(alpha),
                                  int(num_edges), N.ptr(out["stats"]), N.ptr(out["edges"]) if num_edges else None, N.ptr(out["kept"]),
                                  N.ptr(out["status"]), N.ptr(work), nbytes, N.stream_ptr())
    if rc < 0:
        raise ValueError(N.last_error())
    N._check(rc, "lgn_column_stats_f64")
    return out


def hist_fwhm(counts: torch.Tensor, edges: PackedEdges) -> torch.Tensor:
    """find_fwhm of the reference on what histogram() returned for these edges: (cols,) fp64 on the device."""
    _need_cuda(counts)
    if counts.dtype != torch.int64 or counts.dim() != 2:
        raise ValueError("hist_fwhm takes the (cols, max_bins) int64 counts of histogram()")
    cols = int(counts.shape[0])
    out = torch.empty(cols, device=counts.device, dtype=torch.float64)
    n_edges = (C.c_int * cols)(*edges.n_edges)
    rc = N.lib().lgn_hist_fwhm_f64(N.ptr(counts), int(counts.shape[1]), N.ptr(edges.device), int(edges.device.shape[1]), n_edges, cols,
                                   N.ptr(out), N.stream_ptr())
    if rc < 0:
        raise ValueError(N.last_error())
    N._check(rc, "lgn_hist_fwhm_f64")
    return out


def stats_dict(row, fwhm: float, kept: int) -> dict:
    """One column's statistics (a sequence of len(STAT_NAMES) numbers) as the reference's get_stats dict of Python floats: its keys in
    its order, None where it gives None (a NaN mean, std_dev, skew or kurtosis; max, min and abs_min of an empty column)."""
    d = {}
    for i, name in enumerate(REFERENCE_STAT_KEYS):
        v = float(fwhm) if name == "FWHM" else float(row[i])
        if (name in _NONE_IF_NAN and v != v) or (name in _NONE_IF_EMPTY and kept == 0):
            v = None
        d[name] = v
    return d


def get_stats(res: torch.Tensor, bins) -> dict:
    """get_stats(res, bins) of utils/jet_analysis/utils.py for a 1-d device tensor: column statistics, np.histogram(res, bins) and
    find_fwhm in three native calls, one host copy at the end.  bins: a 1-d array of edges, on the device or the host."""
    _need_cuda(res)
    res = res.reshape(-1)
    cs = column_stats(res)
    if isinstance(bins, torch.Tensor) and bins.is_cuda:
        b = bins.detach().to(torch.float64).reshape(1, -1).contiguous()
        bins = PackedEdges(b, [b.shape[1]])
    else:
        bins = pack_edges(bins, 1)
    fw = hist_fwhm(histogram(res, bins), bins)
    flat = torch.cat((cs["stats"].reshape(-1), fw, cs["kept"].to(torch.float64))).cpu().numpy()
    return stats_dict(flat[:N.STATS_COUNT], flat[N.STATS_COUNT], int(flat[N.STATS_COUNT + 1]))


def _linspace(start: torch.Tensor, stop: torch.Tensor, num: int) -> torch.Tensor:
    """np.linspace(start[c], stop[c], num) per column on the device, rounded as numpy rounds it: arange * step + start, last = stop."""
    step = (stop - start) / (num - 1)
    e = torch.arange(num, device=start.device, dtype=torch.float64).unsqueeze(0) * step.unsqueeze(1)
    e = e + start.unsqueeze(1)
    e[:, -1] = stop
    return e


def recon_stats(analysis: Dict[str, torch.Tensor], abs_coord: bool = True, custom_ranges=None) -> dict:
    """The err_dict JSON of plot_particle_recon_err and plot_jet_recon_err from what recon_analysis returned, and the histograms the
    two draw: {"particle": {frame: {"rel_err": [3 dicts], "pad_recons": [3 dicts or none]}}, "jet": {"cartesian": [<= 4 dicts],
    "polar": [..]}, "hist": {name: {"counts": (cols, 80) int64, "edges": (cols, 81) fp64}}} with the hist entries device tensors over
    bins_suitable = linspace(median - 4 IQR, median + 4 IQR, 81).  Every statistic, edge and count is computed on the device; the one
    synchronisation is the copy of the statistics at the end.
    custom_ranges: None is custom_particle_recons_ranges=False.  Otherwise the `ranges` argument of plot_particle_recon_err -- per
    frame (real, padded), each three host arrays of edges -- which the reference then uses both as get_stats' FWHM bins and as the
    bins it draws: the six particle entries of "hist" are then counted over those edges ("edges": (3, longest) zero padded, and
    "n_edges": their lengths).  The jet plot's ranges are never custom here (custom_jet_recons_ranges=False).
    The reference's plot_p also takes a `cutoff`; neither error plot reads it (it only selects the particles of the feature
    histograms, which particle_histograms() counts), so this function has no such argument."""
    _need_cuda(analysis["rel_err"])
    dev = analysis["rel_err"].device
    pad = analysis["is_padded"].reshape(-1)
    r = analysis["recons"].reshape(-1, 4)
    feats = {"cartesian": r[:, 1:], "polar": analysis["part_polar"][1].reshape(-1, 3),
             "polarrel": (analysis["part_polarrel"] if abs_coord else analysis["part_polar"])[1].reshape(-1, 3)}
    jobs = []                                   # (group, x, mask, mask_keep, column statistics)
    for f, frame in enumerate(FRAMES):
        x = analysis["rel_err"][f].reshape(-1, 3)
        jobs.append((f"rel_err_{frame}", x, pad, False, column_stats(x, pad, False, 4.0, NUM_BINS)))
        jobs.append((f"padded_{frame}", feats[frame], pad, True, column_stats(feats[frame], pad, True, 4.0, NUM_BINS)))
    for s, system in enumerate(("cartesian", "polar")):
        x, keep = analysis["jet_rel_err"][s], analysis["jet_keep"][s]
        jobs.append((f"jet_{system}", x, keep, True, column_stats(x, keep, True, 4.0, NUM_BINS)))
    by_name = {j[0]: j for j in jobs}

    def min_max_bins(name):                     # get_min_max + np.linspace with its default of 50 points
        st = by_name[name][4]["stats"]
        med, iqr = st[:, 0], st[:, 1]
        return _linspace(med - 4.0 * iqr, med + 4.0 * iqr, 50)

    # particle_recon_err.py:355 -- get_bins takes the PADDED Cartesian range from the real Cartesian relative errors
    # particle_recon_err.py:373 -- and the REAL relative-polar range from the padded relative-polar features
    fwhm_source = {"rel_err_cartesian": "rel_err_cartesian", "padded_cartesian": "rel_err_cartesian", "rel_err_polar": "rel_err_polar",
                   "padded_polar": "padded_polar", "rel_err_polarrel": "padded_polarrel", "padded_polarrel": "padded_polarrel"}
    fw, hist = {}, {}
    for name, x, mask, keep_flag, cs in jobs:
        keep = mask if keep_flag else ~mask
        if name.startswith("jet_"):
            # jet_recon_err.py:168 -- get_bins indexes the first component's array: component k gets linspace(e, e, NUM_BINS) with e
            # the k-th kept jet's first relative error
            order = torch.cumsum(keep.to(torch.int64), 0)
            idx = torch.searchsorted(order, torch.arange(1, 5, device=dev)).clamp_(max=max(int(x.shape[0]) - 1, 0))
            e = x[idx, 0] if x.shape[0] else torch.full((4,), float("nan"), device=dev, dtype=torch.float64)
            bins = _linspace(e, e, NUM_BINS)
        elif custom_ranges is not None:
            f = FRAMES.index(name.split("_")[-1])
            bins = pack_edges([np.asarray(b) for b in custom_ranges[f][int(name.startswith("padded"))]])
        else:
            bins = PackedEdges(min_max_bins(fwhm_source[name]), [50] * 3)
        if not isinstance(bins, PackedEdges):
            bins = PackedEdges(bins.contiguous(), [bins.shape[1]] * bins.shape[0])
        counts = histogram(x, bins, keep=keep)
        fw[name] = hist_fwhm(counts, bins)
        if custom_ranges is not None and not name.startswith("jet_"):
            hist[name] = {"counts": counts, "edges": bins.device, "n_edges": bins.n_edges}
        else:
            own = PackedEdges(cs["edges"], [NUM_BINS] * int(cs["edges"].shape[0]))
            hist[name] = {"counts": histogram(x, own, keep=keep), "edges": cs["edges"]}

    flat = torch.cat([torch.cat((cs["stats"].reshape(-1), fw[name], cs["kept"].to(torch.float64))) for name, _, _, _, cs in jobs])
    flat = flat.cpu().numpy()                   # the one synchronisation
    dicts, o = {}, 0
    for name, x, _, _, _ in jobs:
        cols = int(x.shape[1])
        st = flat[o:o + cols * N.STATS_COUNT].reshape(cols, N.STATS_COUNT)
        f = flat[o + cols * N.STATS_COUNT:o + cols * (N.STATS_COUNT + 1)]
        kept = flat[o + cols * (N.STATS_COUNT + 1):o + cols * (N.STATS_COUNT + 2)]
        o += cols * (N.STATS_COUNT + 2)
        dicts[name] = [stats_dict(st[c], f[c], int(kept[c])) for c in range(cols)], int(kept[0])
    particle = {}
    for frame in FRAMES:
        padded, n_pad = dicts[f"padded_{frame}"]
        particle[frame] = {"rel_err": dicts[f"rel_err_{frame}"][0], "pad_recons": padded if n_pad else []}   # len(p) == 0: continue
    jet = {system: dicts[f"jet_{system}"][0][:min(4, dicts[f"jet_{system}"][1])] for system in ("cartesian", "polar")}
    return {"particle": particle, "jet": jet, "hist": hist}


def jet_image(jets: torch.Tensor, frame_jets: Optional[torch.Tensor] = None, mode: int = 0, npix: int = 24, maxR: float = 0.5,
              first_n: int = 0):
    """lgn_jet_images_f64 (include/lgn_amd.h): jets (B, N, 3) polar (pt, eta, phi) on the device -> (images (min(first_n, B), npix,
    npix), average (npix, npix)) device tensors.  mode 0: relative already; 1: each jet in its own frame; 2: in frame_jets' frame."""
    _need_cuda(jets, frame_jets)
    if jets.dim() != 3 or jets.shape[-1] != 3 or (frame_jets is not None and frame_jets.shape != jets.shape):
        raise ValueError(f"jet_image takes (B, N, 3) polar jets; got {tuple(jets.shape)}")
    jets = N.f64(jets.detach().to(torch.float64))
    frame_jets = None if frame_jets is None else N.f64(frame_jets.detach().to(torch.float64))
    B, n = int(jets.shape[0]), int(jets.shape[1])
    lib = N.lib()
    nbytes = lib.lgn_jet_images_workspace_bytes(B, int(npix))
    if nbytes < 0:
        raise ValueError(N.last_error())
    k = max(0, min(int(first_n), B))
    images = torch.empty(k, npix, npix, device=jets.device, dtype=torch.float64)
    average = torch.empty(npix, npix, device=jets.device, dtype=torch.float64)
    work = torch.empty(nbytes // 8, device=jets.device, dtype=torch.int64)
    rc = lib.lgn_jet_images_f64(N.ptr(jets), N.ptr(frame_jets), B, n, int(mode), int(npix), float(maxR), int(first_n),
                                N.ptr(images) if k else None, N.ptr(average), N.ptr(work), nbytes, N.stream_ptr())
    if rc < 0:
        raise ValueError(N.last_error())
    N._check(rc, "lgn_jet_images_f64")
    return images, average


def jet_images(p_target_polar: torch.Tensor, p_recons_polar: torch.Tensor, num_jet_images: int, jet_image_npix: int, abs_coord: bool,
               same_norm: bool = True, maxR: float = 0.5):
    """The four arrays plot_jet_image returns (target average, recons average, target images, recons images) as numpy arrays, with
    its branch: same_norm and abs_coord normalise both sides by the target's frame, else each side by its own (abs_coord) or not at
    all."""
    if same_norm and abs_coord:
        t_pix, t_avg = jet_image(p_target_polar, p_target_polar, 2, jet_image_npix, maxR, num_jet_images)
        r_pix, r_avg = jet_image(p_recons_polar, p_target_polar, 2, jet_image_npix, maxR, num_jet_images)
    else:
        mode = 1 if abs_coord else 0
        t_pix, t_avg = jet_image(p_target_polar, None, mode, jet_image_npix, maxR, num_jet_images)
        r_pix, r_avg = jet_image(p_recons_polar, None, mode, jet_image_npix, maxR, num_jet_images)
    return tuple(a.cpu().numpy() for a in (t_avg, r_avg, t_pix, r_pix))
