"""
Per-jet anomaly scores on the GPU: the drop-in of the reference's utils/jet_analysis/anomaly_detection.py ``anomaly_scores()`` /
``anomaly_scores_sig_bkg()`` (Chamfer, Hungarian and MSE in five frames, their Lorentz-metric versions and three jet-level scores),
plus the batched exact assignment solver the Hungarian scores use (``linear_sum_assignment``, scipy's ``col_ind``, ties included).

One HIP kernel launch per chunk of jets (csrc/anomaly.hip, C ABI ``lgn_anomaly_scores_f64``).  There is no CPU fallback: the scores
need a GPU.  Deliberate differences from the reference:
  * ``batch_size`` is only a chunk size.  The reference's batched paths (batch_size > 0) score the reconstruction against itself
    and return zeros for every Chamfer and Hungarian score; here every batch size returns the unbatched scores.
  * ``include_emd=True`` raises NotImplementedError (EMD needs the energyflow package and is out of scope).
  * The Hungarian pairing is the reference's own, p[col_ind[r]] against q[r], not the optimal one; kept on purpose.
  * The scores are computed in fp64 whatever the input dtype.
"""
from typing import Dict, Optional, Tuple

import numpy as np
import torch

from . import _native as N

# the reference's key strings (anomaly_detection.py), in the order anomaly_scores() inserts them
CHAMFER_PARTICLE_CARTESIAN = "particle, Cartesian, Chamfer distance"
CHAMFER_PARTICLE_POLAR = "particle, polar, Chamfer distance"
CHAMFER_PARTICLE_NORMALIZED_CARTESIAN = "particle, normalized Cartesian, Chamfer distance"
CHAMFER_PARTICLE_NORMALIZED_POLAR = "particle, normalized polar, Chamfer distance"
CHAMFER_PARTICLE_RELATIVE_POLAR = "particle, relative polar, Chamfer distance"

HUNGARIAN_PARTICLE_CARTESIAN = "particle, Cartesian, Hungarian distance"
HUNGARIAN_PARTICLE_POLAR = "particle, polar, Hungarian distance"
HUNGARIAN_PARTICLE_NORMALIZED_CARTESIAN = "particle, normalized Cartesian, Hungarian distance"
HUNGARIAN_PARTICLE_NORMALIZED_POLAR = "particle, normalized polar, Hungarian distance"
HUNGARIAN_PARTICLE_RELATIVE_POLAR = "particle, relative polar, Hungarian distance"

MSE_PARTICLE_CARTESIAN = "particle, Cartesian, MSE"
MSE_PARTICLE_POLAR = "particle, polar, MSE"
MSE_PARTICLE_NORMALIZED_CARTESIAN = "particle, normalized Cartesian, MSE"
MSE_PARTICLE_NORMALIZED_POLAR = "particle, normalized polar, MSE"
MSE_PARTICLE_RELATIVE_POLAR = "particle, relative polar, MSE"

JET_CARTESIAN = "jet, Cartesian"
JET_POLAR = "jet, polar"
MSE_PARTICLE_LORENTZ = "particle, Lorentz norms, MSE"
CHAMFER_PARTICLE_LORENTZ = "particle, Lorentz norms, Chamfer distance"
HUNGARIAN_PARTICLE_LORENTZ = "particle, Lorentz norms, Hungarian distance"
JET_LORENTZ = "jet, Lorentz norms"
EMD_RELATIVE = "emd (relative coordinates)"

SCORE_KEYS = (
    CHAMFER_PARTICLE_CARTESIAN, CHAMFER_PARTICLE_POLAR, CHAMFER_PARTICLE_NORMALIZED_CARTESIAN, CHAMFER_PARTICLE_NORMALIZED_POLAR,
    CHAMFER_PARTICLE_RELATIVE_POLAR,
    HUNGARIAN_PARTICLE_CARTESIAN, HUNGARIAN_PARTICLE_POLAR, HUNGARIAN_PARTICLE_NORMALIZED_CARTESIAN,
    HUNGARIAN_PARTICLE_NORMALIZED_POLAR, HUNGARIAN_PARTICLE_RELATIVE_POLAR,
    MSE_PARTICLE_CARTESIAN, MSE_PARTICLE_POLAR, MSE_PARTICLE_NORMALIZED_CARTESIAN, MSE_PARTICLE_NORMALIZED_POLAR,
    MSE_PARTICLE_RELATIVE_POLAR,
    JET_CARTESIAN, JET_POLAR,
    CHAMFER_PARTICLE_LORENTZ, HUNGARIAN_PARTICLE_LORENTZ, MSE_PARTICLE_LORENTZ, JET_LORENTZ,
)
HUNGARIAN_INDEX = (5, 6, 7, 8, 9, 18)      # score slots of the six assignment variants: the row order of col4row
NMAX = 192                                 # include/lgn_amd.h: LGN_ANOMALY_NMAX
ALL = (1 << 21) - 1                        # LGN_ANOMALY_ALL
NO_HUNGARIAN = ALL & ~sum(1 << s for s in HUNGARIAN_INDEX)
DEFAULT_CHUNK = 65536


def _device() -> torch.device:
    if not torch.cuda.is_available():
        raise RuntimeError("lgn.anomaly needs a GPU (liblgn_amd.so); there is no CPU fallback")
    return torch.device("cuda", torch.cuda.current_device())


def _check_shapes(*xs: torch.Tensor) -> Tuple[int, int]:
    shape = xs[0].shape
    if len(shape) != 3 or shape[-1] != 4:
        raise ValueError(f"anomaly scores take (B, N, 4) Cartesian 4-vectors; got {tuple(shape)}")
    for x in xs[1:]:
        if x.shape != shape:
            raise ValueError(f"recons, target and their normalized versions must have one shape; got {tuple(shape)} and {tuple(x.shape)}")
    B, n = int(shape[0]), int(shape[1])
    if not 1 <= n <= NMAX:
        raise ValueError(f"anomaly scores support 1 <= N <= {NMAX} particles per jet; got N = {n}")
    return B, n


def _launch(xs, mask: int, scores, status, col4row=None):
    B, n = int(xs[0].shape[0]), int(xs[0].shape[1])
    rc = N.lib().lgn_anomaly_scores_f64(*(N.ptr(x) for x in xs), B, n, int(mask), N.ptr(scores), N.ptr(col4row), N.ptr(status),
                                        N.stream_ptr())
    N._check(rc, "lgn_anomaly_scores_f64")


def score_tensor(recons: torch.Tensor, target: torch.Tensor, recons_normalized: torch.Tensor, target_normalized: torch.Tensor,
                 hungarian: bool = True, return_status: bool = False, col4row: Optional[torch.Tensor] = None):
    """The 21 scores of device tensors as one (B, 21) fp64 device tensor, columns in SCORE_KEYS order, with no host sync (chain it
    after NativeEvalStep.run()).  hungarian=False skips the six assignments (their columns are NaN).  A jet whose Hungarian cost
    holds NaN / -inf gets NaN there and a status bit (return_status=True also returns the (B,) int32 status; see
    include/lgn_amd.h).  col4row: optional (6, B, N) int32 device tensor that receives the six assignments."""
    B, n = _check_shapes(recons, target, recons_normalized, target_normalized)
    xs = [N.f64(x.to(torch.float64)) for x in (recons, target, recons_normalized, target_normalized)]
    dev = xs[0].device
    scores = torch.empty(B, 21, device=dev, dtype=torch.float64)
    status = torch.empty(B, device=dev, dtype=torch.int32)
    if col4row is not None and (col4row.shape != (6, B, n) or col4row.dtype != torch.int32):
        raise ValueError(f"col4row must be a (6, {B}, {n}) int32 tensor")
    if B > 0:
        _launch(xs, ALL if hungarian else NO_HUNGARIAN, scores, status, col4row)
    return (scores, status) if return_status else scores


def _raise_for_status(status: np.ndarray):
    bad = np.flatnonzero(status)
    if len(bad):
        s = int(status[bad[0]])
        what = "matrix contains invalid numeric entries" if s & 0xFF else "cost matrix is infeasible"
        raise ValueError(f"{what} (jet {int(bad[0])}, {len(bad)} jet(s) in all)")


def anomaly_scores(recons: torch.Tensor, target: torch.Tensor, recons_normalized: torch.Tensor, target_normalized: torch.Tensor,
                   include_emd: bool = False, batch_size: int = -1) -> Dict[str, np.ndarray]:
    """anomaly_scores() of utils/jet_analysis/anomaly_detection.py: {key: (B,) np.ndarray} for the 21 keys, in the reference's order.
    Inputs may be CPU or device tensors (B, N, 4); CPU inputs travel to the GPU in chunks through pinned buffers.  batch_size > 0
    is the chunk size (default 65,536 jets) and never changes the values.  Raises ValueError, worded as scipy words it, when a
    Hungarian cost holds NaN or -inf."""
    if include_emd:
        raise NotImplementedError("include_emd=True: the EMD score needs the energyflow package and is not implemented natively; "
                                  "call anomaly_scores(..., include_emd=False)")
    xs = (recons, target, recons_normalized, target_normalized)
    B, n = _check_shapes(*xs)
    dev = _device()
    chunk = int(batch_size) if batch_size is not None and batch_size > 0 else DEFAULT_CHUNK
    chunk = max(1, min(chunk, B))
    scores = torch.empty(B, 21, device=dev, dtype=torch.float64)
    status = torch.empty(B, device=dev, dtype=torch.int32)
    on_host = [not x.is_cuda for x in xs]
    pinned = [torch.empty(chunk, n, 4, dtype=torch.float64).pin_memory() if h else None for h in on_host]
    staged = [torch.empty(chunk, n, 4, device=dev, dtype=torch.float64) if h else None for h in on_host]
    copied = None
    for b0 in range(0, B, chunk):
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
                part.append(N.f64(x[b0:b0 + m].to(device=dev, dtype=torch.float64)))
        copied = torch.cuda.Event()
        copied.record()
        _launch(part, ALL, scores[b0:b0 + m], status[b0:b0 + m])
    scores_h = scores.cpu().numpy()
    _raise_for_status(status.cpu().numpy())
    return {k: np.ascontiguousarray(scores_h[:, i]) for i, k in enumerate(SCORE_KEYS)}


def anomaly_scores_sig_bkg(sig_recons: torch.Tensor, sig_target: torch.Tensor, sig_recons_normalized: torch.Tensor,
                           sig_target_normalized: torch.Tensor, bkg_recons: torch.Tensor, bkg_target: torch.Tensor,
                           bkg_recons_normalized: torch.Tensor, bkg_target_normalized: torch.Tensor, include_emd: bool = False,
                           batch_size: int = -1):
    """anomaly_scores_sig_bkg() of the reference: (scores, true_labels, sig_scores, bkg_scores) with the signal first, labels +1
    for signal and -1 for background."""
    sig = anomaly_scores(sig_recons, sig_target, sig_recons_normalized, sig_target_normalized, include_emd=include_emd,
                         batch_size=batch_size)
    bkg = anomaly_scores(bkg_recons, bkg_target, bkg_recons_normalized, bkg_target_normalized, include_emd=include_emd,
                         batch_size=batch_size)
    scores = {k: np.concatenate([sig[k], bkg[k]]) for k in sig}
    labels = np.concatenate([np.ones_like(sig[CHAMFER_PARTICLE_CARTESIAN]), -np.ones_like(bkg[CHAMFER_PARTICLE_CARTESIAN])])
    return scores, labels, sig, bkg


def linear_sum_assignment(cost: torch.Tensor) -> torch.Tensor:
    """Batched scipy.optimize.linear_sum_assignment(cost[b])[1]: cost (B, n, n) (or one (n, n)) device tensor -> col_ind (B, n)
    (or (n,)) int64, ties broken as scipy breaks them.  1 <= n <= 192.  Raises ValueError, as scipy does, for a matrix holding NaN
    or -inf, or an infeasible one."""
    single = cost.dim() == 2
    c = cost.unsqueeze(0) if single else cost
    if c.dim() != 3 or c.shape[1] != c.shape[2]:
        raise ValueError(f"linear_sum_assignment takes square cost matrices (B, n, n); got {tuple(cost.shape)}")
    B, n = int(c.shape[0]), int(c.shape[1])
    if not 1 <= n <= NMAX:
        raise ValueError(f"linear_sum_assignment supports 1 <= n <= {NMAX}; got n = {n}")
    c = N.f64(c.to(torch.float64))
    col = torch.empty(B, n, device=c.device, dtype=torch.int32)
    status = torch.empty(B, device=c.device, dtype=torch.int32)
    if B > 0:
        rc = N.lib().lgn_linear_sum_assignment_f64(N.ptr(c), B, n, N.ptr(col), N.ptr(status), N.stream_ptr())
        N._check(rc, "lgn_linear_sum_assignment_f64")
        _raise_for_status(status.cpu().numpy())
    col = col.to(torch.int64)
    return col[0] if single else col
