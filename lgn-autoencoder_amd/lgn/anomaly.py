"""
Per-jet anomaly scores on the GPU: the drop-in of the reference's utils/jet_analysis/anomaly_detection.py ``anomaly_scores()`` /
``anomaly_scores_sig_bkg()`` (Chamfer, Hungarian and MSE in five frames, their Lorentz-metric versions and three jet-level scores),
plus the batched exact assignment solver the Hungarian scores use (``linear_sum_assignment``, scipy's ``col_ind``, ties included)
and the drop-in of its ``get_ROC_AUC()``: ROC curves and AUCs of every score kind, sorted on the GPU (``roc_auc_tensor``,
csrc/roc.hip, C ABI ``lgn_roc_auc_f64``).

One HIP kernel launch per chunk of jets (csrc/anomaly.hip, C ABI ``lgn_anomaly_scores_f64``).  There is no CPU fallback: the scores
need a GPU.  Deliberate differences from the reference:
  * ``batch_size`` is only a chunk size.  The reference's batched paths (batch_size > 0) score the reconstruction against itself
    and return zeros for every Chamfer and Hungarian score; here every batch size returns the unbatched scores.
  * ``include_emd=True`` raises NotImplementedError, as before the EMD score existed here; ``include_emd="native"`` adds the
    reference's 22nd score, "emd (relative coordinates)", computed exactly on the GPU (lgn/emd.py, csrc/emd.hip: an optimal-transport
    solver, one wavefront per jet) from energyflow's documented definition -- the energyflow package is not needed and was not
    available to compare with.  A jet whose two sides are both weightless raises (what energyflow returns there is not known).
  * The Hungarian pairing is the reference's own, p[col_ind[r]] against q[r], not the optimal one; kept on purpose.
  * The scores are computed in fp64 whatever the input dtype.
  * ``get_ROC_AUC`` logs what the reference logs and saves what it saves, but draws nothing; the ROC of labels in {0, 1} flips as
    that of labels in {-1, 1} does (the reference's negated {0, -1} labels make sklearn raise).
"""
import logging
from pathlib import Path
from typing import Dict, List, Optional, Tuple, Union

import numpy as np
import torch

from . import _native as N
from . import emd as _emd

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
SCORE_KEYS_EMD = SCORE_KEYS + (EMD_RELATIVE,)     # the 22 keys of include_emd="native", in the reference's order
EMD_STATUS_SHIFT = 16                      # the EMD score's LGN_EMD_* bits in a combined status
DEFAULT_CHUNK = 65536
ROC_TILE = N.ROC_TILE                      # LGN_ROC_TILE: rows per sort tile of roc_auc_tensor (its sort changes path at multiples)
ROC_GROUP_BYTES = 1 << 30                  # get_ROC_AUC: curve buffers + workspace of one group of columns stay below this


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
                 hungarian: bool = True, return_status: bool = False, col4row: Optional[torch.Tensor] = None, emd: bool = False):
    """The 21 scores of device tensors as one (B, 21) fp64 device tensor, columns in SCORE_KEYS order, with no host sync (chain it
    after NativeEvalStep.run()).  hungarian=False skips the six assignments (their columns are NaN).  A jet whose Hungarian cost
    holds NaN / -inf gets NaN there and a status bit (return_status=True also returns the (B,) int32 status; see
    include/lgn_amd.h).  col4row: optional (6, B, N) int32 device tensor that receives the six assignments.  emd=True: (B, 22), the
    22nd column the EMD score (SCORE_KEYS_EMD order; N <= 191); its LGN_EMD_* status bits are in the status from bit EMD_STATUS_SHIFT
    up, and such a jet's EMD is NaN."""
    B, n = _check_shapes(recons, target, recons_normalized, target_normalized)
    xs = [N.f64(x.to(torch.float64)) for x in (recons, target, recons_normalized, target_normalized)]
    dev = xs[0].device
    scores = torch.empty(B, 21, device=dev, dtype=torch.float64)
    status = torch.empty(B, device=dev, dtype=torch.int32)
    if col4row is not None and (col4row.shape != (6, B, n) or col4row.dtype != torch.int32):
        raise ValueError(f"col4row must be a (6, {B}, {n}) int32 tensor")
    if B > 0:
        _launch(xs, ALL if hungarian else NO_HUNGARIAN, scores, status, col4row)
    if emd:
        e, est = _emd.emd_relative_tensor(xs[0], xs[1], return_status=True)
        scores = torch.cat([scores, e.unsqueeze(1)], dim=1)
        status = status | (est << EMD_STATUS_SHIFT)
    return (scores, status) if return_status else scores


def _raise_for_status(status: np.ndarray):
    bad = np.flatnonzero(status)
    if len(bad):
        s = int(status[bad[0]])
        if s & 0xFFFF:
            what = "matrix contains invalid numeric entries" if s & 0xFF else "cost matrix is infeasible"
        else:
            what = "EMD score: " + _emd.status_message(s >> EMD_STATUS_SHIFT)
        raise ValueError(f"{what} (jet {int(bad[0])}, {len(bad)} jet(s) in all)")


def anomaly_scores(recons: torch.Tensor, target: torch.Tensor, recons_normalized: torch.Tensor, target_normalized: torch.Tensor,
                   include_emd: Union[bool, str] = False, batch_size: int = -1) -> Dict[str, np.ndarray]:
    """anomaly_scores() of utils/jet_analysis/anomaly_detection.py: {key: (B,) np.ndarray} for the 21 keys, in the reference's order.
    Inputs may be CPU or device tensors (B, N, 4); CPU inputs travel to the GPU in chunks through pinned buffers.  batch_size > 0
    is the chunk size (default 65,536 jets) and never changes the values.  Raises ValueError, worded as scipy words it, when a
    Hungarian cost holds NaN or -inf.  include_emd="native": the same 21 keys, then EMD_RELATIVE as the 22nd (N <= 191), computed in
    the same chunks; raises ValueError when a jet's EMD has a status bit (lgn/emd.py)."""
    native_emd = isinstance(include_emd, str) and include_emd == "native"
    if include_emd and not native_emd:
        raise NotImplementedError("include_emd=True: the EMD score needs the energyflow package and is not implemented natively; "
                                  "call anomaly_scores(..., include_emd=False)")
    xs = (recons, target, recons_normalized, target_normalized)
    B, n = _check_shapes(*xs)
    dev = _device()
    chunk = int(batch_size) if batch_size is not None and batch_size > 0 else DEFAULT_CHUNK
    chunk = max(1, min(chunk, B))
    scores = torch.empty(B, 21, device=dev, dtype=torch.float64)
    status = torch.empty(B, device=dev, dtype=torch.int32)
    if native_emd:
        if n > _emd.NMAX:
            raise ValueError(f"the EMD score supports 1 <= N <= {_emd.NMAX} particles per jet; got N = {n}")
        emd = torch.empty(B, device=dev, dtype=torch.float64)
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
        if native_emd:
            e, est = _emd.emd_relative_tensor(part[0], part[1], return_status=True)
            emd[b0:b0 + m] = e
            status[b0:b0 + m] |= est << EMD_STATUS_SHIFT
    scores_h = scores.cpu().numpy()
    _raise_for_status(status.cpu().numpy())
    out = {k: np.ascontiguousarray(scores_h[:, i]) for i, k in enumerate(SCORE_KEYS)}
    if native_emd:
        out[EMD_RELATIVE] = emd.cpu().numpy()
    return out


def anomaly_scores_sig_bkg(sig_recons: torch.Tensor, sig_target: torch.Tensor, sig_recons_normalized: torch.Tensor,
                           sig_target_normalized: torch.Tensor, bkg_recons: torch.Tensor, bkg_target: torch.Tensor,
                           bkg_recons_normalized: torch.Tensor, bkg_target_normalized: torch.Tensor,
                           include_emd: Union[bool, str] = False,
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


def roc_auc_tensor(scores: torch.Tensor, labels: torch.Tensor) -> Dict[str, torch.Tensor]:
    """ROC curve and AUC of every column of a (M, K) fp64 device tensor against labels (M,) (any real dtype; 1 is the positive
    class, the other is 0 or -1), with no host sync: chain it after score_tensor().  Per column sklearn's roc_curve(labels, column)
    with its defaults, sklearn's auc, and the reference's flip (AUC < 0.5: the curve of the negated labels).  A column view of a wider
    tensor (unit column stride) is read in place.  Returns device tensors: fpr, tpr, thresholds (K, M + 1), of which the first
    length[k] entries of row k are the curve; length, flipped, status (K,) int32; auc (K,) fp64.  A column with a status bit
    (_native.ROC_NONFINITE / ROC_SINGLE_CLASS / ROC_BAD_LABEL) has length 0 and auc NaN."""
    _device()
    if scores.dim() != 2 or scores.dtype != torch.float64 or not scores.is_cuda:
        raise ValueError(f"roc_auc_tensor takes a (M, K) fp64 device tensor of scores; got {tuple(scores.shape)} {scores.dtype} on "
                         f"{scores.device}")
    M, K = int(scores.shape[0]), int(scores.shape[1])
    if M < 1 or K < 1:
        raise ValueError(f"roc_auc_tensor needs at least one row and one column; got {tuple(scores.shape)}")
    if labels.dim() != 1 or labels.shape[0] != M or labels.is_complex():
        raise ValueError(f"labels must be a real ({M},) tensor; got {tuple(labels.shape)} {labels.dtype}")
    if scores.stride(1) != 1 and K > 1 or scores.stride(0) < K and M > 1:
        scores = scores.contiguous()
    ld = int(scores.stride(0)) if M > 1 and scores.stride(0) >= K else K
    dev = scores.device
    labels = labels.to(device=dev, dtype=torch.float64).contiguous()
    L = N.lib()
    nbytes = L.lgn_roc_workspace_bytes(M, K)
    if nbytes < 0:
        raise ValueError(N.last_error())
    curves = torch.empty(3, K, M + 1, device=dev, dtype=torch.float64)
    ints = torch.empty(3, K, device=dev, dtype=torch.int32)
    auc = torch.empty(K, device=dev, dtype=torch.float64)
    work = torch.empty(nbytes, device=dev, dtype=torch.uint8)
    rc = L.lgn_roc_auc_f64(scores.data_ptr(), M, ld, K, N.ptr(labels), curves[0].data_ptr(), curves[1].data_ptr(),
                           curves[2].data_ptr(), ints[0].data_ptr(), N.ptr(auc), ints[1].data_ptr(), ints[2].data_ptr(),
                           N.ptr(work), nbytes, N.stream_ptr())
    N._check(rc, "lgn_roc_auc_f64")
    return dict(fpr=curves[0], tpr=curves[1], thresholds=curves[2], length=ints[0], auc=auc, flipped=ints[1], status=ints[2])


def _raise_for_roc_status(status: np.ndarray):
    bad = np.flatnonzero(status)
    if not len(bad):
        return
    s = int(np.bitwise_or.reduce(status))
    if s & N.ROC_BAD_LABEL:
        raise ValueError("true_labels must hold two classes: 1 and either 0 or -1")
    k = next((i for i in bad if status[i] & N.ROC_NONFINITE), None)
    if k is not None:            # sklearn's wording (check_array on y_score); a NaN goes first there too
        what = "NaN" if status[k] & N.ROC_NAN else "infinity or a value too large for dtype('float64')"
        raise ValueError(f"Input contains {what}.")
    raise ValueError("Only one class present in true_labels: the ROC curve is not defined (sklearn's rates are NaN and its auc "
                     "raises)")


def get_ROC_AUC(scores_dict, true_labels, save_path: Union[str, Path] = None, plot_rocs: bool = True,
                rocs_hlines: List[float] = [1e-1, 1e-2]):
    """get_ROC_AUC() of utils/jet_analysis/anomaly_detection.py: (roc_curves, aucs) with the keys of scores_dict in its order,
    roc_curves[kind] = (fpr, tpr, thresholds) as numpy arrays of the true length, aucs[kind] a float.  The values of scores_dict and
    true_labels may be numpy arrays or CPU or device tensors.  Sorted and summed on the GPU, the columns in groups when they are many
    and long, with one synchronisation at the end.  Raises ValueError as sklearn words it for NaN or infinite scores, and for labels
    of one class.  save_path: scores.pt, true_labels.pt, roc_curves.pt and aucs.pt, as the reference saves them.  plot_rocs logs the
    best AUC and each kind's intercepts at rocs_hlines; nothing is drawn."""
    dev = _device()
    keys = list(scores_dict)
    if not keys:
        return dict(), dict()
    cols = [torch.as_tensor(scores_dict[k]).reshape(-1).to(device=dev, dtype=torch.float64) for k in keys]
    M = int(cols[0].shape[0])
    if any(int(c.shape[0]) != M for c in cols):
        raise ValueError("every score kind must have one score per label")
    labels = torch.as_tensor(true_labels).reshape(-1).to(device=dev)
    per_col = 3 * 8 * (M + 1) + max(1, N.lib().lgn_roc_workspace_bytes(max(M, 1), 1))
    group = max(1, min(len(keys), ROC_GROUP_BYTES // per_col))
    host, small = [], []
    for k0 in range(0, len(keys), group):
        out = roc_auc_tensor(torch.stack(cols[k0:k0 + group], dim=1), labels)
        kg = out["auc"].shape[0]
        pinned = torch.empty(3, kg, M + 1, dtype=torch.float64).pin_memory()
        for i, name in enumerate(("fpr", "tpr", "thresholds")):
            pinned[i].copy_(out[name], non_blocking=True)
        meta = torch.empty(4, kg, dtype=torch.float64).pin_memory()
        for i, name in enumerate(("length", "auc", "flipped", "status")):
            meta[i].copy_(out[name].to(torch.float64), non_blocking=True)
        host.append(pinned)
        small.append(meta)
    torch.cuda.current_stream().synchronize()
    meta = torch.cat(small, dim=1).numpy()
    _raise_for_roc_status(meta[3].astype(np.int64))
    roc_curves, aucs = dict(), dict()
    for k, kind in enumerate(keys):
        g, j = divmod(k, group)
        n = int(meta[0][k])
        roc_curves[kind] = tuple(host[g][i, j, :n].numpy().copy() for i in range(3))
        aucs[kind] = float(meta[1][k])

    if save_path is not None:
        save_path = Path(save_path)
        save_path.mkdir(exist_ok=True, parents=True)
        torch.save(scores_dict, save_path / "scores.pt")
        torch.save(true_labels, save_path / "true_labels.pt")
        torch.save(roc_curves, save_path / "roc_curves.pt")
        torch.save(aucs, save_path / "aucs.pt")

    if plot_rocs:
        auc_sorted = list(sorted(aucs.items(), key=lambda x: x[1], reverse=True))
        logging.info(f"Best AUC: {auc_sorted[0]}")
        for kind, _ in auc_sorted:
            fpr, tpr, _ = roc_curves[kind]
            logging.info(f"{kind}: {dict((h, tpr[np.searchsorted(fpr, h)]) for h in rocs_hlines)}")
    return roc_curves, aucs
