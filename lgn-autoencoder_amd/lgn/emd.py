"""
The energy mover's distance on the GPU, exactly: a batched optimal-transport solver (csrc/emd_wave.hpp, one wavefront per pair of
events, successive shortest paths) and the reference's 22nd anomaly score on top of it (``emd_loss()`` of
utils/jet_analysis/anomaly_detection.py, which calls ``energyflow.emd.emd`` per jet in a Python loop).

    theta_ij = sqrt((y_i - y'_j)^2 + (phi_i - phi'_j)^2) / R
    EMD      = min over f >= 0 of sum f_ij theta_ij + |sum pT - sum pT'|
               with sum_j f_ij <= pT_i, sum_i f_ij <= pT'_j, sum f_ij = min(sum pT, sum pT')

at energyflow's defaults beta = 1, norm = False, no periodic phi; ``emd`` takes those three as keywords and ``emds`` is
energyflow.emd.emds, the matrix of distances between every event of one set and every event of another or of one set with itself, in
one launch that reads each event where it lies (csrc/emd_pairs.hip).  The ground distance is Euclidean in (y, phi).  energyflow was not
available when this was written: the definitions in include/lgn_amd.h, from its documentation, are the specification (tests/_emd_ref.py
and tests/_emd_pairs_ref.py restate them as LPs).  What energyflow returns for two weightless events is not known; here that is a status
bit and NaN.

The distance is differentiable here as well: by LP sensitivity the gradient with respect to positions and weights is a closed form
in the optimal flow and the potentials, which the solving wavefront evaluates as an epilogue of the same launch (``emd_grad``,
``emd_differentiable``, ``EMDFn`` / ``EMDRelativeFn``; the formulas stand in include/lgn_amd.h).  ``lgn.losses.EMDLoss`` and
``HybridLoss`` are training losses on top of it for the module-API steps.  What is offered is the exact LP on the relative-polar frame
of the anomaly score, so that the training loss and the score are one quantity.  What is NOT offered: jetnet's regularised
differentiable QP, which the reference's ``EMDLoss`` wraps -- and that wrapper unbinds its (eta, phi, pt) columns as (eta, pt, phi),
handing jetnet an angle ratio as the weight, which is not reproduced; gradients under beta != 1, norm or periodic phi (``emd_grad``,
``emd_differentiable`` and the losses are the default options only) and gradients of ``emds``; energyflow's gdim, spherical measure,
coords and mask; the names ``--loss-choice emd`` / ``hybrid`` and the EMD inside the whole-step native calls, which stay refused.
There is no CPU fallback.
"""
from typing import Optional

import torch

from . import _native as N

NMAX = N.EMD_NMAX
INVALID, EMPTY, ITER, INFEASIBLE = N.EMD_INVALID, N.EMD_EMPTY, N.EMD_ITER, N.EMD_INFEASIBLE


FULL, UPPER, ALIGNED = N.EMD_PAIRS_FULL, N.EMD_PAIRS_UPPER, N.EMD_PAIRS_ALIGNED


def status_message(s: int, norm: bool = False) -> str:
    if s & INVALID:
        return "events hold NaN, infinity or a negative weight"
    if s & EMPTY:
        return "an event is weightless and cannot be normalised" if norm else "both events are weightless"
    if s & ITER:
        return "the cap of the solver's augmentations was hit"
    return "the weights left over exceed the rounding of the two sums"


def _workspace(B: int, n: int, dev) -> Optional[torch.Tensor]:
    nbytes = N.lib().lgn_emd_workspace_bytes(B, n)
    if nbytes < 0:
        raise ValueError(N.last_error())
    return torch.empty(nbytes, device=dev, dtype=torch.uint8) if nbytes else None


def flow_in_lds(n: int) -> bool:
    """Plan-time query: does the flow matrix of events of n particles live in LDS (else in a workspace in device memory)?"""
    nbytes = N.lib().lgn_emd_lds_bytes(n)
    if nbytes < 0:
        raise ValueError(N.last_error())
    return nbytes >= 8 * (n + 1) * (n + 1)


def _options(who: str, R, beta, norm, periodic_phi) -> "N.EmdOpts":
    if not (R > 0 and R < float("inf")):
        raise ValueError(f"{who} needs a finite R > 0; got {R}")
    if not (beta > 0 and beta < float("inf")):
        raise ValueError(f"{who} needs a finite beta > 0; got {beta}")
    return N.EmdOpts(float(R), float(beta), int(bool(norm)), int(bool(periodic_phi)))


def _pairs_workspace(P: int, n: int, dev) -> Optional[torch.Tensor]:
    return _workspace(min(P, 2 ** 31 - 1), n, dev)


def emds(X0: torch.Tensor, X1: Optional[torch.Tensor] = None, R: float = 1.0, beta: float = 1.0, norm: bool = False,
         periodic_phi: bool = False, return_status: bool = False):
    """energyflow.emd.emds: the (B0, B1) fp64 device tensor of the EMDs of every event of X0 (B0, n, 3) against every event of X1
    (B1, m, 3), zero-padded events of (pT, y, phi), in one launch and without a gathered copy of the events.  X1=None is the symmetric
    form, X0 against itself: the pairs i < j are solved and mirrored, the diagonal is 0.  R, beta, norm and periodic_phi as in emd().
    Raises ValueError at the first pair with a status bit; return_status=True returns the (B0, B1) int32 status as well (the distance
    of such a pair is NaN) and does not wait for the device.  No gradients."""
    sym = X1 is None
    a, b = X0, (X0 if sym else X1)
    if a.dim() != 3 or b.dim() != 3 or a.shape[-1] != 3 or b.shape[-1] != 3:
        raise ValueError(f"emds takes events (B0, n, 3) and (B1, m, 3) of (pT, y, phi); got {tuple(a.shape)} and {tuple(b.shape)}")
    B0, B1, n, m = int(a.shape[0]), int(b.shape[0]), int(a.shape[1]), int(b.shape[1])
    if not (1 <= n <= NMAX and 1 <= m <= NMAX):
        raise ValueError(f"emd supports 1 <= n, m <= {NMAX} particles per event; got n = {n}, m = {m}")
    opts = _options("emds", R, beta, norm, periodic_phi)
    if not (a.is_cuda and b.is_cuda):
        raise RuntimeError(f"lgn (MI355X build): emds runs only in the HIP kernels of liblgn_amd.so on a GPU device; got tensors on "
                           f"'{a.device}' and '{b.device}'. There is no CPU fallback.")
    a = N.f64(a.to(torch.float64))
    b = a if sym else N.f64(b.to(torch.float64))
    dev = a.device
    out = torch.empty(B0, B1, device=dev, dtype=torch.float64)
    status = torch.empty(B0, B1, device=dev, dtype=torch.int32)
    if B0 > 0 and B1 > 0:
        P = B0 * (B0 - 1) // 2 if sym else B0 * B1
        work = _pairs_workspace(max(P, 1), max(n, m), dev)
        rc = N.lib().lgn_emd_pairs_f64(N.ptr(a), None if sym else N.ptr(b), B0, B1, n, m, UPPER if sym else FULL, opts, N.ptr(out), None,
                                       None, None, N.ptr(status), N.ptr(work), work.numel() if work is not None else 0, N.stream_ptr())
        N._check(rc, "lgn_emd_pairs_f64")
    if not return_status:
        bad = status.nonzero().cpu().numpy()
        if len(bad):
            i, j = int(bad[0][0]), int(bad[0][1])
            raise ValueError(f"emds: {status_message(int(status[i, j].item()), bool(norm))} (pair ({i}, {j}), {len(bad)} pair(s) in all)")
    return (out, status) if return_status else out


def emd(ev0: torch.Tensor, ev1: torch.Tensor, R: float = 1.0, return_flow: bool = False, return_duals: bool = False,
        return_status: bool = False, beta: float = 1.0, norm: bool = False, periodic_phi: bool = False):
    """EMD of events of (pT, y, phi) particles: ev0 (B, n, 3) against ev1 (B, m, 3) device tensors (or one (n, 3) against one (m, 3)),
    n != m allowed, 1 <= n, m <= 191.  Returns the (B,) fp64 device tensor of distances (a 0-dim tensor for one pair); with
    return_flow also the optimal flow (B, n + 1, m + 1), with return_duals also the potentials (B, n + 1) and (B, m + 1) -- row n and
    column m are the fictitious particle that carries the weight difference.  Raises ValueError when a pair has a status bit (NaN,
    infinity or a negative weight; both events weightless; ...); return_status=True returns the (B,) int32 status last instead (the
    distance of such a pair is NaN) and does not wait for the device.
    beta, norm, periodic_phi: energyflow's arguments, as include/lgn_amd.h defines them -- the angular cost is theta^beta (the term of
    the weight difference is not raised), norm divides each event's weights by that event's sum (flow and potentials then refer to the
    normalised weights; an event without weight is a status bit), periodic_phi takes the minimum image of the phi difference.  At
    their defaults the call is the one it always was; otherwise the pairs kernel solves (csrc/emd_pairs.hip)."""
    single = ev0.dim() == 2
    a, b = (ev0.unsqueeze(0), ev1.unsqueeze(0)) if single else (ev0, ev1)
    if a.dim() != 3 or b.dim() != 3 or a.shape[-1] != 3 or b.shape[-1] != 3 or a.shape[0] != b.shape[0]:
        raise ValueError(f"emd takes events (B, n, 3) and (B, m, 3) of (pT, y, phi); got {tuple(ev0.shape)} and {tuple(ev1.shape)}")
    B, n, m = int(a.shape[0]), int(a.shape[1]), int(b.shape[1])
    if not (1 <= n <= NMAX and 1 <= m <= NMAX):
        raise ValueError(f"emd supports 1 <= n, m <= {NMAX} particles per event; got n = {n}, m = {m}")
    if not (R > 0 and R < float("inf")):
        raise ValueError(f"emd needs a finite R > 0; got {R}")
    a, b = N.f64(a.to(torch.float64)), N.f64(b.to(torch.float64))
    dev = a.device
    out = torch.empty(B, device=dev, dtype=torch.float64)
    status = torch.empty(B, device=dev, dtype=torch.int32)
    flow = torch.empty(B, n + 1, m + 1, device=dev, dtype=torch.float64) if return_flow else None
    d0 = torch.empty(B, n + 1, device=dev, dtype=torch.float64) if return_duals else None
    d1 = torch.empty(B, m + 1, device=dev, dtype=torch.float64) if return_duals else None
    optioned = beta != 1.0 or bool(norm) or bool(periodic_phi)
    opts = _options("emd", R, beta, norm, periodic_phi) if optioned else None
    if B > 0:
        work = _workspace(B, max(n, m), dev)
        if optioned:
            rc = N.lib().lgn_emd_pairs_f64(N.ptr(a), N.ptr(b), B, B, n, m, ALIGNED, opts, N.ptr(out), N.ptr(flow), N.ptr(d0), N.ptr(d1),
                                           N.ptr(status), N.ptr(work), work.numel() if work is not None else 0, N.stream_ptr())
            N._check(rc, "lgn_emd_pairs_f64")
        else:
            rc = N.lib().lgn_emd_f64(N.ptr(a), N.ptr(b), B, n, m, float(R), N.ptr(out), N.ptr(flow), N.ptr(d0), N.ptr(d1), N.ptr(status),
                                     N.ptr(work), work.numel() if work is not None else 0, N.stream_ptr())
            N._check(rc, "lgn_emd_f64")
    if not return_status:
        st = status.cpu().numpy()
        bad = st.nonzero()[0]
        if len(bad):
            raise ValueError(f"emd: {status_message(int(st[bad[0]]), bool(norm))} (pair {int(bad[0])}, {len(bad)} pair(s) in all)")
    res = [out] + ([flow] if return_flow else []) + ([d0, d1] if return_duals else [])
    if single:
        res = [x[0] for x in res]
    if return_status:
        res.append(status[0] if single else status)
    return res[0] if len(res) == 1 else tuple(res)


def emd_grad(ev0: torch.Tensor, ev1: torch.Tensor, R: float = 1.0, return_status: bool = False, return_flow: bool = False,
             return_duals: bool = False, need_g0: bool = True, need_g1: bool = True):
    """emd() with its gradients, in one launch: returns (emd (B,), g0 (B, n, 3), g1 (B, m, 3)[, flow][, dual0, dual1][, status]) --
    g0 = d emd / d ev0 and g1 = d emd / d ev1 in the events' column order (pT, y, phi); a gradient that is not needed (need_g0 /
    need_g1 False, not both) is None.  The value is emd()'s bit for bit.  A pair with a status bit has NaN gradients; ValueError and
    return_status as in emd().  One pair (n, 3) against (m, 3) is accepted like there."""
    single = ev0.dim() == 2
    a, b = (ev0.unsqueeze(0), ev1.unsqueeze(0)) if single else (ev0, ev1)
    if a.dim() != 3 or b.dim() != 3 or a.shape[-1] != 3 or b.shape[-1] != 3 or a.shape[0] != b.shape[0]:
        raise ValueError(f"emd_grad takes events (B, n, 3) and (B, m, 3) of (pT, y, phi); got {tuple(ev0.shape)} and {tuple(ev1.shape)}")
    B, n, m = int(a.shape[0]), int(a.shape[1]), int(b.shape[1])
    if not (1 <= n <= NMAX and 1 <= m <= NMAX):
        raise ValueError(f"emd supports 1 <= n, m <= {NMAX} particles per event; got n = {n}, m = {m}")
    if not (R > 0 and R < float("inf")):
        raise ValueError(f"emd needs a finite R > 0; got {R}")
    if not (need_g0 or need_g1):
        raise ValueError("emd_grad: at least one of the two gradients must be asked for (emd() is the call without gradients)")
    if not (a.is_cuda and b.is_cuda):
        raise RuntimeError(f"lgn (MI355X build): emd_grad runs only in the HIP kernels of liblgn_amd.so on a GPU device; got tensors "
                           f"on '{a.device}' and '{b.device}'. There is no CPU fallback.")
    a, b = N.f64(a.to(torch.float64)), N.f64(b.to(torch.float64))
    dev = a.device
    out = torch.empty(B, device=dev, dtype=torch.float64)
    status = torch.empty(B, device=dev, dtype=torch.int32)
    g0 = torch.empty(B, n, 3, device=dev, dtype=torch.float64) if need_g0 else None
    g1 = torch.empty(B, m, 3, device=dev, dtype=torch.float64) if need_g1 else None
    flow = torch.empty(B, n + 1, m + 1, device=dev, dtype=torch.float64) if return_flow else None
    d0 = torch.empty(B, n + 1, device=dev, dtype=torch.float64) if return_duals else None
    d1 = torch.empty(B, m + 1, device=dev, dtype=torch.float64) if return_duals else None
    if B > 0:
        work = _workspace(B, max(n, m), dev)
        rc = N.lib().lgn_emd_grad_f64(N.ptr(a), N.ptr(b), B, n, m, float(R), N.ptr(out), N.ptr(g0), N.ptr(g1), N.ptr(flow), N.ptr(d0),
                                      N.ptr(d1), N.ptr(status), N.ptr(work), work.numel() if work is not None else 0, N.stream_ptr())
        N._check(rc, "lgn_emd_grad_f64")
    if not return_status:
        st = status.cpu().numpy()
        bad = st.nonzero()[0]
        if len(bad):
            raise ValueError(f"emd: {status_message(int(st[bad[0]]))} (pair {int(bad[0])}, {len(bad)} pair(s) in all)")
    res = [out, g0, g1] + ([flow] if return_flow else []) + ([d0, d1] if return_duals else [])
    if single:
        res = [None if x is None else x[0] for x in res]
    if return_status:
        res.append(status[0] if single else status)
    return tuple(res)


def emd_relative_grad(recons: torch.Tensor, target: torch.Tensor, need_g_target: bool = False):
    """emd_relative_tensor() with its gradient with respect to the Cartesian jets, in one launch and with no host sync: returns
    (emd (B,), g_recons (B, N, 4), g_target (B, N, 4) or None, status (B,) int32).  The E column of the gradients is 0; a jet with a
    status bit has NaN gradients."""
    if recons.dim() != 3 or recons.shape[-1] != 4 or recons.shape != target.shape:
        raise ValueError(f"emd_relative_grad takes two (B, N, 4) Cartesian tensors; got {tuple(recons.shape)} and {tuple(target.shape)}")
    B, n = int(recons.shape[0]), int(recons.shape[1])
    if not 1 <= n <= NMAX:
        raise ValueError(f"the EMD supports 1 <= N <= {NMAX} particles per jet; got N = {n}")
    if not (recons.is_cuda and target.is_cuda):
        raise RuntimeError(f"lgn (MI355X build): the EMD runs only in the HIP kernels of liblgn_amd.so on a GPU device; got tensors on "
                           f"'{recons.device}' and '{target.device}'. There is no CPU fallback.")
    r, t = N.f64(recons.to(torch.float64)), N.f64(target.to(torch.float64))
    dev = r.device
    out = torch.empty(B, device=dev, dtype=torch.float64)
    status = torch.empty(B, device=dev, dtype=torch.int32)
    g_r = torch.empty(B, n, 4, device=dev, dtype=torch.float64)
    g_t = torch.empty(B, n, 4, device=dev, dtype=torch.float64) if need_g_target else None
    if B > 0:
        work = _workspace(B, n, dev)
        rc = N.lib().lgn_emd_relative_grad_f64(N.ptr(r), N.ptr(t), B, n, N.ptr(out), N.ptr(g_r), N.ptr(g_t), N.ptr(status), N.ptr(work),
                                               work.numel() if work is not None else 0, N.stream_ptr())
        N._check(rc, "lgn_emd_relative_grad_f64")
    return out, g_r, g_t, status


def _per_pair(g, grad):
    return grad * g.reshape(-1, 1, 1)


class EMDFn(torch.autograd.Function):
    """(ev0 (B,n,3), ev1 (B,m,3), R) -> (B,) distances.  One launch in forward, which also returns the gradients for an upstream
    gradient of one; backward scales them per pair.  A pair with a status bit is NaN, value and gradients."""

    @staticmethod
    def forward(ctx, ev0, ev1, R):
        need1 = bool(ctx.needs_input_grad[1])
        need0 = bool(ctx.needs_input_grad[0]) or not need1            # (the launch needs one gradient output at least)
        out, g0, g1, _ = emd_grad(ev0.detach(), ev1.detach(), R, return_status=True, need_g0=need0, need_g1=need1)
        ctx.has = (g0 is not None, g1 is not None)
        ctx.save_for_backward(*[g for g in (g0, g1) if g is not None])
        return out

    @staticmethod
    def backward(ctx, g):
        saved = list(ctx.saved_tensors)
        g0 = saved.pop(0) if ctx.has[0] else None
        g1 = saved.pop(0) if ctx.has[1] else None
        return (_per_pair(g, g0) if ctx.needs_input_grad[0] else None), (_per_pair(g, g1) if ctx.needs_input_grad[1] else None), None


class EMDRelativeFn(torch.autograd.Function):
    """(recons (B,N,4), target (B,N,4), owner) -> (B,) distances on the relative-polar frames, emd_relative_tensor()'s bit for bit;
    the gradient of the target is computed only if the target needs one.  ``owner.status`` receives the (B,) int32 flags."""

    @staticmethod
    def forward(ctx, recons, target, owner):
        out, g_r, g_t, status = emd_relative_grad(recons.detach(), target.detach(), need_g_target=ctx.needs_input_grad[1])
        if owner is not None:
            owner.status = status
        ctx.has_target = g_t is not None
        ctx.save_for_backward(*([g_r, g_t] if g_t is not None else [g_r]))
        return out

    @staticmethod
    def backward(ctx, g):
        saved = ctx.saved_tensors
        return ((_per_pair(g, saved[0]) if ctx.needs_input_grad[0] else None),
                (_per_pair(g, saved[1]) if ctx.has_target and ctx.needs_input_grad[1] else None), None)


def emd_differentiable(ev0: torch.Tensor, ev1: torch.Tensor, R: float = 1.0) -> torch.Tensor:
    """emd() of (B, n, 3) against (B, m, 3) device tensors as a (B,) tensor with autograd (gradients with respect to pT, y and phi of
    both events).  No host sync: a pair with a status bit is NaN, value and gradients (emd_grad(return_status=True) shows the flags)."""
    if ev0.dim() != 3 or ev1.dim() != 3:
        raise ValueError(f"emd_differentiable takes events (B, n, 3) and (B, m, 3); got {tuple(ev0.shape)} and {tuple(ev1.shape)}")
    return EMDFn.apply(ev0, ev1, float(R))


def emd_relative_tensor(recons: torch.Tensor, target: torch.Tensor, return_status: bool = False):
    """The reference's score "emd (relative coordinates)" of (B, N, 4) Cartesian device tensors as a (B,) fp64 device tensor, with no
    host sync (chain it after NativeEvalStep.run()): each jet is staged into its relative-polar frame (pT / (jet pT + 1e-16), eta - jet
    eta, wrapped phi - jet phi) exactly as the other 21 scores stage it, then energyflow.emd.emd(target_rel, recons_rel).  A jet with
    a status bit (see emd()) gets NaN; return_status=True also returns the (B,) int32 status."""
    if recons.dim() != 3 or recons.shape[-1] != 4 or recons.shape != target.shape:
        raise ValueError(f"emd_relative_tensor takes two (B, N, 4) Cartesian tensors; got {tuple(recons.shape)} and {tuple(target.shape)}")
    B, n = int(recons.shape[0]), int(recons.shape[1])
    if not 1 <= n <= NMAX:
        raise ValueError(f"the EMD score supports 1 <= N <= {NMAX} particles per jet; got N = {n}")
    r, t = N.f64(recons.to(torch.float64)), N.f64(target.to(torch.float64))
    dev = r.device
    out = torch.empty(B, device=dev, dtype=torch.float64)
    status = torch.empty(B, device=dev, dtype=torch.int32)
    if B > 0:
        work = _workspace(B, n, dev)
        rc = N.lib().lgn_emd_relative_f64(N.ptr(r), N.ptr(t), B, n, N.ptr(out), N.ptr(status), N.ptr(work),
                                          work.numel() if work is not None else 0, N.stream_ptr())
        N._check(rc, "lgn_emd_relative_f64")
    return (out, status) if return_status else out


def max_augmentations(reset: bool = True) -> int:
    """Debug counter: the largest number of augmentations any pair needed since the last reset (waits for the device)."""
    import ctypes
    v = ctypes.c_int(0)
    N._check(N.lib().lgn_emd_debug_max_augmentations(ctypes.byref(v), int(reset)), "lgn_emd_debug_max_augmentations")
    return v.value
