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
of the anomaly score, so that the training loss and the score are one quantity.  The gradients exist under R, beta, norm and
periodic_phi as well (csrc/emd_grad_opts.hip: the same epilogue under the option cost and weights): ``emd_grad``,
``emd_differentiable``, ``emd_relative_grad``, ``emd_relative_tensor`` and the losses take the options as keywords, and at their
defaults make the calls they always made.  ``emds_differentiable`` is ``emds`` with autograd, composed from ``emd_grad`` or, with
``backward="native"``, on the matrix-gradient kernels (csrc/emd_pairs_grad.hip): ``emds_pair_grads`` solves every pair once and returns
its gradients, ``emds_grad`` sums them under an upstream matrix in a fixed order, chunk after chunk of rows.  What is NOT
offered: jetnet's regularised differentiable QP, which the reference's ``EMDLoss`` wraps -- and that wrapper unbinds its (eta, phi, pt)
columns as (eta, pt, phi), handing jetnet an angle ratio as the weight, which is not reproduced; energyflow's gdim, spherical measure,
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
    of such a pair is NaN) and does not wait for the device.  No gradients: emds_differentiable() is the form with autograd."""
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
             return_duals: bool = False, need_g0: bool = True, need_g1: bool = True, beta: float = 1.0, norm: bool = False,
             periodic_phi: bool = False):
    """emd() with its gradients, in one launch: returns (emd (B,), g0 (B, n, 3), g1 (B, m, 3)[, flow][, dual0, dual1][, status]) --
    g0 = d emd / d ev0 and g1 = d emd / d ev1 in the events' column order (pT, y, phi); a gradient that is not needed (need_g0 /
    need_g1 False, not both) is None.  The value is emd()'s bit for bit.  A pair with a status bit has NaN gradients; ValueError and
    return_status as in emd().  One pair (n, 3) against (m, 3) is accepted like there.
    beta, norm, periodic_phi as in emd(): at their defaults the call is the one it always was, otherwise lgn_emd_grad_opts_f64 solves
    and differentiates under the options (include/lgn_amd.h has the formulas; under norm the weight gradients are those of the given,
    unnormalised pT, and flow and potentials refer to the normalised weights)."""
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
    optioned = beta != 1.0 or bool(norm) or bool(periodic_phi)
    opts = _options("emd_grad", R, beta, norm, periodic_phi) if optioned else None
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
        if opts is not None:
            rc = N.lib().lgn_emd_grad_opts_f64(N.ptr(a), N.ptr(b), B, n, m, opts, N.ptr(out), N.ptr(g0), N.ptr(g1), N.ptr(flow), N.ptr(d0),
                                               N.ptr(d1), N.ptr(status), N.ptr(work), work.numel() if work is not None else 0,
                                               N.stream_ptr())
            N._check(rc, "lgn_emd_grad_opts_f64")
        else:
            rc = N.lib().lgn_emd_grad_f64(N.ptr(a), N.ptr(b), B, n, m, float(R), N.ptr(out), N.ptr(g0), N.ptr(g1), N.ptr(flow),
                                          N.ptr(d0), N.ptr(d1), N.ptr(status), N.ptr(work), work.numel() if work is not None else 0,
                                          N.stream_ptr())
            N._check(rc, "lgn_emd_grad_f64")
    if not return_status:
        st = status.cpu().numpy()
        bad = st.nonzero()[0]
        if len(bad):
            raise ValueError(f"emd: {status_message(int(st[bad[0]]), bool(norm))} (pair {int(bad[0])}, {len(bad)} pair(s) in all)")
    res = [out, g0, g1] + ([flow] if return_flow else []) + ([d0, d1] if return_duals else [])
    if single:
        res = [None if x is None else x[0] for x in res]
    if return_status:
        res.append(status[0] if single else status)
    return tuple(res)


def _relative_options(who: str, R, beta, norm, periodic_phi) -> Optional["N.EmdOpts"]:
    """None at the defaults (the calls without options then run), else the checked lgn_emd_opts"""
    if R == 1.0 and beta == 1.0 and not norm and not periodic_phi:
        return None
    return _options(who, R, beta, norm, periodic_phi)


def emd_relative_grad(recons: torch.Tensor, target: torch.Tensor, need_g_target: bool = False, R: float = 1.0, beta: float = 1.0,
                      norm: bool = False, periodic_phi: bool = False):
    """emd_relative_tensor() with its gradient with respect to the Cartesian jets, in one launch and with no host sync: returns
    (emd (B,), g_recons (B, N, 4), g_target (B, N, 4) or None, status (B,) int32).  The E column of the gradients is 0; a jet with a
    status bit has NaN gradients.  R, beta, norm, periodic_phi as in emd(), applied to the relative-polar frames; at their defaults
    the call is the one it always was, otherwise lgn_emd_relative_opts_f64 runs."""
    opts = _relative_options("emd_relative_grad", R, beta, norm, periodic_phi)
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
        if opts is not None:
            rc = N.lib().lgn_emd_relative_opts_f64(N.ptr(r), N.ptr(t), B, n, opts, N.ptr(out), N.ptr(g_r), N.ptr(g_t), N.ptr(status),
                                                   N.ptr(work), work.numel() if work is not None else 0, N.stream_ptr())
            N._check(rc, "lgn_emd_relative_opts_f64")
        else:
            rc = N.lib().lgn_emd_relative_grad_f64(N.ptr(r), N.ptr(t), B, n, N.ptr(out), N.ptr(g_r), N.ptr(g_t), N.ptr(status),
                                                   N.ptr(work), work.numel() if work is not None else 0, N.stream_ptr())
            N._check(rc, "lgn_emd_relative_grad_f64")
    return out, g_r, g_t, status


def _per_pair(g, grad):
    return grad * g.reshape(-1, 1, 1)


class EMDFn(torch.autograd.Function):
    """(ev0 (B,n,3), ev1 (B,m,3), R[, beta, norm, periodic_phi]) -> (B,) distances.  One launch in forward, which also returns the
    gradients for an upstream gradient of one; backward scales them per pair.  A pair with a status bit is NaN, value and gradients."""

    @staticmethod
    def forward(ctx, ev0, ev1, R, beta=1.0, norm=False, periodic_phi=False):
        need1 = bool(ctx.needs_input_grad[1])
        need0 = bool(ctx.needs_input_grad[0]) or not need1            # (the launch needs one gradient output at least)
        out, g0, g1, _ = emd_grad(ev0.detach(), ev1.detach(), R, return_status=True, need_g0=need0, need_g1=need1, beta=beta, norm=norm,
                                  periodic_phi=periodic_phi)
        ctx.has = (g0 is not None, g1 is not None)
        ctx.save_for_backward(*[g for g in (g0, g1) if g is not None])
        return out

    @staticmethod
    def backward(ctx, g):
        saved = list(ctx.saved_tensors)
        g0 = saved.pop(0) if ctx.has[0] else None
        g1 = saved.pop(0) if ctx.has[1] else None
        return ((_per_pair(g, g0) if ctx.needs_input_grad[0] else None), (_per_pair(g, g1) if ctx.needs_input_grad[1] else None), None,
                None, None, None)


class EMDRelativeFn(torch.autograd.Function):
    """(recons (B,N,4), target (B,N,4), owner[, R, beta, norm, periodic_phi]) -> (B,) distances on the relative-polar frames,
    emd_relative_tensor()'s bit for bit; the gradient of the target is computed only if the target needs one.  ``owner.status``
    receives the (B,) int32 flags."""

    @staticmethod
    def forward(ctx, recons, target, owner, R=1.0, beta=1.0, norm=False, periodic_phi=False):
        out, g_r, g_t, status = emd_relative_grad(recons.detach(), target.detach(), need_g_target=ctx.needs_input_grad[1], R=R, beta=beta,
                                                  norm=norm, periodic_phi=periodic_phi)
        if owner is not None:
            owner.status = status
        ctx.has_target = g_t is not None
        ctx.save_for_backward(*([g_r, g_t] if g_t is not None else [g_r]))
        return out

    @staticmethod
    def backward(ctx, g):
        saved = ctx.saved_tensors
        return ((_per_pair(g, saved[0]) if ctx.needs_input_grad[0] else None),
                (_per_pair(g, saved[1]) if ctx.has_target and ctx.needs_input_grad[1] else None), None, None, None, None, None)


def emd_differentiable(ev0: torch.Tensor, ev1: torch.Tensor, R: float = 1.0, beta: float = 1.0, norm: bool = False,
                       periodic_phi: bool = False) -> torch.Tensor:
    """emd() of (B, n, 3) against (B, m, 3) device tensors as a (B,) tensor with autograd (gradients with respect to pT, y and phi of
    both events), under emd()'s options.  No host sync: a pair with a status bit is NaN, value and gradients
    (emd_grad(return_status=True) shows the flags)."""
    if ev0.dim() != 3 or ev1.dim() != 3:
        raise ValueError(f"emd_differentiable takes events (B, n, 3) and (B, m, 3); got {tuple(ev0.shape)} and {tuple(ev1.shape)}")
    if beta == 1.0 and not norm and not periodic_phi:
        return EMDFn.apply(ev0, ev1, float(R))
    return EMDFn.apply(ev0, ev1, float(R), float(beta), bool(norm), bool(periodic_phi))


def emd_relative_tensor(recons: torch.Tensor, target: torch.Tensor, return_status: bool = False, R: float = 1.0, beta: float = 1.0,
                        norm: bool = False, periodic_phi: bool = False):
    """The reference's score "emd (relative coordinates)" of (B, N, 4) Cartesian device tensors as a (B,) fp64 device tensor, with no
    host sync (chain it after NativeEvalStep.run()): each jet is staged into its relative-polar frame (pT / (jet pT + 1e-16), eta - jet
    eta, wrapped phi - jet phi) exactly as the other 21 scores stage it, then energyflow.emd.emd(target_rel, recons_rel).  A jet with
    a status bit (see emd()) gets NaN; return_status=True also returns the (B,) int32 status.  R, beta, norm, periodic_phi: emd()'s
    options on the frames (the score itself is the defaults, at which the call is the one it always was)."""
    if recons.dim() != 3 or recons.shape[-1] != 4 or recons.shape != target.shape:
        raise ValueError(f"emd_relative_tensor takes two (B, N, 4) Cartesian tensors; got {tuple(recons.shape)} and {tuple(target.shape)}")
    B, n = int(recons.shape[0]), int(recons.shape[1])
    if not 1 <= n <= NMAX:
        raise ValueError(f"the EMD score supports 1 <= N <= {NMAX} particles per jet; got N = {n}")
    opts = _relative_options("emd_relative_tensor", R, beta, norm, periodic_phi)
    r, t = N.f64(recons.to(torch.float64)), N.f64(target.to(torch.float64))
    dev = r.device
    out = torch.empty(B, device=dev, dtype=torch.float64)
    status = torch.empty(B, device=dev, dtype=torch.int32)
    if B > 0:
        work = _workspace(B, n, dev)
        if opts is not None:
            rc = N.lib().lgn_emd_relative_opts_f64(N.ptr(r), N.ptr(t), B, n, opts, N.ptr(out), None, None, N.ptr(status), N.ptr(work),
                                                   work.numel() if work is not None else 0, N.stream_ptr())
            N._check(rc, "lgn_emd_relative_opts_f64")
        else:
            rc = N.lib().lgn_emd_relative_f64(N.ptr(r), N.ptr(t), B, n, N.ptr(out), N.ptr(status), N.ptr(work),
                                              work.numel() if work is not None else 0, N.stream_ptr())
            N._check(rc, "lgn_emd_relative_f64")
    return (out, status) if return_status else out


class EMDsFn(torch.autograd.Function):
    """emds() with autograd: forward is emds(); backward solves the pairs once more, in chunks of whole rows of the matrix, through
    emd_grad() and sums each side in a fixed order."""

    @staticmethod
    def forward(ctx, X0, X1, sym, R, beta, norm, periodic_phi, chunk_pairs):
        a = X0.detach()
        out, _ = emds(a, None if sym else X1.detach(), R=R, beta=beta, norm=norm, periodic_phi=periodic_phi, return_status=True)
        ctx.save_for_backward(a, a if sym else X1.detach())
        ctx.conf = (sym, R, beta, norm, periodic_phi, chunk_pairs)
        return out

    @staticmethod
    def backward(ctx, G):
        a, b = ctx.saved_tensors
        sym, R, beta, norm, periodic_phi, chunk_pairs = ctx.conf
        B0, B1, n, m = a.shape[0], b.shape[0], a.shape[1], b.shape[1]
        G = G.to(torch.float64)
        need0, need1 = ctx.needs_input_grad[0], (not sym and ctx.needs_input_grad[1])
        g_a = torch.zeros_like(a) if need0 else None
        g_b = torch.zeros(B1, m, 3, device=b.device, dtype=torch.float64) if (need1 or (sym and need0)) else None
        rows = max(1, chunk_pairs // max(B1, 1))
        for r0 in range(0, B0, rows):
            r1 = min(B0, r0 + rows)
            k = r1 - r0
            ea = a[r0:r1].unsqueeze(1).expand(k, B1, n, 3).reshape(k * B1, n, 3)
            eb = b.unsqueeze(0).expand(k, B1, m, 3).reshape(k * B1, m, 3)
            _, g0, g1, _ = emd_grad(ea, eb, R, return_status=True, need_g0=g_a is not None, need_g1=g_b is not None, beta=beta, norm=norm,
                                    periodic_phi=periodic_phi)
            w = G[r0:r1].reshape(k * B1, 1, 1)
            t0, t1 = (None if g0 is None else g0 * w), (None if g1 is None else g1 * w)
            if sym:                  # the diagonal is the constant 0 whatever the event holds: it gives nothing (not even a NaN)
                eye = (torch.arange(r0, r1, device=a.device).unsqueeze(1) == torch.arange(B1, device=a.device).unsqueeze(0)).view(-1, 1, 1)
                t0, t1 = t0.masked_fill(eye, 0.0), t1.masked_fill(eye, 0.0)
            if g_a is not None:
                g_a[r0:r1] = t0.reshape(k, B1, n, 3).sum(1)
            if g_b is not None:
                g_b += t1.reshape(k, B1, m, 3).sum(0)
        if sym:
            return (g_a + g_b if need0 else None), None, None, None, None, None, None, None
        return g_a, (g_b if need1 else None), None, None, None, None, None, None


class _Matrix:
    """The checked arguments of a matrix call: emds()'s shape and option checks, with its messages."""

    def __init__(self, who: str, X0, X1, R, beta, norm, periodic_phi):
        self.sym = X1 is None
        a, b = X0, (X0 if self.sym else X1)
        if a.dim() != 3 or b.dim() != 3 or a.shape[-1] != 3 or b.shape[-1] != 3:
            raise ValueError(f"emds takes events (B0, n, 3) and (B1, m, 3) of (pT, y, phi); got {tuple(a.shape)} and {tuple(b.shape)}")
        self.B0, self.B1, self.n, self.m = int(a.shape[0]), int(b.shape[0]), int(a.shape[1]), int(b.shape[1])
        if not (1 <= self.n <= NMAX and 1 <= self.m <= NMAX):
            raise ValueError(f"emd supports 1 <= n, m <= {NMAX} particles per event; got n = {self.n}, m = {self.m}")
        self.opts = _options("emds", R, beta, norm, periodic_phi)
        if not (a.is_cuda and b.is_cuda):
            raise RuntimeError(f"lgn (MI355X build): {who} runs only in the HIP kernels of liblgn_amd.so on a GPU device; got tensors "
                               f"on '{a.device}' and '{b.device}'. There is no CPU fallback.")
        self.a = N.f64(a.to(torch.float64))
        self.b = self.a if self.sym else N.f64(b.to(torch.float64))
        self.dev = self.a.device
        self.mode = UPPER if self.sym else FULL
        self.norm = bool(norm)

    def row_pairs(self, i: int) -> int:
        return self.B0 - 1 - i if self.sym else self.B1

    def pairs(self, r0: int, k: int) -> int:
        """the pairs of the rows [r0, r0 + k) of the matrix, by the library's plan-time query"""
        nbytes = N.lib().lgn_emd_pairs_grad_slab_bytes(self.mode, self.B0, self.B1, self.n, self.m, r0, k)
        if nbytes < 0:
            raise ValueError(N.last_error())
        return nbytes // (24 * (self.n + self.m))

    def chunks(self, max_slab_bytes: int):
        """whole rows in ascending order, as many per chunk as keep its two slabs within max_slab_bytes (one row at least)"""
        out, r0, per_pair = [], 0, 24 * (self.n + self.m)
        while r0 < self.B0:
            k, P = 1, self.row_pairs(r0)
            while r0 + k < self.B0 and (P + self.row_pairs(r0 + k)) * per_pair <= max_slab_bytes:
                P += self.row_pairs(r0 + k)
                k += 1
            out.append((r0, k))
            r0 += k
        return out

    def slabs(self, P: int):
        """(s0, s1) for P pairs (never zero-sized: the library refuses null pointers)"""
        return (torch.empty(max(P, 1), self.n, 3, device=self.dev, dtype=torch.float64),
                torch.empty(max(P, 1), self.m, 3, device=self.dev, dtype=torch.float64))

    def solve(self, r0, k, E, s0, s1, status, work):
        rc = N.lib().lgn_emd_pairs_grad_f64(N.ptr(self.a), None if self.sym else N.ptr(self.b), self.B0, self.B1, self.n, self.m, self.mode,
                                            self.opts, r0, k, N.ptr(E), N.ptr(s0), N.ptr(s1), N.ptr(status), N.ptr(work),
                                            work.numel() if work is not None else 0, N.stream_ptr())
        N._check(rc, "lgn_emd_pairs_grad_f64")

    def reduce(self, r0, k, s0, s1, G, g0, g1):
        rc = N.lib().lgn_emd_pairs_grad_reduce_f64(N.ptr(s0), N.ptr(s1), N.ptr(G), self.B0, self.B1, self.n, self.m, self.mode, r0, k,
                                                   N.ptr(g0), N.ptr(g1), N.stream_ptr())
        N._check(rc, "lgn_emd_pairs_grad_reduce_f64")

    def outputs(self, need0: bool = True, need1: bool = True):
        """(g0, g1): what the reduction writes; g1 is None in the symmetric form.  Without pairs the sums are empty: zeros."""
        make = torch.zeros if self.B0 * self.B1 == 0 else torch.empty
        g0 = make(self.B0, self.n, 3, device=self.dev, dtype=torch.float64) if need0 else None
        g1 = make(self.B1, self.m, 3, device=self.dev, dtype=torch.float64) if (need1 and not self.sym) else None
        return g0, g1

    def solve_and_reduce(self, G, E, status, g0, g1, max_slab_bytes: int):
        """row chunk after row chunk in ascending order: solve into one pair of slabs, sum them into g0 and g1"""
        if self.B0 * self.B1 == 0:
            return
        chunks = self.chunks(max_slab_bytes)
        P = max(self.pairs(r0, k) for r0, k in chunks)
        s0, s1 = self.slabs(P)
        work = _pairs_workspace(max(P, 1), max(self.n, self.m), self.dev)
        for r0, k in chunks:
            self.solve(r0, k, E, s0, s1, status, work)
            self.reduce(r0, k, s0, s1, G, g0, g1)


def _upstream(who: str, G, M: "_Matrix") -> Optional[torch.Tensor]:
    if G is None:
        return None
    if tuple(G.shape) != (M.B0, M.B1):
        raise ValueError(f"{who}: the upstream matrix G is {tuple(G.shape)}; the matrix of distances is ({M.B0}, {M.B1})")
    if not G.is_cuda:
        raise RuntimeError(f"lgn (MI355X build): {who} runs only in the HIP kernels of liblgn_amd.so on a GPU device; got G on "
                           f"'{G.device}'. There is no CPU fallback.")
    return N.f64(G.to(torch.float64))


def emds_pair_grads(X0: torch.Tensor, X1: Optional[torch.Tensor] = None, R: float = 1.0, beta: float = 1.0, norm: bool = False,
                    periodic_phi: bool = False):
    """emds() with the gradient of every pair, each pair solved once in one launch (csrc/emd_pairs_grad.hip): returns
    (E (B0, B1), s0 (P, n, 3), s1 (P, m, 3), status (B0, B1) int32).  Row p of the slabs is pair number p of the matrix -- p = i B1 + j,
    or, with X1=None, the pairs i < j row-major over the upper triangle -- and holds d E[i, j] / d X0[i] and d E[i, j] / d X1[j] in the
    column order (pT, y, phi), with the bits emd_grad() gives for that ordered pair; E has emds()'s bits.  A pair with a status bit is
    NaN, value and gradients.  No host sync.  The slabs take P (n + m) 24 bytes: emds_grad() sums them in chunks of rows."""
    M = _Matrix("emds_pair_grads", X0, X1, R, beta, norm, periodic_phi)
    E = torch.empty(M.B0, M.B1, device=M.dev, dtype=torch.float64)
    status = torch.empty(M.B0, M.B1, device=M.dev, dtype=torch.int32)
    P = M.pairs(0, M.B0) if M.B0 * M.B1 else 0
    s0, s1 = M.slabs(P)
    if M.B0 * M.B1:
        M.solve(0, M.B0, E, s0, s1, status, _pairs_workspace(max(P, 1), max(M.n, M.m), M.dev))
    return E, s0[:P], s1[:P], status


def emds_grad(X0: torch.Tensor, X1: Optional[torch.Tensor] = None, G: Optional[torch.Tensor] = None, R: float = 1.0, beta: float = 1.0,
              norm: bool = False, periodic_phi: bool = False, return_status: bool = False, max_slab_bytes: int = 2 ** 30):
    """emds() with the gradient of sum(G * E): returns (E (B0, B1), g0 (B0, n, 3), g1 (B1, m, 3)[, status]), g0 = d sum(G E) / d X0 and
    g1 = d sum(G E) / d X1; G (B0, B1) is the upstream matrix, None is all ones.  X1=None is the symmetric form: g1 is None and g0
    holds an event's share from both of its roles (pair i < j weighs G[i, j] + G[j, i]; the diagonal gives nothing).  Every pair is
    solved once; whole rows of the matrix are solved and summed at a time, as many as keep the per-pair gradients within
    max_slab_bytes (one row at least).  The sums run in a fixed order, one rounded product and one rounded sum per pair, partners
    ascending (include/lgn_amd.h): the bits do not depend on max_slab_bytes or on the run.  A pair with a status bit is NaN in E and
    makes the gradients of both its events NaN whatever G holds there; ValueError and return_status as in emds()."""
    M = _Matrix("emds_grad", X0, X1, R, beta, norm, periodic_phi)
    G = _upstream("emds_grad", G, M)
    E = torch.empty(M.B0, M.B1, device=M.dev, dtype=torch.float64)
    status = torch.empty(M.B0, M.B1, device=M.dev, dtype=torch.int32)
    g0, g1 = M.outputs()
    M.solve_and_reduce(G, E, status, g0, g1, int(max_slab_bytes))
    if not return_status:
        bad = status.nonzero().cpu().numpy()
        if len(bad):
            i, j = int(bad[0][0]), int(bad[0][1])
            raise ValueError(f"emds_grad: {status_message(int(status[i, j].item()), M.norm)} (pair ({i}, {j}), {len(bad)} pair(s) in all)")
    return (E, g0, g1, status) if return_status else (E, g0, g1)


class EMDsNativeFn(torch.autograd.Function):
    """emds() with autograd on the matrix-gradient kernels.  When the per-pair gradients of the whole matrix fit keep_bytes, forward
    is the launch that solves and differentiates every pair and backward is the weighted sum alone; otherwise forward is emds() and
    backward solves and sums chunk after chunk of rows."""

    @staticmethod
    def forward(ctx, X0, X1, sym, R, beta, norm, periodic_phi, keep_bytes, max_slab_bytes):
        a = X0.detach()
        b = None if sym else X1.detach()
        M = _Matrix("emds_differentiable", a, b, R, beta, norm, periodic_phi)
        ctx.conf = (sym, R, beta, norm, periodic_phi, max_slab_bytes)
        ctx.kept = 24 * (M.n + M.m) * (M.pairs(0, M.B0) if M.B0 * M.B1 else 0) <= keep_bytes
        if ctx.kept:
            out, s0, s1, _ = emds_pair_grads(a, b, R=R, beta=beta, norm=norm, periodic_phi=periodic_phi)
            ctx.save_for_backward(M.a, M.b, s0, s1)
        else:
            out, _ = emds(a, b, R=R, beta=beta, norm=norm, periodic_phi=periodic_phi, return_status=True)
            ctx.save_for_backward(M.a, M.b)
        return out

    @staticmethod
    def backward(ctx, G):
        sym, R, beta, norm, periodic_phi, max_slab_bytes = ctx.conf
        saved = ctx.saved_tensors
        M = _Matrix("emds_differentiable", saved[0], None if sym else saved[1], R, beta, norm, periodic_phi)
        G = N.f64(G.to(torch.float64))
        g0, g1 = M.outputs(bool(ctx.needs_input_grad[0]), bool(ctx.needs_input_grad[1]))
        if g0 is None and g1 is None:
            return (None,) * 9
        if ctx.kept:
            if M.B0 * M.B1:
                s0, s1 = M.slabs(0) if saved[2].shape[0] == 0 else (saved[2], saved[3])
                M.reduce(0, M.B0, s0, s1, G, g0, g1)
        else:
            M.solve_and_reduce(G, None, None, g0, g1, max_slab_bytes)
        return (g0, g1) + (None,) * 7


def emds_differentiable(X0: torch.Tensor, X1: Optional[torch.Tensor] = None, R: float = 1.0, beta: float = 1.0, norm: bool = False,
                        periodic_phi: bool = False, chunk_pairs: int = 65536, backward: str = "rows",
                        keep_bytes: int = 2 ** 30) -> torch.Tensor:
    """emds() as a (B0, B1) tensor with autograd (gradients with respect to pT, y and phi of every event); the value has emds()'s
    bits, with no host sync (a pair with a status bit is NaN, value and gradients).  X1=None is the symmetric form: X0 receives its
    share from both of its roles, the diagonal gives nothing.  ``backward`` chooses how the gradient is made:
    "rows" (the default) is the composition over emd_grad(): forward is emds(), backward solves the pairs again, whole rows of the
    matrix at a time, at most max(chunk_pairs, B1) pairs per chunk, whose gathered events and whose gradients take that many times
    (n + m) * 3 doubles of scratch each, and sums each side with one reshaped sum per chunk (over the columns for X0, over the rows for
    X1), an order that does not depend on the run.  The symmetric form solves every pair i != j in both orders.
    "native" runs the matrix-gradient kernels (emds_pair_grads(), emds_grad()): no gathered events, every pair solved in one order
    only.  When the per-pair gradients of the whole matrix, P (n + m) 24 bytes, fit keep_bytes, forward solves and differentiates
    every pair in one launch and keeps them, and backward is the weighted sum alone: one solve per pair in all.  Otherwise forward is
    emds() and backward solves and sums at most max(chunk_pairs, one row) pairs at a time: two solves per pair and chunk_pairs
    (n + m) 24 bytes of scratch.  Its sums run in emds_grad()'s fixed order: the bits depend neither on keep_bytes, nor on
    chunk_pairs, nor on the run."""
    sym = X1 is None
    if backward == "rows":
        return EMDsFn.apply(X0, X0 if sym else X1, sym, float(R), float(beta), bool(norm), bool(periodic_phi), int(chunk_pairs))
    if backward != "native":
        raise ValueError(f"emds_differentiable: backward is 'rows' or 'native'; got {backward!r}")
    per_pair = 24 * (int(X0.shape[-2]) + int((X0 if sym else X1).shape[-2])) if X0.dim() == 3 and (sym or X1.dim() == 3) else 0
    return EMDsNativeFn.apply(X0, X0 if sym else X1, sym, float(R), float(beta), bool(norm), bool(periodic_phi), int(keep_bytes),
                              int(chunk_pairs) * per_pair)


def max_augmentations(reset: bool = True) -> int:
    """Debug counter: the largest number of augmentations any pair needed since the last reset (waits for the device)."""
    import ctypes
    v = ctypes.c_int(0)
    N._check(N.lib().lgn_emd_debug_max_augmentations(ctypes.byref(v), int(reset)), "lgn_emd_debug_max_augmentations")
    return v.value
