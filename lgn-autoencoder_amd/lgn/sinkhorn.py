"""
Entropic optimal transport and the Sinkhorn divergence on the GPU: the smooth, regularised relative of the exact energy mover's
distance of lgn.emd, solved by Sinkhorn iterations in the log domain (csrc/sinkhorn.hip, one wavefront per pair of events).

    OT_eps(a, b) = min over P of <P, C> + eps KL(P | a (x) b / S)
    f_i <- -eps log sum_j (b_j / S) exp((g_j - C_ij) / eps),   g_j <- -eps log sum_i (a_i / S) exp((f_i - C_ij) / eps),   from g = 0

on the EMD's extended problem: the cost C and the staging are lgn.emd.emd()'s under R, beta, norm and periodic_phi, the lighter event
gets the EMD's fictitious particle (none under norm).  The value is E = <a, f> + <b, g>, a lower bound of OT_eps that is tight when
the iteration has converged; EMD <= OT_eps <= EMD + eps S log(S / w_min).  The gradient with respect to positions and weights is the
EMD's closed form with the optimal flow replaced by the plan P and the LP's potentials by (f, g) (envelope theorem), from the same
launch; it is smooth where the LP's gradient jumps from one optimal basis to the next.  ``debias=True`` is the Sinkhorn divergence
OT_eps(x, y) - OT_eps(x, x) / 2 - OT_eps(y, y) / 2, which is zero for equal events.  include/lgn_amd.h is the specification
(energyflow, POT and geomloss were not available when this was written; tests/_sinkhorn_ref.py restates the definition in numpy).

The iteration stops when the row-marginal violation err falls to tol * S, or after max_iter iterations; a pair that misses a
positive tol gets the status bit ITER and still delivers value and gradients.  ``lgn.losses.SinkhornLoss`` is the training loss on
top of ``sinkhorn_relative_tensor``.

What is NOT offered: the loss as a stage inside the whole-step native calls (the native step classes refuse the module;
``native_train_step`` then returns a CapturedModuleStep), epsilon scaling (annealing), an all-pairs matrix form, unbalanced
(KL-relaxed) marginals.  There is no CPU fallback.
"""
import torch

from . import _native as N

NMAX = N.EMD_NMAX
INVALID, EMPTY, ITER = N.EMD_INVALID, N.EMD_EMPTY, N.SINKHORN_ITER


def status_message(s: int, norm: bool = False) -> str:
    if s & INVALID:
        return "events hold NaN, infinity or a negative weight"
    if s & EMPTY:
        return "an event is weightless and cannot be normalised" if norm else "both events are weightless"
    if s & ITER:
        return "the Sinkhorn iteration stopped at max_iter with a marginal error above tol"
    return "no status bit is set"


def _options(who: str, epsilon, max_iter, tol, debias, R, beta, norm, periodic_phi) -> "N.SinkhornOpts":
    from .emd import _options as emd_options
    base = emd_options(who, R, beta, norm, periodic_phi)
    if not (epsilon > 0 and epsilon < float("inf")):
        raise ValueError(f"{who} needs a finite epsilon > 0; got {epsilon}")
    if not (tol >= 0 and tol < float("inf")):
        raise ValueError(f"{who} needs a finite tol >= 0; got {tol}")
    if int(max_iter) != max_iter or max_iter < 1:
        raise ValueError(f"{who} needs an integer max_iter >= 1; got {max_iter}")
    return N.SinkhornOpts(base, float(epsilon), float(tol), int(max_iter), int(bool(debias)))


def cost_in_lds(n: int, m: int) -> bool:
    """Plan-time query: is the scaled cost matrix of events of n and m particles kept in LDS (else recomputed in every sweep)?"""
    nbytes = N.lib().lgn_sinkhorn_lds_bytes(n, m)
    if nbytes < 0:
        raise ValueError(N.last_error())
    R = max(n, m) + 1
    return nbytes >= 8 * R * R


def _events(who: str, ev0, ev1):
    single = ev0.dim() == 2
    a, b = (ev0.unsqueeze(0), ev1.unsqueeze(0)) if single else (ev0, ev1)
    if a.dim() != 3 or b.dim() != 3 or a.shape[-1] != 3 or b.shape[-1] != 3 or a.shape[0] != b.shape[0]:
        raise ValueError(f"{who} takes events (B, n, 3) and (B, m, 3) of (pT, y, phi); got {tuple(ev0.shape)} and {tuple(ev1.shape)}")
    n, m = int(a.shape[1]), int(b.shape[1])
    if not (1 <= n <= NMAX and 1 <= m <= NMAX):
        raise ValueError(f"{who} supports 1 <= n, m <= {NMAX} particles per event; got n = {n}, m = {m}")
    return single, a, b


def _device(who: str, a, b):
    if not (a.is_cuda and b.is_cuda):
        raise RuntimeError(f"lgn (MI355X build): {who} runs only in the HIP kernels of liblgn_amd.so on a GPU device; got tensors on "
                           f"'{a.device}' and '{b.device}'. There is no CPU fallback.")


def _raise_on_status(who: str, status, norm):
    st = status.cpu().numpy()
    bad = st.nonzero()[0]
    if len(bad):
        raise ValueError(f"{who}: {status_message(int(st[bad[0]]), bool(norm))} (pair {int(bad[0])}, {len(bad)} pair(s) in all)")


def _call(who, a, b, opts, need_g0, need_g1, potentials, plan):
    """one launch of lgn_sinkhorn_f64: (value, g0, g1, f, g, plan, iters, err, status), what was not asked for is None"""
    B, n, m = int(a.shape[0]), int(a.shape[1]), int(b.shape[1])
    a, b = N.f64(a.to(torch.float64)), N.f64(b.to(torch.float64))
    dev = a.device

    def new(*shape, dtype=torch.float64):
        return torch.empty(*shape, device=dev, dtype=dtype)
    value, status, iters, err = new(B), new(B, dtype=torch.int32), new(B, dtype=torch.int32), new(B)
    g0 = new(B, n, 3) if need_g0 else None
    g1 = new(B, m, 3) if need_g1 else None
    f = new(B, n + 1) if potentials else None
    g = new(B, m + 1) if potentials else None
    P = new(B, n + 1, m + 1) if plan else None
    if B > 0:
        rc = N.lib().lgn_sinkhorn_f64(N.ptr(a), N.ptr(b), B, n, m, opts, N.ptr(value), N.ptr(g0), N.ptr(g1), N.ptr(f), N.ptr(g), N.ptr(P),
                                      N.ptr(iters), N.ptr(err), N.ptr(status), N.stream_ptr())
        N._check(rc, "lgn_sinkhorn_f64")
    return value, g0, g1, f, g, P, iters, err, status


def sinkhorn(ev0: torch.Tensor, ev1: torch.Tensor, epsilon: float, max_iter: int = 200, tol: float = 1e-6, debias: bool = False,
             R: float = 1.0, beta: float = 1.0, norm: bool = False, periodic_phi: bool = False, return_potentials: bool = False,
             return_plan: bool = False, return_info: bool = False, return_status: bool = False):
    """The entropic transport value of events of (pT, y, phi) particles: ev0 (B, n, 3) against ev1 (B, m, 3) device tensors (or one
    (n, 3) against one (m, 3)), n != m allowed, 1 <= n, m <= 191.  Returns the (B,) fp64 device tensor of values (a 0-dim tensor for
    one pair); with return_potentials also f (B, n + 1) and g (B, m + 1), with return_plan the plan (B, n + 1, m + 1) -- row n and
    column m are the fictitious particle that carries the weight difference -- and with return_info the applied iterations (B,) int32
    and the final marginal error (B,).  With debias the value is the Sinkhorn divergence; potentials, plan, iterations and error
    still refer to the cross term.  Raises ValueError when a pair has a status bit (NaN, infinity or a negative weight; weightless
    events; a positive tol that max_iter iterations did not reach -- that pair's value is still delivered); return_status=True
    returns the (B,) int32 status last instead and does not wait for the device.
    R, beta, norm, periodic_phi: the cost and the weights of lgn.emd.emd()."""
    single, a, b = _events("sinkhorn", ev0, ev1)
    opts = _options("sinkhorn", epsilon, max_iter, tol, debias, R, beta, norm, periodic_phi)
    _device("sinkhorn", a, b)
    value, _, _, f, g, P, iters, err, status = _call("sinkhorn", a, b, opts, False, False, return_potentials, return_plan)
    if not return_status:
        _raise_on_status("sinkhorn", status, norm)
    res = [value] + ([f, g] if return_potentials else []) + ([P] if return_plan else []) + ([iters, err] if return_info else [])
    if return_status:
        res.append(status)
    if single:
        res = [x[0] for x in res]
    return res[0] if len(res) == 1 else tuple(res)


def sinkhorn_grad(ev0: torch.Tensor, ev1: torch.Tensor, epsilon: float, max_iter: int = 200, tol: float = 1e-6, debias: bool = False,
                  R: float = 1.0, beta: float = 1.0, norm: bool = False, periodic_phi: bool = False, need_g0: bool = True,
                  need_g1: bool = True, return_potentials: bool = False, return_plan: bool = False, return_info: bool = False,
                  return_status: bool = False):
    """sinkhorn() with its gradients, in one launch: returns (value (B,), g0 (B, n, 3), g1 (B, m, 3)[, f, g][, plan][, iters, err]
    [, status]) -- g0 = d value / d ev0 and g1 = d value / d ev1 in the events' column order (pT, y, phi); a gradient that is not
    needed is None.  The value is sinkhorn()'s bit for bit.  A pair flagged INVALID or EMPTY has NaN gradients; a pair flagged ITER
    has the gradients of the state the iteration reached.  ValueError and return_status as in sinkhorn()."""
    single, a, b = _events("sinkhorn_grad", ev0, ev1)
    opts = _options("sinkhorn_grad", epsilon, max_iter, tol, debias, R, beta, norm, periodic_phi)
    if not (need_g0 or need_g1):
        raise ValueError("sinkhorn_grad: at least one of the two gradients must be asked for (sinkhorn() is the call without gradients)")
    _device("sinkhorn_grad", a, b)
    value, g0, g1, f, g, P, iters, err, status = _call("sinkhorn_grad", a, b, opts, need_g0, need_g1, return_potentials, return_plan)
    if not return_status:
        _raise_on_status("sinkhorn_grad", status, norm)
    res = [value, g0, g1] + ([f, g] if return_potentials else []) + ([P] if return_plan else []) + ([iters, err] if return_info else [])
    if return_status:
        res.append(status)
    if single:
        res = [None if x is None else x[0] for x in res]
    return tuple(res)


def sinkhorn_relative_grad(recons: torch.Tensor, target: torch.Tensor, epsilon: float, max_iter: int = 200, tol: float = 1e-6,
                           debias: bool = False, R: float = 1.0, beta: float = 1.0, norm: bool = False, periodic_phi: bool = False,
                           need_grad: bool = True, need_g_target: bool = False):
    """The value on the relative-polar frames of (B, N, 4) Cartesian jets with its gradient with respect to the jets, in one launch and
    with no host sync: returns (value (B,), g_recons (B, N, 4) or None, g_target (B, N, 4) or None, iters (B,) int32, err (B,),
    status (B,) int32).  The E column of the gradients is 0."""
    opts = _options("sinkhorn_relative_grad", epsilon, max_iter, tol, debias, R, beta, norm, periodic_phi)
    if recons.dim() != 3 or recons.shape[-1] != 4 or recons.shape != target.shape:
        raise ValueError(f"sinkhorn_relative_grad takes two (B, N, 4) Cartesian tensors; got {tuple(recons.shape)} and "
                         f"{tuple(target.shape)}")
    B, n = int(recons.shape[0]), int(recons.shape[1])
    if not 1 <= n <= NMAX:
        raise ValueError(f"sinkhorn supports 1 <= N <= {NMAX} particles per jet; got N = {n}")
    if need_g_target and not need_grad:
        raise ValueError("sinkhorn_relative_grad: need_g_target without need_grad")
    _device("sinkhorn_relative_grad", recons, target)
    r, t = N.f64(recons.to(torch.float64)), N.f64(target.to(torch.float64))
    dev = r.device
    value = torch.empty(B, device=dev, dtype=torch.float64)
    err = torch.empty(B, device=dev, dtype=torch.float64)
    status = torch.empty(B, device=dev, dtype=torch.int32)
    iters = torch.empty(B, device=dev, dtype=torch.int32)
    g_r = torch.empty(B, n, 4, device=dev, dtype=torch.float64) if need_grad else None
    g_t = torch.empty(B, n, 4, device=dev, dtype=torch.float64) if need_g_target else None
    if B > 0:
        rc = N.lib().lgn_sinkhorn_relative_f64(N.ptr(r), N.ptr(t), B, n, opts, N.ptr(value), N.ptr(g_r), N.ptr(g_t), N.ptr(iters),
                                               N.ptr(err), N.ptr(status), N.stream_ptr())
        N._check(rc, "lgn_sinkhorn_relative_f64")
    return value, g_r, g_t, iters, err, status


def sinkhorn_relative_tensor(recons: torch.Tensor, target: torch.Tensor, epsilon: float, max_iter: int = 200, tol: float = 1e-6,
                             debias: bool = False, R: float = 1.0, beta: float = 1.0, norm: bool = False, periodic_phi: bool = False,
                             return_info: bool = False, return_status: bool = False):
    """The value of (B, N, 4) Cartesian device tensors as a (B,) fp64 device tensor, with no host sync: each jet is staged into its
    relative-polar frame exactly as lgn.emd.emd_relative_tensor() stages it.  A jet flagged INVALID or EMPTY gets NaN.  return_info
    adds the iterations and the marginal error, return_status the (B,) int32 status."""
    value, _, _, iters, err, status = sinkhorn_relative_grad(recons, target, epsilon, max_iter, tol, debias, R, beta, norm, periodic_phi,
                                                             need_grad=False)
    res = [value] + ([iters, err] if return_info else []) + ([status] if return_status else [])
    return res[0] if len(res) == 1 else tuple(res)


def _per_pair(g, grad):
    return grad * g.reshape(-1, 1, 1)


class SinkhornFn(torch.autograd.Function):
    """(ev0 (B,n,3), ev1 (B,m,3), opts) -> (B,) values.  One launch in forward, which also returns the gradients for an upstream
    gradient of one; backward scales them per pair."""

    @staticmethod
    def forward(ctx, ev0, ev1, opts):
        need1 = bool(ctx.needs_input_grad[1])
        need0 = bool(ctx.needs_input_grad[0]) or not need1
        out, g0, g1 = _call("sinkhorn_differentiable", ev0.detach(), ev1.detach(), opts, need0, need1, False, False)[:3]
        ctx.has = (g0 is not None, g1 is not None)
        ctx.save_for_backward(*[g for g in (g0, g1) if g is not None])
        return out

    @staticmethod
    def backward(ctx, g):
        saved = list(ctx.saved_tensors)
        g0 = saved.pop(0) if ctx.has[0] else None
        g1 = saved.pop(0) if ctx.has[1] else None
        return ((_per_pair(g, g0) if ctx.needs_input_grad[0] else None), (_per_pair(g, g1) if ctx.needs_input_grad[1] else None), None)


class SinkhornRelativeFn(torch.autograd.Function):
    """(recons (B,N,4), target (B,N,4), owner, keyword tuple) -> (B,) values on the relative-polar frames,
    sinkhorn_relative_tensor()'s bit for bit; the gradient of the target is computed only if the target needs one.  ``owner``
    receives .status, .iters and .err of the launch."""

    @staticmethod
    def forward(ctx, recons, target, owner, conf):
        epsilon, max_iter, tol, debias, R, beta, norm, periodic_phi = conf
        out, g_r, g_t, iters, err, status = sinkhorn_relative_grad(recons.detach(), target.detach(), epsilon, max_iter, tol, debias, R,
                                                                   beta, norm, periodic_phi, need_g_target=ctx.needs_input_grad[1])
        if owner is not None:
            owner.status, owner.iters, owner.err = status, iters, err
        ctx.has_target = g_t is not None
        ctx.save_for_backward(*([g_r, g_t] if g_t is not None else [g_r]))
        return out

    @staticmethod
    def backward(ctx, g):
        saved = ctx.saved_tensors
        return ((_per_pair(g, saved[0]) if ctx.needs_input_grad[0] else None),
                (_per_pair(g, saved[1]) if ctx.has_target and ctx.needs_input_grad[1] else None), None, None)


def sinkhorn_differentiable(ev0: torch.Tensor, ev1: torch.Tensor, epsilon: float, max_iter: int = 200, tol: float = 1e-6,
                            debias: bool = False, R: float = 1.0, beta: float = 1.0, norm: bool = False,
                            periodic_phi: bool = False) -> torch.Tensor:
    """sinkhorn() of (B, n, 3) against (B, m, 3) device tensors as a (B,) tensor with autograd (gradients with respect to pT, y and
    phi of both events).  No host sync: a pair flagged INVALID or EMPTY is NaN, value and gradients
    (sinkhorn_grad(return_status=True) shows the flags)."""
    if ev0.dim() != 3 or ev1.dim() != 3:
        raise ValueError(f"sinkhorn_differentiable takes events (B, n, 3) and (B, m, 3); got {tuple(ev0.shape)} and {tuple(ev1.shape)}")
    _, a, b = _events("sinkhorn_differentiable", ev0, ev1)
    opts = _options("sinkhorn_differentiable", epsilon, max_iter, tol, debias, R, beta, norm, periodic_phi)
    _device("sinkhorn_differentiable", a, b)
    return SinkhornFn.apply(ev0, ev1, opts)
