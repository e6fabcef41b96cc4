"""Losses of the training step as native operators.

``ChamferLoss`` is the drop-in of the reference's ``utils.losses.ChamferLoss`` (utils/losses/chamfer_loss/chamfer_loss.py:7-31,
cdist of distance_sq.py:263-304 with its default even p: the plain sum of squared component differences): same constructor, same
``forward(x, y, jet_features=False)``, one HIP kernel (csrc/net_kernels.hip: chamfer_kernel) for the loss and both gradients
instead of ~25 elementwise / reduction launches.  ``lgn.step.NativeTrainStep`` does not use it -- there the loss is the tail of the
decoder's last kernel.

``HungarianMSELoss`` is the drop-in of ``utils.losses.HungarianMSELoss`` (utils/losses/hungarian_mse/hungarian_mse.py:8-84): the four
coordinate frames, the assignment (scipy's ``linear_sum_assignment``, ties included, solved by one wavefront per jet), the MSE of the
paired rows and its gradient in one HIP kernel (csrc/assign_loss.hip) -- no copy of the cost matrices to the host, no Python loop
over the jets, capturable into a graph.

``EMDLoss`` and ``HybridLoss`` have the interface of ``utils.losses.EMDLoss`` and of get_loss()'s hybrid branch, on the exact
energy mover's distance of lgn.emd (csrc/emd.hip: the transportation LP and its closed-form gradient in one launch) -- not jetnet's
regularised QP.  Both take energyflow's R, beta, norm and periodic_phi as keywords (csrc/emd_grad_opts.hip).  No --loss-choice string selects them (``loss_kind`` keeps refusing 'emd' and 'hybrid'): pass an instance as
``loss_choice`` to the module-API steps of lgn.step, or -- with ``native_emd=True`` -- to NativeTrainStep / NativeEvalStep /
native_train_step / native_eval_step, where the EMD then runs as the step's loss stage (csrc/emd_loss.hip: the same per-jet value bit
for bit; HybridLoss on top of the step's own Chamfer loss) and the module's ``status`` is the step's status buffer.  ``native_emd``
defaults to False only because tests pin the refusal of loss modules by the native steps; a later change flips it.

``SinkhornLoss`` has ``EMDLoss``'s interface on the entropic relative of that distance (lgn.sinkhorn, csrc/sinkhorn.hip: Sinkhorn
iterations in the log domain, by default the debiased Sinkhorn divergence): a smooth loss for the module-API steps.  It is not a stage
of the whole-step native calls: the native step classes refuse it and ``native_train_step`` returns a CapturedModuleStep for it."""
from typing import Optional

import torch
from torch import nn

from . import _native as N


class ChamferFn(torch.autograd.Function):
    """(x (B,N,4), y (B,M,4), jet_features) -> scalar loss.  The kernel returns the gradients for an upstream gradient of one;
    backward scales them."""

    @staticmethod
    def forward(ctx, x, y, jet_features):
        part, gx, gy = N.chamfer(x.detach(), y.detach(), jet_features)
        ctx.save_for_backward(gx, gy)
        return part.sum()

    @staticmethod
    def backward(ctx, g):
        gx, gy = ctx.saved_tensors
        return (gx * g if ctx.needs_input_grad[0] else None), (gy * g if ctx.needs_input_grad[1] else None), None


class ChamferLoss(nn.Module):
    """utils/losses/chamfer_loss/chamfer_loss.py:7-31.  x, y: real 4-vectors (..., N, 4) / (..., M, 4) with the same leading
    batch shape; returns sum over the batch of (sum_i min_j d_ij + sum_j min_i d_ij) / 2, plus nn.MSELoss() of the summed
    momenta when ``jet_features``."""

    def __init__(self, device: Optional[torch.device] = None):
        super().__init__()
        self.device = device if device is not None else torch.device("cuda" if torch.cuda.is_available() else "cpu")

    def forward(self, x: torch.Tensor, y: torch.Tensor, jet_features: bool = False):
        x, y = x.to(self.device), y.to(self.device)
        if x.shape[-1] != 4 or y.shape[-1] != 4:
            raise ValueError(f"x and y must be 4-vectors. Found: {x.shape[-1]=} and {y.shape[-1]=}.")     # (3-vectors: reference only)
        if x.device.type != "cuda":
            raise RuntimeError("lgn (MI355X build): ChamferLoss runs only in the HIP kernels of liblgn_amd.so on a GPU device; "
                               f"got tensors on '{x.device}'. There is no CPU fallback.")
        if x.dim() == 2 and y.dim() == 2:                       # one unbatched jet (N, 4): the reference's formula takes it as it is
            x, y = x.unsqueeze(0), y.unsqueeze(0)
        if x.shape[:-2] != y.shape[:-2] or x.dim() < 3:
            raise ValueError(f"x {tuple(x.shape)} and y {tuple(y.shape)} must share their batch shape")
        if x.shape[-2] != y.shape[-2]:
            # the reference adds the (..., N) row minima to the (..., M) column minima elementwise (chamfer_loss.py:20-23): N != M
            # raises there (or silently broadcasts when one of them is 1).  The kernel itself handles N != M (lgn_chamfer_f64).
            raise RuntimeError(f"The size of tensor a ({x.shape[-2]}) must match the size of tensor b ({y.shape[-2]}) at non-singleton "
                               "dimension 1 (the reference's ChamferLoss takes sets of equal size)")
        return ChamferFn.apply(x.reshape(-1, x.shape[-2], 4), y.reshape(-1, y.shape[-2], 4), jet_features)


def loss_kind(loss_choice: str) -> int:
    """LGN_LOSS_* of a --loss-choice string, matched as get_loss() matches it (utils/train.py:416-480: lower-cased, tests in the
    reference's order).  EMD and the hybrid loss need jetnet / energyflow, which this build does not have: refused by name."""
    c = str(loss_choice).lower()
    if "chamfer" in c:
        return N.LOSS_CHAMFER
    if "emd" in c or c in ("hybrid", "combined", "mix"):
        raise NotImplementedError(f"loss choice ({loss_choice}): the EMD and hybrid losses are not implemented in this build. "
                                  "The available options are ('chamfer', 'mse', 'hungarian')")
    if "mse" in c:
        return N.LOSS_MSE
    if "jet" in c or "hungarian" in c:
        return N.LOSS_HUNGARIAN
    raise NotImplementedError(f"Current loss choice ({loss_choice}) is not implemented. "
                              "The available options are ('chamfer', 'mse', 'hungarian')")


def loss_columns(kind: int, abs_coord: bool = True, polar_coord: bool = False) -> int:
    """D: columns the mean of the loss runs over (4: MSE and the absolute Cartesian frame; 3: the (pt, eta, phi)-derived frames)."""
    return 4 if kind == N.LOSS_MSE or (abs_coord and not polar_coord) else 3


class HungarianMSEFn(torch.autograd.Function):
    """(recons (B,N,4), target (B,N,4), abs_coord, polar_coord, owner) -> scalar loss; the assignment carries no gradient, and
    neither does the target (as in the reference, whose target is data)."""

    @staticmethod
    def forward(ctx, x, y, abs_coord, polar_coord, owner):
        part, gx, assignment, status = N.hungarian_mse(x.detach(), y.detach(), N.LOSS_HUNGARIAN, abs_coord, polar_coord)
        ctx.save_for_backward(gx)
        owner._assignment, owner.status = assignment, status
        return part.sum()

    @staticmethod
    def backward(ctx, g):
        (gx,) = ctx.saved_tensors
        return (gx * g if ctx.needs_input_grad[0] else None), None, None, None, None


class HungarianMSELoss(nn.Module):
    """utils/losses/hungarian_mse/hungarian_mse.py:8-44.  recons, target: real 4-vectors (B, N, 4); returns the mean over
    (B, N, D) of (p[col[r]] - q[r])^2 in the chosen frame.  After a forward, ``assignment`` (B, N) int64 -- col of every jet -- and
    ``status`` (B,) int32 (non-zero: that jet's cost matrix held NaN / -inf or was infeasible; its term is NaN) are readable."""

    def __init__(self):
        super().__init__()
        self._assignment = self.status = None

    @property
    def assignment(self):
        return None if self._assignment is None else self._assignment.long()

    def forward(self, recons: torch.Tensor, target: torch.Tensor, abs_coord: bool = True, polar_coord: bool = False):
        self.abs_coord, self.polar_coord, self.device = abs_coord, polar_coord, recons.device
        target = target.to(recons.device)
        if recons.shape[-1] != 4 or target.shape[-1] != 4:
            raise ValueError(f"Wrong last dimension of p. Should be 4 but found: {recons.shape[-1]} / {target.shape[-1]} "
                             "(3-vectors: reference only).")
        if recons.device.type != "cuda":
            raise RuntimeError("lgn (MI355X build): HungarianMSELoss runs only in the HIP kernels of liblgn_amd.so on a GPU device; "
                               f"got tensors on '{recons.device}'. There is no CPU fallback.")
        if recons.dim() != 3 or recons.shape != target.shape:
            raise ValueError(f"recons {tuple(recons.shape)} and target {tuple(target.shape)} must both be (batch, particles, 4)")
        return HungarianMSEFn.apply(recons, target, bool(abs_coord), bool(polar_coord), self)


class EMDLoss(nn.Module):
    """The energy mover's distance as a training loss, with the interface of the reference's ``utils.losses.EMDLoss``
    (utils/losses/emd_loss.py): ``EMDLoss(num_particles=..., device=...)`` as get_loss() writes it -- jetnet's constructor arguments
    are taken and ignored -- and ``forward(p4_recons, p4_target)`` -> the sum over the batch.

    It is NOT that class's algorithm.  The reference wraps jetnet's regularised differentiable QP; this is the exact transportation LP
    (csrc/emd.hip) on the relative-polar frame of the 22nd anomaly score: the value is ``lgn.emd.emd_relative_tensor(recons,
    target).sum()`` bit for bit, so that the training loss and the score are one quantity, and the gradient is the closed form in the
    optimal flow and the potentials (include/lgn_amd.h), from the same launch.  The reference's wrapper also unbinds its (eta, phi, pt)
    columns as (eta, pt, phi), which hands jetnet an angle ratio as the weight; that mix-up is not reproduced.  After a forward
    ``status`` holds the (B,) int32 flags (LGN_EMD_*; a flagged jet makes the loss NaN).

    ``R``, ``beta``, ``norm`` and ``periodic_phi`` (keywords only) are energyflow's options as lgn.emd.emd() defines them, applied to
    the relative-polar frames: beta = 2 is the squared ground distance, norm = True compares the shapes of the two jets and drops the
    |sum pT - sum pT'| term.  The value is then ``emd_relative_tensor(recons, target, **options).sum()``; at the defaults the loss is
    the one described above, bit for bit."""

    def __init__(self, *args, R: float = 1.0, beta: float = 1.0, norm: bool = False, periodic_phi: bool = False, **kwargs):
        super().__init__()
        from .emd import _options
        _options("EMDLoss", R, beta, norm, periodic_phi)
        self.R, self.beta, self.norm, self.periodic_phi = float(R), float(beta), bool(norm), bool(periodic_phi)
        self.status = None

    def forward(self, p4_recons: torch.Tensor, p4_target: torch.Tensor) -> torch.Tensor:
        from .emd import EMDRelativeFn
        if p4_recons.shape[-1] != 4:
            raise ValueError(f"p4_recons must be a 4-vector. Got: {p4_recons.shape=}")
        if p4_target.shape[-1] != 4:
            raise ValueError(f"p4_target must be a 4-vector. Got: {p4_target.shape=}")
        if p4_recons.device.type != "cuda" or p4_target.device.type != "cuda":
            raise RuntimeError("lgn (MI355X build): EMDLoss runs only in the HIP kernels of liblgn_amd.so on a GPU device; "
                               f"got tensors on '{p4_recons.device}' and '{p4_target.device}'. There is no CPU fallback.")
        if p4_recons.dim() == 2 and p4_target.dim() == 2:       # one unbatched jet
            p4_recons, p4_target = p4_recons.unsqueeze(0), p4_target.unsqueeze(0)
        if p4_recons.dim() != 3 or p4_recons.shape != p4_target.shape:
            raise ValueError(f"p4_recons {tuple(p4_recons.shape)} and p4_target {tuple(p4_target.shape)} must both be "
                             "(batch, particles, 4)")
        return EMDRelativeFn.apply(p4_recons, p4_target, self, self.R, self.beta, self.norm, self.periodic_phi).sum()    # sum over batch


class HybridLoss(nn.Module):
    """The reference's hybrid loss (get_loss(), utils/train.py:446-457) as one module:
    ``chamfer_loss_weight * ChamferLoss(x, t, jet_features) + EMDLoss(x, t)``, both sums over the jets, with this package's
    ``ChamferLoss`` and ``EMDLoss`` (the exact LP, not jetnet's QP).  ``status``: the EMD's flags of the last forward.
    ``emd_options`` (R, beta, norm, periodic_phi) go to the ``EMDLoss``."""

    def __init__(self, chamfer_loss_weight: float = 1.0, device: Optional[torch.device] = None, **emd_options):
        super().__init__()
        self.chamfer_loss_weight = chamfer_loss_weight
        self.chamfer, self.emd = ChamferLoss(device=device), EMDLoss(**emd_options)

    @property
    def status(self):
        return self.emd.status

    def forward(self, p4_recons: torch.Tensor, p4_target: torch.Tensor, jet_features: bool = False) -> torch.Tensor:
        if p4_recons.device.type != "cuda" or p4_target.device.type != "cuda":
            raise RuntimeError("lgn (MI355X build): HybridLoss runs only in the HIP kernels of liblgn_amd.so on a GPU device; "
                               f"got tensors on '{p4_recons.device}' and '{p4_target.device}'. There is no CPU fallback.")
        return self.chamfer_loss_weight * self.chamfer(p4_recons, p4_target, jet_features=jet_features) + self.emd(p4_recons, p4_target)


class SinkhornLoss(nn.Module):
    """The Sinkhorn divergence as a training loss, with ``EMDLoss``'s interface: jetnet's constructor arguments
    (``num_particles=..., device=...``) are taken and ignored, and ``forward(p4_recons, p4_target)`` returns the sum over the jets.

    Per jet the value is ``lgn.sinkhorn.sinkhorn_relative_tensor(recons, target, **options)``, bit for bit: the entropic transport
    problem on the relative-polar frames of the EMD score (include/lgn_amd.h defines it), by default debiased --
    OT_eps(x, t) - OT_eps(x, x) / 2 - OT_eps(t, t) / 2, zero for equal jets -- with the envelope gradient from the same launch.  Where
    the exact LP of ``EMDLoss`` has a gradient that jumps between optimal bases, this loss is smooth.  ``R``, ``beta``, ``norm`` and
    ``periodic_phi`` are the EMD's options.  After a forward ``status`` (LGN_EMD_INVALID, LGN_EMD_EMPTY, LGN_SINKHORN_ITER), ``iters``
    and ``err`` hold the (B,) flags, iteration counts and marginal errors of the cross terms; a jet flagged INVALID or EMPTY makes the
    loss NaN, a jet that only missed ``tol`` within ``max_iter`` iterations still contributes its value and gradient.

    The defaults (epsilon = 0.02, max_iter = 200, tol = 1e-6) are a starting point, not a measured optimum: epsilon sets both the
    smoothing and the number of iterations a jet needs, and no training run has tuned them."""

    def __init__(self, *args, epsilon: float = 0.02, max_iter: int = 200, tol: float = 1e-6, debias: bool = True, R: float = 1.0,
                 beta: float = 1.0, norm: bool = False, periodic_phi: bool = False, **kwargs):
        super().__init__()
        from .sinkhorn import _options
        _options("SinkhornLoss", epsilon, max_iter, tol, debias, R, beta, norm, periodic_phi)
        self.epsilon, self.max_iter, self.tol, self.debias = float(epsilon), int(max_iter), float(tol), bool(debias)
        self.R, self.beta, self.norm, self.periodic_phi = float(R), float(beta), bool(norm), bool(periodic_phi)
        self.status = self.iters = self.err = None

    def forward(self, p4_recons: torch.Tensor, p4_target: torch.Tensor) -> torch.Tensor:
        from .sinkhorn import SinkhornRelativeFn
        if p4_recons.shape[-1] != 4:
            raise ValueError(f"p4_recons must be a 4-vector. Got: {p4_recons.shape=}")
        if p4_target.shape[-1] != 4:
            raise ValueError(f"p4_target must be a 4-vector. Got: {p4_target.shape=}")
        if p4_recons.device.type != "cuda" or p4_target.device.type != "cuda":
            raise RuntimeError("lgn (MI355X build): SinkhornLoss runs only in the HIP kernels of liblgn_amd.so on a GPU device; "
                               f"got tensors on '{p4_recons.device}' and '{p4_target.device}'. There is no CPU fallback.")
        if p4_recons.dim() == 2 and p4_target.dim() == 2:       # one unbatched jet
            p4_recons, p4_target = p4_recons.unsqueeze(0), p4_target.unsqueeze(0)
        if p4_recons.dim() != 3 or p4_recons.shape != p4_target.shape:
            raise ValueError(f"p4_recons {tuple(p4_recons.shape)} and p4_target {tuple(p4_target.shape)} must both be "
                             "(batch, particles, 4)")
        conf = (self.epsilon, self.max_iter, self.tol, self.debias, self.R, self.beta, self.norm, self.periodic_phi)
        return SinkhornRelativeFn.apply(p4_recons, p4_target, self, conf).sum()    # sum over batch
