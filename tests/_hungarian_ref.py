"""torch restatement of the reference's HungarianMSELoss (utils/losses/hungarian_mse/hungarian_mse.py:46-84 and utils.py next to it)
with the assignment taken from EXACT costs (sqrt of the sum of squares in a fixed order, not torch.cdist's matrix-multiply route)
through _anomaly_ref.lsap -- no scipy dependency -- and the loss as a differentiable expression that takes the assignment as an
argument, so that a test can score any assignment.  Not a test module."""
import numpy as np
import torch

import _anomaly_ref as A

EPS = 1e-16
FRAMES = {"abs_cart": (True, False), "abs_polar": (True, True), "rel_polar": (False, True), "rel_cart": (False, False)}


def p_polar(p):
    """get_p_polar: (pt, eta, phi) with eps under the root."""
    px, py, pz = p[..., 1], p[..., 2], p[..., 3]
    pt = torch.sqrt((px * px + py * py) + EPS)
    return torch.stack((pt, torch.asinh(pz / (pt + EPS)), torch.atan2(py + EPS, px + EPS)), dim=-1)


def jet_sum(t):
    """target.sum(-2) with the rows added in order."""
    s = torch.zeros_like(t[..., 0, :])
    for r in range(t.shape[-2]):
        s = s + t[..., r, :]
    return s


def frames(x, t, abs_coord=True, polar_coord=False):
    """preprocess(): the frames (p, q) of (x, t), both (B, N, 4) -> (B, N, D)."""
    if abs_coord:
        return (p_polar(x), p_polar(t)) if polar_coord else (x, t)
    jet = p_polar(jet_sum(t.detach())).unsqueeze(-2)          # the TARGET's jet for both sides
    out = []
    for p in (p_polar(x), p_polar(t)):
        rel = torch.stack((p[..., 0] / jet[..., 0], p[..., 1] - jet[..., 1], p[..., 2] - jet[..., 2]), dim=-1)
        if not polar_coord:                                   # get_p_cartesian: py = pt cos(phi) as the reference has it
            c = rel[..., 0] * torch.cos(rel[..., 2])
            rel = torch.stack((c, c, rel[..., 0] * torch.sinh(rel[..., 1])), dim=-1)
        out.append(rel)
    return out[0], out[1]


def costs(p, q):
    """cost[b][i][j] = |p_i - q_j|, the squares added in column order (numpy, exact IEEE operations)."""
    p, q = p.detach().cpu().numpy(), q.detach().cpu().numpy()
    d = p[:, :, None, :] - q[:, None, :, :]
    s = d[..., 0] * d[..., 0]
    for c in range(1, d.shape[-1]):
        s = s + d[..., c] * d[..., c]
    return np.sqrt(s)


def assignment(x, t, abs_coord=True, polar_coord=False):
    """col (B, N) int64: linear_sum_assignment of the exact costs, ties as scipy breaks them."""
    p, q = frames(x.detach(), t.detach(), abs_coord, polar_coord)
    return torch.from_numpy(np.stack([A.lsap(c) for c in costs(p, q)])).long()


def total_cost(x, t, col, abs_coord=True, polar_coord=False):
    """sum_r cost[r][col[r]] per jet (B,) -- what the assignment minimises."""
    p, q = frames(x.detach(), t.detach(), abs_coord, polar_coord)
    c = torch.from_numpy(costs(p, q))
    return torch.gather(c, 2, col.cpu().long().unsqueeze(-1)).squeeze(-1).sum(-1)


def per_jet(x, t, col, abs_coord=True, polar_coord=False, n_jets=None):
    """Per-jet terms (B,) of the loss for the assignment `col`: sum_r sum_c (p[col[r]][c] - q[r][c])^2 / (n_jets N D)."""
    p, q = frames(x, t, abs_coord, polar_coord)
    ps = torch.gather(p, 1, col.to(p.device).long().unsqueeze(-1).expand_as(p))
    B, N, D = p.shape
    return ((ps - q) ** 2).sum((-1, -2)) / ((n_jets or B) * N * D)


def loss(x, t, col=None, abs_coord=True, polar_coord=False, n_jets=None):
    if col is None:
        col = assignment(x, t, abs_coord, polar_coord)
    return per_jet(x, t, col, abs_coord, polar_coord, n_jets).sum()


def mse_per_jet(x, t, n_jets=None):
    """nn.MSELoss()(x, t) split into per-jet terms."""
    B, N, D = x.shape
    return ((x - t) ** 2).sum((-1, -2)) / ((n_jets or B) * N * D)


def jets(B, N, n_real=None, seed=0):
    """Random jets of 4-vectors (E, px, py, pz) and a perturbed copy as the reconstruction; rows n_real .. N-1 of the TARGET are zero."""
    g = torch.Generator().manual_seed(seed)
    p3 = torch.randn(B, N, 3, generator=g, dtype=torch.float64) * torch.tensor([1.0, 1.0, 2.0], dtype=torch.float64)
    t = torch.cat((p3.norm(dim=-1, keepdim=True) * 1.01, p3), dim=-1)
    if n_real is not None:
        t[:, n_real:] = 0.0
    x = t[:, torch.randperm(N, generator=g)] + 0.05 * torch.randn(B, N, 4, generator=g, dtype=torch.float64)
    return x, t
