"""Torch restatement of the reference's per-jet normalisation (utils/normalize_p4.py) and of its method-name matching, for the tests
of the native --normalize path.  Runs on any device; nothing here touches the native library."""
import logging

import torch

EPS = 1e-16
METHODS = ("component_max", "overall_max", "jet_E")


def method_key(method: str) -> str:
    """The name as the reference matches it (lower-cased, ' ' and '-' read as '_'); an unknown name warns -- the text says
    component_max -- and means overall_max."""
    key = str(method).lower().replace(" ", "_").replace("-", "_")
    if key not in ("component_max", "overall_max", "jet_e"):
        logging.warning(f"Normalization method {method} not recognized. Using component_max.")
        key = "overall_max"
    return key


def factor(p4: torch.Tensor, method: str) -> torch.Tensor:
    key = method_key(method)
    if key == "component_max":
        return torch.abs(p4).amax(dim=-2, keepdim=True) + EPS
    if key == "overall_max":
        return torch.abs(p4).amax(dim=-1, keepdim=True).amax(dim=-2, keepdim=True) + EPS
    # (the reference unsqueezes once more: its factor is (B, 1, 1, 1) and its quotient the (B, B, N, 4) table p4[b] / factor[a], which
    # its own encoder refuses; the per-jet normalisation the option describes is that table's diagonal, and this is what is restated)
    return p4.sum(dim=-2, keepdim=True)[..., 0].unsqueeze(-1) + EPS


def normalize_p4(p4: torch.Tensor, method: str = "overall_max"):
    f = factor(p4, method)
    return p4 / f, f


def factor4(p4: torch.Tensor, method: str) -> torch.Tensor:
    """The factor as the native call stores it: (B, 4), a scalar factor four times."""
    return factor(p4, method).expand(p4.shape[0], 1, 4).reshape(p4.shape[0], 4).contiguous()


def jets(B: int, N: int, seed: int, n_real=None) -> torch.Tensor:
    """(B, N, 4) jets with non-negative energies of very different scales per jet; rows n_real .. N - 1 are zero."""
    g = torch.Generator().manual_seed(seed)
    p3 = torch.randn(B, N, 3, generator=g, dtype=torch.float64) * torch.tensor([1.0, 1.0, 3.0], dtype=torch.float64)
    p4 = torch.cat((p3.norm(dim=-1, keepdim=True) * 1.01, p3), dim=-1)
    p4 = p4 * torch.logspace(-2, 3, B, dtype=torch.float64).view(B, 1, 1)
    if n_real is not None:
        p4[:, n_real:] = 0.0
    return p4
