#!/usr/bin/env python3
"""
Generate the g19 golden vectors under tests/golden/: the reference's HungarianMSELoss (utils/losses/hungarian_mse) and nn.MSELoss as
training losses, by importing the *reference* implementation (as gen_golden.py does; run it the same way, scipy installed):

    cd "$(mktemp -d)" && PYTHONDONTWRITEBYTECODE=1 PYTHONPATH=<reference checkout> \
        python3 <this repo>/tests/golden/gen_golden_g19.py

Loss level (x = reconstruction, t = target, (B, N, 4); per frame f in abs_cart / abs_polar / rel_polar / rel_cart the reference's
loss.f, its gradient grad.f = d loss / d x and col.f, the linear_sum_assignment of torch.cdist of every jet):
  g19_loss_n30.npz       64 jets, N = 30, no padding
  g19_loss_n30_pad.npz   128 jets, N = 30, 20 real particles then zero rows in the target; also loss.mse / grad.mse of nn.MSELoss
  g19_loss_n150.npz      16 jets, N = 150, no padding
Step level (the cfg1-style networks of g17, get_real 'real'): p4, labels, meta, recon, loss, grad.{enc,dec}.* and col (the reference's
assignment; the identity for mse)
  g19_step_{hungarian,relpolar,mse}_maxdim{2,3}.npz
One jet is zero padded by ONE row: two or more zero rows are tied columns, which leave several optima of one total cost; which of them
a solver finds turns on the last bits of the reconstruction, and the reference's pairing p[col[r]] - q[r] makes loss and gradients
depend on it -- such a fixture could not be compared gradient for gradient.  The batch seed of a network is the first one from g17's
on at which, in every case, the optimum is DECIDABLE: the assignment of exact costs is the reference's on every jet, and stays the
same under 20 random relative perturbations of the reconstruction of 1e-8 (a hundred times the tolerance the steps are held to).
The script prints, per padded frame, the share of jets on which the assignment of EXACT costs (tests/_hungarian_ref.py) is another
optimum than the reference's (torch.cdist rounds differently; tied zero columns): the committed fixture keeps it at or below 5 %.
"""
import json
import os
import sys

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import gen_golden as G  # noqa: E402  (imports the reference's lgn / utils; stands in an empty jetnet)
import gen_golden_g17 as G17  # noqa: E402
from utils.losses.hungarian_mse.hungarian_mse import HungarianMSELoss, preprocess  # noqa: E402
from scipy import optimize  # noqa: E402

import _hungarian_ref as H  # noqa: E402  (only for the printed share)

FRAMES = {"abs_cart": (True, False), "abs_polar": (True, True), "rel_polar": (False, True), "rel_cart": (False, False)}


def jets(B, N, n_real, seed):
    g = torch.Generator().manual_seed(seed)
    p3 = torch.randn(B, N, 3, generator=g, dtype=torch.float64) * torch.tensor([1.0, 1.0, 2.0], dtype=torch.float64)
    t = torch.cat((p3.norm(dim=-1, keepdim=True) * 1.01, p3), dim=-1)
    if n_real is not None:
        t[:, n_real:] = 0.0
    x = t[:, torch.randperm(N, generator=g)] + 0.05 * torch.randn(B, N, 4, generator=g, dtype=torch.float64)
    return x, t


def loss_level(name, B, N, n_real, seed, mse=False):
    x, t = jets(B, N, n_real, seed)
    store = {"x": G.npy(x), "t": G.npy(t), "meta": np.array(json.dumps(dict(B=B, N=N, n_real=n_real, seed=seed)))}
    for f, (a, p) in FRAMES.items():
        xx = x.clone().requires_grad_(True)
        loss = HungarianMSELoss()(xx, t.clone(), abs_coord=a, polar_coord=p)
        loss.backward()
        with torch.no_grad():
            rp, tp = preprocess(x.clone(), t.clone(), abs_coord=a, polar_coord=p)
            cost = torch.cdist(rp, tp).numpy()
        col = np.stack([optimize.linear_sum_assignment(c)[1] for c in cost])
        store[f"loss.{f}"], store[f"grad.{f}"], store[f"col.{f}"] = G.npy(loss), G.npy(xx.grad), col.astype(np.int16)
        differ = (H.assignment(x, t, a, p).numpy() != col).any(-1).mean()
        print(f"{name} {f}: loss {loss.item():.12g}, exact-cost assignment differs on {100 * differ:.2f} % of the jets")
    if mse:
        xx = x.clone().requires_grad_(True)
        loss = torch.nn.MSELoss()(xx, t)
        loss.backward()
        store["loss.mse"], store["grad.mse"] = G.npy(loss), G.npy(xx.grad)
    np.savez_compressed(os.path.join(G.OUT, name), **store)


def PAD_ROWS(N):
    return ((1, N - 1),)          # jet 1: its last row is zero


STEP_CASES = [("hungarian", "hungarian", True, False), ("relpolar", "hungarian", False, True), ("mse", "mse", True, False)]


def step_level(tag, choice, a, p, maxdim, batch_seed, write=True):
    """Returns whether the exact-cost assignment is the reference's on every jet."""
    n = G17.NETS[maxdim]
    B, N = n["B"], n["N"]
    enc, dec = G.build(N, maxdim, n["ch_enc"], n["ch_dec"], n["seed"])
    p4, labels = G.jets(B, N, batch_seed, PAD_ROWS(N))
    meta = dict(batch_seed=batch_seed, B=B, N=N, maxdim=maxdim, ch_enc=list(n["ch_enc"]), ch_dec=list(n["ch_dec"]), seed=n["seed"], l1_lambda=0.0,
                get_real_method="real", loss_choice=choice, hungarian_abs_coord=a, hungarian_polar_coord=p)
    enc.zero_grad(); dec.zero_grad()
    recon = dec(enc({"p4": p4, "labels": labels}))
    x = G.get_real(recon, "real")
    loss = torch.nn.MSELoss()(x, p4) if choice == "mse" else HungarianMSELoss()(x, p4.clone(), abs_coord=a, polar_coord=p)
    with torch.no_grad():
        if choice == "mse":
            col = np.tile(np.arange(N), (B, 1))
        else:
            rp, tp = preprocess(x.detach().clone(), p4.clone(), abs_coord=a, polar_coord=p)
            col = np.stack([optimize.linear_sum_assignment(c)[1] for c in torch.cdist(rp, tp).numpy()])
    same = choice == "mse" or bool((H.assignment(x.detach(), p4, a, p).numpy() == col).all())
    if same and choice != "mse":
        g = torch.Generator().manual_seed(batch_seed)
        for _ in range(20):
            xp = x.detach() * (1 + 1e-8 * torch.randn(x.shape, generator=g, dtype=x.dtype))
            same = same and bool((H.assignment(xp, p4, a, p).numpy() == col).all())
    if not write:
        return same
    loss.backward()
    store = {"p4": G.npy(p4), "labels": G.npy(labels), "meta": np.array(json.dumps(meta)), "recon": G.npy(recon), "loss": G.npy(loss),
             "col": col.astype(np.int16)}
    for pre, mod in (("enc", enc), ("dec", dec)):
        for k, q in mod.named_parameters():
            store[f"grad.{pre}.{k}"] = G.npy(q.grad if q.grad is not None else torch.zeros_like(q))
    name = f"g19_step_{tag}_maxdim{maxdim}.npz"
    np.savez_compressed(os.path.join(G.OUT, name), **store)
    print(name, "batch seed", batch_seed, "loss", loss.item(), "n arrays", len(store), "decidable optimum:", same)
    return same


if __name__ == "__main__":
    torch.set_num_threads(8)
    loss_level("g19_loss_n30.npz", 64, 30, None, 190)
    loss_level("g19_loss_n30_pad.npz", 128, 30, 20, 191, mse=True)
    loss_level("g19_loss_n150.npz", 16, 150, None, 192)
    for maxdim in (2, 3):
        seed = G17.NETS[maxdim]["seed"] + 100
        while not all(step_level(tag, choice, a, p, maxdim, seed, write=False) for tag, choice, a, p in STEP_CASES):
            seed += 1
        for tag, choice, a, p in STEP_CASES:
            step_level(tag, choice, a, p, maxdim, seed)
