#!/usr/bin/env python3
"""
Generate the g17 golden vectors under tests/golden/: the training-step loss with the reference's --get-real-method and
--chamfer-jet-features options, by importing the *reference* implementation (as gen_golden.py does; run it the same way):

    cd "$(mktemp -d)" && PYTHONDONTWRITEBYTECODE=1 PYTHONPATH=<reference checkout> \
        python3 <this repo>/tests/golden/gen_golden_g17.py

Fixtures (cfg1-style networks, ch 3344/4433 at maxdim 2 and 4466/6644 at maxdim 3, one jet zero padded; the weights are the seeded
initialisation of gen_golden.build, rebuilt by the tests from meta.seed):
  g17_real_maxdim{2,3}.npz     get_real(recon, 'real'), the reference's default (main.py --get-real-method)
  g17_norm_maxdim{2,3}.npz     get_real(recon, 'norm')
  g17_realjet_maxdim{2,3}.npz  get_real(recon, 'real') and ChamferLoss(..., jet_features=True) (--chamfer-jet-features)
Each holds p4, labels, meta, recon (2,B,N,4), loss (Chamfer [+ jet MSE], no L1 term) and grad.{enc,dec}.<parameter> of that loss.
"""
import json
import os
import sys

sys.dont_write_bytecode = True
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import gen_golden as G  # noqa: E402  (imports the reference's lgn / utils)

CASES = [("real", "real", False), ("norm", "norm", False), ("realjet", "real", True)]
NETS = {2: dict(B=3, N=12, ch_enc=(3, 3, 4, 4), ch_dec=(4, 4, 3, 3), seed=40, pad_rows=((1, 8),)),
        3: dict(B=2, N=12, ch_enc=(4, 4, 6, 6), ch_dec=(6, 6, 4, 4), seed=41, pad_rows=((1, 9),))}


def case(tag, method, jet, maxdim):
    n = NETS[maxdim]
    B, N = n["B"], n["N"]
    enc, dec = G.build(N, maxdim, n["ch_enc"], n["ch_dec"], n["seed"])
    p4, labels = G.jets(B, N, n["seed"] + 100, n["pad_rows"])
    meta = dict(B=B, N=N, maxdim=maxdim, ch_enc=list(n["ch_enc"]), ch_dec=list(n["ch_dec"]), seed=n["seed"], l1_lambda=0.0,
                get_real_method=method, chamfer_jet_features=jet)
    enc.zero_grad(); dec.zero_grad()
    recon = dec(enc({"p4": p4, "labels": labels}))
    loss = G.ChamferLoss(device=G.CPU)(G.get_real(recon, method), p4, jet_features=jet)
    loss.backward()
    store = {"p4": G.npy(p4), "labels": G.npy(labels), "meta": np.array(json.dumps(meta)), "recon": G.npy(recon), "loss": G.npy(loss)}
    for pre, mod in (("enc", enc), ("dec", dec)):
        for k, p in mod.named_parameters():
            store[f"grad.{pre}.{k}"] = G.npy(p.grad if p.grad is not None else torch.zeros_like(p))
    name = f"g17_{tag}_maxdim{maxdim}.npz"
    np.savez_compressed(os.path.join(G.OUT, name), **store)
    print(name, "loss", loss.item(), "n arrays", len(store))


if __name__ == "__main__":
    torch.set_num_threads(8)
    for maxdim in (2, 3):
        for tag, method, jet in CASES:
            case(tag, method, jet, maxdim)
