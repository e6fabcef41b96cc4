#!/usr/bin/env python3
"""
Generate the g21 golden vectors under tests/golden/: the reference's --normalize (utils/normalize_p4.py, utils/train.py:281-320), by
importing the *reference* implementation (as gen_golden.py does; run it the same way):

    cd "$(mktemp -d)" && PYTHONDONTWRITEBYTECODE=1 PYTHONPATH=<reference checkout> \
        python3 <this repo>/tests/golden/gen_golden_g21.py

  g21_normalize.npz   p4 (6, 30, 4): a full jet, 20 real rows + 10 zero rows, one real row, an all-zero jet, a jet whose largest entry is
                      a negative pz, a jet with one NaN; out.<name> / factor.<name> of utils.normalize_p4.normalize_p4 for the three methods
                      and the spellings 'Overall-Max', 'jet e' and 'bogus' (names: the list in `names`).  The reference's jet_E
                      returns its factor as (B, 1, 1, 1), so its quotient broadcasts to (B, B, N, 4) with out[a][b] = p4[b] / factor[a]:
                      recorded as the reference returns it; the per-jet normalisation is its diagonal out[b][b]
  g21_step_normalize_maxdim2.npz   the loop body of train() with args.normalize (normalize_p4 -> encoder -> decoder -> get_real ->
                      ChamferLoss, default options: get_real 'real', no regularisation term recorded) on the g1 network (gen_golden.build,
                      seed 0) and 4 raw jets of 30 particles, two of them zero padded: per method loss.<m>, recon_denorm.<m> =
                      p4_recons * norm_factor, norm_factor.<m>.  With jet_E the reference's own loop stops in the encoder (the 4-d
                      quotient above); that case runs the same loop body on the diagonal -- every jet divided by its own factor --
                      with the factor reshaped to (B, 1, 1)
"""
import json
import os
import sys

sys.dont_write_bytecode = True
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import gen_golden as G  # noqa: E402  (imports the reference's lgn / utils)
from utils.normalize_p4 import METHODS, normalize_p4  # noqa: E402

SPELLINGS = ("Overall-Max", "jet e", "bogus")


def raw_jets(B, N, seed):
    g = torch.Generator().manual_seed(seed)
    p3 = torch.randn(B, N, 3, generator=g, dtype=G.F64) * torch.tensor([1.0, 1.0, 3.0], dtype=G.F64)
    p4 = torch.cat((p3.norm(dim=-1, keepdim=True) * 1.01, p3), dim=-1)
    return p4 * torch.logspace(0, 2.5, B, dtype=G.F64).view(B, 1, 1)


def normalize_level():
    p4 = raw_jets(6, 30, 210)
    p4[1, 20:] = 0.0
    p4[2, 1:] = 0.0
    p4[3] = 0.0
    p4[4, 7, 3] = -3.0 * p4[4].abs().max()
    p4[5, 11, 2] = float("nan")
    names = list(METHODS) + list(SPELLINGS)
    store = {"p4": G.npy(p4), "names": np.array(json.dumps(names))}
    for name in names:
        out, f = normalize_p4(p4.clone(), name)
        store[f"out.{name}"], store[f"factor.{name}"] = G.npy(out), G.npy(f)
        print(name, "factor", tuple(f.shape), f.flatten()[:4].tolist())
    np.savez_compressed(os.path.join(G.OUT, "g21_normalize.npz"), **store)


def step_level():
    B, N, maxdim, che, chd, seed = 4, 30, 2, (3, 3, 4, 4), (4, 4, 3, 3), 0
    p4 = raw_jets(B, N, 211)
    p4[1, 17:] = 0.0
    p4[3, 25:] = 0.0
    meta = dict(B=B, N=N, maxdim=maxdim, ch_enc=list(che), ch_dec=list(chd), seed=seed, get_real_method="real", methods=list(METHODS))
    store = {"p4": G.npy(p4), "meta": np.array(json.dumps(meta))}
    for method in METHODS:
        enc, dec = G.build(N, maxdim, che, chd, seed)
        with torch.no_grad():
            batch = {"p4": p4.clone()}
            batch["p4"], norm_factor = normalize_p4(batch["p4"], method)
            if batch["p4"].dim() == 4:          # jet_E (see the module docstring)
                batch["p4"] = torch.stack([batch["p4"][b, b] for b in range(B)])
                norm_factor = norm_factor.reshape(B, 1, 1)
            p4_recons = G.get_real(dec(enc(batch)), "real")
            loss = G.ChamferLoss(device=G.CPU)(p4_recons, batch["p4"], jet_features=False)
        store[f"loss.{method}"], store[f"norm_factor.{method}"] = G.npy(loss), G.npy(norm_factor)
        store[f"recon_denorm.{method}"] = G.npy(p4_recons * norm_factor)
        print("step", method, "loss", loss.item())
    np.savez_compressed(os.path.join(G.OUT, "g21_step_normalize_maxdim2.npz"), **store)


if __name__ == "__main__":
    torch.set_num_threads(8)
    normalize_level()
    step_level()
