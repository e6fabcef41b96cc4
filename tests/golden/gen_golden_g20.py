#!/usr/bin/env python3
"""
Generate tests/golden/g20_optimizer_defaults.json: what the reference's utils.initialize.initialize_optimizers builds for
--optimizer adam and --optimizer rmsprop (fp64) -- the class name and ``defaults`` of both optimisers, settings only.  The
reference's ``utils`` package is imported, with the empty ``jetnet`` stand-in of gen_golden.py; THIS repo's ``lgn`` package takes
the place of the reference's (its LGNEncoder / LGNDecoder are what the optimisers are built on).  Run it with this repo's package
in front of the reference checkout:

    cd "$(mktemp -d)" && PYTHONDONTWRITEBYTECODE=1 PYTHONPATH=<this repo>/lgn-autoencoder_amd:<reference checkout> \
        python3 <this repo>/tests/golden/gen_golden_g20.py

The tests read the JSON, never the reference (tests/test_host_optimizer_options.py).
"""
import argparse
import json
import os
import sys
import types

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

sys.modules.setdefault("jetnet", types.ModuleType("jetnet"))  # EMD wrapper is never instantiated

import lgn  # noqa: E402
from utils.initialize import initialize_optimizers  # noqa: E402
import __graft_entry__ as G  # noqa: E402

assert os.path.abspath(lgn.__file__).startswith(os.path.join(ROOT, "lgn-autoencoder_amd")), "put this repo's package first"


KEYS = {"adam": ("lr", "betas", "eps", "weight_decay", "amsgrad"),
        "rmsprop": ("lr", "alpha", "eps", "weight_decay", "momentum", "centered")}


def plain(v):
    return list(v) if isinstance(v, tuple) else v


def main():
    enc, dec = G._models(30, (3, 3, 4, 4), (4, 4, 3, 3), torch.device("cpu"))
    out = {"args": {"lr": 5e-4, "dtype": "torch.float64"}, "choices": {}}
    for choice in ("adam", "rmsprop"):
        args = argparse.Namespace(optimizer=choice, lr=5e-4, dtype=torch.float64)
        opts = initialize_optimizers(args, enc, dec)
        # the settings that define the update rule; torch's execution switches (foreach, fused, capturable, ...) come and go with
        # its versions and are not recorded
        out["choices"][choice] = [{"type": type(o).__name__, "defaults": {k: plain(o.defaults[k]) for k in KEYS[choice]}} for o in opts]
    try:
        initialize_optimizers(argparse.Namespace(optimizer="sgd", lr=5e-4, dtype=torch.float64), enc, dec)
        out["unknown_raises"] = None
    except Exception as exc:      # noqa: BLE001
        out["unknown_raises"] = type(exc).__name__
    path = os.path.join(HERE, "g20_optimizer_defaults.json")
    with open(path, "w") as fh:
        json.dump(out, fh, sort_keys=True)
        fh.write("\n")
    print(f"wrote {path} ({os.path.getsize(path)} B)")


if __name__ == "__main__":
    main()
