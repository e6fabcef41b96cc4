#!/usr/bin/env python3
"""
Generate the g22 golden vectors under tests/golden/: the arrays the *reference's* plot_p draws its reconstruction plots from
(utils/jet_analysis/utils.py, particle_recon_err.py, jet_recon_err.py).  Run it as gen_golden.py is run:

    cd "$(mktemp -d)" && PYTHONDONTWRITEBYTECODE=1 PYTHONPATH=<reference checkout> \
        python3 <this repo>/tests/golden/gen_golden_g22.py

utils/jet_analysis/__init__.py imports coffea and the three files import matplotlib, neither of which the numbers need: the files are
loaded by path under stub `utils`, `utils.jet_analysis`, `utils.utils`, `matplotlib`, `matplotlib.pyplot` and `energyflow` modules.

Fixtures (jets as gen_golden_g18.jets(): reconstruction = target + N(0, 0.3), padded rows ~ 1e-3):
  g22_analysis_n12.npz   N = 12, B = 16: four jets zero padded (one down to 3 real particles), one jet with recons == target
  g22_analysis_n30.npz   N = 30, B = 64: twenty jets zero padded
  g22_analysis_n150.npz  N = 150, B = 8: two jets zero padded
Each holds target, recons [B][N][4]; rel_err [3][B][N][3] (get_rel_err_find_match's Cartesian, polar, relative polar);
part_polar, part_polarrel [2][B][N][3] (get_p_polar_tensor, get_p_polarrel_tensor; 0 = target, 1 = recons); jet_cart, jet_polar
[2][B][4] (get_jet_feature_cartesian / _polar); jet_rel_err [2][B][4] (the default get_rel_err lambda of plot_jet_recon_err, called
in that function's argument order, on every jet); jet_keep [2][B] (the jets filter_out_zeros keeps); col4row [2][B][N] (scipy's
col_ind on the Cartesian and the relative-polar costs); is_padded [B][N]; meta.

torch.cdist switches to a matrix-product formula past 25 points, so there the reference's costs are not the exact distances in the
last bits.  A jet whose scipy assignment on the reference's costs differs from the one on exact costs (tests/_analysis_ref.cost3),
for either cost, is left out of the fixture (meta.dropped): only padded (tied) jets may be, and never at N <= 25 -- asserted.  The tie
behaviour of dropped jets is pinned against tests/_analysis_ref.py instead.  (Up to 25 points torch.cdist takes its direct kernel,
but on three-component rows that kernel does not always round as the ordered sum either -- a few costs per jet differ by an ulp --
so a tied jet can resolve differently even there: seeds 2212 and 2213 of the N = 12 case trip the assertion, the fixture's 2214
does not.)
"""
import importlib.util
import inspect
import json
import os
import sys
import types

sys.dont_write_bytecode = True
import numpy as np  # noqa: E402
import torch  # noqa: E402
from scipy.optimize import linear_sum_assignment  # noqa: E402

OUT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(OUT))
sys.path.insert(0, OUT)
import _analysis_ref as R  # noqa: E402
from gen_golden_g18 import jets  # noqa: E402


def load_reference():
    root = next(p for p in sys.path if p and os.path.isfile(os.path.join(p, "utils", "jet_analysis", "particle_recon_err.py")))
    ja = os.path.join(root, "utils", "jet_analysis")
    for name, path in (("utils", os.path.join(root, "utils")), ("utils.jet_analysis", ja)):
        pkg = types.ModuleType(name)
        pkg.__path__ = [path]
        sys.modules[name] = pkg
    uu = types.ModuleType("utils.utils")
    uu.make_dir = lambda path: path
    sys.modules["utils.utils"] = uu
    mpl = types.ModuleType("matplotlib")
    mpl.pyplot = types.ModuleType("matplotlib.pyplot")
    sys.modules["matplotlib"], sys.modules["matplotlib.pyplot"] = mpl, mpl.pyplot
    sys.modules["energyflow"] = types.ModuleType("energyflow")
    mods = {}
    for sub in ("utils", "particle_recon_err", "jet_recon_err"):
        spec = importlib.util.spec_from_file_location(f"utils.jet_analysis.{sub}", os.path.join(ja, f"{sub}.py"))
        m = importlib.util.module_from_spec(spec)
        sys.modules[spec.name] = m
        spec.loader.exec_module(m)
        mods[sub] = m
    return mods["utils"], mods["particle_recon_err"], mods["jet_recon_err"]


def case(ref, name, B, N, seed, pad=(), same=()):
    U, PR, JR = ref
    rng = np.random.default_rng(seed)
    target = jets(rng, B, N, pad)
    recons = target + rng.normal(scale=0.3, size=target.shape)
    for b, n in pad:
        recons[b, n:] = rng.normal(scale=1e-3, size=(N - n, 4))     # the decoder does not reproduce exact zeros
    for b in same:
        recons[b] = target[b]
    t, r = torch.from_numpy(target), torch.from_numpy(recons)

    # plot_particle_recon_err's inputs (abs_coord=True) and its matched relative errors
    t3, r3 = t[..., 1:], r[..., 1:]
    tp, rp = U.get_p_polar_tensor(t), U.get_p_polar_tensor(r)
    tq, rq = U.get_p_polarrel_tensor(t), U.get_p_polarrel_tensor(r)
    rel = [e.numpy().reshape(B, N, 3) for e in PR.get_rel_err_find_match(t3, r3, tp, rp, tq, rq, gpu=False)]
    is_padded = np.isinf(rel[0]).any(-1)

    # plot_jet_recon_err's inputs, relative errors and filter
    jc = [U.get_jet_feature_cartesian(x, gpu=False, return_arr=True).numpy() for x in (t, r)]
    jp = [U.get_jet_feature_polar(x, gpu=False, return_arr=True) for x in (t, r)]
    lam = inspect.signature(JR.plot_jet_recon_err).parameters["get_rel_err"].default
    eps = inspect.signature(JR.plot_jet_recon_err).parameters["eps"].default
    with np.errstate(all="ignore"):
        jre = [np.stack([lam(f[1][:, i], f[0][:, i], eps) for i in range(4)], -1) for f in (jc, jp)]   # (recons, target): its call's order
    idx = tuple(np.arange(B) for _ in range(4))
    jet_keep = []
    for f in (jc, jp):
        _, kept = JR.filter_out_zeros(tuple(f[0][:, i] for i in range(4)), idx)
        mask = np.zeros(B, bool)
        mask[kept[0]] = True
        jet_keep.append(mask)

    # scipy's col_ind on the reference's costs and on the exact ones
    col = np.zeros((2, B, N), dtype=np.int64)
    keep = np.ones(B, bool)
    n_drop = [0, 0]
    for k, (x, y) in enumerate(((t3, r3), (tq, rq))):
        ref_cost = torch.cdist(x, y).numpy()
        exact = R.cost3(x.numpy(), y.numpy())
        for b in range(B):
            c_ref, c_ex = linear_sum_assignment(ref_cost[b])[1], linear_sum_assignment(exact[b])[1]
            col[k, b] = c_ex
            if not np.array_equal(c_ref, c_ex):
                keep[b] = False
                n_drop[k] += 1
    dropped = [int(b) for b in np.flatnonzero(~keep)]
    padded = {b for b, _ in pad}
    assert all(b in padded for b in dropped) and (N > 25 or not dropped), (name, dropped)
    k = keep
    meta = dict(B=int(k.sum()), N=N, seed=seed, pad=[list(map(int, x)) for x in pad], same=list(map(int, same)), dropped=dropped,
                padded_kept=[int(i) for i, b in enumerate(np.flatnonzero(k)) if int(b) in padded],
                source="utils/jet_analysis/{utils,particle_recon_err,jet_recon_err}.py")
    np.savez_compressed(os.path.join(OUT, name), target=target[k], recons=recons[k], rel_err=np.stack(rel)[:, k],
                        part_polar=np.stack((tp.numpy(), rp.numpy()))[:, k], part_polarrel=np.stack((tq.numpy(), rq.numpy()))[:, k],
                        jet_cart=np.stack(jc)[:, k], jet_polar=np.stack(jp)[:, k], jet_rel_err=np.stack(jre)[:, k],
                        jet_keep=np.stack(jet_keep)[:, k], col4row=col[:, k], is_padded=is_padded[k], meta=np.array(json.dumps(meta)))
    print(name, "jets", int(k.sum()), "dropped", dropped, "per cost", n_drop)


if __name__ == "__main__":
    torch.set_num_threads(8)
    ref = load_reference()
    rng = np.random.default_rng(22)
    pad12 = ((1, 3), (4, 9), (7, 11), (10, 6))
    case(ref, "g22_analysis_n12.npz", 16, 12, 2214, pad=pad12, same=(5,))
    pad30 = tuple((b, int(rng.integers(8, 30))) for b in range(20))
    case(ref, "g22_analysis_n30.npz", 64, 30, 2230, pad=pad30)
    case(ref, "g22_analysis_n150.npz", 8, 150, 22150, pad=((0, 100), (3, 149)))
