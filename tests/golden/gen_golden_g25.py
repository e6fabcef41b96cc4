#!/usr/bin/env python3
"""
Generate the g25 golden vectors under tests/golden/: what the *reference's* get_stats, find_fwhm, plot_particle_recon_err,
plot_jet_recon_err and pixelate compute.  Run it as gen_golden_g22.py is run:

    cd "$(mktemp -d)" && PYTHONDONTWRITEBYTECODE=1 PYTHONPATH=<reference checkout> \
        python3 <this repo>/tests/golden/gen_golden_g25.py

The reference's utils.py, particle_recon_err.py, jet_recon_err.py and jet_images.py are loaded by path under stub `utils.utils`,
`energyflow`, `awkward` and `coffea` modules (ak.behavior a dict, vector.behavior empty); matplotlib is the real one with the Agg
backend, so the two plot functions run as they are, into a temporary directory, and the JSON they write is what is stored.

  g25_err_dict.json   {"n12" | "n30": {"particle": <particle_reconstruction_errors.json>, "jet": <jet_reconstruction_errors.json>}}
                      on the g22 n12 and n30 inputs with abs_coord=True and both custom_*_ranges=False.  The jet plot is fed g22's own
                      jet_cart / jet_polar arrays.
  g25_stats.npz       col_<name>: synthetic columns; stat_<name>: get_stats(col, bins_<name>) as 17 numbers in the dict's order (NaN
                      where it gives None); jets_<k> [B][N][3] relative (pt, eta, phi) jets with images_<k> =
                      get_n_jet_images(abs_coord=False) and average_<k> = get_average_jet_image(abs_coord=False); meta.
awkward and coffea are not installed where this was run: no value of modes 1 and 2 (abs_coord=True images) was produced by them.
Those modes are specified by the formula in include/lgn_amd.h and checked against tests/_stats_ref.py.

meta.heavy_scipy_vs_longdouble: |scipy - np.longdouble two-pass| of skew and kurtosis on the heavy-tailed column, measured here.
"""
import importlib.util
import json
import os
import sys
import tempfile
import types

sys.dont_write_bytecode = True
import matplotlib  # noqa: E402

matplotlib.use("Agg")
import numpy as np  # noqa: E402
import torch  # noqa: E402

OUT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(OUT))
import _stats_ref as S  # noqa: E402


def load_reference():
    root = next(p for p in sys.path if p and os.path.isfile(os.path.join(p, "utils", "jet_analysis", "particle_recon_err.py")))
    ja = os.path.join(root, "utils", "jet_analysis")
    for name, path in (("utils", os.path.join(root, "utils")), ("utils.jet_analysis", ja)):
        pkg = types.ModuleType(name)
        pkg.__path__ = [path]
        sys.modules[name] = pkg
    uu = types.ModuleType("utils.utils")

    def make_dir(path):
        os.makedirs(path, exist_ok=True)
        return path
    uu.make_dir = make_dir
    sys.modules["utils.utils"] = uu
    sys.modules["energyflow"] = types.ModuleType("energyflow")
    ak = types.ModuleType("awkward")
    ak.behavior = {}
    ak.Array = object
    sys.modules["awkward"] = ak
    for name in ("coffea", "coffea.nanoevents", "coffea.nanoevents.methods", "coffea.nanoevents.methods.vector"):
        sys.modules[name] = types.ModuleType(name)
    sys.modules["coffea.nanoevents.methods.vector"].behavior = {}
    sys.modules["coffea.nanoevents.methods"].vector = sys.modules["coffea.nanoevents.methods.vector"]
    mods = {}
    for sub in ("utils", "particle_recon_err", "jet_recon_err", "jet_images"):
        spec = importlib.util.spec_from_file_location(f"utils.jet_analysis.{sub}", os.path.join(ja, f"{sub}.py"))
        m = importlib.util.module_from_spec(spec)
        sys.modules[spec.name] = m
        spec.loader.exec_module(m)
        mods[sub] = m
    return mods


def err_dicts(mods, name):
    g = np.load(os.path.join(OUT, f"g22_analysis_{name}.npz"))
    t, r = torch.from_numpy(g["target"]), torch.from_numpy(g["recons"])
    with tempfile.TemporaryDirectory() as tmp, np.errstate(all="ignore"):
        mods["particle_recon_err"].plot_particle_recon_err(t, r, abs_coord=True, custom_particle_recons_ranges=False, find_match=True,
                                                           save_dir=tmp, epoch=None)
        jc, jp = g["jet_cart"], g["jet_polar"]
        cols = lambda a: tuple(a[:, i] for i in range(4))
        mods["jet_recon_err"].plot_jet_recon_err(cols(jc[0]), cols(jc[1]), cols(jp[0]), cols(jp[1]), save_dir=tmp, abs_coord=True,
                                                 custom_jet_recons_ranges=False, epoch=None)
        with open(os.path.join(tmp, "particle_reconstruction_errors.json")) as f:
            particle = json.load(f)
        with open(os.path.join(tmp, "jet_reconstruction_errors.json")) as f:
            jet = json.load(f)
    # the plot's own matching must be the fixture's: the g25 numbers then belong to g22's stored rel_err and is_padded
    PR, U = mods["particle_recon_err"], mods["utils"]
    rel = PR.get_rel_err_find_match(t[..., 1:], r[..., 1:], U.get_p_polar_tensor(t), U.get_p_polar_tensor(r),
                                    U.get_p_polarrel_tensor(t), U.get_p_polarrel_tensor(r), gpu=False)
    for f in range(3):
        assert np.array_equal(rel[f].numpy().reshape(g["rel_err"][f].shape), g["rel_err"][f], equal_nan=True), (name, f)
    return {"particle": particle, "jet": jet}


def columns():
    rng = np.random.default_rng(25)
    T = 2048                              # LGN_STATS_TILE
    cols = {}
    for n in (1, 2, 3, 4, 5, 9, 10, 11, T - 1, T, T + 1, 2 * T + 3, 5 * T + 17):
        cols[f"normal_{n}"] = rng.normal(loc=0.3, scale=2.0, size=n)
    cols["constant"] = np.full(37, 1.25)
    cols["ties"] = rng.integers(-3, 4, size=501).astype(np.float64) / 4
    z = rng.normal(size=64)
    z[::3] = 0.0
    z[1::6] = -0.0
    cols["zeros"] = z
    heavy = rng.standard_cauchy(size=3000)
    heavy[1234] = 1e12
    cols["heavy"] = heavy
    return cols


def small_jets():
    rng = np.random.default_rng(2525)
    out = []
    for k, (B, N, npix, maxR) in enumerate(((1, 1, 1, 0.5), (3, 12, 24, 0.5), (70, 30, 64, 0.5), (5, 30, 24, 0.4))):
        j = np.stack((rng.exponential(0.1, size=(B, N)), rng.normal(scale=0.2, size=(B, N)), rng.normal(scale=0.2, size=(B, N))), -1)
        if N >= 12:
            bins = np.linspace(-maxR, maxR, npix + 1)
            j[0, 0, 1:] = (bins[3], bins[5])              # exactly on bin edges
            j[0, 1, 1:] = (maxR, 0.0)                     # exactly at +maxR: dropped
            j[0, 2, 1:] = (0.0, -maxR)                    # exactly at -maxR: the first bin
            j[0, 3, 1:] = (2.0 * maxR, 0.1)               # outside
            j[0, 4] = 0.0                                 # a zero-padded particle
            j[0, 5, 1:] = (bins[3], bins[5])              # the same pixel twice
            j[-1, 6, 1] = np.nan
        out.append((j, npix, maxR))
    return out


if __name__ == "__main__":
    mods = load_reference()
    U, JI = mods["utils"], mods["jet_images"]
    with open(os.path.join(OUT, "g25_err_dict.json"), "w") as f:
        json.dump({name: err_dicts(mods, name) for name in ("n12", "n30")}, f)

    arrays, meta = {}, {"columns": [], "jets": []}
    for name, col in columns().items():
        bins = np.linspace(-3.0, 3.0, 50) if name != "heavy" else S.edges(col, 4.0, 81)
        with np.errstate(all="ignore"):
            d = U.get_stats(col.copy(), bins)
        assert tuple(d) == S.KEYS
        arrays[f"col_{name}"], arrays[f"bins_{name}"] = col, bins
        arrays[f"stat_{name}"] = np.array([np.nan if d[k] is None else d[k] for k in S.KEYS], dtype=np.float64)
        meta["columns"].append(name)
    heavy = arrays["col_heavy"]
    ld = S.moments_longdouble(heavy)
    d = U.get_stats(heavy.copy(), arrays["bins_heavy"])
    meta["heavy_scipy_vs_longdouble"] = {k: abs(float(d[k]) - ld[k][0]) for k in ("skew", "kurtosis")}
    for k, (j, npix, maxR) in enumerate(small_jets()):
        arrays[f"jets_{k}"] = j
        with np.errstate(all="ignore"):
            arrays[f"images_{k}"] = JI.get_n_jet_images(j.copy(), num_jets=4, maxR=maxR, npix=npix, abs_coord=False)
            arrays[f"average_{k}"] = JI.get_average_jet_image(j.copy(), maxR=maxR, npix=npix, abs_coord=False)
        meta["jets"].append({"npix": npix, "maxR": maxR, "first_n": 4})
    meta["source"] = "utils/jet_analysis/{utils,particle_recon_err,jet_recon_err,jet_images}.py"
    np.savez_compressed(os.path.join(OUT, "g25_stats.npz"), meta=np.array(json.dumps(meta)), **arrays)
    print("g25 written:", len(meta["columns"]), "columns,", len(meta["jets"]), "jet sets; heavy:", meta["heavy_scipy_vs_longdouble"])
