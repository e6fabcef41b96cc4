"""Host-side tests of the native reconstruction statistics (no GPU): the numpy / scipy restatement tests/_stats_ref.py against the
reference-made g25 fixture, the C ABI of csrc/stats.hip (symbols, header, version, every argument refusal before any launch), the host
halves of lgn.analysis' drop-ins and their refusal of CPU tensors."""
import json
import os

import numpy as np
import pytest
import torch

import _stats_ref as S
import _util as U
from lgn import _native as N

P = 16          # placeholder device pointer: every call below must be refused before anything touches it
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "lgn_amd.h")
NEW = ("lgn_column_stats_workspace_bytes", "lgn_column_stats_f64", "lgn_hist_fwhm_f64", "lgn_jet_images_workspace_bytes",
       "lgn_jet_images_f64")


@pytest.fixture(scope="module")
def g25():
    g = U.load("g25_stats.npz")
    return g, json.loads(str(g["meta"]))


def test_restatement_reproduces_the_reference_fixture(g25):
    g, meta = g25
    for name in meta["columns"]:
        col, bins, ref = g[f"col_{name}"], g[f"bins_{name}"], g[f"stat_{name}"]
        mine = S.get_stats(col, bins)
        for i, k in enumerate(S.KEYS):
            v = np.nan if mine[k] is None else mine[k]
            if k in S.MOMENT_KEYS or k.startswith("abs_mean_within"):
                assert (np.isnan(v) and np.isnan(ref[i])) or abs(v - ref[i]) <= 1e-13 * abs(ref[i]), (name, k)
            else:                       # order statistics and FWHM: bitwise
                assert v == ref[i], (name, k, v, ref[i])
    for k, m in enumerate(meta["jets"]):
        images, average = S.jet_images(g[f"jets_{k}"], None, 0, m["npix"], m["maxR"], m["first_n"])
        assert np.array_equal(images, g[f"images_{k}"]) and np.array_equal(average, g[f"average_{k}"])
    assert set(meta["heavy_scipy_vs_longdouble"]) == {"skew", "kurtosis"}


def test_fixture_err_dict_has_the_references_shape():
    with open(os.path.join(os.path.dirname(HEADER), "..", "tests", "golden", "g25_err_dict.json")) as f:
        ref = json.load(f)
    for name in ("n12", "n30"):
        for frame in ("cartesian", "polar", "polarrel"):
            for kind in ("rel_err", "pad_recons"):
                assert [tuple(d) for d in ref[name]["particle"][frame][kind]] == [S.KEYS] * 3
        for system in ("cartesian", "polar"):
            assert [tuple(d) for d in ref[name]["jet"][system]] == [S.KEYS] * 4
            assert all(d["FWHM"] == 0.0 for d in ref[name]["jet"][system])


def test_symbols_header_and_abi():
    lib = N.lib()
    with open(HEADER) as f:
        header = f.read()
    for name in NEW:
        assert name in N.EXPORTED_SYMBOLS and hasattr(lib, name) and f" {name}(" in header, name
    assert lib.lgn_abi_version() == N.ABI_VERSION == 19 and "#define LGN_AMD_ABI_VERSION 19 " in header
    for i, name in enumerate(N.STAT_NAMES):
        assert f"#define LGN_STAT_{name.upper()} {i}\n" in header, name
    assert f"#define LGN_STATS_COUNT {N.STATS_COUNT}\n" in header and f"#define LGN_STATS_TILE {N.STATS_TILE}\n" in header
    assert f"#define LGN_STATS_MAX_COLS {N.STATS_MAX_COLS}\n" in header and N.STATS_MAX_COLS >= 16
    assert f"#define LGN_JET_IMAGE_MAX_NPIX {N.JET_IMAGE_MAX_NPIX}\n" in header and N.JET_IMAGE_MAX_NPIX >= 64
    assert f"#define LGN_JET_IMAGE_PARTS {N.JET_IMAGE_PARTS}\n" in header
    assert N.STAT_NAMES[:17] == S.KEYS


def stats_call(x=P, rows=100, ld=3, cols=3, alpha=4.0, num_edges=81, stats=P, edges=P, kept=P, status=P, work=P, nbytes=1 << 40):
    return N.lib().lgn_column_stats_f64(x, rows, ld, cols, None, 1, alpha, num_edges, stats, edges, kept, status, work, nbytes, None)


@pytest.mark.parametrize("kw, text", [
    (dict(x=None), "null"), (dict(stats=None), "null"), (dict(edges=None), "null"), (dict(kept=None), "null"), (dict(status=None), "null"),
    (dict(work=None), "null"), (dict(rows=-1), "rows"), (dict(rows=1 << 31), "rows"), (dict(cols=0), "cols"), (dict(cols=17, ld=17), "cols"),
    (dict(ld=2), "ld"), (dict(num_edges=1), "num_edges"), (dict(num_edges=1026), "num_edges"), (dict(num_edges=-3), "num_edges"),
    (dict(alpha=float("nan")), "alpha"), (dict(alpha=float("inf")), "alpha"), (dict(nbytes=1000), "too short"),
    (dict(work=P + 4), "aligned")])
def test_column_stats_refusals(kw, text):
    assert stats_call(**kw) < 0 and text in N.last_error()


def test_workspace_queries():
    lib = N.lib()
    assert lib.lgn_column_stats_workspace_bytes(0, 1) > 0
    small, big = lib.lgn_column_stats_workspace_bytes(1000, 2), lib.lgn_column_stats_workspace_bytes(100000, 16)
    assert 2 * 8 * 1000 * 2 <= small < big and big >= 2 * 8 * 100000 * 16
    for rows, cols in ((-1, 1), (1 << 31, 1), (10, 0), (10, 17)):
        assert lib.lgn_column_stats_workspace_bytes(rows, cols) < 0
    assert lib.lgn_jet_images_workspace_bytes(70, 64) >= 70 * 64 * 64 * 8
    assert lib.lgn_jet_images_workspace_bytes(10 ** 6, 64) < 1 << 26          # the partial images do not grow with B past the parts
    for B, npix in ((0, 8), (4, 0), (4, 65)):
        assert lib.lgn_jet_images_workspace_bytes(B, npix) < 0


def images_call(jets=P, frame=None, B=4, n=30, mode=0, npix=24, maxR=0.5, first_n=2, images=P, average=P, work=P, nbytes=1 << 40):
    return N.lib().lgn_jet_images_f64(jets, frame, B, n, mode, npix, maxR, first_n, images, average, work, nbytes, None)


@pytest.mark.parametrize("kw, text", [
    (dict(jets=None), "null"), (dict(average=None), "null"), (dict(images=None), "null"), (dict(work=None), "null"),
    (dict(mode=2), "null"), (dict(B=0), "B ="), (dict(n=0), "N ="), (dict(n=193), "N ="), (dict(npix=0), "npix"), (dict(npix=65), "npix"),
    (dict(maxR=0.0), "maxR"), (dict(maxR=-0.5), "maxR"), (dict(maxR=float("nan")), "maxR"), (dict(maxR=float("inf")), "maxR"),
    (dict(mode=3), "mode"), (dict(first_n=-1), "first_n"), (dict(nbytes=100), "too short"), (dict(work=P + 4), "aligned")])
def test_jet_images_refusals(kw, text):
    assert images_call(**kw) < 0 and text in N.last_error()


def test_hist_fwhm_refusals():
    import ctypes as C
    lib = N.lib()
    ne = (C.c_int * 2)(81, 81)
    assert lib.lgn_hist_fwhm_f64(None, 80, P, 81, ne, 2, P, None) < 0 and "null" in N.last_error()
    assert lib.lgn_hist_fwhm_f64(P, 80, P, 81, ne, 0, P, None) < 0 and "cols" in N.last_error()
    assert lib.lgn_hist_fwhm_f64(P, 80, P, 81, ne, 17, P, None) < 0 and "cols" in N.last_error()
    assert lib.lgn_hist_fwhm_f64(P, 70, P, 81, ne, 2, P, None) < 0 and "max_bins" in N.last_error()
    assert lib.lgn_hist_fwhm_f64(P, 80, P, 80, ne, 2, P, None) < 0 and "n_edges" in N.last_error()
    ne[1] = 1
    assert lib.lgn_hist_fwhm_f64(P, 80, P, 81, ne, 2, P, None) < 0 and "n_edges" in N.last_error()


def test_stats_dict_is_the_references_dict():
    from lgn import analysis as A
    row = np.arange(N.STATS_COUNT, dtype=np.float64) + 0.5
    d = A.stats_dict(row, 7.0, 12)
    assert tuple(d) == S.KEYS and all(type(v) is float for v in d.values())
    assert d["FWHM"] == 7.0 and d["median"] == 0.5 and d["abs_mean_within_idr"] == 16.5 and "q10" not in d
    json.dumps(d)
    nan = np.full(N.STATS_COUNT, np.nan)
    d = A.stats_dict(nan, np.nan, 5)          # a NONFINITE column: None exactly where get_stats maps NaN to None
    assert [k for k, v in d.items() if v is None] == ["mean", "std_dev", "skew", "kurtosis"]
    assert np.isnan(d["median"]) and np.isnan(d["FWHM"]) and np.isnan(d["max"])
    d = A.stats_dict(nan, np.nan, 0)          # an empty one: np.max raises there
    assert [k for k, v in d.items() if v is None] == ["mean", "max", "min", "abs_min", "std_dev", "skew", "kurtosis"]
    const = row.copy()
    const[[11, 12]] = np.nan                  # a constant column: skew and kurtosis are 0 / 0
    d = A.stats_dict(const, 0.0, 9)
    assert d["skew"] is None and d["kurtosis"] is None and d["std_dev"] == 10.5


def test_cpu_tensors_are_refused():
    from lgn import analysis as A
    x = torch.zeros(8, 2, dtype=torch.float64)
    for call in (lambda: A.column_stats(x), lambda: A.get_stats(x[:, 0], np.linspace(0, 1, 5)),
                 lambda: A.jet_image(torch.zeros(2, 3, 3, dtype=torch.float64)),
                 lambda: A.jet_images(torch.zeros(2, 3, 3), torch.zeros(2, 3, 3), 1, 8, True),
                 lambda: A.hist_fwhm(torch.zeros(1, 4, dtype=torch.int64), None),
                 lambda: A.recon_stats({"rel_err": torch.zeros(3, 1, 2, 3)})):
        with pytest.raises(RuntimeError, match="GPU"):
            call()
