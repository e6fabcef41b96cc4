"""Host-side checks of the reconstruction analysis: the numpy / scipy restatement (tests/_analysis_ref.py) against the reference-pinned
g22 fixtures, its histogram rule against np.histogram, the new C entry points' symbols, and their refusals before any launch.
No GPU needed."""
import ctypes as C

import numpy as np
import pytest
import torch

import _analysis_ref as R
from _util import load, meta
from lgn import _native as N

G22 = ("g22_analysis_n12.npz", "g22_analysis_n30.npz", "g22_analysis_n150.npz")


assert_same, assert_mass = R.assert_same, R.assert_mass


@pytest.mark.parametrize("name", G22)
def test_restatement_matches_the_reference_fixture(name):
    z = load(name)
    m = meta(z)
    # on the fixture's own frames the assignments and the gathers are the reference's, bit for bit
    rel, col, status = R.matched_rel_err(z["target"][..., 1:], z["recons"][..., 1:], *z["part_polar"], *z["part_polarrel"])
    assert np.array_equal(col, z["col4row"]) and (status == 0).all() and np.array_equal(rel, z["rel_err"], equal_nan=True)
    # from the inputs: numpy's asinh / atan2 differ from torch's in the last bit, which can reorder the exactly tied relative-polar
    # costs of a padded jet; everything else is pinned
    want = R.recon_analysis(z["target"], z["recons"])
    assert (want["status"] == 0).all()
    assert np.array_equal(want["col4row"][0], z["col4row"][0])
    tied = [b for b in m["padded_kept"] if not np.array_equal(want["col4row"][1, b], z["col4row"][1, b])]
    firm = np.setdiff1d(np.arange(m["B"]), tied)
    assert np.array_equal(want["col4row"][1, firm], z["col4row"][1, firm])
    for b in tied:
        R.assert_tied_assignment(z["part_polarrel"][0, b], z["part_polarrel"][1, b], want["col4row"][1, b], z["col4row"][1, b],
                                 want["rel_err"][2, b], f"{name} jet {b}")
    # rtol 1e-12, but 1e-11 for the relative-polar frame and its errors: eta_rel = Eta - eta and the wrapped phi_rel cancel, which
    # magnifies the last-bit difference between numpy's and torch's asinh / atan2 (measured: 6.5e-12 on 2 of 3150 relative-polar
    # errors of n150, 2e-12 on 3 of n30; everything else is under 1e-12)
    assert_same(want["rel_err"][:2], z["rel_err"][:2], 1e-12, f"{name} rel_err Cartesian, polar")
    assert_same(want["rel_err"][2, firm], z["rel_err"][2, firm], 1e-11, f"{name} rel_err polarrel")
    assert_same(want["part_polar"], z["part_polar"], 1e-12, f"{name} part_polar")
    assert_same(want["part_polarrel"], z["part_polarrel"], 1e-11, f"{name} part_polarrel")
    assert_same(want["jet_rel_err"][:, :, 1:], z["jet_rel_err"][:, :, 1:], 1e-12, f"{name} jet_rel_err")
    for k in ("jet_cart", "jet_polar"):
        assert_same(want[k][..., 1:], z[k][..., 1:], 1e-12, f"{name} {k}")
        for side, p in enumerate((z["target"], z["recons"])):
            assert_mass(want[k][side, :, 0], p, f"{name} {k} mass")
            assert_mass(z[k][side, :, 0], p, f"{name} {k} fixture mass")
    # the mass component of the jet relative error: the masses themselves differ by the cancellation in m^2 (above), so the
    # definition -- (recons - target) / (recons + 1e-16) -- is checked on each side's own masses, where it is exact
    for src in (want, z):
        for k, f in (("jet_cart", 0), ("jet_polar", 1)):
            m_t, m_r = src[k][0][:, 0], src[k][1][:, 0]
            assert np.array_equal(src["jet_rel_err"][f][:, 0], (m_r - m_t) / (m_r + 1e-16), equal_nan=True), (name, k)
    assert np.array_equal(want["is_padded"], z["is_padded"]) and np.array_equal(want["jet_keep"], z["jet_keep"])
    assert m["B"] == z["target"].shape[0] and (m["N"] > 25 or not m["dropped"])
    assert all(b in [p[0] for p in m["pad"]] for b in m["dropped"])


def test_fixture_n12_holds_the_degenerate_jets():
    z = load("g22_analysis_n12.npz")
    m = meta(z)
    assert not m["dropped"] and len(m["pad"]) == 4 and min(n for _, n in m["pad"]) == 3
    assert np.array_equal(z["recons"][m["same"][0]], z["target"][m["same"][0]])
    assert z["is_padded"].sum() == sum(m["N"] - n for _, n in m["pad"])


def _edge_data(edges, rng):
    e = np.asarray(edges)
    return np.concatenate([e, np.nextafter(e, np.inf), np.nextafter(e, -np.inf), [np.nan, np.inf, -np.inf],
                           rng.uniform(e[0] - 1, e[-1] + 1, size=200)])


@pytest.mark.parametrize("edges", [np.array([0.0, 1.0]), np.linspace(-2.0, 3.0, 82), np.linspace(-1.0, 1.0, 1025),
                                   np.array([0.0, 0.5, 0.5, 0.5, 2.0, 2.0])])
def test_histogram_rule_is_numpys(edges):
    rng = np.random.default_rng(len(edges))
    v = _edge_data(edges, rng)
    w = rng.normal(size=len(v))
    keep = rng.random(len(v)) < 0.7
    x = v[:, None]
    assert np.array_equal(R.histogram(x, [edges])[0], np.histogram(v, bins=edges)[0])
    assert np.array_equal(R.histogram(x, [edges], keep=keep)[0], np.histogram(v[keep], bins=edges)[0])
    got, want = R.histogram(x, [edges], weights=w)[0], np.histogram(v, bins=edges, weights=w)[0]
    np.testing.assert_allclose(got, want, rtol=0, atol=len(v) * 2.0 ** -52 * np.abs(w).sum())


def test_analysis_symbols_are_exported():
    lib = N.lib()
    for name in ("lgn_recon_analysis_f64", "lgn_match_rel_err_f64", "lgn_histogram_f64"):
        assert name in N.EXPORTED_SYMBOLS
        assert hasattr(lib, name)
    assert lib.lgn_abi_version() == 19 and N.ABI_VERSION == 19


P = 8          # placeholder device pointer: every call below must be refused before anything touches it


def _analysis(target=P, recons=P, B=4, n=30, jets=(P, P, P, P), rel=(P, P, P, P)):
    return N.lib().lgn_recon_analysis_f64(target, recons, B, n, 1, 1, P, P, *jets, *rel, None)


@pytest.mark.parametrize("kw,what", [
    (dict(n=0), "N = 0"),
    (dict(n=193), "N = 193"),
    (dict(B=-1), "B = -1"),
    (dict(target=None), "null input"),
    (dict(recons=None), "null input"),
    (dict(jets=(P, None, P, P)), "null jet output"),
    (dict(rel=(P, P, P, None)), "rel_err without status"),
    (dict(rel=(P, P, None, P)), "rel_err without is_padded"),
    (dict(rel=(None, P, None, None)), "col4row without rel_err"),
])
def test_recon_analysis_refusals(kw, what):
    assert _analysis(**kw) < 0
    assert what in N.last_error()


def test_recon_analysis_of_no_jets_is_no_work():
    assert _analysis(B=0) == 0


def _hist(x=P, rows=10, ld=3, cols=3, edges=P, n_edges=(2, 82, 5), max_edges=82, weights=None, counts=P, wcounts=None, max_bins=81):
    ne = (C.c_int * len(n_edges))(*n_edges) if n_edges is not None else None
    return N.lib().lgn_histogram_f64(x, rows, ld, cols, edges, ne, max_edges, None, weights, counts, wcounts, max_bins, None)


@pytest.mark.parametrize("kw,what", [
    (dict(n_edges=(2, 1, 5)), "n_edges = 1"),
    (dict(n_edges=(2, 83, 5)), "n_edges = 83"),
    (dict(n_edges=None), "null n_edges"),
    (dict(max_edges=1026), "max_edges = 1026"),
    (dict(max_bins=80), "max_bins = 80"),
    (dict(cols=0), "cols = 0"),
    (dict(cols=17), "cols = 17"),
    (dict(ld=2), "ld = 2"),
    (dict(rows=-1), "rows = -1"),
    (dict(x=None), "null x"),
    (dict(edges=None), "null edges"),
    (dict(counts=None), "exactly one"),
    (dict(weights=P), "exactly one"),
])
def test_histogram_refusals(kw, what):
    assert _hist(**kw) < 0
    assert what in N.last_error()


def test_analysis_without_a_gpu_raises(monkeypatch):
    from lgn import analysis as A
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    x = torch.zeros(2, 5, 4)
    with pytest.raises(RuntimeError, match="needs a GPU"):
        A.recon_analysis(x, x)
    with pytest.raises(RuntimeError, match="needs a GPU"):
        A.histogram(torch.zeros(4, 1), np.array([0.0, 1.0]))
