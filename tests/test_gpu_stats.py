"""GPU tests of the native reconstruction statistics (csrc/stats.hip, lgn.analysis): column statistics against numpy / scipy
(tests/_stats_ref.py) and the reference-made g25 fixture, histogram edges, find_fwhm, the get_stats and recon_stats drop-ins, jet
images.  Tolerances are derived from the data (see _stats_ref): selected elements exact, interpolated order statistics within
4 * 2^-52 of their neighbours, moments against a np.longdouble two-pass evaluation."""
import json
import os

import numpy as np
import pytest
import torch

import _stats_ref as S
import _util as U
from lgn import _native as N

pytestmark = pytest.mark.gpu
T = N.STATS_TILE
IDX = {k: i for i, k in enumerate(N.STAT_NAMES)}


@pytest.fixture(scope="module")
def A():
    from lgn import analysis
    return analysis


@pytest.fixture(scope="module")
def g25():
    g = U.load("g25_stats.npz")
    return g, json.loads(str(g["meta"]))


def dev(x, dtype=torch.float64):
    return torch.as_tensor(np.ascontiguousarray(x)).to(device="cuda", dtype=dtype)


def check_column(col, row, kept, status, edges=None, alpha=4.0, what=""):
    """One column of the native output against numpy / scipy on the same values."""
    n = len(col)
    assert kept == n, what
    if n == 0:
        assert status == N.STATS_EMPTY and np.isnan(row).all() and (edges is None or np.isnan(edges).all()), what
        return
    assert status == 0, what
    with np.errstate(all="ignore"):
        ref = S.get_stats(col, np.array([0.0, 1.0]))
        ref["q10"], ref["q90"] = np.quantile(col, 0.1), np.quantile(col, 0.9)
    tol = S.order_tolerances(col)
    for k, t in tol.items():
        print(f"{what} {k}: native {row[IDX[k]]!r} ref {ref[k]!r} tol {t:.3e}")
        assert abs(row[IDX[k]] - ref[k]) <= t, (what, k, row[IDX[k]], ref[k], t)
    assert np.isnan(row[IDX["FWHM"]])
    mom = S.moments_longdouble(col)
    constant = np.ptp(col) == 0
    for k, (v, t) in mom.items():
        got = row[IDX[k]]
        print(f"{what} {k}: native {got!r} longdouble {v!r} tol {t:.3e}")
        if constant and k in ("skew", "kurtosis"):
            assert np.isnan(got), (what, k, got)
        else:
            assert abs(got - v) <= t, (what, k, got, v, t)
    for k, width in (("abs_mean_within_iqr", row[IDX["IQR"]]), ("abs_mean_within_idr", row[IDX["IDR"]])):     # the NATIVE widths
        v, t = S.within_longdouble(col, width)
        assert abs(row[IDX[k]] - v) <= t, (what, k, row[IDX[k]], v, t)
    if edges is not None:
        e = np.linspace(ref["median"] - alpha * ref["IQR"], ref["median"] + alpha * ref["IQR"], len(edges))
        te = 4 * S.U * np.abs(e).max()
        assert np.abs(edges - e).max() <= te, (what, "edges")
        assert edges[-1] == row[IDX["median"]] + alpha * row[IDX["IQR"]], (what, "the last edge is stop itself")


def run(A, x, **kw):
    out = A.column_stats(dev(x), **kw)
    return {k: v.cpu().numpy() for k, v in out.items()}


@pytest.mark.parametrize("n", [0, 1, 2, 3, 4, 5, 9, 10, 11, T - 1, T, T + 1, 2 * T + 3, 5 * T + 17])
def test_sizes(A, g25, n):
    col = g25[0][f"col_normal_{n}"] if n else np.zeros(0)
    out = run(A, col.reshape(-1, 1), num_edges=81)
    check_column(col, out["stats"][0], int(out["kept"][0]), int(out["status"][0]), out["edges"][0], what=f"n={n}")
    if n:           # and against the reference's own get_stats
        ref = g25[0][f"stat_normal_{n}"]
        tol = S.order_tolerances(col)
        for k in S.ORDER_KEYS:
            assert abs(out["stats"][0][IDX[k]] - ref[IDX[k]]) <= tol[k], (n, k)


def test_sixteen_columns_ld19_masks_and_awkward_columns(A, g25):
    g = g25[0]
    rng = np.random.default_rng(7)
    rows = 3000
    names = ["constant", "ties", "zeros", "heavy"]
    x = rng.normal(size=(rows, 19))
    x[:, 5] *= 1e-3
    cols = {}
    for c, name in enumerate(names):
        v = g[f"col_{name}"]
        x[:, c] = np.resize(v, rows)
        cols[c] = x[:, c]
    x[17, 9] = np.nan                   # column 9: NONFINITE when row 17 is kept
    x[40, 10] = np.inf
    xd = dev(x)[:, :16]                 # a view with ld = 19
    mask = rng.random(rows) < 0.6
    mask[17], mask[40] = True, False
    for keep_flag in (None, True, False):
        kw = {} if keep_flag is None else dict(mask=dev(mask, torch.bool), mask_keep=keep_flag)
        out = {k: v.cpu().numpy() for k, v in A.column_stats(xd, alpha=2.5, num_edges=50, **kw).items()}
        sel = np.ones(rows, bool) if keep_flag is None else (mask == keep_flag)
        for c in range(16):
            bad = not np.isfinite(x[sel, c]).all()
            if bad:
                assert out["status"][c] == N.STATS_NONFINITE and np.isnan(out["stats"][c]).all() and np.isnan(out["edges"][c]).all()
                assert out["kept"][c] == sel.sum()
            else:
                check_column(x[sel, c], out["stats"][c], int(out["kept"][c]), int(out["status"][c]), out["edges"][c], alpha=2.5,
                             what=f"keep={keep_flag} col={c}")
        assert (out["status"][9] != 0) == bool(sel[17]) and (out["status"][10] != 0) == bool(sel[40])
    none = run(A, x[:, :3], mask=dev(np.zeros(rows, bool), torch.bool), mask_keep=True, num_edges=5)
    assert (none["status"] == N.STATS_EMPTY).all() and (none["kept"] == 0).all() and np.isnan(none["stats"]).all()
    assert np.isnan(none["edges"]).all()


def test_empty_filtered_means_give_1e32(A):
    out = run(A, np.full((9, 1), 2.0))             # IQR = IDR = 0: nothing is within
    assert out["stats"][0][IDX["abs_mean_within_iqr"]] == 1e32 and out["stats"][0][IDX["abs_mean_within_idr"]] == 1e32
    assert np.isnan(out["stats"][0][IDX["skew"]]) and out["stats"][0][IDX["std_dev"]] == 0.0


def test_same_bits_on_every_run_and_for_every_column_count(A, g25):
    col = g25[0][f"col_normal_{5 * T + 17}"]
    rng = np.random.default_rng(3)
    x = np.stack([col] + [rng.permutation(col) for _ in range(3)], 1)
    a = run(A, x[:, :2], num_edges=81)
    b = run(A, x[:, :2], num_edges=81)
    c = run(A, x, num_edges=81)
    for k in ("stats", "edges"):
        assert np.array_equal(a[k], b[k], equal_nan=True)
        assert np.array_equal(a[k], c[k][:2], equal_nan=True)
        # the sums run over the sorted column: a permutation of the rows gives the same bits too
        assert all(np.array_equal(c[k][0], c[k][j], equal_nan=True) for j in range(1, 4))
    keep = rng.random(len(col) * 2) < 0.5          # and so does reaching the same values through a mask
    y = rng.normal(size=len(keep))
    keep[np.flatnonzero(keep)[len(col):]] = False
    extra = len(col) - keep.sum()
    if extra > 0:
        keep[np.flatnonzero(~keep)[:extra]] = True
    y[keep] = col
    d = run(A, y.reshape(-1, 1), mask=dev(keep, torch.bool), num_edges=81)
    assert np.array_equal(d["stats"][0], a["stats"][0], equal_nan=True)


def fwhm_cases():
    return [np.array([0, 1, 5, 9, 5, 9, 2, 0]), np.array([3, 3, 3, 3]), np.zeros(6, dtype=np.int64), np.array([7]),
            np.array([1, 2, 4, 8, 100, 49, 51, 50, 3]), np.arange(100)[::-1].copy()]


def test_fwhm_is_find_fwhm_bitwise(A):
    rng = np.random.default_rng(11)
    cases = fwhm_cases()
    max_bins = max(len(c) for c in cases)
    counts = np.zeros((len(cases), max_bins), dtype=np.int64)
    edges = np.zeros((len(cases), max_bins + 1))
    for i, c in enumerate(cases):
        counts[i, :len(c)] = c
        counts[i, len(c):] = 10 ** 6               # past a column's own bins: never read
        edges[i, :len(c) + 1] = np.sort(rng.normal(size=len(c) + 1))
    packed = A.PackedEdges(dev(edges), [len(c) + 1 for c in cases])
    got = A.hist_fwhm(dev(counts, torch.int64), packed).cpu().numpy()
    for i, c in enumerate(cases):
        assert got[i] == S.find_fwhm_counts(c, edges[i, :len(c) + 1]), i


def test_histogram_over_native_edges_and_fwhm(A, g25):
    g = g25[0]
    x = np.stack([np.resize(g[f"col_{k}"], 3000) for k in ("heavy", "ties", "normal_4099")], 1)
    xd = dev(x)
    out = A.column_stats(xd, num_edges=81)
    packed = A.PackedEdges(out["edges"], [81] * 3)
    counts = A.histogram(xd, packed)
    fw = A.hist_fwhm(counts, packed).cpu().numpy()
    e, h = out["edges"].cpu().numpy(), counts.cpu().numpy()
    for c in range(3):
        assert np.array_equal(h[c], np.histogram(x[:, c], e[c])[0]), c
        assert fw[c] == S.find_fwhm(x[:, c], e[c]), c


def test_three_call_chain_is_capturable(A, g25):
    g = g25[0]
    rows = 2 * T + 3
    lib = N.lib()
    x = dev(np.stack([g[f"col_normal_{rows}"], np.resize(g["col_heavy"], rows)], 1))
    nbytes = lib.lgn_column_stats_workspace_bytes(rows, 2)
    f64 = dict(device="cuda", dtype=torch.float64)
    stats, edges, fw = torch.empty(2, N.STATS_COUNT, **f64), torch.empty(2, 81, **f64), torch.empty(2, **f64)
    kept, status = torch.empty(2, device="cuda", dtype=torch.int64), torch.empty(2, device="cuda", dtype=torch.int32)
    counts = torch.empty(2, 80, device="cuda", dtype=torch.int64)
    work = torch.empty(nbytes // 8, device="cuda", dtype=torch.int64)
    import ctypes as C
    ne = (C.c_int * 2)(81, 81)

    def chain():
        s = N.stream_ptr()
        N._check(lib.lgn_column_stats_f64(N.ptr(x), rows, 2, 2, None, 1, 4.0, 81, N.ptr(stats), N.ptr(edges), N.ptr(kept), N.ptr(status),
                                          N.ptr(work), nbytes, s), "stats")
        N._check(lib.lgn_histogram_f64(N.ptr(x), rows, 2, 2, N.ptr(edges), ne, 81, None, None, N.ptr(counts), None, 80, s), "hist")
        N._check(lib.lgn_hist_fwhm_f64(N.ptr(counts), 80, N.ptr(edges), 81, ne, 2, N.ptr(fw), s), "fwhm")

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        chain()                                    # warm-up outside the capture
        side.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            chain()
    torch.cuda.synchronize()
    x.copy_(dev(np.stack([np.resize(g["col_ties"], rows), g[f"col_normal_{rows}"] * 3.0], 1)))
    graph.replay()
    torch.cuda.synchronize()
    replayed = [t.clone() for t in (stats, edges, kept, status, counts, fw)]
    chain()
    torch.cuda.synchronize()
    for a, b in zip(replayed, (stats, edges, kept, status, counts, fw)):
        assert torch.equal(a.view(torch.int64) if a.dtype == torch.float64 else a, b.view(torch.int64) if b.dtype == torch.float64 else b)
    assert int(status.abs().sum()) == 0 and int(counts.sum()) > 0


def stat_tolerances(col):
    tol = S.order_tolerances(col)
    mom = S.moments_longdouble(col)
    return tol, mom


def check_dict(got, ref, col, fwhm_tol=0.0, what=""):
    """A native get_stats dict against the reference's (None where it gives None) for the same values `col`."""
    assert list(got) == list(S.KEYS) and list(ref) == list(S.KEYS), what
    tol, mom = stat_tolerances(col)
    for k in S.KEYS:
        g, r = got[k], ref[k]
        if r is None or (isinstance(r, float) and np.isnan(r)):
            assert g is None or np.isnan(g), (what, k, g, r)
            assert (g is None) == (r is None), (what, k, g, r)
            continue
        assert isinstance(g, float), (what, k, type(g))
        if k in tol:
            t = tol[k]
        elif k in mom:
            # the reference's own float64 value is itself within the bound of the longdouble one
            t = 2 * mom[k][1]
        elif k == "FWHM":
            t = fwhm_tol
        else:
            w = got["IQR"] if k.endswith("iqr") else got["IDR"]
            rw = ref["IQR"] if k.endswith("iqr") else ref["IDR"]
            if ((np.abs(col) < w) != (np.abs(col) < rw)).any():
                continue                           # the native width selects other values: checked at the native width elsewhere
            t = 2 * S.within_longdouble(col, w)[1]
        print(f"{what} {k}: native {g!r} ref {r!r} tol {t:.3e}")
        assert abs(g - r) <= t, (what, k, g, r, t)


def test_get_stats_is_the_references(A, g25):
    g, meta = g25
    for name in meta["columns"]:
        col, bins, ref = g[f"col_{name}"], g[f"bins_{name}"], g[f"stat_{name}"]
        refd = {k: (None if np.isnan(ref[i]) and k in ("mean", "std_dev", "skew", "kurtosis") else float(ref[i]))
                for i, k in enumerate(S.KEYS)}
        for bins_dev in (False, True):
            got = A.get_stats(dev(col), dev(bins) if bins_dev else bins)
            check_dict(got, refd, col, 0.0, what=name)


def fixture_analysis(name):
    g = U.load(f"g22_analysis_{name}.npz")
    out = {k: dev(g[k]) for k in ("recons", "target", "rel_err", "part_polar", "part_polarrel", "jet_rel_err")}
    out["is_padded"] = dev(g["is_padded"], torch.bool)
    out["jet_keep"] = dev(g["jet_keep"], torch.bool)
    return g, out


@pytest.mark.parametrize("name", ["n12", "n30"])
def test_recon_stats_gives_the_references_err_dict(A, name):
    with open(os.path.join(os.path.dirname(__file__), "golden", "g25_err_dict.json")) as f:
        ref = json.load(f)[name]
    g, analysis = fixture_analysis(name)
    got = A.recon_stats(analysis)
    assert set(got) == {"particle", "jet", "hist"}
    pad = g["is_padded"].reshape(-1)
    feats = {"cartesian": g["recons"].reshape(-1, 4)[:, 1:], "polar": g["part_polar"][1].reshape(-1, 3),
             "polarrel": g["part_polarrel"][1].reshape(-1, 3)}
    assert list(got["particle"]) == list(ref["particle"]) == ["cartesian", "polar", "polarrel"]
    for f, frame in enumerate(ref["particle"]):
        assert list(got["particle"][frame]) == ["rel_err", "pad_recons"]
        data = {(fr, "rel_err"): g["rel_err"][i].reshape(-1, 3)[~pad] for i, fr in enumerate(ref["particle"])}
        data.update({(fr, "pad_recons"): feats[fr][pad] for fr in feats})
        # the FWHM bins of a column are get_bins': 50 edges median -+ 4 IQR of ANOTHER column for two of the six (see recon_stats)
        source = {("cartesian", "pad_recons"): ("cartesian", "rel_err"), ("polarrel", "rel_err"): ("polarrel", "pad_recons")}
        for kind in ("rel_err", "pad_recons"):
            x = data[frame, kind]
            src = source.get((frame, kind), (frame, kind))
            assert len(got["particle"][frame][kind]) == len(ref["particle"][frame][kind]) == 3
            for c in range(3):
                r = ref["particle"][frame][kind][c]
                # FWHM = 2 |e_i - e_j|, each edge within the edge tolerance of its source column when the counts agree
                rs = ref["particle"][src[0]][src[1]][c]
                tol = S.order_tolerances(data[src][:, c])
                edge_tol = 4 * S.U * (abs(rs["median"]) + 4 * abs(rs["IQR"])) + tol["median"] + 4 * tol["IQR"]
                check_dict(got["particle"][frame][kind][c], r, x[:, c], 4 * edge_tol + 1e-300, what=f"{frame} {kind} {c}")
    for s, system in enumerate(("cartesian", "polar")):
        keep = g["jet_keep"][s]
        assert len(got["jet"][system]) == len(ref["jet"][system]) == min(4, keep.sum())
        for c in range(len(ref["jet"][system])):
            assert got["jet"][system][c]["FWHM"] == 0.0 == ref["jet"][system][c]["FWHM"]      # by construction: constant bins
            check_dict(got["jet"][system][c], ref["jet"][system][c], g["jet_rel_err"][s][keep][:, c], 0.0, what=f"jet {system} {c}")
    for k, h in got["hist"].items():
        assert h["counts"].shape[1] == 80 and h["edges"].shape[1] == 81 and h["counts"].is_cuda
    h = got["hist"]["rel_err_cartesian"]
    x = g["rel_err"][0].reshape(-1, 3)[~pad]
    for c in range(3):
        assert np.array_equal(h["counts"][c].cpu().numpy(), np.histogram(x[:, c], h["edges"][c].cpu().numpy())[0])


def test_recon_stats_with_custom_ranges(A):
    """custom_particle_recons_ranges=True: the given edges are get_stats' FWHM bins and the bins that are drawn; nothing else moves."""
    g, analysis = fixture_analysis("n12")
    rng = np.random.default_rng(12)
    ranges = tuple((tuple(np.linspace(-3.0 - c, 2.0 + f, 41 + 10 * c) for c in range(3)),
                    tuple(np.sort(rng.normal(scale=2.0, size=30 + f + c)) for c in range(3))) for f in range(3))
    plain, got = A.recon_stats(analysis), A.recon_stats(analysis, custom_ranges=ranges)
    pad = g["is_padded"].reshape(-1)
    feats = {"cartesian": g["recons"].reshape(-1, 4)[:, 1:], "polar": g["part_polar"][1].reshape(-1, 3),
             "polarrel": g["part_polarrel"][1].reshape(-1, 3)}
    assert got["jet"] == plain["jet"]
    for f, frame in enumerate(("cartesian", "polar", "polarrel")):
        for k, (kind, name, x) in enumerate((("rel_err", f"rel_err_{frame}", g["rel_err"][f].reshape(-1, 3)[~pad]),
                                            ("pad_recons", f"padded_{frame}", feats[frame][pad]))):
            h = got["hist"][name]
            assert h["n_edges"] == [len(b) for b in ranges[f][k]]
            for c in range(3):
                bins = ranges[f][k][c]
                d, p = got["particle"][frame][kind][c], plain["particle"][frame][kind][c]
                assert d["FWHM"] == S.find_fwhm(x[:, c], bins), (name, c)
                assert {a: v for a, v in d.items() if a != "FWHM"} == {a: v for a, v in p.items() if a != "FWHM"}
                assert np.array_equal(h["edges"][c, :len(bins)].cpu().numpy(), bins)
                assert np.array_equal(h["counts"][c, :len(bins) - 1].cpu().numpy(), np.histogram(x[:, c], bins)[0]), (name, c)


def test_recon_stats_without_padded_particles(A):
    g, _ = fixture_analysis("n12")
    meta = json.loads(str(g["meta"]))
    full = [b for b in range(g["target"].shape[0]) if b not in meta["padded_kept"]]
    t, r = dev(g["target"][full]), dev(g["recons"][full])
    analysis = A.recon_analysis(t, r)
    assert not bool(analysis["is_padded"].any())
    got = A.recon_stats(analysis)
    for frame in ("cartesian", "polar", "polarrel"):
        assert got["particle"][frame]["pad_recons"] == [] and len(got["particle"][frame]["rel_err"]) == 3
        assert list(got["particle"][frame]["rel_err"][0]) == list(S.KEYS)
    rel = analysis["rel_err"][1].reshape(-1, 3).cpu().numpy()
    assert abs(got["particle"]["polar"]["rel_err"][2]["median"] - np.median(rel[:, 2])) <= S.order_tolerances(rel[:, 2])["median"]
    assert np.isnan(got["particle"]["polarrel"]["rel_err"][0]["FWHM"])      # its bins come from the (empty) padded features


# ---- jet images ------------------------------------------------------------------------------------------------------------------------

def test_jet_images_mode0_against_the_reference(A, g25):
    g, meta = g25
    for k, m in enumerate(meta["jets"]):
        jets = g[f"jets_{k}"]
        B, n = jets.shape[:2]
        images, average = A.jet_image(dev(jets), None, 0, m["npix"], m["maxR"], m["first_n"])
        again = A.jet_image(dev(jets), None, 0, m["npix"], m["maxR"], m["first_n"])
        assert torch.equal(images, again[0]) and torch.equal(average.view(torch.int64), again[1].view(torch.int64))
        images, average = images.cpu().numpy(), average.cpu().numpy()
        assert images.shape == g[f"images_{k}"].shape == (min(B, 4), m["npix"], m["npix"])          # first_n > B at B = 1, 3
        spt = np.nansum(jets[:, :, 0], axis=1)
        for b in range(len(images)):
            assert np.abs(images[b] - g[f"images_{k}"][b]).max() <= n * S.U * spt[b], (k, b)
            assert np.array_equal(images[b] != 0, g[f"images_{k}"][b] != 0), (k, b)
        assert np.abs(average - g[f"average_{k}"]).max() <= (n + B) * S.U * spt.sum() / B, k
        ref_images, ref_avg = S.jet_images(jets, None, 0, m["npix"], m["maxR"], 4)
        assert np.array_equal(ref_images, g[f"images_{k}"]) and np.array_equal(ref_avg, g[f"average_{k}"])


@pytest.mark.parametrize("mode", [1, 2])
def test_jet_images_in_a_frame(A, mode):
    rng = np.random.default_rng(40 + mode)
    for B, n, npix in ((1, 1, 1), (3, 12, 24), (70, 30, 64)):
        def make():
            phi0, eta0 = rng.uniform(-3, 3, size=(B, 1)), rng.normal(size=(B, 1))
            j = np.stack((rng.exponential(20.0, size=(B, n)), eta0 + rng.normal(scale=0.15, size=(B, n)),
                          phi0 + rng.normal(scale=0.15, size=(B, n))), -1)
            j[0, n // 2] = 0.0                                  # a zero-padded particle
            return j
        jets, other = make(), make()
        other[:, :, 1:] = jets[:, :, 1:] + rng.normal(scale=0.02, size=(B, n, 2))
        fr = other if mode == 2 else None
        images, average = (x.cpu().numpy() for x in A.jet_image(dev(jets), None if fr is None else dev(fr), mode, npix, 0.5, 100))
        ref_images, ref_avg = S.jet_images(jets, fr, mode, npix, 0.5, 100)
        assert images.shape == (B, npix, npix)
        norm = S.normalize(jets, S.frame(fr if mode == 2 else jets))
        spt = norm[:, :, 0].sum(1)
        # a particle within a few ulp of a pixel edge may land next door (device cos / sin / sinh are not libm's): none here
        for b in range(B):
            assert np.abs(images[b] - ref_images[b]).max() <= (n + 16) * S.U * spt[b], (B, b)
        assert np.abs(average - ref_avg).max() <= (n + B + 16) * S.U * spt.sum() / B


def test_jet_images_escape_when_every_jet_is_at_rest(A):
    rng = np.random.default_rng(9)
    B, n = 5, 4
    jets = np.stack((rng.exponential(1.0, size=(B, n)), rng.normal(scale=0.2, size=(B, n)), rng.normal(scale=0.2, size=(B, n))), -1)
    jets[:, 2:, 0] = jets[:, :2, 0]
    jets[:, 2:, 1] = -jets[:, :2, 1]
    jets[:, 2:, 2] = jets[:, :2, 2] + np.pi                      # back to back: Pt ~ 1e-16 for every jet
    assert np.isclose(S.frame(jets)[:, 0], 0).all()
    raw = A.jet_image(dev(jets), None, 0, 24, 4.0, B)
    esc = A.jet_image(dev(jets), None, 1, 24, 4.0, B)
    assert torch.equal(raw[0], esc[0]) and torch.equal(raw[1], esc[1])
    jets[0, 0, 0] += 3.0                                        # one moving jet: every jet is normalised
    got = A.jet_image(dev(jets), None, 1, 24, 4.0, B)[0].cpu().numpy()
    ref = S.jet_images(jets, None, 1, 24, 4.0, B)[0]
    assert np.abs(got[0] - ref[0]).max() <= 64 * S.U * np.abs(ref[0]).max()
    assert not np.array_equal(got[0], raw[0][0].cpu().numpy())


def test_jet_images_drop_in(A, g25):
    g, meta = g25
    jets, m = g["jets_1"], meta["jets"][1]
    out = A.jet_images(dev(jets), dev(jets[::-1].copy()), 2, m["npix"], abs_coord=False, same_norm=True, maxR=m["maxR"])
    assert [a.shape for a in out] == [(24, 24), (24, 24), (2, 24, 24), (2, 24, 24)]
    assert np.array_equal(out[2], A.jet_image(dev(jets), None, 0, 24, m["maxR"], 2)[0].cpu().numpy())
    same = A.jet_images(dev(jets), dev(jets), 2, 24, abs_coord=True, same_norm=True)
    own = A.jet_images(dev(jets), dev(jets), 2, 24, abs_coord=True, same_norm=False)
    assert all(np.array_equal(a, b) for a, b in zip(same, own))   # the target's frame is its own


def test_refusals(A):
    x = torch.zeros(8, 2, dtype=torch.float64)
    with pytest.raises(RuntimeError):
        A.column_stats(x)
    with pytest.raises(RuntimeError):
        A.get_stats(x[:, 0], np.linspace(0, 1, 5))
    with pytest.raises(RuntimeError):
        A.jet_image(torch.zeros(2, 3, 3, dtype=torch.float64))
    j = torch.zeros(2, 3, 3, dtype=torch.float64, device="cuda")
    for kw in (dict(npix=0), dict(npix=65), dict(maxR=0.0), dict(maxR=-1.0), dict(maxR=float("inf")), dict(mode=2)):
        with pytest.raises(ValueError):
            A.jet_image(j, **kw)
    with pytest.raises(ValueError):
        A.column_stats(torch.zeros(8, 0, dtype=torch.float64, device="cuda"))
    with pytest.raises(ValueError):
        A.column_stats(torch.zeros(8, 17, dtype=torch.float64, device="cuda"))
    with pytest.raises(ValueError):
        A.column_stats(x.cuda(), num_edges=1)
    lib = N.lib()
    xd, out = x.cuda(), torch.zeros(64, dtype=torch.float64, device="cuda")
    need = lib.lgn_column_stats_workspace_bytes(8, 2)
    work = torch.zeros(need // 8, dtype=torch.int64, device="cuda")
    args = lambda nbytes: (N.ptr(xd), 8, 2, 2, None, 1, 4.0, 0, N.ptr(out), None, N.ptr(work), N.ptr(work), N.ptr(work), nbytes, None)
    assert lib.lgn_column_stats_f64(*args(need - 1)) < 0 and "too short" in N.last_error()
    need = lib.lgn_jet_images_workspace_bytes(2, 8)
    assert lib.lgn_jet_images_f64(N.ptr(j), None, 2, 3, 0, 8, 0.5, 0, None, N.ptr(out), N.ptr(work), need - 1, None) < 0
    assert "too short" in N.last_error()
