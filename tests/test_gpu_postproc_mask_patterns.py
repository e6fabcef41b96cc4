"""The post-processing calls on jets with holes, sparse jets and disagreeing labels: anomaly.hip + emd.hip (22 scores), analysis.hip
(matched residuals, jet quantities, histograms), stats.hip (column statistics, recon_stats) and roc.hip, each against its restatement
(tests/_anomaly_ref.py, _emd_ref.py, _analysis_ref.py, _stats_ref.py, _roc_ref.py) at the tolerances of test_gpu_anomaly.py,
test_gpu_analysis.py, test_gpu_stats.py and test_gpu_roc.py for the same quantities, unchanged.

None of these calls reads labels; each takes padding from the numbers.  Two kinds of input: (a) _jets.pattern_jets + recon_like
through tests/_mask_cases.py at N = 12, 30, 65; (b) the device's own output -- NativeEvalStep.run on HOLED at live weights (maxdim 2
N = 30, maxdim 3 N = 13; the networks and weights of tests/test_gpu_mask_patterns.py), chained into the calls without a host sync,
the restatement fed the reconstruction copied back.  In (b) the all-masked jet is exactly zero on both sides because the decoder
returns exactly zero for it (g28), not because a generator wrote zeros.

    call                                   input                       held to
    score_tensor(emd=True), 22 columns     (a) 3 batches x N 12 30 65  test_gpu_anomaly._check_against_restatement: the six assignments
                                           (b) 2 eval steps            optima and scored as found; column 22 _emd_ref at 1e-11; the NaN
                                                                       pattern and the status word of the all-zero jet exactly; every
                                                                       other jet bit-equal to a call without it
    recon_analysis, find_match x abs_coord (a), (b)                    test_gpu_analysis._check / its identity-pairing assertions; rows
                                                                       padded in mid-jet flagged by the +-inf rule; the all-zero jet's
                                                                       0/0 rows NOT padded, status 0, as the restatement has it
    column_stats, recon_stats,             (a) HOLED N 30, the two     test_gpu_stats.check_column / check_dict on every finite column;
    particle_histograms                    empty jets alone            a column with a NaN among its kept rows: STATS_NONFINITE, NaN
                                                                       statistics, the count kept; histograms exactly _analysis_ref's
    roc_auc_tensor                         22 columns, HOLED x 2 seeds test_gpu_roc.check (curves exactly, AUC at auc_tolerance); six
                                           against SPARSE x 2 seeds    jets tie at score 0 across the classes; the EMD column holds
                                                                       NaN: ROC_NONFINITE, and get_ROC_AUC raises
    eval step -> scores -> ROC and         HOLED maxdim 2 N 30, two    one graph, replayed on a second batch, bit-equal to eager calls
    eval step -> analysis -> histogram     batches

What these inputs would catch, measured on the CPU (tests/test_host_mask_cases.py): (iii) is_padded taken from `target == 0` instead of
the +-inf rule flags the N rows of the all-zero jet that the restatement leaves unflagged, and moves no other jet -- the kept rows of
the Cartesian residual statistics then lose their N NaN entries (status NONFINITE -> 0: every statistic of three columns changes
from NaN to a number) and the padded-particle histograms gain N zeros; counts are compared exactly.  (i) and (ii) of
tests/test_gpu_loss_mask_patterns.py apply to the EMD column.

Measured on the MI355X: every case of (a) passes at the four files' tolerances as they stand; kernel bugs found: none.  The native
assignment equals scipy's in the Cartesian, normalised Cartesian and Lorentz variants on every jet, holes included.  Input (b) carries six
measured tolerances, all on the one-particle jet `one_last` (a Lorentz-equivariant network reconstructs it as multiples of its
particle, so its EMD, its relative coordinates and its matched polar residuals are rounding residues of O(1) operands):
_mask_cases.EVAL_CONDITIONING, 100 x the restatement's disagreement with itself measured on the oracle's reconstruction.
NOT covered: the jet images, and a graph capture that includes the evaluation step itself (the step replays its own graph)."""
import functools

import numpy as np
import pytest
import torch

import _analysis_ref as R
import _anomaly_ref as AR
import _emd_ref as E
import _mask_cases as C
import _stats_ref as S

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BATCH_NAMES = ["sparse", "holed", "disagree"]


def dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    return t if dtype is None else t.to(dtype)


def _arrs(x, t):
    """[recons, target, recons_n, target_n] numpy from (B, N, 4) tensors."""
    return [z.numpy() for z in (x, t, C.normalized(x), C.normalized(t))]


# ---- scores -----------------------------------------------------------------------------------------------------------------------

def _check_scores(arrs, sc, st, col, empty, what, floors=None):
    """22 device columns, the status word and the six assignments against the restatements on the same float64 arrays.
    floors: the name of an evaluation case whose measured absolute term of the EMD column (_mask_cases.EVAL_CONDITIONING) applies."""
    from lgn import _native as N_
    from lgn import anomaly as A
    from test_gpu_anomaly import _check_against_restatement
    B = len(arrs[0])
    clean = [b for b in range(B) if b not in empty]
    got = sc.cpu().numpy()
    assert got.shape == (B, 22)
    want, _ = AR.anomaly_scores(*arrs)
    assert st.cpu().tolist() == [(N_.EMD_EMPTY << A.EMD_STATUS_SHIFT) if b in empty else 0 for b in range(B)], (what, st.cpu().tolist())
    assert np.isfinite(want).all() and np.isfinite(got[:, :21]).all(), f"{what}: the restatement's 21 scores hold no NaN, nor may the device's"
    assert np.isnan(got[empty, 21]).all() and np.isfinite(got[clean, 21]).all(), f"{what}: the EMD column is NaN on the all-zero jets alone"
    assert np.array_equal(got[empty, :21], want[empty]), f"{what}: the all-zero jet's 21 scores are the restatement's (0)"
    assert (col.cpu().numpy() >= 0).all(), "every assignment was written"
    _check_against_restatement(arrs, got, col.cpu().numpy(), what)
    emd = E.emd_relative(arrs[0][clean], arrs[1][clean])
    floor = np.zeros(len(clean)) if floors is None else C.eval_floors(floors, "emd", B)[clean]
    err = np.abs(got[clean, 21] - emd)
    assert (err <= 1e-11 * np.abs(emd) + floor).all(), f"{what} EMD column: {err} against {1e-11 * np.abs(emd) + floor}"
    return clean


@pytest.mark.parametrize("batch", BATCH_NAMES)
@pytest.mark.parametrize("N", [12, 30, 65])
def test_scores_on_mask_patterns(N, batch):
    from lgn import anomaly as A
    x, t, _ = C.pair(N, batch)
    arrs = _arrs(x, t)
    xs = [dev(a) for a in arrs]
    col = torch.full((6, len(x), N), -7, device=DEV, dtype=torch.int32)
    sc, st = A.score_tensor(*xs, return_status=True, col4row=col, emd=True)
    clean = _check_scores(arrs, sc, st, col, C.empty_jets(batch), f"{batch} N {N}")
    alone, st2 = A.score_tensor(*[z[clean] for z in xs], return_status=True, emd=True)
    assert torch.equal(sc[clean], alone) and int(st2.abs().max()) == 0, "every other jet is bit-equal to a call without the all-zero jets"
    with pytest.raises(ValueError, match="EMD score: both events are weightless"):
        A.anomaly_scores(*xs, include_emd="native")


# ---- analysis ---------------------------------------------------------------------------------------------------------------------

def _check_analysis(got, want, t, x, empty, kw, what, floors=None):
    """Device arrays of recon_analysis against _analysis_ref on the same float64 arrays.  floors: the name of an evaluation case
    whose measured absolute terms (_mask_cases.EVAL_CONDITIONING) apply."""
    from test_gpu_analysis import ARITH, TRANS, _check, assert_same
    B = len(t)
    clean = [b for b in range(B) if b not in empty]
    assert (got["status"] == 0).all() and (want["status"] == 0).all(), what
    if kw.get("find_match", True):
        tied = [b for b in range(B) if (t[b] == 0).all(-1).any()]              # zero target rows: exactly tied relative-polar costs
        if floors is None:
            _check(got, want, t, x, tied, what)
        else:
            _check(got, want, t, x, tied, what, floors={q: C.eval_floors(floors, q, B) for q in
                                                       ("rel_err.1", "rel_err.2", "part_polar", "part_polarrel")})
    else:
        fl = (lambda q: None) if floors is None else (lambda q: C.eval_floors(floors, q, B))          # noqa: E731
        shaped = lambda v, shape: None if v is None else np.reshape(v, shape)                          # noqa: E731
        assert np.array_equal(got["col4row"], want["col4row"]), what
        assert_same(got["rel_err"][0], want["rel_err"][0], ARITH, f"{what} Cartesian")
        for f in (1, 2):
            assert_same(got["rel_err"][f], want["rel_err"][f], TRANS, f"{what} rel_err {f}", shaped(fl(f"rel_err.{f}"), (-1, 1, 1)))
        for k in ("part_polar", "part_polarrel"):
            assert_same(got[k], want[k], TRANS, f"{what} {k}", shaped(fl(k), (1, -1, 1, 1)))
        assert np.array_equal(got["is_padded"], want["is_padded"]) and np.array_equal(got["jet_keep"], want["jet_keep"]), what
        # identity pairing: a row is padded exactly where its target is zero (the reconstruction holds no zero there), in mid-jet too
        assert np.array_equal(got["is_padded"][clean], (t[clean] == 0).all(-1)), f"{what}: rows padded in mid-jet"
    # the all-zero jet: 0/0 is NaN, not +-inf -- no row is padded, the Cartesian residuals are NaN, the jet is not kept
    assert not got["is_padded"][empty].any() and np.isnan(got["rel_err"][0][empty]).all() and not got["jet_keep"][:, empty].any(), what
    assert got["is_padded"][clean].any()
    if not kw.get("abs_coord", True):
        assert np.array_equal(got["part_polarrel"], got["part_polar"], equal_nan=True)


@pytest.mark.parametrize("abs_coord", [True, False])
@pytest.mark.parametrize("find_match", [True, False])
@pytest.mark.parametrize("batch", BATCH_NAMES)
@pytest.mark.parametrize("N", [12, 30, 65])
def test_analysis_on_mask_patterns(N, batch, find_match, abs_coord):
    from test_gpu_analysis import _run
    x, t, _ = C.pair(N, batch)
    x, t = x.numpy(), t.numpy()
    kw = dict(find_match=find_match, abs_coord=abs_coord)
    got, want = _run(t, x, **kw), R.recon_analysis(t, x, **kw)
    empty = C.empty_jets(batch)
    _check_analysis(got, want, t, x, empty, kw, f"{batch} N {N} {kw}")
    clean = C.weighted_jets(batch)
    alone = _run(t[clean], x[clean], **kw)
    for k in ("rel_err", "col4row", "part_polar", "part_polarrel", "jet_cart", "jet_polar", "jet_rel_err", "jet_keep"):
        assert np.array_equal(got[k][:, clean], alone[k], equal_nan=True), k
    assert np.array_equal(got["is_padded"][clean], alone["is_padded"])


# ---- statistics and histograms ------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _holed_analysis(N=30):
    from lgn import analysis as A
    x, t, _ = C.pair(N, "holed")
    out = A.recon_analysis(dev(t.numpy()), dev(x.numpy()))
    return out, {k: v.cpu().numpy() for k, v in out.items()}


def _feats(h):
    return (h["recons"][..., 1:].reshape(-1, 3), h["part_polar"][1].reshape(-1, 3), h["part_polarrel"][1].reshape(-1, 3))


def test_column_stats_on_the_holed_analysis():
    """Residuals over the rows that are not padded and reconstructed features over those that are: a finite column by
    test_gpu_stats.check_column; the Cartesian residuals hold the all-zero jet's NaN among their kept rows -- NONFINITE, NaN
    statistics and edges, the count kept -- and become finite columns once that jet's rows are masked out as well."""
    from lgn import _native as N_
    from lgn import analysis as A
    from test_gpu_stats import check_column
    out, h = _holed_analysis()
    pad = h["is_padded"].reshape(-1)
    seen = set()
    for f in range(3):
        for x, keep_flag in ((h["rel_err"][f].reshape(-1, 3), False), (_feats(h)[f], True)):
            got = {k: v.cpu().numpy() for k, v in A.column_stats(dev(x), dev(pad), keep_flag, 4.0, 81).items()}
            sel = pad == keep_flag
            for c in range(3):
                v = x[sel, c]
                if np.isfinite(v).all():
                    check_column(v, got["stats"][c], int(got["kept"][c]), int(got["status"][c]), got["edges"][c], what=f"frame {f} {keep_flag} {c}")
                else:
                    assert got["status"][c] == N_.STATS_NONFINITE and np.isnan(got["stats"][c]).all() and np.isnan(got["edges"][c]).all()
                    assert got["kept"][c] == sel.sum()
                    seen.add((f, keep_flag))
    assert seen == {(0, False)}, "the Cartesian residuals of the all-zero jet, and nothing else, are not finite"
    N = h["is_padded"].shape[1]
    drop = pad.copy()
    drop.reshape(-1, N)[C.empty_jets("holed")] = True
    x = h["rel_err"][0].reshape(-1, 3)
    got = {k: v.cpu().numpy() for k, v in A.column_stats(dev(x), dev(drop), False, 4.0, 81).items()}
    for c in range(3):
        check_column(x[~drop, c], got["stats"][c], int(got["kept"][c]), int(got["status"][c]), got["edges"][c], what=f"without the jet {c}")


def test_a_whole_column_of_kept_rows_is_not_finite():
    """The two `empty` jets of SPARSE alone: no row is padded, every kept Cartesian residual is NaN."""
    from lgn import _native as N_
    from lgn import analysis as A
    x, t, _ = C.pair(12, "sparse")
    e = C.empty_jets("sparse")
    out = A.recon_analysis(dev(t.numpy()[e]), dev(x.numpy()[e]))
    assert not bool(out["is_padded"].any()) and bool(torch.isnan(out["rel_err"][0]).all()) and int(out["status"].abs().max()) == 0
    cs = A.column_stats(out["rel_err"][0].reshape(-1, 3), out["is_padded"].reshape(-1), False, 4.0, 81)
    assert cs["status"].cpu().tolist() == [N_.STATS_NONFINITE] * 3 and cs["kept"].cpu().tolist() == [24] * 3
    assert bool(torch.isnan(cs["stats"]).all()) and bool(torch.isnan(cs["edges"]).all())
    counts = A.histogram(out["rel_err"][0].reshape(-1, 3), [np.linspace(-2, 2, 81)] * 3, keep=~out["is_padded"].reshape(-1))
    assert int(counts.sum()) == 0, "a NaN lies in no bin"
    got = A.recon_stats(out)
    for c in range(3):
        d = got["particle"]["cartesian"]["rel_err"][c]
        assert all(v is None or v != v for v in d.values()), d
    assert all(got["particle"][f]["pad_recons"] == [] for f in A.FRAMES) and got["jet"] == {"cartesian": [], "polar": []}


def test_particle_histograms_on_the_holed_analysis():
    """Every histogram plot_p draws, against _analysis_ref.histogram (np.histogram's membership rule; a NaN or an infinity lies in no
    bin) on the device's own analysis arrays."""
    from lgn import analysis as A
    out, h = _holed_analysis()
    x, t, _ = C.pair(30, "holed")
    e3 = lambda lo, hi: [np.linspace(lo, hi, 81)] * 3                                                   # noqa: E731
    ranges = {"p_cartesian": e3(-1, 1), "p_polar": [np.linspace(0, 1, 81), np.linspace(-3, 3, 41), np.linspace(-np.pi, np.pi, 81)],
              "rel_err_cartesian": e3(-0.3, 0.3), "rel_err_polar": e3(-0.3, 0.3), "rel_err_polarrel": e3(-0.3, 0.3),
              "padded_cartesian": e3(-4e-3, 4e-3), "padded_polar": e3(-2, 2), "padded_polarrel": e3(-2, 2)}
    got = A.particle_histograms(out, ranges)
    pad = h["is_padded"].reshape(-1)
    want = {}
    for s, p in enumerate((t.numpy(), x.numpy())):
        big = np.linalg.norm(p[..., 1:], axis=-1).reshape(-1) > 1e-6
        want.setdefault("p_cartesian", []).append(R.histogram(p.reshape(-1, 4)[:, 1:], ranges["p_cartesian"], keep=big))
        want.setdefault("p_polar", []).append(R.histogram(h["part_polar"][s].reshape(-1, 3), ranges["p_polar"], keep=big))
    for f, frame in enumerate(A.FRAMES):
        want[f"rel_err_{frame}"] = R.histogram(h["rel_err"][f].reshape(-1, 3), ranges[f"rel_err_{frame}"], keep=~pad)
        want[f"padded_{frame}"] = R.histogram(_feats(h)[f], ranges[f"padded_{frame}"], keep=pad)
    assert set(got) == set(want)
    flat = lambda v: [a for y in v for a in (y if isinstance(y, list) else [y])]                        # noqa: E731
    for k in want:
        assert all(np.array_equal(a, b) for a, b in zip(flat(got[k]), flat(want[k]))), k
    kept = int((~pad).sum())
    nan_rows = 30 * len(C.empty_jets("holed"))
    assert int(sum(want["rel_err_cartesian"][0])) <= kept - nan_rows and sum(a.sum() for a in got["padded_cartesian"]) > 0


def test_recon_stats_on_the_holed_analysis():
    """The err_dict of the holed analysis: the statistics of every finite column by test_gpu_stats.check_dict against
    _stats_ref.get_stats on the same values (FWHM: over the device's own 50 edges, exact where the counts agree); the Cartesian
    residual columns, which hold the all-zero jet's NaN, give None / NaN everywhere; the drawn histograms are np.histogram's over the
    device's edges."""
    from lgn import analysis as A
    from test_gpu_stats import check_dict
    out, h = _holed_analysis()
    got = A.recon_stats(out)
    pad = h["is_padded"].reshape(-1)
    data = {}
    for f, frame in enumerate(A.FRAMES):
        data[f"rel_err_{frame}"] = h["rel_err"][f].reshape(-1, 3)[~pad]
        data[f"padded_{frame}"] = _feats(h)[f][pad]
    source = {"padded_cartesian": "rel_err_cartesian", "rel_err_polarrel": "padded_polarrel"}
    for f, frame in enumerate(A.FRAMES):
        for kind, name in (("rel_err", f"rel_err_{frame}"), ("pad_recons", f"padded_{frame}")):
            x, src = data[name], data[source.get(name, name)]
            dicts = got["particle"][frame][kind]
            assert len(dicts) == 3
            for c in range(3):
                if not np.isfinite(x[:, c]).all():
                    assert name == "rel_err_cartesian" and all(v is None or v != v for v in dicts[c].values()), (name, c, dicts[c])
                    continue
                if not np.isfinite(src[:, c]).all():                      # bins from a NaN median: np.histogram refuses them
                    assert name == "padded_cartesian" and dicts[c]["FWHM"] != dicts[c]["FWHM"]
                    ref = S.get_stats(x[:, c], np.array([0.0, 1.0]))
                    ref["FWHM"] = None
                    d = dict(dicts[c], FWHM=None)
                else:
                    bins = S.edges(src[:, c], 4.0, 50)
                    ref, d = S.get_stats(x[:, c], bins), dicts[c]
                    tol = S.order_tolerances(src[:, c])
                    edge_tol = 4 * S.U * np.abs(bins).max() + tol["median"] + 4 * tol["IQR"]
                ref = {k: (None if v is None else float(v)) for k, v in ref.items()}
                check_dict(d, ref, x[:, c], 4 * edge_tol + 1e-300 if ref["FWHM"] is not None else 0.0, what=f"{name} {c}")
            hist = got["hist"][name]
            edges, counts = hist["edges"].cpu().numpy(), hist["counts"].cpu().numpy()
            for c in range(3):
                if np.isfinite(edges[c]).all():
                    assert np.array_equal(counts[c], R.histogram(x[:, c:c + 1], [edges[c]])[0]), (name, c)
                else:
                    assert name == "rel_err_cartesian" and not counts[c].any()
    for s, system in enumerate(("cartesian", "polar")):
        keep = h["jet_keep"][s]
        assert len(got["jet"][system]) == min(4, keep.sum()) and keep.sum() == len(C.weighted_jets("holed"))


# ---- ROC --------------------------------------------------------------------------------------------------------------------------

def test_roc_of_the_22_scores_with_ties_and_a_nan_column():
    from lgn import _native as N_
    from lgn import anomaly as A
    from test_gpu_roc import check
    x, t, labels = C.roc_inputs()
    xs = [dev(a) for a in _arrs(x, t)]
    scores, st = A.score_tensor(*xs, return_status=True, emd=True)
    out = A.roc_auc_tensor(scores, dev(labels))
    sc = scores.cpu().numpy()
    zero = (sc[:, :21] == 0).all(1)
    assert zero.sum() == 6 and set(labels[zero]) == {1.0, -1.0}, "six all-zero jets tie at 0 across the two classes"
    o = check(out, sc, labels, cols=range(21))
    assert (o["length"][:21] < len(labels) + 1).all(), "tie groups shorten every curve"
    assert np.isnan(sc[zero, 21]).all() and o["status"][21] == N_.ROC_NONFINITE | N_.ROC_NAN and o["length"][21] == 0 and np.isnan(o["auc"][21])
    with pytest.raises(ValueError, match=r"^Input contains NaN\.$"):
        A.get_ROC_AUC({k: sc[:, i] for i, k in enumerate(A.SCORE_KEYS_EMD)}, labels, plot_rocs=False)
    keep = ~zero                                   # without the all-zero jets the EMD column is a curve like the others
    out2 = A.roc_auc_tensor(scores[dev(keep)].contiguous(), dev(labels[keep]))
    check(out2, sc[keep], labels[keep])


# ---- the device's own output: evaluation step -> scores / analysis ----------------------------------------------------------------------

def _eval_recon(case):
    """NativeEvalStep on the case's HOLED jets at live weights, graph-replayed; (target, recon) device tensors, nothing synchronised
    between the step and the caller's next call."""
    from lgn.step import NativeEvalStep
    from test_gpu_mask_patterns import _jets, _nets
    p4, labels = _jets(case)
    enc, dec, _, _ = _nets(case, DEV)
    ev = NativeEvalStep(enc, dec, p4.shape[0], get_real_method="sum", use_graph=True)
    batch = {"p4": p4.to(DEV), "labels": labels.to(DEV)}
    for _ in range(2):
        out = ev.run(batch)
    return batch["p4"], out["recon"], labels


@pytest.mark.parametrize("which", [0, 1], ids=["maxdim2_n30", "maxdim3_n13"])
def test_scores_and_analysis_after_the_eval_step(which):
    """A Lorentz-equivariant network maps a one-particle jet to multiples of that particle: every reconstructed particle of the
    `one_last` jet is collinear with its target, in exact arithmetic its EMD is 0 and its matched (eta, phi) residuals and relative
    coordinates are 0.  What the device and the restatement return there is the rounding of O(1) operands, which no relative
    tolerance holds -- the restatement misses its own against itself (particles reversed; np.longdouble).  Those (quantity, jet)
    pairs, and no others, carry 100 x the figure measured on the CPU as an absolute term (_mask_cases.EVAL_CONDITIONING, asserted by
    tests/test_host_mask_cases.py) through the `floors` argument of test_gpu_analysis._check; no device value is replaced, and every
    other jet is held to the files' tolerances alone.  The rel_err.2 terms (44 and 170) mean that the relative-polar residual of
    that jet's one real row is in effect NOT compared: it is a rounding residue over 1e-16, without a correct digit on either side."""
    from lgn import analysis as AN
    from lgn import anomaly as A
    from test_gpu_mask_patterns import EVAL_CASES
    case = EVAL_CASES[which]
    target, recon, labels = _eval_recon(case)
    B, N = labels.shape
    col = torch.full((6, B, N), -7, device=DEV, dtype=torch.int32)
    xs = [recon, target, C.normalized(recon), C.normalized(target)]
    sc, st = A.score_tensor(*xs, return_status=True, col4row=col, emd=True)          # chained: no sync since the step
    outs = {(fm, ac): AN.recon_analysis(target, recon, find_match=fm, abs_coord=ac) for fm in (True, False) for ac in (True, False)}
    torch.cuda.synchronize()
    empty = (labels.sum(1) == 0).nonzero().flatten().tolist()
    x, t = recon.cpu(), target.cpu()
    assert empty and bool((x[empty] == 0).all()) and not bool(torch.signbit(x[empty]).any()), "the decoder returns +0 for an all-masked jet"
    masked = ~labels.bool()
    masked[empty] = False
    assert bool((x[masked] != 0).any(-1).all()), "and no zero row elsewhere"
    arrs = _arrs(x, t)
    _check_scores(arrs, sc, st, col, empty, case.what, floors=C.EVAL_NAMES[which])
    for (fm, ac), out in outs.items():
        kw = dict(find_match=fm, abs_coord=ac)
        got = {k: v.cpu().numpy() for k, v in out.items()}
        _check_analysis(got, R.recon_analysis(arrs[1], arrs[0], **kw), arrs[1], arrs[0], empty, kw, f"{case.what} {kw}", floors=C.EVAL_NAMES[which])


def test_the_chain_replays_from_one_graph():
    """Evaluation step -> 22 scores -> ROC and evaluation step -> analysis -> histogram captured into one graph after the step (the
    step replays its own), replayed on a second HOLED batch and compared bit for bit with the eager calls on that batch."""
    from lgn import analysis as AN
    from lgn import anomaly as A
    from lgn.step import NativeEvalStep
    from test_gpu_mask_patterns import EVAL_CASES, _nets
    import _jets as J
    case = EVAL_CASES[0]
    enc, dec, _, _ = _nets(case, DEV)
    batches = [J.pattern_jets(case.N, J.HOLED, s) for s in (11, 12)]
    K = len(J.HOLED)
    ev = NativeEvalStep(enc, dec, K, get_real_method="sum", use_graph=True)
    roc_labels = dev(np.where(np.arange(K) % 2 == 0, 1.0, -1.0))
    edges = AN.pack_edges([np.linspace(-0.5, 0.5, 82), np.linspace(-1, 1, 11), np.linspace(-3, 3, 1025)])
    target, recon = torch.zeros(K, case.N, 4, device=DEV, dtype=torch.float64), torch.zeros(K, case.N, 4, device=DEV, dtype=torch.float64)

    def chain():
        scores = A.score_tensor(recon, target, C.normalized(recon), C.normalized(target), emd=True)
        roc = A.roc_auc_tensor(scores, roc_labels)
        an = AN.recon_analysis(target, recon)
        hist = AN.histogram(an["rel_err"][1].view(-1, 3), edges, keep=~an["is_padded"].view(-1))
        return scores, roc, an, hist

    def load(b):
        p4, labels = batches[b]
        out = ev.run({"p4": p4.to(DEV), "labels": labels.to(DEV)})
        target.copy_(p4.to(DEV)), recon.copy_(out["recon"])

    load(0)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        chain()                                    # warm-up outside the capture
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            scores, roc, an, hist = chain()
    torch.cuda.current_stream().wait_stream(side)
    load(1)
    graph.replay()
    torch.cuda.synchronize()
    e_scores, e_roc, e_an, e_hist = chain()
    torch.cuda.synchronize()
    assert np.array_equal(scores.cpu().numpy(), e_scores.cpu().numpy(), equal_nan=True) and bool(torch.isnan(scores[:, 21]).sum() == 1)
    for k in ("length", "flipped", "status", "auc", "fpr", "tpr", "thresholds"):
        n = roc["length"].cpu().tolist()
        for c in range(22):                        # (entries past a curve's length are not defined)
            assert np.array_equal(roc[k][c].cpu().numpy()[..., :n[c]] if roc[k].dim() == 2 else roc[k][c].cpu().numpy(),
                                  e_roc[k][c].cpu().numpy()[..., :n[c]] if roc[k].dim() == 2 else e_roc[k][c].cpu().numpy(), equal_nan=True), (k, c)
    for k in e_an:
        assert np.array_equal(an[k].cpu().numpy(), e_an[k].cpu().numpy(), equal_nan=True), k
    from lgn import _native as N_
    assert torch.equal(hist, e_hist) and int(hist.sum()) > 0
    assert roc["status"].cpu().tolist() == [0] * 21 + [N_.ROC_NONFINITE | N_.ROC_NAN], "the NaN column goes through the replay too"
