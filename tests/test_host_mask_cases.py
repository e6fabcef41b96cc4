"""CPU tests of tests/_mask_cases.py: every decision that makes a case of tests/test_gpu_loss_mask_patterns.py and
tests/test_gpu_postproc_mask_patterns.py usable is taken on the restatements alone and asserted here, so that it holds on a machine
without a GPU; and the "would catch" figures those files quote are measured here with deliberately wrong restatements."""
import numpy as np
import pytest
import torch

import _analysis_ref as R
import _anomaly_ref as A
import _emd_opts_grad_ref as GO
import _emd_pairs_ref as P
import _emd_ref as E
import _hungarian_ref as H
import _mask_cases as C
import _sinkhorn_ref as S

BATCH_NAMES = ["sparse", "holed", "disagree"]


@pytest.mark.parametrize("batch", BATCH_NAMES)
@pytest.mark.parametrize("N", [12, 30, 63, 64])
def test_the_recorded_seeds_give_nondegenerate_optima(N, batch):
    """Target events against reconstruction events, default options and the set "all": every jet of lp_jets passes; the one jet
    lp_jets leaves out (`disagree` jet 1, two identical target rows) fails under the default options, as it must."""
    p, q = C.events(N, batch, C.EMD_SEEDS[(N, batch)])
    for o in ({}, C.EMD_ALL):
        for b in C.lp_jets(batch):
            assert C.nondegenerate(q[b], p[b], o), (N, batch, b, o)
    assert set(C.weighted_jets(batch)) - set(C.lp_jets(batch)) == ({1} if batch == "disagree" else set())
    if batch == "disagree":                        # two identical target rows: degenerate under both option sets, at other seeds too
        for seed in (C.EMD_SEEDS[(N, batch)], 12, 13):
            ps, qs = C.events(N, batch, seed)
            assert not C.nondegenerate(qs[1], ps[1], {}) and not C.nondegenerate(qs[1], ps[1], C.EMD_ALL), seed


@pytest.mark.parametrize("batch", BATCH_NAMES)
def test_only_the_empty_jets_are_flagged(batch):
    """What the restatements give for the all-zero jet, and that they flag no other: assignment losses 0 with gradient 0 in every
    frame, 21 scores 0 and finite, EMD and Sinkhorn NaN / EMPTY, the analysis status 0 with no row padded (0/0 is NaN, not inf)."""
    N = 12
    x, t, labels = C.pair(N, batch)
    empty, clean = C.empty_jets(batch), C.weighted_jets(batch)
    assert empty and bool((x[empty] == 0).all()) and bool((t[empty] == 0).all()) and bool((x[clean] != 0).all())
    for a, p in H.FRAMES.values():
        xr = x.clone().requires_grad_(True)
        per = H.per_jet(xr, t, H.assignment(x, t, a, p), a, p)
        per.sum().backward()
        assert bool((per[empty] == 0).all()) and bool((xr.grad[empty] == 0).all()) and bool((per[clean] > 0).all())
        assert bool(np.isfinite(xr.grad.numpy()).all())
    arrs = [z.numpy() for z in (x, t, C.normalized(x), C.normalized(t))]
    sc, _ = A.anomaly_scores(*arrs)
    assert np.isfinite(sc).all() and (sc[empty] == 0).all()
    p, q = E.relative_events(arrs[0]), E.relative_events(arrs[1])
    for o in ({}, C.EMD_ALL):
        flagged = [b for b in range(len(p)) if np.isnan(P.emd(q[b], p[b], **o))]
        assert flagged == empty
    st = [S.sinkhorn(q[b], p[b], 0.1, max_iter=3, tol=0.0, debias=True)["status"] for b in range(len(p))]
    assert [b for b, s in enumerate(st) if s] == empty
    for fm in (True, False):
        out = R.recon_analysis(arrs[1], arrs[0], find_match=fm)
        assert (out["status"] == 0).all() and not out["is_padded"][empty].any() and np.isnan(out["rel_err"][0][empty]).all()
        assert not out["jet_keep"][:, empty].any()
    # identity pairing: the +-inf rule flags exactly the rows whose target is zero, in mid-jet too (the reconstruction has no zero)
    want = (t[clean] == 0).all(-1).numpy()
    assert np.array_equal(out["is_padded"][clean], want) and want.any()
    if batch != "disagree":
        assert np.array_equal(want, ~labels[clean].bool().numpy())


def test_a_target_multiplied_by_the_labels_moves_the_disagreeing_jet():
    """(i): on `disagree` jet 0 the target carries momenta on masked rows.  A loss stage that applied the labels to its target would
    move that jet's term by 0.7 .. 1.0 of itself -- ten orders above the 1e-10 the terms are held to."""
    x, t, labels = C.pair(12, "disagree")
    tl = t * labels.unsqueeze(-1).double()
    moved = {"mse": float((H.mse_per_jet(x, t) - H.mse_per_jet(x, tl)).abs()[0] / H.mse_per_jet(x, t)[0])}
    for f, (a, p) in H.FRAMES.items():
        r, w = (H.per_jet(x, y, H.assignment(x, y, a, p), a, p) for y in (t, tl))
        moved[f] = float((r - w).abs()[0] / r[0])
    p, q, qw = (E.relative_events(z.numpy()) for z in (x, t, tl))
    for name, o in (("emd", {}), ("emd all", C.EMD_ALL)):
        moved[name] = abs(P.emd(q[0], p[0], **o) - P.emd(qw[0], p[0], **o)) / P.emd(q[0], p[0], **o)
    kw = dict(max_iter=6, tol=0.0, debias=True)
    r, w = (S.sinkhorn_relative(x.numpy()[0], y.numpy()[0], 1.0, **kw)["value"] for y in (t, tl))
    moved["sinkhorn"] = abs(r - w) / abs(r)
    print("(i) jet 0 moves by", {k: f"{v:.2f}" for k, v in moved.items()})
    assert all(v > 0.5 for v in moved.values()), moved


@pytest.mark.parametrize("N", [12, 30, 64])
def test_compacted_weightless_particles_move_the_gradients_not_the_value(N):
    """(ii): the target's weightless particles moved behind the weighted ones and the results left in that order.  The value does not
    move (1e-14); the position gradients of every jet whose holes are not a suffix move by 0.4 or more of their largest entry, the
    Sinkhorn gradients likewise -- so the tests compare gradients, flow and potentials per particle."""
    p, q = C.events(N, "holed", C.EMD_SEEDS[(N, "holed")])
    qc = C.compact(q)
    names = C.BATCHES["holed"]
    for b in C.weighted_jets("holed"):
        prefix = names[b] in ("prefix_minus_one", "full")
        for o in ({}, C.EMD_ALL):
            v, g0, _ = GO.emd_grad(q[b], p[b], **o)
            vc, c0, _ = GO.emd_grad(qc[b], p[b], **o)
            assert abs(v - vc) <= 1e-13 * abs(v)
            moved = np.abs(g0 - c0)[:, 1:].max() / np.abs(g0[:, 1:]).max()
            assert (moved == 0) if prefix else (moved > 0.4), (N, names[b], o, moved)
    kw = dict(max_iter=25, tol=0.0, debias=True)
    for b in (0, 1, 2):                                                  # odd, mod4, block_hole
        r, w = S.sinkhorn(q[b], p[b], 0.1, **kw), S.sinkhorn(qc[b], p[b], 0.1, **kw)
        assert abs(r["value"] - w["value"]) <= 1e-13 * abs(r["value"])
        assert np.abs(r["g0"] - w["g0"]).max() > 0.2 * np.abs(r["g0"]).max()


@pytest.mark.parametrize("batch", BATCH_NAMES)
@pytest.mark.parametrize("N", [12, 30])
def test_the_sinkhorn_conditioning_table_is_what_the_restatement_measures(N, batch):
    """The restatement against itself with a jet's particles reversed keeps the rule's bound on every gradient but the listed ones;
    a listed figure is the measured one (to 2 %)."""
    for key, (bound, self_) in C.sinkhorn_relative_self(batch, N).items():
        if key in C.SINKHORN_CONDITIONING:
            assert self_ > bound and abs(self_ - C.SINKHORN_CONDITIONING[key]) <= 0.02 * self_, (key, bound, self_)
        else:
            assert self_ <= bound, (key, bound, self_)
    assert all(k[0] in BATCH_NAMES and k[1] in (12, 30) for k in C.SINKHORN_CONDITIONING)


def test_the_roc_batches_keep_every_auc_off_one_half():
    """36 jets, 22 signal; six all-zero jets of both classes tie at 0 in the 21 scores and are NaN in the EMD column; with and
    without them no column's AUC (before the flip) is within 1e-6 of 0.5."""
    import _roc_ref as ROC
    x, t, labels = C.roc_inputs()
    arrs = [z.numpy() for z in (x, t, C.normalized(x), C.normalized(t))]
    sc, _ = A.anomaly_scores(*arrs)
    zero = (sc == 0).all(1)
    assert len(labels) == 36 and zero.sum() == 6 and set(labels[zero]) == {1.0, -1.0} and bool((x[zero] == 0).all())
    emd = E.emd_relative(arrs[0], arrs[1])
    assert np.array_equal(np.isnan(emd), zero)
    for keep, cols in ((np.ones(36, bool), sc), (~zero, np.concatenate([sc, emd[:, None]], 1)[~zero])):
        for k in range(cols.shape[1]):
            fpr, tpr, _ = ROC.roc_curve(labels[keep], cols[:, k])
            assert abs(ROC.auc(fpr, tpr) - 0.5) >= 1e-6, (k, ROC.auc(fpr, tpr))
            assert len(fpr) < keep.sum() + 1 or not zero[keep].any()


@pytest.mark.parametrize("N", [12, 30, 65])
def test_padding_taken_from_a_zero_target_moves_the_all_zero_jet(N):
    """(iii): is_padded from `target == 0` instead of the +-inf rule agrees on every jet but the all-zero one, whose N rows it flags
    (the restatement: 0/0 is NaN, none is padded).  That moves the kept rows of the residual histograms and statistics by N NaN
    entries and the padded-particle histograms by N zeros: counts are compared exactly, so one row is enough."""
    x, t, _ = C.pair(N, "holed")
    out = R.recon_analysis(t.numpy(), x.numpy(), find_match=False)
    wrong = (t == 0).all(-1).numpy()
    differ = (out["is_padded"] != wrong).sum(-1)
    assert differ.tolist() == [N if b in C.empty_jets("holed") else 0 for b in range(len(x))]


@pytest.mark.parametrize("name,method", C.STEP_RUNS)
def test_the_step_cases_are_live_under_every_assignment_loss(name, method):
    """U.assert_live on the oracle with each restated loss (scored on the restatement's own assignment): the condition that makes a
    step case usable, decided without a GPU.  An all-masked jet's reconstruction is exactly zero and, with get_real 'real', so is
    its term ('norm' takes sqrt(re^2 + im^2 + 1e-16): 1e-8 per component, and the restatement's term of that)."""
    p4, labels = C.step_forward(name)[:2]
    empty = (labels.sum(1) == 0).nonzero().flatten().tolist()
    for loss in [("mse", True, False)] + [("hungarian",) + H.FRAMES[f] for f in H.FRAMES]:
        terms, grads, floor, x_o = C.step_reference(name, loss, method)
        assert empty and bool((C.step_forward(name)[4].detach()[:, empty] == 0).all())
        if method == "real":
            assert bool((x_o[empty] == 0).all()) and bool((terms[empty] == 0).all()) and int((terms > 0).sum()) == len(p4) - len(empty)


# ---- the comparator first: the restatement against the reference on these inputs (fixture g29) ---------------------------------------
def test_g29_inputs_are_this_modules_recipe():
    """The fixture's generator restates pattern_jets with the reference's normalize_p4; the stored target is what tests/_jets.py gives
    (HOLED, then its disagreeing copy), the stored reconstruction is recon_like of the stored target."""
    import _jets as J
    import _util as U
    z = U.load("g29_loss_masks.npz")
    m = U.meta(z)
    p4, labels = J.pattern_jets(m["N"], J.HOLED, m["seed"])
    q4, q_labels = J.disagree(p4, labels, torch.Generator().manual_seed(m["seed"] + 1))
    t, lab = torch.from_numpy(z["t"]), torch.from_numpy(z["labels"])
    assert torch.equal(lab, torch.cat([labels, q_labels])) and tuple(t.shape) == (22, 12, 4)
    np.testing.assert_allclose(z["t"], torch.cat([p4, q4]).numpy(), rtol=1e-14, atol=0)
    assert torch.equal(torch.from_numpy(z["x"]), J.recon_like(t, lab, torch.Generator().manual_seed(m["seed"] + 2)))
    assert bool((t[[7, 18]] == 0).all()) and bool((torch.from_numpy(z["x"])[[7, 18]] == 0).all()), "the two all-zero jets"


@pytest.mark.parametrize("frame", list(H.FRAMES))
def test_hungarian_restatement_matches_the_reference_on_holed_jets(frame):
    """g29: the reference's HungarianMSELoss on HOLED + `disagree` at N = 12.  The zero target rows tie, so the reference (torch.cdist)
    and the restatement (exact costs) may hold different optima: the restatement's assignment is always an optimum (total cost equal to
    1e-12 per jet); the loss and the gradient scored on the REFERENCE's assignment are the reference's to 1e-12 (the tolerances of
    tests/test_host_hungarian_loss.py on g19); the per-jet terms agree wherever the same optimum was found."""
    import _util as U
    z = U.load("g29_loss_masks.npz")
    a, p = H.FRAMES[frame]
    x, t = torch.from_numpy(z["x"]), torch.from_numpy(z["t"])
    col_ref = torch.from_numpy(z[f"col.{frame}"].astype(np.int64))
    col = H.assignment(x, t, a, p)
    same = (col == col_ref).all(-1)
    print(f"g29 {frame}: the restatement's assignment is the reference's on {int(same.sum())} of {len(same)} jets")
    np.testing.assert_allclose(H.total_cost(x, t, col, a, p).numpy(), H.total_cost(x, t, col_ref, a, p).numpy(), rtol=1e-12, atol=0)
    xx = x.clone().requires_grad_(True)
    loss = H.loss(xx, t, col_ref, a, p)
    loss.backward()
    np.testing.assert_allclose(loss.item(), float(z[f"loss.{frame}"]), rtol=1e-12)
    g_ref = torch.from_numpy(z[f"grad.{frame}"])
    assert (xx.grad - g_ref).abs().max().item() <= 1e-12 * g_ref.abs().max().item()
    per_a, per_b = H.per_jet(x, t, col, a, p), H.per_jet(x, t, col_ref, a, p)
    np.testing.assert_allclose(per_a[same].numpy(), per_b[same].numpy(), rtol=1e-12, atol=0)
    assert bool(same.any()) and bool((per_b[[7, 18]] == 0).all()), "zero against zero is 0 in the reference's pairing too"


def test_anomaly_restatement_matches_the_reference_on_holed_jets():
    """g29: the reference's anomaly_scores on HOLED + `disagree` at N = 12, every jet kept.  The 15 scores without an assignment at the
    tolerances of tests/test_host_anomaly.py (1e-12, the polar frames 1e-11).  The six Hungarian variants: the restatement's
    assignment is always an optimum of the exact costs (total cost equal to that of scipy's on the reference's cost matrix, 1e-12),
    and its score is the reference's wherever the same optimum was found.  The two all-zero jets score 0 in the reference too."""
    import _util as U
    z = U.load("g29_loss_masks.npz")
    arrs = [z["x"], z["t"], z["an.recons_n"], z["an.target_n"]]
    np.testing.assert_array_equal(arrs[2], C.normalized(torch.from_numpy(arrs[0])).numpy())
    want, wcol = A.anomaly_scores(*arrs)
    ref, col_ref = z["an.scores"], z["an.col"].astype(np.int64)
    polar = (1, 3, 4, 6, 8, 9, 11, 13, 14)
    assert np.isfinite(ref).all() and (ref[[7, 18]] == 0).all() and (want[[7, 18]] == 0).all()
    for s in range(21):
        if s not in A.HUNGARIAN_INDEX:
            np.testing.assert_allclose(want[:, s], ref[:, s], rtol=1e-11 if s in polar else 1e-12, atol=0, err_msg=A.SCORE_KEYS[s])
    found = 0
    for f, (p, q, lor) in enumerate(A.frames(*arrs)):
        c = A.costs(p, q, lor)
        rows = np.arange(c.shape[1])
        s = A.HUNGARIAN_INDEX[f]
        for b in range(len(c)):
            tot, best = c[b, rows, wcol[f, b]].sum(), c[b, rows, col_ref[f, b]].sum()
            assert abs(tot - best) <= 1e-12 * abs(best), (f, b, tot, best)
            if np.array_equal(wcol[f, b], col_ref[f, b]):
                found += 1
                np.testing.assert_allclose(want[b, s], ref[b, s], rtol=1e-11 if s in polar else 1e-12, atol=0, err_msg=f"{A.SCORE_KEYS[s]} jet {b}")
    print(f"g29 anomaly: the same optimum on {found} of {6 * len(ref)} (variant, jet) pairs")
    assert found >= 0.5 * 6 * len(ref)


def test_analysis_restatement_matches_the_reference_on_holed_jets():
    """g29: the reference's get_rel_err_find_match route on the same jets, at the tolerances of tests/test_host_analysis.py.  Rows
    padded in mid-jet are +-inf in the reference, the all-zero jets' rows are NaN (0/0) and NOT padded; the restatement has both.
    Where the tied zero rows let the two sides hold different optima the residuals of that (frame, jet) are compared by
    assert_tied_assignment's rule instead: the restatement's assignment has the reference's total cost."""
    import _util as U
    z = U.load("g29_loss_masks.npz")
    t, x = z["t"], z["x"]
    want = R.recon_analysis(t, x)
    ref = {k[3:]: z[k] for k in z.files if k.startswith("ra.")}
    col_ref = ref["col"].astype(np.int64)
    assert (want["status"] == 0).all()
    assert np.array_equal(want["is_padded"], ref["is_padded"]) and np.array_equal(want["jet_keep"], ref["jet_keep"])
    assert not ref["is_padded"][[7, 18]].any() and np.isnan(ref["rel_err"][0][[7, 18]]).all(), "0/0: NaN, not padded, in the reference"
    clean = [b for b in range(22) if b not in (7, 18)]
    assert np.array_equal(ref["is_padded"][clean], (t[clean] == 0).all(-1)), "mid-jet padded rows are flagged by the +-inf rule"
    R.assert_same(want["part_polar"], ref["part_polar"], 1e-12, "part_polar")
    R.assert_same(want["part_polarrel"], ref["part_polarrel"], 1e-11, "part_polarrel")
    for k in ("jet_cart", "jet_polar"):
        R.assert_same(want[k][..., 1:], ref[k][..., 1:], 1e-12, k)
    R.assert_same(want["jet_rel_err"][:, :, 1:], ref["jet_rel_err"][:, :, 1:], 1e-12, "jet_rel_err")
    same = [(want["col4row"][k] == col_ref[k]).all(-1) for k in (0, 1)]
    for k, frames_ in ((0, (0, 1)), (1, (2,))):
        cost = R.cost3(t[..., 1:], x[..., 1:]) if k == 0 else R.cost3(ref["part_polarrel"][0], ref["part_polarrel"][1])
        rows = np.arange(12)
        for b in range(22):
            tot, best = cost[b, rows, want["col4row"][k, b]].sum(), cost[b, rows, col_ref[k, b]].sum()
            assert abs(tot - best) <= 1e-12 * abs(best), (k, b, tot, best)
        for f in frames_:
            R.assert_same(want["rel_err"][f][same[k]], ref["rel_err"][f][same[k]], 1e-11 if f == 2 else 1e-12, f"rel_err frame {f}")
    print(f"g29 analysis: the same optimum on {int(same[0].sum())} / {int(same[1].sum())} of 22 jets (Cartesian / relative polar)")
    assert same[0][[6, 17]].all() and same[1][[6, 17]].all(), "the `full` jets have no tied rows: one optimum"


@pytest.mark.parametrize("name", C.EVAL_NAMES)
def test_the_eval_conditioning_table_is_what_the_restatements_measure(name):
    """Every (quantity, jet) on which the restatement misses its own relative tolerance against itself (particles reversed, or the
    formulas in np.longdouble) is listed, with the measured figure (listed >= measured >= 0.8 listed); nothing else is listed; and
    every listed entry lies on the one-particle jet `one_last`, whose reconstruction the network makes collinear with its target."""
    import _jets as J
    measured = C.eval_self_disagreement(name)
    listed = {(q, j): f for (n, q, j), f in C.EVAL_CONDITIONING.items() if n == name}
    assert set(measured) == set(listed), (sorted(measured), sorted(listed))
    for key, (fig, count) in measured.items():
        assert 0.8 * listed[key] <= fig <= listed[key], (key, fig, listed[key])
        assert J.HOLED[key[1]] == "one_last" and count <= 60
    assert len(C.EVAL_CONDITIONING) == 6


@pytest.mark.parametrize("name", C.CHAMFER_RUNS)
def test_the_step_cases_are_live_under_chamfer_with_the_jet_term(name):
    loss, grads, floor = C.chamfer_jet_reference(name)
    assert bool(torch.isfinite(loss)) and float(loss) > 0 and floor <= 10


@pytest.mark.parametrize("name", C.NORMALIZE_RUNS)
def test_the_normalize_case_is_live_and_brings_the_raw_jets_back(name):
    """--normalize overall_max on HOLED scaled per jet: every weighted jet comes back with its largest component 1, the all-masked
    jet stays exactly zero (and so does its reconstruction), the holes stay where they are, and the oracle on it is live."""
    N = C.step_cases()[name].N
    raw, labels = C.raw_holed(N)
    p4, loss, rec, grads, floor = C.normalize_reference(name)
    top = p4.abs().flatten(1).amax(1)
    assert float(raw.abs().max()) > 100 and bool(((top - 1).abs()[C.weighted_jets("holed")] <= 2.0 ** -52).all())
    assert bool((p4[7] == 0).all()) and bool((rec[:, 7] == 0).all()) and torch.equal(p4[..., 0] != 0, labels.bool())


@pytest.mark.parametrize("name", sorted(set(C.SINKHORN_STEP_RUNS) | {n for n, _ in C.EMD_STEP_RUNS}))
def test_what_the_transport_loss_stages_of_the_step_cases_see(name):
    """On the oracle's reconstruction (live by U.assert_live), for the EMD, hybrid and Sinkhorn stages: the all-masked jets and no
    others are EMPTY; every one-particle jet is reconstructed as multiples of its particle (its reconstructed particles sit at no
    more than two positions: along it, against it); and the weighted jets whose optimum is degenerate by the rule of
    test_gpu_emd_step._assert_nondegenerate are exactly those of _mask_cases.EMD_DEGENERATE -- at least one in every case but
    maxdim 3 under "all", which is the one EMD case held to the oracle."""
    p, q, labels = C.step_events(name)
    n_real = labels.sum(1).tolist()
    empty = [b for b, n in enumerate(n_real) if n == 0]
    assert empty and [b for b in range(len(p)) if np.isnan(P.emd(q[b], p[b]))] == empty
    assert [b for b in range(len(p)) if S.sinkhorn(q[b], p[b], 0.05, max_iter=2, tol=0.0)["status"]] == empty
    single = [b for b, n in enumerate(n_real) if n == 1]
    assert single, "every batch holds a one-particle jet"
    for b in single:
        assert len(np.unique(np.round(p[b][:, 1:], 9), axis=0)) <= 2 and float(np.abs(q[b][labels[b].bool().numpy()][:, 1:]).max()) <= 1e-12
    for key, o in (("default", {}), ("all", C.EMD_ALL)):
        found = [b for b in range(len(p)) if b not in empty and not C.nondegenerate(q[b], p[b], o)]
        assert found == C.EMD_DEGENERATE[(name, key)], (name, key, found)
        assert set(single) <= set(found) or (name, key) == ("md3_n13_holed", "all")
