"""The (reconstruction, target) pairs of the loss-stage and post-processing mask-pattern tests (tests/test_gpu_loss_mask_patterns.py,
tests/test_gpu_postproc_mask_patterns.py) and the CPU-side decisions about them (tests/test_host_mask_cases.py asserts every one, so
that they hold on a machine without a GPU): targets _jets.pattern_jets / disagree, reconstructions _jets.recon_like.  Not a test
module."""
import functools

import numpy as np
import torch

import _emd_ref as E
import _jets as J

BATCHES = {"sparse": J.SPARSE, "holed": J.HOLED, "disagree": J.HOLED}
JET_SEED = 11

# (N, batch) -> the seed of pattern_jets for the EMD cases: the first seed from JET_SEED on at which the optimum of every jet of
# lp_jets(batch) is non-degenerate by the rule of test_gpu_emd_step._assert_nondegenerate (nondegenerate() below), under the default
# options and under EMD_ALL; searched on the CPU (the first seed passed at every size), tests/test_host_mask_cases.py asserts each
EMD_SEEDS = {(N, batch): 11 for N in (12, 30, 63, 64) for batch in ("sparse", "holed", "disagree")}
EMD_ALL = dict(R=0.8, beta=2.0, norm=True, periodic_phi=True)


@functools.lru_cache(maxsize=None)
def pair(N, batch, seed=JET_SEED):
    """(x, t, labels): reconstruction and target (B, N, 4) float64 and the labels (B, N) uint8 of a named batch; never modified."""
    t, labels = J.pattern_jets(N, BATCHES[batch], seed)
    if batch == "disagree":
        t, labels = J.disagree(t, labels, torch.Generator().manual_seed(seed + 1))
    x = J.recon_like(t, labels, torch.Generator().manual_seed(seed + 2))
    return x, t, labels


def empty_jets(batch):
    """The jets for which a restatement may set a status or return NaN: pattern `empty` and nothing else."""
    return [b for b, n in enumerate(BATCHES[batch]) if n == "empty"]


def weighted_jets(batch):
    return [b for b, n in enumerate(BATCHES[batch]) if n != "empty"]


def lp_jets(batch):
    """The jets whose EMD gradient is compared with scipy's LP: the weighted ones, but for `disagree`'s jet 1 -- two identical target
    rows are two identical columns of the transport problem, a degenerate optimum at every seed and under every option set
    (tests/test_host_mask_cases.py asserts it at three seeds).  Of that jet the gradient with respect to the RECONSTRUCTION's
    positions is still compared with the LP -- the two rows sit at one position, so it is the same at every optimum -- and the
    whole jet is held to the certificate and to the header's formulas on the returned flow, which hold at any optimum."""
    return [b for b in weighted_jets(batch) if not (batch == "disagree" and b == 1)]


def normalized(x):
    """x / (max |x| over the jet's particles + 1e-16) per component: the scores' normalised inputs, as the existing tests build them."""
    return x / (x.abs().amax(-2, keepdim=True) + 1e-16)


def events(N, batch, seed=JET_SEED):
    """(p, q) numpy (B, N, 3): the relative-polar events (pT, y, phi) of the reconstruction and of the target (E.relative_events)."""
    x, t, _ = pair(N, batch, seed)
    return E.relative_events(x.numpy()), E.relative_events(t.numpy())


# seeds of the ROC batches: signal = HOLED at both seeds, background = SPARSE at both (36 jets, six of them all-zero: they tie at
# score 0 across the two classes).  tests/test_host_mask_cases.py asserts that every column's AUC keeps 1e-6 from 0.5 on the
# restatement's scores, with and without the all-zero jets, so that no flip hinges on the last bit of a sum
ROC_SEEDS = (11, 21)
ROC_N = 12


def roc_inputs():
    """(x, t (36, N, 4) tensors, labels (36,) numpy of +-1)"""
    pairs = [pair(ROC_N, "holed", s) for s in ROC_SEEDS] + [pair(ROC_N, "sparse", s) for s in ROC_SEEDS]
    x, t = torch.cat([p[0] for p in pairs]), torch.cat([p[1] for p in pairs])
    n_sig = len(ROC_SEEDS) * len(J.HOLED)
    return x, t, np.array([1.0] * n_sig + [-1.0] * (len(x) - n_sig))


# {(batch, N, jet, gradient): max |restatement - restatement with the jet's particles reversed|} of _sinkhorn_ref.sinkhorn_relative
# (epsilon 1, 6 iterations, debias) where that exceeds the rule 64 x spread + 8 (2 N + 2) 2^-53 max |g| the gradients are held to
SINKHORN_CONDITIONING = {("sparse", 12, 1, "g_target"): 8.98e-14}
SINKHORN_REL = dict(epsilon=1.0, kw=dict(max_iter=6, tol=0.0, debias=True))


def sinkhorn_relative_self(batch, N):
    """{(batch, N, jet, gradient): (the rule's bound, the restatement against itself reversed)} of every weighted jet."""
    import _sinkhorn_ref as S
    x, t, _ = pair(N, batch)
    x, t = x.numpy(), t.numpy()
    eps, kw = SINKHORN_REL["epsilon"], SINKHORN_REL["kw"]
    out = {}
    for i in weighted_jets(batch):
        r0, r1 = (S.sinkhorn_relative(x[i], t[i], eps, variant=v, **kw) for v in (0, 1))
        rr = S.sinkhorn_relative(x[i][::-1].copy(), t[i][::-1].copy(), eps, variant=0, **kw)
        for key in ("g_recons", "g_target"):
            bound = 64 * np.abs(r0[key] - r1[key]).max() + 8 * (2 * N + 2) * 2.0 ** -53 * np.abs(r0[key]).max()
            out[(batch, N, i, key)] = (bound, np.abs(rr[key][::-1] - r0[key]).max())
    return out


def nondegenerate(p, q, opts):
    """The rule of test_gpu_emd_step._assert_nondegenerate on one pair of events, as a bool: the arcs among weighted particles whose
    reduced cost is below 1e-6 x the largest cost number exactly (weighted rows + weighted columns - 1), and each carries flow above
    1e-9 x the total weight."""
    import _emd_opts_grad_ref as GO
    import _emd_pairs_ref as P
    _, flow, u, v = GO.solve(p, q, **opts)
    c, a, d = P.balanced(p, q, opts.get("R", 1.0), opts.get("beta", 1.0), opts.get("norm", False), opts.get("periodic_phi", False))
    ri, ci = np.flatnonzero(a > 0), np.flatnonzero(d > 0)
    sel = np.ix_(ri, ci)
    tight = (c - u[:, None] - v[None, :])[sel] < 1e-6 * c[sel].max()
    return bool(tight.sum() == len(ri) + len(ci) - 1 and (flow[sel][tight] > 1e-9 * max(a.sum(), d.sum())).all())


def compact(ev):
    """The deliberately wrong staging (ii): every event's weightless particles moved behind its weighted ones, order kept."""
    out = np.zeros_like(ev)
    for b in range(len(ev)):
        w = ev[b, :, 0] > 0
        out[b] = np.concatenate([ev[b][w], ev[b][~w]])
    return out


# ---- the loss stages inside the steps -------------------------------------------------------------------------------------------
def step_cases():
    """The networks and batches of the step cases: those of tests/test_gpu_mask_patterns.py whose weights are live there
    (maxdim 2 N = 30 on SPARSE, HOLED and `disagree`; maxdim 3 N = 13 on SPARSE and HOLED)."""
    import test_gpu_mask_patterns as MP
    return {"md2_n30_sparse": MP.Case(2, 30, MP.CFG2, "sparse"), "md2_n30_holed": MP.Case(2, 30, MP.CFG2, "holed"),
            "md2_n30_disagree": MP.Case(2, 30, MP.CFG2, "disagree"), "md3_n13_sparse": MP.Case(3, 13, MP.WIDE, "sparse"),
            "md3_n13_holed": MP.Case(3, 13, MP.WIDE, "holed")}


STEP_CASE_NAMES = ["md2_n30_sparse", "md2_n30_holed", "md2_n30_disagree", "md3_n13_sparse", "md3_n13_holed"]
# (case, get_real method): real and norm at maxdim 2, real at maxdim 3
STEP_RUNS = [(n, m) for n in STEP_CASE_NAMES for m in (("real", "norm") if n.startswith("md2") else ("real",))]


@functools.lru_cache(maxsize=None)
def step_forward(name):
    """(p4, labels, Pe, Pd, rec with its graph, pooled) of the oracle's networks on the case, computed once and never modified."""
    import _util as U
    import test_gpu_mask_patterns as MP
    from oracle import lgn_oracle as O
    case = step_cases()[name]
    p4, labels = MP._jets(case)
    _, _, Pe, Pd = MP._nets(case, "cpu")
    rec, _, pooled = U.oracle_forward(O, Pe, Pd, *MP._cfgs(case), p4, labels)
    return p4, labels, Pe, Pd, rec, pooled


def step_reference(name, loss, method, col=None, backward=True):
    """The oracle with the restatement as its loss: (per-jet terms (B,), {gradients} or None, assert_live's count of small gradient
    tensors, x = get_real(rec)).  loss = (choice, abs_coord, polar_coord); col: the assignment to score (the restatement's own when
    None).  U.assert_live(..., mask=labels) runs on these outputs alone."""
    import _hungarian_ref as H
    import _util as U
    from oracle import lgn_oracle as O
    p4, labels, Pe, Pd, rec, pooled = step_forward(name)
    x_o = O.get_real(rec.detach(), method)
    choice, a, p = loss
    if choice == "mse":
        terms = H.mse_per_jet(O.get_real(rec, method), p4)
    else:
        col = H.assignment(x_o, p4, a, p) if col is None else col
        terms = H.per_jet(O.get_real(rec, method), p4, col, a, p)
    grads = U.oracle_backward(terms.sum(), Pe, Pd, retain_graph=True) if backward else None
    floor = U.assert_live(O, rec.detach(), grads, p4, x_o, chamfer=False, pooled=pooled, latent_map="min&max", mask=labels)
    return terms.detach(), grads, floor, x_o


# ---- the post-processing calls after the evaluation step: the restatements against themselves ------------------------------------------
EVAL_NAMES = ["maxdim2_n30", "maxdim3_n13"]          # test_gpu_mask_patterns.EVAL_CASES, in its order
TRANS = 1e-11                                         # tests/test_gpu_analysis.py: device asinh / atan2 enter

# {(evaluation case, quantity): the largest |restatement - restatement with every jet's particles reversed| among the entries that
# miss the quantity's relative tolerance (1e-11), on the ORACLE's reconstruction of the case (the device's to 1e-14)}.  A
# Lorentz-equivariant network maps the one-particle jet `one_last` to multiples of that particle: its EMD and its matched (eta, phi)
# residuals and relative coordinates are zero in exact arithmetic, and what any implementation returns there is the rounding of O(1)
# operands.  Keys: (case, quantity, jet).  The device is held to the relative tolerance plus 100 x the figure on that jet, and to the
# relative tolerance alone on every other.  Measured by eval_self_disagreement() (particles reversed, and np.longdouble);
# tests/test_host_mask_cases.py asserts every figure, and that no other quantity needs one.
EVAL_CONDITIONING = {
    ("maxdim2_n30", "emd", 8): 5.7e-17, ("maxdim2_n30", "part_polarrel", 8): 4.2e-16, ("maxdim2_n30", "rel_err.2", 8): 0.44,
    ("maxdim3_n13", "part_polarrel", 8): 4.5e-16, ("maxdim3_n13", "rel_err.1", 8): 1.5e-16, ("maxdim3_n13", "rel_err.2", 8): 1.7,
}
# (rel_err.2 of that jet's one real row is a rounding residue of 1e-16 over target coordinate + 1e-16 with the target coordinate
# exactly 0: a number of order 1 with no correct digit on either side -- its figure says so)


def eval_floors(name, quantity, B):
    """(B,) the absolute term of a quantity per jet: 100 x the measured figure, 0 where none is listed"""
    out = np.zeros(B)
    for (n, q, j), fig in EVAL_CONDITIONING.items():
        if n == name and q == quantity:
            out[j] = 100 * fig
    return out


def _self_miss(a, b, rtol):
    """max |a - b| over the finite entries with |a - b| > rtol |a| (0.0 when there is none), and their number"""
    with np.errstate(all="ignore"):
        ok = np.isfinite(a) & np.isfinite(b)
        d = np.abs(np.asarray(a) - np.asarray(b)).astype(np.float64)
        a = np.asarray(a, dtype=np.float64)
        miss = ok & (d > rtol * np.abs(a))
    return (float(d[miss].max()) if miss.any() else 0.0), int(miss.sum())


@functools.lru_cache(maxsize=None)
def eval_self_disagreement(name):
    """{(quantity, jet): (figure, entries)}, figures above 0 only: _analysis_ref.recon_analysis (both find_match, both abs_coord) and
    _emd_ref.emd_relative on (target, the oracle's get_real(reconstruction)) of an evaluation case against (1) the same with every
    jet's particles reversed and (2) the same formulas in np.longdouble on the same assignment -- reversing moves the jet sums only,
    while the host's asinh / atan2 are themselves good to an ulp of the O(1) coordinates that a residual subtracts."""
    import _analysis_ref as R
    import test_gpu_mask_patterns as MP
    from oracle import lgn_oracle as O
    ref = MP._oracle(MP.EVAL_CASES[EVAL_NAMES.index(name)])
    t, x = ref.p4.numpy(), O.get_real(ref.rec, "sum").numpy()
    tr, xr = t[:, ::-1].copy(), x[:, ::-1].copy()
    B, N = t.shape[:2]
    out = {}

    def note(key, a, b, rtol, jets=None):                                 # a, b: (.., B, ...) with the jets on axis -3, or (B,)
        for j in range(B) if jets is None else jets:
            fig = _self_miss(a[j], b[j], rtol) if np.ndim(a) == 1 else _self_miss(np.take(a, j, -3), np.take(b, j, -3), rtol)
            if fig[0] > 0:
                out[(key, j)] = max(out.get((key, j), (0.0, 0)), fig)

    clean = [b for b in range(B) if t[b].any()]
    e0, e1 = np.full(B, np.nan), np.full(B, np.nan)
    e0[clean], e1[clean] = E.emd_relative(x[clean], t[clean]), E.emd_relative(xr[clean], tr[clean])
    note("emd", e0, e1, TRANS, clean)
    ld = np.longdouble
    for fm in (True, False):
        for ac in (True, False):
            a, b = R.recon_analysis(t, x, abs_coord=ac, find_match=fm), R.recon_analysis(tr, xr, abs_coord=ac, find_match=fm)
            pol = np.stack((R.p_polar(t.astype(ld)), R.p_polar(x.astype(ld))))
            rel = np.stack((R.p_polarrel(t.astype(ld)), R.p_polarrel(x.astype(ld)))) if ac else pol
            for k, exact in (("part_polar", pol), ("part_polarrel", rel)):
                note(k, a[k], b[k][:, :, ::-1], TRANS)
                note(k, a[k], exact, TRANS)
            back = N - 1 - b["col4row"][:, :, ::-1]                        # the reversed run's assignment in the original numbering
            for f, fr, k in ((0, None, 0), (1, pol, 0), (2, rel, 1)):
                same = np.flatnonzero((a["col4row"][k] == back[k]).all(-1))
                note(f"rel_err.{f}", a["rel_err"][f], b["rel_err"][f][:, ::-1], TRANS if f else 1e-12, same)
                if fr is not None:
                    with np.errstate(all="ignore"):
                        matched = np.take_along_axis(fr[1], a["col4row"][k][..., None], 1)
                        exact = (matched - fr[0]) / ((fr[0] + R.EPS) if fm else fr[0])
                    note(f"rel_err.{f}", a["rel_err"][f], exact, TRANS)
    return out


# ---- Chamfer with the jet term, and --normalize, inside the steps ------------------------------------------------------------------------
CHAMFER_RUNS = ["md2_n30_sparse", "md2_n30_holed", "md2_n30_disagree", "md3_n13_holed"]
RAW_SCALE = 40.0                  # raw jets: jet b of HOLED times RAW_SCALE (1 + b / 4); --normalize overall_max brings each back to max 1


def chamfer_jet_reference(name):
    """The oracle's Chamfer loss + jet-feature MSE (get_real 'sum') on a step case: (loss, {gradients}, assert_live's count)."""
    import _util as U
    from oracle import lgn_oracle as O
    p4, labels, Pe, Pd, rec, pooled = step_forward(name)
    loss = U.oracle_loss(O, Pe, Pd, rec, p4, get_real="sum", jet_term=True)
    grads = U.oracle_backward(loss, Pe, Pd, retain_graph=True)
    floor = U.assert_live(O, rec.detach(), grads, p4, O.get_real(rec.detach(), "sum"), pooled=pooled, latent_map="min&max", mask=labels)
    return loss.detach(), grads, floor


NORMALIZE_RUNS = ["md2_n30_holed", "md3_n13_holed"]
SINKHORN_STEP_RUNS = ["md2_n30_sparse", "md2_n30_holed", "md2_n30_disagree", "md3_n13_holed"]
EMD_STEP_LOSSES = {"emd": ("emd", {}), "emd_all": ("emd", EMD_ALL), "hybrid": ("hybrid", 0.5, {})}
EMD_STEP_RUNS = [(n, k) for n in ("md2_n30_sparse", "md2_n30_holed", "md2_n30_disagree", "md3_n13_holed") for k in EMD_STEP_LOSSES]


@functools.lru_cache(maxsize=None)
def raw_holed(N=30):
    """(raw p4, labels): HOLED with jet b scaled by RAW_SCALE (1 + b / 4) -- what --normalize is there for"""
    p4, labels = J.pattern_jets(N, J.HOLED, JET_SEED)
    scale = RAW_SCALE * (1.0 + torch.arange(len(p4), dtype=torch.float64) / 4.0)
    return p4 * scale.view(-1, 1, 1), labels


@functools.lru_cache(maxsize=None)
def normalize_reference(name="md2_n30_holed", method="overall_max"):
    """One oracle step (Chamfer, get_real 'sum') on _normalize_ref.normalize_p4(raw_holed) at the live weights of a HOLED step case,
    the mask taken from the momenta as a batch without labels has it: (normalised p4, loss, rec, {gradients}, assert_live's count)."""
    import _normalize_ref as NR
    import _util as U
    import test_gpu_mask_patterns as MP
    from oracle import lgn_oracle as O
    case = step_cases()[name]
    raw, _ = raw_holed(case.N)
    p4 = NR.normalize_p4(raw, method)[0]
    _, _, Pe, Pd = MP._nets(case, "cpu")
    loss, rec, grads, _, pooled = U.oracle_step(O, Pe, Pd, *MP._cfgs(case), p4, None, with_latent=True)
    floor = U.assert_live(O, rec, grads, p4, O.get_real(rec, "sum"), pooled=pooled, latent_map="min&max")
    return p4, loss, rec, grads, floor


# {(step case, option set): the weighted jets whose transport optimum on the ORACLE's reconstruction is degenerate by nondegenerate()}
# (tests/test_host_mask_cases.py asserts each list, and that every other weighted jet passes).  A one-particle jet is reconstructed
# as multiples of its particle (equivariance): its reconstructed particles share one or two positions and their arcs tie exactly,
# whatever the seed of the jets -- jets 1, 2 of SPARSE, jet 8 of HOLED.  `disagree` adds a jet with tied target rows.  A case with a
# degenerate jet has no reference gradient of the batch; the one case without (maxdim 3 under "all": with normalised weights and no
# fictitious particle the one target column takes every arc) is held to the oracle.
EMD_DEGENERATE = {("md2_n30_sparse", "default"): [1, 2], ("md2_n30_sparse", "all"): [1, 2],
                  ("md2_n30_holed", "default"): [8], ("md2_n30_holed", "all"): [8],
                  ("md2_n30_disagree", "default"): [0, 8], ("md2_n30_disagree", "all"): [1, 8],
                  ("md3_n13_holed", "default"): [8], ("md3_n13_holed", "all"): []}


def step_events(name):
    """(p, q, labels): the relative-polar events of the ORACLE's get_real(reconstruction, 'sum') and of the target of a step case, after
    U.assert_live on the forward alone -- what the EMD, hybrid and Sinkhorn loss stages of that case see."""
    import _util as U
    from oracle import lgn_oracle as O
    p4, labels, _, _, rec, pooled = step_forward(name)
    x = O.get_real(rec.detach(), "sum")
    U.assert_live(O, rec.detach(), None, p4, x, chamfer=False, pooled=pooled, latent_map="min&max", mask=labels)
    return E.relative_events(x.numpy()), E.relative_events(p4.numpy()), labels
