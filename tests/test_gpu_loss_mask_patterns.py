"""The loss kernels alone on jets with holes, sparse jets and disagreeing labels: assign_loss.hip (mse / Hungarian-MSE in four
frames), emd.hip (value, certificate, gradients, the relative forms, the option set "all") and sinkhorn.hip, each held PER JET to its
restatement (tests/_hungarian_ref.py, _emd_ref.py, _emd_grad_ref.py, _emd_opts_grad_ref.py, _sinkhorn_ref.py).

These kernels read no labels: each infers padding from the numbers.  Every other test of them feeds prefix-padded jets with four or
more real rows.  Here the targets are _jets.pattern_jets(N, HOLED | SPARSE) and the `disagree` copy (momenta on rows whose label is
0 -- the reference's losses use those rows), the reconstructions _jets.recon_like (small non-zero momenta on masked rows, the
all-masked jet exactly zero on both sides); tests/_mask_cases.py builds the pairs, tests/test_host_mask_cases.py asserts on the CPU
every decision that makes a case usable (non-degenerate optima at the recorded seeds, the statuses the restatements give).

    family                         sizes                  held to                                                   tolerance
    mse, hungarian x 4 frames      N 12, 30, 64, 65       _hungarian_ref.per_jet on the native assignment, which     1e-10 of the jet's own
                                   (64 | 65: one | two    must be an optimum of the exact costs (1e-12); status 0    loss / largest gradient
                                   solver columns a lane) on every jet, the all-zero one included                    entry
    emd, emd_grad (default, all)   n 12, 30, 63, 64       _emd_ref.emd / _emd_pairs_ref.emd (1e-12), the solver-free 1e-12 (certificate,
                                   (63 | 64: the seam of  certificate, the header's formulas on the returned flow    formulas), 1e-9 of the
                                   the wave layout)       and potentials, _emd(_opts)_grad_ref (scipy's LP)          largest entry (LP)
    emd_relative_tensor / _grad    N 12, 30, 63, 64       _emd_ref.emd_relative (1e-11), the generic kernel on       1e-10 of the jet's
    (default, all)                                        host-staged frames chained back by _frame_backward         largest gradient entry
    sinkhorn_grad (3 option sets)  30x30, 63x64, 64x65,   both float64 variants of _sinkhorn_ref at a fixed count    64 x their spread +
                                   82x82                  (tol = 0, 25 iterations), test_gpu_sinkhorn._compare       the rounding term
    sinkhorn_relative_grad,        N 12, 30               _sinkhorn_ref.sinkhorn_relative; SinkhornLoss bit-equal    as above
    SinkhornLoss                                          to the relative call

An `empty` jet is the only one a restatement flags: EMD and Sinkhorn give it NaN and EMPTY (under norm also when one side alone is
empty); the tests assert that status and that the NaN stays on that jet -- every other jet is bit-equal to a call without it.  The
assignment losses give it status 0, loss 0 and gradient 0 in every frame (the relative frames divide by the eps-guarded jet pT;
the restatement gives exactly 0, and so must the kernel).

The loss stages inside the steps (the last section of the file): NativeTrainStep (graph-replayed, two steps, the second a replay,
step.assignment filled with -7 before each) and NativeEvalStep at the live weights of tests/test_gpu_mask_patterns.py, against the
oracle with the restatement as its loss, scored on the step's own assignment.  mse and hungarian in four frames; get_real real and
norm at maxdim 2 N = 30 on SPARSE, HOLED and `disagree`, real at maxdim 3 N = 13 on SPARSE and HOLED; the evaluation step on HOLED at
both shapes, and the same 11 jets through a step built for 16, bit-equal in per-jet terms, statuses, assignments and
reconstruction.  FWD_TOL = 1e-11 per jet, ASSIGN_LOSS_TOL = 1e-10 per term, GRAD_TOL = 1e-9 per gradient tensor; U.assert_live
(mask = labels) holds on the oracle alone for every case (tests/test_host_mask_cases.py).  Chamfer with chamfer_jet_features=True
(the same cases, training and evaluation step) and --normalize overall_max on raw HOLED jets are held to the oracle in the same
way (--normalize also at maxdim 3 N = 13); SinkhornLoss runs through CapturedModuleStep against TrainStep on SPARSE, HOLED, `disagree`
(maxdim 2) and HOLED (maxdim 3) at the tolerances of tests/test_gpu_sinkhorn.py.  EMD (default, "all") and the hybrid loss with
native_emd=True run on the same four cases; they are held to the ORACLE in one of them only (maxdim 3 under "all"): in every other
an equivariant network reconstructs a one-particle jet as multiples of its particle, that jet's optimum is degenerate at every seed
(_mask_cases.EMD_DEGENERATE, asserted on the CPU) and the batch has no reference gradient.
test_emd_and_hybrid_loss_stages_on_mask_patterns says what every case is held to instead: the per-jet term is the score bit for bit
(hybrid: + weight x the restated Chamfer term), the EMPTY flags, the module-API step's gradients without the flagged jets.

Worst figures on the MI355X (relative to the jet's own term / largest gradient entry / the tensor's own maximum):

    assignment losses alone   sparse: term 6.7e-15, gradient 1.9e-14   holed: 1.3e-14, 1.7e-14   disagree: 1.3e-14, 1.9e-14
                              native assignment = the restatement's on every abs_cart case; in the other frames up to 7 of 11 jets
                              hold another optimum among the tied zero columns, each an optimum of the exact costs to 1e-12
    emd / emd_grad            value 1.2e-14 (default) / 3.7e-14 (all); formulas on the returned flow 2.2e-16 / 9.6e-16; against
                              scipy's LP 5.9e-15 / 2.5e-15
    emd_relative_(tensor|grad) value 1.2e-14 / 4.5e-14; Cartesian gradient against the generic kernel chained on the host 4.8e-14 / 8.0e-15
    sinkhorn                  every quantity inside the rule; one gradient by its measured tolerance (_CONDITIONING)
    training step             md2 N 30: jet recon 4.9e-15, term 7.9e-15, worst gradient tensor 5.0e-13 (disagree)
                              md3 N 13: jet recon 8.3e-15, term 1.6e-14, worst gradient tensor 1.0e-13 (sparse)
    evaluation step           md2 N 30: jet recon 4.7e-15, term 7.5e-15; md3 N 13: 8.3e-15, 1.6e-14; 11 jets in a step of 16: bit-equal
    Chamfer + jet term        loss 1.5e-14, jet recon 8.8e-15, worst gradient tensor 3.0e-14 (md3 N 13 holed)
    --normalize overall_max   loss 8.9e-15, jet recon 6.0e-15, worst gradient tensor 2.8e-14

Tolerances above the project's: one, measured from the reference side (_CONDITIONING below).  Kernel bugs found: none.

What these inputs would catch, measured on the CPU with a deliberately wrong restatement (tests/test_host_mask_cases.py asserts each):
  (i)  a loss target multiplied by the labels, on `disagree` at N = 12: moves jet 0's term by 0.75 .. 0.99 of itself (mse 0.99,
       abs_cart 0.99, abs_polar 0.75, rel_polar 0.75, rel_cart 0.97), its EMD by 0.84 (0.91 under "all"), its Sinkhorn value by 0.80
       -- against the 1e-10 .. 1e-12 the terms are held to.
  (ii) weightless particles compacted to a prefix with the results left in compacted order, HOLED at N = 12, 30, 64: the value does
       not move (1e-14: a transport problem does not depend on the order), the position gradients of every jet whose holes are not a
       suffix move by 0.45 .. 2 of their largest entry, the Sinkhorn gradients by 0.2 .. 1 -- which is why gradients, flow and
       potentials are compared per particle, not the value alone."""
import functools

import numpy as np
import pytest
import torch

import _emd_grad_ref as G
import _emd_opts_grad_ref as GO
import _emd_pairs_ref as P
import _emd_ref as E
import _hungarian_ref as H
import _mask_cases as C
import _sinkhorn_ref as S

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
ASSIGN_LOSS_TOL = 1e-10       # tests/test_gpu_hungarian_loss.py
CERT = 1e-12                  # tests/test_gpu_emd.py
LP_TOL = 1e-9                 # the LP restatements ask HiGHS for feasibility tolerances of 1e-10 on weights scaled to sum 1, so flow and
                              # marginals are promised to 1e-10 only: 10 x that (measured 5.9e-15; the tight check is CERT on the formulas)
REL_GRAD_TOL = 1e-10          # tests/test_gpu_emd_grad.py: the relative kernel against the generic one on host-staged frames
LOSSES = [("mse", True, False)] + [("hungarian",) + H.FRAMES[f] for f in H.FRAMES]
LOSS_IDS = ["mse"] + list(H.FRAMES)
BATCH_NAMES = ["sparse", "holed", "disagree"]

# {(batch, N, jet, quantity): the restatement's disagreement with itself, the jet's particles reversed} -- held to 100 x the figure
# instead of the rule it cannot keep against itself; measured on the CPU, tests/test_host_mask_cases.py asserts each.
#   sinkhorn_relative g_target of SPARSE jet 1 (one_first, N = 12): the frame of a one-particle jet is (1, 0, 0) whatever the
#   particle, so the chain back to the jet cancels terms of 1 / pT to nothing; the rule's bound is 5.4e-14, the restatement against
#   itself differs by 9.0e-14 (the MI355X from the restatement by 9.0e-14)
_CONDITIONING = C.SINKHORN_CONDITIONING


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def host(*xs):
    return [None if x is None else x.detach().cpu().numpy() for x in xs]


def _per_jet_close(got, want, tol, what):
    """got, want (B, ...): jet b within tol of ITS OWN largest |want[b]|; a jet whose restatement is exactly zero must be exactly
    zero.  Returns the worst relative error."""
    got, want = np.asarray(got, dtype=np.float64).reshape(len(want), -1), np.asarray(want, dtype=np.float64).reshape(len(want), -1)
    worst = 0.0
    for b in range(len(want)):
        top, err = np.abs(want[b]).max(), np.abs(got[b] - want[b]).max()
        assert np.isfinite(got[b]).all(), f"{what}: jet {b} is not finite"
        if top == 0:
            assert err == 0, f"{what}: jet {b} must be exactly zero, is {np.abs(got[b]).max():.3e}"
            continue
        assert err <= tol * top, f"{what}: jet {b}: rel err {err / top:.3e} > {tol:.1e} (its max {top:.3e})"
        worst = max(worst, err / top)
    return worst


# ---- assignment losses ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("loss", LOSSES, ids=LOSS_IDS)
@pytest.mark.parametrize("batch", BATCH_NAMES)
@pytest.mark.parametrize("N", [12, 30, 64, 65])
def test_assignment_losses_per_jet(N, batch, loss):
    """lgn_hungarian_mse_f64 on targets with holes: status 0 on every jet, the native assignment a permutation and an optimum of the
    exact costs (identical to the restatement's in the abs Cartesian frame, where both sides have exact IEEE costs), per-jet loss
    terms and the gradient of their sum scored on that assignment."""
    from lgn import _native as N_
    from test_gpu_hungarian_loss import _check_optimal
    choice, a, p = loss
    x, t, _ = C.pair(N, batch)
    kind = N_.LOSS_MSE if choice == "mse" else N_.LOSS_HUNGARIAN
    part, gx, col, status = N_.hungarian_mse(x.to(DEV), t.to(DEV), kind=kind, abs_coord=a, polar_coord=p)
    torch.cuda.synchronize()
    assert status.cpu().tolist() == [0] * len(x), f"status {status.cpu().tolist()}"
    col = col.cpu().long()
    what = f"{batch} N {N} {choice} abs {a} polar {p}"
    xr = x.clone().requires_grad_(True)
    if choice == "mse":
        assert bool((col == torch.arange(N)).all())
        per = H.mse_per_jet(xr, t)
    else:
        _check_optimal(x, t, col, a, p, True, what, pool=False)
        per = H.per_jet(xr, t, col, a, p)
    per.sum().backward()
    empty = C.empty_jets(batch)
    assert all(float(per[b].detach()) == 0 and float(xr.grad[b].abs().max()) == 0 for b in empty), "the restatement's zero against zero is 0"
    e_loss = _per_jet_close(part.cpu().numpy(), per.detach().numpy(), ASSIGN_LOSS_TOL, f"{what} loss term")
    e_grad = _per_jet_close(gx.cpu().numpy(), xr.grad.numpy(), ASSIGN_LOSS_TOL, f"{what} gradient")
    print(f"[{what}] worst jet: loss term {e_loss:.1e}, gradient {e_grad:.1e}")


@pytest.mark.parametrize("frame", list(H.FRAMES))
@pytest.mark.parametrize("N", [12, 65])
def test_assignment_loss_module_on_disagreeing_labels(N, frame):
    """lgn.losses.HungarianMSELoss (autograd) on the `disagree` batch: the sum of the per-jet terms and its gradient; the target's
    momenta on masked rows count, as in the reference."""
    from lgn.losses import HungarianMSELoss
    from test_gpu_hungarian_loss import _check_optimal
    a, p = H.FRAMES[frame]
    x, t, labels = C.pair(N, "disagree")
    assert bool((t[0][~labels[0].bool()] != 0).any()), "jet 0 carries momenta on masked rows"
    xd = x.to(DEV).requires_grad_(True)
    fn = HungarianMSELoss()
    loss = fn(xd, t.to(DEV), abs_coord=a, polar_coord=p)
    (3.0 * loss).backward()
    assert int(fn.status.abs().max()) == 0
    _check_optimal(x, t, fn.assignment, a, p, True, f"disagree N {N} {frame}", pool=False)
    xr = x.clone().requires_grad_(True)
    want = H.loss(xr, t, fn.assignment.cpu(), a, p)
    (3.0 * want).backward()
    assert abs(float(loss.detach()) - float(want.detach())) <= ASSIGN_LOSS_TOL * abs(float(want.detach()))
    _per_jet_close(xd.grad.cpu().numpy(), xr.grad.numpy(), ASSIGN_LOSS_TOL, f"disagree N {N} {frame} module gradient")


# ---- EMD --------------------------------------------------------------------------------------------------------------------------

EMD_OPTS = {"default": {}, "all": C.EMD_ALL}
ROLL = 3


@functools.lru_cache(maxsize=None)
def _event_pairs(N, batch, pairing):
    """(ev0, ev1) numpy (B, N, 3).  'recon': the target's events against the reconstruction's (weightless particles on one side: in
    mid-event, at index 0, as whole groups of four; the `empty` jets weightless on both).  'rolled': the target's events against
    the target of the jet ROLL places before (holes on both sides; an `empty` jet against a weighted one).  ROLL = 3 pairs no two
    one-particle jets: their relative events are both (1, 0, 0) up to rounding, an EMD of 2e-16 that the LP restatement (feasibility
    tolerances 1e-10) answers with 0 -- nothing to hold a value to; and no two `empty` jets, which 'recon' has already."""
    p, q = C.events(N, batch, C.EMD_SEEDS[(N, batch)])
    return (q, p) if pairing == "recon" else (q, np.roll(q, ROLL, axis=0))


def _want_status(ev0, ev1, o):
    from lgn import _native as N_
    return [N_.EMD_EMPTY if np.isnan(P.emd(ev0[b], ev1[b], **o)) else 0 for b in range(len(ev0))]


@pytest.mark.parametrize("opt", list(EMD_OPTS))
@pytest.mark.parametrize("pairing", ["recon", "rolled"])
@pytest.mark.parametrize("batch", BATCH_NAMES)
@pytest.mark.parametrize("n", [12, 30, 63, 64])
def test_emd_on_events_with_weightless_particles(n, batch, pairing, opt):
    from lgn import emd as M
    o = EMD_OPTS[opt]
    a, b = _event_pairs(n, batch, pairing)
    B = len(a)
    what = f"{batch} n {n} {pairing} {opt}"
    out = M.emd_grad(dev(a), dev(b), return_flow=True, return_duals=True, return_status=True, **o)
    val, g0, g1, flow, d0, d1, st = host(*out)
    want_st = _want_status(a, b, o)
    assert st.tolist() == want_st, f"{what}: status {st.tolist()}, the restatement flags {want_st}"
    flagged = [k for k in range(B) if want_st[k]]
    clean = [k for k in range(B) if not want_st[k]]
    empty = C.empty_jets(batch)
    if pairing == "recon":
        assert flagged == empty
    else:                                          # an empty event against a weighted one: the other's sum pT; EMPTY under norm
        assert not any(k in empty and (k - ROLL) % B in empty for k in range(B))
        assert flagged == ([k for k in range(B) if k in empty or (k - ROLL) % B in empty] if o.get("norm") else [])
    for k in flagged:                              # NaN stays on that pair ...
        assert np.isnan(val[k]) and np.isnan(g0[k]).all() and np.isnan(g1[k]).all(), (what, k)
    assert np.isfinite(val[clean]).all() and np.isfinite(g0[clean]).all() and np.isfinite(g1[clean]).all(), what
    if flagged:                                    # ... and every other pair is bit-equal to a call without it
        alone = M.emd_grad(dev(a[clean]), dev(b[clean]), return_flow=True, return_duals=True, return_status=True, **o)
        for x, y in zip(out, alone):
            assert torch.equal(x[clean], y), what
    assert np.array_equal(val, M.emd(dev(a), dev(b), return_status=True, **o)[0].cpu().numpy(), equal_nan=True)
    worst = {"value": 0.0, "formula": 0.0, "lp": 0.0}
    for k in clean:
        P.certify(val[k], flow[k], d0[k], d1[k], a[k], b[k], **o)
        want = P.emd(a[k], b[k], **o)
        assert abs(val[k] - want) <= CERT * abs(want), (what, k, val[k], want)
        worst["value"] = max(worst["value"], abs(val[k] - want) / abs(want) if want else 0.0)
        w0, w1 = GO.formula(a[k], b[k], flow[k], d0[k], d1[k], **o)
        top = max(np.abs(w0).max(), np.abs(w1).max())
        err = max(np.abs(g0[k] - w0).max(), np.abs(g1[k] - w1).max())
        assert top > 0 and err <= CERT * top, (what, k, err, top)
        worst["formula"] = max(worst["formula"], err / top)
        if pairing == "recon" and k not in C.lp_jets(batch):    # `disagree` jet 1: two identical TARGET rows.  The split of a
            # reconstructed particle's flow between them is free, but they sit at one position: the gradient with respect to the
            # reconstruction's positions is the same at every optimum, and is compared; the target's own rows are not
            _, _, l1 = GO.emd_grad(a[k], b[k], **o)
            top = np.abs(l1[:, 1:]).max()
            err = np.abs(g1[k] - l1)[:, 1:].max()
            assert err <= LP_TOL * top, (what, k, err, top)
            worst["lp"] = max(worst["lp"], err / top)
        if pairing == "recon" and k in C.lp_jets(batch):        # the seeds make THIS pairing's optimum non-degenerate
            _, l0, l1 = GO.emd_grad(a[k], b[k], **o)
            # a weightless particle's weight gradient is a free potential (the LP leaves it out): compare where it has weight
            m0, m1 = a[k][:, 0] > 0, b[k][:, 0] > 0
            top = max(np.abs(l0[m0]).max(), np.abs(l1[m1]).max())
            err = max(np.abs(g0[k] - l0)[m0].max(), np.abs(g1[k] - l1)[m1].max(), np.abs(g0[k] - l0)[:, 1:].max(),
                      np.abs(g1[k] - l1)[:, 1:].max())
            assert err <= LP_TOL * top, (what, k, err, top)
            worst["lp"] = max(worst["lp"], err / top)
    print(f"[{what}] worst pair: " + ", ".join(f"{q} {v:.1e}" for q, v in worst.items()))


@pytest.mark.parametrize("opt", list(EMD_OPTS))
@pytest.mark.parametrize("batch", BATCH_NAMES)
@pytest.mark.parametrize("N", [12, 30, 63, 64])
def test_emd_relative_forms_on_jets_with_holes(N, batch, opt):
    """emd_relative_tensor / emd_relative_grad on Cartesian jets whose target has holes: the value against the restatement on
    host-staged frames (1e-11: device asinh / atan2), the Cartesian gradients against the generic kernel on those frames chained
    back on the host; EMPTY and NaN on the `empty` jets only, every other jet bit-equal to a call without them."""
    from lgn import _native as N_
    from lgn import emd as M
    o = EMD_OPTS[opt]
    x, t, _ = C.pair(N, batch, C.EMD_SEEDS[(N, batch)])
    x, t = x.numpy(), t.numpy()
    what = f"{batch} N {N} {opt}"
    out = M.emd_relative_grad(dev(x), dev(t), need_g_target=True, **o)
    val, gr, gt, st = host(*out)
    empty, clean = C.empty_jets(batch), C.weighted_jets(batch)
    assert st.tolist() == [N_.EMD_EMPTY if b in empty else 0 for b in range(len(x))], (what, st.tolist())
    assert np.isnan(val[empty]).all() and np.isnan(gr[empty]).all() and np.isnan(gt[empty]).all()
    assert np.isfinite(val[clean]).all() and np.isfinite(gr[clean]).all() and np.isfinite(gt[clean]).all()
    alone = M.emd_relative_grad(dev(x[clean]), dev(t[clean]), need_g_target=True, **o)
    for a, b in zip(out, alone):
        assert torch.equal(a[clean], b), what
    only, st2 = M.emd_relative_tensor(dev(x), dev(t), return_status=True, **o)
    assert np.array_equal(only.cpu().numpy(), val, equal_nan=True) and torch.equal(st2, out[3])
    p, q = E.relative_events(x), E.relative_events(t)
    v2, g0, g1 = host(*M.emd_grad(dev(p[clean]), dev(q[clean]), **o))
    worst = {"value": 0.0, "gradient": 0.0}
    for i, b in enumerate(clean):
        want = P.emd(p[b], q[b], **o)
        assert abs(val[b] - want) <= 1e-11 * abs(want) and abs(val[b] - v2[i]) <= 1e-11 * abs(want), (what, b, val[b], want, v2[i])
        worst["value"] = max(worst["value"], abs(val[b] - want) / abs(want))
        wr, wt = G._frame_backward(x[b], g0[i]), G._frame_backward(t[b], g1[i])
        top = max(np.abs(wr).max(), np.abs(wt).max())
        err = max(np.abs(gr[b] - wr).max(), np.abs(gt[b] - wt).max())
        assert err <= REL_GRAD_TOL * top, f"{what} jet {b}: |REL - generic chained on the host| = {err:.3e}, max |g| {top:.3e}"
        assert (gr[b][:, 0] == 0).all() and (gt[b][:, 0] == 0).all()
        worst["gradient"] = max(worst["gradient"], err / top)
    print(f"[{what}] worst jet: " + ", ".join(f"{k} {v:.1e}" for k, v in worst.items()))


# ---- Sinkhorn ---------------------------------------------------------------------------------------------------------------------

SINKHORN_OPTS = {"default": {}, "beta2": dict(beta=2.0), "all": C.EMD_ALL}
SINKHORN_EPS = {"default": 0.1, "beta2": 0.2, "all": 1.5}        # 0.1 x the largest cost, as tests/test_gpu_sinkhorn.py's fixed-count cases


@pytest.mark.parametrize("opt", list(SINKHORN_OPTS))
@pytest.mark.parametrize("batch", BATCH_NAMES)
@pytest.mark.parametrize("n,m", [(30, 30), (63, 64), (64, 65), (82, 82)])
def test_sinkhorn_on_events_with_weightless_particles(n, m, batch, opt):
    """sinkhorn_grad at a fixed count (tol = 0: no stopping decision depends on last bits) on the targets' events at N = n against
    the next jet's at N = m: weightless particles in mid-event, at index 0 and as whole groups, on both sides.  The rule of
    test_gpu_sinkhorn._compare on every pair the restatement does not flag; a flagged pair has the restatement's status and NaN."""
    from test_gpu_sinkhorn import _compare, _run
    o = SINKHORN_OPTS[opt]
    a, b = C.events(n, batch)[1], np.roll(C.events(m, batch)[1], 1, axis=0)
    kw = dict(max_iter=25, tol=0.0, debias=True)
    eps = SINKHORN_EPS[opt]
    got = _run(a, b, eps, kw, o)
    what = f"{batch} {n}x{m} {opt}"
    want_st = [S.sinkhorn(a[i], b[i], eps, variant=0, **kw, **o)["status"] for i in range(len(a))]
    assert got["status"].tolist() == want_st, f"{what}: status {got['status'].tolist()}, the restatement's {want_st}"
    clean = [i for i, s in enumerate(want_st) if s == 0]
    for i in set(range(len(a))) - set(clean):
        assert bool(torch.isnan(got["value"][i])) and bool(torch.isnan(got["g0"][i]).all()) and bool(torch.isnan(got["g1"][i]).all())
    empty, B = C.empty_jets(batch), len(a)         # both sides empty, or under norm either: exactly those pairs are flagged
    assert [i for i in range(B) if i not in clean] == [i for i in range(B) if (i in empty and (i - 1) % B in empty)
                                                       or (o.get("norm") and (i in empty or (i - 1) % B in empty))], what
    assert (got["iters"][clean] == 25).all()
    _compare(what, a[clean], b[clean], eps, kw, o, {k: v[clean] for k, v in got.items()})


@pytest.mark.parametrize("batch", BATCH_NAMES)
@pytest.mark.parametrize("N", [12, 30])
def test_sinkhorn_relative_call_and_loss_module_on_jets_with_holes(N, batch):
    """sinkhorn_relative_grad on (reconstruction, target) against the restatement on host-staged frames, by the rule of
    test_gpu_sinkhorn.test_the_relative_call_carries_the_gradients_back_to_the_jets; SinkhornLoss is that call bit for bit: NaN with
    the `empty` jet in the batch, and on the weighted jets alone the same sum and gradient."""
    from lgn import sinkhorn as K
    from lgn.losses import SinkhornLoss
    from test_gpu_sinkhorn import _scales
    x, t, _ = C.pair(N, batch)
    xn, tn = x.numpy(), t.numpy()
    eps, kw = 1.0, dict(max_iter=6, tol=0.0, debias=True)
    value, g_r, g_t, iters, err, status = K.sinkhorn_relative_grad(dev(xn), dev(tn), eps, need_g_target=True, **kw)
    torch.cuda.synchronize()
    empty, clean = C.empty_jets(batch), C.weighted_jets(batch)
    assert [int(s) & 3 for s in status.tolist()] == [K.EMPTY if b in empty else 0 for b in range(len(x))]
    assert bool(torch.isnan(value[empty]).all()) and bool(torch.isnan(g_r[empty]).all()) and bool((iters[clean] == 6).all())
    p, q = E.relative_events(xn), E.relative_events(tn)
    for i in clean:
        r0 = S.sinkhorn_relative(xn[i], tn[i], eps, variant=0, **kw)
        r1 = S.sinkhorn_relative(xn[i], tn[i], eps, variant=1, **kw)
        assert r0["status"] == 0
        bound = 64 * abs(r0["value"] - r1["value"]) + 8 * (2 * N + 2) * 2.0 ** -53 * _scales(p[i], q[i], {})["value"]
        assert abs(float(value[i]) - r0["value"]) <= bound, (batch, N, i, float(value[i]), r0["value"], bound)
        for got, key in ((g_r[i], "g_recons"), (g_t[i], "g_target")):
            top = np.abs(r0[key]).max()
            bound = 64 * np.abs(r0[key] - r1[key]).max() + 8 * (2 * N + 2) * 2.0 ** -53 * top
            if (batch, N, i, key) in _CONDITIONING:
                bound = 100 * _CONDITIONING[(batch, N, i, key)]
            d = np.abs(got.cpu().numpy() - r0[key]).max()
            assert d <= bound, f"{batch} N {N} jet {i}, {key}: {d:.3e} > {bound:.3e}"
    for rows in (list(range(len(x))), clean):
        loss = SinkhornLoss(num_particles=N, device=DEV, epsilon=eps, **kw)
        xd = dev(xn[rows]).requires_grad_(True)
        out = loss(xd, dev(tn[rows]))
        ref = K.sinkhorn_relative_grad(dev(xn[rows]), dev(tn[rows]), eps, **kw)
        assert np.array_equal(out.detach().cpu().numpy(), ref[0].sum().cpu().numpy(), equal_nan=True)
        assert bool(torch.isnan(out)) == (rows is not clean)
        assert torch.equal(loss.status, ref[5]) and torch.equal(loss.iters, ref[3])
        (g,) = torch.autograd.grad(out, xd)
        assert np.array_equal(g.cpu().numpy(), ref[1].cpu().numpy(), equal_nan=True)
        assert np.array_equal(ref[0].cpu().numpy(), value[rows].cpu().numpy(), equal_nan=True)
        assert np.array_equal(ref[1].cpu().numpy(), g_r[rows].cpu().numpy(), equal_nan=True)


# ---- the assignment losses inside the steps -----------------------------------------------------------------------------------------
FWD_TOL = 1e-11               # tests/test_gpu_mask_patterns.py
GRAD_TOL = 1e-9


def _step_opts(loss, method):
    return dict(get_real_method=method, loss_choice=loss[0], hungarian_abs_coord=loss[1], hungarian_polar_coord=loss[2])


def _score_step(name, loss, method, step, recon_real, what):
    """What a step left behind against the oracle with the restatement as its loss, scored on the step's own assignment: status 0 on
    every jet, the assignment an optimum of the exact costs on the step's own reconstruction, the per-jet loss terms at
    ASSIGN_LOSS_TOL of themselves (a zero term exactly zero), get_real(reconstruction) per jet at FWD_TOL (an all-masked jet exactly
    as the oracle has it).  Returns (the oracle's gradients, its count of small tensors, the worst figures)."""
    from test_gpu_hungarian_loss import _check_optimal
    from test_gpu_mask_patterns import _per_jet
    choice, a, p = loss
    p4 = C.step_forward(name)[0]
    col = step.assignment.cpu().long()
    assert step.status.cpu().tolist() == [0] * len(p4), step.status.cpu().tolist()
    if choice == "hungarian":
        _check_optimal(recon_real.detach().cpu(), p4, col, a, p, True, what, pool=False, identical=bool(a and not p and method == "real"))
    else:
        assert bool((col == torch.arange(col.shape[1])).all())
    terms, grads, floor, x_o = C.step_reference(name, loss, method, col=col)
    e_rec = _per_jet(recon_real.detach().unsqueeze(0), x_o.unsqueeze(0), torch.arange(len(p4)), FWD_TOL, f"{what} get_real(recon)",
                     exact_zero=(method == "real"))
    e_term = _per_jet_close(step.loss_part.cpu().numpy()[:len(p4)], terms.numpy(), ASSIGN_LOSS_TOL, f"{what} loss term")
    return grads, floor, {"recon": e_rec, "term": e_term}


@pytest.mark.parametrize("loss", LOSSES, ids=LOSS_IDS)
@pytest.mark.parametrize("name,method", C.STEP_RUNS)
def test_assignment_losses_in_the_training_step(name, method, loss):
    """NativeTrainStep (graph-replayed, two steps, the second a replay, step.assignment filled with -7 before each) on SPARSE, HOLED
    and `disagree`: per-jet terms, reconstruction per jet, every gradient tensor at GRAD_TOL of its own maximum.  On `disagree` the
    target the loss sees carries momenta on rows whose label is 0, and the oracle's loss uses them."""
    import _util as U
    from lgn.step import NativeTrainStep, get_real
    from test_gpu_mask_patterns import _nets
    case = C.step_cases()[name]
    p4, labels = C.step_forward(name)[:2]
    enc, dec, _, _ = _nets(case, DEV)
    step = NativeTrainStep(enc, dec, batch_size=len(p4), l1_lambda=0.0, optimizer=False, use_graph=True, **_step_opts(loss, method))
    batch = {"p4": p4.to(DEV), "labels": labels.to(DEV)}
    for _ in range(2):
        step.assignment.fill_(-7)
        got, recon = step.step(batch)
    torch.cuda.synchronize()
    what = f"train {name} {loss[0]} abs {loss[1]} polar {loss[2]} {method}"
    grads, floor, errs = _score_step(name, loss, method, step, get_real(recon.detach(), method), what)
    terms = C.step_reference(name, loss, method, col=step.assignment.cpu().long(), backward=False)[0]
    U.assert_close(got, terms.sum(), ASSIGN_LOSS_TOL, "loss")
    worst, tensor = U.assert_named_grads_close(U.named_grads(enc, dec), grads, GRAD_TOL, what, max_floor_routed=floor)
    print(f"[{what}] worst jet: recon {errs['recon']:.1e}, loss term {errs['term']:.1e}; worst gradient tensor {tensor}: {worst:.1e}")


@pytest.mark.parametrize("loss", LOSSES, ids=LOSS_IDS)
@pytest.mark.parametrize("name", ["md2_n30_holed", "md3_n13_holed"])
def test_assignment_losses_in_the_evaluation_step(name, loss):
    """NativeEvalStep on HOLED with each assignment loss, and the same 11 jets through a step built for 16: per-jet terms, statuses,
    assignments and reconstruction of the 11 jets bit-equal to the 11-jet step."""
    import _util as U
    from lgn.step import NativeEvalStep
    from test_gpu_mask_patterns import _nets
    case = C.step_cases()[name]
    p4, labels = C.step_forward(name)[:2]
    K = len(p4)
    batch = {"p4": p4.to(DEV), "labels": labels.to(DEV)}
    kept = {}
    for size in (K, 16):
        enc, dec, _, _ = _nets(case, DEV)
        ev = NativeEvalStep(enc, dec, size, use_graph=True, **_step_opts(loss, "real"))
        for _ in range(2):
            ev.assignment.fill_(-7)
            out = ev.run(batch)
        torch.cuda.synchronize()
        kept[size] = (out["loss"].clone(), out["recon"].clone(), ev.loss_part[:K].clone(), ev.status[:K].clone(), ev.assignment[:K].clone(), ev)
    what = f"eval {name} {loss[0]} abs {loss[1]} polar {loss[2]}"
    ev = kept[K][5]
    _, _, errs = _score_step(name, loss, "real", ev, kept[K][1], what)
    terms = C.step_reference(name, loss, "real", col=ev.assignment.cpu().long()[:K], backward=False)[0]
    U.assert_close(kept[K][0], terms.sum(), ASSIGN_LOSS_TOL, "loss")
    for i, k in enumerate(("recon", "loss_part", "status", "assignment"), start=1):
        assert torch.equal(kept[K][i], kept[16][i]), f"{what}: {k} of the 11 jets through the step built for 16"
    U.assert_close(kept[16][0], kept[K][0], 1e-14, "loss of the step built for 16")
    print(f"[{what}] worst jet: recon {errs['recon']:.1e}, loss term {errs['term']:.1e}")


# ---- Chamfer with the jet term, --normalize and SinkhornLoss inside the steps -----------------------------------------------------------

@pytest.mark.parametrize("name", C.CHAMFER_RUNS)
def test_chamfer_with_the_jet_term_in_the_steps(name):
    """chamfer_jet_features=True on SPARSE, HOLED, `disagree` (maxdim 2 N = 30) and HOLED at maxdim 3 N = 13: the jet-feature MSE sums
    ALL rows of both sides, masked ones included -- on `disagree` the target's stray momenta count.  Training step against the oracle
    (loss, reconstruction per jet, every gradient tensor); evaluation step: the loss, and the same jets through a step built for 16
    bit-equal in the reconstruction."""
    import _util as U
    from lgn.step import NativeEvalStep, NativeTrainStep
    from test_gpu_mask_patterns import _nets, _per_jet
    case = C.step_cases()[name]
    p4, labels, _, _, rec_o, _ = C.step_forward(name)
    loss_o, grads, floor = C.chamfer_jet_reference(name)
    K = len(p4)
    enc, dec, _, _ = _nets(case, DEV)
    step = NativeTrainStep(enc, dec, batch_size=K, l1_lambda=0.0, optimizer=False, use_graph=True, get_real_method="sum",
                           chamfer_jet_features=True)
    batch = {"p4": p4.to(DEV), "labels": labels.to(DEV)}
    for _ in range(2):
        got, recon = step.step(batch)
    torch.cuda.synchronize()
    what = f"chamfer + jet term {name}"
    U.assert_close(got, loss_o, FWD_TOL, "loss")
    e_rec = _per_jet(recon, rec_o.detach(), torch.arange(K), FWD_TOL, "recon")
    worst, tensor = U.assert_named_grads_close(U.named_grads(enc, dec), grads, GRAD_TOL, what, max_floor_routed=floor)
    outs = {}
    for size in (K, 16):
        ev = NativeEvalStep(enc, dec, size, get_real_method="sum", chamfer_jet_features=True, use_graph=True)
        for _ in range(2):
            out = ev.run(batch)
        torch.cuda.synchronize()
        outs[size] = (out["loss"].clone(), out["recon"].clone())
        U.assert_close(out["loss"], loss_o, FWD_TOL, f"evaluation loss, step built for {size}")
    assert torch.equal(outs[K][1], outs[16][1])
    print(f"[{what}] loss {U.relerr(got.cpu(), loss_o):.1e}, worst jet recon {e_rec:.1e}, worst gradient tensor {tensor}: {worst:.1e}")


@pytest.mark.parametrize("name", C.NORMALIZE_RUNS)
def test_normalize_on_raw_holed_jets_in_the_training_step(name):
    """--normalize overall_max on HOLED scaled per jet by 40 .. 140 (no labels: the mask is the momenta's, as the reference's loop has
    it): the step normalises on the device; the oracle gets _normalize_ref.normalize_p4 of the raw batch.  The all-masked jet divides
    by its eps-guarded maximum 0 and stays exactly zero."""
    import _util as U
    from lgn.step import NativeTrainStep
    from test_gpu_mask_patterns import _nets, _per_jet
    case = C.step_cases()[name]
    raw, _ = C.raw_holed(case.N)
    p4_o, loss_o, rec_o, grads, floor = C.normalize_reference(name)
    enc, dec, _, _ = _nets(case, DEV)
    step = NativeTrainStep(enc, dec, batch_size=len(raw), l1_lambda=0.0, optimizer=False, use_graph=True, get_real_method="sum",
                           normalize=True, normalize_method="overall_max")
    for _ in range(2):
        got, recon = step.step({"p4": raw.to(DEV)})
    torch.cuda.synchronize()
    U.assert_close(got, loss_o, FWD_TOL, "loss")
    e_rec = _per_jet(recon, rec_o, torch.arange(len(raw)), FWD_TOL, "recon")
    worst, tensor = U.assert_named_grads_close(U.named_grads(enc, dec), grads, GRAD_TOL, f"normalize overall_max {name}", max_floor_routed=floor)
    print(f"[normalize overall_max {name}] loss {U.relerr(got.cpu(), loss_o):.1e}, worst jet recon {e_rec:.1e}, worst gradient tensor {tensor}: {worst:.1e}")


@pytest.mark.parametrize("name", C.SINKHORN_STEP_RUNS)
def test_sinkhorn_loss_in_the_captured_module_step_on_mask_patterns(name):
    """SinkhornLoss through CapturedModuleStep against TrainStep on SPARSE, HOLED, `disagree` (maxdim 2) and HOLED (maxdim 3) at live weights, at the tolerances tests/test_gpu_sinkhorn.py
    states for that pair (1e-10 loss and reconstruction, 1e-9 parameters after one Adam step).  With the all-masked jet in the batch
    both give NaN and flag that jet EMPTY (and no other); the comparison runs on the weighted jets."""
    import _util as U
    from lgn import sinkhorn as K
    from lgn.losses import SinkhornLoss
    from lgn.step import CapturedModuleStep, TrainStep
    from test_gpu_mask_patterns import _nets
    case = C.step_cases()[name]
    p4, labels = C.step_forward(name)[:2]
    kw = dict(epsilon=0.05, max_iter=60, tol=1e-7)
    empty = (labels.sum(1) == 0).nonzero().flatten().tolist()
    clean = [b for b in range(len(p4)) if b not in empty]
    for rows in (list(range(len(p4))), clean):
        (ea, da, _, _), (eb, db, _, _) = _nets(case, DEV), _nets(case, DEV)
        la_mod, lb_mod = SinkhornLoss(**kw), SinkhornLoss(**kw)
        a = CapturedModuleStep(ea, da, batch_size=len(rows), lr=1e-3, l1_lambda=1e-8, use_graph=True, loss_choice=la_mod)
        b = TrainStep(eb, db, lr=1e-3, l1_lambda=1e-8, loss_choice=lb_mod)
        batch = {"p4": p4[rows].to(DEV), "labels": labels[rows].to(DEV)}
        la, ra = a.step(batch)
        lb, rb = b.step(batch)
        torch.cuda.synchronize()
        assert torch.equal(la_mod.iters, lb_mod.iters) and torch.equal(la_mod.status, lb_mod.status)
        want = [K.EMPTY if r in empty else 0 for r in rows]
        assert [int(s) & 3 for s in la_mod.status.tolist()] == want
        if rows is not clean:
            assert bool(torch.isnan(la)) and bool(torch.isnan(lb))
            continue
        assert bool(torch.isfinite(la))
        U.assert_close(la, lb, 1e-10, "loss")
        U.assert_close(ra, rb, 1e-10, "reconstruction")
        U.assert_close(a.flat.flat, b.flat.flat, 1e-9, "parameters after one Adam step")


# ---- EMD and hybrid losses as the loss stage ------------------------------------------------------------------------------------------
EMD_STEP_LOSSES, EMD_STEP_RUNS = C.EMD_STEP_LOSSES, C.EMD_STEP_RUNS


@pytest.mark.parametrize("name,kind", EMD_STEP_RUNS)
def test_emd_and_hybrid_loss_stages_on_mask_patterns(name, kind):
    """NativeTrainStep / NativeEvalStep with native_emd=True on SPARSE, HOLED, `disagree` (maxdim 2 N = 30) and HOLED (maxdim 3 N = 13).
    An oracle comparison only where _mask_cases.EMD_DEGENERATE lists no jet (maxdim 3 under "all"): after a Lorentz-equivariant
    network a one-particle jet is reconstructed as multiples of its particle, its arcs tie and its gradient is a set, whatever the
    seed, so the batch has no reference gradient (tests/test_host_mask_cases.py asserts the table on the oracle's reconstruction).
    Held in every case: the per-jet term is the EMD score of the step's own reconstruction bit for bit (that score is held to its
    restatement on holed jets above and in tests/test_gpu_postproc_mask_patterns.py), for the hybrid loss the score + weight x the
    jet's Chamfer term restated on the CPU; the all-masked jets are flagged EMPTY with a NaN term, and no other jet is; the
    gradients are those of the module-API step (TrainStep with the loss module, under autograd -- the same EMD kernel: this holds
    the stage's wiring) on the batch WITHOUT the flagged jets, at the tolerances of tests/test_gpu_emd_step.py (1e-10
    reconstruction, 1e-9 per gradient tensor); the evaluation step gives the same terms and flags, also through a step built for 16."""
    import _util as U
    from lgn import _native as N_
    from lgn import emd as M
    from lgn.step import NativeEvalStep, NativeTrainStep, TrainStep, get_real
    from test_gpu_emd_step import _grads, _module
    from test_gpu_mask_patterns import _nets
    case = C.step_cases()[name]
    loss = EMD_STEP_LOSSES[kind]
    opts = loss[1] if loss[0] == "emd" else loss[2]
    p4, labels = C.step_forward(name)[:2]
    K = len(p4)
    empty = (labels.sum(1) == 0).nonzero().flatten().tolist()
    clean = [b for b in range(K) if b not in empty]
    batch = {"p4": p4.to(DEV), "labels": labels.to(DEV)}
    (ea, da, _, _), (eb, db, _, _) = _nets(case, DEV), _nets(case, DEV)
    nat = NativeTrainStep(ea, da, batch_size=K, l1_lambda=0.0, optimizer=False, use_graph=True, get_real_method="sum",
                          loss_choice=_module(loss), native_emd=True)
    for _ in range(2):
        _, recon = nat.step(batch)
    torch.cuda.synchronize()
    x = get_real(recon.detach(), "sum")
    score, st = M.emd_relative_tensor(x, batch["p4"], return_status=True, **opts)
    want_st = [N_.EMD_EMPTY if b in empty else 0 for b in range(K)]
    assert nat.status.cpu().tolist() == want_st and st.cpu().tolist() == want_st
    if loss[0] == "emd":
        assert np.array_equal(nat.loss_part.cpu().numpy()[:K], score.cpu().numpy(), equal_nan=True)
    assert bool(torch.isnan(nat.loss_part[empty]).all()) and bool(torch.isfinite(nat.loss_part[clean]).all())
    assert bool(torch.isfinite(nat.flat.grad).all()) and bool((x[empty] == 0).all())
    ref = TrainStep(eb, db, l1_lambda=0.0, optimizer=False, loss_choice=_module(loss), get_real_method="sum")
    _, rec_m = ref.step({k: v[clean] for k, v in batch.items()})
    torch.cuda.synchronize()
    U.assert_close(recon[:, clean], rec_m, 1e-10, "reconstruction")
    worst = U.assert_named_grads_close(U.named_grads(ea, da), _grads(eb, db), 1e-9, f"{name} {kind}")
    kept = {}
    for size in (K, 16):
        ev = NativeEvalStep(ea, da, size, get_real_method="sum", use_graph=True, loss_choice=_module(loss), native_emd=True)
        for _ in range(2):
            out = ev.run(batch)
        torch.cuda.synchronize()
        kept[size] = (ev.loss_part[:K].clone(), ev.status[:K].clone(), out["recon"].clone())
        assert ev.status[:K].cpu().tolist() == want_st
    assert np.array_equal(kept[K][0].cpu().numpy(), nat.loss_part[:K].cpu().numpy(), equal_nan=True)
    assert np.array_equal(kept[K][0].cpu().numpy(), kept[16][0].cpu().numpy(), equal_nan=True) and torch.equal(kept[K][2], kept[16][2])
    if loss[0] == "hybrid":                        # the term is the score + weight x the jet's Chamfer term, restated on the CPU
        per = U.chamfer_per_jet(x.cpu(), p4)
        want = score.cpu()[clean] + loss[1] * per[clean]
        assert float(((nat.loss_part.cpu()[clean] - want).abs() / want.abs()).max()) <= FWD_TOL, "hybrid per-jet term"
    print(f"[{name} {kind}] worst gradient tensor against the module step: {worst}")
    if C.EMD_DEGENERATE[(name, "all" if kind == "emd_all" else "default")]:
        return
    # no degenerate jet (asserted on the CPU): the oracle with the restated EMD of the weighted jets as its loss.  The LP restatement
    # is good to its solver's 1e-10, so, as tests/test_gpu_emd_step.py::test_against_the_oracle has it, no tolerance is fixed: the
    # native step may differ from the oracle by at most 10 x what the module-API step does (floor 1e-12), per gradient tensor
    from test_gpu_emd_step import _RefEMD
    from oracle import lgn_oracle as O
    _, _, Pe, Pd, rec_o, _ = C.step_forward(name)
    frozen = tuple(sorted(opts.items()))
    terms = _RefEMD.apply(O.get_real(rec_o, "sum")[clean], p4[clean], frozen)
    grads_o = U.oracle_backward(terms.sum(), Pe, Pd, retain_graph=True)
    np.testing.assert_allclose(nat.loss_part.cpu().numpy()[clean], terms.detach().numpy(), rtol=1e-11, atol=0)
    mod, got, checked = _grads(eb, db), dict(U.named_grads(ea, da)), 0
    for tname, g in grads_o.items():
        if g is None or float(g.abs().max()) == 0:
            continue
        dm, dn = (float((v[tname].detach().cpu() - g).abs().max() / g.abs().max()) for v in (mod, got))
        assert dn <= max(10 * dm, 1e-12), (tname, dn, dm)
        checked += 1
    assert checked >= 10
    print(f"[{name} {kind}] held to the oracle: {checked} gradient tensors")
