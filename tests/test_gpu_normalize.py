"""GPU tests of the native --normalize path: the staging kernel (csrc/stage.hip) against the torch restatement of
utils/normalize_p4.py and Encoder._prepare_input, the de-normalise kernel, lgn.ops.normalize_p4, and the training / evaluation steps
with ``normalize=True`` against the same steps fed the staged buffers, the module-API steps and the reference's g21 step fixture.

Tolerances (u = 2^-53): max and one add are exact, so the factors of the two max methods are bit-equal; the jet_E factor is a sum of
N non-negative energies, two summation orders of which differ by at most 2 (N - 1) u relative; a correctly rounded quotient of the
kernel's own factor is within one ulp (2^-52 relative) of torch's; a product by the scale is exact to the bit."""
import functools
import json
import types

import numpy as np
import pytest
import torch

import _normalize_ref as R
import _util as U

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
U53 = 2.0 ** -53
METHODS = ["component_max", "overall_max", "jet_E"]
B, B_PAD = 5, 7


@functools.lru_cache(maxsize=None)
def _inputs(N):
    """(p4, labels) on the CPU, shared by every case of a jet size and never modified: jets of very different scales, the last
    third of the rows zero where there are rows to spare, labels that mask rows of their own choosing."""
    p4 = R.jets(B, N, seed=N, n_real=N - N // 3 if N > 2 else None)
    g = torch.Generator().manual_seed(1000 + N)
    labels = (torch.rand(B, N, generator=g) < 0.7).to(torch.uint8)
    return p4, labels


def _stage(p4, code, scale=1.0, labels=None, jet=False, scalars=None, b_pad=B_PAD, alias=False):
    """The raw native call into NaN-filled (mask: 255) buffers.  Returns (p4_in, target, mask, in_scalars, factor)."""
    from lgn import ops
    n, N = p4.shape[0], p4.shape[1]
    Nn, K = N + int(jet), 0 if scalars is None else scalars.shape[-1]
    nan = lambda *s: torch.full(s, float("nan"), device=DEV, dtype=torch.float64)      # noqa: E731
    target = nan(b_pad, N, 4)
    p4_in = target if alias else nan(b_pad, Nn, 4)
    mask = torch.full((b_pad, Nn), 255, device=DEV, dtype=torch.uint8)
    in_scalars = nan(b_pad, Nn, int(jet) + K) if jet or K else None
    factor = nan(b_pad, 4)
    ops.stage_batch(p4.to(DEV), code, p4_in, target, mask, factor, in_scalars, labels=None if labels is None else labels.to(DEV),
                    scalars=None if scalars is None else scalars.to(DEV), scale=scale, jet_features=jet)
    torch.cuda.synchronize()
    return p4_in.cpu(), target.cpu(), mask.cpu(), None if in_scalars is None else in_scalars.cpu(), factor.cpu()


def _check_factor(factor, p4, method, N):
    want = R.factor4(p4, method)
    if R.method_key(method) == "jet_e":
        np.testing.assert_allclose(factor.numpy(), want.numpy(), rtol=2 * max(N - 1, 0) * U53, atol=0, equal_nan=True)
        assert bool((factor == factor[:, :1]).all() | torch.isnan(factor).all())
    else:
        assert np.array_equal(factor.numpy(), want.numpy(), equal_nan=True), "factor of a max method must be bit-equal"


def _check_quotient(target, p4, factor, what):
    want = p4 / factor.unsqueeze(1)
    np.testing.assert_allclose(target.numpy(), want.numpy(), rtol=2.0 ** -52, atol=0, equal_nan=True, err_msg=what)
    same = np.array_equal(target.numpy(), want.numpy(), equal_nan=True)
    print(f"{what}: quotients bit-equal to torch's: {same}")
    return same


@pytest.mark.parametrize("with_labels", [False, True], ids=["nolabels", "labels"])
@pytest.mark.parametrize("scale", [1.0, 0.25])
@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("N", [1, 2, 30, 63, 64, 65, 150, 192])
def test_stage_kernel(N, method, scale, with_labels):
    from lgn.ops import normalize_code
    p4, labels = _inputs(N)
    p4_in, target, mask, in_scalars, factor = _stage(p4, normalize_code(method), scale, labels if with_labels else None)
    assert in_scalars is None
    _check_factor(factor[:B], p4, method, N)
    _check_quotient(target[:B], p4, factor[:B], f"N={N} {method}")
    assert torch.equal(p4_in[:B], target[:B] * scale)
    assert torch.equal(mask[:B], labels if with_labels else (target[:B, :, 0] != 0).to(torch.uint8))
    for t in (p4_in, target, mask, factor):
        assert bool((t[B:] == 0).all()), "padding jets must be written as exact zeros"


def test_stage_kernel_without_normalisation_and_aliased_target():
    """LGN_NORM_NONE: factor one, the batch itself; target and p4_in may be ONE buffer when the scale is 1."""
    from lgn import _native as N_
    p4, _ = _inputs(30)
    for alias in (False, True):
        p4_in, target, mask, _, factor = _stage(p4, N_.NORM_NONE, alias=alias)
        assert torch.equal(target[:B], p4) and torch.equal(p4_in[:B], p4) and bool((factor[:B] == 1).all())
        assert torch.equal(mask[:B], (p4[..., 0] != 0).to(torch.uint8))
        assert bool((target[B:] == 0).all()) and bool((mask[B:] == 0).all()) and bool((factor[B:] == 0).all())


@pytest.mark.parametrize("method", METHODS)
def test_stage_kernel_on_the_reference_inputs(method):
    """g21: the reference's own outputs on a full jet, a padded one, one real row, an all-zero jet, a negative largest entry and a
    jet with one NaN -- which is NaN from end to end while its neighbours are untouched."""
    from lgn.ops import normalize_code
    z = U.load("g21_normalize.npz")
    p4 = torch.from_numpy(z["p4"])
    p4_in, target, mask, _, factor = _stage(p4, normalize_code(method), b_pad=6)
    f_ref, out_ref = z[f"factor.{method}"], z[f"out.{method}"]
    if out_ref.ndim == 4:          # the reference's jet_E: a (B, B, N, 4) table whose diagonal is the per-jet quotient
        f_ref, out_ref = f_ref.reshape(6, 1, 1), np.stack([out_ref[b, b] for b in range(6)])
    f_ref = torch.from_numpy(np.broadcast_to(f_ref, (6, 1, 4)).reshape(6, 4).copy())
    if method == "jet_E":
        np.testing.assert_allclose(factor.numpy(), f_ref.numpy(), rtol=2 * 29 * U53, atol=0, equal_nan=True)
    else:
        assert np.array_equal(factor.numpy(), f_ref.numpy(), equal_nan=True)
    _check_quotient(target, p4, factor, f"g21 {method}")
    np.testing.assert_allclose(target.numpy(), out_ref, rtol=2.0 ** -52 + (2 * 29 * U53 if method == "jet_E" else 0.0), atol=0, equal_nan=True)
    # the NaN (one py entry of jet 5) reaches what the reference lets it reach -- the whole jet under overall_max, the py column under
    # component_max, its own entry under jet_E (assert_allclose above compares the NaN positions) -- and no other jet
    if method == "overall_max":
        assert bool(torch.isnan(factor[5]).all()) and bool(torch.isnan(target[5]).all())
    assert bool(torch.isnan(target[5]).any()) and bool((mask[5] == 1).all())
    assert bool(torch.isfinite(target[:5]).all()) and bool(torch.isfinite(factor[:5]).all())
    assert bool((factor[3] == 1e-16).all()) and bool((target[3] == 0).all()) and bool((mask[3] == 0).all())
    assert np.array_equal(p4_in.numpy(), target.numpy(), equal_nan=True)


@pytest.mark.parametrize("K", [0, 2])
@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("N", [1, 30, 65, 150])
def test_stage_kernel_split_staging(N, method, K):
    """jet_features: jet node, jet-mass scalar and data['scalars'] against Encoder._prepare_input applied to the kernel's own target.
    With A = sum_i |p4_in[i]|_1 per jet: two summation orders of the jet node differ by at most 2 (N - 1) u A; the scalar is normsq4 of
    the doubled jet vector, whose four products and three sums carry that bound to below 64 N 2^-52 A^2."""
    from lgn.models import LGNEncoder
    from lgn.ops import normalize_code
    p4, labels = _inputs(N)
    scale = 0.25
    g = torch.Generator().manual_seed(N + K)
    scalars = torch.randn(B, N + 1, K, generator=g, dtype=torch.float64) if K else None
    p4_in, target, mask, in_scalars, factor = _stage(p4, normalize_code(method), scale, labels, jet=True, scalars=scalars)
    _check_factor(factor[:B], p4, method, N)
    _check_quotient(target[:B], p4, factor[:B], f"split N={N} {method}")
    stub = types.SimpleNamespace(device=torch.device("cpu"), dtype=torch.float64, scale=scale, jet_features=True, tau_input_scalars=2 + K)
    data = {"p4": target[:B], "labels": labels}
    if K:
        data["scalars"] = scalars
    ps, m, sc = LGNEncoder._prepare_input(stub, data)
    assert torch.equal(p4_in[:B, :N], ps[:, :N]) and torch.equal(mask[:B], m)
    A = p4_in[:B, :N].abs().sum(dim=(1, 2))
    jet_err = (p4_in[:B, N] - ps[:, N]).abs().amax(dim=-1)
    assert bool((jet_err <= 2 * (N - 1) * U53 * A).all()), (jet_err, 2 * (N - 1) * U53 * A)
    mass_err = (in_scalars[:B, :, 0] - sc[:, :, 0]).abs().amax(dim=-1)
    assert bool((mass_err <= 64 * N * 2.0 ** -52 * A * A).all()), (mass_err, 64 * N * 2.0 ** -52 * A * A)
    assert bool((in_scalars[:B, :, 0] == in_scalars[:B, :1, 0]).all()), "every node carries the same jet-mass scalar"
    if K:
        assert torch.equal(in_scalars[:B, :, 1:], scalars)
    for t in (p4_in, target, mask, in_scalars, factor):
        assert bool((t[B:] == 0).all())


def test_extra_scalars_without_the_jet_node():
    from lgn.ops import normalize_code
    p4, _ = _inputs(30)
    scalars = torch.randn(B, 30, 3, generator=torch.Generator().manual_seed(3), dtype=torch.float64)
    p4_in, target, mask, in_scalars, _ = _stage(p4, normalize_code("overall_max"), 0.25, scalars=scalars)
    assert torch.equal(in_scalars[:B], scalars) and bool((in_scalars[B:] == 0).all()) and torch.equal(p4_in[:B], target[:B] * 0.25)


@pytest.mark.parametrize("N", [1, 30, 65])
def test_denormalize_is_the_torch_product(N):
    from lgn import ops
    g = torch.Generator().manual_seed(N)
    x0, x1 = (torch.randn(B, N, 4, generator=g, dtype=torch.float64).to(DEV) for _ in range(2))
    f = torch.rand(B, 4, generator=g, dtype=torch.float64).to(DEV) * 100
    o0, o1 = torch.full_like(x0, float("nan")), torch.full_like(x1, float("nan"))
    ops.denormalize(f, x0, o0, x1, o1)
    assert torch.equal(o0, x0 * f.unsqueeze(1)) and torch.equal(o1, x1 * f.unsqueeze(1))
    o0.fill_(float("nan"))
    ops.denormalize(f, x0, o0)
    assert torch.equal(o0, x0 * f.unsqueeze(1))


@pytest.mark.parametrize("method", METHODS + ["Overall-Max", "jet e", "bogus"])
def test_ops_normalize_p4_is_the_drop_in(method):
    from lgn.ops import normalize_p4
    z = U.load("g21_normalize.npz")
    p4 = torch.from_numpy(z["p4"])[:5]          # (without the NaN jet: values are compared below)
    out, f = normalize_p4(p4.to(DEV), method)
    want, f_want = R.normalize_p4(p4, method)
    assert tuple(f.shape) == tuple(f_want.shape) == ((5, 1, 4) if method == "component_max" else (5, 1, 1))
    assert tuple(out.shape) == (5, 30, 4)
    jet_e = R.method_key(method) == "jet_e"
    np.testing.assert_allclose(f.cpu().numpy(), f_want.numpy(), rtol=2 * 29 * U53 if jet_e else 0.0, atol=0)
    np.testing.assert_allclose(out.cpu().numpy(), want.numpy(), rtol=2.0 ** -52 + (2 * 29 * U53 if jet_e else 0.0), atol=0)
    out4, f4 = normalize_p4(p4.reshape(1, 5, 30, 4).to(DEV), method)          # leading axes are kept
    assert tuple(out4.shape) == (1, 5, 30, 4) and tuple(f4.shape) == (1,) + tuple(f.shape) and torch.equal(out4[0], out)


# ---- the steps ---------------------------------------------------------------------------------------------------------------
CH = {2: ((3, 3, 4, 4), (4, 4, 3, 3)), 3: ((2, 3, 4), (4, 3, 2))}
STEP_CASES = [(2, 7, 30, 1.0), (2, 7, 30, 0.25), (3, 3, 12, 1.0)]


def _pair(maxdim, N, scale, n=2, **kw):
    """n pairs of networks on identical initial weights."""
    import __graft_entry__ as G
    nets = [G._models(N, CH[maxdim][0], CH[maxdim][1], torch.device(DEV), seed=17, maxdim=maxdim, **kw) for _ in range(n)]
    for enc, _ in nets:
        enc.scale = scale
    return nets


def _raw(Bn, N, seed):
    return R.jets(Bn, N, seed=seed, n_real=N - N // 4).to(DEV)


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("maxdim,Bn,N,scale", STEP_CASES)
def test_train_step_with_normalize_is_the_plain_step_on_the_staged_batch(maxdim, Bn, N, scale, method):
    from lgn.step import NativeTrainStep
    (ea, da), (eb, db) = _pair(maxdim, N, scale)
    a = NativeTrainStep(ea, da, batch_size=Bn, lr=1e-3, normalize=True, normalize_method=method)
    b = NativeTrainStep(eb, db, batch_size=Bn, lr=1e-3)
    assert not a.split and a.normalize and not b.normalize and bool((b.norm_factor == 1).all())
    for it in range(2):
        p4 = _raw(Bn, N, seed=40 + it)
        a.load_batch({"p4": p4})
        assert torch.equal(a.norm_factor.cpu(), R.factor4(p4.cpu(), method)) or method == "jet_E"
        la, ra = a.step()
        lb, rb = b.step({"p4": a.target.clone(), "labels": a.mask.clone()})
        assert torch.equal(la, lb) and torch.equal(ra, rb), f"step {it}"
    assert torch.equal(a.flat.flat, b.flat.flat)


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("maxdim,Bn,N,scale", STEP_CASES)
def test_eval_step_with_normalize(maxdim, Bn, N, scale, method):
    """Graph replays on two different batches and a short batch of 5 of 7 (2 of 3): loss and reconstruction are the plain step's on
    the staged batch; recon_denorm / target_denorm are the products with the factors; norm_factors has the reference's shape."""
    from lgn.step import NativeEvalStep
    (ea, da), (eb, db) = _pair(maxdim, N, scale)
    a = NativeEvalStep(ea, da, batch_size=Bn, use_graph=True, normalize=True, normalize_method=method)
    b = NativeEvalStep(eb, db, batch_size=Bn, use_graph=True)
    assert "recon_denorm" not in b.run({"p4": _raw(Bn, N, seed=1)})
    for it, n in enumerate((Bn, Bn, Bn - 2 if Bn > 3 else Bn - 1)):
        p4 = _raw(Bn, N, seed=50 + it)[:n]
        out = a.run({"p4": p4})
        ref = b.run({"p4": a.target[:n].clone(), "labels": a.mask[:n].clone()})
        assert torch.equal(out["loss"], ref["loss"]) and torch.equal(out["recon"], ref["recon"]), f"run {it}"
        f = a.norm_factor[:n]
        assert torch.equal(out["recon_denorm"], out["recon"] * f.unsqueeze(1))
        assert torch.equal(out["target_denorm"], a.target[:n] * f.unsqueeze(1))
        assert tuple(out["norm_factors"].shape) == ((n, 1, 4) if method == "component_max" else (n, 1, 1))
        assert torch.equal(out["norm_factors"].expand(n, 1, 4).reshape(n, 4), f)
        # (p / f) * f: two roundings, each within 2^-53 relative -> the batch comes back to within 2^-52 (1 + 2^-53) < 2^-51
        np.testing.assert_allclose(out["target_denorm"].cpu().numpy(), p4.cpu().numpy(), rtol=2.0 ** -51, atol=0)
        assert bool((a.target[n:] == 0).all()) and bool((a.mask[n:] == 0).all())


@pytest.mark.parametrize("method", METHODS)
def test_split_step_with_normalize_matches_the_reference_loop_step(method):
    """jet_features at maxdim 2 (the split staging: jet node and jet-mass scalar from the kernel) against ReferenceLoopStep, whose
    encoder prepares its own input from the normalised batch; tolerances of the native step against the module path."""
    from lgn.step import NativeTrainStep, ReferenceLoopStep
    Bn, N = 5, 30
    (ea, da), (eb, db) = _pair(2, N, 0.5, jet_features=True)
    a = NativeTrainStep(ea, da, batch_size=Bn, optimizer=False, normalize=True, normalize_method=method)
    assert a.split
    b = ReferenceLoopStep(eb, db, optimizer=False, normalize=True, normalize_method=method)
    batch = {"p4": _raw(Bn, N, seed=60)}
    for _ in range(2):
        la, ra = a.step(batch)
    lb, rb = b.step(batch)
    U.assert_close(la, lb, 1e-12, "loss")
    U.assert_close(ra, rb, 1e-12, "recon")
    U.assert_close(a.flat.grad, torch.cat([eb.flat_params.grad, db.flat_params.grad]), 1e-9, "flat gradient")
    assert torch.equal(a.norm_factor, b.norm_factor)


@pytest.mark.parametrize("method", METHODS)
def test_module_steps_with_normalize_match_the_native_steps(method):
    from lgn.step import CapturedModuleStep, ModuleEvalStep, NativeEvalStep, NativeTrainStep, TrainStep
    Bn, N = 5, 30
    nets = _pair(2, N, 1.0, n=5)
    batch = {"p4": _raw(Bn, N, seed=70)}
    kw = dict(normalize=True, normalize_method=method)
    a = NativeTrainStep(*nets[0], batch_size=Bn, optimizer=False, **kw)
    la, ra = a.step(batch)
    c = CapturedModuleStep(*nets[1], batch_size=Bn, optimizer=False, use_graph=True, **kw)
    for _ in range(2):
        lc, rc = c.step(batch)
    t = TrainStep(*nets[2], optimizer=False, **kw)
    lt, rt = t.forward_backward(batch)
    for what, l, r, g in (("captured", lc, rc, c.flat.grad), ("TrainStep", lt, rt, t.flat.grad)):
        U.assert_close(l, la, 1e-12, f"{what}: loss")
        U.assert_close(r, ra, 1e-12, f"{what}: recon")
        U.assert_close(g, a.flat.grad, 1e-9, f"{what}: flat gradient")
    assert torch.equal(c.norm_factor, a.norm_factor) and torch.equal(t.norm_factor, a.norm_factor)
    ne = NativeEvalStep(*nets[3], batch_size=Bn, **kw).run(batch)
    me = ModuleEvalStep(*nets[4], batch_size=Bn, **kw).run(batch)
    for k in ("loss", "recon", "recon_denorm"):
        U.assert_close(me[k], ne[k], 1e-12, f"ModuleEvalStep {k}")
    assert torch.equal(me["target_denorm"], ne["target_denorm"]) and torch.equal(me["norm_factors"], ne["norm_factors"])


@pytest.mark.parametrize("kind", ["native", "eval", "loop"])
@pytest.mark.parametrize("method", METHODS)
def test_steps_match_the_reference_loop_golden(method, kind):
    """g21_step_normalize_maxdim2: the reference's train() loop body under --normalize on raw jets -- its loss (no regularisation
    term), p4_recons * norm_factor and norm_factor; tolerance of the golden end-to-end fixtures."""
    import __graft_entry__ as G
    from lgn.step import NativeEvalStep, NativeTrainStep, ReferenceLoopStep, get_real
    z = U.load("g21_step_normalize_maxdim2.npz")
    m = U.meta(z)
    dev = torch.device(DEV)
    enc, dec = G._models(m["N"], m["ch_enc"], m["ch_dec"], dev, seed=m["seed"], maxdim=m["maxdim"])
    batch = {"p4": torch.from_numpy(z["p4"]).to(dev)}
    kw = dict(get_real_method="real", normalize=True, normalize_method=method)
    if kind == "eval":
        out = NativeEvalStep(enc, dec, m["B"], **kw).run(batch)
        loss, denorm, f = out["loss"], out["recon_denorm"], out["norm_factors"]
        assert tuple(f.shape) == z[f"norm_factor.{method}"].shape
    else:
        step = NativeTrainStep(enc, dec, m["B"], l1_lambda=0.0, optimizer=False, **kw) if kind == "native" else \
            ReferenceLoopStep(enc, dec, l1_lambda=0.0, optimizer=False, **kw)
        loss, recon = step.step(batch)
        f = step.norm_factor
        denorm = get_real(recon, "real") * f.unsqueeze(1)
    f_ref = np.broadcast_to(z[f"norm_factor.{method}"], (m["B"], 1, 4)).reshape(m["B"], 4)
    U.assert_close(f.expand(m["B"], 1, 4).reshape(m["B"], 4) if f.dim() == 3 else f, f_ref, 1e-11, "norm_factor")
    U.assert_close(loss, z[f"loss.{method}"], 1e-11, "loss")
    U.assert_close(denorm, z[f"recon_denorm.{method}"], 1e-11, "p4_recons * norm_factor")
