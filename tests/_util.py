"""Helpers shared by the tests: golden-fixture loading, tolerance helpers."""
import ast
import hashlib
import json
import os

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


def load(name):
    return np.load(os.path.join(GOLDEN, name), allow_pickle=False)


def rep_from(npz, prefix):
    """Rebuild an ordered {(k,n): tensor} from the '<prefix>.__keys__' + '<prefix>.(k, n)' entries."""
    keys = [tuple(k) for k in json.loads(str(npz[prefix + ".__keys__"]))]
    return {k: torch.from_numpy(npz[f"{prefix}.{k}"]) for k in keys}


def params_from(npz, prefix):
    out = {}
    for name in npz.files:
        if name.startswith(prefix + "."):
            out[name[len(prefix) + 1:]] = torch.from_numpy(npz[name])
    return out


def meta(npz):
    return json.loads(str(npz["meta"]))


def sha(bufs):
    """{name: sha256 of the tensor's bytes} of device buffers, after the device has finished: the bit-for-bit pins"""
    torch.cuda.synchronize()
    return {k: hashlib.sha256(np.ascontiguousarray(v.detach().cpu().numpy()).tobytes()).hexdigest() for k, v in bufs.items()}


def relerr(a, b):
    a = torch.as_tensor(a, dtype=torch.float64)
    b = torch.as_tensor(b, dtype=torch.float64)
    denom = b.abs().max().item()
    return (a - b).abs().max().item() / (denom if denom > 0 else 1.0)


def assert_close(a, b, tol, what=""):
    a = torch.as_tensor(a); b = torch.as_tensor(b)
    assert tuple(a.shape) == tuple(b.shape), f"{what}: shape {tuple(a.shape)} vs {tuple(b.shape)}"
    e = relerr(a.detach().cpu(), b.detach().cpu())
    assert e <= tol, f"{what}: rel err {e:.3e} > {tol:.1e}"
    return e


def assert_close_scaled(a, b, tol, scale, what=""):
    """|a - b|max <= tol * max(|b|max, scale): for gradients whose own magnitude is far below the network's gradient scale
    (rounding noise of the sums they come from is absolute, not relative to the survivor of a cancellation)."""
    a = torch.as_tensor(a, dtype=torch.float64).detach().cpu(); b = torch.as_tensor(b, dtype=torch.float64).detach().cpu()
    assert tuple(a.shape) == tuple(b.shape), f"{what}: shape {tuple(a.shape)} vs {tuple(b.shape)}"
    err, ref = (a - b).abs().max().item(), max(b.abs().max().item(), scale)
    assert err <= tol * ref, f"{what}: abs err {err:.3e} > {tol:.1e} * {ref:.3e}"
    return err / ref


ROUNDING = 64 * 2.2e-16       # absolute differences below this x the step's largest gradient entry are rounding of that entry's scale


def named_grads(enc, dec):
    """[('enc.<name>', gradient), ..., ('dec.<name>', gradient), ...] of the two networks, in state_dict order."""
    return [(f"{pre}.{k}", g) for pre, mod in (("enc", enc), ("dec", dec)) for k, g in mod.named_grads()]


def assert_named_grads_close(named_got, ref, tol, what="", scaled=(), add=None, max_floor_routed=None):
    """Every gradient tensor of a step against ITS OWN largest entry.  named_got: (name, tensor) pairs; ref: {name: tensor or None}
    of the same names; add: {name: tensor} of terms the result carries on top of ref (the L1 sub-gradient).

    * A reference gradient that is exactly zero (or None) requires exactly zero (exactly add[name]) as the result.
    * A tensor whose own maximum is below 1e-4 of the step's largest gradient entry may differ by a few roundings OF THAT LARGEST
      entry (ROUNDING x step max, absolute) whatever that is relative to itself; a tensor that needs this floor while being within
      1e4 of the largest gradient is a regression, not rounding, and fails the strict check.
    * The names in `scaled` are survivors of a cancellation: held to tol of 1 % of the step's largest gradient instead.
    Every tensor that did not pass the strict per-tensor check is printed (pytest -s / -rA), so that a drift stays visible.
    max_floor_routed: the most tensors the absolute floor may decide.  Returns (worst relative error of the strictly checked
    tensors, its name)."""
    named_got, add = list(named_got), add or {}
    assert sorted(n for n, _ in named_got) == sorted(ref), f"{what}: gradient names differ from the reference's"
    cpu = lambda t: torch.as_tensor(t, dtype=torch.float64).detach().cpu()      # noqa: E731
    top = max([float(cpu(r).abs().max()) for r in ref.values() if r is not None and torch.as_tensor(r).numel()] + [0.0])
    routed, worst, worst_name = [], 0.0, None
    for name, got in named_got:
        r, extra = ref[name], add.get(name)
        if r is None or float(cpu(r).abs().max()) == 0:
            if extra is None:
                assert got is None or float(cpu(got).abs().max()) == 0, f"{what}: {name} must have exactly zero gradient"
            else:
                assert got is not None and torch.equal(cpu(got), cpu(extra)), f"{what}: {name}: dead parameter must get exactly the added term"
            continue
        assert got is not None, f"{what}: {name} has no gradient"
        got, r = cpu(got), cpu(r) if extra is None else cpu(r) + cpu(extra)
        assert tuple(got.shape) == tuple(r.shape), f"{what}: grad {name}: shape {tuple(got.shape)} vs {tuple(r.shape)}"
        err, own = (got - r).abs().max().item(), r.abs().max().item()
        if name in scaled:
            assert_close_scaled(got, r, tol, 1e-2 * top, f"{what}: grad {name}")
            routed.append((name, "the scaled list", err, own))
        elif err > tol * own and err <= ROUNDING * top and own < 1e-4 * top:
            routed.append((name, "ROUNDING floor", err, own))
        else:
            assert err <= tol * own, f"{what}: grad {name}: rel err {err / own:.3e} > {tol:.1e} (own max {own:.3e}, step max {top:.3e})"
            if err / own > worst or worst_name is None:
                worst, worst_name = err / own, name
    for name, route, err, own in routed:
        print(f"[{what}] grad {name}: passed by {route}: abs err {err:.3e}, own max {own:.3e} (rel {err / own:.3e}), step max {top:.3e}")
    floor_routed = [name for name, route, _, _ in routed if route == "ROUNDING floor"]
    if max_floor_routed is not None:
        assert len(floor_routed) <= max_floor_routed, f"{what}: {len(floor_routed)} tensors decided by the absolute floor: {floor_routed}"
    return worst, worst_name


def live_weights(enc, dec, sigma=0.1, seed=77):
    """Moves both networks off their initial weights, where the reconstruction is ~1e-9 and a third of the gradient tensors lie four
    or more orders below the largest: adds sigma * randn (ONE generator: the encoder's tensors first, then the decoder's, in
    state_dict order) to every state_dict tensor and loads the result back.  Returns the two CPU dicts (what the oracle gets).
    sigma: a number, or ((name part, sigma), ...) -- the LAST pair whose part occurs in the tensor's name decides ('enc.<name>' / 'dec.<name>'; '' matches
    every name) -- for a net whose tensors need different steps to come alive (the draws themselves do not depend on sigma)."""
    g = torch.Generator().manual_seed(seed)
    pairs = sigma if isinstance(sigma, (tuple, list)) else (("", sigma),)
    out = []
    for pre, mod in (("enc.", enc), ("dec.", dec)):
        sd = {k: v.detach().cpu().clone() for k, v in mod.state_dict().items()}
        for k, v in sd.items():
            v.add_([s for part, s in pairs if part in pre + k][-1] * torch.randn(v.shape, dtype=v.dtype, generator=g))
        mod.load_state_dict(sd)
        out.append(sd)
    return out[0], out[1]


def jet_mse(x, y):
    """nn.MSELoss()(x.sum(-2), y.sum(-2)) (utils/losses/chamfer_loss/chamfer_loss.py:25-29): all rows, padding included."""
    return ((x.sum(-2) - y.sum(-2)) ** 2).mean()


def chamfer_per_jet(x, y):
    """The per-jet terms (B,) of O.chamfer_loss: their sum is that loss."""
    dist = torch.sum((x.unsqueeze(-2) - y.unsqueeze(-3)) ** 2, dim=-1)
    return (dist.min(dim=-1).values + dist.min(dim=-2).values).sum(-1) / 2


def oracle_forward(O, Pe, Pd, cfg_enc, cfg_dec, p4, labels, extra_scalars=None):
    """The oracle's networks on the CPU with Pe / Pd themselves as the leaf tensors (their .grad cleared).  Returns (recon with its
    graph, pooled latent, the features the latent map pooled: {irrep: (2, B, N, T, d)})."""
    for P in (Pe, Pd):
        for v in P.values():
            v.requires_grad_(True)
            v.grad = None
    seen, pool = [], O.aggregate_latent

    def spy(method, latent):
        if not seen:                                  # (the '&' / '+' maps call themselves again on the same features)
            seen.append({k: v.detach() for k, v in latent.items()})
        return pool(method, latent)

    O.aggregate_latent = spy
    try:
        lat = O.encoder_forward(Pe, cfg_enc, p4, labels, extra_scalars=extra_scalars)
    finally:
        O.aggregate_latent = pool
    return O.decoder_forward(Pd, cfg_dec, lat), lat, seen[0]


def oracle_loss(O, Pe, Pd, rec, target, l1_lambda=0.0, *, get_real="sum", jet_term=False, loss_fn=None, jet_weights=None,
                l2_lambda=0.0):
    """The loss of a step on the oracle's reconstruction `rec` (with its graph), the options as oracle_step names them."""
    x = O.get_real(rec, get_real)
    if loss_fn is not None:
        loss = loss_fn(x, target)
    elif jet_weights is not None:
        loss = chamfer_per_jet(x, target)
    else:
        loss = O.chamfer_loss(x, target)
    if jet_weights is not None:
        assert loss.dim() == 1, "per-jet weights need per-jet terms"
        loss = (loss * jet_weights.to(loss.dtype)).sum()
    elif loss.dim():
        loss = loss.sum()
    if jet_term:
        assert jet_weights is None
        loss = loss + jet_mse(x, target)
    if l1_lambda:
        loss = loss + l1_lambda * (O.l1_norm(Pe) + O.l1_norm(Pd))
    if l2_lambda:
        loss = loss + l2_lambda * sum((v * v).sum() for P in (Pe, Pd) for v in P.values())
    return loss


def oracle_backward(loss, Pe, Pd, retain_graph=False):
    """loss.backward() into the leaves' .grad (cleared first).  Returns {'enc.<name>' / 'dec.<name>': gradient or None}; with
    retain_graph -- a forward shared by several losses -- the gradients are copies, so that the next backward leaves them alone."""
    for P in (Pe, Pd):
        for v in P.values():
            v.grad = None
    loss.backward(retain_graph=retain_graph)
    keep = (lambda g: None if g is None else g.clone()) if retain_graph else (lambda g: g)
    return {f"{pre}.{k}": keep(v.grad) for pre, P in (("enc", Pe), ("dec", Pd)) for k, v in P.items()}


def oracle_step(O, Pe, Pd, cfg_enc, cfg_dec, p4, labels, l1_lambda=0.0, *, get_real="sum", jet_term=False, loss_fn=None,
                jet_weights=None, extra_scalars=None, target=None, l2_lambda=0.0, with_latent=False):
    """One step of the oracle on the CPU with Pe / Pd themselves as the leaf tensors: encoder, decoder, Chamfer loss (+ l1_lambda *
    sum |w| + l2_lambda * sum w^2, as the reference's loop adds them), backward.  Returns (loss, recon, {'enc.<name>' /
    'dec.<name>': gradient}).

    get_real: the --get-real-method.  jet_term: + the jet-feature MSE (jet_mse).  loss_fn: (x, target) -> per-jet terms (B,) or a
    scalar, in place of Chamfer.  jet_weights (B,): the loss is sum_b w_b term_b -- the loss of a batch that holds jet b w_b times
    (Chamfer's per-jet terms unless loss_fn gives its own).  extra_scalars: data['scalars'] of the encoder.  p4 is what the ENCODER
    is given (it applies cfg_enc.scale itself); target is what the loss compares with, p4 unless given (--normalize: the
    normalised batch goes to both, the encoder's scale to the input alone).  with_latent: returns (loss, recon, grads, pooled
    latent, the features the latent map pooled) instead."""
    rec, lat, feats = oracle_forward(O, Pe, Pd, cfg_enc, cfg_dec, p4, labels, extra_scalars)
    loss = oracle_loss(O, Pe, Pd, rec, p4 if target is None else target, l1_lambda, get_real=get_real, jet_term=jet_term,
                       loss_fn=loss_fn, jet_weights=jet_weights, l2_lambda=l2_lambda)
    grads = oracle_backward(loss, Pe, Pd)
    if with_latent:
        return loss.detach(), rec.detach(), grads, {k: v.detach() for k, v in lat.items()}, feats
    return loss.detach(), rec.detach(), grads


def _runner_up_gap(score, dim):
    """Relative gap (best - next DISTINCT value) / scale along dim, for the minimum of score; +inf where every value is equal."""
    s = score.sort(dim=dim).values.movedim(dim, -1)
    best = s[..., :1]
    nxt = torch.where(s > best, s, torch.full_like(s, float("inf"))).min(-1).values
    best = best.squeeze(-1)
    gap = (nxt - best) / torch.maximum(nxt.abs(), best.abs()).clamp_min(1e-300)
    return torch.where(torch.isinf(nxt), torch.full_like(gap, float("inf")), gap)


def assert_live(O, rec_o, grads_o, p4, x_o, chamfer=True, pooled=None, latent_map="", mask=None):
    """Conditions on a case's INPUTS, decided on the oracle's outputs alone before anything is compared with them:

    * the reconstruction is finite and 1e-3 <= max |rec| <= 1e3 (the networks do something, and nothing overflows on the way);
    * at most 10 % of the tensors with a non-zero reference gradient lie below 1e-4 of the step's largest gradient entry (those
      are the ones the absolute floor of assert_named_grads_close may decide) -- the count is returned: the case's max_floor_routed;
    * chamfer: for every reconstructed particle and every REAL target particle, nearest and second-nearest distinct partner differ
      by >= 1e-8 relative (zero-padded target rows are identical: ties among them select the same value and are skipped) -- a kernel
      that sums the distance in another order must still find the oracle's partner;
    * a latent map with 'min' / 'max' (pooled = the features it pools): the same gap for the pooling score of every channel.  The
      masked particles of a jet (mask (B, N), p4[..., 0] != 0 unless given; nodes beyond N -- the jet node -- are real) carry one and
      the same feature in exact arithmetic, computed with whatever rounding the host's matrix products give each row: they count
      as ONE candidate, whichever of them wins the value is the same."""
    top = float(rec_o.abs().max())
    assert bool(torch.isfinite(rec_o).all()) and 1e-3 <= top <= 1e3, f"the weights are not live: max |recon| {top:.3e}"
    low = 0
    if grads_o is not None:                        # (None: a forward-only case)
        own = [float(g.abs().max()) for g in grads_o.values() if g is not None and g.numel() and float(g.abs().max()) > 0]
        assert own and all(o == o and o != float("inf") for o in own), "non-finite reference gradient"
        low = sum(o < 1e-4 * max(own) for o in own)
        assert low <= 0.10 * len(own), f"{low} of {len(own)} live gradient tensors lie below 1e-4 of the largest"
    if chamfer:
        dist = torch.sum((x_o.unsqueeze(-2) - p4.unsqueeze(-3)) ** 2, dim=-1)           # (B, N rec, N target)
        real = p4[..., 0] != 0
        gap_rec = _runner_up_gap(dist, -1)
        gap_tgt = _runner_up_gap(dist, -2)[real]
        gap = min(float(gap_rec.min()), float(gap_tgt.min()) if gap_tgt.numel() else float("inf"))
        assert gap >= 1e-8, f"Chamfer partners nearly tied: relative gap {gap:.3e}"
    m = latent_map.lower()
    if pooled is not None and ("min" in m or "max" in m):
        masked = ~(p4[..., 0] != 0 if mask is None else mask.bool())
        spare = masked & (torch.cumsum(masked.long(), dim=-1) > 1)                      # every masked particle of a jet but its first
        for key, f in pooled.items():
            msq = O._msq(f) if f.shape[-1] > 1 else None
            scores = []
            if "max" in m:
                scores.append(-(msq if msq is not None else O._msq(f)))
            if "min" in m:
                scores.append(msq if msq is not None else f.min(dim=-1).values)
            for s in scores:                           # (2, B, N, T): the particle axis is -2
                drop = torch.zeros(s.shape[1:3], dtype=torch.bool)
                drop[:, :spare.shape[1]] = spare
                s = s.masked_fill(drop.unsqueeze(0).unsqueeze(-1), float("inf"))
                gap = float(_runner_up_gap(s, -2).min())
                assert gap >= 1e-8, f"pooling scores of {key} nearly tied: relative gap {gap:.3e}"
    return low


def tiled_jets(B, N, K=7, seed=0):
    """A batch of B jets made of K distinct padded jets laid out cyclically (jet b = distinct jet b % K).  Returns (p4 (B, N, 4),
    labels (B, N), the K jets, their labels, copies (K,): how often each occurs).  A loss that is a sum over jets is then sum_k
    copies_k term_k of the K jets, gradient included; K = 7 is coprime to every power of two, so a kernel that reads a neighbour's
    jet at an offset of 1, 2, 4 .. 512 lands on other data."""
    from oracle import lgn_oracle as O
    import _jets
    p4, labels = O.synthetic_jets(K, N, seed=seed, pad=True)
    tiled, tiled_labels, copies = _jets.tile(p4, labels, B)
    return tiled, tiled_labels, p4, labels, copies


def assert_rep_close(rep, ref, tol, what="", check_order=True):
    if check_order:
        assert list(rep.keys()) == list(ref.keys()), f"{what}: key order {list(rep.keys())} vs {list(ref.keys())}"
    else:
        assert set(rep.keys()) == set(ref.keys())
    for k in ref.keys():
        assert_close(rep[k], ref[k], tol, f"{what}{k}")


class OracleNet:
    """Gives the oracle (CPU restatement of the reference) the module call shape the equivariance harness expects."""

    def __init__(self, O, P, cfg, decoder, cg, maxdim=2):
        self.O, self.P, self.cfg, self.decoder = O, P, cfg, decoder
        self.maxdim, self.device, self.dtype, self.cg_dict = maxdim, torch.device("cpu"), torch.float64, cg

    def eval(self):
        return self

    def __call__(self, data, covariance_test=False, nodes_all=None):
        O = self.O
        if not self.decoder:
            return O.encoder_forward(self.P, self.cfg, data["p4"], data.get("labels"), covariance_test=True)
        gen, nodes = O.decoder_forward(self.P, self.cfg, data, covariance_test=True)
        return gen, list(nodes_all) + nodes
