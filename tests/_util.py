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
    state_dict order) to every state_dict tensor and loads the result back.  Returns the two CPU dicts (what the oracle gets)."""
    g = torch.Generator().manual_seed(seed)
    out = []
    for mod in (enc, dec):
        sd = {k: v.detach().cpu().clone() for k, v in mod.state_dict().items()}
        for k, v in sd.items():
            v.add_(sigma * torch.randn(v.shape, dtype=v.dtype, generator=g))
        mod.load_state_dict(sd)
        out.append(sd)
    return out[0], out[1]


def oracle_step(O, Pe, Pd, cfg_enc, cfg_dec, p4, labels, l1_lambda=0.0):
    """One step of the oracle on the CPU with Pe / Pd themselves as the leaf tensors: encoder, decoder, Chamfer loss (+ l1_lambda *
    sum |w|, as the reference's loop adds it), backward.  Returns (loss, recon, {'enc.<name>' / 'dec.<name>': gradient})."""
    for P in (Pe, Pd):
        for v in P.values():
            v.requires_grad_(True)
            v.grad = None
    rec = O.decoder_forward(Pd, cfg_dec, O.encoder_forward(Pe, cfg_enc, p4, labels))
    loss = O.chamfer_loss(O.get_real(rec, "sum"), p4)
    if l1_lambda:
        loss = loss + l1_lambda * (O.l1_norm(Pe) + O.l1_norm(Pd))
    loss.backward()
    grads = {f"{pre}.{k}": v.grad for pre, P in (("enc", Pe), ("dec", Pd)) for k, v in P.items()}
    return loss.detach(), rec.detach(), grads


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
