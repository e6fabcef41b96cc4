"""Whole training steps at LIVE weights against the oracle, per gradient tensor.

At the reference's initial weights the network does almost nothing: the reconstruction is ~1e-9 of the input, the loss is sum |p|^2 to
eleven digits whatever the kernels do, and a third (maxdim 2) to two thirds (maxdim 3) of the gradient tensors lie four or more orders
below the step's largest gradient.  U.live_weights adds 0.1 * randn to every state_dict tensor: reconstructions of O(0.01) .. O(1000),
at most 6 of ~100 live gradient tensors below 1e-4 of the largest, none below 1e-6.  Every case is the smallest shape that enters the
launch regime it names; the reference of every case is the oracle on the CPU (0.1 .. 5.5 s), loss / Chamfer part / reconstruction at
FWD_TOL and every gradient tensor against its own largest entry at GRAD_TOL (U.assert_named_grads_close).

Gradient tensors with a measured tolerance: none.

Parameter tensors with a measured tolerance in test_native_adam_live_weights_follows_oracle (_ADAM_CONDITIONING below), maxdim 3,
B = 5, N = 13, (2,4,7,8)/(8,6,5,3).  The (0, 2) and (2, 0) mixing weights of these levels hold entries whose Chamfer gradient is zero
in exact arithmetic: their gradient is the L1 term, 1e-8, plus the rounding noise of the sums (1e-13 absolute, 1e-15 of the tensor's
largest gradient).  Adam's update lr m / (sqrt(v) + eps) with eps = 1e-8 is at its steepest there -- d(update) / dg = lr / 4e-8 -- so
noise of 1e-13 moves a weight by 1e-9 per step, in the oracle as on the GPU.  The oracle against ITSELF with the particles of every
jet in reverse order (labels included; the exact gradients are equal), three Adam steps, relative to the tensor's largest weight:

    dec.lgn_cg.node_levels.1.cat_mix.mix_reps.weights.(0, 2)    3.57e-08
    dec.lgn_cg.node_levels.1.cat_mix.mix_reps.weights.(2, 0)    1.72e-08
    dec.lgn_cg.node_levels.0.cat_mix.mix_reps.weights.(2, 0)    9.65e-09
    dec.lgn_cg.node_levels.0.cat_mix.mix_reps.weights.(0, 2)    7.98e-09

(every other tensor but the two named next: 1.3e-15 or less; enc.lgn_cg.node_levels.1 ... (2, 0) 2.55e-10 and (0, 2) 1.71e-10 keep the
1e-9).  The listed tensors are held to 100 x their figure -- the GPU changes the order of every sum, not of one -- and their gradients
are held to GRAD_TOL like every other tensor's by test_native_step_live_weights_matches_oracle on the same case."""
import pytest
import torch

import _util as U

pytestmark = pytest.mark.gpu

FWD_TOL = 1e-11
GRAD_TOL = 1e-9
MAX_FLOOR_ROUTED = 6          # the oracle alone has at most 6 of ~100 tensors under 1e-4 of the step's largest at these weights

CFG2 = ((3, 3, 4, 4), (4, 4, 3, 3))
CFG5 = ((4, 4, 6, 6), (6, 6, 4, 4))
WIDE = ((2, 4, 7, 8), (8, 6, 5, 3))

# {(maxdim, B, N, num_basis_fn): {parameter tensor: the oracle's disagreement with itself after three Adam steps}}: see the head of the file
_ADAM_CONDITIONING = {(3, 5, 13, 10): {"dec.lgn_cg.node_levels.1.cat_mix.mix_reps.weights.(0, 2)": 3.57e-08,
                                       "dec.lgn_cg.node_levels.1.cat_mix.mix_reps.weights.(2, 0)": 1.72e-08,
                                       "dec.lgn_cg.node_levels.0.cat_mix.mix_reps.weights.(2, 0)": 9.65e-09,
                                       "dec.lgn_cg.node_levels.0.cat_mix.mix_reps.weights.(0, 2)": 7.98e-09}}


def _setup(maxdim, B, N, che, chd, num_basis_fn=10):
    """Networks at live weights on the GPU, the same weights as CPU dicts, the oracle's two configurations and a padded batch."""
    import __graft_entry__ as G
    from oracle import lgn_oracle as O
    dev = torch.device("cuda:0")
    enc, dec = G._models(N, che, chd, dev, seed=3, maxdim=maxdim, num_basis_fn=num_basis_fn)
    Pe, Pd = U.live_weights(enc, dec)
    ce = O.NetConfig(num_particles=N, num_channels=tuple(che), maxdim=maxdim, num_basis_fn=num_basis_fn)
    cd = O.NetConfig(num_particles=N, num_channels=tuple(chd), maxdim=maxdim, num_basis_fn=num_basis_fn)
    p4, labels = O.synthetic_jets(B, N, seed=B + N, pad=True)
    return O, dev, enc, dec, Pe, Pd, ce, cd, p4, labels


@pytest.mark.parametrize("maxdim,B,N,chans", [
    (2, 130, 30, CFG2),      # jet split 2 (129 .. 256 jets), 16-row chain CGMLP with kept activations
    (2, 272, 30, CFG2),      # one workgroup per jet with the symmetric sweep; 64-row two-role chain CGMLP (>= 8129 rows); 240-row tail partials
    (3, 19, 30, CFG5),       # 9 node tiles and 10 jet pairs: the second XCD group with padding ids, odd B
    (3, 5, 13, WIDE),        # both table kinds x COT 4 / 6 / 8, jets cut by tiles, last tile partly empty
    (3, 7, 21, ((1, 5, 6), (6, 5, 1))),      # one-channel ends, C = 5
    (3, 1, 32, ((3, 4), (4, 3))),            # single jet, full half-wave, lone jet of a pair
    (3, 3, 33, ((3, 4, 4), (4, 4, 3))),      # first N off the static path: node-major layouts, run-time tables
    (3, 2, 65, ((3, 4, 4), (4, 4, 3)))])     # first N beyond the tile-blocked separable decoder kernels (N <= 64)
def test_native_step_live_weights_matches_oracle(maxdim, B, N, chans):
    """The graph-replayed whole-step call (what the chooser takes) at live weights: total loss, Chamfer part, reconstruction and
    every named gradient (+ the L1 sub-gradient the step adds) against the oracle."""
    from lgn.step import NativeTrainStep, native_train_step
    O, dev, enc, dec, Pe, Pd, ce, cd, p4, labels = _setup(maxdim, B, N, *chans)
    lam = 1e-8
    step = native_train_step(enc, dec, B, l1_lambda=lam, optimizer=False, use_graph=True)
    assert isinstance(step, NativeTrainStep), "the chooser must take the whole-step call for this configuration"
    batch = {"p4": p4.to(dev), "labels": labels.to(dev)}
    for _ in range(2):                      # second iteration = graph replay on the same buffers
        total, recon = step.step(batch)
    chamfer_o, rec_o, grads_o = U.oracle_step(O, Pe, Pd, ce, cd, p4, labels)
    l1_o = O.l1_norm(Pe).detach() + O.l1_norm(Pd).detach()
    what = f"maxdim {maxdim} B {B} N {N} {chans[0]}/{chans[1]}"
    errs = {"recon": U.relerr(recon.cpu(), rec_o), "chamfer": U.relerr(step.loss_out[1].cpu(), chamfer_o),
            "loss": U.relerr(total.cpu(), chamfer_o + lam * l1_o)}
    print(f"[{what}] recon abs max {float(rec_o.abs().max()):.3e}, rel errs " + ", ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    assert torch.isfinite(rec_o).all() and float(rec_o.abs().max()) > 1e-3, "the weights are not live"
    U.assert_close(total, chamfer_o + lam * l1_o, FWD_TOL, "total loss")
    U.assert_close(step.loss_out[1], chamfer_o, FWD_TOL, "chamfer")
    U.assert_close(recon, rec_o, FWD_TOL, "recon")
    l1 = {f"{pre}.{k}": lam * torch.sign(v.detach()) for pre, P in (("enc", Pe), ("dec", Pd)) for k, v in P.items()}
    worst, name = U.assert_named_grads_close(U.named_grads(enc, dec), grads_o, GRAD_TOL, what, add=l1, max_floor_routed=MAX_FLOOR_ROUTED)
    print(f"[{what}] worst gradient tensor: {name}: rel err {worst:.2e}")


@pytest.mark.parametrize("maxdim,B,N,chans,num_basis_fn", [(2, 8, 30, CFG2, 10), (3, 5, 13, WIDE, 10), (2, 8, 30, CFG2, 5)])
def test_native_adam_live_weights_follows_oracle(maxdim, B, N, chans, num_basis_fn):
    """Three graph-replayed Adam steps from live weights against three oracle steps with torch.optim.Adam on the CPU leaf tensors
    (the L1 term on the loss, as the reference's loop adds it): the loss of every step at FWD_TOL, every parameter tensor at 1e-9
    (one Adam update carries lr x the gradient's relative error; the tensors of _ADAM_CONDITIONING at 100 x the oracle's own figure).  num_basis_fn = 5: the radial tensors are STORED 20 bells wide --
    their padding columns, zeroed when the live weights were loaded, are exactly zero after the three steps."""
    from lgn.step import NativeTrainStep
    O, dev, enc, dec, Pe, Pd, ce, cd, p4, labels = _setup(maxdim, B, N, *chans, num_basis_fn=num_basis_fn)
    lr, lam = 5e-4, 1e-8
    step = NativeTrainStep(enc, dec, batch_size=B, lr=lr, l1_lambda=lam, use_graph=True)
    batch = {"p4": p4.to(dev), "labels": labels.to(dev)}
    for P in (Pe, Pd):
        for v in P.values():
            v.requires_grad_(True)
    opt = torch.optim.Adam(list(Pe.values()) + list(Pd.values()), lr=lr)
    what = f"maxdim {maxdim} B {B} N {N} bells {2 * num_basis_fn}"
    for it in range(3):
        loss, _ = step.step(batch)
        loss_o, _, _ = U.oracle_step(O, Pe, Pd, ce, cd, p4, labels, l1_lambda=lam)
        opt.step()
        print(f"[{what}] step {it}: loss {float(loss_o):.6e}, rel err {U.relerr(loss.cpu(), loss_o):.2e}")
        U.assert_close(loss, loss_o, FWD_TOL, f"loss at step {it}")
    assert int(step.step_dev.item()) == 3
    measured = _ADAM_CONDITIONING.get((maxdim, B, N, num_basis_fn), {})
    errs = {f"{pre}.{k}": U.relerr(v.cpu(), P[k].detach()) for pre, mod, P in (("enc", enc, Pe), ("dec", dec, Pd)) for k, v in mod.state_dict().items()}
    for k, e in errs.items():
        if k in measured or e > 1e-9:
            print(f"[{what}] parameter {k} after 3 Adam steps: rel err {e:.2e}" + (f" (held to 100 x {measured[k]:.2e})" if k in measured else ""))
    strict = {k: e for k, e in errs.items() if k not in measured}
    name = max(strict, key=strict.get)
    print(f"[{what}] worst parameter tensor after 3 Adam steps: {name}: rel err {strict[name]:.2e}")
    for k, e in errs.items():
        tol = 100 * measured[k] if k in measured else 1e-9
        assert e <= tol, f"{k} after 3 Adam steps: rel err {e:.3e} > {tol:.1e}"
    if num_basis_fn < 10:
        padded = 0
        for mod in (enc, dec):
            mod.named_parameter_views()                  # (the views follow the block the step re-homed)
            for stored, shape in zip(mod._p_stores, mod._p_shapes):
                if tuple(stored.shape) != tuple(shape):
                    padded += 1
                    assert float(stored[..., shape[-1]:].abs().max()) == 0, "padding columns must stay exactly zero through Adam + L1"
        assert padded > 0
