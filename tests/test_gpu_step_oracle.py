"""Whole training steps at LIVE weights against the oracle, per gradient tensor.

At the reference's initial weights the network does almost nothing: the reconstruction is ~1e-9 of the input, the loss is sum |p|^2 to
eleven digits whatever the kernels do, and a third (maxdim 2) to two thirds (maxdim 3) of the gradient tensors lie four or more orders
below the step's largest gradient.  U.live_weights adds 0.1 * randn to every state_dict tensor: reconstructions of O(0.01) .. O(1000),
at most 6 of ~100 live gradient tensors below 1e-4 of the largest, none below 1e-6.  Every case is the smallest shape that enters the
launch regime it names; the reference of every case is the oracle on the CPU (0.1 .. 5.5 s), loss / Chamfer part / reconstruction at
FWD_TOL and every gradient tensor against its own largest entry at GRAD_TOL (U.assert_named_grads_close).  The maxdim-2 regimes
added later (_LIVE below) choose sigma and seed per case so that U.assert_live holds on the oracle's outputs alone, and the BASELINE
sizes (512 x 30, 321 x 64, 256 x 150, 512 x 30 at maxdim 3) run as U.tiled_jets batches: 7 distinct jets laid out cyclically, the
oracle on the 7 with per-jet weights.

enc.input_func_node.weights.(0, 0) depends on how the particle mass is rounded: its gradient is linear in sqrt|E^2 - p^2|, and E^2 and
p^2 cancel to 1e-7 of their size.  The kernels form the mass as the reference does (minkowski_sq_unfused, csrc/common.hpp: no fused
multiply-add); with fused squares in the oracle's normsq4 that tensor alone moves by 1e-9.  Worst tensor of any case here: 1.8e-12
(1 x 150).

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
C123 = ((1, 2, 3, 4), (4, 3, 2, 1))
TILE_K = 7

# {(maxdim, B, N, encoder channels): (sigma, seed) of U.live_weights} of the cases that must pass U.assert_live on the oracle's outputs
# alone.  Measured there (max |recon|; gradient tensors under 1e-4 of the largest, of 100 -- 112 at maxdim 3 -- with a gradient):
#   5 x 30    0.1        9.9e+0  3      70 x 30   0.1        1.4e+2  2      3 x 40    0.1        2.4e+2  3      3 x 41   0.1   1.4e+1  2
#   2 x 63    0.06 / 1   3.5e-1  6      2 x 64    0.08 / 3   3.6e-1  6      2 x 65    0.07       1.7e+0  4      1 x 150  0.07  3.3e+0  9
#   4 x 13 (1,2,3,4)  0.13 / 3  5.6e-2  1
#   tiled 512 x 30  0.1  1.7e+1  1      tiled 321 x 64  0.08 / 3  7.4e-1  3      tiled 512 x 30 maxdim 3  0.07  8.6e-2  5
#   tiled 256 x 150  0.035, the encoder's CGMLP tensors 0.25  7.6e-1  1
# Sigma matters: at N = 63 / 64 the default 0.1 gives reconstructions of 5e5 .. 7e5; at 256 x 150 every uniform sigma leaves 26 .. 33
# tensors (the encoder's CGMLPs, 1e-5 .. 1e-6 of the decoder's first mixing weight) under 1e-4, so those tensors move further.
_LIVE = {(2, 5, 30, CFG2[0]): (0.1, 77), (2, 70, 30, CFG2[0]): (0.1, 77), (2, 3, 40, CFG2[0]): (0.1, 77), (2, 3, 41, CFG2[0]): (0.1, 77),
         (2, 2, 63, CFG2[0]): (0.06, 1), (2, 2, 64, CFG2[0]): (0.08, 3), (2, 2, 65, CFG2[0]): (0.07, 77), (2, 1, 150, CFG2[0]): (0.07, 77),
         (2, 4, 13, C123[0]): (0.13, 3),
         (2, 512, 30, CFG2[0]): (0.1, 77), (2, 321, 64, CFG2[0]): (0.08, 3),
         (2, 256, 150, CFG2[0]): ((("", 0.035), ("enc.lgn_cg.mlp", 0.25)), 77), (3, 512, 30, CFG5[0]): (0.07, 77)}

# {(maxdim, B, N, num_basis_fn): {parameter tensor: the oracle's disagreement with itself after three Adam steps}}: see the head of the file
_ADAM_CONDITIONING = {(3, 5, 13, 10): {"dec.lgn_cg.node_levels.1.cat_mix.mix_reps.weights.(0, 2)": 3.57e-08,
                                       "dec.lgn_cg.node_levels.1.cat_mix.mix_reps.weights.(2, 0)": 1.72e-08,
                                       "dec.lgn_cg.node_levels.0.cat_mix.mix_reps.weights.(2, 0)": 9.65e-09,
                                       "dec.lgn_cg.node_levels.0.cat_mix.mix_reps.weights.(0, 2)": 7.98e-09}}


def _setup(maxdim, B, N, che, chd, num_basis_fn=10, sigma=0.1, wseed=77, dev="cuda:0"):
    """Networks at live weights on the GPU, the same weights as CPU dicts, the oracle's two configurations and a padded batch."""
    import __graft_entry__ as G
    from oracle import lgn_oracle as O
    dev = torch.device(dev)
    enc, dec = G._models(N, che, chd, dev, seed=3, maxdim=maxdim, num_basis_fn=num_basis_fn)
    Pe, Pd = U.live_weights(enc, dec, sigma=sigma, seed=wseed)
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
    (3, 2, 65, ((3, 4, 4), (4, 4, 3))),      # first N beyond the tile-blocked separable decoder kernels (N <= 64)
    # the remaining maxdim-2 launch regimes (_LIVE: their sigma and what the oracle alone gives there)
    (2, 5, 30, CFG2),        # jet split 8, odd B
    (2, 70, 30, CFG2),       # jet split 4 (level_jet_split: 65 .. 128 jets)
    (2, 3, 40, CFG2),        # last N of level_bwd3 and of the rebuilt separable decoder aggregate; ten groups of four
    (2, 3, 41, CFG2),        # first N of mix + one pair sweep, stored aggregate, dec_output_loss_kernel on its own
    (2, 2, 63, CFG2),        # last N below the wide sweep
    (2, 2, 64, CFG2),        # first wide (8-wave) sweep, full wave
    (2, 2, 65, CFG2),        # one particle into the second wave
    (2, 1, 150, CFG2),       # chunked receivers, single jet
    (2, 4, 13, C123)])       # C = 1 / 2 / 3 level and CGMLP instantiations, last tile partly empty
def test_native_step_live_weights_matches_oracle(maxdim, B, N, chans):
    """The graph-replayed whole-step call (what the chooser takes) at live weights: total loss, Chamfer part, reconstruction and
    every named gradient (+ the L1 sub-gradient the step adds) against the oracle.  The cases of _LIVE must first pass
    U.assert_live on the oracle's outputs alone; its count of small gradient tensors is their max_floor_routed."""
    from lgn.step import NativeTrainStep, native_train_step
    live = _LIVE.get((maxdim, B, N, chans[0]))
    O, dev, enc, dec, Pe, Pd, ce, cd, p4, labels = _setup(maxdim, B, N, *chans, **(dict(sigma=live[0], wseed=live[1]) if live else {}))
    lam = 1e-8
    step = native_train_step(enc, dec, B, l1_lambda=lam, optimizer=False, use_graph=True)
    assert isinstance(step, NativeTrainStep), "the chooser must take the whole-step call for this configuration"
    batch = {"p4": p4.to(dev), "labels": labels.to(dev)}
    for _ in range(2):                      # second iteration = graph replay on the same buffers
        total, recon = step.step(batch)
    chamfer_o, rec_o, grads_o, _, pooled = U.oracle_step(O, Pe, Pd, ce, cd, p4, labels, with_latent=True)
    floor = MAX_FLOOR_ROUTED
    if live:
        floor = U.assert_live(O, rec_o, grads_o, p4, O.get_real(rec_o, "sum"), pooled=pooled, latent_map=ce.map_to_latent)
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
    worst, name = U.assert_named_grads_close(U.named_grads(enc, dec), grads_o, GRAD_TOL, what, add=l1, max_floor_routed=floor)
    print(f"[{what}] worst gradient tensor: {name}: rel err {worst:.2e}")


@pytest.mark.parametrize("maxdim,B,N,chans", [
    (2, 512, 30, CFG2),      # cfg2 size: one round, two workgroups per CU, 64-row chain CGMLP at 15 360 rows
    (2, 321, 64, CFG2),      # N >= 64 with B > 320: the 4-wave sweep
    (2, 256, 150, CFG2),     # cfg4 size
    (3, 512, 30, CFG5)])     # cfg5 size
def test_native_step_full_size_tiled_batch_matches_oracle(maxdim, B, N, chans):
    """BASELINE-size batches without a full-size oracle run: the batch is U.tiled_jets' 7 distinct padded jets laid out cyclically,
    the Chamfer loss is a sum over jets, so the oracle on the 7 jets with per-jet weights (the number of copies) gives the loss and
    every gradient of the whole batch exactly; the reconstruction of jet b is the oracle's of jet b % 7, for every b."""
    from lgn.step import NativeTrainStep, native_train_step
    from oracle import lgn_oracle as O
    sigma, wseed = _LIVE[(maxdim, B, N, chans[0])]
    _, dev, enc, dec, Pe, Pd, ce, cd, _, _ = _setup(maxdim, 1, N, *chans, sigma=sigma, wseed=wseed)
    p4, labels, p4_k, labels_k, copies = U.tiled_jets(B, N, K=TILE_K, seed=B + N)
    lam = 1e-8
    step = native_train_step(enc, dec, B, l1_lambda=lam, optimizer=False, use_graph=True)
    assert isinstance(step, NativeTrainStep), "the chooser must take the whole-step call for this configuration"
    batch = {"p4": p4.to(dev), "labels": labels.to(dev)}
    for _ in range(2):
        total, recon = step.step(batch)
    chamfer_o, rec_k, grads_o, _, pooled = U.oracle_step(O, Pe, Pd, ce, cd, p4_k, labels_k, jet_weights=copies, with_latent=True)
    floor = U.assert_live(O, rec_k, grads_o, p4_k, O.get_real(rec_k, "sum"), pooled=pooled, latent_map=ce.map_to_latent)
    rec_o = rec_k[:, torch.arange(B) % TILE_K]
    l1_o = O.l1_norm(Pe).detach() + O.l1_norm(Pd).detach()
    what = f"tiled maxdim {maxdim} B {B} N {N} {chans[0]}/{chans[1]}"
    errs = {"recon": U.relerr(recon.cpu(), rec_o), "chamfer": U.relerr(step.loss_out[1].cpu(), chamfer_o),
            "loss": U.relerr(total.cpu(), chamfer_o + lam * l1_o)}
    print(f"[{what}] recon abs max {float(rec_o.abs().max()):.3e}, rel errs " + ", ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    U.assert_close(total, chamfer_o + lam * l1_o, FWD_TOL, "total loss")
    U.assert_close(step.loss_out[1], chamfer_o, FWD_TOL, "chamfer")
    U.assert_close(recon, rec_o, FWD_TOL, "recon")
    l1 = {f"{pre}.{k}": lam * torch.sign(v.detach()) for pre, P in (("enc", Pe), ("dec", Pd)) for k, v in P.items()}
    worst, name = U.assert_named_grads_close(U.named_grads(enc, dec), grads_o, GRAD_TOL, what, add=l1, max_floor_routed=floor)
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
