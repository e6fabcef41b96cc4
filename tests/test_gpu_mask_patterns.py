"""Level operators, training steps and evaluation steps on jets with holes, sparse jets and disagreeing labels, against the oracle.

Every other jet the suite feeds to a mask-reading kernel is O.synthetic_jets(..., pad=True): real particles first, zero rows after
them, at least min(10, N) real ones.  The kernels that read the mask do index arithmetic on groups of four particles, pair tiles,
half-waves and jet pairs; the batches here (tests/_jets.py) mask a row between real rows, whole groups of four in mid-jet, everything
but the end of the jet, and leave jets of 0, 1, 2 and 3 particles.  `disagree` batches carry momenta on masked rows, two identical
real rows and a real row of zeros: the reference takes the mask from data['labels'] (lgn_encoder.py:386-403), and
tests/test_oracle_golden.py pins the oracle to it on these patterns (g28 fixtures).

The reference of every case is the oracle on the CPU at live weights (U.live_weights; networks G._models(seed=3)); the jets are
_jets.pattern_jets(N, names, JET_SEED).  U.assert_live(..., mask=labels) holds on the oracle's outputs alone for every case, with
the sigma / seed of _LIVE.  Per case below: sigma / seed, the oracle's max |recon|, its count of gradient tensors under 1e-4 of the
largest (the case's max_floor_routed) of those with a gradient, and -- measured on the MI355X -- the worst per-jet reconstruction
error (relative to that jet's own maximum) and the worst strictly checked gradient tensor.

    case                                                          sigma / seed  max |recon|  under 1e-4   worst jet   worst gradient tensor
    sparse maxdim 2 N 30 CFG2                                     0.1 / 77      4.2e-02      1 / 100      3.4e-15     4.4e-15  enc.rad_funcs.rad_funcs.1.linear.1.weight
    holed maxdim 2 N 30 CFG2                                      0.1 / 77      1.8e+02      1 / 100      5.0e-15     1.5e-14  dec.rad_funcs.rad_funcs.1.linear.0.bias
    sparse maxdim 2 N 40 CFG2                                     0.1 / 77      2.8e-02      1 / 100      2.4e-15     5.3e-15  enc.rad_funcs.rad_funcs.0.c
    holed maxdim 2 N 40 CFG2                                      0.09 / 77     1.4e+02      4 / 100      3.1e-15     8.7e-15  dec.rad_funcs.rad_funcs.2.linear.0.bias
    sparse maxdim 2 N 41 CFG2                                     0.1 / 77      3.8e-02      1 / 100      1.2e-15     5.4e-15  enc.lgn_cg.mlp_levels.0.linear.1.weight
    holed maxdim 2 N 41 CFG2                                      0.09 / 77     1.2e+02      7 / 100      2.6e-15     1.3e-14  enc.lgn_cg.mlp_levels.1.linear.3.weight
    sparse maxdim 2 N 64 CFG2                                     0.1 / 77      2.8e-02      2 / 100      4.2e-15     4.0e-14  enc.rad_funcs.rad_funcs.1.linear.1.weight
    holed maxdim 2 N 64 CFG2                                      0.08 / 77     7.2e+02      10 / 100     5.2e-15     1.6e-14  enc.lgn_cg.mlp_levels.0.linear.6.weight
    sparse maxdim 2 N 13 C123                                     0.13 / 3      7.0e-03      0 / 100      1.5e-15     3.5e-15  enc.rad_funcs.rad_funcs.1.c
    holed maxdim 2 N 13 C123                                      0.13 / 3      4.7e-02      0 / 100      1.3e-15     2.3e-15  enc.lgn_cg.mlp_levels.0.linear.6.weight
    sparse maxdim 3 N 13 WIDE                                     0.1 / 77      5.0e-02      4 / 112      2.3e-15     3.6e-14  dec.lgn_cg.node_levels.1.cat_mix.mix_reps.weights.(2, 0)
    holed maxdim 3 N 13 WIDE                                      0.1 / 77      2.0e+02      2 / 112      8.8e-15     2.8e-14  dec.lgn_cg.node_levels.1.cat_mix.mix_reps.weights.(2, 0)
    sparse maxdim 3 N 30 CFG5                                     0.1 / 77      3.0e-02      5 / 112      2.0e-15     1.2e-13  dec.lgn_cg.node_levels.1.cat_mix.mix_reps.weights.(0, 2)
    holed maxdim 3 N 30 CFG5                                      0.08 / 77     1.1e+01      4 / 112      9.4e-15     6.3e-14  dec.lgn_cg.node_levels.1.cat_mix.mix_reps.weights.(0, 2)
    sparse maxdim 3 N 33 OFF_STATIC                               0.1 / 77      1.9e-03      3 / 65       3.2e-15     7.7e-15  dec.lgn_cg.node_levels.0.cat_mix.mix_reps.weights.(2, 2)
    holed maxdim 3 N 33 OFF_STATIC                                0.1 / 77      7.0e-02      2 / 65       4.4e-15     1.1e-14  enc.lgn_cg.node_levels.0.cat_mix.mix_reps.weights.(1, 1)
    holed maxdim 2 N 30 CFG2 tiled to 275                         0.1 / 77      1.8e+02      1 / 100      5.3e-15     1.3e-14  dec.rad_funcs.rad_funcs.2.linear.0.bias
    holed maxdim 3 N 30 CFG5 tiled to 33                          0.08 / 77     1.1e+01      4 / 112      9.4e-15     6.2e-14  dec.lgn_cg.node_levels.1.cat_mix.mix_reps.weights.(0, 2)
    disagree maxdim 2 N 30 CFG2                                   0.1 / 77      1.8e+02      1 / 100      5.0e-15     1.5e-14  dec.rad_funcs.rad_funcs.1.linear.0.bias
    holed maxdim 2 N 12 POOL_CH map_to_latent mean                0.1 / 77      2.3e-02      3 / 100      1.4e-15     1.1e-14  enc.rad_funcs.rad_funcs.2.linear.1.weight
    holed maxdim 2 N 12 POOL_CH map_to_latent mean&max            0.1 / 77      1.0e-02      1 / 100      2.2e-15     2.8e-15  enc.lgn_cg.mlp_levels.1.linear.0.weight
    holed maxdim 2 N 12 POOL_CH map_to_latent min                 0.1 / 77      2.2e-02      1 / 100      2.5e-15     3.8e-15  dec.rad_funcs.rad_funcs.2.linear.0.bias
    holed maxdim 2 N 12 POOL_CH map_to_latent mix                 0.1 / 77      9.8e-02      1 / 100      1.8e-15     2.1e-15  dec.rad_funcs.rad_funcs.1.linear.1.bias
    holed maxdim 2 N 12 POOL_CH jet_features                      0.04 / 1      5.7e-01      7 / 100      2.0e-15     1.2e-14  enc.lgn_cg.node_levels.0.cat_mix.mix_reps.weights.(0, 0)

Evaluation step (forward only) on HOLED: loss 8.2e-15 (maxdim 2, N = 30) / 1.5e-14 (maxdim 3, N = 13), worst jet: get_real(recon)
4.6e-15 / 8.6e-15, latent (0, 0) 2.9e-15 / 3.6e-15, latent (1, 1) 1.1e-15 / 2.0e-15; the same 11 jets through a step built for 16 give
reconstruction and latent bit-equal to the 11-jet step at both shapes.  The level operators alone keep test_gpu_parity's assertions
(1e-11 / 1e-9 of the tensor's maximum) and pass at every shape.  No case needed more than the project's tolerances; no kernel failed.

What these inputs would catch, measured with the oracle against a deliberately wrong oracle (CPU, maxdim 2, N = 30, CFG2): a mask taken
from p4 instead of the labels moves the `disagree` loss by 0.6, the reconstruction of jets 0 and 2 by 2e2 / 0.3 of their maximum and
every gradient tensor by 6e-2 or more; a prefix mask with the same number of real rows moves eight of the eleven HOLED jets by 0.2 .. 1
of their maximum and every gradient tensor by 1.6e-5 or more -- the loss by 1.4e-4 only, which is why the reconstruction is held per jet.

The reconstruction is checked PER JET, max |rec[b] - rec_o[b]| <= FWD_TOL * max |rec_o[b]|: a sparse jet's reconstruction is 1e-3 of
a full jet's, so a batch-wide maximum would hold it to 1e-8 only.  An all-masked jet's reconstruction is exactly zero in the oracle
(and in the reference: g28) and must be exactly zero here.

Tolerances above FWD_TOL = 1e-11 / GRAD_TOL = 1e-9 (_CONDITIONING: 100 x the oracle against itself with every jet's particles and
labels reversed): none."""
import dataclasses
import functools

import pytest
import torch

import _jets as J
import _util as U

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
FWD_TOL = 1e-11
GRAD_TOL = 1e-9
JET_SEED = 11


@dataclasses.dataclass(frozen=True)
class Case:
    maxdim: int
    N: int
    chans: tuple
    batch: str                    # a key of BATCHES
    tile: int = None              # the step's batch: the K jets laid out cyclically to this many
    latent: str = "min&max"
    jet_features: bool = False

    @property
    def what(self):
        opts = (f" tiled to {self.tile}" if self.tile else "") + (f" map_to_latent {self.latent}" if self.latent != "min&max" else "") \
            + (" jet_features" if self.jet_features else "")
        return f"{self.batch} maxdim {self.maxdim} N {self.N} {self.chans[0]}/{self.chans[1]}{opts}"


CFG2 = ((3, 3, 4, 4), (4, 4, 3, 3))
CFG5 = ((4, 4, 6, 6), (6, 6, 4, 4))
WIDE = ((2, 4, 7, 8), (8, 6, 5, 3))
C123 = ((1, 2, 3, 4), (4, 3, 2, 1))
OFF_STATIC = ((3, 4, 4), (4, 4, 3))
POOL_CH = ((2, 2, 3, 3), (3, 3, 2, 2))
BATCHES = {"sparse": J.SPARSE, "holed": J.HOLED, "disagree": J.HOLED}


# {case: (sigma, seed) of U.live_weights}; a case that is not listed takes (0.1, 77).  At 0.1 / 77 the reconstruction of the listed HOLED
# cases is 2e3 .. 1.5e7 (N = 40, 41, 64) resp. 2.3e5 (maxdim 3, N = 30), that of the (1,2,3,4) net 3e-4 .. 7e-4
_LIVE = {Case(2, 40, CFG2, "holed"): (0.09, 77), Case(2, 41, CFG2, "holed"): (0.09, 77), Case(2, 64, CFG2, "holed"): (0.08, 77),
         Case(2, 13, C123, "sparse"): (0.13, 3), Case(2, 13, C123, "holed"): (0.13, 3),
         Case(3, 30, CFG5, "holed"): (0.08, 77), Case(3, 30, CFG5, "holed", tile=33): (0.08, 77),
         # jet_features: 7.5e25 at 0.1; at 0.025 .. 0.05 most seeds leave 11 .. 22 of 100 tensors under 1e-4 of the largest
         Case(2, 12, POOL_CH, "holed", jet_features=True): (0.04, 1)}

# {case: {gradient tensor or 'recon': the oracle's disagreement with itself, particles of every jet reversed}}: held to 100 x the figure
_CONDITIONING = {}


def _jets(case):
    """The K distinct jets of a case."""
    p4, labels = J.pattern_jets(case.N, BATCHES[case.batch], JET_SEED)
    if case.batch == "disagree":
        p4, labels = J.disagree(p4, labels, torch.Generator().manual_seed(JET_SEED + 1))
    return p4, labels


def _nets(case, dev):
    import __graft_entry__ as G
    enc, dec = G._models(case.N, case.chans[0], case.chans[1], torch.device(dev), seed=3, maxdim=case.maxdim, map_to_latent=case.latent,
                         jet_features=case.jet_features)
    sigma, seed = _LIVE.get(case, (0.1, 77))
    Pe, Pd = U.live_weights(enc, dec, sigma=sigma, seed=seed)
    return enc, dec, Pe, Pd


def _cfgs(case):
    from oracle import lgn_oracle as O
    common = dict(num_particles=case.N, maxdim=case.maxdim, map_to_latent=case.latent)
    return (O.NetConfig(num_channels=tuple(case.chans[0]), jet_features=case.jet_features, **common),
            O.NetConfig(num_channels=tuple(case.chans[1]), **common))


@dataclasses.dataclass
class Ref:
    p4: torch.Tensor              # the K distinct jets
    labels: torch.Tensor
    copies: torch.Tensor          # (K,) how often the step's batch holds each (ones unless tiled)
    Pe: dict
    Pd: dict
    chamfer: torch.Tensor
    rec: torch.Tensor             # (2, K, N, 4)
    grads: dict
    latent: dict
    floor: int                    # assert_live's count of small gradient tensors


@functools.lru_cache(maxsize=None)
def _oracle(case):
    """One oracle step of the case on the CPU (computed once, never modified), live by U.assert_live on its outputs alone."""
    from oracle import lgn_oracle as O
    p4, labels = _jets(case)
    K = p4.shape[0]
    copies = J.tile(p4, labels, case.tile)[2] if case.tile else torch.ones(K, dtype=torch.long)
    _, _, Pe, Pd = _nets(case, "cpu")
    ce, cd = _cfgs(case)
    chamfer, rec, grads, lat, pooled = U.oracle_step(O, Pe, Pd, ce, cd, p4, labels, jet_weights=copies if case.tile else None,
                                                     with_latent=True)
    floor = U.assert_live(O, rec, grads, p4, O.get_real(rec, "sum"), pooled=pooled, latent_map=case.latent, mask=labels)
    return Ref(p4, labels, copies, Pe, Pd, chamfer, rec, grads, lat, floor)


def _per_jet(got, ref, idx, tol, what, exact_zero=True):
    """got (.., B, ...) against ref (.., K, ...) on axis 1, jet b against jet idx[b], each relative to ITS OWN maximum in ref; a jet
    whose reference is exactly zero must be exactly zero.  Returns the worst relative error."""
    got, ref = torch.as_tensor(got, dtype=torch.float64).detach().cpu().movedim(1, 0), ref.detach().movedim(1, 0)[idx]
    assert tuple(got.shape) == tuple(ref.shape), f"{what}: shape {tuple(got.shape)} vs {tuple(ref.shape)}"
    err = (got - ref).abs().flatten(1).amax(1)
    top = ref.abs().flatten(1).amax(1)
    zero = top == 0
    if exact_zero:
        assert float(err[zero].max() if zero.any() else 0.0) == 0, f"{what}: jets {zero.nonzero().flatten().tolist()} must be exactly zero"
    rel = torch.where(zero, torch.zeros_like(err), err / top.clamp_min(1e-300))
    b = int(rel.argmax())
    assert float(rel[b]) <= tol, f"{what}: jet {b} (distinct jet {int(idx[b])}): rel err {float(rel[b]):.3e} > {tol:.1e} (its max {float(top[b]):.3e})"
    return float(rel[b])


def _train_case(case, chooser="NativeTrainStep"):
    """Two graph-replayed steps (the second a replay) of what the chooser takes against the oracle: total loss and Chamfer part at
    FWD_TOL, the reconstruction per jet, exact zeros for all-masked jets, every gradient tensor at GRAD_TOL of its own maximum."""
    from lgn import step as S
    from oracle import lgn_oracle as O
    R = _oracle(case)
    enc, dec, _, _ = _nets(case, DEV)
    K = R.p4.shape[0]
    B = case.tile or K
    p4, labels = (J.tile(R.p4, R.labels, B)[:2]) if case.tile else (R.p4, R.labels)
    lam = 1e-8
    step = S.native_train_step(enc, dec, B, l1_lambda=lam, optimizer=False, use_graph=True)
    assert type(step).__name__ == chooser, f"the chooser took {type(step).__name__} for {case.what}"
    batch = {"p4": p4.to(DEV), "labels": labels.to(DEV)}
    for _ in range(2):
        total, recon = step.step(batch)
    torch.cuda.synchronize()
    empty = (R.labels.sum(1) == 0).nonzero().flatten().tolist()
    if case.latent == "min&max" and not case.jet_features:
        assert empty and all(float(R.rec[:, k].abs().max()) == 0 for k in empty), "the oracle's reconstruction of an all-masked jet is exactly 0"
    l1_o = O.l1_norm(R.Pe).detach() + O.l1_norm(R.Pd).detach()
    measured = _CONDITIONING.get(case, {})
    U.assert_close(total, R.chamfer + lam * l1_o, FWD_TOL, "total loss")
    U.assert_close(step.loss_out[1], R.chamfer, FWD_TOL, "chamfer")
    worst_jet = _per_jet(recon, R.rec, torch.arange(B) % K, 100 * measured["recon"] if "recon" in measured else FWD_TOL, "recon")
    l1 = {f"{pre}.{k}": lam * torch.sign(v.detach()) for pre, P in (("enc", R.Pe), ("dec", R.Pd)) for k, v in P.items()}
    named = U.named_grads(enc, dec)
    loose = {n: g for n, g in named if n in measured}
    for n, g in loose.items():
        U.assert_close(g, R.grads[n] + l1[n], 100 * measured[n], f"grad {n} (measured tolerance)")
    worst, name = U.assert_named_grads_close([(n, g) for n, g in named if n not in loose], {n: g for n, g in R.grads.items() if n not in loose},
                                             GRAD_TOL, case.what, add=l1, max_floor_routed=R.floor)
    print(f"[{case.what}] oracle max |recon| {float(R.rec.abs().max()):.1e}, floor tensors {R.floor}; loss rel err "
          f"{U.relerr(total.cpu(), R.chamfer + lam * l1_o):.1e}, worst jet recon {worst_jet:.1e}, worst gradient tensor {name}: {worst:.1e}")
    return step


# ---- (a) encoder level operators alone -------------------------------------------------------------------------------------------
LEVEL_SHAPES = [(4, 4, 30, 11), (3, 4, 30, 11),      # level_bwd3, N <= 40
                (4, 3, 7, 11),                       # partly empty second group
                (4, 4, 41, 11),                      # mix + one pair sweep
                (3, 3, 64, 11),                      # wide sweep
                (4, 4, 150, 11),                     # chunked receivers
                (5, 6, 26, 11)]                      # C > 4: the ordered form
GENERIC_SHAPES = [(3, True, 4, 6, 30, 11),           # static kernels
                  (3, False, 4, 4, 33, 11),          # run-time tables
                  (3, True, 3, 4, 70, 11),           # beyond the tile-blocked kernels
                  (3, True, 8, 8, 13, 11)]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the GPU box"
    return torch.device(DEV)


@pytest.fixture(scope="module")
def O():
    from oracle import lgn_oracle
    return lgn_oracle


def _level_jets(N, batch):
    return _jets(Case(2, N, None, batch))


@pytest.mark.parametrize("batch", ["holed", "disagree"])
@pytest.mark.parametrize("C,CO,N,B", LEVEL_SHAPES)
def test_level_on_mask_patterns(dev, O, C, CO, N, B, batch):
    """LevelFn (test_gpu_parity._level_case, its assertions) on the HOLED jets and on their disagreeing copy."""
    from test_gpu_parity import _level_case
    _level_case(dev, O, False, C, CO, N, B, jets=_level_jets(N, batch))


@pytest.mark.parametrize("batch", ["holed", "disagree"])
@pytest.mark.parametrize("C,CO,N,B", LEVEL_SHAPES[:2])
def test_level_on_mask_patterns_whole_jet_workgroups(dev, O, C, CO, N, B, batch):
    """The 11 jets tiled to 264: every jet owns one workgroup, the backward takes the symmetric sweep.  The oracle runs on the 11;
    every tiled jet is compared with jet b % 11, the parameter gradients through cotangents tiled the same way (copy counts)."""
    from test_gpu_parity import _level_case
    _level_case(dev, O, False, C, CO, N, B, jets=_level_jets(N, batch), tile_to=264)


@pytest.mark.parametrize("batch", ["holed", "disagree"])
@pytest.mark.parametrize("flag", ["LGN_AMD_BWD_ORDERED", "LGN_AMD_LEVEL_V2"])
def test_level_on_mask_patterns_alternative_backwards(dev, O, monkeypatch, flag, batch):
    """The per-ordered-tile backward and the three-kernel backward on the first shape."""
    from test_gpu_parity import _level_case
    monkeypatch.setenv(flag, "1")
    C, CO, N, B = LEVEL_SHAPES[0]
    _level_case(dev, O, False, C, CO, N, B, jets=_level_jets(N, batch))


@pytest.mark.parametrize("batch", ["holed", "disagree"])
@pytest.mark.parametrize("maxdim,full,C,CO,N,B", GENERIC_SHAPES)
def test_generic_level_on_mask_patterns(dev, O, maxdim, full, C, CO, N, B, batch):
    """GenericLevelFn (test_gpu_parity._generic_level_case, its assertions): moments_*, local_*_static / run-time tables."""
    from test_gpu_parity import _generic_level_case
    _generic_level_case(dev, O, False, maxdim, full, C, CO, N, B, jets=_level_jets(N, batch))


# ---- (b) whole training step -----------------------------------------------------------------------------------------------------
STEP_SHAPES = [(2, 30, CFG2),            # jet split 8
               (2, 40, CFG2),            # last N of level_bwd3
               (2, 41, CFG2),            # first N of mix + one pair sweep
               (2, 64, CFG2),            # first wide sweep
               (2, 13, C123),            # C = 1 / 2 / 3 instantiations, last tile partly empty
               (3, 13, WIDE),            # both table kinds
               (3, 30, CFG5),
               (3, 33, OFF_STATIC)]      # off the static path: run-time tables


@pytest.mark.parametrize("batch", ["sparse", "holed"])
@pytest.mark.parametrize("maxdim,N,chans", STEP_SHAPES)
def test_native_step_on_mask_patterns(maxdim, N, chans, batch):
    _train_case(Case(maxdim, N, chans, batch))


@pytest.mark.parametrize("maxdim,N,chans,B", [(2, 30, CFG2, 275),       # one workgroup per jet, symmetric sweep, chain CGMLP
                                              (3, 30, CFG5, 33)])       # 17 jet pairs, the last one half empty
def test_native_step_on_tiled_mask_patterns(maxdim, N, chans, B):
    """HOLED tiled cyclically: the oracle on the 11 jets with per-jet weights gives loss and gradients of the whole batch exactly."""
    _train_case(Case(maxdim, N, chans, "holed", tile=B))


def test_native_step_on_disagreeing_labels():
    """Momenta on masked rows, two identical real rows, a real row of zeros: the mask is data['labels'], as in the reference."""
    _train_case(Case(2, 30, CFG2, "disagree"))


# ---- (c) evaluation step and latent ------------------------------------------------------------------------------------------------
def _eval_outputs(case, batch_size):
    """(NativeEvalStep's output for the case's jets through a step built for batch_size jets, as CPU copies)."""
    from lgn.step import NativeEvalStep
    R = _oracle(case)
    enc, dec, _, _ = _nets(case, DEV)
    ev = NativeEvalStep(enc, dec, batch_size, get_real_method="sum", keep_latent=True, use_graph=True)
    batch = {"p4": R.p4.to(DEV), "labels": R.labels.to(DEV)}
    for _ in range(2):
        out = ev.run(batch)
    torch.cuda.synchronize()
    return {"loss": out["loss"].cpu().clone(), "recon": out["recon"].cpu().clone(), "latent": {k: v.cpu().clone() for k, v in out["latent"].items()}}


EVAL_CASES = [Case(2, 30, CFG2, "holed"), Case(3, 13, WIDE, "holed")]


@pytest.mark.parametrize("case", EVAL_CASES, ids=["maxdim2_n30", "maxdim3_n13"])
def test_eval_step_on_mask_patterns(case):
    """NativeEvalStep on HOLED: loss at FWD_TOL, get_real(reconstruction) and the pooled latent per jet against the oracle."""
    from oracle import lgn_oracle as O
    R = _oracle(case)
    K = R.p4.shape[0]
    out = _eval_outputs(case, K)
    U.assert_close(out["loss"], R.chamfer, FWD_TOL, "loss")
    idx = torch.arange(K)
    errs = {"recon": _per_jet(out["recon"].unsqueeze(0), O.get_real(R.rec, "sum").unsqueeze(0), idx, FWD_TOL, "recon_real")}
    assert set(out["latent"].keys()) == set(R.latent.keys())
    for k in R.latent:
        errs[f"latent {k}"] = _per_jet(out["latent"][k], R.latent[k], idx, FWD_TOL, f"latent {k}")
    print(f"[eval {case.what}] loss rel err {U.relerr(out['loss'], R.chamfer):.1e}, worst jet: " + ", ".join(f"{k} {v:.1e}" for k, v in errs.items()))


@pytest.mark.parametrize("case", EVAL_CASES, ids=["maxdim2_n30", "maxdim3_n13"])
def test_eval_step_padding_path_on_mask_patterns(case):
    """The 11 jets through a step built for 16: the step fills rows 11 .. 15 with all-masked jets of its own.  The loss against the
    oracle; reconstruction and latent of the 11 jets against the 11-jet step, per jet at FWD_TOL and then bit for bit: 11 and 16 jets
    take the same launch shape (at maxdim 2 the level jet split of up to 64 jets), the forward of a jet reads no other jet, and
    the step's kernels add nothing atomically."""
    R = _oracle(case)
    K = R.p4.shape[0]
    own, padded = _eval_outputs(case, K), _eval_outputs(case, 16)
    assert tuple(padded["recon"].shape) == tuple(own["recon"].shape)
    idx = torch.arange(K)
    U.assert_close(padded["loss"], R.chamfer, FWD_TOL, "loss of the padded step")
    _per_jet(padded["recon"].unsqueeze(0), own["recon"].unsqueeze(0), idx, FWD_TOL, "recon_real, padded step against the 11-jet step")
    same = torch.equal(padded["recon"], own["recon"])
    for k in own["latent"]:
        _per_jet(padded["latent"][k], own["latent"][k], idx, FWD_TOL, f"latent {k}, padded step against the 11-jet step")
        same = same and torch.equal(padded["latent"][k], own["latent"][k])
    assert same, f"{case.what}: the padded step's reconstruction / latent of the 11 jets differ in bits from the 11-jet step's"


# ---- (d) pooling maps and the jet node under holes -----------------------------------------------------------------------------------
@pytest.mark.parametrize("latent", ["mean", "mean&max", "min", "mix"])
def test_latent_maps_on_mask_patterns(latent):
    """The junction's pooling over jets with holes; 'mean' divides as the oracle does (pinned to the reference by g28 / g7)."""
    _train_case(Case(2, 12, POOL_CH, "holed", latent=latent))


def test_sum_latent_map_falls_back_on_mask_patterns():
    """'sum' returns an extra axis in the reference (lgn_encoder.py:421-427), on which the reference's own decoder fails, and the
    oracle with it: there is no reference result of a whole step.  The chooser must fall back to CapturedModuleStep; its replayed
    graph is held to the eager module-API step (per-network calls under autograd) on the same weights and the same HOLED jets."""
    from lgn.step import TrainStep, native_train_step
    from oracle import lgn_oracle as O
    case = Case(2, 12, POOL_CH, "holed", latent="sum")
    p4, labels = _jets(case)
    _, _, Pe, Pd = _nets(case, "cpu")
    with pytest.raises(RuntimeError):
        U.oracle_forward(O, Pe, Pd, *_cfgs(case), p4, labels)
    K = p4.shape[0]
    batch = {"p4": p4.to(DEV), "labels": labels.to(DEV)}
    enc, dec, _, _ = _nets(case, DEV)
    a = native_train_step(enc, dec, K, optimizer=False, use_graph=True)
    assert type(a).__name__ == "CapturedModuleStep", f"the chooser took {type(a).__name__} for map_to_latent 'sum'"
    enc_b, dec_b, _, _ = _nets(case, DEV)
    b = TrainStep(enc_b, dec_b, optimizer=False)
    for _ in range(2):
        la, ra = a.step(batch)
    lb, rb = b.forward_backward(batch)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(rb).all()) and float(rb.detach().abs().max()) > 1e-3, "the weights are not live"
    U.assert_close(la, lb, FWD_TOL, "loss")
    _per_jet(ra, rb.detach().cpu(), torch.arange(K), FWD_TOL, "recon")
    ref = {n: (None if g is None else g.detach().cpu()) for n, g in U.named_grads(enc_b, dec_b)}
    U.assert_named_grads_close(U.named_grads(enc, dec), ref, GRAD_TOL, case.what)


def test_jet_features_on_mask_patterns():
    """The jet node (the sum of the jet's momenta, a 13th node that is always real) beside holes, and alone in an all-masked jet."""
    step = _train_case(Case(2, 12, POOL_CH, "holed", jet_features=True))
    assert step.split
