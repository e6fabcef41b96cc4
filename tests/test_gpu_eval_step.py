"""GPU tests of the evaluation step (lgn_step_eval_f64, lgn.step.NativeEvalStep): the reference's validate() loss -- Chamfer
[+ jet-feature MSE], no L1 -- and get_real(reconstruction), against the oracle on both decoder tails, the split step and the
table-driven step, against the reference's g17 vectors, and against the training step on the same weights."""
import functools

import pytest
import torch

import _util as U

pytestmark = pytest.mark.gpu

METHODS = ["real", "imag", "sum", "mean", "norm"]
# (maxdim, N, B): maxdim 2 at 12 particles (the loss rides on the decoder's last level_fwd2) and at 50 (dec_output_eval_kernel on
# its own); maxdim 3 (the table-driven step)
NETS = {"md2_n12": (2, 12, 3), "md2_n50": (2, 50, 2), "md3_n12": (3, 12, 2)}
CH = {2: ((3, 3, 4, 4), (4, 4, 3, 3)), 3: ((2, 3, 4), (4, 3, 2))}
DEV = "cuda:0"


def _models(net, seed=21):
    import __graft_entry__ as G
    maxdim, N, _ = NETS[net]
    return G._models(N, CH[maxdim][0], CH[maxdim][1], torch.device(DEV), seed=seed, maxdim=maxdim)


def _batch(net):
    from oracle import lgn_oracle as O
    _, N, B = NETS[net]
    return O.synthetic_jets(B, N, seed=N + B, pad=True)


_jet_mse = U.jet_mse


def _oracle_eval(enc, dec, p4, labels, method, jet, maxdim):
    """(loss, get_real(recon)) of the CPU oracle on the modules' current weights: the reference's evaluation loss."""
    from oracle import lgn_oracle as O
    N = p4.shape[1]
    Pe = {k: v.detach().cpu().clone() for k, v in enc.state_dict().items()}
    Pd = {k: v.detach().cpu().clone() for k, v in dec.state_dict().items()}
    ce = O.NetConfig(num_particles=N, maxdim=maxdim, num_channels=tuple(enc.num_channels))
    cd = O.NetConfig(num_particles=N, maxdim=maxdim, num_channels=tuple(dec.num_channels))
    with torch.no_grad():
        x = O.get_real(O.decoder_forward(Pd, cd, O.encoder_forward(Pe, ce, p4, labels)), method)
        loss = O.chamfer_loss(x, p4)
        if jet:
            loss = loss + _jet_mse(x, p4)
    return loss, x


@functools.lru_cache(maxsize=None)
def _oracle(net, method, jet):
    enc, dec = _models(net)
    p4, labels = _batch(net)
    return _oracle_eval(enc, dec, p4, labels, method, jet, NETS[net][0])


@pytest.mark.parametrize("use_graph", [False, True])
@pytest.mark.parametrize("net", list(NETS))
@pytest.mark.parametrize("jet", [False, True])
@pytest.mark.parametrize("method", METHODS)
def test_eval_step_matches_oracle(method, jet, net, use_graph):
    from lgn.step import NativeEvalStep
    enc, dec = _models(net)
    p4, labels = _batch(net)
    _, _, B = NETS[net]
    ev = NativeEvalStep(enc, dec, B, get_real_method=method, chamfer_jet_features=jet, use_graph=use_graph)
    batch = {"p4": p4.to(DEV), "labels": labels.to(DEV)}
    for _ in range(2):                      # (with the graph: capture, then a replay on the same buffers)
        out = ev.run(batch)
    loss_o, x_o = _oracle(net, method, jet)
    assert out["loss"].dim() == 0
    U.assert_close(out["loss"], loss_o, 1e-10, "loss")
    U.assert_close(out["recon"], x_o, 1e-10, "recon")


@pytest.mark.parametrize("use_graph", [False, True])
@pytest.mark.parametrize("jet", [False, True])
@pytest.mark.parametrize("method", METHODS)
def test_split_eval_step_matches_module_api(method, jet, use_graph):
    """jet_features: the split form (the encoder works on one node more than the decoder reconstructs), against the module API
    under no_grad on the same weights."""
    import __graft_entry__ as G
    from lgn.step import ModuleEvalStep, NativeEvalStep
    from oracle import lgn_oracle as O
    N, B = 12, 3
    enc, dec = G._models(N, (3, 3, 4, 4), (4, 4, 3, 3), torch.device(DEV), seed=9, jet_features=True)
    p4, labels = O.synthetic_jets(B, N, seed=4, pad=True)
    batch = {"p4": p4.to(DEV), "labels": labels.to(DEV)}
    ev = NativeEvalStep(enc, dec, B, get_real_method=method, chamfer_jet_features=jet, use_graph=use_graph)
    assert ev.split
    for _ in range(2):
        a = ev.run(batch)
    b = ModuleEvalStep(enc, dec, B, get_real_method=method, chamfer_jet_features=jet).run(batch)
    U.assert_close(a["loss"], b["loss"], 1e-10, "loss")
    U.assert_close(a["recon"], b["recon"], 1e-10, "recon")


@pytest.mark.parametrize("name", ["g1_e2e_maxdim2.npz", "g17_real_maxdim2.npz", "g17_norm_maxdim2.npz", "g17_realjet_maxdim2.npz",
                                  "g17_real_maxdim3.npz", "g17_norm_maxdim3.npz", "g17_realjet_maxdim3.npz"])
def test_eval_step_matches_reference_golden(name):
    """The reference's loss and reconstruction (g1: get_real 'sum', its Chamfer term -- the evaluation loss has no L1)."""
    import __graft_entry__ as G
    from lgn.step import NativeEvalStep
    from oracle import lgn_oracle as O
    z = U.load(name)
    m = U.meta(z)
    method = m.get("get_real_method", "sum")
    jet = bool(m.get("chamfer_jet_features", False))
    enc, dec = G._models(m["N"], m["ch_enc"], m["ch_dec"], torch.device(DEV), seed=m["seed"], maxdim=m.get("maxdim", 2))
    batch = {"p4": torch.from_numpy(z["p4"]).to(DEV), "labels": torch.from_numpy(z["labels"]).to(DEV)}
    out = NativeEvalStep(enc, dec, m["B"], get_real_method=method, chamfer_jet_features=jet, keep_latent=True).run(batch)
    g1 = "loss_chamfer" in z.files
    U.assert_close(out["loss"], z["loss_chamfer"] if g1 else z["loss"], 1e-11, "loss")
    U.assert_close(out["recon"], z["recon_real"] if g1 else O.get_real(torch.from_numpy(z["recon"]), method), 1e-11, "recon")
    if g1:
        for key in ((0, 0), (1, 1)):
            U.assert_close(out["latent"][key], z[f"latent.{key}"], 1e-11, f"latent {key}")


def _train_and_eval(net, method, jet, **kw):
    from lgn.step import NativeEvalStep, NativeTrainStep
    enc, dec = _models(net)
    p4, labels = _batch(net)
    B = NETS[net][2]
    batch = {"p4": p4.to(DEV), "labels": labels.to(DEV)}
    tr = NativeTrainStep(enc, dec, batch_size=B, optimizer=False, use_graph=False, get_real_method=method, chamfer_jet_features=jet, **kw)
    ev = NativeEvalStep(enc, dec, B, get_real_method=method, chamfer_jet_features=jet)
    tr.step(batch)
    out = ev.run(batch)
    torch.cuda.synchronize()
    return tr, out


@pytest.mark.parametrize("net", list(NETS))
@pytest.mark.parametrize("method", METHODS)
def test_eval_recon_and_loss_are_the_training_steps(net, method):
    """Same weights and batch: get_real of the training step's reconstruction, bit for bit (norm: the one operation torch and the
    kernel may round differently), and the training loss minus its L1 term."""
    from lgn.step import get_real
    tr, out = _train_and_eval(net, method, True, l1_lambda=1e-3)
    ref = get_real(tr.recon, method)
    if method == "norm":
        U.assert_close(out["recon"], ref, 1e-15, "recon")
    else:
        assert torch.equal(out["recon"], ref)
    chamfer, l1 = tr.loss_out[1].item(), tr.loss_out[2].item()
    assert l1 > 0
    assert abs(out["loss"].item() - chamfer) <= 1e-14 * abs(chamfer)
    U.assert_close(out["loss"], tr.loss_out[0] - 1e-3 * tr.loss_out[2], 1e-13, "loss")


def test_two_replays_give_identical_bits():
    from lgn.step import NativeEvalStep
    enc, dec = _models("md2_n12")
    p4, labels = _batch("md2_n12")
    ev = NativeEvalStep(enc, dec, NETS["md2_n12"][2], get_real_method="norm", chamfer_jet_features=True)
    batch = {"p4": p4.to(DEV), "labels": labels.to(DEV)}
    a = ev.run(batch)["loss"].clone()
    b = ev.run(batch)["loss"].clone()
    c = ev.run()["loss"].clone()
    assert torch.equal(a, b) and torch.equal(b, c)


def test_eval_step_follows_training_updates_without_rebuilding():
    """Built BEFORE three Adam steps of a NativeTrainStep on the same modules: it reads the updated weights where they live."""
    import __graft_entry__ as G
    from lgn.step import NativeEvalStep, NativeTrainStep
    from oracle import lgn_oracle as O
    N, B = 30, 4
    enc, dec = G._models(N, (3, 3, 4, 4), (4, 4, 3, 3), torch.device(DEV), seed=0)
    p4, labels = O.synthetic_jets(B, N, seed=3, pad=True)
    batch = {"p4": p4.to(DEV), "labels": labels.to(DEV)}
    tr = NativeTrainStep(enc, dec, B, lr=1e-2, use_graph=True, get_real_method="real", chamfer_jet_features=True)
    ev = NativeEvalStep(enc, dec, B, get_real_method="real", chamfer_jet_features=True)
    first = ev.run(batch)["loss"].item()
    for _ in range(3):
        tr.step(batch)
    out = ev.run(batch)
    loss_o, x_o = _oracle_eval(enc, dec, p4, labels, "real", True, 2)
    assert abs(out["loss"].item() - first) > 1e-6 * abs(first)
    U.assert_close(out["loss"], loss_o, 1e-10, "loss after 3 Adam steps")
    U.assert_close(out["recon"], x_o, 1e-10, "recon after 3 Adam steps")


def test_eval_step_built_before_the_training_step_follows_the_moved_parameters():
    import __graft_entry__ as G
    from lgn.step import NativeEvalStep, NativeTrainStep
    from oracle import lgn_oracle as O
    N, B = 12, 3
    enc, dec = G._models(N, (3, 3, 4, 4), (4, 4, 3, 3), torch.device(DEV), seed=5)
    p4, labels = O.synthetic_jets(B, N, seed=2, pad=True)
    batch = {"p4": p4.to(DEV), "labels": labels.to(DEV)}
    ev = NativeEvalStep(enc, dec, B)
    ev.run(batch)
    tr = NativeTrainStep(enc, dec, B, lr=1e-2, use_graph=False, get_real_method="real")     # re-homes both blocks
    tr.step(batch)
    out = ev.run(batch)
    loss_o, _ = _oracle_eval(enc, dec, p4, labels, "real", False, 2)
    U.assert_close(out["loss"], loss_o, 1e-10, "loss")


@pytest.mark.parametrize("method", ["real", "norm"])
def test_cfg2_sized_eval_matches_oracle(method):
    """512 jets x 30 particles (cfg2) against the oracle directly."""
    import __graft_entry__ as G
    from lgn.step import NativeEvalStep
    from oracle import lgn_oracle as O
    N, B = 30, 512
    enc, dec = G._models(N, (3, 3, 4, 4), (4, 4, 3, 3), torch.device(DEV), seed=0)
    p4, labels = O.synthetic_jets(B, N, seed=11, pad=True)
    out = NativeEvalStep(enc, dec, B, get_real_method=method, chamfer_jet_features=True).run({"p4": p4.to(DEV), "labels": labels.to(DEV)})
    loss_o, x_o = _oracle_eval(enc, dec, p4, labels, method, True, 2)
    U.assert_close(out["loss"], loss_o, 1e-10, "loss")
    U.assert_close(out["recon"], x_o, 1e-10, "recon")


@pytest.mark.parametrize("use_graph", [False, True])
@pytest.mark.parametrize("jet", [False, True])
def test_partial_last_batch_matches_the_reference_over_its_jets(jet, use_graph):
    """37 jets through a step built for 64: padded with all-masked jets, the loss is the reference's over the 37 (jet-feature MSE
    included: nn.MSELoss on that batch)."""
    import __graft_entry__ as G
    from lgn.step import NativeEvalStep
    from oracle import lgn_oracle as O
    N = 30
    enc, dec = G._models(N, (3, 3, 4, 4), (4, 4, 3, 3), torch.device(DEV), seed=1)
    full, lab_full = O.synthetic_jets(64, N, seed=8, pad=True)
    p4, labels = O.synthetic_jets(37, N, seed=6, pad=True)
    ev = NativeEvalStep(enc, dec, 64, get_real_method="real", chamfer_jet_features=jet, use_graph=use_graph)
    ev.run({"p4": full.to(DEV), "labels": lab_full.to(DEV)})
    out = ev.run({"p4": p4.to(DEV), "labels": labels.to(DEV)})
    loss_o, x_o = _oracle_eval(enc, dec, p4, labels, "real", jet, 2)
    assert out["recon"].shape == (37, N, 4)
    U.assert_close(out["loss"], loss_o, 1e-10, "loss over 37 jets")
    U.assert_close(out["recon"], x_o, 1e-10, "recon")
    out = ev.run({"p4": full.to(DEV), "labels": lab_full.to(DEV)})      # and back to a full batch
    loss_o, _ = _oracle_eval(enc, dec, full, lab_full, "real", jet, 2)
    U.assert_close(out["loss"], loss_o, 1e-10, "loss over 64 jets")


@pytest.mark.parametrize("net", ["md2_n12", "md3_n12"])
def test_keep_latent_equals_the_module_encoder(net):
    from lgn.step import NativeEvalStep
    enc, dec = _models(net)
    p4, labels = _batch(net)
    batch = {"p4": p4.to(DEV), "labels": labels.to(DEV)}
    out = NativeEvalStep(enc, dec, NETS[net][2], keep_latent=True).run(batch)
    with torch.no_grad():
        lat = enc(batch)
    for key in ((0, 0), (1, 1)):
        assert out["latent"][key].shape == lat[key].shape
        U.assert_close(out["latent"][key], lat[key], 1e-12, f"latent {key}")


def test_refused_call_leaves_the_outputs_untouched():
    """A refusal (workspace one double short) comes before any launch: the outputs keep their sentinel."""
    import ctypes as C
    from lgn import _native as N
    from lgn.step import NativeEvalStep
    enc, dec = _models("md2_n12")
    p4, labels = _batch("md2_n12")
    ev = NativeEvalStep(enc, dec, NETS["md2_n12"][2], use_graph=False)
    ev.load_batch({"p4": p4.to(DEV), "labels": labels.to(DEV)})
    ev.recon.fill_(7.0)
    ev.loss_out.fill_(7.0)
    rc = N.lib().lgn_step_eval_f64(C.byref(ev.desc), ev._base, ev.enc_off, ev.dec_off, N.ptr(ev.p4), N.ptr(ev.target), N.ptr(ev.mask),
                                   None, N.ptr(ev.workspace), ev._ws - 1, N.ptr(ev.recon), None, None, N.ptr(ev.loss_part),
                                   N.ptr(ev.loss_out), None, None, None, N.stream_ptr())
    torch.cuda.synchronize()
    assert rc != 0 and "workspace" in N.last_error()
    assert bool((ev.recon == 7.0).all()) and ev.loss_out.item() == 7.0


def test_chooser_falls_back_to_the_module_api():
    import __graft_entry__ as G
    from lgn.step import ModuleEvalStep, NativeEvalStep, native_eval_step
    from oracle import lgn_oracle as O
    dev = torch.device(DEV)
    enc, dec = G._models(12, (3, 3, 4, 4), (4, 4, 3, 3), dev, seed=3)
    assert isinstance(native_eval_step(enc, dec, 3, get_real_method="real"), NativeEvalStep)
    enc, dec = G._models(12, (2, 3, 4), (4, 3, 2), dev, seed=3, maxdim=3, jet_features=True)   # refused natively
    st = native_eval_step(enc, dec, 3, get_real_method="real", chamfer_jet_features=True)
    assert isinstance(st, ModuleEvalStep)
    p4, labels = O.synthetic_jets(3, 12, seed=1, pad=True)
    out = st.run({"p4": p4.to(dev), "labels": labels.to(dev)})
    assert out["recon"].shape == (3, 12, 4) and torch.isfinite(out["loss"])
