"""GPU tests of the whole-step call's loss options (lgn_net_desc.get_real / jet_loss_scale, ABI 18): every --get-real-method and
--chamfer-jet-features run inside the step's last kernel -- against the oracle, against the reference's g17 vectors, on both decoder
tails (riding on the last level forward, a kernel of its own), on the split step, through the chooser, and on two ranks."""
import functools
import os

import pytest
import torch

import _util as U

pytestmark = pytest.mark.gpu

METHODS = ["real", "imag", "sum", "mean", "norm"]
# (maxdim, N, B): maxdim 2 at 12 particles (the loss rides on the decoder's last level_fwd2) and at 50 (> 40: dec_output_loss_kernel on
# its own); maxdim 3 (the table-driven step: dec_output_loss_kernel)
NETS = {"md2_n12": (2, 12, 3), "md2_n50": (2, 50, 2), "md3_n12": (3, 12, 2)}
CH = {2: ((3, 3, 4, 4), (4, 4, 3, 3)), 3: ((2, 3, 4), (4, 3, 2))}


def _models(net, seed=21):
    import __graft_entry__ as G
    maxdim, N, _ = NETS[net]
    return G._models(N, CH[maxdim][0], CH[maxdim][1], torch.device("cuda:0"), seed=seed, maxdim=maxdim)


def _batch(net):
    from oracle import lgn_oracle as O
    _, N, B = NETS[net]
    return O.synthetic_jets(B, N, seed=N + B, pad=True)


_jet_mse = U.jet_mse


@functools.lru_cache(maxsize=None)
def _oracle(net, method, jet):
    """(loss, recon, {'enc.<name>' / 'dec.<name>': gradient or None}) of the CPU oracle."""
    from oracle import lgn_oracle as O
    maxdim, N, _ = NETS[net]
    enc, dec = _models(net)
    p4, labels = _batch(net)
    Pe = {k: v.detach().cpu().clone().requires_grad_(True) for k, v in enc.state_dict().items()}
    Pd = {k: v.detach().cpu().clone().requires_grad_(True) for k, v in dec.state_dict().items()}
    ce = O.NetConfig(num_particles=N, maxdim=maxdim, num_channels=CH[maxdim][0])
    cd = O.NetConfig(num_particles=N, maxdim=maxdim, num_channels=CH[maxdim][1])
    rec = O.decoder_forward(Pd, cd, O.encoder_forward(Pe, ce, p4, labels))
    x = O.get_real(rec, method)
    loss = O.chamfer_loss(x, p4)
    if jet:
        loss = loss + _jet_mse(x, p4)
    loss.backward()
    return loss.detach(), rec.detach(), {f"{pre}.{k}": q.grad for pre, P in (("enc", Pe), ("dec", Pd)) for k, q in P.items()}


@pytest.mark.parametrize("use_graph", [False, True])
@pytest.mark.parametrize("net", list(NETS))
@pytest.mark.parametrize("jet", [False, True])
@pytest.mark.parametrize("method", METHODS)
def test_native_step_loss_options_match_oracle(method, jet, net, use_graph):
    from lgn.step import NativeTrainStep
    enc, dec = _models(net)
    p4, labels = _batch(net)
    _, _, B = NETS[net]
    step = NativeTrainStep(enc, dec, batch_size=B, l1_lambda=0.0, optimizer=False, use_graph=use_graph, get_real_method=method,
                           chamfer_jet_features=jet)
    batch = {"p4": p4.to("cuda:0"), "labels": labels.to("cuda:0")}
    for _ in range(2):                      # (with the graph: capture, then a replay on the same buffers)
        loss, recon = step.step(batch)
    loss_o, rec_o, grads_o = _oracle(net, method, jet)
    U.assert_close(loss, loss_o, 1e-10, "loss")
    U.assert_close(recon, rec_o, 1e-10, "recon")
    U.assert_named_grads_close(U.named_grads(enc, dec), grads_o, 1e-10, f"{net} {method} jet {jet}")


def test_method_names_match_without_regard_to_case_and_unknown_means_real(caplog):
    from lgn.step import NativeTrainStep
    codes = {}
    for name in ("NORM", "Mean", "bogus"):
        enc, dec = _models("md2_n12")
        with caplog.at_level("WARNING"):
            codes[name] = NativeTrainStep(enc, dec, batch_size=3, optimizer=False, get_real_method=name).desc.get_real
    assert codes == {"NORM": 4, "Mean": 3, "bogus": 1}
    assert any("bogus" in r.getMessage() for r in caplog.records)


@pytest.mark.parametrize("use_graph", [False, True])
@pytest.mark.parametrize("name", ["g17_real_maxdim2.npz", "g17_norm_maxdim2.npz", "g17_realjet_maxdim2.npz", "g17_real_maxdim3.npz",
                                  "g17_norm_maxdim3.npz", "g17_realjet_maxdim3.npz"])
def test_native_step_loss_options_match_reference_golden(name, use_graph):
    """The reference's loss, reconstruction and every parameter gradient with get_real 'real' / 'norm' and the jet-feature MSE."""
    import __graft_entry__ as G
    from lgn.step import NativeTrainStep, native_train_step
    dev = torch.device("cuda:0")
    z = U.load(name)
    m = U.meta(z)
    enc, dec = G._models(m["N"], m["ch_enc"], m["ch_dec"], dev, seed=m["seed"], maxdim=m["maxdim"])
    batch = {"p4": torch.from_numpy(z["p4"]).to(dev), "labels": torch.from_numpy(z["labels"]).to(dev)}
    step = native_train_step(enc, dec, m["B"], l1_lambda=0.0, optimizer=False, use_graph=use_graph,
                             get_real_method=m["get_real_method"], chamfer_jet_features=m["chamfer_jet_features"])
    assert isinstance(step, NativeTrainStep)
    for _ in range(2):
        loss, recon = step.step(batch)
    U.assert_close(loss, z["loss"], 1e-11, "loss")
    U.assert_close(recon, z["recon"], 1e-11, "recon")
    # (parameters whose gradient is ~1e-15 -- a cancellation -- are held to the network's gradient scale, not to their own size)
    scale = max(float(abs(z[k]).max()) for k in z.files if k.startswith("grad."))
    for pre, mod in (("enc", enc), ("dec", dec)):
        for k, g in mod.named_grads():
            U.assert_close_scaled(g, torch.from_numpy(z[f"grad.{pre}.{k}"]), 1e-9, scale, f"grad {pre}.{k}")


@pytest.mark.parametrize("method", ["real", "norm"])
def test_split_step_with_jet_loss_matches_captured_module_step(method):
    """An encoder with jet_features (the split form of the whole step: one node more than the decoder reconstructs) with the
    jet-feature loss, against the module-API step under autograd (lgn.losses.ChamferLoss) on the same weights."""
    import __graft_entry__ as G
    from lgn.step import CapturedModuleStep, NativeTrainStep
    from oracle import lgn_oracle as O
    dev = torch.device("cuda:0")
    N, B = 12, 3
    nets = [G._models(N, (3, 3, 4, 4), (4, 4, 3, 3), dev, seed=9, jet_features=True) for _ in range(2)]
    p4, labels = O.synthetic_jets(B, N, seed=4, pad=True)
    batch = {"p4": p4.to(dev), "labels": labels.to(dev)}
    a = NativeTrainStep(*nets[0], batch_size=B, l1_lambda=0.0, optimizer=False, use_graph=True, get_real_method=method,
                        chamfer_jet_features=True)
    assert a.split
    b = CapturedModuleStep(*nets[1], batch_size=B, l1_lambda=0.0, optimizer=False, use_graph=False, get_real_method=method,
                           chamfer_jet_features=True)
    for _ in range(2):
        la, ra = a.step(batch)
    lb, rb = b.step(batch)
    U.assert_close(la, lb, 1e-11, "loss")
    U.assert_close(ra, rb, 1e-11, "recon")
    U.assert_close(a.flat.grad, b.flat.grad, 1e-9, "flat gradient")


def test_chooser_takes_the_native_step_for_loss_options():
    """native_train_step(..., get_real_method='real', chamfer_jet_features=True) is the whole-step call, and three Adam steps of it
    train like CapturedModuleStep with the same options."""
    from lgn.step import CapturedModuleStep, NativeTrainStep, native_train_step
    import __graft_entry__ as G
    from oracle import lgn_oracle as O
    dev = torch.device("cuda:0")
    N, B = 30, 4
    nets = [G._models(N, (3, 3, 4, 4), (4, 4, 3, 3), dev, seed=0) for _ in range(2)]
    p4, labels = O.synthetic_jets(B, N, seed=3, pad=True)
    batch = {"p4": p4.to(dev), "labels": labels.to(dev)}
    opts = dict(lr=5e-4, l1_lambda=1e-8, use_graph=True, get_real_method="real", chamfer_jet_features=True)
    a = native_train_step(*nets[0], B, **opts)
    assert isinstance(a, NativeTrainStep)
    b = CapturedModuleStep(*nets[1], B, **opts)
    for it in range(3):
        la, _ = a.step(batch)
        lb, _ = b.step(batch)
        U.assert_close(la, lb, 1e-9, f"loss at step {it}")
    U.assert_close(a.flat.flat, b.flat.flat, 1e-9, "parameters after 3 Adam steps")


def test_two_ranks_with_jet_loss_match_single_process(tmp_path):
    """2 ranks x 8 jets with the jet-feature MSE (each rank weighs its jets by 1 / (4 x 16)) reproduce one process on all 16 jets."""
    import socket
    import subprocess
    import sys as _sys
    import bench
    import __graft_entry__ as G
    from lgn.step import NativeTrainStep
    dev = torch.device("cuda:0")
    per_rank, world, steps = 8, 2, 3
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    worker = os.path.join(os.path.dirname(os.path.abspath(__file__)), "_dist_loss_options_worker.py")
    procs = [subprocess.Popen([_sys.executable, worker, str(r), str(world), str(port), str(tmp_path), str(per_rank), str(steps)],
                              stdout=subprocess.PIPE, stderr=subprocess.STDOUT) for r in range(world)]
    outs = [p.communicate(timeout=600)[0].decode(errors="replace") for p in procs]
    for r, (p, o) in enumerate(zip(procs, outs)):
        assert p.returncode == 0, f"rank {r} failed:\n{o[-3000:]}"
    enc, dec = G._models(bench.N_PART, bench.CH_ENC, bench.CH_DEC, dev, seed=0)
    ref = NativeTrainStep(enc, dec, batch_size=per_rank * world, lr=5e-4, l1_lambda=1e-8, use_graph=True, get_real_method="real",
                          chamfer_jet_features=True)
    p4, labels = bench.synthetic_jets(per_rank * world, bench.N_PART, seed=5)
    batch = {"p4": p4.to(dev), "labels": labels.to(dev)}
    ref_losses = [float(ref.step(batch)[0]) for _ in range(steps)]
    for r in range(world):
        z = torch.load(os.path.join(str(tmp_path), f"rank{r}.pt"))
        U.assert_close(z["params"].to(dev), ref.flat.flat.detach(), 1e-9, f"rank {r} parameters after {steps} steps")
        for a, b in zip(z["losses"], ref_losses):
            assert abs(a - b) <= 1e-10 * max(1.0, abs(b)), (z["losses"], ref_losses)


@pytest.mark.parametrize("cls", ["native", "native_collective", "captured"])
def test_step_graphs_are_captured_in_thread_local_mode(cls, monkeypatch):
    """Every step graph is captured with capture_error_mode='thread_local': under the default 'global' mode, the HIP event polls
    of a live process group's watchdog thread that land inside a capture window are errors there, and abort the process."""
    import __graft_entry__ as G
    from lgn.step import CapturedModuleStep, NativeTrainStep
    from oracle import lgn_oracle as O
    modes = []
    real = torch.cuda.graph

    def spy(*a, **kw):
        modes.append(kw.get("capture_error_mode", "global"))
        return real(*a, **kw)

    monkeypatch.setattr(torch.cuda, "graph", spy)
    dev = torch.device("cuda:0")
    enc, dec = G._models(12, (2, 2, 3, 3), (3, 3, 2, 2), dev, seed=2)
    p4, labels = O.synthetic_jets(3, 12, seed=1, pad=True)
    import torch.distributed as dist
    if cls == "native_collective":      # a one-rank gloo group: the two-graph form with the all-reduce between the graphs
        import socket
        with socket.socket() as sk:
            sk.bind(("127.0.0.1", 0))
            port = sk.getsockname()[1]
        dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=0, world_size=1)
    try:
        if cls == "captured":
            st = CapturedModuleStep(enc, dec, batch_size=3, use_graph=True, get_real_method="real", chamfer_jet_features=True)
        else:
            st = NativeTrainStep(enc, dec, batch_size=3, use_graph=True, force_collective=cls == "native_collective")
        st.step({"p4": p4.to(dev), "labels": labels.to(dev)})
        torch.cuda.synchronize()
    finally:
        if cls == "native_collective":
            dist.destroy_process_group()
    assert modes and all(m == "thread_local" for m in modes), modes
