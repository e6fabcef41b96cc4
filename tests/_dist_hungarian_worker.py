"""Worker of tests/test_gpu_hungarian_loss.py::test_two_ranks_match_single_process: one rank of a 2-rank data-parallel training step
with --loss-choice mse / hungarian.  Both ranks share the one GPU of the test box and talk over gloo (RCCL refuses two ranks on one
device).  The test imports build() / batch() / params() for its single-process reference.
    python _dist_hungarian_worker.py RANK WORLD PORT OUTDIR JETS_PER_RANK STEPS KIND(native|captured|loop) LOSS"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "lgn-autoencoder_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

N_PART, CH_ENC, CH_DEC = 12, (3, 3, 4, 4), (4, 4, 3, 3)


def build(kind, choice, batch_size):
    """(step, encoder, decoder): l1_lambda is large enough for the L1 term's 1 / world weighting to show in the parameters."""
    import __graft_entry__ as G
    from lgn.step import CapturedModuleStep, NativeTrainStep, ReferenceLoopStep
    dev = torch.device("cuda:0")
    enc, dec = G._models(N_PART, CH_ENC, CH_DEC, dev, seed=0)
    frame = dict(hungarian_abs_coord=False, hungarian_polar_coord=True) if choice.endswith("rel_polar") else {}
    opts = dict(lr=5e-4, l1_lambda=1e-6, get_real_method="real", loss_choice=choice.split("_")[0], **frame)
    if kind == "native":
        step = NativeTrainStep(enc, dec, batch_size=batch_size, use_graph=True, **opts)
    elif kind == "captured":
        step = CapturedModuleStep(enc, dec, batch_size=batch_size, use_graph=True, **opts)
    else:
        step = ReferenceLoopStep(enc, dec, **opts)
    return step, enc, dec


def batch(total, sl):
    from oracle import lgn_oracle as O
    p4, labels = O.synthetic_jets(total, N_PART, seed=5, pad=False)
    return {"p4": p4[sl].to("cuda:0"), "labels": labels[sl].to("cuda:0")}


def params(enc, dec):
    return torch.cat([p.detach().reshape(-1).cpu() for m in (enc, dec) for p in m.parameters()])


def main():
    import torch.distributed as dist
    rank, world, port, outdir, per_rank, steps = int(sys.argv[1]), int(sys.argv[2]), sys.argv[3], sys.argv[4], int(sys.argv[5]), int(sys.argv[6])
    kind, choice = sys.argv[7], sys.argv[8]
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = port
    dist.init_process_group("gloo", rank=rank, world_size=world)
    step, enc, dec = build(kind, choice, per_rank)
    assert step.world == world
    b = batch(per_rank * world, slice(rank * per_rank, (rank + 1) * per_rank))
    losses = [float(step.step(b)[0]) for _ in range(steps)]
    torch.cuda.synchronize()
    torch.save({"params": params(enc, dec), "losses": losses}, os.path.join(outdir, f"rank{rank}.pt"))
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
