"""
Device-resident epochs: the loop around the step (utils/train.py:280-345) without host work per batch.

The reference's loop collates a dict per batch on the host, synchronises on ``batch_loss.item()`` every step and appends
reconstruction and target to Python lists.  Here the dataset stays on the device (``DeviceDataset``), the epoch's order is ONE int32
index tensor fixed up front, and an ``EpochRunner`` replays one linear graph per batch

    [ lgn_stage_gather_f64 | the step's native call(s) | lgn_epoch_collect_f64 ]

in which the staging picks each row's jet by index at a batch cursor kept on the device, and the collect kernel adds the step's loss
to the epoch's sum (one fp64 add per step, in step order: the sum the host loop makes of ``.item()`` values), copies the step's
outputs to their place in epoch-sized buffers and advances the cursor.  An epoch is ``ceil(M / B)`` replays and one synchronisation.

Only tensors whose batch axis leads are collected: ``recon`` / ``recon_denorm`` (evaluation steps), ``target`` / ``target_denorm``,
``norm_factor``.  The latent (2, B, ...) is not.

A short last batch: evaluation steps pad it with all-masked jets, as ``NativeEvalStep.run`` does.  Training steps take whole batches
only (``remainder='drop'``, or ``'error'``): the reference trains on the short batch, but the mean-reduced losses carry 1 / B inside
the captured descriptors, so a faithful short batch would need a second plan -- a deliberate difference, not approximated.
"""
import ctypes as C
from typing import Dict, Optional, Sequence

import torch

from . import _native as N

COLLECTABLE = ("recon", "recon_denorm", "target", "target_denorm", "norm_factor")
REMAINDERS = ("drop", "error", "pad")


def _device_f64(t, what: str) -> torch.Tensor:
    if not isinstance(t, torch.Tensor):
        raise ValueError(f"DeviceDataset: data[{what!r}] is a {type(t).__name__}, not a tensor")
    if not t.is_cuda:
        raise ValueError(f"DeviceDataset: data[{what!r}] is on the {t.device.type}; a device-resident dataset holds GPU tensors "
                         "(move the data once with .to('cuda'); there is no CPU fallback)")
    t = t.to(torch.float64).contiguous()
    return t.clone() if t.data_ptr() % 16 else t


def check_index(index: torch.Tensor, M: int) -> torch.Tensor:
    """An explicit epoch order: M integers in [0, M) (any order, repeats allowed).  Min and max are checked once, on the host;
    returns the index.  ValueError otherwise."""
    if not isinstance(index, torch.Tensor) or index.dtype.is_floating_point or index.dtype == torch.bool or index.dim() != 1:
        raise ValueError("the epoch's index is a 1-d integer tensor")
    if index.numel() != M:
        raise ValueError(f"the epoch's index has {index.numel()} entries, the dataset {M} jets")
    lo, hi = int(index.min().item()), int(index.max().item())
    if lo < 0 or hi >= M:
        raise ValueError(f"the epoch's index runs from {lo} to {hi}, outside [0, {M})")
    return index


def epoch_steps(M: int, B: int, remainder: Optional[str], training: bool):
    """(steps, jets covered) of an epoch of M jets in batches of B.  remainder: 'drop' (whole batches only; the default of a training
    step), 'error' (ValueError when M % B != 0), 'pad' (the short last batch is padded with all-masked jets: evaluation steps only,
    and their default)."""
    if remainder is None:
        remainder = "drop" if training else "pad"
    if remainder not in REMAINDERS:
        raise ValueError(f"remainder is one of {REMAINDERS}; got {remainder!r}")
    if training and remainder == "pad":
        raise ValueError("a training step takes whole batches only (its mean-reduced losses carry 1 / B in the captured descriptors): "
                         "remainder is 'drop' or 'error'")
    if M < 1 or B < 1:
        raise ValueError(f"an epoch needs jets and a batch size; got M = {M}, B = {B}")
    if remainder == "error" and M % B:
        raise ValueError(f"{M} jets do not divide into batches of {B} ({M % B} left over) and remainder='error'")
    steps = -(-M // B) if remainder == "pad" else M // B
    if steps == 0:
        raise ValueError(f"{M} jets do not fill one batch of {B}")
    return steps, min(M, steps * B)


class DeviceDataset:
    """The reference's JetDataset (utils/data/dataset.py) held on the device: ``p4`` (M, N, 4), optional ``labels`` / ``masks`` /
    ``mask`` (M, N) and ``scalars`` (M, N [+ 1 with jet_features], K), contiguous, fp64 (masks uint8).  ``num_pts`` (-1: all, <= 1: a
    fraction, else a count) and ``shuffle`` as there: ``perm`` is drawn once, position i of the dataset is row ``perm[i]`` of the data."""

    def __init__(self, data: Dict[str, torch.Tensor], num_pts=-1, shuffle: bool = True, generator: Optional[torch.Generator] = None):
        if "p4" not in data:
            raise ValueError("DeviceDataset: the data has no 'p4'")
        self.p4 = _device_f64(data["p4"], "p4")
        if self.p4.dim() != 3 or self.p4.shape[-1] != 4 or self.p4.shape[0] < 1 or self.p4.shape[1] < 1:
            raise ValueError(f"DeviceDataset: p4 of shape {tuple(self.p4.shape)}; expected (M, N, 4)")
        total, Np = self.p4.shape[0], self.p4.shape[1]
        if total >= 2 ** 31:
            raise ValueError(f"DeviceDataset: {total} jets; the epoch's index is int32")
        self.labels = None
        for key in ("labels", "masks", "mask"):
            if key in data:
                m = data[key]
                if not isinstance(m, torch.Tensor) or not m.is_cuda:
                    raise ValueError(f"DeviceDataset: data[{key!r}] must be a GPU tensor")
                if tuple(m.shape) != (total, Np):
                    raise ValueError(f"DeviceDataset: mask shape {tuple(m.shape)} != {(total, Np)}")
                self.labels = (m.view(torch.uint8) if m.dtype == torch.bool else m.to(torch.uint8)).contiguous()
                break
        self.scalars = None
        if data.get("scalars") is not None:
            self.scalars = _device_f64(data["scalars"], "scalars")
            if self.scalars.dim() != 3 or self.scalars.shape[0] != total:
                raise ValueError(f"DeviceDataset: scalars of shape {tuple(self.scalars.shape)}; expected ({total}, nodes, K)")
        self.device = self.p4.device
        self.total_pts, self.num_pts_param, self.shuffle = total, num_pts, bool(shuffle)
        if num_pts < 0:
            self.num_pts = total
        elif num_pts <= 1:
            self.num_pts = int(num_pts * total)
        else:
            self.num_pts = min(int(num_pts), total)
        if self.num_pts < 1:
            raise ValueError(f"DeviceDataset: num_pts = {num_pts} leaves no jet of {total}")
        perm = torch.randperm(total, generator=generator)[:self.num_pts] if self.shuffle else torch.arange(self.num_pts)
        self.perm = perm.to(self.device)

    def __len__(self) -> int:
        return self.num_pts


class EpochRunner:
    """An epoch of a NativeTrainStep or NativeEvalStep over a DeviceDataset as replays of one graph (module docstring).

    shuffle / generator: every ``run_epoch()`` draws ``torch.randperm(len(dataset), generator=generator)``; without shuffle the order
    is 0 .. M - 1.  ``index`` (here or per ``run_epoch``): an explicit order, checked on the host once (``check_index``).  The order
    in force is ``self.order`` (dataset positions); ``self.index`` holds the data rows (``dataset.perm[order]``), int32, on the device.
    collect: names out of ``COLLECTABLE`` the step has.  remainder: see ``epoch_steps``.  A split step (``step.split``: jet_features /
    extra input scalars -- a maxdim-2 pair, or a table-driven one built with ``table_split=True``) gets its jet node, jet-mass scalar
    and the dataset's ``scalars`` from the same gather launch.

    Where the step is one graph (a single process with ``use_graph``), gather, step and collect are captured together: one launch per
    batch.  Otherwise -- the data-parallel forms with the all-reduce between two graphs, ``use_graph=False``, and the short last batch
    of an evaluation step whose loss is a mean over the real jets -- gather and collect are launched eagerly around ``step.step(None)``
    / ``step.run(None)``: still no host-side data movement.  ``launches_per_epoch`` counts what the last epoch's steps took (graph
    replays, native calls, collectives); the one lgn_epoch_reset launch ahead of them is not in it.

    ``run_epoch()`` returns {'loss_sum', 'steps', 'avg_loss' (= loss_sum / steps, the reference's epoch_total_loss / len(loader)),
    'status' (0, or LGN_EPOCH_BAD_INDEX), 'collected': {name: (jets covered, ...) tensor}}.  The collected tensors are the runner's
    buffers: the next epoch overwrites them."""

    def __init__(self, step, dataset: DeviceDataset, shuffle: bool = True, generator: Optional[torch.Generator] = None,
                 collect: Sequence[str] = (), remainder: Optional[str] = None, index: Optional[torch.Tensor] = None):
        from .step import NativeEvalStep, NativeTrainStep
        if not isinstance(step, (NativeTrainStep, NativeEvalStep)):
            raise TypeError(f"EpochRunner drives a NativeTrainStep or a NativeEvalStep (static buffers, native calls); got "
                            f"{type(step).__name__}")
        if not isinstance(dataset, DeviceDataset):
            raise TypeError(f"EpochRunner takes a DeviceDataset; got {type(dataset).__name__}")
        self.step, self.dataset, self.training = step, dataset, isinstance(step, NativeTrainStep)
        self.shuffle, self.generator = bool(shuffle), generator
        i = step.inputs
        self.B, self.M = int(i.B), len(dataset)
        dev = i.p4.device
        if dataset.device != dev:
            raise ValueError(f"the dataset is on {dataset.device}, the step on {dev}")
        if tuple(dataset.p4.shape[1:]) != tuple(step.target.shape[1:]):
            raise ValueError(f"the step was built for jets of shape {tuple(step.target.shape[1:])}, the dataset holds "
                             f"{tuple(dataset.p4.shape[1:])}")
        self.steps, self.count = epoch_steps(self.M, self.B, remainder, self.training)
        jet = bool(step.split and getattr(step.encoder, "jet_features", False))
        K = (i.in_scalars.shape[-1] if i.in_scalars is not None else 0) - int(jet)
        scalars = dataset.scalars if step.split and K > 0 else None
        if K > 0 and (scalars is None or tuple(scalars.shape[1:]) != (i.p4.shape[1], K)):
            raise ValueError(f"the encoder takes {K} extra input scalars per node: the dataset needs 'scalars' of shape "
                             f"(M, {i.p4.shape[1]}, {K})")
        # the order of the epoch (static: the graph holds its pointer) and the epoch's state on the device
        self.index = torch.zeros(self.M, device=dev, dtype=torch.int32)
        self.order = None
        self._cursor = torch.zeros(2, device=dev, dtype=torch.int64)
        self._epoch = torch.zeros(2, device=dev, dtype=torch.float64)
        self._status = torch.zeros(1, device=dev, dtype=torch.int32)
        code = i.norm_code if i.normalize else N.NORM_NONE
        self._gather_args = (N.ptr(dataset.p4), N.ptr(dataset.labels), N.ptr(scalars), dataset.total_pts, N.ptr(self.index), self.count,
                             N.ptr(self._cursor), self.B, dataset.p4.shape[1], int(code), float(step.encoder.scale), int(jet),
                             max(K, 0), N.ptr(i.p4), N.ptr(i.target), N.ptr(i.mask), N.ptr(i.in_scalars), N.ptr(i.norm_factor),
                             N.ptr(self._status))
        self._keep = (dataset.p4, dataset.labels, scalars)
        # what is collected: static (B, ...) tensors of the step -> (count, ...) buffers
        names = [collect] if isinstance(collect, str) else list(collect)
        if len(names) > N.EPOCH_MAX_COLLECT or len(set(names)) != len(names):
            raise ValueError(f"collect takes up to {N.EPOCH_MAX_COLLECT} different names out of {COLLECTABLE}; got {names}")
        self._sources, self.collected = [], {}
        for name in names:
            src = getattr(step, name, None) if name in COLLECTABLE else None
            if name == "recon" and self.training:
                raise ValueError("a training step's reconstruction is (2, B, N, 4): its batch axis does not lead, it cannot be collected "
                                 "(collect 'recon' from an evaluation step)")
            if src is None:
                raise ValueError(f"collect: {name!r} is not a tensor this step has (of {COLLECTABLE}; the *_denorm ones need normalize)")
            self._sources.append(src)
            self.collected[name] = torch.zeros((self.count,) + tuple(src.shape[1:]), device=dev, dtype=src.dtype)
        n = len(names)
        self._src = (C.c_void_p * max(n, 1))(*[N.ptr(t) for t in self._sources])
        self._dst = (C.c_void_p * max(n, 1))(*[N.ptr(self.collected[k]) for k in names])
        self._rd = (C.c_int * max(n, 1))(*[t[0].numel() for t in self._sources])
        self._n = n
        self._graph = None
        self.launches_per_epoch = None
        if index is not None:
            index = check_index(index, self.M)
        self._fixed_index = index

    # -- the three native calls on the current stream
    def _reset(self):
        N._check(N.lib().lgn_epoch_reset(N.ptr(self._cursor), N.ptr(self._epoch), N.ptr(self._status), N.stream_ptr()), "lgn_epoch_reset")

    def _gather(self):
        N._check(N.lib().lgn_stage_gather_f64(*self._gather_args, N.stream_ptr()), "lgn_stage_gather_f64")

    def _collect(self):
        N._check(N.lib().lgn_epoch_collect_f64(N.ptr(self.step.loss_out), N.ptr(self._epoch), N.ptr(self._cursor), self.count, self.B,
                                               self._n, self._src, self._dst, self._rd, N.stream_ptr()), "lgn_epoch_collect_f64")

    @property
    def single_graph(self) -> bool:
        """Is the step one graph, so that gather, step and collect are captured together?"""
        s = self.step
        return bool(s.use_graph and not (self.training and s.collective))

    def _capture(self):
        from .step import _capturing, _warm_up
        s = self.step
        snap = s.opt_state.snapshot() if self.training else None

        def once():
            self._reset()
            self._gather()
            s.enqueue(False) if self.training else s.enqueue()
            self._collect()

        _warm_up(once)
        self._graph = torch.cuda.CUDAGraph()
        with _capturing(self._graph):
            self._gather()
            s.enqueue()
            self._collect()
        if snap is not None:
            s.opt_state.restore(snap)

    def _set_order(self, index: Optional[torch.Tensor]):
        dev = self.index.device
        if index is not None:
            order = check_index(index, self.M)
        elif self._fixed_index is not None:
            order = self._fixed_index
        elif self.shuffle:
            order = torch.randperm(self.M, generator=self.generator,
                                   device=self.generator.device if self.generator is not None else dev)
        else:
            order = torch.arange(self.M, device=dev)
        self.order = order.to(dev)
        self.index.copy_(self.dataset.perm[self.order.long()])

    def _eager_step(self, n: int) -> int:
        """gather | step.step(None) / step.run(None) | collect, launched one by one; returns the launches it took."""
        s = self.step
        self._gather()
        if self.training:
            s.step(None)
            inner = s.launches_per_step if s.use_graph else (3 if s.collective else 1)
        else:
            s.n_real = n
            s.run(None)
            inner = 2 if s.normalize and not s.use_graph else 1
        self._collect()
        return 2 + inner

    def run_epoch(self, index: Optional[torch.Tensor] = None) -> dict:
        s = self.step
        self._set_order(index)
        if not self.training and s._follow_params():
            self._graph = None               # the parameter blocks moved: the step re-planned, its calls have new arguments
        tail = self.count - (self.steps - 1) * self.B          # jets of the last batch
        # the means of an evaluation step (jet-feature MSE, mse / hungarian) run over the real jets: its short batch is a call of its
        # own descriptors, outside any graph (the EMD loss stage is a sum over the jets, like Chamfer: no such call)
        eager_tail = not self.training and tail < self.B and (s.chamfer_jet_features or
                                                              s.loss_kind in (s.N.LOSS_MSE, s.N.LOSS_HUNGARIAN))
        if self.single_graph and self._graph is None:
            self._capture()
        self._reset()
        launches = 0
        for it in range(self.steps):
            n = tail if it == self.steps - 1 else self.B
            if self.single_graph and not (eager_tail and n < self.B):
                self._graph.replay()
                launches += 1
            else:
                launches += self._eager_step(n)
        if not self.training:
            s.n_real = tail
        torch.cuda.current_stream().synchronize()          # the epoch's one synchronisation
        loss_sum, steps = self._epoch.tolist()
        status = int(self._status.item())
        if int(steps) != self.steps or int(self._cursor[0].item()) != self.steps:
            raise RuntimeError(f"the epoch counted {steps} steps on the device, {self.steps} were launched")
        self.launches_per_epoch = launches
        return {"loss_sum": loss_sum, "steps": int(steps), "avg_loss": loss_sum / steps, "status": status,
                "collected": dict(self.collected)}
