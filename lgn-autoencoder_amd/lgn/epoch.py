"""
Device-resident epochs: the loop around the step (utils/train.py:280-345) without host work per batch.

The reference's loop collates a dict per batch on the host, synchronises on ``batch_loss.item()`` every step and appends
reconstruction and target to Python lists.  Here the dataset stays on the device (``DeviceDataset``), the epoch's order is ONE int32
index tensor fixed up front, and an ``EpochRunner`` replays one linear graph per batch

    [ lgn_stage_gather_f64 | the step's native call(s) | lgn_epoch_collect_f64 ]

in which the staging picks each row's jet by index at a batch cursor kept on the device, and the collect kernel adds the step's loss
to the epoch's sum (one fp64 add per step, in step order: the sum the host loop makes of ``.item()`` values), copies the step's
outputs to their place in epoch-sized buffers and advances the cursor.  An epoch is ``ceil(M / B)`` replays and one synchronisation.

Collected are the tensors whose batch axis leads -- ``recon`` / ``recon_denorm`` (evaluation steps), ``target`` / ``target_denorm``,
``norm_factor`` -- and the ``latent`` of an evaluation step built with keep_latent, (2, B, ...) per part: each of its two planes is a
run of its own (lgn_epoch_collect_planes_f64), and the epoch's {(0, 0): (2, M, ...), (1, 1): (2, M, ...)} is the reference's
latent_dict (utils/train.py:302-365, torch.cat(v, dim=1)).

A short last batch: evaluation steps pad it with all-masked jets, as ``NativeEvalStep.run`` does.  Training steps drop it by default
(``remainder='drop'``, or ``'error'``).  With ``remainder='short'`` they train on it as the reference's DataLoader does: the
mean-reduced losses carry 1 / B inside the captured descriptors, so the last M mod B = r jets are a step of a second plan built for r
jets (``NativeTrainStep.short_step(r)``: 1 / r in its descriptors, the full step's parameters and optimiser state), captured into a
second graph [ lgn_stage_gather_at_f64 | short step | lgn_epoch_collect_planes_f64 ] and replayed once behind the M // B replays of
the first; the loss sum stays one add per step and ``avg_loss`` divides by ceil(M / B) = len(loader).  A padded batch would not do:
padded jets are not loss-neutral under get_real_method='norm', and a batch of B runs other launch regimes than one of r.
"""
import ctypes as C
from typing import Dict, Optional, Sequence

import torch

from . import _native as N

COLLECTABLE = ("recon", "recon_denorm", "target", "target_denorm", "norm_factor", "latent")
REMAINDERS = ("drop", "error", "pad", "short")


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
    and their default), 'short' (the short last batch is a training step of its own on M % B jets: training steps only)."""
    if remainder is None:
        remainder = "drop" if training else "pad"
    if remainder not in REMAINDERS:
        raise ValueError(f"remainder is one of {REMAINDERS}; got {remainder!r}")
    if training and remainder == "pad":
        raise ValueError("a training step's plan takes whole batches only (its mean-reduced losses carry 1 / B in the captured "
                         "descriptors, and padded jets are not loss-neutral): remainder is 'drop', 'error' or 'short'")
    if not training and remainder == "short":
        raise ValueError("an evaluation step covers its short last batch by padding it with all-masked jets: remainder is 'pad' there "
                         "(or 'drop', 'error'); 'short' is the second plan of a training step")
    if M < 1 or B < 1:
        raise ValueError(f"an epoch needs jets and a batch size; got M = {M}, B = {B}")
    if remainder == "error" and M % B:
        raise ValueError(f"{M} jets do not divide into batches of {B} ({M % B} left over) and remainder='error'")
    steps = -(-M // B) if remainder in ("pad", "short") else M // B
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


class _Plan:
    """One [gather | step | collect] of a runner with every argument fixed: the full batch's step with the calls of the first ABI of
    the epochs (``base`` None, no latent), or -- for the latent, [2][B][...], and for the short last batch's step behind the full
    ones -- lgn_stage_gather_at_f64 / lgn_epoch_collect_planes_f64 with their base row.  ``graph``: the three captured together."""

    def __init__(self, runner, step, base: Optional[int], sources):
        i = step.inputs
        ds, self.step, self.B, self.graph = runner.dataset, step, int(i.B), None
        jet, K, scalars = runner._jet, runner._K, runner._scalars
        code = i.norm_code if i.normalize else N.NORM_NONE
        at = () if base is None else (int(base),)
        self._gather = ("lgn_stage_gather_f64" if base is None else "lgn_stage_gather_at_f64",
                        (N.ptr(ds.p4), N.ptr(ds.labels), N.ptr(scalars), ds.total_pts, N.ptr(runner.index), runner.count) + at +
                        (N.ptr(runner._cursor), self.B, ds.p4.shape[1], int(code), float(step.encoder.scale), int(jet), max(K, 0),
                         N.ptr(i.p4), N.ptr(i.target), N.ptr(i.mask), N.ptr(i.in_scalars), N.ptr(i.norm_factor), N.ptr(runner._status)))
        # what is collected: static ([planes,] B, ...) tensors of this step -> the runner's ([planes,] count, ...) buffers
        n = len(sources)
        src = [getattr(step, attr) for attr, _, _ in sources]
        arrays = ((C.c_void_p * max(n, 1))(*[N.ptr(t) for t in src]), (C.c_void_p * max(n, 1))(*[N.ptr(dst) for _, _, dst in sources]),
                  (C.c_int * max(n, 1))(*[t.numel() // (planes * self.B) for t, (_, planes, _) in zip(src, sources)]))
        head = (N.ptr(step.loss_out), N.ptr(runner._epoch), N.ptr(runner._cursor), runner.count)
        if base is None and all(planes == 1 for _, planes, _ in sources):
            self._collect = ("lgn_epoch_collect_f64", head + (self.B, n) + arrays)
        else:
            self._collect = ("lgn_epoch_collect_planes_f64", head + (int(base or 0), self.B, n) + arrays +
                             ((C.c_int * max(n, 1))(*[planes for _, planes, _ in sources]),))
        self._keep = src

    def gather(self):
        name, args = self._gather
        N._check(getattr(N.lib(), name)(*args, N.stream_ptr()), name)

    def collect(self):
        name, args = self._collect
        N._check(getattr(N.lib(), name)(*args, N.stream_ptr()), name)


class EpochRunner:
    """An epoch of a NativeTrainStep or NativeEvalStep over a DeviceDataset as replays of one graph (module docstring).

    shuffle / generator: every ``run_epoch()`` draws ``torch.randperm(len(dataset), generator=generator)``; without shuffle the order
    is 0 .. M - 1.  ``index`` (here or per ``run_epoch``): an explicit order, checked on the host once (``check_index``).  The order
    in force is ``self.order`` (dataset positions); ``self.index`` holds the data rows (``dataset.perm[order]``), int32, on the device.
    collect: names out of ``COLLECTABLE`` the step has ('latent': an evaluation step built with keep_latent; it takes two of the
    LGN_EPOCH_MAX_COLLECT slots).  remainder: see ``epoch_steps``.  A split step (``step.split``: jet_features /
    extra input scalars -- a maxdim-2 pair, or a table-driven one built with ``table_split=True``) gets its jet node, jet-mass scalar
    and the dataset's ``scalars`` from the same gather launch.

    Where the step is one graph (a single process with ``use_graph``), gather, step and collect are captured together: one launch per
    batch.  Otherwise -- the data-parallel forms with the all-reduce between two graphs, ``use_graph=False``, and the short last batch
    of an evaluation step whose loss is a mean over the real jets -- gather and collect are launched eagerly around ``step.step(None)``
    / ``step.run(None)``: still no host-side data movement.  ``remainder='short'`` (training): the M mod B jets behind the whole
    batches are one more step, ``step.short_step(M mod B)``, in a second graph of the same three parts (eagerly without
    ``use_graph``), replayed once behind the replays of the first.  ``launches_per_epoch`` counts what the last epoch's steps took
    (graph replays, native calls, collectives); the one lgn_epoch_reset launch ahead of them is not in it.

    ``run_epoch()`` returns {'loss_sum', 'steps', 'avg_loss' (= loss_sum / steps, the reference's epoch_total_loss / len(loader)),
    'status' (0, or LGN_EPOCH_BAD_INDEX), 'collected': {name: (jets covered, ...) tensor; 'latent': {(0, 0): (2, jets covered, ...),
    (1, 1): (2, jets covered, ...)}, the layout of the reference's latent_dict}}.  The collected tensors are the runner's buffers:
    the next epoch overwrites them.

    A guarded training step (NativeTrainStep built with max_grad_norm / skip_nonfinite / blow_up_threshold / lr_schedule): the
    running fields of its control block are cleared with the epoch's own reset and come back as 'control': {applied, clipped,
    skipped, first_skipped, grad_norm_max, applied_loss_sum}, read at the same synchronisation.  'loss_sum' / 'avg_loss' stay the
    plain sum over all steps, a skipped step's NaN included (what the reference's loop would print); applied_loss_sum / applied is
    the figure to use."""

    def __init__(self, step, dataset: DeviceDataset, shuffle: bool = True, generator: Optional[torch.Generator] = None,
                 collect: Sequence[str] = (), remainder: Optional[str] = None, index: Optional[torch.Tensor] = None):
        from .step import NativeEvalStep, NativeTrainStep
        if not isinstance(step, (NativeTrainStep, NativeEvalStep)):
            raise TypeError(f"EpochRunner drives a NativeTrainStep or a NativeEvalStep (static buffers, native calls); got "
                            f"{type(step).__name__}")
        self.training = isinstance(step, NativeTrainStep)
        if self.training and remainder == "short" and step.collective:
            raise ValueError("remainder='short' with a data-parallel step: the short last batch would have to be split over the ranks; "
                             "remainder is 'drop' or 'error' there")
        if not isinstance(dataset, DeviceDataset):
            raise TypeError(f"EpochRunner takes a DeviceDataset; got {type(dataset).__name__}")
        self.step, self.dataset = step, dataset
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
        # the jets of the short last batch that is a step of its own (remainder='short'), behind self.full whole batches
        self.full = self.M // self.B
        self.short = self.M - self.full * self.B if remainder == "short" else 0
        self._jet = jet = bool(step.split and getattr(step.encoder, "jet_features", False))
        self._K = K = (i.in_scalars.shape[-1] if i.in_scalars is not None else 0) - int(jet)
        self._scalars = scalars = dataset.scalars if step.split and K > 0 else None
        if K > 0 and (scalars is None or tuple(scalars.shape[1:]) != (i.p4.shape[1], K)):
            raise ValueError(f"the encoder takes {K} extra input scalars per node: the dataset needs 'scalars' of shape "
                             f"(M, {i.p4.shape[1]}, {K})")
        # the order of the epoch (static: the graphs hold its pointer) and the epoch's state on the device
        self.index = torch.zeros(self.M, device=dev, dtype=torch.int32)
        self.order = None
        self._cursor = torch.zeros(2, device=dev, dtype=torch.int64)
        self._epoch = torch.zeros(2, device=dev, dtype=torch.float64)
        self._status = torch.zeros(1, device=dev, dtype=torch.int32)
        # what is collected: (attribute of the step, planes ahead of its batch axis, the epoch's buffer)
        names = [collect] if isinstance(collect, str) else list(collect)
        if len(names) + int("latent" in names) > N.EPOCH_MAX_COLLECT or len(set(names)) != len(names):
            raise ValueError(f"collect takes up to {N.EPOCH_MAX_COLLECT} different names out of {COLLECTABLE} ('latent' counts as two); "
                             f"got {names}")
        self._sources, self.collected = [], {}
        for name in names:
            if name == "latent":
                if self.training or not step.keep_latent:
                    raise ValueError("collect: 'latent' is what a NativeEvalStep built with keep_latent=True produces" +
                                     (" (a training step keeps no latent)" if self.training else ""))
                self.collected[name] = {}
                for key, attr in (((0, 0), "lat_s"), ((1, 1), "lat_v")):
                    src = getattr(step, attr)
                    buf = torch.zeros((src.shape[0], self.count) + tuple(src.shape[2:]), device=dev, dtype=src.dtype)
                    self.collected[name][key] = buf
                    self._sources.append((attr, int(src.shape[0]), buf))
                continue
            src = getattr(step, name, None) if name in COLLECTABLE else None
            if name == "recon" and self.training:
                raise ValueError("a training step's reconstruction is (2, B, N, 4): its batch axis does not lead, it cannot be collected "
                                 "(collect 'recon' from an evaluation step)")
            if src is None:
                raise ValueError(f"collect: {name!r} is not a tensor this step has (of {COLLECTABLE}; the *_denorm ones need normalize)")
            self.collected[name] = torch.zeros((self.count,) + tuple(src.shape[1:]), device=dev, dtype=src.dtype)
            self._sources.append((name, 1, self.collected[name]))
        self._main = _Plan(self, step, None, self._sources)
        self._tail = None                    # the short last batch's plan: built with its step, at the first epoch
        self.launches_per_epoch = None
        if index is not None:
            index = check_index(index, self.M)
        self._fixed_index = index

    def _reset(self):
        N._check(N.lib().lgn_epoch_reset(N.ptr(self._cursor), N.ptr(self._epoch), N.ptr(self._status), N.stream_ptr()), "lgn_epoch_reset")

    @property
    def single_graph(self) -> bool:
        """Is the step one graph, so that gather, step and collect are captured together?"""
        s = self.step
        return bool(s.use_graph and not (self.training and s.collective))

    def _short_plan(self) -> _Plan:
        """The plan of the short last batch: step.short_step(r) on rows full * B .. of the order.  Its calls see the cursor at
        `full`, in units of their own batch size r: base = full * (B - r) puts row b at full * B + b."""
        if self._tail is None:
            self._tail = _Plan(self, self.step.short_step(self.short), self.full * (self.B - self.short), self._sources)
        return self._tail

    def _capture(self, plan: _Plan):
        from .step import _capturing, _warm_up
        s = plan.step
        snap = s.opt_state.snapshot() if self.training else None

        def once():
            self._reset()
            plan.gather()
            s.enqueue(False) if self.training else s.enqueue()
            plan.collect()

        _warm_up(once)
        plan.graph = torch.cuda.CUDAGraph()
        with _capturing(plan.graph):
            plan.gather()
            s.enqueue()
            plan.collect()
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

    def _eager_step(self, plan: _Plan, n: int) -> int:
        """gather | step.step(None) / step.run(None) | collect, launched one by one; returns the launches it took."""
        s = plan.step
        plan.gather()
        if self.training:
            s.step(None)
            inner = s.launches_per_step if s.use_graph else (3 if s.collective else 1)
        else:
            s.n_real = n
            s.run(None)
            inner = 2 if s.normalize and not s.use_graph else 1
        plan.collect()
        return 2 + inner

    def run_epoch(self, index: Optional[torch.Tensor] = None) -> dict:
        s, main = self.step, self._main
        self._set_order(index)
        if not self.training and s._follow_params():
            main.graph = None                # the parameter blocks moved: the step re-planned, its calls have new arguments
        whole = self.steps - int(self.short > 0)               # replays of the full batch's plan
        tail = self.count - (self.steps - 1) * self.B          # jets of the last batch
        # the means of an evaluation step (jet-feature MSE, mse / hungarian) run over the real jets: its short batch is a call of its
        # own descriptors, outside any graph (the EMD loss stage is a sum over the jets, like Chamfer: no such call)
        eager_tail = not self.training and tail < self.B and (s.chamfer_jet_features or
                                                              s.loss_kind in (s.N.LOSS_MSE, s.N.LOSS_HUNGARIAN))
        # (captures run a warm-up step on the epoch's state: all of them come before the reset)
        if self.single_graph and main.graph is None and whole > 0:
            self._capture(main)
        if self.short and self.single_graph and self._short_plan().graph is None:
            self._capture(self._tail)
        self._reset()
        controlled = self.training and s.opt_state.ctl_form
        if controlled:                       # a guarded step: the epoch's counters start over with the epoch (the device lr stays)
            s.opt_state.reset()
        launches = 0
        for it in range(whole):
            n = tail if it == self.steps - 1 else self.B
            if self.single_graph and not (eager_tail and n < self.B):
                main.graph.replay()
                launches += 1
            else:
                launches += self._eager_step(main, n)
        if self.short:                       # the short last batch: one replay of the second graph, behind the first's
            if self.single_graph:
                self._tail.graph.replay()
                launches += 1
            else:
                launches += self._eager_step(self._short_plan(), self.short)
        if not self.training:
            s.n_real = tail
        torch.cuda.current_stream().synchronize()          # the epoch's one synchronisation
        loss_sum, steps = self._epoch.tolist()
        status = int(self._status.item())
        if int(steps) != self.steps or int(self._cursor[0].item()) != self.steps:
            raise RuntimeError(f"the epoch counted {steps} steps on the device, {self.steps} were launched")
        self.launches_per_epoch = launches
        out = {"loss_sum": loss_sum, "steps": int(steps), "avg_loss": loss_sum / steps, "status": status,
               "collected": dict(self.collected)}
        if controlled:
            out["control"] = s.opt_state.stats()
        return out
