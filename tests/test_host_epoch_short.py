"""Host-side tests (no GPU) of the short last batch of a training epoch and of the latent's collection: the rules of
remainder='short', the C ABI of the two entry points csrc/stage.hip gained for them (symbols, version, every argument refusal
before any launch) and the runner's refusals that need no device."""
import ctypes as C

import pytest

from lgn import _native as N

P = 16          # placeholder device pointer (16-byte aligned): every call below must be refused before anything touches it
OUT = (P, P, P, P, P)          # p4_in, target, mask, in_scalars, factor
EP = (P, P, P)                 # index, cursor, status


def test_short_remainder_rules():
    from lgn.epoch import REMAINDERS, epoch_steps
    assert "short" in REMAINDERS
    assert epoch_steps(10, 4, "short", training=True) == (3, 10)
    assert epoch_steps(9, 4, "short", training=True) == (3, 9)
    assert epoch_steps(8, 4, "short", training=True) == (2, 8)          # nothing left over: whole batches only
    assert epoch_steps(3, 4, "short", training=True) == (1, 3)          # the epoch is ONE short step
    with pytest.raises(ValueError, match="'pad'"):
        epoch_steps(10, 4, "short", training=False)
    # what was so stays so: a training step's default drops, 'pad' is refused for it
    assert epoch_steps(10, 4, None, training=True) == (2, 8)
    with pytest.raises(ValueError, match="whole batches only"):
        epoch_steps(10, 4, "pad", training=True)


def test_a_collective_step_refuses_the_short_batch():
    """Splitting r jets over the ranks is out of scope: the runner and short_step itself say so (before they touch a device)."""
    from lgn.epoch import EpochRunner
    from lgn.step import NativeTrainStep
    step = NativeTrainStep.__new__(NativeTrainStep)
    step.collective = True
    with pytest.raises(ValueError, match="data-parallel"):
        EpochRunner(step, None, remainder="short")
    step.desc = N.NetDesc()
    step.desc.B = 4
    with pytest.raises(ValueError, match="data-parallel"):
        step.short_step(2)
    step.collective = False
    for n in (0, 4, 5, -1):
        with pytest.raises(ValueError, match="1 .. 3 jets"):
            step.short_step(n)


def test_latent_is_collectable():
    from lgn.epoch import COLLECTABLE
    assert "latent" in COLLECTABLE


def test_new_epoch_symbols_are_exported_and_the_abi_stands():
    lib = N.lib()
    for name in ("lgn_stage_gather_at_f64", "lgn_epoch_collect_planes_f64"):
        assert name in N.EXPORTED_SYMBOLS
        assert hasattr(lib, name)
    assert lib.lgn_abi_version() == 19 and N.ABI_VERSION == 19
    assert N.EPOCH_MAX_COLLECT == 4


def _gather_at(src=(P, None, None), sizes=(10, 10), base=8, ep=EP, dims=(2, 6), method=2, opts=(1.0, 0, 0), out=OUT):
    p4, labels, scalars = src
    (M, count), (index, cursor, status), (B_pad, n), (scale, jet, K) = sizes, ep, dims, opts
    p4_in, target, mask, in_scalars, factor = out
    return N.lib().lgn_stage_gather_at_f64(p4, labels, scalars, M, index, count, base, cursor, B_pad, n, method, scale, jet, K, p4_in,
                                           target, mask, in_scalars, factor, status, None)


@pytest.mark.parametrize("kw,what", [
    (dict(base=-1), "base = -1"),
    (dict(base=11), "base = 11"),
    (dict(method=4), "unknown method code 4"),
    (dict(sizes=(0, 10)), "M = 0"),
    (dict(sizes=(10, 0), base=0), "count = 0"),
    (dict(dims=(0, 6)), "B_pad = 0"),
    (dict(dims=(2, 0)), "N = 0"),
    (dict(opts=(1.0, 0, -1)), "K = -1"),
    (dict(src=(None, None, None)), "null p4"),
    (dict(ep=(None, P, P)), "null epoch pointer"),
    (dict(ep=(P, None, P)), "null epoch pointer"),
    (dict(ep=(P, P, None)), "null epoch pointer"),
    (dict(out=(None, P, P, P, P)), "null output"),
    (dict(out=(P, None, P, P, P)), "null output"),
    (dict(out=(P, P, None, P, P)), "null output"),
    (dict(out=(P, P, P, P, None)), "null output"),
    (dict(opts=(1.0, 1, 0), out=(P, 32, P, None, P)), "in_scalars missing"),
    (dict(opts=(1.0, 0, 2), out=(P, 32, P, P, P)), "null scalars"),
    (dict(opts=(0.5, 0, 0)), "target may be p4_in only"),
    (dict(src=(8, None, None)), "16-byte aligned"),
    (dict(out=(P, 32, P, P, 8)), "16-byte aligned"),
    (dict(ep=(P, 4, P)), "misaligned index, cursor or status"),
])
def test_stage_gather_at_refusals(kw, what):
    assert _gather_at(**kw) < 0
    assert what in N.last_error()


def _collect_planes(head=(P, P, P), count=10, base=0, B=4, src=(P,), dst=(P,), rd=(24,), planes=(1,)):
    n = max(len(src), 1)
    loss, epoch, cursor = head
    return N.lib().lgn_epoch_collect_planes_f64(loss, epoch, cursor, count, base, B, len(src), (C.c_void_p * n)(*src),
                                                (C.c_void_p * n)(*dst), (C.c_int * n)(*rd), (C.c_int * n)(*planes), None)


@pytest.mark.parametrize("kw,what", [
    (dict(planes=(0,)), "planes = 0 of tensor 0"),
    (dict(src=(P, P), dst=(P, P), rd=(24, 4), planes=(2, -1)), "planes = -1 of tensor 1"),
    (dict(base=-1), "base = -1"),
    (dict(base=11), "base = 11"),
    (dict(src=(P,) * 5, dst=(P,) * 5, rd=(24,) * 5, planes=(1,) * 5), "5 tensors to collect"),
    (dict(count=0), "count = 0"),
    (dict(B=0), "B = 0"),
    (dict(head=(None, P, P)), "null pointer"),
    (dict(head=(P, None, P)), "null pointer"),
    (dict(head=(P, P, None)), "null pointer"),
    (dict(head=(P, 4, P)), "8-byte aligned"),
    (dict(rd=(0,)), "row_doubles = 0"),
    (dict(src=(P, None), dst=(P, P), rd=(24, 4), planes=(1, 1)), "null src or dst of tensor 1"),
    (dict(src=(P, P), dst=(None, P), rd=(24, 4), planes=(1, 1)), "null src or dst of tensor 0"),
    (dict(dst=(4,)), "must be 8-byte aligned"),
])
def test_epoch_collect_planes_refusals(kw, what):
    assert _collect_planes(**kw) < 0
    assert what in N.last_error()


def test_epoch_collect_planes_refuses_missing_arrays():
    lib = N.lib()
    assert lib.lgn_epoch_collect_planes_f64(P, P, P, 10, 0, 4, 1, None, None, None, None, None) < 0
    assert "null src / dst / row_doubles" in N.last_error()
    one = (C.c_void_p * 1)(P)
    assert lib.lgn_epoch_collect_planes_f64(P, P, P, 10, 0, 4, 1, one, one, (C.c_int * 1)(24), None, None) < 0
    assert "null planes array" in N.last_error()
    assert lib.lgn_epoch_collect_planes_f64(P, P, P, 10, 0, 4, -1, None, None, None, None, None) < 0
    assert "-1 tensors to collect" in N.last_error()
