"""Host-side tests of the device-resident epochs (no GPU): the C ABI of csrc/stage.hip's epoch kernels (symbols, version, every
argument refusal before any launch) and the refusals of lgn.epoch's DeviceDataset / EpochRunner."""
import ctypes as C

import pytest
import torch

from lgn import _native as N

P = 16          # placeholder device pointer (16-byte aligned): every call below must be refused before anything touches it
OUT = (P, P, P, P, P)          # p4_in, target, mask, in_scalars, factor
EP = (P, P, P)                 # index, cursor, status


def test_epoch_symbols_are_exported():
    lib = N.lib()
    for name in ("lgn_stage_gather_f64", "lgn_epoch_collect_f64", "lgn_epoch_reset"):
        assert name in N.EXPORTED_SYMBOLS
        assert hasattr(lib, name)
    assert lib.lgn_abi_version() == 19 and N.ABI_VERSION == 19
    assert (N.EPOCH_MAX_COLLECT, N.EPOCH_BAD_INDEX) == (4, 1)


@pytest.mark.parametrize("src,sizes,ep,dims,method,opts,out,what", [
    ((P, None, None), (10, 10), EP, (4, 6), 4, (1.0, 0, 0), OUT, "unknown method code 4"),
    ((P, None, None), (10, 10), EP, (4, 6), -1, (1.0, 0, 0), OUT, "unknown method code -1"),
    ((P, None, None), (0, 10), EP, (4, 6), 2, (1.0, 0, 0), OUT, "M = 0"),
    ((P, None, None), (10, 0), EP, (4, 6), 2, (1.0, 0, 0), OUT, "count = 0"),
    ((P, None, None), (10, 10), EP, (0, 6), 2, (1.0, 0, 0), OUT, "B_pad = 0"),
    ((P, None, None), (10, 10), EP, (4, 0), 2, (1.0, 0, 0), OUT, "N = 0"),
    ((P, None, None), (10, 10), EP, (4, 6), 2, (1.0, 0, -1), OUT, "K = -1"),
    ((None, None, None), (10, 10), EP, (4, 6), 2, (1.0, 0, 0), OUT, "null p4"),
    ((P, None, None), (10, 10), (None, P, P), (4, 6), 2, (1.0, 0, 0), OUT, "null epoch pointer"),
    ((P, None, None), (10, 10), (P, None, P), (4, 6), 2, (1.0, 0, 0), OUT, "null epoch pointer"),
    ((P, None, None), (10, 10), (P, P, None), (4, 6), 2, (1.0, 0, 0), OUT, "null epoch pointer"),
    ((P, None, None), (10, 10), EP, (4, 6), 2, (1.0, 0, 0), (None, P, P, P, P), "null output"),
    ((P, None, None), (10, 10), EP, (4, 6), 2, (1.0, 0, 0), (P, None, P, P, P), "null output"),
    ((P, None, None), (10, 10), EP, (4, 6), 2, (1.0, 0, 0), (P, P, None, P, P), "null output"),
    ((P, None, None), (10, 10), EP, (4, 6), 2, (1.0, 0, 0), (P, P, P, P, None), "null output"),
    ((P, None, None), (10, 10), EP, (4, 6), 2, (1.0, 1, 0), (P, 32, P, None, P), "in_scalars missing"),
    ((P, None, P), (10, 10), EP, (4, 6), 2, (1.0, 0, 2), (P, 32, P, None, P), "in_scalars missing"),
    ((P, None, None), (10, 10), EP, (4, 6), 2, (1.0, 0, 2), (P, 32, P, P, P), "null scalars"),
    ((P, None, None), (10, 10), EP, (4, 6), 2, (0.5, 0, 0), OUT, "target may be p4_in only"),
    ((P, None, None), (10, 10), EP, (4, 6), 2, (1.0, 1, 0), OUT, "target may be p4_in only"),
    ((8, None, None), (10, 10), EP, (4, 6), 2, (1.0, 0, 0), OUT, "16-byte aligned"),
    ((P, None, None), (10, 10), EP, (4, 6), 2, (1.0, 0, 0), (8, 32, P, P, P), "16-byte aligned"),
    ((P, None, None), (10, 10), EP, (4, 6), 2, (1.0, 0, 0), (P, 24, P, P, P), "16-byte aligned"),
    ((P, None, None), (10, 10), EP, (4, 6), 2, (1.0, 0, 0), (P, 32, P, P, 8), "16-byte aligned"),
    ((P, None, None), (10, 10), (P, 4, P), (4, 6), 2, (1.0, 0, 0), OUT, "misaligned index, cursor or status"),
])
def test_stage_gather_refusals(src, sizes, ep, dims, method, opts, out, what):
    p4, labels, scalars = src
    (M, count), (index, cursor, status), (B_pad, n), (scale, jet, K) = sizes, ep, dims, opts
    p4_in, target, mask, in_scalars, factor = out
    assert N.lib().lgn_stage_gather_f64(p4, labels, scalars, M, index, count, cursor, B_pad, n, method, scale, jet, K, p4_in, target,
                                        mask, in_scalars, factor, status, None) < 0
    assert what in N.last_error()


def _arrays(src, dst, rd):
    n = max(len(src), 1)
    return (C.c_void_p * n)(*src), (C.c_void_p * n)(*dst), (C.c_int * n)(*rd)


@pytest.mark.parametrize("head,count,B,src,dst,rd,what", [
    ((P, P, P), 0, 4, [P], [P], [24], "count = 0"),
    ((P, P, P), 10, 0, [P], [P], [24], "B = 0"),
    ((P, P, P), 10, 4, [P] * 5, [P] * 5, [24] * 5, "5 tensors to collect"),
    ((None, P, P), 10, 4, [P], [P], [24], "null pointer"),
    ((P, None, P), 10, 4, [P], [P], [24], "null pointer"),
    ((P, P, None), 10, 4, [P], [P], [24], "null pointer"),
    ((P, 4, P), 10, 4, [P], [P], [24], "8-byte aligned"),
    ((P, P, P), 10, 4, [P], [P], [0], "row_doubles = 0"),
    ((P, P, P), 10, 4, [P, P], [P, P], [24, -3], "row_doubles = -3 of tensor 1"),
    ((P, P, P), 10, 4, [P, None], [P, P], [24, 4], "null src or dst of tensor 1"),
    ((P, P, P), 10, 4, [P, P], [None, P], [24, 4], "null src or dst of tensor 0"),
    ((P, P, P), 10, 4, [P], [4], [24], "must be 8-byte aligned"),
])
def test_epoch_collect_refusals(head, count, B, src, dst, rd, what):
    loss, epoch, cursor = head
    s, d, r = _arrays(src, dst, rd)
    assert N.lib().lgn_epoch_collect_f64(loss, epoch, cursor, count, B, len(src), s, d, r, None) < 0
    assert what in N.last_error()


def test_epoch_collect_refuses_missing_arrays_and_a_negative_count():
    lib = N.lib()
    assert lib.lgn_epoch_collect_f64(P, P, P, 10, 4, 1, None, None, None, None) < 0
    assert "null src / dst / row_doubles" in N.last_error()
    assert lib.lgn_epoch_collect_f64(P, P, P, 10, 4, -1, None, None, None, None) < 0
    assert "-1 tensors to collect" in N.last_error()


@pytest.mark.parametrize("ptrs,what", [((None, P, P), "null pointer"), ((P, None, P), "null pointer"), ((P, P, None), "null pointer"),
                                       ((4, P, P), "misaligned"), ((P, P, 2), "misaligned")])
def test_epoch_reset_refusals(ptrs, what):
    assert N.lib().lgn_epoch_reset(*ptrs, None) < 0
    assert what in N.last_error()


def test_device_dataset_refuses_cpu_tensors_and_bad_shapes():
    from lgn.epoch import DeviceDataset
    p4 = torch.zeros(10, 6, 4, dtype=torch.float64)
    with pytest.raises(ValueError, match="holds GPU tensors"):
        DeviceDataset({"p4": p4})
    with pytest.raises(ValueError, match="not a tensor"):
        DeviceDataset({"p4": p4.numpy()})
    with pytest.raises(ValueError, match="no 'p4'"):
        DeviceDataset({"labels": torch.zeros(10, 6)})


def test_epoch_runner_refuses_an_unsupported_step_class_and_dataset():
    from lgn.epoch import EpochRunner
    from lgn.step import ModuleEvalStep

    class Loop:
        pass

    with pytest.raises(TypeError, match="NativeTrainStep or a NativeEvalStep.*Loop"):
        EpochRunner(Loop(), None)
    with pytest.raises(TypeError, match="ModuleEvalStep"):
        EpochRunner(ModuleEvalStep.__new__(ModuleEvalStep), None)


def test_index_outside_the_dataset_is_refused_on_the_host():
    from lgn.epoch import check_index
    ok = torch.tensor([3, 1, 2, 0, 0], dtype=torch.int32)
    assert check_index(ok, 5) is ok
    for bad, what in ((torch.tensor([0, 1, 2, 3, 5]), r"from 0 to 5, outside \[0, 5\)"),
                      (torch.tensor([0, -1, 2, 3, 4]), r"from -1 to 4, outside \[0, 5\)"),
                      (torch.tensor([0, 1, 2]), "3 entries, the dataset 5"),
                      (torch.tensor([0.0, 1.0, 2.0, 3.0, 4.0]), "1-d integer tensor"),
                      (torch.zeros(5, 1, dtype=torch.int64), "1-d integer tensor")):
        with pytest.raises(ValueError, match=what):
            check_index(bad, 5)


def test_remainder_rules():
    from lgn.epoch import epoch_steps
    assert epoch_steps(10, 4, None, training=True) == (2, 8)          # a training step drops the short batch
    assert epoch_steps(10, 4, None, training=False) == (3, 10)        # an evaluation step pads it
    assert epoch_steps(10, 4, "drop", training=False) == (2, 8)
    assert epoch_steps(12, 4, "error", training=True) == (3, 12)
    for training in (True, False):
        with pytest.raises(ValueError, match="2 left over"):
            epoch_steps(10, 4, "error", training=training)
    with pytest.raises(ValueError, match="whole batches only"):
        epoch_steps(10, 4, "pad", training=True)
    with pytest.raises(ValueError, match="do not fill one batch"):
        epoch_steps(3, 4, "drop", training=True)
    with pytest.raises(ValueError, match="remainder is one of"):
        epoch_steps(10, 4, "keep", training=True)
