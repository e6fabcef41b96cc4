"""Host tests of the EMD loss stage of the whole-step calls (csrc/emd_loss.hip, LGN_LOSS_EMD): the kind and lgn_emd_loss_desc are
declared with the layout the header documents, the ctypes struct has it, the ABI is still 19, lgn_emd_loss_lds_bytes is exported and
counts what the header says, and lgn.step._loss_desc builds the descriptor from an EMDLoss / HybridLoss only when asked to
(native_emd=True).  No GPU."""
import ctypes
import os
import re
import types

import pytest
import torch

import _util as U


def _header():
    with open(os.path.join(U.ROOT, "include", "lgn_amd.h")) as f:
        return f.read()


def _decoder(n=30, c=4):
    """what _loss_desc reads of a decoder"""
    return types.SimpleNamespace(num_output_particles=n, num_channels=[c, c, c])


def test_the_kind_and_the_struct_are_declared_and_the_abi_is_19():
    from lgn import _native as N
    header = _header()
    assert re.search(r"#define LGN_LOSS_EMD 3\b", header) and N.LOSS_EMD == 3
    m = re.search(r"typedef struct lgn_emd_loss_desc \{(.*?)\} lgn_emd_loss_desc;", header, re.S)
    assert m, "lgn_emd_loss_desc is not declared"
    members = re.findall(r"^\s*(\w+)\s+(\w+);", m.group(1), re.M)
    assert members == [("lgn_loss_desc", "base"), ("lgn_emd_opts", "opts"), ("double", "chamfer_weight")]
    assert header.index("} lgn_emd_opts;") < m.start(), "the struct uses lgn_emd_opts before its definition"
    assert re.search(r"\blong long lgn_emd_loss_lds_bytes\(int N, int C\);", header)
    assert N.ABI_VERSION == 19 and re.search(r"#define LGN_AMD_ABI_VERSION 19\b", header) and N.lib().lgn_abi_version() == 19
    assert "the EMD inside the whole-step calls" not in header        # (what the header used to list as not offered)


def test_the_ctypes_struct_has_the_documented_layout():
    from lgn import _native as N
    header = _header()
    doc = re.search(r"sizeof\(lgn_emd_loss_desc\) = (\d+); offsets base (\d+) \(kind (\d+), abs_coord (\d+), polar_coord (\d+), "
                    r"scale (\d+)\), opts (\d+) \(R (\d+), beta (\d+),\s*\*?\s*norm (\d+), periodic_phi (\d+)\), chamfer_weight (\d+)",
                    header)
    assert doc, "the header does not document the layout"
    size, base, kind, a, p, scale, opts, R, beta, norm, per, cw = (int(x) for x in doc.groups())
    D, L, O = N.EMDLossDesc, N.LossDesc, N.EmdOpts
    assert ctypes.sizeof(D) == size == 56
    assert (D.base.offset, D.opts.offset, D.chamfer_weight.offset) == (base, opts, cw) == (0, 24, 48)
    assert (L.kind.offset, L.abs_coord.offset, L.polar_coord.offset, L.scale.offset) == (kind, a, p, scale)
    assert (opts + O.R.offset, opts + O.beta.offset, opts + O.norm.offset, opts + O.periodic_phi.offset) == (R, beta, norm, per)
    # the prefix idiom: a pointer to the first member is a pointer to the struct
    d = D()
    assert ctypes.addressof(d.base) == ctypes.addressof(d)
    assert N.loss_ref(None) is None


def test_the_lds_count_is_the_documented_sum():
    from lgn import _native as N
    lib = N.lib()
    assert "lgn_emd_loss_lds_bytes" in N.EXPORTED_SYMBOLS and "lgn_emd_loss_lds_bytes" in N._LL_SIGNATURES
    for bad in ((0, 4), (-3, 4), (30, 0), (30, -1)):
        assert lib.lgn_emd_loss_lds_bytes(*bad) == -1, bad
        assert "emd_loss_lds_bytes" in N.last_error()
    for C in (1, 2, 4, 8):
        last = 0
        for n in list(range(1, 70)) + [127, 128, 150, 191]:
            got = lib.lgn_emd_loss_lds_bytes(n, C)
            emd_doubles = 5 * (n + 1) + 8 + (n + 1) * (n + 1)           # emd_lds_doubles(n, n, true) of csrc/emd_plan.hpp
            stage = 8 * (20 * n + 10 * n * C + 2 * C)
            assert got == stage + 8 * emd_doubles + 8 * (n + 1), (n, C)
            # the output stage's block is the assignment stage's without that loss's own block (18 N + 4 doubles and N ints, padded)
            assert stage == lib.lgn_assign_loss_lds_bytes(n, C) - 8 * (18 * n + 4 + (n + 1) // 2), (n, C)
            # one wavefront's share is what the EMD calls themselves count where their flow is in LDS
            if 8 * emd_doubles + 8 * (n + 1) <= 64 * 1024:
                assert got - stage == lib.lgn_emd_lds_bytes(n), n
            assert got > last, (n, C)
            last = got
    assert lib.lgn_emd_loss_lds_bytes(150, 4) > N.LDS_LIMIT >= lib.lgn_emd_loss_lds_bytes(64, 4)


def test_loss_desc_of_an_emd_loss():
    from lgn import _native as N
    from lgn.losses import EMDLoss
    from lgn.step import _loss_desc
    module = EMDLoss(beta=2.0)
    kind, d = _loss_desc(module, True, False, False, 4, _decoder(), native_emd=True)
    assert kind == N.LOSS_EMD and isinstance(d, N.EMDLossDesc)
    assert (d.base.kind, d.base.abs_coord, d.base.polar_coord, d.base.scale) == (N.LOSS_EMD, 0, 0, 1.0)
    assert (d.opts.R, d.opts.beta, d.opts.norm, d.opts.periodic_phi) == (1.0, 2.0, 0, 0)
    assert d.chamfer_weight == 0.0
    # the scale does not depend on the batch: the loss is a sum over the jets
    assert _loss_desc(module, True, False, False, 4096, _decoder(), native_emd=True)[1].base.scale == 1.0
    kind, d = _loss_desc(EMDLoss(R=0.8, beta=2.0, norm=True, periodic_phi=True), True, False, False, 4, _decoder(), native_emd=True)
    assert (d.opts.R, d.opts.beta, d.opts.norm, d.opts.periodic_phi) == (0.8, 2.0, 1, 1)


def test_loss_desc_of_a_hybrid_loss():
    from lgn import _native as N
    from lgn.losses import HybridLoss
    from lgn.step import _loss_desc
    kind, d = _loss_desc(HybridLoss(0.5, norm=True), True, False, False, 4, _decoder(), native_emd=True)
    assert kind == N.LOSS_EMD and d.base.kind == N.LOSS_EMD
    assert d.chamfer_weight == 0.5 and d.opts.norm == 1 and d.opts.beta == 1.0 and d.base.scale == 1.0
    with pytest.raises(NotImplementedError, match="chamfer_jet_features"):
        _loss_desc(HybridLoss(0.5), True, False, True, 4, _decoder(), native_emd=True)


def test_what_is_refused():
    from lgn.losses import ChamferLoss, EMDLoss, HybridLoss
    from lgn.step import _loss_desc
    # the default keeps refusing every module (what the earlier tests pin), the keyword is the last one
    for module in (EMDLoss(), HybridLoss(0.5)):
        with pytest.raises(NotImplementedError, match="module API"):
            _loss_desc(module, True, False, False, 4, _decoder())
        with pytest.raises(NotImplementedError, match="module API"):
            _loss_desc(module, True, False, False, 4, _decoder(), False)
    # any other module still raises
    for module in (ChamferLoss(device=torch.device("cpu")), torch.nn.MSELoss()):
        with pytest.raises(NotImplementedError, match="module API"):
            _loss_desc(module, True, False, False, 4, _decoder(), native_emd=True)
    # a decoder whose stage does not fit names the count and the limit
    with pytest.raises(NotImplementedError, match=r"lgn_emd_loss_lds_bytes.*163840"):
        _loss_desc(EMDLoss(), True, False, False, 4, _decoder(150, 4), native_emd=True)
    # names stay names
    from lgn.losses import loss_kind
    for name in ("emd", "hybrid"):
        with pytest.raises(NotImplementedError):
            loss_kind(name)
