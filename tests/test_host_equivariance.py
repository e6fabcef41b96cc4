"""Host-side tests of the native equivariance test (no GPU): the C ABI of csrc/equivariance.hip (symbols, header, version, constants,
refusals before any launch), the argument errors of lgn.equivariance and its chunk arithmetic."""
import ctypes as C
import os

import pytest
import torch

from lgn import _native as N

P = 16          # placeholder device pointer: every call below must be refused before anything touches it
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "lgn_amd.h")
NEW = ("lgn_transform_jets_f64", "lgn_rep_deviation_workspace_bytes", "lgn_rep_deviation_f64")


def test_symbols_header_abi_and_constants():
    from lgn import equivariance as E
    lib = N.lib()
    with open(HEADER) as f:
        header = f.read()
    for name in NEW:
        assert name in N.EXPORTED_SYMBOLS and hasattr(lib, name) and f" {name}(" in header, name
        assert list(getattr(lib, name).argtypes) == list(N._SIGNATURES.get(name) or N._LL_SIGNATURES[name])
    assert lib.lgn_rep_deviation_workspace_bytes.restype is C.c_longlong and lib.lgn_rep_deviation_f64.restype is C.c_int
    assert lib.lgn_abi_version() == N.ABI_VERSION == 19 and "#define LGN_AMD_ABI_VERSION 19 " in header
    assert f"#define LGN_EQUI_TILE {N.EQUI_TILE}\n" in header and f"#define LGN_EQUI_MAX_PARTS {N.EQUI_MAX_PARTS}\n" in header
    assert (E.EQUI_TILE, E.EQUI_MAX_PARTS) == (N.EQUI_TILE, N.EQUI_MAX_PARTS) and N.EQUI_MAX_PARTS >= 57     # 11 GVecs x 5 + output


def test_native_harness_is_reexported():
    from lgn.models import autotest
    assert callable(autotest.lgn_tests_native) and autotest.lgn_tests_native is not autotest.lgn_tests


def ints(*xs):
    return (C.c_int * len(xs))(*xs)


def ptrs(n, value=P):
    return (C.c_void_p * n)(*([value] * n))


def deviation_call(parts=2, T=3, B=2, a=None, b=None, D=None, n=(5, 5), c=(2, 3), d=(1, 4), perm=None, stats=P, work=P, nbytes=1 << 40):
    k = max(parts, 1)
    a, b, D = (ptrs(k) if x is None else x for x in (a, b, D))
    pad = lambda xs: ints(*(tuple(xs) + (xs[-1],) * k)[:max(k, len(xs))])
    return N.lib().lgn_rep_deviation_f64(parts, T, B, a, b, D, pad(n), pad(c), pad(d), perm, stats, work, nbytes, None)


@pytest.mark.parametrize("kw, text", [
    (dict(d=(1, 2)), "d = 2"), (dict(d=(5, 4)), "d = 5"), (dict(d=(1, 16)), "d = 16"), (dict(d=(0, 1)), "d = 0"),
    (dict(parts=N.EQUI_MAX_PARTS + 1), "parts"), (dict(parts=0), "parts"), (dict(T=0), "T ="), (dict(T=65536), "T ="), (dict(B=0), "B ="),
    (dict(n=(5, 0)), "N ="), (dict(c=(0, 3)), "C ="), (dict(stats=None), "null"), (dict(work=None), "null"),
    (dict(a=ptrs(2, None)), "null"), (dict(b=ptrs(2, None)), "null"), (dict(D=ptrs(2, None)), "null"),
    (dict(nbytes=8), "too short"), (dict(work=P + 4), "aligned"), (dict(perm=P, n=(5, 6)), "same N"),
    (dict(B=1 << 20, n=(1 << 10, 5)), "rows")])
def test_rep_deviation_refusals(kw, text):
    assert deviation_call(**kw) < 0 and text in N.last_error(), N.last_error()


def test_workspace_query():
    lib = N.lib()
    tile = N.EQUI_TILE
    # B * N * C rows in tiles of `tile`, five doubles per (tile, t)
    assert lib.lgn_rep_deviation_workspace_bytes(1, 1, 1, ints(1), ints(1), ints(1)) == 5 * 8
    assert lib.lgn_rep_deviation_workspace_bytes(1, 3, 1, ints(tile + 1), ints(1), ints(9)) == 2 * 3 * 5 * 8
    assert lib.lgn_rep_deviation_workspace_bytes(2, 26, 6, ints(30, 30), ints(4, 3), ints(1, 4)) == \
        (-(-6 * 30 * 4 // tile) + -(-6 * 30 * 3 // tile)) * 26 * 5 * 8
    assert lib.lgn_rep_deviation_workspace_bytes(1, 1, 1, ints(1), ints(1), ints(2)) < 0 and "d = 2" in N.last_error()
    assert lib.lgn_rep_deviation_workspace_bytes(N.EQUI_MAX_PARTS + 1, 1, 1, ints(1), ints(1), ints(1)) < 0 and "parts" in N.last_error()
    assert lib.lgn_rep_deviation_workspace_bytes(1, 1, 1, None, ints(1), ints(1)) < 0 and "null" in N.last_error()


def transform_call(p4=P, R=P, perm=None, scalars=None, T=3, B=2, n=5, K=0, out=P, scalars_out=None):
    return N.lib().lgn_transform_jets_f64(p4, R, perm, scalars, T, B, n, K, out, scalars_out, None)


@pytest.mark.parametrize("kw, text", [
    (dict(p4=None), "null"), (dict(R=None), "null"), (dict(out=None), "null"), (dict(K=2), "null"), (dict(K=2, scalars=P), "null"),
    (dict(T=0), "T ="), (dict(T=65536), "T ="), (dict(B=0), "B ="), (dict(n=0), "N ="), (dict(K=-1), "K ="),
    (dict(B=1 << 16, n=1 << 15), "rows")])
def test_transform_jets_refusals(kw, text):
    assert transform_call(**kw) < 0 and text in N.last_error(), N.last_error()


def test_argument_errors_of_the_python_layer():
    from lgn import equivariance as E
    with pytest.raises(ValueError, match="test_type must be one of 'boost' or 'rotation'"):
        E.covariance_test(None, None, {}, "translation")
    z = torch.zeros
    with pytest.raises(RuntimeError, match="GPU"):
        E.transform_jets(z(2, 5, 4, dtype=torch.float64), z(1, 4, 4, dtype=torch.float64))
    with pytest.raises(RuntimeError, match="GPU"):
        E.rep_deviation([z(2, 2, 5, 2, 1, dtype=torch.float64)], [z(2, 2, 5, 2, 1, dtype=torch.float64)], [z(1, 2, 1, 1, dtype=torch.float64)])
    with pytest.raises(ValueError, match="equally long"):
        E.rep_deviation([], [], [])


def test_chunk_arithmetic():
    from lgn.equivariance import angle_chunks
    assert angle_chunks(6, 26, 512) == [(0, 26)]
    chunks = angle_chunks(6, 26, 30)
    assert chunks == [(0, 5), (5, 10), (10, 15), (15, 20), (20, 25), (25, 26)]
    assert all((t1 - t0) * 6 <= 30 for t0, t1 in chunks)
    assert angle_chunks(6, 26, 6) == [(t, t + 1) for t in range(26)]
    assert angle_chunks(64, 26, 512) == [(0, 8), (8, 16), (16, 24), (24, 26)]
    with pytest.raises(ValueError, match="max_jets = 5 is smaller than the batch of 6 jets"):
        angle_chunks(6, 26, 5)
