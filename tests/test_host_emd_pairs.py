"""Host tests of the EMD matrices and options (csrc/emd_pairs.hip): the restatement tests/_emd_pairs_ref.py against an independent solver
and closed forms, the pair decode of the kernel (exported as a host call) against a Python enumeration up to pair numbers no GPU test
reaches, the ABI, and every refusal before any launch.  No GPU."""
import ctypes
import itertools
import os
import re

import numpy as np
import pytest

import _emd_pairs_ref as P
import _util as U

SYMBOLS = ("lgn_emd_pairs_f64", "lgn_emd_pairs_decode")
FULL, UPPER, ALIGNED = 0, 1, 2


# ---- 1. the restatement --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [1, 2, 7, 30, 64])
def test_the_restatement_is_the_assignment_optimum_on_equal_normalised_weights(n):
    """Equal weights with norm=True: every particle carries 1 / n, the optimal flow is a permutation (Birkhoff), the EMD is the
    assignment optimum on the option cost matrix divided by n.  1e-13: the bound tests/test_host_emd.py uses for the same identity."""
    from scipy.optimize import linear_sum_assignment
    rng = np.random.default_rng(1000 + n)
    for beta, periodic in itertools.product((1.0, 2.0, 0.5), (False, True)):
        a = np.stack([np.full(n, 3.0), rng.normal(size=n), rng.uniform(0, 2 * np.pi, n)], -1)
        b = np.stack([np.full(n, 0.7), rng.normal(size=n), rng.uniform(0, 2 * np.pi, n)], -1)
        opts = dict(R=0.8, beta=beta, periodic_phi=periodic)
        c = P.thetas(a, b, **opts)
        r, k = linear_sum_assignment(c)
        want = c[r, k].sum() / n
        got = P.emd(a, b, norm=True, **opts)
        assert abs(got - want) <= 1e-13 * want, (beta, periodic, got, want)


def test_the_restatement_meets_the_closed_forms():
    # one particle on each side under every option
    p, q = np.array([[2.0, 0.1, 0.3]]), np.array([[0.5, 0.4, 6.1]])
    for R, beta, norm, periodic in itertools.product((1.0, 0.8), (1.0, 2.0, 0.5), (False, True), (False, True)):
        dphi = 0.3 - 6.1
        if periodic:
            dphi = np.pi - abs(np.pi - abs(dphi))
        theta = np.sqrt(0.3 ** 2 + dphi ** 2) / R
        want = theta ** beta if norm else 0.5 * theta ** beta + 1.5
        got = P.emd(p, q, R=R, beta=beta, norm=norm, periodic_phi=periodic)
        assert abs(got - want) <= 1e-14 * want, (R, beta, norm, periodic, got, want)
    # periodic: phi = 0.1 against phi = 2 pi - 0.1 is 0.2 apart (1e-14: the angles and pi round at ulp(2 pi) = 9e-16, five operations)
    a, b = np.array([[1.0, 0.0, 0.1]]), np.array([[1.0, 0.0, 2 * np.pi - 0.1]])
    assert abs(P.emd(a, b, periodic_phi=True) - 0.2) <= 1e-14
    assert abs(P.emd(a, b) - (2 * np.pi - 0.2)) <= 1e-14
    # beta leaves the weight-difference term alone: 3 against 1 at distance 0.5 moves 1 and pays |3 - 1| once, not |3 - 1|^beta
    a, b = np.array([[3.0, 0.0, 0.0]]), np.array([[1.0, 0.3, 0.4]])
    for beta in (2.0, 0.5, 3.0):
        assert abs(P.emd(a, b, beta=beta) - (0.5 ** beta + 2.0)) <= 1e-14
    # at the defaults the restatement is tests/_emd_ref.py's
    import _emd_ref as E
    rng = np.random.default_rng(3)
    x = np.stack([rng.random(6) + 0.1, rng.normal(size=6), rng.normal(size=6)], -1)
    y = np.stack([rng.random(9) + 0.1, rng.normal(size=9), rng.normal(size=9)], -1)
    assert P.emd(x, y) == E.emd(x, y) and P.emd(x, y, R=0.4) == E.emd(x, y, R=0.4)
    # norm: an event without weight cannot be normalised
    assert np.isnan(P.emd(np.zeros((3, 3)), y, norm=True)) and np.isfinite(P.emd(np.zeros((3, 3)), y))
    m = P.emds(np.stack([x, x[::-1]]))
    assert m.shape == (2, 2) and m[0, 0] == 0.0 and m[0, 1] == m[1, 0] <= 1e-15


# ---- 2. the pair decode ----------------------------------------------------------------------------------------------------------------

def _decode(lib, mode, p, B0, B1):
    i, j = ctypes.c_int(-1), ctypes.c_int(-1)
    assert lib.lgn_emd_pairs_decode(mode, p, B0, B1, ctypes.byref(i), ctypes.byref(j)) == 0, (mode, p, B0, B1)
    return i.value, j.value


def _row_start(i, B):
    return i * (2 * B - i - 1) // 2


@pytest.mark.parametrize("B", [2, 3, 5, 64, 65])
def test_the_decode_of_every_pair_number(B):
    from lgn import _native as N
    lib = N.lib()
    for p, want in enumerate(P.upper_pairs(B)):
        assert _decode(lib, UPPER, p, B, B) == want, (B, p)
    B1 = B + 3
    for p in range(B * B1):
        assert _decode(lib, FULL, p, B, B1) == (p // B1, p % B1), (B, p)
    for p in range(B):
        assert _decode(lib, ALIGNED, p, B, B) == (p, p)
    i, j = ctypes.c_int(), ctypes.c_int()
    for mode, bad in ((UPPER, B * (B - 1) // 2), (FULL, B * B), (ALIGNED, B), (UPPER, -1)):
        assert lib.lgn_emd_pairs_decode(mode, bad, B, B, ctypes.byref(i), ctypes.byref(j)) < 0 and "outside" in N.last_error()


@pytest.mark.parametrize("B", [2049, 65536, 2 ** 20])
def test_the_decode_at_row_changes_of_large_sets(B):
    """The first and last pair number and both sides of every row change near the first, middle and last rows: where a decode seeded
    by a floating square root would go wrong if the root decided it."""
    from lgn import _native as N
    lib = N.lib()
    total = B * (B - 1) // 2
    assert _decode(lib, UPPER, 0, B, B) == (0, 1) and _decode(lib, UPPER, total - 1, B, B) == (B - 2, B - 1)
    rows = sorted({r for c in (0, B // 2, B - 2) for r in range(c - 4, c + 5) if 0 <= r <= B - 2})
    for r in rows:
        first = _row_start(r, B)
        assert _decode(lib, UPPER, first, B, B) == (r, r + 1), (B, r)
        assert _decode(lib, UPPER, first + (B - 2 - r), B, B) == (r, B - 1), (B, r)          # the last pair of row r
        if r > 0:
            assert _decode(lib, UPPER, first - 1, B, B) == (r - 1, B - 1), (B, r)
    B1 = B - 1                                                                                  # FULL: rows of another length
    assert _decode(lib, FULL, 0, B, B1) == (0, 0) and _decode(lib, FULL, B * B1 - 1, B, B1) == (B - 1, B1 - 1)
    for r in rows:
        assert _decode(lib, FULL, r * B1, B, B1) == (r, 0) and _decode(lib, FULL, r * B1 + B1 - 1, B, B1) == (r, B1 - 1)
        if r > 0:
            assert _decode(lib, FULL, r * B1 - 1, B, B1) == (r - 1, B1 - 1)


# ---- 3. the ABI --------------------------------------------------------------------------------------------------------------------------

def test_the_entry_points_are_declared_and_the_abi_is_19():
    from lgn import _native as N
    with open(os.path.join(U.ROOT, "include", "lgn_amd.h")) as f:
        header = f.read()
    lib = N.lib()
    for s in SYMBOLS:
        assert re.search(r"\bint " + s + r"\(", header), s
        assert s in N.EXPORTED_SYMBOLS and s in N._SIGNATURES and hasattr(lib, s), s
        assert list(getattr(lib, s).argtypes) == list(N._SIGNATURES[s])
    assert len(N._SIGNATURES["lgn_emd_pairs_f64"]) == 16 and len(N._SIGNATURES["lgn_emd_pairs_decode"]) == 6
    for name, value in (("FULL", N.EMD_PAIRS_FULL), ("UPPER", N.EMD_PAIRS_UPPER), ("ALIGNED", N.EMD_PAIRS_ALIGNED)):
        assert re.search(rf"#define LGN_EMD_PAIRS_{name} {value}\b", header), name
    assert re.search(r"struct lgn_emd_opts \{\s*double R, beta;\s*int norm, periodic_phi;\s*\}", header)
    assert [f[0] for f in N.EmdOpts._fields_] == ["R", "beta", "norm", "periodic_phi"] and ctypes.sizeof(N.EmdOpts) == 24
    assert N.ABI_VERSION == 19 and re.search(r"#define LGN_AMD_ABI_VERSION 19\b", header) and lib.lgn_abi_version() == 19


# ---- 4. refusals -------------------------------------------------------------------------------------------------------------------------

def test_arguments_are_refused_before_any_launch():
    """As tests/test_host_emd.py, calls that cannot reach a launch whatever the check under test does: the output pointers are null
    in every call up to the null check; the checks after it (UPPER's shape, ALIGNED's, the options, flow outside ALIGNED) are given
    host addresses with n = 150 and no workspace, which the last check refuses.  Only the workspace checks themselves stand alone.
    Refusals with real device buffers: tests/test_gpu_emd_pairs.py."""
    from lgn import _native as N
    lib = N.lib()
    big = N.EMD_NMAX + 1

    def call(ev0=None, ev1=None, B0=2, B1=2, n=5, m=5, mode=FULL, opts=None, emd=None, flow=None, d0=None, d1=None, status=None,
             work=None, work_bytes=0):
        return lib.lgn_emd_pairs_f64(ev0, ev1, B0, B1, n, m, mode, opts, emd, flow, d0, d1, status, work, work_bytes, None)

    assert call(mode=3) < 0 and "unknown mode" in N.last_error()
    assert call(mode=-1) < 0 and "unknown mode" in N.last_error()
    assert call(B0=0) < 0 and "B0 = 0" in N.last_error()
    assert call(B1=0) < 0 and "B1 = 0" in N.last_error()
    for kw in (dict(n=big), dict(m=big), dict(n=0), dict(m=0)):
        assert call(**kw) < 0 and "outside" in N.last_error(), kw
    assert call() < 0 and "null pointer" in N.last_error()
    # past the null check: a host buffer stands in for the device pointers; every call below is refused before it would be used
    host = (ctypes.c_double * 8)()
    h = ctypes.cast(host, ctypes.c_void_p)
    ok = dict(ev0=h, ev1=h, emd=h, status=h, n=150, m=150)
    assert call(ev0=h, emd=h, status=None) < 0 and "null pointer" in N.last_error()
    assert call(ev0=h, emd=None, status=h) < 0 and "null pointer" in N.last_error()
    assert call(ev0=None, emd=h, status=h) < 0 and "null pointer" in N.last_error()
    assert call(**dict(ok, ev1=None), mode=FULL) < 0 and "ev1" in N.last_error()
    assert call(**dict(ok, ev1=None), mode=ALIGNED) < 0 and "ev1" in N.last_error()
    assert call(**dict(ok, m=151), mode=UPPER) < 0 and "UPPER" in N.last_error()
    assert call(**ok, mode=UPPER, B0=2, B1=3) < 0 and "UPPER" in N.last_error()
    other_buf = (ctypes.c_double * 8)()
    assert call(**dict(ok, ev1=ctypes.cast(other_buf, ctypes.c_void_p)), mode=UPPER) < 0 and "NULL or ev0" in N.last_error()
    assert call(**ok, mode=ALIGNED, B0=2, B1=3) < 0 and "ALIGNED" in N.last_error()
    for R in (0.0, -1.0, float("inf"), float("nan")):
        assert call(**ok, opts=ctypes.byref(N.EmdOpts(R, 1.0, 0, 0))) < 0 and "R = " in N.last_error(), R
    for beta in (0.0, -2.0, float("inf"), float("nan")):
        assert call(**ok, opts=ctypes.byref(N.EmdOpts(1.0, beta, 0, 0))) < 0 and "beta = " in N.last_error(), beta
    for kw in (dict(flow=h), dict(d0=h), dict(d1=h)):
        for mode in (FULL, UPPER):
            assert call(**ok, mode=mode, **kw) < 0 and "ALIGNED mode only" in N.last_error(), (mode, kw)
    # n = 150 keeps the flow in a workspace: missing, short, misaligned
    need = lib.lgn_emd_workspace_bytes(4, 150)
    assert need == 4 * 151 * 151 * 8
    assert call(**ok) < 0 and "null work" in N.last_error()
    assert call(**dict(ok, ev1=None), mode=UPPER) < 0 and "null work" in N.last_error()            # ev1 NULL is UPPER's other form
    assert call(**ok, work=h, work_bytes=need - 8) < 0 and "too short" in N.last_error()
    assert call(**dict(ok, m=20), work=ctypes.c_void_p(h.value + 4), work_bytes=need) < 0 and "aligned" in N.last_error()
    # the workspace saturates at the resident waves of the workspace path: P = 2^40 pairs need what 2^31 - 1 need
    assert lib.lgn_emd_workspace_bytes(2 ** 31 - 1, 150) == lib.lgn_emd_workspace_bytes(2048, 150) == 2048 * 151 * 151 * 8


def test_python_refuses_what_the_library_would_and_has_no_cpu_path():
    import torch
    from lgn import emd as M
    x = torch.rand(3, 5, 3, dtype=torch.float64)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        M.emds(x)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        M.emds(x, x[:2])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        M.emd(x, x, beta=2.0)
    with pytest.raises(ValueError, match="beta"):
        M.emds(x, beta=0.0)
    with pytest.raises(ValueError, match="finite R"):
        M.emds(x, R=float("inf"))
    with pytest.raises(ValueError, match=r"\(B0, n, 3\)"):
        M.emds(x[0])
    with pytest.raises(ValueError, match="191"):
        M.emds(torch.rand(2, 192, 3, dtype=torch.float64))
    assert M.status_message(M.EMPTY) == "both events are weightless" and "normalised" in M.status_message(M.EMPTY, norm=True)
