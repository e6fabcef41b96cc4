"""Host tests of the EMD score's yardstick and ABI: the LP restatement tests/_emd_ref.py reproduces the g24 fixture, equals the exact
assignment optimum on equal-weight events and meets the closed forms; the new entry points are declared in include/lgn_amd.h and in
lgn/_native.py, the ABI is still 19, and the ctypes signatures load.  No GPU."""
import ctypes
import os
import re

import numpy as np
import pytest

import _emd_ref as E
import _util as U

GENERIC = ("5x8", "1x7", "64x65")
REL = ("n12", "n30", "n150")
SYMBOLS = ("lgn_emd_f64", "lgn_emd_relative_f64", "lgn_emd_workspace_bytes", "lgn_emd_lds_bytes")


def test_the_restatement_reproduces_the_fixture():
    z = U.load("g24_emd.npz")
    for tag in GENERIC:
        a, b = z[f"gen_{tag}_ev0"], z[f"gen_{tag}_ev1"]
        got = np.array([E.emd(a[i], b[i]) for i in range(len(a))])
        np.testing.assert_allclose(got, z[f"gen_{tag}_emd"], rtol=1e-12, atol=1e-300, err_msg=tag)
    for tag in REL:
        got = E.emd_relative(z[f"rel_{tag}_recons"], z[f"rel_{tag}_target"])
        assert got.shape == z[f"rel_{tag}_emd"].shape and len(got) <= 16
        np.testing.assert_allclose(got, z[f"rel_{tag}_emd"], rtol=1e-12, atol=1e-300, err_msg=tag)


@pytest.mark.parametrize("n", [6, 30, 150])
def test_the_restatement_is_the_assignment_optimum_on_equal_weights(n):
    from scipy.optimize import linear_sum_assignment
    rng = np.random.default_rng(n)
    a = np.concatenate([np.ones((n, 1)), rng.normal(size=(n, 2))], -1)
    b = np.concatenate([np.ones((n, 1)), rng.normal(size=(n, 2))], -1)
    c = E.thetas(a, b)
    r, k = linear_sum_assignment(c)
    want = c[r, k].sum()
    got = E.emd(a, b)
    assert abs(got - want) <= 1e-13 * want
    assert abs(E.emd(b, a) - got) <= 1e-13 * want              # symmetric in its arguments
    a[:, 0] = b[:, 0] = 1.0 / n
    assert abs(n * E.emd(a, b) - want) <= 1e-13 * want


def test_the_restatement_meets_the_closed_forms():
    rng = np.random.default_rng(5)
    a = np.stack([rng.random(9) + 0.1, rng.normal(size=9), rng.normal(size=9)], -1)
    assert E.emd(a, a) == 0.0
    assert E.emd(a, a[::-1]) <= 1e-15
    for p, q in (((2.0, 0.1, -0.3), (0.5, 0.4, 0.1)), ((0.25, 1.0, 1.0), (3.0, -1.0, 0.5)), ((1.0, 0.0, 0.0), (1.0, 3.0, 4.0))):
        p, q = np.array([p]), np.array([q])
        theta = np.sqrt((p[0, 1] - q[0, 1]) ** 2 + (p[0, 2] - q[0, 2]) ** 2)
        want = min(p[0, 0], q[0, 0]) * theta + abs(p[0, 0] - q[0, 0])
        assert abs(E.emd(p, q) - want) <= 1e-14 * want
        assert abs(E.emd(p, q, R=0.4) - (min(p[0, 0], q[0, 0]) * theta / 0.4 + abs(p[0, 0] - q[0, 0]))) <= 1e-14 * want / 0.4
    empty = np.zeros((4, 3))
    assert abs(E.emd(empty, a) - a[:, 0].sum()) <= 1e-14 * a[:, 0].sum()      # one event weightless: the other's sum pT
    assert np.isnan(E.emd(empty, empty))


def test_the_entry_points_are_declared_and_the_abi_is_19():
    from lgn import _native as N
    with open(os.path.join(U.ROOT, "include", "lgn_amd.h")) as f:
        header = f.read()
    for s in SYMBOLS:
        assert re.search(r"\b(int|long long) " + s + r"\(", header), s
        assert s in N.EXPORTED_SYMBOLS, s
    m = re.search(r"#define LGN_EMD_NMAX (\d+)", header)
    assert m and int(m.group(1)) >= 150 and int(m.group(1)) == N.EMD_NMAX
    for name, bit in (("INVALID", N.EMD_INVALID), ("EMPTY", N.EMD_EMPTY), ("ITER", N.EMD_ITER), ("INFEASIBLE", N.EMD_INFEASIBLE)):
        assert re.search(rf"#define LGN_EMD_{name} {bit}\b", header), name
    assert N.ABI_VERSION == 19 and re.search(r"#define LGN_AMD_ABI_VERSION 19\b", header)
    assert len(N._SIGNATURES["lgn_emd_f64"]) == 14 and len(N._SIGNATURES["lgn_emd_relative_f64"]) == 9
    assert N._LL_SIGNATURES["lgn_emd_workspace_bytes"] == [ctypes.c_int, ctypes.c_int]
    assert N._LL_SIGNATURES["lgn_emd_lds_bytes"] == [ctypes.c_int]


def test_the_ctypes_signatures_load():
    from lgn import _native as N
    lib = N.lib()                       # binds every signature; raises on a missing symbol
    for s in SYMBOLS:
        assert hasattr(lib, s)
    # plan-time queries are host arithmetic: the flow fits LDS at the small shapes, not at the project's largest jet
    assert lib.lgn_emd_workspace_bytes(8, 30) == 0 and lib.lgn_emd_lds_bytes(30) >= 8 * 31 * 31
    assert lib.lgn_emd_workspace_bytes(8, 150) == 8 * 151 * 151 * 8 and lib.lgn_emd_lds_bytes(150) < 8 * 151 * 151
    assert lib.lgn_emd_workspace_bytes(8, N.EMD_NMAX + 1) < 0 and lib.lgn_emd_lds_bytes(0) < 0


def test_arguments_are_refused_before_any_launch():
    """Only calls that cannot reach a launch whatever the other checks do: the output pointers are null, so even if the check under
    test regressed the null-pointer check would still refuse the call.  Refusals with real device buffers: tests/test_gpu_emd.py."""
    from lgn import _native as N
    lib = N.lib()
    big = N.EMD_NMAX + 1
    null = (None, None)                 # ev0, ev1
    assert lib.lgn_emd_f64(*null, 2, big, 5, 1.0, None, None, None, None, None, None, 0, None) < 0 and "outside" in N.last_error()
    assert lib.lgn_emd_f64(*null, 2, 5, big, 1.0, None, None, None, None, None, None, 0, None) < 0 and "outside" in N.last_error()
    assert lib.lgn_emd_f64(*null, 0, 5, 5, 1.0, None, None, None, None, None, None, 0, None) < 0 and "B = 0" in N.last_error()
    assert lib.lgn_emd_f64(*null, 2, 5, 5, 1.0, None, None, None, None, None, None, 0, None) < 0 and "null pointer" in N.last_error()
    assert lib.lgn_emd_relative_f64(*null, 2, big, None, None, None, 0, None) < 0 and "outside" in N.last_error()
    assert lib.lgn_emd_relative_f64(*null, 2, 30, None, None, None, 0, None) < 0 and "null pointer" in N.last_error()
    assert lib.lgn_emd_workspace_bytes(2, 150) == 2 * 151 * 151 * 8
