"""Host tests of the matrix gradients of the EMD (csrc/emd_pairs_grad.hip): the ABI, every refusal before any launch, the Python
refusals, and the numpy restatement of the fixed-order weighted sum (tests/_emd_pairs_grad_ref.py) against np.einsum.  No GPU."""
import ctypes
import os
import re

import numpy as np
import pytest

import _emd_pairs_grad_ref as R
import _util as U

SYMBOLS = ("lgn_emd_pairs_grad_f64", "lgn_emd_pairs_grad_reduce_f64")
FULL, UPPER, ALIGNED = 0, 1, 2


# ---- 1. the ABI --------------------------------------------------------------------------------------------------------------------------

def test_the_entry_points_are_declared_and_the_abi_is_19():
    from lgn import _native as N
    with open(os.path.join(U.ROOT, "include", "lgn_amd.h")) as f:
        header = f.read()
    lib = N.lib()
    for s in SYMBOLS:
        assert re.search(r"\bint " + s + r"\(", header), s
        assert s in N.EXPORTED_SYMBOLS and s in N._SIGNATURES and hasattr(lib, s), s
        assert list(getattr(lib, s).argtypes) == list(N._SIGNATURES[s])
    q = "lgn_emd_pairs_grad_slab_bytes"
    assert re.search(r"\blong long " + q + r"\(", header) and q in N.EXPORTED_SYMBOLS and q in N._LL_SIGNATURES
    assert lib.lgn_emd_pairs_grad_slab_bytes.restype is ctypes.c_longlong
    assert len(N._SIGNATURES["lgn_emd_pairs_grad_f64"]) == 17 and len(N._SIGNATURES["lgn_emd_pairs_grad_reduce_f64"]) == 13
    assert N._LL_SIGNATURES[q] == [ctypes.c_int] * 7
    assert N.ABI_VERSION == 19 and re.search(r"#define LGN_AMD_ABI_VERSION 19\b", header) and lib.lgn_abi_version() == 19
    assert "gradients of the FULL and UPPER matrices in one launch (the" not in header     # (what the header used to list as not offered)


def test_the_slab_query_counts_the_pairs_of_a_row_range():
    from lgn import _native as N
    q = N.lib().lgn_emd_pairs_grad_slab_bytes
    assert q(FULL, 5, 7, 3, 4, 0, 5) == 5 * 7 * 7 * 24 and q(FULL, 5, 7, 3, 4, 2, 1) == 7 * 7 * 24
    B = 6
    assert q(UPPER, B, B, 4, 4, 0, B) == B * (B - 1) // 2 * 8 * 24
    for r0 in range(B):
        for k in range(1, B - r0 + 1):
            assert q(UPPER, B, B, 4, 4, r0, k) == sum(B - 1 - i for i in range(r0, r0 + k)) * 8 * 24, (r0, k)
    assert q(UPPER, 1, 1, 4, 4, 0, 1) == 0 and q(UPPER, B, B, 4, 4, B - 1, 1) == 0
    # 2^20 events of 191 particles: the count does not wrap
    big = 2 ** 20
    assert q(UPPER, big, big, 191, 191, 0, big) == big * (big - 1) // 2 * 382 * 24
    for kw in ((ALIGNED, 3, 3, 4, 4, 0, 3), (UPPER, 3, 4, 4, 4, 0, 3), (UPPER, 3, 3, 4, 5, 0, 3), (FULL, 3, 3, 4, 4, 0, 4),
               (FULL, 3, 3, 4, 4, 3, 1), (FULL, 3, 3, 4, 4, -1, 2), (FULL, 3, 3, 4, 4, 0, 0), (FULL, 0, 3, 4, 4, 0, 1),
               (FULL, 3, 3, 192, 4, 0, 1)):
        assert q(*kw) < 0, kw


# ---- 2. refusals -------------------------------------------------------------------------------------------------------------------------

def test_the_solve_call_refuses_its_arguments_before_any_launch():
    """As tests/test_host_emd_pairs.py, calls that cannot reach a launch whatever the check under test does: the pointers are null in
    every call up to the null check; the checks after it are given host addresses with n = 150 and no workspace, which the last check
    refuses.  Only the workspace checks themselves stand alone."""
    from lgn import _native as N
    lib = N.lib()
    big = N.EMD_NMAX + 1

    def call(ev0=None, ev1=None, B0=2, B1=2, n=5, m=5, mode=FULL, opts=None, r0=0, k=None, emd=None, s0=None, s1=None, status=None,
             work=None, work_bytes=0):
        return lib.lgn_emd_pairs_grad_f64(ev0, ev1, B0, B1, n, m, mode, opts, r0, B0 if k is None else k, emd, s0, s1, status, work,
                                          work_bytes, None)

    assert call(mode=ALIGNED) < 0 and "FULL and UPPER" in N.last_error()
    assert call(mode=3) < 0 and "FULL and UPPER" in N.last_error()
    assert call(mode=-1) < 0 and "FULL and UPPER" in N.last_error()
    assert call(B0=0, k=1) < 0 and "B0 = 0" in N.last_error()
    assert call(B1=0) < 0 and "B1 = 0" in N.last_error()
    for kw in (dict(n=big), dict(m=big), dict(n=0), dict(m=0)):
        assert call(**kw) < 0 and "outside 1 .." in N.last_error(), kw
    for kw in (dict(r0=-1, k=1), dict(r0=0, k=0), dict(r0=0, k=3), dict(r0=2, k=1), dict(r0=1, k=2), dict(r0=1, k=2 ** 31 - 1)):
        assert call(**kw) < 0 and "rows of the matrix" in N.last_error(), kw
    assert call() < 0 and "null pointer" in N.last_error()
    host = (ctypes.c_double * 8)()
    h = ctypes.cast(host, ctypes.c_void_p)
    ok = dict(ev0=h, ev1=h, s0=h, s1=h, n=150, m=150)
    for miss in ("ev0", "s0", "s1"):
        assert call(**dict(ok, **{miss: None})) < 0 and "null pointer" in N.last_error(), miss
    assert call(**dict(ok, ev1=None)) < 0 and "ev1" in N.last_error()
    assert call(**dict(ok, m=151), mode=UPPER) < 0 and "UPPER" in N.last_error()
    assert call(**ok, mode=UPPER, B0=2, B1=3) < 0 and "UPPER" in N.last_error()
    other = (ctypes.c_double * 8)()
    assert call(**dict(ok, ev1=ctypes.cast(other, ctypes.c_void_p)), mode=UPPER) < 0 and "NULL or ev0" in N.last_error()
    for Rr in (0.0, -1.0, float("inf"), float("nan")):
        assert call(**ok, opts=ctypes.byref(N.EmdOpts(Rr, 1.0, 0, 0))) < 0 and "R = " in N.last_error(), Rr
    for beta in (0.0, -2.0, float("inf"), float("nan")):
        assert call(**ok, opts=ctypes.byref(N.EmdOpts(1.0, beta, 0, 0))) < 0 and "beta = " in N.last_error(), beta
    # n = 150 keeps the flow in a workspace: missing, short, misaligned; emd and status are nullable, so these calls got that far
    need = lib.lgn_emd_workspace_bytes(4, 150)
    assert call(**ok) < 0 and "null work" in N.last_error()
    assert call(**dict(ok, ev1=None), mode=UPPER) < 0 and "null work" in N.last_error()
    assert call(**ok, work=h, work_bytes=need - 8) < 0 and "too short" in N.last_error()
    assert call(**ok, r0=1, k=1, work=h, work_bytes=need // 2 - 8) < 0 and "too short" in N.last_error()      # (one row: two pairs)
    assert call(**dict(ok, m=20), work=ctypes.c_void_p(h.value + 4), work_bytes=need) < 0 and "aligned" in N.last_error()


def test_the_reduce_call_refuses_its_arguments_before_any_launch():
    """Every call below fails a check; none passes them all (that would launch).  The pointers that are not null are host addresses."""
    from lgn import _native as N
    lib = N.lib()
    big = N.EMD_NMAX + 1
    host = (ctypes.c_double * 8)()
    h = ctypes.cast(host, ctypes.c_void_p)

    def call(s0=h, s1=h, G=None, B0=2, B1=2, n=5, m=5, mode=FULL, r0=0, k=None, g0=None, g1=None):
        return lib.lgn_emd_pairs_grad_reduce_f64(s0, s1, G, B0, B1, n, m, mode, r0, B0 if k is None else k, g0, g1, None)

    assert call(mode=ALIGNED, g0=h) < 0 and "FULL and UPPER" in N.last_error()
    assert call(mode=7, g0=h) < 0 and "FULL and UPPER" in N.last_error()
    assert call(B0=0, k=1, g0=h) < 0 and "B0 = 0" in N.last_error()
    assert call(B1=0, g0=h) < 0 and "B1 = 0" in N.last_error()
    for kw in (dict(n=big), dict(m=big), dict(n=0), dict(m=0)):
        assert call(g0=h, **kw) < 0 and "outside 1 .." in N.last_error(), kw
    for kw in (dict(r0=-1, k=1), dict(r0=0, k=0), dict(r0=0, k=3), dict(r0=2, k=1), dict(r0=1, k=2)):
        assert call(g0=h, **kw) < 0 and "rows of the matrix" in N.last_error(), kw
    assert call(g0=h, mode=UPPER, m=6) < 0 and "UPPER" in N.last_error()
    assert call(g0=h, mode=UPPER, B1=3) < 0 and "UPPER" in N.last_error()
    assert call(s0=None, g0=h) < 0 and "null pointer" in N.last_error()
    assert call(s1=None, g0=h) < 0 and "null pointer" in N.last_error()
    assert call() < 0 and "both null" in N.last_error()
    assert call(G=h) < 0 and "both null" in N.last_error()
    assert call(mode=UPPER, g0=h, g1=h) < 0 and "g1 must be null" in N.last_error()
    assert call(mode=UPPER, g1=h) < 0 and "g1 must be null" in N.last_error()


def test_python_refuses_what_the_library_would_and_has_no_cpu_path():
    import torch
    from lgn import emd as M
    x = torch.rand(3, 5, 3, dtype=torch.float64)
    for f in (M.emds_pair_grads, M.emds_grad, lambda *a, **k: M.emds_differentiable(*a, backward="native", **k)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            f(x)
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            f(x, x[:2])
        with pytest.raises(ValueError, match="beta"):
            f(x, beta=0.0)
        with pytest.raises(ValueError, match="finite R"):
            f(x, R=float("inf"))
        with pytest.raises(ValueError, match=r"\(B0, n, 3\)"):
            f(x[0])
        with pytest.raises(ValueError, match="191"):
            f(torch.rand(2, 192, 3, dtype=torch.float64))
    with pytest.raises(ValueError, match="'rows' or 'native'"):
        M.emds_differentiable(x, backward="nonsense")
    with pytest.raises(ValueError, match="'rows' or 'native'"):
        M.emds_differentiable(x, x[:2], backward="nonsense", keep_bytes=0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        M.emds_differentiable(x, backward="native", keep_bytes=0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):                          # the default is the composition it always was
        M.emds_differentiable(x)


# ---- 3. the restatement of the weighted sum ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("B0,B1", [(3, 4), (1, 4), (3, 1), (7, 9)])
def test_the_full_restatement_is_the_weighted_sum(B0, B1):
    """Against np.einsum within (T + 1) 2^-52 sum |terms| (T terms per sum: either order is good to (T - 1) 2^-53 of that sum), the
    bound of the matrix test of tests/test_gpu_emd_opts_grad.py."""
    rng = np.random.default_rng(100 * B0 + B1)
    n, m = 5, 8
    s0, s1 = rng.normal(size=(B0 * B1, n, 3)), rng.normal(size=(B0 * B1, m, 3))
    G = rng.normal(size=(B0, B1))
    G[rng.random((B0, B1)) < 0.2] = 0.0
    g0, g1 = R.reduce_full(s0, s1, G, B0, B1)
    a0, a1 = R.abs_terms_full(s0, s1, G, B0, B1)
    w0 = np.einsum("ij,ijnc->inc", G, s0.reshape(B0, B1, n, 3))
    w1 = np.einsum("ij,ijmc->jmc", G, s1.reshape(B0, B1, m, 3))
    assert (np.abs(g0 - w0) <= (B1 + 1) * 2.0 ** -52 * a0).all() and (np.abs(g1 - w1) <= (B0 + 1) * 2.0 ** -52 * a1).all()
    ones = R.reduce_full(s0, s1, None, B0, B1)
    same = R.reduce_full(s0, s1, np.ones((B0, B1)), B0, B1)
    assert np.array_equal(ones[0], same[0]) and np.array_equal(ones[1], same[1])
    # a one-hot G picks that pair's rows
    hot = np.zeros((B0, B1))
    hot[B0 - 1, 0] = 1.0
    p0, p1 = R.reduce_full(s0, s1, hot, B0, B1)
    assert np.array_equal(p0[B0 - 1], s0[(B0 - 1) * B1]) and np.array_equal(p1[0], s1[(B0 - 1) * B1])
    assert not p0[:B0 - 1].any() and not p1[1:].any()


@pytest.mark.parametrize("B", [1, 2, 4, 9])
def test_the_upper_restatement_is_the_weighted_sum_of_both_roles(B):
    rng = np.random.default_rng(200 + B)
    n, pairs = 6, R.upper_pairs(B)
    assert [R.upper_index(i, j, B) for i, j in pairs] == list(range(len(pairs)))
    s0, s1 = rng.normal(size=(len(pairs), n, 3)), rng.normal(size=(len(pairs), n, 3))
    G = rng.normal(size=(B, B))
    G[rng.random((B, B)) < 0.2] = 0.0
    g = R.reduce_upper(s0, s1, G, B)
    want, a = np.zeros((B, n, 3)), np.zeros((B, n, 3))
    for p, (i, j) in enumerate(pairs):
        w = G[i, j] + G[j, i]
        want[i] += w * s0[p]
        want[j] += w * s1[p]
        a[i] += np.abs(w * s0[p])
        a[j] += np.abs(w * s1[p])
    assert (np.abs(g - want) <= B * 2.0 ** -52 * a).all()                                # (T = B - 1 terms per sum)
    assert np.array_equal(R.reduce_upper(s0, s1, None, B), R.reduce_upper(s0, s1, np.ones((B, B)), B))
    if B >= 2:
        hot = np.zeros((B, B))
        hot[B - 1, 0] = 1.0                                                              # below the diagonal: the pair (0, B - 1)
        one = R.reduce_upper(s0, s1, hot, B)
        p = R.upper_index(0, B - 1, B)
        assert np.array_equal(one[0], s0[p]) and np.array_equal(one[B - 1], s1[p]) and not one[1:B - 1].any()
