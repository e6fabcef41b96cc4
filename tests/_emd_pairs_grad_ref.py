"""The weighted fixed-order sum of per-pair EMD gradients (csrc/emd_pairs_grad.hip, include/lgn_amd.h), restated in numpy: one rounded
product and one rounded sum per pair, partners ascending, every sum from +0.0.  numpy rounds ``w * s`` and ``acc + term`` separately
(no fused multiply-add), which is the kernel's arithmetic; the loops below are its order.

    FULL   slabs s0 (B0 B1, n, 3), s1 (B0 B1, m, 3), pair p = i B1 + j
           g0[i] = sum over j ascending of G[i, j] s0[i B1 + j]        g1[j] = sum over i ascending of G[i, j] s1[i B1 + j]
    UPPER  slabs s0, s1 (B (B - 1) / 2, n, 3), the pairs i < j row-major over the upper triangle; w(i, j) = G[i, j] + G[j, i]
           g[e]  = sum over k < e ascending of w(k, e) s1[pair (k, e)], then over k > e ascending of w(e, k) s0[pair (e, k)]
"""
import numpy as np


def upper_pairs(B):
    return [(i, j) for i in range(B) for j in range(i + 1, B)]


def upper_index(i, j, B):
    """the pair number of i < j"""
    return i * (2 * B - i - 1) // 2 + (j - i - 1)


def reduce_full(s0, s1, G, B0, B1):
    s0, s1 = np.asarray(s0, np.float64), np.asarray(s1, np.float64)
    G = np.ones((B0, B1)) if G is None else np.asarray(G, np.float64)
    g0 = np.zeros((B0,) + s0.shape[1:])
    g1 = np.zeros((B1,) + s1.shape[1:])
    for i in range(B0):
        for j in range(B1):
            term = G[i, j] * s0[i * B1 + j]
            g0[i] = g0[i] + term
    for j in range(B1):
        for i in range(B0):
            term = G[i, j] * s1[i * B1 + j]
            g1[j] = g1[j] + term
    return g0, g1


def reduce_upper(s0, s1, G, B):
    s0, s1 = np.asarray(s0, np.float64), np.asarray(s1, np.float64)
    G = np.ones((B, B)) if G is None else np.asarray(G, np.float64)
    g = np.zeros((B,) + s0.shape[1:])
    for e in range(B):
        for k in range(e):
            w = G[k, e] + G[e, k]
            term = w * s1[upper_index(k, e, B)]
            g[e] = g[e] + term
        for k in range(e + 1, B):
            w = G[e, k] + G[k, e]
            term = w * s0[upper_index(e, k, B)]
            g[e] = g[e] + term
    return g


def abs_terms_full(s0, s1, G, B0, B1):
    """sum of |terms| of every output of reduce_full, and the number of terms of each sum: (a0, T0 = B1), (a1, T1 = B0)"""
    G = np.ones((B0, B1)) if G is None else np.asarray(G, np.float64)
    a0 = np.abs(G[:, :, None, None] * np.asarray(s0).reshape(B0, B1, *s0.shape[1:])).sum(1)
    a1 = np.abs(G[:, :, None, None] * np.asarray(s1).reshape(B0, B1, *s1.shape[1:])).sum(0)
    return a0, a1
