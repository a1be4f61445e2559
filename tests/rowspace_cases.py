"""What m4ri_amd_rowspace_weights_batch_dev (include/m4ri_amd.h) has to give, in NumPy by brute force on the unpacked bits of one
member: G (uint8, k x n), V (uint8, n, or None).  Message x selects the rows i of G with bit i of x set; c(x) = V ^ their sum.
tests/test_rowspace_weights_plan.py pins these to hand-checked codes and to the reference's mzd_make_table;
tests/test_gpu_rowspace_weights.py judges the kernels with them."""
from math import comb

import numpy as np

CHUNK = 1 << 16  # messages per product


def messages(k, x0, x1):
    """The bits of the messages x0 .. x1-1 (uint8, (x1 - x0) x k): column i is bit i of x."""
    x = np.arange(x0, x1, dtype=np.int64)
    return ((x[:, None] >> np.arange(k, dtype=np.int64)[None, :]) & 1).astype(np.uint8)


def weights(G, V=None):
    """wt(c(x)) for x = 0 .. 2^k - 1 (int64): C = (X @ G + V) % 2, row sums.  The products are exact in float32 (sums of at most k
    ones), which keeps 2^20 messages quick."""
    k, n = G.shape
    v = np.zeros(n, dtype=np.int64) if V is None else V.astype(np.int64)
    Gf = G.astype(np.float32)
    out = np.empty(1 << k, dtype=np.int64)
    for x0 in range(0, 1 << k, CHUNK):
        x1 = min(1 << k, x0 + CHUNK)
        C = (messages(k, x0, x1).astype(np.float32) @ Gf).astype(np.int64)
        out[x0:x1] = ((C + v[None, :]) % 2).sum(axis=1)
    return out


def hist_of(w, n):
    """hist[j] = the number of messages of weight j, n + 1 entries."""
    return np.bincount(w, minlength=n + 1).astype(np.int64)


def lightest_of(w, w_min):
    """The minimum of (wt << 40) | x over the x with wt >= w_min, -1 if there is none."""
    x = np.flatnonzero(w >= w_min)
    if x.size == 0:
        return -1
    return int(((w[x] << 40) | x).min())


def expect(G, V, w_min):
    """(hist, lightest) of one member."""
    w = weights(G, V)
    return hist_of(w, G.shape[1]), lightest_of(w, w_min)


def doubled_identity(k):
    """G = [I_k | I_k]: c(x) repeats x, so hist[2j] = C(k, j); with V = ones on the first half every word weighs k."""
    eye = np.eye(k, dtype=np.uint8)
    return np.concatenate([eye, eye], axis=1)


def doubled_identity_hist(k):
    h = np.zeros(2 * k + 1, dtype=np.int64)
    h[0::2] = [comb(k, j) for j in range(k + 1)]
    return h
