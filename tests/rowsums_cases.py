"""What m4ri_amd_row_sums_weights_batch_dev (include/m4ri_amd.h) has to give, in NumPy by brute force on the unpacked bits of one
member: G (uint8, k x n), V (uint8, n, or None).  A set S = {i_0 < ... < i_{t-1}} of row indices has the word c(S) = V ^ the rows of G
in S and the colexicographic rank r(S) = sum_j C(i_j, j + 1).  Closed forms for members too large for brute force.
tests/test_row_sums_weights_plan.py pins these to hand-checked codes and to tests/rowspace_cases.py;
tests/test_gpu_row_sums_weights.py judges the kernels with them."""
from itertools import combinations, islice
from math import comb

import numpy as np

CHUNK = 1 << 14  # sets per block of the brute force


def rank(S):
    """The colexicographic rank of the set S of distinct row indices."""
    return sum(comb(i, j + 1) for j, i in enumerate(sorted(S)))


def unrank(r, t):
    """The set of t row indices of rank r, ascending."""
    out = []
    for m in range(t, 0, -1):
        i = m - 1
        while comb(i + 1, m) <= r:  # the largest i with C(i, m) <= r
            i += 1
        out.append(i)
        r -= comb(i, m)
    assert r == 0
    return tuple(reversed(out))


def weights(G, V, t):
    """(wt(c(S)), r(S)) for all C(k, t) sets S, two int64 arrays in the order of itertools.combinations."""
    k, n = G.shape
    v = np.zeros(n, dtype=np.uint8) if V is None else V.astype(np.uint8)
    if t == 0:
        return np.array([int(v.sum())], dtype=np.int64), np.zeros(1, dtype=np.int64)
    total = comb(k, t)
    wts, ranks = np.empty(total, dtype=np.int64), np.empty(total, dtype=np.int64)
    binom = np.array([[comb(i, j + 1) for j in range(t)] for i in range(max(k, 1))], dtype=np.int64)
    it, at = combinations(range(k), t), 0
    while at < total:
        idx = np.array(list(islice(it, CHUNK)), dtype=np.int64).reshape(-1, t)
        c = np.bitwise_xor.reduce(G[idx], axis=1) ^ v[None, :]
        wts[at:at + len(idx)] = c.sum(axis=1, dtype=np.int64)
        ranks[at:at + len(idx)] = binom[idx, np.arange(t)[None, :]].sum(axis=1)
        at += len(idx)
    return wts, ranks


def hist_of(w, n):
    return np.bincount(w, minlength=n + 1).astype(np.int64)


def lightest_of(w, r, w_min):
    """The minimum of (wt << 40) | rank over the sets with wt >= w_min, -1 if there is none."""
    sel = w >= w_min
    if not sel.any():
        return -1
    return int(((w[sel] << 40) | r[sel]).min())


def expect(G, V, t, w_min):
    """(hist, lightest) of one member."""
    w, r = weights(G, V, t)
    return hist_of(w, G.shape[1]), lightest_of(w, r, w_min)


# ---- closed forms -----------------------------------------------------------------------------------------------------------------------

def doubled_identity(k):
    """G = [I_k | I_k]: the sum of t rows weighs 2t."""
    eye = np.eye(k, dtype=np.uint8)
    return np.concatenate([eye, eye], axis=1)


def doubled_identity_expect(k, t, w_min):
    h = np.zeros(2 * k + 1, dtype=np.int64)
    if t <= k:
        h[2 * t] = comb(k, t)
    return h, ((2 * t) << 40 if t <= k and 2 * t >= w_min else -1)   # every set ties: rank 0


def rigged(k, a, b, c):
    """R(k, a, b, c): the doubled identity with the second half of row c replaced by e_a ^ e_b (a, b, c distinct)."""
    G = doubled_identity(k)
    G[c, k:] = 0
    G[c, k + a] = G[c, k + b] = 1
    return G


def rigged_hist(k, t):
    """The weight distribution of the t-sums of R(k, a, b, c), whatever a, b, c.  A set without c weighs 2t.  A set with c and j of
    {a, b} has t ones on the left and, on the right, the t - 1 other rows' ones with e_a ^ e_b added: t - 1 + 2 - 2j.  So it weighs
    2t + 1 - 2j, and there are C(2, j) * C(k - 3, t - 1 - j) of them."""
    h = np.zeros(2 * k + 1, dtype=np.int64)
    h[2 * t] += comb(k - 1, t)
    for j in range(3):
        if t - 1 - j >= 0:
            h[2 * t + 1 - 2 * j] += comb(2, j) * comb(k - 3, t - 1 - j)
    return h


def rigged_lightest(k, a, b, c, t):
    """lightest at w_min = 1 for t >= 3: the sets with a, b and c weigh 2t - 3, less than all others; the smallest rank among them
    fills up with the smallest free rows."""
    free = [i for i in range(k) if i not in (a, b, c)][:t - 3]
    return ((2 * t - 3) << 40) | rank([a, b, c] + free)
