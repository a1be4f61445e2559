"""What m4ri_amd_row_sums_collide_batch_dev (include/m4ri_amd.h) has to give, in NumPy on the unpacked bits of one member: G (uint8,
k x n), V (uint8, n, or None), the window `cols` (a sequence of column indices, any order, repeats allowed).  Rows 0 .. k1-1 are the
left rows, k1 .. k-1 the right rows; S1 is a set of t1 left rows of colexicographic rank r1, S2 a set of t2 right rows, r2 the rank of
{i - k1}; the word is c = V ^ rows S1 ^ rows S2, the pair's rank r1 * N2 + r2, and it collides iff c is 0 at every window column.
brute() takes every pair; joined() finds the collisions by sorting the keys and weighs only those, for members too big for brute().
Closed forms on the members of tests/rowsums_cases.py.  tests/test_row_sums_collide_plan.py holds these to each other, to a
hand-checked member and to tests/rowsums_cases.py; tests/test_gpu_row_sums_collide.py judges the kernels with them."""
from itertools import combinations
from math import comb

import numpy as np

import rowsums_cases as rc

BRUTE_MAX = 1 << 26  # N1 * N2 * n bytes brute() is asked for at most by collisions()
CHUNK = 1 << 14      # pairs per block of joined()'s weighing


def subsets(k, t):
    """All t-subsets of range(k) as an (C(k, t), t) array of ascending rows; row r is the set of colexicographic rank r."""
    if t == 0:
        return np.zeros((1, 0), dtype=np.int64)
    idx = np.array(list(combinations(range(k), t)), dtype=np.int64).reshape(-1, t)
    if len(idx) == 0:
        return idx
    binom = np.array([[comb(i, j + 1) for j in range(t)] for i in range(k)], dtype=np.int64)
    out = np.empty_like(idx)
    out[binom[idx, np.arange(t)[None, :]].sum(axis=1)] = idx
    return out


def half_sums(G, k1, t1, t2):
    """(L, R): the sums of the t1-subsets of the left rows (N1 x n) and of the t2-subsets of the right rows (N2 x n), by rank."""
    n = G.shape[1]
    left, right = subsets(k1, t1), subsets(G.shape[0] - k1, t2) + k1
    xor = lambda sets: np.bitwise_xor.reduce(G[sets], axis=1).reshape(len(sets), n) if sets.shape[1] else np.zeros((len(sets), n), dtype=np.uint8)
    return xor(left), xor(right)


def _v(V, n):
    return np.zeros(n, dtype=np.uint8) if V is None else V.astype(np.uint8)


def refused(n, cols):
    return any(not 0 <= int(c) < n for c in cols)


def brute(G, V, k1, t1, t2, cols):
    """(wt, pair rank, collides) of ALL N1 * N2 pairs, three arrays in the order of the pair rank.  The window must be inside."""
    n = G.shape[1]
    L, R = half_sums(G, k1, t1, t2)
    c = L[:, None, :] ^ R[None, :, :] ^ _v(V, n)[None, None, :]
    w = c.sum(axis=2, dtype=np.int64).ravel()
    hit = ~c[:, :, np.asarray(cols, dtype=np.int64)].any(axis=2).ravel()
    return w, np.arange(len(L) * len(R), dtype=np.int64), hit


def _keys(M, cols):
    """The window bits of every row of M as one uint64 (ell <= 64), bit j = column cols[j]."""
    key = np.zeros(len(M), dtype=np.uint64)
    for j, c in enumerate(cols):
        key |= M[:, int(c)].astype(np.uint64) << np.uint64(j)
    return key


def joined(G, V, k1, t1, t2, cols):
    """(wt, pair rank) of the COLLIDING pairs only, in no particular order: the left keys sorted, each right key (with V's) looked up."""
    n = G.shape[1]
    v = _v(V, n)
    L, R = half_sums(G, k1, t1, t2)
    if len(L) == 0 or len(R) == 0:
        return np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64)
    key1, key2 = _keys(L, cols), _keys(R ^ v[None, :], cols)
    order = np.argsort(key1, kind="stable")
    lo, hi = np.searchsorted(key1[order], key2, "left"), np.searchsorted(key1[order], key2, "right")
    cnt = hi - lo
    r2 = np.repeat(np.arange(len(R), dtype=np.int64), cnt)
    within = np.arange(int(cnt.sum()), dtype=np.int64) - np.repeat(np.cumsum(cnt) - cnt, cnt)
    r1 = order[np.repeat(lo, cnt) + within].astype(np.int64)
    w = np.empty(len(r1), dtype=np.int64)
    for at in range(0, len(r1), CHUNK):
        s = slice(at, at + CHUNK)
        w[s] = (L[r1[s]] ^ R[r2[s]] ^ v[None, :]).sum(axis=1, dtype=np.int64)
    return w, r1 * len(R) + r2


def collisions(G, V, k1, t1, t2, cols):
    """(wt, pair rank) of the colliding pairs of a member whose window is inside: by brute() where that is small, else by joined()."""
    k, n = G.shape
    if comb(k1, t1) * comb(k - k1, t2) * max(n, 1) <= BRUTE_MAX:
        w, r, hit = brute(G, V, k1, t1, t2, cols)
        return w[hit], r[hit]
    return joined(G, V, k1, t1, t2, cols)


def refused_form(n):
    return np.full(n + 1, -1, dtype=np.int64), -2


def expect(G, V, k1, t1, t2, cols, w_min):
    """(hist, lightest) of one member; a window entry outside 0 .. n-1 gives the refused form: every bin -1, lightest -2."""
    n = G.shape[1]
    if refused(n, cols):
        return refused_form(n)
    w, r = collisions(G, V, k1, t1, t2, cols)
    return rc.hist_of(w, n), rc.lightest_of(w, r, w_min)


def pair_rank(S1, S2, k1, k, t2):
    return rc.rank(S1) * comb(k - k1, t2) + rc.rank([i - k1 for i in S2])


# ---- closed forms -----------------------------------------------------------------------------------------------------------------------

def doubled_identity_zeros(k, z):
    """[I_k | I_k | 0]: z zero columns behind rowsums_cases.doubled_identity(k).  On a window inside them every pair collides."""
    return np.concatenate([rc.doubled_identity(k), np.zeros((k, z), dtype=np.uint8)], axis=1)


def doubled_identity_expect(k, z, k1, t1, t2, cols, w_min):
    """(hist, lightest) of doubled_identity_zeros(k, z) without V: every pair weighs 2 (t1 + t2), and it collides iff it has none of the
    rows J whose columns (j and k + j) the window names.  All colliding pairs tie: the lightest is the one of the smallest rank, the
    first free rows of each half."""
    n, t = 2 * k + z, t1 + t2
    J = {int(c) % k for c in cols if c < 2 * k}
    free1, free2 = [i for i in range(k1) if i not in J], [i for i in range(k1, k) if i not in J]
    count = comb(len(free1), t1) * comb(len(free2), t2)
    h = np.zeros(n + 1, dtype=np.int64)
    h[2 * t] = count
    return h, ((2 * t) << 40 | pair_rank(free1[:t1], free2[:t2], k1, k, t2) if count and 2 * t >= w_min else -1)


def rigged_window(k, a, b):
    """The window of rigged_expect: the two columns of the right half that row c of rowsums_cases.rigged(k, a, b, c) took over."""
    return [k + b, k + a]


def rigged_expect(k, a, b, c, k1, t1, t2, w_min):
    """(hist, lightest) of rowsums_cases.rigged(k, a, b, c) with a, b left rows and c a right row, on rigged_window(k, a, b), without V.
    Column k + a of the word is [a in S] ^ [c in S], column k + b likewise with b: the pair collides iff it has none of a, b, c, and
    then weighs 2t, or all three, and then weighs 2t - 3 (t = t1 + t2; row c's two ones on the right cancel those of rows a and b, its
    own diagonal one is missing)."""
    assert a < k1 and b < k1 <= c and a != b
    t, k2 = t1 + t2, k - k1
    h = np.zeros(2 * k + 1, dtype=np.int64)
    none, allthree = comb(k1 - 2, t1) * comb(k2 - 1, t2), (comb(k1 - 2, t1 - 2) * comb(k2 - 1, t2 - 1) if t1 >= 2 and t2 >= 1 else 0)
    h[2 * t] += none
    cands = []
    if allthree:
        h[2 * t - 3] += allthree
        free1, free2 = [i for i in range(k1) if i not in (a, b)], [i for i in range(k1, k) if i != c]
        cands.append((2 * t - 3, pair_rank([a, b] + free1[:t1 - 2], [c] + free2[:t2 - 1], k1, k, t2)))
    if none:
        free1, free2 = [i for i in range(k1) if i not in (a, b)], [i for i in range(k1, k) if i != c]
        cands.append((2 * t, pair_rank(free1[:t1], free2[:t2], k1, k, t2)))
    keys = [(w << 40) | r for w, r in cands if w >= w_min]
    return h, (min(keys) if keys else -1)
