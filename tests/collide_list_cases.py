"""What m4ri_amd_row_sums_collide_list_batch_dev and m4ri_amd_row_sums_words_batch_dev (include/m4ri_amd.h) have to give, in NumPy on
the unpacked bits of one member, on top of tests/collide_cases.py: of the colliding pairs (collide_cases.collisions: weights and pair
ranks) those with w_min <= wt <= w_max QUALIFY; the list holds their keys (wt << 40) | rank, count their number, a refused member has
count -1 and no key; words_of() is the word V ^ rows S1 ^ rows S2 of a pair rank.  tests/test_row_sums_collide_list_plan.py holds
these to brute force on a hand-checked member; tests/test_gpu_row_sums_collide_list.py judges the kernels with them."""
from math import comb

import numpy as np

import collide_cases as cc

RANK_MASK = (1 << 40) - 1
REFUSED_COUNT = -1


def keys_of(w, r, w_min, w_max):
    """The sorted keys of the qualifying pairs among the colliding ones (w: weights, r: pair ranks)."""
    w, r = np.asarray(w, dtype=np.int64), np.asarray(r, dtype=np.int64)
    take = (w >= w_min) & (w <= w_max)
    return np.sort((w[take] << 40) | r[take])


def expect(G, V, k1, t1, t2, cols, w_min, w_max):
    """(sorted qualifying keys, count) of one member; a window entry outside 0 .. n-1: (no keys, -1)."""
    n = G.shape[1]
    if cc.refused(n, cols):
        return np.zeros(0, dtype=np.int64), REFUSED_COUNT
    keys = keys_of(*cc.collisions(G, V, k1, t1, t2, cols), w_min, w_max)
    return keys, len(keys)


def words_of(G, V, k1, t1, t2, ranks):
    """The words (len(ranks) x n, uint8) of the pairs of these ranks: V ^ rows S1 ^ rows S2, S1 the t1-set of the left rows of rank
    r // N2, S2 the t2-set of the right rows whose {i - k1} has rank r % N2."""
    k, n = G.shape
    ranks = np.asarray(list(ranks), dtype=np.int64).reshape(-1)
    n1, n2 = comb(k1, t1), comb(k - k1, t2)
    assert ((ranks >= 0) & (ranks < n1 * n2)).all()
    if len(ranks) == 0:
        return np.zeros((0, n), dtype=np.uint8)
    L, R = cc.half_sums(G, k1, t1, t2)
    v = np.zeros(n, dtype=np.uint8) if V is None else V.astype(np.uint8)
    return L[ranks // n2] ^ R[ranks % n2] ^ v[None, :]
