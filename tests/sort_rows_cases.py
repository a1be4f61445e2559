"""What m4ri_amd_sort_rows_batch_dev (include/m4ri_amd.h) has to give, in NumPy on the unpacked bits of one member: A (m x n, uint8, the
rows that count) and a window `cols`.  Row i goes before row j iff (key_i, w_i[0], ..., w_i[words-1], i) is lexicographically smaller
than the same tuple of j: key = the window bits as one unsigned number (lists_collide_cases.window_keys), w = the row's 64-bit words as
unsigned numbers, the bits behind column n zero.  The rule is written TWICE -- by_lexsort() with np.lexsort over (index, the words from
last to first, key), by_sorted() with Python's sorted on the tuples -- and tests/test_sort_rows_plan.py holds the two to each other and to
np.unique(axis=0); tests/test_gpu_sort_rows.py judges the kernels with them.  uniq and mult come from either as the heads and the
lengths of the runs of equal rows."""
import numpy as np

import lists_collide_cases as lc

REFUSED_UCOUNT = -1


def words(A):
    """The rows as unsigned 64-bit words (m x width(n)), the bits behind column n zero."""
    A = np.asarray(A, dtype=np.uint8)
    if A.shape[1] == 0:
        return np.zeros((A.shape[0], 0), dtype=np.uint64)
    return lc.pack(A).view(np.uint64)


def by_lexsort(A, cols):
    """The order as np.lexsort gives it: its LAST key is the first to count."""
    A = np.asarray(A, dtype=np.uint8)
    w = words(A)
    keys = (np.arange(A.shape[0], dtype=np.int64),) + tuple(w[:, j] for j in range(w.shape[1] - 1, -1, -1)) + (lc.window_keys(A, cols),)
    return np.lexsort(keys).astype(np.int64)


def by_sorted(A, cols):
    """The same by Python's sorted on the tuples (key, w[0], ..., w[words-1], i)."""
    A = np.asarray(A, dtype=np.uint8)
    w, key = words(A), lc.window_keys(A, cols)
    tuples = [(int(key[i]),) + tuple(int(x) for x in w[i]) + (i,) for i in range(A.shape[0])]
    return np.array([t[-1] for t in sorted(tuples)], dtype=np.int64)


def classes(A, order):
    """(uniq, mult) of an order: the heads of the runs of equal rows (their smallest index, since the index is the last thing the order
    looks at) and the lengths of the runs."""
    A = np.asarray(A, dtype=np.uint8)
    m = len(order)
    if m == 0:
        return np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64)
    S = A[order]
    head = np.ones(m, dtype=bool)
    head[1:] = (S[1:] != S[:-1]).any(axis=1)
    at = np.nonzero(head)[0]
    return order[at], np.diff(np.append(at, m)).astype(np.int64)


def expect(A, cols, rule=by_lexsort):
    """(order, uniq, mult) of one member, or None for a refused one (a window entry outside 0 .. n-1)."""
    A = np.asarray(A, dtype=np.uint8)
    if lc.refused(A.shape[1], cols):
        return None
    order = rule(A, cols)
    return (order,) + classes(A, order)


def pool_rows(rng, rows, n, pool):
    """`rows` rows of n bits drawn from a pool of `pool` random rows: classes are large."""
    P = rng.integers(0, 2, size=(pool, n), dtype=np.uint8)
    return P[rng.integers(0, pool, size=rows)]
