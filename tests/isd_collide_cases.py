"""What m4ri_amd_isd_collide_search_dev (include/m4ri_amd.h) has to give, in NumPy on the unpacked bits of one member, written literally
from the header as the composition it is defined as: tests/exchange_cases.py's exchange for the steps before an iteration,
tests/collide_cases.py's expect on the window order[k : k + ell] for its key, tests/isd_cases.py's iteration_seed for the seed of the
steps.  tests/test_isd_collide_search_plan.py pins it to those parts and to tests/isd_cases.py's search;
tests/test_gpu_isd_collide_search.py and tests/test_gpu_far_isd_collide_search.py judge the kernel with it."""
from collections import namedtuple
from math import comb

import numpy as np

import collide_cases as cc
import exchange_cases as xc
import isd_cases as ic
import rowsums_cases as rc

Result = namedtuple("Result", "bits pivots order best best_iter iters_run done W keys")


def window(order, pivot_rows, ell):
    """The window of an iteration: entries pivot_rows .. pivot_rows + ell - 1 of the order as it stands; empty at ell = 0."""
    return [] if ell == 0 else [int(c) for c in order[pivot_rows: pivot_rows + ell]]


def word_of(bits, pivot_rows, key, k1, t1, t2):
    """V (row pivot_rows, or zero) ^ rows S1 ^ rows S2 of the pair of the key's rank on this form."""
    k = pivot_rows
    w = bits[k].copy() if bits.shape[0] > k else np.zeros(bits.shape[1], dtype=np.uint8)
    r1, r2 = divmod(key & ((1 << 40) - 1), comb(k - k1, t2))
    for i in rc.unrank(r1, t1):
        w ^= bits[i]
    for i in rc.unrank(r2, t2):
        w ^= bits[k1 + i]
    return w


def search(bits, pivots, rank, pivot_rows, iters, steps, seed, k1, t1, t2, ell, w_min, w_stop, b=0, order=None):
    """The rule for member b.  bits: uint8 nrows x ncols, the form as the caller left it; pivots: min(pivot_rows, ncols) entries; order:
    the entries kept (at least pivot_rows + ell of them where ell > 0), or None.  Returns Result: the final bits, pivots and order, best,
    best_iter (-1 with best = -1), iters_run, done, W (the word of the best, None with best = -1) and the keys of the iterations run
    (-2: the window of that iteration had an entry outside).  The arguments are not written."""
    bits = np.array(bits, dtype=np.uint8) & 1
    pivots = np.array(pivots, dtype=np.int32)
    order = None if order is None else np.array(order, dtype=np.int32)
    k = pivot_rows
    assert ell == 0 or (order is not None and len(order) >= k + ell)
    best, best_iter, W, done, run, keys = -1, -1, None, 0, 0, []
    for it in range(iters):
        if it > 0:
            bits, pivots, order, did, _ = xc.exchange(bits, pivots, rank, k, steps, seed=ic.iteration_seed(seed, it), b=b, order=order)
            done += did
        if it > 0 and did == 0:
            key = keys[-1]          # the same form and the same order: the same key
        else:
            key = cc.expect(bits[:k], bits[k] if bits.shape[0] > k else None, k1, t1, t2, window(order, k, ell), w_min)[1]
        keys.append(key)
        if key >= 0 and (best < 0 or (key >> 40) < (best >> 40)):
            best, best_iter, W = key, it, word_of(bits, k, key, k1, t1, t2)
        run = it + 1
        if best >= 0 and (best >> 40) <= w_stop:
            break
    return Result(bits, pivots, order, best, best_iter, run, done, W, keys)
