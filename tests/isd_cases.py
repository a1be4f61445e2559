"""What m4ri_amd_isd_search_dev (include/m4ri_amd.h) has to give, in NumPy on the unpacked bits of one member, written literally from the
header as the composition it is defined as: tests/exchange_cases.py's exchange for the steps before an iteration, tests/rowsums_cases.py's
expect for its key.  tests/test_isd_search_plan.py pins it to those two and to the elimination from scratch;
tests/test_gpu_isd_search.py and tests/test_gpu_far_isd_search.py judge the kernels with it."""
from collections import namedtuple

import numpy as np

import exchange_cases as xc
import rowsums_cases as rc
from order_cases import splitmix

Result = namedtuple("Result", "bits pivots order best best_iter iters_run done W keys")


def iteration_seed(seed, it):
    """seed_it: output number `it` of the stream seeded `seed`."""
    return splitmix(seed & ((1 << 64) - 1), it)


def word_of(bits, pivot_rows, key, t):
    """c(S) of the key on this form: V (row pivot_rows, or zero) ^ the rows of the set of the key's rank."""
    w = bits[pivot_rows].copy() if bits.shape[0] > pivot_rows else np.zeros(bits.shape[1], dtype=np.uint8)
    for i in rc.unrank(key & ((1 << 40) - 1), t):
        w ^= bits[i]
    return w


def search(bits, pivots, rank, pivot_rows, iters, steps, seed, t, w_min, w_stop, b=0, order=None):
    """The rule for member b.  bits: uint8 nrows x ncols, the form as the caller left it; pivots: min(pivot_rows, ncols) entries; order:
    the entries kept, or None.  Returns Result: the final bits, pivots and order, best, best_iter (-1 with best = -1), iters_run, done,
    W (the word of the best, None with best = -1) and the keys of the iterations run.  The arguments are not written."""
    bits = np.array(bits, dtype=np.uint8) & 1
    pivots = np.array(pivots, dtype=np.int32)
    order = None if order is None else np.array(order, dtype=np.int32)
    k = pivot_rows
    best, best_iter, W, done, run, keys = -1, -1, None, 0, 0, []
    for it in range(iters):
        if it > 0:
            bits, pivots, order, did, _ = xc.exchange(bits, pivots, rank, k, steps, seed=iteration_seed(seed, it), b=b, order=order)
            done += did
        if it > 0 and did == 0:
            key = keys[-1]          # the same form: the same key
        else:
            key = rc.expect(bits[:k], bits[k] if bits.shape[0] > k else None, t, w_min)[1]
        keys.append(key)
        if key >= 0 and (best < 0 or (key >> 40) < (best >> 40)):
            best, best_iter, W = key, it, word_of(bits, k, key, t)
        run = it + 1
        if best >= 0 and (best >> 40) <= w_stop:
            break
    return Result(bits, pivots, order, best, best_iter, run, done, W, keys)
