"""The host side of m4ri_amd_isd_collide_search_dev, without a GPU: the NumPy rule of tests/isd_collide_cases.py against the parts it
composes (tests/exchange_cases.py, tests/collide_cases.py, tests/isd_cases.py's seeds) run separately and against tests/isd_cases.py's
search where the join degenerates, the boundaries of m4ri_amd_plan_isd_collide_search and the argument checks (which run before any HIP
call; the expected codes are written here by hand from the header).  tests/test_gpu_isd_collide_search.py judges the kernel with the
same rule."""
from math import comb

import numpy as np
import pytest

import collide_cases as cc
import exchange_cases as xc
import isd_cases as ic
import isd_collide_cases as icc
import m4ri_amd
import order_cases as oc

INVALID, NOT_SUPPORTED = 1, 801      # hipErrorInvalidValue, hipErrorNotSupported
LDS_BUDGET = 160 * 1024              # batch_common.h's BATCH_LDS_BUDGET
THREADS = "M4RI_AMD_ISD_COLLIDE_SEARCH_THREADS"
SEARCH, PLAN = m4ri_amd.isd_collide_search_dev, m4ri_amd.plan_isd_collide_search     # what this module is about: without the call none of it holds


def _state(rng, k, n, followers):
    """A full-rank k x n generator over `followers` more rows in reduced form on a random order: (as it was, the form, pivots, order)."""
    while True:
        A = rng.integers(0, 2, size=(k + followers, n), dtype=np.uint8)
        order = rng.permutation(n).astype(np.int32)
        S, rank, piv = oc.ech_order(A, order, 1, k)
        if rank == k:
            return A, S, piv, order


# ---- the rule -----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k,n,followers,k1,t1,t2,ell", [(4, 12, 1, 2, 1, 1, 0), (8, 24, 1, 4, 1, 1, 3), (8, 24, 2, 3, 2, 1, 2), (12, 40, 0, 6, 2, 2, 5),
                                                        (16, 70, 1, 0, 0, 2, 4), (16, 70, 1, 16, 2, 0, 4), (6, 20, 1, 2, 3, 1, 1)])
def test_one_iteration_is_the_collision_step(k, n, followers, k1, t1, t2, ell):
    rng = np.random.default_rng(10 * k + t1 + ell)
    _A, S, piv, order = _state(rng, k, n, followers)
    for w_min in (0, 1, n + 1):
        r = icc.search(S, piv, k, k, 1, 3, 5, k1, t1, t2, ell, w_min, -1, order=order)
        want = cc.expect(S[:k], S[k] if followers else None, k1, t1, t2, order[k: k + ell], w_min)[1]
        assert r.best == want and r.keys == [want] and r.iters_run == 1 and r.done == 0 and r.best_iter == (0 if want >= 0 else -1)
        assert np.array_equal(r.bits, S) and np.array_equal(r.pivots, piv) and np.array_equal(r.order, order)
        if want >= 0:
            assert int(r.W.sum()) == want >> 40 and not r.W[order[k: k + ell]].any()       # the word vanishes on the window
            S1, S2 = m4ri_amd.row_pair_unrank(want & ((1 << 40) - 1), k1, k, t1, t2)
            word = S[k].copy() if followers else np.zeros(n, dtype=np.uint8)
            for i in list(S1) + list(S2):
                word ^= S[i]
            assert np.array_equal(r.W, word)
        else:
            assert r.W is None and (want == -1)


@pytest.mark.parametrize("k,n,followers,k1,t1,t2,ell,steps", [(4, 12, 1, 2, 1, 1, 1, 1), (8, 24, 2, 4, 1, 1, 3, 3), (16, 64, 1, 8, 1, 1, 4, 1),
                                                              (20, 70, 1, 10, 2, 1, 6, 2)])
def test_the_loop_is_the_composition(k, n, followers, k1, t1, t2, ell, steps):
    """The loop against its parts called one after the other by hand, and on these full-rank members the final form against ech_order
    from scratch on the final pivots; the stop at the first iteration whose running minimum is low enough."""
    rng = np.random.default_rng(100 * k + n)
    for member in range(5):
        A, S, piv, order = _state(rng, k, n, followers)
        iters, seed = 9, 1000 + member
        r = icc.search(S, piv, k, k, iters, steps, seed, k1, t1, t2, ell, 1, -1, b=member, order=order)
        cur, cp, co, keys, done = S, piv, order, [], 0
        for it in range(iters):
            if it:
                cur, cp, co, did, _ = xc.exchange(cur, cp, k, k, steps, seed=ic.iteration_seed(seed, it), b=member, order=co)
                done += did
            keys.append(cc.expect(cur[:k], cur[k], k1, t1, t2, co[k: k + ell], 1)[1])
        assert r.keys == keys and r.done == done and done > 0 and r.iters_run == iters
        assert np.array_equal(r.bits, cur) and np.array_equal(r.pivots, cp) and np.array_equal(r.order, co)
        assert sorted(co.tolist()) == list(range(n))                                    # the exchanges only swap entries of the order
        weights = [key >> 40 if key >= 0 else 1 << 30 for key in keys]
        if min(weights) < 1 << 30:
            assert r.best_iter == weights.index(min(weights)) and r.best == keys[r.best_iter]            # the earliest among equal weights
            w_stop = sorted(w for w in weights if w < 1 << 30)[len([w for w in weights if w < 1 << 30]) // 2]
            first = next(i for i, w in enumerate(weights) if w <= w_stop)
            s = icc.search(S, piv, k, k, iters, steps, seed, k1, t1, t2, ell, 1, w_stop, b=member, order=order)
            assert s.iters_run == first + 1 and s.best == keys[first] and s.best_iter == first and s.keys == keys[:first + 1]
        else:
            assert r.best == -1 and r.best_iter == -1 and r.W is None
        want, rank, piv3 = oc.ech_order(A, r.pivots, 1, k)
        assert rank == k and np.array_equal(piv3, r.pivots) and np.array_equal(r.bits, want)


@pytest.mark.parametrize("k,n,followers,t,steps", [(3, 9, 1, 1, 1), (8, 20, 2, 2, 3), (16, 64, 1, 1, 1), (12, 40, 0, 3, 2)])
def test_without_a_right_half_and_a_window_it_is_the_plain_search(k, n, followers, t, steps):
    """t2 = 0, k1 = k, ell = 0: N2 = 1, every pair collides and its rank is r1, so the keys are those of isd_cases.search at t = t1."""
    rng = np.random.default_rng(7 * k + t)
    for member in range(4):
        _A, S, piv, order = _state(rng, k, n, followers)
        for w_stop in (-1, n // 4):
            a = icc.search(S, piv, k, k, 8, steps, 50 + member, k, t, 0, 0, 1, w_stop, b=member, order=order)
            b = ic.search(S, piv, k, k, 8, steps, 50 + member, t, 1, w_stop, b=member, order=order)
            assert a.keys == b.keys and (a.best, a.best_iter, a.iters_run, a.done) == (b.best, b.best_iter, b.iters_run, b.done)
            assert np.array_equal(a.bits, b.bits) and np.array_equal(a.pivots, b.pivots) and np.array_equal(a.order, b.order)
            assert (a.W is None and b.W is None) or np.array_equal(a.W, b.W)


def test_a_refused_window_gives_no_best():
    rng = np.random.default_rng(8)
    _A, S, piv, order = _state(rng, 8, 24, 1)
    for bad in (24, -1):
        o = order.copy()
        o[8 + 1] = bad
        r = icc.search(S, piv, 8, 8, 4, 2, 3, 4, 1, 1, 3, 0, -1, order=o)
        assert r.keys == [-2] * 4 and r.best == -1 and r.best_iter == -1 and r.W is None and r.iters_run == 4 and r.done > 0
    o = order.copy()
    o[-1] = 99                                             # beyond the window, and no step to bring it in
    r = icc.search(S, piv, 8, 8, 4, 0, 3, 4, 1, 1, 3, 0, -1, order=o)
    assert r.keys == [r.keys[0]] * 4 and r.keys[0] != -2 and r.best == r.keys[0]


def test_a_short_order_keeps_its_entries_and_the_window_comes_to_hold_a_pivot():
    """olen = pivot_rows + ell exactly: an exchanged-in column outside the order leaves the order as it is, so the leaving pivot stays in
    the first k entries and a later exchange may bring a window column in as a pivot."""
    rng = np.random.default_rng(9)
    held = 0
    for member in range(12):
        _A, S, piv, order = _state(rng, 8, 24, 1)
        r = icc.search(S, piv, 8, 8, 12, 2, 5, 4, 1, 1, 4, 0, -1, b=member, order=order[:12])
        assert sorted(r.order.tolist()) == sorted(order[:12].tolist()) and r.done > 0
        held += bool(set(r.order[8:12].tolist()) & set(r.pivots.tolist()))
    assert held > 0


def test_no_iteration():
    rng = np.random.default_rng(4)
    _A, S, piv, order = _state(rng, 8, 20, 1)
    r = icc.search(S, piv, 8, 8, 0, 3, 5, 4, 1, 1, 2, 0, -1, order=order)
    assert (r.best, r.best_iter, r.iters_run, r.done, r.W) == (-1, -1, 0, 0, None)


# ---- the plan -----------------------------------------------------------------------------------------------------------------------------

def _pad16(x):
    return (x + 15) // 16 * 16


def _q(ell, n1):
    q = 0
    while q < ell and (1 << q) < n1:
        q += 1
    return q


def _lds_bytes(m, n, k, k1, t1, t2, ell):
    """By the documented layout: path 1's staging of plan_isd_search (the word and an order of ncols entries included) to 16 bytes, then
    k + 1 row keys, N1 sorted keys, 128 bytes of wave minima, 2^q bucket ends, 4096 bytes of scan sums, the window (256 bytes), N1 left
    indices (to 16 bytes), and the kernel's own 256."""
    w = (n + 63) // 64
    ldw = w + ((w & 1) ^ 1)
    n1 = comb(k1, t1)
    staged = m * ldw * 8 + _pad16(m * 4) + ((m + 63) // 64) * 8 + 128 + 128 + 8 * w + 4 * n
    join = (k + 1) * 8 + 8 * n1 + 128 + 4 * (1 << _q(ell, n1)) + 4096 + 256 + 2 * n1
    return _pad16(staged) + _pad16(join) + 256


def _want_plan(m, n, k, k1, t1, t2, ell):
    if k > 1024 or n > 1024 or t1 > 8 or t2 > 8 or ell > 64:
        return 2
    n1, n2 = comb(k1, t1), comb(k - k1, t2)
    if n1 > 8192 or n2 > 1 << 24 or n1 * n2 > 1 << 40:
        return 2
    return 1 if _lds_bytes(m, n, k, k1, t1, t2, ell) <= LDS_BUDGET else 2


def test_plan_boundaries():
    P = PLAN
    assert [P(m, n, min(m, 4), min(m, 4) // 2, 1, 1, 0) for (m, n) in [(0, 0), (1, 1), (64, 64), (65, 64), (64, 65), (512, 1024)]] == [1] * 6      # no wave path
    # the LDS bound, from the documented layout: small table, large table, a window that holds q below ceil(log2 N1)
    for (n, k, k1, t1, t2, ell) in [(1024, 16, 8, 1, 1, 3), (65, 16, 8, 1, 1, 0), (513, 200, 128, 2, 1, 13), (513, 200, 128, 2, 1, 5), (200, 136, 128, 2, 1, 64)]:
        m = max(m for m in range(k, 9000) if _lds_bytes(m, n, k, k1, t1, t2, ell) <= LDS_BUDGET)
        assert (P(m, n, k, k1, t1, t2, ell), P(m + 1, n, k, k1, t1, t2, ell)) == (1, 2), (n, k, k1, t1, t2, ell, m)
    # the bucket bits decide at the edge: q = 13 fits, one row more does not, q = 5 does
    m = max(m for m in range(200, 9000) if _lds_bytes(m, 513, 200, 128, 2, 1, 13) <= LDS_BUDGET)
    assert P(m + 1, 513, 200, 128, 2, 1, 13) == 2 and P(m + 1, 513, 200, 128, 2, 1, 5) == 1
    # the limits
    assert (P(1025, 64, 1024, 4, 1, 1, 2), P(1026, 64, 1025, 4, 1, 1, 2), P(5, 1025, 4, 2, 1, 1, 2)) == (1, 2, 2)
    assert (P(20, 64, 16, 8, 8, 8, 2), P(20, 64, 16, 8, 9, 1, 2), P(20, 64, 16, 8, 1, 9, 2), P(20, 64, 16, 2, 9, 1, 2)) == (1, 2, 2, 2)
    assert (P(20, 64, 16, 8, 1, 1, 64), P(20, 64, 16, 8, 1, 1, 65)) == (1, 2)
    assert comb(128, 2) == 8128 and comb(129, 2) == 8256
    assert (P(137, 200, 136, 128, 2, 1, 10), P(138, 200, 137, 129, 2, 1, 10)) == (1, 2)                   # N1 = 8128 against 8256
    assert (P(9000, 64, 8192, 8192, 1, 0, 3), P(1024, 64, 1024, 1024, 1, 0, 3)) == (2, 1)                 # k first
    k2 = max(k for k in range(3, 1025) if comb(k, 3) <= 1 << 24)
    assert comb(k2 + 1, 3) > 1 << 24 and (P(k2 + 9, 64, k2 + 8, 8, 1, 3, 6), P(k2 + 10, 64, k2 + 9, 8, 1, 3, 6)) == (1, 2)      # N2 at 2^24
    assert comb(33, 8) < 1 << 24 < comb(34, 8) and (P(42, 64, 41, 8, 1, 8, 6), P(43, 64, 42, 8, 1, 8, 6)) == (1, 2)
    assert P(1 << 40, 1 << 40, 4, 2, 1, 1, 0) == 2 and P(1 << 40, 64, 4, 2, 1, 1, 0) == 2 and P(1 << 62, 1 << 62, 1 << 62, 1 << 62, 1 << 62, 1 << 62, 1 << 62) == 2
    rng = np.random.default_rng(1)
    for m, n, t1, t2, ell in rng.integers(0, [1300, 1100, 4, 4, 70], size=(400, 5)).tolist():
        k = int(rng.integers(0, m + 1))
        k1 = int(rng.integers(0, k + 1))
        assert P(m, n, k, k1, t1, t2, ell) == _want_plan(m, n, k, k1, t1, t2, ell), (m, n, k, k1, t1, t2, ell)


def test_plan_negative_sizes():
    P = PLAN
    assert P(-1, 5, 0, 0, 1, 1, 0) == -1 and P(5, -1, 1, 0, 1, 1, 0) == -1 and P(5, 5, -1, 0, 1, 1, 0) == -1 and P(5, 5, 4, -1, 1, 1, 0) == -1
    assert P(5, 5, 4, 2, -1, 1, 0) == -1 and P(5, 5, 4, 2, 1, -1, 0) == -1 and P(5, 5, 4, 2, 1, 1, -1) == -1 and P(5, 5, 4, 5, 1, 1, 0) == -1
    assert P(-1, 1 << 40, 2000, 9, 9, 9, 99) == -1


def test_plan_ignores_the_threads_variable(monkeypatch):
    for v in ("64", "1024", "junk", "-7", "100000"):
        monkeypatch.setenv(THREADS, v)
        assert (PLAN(33, 64, 32, 16, 1, 1, 4), PLAN(2000, 1024, 4, 2, 1, 1, 0), PLAN(64, 64, 64, 32, 9, 1, 0)) == (1, 2, 2), v


# ---- the argument checks ------------------------------------------------------------------------------------------------------------------
# D: 2 members of 5 x 64 (5 words each, 80 bytes in all) at D0, four pivot rows split 2 + 2 and the received word; pivots: 2 x 4 entries
# (32 bytes); rank: 2 entries (8 bytes); order: 2 x 64 entries (512 bytes), the window its entries 4 .. 6; best: 2 entries of 8 bytes;
# best_iter, iters_run, done: 2 entries of 4 bytes each; W: 2 members of one word (16 bytes).  All far from each other, none of it memory:
# the checks return before any HIP call.
AT = dict(D=1 << 20, pivots=1 << 22, rank=1 << 24, order=1 << 26, best=1 << 28, best_iter=1 << 30, iters_run=1 << 32, done=1 << 34, W=1 << 36)
BYTES = dict(D=80, pivots=32, rank=8, order=512, best=16, best_iter=8, iters_run=8, done=8, W=16)
OPERANDS = tuple(AT)


def _call(nrows=5, ncols=64, pivot_rows=4, d_stride=1, d_bs=5, batch=2, iters=6, steps=3, seed=7, k1=2, t1=1, t2=1, ell=3, w_min=1, w_stop=3, o_bs=64, olen=64,
          w_bs=1, **ptrs):
    a = dict(AT, **ptrs)
    return m4ri_amd.lib().m4ri_amd_isd_collide_search_dev(a["D"], d_stride, d_bs, nrows, ncols, pivot_rows, a["pivots"], a["rank"], batch, iters, steps, seed, k1,
                                                          t1, t2, ell, w_min, w_stop, a["order"], o_bs, olen, a["best"], a["best_iter"], a["iters_run"],
                                                          a["done"], a["W"], w_bs, None)


@pytest.mark.parametrize("kw", [
    dict(nrows=-1, pivot_rows=0, k1=0), dict(ncols=-1, olen=0, ell=0), dict(pivot_rows=-1, k1=0), dict(olen=-1), dict(batch=-1), dict(iters=-1), dict(steps=-1),
    dict(w_min=-1), dict(d_stride=-1), dict(d_bs=-1), dict(o_bs=-1), dict(w_bs=-1),                                  # negative
    dict(k1=-1), dict(k1=5), dict(t1=-1), dict(t2=-1), dict(ell=-1), dict(k1=1 << 62),                               # the split and the window
    dict(order=None), dict(olen=6), dict(olen=0, o_bs=0), dict(ell=61), dict(ell=64), dict(pivot_rows=5, ell=60), dict(order=None, ell=1),
    dict(pivot_rows=6), dict(nrows=3), dict(nrows=0), dict(olen=65), dict(ncols=63), dict(ncols=0),                  # pivot_rows > nrows, olen > ncols
    dict(d_stride=0), dict(ncols=65, d_bs=10, w_bs=2), dict(ncols=129, d_stride=2, d_bs=20, w_bs=3),                 # a stride below the width
    dict(d_bs=4), dict(d_bs=0), dict(d_stride=3, d_bs=12),                                                           # overlapping D members
    dict(o_bs=63), dict(o_bs=0), dict(olen=7, o_bs=6),                                                               # orders that overlap
    dict(w_bs=0), dict(ncols=65, d_stride=2, d_bs=10, w_bs=1), dict(ncols=1024, d_stride=16, d_bs=80, w_bs=15),      # words that overlap
    dict(D=None), dict(best=None), dict(pivots=None), dict(rank=None), dict(best=None, iters=0), dict(best=None, nrows=0, pivot_rows=0, k1=0, ell=0),
    dict(D=None, steps=0), dict(pivots=None, iters=2, steps=1), dict(rank=None, iters=2, steps=1),
    dict(D=None, W=None, best_iter=None, iters_run=None, done=None),
])
def test_invalid_arguments(kw):
    """Rejected before any HIP call: the pointers are not device memory (and this machine may have no GPU at all)."""
    assert _call(**kw) == INVALID


def test_a_window_needs_its_order_whatever_the_batch():
    assert _call(order=None, batch=0) == INVALID and _call(olen=6, batch=0) == INVALID and _call(olen=7, o_bs=7, batch=0) == 0
    assert _call(order=None, ell=0, batch=0) == 0 and _call(order=None, ell=0, olen=0, o_bs=0, batch=0) == 0


PAIRS = [(a, b) for i, a in enumerate(OPERANDS) for b in OPERANDS[i + 1:]]


@pytest.mark.parametrize("a,b", PAIRS, ids=[f"{a}-{b}" for a, b in PAIRS])
def test_operands_that_meet(a, b):
    """Any two of the nine operands: b on a's last entry, b's last entry on a's first, and b inside a or a inside b."""
    entry = 8 if b in ("D", "best", "W") else 4
    assert _call(**{b: AT[a] + BYTES[a] - entry}) == INVALID
    assert _call(**{b: AT[a] - BYTES[b] + entry}) == INVALID
    assert _call(**{b: AT[a]}) == INVALID
    entry = 8 if a in ("D", "best", "W") else 4
    assert _call(**{a: AT[b] + BYTES[b] - entry}) == INVALID


@pytest.mark.parametrize("kw", [
    dict(), dict(order=None, ell=0), dict(order=None, o_bs=0, olen=0, ell=0), dict(olen=0, o_bs=0, ell=0), dict(olen=7, o_bs=7), dict(best_iter=None),
    dict(iters_run=None), dict(done=None), dict(W=None), dict(W=None, w_bs=0), dict(best_iter=None, iters_run=None, done=None, W=None), dict(pivot_rows=0, k1=0),
    dict(pivot_rows=5, k1=5), dict(k1=0), dict(k1=4), dict(t1=0), dict(t2=0), dict(t1=0, t2=0), dict(t1=8, t2=8), dict(t1=3), dict(ell=0), dict(ell=60),
    dict(d_stride=3, d_bs=13), dict(ncols=65, olen=65, o_bs=65, d_stride=2, d_bs=10, w_bs=2), dict(iters=0), dict(steps=0),
    dict(iters=0, D=None, pivots=None, rank=None), dict(iters=1, pivots=None, rank=None), dict(steps=0, pivots=None, rank=None),
    dict(nrows=0, pivot_rows=0, k1=0, D=None, pivots=None, rank=None), dict(ncols=0, olen=0, ell=0, D=None, pivots=None, rank=None, order=None),
    dict(w_stop=-1), dict(w_stop=-(1 << 62)), dict(w_stop=1 << 62), dict(w_min=1 << 62), dict(iters=(1 << 31) - 1, steps=1), dict(iters=2, steps=(1 << 31) - 1),
    dict(iters=1, steps=1 << 62), dict(nrows=1024, ncols=1024, pivot_rows=1024, k1=8, d_stride=16, d_bs=1 << 16, olen=0, ell=0, w_bs=16),
    dict(nrows=137, ncols=200, pivot_rows=136, k1=128, t1=2, t2=1, ell=64, d_stride=4, d_bs=1 << 10, olen=200, o_bs=200, w_bs=4),
])
def test_batch_zero_is_success(kw):
    """Legal sizes, strides and absent operands, shown with batch = 0, which returns before any HIP call.  The accepted neighbours of the
    refusals above need members: tests/test_gpu_isd_collide_search.py runs absent operands and operands packed back to back."""
    assert _call(**dict(kw, batch=0)) == 0


@pytest.mark.parametrize("kw", [
    dict(nrows=1025, pivot_rows=1025, ell=0, d_bs=1 << 20), dict(ncols=1025, d_stride=17, d_bs=1 << 20, w_bs=17), dict(t1=9), dict(t2=9), dict(t1=1 << 62),
    dict(t2=1 << 62), dict(ell=65, ncols=128, d_stride=2, d_bs=10, olen=128, o_bs=128, w_bs=2),                          # ell > 64 with an order that holds it
    dict(nrows=138, pivot_rows=137, k1=129, t1=2, ell=0, d_bs=1 << 20),                                                        # N1 = 8256
    dict(nrows=1025, pivot_rows=1024, k1=8, t2=3, ell=0, d_bs=1 << 20), dict(nrows=64, pivot_rows=64, k1=8, t2=8, ell=0, d_bs=64),    # N2 > 2^24
    dict(nrows=2000, ncols=1024, d_stride=16, d_bs=1 << 20, olen=1024, o_bs=1024, w_bs=16), dict(nrows=1 << 40, d_bs=1 << 50),      # beyond LDS
    dict(nrows=1025, ncols=1024, pivot_rows=1024, k1=128, t1=2, ell=0, d_stride=16, d_bs=1 << 20, olen=1024, o_bs=1024, w_bs=16),        # the member and the table
    dict(iters=1 << 31), dict(iters=1 << 62), dict(iters=3, steps=1 << 30), dict(iters=1 << 20, steps=1 << 20), dict(iters=2, steps=1 << 31),   # 32-bit counts
    dict(iters=(1 << 63) - 1, steps=(1 << 63) - 1),
])
@pytest.mark.parametrize("batch", [0, 2])
def test_beyond_the_limits_is_not_supported(kw, batch):
    assert _call(**dict(kw, batch=batch)) == NOT_SUPPORTED


def test_sizes_and_strides_are_checked_before_the_limits():
    big = dict(nrows=1025, pivot_rows=1025, ell=0, d_bs=1 << 20)
    assert _call(**big) == NOT_SUPPORTED
    assert _call(**dict(big, d_stride=0)) == INVALID and _call(**dict(big, batch=-1)) == INVALID and _call(**dict(big, pivot_rows=1026)) == INVALID
    assert _call(**dict(big, iters=-1)) == INVALID and _call(t1=9, w_min=-1) == INVALID and _call(t1=9, olen=65) == INVALID
    assert _call(t1=9, order=None) == INVALID and _call(t1=9, k1=5) == INVALID and _call(ell=65) == INVALID          # olen = 64 < 4 + 65
    assert _call(t1=9, d_bs=4) == NOT_SUPPORTED and _call(t1=9, best=None) == NOT_SUPPORTED          # the members' fit and the pointers come after


def test_the_threads_variable_cannot_lift_a_limit(monkeypatch):
    for v in ("junk", "-99999999999999999999", "64", "1024"):
        monkeypatch.setenv(THREADS, v)
        assert _call(batch=0) == 0 and _call(t1=9, batch=0) == NOT_SUPPORTED
        assert _call(nrows=2000, ncols=1024, d_stride=16, d_bs=1 << 20, olen=1024, o_bs=1024, w_bs=16, batch=0) == NOT_SUPPORTED


def test_python_wrappers_are_bound():
    a = AT
    with pytest.raises(RuntimeError):
        SEARCH(a["D"], 1, 5, 5, 64, 4, a["pivots"], a["rank"], 2, 6, 3, 7, 2, 1, 1, 0, 1, 3, 0)                           # no best
    with pytest.raises(RuntimeError):
        SEARCH(a["D"], 1, 5, 5, 64, 4, a["pivots"], a["rank"], 2, 6, 3, 7, 2, 1, 1, 0, 1, 3, a["best"], done=a["rank"] + 4)
    with pytest.raises(RuntimeError):
        SEARCH(a["D"], 1, 5, 5, 64, 4, a["pivots"], a["rank"], 0, 6, 3, 7, 2, 1, 1, 3, 1, 3, a["best"])                   # a window without its order
    with pytest.raises(RuntimeError, match="801"):
        SEARCH(a["D"], 1, 5, 5, 64, 4, a["pivots"], a["rank"], 2, 6, 3, 7, 2, 9, 1, 0, 1, 3, a["best"])
    SEARCH(a["D"], 1, 5, 5, 64, 4, a["pivots"], a["rank"], 0, 6, 3, -1, 2, 1, 1, 3, 1, -1, a["best"], a["order"], 64, 64, a["best_iter"], a["iters_run"],
           a["done"], a["W"], 1, stream=0)                                                                                 # batch = 0; any 64-bit seed
    SEARCH(a["D"], 1, 5, 5, 64, 4, 0, 0, 0, 1, 0, 0, 0, 0, 0, 0, 0, -1, a["best"])
    assert PLAN(5, 64, 4, 2, 1, 1, 3) == 1 and PLAN(5, 64, 4, 5, 1, 1, 3) == -1
    assert m4ri_amd.isd_iteration_seed(7, 3) == ic.iteration_seed(7, 3)
