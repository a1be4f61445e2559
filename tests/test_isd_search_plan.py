"""The host side of m4ri_amd_isd_search_dev, without a GPU: the NumPy rule of tests/isd_cases.py against the two rules it composes
(tests/exchange_cases.py, tests/rowsums_cases.py) and against the elimination from scratch, m4ri_amd.isd_iteration_seed, the path
boundaries of m4ri_amd_plan_isd_search and the argument checks (which run before any HIP call; the expected codes are written here by
hand from the header).  tests/test_gpu_isd_search.py judges the kernels with the same rule."""
from math import comb

import numpy as np
import pytest

import exchange_cases as xc
import isd_cases as ic
import m4ri_amd
import order_cases as oc
import rowsums_cases as rc

INVALID, NOT_SUPPORTED = 1, 801      # hipErrorInvalidValue, hipErrorNotSupported
PATH0 = "M4RI_AMD_ISD_SEARCH_PATH0_MAX"
LDS_BUDGET = 160 * 1024              # batch_common.h's BATCH_LDS_BUDGET
SEARCH, PLAN = m4ri_amd.isd_search_dev, m4ri_amd.plan_isd_search     # what this module is about: without the call none of it holds


def _state(rng, k, n, followers):
    """A full-rank k x n generator over `followers` more rows in reduced form on a random order: (as it was, the form, pivots, order)."""
    while True:
        A = rng.integers(0, 2, size=(k + followers, n), dtype=np.uint8)
        order = rng.permutation(n).astype(np.int32)
        S, rank, piv = oc.ech_order(A, order, 1, k)
        if rank == k:
            return A, S, piv, order


# ---- the rule -----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k,n,followers,t", [(1, 2, 0, 1), (4, 9, 1, 0), (8, 20, 1, 2), (8, 20, 2, 3), (12, 30, 0, 4), (16, 70, 1, 1)])
def test_one_iteration_is_the_enumeration(k, n, followers, t):
    rng = np.random.default_rng(10 * k + t)
    _A, S, piv, order = _state(rng, k, n, followers)
    for w_min in (0, 1, n + 1):
        r = ic.search(S, piv, k, k, 1, 3, 5, t, w_min, -1, order=order)
        want = rc.expect(S[:k], S[k] if followers else None, t, w_min)[1]
        assert r.best == want and r.keys == [want] and r.iters_run == 1 and r.done == 0 and r.best_iter == (0 if want >= 0 else -1)
        assert np.array_equal(r.bits, S) and np.array_equal(r.pivots, piv) and np.array_equal(r.order, order)
        if want >= 0:
            assert int(r.W.sum()) == want >> 40 and np.array_equal(r.W, ic.word_of(S, k, want, t))
        else:
            assert r.W is None


def test_the_word_of_a_key():
    rng = np.random.default_rng(3)
    _A, S, piv, _o = _state(rng, 8, 20, 1)
    key = (5 << 40) | rc.rank((1, 4, 6))
    assert np.array_equal(ic.word_of(S, 8, key, 3), S[8] ^ S[1] ^ S[4] ^ S[6])
    assert np.array_equal(ic.word_of(S[:8], 8, key, 3), S[1] ^ S[4] ^ S[6])     # no follower: the zero word
    assert np.array_equal(ic.word_of(S, 8, 7 << 40, 0), S[8])


def test_no_steps_means_iteration_zero():
    rng = np.random.default_rng(4)
    _A, S, piv, order = _state(rng, 8, 20, 1)
    key = rc.expect(S[:8], S[8], 2, 0)[1]
    r = ic.search(S, piv, 8, 8, 7, 0, 5, 2, 0, -1, order=order)
    assert (r.best, r.best_iter, r.iters_run, r.done) == (key, 0, 7, 0) and np.array_equal(r.bits, S)
    r = ic.search(S, piv, 8, 8, 7, 0, 5, 2, 0, key >> 40, order=order)             # stops at once
    assert (r.best, r.best_iter, r.iters_run, r.done) == (key, 0, 1, 0)
    r = ic.search(S, piv, 8, 8, 7, 0, 5, 2, 0, (key >> 40) - 1, order=order) if key >> 40 else r
    assert r.iters_run == (7 if key >> 40 else 1)
    r = ic.search(S, piv, 8, 8, 0, 3, 5, 2, 0, -1)                                   # no iteration at all
    assert (r.best, r.best_iter, r.iters_run, r.done, r.W) == (-1, -1, 0, 0, None)


@pytest.mark.parametrize("k,n,followers,t,steps", [(3, 9, 1, 1, 1), (8, 20, 2, 2, 3), (16, 64, 1, 1, 1), (20, 70, 1, 2, 2)])
def test_the_loop_is_the_composition(k, n, followers, t, steps):
    """The loop against its two parts called one after the other by hand, and on these full-rank members the final form against
    ech_order from scratch on the final pivots."""
    rng = np.random.default_rng(100 * k + n)
    for member in range(6):
        A, S, piv, order = _state(rng, k, n, followers)
        iters, seed = 9, 1000 + member
        r = ic.search(S, piv, k, k, iters, steps, seed, t, 1, -1, b=member, order=order)
        cur, cp, co, keys, done = S, piv, order, [], 0
        for it in range(iters):
            if it:
                cur, cp, co, did, _ = xc.exchange(cur, cp, k, k, steps, seed=oc.splitmix(seed, it), b=member, order=co)
                done += did
            keys.append(rc.expect(cur[:k], cur[k], t, 1)[1])
        assert r.keys == keys and r.done == done and done > 0 and r.iters_run == iters
        assert np.array_equal(r.bits, cur) and np.array_equal(r.pivots, cp) and np.array_equal(r.order, co)
        weights = [key >> 40 for key in keys]
        assert r.best_iter == weights.index(min(weights)) and r.best == keys[r.best_iter]            # the earliest among equal weights
        want, rank, piv3 = oc.ech_order(A, r.pivots, 1, k)
        assert rank == k and np.array_equal(piv3, r.pivots) and np.array_equal(r.bits, want)
        # the stop: at the first iteration whose running minimum is low enough
        w_stop = sorted(weights)[len(weights) // 2]
        first = next(i for i, w in enumerate(weights) if w <= w_stop)
        s = ic.search(S, piv, k, k, iters, steps, seed, t, 1, w_stop, b=member, order=order)
        assert s.iters_run == first + 1 and s.best == keys[first] and s.best_iter == first and s.keys == keys[:first + 1]


def test_a_refused_member_is_still_enumerated():
    rng = np.random.default_rng(6)
    A = rng.integers(0, 2, size=(9, 20), dtype=np.uint8)
    r = ic.search(A, np.full(8, -1, dtype=np.int32), -1, 8, 5, 3, 7, 2, 0, -1)
    assert r.done == 0 and r.iters_run == 5 and r.best == rc.expect(A[:8], A[8], 2, 0)[1] and r.best_iter == 0 and np.array_equal(r.bits, A)


def test_iteration_seed_is_the_stream():
    for seed, it in [(0, 0), (7, 1), (7, 39), ((1 << 64) - 1, 5), (-3 & ((1 << 64) - 1), 1 << 31)]:
        assert m4ri_amd.isd_iteration_seed(seed, it) == oc.splitmix(seed, it) == ic.iteration_seed(seed, it)
    assert m4ri_amd.isd_iteration_seed(7, 0) == 0x63cbe1e459320dd7                      # the stream of m4ri_amd_fill_dev
    assert m4ri_amd.isd_iteration_seed(-3, 2) == oc.splitmix(-3 & ((1 << 64) - 1), 2)     # any 64-bit seed
    r, start = m4ri_amd.exchange_draw(m4ri_amd.isd_iteration_seed(7, 3), 4, 2, 1, 8, 30)
    assert (r, start) == xc.draw(oc.splitmix(7, 3), 4, 2, 1, 8, 30)
    with pytest.raises(ValueError):
        m4ri_amd.isd_iteration_seed(7, -1)


# ---- the plan -----------------------------------------------------------------------------------------------------------------------------

def _lds_bytes(m, n):
    """Path 1's LDS by the documented layout: rows at an odd pitch, the row index, one flag buffer, 128 bytes of slots, 128 bytes of key
    slots, the word, an order of ncols entries."""
    w = (n + 63) // 64
    ldw = w + ((w & 1) ^ 1)
    return m * ldw * 8 + (m * 4 + 15) // 16 * 16 + ((m + 63) // 64) * 8 + 128 + 128 + 8 * w + 4 * n


def _want_path(m, n, k, t):
    if k > 1024 or n > 1024 or t > 8 or comb(k, t) > 1 << 24:
        return 2
    if m <= 64 and n <= 64:
        return 0
    return 1 if _lds_bytes(m, n) <= LDS_BUDGET else 2


def test_path_boundaries():
    P = m4ri_amd.plan_isd_search
    assert [P(m, n, min(m, 4), 2) for (m, n) in [(0, 0), (1, 1), (64, 64), (65, 1), (1, 65), (65, 64), (64, 65), (65, 65), (64, 1024), (512, 1024)]] \
        == [0, 0, 0, 1, 1, 1, 1, 1, 1, 1]
    assert P(64, 64, 64, 3) == 0 and P(65, 64, 64, 3) == 1
    # the LDS bound, from the documented layout
    m = max(m for m in range(1, 3000) if _lds_bytes(m, 1024) <= LDS_BUDGET)
    assert m > 1024 and (P(m, 1024, 1024, 2), P(m + 1, 1024, 1024, 2)) == (1, 2)
    m = max(m for m in range(1, 20000) if _lds_bytes(m, 65) <= LDS_BUDGET)
    assert (P(m, 65, 16, 2), P(m + 1, 65, 16, 2)) == (1, 2)
    m = max(m for m in range(1, 3000) if _lds_bytes(m, 513) <= LDS_BUDGET)              # nine words: an odd width keeps its pitch
    assert (P(m, 513, 16, 2), P(m + 1, 513, 16, 2)) == (1, 2) and _lds_bytes(1024, 1024) <= LDS_BUDGET
    # the limits of the enumeration
    assert (P(1024, 1024, 1024, 1), P(1025, 1024, 1025, 1), P(1024, 1025, 1024, 1), P(1025, 64, 1024, 1)) == (1, 2, 2, 1)
    assert (P(20, 64, 16, 8), P(20, 64, 16, 9), P(20, 64, 8, 9)) == (0, 2, 2)           # t > 8 even where there are no sums
    assert (P(1024, 64, 1024, 2), P(1024, 64, 1024, 3)) == (1, 2)                      # C(1024, 2) = 523 776, C(1024, 3) > 2^24
    for t in (3, 4, 8):
        k = max(k for k in range(t, 1025) if comb(k, t) <= 1 << 24)
        assert comb(k + 1, t) > 1 << 24 and (P(k + 1, 64, k, t), P(k + 2, 64, k + 1, t)) == (1 if k + 1 > 64 else 0, 2), (t, k)
    assert comb(26, 8) < 1 << 24 < comb(64, 8) and P(30, 64, 26, 8) == 0 and P(64, 64, 64, 8) == 2
    assert P(1 << 40, 1 << 40, 4, 2) == 2 and P(0, 1 << 40, 0, 0) == 2 and P(1 << 40, 64, 4, 0) == 2 and P(1 << 62, 1 << 62, 1 << 62, 1 << 62) == 2
    rng = np.random.default_rng(1)
    for m, n, t in rng.integers(0, [1300, 1100, 10], size=(400, 3)).tolist():
        k = int(rng.integers(0, m + 1))
        assert P(m, n, k, t) == _want_path(m, n, k, t), (m, n, k, t)


def test_negative_sizes():
    P = m4ri_amd.plan_isd_search
    assert P(-1, 5, 0, 1) == -1 and P(5, -1, 1, 1) == -1 and P(5, 5, -1, 1) == -1 and P(5, 5, 1, -1) == -1 and P(-1, 1 << 40, 2000, 9) == -1


def test_plan_ignores_the_override_variable(monkeypatch):
    P = m4ri_amd.plan_isd_search
    for v in ("0", "1", "63", "64", "100000", "junk", "-7"):
        monkeypatch.setenv(PATH0, v)
        assert (P(1, 1, 1, 1), P(64, 64, 63, 2), P(65, 65, 64, 2), P(2000, 1024, 4, 2), P(64, 64, 64, 9)) == (0, 0, 1, 2, 2), v


# ---- the argument checks ------------------------------------------------------------------------------------------------------------------
# D: 2 members of 5 x 64 (5 words each, 80 bytes in all) at D0, four pivot rows and the received word; pivots: 2 x 4 entries (32 bytes);
# rank: 2 entries (8 bytes); order: 2 x 64 entries (512 bytes); best: 2 entries of 8 bytes; best_iter, iters_run, done: 2 entries of 4
# bytes each; W: 2 members of one word (16 bytes).  All far from each other, none of it memory: the checks return before any HIP call.
AT = dict(D=1 << 20, pivots=1 << 22, rank=1 << 24, order=1 << 26, best=1 << 28, best_iter=1 << 30, iters_run=1 << 32, done=1 << 34, W=1 << 36)
BYTES = dict(D=80, pivots=32, rank=8, order=512, best=16, best_iter=8, iters_run=8, done=8, W=16)
OPERANDS = tuple(AT)


def _call(nrows=5, ncols=64, pivot_rows=4, d_stride=1, d_bs=5, batch=2, iters=6, steps=3, seed=7, t=2, w_min=1, w_stop=3, o_bs=64, olen=64, w_bs=1, **ptrs):
    a = dict(AT, **ptrs)
    return m4ri_amd.lib().m4ri_amd_isd_search_dev(a["D"], d_stride, d_bs, nrows, ncols, pivot_rows, a["pivots"], a["rank"], batch, iters, steps, seed, t, w_min,
                                                  w_stop, a["order"], o_bs, olen, a["best"], a["best_iter"], a["iters_run"], a["done"], a["W"], w_bs, None)


@pytest.mark.parametrize("kw", [
    dict(nrows=-1, pivot_rows=0), dict(ncols=-1, olen=0), dict(pivot_rows=-1), dict(olen=-1), dict(batch=-1), dict(iters=-1), dict(steps=-1), dict(t=-1),
    dict(w_min=-1), dict(d_stride=-1), dict(d_bs=-1), dict(o_bs=-1), dict(w_bs=-1),                                  # negative
    dict(pivot_rows=6), dict(nrows=3), dict(nrows=0), dict(olen=65), dict(ncols=63), dict(ncols=0),                  # pivot_rows > nrows, olen > ncols
    dict(d_stride=0), dict(ncols=65, d_bs=10, w_bs=2), dict(ncols=129, d_stride=2, d_bs=20, w_bs=3),                 # a stride below the width
    dict(d_bs=4), dict(d_bs=0), dict(d_stride=3, d_bs=12),                                                           # overlapping D members
    dict(o_bs=63), dict(o_bs=0), dict(olen=7, o_bs=6),                                                               # orders that overlap
    dict(w_bs=0), dict(ncols=65, d_stride=2, d_bs=10, w_bs=1), dict(ncols=1024, d_stride=16, d_bs=80, w_bs=15),      # words that overlap
    dict(D=None), dict(best=None), dict(pivots=None), dict(rank=None), dict(best=None, iters=0), dict(best=None, nrows=0, pivot_rows=0),
    dict(D=None, steps=0), dict(pivots=None, iters=2, steps=1), dict(rank=None, iters=2, steps=1),
    dict(D=None, W=None, order=None, best_iter=None, iters_run=None, done=None),
])
def test_invalid_arguments(kw):
    """Rejected before any HIP call: the pointers are not device memory (and this machine may have no GPU at all)."""
    assert _call(**kw) == INVALID


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
    dict(), dict(order=None), dict(order=None, o_bs=0, olen=0), dict(olen=0, o_bs=0), dict(olen=7, o_bs=7), dict(best_iter=None), dict(iters_run=None),
    dict(done=None), dict(W=None), dict(W=None, w_bs=0), dict(best_iter=None, iters_run=None, done=None, W=None, order=None), dict(pivot_rows=0),
    dict(pivot_rows=5), dict(d_stride=3, d_bs=13), dict(ncols=65, olen=65, o_bs=65, d_stride=2, d_bs=10, w_bs=2), dict(iters=0), dict(steps=0),
    dict(iters=0, D=None, pivots=None, rank=None), dict(iters=1, pivots=None, rank=None), dict(steps=0, pivots=None, rank=None),
    dict(nrows=0, pivot_rows=0, D=None, pivots=None, rank=None), dict(ncols=0, olen=0, D=None, pivots=None, rank=None, order=None), dict(t=0), dict(t=8),
    dict(w_stop=-1), dict(w_stop=-(1 << 62)), dict(w_stop=1 << 62), dict(w_min=1 << 62), dict(iters=(1 << 31) - 1, steps=1), dict(iters=2, steps=(1 << 31) - 1),
    dict(iters=1, steps=1 << 62), dict(nrows=1024, ncols=1024, pivot_rows=1024, d_stride=16, d_bs=1 << 16, olen=0, w_bs=16),
])
def test_batch_zero_is_success(kw):
    """Legal sizes, strides and absent operands, shown with batch = 0, which returns before any HIP call.  The accepted neighbours of the
    refusals above need members: tests/test_gpu_isd_search.py runs absent operands and operands packed back to back."""
    assert _call(**dict(kw, batch=0)) == 0


@pytest.mark.parametrize("kw", [
    dict(nrows=1025, pivot_rows=1025, d_bs=1 << 20), dict(ncols=1025, d_stride=17, d_bs=1 << 20, w_bs=17), dict(t=9), dict(t=1 << 62),
    dict(nrows=1025, pivot_rows=1024, d_bs=1 << 20, t=3), dict(nrows=64, pivot_rows=64, d_bs=64, t=8),                  # C(k, t) > 2^24
    dict(nrows=2000, ncols=1024, d_stride=16, d_bs=1 << 20, w_bs=16), dict(nrows=1 << 40, d_bs=1 << 50),                # beyond path 1
    dict(iters=1 << 31), dict(iters=1 << 62), dict(iters=3, steps=1 << 30), dict(iters=1 << 20, steps=1 << 20), dict(iters=2, steps=1 << 31),   # 32-bit counts
    dict(iters=(1 << 63) - 1, steps=(1 << 63) - 1),
])
@pytest.mark.parametrize("batch", [0, 2])
def test_beyond_the_limits_is_not_supported(kw, batch):
    assert _call(**dict(dict(order=None, o_bs=0, olen=0), **kw, batch=batch)) == NOT_SUPPORTED


def test_sizes_and_strides_are_checked_before_the_limits():
    big = dict(nrows=1025, pivot_rows=1025, d_bs=1 << 20)
    assert _call(**big) == NOT_SUPPORTED
    assert _call(**dict(big, d_stride=0)) == INVALID and _call(**dict(big, batch=-1)) == INVALID and _call(**dict(big, pivot_rows=1026)) == INVALID
    assert _call(**dict(big, iters=-1)) == INVALID and _call(t=9, w_min=-1) == INVALID and _call(t=9, olen=65) == INVALID
    assert _call(t=9, d_bs=4) == NOT_SUPPORTED and _call(t=9, best=None) == NOT_SUPPORTED          # the members' fit and the pointers come after


def test_the_override_cannot_lift_a_limit(monkeypatch):
    monkeypatch.setenv(PATH0, "junk")
    assert _call(batch=0) == 0 and _call(t=9, batch=0) == NOT_SUPPORTED
    monkeypatch.setenv(PATH0, "-99999999999999999999")
    assert _call(batch=0) == 0 and _call(nrows=2000, ncols=1024, d_stride=16, d_bs=1 << 20, w_bs=16, batch=0) == NOT_SUPPORTED


def test_python_wrappers_are_bound():
    a = AT
    with pytest.raises(RuntimeError):
        m4ri_amd.isd_search_dev(a["D"], 1, 5, 5, 64, 4, a["pivots"], a["rank"], 2, 6, 3, 7, 2, 1, 3, 0)                     # no best
    with pytest.raises(RuntimeError):
        m4ri_amd.isd_search_dev(a["D"], 1, 5, 5, 64, 4, a["pivots"], a["rank"], 2, 6, 3, 7, 2, 1, 3, a["best"], done=a["rank"] + 4)
    with pytest.raises(RuntimeError, match="801"):
        m4ri_amd.isd_search_dev(a["D"], 1, 5, 5, 64, 4, a["pivots"], a["rank"], 2, 6, 3, 7, 9, 1, 3, a["best"])
    m4ri_amd.isd_search_dev(a["D"], 1, 5, 5, 64, 4, a["pivots"], a["rank"], 0, 6, 3, -1, 2, 1, -1, a["best"], a["order"], 64, 64, a["best_iter"],
                            a["iters_run"], a["done"], a["W"], 1, stream=0)                                                  # batch = 0; any 64-bit seed
    m4ri_amd.isd_search_dev(a["D"], 1, 5, 5, 64, 4, 0, 0, 0, 1, 0, 0, 0, 0, -1, a["best"])
    assert m4ri_amd.plan_isd_search(5, 64, 4, 2) == 0
