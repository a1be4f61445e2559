"""The host side of m4ri_amd_pivot_exchange_batch_dev, without a GPU: the NumPy rule of tests/exchange_cases.py against
tests/order_cases.py's ech_order from scratch on the new pivots and against its own invariants, the random requests of
m4ri_amd.exchange_draw, the path boundaries of m4ri_amd_plan_pivot_exchange_batch and the argument checks (which run before any HIP
call).  tests/test_gpu_pivot_exchange_batch.py judges the kernels with the same rule."""
import numpy as np
import pytest

import exchange_cases as xc
import m4ri_amd
import order_cases as oc

HIP_ERROR_INVALID_VALUE, HIP_ERROR_NOT_SUPPORTED = 1, 801
PATH0, PATH1 = "M4RI_AMD_PIVOT_EXCHANGE_PATH0_MAX", "M4RI_AMD_PIVOT_EXCHANGE_PATH1_MAX"
LDS_BUDGET, CAP_WORDS = 160 * 1024, 512 * 1024 // 8   # batch_common.h's BATCH_LDS_BUDGET and BATCH_CAP_BYTES


def full_rank_state(rng, k, n, followers):
    """A random k x n generator over `followers` more rows, in reduced form on a random order: (the stacked bits as they were, the form,
    pivots, order), full rank (drawn again until it is)."""
    while True:
        A = rng.integers(0, 2, size=(k + followers, n), dtype=np.uint8)
        order = rng.permutation(n).astype(np.int32)
        S, rank, piv = oc.ech_order(A, order, 1, k)
        if rank == k:
            return A, S, piv, order


# ---- the rule against the elimination from scratch ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("k,n,followers", [(1, 2, 0), (3, 9, 1), (8, 20, 2), (16, 64, 1), (20, 70, 3), (33, 130, 1)])
def test_exchanges_give_the_form_from_scratch_on_the_new_pivots(k, n, followers):
    """Sixty members per shape, 360 in all: random requests and requests from a list, invalid ones among them; the result is
    ech_order(the matrix as it was, order = the new pivots, full = 1), followers included, and its pivots are the new pivots."""
    rng = np.random.default_rng(100 * k + n)
    performed = 0
    for member in range(60):
        A, S, piv, order = full_rank_state(rng, k, n, followers)
        steps = int(rng.integers(1, 2 * k + 2))
        if member % 2:
            req = np.stack([rng.integers(-1, k + 1, size=steps), rng.integers(-1, n + 1, size=steps)], axis=1)
            S2, piv2, order2, done, met = xc.exchange(S, piv, k, k, steps, req=req, order=order)
        else:
            S2, piv2, order2, done, met = xc.exchange(S, piv, k, k, steps, seed=member, b=member, order=order)
        performed += done
        want, rank, piv3 = oc.ech_order(A, piv2, 1, k)
        assert rank == k and np.array_equal(piv3, piv2) and np.array_equal(S2, want), (member, done)
        assert np.array_equal(S2[:k][:, piv2], np.eye(k, dtype=np.uint8)) and not S2[k:][:, piv2].any()
        where, where2 = np.flatnonzero(np.isin(order, piv)), np.flatnonzero(np.isin(order2, piv2))
        assert sorted(order2.tolist()) == list(range(n)) and np.array_equal(where, where2)    # the pivots stand where pivots stood
    assert performed >= 15       # exchanges did happen (at 1 x 2 every other row holds one bit only)


def test_the_order_keeps_the_information_set_in_front():
    rng = np.random.default_rng(5)
    while True:   # a form whose order has k independent columns in front: its first k entries are the pivots
        A, S, piv, order = full_rank_state(rng, 10, 40, 1)
        if set(order[:10].tolist()) == set(piv.tolist()):
            break
    S2, piv2, order2, done, _ = xc.exchange(S, piv, 10, 10, 25, seed=3, order=order)
    assert done == 25 and set(order2[:10].tolist()) == set(piv2.tolist()) and set(piv2.tolist()) != set(piv.tolist())
    assert not S2[:, order2[:10]][10:].any()                    # cols = order + k: no information column among them


@pytest.mark.parametrize("k,n", [(1, 2), (5, 64), (16, 70), (33, 130)])
def test_involution(k, n):
    """(r, c) followed by (r, old) restores bits, pivots and order."""
    rng = np.random.default_rng(k + n)
    for _ in range(20):
        A, S, piv, order = full_rank_state(rng, k, n, 1)
        r = int(rng.integers(0, k))
        c = xc.scan(S[r], int(piv[r]), int(rng.integers(0, n)))
        if c is None:
            continue
        S1, piv1, order1, done, _ = xc.exchange(S, piv, k, k, 1, req=[(r, c)], order=order)
        assert done == 1 and piv1[r] == c and not np.array_equal(piv1, piv)
        S2, piv2, order2, done, _ = xc.exchange(S1, piv1, k, k, 1, req=[(r, int(piv[r]))], order=order1)
        assert done == 1 and np.array_equal(S2, S) and np.array_equal(piv2, piv) and np.array_equal(order2, order)
        S3, piv3, order3, done, _ = xc.exchange(S, piv, k, k, 2, req=[(r, c), (r, int(piv[r]))], order=order)
        assert done == 2 and np.array_equal(S3, S) and np.array_equal(piv3, piv) and np.array_equal(order3, order)


def test_invalid_requests_are_skipped():
    rng = np.random.default_rng(11)
    A, S, piv, order = full_rank_state(rng, 6, 20, 1)
    clear = next(c for c in range(20) if not S[2, c])
    for (r, c) in [(-1, 3), (6, 3), (7, 3), (2, -1), (2, 20), (2, clear), (2, int(piv[2])), (2, int(piv[3])), (-(1 << 31), (1 << 31) - 1)]:
        S2, piv2, order2, done, _ = xc.exchange(S, piv, 6, 6, 1, req=[(r, c)], order=order)
        assert done == 0 and np.array_equal(S2, S) and np.array_equal(piv2, piv) and np.array_equal(order2, order), (r, c)
    # a rank below pivot_rows: rows from the rank on are no pivot rows; a refused member's rank -1 reads as 0
    assert xc.exchange(S, piv, 2, 6, 1, req=[(2, xc.scan(S[2], int(piv[2]), 0))])[3] == 0
    assert xc.exchange(S, piv, -1, 6, 3, seed=1)[3] == 0 and xc.exchange(S, piv, -1, 6, 3, seed=1)[4] == [None] * 3


def test_order_variants():
    rng = np.random.default_rng(12)
    A, S, piv, order = full_rank_state(rng, 6, 20, 0)
    r = 1
    c = xc.scan(S[r], int(piv[r]), 0)
    old = int(piv[r])
    assert xc.exchange(S, piv, 6, 6, 1, req=[(r, c)])[2] is None
    absent = order[order != c]                                                    # one value absent: unchanged
    assert np.array_equal(xc.exchange(S, piv, 6, 6, 1, req=[(r, c)], order=absent)[2], absent)
    twice = np.concatenate([order, order])                                        # present twice: the first positions
    got = xc.exchange(S, piv, 6, 6, 1, req=[(r, c)], order=twice)[2]
    p, q = int(np.flatnonzero(order == old)[0]), int(np.flatnonzero(order == c)[0])
    want = twice.copy()
    want[p], want[q] = c, old
    assert np.array_equal(got, want) and got[20 + p] == old and got[20 + q] == c
    wild = np.array([1 << 30, -(1 << 31), old, -5, c, (1 << 31) - 1], dtype=np.int32)   # entries are only compared
    assert xc.exchange(S, piv, 6, 6, 1, req=[(r, c)], order=wild)[2].tolist() == [1 << 30, -(1 << 31), c, -5, old, (1 << 31) - 1]


# ---- the random requests ------------------------------------------------------------------------------------------------------------------

def test_exchange_draw_is_the_rule():
    for (seed, b, steps, s, R, n) in [(0, 0, 1, 0, 1, 1), (7, 0, 3, 1, 5, 64), (7, 3, 16, 15, 33, 130), ((1 << 64) - 1, 1000, 7, 6, 64, 4096),
                                      (-3 & ((1 << 64) - 1), 5, 2, 0, 1, 2)]:
        h = oc.splitmix(seed, b * steps + s)
        assert m4ri_amd.exchange_draw(seed, b, steps, s, R, n) == xc.draw(seed, b, steps, s, R, n) == ((h >> 32) % R, (h & 0xFFFFFFFF) % n)
    assert m4ri_amd.exchange_draw(7, 0, 1, 0, 5, 64) == ((0x63cbe1e459320dd7 >> 32) % 5, 0x59320dd7 % 64)   # the stream of m4ri_amd_fill_dev
    for bad in [(7, 0, 3, 3, 5, 64), (7, 0, 3, -1, 5, 64), (7, 0, 3, 0, 0, 64), (7, 0, 3, 0, 5, 0), (7, -1, 3, 0, 5, 64)]:
        with pytest.raises(ValueError):
            m4ri_amd.exchange_draw(*bad)


def test_the_requests_met_are_the_draws_scanned():
    rng = np.random.default_rng(13)
    A, S, piv, order = full_rank_state(rng, 8, 30, 0)
    _, _, _, done, met = xc.exchange(S, piv, 8, 8, 1, seed=21, b=4)
    r, start = m4ri_amd.exchange_draw(21, 4, 1, 0, 8, 30)
    assert met == [(r, xc.scan(S[r], int(piv[r]), start))] and done == 1
    row = np.zeros(30, dtype=np.uint8)
    row[[3, 17]] = 1
    assert [xc.scan(row, 3, s) for s in (0, 4, 17, 18, 29)] == [17] * 5 and xc.scan(row, 17, 18) == 3    # past column ncols - 1 and round
    row[17] = 0
    assert xc.scan(row, 3, 0) is None                       # a row holding only its own pivot bit


# ---- the plan -----------------------------------------------------------------------------------------------------------------------------

def _lds_bytes(m, n):
    w = (n + 63) // 64
    ldw = w + ((w & 1) ^ 1)
    return m * ldw * 8 + (m * 4 + 15) // 16 * 16 + ((m + 63) // 64) * 8 + 128 + 4 * n


def _want_path(m, n, steps):
    w = (n + 63) // 64
    if m <= 64 and n <= 64:
        return 0
    if m > CAP_WORDS or w > CAP_WORDS or m * w > CAP_WORDS:
        return 3
    return 1 if _lds_bytes(m, n) <= LDS_BUDGET and steps != 1 else 2      # one step: in place even where the member fits


@pytest.mark.parametrize("steps", [0, 2, 4, 16, 1 << 40])
def test_path_boundaries(steps):
    def P(m, n):
        return m4ri_amd.plan_pivot_exchange_batch(m, n, steps)
    assert [P(*s) for s in [(0, 0), (1, 1), (64, 64), (65, 1), (1, 65), (65, 64), (64, 65), (64, 1024), (512, 1024)]] == [0, 0, 0, 1, 1, 1, 1, 1, 1]
    assert P(1100, 1100) == 2 and _lds_bytes(1100, 1100) > LDS_BUDGET
    n = max(n for n in range(65, 1200) if _lds_bytes(n, n) <= LDS_BUDGET)     # the largest square of path 1 by the documented formula
    assert (P(n, n), P(n + 1, n + 1)) == (1, 2)
    m = max(m for m in range(1, 3000) if _lds_bytes(m, 1024) <= LDS_BUDGET)
    assert (P(m, 1024), P(m + 1, 1024)) == (1, 2)
    assert [P(*s) for s in [(1024, 4096), (1025, 4096), (1024, 4097), (1, 64 * 65536), (1, 64 * 65536 + 1), (65536, 64), (65537, 1), (65536, 65)]] \
        == [2, 3, 3, 2, 3, 2, 3, 3]
    assert P(1 << 40, 1 << 40) == 3 and P(0, 1 << 40) == 3 and P(1 << 40, 0) == 3
    rng = np.random.default_rng(1)
    for m, n in rng.integers(0, 3000, size=(300, 2)).tolist():
        assert P(m, n) == _want_path(m, n, steps), (m, n)


def test_one_step_goes_in_place():
    """The step count's part in the plan: a call of one step takes path 2 wherever path 1 would hold the member; paths 0 and 3 and
    every other step count are as the shape says."""
    P = m4ri_amd.plan_pivot_exchange_batch
    assert [P(m, n, 1) for (m, n) in [(0, 0), (64, 64), (65, 1), (1, 65), (64, 1024), (512, 1024), (1100, 1100), (1024, 4096), (1025, 4096)]] \
        == [0, 0, 2, 2, 2, 2, 2, 2, 3]
    assert [P(65, 65, s) for s in (0, 1, 2, 3, 4)] == [1, 2, 1, 1, 1]
    rng = np.random.default_rng(2)
    for m, n in rng.integers(0, 3000, size=(300, 2)).tolist():
        assert P(m, n, 1) == _want_path(m, n, 1), (m, n)


def test_plan_ignores_the_override_variables(monkeypatch):
    P = m4ri_amd.plan_pivot_exchange_batch
    for v in ("0", "1", "64", "100000", "163840", "junk", "-7"):
        monkeypatch.setenv(PATH0, v)
        monkeypatch.setenv(PATH1, v)
        assert (P(1, 1, 1), P(64, 64, 4), P(65, 65, 1), P(65, 65, 2), P(1100, 1100, 16), P(1025, 4096, 1)) == (0, 0, 2, 1, 2, 3), v


def test_negative_sizes():
    P = m4ri_amd.plan_pivot_exchange_batch
    assert P(-1, 5, 1) == -1 and P(5, -1, 1) == -1 and P(5, 5, -1) == -1 and P(-1, 1 << 40, 1) == -1 and P(1 << 40, 1 << 40, -1) == -1


# ---- the argument checks ------------------------------------------------------------------------------------------------------------------
# D: 2 members of 4 x 64 (4 words each, 64 bytes in all) at D0; pivots: 2 x 4 entries (32 bytes) at P0; rank: 2 entries (8 bytes) at R0;
# req: 2 x 3 pairs (48 bytes) at Q0; order: 2 x 64 entries (512 bytes) at O0; done: 2 entries (8 bytes) at N0; all far from each other.
D0, P0, R0, Q0, O0, N0 = 1 << 20, 1 << 22, 1 << 24, 1 << 26, 1 << 28, 1 << 30


def _call(D=D0, d_stride=1, d_bs=4, nrows=4, ncols=64, pivot_rows=4, pivots=P0, rank=R0, batch=2, req=Q0, r_bs=6, steps=3, seed=7, order=O0,
          o_bs=64, olen=64, done=N0):
    return m4ri_amd.lib().m4ri_amd_pivot_exchange_batch_dev(D, d_stride, d_bs, nrows, ncols, pivot_rows, pivots, rank, batch, req, r_bs, steps, seed,
                                                            order, o_bs, olen, done, None)


@pytest.mark.parametrize("kw", [
    dict(nrows=-1, pivot_rows=0), dict(ncols=-1, olen=0), dict(pivot_rows=-1), dict(olen=-1), dict(batch=-1), dict(steps=-1), dict(d_stride=-1),
    dict(d_bs=-1), dict(r_bs=-1), dict(o_bs=-1),
    dict(pivot_rows=5), dict(olen=65), dict(nrows=0), dict(ncols=0),                     # pivot_rows > nrows, olen > ncols
    dict(d_stride=0), dict(ncols=65, d_bs=8), dict(ncols=129, d_stride=2, d_bs=16),      # a stride below the width
    dict(d_bs=3), dict(d_bs=0),                                                          # overlapping D members
    dict(r_bs=5), dict(r_bs=1), dict(steps=4), dict(o_bs=63), dict(o_bs=0),              # request lists or orders that overlap
    dict(D=None), dict(pivots=None), dict(rank=None), dict(D=None, req=None), dict(pivots=None, order=None, done=None),
    dict(pivots=D0 + 60), dict(pivots=D0 - 28), dict(rank=D0 + 60), dict(rank=D0 - 4), dict(req=D0 + 60), dict(req=D0 - 44),   # D meeting each
    dict(req=D0 - 20, r_bs=0), dict(order=D0 + 60), dict(order=D0 - 508), dict(done=D0 + 60), dict(done=D0 - 4),
    dict(rank=P0 + 28), dict(rank=P0 - 4), dict(req=P0 + 28), dict(req=P0 - 44), dict(order=P0 + 28), dict(order=P0 - 508),    # pivots meeting
    dict(done=P0 + 28), dict(done=P0 - 4),
    dict(req=R0 + 4), dict(req=R0 - 44), dict(order=R0 + 4), dict(order=R0 - 508), dict(done=R0 + 4), dict(done=R0 - 4), dict(done=R0),   # rank
    dict(order=Q0 + 44), dict(order=Q0 - 508), dict(done=Q0 + 44), dict(done=Q0 - 4), dict(done=Q0 + 20, r_bs=0),              # req meeting
    dict(done=O0 + 508), dict(done=O0 - 4),                                                                                    # order and done
    dict(pivots=R0 + 4, pivot_rows=1), dict(pivots=R0 - 4, pivot_rows=1),                # pm = 1: two entries
])
def test_invalid_arguments(kw):
    """Rejected before any HIP call: the pointers are not device memory (and this machine may have no GPU at all)."""
    assert _call(**kw) == HIP_ERROR_INVALID_VALUE


@pytest.mark.parametrize("kw", [
    dict(), dict(req=None), dict(r_bs=0), dict(order=None), dict(order=None, o_bs=0, olen=0), dict(olen=0, o_bs=0), dict(olen=7, o_bs=7), dict(done=None),
    dict(pivot_rows=0), dict(pivot_rows=3), dict(d_stride=3, d_bs=10), dict(ncols=65, olen=65, o_bs=65, d_stride=2, d_bs=8), dict(steps=0),
    dict(steps=0, D=None, pivots=None, rank=None), dict(nrows=0, pivot_rows=0, D=None, pivots=None, rank=None),
    dict(ncols=0, olen=0, D=None, pivots=None, rank=None, order=None), dict(r_bs=7), dict(steps=1, r_bs=2), dict(req=None, r_bs=0, steps=1 << 40),
    dict(nrows=1024, ncols=4096, pivot_rows=1024, d_stride=64, d_bs=1 << 16, olen=0),                                          # the cap itself
])
def test_batch_zero_is_success(kw):
    """Legal sizes, strides and absent operands, shown with batch = 0, which returns before any HIP call.  The accepted neighbours of
    the overlaps above need members: tests/test_gpu_pivot_exchange_batch.py runs the operands packed back to back."""
    assert _call(**dict(kw, batch=0)) == 0


@pytest.mark.parametrize("kw", [
    dict(nrows=1025, ncols=4096, pivot_rows=0), dict(nrows=1024, ncols=4097), dict(nrows=1, pivot_rows=1, ncols=64 * 65536 + 1),
    dict(nrows=65537, ncols=1), dict(nrows=1 << 40, ncols=1 << 40),
])
@pytest.mark.parametrize("batch", [0, 2])
def test_beyond_the_cap_is_not_supported(kw, batch):
    w = (kw["ncols"] + 63) // 64
    big = dict(d_stride=w, d_bs=1 << 50, order=None, o_bs=0, olen=0)
    assert _call(**dict(big, **kw, batch=batch)) == HIP_ERROR_NOT_SUPPORTED


def test_sizes_and_strides_are_checked_before_the_cap():
    assert _call(nrows=1025, ncols=4096, d_stride=63) == HIP_ERROR_INVALID_VALUE
    assert _call(nrows=1025, ncols=4096, d_stride=64, batch=-1) == HIP_ERROR_INVALID_VALUE
    assert _call(nrows=1025, ncols=4096, d_stride=64, pivot_rows=1026) == HIP_ERROR_INVALID_VALUE
    assert _call(nrows=1025, ncols=4096, d_stride=64, steps=-1) == HIP_ERROR_INVALID_VALUE


def test_python_wrappers_are_bound():
    with pytest.raises(RuntimeError):
        m4ri_amd.pivot_exchange_batch_dev(D0, 1, 4, 4, 64, 4, 0, R0, 2, steps=1)                      # no pivots
    with pytest.raises(RuntimeError):
        m4ri_amd.pivot_exchange_batch_dev(D0, 1, 4, 4, 64, 4, P0, R0, 2, steps=1, done=R0 + 4)        # done meets rank
    with pytest.raises(RuntimeError, match="801"):
        m4ri_amd.pivot_exchange_batch_dev(D0, 64, 1 << 20, 1025, 4096, 4, P0, R0, 2, steps=1)
    m4ri_amd.pivot_exchange_batch_dev(D0, 1, 4, 4, 64, 4, P0, R0, 0, Q0, 6, 3, -1, O0, 64, 64, N0, stream=0)   # batch = 0; any 64-bit seed
    m4ri_amd.pivot_exchange_batch_dev(D0, 1, 4, 4, 64, 4, P0, R0, 0)
