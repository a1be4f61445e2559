"""The host side of m4ri_amd_sort_rows_batch_dev, without a GPU: the two NumPy forms of the order of tests/sort_rows_cases.py against each
other and against np.unique, the plan, units and scratch arithmetic, the argument checks of the call (they run before any HIP call, so
the pointers are never dereferenced) and the argument order of the Python wrappers."""
import inspect

import numpy as np
import pytest

import lists_collide_cases as lc
import m4ri_amd
import sort_rows_cases as sr

HIP_ERROR_INVALID_VALUE, HIP_ERROR_NOT_SUPPORTED = 1, 801
C = m4ri_amd.sort_rows_units(1, 1, 0, 1)[0]      # the entries of a chunk, whatever the library chose
ROWS_MAX = 1 << 24


# ---- the NumPy rule, twice --------------------------------------------------------------------------------------------------------------

def test_a_hand_checked_member():
    """Five rows of 4 bits (bit 0 first): 1100, 0010, 1100, 0001, 0010 are the words 3, 4, 3, 8, 4.  No window: by the words, then the index.
    Window column 2: the key is 1 for the rows 1 and 4 only, so they go last."""
    A = np.array([[1, 1, 0, 0], [0, 0, 1, 0], [1, 1, 0, 0], [0, 0, 0, 1], [0, 0, 1, 0]], dtype=np.uint8)
    for rule in (sr.by_lexsort, sr.by_sorted):
        order, uniq, mult = sr.expect(A, [], rule)
        assert order.tolist() == [0, 2, 1, 4, 3] and uniq.tolist() == [0, 1, 3] and mult.tolist() == [2, 2, 1]
        order, uniq, mult = sr.expect(A, [2], rule)
        assert order.tolist() == [0, 2, 3, 1, 4] and uniq.tolist() == [0, 3, 1] and mult.tolist() == [2, 1, 2]
        order, uniq, mult = sr.expect(A, [3, 2, 3], rule)            # keys 0, 2, 0, 5, 2
        assert order.tolist() == [0, 2, 1, 4, 3] and uniq.tolist() == [0, 1, 3]
        for cols in ([4], [-1], [0, 4, 1]):
            assert sr.expect(A, cols, rule) is None
        order, uniq, mult = sr.expect(A[:0], [1], rule)
        assert len(order) == len(uniq) == len(mult) == 0
        order, uniq, mult = sr.expect(np.zeros((3, 0), dtype=np.uint8), [], rule)    # n = 0: all rows equal
        assert order.tolist() == [0, 1, 2] and uniq.tolist() == [0] and mult.tolist() == [3]


def test_the_two_forms_and_np_unique_on_the_pinned_input():
    """300 rows of 130 bits from a pool of 37, window [129, 3, 64, 3, 70]: 37 classes, the largest of 14 rows."""
    rng = np.random.default_rng(302)
    A = sr.pool_rows(rng, 300, 130, 37)
    cols = [129, 3, 64, 3, 70]
    a, b = sr.expect(A, cols, sr.by_lexsort), sr.expect(A, cols, sr.by_sorted)
    for x, y in zip(a, b):
        assert np.array_equal(x, y)
    order, uniq, mult = a
    rows, first, counts = np.unique(A, axis=0, return_index=True, return_counts=True)
    assert len(uniq) == len(rows) == 37 and mult.max() == counts.max() == 14
    assert sorted(uniq.tolist()) == sorted(first.tolist())                       # the smallest index of each class
    back = {int(i): int(c) for i, c in zip(first, counts)}
    assert [back[int(i)] for i in uniq] == mult.tolist() and mult.sum() == 300
    assert sorted(order.tolist()) == list(range(300))
    key = lc.window_keys(A, cols)
    assert (np.diff(key[order].astype(np.int64)) >= 0).all()                     # the key counts first


@pytest.mark.parametrize("rows,n,pool,ell", [(0, 5, 1, 0), (1, 1, 1, 1), (40, 64, 5, 0), (90, 65, 90, 3), (200, 130, 11, 13), (64, 63, 2, 1), (70, 200, 70, 64)])
def test_the_two_forms_agree(rows, n, pool, ell):
    rng = np.random.default_rng(rows * 7 + n)
    A = sr.pool_rows(rng, rows, n, pool)
    cols = [int(c) for c in rng.integers(0, n, ell)]
    a, b = sr.expect(A, cols, sr.by_lexsort), sr.expect(A, cols, sr.by_sorted)
    for x, y in zip(a, b):
        assert np.array_equal(x, y)
    order, uniq, mult = a
    rows_u, first, counts = np.unique(A, axis=0, return_index=True, return_counts=True)
    assert sorted(uniq.tolist()) == sorted(first.tolist()) and mult.sum() == rows and len(uniq) == len(rows_u)
    assert np.array_equal(np.unique(A[uniq], axis=0), rows_u)


def test_the_words_are_compared_as_unsigned_numbers_and_dirt_does_not_count():
    """Bit 63 set must go AFTER bit 63 clear; two rows that differ only behind column n are one class."""
    A = np.zeros((3, 70), dtype=np.uint8)
    A[0, 63] = 1
    A[1, 62] = 1
    order, uniq, mult = sr.expect(A, [])
    assert order.tolist() == [2, 1, 0]
    rng = np.random.default_rng(1)
    B = rng.integers(0, 2, (4, 70), dtype=np.uint8)
    assert np.array_equal(lc.unpack(lc.pack(B, 3, rng), 70), B) and np.array_equal(sr.words(B), lc.pack(B).view(np.uint64))


# ---- plan, units, scratch ---------------------------------------------------------------------------------------------------------------

def _pow2(x):
    p = 2
    while p < x:
        p *= 2
    return p


def test_the_chunk_is_what_lds_holds():
    assert C & (C - 1) == 0 and 2048 <= C and C * 12 <= 160 * 1024


@pytest.mark.parametrize("nx", [0, 1, 2, 3, 63, 64, 65, 255, 256, 257, C - 1, C, C + 1, 2 * C, 2 * C + 1, 4 * C + 3, 1 << 20, ROWS_MAX])
@pytest.mark.parametrize("batch", [0, 1, 5, 1024])
def test_plan_units_and_scratch(nx, batch):
    path = m4ri_amd.plan_sort_rows_batch(nx, 130, 13, batch)
    c, padded, launches = m4ri_amd.sort_rows_units(nx, 130, 13, batch)
    need = m4ri_amd.sort_rows_scratch_bytes(nx, 130, 13, batch)
    assert path == (0 if nx <= C else 1) and c == C and padded == _pow2(nx)
    if path == 0:
        assert launches == 1 and need == 0
    else:
        levels = (padded // C).bit_length() - 1
        assert launches == 1 + sum(l + 1 for l in range(1, levels + 1)) + 4
        per_member = padded * 13 + padded // 1024 * 4 + 4
        assert need % 16 == 0 and 0 <= need - batch * per_member < 16 if batch else need == 0


def test_the_boundary_and_the_levels_the_gpu_tests_pin():
    P, U = m4ri_amd.plan_sort_rows_batch, m4ri_amd.sort_rows_units
    assert P(C, 64, 8, 3) == 0 and P(C + 1, 64, 8, 3) == 1
    assert U(C + 1, 64, 8, 1)[1:] == (2 * C, 1 + 2 + 4) and U(2 * C, 64, 8, 1)[1:] == (2 * C, 7)
    assert U(2 * C + 1, 64, 8, 1)[1:] == (4 * C, 1 + 2 + 3 + 4) and U(4 * C + 3, 64, 8, 1)[1:] == (8 * C, 1 + 2 + 3 + 4 + 4)   # three global levels
    assert U(ROWS_MAX, 64, 8, 1)[1] == ROWS_MAX


def test_degenerate_and_huge_shapes():
    P = m4ri_amd.plan_sort_rows_batch
    for bad in ((-1, 1, 0, 1), (1, -1, 0, 1), (1, 1, -1, 1), (1, 1, 0, -1)):
        assert P(*bad) == -1 and m4ri_amd.lib().m4ri_amd_sort_rows_scratch_bytes(*bad) == -1
        with pytest.raises(ValueError):
            m4ri_amd.sort_rows_units(*bad)
        with pytest.raises(ValueError):
            m4ri_amd.sort_rows_scratch_bytes(*bad)
    assert m4ri_amd.lib().m4ri_amd_sort_rows_units(5, 64, 3, 1, None, None, None) == 0             # every pointer is optional
    big = (1 << 63) - 1                                             # beyond the call's limits: the same rule, no overflow
    assert P(big, 64, 3, big) == 1 and m4ri_amd.sort_rows_units(big, 64, 3, big)[0] == C
    assert m4ri_amd.lib().m4ri_amd_sort_rows_scratch_bytes(ROWS_MAX, 64, 3, big) == -1               # beyond int64
    assert m4ri_amd.sort_rows_scratch_bytes(ROWS_MAX, 1024, 64, 1) == ROWS_MAX * 13 + ROWS_MAX // 1024 * 4 + 16


# ---- the argument checks ----------------------------------------------------------------------------------------------------------------
# X two members of 6 rows of 64 bits (12 words, 96 bytes) at X0, xcount (2 entries) at N0, two windows of three entries at C0; order, uniq
# and mult, two members of 6 entries l_bs = 7 apart (104 bytes), at O0, U0 and M0; ucount (2 entries) at K0; the scratch at S0.
X0, N0, C0, O0, U0, M0, K0, S0 = 1 << 20, 1 << 22, 1 << 24, 1 << 26, 1 << 28, 1 << 29, 1 << 30, 1 << 32
LB = (7 + 6) * 8


def _sort(X=X0, x_stride=1, x_bs=6, nx=6, n=64, xcount=N0, batch=2, cols=C0, c_bs=3, ell=3, order=O0, ucount=K0, uniq=U0, mult=M0, l_bs=7, scratch=None,
          scratch_bytes=0):
    return m4ri_amd.lib().m4ri_amd_sort_rows_batch_dev(X, x_stride, x_bs, nx, n, xcount, batch, cols, c_bs, ell, order, ucount, uniq, mult, l_bs, scratch,
                                                       scratch_bytes, None)


OUTS = {"order": (O0, LB), "uniq": (U0, LB), "mult": (M0, LB), "ucount": (K0, 16)}
INS = {"X": (X0, 96), "xcount": (N0, 16), "cols": (C0, 24)}
OVERLAPS = [{o: base + ib - 8} for o in OUTS for base, ib in INS.values()] + [{o: base - ob + 8} for o, (_, ob) in OUTS.items() for base, _ in INS.values()]
OVERLAPS += [{o: b2 + ob2 - 8} for o in OUTS for o2, (b2, ob2) in OUTS.items() if o2 != o]
NEIGHBOURS = [{o: base + ib} for o in OUTS for base, ib in INS.values()] + [{o: base - ob} for o, (_, ob) in OUTS.items() for base, _ in INS.values()]
NEIGHBOURS += [{o: b2 + ob2} for o in OUTS for o2, (b2, ob2) in OUTS.items() if o2 != o]


def test_no_members():
    assert _sort(batch=0) == 0                                       # batch = 0 touches nothing
    assert _sort(batch=0, X=None, order=O0, ucount=None, uniq=None, mult=None) == 0


@pytest.mark.parametrize("kw", [dict(nx=-1), dict(n=-1), dict(ell=-1), dict(batch=-1), dict(x_stride=-1), dict(x_bs=-1), dict(c_bs=-1), dict(l_bs=-1),
                                dict(scratch_bytes=-1), dict(x_stride=0), dict(n=130, x_stride=2), dict(l_bs=5), dict(X=None),
                                dict(order=None, ucount=None, uniq=None, mult=None), dict(ucount=None), dict(ucount=None, uniq=None), dict(uniq=None),
                                dict(cols=None, n=2, ell=3), dict(cols=None, n=0, ell=1, x_stride=0)])
def test_invalid_value(kw):
    assert _sort(**kw) == HIP_ERROR_INVALID_VALUE
    assert _sort(**dict(kw, batch=0)) in (0, HIP_ERROR_INVALID_VALUE)


def test_checks_that_need_members():
    assert _sort(batch=0, X=None) == 0 and _sort(batch=0, l_bs=0) == 0           # no member: nothing is read, nothing has a stride
    assert _sort(batch=1, l_bs=0, order=None) != HIP_ERROR_INVALID_VALUE         # one member needs no batch stride
    assert _sort(nx=1, x_stride=0, l_bs=1) != HIP_ERROR_INVALID_VALUE            # one row needs no stride
    assert _sort(X=None, n=0, ell=0, cols=None, x_stride=0) != HIP_ERROR_INVALID_VALUE       # n = 0: no row is read
    assert _sort(X=None, nx=0) != HIP_ERROR_INVALID_VALUE


@pytest.mark.parametrize("kw", [dict(n=1025, x_stride=17), dict(ell=65, c_bs=65), dict(nx=ROWS_MAX + 1, l_bs=ROWS_MAX + 1), dict(nx=(1 << 63) - 1, l_bs=(1 << 63) - 1)])
def test_not_supported(kw):
    assert _sort(**kw) == HIP_ERROR_NOT_SUPPORTED
    assert _sort(**dict(kw, batch=0)) == HIP_ERROR_NOT_SUPPORTED


@pytest.mark.parametrize("kw", OVERLAPS)
def test_an_output_that_meets_an_operand_or_another_output(kw):
    assert _sort(**kw) == HIP_ERROR_INVALID_VALUE


@pytest.mark.parametrize("kw", NEIGHBOURS)
def test_neighbours_do_not_meet(kw):
    assert _sort(**kw) != HIP_ERROR_INVALID_VALUE


def test_the_scratch():
    nx = C + 1
    need = m4ri_amd.sort_rows_scratch_bytes(nx, 64, 3, 2)
    long = dict(nx=nx, x_bs=nx, l_bs=nx, order=O0, ucount=K0, uniq=None, mult=None)
    assert need > 0
    assert _sort(**long, scratch=None, scratch_bytes=need) == HIP_ERROR_INVALID_VALUE
    assert _sort(**long, scratch=S0, scratch_bytes=need - 1) == HIP_ERROR_INVALID_VALUE
    assert _sort(**long, scratch=S0 + 4, scratch_bytes=need) == HIP_ERROR_INVALID_VALUE              # not 8-byte aligned
    assert _sort(**long, scratch=S0, scratch_bytes=need) != HIP_ERROR_INVALID_VALUE
    assert _sort(**long, scratch=X0 + 8, scratch_bytes=need) == HIP_ERROR_INVALID_VALUE              # on X
    assert _sort(**long, scratch=K0 - need + 8, scratch_bytes=need) == HIP_ERROR_INVALID_VALUE       # its end on ucount
    assert _sort(**long, scratch=K0 - need, scratch_bytes=need) != HIP_ERROR_INVALID_VALUE
    assert _sort(**long, scratch=O0 + 16, scratch_bytes=need) == HIP_ERROR_INVALID_VALUE             # on order
    assert _sort(**dict(long, batch=0), scratch=None, scratch_bytes=0) == 0
    assert _sort(scratch=X0, scratch_bytes=1 << 20) != HIP_ERROR_INVALID_VALUE                       # path 0: the scratch is ignored


# ---- the wrappers -------------------------------------------------------------------------------------------------------------------------

def test_the_wrapper_passes_its_arguments_in_the_order_of_the_header(monkeypatch):
    names = ["X", "x_stride", "x_bs", "nx", "n", "xcount", "batch", "cols", "c_bs", "ell", "order", "ucount", "uniq", "mult", "l_bs", "scratch", "scratch_bytes",
             "stream"]
    assert list(inspect.signature(m4ri_amd.sort_rows_batch_dev).parameters) == names
    seen = {}

    class Lib:
        def m4ri_amd_sort_rows_batch_dev(self, *args):
            seen["args"] = args
            return 0

    monkeypatch.setattr(m4ri_amd, "lib", lambda: Lib())
    m4ri_amd.sort_rows_batch_dev(*range(101, 119))
    assert seen["args"] == tuple(range(101, 119))
    m4ri_amd.sort_rows_batch_dev(101, 1, 2, 3, 4, order=7)
    assert seen["args"] == (101, 1, 2, 3, 4, None, 1, None, 0, 0, 7, None, None, None, 0, None, 0, 0)


def test_the_wrapper_raises_what_the_call_returns():
    with pytest.raises(Exception):
        m4ri_amd.sort_rows_batch_dev(X0, 1, 6, 6, 64, batch=2, l_bs=7)              # no output
    m4ri_amd.sort_rows_batch_dev(X0, 1, 6, 6, 64, batch=0, order=O0, l_bs=7)
    assert m4ri_amd.plan_sort_rows_batch(5, 64, 3, 2) == 0 and m4ri_amd.sort_rows_scratch_bytes(5, 64, 3, 2) == 0
