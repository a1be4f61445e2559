"""The host side of m4ri_amd_lists_collide_batch_dev and m4ri_amd_lists_words_batch_dev, without a GPU: the two NumPy rules of
tests/lists_collide_cases.py against each other, the plan and units arithmetic, the argument checks of both calls (they run before any HIP
call, so the pointers are never dereferenced) and the argument order of the Python wrappers."""
import inspect

import numpy as np
import pytest

import lists_collide_cases as lc
import m4ri_amd

HIP_ERROR_INVALID_VALUE, HIP_ERROR_NOT_SUPPORTED = 1, 801
C = m4ri_amd.lists_collide_units(1, 1, 1, 0, 1)[0]      # the rows of a chunk, whatever the library chose


# ---- the NumPy rule, twice --------------------------------------------------------------------------------------------------------------

def test_a_hand_checked_member():
    """X = {1011, 0110}, Y = {1001, 0111, 1011}, window columns 1 and 0: the pairs (0, 0) 0010, (0, 2) 0000 and (1, 1) 0001 collide."""
    X = np.array([[1, 0, 1, 1], [0, 1, 1, 0]], dtype=np.uint8)
    Y = np.array([[1, 0, 0, 1], [0, 1, 1, 1], [1, 0, 1, 1]], dtype=np.uint8)
    for rule in (lc.brute, lc.join):
        h, l, k, c = lc.expect(X, Y, None, [1, 0], 0, 4, rule)
        assert h.tolist() == [1, 2, 0, 0, 0] and l == 2 and k.tolist() == [2, (1 << 40) | 0, (1 << 40) | 4] and c == 3
        h, l, k, c = lc.expect(X, Y, None, [1, 0], 1, 1, rule)
        assert l == (1 << 40) | 0 and k.tolist() == [(1 << 40) | 0, (1 << 40) | 4] and c == 2
        h, l, k, c = lc.expect(X, Y, np.array([0, 0, 1, 1], dtype=np.uint8), [1, 0], 0, 9, rule)     # the same pairs, 1 more bit: 0001, 0011, 0010
        assert h.tolist() == [0, 2, 1, 0, 0] and k.tolist() == [(1 << 40) | 0, (1 << 40) | 4, (2 << 40) | 2]
        for cols in ([4], [-1], [0, 1, 4]):
            h, l, k, c = lc.expect(X, Y, None, cols, 0, 4, rule)
            assert h.tolist() == [-1] * 5 and l == -2 and len(k) == 0 and c == -1
        assert lc.expect(X, Y, None, [], 0, 4, rule)[3] == 6                                        # no window: every pair
    assert ["".join(map(str, r)) for r in lc.words_of(X, Y, None, [0, 2, 4])] == ["0010", "0000", "0001"]


@pytest.mark.parametrize("nx,ny,n,ell,repeat", [(7, 9, 5, 0, False), (40, 30, 70, 3, True), (33, 65, 64, 4, False), (50, 50, 130, 5, True),
                                                (64, 3, 64, 64, True), (1, 1, 1, 1, False), (90, 80, 100, 6, True)])
def test_brute_force_and_the_sorted_join_agree(nx, ny, n, ell, repeat):
    rng = np.random.default_rng(nx * 1000 + ny)
    X, Y = rng.integers(0, 2, (nx, n), dtype=np.uint8), rng.integers(0, 2, (ny, n), dtype=np.uint8)
    V = rng.integers(0, 2, n, dtype=np.uint8)
    if repeat:                                  # repeated rows on both sides, and a right row that is V ^ a left row: weight 0
        X[nx // 2] = X[0]
        Y[ny - 1] = Y[0]
        Y[1] = X[nx - 1] ^ V
    cols = [int(c) for c in rng.integers(0, n, ell)] if ell <= n else None
    if ell == 64:
        cols = [int(c) for c in rng.permutation(n)[:63]] + [int(rng.integers(0, n))]
    for v in (None, V):
        wb, rb = lc.brute(X, Y, v, cols)
        wj, rj = lc.join(X, Y, v, cols)
        ob, oj = np.argsort(rb), np.argsort(rj)
        assert np.array_equal(rb[ob], rj[oj]) and np.array_equal(wb[ob], wj[oj]) and len(set(rb.tolist())) == len(rb)
        for w_min, w_max in ((0, n), (1, n // 2), (n // 2, 2 * n), (3, 2)):
            a, b = lc.expect(X, Y, v, cols, w_min, w_max, lc.brute), lc.expect(X, Y, v, cols, w_min, w_max, lc.join)
            assert np.array_equal(a[0], b[0]) and a[1] == b[1] and np.array_equal(a[2], b[2]) and a[3] == b[3]
            assert a[0].sum() == len(rb) and a[3] == a[0][w_min:min(w_max, n) + 1].sum()
    if repeat:
        assert 0 in lc.brute(X, Y, V, cols)[0]
    if ell == 0:
        assert len(lc.brute(X, Y, V, cols)[1]) == nx * ny


def test_dirty_bits_do_not_count():
    """pack() puts dirt behind column n and into the padding; unpack() and the rule see the n valid bits only."""
    rng = np.random.default_rng(5)
    for n in (1, 63, 64, 65, 130):
        B = rng.integers(0, 2, (6, n), dtype=np.uint8)
        clean, dirty = lc.pack(B, lc.width(n) + 2), lc.pack(B, lc.width(n) + 2, rng)
        assert np.array_equal(lc.unpack(clean, n), B) and np.array_equal(lc.unpack(dirty, n), B)
        assert (clean[:, lc.width(n):] == 0).all() and (dirty[:, lc.width(n):] != 0).any()
        assert n % 64 == 0 or not np.array_equal(clean[:, lc.width(n) - 1], dirty[:, lc.width(n) - 1])


# ---- plan and units ---------------------------------------------------------------------------------------------------------------------

def _units(nx, ny, n=64, ell=8, batch=1):
    return m4ri_amd.lists_collide_units(nx, ny, n, ell, batch)


def test_the_chunk():
    assert 1 <= C <= 65536
    for nx in (1, C - 1, C, C + 1, 2 * C, 2 * C + 1, 3 * C + 5, (1 << 31) - 1):
        c, chunks, slices = _units(nx, 1)
        assert c == C and chunks == -(-nx // C) and slices == 1
    assert _units(C, 700) == (C, 1, 1) and _units(C + 1, 700) == (C, 2, 1)
    assert m4ri_amd.plan_lists_collide_batch(C, 700, 130, 10, 1) == 0 and m4ri_amd.plan_lists_collide_batch(C + 1, 700, 130, 10, 1) == 1


@pytest.mark.parametrize("nx", [1, 2, 255, 256, 257, 300, 5000, C - 1, C, C + 1, 2 * C + 1, 32640, 1 << 20])
@pytest.mark.parametrize("ny", [1, 255, 256, 257, 511, 512, 700, 32640, 300000, 1 << 20, (1 << 31) - 1])
@pytest.mark.parametrize("batch", [1, 5, 1024, 5000])
def test_plan_and_units(nx, ny, batch):
    if nx * ny > 1 << 40:
        return
    c, chunks, slices = _units(nx, ny, batch=batch)
    path = m4ri_amd.plan_lists_collide_batch(nx, ny, 64, 8, batch)
    assert chunks == -(-nx // C) and slices >= 1
    assert (path == 0) == (chunks == 1 and slices == 1) and path in (0, 1)
    slice_len = -(-ny // slices)                                     # no slice is longer than this
    chunk = min(nx, C)
    assert chunk * slice_len < 1 << 32                               # the 32-bit bins of a workgroup hold
    assert slice_len >= min(ny, max(chunk, 256))                     # the floor: the table build is amortised
    if slices > 1:                                                   # cut only until the call has about 1024 workgroups
        assert batch * chunks * (slices - 1) < 1024 or chunk * (-(-ny // (slices - 1))) >= 1 << 32


def test_the_shapes_the_gpu_tests_pin():
    for nx in (1, 2, 63, 64, 65, 300):
        for ny in (1, 64, 257):
            for batch in (1, 5):
                assert m4ri_amd.plan_lists_collide_batch(nx, ny, 130, 7, batch) == 0
    c, chunks, slices = _units(2 * C + 1, 300000, 64, 24, 1)
    assert chunks == 3 and slices >= 3 and (2 * C + 1) * 300000 < 5 * 10**9


def test_degenerate_shapes():
    P = m4ri_amd.plan_lists_collide_batch
    assert P(0, 5, 64, 3, 1) == 0 and P(5, 0, 64, 3, 1) == 0 and P(1 << 20, 1 << 20, 0, 0, 1) == 0 and P(5, 5, 64, 3, 0) == 0
    assert _units(0, 5)[1:] == (0, 0) and _units(5, 0)[1:] == (0, 0) and _units(5, 5, n=0, ell=0)[1:] == (0, 0)
    for bad in ((-1, 1, 1, 0, 1), (1, -1, 1, 0, 1), (1, 1, -1, 0, 1), (1, 1, 1, -1, 1), (1, 1, 1, 0, -1)):
        assert P(*bad) == -1
        with pytest.raises(ValueError):
            m4ri_amd.lists_collide_units(*bad)
    assert m4ri_amd.lib().m4ri_amd_lists_collide_units(5, 5, 64, 3, 1, None, None, None) == 0       # every pointer is optional
    big = (1 << 63) - 1                                             # beyond the call's limits: the same rule, no overflow
    assert P(big, big, 64, 3, big) == 1 and _units(big, big, batch=big)[1] == -(-big // C) and P(1, big, 64, 3, 1) == 1


# ---- the argument checks of the join ----------------------------------------------------------------------------------------------------
# X two members of 4 rows of 64 bits (8 words) at X0, Y two members of 3 rows (6 words) at Y0, V two words at V0, two windows of three
# entries at C0, hist (2 * 65 entries) at H0, lightest (2) at L0; the list, two members of cap = 5 keys l_bs = 6 apart (88 bytes), at K0,
# count (2 entries) at N0.
X0, Y0, V0, C0, H0, L0, K0, N0 = 1 << 20, 1 << 22, 1 << 24, 1 << 26, 1 << 28, 1 << 29, 1 << 30, 1 << 31
HB, KB = 2 * 65 * 8, (6 + 5) * 8


def _join(X=X0, x_stride=1, x_bs=4, nx=4, Y=Y0, y_stride=1, y_bs=3, ny=3, n=64, V=V0, v_bs=1, batch=2, cols=C0, c_bs=3, ell=3, w_min=0, w_max=64,
          hist=H0, lightest=L0, lst=K0, l_bs=6, cap=5, count=N0):
    return m4ri_amd.lib().m4ri_amd_lists_collide_batch_dev(X, x_stride, x_bs, nx, Y, y_stride, y_bs, ny, n, V, v_bs, batch, cols, c_bs, ell, w_min, w_max,
                                                           hist, lightest, lst, l_bs, cap, count, None)


OUTS = {"hist": (H0, HB), "lightest": (L0, 16), "lst": (K0, KB), "count": (N0, 16)}
INS = {"X": (X0, 64), "Y": (Y0, 48), "V": (V0, 16), "cols": (C0, 24)}
OVERLAPS = [{o: base + ib - 8} for o in OUTS for base, ib in INS.values()] + [{o: base - ob + 8} for o, (_, ob) in OUTS.items() for base, _ in INS.values()]
OVERLAPS += [{o: b2 + ob2 - 8} for o in OUTS for o2, (b2, ob2) in OUTS.items() if o2 != o]
NEIGHBOURS = [{o: base + ib} for o in OUTS for base, ib in INS.values()] + [{o: base - ob} for o, (_, ob) in OUTS.items() for base, _ in INS.values()]
NEIGHBOURS += [{o: b2 + ob2} for o in OUTS for o2, (b2, ob2) in OUTS.items() if o2 != o]


@pytest.mark.parametrize("kw", [
    dict(nx=-1), dict(ny=-1), dict(n=-1), dict(batch=-1), dict(ell=-1), dict(x_stride=-1), dict(x_bs=-1), dict(y_stride=-1), dict(y_bs=-1), dict(v_bs=-1),
    dict(c_bs=-1), dict(w_min=-1), dict(w_max=-1), dict(cap=-1), dict(l_bs=-1), dict(cap=-1, lst=None, count=None),
    dict(x_stride=0), dict(y_stride=0), dict(n=65, x_stride=1, y_stride=2), dict(n=65, x_stride=2, y_stride=1),      # a stride below words(n), rows > 1
    dict(X=None), dict(Y=None), dict(X=None, Y=None),                 # rows are read
    dict(cols=None, n=10, ell=11), dict(cols=None, n=0, ell=1),
    dict(count=None), dict(lst=None), dict(count=None, cap=0),        # a list without a count, a count without a list at cap > 0
    dict(hist=None, lightest=None, lst=None, count=None), dict(hist=None, lightest=None, lst=None, count=None, cap=0),   # no output at all
    dict(l_bs=4), dict(l_bs=0),                                       # l_bs < cap with batch > 1
    dict(lst=K0, l_bs=100, count=K0 + 8 * 104),                       # members 100 apart: the span ends behind entry 104
    dict(count=N0, lst=N0 + 8, cap=0, hist=N0),                       # hist on count where the list is not given
] + OVERLAPS)
def test_invalid_arguments_of_the_join(kw):
    assert _join(**kw) == HIP_ERROR_INVALID_VALUE


@pytest.mark.parametrize("kw", [
    dict(), dict(hist=None), dict(lightest=None), dict(hist=None, lightest=None), dict(lst=None, count=None), dict(lst=None, cap=0),
    dict(lst=None, cap=0, hist=None, lightest=None), dict(cap=0, l_bs=0), dict(l_bs=5), dict(cap=1 << 50, l_bs=1 << 50),
    dict(w_max=0), dict(w_max=1 << 40), dict(w_min=9, w_max=3), dict(x_bs=0), dict(y_bs=0), dict(v_bs=0), dict(c_bs=0), dict(V=None), dict(cols=None),
    dict(Y=X0, y_bs=4, ny=4), dict(Y=X0 + 8),                         # a self-join, and lists that overlap
    dict(nx=1, x_stride=0), dict(ny=1, y_stride=0), dict(nx=0, X=None), dict(ny=0, Y=None), dict(n=0, ell=0, X=None, Y=None, x_stride=0, y_stride=0),
    dict(cols=None, ell=64), dict(ell=64, c_bs=64), dict(n=1024, x_stride=16, x_bs=64, y_stride=16, y_bs=48),
    dict(nx=1 << 20, ny=1 << 20, x_bs=1 << 20, y_bs=1 << 20),         # nx * ny = 2^40
    dict(nx=(1 << 31) - 1, ny=512, x_bs=1 << 31, y_bs=512), dict(nx=512, ny=(1 << 31) - 1, x_bs=512, y_bs=1 << 31),
    dict(lst=K0, l_bs=100, count=K0 + 8 * 105), dict(lst=X0, cap=0),  # an empty list meets nothing
] + NEIGHBOURS)
def test_legal_arguments_of_the_join(kw):
    """Legal arguments, the accepted neighbours of the overlaps above among them: shown with batch = 0, which returns before any HIP call."""
    assert _join(**dict(kw, batch=0)) == 0


def test_one_member_needs_no_batch_stride():
    assert _join(batch=1, l_bs=0, X=None) == HIP_ERROR_INVALID_VALUE       # reaches the NULL-X check: l_bs < cap is fine with one member
    assert _join(batch=2, l_bs=0, X=None, lst=None, count=None) == HIP_ERROR_INVALID_VALUE


@pytest.mark.parametrize("kw", [
    dict(n=1025, x_stride=17, y_stride=17), dict(ell=65, c_bs=65), dict(nx=1 << 31), dict(ny=1 << 31), dict(nx=(1 << 20) + 1, ny=1 << 20),
    dict(nx=1 << 20, ny=(1 << 20) + 1), dict(nx=(1 << 40) + 1, ny=1), dict(nx=1 << 62, ny=1 << 62), dict(n=1025, x_stride=17, y_stride=17, batch=0),
])
def test_the_join_beyond_the_limits(kw):
    assert _join(**kw) == HIP_ERROR_NOT_SUPPORTED


def test_negative_sizes_come_before_the_limits():
    assert _join(n=1025, cap=-1) == HIP_ERROR_INVALID_VALUE and _join(ell=65, l_bs=-1) == HIP_ERROR_INVALID_VALUE
    assert _join(nx=1 << 31, w_max=-1) == HIP_ERROR_INVALID_VALUE and _words(n=1025, cap=-1) == HIP_ERROR_INVALID_VALUE


def test_the_existing_bound_stays():
    """C(129, 2) = 8256 left sums are still refused by the row-sum join: the new call is the way beyond."""
    old = m4ri_amd.lib().m4ri_amd_row_sums_collide_list_batch_dev
    assert old(X0, 1, 400, 200, 64, None, 0, 0, 129, 2, 1, None, 0, 3, 0, 64, H0, L0, K0, 6, 5, N0, None) == HIP_ERROR_NOT_SUPPORTED
    assert _join(nx=8256, ny=71, x_bs=8256, y_bs=71, batch=0) == 0


# ---- the argument checks of the words call ----------------------------------------------------------------------------------------------
# X, Y, V as above; keys two members of cap = 5, l_bs = 6 apart at K0; count at N0; W two members of 5 rows of one word, rows 2 words apart,
# members 12 apart: 12 + 8 + 1 = 21 words at W0; skipped (2 int32) at S0.
W0, S0 = 1 << 32, 1 << 33
WB = 21 * 8


def _words(X=X0, x_stride=1, x_bs=4, nx=4, Y=Y0, y_stride=1, y_bs=3, ny=3, n=64, V=V0, v_bs=1, batch=2, keys=K0, l_bs=6, cap=5, count=N0, W=W0, w_stride=2,
           w_bs=12, skipped=S0):
    return m4ri_amd.lib().m4ri_amd_lists_words_batch_dev(X, x_stride, x_bs, nx, Y, y_stride, y_bs, ny, n, V, v_bs, batch, keys, l_bs, cap, count, W, w_stride,
                                                         w_bs, skipped, None)


W_INS = {"X": (X0, 64), "Y": (Y0, 48), "V": (V0, 16), "keys": (K0, KB), "count": (N0, 16)}


@pytest.mark.parametrize("kw", [
    dict(nx=-1), dict(ny=-1), dict(n=-1), dict(batch=-1), dict(x_stride=-1), dict(x_bs=-1), dict(y_stride=-1), dict(y_bs=-1), dict(v_bs=-1), dict(l_bs=-1),
    dict(cap=-1), dict(w_stride=-1), dict(w_bs=-1),
    dict(x_stride=0), dict(y_stride=0), dict(n=65, x_stride=1, y_stride=2, w_stride=2), dict(n=65, x_stride=2, y_stride=1, w_stride=2),
    dict(w_stride=0), dict(n=129, x_stride=3, x_bs=12, y_stride=3, y_bs=9, w_stride=2, w_bs=20),      # w_stride below words(n) with cap > 1
    dict(l_bs=4), dict(w_bs=8), dict(w_bs=0),                         # too small for cap keys / cap rows with batch > 1
    dict(keys=None), dict(W=None), dict(X=None), dict(Y=None),
] + [dict(W=base + ib - 8) for base, ib in W_INS.values()] + [dict(W=base - WB + 8) for base, _ in W_INS.values()]
  + [dict(skipped=base + ib - 4) for base, ib in W_INS.values()] + [dict(skipped=base - 4) for base, _ in W_INS.values()]
  + [dict(W=S0 + 4), dict(W=S0 - WB + 8), dict(skipped=W0 + WB - 4), dict(skipped=W0 - 4)])
def test_invalid_arguments_of_the_words_call(kw):
    assert _words(**kw) == HIP_ERROR_INVALID_VALUE


@pytest.mark.parametrize("kw", [
    dict(), dict(count=None), dict(skipped=None), dict(V=None), dict(x_bs=0), dict(y_bs=0), dict(v_bs=0), dict(cap=0, keys=None, W=None, X=None, Y=None),
    dict(l_bs=5, w_bs=9), dict(cap=1, w_stride=0, l_bs=1, w_bs=1), dict(n=0, x_stride=0, y_stride=0, W=None, X=None, Y=None, w_stride=0, w_bs=0),
    dict(nx=0, X=None, Y=None), dict(ny=0, X=None, Y=None),           # no pairs: every key is skipped, no row read
    dict(Y=X0, y_bs=4, ny=4),
    dict(count=None, W=N0), dict(V=None, W=V0),
    dict(nx=1 << 20, ny=1 << 20, x_bs=1 << 20, y_bs=1 << 20), dict(n=1024, x_stride=16, x_bs=64, y_stride=16, y_bs=48, w_stride=16, w_bs=80),
] + [dict(W=base + ib) for base, ib in W_INS.values()] + [dict(W=base - WB) for base, _ in W_INS.values()]
  + [dict(skipped=base + ib) for base, ib in W_INS.values()] + [dict(skipped=base - 8) for base, _ in W_INS.values()]
  + [dict(W=S0 + 8), dict(W=S0 - WB), dict(skipped=W0 + WB), dict(skipped=W0 - 8)])
def test_legal_arguments_of_the_words_call(kw):
    assert _words(**dict(kw, batch=0)) == 0


@pytest.mark.parametrize("kw", [
    dict(n=1025, x_stride=17, y_stride=17, w_stride=17, w_bs=100), dict(nx=1 << 31), dict(ny=1 << 31), dict(nx=(1 << 20) + 1, ny=1 << 20),
    dict(nx=(1 << 40) + 1, ny=1), dict(nx=1 << 20, ny=(1 << 20) + 1, batch=0),
])
def test_the_words_call_beyond_the_limits(kw):
    assert _words(**kw) == HIP_ERROR_NOT_SUPPORTED


# ---- the Python layer -------------------------------------------------------------------------------------------------------------------

def test_the_wrappers_signatures():
    J, Wd = m4ri_amd.lists_collide_batch_dev, m4ri_amd.lists_words_batch_dev
    assert list(inspect.signature(J).parameters) == ["X", "x_stride", "x_bs", "nx", "Y", "y_stride", "y_bs", "ny", "n", "V", "v_bs", "batch", "cols", "c_bs",
                                                     "ell", "w_min", "w_max", "hist", "lightest", "list", "l_bs", "cap", "count", "stream"]
    assert list(inspect.signature(Wd).parameters) == ["X", "x_stride", "x_bs", "nx", "Y", "y_stride", "y_bs", "ny", "n", "V", "v_bs", "batch", "keys", "l_bs",
                                                      "cap", "count", "W", "w_stride", "w_bs", "skipped", "stream"]
    assert list(inspect.signature(m4ri_amd.plan_lists_collide_batch).parameters) == ["nx", "ny", "n", "ell", "batch"]
    assert list(inspect.signature(m4ri_amd.lists_collide_units).parameters) == ["nx", "ny", "n", "ell", "batch"]
    J(X0, 1, 4, 4, Y0, 1, 3, 3, 64, V0, 1, 0, C0, 3, 3, 0, 64, H0, L0, K0, 6, 5, N0, 0)            # batch = 0: success, nothing touched
    J(X0, 1, 4, 4, Y0, 1, 3, 3, 64, batch=0, list=K0, l_bs=6, cap=5, count=N0)
    J(X0, 1, 4, 4, Y0, 1, 3, 3, 64, batch=0, count=N0)                                          # a filtered count
    with pytest.raises(RuntimeError):
        J(X0, 1, 4, 4, Y0, 1, 3, 3, 64, batch=2)                                                # no output
    with pytest.raises(RuntimeError):
        J(X0, 1, 4, 4, Y0, 1, 3, 3, 64, batch=2, list=K0, l_bs=6, cap=5)                        # a list without a count
    with pytest.raises(RuntimeError):
        J(X0, 1, 4, 4, Y0, 1, 3, 3, 64, 0, 0, 2, 0, 0, 0, 0, -1, H0)                            # w_max is the seventeenth argument
    with pytest.raises(RuntimeError, match="801"):
        J(X0, 1, 4, 4, Y0, 1, 3, 3, 1025, batch=2, count=N0)
    Wd(X0, 1, 4, 4, Y0, 1, 3, 3, 64, V0, 1, 0, K0, 6, 5, N0, W0, 2, 12, S0, 0)
    Wd(X0, 1, 4, 4, Y0, 1, 3, 3, 64, 0, 0, 0, K0, 6, 5, 0, W0, 2, 12)
    with pytest.raises(RuntimeError):
        Wd(X0, 1, 4, 4, Y0, 1, 3, 3, 64, 0, 0, 2, K0, 4, 5, 0, W0, 2, 12)                        # l_bs 4 < cap 5
    with pytest.raises(RuntimeError):
        Wd(X0, 1, 4, 4, Y0, 1, 3, 3, 64, 0, 0, 2, K0, 6, 5, 0, W0, 2, 12, skipped=W0 + 8)        # skipped inside W
    with pytest.raises(RuntimeError, match="801"):
        Wd(X0, 1, 4, 1 << 31, Y0, 1, 3, 3, 64, 0, 0, 2, K0, 6, 5, 0, W0, 2, 12)
    assert m4ri_amd.plan_lists_collide_batch(4, 3, 64, 3, 2) == 0 and m4ri_amd.lists_collide_units(4, 3, 64, 3, 2) == (C, 1, 1)
