"""The host side of m4ri_amd_row_sums_collide_list_batch_dev and m4ri_amd_row_sums_words_batch_dev, without a GPU: the NumPy rule of
tests/collide_list_cases.py against brute force on the hand-checked member of tests/test_row_sums_collide_plan.py, the argument checks of
both calls (they run before any HIP call) and the argument order of the Python wrappers."""
from math import comb

import numpy as np
import pytest

import collide_cases as cc
import collide_list_cases as cl
import m4ri_amd
from m4ri_amd.mzd import Mzd

HIP_ERROR_INVALID_VALUE, HIP_ERROR_NOT_SUPPORTED = 1, 801

HAND = np.array([[1, 0, 1, 1, 0, 0],
                 [0, 1, 1, 0, 1, 0],
                 [1, 0, 0, 1, 1, 1],
                 [0, 1, 1, 0, 0, 1]], dtype=np.uint8)


# ---- the NumPy rule ---------------------------------------------------------------------------------------------------------------------

def test_a_hand_checked_member():
    """k1 = 2, t1 = t2 = 1, the window columns 1 and 0.  The four pairs by rank: rows 0 + 2 = 001011 (collides, weight 3), 0 + 3 = 110101,
    1 + 2 = 111101 (no collision), 1 + 3 = 000011 (collides, weight 2)."""
    E = lambda w_min, w_max, cols=(1, 0), V=None: (lambda k, c: (k.tolist(), c))(*cl.expect(HAND, V, 2, 1, 1, list(cols), w_min, w_max))
    assert E(0, 6) == ([(2 << 40) | 3, (3 << 40) | 0], 2)
    assert E(0, 1000) == E(0, 6) and E(2, 3) == E(0, 6)
    assert E(3, 3) == ([3 << 40], 1) and E(2, 2) == ([(2 << 40) | 3], 1) and E(0, 1) == ([], 0) and E(4, 6) == ([], 0) and E(3, 2) == ([], 0)
    assert E(0, 6, cols=()) == ([(2 << 40) | 3, (3 << 40) | 0, (4 << 40) | 1, (5 << 40) | 2], 4)      # no window: every pair
    v = np.array([0, 0, 0, 0, 1, 0], dtype=np.uint8)                                           # 001001 (rank 0) and 000001 (rank 3)
    assert E(0, 6, V=v) == ([(1 << 40) | 3, (2 << 40) | 0], 2) and E(2, 6, V=v) == ([2 << 40], 1)
    for cols in ([6], [-1], [0, 1, 6]):
        assert E(0, 6, cols=cols) == ([], -1)
    W = cl.words_of(HAND, None, 2, 1, 1, [0, 1, 2, 3])
    assert ["".join(map(str, r)) for r in W] == ["001011", "110101", "111101", "000011"]
    assert ["".join(map(str, r)) for r in cl.words_of(HAND, v, 2, 1, 1, [3, 0])] == ["000001", "001001"]
    assert ["".join(map(str, r)) for r in cl.words_of(HAND, None, 4, 2, 0, [0, 5])] == ["110110", "111110"]      # rows {0, 1} and {2, 3}


@pytest.mark.parametrize("k,n,k1,t1,t2,ell", [(9, 40, 4, 2, 2, 3), (10, 70, 5, 3, 2, 4), (8, 30, 8, 2, 0, 0), (8, 30, 0, 0, 2, 2), (12, 65, 7, 2, 3, 5)])
def test_the_rule_against_brute_force(k, n, k1, t1, t2, ell):
    """Every pair taken, the word made from the rows of row_pair_unrank: the keys, the count and the words of the helper."""
    G, V = Mzd.random(k, n, k + n).to_bits(), Mzd.random(1, n, 3).to_bits()[0]
    cols = [int(c) for c in np.random.default_rng(k).permutation(n)[:ell]]
    n1, n2 = comb(k1, t1), comb(k - k1, t2)
    words, keys = [], []
    for r in range(n1 * n2):
        S1, S2 = m4ri_amd.row_pair_unrank(r, k1, k, t1, t2)
        c = V.copy()
        for i in S1 + S2:
            c ^= G[i]
        words.append(c)
        if not c[cols].any():
            keys.append((int(c.sum()) << 40) | r)
    assert np.array_equal(cl.words_of(G, V, k1, t1, t2, range(n1 * n2)), np.array(words))
    weights = sorted({x >> 40 for x in keys})
    for w_min, w_max in [(0, n), (0, 2 * n), (weights[0], weights[0]), (weights[1], weights[-2]), (weights[-1] + 1, n), (5, 4)]:
        got, count = cl.expect(G, V, k1, t1, t2, cols, w_min, w_max)
        want = sorted(x for x in keys if w_min <= x >> 40 <= w_max)
        assert got.tolist() == want and count == len(want)
    assert len(keys) >= 2


# ---- the argument checks of the list call -----------------------------------------------------------------------------------------------
# The operands of tests/test_row_sums_collide_plan.py: G two members of 4 x 64 (8 words) at G0, V two words at V0, two windows of three
# entries at C0, hist (2 * 65 entries) at H0, lightest (2) at L0; the list, two members of cap = 5 keys l_bs = 6 apart (88 bytes), at
# K0, count (2 entries) at N0.
G0, V0, C0, H0, L0, K0, N0 = 1 << 20, 1 << 24, 1 << 26, 1 << 28, 1 << 29, 1 << 30, 1 << 31
HB, KB = 2 * 65 * 8, (6 + 5) * 8


def _list(G=G0, g_stride=1, g_bs=4, k=4, n=64, V=V0, v_bs=1, batch=2, k1=2, t1=1, t2=1, cols=C0, c_bs=3, ell=3, w_min=0, w_max=64, hist=H0, lightest=L0,
          lst=K0, l_bs=6, cap=5, count=N0):
    return m4ri_amd.lib().m4ri_amd_row_sums_collide_list_batch_dev(G, g_stride, g_bs, k, n, V, v_bs, batch, k1, t1, t2, cols, c_bs, ell, w_min, w_max, hist,
                                                                   lightest, lst, l_bs, cap, count, None)


@pytest.mark.parametrize("kw", [
    dict(k=-1), dict(n=-1), dict(batch=-1), dict(g_stride=-1), dict(g_bs=-1), dict(v_bs=-1), dict(w_min=-1), dict(t1=-1), dict(t2=-1), dict(k1=-1),
    dict(c_bs=-1), dict(ell=-1), dict(k1=5), dict(cols=None, n=10, ell=11), dict(g_stride=0), dict(G=None),      # what the existing call refuses
    dict(w_max=-1), dict(cap=-1), dict(l_bs=-1), dict(cap=-1, lst=None, count=None), dict(l_bs=-1, lst=None, count=None),
    dict(l_bs=4), dict(l_bs=0),                                       # l_bs < cap with batch > 1
    dict(count=None), dict(lst=None),                                 # a list without a count, a count without a list at cap > 0
    dict(count=None, cap=0),
    dict(hist=None, lightest=None, lst=None, count=None), dict(hist=None, lightest=None, lst=None, count=None, cap=0),   # no output at all
    dict(lst=G0), dict(lst=G0 + 8 * 7), dict(lst=G0 - KB + 8), dict(count=G0 - 8), dict(count=G0 + 8 * 7),
    dict(lst=V0 + 8), dict(lst=V0 - KB + 8), dict(count=V0 - 8), dict(count=V0 + 8),
    dict(lst=C0 + 16), dict(lst=C0 - KB + 8), dict(count=C0 - 8), dict(count=C0 + 16),
    dict(lst=H0 + HB - 8), dict(lst=H0 - KB + 8), dict(lst=L0 + 8), dict(lst=L0 - KB + 8), dict(lst=N0 + 8), dict(lst=N0 - KB + 8),
    dict(count=H0 + HB - 8), dict(count=H0 - 8), dict(count=L0 + 8), dict(count=L0 - 8), dict(count=K0 + KB - 8), dict(count=K0 - 8),
    dict(hist=L0 - HB + 8), dict(lightest=H0 - 8), dict(hist=G0), dict(lightest=C0 + 16),       # and the old outputs among themselves, as before
    dict(lst=K0, l_bs=100, count=K0 + 8 * 104),                       # members 100 apart: the span ends behind entry 104
    dict(count=N0, lst=N0 + 8, cap=0, hist=N0),                       # hist on count where the list is not given
])
def test_invalid_arguments_of_the_list_call(kw):
    """Rejected before any HIP call: the pointers are not device memory (and this machine may have no GPU at all)."""
    assert _list(**kw) == HIP_ERROR_INVALID_VALUE


@pytest.mark.parametrize("kw", [
    dict(), dict(hist=None), dict(lightest=None), dict(hist=None, lightest=None), dict(lst=None, count=None), dict(lst=None, count=None, cap=0),
    dict(lst=None, cap=0), dict(lst=None, cap=0, hist=None, lightest=None), dict(cap=0), dict(cap=0, l_bs=0), dict(l_bs=5), dict(cap=1 << 50, l_bs=1 << 50),
    dict(w_max=0), dict(w_max=1 << 40), dict(w_min=9, w_max=3), dict(g_bs=0), dict(V=None), dict(cols=None),
    dict(lst=G0 + 8 * 8), dict(lst=G0 - KB), dict(count=G0 - 16), dict(count=G0 + 8 * 8), dict(lst=V0 + 16), dict(lst=V0 - KB), dict(count=V0 + 16),
    dict(lst=C0 + 24), dict(lst=C0 - KB), dict(count=C0 + 24), dict(lst=H0 + HB), dict(lst=H0 - KB), dict(lst=L0 + 16), dict(lst=L0 - KB),
    dict(lst=N0 + 16), dict(lst=N0 - KB), dict(count=K0 + KB), dict(count=K0 - 16),
    dict(lst=K0, l_bs=100, count=K0 + 8 * 105),
    dict(lst=G0, cap=0),                                              # an empty list meets nothing
    dict(k=1024, k1=128, t1=2, t2=2), dict(k=1024, n=1024, g_stride=16, k1=128, t1=2, t2=3),
])
def test_legal_arguments_of_the_list_call(kw):
    """Legal arguments, the accepted neighbours of the overlaps above among them: shown with batch = 0, which returns before any HIP call."""
    assert _list(**dict(kw, batch=0)) == 0


def test_one_member_needs_no_batch_stride():
    assert _list(batch=1, l_bs=0, G=None) == HIP_ERROR_INVALID_VALUE       # reaches the NULL-G check: l_bs < cap is fine with one member
    assert _list(batch=2, l_bs=0, G=None, lst=None, count=None) == HIP_ERROR_INVALID_VALUE      # and without a list l_bs means nothing


@pytest.mark.parametrize("kw", [
    dict(t1=9), dict(t2=9, batch=0), dict(ell=65, c_bs=65), dict(n=1025, g_stride=17), dict(k=1025), dict(k=1024, k1=512, t1=2, t2=2),
    dict(k=200, k1=129, t1=2, t2=1), dict(k=1024, k1=24, t1=3, t2=4), dict(k=1025, lst=None, cap=0),
])
def test_the_list_call_beyond_the_limits(kw):
    assert _list(**kw) == HIP_ERROR_NOT_SUPPORTED


def test_negative_sizes_come_before_the_limits():
    assert _list(k=1025, cap=-1) == HIP_ERROR_INVALID_VALUE and _list(t1=9, w_max=-1) == HIP_ERROR_INVALID_VALUE
    assert _list(ell=65, l_bs=-1) == HIP_ERROR_INVALID_VALUE and _words(k=1025, cap=-1) == HIP_ERROR_INVALID_VALUE


def test_the_existing_call_refuses_what_it_refused():
    """The shared launcher does not let the list's arguments leak into the old entry point."""
    old = m4ri_amd.lib().m4ri_amd_row_sums_collide_batch_dev
    assert old(G0, 1, 4, 4, 64, V0, 1, 2, 2, 1, 1, C0, 3, 3, 0, None, None, None) == HIP_ERROR_INVALID_VALUE
    assert old(G0, 1, 4, 4, 64, V0, 1, 0, 2, 1, 1, C0, 3, 3, 0, H0, L0, None) == 0


# ---- the argument checks of the words call ----------------------------------------------------------------------------------------------
# G, V as above; keys two members of cap = 5, l_bs = 6 apart at K0; count at N0; W two members of 5 rows of one word, rows 2 words apart,
# members 12 apart: 12 + 8 + 1 = 21 words at W0; skipped (2 int32) at S0.
W0, S0 = 1 << 32, 1 << 33
WB = 21 * 8


def _words(G=G0, g_stride=1, g_bs=4, k=4, n=64, V=V0, v_bs=1, batch=2, k1=2, t1=1, t2=1, keys=K0, l_bs=6, cap=5, count=N0, W=W0, w_stride=2, w_bs=12,
           skipped=S0):
    return m4ri_amd.lib().m4ri_amd_row_sums_words_batch_dev(G, g_stride, g_bs, k, n, V, v_bs, batch, k1, t1, t2, keys, l_bs, cap, count, W, w_stride, w_bs,
                                                            skipped, None)


@pytest.mark.parametrize("kw", [
    dict(k=-1), dict(n=-1), dict(batch=-1), dict(g_stride=-1), dict(g_bs=-1), dict(v_bs=-1), dict(k1=-1), dict(t1=-1), dict(t2=-1), dict(l_bs=-1),
    dict(cap=-1), dict(w_stride=-1), dict(w_bs=-1), dict(k1=5),
    dict(g_stride=0), dict(n=65, g_bs=8, w_stride=2),                 # g_stride below words(n) with k > 1
    dict(w_stride=0), dict(n=129, g_stride=3, g_bs=12, w_stride=2, w_bs=20),      # w_stride below words(n) with cap > 1
    dict(l_bs=4), dict(w_bs=8), dict(w_bs=0),                         # too small for cap keys / cap rows with batch > 1
    dict(keys=None), dict(W=None), dict(G=None), dict(G=None, t2=0), dict(G=None, t1=0),
    dict(W=G0), dict(W=G0 + 8 * 7), dict(W=G0 - WB + 8), dict(W=V0 + 8), dict(W=V0 - WB + 8), dict(W=K0 + KB - 8), dict(W=K0 - WB + 8), dict(W=N0 + 8),
    dict(W=N0 - WB + 8), dict(W=S0 + 4), dict(W=S0 - WB + 8),
    dict(skipped=G0 - 4), dict(skipped=G0 + 8 * 7 + 4), dict(skipped=V0 + 12), dict(skipped=K0 + KB - 4), dict(skipped=K0 - 4), dict(skipped=N0 + 12),
    dict(skipped=N0 - 4), dict(skipped=W0 + WB - 4), dict(skipped=W0 - 4),
])
def test_invalid_arguments_of_the_words_call(kw):
    assert _words(**kw) == HIP_ERROR_INVALID_VALUE


@pytest.mark.parametrize("kw", [
    dict(), dict(count=None), dict(skipped=None), dict(V=None), dict(g_bs=0), dict(v_bs=0), dict(cap=0, keys=None, W=None, G=None), dict(l_bs=5, w_bs=9),
    dict(cap=1, w_stride=0, l_bs=1, w_bs=1), dict(n=0, g_stride=0, W=None, G=None, w_stride=0, w_bs=0), dict(k1=4, t1=2, t2=0), dict(t1=0, t2=0, G=None),
    dict(t1=3, G=None),                                               # no pairs: every key is skipped, no row of G read
    dict(W=G0 + 8 * 8), dict(W=G0 - WB), dict(W=V0 + 16), dict(W=K0 + KB), dict(W=K0 - WB), dict(W=N0 + 16), dict(W=S0 + 8), dict(W=S0 - WB),
    dict(skipped=G0 - 8), dict(skipped=G0 + 8 * 8), dict(skipped=W0 + WB), dict(skipped=W0 - 8), dict(skipped=N0 + 16), dict(skipped=K0 + KB),
    dict(count=None, W=N0), dict(V=None, W=V0),
    dict(k=1024, k1=512, t1=2, t2=2),                                 # no bound on N1: C(512, 2)^2 = 1.7e10 pairs
    dict(k=1024, k1=1024, t1=4, t2=0), dict(k=1024, n=1024, g_stride=16, g_bs=1 << 14, w_stride=16, w_bs=80),
])
def test_legal_arguments_of_the_words_call(kw):
    assert _words(**dict(kw, batch=0)) == 0


@pytest.mark.parametrize("kw", [
    dict(t1=9), dict(t2=9, batch=0), dict(n=1025, g_stride=17, w_stride=17, w_bs=100), dict(k=1025), dict(k=1024, k1=1024, t1=5, t2=0),
    dict(k=1024, k1=512, t1=3, t2=3), dict(k=1024, k1=24, t1=3, t2=4),
])
def test_the_words_call_beyond_the_limits(kw):
    assert _words(**kw) == HIP_ERROR_NOT_SUPPORTED


def test_the_edge_of_the_pair_limit():
    """N1 * N2 <= 2^40, whatever N1 is: C(1024, 4) = 4.6e10 fits, and so does the largest k2 against N1 = C(512, 2) = 130 816."""
    assert comb(1024, 4) <= 1 << 40 < comb(1024, 5)
    n1 = comb(512, 2)
    k2 = max(x for x in range(3, 513) if n1 * comb(x, 3) <= 1 << 40)
    assert k2 < 512 and _words(k=512 + k2, k1=512, t1=2, t2=3, batch=0) == 0
    assert _words(k=512 + k2 + 1, k1=512, t1=2, t2=3, batch=0) == HIP_ERROR_NOT_SUPPORTED


# ---- the Python layer -------------------------------------------------------------------------------------------------------------------

def test_python_wrappers_are_bound():
    L, Wd = m4ri_amd.row_sums_collide_list_batch_dev, m4ri_amd.row_sums_words_batch_dev
    L(G0, 1, 4, 4, 64, V0, 1, 0, 2, 1, 1, C0, 3, 3, 0, 64, H0, L0, K0, 6, 5, N0, 0)            # batch = 0: success, nothing touched
    L(G0, 1, 4, 4, 64, 0, 0, 0, 2, 1, 1, list=K0, l_bs=6, cap=5, count=N0)
    L(G0, 1, 4, 4, 64, 0, 0, 0, 2, 1, 1, count=N0)                                          # a filtered count
    with pytest.raises(RuntimeError):
        L(G0, 1, 4, 4, 64, 0, 0, 2, 2, 1, 1)                                                # no output
    with pytest.raises(RuntimeError):
        L(G0, 1, 4, 4, 64, 0, 0, 2, 2, 1, 1, list=K0, l_bs=6, cap=5)                        # a list without a count
    with pytest.raises(RuntimeError):
        L(G0, 1, 4, 4, 64, 0, 0, 2, 2, 1, 1, list=K0, l_bs=4, cap=5, count=N0)              # positional l_bs, cap: 4 < 5
    with pytest.raises(RuntimeError):
        L(G0, 1, 4, 4, 64, 0, 0, 2, 2, 1, 1, 0, 0, 0, 0, -1, H0)                            # w_max is the sixteenth argument
    with pytest.raises(RuntimeError, match="801"):
        L(G0, 1, 4, 400, 64, 0, 0, 2, 129, 2, 1, count=N0)
    Wd(G0, 1, 4, 4, 64, V0, 1, 0, 2, 1, 1, K0, 6, 5, N0, W0, 2, 12, S0, 0)
    Wd(G0, 1, 4, 4, 64, 0, 0, 0, 2, 1, 1, K0, 6, 5, 0, W0, 2, 12)
    with pytest.raises(RuntimeError):
        Wd(G0, 1, 4, 4, 64, 0, 0, 2, 2, 1, 1, K0, 4, 5, 0, W0, 2, 12)                        # l_bs 4 < cap 5
    with pytest.raises(RuntimeError):
        Wd(G0, 1, 4, 4, 64, 0, 0, 2, 2, 1, 1, K0, 6, 5, 0, W0, 2, 8)                         # w_bs 8 < 4 * 2 + 1
    with pytest.raises(RuntimeError):
        Wd(G0, 1, 4, 4, 64, 0, 0, 2, 2, 1, 1, 0, 6, 5, 0, W0, 2, 12)                         # no keys
    with pytest.raises(RuntimeError):
        Wd(G0, 1, 4, 4, 64, 0, 0, 2, 2, 1, 1, K0, 6, 5, 0, W0, 2, 12, skipped=W0 + 8)        # skipped inside W
    with pytest.raises(RuntimeError, match="801"):
        Wd(G0, 1, 4, 1024, 64, 0, 0, 2, 1024, 5, 0, K0, 6, 5, 0, W0, 2, 12)
