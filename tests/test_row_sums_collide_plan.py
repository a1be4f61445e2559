"""The host side of m4ri_amd_row_sums_collide_batch_dev, without a GPU: the NumPy expectations of tests/collide_cases.py against each
other (the join against brute force), against tests/rowsums_cases.py, a hand-checked member and the closed forms; the pair ranks of
the Python layer; the path boundary of m4ri_amd_plan_row_sums_collide_batch, the slices of m4ri_amd_row_sums_collide_slices and the
argument checks, which run before any HIP call."""
from math import comb

import numpy as np
import pytest

import collide_cases as cc
import m4ri_amd
import rowsums_cases as rc
from m4ri_amd.mzd import Mzd

HIP_ERROR_INVALID_VALUE, HIP_ERROR_NOT_SUPPORTED = 1, 801
PATH0 = "M4RI_AMD_ROW_SUMS_COLLIDE_PATH0_MAX"
P0 = 33205536  # rowsums_collide_batch.hip's RC_P0 = C(64, 2) * C(182, 2): path 0 up to this many pairs per member, the measured bound


def _bits(rows, cols, seed):
    return Mzd.random(rows, cols, seed).to_bits()


# ---- the NumPy expectations -------------------------------------------------------------------------------------------------------------

HAND = np.array([[1, 0, 1, 1, 0, 0],
                 [0, 1, 1, 0, 1, 0],
                 [1, 0, 0, 1, 1, 1],
                 [0, 1, 1, 0, 0, 1]], dtype=np.uint8)


def test_a_hand_checked_member():
    """k1 = 2, t1 = t2 = 1, the window columns 1 and 0.  The four pairs by rank: rows 0 + 2 = 001011 (collides, weight 3), 0 + 3 = 110101,
    1 + 2 = 111101 (column 1 or 0 set: no collision), 1 + 3 = 000011 (collides, weight 2)."""
    w, r, hit = cc.brute(HAND, None, 2, 1, 1, [1, 0])
    assert w.tolist() == [3, 4, 5, 2] and r.tolist() == [0, 1, 2, 3] and hit.tolist() == [True, False, False, True]
    h, light = cc.expect(HAND, None, 2, 1, 1, [1, 0], 0)
    assert h.tolist() == [0, 0, 1, 1, 0, 0, 0] and light == (2 << 40) | 3
    assert cc.expect(HAND, None, 2, 1, 1, [1, 0], 3)[1] == 3 << 40 and cc.expect(HAND, None, 2, 1, 1, [1, 0], 4)[1] == -1
    # V = 000010 turns the two colliding words into 001001 (rank 0) and 000001 (rank 3); V = 010000 makes 0 + 3 and 1 + 2 the colliding ones
    v = np.array([0, 0, 0, 0, 1, 0], dtype=np.uint8)
    h, light = cc.expect(HAND, v, 2, 1, 1, [1, 0], 0)
    assert h.tolist() == [0, 1, 1, 0, 0, 0, 0] and light == (1 << 40) | 3 and cc.expect(HAND, v, 2, 1, 1, [1, 0], 2)[1] == 2 << 40
    v = np.array([0, 1, 0, 0, 0, 0], dtype=np.uint8)
    assert cc.brute(HAND, v, 2, 1, 1, [1])[2].tolist() == [False, True, True, False]
    assert cc.brute(HAND, v, 2, 1, 1, [1, 0])[2].tolist() == [False, False, False, False]     # both have column 0 set
    assert cc.expect(HAND, v, 2, 1, 1, [1, 1], 0)[1] == (3 << 40) | 1                         # 0 + 3 + V = 100101; a repeated column
    assert m4ri_amd.row_pair_unrank(3, 2, 4, 1, 1) == ((1,), (3,)) and m4ri_amd.row_pair_unrank(0, 2, 4, 1, 1) == ((0,), (2,))
    for cols in ([6], [-1], [0, 1, 6], [2, -5, 1]):
        h, light = cc.expect(HAND, None, 2, 1, 1, cols, 0)
        assert h.tolist() == [-1] * 7 and light == -2


LADDER = [(4, 6, 2, 1, 1, 2), (6, 20, 3, 2, 1, 3), (9, 40, 4, 2, 2, 4), (10, 70, 5, 3, 2, 5), (12, 65, 7, 2, 3, 6), (13, 33, 6, 1, 4, 3),
          (8, 30, 0, 0, 2, 2), (8, 30, 8, 2, 0, 2), (8, 30, 3, 0, 0, 1), (8, 30, 3, 4, 1, 1), (8, 30, 3, 1, 6, 1), (14, 64, 7, 3, 3, 0),
          (14, 64, 7, 3, 3, 1), (11, 130, 5, 2, 2, 64), (16, 24, 8, 2, 2, 9)]


@pytest.mark.parametrize("k,n,k1,t1,t2,ell", LADDER)
def test_the_join_agrees_with_brute_force(k, n, k1, t1, t2, ell):
    rng = np.random.default_rng(k * n + ell)
    G = _bits(k, n, k + n)
    G[:, : n // 3] &= (rng.random((k, n // 3)) < 0.3).astype(np.uint8)     # sparse columns: collisions on wide windows too
    for V in (None, _bits(1, n, 5)[0] & G[0]):
        for cols in (list(range(ell)), [int(c) for c in rng.integers(0, n, size=ell)], [int(c) for c in rng.integers(0, max(n // 3, 1), size=ell)]):
            w, r, hit = cc.brute(G, V, k1, t1, t2, cols)
            assert len(w) == comb(k1, t1) * comb(k - k1, t2)
            jw, jr = cc.joined(G, V, k1, t1, t2, cols)
            order = np.argsort(jr)
            assert np.array_equal(jr[order], r[hit]) and np.array_equal(jw[order], w[hit]), (cols, V is None)
            if ell == 0:
                assert hit.all()


def test_without_window_and_right_half_it_is_the_row_sums():
    """ell = 0, t2 = 0, k1 = k: every pair collides, N2 = 1, the pair rank is r1: rowsums_cases.expect exactly, ranks included."""
    for k, n, t in [(7, 20, 0), (7, 20, 1), (7, 20, 3), (9, 65, 2), (6, 10, 6), (6, 10, 7)]:
        G, V = _bits(k, n, k + t), _bits(1, n, t)[0]
        for w_min in (0, 1, n // 2):
            for v in (None, V):
                h, light = cc.expect(G, v, k, t, 0, [], w_min)
                wh, wl = rc.expect(G, v, t, w_min) if k >= t else (np.zeros(n + 1, dtype=np.int64), -1)
                assert np.array_equal(h, wh) and light == wl, (k, n, t, w_min)
                jw, jr = cc.joined(G, v, k, t, 0, [])
                assert np.array_equal(rc.hist_of(jw, n), wh) and rc.lightest_of(jw, jr, w_min) == wl
    # the halves together make up the sets of t rows: over t1 + t2 = t the collision-free counts add up to C(k, t)
    G = _bits(9, 30, 1)
    total = sum(cc.expect(G, None, 4, t1, 3 - t1, [], 0)[0] for t1 in range(4))
    assert np.array_equal(total, rc.expect(G, None, 3, 0)[0])


def test_closed_forms():
    for k, z, k1, t1, t2, cols in [(8, 3, 4, 2, 2, [16, 18]), (8, 3, 4, 2, 2, [17, 1, 13]), (7, 1, 3, 1, 2, [0, 7]), (6, 2, 3, 2, 1, [12, 13, 12]),
                                   (6, 2, 3, 3, 1, [1]), (6, 2, 3, 1, 1, [])]:
        G = cc.doubled_identity_zeros(k, z)
        for w_min in (0, 2 * (t1 + t2), 2 * (t1 + t2) + 1):
            h, light = cc.expect(G, None, k1, t1, t2, cols, w_min)
            wh, wl = cc.doubled_identity_expect(k, z, k1, t1, t2, cols, w_min)
            assert np.array_equal(h, wh) and light == wl, (k, cols, w_min)
    for k, (a, b, c), k1, t1, t2 in [(10, (1, 3, 7), 5, 2, 1), (10, (4, 0, 5), 5, 2, 2), (12, (2, 5, 11), 6, 3, 2), (9, (0, 1, 8), 4, 1, 1),
                                     (9, (3, 2, 6), 4, 2, 0)]:
        G = rc.rigged(k, a, b, c)
        for w_min in (0, 1, 2 * (t1 + t2) - 2, 2 * (t1 + t2) + 1):
            h, light = cc.expect(G, None, k1, t1, t2, cc.rigged_window(k, a, b), w_min)
            wh, wl = cc.rigged_expect(k, a, b, c, k1, t1, t2, w_min)
            assert np.array_equal(h, wh) and light == wl, (k, a, b, c, t1, t2, w_min)


# ---- the Python layer's ranks -----------------------------------------------------------------------------------------------------------

def test_row_pair_ranks_round_trip():
    for k1, k, t1, t2 in [(2, 4, 1, 1), (5, 12, 2, 3), (0, 6, 0, 2), (6, 6, 3, 0), (4, 9, 0, 0), (3, 10, 3, 1)]:
        n1, n2 = comb(k1, t1), comb(k - k1, t2)
        left, right = cc.subsets(k1, t1), cc.subsets(k - k1, t2) + k1
        for r in range(n1 * n2):
            S1, S2 = m4ri_amd.row_pair_unrank(r, k1, k, t1, t2)
            assert S1 == tuple(left[r // n2]) and S2 == tuple(right[r % n2])
            assert m4ri_amd.row_pair_rank(S1, S2, k1, k, t2) == cc.pair_rank(S1, S2, k1, k, t2) == r
            assert m4ri_amd.row_pair_rank(reversed(S1), reversed(S2), k1, k, t2) == r    # any order
        with pytest.raises(ValueError):
            m4ri_amd.row_pair_unrank(n1 * n2, k1, k, t1, t2)
    S1, S2 = (126, 127), (1020, 1021, 1022, 1023)
    r = m4ri_amd.row_pair_rank(S1, S2, 128, 1024, 4)
    assert r == (comb(128, 2) - 1) * comb(896, 4) + comb(896, 4) - 1 and m4ri_amd.row_pair_unrank(r, 128, 1024, 2, 4) == (S1, S2)
    for bad in [((0, 5), (6,), 5, 8, 1), ((0,), (3,), 4, 8, 1), ((0,), (5, 6), 4, 8, 1), ((1, 1), (5,), 4, 8, 1), ((0,), (8,), 4, 8, 1)]:
        with pytest.raises(ValueError):
            m4ri_amd.row_pair_rank(*bad)
    with pytest.raises(ValueError):
        m4ri_amd.row_pair_unrank(-1, 2, 4, 1, 1)
    with pytest.raises(ValueError):
        m4ri_amd.row_pair_unrank(0, 5, 4, 1, 1)


# ---- the plan ---------------------------------------------------------------------------------------------------------------------------

def _pairs(k, k1, t1, t2):
    return comb(k1, t1) * comb(k - k1, t2)


def test_path_boundary():
    P = m4ri_amd.plan_row_sums_collide_batch
    assert 1 <= P0 <= (1 << 32) - 1
    seen = set()
    for n in (1, 64, 1024):
        for ell in (0, 1, 16, 64):     # ONE boundary in the number of pairs, whatever n > 0 and the window
            for k, k1, t1, t2 in [(k, k // 2, t1, t2) for k in (8, 20, 64, 90, 128, 200, 256, 512, 1024) for t1 in range(4) for t2 in range(4)] + \
                    [(1024, 128, 2, 2), (1024, 1, 1, 4), (600, 100, 2, 3), (300, 20, 3, 2)]:
                want = 0 if _pairs(k, k1, t1, t2) <= P0 else 1
                assert P(k, n, k1, t1, t2, ell) == want, (k, n, k1, t1, t2, ell)
                seen.add(want)
    assert seen == {0, 1}
    # the measured shape itself and the next one: C(64, 2) * C(182, 2) = P0 and C(64, 2) * C(183, 2); the rung where path 0 was measured to lose
    assert _pairs(246, 64, 2, 2) == P0 and _pairs(247, 64, 2, 2) > P0 + 1
    assert (P(246, 256, 64, 2, 2, 16), P(247, 256, 64, 2, 2, 16), P(320, 256, 64, 2, 2, 16), P(246, 256, 182, 2, 2, 0)) == (0, 1, 1, 0)
    for s in [(0, 0, 0, 0, 0, 0), (1024, 0, 512, 2, 2, 0), (1024, 0, 512, 2, 2, 5), (64, 64, 2, 3, 1, 8), (64, 64, 62, 1, 3, 8),
              (64, 64, 0, 1, 2, 8), (1024, 1024, 512, 0, 0, 64)]:     # no columns, no pairs, one pair
        assert P(*s) == 0, s
    for s in [(1024, 1, 512, 2, 2, 0), (1024, 1024, 512, 8, 8, 64), (2000, 64, 1000, 3, 3, 100), (1024, 64, 129, 2, 2, 8)]:   # beyond the limits: the same rule
        assert P(*s) == 1, s


def test_plan_ignores_the_override_variable(monkeypatch):
    P = m4ri_amd.plan_row_sums_collide_batch
    for v in ("-1", "0", "5", "4294967295", "1000000000000", "junk", "-7"):
        monkeypatch.setenv(PATH0, v)
        assert (P(8, 64, 4, 2, 2, 4), P(1024, 64, 128, 2, 2, 16), P(4, 64, 2, 3, 1, 1), P(246, 64, 64, 2, 2, 8), P(247, 64, 64, 2, 2, 8)) == (0, 1, 0, 0, 1), v
    monkeypatch.delenv(PATH0)


def test_negative_sizes():
    P, S = m4ri_amd.plan_row_sums_collide_batch, m4ri_amd.row_sums_collide_slices
    good = (8, 64, 4, 2, 2, 4)
    assert P(*good) == 0
    for i in range(6):
        bad = list(good)
        bad[i] = -1
        assert P(*bad) == -1 and S(*bad, 1) == -1, bad
    assert P(8, 64, 9, 2, 2, 4) == -1 and S(8, 64, 9, 2, 2, 4, 1) == -1      # k1 > k: a negative k2
    assert S(*good, -1) == -1


def test_slices():
    """Slices of at least max(N1, 256) right sums, as many as bring the call to 1024 workgroups, a slice times N1 below 2^32."""
    S = m4ri_amd.row_sums_collide_slices
    assert S(8, 64, 4, 2, 2, 4, 1) == 1                                     # N2 = 6: one short slice
    assert S(44, 64, 4, 2, 2, 4, 2) == 4 and comb(40, 2) == 780 == 3 * 256 + 12          # slices of 256, a ragged last one
    assert S(44, 64, 4, 2, 2, 4, 1024) == 1 and S(44, 64, 4, 2, 2, 4, 0) == 4
    assert S(152, 256, 128, 2, 2, 10, 1) == 1 and comb(24, 2) < comb(128, 2)             # never shorter than N1 unless the list is
    assert S(328, 256, 128, 2, 2, 10, 1) == -(-comb(200, 2) // 8128)                       # N1 = 8128 long
    assert S(1024, 64, 2, 1, 3, 8, 1) == 1024 and S(1024, 64, 2, 1, 3, 8, 512) == 2 and S(1024, 64, 2, 1, 3, 8, 4096) == 1
    # a slice times N1 stays below 2^32: N1 = 8128, N2 = C(896, 3) = 1.2e8 at batch 4096 would be one slice of 9.7e11 pairs
    n1, n2 = comb(128, 2), comb(896, 3)
    cap = ((1 << 32) - 1) // n1
    assert S(1024, 64, 128, 2, 3, 8, 4096) == -(-n2 // cap) and cap * n1 < 1 << 32 and n1 * n2 <= 1 << 40
    for s in [(8, 0, 4, 2, 2, 0, 1), (8, 64, 4, 5, 2, 4, 1), (8, 64, 4, 2, 5, 4, 1), (400, 64, 129, 2, 2, 4, 1)]:   # no columns, no pairs, N1 > 8192
        assert S(*s) == 0, s


# ---- the argument checks ----------------------------------------------------------------------------------------------------------------
# G: 2 members of 4 x 64 (4 words each, 8 words in all) at G0, V: 2 words at V0, cols: 2 windows of 3 entries (24 bytes) at C0; hist
# (2 * 65 entries, 1040 bytes) at H0 and lightest (2 entries) at L0, far away.
G0, V0, C0, H0, L0 = 1 << 20, 1 << 24, 1 << 26, 1 << 28, 1 << 29
HB = 2 * 65 * 8


def _call(G=G0, g_stride=1, g_bs=4, k=4, n=64, V=V0, v_bs=1, batch=2, k1=2, t1=1, t2=1, cols=C0, c_bs=3, ell=3, w_min=0, hist=H0, lightest=L0):
    return m4ri_amd.lib().m4ri_amd_row_sums_collide_batch_dev(G, g_stride, g_bs, k, n, V, v_bs, batch, k1, t1, t2, cols, c_bs, ell, w_min, hist,
                                                              lightest, None)


@pytest.mark.parametrize("kw", [
    dict(k=-1), dict(n=-1), dict(batch=-1), dict(g_stride=-1), dict(g_bs=-1), dict(v_bs=-1), dict(w_min=-1), dict(t1=-1), dict(t2=-1),
    dict(k1=-1), dict(c_bs=-1), dict(ell=-1), dict(V=None, v_bs=-1), dict(cols=None, c_bs=-1),
    dict(k1=5),                                              # k1 > k
    dict(cols=None, n=10, ell=11), dict(cols=None, n=2, ell=3),   # no window given and more columns asked for than there are
    dict(cols=None, n=0, ell=1, g_stride=0),
    dict(g_stride=0),                                        # below words(64) = 1 with k > 1
    dict(n=65, g_stride=1, g_bs=8),                          # g_stride 1 < words(65) = 2
    dict(G=None), dict(G=None, t2=0), dict(G=None, t1=0), dict(G=None, t1=2, t2=2),   # a NULL G where rows are read
    dict(hist=None, lightest=None),                          # no output at all
    dict(hist=G0), dict(hist=G0 + 8 * 7),                    # hist[0] on G's first / last word
    dict(hist=G0 - HB + 8),                                  # hist's last entry is G's first word
    dict(lightest=G0 - 8), dict(lightest=G0 + 8 * 7),
    dict(hist=G0 + 8 * 3, g_bs=0), dict(lightest=G0 + 8 * 3, g_bs=0),   # one shared G: its span is one member
    dict(hist=V0 + 8), dict(hist=V0 - HB + 8), dict(lightest=V0 - 8), dict(lightest=V0 + 8),
    dict(lightest=V0, v_bs=0), dict(hist=V0, v_bs=0),        # one shared V: one word
    dict(hist=C0), dict(hist=C0 + 16), dict(hist=C0 - HB + 8), dict(lightest=C0 - 8), dict(lightest=C0 + 16),   # the windows: 24 bytes
    dict(lightest=C0 + 8, c_bs=0), dict(hist=C0 + 8, c_bs=0),   # one shared window: 12 bytes
    dict(hist=C0 + 32, c_bs=8),                              # windows 8 entries apart: 44 bytes
    dict(hist=L0 - HB + 8), dict(hist=L0 + 8),               # hist's last entry on lightest[0]; hist[0] on lightest[1]
    dict(lightest=H0 + HB - 8), dict(lightest=H0 - 8),
    dict(hist=G0, t1=0, t2=0), dict(hist=G0, t1=3),          # G is not read then, but its span is still no place for an output
])
def test_invalid_arguments(kw):
    """Rejected before any HIP call: the pointers are not device memory (and this machine may have no GPU at all)."""
    assert _call(**kw) == HIP_ERROR_INVALID_VALUE


@pytest.mark.parametrize("kw", [
    dict(), dict(g_bs=0), dict(v_bs=0), dict(c_bs=0), dict(V=None), dict(V=None, v_bs=0), dict(cols=None), dict(cols=None, ell=64),
    dict(cols=None, ell=0), dict(ell=0), dict(ell=64, c_bs=64), dict(w_min=1 << 40), dict(hist=None), dict(lightest=None),
    dict(g_stride=7, g_bs=3),                                                 # g_bs is free: G is only read
    dict(n=65, g_stride=2, g_bs=8), dict(n=2, ell=3),                         # a window beyond n is the device's to refuse
    dict(k=1, k1=1, g_stride=0, t2=0), dict(k=0, k1=0, g_stride=0, G=None, t1=0, t2=0),   # a stride only counts between two rows
    dict(n=0, g_stride=0, G=None, V=None, ell=0), dict(n=0, g_stride=0, G=None, V=None),
    dict(k1=0, t1=0), dict(k1=4, t2=0), dict(k1=0), dict(k1=4), dict(t1=0, t2=0, G=None), dict(t1=3, G=None), dict(t2=8, G=None),
    dict(k=1024, k1=128, t1=2, t2=2), dict(k=1024, n=1024, g_stride=16, k1=128, t1=2, t2=3), dict(k=1024, k1=512, t1=1, t2=3),
    dict(k=1024, k1=1, t1=1, t2=4), dict(k=16, k1=8, t1=8, t2=8), dict(n=1024, g_stride=16),
])
def test_batch_zero_is_success(kw):
    """Legal arguments: shown with batch = 0, which returns before any HIP call."""
    assert _call(**dict(kw, batch=0)) == 0


@pytest.mark.parametrize("kw", [
    dict(hist=G0 + 8 * 8), dict(hist=G0 - HB), dict(lightest=G0 - 16), dict(lightest=G0 + 8 * 8),
    dict(hist=G0 + 8 * 4, g_bs=0), dict(lightest=G0 + 8 * 4, g_bs=0),
    dict(hist=V0 + 16), dict(hist=V0 - HB), dict(lightest=V0 - 16), dict(lightest=V0 + 16),
    dict(lightest=V0 + 8, v_bs=0), dict(hist=V0 + 8, v_bs=0),
    dict(hist=C0 + 24), dict(hist=C0 - HB), dict(lightest=C0 - 16), dict(lightest=C0 + 24), dict(lightest=C0 + 16, c_bs=0),
    dict(hist=C0, ell=0), dict(hist=C0, cols=None),
    dict(hist=L0 - HB), dict(hist=L0 + 16), dict(lightest=H0 + HB), dict(lightest=H0 - 16),
    dict(V=None, hist=V0), dict(V=None, lightest=V0),
])
def test_outputs_beside_the_operands_are_accepted(kw):
    """The accepted neighbours of the overlaps above, one element further out.  Shown with batch = 0, as every legal call is here."""
    assert _call(**dict(kw, batch=0)) == 0


@pytest.mark.parametrize("kw", [
    dict(t1=9), dict(t2=9), dict(t1=9, batch=0), dict(ell=65, c_bs=65), dict(ell=65, batch=0), dict(cols=None, n=128, g_stride=2, ell=65),
    dict(n=1025, g_stride=17), dict(n=1025, g_stride=17, batch=0), dict(k=1025), dict(k=1025, t1=0, t2=0), dict(k=1 << 40),
    dict(n=1 << 40, g_stride=1 << 40), dict(t1=1 << 40), dict(ell=1 << 40),
    dict(k=1024, k1=512, t1=2, t2=2),                       # N1 = C(512, 2) = 130816 > 8192
    dict(k=200, k1=129, t1=2, t2=1), dict(k=200, k1=129, t1=2, t2=0, batch=0),
    dict(k=1024, k1=24, t1=3, t2=4),                        # N1 = 2024, N2 = C(1000, 4) = 4.1e10: 8.4e13 pairs
])
def test_beyond_the_limits_is_not_supported(kw):
    assert _call(**kw) == HIP_ERROR_NOT_SUPPORTED


def test_the_edges_of_the_limits():
    """N1 <= 8192: C(128, 2) = 8128 fits, C(129, 2) = 8256 does not; N1 * N2 <= 2^40, just below and just above."""
    assert comb(128, 2) == 8128 and comb(129, 2) == 8256
    assert _call(k=200, k1=128, t1=2, t2=1, batch=0) == 0 and _call(k=200, k1=129, t1=2, t2=1, batch=0) == HIP_ERROR_NOT_SUPPORTED
    for t1 in range(1, 9):
        k1 = max(x for x in range(t1, 1025) if comb(x, t1) <= 8192)
        assert _call(k=1024, k1=k1, t1=t1, t2=0, batch=0) == 0, (k1, t1)
        if k1 < 1024:
            assert _call(k=1024, k1=k1 + 1, t1=t1, t2=0, batch=0) == HIP_ERROR_NOT_SUPPORTED, (k1 + 1, t1)
    # N1 = C(64, 2) = 2016 leaves k2 up to 960: the largest k2 with 2016 * C(k2, 4) <= 2^40 and the next one
    k2 = max(x for x in range(4, 961) if 2016 * comb(x, 4) <= 1 << 40)
    assert 2016 * comb(k2, 4) <= 1 << 40 < 2016 * comb(k2 + 1, 4) and k2 + 1 <= 960
    assert _call(k=64 + k2, k1=64, t1=2, t2=4, batch=0) == 0 and _call(k=64 + k2 + 1, k1=64, t1=2, t2=4, batch=0) == HIP_ERROR_NOT_SUPPORTED
    # one left row: N2 alone up to 2^40, as the rank of m4ri_amd_row_sums_weights_batch_dev
    assert _call(k=1024, k1=1, t1=1, t2=4, batch=0) == 0 and comb(1023, 4) <= 1 << 40
    assert _call(k=1024, k1=2, t1=1, t2=5, batch=0) == HIP_ERROR_NOT_SUPPORTED


def test_negative_sizes_come_before_the_limits():
    assert _call(k=1025, n=-1) == HIP_ERROR_INVALID_VALUE and _call(k=-1, n=1025) == HIP_ERROR_INVALID_VALUE
    assert _call(t1=9, w_min=-1) == HIP_ERROR_INVALID_VALUE and _call(ell=65, t2=-1) == HIP_ERROR_INVALID_VALUE
    assert _call(k=1024, k1=1025, t1=2) == HIP_ERROR_INVALID_VALUE


def test_python_wrappers_are_bound():
    assert m4ri_amd.plan_row_sums_collide_batch(0, 0, 0, 0, 0, 0) == 0 and m4ri_amd.plan_row_sums_collide_batch(-1, 3, 0, 1, 1, 0) == -1
    assert m4ri_amd.plan_row_sums_collide_batch(1024, 64, 128, 2, 2, 16) == 1
    assert m4ri_amd.row_sums_collide_slices(44, 64, 4, 2, 2, 4, 2) == 4
    with pytest.raises(RuntimeError):
        m4ri_amd.row_sums_collide_batch_dev(G0, 1, 4, 4, 64, 0, 0, 2, 2, 1, 1)                        # no output
    with pytest.raises(RuntimeError):
        m4ri_amd.row_sums_collide_batch_dev(G0, 0, 4, 4, 64, 0, 0, 2, 2, 1, 1, hist=H0)               # G's stride 0 < width 1
    with pytest.raises(RuntimeError, match="801"):
        m4ri_amd.row_sums_collide_batch_dev(G0, 1, 4, 400, 64, 0, 0, 2, 129, 2, 1, hist=H0)           # the left list beyond the table
    m4ri_amd.row_sums_collide_batch_dev(G0, 1, 4, 4, 64, 0, 0, 0, 2, 1, 1, hist=H0)                   # batch = 0: success, nothing touched
    m4ri_amd.row_sums_collide_batch_dev(G0, 1, 4, 4, 64, V0, 1, 0, 2, 1, 1, C0, 3, 3, w_min=1, lightest=L0, stream=0)
    m4ri_amd.row_sums_collide_batch_dev(G0, 1, 0, 4, 64, V0, 0, 0, 2, 1, 1, C0, 0, 3, 0, H0, L0, 0)
