"""The host side of m4ri_amd_row_sums_weights_batch_dev, without a GPU: the NumPy expectations and closed forms of
tests/rowsums_cases.py on hand-checked codes and against tests/rowspace_cases.py, the subset ranks of the Python layer, the path
boundary of m4ri_amd_plan_row_sums_weights_batch and the argument checks, which run before any HIP call."""
from itertools import combinations
from math import comb

import numpy as np
import pytest

import m4ri_amd
import rowspace_cases as rw
import rowsums_cases as rc
from m4ri_amd.mzd import Mzd
from test_rowspace_weights_plan import HAMMING_7_4

HIP_ERROR_INVALID_VALUE, HIP_ERROR_NOT_SUPPORTED = 1, 801
PATH0 = "M4RI_AMD_ROW_SUMS_PATH0_MAX"
M0 = 16471  # rowsums_batch.hip's RS_M0 = C(182, 2): path 0 up to this many sums per member, the measured bound


def test_numpy_expectations_on_hand_checked_cases():
    want = [[1, 0, 0, 0, 0, 0, 0, 0], [0, 0, 0, 3, 1, 0, 0, 0], [0, 0, 0, 3, 3, 0, 0, 0], [0, 0, 0, 1, 3, 0, 0, 0], [0, 0, 0, 0, 0, 0, 0, 1]]
    for t in range(5):
        assert rc.expect(HAMMING_7_4, None, t, 0)[0].tolist() == want[t], t
    assert rc.expect(HAMMING_7_4, None, 2, 1)[1] == (3 << 40) | 3 and rc.unrank(3, 2) == (0, 3)   # rows 0 + 3 = 1001001
    assert rc.expect(HAMMING_7_4, None, 1, 1)[1] == 3 << 40                                     # row 0 weighs 3
    assert rc.expect(HAMMING_7_4, None, 0, 0)[1] == 0 and rc.expect(HAMMING_7_4, None, 0, 1)[1] == -1
    assert rc.expect(HAMMING_7_4, None, 5, 0)[0].tolist() == [0] * 8 and rc.expect(HAMMING_7_4, None, 5, 0)[1] == -1   # k < t: no sums
    v = HAMMING_7_4[1] ^ HAMMING_7_4[2]
    assert rc.expect(HAMMING_7_4, v, 2, 0)[1] == rc.rank([1, 2]) == 2                           # V is that sum: weight 0
    assert rc.expect(HAMMING_7_4, v, 0, 0)[0].tolist() == [0, 0, 0, 0, 1, 0, 0, 0] and rc.expect(HAMMING_7_4, v, 0, 0)[1] == 4 << 40
    z = np.zeros((5, 0), dtype=np.uint8)
    assert rc.expect(z, None, 2, 0)[0].tolist() == [10] and rc.expect(z, None, 2, 0)[1] == 0 and rc.expect(z, None, 2, 1)[1] == -1


@pytest.mark.parametrize("k", range(0, 9))
@pytest.mark.parametrize("with_v", [False, True])
def test_the_t_sums_make_up_the_row_space(k, with_v):
    n = 37
    G = Mzd.random(max(k, 1), n, 300 + k).to_bits()[:k]
    V = Mzd.random(1, n, 320 + k).to_bits()[0] if with_v else None
    total = sum(rc.expect(G, V, t, 0)[0] for t in range(k + 1))
    assert np.array_equal(total, rw.expect(G, V, 0)[0])
    w = rw.weights(G, V)   # and the lightest of each t is the lightest message of that many rows
    for t in range(k + 1):
        msgs = [x for x in range(1 << k) if bin(x).count("1") == t]
        best = min((int(w[x]), rc.rank([i for i in range(k) if x >> i & 1])) for x in msgs)
        assert rc.expect(G, V, t, 0)[1] == (best[0] << 40) | best[1]


def test_closed_forms_match_brute_force():
    k, a, b, c = 20, 3, 11, 17
    G = rc.rigged(k, a, b, c)
    hist, light = rc.expect(G, None, 3, 1)
    assert (hist[3], hist[5], hist[6], hist[7]) == (1, 2 * (k - 3), comb(k - 1, 3), comb(k - 3, 2)) and int(hist.sum()) == comb(k, 3)
    assert light == (3 << 40) | 738 and rc.rank([a, b, c]) == 738
    hist, light = rc.expect(G, None, 4, 1)
    assert [int(hist[w]) for w in (5, 7, 8, 9)] == [17, 272, 3876, 680] and light == (5 << 40) | 2548
    for kk, abc in ((20, (3, 11, 17)), (12, (11, 0, 5)), (9, (0, 1, 2))):
        for t in range(1, 6):
            hist, light = rc.expect(rc.rigged(kk, *abc), None, t, 1)
            assert np.array_equal(hist, rc.rigged_hist(kk, t)), (kk, t)
            if t >= 3:
                assert light == rc.rigged_lightest(kk, *abc, t), (kk, t)
    for kk in (1, 4, 9):
        for t in range(0, 6):
            for w_min in (0, 2 * t, 2 * t + 1):
                h, light = rc.expect(rc.doubled_identity(kk), None, t, w_min)
                wh, wl = rc.doubled_identity_expect(kk, t, w_min)
                assert np.array_equal(h, wh) and light == wl, (kk, t, w_min)


def test_subset_ranks():
    for k, t in [(0, 0), (5, 0), (5, 1), (6, 2), (7, 3), (9, 4), (10, 8)]:
        sets = sorted(combinations(range(k), t), key=lambda S: S[::-1])     # colexicographic: compare the largest element first
        for r, S in enumerate(sets):
            assert m4ri_amd.row_subset_rank(S) == rc.rank(S) == r
            assert m4ri_amd.row_subset_unrank(r, t) == rc.unrank(r, t) == S
        assert m4ri_amd.row_subset_rank(reversed(sets[-1])) == comb(k, t) - 1    # any order
    last = comb(1024, 4) - 1
    assert m4ri_amd.row_subset_unrank(last, 4) == (1020, 1021, 1022, 1023) and m4ri_amd.row_subset_rank((1020, 1021, 1022, 1023)) == last
    assert last < 1 << 40 <= comb(1024, 5)
    rng = np.random.default_rng(4)
    for _ in range(50):
        t = int(rng.integers(1, 9))
        S = tuple(sorted(rng.choice(1024, size=t, replace=False).tolist()))
        assert m4ri_amd.row_subset_unrank(m4ri_amd.row_subset_rank(S), t) == S
    with pytest.raises(ValueError):
        m4ri_amd.row_subset_rank((1, 1))
    with pytest.raises(ValueError):
        m4ri_amd.row_subset_unrank(-1, 2)
    with pytest.raises(ValueError):
        m4ri_amd.row_subset_unrank(1, 0)


# ---- the plan ---------------------------------------------------------------------------------------------------------------------------

def test_path_boundary():
    P = m4ri_amd.plan_row_sums_weights_batch
    assert 1 <= M0 <= 1 << 24
    for n in (1, 64, 65, 1024):
        for t in range(1, 9):     # ONE boundary in the number of sums, whatever t and n > 0
            for k in list(range(0, 130)) + [255, 256, 511, 512, 1023, 1024]:
                assert P(k, n, t) == (0 if k < t or comb(k, t) <= M0 else 1), (k, n, t)
    # the measured shape itself and the next ones: C(182, 2) = M0 and C(183, 2) = 16653; C(47, 3) = 16215 and C(48, 3) = 17296; C(50, 3)
    # = 19600, where path 0 was measured to lose; every t = 1 is path 0
    assert comb(182, 2) == M0 and comb(183, 2) > M0 + 1 and comb(47, 3) <= M0 < comb(48, 3)
    assert (P(182, 256, 2), P(183, 256, 2), P(47, 64, 3), P(48, 64, 3), P(50, 256, 3), P(1024, 1024, 1)) == (0, 1, 0, 1, 1, 0)
    for s in [(0, 0, 0), (5, 0, 2), (1024, 0, 4), (5, 64, 0), (1024, 64, 0), (3, 64, 4), (1024, 1024, 0)]:   # no columns, t = 0, no sums
        assert P(*s) == 0, s
    for s in [(1024, 1, 2), (1024, 1024, 4), (1024, 64, 5), (2000, 64, 3), (100, 64, 9)]:   # beyond the limits: the same rule
        assert P(*s) == 1, s


def test_plan_ignores_the_override_variable(monkeypatch):
    P = m4ri_amd.plan_row_sums_weights_batch
    for v in ("-1", "0", "5", "16777216", "1000000000000", "junk", "-7"):
        monkeypatch.setenv(PATH0, v)
        assert (P(182, 64, 2), P(183, 64, 2), P(4, 64, 1), P(1024, 1024, 3)) == (0, 1, 0, 1), v
    monkeypatch.delenv(PATH0)


def test_negative_sizes():
    P = m4ri_amd.plan_row_sums_weights_batch
    assert P(-1, 5, 2) == -1 and P(5, -1, 2) == -1 and P(5, 5, -1) == -1 and P(-1, -1, -1) == -1 and P(-1, 0, 0) == -1


# ---- the argument checks ----------------------------------------------------------------------------------------------------------------
# G: 2 members of 4 x 64 (4 words each, 8 words in all) at G0, V: 2 words at V0; hist (2 * 65 entries, 1040 bytes) at H0 and lightest
# (2 entries) at L0, far away.
G0, V0, H0, L0 = 1 << 20, 1 << 24, 1 << 28, 1 << 29
HB = 2 * 65 * 8


def _call(G=G0, g_stride=1, g_bs=4, k=4, n=64, V=V0, v_bs=1, batch=2, t=2, w_min=0, hist=H0, lightest=L0):
    return m4ri_amd.lib().m4ri_amd_row_sums_weights_batch_dev(G, g_stride, g_bs, k, n, V, v_bs, batch, t, w_min, hist, lightest, None)


@pytest.mark.parametrize("kw", [
    dict(k=-1), dict(n=-1), dict(batch=-1), dict(g_stride=-1), dict(g_bs=-1), dict(v_bs=-1), dict(w_min=-1), dict(t=-1),
    dict(V=None, v_bs=-1),
    dict(g_stride=0),                                        # below words(64) = 1 with k > 1
    dict(n=65, g_stride=1, g_bs=8),                          # g_stride 1 < words(65) = 2
    dict(k=2, g_stride=0),                                   # the smallest k that has a stride
    dict(G=None), dict(G=None, t=1), dict(G=None, t=4),      # a NULL G with non-empty members that have sums
    dict(hist=None, lightest=None),                          # no output at all
    dict(hist=G0), dict(hist=G0 + 8 * 7),                    # hist[0] on G's first / last word
    dict(hist=G0 - HB + 8),                                  # hist's last entry is G's first word
    dict(lightest=G0 - 8), dict(lightest=G0 + 8 * 7),        # two entries: the second is G's first word; the first is G's last
    dict(hist=G0 + 8 * 3, g_bs=0),                           # one shared G: its span is one member
    dict(lightest=G0 + 8 * 3, g_bs=0),
    dict(hist=V0 + 8), dict(hist=V0 - HB + 8), dict(lightest=V0 - 8), dict(lightest=V0 + 8),
    dict(lightest=V0, v_bs=0), dict(hist=V0, v_bs=0),        # one shared V: one word
    dict(hist=L0 - HB + 8), dict(hist=L0 + 8),               # hist's last entry on lightest[0]; hist[0] on lightest[1]
    dict(lightest=H0 + HB - 8), dict(lightest=H0 - 8),
    dict(hist=G0, t=0), dict(hist=G0, t=5),                  # G is not read then, but its span is still no place for an output
])
def test_invalid_arguments(kw):
    """Rejected before any HIP call: the pointers are not device memory (and this machine may have no GPU at all)."""
    assert _call(**kw) == HIP_ERROR_INVALID_VALUE


@pytest.mark.parametrize("kw", [
    dict(), dict(g_bs=0), dict(v_bs=0), dict(V=None), dict(V=None, v_bs=0), dict(G=None), dict(w_min=0), dict(w_min=1 << 40),
    dict(hist=None), dict(lightest=None), dict(g_stride=7, g_bs=3),           # g_bs is free: G is only read
    dict(n=65, g_stride=2, g_bs=8),
    dict(k=1, g_stride=0, t=1), dict(k=0, g_stride=0, G=None),                # a stride only counts between two rows
    dict(n=0, g_stride=0, G=None, V=None),
    dict(t=0), dict(t=4), dict(t=5), dict(t=8), dict(t=0, G=None), dict(t=5, G=None),
    dict(k=1024, g_stride=1, t=4), dict(k=1024, n=1024, g_stride=16, t=4), dict(k=1024, t=0), dict(k=1024, t=1),   # the limits themselves
    dict(k=1024, n=1024, g_stride=16, t=3), dict(k=100, t=8), dict(n=1024, g_stride=16),
])
def test_batch_zero_is_success(kw):
    """Legal arguments: shown with batch = 0, which returns before any HIP call."""
    assert _call(**dict(kw, batch=0)) == 0


def test_a_null_g_is_accepted_where_no_row_is_read():
    """Members without sums (k < t) or without columns; the launch itself is not reached with batch = 0, the check is."""
    assert _call(G=None, t=5, batch=0) == 0 and _call(G=None, n=0, V=None, batch=0) == 0 and _call(G=None, t=0, batch=0) == 0


@pytest.mark.parametrize("kw", [
    dict(hist=G0 + 8 * 8), dict(hist=G0 - HB), dict(lightest=G0 - 16), dict(lightest=G0 + 8 * 8),
    dict(hist=G0 + 8 * 4, g_bs=0), dict(lightest=G0 + 8 * 4, g_bs=0),
    dict(hist=V0 + 16), dict(hist=V0 - HB), dict(lightest=V0 - 16), dict(lightest=V0 + 16),
    dict(lightest=V0 + 8, v_bs=0), dict(hist=V0 + 8, v_bs=0),
    dict(hist=L0 - HB), dict(hist=L0 + 16), dict(lightest=H0 + HB), dict(lightest=H0 - 16),
    dict(V=None, hist=V0), dict(V=None, lightest=V0),
])
def test_outputs_beside_the_operands_are_accepted(kw):
    """The accepted neighbours of the overlaps above, one element further out.  Shown with batch = 0, as every legal call is here."""
    assert _call(**dict(kw, batch=0)) == 0


@pytest.mark.parametrize("kw", [
    dict(k=1024, t=5), dict(k=1024, t=5, batch=0), dict(t=9), dict(t=9, batch=0), dict(n=1025, g_stride=17), dict(n=1025, g_stride=17, batch=0),
    dict(k=1025), dict(k=1025, t=0), dict(k=1 << 40), dict(n=1 << 40, g_stride=1 << 40), dict(t=1 << 40), dict(k=200, t=8), dict(k=700, t=5),
])
def test_beyond_the_limits_is_not_supported(kw):
    assert _call(**kw) == HIP_ERROR_NOT_SUPPORTED


def test_the_limit_of_the_rank_is_two_to_the_forty():
    for t in range(1, 9):
        k = max(k for k in range(t, 1025) if comb(k, t) <= 1 << 40)
        assert _call(k=k, t=t, batch=0) == 0, (k, t)
        if k < 1024:
            assert _call(k=k + 1, t=t, batch=0) == HIP_ERROR_NOT_SUPPORTED, (k + 1, t)


def test_negative_sizes_come_before_the_limits():
    assert _call(k=1025, n=-1) == HIP_ERROR_INVALID_VALUE and _call(k=-1, n=1025) == HIP_ERROR_INVALID_VALUE
    assert _call(t=9, w_min=-1) == HIP_ERROR_INVALID_VALUE and _call(k=1024, t=-1) == HIP_ERROR_INVALID_VALUE


def test_python_wrappers_are_bound():
    assert m4ri_amd.plan_row_sums_weights_batch(0, 0, 0) == 0 and m4ri_amd.plan_row_sums_weights_batch(-1, 3, 1) == -1
    assert m4ri_amd.plan_row_sums_weights_batch(1024, 64, 3) == 1
    with pytest.raises(RuntimeError):
        m4ri_amd.row_sums_weights_batch_dev(G0, 1, 4, 4, 64, 0, 0, 2, 2)                          # no output
    with pytest.raises(RuntimeError):
        m4ri_amd.row_sums_weights_batch_dev(G0, 0, 4, 4, 64, 0, 0, 2, 2, hist=H0)                 # G's stride 0 < width 1
    with pytest.raises(RuntimeError, match="801"):
        m4ri_amd.row_sums_weights_batch_dev(G0, 1, 4, 1024, 64, 0, 0, 2, 5, hist=H0)              # the rank beyond the key
    m4ri_amd.row_sums_weights_batch_dev(G0, 1, 4, 4, 64, 0, 0, 0, 2, hist=H0)                     # batch = 0: success, nothing touched
    m4ri_amd.row_sums_weights_batch_dev(G0, 1, 4, 4, 64, V0, 1, 0, 3, w_min=1, lightest=L0, stream=0)
    m4ri_amd.row_sums_weights_batch_dev(G0, 1, 0, 4, 64, V0, 0, 0, 2, 0, H0, L0, 0)
