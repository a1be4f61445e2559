"""The host side of m4ri_amd_rowspace_weights_batch_dev, without a GPU: the NumPy expectations of tests/rowspace_cases.py on
hand-checked codes and against the reference's mzd_make_table, the path boundary of m4ri_amd_plan_rowspace_weights_batch and the
argument checks, which run before any HIP call."""
import numpy as np
import pytest

import elim_cases as ec
import m4ri_amd
import rowspace_cases as rw
from m4ri_amd.mzd import Mzd

HIP_ERROR_INVALID_VALUE, HIP_ERROR_NOT_SUPPORTED = 1, 801
PATH0 = "M4RI_AMD_ROWSPACE_PATH0_MAX"

HAMMING_7_4 = np.array([[1, 0, 0, 0, 1, 1, 0],
                        [0, 1, 0, 0, 1, 0, 1],
                        [0, 0, 1, 0, 0, 1, 1],
                        [0, 0, 0, 1, 1, 1, 1]], dtype=np.uint8)


def test_numpy_expectations_on_hand_checked_cases():
    hist, light = rw.expect(HAMMING_7_4, None, 1)
    assert hist.tolist() == [1, 0, 0, 7, 7, 0, 0, 1]
    assert light == (3 << 40) | 1                       # row 0 alone weighs 3: x0 = 1
    assert rw.expect(HAMMING_7_4, None, 0)[1] == 0      # the zero word, message 0
    assert rw.expect(HAMMING_7_4, None, 4)[1] == (4 << 40) | 3   # rows 0 + 1 = 1100011
    assert rw.expect(HAMMING_7_4, None, 7)[1] == (7 << 40) | 15  # all four rows: the all-ones word
    assert rw.expect(HAMMING_7_4, None, 8)[1] == -1
    # a received word one bit away from codeword x = 5 (rows 0 and 2): distance 1, message 5
    v = (HAMMING_7_4[0] ^ HAMMING_7_4[2]).copy()
    v[6] ^= 1
    hist, light = rw.expect(HAMMING_7_4, v, 0)
    assert light == (1 << 40) | 5 and hist.tolist() == [0, 1, 3, 4, 4, 3, 1, 0]   # a perfect code: one codeword at distance 1
    # a repeated row: messages are counted, not words
    r = np.array([1, 1, 0, 1, 0], dtype=np.uint8)
    hist, light = rw.expect(np.stack([r, r]), None, 1)
    assert hist.tolist() == [2, 0, 0, 2, 0, 0] and light == (3 << 40) | 1
    hist, light = rw.expect(np.stack([r, r]), r, 0)     # V in the span: weight 0 at x = 1 and x = 2
    assert hist.tolist() == [2, 0, 0, 2, 0, 0] and light == 1
    # a zero matrix: nothing of weight >= 1
    z = np.zeros((3, 9), dtype=np.uint8)
    hist, light = rw.expect(z, None, 1)
    assert hist.tolist() == [8] + [0] * 9 and light == -1 and rw.expect(z, None, 0)[1] == 0
    # k = 0: the one message, c = V; n = 0: every word weighs 0
    v9 = np.array([1, 0, 1, 1, 0, 0, 0, 0, 1], dtype=np.uint8)
    hist, light = rw.expect(np.zeros((0, 9), dtype=np.uint8), v9, 0)
    assert hist.tolist() == [0, 0, 0, 0, 1, 0, 0, 0, 0, 0] and light == 4 << 40
    hist, light = rw.expect(np.zeros((5, 0), dtype=np.uint8), None, 0)
    assert hist.tolist() == [32] and light == 0 and rw.expect(np.zeros((5, 0), dtype=np.uint8), None, 1)[1] == -1
    # the closed form of the doubled identity
    for k in (1, 2, 5, 9):
        G = rw.doubled_identity(k)
        assert rw.expect(G, None, 1)[0].tolist() == rw.doubled_identity_hist(k).tolist() and rw.expect(G, None, 1)[1] == (2 << 40) | 1
        ones = np.concatenate([np.ones(k, dtype=np.uint8), np.zeros(k, dtype=np.uint8)])
        assert rw.expect(G, ones, 0)[0][k] == 1 << k and rw.expect(G, ones, 0)[1] == k << 40
        assert rw.expect(G, None, 2 * k)[1] == ((2 * k) << 40) | ((1 << k) - 1)


@pytest.mark.parametrize("k", range(1, 9))
def test_numpy_expectations_match_the_reference_table(reference, k):
    """mzd_make_table on k rows: table row L[x] is the combination of the rows that x selects, so its weight is wt(c(x))."""
    RL = ec.bind_reference(reference)
    n = 131
    M = Mzd.random(k + 3, n, 50 + k)
    T, L = Mzd.init(1 << k, n), np.zeros(1 << k, dtype=np.int32)
    ec.call_make_table(RL, M, 2, 0, k, T, L)            # rows 2 .. 2 + k - 1
    table_weights = T.to_bits().sum(axis=1, dtype=np.int64)
    G = M.to_bits()[2:2 + k]
    w = rw.weights(G)
    assert np.array_equal(w, table_weights[L])
    assert sorted(L.tolist()) == list(range(1 << k))
    assert np.array_equal(rw.hist_of(w, n), np.bincount(table_weights, minlength=n + 1))
    want = min((int(table_weights[L[x]]) << 40) | x for x in range(1 << k) if table_weights[L[x]] >= 1)
    assert rw.lightest_of(w, 1) == want


# ---- the plan ---------------------------------------------------------------------------------------------------------------------------

def _k0(n=64):
    """The path-0 bound, found by scanning k."""
    P = m4ri_amd.plan_rowspace_weights_batch
    return max(k for k in range(0, 41) if P(k, n) == 0)


def test_path_boundary():
    P, K0 = m4ri_amd.plan_rowspace_weights_batch, _k0()
    assert 6 <= K0 <= 26
    for n in (1, 64, 65, 1024):
        for k in range(0, 41):  # ONE boundary, the same at every n > 0: nothing above it comes back
            assert P(k, n) == (0 if k <= K0 else 1), (k, n)
    for s in [(0, 0), (0, 1), (K0, 1), (K0, 1024), (40, 0), (K0 + 1, 0)]:   # path 0: the bound, and members without columns
        assert P(*s) == 0, s
    for s in [(K0 + 1, 1), (K0 + 1, 1024), (40, 1), (40, 1024)]:            # path 1: one above the bound, and the largest member
        assert P(*s) == 1, s


def test_plan_ignores_the_override_variable(monkeypatch):
    K0 = _k0()
    for v in ("-1", "0", "5", "26", "40", "junk", "-7"):
        monkeypatch.setenv(PATH0, v)
        assert (_k0(), _k0(1024)) == (K0, K0), v
    monkeypatch.delenv(PATH0)


def test_negative_sizes():
    P = m4ri_amd.plan_rowspace_weights_batch
    assert P(-1, 5) == -1 and P(5, -1) == -1 and P(-1, -1) == -1 and P(-1, 0) == -1


# ---- the argument checks ----------------------------------------------------------------------------------------------------------------
# G: 2 members of 4 x 64 (4 words each, 8 words in all) at G0, V: 2 words at V0; hist (2 * 65 entries, 1040 bytes) at H0 and lightest
# (2 entries) at L0, far away.
G0, V0, H0, L0 = 1 << 20, 1 << 24, 1 << 28, 1 << 29
HB = 2 * 65 * 8


def _call(G=G0, g_stride=1, g_bs=4, k=4, n=64, V=V0, v_bs=1, batch=2, w_min=0, hist=H0, lightest=L0):
    return m4ri_amd.lib().m4ri_amd_rowspace_weights_batch_dev(G, g_stride, g_bs, k, n, V, v_bs, batch, w_min, hist, lightest, None)


@pytest.mark.parametrize("kw", [
    dict(k=-1), dict(n=-1), dict(batch=-1), dict(g_stride=-1), dict(g_bs=-1), dict(v_bs=-1), dict(w_min=-1),
    dict(V=None, v_bs=-1),
    dict(g_stride=0),                                        # below words(64) = 1 with k > 1
    dict(n=65, g_stride=1, g_bs=8),                          # g_stride 1 < words(65) = 2
    dict(k=2, g_stride=0),                                   # the smallest k that has a stride
    dict(G=None),                                            # a NULL G with non-empty members
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
])
def test_invalid_arguments(kw):
    """Rejected before any HIP call: the pointers are not device memory (and this machine may have no GPU at all)."""
    assert _call(**kw) == HIP_ERROR_INVALID_VALUE


@pytest.mark.parametrize("kw", [
    dict(), dict(g_bs=0), dict(v_bs=0), dict(V=None), dict(V=None, v_bs=0), dict(G=None), dict(w_min=0), dict(w_min=1 << 40),
    dict(hist=None), dict(lightest=None), dict(g_stride=7, g_bs=3),           # g_bs is free: G is only read
    dict(n=65, g_stride=2, g_bs=8),
    dict(k=1, g_stride=0), dict(k=0, g_stride=0, G=None),                     # a stride only counts between two rows
    dict(n=0, g_stride=0, G=None, V=None),
    dict(k=40, g_stride=1), dict(n=1024, g_stride=16), dict(k=40, n=1024, g_stride=16),   # the limits themselves
])
def test_batch_zero_is_success(kw):
    """Legal arguments: shown with batch = 0, which returns before any HIP call."""
    assert _call(**dict(kw, batch=0)) == 0


@pytest.mark.parametrize("kw", [
    dict(hist=G0 + 8 * 8), dict(hist=G0 - HB), dict(lightest=G0 - 16), dict(lightest=G0 + 8 * 8),
    dict(hist=G0 + 8 * 4, g_bs=0), dict(lightest=G0 + 8 * 4, g_bs=0),
    dict(hist=V0 + 16), dict(hist=V0 - HB), dict(lightest=V0 - 16), dict(lightest=V0 + 16),
    dict(lightest=V0 + 8, v_bs=0), dict(hist=V0 + 8, v_bs=0),
    dict(hist=L0 - HB), dict(hist=L0 + 16), dict(lightest=H0 + HB), dict(lightest=H0 - 16),
    dict(V=None, hist=V0), dict(V=None, lightest=V0),
])
def test_outputs_beside_the_operands_are_accepted(kw):
    """The accepted neighbours of the overlaps above, one element further out: an output that ends where an operand (or the other
    output) starts, or starts where it ends.  Shown with batch = 0, as every legal call is here."""
    assert _call(**dict(kw, batch=0)) == 0


@pytest.mark.parametrize("kw", [dict(k=41), dict(n=1025, g_stride=17), dict(k=41, n=1025, g_stride=17), dict(k=41, batch=0),
                                dict(n=1025, g_stride=17, batch=0), dict(k=1 << 40), dict(n=1 << 40, g_stride=1 << 40)])
def test_beyond_the_limits_is_not_supported(kw):
    assert _call(**kw) == HIP_ERROR_NOT_SUPPORTED


def test_negative_sizes_come_before_the_limits():
    assert _call(k=41, n=-1) == HIP_ERROR_INVALID_VALUE and _call(k=-1, n=1025) == HIP_ERROR_INVALID_VALUE
    assert _call(k=41, w_min=-1) == HIP_ERROR_INVALID_VALUE


def test_python_wrappers_are_bound():
    assert m4ri_amd.plan_rowspace_weights_batch(0, 0) == 0 and m4ri_amd.plan_rowspace_weights_batch(-1, 3) == -1
    assert m4ri_amd.plan_rowspace_weights_batch(40, 64) == 1
    with pytest.raises(RuntimeError):
        m4ri_amd.rowspace_weights_batch_dev(G0, 1, 4, 4, 64, 0, 0, 2)                          # no output
    with pytest.raises(RuntimeError):
        m4ri_amd.rowspace_weights_batch_dev(G0, 0, 4, 4, 64, 0, 0, 2, hist=H0)                 # G's stride 0 < width 1
    with pytest.raises(RuntimeError, match="801"):
        m4ri_amd.rowspace_weights_batch_dev(G0, 1, 4, 41, 64, 0, 0, 2, hist=H0)                # k beyond the key
    m4ri_amd.rowspace_weights_batch_dev(G0, 1, 4, 4, 64, 0, 0, 0, hist=H0)                     # batch = 0: success, nothing touched
    m4ri_amd.rowspace_weights_batch_dev(G0, 1, 4, 4, 64, V0, 1, 0, w_min=1, lightest=L0, stream=0)
    m4ri_amd.rowspace_weights_batch_dev(G0, 1, 0, 4, 64, V0, 0, 0, 0, H0, L0, 0)
