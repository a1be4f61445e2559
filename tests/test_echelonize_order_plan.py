"""The host side of m4ri_amd_echelonize_order_batch_dev and m4ri_amd_random_orders_batch_dev, without a GPU: the NumPy reference of
tests/order_cases.py against the oracle's gf2o_echelonize and against its own invariants, the random orders, the path boundaries of
m4ri_amd_plan_echelonize_order_batch, the argument checks (which run before any HIP call) and the Lee-Brickell pipeline in NumPy alone
that tests/test_gpu_echelonize_order_batch.py repeats on the device."""
import numpy as np
import pytest

import m4ri_amd
import order_cases as oc
import rowsums_cases as rc
from m4ri_amd.mzd import Mzd

HIP_ERROR_INVALID_VALUE, HIP_ERROR_NOT_SUPPORTED = 1, 801
PATH0, PATH1 = "M4RI_AMD_ECH_ORDER_PATH0_MAX", "M4RI_AMD_ECH_ORDER_PATH1_MAX"
LDS_BUDGET, CAP_WORDS = 160 * 1024, 512 * 1024 // 8   # batch_common.h's BATCH_LDS_BUDGET and BATCH_CAP_BYTES


def _bits(m, n, seed, rank_defect=0):
    G = Mzd.random(max(m, 1), max(n, 1), seed).to_bits()[:m, :n]
    for i in range(min(rank_defect, m // 2)):
        G[m - 1 - i] = G[i]   # repeated rows: rank-deficient
    return G


def _leading(M, rank):
    return [int(np.flatnonzero(M[i])[0]) for i in range(rank)]


# ---- the reference against itself ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("m,n", [(1, 1), (7, 5), (20, 37), (37, 20), (64, 64), (30, 130)])
@pytest.mark.parametrize("full", [0, 1])
def test_natural_order_is_the_oracles_echelon_form(oracle, m, n, full):
    G = _bits(m, n, 10 + m + n, rank_defect=3)
    W = Mzd.from_bits(G)
    r = oracle.echelonize(W, full)
    for order in (None, list(range(n))):
        S, rank, piv = oc.ech_order(G, order, full, m)
        assert rank == r and np.array_equal(S, W.to_bits())
        assert piv[:rank].tolist() == _leading(S, rank) and (piv[rank:] == -1).all() and len(piv) == min(m, n)


@pytest.mark.parametrize("m,n", [(7, 5), (20, 37), (37, 20), (64, 64), (30, 130)])
@pytest.mark.parametrize("full", [0, 1])
def test_a_permutation_order_is_gather_echelonize_scatter(oracle, m, n, full):
    G = _bits(m, n, 20 + m + n, rank_defect=2)
    for perm in (np.arange(n)[::-1], oc.random_order(5, m, n)):
        W = Mzd.from_bits(G[:, perm])
        r = oracle.echelonize(W, full)
        want = np.zeros_like(G)
        want[:, perm] = W.to_bits()
        S, rank, piv = oc.ech_order(G, perm, full, m)
        assert rank == r and np.array_equal(S, want)
        assert piv[:rank].tolist() == [int(perm[j]) for j in _leading(W.to_bits(), rank)]


def test_a_descending_order_leaves_bits_left_of_the_pivots():
    """Why the update and the swap cover whole rows: under a right-to-left walk the pivot rows have bits on the left of their pivot."""
    G = _bits(32, 64, 3)
    S, rank, piv = oc.ech_order(G, np.arange(64)[::-1], 0, 32)
    assert rank == 32 and sum(bool(S[i, :piv[i]].any()) for i in range(rank)) >= 24


@pytest.mark.parametrize("m,n,pr", [(20, 37, 20), (20, 37, 12), (37, 20, 37), (37, 20, 30), (10, 70, 9)])
def test_full_form_has_an_identity_on_its_pivots(m, n, pr):
    G = _bits(m, n, 40 + m + pr, rank_defect=2)
    S, rank, piv = oc.ech_order(G, oc.random_order(9, pr, n), 1, pr)
    assert np.array_equal(S[:rank][:, piv[:rank]], np.eye(rank, dtype=np.uint8))
    assert not S[rank:pr].any()                    # every column was visited: what is left below the rank is zero
    assert not S[pr:][:, piv[:rank]].any()         # the followers are reduced too


@pytest.mark.parametrize("full", [0, 1])
def test_a_follower_row_is_reduced_by_the_generator(full):
    k, n = 12, 40
    G, y = _bits(k, n, 50), _bits(1, n, 51)[0]
    order = oc.random_order(11, 0, n)
    S, rank, piv = oc.ech_order(np.vstack([G, y[None, :]]), order, full, k)
    Gs, rank_g, piv_g = oc.ech_order(G, order, full, k)
    assert rank == rank_g == k and np.array_equal(S[:k], Gs) and np.array_equal(piv, piv_g)    # the follower changes nothing above it
    if full:   # y ^ y_I G' with I the pivot columns: the error pattern Lee-Brickell starts from
        want = y.copy()
        for i in range(rank):
            if y[piv[i]]:
                want ^= Gs[i]
        assert np.array_equal(S[k], want) and not S[k][piv[:rank]].any()
    else:      # below every rank: the rows at and below the rank see the same additions under both values of `full`, the follower too
        assert not S[k][piv[:rank]].any()
        assert np.array_equal(S[k], oc.ech_order(np.vstack([G, y[None, :]]), order, 1, k)[0][k])


def test_partial_orders_duplicates_and_bad_entries():
    G = _bits(9, 30, 60)
    S, rank, piv = oc.ech_order(G, [], 1, 9)
    assert rank == 0 and np.array_equal(S, G) and (piv == -1).all()
    S, rank, piv = oc.ech_order(G, [4, 4, 4], 1, 9)
    assert rank == 1 and piv[0] == 4 and S[:, 4].sum() == 1
    S2, rank2, piv2 = oc.ech_order(G, [4, 17, 4, 17, 2], 0, 9)
    S3, rank3, piv3 = oc.ech_order(G, [4, 17, 2], 0, 9)
    assert rank2 == rank3 and np.array_equal(S2, S3) and np.array_equal(piv2, piv3)
    assert np.array_equal(oc.ech_order(G, None, 1, 0)[0], G) and oc.ech_order(G, None, 1, 0)[1] == 0
    for bad in (-1, 30, -(1 << 31), (1 << 31) - 1):
        S, rank, piv = oc.ech_order(G, [3, bad, 5], 1, 9)
        assert rank == -1 and np.array_equal(S, G) and (piv == -1).all() and len(piv) == 9


# ---- the random orders --------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [0, 1, 2, 63, 64, 65, 4095, 4096])
def test_random_order_is_a_permutation(n):
    a, b = m4ri_amd.random_order(3, 2, n), m4ri_amd.random_order(3, 3, n)
    assert a.dtype == np.int32 and sorted(a.tolist()) == list(range(n))
    assert np.array_equal(a, oc.random_order(3, 2, n))            # the vectorised one of the package = the plain-integer one here
    if n >= 63:
        assert not np.array_equal(a, b) and not np.array_equal(a, m4ri_amd.random_order(4, 2, n))


def test_random_order_hand_written():
    """Seed 7, eight columns.  The first outputs of the stream (m4ri_amd_fill_dev's) and, from them, member 0: the keys are the outputs
    with their low 12 bits replaced by 0 .. 7; 0x044c... is the smallest (j = 1), 0x63cb... (j = 0) the fourth."""
    assert [hex(oc.splitmix(7, j)) for j in range(3)] == ["0x63cbe1e459320dd7", "0x44c3cd7f43c661c", "0xe6984080bab12a02"]
    assert m4ri_amd.splitmix_words(7, 0, 3).tolist() == [oc.splitmix(7, j) for j in range(3)]
    assert m4ri_amd.random_order(7, 0, 8).tolist() == [1, 5, 7, 0, 4, 6, 3, 2]
    assert m4ri_amd.random_order(7, 1, 8).tolist() == [2, 0, 1, 7, 6, 5, 4, 3]   # outputs 8 .. 15
    with pytest.raises(ValueError):
        m4ri_amd.random_order(7, 0, 4097)


def test_transpositions_gather_and_scatter():
    for n in (1, 2, 17, 64, 130):
        perm = oc.random_order(13, n, n)
        P = oc.transpositions(perm)
        cols = np.arange(n)
        for i in range(n - 1, -1, -1):    # apply_p_right, trans = 0: descending
            cols[[i, P[i]]] = cols[[P[i], i]]
        assert np.array_equal(cols, perm)
        for i in range(n):                # trans = 1: ascending, back
            cols[[i, P[i]]] = cols[[P[i], i]]
        assert np.array_equal(cols, np.arange(n))


# ---- the plan -----------------------------------------------------------------------------------------------------------------------------

def _lds_bytes(m, n):
    w = (n + 63) // 64
    ldw = w + ((w & 1) ^ 1)
    return m * ldw * 8 + (m * 4 + 15) // 16 * 16 + 2 * ((m + 63) // 64) * 8 + 64 + 4 * n


def _want_path(m, n):
    w = (n + 63) // 64
    if m <= 64 and n <= 64:
        return 0
    if m > CAP_WORDS or w > CAP_WORDS or m * w > CAP_WORDS:
        return 3
    return 1 if _lds_bytes(m, n) <= LDS_BUDGET else 2


def test_path_boundaries():
    P = m4ri_amd.plan_echelonize_order_batch
    assert [P(*s) for s in [(0, 0), (1, 1), (64, 64), (65, 1), (1, 65), (65, 64), (64, 65), (64, 1024), (512, 1024)]] == [0, 0, 0, 1, 1, 1, 1, 1, 1]
    assert P(1100, 1100) == 2 and _lds_bytes(1100, 1100) > LDS_BUDGET
    # the largest square of path 1, found with the documented formula, and the next one
    n = max(n for n in range(65, 1200) if _lds_bytes(n, n) <= LDS_BUDGET)
    assert (P(n, n), P(n + 1, n + 1)) == (1, 2)
    # the order's 4 bytes per column count: a shape that m4ri_amd_plan_echelonize_batch keeps in LDS and this plan does not
    m = max(m for m in range(1, 3000) if _lds_bytes(m, 1024) <= LDS_BUDGET)
    assert (P(m, 1024), P(m + 1, 1024)) == (1, 2) and m4ri_amd.plan_echelonize_batch(m + 1, 1024) == 1
    # the cap: 65536 valid words
    assert [P(*s) for s in [(1024, 4096), (1025, 4096), (1024, 4097), (1, 64 * 65536), (1, 64 * 65536 + 1), (65536, 64), (65537, 1), (65536, 65)]] \
        == [2, 3, 3, 2, 3, 2, 3, 3]
    assert P(1 << 40, 1 << 40) == 3 and P(0, 1 << 40) == 3 and P(1 << 40, 0) == 3
    rng = np.random.default_rng(1)
    for m, n in rng.integers(0, 3000, size=(300, 2)).tolist():
        assert P(m, n) == _want_path(m, n), (m, n)


def test_plan_ignores_the_override_variables(monkeypatch):
    P = m4ri_amd.plan_echelonize_order_batch
    for v in ("0", "1", "64", "100000", "163840", "junk", "-7"):
        monkeypatch.setenv(PATH0, v)
        monkeypatch.setenv(PATH1, v)
        assert (P(1, 1), P(64, 64), P(65, 65), P(1100, 1100), P(1025, 4096)) == (0, 0, 1, 2, 3), v


def test_negative_sizes():
    P = m4ri_amd.plan_echelonize_order_batch
    assert P(-1, 5) == -1 and P(5, -1) == -1 and P(-1, -1) == -1 and P(-1, 1 << 40) == -1


# ---- the argument checks ------------------------------------------------------------------------------------------------------------------
# D and A: 2 members of 4 x 64 (4 words each, 64 bytes in all) at D0 and A0; order: 2 x 64 entries (512 bytes) at O0; rank: 2 entries
# (8 bytes) at R0; pivots: 2 x 4 entries (32 bytes) at P0; all far from each other.
D0, A0, O0, R0, P0 = 1 << 20, 1 << 22, 1 << 24, 1 << 26, 1 << 28


def _call(D=D0, d_stride=1, d_bs=4, A=A0, a_stride=1, a_bs=4, nrows=4, ncols=64, pivot_rows=4, order=O0, o_bs=64, olen=64, batch=2, full=1,
          rank=R0, pivots=P0):
    return m4ri_amd.lib().m4ri_amd_echelonize_order_batch_dev(D, d_stride, d_bs, A, a_stride, a_bs, nrows, ncols, pivot_rows, order, o_bs, olen,
                                                              batch, full, rank, pivots, None)


@pytest.mark.parametrize("kw", [
    dict(nrows=-1, pivot_rows=0), dict(ncols=-1, olen=0), dict(pivot_rows=-1), dict(olen=-1), dict(batch=-1), dict(d_stride=-1), dict(d_bs=-1),
    dict(a_stride=-1), dict(a_bs=-1), dict(o_bs=-1),
    dict(pivot_rows=5), dict(olen=65), dict(nrows=0), dict(ncols=0),                    # pivot_rows > nrows, olen > ncols
    dict(d_stride=0), dict(a_stride=0), dict(ncols=65, d_bs=8, a_bs=8),                 # a stride below the width
    dict(ncols=65, d_stride=2, d_bs=8, a_bs=8), dict(ncols=65, a_stride=2, d_bs=8, a_bs=8),
    dict(d_bs=3), dict(d_bs=0),                                                         # overlapping D members
    dict(A=D0, d_bs=0, a_bs=0), dict(A=D0, d_stride=0, a_stride=0, d_bs=0, a_bs=0, nrows=1, pivot_rows=1),   # in place from one shared A
    dict(A=D0, a_bs=0),                                                                 # D on a shared A, not in place
    dict(A=D0, d_stride=2, d_bs=8), dict(A=D0, a_stride=2, a_bs=8), dict(A=D0, a_bs=5), # D == A, but not the same layout
    dict(D=A0 + 8), dict(D=A0 - 8), dict(D=A0 + 56), dict(D=A0 - 56),                   # D's last word on A's first, and the other way
    dict(D=A0 + 24, a_bs=0), dict(D=A0 - 56, a_bs=0),                                   # one shared A: its span is one member
    dict(order=D0 + 60), dict(order=D0 - 508), dict(order=D0 - 252, o_bs=0),            # D meeting order
    dict(rank=D0 + 60), dict(rank=D0 - 4), dict(pivots=D0 + 60), dict(pivots=D0 - 28),  # D meeting rank, pivots
    dict(pivots=R0 + 4), dict(pivots=R0 - 28), dict(rank=P0 + 28), dict(rank=P0 - 4),   # rank meeting pivots
    dict(order=R0 + 4), dict(order=R0 - 508), dict(order=P0 + 28), dict(order=P0 - 508),  # rank and pivots meeting order
    dict(pivots=R0 + 4, pivot_rows=1), dict(pivots=R0 - 4, pivot_rows=1),               # pm = 1: two entries
    dict(rank=None), dict(A=None), dict(D=None), dict(A=None, D=None),
])
def test_invalid_arguments(kw):
    """Rejected before any HIP call: the pointers are not device memory (and this machine may have no GPU at all)."""
    assert _call(**kw) == HIP_ERROR_INVALID_VALUE


@pytest.mark.parametrize("kw", [
    dict(), dict(A=D0), dict(a_bs=0), dict(o_bs=0), dict(order=None), dict(order=None, olen=0), dict(olen=0), dict(olen=7), dict(pivots=None),
    dict(pivot_rows=0), dict(pivot_rows=3), dict(full=0), dict(d_stride=3, d_bs=10), dict(a_stride=7, a_bs=1),    # a_bs is free: A is only read
    dict(A=D0, d_stride=2, a_stride=2, d_bs=8, a_bs=8), dict(ncols=65, olen=65, d_stride=2, a_stride=2, d_bs=8, a_bs=8),
    dict(nrows=0, pivot_rows=0, A=None, D=None), dict(ncols=0, olen=0, A=None, D=None, order=None),
    dict(nrows=1024, ncols=4096, pivot_rows=1024, d_stride=64, a_stride=64, d_bs=1 << 16, a_bs=1 << 16),          # the cap itself
    dict(D=A0 + 64), dict(D=A0 - 64), dict(D=A0 + 32, a_bs=0), dict(D=A0 - 64, a_bs=0),
    dict(order=D0 + 64), dict(order=D0 - 512), dict(order=D0 - 256, o_bs=0),
    dict(rank=D0 + 64), dict(rank=D0 - 8), dict(pivots=D0 + 64), dict(pivots=D0 - 32),
    dict(pivots=R0 + 8), dict(pivots=R0 - 32), dict(rank=P0 + 32), dict(rank=P0 - 8),
    dict(order=R0 + 8), dict(order=R0 - 512), dict(order=P0 + 32), dict(order=P0 - 512),
    dict(pivots=R0 + 8, pivot_rows=1), dict(pivots=R0 - 8, pivot_rows=1),
    dict(order=None, pivots=None, rank=R0),
])
def test_batch_zero_is_success(kw):
    """Legal arguments, among them the accepted neighbours of the overlaps above, one element further out: shown with batch = 0,
    which returns before any HIP call, as every legal call must be shown here (tests/test_gpu_echelonize_order_batch.py runs outputs
    packed back to back)."""
    assert _call(**dict(kw, batch=0)) == 0


@pytest.mark.parametrize("kw", [
    dict(nrows=1025, ncols=4096, pivot_rows=0), dict(nrows=1024, ncols=4097), dict(nrows=1, pivot_rows=1, ncols=64 * 65536 + 1),
    dict(nrows=65537, ncols=1, olen=1), dict(nrows=1 << 40, ncols=1 << 40),
])
@pytest.mark.parametrize("batch", [0, 2])
def test_beyond_the_cap_is_not_supported(kw, batch):
    w = (kw["ncols"] + 63) // 64
    big = dict(d_stride=w, a_stride=w, d_bs=1 << 50, a_bs=0, order=None, olen=0, pivots=None)
    assert _call(**dict(big, **kw, batch=batch)) == HIP_ERROR_NOT_SUPPORTED


def test_sizes_and_strides_are_checked_before_the_cap():
    assert _call(nrows=1025, ncols=4096, d_stride=64, a_stride=63) == HIP_ERROR_INVALID_VALUE
    assert _call(nrows=1025, ncols=4096, d_stride=64, a_stride=64, batch=-1) == HIP_ERROR_INVALID_VALUE
    assert _call(nrows=1025, ncols=4096, d_stride=64, a_stride=64, pivot_rows=1026) == HIP_ERROR_INVALID_VALUE


RO = 1 << 30


@pytest.mark.parametrize("args,want", [
    ((RO, 10, -1, 2, 7), 1), ((RO, -1, 5, 2, 7), 1), ((RO, 10, 5, -1, 7), 1), ((RO, 4, 5, 2, 7), 1), ((None, 10, 5, 2, 7), 1), ((None, 10, 5, 1, 7), 1),
    ((RO, 10, 4097, 2, 7), 801), ((RO, 10, 4097, 0, 7), 801), ((RO, 1 << 40, 1 << 40, 2, 7), 801),
    ((RO, 10, 5, 0, 7), 0), ((RO, 4096, 4096, 0, 7), 0), ((None, 0, 0, 5, 7), 0), ((RO, 0, 0, 5, 7), 0), ((None, 10, 5, 0, 7), 0),
    ((RO, 5, 5, 0, 7), 0), ((RO, 0, 5, 0, 7), 0),
])
def test_random_orders_argument_checks(args, want):
    assert m4ri_amd.lib().m4ri_amd_random_orders_batch_dev(*args, None) == want


def test_python_wrappers_are_bound():
    assert m4ri_amd.plan_echelonize_order_batch(0, 0) == 0 and m4ri_amd.plan_echelonize_order_batch(-1, 3) == -1
    with pytest.raises(RuntimeError):
        m4ri_amd.echelonize_order_batch_dev(D0, 1, 4, A0, 1, 4, 4, 64, 4, O0, 64, 64, 2, 1, 0)               # no rank
    with pytest.raises(RuntimeError):
        m4ri_amd.echelonize_order_batch_dev(D0, 1, 4, A0 + 8, 1, 4, 4, 64, 4, 0, 0, 64, 2, 1, R0)            # D meets A
    with pytest.raises(RuntimeError, match="801"):
        m4ri_amd.echelonize_order_batch_dev(D0, 64, 1 << 20, A0, 64, 0, 1025, 4096, 4, 0, 0, 0, 2, 1, R0)
    m4ri_amd.echelonize_order_batch_dev(D0, 1, 4, A0, 1, 4, 4, 64, 4, O0, 64, 64, 0, 1, R0)                  # batch = 0: success, nothing touched
    m4ri_amd.echelonize_order_batch_dev(D0, 1, 4, D0, 1, 4, 4, 64, 3, 0, 0, 64, 0, 0, R0, pivots=P0, stream=0)
    with pytest.raises(RuntimeError, match="801"):
        m4ri_amd.random_orders_batch_dev(RO, 5000, 4097, 2, 7)
    with pytest.raises(RuntimeError):
        m4ri_amd.random_orders_batch_dev(RO, 3, 5, 2, 7)
    m4ri_amd.random_orders_batch_dev(RO, 64, 64, 0, 7)
    m4ri_amd.random_orders_batch_dev(RO, 64, 64, 0, -1, stream=0)                                          # any 64-bit seed


# ---- one iteration of Lee-Brickell, many members, in NumPy alone --------------------------------------------------------------------------

def pipeline(k=16, n=64, members=32, gen_seed=1, order_seed=7):
    """Generator Mzd.random(k, n, gen_seed); member b: the systematic form on random_order(order_seed, b, n), then the lightest single
    row and the lightest sum of two rows (w_min = 1) in the key of m4ri_amd_row_sums_weights_batch_dev.  Returns (G, the orders, the
    forms, lightest[t - 1][b])."""
    G = Mzd.random(k, n, gen_seed).to_bits()
    orders = [oc.random_order(order_seed, b, n) for b in range(members)]
    forms = [oc.ech_order(G, o, 1, k) for o in orders]
    lightest = [[rc.expect(S, None, t, 1)[1] for (S, _r, _p) in forms] for t in (1, 2)]
    return G, orders, forms, lightest


def test_pipeline_finds_the_minimum_distance():
    G, orders, forms, lightest = pipeline()
    k = G.shape[0]
    msgs = ((np.arange(1, 1 << k)[:, None] >> np.arange(k)[None, :]) & 1).astype(np.uint8)
    d = int(((msgs @ G) & 1).sum(axis=1).min())      # all 2^16 - 1 messages
    assert all(r == k for (_S, r, _p) in forms)
    best = [min(lightest[0][b], lightest[1][b]) >> 40 for b in range(len(forms))]
    assert min(best) == d == 16
    assert sum(x == d for x in best) == 9           # at least one member reaches it; with these seeds nine do
