"""The host side of assemble_batch.hip, without a GPU: the NumPy expectations of tests/assemble_cases.py pinned to the real reference
(mzd_submatrix, mzd_concat, mzd_stack, mzd_extract_u, mzd_extract_l, the four mzd_apply_p_*), the identity L * U = P^T A Q^T that the
triangle rules with a rank make hold for every rank, the path boundaries of m4ri_amd_plan_perm_batch, and the argument checks of the
four entry points, which run before any HIP call."""
import ctypes

import numpy as np
import pytest

import assemble_cases as ac
import cpu_libs
import m4ri_amd
from m4ri_amd.mzd import Mzd, MzdPtr

HIP_ERROR_INVALID_VALUE = 1
PATH0, PATH1 = "M4RI_AMD_PERM_BATCH_PATH0_MAX", "M4RI_AMD_PERM_BATCH_PATH1_MAX"
LDS = 160 * 1024


# ---- the expectations against the reference -----------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def ref():
    r = cpu_libs.reference()
    if r is None:
        pytest.skip("the reference build is absent")
    I = ctypes.c_int
    for name, args in (("mzd_submatrix", [MzdPtr, MzdPtr, I, I, I, I]), ("mzd_concat", [MzdPtr] * 3), ("mzd_stack", [MzdPtr] * 3),
                       ("mzd_extract_u", [MzdPtr] * 2), ("mzd_extract_l", [MzdPtr] * 2)):
        fn = getattr(r.L, name)
        fn.restype, fn.argtypes = MzdPtr, args
    return r


def _rand(r, c, seed):
    return Mzd.random(r, c, seed)


@pytest.mark.parametrize("lowc", [0, 64, 1, 63, 65, 13])
def test_block_copy_is_mzd_submatrix(ref, lowc):
    A = _rand(70, 300, 11 + lowc)
    for lowr, rows, cols in [(0, 70, 129), (3, 64, 64), (5, 1, 1), (2, 65, 200)]:
        S = Mzd(rows, cols)
        ref.L.mzd_submatrix(S.ptr, A.ptr, lowr, lowc, lowr + rows, lowc + cols)
        want = ac.copy_block(np.ones((rows, cols), dtype=np.uint8), 0, 0, A.to_bits(), lowr, lowc, rows, cols)
        assert np.array_equal(S.to_bits(), want), (lowr, rows, cols)


@pytest.mark.parametrize("ca,cb", [(64, 64), (65, 65), (1, 129), (100, 37)])
def test_two_block_copies_are_mzd_concat_and_mzd_stack(ref, ca, cb):
    A, B = _rand(33, ca, 1), _rand(33, cb, 2)
    C = Mzd(33, ca + cb)
    ref.L.mzd_concat(C.ptr, A.ptr, B.ptr)
    want = ac.copy_block(np.ones((33, ca + cb), dtype=np.uint8), 0, 0, A.to_bits(), 0, 0, 33, ca)
    want = ac.copy_block(want, 0, ca, B.to_bits(), 0, 0, 33, cb)
    assert np.array_equal(C.to_bits(), want) and np.array_equal(want, np.hstack([A.to_bits(), B.to_bits()]))
    A, B = _rand(ca, 70, 3), _rand(cb, 70, 4)
    C = Mzd(ca + cb, 70)
    ref.L.mzd_stack(C.ptr, A.ptr, B.ptr)
    want = ac.copy_block(np.ones((ca + cb, 70), dtype=np.uint8), 0, 0, A.to_bits(), 0, 0, ca, 70)
    want = ac.copy_block(want, ca, 0, B.to_bits(), 0, 0, cb, 70)
    assert np.array_equal(C.to_bits(), want) and np.array_equal(want, np.vstack([A.to_bits(), B.to_bits()]))


@pytest.mark.parametrize("n", [1, 63, 64, 65, 130])
def test_triangles_are_mzd_extract_u_and_l(ref, n):
    A = _rand(n, n, 20 + n)
    U, L = Mzd(n, n), Mzd(n, n)
    ref.L.mzd_extract_u(U.ptr, A.ptr)
    ref.L.mzd_extract_l(L.ptr, A.ptr)
    assert np.array_equal(U.to_bits(), ac.triangle(A.to_bits(), True, 2))
    assert np.array_equal(L.to_bits(), ac.triangle(A.to_bits(), False, 2))


@pytest.mark.parametrize("which,right,trans", [("mzd_apply_p_left", 0, 0), ("mzd_apply_p_left_trans", 0, 1), ("mzd_apply_p_right", 1, 0),
                                               ("mzd_apply_p_right_trans", 1, 1)])
@pytest.mark.parametrize("shape", [(1, 1), (64, 64), (65, 130), (200, 100)])
def test_transpositions_are_mzd_apply_p(ref, which, right, trans, shape):
    n = shape[1] if right else shape[0]
    for name, P in ac.perm_members(n, 7 + n)[:4]:
        for length in ac.perm_lengths(n):
            if length > n:
                continue  # an mzp_t is as long as the side it acts on
            A = _rand(*shape, 5)
            bits = A.to_bits()
            # the identity from `length` on: the reference writes back only the columns below the mzp_t's length (mzp.c:88), so
            # a short one with an entry beyond its length is outside what it supports
            ref.apply_p(A, np.concatenate([P[:length], np.arange(length, n)]), which)
            assert np.array_equal(A.to_bits(), ac.apply_p(bits, P, length, right, trans)), (name, length)


def test_a_length_beyond_the_side_and_bad_entries():
    A = Mzd.random(5, 7, 1).to_bits()
    P = np.array([2, 2, 4, 3, 4, 9, 9, 9, 9, 9])
    assert np.array_equal(ac.apply_p(A, P, 10, 0, 0), ac.apply_p(A, P, 5, 0, 0))
    assert ac.apply_p(A, P, 10, 1, 0) is None and ac.apply_p(A, [0, -1], 2, 0, 0) is None and ac.apply_p(A, [5], 1, 0, 0) is None
    assert np.array_equal(ac.apply_p(A, [0, -1], 1, 0, 0), A)


@pytest.mark.parametrize("shape", ac.CHAIN_SHAPES + ((130, 64),))
def test_l_times_u_is_the_permuted_original_at_every_rank(shape):
    """The oracle's PLUQ: extract(lower, 1, rank) * extract(upper, 2, rank) = mzd_apply_p_left, then mzd_apply_p_right_trans, of the
    original -- at rank 0, a partial rank and the full rank."""
    o = cpu_libs.oracle()
    k = min(shape)
    for r in (0, k // 3 + 1, k):
        orig = ac.with_rank(*shape, r, 100 + r)
        F = Mzd.from_bits(orig)
        rank, P, Q = o.ple(F, pluq=True)
        assert rank == r
        L, U = ac.triangle(F.to_bits(), False, 1, rank), ac.triangle(F.to_bits(), True, 2, rank)
        assert L.shape == (shape[0], k) and U.shape == (k, shape[1])
        W = Mzd.from_bits(orig)
        o.apply_p_left(W, P)
        o.apply_p_right(W, Q, trans=True)
        assert np.array_equal(ac.matmul(L, U), W.to_bits()), r
        want = ac.apply_p(ac.apply_p(orig, P, shape[0], 0, 0), Q, shape[1], 1, 1)
        assert np.array_equal(want, W.to_bits()), r


def test_triangle_rules():
    A = np.ones((5, 3), dtype=np.uint8)
    assert ac.triangle(A, True, 0).tolist() == [[0, 1, 1], [0, 0, 1], [0, 0, 0]]
    assert ac.triangle(A, False, 1).tolist() == [[1, 0, 0], [1, 1, 0], [1, 1, 1], [1, 1, 1], [1, 1, 1]]
    assert ac.triangle(A, True, 1, 1).tolist() == [[1, 1, 1], [0, 0, 0], [0, 0, 0]]
    assert ac.triangle(A, False, 1, 1).tolist() == [[1, 0, 0], [1, 1, 0], [1, 0, 1], [1, 0, 0], [1, 0, 0]]
    assert np.array_equal(ac.triangle(A, False, 2, 9), ac.triangle(A, False, 2)) and np.array_equal(ac.triangle(A, True, 2, -4), np.zeros((3, 3)))


# ---- the plan -----------------------------------------------------------------------------------------------------------------------

def _lds(nrows, ncols, right):
    return nrows * ac.words(ncols) * 8 + 8 * (ncols if right else nrows) + 8


def test_plan_boundaries():
    P = m4ri_amd.plan_perm_batch
    for right in (False, True):
        for s in [(0, 0), (1, 1), (64, 64), (64, 1), (1, 64), (0, 64), (63, 37)]:
            assert P(*s, right) == 0, s
        for s in [(65, 1), (1, 65), (65, 64), (64, 65), (65, 65), (300, 300), (1024, 1024), (200, 100)]:
            assert P(*s, right) == 1, s
        for s in [(4096, 4096), (1 << 40, 1), (1, 1 << 40), (1 << 40, 1 << 40), (20481, 1)]:
            assert P(*s, right) == 2, s
        assert P(-1, 5, right) == -1 and P(5, -1, right) == -1
        for ncols in (65, 640, 1000, 1088, 4096):  # the LDS boundary in the rows at this width, to the row
            rows = max(r for r in range(1, 12000) if _lds(r, ncols, right) <= LDS)
            assert P(rows, ncols, right) == 1 and P(rows + 1, ncols, right) == 2, (ncols, rows)
    assert _lds(100, 10000, False) <= LDS < _lds(100, 10000, True)  # the two sides differ where the index is the longer one
    assert P(100, 10000, False) == 1 and P(100, 10000, True) == 2


def test_plan_ignores_the_override_variables(monkeypatch):
    P = m4ri_amd.plan_perm_batch
    for v in ("0", "1", "64", "1000", "163840", "junk", "-5"):
        monkeypatch.setenv(PATH0, v)
        monkeypatch.setenv(PATH1, v)
        assert P(64, 64, 0) == 0 and P(65, 65, 1) == 1 and P(1024, 1024, 0) == 1 and P(4096, 4096, 1) == 2, v


# ---- the argument checks ------------------------------------------------------------------------------------------------------------

A0, D0, R0 = 1 << 20, 1 << 28, 1 << 30


def _copy(D=D0, d_stride=3, d_bs=200, d_row=0, d_col=0, A=A0, a_stride=3, a_bs=200, a_row=0, a_col=0, rows=64, cols=130, batch=2):
    return m4ri_amd.lib().m4ri_amd_copy_block_batch_dev(D, d_stride, d_bs, d_row, d_col, A, a_stride, a_bs, a_row, a_col, rows, cols, batch, None)


def _tri(D=D0, d_stride=3, d_bs=200, A=A0, a_stride=3, a_bs=200, nrows=64, ncols=130, batch=2, upper=1, diag=2, rank=None):
    return m4ri_amd.lib().m4ri_amd_extract_tri_batch_dev(D, d_stride, d_bs, A, a_stride, a_bs, nrows, ncols, batch, upper, diag, rank, None)


def _perm(side, A=A0, stride=3, a_bs=200, nrows=64, ncols=130, batch=2, P=D0, p_bs=130, length=64, trans=0, status=None):
    fn = m4ri_amd.lib().m4ri_amd_apply_p_right_batch_dev if side else m4ri_amd.lib().m4ri_amd_apply_p_left_batch_dev
    return fn(A, stride, a_bs, nrows, ncols, batch, P, p_bs, length, trans, status, None)


@pytest.mark.parametrize("kw", [
    dict(rows=-1), dict(cols=-1), dict(batch=-1), dict(d_stride=-1), dict(d_bs=-1), dict(a_stride=-1), dict(a_bs=-1), dict(d_row=-1), dict(d_col=-1),
    dict(a_row=-1), dict(a_col=-1),
    dict(d_stride=2), dict(a_stride=2),                              # words(130) = 3
    dict(d_col=63), dict(a_col=63),                                       # one word too short for col + cols = 193: 4 words
    dict(cols=64, d_col=129, d_stride=3), dict(cols=64, a_col=129),  # 129 + 64 = 193
    dict(d_stride=0), dict(a_stride=0),
    dict(d_bs=191),                                                  # overlapping D members: need 63 * 3 + 3 = 192
    dict(d_bs=0),
    dict(cols=64, d_col=64, d_bs=189),                               # the block's own words count: 63 * 3 + 1 = 190
    dict(D=A0 + 8 * 100), dict(D=A0 + 8 * 391), dict(D=A0 - 8 * 391),  # D meets A: two members of 192 words, 200 apart
    dict(D=A0 + 8 * 191, a_bs=0),                                    # one shared A
    dict(D=A0, d_col=64, a_col=0, d_stride=4, a_stride=4, cols=64),  # the same rows: word 1 of D's rows lies inside A's span
    dict(D=None), dict(A=None),
    dict(cols=1 << 40, d_stride=1 << 35, a_stride=1 << 35, d_bs=1 << 50),  # more columns than a launch can number
])
def test_copy_block_refuses(kw):
    assert _copy(**kw) == HIP_ERROR_INVALID_VALUE


@pytest.mark.parametrize("kw", [
    dict(), dict(d_bs=192), dict(cols=64, d_col=64, d_bs=190), dict(a_bs=0), dict(d_col=62), dict(a_col=62), dict(d_col=63, d_stride=4), dict(a_col=63, a_stride=4),
    dict(D=A0 + 8 * 392), dict(D=A0 - 8 * 392), dict(D=A0 + 8 * 192, a_bs=0), dict(D=None, A=None), dict(d_row=1 << 30, a_row=1 << 30),
])
def test_copy_block_accepts(kw):
    """Legal arguments: shown with batch = 0, which returns before any HIP call."""
    assert _copy(batch=0, **kw) == 0


def test_copy_block_empty_blocks_need_nothing():
    assert _copy(rows=0, D=None, A=None) == 0 and _copy(cols=0, D=None, A=None) == 0
    assert _copy(rows=0, D=A0, d_bs=0, d_stride=0, a_stride=0) == 0


@pytest.mark.parametrize("kw", [
    dict(nrows=-1), dict(ncols=-1), dict(batch=-1), dict(d_stride=-1), dict(d_bs=-1), dict(a_stride=-1), dict(a_bs=-1),
    dict(diag=3), dict(diag=-1),
    dict(d_stride=2), dict(a_stride=2), dict(upper=0, a_stride=2), dict(d_stride=0, upper=0),
    dict(d_bs=191), dict(d_bs=0), dict(upper=0, d_stride=1, d_bs=63),   # D members: 64 x 130 (upper), 64 x 64 (lower)
    dict(D=A0 + 8 * 100), dict(D=A0 + 8 * 391), dict(D=A0 - 8 * 391), dict(D=A0 + 8 * 191, a_bs=0), dict(D=A0),
    dict(rank=D0), dict(rank=D0 + 8 * 391), dict(rank=D0 - 4),         # D meets the rank array (two entries)
    dict(D=None), dict(A=None),
    dict(nrows=1 << 31, ncols=64, d_stride=1, a_stride=1, d_bs=1 << 40, a_bs=1 << 40),
])
def test_extract_tri_refuses(kw):
    assert _tri(**kw) == HIP_ERROR_INVALID_VALUE


@pytest.mark.parametrize("kw", [
    dict(), dict(upper=0), dict(diag=0), dict(diag=1), dict(d_bs=192), dict(upper=0, d_stride=1, d_bs=64), dict(a_bs=0), dict(rank=R0),
    dict(D=A0 + 8 * 392), dict(rank=D0 + 8 * 392), dict(rank=D0 - 8), dict(D=None, A=None),
])
def test_extract_tri_accepts(kw):
    assert _tri(batch=0, **kw) == 0


def test_extract_tri_empty_members_need_nothing():
    assert _tri(nrows=0, D=None, A=None) == 0 and _tri(ncols=0, D=None, A=None, d_stride=0, a_stride=0) == 0
    assert _tri(nrows=0, diag=3, D=None, A=None) == HIP_ERROR_INVALID_VALUE


@pytest.mark.parametrize("side", [0, 1])
@pytest.mark.parametrize("kw", [
    dict(nrows=-1), dict(ncols=-1), dict(batch=-1), dict(stride=-1), dict(a_bs=-1), dict(p_bs=-1), dict(length=-1),
    dict(stride=2), dict(stride=0),
    dict(a_bs=191), dict(a_bs=0),                                       # the members are written: they may not overlap, nor be one
    dict(A=None), dict(P=None),
    dict(P=A0 + 8 * 100), dict(P=A0 + 8 * 391), dict(P=A0 - 4),         # A meets P
    dict(status=A0), dict(status=A0 + 8 * 391), dict(status=D0), dict(status=D0 + 4 * 130 + 4 * 63),  # status meets A, or P
])
def test_apply_p_refuses(side, kw):
    assert _perm(side, **kw) == HIP_ERROR_INVALID_VALUE


@pytest.mark.parametrize("side", [0, 1])
@pytest.mark.parametrize("kw", [
    dict(), dict(a_bs=192), dict(p_bs=0), dict(p_bs=1), dict(length=0, P=None), dict(length=1 << 40), dict(trans=1), dict(status=R0),
    dict(P=A0 + 8 * 392), dict(status=A0 + 8 * 392), dict(A=None, P=None),
])
def test_apply_p_accepts(side, kw):
    assert _perm(side, batch=0, **kw) == 0


def test_apply_p_empty_members_need_nothing():
    for side in (0, 1):
        assert _perm(side, nrows=0, A=None, P=None) == 0 and _perm(side, ncols=0, A=None, P=None, stride=0) == 0


def test_python_wrappers_are_bound():
    assert m4ri_amd.plan_perm_batch(64, 64, False) == 0 and m4ri_amd.plan_perm_batch(-1, 3, True) == -1
    with pytest.raises(RuntimeError):
        m4ri_amd.copy_block_batch_dev(D0, 1, 64, 0, 1, A0, 1, 64, 0, 0, 64, 64, 1)   # d_col 1 + 64 columns: two words, stride 1
    with pytest.raises(RuntimeError):
        m4ri_amd.submatrix_batch_dev(D0, 1, 64, A0, 1, 64, 0, 1, 64, 65, 1)          # the same on A's side
    with pytest.raises(RuntimeError):
        m4ri_amd.concat_batch_dev(D0, 1, 64, A0, 1, 64, 64, R0, 1, 64, 1, 64, 1)     # 65 columns in a stride of 1
    with pytest.raises(RuntimeError):
        m4ri_amd.stack_batch_dev(D0, 1, 64, A0, 1, 32, 32, R0, 1, 33, 33, 64, 2)     # 65 rows in members 64 words apart
    with pytest.raises(RuntimeError):
        m4ri_amd.extract_tri_batch_dev(D0, 1, 64, A0, 1, 64, 64, 64, 1, True, diag=3)
    with pytest.raises(RuntimeError):
        m4ri_amd.apply_p_left_batch_dev(A0, 1, 64, 64, 64, 1, 0, 64, 64)             # no P
    with pytest.raises(RuntimeError):
        m4ri_amd.apply_p_right_batch_dev(A0, 1, 64, 64, 64, 1, 0, 64, 64)
    m4ri_amd.copy_block_batch_dev(D0, 1, 64, 0, 0, A0, 1, 64, 0, 0, 64, 64, 0)
    m4ri_amd.submatrix_batch_dev(D0, 1, 64, A0, 2, 128, 0, 13, 64, 77, 0)
    m4ri_amd.concat_batch_dev(D0, 2, 128, A0, 1, 64, 64, R0, 1, 64, 64, 64, 0)
    m4ri_amd.stack_batch_dev(D0, 1, 128, A0, 1, 64, 64, R0, 1, 64, 64, 64, 0)
    m4ri_amd.extract_tri_batch_dev(D0, 1, 64, A0, 1, 64, 64, 64, 0, False, diag=1, rank=R0, stream=0)
    m4ri_amd.apply_p_left_batch_dev(A0, 1, 64, 64, 64, 0, D0, 64, 64, trans=True, status=R0)
    m4ri_amd.apply_p_right_batch_dev(A0, 1, 64, 64, 64, 0, D0, 64, 64)
