"""The host side of m4ri_amd_weight_batch_dev, m4ri_amd_mismatch_batch_dev and m4ri_amd_row_span_batch_dev, without a GPU: the
NumPy expectations of tests/reduce_cases.py against the reference, the path boundaries of m4ri_amd_plan_reduce_batch and the
argument checks, which run before any HIP call."""
import ctypes

import numpy as np
import pytest

import m4ri_amd
import reduce_cases as rc
from m4ri_amd.mzd import Mzd, MzdPtr

HIP_ERROR_INVALID_VALUE = 1
PATH0, PATH1 = "M4RI_AMD_REDUCE_BATCH_PATH0_MAX", "M4RI_AMD_REDUCE_BATCH_PATH1_MAX"
INT32_MAX = (1 << 31) - 1


def test_numpy_expectations_match_the_reference(reference):
    """mzd_equal, mzd_is_zero and mzd_first_zero_row on a dozen small matrices: zero, single bits at the corners and around a word
    boundary, random."""
    L = reference.L
    L.mzd_is_zero.restype, L.mzd_is_zero.argtypes = ctypes.c_int, [MzdPtr]
    L.mzd_first_zero_row.restype, L.mzd_first_zero_row.argtypes = ctypes.c_int, [MzdPtr]
    nrows, ncols = 37, 130
    mats = [np.zeros((nrows, ncols), dtype=np.uint8)] + [rc.single(nrows, ncols, r, c) for (r, c) in rc.corners(nrows, ncols)]
    mats += [Mzd.random(nrows, ncols, s).to_bits() for s in range(4)]
    low = Mzd.random(nrows, ncols, 9).to_bits()
    low[20:] = 0  # zero rows at the bottom, non-zero ones above
    mats.append(low)
    assert len(mats) >= 12
    Ms = [Mzd.from_bits(b) for b in mats]
    for i, (b, M) in enumerate(zip(mats, Ms)):
        assert (rc.end_nonzero(b) == 0) == bool(L.mzd_is_zero(M.ptr)), i
        assert rc.end_nonzero(b) == L.mzd_first_zero_row(M.ptr), i
        assert (rc.total(b) == 0) == bool(L.mzd_is_zero(M.ptr)), i
        assert (rc.first_nonzero(b) == nrows) == bool(L.mzd_is_zero(M.ptr)), i
        for j, (b2, M2) in enumerate(zip(mats, Ms)):
            assert (rc.first_mismatch(b, b2) == -1) == bool(L.mzd_equal(M.ptr, M2.ptr)), (i, j)
            assert rc.first_mismatch(b, b2) == (-1 if np.array_equal(b, b2) else rc.first_nonzero(b ^ b2)), (i, j)


def test_numpy_expectations_on_plain_cases():
    b = np.array([[1, 1, 0], [0, 1, 0], [1, 0, 0], [0, 0, 0]], dtype=np.uint8)
    assert rc.row_weights(b).tolist() == [2, 1, 1, 0] and rc.total(b) == 4
    assert rc.lightest(b) == (0 << 32) | 3 and rc.lightest(b[:3]) == (1 << 32) | 1  # two rows tied: the first
    assert rc.first_nonzero(b) == 0 and rc.end_nonzero(b) == 3 and rc.first_nonzero(b[3:]) == 1 and rc.end_nonzero(b[3:]) == 0
    assert rc.first_mismatch(b, b) == -1 and rc.first_mismatch(b, b ^ rc.single(4, 3, 2, 2) ^ rc.single(4, 3, 3, 0)) == 2
    e = np.zeros((0, 5), dtype=np.uint8)
    assert rc.lightest(e) == -1 and rc.total(e) == 0 and rc.first_nonzero(e) == 0 and rc.end_nonzero(e) == 0 and rc.first_mismatch(e, e) == -1
    z = np.zeros((5, 0), dtype=np.uint8)
    assert rc.lightest(z) == 0 and rc.first_nonzero(z) == 5 and rc.end_nonzero(z) == 0 and rc.first_mismatch(z, z) == -1


# ---- the plan ---------------------------------------------------------------------------------------------------------------------------

def _w0():
    """The path-0 bound in words per row, found by scanning the widths at 64 rows."""
    P = m4ri_amd.plan_reduce_batch
    return max(w for w in range(1, 65) if P(64, 64 * w) == 0)


def _d1():
    """The path-1 bound as the largest square (in steps of 64) not on path 2."""
    P = m4ri_amd.plan_reduce_batch
    return max(d for d in range(64, 8193, 64) if P(d, d) != 2)


def test_wave_path_boundary():
    P, W0 = m4ri_amd.plan_reduce_batch, _w0()
    assert 1 <= W0 <= 16
    for w in range(1, 65):  # ONE boundary: nothing above it comes back
        assert (P(64, 64 * w) == 0) == (w <= W0), w
        assert (P(1, 64 * w) == 0) == (w <= W0), w
    for s in [(1, 1), (64, 1), (64, 64 * W0), (1, 64 * W0), (63, 64 * W0 - 1), (0, 0), (0, 5), (5, 0), (0, 1 << 40), (1 << 40, 0)]:
        assert P(*s) == 0, s
    for s in [(65, 1), (65, 64 * W0), (64, 64 * W0 + 1), (1, 64 * W0 + 1), (65, 65)]:
        assert P(*s) in (1, 2), s


def test_block_path_boundary():
    P, D1 = m4ri_amd.plan_reduce_batch, _d1()
    assert 64 < D1 < 8192
    for d in range(128, 8193, 64):  # ONE boundary
        assert (P(d, d) == 1) == (d <= D1), d
        assert (P(d, d) == 2) == (d > D1), d
    T1 = D1 * D1 // 64  # words of the largest path-1 square; the bound itself lies in [T1, words of the next square)
    assert P(T1, 64) == 1 and P(65, 64 * (T1 // 65)) == 1
    for s in [(D1 + 64, D1 + 64), (1 << 20, 1 << 20), (1 << 40, 1), (1, 1 << 40), (1 << 40, 1 << 40), (65536, 65536), (5000, 3000)]:
        assert P(*s) == 2, s


def test_plan_ignores_the_override_variables(monkeypatch):
    W0, D1 = _w0(), _d1()
    for name in (PATH0, PATH1):
        for v in ("0", "1", "16", "1073741824", "junk", "-5"):
            monkeypatch.setenv(name, v)
            assert (_w0(), _d1()) == (W0, D1), (name, v)
        monkeypatch.delenv(name)


def test_negative_sizes():
    P = m4ri_amd.plan_reduce_batch
    assert P(-1, 5) == -1 and P(5, -1) == -1 and P(-1, -1) == -1 and P(-1, 1 << 40) == -1


# ---- the argument checks ----------------------------------------------------------------------------------------------------------------
# A: 2 members of 64 x 64 (64 words each) at A0, B likewise at B0; the outputs far away at O0.
A0, B0, O0 = 1 << 20, 1 << 24, 1 << 28


def _weight(A=A0, a_stride=1, a_bs=64, B=B0, b_stride=1, b_bs=64, nrows=64, ncols=64, batch=2, total=O0, row_weight=O0 + 4096, lightest=O0 + 8192):
    return m4ri_amd.lib().m4ri_amd_weight_batch_dev(A, a_stride, a_bs, B, b_stride, b_bs, nrows, ncols, batch, total, row_weight, lightest, None)


def _mismatch(A=A0, a_stride=1, a_bs=64, B=B0, b_stride=1, b_bs=64, nrows=64, ncols=64, batch=2, first_row=O0):
    return m4ri_amd.lib().m4ri_amd_mismatch_batch_dev(A, a_stride, a_bs, B, b_stride, b_bs, nrows, ncols, batch, first_row, None)


def _span(A=A0, a_stride=1, a_bs=64, nrows=64, ncols=64, batch=2, first_nonzero=O0, end_nonzero=O0 + 4096):
    return m4ri_amd.lib().m4ri_amd_row_span_batch_dev(A, a_stride, a_bs, nrows, ncols, batch, first_nonzero, end_nonzero, None)


COMMON_BAD = [
    dict(nrows=-1), dict(ncols=-1), dict(batch=-1), dict(a_stride=-1), dict(a_bs=-1),
    dict(a_stride=0),                                        # below words(64) = 1
    dict(ncols=65, a_bs=200),                                # a_stride 1 < words(65) = 2
    dict(A=None),                                            # a NULL operand with non-empty members
    dict(nrows=INT32_MAX + 1, a_bs=0),
]
COMMON_GOOD = [
    dict(), dict(a_bs=0), dict(A=None), dict(a_stride=7, a_bs=3),   # a_bs is free: A is only read
    dict(nrows=INT32_MAX, a_bs=0),
    dict(nrows=0, A=None, a_stride=0), dict(ncols=0, A=None, a_stride=0),
]


@pytest.mark.parametrize("kw", COMMON_BAD + [
    dict(b_stride=-1), dict(b_bs=-1), dict(b_stride=0), dict(ncols=65, a_stride=2, a_bs=200, b_bs=200),
    dict(B=None, b_stride=-1), dict(B=None, b_bs=-1),
    dict(total=None, row_weight=None, lightest=None),        # no output at all
    dict(total=A0), dict(total=A0 + 8 * 127),                # total[0] on A's first / last word
    dict(total=A0 - 8), dict(lightest=A0 - 8),               # two entries: the second is A's first word
    dict(row_weight=A0 - 4 * 127),                           # 128 entries: the last one lies in A's first word
    dict(row_weight=B0 + 8 * 127), dict(lightest=B0 + 8 * 64), dict(total=B0 + 8 * 100),
    dict(total=A0 + 8 * 63, a_bs=0),                         # one shared A: its span is one member
])
def test_weight_invalid_arguments(kw):
    """Rejected before any HIP call: the pointers are not device memory (and this machine may have no GPU at all)."""
    assert _weight(**kw) == HIP_ERROR_INVALID_VALUE


@pytest.mark.parametrize("kw", COMMON_GOOD + [
    dict(B=None), dict(B=None, b_stride=0, b_bs=0), dict(b_bs=0), dict(A=A0, B=A0),
    dict(total=None), dict(row_weight=None), dict(lightest=None), dict(total=None, row_weight=None), dict(row_weight=None, lightest=None),
    dict(ncols=65, a_stride=2, b_stride=2, a_bs=200, b_bs=200),
])
def test_weight_batch_zero_is_success(kw):
    """Legal arguments: shown with batch = 0, which returns before any HIP call."""
    assert _weight(**dict(kw, batch=0)) == 0


@pytest.mark.parametrize("kw", [
    dict(total=A0 + 8 * 128), dict(total=A0 - 16), dict(lightest=A0 - 16), dict(row_weight=A0 - 4 * 128), dict(row_weight=B0 + 8 * 128),
    dict(total=A0 + 8 * 64, a_bs=0), dict(B=None, total=B0),
])
def test_weight_outputs_beside_the_operands_are_accepted(kw):
    """The accepted neighbours of the overlaps above, one element further out: an output that ends where an operand starts, or starts
    where it ends.  Shown with batch = 0, as every legal call is here."""
    assert _weight(**dict(kw, batch=0)) == 0


@pytest.mark.parametrize("kw", COMMON_BAD + [
    dict(b_stride=-1), dict(b_bs=-1), dict(b_stride=0), dict(B=None), dict(first_row=None),
    dict(first_row=A0 + 8 * 127), dict(first_row=A0 - 4), dict(first_row=B0), dict(first_row=B0 + 8 * 127 + 4),
])
def test_mismatch_invalid_arguments(kw):
    assert _mismatch(**kw) == HIP_ERROR_INVALID_VALUE


@pytest.mark.parametrize("kw", COMMON_GOOD + [dict(b_bs=0), dict(B=A0), dict(B=None), dict(first_row=A0 - 8), dict(first_row=B0 + 8 * 128)])
def test_mismatch_batch_zero_is_success(kw):
    assert _mismatch(**dict(kw, batch=0)) == 0


@pytest.mark.parametrize("kw", COMMON_BAD + [
    dict(first_nonzero=None, end_nonzero=None), dict(first_nonzero=A0 + 8 * 5), dict(end_nonzero=A0 - 4), dict(end_nonzero=A0 + 8 * 127 + 4),
])
def test_row_span_invalid_arguments(kw):
    assert _span(**kw) == HIP_ERROR_INVALID_VALUE


@pytest.mark.parametrize("kw", COMMON_GOOD + [dict(first_nonzero=None), dict(end_nonzero=None), dict(end_nonzero=A0 - 8), dict(end_nonzero=A0 + 8 * 128)])
def test_row_span_batch_zero_is_success(kw):
    assert _span(**dict(kw, batch=0)) == 0


def test_python_wrappers_are_bound():
    assert m4ri_amd.plan_reduce_batch(1, 1) == 0 and m4ri_amd.plan_reduce_batch(-1, 3) == -1
    with pytest.raises(RuntimeError):
        m4ri_amd.weight_batch_dev(A0, 1, 64, 0, 0, 0, 64, 64, 2)                          # no output
    with pytest.raises(RuntimeError):
        m4ri_amd.weight_batch_dev(A0, 0, 64, 0, 0, 0, 64, 64, 2, total=O0)                # A's stride 0 < width 1
    with pytest.raises(RuntimeError):
        m4ri_amd.mismatch_batch_dev(A0, 1, 64, 0, 1, 64, 64, 64, 2, O0)                   # B is required
    with pytest.raises(RuntimeError):
        m4ri_amd.row_span_batch_dev(A0, 1, 64, 64, 64, 2)                                 # no output
    m4ri_amd.weight_batch_dev(A0, 1, 64, 0, 0, 0, 64, 64, 0, total=O0)                    # batch = 0: success, nothing touched
    m4ri_amd.weight_batch_dev(A0, 1, 64, B0, 1, 64, 64, 64, 0, row_weight=O0, lightest=O0 + 4096, stream=0)
    m4ri_amd.mismatch_batch_dev(A0, 1, 64, B0, 1, 64, 64, 64, 0, O0, stream=0)
    m4ri_amd.row_span_batch_dev(A0, 1, 64, 64, 64, 0, end_nonzero=O0)
    m4ri_amd.row_span_batch_dev(A0, 1, 64, 64, 64, 0, first_nonzero=O0, stream=0)
