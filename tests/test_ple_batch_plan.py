"""m4ri_amd_ple_batch_dev's and m4ri_amd_pluq_solve_left_batch_dev's host side, without a GPU: the path boundaries of
m4ri_amd_plan_ple_batch and m4ri_amd_plan_pluq_solve_batch and the argument checks, which run before any HIP call."""
import pytest

import m4ri_amd

HIP_ERROR_INVALID_VALUE = 1
LDS_BUDGET = 160 * 1024
CAP_WORDS = 512 * 1024 // 8


def _w(n):
    return (n + 63) // 64


def _pad16(x):
    return (x + 15) & ~15


def _ple_lds_bytes(nrows, ncols):
    """What path 1 of the decomposition declares: nrows rows of words(ncols) words padded to an odd count, three int32 arrays (the row
    index, P, Q) each rounded up to 16 bytes, and two flag words per 64 rows."""
    W = _w(ncols)
    ldw = W if W % 2 else W + 1
    return nrows * ldw * 8 + 2 * _pad16(nrows * 4) + _pad16(ncols * 4) + 2 * _w(nrows) * 8


def _solve_lds_bytes(m, n, k):
    """Path 1 of the solve: max(m, n) rows of words(k) words padded to an odd count, the row index, min(m, n) entries of P / Q, flags,
    and a word of A per row of A."""
    W, R = _w(k), max(m, n)
    ldw = W if W % 2 else W + 1
    return R * ldw * 8 + _pad16(R * 4) + _pad16(min(m, n) * 4) + 16 + m * 8


def test_ple_wave_path_boundary():
    P = m4ri_amd.plan_ple_batch
    for m, n in [(0, 0), (1, 1), (7, 5), (5, 7), (64, 64), (64, 1), (1, 64), (0, 64), (64, 0)]:
        assert P(m, n) == 0, (m, n)
    assert P(65, 64) == 1 and P(64, 65) == 1 and P(65, 65) == 1 and P(65, 1) == 1 and P(1, 65) == 1


@pytest.mark.parametrize("n", [1, 64, 65, 200, 512, 1024, 3000])
def test_ple_lds_path_boundary_in_rows(n):
    P = m4ri_amd.plan_ple_batch
    last = max(m for m in range(0, 25000) if _ple_lds_bytes(m, n) <= LDS_BUDGET)
    assert last >= 64
    assert P(last, n) == 1 and P(last + 1, n) == 2, (last, n)


@pytest.mark.parametrize("m", [1, 65, 100, 1024])
def test_ple_lds_path_boundary_in_columns(m):
    P = m4ri_amd.plan_ple_batch
    last = max(n for n in range(0, 45000) if _ple_lds_bytes(m, n) <= LDS_BUDGET)
    assert last >= 1024 and m * _w(last + 1) <= CAP_WORDS
    assert P(m, last) == 1 and P(m, last + 1) == 2, (m, last)


def test_ple_largest_square_on_path1():
    P = m4ri_amd.plan_ple_batch
    n = max(n for n in range(65, 3000) if P(n, n) == 1)
    assert _ple_lds_bytes(n, n) <= LDS_BUDGET < _ple_lds_bytes(n + 1, n + 1)
    assert n >= 1024 and P(n + 1, n + 1) == 2


def test_ple_cap_and_negative_sizes():
    P = m4ri_amd.plan_ple_batch
    assert P(1024, 4096) == 2 and P(1024, 4097) == 3               # 1024 x 64 words = 512 KiB
    assert P(2048, 2048) == 2 and P(2049, 2048) == 3
    assert P(CAP_WORDS, 64) == 2 and P(CAP_WORDS + 1, 64) == 3 and P(65, CAP_WORDS * 64 // 65) in (2, 3)
    assert P(1, CAP_WORDS * 64) == 2 and P(1, CAP_WORDS * 64 + 1) == 3
    assert P(1500, 1500) == 2 and P(3000, 3000) == 3 and P(1 << 40, 1 << 40) == 3
    assert P(-1, 5) == -1 and P(5, -1) == -1 and P(-1, -1) == -1


def test_solve_plan():
    S = m4ri_amd.plan_pluq_solve_batch
    for m, n, k in [(0, 0, 0), (1, 1, 1), (64, 64, 64), (64, 1, 64), (1, 64, 1), (64, 64, 0)]:
        assert S(m, n, k) == 0, (m, n, k)
    assert S(65, 64, 64) == 1 and S(64, 65, 64) == 1 and S(64, 64, 65) == 1
    for n, k in [(100, 1), (100, 200), (1000, 65), (300, 1024)]:
        last = max(m for m in range(n, 25000) if _solve_lds_bytes(m, n, k) <= LDS_BUDGET)
        assert S(last, n, k) == 1 and S(last + 1, n, k) == 2, (last, n, k)
        assert S(n, last, k) == (1 if _solve_lds_bytes(n, last, k) <= LDS_BUDGET else 2)
    assert S(1 << 40, 1, 1) == 2 and S(1, 1, 1 << 40) == 2
    assert S(-1, 1, 1) == -1 and S(1, -1, 1) == -1 and S(1, 1, -1) == -1
    assert S(1100, 1100, 130) == 1 and m4ri_amd.plan_solve_batch(1100, 1100, 130) == 2  # only B is staged


def _ple(A=1 << 20, stride=1, a_bs=64, nrows=64, ncols=64, batch=2, pluq=0, P=1 << 21, Q=1 << 22, rank=1 << 23):
    return m4ri_amd.lib().m4ri_amd_ple_batch_dev(A, stride, a_bs, nrows, ncols, batch, pluq, P, Q, rank, None)


@pytest.mark.parametrize("kw", [
    dict(nrows=-1), dict(ncols=-1), dict(batch=-1), dict(stride=-1), dict(a_bs=-1),
    dict(ncols=65, a_bs=200),                                  # stride 1 < words(65)
    dict(stride=0),
    dict(a_bs=63),                                             # overlapping members: need (64 - 1) * 1 + 1 = 64
    dict(nrows=100, ncols=100, stride=3, a_bs=298),            # (100 - 1) * 3 + 2 = 299
    dict(A=None),
    dict(rank=None),
    dict(rank=None, nrows=0, ncols=0),
    dict(P=None), dict(P=None, ncols=0),
    dict(Q=None), dict(Q=None, nrows=0),
    dict(pluq=1, Q=None),
])
def test_ple_invalid_arguments(kw):
    """Rejected before any HIP call: the pointers are not device memory (and this machine may have no GPU at all)."""
    assert _ple(**kw) == HIP_ERROR_INVALID_VALUE


def test_ple_batch_zero_is_success():
    assert _ple(batch=0, A=None, P=None, Q=None, rank=None) == 0
    assert _ple(batch=0, nrows=5000, ncols=5000, stride=79, a_bs=0, A=None, P=None, Q=None, rank=None) == 0


def _solve(A=1 << 20, a_stride=1, a_bs=64, m=64, n=64, rank=1 << 23, P=1 << 24, Q=1 << 25, B=1 << 22, b_stride=1, b_bs=64, k=64, batch=2,
           status=1 << 21):
    return m4ri_amd.lib().m4ri_amd_pluq_solve_left_batch_dev(A, a_stride, a_bs, m, n, rank, P, Q, B, b_stride, b_bs, k, batch, status, None)


@pytest.mark.parametrize("kw", [
    dict(m=-1), dict(n=-1), dict(k=-1), dict(batch=-1), dict(a_stride=-1), dict(a_bs=-1), dict(b_stride=-1), dict(b_bs=-1),
    dict(n=65, a_bs=200),                                      # A's stride < words(n)
    dict(k=65, b_bs=200),                                      # B's stride < words(k)
    dict(b_bs=63),                                             # overlapping B members
    dict(m=10, n=100, a_stride=2, a_bs=20, k=70, b_stride=2, b_bs=199),  # max(m, n) rows: (100 - 1) * 2 + 2 = 200
    dict(status=None), dict(rank=None), dict(P=None), dict(Q=None),
    dict(rank=None, m=0, n=0, k=0),
    dict(A=None), dict(B=None), dict(B=None, m=0),
    dict(B=1 << 20),                                           # B at A
    dict(B=(1 << 20) + 8 * 100),                               # B starts inside A's members (2 x 64 words)
    dict(B=(1 << 20) - 8 * 100),                               # B's members run into A's first member
    dict(B=(1 << 20) + 8 * 63, a_bs=0),                        # the shared A's last word
])
def test_solve_invalid_arguments(kw):
    assert _solve(**kw) == HIP_ERROR_INVALID_VALUE


def test_solve_batch_zero_is_success():
    assert _solve(batch=0, A=None, B=None, rank=None, P=None, Q=None, status=None) == 0
    assert _solve(batch=0, B=1 << 20, status=None) == 0  # nothing to write: no overlap to reject


def test_python_wrappers_are_bound():
    assert m4ri_amd.plan_ple_batch(64, 64) == 0 and m4ri_amd.plan_pluq_solve_batch(64, 64, 64) == 0
    with pytest.raises(RuntimeError):
        m4ri_amd.ple_batch_dev(1 << 20, 0, 4, 4, 4, 1, True, 1 << 21, 1 << 22, 1 << 23)         # stride 0 < width 1
    with pytest.raises(RuntimeError):
        m4ri_amd.ple_batch_dev(1 << 20, 1, 4, 4, 4, 1, False, 1 << 21, 1 << 22, 0)               # rank == NULL
    with pytest.raises(RuntimeError):
        m4ri_amd.pluq_solve_left_batch_dev(1 << 20, 1, 4, 4, 4, 1 << 23, 1 << 24, 1 << 25, 1 << 22, 0, 4, 4, 1, 1 << 21)  # B's stride 0
    m4ri_amd.ple_batch_dev(0, 1, 4, 4, 4, 0, True, 0, 0, 0)                                      # batch 0
