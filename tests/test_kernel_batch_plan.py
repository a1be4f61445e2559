"""m4ri_amd_kernel_left_batch_dev's host side, without a GPU: the path boundaries of m4ri_amd_plan_kernel_batch and the argument
checks, which run before any HIP call."""
import pytest

import m4ri_amd

HIP_ERROR_INVALID_VALUE = 1
LDS_BUDGET = 160 * 1024


def _path1_lds_bytes(m, n):
    """What path 1 declares: m rows of words(n) words padded to an odd count, a 4-byte row index (16-byte aligned), three flag words
    per 64 of max(m, n), and two int32 tables of n entries (the swap rule's arrangement, the pivot row / basis column of a column)."""
    W = (n + 63) // 64
    ldw = W if W % 2 else W + 1
    return m * ldw * 8 + ((m * 4 + 15) & ~15) + 3 * ((max(m, n) + 63) // 64) * 8 + 8 * n


def test_wave_path_boundary():
    P = m4ri_amd.plan_kernel_batch
    for m, n in [(0, 0), (1, 1), (7, 5), (5, 7), (64, 64), (64, 1), (1, 64), (0, 64), (64, 0)]:
        assert P(m, n) == 0, (m, n)
    assert P(65, 64) == 1 and P(64, 65) == 1 and P(65, 65) == 1 and P(65, 1) == 1 and P(1, 65) == 1


@pytest.mark.parametrize("n", [1, 64, 65, 200, 512, 1024, 3000])
def test_lds_path_boundary_in_m(n):
    P = m4ri_amd.plan_kernel_batch
    last = max(m for m in range(0, 25000) if _path1_lds_bytes(m, n) <= LDS_BUDGET)
    assert last >= 64
    assert P(last, n) == 1 and P(last + 1, n) == 2, (last, n)


@pytest.mark.parametrize("m", [0, 1, 100, 1024])
def test_lds_path_boundary_in_n(m):
    P = m4ri_amd.plan_kernel_batch
    last = max(n for n in range(0, 25000) if _path1_lds_bytes(m, n) <= LDS_BUDGET)
    assert last >= 1024
    assert P(m, last) == 1 and P(m, last + 1) == 2, (m, last)


def test_1024_square_on_path1():
    assert _path1_lds_bytes(1024, 1024) <= LDS_BUDGET
    assert m4ri_amd.plan_kernel_batch(1024, 1024) == 1


def test_one_by_one_path_and_negative_sizes():
    P = m4ri_amd.plan_kernel_batch
    assert P(2000, 2000) == 2 and P(1 << 40, 1 << 40) == 2 and P(1, 1 << 40) == 2 and P(1 << 40, 1) == 2
    assert P(-1, 5) == -1 and P(5, -1) == -1 and P(-1, -1) == -1


def _kernel(A=1 << 20, a_stride=1, a_bs=64, m=64, n=64, R=1 << 22, r_stride=1, r_bs=64, kc=64, batch=2, rank=1 << 21):
    return m4ri_amd.lib().m4ri_amd_kernel_left_batch_dev(A, a_stride, a_bs, m, n, R, r_stride, r_bs, kc, batch, rank, None)


@pytest.mark.parametrize("kw", [
    dict(m=-1), dict(n=-1), dict(kc=-1), dict(batch=-1),
    dict(a_stride=-1), dict(a_bs=-1), dict(r_stride=-1), dict(r_bs=-1),
    dict(kc=65),                                               # kc > n
    dict(m=0, n=10, kc=11),
    dict(n=65, kc=1, a_stride=1, a_bs=200, r_bs=200),          # A's stride < words(n)
    dict(n=100, kc=65, a_stride=2, r_stride=1, a_bs=200, r_bs=200),  # R's stride < words(kc)
    dict(n=100, kc=70, a_stride=2, r_stride=2, a_bs=200, r_bs=199),  # overlapping R members: need (100 - 1) * 2 + 2 = 200
    dict(n=100, kc=10, a_stride=2, r_stride=3, a_bs=200, r_bs=297),  # (100 - 1) * 3 + 1 = 298
    dict(R=1 << 20),                                           # R at A
    dict(R=(1 << 20) + 8 * 100),                               # R starts inside A's members (2 x 64 words)
    dict(R=(1 << 20) - 8 * 100),                               # R's members run into A's first member
    dict(R=(1 << 20) + 8 * 127, batch=2),                      # R starts at A's last word
    dict(rank=None),                                           # rank == NULL with batch > 0
    dict(rank=None, m=0, n=0, kc=0),
    dict(A=None),                                              # NULL data pointers with non-empty members
    dict(R=None),
    dict(R=None, m=0),                                         # m = 0: R is still n x kc
])
def test_invalid_arguments(kw):
    """Rejected before any HIP call: the pointers are not device memory (and this machine may have no GPU at all)."""
    assert _kernel(**kw) == HIP_ERROR_INVALID_VALUE


def test_batch_zero_is_success():
    assert _kernel(batch=0, A=None, R=None, rank=None) == 0
    assert _kernel(batch=0, m=5000, n=5000, kc=5000, a_stride=79, r_stride=79, a_bs=0, r_bs=0, A=None, R=None, rank=None) == 0
    assert _kernel(batch=0, R=1 << 20, rank=None) == 0  # nothing to write: no overlap to reject


def test_python_wrappers_are_bound():
    assert m4ri_amd.plan_kernel_batch(64, 64) == 0
    with pytest.raises(RuntimeError):
        m4ri_amd.kernel_left_batch_dev(1 << 20, 0, 0, 4, 4, 1 << 22, 1, 4, 4, 1, 1 << 21)   # A's stride 0 < width 1
    with pytest.raises(RuntimeError):
        m4ri_amd.kernel_left_batch_dev(1 << 20, 1, 4, 4, 4, 1 << 22, 1, 4, 5, 1, 1 << 21)   # kc > n
