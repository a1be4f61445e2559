"""m4ri_amd_solve_left_batch_dev's and m4ri_amd_inv_batch_dev's host side, without a GPU: the path boundaries of
m4ri_amd_plan_solve_batch (the single source of truth for both entry points) and the argument checks, which run before any HIP
call."""
import pytest

import m4ri_amd

HIP_ERROR_INVALID_VALUE = 1
LDS_BUDGET = 160 * 1024


def _path1_lds_bytes(m, n, k):
    """What path 1 declares: max(m, n) rows of words(n) + words(k) words padded to an odd count, a 4-byte row index (16-byte
    aligned), three flag words per 64 rows."""
    R = max(m, n)
    W = (n + 63) // 64 + (k + 63) // 64
    ldw = W if W % 2 else W + 1
    return R * ldw * 8 + ((R * 4 + 15) & ~15) + 3 * ((R + 63) // 64) * 8


def test_wave_path_boundary():
    P = m4ri_amd.plan_solve_batch
    for m, n, k in [(0, 0, 0), (1, 1, 1), (7, 5, 3), (5, 7, 64), (64, 64, 64), (64, 1, 1), (1, 64, 64), (64, 64, 0)]:
        assert P(m, n, k) == 0, (m, n, k)
    assert P(65, 64, 64) == 1 and P(64, 65, 64) == 1 and P(64, 64, 65) == 1 and P(65, 65, 65) == 1
    assert P(10, 10, 200) == 1


@pytest.mark.parametrize("n,k", [(65, 1), (100, 64), (256, 256), (300, 130), (512, 1000), (1000, 64), (64, 3000)])
def test_lds_path_boundary(n, k):
    P = m4ri_amd.plan_solve_batch
    last = max(m for m in range(65, 25000) if _path1_lds_bytes(m, n, k) <= LDS_BUDGET)
    assert last >= n
    assert P(last, n, k) == 1 and P(last + 1, n, k) == 2, (last, n, k)
    assert P(n // 2, n, k) == 1  # m < n: n rows, the padding rows included


def test_inverse_path_pinned():
    P = m4ri_amd.plan_solve_batch
    assert P(64, 64, 64) == 0 and P(65, 65, 65) == 1
    assert P(256, 256, 256) == 1 and P(768, 768, 768) == 1 and P(769, 769, 769) == 2
    assert _path1_lds_bytes(768, 768, 768) <= LDS_BUDGET < _path1_lds_bytes(769, 769, 769)


def test_one_by_one_path_and_negative_sizes():
    P = m4ri_amd.plan_solve_batch
    assert P(2000, 2000, 1) == 2 and P(1 << 40, 1 << 40, 1 << 40) == 2 and P(1, 1, 1 << 40) == 2
    assert P(-1, 5, 5) == -1 and P(5, -1, 5) == -1 and P(5, 5, -1) == -1


def _solve(A=1 << 20, a_stride=1, a_bs=64, m=64, n=64, B=1 << 22, b_stride=1, b_bs=64, k=64, batch=2, status=1 << 21, rank=None):
    return m4ri_amd.lib().m4ri_amd_solve_left_batch_dev(A, a_stride, a_bs, m, n, B, b_stride, b_bs, k, batch, status, rank, None)


def _inv(Binv=1 << 22, b_stride=1, b_bs=64, A=1 << 20, a_stride=1, a_bs=64, n=64, batch=2, rank=None):
    return m4ri_amd.lib().m4ri_amd_inv_batch_dev(Binv, b_stride, b_bs, A, a_stride, a_bs, n, batch, rank, None)


@pytest.mark.parametrize("kw", [
    dict(m=-1), dict(n=-1), dict(k=-1), dict(batch=-1),
    dict(a_stride=-1), dict(a_bs=-1), dict(b_stride=-1), dict(b_bs=-1),
    dict(n=65, a_stride=1),                                    # A's stride < width
    dict(k=65, b_stride=1),                                    # B's stride < width
    dict(m=10, n=20, k=130, b_stride=3, b_bs=59),              # overlapping B members (max(m, n) rows): need (20 - 1) * 3 + 3 = 60
    dict(m=30, n=20, k=130, b_stride=3, b_bs=89),              # (30 - 1) * 3 + 3 = 90
    dict(status=None),                                         # status == NULL with batch > 0
    dict(status=None, m=0, n=0),
    dict(A=None),                                              # NULL data pointers with non-empty members
    dict(B=None),
    dict(B=None, k=0, A=None, m=5),                            # A is 5 x 64: not empty
])
def test_solve_invalid_arguments(kw):
    """Rejected before any HIP call: the pointers are not device memory (and this machine may have no GPU at all)."""
    assert _solve(**kw) == HIP_ERROR_INVALID_VALUE


@pytest.mark.parametrize("kw", [
    dict(n=-1), dict(batch=-1), dict(b_stride=-1), dict(b_bs=-1), dict(a_stride=-1), dict(a_bs=-1),
    dict(n=65, a_stride=1, b_stride=2, b_bs=200, a_bs=200),    # A's stride < width
    dict(n=65, b_stride=1, a_stride=2, b_bs=200, a_bs=200),    # Binv's stride < width
    dict(n=100, b_stride=2, a_stride=2, b_bs=199, a_bs=400),   # overlapping Binv members: need (100 - 1) * 2 + 2 = 200
    dict(Binv=None), dict(A=None),
    dict(Binv=1 << 20, a_bs=128),                              # in place with another batch stride
    dict(Binv=1 << 20, b_stride=2, a_stride=1, b_bs=128, a_bs=128),  # in place with another stride
    dict(Binv=(1 << 20) + 8 * 100, b_bs=64, a_bs=64),          # Binv starts inside A's members (2 x 64 words)
])
def test_inv_invalid_arguments(kw):
    assert _inv(**kw) == HIP_ERROR_INVALID_VALUE


def test_batch_zero_is_success():
    assert _solve(batch=0, A=None, B=None, status=None) == 0
    assert _solve(batch=0, m=5000, n=5000, k=5000, a_stride=79, b_stride=79, a_bs=0, b_bs=0, A=None, B=None, status=None) == 0
    assert _inv(batch=0, Binv=None, A=None) == 0
    assert _inv(batch=0, n=5000, b_stride=79, a_stride=79, b_bs=0, a_bs=0, Binv=None, A=None) == 0


def test_python_wrappers_are_bound():
    assert m4ri_amd.plan_solve_batch(64, 64, 64) == 0
    with pytest.raises(RuntimeError):
        m4ri_amd.solve_left_batch_dev(1 << 20, 0, 0, 4, 4, 1 << 22, 1, 4, 4, 1, 1 << 21)   # A's stride 0 < width 1
    with pytest.raises(RuntimeError):
        m4ri_amd.inv_batch_dev(1 << 22, 0, 0, 1 << 20, 1, 4, 4, 1)                         # Binv's stride 0 < width 1
