"""m4ri_amd_echelonize_batch_dev's host side, without a GPU: the path boundaries of m4ri_amd_plan_echelonize_batch (the entry
point's single source of truth for them) and the argument checks, which run before any HIP call."""
import ctypes

import pytest

import m4ri_amd

HIP_ERROR_INVALID_VALUE = 1
LDS_BUDGET = 160 * 1024
CAP_BYTES = 512 * 1024


def _path1_lds_bytes(nrows, ncols):
    """What path 1 declares: rows padded to an odd number of words, a 4-byte row index (16-byte aligned), two flag words per 64 rows."""
    width = (ncols + 63) // 64
    ldw = width if width % 2 else width + 1
    return nrows * ldw * 8 + ((nrows * 4 + 15) & ~15) + 2 * ((nrows + 63) // 64) * 8


def test_wave_path_boundary():
    P = m4ri_amd.plan_echelonize_batch
    for m, n in [(1, 1), (7, 5), (32, 32), (63, 40), (64, 1), (1, 64), (64, 64)]:
        assert P(m, n) == 0, (m, n)
    assert P(65, 64) == 1 and P(64, 65) == 1 and P(65, 65) == 1


@pytest.mark.parametrize("ncols", [65, 130, 300, 1000, 1024, 1280, 3488])
def test_lds_path_boundary(ncols):
    P = m4ri_amd.plan_echelonize_batch
    last = max(n for n in range(65, 25000) if _path1_lds_bytes(n, ncols) <= LDS_BUDGET)
    assert P(last, ncols) == 1 and P(last + 1, ncols) == 2, (last, ncols)


def test_lds_path_pinned_shapes():
    P = m4ri_amd.plan_echelonize_batch
    assert P(1024, 1024) == 1 and P(1168, 1024) == 1 and P(1169, 1024) == 2
    assert P(1088, 1088) == 1 and P(1089, 1089) == 2          # the largest square in LDS
    for m, n in [(100, 300), (256, 256), (300, 130), (512, 1000)]:
        assert P(m, n) == 1, (m, n)
    assert P(1100, 1100) == 2 and P(768, 3488) == 2


def test_global_path_cap():
    P = m4ri_amd.plan_echelonize_batch
    assert P(2048, 2048) == 2 and P(2049, 2048) == 3 and P(2048, 2049) == 3   # 2048 x 32 words = the cap
    words = CAP_BYTES // 8
    assert P(1, words * 64) == 2 and P(1, words * 64 + 1) == 3                # one row: the cap, then one word more
    assert P(words, 64 + 1) == 3 and P(words // 2, 65) == 2
    assert P(1 << 40, 1 << 40) == 3
    assert P(-1, 5) == -1 and P(5, -1) == -1


def _call(A=1 << 20, stride=1, a_bs=64, nrows=64, ncols=64, batch=2, full=0, rank=1 << 21, pivots=None):
    return m4ri_amd.lib().m4ri_amd_echelonize_batch_dev(A, stride, a_bs, nrows, ncols, batch, full, rank, pivots, None)


@pytest.mark.parametrize("kw", [
    dict(nrows=-1), dict(ncols=-1), dict(batch=-1), dict(stride=-1), dict(a_bs=-1),
    dict(ncols=65, stride=1),                                  # stride < width
    dict(nrows=10, ncols=130, stride=2, a_bs=19),             # overlapping members: need (10 - 1) * 2 + 3 = 21
    dict(nrows=10, ncols=130, stride=3, a_bs=28),             # (10 - 1) * 3 + 3 = 30
    dict(rank=None),                                           # rank == NULL with batch > 0
    dict(rank=None, nrows=0),
])
def test_invalid_arguments(kw):
    """Rejected before any HIP call: the pointers are not device memory (and this machine may have no GPU at all)."""
    assert _call(**kw) == HIP_ERROR_INVALID_VALUE


def test_batch_zero_is_success():
    assert _call(batch=0, A=None, rank=None) == 0
    assert _call(batch=0, nrows=5000, ncols=5000, stride=79, a_bs=0, A=None, rank=None) == 0


def test_python_wrappers_are_bound():
    assert m4ri_amd.plan_echelonize_batch(64, 64) == 0
    with pytest.raises(RuntimeError):
        m4ri_amd.echelonize_batch_dev(1 << 20, 0, 0, 4, 4, 1, 0, 1 << 21)   # stride 0 < width 1
