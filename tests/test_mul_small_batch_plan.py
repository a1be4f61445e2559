"""m4ri_amd_mul_small_batch_dev's host side, without a GPU: the path boundaries of m4ri_amd_plan_mul_small_batch and the argument
checks, which run before any HIP call."""
import itertools

import pytest

import m4ri_amd

HIP_ERROR_INVALID_VALUE = 1


def _d1():
    """The path-1 bound, found by scanning the cubes in steps of 64: the largest cube not on path 2."""
    P = m4ri_amd.plan_mul_small_batch
    return max(d for d in range(64, 1025, 64) if P(d, d, d) != 2)


def test_wave_path_boundary():
    P = m4ri_amd.plan_mul_small_batch
    for s in [(0, 0, 0), (1, 1, 1), (64, 64, 64), (64, 1, 1), (1, 64, 1), (1, 1, 64)]:
        assert P(*s) == 0, s
    for s in [(65, 64, 64), (64, 65, 64), (64, 64, 65)]:
        assert P(*s) in (1, 2), s


def test_block_path_boundary():
    P, D1 = m4ri_amd.plan_mul_small_batch, _d1()
    assert D1 in (64, 128, 192, 256)
    for d in range(64, 1025, 64):  # the scan found ONE boundary: nothing above it comes back
        assert (P(d, d, d) != 2) == (d <= D1), d
    sizes = sorted({1, 64, 65, D1 - 1, D1})
    for s in itertools.product(sizes, repeat=3):
        if max(s) > 64:
            assert P(*s) == 1, s
        else:
            assert P(*s) == 0, s
    for s in [(D1 + 1, 1, 1), (1, D1 + 1, 1), (1, 1, D1 + 1), (4096, 4096, 4096), (1 << 40, 1, 1), (1, 1 << 40, 1), (1, 1, 1 << 40),
              (1 << 40, 1 << 40, 1 << 40)]:
        assert P(*s) == 2, s


def test_plan_ignores_the_override_variable(monkeypatch):
    D1 = _d1()
    for v in ("64", "256", "0", "junk"):
        monkeypatch.setenv("M4RI_AMD_MUL_SMALL_BATCH_PATH1_MAX", v)
        assert _d1() == D1, v


def test_negative_sizes():
    P = m4ri_amd.plan_mul_small_batch
    assert P(-1, 5, 5) == -1 and P(5, -1, 5) == -1 and P(5, 5, -1) == -1 and P(-1, -1, -1) == -1


A0, B0, C0 = 1 << 20, 1 << 24, 1 << 28


def _mul(C=C0, c_stride=1, c_bs=64, A=A0, a_stride=1, a_bs=64, B=B0, b_stride=1, b_bs=64, m=64, l=64, n=64, batch=2, add=0):
    return m4ri_amd.lib().m4ri_amd_mul_small_batch_dev(C, c_stride, c_bs, A, a_stride, a_bs, B, b_stride, b_bs, m, l, n, batch, add, None)


@pytest.mark.parametrize("kw", [
    dict(m=-1), dict(l=-1), dict(n=-1), dict(batch=-1),
    dict(c_stride=-1), dict(c_bs=-1), dict(a_stride=-1), dict(a_bs=-1), dict(b_stride=-1), dict(b_bs=-1),
    dict(l=65, a_stride=1, a_bs=200),                                   # a_stride < words(l) = 2
    dict(n=65, b_stride=1, c_stride=2, c_bs=200),                       # b_stride < words(n) = 2
    dict(n=65, b_stride=2, c_stride=1, b_bs=200, c_bs=200),             # c_stride < words(n) = 2
    dict(a_stride=0), dict(b_stride=0), dict(c_stride=0),
    dict(m=50, n=100, b_stride=2, b_bs=128, c_stride=3, c_bs=148),      # overlapping C members: need (50 - 1) * 3 + 2 = 149
    dict(m=64, n=64, c_bs=63),                                          # (64 - 1) * 1 + 1 = 64
    dict(c_bs=0),
    dict(C=A0),                                                         # C at A
    dict(C=A0 + 8 * 100),                                               # C starts inside A's members (2 x 64 words)
    dict(C=A0 + 8 * 127),                                               # C starts at A's last word
    dict(C=A0 - 8 * 100),                                               # C's members run into A's first member
    dict(C=B0),                                                         # C at B
    dict(C=B0 - 8 * 127),                                               # C's last word is B's first
    dict(C=B0 + 8 * 63, b_bs=0),                                        # one shared B: its span is one member, C starts at its last word
    dict(C=A0 + 8 * 63, a_bs=0),
    dict(C=None), dict(A=None), dict(B=None),                           # NULL data pointers with non-empty members
])
def test_invalid_arguments(kw):
    """Rejected before any HIP call: the pointers are not device memory (and this machine may have no GPU at all)."""
    assert _mul(**kw) == HIP_ERROR_INVALID_VALUE


@pytest.mark.parametrize("kw", [
    dict(m=50, n=100, b_stride=2, b_bs=128, c_stride=3, c_bs=149),      # exactly (50 - 1) * 3 + 2
    dict(m=64, n=64, c_bs=64),
    dict(C=A0 + 8 * 128), dict(C=A0 - 8 * 128),                         # C's span touches A's span end to end
    dict(C=B0 + 8 * 64, b_bs=0),                                        # right behind the one shared B
    dict(A=B0, B=B0),                                                   # A == B
    dict(A=B0 + 8 * 10, B=B0),                                          # A and B overlapping
    dict(C=None, A=None, B=None),
    dict(C=None, A=None, B=None, m=5000, l=5000, n=5000, a_stride=79, b_stride=79, c_stride=79, a_bs=0, b_bs=0, c_bs=0),
    dict(C=A0),                                                         # nothing to write: no overlap to reject
])
def test_batch_zero_is_success(kw):
    """Legal arguments: shown with batch = 0, which returns before any HIP call."""
    assert _mul(batch=0, **kw) == 0


def test_empty_members_need_no_pointers():
    """m = 0 or n = 0: C is empty, nothing is touched, and the call returns before any HIP call whatever the batch."""
    assert _mul(m=0, C=None, A=None, batch=3) == 0
    assert _mul(n=0, C=None, B=None, batch=3) == 0
    assert _mul(m=0, C=A0, batch=3) == 0  # an empty C overlaps nothing


def test_python_wrappers_are_bound():
    assert m4ri_amd.plan_mul_small_batch(64, 64, 64) == 0
    with pytest.raises(RuntimeError):
        m4ri_amd.mul_small_batch_dev(C0, 1, 4, A0, 0, 4, B0, 1, 4, 4, 4, 4, 1)       # A's stride 0 < width 1
    with pytest.raises(RuntimeError):
        m4ri_amd.mul_small_batch_dev(C0, 1, 70, A0, 1, 70, B0, 1, 70, 70, 4, 70, 1)  # B's and C's stride 1 < words(70)
    m4ri_amd.mul_small_batch_dev(C0, 1, 4, A0, 1, 4, B0, 1, 4, 4, 4, 4, 0, add=True)  # batch = 0: success, nothing touched
