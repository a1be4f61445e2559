"""m4ri_amd_transpose_batch_dev's host side, without a GPU: the path boundaries of m4ri_amd_plan_transpose_batch and the argument
checks, which run before any HIP call."""
import pytest

import m4ri_amd

HIP_ERROR_INVALID_VALUE = 1
OVERRIDE = "M4RI_AMD_TRANSPOSE_BATCH_PATH1_MAX"


def _t1():
    """The path-1 bound, found by scanning the squares in steps of 64: the largest square not on path 2."""
    P = m4ri_amd.plan_transpose_batch
    return max(d for d in range(64, 2049, 64) if P(d, d) != 2)


def test_wave_path_boundary():
    P = m4ri_amd.plan_transpose_batch
    for s in [(0, 0), (1, 1), (64, 64), (64, 1), (1, 64), (0, 64), (63, 37)]:
        assert P(*s) == 0, s
    for s in [(65, 1), (1, 65), (65, 64), (64, 65), (65, 65)]:
        assert P(*s) in (1, 2), s


def test_block_path_boundary():
    P, T1 = m4ri_amd.plan_transpose_batch, _t1()
    assert T1 in range(64, 1025, 64)
    for d in range(64, 2049, 64):  # the scan found ONE boundary: nothing above it comes back
        assert (P(d, d) != 2) == (d <= T1), d
    sizes = sorted({1, 64, T1 - 1, T1} | ({65} if T1 > 64 else set()))
    for s in [(a, b) for a in sizes for b in sizes]:
        assert P(*s) == (1 if max(s) > 64 else 0), s
    for s in [(T1 + 1, 1), (1, T1 + 1), (T1 + 1, T1 + 1), (1025, 1025), (1025, 1), (4096, 64), (1 << 40, 1), (1, 1 << 40), (1 << 40, 1 << 40)]:
        assert P(*s) == 2, s


def test_plan_ignores_the_override_variable(monkeypatch):
    T1 = _t1()
    for v in ("64", "1024", "0", "junk", "100000"):
        monkeypatch.setenv(OVERRIDE, v)
        assert _t1() == T1, v


def test_negative_sizes():
    P = m4ri_amd.plan_transpose_batch
    assert P(-1, 5) == -1 and P(5, -1) == -1 and P(-1, -1) == -1 and P(-1, 1 << 40) == -1


A0, D0 = 1 << 20, 1 << 28


def _tr(D=D0, d_stride=1, d_bs=64, A=A0, a_stride=1, a_bs=64, nrows=64, ncols=64, batch=2):
    return m4ri_amd.lib().m4ri_amd_transpose_batch_dev(D, d_stride, d_bs, A, a_stride, a_bs, nrows, ncols, batch, None)


@pytest.mark.parametrize("kw", [
    dict(nrows=-1), dict(ncols=-1), dict(batch=-1), dict(d_stride=-1), dict(d_bs=-1), dict(a_stride=-1), dict(a_bs=-1),
    dict(ncols=65, a_stride=1, a_bs=200, d_bs=200),                     # a_stride < words(ncols) = 2
    dict(nrows=65, d_stride=1, a_bs=200, d_bs=200),                     # d_stride < words(nrows) = 2
    dict(a_stride=0), dict(d_stride=0),
    dict(nrows=100, ncols=50, a_bs=128, d_stride=3, d_bs=148),          # overlapping D members: need (50 - 1) * 3 + 2 = 149
    dict(d_bs=63),                                                      # (64 - 1) * 1 + 1 = 64
    dict(d_bs=0),
    dict(D=A0 + 8 * 100),                                               # D starts inside A's members (2 x 64 words)
    dict(D=A0 + 8 * 127),                                               # D starts at A's last word
    dict(D=A0 - 8 * 100),                                               # D's members run into A's first member
    dict(D=A0 - 8 * 127),                                               # D's last word is A's first
    dict(D=A0 + 8 * 63, a_bs=0),                                        # one shared A: its span is one member, D starts at its last word
    dict(D=None), dict(A=None),                                         # NULL data pointers with non-empty members
])
def test_invalid_arguments(kw):
    """Rejected before any HIP call: the pointers are not device memory (and this machine may have no GPU at all)."""
    assert _tr(**kw) == HIP_ERROR_INVALID_VALUE


@pytest.mark.parametrize("kw", [
    dict(nrows=100, ncols=50, a_bs=128, d_stride=3, d_bs=149),          # exactly (50 - 1) * 3 + 2
    dict(d_bs=64),
    dict(D=A0 + 8 * 128), dict(D=A0 - 8 * 128),                         # D's span touches A's span end to end
    dict(a_bs=0),                                                       # one A for every member
    dict(D=A0 + 8 * 64, a_bs=0),                                        # right behind the one shared A
    dict(D=None, A=None),
    dict(D=None, A=None, nrows=5000, ncols=7000, a_stride=110, d_stride=79, a_bs=0, d_bs=0),
    dict(D=A0 + 8),                                                     # nothing to write: no overlap to reject
    dict(D=A0),                                                         # in place, 64 x 64
])
def test_batch_zero_is_success(kw):
    """Legal arguments: shown with batch = 0, which returns before any HIP call."""
    assert _tr(batch=0, **kw) == 0


def _inplace(n, batch=2, **kw):
    w = (n + 63) // 64
    args = dict(D=A0, A=A0, d_stride=w, a_stride=w, d_bs=n * w, a_bs=n * w, nrows=n, ncols=n, batch=batch)
    args.update(kw)
    return _tr(**args)


def test_in_place_is_accepted_for_square_members_up_to_1024_only():
    """D == A is judged by the members' shape whatever the batch, so batch = 0 (which returns before any HIP call) shows the accepted
    side here; tests/test_gpu_transpose_batch.py runs it.  D near A is an overlap, which needs members to overlap: batch = 2."""
    assert _inplace(1024, batch=0) == 0 and _inplace(64, batch=0) == 0 and _inplace(130, batch=0) == 0 and _inplace(1, batch=0) == 0
    assert _inplace(1088, batch=0) == HIP_ERROR_INVALID_VALUE                         # above 1024
    assert _inplace(1088) == HIP_ERROR_INVALID_VALUE
    assert _inplace(64, nrows=64, ncols=63, batch=0) == HIP_ERROR_INVALID_VALUE
    assert _inplace(64, d_stride=2, d_bs=128, a_bs=128, batch=0) == HIP_ERROR_INVALID_VALUE
    assert _inplace(64, a_bs=65, batch=0) == HIP_ERROR_INVALID_VALUE
    assert _inplace(64, nrows=64, ncols=63) == HIP_ERROR_INVALID_VALUE               # not square
    assert _inplace(64, nrows=63, ncols=64) == HIP_ERROR_INVALID_VALUE
    assert _inplace(128, nrows=128, ncols=64, d_bs=256, a_bs=256) == HIP_ERROR_INVALID_VALUE
    assert _inplace(64, d_stride=2, d_bs=128, a_bs=128) == HIP_ERROR_INVALID_VALUE    # unequal strides
    assert _inplace(64, a_stride=2, d_bs=128, a_bs=128) == HIP_ERROR_INVALID_VALUE
    assert _inplace(64, d_bs=65) == HIP_ERROR_INVALID_VALUE                           # unequal batch strides
    assert _inplace(64, a_bs=65) == HIP_ERROR_INVALID_VALUE
    assert _inplace(64, D=A0 + 8) == HIP_ERROR_INVALID_VALUE                          # one word apart is no in-place call
    assert _inplace(1024, D=A0 + 8) == HIP_ERROR_INVALID_VALUE
    assert _inplace(64, d_bs=63, a_bs=63) == HIP_ERROR_INVALID_VALUE                  # in place, but the members overlap each other


def test_in_place_validity_ignores_the_override_variable(monkeypatch):
    for v in ("64", "1024"):
        monkeypatch.setenv(OVERRIDE, v)
        assert _inplace(1024, batch=0) == 0 and _inplace(1088, batch=0) == HIP_ERROR_INVALID_VALUE


def test_empty_members_need_no_pointers():
    """nrows = 0 or ncols = 0: nothing is touched, and the call returns before any HIP call whatever the batch."""
    assert _tr(nrows=0, D=None, A=None, batch=3) == 0
    assert _tr(ncols=0, D=None, A=None, batch=3) == 0
    assert _tr(nrows=0, ncols=0, D=None, A=None, batch=3) == 0
    assert _tr(nrows=0, D=A0, batch=3) == 0      # an empty member overlaps nothing
    assert _tr(ncols=0, d_bs=0, batch=3) == 0    # and empty members do not overlap each other


def test_python_wrappers_are_bound():
    assert m4ri_amd.plan_transpose_batch(64, 64) == 0 and m4ri_amd.plan_transpose_batch(-1, 3) == -1
    with pytest.raises(RuntimeError):
        m4ri_amd.transpose_batch_dev(D0, 1, 4, A0, 0, 4, 4, 4, 1)        # A's stride 0 < width 1
    with pytest.raises(RuntimeError):
        m4ri_amd.transpose_batch_dev(D0, 1, 70, A0, 1, 70, 70, 4, 1)     # D's stride 1 < words(70)
    m4ri_amd.transpose_batch_dev(D0, 1, 4, A0, 1, 4, 4, 4, 0)            # batch = 0: success, nothing touched
    m4ri_amd.transpose_batch_dev(D0, 1, 4, A0, 1, 4, 4, 4, 0, stream=0)
