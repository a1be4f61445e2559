"""m4ri_amd_mul_small_batch_op_dev's host side, without a GPU: the path boundaries of m4ri_amd_plan_mul_small_batch_op for every
(trans_a, trans_b) and the argument checks, which follow the STORED shapes of the operands (A l x m under trans_a, B n x l under
trans_b) and run before any HIP call."""
import itertools

import pytest

import m4ri_amd

HIP_ERROR_INVALID_VALUE = 1
HIP_ERROR_NOT_SUPPORTED = 801
OPS = [(0, 0), (0, 1), (1, 0), (1, 1)]
TRANSPOSED = OPS[1:]
OVERRIDE = "M4RI_AMD_MUL_SMALL_BATCH_PATH1_MAX"


def _d1op(ta, tb):
    """The path-1 bound of an op, found by scanning the cubes in steps of 64: the largest cube not on path 2."""
    P = m4ri_amd.plan_mul_small_batch_op
    return max(d for d in range(64, 1025, 64) if P(d, d, d, ta, tb) != 2)


@pytest.mark.parametrize("ta,tb", OPS)
def test_wave_path_boundary(ta, tb):
    P = m4ri_amd.plan_mul_small_batch_op
    for s in [(0, 0, 0), (1, 1, 1), (64, 64, 64), (64, 1, 1), (1, 64, 1), (1, 1, 64)]:
        assert P(*s, ta, tb) == 0, s
    for s in [(65, 64, 64), (64, 65, 64), (64, 64, 65)]:
        assert P(*s, ta, tb) in (1, 2), s


@pytest.mark.parametrize("ta,tb", OPS)
def test_block_path_boundary(ta, tb):
    P, D1 = m4ri_amd.plan_mul_small_batch_op, _d1op(ta, tb)
    assert D1 in (64, 128, 192, 256)
    for d in range(64, 1025, 64):  # the scan found ONE boundary: nothing above it comes back
        assert (P(d, d, d, ta, tb) != 2) == (d <= D1), d
    for s in itertools.product(sorted({1, 64, 65, D1 - 1, D1}), repeat=3):
        assert P(*s, ta, tb) == (1 if max(s) > 64 else 0), s
    for s in [(D1 + 1, 1, 1), (1, D1 + 1, 1), (1, 1, D1 + 1), (4096, 4096, 4096), (1 << 40, 1, 1), (1, 1 << 40, 1), (1, 1, 1 << 40)]:
        assert P(*s, ta, tb) == 2, s


def test_transposed_ops_share_one_bound():
    assert len({_d1op(ta, tb) for ta, tb in TRANSPOSED}) == 1


def test_untransposed_plan_is_the_existing_plan():
    P, Q = m4ri_amd.plan_mul_small_batch_op, m4ri_amd.plan_mul_small_batch
    sizes = (-1, 0, 1, 63, 64, 65, 127, 128, 129, 192, 193, 256, 257, 320, 1000)
    for s in itertools.product(sizes, repeat=3):
        assert P(*s, 0, 0) == Q(*s), s
    assert P(64, 64, 64) == Q(64, 64, 64) and P(300, 1, 1) == Q(300, 1, 1)  # the flags default to "not transposed"


@pytest.mark.parametrize("ta,tb", OPS)
def test_negative_sizes(ta, tb):
    P = m4ri_amd.plan_mul_small_batch_op
    assert P(-1, 5, 5, ta, tb) == -1 and P(5, -1, 5, ta, tb) == -1 and P(5, 5, -1, ta, tb) == -1 and P(-1, -1, -1, ta, tb) == -1


@pytest.mark.parametrize("ta,tb", OPS)
def test_plan_ignores_the_override_variable(monkeypatch, ta, tb):
    monkeypatch.delenv(OVERRIDE, raising=False)
    D1 = _d1op(ta, tb)
    for v in ("64", "256", "0", "junk"):
        monkeypatch.setenv(OVERRIDE, v)
        assert _d1op(ta, tb) == D1, v


A0, B0, C0 = 1 << 20, 1 << 24, 1 << 28


def _mul(ta, tb, C=C0, c_stride=1, c_bs=64, A=A0, a_stride=1, a_bs=64, B=B0, b_stride=1, b_bs=64, m=64, l=64, n=64, batch=2, add=0):
    return m4ri_amd.lib().m4ri_amd_mul_small_batch_op_dev(C, c_stride, c_bs, A, a_stride, a_bs, B, b_stride, b_bs, m, l, n, batch, ta, tb, add,
                                                          None)


# whatever the op: signs, C's own shape, NULL pointers, C on the 64 x 64 members of A or B (their stored shape is the same either way)
COMMON_INVALID = [
    dict(m=-1), dict(l=-1), dict(n=-1), dict(batch=-1),
    dict(c_stride=-1), dict(c_bs=-1), dict(a_stride=-1), dict(a_bs=-1), dict(b_stride=-1), dict(b_bs=-1),
    dict(a_stride=0), dict(b_stride=0), dict(c_stride=0),
    dict(m=64, n=64, c_bs=63),                                          # overlapping C members: need (64 - 1) * 1 + 1 = 64
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
]


@pytest.mark.parametrize("ta,tb", OPS)
@pytest.mark.parametrize("kw", COMMON_INVALID)
def test_invalid_arguments(ta, tb, kw):
    """Rejected before any HIP call: the pointers are not device memory (and there may be no GPU at all)."""
    assert _mul(ta, tb, **kw) == HIP_ERROR_INVALID_VALUE


def _strides(ta, tb, m, l, n):
    """The widths of the stored operands and of C: the smallest legal strides."""
    w = lambda x: (x + 63) // 64
    return w(m if ta else l), w(l if tb else n), w(n)


@pytest.mark.parametrize("ta,tb", OPS)
def test_widths_follow_the_stored_shapes(ta, tb):
    """(m, l, n) = (65, 129, 193): words 2, 3, 4, so every operand has its own width in either orientation."""
    m, l, n = 65, 129, 193
    sa, sb, sc = _strides(ta, tb, m, l, n)
    assert (sa, sb) == ((2 if ta else 3), (3 if tb else 4))
    big = dict(m=m, l=l, n=n, a_bs=1000, b_bs=1000, c_bs=1000, batch=0)
    assert _mul(ta, tb, a_stride=sa, b_stride=sb, c_stride=sc, **big) == 0
    assert _mul(ta, tb, a_stride=sa - 1, b_stride=sb, c_stride=sc, **big) == HIP_ERROR_INVALID_VALUE
    assert _mul(ta, tb, a_stride=sa, b_stride=sb - 1, c_stride=sc, **big) == HIP_ERROR_INVALID_VALUE
    assert _mul(ta, tb, a_stride=sa, b_stride=sb, c_stride=sc - 1, **big) == HIP_ERROR_INVALID_VALUE
    # overlapping C members: (m - 1) * c_stride + words(n) whatever the op
    assert _mul(ta, tb, m=50, l=64, n=100, b_stride=2, b_bs=200, c_stride=3, c_bs=148) == HIP_ERROR_INVALID_VALUE
    assert _mul(ta, tb, m=50, l=64, n=100, b_stride=2, b_bs=200, c_stride=3, c_bs=149, batch=0) == 0


@pytest.mark.parametrize("ta,tb", OPS)
def test_span_of_c_against_the_stored_row_counts(ta, tb):
    """m = 8, l = 40, n = 24, one word per row, members 64 words apart, batch 2: stored A ends (64 + rows - 1) words behind its start
    with rows = l under trans_a and m otherwise; stored B likewise with n under trans_b and l otherwise."""
    shape = dict(m=8, l=40, n=24, batch=2)
    ra, rb = (40 if ta else 8), (24 if tb else 40)
    for X, rows, other in ((A0, ra, "A"), (B0, rb, "B")):
        last = 64 + rows - 1  # the last word of the stored span
        assert _mul(ta, tb, C=X + 8 * last, **shape) == HIP_ERROR_INVALID_VALUE, other
        assert _mul(ta, tb, C=X + 8 * (last + 1), batch=0, **{k: v for k, v in shape.items() if k != "batch"}) == 0, other
        # one word behind the stored span is legal with a real batch too, shown where the call ends before any HIP call: m = 0 below
    # C's span is (64 + 8 - 1) + 1 = 72 words: it reaches the first word of an operand 71 words behind its start
    assert _mul(ta, tb, C=A0 - 8 * 71, **shape) == HIP_ERROR_INVALID_VALUE
    assert _mul(ta, tb, C=B0 - 8 * 71, **shape) == HIP_ERROR_INVALID_VALUE
    assert _mul(ta, tb, C=A0 - 8 * 72, **dict(shape, batch=0)) == 0


@pytest.mark.parametrize("ta,tb", TRANSPOSED)
def test_spans_differ_from_the_untransposed_call(ta, tb):
    """The same arguments are an overlap for one orientation and legal for the other: the check reads the stored row counts."""
    shape = dict(m=8, l=40, n=24, batch=1, a_bs=0, b_bs=0)
    if ta:  # stored A has 40 rows, not 8: its word 20 exists
        assert _mul(ta, tb, C=A0 + 8 * 20, **shape) == HIP_ERROR_INVALID_VALUE
        assert _mul(0, tb, C=A0 + 8 * 20, **dict(shape, batch=0)) == 0
    if tb:  # stored B has 24 rows, not 40: its word 30 does not exist
        assert _mul(ta, 0, C=B0 + 8 * 30, **shape) == HIP_ERROR_INVALID_VALUE
        assert _mul(ta, tb, C=B0 + 8 * 30, **dict(shape, batch=0)) == 0


@pytest.mark.parametrize("ta,tb", TRANSPOSED)
def test_transposed_beyond_the_bound_is_not_supported(monkeypatch, ta, tb):
    """Plan 2 with a transposed operand: hipErrorNotSupported before any HIP call (the pointers are not device memory)."""
    monkeypatch.delenv(OVERRIDE, raising=False)
    D1 = _d1op(ta, tb)
    for (m, l, n) in [(D1 + 1, 64, 64), (64, D1 + 1, 64), (64, 64, D1 + 1), (300, 300, 300)]:
        assert m4ri_amd.plan_mul_small_batch_op(m, l, n, ta, tb) == 2
        sa, sb, sc = _strides(ta, tb, m, l, n)
        kw = dict(m=m, l=l, n=n, a_stride=sa, b_stride=sb, c_stride=sc, a_bs=1 << 12, b_bs=1 << 12, c_bs=1 << 12)
        assert _mul(ta, tb, **kw) == HIP_ERROR_NOT_SUPPORTED, (m, l, n)
        assert _mul(ta, tb, **dict(kw, batch=0)) == 0                                   # nothing to do comes first
        assert _mul(ta, tb, **dict(kw, c_stride=sc - 1)) == HIP_ERROR_INVALID_VALUE     # and so does a bad argument
    monkeypatch.setenv(OVERRIDE, "64")  # the override moves the routing of the call, not the plan
    assert m4ri_amd.plan_mul_small_batch_op(65, 64, 64, ta, tb) == (1 if D1 > 64 else 2)
    sa, sb, sc = _strides(ta, tb, 65, 64, 64)
    assert _mul(ta, tb, m=65, a_stride=sa, b_stride=sb, c_stride=sc, a_bs=200, b_bs=200, c_bs=200) == HIP_ERROR_NOT_SUPPORTED


@pytest.mark.parametrize("ta,tb", OPS)
@pytest.mark.parametrize("kw", [
    dict(m=64, n=64, c_bs=64),
    dict(C=A0 + 8 * 128), dict(C=A0 - 8 * 128),                         # C's span touches A's span end to end
    dict(C=B0 + 8 * 64, b_bs=0),                                        # right behind the one shared B
    dict(A=B0, B=B0),                                                   # A == B: the Gram products A A^T and A^T A
    dict(A=B0 + 8 * 10, B=B0),                                          # A and B overlapping
    dict(C=None, A=None, B=None),
    dict(C=None, A=None, B=None, m=5000, l=5000, n=5000, a_stride=79, b_stride=79, c_stride=79, a_bs=0, b_bs=0, c_bs=0),
    dict(C=A0),                                                         # nothing to write: no overlap to reject
])
def test_batch_zero_is_success(ta, tb, kw):
    """Legal arguments: shown with batch = 0, which returns before any HIP call."""
    assert _mul(ta, tb, batch=0, **kw) == 0


@pytest.mark.parametrize("ta,tb", OPS)
def test_empty_members_need_no_pointers(ta, tb):
    """m = 0 or n = 0: C is empty, nothing is touched, and the call returns before any HIP call whatever the batch and the plan."""
    assert _mul(ta, tb, m=0, C=None, A=None, batch=3) == 0
    assert _mul(ta, tb, n=0, C=None, B=None, batch=3) == 0
    assert _mul(ta, tb, m=0, C=A0, batch=3) == 0  # an empty C overlaps nothing
    assert _mul(ta, tb, m=0, l=300, a_stride=5, b_stride=5, C=None, A=None, batch=3) == 0


def test_python_wrappers_are_bound():
    assert m4ri_amd.plan_mul_small_batch_op(64, 64, 64, trans_a=True, trans_b=True) == 0
    assert m4ri_amd.plan_mul_small_batch_op(65, 64, 64, trans_b=True) in (1, 2)
    with pytest.raises(RuntimeError):
        m4ri_amd.mul_small_batch_op_dev(C0, 1, 4, A0, 0, 4, B0, 1, 4, 4, 4, 4, 1, trans_a=True)   # A's stride 0 < width 1
    with pytest.raises(RuntimeError):  # stored B is 4 x 70: stride 1 < words(70)
        m4ri_amd.mul_small_batch_op_dev(C0, 1, 4, A0, 2, 8, B0, 1, 4, 4, 70, 4, 1, trans_b=True)
    m4ri_amd.mul_small_batch_op_dev(C0, 1, 4, A0, 2, 8, B0, 1, 70, 4, 70, 4, 0, add=True)         # untransposed B is 70 x 4: legal; batch = 0
    m4ri_amd.mul_small_batch_op_dev(C0, 1, 4, A0, 1, 70, B0, 2, 8, 4, 70, 4, 0, trans_a=True, trans_b=True, stream=0)
