"""The single-matrix device entry points of include/m4ri_amd.h, called the way a caller with device-resident data calls them:
through m4ri_amd.lib(), on device buffers the test owns, against the CPU oracle, bit for bit.

Every operand sits in a frame (tests/dev_frame.py): pattern-filled guard rows before and after it, pattern-filled padding words
between its width and its stride, and three layouts -- `even` (what the host shim gives), `odd` (odd stride, the base 8- but not
16-byte aligned) and `wide` (stride = width + 3).  After the call the whole buffer is read back: the valid bits must be the
oracle's, every word outside the operand's rows and words [0, width) must be unchanged, and the bits beyond the last column
must be what the function's header comment says.  The shapes are the smallest that reach each path: the 64-row and 64-column
TRSM base kernels over two and three workgroups, the 512-row block inverses with a ragged last block, a non-zero `cutoff`,
two solves and a trtri in flight on three streams, two right-hand solves and two trtri on two, the column gather on rows wider
than 64 KiB, and each of the three update kernels of m4ri_amd_process_rows_dev."""
import ctypes

import numpy as np
import pytest
import torch

import dev_frame as df
import elim_cases as ec
import m4ri_amd
from dev_frame import LAYOUTS, Frame
from m4ri_amd.mzd import Mzd
from test_ple_oracle import _make

pytestmark = pytest.mark.gpu
INVALID = 1  # hipErrorInvalidValue


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    assert m4ri_amd.lib().m4ri_amd_device_count() >= 1, "no HIP device visible: the gpu tests have nothing to run on"
    m4ri_amd.init(0)
    torch.cuda.set_device(0)


def _call(name, *args):
    rc = getattr(m4ri_amd.lib(), name)(*args)
    assert rc == 0, (name, rc)


def _i32(a):
    return np.ascontiguousarray(a, dtype=np.int32)


# ---- triangular solves ----------------------------------------------------------------------------------------------------

LEFT = [(64, 4097), (37, 8256),                       # the 64-row base kernel on 65 and 129 words: 2 and 3 workgroups, the last partial
        (65, 130), (512, 64), (513, 200), (1100, 70)]  # one inverted block, a ragged second block, three blocks
RIGHT = [(257, 64), (700, 33), (1, 64),                # the 64-column base kernel on 2 and 3 workgroups of 256 rows, and on one row
         (300, 130), (70, 513), (129, 1100)]


def _triangles(n, upper, seed, right):
    """Random (diagonal and other triangle junk), every bit set, and exactly one bit at the far corner.  The right-hand oracle
    wants the unit diagonal present, as tests/test_gpu_trsm.py sets it."""
    corner = df.one_bit(n, n, 0, n - 1) if upper else df.one_bit(n, n, n - 1, 0)
    out = [("random", Mzd.random(n, n, seed)), ("ones", df.ones(n, n)), ("corner", corner)]
    return [(k, df.unit_diag(T)) for k, T in out] if right else out


def _solve(oracle, side, upper, T, B, layout, cutoff=0, stream=0, seed=1, want=None, dirty=False):
    """dirty: T and B framed with pattern bits beyond their last column (systems of at most 64 rows / columns ignore both)."""
    name = f"trsm_{'upper' if upper else 'lower'}_{side}"
    if want is None:
        want = getattr(oracle, name)(T, B.copy())
    fT, fB = Frame(T, layout, seed, dirty_tail=dirty).upload(), Frame(B, layout, seed + 1, dirty_tail=dirty).upload()
    _call(f"m4ri_amd_{name}_dev", fT.ptr, fT.stride, fB.ptr, fB.stride, B.nrows, B.ncols, cutoff, stream)
    torch.cuda.synchronize()
    return want, fT, fB


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("upper", [False, True], ids=["lower", "upper"])
@pytest.mark.parametrize("mb,nb", LEFT)
def test_trsm_left(oracle, mb, nb, upper, layout):
    """B <- T^-1 B: B's valid bits the oracle's, its tail zero in and zero out (kept, whatever it is, up to 64 rows), its padding
    and guard rows and all of T untouched."""
    for kind, T in _triangles(mb, upper, 100 + mb, right=False):
        for bk, B in (("random", Mzd.random(mb, nb, 200 + nb)), ("identity", df.identity_like(mb, nb))):
            want, fT, fB = _solve(oracle, "left", upper, T, B, layout)
            fB.check(want, "zero", f"B ({kind} T, {bk} B)")
            fT.check_unchanged(f"T ({kind})")
            if mb <= 64:   # the base kernel: T's bits beyond column mb are not read, B's beyond column nb are kept
                want, fT, fB = _solve(oracle, "left", upper, T, B, layout, dirty=True)
                fB.check(want, "kept", f"B with a dirty tail ({kind} T with a dirty tail, {bk} B)")
                fT.check_unchanged(f"T ({kind})")


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("upper", [False, True], ids=["lower", "upper"])
@pytest.mark.parametrize("mb,nb", RIGHT)
def test_trsm_right(oracle, mb, nb, upper, layout):
    """B <- B T^-1, T nb x nb with its unit diagonal set."""
    for kind, T in _triangles(nb, upper, 300 + nb, right=True):
        for bk, B in (("random", Mzd.random(mb, nb, 400 + mb)), ("identity", df.identity_like(mb, nb))):
            want, fT, fB = _solve(oracle, "right", upper, T, B, layout)
            fB.check(want, "zero", f"B ({kind} T, {bk} B)")
            fT.check_unchanged(f"T ({kind})")
            if nb <= 64:   # the base kernel, as above (at nb = 64 there is no tail: the same call again)
                want, fT, fB = _solve(oracle, "right", upper, T, B, layout, dirty=True)
                fB.check(want, "kept", f"B with a dirty tail ({kind} T with a dirty tail, {bk} B)")
                fT.check_unchanged(f"T ({kind})")


@pytest.mark.parametrize("upper", [False, True], ids=["lower", "upper"])
@pytest.mark.parametrize("side,mb,nb", [("left", 2049, 2100), ("right", 2100, 2049)])
def test_trsm_cutoff_is_a_hint(oracle, side, mb, nb, upper):
    """`cutoff` reaches every product of the recursion (five 512-row blocks, the last one row): 0, 64 and 1024 give the oracle's
    bits, in the even and the odd layout (one oracle solve serves all six calls: T and B do not depend on the layout).
    The oracle's right-hand substitution works bit by bit (11 s at 2100 x 2049), so its result for X T = B is taken from its
    left-hand solve of T^T X^T = B^T (tests/dev_frame.py; tests/test_dev_frame_cpu.py pins the two to each other)."""
    n = mb if side == "left" else nb
    T = Mzd.random(n, n, 500 + n)
    if side == "right":
        df.unit_diag(T)
    B = Mzd.random(mb, nb, 600 + nb)
    if side == "left":
        expect = (oracle.trsm_upper_left if upper else oracle.trsm_lower_left)(T, B.copy())
    else:
        expect = df.trsm_right_by_transposition(oracle, T, B, upper)
    for layout in ("even", "odd"):
        results = []
        for cutoff in (0, 64, 1024):
            want, fT, fB = _solve(oracle, side, upper, T, B, layout, cutoff=cutoff, want=expect)
            fB.check(want, "zero", f"{layout}, cutoff {cutoff}")
            fT.check_unchanged(f"T, {layout}, cutoff {cutoff}")
            results.append(fB.download())
        assert np.array_equal(results[0], results[1]) and np.array_equal(results[0], results[2]), layout


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("n", [2, 64, 65, 512, 513, 1100])
def test_trtri_upper(oracle, n, layout):
    """U <- U^-1: only the bits strictly above the diagonal change; the junk on and below it, the (dirty) bits beyond column n,
    the padding and the guard rows come back untouched."""
    for kind, U in (("random", Mzd.random(n, n, 700 + n)), ("ones", df.ones(n, n)), ("corner", df.one_bit(n, n, 0, n - 1))):
        want = oracle.trtri_upper(U.copy())
        strict = np.triu(np.ones((n, n), dtype=np.uint8), 1)
        assert np.array_equal(want.to_bits() & (1 - strict), U.to_bits() & (1 - strict))  # the oracle keeps diagonal and lower part
        f = Frame(U, layout, 7, dirty_tail=True).upload()
        _call("m4ri_amd_trtri_upper_dev", f.ptr, f.stride, n, 0)
        torch.cuda.synchronize()
        f.check(want, "kept", kind)


def test_solves_in_flight_on_two_streams_and_a_trtri_on_a_third(oracle):
    """Two left solves of different sizes share the per-device scratch, guarded by an event: issued on two streams with no host
    synchronisation between them (the scratch does not grow on this second round), both give the oracle's bits; then the same
    with a trtri on a third stream."""
    cases = [(1100, 200, False), (600, 4200, True)]
    ops = [(Mzd.random(mb, mb, 800 + mb), Mzd.random(mb, nb, 900 + nb), up) for mb, nb, up in cases]
    wants = [(oracle.trsm_upper_left if up else oracle.trsm_lower_left)(T, B.copy()) for T, B, up in ops]
    U = Mzd.random(700, 700, 77)
    want_u = oracle.trtri_upper(U.copy())
    streams = [torch.cuda.Stream() for _ in range(3)]

    def issue(with_trtri):
        frames = [(Frame(T, "odd", 3).upload(), Frame(B, "odd", 4).upload()) for T, B, _ in ops]
        fU = Frame(U, "odd", 5, dirty_tail=True).upload()
        torch.cuda.synchronize()  # the uploads ran on the null stream; torch's own streams do not wait for it
        for (fT, fB), (T, B, up), st in zip(frames, ops, streams):
            _call("m4ri_amd_trsm_upper_left_dev" if up else "m4ri_amd_trsm_lower_left_dev", fT.ptr, fT.stride, fB.ptr, fB.stride, B.nrows,
                  B.ncols, 0, st.cuda_stream)
        if with_trtri:
            _call("m4ri_amd_trtri_upper_dev", fU.ptr, fU.stride, U.nrows, streams[2].cuda_stream)
        torch.cuda.synchronize()
        return frames, fU

    issue(True)  # first round: the scratch grows here (growing synchronises the device)
    for with_trtri in (False, True):
        frames, fU = issue(with_trtri)
        for (fT, fB), want in zip(frames, wants):
            fB.check(want, "zero", f"B {fB.nrows} x {fB.ncols}")
            fT.check_unchanged("T")
        fU.check(want_u if with_trtri else None, "kept", "U")


def test_two_trtri_in_flight_on_two_streams(oracle):
    """Two inverses of different sizes, both above 512 rows (the product levels), share the trtri's per-device scratch, which is
    sized for the larger one: issued on two streams with no host synchronisation between them, after a round in which the scratch
    grew, both give the oracle's bits -- each call takes its turn on the scratch."""
    Us = [Mzd.random(n, n, 1000 + n) for n in (1300, 700)]
    wants = [oracle.trtri_upper(U.copy()) for U in Us]
    streams = [torch.cuda.Stream() for _ in Us]

    def issue():
        frames = [Frame(U, "odd", 6 + i, dirty_tail=True).upload() for i, U in enumerate(Us)]
        torch.cuda.synchronize()  # the uploads ran on the null stream; torch's own streams do not wait for it
        for f, U, st in zip(frames, Us, streams):
            _call("m4ri_amd_trtri_upper_dev", f.ptr, f.stride, U.nrows, st.cuda_stream)
        torch.cuda.synchronize()
        return frames

    issue()  # first round: the scratch grows here (growing synchronises the device)
    for f, want in zip(issue(), wants):
        f.check(want, "kept", f"U {f.nrows} x {f.ncols}")


def test_right_solves_in_flight_on_two_streams(oracle):
    """The right-hand solves share the same scratch and the same event as the left-hand ones: an upper and a lower solve with
    different triangles above 512 columns, on two streams, as above."""
    cases = [(300, 1100, True), (129, 600, False)]
    ops = [(df.unit_diag(Mzd.random(nb, nb, 1100 + nb)), Mzd.random(mb, nb, 1200 + mb), up) for mb, nb, up in cases]
    wants = [(oracle.trsm_upper_right if up else oracle.trsm_lower_right)(T, B.copy()) for T, B, up in ops]
    streams = [torch.cuda.Stream() for _ in ops]

    def issue():
        frames = [(Frame(T, "odd", 3).upload(), Frame(B, "odd", 4).upload()) for T, B, _ in ops]
        torch.cuda.synchronize()
        for (fT, fB), (T, B, up), st in zip(frames, ops, streams):
            _call("m4ri_amd_trsm_upper_right_dev" if up else "m4ri_amd_trsm_lower_right_dev", fT.ptr, fT.stride, fB.ptr, fB.stride, B.nrows,
                  B.ncols, 0, st.cuda_stream)
        torch.cuda.synchronize()
        return frames

    issue()  # first round: the scratch grows here
    for (fT, fB), want in zip(issue(), wants):
        fB.check(want, "zero", f"B {fB.nrows} x {fB.ncols}")
        fT.check_unchanged("T")


# ---- permutations -----------------------------------------------------------------------------------------------------------

def _wide_p(ncols, kind):
    """spread: transpositions near both ends and across the middle, so the touched words [lo, hi] are the whole row;
    tail: only words 8190 .. 8192 (as far as the row has them)."""
    P = np.arange(ncols, dtype=np.int32)
    if kind == "spread":
        P[0], P[1], P[63], P[ncols // 2 - 1], P[ncols - 130] = ncols - 1, ncols // 2, 64, ncols // 2 + 70, ncols - 2
    else:
        P[8190 * 64 + 5] = ncols - 1
        P[8190 * 64 + 70] = 8190 * 64 + 100
    return P


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("kind", ["spread", "tail"])
@pytest.mark.parametrize("m,n", [(3, 524352), (2, 524289), (5, 524288)])
def test_apply_p_right_on_rows_wider_than_64_kib(m, n, kind, layout):
    """Rows of 8193 words (a whole and a one-bit last word) take the gather from a copy of the rows in global memory; 8192 words
    is the last size that goes through LDS.  The reference is the NumPy gather of tests/dev_frame.py (pinned to the oracle in
    tests/test_dev_frame_cpu.py).  The loop over chunks of 4096 rows at this width needs a 268 MB operand: left out."""
    A = Mzd.random(m, n, 1000 + n)
    P = _wide_p(n, kind)
    bits = A.to_bits()
    for trans in (0, 1):
        want = df.pack_bits(df.apply_p_right_bits(bits, P, bool(trans)))
        f = Frame(A, layout, 11).upload()
        _call("m4ri_amd_apply_p_right_dev", f.ptr, f.stride, m, n, P.ctypes.data, n, trans, 0)
        f.check(want, "zero", f"trans {trans}")


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("m,n", [(70, 130), (200, 333)])
def test_apply_p_right_small(oracle, m, n, layout):
    rng = np.random.default_rng(m + n)
    A = Mzd.random(m, n, 5)
    P = _i32([rng.integers(i, n) for i in range(n)])
    for trans in (0, 1):
        want = A.copy()
        oracle.apply_p_right(want, P, bool(trans))
        f = Frame(A, layout, 12).upload()
        _call("m4ri_amd_apply_p_right_dev", f.ptr, f.stride, m, n, P.ctypes.data, n, trans, 0)
        f.check(want, "zero", f"trans {trans}")


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("m,n", [(70, 130), (200, 333)])
def test_apply_p_left(oracle, m, n, layout):
    """Whole rows of `width` words move: every row keeps its own tail bits, here zero."""
    rng = np.random.default_rng(m * 7 + n)
    A = Mzd.random(m, n, 6)
    P = _i32([rng.integers(i, m) for i in range(m)])
    for trans in (0, 1):
        want = A.copy()
        oracle.apply_p_left(want, P, bool(trans))
        f = Frame(A, layout, 13).upload()
        _call("m4ri_amd_apply_p_left_dev", f.ptr, f.stride, m, n, P.ctypes.data, m, trans, 0)
        f.check(want, "zero", f"trans {trans}")


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("m,n", [(70, 130), (200, 333)])
def test_apply_p_right_trans_tri(oracle, m, n, layout):
    """The column step that turns the oracle's PLE into the oracle's PLUQ (ple.c:50-60), on the PLE's first `rank` rows."""
    A = _make("lowrank", m, n, 40 + n)
    E, U = A.copy(), A.copy()
    r, _, Q = oracle.ple(E)
    ru, _, Qu = oracle.ple(U, pluq=True)
    assert r == ru and 0 < r < m and np.array_equal(Q, Qu) and not np.array_equal(E.valid_words(), U.valid_words())
    f = Frame(E, layout, 14).upload()
    Qh = _i32(Q)
    _call("m4ri_amd_apply_p_right_trans_tri_dev", f.ptr, f.stride, r, n, Qh.ctypes.data, 0)
    f.check(U, "zero")


# ---- echelon forms ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("kind", ["random", "lowrank"])
@pytest.mark.parametrize("full", [0, 1])
@pytest.mark.parametrize("m,n", [(70, 130), (200, 333), (333, 200), (513, 700)])
def test_echelonize(oracle, m, n, full, kind, layout):
    A = _make(kind, m, n, 2000 + 7 * m + n)
    want = A.copy()
    rank_o = oracle.echelonize(want, full)
    f = Frame(A, layout, 15).upload()
    rank = ctypes.c_int32(-1)
    _call("m4ri_amd_echelonize_dev", f.ptr, f.stride, m, n, full, ctypes.byref(rank), 0)
    assert rank.value == rank_o
    f.check(want, "zero")


@pytest.mark.parametrize("layout", LAYOUTS)
def test_echelonize_with_pivots_8192_words_apart(oracle, layout):
    """3 x 524352, reduced: the pivots sit in words 0, 4096 and 8192, so the column permutation at the end covers the whole
    8193-word row and runs the gather from global memory."""
    m, n = 3, 524352
    piv = [5, 4096 * 64 + 9, 8192 * 64 + 3]
    A = Mzd.random(m, n, 99)
    w = A.valid_words()
    for i, p in enumerate(piv):   # row i: zero before its pivot, a bit at it; the rows below it zero up to and at it
        w[i, : p // 64] = 0
        w[i, p // 64] &= ~np.uint64(0) << np.uint64(p % 64)
        w[i, p // 64] |= np.uint64(1) << np.uint64(p % 64)
        for j in range(i + 1, m):
            w[j, : p // 64 + 1] = 0
    want = A.copy()
    assert oracle.echelonize(want, 1) == 3
    f = Frame(A, layout, 16).upload()
    rank = ctypes.c_int32(-1)
    _call("m4ri_amd_echelonize_dev", f.ptr, f.stride, m, n, 1, ctypes.byref(rank), 0)
    assert rank.value == 3
    f.check(want, "zero")


# ---- systems, kernels, inverses -----------------------------------------------------------------------------------------------

SYSTEMS = [(70, 70, 65), (130, 70, 130), (70, 130, 33), (513, 513, 200)]


def _rhs(oracle, A, rows, k, consistent):
    B = Mzd(rows, k)
    src = oracle.mul(None, A, Mzd.random(A.ncols, k, 77), 0) if consistent else Mzd.random(A.nrows, k, 78)
    B.valid_words()[: A.nrows] = src.valid_words()
    return B


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("consistent", [True, False], ids=["consistent", "inconsistent"])
@pytest.mark.parametrize("kind", ["random", "lowrank"])
@pytest.mark.parametrize("m,n,k", SYSTEMS)
def test_solve_left(oracle, m, n, k, kind, consistent, layout):
    """A <- its PLUQ, B <- the solution, with the check on; both exactly as the oracle leaves them (an inconsistent system
    returns -1 with B holding the reference's intermediate state, solve.c:81-121), nothing around either written."""
    A = _make(kind, m, n, 3000 + 7 * m + n)
    B = _rhs(oracle, A, max(m, n), k, consistent)
    Ao, Bo = A.copy(), B.copy()
    want = oracle.solve_left(Ao, Bo, True)
    if not consistent and kind == "lowrank":
        assert want == -1
    fA, fB = Frame(A, layout, 21).upload(), Frame(B, layout, 22).upload()
    ret = ctypes.c_int(7)
    _call("m4ri_amd_solve_left_dev", fA.ptr, fA.stride, m, n, fB.ptr, fB.stride, B.nrows, k, 0, 1, ctypes.byref(ret), 0)
    assert ret.value == want
    fA.check(Ao, "zero", "A")
    fB.check(Bo, "zero", "B")


@pytest.mark.parametrize("layout", LAYOUTS)
def test_solve_left_refuses_dirty_padding_rows_without_touching_anything(oracle, layout):
    """m < n with the check on: a set bit in rows m+1 .. n-1 of B returns -1 before anything is computed -- every byte of A and
    B is as before."""
    m, n, k = 70, 130, 33
    A = _make("random", m, n, 5)
    B = _rhs(oracle, A, n, k, True)
    B.valid_words()[n - 1, 0] = np.uint64(4)
    assert oracle.solve_left(A.copy(), B.copy(), True) == -1
    fA, fB = Frame(A, layout, 23).upload(), Frame(B, layout, 24).upload()
    ret = ctypes.c_int(7)
    _call("m4ri_amd_solve_left_dev", fA.ptr, fA.stride, m, n, fB.ptr, fB.stride, n, k, 0, 1, ctypes.byref(ret), 0)
    assert ret.value == -1
    fA.check_unchanged("A")
    fB.check_unchanged("B")


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("consistent", [True, False], ids=["consistent", "inconsistent"])
@pytest.mark.parametrize("m,n,k", SYSTEMS)
def test_pluq_solve_left(oracle, m, n, k, consistent, layout):
    """From the oracle's decomposition: A is read only."""
    A = _make("lowrank", m, n, 4000 + 7 * m + n)
    B = _rhs(oracle, A, max(m, n), k, consistent)
    Ad = A.copy()
    r, P, Q = oracle.ple(Ad, pluq=True, recursive=True)
    Bo = B.copy()
    want = oracle.pluq_solve_left(Ad, r, P, Q, Bo, True)
    assert want == (0 if consistent else -1)
    fA, fB = Frame(Ad, layout, 25).upload(), Frame(B, layout, 26).upload()
    ret = ctypes.c_int(7)
    Ph, Qh = _i32(P), _i32(Q)
    _call("m4ri_amd_pluq_solve_left_dev", fA.ptr, fA.stride, m, n, r, Ph.ctypes.data, Qh.ctypes.data, fB.ptr, fB.stride, B.nrows, k, 0, 1,
          ctypes.byref(ret), 0)
    assert ret.value == want
    fA.check_unchanged("A")
    fB.check(Bo, "zero", "B")


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("kind", ["random", "lowrank"])
@pytest.mark.parametrize("m,n", [(70, 70), (130, 70), (70, 130), (513, 513)])
def test_kernel_left_pluq(oracle, m, n, kind, layout):
    """A <- its PLUQ (checked against the oracle's A); R, zeroed by the caller, <- the basis; R untouched when the rank is n."""
    A = _make(kind, m, n, 5000 + 7 * m + n)
    Ao = A.copy()
    r, Ro = oracle.kernel_left_pluq(Ao)
    kc = max(1, n - r)
    fA, fR = Frame(A, layout, 27).upload(), Frame(Mzd(n, kc), layout, 28).upload()
    rank = ctypes.c_int32(-1)
    _call("m4ri_amd_kernel_left_pluq_dev", fA.ptr, fA.stride, m, n, fR.ptr, fR.stride, 0, ctypes.byref(rank), 0)
    assert rank.value == r
    fA.check(Ao, "zero", "A")
    if Ro is None:
        fR.check_unchanged("R")
    else:
        fR.check(Ro, "zero", "R")


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("singular", [False, True], ids=["invertible", "singular"])
@pytest.mark.parametrize("n", [65, 200, 513])
def test_inv(oracle, n, singular, layout):
    """Binv is written whole, tail included (dirty on entry, zero on return); A is read only."""
    for seed in range(1, 60):
        A = Mzd.random(n, n, 6000 + n + seed)
        if oracle.echelonize(A.copy(), 0) == n:
            break
    else:
        pytest.fail("no invertible matrix among 59 seeds")
    if singular:
        A.valid_words()[n // 2] = A.valid_words()[0]
    want = oracle.inv(A)
    fA, fB = Frame(A, layout, 29).upload(), Frame(Mzd.random(n, n, 3), layout, 30, dirty_tail=True).upload()
    _call("m4ri_amd_inv_dev", fB.ptr, fB.stride, fA.ptr, fA.stride, n, 0)
    torch.cuda.synchronize()
    fA.check_unchanged("A")
    fB.check(want, "zero", "Binv")


# ---- the table primitives ---------------------------------------------------------------------------------------------------

# Which update kernel m4ri_amd_process_rows_dev launches (elim.hip): the scalar apply_tables_kernel<word> unless M's base is
# 16-byte aligned, `stride`, `block` = startcol / 64 and `wide` = width - block are even and every table's base is 16-byte
# aligned with an even stride; then apply_tables_slab_kernel<word2> when ntables >= 2 and wide / 2 >= 64, else
# apply_tables_kernel<word2>.  (M layout, table layouts, width, block, ntables) -> id says which and why.
PROCESS = [
    ("scalar:odd-stride", "odd", "even", 131, 2, 2),
    ("scalar:odd-block", "even", "even", 133, 1, 3),
    ("scalar:odd-wide", "even", "even", 133, 2, 2),
    ("scalar:one-table-odd-t_stride", "even", "one-odd", 132, 2, 3),
    ("vec2:one-table", "even", "even", 132, 2, 1),
    ("vec2:one-table-wide/2=130", "even", "even", 260, 0, 1),
    ("vec2:three-tables-wide/2=63", "even", "even", 128, 2, 3),
    ("slab:two-tables-wide/2=64", "even", "even", 130, 2, 2),
    ("slab:six-tables-wide/2=64", "even", "even", 128, 0, 6),
    ("slab:two-tables-wide/2=65", "even", "even", 130, 0, 2),
    ("slab:six-tables-wide/2=65", "even", "even", 134, 4, 6),
    ("slab:two-tables-wide/2=71", "even", "even", 142, 0, 2),
    ("slab:six-tables-wide/2=71", "even", "even", 144, 2, 6),
]


def _expected_kernel(fM, fTs, block, wide, nt):
    """The TEST's copy of the launcher's choice (the switch that would force it is read once per process and must not be set):
    it guards the case ids against a mistake in a case's own numbers, not against a change of the launcher's condition.  What
    shows that a `slab:` or `scalar:` case really runs that kernel is the mutation check: with the slab arithmetic of
    apply_tables_slab_kernel broken only `slab:` cases fail, with the apply_tables_kernel<word> launch broken only `scalar:` ones.
    Repeat it when the conditions in elim.hip change."""
    vec = fM.ptr % 16 == 0 and fM.stride % 2 == 0 and block % 2 == 0 and wide % 2 == 0 and all(f.ptr % 16 == 0 and f.stride % 2 == 0 for f in fTs)
    return "scalar" if not vec else ("slab" if nt >= 2 and wide // 2 >= 64 else "vec2")


@pytest.mark.parametrize("count", [1, 255, 257, 1000])
@pytest.mark.parametrize("name,m_layout,t_layout,width,block,nt", PROCESS, ids=[p[0] for p in PROCESS])
def test_process_rows(oracle, name, m_layout, t_layout, width, block, nt, count):
    """Tables and L from the oracle's make_table, rows [k, k + count) processed: only the words [block, width) of those rows may
    change, and they must be the oracle's."""
    k = 2 * nt + 1
    nrows, ncols = k + count + 2, 64 * width - 3
    startcol = 64 * block + 7
    M = Mzd.random(nrows, ncols, 31 * width + count)
    Ts, Ls = ec.tables_for(oracle.make_table, M, 0, startcol, k, nt)
    kb = ec.split_k(k, nt)
    want = M.copy()
    oracle.process_rows(want, k, k + count, startcol, k, Ts, Ls)
    fM = Frame(M, m_layout, 41).upload()
    fTs = [Frame(T, "odd" if (t_layout == "one-odd" and t == 1) else "even", 50 + t).upload() for t, T in enumerate(Ts)]
    assert _expected_kernel(fM, fTs, block, width - block, nt) == name.split(":")[0]
    dL = [torch.from_numpy(_i32(l)).cuda() for l in Ls]
    idx = torch.zeros(6 * count, dtype=torch.int32, device="cuda")
    kbits = (ctypes.c_int32 * 6)(*kb)
    Tp = (ctypes.c_void_p * 6)(*[f.ptr for f in fTs])
    Ts_ = (ctypes.c_int64 * 6)(*[f.stride for f in fTs])
    Lp = (ctypes.c_void_p * 6)(*[l.data_ptr() for l in dL])
    _call("m4ri_amd_process_rows_dev", fM.ptr, fM.stride, width, k, k + count, startcol, nt, kbits, Tp, Ts_, Lp, idx.data_ptr(), 0)
    torch.cuda.synchronize()
    fM.check(want, "zero", name)
    for f in fTs:
        f.check_unchanged("table")
    after, before = fM.view(fM.download()), fM.view(fM.before)
    untouched = np.ones((nrows, width), dtype=bool)
    untouched[k:k + count, block:] = False
    assert np.array_equal(after[untouched], before[untouched])


def _jstar(k, r, m_rows):
    js, out = 0, np.zeros(1 << k, dtype=np.int32)
    for i in range(1, 1 << k):
        if r + ((i & -i).bit_length() - 1) >= m_rows:
            js = i
        out[i] = js
    return out


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("k,r", [(1, 19), (1, 20), (8, 5), (8, 15)], ids=["k1", "k1-stale", "k8", "k8-stale"])
@pytest.mark.parametrize("ncols,c", [(192, 130), (193, 192), (300, 70)], ids=["c-in-full-last-word", "c-in-one-bit-last-word", "c-inside"])
def test_make_table(oracle, ncols, c, k, r, layout):
    """Rows 1 .. 2^k - 1 of Tout, words c / 64 .. width - 1: the oracle's table; rows whose source row does not exist (r + k > 20)
    keep their content; row 0, the words before c / 64, the padding and the guard rows are not written."""
    m_rows = 20
    M = Mzd.random(m_rows, ncols, 8 + ncols)
    T0 = Mzd.random(1 << k, ncols, 9)
    want, Lw = T0.copy(), np.zeros(1 << k, dtype=np.int32)
    oracle.make_table(M, r, c, k, want, Lw)
    fM, fT = Frame(M, layout, 61).upload(), Frame(T0, layout, 62).upload()
    dj = torch.from_numpy(_jstar(k, r, m_rows)).cuda()
    _call("m4ri_amd_make_table_dev", fM.ptr, fM.stride, m_rows, ncols, r, c, k, fT.ptr, fT.ptr, fT.stride, dj.data_ptr(), 0)
    torch.cuda.synchronize()
    fM.check_unchanged("M")
    fT.check(want, "zero", "Tout")
    after, before = fT.view(fT.download()), fT.view(fT.before)
    assert np.array_equal(after[0], before[0]) and np.array_equal(after[:, : c // 64], before[:, : c // 64])


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("rows", [1, 300])
@pytest.mark.parametrize("ncols", [1, 64, 65, 4097])
def test_mask_tail(rows, ncols, layout):
    """Only the bits beyond column ncols of each row's last word change: they become zero."""
    M = Mzd.random(rows, ncols, 70 + ncols)
    f = Frame(M, layout, 63, dirty_tail=True).upload()
    _call("m4ri_amd_mask_tail_dev", f.ptr, f.stride, rows, ncols, 0)
    torch.cuda.synchronize()
    f.check(M, "zero")


@pytest.mark.parametrize("layout", LAYOUTS)
def test_make_table_from_a_separate_tin(oracle, layout):
    """Tin != Tout: the chain starts from Tin's row 0 and the rows whose source row does not exist (r + k > 20) are copied from
    Tin, tail included; Tin itself and Tout's row 0 are not written."""
    m_rows, ncols, r, c, k = 20, 300, 15, 70, 8
    M = Mzd.random(m_rows, ncols, 8 + ncols)
    Tin, Tout = Mzd.random(1 << k, ncols, 9), Mzd.random(1 << k, ncols, 10)
    want, Lw = Tin.copy(), np.zeros(1 << k, dtype=np.int32)
    oracle.make_table(M, r, c, k, want, Lw)   # the oracle works in place: on a copy of Tin
    stale = _jstar(k, r, m_rows) == np.arange(1 << k)
    assert stale[1:].any() and not stale[1:].all()
    home = c // 64
    want.valid_words()[0] = Tout.valid_words()[0]                  # row 0 and the words before c / 64 stay Tout's
    want.valid_words()[:, :home] = Tout.valid_words()[:, :home]
    fM, fI, fO = Frame(M, layout, 61).upload(), Frame(Tin, layout, 64, dirty_tail=True).upload(), Frame(Tout, layout, 65).upload()
    assert fI.stride == fO.stride
    dj = torch.from_numpy(_jstar(k, r, m_rows)).cuda()
    _call("m4ri_amd_make_table_dev", fM.ptr, fM.stride, m_rows, ncols, r, c, k, fI.ptr, fO.ptr, fO.stride, dj.data_ptr(), 0)
    torch.cuda.synchronize()
    fM.check_unchanged("M")
    fI.check_unchanged("Tin")
    after, tin = fO.view(fO.download()), fI.view(fI.before)
    outside_ok = np.array_equal(fO.download()[fO.outside], fO.before[fO.outside])
    assert outside_ok, "words around Tout changed"
    got = after.copy()
    got[:, -1] &= fO.mask
    assert np.array_equal(got, want.masked())
    tail = after[:, -1] & ~fO.mask
    rows = np.arange(1 << k)
    computed = ~stale & (rows > 0)
    assert np.all(tail[computed] == 0) and np.all(tail[0] == 0)                      # computed rows: masked; row 0: Tout's clean tail
    assert np.array_equal(tail[stale & (rows > 0)], (tin[:, -1] & ~fI.mask)[stale & (rows > 0)])   # copied rows: Tin's (dirty) tail


# ---- arguments refused before any HIP call -----------------------------------------------------------------------------------

def test_arguments_refused_before_any_hip_call():
    L = m4ri_amd.lib()
    f = Frame(Mzd.random(8, 8, 1), "even", 1).upload()
    P = np.zeros(8, dtype=np.int32)
    rank, ret = ctypes.c_int32(0), ctypes.c_int(0)
    for name in ("m4ri_amd_trsm_lower_left_dev", "m4ri_amd_trsm_upper_left_dev", "m4ri_amd_trsm_lower_right_dev", "m4ri_amd_trsm_upper_right_dev"):
        assert getattr(L, name)(f.ptr, f.stride, f.ptr, f.stride, -1, 8, 0, 0) == INVALID
        assert getattr(L, name)(f.ptr, f.stride, f.ptr, f.stride, 8, -1, 0, 0) == INVALID
        assert getattr(L, name)(f.ptr, f.stride, f.ptr, f.stride, 8, 8, -1, 0) == INVALID
    assert L.m4ri_amd_trtri_upper_dev(f.ptr, f.stride, -1, 0) == INVALID
    assert L.m4ri_amd_echelonize_dev(f.ptr, f.stride, 8, 8, 1, None, 0) == INVALID
    assert L.m4ri_amd_echelonize_dev(f.ptr, f.stride, -1, 8, 1, ctypes.byref(rank), 0) == INVALID
    assert L.m4ri_amd_apply_p_right_dev(f.ptr, f.stride, 8, 8, None, 8, 0, 0) == INVALID
    assert L.m4ri_amd_apply_p_left_dev(f.ptr, f.stride, 8, -1, P.ctypes.data, 8, 0, 0) == INVALID
    assert L.m4ri_amd_apply_p_right_trans_tri_dev(f.ptr, f.stride, 8, 8, None, 0) == INVALID
    assert L.m4ri_amd_solve_left_dev(f.ptr, f.stride, 8, 8, f.ptr, f.stride, 8, 8, 0, 1, None, 0) == INVALID
    assert L.m4ri_amd_solve_left_dev(f.ptr, f.stride, 8, 8, f.ptr, f.stride, 7, 8, 0, 1, ctypes.byref(ret), 0) == INVALID
    assert L.m4ri_amd_pluq_solve_left_dev(f.ptr, f.stride, 8, 8, 9, P.ctypes.data, P.ctypes.data, f.ptr, f.stride, 8, 8, 0, 1, ctypes.byref(ret), 0) == INVALID
    assert L.m4ri_amd_kernel_left_pluq_dev(f.ptr, f.stride, 8, 8, f.ptr, f.stride, 0, None, 0) == INVALID
    g, h = Frame(Mzd.random(8, 8, 2), "even", 2).upload(), Frame(Mzd(8, 8), "even", 3).upload()   # B / R of their own: a call that went
    assert L.m4ri_amd_solve_left_dev(f.ptr, f.stride, 8, 8, g.ptr, g.stride, 8, 8, -1, 1, ctypes.byref(ret), 0) == INVALID   # on would
    assert L.m4ri_amd_kernel_left_pluq_dev(f.ptr, f.stride, 8, 8, h.ptr, h.stride, -1, ctypes.byref(rank), 0) == INVALID    # factor A
    assert L.m4ri_amd_pluq_solve_left_dev(f.ptr, f.stride, 8, 8, 0, P.ctypes.data, P.ctypes.data, g.ptr, g.stride, 8, 8, -1, 1, ctypes.byref(ret), 0) == INVALID
    g.check_unchanged("B of a refused call")
    h.check_unchanged("R of a refused call")
    assert L.m4ri_amd_inv_dev(f.ptr, f.stride, f.ptr, f.stride, -1, 0) == INVALID
    assert L.m4ri_amd_process_rows_dev(f.ptr, f.stride, 1, 0, 8, 0, 7, None, None, None, None, None, 0) == INVALID
    assert L.m4ri_amd_process_rows_dev(f.ptr, f.stride, 1, 5, 4, 0, 1, None, None, None, None, None, 0) == INVALID
    assert L.m4ri_amd_make_table_dev(f.ptr, f.stride, 8, 8, 0, 0, 0, f.ptr, f.ptr, f.stride, None, 0) == INVALID
    assert L.m4ri_amd_make_table_dev(f.ptr, f.stride, 8, 0, 0, 0, 4, f.ptr, f.ptr, f.stride, None, 0) == INVALID
    f.check_unchanged("a refused call")
