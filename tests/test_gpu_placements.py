"""Every host entry point of the solver family against every PLACEMENT of the matrix it reads and writes
(m4ri_amd/csrc/mzd_api.hip: the placement rule).  Where a matrix lives decides how the drop-in layer binds it:

  host            a fresh non-window matrix, ragged ncols                          upload / download
  host-window     a ragged window of an unpinned parent (neighbours in its last word)   upload / masked download
  pinned          the pinned matrix itself, ragged ncols                           in place
  pinned-aligned  a 128-column window of a pinned parent                           in place
  pinned-ragged   a 130-column window of a pinned parent                           staged copy, masked copy back
  pinned-rows     a row window over the full width of a pinned parent with ragged ncols   in place, ragged

Parents are 200 x 320 (200 x 300 for pinned-rows); windows start at row 3 and, unless they span the full width, at column 64.
A square operand of placement pinned-rows is a 130-row window of a 200 x 130 parent: the 200 x 300 parent has no room for a
300 x 300 window.  Where two operands must agree in a dimension and one of them is pinned-aligned, both take 128: a
pinned-ragged partner is then on the word grid for that one combination.

Each case runs the oracle on identically shaped windows of a host copy of the same parents, runs the library, unpins, and then
compares the WHOLE parents bit for bit: the result, and that nothing outside the window moved.  Return values are compared too.
While a written parent is still pinned its status must be 2 (device copy newer), that of a parent only read 1.
mzd_apply_p_right_trans_tri has no oracle restatement: its expectation is the numpy replay of tests/test_gpu_ple.py."""
import numpy as np
import pytest

import m4ri_amd
from m4ri_amd.mzd import Mzd

pytestmark = pytest.mark.gpu

PLACEMENTS = ["host", "host-window", "pinned", "pinned-aligned", "pinned-ragged", "pinned-rows"]
READ_PLACEMENTS = ["host", "pinned", "pinned-ragged"]  # of the operands that are only read
ROWS = 70


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    assert m4ri_amd.lib().m4ri_amd_device_count() >= 1, "no HIP device visible: the gpu tests have nothing to run on"
    m4ri_amd.init(0)


def side(placement):
    """The size of a square operand of this placement."""
    return 128 if placement == "pinned-aligned" else 130


def width(placement):
    """The column count of an operand of this placement whose shape is free."""
    return {"pinned-aligned": 128, "pinned-rows": 300}.get(placement, 130)


class Placed:
    """One operand: `g` for the library (inside parent `gp`, pinned or not) and `o`, the same bits in a host copy, for the oracle."""

    def __init__(self, placement, rows, cols, seed, content=None):
        self.pinned = placement.startswith("pinned")
        if placement in ("host", "pinned"):
            parent, win = Mzd.random(rows, cols, seed), None
        elif placement == "pinned-rows":
            parent, win = Mzd.random(200, cols, seed), (3, 0, 3 + rows, cols)
        else:
            parent, win = Mzd.random(200, 320, seed), (3, 64, 3 + rows, 64 + cols)
        self.gp = parent
        self.g = parent.window(*win) if win else parent
        if content is not None:  # given bits (a decomposition): only the valid ones, the neighbours stay
            assert (content.nrows, content.ncols) == (rows, cols)
            v, c = self.g.valid_words(), content.masked()
            mask = np.uint64(self.g.high_bitmask)
            v[:, :-1] = c[:, :-1]
            v[:, -1] = (v[:, -1] & ~mask) | c[:, -1]
        self.op = Mzd(parent.nrows, parent.ncols, buf=parent.buf.copy())
        self.o = self.op.window(*win) if win else self.op
        assert (self.g.nrows, self.g.ncols) == (rows, cols) == (self.o.nrows, self.o.ncols)


def check(operands, call, expect):
    """Pin what is to be pinned, run `call` (the library) and `expect` (the oracle), unpin, and compare the whole parents.
    operands: [(Placed, written)].  Returns (got, want) for the caller to compare."""
    pinned = []
    try:
        for p, _ in operands:
            if p.pinned:
                m4ri_amd.pin(p.gp)
                pinned.append(p.gp)
        want = expect()
        got = call()
        for p, written in operands:
            if p.pinned:
                assert m4ri_amd.is_pinned(p.gp) == (2 if written else 1), "status of the pinned parent after the call"
                assert m4ri_amd.is_pinned(p.g) == (2 if written else 1)
    finally:
        for gp in pinned:
            m4ri_amd.unpin(gp)
    for k, (p, _) in enumerate(operands):
        assert m4ri_amd.is_pinned(p.gp) == 0
        assert np.array_equal(p.gp.valid_words(), p.op.valid_words()), "operand %d: the WHOLE parent must match the oracle's" % k
    return got, want


def same_ple(got, want):
    assert got[0] == want[0], ("rank", got[0], want[0])
    assert np.array_equal(got[1], want[1]), "P differs"
    assert np.array_equal(got[2], want[2]), "Q differs"


@pytest.mark.parametrize("pluq", [False, True], ids=["mzd_ple", "mzd_pluq"])
@pytest.mark.parametrize("placement", PLACEMENTS)
def test_ple(oracle, placement, pluq):
    a = Placed(placement, ROWS, width(placement), 11)
    got, want = check([(a, True)], lambda: m4ri_amd.mzd_ple(a.g, 0, "mzd_pluq" if pluq else "mzd_ple"), lambda: oracle.ple(a.o, pluq=pluq))
    same_ple(got, want)


@pytest.mark.parametrize("full", [0, 1])
@pytest.mark.parametrize("placement", PLACEMENTS)
def test_echelonize(oracle, placement, full):
    a = Placed(placement, ROWS, width(placement), 12)
    got, want = check([(a, True)], lambda: m4ri_amd.mzd_echelonize(a.g, full), lambda: oracle.echelonize(a.o, full))
    assert got == want


@pytest.mark.parametrize("trans", [False, True], ids=["plain", "trans"])
@pytest.mark.parametrize("placement", PLACEMENTS)
def test_apply_p_left(oracle, placement, trans):
    a = Placed(placement, ROWS, width(placement), 13)
    rng = np.random.default_rng(5)
    P = np.array([rng.integers(i, ROWS) for i in range(ROWS)], dtype=np.int32)
    check([(a, True)], lambda: m4ri_amd.mzd_apply_p_left(a.g, P, trans), lambda: oracle.apply_p_left(a.o, P, trans))


@pytest.mark.parametrize("trans", [False, True], ids=["plain", "trans"])
@pytest.mark.parametrize("placement", PLACEMENTS)
def test_apply_p_right(oracle, placement, trans):
    n = width(placement)
    a = Placed(placement, ROWS, n, 14)
    rng = np.random.default_rng(6)
    Q = np.array([rng.integers(i, n) for i in range(n)], dtype=np.int32)
    check([(a, True)], lambda: m4ri_amd.mzd_apply_p_right(a.g, Q, trans), lambda: oracle.apply_p_right(a.o, Q, trans))


@pytest.mark.parametrize("placement", PLACEMENTS)
def test_apply_p_right_trans_tri(placement):
    n = width(placement)
    a = Placed(placement, ROWS, n, 15)
    rng = np.random.default_rng(7)
    Q = np.array([rng.integers(i, n) if rng.random() < 0.7 else i for i in range(n)], dtype=np.int32)

    def replay():  # row r takes the swaps i > r in ascending order; written back under the column mask
        b = a.o.to_bits()
        for i in range(n):
            if Q[i] != i:
                rows = slice(0, min(ROWS, i))
                b[rows, [i, Q[i]]] = b[rows, [Q[i], i]]
        v, mask = a.o.valid_words(), np.uint64(a.o.high_bitmask)
        w = Mzd.from_bits(b).valid_words()
        v[:, :-1] = w[:, :-1]
        v[:, -1] = (v[:, -1] & ~mask) | (w[:, -1] & mask)

    check([(a, True)], lambda: m4ri_amd.mzd_apply_p_right_trans_tri(a.g, Q), replay)


@pytest.mark.parametrize("placement", PLACEMENTS)
def test_trtri_upper(oracle, placement):
    n = side(placement)
    a = Placed(placement, n, n, 16)
    check([(a, True)], lambda: m4ri_amd.mzd_trtri_upper(a.g), lambda: oracle.trtri_upper(a.o))


@pytest.mark.parametrize("pb", PLACEMENTS)
@pytest.mark.parametrize("pa", ["host", "pinned-ragged"])
def test_solve_left(oracle, pa, pb):
    """A (130 x 130, decomposed in place) and B (130 rows, as wide as its placement makes it) placed independently."""
    a, b = Placed(pa, 130, 130, 17), Placed(pb, 130, width(pb), 18)
    got, want = check([(a, True), (b, True)], lambda: m4ri_amd.mzd_solve_left(a.g, b.g, 0, True), lambda: oracle.solve_left(a.o, b.o, True))
    assert got == want


@pytest.mark.parametrize("pb", PLACEMENTS)
@pytest.mark.parametrize("pa", READ_PLACEMENTS)
def test_pluq_solve_left(oracle, pa, pb):
    D = Mzd.random(130, 130, 19)
    r, P, Q = oracle.ple(D, pluq=True)
    a, b = Placed(pa, 130, 130, 20, content=D), Placed(pb, 130, width(pb), 21)
    got, want = check([(a, False), (b, True)], lambda: m4ri_amd.mzd_pluq_solve_left(a.g, r, P, Q, b.g, 0, True),
                      lambda: oracle.pluq_solve_left(a.o, r, P, Q, b.o, True))
    assert got == want


@pytest.mark.parametrize("placement", PLACEMENTS)
def test_kernel_left_pluq(oracle, placement):
    a = Placed(placement, ROWS, width(placement), 22)
    Rg, (r, Ro) = check([(a, True)], lambda: m4ri_amd.mzd_kernel_left_pluq(a.g), lambda: oracle.kernel_left_pluq(a.o))
    assert (Ro is None) == (Rg is None)
    assert Ro is not None, "70 rows cannot have full column rank: a basis is expected"
    assert (Rg.nrows, Rg.ncols) == (Ro.nrows, Ro.ncols) == (a.g.ncols, a.g.ncols - r) and np.array_equal(Rg.valid_words(), Ro.valid_words())


@pytest.mark.parametrize("pb", PLACEMENTS)
@pytest.mark.parametrize("pa", READ_PLACEMENTS)
def test_inv_m4ri(oracle, pa, pb):
    """A ragged window of a pinned parent as A carries the parent's neighbouring columns in its last word on the device; the
    inverse must not see them (mzd_inv_m4ri inverts such an A from a masked copy: m4ri_amd_inv_dev wants a clean tail)."""
    n = side(pb)
    a, b = Placed(pa, n, n, 23), Placed(pb, n, n, 24)

    def expect():  # the oracle returns a fresh inverse: written into B's window under the column mask
        w = oracle.inv(a.o).masked()
        v, mask = b.o.valid_words(), np.uint64(b.o.high_bitmask)
        v[:, :-1] = w[:, :-1]
        v[:, -1] = (v[:, -1] & ~mask) | w[:, -1]

    got, _ = check([(a, False), (b, True)], lambda: m4ri_amd.mzd_inv_m4ri(a.g, b.g), expect)
    assert got is b.g


@pytest.mark.parametrize("pd", PLACEMENTS)
@pytest.mark.parametrize("pa", READ_PLACEMENTS)
def test_transpose(oracle, pa, pd):
    n = side(pd)
    a, d = Placed(pa, n, 130, 25), Placed(pd, 130, n, 26)
    got, _ = check([(a, False), (d, True)], lambda: m4ri_amd.mzd_transpose(a.g, d.g), lambda: oracle.transpose(a.o, d.o))
    assert got is d.g


@pytest.mark.parametrize("pb", PLACEMENTS)
@pytest.mark.parametrize("which", ["upper_left", "lower_right"])
def test_trsm(oracle, which, pb):
    """T a window of a pinned parent (ragged wherever B's placement leaves it 130 columns), B in every placement."""
    if which == "upper_left":
        t, b = Placed("pinned-ragged", 130, 130, 27), Placed(pb, 130, width(pb), 28)
        call, expect = (lambda: m4ri_amd.mzd_trsm_upper_left(t.g, b.g)), (lambda: oracle.trsm_upper_left(t.o, b.o))
    else:
        n = side(pb)
        t, b = Placed("pinned-ragged", n, n, 27), Placed(pb, ROWS, n, 28)
        call, expect = (lambda: m4ri_amd.lib().mzd_trsm_lower_right(t.g.ptr, b.g.ptr, 0)), (lambda: oracle.trsm_lower_right(t.o, b.o))
    check([(t, False), (b, True)], call, expect)


@pytest.mark.parametrize("placement", PLACEMENTS)
def test_addmul(oracle, placement):
    n = width(placement)
    c = Placed(placement, ROWS, n, 29)
    A, B = Mzd.random(ROWS, 100, 30), Mzd.random(100, n, 31)
    got, _ = check([(c, True)], lambda: m4ri_amd.mzd_addmul(c.g, A, B, 0), lambda: oracle.addmul(c.o, A, B, 0))
    assert got is c.g
