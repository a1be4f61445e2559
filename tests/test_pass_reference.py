"""The NumPy reference of the fused passes (tests/pass_reference.py) is proven on the CPU before it judges a kernel.

The bilinear identity: for every pass depth, down(A) and down(B) give the leaf operands, every leaf product comes from the CPU oracle, and
up(products) must equal the oracle's product of the whole matrices (acc: added onto a random C0, against the oracle's addmul).  Together
with the fixed, documented descendant order (pass_reference's docstring) this makes the reference independent of the kernels it is
compared with in tests/test_gpu_passes.py.  Shapes: the smallest that are still general -- crows in {1, 3}, words per leaf row of A and of
B in {1, 2}.  No GPU anywhere in this module.
"""
import numpy as np
import pytest

import pass_reference as ref
from m4ri_amd.mzd import Mzd

DEPTHS = [("winograd", L) for L in (1, 2, 3, 4)] + [("scheme", L) for L in (2, 3, 4)]
SHAPES = [(1, 1, 1), (3, 1, 2), (3, 2, 1), (1, 2, 2)]   # crows, cwa, cwb: both values of each, every pair of values of two of them


def _mzd_of(words: np.ndarray) -> Mzd:
    """A (rows, w) uint64 array as an Mzd with rowstride w (a copy)."""
    rows, w = words.shape
    return Mzd(rows, 64 * w, np.ascontiguousarray(words).reshape(-1).copy(), rowstride=w)


def _words_of(M: Mzd) -> np.ndarray:
    return M.rows()[:, :M.width].copy()


_leaf_cache = {}


def _case(oracle, kind, L, crows, cwa, cwb):
    key = (kind, L, crows, cwa, cwb)
    if key not in _leaf_cache:
        _leaf_cache.clear()   # one case at a time: the parametrisation runs acc 0 and 1 of a case back to back
        scheme = kind == "scheme"
        rng = np.random.default_rng(1000 * L + 100 * crows + 10 * cwa + cwb + (7 if scheme else 0))
        f = 1 << L
        A = rng.integers(0, 1 << 64, size=(f * crows, f * cwa), dtype=np.uint64)
        B = rng.integers(0, 1 << 64, size=(f * 64 * cwa, f * cwb), dtype=np.uint64)
        dA = ref.down(A[None], L, scheme, False)[0]
        dB = ref.down(B[None], L, scheme, True)[0]
        n = ref.leaves(L, scheme)
        assert dA.shape == (n, crows, cwa) and dB.shape == (n, 64 * cwa, cwb)
        prods = np.empty((n, crows, cwb), dtype=np.uint64)
        for d in range(n):
            prods[d] = _words_of(oracle.mul(None, _mzd_of(dA[d]), _mzd_of(dB[d]), 0))
        _leaf_cache[key] = (A, B, prods)
    return _leaf_cache[key]


@pytest.mark.parametrize("acc", [0, 1])
@pytest.mark.parametrize("crows,cwa,cwb", SHAPES)
@pytest.mark.parametrize("kind,L", DEPTHS)
def test_down_leaf_products_up_is_the_product(oracle, kind, L, crows, cwa, cwb, acc):
    A, B, prods = _case(oracle, kind, L, crows, cwa, cwb)
    scheme = kind == "scheme"
    got = ref.up(prods[None], L, scheme)[0]
    mA, mB = _mzd_of(A), _mzd_of(B)
    if acc:
        C0 = np.random.default_rng(5).integers(0, 1 << 64, size=got.shape, dtype=np.uint64)
        want = _words_of(oracle.addmul(_mzd_of(C0), mA, mB, 0))
        got = got ^ C0
    else:
        want = _words_of(oracle.mul(None, mA, mB, 0))
    bad = np.argwhere(got != want)
    assert bad.size == 0, f"{kind} levels {L}: up(down x down) differs from the oracle's product at (row, word) {bad[:4].tolist()}"


@pytest.mark.parametrize("kind,L", [d for d in DEPTHS if d not in (("winograd", 1), ("scheme", 2))])
def test_descendant_order_is_the_recursion(kind, L):
    """Levels 2 ... 4 are one level applied recursively, the top level's child most significant: descendant n_rest * j_top + d_rest of
    the parent is descendant d_rest of the (L - 1 or L - 2)-level pass of its top-level child j_top."""
    scheme = kind == "scheme"
    steps = ref.pass_steps(L, scheme)
    rng = np.random.default_rng(L)
    f = 1 << L
    for bside in (False, True):
        X = rng.integers(0, 1 << 64, size=(2, f * 2, f * 1), dtype=np.uint64)
        whole = ref.down(X, L, scheme, bside)
        top = ref.winograd_down1(X, bside) if steps[0] == "w" else ref.scheme_down1(X, bside)
        ktop = top.shape[1]
        rest_levels = L - (1 if steps[0] == "w" else 2)
        rest_scheme = scheme and "s" in steps[1:]
        rest = ref.down(top.reshape((-1,) + top.shape[-2:]), rest_levels, rest_scheme, bside)
        nrest = rest.shape[1]
        assert whole.shape[1] == ktop * nrest == ref.leaves(L, scheme)
        assert np.array_equal(whole.reshape(2, ktop, nrest, 2, 1), rest.reshape(2, ktop, nrest, 2, 1))


@pytest.mark.parametrize("rot", [0, 1])
@pytest.mark.parametrize("m,w,m_pad", [(1, 1, 4), (7, 3, 8), (64, 1, 64), (288, 2, 288), (330, 1, 332)])
def test_unpacking_the_packed_a_gives_the_descendants_back(rot, m, w, m_pad):
    rng = np.random.default_rng(m + w)
    D = rng.integers(0, 1 << 64, size=(3, m, w), dtype=np.uint64)
    P = ref.pack_a4(D, rot, m_pad)
    assert P.shape == (3, 2 * w, m_pad) and P.dtype == np.uint32
    assert not P[:, :, m:].any(), "rows m .. m_pad - 1 of the packed form are zero"
    assert np.array_equal(ref.unpack_a4(P, rot, m), D)
    # the layout itself, entry by entry on a few: dword q of row r, byte i of the stored dword = byte (i + (r >> 6)) & 3 of the plain one
    for (n, r, q) in [(0, 0, 0), (1, m - 1, 2 * w - 1), (2, m // 2, w)]:
        plain = int(D[n, r, q // 2] >> np.uint64(32 * (q & 1))) & 0xFFFFFFFF
        s = ((r >> 6) & 3) if rot else 0
        want = sum(((plain >> (8 * ((i + s) & 3))) & 0xFF) << (8 * i) for i in range(4))
        assert int(P[n, q, r]) == want, (n, r, q)
    if rot and m > 64:
        assert not np.array_equal(P, ref.pack_a4(D, 0, m_pad)), "rows 64 and above are rotated"


def test_operand_views_and_frames():
    rng = np.random.default_rng(3)
    op = ref.make_operand(rng, nparents=3, rows=4, words=2, off=1, stride_pad=1, gap=5, guard=7)
    assert (op.off, op.stride, op.bs) == (8, 3, 17)
    v = op.view()
    assert v.shape == (3, 4, 2) and v[2, 3, 1] == op.buf[8 + 2 * 17 + 3 * 3 + 1]
    m = op.written_mask()
    assert m.sum() == 3 * 4 * 2 and not m[:8].any() and not m[-7:].any() and not m[8 + 2] and m[8 + 17]
    z = ref.make_operand(rng, 1, 4, 2, zero_bs=True)
    assert z.bs == 0 and z.view().shape == (1, 4, 2)
