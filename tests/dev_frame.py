"""The frame of tests/test_gpu_dev_api.py: an r x c operand placed inside a larger, pattern-filled buffer -- guard rows before and
after it, pattern-filled padding words between its width and its stride, its first word at a chosen word offset -- so that a
device function can be held to what include/m4ri_amd.h says about the memory AROUND its operand.  Pure numpy (the upload is
the only torch call), and the plain reference of the wide column gather, pinned on the CPU by tests/test_dev_frame_cpu.py."""
import numpy as np

from m4ri_amd.mzd import Mzd, splitmix_words

LAYOUTS = ("even", "odd", "wide")
GUARD = 2  # pattern-filled rows before and after the operand
_ONES = np.uint64(0xFFFFFFFFFFFFFFFF)


def geometry(width, layout):
    """(stride, base) in words: the distance between rows and the index of the operand's first word in the flat buffer.
    even: the host shim's layout, stride = width rounded up to even, the base 16-byte aligned;
    odd:  stride odd and > width, the base at an odd word (8- but not 16-byte aligned; every other row is 16-byte aligned);
    wide: stride = width + 3, the base at an even word."""
    if layout == "even":
        stride = width + (width & 1)
        base = GUARD * stride
    elif layout == "odd":
        stride = width + 1 + (width & 1)
        base = GUARD * stride + 1
    elif layout == "wide":
        stride = width + 3
        base = GUARD * stride
        base += base & 1
    else:
        raise ValueError(layout)
    return stride, base


class Frame:
    """The valid bits of M inside a pattern-filled buffer.  dirty_tail: the bits of the last word beyond M's columns keep the
    pattern (for functions that promise to ignore them); otherwise they are zero (for functions that require that)."""

    def __init__(self, M: Mzd, layout: str, seed: int, dirty_tail: bool = False):
        self.nrows, self.ncols, self.width = M.nrows, M.ncols, M.width
        self.mask = np.uint64(M.high_bitmask)
        self.stride, self.base = geometry(self.width, layout)
        total = self.base + (self.nrows + GUARD) * self.stride
        self.before = splitmix_words(seed, 0, total)
        v = self.view(self.before)
        w = M.masked()
        if dirty_tail:
            w[:, -1] |= v[:, -1] & ~self.mask
        v[:, :] = w
        inside = np.zeros(total, dtype=bool)
        self.view(inside)[:, :] = True
        self.outside = ~inside
        self.t = None

    def view(self, flat):
        """The operand's nrows x width words inside a flat buffer of this frame's geometry."""
        return np.lib.stride_tricks.as_strided(flat[self.base:], shape=(self.nrows, self.width),
                                               strides=(flat.itemsize * self.stride, flat.itemsize), writeable=True)

    def upload(self):
        import torch
        self.t = torch.from_numpy(self.before.view(np.int64).copy()).cuda()
        assert self.t.data_ptr() % 16 == 0
        return self

    @property
    def ptr(self):
        return self.t.data_ptr() + 8 * self.base

    def download(self):
        return self.t.cpu().numpy().view(np.uint64)

    def check(self, want, tail: str, what: str = ""):
        """After the call: every word outside the operand's rows and words [0, width) unchanged; the valid bits those of
        `want` (an Mzd, or None: unchanged); the tail bits "zero" or "kept" (as on entry)."""
        after = self.download()
        changed = np.flatnonzero(after[self.outside] != self.before[self.outside])
        assert changed.size == 0, f"{what}: {changed.size} words outside the operand changed, the first at flat index " \
                                  f"{np.flatnonzero(self.outside)[changed[0]]} (base {self.base}, stride {self.stride}, width {self.width})"
        got, was = self.view(after).copy(), self.view(self.before)
        exp = was.copy() if want is None else want.masked()
        exp[:, -1] &= self.mask
        g = got.copy()
        g[:, -1] &= self.mask
        bad = np.argwhere(g != exp)
        assert bad.size == 0, f"{what}: {len(bad)} words of the result differ, the first at (row, word) {tuple(bad[0])}"
        t_got = got[:, -1] & ~self.mask
        t_exp = (was[:, -1] & ~self.mask) if tail == "kept" else np.zeros(self.nrows, dtype=np.uint64)
        assert np.array_equal(t_got, t_exp), f"{what}: the bits beyond column {self.ncols} are not {tail}"

    def check_unchanged(self, what: str = ""):
        assert np.array_equal(self.download(), self.before), f"{what}: a read-only operand or its surroundings changed"


def ones(r, c):
    M = Mzd(r, c)
    M.valid_words()[:, :] = _ONES
    M.valid_words()[:, -1] &= np.uint64(M.high_bitmask)
    return M


def one_bit(r, c, i, j):
    M = Mzd(r, c)
    M.valid_words()[i, j // 64] = np.uint64(1) << np.uint64(j % 64)
    return M


def identity_like(r, c):
    """One bit per row: (i, i mod c)."""
    M = Mzd(r, c)
    i = np.arange(r)
    j = i % c
    M.valid_words()[i, j // 64] = np.uint64(1) << (j % 64).astype(np.uint64)
    return M


def unit_diag(T):
    i = np.arange(min(T.nrows, T.ncols))
    T.valid_words()[i, i // 64] |= np.uint64(1) << (i % 64).astype(np.uint64)
    return T


def apply_p_right_bits(bits, P, trans):
    """mzd_apply_p_right (trans false: A * P, the transpositions (i, P[i]) with i descending) / mzd_apply_p_right_trans (A * P^T,
    i ascending) on an unpacked rows x ncols bit array: the swaps are replayed on the array `src` (src[c] = the column that
    stands at position c), then every row is gathered through it."""
    ncols = bits.shape[1]
    P = np.asarray(P[:ncols], dtype=np.int64)
    src = np.arange(ncols)
    moved = np.flatnonzero(P != np.arange(len(P)))
    for i in (moved if trans else moved[::-1]):
        j = P[i]
        src[i], src[j] = src[j], src[i]
    return bits[:, src]


def pack_bits(bits):
    return Mzd.from_bits(np.ascontiguousarray(bits, dtype=np.uint8))


def trsm_right_by_transposition(oracle, T, B, upper):
    """The oracle's solution of X T = B (T unit upper / lower triangular) from its left-hand solve of T^T X^T = B^T: the
    transpose of an upper triangle is a lower one, and the solution is unique."""
    Tt, Bt = oracle.transpose(T), oracle.transpose(B)
    (oracle.trsm_lower_left if upper else oracle.trsm_upper_left)(Tt, Bt)
    return oracle.transpose(Bt)
