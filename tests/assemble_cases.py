"""What tests/test_assemble_batch_plan.py and tests/test_gpu_assemble_batch.py share: the expected results of the calls of
assemble_batch.hip in NumPy on unpacked bits (block copy, the triangle rules, sequential transpositions on rows and columns), a
batch of members inside a buffer of random words seen as bits, and the shape lists.  No GPU here (the upload is the only torch call)."""
import numpy as np


def words(n):
    return (n + 63) // 64


# ---- the expected results, on rows x cols arrays of 0 / 1 -----------------------------------------------------------------------

def copy_block(D, d_row, d_col, A, a_row, a_col, rows, cols):
    """D with its block at (d_row, d_col) replaced by A's block at (a_row, a_col); a new array."""
    out = D.copy()
    out[d_row:d_row + rows, d_col:d_col + cols] = A[a_row:a_row + rows, a_col:a_col + cols]
    return out


def triangle(A, upper, diag, rank=None):
    """m4ri_amd_extract_tri_batch_dev's rules: the k x ncols upper or nrows x k lower triangle of A, k = min(nrows, ncols); the
    diagonal 0 / 1 / A's for diag 0 / 1 / 2; rank (clamped to 0 .. k) zeroes the upper form's rows from it on, diagonal included,
    and keeps the lower form's columns from it on free of A: the diagonal rule's bit and zeros."""
    nrows, ncols = A.shape
    k = min(nrows, ncols)
    r = k if rank is None else min(max(int(rank), 0), k)
    i, j = np.arange(nrows)[:, None], np.arange(ncols)[None, :]
    d = {0: np.zeros_like(A), 1: np.ones_like(A), 2: A}[diag]
    if upper:
        out = np.where(j > i, A, 0) + np.where(j == i, d, 0)
        out = np.where(i < r, out, 0)
        return out[:k].astype(np.uint8)
    out = np.where((i > j) & (j < r), A, 0) + np.where(i == j, d, 0)
    return out[:, :k].astype(np.uint8)


def gather_index(P, n, length, ascending):
    """The transpositions (i, P[i]), i < min(length, n), replayed in order on the identity: position x ends up holding what stood at
    src[x].  None if an entry lies outside 0 .. n-1."""
    L = min(length, n)
    P = np.asarray(P[:L], dtype=np.int64)
    if ((P < 0) | (P >= n)).any():
        return None
    src = np.arange(n)
    for i in (range(L) if ascending else range(L - 1, -1, -1)):
        j = P[i]
        src[i], src[j] = src[j], src[i]
    return src


def apply_p(A, P, length, right, trans):
    """mzd_apply_p_left (rows, ascending) / _left_trans (descending) / _right (columns, descending) / _right_trans (ascending) as the
    sequence of swaps it is; None (the member stays untouched) for an entry out of range."""
    n = A.shape[1] if right else A.shape[0]
    src = gather_index(P, n, length, ascending=bool(trans) if right else not trans)
    if src is None:
        return None
    return A[:, src] if right else A[src, :]


def with_rank(nrows, ncols, r, seed):
    """A random nrows x ncols member of rank exactly r whose pivots are not where they end up: [I; X] * [I | Y] under random row and
    column orders."""
    rng = np.random.default_rng(seed)
    X = np.vstack([np.eye(r, dtype=np.int64), rng.integers(0, 2, size=(nrows - r, r))])
    Y = np.hstack([np.eye(r, dtype=np.int64), rng.integers(0, 2, size=(r, ncols - r))])
    A = (X @ Y) & 1
    return A[rng.permutation(nrows)][:, rng.permutation(ncols)].astype(np.uint8)


def matmul(A, B):
    return ((A.astype(np.int64) @ B.astype(np.int64)) & 1).astype(np.uint8)


# ---- a batch inside random words ------------------------------------------------------------------------------------------------

def to_bits(w):
    return np.unpackbits(w.view(np.uint8), bitorder="little")


def to_words(bits):
    return np.packbits(bits, bitorder="little").view(np.uint64)


class Batch:
    """`batch` members of `rows` rows, `stride` words apart, `bs` words from member to member (shared: one member, bs = 0), the first
    at word `base` of a buffer of random words -- valid bits, tail bits, padding words, gaps and guards all random.  self.bits is the
    buffer bit by bit; member(bits, b) is a writable rows x 64 * stride view of member b in such an array, on which an expected image
    is made with the functions above."""

    def __init__(self, rows, ncols, batch, seed, pad=1, gap=3, base=5, shared=False):
        self.rows, self.ncols, self.batch, self.base = rows, ncols, batch, base
        self.stride = words(ncols) + pad
        self.bs = 0 if shared else rows * self.stride + gap
        n = 1 if shared else batch
        total = base + max(n - 1, 0) * self.bs + rows * self.stride + 7
        self.h = np.random.default_rng(seed).integers(0, 1 << 64, size=total, dtype=np.uint64)
        self.bits = to_bits(self.h)
        self.t = None

    def member(self, bits, b):
        start = 64 * (self.base + b * self.bs)
        assert start + 64 * self.rows * self.stride <= bits.size
        return np.lib.stride_tricks.as_strided(bits[start:], shape=(self.rows, 64 * self.stride), strides=(64 * self.stride, 1), writeable=True)

    def valid(self, b, bits=None):
        """A copy of member b's rows x ncols valid bits."""
        return self.member(self.bits if bits is None else bits, b)[:, :self.ncols].copy()

    def set_valid(self, b, M):
        """Before the upload: member b's valid bits <- M."""
        assert self.t is None
        self.member(self.bits, b)[:, :self.ncols] = M
        self.h = to_words(self.bits)

    def upload(self):
        import torch
        self.t = torch.from_numpy(self.h.view(np.int64).copy()).cuda()
        return self

    @property
    def ptr(self):
        return self.t.data_ptr() + 8 * self.base

    def download(self):
        return self.t.cpu().numpy().view(np.uint64)

    def check(self, exp_bits, what=""):
        """The whole buffer word for word against the expected image (bits)."""
        got, exp = self.download(), to_words(exp_bits)
        bad = np.flatnonzero(got != exp)
        assert bad.size == 0, f"{what}: {bad.size} words differ from the expected image, the first at word {bad[0]} " \
                              f"(base {self.base}, stride {self.stride}, bs {self.bs}): got {int(got[bad[0]]):#x}, expected {int(exp[bad[0]]):#x}"

    def check_unchanged(self, what=""):
        assert np.array_equal(self.download(), self.h), f"{what}: a read-only operand or its surroundings changed"


# ---- the shapes -----------------------------------------------------------------------------------------------------------------

COPY_COL_OFFSETS = (0, 1, 63, 64, 65)
COPY_COLS = (1, 63, 64, 65, 127, 128, 129)
COPY_ROWS = (1, 64, 65)
COPY_ROW_OFFSETS = (0, 3)
TRI_SHAPES = ((1, 1), (63, 63), (64, 64), (65, 65), (64, 130), (130, 64), (200, 100))
PERM_SHAPES = TRI_SHAPES + ((300, 300),)
CHAIN_SHAPES = ((64, 64), (65, 130), (200, 100))


def tri_ranks(k):
    """The rank array of the triangle tests: 0, 1, 64, k and one value above k (clamped)."""
    return np.array([0, 1, 64, k, k + 3], dtype=np.int32)


def perm_lengths(n):
    return sorted({0, 1, max(n - 1, 0), n, n + 5})


def perm_members(n, seed):
    """(name, P) of the members of one permutation call, each P with n + 5 entries: the identity, a full reversal, entries of any
    order (P[i] < i among them), LAPACK-style entries P[i] >= i, one member with an entry equal to n and one with a negative entry
    (both at index 0, so that every length >= 1 sees them)."""
    rng = np.random.default_rng(seed)
    i = np.arange(n + 5)
    anyp = rng.integers(0, n, size=n + 5)
    lap = np.minimum(i + rng.integers(0, n, size=n + 5), n - 1)
    lap[:n] = np.maximum(lap[:n], i[:n])
    toobig, neg = anyp.copy(), lap.copy()
    toobig[0], neg[0] = n, -1
    rev = np.clip(n - 1 - i, 0, n - 1)
    ident = np.minimum(i, n - 1)
    return [("identity", ident), ("reversal", rev), ("any", anyp), ("lapack", lap), ("too big", toobig), ("negative", neg)]
