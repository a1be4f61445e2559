"""The arena of tests/test_gpu_far_operands.py: ONE device allocation in which the operands of a device entry point are placed
so far apart -- two rows of one operand, or two members of one batch, 2 GiB to 16 GiB from each other -- that an offset computed
in 32 bits somewhere between the public call and a load or store no longer reaches the word it means.  The arithmetic is pure
Python / NumPy (tests/test_far_arena_cpu.py checks it for every declared case without a GPU); the torch part only fills, uploads,
reads back and compares.

The arena is a single torch.empty(N, int64) filled in place with a position-dependent pattern, word i = i * PATTERN_MUL mod 2^64
(an odd constant: the map is a bijection, and two words 2^32 bytes or 2^31 words apart never hold the same value).  No second
buffer of that size exists at any time; filling and checking work on the device in chunks of at most 1 GiB.

No faults by construction.  Word 0 of every operand lies BASE = 2^31 + 2^20 words (16 GiB and a bit) into the arena, plus an offset
inside the first pitch.  A case makes ONE axis far, its row stride or its batch stride, never both, so an address has one large
term and one truncation to suffer.  True offsets run from 0 to a little over 2^31 words above the operand's first word.  What a
32-bit defect turns such an offset x (in words, 8 x in bytes) into:
  * the byte offset as uint32: (8 x mod 2^32) / 8, in [0, 2^29) words = [0, 4 GiB) above the operand's first word;
  * the byte offset as int32: in [-2^28, 2^28) words = [-2 GiB, 2 GiB);
  * the word offset as int32: in [-2^31, 2^31) words = [-16 GiB, 16 GiB);
  * row * stride (or b * batch stride) alone wrapped to 32 bits before the rest is added: the same interval, shifted by less than
    one member.
All of that is arena: 16 GiB of pattern lie below BASE, the operands and more than 16 GiB above it.  So a 32-bit defect reads
pattern words (a wrong result) or overwrites them (the pattern check finds the word); it does not leave the allocation.
test_far_arena_cpu.py proves the four images per case, for every row of every operand.  Word indices held in a uint32 wrap at
32 GiB; showing those would take an arena of 70 GiB and is out of scope."""
from dataclasses import dataclass

import numpy as np

# ---- geometry (all in 64-bit words) ---------------------------------------------------------------------------------------------
# launch_leaf (engine.hip) cuts a product so that the l rows of one B chunk stay below LEAF_LIMIT bytes, and a chunk has at least 64
# rows: a B side is legal up to a stride of LEAF_LIMIT / (64 * 8) = 8 386 560 words.
LEAF_LIMIT = (1 << 32) - (1 << 20)
B_STRIDE_MAX = LEAF_LIMIT // (64 * 8)
# Far row strides, one odd (every other row 8- but not 16-byte aligned) and one even (the 16-byte paths), both below B_STRIDE_MAX so
# that products on such operands are chunked, not refused.  With them a row offset crosses 2^31 bytes at row 34 (34 * 8 000 001 * 8
# >= 2^31), 2^32 bytes at row 68 and 2^31 words at row 269 (269 * 8 000 001 = 2 152 000 269 >= 2 147 483 648).
S_ODD, S_EVEN = 8_000_001, 8_000_002
FAR_ROWS_MIN, FAR_ROWS_MAX = 270, 300   # an operand that goes far by its rows has this many, unless its case says why not
# Operands of at most 256 rows that are no engine operands (the tables of m4ri_amd_process_rows_dev / m4ri_amd_make_table_dev):
# 255 * 9 000 001 = 2 295 000 255 >= 2^31 words.
S_TABLE = 9_000_001
S_TABLE_EVEN = S_TABLE + 1              # tables with an even stride: what the 16-byte update kernels of process_rows require
# The first stride of a B side that is refused: 64 rows of (1 << 23) + 1 words are 2^32 + 512 bytes.
S_REFUSED = (1 << 23) + 1
# Far batch strides with batch = 4: 3 * 715 827 885 = 2 147 483 655 >= 2^31 words; members at 0, 5.3, 10.7 and 16.0+ GiB.
BATCH = 4
BS_ODD = 715_827_885
BS_EVEN = BS_ODD + 1
# Word 0 of every operand is at least this far into the arena: what int32 word offsets can reach below an operand, and 2^20 more.
BASE = (1 << 31) + (1 << 20)
TAIL_ROOM = 1 << 20                     # the arena ends this many words after the highest word any declared case uses
CHUNK = 1 << 27                         # fill and check 1 GiB at a time
PATTERN_MUL = 0x9E3779B97F4A7C15        # odd
_MUL_I64 = PATTERN_MUL - (1 << 64)      # the same constant as torch's int64 sees it
_MUL_U64 = np.uint64(PATTERN_MUL)

assert S_EVEN < B_STRIDE_MAX < S_REFUSED and 64 * S_REFUSED * 8 >= LEAF_LIMIT
assert 33 * S_ODD * 8 < 1 << 31 <= 34 * S_ODD * 8 and 67 * S_ODD * 8 < 1 << 32 <= 68 * S_ODD * 8 and 268 * S_ODD < 1 << 31 <= 269 * S_ODD
assert 255 * S_TABLE >= 1 << 31 and (BATCH - 1) * BS_ODD >= 1 << 31

THRESHOLDS = (("int32-bytes", (1 << 31) // 8), ("uint32-bytes", (1 << 32) // 8), ("int32-words", 1 << 31))   # name, first word offset beyond


@dataclass(frozen=True)
class Win:
    """Where one operand of a call lies: `batch` members of rows x width words, member b's row r at off + b * bs + r * stride words
    above BASE.  bs == 0 with batch == 1 is a single (or shared) operand."""
    off: int
    rows: int
    width: int
    stride: int
    batch: int = 1
    bs: int = 0

    def starts(self):
        """The word offset above BASE of every row of every member, as int64 (batch, rows)."""
        return self.off + np.arange(self.batch, dtype=np.int64)[:, None] * self.bs + np.arange(self.rows, dtype=np.int64)[None, :] * self.stride

    def last_word(self):
        """The highest word offset above `off` that belongs to the operand."""
        return (self.batch - 1) * self.bs + (self.rows - 1) * self.stride + self.width - 1

    def crossed(self):
        return tuple(name for name, first in THRESHOLDS if self.last_word() >= first)


def disjoint(wins):
    """No word belongs to two rows of these windows (rows of one window included)."""
    s = np.concatenate([w.starts().ravel() for w in wins])
    e = np.concatenate([w.starts().ravel() + w.width for w in wins])
    o = np.argsort(s, kind="stable")
    return bool(np.all(e[o][:-1] <= s[o][1:]))


def _wrap(x, bits, signed):
    x = np.asarray(x, dtype=np.int64) & ((1 << bits) - 1)
    return np.where(x >= 1 << (bits - 1), x - (1 << bits), x) if signed else x


def truncation_images(w: Win):
    """For the first and the last word of every row of the operand: the arena index (BASE included) a kernel reaches when it
    truncates the true offset from the operand's first word in one of the four ways of the module's docstring.  The images of the
    words in between lie between those of the row's ends, except where a row straddles a wrap; then they are at the interval's
    ends, which the bounds below cover: returns {name: (lowest, highest)} with the closed-form interval ends folded in."""
    first = w.starts() - w.off                      # true word offsets from the operand's pointer
    by_batch = w.bs * (w.batch - 1) > w.stride * (w.rows - 1)   # the far axis: the one that reaches further
    far = (np.arange(w.batch, dtype=np.int64)[:, None] * w.bs) if by_batch else (np.arange(w.rows, dtype=np.int64)[None, :] * w.stride)
    near = first - far                              # the other axis: added after the wrap
    out = {}
    p = BASE + w.off
    for name, bits, signed, unit in (("uint32-bytes", 32, False, 8), ("int32-bytes", 32, True, 8), ("int32-words", 32, True, 1)):
        ends = np.stack([_wrap(first * unit, bits, signed), _wrap((first + w.width - 1) * unit, bits, signed)]) // unit
        lo, hi = int(ends.min()), int(ends.max())
        straddles = np.any(_wrap(first * unit, bits, signed) > _wrap((first + w.width - 1) * unit, bits, signed))
        if straddles:                               # a row crosses the wrap: its words reach both ends of the interval
            lo = -(1 << (bits - 1)) // unit if signed else 0
            hi = ((1 << (bits - 1)) - 1) // unit if signed else ((1 << bits) - 1) // unit
        out[name] = (p + lo, p + hi)
    prod = np.stack([_wrap(far, 32, True), _wrap(far, 32, False)])          # the product alone, wrapped either way
    out["product-32"] = (p + int((prod + near).min()), p + int((prod + near).max()) + w.width - 1)
    return out


def arena_words(wins):
    """The arena for these windows: it ends TAIL_ROOM words after the highest word any of them uses."""
    return BASE + max(w.off + w.last_word() for w in wins) + 1 + TAIL_ROOM


def pattern_np(idx):
    """The pattern at flat arena indices `idx` (any integer array), as uint64."""
    with np.errstate(over="ignore"):
        return np.asarray(idx).astype(np.uint64) * _MUL_U64


# ---- the torch part ---------------------------------------------------------------------------------------------------------------

class Placed:
    """One operand in the arena.  `before`: its (batch, rows, width) words as they were uploaded."""

    def __init__(self, arena, win, before, mask, ncols):
        self.arena, self.win, self.before, self.mask, self.ncols = arena, win, before, np.uint64(mask), ncols

    @property
    def ptr(self):
        return self.arena.t.data_ptr() + 8 * (BASE + self.win.off)

    def fetch(self):
        return self.arena.view(self.win).cpu().numpy().view(np.uint64)

    def check_unchanged(self, what=""):
        assert np.array_equal(self.fetch(), self.before), f"{what}: a read-only operand changed"

    def check(self, want, tail, what=""):
        """The valid bits those of `want` (an Mzd, a list of one Mzd per member, or None: unchanged); the bits of the last word
        beyond the last column "zero" or "kept" (as on entry)."""
        got = self.fetch()
        if want is None:
            exp = self.before.copy()
        else:
            exp = np.stack([m.masked() for m in (want if isinstance(want, (list, tuple)) else [want])])
        assert exp.shape == got.shape, (what, exp.shape, got.shape)
        exp[:, :, -1] &= self.mask
        g = got.copy()
        g[:, :, -1] &= self.mask
        bad = np.argwhere(g != exp)
        assert bad.size == 0, f"{what}: {len(bad)} words of the result differ, the first at (member, row, word) {tuple(bad[0])}"
        t_exp = (self.before[:, :, -1] & ~self.mask) if tail == "kept" else np.zeros_like(got[:, :, -1])
        assert np.array_equal(got[:, :, -1] & ~self.mask, t_exp), f"{what}: the bits beyond column {self.ncols} are not {tail}"


class Arena:
    def __init__(self, nwords):
        import torch
        self.torch, self.n = torch, int(nwords)
        self.t = torch.empty(self.n, dtype=torch.int64, device="cuda")
        assert self.t.data_ptr() % 16 == 0
        self.placed = []
        self.fill()

    def fill(self):
        torch = self.torch
        for lo in range(0, self.n, CHUNK):
            hi = min(self.n, lo + CHUNK)
            torch.arange(lo, hi, dtype=torch.int64, device="cuda", out=self.t[lo:hi])
            self.t[lo:hi].mul_(_MUL_I64)
        self.placed = []

    def view(self, win: Win):
        return self.torch.as_strided(self.t, (win.batch, win.rows, win.width), (win.bs, win.stride, 1), BASE + win.off)

    def ptr(self, win: Win):
        """The device address of a window that is not placed (it keeps the pattern: the output of a call that must be refused)."""
        return self.t.data_ptr() + 8 * (BASE + win.off)

    def place(self, win: Win, mats, dirty_tail=False):
        """Upload an Mzd (or one per member) into the window.  dirty_tail: the bits beyond the last column keep the pattern."""
        mats = list(mats) if isinstance(mats, (list, tuple)) else [mats]
        assert len(mats) == win.batch and all((m.nrows, m.width) == (win.rows, win.width) for m in mats), (win, mats)
        words = np.stack([m.masked() for m in mats])
        mask = np.uint64(mats[0].high_bitmask)
        if dirty_tail:
            words[:, :, -1] |= pattern_np(BASE + win.starts() + win.width - 1) & ~mask
        assert BASE + win.off + win.last_word() < self.n
        self.view(win).copy_(self.torch.from_numpy(words.view(np.int64)))
        p = Placed(self, win, words, mask, mats[0].ncols)
        self.placed.append(p)
        return p

    def restore(self):
        """The pattern back over every placed window."""
        torch = self.torch
        for p in self.placed:
            w = p.win
            idx = (BASE + w.off + torch.arange(w.batch, device="cuda")[:, None, None] * w.bs + torch.arange(w.rows, device="cuda")[None, :, None] * w.stride
                   + torch.arange(w.width, device="cuda")[None, None, :])
            self.view(w).copy_(idx * _MUL_I64)
        self.placed = []

    def assert_pattern(self, what=""):
        """The whole arena against the regenerated pattern, on the device, a chunk at a time."""
        torch = self.torch
        flags = []
        for lo in range(0, self.n, CHUNK):
            hi = min(self.n, lo + CHUNK)
            flags.append((self.t[lo:hi] != torch.arange(lo, hi, dtype=torch.int64, device="cuda") * _MUL_I64).any())
        bad = torch.stack(flags).cpu().numpy()
        if not bad.any():
            return
        lo = int(np.flatnonzero(bad)[0]) * CHUNK
        hi = min(self.n, lo + CHUNK)
        ne = self.t[lo:hi] != torch.arange(lo, hi, dtype=torch.int64, device="cuda") * _MUL_I64
        first, count = lo + int(ne.nonzero()[0, 0]), int(ne.sum())
        dw = first - BASE
        raise AssertionError(
            f"{what}: a word outside every operand changed: first at flat index {first} ({count} in its 1 GiB chunk, {int(bad.sum())} chunks "
            f"hit); {dw} words = {8 * dw} bytes from BASE; modulo 2^32: {dw % (1 << 32)} words, {(8 * dw) % (1 << 32)} bytes "
            f"(row of a far operand: {dw // S_ODD} at S_ODD, member: {dw // BS_ODD} at BS_ODD)")
