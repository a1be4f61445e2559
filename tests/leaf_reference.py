"""A plain NumPy statement of what the M4RM leaves compute (host only; the second opinion of tests/test_gpu_leaves.py, proven on the CPU by
tests/test_leaf_reference.py).

The product is stated on WHOLE WORDS, because that is what the leaves write ("callers mask excess columns", m4rm_small.hip): A is
m x l bits -- the bits of its last word from column l on do not belong to it, whatever they hold -- and B is l rows of wn whole words,
the excess bits of its last word included; C = A B is m rows of wn whole words.  The method is the definition: bits unpacked, a matrix
product in float32 (exact: every sum is an integer below 2^24), reduced mod 2.

The geometry is written from the documented contracts, not from the kernels' index arithmetic:

  * tiles (gf2_common.h, LeafArgs): a product's C is cut into tiles of `rows` x `tw` words -- 32 rg x 32 for generation 1, 4096 x 8 for
    generation 4, 256 x 8 for generation 5; the linear tile order of a batch is tile_m fastest, then tile_n, then the batch member;
  * inner splits: a launch asked for `ks` splits cuts the inner dimension into units of 16 bits (generation 1), 32 bits (generation 4:
    one dword of the packed A) or 64 bits (generation 5: one word of A); a split takes ceil(units / ks) of them, and in generations 1
    and 4 an EVEN number, at least two ("a split always starts on a 32-bit A chunk" / "starts in table buffer 0"); the number of splits
    that are not empty is what the launch really uses (gf2_m4rm8q_effective_ksplit);
  * slabs (leaf mode 2): split k of the launch's tile number j (counted from tile_base) stores its whole tile, dense, 4096 rows of 8
    words, as slab j * splits + k.  Only the tile's rows below m and words below wn mean anything.
  * the packed A of generation 4: pass_reference.pack_a4.
"""
from __future__ import annotations

import numpy as np

from pass_reference import pack_a4  # noqa: F401  (re-exported: the packed A the generation-4 rows are fed)

# generation -> (tile rows, tile words, inner bits per unit of a split, units per split must be even)
G4_ROWS, G4_TW, G5_ROWS, G5_TW, G1_TW = 4096, 8, 256, 8, 32
SLAB_WORDS = G4_ROWS * G4_TW


def tile_shape(gen: int, rg: int = 32):
    return {1: (32 * rg, G1_TW), 4: (G4_ROWS, G4_TW), 5: (G5_ROWS, G5_TW)}[gen]


def words_of(ncols: int) -> int:
    return (ncols + 63) // 64


# ---- bits and the product ----------------------------------------------------------------------------------------------------------------
def bits_of(W: np.ndarray) -> np.ndarray:
    """(rows, w) uint64 -> (rows, 64 w) uint8, column c = bit c % 64 of word c // 64 (LSB = lowest column, gf2_common.h)."""
    W = np.ascontiguousarray(W, dtype="<u8")
    return np.unpackbits(W.view(np.uint8).reshape(W.shape[0], -1), axis=1, bitorder="little")


def words_of_bits(bits: np.ndarray) -> np.ndarray:
    """(rows, 64 w) 0/1 -> (rows, w) uint64."""
    rows = bits.shape[0]
    return np.packbits(bits.astype(np.uint8), axis=1, bitorder="little").view("<u8").reshape(rows, -1).astype(np.uint64)


def partial_product(A: np.ndarray, B: np.ndarray, l: int, k0: int = 0, k1: int | None = None) -> np.ndarray:
    """The part of A B that the inner bits [k0, k1) of [0, l) contribute: A (m, >= words_of(l)) words, B (>= l, wn) words -> (m, wn) words.
    Whole words of B; the bits of A from column l on are not looked at."""
    k1 = l if k1 is None else min(k1, l)
    k0 = min(k0, k1)
    m, wn = A.shape[0], B.shape[1]
    if k1 <= k0 or m == 0 or wn == 0:
        return np.zeros((m, wn), dtype=np.uint64)
    assert k1 - k0 < (1 << 24)
    a = bits_of(A[:, k0 // 64:words_of(k1)])[:, k0 % 64:k0 % 64 + (k1 - k0)].astype(np.float32)
    b = bits_of(B[k0:k1]).astype(np.float32)
    c = a @ b
    return words_of_bits(np.bitwise_and(c.astype(np.int64), 1))


def product(A: np.ndarray, B: np.ndarray, l: int) -> np.ndarray:
    return partial_product(A, B, l, 0, l)


# ---- inner splits ----------------------------------------------------------------------------------------------------------------------------
def split_bounds(gen: int, l: int, ks: int):
    """The inner bit ranges [k0, k1) of the splits a launch of generation `gen` asked for `ks` really makes (see the module docstring); their
    number is the effective split count.  l = 0: one empty split."""
    unit, even = {1: (16, True), 4: (32, True), 5: (64, False)}[gen]
    units = 2 * words_of(l) if gen == 4 else (l + unit - 1) // unit      # generation 4 works on whole words of A: two dwords each
    ks = max(ks, 1)
    per = -(-units // ks)
    if even:
        per = max(per + (per & 1), 2)
    per = max(per, 1)
    out = [(u * unit, min((u + per) * unit, l)) for u in range(0, units, per)]
    return out or [(0, 0)]


def partials(A: np.ndarray, B: np.ndarray, l: int, bounds) -> list:
    return [partial_product(A, B, l, k0, k1) for (k0, k1) in bounds]


# ---- tiles -----------------------------------------------------------------------------------------------------------------------------------
def tile_grid(m: int, wn: int, rows: int, tw: int):
    return -(-m // rows), -(-wn // tw)


def tile_of(t: int, tiles_m: int, tiles_n: int):
    """Linear tile number -> (batch member, tile_n, tile_m): tile_m fastest, then tile_n, then the member."""
    return t // (tiles_m * tiles_n), (t // tiles_m) % tiles_n, t % tiles_m


def tile_order(tiles_m: int, tiles_n: int, batch: int):
    return [(b, tn, tm) for b in range(batch) for tn in range(tiles_n) for tm in range(tiles_m)]


def tile_extent(tm: int, tn: int, m: int, wn: int, rows: int, tw: int):
    """(row0, row1, word0, word1) of the tile inside the matrix."""
    return tm * rows, min((tm + 1) * rows, m), tn * tw, min((tn + 1) * tw, wn)


def range_mask(m: int, wn: int, batch: int, rows: int, tw: int, tile_base: int, tile_count: int) -> np.ndarray:
    """(batch, m, wn) bool: the words of C that belong to the tiles [tile_base, tile_base + tile_count)."""
    tiles_m, tiles_n = tile_grid(m, wn, rows, tw)
    mask = np.zeros((batch, m, wn), dtype=bool)
    for t in range(tile_base, tile_base + tile_count):
        b, tn, tm = tile_of(t, tiles_m, tiles_n)
        r0, r1, w0, w1 = tile_extent(tm, tn, m, wn, rows, tw)
        mask[b, r0:r1, w0:w1] = True
    return mask


def slab_image(P: np.ndarray, tm: int, tn: int):
    """The dense slab of generation 4's tile (tm, tn) of the (m, wn) product P, and the mask of its words that mean something: (4096, 8)
    uint64 and bool.  Slab words outside the mask are not specified."""
    m, wn = P.shape
    r0, r1, w0, w1 = tile_extent(tm, tn, m, wn, G4_ROWS, G4_TW)
    img = np.zeros((G4_ROWS, G4_TW), dtype=np.uint64)
    valid = np.zeros((G4_ROWS, G4_TW), dtype=bool)
    img[:r1 - r0, :w1 - w0] = P[r0:r1, w0:w1]
    valid[:r1 - r0, :w1 - w0] = True
    return img, valid
