"""What m4ri_amd_echelonize_order_batch_dev and m4ri_amd_random_orders_batch_dev (include/m4ri_amd.h) have to give, in NumPy and plain
Python on the unpacked bits of one member, and the host images the GPU tests pack them into.  tests/test_echelonize_order_plan.py pins
these to the oracle's gf2o_echelonize and to hand-written cases; tests/test_gpu_echelonize_order_batch.py judges the kernels with them."""
import numpy as np

MASK64 = (1 << 64) - 1


def ech_order(bits, order, full, pivot_rows):
    """The rule of the header, literally.  bits: uint8 nrows x ncols; order: the visited columns (None: all, left to right).
    Returns (the form, rank, pivots of min(pivot_rows, ncols) entries); a member with an entry out of range comes back unchanged with
    rank -1 and pivots -1."""
    bits = np.array(bits, dtype=np.uint8) & 1
    nrows, ncols = bits.shape
    order = list(range(ncols)) if order is None else [int(c) for c in order]
    piv = np.full(min(pivot_rows, ncols), -1, dtype=np.int32)
    if any(c < 0 or c >= ncols for c in order):
        return bits, -1, piv
    M = to_words(bits)   # the rows as packed words: a row addition is one XOR of `width` words
    rank = 0
    for c in order:
        if rank >= pivot_rows:
            break
        col = (M[:, c >> 6] >> np.uint64(c & 63)) & np.uint64(1)
        hits = np.flatnonzero(col[rank:pivot_rows])
        if hits.size == 0:
            continue
        i = rank + int(hits[0])
        M[[rank, i]] = M[[i, rank]]
        col[[rank, i]] = col[[i, rank]]
        col[rank] = 0                                   # every OTHER row with the bit
        if not full:
            col[:rank] = 0                              # the rows > rank only
        M[np.flatnonzero(col)] ^= M[rank]
        piv[rank] = c
        rank += 1
    return from_words(M, ncols), rank, piv


def splitmix(seed, k):
    """Output number k of the counter-form splitmix64 stream seeded `seed`, in plain integers."""
    z = (seed + (k + 1) * 0x9E3779B97F4A7C15) & MASK64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK64
    return z ^ (z >> 31)


def random_order(seed, b, n):
    """Member b's permutation of 0 .. n-1: the keys (output b * n + j with its low 12 bits replaced by j) sorted ascending, their low
    12 bits."""
    keys = sorted((splitmix(seed, b * n + j) & ~4095) | j for j in range(n))
    return np.array([k & 4095 for k in keys], dtype=np.int32)


def transpositions(perm):
    """The sequence P that m4ri_amd_apply_p_right_batch_dev takes to GATHER the columns: after the swaps (i, P[i]), i = n-1 down to 0
    (trans = 0), column i is the old column perm[i]; the same P ascending (trans = 1) scatters them back."""
    n = len(perm)
    at, pos = list(range(n)), list(range(n))   # at[p]: the old column at position p; pos[c]: where old column c is
    P = np.zeros(n, dtype=np.int32)
    for i in range(n - 1, -1, -1):
        p = pos[int(perm[i])]
        assert p <= i, "not a permutation"
        P[i] = p
        a, c = at[i], at[p]
        at[i], at[p], pos[c], pos[a] = c, a, i, p
    return P


def to_words(bits):
    """uint8 nrows x ncols -> uint64 nrows x words(ncols), bit c of a row at word c // 64, bit c % 64."""
    nrows, ncols = bits.shape
    width = (ncols + 63) // 64
    if nrows == 0 or width == 0:
        return np.zeros((nrows, width), dtype=np.uint64)
    pad = np.zeros((nrows, width * 64), dtype=np.uint8)
    pad[:, :ncols] = bits & 1
    return np.packbits(pad, axis=1, bitorder="little").view(np.uint64).reshape(nrows, width)


def from_words(words, ncols):
    """The inverse of to_words."""
    nrows = words.shape[0]
    if nrows == 0 or ncols == 0:
        return np.zeros((nrows, ncols), dtype=np.uint8)
    return np.unpackbits(np.ascontiguousarray(words).view(np.uint8).reshape(nrows, -1), axis=1, bitorder="little")[:, :ncols]


def word_masks(ncols):
    valid = np.full((ncols + 63) // 64, ~np.uint64(0), dtype=np.uint64)
    if ncols % 64:
        valid[-1] = np.uint64((1 << (ncols % 64)) - 1)
    return valid


def index(nrows, ncols, batch, stride, bs):
    """The word offsets of the members' valid words, batch x nrows x width."""
    width = (ncols + 63) // 64
    return (np.arange(batch, dtype=np.int64)[:, None, None] * bs + np.arange(nrows, dtype=np.int64)[None, :, None] * stride
            + np.arange(width, dtype=np.int64)[None, None, :])


def pack(members, nrows, ncols, stride, bs, seed):
    """The host image of a batch of bit matrices: padding words, tail bits and the gaps between members random, the valid bits the
    members'.  Returns (image, index, masks)."""
    batch = len(members)
    total = (batch - 1) * bs + nrows * stride + 5
    rng = np.random.default_rng(seed)
    h = rng.integers(0, 1 << 63, size=total, dtype=np.int64).view(np.uint64) * np.uint64(3)
    idx, valid = index(nrows, ncols, batch, stride, bs), word_masks(ncols)
    if nrows and ncols:
        h[idx] = (h[idx] & ~valid) | (np.stack([to_words(M) for M in members]) & valid)
    return h, idx, valid


def put(image, idx, valid, b, bits):
    """Member b's valid bits of the image <- bits, everything else as it is."""
    if bits.size:
        image[idx[b]] = (image[idx[b]] & ~valid) | (to_words(bits) & valid)
