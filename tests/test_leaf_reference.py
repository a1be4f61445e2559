"""The NumPy reference of the M4RM leaves (tests/leaf_reference.py) is proven on the CPU before it judges a kernel.

  * Its whole-word product equals the CPU oracle's gf2o_mul / gf2o_addmul on ragged shapes (B is handed to the oracle as l x 64 wn bits, so
    every bit of its last word is a column of the product; the bits of A from column l on hold junk for the reference and are masked for
    the oracle, which wants them zero).
  * The partial products of the inner splits of every generation XOR to the whole product, and the splits tile [0, l) in order.
  * The tile order maps every (batch member, tile_n, tile_m) exactly once, tile_m fastest; the range masks of a partition of the tiles
    partition C; a slab image holds the tile's words and marks nothing else.
No GPU anywhere in this module.
"""
import numpy as np
import pytest

import leaf_reference as ref
from m4ri_amd.mzd import Mzd

SHAPES = [(1, 1, 1), (3, 131, 257), (5, 64, 64), (70, 63, 65), (33, 65, 511), (17, 777, 1234), (40, 300, 513), (9, 2049, 100)]


def _mzd_of(words: np.ndarray, ncols=None) -> Mzd:
    rows, w = words.shape
    return Mzd(rows, 64 * w if ncols is None else ncols, np.ascontiguousarray(words).reshape(-1).copy(), rowstride=w)


def _words_of(M: Mzd) -> np.ndarray:
    return M.rows()[:, :M.width].copy()


def _operands(m, l, n, seed=0):
    rng = np.random.default_rng(1000 * m + l + n + seed)
    wl, wn = ref.words_of(l), ref.words_of(n)
    A = rng.integers(0, 1 << 64, size=(m, wl), dtype=np.uint64)     # junk from column l on
    B = rng.integers(0, 1 << 64, size=(l, wn), dtype=np.uint64)     # whole words
    Am = A.copy()
    if l % 64:
        Am[:, -1] &= np.uint64((1 << (l % 64)) - 1)
    return A, Am, B


@pytest.mark.parametrize("m,l,n", SHAPES)
def test_the_product_is_the_oracles(oracle, m, l, n):
    A, Am, B = _operands(m, l, n)
    want = _words_of(oracle.mul(None, _mzd_of(Am, l), _mzd_of(B), 0))
    got = ref.product(A, B, l)
    assert got.dtype == np.uint64 and np.array_equal(got, want)
    assert np.array_equal(ref.product(Am, B, l), want), "the bits of A beyond column l reached the product"
    C0 = np.random.default_rng(7).integers(0, 1 << 64, size=want.shape, dtype=np.uint64)
    want_acc = _words_of(oracle.addmul(_mzd_of(C0), _mzd_of(Am, l), _mzd_of(B), 0))
    assert np.array_equal(C0 ^ got, want_acc)


@pytest.mark.parametrize("gen", [1, 4, 5])
@pytest.mark.parametrize("m,l,n", SHAPES)
def test_split_partials_xor_to_the_product(gen, m, l, n):
    A, _, B = _operands(m, l, n, seed=gen)
    whole = ref.product(A, B, l)
    unit = {1: 16, 4: 32, 5: 64}[gen]
    for ks in (1, 2, 3, 4, 7, 16, 1000):
        bounds = ref.split_bounds(gen, l, ks)
        assert 1 <= len(bounds) <= ks
        assert bounds[0][0] == 0 and bounds[-1][1] == l and all(a[1] == b[0] for a, b in zip(bounds, bounds[1:]))
        assert all(k0 < k1 and k0 % unit == 0 for (k0, k1) in bounds)
        sizes = {k1 - k0 for (k0, k1) in bounds[:-1]}
        assert len(sizes) <= 1 and all(s % (2 * unit if gen != 5 else unit) == 0 for s in sizes)
        acc = np.zeros_like(whole)
        for p in ref.partials(A, B, l, bounds):
            acc ^= p
        assert np.array_equal(acc, whole), (gen, ks, bounds)
    assert ref.split_bounds(gen, 0, 3) == [(0, 0)]


def test_split_counts_by_hand():
    # generation 4: 2 dwords per word of A, an even number per split
    assert len(ref.split_bounds(4, 64, 4)) == 1 and len(ref.split_bounds(4, 65, 2)) == 2 and len(ref.split_bounds(4, 65, 3)) == 2
    assert ref.split_bounds(4, 300, 3) == [(0, 128), (128, 256), (256, 300)]        # 10 dwords: 4 + 4 + 2
    assert ref.split_bounds(4, 300, 4) == [(0, 128), (128, 256), (256, 300)]        # asked for 4, gets 3
    # generation 1: 16-bit stages, an even number per split
    assert ref.split_bounds(1, 300, 3) == [(0, 128), (128, 256), (256, 300)]        # 19 stages: 8 + 8 + 3
    assert ref.split_bounds(1, 65, 2) == [(0, 64), (64, 65)]                        # 5 stages: 4 + 1
    assert len(ref.split_bounds(1, 32, 2)) == 1
    # generation 5: words of A, capped at their number
    assert ref.split_bounds(5, 300, 3) == [(0, 128), (128, 256), (256, 300)]        # 5 words: 2 + 2 + 1
    assert ref.split_bounds(5, 300, 4) == [(0, 128), (128, 256), (256, 300)]
    assert len(ref.split_bounds(5, 300, 99)) == 5 and len(ref.split_bounds(5, 64, 2)) == 1


@pytest.mark.parametrize("tiles_m,tiles_n,batch", [(1, 1, 1), (3, 1, 2), (1, 4, 1), (2, 3, 5)])
def test_the_tile_order_maps_every_tile_once(tiles_m, tiles_n, batch):
    order = ref.tile_order(tiles_m, tiles_n, batch)
    assert len(order) == len(set(order)) == tiles_m * tiles_n * batch
    assert set(order) == {(b, tn, tm) for b in range(batch) for tn in range(tiles_n) for tm in range(tiles_m)}
    for t, triple in enumerate(order):
        assert ref.tile_of(t, tiles_m, tiles_n) == triple
    # tile_m fastest, then tile_n, then the member
    assert order[0] == (0, 0, 0)
    if tiles_m > 1:
        assert order[1] == (0, 0, 1)
    if tiles_n > 1:
        assert order[tiles_m] == (0, 1, 0)
    if batch > 1:
        assert order[tiles_m * tiles_n] == (1, 0, 0)


@pytest.mark.parametrize("m,wn,batch,rows,tw", [(4097, 9, 2, 4096, 8), (300, 20, 1, 256, 8), (1025, 33, 2, 512, 32), (1, 1, 1, 4096, 8)])
def test_range_masks_partition_c(m, wn, batch, rows, tw):
    tiles_m, tiles_n = ref.tile_grid(m, wn, rows, tw)
    T = tiles_m * tiles_n * batch
    count = np.zeros((batch, m, wn), dtype=np.int64)
    for t in range(T):
        one = ref.range_mask(m, wn, batch, rows, tw, t, 1)
        b, tn, tm = ref.tile_of(t, tiles_m, tiles_n)
        assert one[b].any() and not np.delete(one, b, axis=0).any()
        count += one
    assert (count == 1).all()
    cut = T // 2
    assert np.array_equal(ref.range_mask(m, wn, batch, rows, tw, 0, cut) | ref.range_mask(m, wn, batch, rows, tw, cut, T - cut), count == 1)


def test_slab_image():
    P = np.arange(1, 4100 * 9 + 1, dtype=np.uint64).reshape(4100, 9)
    img, valid = ref.slab_image(P, 0, 0)
    assert valid.all() and np.array_equal(img, P[:4096, :8])
    img, valid = ref.slab_image(P, 1, 1)
    assert valid.sum() == 4 and np.array_equal(img[:4, 0], P[4096:, 8]) and valid[:4, 0].all() and not img[~valid].any()
    assert img.shape == (ref.G4_ROWS, ref.G4_TW) and img.size == ref.SLAB_WORDS
