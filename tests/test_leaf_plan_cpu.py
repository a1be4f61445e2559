"""The plan of one leaf launch (engine.hip plan_leaf_launch, exported as m4ri_amd_plan_leaf_launch; launch_leaf_one executes it and decides
nothing itself), pinned without a GPU: the branches at the shapes tests/test_gpu_leaf_launch.py runs, for 256 compute units; the
invariants between its fields over seeded random shapes; and, over the same shapes, a restatement of the cost model in Python, written
from the launch function as it stood before the plan was moved out of it."""
import os

import numpy as np
import pytest

import m4ri_amd
from m4ri_amd import ZERO_ALL, ZERO_NOTHING, ZERO_TAIL

KNOBS = ("M4RI_AMD_LEAF_GEN", "M4RI_AMD_SMALL_LEAF", "M4RI_AMD_SMALL_LEAF_WORK", "M4RI_AMD_SMALL_KS", "M4RI_AMD_TAIL_KSPLIT")
SLABS = 768  # engine.hip PART_SLABS


@pytest.fixture(autouse=True)
def _own_plan():
    if any(os.environ.get(k) for k in KNOBS):
        pytest.skip("the leaf launch's plan is overridden by the environment")


def plan(m, l, n, batch=1, **kw):
    kw.setdefault("cus", 256)
    return m4ri_amd.plan_leaf_launch(m, l, n, batch, **kw)


def fields(p, *names):
    return tuple(getattr(p, k) for k in names)


ALL = ("gen", "rg", "tile_rows", "tile_words", "tiles", "ksplit", "tail_tiles", "tail_ksplit", "mode", "tail_mode", "slabs", "zero", "pack_a")


@pytest.mark.parametrize("shape,kw,want", [
    #  (m, l, n, batch)                                 gen rg rows  tw tiles ks tail tks mode tmode slabs zero pack
    ((192, 704, 512, 256), {},                          (4, 0, 4096, 8, 256, 1, 0, 1, 0, 0, 0, 0, 1)),   # one full round: unsplit, no tail
    ((192, 1024, 512, 300), {},                         (4, 0, 4096, 8, 300, 1, 44, 4, 0, 2, 1, 0, 1)),  # hybrid: the 44 tiles of the last round split 4 ways, slabs
    ((192, 1024, 512, 257), {},                         (4, 0, 4096, 8, 257, 1, 1, 8, 0, 2, 1, 0, 1)),   # hybrid: a tail of one tile
    ((200, 1024, 153523, 1), {},                        (4, 0, 4096, 8, 300, 1, 44, 4, 0, 2, 1, 0, 1)),  # one product, last column tile and last word ragged
    ((192, 2048, 512, 100), {},                         (4, 0, 4096, 8, 100, 2, 0, 1, 2, 0, 1, 0, 1)),   # the whole launch split in 2, slabs
    ((300, 8192, 1000, 9), {},                          (4, 0, 4096, 8, 18, 13, 0, 1, 2, 0, 1, 0, 1)),   # ... in 13
    ((192, 512, 51200, 1), dict(ksplit=8),              (4, 0, 4096, 8, 100, 8, 0, 1, 1, 0, 0, 1, 1)),   # 100 tiles x 8 > 768 slabs: atomics, all of C cleared
    ((192, 512, 51200, 1), dict(ksplit=8, add=True),    (4, 0, 4096, 8, 100, 8, 0, 1, 1, 0, 0, 0, 1)),   # ... accumulating: nothing cleared
    ((192, 512, 51200, 1), dict(ksplit=7),              (4, 0, 4096, 8, 100, 4, 0, 1, 2, 0, 1, 0, 1)),   # 7 asked, 4 made (16 dwords of A in pairs): 400 slabs
    ((100, 2048, 3000, 1), dict(ksplit=4),              (1, 16, 512, 32, 2, 4, 0, 1, 1, 0, 0, 1, 0)),    # generation 1, 512-row tiles, atomics
    ((100, 2048, 3000, 1), dict(ksplit=1, add=True),    (1, 16, 512, 32, 2, 1, 0, 1, 1, 0, 0, 0, 0)),
    ((300, 100, 1000, 1), dict(ksplit=64),              (4, 0, 4096, 8, 2, 2, 0, 1, 2, 0, 1, 0, 1)),     # more splits asked than four dwords of A allow
    ((100, 100, 3000, 1), dict(ksplit=64),              (1, 16, 512, 32, 2, 64, 0, 1, 1, 0, 0, 1, 0)),   # generation 1 rounds in its launcher
    # the generation-4 rows without the scratch: generation 1 in 1024-row tiles, the launch's split kept and met by atomics, no tail
    ((192, 704, 512, 256), dict(scratch_ok=False),      (1, 32, 1024, 32, 256, 1, 0, 1, 0, 0, 0, 0, 0)),
    ((192, 1024, 512, 300), dict(scratch_ok=False),     (1, 32, 1024, 32, 300, 1, 0, 1, 0, 0, 0, 0, 0)),
    ((192, 1024, 512, 300), dict(scratch_ok=False, add=True), (1, 32, 1024, 32, 300, 1, 0, 1, 1, 0, 0, 0, 0)),
    ((192, 1024, 512, 257), dict(scratch_ok=False),     (1, 32, 1024, 32, 257, 1, 0, 1, 0, 0, 0, 0, 0)),
    ((200, 1024, 153523, 1), dict(scratch_ok=False),    (1, 32, 1024, 32, 75, 1, 0, 1, 0, 0, 0, 0, 0)),
    ((192, 2048, 512, 100), dict(scratch_ok=False),     (1, 32, 1024, 32, 100, 2, 0, 1, 1, 0, 0, 1, 0)),
    ((300, 8192, 1000, 9), dict(scratch_ok=False),      (1, 32, 1024, 32, 9, 13, 0, 1, 1, 0, 0, 1, 0)),
    ((300, 8192, 1000, 9), dict(scratch_ok=False, add=True), (1, 32, 1024, 32, 9, 13, 0, 1, 1, 0, 0, 0, 0)),
    ((192, 512, 51200, 1), dict(ksplit=8, scratch_ok=False), (1, 32, 1024, 32, 25, 8, 0, 1, 1, 0, 0, 1, 0)),
    # the small leaf and its inner split
    ((256, 8192, 512, 1), {},                           (5, 0, 256, 8, 1, 43, 0, 1, 1, 0, 0, 1, 0)),
    ((256, 8192, 512, 1), dict(add=True),               (5, 0, 256, 8, 1, 43, 0, 1, 1, 0, 0, 0, 0)),
    ((4096, 256, 4096, 1), {},                          (5, 0, 256, 8, 128, 1, 0, 1, 0, 0, 0, 0, 0)),
    ((256, 8192, 512, 1), dict(ksplit=1),               (4, 0, 4096, 8, 1, 1, 0, 1, 0, 0, 0, 0, 1)),     # a requested split is generation 4's or 1's
])
def test_plans_at_256_compute_units(shape, kw, want):
    p = plan(*shape, **kw)
    assert fields(p, *ALL) == want, p


def test_small_leaf_up_to_2_to_the_34_bit_operations():
    """At the bound the small leaf, one column more generation 4; the small leaf's split is m4ri_amd_plan_small_leaf's."""
    small = m4ri_amd.lib().m4ri_amd_plan_small_leaf
    at, above = (1024, 1024, 16384), (1024, 1024, 16385)
    assert at[0] * at[1] * at[2] == 1 << 34
    p, q = plan(*at), plan(*above)
    assert p.gen == 5 and p.ksplit == small(*at, 1, 256) and q.gen == 4 and small(*above, 1, 256) == 0
    assert plan(1024, 1024, 1024, 16).gen == 5 and plan(1024, 1024, 1024, 17).gen == 4  # the batch counts
    for shape, batch in [((512, 512, 512), 1), ((2048, 2048, 2048), 1), ((64, 1 << 20, 64), 1), ((1536, 1536, 1536), 1), ((1024, 1024, 1024), 4)]:
        for ncu in (256, 8, 304):
            p = plan(*shape, batch, cus=ncu)
            assert (p.gen, p.ksplit) == (5, small(*shape, batch, ncu)), (shape, batch, ncu, p)
            assert p.zero == (ZERO_ALL if p.ksplit > 1 else ZERO_NOTHING) and p.mode == (1 if p.ksplit > 1 else 0)
    assert plan(512, 512, 512, a_prepacked=True).gen == 4     # a packed A is generation 4's


def test_nothing_to_multiply():
    for add, zero in ((False, ZERO_ALL), (True, ZERO_NOTHING)):
        for kw in ({}, dict(ksplit=4), dict(scratch_ok=False), dict(a_prepacked=True)):
            p = plan(300, 0, 200, 3, add=add, **kw)
            assert fields(p, "gen", "zero", "pack_a", "slabs", "tail_tiles") == (0, zero, 0, 0, 0), (add, kw, p)
    for shape in ((0, 5, 5, 1), (5, 5, 0, 1), (5, 5, 5, 0)):
        assert fields(plan(*shape), "gen", "zero") == (0, ZERO_NOTHING)


def test_what_the_plan_refuses():
    L, out = m4ri_amd.lib(), m4ri_amd.LeafPlan()
    import ctypes
    call = lambda *a: L.m4ri_amd_plan_leaf_launch(*a, ctypes.byref(out))  # noqa: E731
    assert call(64, 64, 64, 1, 0, 0, 256, 0, 1) == 0
    assert call(-1, 64, 64, 1, 0, 0, 256, 0, 1) == 1 and call(1 << 31, 64, 64, 1, 0, 0, 256, 0, 1) == 1 and call(64, 64, 1 << 31, 1, 0, 0, 256, 0, 1) == 1
    assert L.m4ri_amd_plan_leaf_launch(64, 64, 64, 1, 0, 0, 256, 0, 1, None) == 1
    assert call(100, 4096, 4096, 1, 0, 0, 256, 1, 1) == 1     # a packed A for a shape generation 1 takes
    assert call(4096, 4096, 4096, 1, 0, 0, 256, 1, 0) == 1    # ... or without the scratch that would hold it
    assert call(4096, 4096, 4096, 1, 0, 0, 256, 1, 1) == 0 and out.gen == 4 and out.pack_a == 0
    assert plan(300, 1024, 512, 3, cus=0).ksplit == plan(300, 1024, 512, 3, cus=256).ksplit == plan(300, 1024, 512, 3, cus=-5).ksplit


# ---- the model, restated ---------------------------------------------------------------------------------------------------------------------
KINDS = ((4, 32, 4096, 6.7), (1, 32, 1024, 4.1), (1, 24, 768, 3.4), (1, 16, 512, 2.8))   # generation, rg, tile rows, relative rate


def model_kind(m, l, n):
    def cheapest(kinds):
        best, best_cost = KINDS[1], 1e300
        for k in kinds:
            cost = float(-(-m // k[2]) * k[2]) / k[3]
            if cost < best_cost:
                best, best_cost = k, cost
        return best
    ln = float(l) * float(n)
    if n >= 16384 and ((m <= 512 and ln >= 268435456.0) or (m <= 1024 and ln >= 1073741824.0)):
        return cheapest([k for k in KINDS if k[0] == 1])     # a few rows against a large B
    return KINDS[0] if m >= 192 else cheapest(KINDS)


def g4_splits(l, ks):
    """The splits generation 4 makes of `ks` asked: an even number of 32-bit chunks of A each, at least two."""
    nq = 2 * ((l + 63) // 64)
    per = -(-nq // max(ks, 1))
    per = max(per + (per & 1), 2)
    return -(-nq // per)


def model_plan(m, l, n, batch, add, ksplit_req, cus, scratch_ok):
    """(gen, rg, ksplit, tail_tiles, tail_ksplit, mode, tail_mode, slabs, zero, pack_a) of a launch the small leaf does not take."""
    gen, rg, rows, _ = model_kind(m, l, n)
    wn = (n + 63) // 64
    tw = 8 if gen == 4 else 32
    tiles = -(-m // rows) * -(-wn // tw) * batch
    sbits = 32 if gen == 4 else 16
    stages = -(-l // sbits)
    ksplit, tail_tiles, tail_ksplit = ksplit_req, 0, 1
    if ksplit <= 0:
        fixed = 192.0 / sbits

        def split_cost(nt, ks):
            return (256.0 + 2.0 * float(nt * ks)) / sbits if gen == 4 else 512.0 / sbits

        def cost(ks):
            rounds = -(-tiles * ks // cus)
            return float(rounds) * (float(-(-stages // ks)) + fixed + (split_cost(tiles, ks) if ks > 1 else 0.0))
        cap = min(max(stages * sbits // (128 if gen == 4 else 512), 1), 32)
        ksplit, best = 1, cost(1) * 0.97
        for ks in range(2, cap + 1):
            if cost(ks) < best:
                best, ksplit = cost(ks), ks
        if gen == 4 and tiles > cus and tiles % cus:
            rem, full = tiles % cus, tiles // cus
            for ks in range(2, cap + 1):
                rounds = -(-rem * ks // cus)
                c = float(full) * (float(stages) + fixed) + float(rounds) * (float(-(-stages // ks)) + fixed) + (256.0 + 1.0 * float(rem * ks)) / sbits
                if c < best * 0.99:
                    best, tail_tiles, tail_ksplit = c, rem, ks
            if tail_tiles:
                ksplit = 1
    if gen == 4:
        ksplit, tail_ksplit = g4_splits(l, ksplit), g4_splits(l, tail_ksplit)
    fits = gen == 4 and scratch_ok
    if tail_tiles:
        slabs = fits and tail_tiles * tail_ksplit <= SLABS
    else:
        slabs = fits and ksplit > 1 and tiles * ksplit <= SLABS
    zero = ZERO_ALL if ksplit > 1 and not add and not slabs else ZERO_NOTHING
    mode = 2 if ksplit > 1 and slabs else 1 if add or ksplit > 1 else 0
    pack, tail_mode = 0, 0
    if gen == 4 and not fits:
        gen, rg, tail_tiles, tail_ksplit = 1, 32, 0, 1
    elif gen == 4:
        pack = 1
        if tail_tiles:
            tail_mode = 2 if slabs else 1
            if not add and not slabs:
                zero = ZERO_TAIL
    return (gen, rg if gen == 1 else 0, ksplit, tail_tiles, tail_ksplit, mode, tail_mode, int(slabs), zero, pack)


def random_launches(count, seed):
    """Seeded shapes over every region of the plan: few and many tiles, batches around whole rounds of several compute-unit counts,
    short and long inner dimensions, requested splits, the scratch present and absent."""
    r = np.random.default_rng(seed)
    for i in range(count):
        ncu = int(r.choice([256, 256, 304, 120, 8]))
        m = int(r.choice([r.integers(1, 192), r.integers(192, 700), r.integers(700, 9000)]))
        l = int(r.choice([r.integers(1, 300), r.integers(300, 3000), r.integers(3000, 40000)]))
        n = int(r.choice([r.integers(1, 600), r.integers(600, 5000), r.integers(5000, 200000)]))
        batch = int(r.choice([1, 1, r.integers(2, 12), ncu + int(r.integers(-3, 60)), 2 * ncu + int(r.integers(1, ncu))]))
        if i % 3 == 0:  # batches of one tile each: whole rounds and a little more
            m, n = int(r.integers(192, 4097)), int(r.integers(1, 513))
        ksplit = int(r.choice([0, 0, 0, 1, 2, 3, 8, 64]))
        yield m, l, n, batch, bool(r.integers(0, 2)), ksplit, ncu, bool(r.integers(0, 4))


def test_invariants_of_the_plan_over_random_launches():
    seen = set()
    for (m, l, n, batch, add, ksplit, ncu, ok) in random_launches(600, 20260):
        p = plan(m, l, n, batch, add=add, ksplit=ksplit, cus=ncu, scratch_ok=ok)
        what = ((m, l, n, batch, add, ksplit, ncu, ok), p)
        assert p.gen in (1, 4, 5) and p.tiles == p.tiles_m * p.tiles_n * batch and p.tiles_m == -(-m // p.tile_rows), what
        assert p.tiles_n == -(-((n + 63) // 64) // p.tile_words) and p.ksplit >= 1 and p.tail_ksplit >= 1, what
        assert 0 <= p.tail_tiles < ncu and p.tail_tiles < p.tiles, what
        if p.tail_tiles:                                   # a tail excludes a whole-launch split, and is generation 4's
            assert p.ksplit == 1 and p.gen == 4 and p.tail_ksplit > 1 and p.tail_tiles == p.tiles % ncu, what
        else:
            assert p.tail_ksplit == 1 and p.tail_mode == 0, what
        if p.slabs:
            assert p.gen == 4 and ok and (p.tail_tiles * p.tail_ksplit if p.tail_tiles else p.tiles * p.ksplit) <= SLABS, what
        assert (p.mode == 2) == bool(p.slabs and p.ksplit > 1), what             # mode 2 exactly when slabs are used and something is split
        assert (p.tail_mode == 2) == bool(p.slabs and p.tail_tiles), what
        assert p.slabs == int((p.mode == 2) or (p.tail_mode == 2)), what
        if p.mode == 0:
            assert not add and p.ksplit == 1, what
        atomics = (p.ksplit > 1 or p.tail_tiles > 0) and not p.slabs
        assert p.zero == (ZERO_NOTHING if add or not atomics else ZERO_TAIL if p.tail_tiles else ZERO_ALL), what   # cleared exactly when splits meet by atomics and add is off
        assert p.pack_a == int(p.gen == 4) and (p.rg > 0) == (p.gen == 1), what
        if ksplit > 0:
            assert p.gen != 5 and p.tail_tiles == 0, what
        seen.add((p.gen, bool(p.tail_tiles), p.ksplit > 1, bool(p.slabs), p.zero))
    # the shapes reach every branch: unsplit, split and hybrid generation 4 with slabs and with atomics, generation 1 by shape and by fallback, the small leaf
    for branch in [(4, False, False, False, 0), (4, False, True, True, 0), (4, False, True, False, 1), (4, True, False, True, 0),
                   (1, False, False, False, 0), (1, False, True, False, 1), (5, False, False, False, 0), (5, False, True, False, 1)]:
        assert branch in seen, branch


def test_plan_is_the_cost_model_of_the_launch_function():
    """The restated model and the library agree on every field, launch by launch."""
    checked = 0
    for (m, l, n, batch, add, ksplit, ncu, ok) in random_launches(600, 20261):
        p = plan(m, l, n, batch, add=add, ksplit=ksplit, cus=ncu, scratch_ok=ok)
        if p.gen == 5:
            assert ksplit <= 0 and m4ri_amd.lib().m4ri_amd_plan_small_leaf(m, l, n, batch, ncu) == p.ksplit
            continue
        got = fields(p, "gen", "rg", "ksplit", "tail_tiles", "tail_ksplit", "mode", "tail_mode", "slabs", "zero", "pack_a")
        assert got == model_plan(m, l, n, batch, add, ksplit, ncu, ok), ((m, l, n, batch, add, ksplit, ncu, ok), p)
        checked += 1
    assert checked > 300
