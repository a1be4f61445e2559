"""The plan of the host block pipeline (host_pipeline_plan.cpp, exported as m4ri_amd_plan_host_pipeline; mzd_api.hip run_pipelined
executes it and decides nothing itself), pinned without a GPU: whether a product from host memory is pipelined, the cuts of its block
grid and the staging arena's words at the shapes the design and tests/test_gpu_host_pipeline.py name; a restatement in Python of the
arithmetic, written from run_pipelined as it stood before the plan was moved out of it, over seeded random shapes; and the invariants
of the cuts over the same shapes."""
import numpy as np
import pytest

import m4ri_amd

MIB64 = 64 << 20


def plan(m, l, n, min_bytes=MIB64, grid=None):
    return m4ri_amd.plan_host_pipeline(m, l, n, min_bytes=min_bytes, grid=grid)


def words_of(ncols):
    return (ncols + 63) >> 6


def dev_words(rows, ncols):
    w = words_of(ncols)
    st = (w + 1) & ~1
    return ((rows if rows > 0 else 1) * (st if st > 0 else 2) + 31) & ~31


def coarse_cut(total, parts, i, unit0, prev, rows):
    target = total * i // parts
    fine = (target + 4095) // 4096 * 4096 if rows else target // 64 * 64
    for j in range(5, 0, -1):
        unit = unit0 << j
        c = (target + unit // 2) // unit * unit
        if c > prev and c < total and abs(c - target) * 100 <= 8 * (total // parts):
            return c
    return fine


def restated(m, l, n, min_bytes, env=()):
    """run_pipelined's decisions as the function made them itself; env: the numbers read from M4RI_AMD_PIPE_GRID.  Returns None (not
    pipelined) or (rcut, ccut, kcut, need)."""
    nbytes = (m * words_of(l) + l * words_of(n) + m * words_of(n)) * 8
    if min_bytes == 0 or nbytes < min_bytes or m < 4 * 4096:
        return None
    nenv = len(env)
    egi, egj, egk = (tuple(env) + (0, 0, 1)[nenv:])[:3]
    if nenv >= 2 and egi >= 1 and egj >= 1 and egk >= 1 and m >= egi * 4096 and n >= egj * 64 and l >= egk * 64:
        if nenv < 3:
            egk = 1
    elif n >= 16384:
        egi, egj = 2, 2
        egk = 2 if (l >= 65536 and m >= 65536 and n >= 65536) else 1
    else:
        srows = (m // 4 + 4095) // 4096 * 4096
        egi, egj, egk = (m + srows - 1) // srows, 1, 1
    if n >= 16384 or nenv >= 2:
        rcut = [0]
        for i in range(1, egi):
            rcut.append(coarse_cut(m, egi, i, 4096, rcut[-1], True))
        rcut.append(m)
    else:
        srows = (m // 4 + 4095) // 4096 * 4096
        rcut = list(range(0, m, srows)) + [m]
    ccut = [0]
    for j in range(1, egj):
        ccut.append(coarse_cut(n, egj, j, 1024, ccut[-1], False))
    ccut.append(n)
    kcut = [0]
    for k in range(1, egk):
        kcut.append(coarse_cut(l, egk, k, 1024, kcut[-1], False))
    kcut.append(l)
    return rcut, ccut, kcut, need_of(rcut, ccut, kcut)


def need_of(rcut, ccut, kcut):
    R, C, K = (np.diff(x).tolist() for x in (rcut, ccut, kcut))
    return (sum(dev_words(r, k) for r in R for k in K) + sum(dev_words(k, c) for k in K for c in C)
            + sum(dev_words(r, c) for r in R for c in C))


def steps(lo, hi, step):
    return list(range(lo, hi + 1, step))


NAMED = [
    ((65536, 65536, 65536), {}, [0, 32768, 65536], [0, 32768, 65536], [0, 32768, 65536], 201326592),
    ((32768, 32768, 32768), {}, [0, 16384, 32768], [0, 16384, 32768], [0, 32768], 50331648),
    ((65664, 65536, 65536), {}, [0, 32768, 65664], [0, 32768, 65536], [0, 32768, 65536], 201588736),   # 32768 + 32896 rows, not 36864 + 28800
    ((70000, 70000, 70000), {}, [0, 32768, 70000], [0, 32768, 70000], [0, 32768, 70000], 229740000),
    ((24576, 24576, 24576), {}, [0, 12288, 24576], [0, 12288, 24576], [0, 24576], 28311552),
    ((16384, 16384, 16384), {}, [0, 8192, 16384], [0, 8192, 16384], [0, 16384], 12582912),
    ((33000, 300, 16385), dict(min_bytes=1), [0, 16384, 33000], [0, 8192, 16385], [0, 300], 8789440),
    ((20001, 700, 17013), dict(min_bytes=1), [0, 12288, 20001], [0, 8192, 17013], [0, 700], 5746528),
    ((16500, 64, 30000), dict(min_bytes=1), [0, 8192, 16500], [0, 14336, 30000], [0, 64], 7818112),
    ((40000, 640, 640), dict(min_bytes=1), [0, 12288, 24576, 36864, 40000], [0, 640], [0, 640], 806400),   # row slabs: n < 16384
    ((16385, 64, 1), dict(min_bytes=1), [0, 4096, 8192, 12288, 16384, 16385], [0, 1], [0, 64], 65728),     # five slabs, not four
    ((16384, 1000, 900), dict(min_bytes=1), [0, 4096, 8192, 12288, 16384], [0, 900], [0, 1000], 540288),
    ((16384, 128, 128), dict(min_bytes=1, grid=(2, 2, 2)), [0, 8192, 16384], [0, 64, 128], [0, 64, 128], 131584),
    ((16421, 200, 130), dict(min_bytes=1, grid=(2, 2, 2)), [0, 8192, 16421], [0, 64, 130], [0, 64, 200], 165120),
    ((16384, 128, 128), dict(min_bytes=1, grid=(2, 2)), [0, 8192, 16384], [0, 64, 128], [0, 128], 98816),
    ((32768, 640, 256), dict(min_bytes=1, grid=(8, 2, 2)), steps(0, 32768, 4096), [0, 128, 256], [0, 320, 640], 526848),
]


@pytest.mark.parametrize("shape,kw,rcut,ccut,kcut,need", NAMED,
                         ids=["x".join(map(str, r[0])) + ("-grid" + "x".join(map(str, r[1]["grid"])) if "grid" in r[1] else "") for r in NAMED])
def test_plans_of_named_shapes(shape, kw, rcut, ccut, kcut, need):
    p = plan(*shape, **kw)
    assert p is not None and (p.rcut, p.ccut, p.kcut, p.arena_words) == (rcut, ccut, kcut, need), p
    assert p.grid == (len(rcut) - 1, len(ccut) - 1, len(kcut) - 1)


def test_products_that_are_not_pipelined():
    assert plan(16383, 70000, 70000) is None                # fewer than four tiles of rows
    assert plan(16384, 4096, 4096) is None                  # 24 MiB of operands, below the 64 MiB default
    assert plan(16384, 4096, 4096, min_bytes=1) is not None
    assert plan(16384, 16384, 16384, min_bytes=0) is None   # 0 switches the pipeline off
    old = m4ri_amd.set_host_pipeline(-1)                    # min_bytes=None: the library's current setting
    assert (m4ri_amd.plan_host_pipeline(16384, 16384, 16384) is None) == (old == 0 or old > 96 << 20)


def test_a_refused_grid_request_is_no_request():
    """Too few rows, words or inner bits for the requested grid, or numbers below 1: the default plan (for n < 16384 the row slabs)."""
    for shape, grid in [((16384, 1000, 900), (5, 1, 1)), ((40000, 640, 640), (2, 11, 1)), ((40000, 640, 640), (2, 2, 11)),
                        ((20000, 100, 100), (0, 2, 2)), ((20000, 100, 100), (2, 2, 0)), ((70000, 70000, 70000), (18, 1, 1))]:
        p, q = plan(*shape, min_bytes=1, grid=grid), plan(*shape, min_bytes=1)
        assert (p.rcut, p.ccut, p.kcut, p.arena_words) == (q.rcut, q.ccut, q.kcut, q.arena_words), (shape, grid)


def test_capacity_of_the_cut_arrays():
    """The C entry point with arrays too short for a list: -1, the grid and the arena words still written, no array touched."""
    import ctypes
    fn = m4ri_amd.lib().m4ri_amd_plan_host_pipeline
    cuts = [(ctypes.c_int64 * 5)(*([-7] * 5)) for _ in range(3)]
    grid, words = (ctypes.c_int * 3)(), ctypes.c_int64()
    ptr = [ctypes.cast(c, ctypes.c_void_p) for c in cuts]
    args = (40000, 640, 640, 1, 0, 0, 0)
    assert fn(*args, *ptr, 4, ctypes.cast(grid, ctypes.c_void_p), ctypes.cast(ctypes.pointer(words), ctypes.c_void_p)) == -1
    assert list(grid) == [4, 1, 1] and words.value == 806400 and all(list(c) == [-7] * 5 for c in cuts)
    assert fn(*args, *ptr, 5, None, None) == 1 and list(cuts[0]) == [0, 12288, 24576, 36864, 40000] and list(cuts[1])[:2] == [0, 640]
    assert fn(*args, None, None, None, 0, None, None) == 1
    assert fn(-1, 640, 640, 1, 0, 0, 0, None, None, None, 0, None, None) == 0


def random_shapes(count=720, seed=20240611):
    """(m, l, n, min_bytes, grid): m in 16384 ... 140000, l and n in 1 ... 140000, half of the dimensions on or within a few bits of a
    multiple of 1024 or 4096; every third case with a grid request up to 8 x 4 x 4 that the shape accepts (two or three numbers)."""
    rng = np.random.default_rng(seed)

    def dim(lo):
        if rng.random() < 0.5:
            unit = int(rng.choice([1024, 4096]))
            v = int(rng.integers((lo + unit - 1) // unit, 140000 // unit + 1)) * unit + int(rng.choice([0, 0, 1, -1, 37, -63, 64]))
        else:
            v = int(rng.integers(lo, 140001))
        return min(max(v, lo), 140000)

    out = []
    while len(out) < count:
        m, l, n = dim(16384), dim(1), dim(1)
        min_bytes = int(rng.choice([1, 1, MIB64]))
        grid = None
        if len(out) % 3 == 2:
            gi, gj, gk = int(rng.integers(1, min(8, m // 4096) + 1)), int(rng.integers(1, 5)), int(rng.integers(1, 5))
            if n < gj * 64 or l < gk * 64:
                continue
            grid = (gi, gj, gk) if rng.random() < 0.7 else (gi, gj)
        out.append((m, l, n, min_bytes, grid))
    return out


SHAPES = random_shapes()


def test_the_export_equals_the_restated_arithmetic():
    assert len(SHAPES) >= 600 and sum(g is not None for *_, g in SHAPES) >= len(SHAPES) // 3
    pipelined = 0
    for m, l, n, min_bytes, grid in SHAPES:
        want, p = restated(m, l, n, min_bytes, grid or ()), plan(m, l, n, min_bytes, grid)
        assert (want is None) == (p is None), (m, l, n, min_bytes, grid)
        if p is not None:
            pipelined += 1
            assert (p.rcut, p.ccut, p.kcut, p.arena_words) == want, (m, l, n, min_bytes, grid, p)
            if grid is not None:
                assert p.grid == (tuple(grid) + (1,))[:3], (m, l, n, grid, p)   # an accepted request is the grid
    assert pipelined >= 500


def test_invariants_of_the_cuts():
    for m, l, n, min_bytes, grid in SHAPES:
        p = plan(m, l, n, min_bytes, grid)
        if p is None:
            continue
        what = (m, l, n, min_bytes, grid, p)
        for cuts, total in ((p.rcut, m), (p.ccut, n), (p.kcut, l)):
            assert cuts[0] == 0 and cuts[-1] == total and all(a < b for a, b in zip(cuts, cuts[1:])), what
        assert all(r % 4096 == 0 for r in p.rcut[:-1]), what      # whole tiles of rows in every block before the last
        assert all(c % 64 == 0 for c in p.ccut[:-1] + p.kcut[:-1]), what   # whole words
        assert p.arena_words == need_of(p.rcut, p.ccut, p.kcut), what


def test_the_plan_takes_no_add_argument():
    """C = A * B and C += A * B run the same plan: the entry point has no parameter that could tell them apart (C's blocks take their
    arena words either way, uploaded or only placed)."""
    import inspect
    assert list(inspect.signature(m4ri_amd.plan_host_pipeline).parameters) == ["m", "l", "n", "min_bytes", "grid"]
    assert len(m4ri_amd.lib().m4ri_amd_plan_host_pipeline.argtypes) == 13
