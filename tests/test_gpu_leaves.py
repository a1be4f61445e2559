"""Every M4RM leaf kernel and every way its inner splits combine, called directly and compared word for word with the NumPy reference
(tests/leaf_reference.py, proven on the CPU by tests/test_leaf_reference.py).  Run this module first when you touch a leaf: a case works
on megabytes, and a mismatch names the row, the batch member, the tile, the row and the word, and which split's partial explains it.

The launchers of m4ri_amd/csrc/gf2_internal.h -- gf2_launch_m4rm_leaf / _variant (generation 1, m4rm_leaf.hip), gf2_launch_m4rm8q with
gf2_launch_a4_pack_rot (generation 4, m4rm8q_leaf.hip, a4_pack.hip), gf2_launch_m4rm_small (generation 5, m4rm_small.hip) and the
helpers of a split launch, gf2_launch_reduce_partials and gf2_launch_zero_tiles (aux_kernels.hip) -- are reached through the test-only
library tests/leaf_lib.py binds, so every configuration is run whatever engine.hip's launch_leaf_one would pick on the chip at hand.
Every row checks

  * the result, equal to the reference in every word of every row of C, the excess bits of the last word included;
  * the frame, which holds its poison (all ones): the row padding of C, the gaps between batch members, a guard block before and after C,
    guard blocks around the slab buffer and every slab beyond tiles x effective split; the tiles outside a launch's tile range;
  * A, B and the packed A, unchanged;
  * the launcher's answer: success, or hipErrorInvalidValue for what it documents as refused -- and then nothing written.

The operands are views: rows padded by an odd number of poisoned words, bases only 8-byte aligned, gaps between batch members.  A's
bits from column l on hold junk in every row (generation 5 documents that they never matter; for generations 1 and 4 the same follows
from B's descriptor bound: rows of B from l on read as zero), and generation 4 is fed the NumPy-packed A (pass_reference.pack_a4) with
that junk in it, so the leaf is tested apart from the pack pass; the rows with pack = "kernel" go through gf2_launch_a4_pack_rot(rot = 1).
Mode 2 rows also compare every slab with the dense image of its split's partial product (the tile's valid rows and words only) before
the reduce pass runs.

ROWS below is the parameter table as data: per row the kernel instantiation(s) it must reach (`reach`, written out from the launchers'
dispatch) and why.  test_the_table_names_every_instantiation compares the table with the instantiations in the sources.

Wall time of the module on one MI355X: 6 s (WALL_TIME below) -- the class of tests/test_gpu_passes.py.

Not in scope:
  * grids beyond 2^31 - 1 workgroups (the launchers' refusal of them): no array that large is allocated here;
  * packed operands of 4 GiB (gf2_launch_m4rm8q's and gf2_launch_a4_pack_rot's refusal) and 32-bit offset overflow inside one operand:
    engine.hip's launch_leaf chunks such products before a leaf sees them, tests/test_gpu_parity.py runs that path;
  * anything that needs more than a few hundred MiB -- the largest row here holds 17 MiB of slabs;
  * ug values other than the tuned default (LEAF_VARIANTS instantiates one per tile height), rot = 0 / 2 of the pack pass
    (tests/test_gpu_passes.py: test_a4_pack_kernel_alone);
  * which physical kernel ran: `reach` is what the launcher's dispatch selects for the row's arguments, read from the source; the rows do
    not trace kernel names.
"""
import os
import re
import subprocess
from collections import namedtuple

import numpy as np
import pytest
import torch

import leaf_lib as L
import leaf_reference as ref
import pass_reference as pref

# Measured wall time of `pytest tests/test_gpu_leaves.py -m gpu` on one MI355X (reported, not asserted).
WALL_TIME = "377 rows in 4.6 s of pytest, 6 s of wall with the interpreter's start (one run, one MI355X, 16 host threads)"

GUARD = 32            # words of poison before and after every buffer
POISON = np.uint64(0xFFFFFFFFFFFFFFFF)
CSRC = os.path.join(L.ROOT, "m4ri_amd", "csrc")

# gen: 1 / 4 / 5.  op: "leaf" (one launch; mode 2 is followed by the reduce pass; tc > 0: the tile range [tb, tb + tc)), "hybrid"
# (generation 4, the engine's plan: head [0, T - tc) unsplit, tail [T - tc, T) split ks ways through slabs (mode 2) or atomics (mode 1)),
# "zero" / "reduce" (the helper alone on the tiles [tb, tb + tc) of the generation's tile grid; reduce: ks host-made slabs per tile).
# init: what C holds before -- "poison", "random" (an accumulation: hybrid and mode 2 then add) or "zero".  pad / off / gap: words of row
# padding, of base offset and between batch members, for A, B and C alike.  bshare: b_bs = 0 with batch > 1.  bs0: batch 1 with all batch
# strides 0.  pack: generation 4's packed A from "numpy" or from the pack "kernel".  rc: the launcher's answer.
Row = namedtuple("Row", "gen op m l n batch ks mode rg init pad off gap bshare bs0 pack tb tc ug pipe nopart rc reach why")


def _b(x):
    return "true" if x else "false"


def _reach(gen, op, l, ks, mode, rg, init, nothing, rc):
    """The launchers' dispatch, written out: m4rm_leaf.hip LEAF_CASE, m4rm8q_leaf.hip and m4rm_small.hip's launchers, aux_kernels.hip."""
    if rc != 0:
        return "(refused)"
    if nothing:
        return "(nothing)"
    acc = init == "random"
    if op == "zero":
        return "zero_tiles_kernel"
    if op == "reduce":
        return f"reduce_partials_kernel<{_b(acc)}>"
    if op == "hybrid":
        head = f"m4rm8q_kernel<{_b(acc)}>"
        if mode == 2:
            return f"{head} + m4rm8q_kernel<false> + reduce_partials_kernel<{_b(acc)}>"
        return ("" if acc else "zero_tiles_kernel + ") + f"{head} + m4rm8q_kernel<true>"
    if gen == 1:
        return f"m4rm_leaf_kernel<{rg},4,{_b(mode != 0)}>"
    if gen == 4:
        return f"m4rm8q_kernel<{_b(mode == 1)}>" + (f" + reduce_partials_kernel<{_b(acc)}>" if mode == 2 else "")
    eff = len(ref.split_bounds(5, l, ks))
    return f"m4rm_small_kernel<{_b(mode != 0)},{_b(-(-ref.words_of(l) // eff) > 1)}>"


def _row(gen, m, l, n, why, *, op="leaf", batch=1, ks=1, mode=0, rg=32, init=None, pad=1, off=1, gap=3, bshare=False, bs0=False, pack="numpy",
         tb=0, tc=0, ug=0, pipe=0, nopart=False, rc=0, nothing=None):
    if init is None:
        init = "random" if mode == 1 else "poison"
    if nothing is None:
        nothing = m * n * batch == 0 or (l == 0 and gen != 1) or (op in ("zero", "reduce") and tc == 0)
    if bs0:
        gap = 0
    return Row(gen, op, m, l, n, batch, ks, mode, rg, init, pad, off, gap, bshare, bs0, pack, tb, tc, ug, pipe, nopart, rc,
               _reach(gen, op, l, ks, mode, rg, init, nothing, rc), why)


L_EDGES = [1, 15, 16, 17, 31, 32, 33, 48, 63, 64, 65, 127, 128, 129, 3001]   # 48: three 16-bit stages (an odd number); 3001: off the word grid


def _generation_rows(gen, rg, m_edges, n_edges, wide_n):
    """The sweeps every generation gets: each of m, l, n over its edges with the others fixed, the batches, the modes."""
    R = ref.tile_shape(gen, rg)[0]
    kw = dict(rg=rg)
    rows = []
    for m in m_edges:
        rows.append(_row(gen, m, 131, 257, f"m = {m} against the tile height {R}", **kw))
    rows.append(_row(gen, m_edges[-1], 131, 257, f"m = {m_edges[-1]}: two row tiles and a partial one, as an accumulation", mode=1, **kw))
    for l in L_EDGES:
        rows.append(_row(gen, 70, l, 130, f"l = {l}", **kw))
        if l in (1, 33, 64, 65, 3001):
            rows.append(_row(gen, 70, l, 130, f"l = {l}, onto random content", mode=1, **kw))
    for n in n_edges:
        rows.append(_row(gen, 40, 77, n, f"n = {n}", **kw))
    rows.append(_row(gen, 40, 77, wide_n, f"n = {wide_n}: a partial last column tile, onto random content", mode=1, **kw))
    # batches, gaps, strides
    rows.append(_row(gen, 33, 100, 200, "no padding, 16-byte bases, members back to back", batch=2, pad=0, off=0, gap=0, **kw))
    rows.append(_row(gen, 33, 100, 200, "batch 2, stride padded by 3 words", batch=2, pad=3, **kw))
    rows.append(_row(gen, R + 1, 100, wide_n, "batch 5 with gaps", batch=5, gap=7, **kw))
    rows.append(_row(gen, 33, 100, 200, "batch 5, one B shared by all members (b_bs = 0)", batch=5, bshare=True, mode=1, **kw))
    rows.append(_row(gen, R + 1, 100, 200, "batch 1 with all batch strides 0: what the engine passes", bs0=True, **kw))
    rows.append(_row(gen, R + 1, 100, 200, "batch 1 with all batch strides 0, accumulation", bs0=True, mode=1, **kw))
    # inner splits that meet by atomic XOR: onto a zeroed C and as an accumulation
    for init in ("zero", "random"):
        rows.append(_row(gen, R + 1, 300, wide_n, f"three splits by atomic XOR onto {init} content", batch=2, ks=3, mode=1, init=init, **kw))
        rows.append(_row(gen, 3, 3001, 65, f"16 splits by atomic XOR onto {init} content", ks=16, mode=1, init=init, **kw))
    rows.append(_row(gen, 70, 300, 130, "a request of 4 splits that the launcher rounds to 3", ks=4, mode=1, init="zero", **kw))
    return rows


# the shapes of tools/leaf_check.cpp's check() calls: (m, l, n, batch, ksplit, mode, pad)
_LEAF_CHECK = [(1024, 1024, 2048, 1, 1, 0, 0), (1000, 777, 1234, 1, 1, 0, 1), (1000, 777, 1234, 2, 1, 1, 3), (1, 1, 1, 1, 1, 0, 0), (3, 131, 257, 1, 1, 0, 0),
               (2100, 300, 4100, 2, 3, 1, 2), (64, 64, 64, 5, 1, 0, 0), (193, 65, 65, 1, 2, 1, 0)]
_LEAF_CHECK_V4 = [(5000, 1111, 700, 1, 1, 0, 1), (4096, 96, 512, 2, 1, 1, 0), (193, 65, 65, 1, 1, 0, 0), (2048, 512, 1024, 1, 1, 0, 0), (3000, 1000, 3000, 1, 1, 0, 1)]


def _leaf_check_rows(gen, rg, shapes):
    # check() lays the members out 3 / 5 / 7 words apart beyond their rows; one gap for all three operands here
    return [_row(gen, m, l, n, "tools/leaf_check.cpp check()", batch=batch, ks=ks, mode=mode, pad=pad, off=0, gap=5, rg=rg)
            for (m, l, n, batch, ks, mode, pad) in shapes]


def _gen1_rows():
    rows = []
    for rg in (32, 24, 16):
        R = 32 * rg
        rows += _generation_rows(1, rg, [1, 3, R - 1, R, R + 1, 2 * R + 77], [1, 63, 64, 65, 2047, 2048, 2049], 4100)
        rows += _leaf_check_rows(1, rg, _LEAF_CHECK)
        rows.append(_row(1, 5, 0, 70, "l = 0, mode 0: no stage runs and the epilogue stores the empty product, C = 0 (the engine never asks: it clears C itself)",
                         rg=rg, nothing=False))
        rows.append(_row(1, 5, 0, 70, "l = 0, mode 1: the epilogue XORs zeros, C keeps its content", rg=rg, mode=1, nothing=False))
        rows.append(_row(1, 70, 300, 130, "ksplit > 1 with mode 0", rg=rg, ks=3, rc=1))
    rows.append(_row(1, 70, 32, 130, "mode 0 with a request of 2 splits that rounds to 1 (two stages): taken", ks=2))
    rows.append(_row(1, 70, 300, 130, "rg = 8: no such instantiation", rg=8, rc=1))
    rows.append(_row(1, 70, 300, 130, "pipe = 1: the removed variants' selector", ug=4, pipe=1, rc=1))
    rows.append(_row(1, 70, 300, 130, "ug = 4 given explicitly through the variant launcher", ug=4))
    return rows


def _gen4_rows():
    rows = _generation_rows(4, 32, [1, 3, 4095, 4096, 4097, 8192 + 600], [1, 63, 64, 65, 511, 512, 513], 1100)
    rows += _leaf_check_rows(4, 32, _LEAF_CHECK + _LEAF_CHECK_V4)
    rows.append(_row(4, 4096 + 513, 200, 130, "last row tile of 513 rows: two of its waves gather, six (all four builders) own only padding rows"))
    rows.append(_row(4, 2100, 200, 130, "one row tile of 2100 rows: a builder wave with 52 rows, three builder waves of padding", mode=1))
    # through the pack pass: one row per shape class
    for (m, l, n, batch, ks, mode, why) in ((1, 1, 1, 1, 1, 0, "smallest"), (4097, 131, 513, 2, 1, 0, "two tiles each way, batch 2"), (70, 3001, 130, 1, 1, 1, "long inner dimension off the word grid"),
                                            (8192 + 600, 65, 65, 1, 1, 0, "two row tiles and a partial one"), (300, 300, 1100, 5, 3, 1, "batch 5, three splits by atomic XOR"),
                                            (4085, 2057, 139, 1, 5, 2, "slabs")):
        rows.append(_row(4, m, l, n, "packed by gf2_launch_a4_pack_rot(rot = 1): " + why, batch=batch, ks=ks, mode=mode, pack="kernel"))
    # mode 2: slabs + the reduce pass
    for init in ("poison", "random"):
        rows.append(_row(4, 4097, 300, 513, "slabs, three splits, four tiles a member", batch=2, ks=3, mode=2, init=init))
        rows.append(_row(4, 70, 3001, 130, "slabs, 16 splits of a long inner dimension", ks=16, mode=2, init=init))
        rows.append(_row(4, 70, 64, 130, "slabs with one split: one slab a tile", ks=1, mode=2, init=init))
        rows.append(_row(4, 33, 100, 200, "slabs, one B shared by 5 members", batch=5, ks=2, mode=2, init=init, bshare=True))
    # requested splits the launcher rounds: test_inner_dimension_splits_fold_to_the_same_bits' values on an eighth of its inner dimension
    # (33 words of A = 66 stages = 33 stage pairs); 64 is a request above the number of stage pairs
    for ks in (2, 3, 5, 7, 16, 32, 64):
        eff = len(ref.split_bounds(4, 2057, ks))
        rows.append(_row(4, 4085, 2057, 139, f"slabs, {ks} splits asked, {eff} used", ks=ks, mode=2, init="random" if ks % 2 else "poison"))
    rows.append(_row(4, 70, 2057, 139, "64 splits asked, 33 used, by atomic XOR", ks=64, mode=1, init="zero"))
    rows.append(_row(4, 70, 64, 130, "mode 0 with a request of 4 splits that rounds to 1 (one stage pair): taken", ks=4))
    # the engine's hybrid plan (launch_leaf_one): 8 tiles = 2 row tiles x 2 column tiles x 2 members; tails of 3 (crosses a tile_n
    # boundary; the head crosses the member boundary) and 5 (crosses the member boundary)
    for t in (3, 5):
        for mode in (2, 1):
            for init in ("poison", "random"):
                rows.append(_row(4, 4097, 300, 513, f"hybrid plan, tail of {t} tiles in three splits, {'slabs' if mode == 2 else 'atomics'}, {'add' if init == 'random' else 'no add'}",
                                 op="hybrid", batch=2, ks=3, mode=mode, init=init, tc=t))
    rows.append(_row(4, 4097, 300, 513, "hybrid plan, tail split 4 asked -> 3 used", op="hybrid", batch=2, ks=4, mode=2, tc=1))
    # a range strictly inside the grid, each kernel on its own: tiles 1 .. 6 of 8 cross a tile_n and the member boundary
    rows.append(_row(4, 4097, 300, 513, "tiles [1, 7) of 8, plain stores", batch=2, tb=1, tc=6))
    rows.append(_row(4, 4097, 300, 513, "tiles [1, 7) of 8, read-modify-write", batch=2, mode=1, tb=1, tc=6))
    rows.append(_row(4, 4097, 300, 513, "tiles [1, 7) of 8, atomics", batch=2, ks=3, mode=1, tb=1, tc=6))
    rows.append(_row(4, 4097, 300, 513, "tiles [1, 7) of 8, slabs and the reduce pass on the range", batch=2, ks=3, mode=2, tb=1, tc=6))
    rows.append(_row(4, 4097, 300, 513, "tile [3, 4) alone: the last tile of member 0", batch=2, tb=3, tc=1))
    for init in ("poison", "random"):
        rows.append(_row(4, 4097, 0, 513, "reduce pass alone on tiles [1, 7) of 8, three host-made slabs a tile", op="reduce", batch=2, ks=3, init=init, tb=1, tc=6))
        rows.append(_row(4, 4100, 0, 513, "reduce pass alone, one slab a tile, the whole grid", op="reduce", ks=1, init=init, tb=0, tc=4))
    rows.append(_row(4, 4097, 0, 513, "zero_tiles alone on tiles [1, 7) of 8", op="zero", batch=2, tb=1, tc=6))
    rows.append(_row(4, 4097, 0, 513, "zero_tiles alone on the whole grid", op="zero", batch=2, init="random", tb=0, tc=8))
    rows.append(_row(4, 4097, 0, 513, "zero_tiles with ntiles = 0", op="zero", batch=2, tb=2, tc=0))
    rows.append(_row(4, 4097, 0, 513, "reduce_partials with ntiles = 0", op="reduce", batch=2, ks=2, tb=2, tc=0))
    # the helpers on the other generations' tile shapes (the launchers take the geometry as arguments)
    rows.append(_row(1, 1025, 0, 2049, "zero_tiles on generation 1's tiles [1, 5) of 8", op="zero", batch=2, tb=1, tc=4))
    rows.append(_row(5, 300, 0, 1100, "zero_tiles on generation 5's tiles [2, 5) of 6", op="zero", tb=2, tc=3))
    # refusals
    rows.append(_row(4, 70, 300, 130, "ksplit > 1 with mode 0", ks=3, rc=1))
    rows.append(_row(4, 70, 300, 130, "mode 2 without Cpart", ks=3, mode=2, nopart=True, rc=1))
    rows.append(_row(4, 70, 300, 130, "mode 2 without Cpart, one split", ks=1, mode=2, nopart=True, rc=1))
    rows.append(_row(4, 4097, 300, 513, "tile_base < 0", batch=2, tb=-1, tc=2, rc=1))
    rows.append(_row(4, 4097, 300, 513, "tile_base + tile_count one beyond the grid", batch=2, tb=3, tc=6, rc=1))
    rows.append(_row(4, 4097, 300, 513, "tile_base beyond the grid", batch=2, mode=1, tb=8, tc=1, rc=1))
    return rows


def _gen5_rows():
    rows = _generation_rows(5, 32, [1, 3, 255, 256, 257, 512 + 77], [1, 63, 64, 65, 511, 512, 513], 1100)
    rows += _leaf_check_rows(5, 32, _LEAF_CHECK[1:])
    # PIPE = false: one step per workgroup, unsplit (l <= 64) or split down to single steps
    rows.append(_row(5, 257, 64, 513, "unsplit, one step: PIPE = false, plain stores"))
    rows.append(_row(5, 257, 64, 513, "unsplit, one step: PIPE = false, read-modify-write", mode=1))
    for init in ("zero", "random"):
        rows.append(_row(5, 257, 300, 513, "5 splits of one step each: PIPE = false, atomics", ks=5, mode=1, init=init, batch=2))
        rows.append(_row(5, 257, 300, 513, "99 splits asked, above wl = 5: capped to 5", ks=99, mode=1, init=init))
        rows.append(_row(5, 70, 3001, 130, "7 splits of 47 words: 7 steps each, the last split 5", ks=7, mode=1, init=init))
        rows.append(_row(5, 70, 3001, 130, "32 asked -> steps of 2 -> 24 used", ks=32, mode=1, init=init))
    rows.append(_row(5, 70, 64, 130, "mode 0 with a request of 2 splits, capped to wl = 1: taken", ks=2))
    rows.append(_row(5, 70, 300, 130, "ksplit > 1 with mode 0", ks=3, rc=1))
    return rows


def _zero_rows():
    rows = []
    for gen in (1, 4, 5):
        for (m, l, n, batch) in ((0, 100, 100, 2), (70, 100, 0, 2), (70, 100, 100, 0)) + (((70, 0, 100, 2),) if gen != 1 else ()):
            for mode in (0, 1):
                rows.append(_row(gen, m, l, n, "a dimension of 0: success, nothing launched", batch=batch, mode=mode))
    rows.append(_row(4, 70, 0, 100, "l = 0 in mode 2: success, nothing launched", mode=2, ks=2))
    return rows


ROWS = _gen1_rows() + _gen4_rows() + _gen5_rows() + _zero_rows()


def row_id(r: Row) -> str:
    flags = ("-bshare" if r.bshare else "") + ("-bs0" if r.bs0 else "") + ("-packk" if r.pack == "kernel" else "") + ("-nopart" if r.nopart else "")
    flags += (f"-ug{r.ug}pipe{r.pipe}" if r.ug or r.pipe else "") + (f"-t{r.tb}+{r.tc}" if r.tc or r.tb or r.op != "leaf" else "")
    return f"g{r.gen}rg{r.rg}-{r.op}-m{r.m}-l{r.l}-n{r.n}-b{r.batch}-ks{r.ks}-mode{r.mode}-{r.init}-pad{r.pad}-o{r.off}-gap{r.gap}{flags}"


def _what(r: Row) -> str:
    return f"generation {r.gen}, {r.op}, reach {r.reach}; row {row_id(r)} ({r.why})"


# ---- the table against the sources -------------------------------------------------------------------------------------------------------
def instantiations_in_sources():
    """Every kernel instantiation the launchers of the four sources can start, read from their launch statements."""
    tf = ("true", "false")
    out = set()
    text = open(os.path.join(CSRC, "m4rm_leaf.hip")).read()
    variants = re.findall(r"X\((\d+),\s*(\d+)\)", re.search(r"#define LEAF_VARIANTS\(X\)(.*)", text).group(1))
    launched = set(re.findall(r"hipLaunchKernelGGL\(\(m4rm_leaf_kernel<RGV, UGV, (true|false)>\)", text))
    assert variants and launched == set(tf)
    out |= {f"m4rm_leaf_kernel<{rg},{ug},{b}>" for (rg, ug) in variants for b in tf}
    for src, names in (("m4rm8q_leaf.hip", ("m4rm8q_kernel",)), ("m4rm_small.hip", ("m4rm_small_kernel",)),
                       ("aux_kernels.hip", ("reduce_partials_kernel", "zero_tiles_kernel"))):
        text = open(os.path.join(CSRC, src)).read()
        found = set()
        for name, targs in re.findall(r"hipLaunchKernelGGL\(\(?\s*(\w+)\s*(<[^>]*>)?", text):
            if name in names:
                found.add(name + targs.replace(" ", ""))
        assert {f.split("<")[0] for f in found} == set(names), (src, found)
        out |= found
    return out


def kernels_named():
    names = set()
    for r in ROWS:
        for k in r.reach.split(" + "):
            if not k.startswith("("):
                names.add(k)
    return names


def test_the_table_names_every_instantiation():
    """No GPU needed: the table names every instantiation of a leaf kernel and of the two helpers that the sources launch, and nothing else."""
    want = instantiations_in_sources()
    assert len(want) == 15, sorted(want)
    assert kernels_named() == want, sorted(kernels_named() ^ want)
    ids = [row_id(r) for r in ROWS]
    assert len(ids) == len(set(ids)), sorted(i for i in ids if ids.count(i) > 1)
    for r in ROWS:
        assert r.why and (r.rc in (0, 1))


def test_the_leaf_library_exports_what_the_binding_binds():
    """No GPU needed: m4ri_amd/build.py links the test-only library with exactly the names tests/leaf_lib.py binds (the product library's
    own export list is pinned by test_cabi.py and does not hold them)."""
    from m4ri_amd import build
    build.build(verbose=False)
    out = subprocess.run(["nm", "-D", "--defined-only", L.PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert exported == set(L._SIGNATURES) == set(build.LEAF_EXPORTS), sorted(exported ^ set(L._SIGNATURES))
    assert L.PATH == build.LEAF_LIB
    assert L.a4_words(5, 65, 3) == 3 * 8 * 4 // 2


def test_small_ksplit_is_a_fixed_point_of_the_launchers_rounding():
    """gf2_m4rm_small_ksplit is host arithmetic (no GPU needed): over a grid of (tiles, wl, cus, c_words) the split lies in
    [1, min(wl, 256)], the launcher's rounding ceil(wl / ceil(wl / ks)) leaves it alone, and it is 1 for wl < 2."""
    for tiles in (0, 1, 2, 7, 64, 255, 256, 257, 1000, 100000):
        for wl in (0, 1, 2, 3, 5, 8, 33, 64, 100, 255, 256, 257, 1000, 5000):
            for cus in (0, 1, 8, 64, 256, 304):
                for c_words in (1, 1000, 1 << 20, 1 << 28):
                    ks = L.m4rm_small_ksplit(tiles, wl, cus, c_words)
                    what = f"gf2_m4rm_small_ksplit({tiles}, {wl}, {cus}, {c_words}) = {ks}"
                    assert 1 <= ks <= max(1, min(wl, 256)), what
                    if wl < 2 or tiles <= 0:
                        assert ks == 1, what
                    else:
                        assert -(-wl // -(-wl // ks)) == ks, what + ": the launcher would round it"
                        assert len(ref.split_bounds(5, 64 * wl, ks)) == ks, what


def test_effective_ksplit_is_the_references_split_count():
    """gf2_m4rm8q_effective_ksplit (host arithmetic, no GPU needed) against the documented rule, stated in leaf_reference.split_bounds."""
    for l in (1, 63, 64, 65, 128, 129, 300, 2057, 3001, 16453, 65536):
        for ks in (-1, 0, 1, 2, 3, 4, 5, 7, 16, 29, 32, 33, 64, 1000):
            assert L.m4rm8q_effective_ksplit(l, ks) == len(ref.split_bounds(4, l, ks)), (l, ks)
    assert L.m4rm8q_effective_ksplit(16453, 32) == 29    # the figure tests/test_gpu_parity.py quotes
    assert L.m4rm8q_effective_ksplit(0, 3) == 0          # no stage, no split: at l = 0 the launcher starts nothing


# ---- running a row ----------------------------------------------------------------------------------------------------------------------------
def _dev(buf: np.ndarray) -> torch.Tensor:
    return torch.from_numpy(buf.view(np.int64)).cuda()


def _host(t: torch.Tensor) -> np.ndarray:
    return t.cpu().numpy().view(np.uint64)


def _operand(rng, r: Row, members, rows, words, fill):
    """`members` matrices of rows x words inside a poisoned buffer (guards, base offset, row padding, gaps), filled as asked."""
    op = pref.make_operand(rng, members, rows, words, off=r.off, stride_pad=r.pad, gap=r.gap, zero_bs=r.bs0, fill="poison", guard=GUARD)
    if fill == "random":
        op.view()[...] = rng.integers(0, 1 << 64, size=(members, rows, words), dtype=np.uint64)
    elif fill == "zero":
        op.view()[...] = 0
    return op


def _first_difference(r: Row, got, want, rows_t, tw, parts=None, bounds=None) -> str:
    """got / want: (batch, m, wn).  The first differing word by member, tile, row and word; for a split row, the split whose partial product
    (inside that tile) equals the difference."""
    bad = np.argwhere(got != want)
    b, row, w = (int(x) for x in bad[0])
    tm, tn = row // rows_t, w // tw
    msg = (f"{_what(r)}: {len(bad)} of {got.size} words of C differ; first: batch member {b}, tile (tile_m {tm}, tile_n {tn}), row {row} (row {row % rows_t} of the tile), "
           f"word {w} (word {w % tw} of the tile): got {int(got[b, row, w]):#018x}, want {int(want[b, row, w]):#018x}")
    tiles = sorted({(int(x[0]), int(x[1]) // rows_t, int(x[2]) // tw) for x in bad[:100000]})
    msg += f"; (member, tile_m, tile_n) that differ: {tiles[:8]}{' ...' if len(tiles) > 8 else ''}"
    if parts is not None and len(parts[b]) > 1:
        sl = (slice(tm * rows_t, (tm + 1) * rows_t), slice(tn * tw, (tn + 1) * tw))
        d = got[b][sl] ^ want[b][sl]
        hits = [k for k, p in enumerate(parts[b]) if np.array_equal(d, p[sl])]
        msg += (f"; inside that tile got ^ want is exactly the partial product of split {hits[0]} (inner bits {bounds[hits[0]][0]} .. {bounds[hits[0]][1]}): that split is missing or counted twice"
                if hits else f"; no single one of the {len(parts[b])} splits' partial products equals got ^ want inside that tile")
    return msg


def _compare_c(r: Row, C, got_buf, want_v, rows_t, tw, parts=None, bounds=None):
    """The whole buffer of C: the frame first (everything outside the members' own words keeps its poison), then the words."""
    m_, wn = want_v.shape[1], want_v.shape[2]
    mask = C.written_mask()
    out = np.flatnonzero((got_buf != POISON) & ~mask)
    assert out.size == 0, (f"{_what(r)}: {out.size} words outside C (row padding, the gaps between members, the guards) lost their poison, first at word "
                           f"{int(out[0]) - C.off} relative to the base (stride {C.stride}, bs {C.bs}, {m_} rows of {wn} words)")
    got_v = pref.Operand(got_buf, C.off, C.stride, C.bs, C.nparents, C.rows, C.words).view()
    assert np.array_equal(got_v, want_v), _first_difference(r, got_v, want_v, rows_t, tw, parts, bounds)


def _check_slabs(r: Row, got, base, nslabs_alloc, tiles, eff, parts, bounds, tiles_m, tiles_n, tb):
    """The slab buffer after a mode-2 launch over `tiles` tiles from tile tb: guards and the slabs from tiles x eff on are poison; slab
    j * eff + k holds the dense image of split k's partial of tile tb + j in the tile's valid rows and words."""
    S = ref.SLAB_WORDS
    for name, part in (("before", got[:base]), ("after", got[base + nslabs_alloc * S:])):
        bad = np.flatnonzero(part != POISON)
        assert bad.size == 0, f"{_what(r)}: {bad.size} guard words {name} the slab buffer were written"
    used = tiles * eff
    rest = got[base + used * S:base + nslabs_alloc * S]
    bad = np.flatnonzero(rest != POISON)
    assert bad.size == 0, (f"{_what(r)}: {tiles} tiles x {eff} splits (gf2_m4rm8q_effective_ksplit) = {used} slabs, yet slab {used + int(bad[0]) // S} was written "
                           f"(first at its word {int(bad[0]) % S})")
    for j in range(tiles):
        b, tn, tm = ref.tile_of(tb + j, tiles_m, tiles_n)
        for k in range(eff):
            slab = got[base + (j * eff + k) * S:base + (j * eff + k + 1) * S].reshape(ref.G4_ROWS, ref.G4_TW)
            img, valid = ref.slab_image(parts[b][k], tm, tn)
            assert not (slab[valid] == POISON).all() or (img[valid] == POISON).all(), \
                f"{_what(r)}: slab {j * eff + k} (tile {tb + j} = member {b}, tile_m {tm}, tile_n {tn}; split {k}) was not written"
            if not np.array_equal(slab[valid], img[valid]):
                bad = np.argwhere((slab != img) & valid)
                row, w = (int(x) for x in bad[0])
                raise AssertionError(f"{_what(r)}: slab {j * eff + k} (tile {tb + j} = member {b}, tile_m {tm}, tile_n {tn}; split {k}, inner bits {bounds[k][0]} .. {bounds[k][1]}): "
                                     f"{len(bad)} valid words differ from the split's partial product, first at row {row}, word {w}: got {int(slab[row, w]):#018x}, want {int(img[row, w]):#018x}")


def run_row(r: Row):
    """Launch what the row says, return the launcher's answer, and check everything that answer promises."""
    rng = np.random.default_rng(sum(map(ord, row_id(r))))
    rows_t, tw = ref.tile_shape(r.gen, r.rg if r.rg in (16, 24, 32) else 32)
    m_, l_, n_, batch_ = max(r.m, 1), max(r.l, 1), max(r.n, 1), max(r.batch, 1)     # the allocation; the launcher is given the zeros
    wl, wn = ref.words_of(l_), ref.words_of(n_)
    tiles_m, tiles_n = ref.tile_grid(m_, wn, rows_t, tw)
    T = tiles_m * tiles_n * batch_
    nothing = r.m * r.n * r.batch == 0 or (r.l == 0 and r.gen != 1 and r.op in ("leaf", "hybrid"))
    A = _operand(rng, r, batch_, m_, wl, "random")                                    # whole random words: junk from column l on
    B = _operand(rng, r, 1 if r.bshare else batch_, l_, wn, "random")
    C = _operand(rng, r, batch_, m_, wn, r.init)
    dA, dB, dC = _dev(A.buf), _dev(B.buf), _dev(C.buf)
    pA, pB, pC = dA.data_ptr() + 8 * A.off, dB.data_ptr() + 8 * B.off, dC.data_ptr() + 8 * C.off
    b_bs = 0 if r.bshare else B.bs
    Av, Bv, C0 = A.view(), B.view(), C.view().copy()
    Bof = (lambda b: Bv[0]) if r.bshare else (lambda b: Bv[b])
    bounds = ref.split_bounds(r.gen, r.l, r.ks) if r.op in ("leaf", "hybrid") else [(0, r.l)]
    eff = len(bounds)

    # generation 4: the packed A and the slab buffer
    a4 = a4_host = None
    p4 = None
    if r.gen == 4 and r.op in ("leaf", "hybrid"):
        m_pad = (m_ + 3) & ~3
        words4 = (batch_ * m_pad * 2 * wl + 1) // 2
        if not nothing:
            assert L.a4_words(r.m, r.l, r.batch) == words4
        a4_host = np.full(GUARD + words4 + GUARD, POISON, dtype=np.uint64)
        if r.pack == "numpy":
            packed = ref.pack_a4(Av, 1, m_pad).reshape(-1)
            a4_host[GUARD:GUARD + words4].view("<u4")[:packed.size] = packed
        a4 = _dev(a4_host)
        p4 = a4.data_ptr() + 8 * GUARD
    slabs = part_host = None
    pP = None
    nslabs = 0
    if r.gen == 4 and (r.mode == 2 or r.op in ("hybrid", "reduce")):
        span = r.tc if (r.tc or r.op != "leaf") else T
        nslabs = max(span, 1) * max(r.ks, 1) + 2
        base = GUARD + r.off
        if r.op == "reduce":
            part_host = rng.integers(0, 1 << 64, size=base + nslabs * ref.SLAB_WORDS + GUARD, dtype=np.uint64)
        else:
            part_host = np.full(base + nslabs * ref.SLAB_WORDS + GUARD, POISON, dtype=np.uint64)
        slabs = _dev(part_host)
        pP = slabs.data_ptr() + 8 * base

    def args(**kw):
        return L.leaf_args(pA, A.stride, A.bs, pB, B.stride, b_bs, pC, C.stride, C.bs, r.m, r.l, r.n, r.batch, **kw)

    def launch(a):
        if r.gen == 1:
            return L.m4rm_leaf_variant(a, r.rg, r.ug, r.pipe) if (r.ug or r.pipe) else L.m4rm_leaf(a, r.rg)
        return L.m4rm8q(a, p4) if r.gen == 4 else L.m4rm_small(a)

    parts = None
    if not nothing and r.rc == 0 and r.op in ("leaf", "hybrid"):
        parts = [ref.partials(Av[b], Bof(b), r.l, bounds) for b in range(batch_)]

    def slab_check(tiles, tb):
        nonlocal checked_slabs
        checked_slabs = (tiles, tb)
        torch.cuda.synchronize()
        _check_slabs(r, _host(slabs), GUARD + r.off, nslabs, tiles, eff, parts, bounds, tiles_m, tiles_n, tb)

    geometry = (C.stride, C.bs, r.m, wn, rows_t, tw, tiles_m, tiles_n)
    rc = 0
    checked_slabs = None
    if r.rc == 0 and not nothing:   # (a typing error in the table must not become a launch beyond the grid)
        assert 0 <= r.tb and r.tb + r.tc <= T, f"{_what(r)}: the table's tile range leaves the grid of {T} tiles"
    if r.op in ("leaf", "hybrid") and r.gen == 4 and r.l > 0:
        assert L.m4rm8q_effective_ksplit(r.l, r.ks) == eff, f"{_what(r)}: gf2_m4rm8q_effective_ksplit({r.l}, {r.ks}) = {L.m4rm8q_effective_ksplit(r.l, r.ks)}, the documented rule gives {eff}"
        if r.pack == "kernel" and not nothing and r.rc == 0:
            rc4 = L.a4_pack_rot(args(), p4, 1)
            torch.cuda.synchronize()
            assert rc4 == 0, f"{_what(r)}: gf2_launch_a4_pack_rot returned HIP error {rc4}"
            masked = Av.copy()
            if r.l % 64:
                masked[:, :, -1] &= np.uint64((1 << (r.l % 64)) - 1)
            packed = ref.pack_a4(masked, 1, (m_ + 3) & ~3).reshape(-1)
            a4_host[GUARD:GUARD + packed.size // 2].view("<u4")[:] = packed      # (an even number of dwords: two per word of A)
            g4 = _host(a4)
            bad = np.flatnonzero(g4 != a4_host)
            assert bad.size == 0, f"{_what(r)}: the pack pass's output differs from pass_reference.pack_a4 in {bad.size} words (guards included), first at word {int(bad[0]) - GUARD}"
    if r.op == "leaf":
        rc = launch(args(ksplit=r.ks, mode=r.mode, tile_base=r.tb, tile_count=r.tc, Cpart=None if (r.nopart or pP is None) else pP))
        if rc == 0 and r.mode == 2 and not nothing:
            span, tb = (r.tc, r.tb) if r.tc else (T, 0)
            slab_check(span, tb)
            rc2 = L.reduce_partials(r.init == "random", pC, *geometry, tb, span, eff, pP)
            assert rc2 == 0, f"{_what(r)}: gf2_launch_reduce_partials returned HIP error {rc2}"
    elif r.op == "hybrid":
        add, use_slabs, t = r.init == "random", r.mode == 2, r.tc
        assert 0 < t < T
        head = args(ksplit=1, mode=1 if add else 0, tile_base=0, tile_count=T - t, Cpart=pP)
        tail = args(ksplit=eff, mode=2 if use_slabs else 1, tile_base=T - t, tile_count=t, Cpart=pP)
        steps = []
        if not add and not use_slabs:
            steps.append(L.zero_tiles(pC, *geometry, T - t, t))
        steps += [launch(head), launch(tail)]
        if use_slabs and not any(steps):
            slab_check(t, T - t)
            steps.append(L.reduce_partials(add, pC, *geometry, T - t, t, eff, pP))
        rc = next((s for s in steps if s), 0)
    elif r.op == "zero":
        rc = L.zero_tiles(pC, *geometry, r.tb, r.tc)
    elif r.op == "reduce":
        rc = L.reduce_partials(r.init == "random", pC, *geometry, r.tb, r.tc, r.ks, pP)
    torch.cuda.synchronize()
    assert rc in (L.HIP_SUCCESS, L.HIP_INVALID_VALUE), f"{_what(r)}: the launcher returned HIP error {rc}"

    # the operands are unchanged
    assert np.array_equal(_host(dA), A.buf), f"{_what(r)}: A was written"
    assert np.array_equal(_host(dB), B.buf), f"{_what(r)}: B was written"
    if a4 is not None:
        assert np.array_equal(_host(a4), a4_host), f"{_what(r)}: the packed A (or the guards around it) was written"
    got = _host(dC)
    if rc != 0 or nothing:
        bad = np.flatnonzero(got != C.buf)
        assert bad.size == 0, f"{_what(r)}: answer {rc}, yet {bad.size} words of C's buffer changed, first at word {int(bad[0]) - C.off} relative to the base"
        if slabs is not None:
            bad = np.flatnonzero(_host(slabs) != part_host)
            assert bad.size == 0, f"{_what(r)}: answer {rc}, yet {bad.size} words of the slab buffer changed"
        return rc

    if checked_slabs is not None:      # the reduce pass only reads them
        _check_slabs(r, _host(slabs), GUARD + r.off, nslabs, checked_slabs[0], eff, parts, bounds, tiles_m, tiles_n, checked_slabs[1])
    elif slabs is not None and r.op != "reduce":
        assert np.array_equal(_host(slabs), part_host), f"{_what(r)}: no launch of this row writes slabs, yet the slab buffer changed"

    # what C must hold
    want = C0.copy()
    if r.op in ("leaf", "hybrid"):
        P = np.stack([np.bitwise_xor.reduce(np.stack(parts[b]), axis=0) for b in range(batch_)])
        accumulate = (r.mode == 1) if r.op == "leaf" and r.mode != 2 else r.init == "random"
        span, tb = (r.tc, r.tb) if (r.op == "leaf" and r.tc) else (T, 0)
        mask = ref.range_mask(m_, wn, batch_, rows_t, tw, tb, span)
        want[mask] = ((C0 ^ P) if accumulate else P)[mask]
    elif r.op == "zero":
        want[ref.range_mask(m_, wn, batch_, rows_t, tw, r.tb, r.tc)] = 0
    else:
        assert np.array_equal(_host(slabs), part_host), f"{_what(r)}: the reduce pass wrote its slabs"
        S, base = ref.SLAB_WORDS, GUARD + r.off
        for j in range(r.tc):
            b, tn, tm = ref.tile_of(r.tb + j, tiles_m, tiles_n)
            r0, r1, w0, w1 = ref.tile_extent(tm, tn, m_, wn, rows_t, tw)
            x = np.zeros((r1 - r0, w1 - w0), dtype=np.uint64)
            for k in range(r.ks):
                x ^= part_host[base + (j * r.ks + k) * S:base + (j * r.ks + k + 1) * S].reshape(rows_t, tw)[:r1 - r0, :w1 - w0]
            want[b, r0:r1, w0:w1] = (C0[b, r0:r1, w0:w1] ^ x) if r.init == "random" else x
    _compare_c(r, C, got, want, rows_t, tw, parts if r.op in ("leaf", "hybrid") else None, bounds)
    return rc


gpu = pytest.mark.gpu


@gpu
@pytest.mark.parametrize("r", ROWS, ids=row_id)
def test_leaf_matches_reference(r):
    rc = run_row(r)
    assert rc == r.rc, f"{_what(r)}: the launcher answered {rc}, the table says {r.rc}"
