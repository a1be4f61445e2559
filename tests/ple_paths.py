"""Inputs that steer the PLE's pivot searches (m4ri_amd/csrc/ple.hip) down every one of their paths, and a predictor that says --
from a decomposition's P and Q alone -- which paths a matrix takes.  Plain NumPy; the tests that use it are
tests/test_ple_paths_cpu.py (the predictor on the oracle's results: every path is reached by some case) and
tests/test_gpu_ple_paths.py (the kernels on the same cases, against the oracle).

Which code runs for a 64-column block depends on how far below the rank position each pivot lies:

  * the one-wave search (ple_pivots_wave_kernel) keeps the first 128 remaining rows in registers: positions 0..63 in the low
    slot of a lane, 64..127 in the high slot.  A column in which none of them has a pivot is passed over ("deferred") when more
    rows lie beyond; ple_verify_kernel then looks at those rows, and either confirms the block (ple_commit_stage_kernel, the
    second launch of permute / finish / update) or reports a miss, and the general search redoes the block;
  * the general search (ple_pivots_kernel) watches a window of 1024 rows that moves down by one per pivot: rows that were in it
    from the start are up to date, rows that entered later are stale until a catch-up pass; rows beyond the window are scanned
    in chunks of 1024, from the kernel's copy of the first 1088 rows (s_head) or from the dense slice in global memory.

Random, low-rank and sparse inputs have their pivots a few rows below the rank position.  A "shelf" -- the top D rows emptied in a
run of columns -- puts every pivot of those columns about D rows down (the emptied rows keep their data elsewhere, travel through
the swaps and become ordinary pivots later).
"""
from __future__ import annotations

from collections import namedtuple

import numpy as np

from m4ri_amd.mzd import Mzd

WINDOW = 1024        # ple.hip: SLICE_THREADS, the lanes of the general search
HEAD = WINDOW + 64   # rows the general search keeps in LDS (s_head)
WAVE_ROWS = 128      # rows the one-wave search holds

CLASSES = ("wave_lo", "wave_hi", "deferred_confirmed", "deferred_empty", "missed", "window", "stale", "far_head", "far_global",
           "far_chunk2", "missed_then_wave", "wave_then_missed")
GENERAL_CLASSES = ("window", "stale", "far_head", "far_global", "far_chunk2")


def clear(words: np.ndarray, D: int, c0: int, c1: int) -> None:
    """Zero rows [0, D) in columns [c0, c1) of a matrix given as its (rows x width) word view."""
    for w in range(c0 // 64, (c1 + 63) // 64):
        lo, hi = max(c0, 64 * w) - 64 * w, min(c1, 64 * w + 64) - 64 * w
        mask = (((1 << hi) - 1) ^ ((1 << lo) - 1)) & 0xFFFFFFFFFFFFFFFF
        words[:D, w] &= np.uint64(mask ^ 0xFFFFFFFFFFFFFFFF)


def shelf(m: int, n: int, steps, seed: int, below_rank: int = 0) -> Mzd:
    """Mzd.random(m, n, seed) with rows [0, D) cleared in columns [c0, c1) for every (D, c0, c1) of `steps`; a step
    (D, c0, c1, top) clears rows [top, D) only.  below_rank > 0: the rows from the first step's D on are replaced by a random
    matrix of that rank first."""
    A = Mzd.random(m, n, seed)
    if below_rank:
        D = steps[0][0]
        X = Mzd.random(m - D, below_rank, seed + 1).to_bits().astype(np.int64)
        Y = Mzd.random(below_rank, n, seed + 2).to_bits().astype(np.int64)
        A.valid_words()[D:, :] = Mzd.from_bits(((X @ Y) & 1).astype(np.uint8)).valid_words()
    w = A.valid_words()
    for D, c0, c1, *top in steps:
        top = top[0] if top else 0
        clear(w[top:], min(D, m) - top, c0, min(c1, n))
    return A


def blocks(P, Q, rank: int, m: int, n: int):
    """The 64-column blocks the driver visits (ple_blocks: left to right while rows remain), as (r0, columns in the block,
    [(t, pos), ...]): r0 = pivots found before the block, and for the block's t-th pivot pos = the position below r0 its row
    was found at.  A block without a pivot leaves no trace in P and Q but the gap in Q // 64."""
    out, i = [], 0
    for wb in range((n + 63) // 64):
        r0 = i
        if r0 >= m:
            break
        piv = []
        while i < rank and int(Q[i]) // 64 == wb:
            piv.append((i - r0, int(P[i]) - r0))
            i += 1
        out.append((r0, min(64, n - 64 * wb), piv))
    assert i == rank, "Q's first `rank` entries are not ascending pivot columns"
    return out


def classify(P, Q, rank: int, m: int, n: int, wave: bool = True) -> set:
    """The classes of CLASSES that occur in a decomposition with these P, Q and rank -- the kernels' own conditions restated.
    wave=False: the library run with the one-wave search switched off (every block goes to the general search)."""
    got, prev = set(), None
    for r0, ncb, piv in blocks(P, Q, rank, m, n):
        nleft = m - r0
        beyond = nleft > WAVE_ROWS and any(pos >= WAVE_ROWS for _, pos in piv)
        if wave and not beyond:  # the one-wave search's result stands
            kind = "wave"
            for _, pos in piv:
                got.add("wave_lo" if pos < 64 else "wave_hi")
            if nleft > WAVE_ROWS and len(piv) < min(ncb, nleft):  # a column was passed over with rows lying beyond
                got.add("deferred_confirmed" if piv else "deferred_empty")
        else:
            kind = "missed"
            if wave:
                got.add("missed")
            for t, pos in piv:
                if pos - t < WINDOW:
                    got.add("window" if pos < WINDOW else "stale")
                else:
                    got.add("far_head" if pos < HEAD else "far_global")
                    if pos - t >= 2 * WINDOW:
                        got.add("far_chunk2")
        if wave and prev is not None and prev != kind:
            got.add(prev + "_then_" + kind)
        prev = kind
    return got


Case = namedtuple("Case", "name m n steps below_rank", defaults=(0,))

CASES = [
    Case("hi_slot", 300, 300, [(66, 0, 48), (130, 64, 100)]),    # 48, then 36 pivots at positions 64..127: the one-wave search's high slot
    Case("hi_slot_then_beyond", 300, 300, [(70, 0, 192)]),       # ... starting there and running past 128 within each block: misses
    Case("just_beyond_the_wave", 400, 320, [(130, 0, 192)]),     # ... at 128 and a little more: every shelf block is a miss
    Case("window_then_stale", 1300, 320, [(1000, 0, 192)]),      # inside the first window, then in lanes that entered later
    Case("window_edge", 1400, 300, [(1030, 0, 192)]),            # on both sides of the window's end, rows 1024..1087 from s_head
    Case("beyond_head", 1500, 320, [(1100, 0, 192)]),            # beyond the window and beyond s_head: from the dense slice
    Case("second_chunk", 2500, 320, [(2100, 0, 192)]),           # the far scan's second chunk of 1024
    Case("fourth_chunk", 3400, 200, [(3100, 0, 128)]),           # ... and its fourth
    Case("alternating", 1500, 384, [(200, 64, 128), (1100, 192, 256)]),  # wave, miss, wave, miss, wave, wave
    Case("ragged_last_block", 500, 230, [(200, 0, 230)]),        # the shelf runs to n: the last block has 38 columns and is a miss
    Case("rows_129", 129, 200, [(128, 0, 128)]),                 # one row beyond the wave: it holds the only pivot, then 128 rows are left
    Case("rows_1025", 1025, 200, [(1024, 0, 128)]),              # one row beyond the window
    Case("rows_1089", 1089, 200, [(1088, 0, 128)]),              # one row beyond s_head
    Case("lowrank_below", 500, 256, [(150, 0, 64)], 20),         # rank 20 below the shelf: a miss, full blocks, then confirmed deferrals
    # The rows a shelf's pivots displace are shelf rows themselves, empty in the block, so where the searches keep them is never looked
    # at again within the block.  A step: row 0 is empty in column 0 only, the rows below it in the whole block.  The pivot of column 0
    # comes from D rows down and sends row 0 there -- and row 0 is the next pivot, found where the search put it: in a high slot of the
    # one-wave search, in the general search's copy of rows 1024..1087 (s_head), in its dense slice beyond.
    Case("displaced_row_in_hi_slot", 300, 200, [(70, 0, 1), (100, 1, 16, 1)]),   # (16 columns: the block stays within 128 rows)
    Case("displaced_row_in_head", 1400, 200, [(1030, 0, 1), (1045, 1, 64, 1)]),
    Case("displaced_row_in_slice", 1500, 200, [(1100, 0, 1), (1115, 1, 64, 1)]),
]

# both searches (a 130-row shelf on the first block), then rank updates over a wide trailing matrix: 68 words = two column tiles of
# 64 words, the second partial, odd word count; 18 words = a partial tile of 32 and a partial second tile of 16
WIDE_CASES = [
    Case("wide_68_words", 700, 4293, [(130, 0, 64)]),
    Case("wide_18_words", 300, 1100, [(130, 0, 64)]),
]


def make(case: Case) -> Mzd:
    return shelf(case.m, case.n, case.steps, 4000 + 3 * case.m + case.n, case.below_rank)


_expected = {}


def expected(oracle, case: Case):
    """(A, {flavour: ((rank, P, Q), decomposed matrix)}) by the oracle, computed once per case and shared: callers copy A and
    leave everything here as it is.  Flavours: "flat" (_mzd_ple_russian), "ple" (mzd_ple / _mzd_ple), "pluq" (mzd_pluq)."""
    if case.name not in _expected:
        A, want = make(case), {}
        for flavour, kw in (("flat", {}), ("ple", {"recursive": True}), ("pluq", {"pluq": True, "recursive": True})):
            Ao = A.copy()
            want[flavour] = (oracle.ple(Ao, **kw), Ao)
        _expected[case.name] = (A, want)
    return _expected[case.name]
