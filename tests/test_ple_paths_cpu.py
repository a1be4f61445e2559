"""The shelf inputs of tests/ple_paths.py on the CPU: the oracle's decomposition of every case says which paths of the PLE's pivot
searches (m4ri_amd/csrc/ple.hip) the case takes, and together the cases take all of them -- the condition that keeps
tests/test_gpu_ple_paths.py from silently not reaching a path.  It rests on the oracle alone, never on the code under test; the
oracle itself is pinned to the reference on the same cases."""
import numpy as np
import pytest

from ple_paths import CASES, CLASSES, GENERAL_CLASSES, WIDE_CASES, classify, expected

# what each case is there for: the classes it must show (by the oracle), so that a change to a case that loses its point is noticed
# even where another case still provides the class
PURPOSE = {
    "hi_slot": {"wave_hi", "wave_lo"},
    "hi_slot_then_beyond": {"missed", "window", "missed_then_wave"},
    "just_beyond_the_wave": {"missed", "window"},
    "window_then_stale": {"window", "stale"},
    "window_edge": {"stale", "far_head", "far_global"},
    "beyond_head": {"far_global"},
    "second_chunk": {"far_global", "far_chunk2"},
    "fourth_chunk": {"far_chunk2"},
    "alternating": {"wave_then_missed", "missed_then_wave"},
    "ragged_last_block": {"missed", "window"},
    "rows_129": {"missed", "window"},
    "rows_1025": {"far_head", "deferred_empty"},
    "rows_1089": {"far_global", "deferred_empty"},
    "lowrank_below": {"missed", "deferred_confirmed"},
    "displaced_row_in_hi_slot": {"wave_hi"},
    "displaced_row_in_head": {"far_head"},
    "displaced_row_in_slice": {"far_global"},
}


def _classes(oracle, case, flavour, wave=True):
    (rank, P, Q), _ = expected(oracle, case)[1][flavour]
    return classify(P, Q, rank, case.m, case.n, wave=wave)


def test_every_class_is_covered(oracle):
    reached = set()
    for case in CASES:
        got = _classes(oracle, case, "flat")
        assert PURPOSE[case.name] <= got, (case.name, sorted(PURPOSE[case.name] - got))
        reached |= got
    assert reached == set(CLASSES), sorted(set(CLASSES) - reached)
    # with the one-wave search switched off every pivot goes through the general search
    general = set().union(*(_classes(oracle, case, "flat", wave=False) for case in CASES))
    assert general == set(GENERAL_CLASSES), sorted(set(GENERAL_CLASSES) - general)


def test_every_class_is_covered_by_the_other_flavours(oracle):
    """mzd_ple and mzd_pluq on the same cases: the same pivots, so the same paths."""
    for flavour in ("ple", "pluq"):
        reached = set().union(*(_classes(oracle, case, flavour) for case in CASES))
        assert reached == set(CLASSES), (flavour, sorted(set(CLASSES) - reached))


def test_lowrank_below_has_both_outcomes_of_a_deferral(oracle):
    case = next(c for c in CASES if c.name == "lowrank_below")
    assert {"deferred_confirmed", "missed"} <= _classes(oracle, case, "flat")


def test_wide_cases_run_both_searches(oracle):
    for case in WIDE_CASES:
        assert {"missed", "missed_then_wave", "wave_lo"} <= _classes(oracle, case, "flat"), case.name


@pytest.mark.parametrize("case", CASES + WIDE_CASES, ids=lambda c: c.name)
def test_oracle_matches_reference(oracle, reference, case):
    """_mzd_ple_russian and mzd_pluq of the real library on the shelf family: matrix, P, Q and rank."""
    A, want = expected(oracle, case)
    for which, flavour in (("_mzd_ple_russian", "flat"), ("mzd_ple", "ple"), ("mzd_pluq", "pluq")):
        (rank, P, Q), Ao = want[flavour]
        Ar = A.copy()
        got = reference.ple(Ar, which)
        assert got[0] == rank, which
        assert np.array_equal(got[1], P) and np.array_equal(got[2], Q), which
        assert np.array_equal(Ar.valid_words(), Ao.valid_words()), which


def _pq(m, n, pivots):
    """P, Q as a decomposition with the pivots [(row swapped in, column), ...] leaves them: identity elsewhere."""
    P, Q = np.arange(m, dtype=np.int32), np.arange(n, dtype=np.int32)
    for i, (row, col) in enumerate(pivots):
        P[i], Q[i] = row, col
    return P, Q, len(pivots)


def test_classify_by_hand():
    """Three decompositions worked out by hand.

    1. 10 x 70, pivots (row, column) = (0, 0), (5, 1), (2, 65).  Block 0 starts at r0 = 0 with 10 rows left: positions 0 and 5
       (row 5 found for rank position 1), both in the low slot; with 128 rows or fewer left nothing is ever deferred.  Block 1
       starts at r0 = 2: row 2 is position 0.  Classes: wave_lo only.  Without the one-wave search: three pivots inside the window.

    2. 300 x 128, pivots (70, 0), (1, 3), (150, 64).  Block 0, r0 = 0, 300 rows left: position 70 is a high slot, position 0 (row 1
       for rank position 1) a low one; 2 pivots in 64 columns with rows beyond 128: columns were passed over and, all positions being
       below 128, confirmed.  Block 1, r0 = 2: row 150 is position 148 >= 128 with 298 rows left: a miss, found by the general search
       inside its window (148 < 1024); a wave block followed by a missed one.

    3. 3000 x 192, pivots (1030, 0), (1024, 1), (1100, 2), (2500, 5), (4, 130).  Block 0, r0 = 0: positions 1030, 1024, 1100 and 2500
       for t = 0, 1, 2, 3: a miss.  t = 0: 1030 rows below the window's first lane, beyond the window, below 1088: s_head.  t = 1:
       1024 - 1 = 1023 lanes in, inside the window, but the row entered it after the start: stale.  t = 2: 1098 lanes away, position
       1100 >= 1088: from global memory.  t = 3: 2497 lanes away: global memory, and beyond 2048: a later chunk.  Block 1 has no
       pivot; r0 = 4, 2996 rows left: every column deferred and confirmed empty, after a missed block.  Block 2, r0 = 4: row 4 is
       position 0, low slot, 1 pivot in 64 columns: confirmed deferrals.  Without the one-wave search the last pivot is one more
       inside the window and nothing else changes for the others."""
    P, Q, r = _pq(10, 70, [(0, 0), (5, 1), (2, 65)])
    assert classify(P, Q, r, 10, 70) == {"wave_lo"}
    assert classify(P, Q, r, 10, 70, wave=False) == {"window"}

    P, Q, r = _pq(300, 128, [(70, 0), (1, 3), (150, 64)])
    assert classify(P, Q, r, 300, 128) == {"wave_hi", "wave_lo", "deferred_confirmed", "missed", "window", "wave_then_missed"}
    assert classify(P, Q, r, 300, 128, wave=False) == {"window"}

    P, Q, r = _pq(3000, 192, [(1030, 0), (1024, 1), (1100, 2), (2500, 5), (4, 130)])
    assert classify(P, Q, r, 3000, 192) == {"missed", "far_head", "stale", "far_global", "far_chunk2", "deferred_empty", "missed_then_wave",
                                            "wave_lo", "deferred_confirmed"}
    assert classify(P, Q, r, 3000, 192, wave=False) == {"far_head", "stale", "far_global", "far_chunk2", "window"}
