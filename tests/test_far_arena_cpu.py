"""The arithmetic of tests/far_arena.py and of the case table of tests/test_gpu_far_operands.py, without a GPU: every declared
case really crosses the 32-bit thresholds it claims, its windows are disjoint and inside the arena, every truncation image of every
word of every operand lies inside the arena (the argument that a 32-bit defect cannot fault), every B side is one launch_leaf can
cut -- and the table names every device entry point the header declares."""
import numpy as np
import pytest

import far_arena as fa
import m4ri_amd
import m4ri_amd.build
import test_gpu_far_operands as far
from far_arena import BASE, Win

CASES, ARENA = far.CASES, far.ARENA_WORDS
ALL = tuple(name for name, _ in fa.THRESHOLDS)
ids = [c.id for c in CASES]

# The thresholds a case declares unreachable, pinned: (entry point, the case's own label) -> thresholds.  A threshold cannot drop out of
# the table without this list changing.
UNREACHED = {
    ("m4ri_amd_mul_dev", "B alone far, 70 rows"): ("int32-words",),
    ("m4ri_amd_m4rm_dev", "B alone far, 70 rows"): ("int32-words",),
    ("m4ri_amd_trsm_lower_left_dev", "64-row base kernel"): ("uint32-bytes", "int32-words"),
    ("m4ri_amd_trsm_upper_left_dev", "64-row base kernel"): ("uint32-bytes", "int32-words"),
    ("m4ri_amd_apply_p_right_trans_tri_dev", "the first rank rows"): ("int32-words",),
    ("m4ri_amd_mul_dev", "refused, 256 rows"): ("int32-words",),
    ("m4ri_amd_mul_batch_dev", "refused, 256 rows"): ("int32-words",),
}


def test_geometry_constants():
    assert fa.S_ODD % 2 == 1 and fa.S_EVEN % 2 == 0 and fa.BS_ODD % 2 == 1 and fa.BS_EVEN % 2 == 0 and fa.S_TABLE % 2 == 1 and fa.S_TABLE_EVEN % 2 == 0
    assert fa.B_STRIDE_MAX == 8_386_560 and fa.S_EVEN < fa.B_STRIDE_MAX
    assert Win(0, 270, 1, fa.S_ODD).crossed() == ALL and Win(0, 269, 1, fa.S_ODD).crossed() == ALL[:2]
    assert Win(0, 256, 1, fa.S_TABLE).crossed() == ALL
    assert Win(0, 1, 1, 2, fa.BATCH, fa.BS_ODD).crossed() == ALL and Win(0, 1, 1, 2, fa.BATCH - 1, fa.BS_EVEN).crossed() == ALL[:2]
    assert BASE - (1 << 31) >= 0
    # about 35 GiB: the far rows of the refused stride reach furthest
    assert 34 << 30 < 8 * ARENA < 36 << 30, 8 * ARENA / 2**30
    assert ARENA == BASE + 299 * fa.S_REFUSED + 4096 * 5 + 5 + fa.TAIL_ROOM   # C of the second member of a refused batch


def test_pattern_is_position_dependent():
    i = np.array([0, 1, 2, 1 << 29, (1 << 29) + 1, 1 << 31, (1 << 31) + 1, ARENA - 1], dtype=np.uint64)
    p = fa.pattern_np(i)
    assert len(set(p.tolist())) == len(i) and p[1] == fa.PATTERN_MUL and fa.PATTERN_MUL % 2 == 1
    assert (fa._MUL_I64 + (1 << 64)) == fa.PATTERN_MUL and -(1 << 63) <= fa._MUL_I64 < 0


def test_truncation_images_of_a_known_window():
    w = Win(4096, 300, 5, fa.S_ODD)
    im = fa.truncation_images(w)
    p = BASE + 4096
    assert im["uint32-bytes"][0] >= p and im["uint32-bytes"][1] < p + (1 << 29)
    assert im["int32-bytes"][0] >= p - (1 << 28) and im["int32-bytes"][1] < p + (1 << 28)
    assert im["int32-words"][0] >= p - (1 << 31) and im["int32-words"][1] < p + (1 << 31)
    assert im["int32-words"][0] == p + 269 * fa.S_ODD - (1 << 32)     # row 269 is the first whose word offset goes negative as int32
    assert im["product-32"][0] == im["int32-words"][0] and im["product-32"][1] == p + 299 * fa.S_ODD + 4
    assert fa.disjoint([w, Win(0, 300, 5, fa.S_ODD)]) and not fa.disjoint([w, Win(4100, 300, 5, fa.S_ODD)]) and not fa.disjoint([Win(0, 2, 5, 4)])


@pytest.mark.parametrize("case", CASES, ids=ids)
def test_case_arithmetic(case):
    assert case.axis in ("rows", "batch") and set(case.far) <= set(case.wins) and case.far
    # thresholds: crossed by the rows the call touches of a far operand, or declared unreachable -- and then really not crossed
    crossed, most = set(), 0
    assert set(case.touched) <= set(case.far) and bool(case.unreached) == bool(case.label)
    for name in case.far:
        w = case.wins[name]
        rows = case.touched.get(name, w.rows)
        assert 0 < rows <= w.rows
        crossed |= set(Win(w.off, rows, w.width, w.stride, w.batch, w.bs).crossed())
        most = max(most, rows if w.stride not in (fa.S_TABLE, fa.S_TABLE_EVEN) else fa.FAR_ROWS_MIN)
        by_rows, by_batch = (w.rows - 1) * w.stride, (w.batch - 1) * w.bs
        if case.axis == "rows":
            assert w.stride in (case.stride, fa.S_TABLE, fa.S_TABLE_EVEN) and w.rows <= fa.FAR_ROWS_MAX and by_batch < 1 << 20, "far by its rows only, at most 300 of them"
        else:
            assert w.bs == case.stride and w.batch == fa.BATCH and by_rows < 1 << 20, "far by its batch stride only"
    if case.axis == "rows" and not case.unreached:
        assert most >= fa.FAR_ROWS_MIN, "no far operand with the rows it takes to cross 2^31 words, and no reason given"
    assert crossed | set(case.unreached) == set(ALL) and not crossed & set(case.unreached), (crossed, case.unreached)
    # windows: inside the arena, and disjoint unless declared one operand
    wins = dict(case.wins)
    for a, b in case.same:
        assert wins[a] == wins[b]
        del wins[b]
    for w in wins.values():
        assert w.off >= 0 and BASE + w.off + w.last_word() + fa.TAIL_ROOM <= ARENA
        if w.batch > 1:
            assert w.bs >= (w.rows - 1) * w.stride + w.width or case.axis == "rows"
    assert fa.disjoint(list(wins.values()))
    # the four truncation images of every word of every operand stay inside the arena
    for name, w in wins.items():
        for kind, (lo, hi) in fa.truncation_images(w).items():
            assert 0 <= lo and hi < ARENA, (name, kind, lo, hi)
    # B sides
    for name in case.b_sides:
        w = case.wins[name]
        assert (64 * w.stride * 8 >= fa.LEAF_LIMIT) == case.refused, (name, w.stride)
    if case.refused:
        assert case.stride == fa.S_REFUSED
    # the path the shape is declared to reach (pure host arithmetic of the library)
    if case.plan:
        fn, args, want = case.plan
        assert getattr(m4ri_amd.lib(), fn)(*args) == want, case.plan


def test_unreached_thresholds_are_pinned():
    got = {}
    for c in CASES:
        if c.unreached:
            assert all(isinstance(v, str) and v for v in c.unreached.values()), "a reason for every threshold"
            got.setdefault((c.entry, c.label), set()).add(tuple(sorted(c.unreached)))
    assert {k: {tuple(sorted(v))} for k, v in UNREACHED.items()} == got


def test_both_parities_of_every_far_stride():
    by_entry = {}
    for c in CASES:
        if not c.refused and c.stride != fa.S_REFUSED:
            by_entry.setdefault((c.entry, c.axis), set()).add(c.stride % 2)
    assert all(v == {0, 1} for v in by_entry.values()), {k: v for k, v in by_entry.items() if v != {0, 1}}


def test_every_device_entry_point_has_a_far_case_or_a_reason():
    """Every function of include/m4ri_amd.h that takes a device matrix (its name ends in _dev) is in the case table or in the list
    of what is left out, with the reason: a new entry point cannot be added without one or the other."""
    declared = {n for n in m4ri_amd.build.declared_functions() if n.endswith("_dev")}
    covered = {c.entry for c in CASES}
    assert covered <= declared, covered - declared
    assert not covered & set(far.LEFT_OUT)
    assert declared == covered | set(far.LEFT_OUT), (declared - covered - set(far.LEFT_OUT), set(far.LEFT_OUT) - declared)
    assert all(k in far.__doc__ for k in far.LEFT_OUT)
