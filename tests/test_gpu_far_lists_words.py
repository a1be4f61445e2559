"""m4ri_amd_lists_words_batch_dev on lists, words and outputs whose batch members lie 5 GiB and more apart: the cases of
tests/test_gpu_far_operands.py for this entry point, built with that module's own pieces (Case, lay, the arena) and run the same way,
as tests/test_gpu_far_row_sums_words.py does for the words of row sums.  W, the written operand, is placed far as well as X, Y and V --
in cases of its own: the call refuses a W whose span (first member's start to last member's end) meets the span of X, Y or V, and far
operands of one call lie interleaved, so either the read-only operands are far and W compact below them, or the other way round.

The cases are ADDED to that module's table when this module is imported: tests/test_far_arena_cpu.py holds the table to every device
entry point the header declares, and compares the two when it runs, after every test module has been imported.  The table both
modules look up by name (their global CASES) becomes a NEW list, the old one followed by these cases; the old list object, which
their parametrised tests were built from, stays as it is, so those tests are the same in whatever order the files are collected.  A
run of tests/test_far_arena_cpu.py alone, without this module, reports the entry point as missing from the table; a run of the suite,
or of both files, does not.  The arena's size was fixed before the cases were added: they lie inside it (checked below).  The keys and
the skipped counts are ordinary small tensors."""
import numpy as np
import pytest
import torch

import far_arena as fa
import lists_collide_cases as lc
import m4ri_amd
import test_far_arena_cpu as table_checks
import test_gpu_far_operands as far
from far_arena import BATCH, BS_EVEN, BS_ODD
from m4ri_amd.mzd import Mzd
from test_gpu_far_operands import arena  # noqa: F401  (the fixture: one arena for this module, as for that one)

ENTRY = "m4ri_amd_lists_words_batch_dev"
PLAN = "m4ri_amd_plan_lists_collide_batch"
CAP = 70
C = m4ri_amd.lists_collide_units(1, 1, 1, 0, 1)[0]


def _cases():
    """CAP = 70 keys per member (count = NULL: every row of W is written); the lists of one chunk (40 x 60 rows of 130 bits: three words,
    four lanes per row) and of two chunks (C + 1 rows on the left, 1000 bits: sixteen words, the last one partly valid), pinned through the
    plan function of the join; X, Y and V far (one shared X: Y and V) with a compact W, and W far with compact X, Y and V."""
    out = []
    for BS in (BS_ODD, BS_EVEN):
        s = far.sname(BS)
        for (nx, ny, n, p) in ((40, 60, 130, 0), (C + 1, 300, 1000, 1)):
            for shared, names in ((False, ("X", "Y", "V")), (True, ("Y", "V")), (False, ("W",))):
                def run_words(ar, oracle, c, nx=nx, ny=ny, n=n, shared=shared):
                    Xb = far.members(lambda b: Mzd.random(nx, n, 3700 + (0 if shared else b)).to_bits())
                    Yb = far.members(lambda b: Mzd.random(ny, n, 3750 + b).to_bits())
                    Vb = far.members(lambda b: Mzd.random(1, n, 3800 + b).to_bits())
                    ranks = np.random.default_rng(3850 + nx).integers(0, nx * ny, size=(BATCH, CAP))
                    ranks[:, 0], ranks[:, 1], ranks[:, -1] = 0, (nx - 1) * ny, nx * ny - 1      # the first row, the last chunk's first, the last pair
                    want = far.memo(("lists_words", nx, ny, n, shared), lambda: [far.bits_to(lc.words_of(X, Y, V[0], r)) for X, Y, V, r in zip(Xb, Yb, Vb, ranks)])
                    pX = ar.place(c.wins["X"], [far.bits_to(x) for x in (Xb[:1] if shared else Xb)], dirty_tail=True)
                    pY = ar.place(c.wins["Y"], [far.bits_to(x) for x in Yb], dirty_tail=True)
                    pV = ar.place(c.wins["V"], [far.bits_to(x) for x in Vb], dirty_tail=True)
                    pW = ar.place(c.wins["W"], far.members(lambda b: Mzd.random(CAP, n, 3900 + b)), dirty_tail=True)
                    keys = torch.from_numpy(ranks | (np.int64(5) << 40)).cuda()
                    skipped = torch.full((BATCH,), -7, dtype=torch.int32, device="cuda")
                    wX, wY, wV, wW = c.wins["X"], c.wins["Y"], c.wins["V"], c.wins["W"]
                    far._call(ENTRY, pX.ptr, wX.stride, wX.bs, nx, pY.ptr, wY.stride, wY.bs, ny, n, pV.ptr, wV.bs, BATCH, keys.data_ptr(), CAP, CAP, None, pW.ptr,
                              wW.stride, wW.bs, skipped.data_ptr(), None)
                    pW.check(want, "kept", "W")
                    assert skipped.cpu().numpy().tolist() == [0] * BATCH
                    assert np.array_equal(keys.cpu().numpy(), ranks | (np.int64(5) << 40))
                    pX.check_unchanged("X")
                    pY.check_unchanged("Y")
                    pV.check_unchanged("V")
                out.append(far.Case(f"lists_words_batch-{s}-{nx}x{ny}-n{n}-far:{''.join(names)}" + ("-shared-X" if shared else ""), ENTRY, "batch", BS,
                                    (nx, ny, n, CAP), "one kernel: a thread per key, then a group of lanes per row",
                                    far.lay(BS, names, X=(nx, n, "shared") if shared else (nx, n), Y=(ny, n), V=(1, n), W=(CAP, n)), names, run_words,
                                    plan=(PLAN, (nx, ny, n, 0, BATCH), p)))
    return out


CASES = _cases()
far.CASES = table_checks.CASES = far.CASES + CASES
assert len({c.id for c in far.CASES}) == len(far.CASES)
IDS = [c.id for c in CASES]


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_case_arithmetic(case):
    """What tests/test_far_arena_cpu.py asks of every case of the table, without a GPU: the thresholds crossed, the windows disjoint
    and inside the arena as it was sized, every truncation image inside it."""
    table_checks.test_case_arithmetic(case)
    assert case.far in (("X", "Y", "V"), ("Y", "V"), ("W",))
    for operand in case.far:          # every far operand crosses all three thresholds
        assert set(case.wins[operand].crossed()) == {name for name, _ in fa.THRESHOLDS}


def test_the_table_names_the_entry_point():
    assert ENTRY in {c.entry for c in far.CASES} and ENTRY not in far.LEFT_OUT
    table_checks.test_both_parities_of_every_far_stride()


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_far_operands(case, arena, oracle):  # noqa: F811
    far.test_far_operands(case, arena, oracle)
