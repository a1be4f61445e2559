"""m4ri_amd_sort_rows_batch_dev on lists and outputs whose batch members lie 5 GiB and more apart: the cases of
tests/test_gpu_far_operands.py for this entry point, built with that module's own pieces (Case, lay, the arena) and run the same way,
as tests/test_gpu_far_lists_words.py does for the words of two lists.  The written operands are placed far as well as X, in cases of their
own: the call refuses an output whose span (first member's start to last member's end) meets the span of X or of another output, and far
operands of one call lie interleaved, so either X is far and the outputs compact below it, or ONE output is far above a compact X.  order,
uniq and mult share one batch stride l_bs, so with a far l_bs the other two are not asked for (their spans would meet): order far with
ucount alone, and uniq far with ucount.  mult needs uniq beside it and is therefore never far; it is indexed as uniq is, entry by entry.
An output member is a window of ONE row of nx words, an int64 entry each.

The cases are ADDED to that module's table when this module is imported: tests/test_far_arena_cpu.py holds the table to every device
entry point the header declares, and compares the two when it runs, after every test module has been imported.  The table both
modules look up by name (their global CASES) becomes a NEW list, the old one followed by these cases; the old list object, which
their parametrised tests were built from, stays as it is, so those tests are the same in whatever order the files are collected.  A
run of tests/test_far_arena_cpu.py alone, without this module, reports the entry point as missing from the table; a run of the suite,
or of both files, does not.  The arena's size was fixed before the cases were added: they lie inside it (checked below).  xcount, the
windows, ucount and the scratch are ordinary small tensors."""
import numpy as np
import pytest
import torch

import far_arena as fa
import m4ri_amd
import sort_rows_cases as sr
import test_far_arena_cpu as table_checks
import test_gpu_far_operands as far
from far_arena import BATCH, BS_EVEN, BS_ODD
from m4ri_amd.mzd import Mzd
from test_gpu_far_operands import arena  # noqa: F401  (the fixture: one arena for this module, as for that one)

ENTRY = "m4ri_amd_sort_rows_batch_dev"
PLAN = "m4ri_amd_plan_sort_rows_batch"
ELL = 9
C = m4ri_amd.sort_rows_units(1, 1, 0, 1)[0]
OUTS = ("O", "U", "M")


def _cases():
    """300 rows of 130 bits sort in one workgroup's LDS (path 0), C + 1 rows of 130 bits go through the scratch (path 1), pinned through the
    plan function; the rows come from a small pool, a window per member, and two members are shorter than nx, so every output has
    entries that must keep what they held.  X far with all four outputs compact, order far with a compact X, uniq far with a compact X."""
    out = []
    for BS in (BS_ODD, BS_EVEN):
        s = far.sname(BS)
        for (nx, n, p) in ((300, 130, 0), (C + 1, 130, 1)):
            for names in (("X",), ("O",), ("U",)):
                asked = OUTS if names == ("X",) else names
                def run_sort(ar, oracle, c, nx=nx, n=n, asked=asked):
                    Xb = far.members(lambda b: sr.pool_rows(np.random.default_rng(4100 + b), nx, n, 40 + b))
                    counts = [nx, nx - 3, nx // 2, nx][:BATCH] + [nx] * (BATCH - 4)
                    wins = far.members(lambda b: [int(x) for x in np.random.default_rng(4150 + b).permutation(n)[:ELL]])
                    want = far.memo(("sort_rows", nx, n), lambda: [sr.expect(X[:m], w) for X, m, w in zip(Xb, counts, wins)])
                    pX = ar.place(c.wins["X"], [far.bits_to(x) for x in Xb], dirty_tail=True)
                    placed = {k: ar.place(c.wins[k], far.members(lambda b: Mzd.random(1, 64 * nx, 4200 + 10 * i + b))) for i, k in enumerate(OUTS) if k in asked}
                    ptr = lambda k: placed[k].ptr if k in placed else None
                    xcount = torch.from_numpy(np.array(counts, dtype=np.int64)).cuda()
                    cols = torch.from_numpy(np.array(wins, dtype=np.int32)).cuda()
                    ucount = torch.full((BATCH,), -7, dtype=torch.int64, device="cuda")
                    need = m4ri_amd.sort_rows_scratch_bytes(nx, n, ELL, BATCH)
                    scratch = torch.zeros(max(need, 16), dtype=torch.uint8, device="cuda")
                    wX, l_bs = c.wins["X"], {c.wins[k].bs for k in asked}
                    assert len(l_bs) == 1
                    far._call(ENTRY, pX.ptr, wX.stride, wX.bs, nx, n, xcount.data_ptr(), BATCH, cols.data_ptr(), ELL, ELL, ptr("O"), ucount.data_ptr(), ptr("U"),
                              ptr("M"), l_bs.pop(), scratch.data_ptr(), need, None)
                    assert ucount.cpu().numpy().tolist() == [len(w[1]) for w in want]
                    for k, name in enumerate(OUTS):
                        if name not in placed:
                            continue
                        got, before = placed[name].fetch().view(np.int64), placed[name].before.view(np.int64)
                        for b, w in enumerate(want):
                            assert np.array_equal(got[b, 0, :len(w[k])], w[k]), (name, b)
                            assert np.array_equal(got[b, 0, len(w[k]):], before[b, 0, len(w[k]):]), (name, b, "behind the last entry")
                    assert xcount.cpu().numpy().tolist() == counts and cols.cpu().numpy().tolist() == wins
                    pX.check_unchanged("X")
                out.append(far.Case(f"sort_rows_batch-{s}-{nx}-n{n}-path{p}-far:{''.join(names)}", ENTRY, "batch", BS, (nx, n, ELL),
                                    f"path{p}: {PLAN}", far.lay(BS, names, X=(nx, n), **{k: (1, 64 * nx) for k in asked}), names, run_sort,
                                    plan=(PLAN, (nx, n, ELL, BATCH), p)))
    return out


CASES = _cases()
far.CASES = table_checks.CASES = far.CASES + CASES
assert len({c.id for c in far.CASES}) == len(far.CASES)
IDS = [c.id for c in CASES]


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_case_arithmetic(case):
    """What tests/test_far_arena_cpu.py asks of every case of the table, without a GPU: the thresholds crossed, the windows disjoint
    and inside the arena as it was sized, every truncation image inside it, the declared path."""
    table_checks.test_case_arithmetic(case)
    assert case.far in (("X",), ("O",), ("U",))
    for operand in case.far:          # every far operand crosses all three thresholds
        assert set(case.wins[operand].crossed()) == {name for name, _ in fa.THRESHOLDS}
    assert (case.shape[0] > C) == (case.plan[2] == 1)
    outs = [case.wins[k] for k in OUTS if k in case.wins]
    assert len({w.bs for w in outs}) == 1 and outs[0].bs >= case.shape[0]                          # one l_bs for the outputs of a call


def test_the_table_names_the_entry_point():
    assert ENTRY in {c.entry for c in far.CASES} and ENTRY not in far.LEFT_OUT
    table_checks.test_both_parities_of_every_far_stride()


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_far_operands(case, arena, oracle):  # noqa: F811
    far.test_far_operands(case, arena, oracle)
