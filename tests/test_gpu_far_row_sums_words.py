"""m4ri_amd_row_sums_words_batch_dev on generators, words and outputs whose batch members lie 5 GiB and more apart: the cases of
tests/test_gpu_far_operands.py for this entry point, built with that module's own pieces (Case, lay, the arena) and run the same way,
as tests/test_gpu_far_row_sums_collide.py does for its entry point.  W, the written operand, is placed far as well as G and V -- in
cases of its own: the call refuses a W whose span (first member's start to last member's end) meets the span of G or V, and far
operands of one call lie interleaved, so either the read-only operands are far and W compact below them, or the other way round.

The cases are ADDED to that module's table when this module is imported: tests/test_far_arena_cpu.py holds the table to every device
entry point the header declares, and compares the two when it runs, after every test module has been imported.  The table both
modules look up by name (their global CASES) becomes a NEW list, the old one followed by these cases; the old list object, which
their parametrised tests were built from, stays as it is, so those tests are the same in whatever order the files are collected.  A
run of tests/test_far_arena_cpu.py alone, without this module, reports the entry point as missing from the table; a run of the suite,
or of both files, does not.  The arena's size was fixed before the cases were added: they lie inside it (checked below).  The keys and
the skipped counts are ordinary small tensors."""
from math import comb

import numpy as np
import pytest
import torch

import collide_list_cases as cl
import far_arena as fa
import test_far_arena_cpu as table_checks
import test_gpu_far_operands as far
from far_arena import BATCH, BS_EVEN, BS_ODD
from m4ri_amd.mzd import Mzd
from test_gpu_far_operands import arena  # noqa: F401  (the fixture: one arena for this module, as for that one)

ENTRY = "m4ri_amd_row_sums_words_batch_dev"
CAP = 70


def _cases():
    """CAP = 70 keys per member (count = NULL: every row of W is written), n = 130 (three words, four lanes per row) and n = 1000
    (sixteen words, the last one partly valid); G and V far (one shared G: V alone) with a compact W, and W far with compact G and V."""
    out = []
    for BS in (BS_ODD, BS_EVEN):
        s = far.sname(BS)
        for (k1, t1, k2, t2, n) in ((6, 2, 8, 2, 130), (30, 2, 40, 3, 1000)):
            k = k1 + k2
            for shared, names in ((False, ("G", "V")), (True, ("V",)), (False, ("W",))):
                def run_words(ar, oracle, c, k=k, n=n, k1=k1, t1=t1, t2=t2, shared=shared):
                    Gb = far.members(lambda b: Mzd.random(k, n, 3300 + (0 if shared else b)).to_bits())
                    Vb = far.members(lambda b: Mzd.random(1, n, 3350 + b).to_bits())
                    pairs = comb(k1, t1) * comb(k - k1, t2)
                    ranks = np.random.default_rng(3400 + k).integers(0, pairs, size=(BATCH, CAP))
                    ranks[:, 0], ranks[:, -1] = 0, pairs - 1
                    want = far.memo(("row_sums_words", k, n, k1, t1, t2, shared),
                                    lambda: [far.bits_to(cl.words_of(G, V[0], k1, t1, t2, r)) for G, V, r in zip(Gb, Vb, ranks)])
                    pG = ar.place(c.wins["G"], [far.bits_to(x) for x in (Gb[:1] if shared else Gb)], dirty_tail=True)
                    pV = ar.place(c.wins["V"], [far.bits_to(x) for x in Vb], dirty_tail=True)
                    pW = ar.place(c.wins["W"], far.members(lambda b: Mzd.random(CAP, n, 3450 + b)), dirty_tail=True)
                    keys = torch.from_numpy(ranks | (np.int64(5) << 40)).cuda()
                    skipped = torch.full((BATCH,), -7, dtype=torch.int32, device="cuda")
                    wG, wV, wW = c.wins["G"], c.wins["V"], c.wins["W"]
                    far._call(ENTRY, pG.ptr, wG.stride, wG.bs, k, n, pV.ptr, wV.bs, BATCH, k1, t1, t2, keys.data_ptr(), CAP, CAP, None, pW.ptr, wW.stride, wW.bs,
                              skipped.data_ptr(), None)
                    pW.check(want, "kept", "W")
                    assert skipped.cpu().numpy().tolist() == [0] * BATCH
                    assert np.array_equal(keys.cpu().numpy(), ranks | (np.int64(5) << 40))
                    pG.check_unchanged("G")
                    pV.check_unchanged("V")
                out.append(far.Case(f"row_sums_words_batch-{s}-k{k1}+{k2}-n{n}-t{t1}+{t2}-far:{''.join(names)}" + ("-shared-G" if shared else ""), ENTRY, "batch",
                                    BS, (k, n, k1, t1, t2, CAP), "one kernel: a thread per key, then a group of lanes per row",
                                    far.lay(BS, names, G=(k, n, "shared") if shared else (k, n), V=(1, n), W=(CAP, n)), names, run_words))
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
    assert case.far in (("G", "V"), ("V",), ("W",))
    for operand in case.far:
        if operand != "G" or "shared-G" not in case.id:   # every far operand crosses all three thresholds
            assert set(case.wins[operand].crossed()) == {name for name, _ in fa.THRESHOLDS}


def test_the_table_names_the_entry_point():
    assert ENTRY in {c.entry for c in far.CASES} and ENTRY not in far.LEFT_OUT
    table_checks.test_every_device_entry_point_has_a_far_case_or_a_reason()
    table_checks.test_both_parities_of_every_far_stride()


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_far_operands(case, arena, oracle):  # noqa: F811
    far.test_far_operands(case, arena, oracle)
