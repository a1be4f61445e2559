"""m4ri_amd_row_sums_collide_list_batch_dev on generators and words whose batch members lie 5 GiB and more apart: the cases of
tests/test_gpu_far_operands.py for this entry point, built with that module's own pieces (Case, lay, the arena) and run the same way,
as tests/test_gpu_far_row_sums_collide.py does for the call without the list.

The cases are ADDED to that module's table when this module is imported: tests/test_far_arena_cpu.py holds the table to every device
entry point the header declares, and compares the two when it runs, after every test module has been imported.  The table both
modules look up by name (their global CASES) becomes a NEW list, the old one followed by these cases; the old list object, which
their parametrised tests were built from, stays as it is, so those tests are the same in whatever order the files are collected.  A
run of tests/test_far_arena_cpu.py alone, without this module, reports the entry point as missing from the table; a run of the suite,
or of both files, does not.  The arena's size was fixed before the cases were added: they lie inside it (checked below).  The windows
(cols), the list and the count are ordinary small tensors."""
import numpy as np
import pytest
import torch

import collide_cases as cc
import collide_list_cases as cl
import far_arena as fa
import test_far_arena_cpu as table_checks
import test_gpu_far_operands as far
from far_arena import BATCH, BS_EVEN, BS_ODD
from m4ri_amd.mzd import Mzd
from test_gpu_far_operands import arena  # noqa: F401  (the fixture: one arena for this module, as for that one)

ENTRY = "m4ri_amd_row_sums_collide_list_batch_dev"
PLAN = "m4ri_amd_plan_row_sums_collide_batch"
CAP = 64


def _cases():
    """The shapes of tests/test_gpu_far_row_sums_collide.py: C(6, 2) * C(8, 2) = 420 pairs per member is path 0, C(30, 2) * C(80, 3) =
    3.6 * 10^7 path 1 (189 slices), pinned through the plan function; the band 1 .. w_max leaves every member a few keys below CAP."""
    out = []
    for BS in (BS_ODD, BS_EVEN):
        s = far.sname(BS)
        for (k1, t1, k2, t2, n, ell, w_max, p) in ((6, 2, 8, 2, 130, 4, 62, 0), (30, 2, 80, 3, 130, 12, 44, 1)):
            k = k1 + k2
            for shared in (False, True):
                def run_list(ar, oracle, c, k=k, n=n, k1=k1, t1=t1, t2=t2, ell=ell, w_max=w_max, shared=shared):
                    Gb = far.members(lambda b: Mzd.random(k, n, 3100 + (0 if shared else b)).to_bits())
                    Vb = far.members(lambda b: Mzd.random(1, n, 3150 + b).to_bits())
                    wins = far.members(lambda b: [int(x) for x in np.random.default_rng(3200 + b).permutation(n)[:ell]])
                    want = far.memo(("row_sums_collide_list", k, n, k1, t1, t2, ell, shared),
                                    lambda: [cc.expect(G, V[0], k1, t1, t2, w, 1) + cl.expect(G, V[0], k1, t1, t2, w, 1, w_max) for G, V, w in zip(Gb, Vb, wins)])
                    assert all(0 < m <= CAP for _, _, _, m in want)
                    pG = ar.place(c.wins["G"], [far.bits_to(x) for x in (Gb[:1] if shared else Gb)], dirty_tail=True)
                    pV = ar.place(c.wins["V"], [far.bits_to(x) for x in Vb], dirty_tail=True)
                    cols = torch.from_numpy(np.array(wins, dtype=np.int32)).cuda()
                    hist = torch.full((BATCH * (n + 1),), -7, dtype=torch.int64, device="cuda")
                    light = torch.full((BATCH,), -7, dtype=torch.int64, device="cuda")
                    lst = torch.full((BATCH, CAP), -7, dtype=torch.int64, device="cuda")
                    count = torch.full((BATCH,), -7, dtype=torch.int64, device="cuda")
                    wG, wV = c.wins["G"], c.wins["V"]
                    far._call(ENTRY, pG.ptr, wG.stride, wG.bs, k, n, pV.ptr, wV.bs, BATCH, k1, t1, t2, cols.data_ptr(), ell, ell, 1, w_max, hist.data_ptr(),
                              light.data_ptr(), lst.data_ptr(), CAP, CAP, count.data_ptr(), None)
                    assert np.array_equal(hist.cpu().numpy(), np.concatenate([h for h, _, _, _ in want]))
                    assert light.cpu().numpy().tolist() == [x for _, x, _, _ in want]
                    assert count.cpu().numpy().tolist() == [m for _, _, _, m in want]
                    got = lst.cpu().numpy()
                    for b, (_, _, keys, m) in enumerate(want):
                        assert np.array_equal(np.sort(got[b, :m]), keys) and (got[b, m:] == -7).all(), b
                    assert cols.cpu().numpy().tolist() == wins
                    pG.check_unchanged("G")
                    pV.check_unchanged("V")
                names = ("V",) if shared else ("G", "V")
                out.append(far.Case(f"row_sums_collide_list_batch-{s}-k{k1}+{k2}-n{n}-t{t1}+{t2}-ell{ell}-path{p}" + ("-shared-G" if shared else ""), ENTRY, "batch",
                                    BS, (k, n, k1, t1, t2, ell), f"path{p}: {PLAN}", far.lay(BS, names, G=(k, n, "shared") if shared else (k, n), V=(1, n)),
                                    names, run_list, plan=(PLAN, (k, n, k1, t1, t2, ell), p)))
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
    assert set(case.wins["V"].crossed()) == {name for name, _ in fa.THRESHOLDS}   # V is far in every case: all three thresholds


def test_the_table_names_the_entry_point():
    assert ENTRY in {c.entry for c in far.CASES} and ENTRY not in far.LEFT_OUT
    table_checks.test_every_device_entry_point_has_a_far_case_or_a_reason()
    table_checks.test_both_parities_of_every_far_stride()


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_far_operands(case, arena, oracle):  # noqa: F811
    far.test_far_operands(case, arena, oracle)
