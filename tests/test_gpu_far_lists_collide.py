"""m4ri_amd_lists_collide_batch_dev on lists and words whose batch members lie 5 GiB and more apart: the cases of
tests/test_gpu_far_operands.py for this entry point, built with that module's own pieces (Case, lay, the arena) and run the same way,
as tests/test_gpu_far_row_sums_collide_list.py does for the join of row sums.

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

import far_arena as fa
import lists_collide_cases as lc
import m4ri_amd
import test_far_arena_cpu as table_checks
import test_gpu_far_operands as far
from far_arena import BATCH, BS_EVEN, BS_ODD
from m4ri_amd.mzd import Mzd
from test_gpu_far_operands import arena  # noqa: F401  (the fixture: one arena for this module, as for that one)

ENTRY = "m4ri_amd_lists_collide_batch_dev"
PLAN = "m4ri_amd_plan_lists_collide_batch"
CAP = 128
C = m4ri_amd.lists_collide_units(1, 1, 1, 0, 1)[0]


def _cases():
    """40 x 60 rows is one chunk and one slice (path 0), C + 1 rows on the left two chunks (path 1), pinned through the plan function; the
    windows leave every member some tens of collisions, all listed.  X, Y and V far; and one X shared by all members with Y and V far."""
    out = []
    for BS in (BS_ODD, BS_EVEN):
        s = far.sname(BS)
        for (nx, ny, n, ell, p) in ((40, 60, 130, 6, 0), (C + 1, 300, 130, 16, 1)):
            for shared in (False, True):
                def run_join(ar, oracle, c, nx=nx, ny=ny, n=n, ell=ell, shared=shared):
                    Xb = far.members(lambda b: Mzd.random(nx, n, 3500 + (0 if shared else b)).to_bits())
                    Yb = far.members(lambda b: Mzd.random(ny, n, 3550 + b).to_bits())
                    Vb = far.members(lambda b: Mzd.random(1, n, 3600 + b).to_bits())
                    wins = far.members(lambda b: [int(x) for x in np.random.default_rng(3650 + b).permutation(n)[:ell]])
                    want = far.memo(("lists_collide", nx, ny, n, ell, shared), lambda: [lc.expect(X, Y, V[0], w, 1, n) for X, Y, V, w in zip(Xb, Yb, Vb, wins)])
                    assert all(0 < m <= CAP for _, _, _, m in want)
                    pX = ar.place(c.wins["X"], [far.bits_to(x) for x in (Xb[:1] if shared else Xb)], dirty_tail=True)
                    pY = ar.place(c.wins["Y"], [far.bits_to(x) for x in Yb], dirty_tail=True)
                    pV = ar.place(c.wins["V"], [far.bits_to(x) for x in Vb], dirty_tail=True)
                    cols = torch.from_numpy(np.array(wins, dtype=np.int32)).cuda()
                    hist = torch.full((BATCH * (n + 1),), -7, dtype=torch.int64, device="cuda")
                    light = torch.full((BATCH,), -7, dtype=torch.int64, device="cuda")
                    lst = torch.full((BATCH, CAP), -7, dtype=torch.int64, device="cuda")
                    count = torch.full((BATCH,), -7, dtype=torch.int64, device="cuda")
                    wX, wY, wV = c.wins["X"], c.wins["Y"], c.wins["V"]
                    far._call(ENTRY, pX.ptr, wX.stride, wX.bs, nx, pY.ptr, wY.stride, wY.bs, ny, n, pV.ptr, wV.bs, BATCH, cols.data_ptr(), ell, ell, 1, n,
                              hist.data_ptr(), light.data_ptr(), lst.data_ptr(), CAP, CAP, count.data_ptr(), None)
                    assert np.array_equal(hist.cpu().numpy(), np.concatenate([h for h, _, _, _ in want]))
                    assert light.cpu().numpy().tolist() == [x for _, x, _, _ in want]
                    assert count.cpu().numpy().tolist() == [m for _, _, _, m in want]
                    got = lst.cpu().numpy()
                    for b, (_, _, keys, m) in enumerate(want):
                        assert np.array_equal(np.sort(got[b, :m]), keys) and (got[b, m:] == -7).all(), b
                    assert cols.cpu().numpy().tolist() == wins
                    pX.check_unchanged("X")
                    pY.check_unchanged("Y")
                    pV.check_unchanged("V")
                names = ("Y", "V") if shared else ("X", "Y", "V")
                out.append(far.Case(f"lists_collide_batch-{s}-{nx}x{ny}-n{n}-ell{ell}-path{p}" + ("-shared-X" if shared else ""), ENTRY, "batch", BS,
                                    (nx, ny, n, ell), f"path{p}: {PLAN}", far.lay(BS, names, X=(nx, n, "shared") if shared else (nx, n), Y=(ny, n), V=(1, n)),
                                    names, run_join, plan=(PLAN, (nx, ny, n, ell, BATCH), p)))
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
    for name in ("Y", "V"):           # far in every case: all three thresholds
        assert set(case.wins[name].crossed()) == {name for name, _ in fa.THRESHOLDS}
    assert (case.shape[0] > C) == (case.plan[2] == 1)


def test_the_table_names_the_entry_point():
    assert ENTRY in {c.entry for c in far.CASES} and ENTRY not in far.LEFT_OUT
    table_checks.test_both_parities_of_every_far_stride()


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_far_operands(case, arena, oracle):  # noqa: F811
    far.test_far_operands(case, arena, oracle)
