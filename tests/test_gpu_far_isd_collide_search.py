"""m4ri_amd_isd_collide_search_dev on operands whose batch members lie 5 GiB and more apart: the cases of tests/test_gpu_far_operands.py
for this entry point, built with that module's own pieces (Case, lay, the arena) and run the same way, as tests/test_gpu_far_isd_search.py
does for its entry point.

The cases are ADDED to that module's table when this module is imported: tests/test_far_arena_cpu.py holds the table to every device
entry point the header declares, and compares the two when it runs, after every test module has been imported.  The table the modules
look up by name (their global CASES) becomes a NEW list, the old one followed by these cases; the old list object, which their
parametrised tests were built from, stays as it is.  The arena's size was fixed before the cases were added: they lie inside it
(checked below).

The call refuses operands whose spans meet, so one operand of a case is far -- D, or W, one row of ncols bits per member -- and the
other is compact below it; pivots, rank, the order (whose entries pivot_rows .. pivot_rows + ell - 1 are the window) and the small
outputs are arrays outside the arena.  Two shapes, one word and three words wide, three iterations."""
import numpy as np
import pytest
import torch

import far_arena as fa
import isd_collide_cases as icc
import m4ri_amd
import order_cases as oc
import test_far_arena_cpu as table_checks
import test_gpu_far_operands as far
from far_arena import BATCH, BS_EVEN, BS_ODD
from m4ri_amd.mzd import Mzd
from test_gpu_far_operands import arena  # noqa: F401  (the fixture: one arena for this module, as for that one)

ENTRY, PLAN = "m4ri_amd_isd_collide_search_dev", "m4ri_amd_plan_isd_collide_search"
assert ENTRY in m4ri_amd.SYMBOLS and PLAN in m4ri_amd.SYMBOLS        # the library has the call: without it none of this module holds
ITERS, STEPS, SEED, T1, T2, W_MIN = 3, 5, 43, 1, 1, 1
# (rows, columns, pivot_rows, k1, ell)
SHAPES = ((33, 64, 32, 16, 2), (70, 130, 60, 30, 3))


def _reference(nr, nc, pr, k1, ell):
    """Per member: (the form, pivots, rank, order) before and the rule's Result."""
    out = []
    for b in range(BATCH):
        order = oc.random_order(33, b, nc)
        S, rank, piv = oc.ech_order(Mzd.random(nr, nc, 3400 + b).to_bits(), order, 1, pr)
        out.append(((S, piv, rank, order), icc.search(S, piv, rank, pr, ITERS, STEPS, SEED, k1, T1, T2, ell, W_MIN, -1, b=b, order=order)))
    return out


def _cases():
    out = []
    for BS in (BS_ODD, BS_EVEN):
        s = far.sname(BS)
        for (nr, nc, pr, k1, ell) in SHAPES:
            for which in ("D", "W"):
                def run(ar, oracle, c, nr=nr, nc=nc, pr=pr, k1=k1, ell=ell):
                    ref = far.memo(("isd_collide_search", nr, nc, pr), lambda: _reference(nr, nc, pr, k1, ell))
                    pD = ar.place(c.wins["D"], [Mzd.from_bits(before[0]) for before, _after in ref], dirty_tail=True)
                    pW = ar.place(c.wins["W"], [Mzd(1, nc) for _ in ref], dirty_tail=True)
                    pv = far._dev(np.concatenate([before[1] for before, _after in ref]))
                    rk = far._dev(np.array([before[2] for before, _after in ref]))
                    od = far._dev(np.concatenate([before[3] for before, _after in ref]))
                    best = torch.full((BATCH,), -7, dtype=torch.int64, device="cuda")
                    bi, ru, dn = (torch.full((BATCH,), -7, dtype=torch.int32, device="cuda") for _ in range(3))
                    wD, wW = c.wins["D"], c.wins["W"]
                    far._call(ENTRY, pD.ptr, wD.stride, wD.bs, nr, nc, pr, pv.data_ptr(), rk.data_ptr(), BATCH, ITERS, STEPS, SEED, k1, T1, T2, ell, W_MIN, -1,
                              od.data_ptr(), nc, nc, best.data_ptr(), bi.data_ptr(), ru.data_ptr(), dn.data_ptr(), pW.ptr, wW.bs, None)
                    assert far._host(best).tolist() == [r.best for _before, r in ref] and far._host(bi).tolist() == [r.best_iter for _before, r in ref]
                    assert far._host(ru).tolist() == [ITERS] * BATCH and far._host(dn).tolist() == [r.done for _before, r in ref]
                    assert np.array_equal(far._host(pv), np.concatenate([r.pivots for _before, r in ref]))
                    assert np.array_equal(far._host(od), np.concatenate([r.order for _before, r in ref]))
                    pD.check([Mzd.from_bits(r.bits) for _before, r in ref], "kept", "D")
                    pW.check([Mzd.from_bits(r.W[None, :]) for _before, r in ref], "kept", "W")
                out.append(far.Case(f"isd_collide_search-{s}-{nr}x{nc}-far:{which}", ENTRY, "batch", BS, (nr, nc), f"path1: {PLAN}",
                                    far.lay(BS, (which,), D=(nr, nc), W=(1, nc)), (which,), run, plan=(PLAN, (nr, nc, pr, k1, T1, T2, ell), 1)))
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
    assert len(case.far) == 1 and set(case.wins[case.far[0]].crossed()) == {name for name, _ in fa.THRESHOLDS}


def test_the_table_names_the_entry_point():
    """The comparison of the whole table with the header is tests/test_far_arena_cpu.py's, once every module has added its cases."""
    assert ENTRY in {c.entry for c in far.CASES} and ENTRY not in far.LEFT_OUT
    assert {c.stride for c in CASES} == {BS_ODD, BS_EVEN}
    table_checks.test_both_parities_of_every_far_stride()


def test_the_reference_searches():
    """The members of the GPU cases, on the host: every member performs steps and finds a word, the best of some member comes from a
    later iteration, so a far operand that is not reached shows."""
    for (nr, nc, pr, k1, ell) in SHAPES:
        ref = far.memo(("isd_collide_search", nr, nc, pr), lambda: _reference(nr, nc, pr, k1, ell))
        assert all(r.done > 0 and r.best >= 0 and r.W.any() and not np.array_equal(before[0], r.bits) for before, r in ref)
        assert any(r.best_iter > 0 for _before, r in ref)


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_far_operands(case, arena, oracle):  # noqa: F811
    far.test_far_operands(case, arena, oracle)
