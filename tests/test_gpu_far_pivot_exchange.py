"""m4ri_amd_pivot_exchange_batch_dev on operands whose batch members lie 5 GiB and more apart: the cases of
tests/test_gpu_far_operands.py for this entry point, built with that module's own pieces (Case, lay, the arena) and run the same way,
as tests/test_gpu_far_echelonize_order.py does for its entry points.

The cases are ADDED to that module's table when this module is imported: tests/test_far_arena_cpu.py holds the table to every device
entry point the header declares, and compares the two when it runs, after every test module has been imported.  The table the modules
look up by name (their global CASES) becomes a NEW list, the old one followed by these cases; the old list object, which their
parametrised tests were built from, stays as it is.  The arena's size was fixed before the cases were added: they lie inside it
(checked below).

The call refuses operands whose spans meet, so one operand of a case is far -- D, or the order, int32 entries in a window of
ncols / 2 words per member, its batch stride twice the window's in entries -- and the other is compact below it; pivots, rank and done
are small arrays outside the arena.  One shape per path, requests drawn on the device."""
import numpy as np
import pytest
import torch

import exchange_cases as xc
import far_arena as fa
import order_cases as oc
import test_far_arena_cpu as table_checks
import test_gpu_far_operands as far
from far_arena import BATCH, BS_EVEN, BS_ODD
from m4ri_amd.mzd import Mzd
from test_gpu_far_operands import arena  # noqa: F401  (the fixture: one arena for this module, as for that one)

ENTRY, PLAN = "m4ri_amd_pivot_exchange_batch_dev", "m4ri_amd_plan_pivot_exchange_batch"
STEPS, SEED = 5, 41
# (rows, columns, path, pivot_rows)
SHAPES = ((33, 64, 0, 32), (70, 130, 1, 60), (300, 4500, 2, 290))


def _reference(nr, nc, pr):
    """Per member: (the form, pivots, rank, order) before and (the form, pivots, order, done) after."""
    out = []
    for b in range(BATCH):
        order = oc.random_order(31, b, nc)
        S, rank, piv = oc.ech_order(Mzd.random(nr, nc, 3300 + b).to_bits(), order, 1, pr)
        out.append(((S, piv, rank, order), xc.exchange(S, piv, rank, pr, STEPS, seed=SEED, b=b, order=order)[:4]))
    return out


def _order_words(order):
    M = Mzd(1, 32 * len(order))
    M.valid_words()[0, :] = np.ascontiguousarray(order, dtype=np.int32).view(np.uint64)
    return M


def _cases():
    out = []
    for BS in (BS_ODD, BS_EVEN):
        s = far.sname(BS)
        for (nr, nc, p, pr) in SHAPES:
            for which in ("D", "O"):
                def run(ar, oracle, c, nr=nr, nc=nc, pr=pr):
                    ref = far.memo(("pivot_exchange", nr, nc, pr), lambda: _reference(nr, nc, pr))
                    pm = min(pr, nc)
                    pD = ar.place(c.wins["D"], [Mzd.from_bits(S) for (S, _p, _r, _o), _after in ref], dirty_tail=True)
                    pO = ar.place(c.wins["O"], [_order_words(o) for (_S, _p, _r, o), _after in ref])
                    pv = far._dev(np.concatenate([piv for (_S, piv, _r, _o), _after in ref]))
                    rk = far._dev(np.array([r for (_S, _p, r, _o), _after in ref]))
                    dn = torch.full((BATCH,), -7, dtype=torch.int32, device="cuda")
                    wD, wO = c.wins["D"], c.wins["O"]
                    far._call(ENTRY, pD.ptr, wD.stride, wD.bs, nr, nc, pr, pv.data_ptr(), rk.data_ptr(), BATCH, None, 0, STEPS, SEED, pO.ptr, 2 * wO.bs, nc,
                              dn.data_ptr(), None)
                    assert far._host(dn).tolist() == [did for _before, (_S, _p, _o, did) in ref] and min(far._host(dn)) > 0
                    assert np.array_equal(far._host(pv), np.concatenate([piv for _before, (_S, piv, _o, _d) in ref]))
                    assert far._host(pv).size == BATCH * pm
                    pD.check([Mzd.from_bits(S) for _before, (S, _p, _o, _d) in ref], "kept", "D")
                    assert np.array_equal(pO.fetch().view(np.int32).reshape(BATCH, nc), np.stack([o for _before, (_S, _p, o, _d) in ref]))
                out.append(far.Case(f"pivot_exchange_batch-{s}-{nr}x{nc}-path{p}-far:{which}", ENTRY, "batch", BS, (nr, nc), f"path{p}: {PLAN}",
                                    far.lay(BS, (which,), D=(nr, nc), O=(1, 32 * nc)), (which,), run, plan=(PLAN, (nr, nc, STEPS), p)))
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


def test_the_reference_exchanges():
    """The members of the GPU cases, on the host: every member performs steps, so a far operand that is not reached shows."""
    for (nr, nc, _p, pr) in SHAPES[:2]:
        ref = far.memo(("pivot_exchange", nr, nc, pr), lambda: _reference(nr, nc, pr))
        assert all(after[3] > 0 and not np.array_equal(before[0], after[0]) and not np.array_equal(before[3], after[2]) for before, after in ref)


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_far_operands(case, arena, oracle):  # noqa: F811
    far.test_far_operands(case, arena, oracle)
