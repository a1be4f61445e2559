"""m4ri_amd_echelonize_order_batch_dev and m4ri_amd_random_orders_batch_dev on operands whose batch members lie 5 GiB and more apart:
the cases of tests/test_gpu_far_operands.py for these two entry points, built with that module's own pieces (Case, lay, the arena) and
run the same way, as tests/test_gpu_far_row_sums.py does for its entry point.

The cases are ADDED to that module's table when this module is imported: tests/test_far_arena_cpu.py holds the table to every device
entry point the header declares, and compares the two when it runs, after every test module has been imported.  The table the modules
look up by name (their global CASES) becomes a NEW list, the old one followed by these cases; the old list object, which their
parametrised tests were built from, stays as it is.  A run of tests/test_far_arena_cpu.py alone, without this module, reports the
entry points as missing from the table; a run of the suite does not.  The arena's size was fixed before the cases were added: they lie
inside it (checked below).

The call refuses operands whose spans meet, so one operand of a case is far (D, or A, or the one operand of a call in place) and the
other is compact below it.  The orders of m4ri_amd_random_orders_batch_dev are int32: a window of n / 2 words per member, its batch
stride twice the window's in entries."""
import numpy as np
import pytest
import torch

import far_arena as fa
import order_cases as oc
import test_far_arena_cpu as table_checks
import test_gpu_far_operands as far
from far_arena import BATCH, BS_EVEN, BS_ODD
from m4ri_amd.mzd import Mzd
from test_gpu_far_operands import arena  # noqa: F401  (the fixture: one arena for this module, as for that one)

ENTRY, ENTRY_RO = "m4ri_amd_echelonize_order_batch_dev", "m4ri_amd_random_orders_batch_dev"
PLAN = "m4ri_amd_plan_echelonize_order_batch"
# (rows, columns, path, pivot_rows, full, which operand is far: D, A, or the one of a call in place; one shared A)
SHAPES = ((33, 64, 0, 32, 1, "D", False), (70, 130, 1, 70, 0, "A", False), (70, 130, 1, 69, 1, "D", True), (300, 4500, 2, 300, 1, "inplace", False))
RO_N = 130


def _cases():
    out = []
    for BS in (BS_ODD, BS_EVEN):
        s = far.sname(BS)
        for (nr, nc, p, pr, full, which, shared) in SHAPES:
            def run(ar, oracle, c, nr=nr, nc=nc, pr=pr, full=full, which=which, shared=shared):
                Ab = far.members(lambda b: Mzd.random(nr, nc, 3100 + (0 if shared else b)).to_bits())
                orders = np.stack([oc.random_order(31, b, nc) for b in range(BATCH)])
                want = far.memo(("ech_order", nr, nc, pr, full, shared), lambda: [oc.ech_order(A, o, full, pr) for A, o in zip(Ab, orders)])
                pm = min(pr, nc)
                pA = ar.place(c.wins["A"], [Mzd.from_bits(x) for x in (Ab[:1] if shared else Ab)], dirty_tail=True)
                pD = pA if which == "inplace" else ar.place(c.wins["D"], far.members(lambda b: Mzd.random(nr, nc, 3150 + b)), dirty_tail=True)
                wA, wD = c.wins["A"], c.wins["A" if which == "inplace" else "D"]
                dO = far._dev(orders.reshape(-1))
                rk = torch.full((BATCH,), -7, dtype=torch.int32, device="cuda")
                pv = torch.full((BATCH * pm,), -7, dtype=torch.int32, device="cuda")
                far._call(ENTRY, pD.ptr, wD.stride, wD.bs, pA.ptr, wA.stride, wA.bs, nr, nc, pr, dO.data_ptr(), nc, nc, BATCH, full, rk.data_ptr(),
                          pv.data_ptr(), None)
                assert far._host(rk).tolist() == [r for _, r, _ in want]
                assert np.array_equal(far._host(pv), np.concatenate([piv for _, _, piv in want]))
                pD.check([Mzd.from_bits(S) for S, _, _ in want], "kept", "D")
                if which != "inplace":
                    pA.check_unchanged("A")
            names = ("A",) if which == "inplace" else (which,)
            ops = dict(A=(nr, nc, "shared") if shared else (nr, nc)) if which == "inplace" else dict(D=(nr, nc), A=(nr, nc, "shared") if shared else (nr, nc))
            out.append(far.Case(f"echelonize_order_batch-{s}-{nr}x{nc}-path{p}-far:{which}" + ("-shared-A" if shared else ""), ENTRY, "batch", BS, (nr, nc),
                                f"path{p}: {PLAN}", far.lay(BS, names, **ops), names, run, plan=(PLAN, (nr, nc), p)))

        def run_orders(ar, oracle, c):
            p = ar.place(c.wins["O"], far.members(lambda b: Mzd.random(1, 32 * RO_N, 3190 + b)))
            far._call(ENTRY_RO, p.ptr, 2 * c.wins["O"].bs, RO_N, BATCH, 99, None)
            got = p.fetch().view(np.int32).reshape(BATCH, RO_N)
            assert np.array_equal(got, np.stack([oc.random_order(99, b, RO_N) for b in range(BATCH)]))
        out.append(far.Case(f"random_orders_batch-{s}-n{RO_N}", ENTRY_RO, "batch", BS, (RO_N,), "one workgroup per member", {"O": far.M_(0, 1, 32 * RO_N, BS)},
                            ("O",), run_orders))
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


def test_the_table_names_the_entry_points():
    assert {ENTRY, ENTRY_RO} <= {c.entry for c in far.CASES} and not {ENTRY, ENTRY_RO} & set(far.LEFT_OUT)
    table_checks.test_every_device_entry_point_has_a_far_case_or_a_reason()
    table_checks.test_both_parities_of_every_far_stride()


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_far_operands(case, arena, oracle):  # noqa: F811
    far.test_far_operands(case, arena, oracle)
