"""The batched small-matrix calls (include/m4ri_amd.h) at EVERY shape up to 64 x 64 -- where each takes its path 0, a wave per member,
lane i holding row i, and is made of predicates on the shape -- and at the first shapes across that boundary (a side of 65, 66, 127, 128
or 129 against every side up to 66 and 127 .. 129), five members of rotating kinds per shape, every comparison exact.  The cases, the
arenas, the expectations (the oracle for the eliminations, NumPy for products and transposes) and the comparison are
tests/sweep_cases.py, pinned by tests/test_sweep_cases_cpu.py; here an arena per operand and row count is uploaded, every shape of it
launched, and everything downloaded once and compared whole: the valid bits, and that nothing outside them was written.  Most of the
time is the oracle's and NumPy's: on an MI355X host the slowest case takes 1.5 s (the permutation orders, m = 49 .. 64) and the file 41 s."""
import numpy as np
import pytest
import torch

import m4ri_amd
import sweep_cases as sc

pytestmark = pytest.mark.gpu
MUL_OVERRIDE, TRANSPOSE_OVERRIDE = "M4RI_AMD_MUL_SMALL_BATCH_PATH1_MAX", "M4RI_AMD_TRANSPOSE_BATCH_PATH1_MAX"
ROWS = sc.rows_of(sc.S0 + sc.S1)                   # one arena per row count: 69 shapes each
CHUNKS = [[r for r in ROWS if lo <= r[0][0] <= hi] for lo, hi in ((1, 16), (17, 32), (33, 48), (49, 64), (65, 129))]
IDS = ["m1-16", "m17-32", "m33-48", "m49-64", "m65-129"]
BEYOND = set(sc.S1)
_stopped = []


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    assert m4ri_amd.lib().m4ri_amd_device_count() >= 1, "no HIP device visible: the gpu tests have nothing to run on"
    m4ri_amd.init(0)
    torch.cuda.set_device(0)


@pytest.fixture(autouse=True)
def _nothing_more_after_a_failed_launch():
    if _stopped:
        pytest.fail(f"no further GPU work after {_stopped[0]}")


def _run(fn, job):
    """Upload the job's arenas, launch every shape, synchronise and download once; the failures as sweep_cases names them.  A launch
    that returns an error, or a failed synchronisation, raises, and no test of this file touches the GPU after it."""
    fails = []
    try:
        dev = {name: torch.from_numpy(h.view(np.int64) if h.dtype == np.uint64 else h).cuda() for name, h in job.bufs.items()}
        torch.cuda.synchronize()
        for key, args, error in job.launches:
            args = [dev[a.name].data_ptr() + dev[a.name].element_size() * a.off if isinstance(a, sc.Ptr) else a for a in args]
            if error is None:
                fn(*args)
                continue
            try:   # a shape the call has to refuse before it launches anything
                fn(*args)
                fails.append((key, f"{key} was not refused"))
            except RuntimeError as e:
                if str(error) not in str(e):
                    raise
        torch.cuda.synchronize()
        got = {name: t.cpu().numpy().view(job.bufs[name].dtype) for name, t in dev.items()}
    except BaseException as e:
        _stopped.append(f"{job.call} ({job.flags}): {e!r}")
        raise
    return fails + job.failures(got)


def _sweep(fn, jobs):
    fails, shapes, job = [], 0, None
    for job in jobs:
        fails += _run(fn, job)
        shapes += len(job.launches)
    sc.verdict(job.call, job.flags, fails, shapes)


@pytest.mark.parametrize("rows", CHUNKS, ids=IDS)
@pytest.mark.parametrize("full", [0, 1])
def test_echelonize_batch(oracle, rows, full):
    """Words, rank and pivots with their -1 tail."""
    _sweep(m4ri_amd.echelonize_batch_dev, (sc.ech_job(oracle, r, full) for r in rows))


@pytest.mark.parametrize("rows", CHUNKS, ids=IDS)
@pytest.mark.parametrize("full", [0, 1])
def test_echelonize_order_batch_natural_order_in_place(oracle, rows, full):
    """order = NULL, olen = ncols, pivot_rows = nrows, D == A: what the sweep above expects, bit for bit."""
    _sweep(m4ri_amd.echelonize_order_batch_dev, (sc.ech_job(oracle, r, full, order=True) for r in rows))


@pytest.mark.parametrize("rows", CHUNKS, ids=IDS)
def test_echelonize_order_batch_permutation_orders(rows):
    """A seeded permutation per member, out of place, full = 1, against the NumPy rule of tests/order_cases.py."""
    _sweep(m4ri_amd.echelonize_order_batch_dev, (sc.order_job(r) for r in rows))


@pytest.mark.parametrize("rows", CHUNKS, ids=IDS)
@pytest.mark.parametrize("pluq", [0, 1])
def test_ple_batch(oracle, rows, pluq):
    """Words, P, Q, rank and the entries behind each array; for PLUQ up to 64 x 64 also P L U Q = A of member 0 without the oracle."""
    _sweep(m4ri_amd.ple_batch_dev, (sc.ple_job(oracle, r, pluq) for r in rows))


@pytest.mark.parametrize("rows", CHUNKS, ids=IDS)
def test_solve_left_batch(oracle, rows):
    _sweep(m4ri_amd.solve_left_batch_dev, (sc.solve_job(oracle, r) for r in rows))


@pytest.mark.parametrize("inplace", [False, True], ids=["out_of_place", "in_place"])
def test_inv_batch(oracle, inplace):
    _sweep(m4ri_amd.inv_batch_dev, (sc.inv_job(oracle, [n], inplace) for n in sc.SQUARES))


@pytest.mark.parametrize("rows", CHUNKS, ids=IDS)
def test_kernel_left_batch(oracle, rows):
    _sweep(m4ri_amd.kernel_left_batch_dev, (sc.kernel_job(oracle, r) for r in rows))


@pytest.mark.parametrize("rows", CHUNKS, ids=IDS)
def test_pluq_solve_left_batch(oracle, rows):
    """Fed the oracle's decomposition, so that a fault of ple_batch_dev neither hides nor fakes one here."""
    _sweep(m4ri_amd.pluq_solve_left_batch_dev, (sc.pluq_solve_job(oracle, r) for r in rows))


def test_pluq_solve_left_batch_one_decomposition_for_all(oracle):
    """a_bs = 0 on the squares of the domain."""
    squares = [s for s in sc.S0 + sc.S1 if s[0] == s[1]]
    _sweep(m4ri_amd.pluq_solve_left_batch_dev, (sc.pluq_solve_job(oracle, [s], shared=True) for s in squares))


def _pairs(rows):
    """What the product sweeps need to know about the shapes beyond 64: the route there depends on a measured bound, so it is set to
    128 and only the results are compared; a side of 129 is then forwarded -- or refused when an operand is transposed."""
    return [dict(pairs=r, results_only=BEYOND & set(r)) for r in rows]


@pytest.mark.parametrize("rows", CHUNKS, ids=IDS)
@pytest.mark.parametrize("add", [0, 1])
@pytest.mark.parametrize("plane", sc.PLANES)
def test_mul_small_batch(monkeypatch, plane, add, rows):
    monkeypatch.setenv(MUL_OVERRIDE, "128")   # read per call
    _sweep(m4ri_amd.mul_small_batch_dev, (sc.mul_job(plane, add=add, **kw) for kw in _pairs(rows)))


@pytest.mark.parametrize("rows", CHUNKS, ids=IDS)
@pytest.mark.parametrize("add", [0, 1])
@pytest.mark.parametrize("plane,op", [("ml", sc.NT), ("ln", sc.TN), ("mn", sc.TT)], ids=["NT", "TN", "TT"])
def test_mul_small_batch_op(monkeypatch, plane, op, add, rows):
    """With a transposed operand nothing is forwarded: every word of C's arena is compared at every shape the bound of 128 admits,
    and a shape with a side of 129 has to be refused (801) with nothing written."""
    monkeypatch.setenv(MUL_OVERRIDE, "128")
    _sweep(m4ri_amd.mul_small_batch_op_dev,
           (sc.mul_job(plane, r, add, op, refused={p for p in r if max(sc.triple(plane, *p)) > 128}) for r in rows))


@pytest.mark.parametrize("rows", CHUNKS, ids=IDS)
def test_transpose_batch(monkeypatch, rows):
    monkeypatch.setenv(TRANSPOSE_OVERRIDE, "1024")   # tests/test_gpu_transpose_batch.py: the register paths whatever the bound is
    _sweep(m4ri_amd.transpose_batch_dev, (sc.transpose_job(r) for r in rows))


def test_transpose_batch_in_place():
    _sweep(m4ri_amd.transpose_batch_dev, (sc.transpose_job([(n, n)], inplace=True) for n in sc.SQUARES))
