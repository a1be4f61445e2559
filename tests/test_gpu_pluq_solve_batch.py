"""m4ri_amd_pluq_solve_left_batch_dev (include/m4ri_amd.h, ple_batch.hip): factor a batch once with m4ri_amd_ple_batch_dev(pluq = 1),
then solve A_b X_b = B_b from the stored factors, on all three paths of m4ri_amd_plan_pluq_solve_batch.  Status and every byte of B
against m4ri_amd_solve_left_batch_dev on the original members and the same dirty B, against the oracle's gf2o_pluq_solve_left with the
check on (pinned to mzd_pluq_solve_left by tests/test_solve_oracle.py) on the oracle's own decomposition, and A X = B in NumPy;
inconsistent members' B untouched; the factors, P, Q, rank and every frame unchanged."""
import numpy as np
import pytest
import torch

import m4ri_amd
from m4ri_amd.mzd import Mzd
from test_gpu_ple_batch import _bits
from test_gpu_solve_batch import _solve_case, _system
from test_ple_oracle import _make

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    assert m4ri_amd.lib().m4ri_amd_device_count() >= 1, "no HIP device visible: the gpu tests have nothing to run on"
    m4ri_amd.init(0)
    torch.cuda.set_device(0)


def _w(n):
    return (n + 63) // 64


def _systems(oracle, m, n, k, batch, seed, shared, consistent_only):
    """test_gpu_solve_batch's members: two consistent ones (B = A X0), then a random B on a low-rank A, and so on; consistent_only
    makes the third kind consistent too.  shared: one low-rank A for all."""
    systems = [_system(oracle, m, n, k, (b if b % 3 != 2 else b - 1) if consistent_only else b, seed + 11 * b) for b in range(batch)]
    if shared:
        A0 = _make("lowrank", m, n, seed)
        for b in range(batch):
            B = systems[b][1]
            if b % 3 != 2 or consistent_only:
                B.valid_words()[:m] = oracle.mul(None, A0, Mzd.random(n, k, seed + 11 * b + 1), 0).valid_words()
            systems[b] = (A0, B)
    return systems


def _run(oracle, m, n, k, batch, seed, path=None, shared=False, consistent_only=False, stream=None, **layout):
    if path is not None:
        assert m4ri_amd.plan_pluq_solve_batch(m, n, k) == path
    R, nf = max(m, n), 1 if shared else batch
    systems = _systems(oracle, m, n, k, batch, seed, shared, consistent_only)
    c = _solve_case(oracle, m, n, k, batch, seed, shared=shared, systems=systems, **layout)
    status = c["status"]
    # no vacuous case: some member is solved, and the mixed cases have a member without a solution
    assert (status == 0).any()
    assert consistent_only or batch < 3 or (status == -1).any()
    a_bs_f = c["a_bs"] if not shared else m * c["a_stride"] + 3
    tA = torch.from_numpy(c["hA"].view(np.int64).copy()).cuda()       # the original members, for the one-call solve
    tF = tA.clone()                                                    # decomposed in place
    tP = torch.full((nf * m + 1,), -7, dtype=torch.int32, device="cuda")
    tQ = torch.full((nf * n + 1,), -7, dtype=torch.int32, device="cuda")
    tr = torch.full((nf + 1,), -7, dtype=torch.int32, device="cuda")
    tB1 = torch.from_numpy(c["hB"].view(np.int64).copy()).cuda()
    tB2 = tB1.clone()
    ts1 = torch.full((batch + 1,), -7, dtype=torch.int32, device="cuda")
    ts2 = ts1.clone()
    torch.cuda.synchronize()
    s = stream.cuda_stream if stream is not None else 0
    m4ri_amd.ple_batch_dev(tF.data_ptr(), c["a_stride"], a_bs_f, m, n, nf, True, tP.data_ptr(), tQ.data_ptr(), tr.data_ptr(), s)
    (stream.synchronize if stream is not None else torch.cuda.synchronize)()
    before = [x.clone() for x in (tF, tP, tQ, tr)]
    torch.cuda.synchronize()
    m4ri_amd.pluq_solve_left_batch_dev(tF.data_ptr(), c["a_stride"], c["a_bs"], m, n, tr.data_ptr(), tP.data_ptr(), tQ.data_ptr(),
                                       tB1.data_ptr(), c["b_stride"], c["b_bs"], k, batch, ts1.data_ptr(), s)
    (stream.synchronize if stream is not None else torch.cuda.synchronize)()
    m4ri_amd.solve_left_batch_dev(tA.data_ptr(), c["a_stride"], c["a_bs"], m, n, tB2.data_ptr(), c["b_stride"], c["b_bs"], k, batch,
                                  ts2.data_ptr())
    torch.cuda.synchronize()
    got, one_call = tB1.cpu().numpy().view(np.uint64), tB2.cpu().numpy().view(np.uint64)
    st = ts1.cpu().numpy()
    # (a) the same status and the same bytes as the one-call solve
    assert np.array_equal(st, ts2.cpu().numpy()) and st[batch] == -7
    assert np.array_equal(st[:batch], status)
    bad = np.flatnonzero(got != one_call)
    assert bad.size == 0, f"{bad.size} words of B differ from solve_left_batch_dev, first at {bad[:5]} (member {bad[0] // c['b_bs']})"
    # (d), and the frame of B: only the valid bits of solved members changed (exp comes from the oracle's gf2o_solve_left)
    assert np.array_equal(got, c["exp"])
    # (e) the factors, P, Q and rank as the decomposition left them
    for x, y in zip((tF, tP, tQ, tr), before):
        assert torch.equal(x, y), "the solve wrote into the decomposition"
    assert (tP[nf * m:] == -7).all() and (tQ[nf * n:] == -7).all() and (tr[nf:] == -7).all()
    mask = np.full(_w(k), ~np.uint64(0), np.uint64)
    if k % 64:
        mask[-1] = np.uint64((1 << (k % 64)) - 1)
    for b, (A, B) in enumerate(systems):
        if status[b] or not (m and n and k) or (b >= 4 and R > 300):
            continue
        mine = got[b * c["b_bs"] + np.arange(R)[:, None] * c["b_stride"] + np.arange(_w(k))[None, :]] & mask
        # (b) the oracle's solve from the oracle's own decomposition
        F, X = A.copy(), B.copy()
        r, P, Q = oracle.ple(F, pluq=True)
        assert oracle.pluq_solve_left(F, r, P, Q, X, True) == 0
        assert np.array_equal(mine, X.valid_words()), f"member {b} differs from gf2o_pluq_solve_left"
        # (c) A X = B, the rows of X behind n zero
        Xb = _bits(mine, k)
        AX = np.rint(A.to_bits().astype(np.float32) @ Xb[:n].astype(np.float32)).astype(np.int64) & 1  # sums up to n < 2^24: exact
        assert np.array_equal(AX.astype(np.uint8), B.to_bits()[:m]), f"A X != B for member {b}"
        assert not Xb[n:].any()
    return c


# (m, n, k): m < n, m = n, m > n; k = 1, 64, 65, 200
PATH0 = [(40, 50, 1), (64, 64, 64), (63, 40, 37), (5, 5, 3), (30, 64, 17), (64, 20, 64)]
PATH1 = [(65, 63, 65), (63, 65, 64), (100, 100, 200), (200, 70, 65), (70, 200, 200), (300, 300, 64), (300, 300, 1), (513, 511, 200),
         (1100, 1100, 130)]
PATH2 = [(1100, 900, 1300), (900, 1100, 1300), (1000, 1000, 1300)]


@pytest.mark.parametrize("m,n,k", PATH0)
@pytest.mark.parametrize("batch", [37, 1001])
def test_wave_path(oracle, m, n, k, batch):
    _run(oracle, m, n, k, batch, 100 + m + n + k, path=0)


@pytest.mark.parametrize("m,n,k", PATH1)
def test_lds_path(oracle, m, n, k):
    _run(oracle, m, n, k, 7, 200 + m + n + k, path=1)


@pytest.mark.parametrize("m,n,k", PATH2)
def test_one_by_one_path(oracle, m, n, k):
    _run(oracle, m, n, k, 3, 300 + m + n + k, path=2)


@pytest.mark.parametrize("m,n,k", [(64, 64, 64), (200, 70, 65), (900, 1100, 1300)])
def test_consistent_members_only(oracle, m, n, k):
    c = _run(oracle, m, n, k, 5, 350 + m, consistent_only=True)
    assert (c["status"] == 0).all()


@pytest.mark.parametrize("m,n,k", [(33, 50, 20), (64, 64, 64), (200, 450, 70), (1100, 900, 1300)])
@pytest.mark.parametrize("layout", ["tight", "loose"])
def test_frames(oracle, m, n, k, layout):
    R = max(m, n)
    if layout == "tight":
        kw = dict(a_stride=_w(n), a_bs=m * _w(n), b_stride=_w(k), b_bs=R * _w(k))
    else:
        kw = dict(a_stride=_w(n) + 3, a_bs=m * (_w(n) + 3) + 17, b_stride=_w(k) + 4, b_bs=R * (_w(k) + 4) + 9)
    _run(oracle, m, n, k, 3, 400 + m, **kw)


@pytest.mark.parametrize("m,n,k", [(40, 64, 30), (300, 300, 64), (1100, 900, 1300)])
def test_shared_decomposition(oracle, m, n, k):
    """a_bs = 0: one decomposition (A, rank[0], the first m entries of P, the first n of Q) for every member."""
    _run(oracle, m, n, k, 6, 500 + m, shared=True)


@pytest.mark.parametrize("m,n,k", [(0, 5, 3), (5, 0, 3), (5, 5, 0), (0, 0, 0), (0, 100, 70), (100, 0, 70), (100, 100, 0), (0, 30000, 64),
                                   (30000, 0, 64)])
def test_degenerate_sizes(oracle, m, n, k):
    """An empty A has a solution (X = 0) only for B = 0; k = 0 always has one."""
    R = max(m, n)
    for zero_b in (True, False):
        A = Mzd.random(m, n, 4) if m and n else Mzd(m, n)
        B = Mzd(R, k) if zero_b or not (R and k) else Mzd.random(R, k, 5)
        c = _solve_case(oracle, m, n, k, 1, 6, systems=[(A, B)])
        tF = torch.from_numpy(c["hA"].view(np.int64).copy()).cuda()
        tB = torch.from_numpy(c["hB"].view(np.int64).copy()).cuda()
        tP = torch.zeros(max(1, m), dtype=torch.int32, device="cuda")
        tQ = torch.zeros(max(1, n), dtype=torch.int32, device="cuda")
        tr = torch.full((1,), -7, dtype=torch.int32, device="cuda")
        ts = torch.full((1,), -7, dtype=torch.int32, device="cuda")
        m4ri_amd.ple_batch_dev(tF.data_ptr(), c["a_stride"], c["a_bs"], m, n, 1, True, tP.data_ptr(), tQ.data_ptr(), tr.data_ptr())
        m4ri_amd.pluq_solve_left_batch_dev(tF.data_ptr(), c["a_stride"], c["a_bs"], m, n, tr.data_ptr(), tP.data_ptr(), tQ.data_ptr(),
                                           tB.data_ptr(), c["b_stride"], c["b_bs"], k, 1, ts.data_ptr())
        torch.cuda.synchronize()
        assert ts.cpu().tolist() == c["status"].tolist(), (m, n, k, zero_b)
        assert np.array_equal(tB.cpu().numpy().view(np.uint64), c["exp"])


def test_non_default_stream(oracle):
    s = torch.cuda.Stream()
    _run(oracle, 64, 64, 64, 300, 600, stream=s)
    _run(oracle, 256, 256, 100, 40, 700, stream=s)


def test_captured_into_a_graph(oracle):
    """Paths 0 and 1 are one launch each and capturable (path 2 blocks and is never captured): a shape of each captured on one stream,
    one chain, on decompositions made before the capture -- nothing runs, B and status keep their dirt -- then replayed once and
    compared with the oracle's gf2o_solve_left.  _run's ordinary call of each kernel comes first: a process's first call sets function
    attributes, which is not what this test is about."""
    cases = []
    for path, (m, n, k, batch) in enumerate([(40, 50, 17, 6), (100, 70, 130, 6)]):
        _run(oracle, m, n, k, batch, 800 + m, path=path)
        c = _solve_case(oracle, m, n, k, batch, 810 + m, systems=_systems(oracle, m, n, k, batch, 810 + m, False, False))
        assert (c["status"] == 0).any() and (c["status"] == -1).any() and not np.array_equal(c["exp"], c["hB"])
        c["tF"] = torch.from_numpy(c["hA"].view(np.int64).copy()).cuda()
        c["tB"] = torch.from_numpy(c["hB"].view(np.int64).copy()).cuda()
        c["tP"], c["tQ"], c["tr"], c["ts"] = (torch.full((x,), -7, dtype=torch.int32, device="cuda") for x in (batch * m, batch * n, batch, batch))
        m4ri_amd.ple_batch_dev(c["tF"].data_ptr(), c["a_stride"], c["a_bs"], m, n, batch, True, c["tP"].data_ptr(), c["tQ"].data_ptr(), c["tr"].data_ptr())
        cases.append(c)
    torch.cuda.synchronize()
    before = [[c[x].clone() for x in ("tF", "tP", "tQ", "tr")] for c in cases]
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for c in cases:
            m4ri_amd.pluq_solve_left_batch_dev(c["tF"].data_ptr(), c["a_stride"], c["a_bs"], c["m"], c["n"], c["tr"].data_ptr(), c["tP"].data_ptr(),
                                               c["tQ"].data_ptr(), c["tB"].data_ptr(), c["b_stride"], c["b_bs"], c["k"], c["batch"], c["ts"].data_ptr(),
                                               torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    for c in cases:
        assert np.array_equal(c["tB"].cpu().numpy().view(np.uint64), c["hB"]) and (c["ts"] == -7).all(), (c["m"], c["n"])
    g.replay()
    torch.cuda.synchronize()
    for c, kept in zip(cases, before):
        assert np.array_equal(c["ts"].cpu().numpy(), c["status"]), (c["m"], c["n"])
        assert np.array_equal(c["tB"].cpu().numpy().view(np.uint64), c["exp"]), (c["m"], c["n"])
        assert all(torch.equal(c[x], y) for x, y in zip(("tF", "tP", "tQ", "tr"), kept)), "the solve wrote into the decomposition"
