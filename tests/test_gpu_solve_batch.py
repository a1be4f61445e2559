"""m4ri_amd_solve_left_batch_dev and m4ri_amd_inv_batch_dev (include/m4ri_amd.h, solve_batch.hip): `batch` independent systems
A_b X_b = B_b and inverses in one call, on all three paths of m4ri_amd_plan_solve_batch.  Solve: the status from the ranks of A and
of [A | B] (zero-padded to max(m, n) rows), X of the consistent members against the oracle's gf2o_solve_left (pinned to
mzd_solve_left by tests/test_solve_oracle.py) and A X = B, inconsistent members' B untouched.  Inverse: against gf2o_inv (pinned
to mzd_inv_m4ri), singular members included.  Every buffer has dirty padding words, tail bits and gaps between members that must
come out unchanged, and A must come out unchanged."""
import ctypes

import numpy as np
import pytest
import torch

import m4ri_amd
from m4ri_amd.mzd import Mzd
from test_gpu_echelonize_batch import _pack
from test_ple_oracle import _defects, _make

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    assert m4ri_amd.lib().m4ri_amd_device_count() >= 1, "no HIP device visible: the gpu tests have nothing to run on"
    m4ri_amd.init(0)
    torch.cuda.set_device(0)


def _w(n):
    return (n + 63) // 64


def _rank(oracle, M):
    return oracle.echelonize(M.copy(), 0) if M.nrows and M.ncols else 0


def _augmented(A, B):
    """[A | B] with A padded by zero rows to B's row count."""
    bits = np.zeros((B.nrows, A.ncols + B.ncols), dtype=np.uint8)
    if A.nrows and A.ncols:
        bits[: A.nrows, : A.ncols] = A.to_bits()
    if B.nrows and B.ncols:
        bits[:, A.ncols:] = B.to_bits()
    return Mzd.from_bits(bits)


def _system(oracle, m, n, k, b, seed):
    """Member b: consistent (B = A X) for b % 3 != 2, else a random B on a low-rank A (inconsistent unless it happens to fit)."""
    R = max(m, n)
    consistent = b % 3 != 2
    kind = ("random", "zerocols", "lowrank", "defects")[b % 4] if consistent else "lowrank"
    if m == 0 or n == 0:
        A = Mzd(m, n)
    elif kind == "defects":
        A = _defects(m, n, seed, m // 8, m // 16) if n >= 4 else Mzd.random(m, n, seed)
    else:
        A = _make(kind, m, n, seed)
    B = Mzd(R, k)
    if m and k:
        if consistent:
            if n:
                B.valid_words()[:m] = oracle.mul(None, A, Mzd.random(n, k, seed + 1), 0).valid_words()
        else:
            B.valid_words()[:m] = Mzd.random(m, k, seed + 2).valid_words()
    return A, B


def _expect_solve(oracle, A, B):
    """(status, rank, the B the call must leave)."""
    m, n, k = A.nrows, A.ncols, B.ncols
    ra = _rank(oracle, A)
    status = 0 if _rank(oracle, _augmented(A, B)) == ra else -1
    if status or not k:
        return status, ra, B
    if m and n:
        Ao, X = A.copy(), B.copy()
        assert oracle.solve_left(Ao, X, True) == 0
        top = Mzd.from_bits(X.to_bits()[:n])
        assert np.array_equal(oracle.mul(None, A, top, 0).valid_words(), B.valid_words()[:m]), "oracle: A X != B"
        return 0, ra, X
    return 0, ra, Mzd(B.nrows, k)  # A = 0: consistent only for B = 0, and X = 0


def _solve_case(oracle, m, n, k, batch, seed, a_stride=None, a_bs=None, b_stride=None, b_bs=None, shared=False, systems=None):
    R = max(m, n)
    a_stride = _w(n) + 1 if a_stride is None else a_stride
    b_stride = _w(k) + 2 if b_stride is None else b_stride
    a_bs = (0 if shared else m * a_stride + 3) if a_bs is None else a_bs
    b_bs = R * b_stride + 5 if b_bs is None else b_bs
    if systems is None:
        systems = [_system(oracle, m, n, k, b, seed + 11 * b) for b in range(batch)]
        if shared:  # a low-rank A, so that random right-hand sides are inconsistent
            A0 = _make("lowrank", m, n, seed) if m and n else Mzd(m, n)
            for b in range(batch):  # the B of consistent members rebuilt on the shared A
                _, B = _system(oracle, m, n, k, b, seed + 11 * b)
                if b % 3 != 2 and m and n and k:
                    B.valid_words()[:m] = oracle.mul(None, A0, Mzd.random(n, k, seed + 11 * b + 1), 0).valid_words()
                systems[b] = (A0, B)
    As = [systems[0][0]] if shared else [s[0] for s in systems]
    hA, _, _ = _pack(As, m, n, a_stride, a_bs, seed)
    hB, idx, valid = _pack([s[1] for s in systems], R, k, b_stride, b_bs, seed + 1)
    exp = hB.copy()
    want_status, want_rank = [], []
    for b, (A, B) in enumerate(systems):
        st, r, X = _expect_solve(oracle, A, B)
        want_status.append(st)
        want_rank.append(r)
        if R and k:
            exp[idx[b]] = (hB[idx[b]] & ~valid) | (X.valid_words() & valid)
    return dict(m=m, n=n, k=k, batch=batch, a_stride=a_stride, a_bs=a_bs, b_stride=b_stride, b_bs=b_bs, hA=hA, hB=hB, exp=exp,
                status=np.array(want_status, np.int32), rank=np.array(want_rank, np.int32))


def _upload(c):
    c["tA"] = torch.from_numpy(c["hA"].view(np.int64).copy()).cuda()
    c["tB"] = torch.from_numpy(c["hB"].view(np.int64).copy()).cuda()
    c["ts"] = torch.full((max(1, c["batch"]),), -7, dtype=torch.int32, device="cuda")
    c["tr"] = torch.full((max(1, c["batch"]),), -7, dtype=torch.int32, device="cuda")


def _launch(c, stream=0, rank=True):
    m4ri_amd.solve_left_batch_dev(c["tA"].data_ptr(), c["a_stride"], c["a_bs"], c["m"], c["n"], c["tB"].data_ptr(), c["b_stride"], c["b_bs"],
                                  c["k"], c["batch"], c["ts"].data_ptr(), c["tr"].data_ptr() if rank else 0, stream)


def _verify(c, rank=True):
    assert np.array_equal(c["tA"].cpu().numpy().view(np.uint64), c["hA"]), "A (or its frame) was written"
    got = c["tB"].cpu().numpy().view(np.uint64)
    bad = np.flatnonzero(got != c["exp"])
    assert bad.size == 0, f"{bad.size} words of B differ, first at {bad[:5]} (member {bad[0] // c['b_bs'] if c['b_bs'] else 0})"
    assert np.array_equal(c["ts"].cpu().numpy()[: c["batch"]], c["status"])
    if rank:
        assert np.array_equal(c["tr"].cpu().numpy()[: c["batch"]], c["rank"])
    else:
        assert (c["tr"].cpu().numpy() == -7).all()


def _run_solve(oracle, m, n, k, batch, seed, path=None, **kw):
    if path is not None:
        assert m4ri_amd.plan_solve_batch(m, n, k) == path
    c = _solve_case(oracle, m, n, k, batch, seed, **kw)
    assert (c["status"] == 0).any() and (batch < 3 or (c["status"] == -1).any()), "the batch should mix both kinds of member"
    _upload(c)
    torch.cuda.synchronize()
    _launch(c)
    torch.cuda.synchronize()
    _verify(c)
    return c


# (m, n, k): m < n, m = n, m > n; k = 1, not a multiple of 64, 64 or more
PATH0 = [(40, 50, 1), (64, 64, 64), (63, 40, 37), (5, 5, 3), (30, 64, 17), (64, 20, 64)]
PATH1 = [(65, 63, 10), (63, 65, 70), (100, 100, 130), (200, 70, 33), (70, 200, 129), (300, 300, 64), (300, 300, 1), (513, 511, 200)]
PATH2 = [(1100, 1000, 70), (900, 1100, 1), (1100, 1100, 130)]


@pytest.mark.parametrize("m,n,k", PATH0)
@pytest.mark.parametrize("batch", [37, 1000])
def test_solve_wave_path(oracle, m, n, k, batch):
    _run_solve(oracle, m, n, k, batch, 100 + m + n + k, path=0)


@pytest.mark.parametrize("m,n,k", PATH1)
def test_solve_lds_path(oracle, m, n, k):
    _run_solve(oracle, m, n, k, 7, 200 + m + n + k, path=1)


@pytest.mark.parametrize("m,n,k", PATH2)
def test_solve_one_by_one_path(oracle, m, n, k):
    _run_solve(oracle, m, n, k, 3, 300 + m + n + k, path=2)


@pytest.mark.parametrize("m,n,k", [(33, 50, 20), (64, 64, 64), (200, 450, 70), (1100, 1000, 70)])
@pytest.mark.parametrize("layout", ["tight", "loose"])
def test_solve_frame_and_null_rank(oracle, m, n, k, layout):
    """Tight: stride = width, members back to back; loose: padding words and gaps.  Every word outside the members' valid bits is
    random before the call and must be the same after it; rank = NULL is accepted and nothing is written for it."""
    R = max(m, n)
    if layout == "tight":
        kw = dict(a_stride=_w(n), a_bs=m * _w(n), b_stride=_w(k), b_bs=R * _w(k))
    else:
        kw = dict(a_stride=_w(n) + 3, a_bs=m * (_w(n) + 3) + 17, b_stride=_w(k) + 4, b_bs=R * (_w(k) + 4) + 9)
    c = _solve_case(oracle, m, n, k, 3, 400 + m, **kw)
    _upload(c)
    torch.cuda.synchronize()
    _launch(c, rank=False)
    torch.cuda.synchronize()
    _verify(c, rank=False)


@pytest.mark.parametrize("m,n,k", [(40, 64, 30), (300, 300, 64), (1100, 1000, 70)])
def test_solve_shared_a(oracle, m, n, k):
    """a_bs = 0: one A for every member."""
    _run_solve(oracle, m, n, k, 6, 500 + m, shared=True)


def _inv_member(oracle, n, b, seed):
    kind = b % 4
    if kind == 0:  # invertible: lower times upper unitriangular
        bits = np.tril(Mzd.random(n, n, seed).to_bits(), -1)
        np.fill_diagonal(bits, 1)
        L = Mzd.from_bits(bits)
        bits = np.triu(Mzd.random(n, n, seed + 1).to_bits(), 1)
        np.fill_diagonal(bits, 1)
        return oracle.mul(None, L, Mzd.from_bits(bits), 0)
    if kind == 1:
        return Mzd.random(n, n, seed)
    if kind == 2:  # singular: a repeated row (n >= 2)
        A = Mzd.random(n, n, seed)
        if n > 1:
            A.valid_words()[n // 2] = A.valid_words()[0]
        else:
            A.valid_words()[:] = 0
        return A
    return Mzd(n, n)


def _inv_case(oracle, n, batch, seed, inplace=False, layout="loose"):
    wn = _w(n)
    if layout == "tight":
        a_stride, a_bs = wn, n * wn
    else:
        a_stride, a_bs = wn + 2, n * (wn + 2) + 7
    b_stride, b_bs = (a_stride, a_bs) if inplace else (wn + 1, n * (wn + 1) + 3)
    members = [_inv_member(oracle, n, b, seed + 13 * b) for b in range(batch)]
    hA, idxA, valid = _pack(members, n, n, a_stride, a_bs, seed)
    hB, idxB, _ = (hA, idxA, valid) if inplace else _pack([Mzd(n, n)] * batch, n, n, b_stride, b_bs, seed + 1)
    exp = hB.copy()
    ranks = []
    for b, A in enumerate(members):
        exp[idxB[b]] = (hB[idxB[b]] & ~valid) | (oracle.inv(A).valid_words() & valid)
        ranks.append(_rank(oracle, A))
    return dict(n=n, batch=batch, a_stride=a_stride, a_bs=a_bs, b_stride=b_stride, b_bs=b_bs, hA=hA, hB=hB, exp=exp, members=members,
                rank=np.array(ranks, np.int32), inplace=inplace)


def _run_inv(oracle, n, batch, seed, path=None, inplace=False, layout="loose", stream=0, sync=True):
    if path is not None:
        assert m4ri_amd.plan_solve_batch(n, n, n) == path
    c = _inv_case(oracle, n, batch, seed, inplace, layout)
    tA = torch.from_numpy(c["hA"].view(np.int64).copy()).cuda()
    tB = tA if inplace else torch.from_numpy(c["hB"].view(np.int64).copy()).cuda()
    tr = torch.full((batch,), -7, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    m4ri_amd.inv_batch_dev(tB.data_ptr(), c["b_stride"], c["b_bs"], tA.data_ptr(), c["a_stride"], c["a_bs"], n, batch, tr.data_ptr(), stream)
    torch.cuda.synchronize()
    got = tB.cpu().numpy().view(np.uint64)
    bad = np.flatnonzero(got != c["exp"])
    assert bad.size == 0, f"{bad.size} words of Binv differ, first at {bad[:5]} (member {bad[0] // c['b_bs']})"
    if not inplace:
        assert np.array_equal(tA.cpu().numpy().view(np.uint64), c["hA"]), "A (or its frame) was written"
    assert np.array_equal(tr.cpu().numpy(), c["rank"])
    assert (c["rank"] == n).any() and (c["rank"] < n).any()
    return c, tA, tB


@pytest.mark.parametrize("n", [1, 5, 63, 64])
@pytest.mark.parametrize("batch", [8, 1001])
def test_inverse_wave_path(oracle, n, batch):
    _run_inv(oracle, n, batch, 600 + n, path=0)


@pytest.mark.parametrize("n", [65, 100, 256, 768])
def test_inverse_lds_path(oracle, n):
    _run_inv(oracle, n, 8, 700 + n, path=1)


@pytest.mark.parametrize("n", [769, 1000])
def test_inverse_one_by_one_path(oracle, n):
    _run_inv(oracle, n, 4, 800 + n, path=2)


@pytest.mark.parametrize("n", [40, 64, 200, 769])
@pytest.mark.parametrize("layout", ["tight", "loose"])
def test_inverse_in_place(oracle, n, layout):
    _run_inv(oracle, n, 4, 900 + n, inplace=True, layout=layout)


@pytest.mark.parametrize("n", [50, 300, 769])
def test_inverse_bit_identical_to_inv_dev(oracle, n):
    c, tA, tB = _run_inv(oracle, n, 4, 1000 + n)
    L = m4ri_amd.lib()
    wn = _w(n)
    for b, A in enumerate(c["members"]):
        dA = torch.from_numpy(A.valid_words().copy().view(np.int64)).cuda()
        dX = torch.zeros(n * wn, dtype=torch.int64, device="cuda")
        assert L.m4ri_amd_inv_dev(dX.data_ptr(), wn, dA.data_ptr(), wn, n, None) == 0
        torch.cuda.synchronize()
        got = tB.cpu().numpy().view(np.uint64)[b * c["b_bs"] + np.arange(n)[:, None] * c["b_stride"] + np.arange(wn)[None, :]]
        mask = np.full(wn, ~np.uint64(0), np.uint64)
        if n % 64:
            mask[-1] = np.uint64((1 << (n % 64)) - 1)
        assert np.array_equal(got & mask, dX.cpu().numpy().view(np.uint64).reshape(n, wn)), (n, b)


@pytest.mark.parametrize("m,n,k", [(40, 50, 30), (64, 64, 64), (200, 70, 33), (70, 200, 129), (1100, 1000, 70)])
def test_solve_bit_identical_to_solve_left_dev(oracle, m, n, k):
    """A random subset of the members through m4ri_amd_solve_left_dev, with both values of the check: the consistent ones give the
    same bits, the inconsistent ones -1 with the check on."""
    c = _run_solve(oracle, m, n, k, 9, 1100 + m + k)
    R, wa, wb = max(m, n), _w(n), _w(k)
    hA, exp = c["hA"], c["exp"]
    L = m4ri_amd.lib()
    rng = np.random.default_rng(m + n + k)
    for b in sorted(rng.choice(9, size=5, replace=False)):
        a_idx = b * c["a_bs"] + np.arange(m)[:, None] * c["a_stride"] + np.arange(wa)[None, :]
        b_idx = b * c["b_bs"] + np.arange(R)[:, None] * c["b_stride"] + np.arange(wb)[None, :]
        am = np.full(wa, ~np.uint64(0), np.uint64)
        bm = np.full(wb, ~np.uint64(0), np.uint64)
        if n % 64:
            am[-1] = np.uint64((1 << (n % 64)) - 1)
        if k % 64:
            bm[-1] = np.uint64((1 << (k % 64)) - 1)
        for check in (0, 1):
            dA = torch.from_numpy((hA[a_idx] & am).view(np.int64).copy()).cuda()
            dB = torch.from_numpy((c["hB"][b_idx] & bm).view(np.int64).copy()).cuda()
            ret = ctypes.c_int(7)
            assert L.m4ri_amd_solve_left_dev(dA.data_ptr(), wa, m, n, dB.data_ptr(), wb, R, k, 0, check, ctypes.byref(ret), None) == 0
            torch.cuda.synchronize()
            if c["status"][b] == 0:
                assert ret.value == 0
                assert np.array_equal(dB.cpu().numpy().view(np.uint64), exp[b_idx] & bm), (b, check)
            elif check:
                assert ret.value == -1, b


def test_b_row_m_divergence(oracle):
    """m < n: the batch call checks every padding row of B, so a non-zero row m alone makes the member -1 and leaves B untouched,
    while m4ri_amd_solve_left_dev (as _mzd_solve_left, which looks from row m + 1 on) still returns 0.  Documented in the header."""
    for m, n, k, path in [(30, 50, 20, 0), (100, 160, 70, 1), (900, 1100, 64, 2)]:
        assert m4ri_amd.plan_solve_batch(m, n, k) == path
        A = Mzd.random(m, n, 1)
        B = Mzd(n, k)
        B.valid_words()[:m] = oracle.mul(None, A, Mzd.random(n, k, 2), 0).valid_words()
        B.valid_words()[m, 0] = np.uint64(5)
        c = _solve_case(oracle, m, n, k, 1, 3, systems=[(A, B)])
        assert c["status"][0] == -1 and np.array_equal(c["exp"], c["hB"])
        _upload(c)
        torch.cuda.synchronize()
        _launch(c)
        torch.cuda.synchronize()
        _verify(c)
        dA = torch.from_numpy(A.valid_words().copy().view(np.int64)).cuda()
        dB = torch.from_numpy(B.valid_words().copy().view(np.int64)).cuda()
        ret = ctypes.c_int(7)
        assert m4ri_amd.lib().m4ri_amd_solve_left_dev(dA.data_ptr(), _w(n), m, n, dB.data_ptr(), _w(k), n, k, 0, 1, ctypes.byref(ret), None) == 0
        assert ret.value == 0, (m, n, k)


@pytest.mark.parametrize("m,n,k", [(0, 5, 3), (5, 0, 3), (5, 5, 0), (0, 0, 0), (0, 100, 70), (100, 0, 70), (100, 100, 0), (0, 3000, 64),
                                   (3000, 0, 64), (2000, 2000, 0)])
def test_solve_degenerate_sizes(oracle, m, n, k):
    R = max(m, n)
    for zero_b in (True, False):
        A = Mzd.random(m, n, 4) if m and n else Mzd(m, n)
        B = Mzd(R, k) if zero_b or not (R and k) else Mzd.random(R, k, 5)
        c = _solve_case(oracle, m, n, k, 1, 6, systems=[(A, B)])
        _upload(c)
        torch.cuda.synchronize()
        _launch(c)
        torch.cuda.synchronize()
        _verify(c)


def test_inverse_degenerate_sizes():
    h = np.arange(1, 65, dtype=np.int64)
    tA = torch.from_numpy(h).cuda()
    tr = torch.full((3,), -7, dtype=torch.int32, device="cuda")
    m4ri_amd.inv_batch_dev(tA.data_ptr(), 0, 0, tA.data_ptr(), 0, 0, 0, 3, tr.data_ptr())
    torch.cuda.synchronize()
    assert tr.cpu().tolist() == [0, 0, 0] and np.array_equal(tA.cpu().numpy(), h)


def test_two_streams(oracle):
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    c1 = _solve_case(oracle, 64, 64, 64, 300, 1200)
    c2 = _solve_case(oracle, 256, 256, 256, 40, 1300)
    ci = _inv_case(oracle, 200, 40, 1400)
    for c in (c1, c2):
        _upload(c)
    iA = torch.from_numpy(ci["hA"].view(np.int64).copy()).cuda()
    iB = torch.from_numpy(ci["hB"].view(np.int64).copy()).cuda()
    torch.cuda.synchronize()
    _launch(c1, s1.cuda_stream)
    _launch(c2, s2.cuda_stream)
    m4ri_amd.inv_batch_dev(iB.data_ptr(), ci["b_stride"], ci["b_bs"], iA.data_ptr(), ci["a_stride"], ci["a_bs"], 200, 40, 0, s1.cuda_stream)
    s1.synchronize()
    s2.synchronize()
    _verify(c1)
    _verify(c2)
    assert np.array_equal(iB.cpu().numpy().view(np.uint64), ci["exp"])


def test_captured_into_a_graph(oracle):
    """Paths 0 and 1 of the solve and of the inverse are one launch each and capturable (path 2 blocks and is never captured): a
    shape of each, solves and inverses in ONE graph on one stream, one chain -- nothing runs, B, Binv, status and rank keep their
    dirt -- then replayed once.  An ordinary call of each kernel comes first: a process's first call sets function attributes, which
    is not what this test is about."""
    solves, invs = [], []
    for path, (m, n, k, batch) in enumerate([(40, 50, 17, 6), (100, 70, 130, 6)]):
        _run_solve(oracle, m, n, k, batch, 1500 + m, path=path)
        c = _solve_case(oracle, m, n, k, batch, 1510 + m)
        assert (c["status"] == 0).any() and (c["status"] == -1).any() and not np.array_equal(c["exp"], c["hB"])
        _upload(c)
        solves.append(c)
    for path, n in enumerate([37, 100]):
        _run_inv(oracle, n, 4, 1520 + n, path=path)
        c = _inv_case(oracle, n, 4, 1530 + n)
        c["tA"], c["tB"] = (torch.from_numpy(c[x].view(np.int64).copy()).cuda() for x in ("hA", "hB"))
        c["tr"] = torch.full((4,), -7, dtype=torch.int32, device="cuda")
        invs.append(c)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        st = torch.cuda.current_stream().cuda_stream
        for c in solves:
            _launch(c, st)
        for c in invs:
            m4ri_amd.inv_batch_dev(c["tB"].data_ptr(), c["b_stride"], c["b_bs"], c["tA"].data_ptr(), c["a_stride"], c["a_bs"], c["n"], 4,
                                   c["tr"].data_ptr(), st)
    torch.cuda.synchronize()
    for c in solves + invs:
        assert np.array_equal(c["tB"].cpu().numpy().view(np.uint64), c["hB"]) and (c["tr"] == -7).all()
    assert all((c["ts"] == -7).all() for c in solves)
    g.replay()
    torch.cuda.synchronize()
    for c in solves:
        _verify(c)
    for c in invs:
        assert np.array_equal(c["tB"].cpu().numpy().view(np.uint64), c["exp"]) and not np.array_equal(c["exp"], c["hB"])
        assert np.array_equal(c["tA"].cpu().numpy().view(np.uint64), c["hA"]) and np.array_equal(c["tr"].cpu().numpy(), c["rank"])
