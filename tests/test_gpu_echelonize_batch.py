"""m4ri_amd_echelonize_batch_dev (include/m4ri_amd.h, echelon_batch.hip): `batch` independent (reduced) row echelon forms in one
call, every member against the oracle's gf2o_echelonize (pinned to mzd_echelonize by tests/test_echelon_oracle.py) on all four
paths of m4ri_amd_plan_echelonize_batch -- words, rank and pivot columns -- with dirty padding words, tail bits and gaps between
members that must come out unchanged."""
import ctypes

import numpy as np
import pytest
import torch

import m4ri_amd
from m4ri_amd.mzd import Mzd
from test_ple_oracle import _defects, _make

pytestmark = pytest.mark.gpu
KINDS = ("random", "lowrank", "sparse", "zerocols", "defects")


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    assert m4ri_amd.lib().m4ri_amd_device_count() >= 1, "no HIP device visible: the gpu tests have nothing to run on"
    m4ri_amd.init(0)
    torch.cuda.set_device(0)


def _member(kind, m, n, seed):
    if kind == "defects":
        return _defects(m, n, seed, m // 8, m // 16) if n >= 4 else Mzd.random(m, n, seed)
    return _make(kind, m, n, seed)


def _word_masks(n):
    width = (n + 63) // 64
    valid = np.full(width, ~np.uint64(0), dtype=np.uint64)
    if n % 64:
        valid[-1] = np.uint64((1 << (n % 64)) - 1)
    return valid


def _index(m, n, batch, stride, a_bs):
    width = (n + 63) // 64
    return (np.arange(batch, dtype=np.int64)[:, None, None] * a_bs + np.arange(m, dtype=np.int64)[None, :, None] * stride
            + np.arange(width, dtype=np.int64)[None, None, :])


def _pack(members, m, n, stride, a_bs, seed, dirty=True):
    """Host image of the batch: every word the call may not write is random (dirty=True), the valid bits are the members'."""
    batch = len(members)
    total = (batch - 1) * a_bs + m * stride + 5
    rng = np.random.default_rng(seed)
    h = rng.integers(0, 1 << 63, size=total, dtype=np.int64).view(np.uint64) * np.uint64(3) if dirty else np.zeros(total, np.uint64)
    idx, valid = _index(m, n, batch, stride, a_bs), _word_masks(n)
    vals = np.stack([M.valid_words() & valid for M in members])
    h[idx] = (h[idx] & ~valid) | vals
    return h, idx, valid


def _leading(words, rank, mn):
    piv = np.full(mn, -1, dtype=np.int32)
    for i in range(rank):
        w = int(np.flatnonzero(words[i])[0])
        x = int(words[i, w])
        piv[i] = w * 64 + (x & -x).bit_length() - 1
    return piv


def _expected(oracle, members, h, idx, valid, full):
    exp = h.copy()
    ranks, pivs = [], []
    mn = min(members[0].nrows, members[0].ncols)
    for b, M in enumerate(members):
        W = M.copy()
        r = oracle.echelonize(W, full)
        ranks.append(r)
        pivs.append(_leading(W.valid_words() & valid, r, mn))
        exp[idx[b]] = (h[idx[b]] & ~valid) | (W.valid_words() & valid)
    return exp, np.array(ranks, dtype=np.int32), np.concatenate(pivs) if mn else np.zeros(0, np.int32)


def _run(oracle, m, n, batch, full, stride=None, a_bs=None, seed=0, pivots=True, stream=None):
    width = (n + 63) // 64
    stride = width + 1 if stride is None else stride
    a_bs = m * stride + 3 if a_bs is None else a_bs
    members = [_member(KINDS[b % len(KINDS)], m, n, seed + 7 * b) for b in range(batch)]
    h, idx, valid = _pack(members, m, n, stride, a_bs, seed)
    exp, want_rank, want_piv = _expected(oracle, members, h, idx, valid, full)
    mn = min(m, n)
    tA = torch.from_numpy(h.view(np.int64).copy()).cuda()
    tr = torch.full((batch,), -7, dtype=torch.int32, device="cuda")
    tp = torch.full((max(1, batch * mn),), -7, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    s = stream.cuda_stream if stream is not None else 0
    m4ri_amd.echelonize_batch_dev(tA.data_ptr(), stride, a_bs, m, n, batch, full, tr.data_ptr(), tp.data_ptr() if pivots else 0, s)
    torch.cuda.synchronize()
    got = tA.cpu().numpy().view(np.uint64)
    bad = np.flatnonzero(got != exp)
    assert bad.size == 0, f"{bad.size} words differ, first at {bad[:5]} (member {bad[0] // a_bs if a_bs else 0})"
    assert np.array_equal(tr.cpu().numpy(), want_rank)
    if pivots:
        assert np.array_equal(tp.cpu().numpy()[: batch * mn], want_piv)
    else:
        assert (tp.cpu().numpy() == -7).all()
    return want_rank


PATH0 = [(1, 1), (7, 5), (32, 32), (63, 40), (64, 1), (1, 64), (64, 64)]


@pytest.mark.parametrize("m,n", PATH0)
@pytest.mark.parametrize("batch", [1, 37, 4096])
@pytest.mark.parametrize("full", [0, 1])
def test_wave_path_matches_oracle(oracle, m, n, batch, full):
    assert m4ri_amd.plan_echelonize_batch(m, n) == 0
    _run(oracle, m, n, batch, full, seed=100 + m + n + batch)


PATH1 = [(65, 65), (100, 300), (256, 256), (300, 130), (512, 1000), (1088, 1088), (1168, 1024), (2000, 70)]


@pytest.mark.parametrize("m,n", PATH1)
@pytest.mark.parametrize("full", [0, 1])
def test_lds_path_matches_oracle(oracle, m, n, full):
    assert m4ri_amd.plan_echelonize_batch(m, n) == 1
    _run(oracle, m, n, 5, full, seed=200 + m + n)


@pytest.mark.parametrize("m,n", [(1100, 1100), (768, 3488), (1169, 1024), (5000, 300)])
@pytest.mark.parametrize("full", [0, 1])
def test_global_path_matches_oracle(oracle, m, n, full):
    assert m4ri_amd.plan_echelonize_batch(m, n) == 2
    _run(oracle, m, n, 5, full, seed=300 + m + n)


@pytest.mark.parametrize("full", [0, 1])
def test_one_by_one_path_matches_oracle(oracle, full):
    m, n = 1100, 3900
    assert m4ri_amd.plan_echelonize_batch(m, n) == 3
    _run(oracle, m, n, 2, full, seed=400)


@pytest.mark.parametrize("m,n", [(33, 50), (64, 64), (200, 450), (1100, 1100), (1100, 3900)])
@pytest.mark.parametrize("layout", ["tight", "loose"])
def test_frame_is_untouched(oracle, m, n, layout):
    """Tight: stride = width and members back to back; loose: padding words and gaps.  Every word outside the members' valid bits
    is random before the call and must be the same after it (_run compares the whole buffer)."""
    width = (n + 63) // 64
    if layout == "tight":
        _run(oracle, m, n, 3, 1, stride=width, a_bs=(m - 1) * width + width, seed=500 + m)
    else:
        _run(oracle, m, n, 3, 0, stride=width + 3, a_bs=m * (width + 3) + 17, seed=600 + m)


@pytest.mark.parametrize("m,n", [(300, 700), (1100, 1100)])
@pytest.mark.parametrize("full", [0, 1])
def test_bit_identical_to_echelonize_dev(m, n, full):
    batch, width = 4, (n + 63) // 64
    stride, a_bs = width, m * width
    t = torch.zeros(batch * a_bs, dtype=torch.int64, device="cuda")
    for b in range(batch):
        m4ri_amd.fill_dev(t.data_ptr() + 8 * b * a_bs, stride, m, n, 70 + b, 0)
    if m == 300:  # rank-deficient members: the second half of the rows repeats the first
        t.view(batch, m, width)[:, 150:] = t.view(batch, m, width)[:, :150]
    ref = t.clone()
    torch.cuda.synchronize()
    L = m4ri_amd.lib()
    ranks = []
    for b in range(batch):
        r = ctypes.c_int32(0)
        assert L.m4ri_amd_echelonize_dev(ref.data_ptr() + 8 * b * a_bs, stride, m, n, full, ctypes.byref(r), None) == 0
        ranks.append(r.value)
    tr = torch.zeros(batch, dtype=torch.int32, device="cuda")
    m4ri_amd.echelonize_batch_dev(t.data_ptr(), stride, a_bs, m, n, batch, full, tr.data_ptr())
    torch.cuda.synchronize()
    assert torch.equal(t, ref)
    assert tr.cpu().tolist() == ranks
    if m == 300:
        assert max(ranks) <= 150


def test_pivots_null_and_degenerate_sizes(oracle):
    for m, n in [(40, 40), (200, 200), (1100, 1100)]:
        _run(oracle, m, n, 3, 1, pivots=False, seed=700 + m)
    for m, n in [(0, 0), (0, 70), (70, 0)]:
        h = np.arange(1, 65, dtype=np.int64)
        tA = torch.from_numpy(h).cuda()
        tr = torch.full((3,), -7, dtype=torch.int32, device="cuda")
        m4ri_amd.echelonize_batch_dev(tA.data_ptr(), 3, 300, m, n, 3, 1, tr.data_ptr())  # a_bs >= (70 - 1) * 3: legal, never used
        torch.cuda.synchronize()
        assert tr.cpu().tolist() == [0, 0, 0] and np.array_equal(tA.cpu().numpy(), h), (m, n)


def test_two_streams(oracle):
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    jobs = []
    for (m, n, full, s) in [(64, 64, 0, s1), (256, 256, 1, s2)]:
        width = (n + 63) // 64
        batch = 300
        members = [_member(KINDS[b % len(KINDS)], m, n, 800 + b) for b in range(batch)]
        h, idx, valid = _pack(members, m, n, width, m * width, 800 + m)
        exp, want_rank, want_piv = _expected(oracle, members, h, idx, valid, full)
        tA = torch.from_numpy(h.view(np.int64).copy()).cuda()
        tr = torch.zeros(batch, dtype=torch.int32, device="cuda")
        tp = torch.zeros(batch * min(m, n), dtype=torch.int32, device="cuda")
        jobs.append((m, n, full, s, tA, tr, tp, exp, want_rank, want_piv))
    torch.cuda.synchronize()
    for (m, n, full, s, tA, tr, tp, *_rest) in jobs:
        m4ri_amd.echelonize_batch_dev(tA.data_ptr(), (n + 63) // 64, m * ((n + 63) // 64), m, n, 300, full, tr.data_ptr(), tp.data_ptr(), s.cuda_stream)
    s1.synchronize()
    s2.synchronize()
    for (m, n, full, s, tA, tr, tp, exp, want_rank, want_piv) in jobs:
        assert np.array_equal(tA.cpu().numpy().view(np.uint64), exp), (m, n)
        assert np.array_equal(tr.cpu().numpy(), want_rank) and np.array_equal(tp.cpu().numpy(), want_piv), (m, n)


def test_captured_into_a_graph(oracle):
    """Paths 0, 1 and 2 are one launch each and capturable (path 3 blocks and is never captured): a shape of each captured on one
    stream, one chain -- nothing runs, the buffers keep their dirt -- then replayed once.  An ordinary call of each kernel comes
    first: a process's first call sets function attributes, which is not what this test is about."""
    jobs = []
    for path, (m, n, full, batch) in enumerate([(33, 50, 1, 5), (130, 70, 0, 3), (1100, 1100, 1, 2)]):
        assert m4ri_amd.plan_echelonize_batch(m, n) == path
        _run(oracle, m, n, batch, full, seed=900 + m)
        stride, a_bs = (n + 63) // 64 + 1, m * ((n + 63) // 64 + 1) + 3
        members = [_member(KINDS[b % len(KINDS)], m, n, 910 + m + 7 * b) for b in range(batch)]
        h, idx, valid = _pack(members, m, n, stride, a_bs, 920 + m)
        exp, want_rank, want_piv = _expected(oracle, members, h, idx, valid, full)
        tA = torch.from_numpy(h.view(np.int64).copy()).cuda()
        tr = torch.full((batch,), -7, dtype=torch.int32, device="cuda")
        tp = torch.full((batch * min(m, n),), -7, dtype=torch.int32, device="cuda")
        jobs.append((m, n, full, batch, stride, a_bs, h, exp, want_rank, want_piv, tA, tr, tp))
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        st = torch.cuda.current_stream().cuda_stream
        for (m, n, full, batch, stride, a_bs, h, exp, want_rank, want_piv, tA, tr, tp) in jobs:
            m4ri_amd.echelonize_batch_dev(tA.data_ptr(), stride, a_bs, m, n, batch, full, tr.data_ptr(), tp.data_ptr(), st)
    torch.cuda.synchronize()
    for (m, n, full, batch, stride, a_bs, h, exp, want_rank, want_piv, tA, tr, tp) in jobs:
        assert np.array_equal(tA.cpu().numpy().view(np.uint64), h) and (tr == -7).all() and (tp == -7).all(), (m, n)
    g.replay()
    torch.cuda.synchronize()
    for (m, n, full, batch, stride, a_bs, h, exp, want_rank, want_piv, tA, tr, tp) in jobs:
        assert not np.array_equal(exp, h)
        assert np.array_equal(tA.cpu().numpy().view(np.uint64), exp), (m, n)
        assert np.array_equal(tr.cpu().numpy(), want_rank) and np.array_equal(tp.cpu().numpy(), want_piv), (m, n)
