"""m4ri_amd_kernel_left_batch_dev (include/m4ri_amd.h, solve_batch.hip): `batch` null-space bases {x : A_b x = 0} in one call, on all
three paths of m4ri_amd_plan_kernel_batch.  Every member's R against three references: the oracle's gf2o_kernel_left_pluq (pinned to
mzd_kernel_left_pluq by tests/test_solve_oracle.py), A R = 0 with R of full column rank, and the rule below restated from the reduced
echelon form; a few members also against m4ri_amd_kernel_left_pluq_dev.  The R buffers start dirty (valid bits, tail bits, padding
words, gaps between members) and only the valid bits may change; A must come out unchanged."""
import ctypes

import numpy as np
import pytest
import torch

import m4ri_amd
from m4ri_amd.mzd import Mzd
from test_gpu_echelonize_batch import _pack
from test_ple_oracle import _defects, _make

pytestmark = pytest.mark.gpu
KINDS = ("random", "zerocols", "lowrank", "defects", "fullcol", "zero")


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    assert m4ri_amd.lib().m4ri_amd_device_count() >= 1, "no HIP device visible: the gpu tests have nothing to run on"
    m4ri_amd.init(0)
    torch.cuda.set_device(0)


def _w(n):
    return (n + 63) // 64


def _member(m, n, b, seed):
    kind = KINDS[b % len(KINDS)]
    if m == 0 or n == 0 or kind == "zero":
        return Mzd(m, n)
    if kind == "defects" and n > 64:
        return _defects(m, n, seed, m // 8, m // 16)
    if kind == "defects":  # (_defects clears the first word column): a repeated column and repeated rows
        bits = Mzd.random(m, n, seed).to_bits()
        if n > 1:
            bits[:, n // 2] = bits[:, n // 2 - 1]
        bits[m - m // 4:] = bits[: m // 4]
        return Mzd.from_bits(bits)
    if kind == "fullcol":  # rank min(m, n): a unit lower triangle on top
        bits = Mzd.random(m, n, seed).to_bits()
        d = min(m, n)
        bits[:d, :d] = np.tril(bits[:d, :d], -1)
        bits[np.arange(d), np.arange(d)] = 1
        return Mzd.from_bits(bits)
    return _make(kind, m, n, seed)


def _rule(oracle, A, kc=None):
    """mzd_kernel_left_pluq's basis from the reduced echelon form E (pivots p_0 < ... < p_{r-1}): pos = [0 .. n-1], swap pos[i] and
    pos[p_i] for i ascending; free columns f_j = pos[r + j]; column j has a 1 in row f_j and E[i][f_j] in row p_i.  (rank, the first
    min(kc, n - r) columns as n x . bits; kc = None: all of them)"""
    m, n = A.nrows, A.ncols
    if m and n:
        E = A.copy()
        r = oracle.echelonize(E, 1)
        Eb = E.to_bits()[:r]
    else:
        r, Eb = 0, np.zeros((0, n), np.uint8)
    piv = [int(np.flatnonzero(Eb[i])[0]) for i in range(r)]
    pos = list(range(n))
    for i, p in enumerate(piv):
        pos[i], pos[p] = pos[p], pos[i]
    free = np.array(pos[r:][: None if kc is None else kc], dtype=np.int64)
    R = np.zeros((n, free.size), np.uint8)
    R[free, np.arange(free.size)] = 1
    R[np.array(piv, dtype=np.int64), :] = Eb[:, free]
    return r, R


def _basis(oracle, A):
    """(rank, n x (n - rank) bits) from the oracle, checked against the rule and against A R = 0, R of full column rank."""
    m, n = A.nrows, A.ncols
    r, R = _rule(oracle, A)
    if m and n:
        ro, Ro = oracle.kernel_left_pluq(A.copy())
        assert ro == r
        assert np.array_equal(Ro.to_bits() if Ro is not None else np.zeros((n, 0), np.uint8), R), "rule != oracle"
    if R.shape[1]:
        if m:
            assert not ((A.to_bits().astype(np.int64) @ R.astype(np.int64)) & 1).any(), "A R != 0"
        assert _rank_bits(oracle, R) == R.shape[1], "R is not of full column rank"
    return r, R


def _rank_bits(oracle, bits):
    return oracle.echelonize(Mzd.from_bits(bits.copy()), 0) if bits.size else 0


def _case(oracle, m, n, kc, batch, seed, members=None, a_stride=None, a_bs=None, r_stride=None, r_bs=None, shared=False, checked=True):
    a_stride = _w(n) + 1 if a_stride is None else a_stride
    r_stride = _w(kc) + 2 if r_stride is None else r_stride
    a_bs = (0 if shared else m * a_stride + 3) if a_bs is None else a_bs
    r_bs = n * r_stride + 5 if r_bs is None else r_bs
    if members is None:
        members = [_member(m, n, 0 if shared else b, seed + 17 * b) for b in range(1 if shared else batch)]
    hA, _, _ = _pack(members, m, n, a_stride, a_bs, seed)
    dirty = [Mzd.random(n, kc, seed + 5 + b) if n and kc else Mzd(n, kc) for b in range(batch)]
    hR, idx, valid = _pack(dirty, n, kc, r_stride, r_bs, seed + 1)
    exp, ranks, nullity = hR.copy(), [], []
    for b in range(batch):
        A = members[0 if shared else b]
        r, R = _basis(oracle, A) if checked else _rule(oracle, A, kc)
        ranks.append(r)
        nullity.append(n - r)
        if n and kc:
            want = np.zeros((n, kc), np.uint8)
            c = min(kc, n - r)
            want[:, :c] = R[:, :c]
            exp[idx[b]] = (hR[idx[b]] & ~valid) | (Mzd.from_bits(want).valid_words() & valid)
    return dict(m=m, n=n, kc=kc, batch=batch, a_stride=a_stride, a_bs=a_bs, r_stride=r_stride, r_bs=r_bs, hA=hA, hR=hR, exp=exp,
                rank=np.array(ranks, np.int32), nullity=np.array(nullity), members=members, shared=shared)


def _upload(c):
    c["tA"] = torch.from_numpy(c["hA"].view(np.int64).copy()).cuda()
    c["tR"] = torch.from_numpy(c["hR"].view(np.int64).copy()).cuda()
    c["tr"] = torch.full((max(1, c["batch"]),), -7, dtype=torch.int32, device="cuda")


def _launch(c, stream=0):
    m4ri_amd.kernel_left_batch_dev(c["tA"].data_ptr(), c["a_stride"], c["a_bs"], c["m"], c["n"], c["tR"].data_ptr(), c["r_stride"],
                                   c["r_bs"], c["kc"], c["batch"], c["tr"].data_ptr(), stream)


def _verify(c):
    assert np.array_equal(c["tA"].cpu().numpy().view(np.uint64), c["hA"]), "A (or its frame) was written"
    got = c["tR"].cpu().numpy().view(np.uint64)
    bad = np.flatnonzero(got != c["exp"])
    assert bad.size == 0, f"{bad.size} words of R differ, first at {bad[:5]} (member {bad[0] // c['r_bs'] if c['r_bs'] else 0})"
    assert np.array_equal(c["tr"].cpu().numpy()[: c["batch"]], c["rank"])


def _run(oracle, m, n, kc, batch, seed, path=None, **kw):
    if path is not None:
        assert m4ri_amd.plan_kernel_batch(m, n) == path
    c = _case(oracle, m, n, kc, batch, seed, **kw)
    _upload(c)
    torch.cuda.synchronize()
    _launch(c)
    torch.cuda.synchronize()
    _verify(c)
    return c


# (m, n): m < n, m = n, m > n
PATH0 = [(40, 50), (64, 64), (63, 40), (5, 5), (30, 64), (64, 20), (1, 64), (64, 1)]
PATH1 = [(65, 63), (63, 65), (100, 100), (200, 70), (70, 200), (300, 300), (513, 511), (20, 1000), (1024, 1024)]
PATH2 = [(1300, 1000), (900, 1300), (1100, 1100)]


@pytest.mark.parametrize("m,n", PATH0)
@pytest.mark.parametrize("batch", [37, 1000])
def test_wave_path(oracle, m, n, batch):
    c = _run(oracle, m, n, n, batch, 100 + m + n, path=0, checked=batch < 100)
    assert (c["nullity"] > 0).any()


@pytest.mark.parametrize("m,n", PATH1)
def test_lds_path(oracle, m, n):
    c = _run(oracle, m, n, n, 7, 200 + m + n, path=1)
    assert (c["nullity"] > 0).any()


@pytest.mark.parametrize("m,n", PATH2)
def test_one_by_one_path(oracle, m, n):
    _run(oracle, m, n, n, 3, 300 + m + n, path=2)


@pytest.mark.parametrize("m,n", [(40, 50), (64, 64), (100, 100), (70, 200), (1300, 1000)])
def test_truncated_bases(oracle, m, n):
    """kc = 0, 1, a value below the nullity of the low-rank members, and n; the columns past the nullity are written zero."""
    for kc in (0, 1, 7, n):
        c = _run(oracle, m, n, kc, 6, 400 + m + kc)
        if kc == 7:
            assert (c["nullity"] > kc).any()


@pytest.mark.parametrize("m,n,kc", [(33, 50, 20), (64, 64, 64), (200, 450, 70), (1300, 1000, 130)])
@pytest.mark.parametrize("layout", ["tight", "loose"])
def test_frames(oracle, m, n, kc, layout):
    """Tight: stride = width, members back to back; loose: padding words and gaps.  Every word outside the members' valid bits is
    random before the call and must be the same after it."""
    if layout == "tight":
        kw = dict(a_stride=_w(n), a_bs=m * _w(n), r_stride=_w(kc), r_bs=n * _w(kc))
    else:
        kw = dict(a_stride=_w(n) + 3, a_bs=m * (_w(n) + 3) + 17, r_stride=_w(kc) + 4, r_bs=n * (_w(kc) + 4) + 9)
    _run(oracle, m, n, kc, 4, 500 + m, **kw)


@pytest.mark.parametrize("m,n", [(40, 64), (300, 300), (1300, 1000)])
def test_shared_a(oracle, m, n):
    """a_bs = 0: one A for every member."""
    c = _run(oracle, m, n, n, 5, 600 + m, shared=True)
    assert len(set(c["rank"].tolist())) == 1


@pytest.mark.parametrize("m,n,kc", [(0, 5, 3), (0, 64, 64), (0, 100, 70), (0, 3000, 100), (0, 30000, 5), (5, 0, 0), (100, 0, 0),
                                    (30000, 0, 0), (0, 0, 0)])
def test_degenerate_sizes(oracle, m, n, kc):
    """m = 0: rank 0 and the first kc columns of the identity; n = 0: rank 0 and nothing else written.  Against the rule."""
    if m == 0 and n:
        assert _rule(oracle, Mzd(0, n), kc)[1].tolist() == np.eye(n, kc, dtype=np.uint8).tolist()
    c = _run(oracle, m, n, kc, 2, 700, checked=False)
    assert (c["rank"] == 0).all()


@pytest.mark.parametrize("m,n", [(40, 50), (64, 64), (64, 20), (200, 70), (70, 200), (300, 300), (1300, 1000)])
def test_bit_identical_to_kernel_left_pluq_dev(oracle, m, n):
    c = _run(oracle, m, n, n, 6, 800 + m + n)
    L = m4ri_amd.lib()
    wa = _w(n)
    got = c["tR"].cpu().numpy().view(np.uint64)
    for b, A in enumerate(c["members"]):
        dA = torch.from_numpy(A.valid_words().copy().view(np.int64)).cuda()
        dR = torch.zeros(max(1, n * wa), dtype=torch.int64, device="cuda")
        r = ctypes.c_int32(-1)
        assert L.m4ri_amd_kernel_left_pluq_dev(dA.data_ptr(), wa, m, n, dR.data_ptr(), wa, 0, ctypes.byref(r), None) == 0
        torch.cuda.synchronize()
        assert r.value == c["rank"][b]
        k = n - r.value
        if not k:
            continue
        kw = _w(k)
        mask = np.full(kw, ~np.uint64(0), np.uint64)
        if k % 64:
            mask[-1] = np.uint64((1 << (k % 64)) - 1)
        want = dR.cpu().numpy().view(np.uint64).reshape(n, wa)[:, :kw] & mask
        mine = got[b * c["r_bs"] + np.arange(n)[:, None] * c["r_stride"] + np.arange(kw)[None, :]] & mask
        assert np.array_equal(mine, want), (m, n, b)


def test_two_streams(oracle):
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    c1 = _case(oracle, 64, 64, 64, 300, 900, checked=False)
    c2 = _case(oracle, 256, 256, 100, 40, 1000)
    for c in (c1, c2):
        _upload(c)
    torch.cuda.synchronize()
    _launch(c1, s1.cuda_stream)
    _launch(c2, s2.cuda_stream)
    s1.synchronize()
    s2.synchronize()
    _verify(c1)
    _verify(c2)


def test_captured_into_a_graph(oracle):
    """Paths 0 and 1 are one launch each and capturable (path 2 blocks and is never captured): a shape of each captured on one stream,
    one chain -- nothing runs, R and rank keep their dirt -- then replayed once.  An ordinary call of each kernel comes first: a
    process's first call sets function attributes, which is not what this test is about."""
    cases = []
    for path, (m, n, kc, batch) in enumerate([(40, 50, 50, 7), (70, 200, 100, 7)]):
        _run(oracle, m, n, kc, batch, 1100 + m, path=path)
        c = _case(oracle, m, n, kc, batch, 1110 + m)
        assert not np.array_equal(c["exp"], c["hR"])
        _upload(c)
        cases.append(c)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for c in cases:
            _launch(c, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    for c in cases:
        assert np.array_equal(c["tR"].cpu().numpy().view(np.uint64), c["hR"]) and (c["tr"] == -7).all(), (c["m"], c["n"])
    g.replay()
    torch.cuda.synchronize()
    for c in cases:
        _verify(c)
