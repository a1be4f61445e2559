"""m4ri_amd_ple_batch_dev (include/m4ri_amd.h, ple_batch.hip): `batch` PLE / PLUQ decompositions in one call, on all four paths of
m4ri_amd_plan_ple_batch.  Every member's valid bits, P, Q and rank against the oracle's gf2o_ple / gf2o_pluq (pinned to
_mzd_ple_russian / _mzd_pluq_russian by tests/test_ple_oracle.py); for PLUQ also a NumPy reconstruction P L U Q = A that does not use
the oracle; a few members against m4ri_amd_ple_dev / m4ri_amd_pluq_dev.  The buffers start dirty (tail bits, padding words, gaps
between members, P, Q, rank) and only the valid bits may change."""
import ctypes

import numpy as np
import pytest
import torch

import m4ri_amd
from test_gpu_echelonize_batch import _pack
from test_gpu_kernel_batch import _member

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    assert m4ri_amd.lib().m4ri_amd_device_count() >= 1, "no HIP device visible: the gpu tests have nothing to run on"
    m4ri_amd.init(0)
    torch.cuda.set_device(0)


def _w(n):
    return (n + 63) // 64


def _reconstruct(bits, rank, P, Q):
    """P L U Q from the PLUQ form: L the unit lower triangle of the first `rank` columns, U the unit upper first `rank` rows; Q's
    transpositions undone on the columns of L U, then P's on its rows (both descending)."""
    m, n = bits.shape
    L = np.zeros((m, rank), np.float32)
    L[:, :] = np.tril(bits[:, :rank], -1)
    L[np.arange(rank), np.arange(rank)] = 1
    U = np.triu(bits[:rank], 1).astype(np.float32)
    U[np.arange(rank), np.arange(rank)] = 1
    X = (np.rint(L @ U).astype(np.int64) & 1).astype(np.uint8)  # sums up to `rank` < 2^24: exact in float32
    for j in range(rank - 1, -1, -1):
        if Q[j] != j:
            X[:, [j, Q[j]]] = X[:, [Q[j], j]]
    for i in range(rank - 1, -1, -1):
        if P[i] != i:
            X[[i, P[i]]] = X[[P[i], i]]
    return X


def _case(oracle, m, n, batch, pluq, seed, stride=None, a_bs=None):
    stride = _w(n) + 1 if stride is None else stride
    a_bs = m * stride + 3 if a_bs is None else a_bs
    members = [_member(m, n, b, seed + 17 * b) for b in range(batch)]
    h, idx, valid = _pack(members, m, n, stride, a_bs, seed)
    exp, ranks, Ps, Qs = h.copy(), [], [], []
    for b, A in enumerate(members):
        W = A.copy()
        if m and n:
            r, P, Q = oracle.ple(W, pluq=bool(pluq))
            exp[idx[b]] = (h[idx[b]] & ~valid) | (W.valid_words() & valid)
        else:
            r, P, Q = 0, np.arange(m, dtype=np.int32), np.arange(n, dtype=np.int32)
        assert (P[r:] == np.arange(r, m)).all() and (Q[r:] == np.arange(r, n)).all(), "the identity behind the rank"
        ranks.append(r)
        Ps.append(P.copy())
        Qs.append(Q.copy())
        if pluq and m and n and (b < 4 or m <= 300):
            assert np.array_equal(_reconstruct(W.to_bits(), r, P, Q), A.to_bits()), "oracle: P L U Q != A"
    return dict(m=m, n=n, batch=batch, pluq=pluq, stride=stride, a_bs=a_bs, members=members, h=h, idx=idx, valid=valid, exp=exp,
                rank=np.array(ranks, np.int32), P=np.concatenate(Ps) if batch * m else np.zeros(0, np.int32),
                Q=np.concatenate(Qs) if batch * n else np.zeros(0, np.int32))


def _upload(c):
    c["tA"] = torch.from_numpy(c["h"].view(np.int64).copy()).cuda()
    c["tP"] = torch.full((max(1, c["batch"] * c["m"]) + 3,), -7, dtype=torch.int32, device="cuda")
    c["tQ"] = torch.full((max(1, c["batch"] * c["n"]) + 3,), -7, dtype=torch.int32, device="cuda")
    c["tr"] = torch.full((max(1, c["batch"]) + 3,), -7, dtype=torch.int32, device="cuda")


def _launch(c, stream=0):
    m4ri_amd.ple_batch_dev(c["tA"].data_ptr(), c["stride"], c["a_bs"], c["m"], c["n"], c["batch"], c["pluq"], c["tP"].data_ptr(),
                           c["tQ"].data_ptr(), c["tr"].data_ptr(), stream)


def _verify(c):
    m, n, batch = c["m"], c["n"], c["batch"]
    got = c["tA"].cpu().numpy().view(np.uint64)
    r, P, Q = c["tr"].cpu().numpy(), c["tP"].cpu().numpy(), c["tQ"].cpu().numpy()
    assert np.array_equal(r[:batch], c["rank"]), "rank"
    assert (r[batch:] == -7).all() and (P[batch * m:] == -7).all() and (Q[batch * n:] == -7).all(), "written behind the arrays' ends"
    assert np.array_equal(P[: batch * m], c["P"]), "P"
    assert np.array_equal(Q[: batch * n], c["Q"]), "Q"
    bad = np.flatnonzero(got != c["exp"])  # (a) the valid bits and (b) the frame in one comparison
    assert bad.size == 0, f"{bad.size} words differ, first at {bad[:5]} (member {bad[0] // c['a_bs'] if c['a_bs'] else 0})"
    if c["pluq"] and m and n:  # (c) straight from the device's output
        for b in range(min(batch, 3)):
            bits = _bits(got[c["idx"][b]] & c["valid"], n)
            X = _reconstruct(bits, int(r[b]), P[b * m:(b + 1) * m], Q[b * n:(b + 1) * n])
            assert np.array_equal(X, c["members"][b].to_bits()), f"P L U Q != A for member {b}"


def _bits(words, n):
    """rows x width uint64 words -> rows x n bits"""
    b = np.unpackbits(np.ascontiguousarray(words).view(np.uint8), axis=1, bitorder="little")
    return b[:, :n]


def _run(oracle, m, n, batch, pluq, seed, path=None, **kw):
    if path is not None:
        assert m4ri_amd.plan_ple_batch(m, n) == path
    c = _case(oracle, m, n, batch, pluq, seed, **kw)
    _upload(c)
    torch.cuda.synchronize()
    _launch(c)
    torch.cuda.synchronize()
    _verify(c)
    return c


PATH0 = [(1, 1), (64, 64), (64, 17), (17, 64), (33, 50), (1, 64), (64, 1)]
PATH1 = [(65, 64), (64, 65), (100, 200), (200, 100), (256, 256), (513, 300)]


@pytest.mark.parametrize("m,n", PATH0)
@pytest.mark.parametrize("batch", [1, 37, 1001])
@pytest.mark.parametrize("pluq", [0, 1])
def test_wave_path(oracle, m, n, batch, pluq):
    c = _run(oracle, m, n, batch, pluq, 100 + m + n + batch, path=0)
    if batch > 6 and min(m, n) > 8:
        assert (c["rank"] < min(m, n)).any() and (c["rank"] == min(m, n)).any()


@pytest.mark.parametrize("m,n", PATH1)
@pytest.mark.parametrize("pluq", [0, 1])
def test_lds_path(oracle, m, n, pluq):
    c = _run(oracle, m, n, 7, pluq, 200 + m + n, path=1)
    assert (c["rank"] < min(m, n)).any() and (c["rank"] == min(m, n)).any()
    assert any((c["Q"][b * n:(b + 1) * n] != np.arange(n)).any() for b in range(7)), "no member moves a column: L is never compressed"


@pytest.mark.parametrize("pluq", [0, 1])
def test_largest_square_of_the_lds_path(oracle, pluq):
    n = max(n for n in range(65, 3000) if m4ri_amd.plan_ple_batch(n, n) == 1)
    assert m4ri_amd.plan_ple_batch(n + 1, n + 1) == 2
    _run(oracle, n, n, 3, pluq, 250, path=1)
    _run(oracle, n + 1, n + 1, 2, pluq, 251, path=2)


@pytest.mark.parametrize("m,n", [(1500, 1500), (1300, 2100), (5000, 300)])
@pytest.mark.parametrize("pluq", [0, 1])
def test_global_path(oracle, m, n, pluq):
    _run(oracle, m, n, 3, pluq, 300 + m + n, path=2)


@pytest.mark.parametrize("pluq", [0, 1])
def test_one_by_one_path(oracle, pluq):
    _run(oracle, 3000, 3000, 2, pluq, 400, path=3)


@pytest.mark.parametrize("m,n", [(33, 50), (64, 64), (200, 450), (1500, 1500), (1100, 3900)])
@pytest.mark.parametrize("layout", ["tight", "loose"])
def test_frame_is_untouched(oracle, m, n, layout):
    """Tight: stride = width (odd or even) and members back to back; loose: padding words and gaps.  Every word outside the members'
    valid bits is random before the call and must be the same after it (_verify compares the whole buffer)."""
    width = _w(n)
    if layout == "tight":
        _run(oracle, m, n, 3, 1, 500 + m, stride=width, a_bs=m * width)
    else:
        _run(oracle, m, n, 3, 0, 600 + m, stride=width + 3, a_bs=m * (width + 3) + 17)


@pytest.mark.parametrize("m,n", [(0, 0), (0, 70), (70, 0), (0, 64), (64, 0), (0, 3000)])
@pytest.mark.parametrize("pluq", [0, 1])
def test_zero_sizes(oracle, m, n, pluq):
    """rank 0, the identity in P and Q, no matrix word written."""
    c = _case(oracle, m, n, 3, pluq, 700, stride=_w(n) + 1, a_bs=max(m, 1) * (_w(n) + 1) + 3)
    _upload(c)
    torch.cuda.synchronize()
    _launch(c)
    torch.cuda.synchronize()
    _verify(c)
    assert (c["rank"] == 0).all() and np.array_equal(c["exp"], c["h"])


@pytest.mark.parametrize("m,n", [(40, 50), (64, 64), (200, 70), (70, 200), (300, 300), (1500, 1500), (3000, 3000)])  # paths 0 ... 3
@pytest.mark.parametrize("pluq", [0, 1])
def test_bit_identical_to_the_per_member_call(oracle, m, n, pluq):
    c = _run(oracle, m, n, 6, pluq, 800 + m + n)
    L = m4ri_amd.lib()
    fn = L.m4ri_amd_pluq_dev if pluq else L.m4ri_amd_ple_dev
    wa = _w(n)
    got = c["tA"].cpu().numpy().view(np.uint64)
    for b in (0, 2, 3, 4):  # random, low rank, repeated rows and columns, full column rank
        dA = torch.from_numpy(c["members"][b].valid_words().copy().view(np.int64)).cuda()
        P, Q = np.full(m, -1, np.int32), np.full(n, -1, np.int32)
        r = ctypes.c_int32(-1)
        assert fn(dA.data_ptr(), wa, m, n, P.ctypes.data, Q.ctypes.data, ctypes.byref(r), 0, None) == 0
        torch.cuda.synchronize()
        assert r.value == c["rank"][b]
        assert np.array_equal(P, c["P"][b * m:(b + 1) * m]) and np.array_equal(Q, c["Q"][b * n:(b + 1) * n])
        assert np.array_equal(dA.cpu().numpy().view(np.uint64).reshape(m, wa), got[c["idx"][b]] & c["valid"]), (m, n, b)


def test_non_default_stream(oracle):
    """A path-0 and a path-1 shape on a stream of their own, compared after synchronising that stream only."""
    s = torch.cuda.Stream()
    c1 = _case(oracle, 64, 64, 300, 1, 900)
    c2 = _case(oracle, 256, 256, 40, 0, 1000)
    for c in (c1, c2):
        _upload(c)
    torch.cuda.synchronize()
    _launch(c1, s.cuda_stream)
    _launch(c2, s.cuda_stream)
    s.synchronize()
    _verify(c1)
    _verify(c2)


def test_captured_into_a_graph(oracle):
    """Paths 0, 1 and 2 are one launch each and capturable (path 3 blocks and is never captured): a shape of each captured on one
    stream, one chain -- nothing runs, the matrices, P, Q and rank keep their dirt -- then replayed once.  An ordinary call of each
    kernel comes first: a process's first call sets function attributes, which is not what this test is about."""
    cases = []
    for path, (m, n, batch, pluq) in enumerate([(33, 50, 5, 1), (100, 200, 3, 0), (1500, 1500, 2, 1)]):
        _run(oracle, m, n, batch, pluq, 1100 + m, path=path)
        c = _case(oracle, m, n, batch, pluq, 1110 + m)
        _upload(c)
        cases.append(c)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for c in cases:
            _launch(c, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    for c in cases:
        assert np.array_equal(c["tA"].cpu().numpy().view(np.uint64), c["h"]) and not np.array_equal(c["exp"], c["h"]), (c["m"], c["n"])
        assert (c["tP"] == -7).all() and (c["tQ"] == -7).all() and (c["tr"] == -7).all(), (c["m"], c["n"])
    g.replay()
    torch.cuda.synchronize()
    for c in cases:
        _verify(c)
