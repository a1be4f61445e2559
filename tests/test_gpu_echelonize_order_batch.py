"""m4ri_amd_echelonize_order_batch_dev and m4ri_amd_random_orders_batch_dev (include/m4ri_amd.h, echelon_order_batch.hip) on the device:
every member against the NumPy rule of tests/order_cases.py (pinned to the oracle by tests/test_echelonize_order_plan.py) on the three
paths of m4ri_amd_plan_echelonize_order_batch -- ALL words of the images, the dirty padding words, tail bits and gaps between members
included, rank and pivots exactly --, against m4ri_amd_echelonize_batch_dev and the four-launch composition bit for bit, and one
iteration of Lee-Brickell, orders to weights, against the NumPy pipeline."""
from functools import lru_cache

import numpy as np
import pytest
import torch

import m4ri_amd
import order_cases as oc
from m4ri_amd.mzd import Mzd
from test_echelonize_order_plan import pipeline

pytestmark = pytest.mark.gpu
PATH0_MAX, PATH1_MAX = "M4RI_AMD_ECH_ORDER_PATH0_MAX", "M4RI_AMD_ECH_ORDER_PATH1_MAX"
I32_MIN, I32_MAX = -(1 << 31), (1 << 31) - 1
ORDERS = ("natural", "reversed", "perm", "partial", "empty", "dups", "null", "null_partial")
# (order, one order for all members, where A and D are, batch): every order, both sharings, the three placements, batch 1 and 5
CONFIGS = [("natural", False, "inplace", 5), ("null", True, "inplace", 1), ("reversed", True, "out", 5), ("perm", False, "shared_a", 5),
           ("perm", False, "out", 1), ("partial", False, "inplace", 5), ("empty", True, "out", 5), ("dups", False, "shared_a", 5),
           ("null_partial", True, "out", 5), ("perm", True, "inplace", 5), ("dups", True, "inplace", 1), ("partial", True, "shared_a", 5)]
SHAPES0 = [(1, 1), (7, 5), (33, 64), (64, 1), (1, 64), (64, 64)]
SHAPES1 = [(5, 65), (65, 65), (70, 130), (130, 70), (64, 1024)]


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    assert m4ri_amd.lib().m4ri_amd_device_count() >= 1, "no HIP device visible: the gpu tests have nothing to run on"
    m4ri_amd.init(0)
    torch.cuda.set_device(0)


def _route(monkeypatch, path, m, n):
    """Send members of this shape down `path`: the natural one, or path 1 / 2 by the overrides (read per call)."""
    monkeypatch.delenv(PATH0_MAX, raising=False)
    monkeypatch.delenv(PATH1_MAX, raising=False)
    natural = m4ri_amd.plan_echelonize_order_batch(m, n)
    assert natural <= path
    if path > natural:
        monkeypatch.setenv(PATH0_MAX, "0")
        if path == 2:
            monkeypatch.setenv(PATH1_MAX, "0")


def _member(rng, m, n, b):
    """Random bits; every third member rank-deficient (repeated rows), every fourth with zero columns."""
    G = rng.integers(0, 2, size=(m, n), dtype=np.uint8)
    if b % 3 == 1 and m >= 4:
        G[m // 2:] = G[: m - m // 2]
    if b % 4 == 2 and n >= 4:
        G[:, rng.integers(0, n, size=n // 3)] = 0
    return G


def _order(rng, kind, n, b):
    """(entries or None, olen)"""
    if kind == "natural":
        return np.arange(n, dtype=np.int32), n
    if kind == "reversed":
        return np.arange(n, dtype=np.int32)[::-1].copy(), n
    if kind == "perm":
        return rng.permutation(n).astype(np.int32), n
    if kind == "partial":
        return rng.permutation(n).astype(np.int32)[: n // 2], n // 2
    if kind == "empty":
        return np.zeros(0, dtype=np.int32), 0
    if kind == "dups":
        return rng.integers(0, n, size=n).astype(np.int32), n
    return None, (n if kind == "null" else n // 2)


class Case:
    """The host side of one call: images, orders, and what has to come back.  Built once per argument tuple (the paths share it)."""

    def __init__(self, m, n, batch, full, kind, shared_order, mode, pivot_rows, seed, bad=()):
        rng = np.random.default_rng(seed)
        self.m, self.n, self.batch, self.full, self.mode, self.pr = m, n, batch, full, mode, pivot_rows
        self.pm = min(pivot_rows, n)
        width = (n + 63) // 64
        self.a_stride, self.d_stride = width + 1, width + 2
        na = 1 if mode == "shared_a" else batch
        self.a_bs = 0 if mode == "shared_a" else m * self.a_stride + 3
        self.d_bs = m * self.d_stride + 5
        if mode == "inplace":
            self.d_stride, self.d_bs = self.a_stride, self.a_bs
        members = [_member(rng, m, n, b) for b in range(na)]
        self.A, a_idx, valid = oc.pack(members, m, n, self.a_stride, self.a_bs if na > 1 else m * self.a_stride, seed + 1)
        if mode == "inplace":
            self.D, d_idx = self.A, a_idx
        else:   # D's valid bits hold something else before the call
            self.D, d_idx, _ = oc.pack([_member(rng, m, n, 0) for _ in range(batch)], m, n, self.d_stride, self.d_bs, seed + 2)
        # the orders, member b's at b * o_bs, the gaps and the entries behind olen out of range
        no = 1 if shared_order else batch
        orders = [_order(rng, kind, n, b) for b in range(no)]
        self.olen = orders[0][1]
        self.null = orders[0][0] is None
        self.o_bs = 0 if shared_order else self.olen + 3
        self.O = np.full((no - 1) * self.o_bs + self.olen + 4, I32_MAX, dtype=np.int32)
        for b, (o, _olen) in enumerate(orders):
            if o is not None:
                self.O[b * self.o_bs: b * self.o_bs + self.olen] = o
        for (b, at, value) in bad:   # entries out of range in some members
            self.O[b * self.o_bs + at % self.olen] = value
        self.want_D = self.D.copy()
        self.want_rank = np.zeros(batch, dtype=np.int32)
        self.want_piv = np.full(batch * self.pm, -1, dtype=np.int32)
        for b in range(batch):
            o = None if self.null else self.O[(b * self.o_bs if not shared_order else 0):][: self.olen]
            o = list(range(self.olen)) if o is None else o
            S, r, piv = oc.ech_order(members[b if na > 1 else 0], o, full, pivot_rows)
            self.want_rank[b] = r
            self.want_piv[b * self.pm: (b + 1) * self.pm] = piv
            if r >= 0:   # a refused member is not written at all
                oc.put(self.want_D, d_idx, valid, b, S)

    def run(self, stream=0, pivots=True):
        tA = torch.from_numpy(self.A.view(np.int64).copy()).cuda()
        tD = tA if self.mode == "inplace" else torch.from_numpy(self.D.view(np.int64).copy()).cuda()
        tO = torch.from_numpy(self.O.copy()).cuda()
        tr = torch.full((self.batch + 2,), -7, dtype=torch.int32, device="cuda")
        tp = torch.full((self.batch * self.pm + 2,), -7, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        m4ri_amd.echelonize_order_batch_dev(tD.data_ptr(), self.d_stride, self.d_bs, tA.data_ptr(), self.a_stride, self.a_bs, self.m, self.n, self.pr,
                                            0 if self.null else tO.data_ptr(), self.o_bs, self.olen, self.batch, self.full, tr.data_ptr(),
                                            tp.data_ptr() if pivots else 0, stream)
        torch.cuda.synchronize()
        got = tD.cpu().numpy().view(np.uint64)
        wrong = np.flatnonzero(got != self.want_D)
        assert wrong.size == 0, f"{wrong.size} words of D differ, first at {wrong[:5]} (d_bs {self.d_bs})"
        if self.mode != "inplace":
            assert np.array_equal(tA.cpu().numpy().view(np.uint64), self.A), "A was written"
        assert np.array_equal(tO.cpu().numpy(), self.O)
        r, p = tr.cpu().numpy(), tp.cpu().numpy()
        assert np.array_equal(r[: self.batch], self.want_rank) and (r[self.batch:] == -7).all()
        assert np.array_equal(p[: self.batch * self.pm], self.want_piv if pivots else np.full(self.batch * self.pm, -7)) and (p[self.batch * self.pm:] == -7).all()


@lru_cache(maxsize=None)
def _case(*args):
    return Case(*args)


def _sweep(monkeypatch, path, m, n, full):
    _route(monkeypatch, path, m, n)
    for i, (kind, shared, mode, batch) in enumerate(CONFIGS):
        _case(m, n, batch, full, kind, shared, mode, m, 1000 * m + 10 * n + i).run(pivots=i % 4 != 3)


@pytest.mark.parametrize("m,n", SHAPES0)
@pytest.mark.parametrize("full", [0, 1])
def test_wave_path(monkeypatch, m, n, full):
    assert m4ri_amd.plan_echelonize_order_batch(m, n) == 0
    _sweep(monkeypatch, 0, m, n, full)


@pytest.mark.parametrize("m,n", SHAPES1)
@pytest.mark.parametrize("full", [0, 1])
def test_lds_path(monkeypatch, m, n, full):
    assert m4ri_amd.plan_echelonize_order_batch(m, n) == 1
    _sweep(monkeypatch, 1, m, n, full)


@pytest.mark.parametrize("m,n", SHAPES0 + SHAPES1)
@pytest.mark.parametrize("full", [0, 1])
def test_global_path_by_override(monkeypatch, m, n, full):
    _sweep(monkeypatch, 2, m, n, full)


@pytest.mark.parametrize("m,n", SHAPES0)
def test_lds_path_by_override(monkeypatch, m, n):
    _sweep(monkeypatch, 1, m, n, 1)


@pytest.mark.parametrize("mode,kind,full", [("out", "perm", 1), ("inplace", "reversed", 0)])
def test_global_path_natural_member(monkeypatch, mode, kind, full):
    m = n = 1100
    _route(monkeypatch, 2, m, n)
    assert m4ri_amd.plan_echelonize_order_batch(m, n) == 2
    _case(m, n, 2, full, kind, False, mode, m, 77).run()


@pytest.mark.parametrize("path,m,n", [(0, 33, 64), (1, 70, 130), (2, 7, 5), (2, 65, 65)])
def test_batch_of_257(monkeypatch, path, m, n):
    """More members than one workgroup of the wave path holds, and than a few rounds of the others: per-member orders from one shared A."""
    _route(monkeypatch, path, m, n)
    _case(m, n, 257, 1, "perm", False, "shared_a", m, 300 + m).run()
    _case(m, n, 257, 0, "dups", False, "inplace", m, 301 + m).run()


@pytest.mark.parametrize("path,m,n,prs", [(0, 33, 64, (33, 32, 0, 1)), (0, 64, 64, (64, 63, 0)), (1, 130, 70, (130, 129, 0, 63, 64, 65)),
                                          (2, 130, 70, (130, 129, 0, 63, 64, 65)), (1, 70, 130, (70, 69, 64, 1)), (2, 33, 64, (32, 0))])
@pytest.mark.parametrize("full", [0, 1])
def test_rows_that_only_follow(monkeypatch, path, m, n, prs, full):
    """pivot_rows below nrows: the rows behind take the updates, are never pivots and never move; either side of a flag word's 64 rows."""
    _route(monkeypatch, path, m, n)
    for pr in prs:
        _case(m, n, 5, full, "perm", False, "out", pr, 400 + pr).run()
        _case(m, n, 5, full, "null", True, "inplace", pr, 500 + pr).run()


@pytest.mark.parametrize("path,m,n", [(0, 33, 64), (1, 70, 130), (2, 70, 130), (2, 33, 64)])
@pytest.mark.parametrize("mode", ["inplace", "out", "shared_a"])
def test_bad_entries_refuse_their_members_only(monkeypatch, path, m, n, mode):
    """Entries out of range in members 1, 2, 4 and 5 of 7 (first, last and middle positions): rank -1, pivots -1, D_b byte for byte what
    it was; members 0, 3 and 6 correct.  The range check answers these; nothing goes out of bounds."""
    _route(monkeypatch, path, m, n)
    bad = ((1, 0, -1), (2, -1, n), (4, n // 2, I32_MIN), (5, 3, I32_MAX), (5, 7, -5))
    c = _case(m, n, 7, 1, "perm", False, mode, m, 600 + m, bad)
    assert c.want_rank.tolist().count(-1) == 4 and c.want_rank[0] >= 0 and c.want_rank[3] >= 0 and c.want_rank[6] >= 0
    c.run()
    c.run(pivots=False)


def test_one_bad_shared_order_refuses_every_member(monkeypatch):
    for path, (m, n) in ((0, (33, 64)), (1, (70, 130)), (2, (70, 130))):
        _route(monkeypatch, path, m, n)
        c = _case(m, n, 3, 0, "perm", True, "out", m, 650, ((0, 5, n),))
        assert c.want_rank.tolist() == [-1, -1, -1]
        c.run()


def test_degenerate_sizes(monkeypatch):
    for path in (0, 1, 2):
        for (m, n) in ((0, 5), (5, 0), (0, 0), (0, 70)):
            _route(monkeypatch, max(path, m4ri_amd.plan_echelonize_order_batch(m, n)), m, n)
            _case(m, n, 3, 1, "null", True, "out", 0, 700).run()
    _route(monkeypatch, 1, 0, 70)
    _case(0, 70, 3, 1, "perm", False, "out", 0, 701, ((1, 2, 70),)).run()    # no rows, and still a bad entry is a bad entry


def test_outputs_packed_back_to_back():
    """The accepted neighbours of the overlap checks, on the device: order, rank and pivots in one allocation with nothing between
    them, D right behind A."""
    m, n, batch = 20, 64, 4
    rng = np.random.default_rng(9)
    G = [_member(rng, m, n, b) for b in range(batch)]
    words = np.concatenate([oc.to_words(g).reshape(-1) for g in G])
    orders = np.stack([rng.permutation(n).astype(np.int32) for _ in range(batch)])
    tM = torch.zeros(2 * batch * m, dtype=torch.int64, device="cuda")
    tM[: batch * m] = torch.from_numpy(words.view(np.int64)).cuda()
    tI = torch.zeros(batch * n + batch + batch * m, dtype=torch.int32, device="cuda")
    tI[: batch * n] = torch.from_numpy(orders.reshape(-1)).cuda()
    torch.cuda.synchronize()
    A, O = tM.data_ptr(), tI.data_ptr()
    D, R = A + 8 * batch * m, O + 4 * batch * n
    m4ri_amd.echelonize_order_batch_dev(D, 1, m, A, 1, m, m, n, m, O, n, n, batch, 1, R, R + 4 * batch)
    torch.cuda.synchronize()
    got, ints = tM.cpu().numpy().view(np.uint64), tI.cpu().numpy()
    assert np.array_equal(got[: batch * m], words) and np.array_equal(ints[: batch * n], orders.reshape(-1))
    for b in range(batch):
        S, r, piv = oc.ech_order(G[b], orders[b], 1, m)
        assert np.array_equal(got[(batch + b) * m: (batch + b + 1) * m], oc.to_words(S).reshape(-1))
        assert ints[batch * n + b] == r and np.array_equal(ints[batch * n + batch + b * m:][:m], piv)


# ---- ties to code that exists -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("m,n,batch", [(33, 64, 9), (64, 64, 9), (70, 130, 5), (64, 1024, 5), (300, 200, 3), (1100, 1100, 2)])
@pytest.mark.parametrize("full", [0, 1])
def test_natural_order_in_place_is_echelonize_batch_dev(m, n, batch, full):
    width = (n + 63) // 64
    stride, bs = width + 1, m * (width + 1) + 3
    rng = np.random.default_rng(m + n)
    h, _idx, _valid = oc.pack([_member(rng, m, n, b) for b in range(batch)], m, n, stride, bs, 800 + m)
    mn = min(m, n)
    t1, t2 = (torch.from_numpy(h.view(np.int64).copy()).cuda() for _ in range(2))
    r1, r2 = (torch.full((batch,), -7, dtype=torch.int32, device="cuda") for _ in range(2))
    p1, p2 = (torch.full((batch * mn,), -7, dtype=torch.int32, device="cuda") for _ in range(2))
    torch.cuda.synchronize()
    m4ri_amd.echelonize_batch_dev(t1.data_ptr(), stride, bs, m, n, batch, full, r1.data_ptr(), p1.data_ptr())
    m4ri_amd.echelonize_order_batch_dev(t2.data_ptr(), stride, bs, t2.data_ptr(), stride, bs, m, n, m, 0, 0, n, batch, full, r2.data_ptr(), p2.data_ptr())
    torch.cuda.synchronize()
    assert torch.equal(t1, t2) and torch.equal(r1, r2) and torch.equal(p1, p2)
    assert not np.array_equal(t1.cpu().numpy().view(np.uint64), h)


def composition(D, stride, bs, A, m, n, batch, P, full, rank, pivots, stream=0):
    """All the library offered before: broadcast copy, gather the columns by transpositions, echelonize, scatter them back."""
    m4ri_amd.copy_block_batch_dev(D, stride, bs, 0, 0, A, stride, 0, 0, 0, m, n, batch, stream)
    m4ri_amd.apply_p_right_batch_dev(D, stride, bs, m, n, batch, P, n, n, False, 0, stream)
    m4ri_amd.echelonize_batch_dev(D, stride, bs, m, n, batch, full, rank, pivots, stream)
    m4ri_amd.apply_p_right_batch_dev(D, stride, bs, m, n, batch, P, n, n, True, 0, stream)


@pytest.mark.parametrize("m,n", [(33, 64), (64, 64), (70, 130), (64, 1024)])
@pytest.mark.parametrize("full", [0, 1])
def test_a_permutation_order_is_the_four_launch_composition(m, n, full):
    batch, width = 6, (n + 63) // 64
    stride, bs = width + 1, m * (width + 1) + 3
    rng = np.random.default_rng(m * n)
    hA, _i, _v = oc.pack([_member(rng, m, n, 1)], m, n, stride, m * stride, 900 + m)
    hD, _i, _v = oc.pack([_member(rng, m, n, 0) for _ in range(batch)], m, n, stride, bs, 901 + m)
    orders = np.stack([rng.permutation(n).astype(np.int32) for _ in range(batch)])
    P = np.stack([oc.transpositions(o) for o in orders])
    mn = min(m, n)
    tA, tO, tP = torch.from_numpy(hA.view(np.int64)).cuda(), torch.from_numpy(orders).cuda(), torch.from_numpy(P).cuda()
    t1, t2 = (torch.from_numpy(hD.view(np.int64).copy()).cuda() for _ in range(2))
    r1, r2 = (torch.full((batch,), -7, dtype=torch.int32, device="cuda") for _ in range(2))
    p1, p2 = (torch.full((batch * mn,), -7, dtype=torch.int32, device="cuda") for _ in range(2))
    torch.cuda.synchronize()
    composition(t1.data_ptr(), stride, bs, tA.data_ptr(), m, n, batch, tP.data_ptr(), full, r1.data_ptr(), p1.data_ptr())
    m4ri_amd.echelonize_order_batch_dev(t2.data_ptr(), stride, bs, tA.data_ptr(), stride, 0, m, n, m, tO.data_ptr(), n, n, batch, full, r2.data_ptr(),
                                        p2.data_ptr())
    torch.cuda.synchronize()
    assert torch.equal(t1, t2) and torch.equal(r1, r2)
    a, b = p1.cpu().numpy().reshape(batch, mn), p2.cpu().numpy().reshape(batch, mn)   # the composition's pivots are positions in the order
    for i in range(batch):
        assert np.array_equal(np.where(a[i] >= 0, orders[i][np.maximum(a[i], 0)], -1), b[i])


# ---- the random orders and the pipeline ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 1000, 4096])
@pytest.mark.parametrize("batch", [1, 37])
def test_random_orders_match_the_host(n, batch):
    o_bs, seed = n + 5, 1234567 + n
    t = torch.full(((batch - 1) * o_bs + n + 5,), -7, dtype=torch.int32, device="cuda")
    want = t.cpu().numpy().copy()
    for b in range(batch):
        want[b * o_bs: b * o_bs + n] = m4ri_amd.random_order(seed, b, n)
    m4ri_amd.random_orders_batch_dev(t.data_ptr(), o_bs, n, batch, seed)
    torch.cuda.synchronize()
    assert np.array_equal(t.cpu().numpy(), want)


class Pipeline:
    """One iteration of Lee-Brickell for 32 members on the device, three calls and no host round trip: random orders, systematic forms
    of one shared generator, the lightest single row and the lightest sum of two rows."""

    def __init__(self):
        self.G, self.orders, self.forms, self.lightest = pipeline()
        self.k, self.n, self.batch = self.G.shape[0], self.G.shape[1], len(self.orders)
        self.tG = torch.from_numpy(Mzd.from_bits(self.G).valid_words().copy().view(np.int64).reshape(-1)).cuda()
        self.fresh()

    def fresh(self):
        self.tO = torch.full((self.batch * self.n,), -7, dtype=torch.int32, device="cuda")
        self.tD = torch.full((self.batch * self.k,), -7, dtype=torch.int64, device="cuda")
        self.tr = torch.full((self.batch,), -7, dtype=torch.int32, device="cuda")
        self.tp = torch.full((self.batch * self.k,), -7, dtype=torch.int32, device="cuda")
        self.tl = torch.full((2, self.batch), -7, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()

    def launch(self, stream=0):
        k, n, batch = self.k, self.n, self.batch
        m4ri_amd.random_orders_batch_dev(self.tO.data_ptr(), n, n, batch, 7, stream)
        m4ri_amd.echelonize_order_batch_dev(self.tD.data_ptr(), 1, k, self.tG.data_ptr(), 1, 0, k, n, k, self.tO.data_ptr(), n, n, batch, 1,
                                            self.tr.data_ptr(), self.tp.data_ptr(), stream)
        for t in (1, 2):
            m4ri_amd.row_sums_weights_batch_dev(self.tD.data_ptr(), 1, k, k, n, 0, 0, batch, t, 1, 0, self.tl[t - 1].data_ptr(), stream)

    def untouched(self):
        return bool((self.tl == -7).all()) and bool((self.tr == -7).all()) and bool((self.tO == -7).all())

    def check(self):
        assert np.array_equal(self.tO.cpu().numpy().reshape(self.batch, self.n), np.stack(self.orders))
        D = self.tD.cpu().numpy().view(np.uint64).reshape(self.batch, self.k, 1)
        for b, (S, r, piv) in enumerate(self.forms):
            assert np.array_equal(D[b], oc.to_words(S)), b
            assert self.tr[b].item() == r and np.array_equal(self.tp.cpu().numpy()[b * self.k:][: self.k], piv), b
        assert self.tl.cpu().numpy().tolist() == self.lightest     # member by member, t = 1 and t = 2


def test_lee_brickell_iteration_matches_the_numpy_pipeline():
    p = Pipeline()
    p.launch()
    torch.cuda.synchronize()
    p.check()
    best = (torch.minimum(p.tl[0], p.tl[1]) >> 40).cpu().numpy()
    assert best.min() == 16 and int((best == 16).sum()) == 9      # the minimum distance, as tests/test_echelonize_order_plan.py found it


def test_pipeline_on_a_side_stream_and_captured_into_a_graph():
    """The five calls are plain launches on the stream they are given: a side stream first; then a capture, during which nothing runs
    (the outputs keep their dirt), and one replay.  One stream: the captured graph is a single chain without parallel branches."""
    p = Pipeline()
    side = torch.cuda.Stream()
    p.launch(side.cuda_stream)
    side.synchronize()
    p.check()
    p.fresh()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        p.launch(torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert p.untouched()
    g.replay()
    torch.cuda.synchronize()
    p.check()
