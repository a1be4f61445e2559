"""m4ri_amd_mul_small_batch_dev (include/m4ri_amd.h, mul_small_batch.hip): `batch` products of tiny matrices in one call, every member
against the oracle's gf2o_mul / gf2o_addmul (mzd_mul / mzd_addmul) on all three paths of m4ri_amd_plan_mul_small_batch, and a few
members against NumPy's integer product mod 2.  C starts dirty everywhere -- valid bits, tail bits, padding words, gaps -- A and B
are dirty in their excess bits and padding; on paths 0 and 1 every word and bit outside C's valid bits must come out unchanged."""
import numpy as np
import pytest
import torch

import m4ri_amd
from m4ri_amd.mzd import Mzd
from test_gpu_echelonize_batch import _pack

pytestmark = pytest.mark.gpu
OVERRIDE = "M4RI_AMD_MUL_SMALL_BATCH_PATH1_MAX"


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    assert m4ri_amd.lib().m4ri_amd_device_count() >= 1, "no HIP device visible: the gpu tests have nothing to run on"
    m4ri_amd.init(0)
    torch.cuda.set_device(0)


def _d1():
    return max(d for d in (64, 128, 192, 256) if m4ri_amd.plan_mul_small_batch(d, d, d) != 2)


def _planned(m, l, n):
    """The path of the plan function, from its own D1."""
    mx = max(m, l, n)
    return 0 if mx <= 64 else 1 if mx <= _d1() else 2


def _image(members, rows, cols, stride, bs, seed):
    """Dirty host image of one operand (tests/test_gpu_echelonize_batch._pack); an empty operand is all dirt."""
    if rows == 0 or cols == 0:
        rng = np.random.default_rng(seed)
        total = (len(members) - 1) * bs + rows * stride + 5
        return rng.integers(0, 1 << 63, size=total, dtype=np.int64).view(np.uint64) * np.uint64(3), None, None
    return _pack(members, rows, cols, stride, bs, seed)


def _special(kind, rows, cols, seed):
    if kind == "identity":
        return Mzd.from_bits(np.eye(rows, cols, dtype=np.uint8))
    if kind == "ones":
        return Mzd.from_bits(np.ones((rows, cols), dtype=np.uint8))
    return Mzd.random(rows, cols, seed)


class Case:
    """One batch on the device with its expected image of C."""

    def __init__(self, oracle, m, l, n, batch, add, share_a=False, share_b=False, square=False, dense=False, seed=0, kinds=()):
        self.m, self.l, self.n, self.batch, self.add = m, l, n, batch, add
        wl, wn = (l + 63) // 64, (n + 63) // 64
        kind = lambda b: kinds[b] if b < len(kinds) else "random"
        na, nb = (1 if share_a else batch), (1 if share_b or square else batch)
        self.A = [_special(kind(b), m, l, seed + 3 * b) for b in range(na)]
        self.B = self.A if square else [_special(kind(b + 1), l, n, seed + 3 * b + 1) for b in range(nb)]
        self.C = [Mzd.random(m, n, seed + 3 * b + 2) for b in range(batch)]
        if dense:
            self.sa, self.sb, self.sc = wl, wn, wn
            self.abs, self.bbs, self.cbs = m * wl, l * wn, m * wn
        else:  # odd gaps: rows, members
            self.sa, self.sb, self.sc = wl + 1, wn + 3, wn + 1
            self.abs, self.bbs, self.cbs = m * self.sa + 3, l * self.sb + 5, m * self.sc + 7
        if share_a:
            self.abs = 0
        if share_b:
            self.bbs = 0
        self.hA, _, _ = _image(self.A, m, l, self.sa, self.abs, seed + 1000)
        self.hC, self.idx, self.valid = _image(self.C, m, n, self.sc, self.cbs, seed + 3000)
        self.tA = torch.from_numpy(self.hA.view(np.int64).copy()).cuda()
        if square:
            assert (m, l) == (l, n)
            self.sb, self.bbs, self.hB, self.tB = self.sa, self.abs, self.hA, self.tA
        else:
            self.hB, _, _ = _image(self.B, l, n, self.sb, self.bbs, seed + 2000)
            self.tB = torch.from_numpy(self.hB.view(np.int64).copy()).cuda()
        self.tC = torch.from_numpy(self.hC.view(np.int64).copy()).cuda()
        self.exp = self.hC.copy()
        if self.idx is not None:
            for b in range(batch):
                want = self.C[b].copy() if add else Mzd(m, n)
                (oracle.addmul if add else oracle.mul)(want, self.a(b), self.b(b), 0)
                self.exp[self.idx[b]] = (self.hC[self.idx[b]] & ~self.valid) | (want.valid_words() & self.valid)
        torch.cuda.synchronize()

    def a(self, b):
        return self.A[b if len(self.A) > 1 else 0]

    def b(self, b):
        return self.B[b if len(self.B) > 1 else 0]

    def args(self, tC=None):
        return ((tC if tC is not None else self.tC).data_ptr(), self.sc, self.cbs, self.tA.data_ptr(), self.sa, self.abs, self.tB.data_ptr(), self.sb,
                self.bbs, self.m, self.l, self.n, self.batch)

    def call(self, stream=0):
        m4ri_amd.mul_small_batch_dev(*self.args(), add=bool(self.add), stream=stream)

    def check(self, whole=True):
        """whole: every word of C's buffer (paths 0 and 1); else the valid bits alone (path 2: m4ri_amd_m4rm_batch_dev's contract)."""
        torch.cuda.synchronize()
        got = self.tC.cpu().numpy().view(np.uint64)
        if whole:
            bad = np.flatnonzero(got != self.exp)
            assert bad.size == 0, f"{bad.size} words of C differ, first at {bad[:5]} (member {bad[0] // self.cbs if self.cbs else 0})"
        else:
            assert np.array_equal(got[self.idx] & self.valid, self.exp[self.idx] & self.valid)
        assert np.array_equal(self.tA.cpu().numpy().view(np.uint64), self.hA), "A was written"
        assert np.array_equal(self.tB.cpu().numpy().view(np.uint64), self.hB), "B was written"
        if self.idx is not None:
            for b in sorted({0, self.batch // 2, self.batch - 1}):  # the second check: NumPy's integer product mod 2
                bits = self.a(b).to_bits().astype(np.int64) @ self.b(b).to_bits().astype(np.int64)
                if self.add:
                    bits = bits + self.C[b].to_bits()
                G = Mzd(self.m, self.n)
                G.valid_words()[:, :] = got[self.idx[b]]
                assert np.array_equal(G.to_bits(), (bits & 1).astype(np.uint8)), b


PATH0 = [(1, 1, 1), (64, 64, 64), (63, 64, 1), (1, 64, 64), (37, 5, 64), (64, 33, 17), (17, 64, 33), (64, 64, 63), (5, 0, 7)]


@pytest.mark.parametrize("m,l,n", PATH0)
@pytest.mark.parametrize("add", [0, 1])
def test_wave_path_matches_oracle(oracle, m, l, n, add):
    assert m4ri_amd.plan_mul_small_batch(m, l, n) == _planned(m, l, n) == 0
    c = Case(oracle, m, l, n, 5, add, seed=100 + m + 2 * l + 3 * n)
    c.call()
    c.check()


@pytest.mark.parametrize("m,l,n", [(64, 64, 64), (37, 5, 64), (17, 64, 33)])
@pytest.mark.parametrize("batch", [1, 257])
@pytest.mark.parametrize("add", [0, 1])
def test_wave_path_batches(oracle, m, l, n, batch, add):
    """Batches that are no multiple of the four members of a workgroup: the last workgroup of 257 members holds one."""
    c = Case(oracle, m, l, n, batch, add, seed=200 + m + batch)
    c.call()
    c.check()


@pytest.mark.parametrize("m,l,n", [(0, 5, 5), (5, 5, 0), (0, 0, 0)])
@pytest.mark.parametrize("add", [0, 1])
def test_empty_results_touch_nothing(oracle, m, l, n, add):
    assert m4ri_amd.plan_mul_small_batch(m, l, n) == 0
    c = Case(oracle, m, l, n, 5, add, seed=300 + m + n)
    c.call()
    c.check()


@pytest.mark.parametrize("add", [0, 1])
def test_wave_path_dense_unit_stride(oracle, add):
    """x_stride == 1, members back to back: a wave's load is one 512-byte run, and there is no frame to hide a slip in."""
    c = Case(oracle, 64, 64, 64, 9, add, dense=True, seed=400)
    assert (c.sa, c.sb, c.sc, c.abs, c.bbs, c.cbs) == (1, 1, 1, 64, 64, 64)
    c.call()
    c.check()


@pytest.mark.parametrize("how", ["share_a", "share_b", "square"])
@pytest.mark.parametrize("add", [0, 1])
def test_wave_path_shared_operands(oracle, how, add):
    c = Case(oracle, 64, 64, 64, 6, add, seed=500, **{how: True})
    assert (how != "share_a" or c.abs == 0) and (how != "share_b" or c.bbs == 0)
    assert how != "square" or (c.tA.data_ptr() == c.tB.data_ptr() and (c.sa, c.abs) == (c.sb, c.bbs))
    c.call()
    c.check()


@pytest.mark.parametrize("m,l,n", [(64, 64, 64), (37, 64, 50)])
@pytest.mark.parametrize("add", [0, 1])
def test_wave_path_identity_and_all_ones(oracle, m, l, n, add):
    """Members a lane or bit-order slip cannot cancel in: A_0 = I, B_0 = A_1 = all ones, B_1 = I."""
    c = Case(oracle, m, l, n, 3, add, seed=600, kinds=("identity", "ones", "identity"))
    c.call()
    c.check()


PATH1 = [(65, 64, 64), (64, 65, 64), (64, 64, 65), (128, 128, 128), (129, 191, 70), (200, 130, 100), (256, 256, 256), (100, 256, 1), (1, 200, 256)]


@pytest.mark.parametrize("m,l,n", PATH1)
@pytest.mark.parametrize("add", [0, 1])
def test_block_path_matches_oracle(oracle, monkeypatch, m, l, n, add):
    assert m4ri_amd.plan_mul_small_batch(m, l, n) == _planned(m, l, n) != 0
    monkeypatch.setenv(OVERRIDE, "256")  # path 1 whatever D1 is
    c = Case(oracle, m, l, n, 3, add, seed=700 + m + 2 * l + 3 * n)
    c.call()
    c.check()


@pytest.mark.parametrize("batch", [1, 6])
@pytest.mark.parametrize("share", [None, "share_b", "share_a"])
def test_block_path_batches_and_shared_operands(oracle, monkeypatch, batch, share):
    monkeypatch.setenv(OVERRIDE, "256")
    c = Case(oracle, 129, 191, 70, batch, batch % 2, seed=800 + batch, **({share: True} if share else {}))
    c.call()
    c.check()


def test_block_path_inner_dimension_zero_and_identity(oracle, monkeypatch):
    monkeypatch.setenv(OVERRIDE, "256")
    for add in (0, 1):
        c = Case(oracle, 100, 0, 70, 3, add, seed=850)
        c.call()
        c.check()
    c = Case(oracle, 130, 130, 130, 3, 1, seed=860, kinds=("identity", "ones", "identity"))
    c.call()
    c.check()


@pytest.mark.parametrize("m,l,n,share", [(300, 200, 600, None), (257, 64, 64, None), (300, 200, 600, "share_b"), (257, 64, 64, "share_a")])
@pytest.mark.parametrize("add", [0, 1])
def test_forwarded_path_matches_oracle(oracle, monkeypatch, m, l, n, share, add):
    monkeypatch.delenv(OVERRIDE, raising=False)
    assert m4ri_amd.plan_mul_small_batch(m, l, n) == _planned(m, l, n) == 2
    c = Case(oracle, m, l, n, 3, add, seed=900 + m, **({share: True} if share else {}))
    c.call()
    c.check(whole=False)


@pytest.mark.parametrize("m,l,n,path", [(64, 33, 17, 0), (129, 191, 70, 1), (300, 200, 600, 2)])
@pytest.mark.parametrize("add", [0, 1])
def test_same_valid_bits_as_m4rm_batch_dev(oracle, monkeypatch, m, l, n, path, add):
    """One shape per path against m4ri_amd_m4rm_batch_dev on a copy of the same buffers, and the path a call really took: the engine's
    leaf statistics belong to the last product that went through the engine, which a call on path 0 or 1 is not."""
    if path == 1:
        monkeypatch.setenv(OVERRIDE, "256")
    else:
        monkeypatch.delenv(OVERRIDE, raising=False)
        assert m4ri_amd.plan_mul_small_batch(m, l, n) == path
    c = Case(oracle, m, l, n, 5, add, seed=1000 + m)
    tR = c.tC.clone()
    assert m4ri_amd.lib().m4ri_amd_m4rm_batch_dev(*c.args(tR), add, None) == 0
    torch.cuda.synchronize()
    assert int(m4ri_amd.get_stats().leaf_products) == 5
    marker = torch.zeros(7 * 64, dtype=torch.int64, device="cuda")  # a product of another batch size through the engine
    assert m4ri_amd.lib().m4ri_amd_m4rm_batch_dev(marker.data_ptr(), 1, 64, c.tA.data_ptr(), c.sa, 0, c.tB.data_ptr(), c.sb, 0, 1, 1, 1, 7, 0, None) == 0
    assert int(m4ri_amd.get_stats().leaf_products) == 7
    c.call()
    c.check(whole=path != 2)
    assert int(m4ri_amd.get_stats().leaf_products) == (5 if path == 2 else 7)
    got, ref = c.tC.cpu().numpy().view(np.uint64), tR.cpu().numpy().view(np.uint64)
    assert np.array_equal(got[c.idx] & c.valid, ref[c.idx] & c.valid)


def test_override_is_clamped_and_read_per_call(oracle, monkeypatch):
    """(65, 64, 64) is path 1 for every override the clamp lets through and for a D1 above 64; with the override at 64 it is forwarded."""
    for value, block in [("256", True), ("100000", True), ("128", True), ("127", False), ("64", False), ("0", False)]:
        monkeypatch.setenv(OVERRIDE, value)
        marker = torch.zeros(7 * 64, dtype=torch.int64, device="cuda")
        c = Case(oracle, 65, 64, 64, 2, 0, seed=1100)
        assert m4ri_amd.lib().m4ri_amd_m4rm_batch_dev(marker.data_ptr(), 1, 64, c.tA.data_ptr(), c.sa, 0, c.tB.data_ptr(), c.sb, 0, 1, 1, 1, 7, 0, None) == 0
        c.call()
        c.check(whole=block)
        assert int(m4ri_amd.get_stats().leaf_products) == (7 if block else 2), value


def test_on_a_side_stream(oracle, monkeypatch):
    monkeypatch.setenv(OVERRIDE, "256")
    s = torch.cuda.Stream()
    for (m, l, n) in [(64, 64, 64), (129, 191, 70)]:
        c = Case(oracle, m, l, n, 5, 1, seed=1200 + m)
        c.call(stream=s.cuda_stream)
        s.synchronize()
        c.check()


def test_captured_into_a_graph(oracle):
    """A path-0 call is a plain launch: captured (nothing runs, C keeps its dirt), then replayed once.  One branch, default queues."""
    c = Case(oracle, 64, 33, 17, 5, 0, seed=1300)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        c.call(stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert np.array_equal(c.tC.cpu().numpy().view(np.uint64), c.hC)
    g.replay()
    c.check()
