"""m4ri_amd_mul_small_batch_op_dev (include/m4ri_amd.h, mul_small_batch.hip): C_b (+)= op(A_b) * op(B_b) with A stored l x m and / or B
stored n x l, one launch for the batch, against NumPy's integer product mod 2 of the transposed bit arrays.  C starts dirty
everywhere -- valid bits, tail bits, padding words, gaps -- and A and B are dirty in the excess bits of their STORED last words, in
their padding and between members; every word of C's buffer is compared with the expected image, and A and B with what they were."""
import numpy as np
import pytest
import torch

import m4ri_amd
from m4ri_amd.mzd import Mzd
from test_gpu_echelonize_batch import _pack

pytestmark = pytest.mark.gpu
OVERRIDE = "M4RI_AMD_MUL_SMALL_BATCH_PATH1_MAX"
NT, TN, TT = (0, 1), (1, 0), (1, 1)
OPS = [NT, TN, TT]
OP_IDS = ["NT", "TN", "TT"]


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    assert m4ri_amd.lib().m4ri_amd_device_count() >= 1, "no HIP device visible: the gpu tests have nothing to run on"
    m4ri_amd.init(0)
    torch.cuda.set_device(0)


def _words(n):
    return (n + 63) // 64


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


def _device(h):
    return torch.from_numpy(h.view(np.int64).copy()).cuda()


class Case:
    """One batch on the device, the operands as stored, with the expected image of C."""

    def __init__(self, m, l, n, batch, op, add, share_a=False, share_b=False, gram=False, dense=False, seed=0, kinds=()):
        ta, tb = op
        self.m, self.l, self.n, self.batch, self.ta, self.tb, self.add = m, l, n, batch, ta, tb, add
        self.ra, self.ca = (l, m) if ta else (m, l)  # A as stored
        self.rb, self.cb = (n, l) if tb else (l, n)  # B as stored
        wa, wb, wn = _words(self.ca), _words(self.cb), _words(n)
        kind = lambda b: kinds[b] if b < len(kinds) else "random"
        na, nb = (1 if share_a else batch), (1 if share_b else batch)
        self.A = [_special(kind(b), self.ra, self.ca, seed + 3 * b) for b in range(na)]
        self.B = self.A if gram else [_special(kind(b + 1), self.rb, self.cb, seed + 3 * b + 1) for b in range(nb)]
        self.C = [Mzd.random(m, n, seed + 3 * b + 2) for b in range(batch)]
        if dense:
            self.sa, self.sb, self.sc = wa, wb, wn
            self.abs, self.bbs, self.cbs = self.ra * wa, self.rb * wb, m * wn
        else:  # odd gaps: rows, members
            self.sa, self.sb, self.sc = wa + 1, wb + 3, wn + 1
            self.abs, self.bbs, self.cbs = self.ra * self.sa + 3, self.rb * self.sb + 5, m * self.sc + 7
        if share_a:
            self.abs = 0
        if share_b:
            self.bbs = 0
        self.hA, _, _ = _image(self.A, self.ra, self.ca, self.sa, self.abs, seed + 1000)
        self.hC, self.idx, self.valid = _image(self.C, m, n, self.sc, self.cbs, seed + 3000)
        self.tA = _device(self.hA)
        if gram:  # B is A: the same pointer, the same stored shape
            assert (self.ra, self.ca) == (self.rb, self.cb) and ta != tb
            self.sb, self.bbs, self.hB, self.tB = self.sa, self.abs, self.hA, self.tA
        else:
            self.hB, _, _ = _image(self.B, self.rb, self.cb, self.sb, self.bbs, seed + 2000)
            self.tB = _device(self.hB)
        self.tC = _device(self.hC)
        self.exp = self.hC.copy()
        if self.idx is not None:
            for b in range(batch):
                a = self.A[b if len(self.A) > 1 else 0].to_bits().astype(np.int64)
                bb = self.B[b if len(self.B) > 1 else 0].to_bits().astype(np.int64)
                bits = (a.T if ta else a) @ (bb.T if tb else bb)
                if add:
                    bits = bits + self.C[b].to_bits()
                want = Mzd.from_bits((bits & 1).astype(np.uint8))
                self.exp[self.idx[b]] = (self.hC[self.idx[b]] & ~self.valid) | (want.valid_words() & self.valid)
        torch.cuda.synchronize()

    def args(self, tC=None):
        return ((tC if tC is not None else self.tC).data_ptr(), self.sc, self.cbs, self.tA.data_ptr(), self.sa, self.abs, self.tB.data_ptr(), self.sb,
                self.bbs, self.m, self.l, self.n, self.batch)

    def call(self, stream=0):
        m4ri_amd.mul_small_batch_op_dev(*self.args(), trans_a=bool(self.ta), trans_b=bool(self.tb), add=bool(self.add), stream=stream)

    def got(self, t=None):
        torch.cuda.synchronize()
        return (self.tC if t is None else t).cpu().numpy().view(np.uint64)

    def check(self, exp=None):
        """Every word of C's buffer; A and B as they were."""
        got, exp = self.got(), self.exp if exp is None else exp
        bad = np.flatnonzero(got != exp)
        assert bad.size == 0, f"{bad.size} words of C differ, first at {bad[:5]} (member {bad[0] // self.cbs if self.cbs else 0})"
        assert np.array_equal(self.tA.cpu().numpy().view(np.uint64), self.hA), "A was written"
        assert np.array_equal(self.tB.cpu().numpy().view(np.uint64), self.hB), "B was written"

    def run(self):
        self.call()
        self.check()


def _seed(*xs):
    return sum((i + 1) * 131 * x for i, x in enumerate(xs))


# 32 / 33 in n: the HI split; (40, 63, 32) and (40, 63, 33) its two sides with stored operands of 63 columns and rows
PATH0 = [(1, 1, 1), (64, 64, 64), (33, 64, 31), (31, 33, 64), (64, 1, 64), (17, 5, 64), (40, 63, 32), (40, 63, 33), (9, 0, 21)]


@pytest.mark.parametrize("m,l,n", PATH0)
@pytest.mark.parametrize("op", OPS, ids=OP_IDS)
@pytest.mark.parametrize("add", [0, 1])
def test_wave_path(m, l, n, op, add):
    assert m4ri_amd.plan_mul_small_batch_op(m, l, n, *op) == 0
    Case(m, l, n, 5, op, add, seed=_seed(m, l, n)).run()


@pytest.mark.parametrize("batch", [1, 2, 3, 4, 5, 9])
@pytest.mark.parametrize("op", OPS, ids=OP_IDS)
@pytest.mark.parametrize("add", [0, 1])
def test_wave_path_batches(batch, op, add):
    """Batches around the four members of a workgroup: the waves past the batch leave."""
    Case(50, 37, 61, batch, op, add, seed=200 + batch).run()


@pytest.mark.parametrize("how", ["share_a", "share_b", "dense"])
@pytest.mark.parametrize("op", OPS, ids=OP_IDS)
@pytest.mark.parametrize("add", [0, 1])
def test_wave_path_shared_operands_and_unit_strides(how, op, add):
    c = Case(64, 64, 64, 6, op, add, seed=300, **{how: True})
    assert (how != "share_a" or c.abs == 0) and (how != "share_b" or c.bbs == 0)
    assert how != "dense" or (c.sa, c.sb, c.sc, c.abs, c.bbs, c.cbs) == (1, 1, 1, 64, 64, 64)
    c.run()


@pytest.mark.parametrize("m,l", [(64, 64), (45, 29)])
@pytest.mark.parametrize("op", [NT, TN], ids=["A.At", "At.A"])
@pytest.mark.parametrize("add", [0, 1])
def test_wave_path_gram(m, l, op, add):
    """B == A, the same pointer: A A^T of A stored m x l, A^T A of A stored l x m."""
    c = Case(m, l, m, 5, op, add, gram=True, seed=400 + m)
    assert c.tA.data_ptr() == c.tB.data_ptr() and (c.sa, c.abs) == (c.sb, c.bbs)
    c.run()
    got = c.got()
    for b in range(c.batch if not add else 0):  # a Gram matrix is symmetric
        G = Mzd(m, m)
        G.valid_words()[:, :] = got[c.idx[b]]
        assert np.array_equal(G.to_bits(), G.to_bits().T), b


PATH1 = [(65, 64, 64), (64, 65, 64), (64, 64, 65), (100, 130, 70), (129, 191, 65), (256, 256, 256)]


@pytest.mark.parametrize("m,l,n", PATH1)
@pytest.mark.parametrize("op", OPS, ids=OP_IDS)
@pytest.mark.parametrize("add", [0, 1])
def test_block_path(monkeypatch, m, l, n, op, add):
    monkeypatch.setenv(OVERRIDE, "256")  # path 1 whatever D1op is
    Case(m, l, n, 3, op, add, seed=_seed(m, l, n) + 1).run()


@pytest.mark.parametrize("op", OPS, ids=OP_IDS)
@pytest.mark.parametrize("add", [0, 1])
def test_block_path_identity_and_all_ones(monkeypatch, op, add):
    """Members a lane or bit-order slip cannot cancel in: stored A_0 = I, stored B_0 = A_1 = all ones, B_1 = I."""
    monkeypatch.setenv(OVERRIDE, "256")
    Case(128, 100, 128, 3, op, add, seed=600, kinds=("identity", "ones", "identity")).run()


@pytest.mark.parametrize("op", OPS, ids=OP_IDS)
def test_block_path_shared_b_and_inner_dimension_zero(monkeypatch, op):
    monkeypatch.setenv(OVERRIDE, "256")
    Case(129, 191, 65, 4, op, 1, share_b=True, seed=700).run()
    Case(100, 0, 70, 3, op, 0, seed=710).run()
    Case(100, 0, 70, 3, op, 1, seed=720).run()


@pytest.mark.parametrize("op", [NT, TN], ids=["A.At", "At.A"])
@pytest.mark.parametrize("add", [0, 1])
def test_block_path_gram(monkeypatch, op, add):
    monkeypatch.setenv(OVERRIDE, "256")
    Case(100, 130, 100, 3, op, add, gram=True, seed=800).run()


@pytest.mark.parametrize("m,l,n", [(40, 63, 33), (129, 191, 65)])
@pytest.mark.parametrize("op", OPS, ids=OP_IDS)
@pytest.mark.parametrize("add", [0, 1])
def test_equals_transpose_then_multiply(monkeypatch, m, l, n, op, add):
    """One shape per path: the whole buffer of C is what m4ri_amd_transpose_batch_dev of the transposed operands into scratch tensors
    followed by m4ri_amd_mul_small_batch_dev leaves from the same dirty start."""
    monkeypatch.setenv(OVERRIDE, "256")
    c = Case(m, l, n, 5, op, add, seed=_seed(m, l, n) + 2)
    tR = c.tC.clone()
    a = (c.tA.data_ptr(), c.sa, c.abs)
    b = (c.tB.data_ptr(), c.sb, c.bbs)
    keep = []
    if c.ta:  # stored l x m -> m x l
        sA = torch.zeros(c.batch * m * _words(l), dtype=torch.int64, device="cuda")
        m4ri_amd.transpose_batch_dev(sA.data_ptr(), _words(l), m * _words(l), *a, l, m, c.batch)
        a = (sA.data_ptr(), _words(l), m * _words(l))
        keep.append(sA)
    if c.tb:  # stored n x l -> l x n
        sB = torch.zeros(c.batch * l * _words(n), dtype=torch.int64, device="cuda")
        m4ri_amd.transpose_batch_dev(sB.data_ptr(), _words(n), l * _words(n), *b, n, l, c.batch)
        b = (sB.data_ptr(), _words(n), l * _words(n))
        keep.append(sB)
    m4ri_amd.mul_small_batch_dev(tR.data_ptr(), c.sc, c.cbs, *a, *b, m, l, n, c.batch, add=bool(add))
    c.run()
    assert np.array_equal(c.got(), c.got(tR))


@pytest.mark.parametrize("m,l,n,path", [(40, 63, 33, 0), (129, 191, 65, 1), (65, 64, 64, 2)])
@pytest.mark.parametrize("add", [0, 1])
def test_untransposed_is_mul_small_batch_dev(monkeypatch, m, l, n, path, add):
    """trans_a == trans_b == 0: the same whole buffer as m4ri_amd_mul_small_batch_dev on paths 0 and 1; on path 2 (the override at 64
    sends 65 x 64 x 64 there) the launch of m4ri_amd_m4rm_batch_dev, compared on the valid bits, which are the product."""
    monkeypatch.setenv(OVERRIDE, "64" if path == 2 else "256")
    c = Case(m, l, n, 5, (0, 0), add, seed=_seed(m, l, n) + 3)
    tR = c.tC.clone()
    m4ri_amd.mul_small_batch_dev(*c.args(tR), add=bool(add))
    marker = torch.zeros(7 * 64, dtype=torch.int64, device="cuda")  # a product of another batch size through the engine
    assert m4ri_amd.lib().m4ri_amd_m4rm_batch_dev(marker.data_ptr(), 1, 64, c.tA.data_ptr(), c.sa, 0, c.tB.data_ptr(), c.sb, 0, 1, 1, 1, 7, 0, None) == 0
    c.call()
    got, ref = c.got(), c.got(tR)
    assert int(m4ri_amd.get_stats().leaf_products) == (5 if path == 2 else 7)  # whether the engine ran this batch
    if path != 2:
        c.check()
        assert np.array_equal(got, ref)
    else:
        assert np.array_equal(got[c.idx] & c.valid, ref[c.idx] & c.valid)
        assert np.array_equal(got[c.idx] & c.valid, c.exp[c.idx] & c.valid)


@pytest.mark.parametrize("op", OPS, ids=OP_IDS)
def test_override_makes_a_transposed_call_unsupported(monkeypatch, op):
    """With the override at 64 path 1 is empty: a transposed 65 x 64 x 64 call raises hipErrorNotSupported and leaves C untouched."""
    monkeypatch.setenv(OVERRIDE, "64")
    c = Case(65, 64, 64, 3, op, 0, seed=900)
    with pytest.raises(RuntimeError, match="801"):
        c.call()
    c.check(exp=c.hC)
    monkeypatch.setenv(OVERRIDE, "128")  # read per call
    c.run()


def test_on_a_side_stream(monkeypatch):
    monkeypatch.setenv(OVERRIDE, "256")
    s = torch.cuda.Stream()
    for (m, l, n), op in [((64, 64, 64), NT), ((129, 191, 65), TT)]:
        c = Case(m, l, n, 5, op, 1, seed=1000 + m)
        c.call(stream=s.cuda_stream)
        s.synchronize()
        c.check()


def test_captured_into_a_graph():
    """A plain launch: captured on one stream (nothing runs, C keeps its dirt), then replayed twice with add = 1.  The first replay
    leaves C + A B^T, the second adds the product again: over GF(2) that is C as it started, which only both replays give."""
    c = Case(50, 37, 61, 5, NT, 1, seed=1100)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        c.call(stream=torch.cuda.current_stream().cuda_stream)
    c.check(exp=c.hC)
    g.replay()
    c.check()
    assert not np.array_equal(c.exp, c.hC)
    g.replay()
    c.check(exp=c.hC)
