"""m4ri_amd_transpose_batch_dev (include/m4ri_amd.h, transpose_batch.hip): `batch` transposes of small matrices in one call, every
member against NumPy's .T on the unpacked bits, on all three paths of m4ri_amd_plan_transpose_batch and in place.  D starts dirty
everywhere -- valid bits, tail bits, padding words, gaps -- and A is dirty in its excess bits and padding; on paths 0 and 1 and in
place every word and bit outside D's valid bits must come out unchanged, on path 2 D's last words are written whole (tail bits zero,
m4ri_amd_transpose_dev's contract) and everything else is unchanged."""
import numpy as np
import pytest
import torch

import m4ri_amd
from m4ri_amd.mzd import Mzd
from test_gpu_echelonize_batch import _pack

pytestmark = pytest.mark.gpu
OVERRIDE = "M4RI_AMD_TRANSPOSE_BATCH_PATH1_MAX"


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    assert m4ri_amd.lib().m4ri_amd_device_count() >= 1, "no HIP device visible: the gpu tests have nothing to run on"
    m4ri_amd.init(0)
    torch.cuda.set_device(0)


def _w(n):
    return (n + 63) // 64


def _image(members, rows, cols, stride, bs, seed):
    """Dirty host image of one operand (tests/test_gpu_echelonize_batch._pack); an empty operand is all dirt."""
    if rows == 0 or cols == 0:
        rng = np.random.default_rng(seed)
        total = (len(members) - 1) * bs + rows * stride + 5
        return rng.integers(0, 1 << 63, size=total, dtype=np.int64).view(np.uint64) * np.uint64(3), None, None
    return _pack(members, rows, cols, stride, bs, seed)


def _bits(kind, rows, cols, seed):
    """The bits of one member.  kind: "random", "identity", "upper" (all ones strictly above the diagonal) or a single bit (r, c)."""
    if kind == "random":
        return Mzd.random(rows, cols, seed).to_bits()
    if kind == "identity":
        return np.eye(rows, cols, dtype=np.uint8)
    if kind == "upper":
        return np.triu(np.ones((rows, cols), dtype=np.uint8), 1)
    b = np.zeros((rows, cols), dtype=np.uint8)
    b[kind] = 1
    return b


def _cuda(h):
    return torch.from_numpy(h.view(np.int64).copy()).cuda()


def _host(t):
    return t.cpu().numpy().view(np.uint64)


class Case:
    """One batch on the device with the expected image of D.  The reference is computed once, here."""

    def __init__(self, nrows, ncols, batch, seed=0, dense=False, inplace=False, kinds=()):
        self.nrows, self.ncols, self.batch, self.inplace = nrows, ncols, batch, inplace
        wa, wd = _w(ncols), _w(nrows)
        if dense:
            self.sa, self.sd, self.abs, self.dbs = wa, wd, nrows * wa, ncols * wd
        else:  # odd gaps: rows, members
            self.sa, self.sd = wa + 1, wd + (1 if inplace else 3)
            self.abs, self.dbs = nrows * self.sa + 3, ncols * self.sd + (3 if inplace else 7)
        self.bits = [_bits(kinds[b] if b < len(kinds) else "random", nrows, ncols, seed + 3 * b) for b in range(batch)]
        A = [Mzd.from_bits(x) for x in self.bits] if nrows and ncols else [None] * batch
        self.hA, self.aidx, self.avalid = _image(A, nrows, ncols, self.sa, self.abs, seed + 1000)
        self.tA = _cuda(self.hA)
        if inplace:
            assert nrows == ncols and (self.sa, self.abs) == (self.sd, self.dbs)
            self.hD, self.idx, self.valid, self.tD = self.hA, self.aidx, self.avalid, self.tA
        else:
            Dm = [Mzd.random(ncols, nrows, seed + 3 * b + 2) for b in range(batch)] if nrows and ncols else [None] * batch
            self.hD, self.idx, self.valid = _image(Dm, ncols, nrows, self.sd, self.dbs, seed + 3000)
            self.tD = _cuda(self.hD)
        self.exp = self.hD.copy()          # paths 0 and 1, in place: the whole image
        self.ours = np.zeros(self.hD.size, dtype=bool)  # the words of D's valid widths
        if self.idx is not None:
            self.ours[self.idx] = True
            for b in range(batch):
                want = Mzd.from_bits(np.ascontiguousarray(self.bits[b].T))
                self.exp[self.idx[b]] = (self.hD[self.idx[b]] & ~self.valid) | (want.valid_words() & self.valid)
        torch.cuda.synchronize()

    def args(self, tD=None):
        return ((tD if tD is not None else self.tD).data_ptr(), self.sd, self.dbs, self.tA.data_ptr(), self.sa, self.abs, self.nrows, self.ncols, self.batch)

    def call(self, stream=0):
        m4ri_amd.transpose_batch_dev(*self.args(), stream=stream)

    def member(self, got, b):
        G = Mzd(self.ncols, self.nrows)
        G.valid_words()[:, :] = got[self.idx[b]]
        return G.to_bits()

    def check(self, whole=True):
        """whole: every word of D's buffer (paths 0 and 1, in place); else path 2's contract."""
        torch.cuda.synchronize()
        got = _host(self.tD)
        if whole:
            bad = np.flatnonzero(got != self.exp)
            assert bad.size == 0, f"{bad.size} words of D differ, first at {bad[:5]} (member {bad[0] // self.dbs if self.dbs else 0})"
        else:
            assert np.array_equal(got[self.idx] & self.valid, self.exp[self.idx] & self.valid), "valid bits"
            assert not (got[self.idx] & ~self.valid).any(), "the tail bits of D's last words are zero on path 2"
            assert np.array_equal(got[~self.ours], self.hD[~self.ours]), "padding words and gaps are not ours"
        if not self.inplace:
            assert np.array_equal(_host(self.tA), self.hA), "A was written"
        if self.idx is not None:
            for b in range(self.batch):  # the second check: the bits themselves
                assert np.array_equal(self.member(got, b), self.bits[b].T), b
        return got


PATH0 = [(1, 1), (64, 64), (63, 64), (64, 63), (1, 64), (64, 1), (37, 5), (5, 37), (33, 17), (32, 32)]


@pytest.mark.parametrize("nrows,ncols", PATH0)
def test_wave_path_matches_numpy(nrows, ncols):
    assert m4ri_amd.plan_transpose_batch(nrows, ncols) == 0
    c = Case(nrows, ncols, 5, seed=100 + nrows + 2 * ncols)
    c.call()
    c.check()


@pytest.mark.parametrize("nrows,ncols", [(0, 5), (5, 0)])
def test_empty_members_touch_nothing(nrows, ncols):
    c = Case(nrows, ncols, 5, seed=150 + nrows)
    c.call()
    c.check()


@pytest.mark.parametrize("nrows,ncols", [(64, 64), (37, 5)])
@pytest.mark.parametrize("batch", [1, 257])
def test_wave_path_batches(nrows, ncols, batch):
    """Batches that are no multiple of the four members of a workgroup: the last workgroup of 257 members holds one."""
    c = Case(nrows, ncols, batch, seed=200 + nrows + batch)
    c.call()
    c.check()


def test_wave_path_dense_unit_stride():
    """Strides of 1, members back to back: a wave's load is one 512-byte run, and there is no frame to hide a slip in."""
    c = Case(64, 64, 9, dense=True, seed=400)
    assert (c.sa, c.sd, c.abs, c.dbs) == (1, 1, 64, 64)
    c.call()
    c.check()


def _slips(nrows, ncols, singles):
    return ("identity", "upper") + tuple(s for s in singles if s[0] < nrows and s[1] < ncols)


def _check_slips(c, kinds):
    got = c.check()
    r, k = c.nrows, c.ncols
    assert np.array_equal(c.member(got, 0), np.eye(k, r, dtype=np.uint8))
    assert np.array_equal(c.member(got, 1), np.tril(np.ones((k, r), dtype=np.uint8), -1)), "strictly upper comes out strictly lower"
    for b, kind in enumerate(kinds[2:], start=2):
        out = c.member(got, b)
        assert out.sum() == 1 and out[kind[1], kind[0]] == 1, kind


@pytest.mark.parametrize("nrows,ncols", [(64, 64), (37, 50)])
def test_wave_path_members_that_cannot_hide_a_slip(nrows, ncols):
    """A symmetric or random member can hide a lane or bit-order slip; the identity, a strict triangle and single bits cannot."""
    kinds = _slips(nrows, ncols, [(0, 63), (63, 0), (31, 32), (0, ncols - 1), (nrows - 1, 0), (nrows - 1, ncols - 1), (nrows - 2, 1), (1, ncols - 2)])
    c = Case(nrows, ncols, len(kinds), seed=500, kinds=kinds)
    c.call()
    _check_slips(c, kinds)


def test_block_path_members_that_cannot_hide_a_slip(monkeypatch):
    monkeypatch.setenv(OVERRIDE, "1024")
    kinds = _slips(130, 70, [(63, 64), (64, 63), (129, 0), (0, 69), (129, 69), (64, 64), (63, 63), (128, 65)])
    c = Case(130, 70, len(kinds), seed=550, kinds=kinds)
    c.call()
    _check_slips(c, kinds)


def test_in_place_members_that_cannot_hide_a_slip():
    kinds = _slips(130, 130, [(63, 64), (64, 63), (129, 0), (0, 129), (129, 129), (128, 5), (70, 128)])
    c = Case(130, 130, len(kinds), seed=560, inplace=True, kinds=kinds)
    c.call()
    _check_slips(c, kinds)


PATH1 = [(65, 64), (64, 65), (128, 128), (129, 70), (70, 129), (200, 130), (256, 256), (100, 1), (1, 200), (1024, 1024), (1024, 1), (1, 1024)]


@pytest.mark.parametrize("nrows,ncols", PATH1)
def test_block_path_matches_numpy(monkeypatch, nrows, ncols):
    assert m4ri_amd.plan_transpose_batch(nrows, ncols) != 0
    monkeypatch.setenv(OVERRIDE, "1024")  # the clamp's maximum: path 1 whatever T1 is
    c = Case(nrows, ncols, 3, seed=700 + nrows + 2 * ncols)
    c.call()
    c.check()


@pytest.mark.parametrize("batch", [1, 6])
def test_block_path_batches(monkeypatch, batch):
    monkeypatch.setenv(OVERRIDE, "1024")
    c = Case(129, 70, batch, seed=800 + batch)
    c.call()
    c.check()


@pytest.mark.parametrize("nrows,ncols,override", [(65, 64, "64"), (1100, 300, "64"), (1025, 64, None)])
def test_tile_path_matches_numpy_and_transpose_dev(monkeypatch, nrows, ncols, override):
    """Path 2: the valid bits against NumPy, the tail bits of D's last words zero, padding and gaps unchanged, and the same valid bits
    as m4ri_amd_transpose_dev member by member on a clone of the same buffers."""
    if override is None:
        monkeypatch.delenv(OVERRIDE, raising=False)
        assert m4ri_amd.plan_transpose_batch(nrows, ncols) == 2
    else:
        monkeypatch.setenv(OVERRIDE, override)
    c = Case(nrows, ncols, 3, seed=900 + nrows)
    tR = c.tD.clone()
    for b in range(c.batch):
        assert m4ri_amd.lib().m4ri_amd_transpose_dev(tR.data_ptr() + 8 * b * c.dbs, c.sd, c.tA.data_ptr() + 8 * b * c.abs, c.sa, nrows, ncols, None) == 0
    c.call()
    got = c.check(whole=False)
    ref = _host(tR)
    assert np.array_equal(got[c.idx] & c.valid, ref[c.idx] & c.valid)


@pytest.mark.parametrize("n", [64, 37, 65, 130, 256, 1024])
def test_in_place_and_back(n):
    """D == A: the whole image, then a second call restores the original word for word (the transpose is an involution)."""
    c = Case(n, n, 3, seed=1000 + n, inplace=True)
    assert c.tD.data_ptr() == c.tA.data_ptr()
    c.call()
    c.check()
    c.call()
    torch.cuda.synchronize()
    assert np.array_equal(_host(c.tD), c.hD)


def test_in_place_ignores_the_override(monkeypatch):
    monkeypatch.setenv(OVERRIDE, "64")  # an out-of-place 130 x 130 would go to the tile kernel, which may not run in place
    c = Case(130, 130, 3, seed=1050, inplace=True)
    c.call()
    c.check()


def test_override_is_clamped_and_read_per_call(monkeypatch):
    """(65, 64) is path 1 for every override the clamp leaves above 64 and is forwarded at 64; D's last words (one valid bit, 63 tail
    bits of dirt) tell the path: kept on path 1, zero on path 2."""
    for value, block in [("100000", True), ("128", True), ("127", False), ("64", False), ("0", False)]:
        monkeypatch.setenv(OVERRIDE, value)
        c = Case(65, 64, 2, seed=1100)
        assert (c.hD[c.idx] & ~c.valid).any()
        c.call()
        c.check(whole=block)


def test_on_a_side_stream(monkeypatch):
    monkeypatch.setenv(OVERRIDE, "1024")
    s = torch.cuda.Stream()
    for (nrows, ncols) in [(64, 33), (129, 70)]:
        c = Case(nrows, ncols, 5, seed=1200 + nrows)
        c.call(stream=s.cuda_stream)
        s.synchronize()
        c.check()


def test_captured_into_a_graph(monkeypatch):
    """Both register paths are plain launches: captured (nothing runs, D keeps its dirt), then replayed once.  One branch, default queues."""
    monkeypatch.setenv(OVERRIDE, "1024")
    c0, c1 = Case(33, 17, 5, seed=1300), Case(129, 70, 3, seed=1310)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        st = torch.cuda.current_stream().cuda_stream
        c0.call(stream=st)
        c1.call(stream=st)
    torch.cuda.synchronize()
    assert np.array_equal(_host(c0.tD), c0.hD) and np.array_equal(_host(c1.tD), c1.hD)
    g.replay()
    c0.check()
    c1.check()
