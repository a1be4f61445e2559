"""m4ri_amd_weight_batch_dev, m4ri_amd_mismatch_batch_dev and m4ri_amd_row_span_batch_dev (include/m4ri_amd.h, reduce_batch.hip): the
weights, first differing rows and non-zero row spans of `batch` matrices in one call each, every member against NumPy on the unpacked
bits (tests/reduce_cases.py), on all three paths of m4ri_amd_plan_reduce_batch.  The operands are dirty in their tail bits, padding
words and gaps (tests/test_gpu_echelonize_batch._pack) and must come back unchanged word for word; every output is a window inside a
larger dirty device array whose frame must come back unchanged."""
import numpy as np
import pytest
import torch

import m4ri_amd
import reduce_cases as rc
from m4ri_amd.mzd import Mzd
from test_gpu_echelonize_batch import _pack

pytestmark = pytest.mark.gpu
PATH0, PATH1 = "M4RI_AMD_REDUCE_BATCH_PATH0_MAX", "M4RI_AMD_REDUCE_BATCH_PATH1_MAX"
NROWS = (1, 2, 63, 64, 65, 129, 257)
NCOLS = (1, 63, 64, 65, 127, 128, 129, 200)
FRAME = 3  # dirty entries before and after an output window


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    assert m4ri_amd.lib().m4ri_amd_device_count() >= 1, "no HIP device visible: the gpu tests have nothing to run on"
    m4ri_amd.init(0)
    torch.cuda.set_device(0)


def _route(monkeypatch, path):
    """Send the next calls to `path` whatever the measured bounds are (None: the library's own routing)."""
    for name, value in zip((PATH0, PATH1), {None: (None, None), 0: ("16", None), 1: ("0", str(1 << 30)), 2: ("0", "0")}[path]):
        if value is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, value)


def _paths(nrows, ncols):
    """The paths members of this shape can be sent to."""
    return ([0] if nrows <= 64 and ncols <= 1024 else []) + [1, 2]


def _w(n):
    return (n + 63) // 64


def _layout(kind, nrows, w):
    """(stride, batch stride, words before the operand's base): "gaps" odd frames around rows and members; "even" the same with even
    strides (16-byte loads); "dense" unit stride, members back to back; "odd" base, stride and batch stride all odd numbers of words."""
    if kind == "dense":
        return w, nrows * w, 0
    if kind == "even":
        s = w + 2 - w % 2
        return s, nrows * s + 4, 0
    if kind == "odd":
        s = w + 1 + w % 2
        return s, nrows * s + 1 + (nrows * s) % 2, 1
    return w + 1, nrows * (w + 1) + 3, 0


class Operand:
    """`members` (bit matrices; one of them = a shared operand, batch stride 0) on the device, dirty outside the valid bits."""

    def __init__(self, members, nrows, ncols, layout, seed, tail_ones=()):
        self.stride, bs, off = _layout(layout, nrows, _w(ncols))
        self.bs = bs if len(members) > 1 else 0
        h, idx, valid = _pack([Mzd.from_bits(m) for m in members], nrows, ncols, self.stride, bs, seed)
        for b in tail_ones:  # every bit beyond the last column of member b set
            h[idx[b][:, -1]] |= ~valid[-1]
        self.host = np.concatenate([np.full(off, 0x5A5A5A5A5A5A5A5A, dtype=np.uint64), h])
        self.dev = torch.from_numpy(self.host.view(np.int64).copy()).cuda()
        self.ptr = self.dev.data_ptr() + 8 * off

    def unchanged(self):
        return np.array_equal(self.dev.cpu().numpy().view(np.uint64), self.host)


class Out:
    """A window of n entries inside a dirty device array."""

    def __init__(self, dtype, n, seed):
        rng = np.random.default_rng(seed)
        self.n = n
        self.host = rng.integers(-(1 << 30), 1 << 30, size=n + 2 * FRAME).astype(dtype)
        self.dev = torch.from_numpy(self.host.copy()).cuda()
        self.ptr = self.dev.data_ptr() + FRAME * self.host.itemsize

    def check(self, want, what):
        got = self.dev.cpu().numpy()
        assert np.array_equal(got[:FRAME], self.host[:FRAME]) and np.array_equal(got[FRAME + self.n:], self.host[FRAME + self.n:]), f"{what}: frame written"
        win = got[FRAME:FRAME + self.n]
        bad = np.flatnonzero(win != np.asarray(want, dtype=self.host.dtype))
        assert bad.size == 0, f"{what}: {bad.size} entries differ, first at {bad[:5]}: got {win[bad[:5]]}, want {np.asarray(want)[bad[:5]]}"

    def untouched(self):
        return np.array_equal(self.dev.cpu().numpy(), self.host)


class Call:
    """One call with its output windows: made ready first, launched (perhaps under capture), checked once the stream is idle."""

    def __init__(self, fn, outs, want, skip=()):
        self.fn, self.outs, self.want, self.skip = fn, outs, want, skip

    def launch(self, stream=0):
        self.fn(stream, **{k: (0 if k in self.skip else o.ptr) for k, o in self.outs.items()})

    def check(self, ran=True):
        for k, o in self.outs.items():
            if k in self.skip or not ran:
                assert o.untouched(), k
            else:
                o.check(self.want[k], k)


class Case:
    """One batch: A (and B) on the device, the expectations computed once."""

    def __init__(self, nrows, ncols, A, B=None, layout="gaps", seed=0, tail_ones=(), same=False):
        self.nrows, self.ncols, self.seed = nrows, ncols, seed
        self.batch = max(len(A), len(B) if B is not None else 1)
        self.A = Operand(A, nrows, ncols, layout, seed + 1, tail_ones)
        self.B = self.A if same else Operand(B, nrows, ncols, layout, seed + 2) if B is not None else None
        pick = lambda M, b: M[b if len(M) > 1 else 0]
        other = A if same else B
        self.a = [pick(A, b) for b in range(self.batch)]
        self.x = [pick(A, b) ^ pick(other, b) for b in range(self.batch)] if other is not None else self.a  # A ^ B

    def _aargs(self):
        return (self.A.ptr, self.A.stride, self.A.bs)

    def _bargs(self):
        return (self.B.ptr, self.B.stride, self.B.bs)

    def weight(self, distance=True, skip=()):
        """weight_batch_dev (of A ^ B if there is a B and distance is set) with every output but those in `skip`."""
        use_b = distance and self.B is not None
        bits = self.x if use_b else self.a
        outs = dict(total=Out(np.int64, self.batch, self.seed + 10), row_weight=Out(np.int32, self.batch * self.nrows, self.seed + 11),
                    lightest=Out(np.int64, self.batch, self.seed + 12))
        want = dict(total=[rc.total(x) for x in bits], row_weight=np.concatenate([rc.row_weights(x) for x in bits]),
                    lightest=[rc.lightest(x) for x in bits])
        fn = lambda stream, **o: m4ri_amd.weight_batch_dev(*self._aargs(), *(self._bargs() if use_b else (0, 0, 0)), self.nrows, self.ncols, self.batch,
                                                           stream=stream, **o)
        return Call(fn, outs, want, skip)

    def mismatch(self):
        want = dict(first_row=[rc.first_mismatch(a, a ^ x) for a, x in zip(self.a, self.x)])
        fn = lambda stream, **o: m4ri_amd.mismatch_batch_dev(*self._aargs(), *self._bargs(), self.nrows, self.ncols, self.batch, stream=stream, **o)
        return Call(fn, dict(first_row=Out(np.int32, self.batch, self.seed + 13)), want)

    def span(self, skip=()):
        outs = dict(first_nonzero=Out(np.int32, self.batch, self.seed + 14), end_nonzero=Out(np.int32, self.batch, self.seed + 15))
        want = dict(first_nonzero=[rc.first_nonzero(x) for x in self.a], end_nonzero=[rc.end_nonzero(x) for x in self.a])
        fn = lambda stream, **o: m4ri_amd.row_span_batch_dev(*self._aargs(), self.nrows, self.ncols, self.batch, stream=stream, **o)
        return Call(fn, outs, want, skip)

    def all_calls(self):
        """Every entry point the case has operands for."""
        return [self.weight(), self.span()] + ([self.weight(distance=False), self.mismatch()] if self.B is not None else [])

    def run(self, calls=None, stream=0):
        calls = self.all_calls() if calls is None else calls
        for c in calls:
            c.launch(stream)
        self.verify(calls)

    def verify(self, calls, ran=True):
        torch.cuda.synchronize()
        for c in calls:
            c.check(ran)
        assert self.A.unchanged(), "A was written"
        assert self.B is None or self.B.unchanged(), "B was written"


def _random(nrows, ncols, seed):
    return Mzd.random(nrows, ncols, seed).to_bits()


def _members(nrows, ncols, batch, seed):
    """A and B of a sweep: random members, every fourth pair equal, every fourth (offset 1) differing in one bit, and one sparse A."""
    A = [_random(nrows, ncols, seed + 2 * b) for b in range(batch)]
    B = [_random(nrows, ncols, seed + 2 * b + 1) for b in range(batch)]
    rng = np.random.default_rng(seed)
    for b in range(batch):
        if b % 4 == 2:
            B[b] = A[b].copy()
        if b % 4 == 3:
            B[b] = A[b] ^ rc.single(nrows, ncols, int(rng.integers(nrows)), int(rng.integers(ncols)))
    if batch > 1:
        A[1] = A[1] & (rng.random((nrows, ncols)) < 0.02).astype(np.uint8)
        if batch > 2:
            A[2] = B[2] = A[2] & (rng.random((nrows, ncols)) < 0.02).astype(np.uint8)
    return A, B


@pytest.mark.parametrize("nrows,path", [(n, p) for n in NROWS for p in _paths(n, max(NCOLS))])
def test_shapes_match_numpy(monkeypatch, nrows, path):
    """Every column count at this row count, in a layout with 8-byte and one with 16-byte loads; batch 5."""
    _route(monkeypatch, path)
    for ncols in NCOLS:
        for layout in ("gaps", "even"):
            A, B = _members(nrows, ncols, 5, seed=1000 * nrows + ncols)
            c = Case(nrows, ncols, A, B, layout=layout, seed=nrows + ncols)
            c.run()


@pytest.mark.parametrize("batch", [1, 257])
@pytest.mark.parametrize("path", [0, 1, 2])
def test_batches_match_numpy(monkeypatch, batch, path):
    """257 members are no multiple of the four of a path-0 workgroup, and one member fills a quarter of one."""
    _route(monkeypatch, path)
    for nrows, ncols in [(1, 63), (64, 65), (63, 200), (65, 63), (257, 129)]:
        if path in _paths(nrows, ncols):
            A, B = _members(nrows, ncols, batch, seed=77 * nrows + ncols + batch)
            c = Case(nrows, ncols, A, B, layout="even" if ncols == 65 else "gaps", seed=batch + nrows)
            c.run()


def test_path_two_at_its_natural_size(monkeypatch):
    """5000 x 3000, two members: path 2 by the plan, several chunks of rows per member, with answers in the first, a middle and the last
    chunk: whatever chunks the calls for row positions leave unread, the results are NumPy's."""
    _route(monkeypatch, None)
    nrows, ncols = 5000, 3000
    assert m4ri_amd.plan_reduce_batch(nrows, ncols) == 2
    A = [_random(nrows, ncols, 1), rc.single(nrows, ncols, 4321, 2999)]
    B = [A[0] ^ rc.single(nrows, ncols, 4999, 2999) ^ rc.single(nrows, ncols, 3333, 0), _random(nrows, ncols, 2)]
    c = Case(nrows, ncols, A, B, layout="even", seed=5)
    c.run()
    assert rc.first_mismatch(A[0], B[0]) == 3333 and rc.first_nonzero(A[1]) == 4321 and rc.end_nonzero(A[1]) == 4322


@pytest.mark.parametrize("path", [0, 1, 2])
@pytest.mark.parametrize("layout", ["dense", "odd"])
def test_dense_and_unaligned_layouts(monkeypatch, path, layout):
    """dense: unit stride (64 x 64) or the width (130 columns), members back to back.  odd: the base an odd number of words, odd strides
    and batch strides: nothing is 16-byte aligned."""
    _route(monkeypatch, path)
    for nrows, ncols in [(64, 64), (64, 130), (130, 128), (100, 200)]:
        if path in _paths(nrows, ncols):
            A, B = _members(nrows, ncols, 6, seed=3 * nrows + ncols)
            c = Case(nrows, ncols, A, B, layout=layout, seed=9)
            if layout == "dense":
                assert (c.A.stride, c.A.bs) == (_w(ncols), nrows * _w(ncols))
            else:
                assert c.A.ptr % 16 == 8 and c.A.stride % 2 == 1 and c.A.bs % 2 == 1
            c.run()


def _tied(nrows, ncols, seed):
    """Dense rows, and two rows of weight 1 (not the first two): the first of them is the lightest."""
    m = np.ones((nrows, ncols), dtype=np.uint8)
    m[:, seed % ncols] = 0 if ncols > 2 else 1
    lo, hi = nrows // 3, nrows - 1
    for r, c in ((lo, ncols - 1), (hi, 0)):
        m[r] = 0
        m[r, c] = 1
    return m, lo


@pytest.mark.parametrize("path", [0, 1, 2])
def test_members_that_cannot_hide_a_slip(monkeypatch, path):
    _route(monkeypatch, path)
    for nrows, ncols in [(64, 130), (63, 64), (130, 70), (257, 129)]:
        if path not in _paths(nrows, ncols):
            continue
        zero, ones = np.zeros((nrows, ncols), dtype=np.uint8), np.ones((nrows, ncols), dtype=np.uint8)
        pos = rc.corners(nrows, ncols)
        tied, lo = _tied(nrows, ncols, 5)
        last = rc.single(nrows, ncols, nrows - 1, ncols - 1)
        two = rc.single(nrows, ncols, nrows // 2, 0) ^ rc.single(nrows, ncols, nrows - 1, ncols - 1)
        r = _random(nrows, ncols, 4)
        #      0     1     2 (tail bits set)  3 ...                                  then: tied, and three random ones for the B side
        A = [zero, ones, zero] + [rc.single(nrows, ncols, *p) for p in pos] + [tied, r, r, r]
        B = [zero, ones, zero] + [zero] * len(pos) + [tied, r, r ^ last, r ^ two]
        c = Case(nrows, ncols, A, B, seed=nrows, tail_ones=(2,))
        n = len(pos)
        # what the expectations must be, spelled out (the NumPy helpers agree, or the test is wrong)
        assert [rc.total(x) for x in c.a[:3 + n]] == [0, nrows * ncols, 0] + [1] * n
        assert [rc.first_nonzero(x) for x in c.a[:3 + n]] == [nrows, 0, nrows] + [p[0] for p in pos]
        assert [rc.end_nonzero(x) for x in c.a[:3 + n]] == [0, nrows, 0] + [p[0] + 1 for p in pos]
        assert all(rc.row_weights(c.a[3 + k]).tolist() == [int(i == p[0]) for i in range(nrows)] for k, p in enumerate(pos))
        assert rc.lightest(tied) == (1 << 32) | lo and rc.lightest(ones) == ncols << 32
        assert [rc.first_mismatch(a, b) for a, b in zip(A, B)][-4:] == [-1, -1, nrows - 1, nrows // 2]
        c.run()
        # the zero member against the one whose tail bits are all set: equal
        z = Case(nrows, ncols, [zero, zero], [zero, zero], seed=nrows + 1, tail_ones=(1,))
        z.run([z.mismatch(), z.weight()])


@pytest.mark.parametrize("path", [0, 1, 2])
def test_distance_forms(monkeypatch, path):
    """One shared A against many B, many A against one shared B, and A == B (the same memory): zeros."""
    _route(monkeypatch, path)
    for nrows, ncols in [(64, 100), (100, 130)]:
        if path not in _paths(nrows, ncols):
            continue
        many = [_random(nrows, ncols, s) for s in range(5)]
        one = [many[3].copy()]
        for A, B in ((one, many), (many, one)):
            c = Case(nrows, ncols, A, B, seed=20)
            assert c.batch == 5 and (c.A.bs == 0) != (c.B.bs == 0)
            c.run([c.weight(), c.mismatch()])
        s = Case(nrows, ncols, many, seed=21, same=True)
        assert s.B is s.A and not any(x.any() for x in s.x)
        s.run([s.weight(), s.mismatch()])


@pytest.mark.parametrize("path", [0, 1, 2])
def test_each_optional_output_left_out_in_turn(monkeypatch, path):
    _route(monkeypatch, path)
    nrows, ncols = (60, 100) if path == 0 else (100, 100)
    A, B = _members(nrows, ncols, 5, seed=31)
    c = Case(nrows, ncols, A, B, seed=30)
    checks = [c.weight(skip=(k,)) for k in ("total", "row_weight", "lightest")]
    checks += [c.weight(skip=("row_weight", "lightest")), c.weight(skip=("total", "lightest")), c.weight(skip=("total", "row_weight"))]
    checks += [c.span(skip=("first_nonzero",)), c.span(skip=("end_nonzero",))]
    c.run(checks)


@pytest.mark.parametrize("nrows,ncols", [(0, 5), (5, 0), (0, 0)])
def test_empty_members_still_get_their_results(nrows, ncols):
    batch = 5
    outs = [Out(np.int64, batch, 1), Out(np.int32, batch * nrows, 2), Out(np.int64, batch, 3), Out(np.int32, batch, 4), Out(np.int32, batch, 5),
            Out(np.int32, batch, 6)]
    m4ri_amd.weight_batch_dev(0, 0, 0, 0, 0, 0, nrows, ncols, batch, outs[0].ptr, outs[1].ptr, outs[2].ptr)
    m4ri_amd.mismatch_batch_dev(0, 0, 0, 0, 0, 0, nrows, ncols, batch, outs[3].ptr)
    m4ri_amd.row_span_batch_dev(0, 0, 0, nrows, ncols, batch, outs[4].ptr, outs[5].ptr)
    torch.cuda.synchronize()
    for o, want, what in zip(outs, (0, 0, -1 if nrows == 0 else 0, -1, nrows, 0), ("total", "row_weight", "lightest", "first_row", "first_nonzero", "end_nonzero")):
        o.check([want] * o.n, what)


def test_totals_beyond_32_bits():
    """65536 x 32768, every bit set (256 MiB, filled on the device): the total is exactly 2^31, every row weighs 32768."""
    nrows, ncols = 65536, 32768
    assert m4ri_amd.plan_reduce_batch(nrows, ncols) == 2
    A = torch.full((nrows * (ncols // 64),), -1, dtype=torch.int64, device="cuda")
    total, rows, light = Out(np.int64, 1, 1), Out(np.int32, nrows, 2), Out(np.int64, 1, 3)
    first, end = Out(np.int32, 1, 4), Out(np.int32, 1, 5)
    m4ri_amd.weight_batch_dev(A.data_ptr(), ncols // 64, 0, 0, 0, 0, nrows, ncols, 1, total.ptr, rows.ptr, light.ptr)
    m4ri_amd.row_span_batch_dev(A.data_ptr(), ncols // 64, 0, nrows, ncols, 1, first.ptr, end.ptr)
    torch.cuda.synchronize()
    total.check([1 << 31], "total")
    rows.check(np.full(nrows, 32768, dtype=np.int32), "row_weight")
    light.check([32768 << 32], "lightest")
    first.check([0], "first_nonzero")
    end.check([nrows], "end_nonzero")
    assert bool((A == -1).all()), "A was written"


def _three_paths():
    """A path-0, a path-1 and a path-2 case, ready: [(path, case, calls)]."""
    out = []
    for path, (nrows, ncols) in ((0, (33, 70)), (1, (129, 70)), (2, (257, 129))):
        A, B = _members(nrows, ncols, 5, seed=40 + path)
        c = Case(nrows, ncols, A, B, seed=41 + path)
        out.append((path, c, c.all_calls()))
    torch.cuda.synchronize()
    return out


def _queue(monkeypatch, cases, stream):
    for path, _, calls in cases:
        _route(monkeypatch, path)  # read per call, on the host
        for call in calls:
            call.launch(stream)


def test_on_a_side_stream(monkeypatch):
    cases = _three_paths()
    s = torch.cuda.Stream()
    _queue(monkeypatch, cases, s.cuda_stream)
    s.synchronize()
    for _, c, calls in cases:
        c.verify(calls)


def test_captured_into_a_graph(monkeypatch):
    """Plain launches on every path, path 2's initialisation included: captured (nothing runs, the outputs keep their dirt), then
    replayed once.  One branch, default queues."""
    cases = _three_paths()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        _queue(monkeypatch, cases, torch.cuda.current_stream().cuda_stream)
    for _, c, calls in cases:
        c.verify(calls, ran=False)
    g.replay()
    for _, c, calls in cases:
        c.verify(calls)
