"""m4ri_amd_row_sums_weights_batch_dev (include/m4ri_amd.h, rowsums_batch.hip): the weight distribution and the lightest of the
C(k, t) sums of exactly t rows of every member, against NumPy's brute force on the unpacked bits and closed forms
(tests/rowsums_cases.py), on every path the member can be routed to.  The operands are dirty in their tail bits, padding words and gaps
(the layouts of tests/test_gpu_reduce_batch.py) and must come back unchanged word for word; every output is a window inside a larger
dirty device array whose frame must come back unchanged.

Where the kernel changes its ways (rowsums_batch.hip; a lane owns an upper part {i_1 .. i_{t-1}}, 64 consecutive ones per wave, and
the wave walks i_0 over a staged segment of rows):
  t = 0, k < t, n = 0   the initialisation kernel alone
  t = 1                 a lane per row, no walk; k = 64, 65: one and two chunks of lanes
  t = 2                 the upper part is i_1 itself: k = 64 fills a wave, 65 and 66 start a second, 129 a third
  t >= 3                one bisection per further element; 64 upper parts are reached at k = 12 (t = 3), crossed at k = 65 .. 67
  segments              path 0: 1024 / WT rows, WT = the register words of a row: 64 rows from n = 513 on, 128 from 257, ... so k = 66,
                        130 at n = 1024 and k = 130 at n = 512 walk two and three segments; path 1: four times as many rows, shared by
                        the four waves of a workgroup, so k = 258 at n = 1024 and k = 514 at n = 512 walk two; k = 1024, n = 1024
                        walks sixteen and four
  path 0 / path 1       a wave per member with plain stores / a wave per (64 upper parts, segment) with atomics after an initialisation"""
from math import comb

import numpy as np
import pytest
import torch

import m4ri_amd
import rowspace_cases as rw
import rowsums_cases as rc
from m4ri_amd.mzd import Mzd
from test_gpu_reduce_batch import Operand, Out

pytestmark = pytest.mark.gpu
PATH0 = "M4RI_AMD_ROW_SUMS_PATH0_MAX"
M0_MAX = 1 << 24  # the largest number of sums per member the override sends to path 0


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    assert m4ri_amd.lib().m4ri_amd_device_count() >= 1, "no HIP device visible: the gpu tests have nothing to run on"
    m4ri_amd.init(0)
    torch.cuda.set_device(0)


def _route(monkeypatch, path):
    """Send the next calls to `path` whatever the measured bound is (None: the library's own routing)."""
    if path is None:
        monkeypatch.delenv(PATH0, raising=False)
    else:
        monkeypatch.setenv(PATH0, {0: str(M0_MAX), 1: "-1"}[path])


def _paths(k, n, t):
    """The paths members of this shape can be sent to: members without columns or sums are always answered on path 0."""
    if n == 0 or t == 0 or k < t:
        return [0]
    return ([0] if comb(k, t) <= M0_MAX else []) + [1]


def _bits(rows, cols, seed):
    return Mzd.random(rows, cols, seed).to_bits()


class Case:
    """One batch on the device: G (a list of k x n bit matrices; one of them = shared) and V (a list of n-bit vectors, one = shared,
    None = absent), the weights and ranks of all sums computed once."""

    def __init__(self, k, n, t, G, V=None, layout="gaps", seed=0, tail_ones=()):
        self.k, self.n, self.t, self.seed = k, n, t, seed
        self.batch = max(len(G), len(V) if V is not None else 1)
        self.G = Operand(G, k, n, layout, seed + 1, tail_ones if len(G) > 1 else ()) if k and n else None
        self.V = Operand([v[None, :] for v in V], 1, n, layout, seed + 2, tail_ones if len(V) > 1 else ()) if V is not None and n else None
        pick = lambda M, b: M[b if len(M) > 1 else 0]
        self.weights = [rc.weights(pick(G, b), pick(V, b) if V is not None else None, t) if k >= t else (np.zeros(0, dtype=np.int64),) * 2
                        for b in range(self.batch)]
        self.want_hist = np.concatenate([rc.hist_of(w, n) for w, _ in self.weights])
        assert all(int(rc.hist_of(w, n).sum()) == comb(k, t) for w, _ in self.weights)

    def call(self, w_min, hist=True, lightest=True, stream=0, outs=None):
        """Launch with fresh dirty output windows (or the given ones); returns them for check()."""
        if outs is None:
            outs = (Out(np.int64, self.batch * (self.n + 1), self.seed + 10), Out(np.int64, self.batch, self.seed + 11))
        g = (self.G.ptr, self.G.stride, self.G.bs) if self.G else (0, 0, 0)
        v = (self.V.ptr, self.V.bs) if self.V else (0, 0)
        m4ri_amd.row_sums_weights_batch_dev(*g, self.k, self.n, *v, self.batch, self.t, w_min, outs[0].ptr if hist else 0,
                                            outs[1].ptr if lightest else 0, stream=stream)
        return outs

    def want_light(self, w_min):
        return [rc.lightest_of(w, r, w_min) for w, r in self.weights]

    def check(self, outs, w_min, hist=True, lightest=True, ran=True):
        torch.cuda.synchronize()
        if hist and ran:
            outs[0].check(self.want_hist, "hist")
        else:
            assert outs[0].untouched(), "hist"
        if lightest and ran:
            outs[1].check(self.want_light(w_min), f"lightest at w_min = {w_min}")
        else:
            assert outs[1].untouched(), "lightest"
        assert self.G is None or self.G.unchanged(), "G was written"
        assert self.V is None or self.V.unchanged(), "V was written"

    def run(self, monkeypatch, w_mins=(1,), forms=((True, True),)):
        """Every path the shape can go to, every w_min, every (hist, lightest) form."""
        for path in _paths(self.k, self.n, self.t):
            _route(monkeypatch, path)
            for w_min in w_mins:
                for hist, lightest in forms:
                    self.check(self.call(w_min, hist, lightest), w_min, hist, lightest)


def _members(k, n, batch, seed):
    """Random generators; member 1 is sparse (light sums, many ties), member 2 has a duplicate and a zero row."""
    G = [_bits(k, n, seed + b) for b in range(batch)]
    rng = np.random.default_rng(seed)
    if batch > 1 and k and n:
        G[1] = G[1] & (rng.random((k, n)) < 0.1).astype(np.uint8)
    if batch > 2 and k > 2:
        G[2][k - 1] = G[2][0]
        G[2][k // 2] = 0
    return G


def _words(n, count, seed):
    return [_bits(1, n, seed + 100 + b)[0] for b in range(count)]


@pytest.mark.parametrize("k,t", [(10, t) for t in range(9)] + [(7, 8), (5, 5), (8, 8), (1, 1), (0, 0), (0, 1)])
def test_t_sweep(monkeypatch, k, t):
    """n = 65 (two words, one valid bit in the second), batch 3, per-member V, on both paths; no sums at all; k = t: one sum."""
    n = 65
    c = Case(k, n, t, _members(k, n, 3, 10 * k + t), _words(n, 3, k + t), layout="gaps" if t % 2 else "even", seed=k + t)
    c.run(monkeypatch, w_mins=(0, 1))


@pytest.mark.parametrize("k,t", [(k, 1) for k in (64, 65)] + [(k, 2) for k in (2, 63, 64, 65, 66, 129)] + [(k, 3) for k in (3, 65, 66, 67, 130)]
                         + [(68, 4)])
def test_lane_and_wave_boundaries(monkeypatch, k, t):
    """The upper parts fill one wave, spill into the next, and cross a 64-lane chunk in the middle of an i_2."""
    n = 70 if t < 4 else 40
    batch = 2 if comb(k, t) < 100000 else 1
    c = Case(k, n, t, _members(k, n, batch, 3 * k + t), _words(n, batch, k), seed=k)
    c.run(monkeypatch, w_mins=(1,))


@pytest.mark.parametrize("k,n,t", [(65, 1024, 2), (66, 1024, 2), (130, 1024, 2), (130, 512, 2), (70, 513, 3), (258, 200, 2),
                                   (258, 1024, 2), (514, 512, 2)])
def test_segment_boundaries(monkeypatch, k, n, t):
    """The walk leaves the first staged segment of rows: 64 rows at 16 register words, 128 at 8, 256 at 4 on path 0, four times as many
    on path 1."""
    c = Case(k, n, t, _members(k, n, 2, k + n), _words(n, 2, k), seed=n + t)
    c.run(monkeypatch, w_mins=(0, n // 2))


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 128, 129, 256, 257, 512, 513, 1023, 1024])
def test_n_sweep(monkeypatch, n):
    """k = 12, t = 3: every register width (1, 2, 4, 8, 16 words), full and partly filled last words, and members without columns."""
    k, t = 12, 3
    c = Case(k, n, t, _members(k, n, 3, 7 * n), _words(n, 3, n), layout="odd" if n % 2 else "dense", seed=n)
    c.run(monkeypatch, w_mins=(0, 1), forms=((True, True), (False, True)))


@pytest.mark.parametrize("batch", [1, 3, 4, 5, 257])
def test_batch_sweep(monkeypatch, batch):
    """Several members share a workgroup; 5 and 257 leave the last workgroup partly filled."""
    k, n, t = 9, 70, 2
    c = Case(k, n, t, _members(k, n, batch, 31 + batch), _words(n, batch, batch), seed=batch)
    c.run(monkeypatch)


@pytest.mark.parametrize("layout", ["dense", "even", "odd", "gaps"])
def test_layouts(monkeypatch, layout):
    for k, n, t in [(10, 64, 2), (6, 130, 3), (13, 200, 4)]:
        c = Case(k, n, t, _members(k, n, 5, k + n), _words(n, 5, k), layout=layout, seed=k)
        if layout == "dense":
            assert (c.G.stride, c.G.bs) == ((n + 63) // 64, k * ((n + 63) // 64))
        if layout == "odd":
            assert c.G.ptr % 16 == 8 and c.G.stride % 2 == 1 and c.G.bs % 2 == 1
        c.run(monkeypatch)


@pytest.mark.parametrize("v_form", ["absent", "shared", "per-member", "shared-G"])
def test_operand_combinations(monkeypatch, v_form):
    """V absent, shared, per member; one shared G with per-member V (information-set decoding of many received words); every w_min that
    matters; each output alone (the other stays untouched) and both."""
    k, n, t, batch = 11, 100, 3, 4
    G = _members(k, n, 1 if v_form == "shared-G" else batch, 5)
    V = {"absent": None, "shared": _words(n, 1, 1), "per-member": _words(n, batch, 2), "shared-G": _words(n, batch, 3)}[v_form]
    c = Case(k, n, t, G, V, seed=len(v_form))
    assert c.batch == batch and (c.G.bs == 0) == (v_form == "shared-G") and (V is None or (c.V.bs == 0) == (v_form == "shared"))
    mid = int(np.median(c.weights[0][0]))
    c.run(monkeypatch, w_mins=(0, 1, mid, n, n + 1), forms=((True, True), (True, False), (False, True)))
    assert c.want_light(n + 1) == [-1] * batch


def test_members_that_cannot_hide_a_slip(monkeypatch):
    """Duplicate rows, zero rows, all zero, V equal to a sum, every bit beyond column n set."""
    k, n = 8, 90
    r = _bits(k, n, 3)
    dup = r.copy()
    dup[1::2] = dup[0::2]                       # four rows, each twice: the sum of a pair is zero
    zrows = r.copy()
    zrows[[0, 3, 7]] = 0
    zero = np.zeros((k, n), dtype=np.uint8)
    for t in (1, 2, 3):
        c = Case(k, n, t, [dup, zrows, zero], seed=t)
        assert c.want_hist[2 * (n + 1)] == comb(k, t) and c.want_light(1)[2] == -1 and c.want_light(0)[2] == 0
        if t == 1:   # the zero row 0 is the lightest from w_min = 0 and out of the race from w_min = 1
            assert c.want_light(0)[1] == 0 and c.want_light(1)[1] >> 40 >= 1
        if t == 2:   # rows 0 and 1 are equal: rank C(0, 1) + C(1, 2) = 0 weighs nothing
            assert c.want_light(0)[0] == 0 and c.want_hist[0] == 4
        c.run(monkeypatch, w_mins=(0, 1))
    in_span = [dup[0] ^ dup[4] ^ dup[6], zrows[1] ^ zrows[2] ^ zrows[6], np.zeros(n, dtype=np.uint8)]
    c = Case(k, n, 3, [dup, zrows, zero], in_span, seed=5)
    assert c.want_light(0) == [rc.rank([0, 4, 6]), rc.rank([1, 2, 6]), 0]
    c.run(monkeypatch, w_mins=(0, 1))
    # every bit beyond column n set in G and V of members 1 and 2 (n = 90 leaves 38 of them per row): they must not count
    c = Case(k, n, 2, [zero, zero, r], [np.zeros(n, dtype=np.uint8)] * 2 + [r[5]], seed=6, tail_ones=(1, 2))
    assert c.want_hist[0] == c.want_hist[n + 1] == comb(k, 2)
    c.run(monkeypatch, w_mins=(0, 1))


def _closed(G, k, n, t, want_hist, lights, what, hist=True):
    """One member given by closed form, on the path the caller has routed to: lights = [(w_min, lightest)], () = hist only."""
    op = Operand([G], k, n, "gaps", k + t)
    for w_min, want_light in lights or [(0, None)]:
        h, light = Out(np.int64, n + 1, 5), Out(np.int64, 1, 6)
        m4ri_amd.row_sums_weights_batch_dev(op.ptr, op.stride, 0, k, n, 0, 0, 1, t, w_min, h.ptr if hist else 0, light.ptr if want_light is not None else 0)
        torch.cuda.synchronize()
        if hist:
            h.check(want_hist, f"hist ({what})")
        else:
            assert h.untouched()
        if want_light is not None:
            light.check([want_light], f"lightest at w_min = {w_min} ({what})")
        else:
            assert light.untouched()
    assert op.unchanged()


def test_rank_at_a_distance_t3(monkeypatch):
    """R(512, 77, 300, 511), n = 1024, t = 3: 2.2 * 10^7 sums, beyond what the override sends to path 0; the one lightest set has its
    largest row last and a rank of 2.2 * 10^7."""
    k, (a, b, c), t = 512, (77, 300, 511), 3
    assert _paths(k, 2 * k, t) == [1]
    want = rc.rigged_hist(k, t)
    assert (want[3], want[5], want[6], want[7]) == (1, 2 * (k - 3), comb(k - 1, 3), comb(k - 3, 2)) and int(want.sum()) == comb(k, t)
    light = (3 << 40) | rc.rank([a, b, c])
    assert light == rc.rigged_lightest(k, a, b, c, t)
    # w_min = 4: the five-weights are {c, a or b, x}: the smallest rank takes a and x = 0;  w_min = 8: nothing weighs more than 7
    _closed(rc.rigged(k, a, b, c), k, 2 * k, t, want, [(1, light), (4, (5 << 40) | rc.rank([0, a, c])), (8, -1)], "path 1")


@pytest.mark.parametrize("path", [0, 1])
def test_rank_at_a_distance_t4(monkeypatch, path):
    """R(96, 5, 40, 95), t = 4: 3.3 * 10^6 sums by the closed form, which tests/test_row_sums_weights_plan.py holds to brute force."""
    k, (a, b, c), t = 96, (5, 40, 95), 4
    _route(monkeypatch, path)
    want = rc.rigged_hist(k, t)
    assert int(want.sum()) == comb(k, t) and want[5] == k - 3
    _closed(rc.rigged(k, a, b, c), k, 2 * k, t, want, [(1, rc.rigged_lightest(k, a, b, c, t)), (0, rc.rigged_lightest(k, a, b, c, t))], f"path {path}")
    _closed(rc.rigged(k, a, b, c), k, 2 * k, t, want, [(1, rc.rigged_lightest(k, a, b, c, t))], f"path {path}, lightest alone", hist=False)


def test_a_bin_above_two_to_the_31(monkeypatch):
    """The doubled identity at k = 512, t = 4, hist only: 2.8 * 10^9 sums in ONE bin: the counters are 64-bit."""
    k, t = 512, 4
    want, _ = rc.doubled_identity_expect(k, t, 0)
    assert want[8] == comb(k, t) > 1 << 31
    _closed(rc.doubled_identity(k), k, 2 * k, t, want, (), "path 1")


def test_the_lds_corner(monkeypatch):
    """k = 1024, n = 1024, t = 2, random: 5 * 10^5 sums by brute force, sixteen segments of rows, on both paths."""
    k = n = 1024
    c = Case(k, n, 2, [_bits(k, n, 77)], [_bits(1, n, 78)[0]], seed=9)
    c.run(monkeypatch, w_mins=(1, n // 2))


def test_the_t_sums_make_up_the_row_space_on_the_device(monkeypatch):
    k, n, batch = 8, 100, 3
    G, V = _members(k, n, batch, 12), _words(n, batch, 13)
    g, v = Operand(G, k, n, "gaps", 1), Operand([x[None, :] for x in V], 1, n, "gaps", 2)
    whole = Out(np.int64, batch * (n + 1), 3)
    m4ri_amd.rowspace_weights_batch_dev(g.ptr, g.stride, g.bs, k, n, v.ptr, v.bs, batch, 0, whole.ptr, 0)
    for path in (0, 1):
        _route(monkeypatch, path)
        parts = [Out(np.int64, batch * (n + 1), 4 + t) for t in range(k + 1)]
        for t, o in enumerate(parts):
            m4ri_amd.row_sums_weights_batch_dev(g.ptr, g.stride, g.bs, k, n, v.ptr, v.bs, batch, t, 0, o.ptr, 0)
        torch.cuda.synchronize()
        total = sum(o.dev.cpu().numpy()[3:-3] for o in parts)
        whole.check(total, f"the sum over t of hist, path {path}")
        assert int(total.sum()) == batch << k


def test_t_1_agrees_with_weight_batch(monkeypatch):
    """t = 1, w_min = 0, no V: the lightest row and its index, as weight_batch_dev gives them with a 32-bit shift."""
    k, n, batch = 70, 130, 5
    G = _members(k, n, batch, 21)
    g = Operand(G, k, n, "gaps", 1)
    rows = torch.full((batch,), -7, dtype=torch.int64, device="cuda")
    m4ri_amd.weight_batch_dev(g.ptr, g.stride, g.bs, 0, 0, 0, k, n, batch, lightest=rows.data_ptr())
    for path in (0, 1):
        _route(monkeypatch, path)
        sums = torch.full((batch,), -7, dtype=torch.int64, device="cuda")
        m4ri_amd.row_sums_weights_batch_dev(g.ptr, g.stride, g.bs, k, n, 0, 0, batch, 1, 0, 0, sums.data_ptr())
        torch.cuda.synchronize()
        a, b = rows.cpu().numpy(), sums.cpu().numpy()
        assert np.array_equal(a >> 32, b >> 40) and np.array_equal(a & 0xFFFFFFFF, b & ((1 << 40) - 1)), path
    assert g.unchanged()


def test_on_a_side_stream_and_captured_into_a_graph(monkeypatch):
    """A capture of one call on path 0, one on path 1 (its initialisation kernel included) and one answered by the initialisation
    kernel alone: nothing runs while capturing (the outputs keep their dirt), then two replays, each on freshly dirtied outputs.  One
    stream, no parallel branches."""
    cases = []
    for path, (k, n, t) in ((0, (10, 100, 3)), (1, (40, 100, 3)), (0, (10, 100, 0))):
        c = Case(k, n, t, _members(k, n, 3, 40 + k), _words(n, 3, path), seed=50 + k + t)
        cases.append((path, c))
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    for i, (path, c) in enumerate(cases):  # a side stream first: the calls are plain launches on the stream they are given
        _route(monkeypatch, path)
        outs = (Out(np.int64, c.batch * (c.n + 1), 80 + i), Out(np.int64, c.batch, 90 + i))
        torch.cuda.synchronize()  # the windows are uploaded on the default stream
        c.call(1, stream=side.cuda_stream, outs=outs)
        side.synchronize()
        c.check(outs, 1)
    held = [(Out(np.int64, c.batch * (c.n + 1), 60 + i), Out(np.int64, c.batch, 70 + i)) for i, (path, c) in enumerate(cases)]
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for (path, c), outs in zip(cases, held):
            _route(monkeypatch, path)  # read per call, on the host
            c.call(1, stream=torch.cuda.current_stream().cuda_stream, outs=outs)
    for (path, c), outs in zip(cases, held):
        c.check(outs, 1, ran=False)
    for replay in range(2):
        for outs in held:
            for o in outs:
                o.dev.copy_(torch.from_numpy(o.host))  # dirty again
        torch.cuda.synchronize()
        g.replay()
        for (path, c), outs in zip(cases, held):
            c.check(outs, 1)
