"""m4ri_amd_rowspace_weights_batch_dev (include/m4ri_amd.h, rowspace_batch.hip): the weight distribution and the lightest word of the
2^k words V_b ^ x * G_b of every member, against NumPy's brute force on the unpacked bits (tests/rowspace_cases.py) on every path the
member can be routed to.  The operands are dirty in their tail bits, padding words and gaps (tests/test_gpu_echelonize_batch._pack,
the layouts of tests/test_gpu_reduce_batch.py) and must come back unchanged word for word; every output is a window inside a larger
dirty device array whose frame must come back unchanged.

Where the kernel changes its ways (rowspace_batch.hip; a message is x = (hi << s) | lo, a lane per hi, 2^s Gray steps per lane):
  path 0 (a wave per member, four members per workgroup)
    k <= 6   s = 0, 2^k lanes of the wave at work; k = 7: s = 1, the whole wave; from k = 8 on the walk is unrolled by four steps
    k = 26   the largest k the override can send here (s = 20: the lane's 32-bit minimum is full); k = 27 goes to path 1 regardless
  path 1 (a member's hi spread over waves, atomics)
    k <= 11  the split of path 0, one wave; k = 12: s = 6, still one wave; k = 13: two waves; k = 15: more than the four waves of a
             workgroup, so a member spans workgroups (k = 13, 14: several members share one)
    k = 26   s grows beyond 6 (s = k - 19); k = 31: s reaches 12 and stays there
The k sweep 0 .. 18 crosses all of these below 19 on both paths; the closed forms at 24 .. 27 and 30 .. 33 cross the others."""
import numpy as np
import pytest
import torch

import m4ri_amd
import rowspace_cases as rw
from m4ri_amd.mzd import Mzd
from test_gpu_reduce_batch import Operand, Out

pytestmark = pytest.mark.gpu
PATH0 = "M4RI_AMD_ROWSPACE_PATH0_MAX"
K0_MAX = 26  # the largest k the override sends to path 0


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
        monkeypatch.setenv(PATH0, {0: str(K0_MAX), 1: "-1"}[path])


def _paths(k, n):
    """The paths members of this shape can be sent to: members without columns are always answered on path 0."""
    return [0] if n == 0 else ([0] if k <= K0_MAX else []) + [1]


def _bits(rows, cols, seed):
    return Mzd.random(rows, cols, seed).to_bits()


class Case:
    """One batch on the device: G (a list of k x n bit matrices; one of them = shared) and V (a list of n-bit vectors, one = shared,
    None = absent), the expectations computed once per w_min."""

    def __init__(self, k, n, G, V=None, layout="gaps", seed=0, tail_ones=()):
        self.k, self.n, self.seed = k, n, seed
        self.batch = max(len(G), len(V) if V is not None else 1)
        self.G = Operand(G, k, n, layout, seed + 1, tail_ones if len(G) > 1 else ()) if k and n else None
        self.V = Operand([v[None, :] for v in V], 1, n, layout, seed + 2, tail_ones if len(V) > 1 else ()) if V is not None and n else None
        pick = lambda M, b: M[b if len(M) > 1 else 0]
        self.weights = [rw.weights(pick(G, b), pick(V, b) if V is not None else None) for b in range(self.batch)]
        self.want_hist = np.concatenate([rw.hist_of(w, n) for w in self.weights])
        assert all(int(rw.hist_of(w, n).sum()) == 1 << k for w in self.weights)

    def call(self, w_min, hist=True, lightest=True, stream=0, outs=None):
        """Launch with fresh dirty output windows (or the given ones); returns them for check()."""
        if outs is None:
            outs = (Out(np.int64, self.batch * (self.n + 1), self.seed + 10), Out(np.int64, self.batch, self.seed + 11))
        g = (self.G.ptr, self.G.stride, self.G.bs) if self.G else (0, 0, 0)
        v = (self.V.ptr, self.V.bs) if self.V else (0, 0)
        m4ri_amd.rowspace_weights_batch_dev(*g, self.k, self.n, *v, self.batch, w_min, outs[0].ptr if hist else 0, outs[1].ptr if lightest else 0,
                                            stream=stream)
        return outs

    def check(self, outs, w_min, hist=True, lightest=True, ran=True):
        torch.cuda.synchronize()
        if hist and ran:
            outs[0].check(self.want_hist, "hist")
        else:
            assert outs[0].untouched(), "hist"
        if lightest and ran:
            outs[1].check([rw.lightest_of(w, w_min) for w in self.weights], f"lightest at w_min = {w_min}")
        else:
            assert outs[1].untouched(), "lightest"
        assert self.G is None or self.G.unchanged(), "G was written"
        assert self.V is None or self.V.unchanged(), "V was written"

    def run(self, monkeypatch, w_mins=(1,), forms=((True, True),)):
        """Every path the shape can go to, every w_min, every (hist, lightest) form."""
        for path in _paths(self.k, self.n):
            _route(monkeypatch, path)
            for w_min in w_mins:
                for hist, lightest in forms:
                    self.check(self.call(w_min, hist, lightest), w_min, hist, lightest)


def _members(k, n, batch, seed):
    """Random generators; member 1 is sparse (light words, many ties), member 2 has a duplicate and a zero row."""
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


@pytest.mark.parametrize("k", range(0, 19))
def test_k_sweep(monkeypatch, k):
    """n = 65 (two words, one valid bit in the second), batch 3, per-member V, on both paths."""
    n = 65
    c = Case(k, n, _members(k, n, 3, 10 * k), _words(n, 3, k), layout="gaps" if k % 2 else "even", seed=k)
    c.run(monkeypatch, w_mins=(0, 1))


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 128, 129, 200, 512, 513, 1024])
def test_n_sweep(monkeypatch, n):
    """k = 9: every register width (1, 2, 4, 8, 16 words), full and partly filled last words, and members without columns."""
    k = 9
    c = Case(k, n, _members(k, n, 3, 7 * n), _words(n, 3, n), layout="odd" if n % 2 else "dense", seed=n)
    c.run(monkeypatch, w_mins=(0, 1), forms=((True, True), (False, True)))


@pytest.mark.parametrize("k", [5, 7])
@pytest.mark.parametrize("batch", [1, 3, 67, 1000])
def test_batch_sweep(monkeypatch, k, batch):
    """Several members share a workgroup; 67 and 1000 leave the last workgroup partly filled or not."""
    n = 70
    c = Case(k, n, _members(k, n, batch, 31 * k + batch), _words(n, batch, batch), seed=batch + k)
    c.run(monkeypatch)


@pytest.mark.parametrize("layout", ["dense", "even", "odd", "gaps"])
def test_layouts(monkeypatch, layout):
    for k, n in [(10, 64), (6, 130), (13, 200)]:
        c = Case(k, n, _members(k, n, 5, k + n), _words(n, 5, k), layout=layout, seed=k)
        if layout == "dense":
            assert (c.G.stride, c.G.bs) == ((n + 63) // 64, k * ((n + 63) // 64))
        if layout == "odd":
            assert c.G.ptr % 16 == 8 and c.G.stride % 2 == 1 and c.G.bs % 2 == 1
        c.run(monkeypatch)


@pytest.mark.parametrize("v_form", ["absent", "shared", "per-member", "shared-G"])
def test_operand_combinations(monkeypatch, v_form):
    """V absent, shared, per member; one shared G with per-member V (nearest-codeword decoding); every w_min that matters; each output
    alone and both."""
    k, n, batch = 11, 100, 4
    G = _members(k, n, 1 if v_form == "shared-G" else batch, 5)
    V = {"absent": None, "shared": _words(n, 1, 1), "per-member": _words(n, batch, 2), "shared-G": _words(n, batch, 3)}[v_form]
    c = Case(k, n, G, V, seed=len(v_form))
    assert c.batch == batch and (c.G.bs == 0) == (v_form == "shared-G") and (V is None or (c.V.bs == 0) == (v_form == "shared"))
    c.run(monkeypatch, w_mins=(0, 1, 3, n, n + 1), forms=((True, True), (True, False), (False, True)))


def test_degenerate_generators(monkeypatch):
    """Duplicate rows, zero rows, all zero; with all zero nothing weighs 1 or more, and a V in the span is found at distance 0."""
    k, n = 8, 90
    r = _bits(k, n, 3)
    dup = r.copy()
    dup[1::2] = dup[0::2]                       # four rows, each twice: rank <= 4, every word counted 16 times or more
    zrows = r.copy()
    zrows[[0, 3, 7]] = 0
    zero = np.zeros((k, n), dtype=np.uint8)
    c = Case(k, n, [dup, zrows, zero], seed=1)
    assert all(h % 16 == 0 for h in c.want_hist[:n + 1]) and c.want_hist[2 * (n + 1)] == 1 << k
    assert rw.lightest_of(c.weights[2], 1) == -1 and rw.lightest_of(c.weights[2], 0) == 0
    c.run(monkeypatch, w_mins=(0, 1))
    in_span = [dup[0] ^ dup[4], zrows[1] ^ zrows[2] ^ zrows[6], np.zeros(n, dtype=np.uint8)]
    c = Case(k, n, [dup, zrows, zero], in_span, seed=2)
    assert all(c.want_hist[b * (n + 1)] > 0 for b in range(3))
    assert [rw.lightest_of(w, 0) for w in c.weights] == [(1 << 0) | (1 << 4), (1 << 1) | (1 << 2) | (1 << 6), 0]
    c.run(monkeypatch, w_mins=(0, 1))
    # every bit beyond column n set in G and V of members 1 and 2 (n = 90 leaves 38 of them per row): they must not count
    t = Case(k, n, [zero, zero, r], [np.zeros(n, dtype=np.uint8)] * 2 + [r[5]], seed=3, tail_ones=(1, 2))
    assert t.want_hist[0] == t.want_hist[n + 1] == 1 << k
    t.run(monkeypatch, w_mins=(0, 1))


def _closed_form(k, ones, what):
    """G = [I_k | I_k], one member, no brute force: hist[2j] = C(k, j); lightest at w_min = 1 is message 1 (weight 2), at w_min = n and
    n - 1 the all-ones message.  ones: V = ones on the first half, so every word weighs k: 2^k counts in ONE bin.  On the path the
    caller has routed to."""
    n = 2 * k
    G = Operand([rw.doubled_identity(k)], k, n, "gaps", k)
    V = Operand([np.concatenate([np.ones(k, dtype=np.uint8), np.zeros(k, dtype=np.uint8)])[None, :]], 1, n, "gaps", k + 1) if ones else None
    v = (V.ptr, 0) if ones else (0, 0)
    if ones:
        want_hist = np.zeros(n + 1, dtype=np.int64)
        want_hist[k] = 1 << k
        cases = [(0, k << 40), (k, k << 40), (k + 1, -1)]
    else:
        want_hist = rw.doubled_identity_hist(k)
        cases = [(1, (2 << 40) | 1), (n, (n << 40) | ((1 << k) - 1)), (n - 1, (n << 40) | ((1 << k) - 1))]
    for w_min, want_light in cases:
        hist, light = Out(np.int64, n + 1, 5), Out(np.int64, 1, 6)
        m4ri_amd.rowspace_weights_batch_dev(G.ptr, G.stride, 0, k, n, *v, 1, w_min, hist.ptr, light.ptr)
        torch.cuda.synchronize()
        hist.check(want_hist, f"hist (k = {k}, {what})")
        light.check([want_light], f"lightest at w_min = {w_min}")
    assert G.unchanged() and (V is None or V.unchanged())
    return want_hist


@pytest.mark.parametrize("ones", [False, True], ids=["binomial", "one-bin"])
def test_closed_forms_at_k_20_also_by_brute_force(monkeypatch, ones):
    k = 20
    G = rw.doubled_identity(k)
    V = np.concatenate([np.ones(k, dtype=np.uint8), np.zeros(k, dtype=np.uint8)]) if ones else None
    brute = rw.hist_of(rw.weights(G, V), 2 * k)
    for path in (0, 1):
        _route(monkeypatch, path)
        assert np.array_equal(_closed_form(k, ones, f"path {path}"), brute)


@pytest.mark.parametrize("ones", [False, True], ids=["binomial", "one-bin"])
@pytest.mark.parametrize("k,path", [(25, 0), (26, 0), (24, 1), (25, 1), (26, 1), (27, 1), (30, 1), (31, 1), (32, 1), (33, 1)])
def test_closed_forms_across_the_splits_beyond_18(monkeypatch, k, path, ones):
    """The splits of the module docstring that the k sweep cannot reach; at k = 33 the one bin holds 2^33: the counters are 64-bit."""
    _route(monkeypatch, path)
    want = _closed_form(k, ones, f"path {path}")
    assert int(want.sum()) == 1 << k and (not ones or k < 33 or int(want.max()) > 1 << 32)


def test_k_27_goes_to_path_1_whatever_the_override(monkeypatch):
    """The override is clamped to 26: a wave of its own would need 21 low bits and more."""
    monkeypatch.setenv(PATH0, "40")
    _closed_form(27, False, "override 40")
    _closed_form(27, True, "override 40")


def test_on_a_side_stream_and_captured_into_a_graph(monkeypatch):
    """A capture of one call on path 0 and one on path 1 (its initialisation kernel included): nothing runs while capturing (the
    outputs keep their dirt), then two replays, each on freshly dirtied outputs.  One stream, no parallel branches."""
    cases = []
    for path, (k, n) in ((0, (10, 100)), (1, (15, 100))):
        c = Case(k, n, _members(k, n, 3, 40 + path), _words(n, 3, path), seed=50 + path)
        cases.append((path, c))
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    for path, c in cases:  # a side stream first: the calls are plain launches on the stream they are given
        _route(monkeypatch, path)
        outs = (Out(np.int64, c.batch * (c.n + 1), 80 + path), Out(np.int64, c.batch, 90 + path))
        torch.cuda.synchronize()  # the windows are uploaded on the default stream
        c.call(1, stream=side.cuda_stream, outs=outs)
        side.synchronize()
        c.check(outs, 1)
    held = [(Out(np.int64, c.batch * (c.n + 1), 60 + path), Out(np.int64, c.batch, 70 + path)) for path, c in cases]
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
