"""m4ri_amd_row_sums_collide_list_batch_dev and m4ri_amd_row_sums_words_batch_dev (include/m4ri_amd.h, rowsums_collide_batch.hip,
rowsums_words_batch.hip): the keys of the colliding pairs in a weight band, their true count, and the words behind listed keys, against
NumPy on the unpacked bits (tests/collide_list_cases.py), on every path a member can be routed to.  Operands, windows and output frames
are those of tests/test_gpu_row_sums_collide.py: everything dirty, every output a window in a dirty frame that must come back unchanged
outside the named entries -- the unwritten tail of a list and the rows of W from m_b on count as outside.

Where the code changes its ways:
  cap            0 (list NULL or given), below, at and above the count: the slot is taken either way, the key stored below cap only
  the band       w_min > w_max, w_min = w_max on an occupied and on an empty weight, w_max > n
  path 0 / 1     the slot from a counter in LDS and one plain store of the count / a returning global atomic per key after the
                 initialisation kernel; refused and degenerate members are answered by the window check and the initialisation kernel
  N1             1, 64, 65 and 1035 (the 1024-thread configuration)
  words          a group of 1, 2, 4, 8, 16 lanes per row; the last word full or one bit; keys the device must skip"""
from math import comb

import numpy as np
import pytest
import torch

import collide_list_cases as cl
import m4ri_amd
import rowsums_cases as rc
from test_gpu_reduce_batch import FRAME, Operand, Out
from test_gpu_row_sums_collide import Case, _bits, _invertible, _members, _paths, _route, _window, _words

pytestmark = pytest.mark.gpu
MASK = cl.RANK_MASK


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    assert m4ri_amd.lib().m4ri_amd_device_count() >= 1, "no HIP device visible: the gpu tests have nothing to run on"
    m4ri_amd.init(0)
    torch.cuda.set_device(0)


def _pack(bits):
    """The words of one row of bits, bit j of word w = column 64 w + j."""
    full = np.zeros((len(bits) + 63) // 64 * 64, dtype=np.uint8)
    full[:len(bits)] = bits
    return np.packbits(full, bitorder="little").view(np.uint64)


class WordsOut:
    """W of a words call: `batch` members of `rows` rows of n bits, dirty in the valid bits, the tail bits, the padding and the gaps."""

    def __init__(self, batch, rows, n, layout, seed):
        self.n, self.width = n, (n + 63) // 64
        self.op = Operand([_bits(rows, n, seed + b) for b in range(max(batch, 2))], rows, n, layout, seed)    # two members at least: a real batch stride
        self.ptr, self.stride, self.bs = self.op.ptr, self.op.stride, self.op.bs
        self.off = (self.op.ptr - self.op.dev.data_ptr()) // 8

    def check(self, want, what):
        """want: {(member, row): bits}; every other bit of the array as it was."""
        exp, valid = self.op.host.copy(), _pack(np.ones(self.n, dtype=np.uint8))
        for (b, i), bits in want.items():
            at = self.off + b * self.bs + i * self.stride
            exp[at:at + self.width] = (exp[at:at + self.width] & ~valid) | _pack(bits)
        got = self.op.dev.cpu().numpy().view(np.uint64)
        bad = np.flatnonzero(got != exp)
        assert bad.size == 0, f"{what}: {bad.size} words of W differ, the first at {bad[:5] - self.off}"


class LCase(Case):
    """tests/test_gpu_row_sums_collide.py's Case with the list call, its checks, and the words of the lists it gives."""

    def __init__(self, k, n, k1, t1, t2, G, V=None, cols=None, ell=None, **kw):
        super().__init__(k, n, k1, t1, t2, G, V, cols, ell, **kw)
        self.Gb, self.Vb = G, V

    def bits(self, b):
        return self.Gb[b if len(self.Gb) > 1 else 0], (None if self.Vb is None else self.Vb[b if len(self.Vb) > 1 else 0])

    def want_keys(self, w_min, w_max):
        """Per member: the sorted qualifying keys, None for a refused member."""
        return [None if f is None else cl.keys_of(f[0], f[1], w_min, w_max) for f in self.found]

    def outs(self, cap, l_bs, seed=0):
        return (Out(np.int64, self.batch * (self.n + 1), self.seed + seed + 10), Out(np.int64, self.batch, self.seed + seed + 11),
                Out(np.int64, max((self.batch - 1) * l_bs + cap, 0), self.seed + seed + 12), Out(np.int64, self.batch, self.seed + seed + 13))

    def call_list(self, w_min, w_max, cap, l_bs=None, hist=True, lightest=True, lst=True, null_list=False, stream=0, outs=None):
        l_bs = cap if l_bs is None else l_bs
        outs = outs or self.outs(cap, l_bs)
        g = (self.G.ptr, self.G.stride, self.G.bs) if self.G else (0, 0, 0)
        v = (self.V.ptr, self.V.bs) if self.V else (0, 0)
        c = (self.cols.ptr, self.cols.bs) if self.cols else (0, 0)
        m4ri_amd.row_sums_collide_list_batch_dev(*g, self.k, self.n, *v, self.batch, self.k1, self.t1, self.t2, *c, self.ell, w_min, w_max,
                                                 outs[0].ptr if hist else 0, outs[1].ptr if lightest else 0, outs[2].ptr if lst and not null_list else 0,
                                                 l_bs, cap, outs[3].ptr if lst else 0, stream=stream)
        return outs

    def check_list(self, outs, w_min, w_max, cap, l_bs=None, hist=True, lightest=True, lst=True, null_list=False, ran=True):
        """Every output and operand; returns the listed keys per member as they stand on the device (None where the list was not written)."""
        l_bs = cap if l_bs is None else l_bs
        self.check(outs[:2], w_min, hist, lightest, ran)
        if not (lst and ran):
            assert outs[2].untouched() and outs[3].untouched(), "list or count written"
            return None
        want = self.want_keys(w_min, w_max)
        outs[3].check([-1 if w is None else len(w) for w in want], f"count at {w_min} .. {w_max}")
        got, exp, listed = outs[2].dev.cpu().numpy(), outs[2].host.copy(), []
        for b, w in enumerate(want):
            m = 0 if w is None or null_list else min(len(w), cap)
            at = FRAME + b * l_bs
            keys = got[at:at + m].copy()
            if w is not None and len(w) <= cap:
                assert np.array_equal(np.sort(keys), w), f"member {b}: the list is not the qualifying set"
            else:
                assert len(set(keys.tolist())) == m and set(keys.tolist()) <= set([] if w is None else w.tolist()), f"member {b}: {m} of {0 if w is None else len(w)}"
            exp[at:at + m] = keys
            listed.append(keys)
        assert np.array_equal(got, exp), "the list was written outside its first min(count, cap) entries"
        return listed

    def words(self, outs, listed, cap, l_bs, layout="gaps"):
        """The words call on the list and the count of a list call whose counts are at most cap: every row the word of its key, its
        weight the key's, everything else of W as it was."""
        W = WordsOut(self.batch, cap, self.n, layout, self.seed + 20)
        skipped, before = Out(np.int32, self.batch, self.seed + 21), outs[2].dev.cpu().numpy()
        g = (self.G.ptr, self.G.stride, self.G.bs) if self.G else (0, 0, 0)
        v = (self.V.ptr, self.V.bs) if self.V else (0, 0)
        m4ri_amd.row_sums_words_batch_dev(*g, self.k, self.n, *v, self.batch, self.k1, self.t1, self.t2, outs[2].ptr, l_bs, cap, outs[3].ptr, W.ptr, W.stride, W.bs,
                                          skipped.ptr)
        torch.cuda.synchronize()
        want = {}
        for b, keys in enumerate(listed):
            G, V = self.bits(b)
            rows = cl.words_of(G, V, self.k1, self.t1, self.t2, keys & MASK)
            assert rows.sum(axis=1).tolist() == (keys >> 40).tolist(), f"member {b}: a key's weight is not its word's"
            want.update({(b, i): r for i, r in enumerate(rows)})
        W.check(want, "words of the list")
        skipped.check([0] * self.batch, "skipped")
        assert np.array_equal(outs[2].dev.cpu().numpy(), before) and (self.G is None or self.G.unchanged()) and (self.V is None or self.V.unchanged())

    def run_list(self, monkeypatch, w_min, w_max, cap, l_bs=None, words=True, **forms):
        """Both paths where the shape allows; the words of the list where it is complete.  Returns the sorted lists per path."""
        l_bs, got = cap if l_bs is None else l_bs, {}
        for path in _paths(self.k, self.n, self.k1, self.t1, self.t2):
            _route(monkeypatch, path)
            outs = self.call_list(w_min, w_max, cap, l_bs, **forms)
            listed = self.check_list(outs, w_min, w_max, cap, l_bs, **forms)
            got[path] = listed
            want = self.want_keys(w_min, w_max)
            if words and listed is not None and self.n and cap and not forms.get("null_list") and all(w is None or len(w) <= cap for w in want):
                self.words(outs, listed, cap, l_bs)
        return got


def _base(ell, batch=2, seed=5):
    """k = 12, k1 = 6, t1 = t2 = 2, n = 75: 225 pairs per member."""
    k, k1, n = 12, 6, 75
    win = [_window(n, ell, seed + b) for b in range(batch)] if ell else None
    return LCase(k, n, k1, 2, 2, _members(k, n, batch, seed, win), _words(n, batch, seed, win), win, ell=ell, seed=seed)


# ---- 1. cap against count ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cap", [0, 1, 224, 225, 300])
def test_cap_against_count(monkeypatch, cap):
    """Without a window all 225 pairs qualify on 0 .. n: below, at and above the count; cap = 0 with and without a list pointer."""
    c = _base(0)
    assert all(len(w) == 225 for w in c.want_keys(0, c.n))
    c.run_list(monkeypatch, 0, c.n, cap)
    if cap == 0:
        c.run_list(monkeypatch, 0, c.n, 0, null_list=True)


def test_batch_zero_touches_nothing(monkeypatch):
    c = _base(3)
    c.batch = 0
    for path in (0, 1):
        _route(monkeypatch, path)
        outs = LCase.outs(c, 4, 4)
        c.check_list(c.call_list(0, c.n, 4, outs=outs), 0, c.n, 4, ran=False)


# ---- 2. the weight band -----------------------------------------------------------------------------------------------------------------

def test_the_weight_band(monkeypatch):
    c = _base(3)
    n, cap = c.n, 225
    weights = sorted(set(c.found[0][0].tolist()))
    empty = next(w for w in range(weights[0], weights[-1]) if w not in weights and all(w not in f[0] for f in c.found))
    assert len(weights) > 3 and all(2 <= len(f[0]) <= cap for f in c.found)
    for w_min, w_max in [(9, 8), (n, 0), (weights[1], weights[1]), (empty, empty), (0, n + 1), (weights[1], 1 << 40), (0, n), (weights[2], weights[-2])]:
        got = c.run_list(monkeypatch, w_min, w_max, cap)
        want = c.want_keys(w_min, w_max)
        if w_min > w_max or w_min == empty:
            assert all(len(w) == 0 for w in want)
        elif w_min == weights[1]:
            assert len(want[0]) > 0
        assert all(np.array_equal(np.sort(x), w) for listed in got.values() for x, w in zip(listed, want))
    # with hist and lightest also given, from the device's own outputs: count is the band sum of hist, min(list) is lightest at w_max = n
    for path in (0, 1):
        _route(monkeypatch, path)
        for w_min, w_max in [(weights[1], weights[-2]), (weights[1], n)]:
            outs = c.call_list(w_min, w_max, cap)
            listed = c.check_list(outs, w_min, w_max, cap)
            h = outs[0].dev.cpu().numpy()[FRAME:FRAME + c.batch * (n + 1)].reshape(c.batch, n + 1)
            count, light = outs[3].dev.cpu().numpy()[FRAME:FRAME + c.batch], outs[1].dev.cpu().numpy()[FRAME:FRAME + c.batch]
            assert count.tolist() == h[:, w_min:w_max + 1].sum(axis=1).tolist()
            if w_max == n:
                assert [int(x.min()) for x in listed] == light.tolist()


# ---- 3. the outputs present or NULL -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("hist,lightest,lst", [(h, l, s) for h in (True, False) for l in (True, False) for s in (True, False) if h or l or s])
def test_every_combination_of_outputs(monkeypatch, hist, lightest, lst):
    c = _base(3)
    c.run_list(monkeypatch, 1, 40, 64, hist=hist, lightest=lightest, lst=lst)
    if lst:
        c.run_list(monkeypatch, 1, 40, 0, hist=hist, lightest=lightest, null_list=True)      # a filtered count alone


# ---- 4. the left list -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k1,t1,k2,t2,ell", [(1, 1, 9, 2, 3), (64, 1, 6, 1, 5), (65, 1, 6, 2, 5), (46, 2, 8, 2, 8)])
def test_left_list_sizes(monkeypatch, k1, t1, k2, t2, ell):
    """N1 = 1, 64, 65 (0, 6 and 7 bucket bits) and 1035: above 1024 the workgroup has 1024 threads."""
    k, n, batch = k1 + k2, 70, 2
    assert comb(k1, t1) in (1, 64, 65, 1035)
    win = [_window(n, ell, k1 + b) for b in range(batch)]
    c = LCase(k, n, k1, t1, t2, _members(k, n, batch, 3 * k + t1, win), _words(n, batch, k, win), win, seed=k)
    w_max = max(int(np.sort(f[0])[min(3, len(f[0]) - 1)]) for f in c.found)      # a band that ends at a low weight and leaves a few
    want = c.want_keys(0, w_max)
    assert all(len(w) >= 2 for w in want) and any(len(w) < len(f[0]) for w, f in zip(want, c.found))
    c.run_list(monkeypatch, 0, w_max, max(len(w) for w in want))
    c.run_list(monkeypatch, 0, w_max, 1)


# ---- 5. refused members -----------------------------------------------------------------------------------------------------------------

def test_refused_members_between_good_ones(monkeypatch):
    """Members 1 and 2 have a window entry of -1 and of n: count -1, no list entry written; members 0 and 3 exact."""
    k, k1, n, batch, ell = 12, 6, 70, 4, 5
    win = [_window(n, ell, 20 + b) for b in range(batch)]
    win[1][3] = -1
    win[2][0], win[2][4] = n, 1 << 30
    c = LCase(k, n, k1, 2, 2, _members(k, n, batch, 17, win), _words(n, batch, 3, win), win, seed=n)
    want = c.want_keys(0, n)
    assert [w is None for w in want] == [False, True, True, False] and len(want[0]) >= 2 and len(want[3]) >= 2
    c.run_list(monkeypatch, 0, n, max(len(want[0]), len(want[3])), l_bs=230)
    c.run_list(monkeypatch, 0, n, 1)
    shared = LCase(k, n, k1, 2, 2, _members(k, n, 2, 18), None, [[0, 1, n, 2]], seed=n + 1)     # one refused window for all members
    assert shared.want_keys(0, n) == [None, None]
    shared.run_list(monkeypatch, 0, n, 8)


# ---- 6. degenerate members --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k,n,k1,t1,t2", [(8, 0, 3, 1, 1), (8, 70, 3, 4, 1), (8, 70, 3, 1, 6), (8, 0, 3, 4, 1)])
def test_degenerate_members(monkeypatch, k, n, k1, t1, t2):
    """No columns: N1 * N2 = 15 pairs of weight 0, listed if w_min = 0; no pairs: count 0.  The initialisation kernel alone."""
    batch = 3
    G = _members(k, n, batch, k + t1) if n else [np.zeros((k, 0), dtype=np.uint8)] * batch
    c = LCase(k, n, k1, t1, t2, G, None, None, ell=0, seed=t1)
    pairs = comb(k1, t1) * comb(k - k1, t2)
    assert pairs == (15 if t1 == t2 == 1 else 0) and [len(w) for w in c.want_keys(0, 5)] == [pairs if n == 0 else 0] * batch
    for cap in (4, 20):
        got = c.run_list(monkeypatch, 0, 5, cap, l_bs=cap + 2)
        c.run_list(monkeypatch, 1, 5, cap)
        c.run_list(monkeypatch, 0, 0, cap, hist=False, lightest=False)
    if pairs:
        assert all(sorted(x.tolist()) == list(range(15)) for x in got[0])


def test_no_columns_but_a_window_is_refused(monkeypatch):
    c = LCase(6, 0, 3, 1, 1, [np.zeros((6, 0), dtype=np.uint8)] * 2, cols=[[0, 0], [0, -3]], seed=3)
    assert c.want_keys(0, 0) == [None, None]
    c.run_list(monkeypatch, 0, 0, 4)


# ---- 7. slices --------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k1,t1,k2,t2,batch,slices", [(4, 2, 40, 2, 2, 4), (30, 2, 60, 2, 1, 5), (3, 1, 24, 3, 3, 8)])
def test_slices_of_the_right_list(monkeypatch, k1, t1, k2, t2, batch, slices):
    """The shapes of tests/test_gpu_row_sums_collide.py's test of the same name: several workgroups of path 1 take slots of one member."""
    k, n, ell = k1 + k2, 75, 6
    n1, n2 = comb(k1, t1), comb(k2, t2)
    length = max(n1, 256)
    assert m4ri_amd.row_sums_collide_slices(k, n, k1, t1, t2, ell, batch) == slices
    win = [_window(n, ell, 50 + b) for b in range(batch)]
    c = LCase(k, n, k1, t1, t2, _members(k, n, batch, k, win, patterns=4), _words(n, batch, k1, win), win, seed=k2)
    want = c.want_keys(0, n)
    assert all(len(set(((w & MASK) % n2 // length).tolist())) == slices for w in want)          # qualifying pairs in every slice
    cap = max(len(w) for w in want)
    got = c.run_list(monkeypatch, 0, n, cap, l_bs=cap + 1)
    assert all(np.array_equal(np.sort(a), np.sort(b)) for a, b in zip(got[0], got[1]))
    small = min(len(w) for w in want) // 2
    assert small >= slices
    c.run_list(monkeypatch, 0, n, small)      # cap below count: the workgroups run into it together


# ---- 8. per-member strides --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("form", ["shared-G", "shared-V", "shared-window", "per-member"])
def test_list_stride_and_operand_sharing(monkeypatch, form):
    k, k1, n, batch, ell = 13, 6, 100, 3, 5
    win = [_window(n, ell, 3 + b) for b in range(1 if form == "shared-window" else batch)]
    wins = win * batch if len(win) == 1 else win
    G = _members(k, n, 1 if form == "shared-G" else batch, 5, wins)
    if form == "shared-G":
        G[0][:, [c for w in wins for c in w]] = 0
    V = _words(n, 1 if form == "shared-V" else batch, 2, wins if form != "shared-V" else None)
    if form == "shared-V":
        V[0][[c for w in wins for c in w]] = 0
    c = LCase(k, n, k1, 2, 2, G, V, win, seed=len(form))
    want = c.want_keys(0, 50)
    assert c.batch == batch and all(len(w) >= 2 for w in want)
    cap = max(len(w) for w in want)
    c.run_list(monkeypatch, 0, 50, cap, l_bs=cap + 7)


# ---- 10. words from other keys ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [64, 65, 130, 300, 1024])
def test_words_from_given_keys(n):
    """count = NULL, a count above cap, -1 and 0 in count; rubbish weight bits; a key < 0 and a key with r = N1 * N2 exactly: skipped and
    counted, their rows and the rows from m_b on as they were.  n = 64 and 1024 fill the last word, 65 has one bit in it; 1, 2, 4, 8 and
    16 lanes per row."""
    k, k1, t1, t2, batch, cap = 11, 5, 2, 3, 4, 9
    pairs, rng = comb(k1, t1) * comb(k - k1, t2), np.random.default_rng(n)
    Gb, Vb = _members(k, n, batch, n), _words(n, batch, n + 1)
    G, V = Operand(Gb, k, n, "odd" if n % 2 else "even", 1), Operand([v[None, :] for v in Vb], 1, n, "gaps", 2)
    l_bs = cap + 2
    keys = Out(np.int64, (batch - 1) * l_bs + cap, 3)
    host = keys.host.copy()
    ranks = rng.integers(0, pairs, size=(batch, cap))
    ranks[0, :3], ranks[3, -1] = (0, pairs - 1, pairs - 1), 0      # the ends of the range, one key twice
    for b in range(batch):
        host[FRAME + b * l_bs:FRAME + b * l_bs + cap] = ranks[b] | (rng.integers(0, 1 << 22, size=cap) << 40)      # rubbish above the rank
    bad = {(1, 2): -1, (1, 5): pairs, (2, 0): (7 << 40) | (pairs + 3), (2, 8): -(1 << 62), (2, 4): MASK}
    for (b, i), x in bad.items():
        host[FRAME + b * l_bs + i] = x
    keys.dev.copy_(torch.from_numpy(host))
    rows = lambda b, m: {(b, i): cl.words_of(Gb[b], Vb[b], k1, t1, t2, [ranks[b, i]])[0] for i in range(m) if (b, i) not in bad}
    for counts in (None, [cap, 3, cap + 5, 0], [-1, cap, -7, 1 << 40]):
        W, skipped = WordsOut(batch, cap, n, "gaps", 4), Out(np.int32, batch, 5)
        count = torch.tensor(counts or [0], dtype=torch.int64, device="cuda")
        m4ri_amd.row_sums_words_batch_dev(G.ptr, G.stride, G.bs, k, n, V.ptr, V.bs, batch, k1, t1, t2, keys.ptr, l_bs, cap, count.data_ptr() if counts else 0,
                                          W.ptr, W.stride, W.bs, skipped.ptr)
        torch.cuda.synchronize()
        m = [cap if counts is None else min(max(x, 0), cap) for x in (counts or [0] * batch)]
        want = {}
        for b in range(batch):
            want.update(rows(b, m[b]))
        W.check(want, f"count {counts}")
        skipped.check([sum(1 for (b2, i) in bad if b2 == b and i < m[b]) for b in range(batch)], f"skipped, count {counts}")
        assert np.array_equal(keys.dev.cpu().numpy(), host) and G.unchanged() and V.unchanged()
    # without the skipped array, one shared G, no V, one member
    W = WordsOut(1, cap, n, "dense", 6)
    m4ri_amd.row_sums_words_batch_dev(G.ptr, G.stride, 0, k, n, 0, 0, 1, k1, t1, t2, keys.ptr, 0, cap, 0, W.ptr, W.stride, 0)
    torch.cuda.synchronize()
    W.check({(0, i): cl.words_of(Gb[0], None, k1, t1, t2, [ranks[0, i]])[0] for i in range(cap)}, "one member")


def test_words_beyond_one_workgroup_of_rows():
    """cap = 600: three workgroups of 256 rows per member, the last one ragged; the count cuts member 1 inside the second."""
    k, k1, t1, t2, n, batch, cap = 20, 10, 2, 2, 200, 2, 600
    pairs = comb(k1, t1) * comb(k - k1, t2)
    Gb = _members(k, n, batch, 8)
    G = Operand(Gb, k, n, "gaps", 1)
    ranks = np.random.default_rng(9).integers(0, pairs, size=(batch, cap))
    keys = torch.from_numpy(ranks.copy()).cuda()
    count = torch.tensor([cap, 300], dtype=torch.int64, device="cuda")
    W, skipped = WordsOut(batch, cap, n, "gaps", 4), Out(np.int32, batch, 5)
    m4ri_amd.row_sums_words_batch_dev(G.ptr, G.stride, G.bs, k, n, 0, 0, batch, k1, t1, t2, keys.data_ptr(), cap, cap, count.data_ptr(), W.ptr, W.stride, W.bs,
                                      skipped.ptr)
    torch.cuda.synchronize()
    want = {}
    for b, m in enumerate((cap, 300)):
        want.update({(b, i): r for i, r in enumerate(cl.words_of(Gb[b], None, k1, t1, t2, ranks[b, :m]))})
    W.check(want, "600 rows")
    skipped.check([0, 0], "skipped")


@pytest.mark.parametrize("k,t", [(10, 0), (10, 1), (40, 3), (12, 5)])
def test_words_of_the_keys_of_row_sums_weights(k, t):
    """t2 = 0, k1 = k on m4ri_amd_row_sums_weights_batch_dev's lightest: the word of the named set, of the weight the key names."""
    n, batch = 100, 3
    Gb, Vb = _members(k, n, batch, 12), _words(n, batch, 13)
    g, v = Operand(Gb, k, n, "gaps", 1), Operand([x[None, :] for x in Vb], 1, n, "gaps", 2)
    light = Out(np.int64, batch, 4)
    m4ri_amd.row_sums_weights_batch_dev(g.ptr, g.stride, g.bs, k, n, v.ptr, v.bs, batch, t, 1, 0, light.ptr)
    W, skipped = WordsOut(batch, 1, n, "gaps", 5), Out(np.int32, batch, 6)
    m4ri_amd.row_sums_words_batch_dev(g.ptr, g.stride, g.bs, k, n, v.ptr, v.bs, batch, k, t, 0, light.ptr, 1, 1, 0, W.ptr, W.stride, W.bs, skipped.ptr)
    torch.cuda.synchronize()
    got = light.dev.cpu().numpy()[FRAME:FRAME + batch]
    light.check([rc.expect(G, V, t, 1)[1] for G, V in zip(Gb, Vb)], "lightest")
    rows = [cl.words_of(G, V, k, t, 0, [x & MASK])[0] for G, V, x in zip(Gb, Vb, got)]
    assert [int(r.sum()) for r in rows] == (got >> 40).tolist()
    W.check({(b, 0): r for b, r in enumerate(rows)}, "the lightest sums")
    skipped.check([0] * batch, "skipped")


# ---- 11. end to end ---------------------------------------------------------------------------------------------------------------------

def test_a_stern_decoder_end_to_end(monkeypatch):
    """The three members of tests/test_gpu_row_sums_collide.py's Stern iteration (a [96, 32] code, wt(e) = 6 with two errors in each half
    of the information set, none in the window): after the systematic form, the list call with w_min = 1, w_max = 6, cap = 4 finds one
    pair per member, and the words call writes exactly the planted e.  Nothing is unranked on the host."""
    k, n, batch, ell, cap = 32, 96, 3, 12, 4
    rng = np.random.default_rng(2024)
    stacked, orders, errors = [], [], []
    for b in range(batch):
        order = rng.permutation(n)
        systematic = np.zeros((k, n), dtype=np.uint8)
        systematic[:, order[:k]] = np.eye(k, dtype=np.uint8)
        systematic[:, order[k:]] = rng.integers(0, 2, size=(k, n - k), dtype=np.uint8)
        G = (_invertible(k, rng).astype(np.int64) @ systematic % 2).astype(np.uint8)
        places = sorted(rng.choice(16, 2, replace=False)) + sorted(16 + rng.choice(16, 2, replace=False)) + \
            sorted(k + ell + rng.choice(n - k - ell, 2, replace=False))
        e = np.zeros(n, dtype=np.uint8)
        e[order[places]] = 1
        y = (rng.integers(0, 2, size=k) @ G.astype(np.int64) % 2).astype(np.uint8) ^ e
        stacked.append(np.concatenate([G, y[None, :]]))
        orders.append(order.astype(np.int32))
        errors.append(e)
    o_bs = n + 4
    order_host = np.full(batch * o_bs, -9, dtype=np.int32)
    for b in range(batch):
        order_host[b * o_bs:b * o_bs + n] = orders[b]
    order_dev = torch.from_numpy(order_host.copy()).cuda()
    for path in (0, 1):
        _route(monkeypatch, path)
        D = Operand(stacked, k + 1, n, "gaps", 5)
        rank = torch.full((batch,), -7, dtype=torch.int32, device="cuda")
        m4ri_amd.echelonize_order_batch_dev(D.ptr, D.stride, D.bs, D.ptr, D.stride, D.bs, k + 1, n, k, order_dev.data_ptr(), o_bs, k, batch, 1, rank.data_ptr())
        lst, count = Out(np.int64, (batch - 1) * (cap + 1) + cap, 6), Out(np.int64, batch, 7)
        W, skipped = WordsOut(batch, cap, n, "gaps", 8), Out(np.int32, batch, 9)
        v = D.ptr + 8 * k * D.stride
        m4ri_amd.row_sums_collide_list_batch_dev(D.ptr, D.stride, D.bs, k, n, v, D.bs, batch, 16, 2, 2, order_dev.data_ptr() + 4 * k, o_bs, ell, 1, 6, 0, 0,
                                                 lst.ptr, cap + 1, cap, count.ptr)
        m4ri_amd.row_sums_words_batch_dev(D.ptr, D.stride, D.bs, k, n, v, D.bs, batch, 16, 2, 2, lst.ptr, cap + 1, cap, count.ptr, W.ptr, W.stride, W.bs, skipped.ptr)
        torch.cuda.synchronize()
        assert rank.cpu().tolist() == [k] * batch
        count.check([1] * batch, "count")
        W.check({(b, 0): errors[b] for b in range(batch)}, "the error vectors")
        skipped.check([0] * batch, "skipped")
        got = lst.dev.cpu().numpy()
        assert [int(got[FRAME + b * (cap + 1)]) >> 40 for b in range(batch)] == [6] * batch
        keep = np.ones(len(got), dtype=bool)
        keep[[FRAME + b * (cap + 1) for b in range(batch)]] = False
        assert np.array_equal(got[keep], lst.host[keep]), "the list was written behind its one entry"
    assert np.array_equal(order_dev.cpu().numpy(), order_host)


# ---- 12. streams and graphs -------------------------------------------------------------------------------------------------------------

def test_on_a_side_stream_and_captured_into_a_graph(monkeypatch):
    """A side stream first; then one capture of a list call on path 0, one on path 1 (its initialisation kernel included) and a words call
    that reads the counts and keys the captured path-1 call leaves: nothing runs while capturing, then one replay on freshly dirtied
    outputs.  One stream, no parallel branches."""
    cap, cases = 40, []
    for path, (k, k1, w_max) in ((0, (12, 6, 42)), (1, (44, 4, 36))):      # bands that leave 6 .. 29 keys per member
        win = [_window(100, 5, 60 + k + b) for b in range(3)]
        cases.append((path, LCase(k, 100, k1, 2, 2, _members(k, 100, 3, 40 + k, win), _words(100, 3, path, win), win, seed=50 + k), w_max))
    assert all(2 <= len(w) <= cap for _, c, w_max in cases for w in c.want_keys(1, w_max))
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    for path, c, w_max in cases:
        _route(monkeypatch, path)
        outs = c.outs(cap, cap, seed=30)
        torch.cuda.synchronize()
        c.call_list(1, w_max, cap, stream=side.cuda_stream, outs=outs)
        side.synchronize()
        c.check_list(outs, 1, w_max, cap)
    held = [c.outs(cap, cap, seed=40) for _, c, _ in cases]
    last = cases[1][1]
    W, skipped = WordsOut(last.batch, cap, last.n, "gaps", 70), Out(np.int32, last.batch, 71)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        st = torch.cuda.current_stream().cuda_stream
        for (path, c, w_max), outs in zip(cases, held):
            _route(monkeypatch, path)
            c.call_list(1, w_max, cap, stream=st, outs=outs)
        m4ri_amd.row_sums_words_batch_dev(last.G.ptr, last.G.stride, last.G.bs, last.k, last.n, last.V.ptr, last.V.bs, last.batch, last.k1, 2, 2, held[1][2].ptr, cap, cap,
                                          held[1][3].ptr, W.ptr, W.stride, W.bs, skipped.ptr, stream=st)
    for (path, c, w_max), outs in zip(cases, held):
        c.check_list(outs, 1, w_max, cap, ran=False)
    W.check({}, "while capturing")
    assert skipped.untouched()
    g.replay()
    torch.cuda.synchronize()
    for (path, c, w_max), outs in zip(cases, held):
        listed = c.check_list(outs, 1, w_max, cap)
    want = {}
    for b, keys in enumerate(listed):
        want.update({(b, i): r for i, r in enumerate(cl.words_of(*last.bits(b), last.k1, 2, 2, keys & MASK))})
    W.check(want, "after the replay")
    skipped.check([0] * last.batch, "skipped")
