"""m4ri_amd_row_sums_collide_batch_dev (include/m4ri_amd.h, rowsums_collide_batch.hip): the weight distribution and the lightest of the
colliding pairs (t1 left rows, t2 right rows, zero on the window) of every member, against NumPy on the unpacked bits and closed forms
(tests/collide_cases.py), on every path the member can be routed to.  The operands are dirty in their tail bits, padding words and gaps
(the layouts of tests/test_gpu_reduce_batch.py), the windows lie in a dirty int32 array with gaps, and all of them must come back
unchanged; every output is a window inside a larger dirty device array whose frame must come back unchanged.

Where the kernel changes its ways (rowsums_collide_batch.hip; a workgroup tables the N1 left keys in LDS, bucketed on their low
q = min(ceil(log2 N1), ell) bits, and walks a slice of the right list, a lane per right sum):
  n = 0, no pairs         the initialisation kernel alone
  N1 = 1, 64, 65, 55, 66  q = 0, 6, 7; 8128 the largest table (1024 threads, 13 bucket bits held at ell = 10)
  ell = 0                 one bucket, every pair collides; ell below q; ell = 63, 64: the key fills the word
  a refused member        stops after the window check: path 0 writes the refused form itself, path 1 leaves it to the initialisation
  path 0 / path 1         a workgroup per member with plain stores / a workgroup per slice of the right list with atomics"""
from math import comb

import numpy as np
import pytest
import torch

import collide_cases as cc
import m4ri_amd
import rowsums_cases as rc
from m4ri_amd.mzd import Mzd
from test_gpu_reduce_batch import FRAME, Operand, Out

pytestmark = pytest.mark.gpu
PATH0 = "M4RI_AMD_ROW_SUMS_COLLIDE_PATH0_MAX"
P0_MAX = (1 << 32) - 1  # the largest number of pairs per member the override sends to path 0
ALL_FORMS = ((True, True), (True, False), (False, True))


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
        monkeypatch.setenv(PATH0, {0: str(P0_MAX), 1: "-1"}[path])


def _paths(k, n, k1, t1, t2):
    """The paths members of this shape can be sent to: members without columns or pairs are always answered on path 0."""
    pairs = comb(k1, t1) * comb(k - k1, t2)
    if n == 0 or pairs == 0:
        return [0]
    return ([0] if pairs <= P0_MAX else []) + [1]


def _bits(rows, cols, seed):
    return Mzd.random(rows, cols, seed).to_bits()


class Windows:
    """`windows` (lists of ell column indices; one of them = a shared window, batch stride 0) as DEVICE int32, each window followed by a
    gap, inside a dirty frame."""

    def __init__(self, windows, ell, seed):
        rng = np.random.default_rng(seed)
        self.bs = ell + 3 if len(windows) > 1 else 0
        self.host = rng.integers(-(1 << 20), 1 << 20, size=2 * FRAME + len(windows) * (ell + 3)).astype(np.int32)
        for b, w in enumerate(windows):
            assert len(w) == ell
            self.host[FRAME + b * (ell + 3):FRAME + b * (ell + 3) + ell] = w
        self.dev = torch.from_numpy(self.host.copy()).cuda()
        self.ptr = self.dev.data_ptr() + 4 * FRAME

    def unchanged(self):
        return np.array_equal(self.dev.cpu().numpy(), self.host)


class Case:
    """One batch on the device: G (a list of k x n bit matrices; one of them = shared), V (a list of n-bit vectors, one = shared, None =
    absent) and the windows (a list of lists of columns, one = shared; None = no array, the columns 0 .. ell-1); the weights and ranks
    of all colliding pairs computed once (None for a refused member)."""

    def __init__(self, k, n, k1, t1, t2, G, V=None, cols=None, ell=None, layout="gaps", seed=0, tail_ones=()):
        self.k, self.n, self.k1, self.t1, self.t2, self.seed = k, n, k1, t1, t2, seed
        self.ell = len(cols[0]) if cols is not None else ell
        self.batch = max(len(G), len(V) if V is not None else 1, len(cols) if cols is not None else 1)
        self.G = Operand(G, k, n, layout, seed + 1, tail_ones if len(G) > 1 else ()) if k and n else None
        self.V = Operand([v[None, :] for v in V], 1, n, layout, seed + 2, tail_ones if len(V) > 1 else ()) if V is not None and n else None
        self.cols = Windows(cols, self.ell, seed + 3) if cols is not None and self.ell else None
        pick = lambda M, b: M[b if len(M) > 1 else 0]
        self.found = []
        for b in range(self.batch):
            win = pick(cols, b) if cols is not None else list(range(self.ell))
            g = pick(G, b) if k and n else np.zeros((k, n), dtype=np.uint8)
            self.found.append(None if cc.refused(n, win) else cc.collisions(g, pick(V, b) if V is not None else None, k1, t1, t2, win))
        self.want_hist = np.concatenate([cc.refused_form(n)[0] if f is None else rc.hist_of(f[0], n) for f in self.found])

    def collisions(self, b):
        return len(self.found[b][0])

    def call(self, w_min, hist=True, lightest=True, stream=0, outs=None):
        """Launch with fresh dirty output windows (or the given ones); returns them for check()."""
        if outs is None:
            outs = (Out(np.int64, self.batch * (self.n + 1), self.seed + 10), Out(np.int64, self.batch, self.seed + 11))
        g = (self.G.ptr, self.G.stride, self.G.bs) if self.G else (0, 0, 0)
        v = (self.V.ptr, self.V.bs) if self.V else (0, 0)
        c = (self.cols.ptr, self.cols.bs) if self.cols else (0, 0)
        m4ri_amd.row_sums_collide_batch_dev(*g, self.k, self.n, *v, self.batch, self.k1, self.t1, self.t2, *c, self.ell, w_min,
                                            outs[0].ptr if hist else 0, outs[1].ptr if lightest else 0, stream=stream)
        return outs

    def want_light(self, w_min):
        return [-2 if f is None else rc.lightest_of(f[0], f[1], w_min) for f in self.found]

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
        assert self.cols is None or self.cols.unchanged(), "cols was written"

    def run(self, monkeypatch, w_mins=None, forms=ALL_FORMS):
        """Every path the shape can go to, w_min = 0, 1 and n + 2, hist alone, lightest alone and both."""
        for path in _paths(self.k, self.n, self.k1, self.t1, self.t2):
            _route(monkeypatch, path)
            for w_min in w_mins or (0, 1, self.n + 2):
                for hist, lightest in forms:
                    self.check(self.call(w_min, hist, lightest), w_min, hist, lightest)
        assert self.want_light(self.n + 2) == [-2 if f is None else -1 for f in self.found]


def _members(k, n, batch, seed, windows=None, patterns=3):
    """Random generators.  With windows (one per member, or one for all): every row's window bits are one of `patterns` random patterns,
    the zero pattern among them, so that pairs collide on windows of any width."""
    G = [_bits(k, n, seed + b) for b in range(batch)]
    rng = np.random.default_rng(seed)
    for b in range(batch if windows is not None else 0):
        win = [c for c in windows[b if len(windows) > 1 else 0] if 0 <= c < n]
        pats = np.concatenate([np.zeros((1, len(win)), dtype=np.uint8), rng.integers(0, 2, size=(patterns - 1, len(win)), dtype=np.uint8)])
        G[b][:, win] = pats[rng.integers(0, patterns, size=k)]
    return G


def _words(n, count, seed, windows=None):
    """Random words, zero on the windows."""
    V = [_bits(1, n, seed + 100 + b)[0] for b in range(count)]
    for b in range(count if windows is not None else 0):
        V[b][[c for c in windows[b if len(windows) > 1 else 0] if 0 <= c < n]] = 0
    return V


def _window(n, ell, seed):
    """ell columns of 0 .. n-1 in no order, distinct while there are enough of them."""
    rng = np.random.default_rng(seed)
    return [int(c) for c in (rng.permutation(n)[:ell] if ell <= n else rng.integers(0, n, size=ell))]


# ---- degenerate members -----------------------------------------------------------------------------------------------------------------

def test_batch_zero_touches_nothing(monkeypatch):
    c = Case(6, 70, 3, 1, 1, _members(6, 70, 2, 1), cols=[[0, 1], [2, 3]], seed=1)
    c.batch = 0
    for path in (0, 1):
        _route(monkeypatch, path)
        c.check(c.call(0), 0, ran=False)


@pytest.mark.parametrize("k,n,k1,t1,t2,ell", [
    (6, 0, 3, 1, 1, 0), (0, 0, 0, 0, 0, 0), (6, 0, 3, 4, 1, 0),   # no columns: all pairs in bin 0; no pairs either
    (8, 70, 4, 2, 2, 0),                                          # no window: every pair collides
    (8, 70, 4, 0, 2, 3), (8, 70, 4, 2, 0, 3), (8, 70, 4, 0, 0, 3), (0, 70, 0, 0, 0, 2),   # an empty set on either side: the one set of rank 0
    (8, 70, 0, 0, 2, 3), (8, 70, 0, 1, 2, 3),                     # k1 = 0: the empty left set, or no left set at all
    (8, 70, 8, 3, 0, 3), (8, 70, 8, 3, 1, 3),                     # k1 = k likewise on the right
    (8, 70, 4, 5, 1, 3), (8, 70, 4, 1, 5, 3),                     # t1 > k1, t2 > k2: no pairs
])
def test_degenerate_members(monkeypatch, k, n, k1, t1, t2, ell):
    batch = 3
    win = [_window(n, ell, 7 + b) for b in range(batch)] if ell and n else None
    G = _members(k, n, batch, 10 * k + t1, win) if k and n else [np.zeros((k, n), dtype=np.uint8)] * batch
    c = Case(k, n, k1, t1, t2, G, _words(n, batch, k + t2, win) if n else None, win, ell=ell, seed=k + t1 + t2)
    pairs = comb(k1, t1) * comb(k - k1, t2)
    if n == 0:
        assert c.want_hist.tolist() == [pairs] * batch and c.want_light(0) == [0 if pairs else -1] * batch and c.want_light(1) == [-1] * batch
    if ell == 0 or pairs == 0:
        assert all(c.collisions(b) == pairs for b in range(batch))
    c.run(monkeypatch)


def test_no_columns_but_a_window_is_refused(monkeypatch):
    """n = 0 with a window given: every entry is outside 0 .. n-1."""
    c = Case(6, 0, 3, 1, 1, [np.zeros((6, 0), dtype=np.uint8)] * 2, cols=[[0, 0], [0, -3]], seed=3)
    assert c.found == [None, None] and c.want_hist.tolist() == [-1, -1]
    c.run(monkeypatch)


# ---- the sizes of the left list and of the sets -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("k1,t1,k2,t2,ell", [(1, 1, 9, 2, 3), (64, 1, 6, 1, 5), (65, 1, 6, 2, 5), (11, 2, 9, 2, 5), (12, 2, 9, 1, 8),
                                             (9, 3, 8, 2, 6), (10, 4, 7, 1, 7), (7, 2, 10, 3, 6), (6, 1, 9, 4, 4), (9, 8, 10, 8, 3)])
def test_left_list_and_set_sizes(monkeypatch, k1, t1, k2, t2, ell):
    """N1 = 1, 64, 65 (t1 = 1), 55 and 66 (t1 = 2): the bucket bits go from 0 to 6 and 7; t1 = 3, 4 and 8, t2 = 3, 4 and 8: the bisection
    in the table of binomials on either side."""
    k, n, batch = k1 + k2, 70, 2
    win = [_window(n, ell, k1 + b) for b in range(batch)]
    c = Case(k, n, k1, t1, t2, _members(k, n, batch, 3 * k + t1, win), _words(n, batch, k, win), win, seed=k)
    assert all(c.collisions(b) > 0 for b in range(batch))
    c.run(monkeypatch)


def test_the_largest_left_list(monkeypatch):
    """N1 = C(128, 2) = 8128 against k2 = 24, t2 = 2 at ell = 10: 1024 threads, 1024 buckets of eight entries; the join weighs the
    expectation's 2200 collisions."""
    k1, k2, n, ell = 128, 24, 130, 10
    win = [_window(n, ell, 5)]
    c = Case(k1 + k2, n, k1, 2, 2, [_bits(k1 + k2, n, 11)], _words(n, 1, 12), win, seed=4)
    assert comb(k1, 2) == 8128 and 1000 < c.collisions(0) < 4000
    c.run(monkeypatch, forms=((True, True), (False, True)))


# ---- the window -------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n,ell", [(1, 1), (63, 1), (63, 63), (64, 63), (64, 64), (65, 64), (65, 3), (1024, 64), (1024, 7), (200, 1)])
def test_window_widths_and_places(monkeypatch, n, ell):
    """ell = 1, 63, 64 at n = 1, 63, 64, 65, 1024: columns in the first and the last word, column n - 1 and column 0 always among them,
    in no order; member 2's window names one column twice (and so one column less)."""
    k, k1, batch = 12, 6, 3
    win = []
    for b in range(batch):
        w = _window(n, ell, n + ell + b)
        w[b % ell] = n - 1
        if ell > 1:
            w[(b + 1) % ell] = 0
        win.append(w)
    if ell > 1:
        win[2][0] = win[2][ell - 1]
    c = Case(k, n, k1, 2, 2, _members(k, n, batch, n + ell, win), _words(n, batch, ell, win), win, layout="odd" if n % 2 else "even", seed=n)
    assert all(n - 1 in w and (ell == 1 or 0 in w or w is win[2]) for w in win) and all(c.collisions(b) > 0 for b in range(batch))
    assert ell == 1 or sorted(win[0]) != win[0]
    c.run(monkeypatch)


@pytest.mark.parametrize("form", ["shared", "per-member", "null", "null-all-columns"])
def test_shared_per_member_and_absent_windows(monkeypatch, form):
    k, k1, n, batch, ell = 14, 7, 40 if form == "null-all-columns" else 100, 3, 6
    if form == "null-all-columns":
        ell = n   # the columns 0 .. n-1: only the zero words collide
    win = {"shared": [_window(n, ell, 1)], "per-member": [_window(n, ell, 2 + b) for b in range(batch)]}.get(form, [list(range(ell))])
    G = _members(k, n, batch, 9, win * batch if form != "per-member" else win)
    c = Case(k, n, k1, 2, 2, G, _words(n, batch, 5, win * batch if form != "per-member" else win), None if form.startswith("null") else win, ell=ell,
             seed=len(form))
    assert (c.cols is None) == form.startswith("null") and (c.cols is None or (c.cols.bs == 0) == (form == "shared"))
    assert all(c.collisions(b) > 0 for b in range(batch))
    c.run(monkeypatch)


@pytest.mark.parametrize("n", [70, 64])
def test_refused_members_between_good_ones(monkeypatch, n):
    """Members 1 and 2 have a window entry of -1 and of n: every bin -1 and lightest -2, nothing else of them read or written; members 0
    and 3 are exact.  Further entries far outside in member 2."""
    k, k1, batch, ell = 12, 6, 4, 5
    win = [_window(n, ell, 20 + b) for b in range(batch)]
    win[1][3] = -1
    win[2][0], win[2][4] = n, 1 << 30
    c = Case(k, n, k1, 2, 2, _members(k, n, batch, 17, win), _words(n, batch, 3, win), win, seed=n)
    assert [f is None for f in c.found] == [False, True, True, False] and c.collisions(0) > 0 and c.collisions(3) > 0
    assert c.want_hist[n + 1:3 * (n + 1)].tolist() == [-1] * (2 * (n + 1)) and c.want_light(0)[1:3] == [-2, -2]
    c.run(monkeypatch)
    shared = Case(k, n, k1, 2, 2, _members(k, n, 2, 18), None, [[0, 1, n, 2]], seed=n + 1)     # one refused window for all members
    assert shared.found == [None, None]
    shared.run(monkeypatch, w_mins=(0,))


# ---- the comparison of the full key -----------------------------------------------------------------------------------------------------

def test_every_pair_in_one_bucket(monkeypatch):
    """The window columns are all zero in G and V: every pair collides, one bucket holds the whole left list of 66."""
    k, k1, n, batch, ell = 20, 12, 90, 2, 9
    win = [_window(n, ell, 31)]
    G = _members(k, n, batch, 23)
    for g in G:
        g[:, win[0]] = 0
    c = Case(k, n, k1, 2, 2, G, _words(n, batch, 7, win * batch), win, seed=8)
    assert all(c.collisions(b) == comb(k1, 2) * comb(k - k1, 2) for b in range(batch))
    c.run(monkeypatch)


def test_keys_that_differ_above_the_bucket_bits_only(monkeypatch):
    """N1 = 66: seven bucket bits.  The first seven window columns are zero in G and V, the other five random: all keys share bucket 0 and
    differ above it.  A kernel that trusts the bucket counts every pair; one pair in 32 collides."""
    k, k1, n, batch, ell = 20, 12, 90, 2, 12
    win = [_window(n, ell, 37)]
    G = _members(k, n, batch, 29)
    for g in G:
        g[:, win[0][:7]] = 0
    c = Case(k, n, k1, 2, 2, G, _words(n, batch, 9, win * batch), win, seed=9)
    pairs = comb(k1, 2) * comb(k - k1, 2)
    assert all(0 < c.collisions(b) < pairs // 8 for b in range(batch))
    c.run(monkeypatch)
    # and the other way round: the keys differ in the bucket bits only
    for g in G:
        g[:, win[0][7:]] = 0
        g[:, win[0][:7]] = _bits(k, 7, 41)
    c = Case(k, n, k1, 2, 2, G, _words(n, batch, 9, win * batch), win, seed=10)
    assert all(0 < c.collisions(b) < pairs // 8 for b in range(batch))
    c.run(monkeypatch)


def test_ties_take_the_smallest_pair_rank(monkeypatch):
    """[I | I | 0] with the window in the zero columns: every pair collides and weighs 2 (t1 + t2): lightest is pair rank 0; with window
    columns of rows 0, 1 (left) and 9 (right) added, the first free rows of each half."""
    k, z, k1 = 16, 5, 7
    G = cc.doubled_identity_zeros(k, z)
    n = 2 * k + z
    for t1, t2, win in [(2, 2, [2 * k + 4, 2 * k]), (2, 2, [2 * k + 1, 0, k + 1, 9]), (3, 1, [k + 9, 1, 0]), (1, 3, [2 * k + 2])]:
        c = Case(k, n, k1, t1, t2, [G], None, [win], seed=t1)
        for w_min in (0, 2 * (t1 + t2), 2 * (t1 + t2) + 1):
            want_h, want_l = cc.doubled_identity_expect(k, z, k1, t1, t2, win, w_min)
            assert np.array_equal(c.want_hist, want_h) and c.want_light(w_min) == [want_l]
        assert c.want_light(0)[0] & ((1 << 40) - 1) == (0 if len(win) < 3 else cc.pair_rank([2, 3, 4][:t1], [7, 8, 10][:t2], k1, k, t2))
        c.run(monkeypatch, w_mins=(0, 2 * (t1 + t2), 2 * (t1 + t2) + 1, n + 2))


# ---- the operands -----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("v_form", ["absent", "shared", "per-member", "shared-G"])
@pytest.mark.parametrize("layout", ["dense", "gaps"])
def test_operand_combinations(monkeypatch, v_form, layout):
    """V absent, shared, per member; one shared G with per-member V (the decoding of many received words); a w_min in the middle."""
    k, k1, n, batch, ell = 13, 6, 100, 4, 5
    win = [_window(n, ell, 3)]
    G = _members(k, n, 1 if v_form == "shared-G" else batch, 5, win * batch)
    V = {"absent": None, "shared": _words(n, 1, 1, win), "per-member": _words(n, batch, 2, win * batch), "shared-G": _words(n, batch, 3, win * batch)}[v_form]
    c = Case(k, n, k1, 2, 2, G, V, win, layout=layout, seed=len(v_form))
    assert c.batch == batch and (c.G.bs == 0) == (v_form == "shared-G") and (V is None or (c.V.bs == 0) == (v_form == "shared"))
    mid = int(np.median(c.found[0][0]))
    c.run(monkeypatch, w_mins=(0, 1, mid, n, n + 1, n + 2))


def test_bits_beyond_the_last_column_do_not_count(monkeypatch):
    """Every bit beyond column n set in G and V of members 1 and 2 (n = 90 leaves 38 of them per row)."""
    k, k1, n, ell = 10, 5, 90, 4
    win = [[89, 64, 3, 70]]
    zero = np.zeros((k, n), dtype=np.uint8)
    c = Case(k, n, k1, 2, 1, [zero, zero, _members(k, n, 1, 3, win)[0]], [np.zeros(n, dtype=np.uint8)] * 2 + _words(n, 1, 4, win), win, seed=6,
             tail_ones=(1, 2))
    assert c.want_hist[0] == c.want_hist[n + 1] == comb(k1, 2) * (k - k1)
    c.run(monkeypatch)


# ---- path 1 -----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k1,t1,k2,t2,batch,slices", [(4, 2, 40, 2, 2, 4), (30, 2, 60, 2, 1, 5), (3, 1, 24, 3, 3, 8)])
def test_slices_of_the_right_list(monkeypatch, k1, t1, k2, t2, batch, slices):
    """The right list in at least three slices with a ragged last one, of 256 sums or of N1: the outputs of path 1 are those of path 0
    byte for byte."""
    k, n, ell = k1 + k2, 75, 6
    n1, n2 = comb(k1, t1), comb(k2, t2)
    length = max(n1, 256)
    assert m4ri_amd.row_sums_collide_slices(k, n, k1, t1, t2, ell, batch) == slices == -(-n2 // length) >= 3 and n2 % length
    win = [_window(n, ell, 50 + b) for b in range(batch)]
    c = Case(k, n, k1, t1, t2, _members(k, n, batch, k, win, patterns=4), _words(n, batch, k1, win), win, seed=k2)
    r2 = [f[1] % n2 for f in c.found]
    assert all(len(set((r // length).tolist())) == slices for r in r2)          # collisions in every slice
    got = {}
    for path in (0, 1):
        _route(monkeypatch, path)
        outs = c.call(1)
        c.check(outs, 1)
        got[path] = [o.dev.cpu().numpy().tobytes() for o in outs]
    assert got[0] == got[1]
    c.run(monkeypatch)


def test_pair_ranks_at_a_distance(monkeypatch):
    """rowsums_cases.rigged(160, 17, 44, 159) with rows 17 and 44 on the left (k1 = 60), on the two columns row 159 took over: 8.7 * 10^6
    pairs by the closed form (which tests/test_row_sums_collide_plan.py holds to brute force), 8.1 * 10^6 of them collide, all in one
    bin; the lightest is the one pair with rows 17, 44 and 159."""
    k, (a, b, cc_), k1, t1, t2 = 160, (17, 44, 159), 60, 2, 2
    n = 2 * k
    G = Operand([rc.rigged(k, a, b, cc_)], k, n, "gaps", 3)
    win = Windows([cc.rigged_window(k, a, b)], 2, 4)
    assert m4ri_amd.row_sums_collide_slices(k, n, k1, t1, t2, 2, 1) == 3
    for path in (0, 1):
        _route(monkeypatch, path)
        for w_min in (0, 6, 9):
            want_h, want_l = cc.rigged_expect(k, a, b, cc_, k1, t1, t2, w_min)
            h, light = Out(np.int64, n + 1, 5), Out(np.int64, 1, 6)
            m4ri_amd.row_sums_collide_batch_dev(G.ptr, G.stride, 0, k, n, 0, 0, 1, k1, t1, t2, win.ptr, 0, 2, w_min, h.ptr, light.ptr)
            torch.cuda.synchronize()
            h.check(want_h, f"hist, path {path}")
            light.check([want_l], f"lightest at w_min = {w_min}, path {path}")
    want_h, want_l = cc.rigged_expect(k, a, b, cc_, k1, t1, t2, 0)
    assert want_h[8] == comb(58, 2) * comb(99, 2) > 1 << 22 and want_h[5] == 99 and want_l >> 40 == 5
    assert m4ri_amd.row_pair_unrank(want_l & ((1 << 40) - 1), k1, k, t1, t2) == ((17, 44), (60, 159))
    assert G.unchanged() and win.unchanged()


# ---- against the rest of the library ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k,t", [(10, 0), (10, 1), (10, 3), (40, 2), (5, 6)])
def test_without_window_and_right_half_it_is_row_sums_weights(monkeypatch, k, t):
    """ell = 0, t2 = 0, k1 = k: hist and lightest are those of m4ri_amd_row_sums_weights_batch_dev bit for bit."""
    n, batch = 100, 3
    g = Operand(_members(k, n, batch, 12), k, n, "gaps", 1)
    v = Operand([x[None, :] for x in _words(n, batch, 13)], 1, n, "gaps", 2)
    for w_min in (0, 1, n // 2):
        want = (Out(np.int64, batch * (n + 1), 3), Out(np.int64, batch, 4))
        m4ri_amd.row_sums_weights_batch_dev(g.ptr, g.stride, g.bs, k, n, v.ptr, v.bs, batch, t, w_min, want[0].ptr, want[1].ptr)
        for path in _paths(k, n, k, t, 0):
            _route(monkeypatch, path)
            got = (Out(np.int64, batch * (n + 1), 3), Out(np.int64, batch, 4))     # the same dirt: the whole arrays are compared
            m4ri_amd.row_sums_collide_batch_dev(g.ptr, g.stride, g.bs, k, n, v.ptr, v.bs, batch, k, t, 0, 0, 0, 0, w_min, got[0].ptr, got[1].ptr)
            torch.cuda.synchronize()
            for a, b in zip(want, got):
                assert a.dev.cpu().numpy().tobytes() == b.dev.cpu().numpy().tobytes(), (path, w_min)
    assert g.unchanged() and v.unchanged()


def _invertible(k, rng):
    lower, upper = np.tril(rng.integers(0, 2, size=(k, k)), -1) + np.eye(k, dtype=np.int64), np.triu(rng.integers(0, 2, size=(k, k)), 1) + np.eye(k, dtype=np.int64)
    return (lower @ upper % 2).astype(np.uint8)


def test_a_stern_iteration_end_to_end(monkeypatch):
    """A [96, 32] code, y = codeword ^ e with wt(e) = 6, three members with their own column orders, built so that two errors fall into
    the first 16 information columns, two into the last 16, none into the 12 window columns after them and two into the rest.
    m4ri_amd_echelonize_order_batch_dev (full = 1, y a follower row) makes G' and V = y ^ y_I G' in place; the collision step on
    cols = order + 32, t1 = t2 = 2 finds e: weight 6, and the pair's rows are the places of the four errors in the order."""
    k, n, batch, ell = 32, 96, 3, 12
    rng = np.random.default_rng(2024)
    stacked, orders, want_rows = [], [], []
    for b in range(batch):
        order = rng.permutation(n)
        systematic = np.zeros((k, n), dtype=np.uint8)
        systematic[:, order[:k]] = np.eye(k, dtype=np.uint8)
        systematic[:, order[k:]] = rng.integers(0, 2, size=(k, n - k), dtype=np.uint8)
        G = (_invertible(k, rng).astype(np.int64) @ systematic % 2).astype(np.uint8)     # the same code, no longer systematic
        places = sorted(rng.choice(16, 2, replace=False)) + sorted(16 + rng.choice(16, 2, replace=False)) + \
            sorted(k + ell + rng.choice(n - k - ell, 2, replace=False))
        e = np.zeros(n, dtype=np.uint8)
        e[order[places]] = 1
        y = (rng.integers(0, 2, size=k) @ G.astype(np.int64) % 2).astype(np.uint8) ^ e
        stacked.append(np.concatenate([G, y[None, :]]))
        orders.append(order.astype(np.int32))
        want_rows.append((tuple(places[:2]), tuple(places[2:4])))
    D = Operand(stacked, k + 1, n, "gaps", 5)
    o_bs = n + 4
    order_host = np.full(batch * o_bs, -9, dtype=np.int32)
    for b in range(batch):
        order_host[b * o_bs:b * o_bs + n] = orders[b]
    order_dev = torch.from_numpy(order_host.copy()).cuda()
    rank = torch.full((batch,), -7, dtype=torch.int32, device="cuda")
    m4ri_amd.echelonize_order_batch_dev(D.ptr, D.stride, D.bs, D.ptr, D.stride, D.bs, k + 1, n, k, order_dev.data_ptr(), o_bs, k, batch, 1, rank.data_ptr())
    for path in (0, 1):
        _route(monkeypatch, path)
        hist, light = Out(np.int64, batch * (n + 1), 6), Out(np.int64, batch, 7)
        m4ri_amd.row_sums_collide_batch_dev(D.ptr, D.stride, D.bs, k, n, D.ptr + 8 * k * D.stride, D.bs, batch, 16, 2, 2, order_dev.data_ptr() + 4 * k, o_bs,
                                            ell, 1, hist.ptr, light.ptr)
        torch.cuda.synchronize()
        assert rank.cpu().tolist() == [k] * batch
        got = light.dev.cpu().numpy()[FRAME:FRAME + batch].tolist()
        assert [x >> 40 for x in got] == [6] * batch, got
        assert [m4ri_amd.row_pair_unrank(x & ((1 << 40) - 1), 16, k, 2, 2) for x in got] == want_rows
        h = hist.dev.cpu().numpy()[FRAME:FRAME + batch * (n + 1)].reshape(batch, n + 1)
        assert (h[:, :6] == 0).all() and (h[:, 6] == 1).all() and (h >= 0).all()      # e is the one word below the code's distance
        assert np.array_equal(hist.dev.cpu().numpy()[:FRAME], hist.host[:FRAME]) and np.array_equal(light.dev.cpu().numpy()[-FRAME:], light.host[-FRAME:])
    assert np.array_equal(order_dev.cpu().numpy(), order_host)


# ---- streams and graphs -----------------------------------------------------------------------------------------------------------------

def test_on_a_side_stream_and_captured_into_a_graph(monkeypatch):
    """A capture of one call on path 0, one on path 1 (its initialisation kernel included) and one answered by the initialisation
    kernel alone: nothing runs while capturing (the outputs keep their dirt), then one replay on freshly dirtied outputs.  One stream, no
    parallel branches."""
    cases = []
    for path, (k, k1, t1, t2) in ((0, (12, 6, 2, 2)), (1, (44, 4, 2, 2)), (0, (12, 6, 7, 2))):
        win = [_window(100, 5, 60 + k + b) for b in range(3)]
        cases.append((path, Case(k, 100, k1, t1, t2, _members(k, 100, 3, 40 + k, win), _words(100, 3, path, win), win, seed=50 + k + t1)))
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
    g.replay()
    for (path, c), outs in zip(cases, held):
        c.check(outs, 1)
