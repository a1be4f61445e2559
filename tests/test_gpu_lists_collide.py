"""m4ri_amd_lists_collide_batch_dev and m4ri_amd_lists_words_batch_dev (include/m4ri_amd.h, lists_collide_batch.hip) against NumPy on
the unpacked bits (tests/lists_collide_cases.py: brute force where the lists are small, the sorted join where they are not), on both
paths, at the edges of a chunk of the left list and with the right list in slices.  C is the chunk m4ri_amd.lists_collide_units reports.
Every operand is dirty behind column n and in its padding; every output lies in a frame of sentinels that must come back unchanged, and
so must every operand.  Every comparison is exact."""
from math import comb

import numpy as np
import pytest
import torch

import lists_collide_cases as lc
import m4ri_amd

pytestmark = pytest.mark.gpu
SENT, FRAME = -7_777_777, 8
MASK = lc.RANK_MASK
C = m4ri_amd.lists_collide_units(1, 1, 1, 0, 1)[0]


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    assert m4ri_amd.lib().m4ri_amd_device_count() >= 1, "no HIP device visible: the gpu tests have nothing to run on"
    m4ri_amd.init(0)
    torch.cuda.set_device(0)


class Arr:
    """A device array with the host copy it was made from."""

    def __init__(self, host):
        self.host = np.ascontiguousarray(host)
        self.dev = torch.from_numpy(self.host.copy()).cuda()

    def ptr(self, off=0):
        return self.dev.data_ptr() + off * self.host.itemsize

    def get(self):
        return self.dev.cpu().numpy()

    def unchanged(self):
        return np.array_equal(self.get(), self.host)


class Out(Arr):
    """`size` entries between two frames of sentinels, sentinels themselves before the call."""

    def __init__(self, size, dtype=np.int64):
        super().__init__(np.full(size + 2 * FRAME, SENT, dtype=dtype))
        self.size = size

    @property
    def p(self):
        return self.ptr(FRAME)

    def body(self):
        got = self.get()
        assert (got[:FRAME] == SENT).all() and (got[FRAME + self.size:] == SENT).all(), "written outside the output"
        return got[FRAME:FRAME + self.size]


class Lists:
    """The members of a list operand, packed: `mats` one bit matrix per member, or ONE for a shared operand (batch stride 0)."""

    def __init__(self, mats, n, pad, rng):
        self.shared = len(mats) == 1
        rows = mats[0].shape[0]
        self.stride = lc.width(n) + pad
        self.bs = 0 if self.shared else (rows + 1) * self.stride + 3
        host = rng.integers(-(1 << 62), 1 << 62, size=max((len(mats) - 1) * self.bs + (rows + 1) * self.stride, 1), dtype=np.int64)
        for b, m in enumerate(mats):
            if rows:
                host[b * self.bs:b * self.bs + rows * self.stride] = lc.pack(m, self.stride, rng).ravel()
        self.arr = Arr(host)


def _band(want):
    """A weight band from the reference's own collisions: from the lightest weight to the median one."""
    ws = np.sort(np.concatenate([k >> 40 for _, _, k, _ in want if len(k)]))
    return int(ws[0]), int(ws[len(ws) // 2])


class Join:
    """One call's operands.  X, Y: lists of bit matrices (one: shared); V: None, or a list of words (one: shared); cols: None (NULL), one
    window (shared) or one per member."""

    def __init__(self, X, Y, V, cols, n, batch, seed=0, pad=1):
        rng = np.random.default_rng(1000 + seed)
        self.n, self.batch, self.Xb, self.Yb, self.Vb, self.colsb = n, batch, X, Y, V, cols
        self.nx, self.ny = X[0].shape[0], Y[0].shape[0]
        self.X, self.Y = Lists(X, n, pad, rng), Lists(Y, n, pad + 1, rng)
        self.V = None if V is None else Lists([v[None, :] for v in V], n, 0, rng)
        if cols is None:
            self.cols, self.ell, self.c_bs = None, 0, 0
        else:
            per = cols if cols and isinstance(cols[0], (list, tuple)) else [cols]
            self.ell = len(per[0])
            self.c_bs = 0 if len(per) == 1 else self.ell + 1
            host = np.full(max((len(per) - 1) * self.c_bs + self.ell, 1), 12345, dtype=np.int32)
            for b, c in enumerate(per):
                host[b * self.c_bs:b * self.c_bs + self.ell] = c
            self.cols = Arr(host)

    def member(self, b):
        pick = lambda xs: None if xs is None else xs[b if len(xs) > 1 else 0]
        cols = self.colsb if not self.colsb or not isinstance(self.colsb[0], (list, tuple)) else pick(self.colsb)
        return pick(self.Xb), pick(self.Yb), pick(self.Vb), (list(range(self.first_ell)) if cols is None else cols)

    first_ell = 0    # with cols = None: the window is the columns 0 .. first_ell-1

    def expect(self, w_min, w_max, rule=lc.join):
        return [lc.expect(*self.member(b), w_min, w_max, rule) for b in range(self.batch)]

    def call(self, w_min, w_max, cap, l_bs=None, outs="hlc", null_list=False, stream=0, held=None, x_ptr=None, y_ptr=None):
        l_bs = cap + 2 if l_bs is None else l_bs
        o = held or (Out(self.batch * (self.n + 1)), Out(self.batch), Out(max((self.batch - 1) * l_bs + cap, 0)), Out(self.batch))
        ell = self.first_ell if self.cols is None else self.ell
        m4ri_amd.lists_collide_batch_dev(x_ptr or self.X.arr.ptr(), self.X.stride, self.X.bs, self.nx, y_ptr or self.Y.arr.ptr(), self.Y.stride, self.Y.bs,
                                         self.ny, self.n, self.V.arr.ptr() if self.V else 0, self.V.bs if self.V else 0, self.batch,
                                         self.cols.ptr() if self.cols else 0, self.c_bs, ell, w_min, w_max, o[0].p if "h" in outs else 0,
                                         o[1].p if "l" in outs else 0, o[2].p if "c" in outs and not null_list else 0, l_bs, cap, o[3].p if "c" in outs else 0,
                                         stream=stream)
        return o

    def check(self, o, want, cap, l_bs=None, outs="hlc", null_list=False):
        torch.cuda.synchronize()
        l_bs = cap + 2 if l_bs is None else l_bs
        h, l, lst, cnt = (x.body() for x in o)
        if "h" in outs:
            assert np.array_equal(h, np.concatenate([w[0] for w in want])), "hist"
        else:
            assert (h == SENT).all()
        if "l" in outs:
            assert l.tolist() == [w[1] for w in want], "lightest"
        else:
            assert (l == SENT).all()
        if "c" not in outs:
            assert (lst == SENT).all() and (cnt == SENT).all()
        else:
            assert cnt.tolist() == [w[3] for w in want], "count"
            for b, (_, _, keys, m) in enumerate(want):
                m = 0 if null_list else min(max(m, 0), cap)
                got, rest = lst[b * l_bs:b * l_bs + m], lst[b * l_bs + m:(b * l_bs + cap) if b == self.batch - 1 else (b + 1) * l_bs]
                assert (rest == SENT).all(), f"member {b}: an entry behind min(count, cap) was written"
                if len(keys) <= cap:
                    assert np.array_equal(np.sort(got), keys), f"member {b}: the list is not the qualifying set"
                else:
                    assert len(set(got.tolist())) == m and set(got.tolist()) <= set(keys.tolist()), f"member {b}: {m} of {len(keys)}"
        for a in (self.X.arr, self.Y.arr) + ((self.V.arr,) if self.V else ()) + ((self.cols,) if self.cols else ()):
            assert a.unchanged(), "a read-only operand changed"


def _bits(rows, n, seed):
    return np.random.default_rng(seed).integers(0, 2, (rows, n), dtype=np.uint8)


def _window(n, ell, seed):
    """ell columns: one from every word first, the rest anywhere, one entry repeated, unsorted."""
    rng = np.random.default_rng(seed)
    cols = [int(64 * w + rng.integers(0, min(64, n - 64 * w))) for w in range(lc.width(n))][:ell]
    cols += [int(c) for c in rng.integers(0, n, ell - len(cols))]
    if ell >= 2:
        cols[-1] = cols[0]
    return [cols[i] for i in rng.permutation(ell)]


def _plant(X, Y, V, cols, i, j, flips=2):
    """Y[j] <- V ^ X[i] with up to `flips` bits flipped outside the window: the pair (i, j) collides, at that weight."""
    v = np.zeros(X.shape[1], dtype=np.uint8) if V is None else V
    Y[j] = X[i] ^ v
    free = [c for c in range(X.shape[1]) if c not in set(cols)]
    for c in free[:flips]:
        Y[j, c] ^= 1


def _assert_something(want):
    """On the NumPy side alone: some pair collides and some pair lies in the band, in some good member."""
    assert any(w[3] > 0 for w in want) and any(w[0].sum() > 0 for w in want if w[3] >= 0)


# ---- path 0 against brute force -------------------------------------------------------------------------------------------------------

P0 = [  # nx, ny, n, ell (None: cols NULL), ell of a NULL window, batch, V ("none", "shared", "each"), shared ("", "X", "Y", "same")
    (1, 1, 1, 1, 0, 1, "none", ""), (2, 64, 63, 7, 0, 5, "each", ""), (63, 257, 64, 0, 0, 1, "shared", ""), (64, 1, 65, 33, 0, 5, "each", "X"),
    (65, 64, 130, 64, 0, 1, "each", ""), (300, 257, 1024, 7, 0, 1, "none", ""), (300, 257, 130, 7, 0, 5, "shared", "Y"), (300, 64, 63, 1, 0, 1, "each", ""),
    (64, 64, 130, 7, 0, 5, "each", "same"), (65, 65, 64, 1, 0, 1, "none", "same"), (63, 64, 1024, 33, 0, 1, "shared", ""), (2, 257, 1, 0, 0, 5, "none", ""),
    (300, 257, 130, None, 7, 5, "each", ""), (65, 257, 64, None, 64, 1, "shared", ""), (64, 64, 65, None, 33, 1, "none", ""), (63, 1, 63, None, 1, 5, "each", "X"),
    (300, 64, 1024, None, 0, 1, "each", ""), (1, 257, 130, 64, 0, 5, "shared", ""),
]


@pytest.mark.parametrize("nx,ny,n,ell,first,batch,vmode,shared", P0, ids=[f"{a}x{b}-n{c}-ell{d}-first{e}-b{f}-V{g}-{h or 'own'}" for a, b, c, d, e, f, g, h in P0])
def test_path0_against_brute_force(nx, ny, n, ell, first, batch, vmode, shared):
    seed = nx * 7 + ny * 3 + n
    assert m4ri_amd.plan_lists_collide_batch(nx, ny, n, first if ell is None else ell, batch) == 0
    cols = None if ell is None else _window(n, ell, seed)
    win = list(range(first)) if ell is None else cols
    V = None if vmode == "none" else [_bits(1, n, seed + 50 + b)[0] for b in range(1 if vmode == "shared" else batch)]
    X = [_bits(nx, n, seed + 100 + b) for b in range(1 if shared in ("X", "same") else batch)]
    Y = [x.copy() for x in X] if shared == "same" else [_bits(ny, n, seed + 200 + b) for b in range(1 if shared == "Y" else batch)]
    if shared != "same":
        for b in range(batch):          # a collision in every member, whatever ell is
            _plant(X[b % len(X)], Y[b % len(Y)], None if V is None else V[b % len(V)], win, (b * 5) % nx, (b * 11) % ny)
        if nx > 3 and len(X) == batch:
            for x in X:
                x[nx - 1] = x[1]        # a repeated row
    j = Join(X, Y, V, cols, n, batch, seed, pad=2)
    j.first_ell = first
    want0 = j.expect(0, n, lc.brute)
    _assert_something(want0)
    w_min, w_max = _band(want0)
    want = j.expect(w_min, w_max, lc.brute)
    _assert_something(want)
    cap = max(w[3] for w in want) + 3
    same = dict(y_ptr=j.X.arr.ptr()) if shared == "same" else {}
    if shared == "same":
        j.Y = j.X                       # X == Y: one memory
    j.check(j.call(w_min, w_max, cap, **same), want, cap)
    j.check(j.call(0, n + 5, 0, null_list=True, **same), want0, 0, null_list=True)      # w_max above n, a filtered count


# ---- chunk edges ------------------------------------------------------------------------------------------------------------------------

_edge_memo = {}


def _edge_case(nx, ell):
    """ny = 700, n = 130; planted: rows `e - 1` and `e` of X identical (e = C where there is a second chunk) and colliding with Y[3]; Y[5]
    colliding with row 7 of every chunk; 200 identical rows in chunk 0 colliding with Y[9]; X[400] and X[401] differing only in the highest
    window bit, X[402] and X[403] only in the lowest, Y[11] colliding with X[400] and Y[12] with X[402]."""
    if (nx, ell) not in _edge_memo:
        n, ny = 130, 700
        X, Y, V = _bits(nx, n, nx + ell), _bits(ny, n, nx + ell + 1), _bits(1, n, nx + ell + 2)[0]
        cols = _window(n, ell, nx)
        e = C if nx > C else nx - 1
        X[e - 1] = X[e]
        _plant(X, Y, V, cols, e, 3)
        for ch in range(-(-nx // C)):
            if ch * C + 7 < nx:
                X[ch * C + 7, cols] = (Y[5] ^ V)[cols]
        X[100:300] = X[100]
        _plant(X, Y, V, cols, 100, 9, flips=4)
        uniq = [c for c in cols if cols.count(c) == 1]      # the window's repeated entry ties two key bits together: not those
        hi, lo = uniq[-1], uniq[0]                          # the highest free key bit (above the bucket bits where ell > log2 C) and the lowest
        X[401] = X[400]
        X[401, hi] ^= 1
        X[403] = X[402]
        X[403, lo] ^= 1
        _plant(X, Y, V, cols, 400, 11)
        _plant(X, Y, V, cols, 402, 12, flips=3)
        j = Join([X], [Y], [V], cols, n, 1, nx)
        _edge_memo[(nx, ell)] = (j, j.expect(0, n), e)
    return _edge_memo[(nx, ell)]


@pytest.mark.parametrize("nx,ell,chunks", [(C - 1, 10, 1), (C, 10, 1), (C + 1, 10, 2), (2 * C, 10, 2), (2 * C + 1, 10, 3), (3 * C + 5, 10, 4), (C + 1, 16, 2)],
                         ids=["C-1", "C", "C+1", "2C", "2C+1", "3C+5", "C+1-ell16"])
def test_chunk_edges(nx, ell, chunks):
    j, want0, e = _edge_case(nx, ell)
    assert m4ri_amd.lists_collide_units(nx, 700, 130, ell, 1) == (C, chunks, 1)
    assert m4ri_amd.plan_lists_collide_batch(nx, 700, 130, ell, 1) == (0 if chunks == 1 else 1)
    ranks = set((want0[0][2] & MASK).tolist())
    assert {(e - 1) * 700 + 3, e * 700 + 3, 400 * 700 + 11, 402 * 700 + 12} <= ranks and not {401 * 700 + 11, 403 * 700 + 12} & ranks
    assert all((ch * C + 7) * 700 + 5 in ranks for ch in range(chunks) if ch * C + 7 < nx) and all(r * 700 + 9 in ranks for r in range(100, 300))
    assert len(ranks) >= 50
    _assert_something(want0)
    cap = want0[0][3] + 5
    j.check(j.call(0, 130, cap), want0, cap)
    w_min, w_max = _band(want0)
    want = j.expect(w_min, w_max)
    _assert_something(want)
    j.check(j.call(w_min, w_max, want[0][3]), want, want[0][3])


def test_chunks_times_slices():
    nx, ny, n, ell = 2 * C + 1, 300_000, 64, 24
    c, chunks, slices = m4ri_amd.lists_collide_units(nx, ny, n, ell, 1)
    assert chunks == 3 and slices >= 3 and nx * ny < 5 * 10**9 and m4ri_amd.plan_lists_collide_batch(nx, ny, n, ell, 1) == 1
    X, Y, V = _bits(nx, n, 1), _bits(ny, n, 2), _bits(1, n, 3)[0]
    cols = [int(c) for c in np.random.default_rng(4).permutation(n)[:ell]]
    _plant(X, Y, V, cols, nx - 1, ny - 1)
    _plant(X, Y, V, cols, C, 0)
    j = Join([X], [Y], [V], cols, n, 1, 5)
    want = j.expect(0, n)
    assert want[0][3] >= 50
    w_min, w_max = _band(want)
    want = j.expect(w_min, w_max)
    _assert_something(want)
    cap = want[0][3]
    j.check(j.call(w_min, w_max, cap), want, cap)


# ---- the list ---------------------------------------------------------------------------------------------------------------------------

def _list_case(path):
    if path == 0:
        n, cols = 130, _window(130, 7, 77)
        X, Y, V = _bits(300, n, 70), _bits(257, n, 71), _bits(1, n, 72)[0]
        _plant(X, Y, V, cols, 5, 6)
        key = ("list", 0)
        if key not in _edge_memo:
            j = Join([X], [Y], [V], cols, n, 1, 73)
            _edge_memo[key] = (j, j.expect(0, n), 0)
        return _edge_memo[key][:2]
    return _edge_case(C + 1, 10)[:2]


@pytest.mark.parametrize("path", [0, 1])
def test_the_cap(path):
    j, want0 = _list_case(path)
    assert m4ri_amd.plan_lists_collide_batch(j.nx, j.ny, j.n, j.ell, 1) == path
    w_min, w_max = _band(want0)
    want = j.expect(w_min, w_max)
    count = want[0][3]
    assert count >= 3
    for cap, null in ((0, True), (0, False), (1, False), (count - 1, False), (count, False), (count + 7, False)):
        j.check(j.call(w_min, w_max, cap, null_list=null), want, cap, null_list=null)


@pytest.mark.parametrize("path", [0, 1])
def test_the_band_and_the_outputs(path):
    j, want0 = _list_case(path)
    ws = np.flatnonzero(want0[0][0])
    lo, hi = int(ws[0]), int(ws[-1])
    for w_min, w_max in ((lo, lo), (hi, hi), (lo, hi), (lo + 1, hi - 1), (hi + 1, j.n), (hi, lo), (0, j.n + 1000), (j.n + 1, j.n + 2)):
        want = j.expect(w_min, w_max)
        cap = want[0][3] + 1
        j.check(j.call(w_min, w_max, cap), want, cap)
    want = j.expect(lo, hi)
    assert want[0][3] == want0[0][3] > 0
    for outs in ("h", "l", "c", "hl", "hc", "lc", "hlc"):
        j.check(j.call(lo, hi, want[0][3], outs=outs), want, want[0][3], outs=outs)


# ---- refused and degenerate members -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("nx", [65, C + 1], ids=["path0", "path1"])
def test_refused_members_among_good_ones(nx):
    n, ny, ell, batch = 130, 300, 8, 4
    assert m4ri_amd.plan_lists_collide_batch(nx, ny, n, ell, batch) == (0 if nx <= C else 1)
    wins = [_window(n, ell, 10 + b) for b in range(batch)]
    wins[1][3], wins[2][ell - 1] = -1, n
    X, Y = [_bits(nx, n, 20)], [_bits(ny, n, 30 + b) for b in range(batch)]
    V = [_bits(1, n, 40 + b)[0] for b in range(batch)]
    for b in (0, 3):
        _plant(X[0], Y[b], V[b], wins[b], b, b + 1)
    j = Join(X, Y, V, wins, n, batch, 50)
    want = j.expect(0, n, lc.brute if nx < 100 else lc.join)
    assert [w[3] for w in want][1:3] == [-1, -1] and want[0][3] > 0 and want[3][3] > 0 and want[1][1] == -2 and (want[2][0] == -1).all()
    cap = max(w[3] for w in want) + 2
    j.check(j.call(0, n, cap), want, cap)
    for outs in ("h", "l", "c"):
        j.check(j.call(0, n, cap, outs=outs), want, cap, outs=outs)


def test_degenerate_members():
    n = 70
    for nx, ny in ((0, 5), (5, 0), (0, 0)):
        j = Join([_bits(nx, n, 1)] * 3, [_bits(ny, n, 2)] * 3, None, _window(n, 4, 3), n, 3)
        want = [(np.zeros(n + 1, dtype=np.int64), -1, np.zeros(0, dtype=np.int64), 0)] * 3
        j.check(j.call(0, n, 4), want, 4)
    j = Join([_bits(0, n, 1)] * 3, [_bits(5, n, 2)] * 3, None, [[1, 2], [1, n], [3, 4]], n, 3)           # a refused member is refused without pairs too
    zero = (np.zeros(n + 1, dtype=np.int64), -1, np.zeros(0, dtype=np.int64), 0)
    j.check(j.call(0, n, 4), [zero, (np.full(n + 1, -1, dtype=np.int64), -2, np.zeros(0, dtype=np.int64), -1), zero], 4)
    # n = 0 with ell = 0: all nx * ny pairs weigh 0
    j = Join([np.zeros((6, 0), dtype=np.uint8)] * 2, [np.zeros((7, 0), dtype=np.uint8)] * 2, None, None, 0, 2)
    j.check(j.call(0, 5, 50), [(np.array([42], dtype=np.int64), 0, np.arange(42, dtype=np.int64), 42)] * 2, 50)
    j.check(j.call(0, 5, 10), [(np.array([42], dtype=np.int64), 0, np.arange(42, dtype=np.int64), 42)] * 2, 10)
    j.check(j.call(1, 5, 10), [(np.array([42], dtype=np.int64), -1, np.zeros(0, dtype=np.int64), 0)] * 2, 10)
    # batch = 0 touches nothing
    j = Join([_bits(5, n, 1)], [_bits(5, n, 2)], None, [1, 2], n, 1)
    o = j.call(0, n, 4)
    held = (Out(n + 1), Out(1), Out(4), Out(1))
    j.batch = 0
    j.call(0, n, 4, held=held)
    torch.cuda.synchronize()
    assert all((x.get() == SENT).all() for x in held) and j.X.arr.unchanged() and j.Y.arr.unchanged()


# ---- against the existing calls, bit for bit ------------------------------------------------------------------------------------------

def _old_list(G, stride, k, n, k1, t1, t2, cols, ell, cap):
    o = (Out(n + 1), Out(1), Out(cap), Out(1))
    m4ri_amd.row_sums_collide_list_batch_dev(G, stride, 0, k, n, 0, 0, 1, k1, t1, t2, cols, 0, ell, 1, n, o[0].p, o[1].p, o[2].p, cap, cap, o[3].p)
    torch.cuda.synchronize()
    return o


def _same(a, b):
    ha, la, ka, ca = (x.body() for x in a)
    hb, lb, kb, cb = (x.body() for x in b)
    m = int(ca[0])
    assert m > 0 and np.array_equal(ha, hb) and np.array_equal(la, lb) and np.array_equal(ca, cb) and np.array_equal(np.sort(ka[:m]), np.sort(kb[:m]))
    assert ha.sum() > 0


def test_the_two_halves_of_a_generator():
    """X = the first k1 rows, Y = the other rows of one generator: the call with t1 = t2 = 1 gives the same, bit for bit."""
    k, k1, n, ell, cap = 300, 120, 200, 6, 2000
    rng = np.random.default_rng(8)
    G = Arr(lc.pack(_bits(k, n, 80), 5, rng).ravel())
    cols = Arr(np.array(_window(n, ell, 81), dtype=np.int32))
    old = _old_list(G.ptr(), 5, k, n, k1, 1, 1, cols.ptr(), ell, cap)
    new = (Out(n + 1), Out(1), Out(cap), Out(1))
    m4ri_amd.lists_collide_batch_dev(G.ptr(), 5, 0, k1, G.ptr(5 * k1), 5, 0, k - k1, n, 0, 0, 1, cols.ptr(), 0, ell, 1, n, new[0].p, new[1].p, new[2].p, cap, cap,
                                     new[3].p)
    torch.cuda.synchronize()
    _same(old, new)
    assert 50 <= int(new[3].body()[0]) <= cap and G.unchanged()


def test_materialised_row_sums():
    """k1 = k2 = 20, t1 = t2 = 2: both halves written out by row_sums_words_batch_dev from an iota of keys (the list index is then the
    colexicographic rank), joined, against row_sums_collide_list_batch_dev on the generator."""
    k1, n, ell, cap, N = 20, 100, 5, 3000, 190
    rng = np.random.default_rng(9)
    G = Arr(lc.pack(_bits(2 * k1, n, 90), 3, rng).ravel())
    cols = Arr(np.array(_window(n, ell, 91), dtype=np.int32))
    iota = Arr(np.arange(N, dtype=np.int64))
    halves = [Arr(rng.integers(-(1 << 62), 1 << 62, size=N * 3, dtype=np.int64)) for _ in range(2)]
    for h, off in zip(halves, (0, 3 * k1)):
        m4ri_amd.row_sums_words_batch_dev(G.ptr(off), 3, 0, k1, n, 0, 0, 1, k1, 2, 0, iota.ptr(), N, N, 0, h.ptr(), 3, 0)
    old = _old_list(G.ptr(), 3, 2 * k1, n, k1, 2, 2, cols.ptr(), ell, cap)
    new = (Out(n + 1), Out(1), Out(cap), Out(1))
    m4ri_amd.lists_collide_batch_dev(halves[0].ptr(), 3, 0, N, halves[1].ptr(), 3, 0, N, n, 0, 0, 1, cols.ptr(), 0, ell, 1, n, new[0].p, new[1].p, new[2].p, cap, cap,
                                     new[3].p)
    torch.cuda.synchronize()
    _same(old, new)
    assert 50 <= int(new[3].body()[0]) <= cap


def _pair_sums(A):
    """The sums of two rows of A in colexicographic order of {i < j}: rank C(j, 2) + i."""
    return np.array([A[i] ^ A[j] for j in range(A.shape[0]) for i in range(j)], dtype=np.uint8).reshape(-1, A.shape[1])


def _join_threads(left, left_256, slice_len):
    """join_threads of join_common.h: 256 threads where they hold the left table and the slice is short."""
    return 256 if left <= left_256 and slice_len <= 4096 else 1024


SCAN_EDGES = [  # k1 = k2, N per side, ell, threads of both kernels, buckets
    (2, 1, 0, 256, 1),           # one entry, one bucket: every thread but one idle in the scan
    (20, 190, 0, 256, 1),        # one bucket, every pair a match: all 32-bit bins and the LDS slot counter in use
    (20, 190, 5, 256, 32),       # fewer buckets than threads
    (65, 2080, 5, 1024, 32),     # 1024 threads in both kernels, fewer buckets than threads
    (65, 2080, 13, 1024, 4096),  # q held at ceil(log2 2080) = 12 below ell: four buckets per thread
]


@pytest.mark.parametrize("k1,N,ell,threads,nb", SCAN_EDGES, ids=[f"k{a}-N{b}-ell{c}" for a, b, c, _, _ in SCAN_EDGES])
def test_both_joins_on_the_scan_edges(k1, N, ell, threads, nb):
    """The join of the row sums (t1 = t2 = 2) and the join of the two materialised lists share the table's scan, the match report and
    the output step (join_common.h), so agreeing with each other proves little: each is judged against the NumPy rule on the materialised
    lists, at the shapes on the edges of the scan.  Both halves are written out by row_sums_words_batch_dev from an iota of keys."""
    n, stride, seed = 100, 3, 7 * k1 + ell
    assert N == comb(k1, 2) and m4ri_amd.plan_row_sums_collide_batch(2 * k1, n, k1, 2, 2, ell) == 0
    assert m4ri_amd.lists_collide_units(N, N, n, ell, 1) == (C, 1, 1) and N <= C         # path 0 in both: the slice is the whole right list
    assert _join_threads(N, 1024, N) == threads and _join_threads(N, 8 * 256, N) == threads   # rc_kernel: N1 <= 1024; lc_kernel: 8 keys per thread
    assert 1 << min(ell, (N - 1).bit_length()) == nb
    rng = np.random.default_rng(seed)
    Gb = _bits(2 * k1, n, 300 + seed)
    G = Arr(lc.pack(Gb, stride, rng).ravel())
    window = _window(n, ell, 400 + seed)
    cols = Arr(np.array(window + [12345], dtype=np.int32))
    X, Y = _pair_sums(Gb[:k1]), _pair_sums(Gb[k1:])
    hist, lightest, keys, count = lc.expect(X, Y, None, window, 0, n, lc.join)
    assert count >= 1 and (ell > 0 or count == N * N)
    cap = count + 7
    iota = Arr(np.arange(N, dtype=np.int64))
    halves = [Arr(rng.integers(-(1 << 62), 1 << 62, size=N * stride, dtype=np.int64)) for _ in range(2)]
    for h, off, want in zip(halves, (0, stride * k1), (X, Y)):
        m4ri_amd.row_sums_words_batch_dev(G.ptr(off), stride, 0, k1, n, 0, 0, 1, k1, 2, 0, iota.ptr(), N, N, 0, h.ptr(), stride, 0)
        torch.cuda.synchronize()
        assert np.array_equal(lc.unpack(h.get().reshape(N, stride), n), want), "the materialised list"
    sums, lists = (Out(n + 1), Out(1), Out(cap), Out(1)), (Out(n + 1), Out(1), Out(cap), Out(1))
    m4ri_amd.row_sums_collide_list_batch_dev(G.ptr(), stride, 0, 2 * k1, n, 0, 0, 1, k1, 2, 2, cols.ptr(), 0, ell, 0, n, sums[0].p, sums[1].p, sums[2].p, cap, cap,
                                             sums[3].p)
    m4ri_amd.lists_collide_batch_dev(halves[0].ptr(), stride, 0, N, halves[1].ptr(), stride, 0, N, n, 0, 0, 1, cols.ptr(), 0, ell, 0, n, lists[0].p, lists[1].p,
                                     lists[2].p, cap, cap, lists[3].p)
    torch.cuda.synchronize()
    for name, o in (("row sums", sums), ("lists", lists)):
        h, l, lst, cnt = (x.body() for x in o)
        assert np.array_equal(h, hist), name
        assert l.tolist() == [lightest] and cnt.tolist() == [count], name
        assert np.array_equal(np.sort(lst[:count]), keys) and (lst[count:] == SENT).all(), name
    assert G.unchanged() and cols.unchanged()


# ---- the words --------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [1, 64, 65, 130, 1024])
@pytest.mark.parametrize("null_count", [False, True])
def test_the_words(n, null_count):
    nx, ny, batch, cap = 37, 29, 4, 300
    rng = np.random.default_rng(n)
    X, Y = [_bits(nx, n, 60 + b) for b in range(batch)], [_bits(ny, n, 61)]           # Y shared
    V = [_bits(1, n, 62 + b)[0] for b in range(batch)]
    j = Join(X, Y, V, None, n, batch, n, pad=1)
    counts = [cap, 150, cap + 50, -1] if not null_count else [cap] * batch                  # at cap, below, above, refused
    ranks = rng.integers(0, nx * ny, size=(batch, cap))
    ranks[:, 0], ranks[:, 1] = 0, nx * ny - 1
    keys = ranks | (rng.integers(0, 1 << 11, size=(batch, cap)) << 40)                     # weight bits: ignored
    bad = {(0, 5): -1, (0, 260): nx * ny, (1, 7): (3 << 40) | (nx * ny + 5), (1, 200): -1, (2, 299): -(1 << 40), (3, 0): -1}
    for (b, i), key in bad.items():
        keys[b, i] = key
    l_bs, w_stride = cap + 3, lc.width(n) + 1
    w_bs = cap * w_stride + 5
    K, Cn = Arr(np.pad(keys, ((0, 0), (0, 3)), constant_values=-1).ravel()), Arr(np.array(counts, dtype=np.int64))
    W, S = Arr(rng.integers(-(1 << 62), 1 << 62, size=batch * w_bs + 9, dtype=np.int64)), Out(batch, np.int32)
    m4ri_amd.lists_words_batch_dev(j.X.arr.ptr(), j.X.stride, j.X.bs, nx, j.Y.arr.ptr(), j.Y.stride, 0, ny, n, j.V.arr.ptr(), j.V.bs, batch, K.ptr(), l_bs, cap,
                                   0 if null_count else Cn.ptr(), W.ptr(), w_stride, w_bs, S.p)
    torch.cuda.synchronize()
    exp, skipped = W.host.copy().view(np.uint64), [0] * batch
    valid = lc.pack(np.ones((1, n), dtype=np.uint8))[0].view(np.uint64)
    for b in range(batch):
        for i in range(min(max(counts[b], 0), cap)):
            if (b, i) in bad:
                skipped[b] += 1
                continue
            at = b * w_bs + i * w_stride
            word = lc.pack(lc.words_of(X[b], Y[0], V[b], [ranks[b, i]]))[0].view(np.uint64)
            exp[at:at + lc.width(n)] = (exp[at:at + lc.width(n)] & ~valid) | word
    got = W.get().view(np.uint64)
    assert np.array_equal(got, exp), f"{np.count_nonzero(got != exp)} words of W differ, the first at {np.flatnonzero(got != exp)[:4]}"
    assert S.body().tolist() == skipped and sum(skipped) >= (3 if null_count else 2)
    assert K.unchanged() and Cn.unchanged() and j.X.arr.unchanged() and j.Y.arr.unchanged() and j.V.arr.unchanged()


# ---- two levels end to end: Wagner's four lists --------------------------------------------------------------------------------------------

def test_two_levels_end_to_end():
    """x1 ^ x2 ^ x3 ^ x4 = V over four lists of 2000 random 64-bit rows with one planted solution: (L1, L2) and (L3, L4 with V) joined on
    11 columns, both results written out as words, those joined on the other 53 columns at weight 0.  Five calls, nothing copied to the
    host in between (the caps are the NumPy counts); the host then follows the keys back through both levels."""
    N, n = 2000, 64
    rng = np.random.default_rng(2024)
    L = [_bits(N, n, 500 + i) for i in range(4)]
    V = _bits(1, n, 504)[0]
    perm = [int(c) for c in rng.permutation(n)]
    A, B = perm[:11], perm[11:]
    a = [17, 1999, 0, 1234]
    d = _bits(1, n, 505)[0]
    d[A] = 0
    L[1][a[1]] = L[0][a[0]] ^ d
    L[3][a[3]] = V ^ L[2][a[2]] ^ d
    w1, r1 = lc.join(L[0], L[1], None, A)
    w2, r2 = lc.join(L[2], L[3], V, A)
    cap1, cap2 = len(r1), len(r2)
    assert cap1 >= 50 and cap2 >= 50 and a[0] * N + a[1] in r1 and a[2] * N + a[3] in r2
    W1b, W2b = lc.words_of(L[0], L[1], None, np.sort(r1)), lc.words_of(L[2], L[3], V, np.sort(r2))
    w3, r3 = lc.join(W1b, W2b, None, B)
    assert len(r3) == 1 and w3[0] == 0                                  # NumPy side: exactly one pair of the second level, at weight 0
    dev = [Arr(lc.pack(x, 2, rng).ravel()) for x in L]
    Vd, Ad, Bd = Arr(lc.pack(V[None, :], 1, None).ravel()), Arr(np.array(A, dtype=np.int32)), Arr(np.array(B, dtype=np.int32))

    def five(st, K1, N1, K2, N2, W1, W2, K3, N3):
        J, Wd = m4ri_amd.lists_collide_batch_dev, m4ri_amd.lists_words_batch_dev
        J(dev[0].ptr(), 2, 0, N, dev[1].ptr(), 2, 0, N, n, 0, 0, 1, Ad.ptr(), 0, 11, 0, n, list=K1.p, l_bs=cap1, cap=cap1, count=N1.p, stream=st)
        J(dev[2].ptr(), 2, 0, N, dev[3].ptr(), 2, 0, N, n, Vd.ptr(), 0, 1, Ad.ptr(), 0, 11, 0, n, list=K2.p, l_bs=cap2, cap=cap2, count=N2.p, stream=st)
        Wd(dev[0].ptr(), 2, 0, N, dev[1].ptr(), 2, 0, N, n, 0, 0, 1, K1.p, cap1, cap1, N1.p, W1.p, 1, 0, stream=st)
        Wd(dev[2].ptr(), 2, 0, N, dev[3].ptr(), 2, 0, N, n, Vd.ptr(), 0, 1, K2.p, cap2, cap2, N2.p, W2.p, 1, 0, stream=st)
        J(W1.p, 1, 0, cap1, W2.p, 1, 0, cap2, n, 0, 0, 1, Bd.ptr(), 0, 53, 0, 0, list=K3.p, l_bs=4, cap=4, count=N3.p, stream=st)

    def solutions(K1, N1, K2, N2, W1, W2, K3, N3):
        torch.cuda.synchronize()
        assert N1.body()[0] == cap1 and N2.body()[0] == cap2 and N3.body()[0] == 1
        k1, k2, k3 = K1.body(), K2.body(), K3.body()
        assert k3[0] >> 40 == 0 and (k3[1:] == SENT).all()
        i, jj = divmod(int(k3[0]) & MASK, cap2)
        return [divmod(int(k1[i]) & MASK, N) + divmod(int(k2[jj]) & MASK, N)]

    fresh = lambda: (Out(cap1), Out(1), Out(cap2), Out(1), Out(cap1), Out(cap2), Out(4), Out(1))
    o = fresh()
    five(0, *o)
    assert solutions(*o) == [tuple(a)]
    o = fresh()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        five(torch.cuda.current_stream().cuda_stream, *o)
    torch.cuda.synchronize()
    assert all((x.get() == SENT).all() for x in o), "the capture ran something"
    g.replay()
    assert solutions(*o) == [tuple(a)]
    assert all(x.unchanged() for x in dev)
