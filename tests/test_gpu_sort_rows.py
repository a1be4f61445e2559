"""m4ri_amd_sort_rows_batch_dev on the GPU against the NumPy rule of tests/sort_rows_cases.py.  order, uniq, mult and ucount are compared
EXACTLY: the order is defined, so there is nothing to compare as a set.  Every case has several members, poison behind m_b (order) and
behind ucount (uniq, mult) that must survive, frames of poison around every output, rows behind m_b that are not the list's (read, they
would change the answer), dirt behind column n and in the padding words, and a scratch full of garbage."""
import numpy as np
import pytest
import torch

import lists_collide_cases as lc
import m4ri_amd
import sort_rows_cases as sr

pytestmark = pytest.mark.gpu
SENT, FRAME = -7_777_777, 8
C = m4ri_amd.sort_rows_units(1, 1, 0, 1)[0]


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

    def load(self, host):
        self.host = np.ascontiguousarray(host)
        self.dev.copy_(torch.from_numpy(self.host.copy()))


class Out(Arr):
    """`size` entries between two frames of poison, poison themselves before the call."""

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

    def reset(self):
        self.dev.fill_(SENT)


def scratch_for(nx, n, ell, batch):
    need = m4ri_amd.sort_rows_scratch_bytes(nx, n, ell, batch)
    return (torch.randint(0, 256, (need + 16,), dtype=torch.uint8, device="cuda"), need) if need else (None, 0)


class Sort:
    """One call's operands.  mats: one bit matrix (nx x n) per member, or ONE for a shared list (x_bs = 0); cols: None (NULL: the columns
    0 .. first_ell-1), one window (shared) or one per member; xcount: None (NULL) or one number per member."""

    def __init__(self, mats, n, cols, batch, xcount=None, pad=1, first_ell=0, seed=0):
        rng = np.random.default_rng(2000 + seed)
        self.n, self.batch, self.mats, self.colsb, self.xc, self.first_ell = n, batch, mats, cols, xcount, first_ell
        self.nx = mats[0].shape[0]
        self.stride = lc.width(n) + pad
        self.bs = 0 if len(mats) == 1 else (self.nx + 1) * self.stride + 3
        host = rng.integers(-(1 << 62), 1 << 62, size=max((len(mats) - 1) * self.bs + (self.nx + 1) * self.stride, 1), dtype=np.int64)
        for b, m in enumerate(mats):
            if self.nx and n:
                host[b * self.bs:b * self.bs + self.nx * self.stride] = lc.pack(m, self.stride, rng).ravel()
        self.X = Arr(host)
        self.N = None if xcount is None else Arr(np.array(xcount, dtype=np.int64))
        if cols is None:
            self.cols, self.ell, self.c_bs = None, first_ell, 0
        else:
            per = cols if cols and isinstance(cols[0], (list, tuple)) else [cols]
            self.ell = len(per[0])
            self.c_bs = 0 if len(per) == 1 else self.ell + 1
            host = np.full(max((len(per) - 1) * self.c_bs + self.ell, 1), 12345, dtype=np.int32)
            for b, c in enumerate(per):
                host[b * self.c_bs:b * self.c_bs + self.ell] = c
            self.cols = Arr(host)
        self.l_bs = self.nx + 2
        self.scratch, self.need = scratch_for(self.nx, n, self.ell, batch)

    def rows(self, b):
        return self.nx if self.xc is None else min(max(int(self.xc[b]), 0), self.nx)

    def member(self, b):
        A = self.mats[b if len(self.mats) > 1 else 0][:self.rows(b)]
        if self.colsb is None:
            return A, list(range(self.first_ell))
        return A, (self.colsb[b] if self.colsb and isinstance(self.colsb[0], (list, tuple)) else self.colsb)

    def expect(self, rule=sr.by_lexsort):
        return [sr.expect(*self.member(b), rule) for b in range(self.batch)]

    def call(self, outs="oucm", stream=0):
        size = max((self.batch - 1) * self.l_bs + self.nx, 0)
        o = (Out(size), Out(self.batch), Out(size), Out(size))
        m4ri_amd.sort_rows_batch_dev(self.X.ptr(), self.stride, self.bs, self.nx, self.n, self.N.ptr() if self.N else 0, self.batch,
                                     self.cols.ptr() if self.cols else 0, self.c_bs, self.ell, o[0].p if "o" in outs else 0, o[1].p if "c" in outs else 0,
                                     o[2].p if "u" in outs else 0, o[3].p if "m" in outs else 0, self.l_bs, self.scratch.data_ptr() if self.need else 0,
                                     self.need, stream)
        return o

    def check(self, o, want, outs="oucm"):
        torch.cuda.synchronize()
        order, ucount, uniq, mult = (x.body() for x in o)
        if "c" in outs:
            assert ucount.tolist() == [sr.REFUSED_UCOUNT if w is None else len(w[1]) for w in want], "ucount"
        else:
            assert (ucount == SENT).all()
        for b, w in enumerate(want):
            end = (b * self.l_bs + self.nx) if b == self.batch - 1 else (b + 1) * self.l_bs
            for name, got, k in (("o", order, 0), ("u", uniq, 1), ("m", mult, 2)):
                mine = got[b * self.l_bs:end]
                if name not in outs or w is None:
                    assert (mine == SENT).all(), f"member {b}: {name} was written"
                    continue
                assert np.array_equal(mine[:len(w[k])], w[k]), f"member {b}: {name}"
                assert (mine[len(w[k]):] == SENT).all(), f"member {b}: an entry of {name} behind the last was written"
        for a in (self.X,) + ((self.N,) if self.N else ()) + ((self.cols,) if self.cols else ()):
            assert a.unchanged(), "a read-only operand changed"

    def run(self, outs="oucm"):
        want = self.expect()
        self.check(self.call(outs), want, outs)
        return want


def _window(n, ell, seed):
    """ell columns: unsorted, across the words, the first repeated at the end where there are three or more."""
    rng = np.random.default_rng(seed)
    cols = [int(c) for c in (rng.permutation(n)[:ell] if ell <= n else rng.integers(0, n, ell))]
    if ell >= 3:
        cols[-1] = cols[0]
    return cols


def _pooled(batch, nx, n, pool, seed):
    return [sr.pool_rows(np.random.default_rng(seed + b), nx, n, pool) for b in range(batch)]


# ---- the list lengths ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("nx", [0, 1, 2, 3, 63, 64, 65, 255, 256, 257, C - 1, C])
def test_path0_lengths(nx):
    n, batch = 130, 3
    assert m4ri_amd.plan_sort_rows_batch(nx, n, 13, batch) == 0
    s = Sort(_pooled(batch, nx, n, max(nx // 7, 1), 10 * nx), n, _window(n, 13, nx), batch, seed=nx)
    want = s.run()
    if nx >= 63:
        assert all(1 < len(w[1]) < nx and w[2].max() > 1 for w in want)         # there are classes, and more than one


@pytest.mark.parametrize("nx,levels", [(C + 1, 1), (2 * C, 1), (2 * C + 1, 2), (4 * C + 3, 3)])
def test_path1_lengths(nx, levels):
    n, batch = 65, 2
    assert m4ri_amd.plan_sort_rows_batch(nx, n, 13, batch) == 1
    assert m4ri_amd.sort_rows_units(nx, n, 13, batch)[1] == C << levels           # that many merge levels with global strides
    s = Sort(_pooled(batch, nx, n, nx // 5, 3 * nx), n, _window(n, 13, nx), batch, seed=nx)
    want = s.run()
    assert all(1 < len(w[1]) < nx and w[2].max() > 1 for w in want)


def test_path1_distinct_rows_and_a_window_that_separates_them():
    """Random rows of 130 bits, all distinct, a window of 32 columns: almost no comparison reads a row."""
    nx, n, batch = 2 * C + 1, 130, 2
    mats = [np.random.default_rng(70 + b).integers(0, 2, (nx, n), dtype=np.uint8) for b in range(batch)]
    want = Sort(mats, n, _window(n, 32, 5), batch, seed=71).run()
    assert all(len(w[1]) == nx for w in want)


# ---- the row widths -------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [1, 63, 64, 65, 130, 1000, 1024])
@pytest.mark.parametrize("pad", [1, 2])
def test_row_widths(n, pad):
    nx, batch = 300, 3
    s = Sort(_pooled(batch, nx, n, 23, n), n, _window(n, min(n, 13), n), batch, pad=pad, seed=n)
    s.run()


# ---- the classes ----------------------------------------------------------------------------------------------------------------------------

def _class_cases(nx, n, window):
    rng = np.random.default_rng(nx)
    base = rng.integers(0, 2, n, dtype=np.uint8)
    equal = np.tile(base, (nx, 1))
    distinct = rng.integers(0, 2, (nx, n), dtype=np.uint8)
    distinct[:, :24] = (np.arange(nx)[:, None] >> np.arange(24)[None, :]) & 1            # the index in the low bits: no two rows equal
    last = equal.copy()
    last[::3, n - 1] ^= 1                                                                # only the last valid bit differs
    out = equal.copy()
    out[::2, n - 1] ^= 1                                                                 # only bits in the words outside the window
    out[::5, 130] ^= 1
    inside = equal.copy()
    inside[:, window[0]] = rng.integers(0, 2, nx)                                        # only inside the window
    inside[:, window[1]] = rng.integers(0, 2, nx)
    return {"equal": (equal, 1), "distinct": (distinct, nx), "last-bit": (last, 2), "outside": (out, 4), "inside": (inside, 4)}


@pytest.mark.parametrize("nx", [257, C + 1], ids=["path0", "path1"])
@pytest.mark.parametrize("kind", ["equal", "distinct", "last-bit", "outside", "inside"])
def test_classes(nx, kind):
    n, window = 200, [70, 3, 69]                      # the window in the words 0 and 1; the words 2 and 3 are outside it
    A, classes = _class_cases(nx, n, window)[kind]
    s = Sort([A, A[::-1].copy()], n, window, 2, seed=nx)
    want = s.run()
    assert [len(w[1]) for w in want] == [classes, classes]


def test_rows_equal_on_the_valid_bits_are_one_class_whatever_the_dirt():
    n = 70
    A = np.zeros((2, n), dtype=np.uint8)
    A[:, 5] = 1
    s = Sort([A, A], n, [5, 69], 2, pad=2)
    X = s.X.get()
    assert X[1] != X[1 + s.stride] and X[2] != X[2 + s.stride]      # the two rows differ behind column n and in the padding
    want = s.run()
    assert [w[1].tolist() for w in want] == [[0], [0]] and [w[2].tolist() for w in want] == [[2], [2]]


# ---- the windows ----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("nx", [300, C + 1], ids=["path0", "path1"])
@pytest.mark.parametrize("ell", [0, 1, 13, 64])
def test_windows(nx, ell):
    n, batch = 130, 3
    mats = _pooled(batch, nx, n, 40, ell)
    Sort(mats, n, _window(n, ell, ell), batch, seed=ell).run()                                        # one window for all members
    Sort(mats, n, [_window(n, ell, 100 + b) for b in range(batch)], batch, seed=ell).run()              # one per member
    Sort(mats, n, None, batch, first_ell=ell, seed=ell).run()                                         # NULL: the columns 0 .. ell-1


@pytest.mark.parametrize("nx", [65, C + 1], ids=["path0", "path1"])
@pytest.mark.parametrize("bad", [130, -1])
def test_refused_members_among_good_ones(nx, bad):
    n, batch = 130, 4
    cols = [_window(n, 5, b) for b in range(batch)]
    cols[1][3] = bad
    cols[3][0] = bad
    s = Sort(_pooled(batch, nx, n, 9, nx), n, cols, batch, seed=nx)
    want = s.run()
    assert [w is None for w in want] == [False, True, False, True]
    for outs in ("o", "c", "oc"):
        s.check(s.call(outs), want, outs)


# ---- xcount ---------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("nx", [300, C + 1], ids=["path0", "path1"])
def test_xcount(nx):
    n = 130
    counts = [nx, 0, -1, nx + 5, 1, nx // 2, 2, nx - 1] + ([C, C - 5, C // 2] if nx > C else [])
    A = sr.pool_rows(np.random.default_rng(nx), nx, n, 30)
    want = Sort([A], n, _window(n, 13, 1), len(counts), xcount=counts, seed=nx).run()        # one shared list, a length per member
    assert [len(w[0]) for w in want] == [min(max(c, 0), nx) for c in counts]
    mats = _pooled(3, nx, n, 30, nx + 1)
    Sort(mats, n, _window(n, 13, 2), 3, xcount=[nx - 2, 0, 7], seed=nx).run()
    Sort(mats, n, _window(n, 13, 2), 3, xcount=None, seed=nx).run()


# ---- the outputs ----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("nx", [257, C + 1], ids=["path0", "path1"])
def test_every_legal_combination_of_outputs(nx):
    n, batch = 65, 3
    s = Sort(_pooled(batch, nx, n, 50, nx), n, _window(n, 13, 3), batch, xcount=[nx, nx - 3, 5], seed=nx)
    want = s.expect()
    for outs in ("o", "c", "oc", "cu", "ocu", "cum", "ocum"):
        s.check(s.call(outs), want, outs)
    if nx <= 300:                                                                    # the other form of the rule, once
        assert all(np.array_equal(a, b) for w, v in zip(want, s.expect(sr.by_sorted)) for a, b in zip(w, v))


def test_degenerate_members():
    # n = 0: all rows are equal
    for nx in (0, 1, 5):
        s = Sort([np.zeros((nx, 0), dtype=np.uint8)] * 2, 0, None, 2, xcount=[nx, nx - 1])
        want = s.run()
        assert [w[0].tolist() for w in want] == [list(range(nx)), list(range(max(nx - 1, 0)))]
        assert [w[1].tolist() for w in want] == [[0] if nx else [], [0] if nx > 1 else []]
    # n = 0 with a window: every entry is outside
    s = Sort([np.zeros((3, 0), dtype=np.uint8)] * 2, 0, [0], 2)
    assert s.run() == [None, None]
    # nx = 0, with and without a refused member
    s = Sort([np.zeros((0, 64), dtype=np.uint8)] * 3, 64, [[1, 2], [1, 64], [0, 0]], 3)
    assert [w is None for w in s.run()] == [False, True, False]
    # batch = 0 touches nothing
    o = Out(4)
    m4ri_amd.sort_rows_batch_dev(0, 1, 0, 4, 64, batch=0, order=o.p, l_bs=4)
    torch.cuda.synchronize()
    assert (o.body() == SENT).all()


# ---- end to end: join, words, sort, gather --------------------------------------------------------------------------------------------------

def _chain_inputs(seed, nx, ny, n, pool):
    rng = np.random.default_rng(seed)
    return [sr.pool_rows(rng, nx, n, pool) for _ in range(2)], [sr.pool_rows(rng, ny, n, pool) for _ in range(2)]


@pytest.mark.parametrize("nx,ny,pool,cap,path", [(100, 100, 30, 4096, 0), (300, 300, 60, 2 * C, 1)], ids=["path0", "path1"])
def test_join_words_sort_gather(nx, ny, pool, cap, path):
    """Two members: X_b and Y_b joined on three columns, the words of the listed pairs written out, those sorted on the next window with
    xcount = the join's count still on the device, and the deduplicated sorted list gathered by lists_words_batch_dev with uniq as its
    keys (Y one zero row, ny = 1).  The join lists its pairs in no particular order, so the indices in uniq may differ from run to run;
    the gathered rows may not: they are np.unique(axis=0) of the joined words, re-ordered by the rule.  Eagerly, then from one captured
    graph replayed on other inputs and on the first again."""
    n, batch, ws = 64, 2, 2
    A, B = [5, 1, 9], [40, 63, 12, 33, 20, 11, 58, 47, 40]
    assert m4ri_amd.plan_sort_rows_batch(cap, n, len(B), batch) == path
    sets = [_chain_inputs(s, nx, ny, n, pool) for s in (900 + path, 950 + path)]
    rng = np.random.default_rng(7)
    packed = lambda mats, stride: np.concatenate([lc.pack(m, stride, rng).ravel() for m in mats])
    Xd, Yd = Arr(packed(sets[0][0], 1)), Arr(packed(sets[0][1], 2))
    Ad, Bd, Zd = Arr(np.array(A, dtype=np.int32)), Arr(np.array(B, dtype=np.int32)), Arr(np.zeros(1, dtype=np.int64))
    scratch, need = scratch_for(cap, n, len(B), batch)
    K1, N1, W1, UC, UQ, MU, W2, SK = Out(batch * cap), Out(batch), Out(batch * cap * ws), Out(batch), Out(batch * cap), Out(batch * cap), Out(batch * cap * ws), Out(batch, np.int32)
    outs = (K1, N1, W1, UC, UQ, MU, W2, SK)

    def chain(st):
        m4ri_amd.lists_collide_batch_dev(Xd.ptr(), 1, nx, nx, Yd.ptr(), 2, 2 * ny, ny, n, 0, 0, batch, Ad.ptr(), 0, len(A), 0, n, list=K1.p, l_bs=cap, cap=cap,
                                         count=N1.p, stream=st)
        m4ri_amd.lists_words_batch_dev(Xd.ptr(), 1, nx, nx, Yd.ptr(), 2, 2 * ny, ny, n, 0, 0, batch, K1.p, cap, cap, N1.p, W1.p, ws, cap * ws, stream=st)
        m4ri_amd.sort_rows_batch_dev(W1.p, ws, cap * ws, cap, n, N1.p, batch, Bd.ptr(), 0, len(B), 0, UC.p, UQ.p, MU.p, cap, scratch.data_ptr() if need else 0,
                                     need, st)
        m4ri_amd.lists_words_batch_dev(W1.p, ws, cap * ws, cap, Zd.ptr(), 1, 0, 1, n, 0, 0, batch, UQ.p, cap, cap, UC.p, W2.p, ws, cap * ws, SK.p, stream=st)

    def check(which):
        torch.cuda.synchronize()
        n1, uc, uq, mu, w1, w2 = N1.body(), UC.body(), UQ.body(), MU.body(), W1.body().reshape(batch, cap, ws), W2.body().reshape(batch, cap, ws)
        assert SK.body().tolist() == [0] * batch
        for b in range(batch):
            X, Y = sets[which][0][b], sets[which][1][b]
            _, r = lc.join(X, Y, None, A)
            assert 0 < len(r) <= cap and n1[b] == len(r) and (path == 0 or len(r) > C)
            rows, counts = np.unique(lc.words_of(X, Y, None, r), axis=0, return_counts=True)
            order = sr.by_lexsort(rows, B)
            assert uc[b] == len(rows) < len(r)                                       # there were duplicates
            assert np.array_equal(lc.unpack(w2[b, :uc[b], :1], n), rows[order]), f"member {b}: the deduplicated sorted list"
            assert np.array_equal(mu[b * cap:b * cap + uc[b]], counts[order]), f"member {b}: mult"
            assert (w2[b, uc[b]:] == SENT).all() and (w2[b, :, 1] == SENT).all() and (mu[b * cap + uc[b]:(b + 1) * cap] == SENT).all()
            heads = uq[b * cap:b * cap + uc[b]]
            assert np.array_equal(lc.unpack(w1[b, heads, :1], n), rows[order]) and (uq[b * cap + uc[b]:(b + 1) * cap] == SENT).all()

    def load(which):
        Xd.load(packed(sets[which][0], 1))
        Yd.load(packed(sets[which][1], 2))
        for o in outs:
            o.reset()

    chain(0)
    check(0)
    load(0)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        chain(torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert all((x.get() == SENT).all() for x in outs), "the capture ran something"
    for which in (1, 0):
        load(which)
        g.replay()
        check(which)
