"""m4ri_amd_isd_search_dev (include/m4ri_amd.h, isd_search_batch.hip) on the device: every output -- ALL words of D's image, the dirty
padding words, tail bits and gaps between members included, pivots, order, best, best_iter, iters_run, done and the image of W with
the entries around them -- against the NumPy rule of tests/isd_cases.py (pinned to the two rules it composes by
tests/test_isd_search_plan.py) on both paths of m4ri_amd_plan_isd_search, the path-0 shapes again forced down path 1 with identical
bytes; against the two-call loop of the library itself; a decoding end to end; and the chain from one captured graph."""
from functools import lru_cache

import numpy as np
import pytest
import torch

import isd_cases as ic
import m4ri_amd
import order_cases as oc

pytestmark = pytest.mark.gpu
PATH0_MAX = "M4RI_AMD_ISD_SEARCH_PATH0_MAX"
# (nrows, ncols, pivot_rows): the row behind pivot_rows is the received word, further rows follow
SHAPES0 = [(1, 1, 1), (2, 64, 1), (9, 17, 8), (33, 40, 32), (64, 64, 63), (64, 64, 64)]
SHAPES1 = [(65, 64, 64), (17, 65, 16), (33, 128, 32), (20, 130, 16), (40, 300, 36), (24, 1024, 20)]
KINDS = ("full", "deficient", "full", "refused", "full")
ALL = (True, True, True, True)        # best_iter, iters_run, done, W wanted


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    assert m4ri_amd.lib().m4ri_amd_device_count() >= 1, "no HIP device visible: the gpu tests have nothing to run on"
    m4ri_amd.init(0)
    torch.cuda.set_device(0)


def _state(rng, m, n, k, kind):
    """One member in the state echelonize_order_batch_dev(full = 1) leaves: (the form, pivots, rank, the order it was made on).  kind:
    "full" (as random bits fall), "deficient" (repeated pivot rows: rank < pivot_rows), "refused" (rank -1, pivots -1, D whatever)."""
    A = rng.integers(0, 2, size=(m, n), dtype=np.uint8)
    if kind == "deficient" and k >= 2:
        A[k // 2: k] = A[: k - k // 2]
    order = rng.permutation(n).astype(np.int32)
    if kind == "refused":
        return A, np.full(min(k, n), -1, dtype=np.int32), -1, order
    S, rank, piv = oc.ech_order(A, order, 1, k)
    return S, piv, rank, order


class Case:
    """The host side of one call: images and what has to come back.  Built once per argument tuple (the paths and the output
    combinations share it).  w_stop: a number, "first" (the weight member 0 has at iteration 0: it stops there) or "mid" (the weight
    member 0's best has reached at iteration iters // 2: the members stop at different iterations)."""

    def __init__(self, m, n, k, t, batch, iters, steps, w_min, w_stop, seed, kinds=("full",), order=True, call_seed=0, tight=False):
        rng = np.random.default_rng(seed)
        self.m, self.n, self.k, self.t, self.batch, self.iters, self.steps, self.w_min, self.seed = m, n, k, t, batch, iters, steps, w_min, call_seed
        self.pm = pm = min(k, n)
        self.width = width = (n + 63) // 64
        self.d_stride = width if tight else width + 2
        self.d_bs = m * self.d_stride if tight else (m * self.d_stride + 5) | 1
        self.w_bs = width if tight else width + 1
        self.states = states = [_state(rng, m, n, k, kinds[b % len(kinds)]) for b in range(batch)]
        orders = [s[3] if order else None for s in states]
        if w_stop in ("first", "mid"):
            free = ic.search(states[0][0], states[0][1], states[0][2], k, iters, steps, call_seed, t, w_min, -1, b=0, order=orders[0])
            upto = free.keys[: 1 if w_stop == "first" else iters // 2 + 1]
            w_stop = min([key >> 40 for key in upto if key >= 0], default=-1)
        self.w_stop = w_stop
        self.ref = [ic.search(S, piv, rank, k, iters, steps, call_seed, t, w_min, w_stop, b=b, order=orders[b]) for b, (S, piv, rank, _o) in enumerate(states)]
        self.D, idx, valid = oc.pack([s[0] for s in states], m, n, self.d_stride, self.d_bs, seed + 1)
        self.P = np.concatenate([s[1] for s in states] + [np.full(2, -7, dtype=np.int32)]).astype(np.int32)
        self.R = np.array([s[2] for s in states] + [-7, -7], dtype=np.int32)
        self.olen = n if order else 0
        self.o_bs = self.olen + 3 if order else 0
        self.O = None
        if order:
            self.O = np.full((batch - 1) * self.o_bs + self.olen + 4, -(1 << 31), dtype=np.int32)
            for b, o in enumerate(orders):
                self.O[b * self.o_bs: b * self.o_bs + n] = o
        self.W = rng.integers(0, 1 << 63, size=(batch - 1) * self.w_bs + width + 3, dtype=np.int64).view(np.uint64) * np.uint64(3)
        # what has to come back
        self.want_D, self.want_P, self.want_O, self.want_W = self.D.copy(), self.P.copy(), None if self.O is None else self.O.copy(), self.W.copy()
        self.want = {name: np.full(batch + 2, -7, dtype=np.int64 if name == "best" else np.int32) for name in ("best", "best_iter", "iters_run", "done")}
        for b, r in enumerate(self.ref):
            oc.put(self.want_D, idx, valid, b, r.bits)
            self.want_P[b * pm: (b + 1) * pm] = r.pivots
            if order:
                self.want_O[b * self.o_bs: b * self.o_bs + n] = r.order
            for name in self.want:
                if iters > 0 or name in ("best", "iters_run"):      # a call of no iteration touches nothing else
                    self.want[name][b] = getattr(r, name)
            if r.best >= 0:
                at = slice(b * self.w_bs, b * self.w_bs + width)
                self.want_W[at] = (self.W[at] & ~valid) | (oc.to_words(r.W[None, :])[0] & valid)

    def run(self, outs=ALL, ints=True, stream=0):
        """The call on fresh copies of the images; every byte that came back, after it was compared.  outs: which of best_iter,
        iters_run, done and W are wanted; ints: pivots and rank passed (they may be absent where no exchange can happen)."""
        tD = torch.from_numpy(self.D.view(np.int64).copy()).cuda()
        tP, tR = torch.from_numpy(self.P.copy()).cuda(), torch.from_numpy(self.R.copy()).cuda()
        tO = None if self.O is None else torch.from_numpy(self.O.copy()).cuda()
        tW = torch.from_numpy(self.W.view(np.int64).copy()).cuda()
        tB = torch.full((self.batch + 2,), -7, dtype=torch.int64, device="cuda")
        tI, tU, tN = (torch.full((self.batch + 2,), -7, dtype=torch.int32, device="cuda") for _ in range(3))
        torch.cuda.synchronize()
        m4ri_amd.isd_search_dev(tD.data_ptr(), self.d_stride, self.d_bs, self.m, self.n, self.k, tP.data_ptr() if ints else 0, tR.data_ptr() if ints else 0,
                                self.batch, self.iters, self.steps, self.seed, self.t, self.w_min, self.w_stop, tB.data_ptr(),
                                0 if tO is None else tO.data_ptr(), self.o_bs, self.olen, tI.data_ptr() if outs[0] else 0, tU.data_ptr() if outs[1] else 0,
                                tN.data_ptr() if outs[2] else 0, tW.data_ptr() if outs[3] else 0, self.w_bs, stream)
        torch.cuda.synchronize()
        got = [tD.cpu().numpy().view(np.uint64), tP.cpu().numpy(), tR.cpu().numpy(), None if tO is None else tO.cpu().numpy(), tB.cpu().numpy(),
               tI.cpu().numpy(), tU.cpu().numpy(), tN.cpu().numpy(), tW.cpu().numpy().view(np.uint64)]
        wrong = np.flatnonzero(got[0] != self.want_D)
        assert wrong.size == 0, f"{wrong.size} words of D differ, first at {wrong[:5]} (d_bs {self.d_bs}, d_stride {self.d_stride})"
        assert np.array_equal(got[1], self.want_P), "pivots"
        assert np.array_equal(got[2], self.R), "rank was written"
        if tO is not None:
            assert np.array_equal(got[3], self.want_O), "order"
        assert np.array_equal(got[4], self.want["best"]), ("best", got[4], self.want["best"])
        untouched = np.full(self.batch + 2, -7, dtype=np.int32)
        for at, name, wanted in ((5, "best_iter", outs[0]), (6, "iters_run", outs[1]), (7, "done", outs[2])):
            assert np.array_equal(got[at], self.want[name] if wanted else untouched), (name, got[at], self.want[name])
        assert np.array_equal(got[8], self.want_W if outs[3] else self.W), "W"
        return got


@lru_cache(maxsize=None)
def _case(*args, **kw):
    return Case(*args, **kw)


def _both(monkeypatch, c, outs=ALL, ints=True):
    """The routed path; a path-0 shape again forced down path 1, and the two leave identical bytes."""
    monkeypatch.delenv(PATH0_MAX, raising=False)
    got = c.run(outs, ints)
    if m4ri_amd.plan_isd_search(c.m, c.n, c.k, c.t) == 0:
        monkeypatch.setenv(PATH0_MAX, "0")
        forced = c.run(outs, ints)
        assert all(np.array_equal(x, y) for x, y in zip(got, forced) if x is not None)
    return got


def _sweep(monkeypatch, m, n, k, t, iters=5):
    base = 1000 * m + 10 * n + t
    if k >= 63 and t == 3:
        iters = 3          # about 40 000 sums per enumeration of the NumPy rule
    a = _case(m, n, k, t, 5, iters, 1, 1, -1, base, kinds=KINDS, order=True, call_seed=base + 50)
    b = _case(m, n, k, t, 4, iters, 3, 0, "mid", base + 1, kinds=("full", "full", "deficient"), order=False, call_seed=base + 51)
    _both(monkeypatch, a)
    _both(monkeypatch, b)
    return a, b


@pytest.mark.parametrize("m,n,k", SHAPES0)
@pytest.mark.parametrize("t", [0, 1, 2, 3])
def test_wave_path_shapes(monkeypatch, m, n, k, t):
    assert m4ri_amd.plan_isd_search(m, n, k, t) == 0
    _sweep(monkeypatch, m, n, k, t)


def test_wave_path_four_rows(monkeypatch):
    assert m4ri_amd.plan_isd_search(13, 30, 12, 4) == 0
    a, _b = _sweep(monkeypatch, 13, 30, 12, 4, iters=9)
    assert sum(r.done for r in a.ref) > 0 and any(r.best_iter > 0 for r in a.ref)


@pytest.mark.parametrize("m,n,k", SHAPES1)
@pytest.mark.parametrize("t", [0, 1, 2, 3])
def test_lds_path_shapes(monkeypatch, m, n, k, t):
    assert m4ri_amd.plan_isd_search(m, n, k, t) == 1
    _sweep(monkeypatch, m, n, k, t)


@pytest.mark.parametrize("m,n,k,t,uppers", [(71, 140, 70, 2, 70), (14, 70, 13, 3, 78), (65, 70, 64, 2, 64), (66, 70, 65, 2, 65)])
def test_both_sides_of_a_chunk_of_upper_parts(monkeypatch, m, n, k, t, uppers):
    """64 upper parts fill one chunk of a wave, 65 start a second one with a single lane; 70 and 78 as well."""
    from math import comb
    assert comb(k, t - 1) == uppers and m4ri_amd.plan_isd_search(m, n, k, t) == 1
    _sweep(monkeypatch, m, n, k, t)


@pytest.mark.parametrize("m,n,k,t", [(9, 17, 2, 3), (3, 64, 1, 2), (20, 130, 2, 3), (66, 64, 0, 1)])
def test_no_sums(monkeypatch, m, n, k, t):
    """k < t: best -1 in every iteration, nothing stops, W untouched; the exchanges are performed all the same."""
    c = _case(m, n, k, t, 3, 5, 2, 0, 5, 7 * m + n, order=True, call_seed=3)
    assert all(r.best == -1 and r.best_iter == -1 and r.iters_run == 5 and r.W is None for r in c.ref)
    assert k == 0 or sum(r.done for r in c.ref) > 0
    _both(monkeypatch, c)


@pytest.mark.parametrize("m,n,k", [(9, 17, 8), (17, 65, 16)])
@pytest.mark.parametrize("iters", [1, 2, 5, 40])
@pytest.mark.parametrize("steps", [0, 1, 3])
def test_loop_parameters(monkeypatch, m, n, k, iters, steps):
    """Every stop (at iteration 0, in the middle, never) with every w_min (0, 1, above every weight), members of every kind that stop at
    different iterations within one batch, an order kept and not kept."""
    stops = set()
    for i, w_stop in enumerate(("first", "mid", -1)):
        for j, w_min in enumerate((0, 1, n + 1)):
            c = _case(m, n, k, 2, 5, iters, steps, w_min, w_stop, 100 * iters + 10 * steps + 3 * i + j, kinds=KINDS, order=(i + j) % 2 == 0,
                      call_seed=iters + steps + i + j)
            _both(monkeypatch, c)
            if w_min == n + 1:
                assert all(r.best == -1 and r.iters_run == iters for r in c.ref)
            elif w_stop == "first":
                assert c.ref[0].iters_run == 1
            stops.add(tuple(r.iters_run for r in c.ref))
    if iters == 40 and steps:
        assert any(len(set(s)) >= 3 for s in stops)          # members that stop at different iterations within one batch


@pytest.mark.parametrize("m,n,k", [(33, 40, 32), (20, 130, 16)])
def test_every_combination_of_the_optional_outputs(monkeypatch, m, n, k):
    c = _case(m, n, k, 2, 4, 6, 2, 1, "mid", 5 * m + n, kinds=("full", "deficient"), order=True, call_seed=17)
    for mask in range(16):
        _both(monkeypatch, c, outs=tuple(bool(mask >> i & 1) for i in range(4)))


@pytest.mark.parametrize("m,n,k", [(9, 17, 8), (17, 65, 16)])
def test_pivots_and_rank_may_be_absent_where_nothing_is_exchanged(monkeypatch, m, n, k):
    _both(monkeypatch, _case(m, n, k, 2, 3, 1, 3, 1, -1, 40 + m, order=False), ints=False)      # one iteration
    _both(monkeypatch, _case(m, n, k, 2, 3, 7, 0, 1, -1, 41 + m, order=False), ints=False)      # no steps


def test_no_iteration_and_no_columns():
    """iters = 0: best -1 and iters_run 0, nothing else touched.  ncols = 0: every word weighs 0, nothing is exchanged."""
    tB = torch.full((5,), -7, dtype=torch.int64, device="cuda")
    tI, tU, tN = (torch.full((5,), -7, dtype=torch.int32, device="cuda") for _ in range(3))
    c = _case(9, 17, 8, 2, 3, 0, 2, 1, -1, 9, order=True)
    assert all(r.best == -1 and r.iters_run == 0 for r in c.ref)
    got = c.run()
    assert got[5][:3].tolist() == [-7] * 3 and got[7][:3].tolist() == [-7] * 3        # best_iter and done of a call without iterations
    for (t, w_min, w_stop, want) in [(0, 0, -1, (0, 0, 6, 0)), (2, 0, 0, (0, 0, 1, 0)), (2, 1, 0, (-1, -1, 6, 0)), (4, 0, 3, (-1, -1, 6, 0))]:
        for x in (tB, tI, tU, tN):
            x.fill_(-7)
        m4ri_amd.isd_search_dev(0, 0, 0, 4, 0, 3, 0, 0, 3, 6, 2, 5, t, w_min, w_stop, tB.data_ptr(), best_iter=tI.data_ptr(), iters_run=tU.data_ptr(),
                                done=tN.data_ptr())
        torch.cuda.synchronize()
        for x, v in zip((tB, tI, tU, tN), want):
            assert x.cpu().tolist() == [v] * 3 + [-7] * 2, (t, w_min, w_stop)


def test_operands_packed_back_to_back(monkeypatch):
    """The accepted neighbours of the overlap checks, on the device: D's members with no word between them, then best and W in the same
    allocation; pivots, rank, order, best_iter, iters_run and done in one allocation with nothing between them."""
    for (m, n, k) in ((33, 40, 32), (20, 130, 16)):
        monkeypatch.delenv(PATH0_MAX, raising=False)
        c = _case(m, n, k, 2, 3, 6, 2, 1, -1, 80 + m, order=True, tight=True, call_seed=5)
        batch, pm, nD = 3, c.pm, 3 * m * c.width
        nO = (batch - 1) * c.o_bs + n
        tL = torch.from_numpy(np.concatenate([c.D[:nD], np.full(batch, 7, dtype=np.uint64), c.W[: batch * c.width]]).view(np.int64)).cuda()
        tS = torch.from_numpy(np.concatenate([c.P[: batch * pm], c.R[:batch], c.O[:nO], np.full(3 * batch, -7, dtype=np.int32)])).cuda()
        at = tS.data_ptr() + 4 * np.cumsum([0, batch * pm, batch, nO, batch, batch])
        m4ri_amd.isd_search_dev(tL.data_ptr(), c.d_stride, c.d_bs, m, n, k, int(at[0]), int(at[1]), batch, c.iters, c.steps, c.seed, c.t, c.w_min, c.w_stop,
                                tL.data_ptr() + 8 * nD, int(at[2]), c.o_bs, n, int(at[3]), int(at[4]), int(at[5]), tL.data_ptr() + 8 * (nD + batch), c.w_bs)
        torch.cuda.synchronize()
        want_L = np.concatenate([c.want_D[:nD], c.want["best"][:batch].view(np.uint64), c.want_W[: batch * c.width]])
        want_S = np.concatenate([c.want_P[: batch * pm], c.R[:batch], c.want_O[:nO], c.want["best_iter"][:batch], c.want["iters_run"][:batch],
                                 c.want["done"][:batch]])
        assert np.array_equal(tL.cpu().numpy().view(np.uint64), want_L) and np.array_equal(tS.cpu().numpy(), want_S)
        assert sum(r.done for r in c.ref) > 0


# ---- against the library itself --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("m,n,k,t,steps", [(33, 64, 32, 2, 1), (64, 64, 64, 1, 4), (65, 128, 64, 2, 1), (40, 300, 36, 2, 4)])
def test_the_two_call_loop_gives_the_same(monkeypatch, m, n, k, t, steps):
    """w_stop = -1: a host loop of pivot_exchange_batch_dev(seed = isd_iteration_seed(seed, it)) and row_sums_weights_batch_dev over the
    same members leaves the same D, pivots and order bit for bit, and the lightest of its keys (the earliest among equal weights) is best."""
    monkeypatch.delenv(PATH0_MAX, raising=False)
    iters, seed, batch = 12, 77, 8
    c = _case(m, n, k, t, batch, iters, steps, 1, -1, 3 * m + n, kinds=("full", "full", "deficient", "refused"), order=True, call_seed=seed)
    got = c.run()
    tD = torch.from_numpy(c.D.view(np.int64).copy()).cuda()
    tP, tR, tO = torch.from_numpy(c.P.copy()).cuda(), torch.from_numpy(c.R.copy()).cuda(), torch.from_numpy(c.O.copy()).cuda()
    tL = torch.full((iters, batch), -7, dtype=torch.int64, device="cuda")
    V = tD.data_ptr() + 8 * k * c.d_stride if m > k else 0
    for it in range(iters):
        if it:
            m4ri_amd.pivot_exchange_batch_dev(tD.data_ptr(), c.d_stride, c.d_bs, m, n, k, tP.data_ptr(), tR.data_ptr(), batch, 0, 0, steps,
                                              m4ri_amd.isd_iteration_seed(seed, it), tO.data_ptr(), c.o_bs, n)
        m4ri_amd.row_sums_weights_batch_dev(tD.data_ptr(), c.d_stride, c.d_bs, k, n, V, c.d_bs, batch, t, 1, 0, tL[it].data_ptr())
    torch.cuda.synchronize()
    assert np.array_equal(tD.cpu().numpy().view(np.uint64), got[0]) and np.array_equal(tP.cpu().numpy(), got[1]) and np.array_equal(tO.cpu().numpy(), got[3])
    keys = tL.cpu().numpy()
    for b in range(batch):
        weights = [(int(key) >> 40 if key >= 0 else 1 << 30) for key in keys[:, b]]
        first = weights.index(min(weights))
        assert got[4][b] == keys[first, b] and got[5][b] == (first if keys[first, b] >= 0 else -1), b


# ---- a decoding, end to end -------------------------------------------------------------------------------------------------------------------

DEC_K, DEC_N, DEC_MEMBERS, DEC_WT, DEC_ITERS = 32, 64, 32, 6, 400
DEC_SEED = 2          # chosen on the CPU with the NumPy rule: it finds a word of weight <= 6 for every member within the 400 iterations
DEC_LONGEST = 316     # (seed 1 leaves some members unfound), and this is the largest iters_run among them


@lru_cache(maxsize=None)
def _decoding():
    """32 random 32 x 64 generators, y = a codeword + an error of weight 6 stacked under each; the forms on the random orders of seed
    DEC_SEED, and the rule's search on them (Lee-Brickell, t = 1, one exchange per iteration)."""
    rng = np.random.default_rng(2024)
    k, n = DEC_K, DEC_N
    stacked, forms, refs = [], [], []
    for b in range(DEC_MEMBERS):
        G = rng.integers(0, 2, size=(k, n), dtype=np.uint8)
        e = np.zeros(n, dtype=np.uint8)
        e[rng.choice(n, DEC_WT, replace=False)] = 1
        y = (rng.integers(0, 2, size=k, dtype=np.uint8) @ G & 1) ^ e
        A = np.concatenate([G, y[None, :]])
        order = oc.random_order(DEC_SEED, b, n)
        S, rank, piv = oc.ech_order(A, order, 1, k)
        stacked.append(A)
        forms.append((S, rank, piv, order))
        refs.append(ic.search(S, piv, rank, k, DEC_ITERS, 1, DEC_SEED, 1, 0, DEC_WT, b=b, order=order))
    return stacked, forms, refs


def _in_row_space(G, w):
    return oc.ech_order(np.concatenate([G, w[None, :]]), None, 1, G.shape[0] + 1)[1] == oc.ech_order(G, None, 1, G.shape[0])[1]


def test_decoding_end_to_end():
    stacked, forms, refs = _decoding()
    k, n, batch = DEC_K, DEC_N, DEC_MEMBERS
    assert all(0 <= r.best >> 40 <= DEC_WT for r in refs) and max(r.iters_run for r in refs) == DEC_LONGEST      # the rule finds all 32
    tA = torch.from_numpy(np.concatenate([oc.to_words(A).reshape(-1) for A in stacked]).view(np.int64)).cuda()
    tD, tO = torch.zeros_like(tA), torch.full((batch * n,), -7, dtype=torch.int32, device="cuda")
    tr, tp = torch.full((batch,), -7, dtype=torch.int32, device="cuda"), torch.full((batch * k,), -7, dtype=torch.int32, device="cuda")
    tB, tW = torch.full((batch,), -7, dtype=torch.int64, device="cuda"), torch.zeros((batch,), dtype=torch.int64, device="cuda")
    tI, tU, tN = (torch.full((batch,), -7, dtype=torch.int32, device="cuda") for _ in range(3))
    m4ri_amd.random_orders_batch_dev(tO.data_ptr(), n, n, batch, DEC_SEED)
    m4ri_amd.echelonize_order_batch_dev(tD.data_ptr(), 1, k + 1, tA.data_ptr(), 1, k + 1, k + 1, n, k, tO.data_ptr(), n, n, batch, 1, tr.data_ptr(), tp.data_ptr())
    m4ri_amd.isd_search_dev(tD.data_ptr(), 1, k + 1, k + 1, n, k, tp.data_ptr(), tr.data_ptr(), batch, DEC_ITERS, 1, DEC_SEED, 1, 0, DEC_WT, tB.data_ptr(),
                            tO.data_ptr(), n, n, tI.data_ptr(), tU.data_ptr(), tN.data_ptr(), tW.data_ptr(), 1)
    torch.cuda.synchronize()
    D, W = tD.cpu().numpy().view(np.uint64).reshape(batch, k + 1, 1), tW.cpu().numpy().view(np.uint64)
    for b, r in enumerate(refs):
        assert (tB[b].item(), tI[b].item(), tU[b].item(), tN[b].item()) == (r.best, r.best_iter, r.iters_run, r.done), b
        assert np.array_equal(D[b], oc.to_words(r.bits)) and np.array_equal(tp.cpu().numpy()[b * k:][:k], r.pivots), b
        assert np.array_equal(tO.cpu().numpy()[b * n:][:n], r.order) and W[b] == oc.to_words(r.W[None, :])[0, 0], b
        word = oc.from_words(W[b: b + 1, None], n)[0]
        y = stacked[b][k]
        assert int(word.sum()) == r.best >> 40 <= DEC_WT and _in_row_space(stacked[b][:k], word ^ y), b


# ---- the chain, captured ----------------------------------------------------------------------------------------------------------------------

def test_chain_from_one_captured_graph_replayed_twice():
    """orders -> form -> search as plain launches on the stream they are given: during the capture nothing runs (the outputs keep their
    dirt); each replay starts from the same stacked matrices, so both give the same.  One stream: a single chain, no parallel branches."""
    stacked, _forms, refs = _decoding()
    k, n, batch = DEC_K, DEC_N, DEC_MEMBERS
    tA = torch.from_numpy(np.concatenate([oc.to_words(A).reshape(-1) for A in stacked]).view(np.int64)).cuda()
    tD, tO = torch.zeros_like(tA), torch.full((batch * n,), -7, dtype=torch.int32, device="cuda")
    tr, tp = torch.full((batch,), -7, dtype=torch.int32, device="cuda"), torch.full((batch * k,), -7, dtype=torch.int32, device="cuda")
    tB, tW = torch.full((batch,), -7, dtype=torch.int64, device="cuda"), torch.zeros((batch,), dtype=torch.int64, device="cuda")
    tU = torch.full((batch,), -7, dtype=torch.int32, device="cuda")

    def launch(stream):
        m4ri_amd.random_orders_batch_dev(tO.data_ptr(), n, n, batch, DEC_SEED, stream)
        m4ri_amd.echelonize_order_batch_dev(tD.data_ptr(), 1, k + 1, tA.data_ptr(), 1, k + 1, k + 1, n, k, tO.data_ptr(), n, n, batch, 1, tr.data_ptr(),
                                            tp.data_ptr(), stream)
        m4ri_amd.isd_search_dev(tD.data_ptr(), 1, k + 1, k + 1, n, k, tp.data_ptr(), tr.data_ptr(), batch, DEC_ITERS, 1, DEC_SEED, 1, 0, DEC_WT, tB.data_ptr(),
                                tO.data_ptr(), n, n, 0, tU.data_ptr(), 0, tW.data_ptr(), 1, stream)

    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        launch(torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert bool((tB == -7).all()) and bool((tU == -7).all()) and bool((tO == -7).all()) and bool((tr == -7).all())
    for _ in range(2):
        g.replay()
        torch.cuda.synchronize()
        assert tB.cpu().tolist() == [r.best for r in refs] and tU.cpu().tolist() == [r.iters_run for r in refs]
        assert np.array_equal(tW.cpu().numpy().view(np.uint64), np.array([oc.to_words(r.W[None, :])[0, 0] for r in refs], dtype=np.uint64))
        assert np.array_equal(tD.cpu().numpy().view(np.uint64).reshape(batch, k + 1), np.stack([oc.to_words(r.bits)[:, 0] for r in refs]))
        tB.fill_(-7)
        tU.fill_(-7)
        torch.cuda.synchronize()
