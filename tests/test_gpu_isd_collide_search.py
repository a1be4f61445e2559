"""m4ri_amd_isd_collide_search_dev (include/m4ri_amd.h, isd_collide_search_batch.hip) on the device: every output -- ALL words of D's
image, the dirty padding words, tail bits and gaps between members included, pivots, order, best, best_iter, iters_run, done and the
image of W with the entries around them -- against the NumPy rule of tests/isd_collide_cases.py (pinned to the rules it composes by
tests/test_isd_collide_search_plan.py), at the routed workgroup size and again at one wave and at 1024 threads with identical bytes;
against the two-call loop of the library itself; a decoding end to end; and the chain from one captured graph."""
from functools import lru_cache
from math import comb

import numpy as np
import pytest
import torch

import collide_cases as cc
import isd_collide_cases as icc
import m4ri_amd
import order_cases as oc
import rowsums_cases as rc

pytestmark = pytest.mark.gpu
THREADS = "M4RI_AMD_ISD_COLLIDE_SEARCH_THREADS"
# (nrows, ncols, pivot_rows): the row behind pivot_rows is the received word, further rows follow
SHAPES = [(9, 17, 8), (33, 64, 32), (17, 65, 16), (65, 128, 64), (20, 130, 16), (40, 300, 36), (66, 64, 0), (32, 64, 32)]
KINDS = ("full", "deficient", "full", "refused", "full")
ALL = (True, True, True, True)        # best_iter, iters_run, done, W wanted
SEARCH, PLAN = m4ri_amd.isd_collide_search_dev, m4ri_amd.plan_isd_collide_search     # what this module is about


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


@lru_cache(maxsize=None)
def _states(m, n, k, batch, kinds, seed):
    """The members of a shape, made once: the eliminations in NumPy are what takes the time."""
    rng = np.random.default_rng(seed)
    return tuple(_state(rng, m, n, k, kinds[b % len(kinds)]) for b in range(batch))


def _ell_for(n1, n2, room):
    """A window that leaves a few hundred colliding pairs of the N1 * N2: the rule weighs them all in NumPy."""
    return max(0, min(room, 64, (n1 * n2).bit_length() - 8))


class Case:
    """The host side of one call: images and what has to come back.  Built once per argument tuple (the workgroup sizes and the output
    combinations share it).  w_stop: a number, "first" (the weight member 0 has at iteration 0: it stops there) or "mid" (the weight
    member 0's best has reached at iteration iters // 2: the members stop at different iterations).  olen: the entries of the order kept
    (None: all ncols; 0: no order, ell = 0).  spoil: (member, position, value) written into that member's order before the call.
    states: the members, instead of random ones."""

    def __init__(self, m, n, k, k1, t1, t2, ell, batch, iters, steps, w_min, w_stop, seed, kinds=("full",), olen=None, call_seed=0, tight=False, spoil=(),
                 states=None):
        rng = np.random.default_rng(seed)
        self.m, self.n, self.k, self.batch, self.iters, self.steps, self.w_min, self.seed = m, n, k, batch, iters, steps, w_min, call_seed
        self.split = (k1, t1, t2, ell)
        self.pm = pm = min(k, n)
        self.width = width = (n + 63) // 64
        self.d_stride = width if tight else width + 2
        self.d_bs = m * self.d_stride if tight else (m * self.d_stride + 5) | 1
        self.w_bs = width if tight else width + 1
        self.states = states = list(states) if states is not None else list(_states(m, n, k, batch, tuple(kinds), seed))
        self.olen = olen = n if olen is None else olen
        orders = [np.array(s[3][:olen], dtype=np.int32) if olen else None for s in states]
        for (b, at, value) in spoil:
            orders[b][at] = value
        self.orders = orders
        search = lambda b, stop: icc.search(states[b][0], states[b][1], states[b][2], k, iters, steps, call_seed, k1, t1, t2, ell, w_min, stop, b=b, order=orders[b])
        if w_stop in ("first", "mid"):
            upto = search(0, -1).keys[: 1 if w_stop == "first" else iters // 2 + 1]
            w_stop = min([key >> 40 for key in upto if key >= 0], default=-1)
        self.w_stop = w_stop
        self.ref = [search(b, w_stop) for b in range(batch)]
        self.D, idx, valid = oc.pack([s[0] for s in states], m, n, self.d_stride, self.d_bs, seed + 1)
        self.P = np.concatenate([s[1] for s in states] + [np.full(2, -7, dtype=np.int32)]).astype(np.int32)
        self.R = np.array([s[2] for s in states] + [-7, -7], dtype=np.int32)
        self.o_bs = olen + 3 if olen else 0
        self.O = None
        if olen:
            self.O = np.full((batch - 1) * self.o_bs + olen + 4, -(1 << 31), dtype=np.int32)
            for b, o in enumerate(orders):
                self.O[b * self.o_bs: b * self.o_bs + olen] = o
        self.W = rng.integers(0, 1 << 63, size=(batch - 1) * self.w_bs + width + 3, dtype=np.int64).view(np.uint64) * np.uint64(3)
        # what has to come back
        self.want_D, self.want_P, self.want_O, self.want_W = self.D.copy(), self.P.copy(), None if self.O is None else self.O.copy(), self.W.copy()
        self.want = {name: np.full(batch + 2, -7, dtype=np.int64 if name == "best" else np.int32) for name in ("best", "best_iter", "iters_run", "done")}
        for b, r in enumerate(self.ref):
            oc.put(self.want_D, idx, valid, b, r.bits)
            self.want_P[b * pm: (b + 1) * pm] = r.pivots
            if olen:
                self.want_O[b * self.o_bs: b * self.o_bs + olen] = r.order
            for name in self.want:
                if iters > 0 or name in ("best", "iters_run"):      # a call of no iteration touches nothing else
                    self.want[name][b] = getattr(r, name)
            if r.best >= 0:
                at = slice(b * self.w_bs, b * self.w_bs + width)
                self.want_W[at] = (self.W[at] & ~valid) | (oc.to_words(r.W[None, :])[0] & valid)

    def run(self, outs=ALL, ints=True, stream=0):
        """The call on fresh copies of the images; every byte that came back, after it was compared.  outs: which of best_iter,
        iters_run, done and W are wanted; ints: pivots and rank passed (they may be absent where no exchange can happen)."""
        k1, t1, t2, ell = self.split
        tD = torch.from_numpy(self.D.view(np.int64).copy()).cuda()
        tP, tR = torch.from_numpy(self.P.copy()).cuda(), torch.from_numpy(self.R.copy()).cuda()
        tO = None if self.O is None else torch.from_numpy(self.O.copy()).cuda()
        tW = torch.from_numpy(self.W.view(np.int64).copy()).cuda()
        tB = torch.full((self.batch + 2,), -7, dtype=torch.int64, device="cuda")
        tI, tU, tN = (torch.full((self.batch + 2,), -7, dtype=torch.int32, device="cuda") for _ in range(3))
        torch.cuda.synchronize()
        SEARCH(tD.data_ptr(), self.d_stride, self.d_bs, self.m, self.n, self.k, tP.data_ptr() if ints else 0, tR.data_ptr() if ints else 0, self.batch,
               self.iters, self.steps, self.seed, k1, t1, t2, ell, self.w_min, self.w_stop, tB.data_ptr(), 0 if tO is None else tO.data_ptr(), self.o_bs,
               self.olen, tI.data_ptr() if outs[0] else 0, tU.data_ptr() if outs[1] else 0, tN.data_ptr() if outs[2] else 0,
               tW.data_ptr() if outs[3] else 0, self.w_bs, stream)
        torch.cuda.synchronize()
        got = [tD.cpu().numpy().view(np.uint64), tP.cpu().numpy(), tR.cpu().numpy(), None if tO is None else tO.cpu().numpy(), tB.cpu().numpy(),
               tI.cpu().numpy(), tU.cpu().numpy(), tN.cpu().numpy(), tW.cpu().numpy().view(np.uint64)]
        assert np.array_equal(got[4], self.want["best"]), ("best", got[4], self.want["best"], [r.keys for r in self.ref])
        wrong = np.flatnonzero(got[0] != self.want_D)
        assert wrong.size == 0, f"{wrong.size} words of D differ, first at {wrong[:5]} (d_bs {self.d_bs}, d_stride {self.d_stride})"
        assert np.array_equal(got[1], self.want_P), "pivots"
        assert np.array_equal(got[2], self.R), "rank was written"
        if tO is not None:
            assert np.array_equal(got[3], self.want_O), "order"
        untouched = np.full(self.batch + 2, -7, dtype=np.int32)
        for at, name, wanted in ((5, "best_iter", outs[0]), (6, "iters_run", outs[1]), (7, "done", outs[2])):
            assert np.array_equal(got[at], self.want[name] if wanted else untouched), (name, got[at], self.want[name])
        assert np.array_equal(got[8], self.want_W if outs[3] else self.W), "W"
        return got


@lru_cache(maxsize=None)
def _case(*args, **kw):
    return Case(*args, **kw)


def _every_size(monkeypatch, c, outs=ALL, ints=True):
    """The routed workgroup size, then one wave and 1024 threads: the three leave identical bytes."""
    monkeypatch.delenv(THREADS, raising=False)
    got = c.run(outs, ints)
    for threads in ("64", "1024"):
        monkeypatch.setenv(THREADS, threads)
        forced = c.run(outs, ints)
        assert all(np.array_equal(x, y) for x, y in zip(got, forced) if x is not None), threads
    monkeypatch.delenv(THREADS, raising=False)
    return got


# ---- shapes and splits --------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("m,n,k", SHAPES)
@pytest.mark.parametrize("t1,t2", [(a, b) for a in range(4) for b in range(4)])
def test_shapes_and_splits(monkeypatch, m, n, k, t1, t2):
    """Every split k1 of {0, 1, k / 2, k - 1, k} at every (t1, t2), the pairs with t1 > k1 or t2 > k - k1 included (no pairs: best -1);
    iterations 1 .. 5 and steps 0, 1, 3 go round with the split."""
    assert PLAN(m, n, k, 0, t1, t2, 0) == 1
    for i, k1 in enumerate(sorted({0, min(1, k), k // 2, max(k - 1, 0), k})):
        n1, n2 = comb(k1, t1), comb(k - k1, t2)
        ell = _ell_for(n1, n2, n - k)
        if n1 > 8192:                       # C(64, 3) left sums: refused, as tests/test_isd_collide_search_plan.py has it
            assert (m, t1) == (65, 3) and k1 >= 63 and PLAN(m, n, k, k1, t1, t2, ell) == 2
            continue
        base = 1000 * m + 10 * n + 4 * t1 + t2
        c = _case(m, n, k, k1, t1, t2, ell, 5, 1 + (i + t1 + t2) % 5, (0, 1, 3)[(i + t2) % 3], (i + t1) % 2, -1 if i % 2 else "mid", base, kinds=KINDS,
                  call_seed=base + 50 + i)
        _every_size(monkeypatch, c)
        if n1 * n2 == 0:
            assert all(r.best == -1 and r.W is None and r.iters_run == c.iters for r in c.ref)


# ---- the table ------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("side", [63, 64, 65, 255, 256, 257])
@pytest.mark.parametrize("swapped", [False, True])
def test_table_sizes(monkeypatch, side, swapped):
    """N1 (swapped: N2) on both sides of a wave and of a small workgroup: t = 1 with that many rows in the half, 8 rows in the other."""
    k = side + 8
    k1 = 8 if swapped else side
    c = _case(k + 1, 300, k, k1, 1, 1, 7, 5, 2, 3, 1, -1, 7000 + side, kinds=KINDS, call_seed=side + swapped)
    assert (comb(k1, 1), comb(k - k1, 1)) == ((8, side) if swapped else (side, 8)) and any(r.best >= 0 for r in c.ref) and sum(r.done for r in c.ref) > 0
    _every_size(monkeypatch, c)


def test_the_largest_table(monkeypatch):
    """N1 = C(128, 2) = 8128 entries on q = 13 bucket bits, two iterations."""
    c = _case(137, 200, 136, 128, 2, 1, 14, 5, 2, 3, 1, -1, 8128, kinds=KINDS, call_seed=3)
    assert PLAN(137, 200, 136, 128, 2, 1, 14) == 1 and any(r.best >= 0 for r in c.ref) and sum(r.done for r in c.ref) > 0
    _every_size(monkeypatch, c)


# ---- the window -----------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("m,n,k", [(17, 100, 16), (17, 130, 16)])
@pytest.mark.parametrize("ell", [0, 1, 7, 63, 64])
def test_window_lengths_on_a_shuffled_order(monkeypatch, m, n, k, ell):
    """The window entries of a random order span both (all three) words of a row.  N1 = 8: q = 3 < ell from 7 on, q = ell at 0 and 1."""
    c = _case(m, n, k, 8, 1, 1, ell, 5, 4, 3, 0, -1, 50 * n + ell, kinds=KINDS, call_seed=ell)
    if ell >= 63:
        assert {int(e) >> 6 for o in c.orders for e in o[k: k + ell]} == set(range((n + 63) // 64))
    _every_size(monkeypatch, c)
    if ell <= 1:
        assert all(r.best >= 0 for r in c.ref)


def _closed_form_states(k, z, ell, rng, kind):
    """Five members [I_k | I_k | 0_z] (kind "doubled") or rowsums_cases.rigged (kind "rigged", no zero columns) in reduced form on the
    identity columns, a follower stacked under each, and an order whose window starts in the zero columns and goes on in the second
    identity: the low bits of every row key agree (one bucket), the bits above tell the rows apart."""
    n = 2 * k + z
    out = []
    for b in range(5):
        if kind == "doubled":
            G = cc.doubled_identity_zeros(k, z)
            ident = min(ell - min(ell, 3), k - 4 - b % 3)                     # rows outside the window are left for the pairs
            low = ell - ident                                                 # zero columns first, at least three: the bucket bits
            assert 3 <= low <= z
            win = list(range(2 * k, 2 * k + low)) + [k + int(j) for j in rng.permutation(k)[:ident]]
        else:
            a, bb, c = 1, 2 + b % 2, k - 1 - b
            G = rc.rigged(k, a, bb, c)
            win = cc.rigged_window(k, a, bb)
        V = np.zeros(n, dtype=np.uint8)
        V[: 2 * k] = rng.integers(0, 2, size=2 * k, dtype=np.uint8)
        V[:k] = 0                                                             # reduced on the pivot columns
        if kind == "doubled":
            V[k: 2 * k] = 0
            left, right = [c for c in win if k <= c < k + k // 2], [c for c in win if k + k // 2 <= c < 2 * k]
            V[left[:1] + right[:1]] = 1                                       # a row of each half has to be in the pair for it to collide
        rest = [c for c in range(k, n) if c not in win]
        order = np.array(list(range(k)) + win + rest, dtype=np.int32)
        out.append((np.concatenate([G, V[None, :]]), np.arange(k, dtype=np.int32), k, order))
    return out


@pytest.mark.parametrize("k,z,k1,t1,t2,ell", [(16, 70, 8, 1, 1, 7), (16, 70, 8, 1, 1, 63), (16, 70, 8, 1, 1, 64), (16, 70, 8, 2, 1, 64), (20, 5, 10, 2, 2, 9)])
def test_keys_that_agree_on_the_bucket_bits(monkeypatch, k, z, k1, t1, t2, ell):
    states = _closed_form_states(k, z, ell, np.random.default_rng(k + ell), "doubled")
    for steps in (0, 2):
        c = Case(k + 1, 2 * k + z, k, k1, t1, t2, ell, 5, 3, steps, 0, -1, 600 + ell, call_seed=ell + steps, states=states)
        assert all(r.keys[0] >= 0 for r in c.ref), [r.keys for r in c.ref]
        _every_size(monkeypatch, c)


def test_rigged_members(monkeypatch):
    k = 12
    states = _closed_form_states(k, 0, 2, np.random.default_rng(12), "rigged")
    for (t1, t2) in ((1, 1), (2, 1), (2, 2)):
        c = Case(k + 1, 2 * k, k, 6, t1, t2, 2, 5, 4, 1, 1, -1, 700 + t1, call_seed=t1 + t2, states=states)
        _every_size(monkeypatch, c)
        # without the follower the first key is the closed form
        G = states[0][0][:k]
        free = Case(k, 2 * k, k, 6, t1, t2, 2, 1, 1, 0, 1, -1, 701, states=[(G, states[0][1], k, states[0][3])])
        assert free.ref[0].keys[0] == cc.rigged_expect(k, 1, 2, k - 1, 6, t1, t2, 1)[1]
        free.run()


@pytest.mark.parametrize("m,n,k,ell", [(9, 17, 8, 4), (17, 65, 16, 5), (20, 130, 16, 7)])
def test_an_order_of_exactly_the_pivots_and_the_window(monkeypatch, m, n, k, ell):
    """olen = pivot_rows + ell: a column exchanged in from outside the order leaves the order as it is."""
    c = _case(m, n, k, k // 2, 1, 1, ell, 5, 5, 3, 0, -1, 30 * n + ell, kinds=KINDS, olen=k + ell, call_seed=11)
    assert sum(r.done for r in c.ref) > 0 and any(not np.array_equal(r.order, o) for r, o in zip(c.ref, c.orders))
    assert any(sorted(r.order.tolist()) == sorted(o.tolist()) and r.done > 0 for r, o in zip(c.ref, c.orders))
    _every_size(monkeypatch, c)


@pytest.mark.parametrize("m,n,k", [(9, 17, 8), (20, 130, 16)])
@pytest.mark.parametrize("bad", ["ncols", -1])
def test_a_window_entry_outside_refuses_one_member_of_five(monkeypatch, m, n, k, bad):
    value = n if bad == "ncols" else -1
    c = _case(m, n, k, k // 2, 1, 1, 3, 5, 4, 3, 0, -1, 40 * n, spoil=((2, k + 1, value),), call_seed=5)
    assert c.ref[2].keys == [-2] * 4 and c.ref[2].best == -1 and c.ref[2].done > 0 and c.ref[2].W is None
    assert any(r.best >= 0 for b, r in enumerate(c.ref) if b != 2) and all(-2 not in r.keys for b, r in enumerate(c.ref) if b != 2)
    _every_size(monkeypatch, c)
    # a bad entry behind the window that no exchange brings in: steps = 0
    c = _case(m, n, k, k // 2, 1, 1, 3, 5, 4, 0, 0, -1, 40 * n + 1, spoil=((2, n - 1, value),), call_seed=5)
    assert any(r.best >= 0 for r in c.ref) and all(-2 not in r.keys for r in c.ref)
    _every_size(monkeypatch, c)


# ---- the loop parameters --------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("m,n,k", [(9, 17, 8), (17, 65, 16)])
@pytest.mark.parametrize("iters", [1, 2, 5, 40])
@pytest.mark.parametrize("steps", [0, 1, 3])
def test_loop_parameters(monkeypatch, m, n, k, iters, steps):
    """Every stop (at iteration 0, in the middle, never) with every w_min (0, 1, above every weight), members of every kind that stop at
    different iterations within one batch, an order kept whole and kept short."""
    stops = set()
    for i, w_stop in enumerate(("first", "mid", -1)):
        for j, w_min in enumerate((0, 1, n + 1)):
            c = _case(m, n, k, k // 2, 1, 1, 2, 5, iters, steps, w_min, w_stop, 100 * iters + 10 * steps + 3 * i + j, kinds=KINDS,
                      olen=None if (i + j) % 2 == 0 else k + 2, call_seed=iters + steps + i + j)
            monkeypatch.delenv(THREADS, raising=False)
            c.run()
            if w_min == n + 1:
                assert all(r.best == -1 and r.iters_run == iters for r in c.ref)
            elif w_stop == "first" and c.ref[0].keys[0] >= 0:
                assert c.ref[0].iters_run == 1
            stops.add(tuple(r.iters_run for r in c.ref))
    if iters == 40 and steps:
        assert any(len(set(s)) >= 3 for s in stops)          # members that stop at different iterations within one batch


def test_ties_go_to_the_earliest_iteration():
    """40 iterations on small members: the best weight is reached again later, and best_iter stays the first."""
    c = _case(9, 17, 8, 4, 1, 1, 2, 5, 40, 1, 1, -1, 4040, kinds=KINDS, call_seed=40)
    tied = 0
    for r in c.ref:
        weights = [key >> 40 for key in r.keys if key >= 0]
        tied += bool(weights) and weights.count(min(weights)) > 1
    assert tied > 0
    c.run()


@pytest.mark.parametrize("m,n,k", [(33, 64, 32), (20, 130, 16)])
def test_every_combination_of_the_optional_outputs(monkeypatch, m, n, k):
    monkeypatch.delenv(THREADS, raising=False)
    c = _case(m, n, k, k // 2, 1, 1, 3, 4, 6, 2, 1, "mid", 5 * m + n, kinds=("full", "deficient"), call_seed=17)
    for mask in range(16):
        c.run(outs=tuple(bool(mask >> i & 1) for i in range(4)))


@pytest.mark.parametrize("m,n,k", [(9, 17, 8), (17, 65, 16)])
def test_pivots_rank_and_order_may_be_absent(monkeypatch, m, n, k):
    _every_size(monkeypatch, _case(m, n, k, k // 2, 1, 1, 3, 3, 1, 3, 1, -1, 40 + m), ints=False)                 # one iteration
    _every_size(monkeypatch, _case(m, n, k, k // 2, 1, 1, 3, 3, 7, 0, 1, -1, 41 + m), ints=False)                 # no steps
    _every_size(monkeypatch, _case(m, n, k, k // 2, 2, 1, 0, 5, 5, 3, 1, -1, 42 + m, kinds=KINDS, olen=0))        # no window: no order needed


def test_no_iteration_and_no_columns():
    """iters = 0: best -1 and iters_run 0, nothing else touched.  ncols = 0: every pair collides and weighs 0, nothing is exchanged."""
    tB = torch.full((5,), -7, dtype=torch.int64, device="cuda")
    tI, tU, tN = (torch.full((5,), -7, dtype=torch.int32, device="cuda") for _ in range(3))
    c = _case(9, 17, 8, 4, 1, 1, 2, 3, 0, 2, 1, -1, 9)
    assert all(r.best == -1 and r.iters_run == 0 for r in c.ref)
    got = c.run()
    assert got[5][:3].tolist() == [-7] * 3 and got[7][:3].tolist() == [-7] * 3        # best_iter and done of a call without iterations
    # 4 x 0 with three pivot rows split 2 + 1
    for (t1, t2, w_min, w_stop, want) in [(0, 0, 0, -1, (0, 0, 6, 0)), (1, 1, 0, 0, (0, 0, 1, 0)), (1, 1, 1, 0, (-1, -1, 6, 0)), (3, 1, 0, 3, (-1, -1, 6, 0)),
                                          (1, 2, 0, 3, (-1, -1, 6, 0))]:
        for x in (tB, tI, tU, tN):
            x.fill_(-7)
        SEARCH(0, 0, 0, 4, 0, 3, 0, 0, 3, 6, 2, 5, 2, t1, t2, 0, w_min, w_stop, tB.data_ptr(), best_iter=tI.data_ptr(), iters_run=tU.data_ptr(), done=tN.data_ptr())
        torch.cuda.synchronize()
        for x, v in zip((tB, tI, tU, tN), want):
            assert x.cpu().tolist() == [v] * 3 + [-7] * 2, (t1, t2, w_min, w_stop)


def test_operands_packed_back_to_back(monkeypatch):
    """The accepted neighbours of the overlap checks, on the device: D's members with no word between them, then best and W in the same
    allocation; pivots, rank, order, best_iter, iters_run and done in one allocation with nothing between them."""
    for (m, n, k) in ((33, 64, 32), (20, 130, 16)):
        monkeypatch.delenv(THREADS, raising=False)
        c = _case(m, n, k, k // 2, 1, 1, 3, 3, 6, 2, 1, -1, 80 + m, tight=True, call_seed=5)
        batch, pm, nD = 3, c.pm, 3 * m * c.width
        nO = (batch - 1) * c.o_bs + n
        tL = torch.from_numpy(np.concatenate([c.D[:nD], np.full(batch, 7, dtype=np.uint64), c.W[: batch * c.width]]).view(np.int64)).cuda()
        tS = torch.from_numpy(np.concatenate([c.P[: batch * pm], c.R[:batch], c.O[:nO], np.full(3 * batch, -7, dtype=np.int32)])).cuda()
        at = tS.data_ptr() + 4 * np.cumsum([0, batch * pm, batch, nO, batch, batch])
        SEARCH(tL.data_ptr(), c.d_stride, c.d_bs, m, n, k, int(at[0]), int(at[1]), batch, c.iters, c.steps, c.seed, *c.split, c.w_min, c.w_stop,
               tL.data_ptr() + 8 * nD, int(at[2]), c.o_bs, n, int(at[3]), int(at[4]), int(at[5]), tL.data_ptr() + 8 * (nD + batch), c.w_bs)
        torch.cuda.synchronize()
        want_L = np.concatenate([c.want_D[:nD], c.want["best"][:batch].view(np.uint64), c.want_W[: batch * c.width]])
        want_S = np.concatenate([c.want_P[: batch * pm], c.R[:batch], c.want_O[:nO], c.want["best_iter"][:batch], c.want["iters_run"][:batch],
                                 c.want["done"][:batch]])
        assert np.array_equal(tL.cpu().numpy().view(np.uint64), want_L) and np.array_equal(tS.cpu().numpy(), want_S)
        assert sum(r.done for r in c.ref) > 0


# ---- against the library itself --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("m,n,k", [(33, 64, 32), (64, 64, 64), (65, 128, 64), (40, 300, 36)])
@pytest.mark.parametrize("t1,t2", [(1, 1), (2, 1)])
def test_the_two_call_loop_gives_the_same(monkeypatch, m, n, k, t1, t2):
    """w_stop = -1: a host loop of pivot_exchange_batch_dev(seed = isd_iteration_seed(seed, it)) and row_sums_collide_batch_dev(cols =
    order + k, lightest only) over the same members leaves the same D, pivots and order bit for bit, and the lightest of its keys (the
    earliest among equal weights) is best."""
    monkeypatch.delenv(THREADS, raising=False)
    iters, seed, batch, steps, k1 = 6, 77, 8, 2, k // 2
    ell = min(n - k, 3 + t1)
    c = _case(m, n, k, k1, t1, t2, ell, batch, iters, steps, 1, -1, 3 * m + n, kinds=("full", "full", "deficient", "refused"), call_seed=seed)
    got = c.run()
    tD = torch.from_numpy(c.D.view(np.int64).copy()).cuda()
    tP, tR, tO = torch.from_numpy(c.P.copy()).cuda(), torch.from_numpy(c.R.copy()).cuda(), torch.from_numpy(c.O.copy()).cuda()
    tL = torch.full((iters, batch), -7, dtype=torch.int64, device="cuda")
    V = tD.data_ptr() + 8 * k * c.d_stride if m > k else 0
    for it in range(iters):
        if it:
            m4ri_amd.pivot_exchange_batch_dev(tD.data_ptr(), c.d_stride, c.d_bs, m, n, k, tP.data_ptr(), tR.data_ptr(), batch, 0, 0, steps,
                                              m4ri_amd.isd_iteration_seed(seed, it), tO.data_ptr(), c.o_bs, n)
        m4ri_amd.lib().m4ri_amd_row_sums_collide_batch_dev(tD.data_ptr(), c.d_stride, c.d_bs, k, n, V or None, c.d_bs, batch, k1, t1, t2,
                                                           (tO.data_ptr() + 4 * k) if ell else None, c.o_bs, ell, 1, None, tL[it].data_ptr(), None)
    torch.cuda.synchronize()
    assert np.array_equal(tD.cpu().numpy().view(np.uint64), got[0]) and np.array_equal(tP.cpu().numpy(), got[1]) and np.array_equal(tO.cpu().numpy(), got[3])
    keys = tL.cpu().numpy()
    for b in range(batch):
        assert keys[:, b].tolist() == c.ref[b].keys, b
        weights = [(int(key) >> 40 if key >= 0 else 1 << 30) for key in keys[:, b]]
        first = weights.index(min(weights))
        assert got[4][b] == (keys[first, b] if keys[first, b] >= 0 else -1) and got[5][b] == (first if keys[first, b] >= 0 else -1), b


# ---- a decoding, end to end -------------------------------------------------------------------------------------------------------------------

DEC_K, DEC_N, DEC_MEMBERS, DEC_WT, DEC_ITERS = 32, 64, 32, 6, 400
DEC_K1, DEC_T1, DEC_T2, DEC_ELL = 16, 1, 1, 4
DEC_SEED = 2          # chosen on the CPU with the NumPy rule: it finds a word of weight <= 6 for every member within the 400 iterations
DEC_LONGEST = 283     # (seed 3 leaves four members unfound), and this is the largest iters_run among them


@lru_cache(maxsize=None)
def _decoding():
    """32 random 32 x 64 generators, y = a codeword + an error of weight 6 stacked under each; the forms on the random orders of seed
    DEC_SEED, and the rule's search on them (Stern, one row of each half, a window of four columns, one exchange per iteration)."""
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
        refs.append(icc.search(S, piv, rank, k, DEC_ITERS, 1, DEC_SEED, DEC_K1, DEC_T1, DEC_T2, DEC_ELL, 0, DEC_WT, b=b, order=order))
    return stacked, forms, refs


def _in_row_space(G, w):
    return oc.ech_order(np.concatenate([G, w[None, :]]), None, 1, G.shape[0] + 1)[1] == oc.ech_order(G, None, 1, G.shape[0])[1]


def _decode(tA, tD, tO, tr, tp, tB, tI, tU, tN, tW, stream=0):
    k, n, batch = DEC_K, DEC_N, DEC_MEMBERS
    m4ri_amd.random_orders_batch_dev(tO.data_ptr(), n, n, batch, DEC_SEED, stream)
    m4ri_amd.echelonize_order_batch_dev(tD.data_ptr(), 1, k + 1, tA.data_ptr(), 1, k + 1, k + 1, n, k, tO.data_ptr(), n, n, batch, 1, tr.data_ptr(), tp.data_ptr(),
                                        stream)
    SEARCH(tD.data_ptr(), 1, k + 1, k + 1, n, k, tp.data_ptr(), tr.data_ptr(), batch, DEC_ITERS, 1, DEC_SEED, DEC_K1, DEC_T1, DEC_T2, DEC_ELL, 0, DEC_WT,
           tB.data_ptr(), tO.data_ptr(), n, n, 0 if tI is None else tI.data_ptr(), tU.data_ptr(), 0 if tN is None else tN.data_ptr(), tW.data_ptr(), 1, stream)


def _decoding_buffers(stacked):
    k, n, batch = DEC_K, DEC_N, DEC_MEMBERS
    tA = torch.from_numpy(np.concatenate([oc.to_words(A).reshape(-1) for A in stacked]).view(np.int64)).cuda()
    tD, tO = torch.zeros_like(tA), torch.full((batch * n,), -7, dtype=torch.int32, device="cuda")
    tr, tp = torch.full((batch,), -7, dtype=torch.int32, device="cuda"), torch.full((batch * k,), -7, dtype=torch.int32, device="cuda")
    tB, tW = torch.full((batch,), -7, dtype=torch.int64, device="cuda"), torch.zeros((batch,), dtype=torch.int64, device="cuda")
    tI, tU, tN = (torch.full((batch,), -7, dtype=torch.int32, device="cuda") for _ in range(3))
    return tA, tD, tO, tr, tp, tB, tI, tU, tN, tW


def test_decoding_end_to_end(monkeypatch):
    monkeypatch.delenv(THREADS, raising=False)
    stacked, forms, refs = _decoding()
    k, n, batch = DEC_K, DEC_N, DEC_MEMBERS
    assert all(0 <= r.best >> 40 <= DEC_WT for r in refs) and max(r.iters_run for r in refs) == DEC_LONGEST      # the rule finds all 32
    tA, tD, tO, tr, tp, tB, tI, tU, tN, tW = bufs = _decoding_buffers(stacked)
    _decode(*bufs)
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

def test_chain_from_one_captured_graph_replayed_twice(monkeypatch):
    """orders -> form -> search as plain launches on the stream they are given: during the capture nothing runs (the outputs keep their
    dirt); each replay starts from the same stacked matrices, so both give the same.  One stream: a single chain, no parallel branches."""
    monkeypatch.delenv(THREADS, raising=False)
    stacked, _forms, refs = _decoding()
    k, n, batch = DEC_K, DEC_N, DEC_MEMBERS
    tA, tD, tO, tr, tp, tB, _tI, tU, _tN, tW = _decoding_buffers(stacked)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        _decode(tA, tD, tO, tr, tp, tB, None, tU, None, tW, torch.cuda.current_stream().cuda_stream)
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
