"""m4ri_amd_pivot_exchange_batch_dev (include/m4ri_amd.h, pivot_exchange_batch.hip) on the device: every output -- ALL words of D's
image, the dirty padding words, tail bits and gaps between members included, pivots, order and done with the entries around them --
against the NumPy rule of tests/exchange_cases.py (pinned to the elimination from scratch by tests/test_pivot_exchange_plan.py) on the
three paths of m4ri_amd_plan_pivot_exchange_batch, against m4ri_amd_echelonize_order_batch_dev from scratch on the new pivots bit for
bit, and the chain random orders -> echelon form -> exchange -> enumeration from one captured graph."""
from functools import lru_cache

import numpy as np
import pytest
import torch

import collide_cases as cc
import dev_frame as df
import exchange_cases as xc
import m4ri_amd
import order_cases as oc
import rowsums_cases as rc
from m4ri_amd.mzd import Mzd

pytestmark = pytest.mark.gpu
PATH0_MAX, PATH1_MAX = "M4RI_AMD_PIVOT_EXCHANGE_PATH0_MAX", "M4RI_AMD_PIVOT_EXCHANGE_PATH1_MAX"
I32_MIN, I32_MAX = -(1 << 31), (1 << 31) - 1
# (nrows, ncols, pivot_rows): the rows behind pivot_rows follow
SHAPES0 = [(1, 1, 1), (1, 2, 1), (5, 64, 5), (63, 64, 63), (64, 64, 64), (33, 64, 32)]
SHAPES12 = [(65, 65, 64), (70, 130, 60), (130, 257, 128)]
STEPS = (0, 1, 7, "more")      # "more": more steps than rows
ORDERS = ("perm", "null", "absent", "twice", "short")


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    assert m4ri_amd.lib().m4ri_amd_device_count() >= 1, "no HIP device visible: the gpu tests have nothing to run on"
    m4ri_amd.init(0)
    torch.cuda.set_device(0)


def _route(monkeypatch, path, m, n):
    """Send members of this shape down `path` at every step count: path 0 as the shape says, paths 1 and 2 by the overrides (read per
    call; the LDS bound, once set, decides alone between 1 and 2, so a call of one step can be held on path 1)."""
    monkeypatch.delenv(PATH0_MAX, raising=False)
    monkeypatch.delenv(PATH1_MAX, raising=False)
    natural = m4ri_amd.plan_pivot_exchange_batch(m, n, 2)
    assert natural <= path
    if path > natural:
        monkeypatch.setenv(PATH0_MAX, "0")
    if path > 0:
        monkeypatch.setenv(PATH1_MAX, "0" if path == 2 else "163840")


def _state(rng, m, n, pr, kind):
    """One member in the state echelonize_order_batch_dev(full = 1) leaves: (the matrix as it was, the form, pivots, rank, the order it
    was made on).  kind: "full" (as random bits fall), "deficient" (repeated pivot rows: rank < pivot_rows), "refused" (rank -1,
    pivots -1, D whatever it was), "bare" (a full member whose row 0 holds its pivot bit only)."""
    A = rng.integers(0, 2, size=(m, n), dtype=np.uint8)
    if kind == "deficient" and pr >= 2:
        A[pr // 2: pr] = A[: pr - pr // 2]
    order = rng.permutation(n).astype(np.int32)
    S, rank, piv = oc.ech_order(A, order, 1, pr)
    if kind == "refused":
        return A, A.copy(), np.full(min(pr, n), -1, dtype=np.int32), -1, order
    if kind == "bare" and rank:
        S[0] = 0
        S[0, piv[0]] = 1
        A = S.copy()
    return A, S, piv, rank, order


def _requests(rng, S, piv, rank, pr, steps):
    """A list of requests for this member, made along the rule: valid ones, the same row twice, the involution, and every kind of
    invalid request in the middle of them."""
    n = S.shape[1]
    R = min(max(rank, 0), len(piv))
    cur, cp, out, last, bad = S, piv, [], None, 0
    for s in range(steps):
        kind = ("valid", "valid", "same", "bad", "valid", "back", "bad", "valid")[s % 8] if R else "bad"
        if kind == "same" and last is not None:
            r = last[0]
            c = xc.scan(cur[r], int(cp[r]), int(rng.integers(0, n)))
            req = (r, int(cp[r]) if c is None else c)
        elif kind == "back" and last is not None:
            req = (last[0], last[1])                      # (r, old) of the last exchange performed
        elif kind == "bad":
            r = int(rng.integers(0, R)) if R else 0
            clear = np.flatnonzero(cur[r] == 0)
            other = [int(c) for c in cp[:R] if c != cp[r]]
            req = [(-1, 0), (R, 0), (r, -1), (r, n), (r, int(clear[0]) if clear.size else n), (r, int(cp[r])), (r, other[0] if other else n),
                   (I32_MIN, 0), (I32_MAX, 0), (r, I32_MIN), (r, I32_MAX), (len(piv), 0), (S.shape[0], 0)][bad % 13]
            bad += 1
        else:
            r = int(rng.integers(0, R))
            c = xc.scan(cur[r], int(cp[r]), int(rng.integers(0, n)))
            req = (r, int(cp[r]) if c is None else c)
        old = int(cp[req[0]]) if 0 <= req[0] < R else None
        cur, cp, _, did, _ = xc.exchange(cur, cp, rank, pr, 1, req=[req])
        if did:
            last = (req[0], old)
        out.append(req)
    return np.array(out, dtype=np.int32).reshape(steps, 2)


def _order(rng, kind, order, piv):
    """The entries kept for a member: the order its form was made on, or a variant of it; None: no order."""
    n = len(order)
    if kind == "null":
        return None
    o = order.copy()
    if kind == "absent" and n >= 2:      # a pivot column's value taken out: exchanges of that column leave the order as it is
        o[np.flatnonzero(o == (piv[0] if len(piv) and piv[0] >= 0 else 0))[0]] = n + 5
    if kind == "twice" and n >= 3:       # a value present twice: the first position counts
        o[n - 1] = o[0]
    if kind == "short":
        o = o[: n // 2]
    return o


class Case:
    """The host side of one call: images and what has to come back.  Built once per argument tuple (the paths share it)."""

    def __init__(self, m, n, pr, batch, steps, mode, okind, seed, kinds=("full",), shared_req=False, call_seed=0, done=True, tight=False):
        rng = np.random.default_rng(seed)
        self.m, self.n, self.pr, self.batch, self.steps, self.mode, self.seed = m, n, pr, batch, steps, mode, call_seed
        self.pm = pm = min(pr, n)
        width = (n + 63) // 64
        self.d_stride = width if tight else width + 2                     # a stride above the width
        self.d_bs = m * self.d_stride if tight else (m * self.d_stride + 5) | 1     # an odd batch stride
        if batch == 1:
            self.d_bs = 0
        states = [_state(rng, m, n, pr, kinds[b % len(kinds)]) for b in range(batch)]
        self.states = states
        self.D, idx, valid = oc.pack([S for (_A, S, _p, _r, _o) in states], m, n, self.d_stride, self.d_bs if batch > 1 else m * self.d_stride, seed + 1)
        self.P = np.concatenate([p for (_A, _S, p, _r, _o) in states] + [np.full(2, -7, dtype=np.int32)]).astype(np.int32)
        self.R = np.array([r for (_A, _S, _p, r, _o) in states] + [-7, -7], dtype=np.int32)
        # the requests: per member (an odd batch stride above 2 * steps) or one list for all, made along member 0
        self.shared_req = shared_req
        self.r_bs = 0 if shared_req or batch == 1 else 2 * steps + 1
        self.Q = None
        if mode == "list":
            lists = [_requests(rng, states[b][1], states[b][2], states[b][3], pr, steps) for b in range(1 if shared_req else batch)]
            self.Q = np.full((len(lists) - 1) * self.r_bs + 2 * steps + 3, I32_MAX, dtype=np.int32)
            for b, q in enumerate(lists):
                self.Q[b * self.r_bs: b * self.r_bs + 2 * steps] = q.reshape(-1)
        # the orders, member b's at b * o_bs
        orders = [_order(rng, okind, states[b][4], states[b][2]) for b in range(batch)]
        self.olen = 0 if orders[0] is None else len(orders[0])
        self.o_bs = self.olen + 3 if batch > 1 else 0
        self.O = None
        if orders[0] is not None:
            self.O = np.full((batch - 1) * self.o_bs + self.olen + 4, I32_MIN, dtype=np.int32)
            for b, o in enumerate(orders):
                self.O[b * self.o_bs: b * self.o_bs + self.olen] = o
        self.want_done = done
        # what has to come back
        self.want_D, self.want_P, self.want_O = self.D.copy(), self.P.copy(), None if self.O is None else self.O.copy()
        self.want_N = np.full(batch + 2, -7, dtype=np.int32)
        self.met = []
        for b, (_A, S, piv, rank, _o) in enumerate(states):
            req = None if self.Q is None else self.Q[b * self.r_bs:][: 2 * steps].reshape(steps, 2)
            S2, piv2, o2, did, met = xc.exchange(S, piv, rank, pr, steps, req=req, seed=call_seed, b=b, order=orders[b])
            self.met.append(met)
            oc.put(self.want_D, idx, valid, b, S2)
            self.want_P[b * pm: (b + 1) * pm] = piv2
            if o2 is not None:
                self.want_O[b * self.o_bs: b * self.o_bs + self.olen] = o2
            self.want_N[b] = did
        self.new_pivots = self.want_P[: batch * pm].reshape(batch, pm)

    def run(self, stream=0):
        tD = torch.from_numpy(self.D.view(np.int64).copy()).cuda()
        tP, tR = torch.from_numpy(self.P.copy()).cuda(), torch.from_numpy(self.R.copy()).cuda()
        tQ = None if self.Q is None else torch.from_numpy(self.Q.copy()).cuda()
        tO = None if self.O is None else torch.from_numpy(self.O.copy()).cuda()
        tN = torch.full((self.batch + 2,), -7, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        m4ri_amd.pivot_exchange_batch_dev(tD.data_ptr(), self.d_stride, self.d_bs, self.m, self.n, self.pr, tP.data_ptr(), tR.data_ptr(), self.batch,
                                          0 if tQ is None else tQ.data_ptr(), self.r_bs, self.steps, self.seed, 0 if tO is None else tO.data_ptr(),
                                          self.o_bs, self.olen, tN.data_ptr() if self.want_done else 0, stream)
        torch.cuda.synchronize()
        got = tD.cpu().numpy().view(np.uint64)
        wrong = np.flatnonzero(got != self.want_D)
        assert wrong.size == 0, f"{wrong.size} words of D differ, first at {wrong[:5]} (d_bs {self.d_bs}, d_stride {self.d_stride})"
        assert np.array_equal(tP.cpu().numpy(), self.want_P), "pivots"
        assert np.array_equal(tR.cpu().numpy(), self.R), "rank was written"
        if tQ is not None:
            assert np.array_equal(tQ.cpu().numpy(), self.Q), "req was written"
        if tO is not None:
            assert np.array_equal(tO.cpu().numpy(), self.want_O), "order"
        assert np.array_equal(tN.cpu().numpy(), self.want_N if self.want_done else np.full(self.batch + 2, -7)), "done"
        return tD, tP


@lru_cache(maxsize=None)
def _case(*args, **kw):
    return Case(*args, **kw)


def _steps(steps, m):
    return m + 9 if steps == "more" else steps


def _sweep(monkeypatch, path, m, n, pr, steps):
    """Requests from a list (per member and shared) and drawn on the device, every kind of order, members of full rank, deficient and
    refused, with and without done."""
    _route(monkeypatch, path, m, n)
    st, base = _steps(steps, m), 1000 * m + 10 * n + 3 * _steps(steps, m)
    kinds = ("full", "deficient", "full", "refused", "full")
    for i, okind in enumerate(ORDERS):
        _case(m, n, pr, 5, st, "list" if i % 2 == 0 else "random", okind, base + i, kinds=kinds, call_seed=base + 50 + i, done=i != 3).run()
    _case(m, n, pr, 3, st, "list", "perm", base + 7, shared_req=True).run()
    _case(m, n, pr, 1, st, "random", "perm", base + 8, call_seed=base).run()        # one member: batch strides of 0


@pytest.mark.parametrize("m,n,pr", SHAPES0)
@pytest.mark.parametrize("steps", STEPS)
def test_wave_path(monkeypatch, m, n, pr, steps):
    assert m4ri_amd.plan_pivot_exchange_batch(m, n, _steps(steps, m)) == 0
    _sweep(monkeypatch, 0, m, n, pr, steps)


@pytest.mark.parametrize("m,n,pr", SHAPES12)
@pytest.mark.parametrize("steps", STEPS)
def test_lds_path(monkeypatch, m, n, pr, steps):
    assert m4ri_amd.plan_pivot_exchange_batch(m, n, 7) == 1
    _sweep(monkeypatch, 1, m, n, pr, steps)


@pytest.mark.parametrize("m,n,pr", SHAPES12)
@pytest.mark.parametrize("steps", STEPS)
def test_global_path_by_override(monkeypatch, m, n, pr, steps):
    _sweep(monkeypatch, 2, m, n, pr, steps)


@pytest.mark.parametrize("path", [1, 2])
@pytest.mark.parametrize("m,n,pr", [(5, 64, 5), (33, 64, 32), (64, 64, 64)])
def test_small_members_on_the_workgroup_paths_by_override(monkeypatch, path, m, n, pr):
    _sweep(monkeypatch, path, m, n, pr, 7)


def test_global_path_natural_member(monkeypatch):
    """A member beyond LDS (words of more than one 64-word chunk of a wave's scan: 70 words): requests drawn on the device."""
    m, n = 300, 4500
    monkeypatch.delenv(PATH0_MAX, raising=False)
    monkeypatch.delenv(PATH1_MAX, raising=False)
    assert m4ri_amd.plan_pivot_exchange_batch(m, n, 4) == 2
    _case(m, n, 290, 2, 4, "random", "perm", 77, call_seed=5).run()


def test_one_step_in_place_by_the_plan(monkeypatch):
    """No override: a call of one step on a member that fits in LDS runs in place (path 2), two steps staged (path 1)."""
    monkeypatch.delenv(PATH0_MAX, raising=False)
    monkeypatch.delenv(PATH1_MAX, raising=False)
    assert [m4ri_amd.plan_pivot_exchange_batch(70, 130, s) for s in (1, 2)] == [2, 1]
    for steps in (1, 2):
        _case(70, 130, 60, 5, steps, "random", "perm", 90 + steps, kinds=("full", "deficient", "refused"), call_seed=3).run()


def test_lists_hold_every_kind_of_request():
    """What the sweeps run, looked at on the host: the lists have requests that are performed and requests of every invalid kind, the
    same row twice and the involution."""
    c = _case(70, 130, 60, 5, 79, "list", "perm", 1000 * 70 + 10 * 130 + 3 * 79, kinds=("full", "deficient", "full", "refused", "full"),
              call_seed=1000 * 70 + 10 * 130 + 3 * 79 + 50, done=True)
    q = c.Q[: 2 * 79].reshape(79, 2)
    assert (q[:, 0] < 0).any() and (q[:, 0] >= 60).any() and (q[:, 1] < 0).any() and (q[:, 1] >= 130).any()
    assert any((q[s, 0] == q[s + 1, 0]) for s in range(78)) and 0 < c.want_N[0] < 79
    assert c.want_N[3] == 0 and c.want_N[1] > 0 and c.R[1] < 60          # the refused member untouched, the deficient one exchanged


# ---- requests drawn on the device ---------------------------------------------------------------------------------------------------------

def _find(make, ok, seeds=range(400)):
    for s in seeds:
        c = make(s)
        if ok(c):
            return c
    raise AssertionError("no seed found")


@pytest.mark.parametrize("path,m,n,pr", [(0, 33, 64, 32), (1, 70, 130, 60), (2, 70, 130, 60), (1, 130, 257, 128)])
def test_a_scan_wraps_past_the_last_column(monkeypatch, path, m, n, pr):
    """Seeds chosen here so that some member's scan starts behind the last bit of its row and finds its column from column 0 on."""
    def wraps(c):
        return any(met is not None and met[1] < m4ri_amd.exchange_draw(c.seed, b, c.steps, s, c.states[b][3], n)[1]
                   for b in range(c.batch) for s, met in enumerate(c.met[b]))
    _route(monkeypatch, path, m, n)
    _find(lambda s: _case(m, n, pr, 4, 3, "random", "perm", 40 + m, call_seed=s), wraps).run()


@pytest.mark.parametrize("path,m,n,pr", [(0, 5, 64, 4), (1, 65, 65, 6), (2, 65, 65, 6)])
def test_a_row_holding_only_its_pivot_bit_is_skipped(monkeypatch, path, m, n, pr):
    _route(monkeypatch, path, m, n)
    c = _find(lambda s: _case(m, n, pr, 3, 7, "random", "perm", 50 + m, kinds=("bare",), call_seed=s),
              lambda c: any(None in met for met in c.met) and (c.want_N > 0).any())
    assert (c.want_N[:3] < 7).any()
    c.run()


@pytest.mark.parametrize("path,m,n", [(0, 5, 64), (0, 1, 2), (1, 65, 65), (2, 70, 130)])
def test_rank_one(monkeypatch, path, m, n):
    _route(monkeypatch, path, m, n)
    c = _case(m, n, 1, 4, 7, "random", "perm", 60 + m, call_seed=9)
    assert all(r <= 1 for r in c.R[:4])
    c.run()


# ---- the frame, the neighbours of the overlap checks, the tie to the elimination from scratch ----------------------------------------------

@pytest.mark.parametrize("layout", df.LAYOUTS)
@pytest.mark.parametrize("path,m,n,pr", [(0, 33, 64, 32), (1, 70, 130, 60), (2, 70, 130, 60)])
def test_framed_members(monkeypatch, layout, path, m, n, pr):
    """The batch as one tall operand of tests/dev_frame.py: members every m + 2 rows, the rows between them, the guard rows around, the
    padding words and the tail bits all come back as they were; the members' valid bits are the rule's."""
    _route(monkeypatch, path, m, n)
    batch, gap, steps = 3, 2, 7
    rng = np.random.default_rng(70 + m)
    states = [_state(rng, m, n, pr, "full") for _ in range(batch)]
    tall = rng.integers(0, 2, size=((batch - 1) * (m + gap) + m, n), dtype=np.uint8)
    want = tall.copy()
    P = np.concatenate([p for (_A, _S, p, _r, _o) in states]).astype(np.int32)
    for b, (_A, S, piv, rank, _o) in enumerate(states):
        tall[b * (m + gap): b * (m + gap) + m] = S
        want[b * (m + gap): b * (m + gap) + m] = xc.exchange(S, piv, rank, pr, steps, seed=3, b=b)[0]
    f = df.Frame(Mzd.from_bits(tall), layout, 71, dirty_tail=True).upload()
    tP, tR = torch.from_numpy(P).cuda(), torch.from_numpy(np.array([r for (_A, _S, _p, r, _o) in states], dtype=np.int32)).cuda()
    m4ri_amd.pivot_exchange_batch_dev(f.ptr, f.stride, (m + gap) * f.stride, m, n, pr, tP.data_ptr(), tR.data_ptr(), batch, steps=steps, seed=3)
    torch.cuda.synchronize()
    f.check(Mzd.from_bits(want), "kept", "D")
    assert not np.array_equal(want, tall)


def test_operands_packed_back_to_back(monkeypatch):
    """The accepted neighbours of the overlap checks, on the device: D's members with no word between them, and pivots, rank, req, order
    and done in one allocation with nothing between them."""
    for path, (m, n, pr) in ((0, (33, 64, 32)), (1, (70, 130, 60))):
        _route(monkeypatch, path, m, n)
        c = _case(m, n, pr, 3, 7, "list", "perm", 80 + m, tight=True)
        pm, batch = c.pm, 3
        ints = np.concatenate([c.P[: batch * pm], c.R[:batch], c.Q[: (batch - 1) * c.r_bs + 14], c.O[: (batch - 1) * c.o_bs + n], np.full(batch, -7, dtype=np.int32)])
        tI = torch.from_numpy(ints).cuda()
        tD = torch.from_numpy(c.D.view(np.int64).copy()).cuda()
        at = np.cumsum([0, batch * pm, batch, (batch - 1) * c.r_bs + 14, (batch - 1) * c.o_bs + n]) * 4 + tI.data_ptr()
        m4ri_amd.pivot_exchange_batch_dev(tD.data_ptr(), c.d_stride, c.d_bs, m, n, pr, int(at[0]), int(at[1]), batch, int(at[2]), c.r_bs, 7, 0, int(at[3]),
                                          c.o_bs, n, int(at[4]))
        torch.cuda.synchronize()
        want = np.concatenate([c.want_P[: batch * pm], c.R[:batch], c.Q[: (batch - 1) * c.r_bs + 14], c.want_O[: (batch - 1) * c.o_bs + n], c.want_N[:batch]])
        assert np.array_equal(tI.cpu().numpy(), want) and np.array_equal(tD.cpu().numpy().view(np.uint64), c.want_D)


@pytest.mark.parametrize("path,k,n", [(0, 32, 64), (1, 64, 130), (2, 64, 130), (1, 129, 257)])
def test_exchanged_form_is_the_elimination_from_scratch_on_the_new_pivots(monkeypatch, path, k, n):
    """Full-rank generators with a received word as follower: after the exchanges, D and pivots are what
    m4ri_amd_echelonize_order_batch_dev gives from the matrix as it was on order = the new pivots, bit for bit."""
    _route(monkeypatch, path, k + 1, n)
    batch, steps = 4, 16
    c = _find(lambda s: _case(k + 1, n, k, batch, steps, "random", "perm", s, call_seed=11, tight=True), lambda c: all(r == k for r in c.R[:batch]))
    tD, tP = c.run()
    assert (c.want_N[:batch] == steps).all()
    A = np.concatenate([oc.to_words(c.states[b][0]).reshape(-1) for b in range(batch)])
    tA = torch.from_numpy(A.view(np.int64)).cuda()
    t2 = torch.zeros_like(tA)
    r2 = torch.full((batch,), -7, dtype=torch.int32, device="cuda")
    p2 = torch.full((batch * k,), -7, dtype=torch.int32, device="cuda")
    w = (n + 63) // 64
    m4ri_amd.echelonize_order_batch_dev(t2.data_ptr(), w, (k + 1) * w, tA.data_ptr(), w, (k + 1) * w, k + 1, n, k, tP.data_ptr(), k, k, batch, 1,
                                        r2.data_ptr(), p2.data_ptr())
    torch.cuda.synchronize()
    assert (r2 == k).all() and torch.equal(p2, tP[: batch * k])
    mask = np.tile(oc.word_masks(n), batch * (k + 1))
    assert np.array_equal(t2.cpu().numpy().view(np.uint64), tD.cpu().numpy().view(np.uint64)[: mask.size] & mask)


# ---- the chain, captured -------------------------------------------------------------------------------------------------------------------

class Chain:
    """Information-set decoding without a host round trip for 32 members: random orders, systematic forms of one shared generator, eight
    exchanges drawn on the device with the order kept, then the lightest single row and sum of two rows, and Stern's collision step on
    the window cols = order + k."""
    K, N, MEMBERS, STEPS, ELL = 16, 64, 32, 8, 4

    def __init__(self):
        k, n = self.K, self.N
        self.G = Mzd.random(k, n, 1).to_bits()
        self.forms, self.orders, self.lightest, self.collide = [], [], [[], []], []
        for b in range(self.MEMBERS):
            order = oc.random_order(7, b, n)
            S, r, piv = oc.ech_order(self.G, order, 1, k)
            S, piv, order, did, _ = xc.exchange(S, piv, r, k, self.STEPS, seed=21, b=b, order=order)
            self.forms.append((S, piv, did))
            self.orders.append(order)
            for t in (1, 2):
                self.lightest[t - 1].append(rc.expect(S, None, t, 1)[1])
            self.collide.append(cc.expect(S, None, k // 2, 1, 1, order[k: k + self.ELL], 1)[1])
        self.tG = torch.from_numpy(Mzd.from_bits(self.G).valid_words().copy().view(np.int64).reshape(-1)).cuda()
        self.fresh()

    def fresh(self):
        k, n, batch = self.K, self.N, self.MEMBERS
        self.tO = torch.full((batch * n,), -7, dtype=torch.int32, device="cuda")
        self.tD = torch.full((batch * k,), -7, dtype=torch.int64, device="cuda")
        self.tr = torch.full((batch,), -7, dtype=torch.int32, device="cuda")
        self.tp = torch.full((batch * k,), -7, dtype=torch.int32, device="cuda")
        self.tn = torch.full((batch,), -7, dtype=torch.int32, device="cuda")
        self.tl = torch.full((3, batch), -7, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()

    def launch(self, stream=0):
        k, n, batch = self.K, self.N, self.MEMBERS
        m4ri_amd.random_orders_batch_dev(self.tO.data_ptr(), n, n, batch, 7, stream)
        m4ri_amd.echelonize_order_batch_dev(self.tD.data_ptr(), 1, k, self.tG.data_ptr(), 1, 0, k, n, k, self.tO.data_ptr(), n, n, batch, 1,
                                            self.tr.data_ptr(), self.tp.data_ptr(), stream)
        m4ri_amd.pivot_exchange_batch_dev(self.tD.data_ptr(), 1, k, k, n, k, self.tp.data_ptr(), self.tr.data_ptr(), batch, 0, 0, self.STEPS, 21,
                                          self.tO.data_ptr(), n, n, self.tn.data_ptr(), stream)
        for t in (1, 2):
            m4ri_amd.row_sums_weights_batch_dev(self.tD.data_ptr(), 1, k, k, n, 0, 0, batch, t, 1, 0, self.tl[t - 1].data_ptr(), stream)
        m4ri_amd.row_sums_collide_batch_dev(self.tD.data_ptr(), 1, k, k, n, 0, 0, batch, k // 2, 1, 1, self.tO.data_ptr() + 4 * k, n, self.ELL, 1, 0,
                                            self.tl[2].data_ptr(), stream)

    def untouched(self):
        return bool((self.tl == -7).all()) and bool((self.tr == -7).all()) and bool((self.tO == -7).all()) and bool((self.tn == -7).all())

    def check(self):
        k = self.K
        assert np.array_equal(self.tO.cpu().numpy().reshape(self.MEMBERS, self.N), np.stack(self.orders))
        D = self.tD.cpu().numpy().view(np.uint64).reshape(self.MEMBERS, k, 1)
        for b, (S, piv, did) in enumerate(self.forms):
            assert np.array_equal(D[b], oc.to_words(S)), b
            assert self.tn[b].item() == did and np.array_equal(self.tp.cpu().numpy()[b * k:][:k], piv), b
        assert self.tl.cpu().numpy().tolist() == [self.lightest[0], self.lightest[1], self.collide]


def test_chain_from_one_captured_graph_replayed_twice():
    """Plain launches on the stream they are given: during the capture nothing runs (the outputs keep their dirt); each replay makes
    the orders and the forms again from the shared generator, so both give the same.  One stream: a single chain, no parallel branches."""
    p = Chain()
    assert all(did == Chain.STEPS for (_S, _p, did) in p.forms) and sum(x >= 0 for x in p.collide) >= 8
    p.launch()
    torch.cuda.synchronize()
    p.check()
    p.fresh()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        p.launch(torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert p.untouched()
    for _ in range(2):
        g.replay()
        torch.cuda.synchronize()
        p.check()
