"""The shape sweep of the batched small-matrix calls (include/m4ri_amd.h: echelonize_batch, echelonize_order_batch, ple_batch,
solve_left_batch, inv_batch, kernel_left_batch, pluq_solve_left_batch, mul_small_batch, mul_small_batch_op, transpose_batch): every
shape up to 64 x 64 -- where each call runs a wave per member, lane i holding row i -- and the first shapes across that boundary, five
members per shape.  Plain NumPy plus the oracle library; no torch, no GPU.

A sweep is a list of Jobs.  A Job holds the host images of one arena per operand (the members of many shapes in one buffer, dirty
tail bits, padding words and gaps), what every buffer has to hold afterwards, and one launch per shape with its pointers given as
(buffer, offset).  tests/test_gpu_batch_shape_sweep.py uploads the images, issues the launches, downloads once and hands the buffers
to Job.failures; tests/test_sweep_cases_cpu.py pins what keeps the sweep from being hollow, on the oracle alone."""
from collections import namedtuple

import numpy as np

import order_cases as oc
from m4ri_amd.mzd import Mzd

BATCH = 5            # four waves of one workgroup and one member in a second workgroup, whose other three waves return
KINDS = ("random", "lowrank", "sparse", "zerocols", "halves", "perm", "ones")
SMALL = range(1, 65)
S0 = [(m, n) for m in SMALL for n in SMALL]
_B = (65, 66, 127, 128, 129)
_T = tuple(SMALL) + (65, 66, 127, 128, 129)
S1 = sorted({(b, t) for b in _B for t in _T} | {(t, b) for b in _B for t in _T})
SQUARES = list(range(1, 131))
I32_MAX = (1 << 31) - 1
NN, NT, TN, TT = (0, 0), (0, 1), (1, 0), (1, 1)


def rows_of(shapes):
    """The shapes grouped by their first size, ascending: one arena each."""
    out = {}
    for s in shapes:
        out.setdefault(s[0], []).append(s)
    return [out[m] for m in sorted(out)]


def _rng(*key):
    return np.random.default_rng(list(key))


# ---- the members ---------------------------------------------------------------------------------------------------------------------

def kind_of(m, n, b):
    """Member 0 of every shape is random -- the dense case, whose rank runs to the last row and column, at every shape --; the others
    take four of the remaining six kinds in a row, starting where m and n say."""
    return KINDS[0] if b % BATCH == 0 else KINDS[1 + (m + 2 * n + b) % (len(KINDS) - 1)]


def bits_of(kind, m, n, rng):
    """One m x n member of a kind that means something down to 1 x 1."""
    G = rng.integers(0, 2, size=(m, n), dtype=np.uint8)
    if kind == "lowrank":      # rank at most max(1, min(m, n) // 3)
        r = max(1, min(m, n) // 3)
        X, Y = rng.integers(0, 2, size=(m, r), dtype=np.int64), rng.integers(0, 2, size=(r, n), dtype=np.int64)
        G = ((X @ Y) & 1).astype(np.uint8)
    elif kind == "sparse":     # about two ones per column
        G = (rng.random((m, n)) * m < 2).astype(np.uint8)
    elif kind == "zerocols":   # a random third of the columns cleared, column 0 among them
        G[:, rng.permutation(n)[: n // 3]] = 0
        G[:, 0] = 0
    elif kind == "halves":     # the lower half of the rows a copy of the upper half
        G[m - m // 2:] = G[: m // 2]
    elif kind == "perm":       # a partial permutation matrix: every pivot far away, every column a swap
        mn = min(m, n)
        r = int(rng.integers((mn + 1) // 2, mn + 1))
        G[:] = 0
        G[rng.permutation(m)[:r], rng.permutation(n)[:r]] = 1
    elif kind == "ones":
        G[:] = 1
    return G


def member(m, n, b, salt=0):
    """Member b of shape (m, n): the kind rotates with m, n and b, the seed depends on (m, n, b) alone."""
    return bits_of(kind_of(m, n, b + salt), m, n, _rng(m, n, b, salt))


def members(m, n, salt=0):
    return np.stack([member(m, n, b, salt) for b in range(BATCH)])


def noise(m, n, salt):
    """BATCH random members: what an output buffer holds in its valid bits before the call."""
    return _rng(m, n, salt).integers(0, 2, size=(BATCH, m, n), dtype=np.uint8)


def to_words(bits):
    """batch x rows x cols bits -> batch x rows x words(cols) words"""
    b, r, c = bits.shape
    return oc.to_words(bits.reshape(b * r, c)).reshape(b, r, (c + 63) // 64)


def from_words(words, cols):
    b, r, w = words.shape
    return oc.from_words(words.reshape(b * r, w), cols).reshape(b, r, cols)


# ---- the schedules of the third size ------------------------------------------------------------------------------------------------

def k_of(m, n):
    """The right-hand sides of a solve: every value in 1 .. 64, and 64 for a quarter of the shapes."""
    return 64 if (m + n) % 4 == 0 else 1 + (5 * m + 3 * n) % 64


def kc_of(m, n):
    """The columns asked of a null space: 1, n, and a value in between."""
    c = (m + n) % 3
    return 1 if c == 0 else n if c == 1 else min(n, 2 + (3 * m + n) % max(1, n - 2))


def third(a, b):
    """The scheduled size of a product whose other two sizes are swept: every value in 1 .. 64 for every a."""
    return 1 + (5 * a + 3 * b) % 64


PLANES = ("ml", "ln", "mn")


def triple(plane, a, b):
    """(m, l, n) of the product at (a, b) of a plane."""
    c = third(a, b)
    return {"ml": (a, b, c), "ln": (c, a, b), "mn": (a, c, b)}[plane]


# ---- arenas -------------------------------------------------------------------------------------------------------------------------

class Block:
    """The `count` members of one shape in an arena: member b's row r at off + b * bs + r * stride."""

    def __init__(self, key, rows, cols, count, off, stride, bs):
        self.key, self.rows, self.cols, self.count, self.off, self.stride, self.bs = key, rows, cols, count, off, stride, bs
        self.idx = off + oc.index(rows, cols, count, stride, bs)
        self.valid = oc.word_masks(cols)
        self.end = off + (count - 1) * bs + rows * stride


class Arena:
    """One word buffer for the members of many shapes, laid out as tests/test_gpu_echelonize_batch._pack lays out one batch: rows
    `pad` words wider than their valid words, `gap` words between members, five words between shapes and at the end."""

    def __init__(self):
        self.blocks, self.size = [], 0

    def add(self, key, rows, cols, count=BATCH, pad=1, gap=3):
        stride = (cols + 63) // 64 + pad
        blk = Block(key, rows, cols, count, self.size, stride, rows * stride + gap)
        self.blocks.append(blk)
        self.size = blk.end + 5
        return blk

    def dirt(self, *seed):
        return _rng(*seed).integers(0, 1 << 63, size=self.size, dtype=np.int64).view(np.uint64) * np.uint64(3)

    def inside(self):
        """The mask of the members' valid bits; its complement is what no call may write."""
        mask = np.zeros(self.size, dtype=np.uint64)
        for blk in self.blocks:
            mask[blk.idx] = blk.valid
        return mask

    def offsets(self):
        return np.array([b.off for b in self.blocks], dtype=np.int64)

    def locate(self, j, i):
        """(shape, member, word within the member) of word i of block j; a word of the gap behind a member counts to that member."""
        blk = self.blocks[j]
        b = min((i - blk.off) // blk.bs, blk.count - 1)
        return blk.key, int(b), int(i - blk.off - b * blk.bs)


def put(image, blk, words):
    """The members' valid bits <- words (count x rows x width), everything else as it is."""
    image[blk.idx] = (image[blk.idx] & ~blk.valid) | (words & blk.valid)


def get(image, blk):
    return image[blk.idx] & blk.valid


class Ints:
    """One int32 buffer for the per-member outputs (or inputs) of many shapes: a shape's entries back to back, member b at b * per,
    then three entries that stay as they were."""

    def __init__(self):
        self.keys, self.offs, self.pers, self.size = [], [], [], 0

    def add(self, key, per, count=BATCH):
        off = self.size
        self.keys.append(key)
        self.offs.append(off)
        self.pers.append(per)
        self.size += per * count + 3
        return off

    def image(self, fill=-7):
        return np.full(self.size, fill, dtype=np.int32)

    def offsets(self):
        return np.array(self.offs, dtype=np.int64)

    def locate(self, j, i):
        return self.keys[j], int((i - self.offs[j]) // max(1, self.pers[j])), int(i - self.offs[j])


Ptr = namedtuple("Ptr", "name off")  # element `off` of buffer `name`


class Job:
    """One arena per operand of one call, with its launches and what has to come back."""

    def __init__(self, call, flags):
        self.call, self.flags = call, flags
        self.bufs, self.want, self.where, self.mask, self.launches, self.extra = {}, {}, {}, {}, [], []

    def buf(self, name, image, want, where, mask=None):
        """want None: the buffer has to come back as it went."""
        self.bufs[name], self.want[name], self.where[name] = image, image if want is None else want, where
        if mask is not None:
            self.mask[name] = mask

    def launch(self, key, *args, error=None):
        """error: the hipError_t the call has to refuse this shape with."""
        self.launches.append((key, args, error))

    def failures(self, got):
        """[(shape, text)] for every buffer that differs from what it has to hold, at most three words per shape and buffer."""
        out = []
        for name, want in self.want.items():
            diff = got[name] != want
            if name in self.mask:
                diff = ((got[name] ^ want) & self.mask[name]) != 0
            at = np.flatnonzero(diff)
            block = np.searchsorted(self.where[name].offsets(), at, side="right") - 1
            for j in np.unique(block):
                for i in at[block == j][:3]:
                    key, b, w = self.where[name].locate(int(j), int(i))
                    out.append((key, f"{key} member {b} {name}[{w}]"))
        for check in self.extra:
            out += check(got)
        return out


def verdict(call, flags, failures, nshapes):
    """The assertion of a sweep: which call, which flags, the first failing shapes with member and word, and how many in all."""
    bad = sorted({key for key, _ in failures})
    assert not failures, (f"{call} ({flags}): {len(bad)} of {nshapes} shapes differ; first " + "; ".join(t for _, t in failures[:12])
                          + f"; failing shapes: {bad[:40]}")


# ---- expectations, computed once per (operation, shape) and shared --------------------------------------------------------------------

_expected = {}


def cached(key, make):
    if key not in _expected:
        _expected[key] = make()
    return _expected[key]


def rank_of(oracle, bits):
    return oracle.echelonize(Mzd.from_bits(bits), 0) if bits.size else 0


def rank_np(bits):
    """The rank without the oracle: the rows as Python integers, eliminated by their leading bits."""
    basis = {}
    for row in bits:
        x = int("".join(map(str, row.tolist())), 2)
        while x and x.bit_length() in basis:
            x ^= basis[x.bit_length()]
        if x:
            basis[x.bit_length()] = x
    return len(basis)


def ech_expected(oracle, m, n, full):
    """(words, rank, pivots with their -1 tail) of the five members, by the oracle's gf2o_echelonize."""
    def make():
        mn = min(m, n)
        W, ranks, piv = [], np.zeros(BATCH, np.int32), np.full((BATCH, mn), -1, np.int32)
        for b, G in enumerate(members(m, n)):
            M = Mzd.from_bits(G)
            r = ranks[b] = oracle.echelonize(M, full)
            piv[b, :r] = np.argmax(M.to_bits()[:r], axis=1)   # the leading one of each of the first r rows
            W.append(M.valid_words().copy())
        return np.stack(W), ranks, piv.reshape(-1)
    return cached(("ech", m, n, full), make)


def orders(m, n):
    """A seeded permutation of the columns per member."""
    return np.stack([_rng(m, n, b, 3).permutation(n).astype(np.int32) for b in range(BATCH)])


def order_expected(m, n):
    """full = 1 on the orders above, by the NumPy rule of tests/order_cases.py."""
    def make():
        mn = min(m, n)
        S, ranks, piv = [], np.zeros(BATCH, np.int32), np.zeros((BATCH, mn), np.int32)
        for b, (G, o) in enumerate(zip(members(m, n), orders(m, n))):
            s, ranks[b], piv[b] = oc.ech_order(G, o, 1, m)
            S.append(s)
        return to_words(np.stack(S)), ranks, piv.reshape(-1)
    return cached(("order", m, n), make)


def ple_expected(oracle, bits, pluq):
    """(words, P, Q, rank) of the members `bits`, by the oracle's gf2o_ple / gf2o_pluq."""
    W, Ps, Qs, ranks = [], [], [], np.zeros(len(bits), np.int32)
    for b, G in enumerate(bits):
        M = Mzd.from_bits(G)
        ranks[b], P, Q = oracle.ple(M, pluq=bool(pluq))
        W.append(M.valid_words().copy())
        Ps.append(P.copy())
        Qs.append(Q.copy())
    return np.stack(W), np.concatenate(Ps), np.concatenate(Qs), ranks


def reconstruct(bits, rank, P, Q):
    """P L U Q from a PLUQ form without the oracle: L the unit lower triangle of the first `rank` columns, U the unit upper first
    `rank` rows; Q's transpositions undone on the columns of L U, then P's on its rows (both descending)."""
    L = np.tril(bits[:, :rank], -1).astype(np.int64)
    L[np.arange(rank), np.arange(rank)] = 1
    U = np.triu(bits[:rank], 1).astype(np.int64)
    U[np.arange(rank), np.arange(rank)] = 1
    X = ((L @ U) & 1).astype(np.uint8)
    for j in range(rank - 1, -1, -1):
        if Q[j] != j:
            X[:, [j, Q[j]]] = X[:, [Q[j], j]]
    for i in range(rank - 1, -1, -1):
        if P[i] != i:
            X[[i, P[i]]] = X[[P[i], i]]
    return X


def solve_expected(oracle, A, B):
    """(status, rank of A, the bits the call leaves in B): the status from the ranks of A and of [A | B] with A padded by zero rows
    to B's max(m, n), the solution by gf2o_solve_left, an inconsistent member's B as it was."""
    (m, n), (R, k) = A.shape, B.shape
    ra = rank_of(oracle, A)
    aug = np.zeros((R, n + k), np.uint8)
    aug[:m, :n], aug[:, n:] = A, B
    if rank_of(oracle, aug) != ra:
        return -1, ra, B
    X = Mzd.from_bits(B)
    assert oracle.solve_left(Mzd.from_bits(A), X, True) == 0
    return 0, ra, X.to_bits()


def systems(m, n, k, shared=False):
    """(A, B) of the five members of a solve: member 2 a random B on a low-rank A, the others B = A X on the members of the shape
    (shared: every member on the one low-rank A).  B has max(m, n) rows, those behind m zero."""
    R = max(m, n)
    low = bits_of("lowrank", m, n, _rng(m, n, 2, 5))
    As, Bs = [], []
    for b in range(BATCH):
        rng = _rng(m, n, b, 6)
        A = low if b == 2 or shared else member(m, n, b)
        B = np.zeros((R, k), np.uint8)
        if b == 2:
            B[:m] = rng.integers(0, 2, size=(m, k), dtype=np.uint8)
        else:
            B[:m] = (A.astype(np.int64) @ rng.integers(0, 2, size=(n, k), dtype=np.int64)) & 1
        As.append(A)
        Bs.append(B)
    return np.stack(As), np.stack(Bs)


def solve_case(oracle, m, n, shared=False):
    """The systems of shape (m, n) at its scheduled k as words, with status, rank, B afterwards (X) and the oracle's PLUQ of every A
    (of the one A when shared) as (words, P, Q, rank)."""
    def make():
        k = k_of(m, n)
        As, Bs = systems(m, n, k, shared)
        res = [solve_expected(oracle, A, B) for A, B in zip(As, Bs)]
        return dict(k=k, A=to_words(As), B=to_words(Bs), status=np.array([r[0] for r in res], np.int32),
                    rank=np.array([r[1] for r in res], np.int32), X=to_words(np.stack([r[2] for r in res])),
                    factors=ple_expected(oracle, As[:1] if shared else As, 1))
    return cached(("solve", m, n, shared), make)


def inv_member(oracle, n, b):
    """Members 0 .. 3 invertible (unit lower times unit upper times a permutation), member 4 singular: a repeated row, a zero column
    or a random matrix, by n."""
    rng = _rng(n, b, 7)
    G = rng.integers(0, 2, size=(n, n), dtype=np.uint8)
    if b < 4:
        L, U = np.tril(G, -1).astype(np.int64), np.triu(rng.integers(0, 2, size=(n, n)), 1).astype(np.int64)
        np.fill_diagonal(L, 1)
        np.fill_diagonal(U, 1)
        return ((L @ U)[:, rng.permutation(n)] & 1).astype(np.uint8)
    if n % 3 == 0:
        G[n // 2] = G[0]
    elif n % 3 == 1:
        G[:, int(rng.integers(0, n))] = 0
    else:
        while rank_of(oracle, G) == n:
            G = rng.integers(0, 2, size=(n, n), dtype=np.uint8)
    return G


def inv_case(oracle, n):
    def make():
        A = np.stack([inv_member(oracle, n, b) for b in range(BATCH)])
        inv = np.stack([oracle.inv(Mzd.from_bits(G)).valid_words().copy() for G in A])
        return dict(A=A, inv=inv, rank=np.array([rank_of(oracle, G) for G in A], np.int32))
    return cached(("inv", n), make)


def kernel_expected(oracle, m, n):
    """(R of n x kc_of(m, n) bits, the columns behind the nullity zero; rank), by the oracle's gf2o_kernel_left_pluq."""
    def make():
        kc = kc_of(m, n)
        R, ranks = np.zeros((BATCH, n, kc), np.uint8), np.zeros(BATCH, np.int32)
        for b, G in enumerate(members(m, n)):
            ranks[b], basis = oracle.kernel_left_pluq(Mzd.from_bits(G))
            c = min(kc, n - ranks[b])
            if c:
                R[b, :, :c] = basis.to_bits()[:, :c]
        return to_words(R), ranks
    return cached(("kernel", m, n), make)


def product_expected(plane, op, a, b):
    """(m, l, n), A and B as stored, C before the call and op(A) op(B) as bits: NumPy's batched integer product mod 2.  (Cheaper to
    compute than to keep: the products and the transposes are not cached.)"""
    m, l, n = triple(plane, a, b)
    ta, tb = op
    A = members(*((l, m) if ta else (m, l)))
    B = members(*((n, l) if tb else (l, n)), salt=1)
    Ao, Bo = (A.transpose(0, 2, 1) if ta else A), (B.transpose(0, 2, 1) if tb else B)
    return (m, l, n), A, B, noise(m, n, 8), ((Ao.astype(np.int64) @ Bo.astype(np.int64)) & 1).astype(np.uint8)


# ---- the jobs: one arena per operand for a list of shapes -------------------------------------------------------------------------------

def ech_job(oracle, shapes, full, order=False):
    """m4ri_amd_echelonize_batch_dev; order: the same through m4ri_amd_echelonize_order_batch_dev, NULL order, in place."""
    job = Job("echelonize_order_batch_dev" if order else "echelonize_batch_dev", f"full={full}" + (", order=NULL, in place" if order else ""))
    A, rank, piv = Arena(), Ints(), Ints()
    lay = [(s, A.add(s, *s), rank.add(s, 1), piv.add(s, min(s))) for s in shapes]
    hA, er, ep = A.dirt(1, *shapes[0]), rank.image(), piv.image()
    for (m, n), blk, _, _ in lay:
        put(hA, blk, to_words(members(m, n)))
    eA = hA.copy()
    for (m, n), blk, ro, po in lay:
        W, r, p = ech_expected(oracle, m, n, full)
        put(eA, blk, W)
        er[ro:ro + BATCH], ep[po:po + p.size] = r, p
        a = Ptr("A", blk.off)
        if order:
            job.launch((m, n), a, blk.stride, blk.bs, a, blk.stride, blk.bs, m, n, m, 0, 0, n, BATCH, full, Ptr("rank", ro), Ptr("pivots", po))
        else:
            job.launch((m, n), a, blk.stride, blk.bs, m, n, BATCH, full, Ptr("rank", ro), Ptr("pivots", po))
    job.buf("A", hA, eA, A)
    job.buf("rank", rank.image(), er, rank)
    job.buf("pivots", piv.image(), ep, piv)
    return job


def order_job(shapes):
    """m4ri_amd_echelonize_order_batch_dev out of place, full = 1, a permutation order per member."""
    job = Job("echelonize_order_batch_dev", "full=1, permutation orders, out of place")
    A, D, O, rank, piv = Arena(), Arena(), Ints(), Ints(), Ints()
    lay = [(s, A.add(s, *s), D.add(s, *s, pad=2, gap=5), O.add(s, s[1]), rank.add(s, 1), piv.add(s, min(s))) for s in shapes]
    hA, hD, hO, er, ep = A.dirt(2, *shapes[0]), D.dirt(3, *shapes[0]), O.image(I32_MAX), rank.image(), piv.image()
    for (m, n), ba, bd, oo, _, _ in lay:
        put(hA, ba, to_words(members(m, n)))
        put(hD, bd, to_words(noise(m, n, 4)))
        hO[oo:oo + BATCH * n] = orders(m, n).reshape(-1)
    eD = hD.copy()
    for (m, n), ba, bd, oo, ro, po in lay:
        W, r, p = order_expected(m, n)
        put(eD, bd, W)
        er[ro:ro + BATCH], ep[po:po + p.size] = r, p
        job.launch((m, n), Ptr("D", bd.off), bd.stride, bd.bs, Ptr("A", ba.off), ba.stride, ba.bs, m, n, m, Ptr("order", oo), n, n, BATCH, 1,
                   Ptr("rank", ro), Ptr("pivots", po))
    job.buf("A", hA, None, A)
    job.buf("D", hD, eD, D)
    job.buf("order", hO, None, O)
    job.buf("rank", rank.image(), er, rank)
    job.buf("pivots", piv.image(), ep, piv)
    return job


def ple_job(oracle, shapes, pluq):
    """m4ri_amd_ple_batch_dev; for PLUQ on the shapes up to 64 x 64 also P L U Q = A from what the device left in member 0."""
    job = Job("ple_batch_dev", f"pluq={pluq}")
    A, P, Q, rank = Arena(), Ints(), Ints(), Ints()
    lay = [(s, A.add(s, *s), P.add(s, s[0]), Q.add(s, s[1]), rank.add(s, 1)) for s in shapes]
    hA, eP, eQ, er = A.dirt(5, *shapes[0]), P.image(), Q.image(), rank.image()
    for (m, n), blk, _, _, _ in lay:
        put(hA, blk, to_words(members(m, n)))
    eA = hA.copy()
    for (m, n), blk, po, qo, ro in lay:
        W, p, q, r = cached(("ple", m, n, pluq), lambda: ple_expected(oracle, members(m, n), pluq))
        put(eA, blk, W)
        eP[po:po + p.size], eQ[qo:qo + q.size], er[ro:ro + BATCH] = p, q, r
        job.launch((m, n), Ptr("A", blk.off), blk.stride, blk.bs, m, n, BATCH, pluq, Ptr("P", po), Ptr("Q", qo), Ptr("rank", ro))
    job.buf("A", hA, eA, A)
    job.buf("P", P.image(), eP, P)
    job.buf("Q", Q.image(), eQ, Q)
    job.buf("rank", rank.image(), er, rank)

    def rebuilt(got):
        out = []
        for (m, n), blk, po, qo, ro in lay:
            if max(m, n) <= 64:
                r = int(got["rank"][ro])
                if not 0 <= r <= min(m, n):
                    out.append(((m, n), f"{(m, n)} member 0 rank {r} out of range"))
                    continue
                bits = oc.from_words(get(got["A"], blk)[0], n)
                Pm, Qm = np.clip(got["P"][po:po + m], 0, m - 1), np.clip(got["Q"][qo:qo + n], 0, n - 1)
                if not np.array_equal(reconstruct(bits, r, Pm, Qm), member(m, n, 0)):
                    out.append(((m, n), f"{(m, n)} member 0: P L U Q != A"))
        return out
    if pluq:
        job.extra.append(rebuilt)
    return job

def solve_job(oracle, shapes):
    """m4ri_amd_solve_left_batch_dev at k_of(m, n): status, rank, B (untouched where the status is -1), A unchanged."""
    job = Job("solve_left_batch_dev", "k scheduled")
    A, B, status, rank = Arena(), Arena(), Ints(), Ints()
    lay = []
    for m, n in shapes:
        c = solve_case(oracle, m, n)
        key = (m, n, c["k"])
        lay.append((key, c, A.add(key, m, n), B.add(key, max(m, n), c["k"], pad=2, gap=5), status.add(key, 1), rank.add(key, 1)))
    hA, hB, es, er = A.dirt(6, *shapes[0]), B.dirt(7, *shapes[0]), status.image(), rank.image()
    for _, c, ba, bb, _, _ in lay:
        put(hA, ba, c["A"])
        put(hB, bb, c["B"])
    eB = hB.copy()
    for (m, n, k), c, ba, bb, so, ro in lay:
        put(eB, bb, c["X"])
        es[so:so + BATCH], er[ro:ro + BATCH] = c["status"], c["rank"]
        job.launch((m, n, k), Ptr("A", ba.off), ba.stride, ba.bs, m, n, Ptr("B", bb.off), bb.stride, bb.bs, k, BATCH, Ptr("status", so),
                   Ptr("rank", ro))
    job.buf("A", hA, None, A)
    job.buf("B", hB, eB, B)
    job.buf("status", status.image(), es, status)
    job.buf("rank", rank.image(), er, rank)
    return job


def pluq_solve_job(oracle, shapes, shared=False):
    """m4ri_amd_pluq_solve_left_batch_dev on the ORACLE's factors, P, Q and rank of the systems of solve_job (shared: one decomposition
    for all five members, a_bs = 0): status and B as the one-call solve, the decomposition unchanged."""
    job = Job("pluq_solve_left_batch_dev", "the oracle's factors, k scheduled" + (", a_bs=0" if shared else ""))
    nf = 1 if shared else BATCH
    F, B, P, Q, rank, status = Arena(), Arena(), Ints(), Ints(), Ints(), Ints()
    lay = []
    for m, n in shapes:
        c = solve_case(oracle, m, n, shared)
        key = (m, n, c["k"])
        lay.append((key, c, F.add(key, m, n, count=nf), B.add(key, max(m, n), c["k"], pad=2, gap=5), P.add(key, m, nf), Q.add(key, n, nf),
                    rank.add(key, 1, nf), status.add(key, 1)))
    hF, hB, hP, hQ, hr, es = F.dirt(8, *shapes[0]), B.dirt(9, *shapes[0]), P.image(), Q.image(), rank.image(), status.image()
    for _, c, bf, bb, po, qo, ro, _ in lay:
        W, p, q, r = c["factors"]
        put(hF, bf, W)
        put(hB, bb, c["B"])
        hP[po:po + p.size], hQ[qo:qo + q.size], hr[ro:ro + nf] = p, q, r
    eB = hB.copy()
    for (m, n, k), c, bf, bb, po, qo, ro, so in lay:
        put(eB, bb, c["X"])
        es[so:so + BATCH] = c["status"]
        job.launch((m, n, k), Ptr("A", bf.off), bf.stride, 0 if shared else bf.bs, m, n, Ptr("rank", ro), Ptr("P", po), Ptr("Q", qo),
                   Ptr("B", bb.off), bb.stride, bb.bs, k, BATCH, Ptr("status", so))
    job.buf("A", hF, None, F)
    job.buf("B", hB, eB, B)
    for name, h, where in (("P", hP, P), ("Q", hQ, Q), ("rank", hr, rank)):
        job.buf(name, h, None, where)
    job.buf("status", status.image(), es, status)
    return job


def inv_job(oracle, ns, inplace):
    """m4ri_amd_inv_batch_dev: the oracle's gf2o_inv of every member, the singular one included, and the ranks."""
    job = Job("inv_batch_dev", "in place" if inplace else "out of place")
    A, B, rank = Arena(), Arena(), Ints()
    lay = [(n, inv_case(oracle, n), A.add((n, n), n, n, pad=2, gap=7), None if inplace else B.add((n, n), n, n), rank.add((n, n), 1))
           for n in ns]
    hA, hB, er = A.dirt(10, ns[0]), B.dirt(11, ns[0]), rank.image()
    for n, c, ba, bb, _ in lay:
        put(hA, ba, to_words(c["A"]))
        if not inplace:
            put(hB, bb, to_words(noise(n, n, 12)))
    eA, eB = hA.copy(), hB.copy()
    for n, c, ba, bb, ro in lay:
        er[ro:ro + BATCH] = c["rank"]
        a = Ptr("A", ba.off)
        if inplace:
            put(eA, ba, c["inv"])
            job.launch((n, n), a, ba.stride, ba.bs, a, ba.stride, ba.bs, n, BATCH, Ptr("rank", ro))
        else:
            put(eB, bb, c["inv"])
            job.launch((n, n), Ptr("Binv", bb.off), bb.stride, bb.bs, a, ba.stride, ba.bs, n, BATCH, Ptr("rank", ro))
    job.buf("A", hA, eA, A)
    if not inplace:
        job.buf("Binv", hB, eB, B)
    job.buf("rank", rank.image(), er, rank)
    return job


def kernel_job(oracle, shapes):
    """m4ri_amd_kernel_left_batch_dev at kc_of(m, n): R with the columns behind the nullity written zero, rank, A unchanged."""
    job = Job("kernel_left_batch_dev", "kc scheduled")
    A, R, rank = Arena(), Arena(), Ints()
    lay = [((m, n, kc_of(m, n)), A.add((m, n, kc_of(m, n)), m, n), R.add((m, n, kc_of(m, n)), n, kc_of(m, n), pad=2, gap=5),
            rank.add((m, n, kc_of(m, n)), 1)) for m, n in shapes]
    hA, hR, er = A.dirt(13, *shapes[0]), R.dirt(14, *shapes[0]), rank.image()
    for (m, n, kc), ba, br, _ in lay:
        put(hA, ba, to_words(members(m, n)))
        put(hR, br, to_words(noise(n, kc, 15)))
    eR = hR.copy()
    for (m, n, kc), ba, br, ro in lay:
        want, r = kernel_expected(oracle, m, n)
        put(eR, br, want)
        er[ro:ro + BATCH] = r
        job.launch((m, n, kc), Ptr("A", ba.off), ba.stride, ba.bs, m, n, Ptr("R", br.off), br.stride, br.bs, kc, BATCH, Ptr("rank", ro))
    job.buf("A", hA, None, A)
    job.buf("R", hR, eR, R)
    job.buf("rank", rank.image(), er, rank)
    return job


def mul_job(plane, pairs, add, op=NN, results_only=(), refused=()):
    """m4ri_amd_mul_small_batch_dev (op NN) or m4ri_amd_mul_small_batch_op_dev at the (a, b) of a plane.  results_only: the pairs at
    which only C's valid bits are compared (beyond 64 the route depends on a measured bound, and a forwarded product may write whole
    last words); refused: the pairs the call has to answer with hipErrorNotSupported, nothing written."""
    ta, tb = op
    name = "mul_small_batch_dev" if op == NN else "mul_small_batch_op_dev"
    job = Job(name, f"plane {plane}, shapes as (m, l, n), add={add}" + ("" if op == NN else f", trans_a={ta}, trans_b={tb}"))
    A, B, C = Arena(), Arena(), Arena()
    lay = []
    for a, b in pairs:
        key, As, Bs, C0, AB = product_expected(plane, op, a, b)
        want = None if (a, b) in refused else to_words(AB ^ C0 if add else AB)
        lay.append((a, b, key, to_words(As), to_words(Bs), to_words(C0), want, A.add(key, *As.shape[1:]),
                    B.add(key, *Bs.shape[1:], pad=3, gap=5), C.add(key, key[0], key[2], gap=7)))
    hA, hB, hC = A.dirt(16, *pairs[0]), B.dirt(17, *pairs[0]), C.dirt(18, *pairs[0])
    mask = np.full(C.size, ~np.uint64(0), np.uint64)
    for a, b, key, As, Bs, C0, want, ba, bb, bc in lay:
        put(hA, ba, As)
        put(hB, bb, Bs)
        put(hC, bc, C0)
    eC = hC.copy()
    for a, b, (m, l, n), As, Bs, C0, want, ba, bb, bc in lay:
        if (a, b) in results_only:
            mask[bc.off:bc.end] = 0
            mask[bc.idx] = bc.valid
        if want is not None:
            put(eC, bc, want)
        args = (Ptr("C", bc.off), bc.stride, bc.bs, Ptr("A", ba.off), ba.stride, ba.bs, Ptr("B", bb.off), bb.stride, bb.bs, m, l, n, BATCH)
        job.launch((m, l, n), *args, *((add,) if op == NN else (ta, tb, add)), error=None if want is not None else 801)
    job.buf("A", hA, None, A)
    job.buf("B", hB, None, B)
    job.buf("C", hC, eC, C, mask)
    return job


def transpose_job(shapes, inplace=False):
    """m4ri_amd_transpose_batch_dev against NumPy's .T; in place on squares."""
    job = Job("transpose_batch_dev", "in place" if inplace else "out of place")
    A, D = Arena(), Arena()
    lay = [(s, members(*s), A.add(s, *s), None if inplace else D.add(s, s[1], s[0], pad=3, gap=7)) for s in shapes]
    hA, hD = A.dirt(19, *shapes[0]), D.dirt(20, *shapes[0])
    for (m, n), G, ba, bd in lay:
        put(hA, ba, to_words(G))
        if not inplace:
            put(hD, bd, to_words(noise(n, m, 21)))
    eA, eD = hA.copy(), hD.copy()
    for (m, n), G, ba, bd in lay:
        want = to_words(np.ascontiguousarray(G.transpose(0, 2, 1)))
        a = Ptr("A", ba.off)
        if inplace:
            put(eA, ba, want)
            job.launch((m, n), a, ba.stride, ba.bs, a, ba.stride, ba.bs, m, n, BATCH)
        else:
            put(eD, bd, want)
            job.launch((m, n), Ptr("D", bd.off), bd.stride, bd.bs, a, ba.stride, ba.bs, m, n, BATCH)
    job.buf("A", hA, eA, A)
    if not inplace:
        job.buf("D", hD, eD, D)
    return job
