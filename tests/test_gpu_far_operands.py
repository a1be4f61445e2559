"""Every device entry point of Part 2 of include/m4ri_amd.h on operands whose rows, or whose batch members, lie 2 GiB to 16 GiB
apart: the header promises any stride >= the width and batch strides of any size, and the classic indexing defect (an int index,
a uint32 byte offset, a buffer descriptor one step too far) shows only where an offset no longer fits in 32 bits.  All operands of
a case are windows of ONE pattern-filled arena (tests/far_arena.py, which also holds the argument why a 32-bit defect changes a
word of the arena instead of faulting); results are compared with the CPU oracle on compact copies, bit for bit, read-only
operands must come back unchanged, and after the operands are restored the whole arena must be the pattern again.

CASES is the table: entry point, far axis ("rows": a far row stride, "batch": a far batch stride), stride, shape, the path the
shape reaches.  tests/test_far_arena_cpu.py checks its arithmetic without a GPU and compares the entry points with the header.

Left out, because:"""
import ctypes
from dataclasses import dataclass, field

import numpy as np
import pytest
import torch

import assemble_cases as ac
import dev_frame as df
import elim_cases as ec
import far_arena as fa
import m4ri_amd
import reduce_cases as rc
from elim_cases import make as _make
from far_arena import BATCH, BS_EVEN, BS_ODD, S_EVEN, S_ODD, S_REFUSED, S_TABLE, S_TABLE_EVEN, Win
from m4ri_amd.mzd import Mzd

LEFT_OUT = {
    "m4ri_amd_shard_down_dev": "the multi-device schedule (its operands are the local slabs of a sharded product): one GPU here",
    "m4ri_amd_shard_up_dev": "the multi-device schedule, as above",
}
__doc__ += "".join(f"\n  {k}: {v}" for k, v in LEFT_OUT.items())

pytestmark = pytest.mark.gpu
INVALID = 1  # hipErrorInvalidValue
HEADROOM = 8 << 30


def words(n):
    return (n + 63) // 64


@dataclass
class Case:
    id: str
    entry: str
    axis: str                 # "rows" or "batch": the one far axis
    stride: int               # the far stride, in words
    shape: tuple
    path: str                 # what the shape reaches
    wins: dict                # name -> Win
    far: tuple                # the names of the windows that go far
    run: object               # run(arena, oracle, case)
    b_sides: tuple = ()       # windows that are the B side of a product
    same: tuple = ()          # pairs of names that are one read-only operand (A == B)
    unreached: dict = field(default_factory=dict)   # threshold -> why no far operand of this case can cross it
    label: str = ""           # with `unreached`: what kind of case this is (tests/test_far_arena_cpu.py pins label -> thresholds)
    touched: dict = field(default_factory=dict)     # name -> the rows of that window the call touches, where not all of them
    refused: bool = False     # the call must return hipErrorInvalidValue
    plan: tuple = ()          # (plan function, arguments, expected path)


CASES = []


def F(slot, rows, ncols, stride):
    """An operand far by its rows: slot i of the pitch (4096 words each, 16-byte aligned)."""
    return Win(4096 * slot, rows, words(ncols), stride)


def K(i, rows, ncols):
    """A compact operand: ordinary stride (one padding word), inside the first pitch, beyond the slots."""
    return Win((1 << 20) + (i << 18), rows, words(ncols), words(ncols) + 1)


def near_stride(w, far):
    """The smallest row stride > w of the far stride's parity (even: all rows 16-byte aligned; odd: every other one)."""
    return w + 1 + ((w + 1 + far) & 1)


FAR_OFF = 64 << 20


def M_(i, rows, ncols, bs, batch=BATCH, shared=False):
    """Members far by their batch stride: operand i of the call, rows an ordinary stride apart.  Far operands of one call are
    interleaved, member by member, like blocks of one parent."""
    w = words(ncols)
    return Win(FAR_OFF + (i << 20), rows, w, near_stride(w, bs), 1 if shared else batch, 0 if shared else bs)


def Mc(i, rows, ncols, batch=BATCH, shared=False):
    """Compact members below the far operands: rows one padding word apart, members three more."""
    w = words(ncols)
    return Win(i << 22, rows, w, w + 1, 1 if shared else batch, 0 if shared else rows * (w + 1) + 3)


def lay(BS, far, **ops):
    """The windows of a call whose entry point refuses operands with meeting SPANS (first member's start to last member's end):
    only the operands named in `far` lie a far batch stride apart, the others are compact and below them.  ops: name -> (rows,
    ncols[, "shared"])."""
    return {name: (M_ if name in far else Mc)(i, spec[0], spec[1], *((BS,) if name in far else ()), shared=len(spec) > 2) for i, (name, spec) in enumerate(ops.items())}


def _call(name, *args):
    rc_ = getattr(m4ri_amd.lib(), name)(*args)
    assert rc_ == 0, (name, rc_)
    torch.cuda.synchronize()


def _dev(a, dtype=np.int32):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).cuda()


def _host(t):
    return t.cpu().numpy()


_memo = {}


def memo(key, fn):
    """One reference per (operation, shape): computed once, shared by the cases that need it, never written."""
    if key not in _memo:
        _memo[key] = fn()
    return _memo[key]


def members(fn, n=BATCH):
    return [fn(b) for b in range(n)]


def bits_to(b):
    return df.pack_bits(b)


def sname(s):
    return {S_ODD: "S_ODD", S_EVEN: "S_EVEN", BS_ODD: "BS_ODD", BS_EVEN: "BS_EVEN", S_REFUSED: "S_REFUSED"}[s]


# ================================================ far by row stride ===============================================================

# ---- products -----------------------------------------------------------------------------------------------------------------------

def _product_wins(m, l, n, S, which):
    fA, fB = which in ("all", "AC", "A==B"), which in ("all", "B", "A==B")
    w = {"A": F(0, m, l, S) if fA else K(0, m, l), "B": F(1, l, n, S) if fB else K(1, l, n), "C": F(2, m, n, S) if fA else K(2, m, n)}
    if which == "A==B":
        w["B"] = w["A"]
    return w


def _run_product(entry, m, l, n, add, extra, same):
    def run(ar, oracle, c):
        A, C0 = Mzd.random(m, l, 11), Mzd.random(m, n, 13)
        B = A if same else Mzd.random(l, n, 12)
        want = memo(("mul", m, l, n, add, same), lambda: oracle.addmul(C0.copy(), A, B) if add else oracle.mul(None, A, B))
        pA = ar.place(c.wins["A"], A)
        pB = pA if same else ar.place(c.wins["B"], B)
        pC = ar.place(c.wins["C"], C0)
        _call(entry, pC.ptr, c.wins["C"].stride, pA.ptr, c.wins["A"].stride, pB.ptr, c.wins["B"].stride, m, l, n, add, extra, None)
        pC.check(want, "zero", "C")
        pA.check_unchanged("A")
        pB.check_unchanged("B")
    return run


def _products():
    for entry in ("m4ri_amd_mul_dev", "m4ri_amd_m4rm_dev"):
        for S in (S_ODD, S_EVEN):
            for shape in ((300, 300, 300), (280, 70, 130)):
                for add in (0, 1):
                    for which in ("all", "AC", "B"):
                        wins = _product_wins(*shape, S, which)
                        far = {"all": ("A", "B", "C"), "AC": ("A", "C"), "B": ("B",)}[which]
                        unreached, label = {}, ""
                        if which == "B" and shape[1] == 70:
                            unreached, label = {"int32-words": "B alone is far and has 70 rows"}, "B alone far, 70 rows"
                        CASES.append(Case(f"{entry[9:-4]}-{sname(S)}-{'x'.join(map(str, shape))}-add{add}-far:{which}", entry, "rows", S, shape,
                                          "launch_leaf cuts rows of A/C and slabs of B to 64", wins, far, _run_product(entry, *shape, add, 0, False),
                                          b_sides=("B",) if which != "AC" else (), unreached=unreached, label=label))
        CASES.append(Case(f"{entry[9:-4]}-S_EVEN-300x300x300-A==B", entry, "rows", S_EVEN, (300, 300, 300), "A and B one operand", _product_wins(300, 300, 300, S_EVEN, "A==B"),
                          ("A", "C"), _run_product(entry, 300, 300, 300, 0, 0, True), b_sides=("B",), same=(("A", "B"),)))
    for S in (S_ODD, S_EVEN):
        for add in (0, 1):
            CASES.append(Case(f"mul-{sname(S)}-300x300x300-add{add}-cutoff64", "m4ri_amd_mul_dev", "rows", S, (300, 300, 300),
                              "two levels: the passes read ancestors with a far p_stride, then the strips", _product_wins(300, 300, 300, S, "all"), ("A", "B", "C"),
                              _run_product("m4ri_amd_mul_dev", 300, 300, 300, add, 64, False), b_sides=("B",)))


# ---- xor, fill, mask ------------------------------------------------------------------------------------------------------------------

def _elementwise():
    r, n = 300, 333
    for S in (S_ODD, S_EVEN):
        def run_xor3(ar, oracle, c):
            A, B, C0 = Mzd.random(r, n, 21), Mzd.random(r, n, 22), Mzd.random(r, n, 23)
            want = oracle.add(Mzd(r, n), A, B)
            pA, pB, pC = ar.place(c.wins["A"], A), ar.place(c.wins["B"], B), ar.place(c.wins["C"], C0, dirty_tail=True)
            _call("m4ri_amd_xor_dev", pC.ptr, c.stride, pA.ptr, c.stride, pB.ptr, c.stride, r, n, None)
            pC.check(want, "kept", "C")
            pA.check_unchanged("A")
            pB.check_unchanged("B")

        def run_xor2(ar, oracle, c):
            A, B = Mzd.random(r, n, 21), Mzd.random(r, n, 22)
            want = oracle.add(Mzd(r, n), A, B)
            pA, pB = ar.place(c.wins["A"], A, dirty_tail=True), ar.place(c.wins["B"], B)
            _call("m4ri_amd_xor_dev", pA.ptr, c.stride, pA.ptr, c.stride, pB.ptr, c.wins["B"].stride, r, n, None)
            pA.check(want, "kept", "C == A")
            pB.check_unchanged("B")

        def run_fill(ar, oracle, c):
            p = ar.place(c.wins["M"], Mzd.random(r, n, 24), dirty_tail=True)
            _call("m4ri_amd_fill_dev", p.ptr, c.stride, r, n, 77, None)
            p.check(Mzd.random(r, n, 77), "zero", "M")

        def run_fill_rows(ar, oracle, c):
            p = ar.place(c.wins["M"], Mzd.random(r, n, 24), dirty_tail=True)
            _call("m4ri_amd_fill_rows_dev", p.ptr, c.stride, 1000, r, n, 77, None)
            whole = Mzd.random(1000 + r, n, 77)
            p.check(Mzd(r, n, whole.valid_words()[1000:].copy().reshape(-1), rowstride=words(n)), "zero", "M")

        def run_mask(ar, oracle, c):
            Mx = Mzd.random(r, n, 25)
            p = ar.place(c.wins["M"], Mx, dirty_tail=True)
            _call("m4ri_amd_mask_tail_dev", p.ptr, c.stride, r, n, None)
            p.check(Mx, "zero", "M")

        CASES.append(Case(f"xor-{sname(S)}-three-operands", "m4ri_amd_xor_dev", "rows", S, (r, n), "rowwise", {"A": F(0, r, n, S), "B": F(1, r, n, S), "C": F(2, r, n, S)},
                          ("A", "B", "C"), run_xor3))
        CASES.append(Case(f"xor-{sname(S)}-in-place-compact-B", "m4ri_amd_xor_dev", "rows", S, (r, n), "rowwise, C == A, strides differ", {"A": F(0, r, n, S), "B": K(0, r, n)},
                          ("A",), run_xor2))
        for name, run in (("fill", run_fill), ("fill_rows", run_fill_rows), ("mask_tail", run_mask)):
            CASES.append(Case(f"{name}-{sname(S)}", f"m4ri_amd_{name}_dev", "rows", S, (r, n), "against splitmix_words", {"M": F(0, r, n, S)}, ("M",), run))


# ---- triangular solves and the triangular inverse ----------------------------------------------------------------------------------------

def _triangular():
    for S in (S_ODD, S_EVEN):
        for side in ("left", "right"):
            for upper in (0, 1):
                name = f"trsm_{'upper' if upper else 'lower'}_{side}"
                for kind, (mb, nb) in (("block-inverse", (300, 300)), ("base", (64, 300) if side == "left" else (300, 64))):
                    tn = mb if side == "left" else nb

                    def run(ar, oracle, c, name=name, mb=mb, nb=nb, tn=tn, side=side, base=kind == "base"):
                        T, B = Mzd.random(tn, tn, 31), Mzd.random(mb, nb, 32)
                        if side == "right":
                            df.unit_diag(T)
                        want = memo((name, mb, nb), lambda: getattr(oracle, name)(T, B.copy()))
                        pT, pB = ar.place(c.wins["T"], T, dirty_tail=base), ar.place(c.wins["B"], B, dirty_tail=base)
                        _call(f"m4ri_amd_{name}_dev", pT.ptr, c.stride, pB.ptr, c.stride, mb, nb, 0, None)
                        pB.check(want, "kept" if base else "zero", "B")
                        pT.check_unchanged("T")
                    unreached, label = {}, ""
                    if kind == "base" and side == "left":
                        unreached, label = {"uint32-bytes": "the 64-row base kernel: 63 * S * 8 < 2^32", "int32-words": "the 64-row base kernel: 64 rows"}, "64-row base kernel"
                    CASES.append(Case(f"{name}-{sname(S)}-{kind}", f"m4ri_amd_{name}_dev", "rows", S, (mb, nb),
                                      "the 512-row block inverse, ragged" if kind != "base" else "the base kernel with a far b_stride",
                                      {"T": F(0, tn, tn, S), "B": F(1, mb, nb, S)}, ("B",) if kind == "base" and side == "right" else ("T", "B"), run,
                                      unreached=unreached, label=label))

        def run_trtri(ar, oracle, c):
            U = Mzd.random(300, 300, 33)
            want = memo("trtri", lambda: oracle.trtri_upper(U.copy()))
            p = ar.place(c.wins["U"], U, dirty_tail=True)
            _call("m4ri_amd_trtri_upper_dev", p.ptr, c.stride, 300, None)
            p.check(want, "kept", "U")
        CASES.append(Case(f"trtri_upper-{sname(S)}", "m4ri_amd_trtri_upper_dev", "rows", S, (300,), "one ragged 512-row block", {"U": F(0, 300, 300, S)}, ("U",), run_trtri))


# ---- the table primitives --------------------------------------------------------------------------------------------------------------

def _tables():
    for S, ST in ((S_ODD, S_TABLE), (S_EVEN, S_TABLE_EVEN)):
        for nt in (1, 2, 6):
            ncols = 2048 if nt == 1 else 8192     # wide / 2 >= 64 for the slab kernel of the even layout
            k, nrows, width = 8 * nt, 300, words(ncols)
            path = "apply_tables_kernel<word>" if S == S_ODD else ("apply_tables_kernel<word2>" if nt == 1 else "apply_tables_slab_kernel<word2>")

            def run(ar, oracle, c, nt=nt, ncols=ncols, k=k, nrows=nrows, width=width):
                Mx = Mzd.random(nrows, ncols, 41 + nt)
                Ts, Ls = ec.tables_for(oracle.make_table, Mx, 0, 0, k, nt)
                want = Mx.copy()
                oracle.process_rows(want, k, nrows, 0, k, Ts, Ls)
                pM = ar.place(c.wins["M"], Mx)
                pT = [ar.place(c.wins[f"T{t}"], T) for t, T in enumerate(Ts)]
                dL = [_dev(l) for l in Ls]
                idx = torch.zeros(6 * (nrows - k), dtype=torch.int32, device="cuda")
                kbits = (ctypes.c_int32 * 6)(*ec.split_k(k, nt))
                Tp = (ctypes.c_void_p * 6)(*[p.ptr for p in pT])
                Tstr = (ctypes.c_int64 * 6)(*[c.wins[f"T{t}"].stride for t in range(nt)])
                Lp = (ctypes.c_void_p * 6)(*[l.data_ptr() for l in dL])
                _call("m4ri_amd_process_rows_dev", pM.ptr, c.stride, width, k, nrows, 0, nt, kbits, Tp, Tstr, Lp, idx.data_ptr(), None)
                pM.check(want, "zero", "M")
                for p in pT:
                    p.check_unchanged("table")
            wins = {"M": F(0, nrows, ncols, S)}
            wins.update({f"T{t}": F(1 + t, 256, ncols, ST) for t in range(nt)})
            CASES.append(Case(f"process_rows-{sname(S)}-{nt}-tables", "m4ri_amd_process_rows_dev", "rows", S, (nrows, ncols, nt), path, wins, tuple(wins), run))

        def run_make(ar, oracle, c):
            m_rows, ncols, r, col, k = 20, 300, 5, 70, 8
            Mx, T0 = Mzd.random(m_rows, ncols, 45), Mzd.random(1 << k, ncols, 46)
            want, Lw = T0.copy(), np.zeros(1 << k, dtype=np.int32)
            oracle.make_table(Mx, r, col, k, want, Lw)
            pM, pT = ar.place(c.wins["M"], Mx), ar.place(c.wins["T"], T0)
            dj = torch.zeros(1 << k, dtype=torch.int32, device="cuda")
            _call("m4ri_amd_make_table_dev", pM.ptr, c.wins["M"].stride, m_rows, ncols, r, col, k, pT.ptr, pT.ptr, c.wins["T"].stride, dj.data_ptr(), None)
            pM.check_unchanged("M")
            pT.check(want, "zero", "Tout")
            got = pT.fetch()[0]
            assert np.array_equal(got[0], pT.before[0, 0]) and np.array_equal(got[:, :col // 64], pT.before[0][:, :col // 64])
        CASES.append(Case(f"make_table-{'S_TABLE' if ST == S_TABLE else 'S_TABLE_EVEN'}", "m4ri_amd_make_table_dev", "rows", ST, (20, 300, 8), "k = 8: 256 table rows",
                          {"M": K(0, 20, 300), "T": F(0, 256, 300, ST)}, ("T",), run_make))


# ---- decompositions, permutations, echelon forms, systems --------------------------------------------------------------------------------

def _invertible(oracle, n, base):
    for seed in range(1, 60):
        A = Mzd.random(n, n, base + seed)
        if oracle.echelonize(A.copy(), 0) == n:
            return A
    raise AssertionError("no invertible matrix among 59 seeds")


def _rhs(oracle, A, rows, k, consistent, seed=77):
    B = Mzd(rows, k)
    src = oracle.mul(None, A, Mzd.random(A.ncols, k, seed), 0) if consistent else Mzd.random(A.nrows, k, seed + 1)
    B.valid_words()[: A.nrows] = src.valid_words()
    return B


def _drivers():
    for S in (S_ODD, S_EVEN):
        s = sname(S)
        for pluq in (0, 1):
            for (m, n) in ((300, 300), (300, 130)):
                for kind in ("random", "lowrank"):
                    entry = "m4ri_amd_pluq_dev" if pluq else "m4ri_amd_ple_dev"

                    def run(ar, oracle, c, m=m, n=n, kind=kind, pluq=pluq, entry=entry):
                        A = _make(kind, m, n, 50 + m + n)
                        want = A.copy()
                        r, P, Q = oracle.ple(want, pluq=bool(pluq))
                        p = ar.place(c.wins["A"], A)
                        Pd, Qd, rk = np.full(m, -1, np.int32), np.full(n, -1, np.int32), ctypes.c_int32(-1)
                        _call(entry, p.ptr, c.stride, m, n, Pd.ctypes.data, Qd.ctypes.data, ctypes.byref(rk), 0, None)
                        assert rk.value == r and np.array_equal(Pd, P) and np.array_equal(Qd, Q)
                        p.check(want, "zero", "A")
                    CASES.append(Case(f"{entry[9:-4]}-{s}-{m}x{n}-{kind}", entry, "rows", S, (m, n), "the blocked elimination on far rows", {"A": F(0, m, n, S)}, ("A",), run))

        m, n = 300, 333
        for trans in (0, 1):
            def run_left(ar, oracle, c, trans=trans, m=m, n=n):
                A = Mzd.random(m, n, 61)
                rng = np.random.default_rng(5)
                P = np.array([rng.integers(i, m) for i in range(m)], dtype=np.int32)
                want = A.copy()
                oracle.apply_p_left(want, P, bool(trans))
                p = ar.place(c.wins["A"], A)
                _call("m4ri_amd_apply_p_left_dev", p.ptr, c.stride, m, n, P.ctypes.data, m, trans, None)
                p.check(want, "zero", "A")

            def run_right(ar, oracle, c, trans=trans, m=m, n=n):
                A = Mzd.random(m, n, 62)
                rng = np.random.default_rng(6)
                P = np.array([rng.integers(i, n) for i in range(n)], dtype=np.int32)
                want = A.copy()
                oracle.apply_p_right(want, P, bool(trans))
                p = ar.place(c.wins["A"], A)
                _call("m4ri_amd_apply_p_right_dev", p.ptr, c.stride, m, n, P.ctypes.data, n, trans, None)
                p.check(want, "zero", "A")
            CASES.append(Case(f"apply_p_left-{s}-trans{trans}", "m4ri_amd_apply_p_left_dev", "rows", S, (m, n), "row swaps across far rows", {"A": F(0, m, n, S)}, ("A",), run_left))
            CASES.append(Case(f"apply_p_right-{s}-trans{trans}", "m4ri_amd_apply_p_right_dev", "rows", S, (m, n), "the LDS gather, a row per workgroup", {"A": F(0, m, n, S)}, ("A",), run_right))

        def run_tri(ar, oracle, c):
            A = _make("lowrank", 300, 333, 63)
            E, U = A.copy(), A.copy()
            r, _, Q = oracle.ple(E)
            ru, _, Qu = oracle.ple(U, pluq=True)
            assert r == ru == 100 and np.array_equal(Q, Qu)
            p = ar.place(F(0, 300, 333, c.stride), E)
            Qh = np.ascontiguousarray(Q, dtype=np.int32)
            _call("m4ri_amd_apply_p_right_trans_tri_dev", p.ptr, c.stride, r, 333, Qh.ctypes.data, None)
            want = E.copy()
            want.valid_words()[:r] = U.valid_words()[:r]
            p.check(want, "zero", "A")
        CASES.append(Case(f"apply_p_right_trans_tri-{s}", "m4ri_amd_apply_p_right_trans_tri_dev", "rows", S, (300, 333), "the PLE's first rank rows (100 of them)",
                          {"A": F(0, 300, 333, S)}, ("A",), run_tri, unreached={"int32-words": "only the first rank = 100 rows are touched; the window has 300"}, label="the first rank rows",
                          touched={"A": 100}))

        for full in (0, 1):
            for kind in ("random", "lowrank"):
                def run_ech(ar, oracle, c, full=full, kind=kind):
                    A = _make(kind, 300, 300, 64)
                    want = A.copy()
                    r = oracle.echelonize(want, full)
                    p = ar.place(c.wins["A"], A)
                    rk = ctypes.c_int32(-1)
                    _call("m4ri_amd_echelonize_dev", p.ptr, c.stride, 300, 300, full, ctypes.byref(rk), None)
                    assert rk.value == r
                    p.check(want, "zero", "A")
                CASES.append(Case(f"echelonize-{s}-full{full}-{kind}", "m4ri_amd_echelonize_dev", "rows", S, (300, 300), "PLE, then the back substitution", {"A": F(0, 300, 300, S)},
                                  ("A",), run_ech))

        for (m, n, k) in ((300, 300, 130), (280, 300, 70)):
            for consistent in (True, False):
                tag = "consistent" if consistent else "inconsistent"

                def run_solve(ar, oracle, c, m=m, n=n, k=k, consistent=consistent):
                    A = _make("lowrank", m, n, 65 + m)
                    B = _rhs(oracle, A, max(m, n), k, consistent)
                    Ao, Bo = A.copy(), B.copy()
                    want = oracle.solve_left(Ao, Bo, True)
                    assert want == (0 if consistent else -1)
                    pA, pB = ar.place(c.wins["A"], A), ar.place(c.wins["B"], B)
                    ret = ctypes.c_int(7)
                    _call("m4ri_amd_solve_left_dev", pA.ptr, c.stride, m, n, pB.ptr, c.stride, B.nrows, k, 0, 1, ctypes.byref(ret), None)
                    assert ret.value == want
                    pA.check(Ao, "zero", "A")
                    pB.check(Bo, "zero", "B")

                def run_pluq_solve(ar, oracle, c, m=m, n=n, k=k, consistent=consistent):
                    A = _make("lowrank", m, n, 66 + m)
                    B = _rhs(oracle, A, max(m, n), k, consistent)
                    Ad = A.copy()
                    r, P, Q = oracle.ple(Ad, pluq=True, recursive=True)
                    Bo = B.copy()
                    want = oracle.pluq_solve_left(Ad, r, P, Q, Bo, True)
                    assert want == (0 if consistent else -1)
                    pA, pB = ar.place(c.wins["A"], Ad), ar.place(c.wins["B"], B)
                    ret = ctypes.c_int(7)
                    Ph, Qh = np.ascontiguousarray(P, np.int32), np.ascontiguousarray(Q, np.int32)
                    _call("m4ri_amd_pluq_solve_left_dev", pA.ptr, c.stride, m, n, r, Ph.ctypes.data, Qh.ctypes.data, pB.ptr, c.stride, B.nrows, k, 0, 1, ctypes.byref(ret), None)
                    assert ret.value == want
                    pA.check_unchanged("A")
                    pB.check(Bo, "zero", "B")
                wins = {"A": F(0, m, n, S), "B": F(1, max(m, n), k, S)}
                CASES.append(Case(f"solve_left-{s}-{m}x{n}x{k}-{tag}", "m4ri_amd_solve_left_dev", "rows", S, (m, n, k), "PLUQ, two trsm, the check", wins, ("A", "B"), run_solve))
                CASES.append(Case(f"pluq_solve_left-{s}-{m}x{n}x{k}-{tag}", "m4ri_amd_pluq_solve_left_dev", "rows", S, (m, n, k), "from the oracle's factors", wins, ("A", "B"),
                                  run_pluq_solve))

        for singular in (False, True):
            tag = "singular" if singular else "invertible"

            def run_kernel(ar, oracle, c, singular=singular):
                A = _make("lowrank", 300, 300, 67) if singular else _invertible(oracle, 300, 6000)
                Ao = A.copy()
                r, Ro = oracle.kernel_left_pluq(Ao)
                assert (r < 300) == singular
                kc = max(1, 300 - r)
                pA, pR = ar.place(c.wins["A"], A), ar.place(Win(c.wins["R"].off, 300, words(kc), c.stride), Mzd(300, kc))
                rk = ctypes.c_int32(-1)
                _call("m4ri_amd_kernel_left_pluq_dev", pA.ptr, c.stride, 300, 300, pR.ptr, c.stride, 0, ctypes.byref(rk), None)
                assert rk.value == r
                pA.check(Ao, "zero", "A")
                if Ro is None:
                    pR.check_unchanged("R")
                else:
                    pR.check(Ro, "zero", "R")

            def run_inv(ar, oracle, c, singular=singular):
                A = _invertible(oracle, 300, 6000)
                if singular:
                    A.valid_words()[150] = A.valid_words()[0]
                want = oracle.inv(A)
                pA, pB = ar.place(c.wins["A"], A), ar.place(c.wins["Binv"], Mzd.random(300, 300, 3), dirty_tail=True)
                _call("m4ri_amd_inv_dev", pB.ptr, c.stride, pA.ptr, c.stride, 300, None)
                pA.check_unchanged("A")
                pB.check(want, "zero", "Binv")
            CASES.append(Case(f"kernel_left_pluq-{s}-{tag}", "m4ri_amd_kernel_left_pluq_dev", "rows", S, (300, 300), "PLUQ, then the basis", {"A": F(0, 300, 300, S), "R": F(1, 300, 300, S)},
                              ("A", "R"), run_kernel))
            CASES.append(Case(f"inv-{s}-{tag}", "m4ri_amd_inv_dev", "rows", S, (300,), "[A | I] reduced", {"A": F(0, 300, 300, S), "Binv": F(1, 300, 300, S)}, ("A", "Binv"), run_inv))

        for which in ("A", "D"):
            def run_tr(ar, oracle, c, which=which):
                A = Mzd.random(300, 290, 68)
                want = bits_to(A.to_bits().T.copy())
                pA, pD = ar.place(c.wins["A"], A, dirty_tail=True), ar.place(c.wins["D"], Mzd.random(290, 300, 69), dirty_tail=True)
                _call("m4ri_amd_transpose_dev", pD.ptr, c.wins["D"].stride, pA.ptr, c.wins["A"].stride, 300, 290, None)
                pD.check(want, "zero", "D")
                pA.check_unchanged("A")
            wins = {"A": F(0, 300, 290, S) if which == "A" else K(0, 300, 290), "D": F(1, 290, 300, S) if which == "D" else K(1, 290, 300)}
            CASES.append(Case(f"transpose-{s}-far-{which}", "m4ri_amd_transpose_dev", "rows", S, (300, 290), "the tile kernel", wins, (which,), run_tr))


# ================================================ far by batch stride =============================================================

def _ptr_args(p, w):
    return (p.ptr, w.stride, w.bs)


def _batch_products():
    for BS in (BS_ODD, BS_EVEN):
        s = sname(BS)

        def product(entry, m, l, n, add, tail_args, path, ta=0, tb=0, shared=False, same=False, dirty=False, tail="zero", plan=(), far="ABC"):
            ar_, ac_ = (l, m) if ta else (m, l)
            br_, bc_ = (n, l) if tb else (l, n)

            def run(ar, oracle, c):
                As = members(lambda b: Mzd.random(ar_, ac_, 100 + b), 1 if shared else BATCH)
                Bs = As if same else members(lambda b: Mzd.random(br_, bc_, 200 + b))
                Cs = members(lambda b: Mzd.random(m, n, 300 + b))

                def ref():
                    out = []
                    for b in range(BATCH):
                        A, B = As[0 if shared else b], Bs[b]
                        A = bits_to(A.to_bits().T.copy()) if ta else A
                        B = bits_to(B.to_bits().T.copy()) if tb else B
                        out.append(oracle.addmul(Cs[b].copy(), A, B) if add else oracle.mul(None, A, B))
                    return out
                want = memo(("bmul", m, l, n, add, ta, tb, shared, same), ref)
                pA = ar.place(c.wins["A"], As, dirty_tail=dirty)
                pB = pA if same else ar.place(c.wins["B"], Bs, dirty_tail=dirty)
                pC = ar.place(c.wins["C"], Cs, dirty_tail=dirty)
                _call(entry, *_ptr_args(pC, c.wins["C"]), *_ptr_args(pA, c.wins["A"]), *_ptr_args(pB, c.wins["B"]), m, l, n, BATCH, *tail_args, None)
                pC.check(want, tail, "C")
                pA.check_unchanged("A")
                pB.check_unchanged("B")
            wins = lay(BS, far, A=(ar_, ac_, "shared") if shared else (ar_, ac_), B=(br_, bc_), C=(m, n))
            if same:
                wins["B"] = wins["A"]
            tag = (f"{entry[9:-4]}-{s}-{m}x{l}x{n}-{path.split(':')[0].replace(' ', '-')}" + (f"-ta{ta}tb{tb}" if ta or tb else "") + ("-shared-A" if shared else "") + ("-A==B" if same else "")
                   + f"-add{add}-far:{far}")
            CASES.append(Case(tag, entry, "batch", BS, (m, l, n), path, wins, tuple(x for x in far if not (shared and x == "A")), run, same=(("A", "B"),) if same else (), plan=plan))

        for add in (0, 1):
            product("m4ri_amd_m4rm_batch_dev", 70, 65, 130, add, (add,), "one batched leaf launch")
            product("m4ri_amd_mul_batch_dev", 70, 65, 130, add, (add, 0), "no level: the batched leaf launch")
            product("m4ri_amd_mul_batch_dev", 256, 256, 256, add, (add, 64), "cutoff 64: two levels, every pass batched", plan=("m4ri_amd_plan_levels", (256, 256, 256, 64), 2))
        product("m4ri_amd_m4rm_batch_dev", 70, 65, 130, 0, (0,), "one batched leaf launch", shared=True)
        # the one-launch products refuse a C whose span meets A's or B's: one far operand at a time
        for (shape, p) in (((33, 64, 17), 0), ((70, 65, 130), 1), ((257, 64, 64), 2)):
            for add in (0, 1):
                for far in "ABC":
                    product("m4ri_amd_mul_small_batch_dev", *shape, add, (add,), f"path{p}: m4ri_amd_plan_mul_small_batch", dirty=p < 2, tail="kept" if p < 2 else "zero",
                            plan=("m4ri_amd_plan_mul_small_batch", shape, p), far=far)
        product("m4ri_amd_mul_small_batch_dev", 33, 64, 17, 0, (0,), "path0: m4ri_amd_plan_mul_small_batch", shared=True, dirty=True, tail="kept", plan=("m4ri_amd_plan_mul_small_batch", (33, 64, 17), 0),
                far="B")
        product("m4ri_amd_mul_small_batch_dev", 64, 64, 64, 0, (0,), "path0: m4ri_amd_plan_mul_small_batch", same=True, tail="kept", plan=("m4ri_amd_plan_mul_small_batch", (64, 64, 64), 0), far="AB")
        for (shape, p) in (((33, 64, 17), 0), ((70, 65, 130), 1)):
            for ta, tb in ((1, 0), (0, 1), (1, 1)):
                for far in "ABC":
                    product("m4ri_amd_mul_small_batch_op_dev", *shape, ta ^ tb, (ta, tb, ta ^ tb), f"path{p}: m4ri_amd_plan_mul_small_batch_op", ta=ta, tb=tb, dirty=True, tail="kept",
                            plan=("m4ri_amd_plan_mul_small_batch_op", shape + (ta, tb), p), far=far)

        for (nr, nc, p) in ((33, 64, 0), (70, 130, 1), (257, 70, 2)):
            for shared, far in ((False, "A"), (False, "D"), (True, "D")):
                def run_tr(ar, oracle, c, nr=nr, nc=nc, p=p, shared=shared):
                    As = members(lambda b: Mzd.random(nr, nc, 400 + b), 1 if shared else BATCH)
                    want = [bits_to(As[0 if shared else b].to_bits().T.copy()) for b in range(BATCH)]
                    pA, pD = ar.place(c.wins["A"], As, dirty_tail=True), ar.place(c.wins["D"], members(lambda b: Mzd.random(nc, nr, 500 + b)), dirty_tail=True)
                    _call("m4ri_amd_transpose_batch_dev", *_ptr_args(pD, c.wins["D"]), *_ptr_args(pA, c.wins["A"]), nr, nc, BATCH, None)
                    pD.check(want, "kept" if p < 2 else "zero", "D")
                    pA.check_unchanged("A")
                CASES.append(Case(f"transpose_batch-{s}-{nr}x{nc}-path{p}-far:{far}" + ("-shared-A" if shared else ""), "m4ri_amd_transpose_batch_dev", "batch", BS, (nr, nc),
                                  f"path{p}: m4ri_amd_plan_transpose_batch", lay(BS, far, A=(nr, nc, "shared") if shared else (nr, nc), D=(nc, nr)), (far,), run_tr,
                                  plan=("m4ri_amd_plan_transpose_batch", (nr, nc), p)))


def _batch_reduce():
    for BS in (BS_ODD, BS_EVEN):
        s = sname(BS)
        for (nr, nc, p) in ((33, 64, 0), (70, 130, 1), (300, 4500, 2)):
            def mats(seed, nr=nr, nc=nc):
                out = []
                for b in range(BATCH):
                    bits = Mzd.random(nr, nc, seed + b).to_bits()
                    bits[: b] = 0                  # leading and trailing zero rows, different in every member
                    bits[nr - 2 * b:] = 0
                    out.append(bits)
                return out

            def run_weight(ar, oracle, c, nr=nr, nc=nc, mats=mats, two=False):
                Ab = mats(600)
                pA = ar.place(c.wins["A"], [bits_to(x) for x in Ab], dirty_tail=True)
                if two:
                    Bb = mats(700)
                    pB = ar.place(c.wins["B"], [bits_to(x) for x in Bb], dirty_tail=True)
                    Ab = [x ^ y for x, y in zip(Ab, Bb)]
                total, roww, light = (torch.full((BATCH,), -7, dtype=torch.int64, device="cuda"), torch.full((BATCH * nr,), -7, dtype=torch.int32, device="cuda"),
                                      torch.full((BATCH,), -7, dtype=torch.int64, device="cuda"))
                wB = c.wins["B"] if two else None
                _call("m4ri_amd_weight_batch_dev", *_ptr_args(pA, c.wins["A"]), pB.ptr if two else None, wB.stride if two else 0, wB.bs if two else 0, nr, nc, BATCH,
                      total.data_ptr(), roww.data_ptr(), light.data_ptr(), None)
                assert _host(total).tolist() == [rc.total(x) for x in Ab]
                assert np.array_equal(_host(roww), np.concatenate([rc.row_weights(x) for x in Ab]))
                assert _host(light).tolist() == [rc.lightest(x) for x in Ab]
                pA.check_unchanged("A")
                if two:
                    pB.check_unchanged("B")

            def run_mismatch(ar, oracle, c, nr=nr, nc=nc, mats=mats):
                Ab = mats(600)
                Bb = [x.copy() for x in Ab]
                Bb[1][nr // 2, nc - 1] ^= 1
                Bb[3][nr - 1, 0] ^= 1
                pA, pB = ar.place(c.wins["A"], [bits_to(x) for x in Ab], dirty_tail=True), ar.place(c.wins["B"], [bits_to(x) for x in Bb], dirty_tail=True)
                first = torch.full((BATCH,), -7, dtype=torch.int32, device="cuda")
                _call("m4ri_amd_mismatch_batch_dev", *_ptr_args(pA, c.wins["A"]), *_ptr_args(pB, c.wins["B"]), nr, nc, BATCH, first.data_ptr(), None)
                assert _host(first).tolist() == [-1, nr // 2, -1, nr - 1]
                assert _host(first).tolist() == [rc.first_mismatch(x, y) for x, y in zip(Ab, Bb)]
                pA.check_unchanged("A")
                pB.check_unchanged("B")

            def run_span(ar, oracle, c, nr=nr, nc=nc, mats=mats):
                Ab = mats(600)
                pA = ar.place(c.wins["A"], [bits_to(x) for x in Ab], dirty_tail=True)
                fn, en = torch.full((BATCH,), -7, dtype=torch.int32, device="cuda"), torch.full((BATCH,), -7, dtype=torch.int32, device="cuda")
                _call("m4ri_amd_row_span_batch_dev", *_ptr_args(pA, c.wins["A"]), nr, nc, BATCH, fn.data_ptr(), en.data_ptr(), None)
                assert _host(fn).tolist() == [rc.first_nonzero(x) for x in Ab] and _host(en).tolist() == [rc.end_nonzero(x) for x in Ab]
                pA.check_unchanged("A")
            plan = ("m4ri_amd_plan_reduce_batch", (nr, nc), p)
            path = f"path{p}: m4ri_amd_plan_reduce_batch"
            one, two = {"A": M_(0, nr, nc, BS)}, {"A": M_(0, nr, nc, BS), "B": M_(1, nr, nc, BS)}
            CASES.append(Case(f"weight_batch-{s}-{nr}x{nc}-path{p}", "m4ri_amd_weight_batch_dev", "batch", BS, (nr, nc), path, one, ("A",), run_weight, plan=plan))
            CASES.append(Case(f"weight_batch-{s}-{nr}x{nc}-path{p}-distance", "m4ri_amd_weight_batch_dev", "batch", BS, (nr, nc), path, two, ("A", "B"),
                              lambda ar, o, c, f=run_weight: f(ar, o, c, two=True), plan=plan))
            CASES.append(Case(f"mismatch_batch-{s}-{nr}x{nc}-path{p}", "m4ri_amd_mismatch_batch_dev", "batch", BS, (nr, nc), path, two, ("A", "B"), run_mismatch, plan=plan))
            CASES.append(Case(f"row_span_batch-{s}-{nr}x{nc}-path{p}", "m4ri_amd_row_span_batch_dev", "batch", BS, (nr, nc), path, one, ("A",), run_span, plan=plan))


def _batch_assemble():
    for BS in (BS_ODD, BS_EVEN):
        s = sname(BS)
        for tag, (d_row, d_col, a_row, a_col, rows, cols) in (("any-bit", (3, 5, 2, 70, 60, 120)), ("word-aligned", (4, 64, 2, 128, 60, 128))):
            def run_copy(ar, oracle, c, g=(d_row, d_col, a_row, a_col, rows, cols)):
                Ab, Db = members(lambda b: Mzd.random(70, 300, 800 + b).to_bits()), members(lambda b: Mzd.random(80, 300, 900 + b).to_bits())
                want = [bits_to(ac.copy_block(D, g[0], g[1], A, g[2], g[3], g[4], g[5])) for A, D in zip(Ab, Db)]
                pA, pD = ar.place(c.wins["A"], [bits_to(x) for x in Ab], dirty_tail=True), ar.place(c.wins["D"], [bits_to(x) for x in Db], dirty_tail=True)
                wD, wA = c.wins["D"], c.wins["A"]
                _call("m4ri_amd_copy_block_batch_dev", pD.ptr, wD.stride, wD.bs, g[0], g[1], pA.ptr, wA.stride, wA.bs, g[2], g[3], g[4], g[5], BATCH, None)
                pD.check(want, "kept", "D")
                pA.check_unchanged("A")
            for far in "AD":
                CASES.append(Case(f"copy_block_batch-{s}-{tag}-far:{far}", "m4ri_amd_copy_block_batch_dev", "batch", BS, (rows, cols),
                                  "funnel shift" if tag == "any-bit" else "whole words (16-byte where even)", lay(BS, far, A=(70, 300), D=(80, 300)), (far,), run_copy))
        for upper in (0, 1):
            def run_tri(ar, oracle, c, upper=upper):
                nr, nc = 70, 130
                Ab = members(lambda b: Mzd.random(nr, nc, 1000 + b).to_bits())
                want = [bits_to(ac.triangle(A, upper, 2)) for A in Ab]
                dr, dc = (nr, nc) if upper else (nr, nr)
                pA, pD = ar.place(c.wins["A"], [bits_to(x) for x in Ab], dirty_tail=True), ar.place(c.wins["D"], members(lambda b: Mzd.random(dr, dc, 1100 + b)), dirty_tail=True)
                _call("m4ri_amd_extract_tri_batch_dev", *_ptr_args(pD, c.wins["D"]), *_ptr_args(pA, c.wins["A"]), nr, nc, BATCH, upper, 2, None, None)
                pD.check(want, "kept", "D")
                pA.check_unchanged("A")
            for far in "AD":
                CASES.append(Case(f"extract_tri_batch-{s}-{'upper' if upper else 'lower'}-far:{far}", "m4ri_amd_extract_tri_batch_dev", "batch", BS, (70, 130), "the block copy's kernel with a row mask",
                                  lay(BS, far, A=(70, 130), D=(70, 130 if upper else 70)), (far,), run_tri))
        for right in (0, 1):
            for (nr, nc, p) in ((33, 64, 0), (70, 130, 1), (300, 4500, 2)):
                for trans in (0, 1):
                    entry = "m4ri_amd_apply_p_right_batch_dev" if right else "m4ri_amd_apply_p_left_batch_dev"

                    def run_perm(ar, oracle, c, right=right, nr=nr, nc=nc, p=p, trans=trans, entry=entry):
                        n = nc if right else nr
                        rng = np.random.default_rng(12 + n)
                        P = np.stack([np.array([rng.integers(i, n) for i in range(n)], dtype=np.int32) for _ in range(BATCH)])
                        Ab = members(lambda b: Mzd.random(nr, nc, 1200 + b).to_bits())
                        want = [bits_to(ac.apply_p(A, P[b], n, bool(right), bool(trans))) for b, A in enumerate(Ab)]
                        pA = ar.place(c.wins["A"], [bits_to(x) for x in Ab], dirty_tail=p < 2)
                        dP, st = _dev(P.reshape(-1)), torch.full((BATCH,), -7, dtype=torch.int32, device="cuda")
                        _call(entry, *_ptr_args(pA, c.wins["A"]), nr, nc, BATCH, dP.data_ptr(), n, n, trans, st.data_ptr(), None)
                        assert _host(st).tolist() == [0] * BATCH
                        pA.check(want, "kept" if p < 2 else "zero", "A")
                    CASES.append(Case(f"{entry[9:-4]}-{s}-{nr}x{nc}-path{p}-trans{trans}", entry, "batch", BS, (nr, nc), f"path{p}: m4ri_amd_plan_perm_batch", {"A": M_(0, nr, nc, BS)}, ("A",),
                                      run_perm, plan=("m4ri_amd_plan_perm_batch", (nr, nc, right), p)))


def _batch_elimination():
    for BS in (BS_ODD, BS_EVEN):
        s = sname(BS)
        for (nr, nc, p) in ((33, 64, 0), (70, 130, 1), (300, 4500, 2), (300, 14100, 3)):
            kinds = ("random", "lowrank", "random", "lowrank")
            for full in (0, 1):
                def run_ech(ar, oracle, c, nr=nr, nc=nc, p=p, full=full, kinds=kinds):
                    As = memo(("members", nr, nc), lambda: members(lambda b: _make(kinds[b], nr, nc, 1300 + b)))

                    def ref():
                        out = [A.copy() for A in As]
                        return out, [oracle.echelonize(x, full) for x in out]
                    want, ranks = memo(("bech", nr, nc, full), ref)
                    pA = ar.place(c.wins["A"], As, dirty_tail=p < 3)
                    rk = torch.full((BATCH,), -7, dtype=torch.int32, device="cuda")
                    _call("m4ri_amd_echelonize_batch_dev", *_ptr_args(pA, c.wins["A"]), nr, nc, BATCH, full, rk.data_ptr(), None, None)
                    assert _host(rk).tolist() == ranks
                    pA.check(want, "kept" if p < 3 else "zero", "A")
                CASES.append(Case(f"echelonize_batch-{s}-{nr}x{nc}-path{p}-full{full}", "m4ri_amd_echelonize_batch_dev", "batch", BS, (nr, nc), f"path{p}: m4ri_amd_plan_echelonize_batch",
                                  {"A": M_(0, nr, nc, BS)}, ("A",), run_ech, plan=("m4ri_amd_plan_echelonize_batch", (nr, nc), p)))
            for pluq in (0, 1):
                def run_ple(ar, oracle, c, nr=nr, nc=nc, p=p, pluq=pluq, kinds=kinds):
                    As = memo(("members", nr, nc), lambda: members(lambda b: _make(kinds[b], nr, nc, 1300 + b)))

                    def ref():
                        out = [A.copy() for A in As]
                        return out, [oracle.ple(x, pluq=bool(pluq)) for x in out]
                    want, rpq = memo(("bple", nr, nc, pluq), ref)
                    pA = ar.place(c.wins["A"], As, dirty_tail=p < 3)
                    rk, dP, dQ = (torch.full((BATCH,), -7, dtype=torch.int32, device="cuda"), torch.full((BATCH * nr,), -7, dtype=torch.int32, device="cuda"),
                                  torch.full((BATCH * nc,), -7, dtype=torch.int32, device="cuda"))
                    _call("m4ri_amd_ple_batch_dev", *_ptr_args(pA, c.wins["A"]), nr, nc, BATCH, pluq, dP.data_ptr(), dQ.data_ptr(), rk.data_ptr(), None)
                    assert _host(rk).tolist() == [r for r, _, _ in rpq]
                    assert np.array_equal(_host(dP), np.concatenate([P for _, P, _ in rpq])) and np.array_equal(_host(dQ), np.concatenate([Q for _, _, Q in rpq]))
                    pA.check(want, "kept" if p < 3 else "zero", "A")
                CASES.append(Case(f"ple_batch-{s}-{nr}x{nc}-path{p}-pluq{pluq}", "m4ri_amd_ple_batch_dev", "batch", BS, (nr, nc), f"path{p}: m4ri_amd_plan_ple_batch", {"A": M_(0, nr, nc, BS)}, ("A",),
                                  run_ple, plan=("m4ri_amd_plan_ple_batch", (nr, nc), p)))

        # systems: members 0 and 2 consistent, 1 and 3 not (a low-rank A and a random right-hand side)
        def systems(oracle, m, n, k, seed):
            As = members(lambda b: _make("lowrank", m, n, seed + b))
            Bs = [_rhs(oracle, As[b], max(m, n), k, b % 2 == 0, seed + 10 + b) for b in range(BATCH)]
            return As, Bs

        for (m, n, k, p) in ((40, 33, 17, 0), (70, 65, 130, 1), (300, 300, 4200, 2)):
            for shared in (False, True):
                def run_solve(ar, oracle, c, m=m, n=n, k=k, shared=shared):
                    As, Bs = systems(oracle, m, n, k, 1500)
                    if shared:
                        As = [As[0]] * BATCH
                        Bs = [_rhs(oracle, As[0], max(m, n), k, b % 2 == 0, 1510 + b) for b in range(BATCH)]

                    def ref():
                        out, st, rk = [], [], []
                        for A, B in zip(As, Bs):
                            Ao, Bo = A.copy(), B.copy()
                            st.append(oracle.solve_left(Ao, Bo, True))
                            out.append(Bo if st[-1] == 0 else B)
                            rk.append(oracle.echelonize(A.copy(), 0))
                        return out, st, rk
                    want, status, ranks = memo(("bsolve", m, n, k, shared), ref)
                    assert status == [0, -1, 0, -1]
                    pA, pB = ar.place(c.wins["A"], As[:1] if shared else As), ar.place(c.wins["B"], Bs, dirty_tail=True)
                    st, rk = torch.full((BATCH,), -7, dtype=torch.int32, device="cuda"), torch.full((BATCH,), -7, dtype=torch.int32, device="cuda")
                    _call("m4ri_amd_solve_left_batch_dev", *_ptr_args(pA, c.wins["A"]), m, n, *_ptr_args(pB, c.wins["B"]), k, BATCH, st.data_ptr(), rk.data_ptr(), None)
                    assert _host(st).tolist() == status and _host(rk).tolist() == ranks
                    pB.check(want, "kept", "B")
                    pA.check_unchanged("A")
                CASES.append(Case(f"solve_left_batch-{s}-{m}x{n}x{k}-path{p}" + ("-shared-A" if shared else ""), "m4ri_amd_solve_left_batch_dev", "batch", BS, (m, n, k),
                                  f"path{p}: m4ri_amd_plan_solve_batch", {"A": M_(0, m, n, BS, shared=shared), "B": M_(1, max(m, n), k, BS)}, ("B",) if shared else ("A", "B"), run_solve,
                                  plan=("m4ri_amd_plan_solve_batch", (m, n, k), p)))

        for (m, n, k, p) in ((40, 33, 17, 0), (70, 65, 130, 1), (300, 300, 4500, 2)):
            def run_pluq_solve(ar, oracle, c, m=m, n=n, k=k):
                As, Bs = systems(oracle, m, n, k, 1600)

                def ref():
                    out, st, fac = [], [], []
                    for A, B in zip(As, Bs):
                        Ad, Bo = A.copy(), B.copy()
                        r, P, Q = oracle.ple(Ad, pluq=True)
                        st.append(oracle.pluq_solve_left(Ad, r, P, Q, Bo, True))
                        out.append(Bo if st[-1] == 0 else B)
                        fac.append((Ad, r, P, Q))
                    return out, st, fac
                want, status, fac = memo(("bpluqsolve", m, n, k), ref)
                assert status == [0, -1, 0, -1]
                pA, pB = ar.place(c.wins["A"], [f[0] for f in fac]), ar.place(c.wins["B"], Bs, dirty_tail=True)
                rk, dP, dQ = _dev([f[1] for f in fac]), _dev(np.concatenate([f[2] for f in fac])), _dev(np.concatenate([f[3] for f in fac]))
                st = torch.full((BATCH,), -7, dtype=torch.int32, device="cuda")
                _call("m4ri_amd_pluq_solve_left_batch_dev", *_ptr_args(pA, c.wins["A"]), m, n, rk.data_ptr(), dP.data_ptr(), dQ.data_ptr(), *_ptr_args(pB, c.wins["B"]), k, BATCH,
                      st.data_ptr(), None)
                assert _host(st).tolist() == status
                pB.check(want, "kept", "B")
                pA.check_unchanged("A")
            for far in "AB":   # B's span must not meet A's: one far operand at a time
                CASES.append(Case(f"pluq_solve_left_batch-{s}-{m}x{n}x{k}-path{p}-far:{far}", "m4ri_amd_pluq_solve_left_batch_dev", "batch", BS, (m, n, k), f"path{p}: m4ri_amd_plan_pluq_solve_batch",
                                  lay(BS, far, A=(m, n), B=(max(m, n), k)), (far,), run_pluq_solve, plan=("m4ri_amd_plan_pluq_solve_batch", (m, n, k), p)))

        for (n, p) in ((33, 0), (70, 1), (769, 2)):
            def run_inv(ar, oracle, c, n=n, inplace=False):
                def make():
                    As = [_invertible(oracle, n, 1700 + 100 * b) for b in range(BATCH)]
                    As[1].valid_words()[n // 2] = As[1].valid_words()[0]     # members 1 and 3 singular
                    As[3].valid_words()[n - 1] = 0
                    return As, [oracle.inv(A) for A in As], [oracle.echelonize(A.copy(), 0) for A in As]
                As, want, ranks = memo(("binv", n), make)
                assert ranks[0] == ranks[2] == n and ranks[1] < n and ranks[3] < n
                pA = ar.place(c.wins["A"], As)
                pB = pA if inplace else ar.place(c.wins["Binv"], members(lambda b: Mzd.random(n, n, 1800 + b)), dirty_tail=True)
                rk = torch.full((BATCH,), -7, dtype=torch.int32, device="cuda")
                _call("m4ri_amd_inv_batch_dev", *_ptr_args(pB, c.wins["Binv"]), *_ptr_args(pA, c.wins["A"]), n, BATCH, rk.data_ptr(), None)
                assert _host(rk).tolist() == ranks
                pB.check(want, "kept", "Binv")
                if not inplace:
                    pA.check_unchanged("A")
            for far in ("A", "Binv"):   # Binv's span must not meet A's, unless the call is in place
                CASES.append(Case(f"inv_batch-{s}-{n}-path{p}-far:{far}", "m4ri_amd_inv_batch_dev", "batch", BS, (n,), f"path{p}: m4ri_amd_plan_solve_batch", lay(BS, (far,), A=(n, n), Binv=(n, n)),
                                  (far,), run_inv, plan=("m4ri_amd_plan_solve_batch", (n, n, n), p)))
            w = M_(0, n, n, BS)
            CASES.append(Case(f"inv_batch-{s}-{n}-path{p}-in-place", "m4ri_amd_inv_batch_dev", "batch", BS, (n,), f"path{p}: m4ri_amd_plan_solve_batch", {"A": w, "Binv": w}, ("A",),
                              lambda ar, o, c, f=run_inv: f(ar, o, c, inplace=True), same=(("A", "Binv"),), plan=("m4ri_amd_plan_solve_batch", (n, n, n), p)))

        for (m, n, kc, p) in ((33, 40, 40, 0), (70, 130, 70, 1), (300, 4500, 130, 2)):
            for shared in (False, True):
                def run_kernel(ar, oracle, c, m=m, n=n, kc=kc, shared=shared):
                    kinds = ("random", "lowrank", "random", "lowrank")
                    As = members(lambda b: _make(kinds[b], m, n, 1900 + b), 1 if shared else BATCH)

                    def ref():
                        out, rk = [], []
                        for A in As:
                            r, Ro = oracle.kernel_left_pluq(A.copy())
                            bits = np.zeros((n, kc), dtype=np.uint8)
                            if Ro is not None:
                                take = min(kc, n - r)
                                bits[:, :take] = Ro.to_bits()[:, :take]
                            out.append(bits_to(bits))
                            rk.append(r)
                        return out * (BATCH if shared else 1), rk * (BATCH if shared else 1)
                    want, ranks = memo(("bkernel", m, n, kc, shared), ref)
                    pA, pR = ar.place(c.wins["A"], As), ar.place(c.wins["R"], members(lambda b: Mzd.random(n, kc, 2000 + b)), dirty_tail=True)
                    rk = torch.full((BATCH,), -7, dtype=torch.int32, device="cuda")
                    _call("m4ri_amd_kernel_left_batch_dev", *_ptr_args(pA, c.wins["A"]), m, n, *_ptr_args(pR, c.wins["R"]), kc, BATCH, rk.data_ptr(), None)
                    assert _host(rk).tolist() == ranks
                    pR.check(want, "kept", "R")
                    pA.check_unchanged("A")
                if shared and p != 1:
                    continue
                for far in ("R",) if shared else ("A", "R"):   # R's span must not meet A's: one far operand at a time
                    CASES.append(Case(f"kernel_left_batch-{s}-{m}x{n}-kc{kc}-path{p}-far:{far}" + ("-shared-A" if shared else ""), "m4ri_amd_kernel_left_batch_dev", "batch", BS, (m, n, kc),
                                      f"path{p}: m4ri_amd_plan_kernel_batch", lay(BS, far, A=(m, n, "shared") if shared else (m, n), R=(n, kc)), (far,), run_kernel,
                                      plan=("m4ri_amd_plan_kernel_batch", (m, n), p)))


# ================================================ batches with far rows; refusals ====================================================

def _batch_far_rows():
    """Two members of 300 x 300 x 300, rows a far stride apart, the members next to each other inside the pitch: members too large
    for the batched leaf launch, which `batch` single calls cut into chunks."""
    for S in (S_ODD, S_EVEN):
        for entry, tail_args in (("m4ri_amd_m4rm_batch_dev", ()), ("m4ri_amd_mul_batch_dev", (0,))):
            for add in (0, 1):
                def run(ar, oracle, c, entry=entry, tail_args=tail_args, add=add):
                    As, Bs, Cs = members(lambda b: Mzd.random(300, 300, 100 + b), 2), members(lambda b: Mzd.random(300, 300, 200 + b), 2), members(lambda b: Mzd.random(300, 300, 300 + b), 2)
                    want = memo(("bfar", add), lambda: [oracle.addmul(Cs[b].copy(), As[b], Bs[b]) if add else oracle.mul(None, As[b], Bs[b]) for b in range(2)])
                    pA, pB, pC = ar.place(c.wins["A"], As), ar.place(c.wins["B"], Bs), ar.place(c.wins["C"], Cs)
                    _call(entry, *_ptr_args(pC, c.wins["C"]), *_ptr_args(pA, c.wins["A"]), *_ptr_args(pB, c.wins["B"]), 300, 300, 300, 2, add, *tail_args, None)
                    pC.check(want, "zero", "C")
                    pA.check_unchanged("A")
                    pB.check_unchanged("B")
                wins = {x: Win(4096 * i, 300, 5, S, 2, 3 * 4096) for i, x in enumerate("ABC")}
                CASES.append(Case(f"{entry[9:-4]}-{sname(S)}-far-rows-batch2-add{add}", entry, "rows", S, (300, 300, 300), "members beyond one descriptor: one by one through the cuts",
                                  wins, ("A", "B", "C"), run, b_sides=("B",)))


def _refusals():
    """A B side whose smallest chunk launch_leaf cannot address: hipErrorInvalidValue from all four product calls, at every depth
    (cutoff 0: no level; cutoff 64: two levels, on a ragged shape with strips and on an even one without), before anything is
    written -- C is never placed, so the pattern check after the case holds it to that.  `far`: A and C lie at the refused stride
    as well, so that the member loop and the row cut of launch_leaf come before the refusal."""
    forms = (("m4ri_amd_mul_dev", 1, (0, 0), 300, False), ("m4ri_amd_m4rm_dev", 1, (0, 0), 300, False), ("m4ri_amd_m4rm_batch_dev", 2, (0,), 300, False),
             ("m4ri_amd_mul_batch_dev", 2, (0, 0), 300, False),
             ("m4ri_amd_mul_dev", 1, (0, 64), 300, False), ("m4ri_amd_mul_dev", 1, (0, 64), 256, False), ("m4ri_amd_mul_dev", 1, (1, 64), 256, True),
             ("m4ri_amd_mul_batch_dev", 2, (0, 64), 300, False), ("m4ri_amd_mul_batch_dev", 2, (0, 64), 256, False),
             ("m4ri_amd_mul_dev", 1, (0, 0), 300, True), ("m4ri_amd_m4rm_dev", 1, (1, 0), 300, True), ("m4ri_amd_m4rm_batch_dev", 2, (0,), 300, True),
             ("m4ri_amd_mul_batch_dev", 2, (1, 0), 300, True), ("m4ri_amd_mul_batch_dev", 2, (0, 64), 256, True))
    for entry, batch, tail_args, d, far in forms:
        def run(ar, oracle, c, entry=entry, batch=batch, tail_args=tail_args, d=d):
            pA = ar.place(c.wins["A"], members(lambda b: Mzd.random(d, d, 100 + b), batch))
            pB = ar.place(c.wins["B"], members(lambda b: Mzd.random(d, d, 200 + b), batch))
            wA, wB, wC = c.wins["A"], c.wins["B"], c.wins["C"]
            if batch == 1:
                got = getattr(m4ri_amd.lib(), entry)(ar.ptr(wC), wC.stride, pA.ptr, wA.stride, pB.ptr, wB.stride, d, d, d, *tail_args, None)
            else:
                got = getattr(m4ri_amd.lib(), entry)(ar.ptr(wC), wC.stride, wC.bs, pA.ptr, wA.stride, wA.bs, pB.ptr, wB.stride, wB.bs, d, d, d, batch, *tail_args, None)
            torch.cuda.synchronize()
            assert got == INVALID, (entry, got)
            pA.check_unchanged("A")
            pB.check_unchanged("B")      # C was never placed: the pattern check that follows holds it to "nothing written"
        w = words(d)
        if far:
            wins = {x: Win(4096 * i, d, w, S_REFUSED, batch, 3 * 4096 if batch > 1 else 0) for i, x in enumerate("ABC")}
        else:
            kb = {"batch": batch, "bs": (1 << 17) if batch > 1 else 0}
            wins = {"A": Win((1 << 20), d, w, w + 1, **kb), "B": Win(0, d, w, S_REFUSED, batch, 4096 if batch > 1 else 0), "C": Win((1 << 20) + (1 << 18), d, w, w + 1, **kb)}
        depth = "cutoff64-" + ("ragged" if d == 300 else "even") if tail_args[-1] == 64 else "no-level"
        unreached, label = ({"int32-words": "256 rows at S_REFUSED: 255 * 8 388 609 < 2^31"}, "refused, 256 rows") if d == 256 else ({}, "")
        CASES.append(Case(f"refused-{entry[9:-4]}-{d}-{depth}-add{tail_args[0]}-" + ("A-B-C" if far else "B") + "-at-S_REFUSED", entry, "rows", S_REFUSED, (d, d, d),
                          "64 rows of B beyond the limit: hipErrorInvalidValue, nothing written", wins, ("A", "B", "C") if far else ("B",), run, b_sides=("B",), refused=True,
                          unreached=unreached, label=label))
    m = l = n = 300
    for entry, cutoff in (("m4ri_amd_mul_dev", 0), ("m4ri_amd_m4rm_dev", 0), ("m4ri_amd_mul_dev", 64)):
        wins = {"A": F(0, m, l, S_REFUSED), "B": K(1, l, n), "C": F(2, m, n, S_REFUSED)}
        CASES.append(Case(f"{entry[9:-4]}-A-and-C-at-S_REFUSED-cutoff{cutoff}", entry, "rows", S_REFUSED, (m, l, n), "rows of A are cut one by one: legal", wins, ("A", "C"),
                          _run_product(entry, m, l, n, 0, cutoff, False), b_sides=("B",)))


for build in (_products, _elementwise, _triangular, _tables, _drivers, _batch_products, _batch_reduce, _batch_assemble, _batch_elimination, _batch_far_rows, _refusals):
    build()
assert len({c.id for c in CASES}) == len(CASES)
ARENA_WORDS = fa.arena_words([w for c in CASES for w in c.wins.values()])


# ================================================ the test ==============================================================================

@pytest.fixture(scope="module")
def arena():
    assert m4ri_amd.lib().m4ri_amd_device_count() >= 1, "no HIP device visible: the gpu tests have nothing to run on"
    m4ri_amd.init(0)
    torch.cuda.set_device(0)
    free, _ = torch.cuda.mem_get_info()
    need = 8 * ARENA_WORDS + HEADROOM
    assert free >= need, f"the far-operand arena needs {need / 2**30:.1f} GiB of free device memory ({8 * ARENA_WORDS / 2**30:.1f} GiB arena + 8 GiB), {free / 2**30:.1f} GiB are free"
    ar = fa.Arena(ARENA_WORDS)
    ar.assert_pattern("after the fill")
    yield ar
    del ar.t
    del ar
    _memo.clear()
    torch.cuda.empty_cache()


@pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
def test_far_operands(case, arena, oracle):
    try:
        case.run(arena, oracle, case)
    finally:
        torch.cuda.synchronize()
        arena.restore()
        try:
            arena.assert_pattern(case.id)
        except AssertionError:
            arena.fill()   # one failure must not cascade into the cases after it
            raise
