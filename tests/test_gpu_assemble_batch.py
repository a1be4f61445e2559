"""The calls of assemble_batch.hip on the GPU (include/m4ri_amd.h): block copies at any bit offset with their three compositions, the
triangles of a factored member, the batched permutations on every path, and two chains whose results never leave the device.  Every
operand holds random bits everywhere -- valid bits, tail bits, padding words, gaps between members, guard words around the batch --
and every written buffer is compared word for word with an expected image made in NumPy (tests/assemble_cases.py), so a stray write
anywhere fails; read-only operands must come back unchanged."""
import numpy as np
import pytest
import torch

import assemble_cases as ac
import m4ri_amd
from assemble_cases import Batch

pytestmark = pytest.mark.gpu
PATH0, PATH1 = "M4RI_AMD_PERM_BATCH_PATH0_MAX", "M4RI_AMD_PERM_BATCH_PATH1_MAX"


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    assert m4ri_amd.lib().m4ri_amd_device_count() >= 1, "no HIP device visible: the gpu tests have nothing to run on"
    m4ri_amd.init(0)
    torch.cuda.set_device(0)


def _i32(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).cuda()


# ---- the block copy ---------------------------------------------------------------------------------------------------------------

def _copy_case(A, d_col, a_col, rows, cols, d_row, a_row, batch, seed, what, **geometry):
    """One call from the uploaded batch A into a fresh D, the whole image of D checked."""
    D = Batch(d_row + rows + 2, d_col + cols + 70, batch, seed, **geometry).upload()
    exp = D.bits.copy()
    for b in range(batch):
        src = A.member(A.bits, b if A.bs else 0)
        D.member(exp, b)[d_row:d_row + rows, d_col:d_col + cols] = src[a_row:a_row + rows, a_col:a_col + cols]
    m4ri_amd.copy_block_batch_dev(D.ptr, D.stride, D.bs, d_row, d_col, A.ptr, A.stride, A.bs, a_row, a_col, rows, cols, batch)
    torch.cuda.synchronize()
    D.check(exp, what)


@pytest.mark.parametrize("a_col", ac.COPY_COL_OFFSETS)
@pytest.mark.parametrize("d_col", ac.COPY_COL_OFFSETS)
def test_block_copy_at_every_offset(d_col, a_col):
    """Every cols x rows x row offset of the lists at this pair of column offsets, batch 3 with odd strides and gaps; among them the
    blocks whose last destination word takes its bits from one source word (d_col = 1, a_col = 0, cols = 64) and the blocks inside
    one destination word (d_col = 1, cols = 1).  The row offset 3 also runs with one shared A (a_bs = 0)."""
    seed = 1000 + 10 * d_col + a_col
    A = Batch(3 + 65 + 1, 65 + 129 + 3, 3, seed).upload()
    S = Batch(3 + 65 + 1, 65 + 129 + 3, 3, seed + 1, shared=True).upload()
    n = 0
    for cols in ac.COPY_COLS:
        for rows in ac.COPY_ROWS:
            for off in ac.COPY_ROW_OFFSETS:
                n += 1
                _copy_case(A, d_col, a_col, rows, cols, off, off, 3, seed + 7 * n, (cols, rows, off))
                if off:
                    _copy_case(S, d_col, a_col, rows, cols, 0, off, 3, seed + 7 * n + 1, (cols, rows, off, "shared"))
    A.check_unchanged()
    S.check_unchanged()


@pytest.mark.parametrize("d_col,a_col,cols", [(5, 40, 20), (5, 50, 20), (62, 0, 1), (0, 63, 1), (10, 10, 54), (1, 0, 64), (0, 1, 64), (63, 62, 66)])
def test_block_copy_edge_words(d_col, a_col, cols):
    """Blocks inside a single destination word with both edge masks in it (from one source word and from two), and blocks whose last
    destination word is fed by exactly one source word."""
    A = Batch(9, 200, 3, 2000 + d_col).upload()
    _copy_case(A, d_col, a_col, 5, cols, 2, 1, 3, 2100 + a_col, (d_col, a_col, cols))
    A.check_unchanged()


@pytest.mark.parametrize("d_col,a_col", [(0, 0), (0, 64), (64, 0), (128, 64)])
@pytest.mark.parametrize("cols", [64, 128, 129, 192, 200, 256])
def test_block_copy_16_byte_path(d_col, a_col, cols):
    """Word-aligned offsets, even strides and batch strides, 16-byte aligned bases: the pairs of words, a masked and an odd last one."""
    g = dict(pad=words_even_pad(a_col + cols + 70), gap=4, base=6)
    A = Batch(68, a_col + cols + 70, 3, 2200 + cols, **g).upload()
    assert A.ptr % 16 == 0 and A.stride % 2 == 0 and A.bs % 2 == 0
    _copy_case(A, d_col, a_col, 65, cols, 1, 2, 3, 2300 + cols, (d_col, a_col, cols), pad=words_even_pad(d_col + cols + 70), gap=4, base=6)
    _copy_case(A, d_col, a_col, 65, cols, 1, 2, 3, 2300 + cols, (d_col, a_col, cols, "odd D"))   # and D on the 8-byte path
    A.check_unchanged()


def words_even_pad(ncols):
    return 2 - ac.words(ncols) % 2


def test_block_copy_of_1000_by_1000_at_shift_13():
    A = Batch(1003, 1100, 2, 2400).upload()
    _copy_case(A, 13, 26, 1000, 1000, 1, 3, 2, 2401, "1000 x 1000")
    _copy_case(A, 0, 13, 1000, 1000, 0, 0, 2, 2402, "mzd_submatrix at column 13")
    A.check_unchanged()


def test_batch_zero_and_empty_blocks_touch_nothing():
    A, D = Batch(8, 100, 2, 2500).upload(), Batch(8, 100, 2, 2501).upload()
    m4ri_amd.copy_block_batch_dev(D.ptr, D.stride, D.bs, 0, 0, A.ptr, A.stride, A.bs, 0, 0, 8, 100, 0)
    m4ri_amd.copy_block_batch_dev(D.ptr, D.stride, D.bs, 1, 3, A.ptr, A.stride, A.bs, 0, 0, 0, 50, 2)
    m4ri_amd.copy_block_batch_dev(D.ptr, D.stride, D.bs, 1, 3, A.ptr, A.stride, A.bs, 0, 0, 5, 0, 2)
    m4ri_amd.extract_tri_batch_dev(D.ptr, D.stride, D.bs, A.ptr, A.stride, A.bs, 8, 100, 0, True)
    m4ri_amd.apply_p_left_batch_dev(D.ptr, D.stride, D.bs, 8, 100, 0, A.ptr, 8, 8)
    torch.cuda.synchronize()
    D.check_unchanged()
    A.check_unchanged()


def test_python_compositions_match_numpy():
    """submatrix_batch_dev, concat_batch_dev and stack_batch_dev against NumPy's slicing, hstack and vstack."""
    batch = 3
    A, B = Batch(70, 130, batch, 2600).upload(), Batch(70, 77, batch, 2601).upload()
    S = Batch(64, 100, batch, 2602).upload()
    exp = S.bits.copy()
    for b in range(batch):
        S.member(exp, b)[:, :100] = A.valid(b)[3:67, 17:117]
    m4ri_amd.submatrix_batch_dev(S.ptr, S.stride, S.bs, A.ptr, A.stride, A.bs, 3, 17, 67, 117, batch)
    C = Batch(70, 207, batch, 2603).upload()
    expc = C.bits.copy()
    for b in range(batch):
        C.member(expc, b)[:, :207] = np.hstack([A.valid(b), B.valid(b)])
    m4ri_amd.concat_batch_dev(C.ptr, C.stride, C.bs, A.ptr, A.stride, A.bs, 130, B.ptr, B.stride, B.bs, 77, 70, batch)
    B2 = Batch(33, 130, batch, 2604).upload()
    T = Batch(103, 130, batch, 2605).upload()
    expt = T.bits.copy()
    for b in range(batch):
        T.member(expt, b)[:, :130] = np.vstack([A.valid(b), B2.valid(b)])
    m4ri_amd.stack_batch_dev(T.ptr, T.stride, T.bs, A.ptr, A.stride, A.bs, 70, B2.ptr, B2.stride, B2.bs, 33, 130, batch)
    torch.cuda.synchronize()
    S.check(exp, "submatrix")
    C.check(expc, "concat")
    T.check(expt, "stack")
    for X in (A, B, B2):
        X.check_unchanged()


# ---- the triangles ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("nrows,ncols", ac.TRI_SHAPES)
def test_triangles(nrows, ncols):
    """Both triangles, the three diagonal rules, without a rank and with the rank array 0, 1, 64, k, k + 3."""
    k, batch = min(nrows, ncols), 5
    A = Batch(nrows, ncols, batch, 3000 + nrows + ncols).upload()
    ranks = ac.tri_ranks(k)
    rk = _i32(ranks)
    n = 0
    for upper in (True, False):
        for diag in (0, 1, 2):
            for with_rank in (False, True):
                n += 1
                D = Batch(k if upper else nrows, ncols if upper else k, batch, 3100 + n).upload()
                exp = D.bits.copy()
                for b in range(batch):
                    D.member(exp, b)[:, :D.ncols] = ac.triangle(A.valid(b), upper, diag, ranks[b] if with_rank else None)
                m4ri_amd.extract_tri_batch_dev(D.ptr, D.stride, D.bs, A.ptr, A.stride, A.bs, nrows, ncols, batch, upper, diag,
                                               rk.data_ptr() if with_rank else 0)
                torch.cuda.synchronize()
                D.check(exp, (upper, diag, with_rank))
    A.check_unchanged()
    assert np.array_equal(rk.cpu().numpy(), ranks)


def test_triangle_of_one_shared_member():
    A = Batch(65, 65, 3, 3200, shared=True).upload()
    D = Batch(65, 65, 3, 3201).upload()
    exp = D.bits.copy()
    for b in range(3):
        D.member(exp, b)[:, :65] = ac.triangle(A.valid(0), False, 1)
    m4ri_amd.extract_tri_batch_dev(D.ptr, D.stride, D.bs, A.ptr, A.stride, 0, 65, 65, 3, False, 1)
    torch.cuda.synchronize()
    D.check(exp)


# ---- the permutations -------------------------------------------------------------------------------------------------------------

def _perm_calls(nrows, ncols, want_path, seed):
    """Both sides and both trans at every length, per-member P (the six members of assemble_cases.perm_members, two of them with an
    entry out of range) and one shared P (p_bs = 0)."""
    for right in (0, 1):
        n = ncols if right else nrows
        assert want_path is None or m4ri_amd.plan_perm_batch(nrows, ncols, right) == want_path
        members = ac.perm_members(n, seed + right)
        p_bs = n + 5
        hP = np.concatenate([p for _, p in members]).astype(np.int32)
        dP = _i32(hP)
        fn = m4ri_amd.apply_p_right_batch_dev if right else m4ri_amd.apply_p_left_batch_dev
        for trans in (0, 1):
            for length in ac.perm_lengths(n):
                for shared in (False, True):
                    batch = 3 if shared else len(members)
                    A = Batch(nrows, ncols, batch, seed + 13 * length + trans).upload()
                    status = _i32(np.full(batch + 2, 77))
                    exp, est = A.bits.copy(), np.full(batch + 2, 77, dtype=np.int32)
                    for b in range(batch):
                        want = ac.apply_p(A.valid(b), members[2 if shared else b][1], length, right, trans)
                        est[b] = -1 if want is None else 0
                        if want is not None:
                            A.member(exp, b)[:, :ncols] = want
                    fn(A.ptr, A.stride, A.bs, nrows, ncols, batch, dP.data_ptr() + (4 * 2 * p_bs if shared else 0), 0 if shared else p_bs, length,
                       bool(trans), status.data_ptr())
                    torch.cuda.synchronize()
                    what = (("right" if right else "left"), trans, length, "shared" if shared else "per member")
                    A.check(exp, what)
                    assert np.array_equal(status.cpu().numpy(), est), what
                    if not shared and length >= 1:
                        assert est[4] == -1 and est[5] == -1 and est[0] == 0
        assert np.array_equal(dP.cpu().numpy(), hP)


@pytest.mark.parametrize("nrows,ncols", ac.PERM_SHAPES)
def test_permutations(nrows, ncols):
    _perm_calls(nrows, ncols, 0 if max(nrows, ncols) <= 64 else 1, 4000 + nrows + 2 * ncols)


@pytest.mark.parametrize("nrows,ncols", [(64, 64), (37, 5), (1, 1)])
def test_small_members_on_the_workgroup_path(monkeypatch, nrows, ncols):
    monkeypatch.setenv(PATH0, "0")
    _perm_calls(nrows, ncols, None, 4500 + nrows)


@pytest.mark.parametrize("nrows,ncols", [(70, 70), (33, 130)])
def test_one_by_one_path_on_a_small_member(monkeypatch, nrows, ncols):
    """Path 2 (blocking), reached with the path-1 bound lowered to just under what the member needs."""
    need = nrows * ac.words(ncols) * 8 + 8 * min(nrows, ncols) + 8
    monkeypatch.setenv(PATH1, str(need - 1))
    _perm_calls(nrows, ncols, None, 4600 + nrows)


def test_status_may_be_null():
    A = Batch(65, 65, 2, 4700).upload()
    P = _i32(np.concatenate([np.arange(65)[::-1], np.full(65, 65)]))
    exp = A.bits.copy()
    A.member(exp, 0)[:, :65] = ac.apply_p(A.valid(0), np.arange(65)[::-1], 65, 1, 0)
    m4ri_amd.apply_p_right_batch_dev(A.ptr, A.stride, A.bs, 65, 65, 2, P.data_ptr(), 65, 65)
    torch.cuda.synchronize()
    A.check(exp)


# ---- chains on the device ---------------------------------------------------------------------------------------------------------

class Chain:
    """factor -> L, U -> L * U -> the original under P and Q^T -> compare, for three members of ranks 0, partial and full of one
    shape; only first_row is ever downloaded."""

    def __init__(self, nrows, ncols, seed):
        self.m, self.n, self.k, self.batch = nrows, ncols, min(nrows, ncols), 3
        self.ranks = (0, self.k // 3 + 1, self.k)
        self.orig = Batch(nrows, ncols, 3, seed)
        self.fill(seed)
        self.orig.upload()
        m, n, k = self.m, self.n, self.k
        self.F, self.W, self.C = Batch(m, n, 3, seed + 1).upload(), Batch(m, n, 3, seed + 2).upload(), Batch(m, n, 3, seed + 3).upload()
        self.L, self.U = Batch(m, k, 3, seed + 4).upload(), Batch(k, n, 3, seed + 5).upload()
        self.P, self.Q, self.rank = _i32(np.full(3 * m, -7)), _i32(np.full(3 * n, -7)), _i32(np.full(3, -7))
        self.first = _i32(np.full(3, 55))
        self.st = _i32(np.full(6, 55))

    def fill(self, seed):
        for b, r in enumerate(self.ranks):
            self.orig.set_valid(b, ac.with_rank(self.m, self.n, r, seed + b))

    def refill(self, seed):
        """Fresh members in the same device buffer."""
        t, self.orig.t = self.orig.t, None
        self.fill(seed)
        t.copy_(torch.from_numpy(self.orig.h.view(np.int64).copy()))
        self.orig.t = t

    def queue(self, s):
        m, n, k, o, F, W, C, L, U = self.m, self.n, self.k, self.orig, self.F, self.W, self.C, self.L, self.U
        for X in (F, W):
            m4ri_amd.copy_block_batch_dev(X.ptr, X.stride, X.bs, 0, 0, o.ptr, o.stride, o.bs, 0, 0, m, n, 3, stream=s)
        m4ri_amd.ple_batch_dev(F.ptr, F.stride, F.bs, m, n, 3, 1, self.P.data_ptr(), self.Q.data_ptr(), self.rank.data_ptr(), stream=s)
        m4ri_amd.extract_tri_batch_dev(L.ptr, L.stride, L.bs, F.ptr, F.stride, F.bs, m, n, 3, False, 1, self.rank.data_ptr(), stream=s)
        m4ri_amd.extract_tri_batch_dev(U.ptr, U.stride, U.bs, F.ptr, F.stride, F.bs, m, n, 3, True, 2, self.rank.data_ptr(), stream=s)
        m4ri_amd.mul_small_batch_dev(C.ptr, C.stride, C.bs, L.ptr, L.stride, L.bs, U.ptr, U.stride, U.bs, m, k, n, 3, stream=s)
        m4ri_amd.apply_p_left_batch_dev(W.ptr, W.stride, W.bs, m, n, 3, self.P.data_ptr(), m, m, False, self.st.data_ptr(), stream=s)
        m4ri_amd.apply_p_right_batch_dev(W.ptr, W.stride, W.bs, m, n, 3, self.Q.data_ptr(), n, n, True, self.st.data_ptr() + 12, stream=s)
        m4ri_amd.mismatch_batch_dev(C.ptr, C.stride, C.bs, W.ptr, W.stride, W.bs, m, n, 3, self.first.data_ptr(), stream=s)

    def verify(self):
        assert self.first.cpu().numpy().tolist() == [-1, -1, -1]


def _chain(nrows, ncols, seed):
    assert m4ri_amd.plan_ple_batch(nrows, ncols) <= 2 and m4ri_amd.plan_mul_small_batch(nrows, min(nrows, ncols), ncols) <= 1
    assert m4ri_amd.plan_perm_batch(nrows, ncols, 0) <= 1 and m4ri_amd.plan_perm_batch(nrows, ncols, 1) <= 1
    return Chain(nrows, ncols, seed)


@pytest.mark.parametrize("nrows,ncols", ac.CHAIN_SHAPES)
def test_factorisations_verified_on_a_side_stream(nrows, ncols):
    c = _chain(nrows, ncols, 5000 + nrows)
    s = torch.cuda.Stream()
    c.queue(s.cuda_stream)
    s.synchronize()
    c.verify()
    assert c.rank.cpu().numpy().tolist() == list(c.ranks) and c.st.cpu().numpy().tolist() == [0] * 6
    c.orig.check_unchanged()


@pytest.mark.parametrize("nrows,ncols", ac.CHAIN_SHAPES)
def test_factorisations_verified_from_a_captured_graph(nrows, ncols):
    """The same chain captured once (after one plain run, which also settles the kernels' attributes) and replayed on fresh members."""
    c = _chain(nrows, ncols, 5100 + nrows)
    c.queue(0)
    torch.cuda.synchronize()
    c.verify()
    c.first.fill_(55)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        c.queue(torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert c.first.cpu().numpy().tolist() == [55] * 3, "capturing ran nothing"
    for round_ in (1, 2):
        c.refill(5200 + 10 * round_ + nrows)
        c.first.fill_(55)
        g.replay()
        torch.cuda.synchronize()
        c.verify()
        assert c.rank.cpu().numpy().tolist() == list(c.ranks)


def test_inverse_from_the_echelon_form_of_a_with_the_identity():
    """[A_b | I] by two block copies (the identity shared, a_bs = 0), echelonize_batch_dev(full), the right half by an unaligned
    submatrix_batch_dev (from column 65), compared with inv_batch_dev on invertible members through mismatch_batch_dev."""
    n, batch = 65, 3
    A = Batch(n, n, batch, 6000)
    for b in range(batch):  # invertible: unit lower times unit upper
        rng = np.random.default_rng(6001 + b)
        Lm = np.tril(rng.integers(0, 2, size=(n, n)), -1) + np.eye(n, dtype=np.int64)
        Um = np.triu(rng.integers(0, 2, size=(n, n)), 1) + np.eye(n, dtype=np.int64)
        A.set_valid(b, ac.matmul(Lm, Um))
    Id = Batch(n, n, 1, 6010, shared=True)
    Id.set_valid(0, np.eye(n, dtype=np.uint8))
    A.upload(), Id.upload()
    AI, R, V = Batch(n, 2 * n, batch, 6011).upload(), Batch(n, n, batch, 6012).upload(), Batch(n, n, batch, 6013).upload()
    rank, rank2, first = _i32(np.zeros(batch)), _i32(np.zeros(batch)), _i32(np.full(batch, 55))
    exp = AI.bits.copy()
    for b in range(batch):
        AI.member(exp, b)[:, :2 * n] = np.hstack([A.valid(b), np.eye(n, dtype=np.uint8)])
    m4ri_amd.copy_block_batch_dev(AI.ptr, AI.stride, AI.bs, 0, 0, A.ptr, A.stride, A.bs, 0, 0, n, n, batch)
    m4ri_amd.copy_block_batch_dev(AI.ptr, AI.stride, AI.bs, 0, n, Id.ptr, Id.stride, 0, 0, 0, n, n, batch)
    torch.cuda.synchronize()
    AI.check(exp, "[A | I]")
    m4ri_amd.echelonize_batch_dev(AI.ptr, AI.stride, AI.bs, n, 2 * n, batch, 1, rank.data_ptr())
    m4ri_amd.submatrix_batch_dev(R.ptr, R.stride, R.bs, AI.ptr, AI.stride, AI.bs, 0, n, n, 2 * n, batch)
    m4ri_amd.inv_batch_dev(V.ptr, V.stride, V.bs, A.ptr, A.stride, A.bs, n, batch, rank2.data_ptr())
    m4ri_amd.mismatch_batch_dev(R.ptr, R.stride, R.bs, V.ptr, V.stride, V.bs, n, n, batch, first.data_ptr())
    torch.cuda.synchronize()
    assert first.cpu().numpy().tolist() == [-1] * batch and rank2.cpu().numpy().tolist() == [n] * batch
    for b in range(batch):  # and the inverse it is
        got = R.valid(b, ac.to_bits(R.download()))
        assert np.array_equal(ac.matmul(A.valid(b), got), np.eye(n, dtype=np.uint8)), b
