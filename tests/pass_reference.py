"""A plain NumPy statement of every fused Strassen pass (host only; the second opinion of tests/test_gpu_passes.py).

Written from the documented definitions -- the header comments of aux_kernels.hip (Winograd's operand sums and recombination),
scheme_passes.hip (leaf (r1, r2), the OUTER / inner applications), a4_pack.hip (the packed A) and scheme444.h (what the bits of U, V, W
mean) -- and not from the kernels' index arithmetic: a pass is a fixed GF(2)-linear map of blocks, so it is stated here on blocks.
tests/test_pass_reference.py proves the statement on the CPU (down, leaf products by the oracle, up == the oracle's whole product) before
it judges a kernel.

Layout.  An operand is a flat uint64 array with a word offset `off` of its base, a row stride `stride` and `bs` words between
consecutive parents (`Operand`), exactly what a launcher is given.  A parent of an L-level pass is 2^L crows rows x 2^L cw words; its
descendants are crows x cw words each, contiguous, descendant d of parent i at index leaves * i + d:

  * Winograd, one level: quadrants X11 X12 / X21 X22, children
        A side [A11, A12, S4, A22, S1, S2, S3],  S1 = A21+A22, S2 = S1+A11, S3 = A11+A21, S4 = A12+S2
        B side [B11, B21, B22, T4, T1, T2, T3],  T1 = B12+B11, T2 = B22+T1, T3 = B22+B12, T4 = T2+B21
    product j = A child j * B child j = P1 ... P7, and
        U2 = P1+P6, U3 = U2+P7, U4 = U2+P5, C11 = P1+P2, C12 = U4+P3, C21 = U3+P4, C22 = U3+P5.
    Levels 2, 3, 4 are this applied recursively: descendant 7 (7 (7 j0 + j1) + j2) + j3, the top level's child most significant.
  * The rank-R scheme of the 4 x 4 x 4 block product (scheme444.h): product r = (sum of the blocks A_ij with bit 4 i + j of U[r]) *
    (sum of the blocks B_jk with bit 4 j + k of V[r]), C_ik = sum of the products r with bit 4 i + k of W[r].  A scheme pass of 2 / 3 / 4
    levels is an OUTER application on the coarse 1 x 1 / 2 x 2 / 4 x 4 split (identity / one Winograd level as above / the scheme itself)
    followed by the scheme on each of its children: leaf (r1, r2) at index r1 * R + r2.
  * Packed A: descendant d as 32-bit dwords, chunk-major: dword q of row r at a4[d * (2 crows cw) + q * m_pad + r] (m_pad = crows in a
    pass), rows m .. m_pad - 1 zero; for rot = 1 every dword rotated right by 8 * ((r >> 6) & 3) bits, i.e. byte i of what is stored is
    byte (i + (r >> 6)) & 3 of the plain dword (v_alignbyte_b32 of the dword with itself).  The pass launchers take rot 0 or 1 and refuse every
    other value (engine.hip passes 0 or 1).
"""
from __future__ import annotations

import os
import re
from dataclasses import dataclass

import numpy as np

_CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "m4ri_amd", "csrc")


# ---- operands in memory -------------------------------------------------------------------------------------------------------------
@dataclass
class Operand:
    """nparents matrices of rows x words uint64 inside the flat array `buf`: word (p, r, w) at buf[off + p * bs + r * stride + w]."""
    buf: np.ndarray
    off: int
    stride: int
    bs: int
    nparents: int
    rows: int
    words: int

    def view(self) -> np.ndarray:
        """(nparents, rows, words) strided view onto buf (writable)."""
        assert self.nparents == 0 or self.off + (self.nparents - 1) * self.bs + (self.rows - 1) * self.stride + self.words <= self.buf.size
        return np.lib.stride_tricks.as_strided(self.buf[self.off:], shape=(self.nparents, self.rows, self.words),
                                               strides=(8 * self.bs, 8 * self.stride, 8), writeable=True)

    def written_mask(self) -> np.ndarray:
        """Boolean mask over buf of the words the operand's matrices occupy (everything else is frame)."""
        m = np.zeros(self.buf.size, dtype=bool)
        Operand(m, self.off, self.stride, self.bs, self.nparents, self.rows, self.words)._view_any()[...] = True
        return m

    def _view_any(self):
        return np.lib.stride_tricks.as_strided(self.buf[self.off:], shape=(self.nparents, self.rows, self.words),
                                               strides=(self.buf.itemsize * self.bs, self.buf.itemsize * self.stride, self.buf.itemsize), writeable=True)


def make_operand(rng, nparents, rows, words, off=0, stride_pad=0, gap=0, zero_bs=False, fill="random", guard=0) -> Operand:
    """A fresh operand: `guard` words before and after, rows `words + stride_pad` apart, parents `rows * stride + gap` apart (zero_bs: bs = 0,
    one parent).  fill: "random" everywhere, or "poison" (all ones) everywhere."""
    stride = words + stride_pad
    bs = 0 if zero_bs else rows * stride + gap
    assert not zero_bs or nparents <= 1
    n = guard + off + max(nparents, 1) * (rows * stride + gap) + guard
    if fill == "random":
        buf = rng.integers(0, 1 << 64, size=n, dtype=np.uint64)
    else:
        buf = np.full(n, ~np.uint64(0), dtype=np.uint64)
    return Operand(buf, guard + off, stride, bs, nparents, rows, words)


# ---- Winograd ---------------------------------------------------------------------------------------------------------------------------
def winograd_down1(X: np.ndarray, bside: bool) -> np.ndarray:
    """(..., 2 r, 2 w) -> (..., 7, r, w): the seven operand sums of one level."""
    r, w = X.shape[-2] // 2, X.shape[-1] // 2
    x11, x12, x21, x22 = X[..., :r, :w], X[..., :r, w:], X[..., r:, :w], X[..., r:, w:]
    if not bside:
        s1 = x21 ^ x22
        s2 = s1 ^ x11
        s3 = x11 ^ x21
        s4 = x12 ^ s2
        kids = [x11, x12, s4, x22, s1, s2, s3]
    else:
        t1 = x12 ^ x11
        t2 = x22 ^ t1
        t3 = x22 ^ x12
        t4 = t2 ^ x21
        kids = [x11, x21, x22, t4, t1, t2, t3]
    return np.stack(kids, axis=-3)


def winograd_up1(P: np.ndarray) -> np.ndarray:
    """(..., 7, r, w) -> (..., 2 r, 2 w): the recombination of one level."""
    p1, p2, p3, p4, p5, p6, p7 = (P[..., j, :, :] for j in range(7))
    u2 = p1 ^ p6
    u3 = u2 ^ p7
    u4 = u2 ^ p5
    c11, c12, c21, c22 = p1 ^ p2, u4 ^ p3, u3 ^ p4, u3 ^ p5
    return np.concatenate([np.concatenate([c11, c12], axis=-1), np.concatenate([c21, c22], axis=-1)], axis=-2)


# ---- the 4 x 4 x 4 scheme ------------------------------------------------------------------------------------------------------------------
def scheme_tables():
    """(R, U, V, W) parsed from scheme444.h."""
    text = open(os.path.join(_CSRC, "scheme444.h")).read()
    R = int(re.search(r"#define SCHEME444_R (\d+)", text).group(1))
    tabs = {name: [int(x, 16) for x in re.findall(r"0x([0-9a-f]{4})", re.search(rf"SCHEME444_{name}\[SCHEME444_R\] = \{{([^}}]*)\}}", text).group(1))]
            for name in "UVW"}
    assert all(len(t) == R for t in tabs.values())
    return R, tabs["U"], tabs["V"], tabs["W"]


def _blocks4(X):
    r, w = X.shape[-2] // 4, X.shape[-1] // 4
    return [[X[..., a * r:(a + 1) * r, b * w:(b + 1) * w] for b in range(4)] for a in range(4)]


def scheme_down1(X: np.ndarray, bside: bool) -> np.ndarray:
    """(..., 4 r, 4 w) -> (..., R, r, w): child r = the sum of the blocks (a, b) of the 4 x 4 split with bit 4 a + b of U[r] (A side) / V[r]."""
    R, U, V, _ = scheme_tables()
    blk = _blocks4(X)
    kids = []
    for m in (V if bside else U):
        acc = np.zeros_like(blk[0][0])
        for a in range(4):
            for b in range(4):
                if (m >> (4 * a + b)) & 1:
                    acc = acc ^ blk[a][b]
        kids.append(acc)
    return np.stack(kids, axis=-3)


def scheme_up1(P: np.ndarray) -> np.ndarray:
    """(..., R, r, w) -> (..., 4 r, 4 w): block (i, k) = the sum of the products r with bit 4 i + k of W[r]."""
    R, _, _, W = scheme_tables()
    assert P.shape[-3] == R
    rows = []
    for i in range(4):
        row = []
        for k in range(4):
            acc = np.zeros_like(P[..., 0, :, :])
            for r in range(R):
                if (W[r] >> (4 * i + k)) & 1:
                    acc = acc ^ P[..., r, :, :]
            row.append(acc)
        rows.append(np.concatenate(row, axis=-1))
    return np.concatenate(rows, axis=-2)


# ---- the passes: a list of one-level applications, top level first ----------------------------------------------------------------------------
def pass_steps(levels: int, scheme: bool):
    """The applications an L-level pass is made of, top level first: "w" one Winograd level (2 x 2), "s" the scheme (4 x 4, two levels)."""
    if not scheme:
        assert 1 <= levels <= 4
        return ["w"] * levels
    assert 2 <= levels <= 4
    return {2: ["s"], 3: ["w", "s"], 4: ["s", "s"]}[levels]


def leaves(levels: int, scheme: bool) -> int:
    R = scheme_tables()[0]
    n = 1
    for s in pass_steps(levels, scheme):
        n *= 7 if s == "w" else R
    return n


def down(X: np.ndarray, levels: int, scheme: bool, bside: bool) -> np.ndarray:
    """(N, 2^L r, 2^L w) parents -> (N, leaves, r, w) descendants, descendant index = ((j_top * n_next + j_next) ...)."""
    N = X.shape[0]
    cur = X
    for s in pass_steps(levels, scheme):
        kids = winograd_down1(cur, bside) if s == "w" else scheme_down1(cur, bside)      # (n, k, r', w')
        cur = kids.reshape((-1,) + kids.shape[-2:])                                      # child j of node n at n * k + j
    return np.ascontiguousarray(cur.reshape((N, -1) + cur.shape[-2:]))


def up(P: np.ndarray, levels: int, scheme: bool) -> np.ndarray:
    """(N, leaves, r, w) products -> (N, 2^L r, 2^L w): the recombination of every level, deepest first."""
    N = P.shape[0]
    cur = P.reshape((-1,) + P.shape[-2:])
    for s in reversed(pass_steps(levels, scheme)):
        k = 7 if s == "w" else scheme_tables()[0]
        grp = cur.reshape((-1, k) + cur.shape[-2:])
        cur = winograd_up1(grp) if s == "w" else scheme_up1(grp)
    assert cur.shape[0] == N
    return np.ascontiguousarray(cur)


# ---- the packed A ---------------------------------------------------------------------------------------------------------------------------
def _rotr_bytes(v: np.ndarray, s: np.ndarray) -> np.ndarray:
    """Every uint32 of v rotated right by 8 * s bits (s in 0 .. 3, broadcast)."""
    sh = (8 * s).astype(np.uint32)
    return np.where(sh == 0, v, (v >> sh) | (v << ((np.uint32(32) - sh) & np.uint32(31)))).astype(np.uint32)


def pack_a4(D: np.ndarray, rot: int, m_pad: int | None = None) -> np.ndarray:
    """(N, m, w) uint64 matrices -> (N, 2 w, m_pad) uint32: dword q of row r at [n, q, r], rows m .. m_pad - 1 zero; rot = 1: each dword
    rotated right by 8 * ((r >> 6) & 3) bits."""
    assert rot in (0, 1), "the pass launchers take rot 0 or 1 only"
    N, m, w = D.shape
    m_pad = m if m_pad is None else m_pad
    dw = np.ascontiguousarray(D).view("<u4").reshape(N, m, 2 * w)     # dword 2 k = low half of word k
    if rot == 1:
        dw = _rotr_bytes(dw, ((np.arange(m) >> 6) & 3)[None, :, None])
    out = np.zeros((N, 2 * w, m_pad), dtype=np.uint32)
    out[:, :, :m] = dw.transpose(0, 2, 1)
    return out


def unpack_a4(P: np.ndarray, rot: int, m: int | None = None) -> np.ndarray:
    """The inverse of pack_a4: (N, 2 w, m_pad) uint32 -> (N, m, w) uint64."""
    assert rot in (0, 1)
    N, q, m_pad = P.shape
    m = m_pad if m is None else m
    dw = np.ascontiguousarray(P[:, :, :m].transpose(0, 2, 1))
    if rot == 1:
        dw = _rotr_bytes(dw, ((4 - ((np.arange(m) >> 6) & 3)) & 3)[None, :, None])
    return np.ascontiguousarray(dw).view("<u8").reshape(N, m, q // 2)
