"""Every fused Strassen pass kernel, called directly and compared word for word with the NumPy reference (tests/pass_reference.py, proven
on the CPU by tests/test_pass_reference.py).  Run this module first when you touch a pass: it takes seconds per case, works on megabytes,
and a mismatch names the pass, the form, the ancestor, the descendant, the row and the word.

The launchers of m4ri_amd/csrc/gf2_internal.h -- gf2_launch_pass_down (both sides), _down_pack, _up, for the Winograd passes of 1 ... 4
levels (aux_kernels.hip) and the rank-R scheme passes of 2 ... 4 levels (scheme_passes.hip), and the pack pass of a4_pack.hip -- are
reached through the test-only library tests/pass_lib.py binds.  Every case checks

  * the result, equal to the reference in every word;
  * the frame: the source is unchanged, and every destination word outside the written region still holds its poison (all ones) -- the
    padding of each ancestor row of an up pass, the gap between parents, a guard block before and after the array;
  * acc = 0 on a poisoned ancestor (no dependence on what was there: this includes the forms that zero first and meet by atomic XOR),
    acc = 1 onto random content;
  * the launcher's answer: success, or hipErrorInvalidValue for a shape it documents as not taken -- and then nothing written.

ROWS below is the parameter table as data: per row the kernel instantiation it is meant to reach (`reach`) and the launcher's condition
that routes there (`why`).  The shape and the flags alone select the form, so one process reaches every instantiation.
`python tools/pass_coverage.py` prints the table and compares it with the kernel names of a rocprofv3 trace of this module
(profiles/passes_kernel_coverage.txt).

Not in scope:
  * the nparents > 65535 loop of the scheme launchers and the matching refusal of the four-level Winograd launchers: the smallest legal
    case writes tens of GiB, and what that costs on a shared machine has not been measured.  Its argument arithmetic (p0 * p_bs,
    p0 * leaves * c_bs) is checked by reading only;
  * more than one trip of the grid-stride loops (more than 2^20 lanes) beyond one level: grid_for() is one function shared by all of
    them, and the one-level rows "trips" run it with two trips; three levels would need 3 GiB of descendants;
  * the launchers' refusals of grids beyond 2^31 - 1 workgroups and, in the four-level atomic up form, of a quadrant row range of 2 GiB
    or more: no array that large is allocated here;
  * nparents = 50 at four levels is run on the small leaf shapes only (the packed forms take up to 7 parents there: 50 would be 0.5 GiB).
"""
import os
import subprocess
from collections import namedtuple

import numpy as np
import pytest
import torch

import pass_lib
import pass_reference as ref

GUARD = 32            # words of poison before and after every destination (a multiple of 2: the base stays 16-byte aligned)
POISON = np.uint64(0xFFFFFFFFFFFFFFFF)

# op: "down" (flag = bside), "pack" (flag = rot), "up" (flag = acc).  soff / doff: word offset of the source / destination base pointer
# (1: only 8-byte aligned).  spad: words of row padding of the ancestor (stride = 2^L cw + spad).  gap: words between parents beyond
# rows * stride; None: bs = 0 (one parent, what multi.hip and engine.hip pass for a single product).  rc: the launcher's answer.
Row = namedtuple("Row", "kind L op flag crows cw np soff doff spad gap rc reach why")


def _b(x):
    return "true" if x else "false"


def _row(kind, L, op, flag, crows, cw, np_, soff=0, doff=0, spad=0, gap=0, rc=0, reach="", why=""):
    return Row(kind, L, op, flag, crows, cw, np_, soff, doff, spad, gap, rc, reach, why)


# ---- one and two Winograd levels: word2 where vec_ok() holds on both sides, the scalar instantiation otherwise --------------------------
# (crows, cw, np, soff, doff, spad, gap, vector?, the reason)
_VEC_CASES = [
    (1, 1, 1, 0, 0, 0, None, False, "cw odd (smallest shape; bs = 0)"),
    (7, 3, 2, 0, 0, 1, 1, False, "cw odd > 1, odd stride, odd bs"),
    (7, 6, 7, 0, 0, 0, 0, True, "vec_ok: 16-byte bases, even stride, bs, cw"),
    (7, 6, 2, 1, 0, 0, 0, False, "source base only 8-byte aligned, np > 1"),
    (7, 6, 2, 0, 1, 0, 0, False, "destination base only 8-byte aligned, np > 1"),
    (7, 6, 2, 0, 0, 1, 0, False, "odd stride (bs even), np > 1"),
    (7, 6, 2, 0, 0, 0, 1, False, "odd bs (stride even), np > 1: the scalar fallback with an odd batch stride"),
    (96, 20, 1, 0, 0, 0, None, True, "vec_ok with bs = 0"),
    (3, 10, 50, 0, 0, 2, 2, True, "vec_ok, 50 parents, crows cw = 30: the tail of the grid-stride loop"),
    (32, 16, 2, 0, 0, 0, 4, True, "vec_ok, cw = 16"),
    (64, 32, 2, 0, 0, 0, 0, True, "vec_ok, cw = 32, crows = 64"),
    (288, 48, 1, 0, 0, 2, 0, True, "vec_ok, cw = 48, crows = 288"),
    (5, 64, 2, 1, 1, 0, 0, False, "both bases only 8-byte aligned, cw = 64"),
    (3, 128, 7, 0, 0, 0, 0, True, "vec_ok, cw = 128"),
]


def _winograd12_rows():
    rows = []
    for L, dn, upn in ((1, "winograd_down_kernel", "winograd_up_kernel"), (2, "winograd_down2_kernel", "winograd_up2_kernel")):
        for flag in (0, 1):
            for (crows, cw, np_, soff, doff, spad, gap, vec, why) in _VEC_CASES:
                v = "word2" if vec else "word"
                rows.append(_row("w", L, "down", flag, crows, cw, np_, soff, doff, spad, gap, 0, f"{dn}<{v},{_b(flag)}>", why))
                rows.append(_row("w", L, "up", flag, crows, cw, np_, soff, doff, spad, gap, 0, f"{upn}<{v},{_b(flag)}>", why))
    # two trips of the grid-stride loop (grid_for: more than 256 * 16 workgroups' worth of lanes): 32 x 288 x 128 = 1 179 648 scalar lanes
    rows.append(_row("w", 1, "down", 0, 288, 128, 32, spad=1, reach="winograd_down_kernel<word,false>", why="odd stride; trips = 2 in grid_for"))
    rows.append(_row("w", 1, "up", 1, 288, 128, 32, spad=1, reach="winograd_up_kernel<word,true>", why="odd stride; trips = 2 in grid_for"))
    return rows


# ---- the packed A side of the Winograd passes --------------------------------------------------------------------------------------------
def _winograd_pack_rows():
    rows = []
    for rot in (0, 1):
        # two levels: vec_ok(source) && crows % 32 == 0 && cw % 16 == 0 && a4 16-byte aligned
        k = f"winograd_down2_pack_kernel<{rot}>"
        ok = "down2_pack_ok: vec_ok source, crows % DP_ROWS == 0, cw % (2 DP_V) == 0, a4 16-byte aligned"
        for (crows, cw, np_, gap) in ((32, 16, 1, None), (64, 32, 2, 2), (96, 16, 7, 0), (288, 16, 1, 0), (32, 48, 50, 0)):
            rows.append(_row("w", 2, "pack", rot, crows, cw, np_, gap=gap, reach=k, why=ok))
        # three levels: crows % 32 == 0 && cw % 16 == 0 (any source alignment)
        for (crows, cw, np_, soff, doff, spad, gap) in ((32, 16, 1, 0, 0, 0, None), (64, 32, 2, 1, 0, 1, 1), (96, 16, 7, 0, 0, 0, 0), (288, 16, 1, 0, 0, 0, 0),
                                                        (32, 48, 2, 0, 0, 2, 0), (32, 16, 50, 0, 0, 0, 0)):
            rows.append(_row("w", 3, "pack", rot, crows, cw, np_, soff, doff, spad, gap, 0, f"winograd_down3_pack_kernel<{rot}>",
                             "down3_pack_ok: crows % DP3_ROWS == 0, cw % DP3_W == 0" + ("; 8-byte source, odd stride and bs" if soff else "")))
        # four levels: the same rule (the form without the transpose is the only one)
        for (crows, cw, np_, soff, doff, spad, gap) in ((32, 16, 1, 0, 0, 0, None), (64, 32, 2, 1, 0, 1, 1), (96, 16, 1, 0, 0, 0, 0), (32, 48, 2, 0, 0, 2, 0),
                                                        (32, 16, 7, 0, 0, 0, 0)) + (((288, 16, 1, 0, 0, 0, 0),) if rot == 1 else ()):
            rows.append(_row("w", 4, "pack", rot, crows, cw, np_, soff, doff, spad, gap, 0, f"winograd_down4_pack_lds_kernel<{rot}>",
                             "down3_pack_ok" + ("; nine row blocks: the second group of eight is partly filled" if crows == 288 else "")))
    # refusals: hipErrorInvalidValue and nothing written
    for (L, crows, cw, soff, doff, spad, gap, why) in (
            (2, 7, 16, 0, 0, 0, 0, "crows % 32 != 0"), (2, 32, 20, 0, 0, 0, 0, "cw % 16 != 0"), (2, 32, 8, 0, 0, 0, 0, "cw % 16 != 0"),
            (2, 1, 1, 0, 0, 0, 0, "smallest shape"), (2, 32, 16, 1, 0, 0, 0, "source only 8-byte aligned"), (2, 32, 16, 0, 0, 1, 0, "odd stride"),
            (2, 32, 16, 0, 0, 0, 1, "odd bs"), (2, 32, 16, 0, 1, 0, 0, "a4 only 8-byte aligned"),
            (3, 7, 16, 0, 0, 0, 0, "crows % 32 != 0"), (3, 32, 8, 0, 0, 0, 0, "cw % 16 != 0"), (3, 32, 20, 0, 0, 0, 0, "cw % 16 != 0"), (3, 1, 1, 0, 0, 0, 0, "smallest shape"),
            (4, 7, 16, 0, 0, 0, 0, "crows % 32 != 0"), (4, 32, 8, 0, 0, 0, 0, "cw % 16 != 0"), (4, 32, 20, 0, 0, 0, 0, "cw % 16 != 0"),
            (1, 32, 16, 0, 0, 0, 0, "no one-level pack pass")):
        rows.append(_row("w", L, "pack", 1, crows, cw, 2, soff, doff, spad, gap, 1, "(refused)", why))
    for L in (2, 3, 4):   # a shape every depth takes with rot 0 or 1
        rows.append(_row("w", L, "pack", 2, 32, 16, 2, rc=1, reach="(refused)", why="rot outside {0, 1}"))
    return rows


# ---- three and four Winograd levels, row-major --------------------------------------------------------------------------------------------
def _winograd34_rows():
    rows = []
    small = [(1, 1, 1, 0, 0, 0, None, "smallest shape; bs = 0"), (7, 3, 2, 1, 1, 1, 1, "8-byte bases, odd stride and bs, np > 1"),
             (7, 5, 50, 0, 0, 0, 0, "50 parents, crows cw = 35"), (32, 16, 2, 0, 0, 0, 2, "cw = 16"), (96, 20, 1, 0, 0, 4, 0, "cw = 20"),
             (64, 48, 1, 0, 0, 0, 0, "cw = 48, crows = 64"), (288, 2, 1, 0, 0, 0, 0, "crows = 288")]
    for flag in (0, 1):
        for (crows, cw, np_, soff, doff, spad, gap, why) in small + [(64, 64, 1, 0, 0, 0, 0, "cw = 64"), (3, 128, 7, 0, 0, 0, 0, "cw = 128"), (5, 32, 2, 0, 0, 0, 0, "cw = 32")]:
            rows.append(_row("w", 3, "down", flag, crows, cw, np_, soff, doff, spad, gap, 0, f"winograd_down3_kernel<{_b(flag)}>", why))
            rows.append(_row("w", 3, "up", flag, crows, cw, np_, soff, doff, spad, gap, 0, f"winograd_up3_kernel<{_b(flag)}>", why))
        # four levels: cw % 32 != 0 -> the direct / atomic forms
        for (crows, cw, np_, soff, doff, spad, gap, why) in small + [(3, 100, 1, 0, 0, 0, 0, "crows cw = 300: a partly filled position block")]:
            rows.append(_row("w", 4, "down", flag, crows, cw, np_, soff, doff, spad, gap, 0, f"winograd_down4_kernel<{_b(flag)}>", "cw % 32 != 0; " + why))
            rows.append(_row("w", 4, "up", flag, crows, cw, np_, soff, doff, spad, gap, 0, "winograd_up4_kernel" + ("" if flag else " + rowwise_kernel (zero first)"),
                             "cw % U4_POS != 0; " + why))
        # cw % 32 == 0 -> the forms through LDS
        for (crows, cw, np_, soff, doff, spad, gap, why) in ((1, 32, 1, 0, 0, 0, None, "smallest; bs = 0"), (7, 32, 2, 1, 1, 1, 1, "8-byte bases, odd stride and bs"),
                                                             (1, 64, 7, 0, 0, 0, 0, "cw = 64"), (2, 128, 1, 0, 0, 2, 0, "cw = 128"), (32, 64, 1, 0, 0, 0, 0, "32 x 64"),
                                                             (1, 32, 50, 0, 0, 0, 6, "50 parents on gridDim.y")):
            rows.append(_row("w", 4, "down", flag, crows, cw, np_, soff, doff, spad, gap, 0, f"winograd_down4_lds_kernel<{_b(flag)}>", "cw % 32 == 0; " + why))
            rows.append(_row("w", 4, "up", flag, crows, cw, np_, soff, doff, spad, gap, 0, f"winograd_up4_lds_kernel<{_b(flag)}>", "cw % U4_POS == 0; " + why))
    return rows


# ---- the scheme passes ----------------------------------------------------------------------------------------------------------------------
def _scheme_rows():
    rows = []
    tmpl = {2: "1,64,1", 3: "2,64,7", 4: "4,64,8"}       # scheme_down_kernel<G, POS, UNITS, BSIDE>
    tmpl_up = {2: "1,64,1", 3: "2,32,8", 4: "4,32,8"}    # scheme_up_kernel<G, POS, UNITS, ACC>, scheme_down_pack_kernel<G, POS, UNITS>
    for L in (2, 3, 4):
        shapes = [(1, 64, 1, 0, 0, 0, None, "smallest legal cw; bs = 0"), (7, 64, 2, 1, 1, 1, 1, "8-byte bases, odd stride and bs, np > 1"),
                  (3, 128, 7, 0, 0, 0, 0, "cw = 128"), (32, 64, 1, 0, 0, 2, 0, "32 x 64" + (": the largest case, 36 MiB of descendants" if L == 4 else "")),
                  (1, 64, 50, 0, 0, 0, 2, "50 parents on gridDim.y"), (2, 192, 2, 0, 0, 0, 0, "cw = 192"), (64, 64, 1, 0, 0, 0, 0, "crows = 64")]
        shapes += {2: [(288, 64, 1, 0, 0, 0, 0, "crows = 288")], 3: [(96, 64, 2, 0, 0, 0, 0, "crows = 96")], 4: []}[L]
        for flag in (0, 1):
            for (crows, cw, np_, soff, doff, spad, gap, why) in shapes:
                rows.append(_row("s", L, "down", flag, crows, cw, np_, soff, doff, spad, gap, 0, f"scheme_down_kernel<{tmpl[L]},{_b(flag)}>", "cw % 64 == 0; " + why))
                rows.append(_row("s", L, "up", flag, crows, cw, np_, soff, doff, spad, gap, 0, f"scheme_up_kernel<{tmpl_up[L]},{_b(flag)}>", "cw % 64 == 0; " + why))
        pos = 64 if L == 2 else 32
        packs = [(pos, 16, 1, 0, 0, 0, None, "smallest legal shape; bs = 0"), (2 * pos, 32, 2, 1, 1, 1, 1, "8-byte bases, odd stride and bs, np > 1"),
                 (9 * pos, 16, 1, 0, 0, 0, 0, "nine row blocks: the second group of eight is partly filled"), (pos, 48, 2, 0, 0, 2, 0, "cw = 48"),
                 (pos, 64, 1, 0, 0, 0, 0, "cw = 64"), (pos, 128, 1, 0, 0, 0, 0, "cw = 128"), (pos, 16, 50 if L == 2 else 7, 0, 0, 0, 0, "many parents on gridDim.y")]
        for (crows, cw, np_, soff, doff, spad, gap, why) in packs:
            rows.append(_row("s", L, "pack", 1, crows, cw, np_, soff, doff, spad, gap, 0, f"scheme_down_pack_kernel<{tmpl_up[L]}>", f"crows % {pos} == 0, cw % 16 == 0; " + why))
        for (op, flag, crows, cw, why) in (("down", 0, 7, 32, "cw % 64 != 0"), ("down", 1, 1, 1, "cw % 64 != 0"), ("down", 1, 7, 96, "cw % 64 != 0"),
                                           ("up", 0, 7, 32, "cw % 64 != 0"), ("up", 1, 1, 1, "cw % 64 != 0"), ("up", 0, 7, 96, "cw % 64 != 0"),
                                           ("pack", 1, 7, 16, f"crows % {pos} != 0"), ("pack", 1, pos // 2, 16, f"crows % {pos} != 0"),
                                           ("pack", 1, pos, 8, "cw % 16 != 0"), ("pack", 1, pos, 20, "cw % 16 != 0"), ("pack", 1, 1, 1, "smallest shape")):
            rows.append(_row("s", L, op, flag, crows, cw, 2, rc=1, reach="(refused)", why=why))
    for op in ("down", "up", "pack"):
        rows.append(_row("s", 1, op, 1, 64, 64, 1, rc=1, reach="(refused)", why="no one-level scheme pass"))
        rows.append(_row("s", 5, op, 1, 64, 64, 1, rc=1, reach="(refused)", why="levels > 4"))
        rows.append(_row("w", 5, op, 1, 64, 64, 1, rc=1, reach="(refused)", why="levels > 4"))
        rows.append(_row("w", 0, op, 1, 64, 64, 1, rc=1, reach="(refused)", why="levels < 1"))
    return rows


# ---- sizes of 0: success, nothing launched, nothing written ---------------------------------------------------------------------------------
def _zero_rows():
    rows = []
    for kind, levels in (("w", (1, 2, 3, 4)), ("s", (2, 3, 4))):
        for L in levels:
            for op in ("down", "up") + (("pack",) if L >= 2 else ()):
                for (crows, cw, np_) in ((32, 64, 0), (0, 64, 2), (32, 0, 2)):
                    rows.append(_row(kind, L, op, 1, crows, cw, np_, reach="(nothing)", why="nparents * crows * cw == 0"))
    return rows


ROWS = _winograd12_rows() + _winograd_pack_rows() + _winograd34_rows() + _scheme_rows() + _zero_rows()


def _id_tail(r: Row) -> str:
    """The ids of the three- and four-level Winograd rows end in the tags they carried while developer switches could re-route them to a
    second form.  The switches and those forms are gone; the ids stay as they were, so that a row's results remain comparable with the
    suite's earlier runs."""
    if r.kind != "w" or r.L < 3 or r.reach.startswith("("):
        return ""
    lds = "_lds_" in r.reach
    return {"down": "-swnt7" + ("-swdown4" if lds else ""), "up": "-swnt0" + ("-swup4" if lds else ""), "pack": "-swnt7" + ("-swpack4" if r.L == 4 else "")}[r.op]


def row_id(r: Row) -> str:
    gap = "bs0" if r.gap is None else f"gap{r.gap}"
    return f"{r.kind}{r.L}-{r.op}{r.flag}-r{r.crows}-c{r.cw}-p{r.np}-o{r.soff}{r.doff}-pad{r.spad}-{gap}" + _id_tail(r)


# every instantiation of a pass kernel the launchers can start (rot is 0 or 1): the table must name each of them
def expected_kernels():
    tf = ("true", "false")
    out = set()
    for k in ("winograd_down_kernel", "winograd_up_kernel", "winograd_down2_kernel", "winograd_up2_kernel"):
        out |= {f"{k}<{v},{b}>" for v in ("word", "word2") for b in tf}
    out |= {f"winograd_down2_pack_kernel<{r}>" for r in (0, 1)}
    for k in ("winograd_down3_kernel", "winograd_up3_kernel", "winograd_down4_kernel", "winograd_down4_lds_kernel", "winograd_up4_lds_kernel"):
        out |= {f"{k}<{b}>" for b in tf}
    out.add("winograd_up4_kernel")
    for k in ("winograd_down3_pack_kernel", "winograd_down4_pack_lds_kernel"):
        out |= {f"{k}<{r}>" for r in (0, 1)}
    for g, gu in (("1,64,1", "1,64,1"), ("2,64,7", "2,32,8"), ("4,64,8", "4,32,8")):
        out |= {f"scheme_down_kernel<{g},{b}>" for b in tf} | {f"scheme_up_kernel<{gu},{b}>" for b in tf} | {f"scheme_down_pack_kernel<{gu}>"}
    out.add("a4_pack_kernel")
    return out


def kernels_named():
    """The instantiations the table means to reach."""
    names = {r.reach.split(" + ")[0] for r in ROWS if not r.reach.startswith("(")}
    names.add("a4_pack_kernel")   # the second opinion of every pack row, and test_a4_pack_kernel_alone
    return names


def test_the_table_names_every_instantiation():
    """No GPU needed: the table names every instantiation of a pass kernel that the launchers can start (expected_kernels: written out
    from the launchers, rot 0 and 1) and nothing else."""
    named = kernels_named()
    assert named == expected_kernels(), sorted(named ^ expected_kernels())
    ids = [row_id(r) for r in ROWS]
    assert len(ids) == len(set(ids)), [i for i in ids if ids.count(i) > 1]
    for r in ROWS:
        assert r.why and r.rc in (0, 1), row_id(r)
        assert (r.rc == 1) == (r.reach == "(refused)"), row_id(r)


def test_the_pass_library_exports_what_the_binding_binds():
    """No GPU needed: m4ri_amd/build.py links the test-only library with exactly the names tests/pass_lib.py binds (the product
    library's own export list is pinned by test_cabi.py and does not hold them)."""
    from m4ri_amd import build
    build.build(verbose=False)
    out = subprocess.run(["nm", "-D", "--defined-only", pass_lib.PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert exported == set(pass_lib._SIGNATURES) == set(build.PASS_EXPORTS), sorted(exported ^ set(pass_lib._SIGNATURES))
    assert pass_lib.PATH == build.PASS_LIB
    assert pass_lib.scheme444_rank() == ref.scheme_tables()[0] and [pass_lib.scheme444_leaves(L) for L in (2, 3, 4)] == [ref.leaves(L, True) for L in (2, 3, 4)]


# ---- running a row ----------------------------------------------------------------------------------------------------------------------------
def _dev(buf: np.ndarray) -> torch.Tensor:
    return torch.from_numpy(buf.view(np.int64)).cuda()


def _host(t: torch.Tensor) -> np.ndarray:
    return t.cpu().numpy().view(np.uint64)


def _digits(r: Row, d: int) -> str:
    parts = []
    for s in reversed(ref.pass_steps(r.L, r.kind == "s")):
        k = 7 if s == "w" else ref.scheme_tables()[0]
        parts.append(str(d % k))
        d //= k
    return "(" + ", ".join(reversed(parts)) + ")"


def _what(r: Row) -> str:
    side = {"down": f"{'B' if r.flag else 'A'} side", "pack": f"packed A, rot {r.flag}", "up": f"acc {r.flag}"}[r.op]
    return f"pass_{'down_pack' if r.op == 'pack' else r.op}, {'scheme' if r.kind == 's' else 'Winograd'}, {r.L} levels, {side}; form {r.reach}; row {row_id(r)}"


def _mismatch_descendants(r: Row, got: np.ndarray, want: np.ndarray, unit: str) -> str:
    """got / want: (np, leaves, a, b).  The exact report of the first difference and how far it spreads."""
    bad = np.argwhere(got != want)
    p, d, a, b = (int(x) for x in bad[0])
    descs = sorted({(int(x[0]), int(x[1])) for x in bad[:100000]})
    return (f"{_what(r)}: {len(bad)} of {got.size} {unit}s differ; first: ancestor {p}, descendant {d} = {_digits(r, d)}, "
            + (f"chunk {a}, row {b}" if unit == "dword" else f"row {a}, word {b}") + f": got {int(got[p, d, a, b]):#x}, want {int(want[p, d, a, b]):#x}; "
            f"(ancestor, descendant) pairs that differ: {descs[:8]}{' ...' if len(descs) > 8 else ''}")


def _check_frame(r: Row, got: np.ndarray, lo: int, hi: int):
    """Everything before word lo and from word hi on is poison."""
    for name, part, base in (("before", got[:lo], 0), ("after", got[hi:], hi)):
        bad = np.flatnonzero(part != POISON)
        assert bad.size == 0, f"{_what(r)}: {bad.size} guard words {name} the destination were written, first at word {base + int(bad[0]) - lo} relative to its base"


def _geometry(r: Row):
    """Shapes with the zero sizes replaced by 1 for the allocation (the launcher is still given the zeros)."""
    return max(r.np, 1), max(r.crows, 1), max(r.cw, 1)


def run_row(r: Row):
    """Launch the row's pass, return the launcher's answer, and check everything that answer promises."""
    scheme = r.kind == "s"
    steps_ok = (1 <= r.L <= 4 and not scheme) or (2 <= r.L <= 4 and scheme)
    np_, crows, cw = _geometry(r)
    nothing = r.np * r.crows * r.cw == 0
    f = 1 << (r.L if steps_ok else 1)
    nleaves = ref.leaves(r.L, scheme) if steps_ok else 7
    rng = np.random.default_rng(sum(map(ord, row_id(r))))
    dwords = np_ * nleaves * crows * cw
    if r.op in ("down", "pack"):
        anc = ref.make_operand(rng, np_, f * crows, f * cw, off=r.soff, stride_pad=r.spad, gap=r.gap or 0, zero_bs=r.gap is None, guard=GUARD)
        src = _dev(anc.buf)
        dst_host = np.full(GUARD + r.doff + dwords + GUARD, POISON, dtype=np.uint64)
        dst = _dev(dst_host)
        sp, dp = src.data_ptr() + 8 * anc.off, dst.data_ptr() + 8 * (GUARD + r.doff)
        if r.op == "down":
            rc = pass_lib.pass_down(r.L, scheme, r.flag, sp, anc.stride, anc.bs, dp, r.np, r.crows, r.cw)
        else:
            rc = pass_lib.pass_down_pack(r.L, scheme, sp, anc.stride, anc.bs, dp, r.np, r.crows, r.cw, r.flag)
        torch.cuda.synchronize()
        assert rc in (pass_lib.HIP_SUCCESS, pass_lib.HIP_INVALID_VALUE), f"{_what(r)}: the launcher returned HIP error {rc}"
        assert np.array_equal(_host(src), anc.buf), f"{_what(r)}: the source was written"
        got = _host(dst)
        lo, hi = GUARD + r.doff, GUARD + r.doff + dwords
        if rc != 0 or nothing:
            bad = np.flatnonzero(got != POISON)
            assert bad.size == 0, f"{_what(r)}: answer {rc}, yet {bad.size} destination words were written, first at word {int(bad[0]) - lo}"
            return rc
        _check_frame(r, got, lo, hi)
        plain = ref.down(anc.view(), r.L, scheme, bool(r.flag) if r.op == "down" else False)      # (np, leaves, crows, cw)
        if r.op == "down":
            g = got[lo:hi].reshape(plain.shape)
            assert np.array_equal(g, plain), _mismatch_descendants(r, g, plain, "word")
            return rc
        rot = 1 if scheme else r.flag
        want = ref.pack_a4(plain.reshape(-1, crows, cw), rot).reshape(np_, nleaves, 2 * cw, crows)
        g = got[lo:hi].view("<u4").reshape(want.shape)
        assert np.array_equal(g, want), _mismatch_descendants(r, g, want, "dword")
        # the second opinion: the pack pass of a4_pack.hip on the plain descendants of pass_down (the route the engine takes when a pack
        # pass is refused); where pass_down itself does not take the shape (the scheme's cw % 64), on the reference's plain descendants
        d2 = torch.full((dwords,), -1, dtype=torch.int64, device="cuda")
        rc2 = pass_lib.pass_down(r.L, scheme, 0, sp, anc.stride, anc.bs, d2.data_ptr(), r.np, r.crows, r.cw)
        torch.cuda.synchronize()
        if rc2 != 0:
            assert scheme and cw % 64 != 0, f"{_what(r)}: pass_down refused the shape (HIP error {rc2})"
            d2 = _dev(plain.reshape(-1))
        else:
            assert np.array_equal(_host(d2).reshape(plain.shape), plain), _mismatch_descendants(r, _host(d2).reshape(plain.shape), plain, "word")
        assert pass_lib.a4_words(crows, 64 * cw, np_ * nleaves) == dwords
        p2 = torch.full((GUARD + dwords + GUARD,), -1, dtype=torch.int64, device="cuda")
        rc3 = pass_lib.a4_pack_rot(d2.data_ptr(), cw, crows * cw, crows, 64 * cw, np_ * nleaves, p2.data_ptr() + 8 * GUARD, rot)
        torch.cuda.synchronize()
        assert rc3 == 0, f"{_what(r)}: gf2_launch_a4_pack_rot returned HIP error {rc3}"
        g2 = _host(p2)
        _check_frame(r, g2, GUARD, GUARD + dwords)
        g2 = g2[GUARD:GUARD + dwords].view("<u4").reshape(want.shape)
        assert np.array_equal(g2, want), "a4_pack_kernel on the plain descendants; " + _mismatch_descendants(r, g2, want, "dword")
        assert g2.tobytes() == g.tobytes() == want.tobytes()
        return rc
    # up
    prods = rng.integers(0, 1 << 64, size=(np_, nleaves, crows, cw), dtype=np.uint64)
    src_host = np.concatenate([rng.integers(0, 1 << 64, size=GUARD + r.soff, dtype=np.uint64), prods.reshape(-1)])
    src = _dev(src_host)
    anc = ref.make_operand(rng, np_, f * crows, f * cw, off=r.doff, stride_pad=r.spad, gap=r.gap or 0, zero_bs=r.gap is None,
                           fill="random" if r.flag else "poison", guard=GUARD)
    dst = _dev(anc.buf)
    rc = pass_lib.pass_up(r.L, scheme, r.flag, src.data_ptr() + 8 * (GUARD + r.soff), dst.data_ptr() + 8 * anc.off, anc.stride, anc.bs, r.np, r.crows, r.cw)
    torch.cuda.synchronize()
    assert rc in (pass_lib.HIP_SUCCESS, pass_lib.HIP_INVALID_VALUE), f"{_what(r)}: the launcher returned HIP error {rc}"
    assert np.array_equal(_host(src), src_host), f"{_what(r)}: the products were written"
    got = _host(dst)
    if rc != 0 or nothing:
        bad = np.flatnonzero(got != anc.buf)
        assert bad.size == 0, f"{_what(r)}: answer {rc}, yet {bad.size} words of the ancestor array changed, first at word {int(bad[0]) - anc.off}"
        return rc
    want = anc.buf.copy()
    inside = ref.up(prods, r.L, scheme)
    wv = ref.Operand(want, anc.off, anc.stride, anc.bs, np_, f * crows, f * cw).view()
    wv[...] = (wv ^ inside) if r.flag else inside
    if not np.array_equal(got, want):
        mask = anc.written_mask()
        out = np.flatnonzero((got != want) & ~mask)
        assert out.size == 0, (f"{_what(r)}: {out.size} words outside the ancestors (row padding, the gap between parents, the guards) were written, "
                               f"first at word {int(out[0]) - anc.off} relative to the base (stride {anc.stride}, bs {anc.bs})")
        gv = ref.Operand(got, anc.off, anc.stride, anc.bs, np_, f * crows, f * cw).view()
        bad = np.argwhere(gv != wv)
        p, row, w = (int(x) for x in bad[0])
        blocks = sorted({(int(x[0]), int(x[1]) // crows, int(x[2]) // cw) for x in bad[:100000]})
        raise AssertionError(f"{_what(r)}: {len(bad)} of {gv.size} words differ; first: ancestor {p}, row {row}, word {w} = block ({row // crows}, {w // cw}) "
                             f"row {row % crows} word {w % cw}: got {int(gv[p, row, w]):#x}, want {int(wv[p, row, w]):#x}; (ancestor, block row, block column) "
                             f"that differ: {blocks[:8]}{' ...' if len(blocks) > 8 else ''}")
    return rc


gpu = pytest.mark.gpu


@gpu
@pytest.mark.parametrize("r", ROWS, ids=row_id)
def test_pass_matches_reference(r):
    rc = run_row(r)
    assert rc == r.rc, f"{_what(r)}: the launcher answered {rc}, the table says {r.rc} ({r.why})"


# ---- the ok predicates ----------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("L", [2, 3, 4])
def test_down_pack_ok_agrees_with_the_launcher(L):
    """gf2_pass_down_pack_ok says yes exactly where the Winograd pack pass of that depth then succeeds (with the right bits: run_row)."""
    seen = set()
    for (crows, cw, soff, doff, spad, gap) in ((32, 16, 0, 0, 0, 0), (32, 16, 1, 0, 0, 0), (32, 16, 0, 1, 0, 0), (32, 16, 0, 0, 1, 0), (32, 16, 0, 0, 0, 1),
                                               (64, 32, 0, 0, 2, 2), (31, 16, 0, 0, 0, 0), (33, 16, 0, 0, 0, 0), (32, 15, 0, 0, 0, 0), (32, 17, 0, 0, 0, 0),
                                               (32, 8, 0, 0, 0, 0), (4, 2, 0, 0, 0, 0)):
        r = _row("w", L, "pack", 1, crows, cw, 2, soff, doff, spad, gap)
        rc = run_row(r)
        # the predicate looks at the alignment of the pointers it is given: hand it addresses with the row's alignment
        base = 1 << 20
        stride = (1 << L) * cw + spad
        ok = pass_lib.pass_down_pack_ok(L, base + 8 * soff, stride, (1 << L) * crows * stride + gap, base + 8 * doff, crows, cw)
        assert ok == (rc == 0), f"{_what(r)}: gf2_pass_down_pack_ok says {ok}, the launcher answered {rc}"
        seen.add(ok)
    assert seen == {True, False}


@gpu
@pytest.mark.parametrize("L", [2, 3, 4])
def test_scheme444_ok_agrees_with_the_launchers(L):
    """Where gf2_scheme444_ok says yes the three scheme launchers take the leaf shapes (and give the right bits: run_row); a launcher that
    succeeds where it says no still gives the right bits (run_row checks every success)."""
    if os.environ.get("M4RI_AMD_SCHEME") is not None:
        pytest.fail("run without M4RI_AMD_SCHEME: the predicate's shape rule is behind that switch")
    assert pass_lib.scheme444_rank() == ref.scheme_tables()[0] and pass_lib.scheme444_leaves(L) == ref.leaves(L, True)
    seen = set()
    for (a_rows, a_cw, b_cw) in ((64, 16, 64), (32, 16, 64), (64, 8, 64), (64, 16, 32), (64, 17, 64), (7, 16, 64)):
        ok = pass_lib.scheme444_ok(L, a_rows, a_cw, 64 * a_cw, b_cw)
        # (the B leaf has 64 a_cw rows; no launcher's rule looks at the rows of the B side, so its pass runs on 2 rows here)
        rcs = [run_row(_row("s", L, "pack", 1, a_rows, a_cw, 1)), run_row(_row("s", L, "down", 1, 2, b_cw, 1)), run_row(_row("s", L, "up", 0, a_rows, b_cw, 1))]
        if ok:
            assert rcs == [0, 0, 0], f"scheme, {L} levels, leaf A {a_rows} x {a_cw} words, B {64 * a_cw} x {b_cw}: ok, but the launchers answered {rcs}"
        seen.add(ok)
    assert seen == {True, False}


# ---- the pack pass of a4_pack.hip on its own: rows up to m_pad zero, the bits from column l on masked ------------------------------------------
@gpu
@pytest.mark.parametrize("rot", [0, 1])
@pytest.mark.parametrize("m,l,batch,spad,gap", [(1, 1, 1, 0, 0), (7, 100, 3, 1, 1), (64, 64, 2, 0, 0), (65, 2048, 1, 0, 0), (330, 2049, 2, 1, 3), (288, 4160, 1, 0, 0),
                                                  (0, 64, 1, 0, 0)])
def test_a4_pack_kernel_alone(rot, m, l, batch, spad, gap):
    rng = np.random.default_rng(m + l)
    wa = (l + 63) // 64
    A = ref.make_operand(rng, batch, max(m, 1), wa, stride_pad=spad, gap=gap, guard=GUARD)
    m_pad = (m + 3) & ~3
    words = pass_lib.a4_words(m, l, batch)
    assert words == (batch * m_pad * 2 * wa + 1) // 2
    src, dst = _dev(A.buf), torch.full((GUARD + words + GUARD,), -1, dtype=torch.int64, device="cuda")
    rc = pass_lib.a4_pack_rot(src.data_ptr() + 8 * A.off, A.stride, A.bs, m, l, batch, dst.data_ptr() + 8 * GUARD, rot)
    torch.cuda.synchronize()
    assert rc == 0
    assert np.array_equal(_host(src), A.buf), "a4_pack_kernel: the source was written"
    got = _host(dst)
    bad = np.flatnonzero(got[:GUARD] != POISON).size + np.flatnonzero(got[GUARD + words:] != POISON).size
    assert bad == 0, f"a4_pack_kernel: {bad} guard words written"
    if m == 0:
        assert (got == POISON).all(), "a4_pack_kernel: m = 0 writes nothing"
        return
    plain = A.view()[:, :m, :].copy()
    if l % 64:
        plain[:, :, -1] &= np.uint64((1 << (l % 64)) - 1)
    want = ref.pack_a4(plain, rot, m_pad)
    g = got[GUARD:GUARD + words].view("<u4")[:want.size].reshape(want.shape)
    bad = np.argwhere(g != want)
    assert bad.size == 0, (f"a4_pack_kernel, rot {rot}, {m} x {l} bits, batch {batch}: {len(bad)} dwords differ, first: matrix {bad[0][0]}, chunk {bad[0][1]}, "
                           f"row {bad[0][2]}: got {int(g[tuple(bad[0])]):#x}, want {int(want[tuple(bad[0])]):#x}")
