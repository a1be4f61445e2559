"""ctypes binding of m4ri_amd/libm4ri_amd_leaves.so, the test-only library m4ri_amd/build.py links from the objects of m4rm_leaf.hip,
a4_pack.hip, m4rm8q_leaf.hip, m4rm_small.hip and aux_kernels.hip (+ scheme_passes.hip, which aux_kernels.hip calls): the internal
launchers of the M4RM leaves and of the helpers of a split launch (m4ri_amd/csrc/gf2_internal.h), which the product library deliberately
keeps local.  Not API: it lives under tests/ and only tests/test_gpu_leaves.py uses it.

Pointers are plain integers (device addresses, e.g. torch's data_ptr() plus a byte offset); every launch goes to the null stream, which
torch's default stream is, so a torch.cuda.synchronize() after a call waits for it.  The launchers return their hipError_t as an int:
0 success, 1 hipErrorInvalidValue (the launch is refused on the host, nothing was started).
"""
from __future__ import annotations

import ctypes
import os

from pass_lib import HIP_INVALID_VALUE, HIP_SUCCESS, LeafArgs   # one definition of struct LeafArgs (its sizeof == 168 is asserted there)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PATH = os.path.join(ROOT, "m4ri_amd", "libm4ri_amd_leaves.so")

_P, _L, _I = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int

assert ctypes.sizeof(LeafArgs) == 168

_SIGNATURES = {
    "gf2_launch_m4rm_leaf": (_I, [_P, LeafArgs, _I]),
    "gf2_launch_m4rm_leaf_variant": (_I, [_P, LeafArgs, _I, _I, _I]),
    "gf2_launch_m4rm_small": (_I, [_P, LeafArgs]),
    "gf2_m4rm_small_ksplit": (_I, [_L, _L, _I, _L]),
    "gf2_m4rm8_a4_words": (_L, [_L, _L, _L]),
    "gf2_launch_a4_pack_rot": (_I, [_P, LeafArgs, _P, _I]),
    "gf2_m4rm8q_effective_ksplit": (_I, [_L, _I]),
    "gf2_launch_m4rm8q": (_I, [_P, LeafArgs, _P]),
    "gf2_launch_reduce_partials": (_I, [_P, _I, _P, _L, _L, _L, _L, _L, _L, _L, _L, _L, _L, _I, _P]),
    "gf2_launch_zero_tiles": (_I, [_P, _P, _L, _L, _L, _L, _L, _L, _L, _L, _L, _L]),
}
_lib = None


def lib() -> ctypes.CDLL:
    global _lib
    if _lib is None:
        if not os.path.exists(PATH):
            raise RuntimeError(f"{PATH} is missing: build it with `python -m m4ri_amd.build`")
        L = ctypes.CDLL(PATH, mode=ctypes.RTLD_LOCAL)
        for name, (res, args) in _SIGNATURES.items():
            fn = getattr(L, name)
            fn.restype, fn.argtypes = res, args
        _lib = L
    return _lib


def leaf_args(A, a_stride, a_bs, B, b_stride, b_bs, C, c_stride, c_bs, m, l, n, batch, ksplit=1, mode=0, tile_base=0, tile_count=0,
              Cpart=None) -> LeafArgs:
    """What a caller fills in (engine.hip: launch_leaf_one); the launchers derive wn, the tile grid and the split geometry themselves."""
    a = LeafArgs()
    a.A, a.B, a.C = A, B, C
    a.a_stride, a.b_stride, a.c_stride = a_stride, b_stride, c_stride
    a.a_bs, a.b_bs, a.c_bs = a_bs, b_bs, c_bs
    a.m, a.l, a.n, a.batch, a.ksplit, a.mode = m, l, n, batch, ksplit, mode
    a.tile_base, a.tile_count, a.Cpart = tile_base, tile_count, Cpart
    return a


def m4rm_leaf(a: LeafArgs, rg: int) -> int:
    """Generation 1 (m4rm_leaf.hip), tiles of 32 rg rows x 2048 columns."""
    return lib().gf2_launch_m4rm_leaf(None, a, rg)


def m4rm_leaf_variant(a: LeafArgs, rg: int, ug: int, pipe: int) -> int:
    return lib().gf2_launch_m4rm_leaf_variant(None, a, rg, ug, pipe)


def m4rm_small(a: LeafArgs) -> int:
    """Generation 5 (m4rm_small.hip), tiles of 256 rows x 512 columns."""
    return lib().gf2_launch_m4rm_small(None, a)


def m4rm_small_ksplit(tiles: int, wl: int, cus: int, c_words: int) -> int:
    return lib().gf2_m4rm_small_ksplit(tiles, wl, cus, c_words)


def a4_words(m: int, l: int, batch: int) -> int:
    return lib().gf2_m4rm8_a4_words(m, l, batch)


def a4_pack_rot(a: LeafArgs, a4: int, rot: int) -> int:
    return lib().gf2_launch_a4_pack_rot(None, a, a4, rot)


def m4rm8q_effective_ksplit(l: int, ksplit: int) -> int:
    return lib().gf2_m4rm8q_effective_ksplit(l, ksplit)


def m4rm8q(a: LeafArgs, a4: int) -> int:
    """Generation 4 (m4rm8q_leaf.hip), tiles of 4096 rows x 512 columns, on the packed A at a4."""
    return lib().gf2_launch_m4rm8q(None, a, a4)


def reduce_partials(acc, C, cs, cbs, m, wn, tile_rows, tw, tiles_m, tiles_n, tile_base, ntiles, ks, Cpart) -> int:
    return lib().gf2_launch_reduce_partials(None, int(acc), C, cs, cbs, m, wn, tile_rows, tw, tiles_m, tiles_n, tile_base, ntiles, ks, Cpart)


def zero_tiles(C, cs, cbs, m, wn, tile_rows, tw, tiles_m, tiles_n, tile_base, ntiles) -> int:
    return lib().gf2_launch_zero_tiles(None, C, cs, cbs, m, wn, tile_rows, tw, tiles_m, tiles_n, tile_base, ntiles)
