"""ctypes binding of m4ri_amd/libm4ri_amd_passes.so, the test-only library m4ri_amd/build.py links from the objects of aux_kernels.hip,
scheme_passes.hip and a4_pack.hip: the internal launchers of the fused Strassen passes (m4ri_amd/csrc/gf2_internal.h), which the product
library deliberately keeps local.  Not API: it lives under tests/ and only tests/test_gpu_passes.py uses it.

Pointers are plain integers (device addresses, e.g. torch's data_ptr() plus a byte offset); every launch goes to the null stream, which
torch's default stream is, so a torch.cuda.synchronize() after a call waits for it.  The functions return the launcher's hipError_t as
an int: 0 success, 1 hipErrorInvalidValue (the shape is not taken).
"""
from __future__ import annotations

import ctypes
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PATH = os.path.join(ROOT, "m4ri_amd", "libm4ri_amd_passes.so")
HIP_SUCCESS, HIP_INVALID_VALUE = 0, 1

_P, _L, _I = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int


class LeafArgs(ctypes.Structure):
    """gf2_common.h: struct LeafArgs (gf2_launch_a4_pack_rot takes it by value and reads A, a_stride, a_bs, m, l, n, batch)."""
    _fields_ = [("A", _P), ("B", _P), ("C", _P), ("Apk", _P), ("apk_stride", _L), ("apk_bs", _L),
                ("a_stride", _L), ("b_stride", _L), ("c_stride", _L), ("a_bs", _L), ("b_bs", _L), ("c_bs", _L),
                ("m", ctypes.c_int32), ("l", ctypes.c_int32), ("n", ctypes.c_int32), ("wn", ctypes.c_int32),
                ("tiles_m", ctypes.c_int32), ("tiles_n", ctypes.c_int32), ("ksplit", ctypes.c_int32), ("stages_per_split", ctypes.c_int32),
                ("chunks_per_split", ctypes.c_int32), ("batch", ctypes.c_int32), ("mode", ctypes.c_int32),
                ("tile_base", _L), ("tile_count", _L), ("Cpart", _P)]


assert ctypes.sizeof(LeafArgs) == 168

_SIGNATURES = {
    "gf2_launch_pass_down": (_I, [_P, _I, _I, _I, _P, _L, _L, _P, _L, _L, _L]),
    "gf2_launch_pass_down_pack": (_I, [_P, _I, _I, _P, _L, _L, _P, _L, _L, _L, _I]),
    "gf2_launch_pass_up": (_I, [_P, _I, _I, _I, _P, _P, _L, _L, _L, _L, _L]),
    "gf2_pass_down_pack_ok": (_I, [_I, _P, _L, _L, _P, _L, _L]),
    "gf2_scheme444_rank": (_I, []),
    "gf2_scheme444_leaves": (_L, [_I]),
    "gf2_scheme444_ok": (_I, [_I, _L, _L, _L, _L]),
    "gf2_launch_a4_pack_rot": (_I, [_P, LeafArgs, _P, _I]),
    "gf2_m4rm8_a4_words": (_L, [_L, _L, _L]),
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


def pass_down(levels, scheme, bside, src, stride, bs, dst, nparents, crows, cw) -> int:
    return lib().gf2_launch_pass_down(None, levels, int(scheme), int(bside), src, stride, bs, dst, nparents, crows, cw)


def pass_down_pack(levels, scheme, src, stride, bs, a4, nparents, crows, cw, rot) -> int:
    return lib().gf2_launch_pass_down_pack(None, levels, int(scheme), src, stride, bs, a4, nparents, crows, cw, rot)


def pass_up(levels, scheme, acc, prod, dst, stride, bs, nparents, crows, cw) -> int:
    return lib().gf2_launch_pass_up(None, levels, int(scheme), int(acc), prod, dst, stride, bs, nparents, crows, cw)


def pass_down_pack_ok(levels, src, stride, bs, a4, crows, cw) -> bool:
    return bool(lib().gf2_pass_down_pack_ok(levels, src, stride, bs, a4, crows, cw))


def scheme444_rank() -> int:
    return lib().gf2_scheme444_rank()


def scheme444_leaves(levels) -> int:
    return lib().gf2_scheme444_leaves(levels)


def scheme444_ok(levels, a_rows, a_cw, b_rows, b_cw) -> bool:
    return bool(lib().gf2_scheme444_ok(levels, a_rows, a_cw, b_rows, b_cw))


def a4_words(m, l, batch) -> int:
    return lib().gf2_m4rm8_a4_words(m, l, batch)


def a4_pack_rot(A, a_stride, a_bs, m, l, batch, a4, rot) -> int:
    """The pack pass of a4_pack.hip on `batch` matrices of m rows x l bits: a4 gets, per matrix, 2 ceil(l / 64) chunks of m_pad =
    (m + 3) & ~3 dwords."""
    a = LeafArgs()
    a.A, a.a_stride, a.a_bs, a.m, a.l, a.n, a.batch = A, a_stride, a_bs, m, l, 64, batch
    return lib().gf2_launch_a4_pack_rot(None, a, a4, rot)
