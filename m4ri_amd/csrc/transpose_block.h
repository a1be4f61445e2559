// transpose_block.h -- the 64 x 64 bit block transpose in registers that transpose.hip (a tile of 1024 x 1024 bits per workgroup) and
// transpose_batch.hip (a wave per small member or per block of one) share.  Internal to the file that includes it (an unnamed
// namespace, as in batch_common.h).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace {

// lane i holds row i of a 64 x 64 bit block in (lo, hi); on return lane j holds column j.  Six exchange stages (lane
// distance = bit distance = 32, 16, ..., 1), none of them through LDS -- with ds_bpermute the six dependent LDS round
// trips per block were what the kernel waited for:
//   32: lanes >= 32 of lo <-> lanes < 32 of hi: one v_permlane32_swap;
//   16: the low halves of both dwords in one register, the high halves in another (v_perm), v_permlane16_swap;
//   8: the same with bytes, two v_perm from the previous form, the exchange a DPP row_ror:8 and three selects, two v_perm back;
//   4, 2, 1: a lane keeps the bits K of its dwords (M for the lower lane of a pair, ~M for the upper one) and hands
//       the others to its partner, both dwords' worth packed into one dword that moves by DPP (row_half_mirror
//       + quad_perm[3,2,1,0] = xor 4; quad_perm for 2 and 1); branch-free, the two roles differ in K and two shift counts.
__device__ __forceinline__ uint32_t dpp_xor8(uint32_t v) { return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x128, 0xf, 0xf, true); }
__device__ __forceinline__ uint32_t dpp_xor4(uint32_t v) {
  const int t = __builtin_amdgcn_update_dpp(0, (int)v, 0x141, 0xf, 0xf, true);  // row_half_mirror: i -> i ^ 7
  return (uint32_t)__builtin_amdgcn_update_dpp(0, t, 0x1B, 0xf, 0xf, true);     // quad_perm [3,2,1,0]: i -> i ^ 3
}
__device__ __forceinline__ uint32_t dpp_xor2(uint32_t v) { return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x4E, 0xf, 0xf, true); }
__device__ __forceinline__ uint32_t dpp_xor1(uint32_t v) { return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0xB1, 0xf, 0xf, true); }

__device__ __forceinline__ void transpose_block(uint32_t &lo, uint32_t &hi, int lane) {
  {
    const auto r = __builtin_amdgcn_permlane32_swap(lo, hi, false, false);
    lo = r[0]; hi = r[1];
  }
  {
    // distance 16: y = the low halves of (lo, hi), x = the high halves; the lower lane of a pair keeps y and gets its
    // partner's y as its new x, the upper lane keeps x and gets its partner's x as its new y
    uint32_t y = __builtin_amdgcn_perm(hi, lo, 0x05040100u);
    uint32_t x = __builtin_amdgcn_perm(hi, lo, 0x07060302u);
    const auto r = __builtin_amdgcn_permlane16_swap(y, x, false, false);  // odd rows of y <-> even rows of x
    y = r[0]; x = r[1];
    // distance 8, straight from that form: y8 = the even bytes of the (lo, hi) that (y, x) stand for, x8 = the odd ones
    const uint32_t y8 = __builtin_amdgcn_perm(x, y, 0x06020400u), x8 = __builtin_amdgcn_perm(x, y, 0x07030501u);
    const bool up = (lane & 8) != 0;
    const uint32_t got = dpp_xor8(up ? y8 : x8);
    const uint32_t ny = up ? got : y8, nx = up ? x8 : got;
    lo = __builtin_amdgcn_perm(nx, ny, 0x05010400u);
    hi = __builtin_amdgcn_perm(nx, ny, 0x07030602u);
  }
#define TR_STAGE(D, M, XCHG)                                                           \
  {                                                                                    \
    const uint32_t up = (uint32_t)lane & (D), K = up ? ~(M) : (M);                     \
    const uint32_t shr = (D) - up, shl = up; /* (D, 0) for the lower lane, (0, D) for the upper */ \
    const uint32_t s  = ((lo & ~K) >> shr) | ((hi & ~K) << shl);                       \
    const uint32_t r  = XCHG(s);                                                       \
    lo = (lo & K) | ((r & (M)) << shr);                                                \
    hi = (hi & K) | ((r & ~(M)) >> shl);                                               \
  }
  TR_STAGE(4, 0x0f0f0f0fu, dpp_xor4)
  TR_STAGE(2, 0x33333333u, dpp_xor2)
  TR_STAGE(1, 0x55555555u, dpp_xor1)
#undef TR_STAGE
}

}  // namespace
