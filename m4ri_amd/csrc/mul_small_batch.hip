// mul_small_batch.hip -- products of many independent tiny matrices, C_b (+)= A_b * B_b, one launch for the batch.
//
// The M4RM leaves (m4rm_small.hip, m4rm8q_leaf.hip) build lookup tables in LDS for tiles of hundreds of rows; a 64 x 64 x 64 member
// fills a thirty-second of one such tile.  Here a member never leaves the registers.  The paths (m4ri_amd_plan_mul_small_batch):
//   0  m, l, n <= 64: a wave per member.  Lane r holds row r of A and of C, lane j holds row j of B, one word each.  For every inner
//      bit j < l the wave takes B's row j with v_readlane (two halves into SGPRs), turns bit j of its own row of A into an all-ones /
//      all-zeros mask (a one-bit signed field extract) and folds c ^= mask & b with one v_bitop3_b32 per half.  No LDS, no barrier.
//   1  max(m, l, n) <= the path-1 bound: the same loop, a wave per 64 x 64 block of C (row block i, word column w of a member),
//      over the words(l) steps of the inner dimension: lane r loads A[64 i + r][q], lane j loads B[64 q + j][w].
//   2  everything else: forwarded to m4ri_amd_m4rm_batch_dev, with its locking and its contract.
// Lanes at rows >= m touch neither A nor C; lanes at inner rows >= l hold a zero row of B, so the bits of A beyond its last column
// meet zeros.  The last word of a row of C is written under the column mask (the old word is read only for that, or to accumulate),
// so paths 0 and 1 never change a bit at a column >= n, a word from the width to c_stride of a row, or anything between members.
// Paths 0 and 1 are plain launches on the caller's stream: no allocation, no copy, no engine workspace, hence no engine lock.
#include <hip/hip_runtime.h>
#include <stdlib.h>
#include "batch_common.h"
#include "../../include/m4ri_amd.h"

namespace {

// (a workgroup is BATCH_WAVE_THREADS threads: four waves = four members (path 0) or four blocks of C (path 1))
// Path 1 up to this max(m, l, n); a multiple of 64 in [64, 256], 64 = path 1 empty.  Measured (tools/bench_mul_small_batch.py,
// profiles/mul_small_batch_bench.txt): on operands of 256 MB path 1 beats m4ri_amd_m4rm_batch_dev 10.7x / 6.6x / 3.8x
// on the cubes of 128 / 192 / 256 with spreads under 1 %, so the bound is the largest candidate.  (At a thousand members the old
// path is m4rm_small_kernel and wins at 192 and 256, 0.68x / 0.44x: DESIGN.md.)  M4RI_AMD_MUL_SMALL_BATCH_PATH1_MAX overrides the
// bound for the routing of a call.
constexpr int64_t MSB_D1    = 256;

// c ^ (mask & b): bitop3's table is the function evaluated on a = 0xF0, b = 0xCC, c = 0xAA
__device__ __forceinline__ uint32_t xor_and(uint32_t mask, uint32_t b, uint32_t c) { return __builtin_amdgcn_bitop3_b32(mask, b, c, 0x6A); }

// acc ^= sum over the inner bits j < count (wave-uniform, <= 64) of a's bit j times lane j's b.  Unrolled in groups of eight under a
// wave-uniform guard; lanes >= count hold b = 0, so the bits a group runs past `count` add nothing.  HI: the upper 32 columns are live.
template <bool HI>
__device__ __forceinline__ void fold64(uint32_t &clo, uint32_t &chi, word a, word b, int count) {
  const uint32_t alo = (uint32_t)a, ahi = (uint32_t)(a >> 32), blo = (uint32_t)b, bhi = (uint32_t)(b >> 32);
#pragma unroll
  for (int g = 0; g < 8; ++g) {
    if (8 * g < count) {
      // the group's eight rows of B first, then the folds: a v_readlane's SGPR is not readable by the next two VALU slots, and
      // back to back with its v_bitop3 every broadcast would wait them out
      uint32_t slo[8], shi[8];
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        slo[k] = (uint32_t)__builtin_amdgcn_readlane((int)blo, 8 * g + k);
        if (HI) shi[k] = (uint32_t)__builtin_amdgcn_readlane((int)bhi, 8 * g + k);
      }
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        const int j         = 8 * g + k;
        const uint32_t mask = (uint32_t)__builtin_amdgcn_sbfe((int)(j < 32 ? alo : ahi), (unsigned)(j & 31), 1u);
        clo = xor_and(mask, slo[k], clo);
        if (HI) chi = xor_and(mask, shi[k], chi);
      }
      __builtin_amdgcn_sched_barrier(0);
    }
  }
}

// path 0: a wave per member.  Members b0 + 4 * blockIdx.x + wave.
template <bool HI>
__global__ __launch_bounds__(BATCH_WAVE_THREADS) void msb_wave_kernel(word *__restrict__ C, int64_t c_stride, int64_t c_bs, const word *A, int64_t a_stride,
                                                                      int64_t a_bs, const word *B, int64_t b_stride, int64_t b_bs, int m, int l, int n,
                                                                      int64_t b0, int64_t batch, int add) {
  const int lane  = threadIdx.x & 63;
  const int64_t b = b0 + (int64_t)blockIdx.x * (BATCH_WAVE_THREADS / 64) + (threadIdx.x >> 6);
  if (b >= batch) return;  // wave-uniform, no barrier in this kernel
  const word mask = tail_mask(n);
  const bool old  = add || (n & 63);  // the old word of C: to accumulate into, or for the bits beyond the last column
  word *c         = C + b * c_bs + (int64_t)lane * c_stride;
  word a = 0, bw = 0, prev = 0;
  if (lane < m && l > 0) a = A[b * a_bs + (int64_t)lane * a_stride];
  if (lane < l) bw = B[b * b_bs + (int64_t)lane * b_stride];
  if (lane < m && old) prev = *c;
  uint32_t clo = add ? (uint32_t)prev : 0u, chi = add ? (uint32_t)(prev >> 32) : 0u;
  fold64<HI>(clo, chi, a, bw, l);
  const word r = ((word)chi << 32) | clo;
  if (lane < m) *c = (r & mask) | (prev & ~mask);
}

// path 1: a wave per 64 x 64 block of C.  Block t = 4 * blockIdx.x + wave of the launch is member b0 + t / (mb * wn), row block
// (t / wn) % mb, word column t % wn; the four blocks of a workgroup may belong to different members.
__global__ __launch_bounds__(BATCH_WAVE_THREADS) void msb_block_kernel(word *__restrict__ C, int64_t c_stride, int64_t c_bs, const word *A, int64_t a_stride,
                                                                       int64_t a_bs, const word *B, int64_t b_stride, int64_t b_bs, int m, int l, int n,
                                                                       int mb, int wn, int64_t b0, int64_t batch, int add) {
  const int lane    = threadIdx.x & 63;
  const uint32_t t  = blockIdx.x * (uint32_t)(BATCH_WAVE_THREADS / 64) + (threadIdx.x >> 6);
  const uint32_t per = (uint32_t)(mb * wn);
  const int64_t b   = b0 + (int64_t)(t / per);
  if (b >= batch) return;  // wave-uniform, no barrier in this kernel
  const uint32_t rem = t % per;
  const int i = (int)(rem / (uint32_t)wn), w = (int)(rem % (uint32_t)wn);
  const int row   = 64 * i + lane;
  const bool last = w == wn - 1;
  const word mask = last ? tail_mask(n) : ~(word)0;
  const bool old  = add || (last && (n & 63));
  const int wl    = (l + 63) >> 6;
  const word *ap  = A + b * a_bs + (int64_t)row * a_stride;                  // lane's row of A
  const word *bp  = B + b * b_bs + (int64_t)lane * b_stride + w;             // lane's row of B in step 0
  word *c         = C + b * c_bs + (int64_t)row * c_stride + w;
  word a = 0, bw = 0, prev = 0;
  if (row < m && wl > 0) a = ap[0];
  if (lane < l) bw = bp[0];
  if (row < m && old) prev = *c;
  uint32_t clo = add ? (uint32_t)prev : 0u, chi = add ? (uint32_t)(prev >> 32) : 0u;
  for (int q = 0; q < wl; ++q) {
    word an = 0, bn = 0;  // the next step's words, in flight under this step's fold
    if (q + 1 < wl) {
      if (row < m) an = ap[q + 1];
      if (64 * (q + 1) + lane < l) bn = bp[(int64_t)64 * (q + 1) * b_stride];
    }
    const int count = l - 64 * q;
    fold64<true>(clo, chi, a, bw, count < 64 ? count : 64);
    a  = an;
    bw = bn;
  }
  const word r = ((word)chi << 32) | clo;
  if (row < m) *c = (r & mask) | (prev & ~mask);
}

// the path-1 bound of this call: MSB_D1 unless the environment overrides it (read per call; [64, 256] in multiples of 64)
int64_t path1_max() {
  const char *s = getenv("M4RI_AMD_MUL_SMALL_BATCH_PATH1_MAX");
  if (!s || !*s) return MSB_D1;
  int64_t v = atoll(s) / 64 * 64;
  if (v < 64) v = 64;
  if (v > 256) v = 256;
  return v;
}

int plan(int64_t m, int64_t l, int64_t n, int64_t d1) {
  if (m < 0 || l < 0 || n < 0) return -1;
  const int64_t mx = m > l ? (m > n ? m : n) : (l > n ? l : n);
  return mx <= 64 ? 0 : mx <= d1 ? 1 : 2;
}

}  // namespace

extern "C" {

int m4ri_amd_plan_mul_small_batch(int64_t m, int64_t l, int64_t n) { return plan(m, l, n, MSB_D1); }

int m4ri_amd_mul_small_batch_dev(word *C, int64_t c_stride, int64_t c_bs, const word *A, int64_t a_stride, int64_t a_bs, const word *B,
                                 int64_t b_stride, int64_t b_bs, int64_t m, int64_t l, int64_t n, int64_t batch, int add, void *stream) {
  if (m < 0 || l < 0 || n < 0 || batch < 0 || c_stride < 0 || c_bs < 0 || a_stride < 0 || a_bs < 0 || b_stride < 0 || b_bs < 0)
    return (int)hipErrorInvalidValue;
  const int64_t wl = words_of(l), wn = words_of(n);
  if (a_stride < wl || b_stride < wn || c_stride < wn) return (int)hipErrorInvalidValue;
  if (batch > 1 && m > 0 && c_bs < (m - 1) * c_stride + wn) return (int)hipErrorInvalidValue;
  const bool c_data = m > 0 && n > 0, a_data = m > 0 && l > 0, b_data = l > 0 && n > 0;
  if (batch > 0 && ((c_data && !C) || (a_data && !A) || (b_data && !B))) return (int)hipErrorInvalidValue;
  if (batch > 0 && c_data) {  // C's span (first member's start to last member's end) must not meet A's or B's
    const uintptr_t cn = member_span_bytes(batch, c_bs, m, c_stride, wn);
    if (a_data && spans_meet(C, cn, A, member_span_bytes(batch, a_bs, m, a_stride, wl))) return (int)hipErrorInvalidValue;
    if (b_data && spans_meet(C, cn, B, member_span_bytes(batch, b_bs, l, b_stride, wn))) return (int)hipErrorInvalidValue;
  }
  if (batch == 0 || m == 0 || n == 0) return 0;
  const int path = plan(m, l, n, path1_max());
  if (path == 2) return m4ri_amd_m4rm_batch_dev(C, c_stride, c_bs, A, a_stride, a_bs, B, b_stride, b_bs, m, l, n, batch, add, stream);
  hipStream_t st    = (hipStream_t)stream;
  const int64_t per = BATCH_WAVE_THREADS / 64;
  if (path == 0) {
    return launch_chunked(batch, BATCH_CHUNK * per, [&](int64_t b0, int64_t nb) {
      const dim3 grid((unsigned)((nb + per - 1) / per));
      if (n > 32)
        hipLaunchKernelGGL(msb_wave_kernel<true>, grid, dim3(BATCH_WAVE_THREADS), 0, st, C, c_stride, c_bs, A, a_stride, a_bs, B, b_stride, b_bs, (int)m, (int)l,
                           (int)n, b0, batch, add != 0);
      else
        hipLaunchKernelGGL(msb_wave_kernel<false>, grid, dim3(BATCH_WAVE_THREADS), 0, st, C, c_stride, c_bs, A, a_stride, a_bs, B, b_stride, b_bs, (int)m, (int)l,
                           (int)n, b0, batch, add != 0);
    });
  }
  const int64_t mb = (m + 63) / 64, blocks = mb * wn;       // waves per member: at most 16
  const int64_t members = BATCH_CHUNK * per / blocks;         // members per launch
  return launch_chunked(batch, members, [&](int64_t b0, int64_t nb) {
    hipLaunchKernelGGL(msb_block_kernel, dim3((unsigned)((nb * blocks + per - 1) / per)), dim3(BATCH_WAVE_THREADS), 0, st, C, c_stride, c_bs, A, a_stride, a_bs,
                       B, b_stride, b_bs, (int)m, (int)l, (int)n, (int)mb, (int)wn, b0, batch, add != 0);
  });
}

}  // extern "C"
