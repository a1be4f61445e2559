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
//
// Transposed operands (m4ri_amd_mul_small_batch_op_dev: C_b (+)= op(A_b) * op(B_b), A stored l x m and / or B stored n x l) are the same
// two kernels with a compile-time flag per operand.  The loop wants row r of op(A) in lane r and row j of op(B) in lane j, and a 64 x 64
// block of a stored operand held a row per lane becomes exactly that under transpose_block (transpose_block.h: six register exchange
// stages, no LDS).  So a lane loads its row of the STORED block -- path 0: lane < l of A, lane < n of B; path 1, step q of block
// (i, w): A[64 q + lane][i], B[64 w + lane][q] -- zero where the stored operand has no such row, and the wave transposes what it
// loaded before it folds.  What stored A holds beyond its column m lands in lanes >= m, which store nothing.  What stored B holds
// beyond its column l lands in the lanes at inner rows >= l, which the fold needs to be zero: they are cleared after the transpose.
// The untransposed instantiations are the kernels as they were.
#include <hip/hip_runtime.h>
#include <stdlib.h>
#include "batch_common.h"
#include "transpose_block.h"
#include "../../include/m4ri_amd.h"

namespace {

// (a workgroup is BATCH_WAVE_THREADS threads: four waves = four members (path 0) or four blocks of C (path 1))
// Path 1 up to this max(m, l, n); a multiple of 64 in [64, 256], 64 = path 1 empty.  Measured (tools/bench_mul_small_batch.py,
// profiles/mul_small_batch_bench.txt): on operands of 256 MB path 1 beats m4ri_amd_m4rm_batch_dev 10.7x / 6.6x / 3.8x
// on the cubes of 128 / 192 / 256 with spreads under 1 %, so the bound is the largest candidate.  (At a thousand members the old
// path is m4rm_small_kernel and wins at 192 and 256, 0.68x / 0.44x: DESIGN.md.)  M4RI_AMD_MUL_SMALL_BATCH_PATH1_MAX overrides the
// bound for the routing of a call.
constexpr int64_t MSB_D1    = 256;
// The same bound for a call with a transposed operand (tools/bench_mul_small_batch_op.py, profiles/mul_small_batch_op_bench.txt,
// DESIGN.md 3.4b): the largest candidate up to which the fused call is not slower, by more than the spread, than
// m4ri_amd_transpose_batch_dev into a scratch buffer followed by m4ri_amd_mul_small_batch_dev, for every op.  On operands of 256 MB
// the fused call is 1.06 ... 1.17x faster than that on the cubes of 128, 192 and 256 for NT, TN and TT, spreads under 0.5 %, so the
// bound is the largest candidate.  Beyond it such a call is refused (hipErrorNotSupported): the engine's workspace is not taken for it.
constexpr int64_t MSB_D1OP  = 256;

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

// lane i holds row i of a 64 x 64 bit block; the value of lane j is column j.  Every lane of the wave takes part.
__device__ __forceinline__ word transposed(word x, int lane) {
  uint32_t lo = (uint32_t)x, hi = (uint32_t)(x >> 32);
  transpose_block(lo, hi, lane);
  return ((word)hi << 32) | lo;
}

// path 0: a wave per member.  Members b0 + 4 * blockIdx.x + wave.  TA: A is stored l x m; TB: B is stored n x l.  A stored block is
// transposed whole whatever HI says: HI = false (n <= 32) drops the upper half of op(B)'s rows, not of stored B's.
template <bool HI, bool TA, bool TB>
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
  if (TA) {
    if (lane < l) a = A[b * a_bs + (int64_t)lane * a_stride];
  } else {
    if (lane < m && l > 0) a = A[b * a_bs + (int64_t)lane * a_stride];
  }
  if (TB) {
    if (lane < n && l > 0) bw = B[b * b_bs + (int64_t)lane * b_stride];
  } else {
    if (lane < l) bw = B[b * b_bs + (int64_t)lane * b_stride];
  }
  if (lane < m && old) prev = *c;
  if (TA) a = transposed(a, lane);
  if (TB) {
    bw = transposed(bw, lane);
    if (lane >= l) bw = 0;  // stored B's columns >= l
  }
  uint32_t clo = add ? (uint32_t)prev : 0u, chi = add ? (uint32_t)(prev >> 32) : 0u;
  fold64<HI>(clo, chi, a, bw, l);
  const word r = ((word)chi << 32) | clo;
  if (lane < m) *c = (r & mask) | (prev & ~mask);
}

// path 1: a wave per 64 x 64 block of C.  Block t = 4 * blockIdx.x + wave of the launch is member b0 + t / (mb * wn), row block
// (t / wn) % mb, word column t % wn; the four blocks of a workgroup may belong to different members.  TA: step q's block of op(A) is
// stored A[64 q + lane][i] transposed; TB: step q's block of op(B) is stored B[64 w + lane][q] transposed.  The words in flight are the
// stored ones; a step transposes its own before it folds.
template <bool TA, bool TB>
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
  // lane's row of A (TA: of stored A's word column i in step 0) and lane's row of B in step 0 (TB: of stored B's rows 64 w ...)
  const word *ap  = TA ? A + b * a_bs + (int64_t)lane * a_stride + i : A + b * a_bs + (int64_t)row * a_stride;
  const word *bp  = TB ? B + b * b_bs + (int64_t)(64 * w + lane) * b_stride : B + b * b_bs + (int64_t)lane * b_stride + w;
  const bool brow = 64 * w + lane < n;  // TB: stored B has this lane's row
  word *c         = C + b * c_bs + (int64_t)row * c_stride + w;
  word a = 0, bw = 0, prev = 0;
  if (TA) {
    if (lane < l) a = ap[0];
  } else {
    if (row < m && wl > 0) a = ap[0];
  }
  if (TB) {
    if (brow && wl > 0) bw = bp[0];
  } else {
    if (lane < l) bw = bp[0];
  }
  if (row < m && old) prev = *c;
  uint32_t clo = add ? (uint32_t)prev : 0u, chi = add ? (uint32_t)(prev >> 32) : 0u;
  for (int q = 0; q < wl; ++q) {
    word an = 0, bn = 0;  // the next step's words, in flight under this step's fold
    if (q + 1 < wl) {
      if (TA) {
        if (64 * (q + 1) + lane < l) an = ap[(int64_t)64 * (q + 1) * a_stride];
      } else {
        if (row < m) an = ap[q + 1];
      }
      if (TB) {
        if (brow) bn = bp[q + 1];
      } else {
        if (64 * (q + 1) + lane < l) bn = bp[(int64_t)64 * (q + 1) * b_stride];
      }
    }
    const int count = l - 64 * q < 64 ? l - 64 * q : 64;
    if (TA) a = transposed(a, lane);
    if (TB) {
      bw = transposed(bw, lane);
      if (lane >= count) bw = 0;  // stored B's columns >= l
    }
    fold64<true>(clo, chi, a, bw, count);
    a  = an;
    bw = bn;
  }
  const word r = ((word)chi << 32) | clo;
  if (row < m) *c = (r & mask) | (prev & ~mask);
}

int plan(int64_t m, int64_t l, int64_t n, int64_t d1) {
  if (m < 0 || l < 0 || n < 0) return -1;
  const int64_t mx = m > l ? (m > n ? m : n) : (l > n ? l : n);
  return mx <= 64 ? 0 : mx <= d1 ? 1 : 2;
}

// the instantiations by [HI][TA][TB] and [TA][TB]
using WaveKernel  = decltype(&msb_wave_kernel<true, false, false>);
using BlockKernel = decltype(&msb_block_kernel<false, false>);
constexpr WaveKernel WAVE_KERNELS[2][2][2] = {
    {{msb_wave_kernel<false, false, false>, msb_wave_kernel<false, false, true>}, {msb_wave_kernel<false, true, false>, msb_wave_kernel<false, true, true>}},
    {{msb_wave_kernel<true, false, false>, msb_wave_kernel<true, false, true>}, {msb_wave_kernel<true, true, false>, msb_wave_kernel<true, true, true>}}};
constexpr BlockKernel BLOCK_KERNELS[2][2] = {{msb_block_kernel<false, false>, msb_block_kernel<false, true>},
                                             {msb_block_kernel<true, false>, msb_block_kernel<true, true>}};

// both entries: C_b (+)= op(A_b) * op(B_b), A stored l x m under ta, B stored n x l under tb
int mul_small_batch(word *C, int64_t c_stride, int64_t c_bs, const word *A, int64_t a_stride, int64_t a_bs, const word *B, int64_t b_stride,
                    int64_t b_bs, int64_t m, int64_t l, int64_t n, int64_t batch, bool ta, bool tb, int add, void *stream) {
  if (m < 0 || l < 0 || n < 0 || batch < 0 || c_stride < 0 || c_bs < 0 || a_stride < 0 || a_bs < 0 || b_stride < 0 || b_bs < 0)
    return (int)hipErrorInvalidValue;
  const int64_t wn = width_of(n);
  const int64_t a_rows = ta ? l : m, wa = width_of(ta ? m : l), b_rows = tb ? n : l, wb = width_of(tb ? l : n);  // as stored
  if (a_stride < wa || b_stride < wb || c_stride < wn) return (int)hipErrorInvalidValue;
  if (!members_fit(batch, c_bs, m, c_stride, wn)) return (int)hipErrorInvalidValue;
  const bool c_data = m > 0 && n > 0, a_data = m > 0 && l > 0, b_data = l > 0 && n > 0;
  if (batch > 0 && ((c_data && !C) || (a_data && !A) || (b_data && !B))) return (int)hipErrorInvalidValue;
  // C's span (first member's start to last member's end) must not meet A's or B's
  if (spans_meet_any({rows_span(C, batch, c_bs, m, c_stride, wn)}, {rows_span(A, batch, a_bs, a_rows, a_stride, wa), rows_span(B, batch, b_bs, b_rows, b_stride, wb)}))
    return (int)hipErrorInvalidValue;
  if (batch == 0 || m == 0 || n == 0) return 0;
  // the path-1 bound: MSB_D1, or MSB_D1OP with a transposed operand, unless the environment overrides it
  const int path = plan(m, l, n, env_bound("M4RI_AMD_MUL_SMALL_BATCH_PATH1_MAX", ta || tb ? MSB_D1OP : MSB_D1, 64, 256, 64));
  if (path == 2) {
    if (ta || tb) return (int)hipErrorNotSupported;
    return m4ri_amd_m4rm_batch_dev(C, c_stride, c_bs, A, a_stride, a_bs, B, b_stride, b_bs, m, l, n, batch, add, stream);
  }
  hipStream_t st    = (hipStream_t)stream;
  const int64_t per = BATCH_WAVE_THREADS / 64;
  if (path == 0) {
    const WaveKernel kernel = WAVE_KERNELS[n > 32][ta][tb];
    return launch_waves(batch, [&](dim3 grid, int64_t b0, int64_t) {
      hipLaunchKernelGGL(kernel, grid, dim3(BATCH_WAVE_THREADS), 0, st, C, c_stride, c_bs, A, a_stride, a_bs, B, b_stride, b_bs, (int)m, (int)l, (int)n, b0,
                         batch, add != 0);
    });
  }
  const int64_t mb = (m + 63) / 64, blocks = mb * wn;       // waves per member: at most 16
  const int64_t members = BATCH_CHUNK * per / blocks;         // members per launch
  const BlockKernel kernel = BLOCK_KERNELS[ta][tb];
  return launch_chunked(batch, members, [&](int64_t b0, int64_t nb) {
    hipLaunchKernelGGL(kernel, dim3((unsigned)((nb * blocks + per - 1) / per)), dim3(BATCH_WAVE_THREADS), 0, st, C, c_stride, c_bs, A, a_stride, a_bs, B,
                       b_stride, b_bs, (int)m, (int)l, (int)n, (int)mb, (int)wn, b0, batch, add != 0);
  });
}

}  // namespace

extern "C" {

int m4ri_amd_plan_mul_small_batch(int64_t m, int64_t l, int64_t n) { return plan(m, l, n, MSB_D1); }

int m4ri_amd_plan_mul_small_batch_op(int64_t m, int64_t l, int64_t n, int trans_a, int trans_b) {
  return plan(m, l, n, trans_a || trans_b ? MSB_D1OP : MSB_D1);
}

int m4ri_amd_mul_small_batch_dev(word *C, int64_t c_stride, int64_t c_bs, const word *A, int64_t a_stride, int64_t a_bs, const word *B,
                                 int64_t b_stride, int64_t b_bs, int64_t m, int64_t l, int64_t n, int64_t batch, int add, void *stream) {
  return mul_small_batch(C, c_stride, c_bs, A, a_stride, a_bs, B, b_stride, b_bs, m, l, n, batch, false, false, add, stream);
}

int m4ri_amd_mul_small_batch_op_dev(word *C, int64_t c_stride, int64_t c_bs, const word *A, int64_t a_stride, int64_t a_bs, const word *B,
                                    int64_t b_stride, int64_t b_bs, int64_t m, int64_t l, int64_t n, int64_t batch, int trans_a, int trans_b,
                                    int add, void *stream) {
  return mul_small_batch(C, c_stride, c_bs, A, a_stride, a_bs, B, b_stride, b_bs, m, l, n, batch, trans_a != 0, trans_b != 0, add, stream);
}

}  // extern "C"
