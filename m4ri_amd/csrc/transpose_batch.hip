// transpose_batch.hip -- transposes of many independent small matrices, D_b = (A_b)^T, one launch for the batch.
//
// The tile kernel of transpose.hip gives a workgroup 1024 x 1024 bits; a 64 x 64 member is one 256th of that, and one block of
// transpose_block (transpose_block.h: 64 x 64 bits, a row per lane, six register exchange stages, no LDS).  Here a member, or a block
// of one, never leaves the registers.  The paths (m4ri_amd_plan_transpose_batch):
//   0  nrows, ncols <= 64: a wave per member.  Lane r < nrows loads the one word of row r, the others hold 0; after transpose_block
//      lane j holds row j of D, and lanes j < ncols store it under the mask of nrows (the old word is read only when nrows is no
//      multiple of 64).  No LDS, no barrier.
//   1  max(nrows, ncols) <= the path-1 bound: a wave per 64 x 64 block.  Block (i, w) of a member -- rows 64 i ..., word column w --
//      is loaded as A[64 i + lane][w] and stored as D[64 w + lane][i], under the mask when i is D's last word column.
//   2  everything else: the tile kernel, the member its grid's second dimension (gf2_launch_transpose_tiles), with
//      m4ri_amd_transpose_dev's contract: D's last words are written whole, the bits beyond column nrows zero.
// In place (D == A, square members up to 1024, equal strides) the register kernels are taken whatever the bound: up to 64 the wave of
// path 0 loads before it stores; above, a wave takes the block pair (i, w), (w, i) with i <= w, transposes both and stores them
// swapped (a diagonal block alone), so no wave reads a word another one writes.
// What a lane brings in beyond A's rows is 0, and what it brings in beyond A's last column ends up in rows of D that do not exist and
// are not stored.  Paths 0 and 1 never change a bit at a column >= nrows of D, a word from the width to d_stride of a row, or
// anything between members.  Every path is plain launches on the caller's stream: no allocation, no copy, no engine workspace.
#include <hip/hip_runtime.h>
#include <stdlib.h>
#include "batch_common.h"
#include "transpose_block.h"
#include "../../include/m4ri_amd.h"

namespace {

// (a workgroup is BATCH_WAVE_THREADS threads: four waves = four members (path 0), four blocks (path 1) or four block pairs (in place))
// Path 1 up to this max(nrows, ncols); a multiple of 64 in [64, 1024], 64 = path 1 empty.  Measured (tools/bench_transpose_batch.py,
// profiles/transpose_batch_bench.txt): with A and D of 256 MB each path 1 beats the batched tile launch 24.8x / 3.0x on
// the squares of 128 / 256 and loses to it at 512 / 1024 (0.76x / 0.39x), every spread under 1 %: the bound is 256.
// M4RI_AMD_TRANSPOSE_BATCH_PATH1_MAX overrides the bound for the routing of an out-of-place call.
constexpr int64_t TRB_T1  = 256;
constexpr int64_t TRB_MAX = 1024;  // the largest bound, and the largest member of an in-place call

__device__ __forceinline__ word transposed(word x, int lane) {
  uint32_t lo = (uint32_t)x, hi = (uint32_t)(x >> 32);
  transpose_block(lo, hi, lane);
  return ((word)hi << 32) | lo;
}

// path 0: a wave per member, members b0 + 4 * blockIdx.x + wave.  D may be A (in place: nrows == ncols, the strides equal): every
// lane's load is done before any lane's store, both in this wave.
__global__ __launch_bounds__(BATCH_WAVE_THREADS) void trb_wave_kernel(word *D, int64_t d_stride, int64_t d_bs, const word *A, int64_t a_stride, int64_t a_bs,
                                                                      int nrows, int ncols, int64_t b0, int64_t batch) {
  const int lane  = threadIdx.x & 63;
  const int64_t b = b0 + (int64_t)blockIdx.x * (BATCH_WAVE_THREADS / 64) + (threadIdx.x >> 6);
  if (b >= batch) return;  // wave-uniform, no barrier in this kernel
  const word mask = tail_mask(nrows);
  word *d         = D + b * d_bs + (int64_t)lane * d_stride;
  word x = 0, prev = 0;
  if (lane < nrows) x = A[b * a_bs + (int64_t)lane * a_stride];
  if (lane < ncols && (nrows & 63)) prev = *d;
  const word r = transposed(x, lane);
  if (lane < ncols) *d = (r & mask) | (prev & ~mask);
}

// path 1: a wave per 64 x 64 block.  Block t = 4 * blockIdx.x + wave of the launch is member b0 + t / (mb * wa), row block
// (t / wa) % mb, word column t % wa of A; the four blocks of a workgroup may belong to different members.
__global__ __launch_bounds__(BATCH_WAVE_THREADS) void trb_block_kernel(word *__restrict__ D, int64_t d_stride, int64_t d_bs, const word *__restrict__ A,
                                                                       int64_t a_stride, int64_t a_bs, int nrows, int ncols, int mb, int wa, int64_t b0,
                                                                       int64_t batch) {
  const int lane     = threadIdx.x & 63;
  const uint32_t t   = blockIdx.x * (uint32_t)(BATCH_WAVE_THREADS / 64) + (threadIdx.x >> 6);
  const uint32_t per = (uint32_t)(mb * wa);
  const int64_t b    = b0 + (int64_t)(t / per);
  if (b >= batch) return;  // wave-uniform, no barrier in this kernel
  const uint32_t rem = t % per;
  const int i = (int)(rem / (uint32_t)wa), w = (int)(rem % (uint32_t)wa);
  const int arow = 64 * i + lane, drow = 64 * w + lane;
  const bool old  = i == mb - 1 && (nrows & 63);  // D's last word column: the bits beyond column nrows stay
  const word mask = old ? tail_mask(nrows) : ~(word)0;
  word *d         = D + b * d_bs + (int64_t)drow * d_stride + i;
  word x = 0, prev = 0;
  if (arow < nrows) x = A[b * a_bs + (int64_t)arow * a_stride + w];
  if (drow < ncols && old) prev = *d;
  const word r = transposed(x, lane);
  if (drow < ncols) *d = (r & mask) | (prev & ~mask);
}

// in place above 64: n x n members, mb = words(n) block rows and columns, a wave per block pair (i, w), i <= w.  Pair p of a member
// counts the pairs row by row: (0, 0) ... (0, mb - 1), (1, 1) ...  The wave loads block (i, w) and block (w, i), transposes both and
// stores the first where the second was and the second where the first was; the bits beyond column n of a last word are the ones the
// same lane loaded from that word.
__global__ __launch_bounds__(BATCH_WAVE_THREADS) void trb_inplace_kernel(word *M, int64_t stride, int64_t bs, int n, int mb, int64_t b0, int64_t batch) {
  const int lane     = threadIdx.x & 63;
  const uint32_t t   = blockIdx.x * (uint32_t)(BATCH_WAVE_THREADS / 64) + (threadIdx.x >> 6);
  const uint32_t per = (uint32_t)(mb * (mb + 1) / 2);
  const int64_t b    = b0 + (int64_t)(t / per);
  if (b >= batch) return;  // wave-uniform, no barrier in this kernel
  int p = (int)(t % per), i = 0;
  while (p >= mb - i) {  // wave-uniform, at most mb <= 16 rounds
    p -= mb - i;
    ++i;
  }
  const int w      = i + p;
  const int rowi   = 64 * i + lane, roww = 64 * w + lane;
  const word maskw = w == mb - 1 ? tail_mask(n) : ~(word)0;  // of word column w; word column i < mb - 1 is whole unless i == w
  word *pu         = M + b * bs + (int64_t)rowi * stride + w;  // this lane's word of block (i, w)
  word *pl         = M + b * bs + (int64_t)roww * stride + i;  // and of block (w, i)
  word u = 0, l = 0;
  if (rowi < n) u = *pu;
  if (i != w && roww < n) l = *pl;
  const word ut = transposed(u, lane);
  if (i == w) {
    if (rowi < n) *pu = (ut & maskw) | (u & ~maskw);
    return;
  }
  const word lt = transposed(l, lane);
  if (roww < n) *pl = ut;                              // i < w <= mb - 1: word column i is no last word
  if (rowi < n) *pu = (lt & maskw) | (u & ~maskw);
}

// M4RI_AMD_TRANSPOSE_BATCH_TILES set and not "0": every out-of-place call takes the tile kernel, members of 64 and below included.
// This is contender (b) of tools/bench_transpose_batch.py, which no bound can route a member of 64 and below to.
bool tiles_forced() {
  const char *s = getenv("M4RI_AMD_TRANSPOSE_BATCH_TILES");
  return s && *s && !(s[0] == '0' && !s[1]);
}

int plan(int64_t nrows, int64_t ncols, int64_t t1) {
  if (nrows < 0 || ncols < 0) return -1;
  const int64_t mx = nrows > ncols ? nrows : ncols;
  return mx <= 64 ? 0 : mx <= t1 ? 1 : 2;
}

}  // namespace

extern "C" {

int m4ri_amd_plan_transpose_batch(int64_t nrows, int64_t ncols) { return plan(nrows, ncols, TRB_T1); }

int m4ri_amd_transpose_batch_dev(word *D, int64_t d_stride, int64_t d_bs, const word *A, int64_t a_stride, int64_t a_bs, int64_t nrows, int64_t ncols,
                                 int64_t batch, void *stream) {
  if (nrows < 0 || ncols < 0 || batch < 0 || d_stride < 0 || d_bs < 0 || a_stride < 0 || a_bs < 0) return (int)hipErrorInvalidValue;
  const int64_t wa = width_of(ncols), wd = width_of(nrows);
  if (a_stride < wa || d_stride < wd) return (int)hipErrorInvalidValue;
  const bool data = nrows > 0 && ncols > 0;
  if (data && !members_fit(batch, d_bs, ncols, d_stride, wd)) return (int)hipErrorInvalidValue;
  if (batch > 0 && data && (!D || !A)) return (int)hipErrorInvalidValue;
  // in place: the same square members of at most 1024 at the same places.  D == A in any other shape is refused whatever the batch
  // (so that what an in-place call may look like is settled by its shape alone); any other meeting of D's span and A's is an overlap.
  const bool inplace = data && D && D == A && nrows == ncols && nrows <= TRB_MAX && d_stride == a_stride && d_bs == a_bs;
  if (data && D && D == A && !inplace) return (int)hipErrorInvalidValue;
  if (!inplace && spans_meet(rows_span(D, batch, d_bs, ncols, d_stride, wd), rows_span(A, batch, a_bs, nrows, a_stride, wa))) return (int)hipErrorInvalidValue;
  if (batch == 0 || !data) return 0;
  hipStream_t st    = (hipStream_t)stream;
  const int64_t per = BATCH_WAVE_THREADS / 64;
  // the path-1 bound: TRB_T1 unless the environment overrides it, [64, TRB_MAX] in multiples of 64
  const int path = inplace ? (nrows <= 64 ? 0 : 1) : tiles_forced() ? 2 : plan(nrows, ncols, env_bound("M4RI_AMD_TRANSPOSE_BATCH_PATH1_MAX", TRB_T1, 64, TRB_MAX, 64));
  if (path == 2) return (int)gf2_launch_transpose_tiles(st, D, d_stride, d_bs, A, a_stride, a_bs, nrows, ncols, batch);
  if (path == 0)
    return launch_waves(batch, [&](dim3 grid, int64_t b0, int64_t nb) {
      hipLaunchKernelGGL(trb_wave_kernel, grid, dim3(BATCH_WAVE_THREADS), 0, st, D, d_stride, d_bs, A, a_stride, a_bs, (int)nrows, (int)ncols, b0, b0 + nb);
    });
  // waves per member: blocks out of place (at most 256), block pairs in place (at most 136)
  const int64_t mb = wd, waves = inplace ? mb * (mb + 1) / 2 : mb * wa;
  return launch_chunked(batch, BATCH_CHUNK * per / waves, [&](int64_t b0, int64_t nb) {
    const dim3 grid((unsigned)((nb * waves + per - 1) / per));
    if (inplace)
      hipLaunchKernelGGL(trb_inplace_kernel, grid, dim3(BATCH_WAVE_THREADS), 0, st, D, d_stride, d_bs, (int)nrows, (int)mb, b0, b0 + nb);
    else
      hipLaunchKernelGGL(trb_block_kernel, grid, dim3(BATCH_WAVE_THREADS), 0, st, D, d_stride, d_bs, A, a_stride, a_bs, (int)nrows, (int)ncols, (int)mb,
                         (int)wa, b0, b0 + nb);
  });
}

}  // extern "C"
