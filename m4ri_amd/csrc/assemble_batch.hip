// assemble_batch.hip -- what a caller does to the members of a batch between two batched calls, without a trip through the host:
// copies of blocks at any bit offset (mzd_submatrix, mzd_concat, mzd_stack, mzd_copy, a broadcast), the triangles of a factored
// member (mzd_extract_u, mzd_extract_l) and the permutations m4ri_amd_ple_batch_dev left on the device (mzd_apply_p_left / _right and
// their _trans forms).
//
// The block copy and the triangles are one kernel.  An item is a destination word (VEC: a pair of words, 16 bytes) of one row of one
// member; the items of a launch are numbered member by member, row by row, and a thread takes ASM_ITEMS of them 256 apart, so that the
// lanes of a wave write consecutive words whatever the members' size.  A destination word is a 64-bit funnel shift of at most two
// source words, stored under the mask of the block's edges; a source word is loaded only if it holds a bit of the block.  The
// triangles add a per-row mask of the source and the diagonal's bit (offsets and shift zero).  HBM-bound: every word of the block is
// read once (twice from the cache at a shift) and written once.
// The permutations compose their transpositions into one gather index first (serial: one lane, or registers across a wave), then
// move every row or column once.  The paths (m4ri_amd_plan_perm_batch):
//   0  nrows, ncols <= 64: a wave per member.  Lane r holds row r and entry r of P and of the index; the transpositions are replayed on
//      the index with readlane, rows move by ds_bpermute, columns as transpose_block -> bpermute -> transpose_block.
//   1  the member, P and the index in LDS within BATCH_LDS_BUDGET: a workgroup per member.  Thread 0 replays the transpositions on the
//      index in LDS while the others stage the rows; then rows are copied out under the index, columns gathered bit by bit.
//   2  everything else: P is downloaded and checked on the host, the members go one by one through m4ri_amd_apply_p_left_dev /
//      m4ri_amd_apply_p_right_dev on a clean scratch copy.  Allocates and BLOCKS.
// Paths 0 and 1 and the copy kernel are plain launches on the caller's stream: no allocation, no copy, no engine workspace.
#include <hip/hip_runtime.h>
#include <vector>
#include "batch_common.h"
#include "transpose_block.h"
#include "../../include/m4ri_amd.h"

namespace {

constexpr int ASM_ITEMS            = 4;                    // items of a thread, BATCH_WAVE_THREADS apart
constexpr int64_t ASM_LAUNCH_ITEMS = (int64_t)1 << 31;     // items of a launch: they are numbered in 32 bits
constexpr int64_t ASM_MAX_UNITS    = (int64_t)1 << 30;     // items of a row: a block of more than 2^36 columns is refused

struct CopyArgs {
  word *D;        // word 0 of row d_row of member 0
  const word *A;  // word 0 of row a_row of member 0
  int64_t d_stride, d_bs, a_stride, a_bs;
  int64_t d_col, a_col, cols;  // bit offsets in the rows, the block's columns
  int64_t d_w0;                // d_col / 64
  uint32_t nw, units;          // destination words of a row; items of a row (VEC: pairs)
  // the triangles (tri != 0: 1 upper, 2 lower; d_col = a_col = 0)
  int tri, diag;
  const int32_t *rank;  // or NULL
  int64_t k;            // min(nrows, ncols): what a rank is clamped to
  // this launch: members b0 ..., rows r0 ... r0 + nr - 1 of the block, `total` items
  int64_t b0, r0;
  uint32_t per_member, total;  // nr * units
};

// destination word w (of nw) of block row i of a member: d and a point at word 0 of that row in D and in A
__device__ __forceinline__ void copy_word(const CopyArgs &p, word *d, const word *a, int64_t i, uint32_t w, int64_t rank) {
  const int64_t j0 = 64 * (int64_t)w - (p.d_col & 63);  // the block column of the word's bit 0
  const int64_t lo = j0 < 0 ? 0 : j0, hi = j0 + 64 < p.cols ? j0 + 64 : p.cols;
  const int b_lo = (int)(lo - j0), b_hi = (int)(hi - j0);  // the word's bits [b_lo, b_hi) are the block's
  const word m = (b_hi == 64 ? ~(word)0 : (((word)1 << b_hi) - 1)) & (~(word)0 << b_lo);
  word amask = ~(word)0, dbit = 0;
  bool need  = true;
  if (p.tri) {  // j0 = 64 w: the word's columns are j0 ... j0 + 63
    const int64_t c = i - j0;  // the diagonal's bit in this word, if in [0, 64)
    if (p.tri == 1) {
      amask = c < 0 ? ~(word)0 : c >= 63 ? 0 : ~(word)0 << (c + 1);
      if (i >= rank) amask = 0;
    } else {
      const int64_t lim = (i < rank ? i : rank) - j0;
      amask = lim <= 0 ? 0 : lim >= 64 ? ~(word)0 : (((word)1 << lim) - 1);
    }
    const bool on = c >= 0 && c < 64 && i < p.k && !(p.tri == 1 && i >= rank);
    if (on && p.diag == 1) dbit = (word)1 << c;
    if (on && p.diag == 2) dbit = a[i >> 6] & ((word)1 << c);
    need = amask != 0;
  }
  word v = 0;
  if (need) {
    const int64_t s = p.a_col + j0, first = p.a_col + lo, end = p.a_col + hi;  // source bits [first, end) are wanted
    const int64_t sw = s >> 6;                                                   // floor: s may be negative in a row's first word
    const int sh = (int)(s & 63);
    if (64 * sw + 64 > first) v = a[sw] >> sh;
    if (sh && 64 * (sw + 1) < end) v |= a[sw + 1] << (64 - sh);
  }
  v = (v & amask) | dbit;
  word *dst = d + p.d_w0 + w;
  *dst = m == ~(word)0 ? v : (v & m) | (*dst & ~m);
}

// VEC: d_col and a_col are multiples of 64, no triangle, and every row's first word is 16-byte aligned in both operands.
template <bool VEC>
__global__ __launch_bounds__(BATCH_WAVE_THREADS) void asm_copy_kernel(CopyArgs p) {
  const uint32_t g0 = blockIdx.x * (uint32_t)(BATCH_WAVE_THREADS * ASM_ITEMS) + threadIdx.x;
#pragma unroll
  for (int it = 0; it < ASM_ITEMS; ++it) {
    const uint32_t g = g0 + (uint32_t)it * BATCH_WAVE_THREADS;
    if (g >= p.total) return;  // g < 2^31 + 1024: no wrap
    const uint32_t mb = g / p.per_member, k = g - mb * p.per_member;
    const uint32_t ri = k / p.units, u = k - ri * p.units;
    const int64_t b = p.b0 + mb, i = p.r0 + ri;
    word *d       = p.D + b * p.d_bs + i * p.d_stride;
    const word *a = p.A + b * p.a_bs + i * p.a_stride;
    int64_t rank  = p.k;
    if (p.tri && p.rank) {
      rank = p.rank[b];
      rank = rank < 0 ? 0 : rank > p.k ? p.k : rank;
    }
    if (VEC) {
      const uint32_t w = 2 * u;
      if (w + 1 < p.nw && (w + 2 < p.nw || !(p.cols & 63))) {  // two whole words
        *reinterpret_cast<ulonglong2 *>(d + p.d_w0 + w) = *reinterpret_cast<const ulonglong2 *>(a + (p.a_col >> 6) + w);
      } else {
        copy_word(p, d, a, i, w, rank);
        if (w + 1 < p.nw) copy_word(p, d, a, i, w + 1, rank);
      }
    } else {
      copy_word(p, d, a, i, u, rank);
    }
  }
}

bool aligned16(const word *p, int64_t stride, int64_t bs) { return ((uintptr_t)p & 15) == 0 && !(stride & 1) && !(bs & 1); }

// the launches of a validated, non-empty copy: p holds everything but the launch's own fields
int launch_copy(CopyArgs p, int64_t rows, int64_t batch, hipStream_t st) {
  const bool vec = !p.tri && !(p.d_col & 63) && !(p.a_col & 63) && aligned16(p.D + p.d_w0, p.d_stride, p.d_bs) &&
                   aligned16(p.A + (p.a_col >> 6), p.a_stride, p.a_bs);
  p.units = vec ? (p.nw + 1) / 2 : p.nw;
  const int64_t rows_per = ASM_LAUNCH_ITEMS / p.units < rows ? ASM_LAUNCH_ITEMS / p.units : rows;  // >= 2: units <= 2^30
  const int64_t members  = ASM_LAUNCH_ITEMS / (rows_per * p.units);                                 // >= 1
  const int64_t per_wg   = BATCH_WAVE_THREADS * ASM_ITEMS;
  for (int64_t r0 = 0; r0 < rows; r0 += rows_per) {
    const int64_t nr = rows - r0 < rows_per ? rows - r0 : rows_per;
    p.r0 = r0, p.per_member = (uint32_t)(nr * p.units);
    HIPTRY(launch_chunked(batch, members, [&](int64_t b0, int64_t nb) {
      p.b0 = b0, p.total = (uint32_t)(nb * p.per_member);  // <= 2^31
      const dim3 grid((unsigned)(((int64_t)p.total + per_wg - 1) / per_wg));
      if (vec) hipLaunchKernelGGL(asm_copy_kernel<true>, grid, dim3(BATCH_WAVE_THREADS), 0, st, p);
      else hipLaunchKernelGGL(asm_copy_kernel<false>, grid, dim3(BATCH_WAVE_THREADS), 0, st, p);
    }));
  }
  return 0;
}

// ---- the permutations -------------------------------------------------------------------------------------------------------------

__device__ __forceinline__ word transposed(word x, int lane) {
  uint32_t lo = (uint32_t)x, hi = (uint32_t)(x >> 32);
  transpose_block(lo, hi, lane);
  return ((word)hi << 32) | lo;
}

// path 0: a wave per member, members b0 + 4 * blockIdx.x + wave.  n = the side the permutation acts on, L = min(length, n), asc: the
// transpositions in ascending order.
__global__ __launch_bounds__(BATCH_WAVE_THREADS) void perm_wave_kernel(word *A, int64_t stride, int64_t a_bs, int nrows, int ncols, const int32_t *P,
                                                                       int64_t p_bs, int L, int right, int asc, int32_t *status, int64_t b0, int64_t batch) {
  const int lane  = threadIdx.x & 63;
  const int64_t b = b0 + (int64_t)blockIdx.x * (BATCH_WAVE_THREADS / 64) + (threadIdx.x >> 6);
  if (b >= batch) return;  // wave-uniform, no barrier in this kernel
  const int n  = right ? ncols : nrows;
  const int pv = lane < L ? P[b * p_bs + lane] : lane;
  if (__ballot(lane < L && (pv < 0 || pv >= n))) {  // wave-uniform: the member stays as it is
    if (status && lane == 0) status[b] = -1;
    return;
  }
  if (status && lane == 0) status[b] = 0;
  int idx = lane;
  for (int t = 0; t < L; ++t) {  // wave-uniform
    const int i = asc ? t : L - 1 - t;
    const int p = __builtin_amdgcn_readlane(pv, i);
    if (p == i) continue;
    const int vi = __builtin_amdgcn_readlane(idx, i), vp = __builtin_amdgcn_readlane(idx, p);
    idx = lane == i ? vp : lane == p ? vi : idx;
  }
  const word mask = tail_mask(ncols);
  word *g         = A + b * a_bs + (int64_t)lane * stride;
  word x          = 0;
  if (lane < nrows) x = *g;
  word y;
  if (right) y = transposed(bpermute64(transposed(x & mask, lane), idx), lane);
  else y = bpermute64(x, idx);
  if (lane < nrows) *g = (y & mask) | (x & ~mask);
}

// path 1: a workgroup per member.  LDS: the member's rows (width words each), then P (L entries), the index (n entries) and a flag.
__global__ __launch_bounds__(BATCH_MAX_THREADS) void perm_block_kernel(word *A, int64_t stride, int64_t a_bs, int nrows, int ncols, const int32_t *P,
                                                                       int64_t p_bs, int L, int right, int asc, int32_t *status, int64_t b0) {
  extern __shared__ word perm_lds[];
  const int t = threadIdx.x, T = blockDim.x;
  const int64_t b = b0 + blockIdx.x;
  const int n = right ? ncols : nrows, width = (ncols + 63) >> 6;
  word *rows   = perm_lds;
  int32_t *pl  = reinterpret_cast<int32_t *>(rows + (size_t)nrows * width);
  int32_t *idx = pl + L;
  word *g      = A + b * a_bs;
  int32_t *flag = idx + n;  // an entry out of range was seen (a flag of the kernel's own: the LDS budget is spent to the byte)
  if (t == 0) *flag = 0;
  for (int i = t; i < n; i += T) idx[i] = i;
  __syncthreads();
  for (int i = t; i < L; i += T) {
    const int v = P[b * p_bs + i];
    pl[i]       = v;
    if (v < 0 || v >= n) *flag = 1;
  }
  __syncthreads();
  if (*flag) {  // workgroup-uniform: the member stays as it is
    if (status && t == 0) status[b] = -1;
    return;
  }
  if (t == 0) {
    if (status) status[b] = 0;
    for (int s = 0; s < L; ++s) {
      const int i = asc ? s : L - 1 - s, p = pl[i];
      if (p == i) continue;
      const int vi = idx[i];
      idx[i] = idx[p];
      idx[p] = vi;
    }
  } else {
    const int total = nrows * width;
    for (int k = t - 1; k < total; k += T - 1) {
      const int i = k / width, w = k - i * width;
      rows[k] = g[(int64_t)i * stride + w];
    }
  }
  __syncthreads();
  const word mask = tail_mask(ncols);
  const int total = nrows * width;
  for (int k = t; k < total; k += T) {
    const int i = k / width, w = k - i * width;
    word v;
    if (!right) {
      v = rows[idx[i] * width + w];
    } else {
      v = 0;
      const word *r = rows + i * width;
      const int c1  = ncols - 64 * w < 64 ? ncols - 64 * w : 64;
      for (int c = 0; c < c1; ++c) {
        const int s = idx[64 * w + c];
        v |= ((r[s >> 6] >> (s & 63)) & 1) << c;
      }
    }
    store_masked(g + (int64_t)i * stride + w, v, w == width - 1, mask);
  }
}

__global__ void perm_status_kernel(int32_t *status, int64_t batch) {
  for (int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; b < batch; b += (int64_t)gridDim.x * blockDim.x) status[b] = 0;
}

int64_t perm_lds_bytes(int64_t nrows, int64_t ncols, int right) { return nrows * width_of(ncols) * 8 + 8 * (right ? ncols : nrows) + 8; }

// p0: the largest side of path 0; p1: the LDS bytes path 1 may use.  Measured (tools/bench_assemble_batch.py,
// profiles/assemble_batch_bench.txt) on 256 MiB of members, every spread under 1 %: at 64 x 64 path 0 beats path 1 3.2x on
// both sides, at 1088 x 1088 (the largest square of path 1) path 1 beats path 2 63x (left) and 15x (right): each path keeps all it can
// hold.  M4RI_AMD_PERM_BATCH_PATH0_MAX and M4RI_AMD_PERM_BATCH_PATH1_MAX override the bounds for the routing of a call.
int plan_perm(int64_t nrows, int64_t ncols, int right, int64_t p0, int64_t p1) {
  if (nrows < 0 || ncols < 0) return -1;
  if (nrows <= p0 && ncols <= p0) return 0;
  const int64_t width = width_of(ncols);
  if (nrows > p1 / 8 || width > p1 / 8 || ncols > p1 / 8 || nrows * width > p1 / 8) return 2;
  return perm_lds_bytes(nrows, ncols, right) <= p1 ? 1 : 2;
}

// path 2.  A validated call with non-empty members and L > 0.
int run_perm_path2(word *A, int64_t stride, int64_t a_bs, int64_t nrows, int64_t ncols, int64_t batch, const int32_t *P, int64_t p_bs, int64_t L, int right,
                   int trans, int32_t *status, hipStream_t st) {
  const int64_t width = width_of(ncols), n = right ? ncols : nrows;
  std::vector<int32_t> hp((size_t)((batch - 1) * p_bs + L)), hs((size_t)batch, 0);
  HIPTRY(hipMemcpyAsync(hp.data(), P, hp.size() * 4, hipMemcpyDeviceToHost, st));
  HIPTRY(hipStreamSynchronize(st));
  word *s = nullptr;
  Scratch scratch(st);
  HIPTRY(scratch.words(&s, nrows * width));
  for (int64_t b = 0; b < batch; ++b) {
    const int32_t *p = &hp[(size_t)(b * p_bs)];
    for (int64_t i = 0; i < L; ++i)
      if (p[i] < 0 || p[i] >= n) hs[(size_t)b] = -1;
    if (hs[(size_t)b]) continue;
    word *Ab = A + b * a_bs;
    HIPTRY(clean_copy(s, width, Ab, stride, nrows, ncols, st));
    HIPTRY(right ? m4ri_amd_apply_p_right_dev(s, width, nrows, ncols, p, L, trans, st) : m4ri_amd_apply_p_left_dev(s, width, nrows, ncols, p, L, trans, st));
    HIPTRY(gf2_launch_copy_masked(st, Ab, stride, s, width, nrows, ncols));
  }
  if (status) HIPTRY(hipMemcpyAsync(status, hs.data(), hs.size() * 4, hipMemcpyHostToDevice, st));
  HIPTRY(hipStreamSynchronize(st));
  return scratch.done();
}

int apply_p_batch(word *A, int64_t stride, int64_t a_bs, int64_t nrows, int64_t ncols, int64_t batch, const int32_t *P, int64_t p_bs, int64_t length,
                  int trans, int32_t *status, int right, hipStream_t st) {
  if (nrows < 0 || ncols < 0 || batch < 0 || stride < 0 || a_bs < 0 || p_bs < 0 || length < 0) return (int)hipErrorInvalidValue;
  const int64_t width = width_of(ncols), n = right ? ncols : nrows;
  const bool data = nrows > 0 && ncols > 0;
  if (data && stride < width) return (int)hipErrorInvalidValue;
  if (data && !members_fit(batch, a_bs, nrows, stride, width)) return (int)hipErrorInvalidValue;
  const int64_t L = length < n ? length : n;
  if (batch > 0 && data && (!A || (L > 0 && !P))) return (int)hipErrorInvalidValue;
  if (batch == 0 || !data) return 0;
  if (spans_meet_any({rows_span(A, batch, a_bs, nrows, stride, width), entries_span(status, batch, 1, 1, 4)}, {entries_span(P, batch, p_bs, L, 4)}))
    return (int)hipErrorInvalidValue;
  if (L == 0) {  // the identity
    if (!status) return 0;
    const int64_t blocks = (batch + 255) / 256;
    hipLaunchKernelGGL(perm_status_kernel, dim3((unsigned)(blocks < 4096 ? blocks : 4096)), dim3(256), 0, st, status, batch);
    return (int)hipGetLastError();
  }
  const int asc  = right ? trans != 0 : trans == 0;
  const int path = plan_perm(nrows, ncols, right, env_bound("M4RI_AMD_PERM_BATCH_PATH0_MAX", 64, 0, 64),
                             env_bound("M4RI_AMD_PERM_BATCH_PATH1_MAX", BATCH_LDS_BUDGET, 0, BATCH_LDS_BUDGET));
  if (path == 0)
    return launch_waves(batch, [&](dim3 grid, int64_t b0, int64_t nb) {
      hipLaunchKernelGGL(perm_wave_kernel, grid, dim3(BATCH_WAVE_THREADS), 0, st, A, stride, a_bs, (int)nrows, (int)ncols, P, p_bs, (int)L, right, asc, status,
                         b0, b0 + nb);
    });
  if (path == 2) return run_perm_path2(A, stride, a_bs, nrows, ncols, batch, P, p_bs, L, right, trans, status, st);
  HIPTRY(set_max_dynamic_lds(BATCH_LDS_BUDGET, perm_block_kernel));
  const size_t lds  = (size_t)(nrows * width * 8 + 4 * (L + n) + 8);
  const int threads = block_threads(nrows, width);
  return launch_members(batch, [&](dim3 grid, int64_t b0) {
    hipLaunchKernelGGL(perm_block_kernel, grid, dim3(threads), lds, st, A, stride, a_bs, (int)nrows, (int)ncols, P, p_bs, (int)L, right, asc,
                       status, b0);
  });
}

}  // namespace

extern "C" {

int m4ri_amd_copy_block_batch_dev(word *D, int64_t d_stride, int64_t d_bs, int64_t d_row, int64_t d_col, const word *A, int64_t a_stride, int64_t a_bs,
                                  int64_t a_row, int64_t a_col, int64_t rows, int64_t cols, int64_t batch, void *stream) {
  if (rows < 0 || cols < 0 || batch < 0 || d_stride < 0 || d_bs < 0 || a_stride < 0 || a_bs < 0 || d_row < 0 || d_col < 0 || a_row < 0 || a_col < 0)
    return (int)hipErrorInvalidValue;
  if (cols > 64 * ASM_MAX_UNITS - 64 || d_col > INT64_MAX - cols - 64 || a_col > INT64_MAX - cols - 64) return (int)hipErrorInvalidValue;
  const bool data  = rows > 0 && cols > 0;
  const int64_t d0 = d_col >> 6, d1 = width_of(d_col + cols), a0 = a_col >> 6, a1 = width_of(a_col + cols);
  if (data && (d_stride < d1 || a_stride < a1)) return (int)hipErrorInvalidValue;
  if (data && !members_fit(batch, d_bs, rows, d_stride, d1 - d0)) return (int)hipErrorInvalidValue;
  if (batch > 0 && data && (!D || !A)) return (int)hipErrorInvalidValue;
  if (batch == 0 || !data) return 0;
  // the blocks: words [d0, d1) and [a0, a1) of `rows` rows from d_row and a_row on.  One that starts beyond the address space is refused.
  const wide d_first = (wide)d_row * (wide)d_stride + (wide)d0, a_first = (wide)a_row * (wide)a_stride + (wide)a0, space = (wide)1 << 61;
  if (d_first >= space || a_first >= space) return (int)hipErrorInvalidValue;
  if (spans_meet(rows_span(D, batch, d_bs, rows, d_stride, d1 - d0, (int64_t)d_first), rows_span(A, batch, a_bs, rows, a_stride, a1 - a0, (int64_t)a_first)))
    return (int)hipErrorInvalidValue;
  CopyArgs p{};
  p.D = D + d_row * d_stride, p.A = A + a_row * a_stride;
  p.d_stride = d_stride, p.d_bs = d_bs, p.a_stride = a_stride, p.a_bs = a_bs;
  p.d_col = d_col, p.a_col = a_col, p.cols = cols, p.d_w0 = d0, p.nw = (uint32_t)(d1 - d0);
  // the kernel counts the block's columns from the destination word's bit 0: d_col below 64 from here on
  p.d_col = d_col & 63;
  return launch_copy(p, rows, batch, (hipStream_t)stream);
}

int m4ri_amd_extract_tri_batch_dev(word *D, int64_t d_stride, int64_t d_bs, const word *A, int64_t a_stride, int64_t a_bs, int64_t nrows, int64_t ncols,
                                   int64_t batch, int upper, int diag, const int32_t *rank, void *stream) {
  if (nrows < 0 || ncols < 0 || batch < 0 || d_stride < 0 || d_bs < 0 || a_stride < 0 || a_bs < 0) return (int)hipErrorInvalidValue;
  if (diag < 0 || diag > 2) return (int)hipErrorInvalidValue;
  if (nrows > INT32_MAX || ncols > INT32_MAX) return (int)hipErrorInvalidValue;  // a rank: 32 bits
  const int64_t k = nrows < ncols ? nrows : ncols, rows = upper ? k : nrows, cols = upper ? ncols : k;
  const int64_t wd = width_of(cols), wa = width_of(ncols);
  const bool data  = k > 0;
  if (data && (d_stride < wd || a_stride < wa)) return (int)hipErrorInvalidValue;
  if (data && !members_fit(batch, d_bs, rows, d_stride, wd)) return (int)hipErrorInvalidValue;
  if (batch > 0 && data && (!D || !A)) return (int)hipErrorInvalidValue;
  if (batch == 0 || !data) return 0;
  if (spans_meet_any({rows_span(D, batch, d_bs, rows, d_stride, wd)}, {rows_span(A, batch, a_bs, nrows, a_stride, wa), entries_span(rank, batch, 1, 1, 4)}))
    return (int)hipErrorInvalidValue;
  CopyArgs p{};
  p.D = D, p.A = A, p.d_stride = d_stride, p.d_bs = d_bs, p.a_stride = a_stride, p.a_bs = a_bs;
  p.cols = cols, p.nw = (uint32_t)wd, p.tri = upper ? 1 : 2, p.diag = diag, p.rank = rank, p.k = k;
  return launch_copy(p, rows, batch, (hipStream_t)stream);
}

int m4ri_amd_apply_p_left_batch_dev(word *A, int64_t stride, int64_t a_bs, int64_t nrows, int64_t ncols, int64_t batch, const int32_t *P, int64_t p_bs,
                                    int64_t length, int trans, int32_t *status, void *stream) {
  return apply_p_batch(A, stride, a_bs, nrows, ncols, batch, P, p_bs, length, trans, status, 0, (hipStream_t)stream);
}

int m4ri_amd_apply_p_right_batch_dev(word *A, int64_t stride, int64_t a_bs, int64_t nrows, int64_t ncols, int64_t batch, const int32_t *P, int64_t p_bs,
                                     int64_t length, int trans, int32_t *status, void *stream) {
  return apply_p_batch(A, stride, a_bs, nrows, ncols, batch, P, p_bs, length, trans, status, 1, (hipStream_t)stream);
}

int m4ri_amd_plan_perm_batch(int64_t nrows, int64_t ncols, int right) { return plan_perm(nrows, ncols, right != 0, 64, BATCH_LDS_BUDGET); }

}  // extern "C"
