// echelon_batch.hip -- (reduced) row echelon forms of many independent small matrices, one launch for the batch.
//
// The rule is mzd_echelonize's (echelon.hip's header, pinned by tests/test_echelon_oracle.py): columns left to right,
// the pivot of a column is the first row at or below the rank with the bit set, it is swapped up to the rank's row, and it is added
// into the rows below (full = 0) or into every other row with the bit (full = 1).  The paths (m4ri_amd_plan_echelonize_batch):
//   0  nrows, ncols <= 64: a wave per member, lane i holds row i; pivot = lowest lane >= rank of a ballot, no LDS, no barrier.
//   1  the member fits in LDS: a workgroup per member, rows staged in LDS under a row-permutation index (the swap of a column is
//      two index entries, applied by their owner threads in the next column's flag pass); two barriers per column with a pivot.
//   2  larger members up to BATCH_CAP_BYTES: a workgroup per member, rows in place in global memory, rows swapped physically (the last
//      word under the column mask); three barriers per column with a pivot.
//   (Paths 1 and 2 are batch_common.h's workgroup-per-member scheme; the column's pieces are there, the update is here.)
//   3  above the cap: the members one by one through m4ri_amd_echelonize_dev, then one launch for the pivots.  Blocking.
// Paths 0-2 are one launch each (plus chunking above 2^30 workgroups), no allocation, no copy, no host synchronisation.
// Memory rules: bits at columns >= ncols of a row's last word are never changed, nor the words from `width` to `stride` of a row,
// nor anything between members.
#include <hip/hip_runtime.h>
#include <vector>
#include "batch_common.h"
#include "../../include/m4ri_amd.h"

namespace {

// path 0: a wave per member, lane i = row i (one word).  Members b0 + 4 * blockIdx.x + wave.
__global__ __launch_bounds__(BATCH_WAVE_THREADS) void eb_wave_kernel(word *__restrict__ A, int64_t stride, int64_t a_bs, int nrows, int ncols,
                                                                     int64_t b0, int64_t batch, int full, int32_t *__restrict__ rank_out,
                                                                     int32_t *__restrict__ pivots, int mn) {
  const int lane  = threadIdx.x & 63;
  const int64_t b = b0 + (int64_t)blockIdx.x * (BATCH_WAVE_THREADS / 64) + (threadIdx.x >> 6);
  if (b >= batch) return;  // wave-uniform, no barrier in this kernel
  word *g          = A + b * a_bs;
  const word mask  = tail_mask(ncols);
  word orig = 0, v = 0;
  if (lane < nrows) {
    orig = g[(int64_t)lane * stride];
    v    = orig & mask;
  }
  int rank = 0, piv = -1;
  for (int c = 0; c < ncols && rank < nrows; ++c) {
    const int bit   = (int)((v >> c) & 1);
    const word cand = __ballot(bit) & (~(word)0 << rank);
    if (!cand) continue;
    const int p   = (int)__builtin_ctzll(cand);
    const word pw = readlane64(v, p);
    if (bit && lane != p && (full || lane > rank)) v ^= pw;
    const word vr = readlane64(v, rank);  // row `rank` has no bit c unless it is the pivot: unchanged by the update
    if (lane == rank) {
      v   = pw;
      piv = c;
    } else if (lane == p) {
      v = vr;
    }
    ++rank;
  }
  if (lane < nrows) g[(int64_t)lane * stride] = (v & mask) | (orig & ~mask);
  if (lane < mn && pivots) pivots[b * mn + lane] = piv;
  if (lane == 0) rank_out[b] = rank;
}

// paths 1 (INLDS) and 2: a workgroup per member.  Dynamic LDS (16-byte carve offsets):
//   INLDS: rows [nrows][ldw] words | perm [nrows] int32 (rounded up to 16 B) | flags [2][nfw] words
//   else:  flags [2][nfw] words
// Row i of the flag pass is owned by thread i % blockDim.x (the lane of its ballot); flags[c & 1] bit i = bit c of logical row i.
template <bool INLDS>
__global__ __launch_bounds__(BATCH_MAX_THREADS) void eb_block_kernel(word *__restrict__ A, int64_t stride, int64_t a_bs, int nrows, int ncols,
                                                                     int ldw, int64_t b0, int full, int32_t *__restrict__ rank_out,
                                                                     int32_t *__restrict__ pivots, int mn) {
  extern __shared__ __attribute__((aligned(16))) char eb_smem[];
  const int T = blockDim.x, t = threadIdx.x;
  const int64_t b  = b0 + blockIdx.x;
  word *g          = A + b * a_bs;
  const int width  = (ncols + 63) >> 6;
  const int nfw    = (nrows + 63) >> 6;
  const word mask  = tail_mask(ncols);
  word *rows       = reinterpret_cast<word *>(eb_smem);
  int32_t *perm    = reinterpret_cast<int32_t *>(eb_smem + (INLDS ? (size_t)nrows * ldw * 8 : 0));
  word *flags      = reinterpret_cast<word *>(eb_smem + (INLDS ? (size_t)nrows * ldw * 8 + pad16((size_t)nrows * 4) : 0));

  if (INLDS) {
    stage_rows_in(rows, ldw, g, stride, nrows, width, mask, t, T);
    for (int i = t; i < nrows; i += T) perm[i] = i;
    __syncthreads();
  }

  int rank = 0;
  PendingSwap sw;  // INLDS: the previous column's pending swap of perm[rank] and perm[p]
  for (int c = 0; c < ncols && rank < nrows; ++c) {
    word *buf    = flags + (c & 1) * nfw;
    const int cw = c >> 6, cb = c & 63;
    if (INLDS) flag_pass<true>(buf, rows, ldw, perm, sw, nrows, cw, cb, t, T);
    else flag_pass<false>(buf, g, stride, perm, sw, nrows, cw, cb, t, T);
    __syncthreads();
    const int p = find_pivot(buf, rank, nfw);
    if (p < 0) continue;  // no writes this column; the next flag pass uses the other buffer
    if (t == 0 && pivots) pivots[b * mn + rank] = c;
    const word *prow;
    if (INLDS) {
      const int P = perm[p];
      prow        = rows + P * ldw;
      sw.record(perm, rank, p, P);
    } else {
      if (p != rank) {  // physical swap, the bits behind ncols stay where they are
        swap_rows_global(g + (int64_t)rank * stride, g + (int64_t)p * stride, cw, width, mask, t, T);
        __syncthreads();
      }
      prow = g + (int64_t)rank * stride;
    }
    // the update: flagged rows i != p (row `rank` is unflagged when p != rank), below the rank only unless full.
    for_each_item(0, nrows, cw, width, t, T, [&](int i, int w) {
      if (flag_of(buf, i) && i != p && (full || i > rank)) {
        word x = prow[w];
        if (INLDS) {
          rows[perm[i] * ldw + w] ^= x;
        } else {
          if (w == width - 1) x &= mask;
          g[(int64_t)i * stride + w] ^= x;
        }
      }
    });
    ++rank;
    __syncthreads();
  }

  if (INLDS) {
    sw.finish(perm, nrows, t, T);
    __syncthreads();
    store_rows_out(g, stride, rows, ldw, perm, nrows, width, mask, t, T);
  }
  if (pivots)
    for (int i = rank + t; i < mn; i += T) pivots[b * mn + i] = -1;
  if (t == 0) rank_out[b] = rank;
}

// path 3 helpers: the last words of every row saved and cleared before m4ri_amd_echelonize_dev (which wants zero bits behind
// ncols and may clear them), merged back after; then rank and pivots from the echelon form (pivot of row i < rank = its first bit).
__global__ void eb_tail_save_kernel(word *__restrict__ A, int64_t stride, int64_t a_bs, int64_t nrows, int64_t width, word mask, int64_t total,
                                    word *__restrict__ save) {
  const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= total) return;
  word *x = A + (k / nrows) * a_bs + (k % nrows) * stride + width - 1;
  save[k] = *x;
  *x &= mask;
}

__global__ void eb_tail_restore_kernel(word *__restrict__ A, int64_t stride, int64_t a_bs, int64_t nrows, int64_t width, word mask, int64_t total,
                                       const word *__restrict__ save) {
  const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= total) return;
  word *x = A + (k / nrows) * a_bs + (k % nrows) * stride + width - 1;
  *x      = (*x & mask) | (save[k] & ~mask);
}

// a wave per (member, row < mn)
__global__ __launch_bounds__(256) void eb_pivots_kernel(const word *__restrict__ A, int64_t stride, int64_t a_bs, int64_t width, word mask, int64_t mn,
                                                        int64_t total, const int32_t *__restrict__ rank, int32_t *__restrict__ pivots) {
  const int64_t k = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const int lane  = threadIdx.x & 63;
  if (k >= total) return;
  const int64_t b = k / mn, i = k % mn;
  int piv         = -1;
  if (i < rank[b]) {
    const word *row = A + b * a_bs + i * stride;
    for (int64_t w0 = 0; w0 < width; w0 += 64) {
      const int64_t w = w0 + lane;
      word x          = w < width ? row[w] : 0;
      if (w == width - 1) x &= mask;
      const word nz = __ballot(x != 0);
      if (nz) {
        const int l = (int)__builtin_ctzll(nz);
        piv         = (int)((w0 + l) * 64 + (int64_t)__builtin_ctzll(readlane64(x, l)));
        break;
      }
    }
  }
  if (lane == 0) pivots[k] = piv;
}

int64_t lds_bytes_path1(int64_t nrows, int64_t width) {
  return nrows * lds_row_words(width) * 8 + (int64_t)pad16((size_t)nrows * 4) + 2 * ((nrows + 63) / 64) * 8;
}

int run_path3(word *A, int64_t stride, int64_t a_bs, int64_t nrows, int64_t ncols, int64_t batch, int full, int32_t *rank, int32_t *pivots,
              hipStream_t st) {
  const int64_t width = width_of(ncols), mn = nrows < ncols ? nrows : ncols;
  const word mask     = tail_mask((int)(ncols & 63));
  const int64_t total = batch * nrows;
  word *save          = nullptr;
  std::vector<int32_t> ranks((size_t)batch);
  Scratch scratch(st);
  if (ncols & 63) {
    HIPTRY(scratch.words(&save, total));
    hipLaunchKernelGGL(eb_tail_save_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, A, stride, a_bs, nrows, width, mask, total, save);
    HIPTRY(hipGetLastError());
  }
  for (int64_t b = 0; b < batch; ++b)
    if (int rc = m4ri_amd_echelonize_dev(A + b * a_bs, stride, nrows, ncols, full, &ranks[(size_t)b], st)) return rc;
  if (save) {
    hipLaunchKernelGGL(eb_tail_restore_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, A, stride, a_bs, nrows, width, mask, total, save);
    HIPTRY(hipGetLastError());
  }
  HIPTRY(hipMemcpyAsync(rank, ranks.data(), (size_t)batch * 4, hipMemcpyHostToDevice, st));
  if (pivots) {
    const int64_t rows = batch * mn;
    hipLaunchKernelGGL(eb_pivots_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, st, A, stride, a_bs, width, mask, mn, rows, rank, pivots);
    HIPTRY(hipGetLastError());
  }
  HIPTRY(hipStreamSynchronize(st));
  return scratch.done();
}

}  // namespace

extern "C" {

int m4ri_amd_plan_echelonize_batch(int64_t nrows, int64_t ncols) {
  if (nrows < 0 || ncols < 0) return -1;
  if (nrows <= 64 && ncols <= 64) return 0;
  const int64_t width = width_of(ncols);
  if (nrows > BATCH_CAP_BYTES / 8 || width > BATCH_CAP_BYTES / 8 || nrows * width > BATCH_CAP_BYTES / 8) return 3;
  return lds_bytes_path1(nrows, width) <= BATCH_LDS_BUDGET ? 1 : 2;
}

int m4ri_amd_echelonize_batch_dev(word *A, int64_t stride, int64_t a_bs, int64_t nrows, int64_t ncols, int64_t batch, int full, int32_t *rank,
                                  int32_t *pivots, void *stream) {
  if (nrows < 0 || ncols < 0 || batch < 0 || stride < 0 || a_bs < 0) return (int)hipErrorInvalidValue;
  const int64_t width = width_of(ncols);
  if (stride < width) return (int)hipErrorInvalidValue;
  if (!members_fit(batch, a_bs, nrows, stride, width)) return (int)hipErrorInvalidValue;
  if (batch > 0 && !rank) return (int)hipErrorInvalidValue;
  if (batch > 0 && nrows > 0 && ncols > 0 && !A) return (int)hipErrorInvalidValue;
  if (batch == 0) return 0;
  hipStream_t st = (hipStream_t)stream;
  if (nrows == 0 || ncols == 0) return (int)hipMemsetAsync(rank, 0, (size_t)batch * 4, st);  // min(nrows, ncols) = 0: no pivots
  const int mn   = (int)(nrows < ncols ? nrows : ncols);
  const int path = m4ri_amd_plan_echelonize_batch(nrows, ncols);
  if (path == 0)
    return launch_waves(batch, [&](dim3 grid, int64_t b0, int64_t) {
      hipLaunchKernelGGL(eb_wave_kernel, grid, dim3(BATCH_WAVE_THREADS), 0, st, A, stride, a_bs, (int)nrows, (int)ncols, b0, batch, full, rank, pivots, mn);
    });
  if (path == 3) return run_path3(A, stride, a_bs, nrows, ncols, batch, full, rank, pivots, st);
  const bool inlds   = path == 1;
  const int threads  = block_threads(nrows, width);
  const int ldw      = inlds ? (int)lds_row_words(width) : 0;
  const size_t lds   = inlds ? (size_t)lds_bytes_path1(nrows, width) : (size_t)(2 * ((nrows + 63) / 64) * 8);
  HIPTRY(set_max_dynamic_lds(BATCH_LDS_BUDGET, eb_block_kernel<true>, eb_block_kernel<false>));
  return launch_members(batch, [&](dim3 grid, int64_t b0) {
    if (inlds) hipLaunchKernelGGL(eb_block_kernel<true>, grid, dim3(threads), lds, st, A, stride, a_bs, (int)nrows, (int)ncols, ldw, b0, full, rank, pivots, mn);
    else hipLaunchKernelGGL(eb_block_kernel<false>, grid, dim3(threads), lds, st, A, stride, a_bs, (int)nrows, (int)ncols, ldw, b0, full, rank, pivots, mn);
  });
}

}  // extern "C"
