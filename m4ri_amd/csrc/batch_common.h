// batch_common.h -- what the batched small-matrix calls share (echelon_batch.hip, solve_batch.hip, ple_batch.hip and the launch side
// of mul_small_batch.hip): the launch constants, the device pieces of the workgroup-per-member elimination (one column at a time:
// flag pass, pivot search, row swap, update) and the host scaffolding around the launches.  Everything here is internal to the file
// that includes it (an unnamed namespace, as in those files); the kernels stay in their files, and so do the bodies of the wave
// kernels, which carry a different payload per lane.
//
// The workgroup-per-member scheme.  A member's rows live either in LDS (INLDS) under a row-permutation index `perm`, logical row i
// at rows[perm[i] * ldw], or in place in global memory.  Per column c: the flag pass makes flags[c & 1] (bit i = bit c of logical
// row i), a barrier, every thread finds the same pivot row p in the flag words, row p goes up to the rank's row (INLDS: as a pending
// swap of two index entries, which their owner threads apply in the next column's flag pass; in global memory: physically, and a
// barrier), the update adds the pivot row into the flagged rows, a barrier.  Two barriers per column with a pivot in LDS, three in
// global memory; a column without a pivot writes nothing, and the next flag pass uses the other flag buffer.
#pragma once
#include <hip/hip_runtime.h>
#include <vector>
#include "dev_scratch.h"  // Scratch: the device temporaries of a one-by-one path
#include "gf2_internal.h"

namespace {

constexpr int BATCH_WAVE_THREADS   = 256;                 // the wave kernels: four waves, four members (or blocks of C) per workgroup
constexpr int BATCH_MAX_THREADS    = 1024;                // the workgroup-per-member kernels
constexpr int64_t BATCH_LDS_BUDGET = 160 * 1024;          // a member staged in LDS: the whole LDS of a CU
constexpr int64_t BATCH_CAP_BYTES  = 512 * 1024;          // a member eliminated in place in global memory: its valid words, bytes
constexpr int64_t BATCH_CHUNK      = (int64_t)1 << 30;    // workgroups per launch

// ---- device helpers -----------------------------------------------------------------------------------------------------------------

// lane `lane`'s 64-bit x (wave-uniform lane)
__device__ __forceinline__ word readlane64(word x, int lane) {
  const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)x, lane);
  const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(x >> 32), lane);
  return ((word)hi << 32) | lo;
}

__device__ __forceinline__ word bpermute64(word x, int src) {  // lane `src`'s x; every lane of the wave must take part
  const uint32_t lo = (uint32_t)__builtin_amdgcn_ds_bpermute(src << 2, (int)(uint32_t)x);
  const uint32_t hi = (uint32_t)__builtin_amdgcn_ds_bpermute(src << 2, (int)(uint32_t)(x >> 32));
  return ((word)hi << 32) | lo;
}

// the valid bits of a row's last word (of ncols only ncols mod 64 counts: the host passes that of its 64-bit counts)
__host__ __device__ __forceinline__ word tail_mask(int ncols) { return (ncols & 63) ? (((word)1 << (ncols & 63)) - 1) : ~(word)0; }

// the 16-byte rounding of the dynamic-LDS carve offsets
__host__ __device__ __forceinline__ size_t pad16(size_t bytes) { return (bytes + 15) & ~(size_t)15; }

// *dst = x; in a row's last word only under the mask, the bits behind it stay what they are
__device__ __forceinline__ void store_masked(word *dst, word x, bool is_last_word, word mask) {
  if (is_last_word && mask != ~(word)0) x = (x & mask) | (*dst & ~mask);
  *dst = x;
}

// INLDS: a column's swap of perm[rank] and perm[p], pending until the next column's flag pass.  Row i of the flag pass is owned by
// thread i % blockDim.x (the lane of its ballot), and between the barrier after a flag pass and the barrier after the update every
// thread may read any perm[i]; so nobody writes perm there.  The swap is recorded in registers by every thread instead (all find
// the same pivot), and in the next flag pass -- after the update's barrier -- the owner of row sw_r and the owner of row sw_p
// each write their own entry, the only threads that read those two entries in that pass.  record() after the pivot search, applied
// and cleared by flag_pass (written out there: as a member function returning the row it made the compiler lay the LDS kernels'
// column loop out differently, and the batched inverse at 256 x 256 2 % slower), finish() after the last column.
struct PendingSwap {
  int sw_r = -1, sw_p = -1, sw_R = 0, sw_P = 0;  // logical rows sw_r (the rank's) and sw_p (the pivot's); their new entries are sw_P, sw_R

  // after the pivot search: logical row p (physical row P) goes to the rank's row.  Reads perm[rank]: before the update, like perm[p].
  __device__ __forceinline__ void record(const int32_t *perm, int rank, int p, int P) {
    if (p != rank) {
      sw_r = rank; sw_p = p; sw_P = P; sw_R = perm[rank];
    }
  }
  // after the last column: its swap (its owners only, as in the flag pass).  The caller's barrier follows.
  __device__ __forceinline__ void finish(int32_t *perm, int nrows, int t, int T) const {
    if (sw_r >= 0) {
      for (int i = t; i < nrows; i += T)
        if (i == sw_r) perm[i] = sw_P;
        else if (i == sw_p) perm[i] = sw_R;
    }
  }
};

// The flag pass of column 64 * cw + cb into buf: each thread its own rows (and, INLDS, their index entries, where it applies the
// pending swap), a ballot per 64 rows.  INLDS says where the rows live: in LDS under perm (row_words = ldw, an int), or in place in
// global memory (row_words = the stride, an int64_t; perm and sw unused).  The caller's barrier follows.
template <bool INLDS, typename Stride>
__device__ __forceinline__ void flag_pass(word *buf, const word *rows, Stride row_words, int32_t *perm, PendingSwap &sw, int nrows, int cw,
                                          int cb, int t, int T) {
  const int lane = t & 63;
  for (int base = t - lane; base < nrows; base += T) {
    const int i = base + lane;
    int bit     = 0;
    if (i < nrows) {
      int ph = i;
      if (INLDS) {  // the physical row of logical row i; the pending swap written to perm[i] if row i is one of its two (by its owner)
        ph = (i == sw.sw_r) ? sw.sw_P : (i == sw.sw_p) ? sw.sw_R : perm[i];
        if (i == sw.sw_r || i == sw.sw_p) perm[i] = ph;
      }
      bit = (int)((rows[ph * row_words + cw] >> cb) & 1);
    }
    const word bal = __ballot(bit);
    if (lane == 0) buf[base >> 6] = bal;
  }
  sw.sw_r = sw.sw_p = -1;
}

// bit i of the flag words
__device__ __forceinline__ int flag_of(const word *buf, int i) { return (int)((buf[i >> 6] >> (i & 63)) & 1); }

// the first flagged row at or below the rank in nfw flag words, -1 if there is none
__device__ __forceinline__ int find_pivot(const word *buf, int rank, int nfw) {
  for (int j = rank >> 6; j < nfw; ++j) {
    word f = buf[j];
    if (j == (rank >> 6)) f &= ~(word)0 << (rank & 63);
    if (f) return j * 64 + (int)__builtin_ctzll(f);
  }
  return -1;
}

// The items (i, w) of an update, rows first_row .. nrows-1 by words cw .. width-1: item k = (i - first_row) * nw + (w - cw) with
// nw = width - cw goes to thread k % T, k = t, t + T, ..., advanced by (qi, qw) without a division per item.
template <typename Body>
__device__ __forceinline__ void for_each_item(int first_row, int nrows, int cw, int width, int t, int T, Body body) {
  const int nw = width - cw;
  const int qi = T / nw, qw = T - qi * nw;
  int i = first_row + t / nw, w = cw + (t - (t / nw) * nw);
  while (i < nrows) {
    body(i, w);
    i += qi;
    w += qw;
    if (w >= width) {
      w -= nw;
      ++i;
    }
  }
}

// the physical swap of two rows in global memory from word w0 on, the bits behind the mask of the last word stay where they are.
// The caller's barrier follows.
__device__ __forceinline__ void swap_rows_global(word *rp, word *pp, int w0, int width, word mask, int t, int T) {
  for (int w = w0 + t; w < width; w += T) {
    const word x = rp[w], y = pp[w];
    if (w == width - 1) {
      rp[w] = (y & mask) | (x & ~mask);
      pp[w] = (x & mask) | (y & ~mask);
    } else {
      rp[w] = y;
      pp[w] = x;
    }
  }
}

// nrows rows of `width` words from g (stride words apart) into LDS rows of ldw words, the last word under the mask
__device__ __forceinline__ void stage_rows_in(word *rows, int ldw, const word *g, int64_t stride, int nrows, int width, word mask, int t, int T) {
  const int total = nrows * width;
  for (int k = t; k < total; k += T) {
    const int i = k / width, w = k - i * width;
    word x = g[(int64_t)i * stride + w];
    if (w == width - 1) x &= mask;
    rows[i * ldw + w] = x;
  }
}

// and back: logical row i = LDS row perm[i], the last word merged with what is behind the mask (`rows` may point into the rows,
// at a word offset)
__device__ __forceinline__ void store_rows_out(word *g, int64_t stride, const word *rows, int ldw, const int32_t *perm, int nrows, int width,
                                               word mask, int t, int T) {
  const int total = nrows * width;
  for (int k = t; k < total; k += T) {
    const int i = k / width, w = k - i * width;
    store_masked(g + (int64_t)i * stride + w, rows[perm[i] * ldw + w], w == width - 1, mask);
  }
}

// ---- host helpers -------------------------------------------------------------------------------------------------------------------

inline int64_t lds_row_words(int64_t width) { return width + ((width & 1) ^ 1); }  // odd: the flag pass reads one word per row

inline int block_threads(int64_t rows, int64_t width) { return rows * width >= 8192 ? BATCH_MAX_THREADS : 256; }

// fn(b0, cnt) launches members b0 .. b0 + cnt - 1, at most members_per_launch of them (what BATCH_CHUNK workgroups hold); the
// launch error is checked after each
template <typename Fn>
int launch_chunked(int64_t batch, int64_t members_per_launch, Fn fn) {
  for (int64_t b0 = 0; b0 < batch; b0 += members_per_launch) {
    fn(b0, batch - b0 < members_per_launch ? batch - b0 : members_per_launch);
    HIPTRY(hipGetLastError());
  }
  return 0;
}

// bytes from the first member's start to the last member's end (batch, rows > 0)
inline uintptr_t member_span_bytes(int64_t batch, int64_t bs, int64_t rows, int64_t stride, int64_t width) {
  return (uintptr_t)(((batch - 1) * bs + (rows - 1) * stride + width) * 8);
}

// do [p, p + pn) and [q, q + qn) (bytes) meet?
inline bool spans_meet(const void *p, uintptr_t pn, const void *q, uintptr_t qn) {
  return (uintptr_t)p < (uintptr_t)q + qn && (uintptr_t)q < (uintptr_t)p + pn;
}

// a clean copy (tail bits zero) of the rows x ncols matrix at src into scratch
inline int clean_copy(word *dst, int64_t dst_stride, const word *src, int64_t src_stride, int64_t rows, int64_t ncols, hipStream_t st) {
  HIPTRY(hipMemsetAsync(dst, 0, (size_t)(rows * dst_stride) * 8, st));
  HIPTRY(gf2_launch_copy_masked(st, dst, dst_stride, src, src_stride, rows, ncols));
  return 0;
}

// are rows r0 .. r1-1 of the k-column matrix at M (stride words) all zero?  Copies them to the host.  Blocking.
inline int rows_zero(const word *M, int64_t stride, int64_t r0, int64_t r1, int64_t k, hipStream_t st, bool *zero) {
  *zero = true;
  const int64_t w = words_of(k);
  if (r1 <= r0 || w == 0) return 0;
  std::vector<word> h((size_t)((r1 - r0) * w));
  HIPTRY(hipMemcpy2DAsync(h.data(), (size_t)w * 8, M + r0 * stride, (size_t)stride * 8, (size_t)w * 8, (size_t)(r1 - r0), hipMemcpyDeviceToHost, st));
  HIPTRY(hipStreamSynchronize(st));
  const word mask = tail_mask((int)(k & 63));
  for (int64_t i = 0; i < r1 - r0; ++i)
    for (int64_t j = 0; j < w; ++j)
      if (h[(size_t)(i * w + j)] & (j == w - 1 ? mask : ~(word)0)) {
        *zero = false;
        return 0;
      }
  return 0;
}

}  // namespace
