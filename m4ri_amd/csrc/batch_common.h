// batch_common.h -- what the batched calls (the *_batch.hip files, join_common.h) share: the launch constants, the device pieces of the
// workgroup-per-member elimination (one column at a time: flag pass, pivot search, row swap, update) and the host side of a call: its
// argument checks (widths, environment bounds, member fit, spans) and its launches.  Everything here is internal to the file
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
#include <cstdlib>
#include <initializer_list>
#include <mutex>
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

// words(ncols) for any ncols >= 0, INT64_MAX included (words_of adds 63 first)
inline int64_t width_of(int64_t ncols) { return ncols / 64 + (ncols % 64 != 0); }

// LDS bytes of a member staged with its row index and `flag_bufs` flag buffers, `extra` bytes behind them
inline int64_t lds_bytes_staged(int64_t nrows, int64_t width, int flag_bufs, int64_t extra) {
  return nrows * lds_row_words(width) * 8 + (int64_t)pad16((size_t)nrows * 4) + flag_bufs * ((nrows + 63) / 64) * 8 + extra;
}

// The paths of the calls that walk a member's columns on an order given per member (echelon_order_batch.hip, pivot_exchange_batch.hip).
// p0: the largest side of path 0; p1: the LDS bytes path 1 may use for lds_bytes_staged and the order, counted at its longest, ncols
// entries; in_place: path 2 although the member fits.
inline int plan_on_order(int64_t nrows, int64_t ncols, int64_t p0, int64_t p1, int flag_bufs, int64_t extra, bool in_place = false) {
  if (nrows < 0 || ncols < 0) return -1;
  if (nrows <= p0 && ncols <= p0) return 0;
  const int64_t width = width_of(ncols), cap = BATCH_CAP_BYTES / 8;
  if (nrows > cap || width > cap || nrows * width > cap) return 3;
  if (in_place) return 2;
  return lds_bytes_staged(nrows, width, flag_bufs, extra) + 4 * ncols <= p1 ? 1 : 2;
}

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

// ---- the host side of a batched call -----------------------------------------------------------------------------------
// Every size, stride and pointer below comes from a caller: nothing here overflows on the way to its answer, which is the one the
// comparison has over the integers.

using wide = unsigned __int128;

// An environment bound of a call, read per call: `dflt` unless the variable is set; rounded down to a multiple, then clamped to [lo, hi].
inline int64_t env_bound(const char *name, int64_t dflt, int64_t lo, int64_t hi, int64_t multiple_of = 1) {
  const char *s = getenv(name);
  if (!s || !*s) return dflt;
  const int64_t v = strtoll(s, nullptr, 10) / multiple_of * multiple_of;
  return v < lo ? lo : v > hi ? hi : v;
}

// May `batch` members of `rows` rows, `stride` words apart and `width` words wide, lie bs words apart?  (No sign is negative.)
inline bool members_fit(int64_t batch, int64_t bs, int64_t rows, int64_t stride, int64_t width) {
  return !(batch > 1 && rows > 0 && (wide)bs < (wide)(rows - 1) * (wide)stride + (wide)width);
}

// The bytes [lo, hi) of an operand, from its first member's start to its last member's end; lo == hi: absent, empty or not read.
// A count beyond the address space is held at 2^64 entries: such a span ends behind every pointer either way.
struct Span {
  wide lo, hi;
};

inline Span span_of(const void *p, wide first, wide count, int size) {
  const wide all = (wide)1 << 64, lo = (wide)(uintptr_t)p + first * (wide)size;
  return Span{lo, lo + (count < all ? count : all) * (wide)size};
}

// rows of `width` words (nothing where there are none), from word `first_word` of M on
inline Span rows_span(const word *M, int64_t batch, int64_t bs, int64_t rows, int64_t stride, int64_t width, int64_t first_word = 0) {
  if (!M || batch <= 0 || rows <= 0 || width <= 0) return Span{0, 0};
  return span_of(M, (wide)first_word, (wide)(batch - 1) * (wide)bs + (wide)(rows - 1) * (wide)stride + (wide)width, 8);
}

// `count` entries of `size` bytes per member, bs entries apart
inline Span entries_span(const void *p, int64_t batch, int64_t bs, wide count, int size) {
  if (!p || batch <= 0 || count == 0) return Span{0, 0};
  return span_of(p, 0, (wide)(batch - 1) * (wide)bs + count, size);
}

inline bool spans_meet(Span a, Span b) { return a.lo < a.hi && b.lo < b.hi && a.lo < b.hi && b.lo < a.hi; }

// does one of the outputs meet another, or an operand?
inline bool spans_meet_any(std::initializer_list<Span> outs, std::initializer_list<Span> operands = {}) {
  for (const Span *o = outs.begin(); o != outs.end(); ++o) {
    for (const Span *o2 = o + 1; o2 != outs.end(); ++o2)
      if (spans_meet(*o, *o2)) return true;
    for (const Span &in : operands)
      if (spans_meet(*o, in)) return true;
  }
  return false;
}

// The most dynamic LDS a kernel may be launched with is an attribute of the kernel.  It is set on the given kernels (a NULL among them
// is passed over) by the first call through each instantiation and the result kept: once per process for a call site, as long as no
// other site of the file passes kernels of the same types -- Site tells such sites apart.
template <int Site = 0, typename... Kernels>
hipError_t set_max_dynamic_lds(size_t bytes, Kernels... kernels) {
  static std::once_flag once;
  static hipError_t attr = hipSuccess;
  std::call_once(once, [&] {
    for (const void *k : {reinterpret_cast<const void *>(kernels)...})
      if (k && attr == hipSuccess) attr = hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
  });
  return attr;
}

// the workgroup-per-member kernels: fn(grid, b0) launches members b0 .. b0 + grid.x - 1
template <typename Fn>
int launch_members(int64_t batch, Fn fn) {
  return launch_chunked(batch, BATCH_CHUNK, [&](int64_t b0, int64_t nb) { fn(dim3((unsigned)nb), b0); });
}

// the wave kernels, four members per workgroup: fn(grid, b0, nb) launches members b0 .. b0 + nb - 1
template <typename Fn>
int launch_waves(int64_t batch, Fn fn) {
  const int64_t per = BATCH_WAVE_THREADS / 64;
  return launch_chunked(batch, BATCH_CHUNK * per, [&](int64_t b0, int64_t nb) { fn(dim3((unsigned)((nb + per - 1) / per)), b0, nb); });
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
  const int64_t w = width_of(k);
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
