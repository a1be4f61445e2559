// echelon_order_batch.hip -- (reduced) row echelon forms of many small matrices on column orders given per member, one launch for the
// batch; and seeded random column orders made on the device.
//
// The rule (include/m4ri_amd.h, m4ri_amd_echelonize_order_batch_dev): the columns are visited in the order order[0 .. olen-1], none is
// ever moved; the pivot of a visited column is the first row at or above the rank and below pivot_rows with the bit set, it is swapped
// up to the rank's row and added into the rows below (full = 0) or into every other row with the bit (full = 1); the rows from
// pivot_rows on only follow.  Member b reads A_b and writes D_b (A may be shared, or D itself).  The paths
// (m4ri_amd_plan_echelonize_order_batch) are echelon_batch.hip's, built from batch_common.h's pieces:
//   0  nrows, ncols <= 64: a wave per member, lane i holds row i, lane j holds order[j]; no LDS, no barrier.
//   1  the member, its row index, flags and order fit in LDS: a workgroup per member, two barriers per column with a pivot.
//   2  larger members up to BATCH_CAP_BYTES: a workgroup per member, in place in D_b (the kernel copies the valid bits of A_b there
//      first when out of place), rows swapped physically; three barriers per column with a pivot.
//   3  above the cap: not supported.
// Where left to right was assumed, and is not here.  echelon_batch.hip's update and physical swap start at the pivot column's word:
// a left-to-right walk leaves zeros to the left of a pivot.  Under an arbitrary order a pivot row has bits on both sides, so both
// cover words 0 .. width-1 here.  And the pivot search offers rows below pivot_rows only, while the flags and the update take all rows.
// The order is range-checked by the whole wave or workgroup before the first write to global memory; a member with a bad entry gets
// rank -1, pivots -1, and its D_b is not written.
#include <hip/hip_runtime.h>
#include "batch_common.h"
#include "../../include/m4ri_amd.h"

namespace {

constexpr int EO_VOTES = BATCH_MAX_THREADS / 64;  // one per wave of a workgroup

struct EoArgs {
  word *D;
  const word *A;  // may be D (in place): no __restrict__ on either
  int64_t d_stride, d_bs, a_stride, a_bs;
  const int32_t *order;  // nullptr: the natural order
  int64_t o_bs;
  int olen, nrows, ncols, pivot_rows, pm, full;
  int32_t *rank, *pivots;
};

// a member with a bad order entry: rank -1, pivots -1 (threads t, t + T, ...)
__device__ __forceinline__ void refuse_member(const EoArgs &p, int64_t b, int t, int T) {
  if (p.pivots)
    for (int i = t; i < p.pm; i += T) p.pivots[b * p.pm + i] = -1;
  if (t == 0) p.rank[b] = -1;
}

// path 0: a wave per member, lane i = row i (one word), lane j = order[j].  Members b0 + 4 * blockIdx.x + wave.
__global__ __launch_bounds__(BATCH_WAVE_THREADS) void eo_wave_kernel(EoArgs p, int64_t b0, int64_t batch) {
  const int lane  = threadIdx.x & 63;
  const int64_t b = b0 + (int64_t)blockIdx.x * (BATCH_WAVE_THREADS / 64) + (threadIdx.x >> 6);
  if (b >= batch) return;  // wave-uniform, no barrier in this kernel
  int ord = lane;
  if (p.order && lane < p.olen) ord = p.order[b * p.o_bs + lane];
  if (__ballot(lane < p.olen && (ord < 0 || ord >= p.ncols))) {  // wave-uniform
    refuse_member(p, b, lane, 64);
    return;
  }
  const word mask = tail_mask(p.ncols);
  word v          = 0;
  if (lane < p.nrows) v = p.A[b * p.a_bs + (int64_t)lane * p.a_stride] & mask;
  const word offered = p.pivot_rows >= 64 ? ~(word)0 : ((word)1 << p.pivot_rows) - 1;  // the rows that may be pivots
  int rank = 0, piv = -1;
  for (int j = 0; j < p.olen && rank < p.pivot_rows; ++j) {
    const int c     = __builtin_amdgcn_readlane(ord, j);
    const int bit   = (int)((v >> c) & 1);
    const word cand = __ballot(bit) & (~(word)0 << rank) & offered;
    if (!cand) continue;
    const int pr  = (int)__builtin_ctzll(cand);
    const word pw = readlane64(v, pr);
    if (bit && lane != pr && (p.full || lane > rank)) v ^= pw;
    const word vr = readlane64(v, rank);  // row `rank` has no bit c unless it is the pivot: unchanged by the update
    if (lane == rank) {
      v   = pw;
      piv = c;
    } else if (lane == pr) {
      v = vr;
    }
    ++rank;
  }
  if (lane < p.nrows) store_masked(p.D + b * p.d_bs + (int64_t)lane * p.d_stride, v, true, mask);
  if (lane < p.pm && p.pivots) p.pivots[b * p.pm + lane] = piv;
  if (lane == 0) p.rank[b] = rank;
}

// the first flagged row in rank .. end-1, -1 if there is none (find_pivot with the rows from `end` on not offered)
__device__ __forceinline__ int find_pivot_below(const word *buf, int rank, int end) {
  for (int j = rank >> 6; j < (end + 63) >> 6; ++j) {
    word f = buf[j];
    if (j == (rank >> 6)) f &= ~(word)0 << (rank & 63);
    if (j == (end >> 6)) f &= ((word)1 << (end & 63)) - 1;  // the last word of a ragged end: end & 63 != 0 here
    if (f) return j * 64 + (int)__builtin_ctzll(f);
  }
  return -1;
}

// paths 1 (INLDS) and 2: a workgroup per member.  Dynamic LDS (16-byte carve offsets):
//   INLDS: rows [nrows][ldw] words | perm [nrows] int32 (rounded up to 16 B) | flags [2][nfw] words | vote [16] int32 | order [olen] int32
//   else:  flags [2][nfw] words | vote [16] int32 (the order is read from global memory, one wave-uniform load per visited column)
// vote[w]: has wave w seen a bad order entry?  (Written out: __syncthreads_or brings static LDS of its own, which a member that fills
// the whole budget has no room for.)
// flags[j & 1] of step j: bit i = bit order[j] of logical row i, all nrows rows.
template <bool INLDS>
__global__ __launch_bounds__(BATCH_MAX_THREADS) void eo_block_kernel(EoArgs p, int ldw, int64_t b0) {
  extern __shared__ __attribute__((aligned(16))) char eo_smem[];
  const int T = blockDim.x, t = threadIdx.x;
  const int64_t b   = b0 + blockIdx.x;
  const word *a     = p.A + b * p.a_bs;
  word *d           = p.D + b * p.d_bs;
  const int nrows   = p.nrows;
  const int width   = (p.ncols + 63) >> 6;
  const int nfw     = (nrows + 63) >> 6;
  const word mask   = tail_mask(p.ncols);
  word *rows        = reinterpret_cast<word *>(eo_smem);
  int32_t *perm     = reinterpret_cast<int32_t *>(eo_smem + (INLDS ? (size_t)nrows * ldw * 8 : 0));
  word *flags       = reinterpret_cast<word *>(eo_smem + (INLDS ? (size_t)nrows * ldw * 8 + pad16((size_t)nrows * 4) : 0));
  int32_t *vote     = reinterpret_cast<int32_t *>(flags + 2 * nfw);
  int32_t *ord      = vote + EO_VOTES;
  const int32_t *og = p.order ? p.order + b * p.o_bs : nullptr;

  // the range check of the whole order (and, INLDS, its staging) before the first write to global memory; a uniform exit
  int bad = 0;
  if (og)
    for (int j = t; j < p.olen; j += T) {
      const int c = og[j];
      if (INLDS) ord[j] = c;
      bad |= (c < 0) | (c >= p.ncols);
    }
  if (INLDS) {
    stage_rows_in(rows, ldw, a, p.a_stride, nrows, width, mask, t, T);
    for (int i = t; i < nrows; i += T) perm[i] = i;
  }
  const word wave_bad = __ballot(bad);
  if ((t & 63) == 0) vote[t >> 6] = wave_bad != 0;
  __syncthreads();
  bad = 0;
  for (int w = 0; w < T >> 6; ++w) bad |= vote[w];
  if (bad) {
    refuse_member(p, b, t, T);
    return;
  }
  if (!INLDS && d != a) {  // out of place: the valid bits of A_b into D_b, then in place there
    const int total = nrows * width;
    for (int k = t; k < total; k += T) {
      const int i = k / width, w = k - i * width;
      store_masked(d + (int64_t)i * p.d_stride + w, a[(int64_t)i * p.a_stride + w], w == width - 1, mask);
    }
    __syncthreads();
  }

  // the width divides the workgroup (every power of two up to 1024 words does): item k = i * width + w of the update keeps its w
  const bool own_word = T % width == 0;
  const int w_own     = t % width;
  int rank = 0;
  PendingSwap sw;  // INLDS: the previous pivot's pending swap of perm[rank] and perm[pr]
  for (int j = 0; j < p.olen && rank < p.pivot_rows; ++j) {
    const int c  = og ? (INLDS ? ord[j] : og[j]) : j;
    word *buf    = flags + (j & 1) * nfw;
    const int cw = c >> 6, cb = c & 63;
    if (INLDS) flag_pass<true>(buf, rows, ldw, perm, sw, nrows, cw, cb, t, T);
    else flag_pass<false>(buf, d, p.d_stride, perm, sw, nrows, cw, cb, t, T);
    __syncthreads();
    const int pr = find_pivot_below(buf, rank, p.pivot_rows);
    if (pr < 0) continue;  // no writes this step; the next flag pass uses the other buffer
    if (t == 0 && p.pivots) p.pivots[b * p.pm + rank] = c;
    const word *prow;
    if (INLDS) {
      const int P = perm[pr];
      prow        = rows + P * ldw;
      sw.record(perm, rank, pr, P);
    } else {
      if (pr != rank) {  // physical swap of the whole rows, the bits behind ncols stay where they are
        swap_rows_global(d + (int64_t)rank * p.d_stride, d + (int64_t)pr * p.d_stride, 0, width, mask, t, T);
        __syncthreads();
      }
      prow = d + (int64_t)rank * p.d_stride;
    }
    // the update, all words of the row: flagged rows i != pr (row `rank` is unflagged when pr != rank), below the rank only unless
    // full; the rows from pivot_rows on are below every rank.
    if (own_word) {  // a thread keeps its word w_own of every row it visits: the pivot row's is read once per pivot
      word x = prow[w_own];
      if (!INLDS && w_own == width - 1) x &= mask;
      for (int i = t / width; i < nrows; i += T / width)
        if (flag_of(buf, i) && i != pr && (p.full || i > rank)) {
          if (INLDS) rows[perm[i] * ldw + w_own] ^= x;
          else d[(int64_t)i * p.d_stride + w_own] ^= x;
        }
    } else {
      for_each_item(0, nrows, 0, width, t, T, [&](int i, int w) {
        if (flag_of(buf, i) && i != pr && (p.full || i > rank)) {
          word x = prow[w];
          if (INLDS) {
            rows[perm[i] * ldw + w] ^= x;
          } else {
            if (w == width - 1) x &= mask;
            d[(int64_t)i * p.d_stride + w] ^= x;
          }
        }
      });
    }
    ++rank;
    __syncthreads();
  }

  if (INLDS) {
    sw.finish(perm, nrows, t, T);
    __syncthreads();
    store_rows_out(d, p.d_stride, rows, ldw, perm, nrows, width, mask, t, T);
  }
  if (p.pivots)
    for (int i = rank + t; i < p.pm; i += T) p.pivots[b * p.pm + i] = -1;
  if (t == 0) p.rank[b] = rank;
}

// path 1 stages two flag buffers and the votes; p0, p1: plan_on_order's
int plan(int64_t nrows, int64_t ncols, int64_t p0, int64_t p1) { return plan_on_order(nrows, ncols, p0, p1, 2, 4 * EO_VOTES); }

// ---- random orders ------------------------------------------------------------------------------------------------------------------

constexpr int RO_MAX = 4096;  // keys of a member: 32 KiB of LDS

// A workgroup per member: key j = (splitmix64 output number b * n + j of the stream seeded `seed`, its low 12 bits replaced by j), keys
// from n on all ones; a bitonic sort of N = 2^e >= n keys ascending; order[i] = the low 12 bits of key i.
__global__ __launch_bounds__(BATCH_MAX_THREADS) void eo_random_orders_kernel(int32_t *__restrict__ order, int64_t o_bs, int n, int N, uint64_t seed,
                                                                             int64_t b0) {
  __shared__ uint64_t keys[RO_MAX];
  const int T = blockDim.x, t = threadIdx.x;
  const int64_t b = b0 + blockIdx.x;
  for (int j = t; j < N; j += T) {
    uint64_t z = ~(uint64_t)0;
    if (j < n) {
      z = splitmix64(seed, (uint64_t)b * (uint64_t)n + (uint64_t)j);
      z = (z & ~(uint64_t)4095) | (uint64_t)j;
    }
    keys[j] = z;
  }
  __syncthreads();
  for (int k = 2; k <= N; k <<= 1)
    for (int s = k >> 1; s > 0; s >>= 1) {
      for (int i = t; i < N / 2; i += T) {
        const int lo = ((i & ~(s - 1)) << 1) | (i & (s - 1)), hi = lo | s;
        const uint64_t x = keys[lo], y = keys[hi];
        if ((x > y) == ((lo & k) == 0)) {
          keys[lo] = y;
          keys[hi] = x;
        }
      }
      __syncthreads();
    }
  for (int i = t; i < n; i += T) order[b * o_bs + i] = (int32_t)(keys[i] & 4095);
}

}  // namespace

extern "C" {

int m4ri_amd_plan_echelonize_order_batch(int64_t nrows, int64_t ncols) { return plan(nrows, ncols, 64, BATCH_LDS_BUDGET); }

int m4ri_amd_echelonize_order_batch_dev(word *D, int64_t d_stride, int64_t d_bs, const word *A, int64_t a_stride, int64_t a_bs, int64_t nrows,
                                        int64_t ncols, int64_t pivot_rows, const int32_t *order, int64_t o_bs, int64_t olen, int64_t batch, int full,
                                        int32_t *rank, int32_t *pivots, void *stream) {
  if (nrows < 0 || ncols < 0 || pivot_rows < 0 || olen < 0 || batch < 0 || d_stride < 0 || d_bs < 0 || a_stride < 0 || a_bs < 0 || o_bs < 0)
    return (int)hipErrorInvalidValue;
  if (pivot_rows > nrows || olen > ncols) return (int)hipErrorInvalidValue;
  const int64_t width = width_of(ncols);
  if (d_stride < width || a_stride < width) return (int)hipErrorInvalidValue;
  // the cap next: below it a member's word counts are small
  const int path = plan(nrows, ncols, env_bound("M4RI_AMD_ECH_ORDER_PATH0_MAX", 64, 0, 64),
                        env_bound("M4RI_AMD_ECH_ORDER_PATH1_MAX", BATCH_LDS_BUDGET, 0, BATCH_LDS_BUDGET));
  if (path == 3) return (int)hipErrorNotSupported;
  const bool data = nrows > 0 && ncols > 0;
  if (data && !members_fit(batch, d_bs, nrows, d_stride, width)) return (int)hipErrorInvalidValue;
  const bool in_place = (const word *)D == A && d_stride == a_stride && d_bs == a_bs;
  if (in_place && a_bs == 0 && batch > 1) return (int)hipErrorInvalidValue;
  const int64_t pm = pivot_rows < ncols ? pivot_rows : ncols;
  if (batch > 0) {
    if (!rank) return (int)hipErrorInvalidValue;
    if (data && (!A || !D)) return (int)hipErrorInvalidValue;
    // D against A unless in place; D, rank and pivots against each other and the order.  rank and pivots are not held against A.
    const Span d = rows_span(D, batch, d_bs, nrows, d_stride, width);
    if (!in_place && spans_meet(d, rows_span(A, batch, a_bs, nrows, a_stride, width))) return (int)hipErrorInvalidValue;
    if (spans_meet_any({d, entries_span(rank, batch, 1, 1, 4), entries_span(pivots, batch, pm, pm, 4)}, {entries_span(order, batch, o_bs, olen, 4)}))
      return (int)hipErrorInvalidValue;
  }
  if (batch == 0) return 0;
  hipStream_t st = (hipStream_t)stream;
  if (ncols == 0) return (int)hipMemsetAsync(rank, 0, (size_t)batch * 4, st);  // no column to visit, no entry to be wrong, pm = 0
  EoArgs p{};
  p.D = D, p.A = A, p.d_stride = d_stride, p.d_bs = d_bs, p.a_stride = a_stride, p.a_bs = a_bs;
  p.order = olen > 0 ? order : nullptr, p.o_bs = o_bs, p.olen = (int)olen;
  p.nrows = (int)nrows, p.ncols = (int)ncols, p.pivot_rows = (int)pivot_rows, p.pm = (int)pm, p.full = full;
  p.rank = rank, p.pivots = pivots;
  if (path == 0)
    return launch_waves(batch, [&](dim3 grid, int64_t b0, int64_t nb) {
      hipLaunchKernelGGL(eo_wave_kernel, grid, dim3(BATCH_WAVE_THREADS), 0, st, p, b0, b0 + nb);
    });
  HIPTRY(set_max_dynamic_lds(BATCH_LDS_BUDGET, eo_block_kernel<true>, eo_block_kernel<false>));
  const bool inlds  = path == 1;
  const int threads = block_threads(nrows, width);
  const int ldw     = inlds ? (int)lds_row_words(width) : 0;
  const size_t lds  = inlds ? (size_t)(lds_bytes_staged(nrows, width, 2, 4 * EO_VOTES) + (p.order ? 4 * olen : 0)) : (size_t)(2 * ((nrows + 63) / 64) * 8 + 4 * EO_VOTES);
  return launch_members(batch, [&](dim3 grid, int64_t b0) {
    if (inlds) hipLaunchKernelGGL(eo_block_kernel<true>, grid, dim3(threads), lds, st, p, ldw, b0);
    else hipLaunchKernelGGL(eo_block_kernel<false>, grid, dim3(threads), lds, st, p, ldw, b0);
  });
}

int m4ri_amd_random_orders_batch_dev(int32_t *order, int64_t o_bs, int64_t n, int64_t batch, uint64_t seed, void *stream) {
  if (n < 0 || batch < 0 || o_bs < 0) return (int)hipErrorInvalidValue;
  if (n > RO_MAX) return (int)hipErrorNotSupported;
  if (batch > 1 && o_bs < n) return (int)hipErrorInvalidValue;
  if (batch > 0 && n > 0 && !order) return (int)hipErrorInvalidValue;
  if (batch == 0 || n == 0) return 0;
  int N = 2;
  while (N < n) N *= 2;
  const int threads = N / 2 < 64 ? 64 : N / 2 > BATCH_MAX_THREADS ? BATCH_MAX_THREADS : N / 2;
  hipStream_t st    = (hipStream_t)stream;
  return launch_members(batch, [&](dim3 grid, int64_t b0) {
    hipLaunchKernelGGL(eo_random_orders_kernel, grid, dim3(threads), 0, st, order, o_bs, (int)n, N, seed, b0);
  });
}

}  // extern "C"
