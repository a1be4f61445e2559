// pivot_exchange_batch.hip -- pivot exchanges on the stored reduced echelon forms of many small matrices, one launch for the batch: the
// step from one information set to the next in information-set decoding (Canteaut-Chabaud, Bernstein-Lange-Peters), which costs one
// pivot step on a form that is already reduced instead of an elimination from scratch.
//
// The rule (include/m4ri_amd.h, m4ri_amd_pivot_exchange_batch_dev): the state is what m4ri_amd_echelonize_order_batch_dev(full = 1)
// left -- D_b, its pivots and its rank.  A step takes a request (r, c), given by the caller or drawn on the device from the splitmix64
// stream; the device decides whether it is valid (r a pivot row, c a column, bit (r, c) set, c not row r's own pivot) and skips it
// otherwise; a performed step adds row r into every other row with bit c set, followers included, makes c the pivot of row r and
// swaps the old and the new pivot column in the caller's order.  The pivot row is chosen by the caller and stays where it is: no row
// swap, no row index.  The paths (m4ri_amd_plan_pivot_exchange_batch) are echelon_order_batch.hip's, from batch_common.h's pieces:
//   0  nrows, ncols <= 64: a wave per member, lane i holds row i and pivots[i], lane j holds order[j]; no LDS, no barrier.
//   1  the member, its flags and its order fit in LDS, more than one step: a workgroup per member, staged once for all steps; two
//      barriers per performed step (after the flag pass, after the update), none for a skipped one.
//   2  larger members up to BATCH_CAP_BYTES, a single step on any member beyond path 0 (and whatever the environment sends here): a
//      workgroup per member, in place in D_b.
//   3  above the cap: not supported.
// Every decision of a step is taken by all threads of the workgroup from the same values (the request, rank, pivots[r], bit (r, c)
// are read by everyone between two barriers that no write to them crosses), so the barriers are reached uniformly.  Nothing is indexed
// by a request before it has passed the checks; entries of the order are only compared.
#include <hip/hip_runtime.h>
#include <cstdlib>
#include "batch_common.h"
#include "../../include/m4ri_amd.h"

namespace {

constexpr int PX_WAVES = BATCH_MAX_THREADS / 64;  // one slot per wave of a workgroup
// Path 2 instead of path 1 for members that fit in LDS when 0 < steps <= this: a step in place touches the rows with the bit, staging
// reads and writes the whole member.  Measured at steps = 1, 4 and 16: in place wins at 1 and loses at 4 on every
// shape; 2 and 3 were not measured and stay staged.
constexpr int64_t PX_INPLACE_MAX_STEPS = 1;

struct PxArgs {
  word *D;
  int64_t d_stride, d_bs;
  int nrows, ncols, pm, olen;
  int64_t steps;
  int32_t *pivots;
  const int32_t *rank;
  const int32_t *req;  // nullptr: drawn from the stream seeded `seed`
  int64_t r_bs;
  uint64_t seed;
  int32_t *order;  // nullptr: none kept
  int64_t o_bs;
  int32_t *done;  // or nullptr
};

__device__ __forceinline__ int px_rank(const PxArgs &p, int64_t b) {
  const int R = p.rank[b];
  return R < 0 ? 0 : R > p.pm ? p.pm : R;
}

// path 0: a wave per member, lane i = row i (one word) and pivots[i], lane j = order[j].  Members b0 + 4 * blockIdx.x + wave.
__global__ __launch_bounds__(BATCH_WAVE_THREADS) void px_wave_kernel(PxArgs p, int64_t b0, int64_t batch) {
  const int lane  = threadIdx.x & 63;
  const int64_t b = b0 + (int64_t)blockIdx.x * (BATCH_WAVE_THREADS / 64) + (threadIdx.x >> 6);
  if (b >= batch) return;  // wave-uniform, no barrier in this kernel
  const int R = px_rank(p, b);
  int cnt     = 0;
  if (R > 0) {
    const word mask = tail_mask(p.ncols);
    word *d         = p.D + b * p.d_bs;
    word v          = 0;
    if (lane < p.nrows) v = d[(int64_t)lane * p.d_stride] & mask;
    int piv = -1, ord = 0;
    if (lane < p.pm) piv = p.pivots[b * p.pm + lane];
    if (p.order && lane < p.olen) ord = p.order[b * p.o_bs + lane];
    const int32_t *rq = p.req ? p.req + b * p.r_bs : nullptr;
    for (int64_t s = 0; s < p.steps; ++s) {
      int r, c;
      if (rq) {
        r = rq[2 * s], c = rq[2 * s + 1];
      } else {
        const uint64_t h = splitmix64(p.seed, (uint64_t)b * (uint64_t)p.steps + (uint64_t)s);
        r                = (int)((uint32_t)(h >> 32) % (uint32_t)R);
        const int start  = (int)((uint32_t)h % (uint32_t)p.ncols);
        word cand        = readlane64(v, r);
        const int own    = __builtin_amdgcn_readlane(piv, r);
        if (own >= 0 && own < 64) cand &= ~((word)1 << own);
        const word hi = cand & (~(word)0 << start);
        c             = hi ? (int)__builtin_ctzll(hi) : cand ? (int)__builtin_ctzll(cand) : -1;
      }
      if (r < 0 || r >= R || c < 0 || c >= p.ncols) continue;  // wave-uniform, as all that follows
      const word pw = readlane64(v, r);
      const int old = __builtin_amdgcn_readlane(piv, r);
      if (c == old || !((pw >> c) & 1)) continue;
      if (lane != r && ((v >> c) & 1)) v ^= pw;
      if (lane == r) piv = c;
      if (p.order) {
        const word at_old = __ballot(lane < p.olen && ord == old), at_new = __ballot(lane < p.olen && ord == c);
        if (at_old && at_new) {
          if (lane == (int)__builtin_ctzll(at_old)) ord = c;
          else if (lane == (int)__builtin_ctzll(at_new)) ord = old;
        }
      }
      ++cnt;
    }
    if (cnt) {
      if (lane < p.nrows) store_masked(d + (int64_t)lane * p.d_stride, v, true, mask);
      if (lane < R) p.pivots[b * p.pm + lane] = piv;
      if (p.order && lane < p.olen) p.order[b * p.o_bs + lane] = ord;
    }
  }
  if (lane == 0 && p.done) p.done[b] = cnt;
}

// The first column, in the cyclic order start, start + 1, ..., ncols - 1, 0, ..., start - 1, at which the row has a bit, the bit of
// column `own` not counted; -1 if there is none.  The whole wave, lane l the words l, l + 64, ...; every wave of a workgroup finds
// the same column for itself, which spares a barrier.
__device__ __forceinline__ int px_cyclic_scan(const word *row, int width, word mask, int own, int start, int lane) {
  const int sw = start >> 6, sb = start & 63;
  int at_lo = -1;
  word w_lo = 0;
  for (int base = 0; base < width; base += 64) {
    const int w = base + lane;
    word x      = 0;
    if (w < width) {
      x = row[w];
      if (w == width - 1) x &= mask;
      if (own >= 0 && w == (own >> 6)) x &= ~((word)1 << (own & 63));
    }
    const word from = ~(word)0 << sb;
    const word hi   = w > sw ? x : w == sw ? x & from : 0;   // at or behind start
    const word lo   = w < sw ? x : w == sw ? x & ~from : 0;  // before it: taken only when nothing is behind
    const word b_hi = __ballot(hi != 0);
    if (b_hi) {
      const int l = (int)__builtin_ctzll(b_hi);
      return (base + l) * 64 + (int)__builtin_ctzll(readlane64(hi, l));
    }
    const word b_lo = __ballot(lo != 0);
    if (at_lo < 0 && b_lo) {
      const int l = (int)__builtin_ctzll(b_lo);
      at_lo       = base + l;
      w_lo        = readlane64(lo, l);
    }
  }
  return at_lo < 0 ? -1 : at_lo * 64 + (int)__builtin_ctzll(w_lo);
}

// paths 1 (INLDS) and 2: a workgroup per member.  Dynamic LDS (16-byte carve offsets):
//   INLDS: rows [nrows][ldw] words | index [nrows] int32 (rounded up to 16 B) | flags [nfw] words | slots [2][16] int32 | order [olen] int32
//   else:  flags [nfw] words | slots [2][16] int32 (pivots and order stay in global memory)
// index: the identity, what store_rows_out takes (no row ever moves here).  slots[0][w], slots[1][w]: the first position at which
// wave w has seen the old and the new pivot column in the order, -1 for none.  One flag buffer: a performed step ends with a barrier.
template <bool INLDS>
__global__ __launch_bounds__(BATCH_MAX_THREADS) void px_block_kernel(PxArgs p, int ldw, int64_t b0) {
  extern __shared__ __attribute__((aligned(16))) char px_smem[];
  const int T = blockDim.x, t = threadIdx.x, lane = t & 63;
  const int64_t b = b0 + blockIdx.x;
  const int R     = px_rank(p, b);
  if (R == 0) {  // uniform: a refused or rank-zero member skips every step, nothing of it is read or written
    if (t == 0 && p.done) p.done[b] = 0;
    return;
  }
  word *d           = p.D + b * p.d_bs;
  const int nrows   = p.nrows;
  const int width   = (p.ncols + 63) >> 6;
  const int nfw     = (nrows + 63) >> 6;
  const word mask   = tail_mask(p.ncols);
  word *rows        = reinterpret_cast<word *>(px_smem);
  int32_t *index    = reinterpret_cast<int32_t *>(px_smem + (INLDS ? (size_t)nrows * ldw * 8 : 0));
  word *flags       = reinterpret_cast<word *>(px_smem + (INLDS ? (size_t)nrows * ldw * 8 + pad16((size_t)nrows * 4) : 0));
  int32_t *slots    = reinterpret_cast<int32_t *>(flags + nfw);
  int32_t *ord      = slots + 2 * PX_WAVES;
  int32_t *og       = p.order ? p.order + b * p.o_bs : nullptr;
  int32_t *pv       = p.pivots + b * p.pm;
  const int32_t *rq = p.req ? p.req + b * p.r_bs : nullptr;
  if (INLDS) {
    stage_rows_in(rows, ldw, d, p.d_stride, nrows, width, mask, t, T);
    for (int i = t; i < nrows; i += T) index[i] = i;
    if (og)
      for (int j = t; j < p.olen; j += T) ord[j] = og[j];
    __syncthreads();
  }
  int32_t *o = INLDS ? ord : og;  // where the order is searched and swapped
  auto row   = [&](int i) -> word * { return INLDS ? rows + i * ldw : d + (int64_t)i * p.d_stride; };

  // the width divides the workgroup (every power of two up to 1024 words does): item k = i * width + w of the update keeps its w
  const bool own_word = T % width == 0;
  const int w_own     = t % width;
  PendingSwap none;  // flag_pass's, unused: no row moves
  int cnt = 0;
  for (int64_t s = 0; s < p.steps; ++s) {
    int r, c;
    if (rq) {
      r = rq[2 * s], c = rq[2 * s + 1];
    } else {
      const uint64_t h = splitmix64(p.seed, (uint64_t)b * (uint64_t)p.steps + (uint64_t)s);
      r                = (int)((uint32_t)(h >> 32) % (uint32_t)R);
      c                = px_cyclic_scan(row(r), width, mask, pv[r], (int)((uint32_t)h % (uint32_t)p.ncols), lane);
    }
    if (r < 0 || r >= R || c < 0 || c >= p.ncols) continue;  // uniform over the workgroup, as all that follows
    const int old    = pv[r];
    const word *prow = row(r);
    const int cw = c >> 6, cb = c & 63;
    if (c == old || !((prow[cw] >> cb) & 1)) continue;
    if (INLDS) flag_pass<false>(flags, rows, ldw, nullptr, none, nrows, cw, cb, t, T);
    else flag_pass<false>(flags, d, p.d_stride, nullptr, none, nrows, cw, cb, t, T);
    if (o) {  // each wave its positions, ascending: the first ballot with a hit holds the wave's first position
      int at_old = -1, at_new = -1;
      for (int base = t - lane; base < p.olen && (at_old < 0 || at_new < 0); base += T) {
        const int j = base + lane;
        const int e = j < p.olen ? o[j] : 0;
        const word h_old = __ballot(j < p.olen && e == old), h_new = __ballot(j < p.olen && e == c);
        if (at_old < 0 && h_old) at_old = base + (int)__builtin_ctzll(h_old);
        if (at_new < 0 && h_new) at_new = base + (int)__builtin_ctzll(h_new);
      }
      if (lane == 0) slots[t >> 6] = at_old, slots[PX_WAVES + (t >> 6)] = at_new;
    }
    __syncthreads();
    if (t == 0) {  // everyone read pivots[r] and its order entries before the barrier; the next reads come after the update's
      pv[r] = c;
      if (o) {
        int at_old = p.olen, at_new = p.olen;
        for (int w = 0; w < T >> 6; ++w) {
          const int x = slots[w], y = slots[PX_WAVES + w];
          if (x >= 0 && x < at_old) at_old = x;
          if (y >= 0 && y < at_new) at_new = y;
        }
        if (at_old < p.olen && at_new < p.olen) o[at_old] = c, o[at_new] = old;
      }
    }
    // the update, all words of the row, every flagged row but r itself; row r is only read
    if (own_word) {  // a thread keeps its word w_own of every row it visits: the pivot row's is read once per step
      word x = prow[w_own];
      if (!INLDS && w_own == width - 1) x &= mask;
      for (int i = t / width; i < nrows; i += T / width)
        if (flag_of(flags, i) && i != r) row(i)[w_own] ^= x;
    } else {
      for_each_item(0, nrows, 0, width, t, T, [&](int i, int w) {
        if (flag_of(flags, i) && i != r) {
          word x = prow[w];
          if (!INLDS && w == width - 1) x &= mask;
          row(i)[w] ^= x;
        }
      });
    }
    ++cnt;
    __syncthreads();
  }

  if (INLDS && cnt) {
    store_rows_out(d, p.d_stride, rows, ldw, index, nrows, width, mask, t, T);
    if (og)
      for (int j = t; j < p.olen; j += T) og[j] = ord[j];
  }
  if (t == 0 && p.done) p.done[b] = cnt;
}

// path 1 stages one flag buffer and the slots; p0, p1: plan_on_order's; few: the step counts sent in place although the member fits
int plan(int64_t nrows, int64_t ncols, int64_t steps, int64_t p0, int64_t p1, int64_t few) {
  return steps < 0 ? -1 : plan_on_order(nrows, ncols, p0, p1, 1, 8 * PX_WAVES, steps > 0 && steps <= few);
}

}  // namespace

extern "C" {

int m4ri_amd_plan_pivot_exchange_batch(int64_t nrows, int64_t ncols, int64_t steps) {
  return plan(nrows, ncols, steps, 64, BATCH_LDS_BUDGET, PX_INPLACE_MAX_STEPS);
}

int m4ri_amd_pivot_exchange_batch_dev(word *D, int64_t d_stride, int64_t d_bs, int64_t nrows, int64_t ncols, int64_t pivot_rows, int32_t *pivots,
                                      const int32_t *rank, int64_t batch, const int32_t *req, int64_t r_bs, int64_t steps, uint64_t seed,
                                      int32_t *order, int64_t o_bs, int64_t olen, int32_t *done, void *stream) {
  if (nrows < 0 || ncols < 0 || pivot_rows < 0 || olen < 0 || batch < 0 || steps < 0 || d_stride < 0 || d_bs < 0 || r_bs < 0 || o_bs < 0)
    return (int)hipErrorInvalidValue;
  if (pivot_rows > nrows || olen > ncols) return (int)hipErrorInvalidValue;
  const int64_t width = width_of(ncols);
  if (d_stride < width) return (int)hipErrorInvalidValue;
  // the cap next: below it a member's word counts are small
  // a caller who sets the LDS bound has chosen between paths 1 and 2: the step count no longer does
  const char *p1_set = getenv("M4RI_AMD_PIVOT_EXCHANGE_PATH1_MAX");
  const int path     = plan(nrows, ncols, steps, env_bound("M4RI_AMD_PIVOT_EXCHANGE_PATH0_MAX", 64, 0, 64),
                            env_bound("M4RI_AMD_PIVOT_EXCHANGE_PATH1_MAX", BATCH_LDS_BUDGET, 0, BATCH_LDS_BUDGET), p1_set && *p1_set ? 0 : PX_INPLACE_MAX_STEPS);
  if (path == 3) return (int)hipErrorNotSupported;
  const bool data = nrows > 0 && ncols > 0;
  if (data && !members_fit(batch, d_bs, nrows, d_stride, width)) return (int)hipErrorInvalidValue;
  if (batch > 1 && req && r_bs != 0 && r_bs / 2 < steps) return (int)hipErrorInvalidValue;  // r_bs < 2 * steps, for any steps
  if (batch > 1 && order && o_bs < olen) return (int)hipErrorInvalidValue;
  const int64_t pm = pivot_rows < ncols ? pivot_rows : ncols;
  if (batch > 0) {
    if (data && steps > 0 && (!D || !pivots || !rank)) return (int)hipErrorInvalidValue;
    // every operand against every other
    if (spans_meet_any({rows_span(D, batch, d_bs, nrows, d_stride, width), entries_span(pivots, batch, pm, pm, 4), entries_span(rank, batch, 1, 1, 4),
                        entries_span(req, batch, r_bs, (wide)2 * steps, 4), entries_span(order, batch, o_bs, olen, 4), entries_span(done, batch, 1, 1, 4)}))
      return (int)hipErrorInvalidValue;
  }
  if (batch == 0) return 0;
  hipStream_t st = (hipStream_t)stream;
  if (steps == 0 || pm == 0)  // no step, or no pivot row: every step is skipped
    return done ? (int)hipMemsetAsync(done, 0, (size_t)batch * 4, st) : 0;
  PxArgs p{};
  p.D = D, p.d_stride = d_stride, p.d_bs = d_bs;
  p.nrows = (int)nrows, p.ncols = (int)ncols, p.pm = (int)pm, p.steps = steps;
  p.pivots = pivots, p.rank = rank, p.req = req, p.r_bs = r_bs, p.seed = seed;
  p.order = olen > 0 ? order : nullptr, p.o_bs = o_bs, p.olen = (int)olen, p.done = done;
  if (path == 0)
    return launch_waves(batch, [&](dim3 grid, int64_t b0, int64_t nb) {
      hipLaunchKernelGGL(px_wave_kernel, grid, dim3(BATCH_WAVE_THREADS), 0, st, p, b0, b0 + nb);
    });
  HIPTRY(set_max_dynamic_lds(BATCH_LDS_BUDGET, px_block_kernel<true>));
  const bool inlds  = path == 1;
  const int threads = block_threads(nrows, width);
  const int ldw     = inlds ? (int)lds_row_words(width) : 0;
  const size_t lds  = inlds ? (size_t)(lds_bytes_staged(nrows, width, 1, 8 * PX_WAVES) + (p.order ? 4 * olen : 0)) : (size_t)(((nrows + 63) / 64) * 8 + 8 * PX_WAVES);
  return launch_members(batch, [&](dim3 grid, int64_t b0) {
    if (inlds) hipLaunchKernelGGL(px_block_kernel<true>, grid, dim3(threads), lds, st, p, ldw, b0);
    else hipLaunchKernelGGL(px_block_kernel<false>, grid, dim3(threads), lds, st, p, ldw, b0);
  });
}

}  // extern "C"
