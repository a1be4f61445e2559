// isd_collide_search_batch.hip -- a whole Stern collision decoding search for many small codes, one launch for the batch: up to `iters`
// times "exchange `steps` pivots of the stored reduced echelon form, then join the sums of t1 of the first k1 pivot rows with the sums of
// t2 of the others (and the received word) on a window of ell non-information columns and weigh the colliding pairs", the lightest word
// seen kept with its key and its iteration, a member stopped as soon as that weight is low enough.
//
// The rule (include/m4ri_amd.h, m4ri_amd_isd_collide_search_dev) is a composition of two calls: iteration `it` > 0 first does what
// m4ri_amd_pivot_exchange_batch_dev(req = NULL, steps, seed = splitmix64(seed, it)) does on the member, every iteration then takes what
// m4ri_amd_row_sums_collide_batch_dev(rows 0 .. k-1, V = row k, k1, t1, t2, cols = order + k, ell, w_min) writes to `lightest`.  What
// this file adds is that the member stays in LDS between the two and from one iteration to the next, and that the row keys of the join
// are gathered from the staged rows: the two-call loop stages the member once per exchange call and reads the rows from global memory
// in every collision call.
//
// One kernel, a workgroup per member (m4ri_amd_plan_isd_collide_search: 1; everything else 2, not supported).  Its dynamic LDS is
// isd_search_batch.hip's path-1 staging (rows at an odd pitch, row index, flags, slots, a key per wave, the word of the best, the
// order), rounded up to 16 bytes, then join_common.h's carve behind k + 1 row keys without bins: the sorted keys, the bucket
// counts / starts / ends, the scan's partial sums, the window, the 16-bit left indices.  An iteration:
//   steps   isd_block_kernel's exchange step on a drawn request, `steps` times.
//   window  order[k .. k + ell - 1] of the STAGED order through join_window: an entry outside 0 .. ncols-1 gives key -2 for this
//           iteration (nothing is enumerated), checked again in every iteration because the exchanges move entries into the window.
//   keys    a thread per row gathers the row's window bits from the staged rows (the odd pitch puts the rows of a half-wave on
//           different banks), k + 1 keys with V's.
//   table   rc_kernel's: count with LDS atomics on q = join_bucket_bits(ell, N1) bits, join_starts, scatter.
//   walk    a lane per r2: key2 = V's key ^ the keys of S2, the full key compared with every entry of bucket key2 mod 2^q; a match is
//           weighed from the staged rows in WT register words; the lane keeps its minimum of (wt << 40) | (r1 * N2 + r2).
//   best    the minima go through shuffles and a slot per wave; every thread reads the same minimum and takes the same decisions (the
//           update of the best, the stop), so the barriers are reached uniformly.  Wave 0 makes the word of a new best in LDS.
// No histogram and no list: no bins, no slot counter, no global atomic.  The exchange step, the staging and the store-out are copies
// of isd_search_batch.hip's, not shared code: lifting them into a header both files include changed that file's device assembly
// (DESIGN 3.18), so it stays as it is.  join_window, join_starts, join_bucket_bits, JoinCarve and JoinLds are join_common.h's,
// unrank_step and binom_capped subset_rank.h's, splitmix64 gf2_common.h's.
#include <hip/hip_runtime.h>
#include <limits.h>
#include "join_common.h"
#include "subset_rank.h"
#include "../../include/m4ri_amd.h"

namespace {

constexpr int ICS_WAVES         = BATCH_MAX_THREADS / 64;  // slots per workgroup
constexpr int64_t ICS_N1_MAX    = 8192;                    // the left table of one workgroup, as in rowsums_collide_batch.hip
constexpr int64_t ICS_N2_MAX    = (int64_t)1 << 24;        // one workgroup walks its member's whole right list in every iteration
constexpr int64_t ICS_VOTES     = 256;                     // static LDS of the window's voting barrier, kept out of the dynamic budget
constexpr unsigned long long ICS_NONE = ~0ull;
constexpr unsigned long long ICS_RANK = ((unsigned long long)1 << 40) - 1;

struct IcsArgs {
  word *D;
  int64_t d_stride, d_bs;
  int nrows, ncols, k, pm, olen;
  int k1, k2, t1, t2, ell, q;
  int n1;        // N1 <= 8192; 0: no pairs
  int64_t n2;    // N2 <= 2^24; 0: no pairs
  int has_v;     // nrows > k: row k is the received word
  int exchange;  // steps > 0, iters > 1 and pm > 0: pivots and rank are there
  int w_min;     // at most ncols + 1
  int64_t iters, steps, w_stop;
  uint64_t seed;
  int32_t *pivots;
  const int32_t *rank;
  int32_t *order;  // nullptr: none kept (then ell = 0)
  int64_t o_bs;
  int64_t *best;
  int32_t *best_iter, *iters_run, *done;  // or nullptr
  word *W;                                // or nullptr
  int64_t w_bs;
  int64_t join_at;  // bytes from the start of the dynamic LDS to the row keys
};

__device__ __forceinline__ int ics_rank(const IcsArgs &p, int64_t b) {
  if (!p.exchange) return 0;
  const int R = p.rank[b];
  return R < 0 ? 0 : R > p.pm ? p.pm : R;
}

__device__ __forceinline__ unsigned long long wave_min(unsigned long long key) {
  for (int o = 32; o; o >>= 1) {
    const unsigned long long x = __shfl_xor(key, o);
    key                        = x < key ? x : key;
  }
  return key;
}

__device__ __forceinline__ bool ics_lighter(unsigned long long key, long long best) {
  return key != ICS_NONE && (best < 0 || (key >> 40) < ((unsigned long long)best >> 40));
}

// isd_cyclic_scan of isd_search_batch.hip: the first column, in the cyclic order start, start + 1, ..., ncols - 1, 0, ..., start - 1,
// at which the row has a bit, the bit of column `own` not counted; -1 if there is none.  The whole wave, lane l the words l, l + 64, ...
__device__ __forceinline__ int ics_cyclic_scan(const word *row, int width, int own, int start, int lane) {
  const int sw = start >> 6, sb = start & 63;
  int at_lo = -1;
  word w_lo = 0;
  for (int base = 0; base < width; base += 64) {
    const int w = base + lane;
    word x      = 0;
    if (w < width) {
      x = row[w];  // staged: the tail bits are clear
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

// the key of the set of rank `rest` among the sets of t of the rows base .. base + kk - 1 (rc_kernel's set_key)
__device__ __forceinline__ word ics_set_key(const word *rowkey, unsigned long long rest, int t, int kk, int base) {
  word key = 0;
  int e    = kk;
  for (int m = t; m >= 1; --m) {
    e = unrank_step(rest, m, e);
    key ^= rowkey[base + e];
  }
  return key;
}

// c ^= the staged rows of that set
template <int WT>
__device__ __forceinline__ void ics_add_set_rows(word (&c)[WT], const word *rows, int ldw, int width, unsigned long long rest, int t, int kk, int base) {
  int e = kk;
  for (int m = t; m >= 1; --m) {
    e             = unrank_step(rest, m, e);
    const word *r = rows + (base + e) * ldw;
#pragma unroll
    for (int w = 0; w < WT; ++w)
      if (w < width) c[w] ^= r[w];
  }
}

// The dynamic LDS (16-byte carve offsets):
//   rows [nrows][ldw] words | index [nrows] int32 (rounded up to 16 B) | flags [nfw] words | slots [2][16] int32 | keys [16] words |
//   wbuf [width] words | order [olen] int32 | (to 16 B; p.join_at) rowkey [k + 1] words | JoinCarve(rows = N1, no bins)
// WT: the power of two >= the width, the register words of a weighed word.
template <int WT>
__global__ __launch_bounds__(BATCH_MAX_THREADS) void ics_kernel(IcsArgs p, int ldw, int64_t b0) {
  extern __shared__ __attribute__((aligned(16))) char ics_smem[];
  const int T = blockDim.x, t = threadIdx.x, lane = t & 63, wave = t >> 6, nwaves = T >> 6;
  const int64_t b = b0 + blockIdx.x;
  const int R     = ics_rank(p, b);
  word *d         = p.D + b * p.d_bs;
  const int nrows = p.nrows, k = p.k;
  const int width = (p.ncols + 63) >> 6;
  const int nfw   = (nrows + 63) >> 6;
  const word mask = tail_mask(p.ncols);
  word *rows      = reinterpret_cast<word *>(ics_smem);
  int32_t *index  = reinterpret_cast<int32_t *>(ics_smem + (size_t)nrows * ldw * 8);
  word *flags     = reinterpret_cast<word *>(ics_smem + (size_t)nrows * ldw * 8 + pad16((size_t)nrows * 4));
  int32_t *slots  = reinterpret_cast<int32_t *>(flags + nfw);
  word *keys      = reinterpret_cast<word *>(slots + 2 * ICS_WAVES);
  word *wbuf      = keys + ICS_WAVES;
  int32_t *ord    = reinterpret_cast<int32_t *>(wbuf + width);
  word *rowkey    = reinterpret_cast<word *>(ics_smem + p.join_at);
  const JoinLds L(rowkey, JoinCarve((size_t)(k + 1) * 8, p.n1, -1, p.q, false));  // n = -1: no bins
  int32_t *og = p.order ? p.order + b * p.o_bs : nullptr;  // staged whenever it is there: the window is read from it
  int32_t *pv = p.pivots + b * p.pm;                       // read and written only with R > 0
  stage_rows_in(rows, ldw, d, p.d_stride, nrows, width, mask, t, T);
  for (int i = t; i < nrows; i += T) index[i] = i;
  if (og)
    for (int j = t; j < p.olen; j += T) ord[j] = og[j];
  __syncthreads();
  const word *vrow = p.has_v ? rows + k * ldw : nullptr;

  const bool own_word = T % width == 0;
  const int w_own     = t % width;
  const bool pairs    = p.n1 > 0 && p.n2 > 0;
  const int n1 = p.n1, nb = 1 << p.q;
  const word qmask = (word)nb - 1;
  PendingSwap none;  // flag_pass's, unused: no row moves
  int cnt = 0, best_it = -1;
  long long best = -1;
  int64_t run    = p.iters;
  for (int64_t it = 0; it < p.iters; ++it) {
    if (it > 0) {
      if (R == 0) break;  // uniform: no exchange ever, every further iteration is this one again
      const int before       = cnt;
      const uint64_t seed_it = splitmix64(p.seed, (uint64_t)it);
      for (int64_t s = 0; s < p.steps; ++s) {  // isd_block_kernel's step on a drawn request
        const uint64_t h = splitmix64(seed_it, (uint64_t)b * (uint64_t)p.steps + (uint64_t)s);
        const int r      = (int)((uint32_t)(h >> 32) % (uint32_t)R);
        const int old    = pv[r];
        const word *prow = rows + r * ldw;
        const int c      = ics_cyclic_scan(prow, width, old, (int)((uint32_t)h % (uint32_t)p.ncols), lane);
        if (c < 0 || c >= p.ncols) continue;  // uniform over the workgroup, as all that follows; bit (r, c) is set and c != old by the scan
        const int cw = c >> 6, cb = c & 63;
        flag_pass<false>(flags, rows, ldw, nullptr, none, nrows, cw, cb, t, T);
        if (og) {  // each wave its positions, ascending: the first ballot with a hit holds the wave's first position
          int at_old = -1, at_new = -1;
          for (int base = t - lane; base < p.olen && (at_old < 0 || at_new < 0); base += T) {
            const int j = base + lane;
            const int e = j < p.olen ? ord[j] : 0;
            const word h_old = __ballot(j < p.olen && e == old), h_new = __ballot(j < p.olen && e == c);
            if (at_old < 0 && h_old) at_old = base + (int)__builtin_ctzll(h_old);
            if (at_new < 0 && h_new) at_new = base + (int)__builtin_ctzll(h_new);
          }
          if (lane == 0) slots[wave] = at_old, slots[ICS_WAVES + wave] = at_new;
        }
        __syncthreads();
        if (t == 0) {  // everyone read pivots[r] and its order entries before the barrier; the next reads come after the update's
          pv[r] = c;
          if (og) {
            int at_old = p.olen, at_new = p.olen;
            for (int w = 0; w < nwaves; ++w) {
              const int x = slots[w], y = slots[ICS_WAVES + w];
              if (x >= 0 && x < at_old) at_old = x;
              if (y >= 0 && y < at_new) at_new = y;
            }
            if (at_old < p.olen && at_new < p.olen) ord[at_old] = c, ord[at_new] = old;
          }
        }
        if (own_word) {  // a thread keeps its word w_own of every row it visits: the pivot row's is read once per step
          const word x = prow[w_own];
          for (int i = t / width; i < nrows; i += T / width)
            if (flag_of(flags, i) && i != r) rows[i * ldw + w_own] ^= x;
        } else {
          for_each_item(0, nrows, 0, width, t, T, [&](int i, int w) {
            if (flag_of(flags, i) && i != r) rows[i * ldw + w] ^= prow[w];
          });
        }
        ++cnt;
        __syncthreads();
      }
      if (cnt == before) continue;  // the form and the order of the iteration before: the same key, not lighter than the best
    }

    // the join on the window order[k .. k + ell - 1] as it stands now; without pairs, or with an entry outside, the key is negative
    unsigned long long key = ICS_NONE;
    if (pairs && !join_window(L.cols, ord, k, p.ell, p.ncols, t)) {  // uniform: join_window votes over the workgroup
      // 1. the keys of the rows and of V, from the staged rows
      for (int i = t; i <= k; i += T) {
        const word *r = i < k ? rows + i * ldw : vrow;
        word rk       = 0;
        if (r)
          for (int j = 0; j < p.ell; ++j) {
            const int c = L.cols[j];
            rk |= ((r[c >> 6] >> (c & 63)) & 1) << j;
          }
        rowkey[i] = rk;
      }
      for (int i = t; i < nb; i += T) L.off[i] = 0;
      __syncthreads();
      // 2. the left table: count, scan, scatter; the keys are made twice, as in rc_kernel
      for (int r1 = t; r1 < n1; r1 += T) atomicAdd(&L.off[(uint32_t)(ics_set_key(rowkey, (unsigned long long)r1, p.t1, p.k1, 0) & qmask)], 1u);
      join_starts(L, nb, t, T);
      for (int r1 = t; r1 < n1; r1 += T) {
        const word lk      = ics_set_key(rowkey, (unsigned long long)r1, p.t1, p.k1, 0);
        const uint32_t pos = atomicAdd(&L.off[(uint32_t)(lk & qmask)], 1u);  // pos < n1: the counts sum to n1
        L.skey[pos]        = lk;
        L.sidx[pos]        = (uint16_t)r1;
      }
      __syncthreads();  // off[i] is now the END of bucket i, the start of bucket i + 1
      // 3. the right walk
      const word vkey = rowkey[k];
      for (int64_t r2 = t; r2 < p.n2; r2 += T) {
        const word key2      = vkey ^ ics_set_key(rowkey, (unsigned long long)r2, p.t2, p.k2, p.k1);
        const uint32_t bkt   = (uint32_t)(key2 & qmask);
        const uint32_t e_end = L.off[bkt];
        for (uint32_t e = bkt ? L.off[bkt - 1] : 0; e < e_end; ++e) {
          if (L.skey[e] != key2) continue;
          const uint32_t r1 = L.sidx[e];
          word c[WT];
#pragma unroll
          for (int w = 0; w < WT; ++w) c[w] = vrow && w < width ? vrow[w] : 0;
          ics_add_set_rows<WT>(c, rows, ldw, width, (unsigned long long)r1, p.t1, p.k1, 0);
          ics_add_set_rows<WT>(c, rows, ldw, width, (unsigned long long)r2, p.t2, p.k2, p.k1);
          int wt = 0;
#pragma unroll
          for (int w = 0; w < WT; ++w) wt += __popcll(c[w]);
          if (wt >= p.w_min) {
            const unsigned long long cand = ((unsigned long long)(uint32_t)wt << 40) | ((unsigned long long)r1 * (unsigned long long)p.n2 + (unsigned long long)r2);
            key                           = cand < key ? cand : key;
          }
        }
      }
    }
    // 4. the workgroup's minimum, the same in every thread
    key = wave_min(key);
    if (lane == 0) keys[wave] = key;
    __syncthreads();
    key = ICS_NONE;
    for (int w = 0; w < nwaves; ++w) key = keys[w] < key ? keys[w] : key;
    if (ics_lighter(key, best)) {
      best = (long long)key, best_it = (int)it;
      if (p.W && wave == 0) {  // lane l keeps the words l, l + 64, ... through all t1 + t2 rows
        const unsigned long long pr = key & ICS_RANK, r1 = pr / (unsigned long long)p.n2;
        unsigned long long rest     = r1;
        for (int w = lane; w < width; w += 64) wbuf[w] = vrow ? vrow[w] : 0;
        int e = p.k1;
        for (int m = p.t1; m >= 1; --m) {
          e = unrank_step(rest, m, e);
          for (int w = lane; w < width; w += 64) wbuf[w] ^= rows[e * ldw + w];
        }
        rest = pr - r1 * (unsigned long long)p.n2;
        e    = p.k2;
        for (int m = p.t2; m >= 1; --m) {
          e = unrank_step(rest, m, e);
          for (int w = lane; w < width; w += 64) wbuf[w] ^= rows[(p.k1 + e) * ldw + w];
        }
      }
    }
    __syncthreads();  // the keys are read and the word is made: the next iteration may write the rows, the slots and the table
    if (best >= 0 && p.w_stop >= 0 && (best >> 40) <= p.w_stop) {
      run = it + 1;
      break;
    }
  }

  if (cnt) {
    store_rows_out(d, p.d_stride, rows, ldw, index, nrows, width, mask, t, T);
    if (og)
      for (int j = t; j < p.olen; j += T) og[j] = ord[j];
  }
  if (p.W && best >= 0)
    for (int w = t; w < width; w += T) store_masked(p.W + b * p.w_bs + w, wbuf[w], w == width - 1, mask);
  if (t == 0) {
    p.best[b] = best;
    if (p.best_iter) p.best_iter[b] = best_it;
    if (p.iters_run) p.iters_run[b] = (int32_t)run;
    if (p.done) p.done[b] = cnt;
  }
}

// Members without columns (every word weighs 0, no exchange is possible, ell = 0: every pair collides) and calls of no iteration: key =
// what every iteration gives, iters_run = the count for every member; with no iteration only best and iters_run are written.
__global__ __launch_bounds__(BATCH_WAVE_THREADS) void ics_const_kernel(IcsArgs p, long long key, int32_t run, int64_t batch) {
  const int64_t step = (int64_t)gridDim.x * BATCH_WAVE_THREADS;
  for (int64_t b = (int64_t)blockIdx.x * BATCH_WAVE_THREADS + threadIdx.x; b < batch; b += step) {
    p.best[b] = key;
    if (p.iters_run) p.iters_run[b] = run;
    if (p.iters > 0) {
      if (p.best_iter) p.best_iter[b] = key >= 0 ? 0 : -1;
      if (p.done) p.done[b] = 0;
    }
  }
}

bool sizes_negative(int64_t nrows, int64_t ncols, int64_t k, int64_t k1, int64_t t1, int64_t t2, int64_t ell) {
  return nrows < 0 || ncols < 0 || k < 0 || k1 < 0 || k1 > k || t1 < 0 || t2 < 0 || ell < 0;
}

// beyond what one workgroup holds or walks; the sizes are not negative
bool beyond_limits(int64_t ncols, int64_t k, int64_t k1, int64_t t1, int64_t t2, int64_t ell) {
  if (k > RS_K_MAX || ncols > RS_N_MAX || t1 > RS_T_MAX || t2 > RS_T_MAX || ell > JOIN_ELL_MAX) return true;
  const int64_t n1 = binom_capped(k1, t1), n2 = binom_capped(k - k1, t2);  // each at most 2^41
  return n1 > ICS_N1_MAX || n2 > ICS_N2_MAX || (wide)n1 * (wide)n2 > (wide)RS_SUMS_MAX;
}

// the staging of isd_search_batch.hip's path 1 behind the flags: the slots, the keys and the word
int64_t staged_extra(int64_t width) { return 8 * ICS_WAVES + 8 * ICS_WAVES + 8 * width; }

// where the row keys start, for an order of `olen` entries, and what the join takes from there
int64_t join_at(int64_t nrows, int64_t width, int64_t olen) { return (int64_t)pad16((size_t)(lds_bytes_staged(nrows, width, 1, staged_extra(width)) + 4 * olen)); }
int64_t join_bytes(int64_t k, int64_t n1, int q) { return (int64_t)JoinCarve((size_t)(k + 1) * 8, (int)n1, -1, q, false).total; }

int plan(int64_t nrows, int64_t ncols, int64_t k, int64_t k1, int64_t t1, int64_t t2, int64_t ell) {
  if (sizes_negative(nrows, ncols, k, k1, t1, t2, ell)) return -1;
  if (beyond_limits(ncols, k, k1, t1, t2, ell)) return 2;
  const int64_t width = width_of(ncols), cap = BATCH_CAP_BYTES / 8;
  if (nrows > cap || nrows * width > cap) return 2;  // far beyond LDS; keeps the sums below in 64 bits
  const int64_t n1 = binom_capped(k1, t1);
  // the order counted at its longest, ncols entries, as in plan_on_order; the votes of the window's barrier are static LDS
  const int64_t need = join_at(nrows, width, ncols) + join_bytes(k, n1, join_bucket_bits(ell, n1)) + ICS_VOTES;
  return need <= BATCH_LDS_BUDGET ? 1 : 2;
}

// The workgroup: a wave per 256 entries of the longer of the two lists and per 512 words of the member, at most BATCH_MAX_THREADS.  Small
// members are one wave, which meets no other at its barriers and leaves the compute unit's wave slots to other members.  Measured
// (DESIGN 3.18, 16 iterations, one step): at 32 x 64 and 64 x 128 with 16 and 32 sums a side one wave runs in 1.30 and 2.05 ms, 256
// threads in 5.1 and 5.7 ms, 1024 in 37.5 and 40.9 ms; at 64 x 128 with 496 a side 128 and 256 threads run in 20.0 and 19.8 ms, one wave
// in 30.3 ms, 512 threads in 25.7 ms, 1024 in 72.7 ms; at 256 x 512 with 8128 a side 1024 threads run in 41.6 ms, 512 in 70.9 ms.
// M4RI_AMD_ISD_COLLIDE_SEARCH_THREADS (a multiple of 64 in [64, 1024]) replaces the rule, read per call: the benchmark measures with it.
int threads_of(int64_t nrows, int64_t width, int64_t n1, int64_t n2) {
  int64_t waves = (n1 + 255) / 256;
  if ((n2 + 255) / 256 > waves) waves = (n2 + 255) / 256;
  if ((nrows * width + 511) / 512 > waves) waves = (nrows * width + 511) / 512;
  waves = waves < 1 ? 1 : waves > ICS_WAVES ? ICS_WAVES : waves;
  return (int)env_bound("M4RI_AMD_ISD_COLLIDE_SEARCH_THREADS", 64 * waves, 64, BATCH_MAX_THREADS, 64);
}

template <int WT>
void launch_block(const IcsArgs &p, dim3 grid, int threads, size_t lds, hipStream_t st, int ldw, int64_t b0) {
  hipLaunchKernelGGL(ics_kernel<WT>, grid, dim3(threads), lds, st, p, ldw, b0);
}

}  // namespace

extern "C" {

int m4ri_amd_plan_isd_collide_search(int64_t nrows, int64_t ncols, int64_t pivot_rows, int64_t k1, int64_t t1, int64_t t2, int64_t ell) {
  return plan(nrows, ncols, pivot_rows, k1, t1, t2, ell);
}

int m4ri_amd_isd_collide_search_dev(word *D, int64_t d_stride, int64_t d_bs, int64_t nrows, int64_t ncols, int64_t pivot_rows, int32_t *pivots,
                                    const int32_t *rank, int64_t batch, int64_t iters, int64_t steps, uint64_t seed, int64_t k1, int64_t t1, int64_t t2,
                                    int64_t ell, int64_t w_min, int64_t w_stop, int32_t *order, int64_t o_bs, int64_t olen, int64_t *best,
                                    int32_t *best_iter, int32_t *iters_run, int32_t *done, word *W, int64_t w_bs, void *stream) {
  if (sizes_negative(nrows, ncols, pivot_rows, k1, t1, t2, ell) || olen < 0 || batch < 0 || iters < 0 || steps < 0 || w_min < 0 || d_stride < 0 || d_bs < 0 ||
      o_bs < 0 || w_bs < 0)
    return (int)hipErrorInvalidValue;
  if (pivot_rows > nrows || olen > ncols) return (int)hipErrorInvalidValue;
  if (ell > 0 && (!order || (wide)olen < (wide)pivot_rows + (wide)ell)) return (int)hipErrorInvalidValue;  // the window is order[k .. k + ell - 1]
  const int64_t width = width_of(ncols);
  if (d_stride < width) return (int)hipErrorInvalidValue;
  if (plan(nrows, ncols, pivot_rows, k1, t1, t2, ell) != 1) return (int)hipErrorNotSupported;
  // best_iter, iters_run and done are 32-bit counts
  if (iters > INT32_MAX || (iters > 1 && (wide)(iters - 1) * (wide)steps > (wide)INT32_MAX)) return (int)hipErrorNotSupported;
  const bool data = nrows > 0 && ncols > 0;
  if (data && !members_fit(batch, d_bs, nrows, d_stride, width)) return (int)hipErrorInvalidValue;
  if (batch > 1 && order && o_bs < olen) return (int)hipErrorInvalidValue;
  if (batch > 1 && W && w_bs < width) return (int)hipErrorInvalidValue;
  const int64_t pm = pivot_rows < ncols ? pivot_rows : ncols;
  if (batch > 0) {
    if (!best) return (int)hipErrorInvalidValue;
    if (data && iters > 0 && !D) return (int)hipErrorInvalidValue;
    if (data && steps > 0 && iters > 1 && (!pivots || !rank)) return (int)hipErrorInvalidValue;
    // every operand against every other
    if (spans_meet_any({rows_span(D, batch, d_bs, nrows, d_stride, width), entries_span(pivots, batch, pm, pm, 4), entries_span(rank, batch, 1, 1, 4),
                        entries_span(order, batch, o_bs, olen, 4), entries_span(best, batch, 1, 1, 8), entries_span(best_iter, batch, 1, 1, 4),
                        entries_span(iters_run, batch, 1, 1, 4), entries_span(done, batch, 1, 1, 4), rows_span(W, batch, w_bs, 1, 0, width)}))
      return (int)hipErrorInvalidValue;
  }
  if (batch == 0) return 0;
  hipStream_t st = (hipStream_t)stream;
  const int64_t n1 = binom_capped(k1, t1), n2 = binom_capped(pivot_rows - k1, t2);
  IcsArgs p{};
  p.D = D, p.d_stride = d_stride, p.d_bs = d_bs;
  p.nrows = (int)nrows, p.ncols = (int)ncols, p.k = (int)pivot_rows, p.pm = (int)pm, p.olen = (int)olen;
  p.k1 = (int)k1, p.k2 = (int)(pivot_rows - k1), p.t1 = (int)t1, p.t2 = (int)t2, p.ell = (int)ell, p.n1 = (int)n1, p.n2 = n2;
  p.q     = join_bucket_bits(ell, n1);
  p.has_v = nrows > pivot_rows, p.exchange = steps > 0 && iters > 1 && pm > 0;
  p.w_min = join_w_min(w_min, ncols);
  p.iters = iters, p.steps = steps, p.w_stop = w_stop, p.seed = seed;
  p.pivots = pivots, p.rank = rank, p.order = olen > 0 ? order : nullptr, p.o_bs = o_bs;
  p.best = best, p.best_iter = best_iter, p.iters_run = iters_run, p.done = done, p.W = W, p.w_bs = w_bs;
  if (iters == 0 || ncols == 0) {
    // no columns: the window is empty (olen <= ncols), every pair collides and weighs 0, rank 0 is the lightest if weight 0 qualifies
    const long long key = iters > 0 && n1 > 0 && n2 > 0 && w_min == 0 ? 0 : -1;
    const int32_t run   = key >= 0 && w_stop >= 0 ? 1 : (int32_t)iters;
    int64_t grid        = (batch + BATCH_WAVE_THREADS - 1) / BATCH_WAVE_THREADS;
    if (grid > 4096) grid = 4096;
    hipLaunchKernelGGL(ics_const_kernel, dim3((unsigned)grid), dim3(BATCH_WAVE_THREADS), 0, st, p, key, run, batch);
    HIPTRY(hipGetLastError());
    return 0;
  }
  HIPTRY(set_max_dynamic_lds(BATCH_LDS_BUDGET - ICS_VOTES, ics_kernel<1>, ics_kernel<2>, ics_kernel<4>, ics_kernel<8>, ics_kernel<16>));
  p.join_at         = join_at(nrows, width, p.order ? olen : 0);
  const int threads = threads_of(nrows, width, n1, n2);
  const int ldw     = (int)lds_row_words(width);
  const size_t lds  = (size_t)(p.join_at + join_bytes(pivot_rows, n1, p.q));
  return launch_members(batch, [&](dim3 grid, int64_t b0) {
    if (width <= 1) launch_block<1>(p, grid, threads, lds, st, ldw, b0);
    else if (width <= 2) launch_block<2>(p, grid, threads, lds, st, ldw, b0);
    else if (width <= 4) launch_block<4>(p, grid, threads, lds, st, ldw, b0);
    else if (width <= 8) launch_block<8>(p, grid, threads, lds, st, ldw, b0);
    else launch_block<16>(p, grid, threads, lds, st, ldw, b0);
  });
}

}  // extern "C"
