// isd_search_batch.hip -- a whole information-set decoding search for many small codes, one launch for the batch: up to `iters` times
// "exchange `steps` pivots of the stored reduced echelon form, then weigh every sum of t pivot rows against the received word", the
// lightest word seen kept with its key and its iteration, a member stopped as soon as that weight is low enough.  t = 0 is Prange,
// t >= 1 Lee-Brickell; without a follower row it is a search for light codewords.
//
// The rule (include/m4ri_amd.h, m4ri_amd_isd_search_dev) is a composition of two calls: iteration `it` > 0 first does what
// m4ri_amd_pivot_exchange_batch_dev(req = NULL, steps, seed = splitmix64(seed, it)) does on the member, every iteration then takes
// what m4ri_amd_row_sums_weights_batch_dev(rows 0 .. k-1, V = row k, t, w_min) writes to `lightest`.  What this file adds is that
// the member stays where it is between the two and from one iteration to the next: the two-call loop stages it twice per iteration
// in launches of their own.  The paths (m4ri_amd_plan_isd_search):
//   0  nrows, ncols <= 64: a wave per member, four members per workgroup, lane i holds row i in one word and pivots[i], lane j holds
//      order[j]; no LDS, no barrier.  The exchange is px_wave_kernel's step.  In the enumeration a lane owns an upper part
//      {i_1 < ... < i_{t-1}}, unranked with subset_rank.h, its prefix fetched from the other lanes by shuffles; the wave walks i_0
//      together, the row broadcast by readlane64; the lane keeps its minimum in 32 bits as rs_kernel does.
//   1  a workgroup per member, staged in LDS once for the whole loop in px_block_kernel<true>'s layout with a key slot per wave and
//      a word buffer for W behind the slots.  The exchange is that kernel's step.  The enumeration is rs_kernel's walk, the waves of
//      the workgroup taking chunks of 64 upper parts each (with few chunks: every chunk, and every nwaves-th row of its walk); the
//      rows are read where they lie (an odd row pitch; row i_0 is one broadcast read per word).  An improvement of the best is rare
//      (at most ncols + 1 per member): wave 0 unranks the key and XORs the rows into the word buffer.  The workgroup has a wave per
//      chunk and per 512 words of the member, at most block_threads(): a small member at t = 2 is a single wave.
//   2  everything else: not supported.  There is no path in place in global memory: this call exists for members that stay resident.
// The steps and the walk are copies of those of pivot_exchange_batch.hip and rowsums_batch.hip, not shared code (DESIGN 3.17 says
// why); unrank_step and binom_elem are subset_rank.h's, splitmix64 is gf2_common.h's.
// Every decision of the loop (a step's validity, whether an iteration enumerates, the update of the best, the stop) is taken by all
// threads of a workgroup from the same values, so the barriers of path 1 are reached uniformly.  An iteration whose steps were all
// skipped enumerates nothing: the form is the one of the iteration before, whose key was not lighter than the best.
#include <hip/hip_runtime.h>
#include <limits.h>
#include "batch_common.h"
#include "subset_rank.h"
#include "../../include/m4ri_amd.h"

namespace {

constexpr int ISD_WAVES        = BATCH_MAX_THREADS / 64;  // slots per workgroup
constexpr int64_t ISD_SUMS_MAX = (int64_t)1 << 24;        // one workgroup walks all sums of its member in every iteration
constexpr unsigned long long ISD_NONE = ~0ull;
constexpr unsigned long long ISD_RANK = ((unsigned long long)1 << 40) - 1;

struct IsdArgs {
  word *D;
  int64_t d_stride, d_bs;
  int nrows, ncols, k, pm, olen, t;
  int has_v;     // nrows > k: row k is the received word
  int exchange;  // steps > 0, iters > 1 and pm > 0: pivots and rank are there
  int w_min;     // at most ncols + 1
  int64_t iters, steps, w_stop;
  uint64_t seed;
  int64_t n_upper;  // C(k, t - 1) upper parts (t = 1: the k rows); only with k >= t >= 1
  int32_t *pivots;
  const int32_t *rank;
  int32_t *order;  // nullptr: none kept
  int64_t o_bs;
  int64_t *best;
  int32_t *best_iter, *iters_run, *done;  // or nullptr
  word *W;                                // or nullptr
  int64_t w_bs;
};

__device__ __forceinline__ int isd_rank(const IsdArgs &p, int64_t b) {
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

__device__ __forceinline__ bool isd_lighter(unsigned long long key, long long best) {
  return key != ISD_NONE && (best < 0 || (key >> 40) < ((unsigned long long)best >> 40));
}

__device__ __forceinline__ void isd_outputs(const IsdArgs &p, int64_t b, long long best, int best_it, int64_t run, int cnt) {
  p.best[b] = best;
  if (p.best_iter) p.best_iter[b] = best_it;
  if (p.iters_run) p.iters_run[b] = (int32_t)run;
  if (p.done) p.done[b] = cnt;
}

// path 0: a wave per member, lane i = row i (one word) and pivots[i], lane j = order[j].  Members b0 + 4 * blockIdx.x + wave.
__global__ __launch_bounds__(BATCH_WAVE_THREADS) void isd_wave_kernel(IsdArgs p, int64_t b0, int64_t batch) {
  const int lane  = threadIdx.x & 63;
  const int64_t b = b0 + (int64_t)blockIdx.x * (BATCH_WAVE_THREADS / 64) + (threadIdx.x >> 6);
  if (b >= batch) return;  // wave-uniform, no barrier in this kernel
  const int k = p.k, tt = p.t;
  const int R     = isd_rank(p, b);
  const word mask = tail_mask(p.ncols);
  word *d         = p.D + b * p.d_bs;
  word v          = 0;
  if (lane < p.nrows) v = d[(int64_t)lane * p.d_stride] & mask;
  int piv = -1, ord = 0;
  if (R > 0 && lane < p.pm) piv = p.pivots[b * p.pm + lane];
  if (R > 0 && p.order && lane < p.olen) ord = p.order[b * p.o_bs + lane];
  int cnt = 0, best_it = -1;
  long long best = -1;
  int64_t run    = p.iters;
  word bw        = 0;  // the word of the best
  for (int64_t it = 0; it < p.iters; ++it) {
    if (it > 0) {
      if (R == 0) break;  // no exchange ever: every further iteration is this one again
      const int before       = cnt;
      const uint64_t seed_it = splitmix64(p.seed, (uint64_t)it);
      for (int64_t s = 0; s < p.steps; ++s) {  // px_wave_kernel's step on a drawn request
        const uint64_t h = splitmix64(seed_it, (uint64_t)b * (uint64_t)p.steps + (uint64_t)s);
        const int r      = (int)((uint32_t)(h >> 32) % (uint32_t)R);
        const int start  = (int)((uint32_t)h % (uint32_t)p.ncols);
        const word pw    = readlane64(v, r);
        const int old    = __builtin_amdgcn_readlane(piv, r);
        word cand        = pw;
        if (old >= 0 && old < 64) cand &= ~((word)1 << old);
        const word hi = cand & (~(word)0 << start);
        const int c   = hi ? (int)__builtin_ctzll(hi) : cand ? (int)__builtin_ctzll(cand) : -1;
        if (c < 0 || c >= p.ncols) continue;  // wave-uniform, as all that follows; bit (r, c) is set and c != old by the scan
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
      if (cnt == before) continue;  // the form of the iteration before
    }
    const word vw          = p.has_v ? readlane64(v, k) : 0;
    unsigned long long key = ISD_NONE;
    if (k >= tt) {  // wave-uniform
      if (tt == 0) {
        const int wt = __popcll(vw);
        if (wt >= p.w_min) key = (unsigned long long)wt << 40;
      } else if (tt == 1) {  // a lane per row
        const int acc = __popcll(vw ^ v) - p.w_min;
        if (lane < k && acc >= 0) key = ((unsigned long long)(uint32_t)(acc + p.w_min) << 40) | (unsigned long long)lane;
      } else {
        const int64_t n_uc = (p.n_upper + 63) >> 6;
        for (int64_t uc = 0; uc < n_uc; ++uc) {
          unsigned long long rest = (unsigned long long)((uc << 6) | lane);
          const bool valid        = rest < (unsigned long long)p.n_upper;
          if (!valid) rest = 0;  // a set that exists: every lane takes part in the shuffles
          word c                  = vw;
          unsigned long long base = 0;
          int e                   = k;
          for (int m = tt - 1; m >= 1; --m) {
            e = unrank_step(rest, m, e);
            base += binom_elem(e, m + 1);
            c ^= bpermute64(v, e);
          }
          const int end = valid ? e : 0;  // i_0 < i_1
          int wave_end  = end;
          for (int o = 32; o; o >>= 1) {
            const int x = __shfl_xor(wave_end, o);
            wave_end    = x > wave_end ? x : wave_end;
          }
          uint32_t low = UINT32_MAX;
          for (int i0 = 0; i0 < wave_end; ++i0) {
            const int acc = __popcll(c ^ readlane64(v, i0)) - p.w_min;
            if (i0 < end) {
              const uint32_t cand = ((uint32_t)acc << 10) | (uint32_t)i0;  // a weight below w_min wraps to 2^31 or more
              low                 = cand < low ? cand : low;
            }
          }
          if (low < 0x80000000u) {
            const unsigned long long cand = ((unsigned long long)((low >> 10) + (uint32_t)p.w_min) << 40) | (base + (low & 1023u));
            key                           = cand < key ? cand : key;
          }
        }
      }
    }
    key = wave_min(key);
    if (isd_lighter(key, best)) {
      best = (long long)key, best_it = (int)it;
      unsigned long long rest = key & ISD_RANK;
      bw                      = vw;
      int e                   = k;
      for (int m = tt; m >= 1; --m) {
        e = unrank_step(rest, m, e);
        bw ^= readlane64(v, e);
      }
    }
    if (best >= 0 && p.w_stop >= 0 && (best >> 40) <= p.w_stop) {
      run = it + 1;
      break;
    }
  }
  if (cnt) {
    if (lane < p.nrows) store_masked(d + (int64_t)lane * p.d_stride, v, true, mask);
    if (lane < R) p.pivots[b * p.pm + lane] = piv;
    if (p.order && lane < p.olen) p.order[b * p.o_bs + lane] = ord;
  }
  if (lane == 0) {
    if (p.W && best >= 0) store_masked(p.W + b * p.w_bs, bw, true, mask);
    isd_outputs(p, b, best, best_it, run, cnt);
  }
}

// px_cyclic_scan of pivot_exchange_batch.hip: the first column, in the cyclic order start, start + 1, ..., ncols - 1, 0, ...,
// start - 1, at which the row has a bit, the bit of column `own` not counted; -1 if there is none.  The whole wave, lane l the words
// l, l + 64, ...; every wave of a workgroup finds the same column for itself.
__device__ __forceinline__ int isd_cyclic_scan(const word *row, int width, int own, int start, int lane) {
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

// path 1: a workgroup per member.  Dynamic LDS (16-byte carve offsets), px_block_kernel<true>'s with the keys and the word behind the slots:
//   rows [nrows][ldw] words | index [nrows] int32 (rounded up to 16 B) | flags [nfw] words | slots [2][16] int32 | keys [16] words |
//   wbuf [width] words | order [olen] int32
// keys[w]: wave w's lightest key of the iteration.  wbuf: the word of the best.  WT: the power of two >= the width, the register words
// of a lane's prefix.
template <int WT>
__global__ __launch_bounds__(BATCH_MAX_THREADS) void isd_block_kernel(IsdArgs p, int ldw, int64_t b0) {
  extern __shared__ __attribute__((aligned(16))) char isd_smem[];
  const int T = blockDim.x, t = threadIdx.x, lane = t & 63, wave = t >> 6, nwaves = T >> 6;
  const int64_t b = b0 + blockIdx.x;
  const int R     = isd_rank(p, b);
  word *d         = p.D + b * p.d_bs;
  const int nrows = p.nrows, k = p.k, tt = p.t;
  const int width = (p.ncols + 63) >> 6;
  const int nfw   = (nrows + 63) >> 6;
  const word mask = tail_mask(p.ncols);
  word *rows      = reinterpret_cast<word *>(isd_smem);
  int32_t *index  = reinterpret_cast<int32_t *>(isd_smem + (size_t)nrows * ldw * 8);
  word *flags     = reinterpret_cast<word *>(isd_smem + (size_t)nrows * ldw * 8 + pad16((size_t)nrows * 4));
  int32_t *slots  = reinterpret_cast<int32_t *>(flags + nfw);
  word *keys      = reinterpret_cast<word *>(slots + 2 * ISD_WAVES);
  word *wbuf      = keys + ISD_WAVES;
  int32_t *ord    = reinterpret_cast<int32_t *>(wbuf + width);
  int32_t *og     = R > 0 && p.order ? p.order + b * p.o_bs : nullptr;
  int32_t *pv     = p.pivots + b * p.pm;  // read and written only with R > 0
  stage_rows_in(rows, ldw, d, p.d_stride, nrows, width, mask, t, T);
  for (int i = t; i < nrows; i += T) index[i] = i;
  if (og)
    for (int j = t; j < p.olen; j += T) ord[j] = og[j];
  __syncthreads();
  const word *vrow = p.has_v ? rows + k * ldw : nullptr;

  constexpr int UNROLL = WT <= 2 ? 4 : WT <= 4 ? 2 : 1;  // steps of the walk in flight, as in rs_kernel
  const bool own_word  = T % width == 0;
  const int w_own     = t % width;
  PendingSwap none;  // flag_pass's, unused: no row moves
  int cnt = 0, best_it = -1;
  long long best = -1;
  int64_t run    = p.iters;
  for (int64_t it = 0; it < p.iters; ++it) {
    if (it > 0) {
      if (R == 0) break;  // uniform: no exchange ever, every further iteration is this one again
      const int before       = cnt;
      const uint64_t seed_it = splitmix64(p.seed, (uint64_t)it);
      for (int64_t s = 0; s < p.steps; ++s) {  // px_block_kernel<true>'s step on a drawn request
        const uint64_t h = splitmix64(seed_it, (uint64_t)b * (uint64_t)p.steps + (uint64_t)s);
        const int r      = (int)((uint32_t)(h >> 32) % (uint32_t)R);
        const int old    = pv[r];
        const word *prow = rows + r * ldw;
        const int c      = isd_cyclic_scan(prow, width, old, (int)((uint32_t)h % (uint32_t)p.ncols), lane);
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
          if (lane == 0) slots[wave] = at_old, slots[ISD_WAVES + wave] = at_new;
        }
        __syncthreads();
        if (t == 0) {  // everyone read pivots[r] and its order entries before the barrier; the next reads come after the update's
          pv[r] = c;
          if (og) {
            int at_old = p.olen, at_new = p.olen;
            for (int w = 0; w < nwaves; ++w) {
              const int x = slots[w], y = slots[ISD_WAVES + w];
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
      if (cnt == before) continue;  // the form of the iteration before
    }

    // the enumeration: rs_kernel's walk on the rows where they lie, wave w the chunks w, w + nwaves, ... of 64 upper parts
    unsigned long long key = ISD_NONE;
    if (k >= tt) {  // uniform
      if (tt == 0) {  // every wave weighs the word for itself
        int wt = 0;
        if (vrow)
          for (int w = lane; w < width; w += 64) wt += __popcll(vrow[w]);
        for (int o = 32; o; o >>= 1) wt += __shfl_xor(wt, o);
        if (wt >= p.w_min) key = (unsigned long long)wt << 40;
      } else {
        const int tu = tt == 1 ? 1 : tt - 1, boff = tt == 1 ? 0 : 1;
        const int negw     = -p.w_min;
        const int64_t n_uc = (p.n_upper + 63) >> 6;
        // Many chunks: a wave takes whole chunks.  Few (t = 2: the chunks are consecutive i_1, the last walks k rows and the first
        // 63): every wave takes every chunk and the rows i_0 = wave, wave + nwaves, ... of its walk, which keeps the waves level.
        const int split = tt == 1 || n_uc >= 4 * nwaves ? 1 : nwaves;
        for (int64_t u = wave; u < n_uc * split; u += nwaves) {
          const int64_t uc = u / split;
          const int phase  = (int)(u - uc * split);
          unsigned long long rest = (unsigned long long)((uc << 6) | lane);
          const bool valid        = rest < (unsigned long long)p.n_upper;
          word c[WT];
#pragma unroll
          for (int w = 0; w < WT; ++w) c[w] = vrow && w < width ? vrow[w] : 0;
          unsigned long long base = 0;
          int e                   = k;  // the element above the one looked for; after the loop i_1 (t = 1: the row)
          if (valid) {
            for (int m = tu; m >= 1; --m) {
              e = unrank_step(rest, m, e);
              base += binom_elem(e, m + boff);
              const word *r = rows + e * ldw;
#pragma unroll
              for (int w = 0; w < WT; ++w)
                if (w < width) c[w] ^= r[w];
            }
          }
          if (tt == 1) {
            if (valid) {
              int acc = negw;
#pragma unroll
              for (int w = 0; w < WT; ++w) acc += __popcll(c[w]);
              if (acc >= 0) {
                const unsigned long long cand = ((unsigned long long)(uint32_t)(acc + p.w_min) << 40) | base;
                key                           = cand < key ? cand : key;
              }
            }
            continue;
          }
          const int end = valid ? e : 0;  // i_0 < i_1
          int wave_end  = end;
          for (int o = 32; o; o >>= 1) {
            const int x = __shfl_xor(wave_end, o);
            wave_end    = x > wave_end ? x : wave_end;
          }
          uint32_t low = UINT32_MAX;
#pragma unroll UNROLL
          for (int i0 = phase; i0 < wave_end; i0 += split) {
            const word *r = rows + i0 * ldw;
            int acc       = negw;
#pragma unroll
            for (int w = 0; w < WT; ++w)
              if (w < width) acc += __popcll(c[w] ^ r[w]);
            if (i0 < end) {
              const uint32_t cand = ((uint32_t)acc << 10) | (uint32_t)i0;  // a weight below w_min wraps to 2^31 or more
              low                 = cand < low ? cand : low;
            }
          }
          if (low < 0x80000000u) {
            const unsigned long long cand = ((unsigned long long)((low >> 10) + (uint32_t)p.w_min) << 40) | (base + (low & 1023u));
            key                           = cand < key ? cand : key;
          }
        }
      }
    }
    key = wave_min(key);
    if (lane == 0) keys[wave] = key;
    __syncthreads();
    key = ISD_NONE;
    for (int w = 0; w < nwaves; ++w) key = keys[w] < key ? keys[w] : key;  // the same in every thread
    if (isd_lighter(key, best)) {
      best = (long long)key, best_it = (int)it;
      if (p.W && wave == 0) {  // lane l keeps the words l, l + 64, ... through all t rows
        unsigned long long rest = key & ISD_RANK;
        for (int w = lane; w < width; w += 64) wbuf[w] = vrow ? vrow[w] : 0;
        int e = k;
        for (int m = tt; m >= 1; --m) {
          e = unrank_step(rest, m, e);
          for (int w = lane; w < width; w += 64) wbuf[w] ^= rows[e * ldw + w];
        }
      }
    }
    __syncthreads();  // the keys are read and the word is made: the next iteration may write the rows and the slots
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
  if (t == 0) isd_outputs(p, b, best, best_it, run, cnt);
}

// Members without columns (every word weighs 0, no exchange is possible) and calls of no iteration: key = what every iteration
// gives, iters_run = the count for every member; with no iteration only best and iters_run are written.
__global__ __launch_bounds__(BATCH_WAVE_THREADS) void isd_const_kernel(IsdArgs p, long long key, int32_t run, int64_t batch) {
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

// the slots, the keys and the word behind path 1's flags
int64_t lds_extra(int64_t width) { return 8 * ISD_WAVES + 8 * ISD_WAVES + 8 * width; }

// p0: the largest side of path 0
int plan(int64_t nrows, int64_t ncols, int64_t pivot_rows, int64_t t, int64_t p0) {
  if (nrows < 0 || ncols < 0 || pivot_rows < 0 || t < 0) return -1;
  if (pivot_rows > RS_K_MAX || ncols > RS_N_MAX || t > RS_T_MAX || binom_capped(pivot_rows, t) > ISD_SUMS_MAX) return 2;
  const int path = plan_on_order(nrows, ncols, p0, BATCH_LDS_BUDGET, 1, lds_extra(width_of(ncols)));
  return path <= 1 ? path : 2;
}

template <int WT>
void launch_block(const IsdArgs &p, dim3 grid, int threads, size_t lds, hipStream_t st, int ldw, int64_t b0) {
  hipLaunchKernelGGL(isd_block_kernel<WT>, grid, dim3(threads), lds, st, p, ldw, b0);
}

}  // namespace

extern "C" {

int m4ri_amd_plan_isd_search(int64_t nrows, int64_t ncols, int64_t pivot_rows, int64_t t) { return plan(nrows, ncols, pivot_rows, t, 64); }

int m4ri_amd_isd_search_dev(word *D, int64_t d_stride, int64_t d_bs, int64_t nrows, int64_t ncols, int64_t pivot_rows, int32_t *pivots, const int32_t *rank,
                            int64_t batch, int64_t iters, int64_t steps, uint64_t seed, int64_t t, int64_t w_min, int64_t w_stop, int32_t *order,
                            int64_t o_bs, int64_t olen, int64_t *best, int32_t *best_iter, int32_t *iters_run, int32_t *done, word *W, int64_t w_bs,
                            void *stream) {
  if (nrows < 0 || ncols < 0 || pivot_rows < 0 || olen < 0 || batch < 0 || iters < 0 || steps < 0 || t < 0 || w_min < 0 || d_stride < 0 || d_bs < 0 ||
      o_bs < 0 || w_bs < 0)
    return (int)hipErrorInvalidValue;
  if (pivot_rows > nrows || olen > ncols) return (int)hipErrorInvalidValue;
  const int64_t width = width_of(ncols);
  if (d_stride < width) return (int)hipErrorInvalidValue;
  const int path = plan(nrows, ncols, pivot_rows, t, env_bound("M4RI_AMD_ISD_SEARCH_PATH0_MAX", 64, 0, 64));
  if (path == 2) return (int)hipErrorNotSupported;
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
  IsdArgs p{};
  p.D = D, p.d_stride = d_stride, p.d_bs = d_bs;
  p.nrows = (int)nrows, p.ncols = (int)ncols, p.k = (int)pivot_rows, p.pm = (int)pm, p.olen = (int)olen, p.t = (int)t;
  p.has_v = nrows > pivot_rows, p.exchange = steps > 0 && iters > 1 && pm > 0;
  p.w_min = (int)(w_min > ncols + 1 ? ncols + 1 : w_min);
  p.iters = iters, p.steps = steps, p.w_stop = w_stop, p.seed = seed;
  p.pivots = pivots, p.rank = rank, p.order = olen > 0 ? order : nullptr, p.o_bs = o_bs;
  p.best = best, p.best_iter = best_iter, p.iters_run = iters_run, p.done = done, p.W = W, p.w_bs = w_bs;
  const int64_t sums = binom_capped(pivot_rows, t);
  if (iters == 0 || ncols == 0) {
    // no columns: every one of the `sums` words weighs 0, rank 0 is the lightest if weight 0 qualifies
    const long long key = iters > 0 && sums > 0 && w_min == 0 ? 0 : -1;
    const int32_t run   = key >= 0 && w_stop >= 0 ? 1 : (int32_t)iters;
    int64_t grid        = (batch + BATCH_WAVE_THREADS - 1) / BATCH_WAVE_THREADS;
    if (grid > 4096) grid = 4096;
    hipLaunchKernelGGL(isd_const_kernel, dim3((unsigned)grid), dim3(BATCH_WAVE_THREADS), 0, st, p, key, run, batch);
    HIPTRY(hipGetLastError());
    return 0;
  }
  p.n_upper = t <= 1 ? pivot_rows : binom_capped(pivot_rows, t - 1);
  if (path == 0)
    return launch_waves(batch, [&](dim3 grid, int64_t b0, int64_t nb) {
      hipLaunchKernelGGL(isd_wave_kernel, grid, dim3(BATCH_WAVE_THREADS), 0, st, p, b0, b0 + nb);
    });
  HIPTRY(set_max_dynamic_lds(BATCH_LDS_BUDGET, isd_block_kernel<1>, isd_block_kernel<2>, isd_block_kernel<4>, isd_block_kernel<8>, isd_block_kernel<16>));
  // A wave per chunk of 64 upper parts and per 512 words of the member, within what the exchange kernels take: a small member at
  // t = 2 is one wave, which meets no other at its barriers and leaves the compute unit's wave slots to other members.
  const int64_t n_uc = t == 0 ? 1 : (p.n_upper + 63) / 64, by_words = (nrows * width + 511) / 512;
  int64_t waves      = n_uc > by_words ? n_uc : by_words;
  if (waves > block_threads(nrows, width) / 64) waves = block_threads(nrows, width) / 64;
  const int threads = 64 * (int)(waves < 1 ? 1 : waves);
  const int ldw     = (int)lds_row_words(width);
  const size_t lds  = (size_t)(lds_bytes_staged(nrows, width, 1, lds_extra(width)) + (p.order ? 4 * olen : 0));
  return launch_members(batch, [&](dim3 grid, int64_t b0) {
    if (width <= 1) launch_block<1>(p, grid, threads, lds, st, ldw, b0);
    else if (width <= 2) launch_block<2>(p, grid, threads, lds, st, ldw, b0);
    else if (width <= 4) launch_block<4>(p, grid, threads, lds, st, ldw, b0);
    else if (width <= 8) launch_block<8>(p, grid, threads, lds, st, ldw, b0);
    else launch_block<16>(p, grid, threads, lds, st, ldw, b0);
  });
}

}  // extern "C"
