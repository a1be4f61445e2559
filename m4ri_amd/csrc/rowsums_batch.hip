// rowsums_batch.hip -- the weights of all sums of exactly t rows of many small matrices, one call for the batch, every result left on
// the device: what Brouwer-Zimmermann minimum-distance bounds, Lee-Brickell / Stern information-set decoding and "any light combination
// of few rows?" filters enumerate, for generators far beyond the k = 40 at which the whole row space (rowspace_batch.hip) ends.
//
// Member b has the generator G_b (k x n) and an optional word V_b (1 x n).  For every set S = {i_0 < ... < i_{t-1}} of row indices
// the word is c_b(S) = V_b ^ the rows of G_b in S, its rank the colexicographic r(S) = sum_j C(i_j, j + 1).
// hist[b * (n + 1) + w] counts the S with wt(c_b(S)) = w, lightest[b] is the minimum of (wt << 40) | r(S) over the S with
// wt >= w_min (-1: none).
//
// One kernel, a wave its unit of work.  A lane owns the UPPER PART U = {i_1 < ... < i_{t-1}} of a set: the 64 lanes of a wave take
// 64 consecutive U in the colexicographic order of (t-1)-subsets of [0, k), which each lane unranks from the top element down: the
// lowest is the rest of the rank itself, the second a square root, the others a bisection in a table of binomials (so t <= 3 reads
// no table).  The lane's prefix V ^ rows of U is gathered from global memory into WT register words, with rank base
// sum_{j >= 1} C(i_j, j + 1).  Then the wave walks i_0 = 0, 1, ... together:
// the row is the same in every lane, one broadcast LDS read per word, and a lane takes part while i_0 < i_1 (for t = 2 the lanes are
// 64 consecutive i_1, for t >= 3 consecutive U mostly differ in i_1 alone).  Per step and register word that is an XOR and a
// population count, with no dependency between steps.  t = 1 has no walk: a lane per row, weighed once.
// The rows of the walk are staged in LDS (tail bits masked, the width padded to WT words) a SEGMENT at a time, so that k = 1024 rows
// of 16 words need no more LDS than k = 64: a unit of work is (64 U, a segment of i_0).
//   lightest  per U the lane keeps the minimum of ((wt - w_min) << 10) | i_0 in 32 bits: a wt below w_min wraps to 2^31 or more, so
//             the filter costs nothing in the loop.  The 64-bit key, with the rank base added, is made once per U and lane, and
//             reduced across the wave by shuffles at the end.
//   hist      32-bit bins in the wave's LDS, C interleaved copies of them (lane % C picks the copy), one LDS atomic per step; a wave
//             counts at most 2^24 sums, so no bin overflows.  The copies are summed into 64 bits at the end.
// The paths (m4ri_amd_plan_row_sums_weights_batch):
//   0  at most RS_M0 sums per member: a wave walks all units of its member, segments outside (RS_ROW_WORDS / WT rows in the wave's own
//      part of LDS), four members per workgroup.  Every output entry is written once with a plain store.
//   1  above: a workgroup per (four consecutive chunks of 64 U, segment); its waves stage the segment together, four times as many
//      rows, and take a chunk each.  A call of few workgroups (one member of many rows at t = 2) halves its segments until there are
//      RS_BLOCKS_MIN of them.  The outputs are set by an initialisation kernel on the same stream and combined with global 64-bit
//      integer atomics, one minimum per wave and one add per non-zero bin per wave: the order of arrival changes nothing.
// Members without sums or columns (t = 0, k < t, n = 0) are answered by the initialisation kernel alone.
// Plain launches on the caller's stream: no allocation, no copy to the host, no synchronisation, no engine workspace or lock.
#include <hip/hip_runtime.h>
#include <limits.h>
#include "batch_common.h"
#include "subset_rank.h"  // the limits RS_*_MAX, binom_capped, binom_elem, unrank_step
#include "../../include/m4ri_amd.h"

namespace {

// Path 0 up to this many sums per member.  Measured (tools/bench_row_sums_weights.py, profiles/row_sums_weights_bench.txt)
// at about 2^24 sums per call and n = 256, t = 2 and 3, with and without hist, the spreads of these rows under 1 %: path 0 is ahead of
// path 1 by 11 % ... 4.1x at 120 ... 16 471 sums per member (k = 182, t = 2: 1.11x and 1.27x), each time by more than the spread, and
// loses from 19 600 on (k = 50, t = 3: 0.66x; 0.31x at 41 664; a wave per member no longer fills the device): M0 = 16 471 = C(182, 2).
// M4RI_AMD_ROW_SUMS_PATH0_MAX overrides it for the routing of a call.
constexpr int64_t RS_M0       = 16471;
constexpr int64_t RS_M0_MAX   = (int64_t)1 << 24;  // the largest path-0 bound: the 32-bit bins of a wave hold
constexpr int RS_WAVES        = BATCH_WAVE_THREADS / 64;
constexpr int RS_ROW_WORDS    = 1024;  // the staged rows of a wave: 8 KiB, a segment of 1024 / WT rows
constexpr int64_t RS_BIN_WORDS = 2048; // the bins of a wave, all copies: 8 KiB
constexpr int RS_SEG_MIN       = 16;   // path 1 halves its segments down to this many rows ...
constexpr int64_t RS_BLOCKS_MIN = 1024; // ... while the call has fewer workgroups than this: four per compute unit

struct RsArgs {
  const word *G, *V;  // V may be NULL
  int64_t g_stride, g_bs, v_bs;
  int k, t, n, width;  // width = words(n) >= 1; 1 <= t <= k
  word mask;           // of a row's last word
  int w_min;           // at most n + 1
  int cshift;          // 1 << cshift copies of the bins
  int bin_words;       // of a wave's part of LDS
  int seg_rows;        // rows per segment: what the wave's part of LDS holds on path 0, the workgroup's on path 1
  int atomic;          // path 1
  int64_t n_upper;     // C(k, t - 1) upper parts (t = 1: the k rows)
  int64_t n_uc;        // chunks of 64 of them
  int64_t n_ucg;       // path 1: groups of four chunks
  int n_seg;           // segments of i_0 (t = 1: one, nothing staged)
  int64_t *hist, *lightest;
  int64_t u0, units;   // this launch: from u0 on, of `units`; path 0: waves, a member each; path 1: batch * n_ucg * n_seg workgroups
};

// Path 0: wave u is member u, stages its own segments and takes every (segment, chunk) of its member.  Path 1: workgroup u is
// (member, four consecutive chunks, segment); its waves share one staged segment, four times as long, and take a chunk each.
template <int WT, bool HIST, bool LIGHT>
__global__ __launch_bounds__(BATCH_WAVE_THREADS) void rs_kernel(RsArgs p) {
  extern __shared__ __align__(16) word rs_lds[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const bool shared = p.atomic;  // the staged rows belong to the workgroup
  const int64_t u   = shared ? p.u0 + blockIdx.x : p.u0 + (int64_t)blockIdx.x * RS_WAVES + wave;
  const bool live   = u < p.units;  // wave-uniform; a wave past the end still meets the barriers
  int64_t b = 0, uc_lo = 0, uc_hi = p.n_uc;
  int seg_lo = 0, seg_hi = p.n_seg;
  if (shared) {
    const int64_t per = p.n_ucg * p.n_seg;
    b                 = u / per;
    const int64_t r   = u - b * per, grp = r / p.n_seg;
    seg_lo            = (int)(r - grp * p.n_seg);
    uc_lo             = grp * RS_WAVES + wave;
    uc_hi = uc_lo + 1 < p.n_uc ? uc_lo + 1 : p.n_uc, seg_hi = seg_lo + 1;  // a wave beyond the last chunk walks nothing
  } else if (live) b = u;
  word *rows     = rs_lds + (shared ? 0 : wave * RS_ROW_WORDS);
  uint32_t *bins = reinterpret_cast<uint32_t *>(rs_lds + RS_WAVES * RS_ROW_WORDS) + wave * p.bin_words;
  const int k = p.k, t = p.t;
  const int tu   = t == 1 ? 1 : t - 1;   // the size of an upper part; for t = 1 it is the set itself
  const int boff = t == 1 ? 0 : 1;       // element m (1 .. tu) of an upper part adds C(e, m + boff) to the rank
  const word *g  = p.G + b * p.g_bs;
  const word *v  = p.V ? p.V + b * p.v_bs : nullptr;
  if (HIST)
    for (int i = lane; i < p.bin_words; i += 64) bins[i] = 0;
  constexpr int UNROLL = WT <= 2 ? 4 : WT <= 4 ? 2 : 1;  // steps of the walk in flight
  const int negw       = -p.w_min;
  const int cshift  = p.cshift;
  uint32_t *my_bins = bins + (p.w_min << cshift) + (lane & ((1 << cshift) - 1));  // indexed by (wt - w_min) << cshift
  unsigned long long key = ~0ull;  // the lane's lightest: none
  for (int seg = seg_lo; seg < seg_hi; ++seg) {
    const int seg0 = seg * p.seg_rows;
    if (seg > seg_lo) __syncthreads();  // the walks of the segment before are over
    if (live && t > 1) {
      const int nr = k - seg0 < p.seg_rows ? k - seg0 : p.seg_rows;
      for (int idx = shared ? (int)threadIdx.x : lane; idx < nr * WT; idx += shared ? BATCH_WAVE_THREADS : 64) {
        const int i = idx / WT, w = idx % WT;
        word x = 0;
        if (w < p.width) {
          x = g[(int64_t)(seg0 + i) * p.g_stride + w];
          if (w == p.width - 1) x &= p.mask;
        }
        rows[idx] = x;
      }
    }
    __syncthreads();
    if (!live) continue;
    for (int64_t uc = uc_lo; uc < uc_hi; ++uc) {
      unsigned long long rest = (unsigned long long)((uc << 6) | lane);
      const bool valid        = rest < (unsigned long long)p.n_upper;
      word c[WT];
#pragma unroll
      for (int w = 0; w < WT; ++w) {
        c[w] = 0;
        if (v && w < p.width) c[w] = w == p.width - 1 ? v[w] & p.mask : v[w];
      }
      unsigned long long base = 0;
      int e = k;  // the element above the one looked for; after the loop, the smallest element: i_1 (t = 1: the row)
      if (valid) {
        for (int m = tu; m >= 1; --m) {  // the largest e' < e with C(e', m) <= rest
          e = unrank_step(rest, m, e);
          base += binom_elem(e, m + boff);
          const word *r = g + (int64_t)e * p.g_stride;
#pragma unroll
          for (int w = 0; w < WT; ++w)
            if (w < p.width) c[w] ^= w == p.width - 1 ? r[w] & p.mask : r[w];
        }
      }
      if (t == 1) {
        if (valid) {
          int acc = negw;
#pragma unroll
          for (int w = 0; w < WT; ++w) acc += __popcll(c[w]);
          if (LIGHT && acc >= 0) {
            const unsigned long long cand = ((unsigned long long)(uint32_t)(acc + p.w_min) << 40) | base;
            key                           = cand < key ? cand : key;
          }
          if (HIST) atomicAdd(my_bins + (int)((uint32_t)acc << cshift), 1u);
        }
        continue;
      }
      // i_0 runs over [seg0, end) in this lane, over [seg0, wave_end) in the wave
      int end = valid ? e : 0;
      if (end > seg0 + p.seg_rows) end = seg0 + p.seg_rows;
      int wave_end = end;
      for (int o = 32; o; o >>= 1) {
        const int x = __shfl_xor(wave_end, o);
        wave_end    = x > wave_end ? x : wave_end;
      }
      uint32_t best = UINT32_MAX;
#pragma unroll UNROLL
      for (int i0 = seg0; i0 < wave_end; ++i0) {
        const word *r = rows + (i0 - seg0) * WT;
        int acc       = negw;
#pragma unroll
        for (int w = 0; w < WT; ++w) acc += __popcll(c[w] ^ r[w]);
        if (i0 < end) {
          if (LIGHT) {
            const uint32_t cand = ((uint32_t)acc << 10) | (uint32_t)i0;
            best                = cand < best ? cand : best;
          }
          if (HIST) atomicAdd(my_bins + (int)((uint32_t)acc << cshift), 1u);
        }
      }
      if (LIGHT && best < 0x80000000u) {
        const unsigned long long cand = ((unsigned long long)((best >> 10) + (uint32_t)p.w_min) << 40) | (base + (best & 1023u));
        key                           = cand < key ? cand : key;
      }
    }
  }
  if (LIGHT) {
    for (int o = 32; o; o >>= 1) {
      const unsigned long long x = __shfl_xor(key, o);
      key                        = x < key ? x : key;
    }
    if (live && lane == 0) {
      if (!p.atomic) p.lightest[b] = (int64_t)key;
      else if (key != ~0ull) {  // most waves find the member's minimum already as low as theirs: ask before the atomic
        unsigned long long *out = reinterpret_cast<unsigned long long *>(p.lightest + b);
        if (key < __hip_atomic_load(out, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMin(out, key);
      }
    }
  }
  if (HIST) {
    __syncthreads();
    if (live) {
      int64_t *h = p.hist + b * ((int64_t)p.n + 1);
      for (int w = lane; w <= p.n; w += 64) {
        unsigned long long s = 0;
        for (int cpy = 0; cpy < (1 << cshift); ++cpy) s += bins[(w << cshift) + cpy];
        if (!p.atomic) h[w] = (int64_t)s;
        else if (s) atomicAdd(reinterpret_cast<unsigned long long *>(h + w), s);
      }
    }
  }
}

struct RsInit {
  int64_t *hist, *lightest;
  int64_t batch, row;      // row = n + 1 entries of hist per member
  int64_t hist0, light_v;  // hist[b][0] = hist0, the other entries 0; lightest[b] = light_v
  // t = 0 with columns: the one sum is V_b.  hist[b][wt(V_b)] = 1, lightest[b] = wt << 40 if wt >= w_min
  int single;
  const word *V;
  int64_t v_bs;
  int width;
  word mask;
  int64_t w_min;
};

// What path 1's atomics start from, and the whole result of members without sums or columns and of t = 0.
__global__ __launch_bounds__(BATCH_WAVE_THREADS) void rs_init_kernel(RsInit p) {
  const int64_t t0 = (int64_t)blockIdx.x * BATCH_WAVE_THREADS + threadIdx.x, step = (int64_t)gridDim.x * BATCH_WAVE_THREADS;
  auto weight = [&](int64_t b) {
    int64_t wt = 0;
    if (p.V)
      for (int w = 0; w < p.width; ++w) wt += __popcll(w == p.width - 1 ? p.V[b * p.v_bs + w] & p.mask : p.V[b * p.v_bs + w]);
    return wt;
  };
  if (p.hist)
    for (int64_t i = t0; i < p.batch * p.row; i += step) {
      const int64_t b = i / p.row, w = i - b * p.row;
      p.hist[i] = p.single ? (int64_t)(w == weight(b)) : w == 0 ? p.hist0 : 0;
    }
  if (p.lightest)
    for (int64_t b = t0; b < p.batch; b += step) {
      int64_t x = p.light_v;
      if (p.single) {
        const int64_t wt = weight(b);
        x = wt >= p.w_min ? wt << 40 : -1;
      }
      p.lightest[b] = x;
    }
}

int launch_init(hipStream_t st, const RsInit &p) {
  const int64_t items = p.hist ? p.batch * p.row : p.batch;
  int64_t grid        = (items + BATCH_WAVE_THREADS - 1) / BATCH_WAVE_THREADS;
  if (grid > 4096) grid = 4096;
  hipLaunchKernelGGL(rs_init_kernel, dim3((unsigned)grid), dim3(BATCH_WAVE_THREADS), 0, st, p);
  HIPTRY(hipGetLastError());
  return 0;
}

template <int WT>
void launch_wt(const RsArgs &p, dim3 grid, size_t lds, hipStream_t st) {
  if (p.hist && p.lightest) hipLaunchKernelGGL((rs_kernel<WT, true, true>), grid, dim3(BATCH_WAVE_THREADS), lds, st, p);
  else if (p.hist) hipLaunchKernelGGL((rs_kernel<WT, true, false>), grid, dim3(BATCH_WAVE_THREADS), lds, st, p);
  else hipLaunchKernelGGL((rs_kernel<WT, false, true>), grid, dim3(BATCH_WAVE_THREADS), lds, st, p);
}

int plan(int64_t k, int64_t n, int64_t t, int64_t m0) {
  if (k < 0 || n < 0 || t < 0) return -1;
  if (n == 0 || t == 0 || k < t) return 0;  // the initialisation kernel alone
  return binom_capped(k, t) <= m0 ? 0 : 1;
}

}  // namespace

extern "C" {

int m4ri_amd_plan_row_sums_weights_batch(int64_t k, int64_t n, int64_t t) { return plan(k, n, t, RS_M0); }

int m4ri_amd_row_sums_weights_batch_dev(const word *G, int64_t g_stride, int64_t g_bs, int64_t k, int64_t n, const word *V, int64_t v_bs, int64_t batch,
                                        int64_t t, int64_t w_min, int64_t *hist, int64_t *lightest, void *stream) {
  hipStream_t st = (hipStream_t)stream;
  if (k < 0 || n < 0 || batch < 0 || g_stride < 0 || g_bs < 0 || v_bs < 0 || t < 0 || w_min < 0) return (int)hipErrorInvalidValue;
  if (k > RS_K_MAX || n > RS_N_MAX || t > RS_T_MAX) return (int)hipErrorNotSupported;
  const int64_t sums = binom_capped(k, t);
  if (sums > RS_SUMS_MAX) return (int)hipErrorNotSupported;
  if (!hist && !lightest) return (int)hipErrorInvalidValue;
  const int64_t width = width_of(n);
  const bool walked   = k >= t && t >= 1 && n > 0;  // and they are read
  if (n > 0 && k > 1 && g_stride < width) return (int)hipErrorInvalidValue;
  if (batch > 0) {
    if (walked && !G) return (int)hipErrorInvalidValue;
    if (spans_meet_any({entries_span(hist, batch, n + 1, n + 1, 8), entries_span(lightest, batch, 1, 1, 8)},
                       {rows_span(G, batch, g_bs, k, g_stride, width), rows_span(V, batch, v_bs, 1, 0, width)}))  // G where it has words, read or not
      return (int)hipErrorInvalidValue;
  }
  if (batch == 0) return 0;
  RsInit in{};
  in.hist = hist, in.lightest = lightest, in.batch = batch, in.row = n + 1, in.light_v = -1;
  if (n == 0 || sums == 0) {  // every word weighs 0: all sums in the one bin, the lightest is rank 0 if weight 0 qualifies; or no sums
    in.hist0 = sums, in.light_v = sums > 0 && w_min == 0 ? 0 : -1;
    return launch_init(st, in);
  }
  const word mask = tail_mask((int)(n & 63));
  if (t == 0) {
    in.single = 1, in.V = V, in.v_bs = v_bs, in.width = (int)width, in.mask = mask, in.w_min = w_min;
    return launch_init(st, in);
  }
  RsArgs p{};
  p.G = G, p.V = V, p.g_stride = g_stride, p.g_bs = g_bs, p.v_bs = v_bs, p.k = (int)k, p.t = (int)t, p.n = (int)n, p.width = (int)width;
  p.mask = mask, p.w_min = (int)(w_min > n + 1 ? n + 1 : w_min), p.hist = hist, p.lightest = lightest;
  p.atomic = plan(k, n, t, env_bound("M4RI_AMD_ROW_SUMS_PATH0_MAX", RS_M0, -1, RS_M0_MAX));  // -1: no path 0
  int wt   = 1;
  while (wt < width) wt *= 2;
  p.seg_rows = (p.atomic ? RS_WAVES : 1) * RS_ROW_WORDS / wt;
  p.n_upper  = t == 1 ? k : binom_capped(k, t - 1);
  p.n_uc     = (p.n_upper + 63) / 64;
  p.n_ucg    = (p.n_uc + RS_WAVES - 1) / RS_WAVES;
  auto n_seg = [&] { return t == 1 || k < 2 ? 1 : (int)((k - 1 + p.seg_rows - 1) / p.seg_rows); };  // i_0 <= k - 2
  // path 1 with few workgroups (one member of many rows at t = 2): shorter segments, down to RS_SEG_MIN rows, until the device is full
  while (p.atomic && p.seg_rows > RS_SEG_MIN && batch * p.n_ucg * n_seg() < RS_BLOCKS_MIN) p.seg_rows /= 2;
  p.n_seg = n_seg();
  if (hist) {
    while (p.cshift < 5 && ((n + 1) << (p.cshift + 1)) <= RS_BIN_WORDS) ++p.cshift;
    p.bin_words = (int)((n + 1) << p.cshift);
  }
  const size_t lds = (size_t)RS_WAVES * ((size_t)RS_ROW_WORDS * 8 + (size_t)p.bin_words * 4);
  if (p.atomic) HIPTRY(launch_init(st, in));
  p.units = p.atomic ? batch * p.n_ucg * p.n_seg : batch;
  return launch_chunked(p.units, p.atomic ? BATCH_CHUNK : BATCH_CHUNK * RS_WAVES, [&](int64_t u0, int64_t nu) {
    p.u0 = u0;
    const dim3 grid((unsigned)(p.atomic ? nu : (nu + RS_WAVES - 1) / RS_WAVES));
    switch (wt) {
      case 1: launch_wt<1>(p, grid, lds, st); break;
      case 2: launch_wt<2>(p, grid, lds, st); break;
      case 4: launch_wt<4>(p, grid, lds, st); break;
      case 8: launch_wt<8>(p, grid, lds, st); break;
      default: launch_wt<16>(p, grid, lds, st); break;
    }
  });
}

}  // extern "C"
