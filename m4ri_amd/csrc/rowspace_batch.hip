// rowspace_batch.hip -- weight distributions and minimum weights of the row spaces of many small matrices, one call for the batch,
// every result left on the device: the Four-Russians table of mzd_make_table (all 2^k combinations of k rows in Gray order) with a
// population count in place of the store.
//
// Member b has the generator G_b (k x n) and an optional word V_b (1 x n).  For every message x in [0, 2^k) the word is
// c_b(x) = V_b ^ XOR of the rows i of G_b with bit i of x set; hist[b * (n + 1) + w] counts the x with wt(c_b(x)) = w, lightest[b] is
// the minimum of (wt << 40) | x over the x with wt >= w_min (-1: none).
//
// One kernel, a wave its unit of work.  A message is split as x = (hi << s) | lo.  A wave stages the member's rows in its part of
// LDS (tail bits masked, the width padded to WT words), every lane takes one hi and forms its prefix V ^ (the rows s .. k-1 that hi
// selects) in WT register words, and then walks the 2^s values of lo in Gray order: step j adds row ctz(j), the same row in every
// lane, so rows 0 and 1 (three steps of four) sit in registers and the others are one broadcast LDS read; after step j the lane holds
// the word of lo = j ^ (j >> 1).  Per step and register word that is an XOR and a population count.
//   lightest  the lane keeps the minimum of ((wt - w_min) << s) | lo in 32 bits: s + 11 <= 31, and a wt below w_min wraps to a value
//             of 2^31 or more, so the filter costs nothing in the loop.  The 64-bit key is made once per lane at the end, reduced
//             across the wave by shuffles.
//   hist      32-bit bins in the wave's LDS, C interleaved copies of them (lane % C picks the copy, so lanes with one weight spread
//             over C banks), one LDS atomic per step; a wave counts at most 2^26 messages, so no bin overflows.  The copies are
//             summed into 64 bits at the end.
// The paths (m4ri_amd_plan_rowspace_weights_batch):
//   0  k <= RSW_K0: a wave owns the member (64 values of hi, s = k - 6; below k = 6 fewer lanes and s = 0), four members per
//      workgroup.  Every output entry is written once with a plain store.
//   1  above: the member's values of hi are spread over 2^(k - s - 6) waves, s = k - 19 held in [6, 12] (k < 12: the split of path 0,
//      one wave).  The outputs are set by an initialisation kernel on the same stream and combined with global 64-bit integer atomics,
//      one minimum per wave and one add per non-zero bin per wave: the order of arrival changes nothing.
// Plain launches on the caller's stream: no allocation, no copy to the host, no synchronisation, no engine workspace or lock.
#include <hip/hip_runtime.h>
#include <limits.h>
#include "batch_common.h"
#include "../../include/m4ri_amd.h"

namespace {

constexpr int64_t RSW_K_MAX  = 40;    // the message fits the key's low 40 bits
constexpr int64_t RSW_N_MAX  = 1024;  // a word in at most 16 register words (32 VGPRs) per lane
// Path 0 up to this k.  Measured (tools/bench_rowspace_weights.py, profiles/rowspace_weights_bench.txt) at 2^24 messages
// per call and n = 256, with and without hist, every spread under 2 %: path 0 is ahead of path 1 by 11 ... 38 % at k = 8, 10 and 12,
// each time by more than the spread, and loses from k = 14 on (0.85x at 1024 members, 0.3x at k = 16 with 256, 0.04x at k = 20 with
// 16: a wave per member no longer fills the device): K0 = 12.  M4RI_AMD_ROWSPACE_PATH0_MAX overrides it for the routing of a call.
constexpr int64_t RSW_K0     = 12;
constexpr int64_t RSW_K0_MAX = 26;    // the largest path-0 bound: s = k - 6 <= 20, the lane's 32-bit minimum and bins hold
constexpr int RSW_WAVES      = BATCH_WAVE_THREADS / 64;
constexpr int RSW_S1_MIN = 6, RSW_S1_MAX = 12, RSW_S1_OFF = 19;  // path 1: s = k - 19 in [6, 12], 2^13 waves and more from k = 25 on
constexpr int64_t RSW_BIN_WORDS = 2048;  // the bins of a wave, all copies: 8 KiB

struct RswArgs {
  const word *G, *V;  // V may be NULL
  int64_t g_stride, g_bs, v_bs;
  int k, s, n, width;  // width = words(n) >= 1
  word mask;           // of a row's last word
  int w_min;           // at most n + 1
  int cshift;          // 1 << cshift copies of the bins
  int row_words, bin_words;  // of a wave's part of LDS
  int wshift;          // 1 << wshift waves per member
  int atomic;          // path 1
  int64_t *hist, *lightest;
  int64_t u0, units;   // this launch: waves u0 .. units - 1 of batch << wshift
};

// wave u of the call: chunk u % 2^wshift of member u >> wshift; lane l takes hi = 64 * chunk + l.
template <int WT, bool HIST, bool LIGHT>
__global__ __launch_bounds__(BATCH_WAVE_THREADS) void rsw_kernel(RswArgs p) {
  extern __shared__ __align__(16) word rsw_lds[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t u = p.u0 + (int64_t)blockIdx.x * RSW_WAVES + wave;
  const bool live = u < p.units;  // wave-uniform; a wave past the end still meets the barriers
  const int64_t b = live ? u >> p.wshift : 0, chunk = u & (((int64_t)1 << p.wshift) - 1);
  word *rows      = rsw_lds + wave * p.row_words;
  uint32_t *bins  = reinterpret_cast<uint32_t *>(rsw_lds + RSW_WAVES * p.row_words) + wave * p.bin_words;
  const int s = p.s, k = p.k;
  if (live) {
    const word *g = p.G + b * p.g_bs;
    for (int idx = lane; idx < k * WT; idx += 64) {
      const int i = idx / WT, w = idx % WT;
      word x = 0;
      if (w < p.width) {
        x = g[(int64_t)i * p.g_stride + w];
        if (w == p.width - 1) x &= p.mask;
      }
      rows[idx] = x;
    }
  }
  if (HIST)
    for (int i = lane; i < p.bin_words; i += 64) bins[i] = 0;
  __syncthreads();
  const int64_t hi = (chunk << 6) | lane;
  const bool valid = live && hi < ((int64_t)1 << (k - s));
  uint32_t best = UINT32_MAX;
  if (valid) {
    word c[WT];
    const word *v = p.V ? p.V + b * p.v_bs : nullptr;
#pragma unroll
    for (int w = 0; w < WT; ++w) {
      c[w] = 0;
      if (v && w < p.width) c[w] = w == p.width - 1 ? v[w] & p.mask : v[w];
    }
    for (int i = 0; i < k - s; ++i) {
      const word m  = (word)0 - (word)((hi >> i) & 1);
      const word *r = rows + (s + i) * WT;
#pragma unroll
      for (int w = 0; w < WT; ++w) c[w] ^= r[w] & m;
    }
    const int negw     = -p.w_min;
    const int cshift   = p.cshift;
    uint32_t *my_bins  = bins + (p.w_min << cshift) + (lane & ((1 << cshift) - 1));  // indexed by (wt - w_min) << cshift
    auto weigh = [&](uint32_t j) {  // the word of lo = j ^ (j >> 1) is in c
      int acc = negw;
#pragma unroll
      for (int w = 0; w < WT; ++w) acc += __popcll(c[w]);
      if (LIGHT) {
        const uint32_t cand = ((uint32_t)acc << s) | (j ^ (j >> 1));
        best                = cand < best ? cand : best;
      }
      if (HIST) atomicAdd(my_bins + (int)((uint32_t)acc << cshift), 1u);
    };
    if (s < 2) {
      weigh(0);
      if (s == 1) {
#pragma unroll
        for (int w = 0; w < WT; ++w) c[w] ^= rows[w];
        weigh(1);
      }
    } else {
      word r0[WT], r1[WT];
#pragma unroll
      for (int w = 0; w < WT; ++w) r0[w] = rows[w], r1[w] = rows[WT + w];
      const uint32_t na = 1u << (s - 2);
      for (uint32_t a = 0; a < na; ++a) {  // steps 4a .. 4a + 3: rows 2 + ctz(a) (a > 0), 0, 1, 0
        if (a) {
          const word *r = rows + (2 + __builtin_ctz(a)) * WT;
#pragma unroll
          for (int w = 0; w < WT; ++w) c[w] ^= r[w];
        }
        weigh(4 * a);
#pragma unroll
        for (int w = 0; w < WT; ++w) c[w] ^= r0[w];
        weigh(4 * a + 1);
#pragma unroll
        for (int w = 0; w < WT; ++w) c[w] ^= r1[w];
        weigh(4 * a + 2);
#pragma unroll
        for (int w = 0; w < WT; ++w) c[w] ^= r0[w];
        weigh(4 * a + 3);
      }
    }
  }
  if (LIGHT) {
    unsigned long long key = ~0ull;  // none
    if (valid && best < 0x80000000u)
      key = ((unsigned long long)((best >> s) + (uint32_t)p.w_min) << 40) | ((unsigned long long)hi << s) | (best & ((1u << s) - 1));
    for (int o = 32; o; o >>= 1) {
      const unsigned long long t = __shfl_xor(key, o);
      key                        = t < key ? t : key;
    }
    if (live && lane == 0) {
      if (!p.atomic) p.lightest[b] = (int64_t)key;
      else {  // most waves find the member's minimum already as low as theirs: ask before the atomic, which all of them would queue for
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
        unsigned long long t = 0;
        for (int cpy = 0; cpy < (1 << p.cshift); ++cpy) t += bins[(w << p.cshift) + cpy];
        if (!p.atomic) h[w] = (int64_t)t;
        else if (t) atomicAdd(reinterpret_cast<unsigned long long *>(h + w), t);
      }
    }
  }
}

// hist[0 .. hist_count) = hist_v, lightest[0 .. batch) = lightest_v: what path 1's atomics start from, and the results of members
// without columns
__global__ __launch_bounds__(BATCH_WAVE_THREADS) void rsw_init_kernel(int64_t *hist, int64_t hist_count, int64_t hist_v, int64_t *lightest, int64_t batch,
                                                                      int64_t lightest_v) {
  const int64_t t0 = (int64_t)blockIdx.x * BATCH_WAVE_THREADS + threadIdx.x, step = (int64_t)gridDim.x * BATCH_WAVE_THREADS;
  if (hist)
    for (int64_t i = t0; i < hist_count; i += step) hist[i] = hist_v;
  if (lightest)
    for (int64_t i = t0; i < batch; i += step) lightest[i] = lightest_v;
}

int launch_init(hipStream_t st, int64_t *hist, int64_t hist_count, int64_t hist_v, int64_t *lightest, int64_t batch, int64_t lightest_v) {
  const int64_t items = hist && hist_count > batch ? hist_count : batch;
  int64_t grid        = (items + BATCH_WAVE_THREADS - 1) / BATCH_WAVE_THREADS;
  if (grid > 4096) grid = 4096;
  hipLaunchKernelGGL(rsw_init_kernel, dim3((unsigned)grid), dim3(BATCH_WAVE_THREADS), 0, st, hist, hist_count, hist_v, lightest, batch, lightest_v);
  HIPTRY(hipGetLastError());
  return 0;
}

template <int WT>
void launch_wt(const RswArgs &p, dim3 grid, size_t lds, hipStream_t st) {
  if (p.hist && p.lightest) hipLaunchKernelGGL((rsw_kernel<WT, true, true>), grid, dim3(BATCH_WAVE_THREADS), lds, st, p);
  else if (p.hist) hipLaunchKernelGGL((rsw_kernel<WT, true, false>), grid, dim3(BATCH_WAVE_THREADS), lds, st, p);
  else hipLaunchKernelGGL((rsw_kernel<WT, false, true>), grid, dim3(BATCH_WAVE_THREADS), lds, st, p);
}

int plan(int64_t k, int64_t n, int64_t k0) {
  if (k < 0 || n < 0) return -1;
  return n == 0 || k <= k0 ? 0 : 1;
}

}  // namespace

extern "C" {

int m4ri_amd_plan_rowspace_weights_batch(int64_t k, int64_t n) { return plan(k, n, RSW_K0); }

int m4ri_amd_rowspace_weights_batch_dev(const word *G, int64_t g_stride, int64_t g_bs, int64_t k, int64_t n, const word *V, int64_t v_bs, int64_t batch,
                                        int64_t w_min, int64_t *hist, int64_t *lightest, void *stream) {
  hipStream_t st = (hipStream_t)stream;
  if (k < 0 || n < 0 || batch < 0 || g_stride < 0 || g_bs < 0 || v_bs < 0 || w_min < 0) return (int)hipErrorInvalidValue;
  if (k > RSW_K_MAX || n > RSW_N_MAX) return (int)hipErrorNotSupported;
  if (!hist && !lightest) return (int)hipErrorInvalidValue;
  const int64_t width = width_of(n);
  const bool data     = k > 0 && n > 0;  // G has words
  if (n > 0 && k > 1 && g_stride < width) return (int)hipErrorInvalidValue;
  if (batch > 0) {
    if (data && !G) return (int)hipErrorInvalidValue;
    if (spans_meet_any({entries_span(hist, batch, n + 1, n + 1, 8), entries_span(lightest, batch, 1, 1, 8)},
                       {rows_span(G, batch, g_bs, k, g_stride, width), rows_span(V, batch, v_bs, 1, 0, width)}))
      return (int)hipErrorInvalidValue;
  }
  if (batch == 0) return 0;
  if (n == 0)  // every word weighs 0: all 2^k messages in the one bin, the lightest is message 0 if weight 0 qualifies
    return launch_init(st, hist, batch, (int64_t)1 << k, lightest, batch, w_min == 0 ? 0 : -1);
  RswArgs p{};
  p.G = G, p.V = V, p.g_stride = g_stride, p.g_bs = g_bs, p.v_bs = v_bs, p.k = (int)k, p.n = (int)n, p.width = (int)width;
  p.mask = tail_mask((int)(n & 63)), p.w_min = (int)(w_min > n + 1 ? n + 1 : w_min), p.hist = hist, p.lightest = lightest;
  p.atomic = plan(k, n, env_bound("M4RI_AMD_ROWSPACE_PATH0_MAX", RSW_K0, -1, RSW_K0_MAX));  // -1: no path 0
  if (!p.atomic || k < 2 * RSW_S1_MIN) p.s = k > 6 ? (int)k - 6 : 0;
  else p.s = k - RSW_S1_OFF < RSW_S1_MIN ? RSW_S1_MIN : k - RSW_S1_OFF > RSW_S1_MAX ? RSW_S1_MAX : (int)k - RSW_S1_OFF;
  p.wshift = k - p.s > 6 ? (int)k - p.s - 6 : 0;
  int wt   = 1;
  while (wt < width) wt *= 2;
  p.row_words = (int)(k > 0 ? k : 1) * wt;
  if (hist) {
    while (p.cshift < 5 && ((n + 1) << (p.cshift + 1)) <= RSW_BIN_WORDS) ++p.cshift;
    p.bin_words = (int)((n + 1) << p.cshift);
  }
  const size_t lds = (size_t)RSW_WAVES * ((size_t)p.row_words * 8 + (size_t)p.bin_words * 4);
  if (p.atomic) HIPTRY(launch_init(st, hist, batch * (n + 1), 0, lightest, batch, -1));
  p.units = batch << p.wshift;
  return launch_waves(p.units, [&](dim3 grid, int64_t u0, int64_t) {
    p.u0 = u0;
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
