// rowsums_collide_batch.hip -- Stern's / Dumer's collision step on many small generators, one call for the batch, every result left on the
// device: of the N1 * N2 pairs (t1 of the first k1 rows, t2 of the other k2 = k - k1) only those whose sum, with V, vanishes on a window
// of ell chosen columns are weighed.  rowsums_batch.hip weighs every sum of t rows; this file joins the two halves on the window bits
// first, so the full-width work falls from C(k, t1 + t2) words to about N1 * N2 / 2^ell.
//
// Member b has the generator G_b (k x n), an optional word V_b and a window cols_b of ell columns.  S1 is a set of t1 LEFT rows
// (0 .. k1-1) of colexicographic rank r1 < N1 = C(k1, t1), S2 a set of t2 RIGHT rows (k1 .. k-1), r2 < N2 = C(k2, t2) the rank of
// {i - k1}.  The word is c = V ^ rows S1 ^ rows S2; the pair COLLIDES iff c is 0 at every window column.  hist[b * (n + 1) + w] counts
// the colliding pairs of weight w (all n columns), lightest[b] is the minimum of (wt << 40) | (r1 * N2 + r2) over the colliding pairs
// with wt >= w_min (-1: none).  A member with a window entry outside [0, n) is REFUSED on the device: every hist entry -1, lightest -2.
//
// One kernel, a workgroup its unit of work: it owns a member and a slice of the member's right sums.
//   keys    the window (range-checked: a refused member's workgroup stops here) goes to LDS, then a thread per row gathers the row's ell
//           window bits into one 64-bit key in LDS, k + 1 of them with V's.
//   table   a thread per r1 unranks S1 (subset_rank.h, as rowsums_batch.hip does) and XORs the row keys.  The N1 entries (key, r1) are
//           counting-sorted in LDS on the key's low q bits, q = ceil(log2 N1) held at ell: count with LDS atomics, scan, scatter.  The
//           keys are made twice (once to count, once to scatter) rather than held: 8192 entries of 8 + 2 bytes, 8192 bucket ends and
//           the row keys are 120 KiB, an unsorted copy of the keys would not fit beside them.
//   walk    a lane per r2 unranks S2, key2 = V's key ^ the row keys, and compares the FULL key of every entry of bucket key2 mod 2^q.
//           For a match the lane gathers V and the t1 + t2 rows from global memory (a member stays in L2), weighs the word, adds to a
//           32-bit bin in LDS and keeps its own minimum key.  Matches are rare by design, so the divergent weighing is left as it is.
//   output  the lanes' minima are reduced by shuffles and through LDS, the bins read out.
// The paths (m4ri_amd_plan_row_sums_collide_batch):
//   0  at most RC_P0 pairs per member: one workgroup takes the member's whole right list and writes every output entry once with a
//      plain store, the refused form included.  N1 * N2 < 2^32, so no 32-bit bin overflows.
//   1  above: the right list is cut into slices (m4ri_amd_row_sums_collide_slices), a workgroup each; every workgroup rebuilds the left
//      table, so a slice is never shorter than N1 (or RC_SLICE_MIN) unless the list is, and slice * N1 < 2^32.  The outputs are set by an
//      initialisation kernel on the same stream (which also answers the refused members: their workgroups return without writing) and
//      combined with global 64-bit integer atomics, one minimum and one add per non-zero bin per workgroup: the order changes nothing.
// Members without pairs (t1 > k1, t2 > k2) or without columns are answered by the initialisation kernel alone.
//
// The list (m4ri_amd_row_sums_collide_list_batch_dev; LIST instantiations only, the others are compiled as before): where a match is
// weighed, a pair with w_min <= wt <= w_max takes a slot and, if the slot is below cap, stores its key (wt << 40) | pair rank at
// list[b * l_bs + slot]; count[b] ends as the number of slots taken, whatever cap is.
//   0  the slot comes from a 32-bit counter in the workgroup's LDS (N1 * N2 < 2^32), count[b] is one plain store at the end: no global
//      atomic.
//   1  the initialisation kernel writes count 0 (-1 for a refused member), every match takes its slot with one returning 64-bit global
//      atomic add on count[b]: the plain form, no aggregation per wave or workgroup (DESIGN.md 3.12 says why).
// Plain launches on the caller's stream: no allocation, no copy to the host, no synchronisation, no engine workspace or lock.
#include <hip/hip_runtime.h>
#include <limits.h>
#include <stdlib.h>
#include <mutex>
#include "batch_common.h"
#include "subset_rank.h"
#include "../../include/m4ri_amd.h"

namespace {

constexpr int64_t RC_ELL_MAX = 64;    // a key is one 64-bit word
constexpr int64_t RC_N1_MAX  = 8192;  // the left table of one workgroup: C(128, 2) = 8128 fits, C(129, 2) = 8256 does not
// Path 0 up to this many pairs per member.  Measured (tools/bench_row_sums_collide.py, profiles/row_sums_collide_bench.txt)
// on a ladder of N2 = C(k2, 2) against N1 = C(64, 2) = 2016 at n = 256, ell = 16, both outputs, about 2^32 pairs per call, the spreads of
// these rows under 1 %: path 0 is ahead of path 1 by 3 % at 241 920 ... 4 064 256 pairs per member (what the initialisation launch
// costs: the right list is one slice there), by 13 %, 2 % and 1 % at 8 255 520, 16 386 048 and 33 205 536 (k2 = 182; 129 members), each
// time by more than the spread, and loses from 65 802 240 on (k2 = 256, 65 members: 0.60x; 0.15x at 263 725 056: a workgroup per member
// no longer fills the device, sixteen slices per member do): P0 = 33 205 536 = C(64, 2) * C(182, 2).  The join looks at every right sum
// once, not at every pair: at these sizes a call is 0.1 ms, and what the bound decides is small either way.
// M4RI_AMD_ROW_SUMS_COLLIDE_PATH0_MAX overrides it for the routing of a call.
constexpr int64_t RC_P0         = 33205536;
constexpr int64_t RC_P0_MAX     = ((int64_t)1 << 32) - 1;  // the largest path-0 bound, and of slice * N1: the 32-bit bins of a workgroup hold
constexpr int64_t RC_BLOCKS_MIN = 1024;                    // path 1 cuts the right lists until the call has this many workgroups ...
constexpr int64_t RC_SLICE_MIN  = 256;                     // ... but no slice shorter than this, or than N1
constexpr int RC_THREADS_MAX    = BATCH_MAX_THREADS;
constexpr int RC_WT             = 16;  // register words of a weighed word: n <= 1024

// where the pieces of a workgroup's LDS are, in bytes; the same arithmetic on both sides of the launch
struct RcCarve {
  size_t skey, wmin, off, part, bins, cols, sr1, slots, total;
  __host__ __device__ RcCarve(int k, int n, int n1, int q, bool list = false) {
    skey  = (size_t)(k + 1) * 8;                  // the row keys first: k + 1 words, V's last
    wmin  = skey + (size_t)n1 * 8;                // the sorted keys
    off   = wmin + (size_t)(RC_THREADS_MAX / 64) * 8;  // a minimum per wave
    part  = off + ((size_t)1 << q) * 4;           // the bucket counts, then starts, then ends
    bins  = part + (size_t)RC_THREADS_MAX * 4;    // the scan's partial sums
    cols  = bins + (size_t)(n + 1) * 4;
    sr1   = cols + (size_t)RC_ELL_MAX * 4;
    slots = pad16(sr1 + (size_t)n1 * 2);          // r1 < 8192 in 16 bits
    total = slots + (list ? 16 : 0);              // the list's slot counter of path 0, only where a list is asked for
  }
};

// the most a workgroup asks for: 128 KiB and a little, which leaves room for the kernel's own static LDS (the votes of a barrier)
const size_t RC_LDS_MAX = RcCarve((int)RS_K_MAX, (int)RS_N_MAX, (int)RC_N1_MAX, 13, true).total;

struct RcArgs {
  const word *G, *V;    // V may be NULL; G too where no row is read (t1 = t2 = 0)
  const int32_t *cols;  // NULL: columns 0 .. ell-1
  int64_t g_stride, g_bs, v_bs, c_bs;
  int k, k1, k2, t1, t2, n, width;  // width = words(n) >= 1
  int ell, q;                       // q bucket bits
  word mask;                        // of a row's last word
  int w_min;                        // at most n + 1
  int n1;                           // 1 <= N1 <= 8192
  int64_t n2;                       // N2 >= 1
  int atomic;                       // path 1
  int64_t slices, slice_len;        // path 1: workgroups per member and right sums per workgroup
  int64_t *hist, *lightest;
  int64_t u0;                       // this launch: workgroups from u0 on
  int w_max;                        // the list: at most n
  int64_t *list, *count;            // list may be NULL at cap = 0
  int64_t l_bs, cap;
};

// the key of the set of rank `rest` among the sets of t of the rows base .. base + kk - 1
__device__ __forceinline__ word set_key(const word *rowkey, unsigned long long rest, int t, int kk, int base) {
  word key = 0;
  int e    = kk;
  for (int m = t; m >= 1; --m) {
    e = unrank_step(rest, m, e);
    key ^= rowkey[base + e];
  }
  return key;
}

// c ^= the rows of that set
__device__ __forceinline__ void add_set_rows(word (&c)[RC_WT], const word *g, int64_t stride, int width, word mask, unsigned long long rest, int t,
                                             int kk, int base) {
  int e = kk;
  for (int m = t; m >= 1; --m) {
    e             = unrank_step(rest, m, e);
    const word *r = g + (int64_t)(base + e) * stride;
#pragma unroll
    for (int w = 0; w < RC_WT; ++w)
      if (w < width) c[w] ^= w == width - 1 ? r[w] & mask : r[w];
  }
}

template <bool HIST, bool LIGHT, bool LIST>
__global__ __launch_bounds__(RC_THREADS_MAX) void rc_kernel(RcArgs p) {
  extern __shared__ __align__(16) word rc_lds[];
  const int tid = threadIdx.x, T = blockDim.x, lane = tid & 63, wave = tid >> 6;
  const int64_t u  = p.u0 + blockIdx.x;
  const int64_t b  = p.atomic ? u / p.slices : u;
  const int64_t sl = p.atomic ? u - b * p.slices : 0;
  const RcCarve at(p.k, p.n, p.n1, p.q, LIST);
  unsigned char *lds = reinterpret_cast<unsigned char *>(rc_lds);
  word *rowkey       = rc_lds;
  word *skey         = reinterpret_cast<word *>(lds + at.skey);
  word *wmin         = reinterpret_cast<word *>(lds + at.wmin);
  uint32_t *off      = reinterpret_cast<uint32_t *>(lds + at.off);
  uint32_t *part     = reinterpret_cast<uint32_t *>(lds + at.part);
  uint32_t *bins     = reinterpret_cast<uint32_t *>(lds + at.bins);
  int32_t *wcols     = reinterpret_cast<int32_t *>(lds + at.cols);
  uint16_t *sr1      = reinterpret_cast<uint16_t *>(lds + at.sr1);
  uint32_t *slots    = reinterpret_cast<uint32_t *>(lds + at.slots);  // LIST, path 0
  const int k = p.k, n = p.n, n1 = p.n1, nb = 1 << p.q;
  const word *g = p.G && p.t1 + p.t2 > 0 ? p.G + b * p.g_bs : nullptr;  // without rows in the sums G is not read at all
  const word *v = p.V ? p.V + b * p.v_bs : nullptr;

  // 1. the window, checked; nothing outside the member is read
  int bad = 0;
  if (tid < p.ell) {
    const int c = p.cols ? p.cols[b * p.c_bs + tid] : tid;
    bad         = c < 0 || c >= n;
    wcols[tid]  = bad ? 0 : c;
  }
  if (__syncthreads_or(bad)) {  // refused: path 1 leaves the answer to the initialisation kernel
    if (!p.atomic) {
      if (HIST)
        for (int w = tid; w <= n; w += T) p.hist[b * ((int64_t)n + 1) + w] = -1;
      if (LIGHT && tid == 0) p.lightest[b] = -2;
      if (LIST && tid == 0) p.count[b] = -1;
    }
    return;
  }
  // the keys of the rows and of V
  for (int i = tid; i <= k; i += T) {
    const word *r = i < k ? (g ? g + (int64_t)i * p.g_stride : nullptr) : v;
    word key      = 0;
    if (r)
      for (int j = 0; j < p.ell; ++j) {
        const int c = wcols[j];
        key |= ((r[c >> 6] >> (c & 63)) & 1) << j;
      }
    rowkey[i] = key;
  }
  for (int i = tid; i < nb; i += T) off[i] = 0;
  if (HIST)
    for (int i = tid; i <= n; i += T) bins[i] = 0;
  if (LIST && tid == 0) slots[0] = 0;
  __syncthreads();

  // 2. the left table: count, scan, scatter
  const word qmask = (word)nb - 1;
  for (int r1 = tid; r1 < n1; r1 += T) atomicAdd(&off[(uint32_t)(set_key(rowkey, (unsigned long long)r1, p.t1, p.k1, 0) & qmask)], 1u);
  __syncthreads();
  const int chunk = (nb + T - 1) / T, c0 = tid * chunk < nb ? tid * chunk : nb, c1 = c0 + chunk < nb ? c0 + chunk : nb;
  {
    uint32_t s = 0;
    for (int i = c0; i < c1; ++i) s += off[i];
    part[tid] = s;
  }
  __syncthreads();
  if (wave == 0) {  // the exclusive scan of the T partial sums: T / 64 per lane, then across the lanes
    const int per = T >> 6;
    uint32_t s    = 0;
    for (int j = 0; j < per; ++j) s += part[lane * per + j];
    uint32_t incl = s;
    for (int o = 1; o < 64; o <<= 1) {
      const uint32_t x = __shfl_up(incl, o);
      if (lane >= o) incl += x;
    }
    uint32_t run = incl - s;
    for (int j = 0; j < per; ++j) {
      const uint32_t x     = part[lane * per + j];
      part[lane * per + j] = run;
      run += x;
    }
  }
  __syncthreads();
  {
    uint32_t run = part[tid];
    for (int i = c0; i < c1; ++i) {
      const uint32_t x = off[i];
      off[i]           = run;  // the bucket's start
      run += x;
    }
  }
  __syncthreads();
  for (int r1 = tid; r1 < n1; r1 += T) {
    const word key     = set_key(rowkey, (unsigned long long)r1, p.t1, p.k1, 0);
    const uint32_t pos = atomicAdd(&off[(uint32_t)(key & qmask)], 1u);  // pos < n1: the counts sum to n1
    skey[pos]          = key;
    sr1[pos]           = (uint16_t)r1;
  }
  __syncthreads();  // off[i] is now the END of bucket i, the start of bucket i + 1

  // 3. the right walk
  const int64_t s0 = sl * p.slice_len;
  const int64_t s1 = p.atomic ? (s0 + p.slice_len < p.n2 ? s0 + p.slice_len : p.n2) : p.n2;
  const word vkey  = rowkey[k];
  unsigned long long best = ~0ull;  // the lane's lightest: none
  for (int64_t r2 = s0 + tid; r2 < s1; r2 += T) {
    const word key2      = vkey ^ set_key(rowkey, (unsigned long long)r2, p.t2, p.k2, p.k1);
    const uint32_t bkt   = (uint32_t)(key2 & qmask);
    const uint32_t j_end = off[bkt];
    for (uint32_t j = bkt ? off[bkt - 1] : 0; j < j_end; ++j) {
      if (skey[j] != key2) continue;
      const uint32_t r1 = sr1[j];
      word c[RC_WT];
#pragma unroll
      for (int w = 0; w < RC_WT; ++w) {
        c[w] = 0;
        if (v && w < p.width) c[w] = w == p.width - 1 ? v[w] & p.mask : v[w];
      }
      add_set_rows(c, g, p.g_stride, p.width, p.mask, (unsigned long long)r1, p.t1, p.k1, 0);
      add_set_rows(c, g, p.g_stride, p.width, p.mask, (unsigned long long)r2, p.t2, p.k2, p.k1);
      int wt = 0;
#pragma unroll
      for (int w = 0; w < RC_WT; ++w) wt += __popcll(c[w]);
      if (HIST) atomicAdd(&bins[wt], 1u);
      if (LIGHT && wt >= p.w_min) {
        const unsigned long long cand = ((unsigned long long)(uint32_t)wt << 40) | ((unsigned long long)r1 * (unsigned long long)p.n2 + (unsigned long long)r2);
        best                          = cand < best ? cand : best;
      }
      if (LIST && wt >= p.w_min && wt <= p.w_max) {  // a slot each, taken whether or not it is below cap: the count is the true total
        const unsigned long long slot = p.atomic ? atomicAdd(reinterpret_cast<unsigned long long *>(p.count + b), 1ull) : (unsigned long long)atomicAdd(slots, 1u);
        if (slot < (unsigned long long)p.cap)
          p.list[b * p.l_bs + (int64_t)slot] = (int64_t)(((unsigned long long)(uint32_t)wt << 40) | ((unsigned long long)r1 * (unsigned long long)p.n2 + (unsigned long long)r2));
      }
    }
  }

  // 4. the outputs
  if (LIGHT) {
    for (int o = 32; o; o >>= 1) {
      const unsigned long long x = __shfl_xor(best, o);
      best                       = x < best ? x : best;
    }
    if (lane == 0) wmin[wave] = best;
  }
  __syncthreads();
  if (LIGHT && tid == 0) {
    for (int i = 1; i < (T >> 6); ++i) best = wmin[i] < best ? wmin[i] : best;
    if (!p.atomic) p.lightest[b] = (int64_t)best;
    else if (best != ~0ull) atomicMin(reinterpret_cast<unsigned long long *>(p.lightest + b), best);
  }
  if (LIST && !p.atomic && tid == 0) p.count[b] = (int64_t)slots[0];  // after the barrier above: every slot is taken
  if (HIST) {
    int64_t *h = p.hist + b * ((int64_t)n + 1);
    for (int w = tid; w <= n; w += T) {
      const uint32_t s = bins[w];
      if (!p.atomic) h[w] = (int64_t)s;
      else if (s) atomicAdd(reinterpret_cast<unsigned long long *>(h + w), (unsigned long long)s);
    }
  }
}

struct RcInit {
  int64_t *hist, *lightest;
  int64_t b0;              // this launch: members from b0 on, a workgroup each
  int n, ell;
  const int32_t *cols;
  int64_t c_bs;
  int64_t hist0, light_v;  // hist[b][0] = hist0, the other entries 0; lightest[b] = light_v
  int64_t *list, *count;   // the list's part: count[b] = count_v, and list[b * l_bs + i] = i (weight 0, rank i) for i < min(count_v, cap):
  int64_t l_bs, cap, count_v;  // count_v > 0 only for members without columns, whose pairs all weigh 0
};

// What path 1's atomics start from, the whole result of members without pairs or columns, and the refused form wherever it runs.
__global__ __launch_bounds__(BATCH_WAVE_THREADS) void rc_init_kernel(RcInit p) {
  const int tid   = threadIdx.x;
  const int64_t b = p.b0 + blockIdx.x;
  int bad         = 0;
  if (p.cols && tid < p.ell) {
    const int c = p.cols[b * p.c_bs + tid];
    bad         = c < 0 || c >= p.n;
  }
  bad = __syncthreads_or(bad);
  if (p.hist)
    for (int w = tid; w <= p.n; w += BATCH_WAVE_THREADS) p.hist[b * ((int64_t)p.n + 1) + w] = bad ? -1 : w == 0 ? p.hist0 : 0;
  if (p.lightest && tid == 0) p.lightest[b] = bad ? -2 : p.light_v;
  if (p.count) {
    if (tid == 0) p.count[b] = bad ? -1 : p.count_v;
    const int64_t m = bad ? 0 : p.count_v < p.cap ? p.count_v : p.cap;
    for (int64_t i = tid; i < m; i += BATCH_WAVE_THREADS) p.list[b * p.l_bs + i] = i;
  }
}

int launch_init(hipStream_t st, RcInit p, int64_t batch) {
  return launch_chunked(batch, BATCH_CHUNK, [&](int64_t b0, int64_t nb) {
    p.b0 = b0;
    hipLaunchKernelGGL(rc_init_kernel, dim3((unsigned)nb), dim3(BATCH_WAVE_THREADS), 0, st, p);
  });
}

// the path-0 bound of this call: RC_P0 unless the variable is set; clamped to [-1, RC_P0_MAX], -1 = no path 0
int64_t env_p0() {
  const char *s = getenv("M4RI_AMD_ROW_SUMS_COLLIDE_PATH0_MAX");
  if (!s || !*s) return RC_P0;
  const int64_t v = atoll(s);
  return v < -1 ? -1 : v > RC_P0_MAX ? RC_P0_MAX : v;
}

bool sizes_negative(int64_t k, int64_t n, int64_t k1, int64_t t1, int64_t t2, int64_t ell) {
  return k < 0 || n < 0 || k1 < 0 || k1 > k || t1 < 0 || t2 < 0 || ell < 0;
}

int plan(int64_t k, int64_t n, int64_t k1, int64_t t1, int64_t t2, int64_t ell, int64_t p0) {
  if (sizes_negative(k, n, k1, t1, t2, ell)) return -1;
  const __int128 pairs = (__int128)binom_capped(k1, t1) * binom_capped(k - k1, t2);
  if (n == 0 || pairs == 0) return 0;  // the initialisation kernel alone
  return pairs <= p0 ? 0 : 1;
}

// path 1: the right sums of a workgroup, for N1, N2 >= 1
int64_t slice_len(int64_t n1, int64_t n2, int64_t batch) {
  const int64_t want = batch >= RC_BLOCKS_MIN ? 1 : (RC_BLOCKS_MIN + batch - 1) / (batch > 0 ? batch : 1);
  int64_t len        = (n2 + want - 1) / want;
  if (len < n1) len = n1;
  if (len < RC_SLICE_MIN) len = RC_SLICE_MIN;
  if (len > RC_P0_MAX / n1) len = RC_P0_MAX / n1;  // at least 2^19 > N1: slice * N1 < 2^32
  return len;
}

template <bool LIST>
void launch_walk(bool hist, bool light, dim3 grid, dim3 block, size_t lds, hipStream_t st, const RcArgs &p) {
  if (hist && light) hipLaunchKernelGGL((rc_kernel<true, true, LIST>), grid, block, lds, st, p);
  else if (hist) hipLaunchKernelGGL((rc_kernel<true, false, LIST>), grid, block, lds, st, p);
  else if (light) hipLaunchKernelGGL((rc_kernel<false, true, LIST>), grid, block, lds, st, p);
  else if constexpr (LIST) hipLaunchKernelGGL((rc_kernel<false, false, true>), grid, block, lds, st, p);  // the list alone
}

// Both entry points.  Without count (and then without list) this is m4ri_amd_row_sums_collide_batch_dev as it always was: the same
// checks in the same order, the same kernels.
int collide(const word *G, int64_t g_stride, int64_t g_bs, int64_t k, int64_t n, const word *V, int64_t v_bs, int64_t batch, int64_t k1, int64_t t1,
            int64_t t2, const int32_t *cols, int64_t c_bs, int64_t ell, int64_t w_min, int64_t w_max, int64_t *hist, int64_t *lightest, int64_t *list,
            int64_t l_bs, int64_t cap, int64_t *count, void *stream) {
  hipStream_t st = (hipStream_t)stream;
  if (sizes_negative(k, n, k1, t1, t2, ell) || batch < 0 || g_stride < 0 || g_bs < 0 || v_bs < 0 || c_bs < 0 || w_min < 0 || w_max < 0 || cap < 0 ||
      l_bs < 0)
    return (int)hipErrorInvalidValue;
  if (k > RS_K_MAX || n > RS_N_MAX || t1 > RS_T_MAX || t2 > RS_T_MAX || ell > RC_ELL_MAX) return (int)hipErrorNotSupported;
  const int64_t n1 = binom_capped(k1, t1), n2 = binom_capped(k - k1, t2);
  if (n1 > RC_N1_MAX) return (int)hipErrorNotSupported;
  const int64_t pairs = n1 * n2;  // at most 2^13 * 2^41
  if (pairs > RS_SUMS_MAX) return (int)hipErrorNotSupported;
  if (!cols && ell > n) return (int)hipErrorInvalidValue;
  if (!hist && !lightest && !count) return (int)hipErrorInvalidValue;
  if ((list && !count) || (count && !list && cap > 0)) return (int)hipErrorInvalidValue;  // they come together; a count alone at cap = 0
  if (count && batch > 1 && l_bs < cap) return (int)hipErrorInvalidValue;
  const int64_t width = words_of(n);
  const bool words    = k > 0 && n > 0;                      // G has words
  const bool walked   = pairs > 0 && n > 0 && t1 + t2 >= 1;  // and they are read
  if (n > 0 && k > 1 && g_stride < width) return (int)hipErrorInvalidValue;
  if (batch > 0) {
    if (walked && !G) return (int)hipErrorInvalidValue;
    const bool listed = count && list && cap > 0;
    const void *outs[4]      = {hist, lightest, count, listed ? list : nullptr};
    const uintptr_t bytes[4] = {(uintptr_t)(batch * (n + 1)) * 8, (uintptr_t)batch * 8, (uintptr_t)batch * 8,
                                ((uintptr_t)(batch - 1) * (uintptr_t)l_bs + (uintptr_t)cap) * 8};
    for (int o = 0; o < 4; ++o) {
      if (!outs[o]) continue;
      for (int o2 = o + 1; o2 < 4; ++o2)
        if (outs[o2] && spans_meet(outs[o], bytes[o], outs[o2], bytes[o2])) return (int)hipErrorInvalidValue;
      if (words && G && spans_meet(outs[o], bytes[o], G, member_span_bytes(batch, g_bs, k, g_stride, width))) return (int)hipErrorInvalidValue;
      if (V && n > 0 && spans_meet(outs[o], bytes[o], V, member_span_bytes(batch, v_bs, 1, 0, width))) return (int)hipErrorInvalidValue;
      if (cols && ell > 0 && spans_meet(outs[o], bytes[o], cols, (uintptr_t)((batch - 1) * c_bs + ell) * 4)) return (int)hipErrorInvalidValue;
    }
  }
  if (batch == 0) return 0;
  RcInit in{};
  in.hist = hist, in.lightest = lightest, in.n = (int)n, in.ell = (int)ell, in.cols = cols, in.c_bs = c_bs, in.light_v = -1;
  in.list = list, in.count = count, in.l_bs = l_bs, in.cap = cap;
  if (n == 0 || pairs == 0) {  // every word weighs 0: all pairs in the one bin, the lightest is rank 0 if weight 0 qualifies; or no pairs
    in.hist0 = pairs, in.light_v = pairs > 0 && w_min == 0 ? 0 : -1;  // n = 0 with a window given: every entry is outside, all refused
    in.count_v = w_min == 0 ? pairs : 0;                              // weight 0 is in the band iff w_min = 0: w_max >= 0
    return launch_init(st, in, batch);
  }
  RcArgs p{};
  p.G = G, p.V = V, p.cols = cols, p.g_stride = g_stride, p.g_bs = g_bs, p.v_bs = v_bs, p.c_bs = c_bs;
  p.k = (int)k, p.k1 = (int)k1, p.k2 = (int)(k - k1), p.t1 = (int)t1, p.t2 = (int)t2, p.n = (int)n, p.width = (int)width, p.ell = (int)ell;
  p.mask = tail_mask((int)(n & 63)), p.w_min = (int)(w_min > n + 1 ? n + 1 : w_min), p.n1 = (int)n1, p.n2 = n2;
  p.hist = hist, p.lightest = lightest;
  p.w_max = (int)(w_max > n ? n : w_max), p.list = list, p.count = count, p.l_bs = l_bs, p.cap = cap;
  while (p.q < ell && ((int64_t)1 << p.q) < n1) ++p.q;
  p.atomic    = plan(k, n, k1, t1, t2, ell, env_p0());
  p.slice_len = p.atomic ? slice_len(n1, n2, batch) : n2;
  p.slices    = (n2 + p.slice_len - 1) / p.slice_len;
  static std::once_flag once;
  static hipError_t attr = hipSuccess;
  std::call_once(once, [] {
    const void *kernels[] = {reinterpret_cast<const void *>(rc_kernel<true, true, false>), reinterpret_cast<const void *>(rc_kernel<true, false, false>),
                             reinterpret_cast<const void *>(rc_kernel<false, true, false>), reinterpret_cast<const void *>(rc_kernel<true, true, true>),
                             reinterpret_cast<const void *>(rc_kernel<true, false, true>), reinterpret_cast<const void *>(rc_kernel<false, true, true>),
                             reinterpret_cast<const void *>(rc_kernel<false, false, true>)};
    for (const void *f : kernels)
      if (attr == hipSuccess) attr = hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, (int)RC_LDS_MAX);
  });
  HIPTRY(attr);
  const size_t lds  = RcCarve((int)k, (int)n, (int)n1, p.q, count != nullptr).total;
  const int threads = n1 <= 1024 && p.slice_len <= 4096 ? BATCH_WAVE_THREADS : RC_THREADS_MAX;
  if (p.atomic) HIPTRY(launch_init(st, in, batch));
  return launch_chunked(batch * p.slices, BATCH_CHUNK, [&](int64_t u0, int64_t nu) {
    p.u0 = u0;
    const dim3 grid((unsigned)nu), block((unsigned)threads);
    if (count) launch_walk<true>(hist != nullptr, lightest != nullptr, grid, block, lds, st, p);
    else launch_walk<false>(hist != nullptr, lightest != nullptr, grid, block, lds, st, p);
  });
}

}  // namespace

extern "C" {

int m4ri_amd_plan_row_sums_collide_batch(int64_t k, int64_t n, int64_t k1, int64_t t1, int64_t t2, int64_t ell) {
  return plan(k, n, k1, t1, t2, ell, RC_P0);
}

int64_t m4ri_amd_row_sums_collide_slices(int64_t k, int64_t n, int64_t k1, int64_t t1, int64_t t2, int64_t ell, int64_t batch) {
  if (sizes_negative(k, n, k1, t1, t2, ell) || batch < 0) return -1;
  const int64_t n1 = binom_capped(k1, t1), n2 = binom_capped(k - k1, t2);
  if (n == 0 || n1 == 0 || n2 == 0 || n1 > RC_N1_MAX) return 0;
  const int64_t len = slice_len(n1, n2, batch);
  return (n2 + len - 1) / len;
}

int m4ri_amd_row_sums_collide_batch_dev(const word *G, int64_t g_stride, int64_t g_bs, int64_t k, int64_t n, const word *V, int64_t v_bs, int64_t batch,
                                        int64_t k1, int64_t t1, int64_t t2, const int32_t *cols, int64_t c_bs, int64_t ell, int64_t w_min,
                                        int64_t *hist, int64_t *lightest, void *stream) {
  return collide(G, g_stride, g_bs, k, n, V, v_bs, batch, k1, t1, t2, cols, c_bs, ell, w_min, 0, hist, lightest, nullptr, 0, 0, nullptr, stream);
}

int m4ri_amd_row_sums_collide_list_batch_dev(const word *G, int64_t g_stride, int64_t g_bs, int64_t k, int64_t n, const word *V, int64_t v_bs,
                                             int64_t batch, int64_t k1, int64_t t1, int64_t t2, const int32_t *cols, int64_t c_bs, int64_t ell,
                                             int64_t w_min, int64_t w_max, int64_t *hist, int64_t *lightest, int64_t *list, int64_t l_bs, int64_t cap,
                                             int64_t *count, void *stream) {
  return collide(G, g_stride, g_bs, k, n, V, v_bs, batch, k1, t1, t2, cols, c_bs, ell, w_min, w_max, hist, lightest, list, l_bs, cap, count, stream);
}

}  // extern "C"
