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
//      table, so a slice is never shorter than N1 (or JOIN_SLICE_MIN) unless the list is, and slice * N1 < 2^32.  The outputs are set by an
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
//
// The table's scan, what happens to a match, the output step, the initialisation kernel, the LDS carve and the host
// side of the launch are join_common.h's, shared with lists_collide_batch.hip.  What is here: the row keys, the keys of the sets, the
// word and the rank of a match, the slices, and the routing.
#include <hip/hip_runtime.h>
#include "join_common.h"
#include "subset_rank.h"
#include "../../include/m4ri_amd.h"

namespace {

constexpr int64_t RC_N1_MAX = 8192;  // the left table of one workgroup: C(128, 2) = 8128 fits, C(129, 2) = 8256 does not
// Path 0 up to this many pairs per member.  Measured (tools/bench_row_sums_collide.py, profiles/row_sums_collide_bench.txt)
// on a ladder of N2 = C(k2, 2) against N1 = C(64, 2) = 2016 at n = 256, ell = 16, both outputs, about 2^32 pairs per call, the spreads of
// these rows under 1 %: path 0 is ahead of path 1 by 3 % at 241 920 ... 4 064 256 pairs per member (what the initialisation launch
// costs: the right list is one slice there), by 13 %, 2 % and 1 % at 8 255 520, 16 386 048 and 33 205 536 (k2 = 182; 129 members), each
// time by more than the spread, and loses from 65 802 240 on (k2 = 256, 65 members: 0.60x; 0.15x at 263 725 056: a workgroup per member
// no longer fills the device, sixteen slices per member do): P0 = 33 205 536 = C(64, 2) * C(182, 2).  The join looks at every right sum
// once, not at every pair: at these sizes a call is 0.1 ms, and what the bound decides is small either way.
// M4RI_AMD_ROW_SUMS_COLLIDE_PATH0_MAX overrides it for the routing of a call.
constexpr int64_t RC_P0 = 33205536;  // the largest bound is JOIN_PAIRS_WG

// the LDS of a workgroup: the row keys first, k + 1 words with V's last, then the table of N1 entries (r1 < 8192 in 16 bits)
__host__ __device__ inline JoinCarve rc_carve(int k, int n, int n1, int q, bool list) { return JoinCarve((size_t)(k + 1) * 8, n1, n, q, list); }

// the most a workgroup asks for: 128 KiB and a little, which leaves room for the kernel's own static LDS (the votes of a barrier)
const size_t RC_LDS_MAX = rc_carve((int)RS_K_MAX, (int)RS_N_MAX, (int)RC_N1_MAX, 13, true).total;

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
__device__ __forceinline__ void add_set_rows(word (&c)[JOIN_WT], const word *g, int64_t stride, int width, word mask, unsigned long long rest, int t,
                                             int kk, int base) {
  int e = kk;
  for (int m = t; m >= 1; --m) {
    e             = unrank_step(rest, m, e);
    const word *r = g + (int64_t)(base + e) * stride;
#pragma unroll
    for (int w = 0; w < JOIN_WT; ++w)
      if (w < width) c[w] ^= w == width - 1 ? r[w] & mask : r[w];
  }
}

template <bool HIST, bool LIGHT, bool LIST>
__global__ __launch_bounds__(JOIN_THREADS_MAX) void rc_kernel(RcArgs p) {
  extern __shared__ __align__(16) word rc_lds[];
  const int tid = threadIdx.x, T = blockDim.x;
  const int64_t u  = p.u0 + blockIdx.x;
  const int64_t b  = p.atomic ? u / p.slices : u;
  const int64_t sl = p.atomic ? u - b * p.slices : 0;
  const JoinOut o{p.hist, p.lightest, p.list, p.count, p.l_bs, p.cap, p.n, p.w_min, p.w_max, p.atomic};
  const JoinLds L(rc_lds, rc_carve(p.k, p.n, p.n1, p.q, LIST));
  word *rowkey = rc_lds;
  const int k = p.k, n1 = p.n1, nb = 1 << p.q;
  const word *g = p.G && p.t1 + p.t2 > 0 ? p.G + b * p.g_bs : nullptr;  // without rows in the sums G is not read at all
  const word *v = p.V ? p.V + b * p.v_bs : nullptr;

  // 1. the window, then the keys of the rows and of V
  if (join_window(L.cols, p.cols, b * p.c_bs, p.ell, p.n, tid)) {
    join_refuse<HIST, LIGHT, LIST>(o, b, tid, T);
    return;
  }
  for (int i = tid; i <= k; i += T) {
    const word *r = i < k ? (g ? g + (int64_t)i * p.g_stride : nullptr) : v;
    word key      = 0;
    if (r)
      for (int j = 0; j < p.ell; ++j) {
        const int c = L.cols[j];
        key |= ((r[c >> 6] >> (c & 63)) & 1) << j;
      }
    rowkey[i] = key;
  }
  join_clear<HIST, LIST>(L, nb, p.n, tid, T);
  __syncthreads();

  // 2. the left table: count, scan, scatter; the keys are made twice
  const word qmask = (word)nb - 1;
  for (int r1 = tid; r1 < n1; r1 += T) atomicAdd(&L.off[(uint32_t)(set_key(rowkey, (unsigned long long)r1, p.t1, p.k1, 0) & qmask)], 1u);
  join_starts(L, nb, tid, T);
  for (int r1 = tid; r1 < n1; r1 += T) {
    const word key     = set_key(rowkey, (unsigned long long)r1, p.t1, p.k1, 0);
    const uint32_t pos = atomicAdd(&L.off[(uint32_t)(key & qmask)], 1u);  // pos < n1: the counts sum to n1
    L.skey[pos]        = key;
    L.sidx[pos]        = (uint16_t)r1;
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
    const uint32_t e_end = L.off[bkt];
    for (uint32_t e = bkt ? L.off[bkt - 1] : 0; e < e_end; ++e) {  // as in lc_kernel; a shared walk taking the match as a callable cost 1-2 VGPRs
      if (L.skey[e] != key2) continue;
      const uint32_t r1 = L.sidx[e];
      word c[JOIN_WT];
#pragma unroll
      for (int w = 0; w < JOIN_WT; ++w) {
        c[w] = 0;
        if (v && w < p.width) c[w] = w == p.width - 1 ? v[w] & p.mask : v[w];
      }
      add_set_rows(c, g, p.g_stride, p.width, p.mask, (unsigned long long)r1, p.t1, p.k1, 0);
      add_set_rows(c, g, p.g_stride, p.width, p.mask, (unsigned long long)r2, p.t2, p.k2, p.k1);
      int wt = 0;
#pragma unroll
      for (int w = 0; w < JOIN_WT; ++w) wt += __popcll(c[w]);
      join_report<HIST, LIGHT, LIST>(o, L, b, wt, (unsigned long long)r1 * (unsigned long long)p.n2 + (unsigned long long)r2, best);
    }
  }

  // 4. the outputs
  join_output<HIST, LIGHT, LIST>(o, L, b, best, tid, T);
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
  const int64_t want = join_slices_wanted(batch);
  const int64_t len = (n2 + want - 1) / want, floor = join_slice_floor(n1);
  return join_slice_held(len < floor ? floor : len, n1);  // slice * N1 < 2^32
}

JoinKernels<RcArgs> rc_kernels = {{{nullptr, rc_kernel<false, true, false>}, {rc_kernel<true, false, false>, rc_kernel<true, true, false>}},
                                  {{rc_kernel<false, false, true>, rc_kernel<false, true, true>}, {rc_kernel<true, false, true>, rc_kernel<true, true, true>}}};

// Both entry points.  Without count (and then without list) this is m4ri_amd_row_sums_collide_batch_dev as it always was: the same
// checks in the same order, the same kernels.
int collide(const word *G, int64_t g_stride, int64_t g_bs, int64_t k, int64_t n, const word *V, int64_t v_bs, int64_t batch, int64_t k1, int64_t t1,
            int64_t t2, const int32_t *cols, int64_t c_bs, int64_t ell, int64_t w_min, int64_t w_max, int64_t *hist, int64_t *lightest, int64_t *list,
            int64_t l_bs, int64_t cap, int64_t *count, void *stream) {
  hipStream_t st = (hipStream_t)stream;
  if (sizes_negative(k, n, k1, t1, t2, ell) || batch < 0 || g_stride < 0 || g_bs < 0 || v_bs < 0 || c_bs < 0 || w_min < 0 || w_max < 0 || cap < 0 ||
      l_bs < 0)
    return (int)hipErrorInvalidValue;
  if (k > RS_K_MAX || n > RS_N_MAX || t1 > RS_T_MAX || t2 > RS_T_MAX || ell > JOIN_ELL_MAX) return (int)hipErrorNotSupported;
  const int64_t n1 = binom_capped(k1, t1), n2 = binom_capped(k - k1, t2);
  if (n1 > RC_N1_MAX) return (int)hipErrorNotSupported;
  const int64_t pairs = n1 * n2;  // at most 2^13 * 2^41
  if (pairs > RS_SUMS_MAX) return (int)hipErrorNotSupported;
  if (const int e = join_check_outputs(cols, ell, n, hist, lightest, list, l_bs, cap, count, batch)) return e;
  const int64_t width = width_of(n);
  const bool walked   = pairs > 0 && n > 0 && t1 + t2 >= 1;  // G's words are read
  if (n > 0 && k > 1 && g_stride < width) return (int)hipErrorInvalidValue;
  if (batch > 0) {
    if (walked && !G) return (int)hipErrorInvalidValue;
    if (join_outputs_meet(hist, lightest, list, l_bs, cap, count, batch, n, cols, c_bs, ell, rows_span(G, batch, g_bs, k, g_stride, width),
                          rows_span(V, batch, v_bs, 1, 0, width)))
      return (int)hipErrorInvalidValue;
  }
  if (batch == 0) return 0;
  const JoinInit in = join_init_of(hist, lightest, list, l_bs, cap, count, n, cols, c_bs, ell);
  if (n == 0 || pairs == 0) return join_launch_init(st, join_unwalked(in, pairs, w_min), batch);
  RcArgs p{};
  p.G = G, p.V = V, p.cols = cols, p.g_stride = g_stride, p.g_bs = g_bs, p.v_bs = v_bs, p.c_bs = c_bs;
  p.k = (int)k, p.k1 = (int)k1, p.k2 = (int)(k - k1), p.t1 = (int)t1, p.t2 = (int)t2, p.n = (int)n, p.width = (int)width, p.ell = (int)ell;
  p.mask = tail_mask((int)(n & 63)), p.w_min = join_w_min(w_min, n), p.n1 = (int)n1, p.n2 = n2;
  p.hist = hist, p.lightest = lightest;
  p.w_max = join_w_max(w_max, n), p.list = list, p.count = count, p.l_bs = l_bs, p.cap = cap;
  p.q         = join_bucket_bits(ell, n1);
  p.atomic    = plan(k, n, k1, t1, t2, ell, env_bound("M4RI_AMD_ROW_SUMS_COLLIDE_PATH0_MAX", RC_P0, -1, JOIN_PAIRS_WG));  // -1: no path 0
  p.slice_len = p.atomic ? slice_len(n1, n2, batch) : n2;
  p.slices    = (n2 + p.slice_len - 1) / p.slice_len;
  return join_launch(rc_kernels, RC_LDS_MAX, st, in, batch, p, batch * p.slices, join_threads(n1, 1024, p.slice_len),
                     rc_carve((int)k, (int)n, (int)n1, p.q, count != nullptr).total);
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
