// join_common.h -- what the joins on a window of bits share (rowsums_collide_batch.hip: the sums of t1 and of t2 rows of a generator;
// lists_collide_batch.hip: two explicit lists of rows) and what the calls that write out the words behind listed keys share
// (rowsums_words_batch.hip, lists_collide_batch.hip).  Everything here is internal to the file that includes it (an unnamed namespace,
// as in batch_common.h); the kernels stay in their files: where a key comes from, how a match's word is formed and what its rank is, and
// how the work is cut differ, and are all that is left there.
//
// The join of one workgroup.  The LEFT entries (key, 16-bit index), at most 8192, are counting-sorted in LDS on the key's low q bits,
// q = ceil(log2 entries) held at ell: the kernel counts into off[] with LDS atomics, join_starts() turns the counts into bucket starts,
// the kernel scatters with a second round of atomics, after which off[i] is the END of bucket i and the start of bucket i + 1.  A lane
// per RIGHT key then compares the FULL key of every entry of bucket key2 mod 2^q (five lines, left in the kernels), weighs the word
// of a match and reports it (join_report): a 32-bit bin in LDS, the lane's minimum of (wt << 40) | rank, and a list slot.
// join_output() reduces the minima and reads the bins out.  On path 0 a workgroup owns its member and writes every output entry once
// with plain stores, the refused form included, and list slots come from a counter in LDS; on path 1 (`atomic`) the initialisation
// kernel sets the outputs and answers the refused members, and the workgroups combine with 64-bit integer atomics: one minimum, one add
// per non-zero bin, one returning add per listed pair.
#pragma once
#include <hip/hip_runtime.h>
#include <limits.h>
#include "batch_common.h"
#include "subset_rank.h"  // RS_N_MAX, RS_SUMS_MAX: the limits of a word and of a rank, which every call of the family has

namespace {

constexpr int64_t JOIN_ELL_MAX    = 64;                      // a key is one 64-bit word
constexpr int JOIN_WT             = 16;                      // register words of a weighed word: n <= RS_N_MAX = 1024
constexpr int64_t JOIN_PAIRS_WG   = ((int64_t)1 << 32) - 1;  // left entries * right keys of a workgroup: its 32-bit bins hold
constexpr int64_t JOIN_BLOCKS_MIN = 1024;                    // the right lists are cut until the call has this many workgroups ...
constexpr int64_t JOIN_SLICE_MIN  = 256;                     // ... but no slice shorter than this, or than the left table
constexpr int JOIN_THREADS_MAX    = BATCH_MAX_THREADS;

// ---- the outputs and the LDS of a workgroup -----------------------------------------------------------------------------------------------

// what a join writes; made inside each kernel from its own arguments
struct JoinOut {
  int64_t *hist, *lightest, *list, *count;  // list may be NULL at cap = 0
  int64_t l_bs, cap;
  int n, w_min, w_max;  // w_min at most n + 1, w_max at most n
  int atomic;           // path 1
};

// where the pieces of a workgroup's LDS are, in bytes; the same arithmetic on both sides of the launch.  front: what the kernel keeps
// before the table (a multiple of 8); rows: the most left entries; list: the slot counter of path 0, only where a list is asked for
struct JoinCarve {
  size_t skey, wmin, off, part, bins, cols, sidx, slots, total;
  __host__ __device__ JoinCarve(size_t front, int rows, int n, int q, bool list) {
    skey  = front;                                         // the sorted keys
    wmin  = skey + (size_t)rows * 8;                       // a minimum per wave
    off   = wmin + (size_t)(JOIN_THREADS_MAX / 64) * 8;    // the bucket counts, then starts, then ends
    part  = off + ((size_t)1 << q) * 4;                    // the scan's partial sums
    bins  = part + (size_t)JOIN_THREADS_MAX * 4;
    cols  = bins + (size_t)(n + 1) * 4;
    sidx  = cols + (size_t)JOIN_ELL_MAX * 4;               // the left index behind each sorted key, 16 bits
    slots = pad16(sidx + (size_t)rows * 2);
    total = slots + (list ? 16 : 0);
  }
};

struct JoinLds {
  word *skey, *wmin;
  uint32_t *off, *part, *bins;
  int32_t *cols;
  uint16_t *sidx;
  uint32_t *slots;  // LIST, path 0
  __device__ __forceinline__ JoinLds(word *base, const JoinCarve &at) {
    unsigned char *lds = reinterpret_cast<unsigned char *>(base);
    skey  = reinterpret_cast<word *>(lds + at.skey);
    wmin  = reinterpret_cast<word *>(lds + at.wmin);
    off   = reinterpret_cast<uint32_t *>(lds + at.off);
    part  = reinterpret_cast<uint32_t *>(lds + at.part);
    bins  = reinterpret_cast<uint32_t *>(lds + at.bins);
    cols  = reinterpret_cast<int32_t *>(lds + at.cols);
    sidx  = reinterpret_cast<uint16_t *>(lds + at.sidx);
    slots = reinterpret_cast<uint32_t *>(lds + at.slots);
  }
};

// ---- the device pieces of a join ----------------------------------------------------------------------------------------------------------

// The window of member b (cols = NULL: the columns 0 .. ell-1), range-checked into LDS; nothing outside the member is read.  True (for
// the whole workgroup) if an entry is outside [0, n): the member is refused.
__device__ __forceinline__ bool join_window(int32_t *wcols, const int32_t *cols, int64_t c_off, int ell, int n, int tid) {
  int bad = 0;
  if (tid < ell) {
    const int c = cols ? cols[c_off + tid] : tid;
    bad         = c < 0 || c >= n;
    wcols[tid]  = bad ? 0 : c;
  }
  return __syncthreads_or(bad);
}

// the refused form: path 1 leaves the answer to the initialisation kernel
template <bool HIST, bool LIGHT, bool LIST>
__device__ __forceinline__ void join_refuse(const JoinOut &o, int64_t b, int tid, int T) {
  if (o.atomic) return;
  if (HIST)
    for (int w = tid; w <= o.n; w += T) o.hist[b * ((int64_t)o.n + 1) + w] = -1;
  if (LIGHT && tid == 0) o.lightest[b] = -2;
  if (LIST && tid == 0) o.count[b] = -1;
}

// the bucket counts, the bins and the slot counter to zero.  The caller's barrier follows.
template <bool HIST, bool LIST>
__device__ __forceinline__ void join_clear(const JoinLds &L, int nb, int n, int tid, int T) {
  for (int i = tid; i < nb; i += T) L.off[i] = 0;
  if (HIST)
    for (int i = tid; i <= n; i += T) L.bins[i] = 0;
  if (LIST && tid == 0) L.slots[0] = 0;
}

// off[0 .. nb-1] from the counts of the buckets to their starts, barriers before and after: a segment of ceil(nb / T) buckets per
// thread, the exclusive scan of the T segment sums in wave 0 (T / 64 per lane, then across the lanes).
__device__ __forceinline__ void join_starts(const JoinLds &L, int nb, int tid, int T) {
  uint32_t *off = L.off, *part = L.part;
  const int lane = tid & 63, wave = tid >> 6;
  __syncthreads();
  const int seg = (nb + T - 1) / T, c0 = tid * seg < nb ? tid * seg : nb, c1 = c0 + seg < nb ? c0 + seg : nb;
  {
    uint32_t s = 0;
    for (int i = c0; i < c1; ++i) s += off[i];
    part[tid] = s;
  }
  __syncthreads();
  if (wave == 0) {
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
}

// A match of weight wt and pair rank `rank`: its bin, the lane's minimum `best`, and within the band a list slot, taken whether or not
// it is below cap (the count is the true total).  The slot comes from LDS on path 0 (a workgroup's pairs are below 2^32) and from one
// returning 64-bit atomic on count[b] on path 1.  (Forming the rank in here, inside the branches, from the two indices was tried: it
// brought rc_kernel's text closer to what it was before the pieces were shared and made its calls 0.5 - 1.5 % slower.)
template <bool HIST, bool LIGHT, bool LIST>
__device__ __forceinline__ void join_report(const JoinOut &o, const JoinLds &L, int64_t b, int wt, unsigned long long rank, unsigned long long &best) {
  const unsigned long long cand = ((unsigned long long)(uint32_t)wt << 40) | rank;
  if (HIST) atomicAdd(&L.bins[wt], 1u);
  if (LIGHT && wt >= o.w_min) best = cand < best ? cand : best;
  if (LIST && wt >= o.w_min && wt <= o.w_max) {
    const unsigned long long slot = o.atomic ? atomicAdd(reinterpret_cast<unsigned long long *>(o.count + b), 1ull) : (unsigned long long)atomicAdd(L.slots, 1u);
    if (slot < (unsigned long long)o.cap) o.list[b * o.l_bs + (int64_t)slot] = (int64_t)cand;
  }
}

// the outputs of the workgroup: the lanes' minima reduced by shuffles and through LDS, the count, the bins
template <bool HIST, bool LIGHT, bool LIST>
__device__ __forceinline__ void join_output(const JoinOut &o, const JoinLds &L, int64_t b, unsigned long long best, int tid, int T) {
  const int lane = tid & 63, wave = tid >> 6;
  if (LIGHT) {
    for (int s = 32; s; s >>= 1) {
      const unsigned long long x = __shfl_xor(best, s);
      best                       = x < best ? x : best;
    }
    if (lane == 0) L.wmin[wave] = best;
  }
  __syncthreads();
  if (LIGHT && tid == 0) {
    for (int i = 1; i < (T >> 6); ++i) best = L.wmin[i] < best ? L.wmin[i] : best;
    if (!o.atomic) o.lightest[b] = (int64_t)best;
    else if (best != ~0ull) atomicMin(reinterpret_cast<unsigned long long *>(o.lightest + b), best);
  }
  if (LIST && !o.atomic && tid == 0) o.count[b] = (int64_t)L.slots[0];  // after the barrier above: every slot is taken
  if (HIST) {
    int64_t *h = o.hist + b * ((int64_t)o.n + 1);
    for (int w = tid; w <= o.n; w += T) {
      const uint32_t s = L.bins[w];
      if (!o.atomic) h[w] = (int64_t)s;
      else if (s) atomicAdd(reinterpret_cast<unsigned long long *>(h + w), (unsigned long long)s);
    }
  }
}

// ---- the initialisation kernel ------------------------------------------------------------------------------------------------------------

struct JoinInit {
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
// Kernel and launcher are templates on the workgroup's size only so that rowsums_words_batch.hip, which includes this header for the
// words alone, gets no copy of the kernel.
template <int THREADS>
__global__ __launch_bounds__(THREADS) void join_init_kernel(JoinInit p) {
  const int tid   = threadIdx.x;
  const int64_t b = p.b0 + blockIdx.x;
  int bad         = 0;
  if (p.cols && tid < p.ell) {
    const int c = p.cols[b * p.c_bs + tid];
    bad         = c < 0 || c >= p.n;
  }
  bad = __syncthreads_or(bad);
  if (p.hist)
    for (int w = tid; w <= p.n; w += THREADS) p.hist[b * ((int64_t)p.n + 1) + w] = bad ? -1 : w == 0 ? p.hist0 : 0;
  if (p.lightest && tid == 0) p.lightest[b] = bad ? -2 : p.light_v;
  if (p.count) {
    if (tid == 0) p.count[b] = bad ? -1 : p.count_v;
    const int64_t m = bad ? 0 : p.count_v < p.cap ? p.count_v : p.cap;
    for (int64_t i = tid; i < m; i += THREADS) p.list[b * p.l_bs + i] = i;
  }
}

template <int THREADS = BATCH_WAVE_THREADS>
int join_launch_init(hipStream_t st, JoinInit p, int64_t batch) {
  return launch_members(batch, [&](dim3 grid, int64_t b0) {
    p.b0 = b0;
    hipLaunchKernelGGL(join_init_kernel<THREADS>, grid, dim3(THREADS), 0, st, p);
  });
}

// ---- the host side of a join --------------------------------------------------------------------------------------------------------------

// the rules of the window and of the outputs that come after the limits of a call
inline int join_check_outputs(const int32_t *cols, int64_t ell, int64_t n, const int64_t *hist, const int64_t *lightest, const int64_t *list, int64_t l_bs,
                              int64_t cap, const int64_t *count, int64_t batch) {
  if (!cols && ell > n) return (int)hipErrorInvalidValue;
  if (!hist && !lightest && !count) return (int)hipErrorInvalidValue;
  if ((list && !count) || (count && !list && cap > 0)) return (int)hipErrorInvalidValue;  // they come together; a count alone at cap = 0
  if (count && batch > 1 && l_bs < cap) return (int)hipErrorInvalidValue;
  return 0;
}

// do the four outputs (batch > 0) meet each other or an operand?  The window is an operand of every join.
inline bool join_outputs_meet(int64_t *hist, int64_t *lightest, int64_t *list, int64_t l_bs, int64_t cap, int64_t *count, int64_t batch, int64_t n,
                              const int32_t *cols, int64_t c_bs, int64_t ell, Span a, Span b, Span c = {0, 0}) {
  return spans_meet_any({entries_span(hist, batch, n + 1, n + 1, 8), entries_span(lightest, batch, 1, 1, 8), entries_span(count, batch, 1, 1, 8),
                         entries_span(count ? list : nullptr, batch, l_bs, cap, 8)},
                        {a, b, c, entries_span(cols, batch, c_bs, ell, 4)});
}

// the initialisation of a call; hist0, light_v and count_v as path 1's atomics need them
inline JoinInit join_init_of(int64_t *hist, int64_t *lightest, int64_t *list, int64_t l_bs, int64_t cap, int64_t *count, int64_t n, const int32_t *cols,
                             int64_t c_bs, int64_t ell) {
  JoinInit in{};
  in.hist = hist, in.lightest = lightest, in.n = (int)n, in.ell = (int)ell, in.cols = cols, in.c_bs = c_bs, in.light_v = -1;
  in.list = list, in.count = count, in.l_bs = l_bs, in.cap = cap;
  return in;
}

// The initialisation that is the whole answer of a call that walks nothing (no columns, or no pairs).  Every word weighs 0: all pairs in
// the one bin, the lightest is rank 0 if weight 0 qualifies; or no pairs.  n = 0 with a window given: every entry is outside, all refused.
inline JoinInit join_unwalked(JoinInit in, int64_t pairs, int64_t w_min) {
  in.hist0 = pairs, in.light_v = pairs > 0 && w_min == 0 ? 0 : -1;
  in.count_v = w_min == 0 ? pairs : 0;  // weight 0 is in the band iff w_min = 0: w_max >= 0
  return in;
}

inline int join_w_min(int64_t w_min, int64_t n) { return (int)(w_min > n + 1 ? n + 1 : w_min); }
inline int join_w_max(int64_t w_max, int64_t n) { return (int)(w_max > n ? n : w_max); }

// the bucket bits of a table of `left` entries: ceil(log2 left), held at ell
inline int join_bucket_bits(int64_t ell, int64_t left) {
  int q = 0;
  while (q < ell && ((int64_t)1 << q) < left) ++q;
  return q;
}

// The cut of the right lists.  A call that has `have` workgroups before the cut wants each right list in this many slices ...
inline int64_t join_slices_wanted(int64_t have) { return have >= JOIN_BLOCKS_MIN ? 1 : (JOIN_BLOCKS_MIN + have - 1) / (have > 0 ? have : 1); }
// ... none shorter than the left table of `left` >= 1 entries or than JOIN_SLICE_MIN ...
inline int64_t join_slice_floor(int64_t left) { return left > JOIN_SLICE_MIN ? left : JOIN_SLICE_MIN; }
// ... and none so long that the workgroup's pairs leave 32 bits: the bound is at least 2^19, above the floor
inline int64_t join_slice_held(int64_t len, int64_t left) { return len > JOIN_PAIRS_WG / left ? JOIN_PAIRS_WG / left : len; }

// 256 threads where they hold the left table (left_256: the most entries they do) and the slice is short, 1024 otherwise
inline int join_threads(int64_t left, int64_t left_256, int64_t slice_len) {
  return left <= left_256 && slice_len <= 4096 ? BATCH_WAVE_THREADS : JOIN_THREADS_MAX;
}

// The instantiations of a join kernel, at [LIST][HIST][LIGHT]; [0][0][0] is NULL, a call has an output.
template <typename Args>
using JoinKernel = void (*)(Args);
template <typename Args>
using JoinKernels = const JoinKernel<Args>[2][2][2];

// Launches the join: once per process the most dynamic LDS for every instantiation, on path 1 the initialisation kernel, then `units`
// workgroups of `threads` threads with `lds` bytes, BATCH_CHUNK per launch.
template <typename Args>
int join_launch(JoinKernels<Args> &kernels, size_t lds_max, hipStream_t st, const JoinInit &in, int64_t batch, Args &p, int64_t units, int threads,
                size_t lds) {
  // once per Args, not per table: a second table of kernels with the same argument struct would need a Site of its own
  HIPTRY(set_max_dynamic_lds(lds_max, kernels[0][0][1], kernels[0][1][0], kernels[0][1][1], kernels[1][0][0], kernels[1][0][1], kernels[1][1][0], kernels[1][1][1]));
  if (p.atomic) HIPTRY(join_launch_init(st, in, batch));
  const JoinKernel<Args> kernel = kernels[p.count != nullptr][p.hist != nullptr][p.lightest != nullptr];
  return launch_members(units, [&](dim3 grid, int64_t u0) {
    p.u0 = u0;
    hipLaunchKernelGGL(kernel, grid, dim3((unsigned)threads), lds, st, p);
  });
}

// ---- the words behind listed keys -----------------------------------------------------------------------------------------------------------

constexpr int JOIN_WORDS_ROWS = BATCH_WAVE_THREADS;  // output rows per workgroup, a thread each in the first phase

// what the words calls share of their arguments
struct JoinWords {
  const int64_t *keys, *count;
  word *W;
  int32_t *skipped;
  int64_t l_bs, cap, w_stride, w_bs;
  int width, group;  // group: lanes per output row, a power of two >= width, 1 where n = 0
  word mask;
  int64_t pairs;     // 0: no key is valid
  int64_t chunks;    // workgroups per member: ceil(cap / JOIN_WORDS_ROWS)
  int64_t u0;        // this launch: workgroups from u0 on
};

// The kernel of a words call, JOIN_WORDS_ROWS output rows per workgroup, two phases around one barrier.  A thread per output row reads
// its key and checks it (key < 0 or rank >= pairs: the row is skipped, no row index is formed from it); split(rank, rows[tid]) turns
// a valid rank ONCE into the indices of the rows behind it.  Then the lanes regroup: `group` lanes per output row, 64 / group rows
// of a wave at a time, lane w of a group on word w, which is word_of(b, rows[lr], w); consecutive words are read and written, the last
// one under the mask, the bits behind it kept.  The member's row count min(max(count[b], 0), cap) is read on the device (count may
// come from a call still in flight on the stream); workgroups beyond it return at once.  skipped[b] is added to by the waves that meet
// a bad key, one atomic per such wave.
template <typename Index, int IDX, typename Split, typename WordOf>
__device__ __forceinline__ void join_words(const JoinWords &p, Index (&rows)[JOIN_WORDS_ROWS][IDX], uint8_t (&live)[JOIN_WORDS_ROWS], Split split,
                                           WordOf word_of) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t u = p.u0 + blockIdx.x, b = u / p.chunks, i0 = (u - b * p.chunks) * JOIN_WORDS_ROWS;
  int64_t m = p.cap;
  if (p.count) {
    const int64_t c = p.count[b];
    m               = c < 0 ? 0 : c < m ? c : m;
  }
  if (i0 >= m) return;  // the whole workgroup
  // 1. a key each
  const int64_t i = i0 + tid;
  int ok = 0, bad = 0;
  if (i < m) {
    const int64_t key          = p.keys[b * p.l_bs + i];
    const unsigned long long r = (unsigned long long)key & (((unsigned long long)1 << 40) - 1);
    bad                        = key < 0 || r >= (unsigned long long)p.pairs;
    ok                         = !bad;
    if (ok) split(r, rows[tid]);
  }
  live[tid] = (uint8_t)ok;
  if (p.skipped) {
    const word votes = __ballot(bad);
    if (votes && lane == 0) atomicAdd(p.skipped + b, __popcll(votes));
  }
  __syncthreads();
  // 2. a group of lanes per output row
  if (p.width == 0) return;
  const int g = p.group, w = lane & (g - 1), per = 64 / g;
  if (w >= p.width) return;
  word *out = p.W + b * p.w_bs;
  for (int pass = 0; pass < g; ++pass) {
    const int lr = wave * 64 + pass * per + (lane >> __builtin_ctz(g));
    if (!live[lr]) continue;
    store_masked(out + (i0 + lr) * p.w_stride + w, word_of(b, rows[lr], w), w == p.width - 1, p.mask);
  }
}

// The checks of a words call that follow its limits and its operands' strides.  missing: a row operand that is read is NULL.
inline int join_words_check(int64_t n, int64_t batch, const int64_t *keys, int64_t l_bs, int64_t cap, const int64_t *count, const word *W, int64_t w_stride,
                            int64_t w_bs, const int32_t *skipped, bool missing, Span a, Span b, Span c = {0, 0}) {
  const int64_t width = width_of(n);
  if (cap > 1 && w_stride < width) return (int)hipErrorInvalidValue;
  if (batch > 1 && cap > 0 && (l_bs < cap || (n > 0 && !members_fit(batch, w_bs, cap, w_stride, width)))) return (int)hipErrorInvalidValue;
  if (batch > 0 && cap > 0) {
    if (!keys || (n > 0 && !W) || missing) return (int)hipErrorInvalidValue;
    if (spans_meet_any({rows_span(W, batch, w_bs, cap, w_stride, width), entries_span(skipped, batch, 1, 1, 4)},
                       {a, b, c, entries_span(keys, batch, l_bs, cap, 8), entries_span(count, batch, 1, 1, 8)}))
      return (int)hipErrorInvalidValue;
  }
  return 0;
}

// Launches a words kernel whose arguments hold a JoinWords `o`; `pairs` = 0 where no key is valid.  skipped is written whole by a memset
// on the stream: 0 for a clean member, and at cap = 0.
template <typename Args>
int join_words_launch(void (*kernel)(Args), Args &p, int64_t n, int64_t batch, const int64_t *keys, int64_t l_bs, int64_t cap, const int64_t *count, word *W,
                      int64_t w_stride, int64_t w_bs, int32_t *skipped, int64_t pairs, hipStream_t st) {
  if (batch == 0) return 0;
  if (skipped) HIPTRY(hipMemsetAsync(skipped, 0, (size_t)batch * 4, st));
  if (cap == 0) return 0;
  JoinWords &o = p.o;
  o.keys = keys, o.count = count, o.W = W, o.skipped = skipped, o.l_bs = l_bs, o.cap = cap, o.w_stride = w_stride, o.w_bs = w_bs;
  o.width = (int)width_of(n), o.group = 1;
  while (o.group < o.width) o.group <<= 1;
  o.mask = tail_mask((int)(n & 63)), o.pairs = pairs;
  o.chunks = (cap + JOIN_WORDS_ROWS - 1) / JOIN_WORDS_ROWS;
  if (batch > INT64_MAX / o.chunks) return (int)hipErrorInvalidValue;
  return launch_members(batch * o.chunks, [&](dim3 grid, int64_t u0) {
    o.u0 = u0;
    hipLaunchKernelGGL(kernel, grid, dim3(JOIN_WORDS_ROWS), 0, st, p);
  });
}

}  // namespace
