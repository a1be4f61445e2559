// sort_rows_batch.hip -- the rows of a list of words sorted and deduplicated, one call for a batch, every result left on the device: the
// relational operator that belongs beside the joins (lists_collide_batch.hip) and the words calls that project their results.  Between two
// joins a level list of Wagner's k-tree or of MMT / BJMM wants its duplicates removed and a defined order; this call gives both in the
// key format m4ri_amd_lists_words_batch_dev reads, so the deduplicated sorted list is written by that call (Y one zero row, ny = 1).
//
// Member b has a list X_b (nx rows of n bits, of which the first m_b = min(max(xcount[b], 0), nx) count) and a window cols_b of ell <= 64
// columns.  THE ORDER: row i goes before row j iff (key_i, w_i[0], ..., w_i[words-1], i) is lexicographically smaller than the same tuple
// of j; key = the window bits as an unsigned 64-bit number (bit t = column cols[t]), w = the row's words as unsigned numbers, the last one
// under the mask of the valid bits.  The index makes the order total, so the result is ONE permutation, whatever network produces it:
// that is what lets the device sort only the next power of two of m_b and skip every stretch of sentinels, and why no atomics are needed.
//
// An ENTRY is (key, index), 8 + 4 bytes.  The comparator reads rows from global memory only where two keys are equal.  An absent entry
// (a SENTINEL) carries an index >= m_b, its position, and compares by that index alone: after every row, never through its key, since at
// ell = 64 every key value is a real one.
//
// Path 0 (nx <= SR_CHUNK = 8192), sr_wg_kernel, one workgroup per member: the window range-checked into LDS (a refused member's ucount
// is -1, nothing else of it is written), the keys gathered once, a bitonic network in LDS over Pm = the next power of two of m_b, then the
// class heads (key differs from the predecessor's, or the rows do), a scan in the workgroup, and order, uniq, mult and ucount written
// with plain stores.
// Path 1 (SR_CHUNK < nx <= 2^24), the entries in the caller's scratch, the grids sized by P = the next power of two of nx on the host,
// m_b read on the device:
//   sr_chunk_kernel (first)   a workgroup per chunk of SR_CHUNK entries: window, keys, the network's levels k = 2 .. SR_CHUNK in LDS; the
//                             workgroup of chunk 0 leaves m_b (or -1: refused) in the scratch for the launches that follow
//   for k = 2 SR_CHUNK .. P   sr_global_kernel once per stride j = k/2 .. SR_CHUNK: one compare-exchange per thread in global memory;
//                             sr_chunk_kernel (merge) once: the strides SR_CHUNK/2 .. 1 of level k in LDS
//   sr_heads_kernel           a flag per entry and a count per block of 1024 entries
//   sr_scan_kernel            one workgroup per member: the block counts to block starts, ucount
//   sr_scatter_kernel         order, uniq, and the position of each class head (over the keys, which are done with)
//   sr_mult_kernel            mult from the head positions
// Workgroups whose entries lie at or beyond Pm, and levels k > Pm, return at once: the network on Pm entries is a complete sort.
// Plain launches on the caller's stream: no allocation, no copy to the host, no synchronisation, no engine workspace or lock.
#include <hip/hip_runtime.h>
#include "join_common.h"
#include "../../include/m4ri_amd.h"

namespace {

constexpr int64_t SR_ROWS_MAX = (int64_t)1 << 24;  // nx: the index fits the low 24 bits of a key of the words calls
constexpr int64_t SR_CHUNK    = 8192;              // entries of a workgroup's LDS: 96 KiB of the 160
constexpr int SR_THREADS      = JOIN_THREADS_MAX;  // of the chunk kernels
constexpr int SR_BLOCK        = 1024;              // entries per workgroup of the heads, scatter and mult kernels, a thread each
constexpr int SR_PAIR_THREADS = 256;               // of the global compare-exchange, a pair each
static_assert(SR_CHUNK >= 2 * SR_THREADS && (SR_CHUNK & (SR_CHUNK - 1)) == 0 && SR_CHUNK % SR_BLOCK == 0 && SR_BLOCK == SR_THREADS, "the chunk");

// the LDS of a workgroup that holds `entries` entries (a power of two, at least 2)
struct SrCarve {
  size_t idx, cols, wsum, total;
  __host__ __device__ SrCarve(int64_t entries) {
    idx   = (size_t)entries * 8;                     // behind the keys
    cols  = pad16(idx + (size_t)entries * 4);
    wsum  = cols + (size_t)JOIN_ELL_MAX * 4;         // the scan's sums, one per wave
    total = wsum + (size_t)(SR_THREADS / 64) * 4;
  }
};

const size_t SR_LDS_MAX = SrCarve(SR_CHUNK).total;

struct SrArgs {
  const word *X;
  const int64_t *xcount;  // NULL: nx rows
  const int32_t *cols;    // NULL: columns 0 .. ell-1
  int64_t x_stride, x_bs, c_bs, nx, l_bs;
  int n, width, ell;
  word mask, fmask;       // of a row's last word; of the key where cols = NULL
  int64_t *order, *ucount, *uniq, *mult;
  // path 1: the scratch, P entries per member
  word *skey;
  uint32_t *sidx, *sblk;  // sblk: P / SR_BLOCK counts per member, then starts
  int32_t *smeta;         // m_b, or -1 for a refused member
  uint8_t *shead;
  int64_t P;              // the padded length: path 0 the entries of the LDS, path 1 of a member's scratch
  uint32_t k, j;          // the level and the stride of this launch
  int first;              // sr_chunk_kernel: the keys are gathered here
  int64_t per;            // workgroups per member of this launch
  int64_t u0;             // this launch: workgroups from u0 on
};

// the rows of a member that count
__device__ __forceinline__ uint32_t sr_rows(const SrArgs &p, int64_t b) {
  int64_t m = p.nx;
  if (p.xcount) {
    const int64_t c = p.xcount[b];
    m               = c < 0 ? 0 : c < m ? c : m;
  }
  return (uint32_t)m;
}

__device__ __forceinline__ uint32_t sr_pow2(uint32_t m) {  // the entries of the network: the next power of two, 1 for no row
  uint32_t P = 1;
  while (P < m) P <<= 1;
  return P;
}

// the ell window bits of row r as one word: lists_collide_batch.hip's gather, which lives in that file with its kernel
__device__ __forceinline__ word sr_window_key(const word *r, const int32_t *wcols, int ell, bool first, word fmask) {
  if (first) return ell ? r[0] & fmask : 0;
  word key = 0, x = 0;
  int cur  = -1;
  for (int j = 0; j < ell; ++j) {
    const int c = wcols[j], wi = c >> 6;
    if (wi != cur) {
      cur = wi;
      x   = r[wi];
    }
    key |= ((x >> (c & 63)) & 1) << j;
  }
  return key;
}

// the rows of a member as the comparator reads them
struct SrRows {
  const word *x;
  int64_t stride;
  int width;
  word mask;
  uint32_t m;
};

// -1, 0, 1: rows ia and ib (both < m) by their words as unsigned numbers, the last one under the mask
__device__ __forceinline__ int sr_rows_cmp(const SrRows &R, uint32_t ia, uint32_t ib) {
  const word *ra = R.x + (int64_t)ia * R.stride, *rb = R.x + (int64_t)ib * R.stride;
  for (int w = 0; w < R.width; ++w) {
    word a = ra[w], c = rb[w];
    if (w == R.width - 1) a &= R.mask, c &= R.mask;
    if (a != c) return a < c ? -1 : 1;
  }
  return 0;
}

// does entry a go before entry b?  Never both ways, and one way for a != b: the order is total.
__device__ __forceinline__ bool sr_before(const SrRows &R, word ka, uint32_t ia, word kb, uint32_t ib) {
  if (ia >= R.m || ib >= R.m) return ia < ib;  // a sentinel: by its index, behind every row
  if (ka != kb) return ka < kb;
  const int c = sr_rows_cmp(R, ia, ib);
  return c ? c < 0 : ia < ib;
}

// The levels k_lo .. k_hi of the bitonic network on the cnt entries (a power of two) in LDS, whose first stands at position `base` of
// the member's network: of each level the strides min(k / 2, cnt / 2) .. 1.  A barrier in front of every step and one behind the last.
// (The strides below 64 across the lanes of a wave, an entry per lane and __shfl_xor on key and index, the levels up to 64 in one
// residence -- 37 barriers for 8192 entries where this has 92 -- were built and measured against this form: 12 ... 36 % slower on every
// shape, DESIGN 3.14.  A shuffle of 12 bytes is three trips through the LDS crossbar, and only the lower lane of a pair compares.)
__device__ __forceinline__ void sr_lds_steps(word *key, uint32_t *idx, uint32_t cnt, uint32_t base, uint32_t k_lo, uint32_t k_hi, const SrRows &R, int tid,
                                             int T) {
  for (uint32_t k = k_lo; k <= k_hi; k <<= 1)
    for (uint32_t j = (k >> 1) < (cnt >> 1) ? (k >> 1) : (cnt >> 1); j > 0; j >>= 1) {
      __syncthreads();
      for (uint32_t t = tid; t < (cnt >> 1); t += T) {
        const uint32_t i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), l = i | j;
        const bool up    = ((base + i) & k) == 0;
        const word ki = key[i], kl = key[l];
        const uint32_t ii = idx[i], il = idx[l];
        if (sr_before(R, kl, il, ki, ii) == up) {
          key[i] = kl, key[l] = ki;
          idx[i] = il, idx[l] = ii;
        }
      }
    }
  __syncthreads();
}

// the exclusive scan of v over the workgroup's threads and its total; barriers inside, wsum free again behind them
__device__ __forceinline__ uint32_t sr_block_scan(uint32_t v, uint32_t *wsum, int tid, int T, uint32_t &total) {
  const int lane = tid & 63, wave = tid >> 6;
  uint32_t incl = v;
  for (int o = 1; o < 64; o <<= 1) {
    const uint32_t x = __shfl_up(incl, o);
    if (lane >= o) incl += x;
  }
  if (lane == 63) wsum[wave] = incl;
  __syncthreads();
  uint32_t before = 0, all = 0;
  for (int i = 0; i < (T >> 6); ++i) {
    const uint32_t s = wsum[i];
    if (i < wave) before += s;
    all += s;
  }
  __syncthreads();
  total = all;
  return before + incl - v;
}

// is the entry at a position > 0 (below m) the head of a class?  Its key or its row differs from the predecessor's.
__device__ __forceinline__ bool sr_head(const SrRows &R, word k, uint32_t i, word k_prev, uint32_t i_prev) { return k != k_prev || sr_rows_cmp(R, i, i_prev) != 0; }

__device__ __forceinline__ SrRows sr_rows_of(const SrArgs &p, int64_t b, uint32_t m) { return SrRows{p.X + b * p.x_bs, p.x_stride, p.width, p.mask, m}; }

// ---- path 0 ---------------------------------------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(SR_THREADS) void sr_wg_kernel(SrArgs p) {
  extern __shared__ __align__(16) word sr_lds[];
  const int tid = threadIdx.x, T = blockDim.x;
  const int64_t b = p.u0 + blockIdx.x;
  const SrCarve at(p.P);
  unsigned char *lds = reinterpret_cast<unsigned char *>(sr_lds);
  word *key          = sr_lds;
  uint32_t *idx      = reinterpret_cast<uint32_t *>(lds + at.idx);
  int32_t *wcols     = reinterpret_cast<int32_t *>(lds + at.cols);
  uint32_t *wsum     = reinterpret_cast<uint32_t *>(lds + at.wsum);

  // 1. the window
  if (join_window(wcols, p.cols, b * p.c_bs, p.ell, p.n, tid)) {
    if (tid == 0 && p.ucount) p.ucount[b] = -1;
    return;
  }
  const uint32_t m  = sr_rows(p, b);
  const uint32_t Pm = sr_pow2(m);  // at most P: m <= nx
  const SrRows R    = sr_rows_of(p, b, m);
  const bool first  = p.cols == nullptr;

  // 2. the entries, then the network
  for (uint32_t i = tid; i < Pm; i += T) {
    key[i] = i < m ? sr_window_key(R.x + (int64_t)i * R.stride, wcols, p.ell, first, p.fmask) : 0;
    idx[i] = i;
  }
  sr_lds_steps(key, idx, Pm, 0, 2, Pm, R, tid, T);

  // 3. the outputs
  const int64_t out = b * p.l_bs;
  if (p.order)
    for (uint32_t i = tid; i < m; i += T) p.order[out + i] = (int64_t)idx[i];
  if (!p.ucount) return;
  const uint32_t E = Pm > (uint32_t)T ? Pm / (uint32_t)T : 1;  // positions tid * E .. tid * E + E - 1 are this thread's; E <= 8
  uint32_t heads = 0, cnt = 0;
  for (uint32_t e = 0; e < E; ++e) {
    const uint32_t pos = (uint32_t)tid * E + e;
    if (pos < m && (pos == 0 || sr_head(R, key[pos], idx[pos], key[pos - 1], idx[pos - 1]))) heads |= 1u << e, ++cnt;
  }
  uint32_t total;
  uint32_t q = sr_block_scan(cnt, wsum, tid, T, total);  // its barriers: nobody reads a key from here on
  if (tid == 0) p.ucount[b] = (int64_t)total;
  if (!p.uniq) return;
  uint32_t *hpos = reinterpret_cast<uint32_t *>(key);  // the position of each head, over the keys
  for (uint32_t e = 0; e < E; ++e)
    if ((heads >> e) & 1) {
      const uint32_t pos = (uint32_t)tid * E + e;
      p.uniq[out + q]    = (int64_t)idx[pos];
      hpos[q]            = pos;
      ++q;
    }
  if (!p.mult) return;
  __syncthreads();
  for (uint32_t c = tid; c < total; c += T) p.mult[out + c] = (int64_t)((c + 1 < total ? hpos[c + 1] : m) - hpos[c]);
}

// ---- path 1 ---------------------------------------------------------------------------------------------------------------------------------

// first: the window, the keys of a chunk and the levels 2 .. SR_CHUNK; otherwise the strides below SR_CHUNK of level k
__global__ __launch_bounds__(SR_THREADS) void sr_chunk_kernel(SrArgs p) {
  extern __shared__ __align__(16) word sr_lds[];
  const int tid = threadIdx.x, T = blockDim.x;
  const int64_t u = p.u0 + blockIdx.x, b = u / p.per, c = u - b * p.per;
  const SrCarve at(SR_CHUNK);
  unsigned char *lds = reinterpret_cast<unsigned char *>(sr_lds);
  word *key          = sr_lds;
  uint32_t *idx      = reinterpret_cast<uint32_t *>(lds + at.idx);
  int32_t *wcols     = reinterpret_cast<int32_t *>(lds + at.cols);
  uint32_t m;
  if (p.first) {
    const bool bad = join_window(wcols, p.cols, b * p.c_bs, p.ell, p.n, tid);
    m              = sr_rows(p, b);
    if (c == 0 && tid == 0) {
      p.smeta[b] = bad ? -1 : (int32_t)m;
      if (bad && p.ucount) p.ucount[b] = -1;
    }
    if (bad) return;
  } else {
    const int32_t mm = p.smeta[b];
    if (mm < 0) return;
    m = (uint32_t)mm;
  }
  const uint32_t Pm = sr_pow2(m), base = (uint32_t)(c * SR_CHUNK);
  if (base >= Pm || (!p.first && p.k > Pm)) return;  // the whole workgroup
  const uint32_t cnt = Pm < (uint32_t)SR_CHUNK ? Pm : (uint32_t)SR_CHUNK;
  const SrRows R     = sr_rows_of(p, b, m);
  word *gkey         = p.skey + b * p.P + base;
  uint32_t *gidx     = p.sidx + b * p.P + base;
  if (p.first) {
    const bool nocols = p.cols == nullptr;
    for (uint32_t i = tid; i < cnt; i += T) {
      const uint32_t pos = base + i;
      key[i] = pos < m ? sr_window_key(R.x + (int64_t)pos * R.stride, wcols, p.ell, nocols, p.fmask) : 0;
      idx[i] = pos;
    }
  } else {
    for (uint32_t i = tid; i < cnt; i += T) key[i] = gkey[i], idx[i] = gidx[i];
  }
  sr_lds_steps(key, idx, cnt, base, p.first ? 2 : p.k, p.first ? cnt : p.k, R, tid, T);
  for (uint32_t i = tid; i < cnt; i += T) gkey[i] = key[i], gidx[i] = idx[i];
}

// stride j >= SR_CHUNK of level k: a compare-exchange per thread
__global__ __launch_bounds__(SR_PAIR_THREADS) void sr_global_kernel(SrArgs p) {
  const int64_t u = p.u0 + blockIdx.x, b = u / p.per, c = u - b * p.per;
  const int32_t mm = p.smeta[b];
  if (mm < 0) return;
  const uint32_t m = (uint32_t)mm, Pm = sr_pow2(m);
  if (p.k > Pm) return;
  const uint32_t t = (uint32_t)(c * SR_PAIR_THREADS) + threadIdx.x, j = p.j;
  const uint32_t i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), l = i | j;  // below P
  if (i >= Pm) return;                                                  // l < Pm with it: j < k <= Pm
  const SrRows R = sr_rows_of(p, b, m);
  word *gkey     = p.skey + b * p.P;
  uint32_t *gidx = p.sidx + b * p.P;
  const bool up  = (i & p.k) == 0;
  const word ki = gkey[i], kl = gkey[l];
  const uint32_t ii = gidx[i], il = gidx[l];
  if (sr_before(R, kl, il, ki, ii) == up) {
    gkey[i] = kl, gkey[l] = ki;
    gidx[i] = il, gidx[l] = ii;
  }
}

// the class heads of SR_BLOCK sorted entries and their number
__global__ __launch_bounds__(SR_BLOCK) void sr_heads_kernel(SrArgs p) {
  const int64_t u = p.u0 + blockIdx.x, b = u / p.per, c = u - b * p.per;
  const int32_t mm = p.smeta[b];
  if (mm < 0 || c * SR_BLOCK >= mm) return;  // the whole workgroup; the scan reads the blocks below m only
  const uint32_t m = (uint32_t)mm, pos = (uint32_t)(c * SR_BLOCK) + threadIdx.x;
  const SrRows R       = sr_rows_of(p, b, m);
  const word *gkey     = p.skey + b * p.P;
  const uint32_t *gidx = p.sidx + b * p.P;
  int head = 0;
  if (pos < m) {
    head                 = pos == 0 || sr_head(R, gkey[pos], gidx[pos], gkey[pos - 1], gidx[pos - 1]);
    p.shead[b * p.P + pos] = (uint8_t)head;
  }
  const int cnt = __syncthreads_count(head);
  if (threadIdx.x == 0) p.sblk[b * (p.P / SR_BLOCK) + c] = (uint32_t)cnt;
}

// a workgroup per member: the counts of its blocks to their starts, and ucount
__global__ __launch_bounds__(SR_THREADS) void sr_scan_kernel(SrArgs p) {
  __shared__ uint32_t wsum[SR_THREADS / 64];
  const int tid = threadIdx.x;
  const int64_t b = p.u0 + blockIdx.x;
  const int32_t mm = p.smeta[b];
  if (mm < 0) return;
  uint32_t *blk = p.sblk + b * (p.P / SR_BLOCK);
  const int nb = (mm + SR_BLOCK - 1) / SR_BLOCK, seg = (nb + SR_THREADS - 1) / SR_THREADS;
  const int c0 = tid * seg < nb ? tid * seg : nb, c1 = c0 + seg < nb ? c0 + seg : nb;
  uint32_t s = 0;
  for (int i = c0; i < c1; ++i) s += blk[i];
  uint32_t total;
  uint32_t run = sr_block_scan(s, wsum, tid, SR_THREADS, total);
  for (int i = c0; i < c1; ++i) {
    const uint32_t x = blk[i];
    blk[i]           = run;
    run += x;
  }
  if (tid == 0) p.ucount[b] = (int64_t)total;
}

// order and uniq of SR_BLOCK entries, and for mult the position of each head
__global__ __launch_bounds__(SR_BLOCK) void sr_scatter_kernel(SrArgs p) {
  __shared__ uint32_t wsum[SR_BLOCK / 64];
  const int tid = threadIdx.x;
  const int64_t u = p.u0 + blockIdx.x, b = u / p.per, c = u - b * p.per;
  const int32_t mm = p.smeta[b];
  if (mm < 0 || c * SR_BLOCK >= mm) return;
  const uint32_t m = (uint32_t)mm, pos = (uint32_t)(c * SR_BLOCK) + tid;
  const uint32_t i = pos < m ? p.sidx[b * p.P + pos] : 0;
  if (p.order && pos < m) p.order[b * p.l_bs + pos] = (int64_t)i;
  if (!p.uniq) return;
  const uint32_t head = pos < m ? p.shead[b * p.P + pos] : 0;
  uint32_t total;
  const uint32_t q = p.sblk[b * (p.P / SR_BLOCK) + c] + sr_block_scan(head, wsum, tid, SR_BLOCK, total);
  if (head) {
    p.uniq[b * p.l_bs + q] = (int64_t)i;
    if (p.mult) reinterpret_cast<uint32_t *>(p.skey + b * p.P)[q] = pos;  // the keys are done with
  }
}

__global__ __launch_bounds__(SR_BLOCK) void sr_mult_kernel(SrArgs p) {
  const int64_t u = p.u0 + blockIdx.x, b = u / p.per, c = u - b * p.per;
  const int32_t mm = p.smeta[b];
  if (mm < 0) return;
  const int64_t total = p.ucount[b], q = c * SR_BLOCK + threadIdx.x;  // written by the scan, a launch before this one
  if (q >= total) return;
  const uint32_t *hpos   = reinterpret_cast<const uint32_t *>(p.skey + b * p.P);
  p.mult[b * p.l_bs + q] = (int64_t)((q + 1 < total ? hpos[q + 1] : (uint32_t)mm) - hpos[q]);
}

// ---- the host side ----------------------------------------------------------------------------------------------------------------------------

bool sizes_negative(int64_t nx, int64_t n, int64_t ell, int64_t batch) { return nx < 0 || n < 0 || ell < 0 || batch < 0; }

int64_t padded_of(int64_t nx) {  // the entries the host sizes a member's network by: the next power of two, at least 2
  int64_t P = 2;
  while (P < nx && P < ((int64_t)1 << 62)) P <<= 1;
  return P;
}

int plan(int64_t nx, int64_t n, int64_t ell, int64_t batch) { return sizes_negative(nx, n, ell, batch) ? -1 : nx <= SR_CHUNK ? 0 : 1; }

int merge_levels(int64_t P) {  // the levels above the chunk: log2(P / SR_CHUNK)
  int L = 0;
  while ((SR_CHUNK << L) < P) ++L;
  return L;
}

// the scratch of path 1: per member P keys, P indices, P flags, P / SR_BLOCK block counts and m_b; -1 beyond int64
int64_t scratch_of(int64_t nx, int64_t batch) {
  if (nx <= SR_CHUNK || batch == 0) return 0;
  const int64_t P      = padded_of(nx);
  const __int128 member = (__int128)P * 13 + P / SR_BLOCK * 4 + 4;  // below 2^66
  if (member > (__int128)INT64_MAX / batch) return -1;
  const __int128 bytes = (__int128)batch * member + 15;
  return bytes > (__int128)INT64_MAX ? -1 : (int64_t)bytes & ~(int64_t)15;
}

template <typename Kernel>
int launch_units(Kernel kernel, SrArgs &p, int64_t batch, int64_t per, int threads, size_t lds, hipStream_t st) {
  p.per = per;
  return launch_members(batch * per, [&](dim3 grid, int64_t u0) {
    p.u0 = u0;
    hipLaunchKernelGGL(kernel, grid, dim3((unsigned)threads), lds, st, p);
  });
}

}  // namespace

extern "C" {

int m4ri_amd_plan_sort_rows_batch(int64_t nx, int64_t n, int64_t ell, int64_t batch) { return plan(nx, n, ell, batch); }

int m4ri_amd_sort_rows_units(int64_t nx, int64_t n, int64_t ell, int64_t batch, int64_t *chunk_rows, int64_t *padded, int64_t *launches) {
  if (sizes_negative(nx, n, ell, batch)) return -1;
  const int64_t P = padded_of(nx);
  const int L     = nx <= SR_CHUNK ? 0 : merge_levels(P);
  if (chunk_rows) *chunk_rows = SR_CHUNK;
  if (padded) *padded = P;
  if (launches) *launches = nx <= SR_CHUNK ? 1 : 1 + (int64_t)L * (L + 1) / 2 + L + 4;
  return 0;
}

int64_t m4ri_amd_sort_rows_scratch_bytes(int64_t nx, int64_t n, int64_t ell, int64_t batch) {
  return sizes_negative(nx, n, ell, batch) ? -1 : scratch_of(nx, batch);
}

int m4ri_amd_sort_rows_batch_dev(const word *X, int64_t x_stride, int64_t x_bs, int64_t nx, int64_t n, const int64_t *xcount, int64_t batch,
                                 const int32_t *cols, int64_t c_bs, int64_t ell, int64_t *order, int64_t *ucount, int64_t *uniq, int64_t *mult, int64_t l_bs,
                                 void *scratch, int64_t scratch_bytes, void *stream) {
  hipStream_t st = (hipStream_t)stream;
  if (sizes_negative(nx, n, ell, batch) || x_stride < 0 || x_bs < 0 || c_bs < 0 || l_bs < 0 || scratch_bytes < 0) return (int)hipErrorInvalidValue;
  if (n > RS_N_MAX || ell > JOIN_ELL_MAX || nx > SR_ROWS_MAX) return (int)hipErrorNotSupported;
  if (!cols && ell > n) return (int)hipErrorInvalidValue;
  if ((!order && !ucount) || (uniq && !ucount) || (mult && !uniq)) return (int)hipErrorInvalidValue;
  const int64_t width = width_of(n);
  if (nx > 1 && x_stride < width) return (int)hipErrorInvalidValue;
  if (batch > 1 && l_bs < nx) return (int)hipErrorInvalidValue;
  const int64_t need = scratch_of(nx, batch);
  if (need < 0) return (int)hipErrorInvalidValue;
  if (batch > 0) {
    if (n > 0 && nx > 0 && !X) return (int)hipErrorInvalidValue;
    if (need > 0 && (!scratch || scratch_bytes < need || ((uintptr_t)scratch & 7))) return (int)hipErrorInvalidValue;
    if (spans_meet_any({entries_span(order, batch, l_bs, nx, 8), entries_span(uniq, batch, l_bs, nx, 8), entries_span(mult, batch, l_bs, nx, 8),
                        entries_span(ucount, batch, 1, 1, 8), entries_span(need > 0 ? scratch : nullptr, 1, 0, need, 1)},
                       {rows_span(X, batch, x_bs, nx, x_stride, width), entries_span(xcount, batch, 1, 1, 8), entries_span(cols, batch, c_bs, ell, 4)}))
      return (int)hipErrorInvalidValue;
  }
  if (batch == 0) return 0;

  HIPTRY(set_max_dynamic_lds(SR_LDS_MAX, sr_wg_kernel, sr_chunk_kernel));

  SrArgs p{};
  p.X = X, p.xcount = xcount, p.cols = cols, p.x_stride = x_stride, p.x_bs = x_bs, p.c_bs = c_bs, p.nx = nx, p.l_bs = l_bs;
  p.n = (int)n, p.width = (int)width, p.ell = (int)ell;
  p.mask = tail_mask((int)(n & 63)), p.fmask = ell >= 64 ? ~(word)0 : ((word)1 << ell) - 1;
  p.order = order, p.ucount = ucount, p.uniq = uniq, p.mult = mult;
  const int64_t P = padded_of(nx);
  p.P             = P;
  if (nx <= SR_CHUNK) {
    const int threads = P / 2 >= SR_THREADS ? SR_THREADS : P / 2 <= 64 ? 64 : (int)(P / 2);
    return launch_units(sr_wg_kernel, p, batch, 1, threads, SrCarve(P).total, st);
  }
  // path 1: the scratch, then the launches
  unsigned char *s = static_cast<unsigned char *>(scratch);
  p.skey           = reinterpret_cast<word *>(s);
  p.sidx           = reinterpret_cast<uint32_t *>(s + (size_t)batch * (size_t)P * 8);
  p.sblk           = p.sidx + (size_t)batch * (size_t)P;
  p.smeta          = reinterpret_cast<int32_t *>(p.sblk + (size_t)batch * (size_t)(P / SR_BLOCK));
  p.shead          = reinterpret_cast<uint8_t *>(p.smeta + batch);
  p.first          = 1;
  if (const int e = launch_units(sr_chunk_kernel, p, batch, P / SR_CHUNK, SR_THREADS, SR_LDS_MAX, st)) return e;
  p.first = 0;
  for (int64_t k = 2 * SR_CHUNK; k <= P; k <<= 1) {
    p.k = (uint32_t)k;
    for (int64_t j = k >> 1; j >= SR_CHUNK; j >>= 1) {
      p.j = (uint32_t)j;
      if (const int e = launch_units(sr_global_kernel, p, batch, P / 2 / SR_PAIR_THREADS, SR_PAIR_THREADS, 0, st)) return e;
    }
    if (const int e = launch_units(sr_chunk_kernel, p, batch, P / SR_CHUNK, SR_THREADS, SR_LDS_MAX, st)) return e;
  }
  if (ucount) {
    if (const int e = launch_units(sr_heads_kernel, p, batch, P / SR_BLOCK, SR_BLOCK, 0, st)) return e;
    if (const int e = launch_units(sr_scan_kernel, p, batch, 1, SR_THREADS, 0, st)) return e;
  }
  if (order || uniq)
    if (const int e = launch_units(sr_scatter_kernel, p, batch, P / SR_BLOCK, SR_BLOCK, 0, st)) return e;
  if (mult)
    if (const int e = launch_units(sr_mult_kernel, p, batch, P / SR_BLOCK, SR_BLOCK, 0, st)) return e;
  return 0;
}

}  // extern "C"
