// lists_collide_batch.hip -- the join of two EXPLICIT lists of words on a window of bits, one call for a batch, every result left on the
// device; and the words behind the keys such a join lists.  rowsums_collide_batch.hip joins the sums of t1 and of t2 rows of one
// generator and tables the whole left list in one workgroup's LDS (N1 <= 8192); here the lists are rows in memory, of any length, so the
// output of one join (written out by m4ri_amd_lists_words_batch_dev below) can be an input of the next.
//
// Member b has a left list X_b (nx rows of n bits), a right list Y_b (ny rows), an optional word V_b and a window cols_b of ell <= 64
// columns.  The word of pair (i, j) is c = V ^ X[i] ^ Y[j]; the pair COLLIDES iff c is 0 at every window column.  The outputs are those
// of m4ri_amd_row_sums_collide_list_batch_dev with the pair rank i * ny + j: hist[b * (n + 1) + w] counts the colliding pairs of weight w,
// lightest[b] is the minimum of (wt << 40) | rank over the colliding pairs with wt >= w_min (-1: none), list / count the keys of the
// pairs with w_min <= wt <= w_max.  A member with a window entry outside [0, n) is REFUSED on the device: hist -1, lightest -2, count -1.
//
// lc_kernel, a workgroup its unit of work: it owns a member, a CHUNK of the left list (LC_CHUNK = 8192 rows, the last one shorter) and
// a SLICE of the right list.
//   window  range-checked into LDS (a refused member's workgroup stops here); thread 0 gathers V's key.
//   table   a thread per left row of the chunk (LC_KPT = 8 rows per thread at 1024 threads) gathers the row's ell window bits from global
//           memory into a 64-bit key and KEEPS it in a register; the (key, index in chunk) entries are counting-sorted in LDS on the
//           key's low q bits, q = ceil(log2 chunk) held at ell: count with LDS atomics, scan, scatter from the registers.  The global
//           rows are read once for the table.  Holding the keys in registers and not in a second LDS array is what lets the chunk be
//           8192: sorted keys 64 KiB, indices 16 KiB, bucket ends 32 KiB, the rest 9 KiB, 121 KiB in all; an unsorted LDS copy of
//           the keys (64 KiB more) would halve it.
//           cols = NULL (the columns 0 .. ell-1) is one masked word per row.
//   walk    a lane per right row of the slice gathers its key, XORs V's, and compares the FULL key of every entry of its bucket.
//   match   the lane reads X[chunk0 + idx], Y[j] and V from global memory, weighs up to 16 words, adds to a 32-bit bin in LDS, keeps its
//           minimum and takes a list slot.
// Paths (m4ri_amd_plan_lists_collide_batch; the units by m4ri_amd_lists_collide_units):
//   0  one chunk and one slice per member: every output entry is written once with a plain store, the refused form included, the count
//      comes from a counter in LDS.  Members without pairs or columns are answered by the initialisation kernel alone and count here.
//   1  otherwise: the initialisation kernel sets the outputs (and answers the refused members), the workgroups combine with 64-bit
//      integer atomics: one minimum, one add per non-zero bin, one returning add per listed pair.
// A workgroup's pairs, chunk * slice, stay below 2^32 (its 32-bit bins hold); a slice is ceil(ny / slices) rows and never shorter than the
// chunk or than 256 rows unless the list is (the last slice takes what is left); the right list is cut only until the call has about
// 1024 workgroups.
//
// The count / scan / scatter of rc_kernel (rowsums_collide_batch.hip) is written again here and not shared: that file's kernels are
// sensitive to register pressure and stay exactly as they are.
// Plain launches on the caller's stream: no allocation, no copy to the host, no synchronisation, no engine workspace or lock.
#include <hip/hip_runtime.h>
#include <limits.h>
#include <mutex>
#include "batch_common.h"
#include "subset_rank.h"
#include "../../include/m4ri_amd.h"

namespace {

constexpr int64_t LC_ELL_MAX    = 64;                      // a key is one 64-bit word
constexpr int64_t LC_ROWS_MAX   = ((int64_t)1 << 31) - 1;  // nx, ny
constexpr int64_t LC_CHUNK      = 8192;                    // left rows per workgroup: what the LDS table holds with the keys in registers
constexpr int LC_CHUNK_BITS     = 13;
constexpr int LC_KPT            = 8;                       // keys a thread keeps: LC_CHUNK / 1024
constexpr int64_t LC_PAIRS_WG   = ((int64_t)1 << 32) - 1;  // chunk * slice: the 32-bit bins of a workgroup hold
constexpr int64_t LC_BLOCKS_MIN = 1024;                    // the right lists are cut until the call has this many workgroups ...
constexpr int64_t LC_SLICE_MIN  = 256;                     // ... but no slice shorter than this, or than the chunk
constexpr int LC_THREADS_MAX    = BATCH_MAX_THREADS;
constexpr int LC_WT             = 16;                      // register words of a weighed word: n <= 1024
static_assert(LC_CHUNK == (int64_t)LC_KPT * LC_THREADS_MAX && LC_CHUNK == (int64_t)1 << LC_CHUNK_BITS && LC_CHUNK <= 65536, "the chunk");

// where the pieces of a workgroup's LDS are, in bytes; the same arithmetic on both sides of the launch.  rows: the longest chunk
struct LcCarve {
  size_t wmin, off, part, bins, cols, sidx, slots, total;
  __host__ __device__ LcCarve(int n, int rows, int q) {
    wmin  = (size_t)rows * 8;                              // the sorted keys first
    off   = wmin + (size_t)(LC_THREADS_MAX / 64 + 2) * 8;  // a minimum per wave, then V's key
    part  = off + ((size_t)1 << q) * 4;                    // the bucket counts, then starts, then ends
    bins  = part + (size_t)LC_THREADS_MAX * 4;             // the scan's partial sums
    cols  = bins + (size_t)(n + 1) * 4;
    sidx  = cols + (size_t)LC_ELL_MAX * 4;
    slots = pad16(sidx + (size_t)rows * 2);                // the index in the chunk, 16 bits
    total = slots + 16;                                    // the list's slot counter of path 0
  }
};

const size_t LC_LDS_MAX = LcCarve((int)RS_N_MAX, (int)LC_CHUNK, LC_CHUNK_BITS).total;

struct LcArgs {
  const word *X, *Y, *V;  // V may be NULL
  const int32_t *cols;    // NULL: columns 0 .. ell-1
  int64_t x_stride, x_bs, y_stride, y_bs, v_bs, c_bs;
  int64_t nx, ny;                    // both >= 1
  int n, width;                      // width = words(n) >= 1
  int ell, q, rows;                  // q bucket bits; rows = min(nx, LC_CHUNK), the carve's
  word mask, fmask;                  // of a row's last word; of the key where cols = NULL
  int w_min, w_max;                  // at most n + 1; at most n
  int atomic;                        // path 1
  int64_t chunks, slices, slice_len; // per member
  int64_t *hist, *lightest, *list, *count;  // list may be NULL at cap = 0
  int64_t l_bs, cap;
  int64_t u0;                        // this launch: workgroups from u0 on
};

// the ell window bits of row r as one word
__device__ __forceinline__ word window_key(const word *r, const int32_t *wcols, int ell, bool first, word fmask) {
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

template <bool HIST, bool LIGHT, bool LIST>
__global__ __launch_bounds__(LC_THREADS_MAX) void lc_kernel(LcArgs p) {
  extern __shared__ __align__(16) word lc_lds[];
  const int tid = threadIdx.x, T = blockDim.x, lane = tid & 63, wave = tid >> 6;
  const int64_t u   = p.u0 + blockIdx.x;
  const int64_t per = p.chunks * p.slices;
  const int64_t b   = u / per;
  const int64_t ch  = (u - b * per) / p.slices;
  const int64_t sl  = u - b * per - ch * p.slices;
  const LcCarve at(p.n, p.rows, p.q);
  unsigned char *lds = reinterpret_cast<unsigned char *>(lc_lds);
  word *skey         = lc_lds;
  word *wmin         = reinterpret_cast<word *>(lds + at.wmin);
  word *vkey         = wmin + LC_THREADS_MAX / 64;
  uint32_t *off      = reinterpret_cast<uint32_t *>(lds + at.off);
  uint32_t *part     = reinterpret_cast<uint32_t *>(lds + at.part);
  uint32_t *bins     = reinterpret_cast<uint32_t *>(lds + at.bins);
  int32_t *wcols     = reinterpret_cast<int32_t *>(lds + at.cols);
  uint16_t *sidx     = reinterpret_cast<uint16_t *>(lds + at.sidx);
  uint32_t *slots    = reinterpret_cast<uint32_t *>(lds + at.slots);  // LIST, path 0
  const int n = p.n, nb = 1 << p.q;
  const bool first   = p.cols == nullptr;
  const int64_t row0 = ch * LC_CHUNK;
  const int nc       = (int)(p.nx - row0 < LC_CHUNK ? p.nx - row0 : LC_CHUNK);  // 1 <= nc <= rows <= LC_KPT * T
  const word *x = p.X + b * p.x_bs + row0 * p.x_stride;
  const word *y = p.Y + b * p.y_bs;
  const word *v = p.V ? p.V + b * p.v_bs : nullptr;

  // 1. the window, checked; nothing outside the member is read
  int bad = 0;
  if (tid < p.ell) {
    const int c = first ? tid : p.cols[b * p.c_bs + tid];
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
  if (tid == 0) vkey[0] = v ? window_key(v, wcols, p.ell, first, p.fmask) : 0;
  for (int i = tid; i < nb; i += T) off[i] = 0;
  if (HIST)
    for (int i = tid; i <= n; i += T) bins[i] = 0;
  if (LIST && tid == 0) slots[0] = 0;
  __syncthreads();

  // 2. the left table: the keys into registers and counted, scan, scatter
  const word qmask = (word)nb - 1;
  word keys[LC_KPT];
#pragma unroll
  for (int i = 0; i < LC_KPT; ++i) {
    const int r = tid + i * T;
    keys[i]     = 0;
    if (r < nc) {
      keys[i] = window_key(x + (int64_t)r * p.x_stride, wcols, p.ell, first, p.fmask);
      atomicAdd(&off[(uint32_t)(keys[i] & qmask)], 1u);
    }
  }
  __syncthreads();
  const int seg = (nb + T - 1) / T, c0 = tid * seg < nb ? tid * seg : nb, c1 = c0 + seg < nb ? c0 + seg : nb;
  {
    uint32_t s = 0;
    for (int i = c0; i < c1; ++i) s += off[i];
    part[tid] = s;
  }
  __syncthreads();
  if (wave == 0) {  // the exclusive scan of the T partial sums: T / 64 per lane, then across the lanes
    const int pl  = T >> 6;
    uint32_t s    = 0;
    for (int j = 0; j < pl; ++j) s += part[lane * pl + j];
    uint32_t incl = s;
    for (int o = 1; o < 64; o <<= 1) {
      const uint32_t t = __shfl_up(incl, o);
      if (lane >= o) incl += t;
    }
    uint32_t run = incl - s;
    for (int j = 0; j < pl; ++j) {
      const uint32_t t    = part[lane * pl + j];
      part[lane * pl + j] = run;
      run += t;
    }
  }
  __syncthreads();
  {
    uint32_t run = part[tid];
    for (int i = c0; i < c1; ++i) {
      const uint32_t t = off[i];
      off[i]           = run;  // the bucket's start
      run += t;
    }
  }
  __syncthreads();
#pragma unroll
  for (int i = 0; i < LC_KPT; ++i) {
    const int r = tid + i * T;
    if (r < nc) {
      const uint32_t pos = atomicAdd(&off[(uint32_t)(keys[i] & qmask)], 1u);  // pos < nc: the counts sum to nc
      skey[pos]          = keys[i];
      sidx[pos]          = (uint16_t)r;
    }
  }
  __syncthreads();  // off[i] is now the END of bucket i, the start of bucket i + 1

  // 3. the right walk
  const int64_t s0 = sl * p.slice_len;
  const int64_t s1 = s0 + p.slice_len < p.ny ? s0 + p.slice_len : p.ny;
  const word vk    = vkey[0];
  unsigned long long best = ~0ull;  // the lane's lightest: none
  for (int64_t j = s0 + tid; j < s1; j += T) {
    const word *yr       = y + j * p.y_stride;
    const word key2      = vk ^ window_key(yr, wcols, p.ell, first, p.fmask);
    const uint32_t bkt   = (uint32_t)(key2 & qmask);
    const uint32_t e_end = off[bkt];
    for (uint32_t e = bkt ? off[bkt - 1] : 0; e < e_end; ++e) {
      if (skey[e] != key2) continue;
      const uint32_t idx = sidx[e];
      const word *xr     = x + (int64_t)idx * p.x_stride;
      int wt             = 0;
#pragma unroll
      for (int w = 0; w < LC_WT; ++w)
        if (w < p.width) {
          word c = xr[w] ^ yr[w];
          if (v) c ^= v[w];
          if (w == p.width - 1) c &= p.mask;
          wt += __popcll(c);
        }
      const unsigned long long rank = (unsigned long long)(row0 + idx) * (unsigned long long)p.ny + (unsigned long long)j;
      const unsigned long long cand = ((unsigned long long)(uint32_t)wt << 40) | rank;
      if (HIST) atomicAdd(&bins[wt], 1u);
      if (LIGHT && wt >= p.w_min) best = cand < best ? cand : best;
      if (LIST && wt >= p.w_min && wt <= p.w_max) {  // a slot each, taken whether or not it is below cap: the count is the true total
        const unsigned long long slot = p.atomic ? atomicAdd(reinterpret_cast<unsigned long long *>(p.count + b), 1ull) : (unsigned long long)atomicAdd(slots, 1u);
        if (slot < (unsigned long long)p.cap) p.list[b * p.l_bs + (int64_t)slot] = (int64_t)cand;
      }
    }
  }

  // 4. the outputs
  if (LIGHT) {
    for (int o = 32; o; o >>= 1) {
      const unsigned long long t = __shfl_xor(best, o);
      best                       = t < best ? t : best;
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

struct LcInit {
  int64_t *hist, *lightest;
  int64_t b0;              // this launch: members from b0 on, a workgroup each
  int n, ell;
  const int32_t *cols;
  int64_t c_bs;
  int64_t hist0, light_v;  // hist[b][0] = hist0, the other entries 0; lightest[b] = light_v
  int64_t *list, *count;   // count[b] = count_v, and list[b * l_bs + i] = i (weight 0, rank i) for i < min(count_v, cap):
  int64_t l_bs, cap, count_v;  // count_v > 0 only for members without columns, whose pairs all weigh 0
};

// What path 1's atomics start from, the whole result of members without pairs or columns, and the refused form wherever it runs.
__global__ __launch_bounds__(BATCH_WAVE_THREADS) void lc_init_kernel(LcInit p) {
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

int launch_init(hipStream_t st, LcInit p, int64_t batch) {
  return launch_chunked(batch, BATCH_CHUNK, [&](int64_t b0, int64_t nb) {
    p.b0 = b0;
    hipLaunchKernelGGL(lc_init_kernel, dim3((unsigned)nb), dim3(BATCH_WAVE_THREADS), 0, st, p);
  });
}

// the chunks and slices of a member with rows on both sides (nx, ny >= 1)
struct LcUnits {
  int64_t chunks, slices, slice_len;
};

LcUnits units_of(int64_t nx, int64_t ny, int64_t batch) {  // no sum or product here leaves int64 for any nx, ny, batch >= 0
  LcUnits u;
  u.chunks            = nx / LC_CHUNK + (nx % LC_CHUNK != 0);
  const int64_t chunk = nx < LC_CHUNK ? nx : LC_CHUNK;
  const int64_t mem   = batch > 0 ? batch : 1;
  const int64_t have  = mem >= LC_BLOCKS_MIN || u.chunks >= LC_BLOCKS_MIN ? LC_BLOCKS_MIN : mem * u.chunks;  // workgroups before the right list is cut
  const int64_t want  = have >= LC_BLOCKS_MIN ? 1 : (LC_BLOCKS_MIN + have - 1) / have;
  const int64_t floor = chunk > LC_SLICE_MIN ? chunk : LC_SLICE_MIN;
  int64_t slices      = ny / floor;  // so that ceil(ny / slices) >= floor
  if (slices > want) slices = want;
  if (slices < 1) slices = 1;
  u.slice_len = ny / slices + (ny % slices != 0);
  if (u.slice_len > LC_PAIRS_WG / chunk) u.slice_len = LC_PAIRS_WG / chunk;  // at least 2^19: above the floor
  u.slices = ny / u.slice_len + (ny % u.slice_len != 0);
  return u;
}

bool sizes_negative(int64_t nx, int64_t ny, int64_t n, int64_t ell, int64_t batch) { return nx < 0 || ny < 0 || n < 0 || ell < 0 || batch < 0; }

int plan(int64_t nx, int64_t ny, int64_t n, int64_t ell, int64_t batch) {
  if (sizes_negative(nx, ny, n, ell, batch)) return -1;
  if (n == 0 || nx == 0 || ny == 0) return 0;  // the initialisation kernel alone
  const LcUnits u = units_of(nx, ny, batch);
  return u.chunks == 1 && u.slices == 1 ? 0 : 1;
}

// beyond the limits of both calls?
bool unsupported(int64_t nx, int64_t ny, int64_t n) {
  return n > RS_N_MAX || nx > LC_ROWS_MAX || ny > LC_ROWS_MAX || (__int128)nx * ny > RS_SUMS_MAX;
}

template <bool LIST>
void launch_walk(bool hist, bool light, dim3 grid, dim3 block, size_t lds, hipStream_t st, const LcArgs &p) {
  if (hist && light) hipLaunchKernelGGL((lc_kernel<true, true, LIST>), grid, block, lds, st, p);
  else if (hist) hipLaunchKernelGGL((lc_kernel<true, false, LIST>), grid, block, lds, st, p);
  else if (light) hipLaunchKernelGGL((lc_kernel<false, true, LIST>), grid, block, lds, st, p);
  else if constexpr (LIST) hipLaunchKernelGGL((lc_kernel<false, false, true>), grid, block, lds, st, p);  // the list alone
}

// ---- the words behind listed keys ---------------------------------------------------------------------------------------------------------

constexpr int LW_ROWS = BATCH_WAVE_THREADS;  // output rows per workgroup, a thread each in the first phase

struct LwArgs {
  const word *X, *Y, *V;  // V may be NULL
  const int64_t *keys, *count;
  word *W;
  int32_t *skipped;
  int64_t x_stride, x_bs, y_stride, y_bs, v_bs, l_bs, cap, w_stride, w_bs;
  int width, group;     // group: lanes per output row, a power of two >= width, 1 where n = 0
  word mask;
  int64_t ny, pairs;    // nx * ny (0: no key is valid)
  int64_t chunks;       // workgroups per member: ceil(cap / LW_ROWS)
  int64_t u0;           // this launch: workgroups from u0 on
};

// As rw_kernel (rowsums_words_batch.hip): a thread per key checks it and splits the rank ONCE into the two row indices, then a group of
// lanes per output row, lane j of a group on word j, reads consecutive words of V, X[i], Y[j] and writes consecutive words of W.
__global__ __launch_bounds__(LW_ROWS) void lw_kernel(LwArgs p) {
  __shared__ uint32_t rows[LW_ROWS][2];
  __shared__ uint8_t live[LW_ROWS];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t u = p.u0 + blockIdx.x, b = u / p.chunks, i0 = (u - b * p.chunks) * LW_ROWS;
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
    if (ok) {
      const unsigned long long ri = r / (unsigned long long)p.ny;
      rows[tid][0]                = (uint32_t)ri;
      rows[tid][1]                = (uint32_t)(r - ri * (unsigned long long)p.ny);
    }
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
  const word *xm = p.X + b * p.x_bs;
  const word *ym = p.Y + b * p.y_bs;
  const word *v  = p.V ? p.V + b * p.v_bs : nullptr;
  word *out      = p.W + b * p.w_bs;
  for (int pass = 0; pass < g; ++pass) {
    const int lr = wave * 64 + pass * per + (lane >> __builtin_ctz(g));
    if (!live[lr]) continue;
    word c = xm[(int64_t)rows[lr][0] * p.x_stride + w] ^ ym[(int64_t)rows[lr][1] * p.y_stride + w];
    if (v) c ^= v[w];
    store_masked(out + (i0 + lr) * p.w_stride + w, c, w == p.width - 1, p.mask);
  }
}

}  // namespace

extern "C" {

int m4ri_amd_plan_lists_collide_batch(int64_t nx, int64_t ny, int64_t n, int64_t ell, int64_t batch) { return plan(nx, ny, n, ell, batch); }

int m4ri_amd_lists_collide_units(int64_t nx, int64_t ny, int64_t n, int64_t ell, int64_t batch, int64_t *chunk_rows, int64_t *chunks, int64_t *slices) {
  if (sizes_negative(nx, ny, n, ell, batch)) return -1;
  LcUnits u{0, 0, 0};
  if (n > 0 && nx > 0 && ny > 0) u = units_of(nx, ny, batch);
  if (chunk_rows) *chunk_rows = LC_CHUNK;
  if (chunks) *chunks = u.chunks;
  if (slices) *slices = u.slices;
  return 0;
}

int m4ri_amd_lists_collide_batch_dev(const word *X, int64_t x_stride, int64_t x_bs, int64_t nx, const word *Y, int64_t y_stride, int64_t y_bs, int64_t ny,
                                     int64_t n, const word *V, int64_t v_bs, int64_t batch, const int32_t *cols, int64_t c_bs, int64_t ell, int64_t w_min,
                                     int64_t w_max, int64_t *hist, int64_t *lightest, int64_t *list, int64_t l_bs, int64_t cap, int64_t *count,
                                     void *stream) {
  hipStream_t st = (hipStream_t)stream;
  if (sizes_negative(nx, ny, n, ell, batch) || x_stride < 0 || x_bs < 0 || y_stride < 0 || y_bs < 0 || v_bs < 0 || c_bs < 0 || w_min < 0 || w_max < 0 ||
      cap < 0 || l_bs < 0)
    return (int)hipErrorInvalidValue;
  if (unsupported(nx, ny, n) || ell > LC_ELL_MAX) return (int)hipErrorNotSupported;
  const int64_t pairs = nx * ny;  // at most 2^40
  if (!cols && ell > n) return (int)hipErrorInvalidValue;
  if (!hist && !lightest && !count) return (int)hipErrorInvalidValue;
  if ((list && !count) || (count && !list && cap > 0)) return (int)hipErrorInvalidValue;  // they come together; a count alone at cap = 0
  if (count && batch > 1 && l_bs < cap) return (int)hipErrorInvalidValue;
  const int64_t width = words_of(n);
  if (n > 0 && ((nx > 1 && x_stride < width) || (ny > 1 && y_stride < width))) return (int)hipErrorInvalidValue;
  const bool walked = pairs > 0 && n > 0;  // rows are read
  if (batch > 0) {
    if (walked && (!X || !Y)) return (int)hipErrorInvalidValue;
    const bool listed = count && list && cap > 0;
    const void *outs[4]      = {hist, lightest, count, listed ? list : nullptr};
    const uintptr_t bytes[4] = {(uintptr_t)(batch * (n + 1)) * 8, (uintptr_t)batch * 8, (uintptr_t)batch * 8,
                                ((uintptr_t)(batch - 1) * (uintptr_t)l_bs + (uintptr_t)cap) * 8};
    for (int o = 0; o < 4; ++o) {
      if (!outs[o]) continue;
      for (int o2 = o + 1; o2 < 4; ++o2)
        if (outs[o2] && spans_meet(outs[o], bytes[o], outs[o2], bytes[o2])) return (int)hipErrorInvalidValue;
      if (nx > 0 && n > 0 && X && spans_meet(outs[o], bytes[o], X, member_span_bytes(batch, x_bs, nx, x_stride, width))) return (int)hipErrorInvalidValue;
      if (ny > 0 && n > 0 && Y && spans_meet(outs[o], bytes[o], Y, member_span_bytes(batch, y_bs, ny, y_stride, width))) return (int)hipErrorInvalidValue;
      if (V && n > 0 && spans_meet(outs[o], bytes[o], V, member_span_bytes(batch, v_bs, 1, 0, width))) return (int)hipErrorInvalidValue;
      if (cols && ell > 0 && spans_meet(outs[o], bytes[o], cols, (uintptr_t)((batch - 1) * c_bs + ell) * 4)) return (int)hipErrorInvalidValue;
    }
  }
  if (batch == 0) return 0;
  LcInit in{};
  in.hist = hist, in.lightest = lightest, in.n = (int)n, in.ell = (int)ell, in.cols = cols, in.c_bs = c_bs, in.light_v = -1;
  in.list = list, in.count = count, in.l_bs = l_bs, in.cap = cap;
  if (!walked) {  // every word weighs 0: all pairs in the one bin, the lightest is rank 0 if weight 0 qualifies; or no pairs
    in.hist0 = pairs, in.light_v = pairs > 0 && w_min == 0 ? 0 : -1;  // n = 0 with a window given: every entry is outside, all refused
    in.count_v = w_min == 0 ? pairs : 0;                              // weight 0 is in the band iff w_min = 0: w_max >= 0
    return launch_init(st, in, batch);
  }
  const LcUnits u = units_of(nx, ny, batch);
  if (batch > INT64_MAX / u.chunks / u.slices) return (int)hipErrorInvalidValue;
  LcArgs p{};
  p.X = X, p.Y = Y, p.V = V, p.cols = cols, p.x_stride = x_stride, p.x_bs = x_bs, p.y_stride = y_stride, p.y_bs = y_bs, p.v_bs = v_bs, p.c_bs = c_bs;
  p.nx = nx, p.ny = ny, p.n = (int)n, p.width = (int)width, p.ell = (int)ell, p.rows = (int)(nx < LC_CHUNK ? nx : LC_CHUNK);
  p.mask = tail_mask((int)(n & 63)), p.fmask = ell >= 64 ? ~(word)0 : ((word)1 << ell) - 1;
  p.w_min = (int)(w_min > n + 1 ? n + 1 : w_min), p.w_max = (int)(w_max > n ? n : w_max);
  p.hist = hist, p.lightest = lightest, p.list = list, p.count = count, p.l_bs = l_bs, p.cap = cap;
  while (p.q < ell && ((int64_t)1 << p.q) < p.rows) ++p.q;
  p.chunks = u.chunks, p.slices = u.slices, p.slice_len = u.slice_len;
  p.atomic = !(u.chunks == 1 && u.slices == 1);
  static std::once_flag once;
  static hipError_t attr = hipSuccess;
  std::call_once(once, [] {
    const void *kernels[] = {reinterpret_cast<const void *>(lc_kernel<true, true, false>), reinterpret_cast<const void *>(lc_kernel<true, false, false>),
                             reinterpret_cast<const void *>(lc_kernel<false, true, false>), reinterpret_cast<const void *>(lc_kernel<true, true, true>),
                             reinterpret_cast<const void *>(lc_kernel<true, false, true>), reinterpret_cast<const void *>(lc_kernel<false, true, true>),
                             reinterpret_cast<const void *>(lc_kernel<false, false, true>)};
    for (const void *f : kernels)
      if (attr == hipSuccess) attr = hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, (int)LC_LDS_MAX);
  });
  HIPTRY(attr);
  const size_t lds  = LcCarve((int)n, p.rows, p.q).total;
  const int threads = p.rows <= LC_KPT * BATCH_WAVE_THREADS && p.slice_len <= 4096 ? BATCH_WAVE_THREADS : LC_THREADS_MAX;  // rows <= LC_KPT * threads
  if (p.atomic) HIPTRY(launch_init(st, in, batch));
  return launch_chunked(batch * u.chunks * u.slices, BATCH_CHUNK, [&](int64_t u0, int64_t nu) {
    p.u0 = u0;
    const dim3 grid((unsigned)nu), block((unsigned)threads);
    if (count) launch_walk<true>(hist != nullptr, lightest != nullptr, grid, block, lds, st, p);
    else launch_walk<false>(hist != nullptr, lightest != nullptr, grid, block, lds, st, p);
  });
}

int m4ri_amd_lists_words_batch_dev(const word *X, int64_t x_stride, int64_t x_bs, int64_t nx, const word *Y, int64_t y_stride, int64_t y_bs, int64_t ny,
                                   int64_t n, const word *V, int64_t v_bs, int64_t batch, const int64_t *keys, int64_t l_bs, int64_t cap,
                                   const int64_t *count, word *W, int64_t w_stride, int64_t w_bs, int32_t *skipped, void *stream) {
  hipStream_t st = (hipStream_t)stream;
  if (nx < 0 || ny < 0 || n < 0 || batch < 0 || x_stride < 0 || x_bs < 0 || y_stride < 0 || y_bs < 0 || v_bs < 0 || l_bs < 0 || cap < 0 || w_stride < 0 ||
      w_bs < 0)
    return (int)hipErrorInvalidValue;
  if (unsupported(nx, ny, n)) return (int)hipErrorNotSupported;
  const int64_t pairs = nx * ny;
  const int64_t width = words_of(n);
  if (n > 0 && ((nx > 1 && x_stride < width) || (ny > 1 && y_stride < width))) return (int)hipErrorInvalidValue;
  if (cap > 1 && w_stride < width) return (int)hipErrorInvalidValue;
  if (batch > 1 && cap > 0 && (l_bs < cap || (n > 0 && (__int128)w_bs < (__int128)(cap - 1) * w_stride + width))) return (int)hipErrorInvalidValue;
  if (batch > 0 && cap > 0) {
    const bool read = pairs > 0 && n > 0;  // rows of X and Y are read
    if (!keys || (n > 0 && !W) || (read && (!X || !Y))) return (int)hipErrorInvalidValue;
    const void *outs[2]      = {n > 0 ? W : nullptr, skipped};
    const uintptr_t bytes[2] = {n > 0 ? member_span_bytes(batch, w_bs, cap, w_stride, width) : 0, (uintptr_t)batch * 4};
    if (outs[0] && outs[1] && spans_meet(outs[0], bytes[0], outs[1], bytes[1])) return (int)hipErrorInvalidValue;
    for (int o = 0; o < 2; ++o) {
      if (!outs[o]) continue;
      if (nx > 0 && n > 0 && X && spans_meet(outs[o], bytes[o], X, member_span_bytes(batch, x_bs, nx, x_stride, width))) return (int)hipErrorInvalidValue;
      if (ny > 0 && n > 0 && Y && spans_meet(outs[o], bytes[o], Y, member_span_bytes(batch, y_bs, ny, y_stride, width))) return (int)hipErrorInvalidValue;
      if (V && n > 0 && spans_meet(outs[o], bytes[o], V, member_span_bytes(batch, v_bs, 1, 0, width))) return (int)hipErrorInvalidValue;
      if (spans_meet(outs[o], bytes[o], keys, ((uintptr_t)(batch - 1) * (uintptr_t)l_bs + (uintptr_t)cap) * 8)) return (int)hipErrorInvalidValue;
      if (count && spans_meet(outs[o], bytes[o], count, (uintptr_t)batch * 8)) return (int)hipErrorInvalidValue;
    }
  }
  if (batch == 0) return 0;
  if (skipped) HIPTRY(hipMemsetAsync(skipped, 0, (size_t)batch * 4, st));  // written whole: 0 for a clean member, and at cap = 0
  if (cap == 0) return 0;
  LwArgs p{};
  p.X = X, p.Y = Y, p.V = n > 0 ? V : nullptr, p.keys = keys, p.count = count, p.W = W, p.skipped = skipped;
  p.x_stride = x_stride, p.x_bs = x_bs, p.y_stride = y_stride, p.y_bs = y_bs, p.v_bs = v_bs, p.l_bs = l_bs, p.cap = cap, p.w_stride = w_stride, p.w_bs = w_bs;
  p.width = (int)width, p.group = 1;
  while (p.group < width) p.group <<= 1;
  p.mask = tail_mask((int)(n & 63)), p.ny = ny > 0 ? ny : 1, p.pairs = pairs;
  p.chunks = (cap + LW_ROWS - 1) / LW_ROWS;
  if (batch > INT64_MAX / p.chunks) return (int)hipErrorInvalidValue;
  return launch_chunked(batch * p.chunks, BATCH_CHUNK, [&](int64_t u0, int64_t nu) {
    p.u0 = u0;
    hipLaunchKernelGGL(lw_kernel, dim3((unsigned)nu), dim3(LW_ROWS), 0, st, p);
  });
}

}  // extern "C"
