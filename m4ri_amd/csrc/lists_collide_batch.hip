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
// The table's scan, what happens to a match, the output step, the initialisation kernel, the LDS carve and the host
// side of the launch are join_common.h's, shared with rowsums_collide_batch.hip, and so is the skeleton of the words kernel, shared
// with rowsums_words_batch.hip.  What is here: the keys of the rows, the word and the rank of a match, the chunks and slices.
// Plain launches on the caller's stream: no allocation, no copy to the host, no synchronisation, no engine workspace or lock.
#include <hip/hip_runtime.h>
#include "join_common.h"
#include "../../include/m4ri_amd.h"

namespace {

constexpr int64_t LC_ROWS_MAX = ((int64_t)1 << 31) - 1;  // nx, ny
constexpr int64_t LC_CHUNK    = 8192;                    // left rows per workgroup: what the LDS table holds with the keys in registers
constexpr int LC_CHUNK_BITS   = 13;
constexpr int LC_KPT          = 8;                       // keys a thread keeps: LC_CHUNK / 1024
static_assert(LC_CHUNK == (int64_t)LC_KPT * JOIN_THREADS_MAX && LC_CHUNK == (int64_t)1 << LC_CHUNK_BITS && LC_CHUNK <= 65536, "the chunk");

// the LDS of a workgroup: V's key first (two words, for the alignment of what follows), then the table of `rows` entries, the longest chunk
__host__ __device__ inline JoinCarve lc_carve(int n, int rows, int q, bool list) { return JoinCarve(16, rows, n, q, list); }

const size_t LC_LDS_MAX = lc_carve((int)RS_N_MAX, (int)LC_CHUNK, LC_CHUNK_BITS, true).total;

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
__global__ __launch_bounds__(JOIN_THREADS_MAX) void lc_kernel(LcArgs p) {
  extern __shared__ __align__(16) word lc_lds[];
  const int tid = threadIdx.x, T = blockDim.x;
  const int64_t u   = p.u0 + blockIdx.x;
  const int64_t per = p.chunks * p.slices;
  const int64_t b   = u / per;
  const int64_t ch  = (u - b * per) / p.slices;
  const int64_t sl  = u - b * per - ch * p.slices;
  const JoinOut o{p.hist, p.lightest, p.list, p.count, p.l_bs, p.cap, p.n, p.w_min, p.w_max, p.atomic};
  const JoinLds L(lc_lds, lc_carve(p.n, p.rows, p.q, LIST));
  word *vkey = lc_lds;
  const int nb = 1 << p.q;
  const bool first   = p.cols == nullptr;
  const int64_t row0 = ch * LC_CHUNK;
  const int nc       = (int)(p.nx - row0 < LC_CHUNK ? p.nx - row0 : LC_CHUNK);  // 1 <= nc <= rows <= LC_KPT * T
  const word *x = p.X + b * p.x_bs + row0 * p.x_stride;
  const word *y = p.Y + b * p.y_bs;
  const word *v = p.V ? p.V + b * p.v_bs : nullptr;

  // 1. the window, then V's key
  if (join_window(L.cols, p.cols, b * p.c_bs, p.ell, p.n, tid)) {
    join_refuse<HIST, LIGHT, LIST>(o, b, tid, T);
    return;
  }
  if (tid == 0) vkey[0] = v ? window_key(v, L.cols, p.ell, first, p.fmask) : 0;
  join_clear<HIST, LIST>(L, nb, p.n, tid, T);
  __syncthreads();

  // 2. the left table: the keys into registers and counted, scan, scatter from the registers
  const word qmask = (word)nb - 1;
  word keys[LC_KPT];
#pragma unroll
  for (int i = 0; i < LC_KPT; ++i) {
    const int r = tid + i * T;
    keys[i]     = 0;
    if (r < nc) {
      keys[i] = window_key(x + (int64_t)r * p.x_stride, L.cols, p.ell, first, p.fmask);
      atomicAdd(&L.off[(uint32_t)(keys[i] & qmask)], 1u);
    }
  }
  join_starts(L, nb, tid, T);
#pragma unroll
  for (int i = 0; i < LC_KPT; ++i) {
    const int r = tid + i * T;
    if (r < nc) {
      const uint32_t pos = atomicAdd(&L.off[(uint32_t)(keys[i] & qmask)], 1u);  // pos < nc: the counts sum to nc
      L.skey[pos]        = keys[i];
      L.sidx[pos]        = (uint16_t)r;
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
    const word key2      = vk ^ window_key(yr, L.cols, p.ell, first, p.fmask);
    const uint32_t bkt   = (uint32_t)(key2 & qmask);
    const uint32_t e_end = L.off[bkt];
    for (uint32_t e = bkt ? L.off[bkt - 1] : 0; e < e_end; ++e) {  // as in rc_kernel; a shared walk taking the match as a callable cost 1-2 VGPRs
      if (L.skey[e] != key2) continue;
      const uint32_t idx = L.sidx[e];
      const word *xr     = x + (int64_t)idx * p.x_stride;
      int wt             = 0;
#pragma unroll
      for (int w = 0; w < JOIN_WT; ++w)
        if (w < p.width) {
          word c = xr[w] ^ yr[w];
          if (v) c ^= v[w];
          if (w == p.width - 1) c &= p.mask;
          wt += __popcll(c);
        }
      join_report<HIST, LIGHT, LIST>(o, L, b, wt, (unsigned long long)(row0 + idx) * (unsigned long long)p.ny + (unsigned long long)j, best);
    }
  }

  // 4. the outputs
  join_output<HIST, LIGHT, LIST>(o, L, b, best, tid, T);
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
  const int64_t have  = mem >= JOIN_BLOCKS_MIN || u.chunks >= JOIN_BLOCKS_MIN ? JOIN_BLOCKS_MIN : mem * u.chunks;  // workgroups before the right list is cut
  const int64_t want  = join_slices_wanted(have);
  int64_t slices      = ny / join_slice_floor(chunk);  // so that ceil(ny / slices) is not below the floor
  if (slices > want) slices = want;
  if (slices < 1) slices = 1;
  u.slice_len = join_slice_held(ny / slices + (ny % slices != 0), chunk);
  u.slices    = ny / u.slice_len + (ny % u.slice_len != 0);
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

JoinKernels<LcArgs> lc_kernels = {{{nullptr, lc_kernel<false, true, false>}, {lc_kernel<true, false, false>, lc_kernel<true, true, false>}},
                                  {{lc_kernel<false, false, true>, lc_kernel<false, true, true>}, {lc_kernel<true, false, true>, lc_kernel<true, true, true>}}};

// ---- the words behind listed keys ---------------------------------------------------------------------------------------------------------

struct LwArgs {
  const word *X, *Y, *V;  // V may be NULL
  int64_t x_stride, x_bs, y_stride, y_bs, v_bs;
  int64_t ny;             // at least 1; o.pairs = nx * ny
  JoinWords o;
};

// join_words with two 32-bit indices per output row: the rank is split ONCE into the rows of X and of Y, the word is V ^ X[i] ^ Y[j]
__global__ __launch_bounds__(JOIN_WORDS_ROWS) void lw_kernel(LwArgs p) {
  __shared__ uint32_t rows[JOIN_WORDS_ROWS][2];
  __shared__ uint8_t live[JOIN_WORDS_ROWS];
  join_words(
      p.o, rows, live,
      [&](unsigned long long r, uint32_t *row) {
        const unsigned long long ri = r / (unsigned long long)p.ny;
        row[0]                      = (uint32_t)ri;
        row[1]                      = (uint32_t)(r - ri * (unsigned long long)p.ny);
      },
      [&](int64_t b, const uint32_t *row, int w) {
        const word c = p.X[b * p.x_bs + (int64_t)row[0] * p.x_stride + w] ^ p.Y[b * p.y_bs + (int64_t)row[1] * p.y_stride + w];
        return p.V ? c ^ p.V[b * p.v_bs + w] : c;
      });
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
  if (unsupported(nx, ny, n) || ell > JOIN_ELL_MAX) return (int)hipErrorNotSupported;
  const int64_t pairs = nx * ny;  // at most 2^40
  if (const int e = join_check_outputs(cols, ell, n, hist, lightest, list, l_bs, cap, count, batch)) return e;
  const int64_t width = width_of(n);
  if (n > 0 && ((nx > 1 && x_stride < width) || (ny > 1 && y_stride < width))) return (int)hipErrorInvalidValue;
  const bool walked = pairs > 0 && n > 0;  // rows are read
  if (batch > 0) {
    if (walked && (!X || !Y)) return (int)hipErrorInvalidValue;
    if (join_outputs_meet(hist, lightest, list, l_bs, cap, count, batch, n, cols, c_bs, ell, rows_span(X, batch, x_bs, nx, x_stride, width),
                          rows_span(Y, batch, y_bs, ny, y_stride, width), rows_span(V, batch, v_bs, 1, 0, width)))
      return (int)hipErrorInvalidValue;
  }
  if (batch == 0) return 0;
  const JoinInit in = join_init_of(hist, lightest, list, l_bs, cap, count, n, cols, c_bs, ell);
  if (!walked) return join_launch_init(st, join_unwalked(in, pairs, w_min), batch);
  const LcUnits u = units_of(nx, ny, batch);
  if (batch > INT64_MAX / u.chunks / u.slices) return (int)hipErrorInvalidValue;
  LcArgs p{};
  p.X = X, p.Y = Y, p.V = V, p.cols = cols, p.x_stride = x_stride, p.x_bs = x_bs, p.y_stride = y_stride, p.y_bs = y_bs, p.v_bs = v_bs, p.c_bs = c_bs;
  p.nx = nx, p.ny = ny, p.n = (int)n, p.width = (int)width, p.ell = (int)ell, p.rows = (int)(nx < LC_CHUNK ? nx : LC_CHUNK);
  p.mask = tail_mask((int)(n & 63)), p.fmask = ell >= 64 ? ~(word)0 : ((word)1 << ell) - 1;
  p.w_min = join_w_min(w_min, n), p.w_max = join_w_max(w_max, n);
  p.hist = hist, p.lightest = lightest, p.list = list, p.count = count, p.l_bs = l_bs, p.cap = cap;
  p.q      = join_bucket_bits(ell, p.rows);
  p.chunks = u.chunks, p.slices = u.slices, p.slice_len = u.slice_len;
  p.atomic = !(u.chunks == 1 && u.slices == 1);
  return join_launch(lc_kernels, LC_LDS_MAX, st, in, batch, p, batch * u.chunks * u.slices, join_threads(p.rows, LC_KPT * BATCH_WAVE_THREADS, p.slice_len),
                     lc_carve((int)n, p.rows, p.q, count != nullptr).total);
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
  const int64_t width = width_of(n);
  if (n > 0 && ((nx > 1 && x_stride < width) || (ny > 1 && y_stride < width))) return (int)hipErrorInvalidValue;
  const bool read = pairs > 0 && n > 0;  // rows of X and Y are read
  if (const int e = join_words_check(n, batch, keys, l_bs, cap, count, W, w_stride, w_bs, skipped, read && (!X || !Y),
                                     rows_span(X, batch, x_bs, nx, x_stride, width), rows_span(Y, batch, y_bs, ny, y_stride, width),
                                     rows_span(V, batch, v_bs, 1, 0, width)))
    return e;
  LwArgs p{};
  p.X = X, p.Y = Y, p.V = n > 0 ? V : nullptr, p.x_stride = x_stride, p.x_bs = x_bs, p.y_stride = y_stride, p.y_bs = y_bs, p.v_bs = v_bs;
  p.ny = ny > 0 ? ny : 1;
  return join_words_launch(lw_kernel, p, n, batch, keys, l_bs, cap, count, W, w_stride, w_bs, skipped, pairs, st);
}

}  // extern "C"
