// rowsums_words_batch.hip -- the words behind the keys of the row-sum enumerations (rowsums_batch.hip, rowsums_collide_batch.hip), written
// out on the device: key (wt << 40) | r names the pair of rank r = r1 * N2 + r2 (S1: t1 of the rows 0 .. k1-1, S2: t2 of the rows
// k1 .. k-1, colexicographic ranks as in subset_rank.h), and row i of W_b becomes V_b ^ rows S1 ^ rows S2 of key i of member b.  With
// t2 = 0, k1 = k the keys are those of m4ri_amd_row_sums_weights_batch_dev.  Only the n valid bits of a row are written.
//
// One kernel, 256 output rows per workgroup, two phases around one barrier:
//   unrank  a thread per output row reads its key, checks it (key < 0 or rank >= N1 * N2: the row is skipped, no row index is formed from
//           it) and unranks both sets ONCE, the t1 + t2 row indices as 16-bit entries into LDS (32 bytes per output row).
//   gather  the lanes regroup: g = the power of two >= words(n) lanes per output row, 64 / g rows of a wave at a time, lane j of a group
//           on word j.  The lanes of a group read consecutive words of V and of each of the t1 + t2 rows of G and write consecutive words of
//           W; the last word goes out under the mask, the bits behind it kept.
// The member's row count m_b = min(max(count[b], 0), cap) is read on the device (count may come from a call still in flight on the
// stream); workgroups beyond it return at once.  skipped[b] is zeroed by a memset on the stream and added to by the waves that meet a bad
// key (one atomic per such wave).  Plain launches on the caller's stream: no allocation, no copy to the host, no synchronisation, no engine
// workspace or lock.
#include <hip/hip_runtime.h>
#include "batch_common.h"
#include "subset_rank.h"
#include "../../include/m4ri_amd.h"

namespace {

constexpr int RW_ROWS = BATCH_WAVE_THREADS;  // output rows per workgroup, a thread each in the first phase
constexpr int RW_SETS = 2 * (int)RS_T_MAX;   // row indices per output row

struct RwArgs {
  const word *G, *V;  // V may be NULL; G too where no row is read
  const int64_t *keys, *count;
  word *W;
  int32_t *skipped;
  int64_t g_stride, g_bs, v_bs, l_bs, cap, w_stride, w_bs;
  int k1, k2, t1, t2, width, group;  // group: lanes per output row, a power of two >= width, 1 where n = 0
  word mask;
  int64_t n2, pairs;                 // N2 and N1 * N2 (0: no key is valid)
  int64_t chunks;                    // workgroups per member: ceil(cap / RW_ROWS)
  int64_t u0;                        // this launch: workgroups from u0 on
};

__global__ __launch_bounds__(RW_ROWS) void rw_kernel(RwArgs p) {
  __shared__ uint16_t rows[RW_ROWS][RW_SETS];
  __shared__ uint8_t live[RW_ROWS];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t u = p.u0 + blockIdx.x, b = u / p.chunks, i0 = (u - b * p.chunks) * RW_ROWS;
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
      unsigned long long r1 = r / (unsigned long long)p.n2, r2 = r - r1 * (unsigned long long)p.n2;
      int e = p.k1, j = 0;
      for (int s = p.t1; s >= 1; --s) rows[tid][j++] = (uint16_t)(e = unrank_step(r1, s, e));
      e = p.k2;
      for (int s = p.t2; s >= 1; --s) rows[tid][j++] = (uint16_t)(p.k1 + (e = unrank_step(r2, s, e)));
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
  const int g = p.group, w = lane & (g - 1), per = 64 / g, t = p.t1 + p.t2;
  if (w >= p.width) return;
  const word *gm = p.G ? p.G + b * p.g_bs : nullptr;
  const word *v  = p.V ? p.V + b * p.v_bs : nullptr;
  word *out      = p.W + b * p.w_bs;
  for (int pass = 0; pass < g; ++pass) {
    const int lr = wave * 64 + pass * per + (lane >> __builtin_ctz(g));
    if (!live[lr]) continue;
    word x = v ? v[w] : 0;
    for (int j = 0; j < t; ++j) x ^= gm[(int64_t)rows[lr][j] * p.g_stride + w];
    store_masked(out + (i0 + lr) * p.w_stride + w, x, w == p.width - 1, p.mask);
  }
}

}  // namespace

extern "C" {

int m4ri_amd_row_sums_words_batch_dev(const word *G, int64_t g_stride, int64_t g_bs, int64_t k, int64_t n, const word *V, int64_t v_bs, int64_t batch,
                                      int64_t k1, int64_t t1, int64_t t2, const int64_t *keys, int64_t l_bs, int64_t cap, const int64_t *count, word *W,
                                      int64_t w_stride, int64_t w_bs, int32_t *skipped, void *stream) {
  hipStream_t st = (hipStream_t)stream;
  if (k < 0 || n < 0 || k1 < 0 || k1 > k || t1 < 0 || t2 < 0 || batch < 0 || g_stride < 0 || g_bs < 0 || v_bs < 0 || l_bs < 0 || cap < 0 || w_stride < 0 ||
      w_bs < 0)
    return (int)hipErrorInvalidValue;
  if (k > RS_K_MAX || n > RS_N_MAX || t1 > RS_T_MAX || t2 > RS_T_MAX) return (int)hipErrorNotSupported;
  const int64_t n1 = binom_capped(k1, t1), n2 = binom_capped(k - k1, t2);
  const __int128 pairs = (__int128)n1 * n2;
  if (pairs > RS_SUMS_MAX) return (int)hipErrorNotSupported;
  const int64_t width = words_of(n);
  if (n > 0 && k > 1 && g_stride < width) return (int)hipErrorInvalidValue;
  if (cap > 1 && w_stride < width) return (int)hipErrorInvalidValue;
  if (batch > 1 && cap > 0 && (l_bs < cap || (n > 0 && (__int128)w_bs < (__int128)(cap - 1) * w_stride + width))) return (int)hipErrorInvalidValue;
  if (batch > 0 && cap > 0) {
    const bool read = pairs > 0 && n > 0 && t1 + t2 >= 1;  // rows of G are read
    if (!keys || (n > 0 && !W) || (read && !G)) return (int)hipErrorInvalidValue;
    const void *outs[2]      = {n > 0 ? W : nullptr, skipped};
    const uintptr_t bytes[2] = {n > 0 ? member_span_bytes(batch, w_bs, cap, w_stride, width) : 0, (uintptr_t)batch * 4};
    if (outs[0] && outs[1] && spans_meet(outs[0], bytes[0], outs[1], bytes[1])) return (int)hipErrorInvalidValue;
    for (int o = 0; o < 2; ++o) {
      if (!outs[o]) continue;
      if (k > 0 && n > 0 && G && spans_meet(outs[o], bytes[o], G, member_span_bytes(batch, g_bs, k, g_stride, width))) return (int)hipErrorInvalidValue;
      if (V && n > 0 && spans_meet(outs[o], bytes[o], V, member_span_bytes(batch, v_bs, 1, 0, width))) return (int)hipErrorInvalidValue;
      if (spans_meet(outs[o], bytes[o], keys, ((uintptr_t)(batch - 1) * (uintptr_t)l_bs + (uintptr_t)cap) * 8)) return (int)hipErrorInvalidValue;
      if (count && spans_meet(outs[o], bytes[o], count, (uintptr_t)batch * 8)) return (int)hipErrorInvalidValue;
    }
  }
  if (batch == 0) return 0;
  if (skipped) HIPTRY(hipMemsetAsync(skipped, 0, (size_t)batch * 4, st));  // written whole: 0 for a clean member, and at cap = 0
  if (cap == 0) return 0;
  RwArgs p{};
  p.G = G, p.V = n > 0 ? V : nullptr, p.keys = keys, p.count = count, p.W = W, p.skipped = skipped;
  p.g_stride = g_stride, p.g_bs = g_bs, p.v_bs = v_bs, p.l_bs = l_bs, p.cap = cap, p.w_stride = w_stride, p.w_bs = w_bs;
  p.k1 = (int)k1, p.k2 = (int)(k - k1), p.t1 = (int)t1, p.t2 = (int)t2, p.width = (int)width, p.group = 1;
  while (p.group < width) p.group <<= 1;
  p.mask = tail_mask((int)(n & 63)), p.n2 = n2, p.pairs = (int64_t)pairs;
  p.chunks = (cap + RW_ROWS - 1) / RW_ROWS;
  if (batch > INT64_MAX / p.chunks) return (int)hipErrorInvalidValue;
  return launch_chunked(batch * p.chunks, BATCH_CHUNK, [&](int64_t u0, int64_t nu) {
    p.u0 = u0;
    hipLaunchKernelGGL(rw_kernel, dim3((unsigned)nu), dim3(RW_ROWS), 0, st, p);
  });
}

}  // extern "C"
