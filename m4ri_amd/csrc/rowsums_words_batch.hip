// rowsums_words_batch.hip -- the words behind the keys of the row-sum enumerations (rowsums_batch.hip, rowsums_collide_batch.hip), written
// out on the device: key (wt << 40) | r names the pair of rank r = r1 * N2 + r2 (S1: t1 of the rows 0 .. k1-1, S2: t2 of the rows
// k1 .. k-1, colexicographic ranks as in subset_rank.h), and row i of W_b becomes V_b ^ rows S1 ^ rows S2 of key i of member b.  With
// t2 = 0, k1 = k the keys are those of m4ri_amd_row_sums_weights_batch_dev.  Only the n valid bits of a row are written.
//
// One kernel, 256 output rows per workgroup, two phases around one barrier (join_common.h: join_words, shared with the words call of
// lists_collide_batch.hip):
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
#include "join_common.h"
#include "subset_rank.h"
#include "../../include/m4ri_amd.h"

namespace {

constexpr int RW_SETS = 2 * (int)RS_T_MAX;  // row indices per output row

struct RwArgs {
  const word *G, *V;  // V may be NULL; G too where no row is read
  int64_t g_stride, g_bs, v_bs;
  int k1, k2, t1, t2;
  int64_t n2;         // N2; o.pairs = N1 * N2
  JoinWords o;
};

__global__ __launch_bounds__(JOIN_WORDS_ROWS) void rw_kernel(RwArgs p) {
  __shared__ uint16_t rows[JOIN_WORDS_ROWS][RW_SETS];
  __shared__ uint8_t live[JOIN_WORDS_ROWS];
  join_words(
      p.o, rows, live,
      [&](unsigned long long r, uint16_t *row) {
        unsigned long long r1 = r / (unsigned long long)p.n2, r2 = r - r1 * (unsigned long long)p.n2;
        int e = p.k1, j = 0;
        for (int s = p.t1; s >= 1; --s) row[j++] = (uint16_t)(e = unrank_step(r1, s, e));
        e = p.k2;
        for (int s = p.t2; s >= 1; --s) row[j++] = (uint16_t)(p.k1 + (e = unrank_step(r2, s, e)));
      },
      [&](int64_t b, const uint16_t *row, int w) {
        word x = p.V ? p.V[b * p.v_bs + w] : 0;
        for (int j = 0; j < p.t1 + p.t2; ++j) x ^= p.G[b * p.g_bs + (int64_t)row[j] * p.g_stride + w];  // G is NULL only where no row is read
        return x;
      });
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
  const int64_t width = width_of(n);
  if (n > 0 && k > 1 && g_stride < width) return (int)hipErrorInvalidValue;
  const bool read = pairs > 0 && n > 0 && t1 + t2 >= 1;  // rows of G are read
  if (const int e = join_words_check(n, batch, keys, l_bs, cap, count, W, w_stride, w_bs, skipped, read && !G, rows_span(G, batch, g_bs, k, g_stride, width),
                                     rows_span(V, batch, v_bs, 1, 0, width)))
    return e;
  RwArgs p{};
  p.G = G, p.V = n > 0 ? V : nullptr, p.g_stride = g_stride, p.g_bs = g_bs, p.v_bs = v_bs;
  p.k1 = (int)k1, p.k2 = (int)(k - k1), p.t1 = (int)t1, p.t2 = (int)t2, p.n2 = n2;
  return join_words_launch(rw_kernel, p, n, batch, keys, l_bs, cap, count, W, w_stride, w_bs, skipped, (int64_t)pairs, st);
}

}  // extern "C"
