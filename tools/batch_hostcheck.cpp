// The argument checks of every batched entry point (the *_batch_dev calls of m4ri_amd/csrc/*_batch.hip) and their host helpers (plan,
// units, slices, scratch size) as a stand-alone program for the host sanitizers: every call returns before any HIP call, so no GPU is
// needed and no pointer is dereferenced; what the launchers forward to beyond their checks is stubbed below and never reached.  The
// expected codes are what each call's documented rule gives over the integers (include/m4ri_amd.h; DESIGN.md 3.16 for the order of the
// checks), sizes, strides and batch strides of INT64_MAX and the in-range 2^40 x 2^40 members included: nothing overflows on the way.
// From the repository root:
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
//         -o batch_hostcheck m4ri_amd/csrc/*_batch.hip tools/batch_hostcheck.cpp && ./batch_hostcheck
#include <hip/hip_runtime.h>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include "../include/m4ri_amd.h"
#include "../m4ri_amd/csrc/gf2_internal.h"
#define EXPECT(expr, want) do { long got_ = (long)(expr); if (got_ != (long)(want)) { printf("FAIL %s = %ld, want %ld\n", #expr, got_, (long)(want)); ++fails; } ++n; } while (0)
static int fails = 0, n = 0;

// ---- the join family: both joins, their words calls and the sort ------------------------------------------------------------------------
static void join_family() {
  word *X = (word *)(1ull << 20), *Y = (word *)(1ull << 22), *V = (word *)(1ull << 24), *W = (word *)(1ull << 32);
  int32_t *C = (int32_t *)(1ull << 26), *S = (int32_t *)(1ull << 33);
  int64_t *H = (int64_t *)(1ull << 28), *L = (int64_t *)(1ull << 29), *K = (int64_t *)(1ull << 30), *N = (int64_t *)(1ull << 31);
  // the join of two lists and its words
  EXPECT(m4ri_amd_lists_collide_batch_dev(X, 1, 4, 4, Y, 1, 3, 3, 64, V, 1, 0, C, 3, 3, 0, 64, H, L, K, 6, 5, N, nullptr), 0);
  EXPECT(m4ri_amd_lists_collide_batch_dev(X, 1, 4, 4, Y, 1, 3, 3, 64, V, 1, 2, C, 3, 3, 0, 64, nullptr, nullptr, nullptr, 6, 5, nullptr, nullptr), 1);
  EXPECT(m4ri_amd_lists_collide_batch_dev(X, 1, 4, 4, Y, 1, 3, 3, 64, V, 1, 2, C, 3, 3, 0, 64, H, L, (int64_t *)X, 6, 5, N, nullptr), 1);
  EXPECT(m4ri_amd_lists_collide_batch_dev(X, 1, 4, -1, Y, 1, 3, 3, 64, V, 1, 2, C, 3, 3, 0, 64, H, L, K, 6, 5, N, nullptr), 1);
  EXPECT(m4ri_amd_lists_collide_batch_dev(nullptr, 1, 4, 4, Y, 1, 3, 3, 64, V, 1, 2, C, 3, 3, 0, 64, H, L, K, 6, 5, N, nullptr), 1);
  EXPECT(m4ri_amd_lists_collide_batch_dev(X, 1, 4, 4, Y, 1, 3, 3, 1025, V, 1, 2, C, 3, 3, 0, 64, H, L, K, 6, 5, N, nullptr), 801);
  EXPECT(m4ri_amd_lists_collide_batch_dev(X, 1, 4, 4, Y, 1, 3, 3, 64, V, 1, 2, C, 65, 65, 0, 64, H, L, K, 6, 5, N, nullptr), 801);
  EXPECT(m4ri_amd_lists_collide_batch_dev(X, 1, 1 << 20, 1 << 20, Y, 1, 1 << 20, 1 << 20, 64, V, 1, 0, C, 3, 3, 0, 64, H, L, K, 6, 5, N, nullptr), 0);
  EXPECT(m4ri_amd_lists_collide_batch_dev(X, 1, 1 << 20, (1 << 20) + 1, Y, 1, 1 << 20, 1 << 20, 64, V, 1, 0, C, 3, 3, 0, 64, H, L, K, 6, 5, N, nullptr), 801);
  EXPECT(m4ri_amd_lists_collide_batch_dev(X, 1, 4, INT64_MAX, Y, 1, 3, INT64_MAX, 64, V, 1, 2, C, 3, 3, 0, 64, H, L, K, 6, 5, N, nullptr), 801);
  EXPECT(m4ri_amd_lists_collide_batch_dev(X, INT64_MAX, INT64_MAX, 4, Y, 1, 3, 3, 64, V, 1, 0, C, 3, 3, 0, 64, H, L, K, INT64_MAX, INT64_MAX, N, nullptr), 0);
  EXPECT(m4ri_amd_lists_collide_batch_dev(X, 1, 4, 4, Y, 1, 3, 3, 64, V, 1, 2, C, 3, 3, 0, 64, H, L, K, 4, 5, N, nullptr), 1);           // l_bs < cap
  EXPECT(m4ri_amd_lists_collide_batch_dev(X, 1, 4, 4, Y, 1, 3, 3, 64, V, 1, 2, C, 3, 3, 0, 64, (int64_t *)(C + 4), L, K, 6, 5, N, nullptr), 1);   // hist on the windows
  EXPECT(m4ri_amd_lists_words_batch_dev(X, 1, 4, 4, Y, 1, 3, 3, 64, V, 1, 0, K, 6, 5, N, W, 2, 12, S, nullptr), 0);
  EXPECT(m4ri_amd_lists_words_batch_dev(X, 1, 4, 4, Y, 1, 3, 3, 64, V, 1, 2, K, 4, 5, N, W, 2, 12, S, nullptr), 1);
  EXPECT(m4ri_amd_lists_words_batch_dev(X, 1, 4, 4, Y, 1, 3, 3, 64, V, 1, 2, K, 6, 5, N, (word *)K, 2, 12, S, nullptr), 1);
  EXPECT(m4ri_amd_lists_words_batch_dev(X, 1, 4, 4, Y, 1, 3, 3, 64, V, 1, 2, K, 6, 5, N, W, 2, 12, (int32_t *)W, nullptr), 1);
  EXPECT(m4ri_amd_lists_words_batch_dev(X, 1, 4, 4, Y, 1, 3, 3, 64, V, 1, 2, nullptr, 6, 5, N, W, 2, 12, S, nullptr), 1);
  EXPECT(m4ri_amd_lists_words_batch_dev(X, 1, 4, 1ll << 31, Y, 1, 3, 3, 64, V, 1, 2, K, 6, 5, N, W, 2, 12, S, nullptr), 801);
  EXPECT(m4ri_amd_lists_words_batch_dev(X, 1, 4, 4, Y, 1, 3, 3, 64, V, 1, 2, K, 6, 5, N, W, INT64_MAX, INT64_MAX, S, nullptr), 1);
  EXPECT(m4ri_amd_plan_lists_collide_batch(4, 3, 64, 3, 2), 0);
  EXPECT(m4ri_amd_plan_lists_collide_batch(-1, 3, 64, 3, 2), -1);
  EXPECT(m4ri_amd_plan_lists_collide_batch(INT64_MAX, INT64_MAX, 64, 3, INT64_MAX), 1);
  int64_t c = 0, ch = 0, sl = 0;
  EXPECT(m4ri_amd_lists_collide_units(INT64_MAX, INT64_MAX, 64, 3, INT64_MAX, &c, &ch, &sl), 0);
  EXPECT(m4ri_amd_lists_collide_units((1ll << 31) - 1, 512, 64, 3, 1, &c, &ch, &sl), 0);
  EXPECT(ch, ((1ll << 31) - 1 + c - 1) / c);
  EXPECT(m4ri_amd_lists_collide_units(1, (1ll << 31) - 1, 1024, 64, 1, &c, &ch, &sl), 0);
  EXPECT(m4ri_amd_lists_collide_units(5, 5, 64, 3, 1, nullptr, nullptr, nullptr), 0);
  EXPECT(m4ri_amd_lists_collide_units(5, -5, 64, 3, 1, &c, &ch, &sl), -1);
  // the join of the row sums of a generator: two members of 4 x 64 at X, windows of 3 entries
  word *G = X;
  EXPECT(m4ri_amd_row_sums_collide_batch_dev(G, 1, 4, 4, 64, V, 1, 0, 2, 1, 1, C, 3, 3, 0, H, L, nullptr), 0);
  EXPECT(m4ri_amd_row_sums_collide_batch_dev(G, 1, 4, 4, 64, V, 1, 2, 2, 1, 1, C, 3, 3, 0, nullptr, nullptr, nullptr), 1);
  EXPECT(m4ri_amd_row_sums_collide_batch_dev(G, 1, 4, 4, 64, V, 1, 2, 2, 1, 1, C, 3, 3, 0, (int64_t *)G, L, nullptr), 1);
  EXPECT(m4ri_amd_row_sums_collide_batch_dev(G, 1, 4, 4, 64, V, 1, 2, 2, 1, 1, C, 3, 3, 0, (int64_t *)(C + 4), L, nullptr), 1);
  EXPECT(m4ri_amd_row_sums_collide_batch_dev(G, 1, 4, 4, 64, V, 1, 2, 2, 1, 1, C, 3, 3, 0, H, (int64_t *)V + 1, nullptr), 1);
  EXPECT(m4ri_amd_row_sums_collide_batch_dev(G, 1, 4, -1, 64, V, 1, 2, 2, 1, 1, C, 3, 3, 0, H, L, nullptr), 1);
  EXPECT(m4ri_amd_row_sums_collide_batch_dev(G, 1, 4, 4, 64, V, 1, 2, 5, 1, 1, C, 3, 3, 0, H, L, nullptr), 1);                         // k1 > k
  EXPECT(m4ri_amd_row_sums_collide_batch_dev(nullptr, 1, 4, 4, 64, V, 1, 2, 2, 1, 1, C, 3, 3, 0, H, L, nullptr), 1);
  EXPECT(m4ri_amd_row_sums_collide_batch_dev(G, 0, 4, 4, 64, V, 1, 2, 2, 1, 1, C, 3, 3, 0, H, L, nullptr), 1);                         // g_stride < words(n)
  EXPECT(m4ri_amd_row_sums_collide_batch_dev(G, 1, 4, 4, 10, V, 1, 2, 2, 1, 1, nullptr, 3, 11, 0, H, L, nullptr), 1);                  // ell > n, no window
  EXPECT(m4ri_amd_row_sums_collide_batch_dev(G, 17, 4, 4, 1025, V, 1, 2, 2, 1, 1, C, 3, 3, 0, H, L, nullptr), 801);
  EXPECT(m4ri_amd_row_sums_collide_batch_dev(G, 1, 4, 4, 64, V, 1, 2, 2, 1, 1, C, 65, 65, 0, H, L, nullptr), 801);
  EXPECT(m4ri_amd_row_sums_collide_batch_dev(G, 1, 4, 1024, 64, V, 1, 2, 512, 2, 2, C, 3, 3, 0, H, L, nullptr), 801);                  // N1 > 8192
  EXPECT(m4ri_amd_row_sums_collide_batch_dev(G, 1, 4, 1024, 64, V, 1, 2, 24, 3, 4, C, 3, 3, 0, H, L, nullptr), 801);                   // 8.4e13 pairs
  EXPECT(m4ri_amd_row_sums_collide_batch_dev(G, 1, 4, 200, 64, V, 1, 0, 128, 2, 1, C, 3, 3, 0, H, L, nullptr), 0);
  EXPECT(m4ri_amd_row_sums_collide_batch_dev(G, 1, 4, 200, 64, V, 1, 0, 129, 2, 1, C, 3, 3, 0, H, L, nullptr), 801);
  EXPECT(m4ri_amd_row_sums_collide_list_batch_dev(G, 1, 4, 4, 64, V, 1, 0, 2, 1, 1, C, 3, 3, 0, 64, H, L, K, 6, 5, N, nullptr), 0);
  EXPECT(m4ri_amd_row_sums_collide_list_batch_dev(G, 1, 4, 4, 64, V, 1, 0, 2, 1, 1, C, 3, 3, 0, 64, H, L, K, INT64_MAX, INT64_MAX, N, nullptr), 0);
  EXPECT(m4ri_amd_row_sums_collide_list_batch_dev(G, 1, 4, 4, 64, V, 1, 2, 2, 1, 1, C, 3, 3, 0, 64, H, L, K, 4, 5, N, nullptr), 1);           // l_bs < cap
  EXPECT(m4ri_amd_row_sums_collide_list_batch_dev(G, 1, 4, 4, 64, V, 1, 2, 2, 1, 1, C, 3, 3, 0, 64, H, L, K, 6, 5, nullptr, nullptr), 1);     // a list without a count
  EXPECT(m4ri_amd_row_sums_collide_list_batch_dev(G, 1, 4, 4, 64, V, 1, 2, 2, 1, 1, C, 3, 3, 0, 64, H, L, nullptr, 6, 5, N, nullptr), 1);     // a count without a list
  EXPECT(m4ri_amd_row_sums_collide_list_batch_dev(G, 1, 4, 4, 64, V, 1, 2, 2, 1, 1, C, 3, 3, 0, 64, H, L, K, 6, -1, N, nullptr), 1);
  EXPECT(m4ri_amd_row_sums_collide_list_batch_dev(G, 1, 4, 4, 64, V, 1, 2, 2, 1, 1, C, 3, 3, 0, 64, H, L, (int64_t *)G, 6, 5, N, nullptr), 1);
  EXPECT(m4ri_amd_row_sums_collide_list_batch_dev(G, 1, 4, 4, 64, V, 1, 2, 2, 1, 1, C, 3, 3, 0, 64, H, L, K, 6, 5, K + 10, nullptr), 1);      // count on the list's last key
  EXPECT(m4ri_amd_row_sums_collide_list_batch_dev(G, 1, 4, 4, 64, V, 1, 2, 2, 1, 1, C, 3, 3, 0, 64, H, L, K, 100, 5, K + 104, nullptr), 1);   // members 100 apart
  EXPECT(m4ri_amd_row_sums_collide_list_batch_dev(G, 1, 4, 4, 64, V, 1, 2, 2, 1, 1, C, 3, 3, 0, 64, N, L, N + 1, 6, 0, N, nullptr), 1);       // hist on count, no list
  EXPECT(m4ri_amd_row_sums_collide_list_batch_dev(G, 1, 4, 1025, 64, V, 1, 2, 2, 1, 1, C, 3, 3, 0, 64, H, L, nullptr, 6, 0, N, nullptr), 801);
  EXPECT(m4ri_amd_row_sums_words_batch_dev(G, 1, 4, 4, 64, V, 1, 0, 2, 1, 1, K, 6, 5, N, W, 2, 12, S, nullptr), 0);
  EXPECT(m4ri_amd_row_sums_words_batch_dev(G, 1, 4, 4, 64, V, 1, 0, 2, 1, 1, K, 6, 5, N, W, INT64_MAX, INT64_MAX, S, nullptr), 0);
  EXPECT(m4ri_amd_row_sums_words_batch_dev(G, 1, 4, 4, 64, V, 1, 2, 2, 1, 1, K, 4, 5, N, W, 2, 12, S, nullptr), 1);                    // l_bs < cap
  EXPECT(m4ri_amd_row_sums_words_batch_dev(G, 1, 4, 4, 64, V, 1, 2, 2, 1, 1, K, 6, 5, N, W, 2, 8, S, nullptr), 1);                     // w_bs too small
  EXPECT(m4ri_amd_row_sums_words_batch_dev(G, 1, 4, 4, 64, V, 1, 2, 2, 1, 1, K, 6, 5, N, W, 0, 12, S, nullptr), 1);                    // w_stride < words(n)
  EXPECT(m4ri_amd_row_sums_words_batch_dev(G, 1, 4, 4, 64, V, 1, 2, 2, 1, 1, K, 6, 5, N, W, INT64_MAX, INT64_MAX, S, nullptr), 1);
  EXPECT(m4ri_amd_row_sums_words_batch_dev(G, 1, 4, 4, 64, V, 1, 2, 2, 1, 1, nullptr, 6, 5, N, W, 2, 12, S, nullptr), 1);
  EXPECT(m4ri_amd_row_sums_words_batch_dev(G, 1, 4, 4, 64, V, 1, 2, 2, 1, 1, K, 6, 5, N, nullptr, 2, 12, S, nullptr), 1);
  EXPECT(m4ri_amd_row_sums_words_batch_dev(nullptr, 1, 4, 4, 64, V, 1, 2, 2, 1, 1, K, 6, 5, N, W, 2, 12, S, nullptr), 1);
  EXPECT(m4ri_amd_row_sums_words_batch_dev(G, 1, 4, 4, 64, V, 1, 2, 2, 1, 1, K, 6, 5, N, G, 2, 12, S, nullptr), 1);
  EXPECT(m4ri_amd_row_sums_words_batch_dev(G, 1, 4, 4, 64, V, 1, 2, 2, 1, 1, K, 6, 5, N, (word *)(K + 10), 2, 12, S, nullptr), 1);     // W on the last key
  EXPECT(m4ri_amd_row_sums_words_batch_dev(G, 1, 4, 4, 64, V, 1, 2, 2, 1, 1, K, 6, 5, N, W, 2, 12, (int32_t *)W - 1, nullptr), 1);     // skipped's end on W
  EXPECT(m4ri_amd_row_sums_words_batch_dev(G, 1, 4, 4, 64, V, 1, 2, 2, 9, 1, K, 6, 5, N, W, 2, 12, S, nullptr), 801);
  EXPECT(m4ri_amd_row_sums_words_batch_dev(G, 1, 4, 1024, 64, V, 1, 2, 512, 3, 3, K, 6, 5, N, W, 2, 12, S, nullptr), 801);
  EXPECT(m4ri_amd_row_sums_words_batch_dev(G, 1, 4, 1024, 64, V, 1, 0, 512, 2, 2, K, 6, 5, N, W, 2, 12, S, nullptr), 0);               // no bound on N1
  EXPECT(m4ri_amd_plan_row_sums_collide_batch(8, 64, 4, 2, 2, 4), 0);
  EXPECT(m4ri_amd_plan_row_sums_collide_batch(1024, 64, 128, 2, 2, 16), 1);
  EXPECT(m4ri_amd_plan_row_sums_collide_batch(246, 64, 64, 2, 2, 8), 0);
  EXPECT(m4ri_amd_plan_row_sums_collide_batch(247, 64, 64, 2, 2, 8), 1);
  EXPECT(m4ri_amd_plan_row_sums_collide_batch(8, 64, 9, 2, 2, 4), -1);
  EXPECT(m4ri_amd_plan_row_sums_collide_batch(8, 0, 4, 2, 2, 0), 0);
  EXPECT(m4ri_amd_row_sums_collide_slices(8, 64, 4, 2, 2, 4, 1), 1);
  EXPECT(m4ri_amd_row_sums_collide_slices(44, 64, 4, 2, 2, 4, 1024), 1);
  EXPECT(m4ri_amd_row_sums_collide_slices(44, 64, 4, 2, 2, 4, 0), 4);
  EXPECT(m4ri_amd_row_sums_collide_slices(152, 256, 128, 2, 2, 10, 1), 1);
  EXPECT(m4ri_amd_row_sums_collide_slices(328, 256, 128, 2, 2, 10, 1), (200 * 199 / 2 + 8127) / 8128);
  EXPECT(m4ri_amd_row_sums_collide_slices(1024, 64, 2, 1, 3, 8, 1), 1024);
  EXPECT(m4ri_amd_row_sums_collide_slices(1024, 64, 2, 1, 3, 8, 512), 2);
  EXPECT(m4ri_amd_row_sums_collide_slices(1024, 64, 2, 1, 3, 8, 4096), 1);
  EXPECT(m4ri_amd_row_sums_collide_slices(400, 64, 129, 2, 2, 4, 1), 0);
  EXPECT(m4ri_amd_row_sums_collide_slices(1024, 64, 1, 1, 4, 8, INT64_MAX), (45367119105ll + (1ll << 32) - 2) / ((1ll << 32) - 1));  // C(1023, 4) in slices below 2^32
  EXPECT(m4ri_amd_row_sums_collide_slices(8, 64, 4, 2, 2, 4, -1), -1);
  // the sort of the rows of a list: two members of 6 rows of 64 bits at X, counts at N, windows at C, order / uniq / mult at K, H, L (l_bs 7), ucount at N + 8
  int64_t *U = N + 8;
  void *T = (void *)(1ull << 34);
  EXPECT(m4ri_amd_sort_rows_batch_dev(X, 1, 6, 6, 64, N, 0, C, 3, 3, K, U, H, L, 7, nullptr, 0, nullptr), 0);
  EXPECT(m4ri_amd_sort_rows_batch_dev(X, 1, 6, -1, 64, N, 2, C, 3, 3, K, U, H, L, 7, nullptr, 0, nullptr), 1);
  EXPECT(m4ri_amd_sort_rows_batch_dev(X, 1, 6, 6, 64, N, 2, C, 3, 3, K, U, H, L, 7, nullptr, -1, nullptr), 1);
  EXPECT(m4ri_amd_sort_rows_batch_dev(X, 0, 6, 6, 64, N, 2, C, 3, 3, K, U, H, L, 7, nullptr, 0, nullptr), 1);                 // x_stride < words(n)
  EXPECT(m4ri_amd_sort_rows_batch_dev(X, 1, 6, 6, 64, N, 2, C, 3, 3, K, U, H, L, 5, nullptr, 0, nullptr), 1);                 // l_bs < nx
  EXPECT(m4ri_amd_sort_rows_batch_dev(nullptr, 1, 6, 6, 64, N, 2, C, 3, 3, K, U, H, L, 7, nullptr, 0, nullptr), 1);
  EXPECT(m4ri_amd_sort_rows_batch_dev(X, 1, 6, 6, 64, N, 2, C, 3, 3, nullptr, nullptr, nullptr, nullptr, 7, nullptr, 0, nullptr), 1);   // no output
  EXPECT(m4ri_amd_sort_rows_batch_dev(X, 1, 6, 6, 64, N, 2, C, 3, 3, K, nullptr, H, nullptr, 7, nullptr, 0, nullptr), 1);      // uniq without ucount
  EXPECT(m4ri_amd_sort_rows_batch_dev(X, 1, 6, 6, 64, N, 2, C, 3, 3, K, U, nullptr, L, 7, nullptr, 0, nullptr), 1);            // mult without uniq
  EXPECT(m4ri_amd_sort_rows_batch_dev(X, 1, 6, 6, 2, N, 2, nullptr, 3, 3, K, U, H, L, 7, nullptr, 0, nullptr), 1);             // ell > n, no window
  EXPECT(m4ri_amd_sort_rows_batch_dev(X, 1, 6, 6, 64, N, 2, C, 3, 3, (int64_t *)X + 11, U, H, L, 7, nullptr, 0, nullptr), 1);  // order on X's last word
  EXPECT(m4ri_amd_sort_rows_batch_dev(X, 1, 6, 6, 64, N, 2, C, 3, 3, K, N + 1, H, L, 7, nullptr, 0, nullptr), 1);              // ucount on xcount
  EXPECT(m4ri_amd_sort_rows_batch_dev(X, 1, 6, 6, 64, N, 2, C, 3, 3, K, U, K + 12, L, 7, nullptr, 0, nullptr), 1);             // uniq on order's last entry
  EXPECT(m4ri_amd_sort_rows_batch_dev(X, 1, 6, 6, 64, N, 2, C, 3, 3, K, U, (int64_t *)(C + 4), L, 7, nullptr, 0, nullptr), 1); // uniq on the windows
  EXPECT(m4ri_amd_sort_rows_batch_dev(X, 17, 6, 6, 1025, N, 2, C, 3, 3, K, U, H, L, 7, nullptr, 0, nullptr), 801);
  EXPECT(m4ri_amd_sort_rows_batch_dev(X, 1, 6, 6, 64, N, 2, C, 65, 65, K, U, H, L, 7, nullptr, 0, nullptr), 801);
  EXPECT(m4ri_amd_sort_rows_batch_dev(X, 1, 6, (1ll << 24) + 1, 64, N, 0, C, 3, 3, K, U, H, L, 1ll << 25, nullptr, 0, nullptr), 801);
  EXPECT(m4ri_amd_sort_rows_batch_dev(X, 1, 6, INT64_MAX, 64, N, 2, C, 3, 3, K, U, H, L, INT64_MAX, nullptr, 0, nullptr), 801);
  EXPECT(m4ri_amd_sort_rows_batch_dev(X, 1, 1 << 24, 1 << 24, 64, N, 0, C, 3, 3, K, U, H, L, 1 << 24, nullptr, 0, nullptr), 0);
  const int64_t need = m4ri_amd_sort_rows_scratch_bytes(10000, 64, 3, 2);
  EXPECT(need, (2 * (16384 * 13 + 16 * 4 + 4) + 15) / 16 * 16);
  EXPECT(m4ri_amd_sort_rows_batch_dev(X, 1, 10000, 10000, 64, N, 2, C, 3, 3, K, U, H, L, 10000, nullptr, need, nullptr), 1);   // no scratch
  EXPECT(m4ri_amd_sort_rows_batch_dev(X, 1, 10000, 10000, 64, N, 2, C, 3, 3, K, U, H, L, 10000, T, need - 1, nullptr), 1);     // too small
  EXPECT(m4ri_amd_sort_rows_batch_dev(X, 1, 10000, 10000, 64, N, 2, C, 3, 3, K, U, H, L, 10000, (char *)T + 4, need, nullptr), 1);   // misaligned
  EXPECT(m4ri_amd_sort_rows_batch_dev(X, 1, 10000, 10000, 64, N, 2, C, 3, 3, K, U, H, L, 10000, (char *)U - need + 8, need, nullptr), 1);   // its end on ucount
  EXPECT(m4ri_amd_sort_rows_batch_dev(X, 1, 10000, 10000, 64, N, 0, C, 3, 3, K, U, H, L, 10000, nullptr, 0, nullptr), 0);
  EXPECT(m4ri_amd_sort_rows_scratch_bytes(8192, 1024, 64, 1000), 0);
  EXPECT(m4ri_amd_sort_rows_scratch_bytes(1 << 24, 1024, 64, INT64_MAX), -1);
  EXPECT(m4ri_amd_sort_rows_scratch_bytes(INT64_MAX, 1024, 64, INT64_MAX), -1);
  EXPECT(m4ri_amd_sort_rows_scratch_bytes(-1, 64, 3, 2), -1);
  EXPECT(m4ri_amd_plan_sort_rows_batch(8192, 64, 3, 2), 0);
  EXPECT(m4ri_amd_plan_sort_rows_batch(8193, 64, 3, 2), 1);
  EXPECT(m4ri_amd_plan_sort_rows_batch(INT64_MAX, 64, 3, INT64_MAX), 1);
  EXPECT(m4ri_amd_plan_sort_rows_batch(5, 64, -3, 2), -1);
  int64_t sc = 0, sp = 0, sl2 = 0;
  EXPECT(m4ri_amd_sort_rows_units(4 * 8192 + 3, 64, 3, 1, &sc, &sp, &sl2), 0);
  EXPECT(sc, 8192);
  EXPECT(sp, 65536);
  EXPECT(sl2, 1 + (1 + 2 + 3) + 3 + 4);
  EXPECT(m4ri_amd_sort_rows_units(INT64_MAX, 64, 3, INT64_MAX, &sc, &sp, &sl2), 0);
  EXPECT(m4ri_amd_sort_rows_units(0, 0, 0, 0, nullptr, nullptr, nullptr), 0);
  EXPECT(m4ri_amd_sort_rows_units(5, 64, 3, -1, &sc, &sp, &sl2), -1);
}

// ---- the pivot exchange -------------------------------------------------------------------------------------------------------------------
static void pivot_exchange() {
  // D: 2 members of 4 x 64 (64 bytes); pivots 2 x 4 entries (32 bytes); rank 8 bytes; req 2 x 3 pairs (48 bytes); order 2 x 64 entries; done 8 bytes
  word *D = (word *)(1ull << 20);
  int32_t *P = (int32_t *)(1ull << 22), *R = (int32_t *)(1ull << 24), *Q = (int32_t *)(1ull << 26), *O = (int32_t *)(1ull << 28), *N = (int32_t *)(1ull << 30);
  auto at = [](void *p, long bytes) { return (int32_t *)((char *)p + bytes); };
  EXPECT(m4ri_amd_pivot_exchange_batch_dev(D, 1, 4, 4, 64, 4, P, R, 0, Q, 6, 3, 7, O, 64, 64, N, nullptr), 0);                 // batch = 0
  EXPECT(m4ri_amd_pivot_exchange_batch_dev(nullptr, 1, 4, 4, 64, 4, nullptr, nullptr, 0, nullptr, 0, 0, 7, nullptr, 0, 0, nullptr, nullptr), 0);
  EXPECT(m4ri_amd_pivot_exchange_batch_dev(D, 1, 4, -1, 64, 0, P, R, 2, Q, 6, 3, 7, O, 64, 64, N, nullptr), 1);
  EXPECT(m4ri_amd_pivot_exchange_batch_dev(D, 1, 4, 4, 64, 4, P, R, -1, Q, 6, 3, 7, O, 64, 64, N, nullptr), 1);
  EXPECT(m4ri_amd_pivot_exchange_batch_dev(D, 1, 4, 4, 64, 4, P, R, 2, Q, 6, -1, 7, O, 64, 64, N, nullptr), 1);                // steps < 0
  EXPECT(m4ri_amd_pivot_exchange_batch_dev(D, 1, 4, 4, 64, 5, P, R, 2, Q, 6, 3, 7, O, 64, 64, N, nullptr), 1);                 // pivot_rows > nrows
  EXPECT(m4ri_amd_pivot_exchange_batch_dev(D, 1, 4, 4, 64, 4, P, R, 2, Q, 6, 3, 7, O, 65, 65, N, nullptr), 1);                 // olen > ncols
  EXPECT(m4ri_amd_pivot_exchange_batch_dev(D, 0, 4, 4, 64, 4, P, R, 2, Q, 6, 3, 7, O, 64, 64, N, nullptr), 1);                 // d_stride < words
  EXPECT(m4ri_amd_pivot_exchange_batch_dev(D, 1, 3, 4, 64, 4, P, R, 2, Q, 6, 3, 7, O, 64, 64, N, nullptr), 1);                 // overlapping members
  EXPECT(m4ri_amd_pivot_exchange_batch_dev(D, 1, 4, 4, 64, 4, P, R, 2, Q, 5, 3, 7, O, 64, 64, N, nullptr), 1);                 // r_bs < 2 steps
  EXPECT(m4ri_amd_pivot_exchange_batch_dev(D, 1, 4, 4, 64, 4, P, R, 2, Q, 6, INT64_MAX, 7, O, 64, 64, N, nullptr), 1);         // and no overflow on the way
  EXPECT(m4ri_amd_pivot_exchange_batch_dev(D, 1, 4, 4, 64, 4, P, R, 2, Q, 6, 3, 7, O, 63, 64, N, nullptr), 1);                 // o_bs < olen
  EXPECT(m4ri_amd_pivot_exchange_batch_dev(nullptr, 1, 4, 4, 64, 4, P, R, 2, Q, 6, 3, 7, O, 64, 64, N, nullptr), 1);
  EXPECT(m4ri_amd_pivot_exchange_batch_dev(D, 1, 4, 4, 64, 4, nullptr, R, 2, Q, 6, 3, 7, O, 64, 64, N, nullptr), 1);
  EXPECT(m4ri_amd_pivot_exchange_batch_dev(D, 1, 4, 4, 64, 4, P, nullptr, 2, Q, 6, 3, 7, O, 64, 64, N, nullptr), 1);
  EXPECT(m4ri_amd_pivot_exchange_batch_dev(D, 1, 4, 4, 64, 4, at(D, 60), R, 2, Q, 6, 3, 7, O, 64, 64, N, nullptr), 1);         // pivots on D's last word
  EXPECT(m4ri_amd_pivot_exchange_batch_dev(D, 1, 4, 4, 64, 4, P, at(P, 28), 2, Q, 6, 3, 7, O, 64, 64, N, nullptr), 1);         // rank on pivots
  EXPECT(m4ri_amd_pivot_exchange_batch_dev(D, 1, 4, 4, 64, 4, P, R, 2, at(R, -44), 6, 3, 7, O, 64, 64, N, nullptr), 1);        // req reaching rank
  EXPECT(m4ri_amd_pivot_exchange_batch_dev(D, 1, 4, 4, 64, 4, P, R, 2, Q, 6, 3, 7, at(Q, 44), 64, 64, N, nullptr), 1);         // order on req
  EXPECT(m4ri_amd_pivot_exchange_batch_dev(D, 1, 4, 4, 64, 4, P, R, 2, Q, 6, 3, 7, O, 64, 64, at(O, 508), nullptr), 1);        // done on order
  EXPECT(m4ri_amd_pivot_exchange_batch_dev(D, 1, 4, 4, 64, 4, P, R, 2, Q, 6, 3, 7, O, 64, 64, R, nullptr), 1);                 // done on rank
  EXPECT(m4ri_amd_pivot_exchange_batch_dev(D, 64, 1ll << 50, 1025, 4096, 4, P, R, 2, Q, 6, 3, 7, nullptr, 0, 0, N, nullptr), 801);
  EXPECT(m4ri_amd_pivot_exchange_batch_dev(D, INT64_MAX, INT64_MAX, INT64_MAX, INT64_MAX, 4, P, R, 0, Q, 6, 3, 7, nullptr, 0, 0, N, nullptr), 801);
  EXPECT(m4ri_amd_pivot_exchange_batch_dev(D, 63, 1ll << 50, 1025, 4096, 4, P, R, 2, Q, 6, 3, 7, nullptr, 0, 0, N, nullptr), 1); // the stride before the cap
  EXPECT(m4ri_amd_pivot_exchange_batch_dev(D, 1, 4, 4, 64, 4, P, R, 0, nullptr, 0, INT64_MAX, 7, O, 64, 64, N, nullptr), 0);
  setenv("M4RI_AMD_PIVOT_EXCHANGE_PATH0_MAX", "junk", 1);
  setenv("M4RI_AMD_PIVOT_EXCHANGE_PATH1_MAX", "-99999999999999999999", 1);
  EXPECT(m4ri_amd_pivot_exchange_batch_dev(D, 1, 4, 4, 64, 4, P, R, 0, Q, 6, 3, 7, O, 64, 64, N, nullptr), 0);
  EXPECT(m4ri_amd_pivot_exchange_batch_dev(D, 64, 1ll << 50, 1025, 4096, 4, P, R, 0, Q, 6, 3, 7, nullptr, 0, 0, N, nullptr), 801);
  EXPECT(m4ri_amd_plan_pivot_exchange_batch(1025, 4096, 1), 3);                                                                  // the plan does not read them
  EXPECT(m4ri_amd_plan_pivot_exchange_batch(0, 0, 0), 0);
  EXPECT(m4ri_amd_plan_pivot_exchange_batch(64, 64, 16), 0);
  EXPECT(m4ri_amd_plan_pivot_exchange_batch(65, 65, 1), 2);
  EXPECT(m4ri_amd_plan_pivot_exchange_batch(65, 65, 2), 1);
  EXPECT(m4ri_amd_plan_pivot_exchange_batch(65, 65, INT64_MAX), 1);
  EXPECT(m4ri_amd_plan_pivot_exchange_batch(1100, 1100, 4), 2);
  EXPECT(m4ri_amd_plan_pivot_exchange_batch(1024, 4096, 4), 2);
  EXPECT(m4ri_amd_plan_pivot_exchange_batch(INT64_MAX, INT64_MAX, INT64_MAX), 3);
  EXPECT(m4ri_amd_plan_pivot_exchange_batch(-1, 5, 1), -1);
  EXPECT(m4ri_amd_plan_pivot_exchange_batch(5, 5, -1), -1);
}

// ---- the search of information-set decoding -------------------------------------------------------------------------------------------------
static void isd_search() {
  // D: 2 members of 5 x 64 (80 bytes), four pivot rows and the received word; pivots 2 x 4 entries; rank 8 bytes; order 2 x 64 entries; best 16 bytes;
  // best_iter, iters_run, done 8 bytes each; W 2 x 1 word
  const int64_t M = INT64_MAX;
  word *D = (word *)(1ull << 20), *W = (word *)(1ull << 36);
  int32_t *P = (int32_t *)(1ull << 22), *R = (int32_t *)(1ull << 24), *O = (int32_t *)(1ull << 26), *I = (int32_t *)(1ull << 30), *U = (int32_t *)(1ull << 32),
          *N = (int32_t *)(1ull << 34);
  int64_t *B = (int64_t *)(1ull << 28);
  auto at = [](void *p, long bytes) { return (int32_t *)((char *)p + bytes); };
  EXPECT(m4ri_amd_isd_search_dev(D, 1, 5, 5, 64, 4, P, R, 0, 6, 3, 7, 2, 1, 3, O, 64, 64, B, I, U, N, W, 1, nullptr), 0);                  // batch = 0
  EXPECT(m4ri_amd_isd_search_dev(nullptr, 1, 5, 5, 64, 4, nullptr, nullptr, 0, 0, 0, 7, 0, 0, -1, nullptr, 0, 0, nullptr, nullptr, nullptr, nullptr, nullptr, 0, nullptr), 0);
  EXPECT(m4ri_amd_isd_search_dev(D, 1, 5, -1, 64, 0, P, R, 2, 6, 3, 7, 2, 1, 3, O, 64, 64, B, I, U, N, W, 1, nullptr), 1);
  EXPECT(m4ri_amd_isd_search_dev(D, 1, 5, 5, 64, 4, P, R, -1, 6, 3, 7, 2, 1, 3, O, 64, 64, B, I, U, N, W, 1, nullptr), 1);
  EXPECT(m4ri_amd_isd_search_dev(D, 1, 5, 5, 64, 4, P, R, 2, -1, 3, 7, 2, 1, 3, O, 64, 64, B, I, U, N, W, 1, nullptr), 1);                 // iters < 0
  EXPECT(m4ri_amd_isd_search_dev(D, 1, 5, 5, 64, 4, P, R, 2, 6, -1, 7, 2, 1, 3, O, 64, 64, B, I, U, N, W, 1, nullptr), 1);                 // steps < 0
  EXPECT(m4ri_amd_isd_search_dev(D, 1, 5, 5, 64, 4, P, R, 2, 6, 3, 7, -1, 1, 3, O, 64, 64, B, I, U, N, W, 1, nullptr), 1);                 // t < 0
  EXPECT(m4ri_amd_isd_search_dev(D, 1, 5, 5, 64, 4, P, R, 2, 6, 3, 7, 2, -1, 3, O, 64, 64, B, I, U, N, W, 1, nullptr), 1);                 // w_min < 0
  EXPECT(m4ri_amd_isd_search_dev(D, 1, 5, 5, 64, 4, P, R, 2, 6, 3, 7, 2, 1, 3, O, 64, 64, B, I, U, N, W, -1, nullptr), 1);                 // w_bs < 0
  EXPECT(m4ri_amd_isd_search_dev(D, 1, 5, 5, 64, 6, P, R, 2, 6, 3, 7, 2, 1, 3, O, 64, 64, B, I, U, N, W, 1, nullptr), 1);                  // pivot_rows > nrows
  EXPECT(m4ri_amd_isd_search_dev(D, 1, 5, 5, 64, 4, P, R, 2, 6, 3, 7, 2, 1, 3, O, 65, 65, B, I, U, N, W, 1, nullptr), 1);                  // olen > ncols
  EXPECT(m4ri_amd_isd_search_dev(D, 0, 5, 5, 64, 4, P, R, 2, 6, 3, 7, 2, 1, 3, O, 64, 64, B, I, U, N, W, 1, nullptr), 1);                  // d_stride < words
  EXPECT(m4ri_amd_isd_search_dev(D, 1, 4, 5, 64, 4, P, R, 2, 6, 3, 7, 2, 1, 3, O, 64, 64, B, I, U, N, W, 1, nullptr), 1);                  // overlapping members
  EXPECT(m4ri_amd_isd_search_dev(D, 1, 5, 5, 64, 4, P, R, 2, 6, 3, 7, 2, 1, 3, O, 63, 64, B, I, U, N, W, 1, nullptr), 1);                  // o_bs < olen
  EXPECT(m4ri_amd_isd_search_dev(D, 1, 5, 5, 64, 4, P, R, 2, 6, 3, 7, 2, 1, 3, O, 64, 64, B, I, U, N, W, 0, nullptr), 1);                  // w_bs < words
  EXPECT(m4ri_amd_isd_search_dev(nullptr, 1, 5, 5, 64, 4, P, R, 2, 6, 3, 7, 2, 1, 3, O, 64, 64, B, I, U, N, W, 1, nullptr), 1);
  EXPECT(m4ri_amd_isd_search_dev(D, 1, 5, 5, 64, 4, nullptr, R, 2, 6, 3, 7, 2, 1, 3, O, 64, 64, B, I, U, N, W, 1, nullptr), 1);
  EXPECT(m4ri_amd_isd_search_dev(D, 1, 5, 5, 64, 4, P, nullptr, 2, 6, 3, 7, 2, 1, 3, O, 64, 64, B, I, U, N, W, 1, nullptr), 1);
  EXPECT(m4ri_amd_isd_search_dev(D, 1, 5, 5, 64, 4, P, R, 2, 6, 3, 7, 2, 1, 3, O, 64, 64, nullptr, I, U, N, W, 1, nullptr), 1);            // best is required
  EXPECT(m4ri_amd_isd_search_dev(D, 1, 5, 5, 64, 4, P, R, 2, 0, 3, 7, 2, 1, 3, O, 64, 64, nullptr, I, U, N, W, 1, nullptr), 1);            // without iterations too
  EXPECT(m4ri_amd_isd_search_dev(D, 1, 5, 5, 64, 4, at(D, 76), R, 2, 6, 3, 7, 2, 1, 3, O, 64, 64, B, I, U, N, W, 1, nullptr), 1);          // pivots on D's last word
  EXPECT(m4ri_amd_isd_search_dev(D, 1, 5, 5, 64, 4, P, at(P, 28), 2, 6, 3, 7, 2, 1, 3, O, 64, 64, B, I, U, N, W, 1, nullptr), 1);          // rank on pivots
  EXPECT(m4ri_amd_isd_search_dev(D, 1, 5, 5, 64, 4, P, R, 2, 6, 3, 7, 2, 1, 3, at(R, 4), 64, 64, B, I, U, N, W, 1, nullptr), 1);           // order on rank
  EXPECT(m4ri_amd_isd_search_dev(D, 1, 5, 5, 64, 4, P, R, 2, 6, 3, 7, 2, 1, 3, O, 64, 64, (int64_t *)at(O, 504), I, U, N, W, 1, nullptr), 1);   // best on order
  EXPECT(m4ri_amd_isd_search_dev(D, 1, 5, 5, 64, 4, P, R, 2, 6, 3, 7, 2, 1, 3, O, 64, 64, B, at(B, 12), U, N, W, 1, nullptr), 1);          // best_iter on best
  EXPECT(m4ri_amd_isd_search_dev(D, 1, 5, 5, 64, 4, P, R, 2, 6, 3, 7, 2, 1, 3, O, 64, 64, B, I, at(I, 4), N, W, 1, nullptr), 1);           // iters_run on best_iter
  EXPECT(m4ri_amd_isd_search_dev(D, 1, 5, 5, 64, 4, P, R, 2, 6, 3, 7, 2, 1, 3, O, 64, 64, B, I, U, U, W, 1, nullptr), 1);                  // done on iters_run
  EXPECT(m4ri_amd_isd_search_dev(D, 1, 5, 5, 64, 4, P, R, 2, 6, 3, 7, 2, 1, 3, O, 64, 64, B, I, U, N, (word *)at(N, 0), 1, nullptr), 1);   // W on done
  EXPECT(m4ri_amd_isd_search_dev(D, 1, 5, 5, 64, 4, P, R, 2, 6, 3, 7, 2, 1, 3, O, 64, 64, B, I, U, N, D + 9, 1, nullptr), 1);              // W on D's last word
  EXPECT(m4ri_amd_isd_search_dev(D, 1, 5, 5, 64, 4, P, R, 2, 6, 3, 7, 2, 1, 3, O, 64, 64, B, I, U, N, (word *)(1ull << 19), M, nullptr), 1);   // W below all: its 2^66 bytes reach everything
  EXPECT(m4ri_amd_isd_search_dev(D, 1, M, 5, 64, 4, P, R, 2, 6, 3, 7, 2, 1, 3, O, 64, 64, B, I, U, N, nullptr, 0, nullptr), 1);            // and D's
  EXPECT(m4ri_amd_isd_search_dev(D, 1, 5, 5, 64, 4, P, R, 2, 6, 3, 7, 2, 1, 3, O, M, 64, B, I, U, N, W, 1, nullptr), 1);                   // and the order's
  // the limits: 801 with and without members, after the sizes and before the pointers
  EXPECT(m4ri_amd_isd_search_dev(D, 1, 5, 5, 64, 4, P, R, 2, 6, 3, 7, 9, 1, 3, O, 64, 64, B, I, U, N, W, 1, nullptr), 801);                // t > 8
  EXPECT(m4ri_amd_isd_search_dev(D, 1, 5, 5, 64, 4, P, R, 0, 6, 3, 7, M, 1, 3, O, 64, 64, B, I, U, N, W, 1, nullptr), 801);
  EXPECT(m4ri_amd_isd_search_dev(D, 1, 1 << 20, 1025, 64, 1025, P, R, 2, 6, 3, 7, 1, 1, 3, O, 64, 64, B, I, U, N, W, 1, nullptr), 801);    // pivot_rows > 1024
  EXPECT(m4ri_amd_isd_search_dev(D, 17, 1 << 20, 5, 1025, 4, P, R, 2, 6, 3, 7, 1, 1, 3, nullptr, 0, 0, B, I, U, N, W, 17, nullptr), 801);  // ncols > 1024
  EXPECT(m4ri_amd_isd_search_dev(D, 1, 1 << 20, 1024, 64, 1024, P, R, 2, 6, 3, 7, 2, 1, 3, O, 64, 64, B, I, U, N, W, 1, nullptr), 1);      // C(1024, 2) is in: D reaches pivots
  EXPECT(m4ri_amd_isd_search_dev(D, 1, 1 << 20, 1024, 64, 1024, P, R, 0, 6, 3, 7, 2, 1, 3, O, 64, 64, B, I, U, N, W, 1, nullptr), 0);
  EXPECT(m4ri_amd_isd_search_dev(D, 1, 1 << 20, 1024, 64, 1024, P, R, 0, 6, 3, 7, 3, 1, 3, O, 64, 64, B, I, U, N, W, 1, nullptr), 801);    // C(1024, 3) > 2^24
  EXPECT(m4ri_amd_isd_search_dev(D, 16, 1 << 20, 2000, 1024, 4, P, R, 2, 6, 3, 7, 2, 1, 3, nullptr, 0, 0, B, I, U, N, W, 16, nullptr), 801);    // beyond LDS
  EXPECT(m4ri_amd_isd_search_dev(D, M, M, M, M, M, P, R, 2, M, M, 7, M, M, M, O, M, M, B, I, U, N, W, M, nullptr), 801);
  EXPECT(m4ri_amd_isd_search_dev(D, M, M, M, 64, 4, P, R, 0, 6, 3, 7, 2, 1, 3, O, 64, 64, B, I, U, N, W, 1, nullptr), 801);                // INT64_MAX rows
  EXPECT(m4ri_amd_isd_search_dev(D, 1, 5, 5, 64, 4, P, R, 2, M, 3, 7, 2, 1, 3, O, 64, 64, B, I, U, N, W, 1, nullptr), 801);                // 32-bit counts
  EXPECT(m4ri_amd_isd_search_dev(D, 1, 5, 5, 64, 4, P, R, 2, 6, M, 7, 2, 1, 3, O, 64, 64, B, I, U, N, W, 1, nullptr), 801);
  EXPECT(m4ri_amd_isd_search_dev(D, 1, 5, 5, 64, 4, P, R, 2, M, M, 7, 2, 1, 3, O, 64, 64, B, I, U, N, W, 1, nullptr), 801);
  EXPECT(m4ri_amd_isd_search_dev(D, 1, 5, 5, 64, 4, P, R, 0, INT32_MAX, 1, 7, 2, M, M, O, 64, 64, B, I, U, N, W, 1, nullptr), 0);
  EXPECT(m4ri_amd_isd_search_dev(D, 1, 5, 5, 64, 4, P, R, 0, 1, M, 7, 2, 1, -M, O, 64, 64, B, I, U, N, W, 1, nullptr), 0);                 // one iteration: no step
  EXPECT(m4ri_amd_isd_search_dev(D, 1, 5, 5, 64, 4, P, R, 0, (int64_t)INT32_MAX + 1, 0, 7, 2, 1, 3, O, 64, 64, B, I, U, N, W, 1, nullptr), 801);
  EXPECT(m4ri_amd_isd_search_dev(D, 0, 5, 5, 64, 4, P, R, 2, 6, 3, 7, 9, 1, 3, O, 64, 64, B, I, U, N, W, 1, nullptr), 1);                  // the stride before the limits
  setenv("M4RI_AMD_ISD_SEARCH_PATH0_MAX", "junk", 1);
  EXPECT(m4ri_amd_isd_search_dev(D, 1, 5, 5, 64, 4, P, R, 0, 6, 3, 7, 2, 1, 3, O, 64, 64, B, I, U, N, W, 1, nullptr), 0);
  setenv("M4RI_AMD_ISD_SEARCH_PATH0_MAX", "-99999999999999999999", 1);
  EXPECT(m4ri_amd_isd_search_dev(D, 1, 5, 5, 64, 4, P, R, 0, 6, 3, 7, 9, 1, 3, O, 64, 64, B, I, U, N, W, 1, nullptr), 801);
  EXPECT(m4ri_amd_plan_isd_search(64, 64, 64, 9), 2);                                                                                      // the plan does not read it
  EXPECT(m4ri_amd_plan_isd_search(0, 0, 0, 0), 0);
  EXPECT(m4ri_amd_plan_isd_search(64, 64, 63, 3), 0);
  EXPECT(m4ri_amd_plan_isd_search(65, 64, 64, 3), 1);
  EXPECT(m4ri_amd_plan_isd_search(1024, 1024, 1024, 2), 1);
  EXPECT(m4ri_amd_plan_isd_search(1024, 1024, 1024, 3), 2);
  EXPECT(m4ri_amd_plan_isd_search(2000, 1024, 4, 2), 2);
  EXPECT(m4ri_amd_plan_isd_search(M, M, M, M), 2);
  EXPECT(m4ri_amd_plan_isd_search(M, 64, 4, 0), 2);
  EXPECT(m4ri_amd_plan_isd_search(-1, 5, 1, 1), -1);
  EXPECT(m4ri_amd_plan_isd_search(5, 5, 1, -1), -1);
}

// ---- the collision search of information-set decoding ---------------------------------------------------------------------------------------
static void isd_collide_search() {
  // the operands of isd_search(); four pivot rows split 2 + 2, a sum of one row of each half, the window the order's entries 4 .. 6
  const int64_t M = INT64_MAX;
  word *D = (word *)(1ull << 20), *W = (word *)(1ull << 36);
  int32_t *P = (int32_t *)(1ull << 22), *R = (int32_t *)(1ull << 24), *O = (int32_t *)(1ull << 26), *I = (int32_t *)(1ull << 30), *U = (int32_t *)(1ull << 32),
          *N = (int32_t *)(1ull << 34);
  int64_t *B = (int64_t *)(1ull << 28);
  auto at = [](void *p, long bytes) { return (int32_t *)((char *)p + bytes); };
#define ICS(D_, ds, dbs, nr, nc, pr, P_, R_, batch, iters, steps, k1, t1, t2, ell, wmin, wstop, O_, obs, olen, B_, I_, U_, N_, W_, wbs) \
  m4ri_amd_isd_collide_search_dev(D_, ds, dbs, nr, nc, pr, P_, R_, batch, iters, steps, 7, k1, t1, t2, ell, wmin, wstop, O_, obs, olen, B_, I_, U_, N_, W_, wbs, nullptr)
  EXPECT(ICS(D, 1, 5, 5, 64, 4, P, R, 0, 6, 3, 2, 1, 1, 3, 1, 3, O, 64, 64, B, I, U, N, W, 1), 0);                       // batch = 0
  EXPECT(ICS(nullptr, 1, 5, 5, 64, 4, nullptr, nullptr, 0, 0, 0, 0, 0, 0, 0, 0, -1, nullptr, 0, 0, nullptr, nullptr, nullptr, nullptr, nullptr, 0), 0);
  EXPECT(ICS(D, 1, 5, -1, 64, 0, P, R, 2, 6, 3, 0, 1, 1, 3, 1, 3, O, 64, 64, B, I, U, N, W, 1), 1);
  EXPECT(ICS(D, 1, 5, 5, 64, 4, P, R, -1, 6, 3, 2, 1, 1, 3, 1, 3, O, 64, 64, B, I, U, N, W, 1), 1);
  EXPECT(ICS(D, 1, 5, 5, 64, 4, P, R, 2, -1, 3, 2, 1, 1, 3, 1, 3, O, 64, 64, B, I, U, N, W, 1), 1);                      // iters < 0
  EXPECT(ICS(D, 1, 5, 5, 64, 4, P, R, 2, 6, -1, 2, 1, 1, 3, 1, 3, O, 64, 64, B, I, U, N, W, 1), 1);                      // steps < 0
  EXPECT(ICS(D, 1, 5, 5, 64, 4, P, R, 2, 6, 3, -1, 1, 1, 3, 1, 3, O, 64, 64, B, I, U, N, W, 1), 1);                      // k1 < 0
  EXPECT(ICS(D, 1, 5, 5, 64, 4, P, R, 2, 6, 3, 5, 1, 1, 3, 1, 3, O, 64, 64, B, I, U, N, W, 1), 1);                       // k1 > pivot_rows
  EXPECT(ICS(D, 1, 5, 5, 64, 4, P, R, 2, 6, 3, M, 1, 1, 3, 1, 3, O, 64, 64, B, I, U, N, W, 1), 1);
  EXPECT(ICS(D, 1, 5, 5, 64, 4, P, R, 2, 6, 3, 2, -1, 1, 3, 1, 3, O, 64, 64, B, I, U, N, W, 1), 1);                      // t1 < 0
  EXPECT(ICS(D, 1, 5, 5, 64, 4, P, R, 2, 6, 3, 2, 1, -1, 3, 1, 3, O, 64, 64, B, I, U, N, W, 1), 1);                      // t2 < 0
  EXPECT(ICS(D, 1, 5, 5, 64, 4, P, R, 2, 6, 3, 2, 1, 1, -1, 1, 3, O, 64, 64, B, I, U, N, W, 1), 1);                      // ell < 0
  EXPECT(ICS(D, 1, 5, 5, 64, 4, P, R, 2, 6, 3, 2, 1, 1, 3, -1, 3, O, 64, 64, B, I, U, N, W, 1), 1);                      // w_min < 0
  EXPECT(ICS(D, 1, 5, 5, 64, 4, P, R, 2, 6, 3, 2, 1, 1, 3, 1, 3, O, 64, 64, B, I, U, N, W, -1), 1);                      // w_bs < 0
  EXPECT(ICS(D, 1, 5, 5, 64, 6, P, R, 2, 6, 3, 2, 1, 1, 3, 1, 3, O, 64, 64, B, I, U, N, W, 1), 1);                       // pivot_rows > nrows
  EXPECT(ICS(D, 1, 5, 5, 64, 4, P, R, 2, 6, 3, 2, 1, 1, 3, 1, 3, O, 65, 65, B, I, U, N, W, 1), 1);                       // olen > ncols
  EXPECT(ICS(D, 1, 5, 5, 64, 4, P, R, 2, 6, 3, 2, 1, 1, 3, 1, 3, nullptr, 64, 64, B, I, U, N, W, 1), 1);                 // a window without its order
  EXPECT(ICS(D, 1, 5, 5, 64, 4, P, R, 0, 6, 3, 2, 1, 1, 3, 1, 3, nullptr, 64, 64, B, I, U, N, W, 1), 1);                 // with no member either
  EXPECT(ICS(D, 1, 5, 5, 64, 4, P, R, 2, 6, 3, 2, 1, 1, 3, 1, 3, O, 64, 6, B, I, U, N, W, 1), 1);                        // olen < pivot_rows + ell
  EXPECT(ICS(D, 1, 5, 5, 64, 4, P, R, 0, 6, 3, 2, 1, 1, 3, 1, 3, O, 64, 7, B, I, U, N, W, 1), 0);                        // olen = pivot_rows + ell
  EXPECT(ICS(D, 1, 5, 5, 64, 4, P, R, 2, 6, 3, 2, 1, 1, M, 1, 3, O, 64, 64, B, I, U, N, W, 1), 1);                       // pivot_rows + ell beyond 64 bits
  EXPECT(ICS(D, 1, 5, 5, 64, 4, P, R, 0, 6, 3, 2, 1, 1, 0, 1, 3, nullptr, 0, 0, B, I, U, N, W, 1), 0);                   // no window: no order needed
  EXPECT(ICS(D, 0, 5, 5, 64, 4, P, R, 2, 6, 3, 2, 1, 1, 3, 1, 3, O, 64, 64, B, I, U, N, W, 1), 1);                       // d_stride < words
  EXPECT(ICS(D, 1, 4, 5, 64, 4, P, R, 2, 6, 3, 2, 1, 1, 3, 1, 3, O, 64, 64, B, I, U, N, W, 1), 1);                       // overlapping members
  EXPECT(ICS(D, 1, 5, 5, 64, 4, P, R, 2, 6, 3, 2, 1, 1, 3, 1, 3, O, 63, 64, B, I, U, N, W, 1), 1);                       // o_bs < olen
  EXPECT(ICS(D, 1, 5, 5, 64, 4, P, R, 2, 6, 3, 2, 1, 1, 3, 1, 3, O, 64, 64, B, I, U, N, W, 0), 1);                       // w_bs < words
  EXPECT(ICS(nullptr, 1, 5, 5, 64, 4, P, R, 2, 6, 3, 2, 1, 1, 3, 1, 3, O, 64, 64, B, I, U, N, W, 1), 1);
  EXPECT(ICS(D, 1, 5, 5, 64, 4, nullptr, R, 2, 6, 3, 2, 1, 1, 3, 1, 3, O, 64, 64, B, I, U, N, W, 1), 1);
  EXPECT(ICS(D, 1, 5, 5, 64, 4, P, nullptr, 2, 6, 3, 2, 1, 1, 3, 1, 3, O, 64, 64, B, I, U, N, W, 1), 1);
  EXPECT(ICS(D, 1, 5, 5, 64, 4, P, R, 2, 6, 3, 2, 1, 1, 3, 1, 3, O, 64, 64, nullptr, I, U, N, W, 1), 1);                 // best is required
  EXPECT(ICS(D, 1, 5, 5, 64, 4, P, R, 2, 0, 3, 2, 1, 1, 3, 1, 3, O, 64, 64, nullptr, I, U, N, W, 1), 1);                 // without iterations too
  EXPECT(ICS(D, 1, 5, 5, 64, 4, at(D, 76), R, 2, 6, 3, 2, 1, 1, 3, 1, 3, O, 64, 64, B, I, U, N, W, 1), 1);               // pivots on D's last word
  EXPECT(ICS(D, 1, 5, 5, 64, 4, P, at(P, 28), 2, 6, 3, 2, 1, 1, 3, 1, 3, O, 64, 64, B, I, U, N, W, 1), 1);               // rank on pivots
  EXPECT(ICS(D, 1, 5, 5, 64, 4, P, R, 2, 6, 3, 2, 1, 1, 3, 1, 3, at(R, 4), 64, 64, B, I, U, N, W, 1), 1);                // order on rank
  EXPECT(ICS(D, 1, 5, 5, 64, 4, P, R, 2, 6, 3, 2, 1, 1, 3, 1, 3, O, 64, 64, (int64_t *)at(O, 504), I, U, N, W, 1), 1);   // best on order
  EXPECT(ICS(D, 1, 5, 5, 64, 4, P, R, 2, 6, 3, 2, 1, 1, 3, 1, 3, O, 64, 64, B, at(B, 12), U, N, W, 1), 1);               // best_iter on best
  EXPECT(ICS(D, 1, 5, 5, 64, 4, P, R, 2, 6, 3, 2, 1, 1, 3, 1, 3, O, 64, 64, B, I, at(I, 4), N, W, 1), 1);                // iters_run on best_iter
  EXPECT(ICS(D, 1, 5, 5, 64, 4, P, R, 2, 6, 3, 2, 1, 1, 3, 1, 3, O, 64, 64, B, I, U, U, W, 1), 1);                       // done on iters_run
  EXPECT(ICS(D, 1, 5, 5, 64, 4, P, R, 2, 6, 3, 2, 1, 1, 3, 1, 3, O, 64, 64, B, I, U, N, (word *)at(N, 0), 1), 1);        // W on done
  EXPECT(ICS(D, 1, 5, 5, 64, 4, P, R, 2, 6, 3, 2, 1, 1, 3, 1, 3, O, 64, 64, B, I, U, N, D + 9, 1), 1);                   // W on D's last word
  EXPECT(ICS(D, 1, 5, 5, 64, 4, P, R, 2, 6, 3, 2, 1, 1, 3, 1, 3, O, 64, 64, B, I, U, N, (word *)(1ull << 19), M), 1);    // W below all: its 2^66 bytes reach everything
  EXPECT(ICS(D, 1, M, 5, 64, 4, P, R, 2, 6, 3, 2, 1, 1, 3, 1, 3, O, 64, 64, B, I, U, N, nullptr, 0), 1);                 // and D's
  EXPECT(ICS(D, 1, 5, 5, 64, 4, P, R, 2, 6, 3, 2, 1, 1, 3, 1, 3, O, M, 64, B, I, U, N, W, 1), 1);                        // and the order's
  // the limits, with and without members
  EXPECT(ICS(D, 1, 5, 5, 64, 4, P, R, 2, 6, 3, 2, 9, 1, 3, 1, 3, O, 64, 64, B, I, U, N, W, 1), 801);                     // t1 > 8
  EXPECT(ICS(D, 1, 5, 5, 64, 4, P, R, 0, 6, 3, 2, 1, M, 3, 1, 3, O, 64, 64, B, I, U, N, W, 1), 801);                     // t2 > 8
  EXPECT(ICS(D, 2, 10, 5, 128, 4, P, R, 0, 6, 3, 2, 1, 1, 65, 1, 3, O, 128, 128, B, I, U, N, W, 2), 801);                // ell > 64
  EXPECT(ICS(D, 2, 10, 5, 128, 4, P, R, 0, 6, 3, 2, 1, 1, 64, 1, 3, O, 128, 128, B, I, U, N, W, 2), 0);
  EXPECT(ICS(D, 1, 1 << 20, 1025, 64, 1025, P, R, 2, 6, 3, 2, 1, 1, 0, 1, 3, O, 64, 64, B, I, U, N, W, 1), 801);         // pivot_rows > 1024
  EXPECT(ICS(D, 17, 1 << 20, 5, 1025, 4, P, R, 2, 6, 3, 2, 1, 1, 0, 1, 3, nullptr, 0, 0, B, I, U, N, W, 17), 801);       // ncols > 1024
  EXPECT(ICS(D, 1, 1 << 20, 137, 64, 136, P, R, 0, 6, 3, 128, 2, 1, 0, 1, 3, O, 64, 64, B, I, U, N, W, 1), 0);           // N1 = 8128
  EXPECT(ICS(D, 1, 1 << 20, 138, 64, 137, P, R, 0, 6, 3, 129, 2, 1, 0, 1, 3, O, 64, 64, B, I, U, N, W, 1), 801);         // N1 = 8256
  EXPECT(ICS(D, 1, 1 << 20, 1024, 64, 1024, P, R, 0, 6, 3, 8, 1, 2, 0, 1, 3, O, 64, 64, B, I, U, N, W, 1), 0);           // N2 = C(1016, 2)
  EXPECT(ICS(D, 1, 1 << 20, 1024, 64, 1024, P, R, 0, 6, 3, 8, 1, 3, 0, 1, 3, O, 64, 64, B, I, U, N, W, 1), 801);         // N2 = C(1016, 3) > 2^24
  EXPECT(ICS(D, 1, 1 << 20, 1024, 64, 1024, P, R, 2, 6, 3, 8, 1, 2, 0, 1, 3, O, 64, 64, B, I, U, N, W, 1), 1);           // in: D reaches pivots
  EXPECT(ICS(D, 16, 1 << 20, 2000, 1024, 4, P, R, 2, 6, 3, 2, 1, 1, 3, 1, 3, nullptr, 0, 0, B, I, U, N, W, 16), 1);      // the window's order before the LDS
  EXPECT(ICS(D, 16, 1 << 20, 2000, 1024, 4, P, R, 2, 6, 3, 2, 1, 1, 0, 1, 3, nullptr, 0, 0, B, I, U, N, W, 16), 801);    // beyond LDS
  EXPECT(ICS(D, M, M, M, M, M, P, R, 2, M, M, M, M, M, 0, M, M, O, M, M, B, I, U, N, W, M), 801);
  EXPECT(ICS(D, M, M, M, M, M, P, R, 2, M, M, M, M, M, M, M, M, O, M, M, B, I, U, N, W, M), 1);                          // 2 M > olen over the integers
  EXPECT(ICS(D, M, M, M, 64, 4, P, R, 0, 6, 3, 2, 1, 1, 3, 1, 3, O, 64, 64, B, I, U, N, W, 1), 801);                     // INT64_MAX rows
  EXPECT(ICS(D, 1, 5, 5, 64, 4, P, R, 2, M, 3, 2, 1, 1, 3, 1, 3, O, 64, 64, B, I, U, N, W, 1), 801);                     // 32-bit counts
  EXPECT(ICS(D, 1, 5, 5, 64, 4, P, R, 2, 6, M, 2, 1, 1, 3, 1, 3, O, 64, 64, B, I, U, N, W, 1), 801);
  EXPECT(ICS(D, 1, 5, 5, 64, 4, P, R, 2, M, M, 2, 1, 1, 3, 1, 3, O, 64, 64, B, I, U, N, W, 1), 801);
  EXPECT(ICS(D, 1, 5, 5, 64, 4, P, R, 0, INT32_MAX, 1, 2, 1, 1, 3, M, M, O, 64, 64, B, I, U, N, W, 1), 0);
  EXPECT(ICS(D, 1, 5, 5, 64, 4, P, R, 0, 1, M, 2, 1, 1, 3, 1, -M, O, 64, 64, B, I, U, N, W, 1), 0);                      // one iteration: no step
  EXPECT(ICS(D, 1, 5, 5, 64, 4, P, R, 0, (int64_t)INT32_MAX + 1, 0, 2, 1, 1, 3, 1, 3, O, 64, 64, B, I, U, N, W, 1), 801);
  EXPECT(ICS(D, 0, 5, 5, 64, 4, P, R, 2, 6, 3, 2, 9, 1, 3, 1, 3, O, 64, 64, B, I, U, N, W, 1), 1);                       // the stride before the limits
  setenv("M4RI_AMD_ISD_COLLIDE_SEARCH_THREADS", "junk", 1);
  EXPECT(ICS(D, 1, 5, 5, 64, 4, P, R, 0, 6, 3, 2, 1, 1, 3, 1, 3, O, 64, 64, B, I, U, N, W, 1), 0);
  setenv("M4RI_AMD_ISD_COLLIDE_SEARCH_THREADS", "-99999999999999999999", 1);
  EXPECT(ICS(D, 1, 5, 5, 64, 4, P, R, 0, 6, 3, 2, 9, 1, 3, 1, 3, O, 64, 64, B, I, U, N, W, 1), 801);
  unsetenv("M4RI_AMD_ISD_COLLIDE_SEARCH_THREADS");
#undef ICS
  EXPECT(m4ri_amd_plan_isd_collide_search(0, 0, 0, 0, 0, 0, 0), 1);
  EXPECT(m4ri_amd_plan_isd_collide_search(64, 64, 63, 31, 3, 3, 12), 1);                                                   // no wave path
  EXPECT(m4ri_amd_plan_isd_collide_search(137, 200, 136, 128, 2, 1, 64), 1);
  EXPECT(m4ri_amd_plan_isd_collide_search(138, 200, 137, 129, 2, 1, 64), 2);
  EXPECT(m4ri_amd_plan_isd_collide_search(1024, 1024, 1024, 8, 1, 1, 0), 1);
  EXPECT(m4ri_amd_plan_isd_collide_search(1024, 1024, 1024, 512, 1, 1, 0), 2);                                             // the table no longer fits beside the member
  EXPECT(m4ri_amd_plan_isd_collide_search(1024, 64, 1024, 8, 1, 3, 0), 2);
  EXPECT(m4ri_amd_plan_isd_collide_search(64, 64, 64, 32, 9, 1, 0), 2);
  EXPECT(m4ri_amd_plan_isd_collide_search(64, 128, 32, 16, 1, 1, 65), 2);
  EXPECT(m4ri_amd_plan_isd_collide_search(2000, 1024, 4, 2, 1, 1, 0), 2);
  EXPECT(m4ri_amd_plan_isd_collide_search(M, M, M, M, M, M, M), 2);
  EXPECT(m4ri_amd_plan_isd_collide_search(M, 64, 4, 2, 0, 0, 0), 2);
  EXPECT(m4ri_amd_plan_isd_collide_search(-1, 5, 1, 0, 1, 1, 0), -1);
  EXPECT(m4ri_amd_plan_isd_collide_search(5, 5, 4, 5, 1, 1, 0), -1);                                                       // k1 > pivot_rows
  EXPECT(m4ri_amd_plan_isd_collide_search(5, 5, 4, 2, 1, 1, -1), -1);
}

// ---- the calls on single operands: elimination, solves, products, transposes, reductions, assembly, weights --------------------------
// Operands at ascending addresses 2^20 apart, A lowest: a span that is too long by the integers reaches every operand above it.
static void sizes_beyond_int64() {
  const int64_t M = INT64_MAX, T = (int64_t)1 << 40, Q = (int64_t)1 << 62, I = INT32_MAX;
  auto at = [](int i) { return (void *)((uintptr_t)(i + 1) << 20); };
  word *A = (word *)at(0), *B = (word *)at(1), *C = (word *)at(2), *V = (word *)at(3), *W = (word *)at(4);
  int32_t *R = (int32_t *)at(5), *P = (int32_t *)at(6), *O = (int32_t *)at(7), *S = (int32_t *)at(8), *E = (int32_t *)at(9);
  int64_t *H = (int64_t *)at(10), *L = (int64_t *)at(11), *K = (int64_t *)at(12), *N = (int64_t *)at(13), *U = (int64_t *)at(14);
  // echelon forms in place: no spans; the members of a batch must fit their stride
  EXPECT(m4ri_amd_echelonize_batch_dev(A, M, M, M, M, 0, 0, R, P, nullptr), 0);
  EXPECT(m4ri_amd_echelonize_batch_dev(A, M, M, M, M, 2, 0, R, P, nullptr), 1);            // a_bs < (nrows - 1) * stride + width, about 2^126
  EXPECT(m4ri_amd_echelonize_batch_dev(A, 1, M, M, M, 2, 0, R, P, nullptr), 1);            // stride < width = 2^57
  EXPECT(m4ri_amd_echelonize_batch_dev(A, T, Q, T, 64, 2, 0, R, P, nullptr), 1);           // 2^62 < (2^40 - 1) * 2^40 + 1
  EXPECT(m4ri_amd_echelonize_batch_dev(A, T, Q, T, 64, 2, 0, nullptr, P, nullptr), 1);
  EXPECT(m4ri_amd_plan_echelonize_batch(M, M), 3);
  EXPECT(m4ri_amd_plan_echelonize_batch(64, M), 3);
  // on a column order: the cap comes before the member fit, the spans after it
  EXPECT(m4ri_amd_echelonize_order_batch_dev(B, M, M, A, M, M, M, M, M, O, M, M, 2, 1, R, P, nullptr), 801);
  EXPECT(m4ri_amd_echelonize_order_batch_dev(B, M, M, A, M, M, 4, 64, 4, O, M, 64, 2, 1, R, P, nullptr), 1);   // d_bs < 3 * d_stride + 1
  EXPECT(m4ri_amd_echelonize_order_batch_dev(B, T, M, A, T, M, 4, 64, 4, O, 64, 64, 2, 1, R, P, nullptr), 1);  // fits; D's 2^66 bytes reach the order
  EXPECT(m4ri_amd_echelonize_order_batch_dev(A, T, M, A, T, M, 4, 64, 4, O, 64, 64, 2, 1, R, P, nullptr), 1);  // in place: still the order
  EXPECT(m4ri_amd_echelonize_order_batch_dev(B, 1, 4, C, 1, 4, 4, 64, 4, (int32_t *)A, M, 64, 2, 1, R, P, nullptr), 1);   // the order's 2^65 bytes reach D
  EXPECT(m4ri_amd_echelonize_order_batch_dev(B, M, M, A, M, M, 4, 64, 4, O, M, 64, 0, 1, R, P, nullptr), 0);
  EXPECT(m4ri_amd_plan_echelonize_order_batch(M, M), 3);
  EXPECT(m4ri_amd_random_orders_batch_dev(O, M, M, M, 7, nullptr), 801);
  EXPECT(m4ri_amd_random_orders_batch_dev(nullptr, M, 4096, M, 7, nullptr), 1);
  EXPECT(m4ri_amd_random_orders_batch_dev(O, 4095, 4096, M, 7, nullptr), 1);
  EXPECT(m4ri_amd_random_orders_batch_dev(O, M, 4096, 0, 7, nullptr), 0);
  EXPECT(m4ri_amd_pivot_exchange_batch_dev(A, T, M, 4, 64, 4, P, R, 2, O, 6, 3, 7, nullptr, 0, 0, S, nullptr), 1);   // D's span reaches pivots
  EXPECT(m4ri_amd_pivot_exchange_batch_dev(A, 1, 4, 4, 64, 4, P, R, 2, O, M, Q, 7, nullptr, 0, 0, S, nullptr), 1);   // the requests' 2^66 bytes reach done
  // solves, inverses, kernels
  EXPECT(m4ri_amd_solve_left_batch_dev(A, M, M, M, M, B, M, M, M, 0, S, R, nullptr), 0);
  EXPECT(m4ri_amd_solve_left_batch_dev(A, M, M, M, M, B, M, M, M, 2, S, R, nullptr), 1);
  EXPECT(m4ri_amd_solve_left_batch_dev(A, T, Q, T, T, B, T, Q, 64, 2, S, R, nullptr), 1);
  EXPECT(m4ri_amd_solve_left_batch_dev(A, 1, Q, T, T, B, T, Q, 64, 1, S, R, nullptr), 1);  // a_stride < 2^34
  EXPECT(m4ri_amd_plan_solve_batch(M, M, M), 2);
  EXPECT(m4ri_amd_inv_batch_dev(B, M, M, A, M, M, M, 2, R, nullptr), 1);
  EXPECT(m4ri_amd_inv_batch_dev(B, T, 0, A, T, 0, T, 1, R, nullptr), 1);                   // one member of 2^83 bytes: A's reaches Binv
  EXPECT(m4ri_amd_inv_batch_dev(A, T, 0, A, T, 1, T, 1, R, nullptr), 1);                   // in place with another layout
  EXPECT(m4ri_amd_inv_batch_dev(B, M, M, A, M, M, M, 0, R, nullptr), 0);
  EXPECT(m4ri_amd_kernel_left_batch_dev(A, M, M, M, M, B, M, M, M, 2, R, nullptr), 1);
  EXPECT(m4ri_amd_kernel_left_batch_dev(A, T, 0, T, T, B, T, 0, T, 1, R, nullptr), 1);     // A's span reaches R
  EXPECT(m4ri_amd_kernel_left_batch_dev(A, T, 0, T, T, B, T, 0, T + 1, 1, R, nullptr), 1); // kc > n
  EXPECT(m4ri_amd_plan_kernel_batch(M, M), 2);
  EXPECT(m4ri_amd_ple_batch_dev(A, M, M, M, M, 0, 1, P, O, R, nullptr), 0);
  EXPECT(m4ri_amd_ple_batch_dev(A, M, M, M, M, 2, 1, P, O, R, nullptr), 1);
  EXPECT(m4ri_amd_ple_batch_dev(A, T, Q, T, 64, 2, 1, P, O, R, nullptr), 1);
  EXPECT(m4ri_amd_plan_ple_batch(M, M), 3);
  EXPECT(m4ri_amd_pluq_solve_left_batch_dev(A, M, M, M, M, R, P, O, B, M, M, M, 2, S, nullptr), 1);
  EXPECT(m4ri_amd_pluq_solve_left_batch_dev(A, T, 0, T, T, R, P, O, B, T, 0, T, 1, S, nullptr), 1);   // A's span reaches B
  EXPECT(m4ri_amd_pluq_solve_left_batch_dev(A, M, M, M, M, R, P, O, B, M, M, M, 0, S, nullptr), 0);
  EXPECT(m4ri_amd_plan_pluq_solve_batch(M, M, M), 2);
  // products and transposes
  EXPECT(m4ri_amd_mul_small_batch_dev(C, M, M, A, M, M, B, M, M, M, M, M, 2, 0, nullptr), 1);
  EXPECT(m4ri_amd_mul_small_batch_dev(C, T, Q, A, 1, 0, B, 1, 0, T, 64, 64, 2, 0, nullptr), 1);       // 2^62 < (2^40 - 1) * 2^40 + 1
  EXPECT(m4ri_amd_mul_small_batch_dev(A, T, 0, B, 1, 0, C, 1, 0, T, 64, 64, 1, 0, nullptr), 1);       // C (at A) is 2^83 bytes: it reaches both operands
  EXPECT(m4ri_amd_mul_small_batch_dev(A, T, Q, B, 1, 0, C, 1, 0, 2, 64, 64, 2, 0, nullptr), 1);       // fits; two members 2^65 bytes apart
  EXPECT(m4ri_amd_mul_small_batch_dev(C, M, M, A, M, M, B, M, M, M, M, M, 0, 0, nullptr), 0);
  EXPECT(m4ri_amd_mul_small_batch_op_dev(C, M, M, A, M, M, B, M, M, M, M, M, 2, 1, 1, 0, nullptr), 1);
  EXPECT(m4ri_amd_mul_small_batch_op_dev(A, T, 0, B, T, 0, C, 1, 0, T, 64, 64, 1, 1, 0, 0, nullptr), 1);
  EXPECT(m4ri_amd_mul_small_batch_op_dev(A, T, 0, B, 1, 0, C, 1, 0, T, 64, 64, 1, 1, 0, 0, nullptr), 1);  // A stored 64 x 2^40: a_stride < 2^34
  EXPECT(m4ri_amd_plan_mul_small_batch(M, M, M), 2);
  EXPECT(m4ri_amd_plan_mul_small_batch_op(M, M, M, 1, 0), 2);
  EXPECT(m4ri_amd_transpose_batch_dev(B, M, M, A, M, M, M, M, 2, nullptr), 1);
  EXPECT(m4ri_amd_transpose_batch_dev(B, T, 0, A, T, 0, T, T, 1, nullptr), 1);             // A's span reaches D
  EXPECT(m4ri_amd_transpose_batch_dev(A, T, 0, A, T, 0, T, T, 1, nullptr), 1);             // in place beyond 1024
  EXPECT(m4ri_amd_transpose_batch_dev(B, M, M, A, M, M, M, M, 0, nullptr), 0);
  EXPECT(m4ri_amd_plan_transpose_batch(M, M), 2);
  // reductions: rows and weights are 32 bits; the outputs against the operands
  EXPECT(m4ri_amd_weight_batch_dev(A, M, M, nullptr, 0, 0, M, M, 2, N, nullptr, nullptr, nullptr), 1);
  EXPECT(m4ri_amd_weight_batch_dev(A, M, M, nullptr, 0, 0, I, 64, 2, N, nullptr, nullptr, nullptr), 1);   // A's span reaches total
  EXPECT(m4ri_amd_weight_batch_dev(A, M, M, B, M, M, I, I, 0, N, R, K, nullptr), 0);
  EXPECT(m4ri_amd_mismatch_batch_dev(A, M, M, B, M, M, I, 64, 2, R, nullptr), 1);
  EXPECT(m4ri_amd_mismatch_batch_dev(A, M, M, B, 0, M, I, 64, 2, R, nullptr), 1);          // b_stride < 1
  EXPECT(m4ri_amd_row_span_batch_dev(A, M, M, I, 64, 2, R, S, nullptr), 1);
  EXPECT(m4ri_amd_row_span_batch_dev(A, M, M, I, I, 0, R, S, nullptr), 0);
  EXPECT(m4ri_amd_plan_reduce_batch(M, M), 2);
  // assembly
  EXPECT(m4ri_amd_copy_block_batch_dev(B, M, M, M, M, A, M, M, M, M, M, M, 2, nullptr), 1);            // more than 2^36 columns
  EXPECT(m4ri_amd_copy_block_batch_dev(B, T, Q, 0, 0, A, T, Q, 0, 0, T, 64, 2, nullptr), 1);           // members do not fit
  EXPECT(m4ri_amd_copy_block_batch_dev(B, T, 0, 0, 0, A, T, 0, 0, 0, T, 64, 1, nullptr), 1);           // A's block reaches D's
  EXPECT(m4ri_amd_copy_block_batch_dev(B, M, 0, M, 0, A, M, 0, 0, 0, 4, 64, 1, nullptr), 1);           // D's block starts beyond the address space
  EXPECT(m4ri_amd_copy_block_batch_dev(B, M, M, M, 0, A, M, M, M, 0, M, 64, 0, nullptr), 0);
  EXPECT(m4ri_amd_extract_tri_batch_dev(B, M, M, A, M, M, M, M, 2, 1, 0, nullptr, nullptr), 1);
  EXPECT(m4ri_amd_extract_tri_batch_dev(B, M, M, A, M, M, I, I, 2, 1, 0, nullptr, nullptr), 1);        // members do not fit
  EXPECT(m4ri_amd_extract_tri_batch_dev(B, M, 0, A, M, 0, I, I, 1, 1, 0, nullptr, nullptr), 1);        // A's span reaches D
  EXPECT(m4ri_amd_extract_tri_batch_dev(B, M, M, A, M, M, I, I, 0, 1, 0, nullptr, nullptr), 0);
  EXPECT(m4ri_amd_apply_p_left_batch_dev(A, M, M, M, M, 2, P, M, M, 0, S, nullptr), 1);
  EXPECT(m4ri_amd_apply_p_left_batch_dev(A, T, 0, T, 64, 1, P, 0, 5, 0, S, nullptr), 1);               // A's span reaches P
  EXPECT(m4ri_amd_apply_p_right_batch_dev(A, M, M, M, M, 2, P, M, M, 0, S, nullptr), 1);
  EXPECT(m4ri_amd_apply_p_right_batch_dev(A, 1, 4, 4, 64, 2, P, M, 5, 0, S, nullptr), 1);              // P's 2^65 bytes reach status
  EXPECT(m4ri_amd_apply_p_right_batch_dev(A, M, M, M, M, 0, P, M, M, 0, S, nullptr), 0);
  EXPECT(m4ri_amd_plan_perm_batch(M, M, 0), 2);
  EXPECT(m4ri_amd_plan_perm_batch(M, M, 1), 2);
  // weights of row spaces and of row sums: the limits first
  EXPECT(m4ri_amd_rowspace_weights_batch_dev(A, M, M, M, M, V, M, 2, 0, H, L, nullptr), 801);
  EXPECT(m4ri_amd_rowspace_weights_batch_dev(A, M, M, 40, 1024, V, M, 2, 0, H, L, nullptr), 1);        // G's span reaches hist
  EXPECT(m4ri_amd_rowspace_weights_batch_dev(A, 16, 640, 40, 1024, V, M, 2, 0, H, L, nullptr), 1);     // V's does
  EXPECT(m4ri_amd_rowspace_weights_batch_dev(A, M, M, 40, 1024, V, M, 0, 0, H, L, nullptr), 0);
  EXPECT(m4ri_amd_plan_rowspace_weights_batch(M, M), 1);
  EXPECT(m4ri_amd_row_sums_weights_batch_dev(A, M, M, M, M, V, M, 2, M, 0, H, L, nullptr), 801);
  EXPECT(m4ri_amd_row_sums_weights_batch_dev(A, M, M, 40, 1024, V, M, 2, 2, 0, H, L, nullptr), 1);
  EXPECT(m4ri_amd_row_sums_weights_batch_dev(A, M, M, 40, 1024, V, M, 0, 2, 0, H, L, nullptr), 0);
  EXPECT(m4ri_amd_plan_row_sums_weights_batch(M, M, 2), 1);
  // the joins with strides of INT64_MAX and members to go with them
  EXPECT(m4ri_amd_row_sums_collide_batch_dev(A, M, M, 4, 64, V, M, 2, 2, 1, 1, O, M, 3, 0, H, L, nullptr), 1);
  EXPECT(m4ri_amd_row_sums_collide_list_batch_dev(A, M, M, 4, 64, V, M, 2, 2, 1, 1, O, M, 3, 0, 64, H, L, K, M, 5, N, nullptr), 1);
  EXPECT(m4ri_amd_row_sums_words_batch_dev(A, M, M, 4, 64, V, M, 2, 2, 1, 1, K, 6, 5, N, W, 2, 12, E, nullptr), 1);
  EXPECT(m4ri_amd_lists_collide_batch_dev(A, M, M, 4, B, M, M, 3, 64, V, M, 2, O, M, 3, 0, 64, H, L, K, 6, 5, N, nullptr), 1);
  EXPECT(m4ri_amd_lists_words_batch_dev(A, M, M, 4, B, M, M, 3, 64, V, M, 2, K, 6, 5, N, W, 2, 12, E, nullptr), 1);
  EXPECT(m4ri_amd_sort_rows_batch_dev(A, M, M, 6, 64, N, 2, O, M, 3, K, U, nullptr, nullptr, M, nullptr, 0, nullptr), 1);   // order's span reaches ucount
}

// ---- what the launchers forward to once an argument has passed: never reached here --------------------------------------------------------
// (-DKEEP_GOING: report and refuse instead, to see every finding of a build whose checks let something through)
#ifdef KEEP_GOING
#define UNREACHED(T) { fprintf(stderr, "batch_hostcheck: %s reached\n", __func__); return (T)999; }
#else
#define UNREACHED(T) { fprintf(stderr, "batch_hostcheck: %s reached\n", __func__); abort(); }
#endif
extern "C" {
hipError_t gf2_launch_copy_masked(hipStream_t, word *, int64_t, const word *, int64_t, int64_t, int64_t) UNREACHED(hipError_t)
hipError_t gf2_launch_transpose_tiles(hipStream_t, word *, int64_t, int64_t, const word *, int64_t, int64_t, int64_t, int64_t, int64_t) UNREACHED(hipError_t)
int m4ri_amd_apply_p_left_dev(word *, int64_t, int64_t, int64_t, const int32_t *, int64_t, int, void *) UNREACHED(int)
int m4ri_amd_apply_p_right_dev(word *, int64_t, int64_t, int64_t, const int32_t *, int64_t, int, void *) UNREACHED(int)
int m4ri_amd_echelonize_dev(word *, int64_t, int64_t, int64_t, int, int32_t *, void *) UNREACHED(int)
int m4ri_amd_inv_dev(word *, int64_t, const word *, int64_t, int64_t, void *) UNREACHED(int)
int m4ri_amd_kernel_left_pluq_dev(word *, int64_t, int64_t, int64_t, word *, int64_t, int, int32_t *, void *) UNREACHED(int)
int m4ri_amd_m4rm_batch_dev(word *, int64_t, int64_t, const word *, int64_t, int64_t, const word *, int64_t, int64_t, int64_t, int64_t, int64_t, int64_t, int,
                            void *) UNREACHED(int)
int m4ri_amd_ple_dev(word *, int64_t, int64_t, int64_t, int32_t *, int32_t *, int32_t *, int64_t, void *) UNREACHED(int)
int m4ri_amd_pluq_dev(word *, int64_t, int64_t, int64_t, int32_t *, int32_t *, int32_t *, int64_t, void *) UNREACHED(int)
int m4ri_amd_pluq_solve_left_dev(const word *, int64_t, int64_t, int64_t, int32_t, const int32_t *, const int32_t *, word *, int64_t, int64_t, int64_t, int, int,
                                 int *, void *) UNREACHED(int)
}

int main() {
  join_family();
  pivot_exchange();
  isd_search();
  isd_collide_search();
  sizes_beyond_int64();
  printf("%d checks, %d failed\n", n, fails);
  return fails != 0;
}
