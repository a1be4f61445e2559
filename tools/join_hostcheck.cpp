// The argument checks of the six entry points of the join family (m4ri_amd_row_sums_collide_batch_dev, m4ri_amd_row_sums_collide_list_batch_dev,
// m4ri_amd_row_sums_words_batch_dev, m4ri_amd_lists_collide_batch_dev, m4ri_amd_lists_words_batch_dev, m4ri_amd_sort_rows_batch_dev) and their
// host helpers (plan, slices, units, scratch size) as a stand-alone program for the host sanitizers: every call returns before any HIP call, so no GPU is needed and no
// pointer is dereferenced.  The expected codes are those of tests/test_row_sums_collide_plan.py, test_row_sums_collide_list_plan.py and
// test_lists_collide_plan.py and test_sort_rows_plan.py.  From the repository root:
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
//         -o join_hostcheck m4ri_amd/csrc/rowsums_collide_batch.hip m4ri_amd/csrc/rowsums_words_batch.hip m4ri_amd/csrc/lists_collide_batch.hip \
//         m4ri_amd/csrc/sort_rows_batch.hip tools/join_hostcheck.cpp && ./join_hostcheck
#include <cstdint>
#include <cstdio>
#include "../include/m4ri_amd.h"
#define EXPECT(expr, want) do { long got_ = (long)(expr); if (got_ != (long)(want)) { printf("FAIL %s = %ld, want %ld\n", #expr, got_, (long)(want)); ++fails; } ++n; } while (0)
int main() {
  int fails = 0, n = 0;
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
  printf("%d checks, %d failed\n", n, fails);
  return fails != 0;
}
