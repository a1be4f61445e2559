// The argument checks of m4ri_amd_lists_collide_batch_dev / m4ri_amd_lists_words_batch_dev and the two host helpers of
// m4ri_amd/csrc/lists_collide_batch.hip as a stand-alone program for the host sanitizers: every call returns before any HIP call, so no
// GPU is needed and no pointer is dereferenced.  From the repository root:
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
//         -o lists_collide_hostcheck m4ri_amd/csrc/lists_collide_batch.hip tools/lists_collide_hostcheck.cpp && ./lists_collide_hostcheck
#include <cstdint>
#include <cstdio>
#include "../include/m4ri_amd.h"
#define EXPECT(expr, want) do { long got_ = (long)(expr); if (got_ != (long)(want)) { printf("FAIL %s = %ld, want %ld\n", #expr, got_, (long)(want)); ++fails; } ++n; } while (0)
int main() {
  int fails = 0, n = 0;
  word *X = (word *)(1ull << 20), *Y = (word *)(1ull << 22), *V = (word *)(1ull << 24), *W = (word *)(1ull << 32);
  int32_t *C = (int32_t *)(1ull << 26), *S = (int32_t *)(1ull << 33);
  int64_t *H = (int64_t *)(1ull << 28), *L = (int64_t *)(1ull << 29), *K = (int64_t *)(1ull << 30), *N = (int64_t *)(1ull << 31);
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
  printf("%d checks, %d failed\n", n, fails);
  return fails != 0;
}
