// The argument checks of m4ri_amd_pivot_exchange_batch_dev and m4ri_amd_plan_pivot_exchange_batch as a stand-alone program for the host
// sanitizers: every call returns before any HIP call, so no GPU is needed and no pointer is dereferenced.  The expected codes are those of
// tests/test_pivot_exchange_plan.py.  From the repository root:
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
//         -o pivot_exchange_hostcheck m4ri_amd/csrc/pivot_exchange_batch.hip tools/pivot_exchange_hostcheck.cpp && ./pivot_exchange_hostcheck
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include "../include/m4ri_amd.h"
#define EXPECT(expr, want) do { long got_ = (long)(expr); if (got_ != (long)(want)) { printf("FAIL %s = %ld, want %ld\n", #expr, got_, (long)(want)); ++fails; } ++n; } while (0)
int main() {
  int fails = 0, n = 0;
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
  printf("%d checks, %d failed\n", n, fails);
  return fails != 0;
}
