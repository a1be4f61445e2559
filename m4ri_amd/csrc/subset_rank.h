// subset_rank.h -- the colexicographic ranks of sets of row indices, r(S) = sum_j C(i_j, j + 1) for S = {i_0 < ... < i_{t-1}}, as the
// enumerations of row sums use them (rowsums_batch.hip, rowsums_collide_batch.hip): the binomials on the device and on the host, and one
// step of the unranking from the top element down.  Internal to the file that includes it (an unnamed namespace, as in batch_common.h).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace {

constexpr int64_t RS_K_MAX    = 1024;  // a row index in the 10 low bits of the lane's 32-bit minimum
constexpr int64_t RS_N_MAX    = 1024;  // a word in at most 16 register words (32 VGPRs) per lane
constexpr int64_t RS_T_MAX    = 8;
constexpr int64_t RS_SUMS_MAX = (int64_t)1 << 40;  // the rank fits the key's low 40 bits

// C(c, m) for m = 1 .. 8 and c < 1024, held at 2^62 where it is larger: a rank below 2^40 never meets such an entry
struct BinomTable {
  unsigned long long c[RS_T_MAX][RS_K_MAX];
};
constexpr BinomTable make_binom_table() {
  BinomTable t{};
  const unsigned long long cap = 1ull << 62;
  for (int i = 0; i < RS_K_MAX; ++i) t.c[0][i] = (unsigned long long)i;
  for (int m = 1; m < RS_T_MAX; ++m) {
    t.c[m][0] = 0;
    for (int i = 1; i < RS_K_MAX; ++i) {  // Pascal: C(i, m + 1) = C(i - 1, m + 1) + C(i - 1, m)
      const unsigned long long s = t.c[m][i - 1] + t.c[m - 1][i - 1];
      t.c[m][i]                  = s > cap ? cap : s;
    }
  }
  return t;
}
__device__ const BinomTable rs_binom = make_binom_table();

// C(k, t) on the host, held at 2^41 from the first partial product above 2^40 on (the partial products C(k - t + j, j) only grow)
inline int64_t binom_capped(int64_t k, int64_t t) {
  if (t < 0 || k < t) return 0;
  if (t > k - t) t = k - t;
  int64_t r = 1;
  for (int64_t j = 1; j <= t; ++j) {
    const __int128 x = (__int128)r * (k - t + j) / j;
    if (x > RS_SUMS_MAX) return RS_SUMS_MAX * 2;
    r = (int64_t)x;
  }
  return r;
}

// C(e, j) of an element e < 1024: j <= 3 is arithmetic (so t <= 3 reads no table), above from the table
__device__ __forceinline__ unsigned long long binom_elem(int e, int j) {
  const uint32_t x = (uint32_t)e;
  if (j == 1) return x;
  if (j == 2) return (x * (x - 1)) >> 1;                                        // e = 0: 0 * (2^32 - 1) = 0
  if (j == 3) return e < 3 ? 0 : (unsigned long long)((x * (x - 1)) >> 1) * (x - 2) / 3;
  return rs_binom.c[j - 1][e];
}

// One step of the unranking: element m (1 .. t, the top one first) of the set whose elements above it are out of `rest` already: the
// largest e' < e with C(e', m) <= rest, e the element above (the number of rows for the top one); rest -= C(e', m) for m >= 2.  The lowest is
// the rest itself, the second a square root, the others a bisection in the table of binomials.  rest < C(e, m) <= 2^40.
__device__ __forceinline__ int unrank_step(unsigned long long &rest, int m, int e) {
  int lo = m - 1, hi = e;        // C(m - 1, m) = 0
  if (m == 1) lo = (int)rest;  // nothing follows the lowest: the rest is left as it is
  else if (m == 2) {  // C(lo, 2) <= rest < C(lo + 1, 2): the root in double (8 rest + 1 < 2^44 is exact), then made sure of
    lo = (int)((1.0 + sqrt(8.0 * (double)rest + 1.0)) * 0.5);
    lo = lo < 1 ? 1 : lo > hi - 1 ? hi - 1 : lo;
    while (binom_elem(lo, 2) > rest) --lo;
    while (lo + 1 < hi && binom_elem(lo + 1, 2) <= rest) ++lo;
    rest -= binom_elem(lo, 2);
  } else {
    const unsigned long long *col = rs_binom.c[m - 1];
    while (hi - lo > 1) {
      const int mid = (lo + hi) >> 1;
      if (col[mid] <= rest) lo = mid;
      else hi = mid;
    }
    rest -= col[lo];
  }
  return lo;
}

}  // namespace
