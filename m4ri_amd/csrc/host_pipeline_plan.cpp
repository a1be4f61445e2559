// host_pipeline_plan.cpp -- every decision of the host block pipeline (mzd_api.hip run_pipelined executes this plan and decides nothing
// itself): whether a product from host memory is cut into blocks  C_ij (+)= A_ik * B_kj, on which gi x gj x gk grid, where the cuts fall,
// and the words of the staging arena the blocks take.  Arithmetic on m, l, n alone: no HIP call, no environment, no global, so it is
// exported (m4ri_amd_plan_host_pipeline) and pinned without a GPU (tests/test_host_pipeline_plan.py).
#include "gf2_internal.h"
#include "../../include/m4ri_amd.h"

namespace {

// cut number i of `parts` through `total`: on the coarsest grid of unit0 * 2^j (j <= 5) that moves it by at most 8 % of a part, else
// on whole tiles of rows / whole words
int64_t coarse_cut(int64_t total, int parts, int i, int64_t unit0, int64_t prev, bool rows) {
  const int64_t target = total * i / parts, fine = rows ? ((target + 4095) / 4096) * 4096 : (target / 64) * 64;
  for (int j = 5; j >= 1; --j) {
    const int64_t unit = unit0 << j, c = ((target + unit / 2) / unit) * unit;
    const int64_t off = c > target ? c - target : target - c;
    if (c > prev && c < total && off * 100 <= 8 * (total / parts)) return c;
  }
  return fine;
}

}  // namespace

HostPipelinePlan gf2_plan_host_pipeline(int64_t m, int64_t l, int64_t n, size_t min_bytes, int gi, int gj, int gk) {
  HostPipelinePlan p;
  const size_t bytes = ((size_t)m * (size_t)words_of(l) + (size_t)l * (size_t)words_of(n) + (size_t)m * (size_t)words_of(n)) * 8;
  if (min_bytes == 0 || bytes < min_bytes || m < 4 * 4096) return p;
  p.pipelined = true;
  // a requested grid counts when the shape has the rows, words and inner bits for it
  const bool asked = gi >= 1 && gj >= 1 && gk >= 1 && m >= (int64_t)gi * 4096 && n >= (int64_t)gj * 64 && l >= (int64_t)gk * 64;
  p.rcut.push_back(0);
  if (asked || n >= 16384) {
    if (!asked) {
      gi = 2; gj = 2;
      // from 65536^3 on also two slices of the inner dimension: the blocks stay cubes (full Strassen depth) and the first
      // product waits for half as many bytes (43.1 instead of 46.0 ms; at 32768^3 the plain 2 x 2 is 3 % faster)
      gk = (l >= 65536 && m >= 65536 && n >= 65536) ? 2 : 1;
    }
    // rows are cut on the coarsest grid of 4096 * 2^j rows that moves the cut by at most 8 % of a block: the engine gives a block of
    // k * 4096 * 2^L rows its full Strassen depth (engine.hip plan_row_blocks) -- 65664 rows cut 32768 + 32896, not 36864 + 28800
    for (int i = 1; i < gi; ++i) p.rcut.push_back(coarse_cut(m, gi, i, 4096, p.rcut.back(), true));
  } else {
    // narrow products: slabs of a quarter of the rows on whole 4096-row tiles (16385 rows: four slabs and a fifth of one row)
    gj = 1; gk = 1;
    const int64_t srows = ((m / 4 + 4095) / 4096) * 4096;
    for (int64_t r = srows; r < m; r += srows) p.rcut.push_back(r);
  }
  p.rcut.push_back(m);
  // columns and inner bits likewise, on 1024 * 2^j bits (whole words at every Strassen level the block will use): no strips in the
  // blocks before the last
  p.ccut.push_back(0);
  for (int j = 1; j < gj; ++j) p.ccut.push_back(coarse_cut(n, gj, j, 1024, p.ccut.back(), false));
  p.ccut.push_back(n);
  p.kcut.push_back(0);
  for (int k = 1; k < gk; ++k) p.kcut.push_back(coarse_cut(l, gk, k, 1024, p.kcut.back(), false));
  p.kcut.push_back(l);
  for (int i = 0; i < p.gi(); ++i)
    for (int k = 0; k < p.gk(); ++k) p.arena_words += dev_words(p.rows(i), p.inner(k));
  for (int k = 0; k < p.gk(); ++k)
    for (int j = 0; j < p.gj(); ++j) p.arena_words += dev_words(p.inner(k), p.cols(j));
  for (int i = 0; i < p.gi(); ++i)
    for (int j = 0; j < p.gj(); ++j) p.arena_words += dev_words(p.rows(i), p.cols(j));
  return p;
}

extern "C" int m4ri_amd_plan_host_pipeline(int64_t m, int64_t l, int64_t n, int64_t min_bytes, int gi, int gj, int gk, int64_t *rcut,
                                           int64_t *ccut, int64_t *kcut, int cap, int *grid, int64_t *arena_words) {
  if (m < 0 || l < 0 || n < 0 || min_bytes < 0) return 0;
  const HostPipelinePlan p = gf2_plan_host_pipeline(m, l, n, (size_t)min_bytes, gi, gj, gk);
  if (!p.pipelined) return 0;
  if (grid) { grid[0] = p.gi(); grid[1] = p.gj(); grid[2] = p.gk(); }
  if (arena_words) *arena_words = (int64_t)p.arena_words;
  const std::vector<int64_t> *cuts[3] = {&p.rcut, &p.ccut, &p.kcut};
  int64_t *out[3] = {rcut, ccut, kcut};
  for (int d = 0; d < 3; ++d)
    if (out[d] && (int64_t)cuts[d]->size() > (int64_t)cap) return -1;
  for (int d = 0; d < 3; ++d)
    for (size_t q = 0; out[d] && q < cuts[d]->size(); ++q) out[d][q] = (*cuts[d])[q];
  return 1;
}
