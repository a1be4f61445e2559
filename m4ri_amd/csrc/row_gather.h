// row_gather.h -- the bit gather along a row that the column permutations share: colperm_gather_kernel (echelon.hip, one map for
// all rows) and qtri_gather_kernel (ple.hip, a map per row).  Internal to the file that includes it (an unnamed namespace, as in
// transpose_block.h).
#pragma once
#include <hip/hip_runtime.h>
#include "gf2_common.h"

namespace {

// new row[c] = old row[map[c]] for the words [w0, w1) of the row, by a workgroup of THREADS threads: the old row's `width` words
// staged in the kernel's dynamic LDS (LDSROW) or read from `copy`, a copy made by the caller; a wave per output word, lane = bit,
// the word assembled by a ballot.
template <bool LDSROW, int THREADS>
__device__ __forceinline__ void gather_row(word *row, int64_t width, const word *copy, const uint32_t *map, int64_t w0, int64_t w1, int64_t ncols) {
  extern __shared__ word lrow[];
  const word *src;
  if (LDSROW) {
    for (int64_t w = threadIdx.x; w < width; w += THREADS) lrow[w] = row[w];
    __syncthreads();
    src = lrow;
  } else {
    src = copy;
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int64_t w = w0 + wave; w < w1; w += THREADS / 64) {
    const int64_t c = w * 64 + lane;
    int bit         = 0;
    if (c < ncols) {
      const uint32_t sc = map[c];
      bit               = (int)((src[sc >> 6] >> (sc & 63)) & 1);
    }
    const word v = __ballot(bit);
    if (lane == 0) row[w] = v;
  }
}

}  // namespace
