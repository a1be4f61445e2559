// gf2_internal.h -- the functions the library's translation units call across files, declared once (and the HIPTRY macro they return errors with).
//
// Every file that defines one of them includes this header, so the compiler checks each definition against the one
// declaration here.  C linkage: tools/leaf_check.cpp links the leaf sources directly, and so do the two test-only
// libraries of build.py (libm4ri_amd_passes.so for tests/pass_lib.py, libm4ri_amd_leaves.so for tests/leaf_lib.py), which
// export the launchers their tests call.  None of these names leaves the product's shared library (build.py's export
// map lists only include/m4ri_amd.h).
#pragma once
#include <hip/hip_runtime.h>
#include <type_traits>
#include <vector>
#include "gf2_common.h"

// return the HIP error of `expr` (a hipError_t or an int status) from the enclosing int-returning function
#define HIPTRY(expr)                                  \
  do {                                                \
    hipError_t e_ = (hipError_t)(expr);               \
    if (e_ != hipSuccess) return (int)e_;             \
  } while (0)

// A run-time flag as a template argument: calls f(std::true_type{}) or f(std::false_type{}).  With a generic lambda,
//   with_bool(acc, [&](auto ACC) { hipLaunchKernelGGL((kernel<decltype(ACC)::value>), ...); });
// instantiates and launches the kernel for both values of the flag from one launch statement.  The launchers nest it for two flags.
template <typename F>
inline void with_bool(bool flag, F &&f) {
  if (flag) f(std::true_type{});
  else f(std::false_type{});
}

// words of the staging arena a device copy of a rows x ncols matrix takes: rows at an even stride, in 256-byte granules
inline size_t dev_words(int64_t rows, int64_t ncols) {
  const int64_t w = words_of(ncols), st = (w + 1) & ~(int64_t)1;
  return (((size_t)(rows > 0 ? rows : 1) * (size_t)(st > 0 ? st : 2)) + 31) & ~(size_t)31;
}

// host_pipeline_plan.cpp: the plan of the host block pipeline -- blocks C_ij (+)= A_ik * B_kj between the cuts (each list from 0 to its
// dimension) and the arena words of all blocks of A, B and C.  A requested grid (gi, gj, gk >= 1) the shape refuses counts as none.
struct HostPipelinePlan {
  bool pipelined = false;
  std::vector<int64_t> rcut, ccut, kcut;
  size_t arena_words = 0;
  int gi() const { return (int)rcut.size() - 1; }
  int gj() const { return (int)ccut.size() - 1; }
  int gk() const { return (int)kcut.size() - 1; }
  int64_t rows(int i) const { return rcut[(size_t)i + 1] - rcut[(size_t)i]; }
  int64_t cols(int j) const { return ccut[(size_t)j + 1] - ccut[(size_t)j]; }
  int64_t inner(int k) const { return kcut[(size_t)k + 1] - kcut[(size_t)k]; }
};
HostPipelinePlan gf2_plan_host_pipeline(int64_t m, int64_t l, int64_t n, size_t min_bytes, int gi, int gj, int gk);

extern "C" {

// ---- the M4RM leaves --------------------------------------------------------------------------------------------------------
// m4rm_leaf.hip: generation 1 (plain A, rg row groups; the variant takes the developer's unroll / pipeline bits)
hipError_t gf2_launch_m4rm_leaf(hipStream_t stream, LeafArgs a, int rg);
hipError_t gf2_launch_m4rm_leaf_variant(hipStream_t stream, LeafArgs a, int rg, int ug, int pipe);
// m4rm_small.hip: the one-launch kernel of small products ("generation 5") and its inner split
hipError_t gf2_launch_m4rm_small(hipStream_t stream, LeafArgs a);
int gf2_m4rm_small_ksplit(int64_t tiles, int64_t wl, int cus, int64_t c_words);
// a4_pack.hip: the packed, chunk-major A of generation 4 (words of scratch it needs; the pack pass)
int64_t gf2_m4rm8_a4_words(int64_t m, int64_t l, int64_t batch);
hipError_t gf2_launch_a4_pack_rot(hipStream_t stream, LeafArgs a, word *a4_ws, int rot);
// m4rm8q_leaf.hip: generation 4 (the split the kernel will really use; the launch)
int gf2_m4rm8q_effective_ksplit(int64_t l, int ksplit);
hipError_t gf2_launch_m4rm8q(hipStream_t stream, LeafArgs a, word *a4_ws);

// ---- the fused passes of `levels` Strassen-Winograd levels (aux_kernels.hip) ------------------------------------------------
// levels 1 ... 4 through the Winograd passes, or (scheme != 0, levels 2 ... 4) through the rank-R scheme of the 4 x 4 x 4 block
// product (scheme_passes.hip).  Down: nparents parents of 2^levels crows rows x 2^levels cw words (row stride `stride`, `bs` words
// apart) -> their descendants, crows x cw words each, back to back; bside selects the B side's operand sums.  Down_pack: the A side
// written straight into generation 4's packed form at a4.  rot: the index-byte rotation of the Winograd passes, 0 (plain chunk-major) or 1
// (generation 4's); with any other value they return hipErrorInvalidValue and write nothing.  The scheme passes ignore rot (they always
// write generation 4's rotation).  Up: the products back into the parents (acc != 0: added onto them).
hipError_t gf2_launch_pass_down(hipStream_t s, int levels, int scheme, int bside, const word *src, int64_t stride, int64_t bs, word *dst,
                                int64_t nparents, int64_t crows, int64_t cw);
hipError_t gf2_launch_pass_down_pack(hipStream_t s, int levels, int scheme, const word *src, int64_t stride, int64_t bs, word *a4,
                                     int64_t nparents, int64_t crows, int64_t cw, int rot);
hipError_t gf2_launch_pass_up(hipStream_t s, int levels, int scheme, int acc, const word *prod, word *dst, int64_t stride, int64_t bs,
                              int64_t nparents, int64_t crows, int64_t cw);
// can the Winograd down_pack pass of `levels` levels take this parent and packed output (descendants of crows x cw words)?
int gf2_pass_down_pack_ok(int levels, const word *src, int64_t stride, int64_t bs, const word *a4, int64_t crows, int64_t cw);

// scheme_passes.hip: the scheme's rank, leaves per ancestor of a `levels`-level pass, whether its passes take these leaf shapes
int gf2_scheme444_rank(void);
int64_t gf2_scheme444_leaves(int levels);
int gf2_scheme444_ok(int levels, int64_t a_rows, int64_t a_cw, int64_t b_rows, int64_t b_cw);
hipError_t gf2_launch_scheme_down(hipStream_t s, int levels, int bside, const word *anc, int64_t p_stride, int64_t p_bs, word *child,
                                  int64_t nparents, int64_t crows, int64_t cw);
hipError_t gf2_launch_scheme_down_pack(hipStream_t s, int levels, const word *anc, int64_t p_stride, int64_t p_bs, word *a4,
                                       int64_t nparents, int64_t crows, int64_t cw);
hipError_t gf2_launch_scheme_up(hipStream_t s, int levels, int acc, const word *prod, word *anc, int64_t o_stride, int64_t o_bs,
                                int64_t nparents, int64_t crows, int64_t cw);

// ---- streaming helpers (aux_kernels.hip) ------------------------------------------------------------------------------------
// op 0: C = A ^ B, 1: C = A, 2: C = 0 (whole words of `w` words per row)
hipError_t gf2_launch_rowwise(hipStream_t s, int op, word *C, int64_t cs, const word *A, int64_t as, const word *B, int64_t bs,
                              int64_t rows, int64_t w);
hipError_t gf2_launch_xor_masked(hipStream_t s, word *C, int64_t cs, const word *A, int64_t as, const word *B, int64_t bs,
                                 int64_t rows, int64_t ncols);
hipError_t gf2_launch_copy_masked(hipStream_t s, word *C, int64_t cs, const word *A, int64_t as, int64_t rows, int64_t ncols);
hipError_t gf2_launch_reduce_partials(hipStream_t s, int acc, word *C, int64_t cs, int64_t cbs, int64_t m, int64_t wn, int64_t tile_rows,
                                      int64_t tw, int64_t tiles_m, int64_t tiles_n, int64_t tile_base, int64_t ntiles, int ks,
                                      const word *Cpart);
hipError_t gf2_launch_zero_tiles(hipStream_t s, word *C, int64_t cs, int64_t cbs, int64_t m, int64_t wn, int64_t tile_rows, int64_t tw,
                                 int64_t tiles_m, int64_t tiles_n, int64_t tile_base, int64_t ntiles);
hipError_t gf2_launch_mask_tail(hipStream_t s, word *M, int64_t stride, int64_t rows, int64_t ncols);
hipError_t gf2_launch_fill_splitmix(hipStream_t s, word *M, int64_t stride, int64_t rows, int64_t ncols, uint64_t seed);
hipError_t gf2_launch_fill_splitmix_rows(hipStream_t s, word *M, int64_t stride, int64_t row0, int64_t rows, int64_t ncols,
                                         uint64_t seed);

// ---- transposes (transpose.hip) -------------------------------------------------------------------------------------------
// the tile kernel on `batch` members (member b: nrows x ncols at A + b * a_bs -> ncols x nrows at D + b * d_bs); one member is
// m4ri_amd_transpose_dev, many are path 2 of m4ri_amd_transpose_batch_dev (transpose_batch.hip)
hipError_t gf2_launch_transpose_tiles(hipStream_t st, word *D, int64_t d_stride, int64_t d_bs, const word *A, int64_t a_stride, int64_t a_bs,
                                      int64_t nrows, int64_t ncols, int64_t batch);

// ---- solver glue (solve.hip) ------------------------------------------------------------------------------------------------
// dst (r rows of words_of(r) words) <- a clean copy of the leading r x r block of A, its last word masked to r columns: the
// triangular solves split their triangle into blocks that go to the multiply engine as operands, which must not carry bits of
// the neighbouring columns
int gf2_square_copy(word *dst, const word *A, int64_t stride, int64_t r, hipStream_t st);

// ---- host side ----------------------------------------------------------------------------------------------------------------
double gf2_small_host_cost(int64_t m, int64_t l, int64_t n);  // small_host.cpp: word operations of the host product
int gf2_multi_wanted(int64_t m, int64_t l, int64_t n);         // multi.hip: would mzd_mul_mp spread this product over devices?
void gf2_release_multi(void);                                  // multi.hip: the per-rank arenas of the multi-device path
void gf2_release_staging(void);                                // mzd_api.hip: the host entry points' staging arena

}  // extern "C"
