/* include/m4ri_amd.h -- C ABI of libm4ri_amd.so, the MI355X-native drop-in for M4RI's dense GF(2)
 * multiply path (mzd_mul -> Strassen-Winograd -> M4RM).  Plain pointers and sizes only.
 *
 * Part 1 is the drop-in boundary: the exact symbols (names, signatures, semantics, fatal-error
 * behaviour) a libm4ri user of this path binds, each citing the reference declaration it replaces.
 * Part 2 is the device-resident API those entry points are built from; hosts that keep matrices
 * in HBM across calls (bench.py, the multi-GPU driver, chains of products) call it directly.
 *
 * All file:line citations are relative to the reference tree (malb/m4ri @ 20251207).
 */
#ifndef M4RI_AMD_H
#define M4RI_AMD_H

#include <stdint.h>
#include <stddef.h>
#include <stdio.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- types: m4ri/misc.h:72,81,87 -------------------------------------------------------------- */
typedef int rci_t;      /* row/column index */
typedef int64_t wi_t;   /* word index       */
typedef uint64_t word;  /* 64 columns, LSB = lowest column */

/* mzd_t: layout-identical to m4ri/mzd.h:68-99 (sizeof == 64; nrows@0 ncols@4 width@8 rowstride@16
 * flags@24 high_bitmask@48 data@56).  Bit (r,c) = (data[r*rowstride + c/64] >> (c%64)) & 1.
 * A program that already includes <m4ri/m4ri.h> must NOT include this header's struct: define
 * M4RI_AMD_NO_MZD_T first and use M4RI's own declaration -- the two are the same bytes. */
#ifndef M4RI_AMD_NO_MZD_T
typedef struct mzd_t {
  rci_t nrows;
  rci_t ncols;
  wi_t width;
  wi_t rowstride;
  uint8_t flags;        /* 0x2 non-zero excess, 0x4 windowed (mzd.h:144,150) */
  uint8_t padding[23];
  word high_bitmask;
  word *data;
} mzd_t;
#endif

/* mzp_t: layout-identical to m4ri/mzp.h:37-49 (LAPACK-style transpositions: values[i] is the index swapped
 * with i, for i ascending). */
#ifndef M4RI_AMD_NO_MZD_T
typedef struct mzp_t {
  rci_t *values;
  rci_t length;
} mzp_t;
#endif

/* =================================================================================================
 * Part 1 -- drop-in entry points (host mzd_t in, host mzd_t out, blocking)
 *
 * Common contract: C == NULL => C is allocated with the host program's mzd_init
 * (resolved with dlsym; see m4ri_amd_mzd_init below when no libm4ri is loaded) and returned;
 * otherwise C must be A->nrows x B->ncols.  A, B, C may be windows; words at index >= width and
 * bits outside high_bitmask of a windowed C are never written; for a non-window C they end up 0.
 * `cutoff` and `k` are performance hints: every value yields the same bits.  A == B is legal.
 * Dimension mismatch or cutoff < 0 prints to stderr and abort()s, like m4ri_die (misc.c:36-42);
 * so does any HIP failure -- there is no CPU fallback.
 * ============================================================================================== */

/* C = A*B.  Replaces mzd_mul, m4ri/strassen.h:52 (strassen.c:345-365). */
mzd_t *mzd_mul(mzd_t *C, mzd_t const *A, mzd_t const *B, int cutoff);
/* C += A*B.  Replaces mzd_addmul, m4ri/strassen.h:68 (strassen.c:675-700). */
mzd_t *mzd_addmul(mzd_t *C, mzd_t const *A, mzd_t const *B, int cutoff);
/* Unchecked variants L4 calls directly.  m4ri/strassen.h:88, :109, :126. */
mzd_t *_mzd_mul_even(mzd_t *C, mzd_t const *A, mzd_t const *B, int cutoff);
mzd_t *_mzd_addmul_even(mzd_t *C, mzd_t const *A, mzd_t const *B, int cutoff);
mzd_t *_mzd_addmul(mzd_t *C, mzd_t const *A, mzd_t const *B, int cutoff);
/* Squaring entry points mzd_mul/_mzd_addmul dispatch to when A == B; exported by libm4ri although
 * not declared in strassen.h (strassen.c:210, :528). */
mzd_t *_mzd_sqr_even(mzd_t *C, mzd_t const *A, int cutoff);
mzd_t *_mzd_addsqr_even(mzd_t *C, mzd_t const *A, int cutoff);
/* M4RM leaf only (no Strassen).  m4ri/brilliantrussian.h:274, :291, :317. */
mzd_t *mzd_mul_m4rm(mzd_t *C, mzd_t const *A, mzd_t const *B, int k);
mzd_t *mzd_addmul_m4rm(mzd_t *C, mzd_t const *A, mzd_t const *B, int k);
mzd_t *_mzd_mul_m4rm(mzd_t *C, mzd_t const *A, mzd_t const *B, int k, int clear);
/* OpenMP block-parallel entry points, m4ri/mp.h:47, :62 (mp.c:277-324): same results.  With several
 * devices configured (part 4: every visible GPU by default) and min(m, l, n) at or above the multi-device
 * threshold, the sub-products of the top Strassen-Winograd level(s) are spread over the devices; otherwise
 * -- one GPU, small products, pinned operands -- they run the single-GPU schedule (where the GPU grid
 * replaces the omp sections). */
mzd_t *mzd_mul_mp(mzd_t *C, mzd_t const *A, mzd_t const *B, int cutoff);
mzd_t *mzd_addmul_mp(mzd_t *C, mzd_t const *A, mzd_t const *B, int cutoff);

/* ---- triangular solves with a matrix right-hand side (the callers of the multiply
 * path one step up; TRSM base cases are where an LD_PRELOADed PLE / solve spends its CPU time) ------------
 * B <- L^-1 B / B <- U^-1 B in place, T unit triangular: its diagonal and its other triangle are never read
 * (m4ri/triangular.c:406-455, :467-514), B and T may be windows, the bits of B's last word outside its
 * columns are kept.  The solution is unique, so every schedule gives the reference's bits; `k` and `cutoff`
 * are hints.  m4ri/triangular.h:115, :127, :142, :153; m4ri/triangular_russian.h:43, :55. */
void mzd_trsm_lower_left(mzd_t const *L, mzd_t *B, const int cutoff);
void _mzd_trsm_lower_left(mzd_t const *L, mzd_t *B, const int cutoff);
void _mzd_trsm_lower_left_russian(mzd_t const *L, mzd_t *B, int k);
void mzd_trsm_upper_left(mzd_t const *U, mzd_t *B, const int cutoff);
void _mzd_trsm_upper_left(mzd_t const *U, mzd_t *B, const int cutoff);
void _mzd_trsm_upper_left_russian(mzd_t const *U, mzd_t *B, int k);
/* The right-hand forms, B <- B U^-1 / B <- B L^-1 (X T = B): m4ri/triangular.h:50, :64, :82, :100 (triangular.c:41-130,
 * :301-393).  Same rules: unique solution, diagonal and other triangle never read, windows allowed. */
void mzd_trsm_upper_right(mzd_t const *U, mzd_t *B, const int cutoff);
void _mzd_trsm_upper_right(mzd_t const *U, mzd_t *B, const int cutoff);
void mzd_trsm_lower_right(mzd_t const *L, mzd_t *B, const int cutoff);
void _mzd_trsm_lower_right(mzd_t const *L, mzd_t *B, const int cutoff);

/* ---- PLE decomposition -----------------------------------------------------------
 * A = P L E Q in place: returns the rank r; afterwards the first r columns of A hold L below the diagonal (unit
 * diagonal implied), E sits in the rows 0..r-1 from each row's pivot column on, P (A->nrows entries) and Q
 * (A->ncols entries) hold the row / column transpositions -- exactly the reference's output, which is fixed by
 * its pivoting rule (first row with a set bit, columns left to right), not by its schedule -- except the entries
 * of Q behind the rank, which mzd_ple / _mzd_ple fill by their recursion on column halves and _mzd_ple_russian
 * leaves as the identity; both are reproduced (M4RI_AMD_PLE_CUTOFF below).  `cutoff`, `k`: hints.  m4ri/ple.h:103, :137; m4ri/ple_russian.h:81 (ple.c:33-171, ple_russian.c:380-617). */
rci_t mzd_ple(mzd_t *A, mzp_t *P, mzp_t *Q, const int cutoff);
rci_t _mzd_ple(mzd_t *A, mzp_t *P, mzp_t *Q, const int cutoff);
rci_t _mzd_ple_russian(mzd_t *A, mzp_t *P, mzp_t *Q, int k);
/* A = P L U Q in place (m4ri/ple.h:70, :120; ple_russian.h:98; ple.c:41-60): the PLE above, then the columns of the
 * first r rows permuted so that U is upper triangular with its pivots on the diagonal
 * (mzd_apply_p_right_trans_tri, m4ri/mzp.h:202, mzp.c:279-293, exported as well). */
rci_t mzd_pluq(mzd_t *A, mzp_t *P, mzp_t *Q, const int cutoff);
rci_t _mzd_pluq(mzd_t *A, mzp_t *P, mzp_t *Q, const int cutoff);
rci_t _mzd_pluq_russian(mzd_t *A, mzp_t *P, mzp_t *Q, int k);
void mzd_apply_p_right_trans_tri(mzd_t *A, mzp_t const *Q);

/* ---- echelon forms (the drivers over the elimination kernels) ---------------------------
 * Row echelon form (full == 0) or reduced row echelon form (full != 0) of A in place; returns the rank.  The three
 * drivers of the reference (Four-Russians strips, PLE/PLUQ based, density heuristic) leave the same matrix -- their
 * common pivoting rule fixes it -- so all of them map to one device routine (echelon.hip); `k`, `heuristic` and
 * `threshold` are hints.  m4ri/echelonform.h:50, :63, :79; m4ri/brilliantrussian.h:215 (echelonform.c:29-139,
 * brilliantrussian.c:603-841). */
rci_t mzd_echelonize(mzd_t *A, int full);
rci_t mzd_echelonize_m4ri(mzd_t *A, int full, int k);
rci_t mzd_echelonize_pluq(mzd_t *A, int full);
rci_t mzd_echelonize_naive(mzd_t *A, int full); /* m4ri/mzd.h:740 (mzd.c:208-233): plain Gaussian elimination -- same pivoting rule, same result */
rci_t _mzd_echelonize_m4ri(mzd_t *A, const int full, int k, int heuristic, const double threshold);
/* A <- A * P / A * P^T: the column transpositions (i, P[i]) on every row, i descending / ascending.
 * m4ri/mzp.h:142, :153 (mzp.c:193-260). */
void mzd_apply_p_right(mzd_t *A, mzp_t const *P);
void mzd_apply_p_right_trans(mzd_t *A, mzp_t const *P);

/* ---- linear systems, kernels, inverses (the drivers over PLUQ; solve.hip) -------------------------------------
 * mzd_solve_left (m4ri/solve.h:50, :123; solve.c:30-152): A X = B.  A (m x n) is left holding its PLUQ decomposition, B
 * (max(m, n) rows) the solution in its first n rows with the undefined rows zero; returns 0, or -1 when
 * inconsistency_check finds no solution.  mzd_pluq_solve_left (solve.h:76, :103): the same from a decomposition.
 * mzd_kernel_left_pluq (solve.h:140; solve.c:154-191): A <- its PLUQ; returns a new n x (n - rank) matrix whose columns
 * span {x : A x = 0}, or NULL when the rank is n.  mzd_inv_m4ri (m4ri/brilliantrussian.h:256; .c:971-997): B <- A^-1
 * through the reduced echelon form of [A | I] (B == NULL: a new matrix).  mzd_apply_p_left{,_trans} (m4ri/mzp.h:120,
 * :131; mzp.c:65-81): the row transpositions (i, P[i]) ascending / descending. */
int mzd_solve_left(mzd_t *A, mzd_t *B, int const cutoff, int const inconsistency_check);
int _mzd_solve_left(mzd_t *A, mzd_t *B, int const cutoff, int const inconsistency_check);
int mzd_pluq_solve_left(mzd_t const *A, rci_t rank, mzp_t const *P, mzp_t const *Q, mzd_t *B, int const cutoff, int const inconsistency_check);
int _mzd_pluq_solve_left(mzd_t const *A, rci_t rank, mzp_t const *P, mzp_t const *Q, mzd_t *B, int const cutoff, int const inconsistency_check);
mzd_t *mzd_kernel_left_pluq(mzd_t *A, int const cutoff);
mzd_t *mzd_inv_m4ri(mzd_t *B, mzd_t const *A, int k);
void mzd_apply_p_left(mzd_t *A, mzp_t const *P);
void mzd_apply_p_left_trans(mzd_t *A, mzp_t const *P);

/* ---- transposes and triangular inverses (transpose.hip, trsm.hip) ------------------------------------------------
 * mzd_transpose (m4ri/mzd.h:611; mzd.c:1118-1139): DST <- A^T (DST == NULL: a new matrix; wrong dimensions die with the
 * reference's message).  DST may be A itself here (the reference forbids it).
 * mzd_trtri_upper (m4ri/triangular.h:163; triangular.c:518-547) and mzd_trtri_upper_russian (m4ri/triangular_russian.h:66;
 * .c:384-470): A <- A^-1 in place for a unit upper triangular A.  As in the reference the diagonal and the lower
 * triangle are not written; unlike the reference they are not read either: a zero on the diagonal (a singular input,
 * outside the reference's contract) makes the reference's result depend on its blocking, while this library returns
 * the inverse of the unit-diagonal matrix. */
mzd_t *mzd_transpose(mzd_t *DST, mzd_t const *A);
mzd_t *mzd_trtri_upper(mzd_t *A);
mzd_t *mzd_trtri_upper_russian(mzd_t *A, int k);

/* ---- the table primitives of M4RI's elimination routines -----------------------------
 * mzd_make_table (m4ri/brilliantrussian.h:56, .c:163-211): T[i], i = 1 .. 2^k - 1, = the Gray-code combinations of
 * rows r .. r+k-1 of M from word c/64 on (first word masked below column c, last word by M's column mask), and
 * L[ord[i]] = i.  mzd_process_rows{,2..6} (brilliantrussian.h:74-190, .c:213-601): for every row in
 * [startrow, endrow) the k-bit strip at column startcol is cut into N groups, group t looked up in L_t, and
 * T_t's row XORed onto the row from word startcol/64 on.  Same bits as the reference for tables made by
 * mzd_make_table (the k == 1 shortcut of mzd_process_rows, .c:220-296, reads T's row 1 without L). */
void mzd_make_table(mzd_t const *M, rci_t r, rci_t c, int k, mzd_t *T, rci_t *L);
void mzd_process_rows(mzd_t *M, rci_t startrow, rci_t endrow, rci_t startcol, int k, mzd_t const *T, rci_t const *L);
void mzd_process_rows2(mzd_t *M, rci_t startrow, rci_t endrow, rci_t startcol, int k, mzd_t const *T0, rci_t const *L0, mzd_t const *T1,
                       rci_t const *L1);
void mzd_process_rows3(mzd_t *M, rci_t startrow, rci_t endrow, rci_t startcol, int k, mzd_t const *T0, rci_t const *L0, mzd_t const *T1,
                       rci_t const *L1, mzd_t const *T2, rci_t const *L2);
void mzd_process_rows4(mzd_t *M, rci_t startrow, rci_t endrow, rci_t startcol, int k, mzd_t const *T0, rci_t const *L0, mzd_t const *T1,
                       rci_t const *L1, mzd_t const *T2, rci_t const *L2, mzd_t const *T3, rci_t const *L3);
void mzd_process_rows5(mzd_t *M, rci_t startrow, rci_t endrow, rci_t startcol, int k, mzd_t const *T0, rci_t const *L0, mzd_t const *T1,
                       rci_t const *L1, mzd_t const *T2, rci_t const *L2, mzd_t const *T3, rci_t const *L3, mzd_t const *T4,
                       rci_t const *L4);
void mzd_process_rows6(mzd_t *M, rci_t startrow, rci_t endrow, rci_t startcol, int k, mzd_t const *T0, rci_t const *L0, mzd_t const *T1,
                       rci_t const *L1, mzd_t const *T2, rci_t const *L2, mzd_t const *T3, rci_t const *L3, mzd_t const *T4,
                       rci_t const *L4, mzd_t const *T5, rci_t const *L5);

/* ---- matrix I/O formats (pure host code, m4ri/io.h:44-193, io.c:49-357) -----------------
 * Text rows "[1 1 :...|...]" (64-bit groups, ':' every four entries); a row-major string of '0'/'1'; the JCF sparse
 * text format ("m n 2", number of non-zeros, then signed 1-based column indices, a negative index starts the next
 * row); 1-bit grayscale PNG, one pixel per entry, black = 1 (written and parsed directly on zlib: libpng is what the
 * reference uses, the files are the same).  Matrices returned are allocated like C == NULL results. */
void mzd_fprint_row(FILE *stream, mzd_t const *M, const rci_t i);
void mzd_fprint(FILE *stream, mzd_t const *M);
void mzd_print(mzd_t const *M);
mzd_t *mzd_from_str(rci_t m, rci_t n, const char *str);
mzd_t *mzd_from_jcf(const char *fn, int verbose);
mzd_t *mzd_from_png(const char *fn, int verbose);
int mzd_to_png(const mzd_t *A, const char *fn, int compression_level, const char *comment, int verbose);

/* Allocation used for C == NULL when the process has no libm4ri (standalone use, our tests):
 * same layout rules as mzd_init/mzd_free (mzd.c:142-157,179-185). */
mzd_t *m4ri_amd_mzd_init(rci_t r, rci_t c);
void m4ri_amd_mzd_free(mzd_t *A);
/* Frees a C == NULL result with the allocator it came from (the host program's mzd_free when its
 * mzd_init produced it, m4ri_amd_mzd_free otherwise) -- for bindings that cannot call mzd_free. */
void m4ri_amd_result_free(mzd_t *A);

/* =================================================================================================
 * Part 2 -- device-resident API.  Matrices live in HBM in the same bit-packed row-major layout:
 * `data` is a device pointer to word (0,0), `stride` the distance between rows in words.
 * Invariant the caller keeps: bits at column >= ncols inside the last word of a row are zero
 * (m4ri_amd_fill_dev and every product below preserve it; m4ri_amd_mask_tail_dev establishes it).
 * All calls are asynchronous on `stream` (a hipStream_t; NULL = the null stream) unless noted and
 * return 0 on success or a hipError_t value.
 * ============================================================================================== */

/* Bind the calling thread's HIP device for later calls and create the engine (idempotent). */
int m4ri_amd_init(int device);
int m4ri_amd_device_count(void);

/* C (+)= A*B on the device: Strassen-Winograd levels over batched M4RM leaves.
 * C: m x n, A: m x l, B: l x n.  add != 0 accumulates.  cutoff: 0 = engine default, otherwise the
 * reference's meaning (recurse until 3*dim < 4*cutoff for some dim, strassen.c:39,51).
 * Asynchronous on `stream`.  The engine has ONE workspace per device, so a product issued on another
 * stream than the previous one first waits (on the device) for that one to finish; several host
 * threads may call concurrently (the host side is serialised).
 * Limits of the four product calls (m4ri_amd_mul_dev, m4ri_amd_m4rm_dev and their batch forms), each hipErrorInvalidValue
 * before any HIP call and whatever the depth (`cutoff`, the engine's own choice of levels), so C is never partly written: the
 * leaf kernels address one chunk of B with 32-bit byte offsets, and the smallest chunk is 64 rows, so for l > 64, 64 rows of B
 * may span at most 2^32 - 2^20 bytes (b_stride at most 8 386 560 words); for l <= 64 the l rows of B must span less than 2^32
 * bytes.  One row of A (a_stride words) may span at most 2^32 - 2^20 bytes, rows of A and C being cut one by one (m = 1: less
 * than 2^32 bytes).  n is at most INT32_MAX.  Within these limits any stride is legal: operands of 4 GiB and more -- windows of
 * a very wide parent included, in a batch as in a single call -- are cut into chunks, same bits. */
int m4ri_amd_mul_dev(word *C, int64_t c_stride, const word *A, int64_t a_stride, const word *B,
                     int64_t b_stride, int64_t m, int64_t l, int64_t n, int add, int cutoff,
                     void *stream);
/* One M4RM leaf launch, no Strassen (the device twin of _mzd_mul_m4rm).  ksplit: 0 = automatic. */
int m4ri_amd_m4rm_dev(word *C, int64_t c_stride, const word *A, int64_t a_stride, const word *B,
                      int64_t b_stride, int64_t m, int64_t l, int64_t n, int add, int ksplit,
                      void *stream);
/* `batch` products of one shape in ONE launch: C_b (+)= A_b * B_b, X_b = X + b * x_bs (word offsets).  Plain M4RM leaves
 * (no Strassen levels): for the many small equal products of a blocked algorithm. */
int m4ri_amd_m4rm_batch_dev(word *C, int64_t c_stride, int64_t c_bs, const word *A, int64_t a_stride, int64_t a_bs, const word *B,
                            int64_t b_stride, int64_t b_bs, int64_t m, int64_t l, int64_t n, int64_t batch, int add, void *stream);
/* `batch` independent products of one shape WITH the Strassen-Winograd levels of m4ri_amd_mul_dev, every pass and the leaf launch
 * shared by the whole batch (what the ranks of a sharded Strassen level use for the several sub-products each of them owns,
 * multi.hip; the sub-products of strassen.c:111-150 are independent).  Bit-identical to `batch` calls of m4ri_amd_mul_dev. */
int m4ri_amd_mul_batch_dev(word *C, int64_t c_stride, int64_t c_bs, const word *A, int64_t a_stride, int64_t a_bs, const word *B,
                           int64_t b_stride, int64_t b_bs, int64_t m, int64_t l, int64_t n, int64_t batch, int add, int cutoff, void *stream);
/* `batch` products of TINY matrices of one shape, C_b (+)= A_b * B_b (mul_small_batch.hip): A_b m x l, B_b l x n, C_b m x n, member b
 * at X + b * x_bs words, rows x_stride words apart.  The valid bits of every C_b are those of m4ri_amd_m4rm_batch_dev (mzd_mul /
 * mzd_addmul); bits of A at columns >= l and bits of B at columns >= n never influence a valid bit of C.  l = 0 clears the valid
 * bits of C_b (add == 0) or keeps them (add != 0); m = 0 or n = 0 touches nothing.  a_bs = 0 / b_bs = 0: one A / one B shared by
 * all members; A and B may overlap each other (A == B squares).  On paths 0 and 1 of m4ri_amd_plan_mul_small_batch, bits at
 * columns >= n of a row's last word, the words from the width to c_stride of a row, the words between members, A and B are never
 * written, and the call is asynchronous on `stream`: one launch (several for a batch beyond one grid), no allocation, no copy, no
 * engine workspace -- so no engine lock and no ordering behind the previous product; capturable.  Path 2 IS the launch of
 * m4ri_amd_m4rm_batch_dev, with its locking and its contract (whole last words of C included).  hipErrorInvalidValue, before any
 * HIP call, for negative sizes, strides or batch strides, a_stride < words(l), b_stride < words(n) or c_stride < words(n),
 * overlapping C members (batch > 1 and c_bs < (m - 1) * c_stride + words(n)), C overlapping A or B (the span from the first
 * member's start to the last member's end of each), or a NULL pointer with a non-empty member.  batch = 0 succeeds without
 * touching anything. */
int m4ri_amd_mul_small_batch_dev(word *C, int64_t c_stride, int64_t c_bs, const word *A, int64_t a_stride, int64_t a_bs, const word *B,
                                 int64_t b_stride, int64_t b_bs, int64_t m, int64_t l, int64_t n, int64_t batch, int add, void *stream);
/* which path m4ri_amd_mul_small_batch_dev takes for this (m, l, n) (pure host arithmetic; -1 for negative sizes): 0 one wave per
 * member, registers and cross-lane broadcasts only (m, l, n <= 64); 1 one wave per 64 x 64 block of C (max(m, l, n) <= the measured
 * bound D1, a multiple of 64 in [64, 256]; 64 = no such shape); 2 forwarded to m4ri_amd_m4rm_batch_dev.  The environment variable
 * M4RI_AMD_MUL_SMALL_BATCH_PATH1_MAX (read per call, clamped to [64, 256] in multiples of 64) replaces D1 in the routing of
 * m4ri_amd_mul_small_batch_dev; this function does not read it. */
int m4ri_amd_plan_mul_small_batch(int64_t m, int64_t l, int64_t n);
/* The same product with transposed operands, C_b (m x n) (+)= op(A_b) * op(B_b), op(A_b) m x l and op(B_b) l x n, in the same one
 * launch and without a scratch buffer: A A^T, A^T A, E H^T.  trans_a != 0: A_b is STORED l x m (a_stride >= words(m)) and
 * op(A_b) = A_b^T; trans_b != 0: B_b is STORED n x l (b_stride >= words(l)) and op(B_b) = B_b^T.  The kernels transpose each 64 x 64
 * block of a stored operand in registers on its way into the product.  Everything else is m4ri_amd_mul_small_batch_dev's: the
 * member addressing, a_bs = 0 / b_bs = 0 for one shared operand, A and B overlapping or the same pointer (A A^T with B == A and
 * trans_b, A^T A with trans_a), l = 0, m = 0, n = 0 and batch = 0.  Memory: only the valid bits of C are written -- bits at columns >= n
 * of a row's last word, the words from the width to c_stride of a row, the words between members, A and B never; bits of a STORED
 * operand beyond its own last column (m for a transposed A, l for a transposed B) never influence a valid bit of C; no word of a
 * stored operand outside its rows' widths is loaded.  Asynchronous on `stream`: one launch (several for a batch beyond one grid), no
 * allocation, no copy, no engine workspace, no engine lock; capturable.  hipErrorInvalidValue, before any HIP call, for the
 * conditions of m4ri_amd_mul_small_batch_dev with the widths and the row counts of the operands AS STORED: a_stride < words(m)
 * under trans_a, b_stride < words(l) under trans_b, C's span meeting the span of the l rows of a transposed A or of the n rows of a
 * transposed B.  With trans_a == trans_b == 0 the call IS m4ri_amd_mul_small_batch_dev, path 2 included.  With a transposed operand
 * there is no path 2: where m4ri_amd_plan_mul_small_batch_op says 2 (or the override of the routing makes it so) the call returns
 * hipErrorNotSupported before any HIP call and touches nothing.  Such a product is composed by the caller, who owns the scratch:
 * m4ri_amd_transpose_batch_dev of every transposed operand into a buffer of its own (D_b = A_b^T: l x m -> m x l; n x l -> l x n),
 * then m4ri_amd_m4rm_batch_dev (or m4ri_amd_mul_small_batch_dev) on the transposes, on the same stream. */
int m4ri_amd_mul_small_batch_op_dev(word *C, int64_t c_stride, int64_t c_bs, const word *A, int64_t a_stride, int64_t a_bs, const word *B,
                                    int64_t b_stride, int64_t b_bs, int64_t m, int64_t l, int64_t n, int64_t batch, int trans_a, int trans_b,
                                    int add, void *stream);
/* which path m4ri_amd_mul_small_batch_op_dev takes (pure host arithmetic; -1 for negative sizes).  trans_a == trans_b == 0:
 * m4ri_amd_plan_mul_small_batch's answer.  Otherwise 0 for m, l, n <= 64; 1 for max(m, l, n) <= D1op, the measured bound up to which
 * the fused call is not slower than transposing into scratch and multiplying (a multiple of 64 in [64, 256]; 64 = no such shape);
 * 2 = not supported.  M4RI_AMD_MUL_SMALL_BATCH_PATH1_MAX replaces D1op in the routing of the call as it replaces D1; this function
 * does not read it. */
int m4ri_amd_plan_mul_small_batch_op(int64_t m, int64_t l, int64_t n, int trans_a, int trans_b);
/* the time model's estimate for `batch` products m x l x n scheduled as one at `levels` levels (pure host arithmetic) */
double m4ri_amd_model_seconds_batch(int64_t m, int64_t l, int64_t n, int levels, int64_t batch);
/* C = A ^ B on rows x ncols bits: the device twin of _mzd_add (mzd.c:1471-1583).  In-place allowed,
 * operands may have different strides; the last word of every row is written under the column mask
 * and the other bits of C's last word are kept (mzd.c:1489). */
int m4ri_amd_xor_dev(word *C, int64_t c_stride, const word *A, int64_t a_stride, const word *B,
                     int64_t b_stride, int64_t rows, int64_t ncols, void *stream);
/* B (mb x nb, device) <- L^-1 B / U^-1 B in place, T (mb x mb, device) unit triangular -- the device twins of
 * _mzd_trsm_lower_left / _mzd_trsm_upper_left: halves recursion down to 512-row blocks solved through their inverses (64 rows
 * or fewer: one substitution kernel), every update one m4ri_amd_mul_dev on views; `cutoff` is handed to each of them and is a
 * hint (every value >= 0 gives the same bits).
 * Memory: of T only the bits strictly inside its triangle are read (diagonal, other triangle and the words from words(mb) to
 * t_stride never); T is never written.  Above 64 rows the caller keeps T's bits at column >= mb zero (its blocks go to the
 * multiply engine as operands); up to 64 rows they are not read.  Of B the rows 0 .. mb-1, words 0 .. words(nb)-1 are read and
 * written.  Bits of B at column >= nb: above 64 rows zero in, zero out (the last word is written whole); up to 64 rows they are
 * kept, whatever they are.  The words from words(nb) to b_stride of a row and the rows before and after B are never written.
 * T and B must not overlap.  Any word alignment and any stride >= the width, odd ones included.
 * Asynchronous on `stream`; above 64 rows the calls share grow-only scratch per device (growing it synchronises the device)
 * and a solve on another stream than the previous one first waits, on the device, for that one.  hipErrorInvalidValue, before
 * any HIP call, for mb < 0, nb < 0 or cutoff < 0. */
int m4ri_amd_trsm_lower_left_dev(const word *L, int64_t t_stride, word *B, int64_t b_stride, int64_t mb, int64_t nb, int cutoff,
                                 void *stream);
int m4ri_amd_trsm_upper_left_dev(const word *U, int64_t t_stride, word *B, int64_t b_stride, int64_t mb, int64_t nb, int cutoff,
                                 void *stream);
/* B (mb x nb) <- B U^-1 / B L^-1, T (nb x nb, device) unit triangular: the right-hand twins (64 columns or fewer: one kernel,
 * a thread per row of B).  The same memory rules with T nb x nb and the threshold at 64 columns: T's proper triangle only is
 * read, never written, its bits at column >= nb zero above 64 columns and not read up to 64; rows 0 .. mb-1, words 0 ..
 * words(nb)-1 of B read and written, bits of B at column >= nb zero in, zero out above 64 columns and kept whatever they are up
 * to 64; padding words and neighbouring rows never written; asynchronous on `stream` with the same shared scratch above 64
 * columns; hipErrorInvalidValue, before any HIP call, for mb < 0, nb < 0 or cutoff < 0. */
int m4ri_amd_trsm_upper_right_dev(const word *U, int64_t t_stride, word *B, int64_t b_stride, int64_t mb, int64_t nb, int cutoff,
                                  void *stream);
int m4ri_amd_trsm_lower_right_dev(const word *L, int64_t t_stride, word *B, int64_t b_stride, int64_t mb, int64_t nb, int cutoff,
                                  void *stream);
/* Device twin of mzd_process_rowsN (elim.hip): streaming, HBM-bound.  kbits[t]: bits of group t (lowest first); L[t]:
 * 2^kbits[t] table row numbers; idx_scratch: 6 * (stoprow - startrow) int32.  kbits, T, t_stride and L are HOST arrays of
 * `ntables` entries (T[t], L[t] and idx_scratch device pointers).  Reads the strip of every row of [startrow, stoprow) and the
 * words startcol/64 .. width-1 of the table rows it selects; XORs whole words onto the words startcol/64 .. width-1 of those
 * rows of M (the last word included: a table row with a clean tail leaves M's tail as it was) and writes nothing else -- not
 * the words before startcol/64, not the words from `width` to `stride`, no other row, no table.  16-byte accesses are used when
 * M and every table allow them (16-byte aligned bases, even strides, startcol/64 and width - startcol/64 even), single words
 * otherwise: any alignment is legal.  Asynchronous on `stream`.  hipErrorInvalidValue, before any HIP call, for ntables
 * outside 1 .. 6, startrow < 0, stoprow < startrow or startcol < 0. */
int m4ri_amd_process_rows_dev(word *M, int64_t stride, int64_t width, int64_t startrow, int64_t stoprow, int64_t startcol, int ntables,
                              const int32_t *kbits, const word *const *T, const int64_t *t_stride, const int32_t *const *L,
                              int32_t *idx_scratch, void *stream);
/* Device twin of mzd_make_table (elim.hip).  jstar: 2^k int32 on the device, see elim.hip (all zeros when rows r .. r+k-1
 * exist).  Reads rows r .. r+k-1 of M below m_rows (never written) and Tin; writes rows 1 .. 2^k - 1 of Tout, words c/64 ..
 * words(ncols)-1: the first of them masked below column c, the last to ncols columns (tail written zero); a row whose source
 * row does not exist is copied from Tin, tail included (Tin == Tout: it stays).  Tin and Tout have the stride t_stride; Tin is
 * not written unless it is Tout.  Row 0, the words before c/64 and the words from words(ncols) to t_stride of Tout are never
 * written.  Asynchronous on `stream`.  hipErrorInvalidValue, before any HIP call, for k outside 1 .. 16 or ncols <= 0. */
int m4ri_amd_make_table_dev(const word *M, int64_t m_stride, int64_t m_rows, int64_t ncols, int64_t r, int64_t c, int k, const word *Tin,
                            word *Tout, int64_t t_stride, const int32_t *jstar, void *stream);
/* PLE of a device matrix in place (bits at column >= ncols zero in, zero out).  P (nrows entries) and Q (ncols
 * entries) are HOST arrays.  Blocking: the pivots of every 64-column block are read back.
 * recursion_cutoff: 0 gives _mzd_ple_russian's Q (the pivot columns, then the identity); M4RI_AMD_PLE_CUTOFF gives
 * _mzd_ple's, whose recursion on column halves (m4ri/ple.c:62-171) leaves other transpositions behind the rank --
 * which ones depends on the recursion's shape, i.e. on __M4RI_PLE_CUTOFF of the reference build (m4ri/ple.h:40:
 * 524288 words for any L3 cache of 4 MiB or more).  Matrix, P, rank and pivots are the same either way. */
#define M4RI_AMD_PLE_CUTOFF 524288
int m4ri_amd_ple_dev(word *A, int64_t stride, int64_t nrows, int64_t ncols, int32_t *P, int32_t *Q, int32_t *rank_out,
                     int64_t recursion_cutoff, void *stream);
/* PLUQ in place (m4ri/ple.c:50-60): the PLE, then the column step below on the first `rank` rows.  Blocking. */
int m4ri_amd_pluq_dev(word *A, int64_t stride, int64_t nrows, int64_t ncols, int32_t *P, int32_t *Q, int32_t *rank_out,
                      int64_t recursion_cutoff, void *stream);
/* Device twins of the drivers over PLUQ (solve.hip); P, Q: HOST arrays; *retval: 0 / -1 as mzd_solve_left.  Blocking: on
 * return the work is complete and `stream` idle.  Memory rules common to the five functions below: every matrix keeps the Part
 * 2 invariant (bits beyond its last column zero in, zero out); of a matrix that is written, only its own rows and the words
 * below its width are -- the words from the width to the stride of a row and the rows before and after it never; any word
 * alignment, any stride >= width. */
/* The row transpositions (i, P[i]), i < min(length, nrows), ascending (trans == 0) or descending: whole rows of words(ncols)
 * words move, each with its own tail bits.  hipErrorInvalidValue, before any HIP call, for negative sizes, P == NULL or an
 * entry of P outside the rows. */
int m4ri_amd_apply_p_left_dev(word *A, int64_t stride, int64_t nrows, int64_t ncols, const int32_t *P, int64_t length, int trans, void *stream);
/* A (m x n, its PLUQ), rank, P, Q are read only; B (b_rows x b_cols, b_rows >= max(m, n)) <- the solution, as
 * _mzd_pluq_solve_left leaves it: also on *retval == -1 (inconsistency_check != 0 and no solution), where B holds the
 * reference's state at that point (solve.c:81-121), not its input.  hipErrorInvalidValue, before any HIP call, for negative
 * sizes, a NULL P, Q or retval, rank > min(m, n), b_rows < max(m, n) or cutoff < 0. */
int m4ri_amd_pluq_solve_left_dev(const word *A, int64_t a_stride, int64_t m, int64_t n, int32_t rank, const int32_t *P, const int32_t *Q, word *B,
                                 int64_t b_stride, int64_t b_rows, int64_t b_cols, int cutoff, int inconsistency_check, int *retval, void *stream);
/* A <- its PLUQ, then the above.  With inconsistency_check != 0 and b_rows > m, a set bit in the rows m+1 .. b_rows-1 of B
 * gives *retval = -1 before anything is computed: A and B are then untouched, byte for byte.  hipErrorInvalidValue, before any
 * HIP call, for negative sizes, retval == NULL, b_rows < max(m, n) or cutoff < 0. */
int m4ri_amd_solve_left_dev(word *A, int64_t a_stride, int64_t m, int64_t n, word *B, int64_t b_stride, int64_t b_rows, int64_t b_cols, int cutoff,
                            int inconsistency_check, int *retval, void *stream);
/* A <- its PLUQ; R (n x (n - rank), its valid words ZERO on entry) <- the basis, whole words of its rows written; rank == n: R
 * is not touched.  hipErrorInvalidValue, before any HIP call, for negative sizes, rank_out == NULL or cutoff < 0. */
int m4ri_amd_kernel_left_pluq_dev(word *A, int64_t a_stride, int64_t m, int64_t n, word *R, int64_t r_stride, int cutoff, int32_t *rank_out,
                                  void *stream);
/* A is read only (bits beyond column n zero); the n x words(n) words of Binv are written whole, whatever they held, the bits
 * beyond column n zero.  Binv must not overlap A.  hipErrorInvalidValue, before any HIP call, for n < 0. */
int m4ri_amd_inv_dev(word *Binv, int64_t b_stride, const word *A, int64_t a_stride, int64_t n, void *stream);
/* Device twin of mzd_transpose: D (ncols x nrows) <- A^T, D must not overlap A; one HBM-bound launch (A read once, D written
 * once, whole 128-byte lines on both sides); asynchronous. */
int m4ri_amd_transpose_dev(word *D, int64_t d_stride, const word *A, int64_t a_stride, int64_t nrows, int64_t ncols, void *stream);
/* `batch` transposes of SMALL matrices of one shape, D_b <- (A_b)^T (transpose_batch.hip): A_b nrows x ncols at A + b * a_bs words,
 * rows a_stride words apart; D_b ncols x nrows at D + b * d_bs words, rows d_stride words apart.  The valid bits of D_b become the
 * transpose; bits of A at columns >= ncols of a row's last word never influence a valid bit of D.  A is never written.  On paths 0
 * and 1 of m4ri_amd_plan_transpose_batch, bits at columns >= nrows of a row's last word of D, the words from the width to d_stride
 * of a row and the words between members are left as they were; on path 2 (m4ri_amd_transpose_dev's kernel and contract, the member
 * a grid dimension) the last word of a row of D is written whole, the bits beyond column nrows zero, and padding words and gaps are
 * left alone.  Every path is asynchronous on `stream`: plain launches (several for a batch beyond one grid), no allocation, no copy,
 * no engine workspace, no engine lock; capturable.  nrows = 0, ncols = 0 or batch = 0 succeeds without touching anything.
 * In place: D == A is allowed exactly when nrows == ncols <= 1024, d_stride == a_stride and d_bs == a_bs; such a call always runs
 * in registers (a wave per member up to 64, a wave per pair of mirrored 64 x 64 blocks above), whatever the bound below or its
 * override; D == A with members of any other shape is refused whatever the batch.  hipErrorInvalidValue, before any HIP call, for negative sizes, strides or batch strides, a_stride < words(ncols),
 * d_stride < words(nrows), overlapping D members (batch > 1 and d_bs < (ncols - 1) * d_stride + words(nrows)), D overlapping A (the
 * span from the first member's start to the last member's end of each) in any but the in-place case, or a NULL pointer with a
 * non-empty member.  a_bs is otherwise free: A is only read, a_bs = 0 transposes one A into every D_b. */
int m4ri_amd_transpose_batch_dev(word *D, int64_t d_stride, int64_t d_bs, const word *A, int64_t a_stride, int64_t a_bs, int64_t nrows,
                                 int64_t ncols, int64_t batch, void *stream);
/* which path an out-of-place m4ri_amd_transpose_batch_dev takes for this shape (pure host arithmetic; -1 for negative sizes): 0 one
 * wave per member, registers only (nrows, ncols <= 64); 1 one wave per 64 x 64 block (max(nrows, ncols) <= the measured bound T1, a
 * multiple of 64 in [64, 1024]; 64 = no such shape); 2 the tile kernel of m4ri_amd_transpose_dev.  The environment variable
 * M4RI_AMD_TRANSPOSE_BATCH_PATH1_MAX (read per call, clamped to [64, 1024] in multiples of 64) replaces T1 in the routing of
 * out-of-place calls; this function does not read it. */
int m4ri_amd_plan_transpose_batch(int64_t nrows, int64_t ncols);
/* The read side of the batched calls (reduce_batch.hip): what a caller wants to know about `batch` matrices of one shape without
 * downloading them.  Conventions of the three calls below: member b of X is the nrows x ncols matrix at X + b * x_bs words, rows
 * x_stride words apart; x_bs = 0 is one operand shared by all members.  Only the valid bits count: bits at columns >= ncols of a
 * row's last word, the words from the width to the stride and the words between members are never looked at.  The operands are
 * READ ONLY; every result array is DEVICE memory and is written whole, whatever it held.  Asynchronous on `stream` on every path of
 * m4ri_amd_plan_reduce_batch: plain launches (on path 2 an initialisation of the outputs goes first, on the same stream), no
 * allocation, no copy to the host, no synchronisation, no engine workspace, no engine lock; capturable.  All results are integer
 * sums, minima and maxima: they do not depend on the order the hardware takes the rows in.
 * hipErrorInvalidValue, before any HIP call, for negative sizes, strides or batch strides, nrows or ncols > INT32_MAX, a stride below
 * words(ncols) or a NULL operand with non-empty members (the latter with batch > 0), no output at all, or an output array whose
 * bytes meet the span (first member's start to last member's end) of an operand.  batch = 0 succeeds without touching anything.
 * Empty members (nrows = 0 or ncols = 0) need no operand pointers; their results are still written: weights 0, lightest -1
 * (nrows = 0) or 0 (ncols = 0 < nrows), first_row -1, first_nonzero = nrows, end_nonzero = 0. */
/* Hamming weights of A_b (B == NULL; b_stride, b_bs ignored but not negative) or of A_b ^ B_b, the distance, which is never
 * written anywhere.  total[b] (int64, batch entries): the member's weight.  row_weight[b * nrows + i] (int32): the weight of row i.
 * lightest[b] (int64): (the smallest row weight << 32) | the index of the first row that has it; -1 for nrows = 0.  Each of the three
 * may be NULL, not all.  A == B is allowed (zeros). */
int m4ri_amd_weight_batch_dev(const word *A, int64_t a_stride, int64_t a_bs, const word *B, int64_t b_stride, int64_t b_bs, int64_t nrows,
                              int64_t ncols, int64_t batch, int64_t *total, int32_t *row_weight, int64_t *lightest, void *stream);
/* first_row[b] (int32, batch entries, required): the smallest i at which rows i of A_b and B_b differ in a valid bit, -1 if there
 * is none: -1 <=> mzd_equal (m4ri/mzd.c:1314).  Both operands are required. */
int m4ri_amd_mismatch_batch_dev(const word *A, int64_t a_stride, int64_t a_bs, const word *B, int64_t b_stride, int64_t b_bs, int64_t nrows,
                                int64_t ncols, int64_t batch, int32_t *first_row, void *stream);
/* first_nonzero[b] (int32): the first row of A_b with a set bit, nrows if there is none.  end_nonzero[b] (int32): one past the last
 * such row, which is mzd_first_zero_row (m4ri/mzd.c:1826); 0 <=> mzd_is_zero (:1629).  Either may be NULL, not both. */
int m4ri_amd_row_span_batch_dev(const word *A, int64_t a_stride, int64_t a_bs, int64_t nrows, int64_t ncols, int64_t batch,
                                int32_t *first_nonzero, int32_t *end_nonzero, void *stream);
/* which path the three calls above take for members of this shape (pure host arithmetic; -1 for negative sizes): 0 one wave per
 * member, a row per lane, registers only (nrows <= 64 and at most W0 words per row; empty members count here); 1 one workgroup
 * per member, reduced through LDS (nrows * words(ncols) <= T1); 2 a member's rows cut into chunks, a workgroup per chunk, the
 * per-member results combined with global atomics.  W0 and T1 are measured bounds.  The environment variables
 * M4RI_AMD_REDUCE_BATCH_PATH0_MAX (words per row, clamped to [0, 16]; 0 = no path 0) and M4RI_AMD_REDUCE_BATCH_PATH1_MAX (words per
 * member, clamped to [0, 2^30]; 0 = no path 1) replace them in the routing of a call, read per call; this function does not read
 * them. */
int m4ri_amd_plan_reduce_batch(int64_t nrows, int64_t ncols);
/* Weight distributions and minimum weights of the ROW SPACES of `batch` small matrices (rowspace_batch.hip): the table of
 * mzd_make_table, all 2^k combinations of k rows in Gray order, with a population count in place of the store; nothing of size 2^k
 * is ever written.  Member b has the generator G_b, k x n at G + b * g_bs words, rows g_stride words apart (g_bs = 0: one shared G),
 * and an optional word V_b, 1 x n at V + b * v_bs words (V == NULL: zero; v_bs = 0: one shared V).  For every message x in
 * [0, 2^k) the word is c_b(x) = V_b ^ the XOR of the rows i of G_b with bit i of x set.  Only the n valid bits count: bits at
 * columns >= n of a last word, the words from the width to the stride and the words between members never influence a result; G and
 * V are READ ONLY.
 * hist (DEVICE int64, batch * (n + 1) entries, or NULL): hist[b * (n + 1) + w] = the number of x with wt(c_b(x)) = w.  MESSAGES are
 * counted, not distinct words: every member's entries sum to 2^k, and a G of rank r counts every word of its span 2^(k - r) times.
 * lightest (DEVICE int64, batch entries, or NULL): lightest[b] = the minimum over the x with wt(c_b(x)) >= w_min of (wt << 40) | x,
 * -1 if no x qualifies; among equal weights the smallest x.  w_min = 1 without V: the minimum distance of the code and the smallest
 * message that attains it, whatever G's rank.  w_min = 0 with V: the distance from V_b to the code and the message of the nearest
 * codeword.  At least one of the two outputs is required; both are written whole, whatever they held.
 * Limits: 0 <= k <= 40 (the message fits the key) and 0 <= n <= 1024 (a word fits 32 registers per lane); beyond either the call
 * returns hipErrorNotSupported (801) before any HIP call.  k = 0 is the one message 0 with c = V; n = 0: every word weighs 0.
 * Asynchronous on `stream` on both paths of m4ri_amd_plan_rowspace_weights_batch: plain launches (on path 1 an initialisation of the
 * outputs goes first, on the same stream), no allocation, no copy to the host, no synchronisation, no engine workspace, no engine
 * lock; capturable.  All results are integer counts and minima: they do not depend on the order the hardware takes the messages in.
 * hipErrorInvalidValue, before any HIP call, for negative sizes, strides or batch strides or w_min < 0, g_stride < words(n) with
 * k > 1, a NULL G with non-empty members (batch > 0, k > 0, n > 0), no output at all, or an output array whose bytes meet the span
 * (first member's start to last member's end) of G, of V or the other output.  batch = 0 succeeds without touching anything.
 * For k > 40 see m4ri_amd_row_sums_weights_batch_dev below: the sums of exactly t rows instead of the whole span. */
int m4ri_amd_rowspace_weights_batch_dev(const word *G, int64_t g_stride, int64_t g_bs, int64_t k, int64_t n, const word *V, int64_t v_bs,
                                        int64_t batch, int64_t w_min, int64_t *hist, int64_t *lightest, void *stream);
/* which path the call above takes for members of this shape (pure host arithmetic; -1 for negative sizes; sizes beyond the call's
 * limits are answered by the same rule): 0 a wave owns the member, four members per workgroup, plain stores, no global atomics
 * (k <= K0, or n = 0); 1 the member's messages are spread over 2^(k - s - 6) waves of s-bit Gray walks, s = k - 19 held in [6, 12],
 * their results combined with global 64-bit integer atomics.  K0 is a measured bound.  The environment variable
 * M4RI_AMD_ROWSPACE_PATH0_MAX (clamped to [-1, 26]; -1 = no path 0 for members with columns) replaces it in the routing of a call,
 * read per call; this function does not read it. */
int m4ri_amd_plan_rowspace_weights_batch(int64_t k, int64_t n);
/* The weights of all sums of exactly t ROWS of `batch` small matrices (rowsums_batch.hip): the enumeration of Brouwer-Zimmermann
 * minimum-distance bounds, of Lee-Brickell and Stern information-set decoding and of "any light combination of few rows?" filters,
 * for generators far beyond the k = 40 of the call above.  The operands are those of that call: member b has G_b, k x n at
 * G + b * g_bs words, rows g_stride words apart (g_bs = 0: one shared G), and an optional word V_b, 1 x n at V + b * v_bs words
 * (V == NULL: zero; v_bs = 0: one shared V); only the n valid bits count, G and V are READ ONLY.  For every set
 * S = {i_0 < i_1 < ... < i_{t-1}} of t row indices below k the word is c_b(S) = V_b ^ the rows of G_b in S, and the rank of S its
 * colexicographic rank r(S) = sum_j C(i_j, j + 1), 0 .. C(k, t) - 1.  t = 0 is the one sum c = V with rank 0; k < t: no sums.
 * hist (DEVICE int64, batch * (n + 1) entries, or NULL): hist[b * (n + 1) + w] = the number of S with wt(c_b(S)) = w.  SETS are
 * counted, not distinct words: every member's entries sum to C(k, t).
 * lightest (DEVICE int64, batch entries, or NULL): lightest[b] = the minimum over the S with wt(c_b(S)) >= w_min of
 * (wt << 40) | r(S), -1 if no S qualifies; among equal weights the smallest rank.  At least one of the two outputs is required; both
 * are written whole, whatever they held.  Members without columns (n = 0) have hist[0] = C(k, t) and lightest 0 if w_min = 0 and
 * there is a sum, otherwise -1; members without sums have every bin 0 and lightest -1.
 * Limits: 0 <= k <= 1024, 0 <= n <= 1024, 0 <= t <= 8 and C(k, t) <= 2^40 (the rank fits the key: C(1024, 4) does, C(1024, 5) does
 * not); beyond any of them the call returns hipErrorNotSupported (801) before any HIP call.
 * Asynchronous on `stream` on both paths of m4ri_amd_plan_row_sums_weights_batch: plain launches (on path 1 an initialisation of the
 * outputs goes first, on the same stream), no allocation, no copy to the host, no synchronisation, no engine workspace, no engine
 * lock; capturable.  All results are integer counts and minima: they do not depend on the order the hardware takes the sums in.
 * hipErrorInvalidValue, before any HIP call, for negative sizes, strides or batch strides, t < 0 or w_min < 0, g_stride < words(n)
 * with k > 1, a NULL G with non-empty members that have sums (batch > 0, k >= t >= 1, n > 0), no output at all, or an output array
 * whose bytes meet the span (first member's start to last member's end) of G, of V or the other output.  batch = 0 succeeds without
 * touching anything. */
int m4ri_amd_row_sums_weights_batch_dev(const word *G, int64_t g_stride, int64_t g_bs, int64_t k, int64_t n, const word *V, int64_t v_bs,
                                        int64_t batch, int64_t t, int64_t w_min, int64_t *hist, int64_t *lightest, void *stream);
/* which path the call above takes for members of this shape (pure host arithmetic; -1 for negative sizes; sizes beyond the call's
 * limits are answered by the same rule): 0 a wave walks all sums of its member, four members per workgroup, plain stores, no global
 * atomics (C(k, t) <= M0; members without columns or sums, and t = 0, count here: an initialisation kernel answers them); 1 a
 * member's sums are spread over waves, 64 upper parts {i_1 .. i_{t-1}} by a segment of i_0 each, their results combined with global
 * 64-bit integer atomics after an initialisation kernel.  M0 is a number of sums per member.  The environment variable
 * M4RI_AMD_ROW_SUMS_PATH0_MAX (clamped to [-1, 2^24]; -1 = no path 0 for members with columns and sums) replaces it in the routing
 * of a call, read per call; this function does not read it. */
int m4ri_amd_plan_row_sums_weights_batch(int64_t k, int64_t n, int64_t t);
/* The collision step of Stern's / Dumer's information-set decoding on `batch` small matrices (rowsums_collide_batch.hip): of the
 * pairs (t1 rows of one half, t2 rows of the other) only those whose sum vanishes on a window of ell chosen columns are weighed.
 * G, V, the stride and batch strides, sharing with a batch stride of 0, "only the n valid bits count" and READ ONLY are those of
 * m4ri_amd_row_sums_weights_batch_dev above.  Rows 0 .. k1-1 of a member are its LEFT rows, rows k1 .. k-1 its RIGHT rows,
 * k2 = k - k1.  S1 is a set of t1 left rows, r1 its colexicographic rank; S2 a set of t2 right rows, r2 the colexicographic rank
 * of {i - k1 : i in S2}; N1 = C(k1, t1), N2 = C(k2, t2), the empty set the one set of rank 0.  The word of the pair is
 * c_b(S1, S2) = V_b ^ the rows of G_b in S1 ^ those in S2.
 * cols (DEVICE int32, or NULL): member b's window, ell column indices at cols + b * c_bs entries (c_bs = 0: one window for all
 * members; NULL: the columns 0 .. ell-1); the entries need not be sorted, distinct or adjacent.  The pair COLLIDES iff c is 0 at
 * every window column; with ell = 0 every pair collides.
 * hist (DEVICE int64, batch * (n + 1) entries, or NULL): hist[b * (n + 1) + w] = the number of colliding pairs with wt(c) = w, the
 * weight over all n columns: a member's entries sum to its number of collisions.
 * lightest (DEVICE int64, batch entries, or NULL): lightest[b] = the minimum over the colliding pairs with wt(c) >= w_min of
 * (wt << 40) | (r1 * N2 + r2), -1 if there is none.  At least one of the two outputs is required; both are written whole.
 * A window entry outside 0 .. n-1 cannot be seen by the host, so the device decides: that member is REFUSED, every one of its hist
 * entries is -1 and its lightest -2, whatever pairs it has; nothing outside the member is read, the other members are unaffected.
 * Members without pairs (N1 = 0 or N2 = 0: t1 > k1 or t2 > k2) have every bin 0 and lightest -1; n = 0 with ell = 0 puts all
 * N1 * N2 pairs into bin 0 (lightest 0 if w_min = 0 and there is a pair); batch = 0 succeeds without touching anything.
 * Limits: k <= 1024, n <= 1024, t1, t2 <= 8, ell <= 64, N1 * N2 <= 2^40 (the pair rank fits the key) and N1 <= 8192 (the left list
 * is tabled in one workgroup's LDS: C(128, 2) = 8128 fits, C(129, 2) = 8256 does not); beyond any of them the call returns
 * hipErrorNotSupported (801) before any HIP call.  Every workgroup tables the left list and walks the right one: THE HALF WITH FEWER
 * SUMS BELONGS FIRST.
 * Asynchronous on `stream` on both paths of m4ri_amd_plan_row_sums_collide_batch: plain launches (on path 1 an initialisation of the
 * outputs goes first, on the same stream), no allocation, no copy to the host, no synchronisation, no engine workspace, no engine
 * lock; capturable.  All results are integer counts and minima: they do not depend on the order the hardware takes the pairs in.
 * hipErrorInvalidValue, before any HIP call, for negative sizes, strides or batch strides, k1 > k, t1, t2, ell or w_min < 0, a NULL
 * cols with ell > n, g_stride < words(n) with k > 1, a NULL G where rows are read (batch > 0, n > 0, pairs, t1 + t2 >= 1), no output
 * at all, or an output array whose bytes meet the span (first member's start to last member's end) of G, of V, of cols or the other
 * output. */
int m4ri_amd_row_sums_collide_batch_dev(const word *G, int64_t g_stride, int64_t g_bs, int64_t k, int64_t n, const word *V, int64_t v_bs,
                                        int64_t batch, int64_t k1, int64_t t1, int64_t t2, const int32_t *cols, int64_t c_bs, int64_t ell,
                                        int64_t w_min, int64_t *hist, int64_t *lightest, void *stream);
/* which path the call above takes for members of this shape (pure host arithmetic; -1 for negative sizes or k1 > k; sizes beyond the
 * call's limits are answered by the same rule): 0 one workgroup takes the member's whole right list and writes its outputs with
 * plain stores, no global atomics (N1 * N2 <= P0; members without pairs or columns count here: an initialisation kernel answers
 * them); 1 the right list is cut into slices, a workgroup each, every one with its own left table, their results combined with
 * global 64-bit integer atomics after an initialisation kernel.  P0 is a number of pairs per member.  The environment variable
 * M4RI_AMD_ROW_SUMS_COLLIDE_PATH0_MAX (clamped to [-1, 2^32 - 1]; -1 = no path 0 for members with columns and pairs) replaces it in
 * the routing of a call, read per call; this function does not read it. */
int m4ri_amd_plan_row_sums_collide_batch(int64_t k, int64_t n, int64_t k1, int64_t t1, int64_t t2, int64_t ell);
/* the workgroups per member of the call above on path 1, whichever path the shape is routed to: the right list in slices of at least
 * max(N1, 256) sums, as many as bring the call to 1024 workgroups, a slice times N1 below 2^32.  0 for members without pairs or
 * columns or with N1 > 8192, -1 for negative sizes. */
int64_t m4ri_amd_row_sums_collide_slices(int64_t k, int64_t n, int64_t k1, int64_t t1, int64_t t2, int64_t ell, int64_t batch);
/* m4ri_amd_row_sums_collide_batch_dev with a LIST of the light colliding pairs beside its two outputs.  Every name, stride, sharing
 * rule (a batch stride of 0), "only the n valid bits count", READ ONLY, the limits, the ranks, the window, the refused members, the
 * paths, the slices and the routing variable are those of that call; hist and lightest (each may be NULL) mean what they mean there,
 * and lightest ignores w_max.  A colliding pair QUALIFIES iff w_min <= wt(c) <= w_max; a w_max above n is n.
 * count (DEVICE int64, batch entries): count[b] = the number of qualifying pairs of member b, the TRUE total however small cap is, so
 * that the caller sees an overflow and can come back with a larger list.  With hist given it is the sum of hist over w_min .. w_max.
 * list (DEVICE int64, member b's entries at list + b * l_bs, cap of them): the entries i < min(count[b], cap) are DISTINCT keys
 * (wt << 40) | (r1 * N2 + r2) of qualifying pairs, in no particular order.  count[b] <= cap: they are all of them.  count[b] > cap:
 * some cap of them; which ones is not specified and may differ from run to run.  The entries from min(count[b], cap) on are NOT
 * written.  m4ri_amd_row_sums_words_batch_dev below turns the keys into words.  ell = 0, t2 = 0, k1 = k lists the sums of
 * m4ri_amd_row_sums_weights_batch_dev in a weight band.
 * list and count come together; list may be NULL only with cap = 0, and then count alone is a filtered count.  At least one of hist,
 * lightest and count is required.
 * A REFUSED member has count -1 and no list entry written (hist and lightest in their refused forms); a member without pairs count 0;
 * n = 0 with ell = 0: count = N1 * N2 if w_min = 0, else 0, and the first min(count, cap) entries are the keys 0, 1, ... (weight 0,
 * the pair ranks in order); batch = 0 succeeds without touching anything.
 * Asynchronous on `stream` and capturable on both paths, as the call above: no allocation, no copy to the host, no synchronisation,
 * no engine lock.  Path 0 takes the slots from a counter in the workgroup's LDS and writes count[b] once, with a plain store: no
 * global atomic.  Path 1 sets count in its initialisation kernel and takes every slot with one returning 64-bit global atomic add,
 * which bounds the rate where nearly every pair qualifies; the call is meant for ell >= log2 N1 and a w_max at the
 * target weight, where a member lists a handful of keys.
 * hipErrorInvalidValue, before any HIP call, for whatever the call above refuses, a negative w_max, cap or l_bs, l_bs < cap with
 * batch > 1 (count given), a list without a count, a count without a list at cap > 0, none of the three outputs, or an output (hist,
 * lightest, count, the list's span from its first member's start to the last member's cap-th entry) whose bytes meet another output
 * or the span of G, of V or of cols.  hipErrorNotSupported as above.  cap is otherwise unbounded; the indexing is 64-bit. */
int m4ri_amd_row_sums_collide_list_batch_dev(const word *G, int64_t g_stride, int64_t g_bs, int64_t k, int64_t n, const word *V, int64_t v_bs,
                                             int64_t batch, int64_t k1, int64_t t1, int64_t t2, const int32_t *cols, int64_t c_bs, int64_t ell,
                                             int64_t w_min, int64_t w_max, int64_t *hist, int64_t *lightest, int64_t *list, int64_t l_bs,
                                             int64_t cap, int64_t *count, void *stream);
/* The words behind listed keys, on the device (rowsums_words_batch.hip).  G, V, k, n, k1, t1, t2, the strides and the ranks are those
 * of m4ri_amd_row_sums_collide_batch_dev; t2 = 0, k1 = k serves the keys of m4ri_amd_row_sums_weights_batch_dev, which are ranks of
 * t-sets.  keys (DEVICE int64): member b's at keys + b * l_bs entries.  count (DEVICE int64, batch entries, or NULL): member b has
 * m_b = min(max(count[b], 0), cap) keys, so a refused member's -1 reads as 0 and a count beyond cap as cap; NULL: cap keys per member.
 * W: member b's rows at W + b * w_bs words, w_stride words apart.  For i < m_b let r = keys[b * l_bs + i] & (2^40 - 1): the weight
 * bits above are ignored.  Row i of W_b becomes V_b ^ rows S1 ^ rows S2 of the pair of rank r = r1 * N2 + r2.  Only the n valid bits
 * are written: bits at columns >= n, padding words, the rows from m_b on and the gaps keep what they held.
 * A key cannot be seen by the host, so the device decides: if keys[...] < 0 or r >= N1 * N2 the row is SKIPPED, it is not written and
 * no row index is formed from the key.  skipped (DEVICE int32, batch entries, or NULL): skipped[b] = the number of such rows, written
 * whole, 0 for a clean member.
 * Limits: k, n <= 1024, t1, t2 <= 8, N1 * N2 <= 2^40; there is no bound on N1, nothing is tabled.  Beyond them hipErrorNotSupported
 * (801) before any HIP call.
 * Asynchronous on `stream`: a memset of skipped and plain launches, no allocation, no copy to the host, no synchronisation, no engine
 * lock; capturable.  count and keys are read on the device, so they may come from a call still in flight on the same stream.
 * hipErrorInvalidValue, before any HIP call, for negative sizes, strides or batch strides, k1 > k, g_stride < words(n) with k > 1,
 * w_stride < words(n) with cap > 1, with batch > 1 and cap > 0 an l_bs < cap or a w_bs below (cap - 1) * w_stride + words(n), a NULL
 * keys, W (n > 0) or G (where rows are read) with batch > 0 and cap > 0, or a W or skipped whose bytes meet the span of G, V, keys,
 * count or each other.  batch = 0 succeeds without touching anything; cap = 0 writes skipped only. */
int m4ri_amd_row_sums_words_batch_dev(const word *G, int64_t g_stride, int64_t g_bs, int64_t k, int64_t n, const word *V, int64_t v_bs,
                                      int64_t batch, int64_t k1, int64_t t1, int64_t t2, const int64_t *keys, int64_t l_bs, int64_t cap,
                                      const int64_t *count, word *W, int64_t w_stride, int64_t w_bs, int32_t *skipped, void *stream);
/* The join of two EXPLICIT lists of words on a window of bits (lists_collide_batch.hip): the merge step that Stern's collision search,
 * Wagner's generalized birthday and the level-1 lists of MMT / BJMM share, for lists that are rows in memory and of any length -- the
 * output of an earlier join among them.  Member b has a LEFT list X_b, nx rows of n bits at X + b * x_bs words, the rows x_stride
 * words apart; a RIGHT list Y_b, ny rows, y_stride, y_bs; an optional word V_b at V + b * v_bs (V = NULL: none).  A batch stride of 0 is
 * one operand shared by all members.  X, Y and V are READ ONLY and only their n valid bits count; X and Y may be the same memory or
 * overlap (a self-join, the pairs i = j included).  The word of pair (i, j) is c_b(i, j) = V_b ^ X_b[i] ^ Y_b[j], its rank i * ny + j.
 * cols (DEVICE int32, or NULL): member b's window, ell column indices at cols + b * c_bs entries (c_bs = 0: one window for all
 * members; NULL: the columns 0 .. ell-1, one masked word per row); the entries need not be sorted, distinct or in one word.  The pair
 * COLLIDES iff c is 0 at every window column; with ell = 0 every pair collides.
 * The outputs are those of m4ri_amd_row_sums_collide_list_batch_dev with this pair rank in the key's low 40 bits:
 * hist (DEVICE int64, batch * (n + 1) entries, or NULL): hist[b * (n + 1) + w] = the number of colliding pairs with wt(c) = w.
 * lightest (DEVICE int64, batch entries, or NULL): the minimum over the colliding pairs with wt(c) >= w_min of (wt << 40) | rank, -1 if
 * there is none; it ignores w_max.
 * count (DEVICE int64, batch entries, or NULL): the number of colliding pairs with w_min <= wt(c) <= w_max (a w_max above n is n), the
 * TRUE total however small cap is.  list (DEVICE int64, member b's entries at list + b * l_bs, cap of them): the entries
 * i < min(count[b], cap) are DISTINCT keys (wt << 40) | rank of such pairs, in no particular order; count[b] > cap: some cap of them,
 * which ones is not specified.  The entries from min(count[b], cap) on are NOT written.  list and count come together; list may be NULL
 * only with cap = 0.  At least one of hist, lightest and count is required.  m4ri_amd_lists_words_batch_dev below turns the keys into
 * words, which can be a list of the next join.
 * A window entry outside 0 .. n-1 cannot be seen by the host, so the device decides: that member is REFUSED, every one of its hist
 * entries is -1, its lightest -2, its count -1 and no list entry is written; nothing outside the member is read, the other members
 * are unaffected.  A member with nx = 0 or ny = 0 has every bin 0, lightest -1 and count 0; n = 0 with ell = 0 puts all nx * ny pairs
 * into bin 0 (lightest 0 if w_min = 0 and there is a pair; count = nx * ny if w_min = 0, else 0, the first min(count, cap) list entries
 * the keys 0, 1, ...); batch = 0 succeeds without touching anything.
 * Limits: n <= 1024, ell <= 64, nx, ny < 2^31 and nx * ny <= 2^40 (the pair rank fits the key); beyond any of them the call returns
 * hipErrorNotSupported (801) before any HIP call.  There is NO bound on nx by LDS: a workgroup owns a member, a chunk of the left
 * list (as many rows as its LDS table holds) and a slice of the right list, see m4ri_amd_lists_collide_units.  Every workgroup
 * re-reads its slice once per left chunk.  Stern beyond the 8192 left sums of m4ri_amd_row_sums_collide_batch_dev: materialise each half
 * with m4ri_amd_row_sums_words_batch_dev (t2 = 0, k1 = k, an iota of keys) and join those; the list index is then the colexicographic
 * rank, so the pair ranks are the same.
 * Asynchronous on `stream` on both paths of m4ri_amd_plan_lists_collide_batch: plain launches (on path 1 an initialisation of the
 * outputs goes first, on the same stream), no allocation, no copy to the host, no synchronisation, no engine workspace, no engine
 * lock; capturable.  All results are integer counts and minima: they do not depend on the order the hardware takes the pairs in.
 * hipErrorInvalidValue, before any HIP call, for negative sizes, strides or batch strides, w_min, w_max, cap or l_bs < 0, a NULL cols
 * with ell > n, x_stride < words(n) with nx > 1 or y_stride < words(n) with ny > 1, a NULL X or Y where rows are read (batch > 0,
 * n > 0, nx > 0, ny > 0), none of the three outputs, a list without a count, a count without a list at cap > 0, l_bs < cap with
 * batch > 1 (count given), or an output (hist, lightest, count, the list's span from its first member's start to the last member's
 * cap-th entry) whose bytes meet another output or the span (first member's start to last member's end) of X, Y, V or cols. */
int m4ri_amd_lists_collide_batch_dev(const word *X, int64_t x_stride, int64_t x_bs, int64_t nx, const word *Y, int64_t y_stride, int64_t y_bs,
                                     int64_t ny, int64_t n, const word *V, int64_t v_bs, int64_t batch, const int32_t *cols, int64_t c_bs,
                                     int64_t ell, int64_t w_min, int64_t w_max, int64_t *hist, int64_t *lightest, int64_t *list, int64_t l_bs,
                                     int64_t cap, int64_t *count, void *stream);
/* which path the call above takes for members of this shape in a batch of this size (pure host arithmetic; -1 for negative sizes; sizes
 * beyond the call's limits are answered by the same rule): 0 a member is one chunk and one slice, one workgroup writes its outputs with
 * plain stores, the count from a counter in LDS, no global atomics (members without pairs or columns count here: an initialisation
 * kernel answers them); 1 a member has several chunks or slices, a workgroup each, their results combined with global 64-bit integer
 * atomics after an initialisation kernel. */
int m4ri_amd_plan_lists_collide_batch(int64_t nx, int64_t ny, int64_t n, int64_t ell, int64_t batch);
/* the units of the call above, whichever path the shape takes: *chunk_rows = the left rows of a chunk (what one workgroup's LDS table
 * holds; the last chunk of a list is shorter), *chunks = ceil(nx / chunk_rows) and *slices = the slices of the right list per member:
 * slices of ceil(ny / slices) rows, no shorter than min(nx, chunk_rows) or than 256 rows unless the list is, as many as bring the call
 * to 1024 workgroups, a slice times a chunk below 2^32.  chunks = slices = 0 for members without pairs or columns.  Each pointer may
 * be NULL.  Returns 0, or -1 for negative sizes (nothing is stored then). */
int m4ri_amd_lists_collide_units(int64_t nx, int64_t ny, int64_t n, int64_t ell, int64_t batch, int64_t *chunk_rows, int64_t *chunks,
                                 int64_t *slices);
/* The words behind listed keys of two explicit lists, on the device (lists_collide_batch.hip): what m4ri_amd_row_sums_words_batch_dev
 * is to the row-sum calls.  X, Y, V, nx, ny, n, the strides and the sharing rule are those of m4ri_amd_lists_collide_batch_dev.
 * keys (DEVICE int64): member b's at keys + b * l_bs entries.  count (DEVICE int64, batch entries, or NULL): member b has
 * m_b = min(max(count[b], 0), cap) keys, so a refused member's -1 reads as 0 and a count beyond cap as cap; NULL: cap keys per member.
 * W: member b's rows at W + b * w_bs words, w_stride words apart.  For i < m_b let r = keys[b * l_bs + i] & (2^40 - 1): the weight
 * bits above are ignored.  Row i of W_b becomes V_b ^ X_b[r / ny] ^ Y_b[r % ny].  Only the n valid bits are written: bits at
 * columns >= n, padding words, the rows from m_b on and the gaps keep what they held.
 * A key cannot be seen by the host, so the device decides: if keys[...] < 0 or r >= nx * ny the row is SKIPPED, it is not written and
 * no row index is formed from the key.  skipped (DEVICE int32, batch entries, or NULL): skipped[b] = the number of such rows, written
 * whole, 0 for a clean member.
 * Limits: those of the join (n <= 1024, nx, ny < 2^31, nx * ny <= 2^40), beyond them hipErrorNotSupported (801) before any HIP call.
 * Asynchronous on `stream`: a memset of skipped and plain launches, no allocation, no copy to the host, no synchronisation, no engine
 * lock; capturable.  count and keys are read on the device, so they may come from a call still in flight on the same stream.
 * hipErrorInvalidValue, before any HIP call, for negative sizes, strides or batch strides, x_stride < words(n) with nx > 1,
 * y_stride < words(n) with ny > 1, w_stride < words(n) with cap > 1, with batch > 1 and cap > 0 an l_bs < cap or a w_bs below
 * (cap - 1) * w_stride + words(n), a NULL keys, W (n > 0), X or Y (where rows are read) with batch > 0 and cap > 0, or a W or skipped
 * whose bytes meet the span of X, Y, V, keys, count or each other.  batch = 0 succeeds without touching anything; cap = 0 writes skipped
 * only. */
int m4ri_amd_lists_words_batch_dev(const word *X, int64_t x_stride, int64_t x_bs, int64_t nx, const word *Y, int64_t y_stride, int64_t y_bs,
                                   int64_t ny, int64_t n, const word *V, int64_t v_bs, int64_t batch, const int64_t *keys, int64_t l_bs, int64_t cap,
                                   const int64_t *count, word *W, int64_t w_stride, int64_t w_bs, int32_t *skipped, void *stream);
/* The rows of a list of words SORTED and DEDUPLICATED, on the device (sort_rows_batch.hip): what a level list of Wagner's k-tree or of
 * MMT / BJMM needs between two joins -- after a join on a window equal words are the rule, and the keys of a join come in no
 * particular order.  Member b has a list X_b, nx rows of n bits at X + b * x_bs words, the rows x_stride words apart (x_bs = 0: one
 * list shared by all members); X is READ ONLY and only the n valid bits count.  xcount (DEVICE int64, batch entries, or NULL): member
 * b has m_b = min(max(xcount[b], 0), nx) rows, the clamp of the words calls, so the count of a join still in flight on the same stream
 * plugs in and a refused member's -1 reads as 0; NULL: nx rows.  The rows from m_b on are NOT read.
 * cols (DEVICE int32, or NULL): member b's window, ell column indices at cols + b * c_bs entries (c_bs = 0: one window for all
 * members; NULL: the columns 0 .. ell-1), exactly as in the joins: unsorted, repeated, in any word.
 * THE ORDER.  Row i goes before row j iff (key_i, w_i[0], ..., w_i[words(n)-1], i) is lexicographically smaller than the same tuple of
 * j: key is the window bits as an unsigned 64-bit number (bit t = column cols[t]), w[.] are the row's 64-bit words compared as
 * unsigned numbers, the last one masked to the valid bits, and the index makes the order total.  The result is therefore ONE fixed
 * permutation, the same on every run and on both paths.  ell = 0 sorts by the words alone.  The window is the caller's discriminator:
 * after a join on the columns 0 .. l-1 every word is 0 there and word 0 says little, so the natural choice is the NEXT join's window.
 * Equal keys are settled by reading the rows from memory; a window that separates nothing (ell = 0 on rows whose low words agree, or a
 * list of few distinct rows) is correct but slow: every comparison then reads both rows.
 * Outputs, all DEVICE int64, member b's entries at + b * l_bs (ucount: batch entries); at least one of order and ucount is required:
 * order (or NULL): the entries p < m_b hold the index of the p-th row in that order.
 * ucount and uniq: ucount[b] = the number of classes of equal rows (equal on the n valid bits); the entries q < ucount[b] of uniq hold
 * the SMALLEST index of the q-th class, the classes ascending in the order above: the entries of order at the class heads.  The high
 * 24 bits of an entry are 0, so it is a valid key of m4ri_amd_lists_words_batch_dev with ny = 1 (rank = row index): with Y one zero row,
 * keys = uniq and count = ucount that call writes the deduplicated sorted list.  uniq may be NULL: ucount alone counts the distinct
 * rows.  mult (or NULL; needs uniq): mult[q] = the size of class q; a member's entries sum to m_b.
 * The entries from m_b on (order) or from ucount[b] on (uniq, mult) are NOT written.
 * A window entry outside 0 .. n-1 cannot be seen by the host, so the device decides: that member is REFUSED, its ucount is -1 and
 * nothing else of it is written; the other members are unaffected.  nx = 0 or m_b = 0: ucount 0 and no entry.  n = 0 (ell = 0) makes
 * all rows equal: order 0 .. m_b-1, ucount min(m_b, 1), uniq 0, mult m_b.  batch = 0 succeeds without touching anything.
 * scratch, scratch_bytes: DEVICE memory of the caller's, 8-byte aligned, at least m4ri_amd_sort_rows_scratch_bytes(nx, n, ell, batch)
 * bytes, which is 0 (scratch is then ignored) on path 0 of m4ri_amd_plan_sort_rows_batch.  Its content before and after is meaningless.
 * Limits: n <= 1024, ell <= 64, nx <= 2^24 (an index fits the low 24 bits of a key); beyond them hipErrorNotSupported (801) before any
 * HIP call.
 * Asynchronous on `stream` on both paths: plain launches (m4ri_amd_sort_rows_units gives their number), no allocation, no copy to the
 * host, no synchronisation, no engine workspace, no engine lock, no atomics; capturable.  xcount is read on the device.
 * hipErrorInvalidValue, before any HIP call, for negative sizes, strides or batch strides, a NULL cols with ell > n, x_stride <
 * words(n) with nx > 1, l_bs < nx with batch > 1, neither order nor ucount, uniq without ucount, mult without uniq, and with batch > 0
 * a NULL X where rows are read (n > 0, nx > 0), a scratch that is NULL, misaligned or too small where one is needed, or an output or
 * the scratch whose bytes (first member's start to last member's nx-th entry) meet another output or the span of X, xcount or cols. */
int m4ri_amd_sort_rows_batch_dev(const word *X, int64_t x_stride, int64_t x_bs, int64_t nx, int64_t n, const int64_t *xcount, int64_t batch,
                                 const int32_t *cols, int64_t c_bs, int64_t ell, int64_t *order, int64_t *ucount, int64_t *uniq, int64_t *mult,
                                 int64_t l_bs, void *scratch, int64_t scratch_bytes, void *stream);
/* which path the call above takes (pure host arithmetic; -1 for negative sizes; sizes beyond the call's limits are answered by the same
 * rule): 0 nx is at most the chunk of m4ri_amd_sort_rows_units, one workgroup per member sorts its entries in LDS and writes every
 * output with plain stores, one launch, no scratch; 1 longer lists, the entries in the caller's scratch: chunks sorted in LDS, merge
 * levels with their long strides in global memory and their short ones in LDS, then the class heads, a scan and a scatter. */
int m4ri_amd_plan_sort_rows_batch(int64_t nx, int64_t n, int64_t ell, int64_t batch);
/* the units of the call above: *chunk_rows = C, the entries one workgroup sorts in LDS (the longest list of path 0); *padded = the
 * entries the host sizes a member's network by, the smallest power of two >= max(nx, 2) (the device sorts the next power of two of
 * m_b, which is no larger); *launches = the kernel launches of one call that asks for every output, for a batch within one grid: 1 on
 * path 0, and with L = log2(padded / C) on path 1 the chunk sort, per level l = 1 .. L its l global strides and one LDS launch, and
 * four launches for heads, scan, scatter and mult.  Each pointer may be NULL.  Returns 0, or -1 for negative sizes (nothing is stored
 * then). */
int m4ri_amd_sort_rows_units(int64_t nx, int64_t n, int64_t ell, int64_t batch, int64_t *chunk_rows, int64_t *padded, int64_t *launches);
/* the bytes of scratch the sort needs for members of this shape in a batch of this size (pure host arithmetic): 0 on path 0 and for
 * batch = 0, on path 1 a multiple of 16 that holds per member `padded` entries of 8 + 4 + 1 bytes, a count per 1024 entries and one
 * word; -1 for negative sizes or a size beyond int64. */
int64_t m4ri_amd_sort_rows_scratch_bytes(int64_t nx, int64_t n, int64_t ell, int64_t batch);
/* Assembling, cutting and permuting the members of a batch where they are (assemble_batch.hip).  Conventions of the calls below, as
 * of the other batched calls: member b of X is at X + b * x_bs words, its rows x_stride words apart; a batch stride of 0 on a
 * READ-ONLY operand is one operand shared by all members.  Every call is asynchronous on `stream`: plain launches (several for a
 * batch beyond one grid), no allocation, no copy to or from the host, no synchronisation, no engine workspace, no engine lock;
 * capturable -- path 2 of the permutations alone allocates and BLOCKS.  Only the bits a call names as written are written: never
 * a row's other bits in a partly covered word, the words from the width to the stride, the words between members or a read-only
 * operand.  batch = 0 or an empty block succeeds without touching anything.  hipErrorInvalidValue, before any HIP call, for negative
 * sizes, offsets, strides or batch strides, a stride that does not reach the last addressed column, written members that overlap
 * each other, a written operand whose span (from the first member's first addressed word to the last member's last) meets a
 * read-only operand's, or a NULL pointer with non-empty members. */
/* For every member, bit (d_row + i, d_col + j) of D_b <- bit (a_row + i, a_col + j) of A_b, i < rows, j < cols; both column offsets
 * may be any bit position (a 64-bit funnel shift per destination word; the first and the last word of a destination row are written
 * under a mask).  Nothing else in D changes.  Of A only words that hold a bit of the block are read: when the last destination word
 * of a row takes all its bits from one source word, the word after that source word is NOT read, so a block may end in the last word
 * of an allocation.  16-byte accesses where both column offsets are multiples of 64, both first words 16-byte aligned and all four
 * strides even.  mzd_submatrix is d_row = d_col = 0; mzd_concat and mzd_stack are two calls; mzd_copy is all four offsets 0;
 * a_bs = 0 broadcasts one block into every member.  D must not meet A (no copy in place).  Also refused: cols above 2^36 - 64.
 * Overlapping D members: batch > 1 and d_bs < (rows - 1) * d_stride + the words a destination row's block touches. */
int m4ri_amd_copy_block_batch_dev(word *D, int64_t d_stride, int64_t d_bs, int64_t d_row, int64_t d_col, const word *A, int64_t a_stride,
                                  int64_t a_bs, int64_t a_row, int64_t a_col, int64_t rows, int64_t cols, int64_t batch, void *stream);
/* The triangles of A_b (nrows x ncols), k = min(nrows, ncols) (mzd_extract_u / mzd_extract_l, m4ri/mzd.h; the block copy's kernel
 * with a mask per row).  upper != 0: D_b is k x ncols, bit (i, j) = A_b(i, j) for j > i and 0 for j < i.  upper == 0: D_b is
 * nrows x k, bit (i, j) = A_b(i, j) for i > j and 0 for i < j.  The diagonal is 0 (diag == 0), 1 (diag == 1) or A_b(i, i)
 * (diag == 2); any other diag is refused.  rank: a DEVICE int32 array of batch entries, or NULL; an entry outside 0 ... k is
 * clamped.  With it, the upper form's rows i >= rank[b] are written zero, diagonal included, and the lower form's columns
 * j >= rank[b] take nothing from A: they hold the diagonal rule's bit and zeros.  ALL valid bits of D_b are written, whatever they
 * held; A's bits beyond column ncols are never looked at.  rank == NULL, diag == 2, square members: mzd_extract_u / mzd_extract_l
 * bit for bit.  On what m4ri_amd_ple_batch_dev(pluq = 1) left, (upper = 0, diag = 1, rank) is L as nrows x k with identity columns
 * behind the rank and (upper = 1, diag = 2, rank) is U as k x ncols with zero rows behind the rank, so L_b * U_b = P^T A Q^T is
 * defined whatever the rank.  L of a plain PLE (pluq = 0: the columns under the pivots, not compressed) is out of scope.
 * Also refused: nrows or ncols > INT32_MAX, D meeting rank. */
int m4ri_amd_extract_tri_batch_dev(word *D, int64_t d_stride, int64_t d_bs, const word *A, int64_t a_stride, int64_t a_bs, int64_t nrows,
                                   int64_t ncols, int64_t batch, int upper, int diag, const int32_t *rank, void *stream);
/* mzd_apply_p_left{,_trans} on every member, in place, P in DEVICE memory: member b's transpositions are at P + b * p_bs entries
 * (p_bs = 0: one permutation for all members) -- the arrays m4ri_amd_ple_batch_dev writes, with p_bs = nrows.  The row
 * transpositions (i, P[i]), i < min(length, nrows), ascending (trans == 0) or descending.  Only the valid bits of a row move: the
 * bits beyond column ncols stay at their row's position.  Entries P[i] < i are legal (the result is that of the sequence of swaps).
 * An entry outside 0 ... nrows - 1 cannot be checked on the host: such a member is left untouched and status[b] = -1, else
 * status[b] = 0 (status: DEVICE int32, batch entries, or NULL); no entry ever leads to an access outside the member.  With
 * non-empty members and min(length, nrows) = 0 only status is written.  Also refused: A meeting P, status meeting A or P.
 * Asynchronous on paths 0 and 1 of m4ri_amd_plan_perm_batch; path 2 downloads P, checks it on the host the same way, allocates and
 * BLOCKS. */
int m4ri_amd_apply_p_left_batch_dev(word *A, int64_t stride, int64_t a_bs, int64_t nrows, int64_t ncols, int64_t batch, const int32_t *P,
                                    int64_t p_bs, int64_t length, int trans, int32_t *status, void *stream);
/* mzd_apply_p_right{,_trans} the same way (m4ri_amd_ple_batch_dev's Q with p_bs = ncols): the column transpositions (i, P[i]),
 * i < min(length, ncols), descending (trans == 0, A * P) or ascending (A * P^T), the order of m4ri_amd_apply_p_right_dev; an entry
 * outside 0 ... ncols - 1 makes the member's status -1. */
int m4ri_amd_apply_p_right_batch_dev(word *A, int64_t stride, int64_t a_bs, int64_t nrows, int64_t ncols, int64_t batch, const int32_t *P,
                                     int64_t p_bs, int64_t length, int trans, int32_t *status, void *stream);
/* which path the two calls above take (right != 0: m4ri_amd_apply_p_right_batch_dev; pure host arithmetic; -1 for negative sizes):
 * 0 one wave per member, a row per lane, the index in registers, rows moved by ds_bpermute and columns between two register
 * transposes (nrows, ncols <= 64); 1 one workgroup per member, the member's nrows * words(ncols) words plus 8 bytes per row (right:
 * per column) of P and index and 8 bytes of flags in LDS within 160 KiB; 2 members one by one through m4ri_amd_apply_p_left_dev /
 * m4ri_amd_apply_p_right_dev (blocking).  The environment variables M4RI_AMD_PERM_BATCH_PATH0_MAX (the largest side of path 0,
 * clamped to [0, 64]; 0 = no path 0) and M4RI_AMD_PERM_BATCH_PATH1_MAX (the LDS bytes of path 1, clamped to [0, 163840]; 0 = no
 * path 1) replace the bounds in the routing of a call, read per call; this function does not read them. */
int m4ri_amd_plan_perm_batch(int64_t nrows, int64_t ncols, int right);
/* Device twin of mzd_trtri_upper: U (n x n) <- U^-1.  Only the bits strictly above the diagonal (and below column n) are read
 * and written: the diagonal, the lower triangle, the bits beyond column n of a row's last word (whatever they are), the words
 * from words(n) to `stride` and the rows around U come back untouched.  Any word alignment, any stride >= words(n).
 * Asynchronous on `stream`; the calls share grow-only scratch per device (growing it synchronises the device), and a call on
 * another stream than the previous one first waits, on the device, for that one.  hipErrorInvalidValue, before any HIP call,
 * for n < 0. */
int m4ri_amd_trtri_upper_dev(word *U, int64_t stride, int64_t n, void *stream);
/* Device twin of mzd_echelonize* (echelon.hip): A (nrows x ncols) <- its (reduced, full != 0) row echelon form, *rank_out the
 * rank.  Blocking.  Bits at column >= ncols: zero in, zero out (rows are written in whole words, last word included).  Only rows
 * 0 .. nrows-1, words 0 .. words(ncols)-1 are written: never the words from the width to `stride`, never a row before or after
 * A.  Any word alignment, any stride >= width.  hipErrorInvalidValue, before any HIP call, for negative sizes or rank_out ==
 * NULL. */
int m4ri_amd_echelonize_dev(word *A, int64_t stride, int64_t nrows, int64_t ncols, int full, int32_t *rank_out, void *stream);
/* `batch` independent (reduced) row echelon forms in place (echelon_batch.hip).  Member b is the nrows x ncols matrix at
 * A + b * a_bs (words), rows `stride` words apart; each comes out bit-identical to m4ri_amd_echelonize_dev (mzd_echelonize) with
 * the same `full`.  rank[b] (DEVICE int32 array, batch entries) = its rank; pivots (DEVICE int32, batch * min(nrows, ncols) entries,
 * member b at b * min(nrows, ncols), or NULL): the pivot column of each of the first rank[b] rows, -1 after them.  Bits at columns
 * >= ncols of a row's last word, the words from the width to `stride` of a row and the words between members are never written.
 * hipErrorInvalidValue, before any HIP call, for negative sizes, stride < width, overlapping members (batch > 1 and
 * a_bs < (nrows - 1) * stride + width) or rank == NULL with batch > 0.  Asynchronous on `stream` (one launch, no allocation, no
 * copy: capturable) on paths 0-2 of m4ri_amd_plan_echelonize_batch; path 3 allocates and BLOCKS. */
int m4ri_amd_echelonize_batch_dev(word *A, int64_t stride, int64_t a_bs, int64_t nrows, int64_t ncols, int64_t batch, int full, int32_t *rank,
                                  int32_t *pivots, void *stream);
/* which path m4ri_amd_echelonize_batch_dev takes for members of this shape (pure host arithmetic; -1 for negative sizes):
 * 0 one wave per member, rows in registers (nrows, ncols <= 64); 1 one workgroup per member, member in LDS (rows padded to an odd
 * number of words, plus a row index and flags, within 160 KiB); 2 one workgroup per member, in place in global memory (valid words
 * up to 512 KiB); 3 members one by one through m4ri_amd_echelonize_dev (blocking) */
int m4ri_amd_plan_echelonize_batch(int64_t nrows, int64_t ncols);
/* `batch` (reduced) row echelon forms on COLUMN ORDERS CHOSEN PER MEMBER, one launch, no column ever moved (echelon_order_batch.hip):
 * the systematic form of a generator on an information set given by the caller, the step before the enumerations of
 * m4ri_amd_row_sums_weights_batch_dev in information-set decoding (a random set per iteration) and Brouwer-Zimmermann bounds
 * (successive disjoint sets).  Member b reads A_b, nrows x ncols at A + b * a_bs words, rows a_stride words apart (a_bs = 0: one A
 * shared by all members), and writes D_b at D + b * d_bs, rows d_stride apart.  A is READ ONLY unless the call is in place: D == A
 * with equal strides and batch strides, which is allowed (refused with a_bs = 0 and batch > 1); any other meeting of D's span with A's
 * is refused.  order (DEVICE int32, or NULL): member b's olen entries at order + b * o_bs (o_bs = 0: one order for all members) are the
 * columns in the order they are visited; NULL is the natural order 0 .. olen-1; 0 <= olen <= ncols.  Entries need not be distinct: a
 * column visited twice finds no pivot the second time.  An entry outside 0 ... ncols - 1 cannot be checked on the host: such a member
 * gets rank[b] = -1 and all its pivots -1, and its D_b is NOT written at all (in place: left untouched); no entry ever leads to an
 * access outside a member.
 * The rule.  rank = 0; for j = 0 .. olen-1, while rank < pivot_rows, with c = order[j]: the pivot is the first row i,
 * rank <= i < pivot_rows, with bit c set; if there is none go on with the next j; else swap it up to row `rank`, add it into every
 * other row with bit c set -- the rows > rank (full == 0) or all rows (full != 0) -- set pivots[b * pm + rank] = c (the column, not
 * j) and ++rank.  pm = min(pivot_rows, ncols); pivots (DEVICE int32, batch * pm entries, or NULL) is -1 from rank[b] on; rank (DEVICE
 * int32, batch entries) is required.  0 <= pivot_rows <= nrows: the rows from pivot_rows on only FOLLOW -- never pivots, never swapped,
 * reduced like any other row with the bit, and below every rank under full == 0.  A received word y stacked under a generator comes
 * out under full = 1 as y ^ y_I G', the starting error pattern of Lee-Brickell and the V of m4ri_amd_row_sums_weights_batch_dev.
 * pivot_rows = 0 copies A_b to D_b with rank 0.
 * order == NULL, olen == ncols, pivot_rows == nrows, in place: m4ri_amd_echelonize_batch_dev bit for bit, words, rank and pivots.
 * order a permutation of all columns: gathering the columns in that order, mzd_echelonize, and scattering them back, bit for bit.
 * Only the valid bits of D_b are written: never the bits at columns >= ncols, the words from the width to the stride or the words
 * between members.  hipErrorInvalidValue, before any HIP call, for negative sizes, strides or batch strides, pivot_rows > nrows,
 * olen > ncols, a stride below words(ncols), overlapping D members (batch > 1 and d_bs < (nrows - 1) * d_stride + width), D's span
 * meeting A's (except exactly in place), order, rank or pivots, rank or pivots meeting each other or order, a NULL rank, or a NULL A or
 * D with non-empty members.  batch = 0 succeeds without touching anything.  Members beyond path 2 of
 * m4ri_amd_plan_echelonize_order_batch return hipErrorNotSupported (801), nothing touched: there is no one-by-one path.  Asynchronous
 * on `stream` on every path: one launch (several for a batch beyond one grid), no allocation, no copy to the host, no
 * synchronisation, no engine lock; capturable. */
int m4ri_amd_echelonize_order_batch_dev(word *D, int64_t d_stride, int64_t d_bs, const word *A, int64_t a_stride, int64_t a_bs, int64_t nrows,
                                        int64_t ncols, int64_t pivot_rows, const int32_t *order, int64_t o_bs, int64_t olen, int64_t batch,
                                        int full, int32_t *rank, int32_t *pivots, void *stream);
/* which path the call above takes for members of this shape (pure host arithmetic; -1 for negative sizes): 0 one wave per member, lane
 * i holds row i and lane j order[j] (nrows, ncols <= 64); 1 one workgroup per member, member in LDS (rows padded to an odd number of
 * words, a row index, flags, 64 bytes of votes and an order of ncols entries, within 160 KiB); 2 one workgroup per member in place in D_b, which the
 * kernel fills from A_b first when out of place (valid words up to 512 KiB); 3 above that: the call returns 801.  The environment
 * variables M4RI_AMD_ECH_ORDER_PATH0_MAX (the largest side of path 0, clamped to [0, 64]) and M4RI_AMD_ECH_ORDER_PATH1_MAX (the LDS
 * bytes of path 1, clamped to [0, 163840]) replace the bounds in the routing of a call, read per call; this function does not read
 * them. */
int m4ri_amd_plan_echelonize_order_batch(int64_t nrows, int64_t ncols);
/* Seeded random column orders for the call above, made on the device: order + b * o_bs (DEVICE int32) receives a permutation of
 * 0 .. n-1 for every member, defined so that any host reproduces it (m4ri_amd.random_order in the Python layer).  h_j = output number
 * b * n + j of the counter-form splitmix64 stream seeded `seed` (the stream of m4ri_amd_fill_dev); key_j = h_j with its low 12 bits
 * replaced by j; the keys sorted ascending as unsigned 64-bit numbers; order[i] = the low 12 bits of the i-th key.  One workgroup per
 * member sorts in LDS; one launch, asynchronous on `stream`, no allocation; capturable.  0 <= n <= 4096, beyond that
 * hipErrorNotSupported (801).  hipErrorInvalidValue for negative n, batch or o_bs, o_bs < n with batch > 1, or a NULL order with
 * batch > 0 and n > 0. */
int m4ri_amd_random_orders_batch_dev(int32_t *order, int64_t o_bs, int64_t n, int64_t batch, uint64_t seed, void *stream);
/* `steps` PIVOT EXCHANGES on the stored reduced echelon forms of `batch` members, one launch (pivot_exchange_batch.hip): the move from
 * one information set to the next in information-set decoding, one pivot step on a form that is already reduced instead of an
 * elimination from scratch.  The state is what m4ri_amd_echelonize_order_batch_dev(full = 1) left: D_b, nrows x ncols at D + b * d_bs
 * words, rows d_stride apart, in place; pivots (DEVICE int32, in/out), member b's pm = min(pivot_rows, ncols) entries at b * pm, entry
 * i the pivot column of row i; rank (DEVICE int32, batch entries, READ ONLY).  R_b = min(max(rank[b], 0), pm): a refused member's -1
 * reads as 0.  The rows from pivot_rows on only follow.
 * The rule.  For s = 0 .. steps-1, in this order, member b:
 * 1. The request (r, c).  With req (DEVICE int32): r = req[b * r_bs + 2 s], c = req[b * r_bs + 2 s + 1] (r_bs = 0: one list for all
 *    members).  With req == NULL it is drawn on the device so that any host reproduces it (m4ri_amd.exchange_draw in the Python layer):
 *    h = output number b * steps + s of the counter-form splitmix64 stream seeded `seed` (the stream of m4ri_amd_fill_dev and
 *    m4ri_amd_random_orders_batch_dev); if R_b = 0 the step is skipped; else r = (h >> 32) mod R_b, start = (h & 0xffffffff) mod ncols,
 *    and c = the first column in the cyclic order start, start + 1, ..., ncols - 1, 0, ..., start - 1 with bit (r, c) of the current D_b
 *    set and c != pivots[r]; if there is none the step is skipped.
 * 2. Validity, decided on the device.  The step is performed iff 0 <= r < R_b, 0 <= c < ncols, bit (r, c) is set and c != pivots[r];
 *    otherwise it is skipped: nothing is written, and no index is formed from the request.  On a reduced form a column that is another
 *    row's pivot has bit (r, c) clear, so such a request falls out here.
 * 3. The exchange.  Every row i != r of all nrows rows, followers included, with bit c set becomes row i ^ row r.  old = pivots[r],
 *    then pivots[r] = c.  With order (DEVICE int32, in/out, member b's olen entries at order + b * o_bs; NULL or olen = 0: none kept):
 *    p = the first position with order[p] == old, q = the first with order[q] == c; if both exist the two entries are swapped,
 *    otherwise order is unchanged.  Entries of order are only compared, never used as indices: they need no range check.
 * done[b] (DEVICE int32, batch entries, or NULL) = the number of steps performed, written whole.  Only the valid bits of D_b are
 * written: never the bits at columns >= ncols, the words from the width to the stride or the words between members; a member with
 * no performed step is not written at all.  After the call D_b is again the reduced form for the new pivots, so calls chain.  For
 * full-rank members the result equals m4ri_amd_echelonize_order_batch_dev(A, order = the new pivots, full = 1) bit for bit, followers
 * included: the reduced form on an information set is unique.  With an order kept (the order the form was made on), cols = order + k
 * stays a window of non-information columns for m4ri_amd_row_sums_collide_batch_dev.
 * hipErrorInvalidValue, before any HIP call, for negative sizes, strides, batch strides or steps, pivot_rows > nrows, olen > ncols,
 * d_stride < words(ncols), overlapping D members (batch > 1 and d_bs < (nrows - 1) * d_stride + width), r_bs < 2 * steps with
 * r_bs != 0 and batch > 1, o_bs < olen with an order and batch > 1 (order is written: it cannot be shared), a NULL D, pivots or rank
 * with non-empty members and steps > 0, or any two of D's span, pivots, rank, req, order and done whose bytes meet.  batch = 0
 * succeeds without touching anything; steps = 0 writes done (zeros) only.  Members beyond path 2 of
 * m4ri_amd_plan_pivot_exchange_batch return hipErrorNotSupported (801), nothing touched.  Asynchronous on `stream`: plain launches
 * (one, several for a batch beyond one grid), no allocation, no copy to the host, no synchronisation, no engine lock, no atomics;
 * capturable. */
int m4ri_amd_pivot_exchange_batch_dev(word *D, int64_t d_stride, int64_t d_bs, int64_t nrows, int64_t ncols, int64_t pivot_rows, int32_t *pivots,
                                      const int32_t *rank, int64_t batch, const int32_t *req, int64_t r_bs, int64_t steps, uint64_t seed,
                                      int32_t *order, int64_t o_bs, int64_t olen, int32_t *done, void *stream);
/* which path the call above takes for members of this shape and this many steps (pure host arithmetic; -1 for negative sizes or
 * steps): 0 one wave per member, lane i holds row i and pivots[i], lane j order[j] (nrows, ncols <= 64); 1 one workgroup per member,
 * the member staged in LDS for all steps (rows padded to an odd number of words, a row index, one flag buffer, 128 bytes of slots and
 * an order of ncols entries, within 160 KiB) and steps != 1; 2 one workgroup per member in place in D_b (valid words up to 512 KiB),
 * which a call of ONE step takes for members that would fit in LDS too: a step in place touches only the rows with the bit while
 * staging moves the whole member, and as measured (steps = 1, 4 and 16) in place wins at one step and loses at four;
 * 3 above the cap: the call returns 801.  The environment variables M4RI_AMD_PIVOT_EXCHANGE_PATH0_MAX (the largest side of path 0,
 * clamped to [0, 64]) and M4RI_AMD_PIVOT_EXCHANGE_PATH1_MAX (the LDS bytes of path 1, clamped to [0, 163840]; when it is set, it
 * alone decides between paths 1 and 2, at any step count) replace the bounds in the routing of a call, read per call; this function
 * does not read them. */
int m4ri_amd_plan_pivot_exchange_batch(int64_t nrows, int64_t ncols, int64_t steps);
/* A whole INFORMATION-SET DECODING SEARCH on the stored reduced echelon forms of `batch` members, one launch (isd_search_batch.hip): up
 * to `iters` times "exchange `steps` pivots, then weigh all sums of t pivot rows against the received word", the lightest word seen
 * kept with its key and its iteration, a member stopped as soon as that weight is <= w_stop.  t = 0 is Prange, t >= 1 Lee-Brickell;
 * without a follower row it is a search for light codewords (w_min = 1).  The rule is a composition of two calls of this header, and
 * the results equal theirs bit for bit.
 * The state is that of m4ri_amd_pivot_exchange_batch_dev: D_b in place, pivots in/out, rank READ ONLY, the optional order in/out.
 * k = pivot_rows; G_b = rows 0 .. k-1 of the current D_b; V_b = row k of the current D_b if nrows > pivot_rows, else the zero word: the
 * first follower is the received word, further followers only follow.
 * The rule.  Iteration it = 0, 1, ... of member b:
 * 1. If it > 0: `steps` exchanges exactly as m4ri_amd_pivot_exchange_batch_dev(req = NULL, steps, seed = seed_it) performs them on this
 *    member -- the same draw h = output number b * steps + s of the stream seeded seed_it, the same validity test, the same update of
 *    D, pivots and order -- with seed_it = output number `it` of the counter-form splitmix64 stream seeded `seed`
 *    (m4ri_amd.isd_iteration_seed in the Python layer).  Iteration 0 enumerates the form as the caller left it.
 * 2. key_it = what m4ri_amd_row_sums_weights_batch_dev(G_b, k, n = ncols, V_b, t, w_min) writes to lightest: the minimum of
 *    (wt << 40) | colexicographic rank over the sets with wt >= w_min, -1 if there is none.
 * 3. The best is replaced when key_it >= 0 and either best < 0 or (key_it >> 40) < (best >> 40): only a strictly lighter word replaces
 *    it, so the earliest iteration wins among equal weights.  Then best = key_it, best_iter = it and W_b = the word c(S) of that key on
 *    the form of this iteration (only the ncols valid bits of W_b, at W + b * w_bs, are written).
 * 4. If best >= 0 and (best >> 40) <= w_stop the member stops, iters_run[b] = it + 1.  A negative w_stop never stops a member.
 * Otherwise the loop ends after `iters` iterations, iters_run[b] = iters.  D_b, pivots and order are left as the last iteration run
 * left them, so calls chain; done[b] = all exchange steps performed.  best (DEVICE int64) is required; best_iter, iters_run, done
 * (DEVICE int32) and W are optional.  Every wanted output is written whole -- best_iter[b] = -1 where best[b] = -1 -- except that W_b
 * of a member with best = -1 is not written, and a member's D, pivots and order are written only if a step was performed.  iters = 0
 * gives best = -1 and iters_run = 0 and touches nothing else.  rank is read by the exchange only: a refused member (rank -1)
 * exchanges nothing and is still enumerated, as the composition would.
 * hipErrorNotSupported (801), before any HIP call: pivot_rows or ncols > 1024, t > 8, C(pivot_rows, t) > 2^24 (one workgroup walks all
 * sums of its member in every iteration; beyond that the two-call iteration, which spreads a member over the chip, is the right
 * tool), a member beyond path 1 of m4ri_amd_plan_isd_search, or counts beyond 32 bits (iters or (iters - 1) * steps > 2^31 - 1).
 * hipErrorInvalidValue, before any HIP call, for negative sizes, strides, batch strides, iters, steps, t or w_min, pivot_rows > nrows,
 * olen > ncols, d_stride < words(ncols), overlapping D members, o_bs < olen with an order and batch > 1, w_bs < words(ncols) with W
 * and batch > 1, a NULL best with batch > 0, a NULL D with non-empty members and iters > 0, a NULL pivots or rank when an exchange
 * can happen (non-empty members, steps > 0 and iters > 1), or any two of D's span, pivots, rank, order, best, best_iter, iters_run,
 * done and W whose bytes meet.  batch = 0 succeeds and touches nothing.  Asynchronous on `stream`: plain launches, no allocation, no
 * copy to the host, no engine lock, no atomics; capturable.
 * WHICH TO USE (measured at t = 2, 16 iterations): this call is ahead of the loop of the two calls at every measured
 * shape -- 1.3x at 32 x 64, 2.0x to 2.6x at 64 x 128, where the loop's launches and stagings are the time, and 1.08x to 1.10x at
 * 256 x 512, where the enumeration is -- and only it can stop a member.  Beyond 2^24 sums per member (refused here) and for a handful
 * of large members, use the two calls: they spread one member's sums over the chip, here one workgroup walks them all. */
int m4ri_amd_isd_search_dev(word *D, int64_t d_stride, int64_t d_bs, int64_t nrows, int64_t ncols, int64_t pivot_rows, int32_t *pivots,
                            const int32_t *rank, int64_t batch, int64_t iters, int64_t steps, uint64_t seed, int64_t t, int64_t w_min, int64_t w_stop,
                            int32_t *order, int64_t o_bs, int64_t olen, int64_t *best, int32_t *best_iter, int32_t *iters_run, int32_t *done, word *W,
                            int64_t w_bs, void *stream);
/* which path the call above takes (pure host arithmetic; -1 for negative sizes): 0 one wave per member, four members per workgroup,
 * lane i holds row i (nrows, ncols <= 64); 1 one workgroup per member, the member staged in LDS once for the whole loop (the layout
 * of path 1 of m4ri_amd_plan_pivot_exchange_batch, with 128 bytes of key slots and a word of words(ncols) words behind the slots,
 * within 160 KiB); 2 everything else, the limits above included: the call returns 801.  There is no path in place in global memory:
 * the call exists for members that stay resident.  The environment variable M4RI_AMD_ISD_SEARCH_PATH0_MAX (the largest side of
 * path 0, clamped to [0, 64]) replaces the bound in the routing of a call, read per call; this function does not read it. */
int m4ri_amd_plan_isd_search(int64_t nrows, int64_t ncols, int64_t pivot_rows, int64_t t);
/* A whole STERN COLLISION DECODING SEARCH on the stored reduced echelon forms of `batch` members, one launch
 * (isd_collide_search_batch.hip): up to `iters` times "exchange `steps` pivots, then join the sums of t1 of the first k1 pivot rows and
 * of t2 of the other pivot rows on a window of ell non-information columns and weigh the colliding pairs against the received word",
 * the lightest word seen kept with its key and its iteration, a member stopped as soon as that weight is <= w_stop.  The rule is a
 * composition of two calls of this header, and the results equal theirs bit for bit.
 * The state is exactly that of m4ri_amd_isd_search_dev: D_b in place, pivots in/out, rank READ ONLY, order in/out.  k = pivot_rows;
 * G_b = rows 0 .. k-1 of the current D_b; V_b = row k of the current D_b if nrows > pivot_rows, else the zero word; further followers
 * only follow.
 * The rule.  Iteration it = 0, 1, ... of member b:
 * 1. If it > 0: `steps` exchanges exactly as m4ri_amd_pivot_exchange_batch_dev(req = NULL, steps, seed = seed_it) performs them on this
 *    member -- the same draw, the same validity test, the same update of D, pivots and order -- with seed_it = output number `it` of the
 *    counter-form splitmix64 stream seeded `seed` (m4ri_amd.isd_iteration_seed).  Iteration 0 enumerates the form as the caller left it.
 * 2. key_it = what m4ri_amd_row_sums_collide_batch_dev(G_b, k, n = ncols, V_b, k1, t1, t2, cols = order + b * o_bs + pivot_rows, ell,
 *    w_min) writes to lightest on the form and the order AS THEY STAND AFTER STEP 1: the minimum of (wt << 40) | (r1 * N2 + r2) over
 *    the colliding pairs with wt >= w_min (N1 = C(k1, t1), N2 = C(k - k1, t2), m4ri_amd.row_pair_unrank splits the rank), -1 if there
 *    is none, and -2 -- the composition's refused form -- if one of the ell window entries is outside 0 .. ncols-1.  The window is
 *    range-checked on the device in every iteration: an exchange swaps the leaving pivot column into the place of the entering one,
 *    which may lie in the window.  With ell = 0 every pair collides and order may be NULL (none kept).
 * 3. The best is replaced iff key_it >= 0 and (best < 0 or (key_it >> 40) < (best >> 40)): only a strictly lighter word replaces it, so
 *    the earliest iteration wins among equal weights.  Then best = key_it, best_iter = it and W_b = V_b ^ rows S1 ^ rows S2 of that pair
 *    on the form of this iteration (only the ncols valid bits of W_b, at W + b * w_bs, are written).
 * 4. If best >= 0 and (best >> 40) <= w_stop the member stops, iters_run[b] = it + 1.  A negative w_stop never stops a member.
 * Otherwise the loop ends after `iters` iterations, iters_run[b] = iters.  D_b, pivots and order are left as the last iteration run
 * left them, so calls chain; done[b] = all exchange steps performed.  best (DEVICE int64) is required; best_iter, iters_run, done
 * (DEVICE int32) and W are optional.  Every wanted output is written whole -- best_iter[b] = -1 where best[b] < 0 -- except that W_b of
 * a member with best < 0 is not written, and a member's D, pivots and order are written only if a step was performed.  iters = 0 gives
 * best = -1 and iters_run = 0 and touches nothing else.  A member whose window is refused in every iteration ends with best = -1.
 * hipErrorInvalidValue, before any HIP call: everything m4ri_amd_isd_search_dev refuses on the arguments the two share; k1 < 0 or
 * k1 > pivot_rows; negative t1, t2 or ell; ell > 0 with a NULL order or with olen < pivot_rows + ell (the window is entries
 * pivot_rows .. pivot_rows + ell - 1 of the order).  hipErrorNotSupported (801), before any HIP call: pivot_rows or ncols > 1024, t1
 * or t2 > 8, ell > 64, N1 > 8192, N2 > 2^24 (one workgroup walks its member's whole right list in every iteration; beyond that the two
 * calls, which slice the list over the chip, are the tool), N1 * N2 > 2^40, counts beyond 32 bits (iters or (iters - 1) * steps >
 * 2^31 - 1), or a member m4ri_amd_plan_isd_collide_search does not place.  batch = 0 succeeds and touches nothing.  Asynchronous on
 * `stream`: plain launches, no allocation, no copy to the host, no engine lock, no global atomics; capturable.
 * WHICH TO USE (measured at 16 iterations, steps 1 and 4, a received word): this call is ahead of the loop of the two
 * calls at every measured shape, each time beyond the spread -- 6.2x and 3.8x at 32 x 64 (65 536 members, t = 1 + 1, ell = 4), 5.8x and
 * 4.6x at 64 x 128 (t = 1 + 1, ell = 5), where the loop's stagings, launches and reads of the rows from global memory are the time;
 * 1.8x at 64 x 128 with t = 2 + 2, ell = 9 and 2.2x and 2.1x at 256 x 512 (4 096 members, t = 2 + 2, ell = 13), where the join is --
 * and only it keeps the running minimum, writes the winning word and stops a member on the device (w_stop at the median best weight:
 * 9.9 of 16 iterations per member in 0.67 of the time).  It lost at no measured shape.  Not measured: other t, shapes between these,
 * and batches too small to fill the chip: there, beyond 2^24 right sums per member (refused here) and for a handful of large members
 * use the two calls, which slice one member's right list over the chip while here one workgroup walks it all. */
int m4ri_amd_isd_collide_search_dev(word *D, int64_t d_stride, int64_t d_bs, int64_t nrows, int64_t ncols, int64_t pivot_rows, int32_t *pivots,
                                    const int32_t *rank, int64_t batch, int64_t iters, int64_t steps, uint64_t seed, int64_t k1, int64_t t1,
                                    int64_t t2, int64_t ell, int64_t w_min, int64_t w_stop, int32_t *order, int64_t o_bs, int64_t olen,
                                    int64_t *best, int32_t *best_iter, int32_t *iters_run, int32_t *done, word *W, int64_t w_bs, void *stream);
/* whether the call above places members of this shape (pure host arithmetic; -1 for negative sizes or k1 > pivot_rows): 1 one
 * workgroup per member, staged in LDS once for the whole loop -- path 1's staging of m4ri_amd_plan_isd_search (the word of
 * words(ncols) words and an order of ncols entries included), rounded up to 16 bytes, then pivot_rows + 1 row keys of 8 bytes, N1
 * sorted keys of 8 bytes, 128 bytes of wave minima, 2^q bucket ends of 4 bytes (q = ceil(log2 N1) held at ell), 4096 bytes of scan
 * sums, a window of 256 bytes and N1 left indices of 2 bytes (rounded up to 16), plus 256 bytes the kernel keeps for itself, within
 * 160 KiB; 2 everything else, the limits above included: the call returns 801.  There is no wave-per-member path: small members get a
 * small workgroup instead.  The environment variable M4RI_AMD_ISD_COLLIDE_SEARCH_THREADS (a multiple of 64 in [64, 1024]) replaces
 * the workgroup size of a call, read per call: results do not depend on it. */
int m4ri_amd_plan_isd_collide_search(int64_t nrows, int64_t ncols, int64_t pivot_rows, int64_t k1, int64_t t1, int64_t t2, int64_t ell);
/* `batch` independent systems A_b X_b = B_b (mzd_solve_left, m4ri/solve.c:30-152; solve_batch.hip).  A_b: the m x n matrix at
 * A + b * a_bs, READ ONLY (a_bs = 0: one A shared by all members).  B_b: the max(m, n) x k matrix at B + b * b_bs.  status[b]
 * (DEVICE int32, required): 0, or -1 when A_b X = B_b has no solution, A_b padded with zero rows to max(m, n).  On status 0, B_b is
 * overwritten exactly as m4ri_amd_solve_left_dev leaves it: X in rows 0 .. n-1 with the rows of the non-pivot columns zero, rows
 * n .. max(m, n)-1 zero.  On -1, B_b is left untouched.  rank[b] (DEVICE int32, or NULL): the rank of A_b.
 * Consistency is always checked, over all padding rows: for m < n a non-zero row m of B makes the member -1 here, while
 * m4ri_amd_solve_left_dev (as _mzd_solve_left, solve.c:124) looks only from row m + 1 on and returns 0.
 * Bits at columns >= k of a row's last word, the words from the width to the stride of a row, the words between members and A are
 * never written.  hipErrorInvalidValue, before any HIP call, for negative sizes, strides or batch strides, a stride below the
 * width, overlapping B members (batch > 1 and b_bs < (max(m, n) - 1) * b_stride + width), status == NULL with batch > 0, or a NULL
 * A or B with a non-empty member.  Asynchronous on `stream` (one launch, no allocation, no copy) on paths 0 and 1 of
 * m4ri_amd_plan_solve_batch; path 2 allocates and BLOCKS. */
int m4ri_amd_solve_left_batch_dev(const word *A, int64_t a_stride, int64_t a_bs, int64_t m, int64_t n, word *B, int64_t b_stride, int64_t b_bs,
                                  int64_t k, int64_t batch, int32_t *status, int32_t *rank, void *stream);
/* `batch` inverses (mzd_inv_m4ri, m4ri/brilliantrussian.c:971-997): Binv_b (n x n at Binv + b * b_bs) <- the right half of the
 * reduced echelon form of [A_b | I], bit-identical to m4ri_amd_inv_dev, singular members included.  rank[b] (DEVICE int32, or
 * NULL) = the rank of A_b (n: invertible).  Binv == A with equal strides and batch strides (in place) is allowed; any other overlap
 * of the two is not (hipErrorInvalidValue).  Memory rules, argument checks and paths as m4ri_amd_solve_left_batch_dev, with
 * m = k = n. */
int m4ri_amd_inv_batch_dev(word *Binv, int64_t b_stride, int64_t b_bs, const word *A, int64_t a_stride, int64_t a_bs, int64_t n, int64_t batch,
                           int32_t *rank, void *stream);
/* which path m4ri_amd_solve_left_batch_dev takes for this (m, n, k) and m4ri_amd_inv_batch_dev for (n, n, n) (pure host arithmetic;
 * -1 for negative sizes): 0 one wave per member (max(m, n) <= 64 and k <= 64); 1 one workgroup per member in LDS (max(m, n) rows of
 * words(n) + words(k) words padded to an odd count, plus a row index and three flag words per 64 rows, within 160 KiB: the largest
 * inverse is 768 x 768); 2 members one by one through the per-member call (blocking) */
int m4ri_amd_plan_solve_batch(int64_t m, int64_t n, int64_t k);
/* `batch` null-space bases {x : A_b x = 0} (mzd_kernel_left_pluq, m4ri/solve.c:154-191; solve_batch.hip).  A_b: the m x n matrix
 * at A + b * a_bs, READ ONLY (a_bs = 0: one A shared by all members; unlike m4ri_amd_kernel_left_pluq_dev, A is not overwritten).
 * R_b: the n x kc matrix at R + b * r_bs (kc <= n).  Its first min(kc, n - rank[b]) columns are the first basis vectors exactly as
 * m4ri_amd_kernel_left_pluq_dev lays them out; the columns from there up to kc are written zero (R need not be cleared).  kc = n
 * holds the whole basis, kc = 1 one dependency (if any).  rank[b] (DEVICE int32, required) = the rank of A_b: the nullity is
 * n - rank[b], and when it exceeds kc the basis was cut.  m = 0 gives the first kc columns of the identity; n = 0 writes only rank.
 * Bits at columns >= kc of a row's last word, the words from the width to r_stride of a row, the words between members and A are
 * never written.  hipErrorInvalidValue, before any HIP call, for negative sizes, strides or batch strides, kc > n, a_stride <
 * words(n) or r_stride < words(kc), overlapping R members (batch > 1 and r_bs < (n - 1) * r_stride + words(kc)), R overlapping A
 * (the span from the first member's start to the last member's end of each), rank == NULL with batch > 0, or a NULL A or R with a
 * non-empty member.  batch = 0 succeeds without touching anything.  Asynchronous on `stream` (one launch, no allocation, no copy:
 * capturable) on paths 0 and 1 of m4ri_amd_plan_kernel_batch; path 2 allocates and BLOCKS. */
int m4ri_amd_kernel_left_batch_dev(const word *A, int64_t a_stride, int64_t a_bs, int64_t m, int64_t n, word *R, int64_t r_stride, int64_t r_bs,
                                   int64_t kc, int64_t batch, int32_t *rank, void *stream);
/* which path m4ri_amd_kernel_left_batch_dev takes for m x n members (pure host arithmetic; -1 for negative sizes): 0 one wave per
 * member (m, n <= 64); 1 one workgroup per member in LDS (m rows of words(n) words padded to an odd count, a row index, three flag
 * words per 64 of max(m, n), two int32 tables of n entries, within 160 KiB: 1024 x 1024 fits); 2 members one by one through
 * m4ri_amd_kernel_left_pluq_dev on scratch copies (blocking) */
int m4ri_amd_plan_kernel_batch(int64_t m, int64_t n);
/* `batch` PLE (pluq == 0) or PLUQ (pluq != 0) decompositions in place (ple_batch.hip).  Member b is the nrows x ncols matrix at
 * A + b * a_bs (words), rows `stride` words apart; it comes out bit-identical to m4ri_amd_ple_dev / m4ri_amd_pluq_dev with
 * recursion_cutoff = 0 (_mzd_ple_russian / _mzd_pluq_russian).  P (DEVICE int32, batch * nrows entries, member b at b * nrows),
 * Q (DEVICE int32, batch * ncols entries, member b at b * ncols) and rank (DEVICE int32, batch entries) are all required: the
 * reference's LAPACK-style transpositions, the identity behind the rank in both.  For every member small enough for paths 0-2
 * _mzd_ple and _mzd_ple_russian leave the same Q (the recursion of ple.c only starts above M4RI_AMD_PLE_CUTOFF words); path 3 calls
 * the per-member functions with recursion_cutoff = 0, so its Q is _mzd_ple_russian's as well.
 * Bits at columns >= ncols of a row's last word, the words from the width to `stride` of a row and the words between members are
 * never written.  hipErrorInvalidValue, before any HIP call, for negative sizes, strides or batch strides, stride < words(ncols),
 * overlapping members (batch > 1 and a_bs < (nrows - 1) * stride + words(ncols)), a NULL A with a non-empty member, rank == NULL with
 * batch > 0, P == NULL with batch * nrows > 0 or Q == NULL with batch * ncols > 0.  batch = 0 succeeds without touching anything;
 * nrows = 0 or ncols = 0 writes rank 0 and the identity to P and Q and no matrix word.  Asynchronous on `stream` (one launch, no
 * allocation, no copy, no host synchronisation) on paths 0-2 of m4ri_amd_plan_ple_batch; path 3 allocates and BLOCKS.
 * To use P, Q and the factors without a download: m4ri_amd_extract_tri_batch_dev gives L and U of every member,
 * m4ri_amd_apply_p_left_batch_dev / m4ri_amd_apply_p_right_batch_dev take P and Q as they lie here (p_bs = nrows / ncols), and
 * m4ri_amd_pluq_solve_left_batch_dev solves from them. */
int m4ri_amd_ple_batch_dev(word *A, int64_t stride, int64_t a_bs, int64_t nrows, int64_t ncols, int64_t batch, int pluq, int32_t *P, int32_t *Q,
                           int32_t *rank, void *stream);
/* which path m4ri_amd_ple_batch_dev takes for members of this shape (pure host arithmetic; -1 for negative sizes): 0 one wave per
 * member, rows, P and Q in registers (nrows, ncols <= 64); 1 one workgroup per member, member in LDS (rows padded to an odd number
 * of words, a row index, P, Q -- each int32 array rounded up to 16 bytes -- and two flag words per 64 rows, within 160 KiB); 2 one
 * workgroup per member, in place in global memory (valid words up to 512 KiB); 3 members one by one through m4ri_amd_ple_dev /
 * m4ri_amd_pluq_dev (blocking) */
int m4ri_amd_plan_ple_batch(int64_t nrows, int64_t ncols);
/* `batch` solves A_b X_b = B_b from stored factors (mzd_pluq_solve_left, m4ri/solve.c:57-121; ple_batch.hip).  A_b (m x n at
 * A + b * a_bs), rank[b], P (member b at b * m) and Q (member b at b * n) are what m4ri_amd_ple_batch_dev(pluq = 1) left; they are
 * READ ONLY, and only the bits of A_b on the proper side of the diagonal are read.  a_bs = 0: one decomposition (A, rank[0], the
 * first m entries of P, the first n of Q) serves every member.  B_b: the max(m, n) x k matrix at B + b * b_bs.
 * The result is that of m4ri_amd_solve_left_batch_dev on the original A_b, byte for byte: status[b] (DEVICE int32, required) is 0,
 * or -1 when there is no solution, consistency checked over all padding rows; on status 0, B_b holds X in rows 0 .. n-1 with the
 * rows of the non-pivot columns zero, rows n .. max(m, n)-1 zero; on -1, B_b is left untouched.  So "factor once, solve later" and
 * "solve in one call" can be exchanged freely.
 * Bits at columns >= k of a row's last word, the words from the width to the stride of a row, the words between members, A, rank,
 * P and Q are never written.  hipErrorInvalidValue, before any HIP call, for negative sizes, strides or batch strides, a stride
 * below the width, overlapping B members (batch > 1 and b_bs < (max(m, n) - 1) * b_stride + words(k)), B overlapping A (the span
 * from the first member's start to the last member's end of each), status or rank == NULL with batch > 0, P == NULL with
 * batch * m > 0, Q == NULL with batch * n > 0, or a NULL A or B with a non-empty member.  Asynchronous on `stream` (one launch, no
 * allocation, no copy) on paths 0 and 1 of m4ri_amd_plan_pluq_solve_batch; path 2 allocates and BLOCKS. */
int m4ri_amd_pluq_solve_left_batch_dev(const word *A, int64_t a_stride, int64_t a_bs, int64_t m, int64_t n, const int32_t *rank, const int32_t *P,
                                       const int32_t *Q, word *B, int64_t b_stride, int64_t b_bs, int64_t k, int64_t batch, int32_t *status,
                                       void *stream);
/* which path m4ri_amd_pluq_solve_left_batch_dev takes (pure host arithmetic; -1 for negative sizes): 0 one wave per member
 * (max(m, n) <= 64 and k <= 64); 1 one workgroup per member, B_b in LDS (max(m, n) rows of words(k) words padded to an odd count,
 * a row index of max(m, n) and a table of min(m, n) int32 entries, each rounded up to 16 bytes, 16 bytes of flags and a word per
 * row of A, within 160 KiB -- only B is staged, so the boundary lies above m4ri_amd_plan_solve_batch's); 2 members one by one through
 * m4ri_amd_pluq_solve_left_dev on scratch copies (blocking) */
int m4ri_amd_plan_pluq_solve_batch(int64_t m, int64_t n, int64_t k);
/* Device twin of mzd_apply_p_right{,_trans} (echelon.hip): the column transpositions (i, P[i]), i < min(length, ncols),
 * descending (trans == 0, A * P) or ascending (A * P^T), on every row.  P: HOST array.  Blocking.  Whole words from the first to
 * the last word that holds a moved column are rewritten: bits at column >= ncols zero in, zero out; the words from the width to
 * `stride` and other rows never written.  Rows up to 64 KiB wide are staged in LDS, wider ones gathered from a copy in global
 * memory, 4096 rows at a time.  hipErrorInvalidValue, before any HIP call, for negative sizes, P == NULL or an entry of P outside
 * the columns. */
int m4ri_amd_apply_p_right_dev(word *A, int64_t stride, int64_t nrows, int64_t ncols, const int32_t *P, int64_t length, int trans, void *stream);
/* Row r <- its columns under the transpositions (i, Q[i]), i = r+1 .. ncols-1 ascending (mzd_apply_p_right_trans_tri,
 * m4ri/mzp.c:279-293).  Q: HOST array, ncols entries, Q[i] >= i.  Blocking.  Whole words of the rows 0 .. nrows-1 are
 * rewritten, from the row's diagonal word to the last word that holds a moved column: bits at column >= ncols zero in, zero
 * out; the words from the width to `stride` and other rows are never written.  hipErrorInvalidValue, before any HIP call, for
 * negative sizes, Q == NULL or an entry Q[i] outside i .. ncols-1. */
int m4ri_amd_apply_p_right_trans_tri_dev(word *A, int64_t stride, int64_t nrows, int64_t ncols, const int32_t *Q, void *stream);
/* Deterministic fill: word (r, j) = splitmix64 stream `seed`, output number r*width + j, last word
 * masked -- the order mzd_randomize_custom fills a matrix in (mzd.c:1282-1292). */
int m4ri_amd_fill_dev(word *M, int64_t stride, int64_t rows, int64_t ncols, uint64_t seed, void *stream);
/* Clears the bits at column >= ncols of word words(ncols)-1 of each of the `rows` rows and writes nothing else (ncols a multiple
 * of 64: nothing at all).  Asynchronous on `stream`. */
int m4ri_amd_mask_tail_dev(word *M, int64_t stride, int64_t rows, int64_t ncols, void *stream);

/* Schedule statistics of the most recent m4ri_amd_mul_dev / m4ri_amd_m4rm_dev on this thread's
 * engine.  With profiling on, every leaf launch is bracketed by HIP events on its own stream and
 * leaf_ms is their sum (reading it synchronises the stream). */
typedef struct m4ri_amd_stats {
  int32_t levels;           /* Strassen-Winograd levels used                       */
  int32_t leaf_launches;    /* kernel launches of the M4RM leaf                     */
  int64_t leaf_products;    /* products those launches computed (batch members)     */
  int32_t leaf_m, leaf_l, leaf_n; /* shape of the batched leaves                     */
  int32_t leaf_gen;         /* generation of the leaf kernel used: 1 m4rm_leaf,
                               4 m4rm8q, 5 m4rm_small (small products, one launch)  */
  double leaf_ms;           /* sum of leaf launch durations (profiling on), else 0  */
  double leaf_bytes;        /* algorithmic bytes of the leaf launches:
                               8*(m*W(l) + l*W(n) + m*W(n)) per product             */
  double aux_bytes;         /* declared bytes of the fused down/up passes           */
  double workspace_bytes;   /* HBM held by the engine's workspace                   */
  double cum_leaf_ms;       /* cumulative profiling (mode 2): leaf time of ALL products since it was
                               switched on, and how many launches that was           */
  int64_t cum_leaf_launches;
} m4ri_amd_stats;
/* 0: off.  1: the stats describe the most recent product only.  2: additionally cum_leaf_ms /
 * cum_leaf_launches accumulate over all products until profiling is set again (no host
 * synchronisation happens until m4ri_amd_get_stats is called). */
void m4ri_amd_set_profiling(int on);
int m4ri_amd_get_stats(m4ri_amd_stats *out);

/* Strassen-Winograd levels the engine uses for an m x l x n product and this cutoff (pure host
   logic, callable without a GPU): cutoff > 0 follows the reference's rule (strassen.c:39,51 --
   halve while no dimension satisfies 3*dim < 4*cutoff, cutoff rounded down to a multiple of 64),
   cutoff == 0 the engine's own plan: the depth a small time model of the schedule gives the first
   (largest) block of rows -- see m4ri_amd_plan_row_blocks; both capped so that every level still
   halves whole words. */
int m4ri_amd_plan_levels(int64_t m, int64_t l, int64_t n, int cutoff);

/* The engine's own plan for an m x l x n product (cutoff == 0), pure host logic: the rows of A and C
   in blocks, largest first, each multiplied by B as a product of its own at its own depth (the leaf's
   tile is 4096 rows: 65664 = 65536 + 128 rows run as a four-level product and a thin one instead of
   one level over rows that do not tile).  Writes the first `cap` blocks to rows[] / levels[] (either
   may be NULL) and returns the number of blocks of the plan. */
int m4ri_amd_plan_row_blocks(int64_t m, int64_t l, int64_t n, int64_t *rows, int *levels, int cap);

/* Does a direct (no Strassen level) product of `batch` members of this shape take the one-launch small leaf (m4rm_small.hip), and with
   how many inner-dimension splits?  0: no (generation 4 / 1); k >= 1: yes, k splits (k > 1: the splits meet by atomic XOR).  `cus`: the
   compute units the launch is planned for (0 = 256, an MI355X).  Pure host arithmetic, callable without a GPU. */
int m4ri_amd_plan_small_leaf(int64_t m, int64_t l, int64_t n, int64_t batch, int cus);

/* What ONE leaf launch of the engine does for `batch` products of m x l x n -- the launch every direct product and every Strassen leaf
   level ends in (engine.hip launch_leaf_one runs exactly this plan and decides nothing itself):
     gen          5 the one-launch small leaf (256 x 8 word tiles), 4 packed A (4096 x 8), 1 plain A (32 rg x 32); 0: no kernel runs
                  (an empty product, or l == 0: C is cleared or kept)
     rg           generation 1: tile rows / 32 (32, 24 or 16); else 0
     tile_rows, tile_words, tiles_m, tiles_n, tiles   the tile grid of one member and the tiles of the whole launch
     ksplit       inner-dimension splits handed to the kernel of the whole launch (hybrid plan: of its head, 1).  Generation 4: the
                  count the kernel really makes (whole stage pairs per split); generations 1 and 5 round the count in their launchers
     tail_tiles, tail_ksplit   hybrid plan (generation 4): the last tail_tiles tiles -- those of the short last round -- go in a second
                  launch with this split; 0 and 1 otherwise
     mode, tail_mode   how the launch (the tail launch) writes C: 0 store, 1 atomic XOR into C, 2 slabs + one reduce pass (tail_mode is 0
                  without a tail)
     slabs        1: the splits meet in slabs of the workspace and one reduce pass writes (add: XORs into) C; 0: by atomic XOR, or unsplit
     zero         what is cleared first: 0 nothing, 1 all of C (every member's m rows of words(n) words), 2 the tail's tiles
     pack_a       1: a separate pass packs A for generation 4 first (0 when a fused pass has: a_prepacked)
   ksplit_req: what the caller asks for (m4ri_amd_m4rm_dev's ksplit; 0 = automatic, every other entry).  cus: the compute units planned
   for (0 or less: 256, an MI355X).  a_prepacked: the fused down pass has written A in packed form (Strassen leaves).  scratch_ok: the
   engine's packed-A scratch and slab region hold this launch -- every entry reserves them first, except m4ri_amd_m4rm_batch_dev, which
   takes what the previous call left and falls back to generation 1 when that is too small.  The developer switches M4RI_AMD_LEAF_GEN,
   M4RI_AMD_SMALL_LEAF, M4RI_AMD_SMALL_LEAF_WORK, M4RI_AMD_SMALL_KS and M4RI_AMD_TAIL_KSPLIT are read as the engine reads them, so the
   answer is what THIS process would do.  Pure host arithmetic, callable without a GPU.  Returns 0, or hipErrorInvalidValue (1) for
   out == NULL, a negative size, a dimension beyond INT32_MAX, or a_prepacked on a launch generation 4 cannot take. */
typedef struct m4ri_amd_leaf_plan {
  int32_t gen, rg;
  int32_t tile_rows, tile_words;
  int64_t tiles_m, tiles_n, tiles;
  int32_t ksplit, tail_ksplit;
  int64_t tail_tiles;
  int32_t mode, tail_mode;
  int32_t slabs, zero, pack_a, reserved;
} m4ri_amd_leaf_plan;
int m4ri_amd_plan_leaf_launch(int64_t m, int64_t l, int64_t n, int64_t batch, int add, int ksplit_req, int cus, int a_prepacked, int scratch_ok,
                              m4ri_amd_leaf_plan *out);
/* What the engine's time model gives ONE m x l x n product at `levels` Strassen-Winograd levels, in seconds on the box the
   constants were measured on (the plans above are minima of sums of it; tools/depth_model_sweep.py prints it beside measurements). */
double m4ri_amd_model_seconds(int64_t m, int64_t l, int64_t n, int levels);

/* Bytes the breadth-first schedule's workspace may take (0 = automatic: what the device has left).
   Levels that do not fit run depth-first, one sub-product after the other, like the reference's
   recursion -- same bits.  Returns the previous value; negative arguments only query. */
int64_t m4ri_amd_set_workspace_budget(int64_t bytes);

/* How many of the deepest Strassen-Winograd levels one fused pass covers each way (1..4, default 4;
   a scheduling knob: results are bit-identical for every value).  Returns the previous value;
   out-of-range arguments only query. */
int m4ri_amd_set_max_fuse(int levels);

/* The M4RI-named products pipeline a large product from host memory over four row slabs of A and C (upload of
   slab k+1 and download of slab k-1 under product k; same bits).  min_bytes: size of A + B + C from which that
   happens (default 64 MiB; 0 = never).  Returns the previous value; negative arguments only query. */
int64_t m4ri_amd_set_host_pipeline(int64_t min_bytes);
/* The plan of that pipeline for an m x l x n product (mzd_api.hip run_pipelined executes it and decides nothing itself), pure host
   arithmetic, callable without a GPU.  min_bytes: the threshold above.  gi, gj, gk: a requested block grid (M4RI_AMD_PIPE_GRID; 0, 0, 0
   for none); a request the shape has not the rows (gi x 4096), columns (gj x 64) or inner bits (gk x 64) for counts as none.  Returns 0
   when the product is not pipelined; else 1, with the blocks  C_ij (+)= A_ik * B_kj  lying between the cuts written to rcut[], ccut[],
   kcut[] (each may be NULL; each list runs from 0 to its dimension), their numbers gi, gj, gk to grid[3] and the words of the staging
   arena the blocks of A, B and C take to *arena_words; or -1, with only grid[] and *arena_words written, when a list has more than
   `cap` entries. */
int m4ri_amd_plan_host_pipeline(int64_t m, int64_t l, int64_t n, int64_t min_bytes, int gi, int gj, int gk, int64_t *rcut, int64_t *ccut,
                                int64_t *kcut, int cap, int *grid, int64_t *arena_words);

/* Small products.  The reference switches algorithm by size inside the functions this library replaces (_mzd_mul_m4rm -> mzd_mul_naive
   below 54 columns / 16 rows, m4ri/brilliantrussian.c:1063-1068, m4ri/mzd.c:1141-1172); here the switch sits where a call's upload,
   launches and download (28 ... 80 us whatever the size) stop paying: a product with m * l * n at or below the threshold whose
   matrices live in host memory is computed by the library's own host Method of Four Russians (small_host.cpp) on the calling
   thread -- on an initialised device, never instead of one: without a GPU the entry points still abort.  Default 2^27; 0 sends
   every product to the GPU; returns the previous value, negative arguments only query.  The routine's own cost is bounded as well
   (threshold / 240 word operations of its algorithm, 39 us at the default: 512^3 -- 31 us on the host, 40 through the GPU -- is the
   largest cube it takes, and degenerate shapes such as 1 x 1 x 2^26 go to the GPU whatever m * l * n says);
   m4ri_amd_small_product_wanted is that rule (pure arithmetic, no GPU: 1 = the host routine would take this product).  The device
   lock is released while the routine runs: small products of many threads run side by side.  m4ri_amd_small_product_count: how
   many products took that path.  m4ri_amd_small_mul_host is the routine itself: C (+)= A * B on host mzd_t (windows allowed, the
   bits outside C's columns kept); returns 0, or -1 on mismatched dimensions. */
int64_t m4ri_amd_set_small_product_threshold(int64_t ops);
int64_t m4ri_amd_small_product_count(void);
int m4ri_amd_small_product_wanted(int64_t m, int64_t l, int64_t n);
int m4ri_amd_small_mul_host(mzd_t *C, const mzd_t *A, const mzd_t *B, int add);

/* Release the engine's workspace (device memory pool) and the host entry points' staging arena;
   pinned matrices keep their device copies. */
void m4ri_amd_release_workspace(void);

/* ---- part 3: residency (device-resident matrix handles) -----------------------------
 * Opt-in, for programs that chain products (TRSM / PLE Schur complements: triangular.c:100,348,439,
 * 503, ple.c:126 call mzd_addmul on windows of the same few matrices).  A pinned matrix keeps a device
 * copy in the host layout; the M4RI-named entry points of part 1 then read pinned operands -- and
 * windows (mzd_init_window) into them -- where they are, and leave a pinned result on the device: no
 * PCIe traffic at all when everything is pinned.  The host copy of a pinned matrix that received a
 * result is STALE until m4ri_amd_sync or m4ri_amd_unpin; the host must not modify a pinned matrix
 * without telling (m4ri_amd_host_modified).  Unpin before mzd_free.  All return 0 on success, -1 if
 * M is NULL / a window / empty (pin) or not pinned (the others). */
int m4ri_amd_pin(mzd_t *M);            /* M owns its block (not a window): upload it now               */
int m4ri_amd_sync(mzd_t *M);           /* bring the host copy up to date (M or a window into it)        */
int m4ri_amd_host_modified(mzd_t *M);  /* the host wrote into M: refresh the device copy               */
int m4ri_amd_unpin(mzd_t *M);          /* sync, then drop the device copy                               */
int m4ri_amd_is_pinned(const mzd_t *M);/* 0 no, 1 yes and host copy current, 2 yes and host copy stale  */

/* ---- part 4: one product over several GPUs (m4ri/mp.c:158-324 is the reference's own
 * block-parallel template) ------------------------------------------------------------------------------
 * The units handed out are the sub-products of the top Strassen level(s) (strassen.c:111-150): 7 (levels = 1), or
 * (levels = 2) the 47 of ONE application of the rank-47 scheme of the 4 x 4 x 4 block product (scheme444.h) -- 49 of
 * Strassen-Winograd twice where the scheme's passes cannot take the slabs (children narrower than 64 words).  Layout: with S = 2^levels row blocks per matrix,
 * rank r of `world` holds rows [cut(r), cut(r+1)) of EVERY block ("slab-cyclic"; cut(r) = rows*r/world),
 * stacked into a local parent of 1/world of the rows and the same quadrant structure -- so the level's
 * additions are ordinary local passes and only slabs of sub-product operands (one way) and of products
 * (the other) cross the links, every rank to every rank.  Dimensions are zero-padded (M, L, N). */
typedef struct m4ri_amd_shard_plan {
  int32_t world, levels, nprod, blocks; /* ranks; sharded levels (1|2); sub-products: 7, 49 or -- two levels as ONE application of the
                                           rank-R scheme of the 4 x 4 x 4 block product, where its passes take the slabs -- R = 47; 2^levels */
  int64_t m, l, n;                      /* the product C (m x n) = A (m x l) * B (l x n)                */
  int64_t M, L, N;                      /* padded: M % blocks == 0, L and N % (64*blocks) == 0          */
  int64_t bm, bl;                       /* rows of a sub-product's A operand (= of its result), of its B */
  int64_t cwl, cwn;                     /* words per row of an A child; of a B child / a product        */
} m4ri_amd_shard_plan;
/* One slab of one sub-product operand (side 0: A child, 1: B child) or result (side 2): it lives at
 * holder_off words into rank `holder`'s child / slab array and at owner_off words into rank `owner`'s
 * operand / product array; sides 0, 1 travel holder -> owner, side 2 owner -> holder. */
typedef struct m4ri_amd_shard_piece {
  int32_t holder, owner;
  int64_t holder_off, owner_off, words;
} m4ri_amd_shard_piece;
enum { M4RI_AMD_SHARD_BUF_LOCAL_A = 0, M4RI_AMD_SHARD_BUF_LOCAL_B, M4RI_AMD_SHARD_BUF_LOCAL_C, /* local parents (stride L/64, N/64, N/64) */
       M4RI_AMD_SHARD_BUF_CHILD_A, M4RI_AMD_SHARD_BUF_CHILD_B, M4RI_AMD_SHARD_BUF_SLABS_P,      /* nprod slabs each, back to back         */
       M4RI_AMD_SHARD_BUF_OPER_A, M4RI_AMD_SHARD_BUF_OPER_B, M4RI_AMD_SHARD_BUF_PROD };         /* whole operands/results of owned j's    */
/* Pure host arithmetic (no GPU needed).  levels: 1, 2 or 0 = automatic.  0 on success. */
int m4ri_amd_shard_plan_make(m4ri_amd_shard_plan *p, int world, int64_t m, int64_t l, int64_t n, int levels);
int64_t m4ri_amd_shard_cut(int64_t rows, int world, int r);
int m4ri_amd_shard_owner(const m4ri_amd_shard_plan *p, int j);             /* rank that multiplies sub-product j */
/* how many of its sub-products a rank multiplies as ONE batched product (m4ri_amd_mul_batch_dev): rounds q, q + 1, ... of a group go
 * together -- by the engine's time model, the smallest group within 5 % of the best; 1 = one sub-product at a time.  Host arithmetic. */
int m4ri_amd_shard_group(const m4ri_amd_shard_plan *p, int cutoff);
int64_t m4ri_amd_shard_slab_rows(const m4ri_amd_shard_plan *p, int rank, int which); /* 0: of A/C/products, 1: of B */
int64_t m4ri_amd_shard_buffer_words(const m4ri_amd_shard_plan *p, int rank, int which);
int m4ri_amd_shard_piece_of(const m4ri_amd_shard_plan *p, int side, int j, int r, m4ri_amd_shard_piece *out);
/* Per-rank device steps (asynchronous on `stream`; one process per GPU moves the pieces itself, e.g. with
 * RCCL send/recv): local parents -> slabs of all children; slabs of all products -> local parent of C.
 * The sub-products themselves are plain m4ri_amd_mul_dev calls of bm x bl x (64*cwn). */
int m4ri_amd_shard_down_dev(const m4ri_amd_shard_plan *p, int rank, const word *A_local, int64_t a_stride, const word *B_local,
                            int64_t b_stride, word *child_a, word *child_b, void *stream);
int m4ri_amd_shard_up_dev(const m4ri_amd_shard_plan *p, int rank, const word *slabs_p, word *C_local, int64_t c_stride, int add,
                          void *stream);
/* Rows [row0, row0 + rows) of the matrix m4ri_amd_fill_dev(seed) would fill, written to M (for filling
 * local parents of a distributed matrix without materialising the whole). */
int m4ri_amd_fill_rows_dev(word *M, int64_t stride, int64_t row0, int64_t rows, int64_t ncols, uint64_t seed, void *stream);
/* ---- one process, all devices: distributed device-resident matrices ----------------------------------
 * The reference's multi-core entry is a C function (mzd_mul_mp, m4ri/mp.c:158-297), so the multi-GPU schedules sit
 * behind this boundary.  A m4ri_amd_dmat is a matrix spread over the configured devices (m4ri_amd_set_devices) and
 * resident in HBM; products leave their result distributed, so they chain without PCIe traffic.  Layouts (every
 * dimension zero-padded to 256 bits in the local buffers, one row stride for all layouts of a matrix):
 *   ROWS        rank r holds rows [r k, (r+1) k), k = ceil(rows / W)            -- the row-slab schedule
 *   CYCLIC1/2   slab-cyclic over the 2 / 4 row blocks of 1 / 2 Strassen-Winograd levels (above)
 *   REPLICATED  every rank holds the whole matrix (a B that needs no gather)
 * Schedules (m4ri_amd_dmat_mul, `variant`): M4RI_AMD_VARIANT_SLABS -- C_r = A_r * B, B's row slabs gathered by peer
 * copies under the product with the rank's own slab (no reduction; SURVEY.md 8e "rectangular"); M4RI_AMD_VARIANT_STRASSEN
 * -- the sub-products of the top Strassen level(s), operand and result slabs pulled by hipMemcpyPeerAsync on copy streams
 * under the products (row chunks).  0 = by the operands' layout, else by shape and world size
 * (m4ri_amd_multi_default_variant: slabs up to 4 ranks and for every product a Strassen level cannot help, e.g.
 * 131072 x 8192 x 131072).  One host thread per rank issues the work; all calls but _mul are blocking, _mul is
 * asynchronous (m4ri_amd_multi_sync).  Return 0 or a hipError_t value unless noted. */
enum { M4RI_AMD_LAYOUT_ROWS = 0, M4RI_AMD_LAYOUT_CYCLIC1 = 1, M4RI_AMD_LAYOUT_CYCLIC2 = 2, M4RI_AMD_LAYOUT_REPLICATED = 3 };
enum { M4RI_AMD_VARIANT_AUTO = 0, M4RI_AMD_VARIANT_SLABS = 1, M4RI_AMD_VARIANT_STRASSEN = 2 };
typedef struct m4ri_amd_dmat m4ri_amd_dmat;
typedef struct m4ri_amd_dmat_info_t {
  int64_t rows, ncols, stride;  /* stride: words of a local row */
  int32_t layout, world, alive; /* alive == 0: the device list changed since the matrix was made -- only _free is valid */
} m4ri_amd_dmat_info_t;
m4ri_amd_dmat *m4ri_amd_dmat_create(int64_t rows, int64_t ncols, int layout);  /* zero matrix; NULL on failure */
void m4ri_amd_dmat_free(m4ri_amd_dmat *d);
int m4ri_amd_dmat_info(const m4ri_amd_dmat *d, m4ri_amd_dmat_info_t *out);
/* device pointer, rows (padding included) and HIP device of rank `rank`'s local buffer */
int m4ri_amd_dmat_local(const m4ri_amd_dmat *d, int rank, word **data, int64_t *local_rows, int *device);
int m4ri_amd_dmat_fill(m4ri_amd_dmat *d, uint64_t seed);                /* the matrix m4ri_amd_fill_dev(seed) fills, distributed */
int m4ri_amd_dmat_upload(m4ri_amd_dmat *d, const mzd_t *M);             /* every device its own rows over its own PCIe link */
int m4ri_amd_dmat_download(const m4ri_amd_dmat *d, mzd_t *M);           /* a windowed M keeps the bits outside its columns */
int m4ri_amd_dmat_convert(m4ri_amd_dmat *dst, const m4ri_amd_dmat *src); /* dst <- src, any two layouts (ROWS -> REPLICATED = all-gather) */
int m4ri_amd_dmat_mul(m4ri_amd_dmat *C, const m4ri_amd_dmat *A, const m4ri_amd_dmat *B, int add, int cutoff, int variant);
/* The same on lane `lane` (0 or 1): every lane has its own streams, events and arenas on every device, and products of different
 * lanes do not wait for each other -- two INDEPENDENT products (different C, neither C an operand of the other) issued
 * alternately on lanes 0 and 1 keep two in flight: the operand and result transport of one under the multiplications of the
 * other (on a device the multiplications themselves take turns: one engine workspace).  Everything that is not a product
 * (fill, upload, convert, download) runs on lane 0 behind the last operation of EVERY lane, and the first product of a lane after
 * such an operation waits for it.  m4ri_amd_dmat_mul == lane 0. */
int m4ri_amd_dmat_mul_lane(m4ri_amd_dmat *C, const m4ri_amd_dmat *A, const m4ri_amd_dmat *B, int add, int cutoff, int variant, int lane);
int m4ri_amd_multi_sync(void);
/* First contact with DIFFERENT devices (the first call that configures the ranks): peer access is enabled pair by pair, then every
 * ordered pair makes one 1 MiB copy behind one cross-device event wait and checks the data; a failure prints the pair and the HIP
 * error and fails the call before any product is scheduled.  Pairs without peer access copy through pinned host memory instead
 * (m4ri_amd_multi_stats.pairs_staged counts them).  Environment, for tests on one GPU: M4RI_AMD_SELFTEST_PAIRS=1 runs the self-test
 * between ranks of one device too; M4RI_AMD_NO_PEER="all" | "i-j,k-l" treats these rank pairs as having no peer access.
 * m4ri_amd_multi_pair_table is the pure rule (no GPU): staged[dst * world + src] from the ranks' devices, the ndev x ndev table
 * can_access[d * ndev + e] (hipDeviceCanAccessPeer) and that hook. */
void m4ri_amd_multi_pair_table(int world, const int *devices, int ndev, const int *can_access, const char *no_peer_spec, char *staged);
/* The links, measured over the ranks' own link streams: `bytes` copied dst <- src for every ordered pair of ranks one at a time
 * (pair_gbs[dst * W + src] in GB/s) and all pairs at once (*all_gbs: all bytes / wall time); staged[] as above; *same_device = 1 when
 * ranks share a device (those pairs report the on-device copy rate).  all_gbs, staged, same_device may be NULL. */
int m4ri_amd_multi_link_probe(int64_t bytes, double *pair_gbs, double *all_gbs, char *staged, int *same_device);
/* what the most recent m4ri_amd_dmat_mul / m4ri_amd_mul_multi / mzd_mul_mp did */
typedef struct m4ri_amd_multi_stats {
  int32_t world, variant, levels, sub_products; /* variant: M4RI_AMD_VARIANT_*; levels / sub_products: Strassen schedule   */
  int32_t chunks, overlap, converted;           /* row chunks per sub-product; slabs: gather under the first product;       */
  int32_t pairs_staged;                         /* operands converted to the schedule's layout first (0 on the fast path);  */
                                                /* ordered rank pairs that copy through the host (no peer access)           */
  int64_t m, l, n;
  double link_bytes;                            /* bytes that crossed between ranks                                          */
  int32_t group, reserved;                      /* Strassen schedule: sub-products of a rank multiplied as one batched product */
} m4ri_amd_multi_stats;
int m4ri_amd_multi_get_stats(m4ri_amd_multi_stats *out);
/* Marks of rank `rank`'s part of the most recent m4ri_amd_dmat_mul, ms after its compute stream entered the operation
 * (synchronises first).  Strassen: down pass done; per unit (round, row chunk): operands in, product done; result slabs
 * in; up pass done.  Slabs: gather done; first product done; all done.  Returns the number of marks, < 0 on error. */
int m4ri_amd_multi_timeline(int rank, double *ms, int cap);
/* Pure host arithmetic (no GPU needed): the schedule a product takes, the layout that schedule wants, and the geometry
 * of a layout -- rows of rank `rank`'s local buffer; its runs of valid global rows (global first row, rows, local first
 * row; returns their number, at most 4). */
int m4ri_amd_multi_default_variant(int world, int64_t m, int64_t l, int64_t n);
int m4ri_amd_multi_layout_for(int variant, int world, int64_t m, int64_t l, int64_t n);
int64_t m4ri_amd_layout_local_rows(int layout, int world, int rank, int64_t rows);
int m4ri_amd_layout_runs(int layout, int world, int rank, int64_t rows, int64_t *g0, int64_t *nrows, int64_t *l0, int cap);
/* Force a schedule for m4ri_amd_mul_multi / mzd_mul_mp and for m4ri_amd_dmat_mul on operands whose layouts fit none
 * (0 automatic, M4RI_AMD_VARIANT_SLABS, M4RI_AMD_VARIANT_STRASSEN); returns the previous value, others only query. */
int m4ri_amd_set_multi_variant(int variant);
/* One process, several devices, HOST matrices: C (+)= A*B = upload into distributed temporaries (kept between calls) +
 * m4ri_amd_dmat_mul + download.  levels: 0 = automatic schedule (above), 1 / 2 = the Strassen schedule with that many
 * sharded levels.  What mzd_mul_mp / mzd_addmul_mp run for large products.  Returns 0 or a hipError_t value. */
int m4ri_amd_mul_multi(mzd_t *C, const mzd_t *A, const mzd_t *B, int add, int cutoff, int levels);
/* The devices mzd_mul_mp / m4ri_amd_mul_multi / the distributed matrices are spread over.  Default: the comma-separated
 * list in the environment variable M4RI_AMD_DEVICES, else every visible device.  An id may repeat (several ranks
 * on one GPU: how the tests exercise the path on a one-GPU box).  n == 0 restores the default. */
int m4ri_amd_set_devices(int n, const int *ids);
int m4ri_amd_get_device_list(int *ids, int cap);
/* Smallest min(m, l, n) that mzd_mul_mp / mzd_addmul_mp spread over several devices (default 16384);
 * returns the previous value, negative arguments only query. */
int64_t m4ri_amd_set_multi_threshold(int64_t min_dim);

#ifdef __cplusplus
}
#endif
#endif /* M4RI_AMD_H */
