// solve_batch.hip -- linear solves A_b X_b = B_b, inverses A_b^-1 and null-space bases of many independent small matrices, one launch
// for the batch.
//
// All three are Gauss-Jordan: on an augmented member [A | B] for the solve, [A | I] for the inverse, on A alone for the null space
// (the op, SB_SOLVE / SB_INV / SB_KER, is the kernels' template argument), with echelon_batch.hip's pivot rule
// (columns left to right, the pivot of a column is the first row at or below the rank with the bit set, swapped up to the rank's
// row) and a full update (every other row with the bit).
//   solve:   the pivot search runs over A's n columns only.  Afterwards the rows at and below the rank have no bit of A left, so
//            the system is consistent iff their B part is zero; X row c = the B part of the row whose pivot is column c, and zero
//            for the non-pivot columns.  That is the solution with its free variables zero, the one PLUQ's Q gives
//            m4ri_amd_solve_left_dev, because the pivot columns are A's column rank profile either way.
//   inverse: the search runs over all 2n columns, so the member ends in the reduced echelon form of [A | I], which is unique: its
//            right half is m4ri_amd_inv_dev's result, for singular members too.
//   kernel:  the search runs over A's n columns; the member ends in the reduced echelon form E of A with pivot columns
//            p_0 < ... < p_{r-1}.  mzd_kernel_left_pluq's basis (solve.c:154-191) depends on E alone: pos = [0 .. n-1], swap pos[i]
//            and pos[p_i] for i = 0 .. r-1 ascending (PLUQ's Q; behind the rank Q is the identity at these sizes), the free
//            columns in basis order are f_j = pos[r + j], and column j of the basis has a 1 in row f_j and E[i][f_j] in row p_i.
// For the solve and the inverse A is padded with zero rows to R = max(m, n) rows (the solve's B has R rows); the kernel keeps R = m.
// The paths (m4ri_amd_plan_solve_batch, m4ri_amd_plan_kernel_batch):
//   0  R <= 64 and k <= 64: a wave per member, lane i holds row i of A and of B (the identity's bit made in a register); pivot = the
//      lowest lane >= rank of a ballot, the pivot row's words by readlane; X gathered by ds_bpermute.  No LDS, no barrier.
//   1  the augmented member fits in LDS: a workgroup per member, batch_common.h's scheme with the rows in LDS (rows under a row
//      index, the swap of a column as two index entries, a flag pass and ballot per column).
//   2  larger members one by one through the per-member calls on scratch copies, then one copy of statuses and ranks.  Blocking.
// Paths 0 and 1 are one launch each (plus chunking above 2^30 workgroups), no allocation, no copy, no host synchronisation.
// Memory rules: A is never written (except as Binv in place); bits at columns >= k (resp. n, kc) of a row's last word of B / Binv /
// the basis, the words from the width to the stride of a row and anything between members are never written.  An inconsistent
// member's B is not written at all.
#include <hip/hip_runtime.h>
#include <vector>
#include "batch_common.h"
#include "../../include/m4ri_amd.h"

namespace {

constexpr int SB_SOLVE = 0, SB_INV = 1, SB_KER = 2;    // the op: X of [A | B], the inverse from [A | I], a null-space basis of A

// path 0: a wave per member, lane i = row i of A (a) and of B or the identity (x, zero for the kernel), one word each.  Members
// b0 + 4 * blockIdx.x + wave.  The kernel's B is the basis R (n x k).
template <int OP>
__global__ __launch_bounds__(BATCH_WAVE_THREADS) void sb_wave_kernel(const word *A, int64_t a_stride, int64_t a_bs, word *B,
                                                                     int64_t b_stride, int64_t b_bs, int m, int n, int k, int64_t b0,
                                                                     int64_t batch, int32_t *__restrict__ status, int32_t *__restrict__ rank_out) {
  constexpr bool INV = OP == SB_INV, AUG = OP != SB_KER;
  const int lane  = threadIdx.x & 63;
  const int64_t b = b0 + (int64_t)blockIdx.x * (BATCH_WAVE_THREADS / 64) + (threadIdx.x >> 6);
  if (b >= batch) return;  // wave-uniform, no barrier in this kernel
  const int R      = m > n ? m : n;
  const word amask = tail_mask(n), bmask = tail_mask(k);
  word *gb         = B + b * b_bs;
  word a = 0, x = 0, orig = 0;
  if (lane < m && n > 0) a = A[b * a_bs + (int64_t)lane * a_stride] & amask;
  if (AUG && lane < (INV ? n : R) && k > 0 && (!INV || bmask != ~(word)0)) orig = gb[(int64_t)lane * b_stride];  // the inverse: tail bits only
  if (INV) x = lane < n ? (word)1 << lane : 0;
  else if (AUG) x = orig & bmask;
  // (Binv == A in place: every lane has loaded its row before any store below)
  int rank = 0;
  word pivcols = 0;  // bit c: column c < n has a pivot (wave-uniform)
  for (int c = 0; c < (INV ? 2 * n : n) && rank < m; ++c) {
    const int bit   = (int)(((INV && c >= n) ? (x >> (c - n)) : (a >> c)) & 1);
    const word cand = __ballot(bit) & (~(word)0 << rank);
    if (!cand) continue;
    const int p    = (int)__builtin_ctzll(cand);
    const word pa  = readlane64(a, p), px = AUG ? readlane64(x, p) : 0;
    if (bit && lane != p) {
      a ^= pa;
      x ^= px;
    }
    const word ra = readlane64(a, rank), rx = AUG ? readlane64(x, rank) : 0;  // row `rank` has no bit c unless it is the pivot: not updated
    if (lane == rank) {
      a = pa;
      x = px;
    } else if (lane == p) {
      a = ra;
      x = rx;
    }
    if (c < n) pivcols |= (word)1 << c;
    ++rank;
  }
  if (OP == SB_KER) {
    // The swap rule with lane l following the column that starts at position l (q: where it is), lane i < rank taking p_i.  Then
    // free column f is basis column q - rank of lane f: row f of R is that bit, row p_i (lane i) gathers E's bits at the free
    // columns.  Every row of R is stored once, by lane f or by lane i.
    int q = lane, pi = 0;
    word rest = pivcols;
    for (int i = 0; rest; ++i, rest &= rest - 1) {
      const int p = (int)__builtin_ctzll(rest);
      if (q == i) q = p;
      else if (q == p) q = i;
      if (lane == i) pi = p;
    }
    const word freecols = n > 0 ? ~pivcols & amask : 0;
    word y = 0;
    for (word fr = freecols; fr; fr &= fr - 1) {
      const int f = (int)__builtin_ctzll(fr), j = __builtin_amdgcn_readlane(q, f) - rank;
      if (j < k) y |= ((a >> f) & 1) << j;
    }
    if (k > 0) {
      if (lane < rank) {
        word *dst = gb + (int64_t)pi * b_stride;
        *dst      = bmask == ~(word)0 ? y : (y & bmask) | (*dst & ~bmask);
      }
      if ((freecols >> lane) & 1) {
        const int j = q - rank;
        const word v = j < k ? (word)1 << j : 0;
        word *dst    = gb + (int64_t)lane * b_stride;
        *dst         = bmask == ~(word)0 ? v : (v & bmask) | (*dst & ~bmask);
      }
    }
    if (lane == 0) rank_out[b] = rank;
    return;
  }
  if (INV) {
    if (lane < n) gb[(int64_t)lane * b_stride] = (x & bmask) | (orig & ~bmask);
    if (lane == 0 && rank_out) rank_out[b] = __builtin_popcountll(pivcols);
    return;
  }
  // rows >= rank have no bit of A left: consistent iff their B words are zero
  const bool bad = __ballot(lane >= rank && x != 0) != 0;
  if (!bad) {
    // X row i (i a pivot column) = B word of the row whose pivot it is: pivots ascend with the rows, so that row is the number of
    // pivot columns below i.  Non-pivot rows and rows n .. R-1 are zero.
    const int src = __builtin_popcountll(pivcols & (((word)1 << lane) - 1));
    word y        = bpermute64(x, src);
    if (!((pivcols >> lane) & 1)) y = 0;
    if (lane < R && k > 0) gb[(int64_t)lane * b_stride] = (y & bmask) | (orig & ~bmask);
  }
  if (lane == 0) {
    status[b] = bad ? -1 : 0;
    if (rank_out) rank_out[b] = rank;
  }
}

// path 1: a workgroup per member.  Dynamic LDS (16-byte carve offsets):
//   rows [R][ldw] words (wa words of A, then wb of B or the identity; the kernel: wa only, R = m) | perm [R] int32 (rounded up to
//   16 B) | flags [2][nfw] words | pivcols [nfw] words (bit c: column c < n has a pivot; nfw = ceil(max(R, n) / 64)) | the kernel
//   only: pos [n] int32 (the swap rule's arrangement) | idx [n] int32 (a pivot column's pivot row, a free column's basis column)
// Row i of the flag pass is owned by thread i % blockDim.x (the lane of its ballot); flags[c & 1] bit i = bit c of logical row i.
template <int OP>
__global__ __launch_bounds__(BATCH_MAX_THREADS) void sb_block_kernel(const word *A, int64_t a_stride, int64_t a_bs, word *B,
                                                                     int64_t b_stride, int64_t b_bs, int m, int n, int k, int ldw, int64_t b0,
                                                                     int32_t *__restrict__ status, int32_t *__restrict__ rank_out) {
  constexpr bool INV = OP == SB_INV;
  extern __shared__ __attribute__((aligned(16))) char sb_smem[];
  const int T = blockDim.x, t = threadIdx.x, lane = t & 63;
  const int64_t b  = b0 + blockIdx.x;
  const word *ga   = A + b * a_bs;
  word *gb         = B + b * b_bs;
  const int R      = (OP == SB_KER || m > n) ? m : n;
  const int wa     = (n + 63) >> 6, wb = OP == SB_KER ? 0 : (k + 63) >> 6, W = wa + wb;
  const int rfw    = (R + 63) >> 6, nfw = ((R > n ? R : n) + 63) >> 6;  // flag words of the rows; words of the flag and pivot buffers
  const word amask = tail_mask(n), bmask = tail_mask(k);
  word *rows       = reinterpret_cast<word *>(sb_smem);
  int32_t *perm    = reinterpret_cast<int32_t *>(sb_smem + (size_t)R * ldw * 8);
  word *flags      = reinterpret_cast<word *>(sb_smem + (size_t)R * ldw * 8 + pad16((size_t)R * 4));
  word *pivcols    = flags + 2 * nfw;

  {
    const int total = R * W;
    for (int q = t; q < total; q += T) {
      const int i = q / W, w = q - i * W;
      word x = 0;
      if (w < wa) {
        if (i < m) {
          x = ga[(int64_t)i * a_stride + w];
          if (w == wa - 1) x &= amask;
        }
      } else if (INV) {
        x = ((i >> 6) == w - wa) ? (word)1 << (i & 63) : 0;
      } else if (OP == SB_SOLVE) {
        x = gb[(int64_t)i * b_stride + (w - wa)];
        if (w == W - 1) x &= bmask;
      }
      rows[i * ldw + w] = x;
    }
    for (int i = t; i < R; i += T) perm[i] = i;
    for (int j = t; j < nfw; j += T) pivcols[j] = 0;
    __syncthreads();
  }

  int rank = 0;
  PendingSwap sw;  // the previous column's pending swap of perm[rank] and perm[p]
  for (int c = 0; c < (INV ? 2 * n : n) && rank < m; ++c) {
    word *buf    = flags + (c & 1) * nfw;
    const int cw = c < n ? c >> 6 : wa + ((c - n) >> 6), cb = (c < n ? c : c - n) & 63;
    flag_pass<true>(buf, rows, ldw, perm, sw, R, cw, cb, t, T);
    __syncthreads();
    const int p = find_pivot(buf, rank, rfw);
    if (p < 0) continue;  // no writes this column; the next flag pass uses the other buffer
    if (t == 0 && c < n) pivcols[c >> 6] |= (word)1 << (c & 63);
    const int P  = perm[p];
    const word *prow = rows + P * ldw;
    sw.record(perm, rank, p, P);
    // the full update: every flagged row i != p (row `rank` is unflagged when p != rank), words cw .. W-1 (the pivot row has no
    // bit left of column c).
    for_each_item(0, R, cw, W, t, T, [&](int i, int w) {
      if (flag_of(buf, i) && i != p) rows[perm[i] * ldw + w] ^= prow[w];
    });
    ++rank;
    __syncthreads();
  }
  sw.finish(perm, R, t, T);
  __syncthreads();

  if (OP == SB_KER) {
    // The swap rule (file comment): step i moves the column at position i to position p_i, so pos[i] = p_i for i < rank, and a free
    // column f goes f -> p_f -> p_{p_f} -> ... until its position is >= rank.  A row of R is a single bit (a free column) or the
    // bits of a row of E at the free columns (a pivot column).
    int32_t *pos = reinterpret_cast<int32_t *>(pivcols + nfw), *idx = pos + n;
    for (int c = t; c < n; c += T) {
      const word pc = pivcols[c >> 6];
      if ((pc >> (c & 63)) & 1) {
        int i = __builtin_popcountll(pc & (((word)1 << (c & 63)) - 1));
        for (int j = 0; j < (c >> 6); ++j) i += __builtin_popcountll(pivcols[j]);
        pos[i] = c;
        idx[c] = i;
      }
    }
    __syncthreads();
    for (int f = t; f < n; f += T) {
      if (!((pivcols[f >> 6] >> (f & 63)) & 1)) {
        int q = f;
        while (q < rank) q = pos[q];
        pos[q] = f;  // q >= rank: no thread reads it in this loop
        idx[f] = q - rank;
      }
    }
    __syncthreads();
    const int wr = (k + 63) >> 6, nb = (n - rank < k) ? n - rank : k;  // nb: the basis columns stored
    for (int q = t; q < n * wr; q += T) {
      const int i = q / wr, w = q - i * wr;
      word x = 0;
      if ((pivcols[i >> 6] >> (i & 63)) & 1) {
        const word *er = rows + perm[idx[i]] * ldw;
        const int je   = (w + 1) * 64 < nb ? (w + 1) * 64 : nb;
        for (int j = w * 64; j < je; ++j) {
          const int f = pos[rank + j];
          x |= ((er[f >> 6] >> (f & 63)) & 1) << (j & 63);
        }
      } else if (idx[i] < k && (idx[i] >> 6) == w) {
        x = (word)1 << (idx[i] & 63);
      }
      store_masked(gb + (int64_t)i * b_stride + w, x, w == wr - 1, bmask);
    }
    if (t == 0) rank_out[b] = rank;
    return;
  }

  if (INV) {
    store_rows_out(gb, b_stride, rows + wa, ldw, perm, n, wb, bmask, t, T);  // the right half
    if (t == 0 && rank_out) {
      int r = 0;
      for (int j = 0; j < nfw; ++j) r += __builtin_popcountll(pivcols[j]);
      rank_out[b] = r;
    }
    return;
  }

  // rows >= rank have no bit of A left: consistent iff their B words are zero.  The verdict in flags[0], the pivot rows below column
  // j * 64 in the second flag buffer (both free now; no __syncthreads_or, whose static LDS would not fit beside a full budget).
  if (t == 0) flags[0] = 0;
  __syncthreads();
  int nz = 0;
  for (int q = rank * wb + t; q < R * wb; q += T) {
    const int i = q / wb, w = q - i * wb;
    nz |= rows[perm[i] * ldw + wa + w] != 0;
  }
  if (__ballot(nz) && lane == 0) flags[0] = 1;
  __syncthreads();
  const bool bad = flags[0] != 0;
  if (!bad) {
    int32_t *below = reinterpret_cast<int32_t *>(flags + nfw);
    if (t == 0) {
      int s = 0;
      for (int j = 0; j < nfw; ++j) {
        below[j] = s;
        s += __builtin_popcountll(pivcols[j]);
      }
    }
    __syncthreads();
    const int total = R * wb;
    for (int q = t; q < total; q += T) {
      const int i = q / wb, w = q - i * wb;
      word x      = 0;
      if (i < n) {
        const word pc = pivcols[i >> 6];
        if ((pc >> (i & 63)) & 1) x = rows[perm[below[i >> 6] + __builtin_popcountll(pc & (((word)1 << (i & 63)) - 1))] * ldw + wa + w];
      }
      store_masked(gb + (int64_t)i * b_stride + w, x, w == wb - 1, bmask);
    }
  }
  if (t == 0) {
    status[b] = bad ? -1 : 0;
    if (rank_out) rank_out[b] = rank;
  }
}

// path 1's LDS (sb_block_kernel): R rows of W words, the row index, flags and pivot columns over max(R, n), `tab` int32 entries
int64_t lds_bytes_path1(int64_t R, int64_t W, int64_t n, int64_t tab) {
  return R * lds_row_words(W) * 8 + (int64_t)pad16((size_t)R * 4) + 3 * (((R > n ? R : n) + 63) / 64) * 8 + tab * 4;
}

// the kernel's path 1: m rows of words(n), the swap rule's arrangement and the index table (n entries each)
int64_t lds_bytes_kernel(int64_t m, int64_t n) { return lds_bytes_path1(m, width_of(n), n, 2 * n); }

template <int OP>
int launch(const word *A, int64_t a_stride, int64_t a_bs, word *B, int64_t b_stride, int64_t b_bs, int64_t m, int64_t n, int64_t k,
           int64_t batch, int path, int32_t *status, int32_t *rank, hipStream_t st) {
  if (path == 0)
    return launch_waves(batch, [&](dim3 grid, int64_t b0, int64_t) {
      hipLaunchKernelGGL(sb_wave_kernel<OP>, grid, dim3(BATCH_WAVE_THREADS), 0, st, A, a_stride, a_bs, B, b_stride, b_bs, (int)m, (int)n, (int)k, b0, batch,
                         status, rank);
    });
  HIPTRY(set_max_dynamic_lds<OP>(BATCH_LDS_BUDGET, sb_block_kernel<OP>));  // the three OPs' kernels have one type
  const bool ker    = OP == SB_KER;
  const int64_t R   = (ker || m > n) ? m : n, W = width_of(n) + (ker ? 0 : width_of(k));
  const int threads = block_threads(R, W);
  const size_t lds  = (size_t)(ker ? lds_bytes_kernel(m, n) : lds_bytes_path1(R, W, n, 0));
  return launch_members(batch, [&](dim3 grid, int64_t b0) {
    hipLaunchKernelGGL(sb_block_kernel<OP>, grid, dim3(threads), lds, st, A, a_stride, a_bs, B, b_stride, b_bs, (int)m, (int)n,
                       (int)k, (int)lds_row_words(W), b0, status, rank);
  });
}

// path 2 of the solve: per member, B's padding rows m .. R-1 checked first (all of them, see the header), then PLUQ of a copy of A_b
// and the solve through it on a copy of B_b -- m4ri_amd_solve_left_dev's two steps, split to keep the rank -- and X copied back only
// when it exists.
int run_path2_solve(const word *A, int64_t a_stride, int64_t a_bs, int64_t m, int64_t n, word *B, int64_t b_stride, int64_t b_bs, int64_t k,
                    int64_t batch, int32_t *status, int32_t *rank, hipStream_t st) {
  const int64_t R = m > n ? m : n, wa = width_of(n), wb = width_of(k);
  std::vector<int32_t> hs((size_t)batch), hr((size_t)batch), P((size_t)(m > 0 ? m : 1)), Q((size_t)(n > 0 ? n : 1));
  word *sA = nullptr, *sB = nullptr;
  Scratch scratch(st);
  if (m > 0 && n > 0) HIPTRY(scratch.words(&sA, m * wa));
  if (wb > 0) HIPTRY(scratch.words(&sB, R * wb));
  for (int64_t b = 0; b < batch; ++b) {
    const word *Ab = A + b * a_bs;
    word *Bb       = B + b * b_bs;
    int32_t r      = 0;
    if (m > 0 && n > 0) {
      HIPTRY(clean_copy(sA, wa, Ab, a_stride, m, n, st));
      HIPTRY(m4ri_amd_pluq_dev(sA, wa, m, n, P.data(), Q.data(), &r, M4RI_AMD_PLE_CUTOFF, st));
    }
    hr[(size_t)b] = r;
    bool zero     = true;
    HIPTRY(rows_zero(Bb, b_stride, (m > 0 && n > 0) ? m : 0, R, k, st, &zero));  // A = 0: every row of B
    int ret = zero ? 0 : -1;
    if (ret == 0 && wb > 0 && m > 0 && n > 0) {
      HIPTRY(clean_copy(sB, wb, Bb, b_stride, R, k, st));
      HIPTRY(m4ri_amd_pluq_solve_left_dev(sA, wa, m, n, r, P.data(), Q.data(), sB, wb, R, k, 0, 1, &ret, st));
      if (ret == 0) HIPTRY(gf2_launch_copy_masked(st, Bb, b_stride, sB, wb, R, k));
    }
    hs[(size_t)b] = ret;
  }
  HIPTRY(hipMemcpyAsync(status, hs.data(), (size_t)batch * 4, hipMemcpyHostToDevice, st));
  if (rank) HIPTRY(hipMemcpyAsync(rank, hr.data(), (size_t)batch * 4, hipMemcpyHostToDevice, st));
  HIPTRY(hipStreamSynchronize(st));
  return scratch.done();
}

// path 2 of the inverse: per member, m4ri_amd_inv_dev on a clean copy of A_b into scratch, copied into Binv_b; the rank (when
// wanted) by m4ri_amd_echelonize_dev of the copy afterwards.
int run_path2_inv(word *Binv, int64_t b_stride, int64_t b_bs, const word *A, int64_t a_stride, int64_t a_bs, int64_t n, int64_t batch, int32_t *rank,
                  hipStream_t st) {
  const int64_t wn = width_of(n);
  std::vector<int32_t> hr((size_t)batch);
  word *sA = nullptr, *sX = nullptr;
  Scratch scratch(st);
  HIPTRY(scratch.words(&sA, n * wn));
  HIPTRY(scratch.words(&sX, n * wn));
  for (int64_t b = 0; b < batch; ++b) {
    HIPTRY(clean_copy(sA, wn, A + b * a_bs, a_stride, n, n, st));
    HIPTRY(m4ri_amd_inv_dev(sX, wn, sA, wn, n, st));
    HIPTRY(gf2_launch_copy_masked(st, Binv + b * b_bs, b_stride, sX, wn, n, n));
    if (rank) HIPTRY(m4ri_amd_echelonize_dev(sA, wn, n, n, 0, &hr[(size_t)b], st));
  }
  if (rank) HIPTRY(hipMemcpyAsync(rank, hr.data(), (size_t)batch * 4, hipMemcpyHostToDevice, st));
  HIPTRY(hipStreamSynchronize(st));
  return scratch.done();
}

// path 2 of the kernel: per member, m4ri_amd_kernel_left_pluq_dev on a clean copy of A_b (m = 0: one zero row, the same basis)
// into an n x n scratch basis cleared before each member, whose first kc columns are copied under the mask.
int run_path2_kernel(const word *A, int64_t a_stride, int64_t a_bs, int64_t m, int64_t n, word *R, int64_t r_stride, int64_t r_bs, int64_t kc,
                     int64_t batch, int32_t *rank, hipStream_t st) {
  const int64_t wn = width_of(n), rows = m > 0 ? m : 1;
  std::vector<int32_t> hr((size_t)batch);
  word *sA = nullptr, *sR = nullptr;
  Scratch scratch(st);
  HIPTRY(scratch.words(&sA, rows * wn));
  HIPTRY(scratch.words(&sR, n * wn));
  for (int64_t b = 0; b < batch; ++b) {
    if (m > 0) {
      HIPTRY(clean_copy(sA, wn, A + b * a_bs, a_stride, m, n, st));
    } else {
      HIPTRY(hipMemsetAsync(sA, 0, (size_t)wn * 8, st));
    }
    HIPTRY(hipMemsetAsync(sR, 0, (size_t)(n * wn) * 8, st));
    HIPTRY(m4ri_amd_kernel_left_pluq_dev(sA, wn, rows, n, sR, wn, 0, &hr[(size_t)b], st));
    if (kc > 0) HIPTRY(gf2_launch_copy_masked(st, R + b * r_bs, r_stride, sR, wn, n, kc));
  }
  HIPTRY(hipMemcpyAsync(rank, hr.data(), (size_t)batch * 4, hipMemcpyHostToDevice, st));
  HIPTRY(hipStreamSynchronize(st));
  return scratch.done();
}

}  // namespace

extern "C" {

int m4ri_amd_plan_solve_batch(int64_t m, int64_t n, int64_t k) {
  if (m < 0 || n < 0 || k < 0) return -1;
  const int64_t R = m > n ? m : n;
  if (R <= 64 && k <= 64) return 0;
  const int64_t W = width_of(n) + width_of(k);
  if (R > BATCH_LDS_BUDGET / 8 || W > BATCH_LDS_BUDGET / 8) return 2;
  return lds_bytes_path1(R, W, n, 0) <= BATCH_LDS_BUDGET ? 1 : 2;
}

int m4ri_amd_solve_left_batch_dev(const word *A, int64_t a_stride, int64_t a_bs, int64_t m, int64_t n, word *B, int64_t b_stride, int64_t b_bs,
                                  int64_t k, int64_t batch, int32_t *status, int32_t *rank, void *stream) {
  if (m < 0 || n < 0 || k < 0 || batch < 0 || a_stride < 0 || a_bs < 0 || b_stride < 0 || b_bs < 0) return (int)hipErrorInvalidValue;
  const int64_t R = m > n ? m : n, wa = width_of(n), wb = width_of(k);
  if (a_stride < wa || b_stride < wb) return (int)hipErrorInvalidValue;
  if (!members_fit(batch, b_bs, R, b_stride, wb)) return (int)hipErrorInvalidValue;
  if (batch > 0 && !status) return (int)hipErrorInvalidValue;
  if (batch > 0 && ((m > 0 && n > 0 && !A) || (R > 0 && k > 0 && !B))) return (int)hipErrorInvalidValue;
  if (batch == 0) return 0;
  hipStream_t st = (hipStream_t)stream;
  const int path = m4ri_amd_plan_solve_batch(m, n, k);
  if (path == 2) return run_path2_solve(A, a_stride, a_bs, m, n, B, b_stride, b_bs, k, batch, status, rank, st);
  return launch<SB_SOLVE>(A, a_stride, a_bs, B, b_stride, b_bs, m, n, k, batch, path, status, rank, st);
}

int m4ri_amd_inv_batch_dev(word *Binv, int64_t b_stride, int64_t b_bs, const word *A, int64_t a_stride, int64_t a_bs, int64_t n, int64_t batch,
                           int32_t *rank, void *stream) {
  if (n < 0 || batch < 0 || b_stride < 0 || b_bs < 0 || a_stride < 0 || a_bs < 0) return (int)hipErrorInvalidValue;
  const int64_t wn = width_of(n);
  if (b_stride < wn || a_stride < wn) return (int)hipErrorInvalidValue;
  if (!members_fit(batch, b_bs, n, b_stride, wn)) return (int)hipErrorInvalidValue;
  if (batch > 0 && n > 0 && (!Binv || !A)) return (int)hipErrorInvalidValue;
  if (batch > 0 && n > 0) {  // in place with the same layout, or no overlap at all
    if (Binv == A) {
      if (a_stride != b_stride || a_bs != b_bs) return (int)hipErrorInvalidValue;
    } else if (spans_meet(rows_span(Binv, batch, b_bs, n, b_stride, wn), rows_span(A, batch, a_bs, n, a_stride, wn))) {
      return (int)hipErrorInvalidValue;
    }
  }
  if (batch == 0) return 0;
  hipStream_t st = (hipStream_t)stream;
  if (n == 0) return rank ? (int)hipMemsetAsync(rank, 0, (size_t)batch * 4, st) : 0;
  const int path = m4ri_amd_plan_solve_batch(n, n, n);
  if (path == 2) return run_path2_inv(Binv, b_stride, b_bs, A, a_stride, a_bs, n, batch, rank, st);
  return launch<SB_INV>(A, a_stride, a_bs, Binv, b_stride, b_bs, n, n, n, batch, path, nullptr, rank, st);
}

int m4ri_amd_plan_kernel_batch(int64_t m, int64_t n) {
  if (m < 0 || n < 0) return -1;
  if (m <= 64 && n <= 64) return 0;
  if (m > BATCH_LDS_BUDGET / 8 || n > BATCH_LDS_BUDGET / 8) return 2;
  return lds_bytes_kernel(m, n) <= BATCH_LDS_BUDGET ? 1 : 2;
}

int m4ri_amd_kernel_left_batch_dev(const word *A, int64_t a_stride, int64_t a_bs, int64_t m, int64_t n, word *R, int64_t r_stride, int64_t r_bs,
                                   int64_t kc, int64_t batch, int32_t *rank, void *stream) {
  if (m < 0 || n < 0 || kc < 0 || batch < 0 || a_stride < 0 || a_bs < 0 || r_stride < 0 || r_bs < 0 || kc > n) return (int)hipErrorInvalidValue;
  const int64_t wa = width_of(n), wr = width_of(kc);
  if (a_stride < wa || r_stride < wr) return (int)hipErrorInvalidValue;
  if (!members_fit(batch, r_bs, n, r_stride, wr)) return (int)hipErrorInvalidValue;
  if (batch > 0 && !rank) return (int)hipErrorInvalidValue;
  const bool a_data = m > 0 && n > 0, r_data = kc > 0;  // kc <= n
  if (batch > 0 && ((a_data && !A) || (r_data && !R))) return (int)hipErrorInvalidValue;
  // R's span and A's span (first member's start to last member's end) must not meet
  if (spans_meet(rows_span(R, batch, r_bs, n, r_stride, wr), rows_span(A, batch, a_bs, m, a_stride, wa))) return (int)hipErrorInvalidValue;
  if (batch == 0) return 0;
  hipStream_t st = (hipStream_t)stream;
  if (n == 0) return (int)hipMemsetAsync(rank, 0, (size_t)batch * 4, st);
  const int path = m4ri_amd_plan_kernel_batch(m, n);
  if (path == 2) return run_path2_kernel(A, a_stride, a_bs, m, n, R, r_stride, r_bs, kc, batch, rank, st);
  return launch<SB_KER>(A, a_stride, a_bs, R, r_stride, r_bs, m, n, kc, batch, path, nullptr, rank, st);
}

}  // extern "C"
