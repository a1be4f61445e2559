// ple_batch.hip -- PLE / PLUQ decompositions of many independent small matrices in one launch, and the solves A_b X_b = B_b from the
// stored factors (mzd_pluq then mzd_pluq_solve_left, m4ri/solve.h:76), one launch for the batch.
//
// The decomposition is the column-by-column one (what _mzd_ple_russian, ple_russian.c:380-617, computes):
// columns left to right, the pivot of a column is the first row at or below the rank with the bit set, it is swapped up to the
// rank's row (P[rank] = that row, Q[rank] = the column) and added into the rows below with the bit FROM THE NEXT COLUMN ON, so the
// multiplier stays in the pivot column.  Then L is compressed to the left: row r takes the column swaps (j, Q[j]) for
// j = 0 .. min(r, rank - 1).  PLUQ: row r then takes the swaps (i, Q[i]) for i = r + 1 .. ncols - 1; Q is the identity behind the
// rank, so together with the compression every row takes the swaps j = 0 .. rank - 1.  The paths (m4ri_amd_plan_ple_batch):
//   0  nrows, ncols <= 64: a wave per member, lane i holds row i, lane t entry t of P and of Q; pivot = lowest lane >= rank of a
//      ballot; the compression is a wave-uniform loop over j of bit swaps predicated on the lane.  No LDS, no barrier.
//   1  the member fits in LDS: a workgroup per member, rows staged in LDS under a row-permutation index (batch_common.h's scheme),
//      P and Q beside them; two barriers per column with a pivot; the compression is a loop of bit swaps per row, a thread per row.
//   2  larger members up to BATCH_CAP_BYTES: a workgroup per member, rows in place in global memory, whole rows swapped physically (the
//      last word under the column mask), P and Q written straight to the output; three barriers per column with a pivot.
//   3  above the cap: the members one by one through m4ri_amd_ple_dev / m4ri_amd_pluq_dev (recursion_cutoff = 0) on a scratch copy,
//      then P, Q and rank in one copy each.  Blocking.
// Paths 0-2 are one launch each (plus chunking above 2^30 workgroups), no allocation, no copy, no host synchronisation.
// Memory rules: bits at columns >= ncols of a row's last word are never changed, nor the words from `width` to `stride` of a row,
// nor anything between members.
//
// The solve follows _mzd_pluq_solve_left (solve.c:57-121) with the check on: B <- P^T B, forward substitution with the unit lower
// L of the first `rank` columns carried on through the rows rank .. m-1 (which then hold B2 + H Y1), consistent iff those rows and the
// padding rows m .. max(m, n)-1 are zero, back substitution with the unit upper U, rows from the rank on zero, B <- Q B.  An
// inconsistent member's B is not written.  Only the bits of A on the proper side of the diagonal are read.  The paths
// (m4ri_amd_plan_pluq_solve_batch):
//   0  max(m, n) <= 64 and k <= 64: a wave per member, lane i holds row i of B and of A; substitution by readlane, the verdict by ballot.
//   1  B_b fits in LDS: a workgroup per member, B staged in LDS under a row index (both permutations are index updates), A read from
//      global memory, a word per row once per 64 columns; one barrier per column of L and of U.
//   2  larger members one by one through m4ri_amd_pluq_solve_left_dev on scratch copies.  Blocking.
#include <hip/hip_runtime.h>
#include <vector>
#include "batch_common.h"
#include "../../include/m4ri_amd.h"

namespace {

__device__ __forceinline__ word swap_bits(word v, int a, int b) {  // bits a and b of v exchanged
  const word x = ((v >> a) ^ (v >> b)) & 1;
  return v ^ (x << a) ^ (x << b);
}

// the column swap (a, b) in a row of words
__device__ __forceinline__ void swap_cols(word *row, int a, int b) {
  const word x = ((row[a >> 6] >> (a & 63)) ^ (row[b >> 6] >> (b & 63))) & 1;
  if (x) {
    row[a >> 6] ^= (word)1 << (a & 63);
    row[b >> 6] ^= (word)1 << (b & 63);
  }
}

// ---- the decomposition ----------------------------------------------------------------------------------------------------------

// path 0: a wave per member, lane i = row i (one word), lane t = P[t] and Q[t].  Members b0 + 4 * blockIdx.x + wave.
__global__ __launch_bounds__(BATCH_WAVE_THREADS) void pb_wave_kernel(word *__restrict__ A, int64_t stride, int64_t a_bs, int nrows, int ncols,
                                                                     int64_t b0, int64_t batch, int pluq, int32_t *__restrict__ P,
                                                                     int32_t *__restrict__ Q, int32_t *__restrict__ rank_out) {
  const int lane  = threadIdx.x & 63;
  const int64_t b = b0 + (int64_t)blockIdx.x * (BATCH_WAVE_THREADS / 64) + (threadIdx.x >> 6);
  if (b >= batch) return;  // wave-uniform, no barrier in this kernel
  word *g         = A + b * a_bs;
  const word mask = tail_mask(ncols);
  word orig = 0, v = 0;
  if (lane < nrows) {
    orig = g[(int64_t)lane * stride];
    v    = orig & mask;
  }
  int rank = 0, pv = lane, qv = lane;
  for (int c = 0; c < ncols && rank < nrows; ++c) {
    const int bit   = (int)((v >> c) & 1);
    const word cand = __ballot(bit) & (~(word)0 << rank);
    if (!cand) continue;
    const int p    = (int)__builtin_ctzll(cand);
    const word pw  = readlane64(v, p);
    const word add = c < 63 ? pw & (~(word)0 << (c + 1)) : 0;  // from the next column on
    if (bit && lane > rank && lane != p) v ^= add;
    const word vr = readlane64(v, rank);  // row `rank` has no bit c unless it is the pivot: unchanged by the update
    if (lane == rank) {
      v  = pw;
      pv = p;
      qv = c;
    } else if (lane == p) {
      v = vr;
    }
    ++rank;
  }
  for (int j = 0; j < rank; ++j) {  // row r takes (j, Q[j]) for j <= r; PLUQ: every row takes it
    const int q = __builtin_amdgcn_readlane(qv, j);
    if (q != j && (pluq || lane >= j)) v = swap_bits(v, j, q);
  }
  if (lane < nrows) {
    g[(int64_t)lane * stride] = (v & mask) | (orig & ~mask);
    P[b * nrows + lane]       = pv;
  }
  if (lane < ncols) Q[b * ncols + lane] = qv;
  if (lane == 0) rank_out[b] = rank;
}

// paths 1 (INLDS) and 2: a workgroup per member.  Dynamic LDS (16-byte carve offsets):
//   INLDS: rows [nrows][ldw] words | perm [nrows] int32 | P [nrows] int32 | Q [ncols] int32 (each rounded up to 16 B) | flags [2][nfw] words
//   else:  flags [2][nfw] words; P and Q are the output arrays
// Row i of the flag pass is owned by thread i % blockDim.x (the lane of its ballot); flags[c & 1] bit i = bit c of logical row i.
template <bool INLDS>
__global__ __launch_bounds__(BATCH_MAX_THREADS) void pb_block_kernel(word *__restrict__ A, int64_t stride, int64_t a_bs, int nrows, int ncols,
                                                                     int ldw, int64_t b0, int pluq, int32_t *__restrict__ P_out,
                                                                     int32_t *__restrict__ Q_out, int32_t *__restrict__ rank_out) {
  extern __shared__ __attribute__((aligned(16))) char pb_smem[];
  const int T = blockDim.x, t = threadIdx.x;
  const int64_t b = b0 + blockIdx.x;
  word *g         = A + b * a_bs;
  const int width = (ncols + 63) >> 6;
  const int nfw   = (nrows + 63) >> 6;
  const word mask = tail_mask(ncols);
  int32_t *Pg = P_out + b * nrows, *Qg = Q_out + b * ncols;
  word *rows    = reinterpret_cast<word *>(pb_smem);
  size_t off    = INLDS ? (size_t)nrows * ldw * 8 : 0;
  int32_t *perm = reinterpret_cast<int32_t *>(pb_smem + off);
  if (INLDS) off += pad16((size_t)nrows * 4);
  int32_t *Pv = INLDS ? reinterpret_cast<int32_t *>(pb_smem + off) : Pg;
  if (INLDS) off += pad16((size_t)nrows * 4);
  int32_t *Qv = INLDS ? reinterpret_cast<int32_t *>(pb_smem + off) : Qg;
  if (INLDS) off += pad16((size_t)ncols * 4);
  word *flags = reinterpret_cast<word *>(pb_smem + off);

  if (INLDS) {
    stage_rows_in(rows, ldw, g, stride, nrows, width, mask, t, T);
    for (int i = t; i < nrows; i += T) perm[i] = i;
  }
  for (int i = t; i < nrows; i += T) Pv[i] = i;
  for (int j = t; j < ncols; j += T) Qv[j] = j;
  __syncthreads();

  int rank = 0;
  PendingSwap sw;  // INLDS: the previous column's pending swap of perm[rank] and perm[p]
  for (int c = 0; c < ncols && rank < nrows; ++c) {
    word *buf    = flags + (c & 1) * nfw;
    const int cw = c >> 6, cb = c & 63;
    if (INLDS) flag_pass<true>(buf, rows, ldw, perm, sw, nrows, cw, cb, t, T);
    else flag_pass<false>(buf, g, stride, perm, sw, nrows, cw, cb, t, T);
    __syncthreads();
    const int p = find_pivot(buf, rank, nfw);
    if (p < 0) continue;  // no writes this column; the next flag pass uses the other buffer
    if (t == 0) {
      Pv[rank] = p;
      Qv[rank] = c;
    }
    const word *prow;
    if (INLDS) {
      const int Pp = perm[p];
      prow         = rows + Pp * ldw;
      sw.record(perm, rank, p, Pp);
    } else {
      if (p != rank) {  // physical swap of the whole rows (the multipliers to the left move too), the bits behind ncols stay
        swap_rows_global(g + (int64_t)rank * stride, g + (int64_t)p * stride, 0, width, mask, t, T);
        __syncthreads();
      }
      prow = g + (int64_t)rank * stride;
    }
    // the update: flagged rows i > rank, i != p (row p holds the old row `rank`, which had no bit c), columns c + 1 .. ncols - 1.
    const word first = cb < 63 ? ~(word)0 << (cb + 1) : 0;
    for_each_item(rank + 1, nrows, cw, width, t, T, [&](int i, int w) {
      if (flag_of(buf, i) && i != p) {
        word x = prow[w];
        if (w == cw) x &= first;
        if (INLDS) {
          rows[perm[i] * ldw + w] ^= x;
        } else {
          if (w == width - 1) x &= mask;
          g[(int64_t)i * stride + w] ^= x;
        }
      }
    });
    ++rank;
    __syncthreads();
  }

  if (INLDS) {
    sw.finish(perm, nrows, t, T);
    __syncthreads();
  }
  // L to the left (and PLUQ's column step): a thread per row, the swaps in order.  Path 2 pays up to `rank` uncoalesced global
  // read-modify-writes per row here (only for the j with Q[j] != j); measured with the rest in profiles/ple_batch_timing.log.
  for (int r = t; r < nrows; r += T) {
    word *row      = INLDS ? rows + perm[r] * ldw : g + (int64_t)r * stride;
    const int last = (pluq || r >= rank) ? rank - 1 : r;
    for (int j = 0; j <= last; ++j) {
      const int q = Qv[j];
      if (q != j) swap_cols(row, j, q);
    }
  }
  if (INLDS) {
    __syncthreads();
    store_rows_out(g, stride, rows, ldw, perm, nrows, width, mask, t, T);
    for (int i = t; i < nrows; i += T) Pg[i] = Pv[i];
    for (int j = t; j < ncols; j += T) Qg[j] = Qv[j];
  }
  if (t == 0) rank_out[b] = rank;
}

// nrows == 0 or ncols == 0: rank 0, P and Q the identity
__global__ void pb_identity_kernel(int32_t *__restrict__ P, int64_t nrows, int32_t *__restrict__ Q, int64_t ncols, int32_t *__restrict__ rank,
                                   int64_t batch) {
  const int64_t step = (int64_t)gridDim.x * blockDim.x;  // grid-stride: the grid is capped at BATCH_CHUNK workgroups
  for (int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; k < batch * nrows || k < batch * ncols || k < batch; k += step) {
    if (k < batch * nrows) P[k] = (int32_t)(k % nrows);
    if (k < batch * ncols) Q[k] = (int32_t)(k % ncols);
    if (k < batch) rank[k] = 0;
  }
}

int64_t lds_bytes_ple(int64_t nrows, int64_t ncols) {
  return nrows * lds_row_words(width_of(ncols)) * 8 + 2 * (int64_t)pad16((size_t)nrows * 4) + (int64_t)pad16((size_t)ncols * 4) +
         2 * ((nrows + 63) / 64) * 8;
}

int run_ple_path3(word *A, int64_t stride, int64_t a_bs, int64_t nrows, int64_t ncols, int64_t batch, int pluq, int32_t *P, int32_t *Q,
                  int32_t *rank, hipStream_t st) {
  const int64_t width = width_of(ncols);
  std::vector<int32_t> hp((size_t)(batch * nrows)), hq((size_t)(batch * ncols)), hr((size_t)batch);
  word *s = nullptr;
  Scratch scratch(st);
  HIPTRY(scratch.words(&s, nrows * width));
  for (int64_t b = 0; b < batch; ++b) {
    word *Ab = A + b * a_bs;
    HIPTRY(clean_copy(s, width, Ab, stride, nrows, ncols, st));
    int32_t *p = &hp[(size_t)(b * nrows)], *q = &hq[(size_t)(b * ncols)];
    HIPTRY(pluq ? m4ri_amd_pluq_dev(s, width, nrows, ncols, p, q, &hr[(size_t)b], 0, st)
                : m4ri_amd_ple_dev(s, width, nrows, ncols, p, q, &hr[(size_t)b], 0, st));
    HIPTRY(gf2_launch_copy_masked(st, Ab, stride, s, width, nrows, ncols));
  }
  HIPTRY(hipMemcpyAsync(P, hp.data(), hp.size() * 4, hipMemcpyHostToDevice, st));
  HIPTRY(hipMemcpyAsync(Q, hq.data(), hq.size() * 4, hipMemcpyHostToDevice, st));
  HIPTRY(hipMemcpyAsync(rank, hr.data(), hr.size() * 4, hipMemcpyHostToDevice, st));
  HIPTRY(hipStreamSynchronize(st));
  return scratch.done();
}

// ---- the solve from the factors -------------------------------------------------------------------------------------------------

__device__ __forceinline__ int clamp_rank(int r, int m, int n) {
  const int mn = m < n ? m : n;
  return r < 0 ? 0 : r > mn ? mn : r;
}

// path 0: a wave per member, lane i = row i of B (x) and of A (a), lane t = P[t] and Q[t].  fb: the member whose decomposition is
// used (0 when one serves all).
__global__ __launch_bounds__(BATCH_WAVE_THREADS) void ps_wave_kernel(const word *__restrict__ A, int64_t a_stride, int64_t a_bs, int m, int n,
                                                                     const int32_t *__restrict__ rank_in, const int32_t *__restrict__ P,
                                                                     const int32_t *__restrict__ Q, word *__restrict__ B, int64_t b_stride,
                                                                     int64_t b_bs, int k, int64_t b0, int64_t batch, int32_t *__restrict__ status) {
  const int lane  = threadIdx.x & 63;
  const int64_t b = b0 + (int64_t)blockIdx.x * (BATCH_WAVE_THREADS / 64) + (threadIdx.x >> 6);
  if (b >= batch) return;  // wave-uniform, no barrier in this kernel
  const int64_t fb = a_bs ? b : 0;
  const int R      = m > n ? m : n;
  const word bmask = tail_mask(k);
  const int rank   = clamp_rank(rank_in[fb], m, n);
  word *gb         = B + b * b_bs;
  word a = 0, x = 0, orig = 0;
  int pv = lane, qv = lane;
  if (rank > 0) {
    if (lane < m) {
      a  = A[b * a_bs + (int64_t)lane * a_stride];
      pv = P[fb * m + lane];
    }
    if (lane < n) qv = Q[fb * n + lane];
  }
  if (lane < R) {
    orig = gb[(int64_t)lane * b_stride];
    x    = orig & bmask;
  }
  for (int i = 0; i < rank; ++i) {  // P^T: the swaps (i, P[i]) ascending (the identity behind the rank)
    const int p = __builtin_amdgcn_readlane(pv, i) & 63;
    if (p == i) continue;
    const word xi = readlane64(x, i), xp = readlane64(x, p);
    if (lane == i) x = xp;
    else if (lane == p) x = xi;
  }
  for (int j = 0; j < rank; ++j) {  // L, and H behind it: row j is final when its column is applied
    const word xj = readlane64(x, j);
    if (lane > j && lane < m && ((a >> j) & 1)) x ^= xj;
  }
  const bool bad = __ballot(lane >= rank && x != 0) != 0;  // rows rank .. m-1: B2 + H Y1; rows m .. R-1: B's padding rows
  if (!bad) {
    for (int j = rank - 1; j > 0; --j) {  // U
      const word xj = readlane64(x, j);
      if (lane < j && ((a >> j) & 1)) x ^= xj;
    }
    if (lane >= rank) x = 0;
    for (int i = rank - 1; i >= 0; --i) {  // Q: the swaps (i, Q[i]) descending
      const int q = __builtin_amdgcn_readlane(qv, i) & 63;
      if (q == i) continue;
      const word xi = readlane64(x, i), xq = readlane64(x, q);
      if (lane == i) x = xq;
      else if (lane == q) x = xi;
    }
    if (lane < R) gb[(int64_t)lane * b_stride] = (x & bmask) | (orig & ~bmask);
  }
  if (lane == 0) status[b] = bad ? -1 : 0;
}

// path 1: a workgroup per member.  Dynamic LDS (16-byte carve offsets):
//   rows [R][ldw] words of B | idx [R] int32: the physical row of logical row i, -1 = a zero row | pq [min(m, n)] int32: P's, then Q's
//   first `rank` entries (each rounded up to 16 B) | two flag words | acol [m] words: the word of A's rows that holds the 64 columns
//   being applied, fetched once per 64 columns (a row of A is a cache line apart from the next: re-read per column it is the
//   kernel's whole memory traffic, 16 times over)
__global__ __launch_bounds__(BATCH_MAX_THREADS) void ps_block_kernel(const word *__restrict__ A, int64_t a_stride, int64_t a_bs, int m, int n,
                                                                     const int32_t *__restrict__ rank_in, const int32_t *__restrict__ P,
                                                                     const int32_t *__restrict__ Q, word *__restrict__ B, int64_t b_stride,
                                                                     int64_t b_bs, int k, int ldw, int64_t b0, int32_t *__restrict__ status) {
  extern __shared__ __attribute__((aligned(16))) char ps_smem[];
  const int T = blockDim.x, t = threadIdx.x, lane = t & 63;
  const int64_t b  = b0 + blockIdx.x;
  const int64_t fb = a_bs ? b : 0;
  const word *ga   = A + b * a_bs;
  word *gb         = B + b * b_bs;
  const int R      = m > n ? m : n, mn = m < n ? m : n;
  const int wb     = (k + 63) >> 6;  // > 0: the host answers k == 0 itself
  const word bmask = tail_mask(k);
  const int rank   = clamp_rank(rank_in[fb], m, n);
  word *rows       = reinterpret_cast<word *>(ps_smem);
  int32_t *idx     = reinterpret_cast<int32_t *>(ps_smem + (size_t)R * ldw * 8);
  int32_t *pq      = reinterpret_cast<int32_t *>(ps_smem + (size_t)R * ldw * 8 + pad16((size_t)R * 4));
  word *flag       = reinterpret_cast<word *>(ps_smem + (size_t)R * ldw * 8 + pad16((size_t)R * 4) + pad16((size_t)mn * 4));
  word *acol       = flag + 2;

  const int total = R * wb;
  stage_rows_in(rows, ldw, gb, b_stride, R, wb, bmask, t, T);
  for (int i = t; i < R; i += T) idx[i] = i;
  for (int i = t; i < rank; i += T) pq[i] = P[fb * m + i];
  if (t == 0) *flag = 0;
  __syncthreads();
  if (t == 0) {  // P^T: the swaps (i, P[i]) ascending, on the index.  Serial: up to `rank` dependent LDS updates on one thread, as is Q below
    for (int i = 0; i < rank; ++i) {
      const int p = pq[i];
      if (p != i && (unsigned)p < (unsigned)m) {
        const int x = idx[i];
        idx[i]      = idx[p];
        idx[p]      = x;
      }
    }
  }
  __syncthreads();
  for (int i = t; i < rank; i += T) pq[i] = Q[fb * n + i];  // nobody reads pq again before the barriers below
  // L, and H behind it: column j into the rows j + 1 .. m - 1 with the bit (row j is final by then)
  for (int j = 0; j < rank; ++j) {
    if ((j & 63) == 0) {  // (the barrier that ended column j - 1 lets acol go)
      for (int i = j + 1 + t; i < m; i += T) acol[i] = ga[(int64_t)i * a_stride + (j >> 6)];
      __syncthreads();
    }
    const word *src = rows + idx[j] * ldw;
    const int items = (m - j - 1) * wb;
    for (int q = t; q < items; q += T) {
      const int i = j + 1 + q / wb, w = q % wb;
      if ((acol[i] >> (j & 63)) & 1) rows[idx[i] * ldw + w] ^= src[w];
    }
    __syncthreads();
  }
  // rows rank .. m-1 hold B2 + H Y1, rows m .. R-1 are B's padding rows: all zero, or there is no solution
  int nz = 0;
  for (int q = rank * wb + t; q < total; q += T) nz |= rows[idx[q / wb] * ldw + q % wb] != 0;
  if (__ballot(nz) && lane == 0) *flag = 1;
  __syncthreads();
  const bool bad = *flag != 0;
  if (!bad) {
    for (int j = rank - 1; j > 0; --j) {  // U: column j into the rows 0 .. j - 1 with the bit
      if ((j & 63) == 63 || j == rank - 1) {
        for (int i = t; i < j; i += T) acol[i] = ga[(int64_t)i * a_stride + (j >> 6)];
        __syncthreads();
      }
      const word *src = rows + idx[j] * ldw;
      const int items = j * wb;
      for (int q = t; q < items; q += T) {
        const int i = q / wb, w = q % wb;
        if ((acol[i] >> (j & 63)) & 1) rows[idx[i] * ldw + w] ^= src[w];
      }
      __syncthreads();
    }
    for (int i = rank + t; i < R; i += T) idx[i] = -1;  // the rows from the rank on are zero
    __syncthreads();
    if (t == 0) {  // Q: the swaps (i, Q[i]) descending, on the index
      for (int i = rank - 1; i >= 0; --i) {
        const int q = pq[i];
        if (q != i && (unsigned)q < (unsigned)n) {
          const int x = idx[i];
          idx[i]      = idx[q];
          idx[q]      = x;
        }
      }
    }
    __syncthreads();
    for (int q = t; q < total; q += T) {
      const int i = q / wb, w = q - i * wb;
      store_masked(gb + (int64_t)i * b_stride + w, idx[i] < 0 ? 0 : rows[idx[i] * ldw + w], w == wb - 1, bmask);
    }
  }
  if (t == 0) status[b] = bad ? -1 : 0;
}

int64_t lds_bytes_solve(int64_t m, int64_t n, int64_t k) {
  const int64_t R = m > n ? m : n, mn = m < n ? m : n;
  return R * lds_row_words(width_of(k)) * 8 + (int64_t)pad16((size_t)R * 4) + (int64_t)pad16((size_t)mn * 4) + 16 + m * 8;
}

// path 2: rank, P and Q to the host once; per member B's padding rows m .. R-1 checked, then m4ri_amd_pluq_solve_left_dev with the
// check on clean copies of A_b (once when shared) and B_b, and X copied back only when it exists.  (R > 64 or k > 64 here, so k > 0.)
int run_solve_path2(const word *A, int64_t a_stride, int64_t a_bs, int64_t m, int64_t n, const int32_t *rank, const int32_t *P, const int32_t *Q,
                    word *B, int64_t b_stride, int64_t b_bs, int64_t k, int64_t batch, int32_t *status, hipStream_t st) {
  const int64_t R = m > n ? m : n, mn = m < n ? m : n, wa = width_of(n), wb = width_of(k), nf = a_bs ? batch : 1;
  std::vector<int32_t> hs((size_t)batch), hr((size_t)nf), hp((size_t)(nf * m)), hq((size_t)(nf * n));
  word *sA = nullptr, *sB = nullptr;
  Scratch scratch(st);
  HIPTRY(hipMemcpyAsync(hr.data(), rank, hr.size() * 4, hipMemcpyDeviceToHost, st));
  if (!hp.empty()) HIPTRY(hipMemcpyAsync(hp.data(), P, hp.size() * 4, hipMemcpyDeviceToHost, st));
  if (!hq.empty()) HIPTRY(hipMemcpyAsync(hq.data(), Q, hq.size() * 4, hipMemcpyDeviceToHost, st));
  HIPTRY(hipStreamSynchronize(st));
  if (mn > 0) HIPTRY(scratch.words(&sA, m * wa));
  HIPTRY(scratch.words(&sB, R * wb));
  for (int64_t b = 0; b < batch; ++b) {
    const int64_t fb = a_bs ? b : 0;
    word *Bb         = B + b * b_bs;
    int32_t r        = hr[(size_t)fb];
    r                = r < 0 ? 0 : r > mn ? (int32_t)mn : r;
    bool zero        = true;
    HIPTRY(rows_zero(Bb, b_stride, mn > 0 ? m : 0, R, k, st, &zero));  // A empty: every row of B
    int ret = zero ? 0 : -1;
    if (ret == 0 && mn > 0) {
      if (b == 0 || a_bs) HIPTRY(clean_copy(sA, wa, A + b * a_bs, a_stride, m, n, st));
      HIPTRY(clean_copy(sB, wb, Bb, b_stride, R, k, st));
      HIPTRY(m4ri_amd_pluq_solve_left_dev(sA, wa, m, n, r, &hp[(size_t)(fb * m)], &hq[(size_t)(fb * n)], sB, wb, R, k, 0, 1, &ret, st));
      if (ret == 0) HIPTRY(gf2_launch_copy_masked(st, Bb, b_stride, sB, wb, R, k));
    }
    hs[(size_t)b] = ret;
  }
  HIPTRY(hipMemcpyAsync(status, hs.data(), (size_t)batch * 4, hipMemcpyHostToDevice, st));
  HIPTRY(hipStreamSynchronize(st));
  return scratch.done();
}

}  // namespace

extern "C" {

int m4ri_amd_plan_ple_batch(int64_t nrows, int64_t ncols) {
  if (nrows < 0 || ncols < 0) return -1;
  if (nrows <= 64 && ncols <= 64) return 0;
  const int64_t width = width_of(ncols);
  if (nrows > BATCH_CAP_BYTES / 8 || width > BATCH_CAP_BYTES / 8 || nrows * width > BATCH_CAP_BYTES / 8) return 3;
  return lds_bytes_ple(nrows, ncols) <= BATCH_LDS_BUDGET ? 1 : 2;
}

int m4ri_amd_ple_batch_dev(word *A, int64_t stride, int64_t a_bs, int64_t nrows, int64_t ncols, int64_t batch, int pluq, int32_t *P, int32_t *Q,
                           int32_t *rank, void *stream) {
  if (nrows < 0 || ncols < 0 || batch < 0 || stride < 0 || a_bs < 0) return (int)hipErrorInvalidValue;
  const int64_t width = width_of(ncols);
  if (stride < width) return (int)hipErrorInvalidValue;
  if (!members_fit(batch, a_bs, nrows, stride, width)) return (int)hipErrorInvalidValue;
  if (batch > 0 && (!rank || (nrows > 0 && !P) || (ncols > 0 && !Q))) return (int)hipErrorInvalidValue;
  if (batch > 0 && nrows > 0 && ncols > 0 && !A) return (int)hipErrorInvalidValue;
  if (batch == 0) return 0;
  hipStream_t st = (hipStream_t)stream;
  if (nrows == 0 || ncols == 0) {
    const int64_t total = batch * (nrows > ncols ? nrows : ncols > 0 ? ncols : 1), blocks = (total + 255) / 256;
    hipLaunchKernelGGL(pb_identity_kernel, dim3((unsigned)(blocks < BATCH_CHUNK ? blocks : BATCH_CHUNK)), dim3(256), 0, st, P, nrows, Q, ncols, rank, batch);
    return (int)hipGetLastError();
  }
  const int path = m4ri_amd_plan_ple_batch(nrows, ncols);
  if (path == 0)
    return launch_waves(batch, [&](dim3 grid, int64_t b0, int64_t) {
      hipLaunchKernelGGL(pb_wave_kernel, grid, dim3(BATCH_WAVE_THREADS), 0, st, A, stride, a_bs, (int)nrows, (int)ncols, b0, batch, pluq, P, Q, rank);
    });
  if (path == 3) return run_ple_path3(A, stride, a_bs, nrows, ncols, batch, pluq, P, Q, rank, st);
  const bool inlds  = path == 1;
  const int threads = block_threads(nrows, width);
  const int ldw     = inlds ? (int)lds_row_words(width) : 0;
  const size_t lds  = inlds ? (size_t)lds_bytes_ple(nrows, ncols) : (size_t)(2 * ((nrows + 63) / 64) * 8);
  HIPTRY(set_max_dynamic_lds(BATCH_LDS_BUDGET, pb_block_kernel<true>, pb_block_kernel<false>));
  return launch_members(batch, [&](dim3 grid, int64_t b0) {
    if (inlds) hipLaunchKernelGGL(pb_block_kernel<true>, grid, dim3(threads), lds, st, A, stride, a_bs, (int)nrows, (int)ncols, ldw, b0, pluq, P, Q, rank);
    else hipLaunchKernelGGL(pb_block_kernel<false>, grid, dim3(threads), lds, st, A, stride, a_bs, (int)nrows, (int)ncols, ldw, b0, pluq, P, Q, rank);
  });
}

int m4ri_amd_plan_pluq_solve_batch(int64_t m, int64_t n, int64_t k) {
  if (m < 0 || n < 0 || k < 0) return -1;
  const int64_t R = m > n ? m : n;
  if (R <= 64 && k <= 64) return 0;
  if (R > BATCH_LDS_BUDGET / 8 || width_of(k) > BATCH_LDS_BUDGET / 8) return 2;
  return lds_bytes_solve(m, n, k) <= BATCH_LDS_BUDGET ? 1 : 2;
}

int m4ri_amd_pluq_solve_left_batch_dev(const word *A, int64_t a_stride, int64_t a_bs, int64_t m, int64_t n, const int32_t *rank, const int32_t *P,
                                       const int32_t *Q, word *B, int64_t b_stride, int64_t b_bs, int64_t k, int64_t batch, int32_t *status,
                                       void *stream) {
  if (m < 0 || n < 0 || k < 0 || batch < 0 || a_stride < 0 || a_bs < 0 || b_stride < 0 || b_bs < 0) return (int)hipErrorInvalidValue;
  const int64_t R = m > n ? m : n, wa = width_of(n), wb = width_of(k);
  if (a_stride < wa || b_stride < wb) return (int)hipErrorInvalidValue;
  if (!members_fit(batch, b_bs, R, b_stride, wb)) return (int)hipErrorInvalidValue;
  if (batch > 0 && (!status || !rank || (m > 0 && !P) || (n > 0 && !Q))) return (int)hipErrorInvalidValue;
  const bool a_data = m > 0 && n > 0, b_data = R > 0 && k > 0;
  if (batch > 0 && ((a_data && !A) || (b_data && !B))) return (int)hipErrorInvalidValue;
  // B's span and A's span (first member's start to last member's end) must not meet
  if (spans_meet(rows_span(B, batch, b_bs, R, b_stride, wb), rows_span(A, batch, a_bs, m, a_stride, wa))) return (int)hipErrorInvalidValue;
  if (batch == 0) return 0;
  hipStream_t st = (hipStream_t)stream;
  if (k == 0) return (int)hipMemsetAsync(status, 0, (size_t)batch * 4, st);  // no right-hand side: nothing to contradict
  const int path = m4ri_amd_plan_pluq_solve_batch(m, n, k);
  if (path == 2) return run_solve_path2(A, a_stride, a_bs, m, n, rank, P, Q, B, b_stride, b_bs, k, batch, status, st);
  if (path == 0)
    return launch_waves(batch, [&](dim3 grid, int64_t b0, int64_t) {
      hipLaunchKernelGGL(ps_wave_kernel, grid, dim3(BATCH_WAVE_THREADS), 0, st, A, a_stride, a_bs, (int)m, (int)n, rank, P, Q, B, b_stride, b_bs, (int)k, b0,
                         batch, status);
    });
  HIPTRY(set_max_dynamic_lds(BATCH_LDS_BUDGET, ps_block_kernel));
  const int threads = block_threads(R, wb);
  const size_t lds  = (size_t)lds_bytes_solve(m, n, k);
  return launch_members(batch, [&](dim3 grid, int64_t b0) {
    hipLaunchKernelGGL(ps_block_kernel, grid, dim3(threads), lds, st, A, a_stride, a_bs, (int)m, (int)n, rank, P, Q, B, b_stride, b_bs,
                       (int)k, (int)lds_row_words(wb), b0, status);
  });
}

}  // extern "C"
