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
//   1  the member fits in LDS: a workgroup per member, rows staged in LDS under a row-permutation index as echelon_batch.hip's path 1,
//      P and Q beside them; two barriers per column with a pivot; the compression is a loop of bit swaps per row, a thread per row.
//   2  larger members up to PB_CAP_BYTES: a workgroup per member, rows in place in global memory, whole rows swapped physically (the
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
#include <mutex>
#include <vector>
#include "gf2_internal.h"
#include "../../include/m4ri_amd.h"

namespace {

constexpr int PB_WAVE_THREADS   = 256;                 // path 0: four members per workgroup
constexpr int PB_MAX_THREADS    = 1024;                // the workgroup paths
constexpr int64_t PB_LDS_BUDGET = 160 * 1024;          // path 1: the whole LDS of a CU
constexpr int64_t PB_CAP_BYTES  = 512 * 1024;          // path 2 of the decomposition: valid words of a member, bytes
constexpr int64_t PB_CHUNK      = (int64_t)1 << 30;    // workgroups per launch

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
__global__ __launch_bounds__(PB_WAVE_THREADS) void pb_wave_kernel(word *__restrict__ A, int64_t stride, int64_t a_bs, int nrows, int ncols,
                                                                  int64_t b0, int64_t batch, int pluq, int32_t *__restrict__ P,
                                                                  int32_t *__restrict__ Q, int32_t *__restrict__ rank_out) {
  const int lane  = threadIdx.x & 63;
  const int64_t b = b0 + (int64_t)blockIdx.x * (PB_WAVE_THREADS / 64) + (threadIdx.x >> 6);
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

__host__ __device__ inline size_t pad16(size_t bytes) { return (bytes + 15) & ~(size_t)15; }

// paths 1 (INLDS) and 2: a workgroup per member.  Dynamic LDS (16-byte carve offsets):
//   INLDS: rows [nrows][ldw] words | perm [nrows] int32 | P [nrows] int32 | Q [ncols] int32 (each rounded up to 16 B) | flags [2][nfw] words
//   else:  flags [2][nfw] words; P and Q are the output arrays
// Row i of the flag pass is owned by thread i % blockDim.x (the lane of its ballot); flags[c & 1] bit i = bit c of logical row i.
template <bool INLDS>
__global__ __launch_bounds__(PB_MAX_THREADS) void pb_block_kernel(word *__restrict__ A, int64_t stride, int64_t a_bs, int nrows, int ncols,
                                                                  int ldw, int64_t b0, int pluq, int32_t *__restrict__ P_out,
                                                                  int32_t *__restrict__ Q_out, int32_t *__restrict__ rank_out) {
  extern __shared__ __attribute__((aligned(16))) char pb_smem[];
  const int T = blockDim.x, t = threadIdx.x, lane = t & 63;
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
    const int total = nrows * width;
    for (int k = t; k < total; k += T) {
      const int i = k / width, w = k - i * width;
      word x = g[(int64_t)i * stride + w];
      if (w == width - 1) x &= mask;
      rows[i * ldw + w] = x;
    }
    for (int i = t; i < nrows; i += T) perm[i] = i;
  }
  for (int i = t; i < nrows; i += T) Pv[i] = i;
  for (int j = t; j < ncols; j += T) Qv[j] = j;
  __syncthreads();

  int rank = 0;
  int sw_r = -1, sw_p = -1, sw_R = 0, sw_P = 0;  // INLDS: the previous column's pending swap of perm[rank] and perm[p]
  for (int c = 0; c < ncols && rank < nrows; ++c) {
    word *buf    = flags + (c & 1) * nfw;
    const int cw = c >> 6, cb = c & 63;
    // flag pass: each thread its own rows (and, INLDS, their index entries)
    for (int base = t - lane; base < nrows; base += T) {
      const int i = base + lane;
      int bit     = 0;
      if (i < nrows) {
        word x;
        if (INLDS) {
          int ph = (i == sw_r) ? sw_P : (i == sw_p) ? sw_R : perm[i];
          if (i == sw_r || i == sw_p) perm[i] = ph;
          x = rows[ph * ldw + cw];
        } else {
          x = g[(int64_t)i * stride + cw];
        }
        bit = (int)((x >> cb) & 1);
      }
      const word bal = __ballot(bit);
      if (lane == 0) buf[base >> 6] = bal;
    }
    sw_r = sw_p = -1;
    __syncthreads();
    int p = -1;
    for (int j = rank >> 6; j < nfw; ++j) {
      word f = buf[j];
      if (j == (rank >> 6)) f &= ~(word)0 << (rank & 63);
      if (f) {
        p = j * 64 + (int)__builtin_ctzll(f);
        break;
      }
    }
    if (p < 0) continue;  // no writes this column; the next flag pass uses the other buffer
    if (t == 0) {
      Pv[rank] = p;
      Qv[rank] = c;
    }
    const word *prow;
    if (INLDS) {
      const int Pp = perm[p];
      prow         = rows + Pp * ldw;
      if (p != rank) {
        sw_r = rank; sw_p = p; sw_P = Pp; sw_R = perm[rank];
      }
    } else {
      if (p != rank) {  // physical swap of the whole rows (the multipliers to the left move too), the bits behind ncols stay
        word *rp = g + (int64_t)rank * stride, *pp = g + (int64_t)p * stride;
        for (int w = t; w < width; w += T) {
          const word x = rp[w], y = pp[w];
          if (w == width - 1) {
            rp[w] = (y & mask) | (x & ~mask);
            pp[w] = (x & mask) | (y & ~mask);
          } else {
            rp[w] = y;
            pp[w] = x;
          }
        }
        __syncthreads();
      }
      prow = g + (int64_t)rank * stride;
    }
    // the update: flagged rows i > rank, i != p (row p holds the old row `rank`, which had no bit c), columns c + 1 .. ncols - 1.
    // Item k = (i, w) with k = (i - rank - 1) * nw + (w - cw), k = t, t + T, ...: advanced by (qi, qw) without a division per item.
    {
      const word first = cb < 63 ? ~(word)0 << (cb + 1) : 0;
      const int nw = width - cw;
      const int qi = T / nw, qw = T - qi * nw;
      int i = rank + 1 + t / nw, w = cw + (t - (t / nw) * nw);
      while (i < nrows) {
        const int f = (int)((buf[i >> 6] >> (i & 63)) & 1);
        if (f && i != p) {
          word x = prow[w];
          if (w == cw) x &= first;
          if (INLDS) {
            rows[perm[i] * ldw + w] ^= x;
          } else {
            if (w == width - 1) x &= mask;
            g[(int64_t)i * stride + w] ^= x;
          }
        }
        i += qi;
        w += qw;
        if (w >= width) {
          w -= nw;
          ++i;
        }
      }
    }
    ++rank;
    __syncthreads();
  }

  if (INLDS) {
    if (sw_r >= 0) {  // the last column's swap (its owners only, as in the flag pass)
      for (int i = t; i < nrows; i += T)
        if (i == sw_r) perm[i] = sw_P;
        else if (i == sw_p) perm[i] = sw_R;
    }
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
    const int total = nrows * width;
    for (int k = t; k < total; k += T) {
      const int i = k / width, w = k - i * width;
      word x      = rows[perm[i] * ldw + w];
      word *dst   = g + (int64_t)i * stride + w;
      if (w == width - 1 && mask != ~(word)0) x = (x & mask) | (*dst & ~mask);
      *dst = x;
    }
    for (int i = t; i < nrows; i += T) Pg[i] = Pv[i];
    for (int j = t; j < ncols; j += T) Qg[j] = Qv[j];
  }
  if (t == 0) rank_out[b] = rank;
}

// nrows == 0 or ncols == 0: rank 0, P and Q the identity
__global__ void pb_identity_kernel(int32_t *__restrict__ P, int64_t nrows, int32_t *__restrict__ Q, int64_t ncols, int32_t *__restrict__ rank,
                                   int64_t batch) {
  const int64_t step = (int64_t)gridDim.x * blockDim.x;  // grid-stride: the grid is capped at PB_CHUNK workgroups
  for (int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; k < batch * nrows || k < batch * ncols || k < batch; k += step) {
    if (k < batch * nrows) P[k] = (int32_t)(k % nrows);
    if (k < batch * ncols) Q[k] = (int32_t)(k % ncols);
    if (k < batch) rank[k] = 0;
  }
}

int64_t lds_row_words(int64_t width) { return width + ((width & 1) ^ 1); }  // odd: the flag pass reads one word per row

int64_t lds_bytes_ple(int64_t nrows, int64_t ncols) {
  return nrows * lds_row_words(words_of(ncols)) * 8 + 2 * (int64_t)pad16((size_t)nrows * 4) + (int64_t)pad16((size_t)ncols * 4) +
         2 * ((nrows + 63) / 64) * 8;
}

int block_threads(int64_t rows, int64_t width) { return rows * width >= 8192 ? PB_MAX_THREADS : 256; }

// a clean copy (tail bits zero) of the rows x ncols matrix at src into scratch
int clean_copy(word *dst, int64_t dst_stride, const word *src, int64_t src_stride, int64_t rows, int64_t ncols, hipStream_t st) {
  HIPTRY(hipMemsetAsync(dst, 0, (size_t)(rows * dst_stride) * 8, st));
  HIPTRY(gf2_launch_copy_masked(st, dst, dst_stride, src, src_stride, rows, ncols));
  return 0;
}

int run_ple_path3(word *A, int64_t stride, int64_t a_bs, int64_t nrows, int64_t ncols, int64_t batch, int pluq, int32_t *P, int32_t *Q,
                  int32_t *rank, hipStream_t st) {
  const int64_t width = words_of(ncols);
  std::vector<int32_t> hp((size_t)(batch * nrows)), hq((size_t)(batch * ncols)), hr((size_t)batch);
  word *s = nullptr;
  auto run = [&]() -> int {
    HIPTRY(hipMalloc(reinterpret_cast<void **>(&s), (size_t)(nrows * width) * 8));
    for (int64_t b = 0; b < batch; ++b) {
      word *Ab = A + b * a_bs;
      if (int rc = clean_copy(s, width, Ab, stride, nrows, ncols, st)) return rc;
      int32_t *p = &hp[(size_t)(b * nrows)], *q = &hq[(size_t)(b * ncols)];
      if (int rc = pluq ? m4ri_amd_pluq_dev(s, width, nrows, ncols, p, q, &hr[(size_t)b], 0, st)
                        : m4ri_amd_ple_dev(s, width, nrows, ncols, p, q, &hr[(size_t)b], 0, st))
        return rc;
      HIPTRY(gf2_launch_copy_masked(st, Ab, stride, s, width, nrows, ncols));
    }
    HIPTRY(hipMemcpyAsync(P, hp.data(), hp.size() * 4, hipMemcpyHostToDevice, st));
    HIPTRY(hipMemcpyAsync(Q, hq.data(), hq.size() * 4, hipMemcpyHostToDevice, st));
    HIPTRY(hipMemcpyAsync(rank, hr.data(), hr.size() * 4, hipMemcpyHostToDevice, st));
    return (int)hipStreamSynchronize(st);
  };
  const int rc = run();
  if (rc) (void)hipStreamSynchronize(st);
  if (s) (void)hipFree(s);
  return rc;
}

// ---- the solve from the factors -------------------------------------------------------------------------------------------------

__device__ __forceinline__ int clamp_rank(int r, int m, int n) {
  const int mn = m < n ? m : n;
  return r < 0 ? 0 : r > mn ? mn : r;
}

// path 0: a wave per member, lane i = row i of B (x) and of A (a), lane t = P[t] and Q[t].  fb: the member whose decomposition is
// used (0 when one serves all).
__global__ __launch_bounds__(PB_WAVE_THREADS) void ps_wave_kernel(const word *__restrict__ A, int64_t a_stride, int64_t a_bs, int m, int n,
                                                                  const int32_t *__restrict__ rank_in, const int32_t *__restrict__ P,
                                                                  const int32_t *__restrict__ Q, word *__restrict__ B, int64_t b_stride,
                                                                  int64_t b_bs, int k, int64_t b0, int64_t batch, int32_t *__restrict__ status) {
  const int lane  = threadIdx.x & 63;
  const int64_t b = b0 + (int64_t)blockIdx.x * (PB_WAVE_THREADS / 64) + (threadIdx.x >> 6);
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
__global__ __launch_bounds__(PB_MAX_THREADS) void ps_block_kernel(const word *__restrict__ A, int64_t a_stride, int64_t a_bs, int m, int n,
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
  for (int q = t; q < total; q += T) {
    const int i = q / wb, w = q - i * wb;
    word x = gb[(int64_t)i * b_stride + w];
    if (w == wb - 1) x &= bmask;
    rows[i * ldw + w] = x;
  }
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
      word x      = idx[i] < 0 ? 0 : rows[idx[i] * ldw + w];
      word *dst   = gb + (int64_t)i * b_stride + w;
      if (w == wb - 1 && bmask != ~(word)0) x = (x & bmask) | (*dst & ~bmask);
      *dst = x;
    }
  }
  if (t == 0) status[b] = bad ? -1 : 0;
}

int64_t lds_bytes_solve(int64_t m, int64_t n, int64_t k) {
  const int64_t R = m > n ? m : n, mn = m < n ? m : n;
  return R * lds_row_words(words_of(k)) * 8 + (int64_t)pad16((size_t)R * 4) + (int64_t)pad16((size_t)mn * 4) + 16 + m * 8;
}

// path 2 helper: are rows r0 .. r1-1 of the k-column matrix at M (stride words) all zero?  Copies them to the host.  Blocking.
int rows_zero(const word *M, int64_t stride, int64_t r0, int64_t r1, int64_t k, hipStream_t st, bool *zero) {
  *zero = true;
  const int64_t w = words_of(k);
  if (r1 <= r0 || w == 0) return 0;
  std::vector<word> h((size_t)((r1 - r0) * w));
  HIPTRY(hipMemcpy2DAsync(h.data(), (size_t)w * 8, M + r0 * stride, (size_t)stride * 8, (size_t)w * 8, (size_t)(r1 - r0), hipMemcpyDeviceToHost, st));
  HIPTRY(hipStreamSynchronize(st));
  const word mask = (k & 63) ? (((word)1 << (k & 63)) - 1) : ~(word)0;
  for (int64_t i = 0; i < r1 - r0; ++i)
    for (int64_t j = 0; j < w; ++j)
      if (h[(size_t)(i * w + j)] & (j == w - 1 ? mask : ~(word)0)) {
        *zero = false;
        return 0;
      }
  return 0;
}

// path 2: rank, P and Q to the host once; per member B's padding rows m .. R-1 checked, then m4ri_amd_pluq_solve_left_dev with the
// check on clean copies of A_b (once when shared) and B_b, and X copied back only when it exists.  (R > 64 or k > 64 here, so k > 0.)
int run_solve_path2(const word *A, int64_t a_stride, int64_t a_bs, int64_t m, int64_t n, const int32_t *rank, const int32_t *P, const int32_t *Q,
                    word *B, int64_t b_stride, int64_t b_bs, int64_t k, int64_t batch, int32_t *status, hipStream_t st) {
  const int64_t R = m > n ? m : n, mn = m < n ? m : n, wa = words_of(n), wb = words_of(k), nf = a_bs ? batch : 1;
  std::vector<int32_t> hs((size_t)batch), hr((size_t)nf), hp((size_t)(nf * m)), hq((size_t)(nf * n));
  word *sA = nullptr, *sB = nullptr;
  auto run = [&]() -> int {
    HIPTRY(hipMemcpyAsync(hr.data(), rank, hr.size() * 4, hipMemcpyDeviceToHost, st));
    if (!hp.empty()) HIPTRY(hipMemcpyAsync(hp.data(), P, hp.size() * 4, hipMemcpyDeviceToHost, st));
    if (!hq.empty()) HIPTRY(hipMemcpyAsync(hq.data(), Q, hq.size() * 4, hipMemcpyDeviceToHost, st));
    HIPTRY(hipStreamSynchronize(st));
    if (mn > 0) HIPTRY(hipMalloc(reinterpret_cast<void **>(&sA), (size_t)(m * wa) * 8));
    HIPTRY(hipMalloc(reinterpret_cast<void **>(&sB), (size_t)(R * wb) * 8));
    for (int64_t b = 0; b < batch; ++b) {
      const int64_t fb = a_bs ? b : 0;
      word *Bb         = B + b * b_bs;
      int32_t r        = hr[(size_t)fb];
      r                = r < 0 ? 0 : r > mn ? (int32_t)mn : r;
      bool zero        = true;
      if (int rc = rows_zero(Bb, b_stride, mn > 0 ? m : 0, R, k, st, &zero)) return rc;  // A empty: every row of B
      int ret = zero ? 0 : -1;
      if (ret == 0 && mn > 0) {
        if (b == 0 || a_bs)
          if (int rc = clean_copy(sA, wa, A + b * a_bs, a_stride, m, n, st)) return rc;
        if (int rc = clean_copy(sB, wb, Bb, b_stride, R, k, st)) return rc;
        if (int rc = m4ri_amd_pluq_solve_left_dev(sA, wa, m, n, r, &hp[(size_t)(fb * m)], &hq[(size_t)(fb * n)], sB, wb, R, k, 0, 1, &ret, st)) return rc;
        if (ret == 0) HIPTRY(gf2_launch_copy_masked(st, Bb, b_stride, sB, wb, R, k));
      }
      hs[(size_t)b] = ret;
    }
    HIPTRY(hipMemcpyAsync(status, hs.data(), (size_t)batch * 4, hipMemcpyHostToDevice, st));
    return (int)hipStreamSynchronize(st);
  };
  const int rc = run();
  if (rc) (void)hipStreamSynchronize(st);
  if (sA) (void)hipFree(sA);
  if (sB) (void)hipFree(sB);
  return rc;
}

}  // namespace

extern "C" {

int m4ri_amd_plan_ple_batch(int64_t nrows, int64_t ncols) {
  if (nrows < 0 || ncols < 0) return -1;
  if (nrows <= 64 && ncols <= 64) return 0;
  const int64_t width = words_of(ncols);
  if (nrows > PB_CAP_BYTES / 8 || width > PB_CAP_BYTES / 8 || nrows * width > PB_CAP_BYTES / 8) return 3;
  return lds_bytes_ple(nrows, ncols) <= PB_LDS_BUDGET ? 1 : 2;
}

int m4ri_amd_ple_batch_dev(word *A, int64_t stride, int64_t a_bs, int64_t nrows, int64_t ncols, int64_t batch, int pluq, int32_t *P, int32_t *Q,
                           int32_t *rank, void *stream) {
  if (nrows < 0 || ncols < 0 || batch < 0 || stride < 0 || a_bs < 0) return (int)hipErrorInvalidValue;
  const int64_t width = words_of(ncols);
  if (stride < width) return (int)hipErrorInvalidValue;
  if (batch > 1 && nrows > 0 && a_bs < (nrows - 1) * stride + width) return (int)hipErrorInvalidValue;
  if (batch > 0 && (!rank || (nrows > 0 && !P) || (ncols > 0 && !Q))) return (int)hipErrorInvalidValue;
  if (batch > 0 && nrows > 0 && ncols > 0 && !A) return (int)hipErrorInvalidValue;
  if (batch == 0) return 0;
  hipStream_t st = (hipStream_t)stream;
  if (nrows == 0 || ncols == 0) {
    const int64_t total = batch * (nrows > ncols ? nrows : ncols > 0 ? ncols : 1), blocks = (total + 255) / 256;
    hipLaunchKernelGGL(pb_identity_kernel, dim3((unsigned)(blocks < PB_CHUNK ? blocks : PB_CHUNK)), dim3(256), 0, st, P, nrows, Q, ncols, rank, batch);
    return (int)hipGetLastError();
  }
  const int path = m4ri_amd_plan_ple_batch(nrows, ncols);
  if (path == 0) {
    const int64_t per = PB_WAVE_THREADS / 64;
    for (int64_t b0 = 0; b0 < batch; b0 += PB_CHUNK * per) {
      const int64_t n = (batch - b0 < PB_CHUNK * per) ? batch - b0 : PB_CHUNK * per;
      hipLaunchKernelGGL(pb_wave_kernel, dim3((unsigned)((n + per - 1) / per)), dim3(PB_WAVE_THREADS), 0, st, A, stride, a_bs, (int)nrows, (int)ncols,
                         b0, batch, pluq, P, Q, rank);
      HIPTRY(hipGetLastError());
    }
    return 0;
  }
  if (path == 3) return run_ple_path3(A, stride, a_bs, nrows, ncols, batch, pluq, P, Q, rank, st);
  const bool inlds  = path == 1;
  const int threads = block_threads(nrows, width);
  const int ldw     = inlds ? (int)lds_row_words(width) : 0;
  const size_t lds  = inlds ? (size_t)lds_bytes_ple(nrows, ncols) : (size_t)(2 * ((nrows + 63) / 64) * 8);
  static std::once_flag once;
  std::call_once(once, [] {
    (void)hipFuncSetAttribute(reinterpret_cast<const void *>(pb_block_kernel<true>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)PB_LDS_BUDGET);
    (void)hipFuncSetAttribute(reinterpret_cast<const void *>(pb_block_kernel<false>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)PB_LDS_BUDGET);
  });
  for (int64_t b0 = 0; b0 < batch; b0 += PB_CHUNK) {
    const int64_t n = (batch - b0 < PB_CHUNK) ? batch - b0 : PB_CHUNK;
    if (inlds)
      hipLaunchKernelGGL(pb_block_kernel<true>, dim3((unsigned)n), dim3(threads), lds, st, A, stride, a_bs, (int)nrows, (int)ncols, ldw, b0, pluq, P, Q,
                         rank);
    else
      hipLaunchKernelGGL(pb_block_kernel<false>, dim3((unsigned)n), dim3(threads), lds, st, A, stride, a_bs, (int)nrows, (int)ncols, ldw, b0, pluq, P, Q,
                         rank);
    HIPTRY(hipGetLastError());
  }
  return 0;
}

int m4ri_amd_plan_pluq_solve_batch(int64_t m, int64_t n, int64_t k) {
  if (m < 0 || n < 0 || k < 0) return -1;
  const int64_t R = m > n ? m : n;
  if (R <= 64 && k <= 64) return 0;
  if (R > PB_LDS_BUDGET / 8 || words_of(k) > PB_LDS_BUDGET / 8) return 2;
  return lds_bytes_solve(m, n, k) <= PB_LDS_BUDGET ? 1 : 2;
}

int m4ri_amd_pluq_solve_left_batch_dev(const word *A, int64_t a_stride, int64_t a_bs, int64_t m, int64_t n, const int32_t *rank, const int32_t *P,
                                       const int32_t *Q, word *B, int64_t b_stride, int64_t b_bs, int64_t k, int64_t batch, int32_t *status,
                                       void *stream) {
  if (m < 0 || n < 0 || k < 0 || batch < 0 || a_stride < 0 || a_bs < 0 || b_stride < 0 || b_bs < 0) return (int)hipErrorInvalidValue;
  const int64_t R = m > n ? m : n, wa = words_of(n), wb = words_of(k);
  if (a_stride < wa || b_stride < wb) return (int)hipErrorInvalidValue;
  if (batch > 1 && R > 0 && b_bs < (R - 1) * b_stride + wb) return (int)hipErrorInvalidValue;
  if (batch > 0 && (!status || !rank || (m > 0 && !P) || (n > 0 && !Q))) return (int)hipErrorInvalidValue;
  const bool a_data = m > 0 && n > 0, b_data = R > 0 && k > 0;
  if (batch > 0 && ((a_data && !A) || (b_data && !B))) return (int)hipErrorInvalidValue;
  if (batch > 0 && a_data && b_data) {  // B's span and A's span (first member's start to last member's end) must not meet
    const uintptr_t bi = (uintptr_t)B, ai = (uintptr_t)A;
    const uintptr_t bend = bi + (uintptr_t)(((batch - 1) * b_bs + (R - 1) * b_stride + wb) * 8);
    const uintptr_t aend = ai + (uintptr_t)(((batch - 1) * a_bs + (m - 1) * a_stride + wa) * 8);
    if (bi < aend && ai < bend) return (int)hipErrorInvalidValue;
  }
  if (batch == 0) return 0;
  hipStream_t st = (hipStream_t)stream;
  if (k == 0) return (int)hipMemsetAsync(status, 0, (size_t)batch * 4, st);  // no right-hand side: nothing to contradict
  const int path = m4ri_amd_plan_pluq_solve_batch(m, n, k);
  if (path == 2) return run_solve_path2(A, a_stride, a_bs, m, n, rank, P, Q, B, b_stride, b_bs, k, batch, status, st);
  if (path == 0) {
    const int64_t per = PB_WAVE_THREADS / 64;
    for (int64_t b0 = 0; b0 < batch; b0 += PB_CHUNK * per) {
      const int64_t cnt = (batch - b0 < PB_CHUNK * per) ? batch - b0 : PB_CHUNK * per;
      hipLaunchKernelGGL(ps_wave_kernel, dim3((unsigned)((cnt + per - 1) / per)), dim3(PB_WAVE_THREADS), 0, st, A, a_stride, a_bs, (int)m, (int)n, rank,
                         P, Q, B, b_stride, b_bs, (int)k, b0, batch, status);
      HIPTRY(hipGetLastError());
    }
    return 0;
  }
  static std::once_flag once;
  std::call_once(once, [] {
    (void)hipFuncSetAttribute(reinterpret_cast<const void *>(ps_block_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)PB_LDS_BUDGET);
  });
  const int threads = block_threads(R, wb);
  const size_t lds  = (size_t)lds_bytes_solve(m, n, k);
  for (int64_t b0 = 0; b0 < batch; b0 += PB_CHUNK) {
    const int64_t cnt = (batch - b0 < PB_CHUNK) ? batch - b0 : PB_CHUNK;
    hipLaunchKernelGGL(ps_block_kernel, dim3((unsigned)cnt), dim3(threads), lds, st, A, a_stride, a_bs, (int)m, (int)n, rank, P, Q, B, b_stride, b_bs,
                       (int)k, (int)lds_row_words(wb), b0, status);
    HIPTRY(hipGetLastError());
  }
  return 0;
}

}  // extern "C"
