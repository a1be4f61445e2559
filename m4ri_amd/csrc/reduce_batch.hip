// reduce_batch.hip -- the read side of the batched calls: Hamming weights, the first differing row and the span of the non-zero
// rows of many matrices of one shape, one call for the batch, every result left on the device.
//
// The three entry points are one reduction.  Row i of member b has the weight w = popcount((A_b[i] ^ B_b[i]) & valid bits) (B absent:
// of A_b[i]); from it come the member's total (the sum), its row weights, its lightest row (the minimum of (w << 32) | i), its
// first non-zero row (the minimum i with w != 0) and one past its last (the maximum i + 1).  m4ri_amd_weight_batch_dev asks for the
// first three, m4ri_amd_mismatch_batch_dev for the fourth on A ^ B, m4ri_amd_row_span_batch_dev for the last two on A.
// The paths (m4ri_amd_plan_reduce_batch):
//   0  nrows <= 64 and at most RDB_W0 words per row: a wave per member, four members per workgroup.  Lane i holds row i's weight;
//      sum and minimum go across the lanes in 32 bits, the two row positions come from one ballot.  No LDS, no atomics.
//   1  nrows * words(ncols) <= RDB_T1: a workgroup per member.  A row belongs to L lanes of a wave (L the power of two that covers
//      the row's words, or pairs of words, at most 64), a wave takes 64 / L rows at a time; the four waves meet in LDS.
//   2  everything else: the rows of a member cut into chunks of about RDB_CHUNK_WORDS words, a workgroup of path 1's kernel per
//      (chunk, member); the per-member results are combined with global atomics (64-bit add and min, 32-bit min and max) on outputs an
//      initialisation kernel on the same stream has set.  All integers: the order of arrival changes nothing.  A call that wants row
//      positions only leaves a chunk unread once the output already holds an answer no row of the chunk can improve.
// On paths 0 and 1 every output word is written exactly once with a plain store.  Words are loaded 16 bytes at a time where every
// operand's base is 16-byte aligned and its strides are even, 8 bytes otherwise.  Every path is plain launches on the caller's stream:
// no allocation, no copy to the host, no synchronisation, no engine workspace or lock.
#include <hip/hip_runtime.h>
#include <limits.h>
#include "batch_common.h"
#include "../../include/m4ri_amd.h"

namespace {

// Path 0 up to this many words per row, path 1 up to this many words per member (nrows * words(ncols)).  Measured
// (tools/bench_reduce_batch.py, profiles/reduce_batch_bench.txt) on 256 MB of dense members, the weight call with all
// three outputs, every spread under 1 %: at 64 rows of 1 / 2 / 4 / 8 words path 0 beats path 1 6.5x / 5.7x / 4.0x / 2.1x and loses to it
// at 16 words (0.25x): W0 = 8.  On the squares of 64 ... 1024 path 1 is ahead of path 2 by 1 % ... 7 %, each time by more than the
// spread, and at 2048 it loses (0.38x: one workgroup per member no longer fills the device): T1 = 1024 * 1024 / 64.
// M4RI_AMD_REDUCE_BATCH_PATH0_MAX and M4RI_AMD_REDUCE_BATCH_PATH1_MAX override them for the routing of a call.
constexpr int64_t RDB_W0          = 8;
constexpr int64_t RDB_W0_MAX      = 16;                 // the largest path-0 bound: a row weight fits (w << 6) | lane in 32 bits
constexpr int64_t RDB_T1          = 16384;
constexpr int64_t RDB_T1_MAX      = (int64_t)1 << 30;   // the largest path-1 bound
constexpr int64_t RDB_CHUNK_WORDS = 16384;              // path 2: the words of a workgroup's rows (128 KiB)
constexpr int RDB_WAVES           = BATCH_WAVE_THREADS / 64;

struct RedArgs {
  const word *A, *B;  // B may be NULL
  int64_t a_stride, a_bs, b_stride, b_bs;
  int64_t nrows, width;  // width = words(ncols) >= 1
  word mask;             // of a row's last word
  int64_t *total;        // the outputs, each may be NULL
  int32_t *row_weight;
  int64_t *lightest;
  int32_t *first, *end;
  int32_t first_none;     // first[b] of a member without a non-zero row: nrows or -1
  int64_t b0, batch;      // this launch: members b0 .. batch - 1
  int lshift;             // paths 1 and 2: L = 1 << lshift lanes per row
  int64_t chunk_rows, chunks;  // paths 1 and 2: rows per workgroup, workgroups per member
};

// the weight of this lane's share of a row of A ^ B: words (VEC: pairs of words) g, g + L, ... of `width`.  A pair is loaded as 16
// bytes only where both words are the row's own: the word behind an odd width may lie behind the operand's last byte.
template <bool VEC>
__device__ __forceinline__ int row_part(const word *__restrict__ a, const word *__restrict__ b, int64_t width, word mask, int g, int L) {
  int c = 0;
  if (VEC) {
    for (int64_t w = 2 * (int64_t)g; w < width; w += 2 * (int64_t)L) {
      word x0, x1 = 0;
      if (w + 1 < width) {
        const ulonglong2 va = *reinterpret_cast<const ulonglong2 *>(a + w);
        x0 = va.x;
        x1 = va.y;
        if (b) {
          const ulonglong2 vb = *reinterpret_cast<const ulonglong2 *>(b + w);
          x0 ^= vb.x;
          x1 ^= vb.y;
        }
        if (w + 2 == width) x1 &= mask;
      } else {
        x0 = a[w];
        if (b) x0 ^= b[w];
        x0 &= mask;
      }
      c += __popcll(x0) + __popcll(x1);
    }
  } else {
    for (int64_t w = g; w < width; w += L) {
      word x = a[w];
      if (b) x ^= b[w];
      if (w + 1 == width) x &= mask;
      c += __popcll(x);
    }
  }
  return c;
}

// path 0: a wave per member, members b0 + 4 * blockIdx.x + wave; lane i holds row i.
template <bool VEC>
__global__ __launch_bounds__(BATCH_WAVE_THREADS) void red_wave_kernel(RedArgs p) {
  const int lane  = threadIdx.x & 63;
  const int64_t b = p.b0 + (int64_t)blockIdx.x * RDB_WAVES + (threadIdx.x >> 6);
  if (b >= p.batch) return;  // wave-uniform, no barrier in this kernel
  const int nrows = (int)p.nrows;
  int w           = 0;
  if (lane < nrows)
    w = row_part<VEC>(p.A + b * p.a_bs + (int64_t)lane * p.a_stride, p.B ? p.B + b * p.b_bs + (int64_t)lane * p.b_stride : nullptr, p.width, p.mask, 0, 1);
  if (p.row_weight && lane < nrows) p.row_weight[b * p.nrows + lane] = w;
  if (p.total) {
    int s = w;
    for (int o = 32; o; o >>= 1) s += __shfl_xor(s, o);
    if (lane == 0) p.total[b] = s;
  }
  if (p.lightest) {  // w <= 64 * RDB_W0_MAX: (w << 6) | lane fits
    int k = lane < nrows ? (w << 6) | lane : INT_MAX;
    for (int o = 32; o; o >>= 1) k = min(k, __shfl_xor(k, o));
    if (lane == 0) p.lightest[b] = ((int64_t)(k >> 6) << 32) | (k & 63);
  }
  if (p.first || p.end) {
    const word bal = __ballot(w != 0);
    if (lane == 0) {
      if (p.first) p.first[b] = bal ? (int32_t)__builtin_ctzll(bal) : p.first_none;
      if (p.end) p.end[b] = bal ? 64 - (int32_t)__builtin_clzll(bal) : 0;
    }
  }
}

// paths 1 and 2: workgroup t of the launch takes chunk t % chunks of member b0 + t / chunks, rows [r0, r1).  ATOMIC: the member's
// results are combined across its workgroups in the outputs, which red_init_kernel has set; else chunks == 1 and they are stored.
template <bool VEC, bool ATOMIC>
__global__ __launch_bounds__(BATCH_WAVE_THREADS) void red_block_kernel(RedArgs p) {
  __shared__ int64_t s_tot[RDB_WAVES], s_key[RDB_WAVES];
  __shared__ uint32_t s_first[RDB_WAVES];
  __shared__ int32_t s_end[RDB_WAVES];
  __shared__ int s_skip;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t t = blockIdx.x;
  const int64_t b = p.b0 + t / p.chunks;
  int64_t c       = t % p.chunks;
  const bool weights = p.total || p.row_weight || p.lightest;
  if (ATOMIC && !weights && !p.first) c = p.chunks - 1 - c;  // the last row alone: from the bottom, so that the early leave below bites
  const int64_t r0 = c * p.chunk_rows, r1 = r0 + p.chunk_rows < p.nrows ? r0 + p.chunk_rows : p.nrows;
  if (ATOMIC && !weights) {  // row positions only: is there anything a row of [r0, r1) could still improve?  One thread asks for all.
    if (threadIdx.x == 0) {
      bool done = true;
      if (p.first)
        done = done && __hip_atomic_load(reinterpret_cast<uint32_t *>(p.first + b), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) <= (uint32_t)r0;
      if (p.end) done = done && __hip_atomic_load(p.end + b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >= (int32_t)r1;
      s_skip = done;
    }
    __syncthreads();
    if (s_skip) return;  // workgroup-uniform
  }
  const int L = 1 << p.lshift, g = lane & (L - 1), sub = lane >> p.lshift, rpw = 64 >> p.lshift;
  const word *A = p.A + b * p.a_bs, *B = p.B ? p.B + b * p.b_bs : nullptr;
  int64_t tot = 0, key = INT64_MAX;
  uint32_t first = UINT32_MAX;
  int32_t end    = 0;
  for (int64_t base = r0 + (int64_t)wave * rpw; base < r1; base += (int64_t)RDB_WAVES * rpw) {  // wave-uniform
    const int64_t i = base + sub;
    int w           = 0;
    if (i < r1) w = row_part<VEC>(A + i * p.a_stride, B ? B + i * p.b_stride : nullptr, p.width, p.mask, g, L);
    for (int o = L >> 1; o; o >>= 1) w += __shfl_xor(w, o);
    if (g == 0 && i < r1) {
      if (p.row_weight) p.row_weight[b * p.nrows + i] = w;
      tot += w;
      const int64_t k = ((int64_t)w << 32) | i;
      key = k < key ? k : key;
      if (w) {
        first = (uint32_t)i < first ? (uint32_t)i : first;
        end   = (int32_t)i + 1 > end ? (int32_t)i + 1 : end;
      }
    }
  }
  for (int o = 32; o; o >>= 1) {
    tot += __shfl_xor(tot, o);
    const int64_t k  = __shfl_xor(key, o);
    const uint32_t f = __shfl_xor(first, o);
    const int32_t e  = __shfl_xor(end, o);
    key   = k < key ? k : key;
    first = f < first ? f : first;
    end   = e > end ? e : end;
  }
  if (lane == 0) {
    s_tot[wave]   = tot;
    s_key[wave]   = key;
    s_first[wave] = first;
    s_end[wave]   = end;
  }
  __syncthreads();
  if (threadIdx.x != 0) return;
  for (int v = 1; v < RDB_WAVES; ++v) {
    tot += s_tot[v];
    key   = s_key[v] < key ? s_key[v] : key;
    first = s_first[v] < first ? s_first[v] : first;
    end   = s_end[v] > end ? s_end[v] : end;
  }
  if (ATOMIC) {  // the keys and rows are not negative: the unsigned minimum is the signed one, and a first[b] of -1 is the largest
    if (p.total && tot) atomicAdd(reinterpret_cast<unsigned long long *>(p.total + b), (unsigned long long)tot);
    if (p.lightest) atomicMin(reinterpret_cast<unsigned long long *>(p.lightest + b), (unsigned long long)key);
    if (p.first && first != UINT32_MAX) atomicMin(reinterpret_cast<uint32_t *>(p.first + b), first);
    if (p.end && end) atomicMax(p.end + b, end);
  } else {
    if (p.total) p.total[b] = tot;
    if (p.lightest) p.lightest[b] = key;
    if (p.first) p.first[b] = first == UINT32_MAX ? p.first_none : (int32_t)first;
    if (p.end) p.end[b] = end;
  }
}

// the per-member outputs of members b0 .. batch - 1: what path 2's atomics start from, and the results of empty members
__global__ __launch_bounds__(BATCH_WAVE_THREADS) void red_init_kernel(int64_t *total, int64_t *lightest, int64_t lightest_v, int32_t *first, int32_t first_v,
                                                                      int32_t *end, int64_t b0, int64_t batch) {
  for (int64_t b = b0 + (int64_t)blockIdx.x * BATCH_WAVE_THREADS + threadIdx.x; b < batch; b += (int64_t)gridDim.x * BATCH_WAVE_THREADS) {
    if (total) total[b] = 0;
    if (lightest) lightest[b] = lightest_v;
    if (first) first[b] = first_v;
    if (end) end[b] = 0;
  }
}

int launch_init(hipStream_t st, const RedArgs &p, int64_t lightest_v, int64_t batch) {
  int64_t grid = (batch + BATCH_WAVE_THREADS - 1) / BATCH_WAVE_THREADS;
  if (grid > 4096) grid = 4096;
  hipLaunchKernelGGL(red_init_kernel, dim3((unsigned)grid), dim3(BATCH_WAVE_THREADS), 0, st, p.total, p.lightest, lightest_v, p.first, p.first_none, p.end,
                     (int64_t)0, batch);
  HIPTRY(hipGetLastError());
  return 0;
}

int plan(int64_t nrows, int64_t ncols, int64_t w0, int64_t t1) {
  if (nrows < 0 || ncols < 0) return -1;
  const int64_t width = width_of(ncols);
  if (nrows == 0 || width == 0) return 0;
  if (nrows <= 64 && width <= w0) return 0;
  return nrows <= t1 / width ? 1 : 2;  // nrows * width <= t1, without the product
}

bool aligned16(const word *p, int64_t stride, int64_t bs) { return ((uintptr_t)p & 15) == 0 && !(stride & 1) && !(bs & 1); }

// The one call behind the three entry points.  need_b: B is an operand that must be there (the mismatch); the outputs not of the
// entry point are NULL in p.
int reduce_batch(RedArgs p, int64_t ncols, int64_t batch, bool need_b, hipStream_t st) {
  if (p.nrows < 0 || ncols < 0 || batch < 0 || p.a_stride < 0 || p.a_bs < 0 || p.b_stride < 0 || p.b_bs < 0) return (int)hipErrorInvalidValue;
  if (p.nrows > INT32_MAX || ncols > INT32_MAX) return (int)hipErrorInvalidValue;  // a row index, a row weight: 32 bits
  if (!p.total && !p.row_weight && !p.lightest && !p.first && !p.end) return (int)hipErrorInvalidValue;
  p.width         = width_of(ncols);
  p.mask          = tail_mask((int)(ncols & 63));
  const bool data = p.nrows > 0 && ncols > 0;
  const bool hasb = need_b || p.B;
  if (data && (p.a_stride < p.width || (hasb && p.b_stride < p.width))) return (int)hipErrorInvalidValue;
  if (batch > 0 && data && (!p.A || (need_b && !p.B))) return (int)hipErrorInvalidValue;
  const Span a = rows_span(p.A, batch, p.a_bs, p.nrows, p.a_stride, p.width), b = rows_span(p.B, batch, p.b_bs, p.nrows, p.b_stride, p.width);
  for (const Span &out : {entries_span(p.total, batch, 1, 1, 8), entries_span(p.row_weight, batch, p.nrows, p.nrows, 4), entries_span(p.lightest, batch, 1, 1, 8),
                          entries_span(p.first, batch, 1, 1, 4), entries_span(p.end, batch, 1, 1, 4)})  // each output against the operands, not each other
    if (spans_meet_any({out}, {a, b})) return (int)hipErrorInvalidValue;
  if (batch == 0) return 0;
  if (!data) {  // empty members: weights 0, no lightest row without rows, no non-zero row
    if (p.row_weight && p.nrows > 0) HIPTRY(hipMemsetAsync(p.row_weight, 0, (size_t)(batch * p.nrows) * 4, st));
    if (p.total || p.lightest || p.first || p.end) return launch_init(st, p, p.nrows == 0 ? -1 : 0, batch);
    return 0;
  }
  const int path = plan(p.nrows, ncols, env_bound("M4RI_AMD_REDUCE_BATCH_PATH0_MAX", RDB_W0, 0, RDB_W0_MAX),
                        env_bound("M4RI_AMD_REDUCE_BATCH_PATH1_MAX", RDB_T1, 0, RDB_T1_MAX));
  const bool vec = aligned16(p.A, p.a_stride, p.a_bs) && (!p.B || aligned16(p.B, p.b_stride, p.b_bs));
  if (path == 0) {
    return launch_waves(batch, [&](dim3 grid, int64_t b0, int64_t nb) {
      p.b0 = b0, p.batch = b0 + nb;
      if (vec) hipLaunchKernelGGL(red_wave_kernel<true>, grid, dim3(BATCH_WAVE_THREADS), 0, st, p);
      else hipLaunchKernelGGL(red_wave_kernel<false>, grid, dim3(BATCH_WAVE_THREADS), 0, st, p);
    });
  }
  const int64_t units = vec ? (p.width + 1) / 2 : p.width;  // what a row's lanes share
  p.lshift            = 0;
  while (p.lshift < 6 && ((int64_t)1 << p.lshift) < units) ++p.lshift;
  const int64_t step = (int64_t)RDB_WAVES * (64 >> p.lshift);  // the rows of one round of a workgroup
  if (path == 1) {
    p.chunk_rows = p.nrows, p.chunks = 1;
  } else {
    p.chunk_rows = (RDB_CHUNK_WORDS / p.width + step - 1) / step * step;
    if (p.chunk_rows < step) p.chunk_rows = step;
    p.chunks = (p.nrows + p.chunk_rows - 1) / p.chunk_rows;
    if (p.total || p.lightest || p.first || p.end) HIPTRY(launch_init(st, p, INT64_MAX, batch));
  }
  return launch_chunked(batch, BATCH_CHUNK / p.chunks > 0 ? BATCH_CHUNK / p.chunks : 1, [&](int64_t b0, int64_t nb) {
    p.b0 = b0, p.batch = b0 + nb;
    const dim3 grid((unsigned)(nb * p.chunks));
    if (path == 1) {
      if (vec) hipLaunchKernelGGL((red_block_kernel<true, false>), grid, dim3(BATCH_WAVE_THREADS), 0, st, p);
      else hipLaunchKernelGGL((red_block_kernel<false, false>), grid, dim3(BATCH_WAVE_THREADS), 0, st, p);
    } else {
      if (vec) hipLaunchKernelGGL((red_block_kernel<true, true>), grid, dim3(BATCH_WAVE_THREADS), 0, st, p);
      else hipLaunchKernelGGL((red_block_kernel<false, true>), grid, dim3(BATCH_WAVE_THREADS), 0, st, p);
    }
  });
}

}  // namespace

extern "C" {

int m4ri_amd_plan_reduce_batch(int64_t nrows, int64_t ncols) { return plan(nrows, ncols, RDB_W0, RDB_T1); }

int m4ri_amd_weight_batch_dev(const word *A, int64_t a_stride, int64_t a_bs, const word *B, int64_t b_stride, int64_t b_bs, int64_t nrows, int64_t ncols,
                              int64_t batch, int64_t *total, int32_t *row_weight, int64_t *lightest, void *stream) {
  RedArgs p{};
  p.A = A, p.a_stride = a_stride, p.a_bs = a_bs, p.B = B, p.b_stride = B ? b_stride : 0, p.b_bs = B ? b_bs : 0, p.nrows = nrows;
  p.total = total, p.row_weight = row_weight, p.lightest = lightest;
  if (!B && (b_stride < 0 || b_bs < 0)) return (int)hipErrorInvalidValue;
  return reduce_batch(p, ncols, batch, false, (hipStream_t)stream);
}

int m4ri_amd_mismatch_batch_dev(const word *A, int64_t a_stride, int64_t a_bs, const word *B, int64_t b_stride, int64_t b_bs, int64_t nrows, int64_t ncols,
                                int64_t batch, int32_t *first_row, void *stream) {
  RedArgs p{};
  p.A = A, p.a_stride = a_stride, p.a_bs = a_bs, p.B = B, p.b_stride = b_stride, p.b_bs = b_bs, p.nrows = nrows;
  p.first = first_row, p.first_none = -1;
  return reduce_batch(p, ncols, batch, true, (hipStream_t)stream);
}

int m4ri_amd_row_span_batch_dev(const word *A, int64_t a_stride, int64_t a_bs, int64_t nrows, int64_t ncols, int64_t batch, int32_t *first_nonzero,
                                int32_t *end_nonzero, void *stream) {
  RedArgs p{};
  p.A = A, p.a_stride = a_stride, p.a_bs = a_bs, p.nrows = nrows;
  p.first = first_nonzero, p.end = end_nonzero, p.first_none = nrows >= 0 && nrows <= INT32_MAX ? (int32_t)nrows : 0;
  return reduce_batch(p, ncols, batch, false, (hipStream_t)stream);
}

}  // extern "C"
