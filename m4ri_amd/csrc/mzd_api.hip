// mzd_api.hip -- the drop-in boundary (include/m4ri_amd.h, parts 1 and 3): M4RI's own entry points, taking and returning host
// mzd_t matrices, implemented on the device engine.  Same names, argument meaning and fatal-error behaviour as the reference
// (each entry point names its place there).  There is NO CPU fallback: a HIP failure is fatal, like every other error on this
// path (misc.c:36-42).
//
// In this order:
//   allocator         m4ri_amd_mzd_init / _free, the cache of large blocks, results allocated beside the upload (LateC)
//   staging           one grow-only device arena per device, re-carved on every call; upload / download; the pinned host buffer
//   residency         the table of pinned matrices (its entry points, m4ri_amd_pin and friends, are at the end of the file)
//   HostCall          one host entry point running on the current device, and the placement of its operands
//   products          mzd_mul, mzd_addmul, _mzd_mul_even ... _mzd_addsqr_even, mzd_mul_m4rm ..., mzd_mul_mp: run(), and run_pipelined(),
//                     which executes the block plan of host_pipeline_plan.cpp (grid, cuts and arena words are decided there)
//   solver family     TRSM, PLE / PLUQ, echelon forms, permutations, systems, kernels, inverses, transposes, triangular inverses
//   table primitives  mzd_make_table, mzd_process_rows{,2..6}
//
// THE PLACEMENT RULE (place() is its only statement).  A matrix that is not pinned is STAGED: uploaded straight out of the
// caller's rows (hipMemcpy2D, so windows cost nothing extra) with the bits beyond its last column cleared on the device, and
// downloaded touching only the words and bits the reference would touch (mzd.h:117-123).  A pinned matrix, or a window of one, IS
// its device copy and is used IN PLACE -- unless it is a window that shares its last word with neighbouring columns of the parent
// (ncols off the word grid and narrower than the parent) AND the call writes it or needs the bits beyond its last column clean:
// then it is staged as a masked device-to-device copy, and what was written goes back under the column mask.  Whatever a call
// writes in a pinned parent leaves the host copy stale until m4ri_amd_sync / m4ri_amd_unpin.
//
// THE LOCKING RULE.  One lock per DEVICE (g_dev_mu) for everything that works on that device's arena, solver scratch and engine:
// a HostCall holds the lock of the current device from its construction on, so threads that drive different GPUs run side by side
// and threads on one GPU take turns.  g_pin_mu guards the LIST of pins only; an ENTRY is guarded by the lock of the device it lives
// on (PinLock), whatever device the calling thread has current.  g_stats_mu guards the statistics.
#include <hip/hip_runtime.h>
#include <dlfcn.h>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <ctime>
#include <sys/mman.h>
#include <sys/sysinfo.h>
#include <algorithm>
#include <atomic>
#include <condition_variable>
#include <list>
#include <mutex>
#include <thread>
#include <vector>
#include "gf2_internal.h"
#include "../../include/m4ri_amd.h"

namespace {

constexpr uint8_t FLAG_EXCESS = 0x2;  // mzd.h:144
constexpr uint8_t FLAG_WINDOW = 0x4;  // mzd.h:150

// The locks of the host entry points (the locking rule above)
std::mutex g_dev_mu[GF2_MAX_DEVICES];
std::mutex g_pin_mu, g_stats_mu;
std::unique_lock<std::mutex> lock_device(int dev) {  // a device HIP could not name or this table does not hold: slot 0
  return std::unique_lock<std::mutex>(g_dev_mu[dev >= 0 && dev < GF2_MAX_DEVICES ? dev : 0]);
}
std::unique_lock<std::mutex> lock_current_device() {
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) dev = 0;
  return lock_device(dev);
}

// M4RI_AMD_STATS=1: at exit, print how many products went through the host entry points, the time
// spent in them (transfers included) and the bytes moved over PCIe -- for judging what an LD_PRELOAD
// run of a larger program (PLE, TRSM) spends where
struct ApiStats {
  double seconds = 0, h2d = 0, d2h = 0;
  long calls = 0;
  int populate_fallback = 0;  // a fresh result's pages were faulted by touching them: no MADV_POPULATE_WRITE here
  ~ApiStats() {
    if (calls && getenv("M4RI_AMD_STATS"))
      fprintf(stderr, "m4ri_amd: %ld products through the host entry points, %.3f s inside them, %.2f GiB up, %.2f GiB down\n",
              calls, seconds, h2d / 1073741824.0, d2h / 1073741824.0);
    if (populate_fallback && getenv("M4RI_AMD_STATS")) fprintf(stderr, "m4ri_amd: MADV_POPULATE_WRITE unavailable, fresh results were pre-faulted by touching their pages\n");
  }
} g_api_stats;

[[noreturn]] void die(const char *fmt, ...) {  // misc.c:36-42
  va_list ap;
  va_start(ap, fmt);
  vfprintf(stderr, fmt, ap);
  va_end(ap);
  abort();
}

#define HIPDIE(expr)                                                                            \
  do {                                                                                          \
    hipError_t e_ = (hipError_t)(expr);                                                         \
    if (e_ != hipSuccess) die("m4ri_amd: HIP failure '%s' in %s (%s:%d)\n", hipGetErrorString(e_), #expr, __FILE__, __LINE__); \
  } while (0)

typedef mzd_t *(*mzd_init_fn)(rci_t, rci_t);
mzd_init_fn host_mzd_init() {
  // the caller will mzd_free() the result, so it has to come from the host program's libm4ri
  // allocator when there is one
  static mzd_init_fn fn = reinterpret_cast<mzd_init_fn>(dlsym(RTLD_DEFAULT, "mzd_init"));
  return fn;
}

mzd_t *result_init(rci_t r, rci_t c) {
  mzd_init_fn host_init = host_mzd_init();
  return host_init ? host_init(r, c) : m4ri_amd_mzd_init(r, c);
}

// Blocks of this size and more come straight from mmap in m4ri_amd_mzd_init: whole zero pages from the kernel, nothing to clear
constexpr size_t BIG_BLOCK = (size_t)8 << 20;
size_t big_len(size_t bytes) { return (bytes + 4095) & ~(size_t)4095; }

// The allocator's cache of large blocks (the counterpart of the reference's m4ri_mmc cache, mmc.c:44-116, which keeps the blocks
// BELOW the L3 size; this one keeps the few huge ones): m4ri_amd_mzd_free parks up to two mappings, at most 4 GiB together, and the
// next allocation of exactly that size takes one back -- its pages are already faulted in, which is the whole cost of a fresh
// 512 MiB result (33 ... 87 ms).  m4ri_amd_release_workspace() returns them to the system.
struct BigCache {
  std::mutex mu;
  struct Slot { void *p = nullptr; size_t len = 0; } slot[2];
  void *take(size_t len) {
    std::lock_guard<std::mutex> lk(mu);
    for (Slot &s : slot)
      if (s.p && s.len == len) { void *p = s.p; s = Slot{}; return p; }
    return nullptr;
  }
  bool park(void *p, size_t len) {
    static const bool enabled = !(getenv("M4RI_AMD_RESULT_CACHE") && atoi(getenv("M4RI_AMD_RESULT_CACHE")) == 0);
    std::lock_guard<std::mutex> lk(mu);
    size_t held = 0;
    for (Slot &s : slot) held += s.len;
    if (!enabled || held + len > ((size_t)4 << 30)) return false;
    for (Slot &s : slot)
      if (!s.p) { s.p = p; s.len = len; return true; }
    return false;
  }
  void drop() {
    std::lock_guard<std::mutex> lk(mu);
    for (Slot &s : slot) {
      if (s.p) munmap(s.p, s.len);
      s = Slot{};
    }
  }
} g_big_cache;

void *big_map(size_t len) {  // a fresh 2 MiB-aligned mapping: zero pages on demand
  const size_t al = (size_t)2 << 20;
  char *raw = static_cast<char *>(mmap(nullptr, len + al, PROT_READ | PROT_WRITE, MAP_PRIVATE | MAP_ANONYMOUS, -1, 0));
  if (raw == MAP_FAILED) return nullptr;
  char *q = reinterpret_cast<char *>((reinterpret_cast<uintptr_t>(raw) + al - 1) & ~(uintptr_t)(al - 1));
  if (q > raw) munmap(raw, (size_t)(q - raw));
  if (raw + len + al > q + len) munmap(q + len, (size_t)((raw + len + al) - (q + len)));
  return q;
}

void zero_with_threads(char *p, size_t bytes) {
  const unsigned hw = std::thread::hardware_concurrency();
  const size_t nt = hw >= 256 ? 32 : hw >= 64 ? 16 : 8, per = ((bytes / nt) + 4095) & ~(size_t)4095;
  std::vector<std::thread> th;
  size_t at = 0;
  try {
    for (; at < bytes; at += per) {
      const size_t len = bytes - at < per ? bytes - at : per;
      th.emplace_back([=] { memset(p + at, 0, len); });
    }
  } catch (...) {  // no more threads to be had: the rest here
    if (at < bytes) memset(p + at, 0, bytes - at);
  }
  for (std::thread &t : th) t.join();
}

mzd_t *descriptor(rci_t r, rci_t c) {  // mzd.c:142-150
  mzd_t *A = static_cast<mzd_t *>(calloc(1, sizeof(mzd_t)));
  if (!A) return nullptr;
  A->nrows        = r;
  A->ncols        = c;
  A->width        = c > 0 ? (c - 1) / 64 + 1 : 0;
  A->rowstride    = (A->width & 1) ? A->width + 1 : A->width;
  A->high_bitmask = (~(word)0) >> ((64 - c % 64) % 64);
  A->flags        = (A->high_bitmask != ~(word)0) ? 0x2 : 0;  // mzd.h:144: non-zero excess
  return A;
}

// A result that is still on its way.  mzd_mul(NULL, A, B, cutoff) is the region the reference's own bench times
// (bench/bench_multiplication.c:85-107), and a fresh 512 MiB matrix costs 33 ... 87 ms of page faults and clearing -- more than
// the 65536^3 product it receives -- when that happens in front of the upload.  Nothing needs C before the first block of the
// result is downloaded, so:
//   * with the host program's allocator (its mzd_init: malloc + ONE memset, misc.h:614-634) the call runs on a thread of its own
//     beside the upload and the first products; the first download waits for it (get());
//   * with this library's allocator the block is mmap'ed (instant, zero pages on demand) and worker threads fault its pages in
//     (MADV_POPULATE_WRITE: never changes a byte, so it may run beside the downloads) while the GPU works.
struct LateC {
  rci_t nrows = 0, ncols = 0;
  mzd_t *C = nullptr;
  std::thread maker;
  std::vector<std::thread> populate;
  std::once_flag once;
  mzd_t *get() {
    std::call_once(once, [this] { if (maker.joinable()) maker.join(); });
    return C;
  }
  mzd_t *finish() {
    get();
    for (std::thread &t : populate) t.join();
    populate.clear();
    return C;
  }
};

#ifndef MADV_POPULATE_WRITE
#define MADV_POPULATE_WRITE 23  // Linux 5.14
#endif

void late_begin(LateC &lc, rci_t r, rci_t c) {
  lc.nrows = r; lc.ncols = c;
  if (mzd_init_fn host_init = host_mzd_init()) {
    try {
      lc.maker = std::thread([&lc, host_init, r, c] { lc.C = host_init(r, c); });
    } catch (...) {  // no thread to be had (RLIMIT_NPROC, a pids cgroup): allocate here and now
      lc.C = host_init(r, c);
    }
    return;
  }
  // this library's allocator.  The product overwrites every valid word of the result, so a parked block of the same size is taken
  // as it is (its padding words cleared when rows have one); a block the cache does not have is a fresh mapping
  mzd_t *C = descriptor(r, c);
  if (!C) die("m4ri_amd: out of memory\n");
  lc.C = C;
  const size_t bytes = (size_t)r * (size_t)C->rowstride * 8, len = big_len(bytes);
  if (void *p = g_big_cache.take(len)) {
    C->data = static_cast<word *>(p);
    // M4RI_AMD_POISON_RESULT=1 (tests/test_gpu_host_pipeline.py): the parked block is filled with a pattern first, so that a run path
    // that failed to write some valid word of the result would show -- the check behind "taken as it is" 
    static const bool poison = getenv("M4RI_AMD_POISON_RESULT") && atoi(getenv("M4RI_AMD_POISON_RESULT")) != 0;
    if (poison) {
      std::memset(p, 0xA5, bytes);
      if (C->rowstride != C->width)
        for (rci_t i = 0; i < r; ++i) C->data[(int64_t)i * C->rowstride + C->width] = 0;
    } else if (C->rowstride != C->width) zero_with_threads(static_cast<char *>(p), bytes);
    return;
  }
  char *base = static_cast<char *>(big_map(len));
  if (!base) die("m4ri_amd: out of memory\n");
  C->data = reinterpret_cast<word *>(base);
  // How the pages of a NEW block come into being (M4RI_AMD_FRESH, a developer switch; measured in profiles/r04_fresh_result/):
  //   populate   worker threads fault them in beside the upload and the products (MADV_POPULATE_WRITE never changes a byte, so it
  //              may run beside the downloads; where the kernel lacks it, an atomic OR of zero per page)
  //   huge       the same after MADV_HUGEPAGE;  lazy: nothing, the downloads fault them;  zero: cleared by threads here and now
  //   auto (default): huge when memory is plentiful, else populate
  // Measured on the GPU box, 65536^3, every result a new block (profiles/r04_fresh_result.log; C given: 42.6 ms): huge 58 ... 61 ms,
  // populate 75 ... 86, lazy 73 ... 78, zero 68 ... 82 -- and 43.8 ms when the cache above has the block.  Huge pages are asked for only
  // when memory is plentiful (8 x the block available): on a host short of memory MADV_HUGEPAGE makes every fault compact memory
  // synchronously (a first 512 MiB block took 0.7 ... 1.7 s in the 8 GiB build container).
  static const char *mode_env = getenv("M4RI_AMD_FRESH");
  char mode = mode_env ? mode_env[0] : 'a';
  if (mode == 'a') {
    struct sysinfo si;
    mode = (sysinfo(&si) == 0 && (double)si.freeram * (double)si.mem_unit >= 8.0 * (double)bytes) ? 'h' : 'p';
  }
  if (mode == 'l') return;
  if (mode == 'z') { zero_with_threads(base, bytes); return; }
  if (mode == 'h') (void)madvise(base, len, 14 /* MADV_HUGEPAGE */);
  const unsigned hw = std::thread::hardware_concurrency();
  const size_t nt = hw >= 64 ? 16 : hw >= 16 ? 8 : 2, chunk = (size_t)16 << 20;
  // the workers walk the block front to back in 16 MiB chunks, round robin: the rows the first download will write come first
  try {
    for (size_t k = 0; k < nt; ++k)
      lc.populate.emplace_back([base, bytes, k, nt, chunk] {
        bool advise = true;
        for (size_t at = k * chunk; at < bytes; at += nt * chunk) {
          const size_t n = bytes - at < chunk ? bytes - at : chunk;
          if (advise && madvise(base + at, big_len(n), MADV_POPULATE_WRITE) == 0) continue;
          advise = false;
          g_api_stats.populate_fallback = 1;
          for (size_t off = 0; off < n; off += 4096) __atomic_fetch_or(reinterpret_cast<unsigned char *>(base + at + off), (unsigned char)0, __ATOMIC_RELAXED);
        }
      });
  } catch (...) {  // fewer (or no) helpers: the downloads fault what is left
  }
}

// ---- staging arena ------------------------------------------------------------------------------
// Device copies of host operands live in ONE grow-only buffer that is re-carved on every call: no
// hipMalloc/hipFree per product (they cost more than a small product itself).
struct Arena {
  word *base  = nullptr;
  size_t cap  = 0;  // words
  size_t used = 0;
};
Arena g_arenas[GF2_MAX_DEVICES];  // one per HIP device: run() works on whatever device is current
thread_local int g_arena_dev = 0;  // the device whose arena this thread is carving (set by arena_reserve, under that device's lock)
#define g_arena g_arenas[g_arena_dev]

void arena_reserve(size_t words) {
  int dev = 0;
  HIPDIE(hipGetDevice(&dev));
  if (dev < 0 || dev >= GF2_MAX_DEVICES) die("m4ri_amd: HIP device %d out of range\n", dev);
  g_arena_dev = dev;
  g_arena.used = 0;
  if (words <= g_arena.cap) return;
  HIPDIE(hipDeviceSynchronize());
  if (g_arena.base) HIPDIE(hipFree(g_arena.base));
  g_arena.base = nullptr; g_arena.cap = 0;
  HIPDIE(hipMalloc(reinterpret_cast<void **>(&g_arena.base), words * 8));
  g_arena.cap = words;
}

struct DevMat {
  word *p        = nullptr;
  int64_t stride = 0;
};

void dev_alloc(DevMat &d, int64_t rows, int64_t ncols) {
  const int64_t w = words_of(ncols);
  d.stride        = (w + 1) & ~(int64_t)1;  // even: rows stay 16-byte aligned
  d.p             = g_arena.base + g_arena.used;
  g_arena.used += dev_words(rows, ncols);
  if (g_arena.used > g_arena.cap) die("m4ri_amd: staging arena overrun (internal error)\n");
}

// host rows -> device matrix with zero excess
void upload(DevMat &d, const mzd_t *M) {
  dev_alloc(d, M->nrows, M->ncols);
  if (M->nrows == 0 || M->width == 0) return;
  if (d.stride != M->width)  // padding word must not stay uninitialised (it is never read as data,
    HIPDIE(hipMemsetAsync(d.p, 0, (size_t)M->nrows * d.stride * 8, 0));  // but keep it deterministic)
  HIPDIE(hipMemcpy2D(d.p, (size_t)d.stride * 8, M->data, (size_t)M->rowstride * 8, (size_t)M->width * 8,
                     (size_t)M->nrows, hipMemcpyHostToDevice));
  { std::lock_guard<std::mutex> sl(g_stats_mu); g_api_stats.h2d += (double)M->width * 8.0 * (double)M->nrows; }
  HIPDIE(m4ri_amd_mask_tail_dev(d.p, d.stride, M->nrows, M->ncols, nullptr));
}

// device result -> host C, writing words [0, width) only and, in the last word, only the bits
// inside high_bitmask when C is a window with excess
void download(const DevMat &d, mzd_t *C) {
  if (C->nrows == 0 || C->width == 0) return;
  { std::lock_guard<std::mutex> sl(g_stats_mu); g_api_stats.d2h += (double)C->width * 8.0 * (double)C->nrows; }
  const bool dangerous = (C->flags & FLAG_WINDOW) && (C->ncols % 64 != 0);
  if (!dangerous) {
    HIPDIE(hipMemcpy2D(C->data, (size_t)C->rowstride * 8, d.p, (size_t)d.stride * 8, (size_t)C->width * 8,
                       (size_t)C->nrows, hipMemcpyDeviceToHost));
    return;
  }
  if (C->width > 1)
    HIPDIE(hipMemcpy2D(C->data, (size_t)C->rowstride * 8, d.p, (size_t)d.stride * 8, (size_t)(C->width - 1) * 8,
                       (size_t)C->nrows, hipMemcpyDeviceToHost));
  std::vector<word> last((size_t)C->nrows);
  HIPDIE(hipMemcpy2D(last.data(), 8, d.p + (C->width - 1), (size_t)d.stride * 8, 8, (size_t)C->nrows, hipMemcpyDeviceToHost));
  const word mask = C->high_bitmask;
  for (rci_t i = 0; i < C->nrows; ++i) {
    word *w = C->data + (int64_t)i * C->rowstride + (C->width - 1);
    *w      = (*w & ~mask) | (last[(size_t)i] & mask);
  }
}

// ---- one transfer each way for products of a few MiB ----------------------------------------------------
// A product from host memory used to cost two blocking 2-D uploads (each with its own clear and tail-mask launch), the
// kernels, a blocking 2-D download and a device synchronisation: 85 ... 130 us whatever the size.  Operands of a few MiB
// are instead packed by the CPU into ONE pinned buffer per device (rows at the device stride, padding words cleared, the bits
// beyond the last column masked on the way -- a window's neighbours never reach the device), sent with one asynchronous copy,
// and the result comes back the same way and is merged into C's rows under the column mask by the CPU.
struct HostStage {
  word *p    = nullptr;
  size_t cap = 0;  // words
};
HostStage g_host_stage[GF2_MAX_DEVICES];
constexpr size_t SMALL_STAGE_BYTES = (size_t)2 << 20;  // A + B + C above this: the 2-D copies straight from / to the caller's rows (4096^3 = 6 MiB: 0.32 ms packed against 0.25 ms direct)

word *host_stage(int dev, size_t words) {
  HostStage &h = g_host_stage[dev];
  if (words > h.cap) {
    if (h.p) { HIPDIE(hipDeviceSynchronize()); HIPDIE(hipHostFree(h.p)); }
    h.p = nullptr; h.cap = 0;
    HIPDIE(hipHostMalloc(reinterpret_cast<void **>(&h.p), words * 8, hipHostMallocDefault));
    h.cap = words;
  }
  return h.p;
}

// rows of M -> `dst` at `stride` words per row: valid words copied, the last one masked, padding words cleared
void pack_rows(word *dst, int64_t stride, const mzd_t *M) {
  const int64_t w = M->width;
  for (rci_t i = 0; i < M->nrows; ++i) {
    word *d       = dst + (int64_t)i * stride;
    const word *r = M->data + (int64_t)i * M->rowstride;
    if (w > 0) {
      memcpy(d, r, (size_t)w * 8);
      d[w - 1] &= M->high_bitmask;
    }
    for (int64_t k = w; k < stride; ++k) d[k] = 0;
  }
}

// `src` (rows at `stride`) -> C's rows: whole words, the last one under the column mask when C is a window
void unpack_rows(mzd_t *C, const word *src, int64_t stride) {
  const int64_t w = C->width;
  if (w == 0) return;
  const bool window = (C->flags & FLAG_WINDOW) != 0;
  const word mask   = C->high_bitmask;
  for (rci_t i = 0; i < C->nrows; ++i) {
    word *c       = C->data + (int64_t)i * C->rowstride;
    const word *r = src + (int64_t)i * stride;
    if (w > 1) memcpy(c, r, (size_t)(w - 1) * 8);
    c[w - 1] = window ? ((c[w - 1] & ~mask) | (r[w - 1] & mask)) : (r[w - 1] & mask);
  }
}

// ---- residency table (include/m4ri_amd.h part 3) ------------------------------------
// A pinned matrix keeps a device copy with the host layout (same rowstride), so any window into it
// is the same offset into the device copy.  Products read pinned operands where they are and leave a
// pinned result on the device (the host copy is stale until m4ri_amd_sync / m4ri_amd_unpin).
struct Pin {
  const word *hbase;  // host block
  size_t words;       // nrows * rowstride
  int64_t rowstride;
  rci_t nrows, ncols;
  word *dbase;
  bool dev_newer;  // written under the pin's device lock (set_newer), read there or by the cheap status query (is_newer): atomic accesses
  mzd_t *owner;
  int device;  // HIP device the copy lives on
};
inline void set_newer(Pin &p, bool v) { __atomic_store_n(&p.dev_newer, v, __ATOMIC_RELEASE); }
inline bool is_newer(const Pin &p) { return __atomic_load_n(&p.dev_newer, __ATOMIC_ACQUIRE); }
std::list<Pin> g_pins;  // a list: entries stay where they are while other threads pin and unpin (g_pin_mu guards the walk and the edits)

// Locking rule of the table: g_pin_mu guards the walk and the edits of the LIST; the lock of the device a pin lives on
// (g_dev_mu[pin.device]) guards the ENTRY -- its device copy, its dev_newer flag, its removal.  A product holds that lock for its
// whole duration (it runs on the pin's device or dies, HostCall::view()), so whoever changes or removes a pin takes the PIN'S device
// lock, not the lock of whatever device its own thread happens to have current (PinLock).  A Pin* from find_pin is therefore valid
// for as long as the caller holds the lock of the device the pin is on.
bool covers(const Pin &p, const mzd_t *M) {  // M is the pinned matrix or a window into it: inside its block, with its layout
  return M->data >= p.hbase && M->data < p.hbase + p.words && M->rowstride == p.rowstride;
}

Pin *pin_of(const mzd_t *M) {  // with g_pin_mu held
  if (!M || !M->data) return nullptr;
  for (Pin &p : g_pins)
    if (covers(p, M)) return &p;
  return nullptr;
}

Pin *find_pin(const mzd_t *M) {
  std::lock_guard<std::mutex> pl(g_pin_mu);
  return pin_of(M);
}

int pin_device(const mzd_t *M) {  // the device M's pinned parent lives on, -1 when there is none (read under the list's lock)
  std::lock_guard<std::mutex> pl(g_pin_mu);
  const Pin *p = pin_of(M);
  return p ? p->device : -1;
}

void erase_pin(const Pin *p) {  // with the lock of the pin's device held
  std::lock_guard<std::mutex> pl(g_pin_mu);
  for (auto it = g_pins.begin(); it != g_pins.end(); ++it)
    if (&*it == p) { g_pins.erase(it); break; }
}

// the pin of M with the lock of ITS device held and that device current (restored on the way out); p == nullptr: not pinned
struct PinLock {
  std::unique_lock<std::mutex> lk;
  Pin *p   = nullptr;
  int prev = -1, dev = -1;  // the caller's current device, the pin's (kept here: unpin erases *p before this object goes)
  explicit PinLock(const mzd_t *M) {
    for (;;) {  // until the look and the lock agree: giving up would report a pinned matrix as "not pinned" (a stale host copy unnoticed)
      const int d = pin_device(M);
      if (d < 0 || d >= GF2_MAX_DEVICES) return;
      lk = std::unique_lock<std::mutex>(g_dev_mu[d]);
      Pin *q = find_pin(M);
      if (q && q->device == d) {
        p   = q;
        dev = d;
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        if (prev != d) HIPDIE(hipSetDevice(d));
        return;
      }
      lk.unlock();  // unpinned, or re-pinned elsewhere, between the look and the lock: look again
    }
  }
  ~PinLock() {
    if (p && prev >= 0 && prev != dev) (void)hipSetDevice(prev);
  }
};

// ---- one host call and the placement of its operands ------------------------------------------------------------------
// What an entry point declares of each matrix (or plain buffer) it works on: decided once, by place(), and used for all three of
// how many words of the arena it takes, how it is bound when the call is staged, and what happens to it when the call finishes.
struct Operand {
  enum Bind { VIEW, UPLOAD, SPACE, COPY_IN, WORDS };  // in the pinned parent | host rows sent up | room only | masked copy out of the parent | plain words
  enum Finish { NOTHING, NEWER, COPY_BACK, DOWNLOAD };  // | parent written in place | masked copy into the parent (then NEWER) | rows sent down
  DevMat d;  // valid after HostCall::stage()
  const mzd_t *M = nullptr;
  Pin *pin       = nullptr;
  Bind bind      = SPACE;
  Finish finish  = NOTHING;
  int64_t rows = 0, ncols = 0;  // of the staged copy
  size_t words = 0;             // of the arena: 0 in place
  const void *src  = nullptr;   // WORDS: host data sent along
  size_t src_bytes = 0;
  bool staged() const { return bind != VIEW; }
};

// THE placement rule (the head of the file).  clean_tail: the call needs the bits beyond the last column zero in a matrix it only
// reads; always_staged: the result is built apart from the matrix it goes to whatever that is (mzd_transpose, where DST may be A)
Operand place(const mzd_t *M, bool read, bool write, bool clean_tail, bool always_staged) {
  Operand o;
  o.M = M; o.rows = M->nrows; o.ncols = M->ncols;
  o.pin = find_pin(M);
  const bool shares_last_word = o.pin && M->ncols % 64 != 0 && M->ncols != o.pin->ncols;
  const bool staged = !o.pin || always_staged || (shares_last_word && (write || clean_tail));
  o.bind   = !staged ? Operand::VIEW : !read ? Operand::SPACE : o.pin ? Operand::COPY_IN : Operand::UPLOAD;
  o.finish = !write ? Operand::NOTHING : !o.pin ? Operand::DOWNLOAD : staged ? Operand::COPY_BACK : Operand::NEWER;
  o.words  = staged ? dev_words(o.rows, o.ncols) : 0;
  return o;
}

// A host entry point running on the current device: the device's lock taken and the device initialised on construction; operands
// declared (in / inout / out / space / words), then stage() -- ONE reserve of what the declarations add up to, and the bindings in
// the order declared -- then the device work on each operand's `d`, then finish(): the write-backs in the order declared, the
// device synchronised, the call counted.  A body that returns before finish() has touched nothing.
struct HostCall {
  enum Kind { COUNTED, UNCOUNTED, PRODUCT };  // PRODUCT: the statistics' seconds run from the lock to the end of the call, which is counted there
  std::unique_lock<std::mutex> lk;
  int dev = 0;
  const Kind kind;
  timespec t0;
  Operand ops[16];  // mzd_process_rows6: M, six tables with their index lists, the row indices
  int nops = 0;

  explicit HostCall(Kind k = COUNTED) : kind(k) {
    const hipError_t no_device = hipGetDevice(&dev);
    lk = lock_device(no_device ? 0 : dev);
    if (kind == PRODUCT) clock_gettime(CLOCK_MONOTONIC, &t0);
    if (no_device) die("m4ri_amd: HIP failure '%s' in hipGetDevice\n", hipGetErrorString(no_device));
    HIPDIE(m4ri_amd_init(dev));
  }
  ~HostCall() {
    if (kind != PRODUCT) return;
    timespec t1;
    clock_gettime(CLOCK_MONOTONIC, &t1);
    std::lock_guard<std::mutex> sl(g_stats_mu);
    g_api_stats.seconds += (double)(t1.tv_sec - t0.tv_sec) + 1e-9 * (double)(t1.tv_nsec - t0.tv_nsec);
    g_api_stats.calls += 1;
  }

  Operand &declare(const Operand &o) {
    if (nops == (int)(sizeof(ops) / sizeof(ops[0]))) die("m4ri_amd: too many operands in one call (internal error)\n");
    return ops[nops++] = o;
  }
  Operand &in(const mzd_t *M, bool clean_tail = false) { return declare(place(M, true, false, clean_tail, false)); }
  Operand &inout(mzd_t *M) { return declare(place(M, true, true, false, false)); }
  Operand &out(mzd_t *M, bool always_staged = false) { return declare(place(M, false, true, false, always_staged)); }
  Operand &space(int64_t rows, int64_t ncols) {  // a matrix of the call's own
    Operand o;
    o.rows = rows; o.ncols = ncols; o.words = dev_words(rows, ncols);
    return declare(o);
  }
  static void download_to(Operand &o, mzd_t *R) {  // ... which finish() is to send down to a fresh host matrix, known only now
    o.M = R; o.finish = Operand::DOWNLOAD;
  }
  Operand &words(size_t n, const void *src = nullptr, size_t src_bytes = 0) {  // plain words (256-byte granules), host data sent along
    Operand o;
    o.bind = Operand::WORDS; o.words = (n + 31) & ~(size_t)31; o.src = src; o.src_bytes = src_bytes;
    return declare(o);
  }

  // M inside its pinned parent: the same offset into the device copy
  DevMat view(const Pin &p, const mzd_t *M) const {
    if (p.device != dev) die("m4ri_amd: matrix pinned on device %d used while device %d is current\n", p.device, dev);
    return DevMat{p.dbase + (M->data - p.hbase), p.rowstride};
  }

  void stage() {
    size_t need = 0;
    for (int i = 0; i < nops; ++i) need += ops[i].words;
    arena_reserve(need);
    for (int i = 0; i < nops; ++i) {
      Operand &o = ops[i];
      switch (o.bind) {
        case Operand::VIEW: o.d = view(*o.pin, o.M); break;
        case Operand::UPLOAD: upload(o.d, o.M); break;
        case Operand::SPACE: dev_alloc(o.d, o.rows, o.ncols); break;
        case Operand::COPY_IN: {
          dev_alloc(o.d, o.rows, o.ncols);
          const DevMat src = view(*o.pin, o.M);
          HIPDIE(hipMemcpy2DAsync(o.d.p, (size_t)o.d.stride * 8, src.p, (size_t)src.stride * 8, (size_t)o.M->width * 8, (size_t)o.M->nrows,
                                  hipMemcpyDeviceToDevice, nullptr));
          HIPDIE(m4ri_amd_mask_tail_dev(o.d.p, o.d.stride, o.M->nrows, o.M->ncols, nullptr));
          break;
        }
        case Operand::WORDS:
          o.d.p = g_arena.base + g_arena.used;
          g_arena.used += o.words;
          if (g_arena.used > g_arena.cap) die("m4ri_amd: staging arena overrun (internal error)\n");
          if (o.src) HIPDIE(hipMemcpyAsync(o.d.p, o.src, o.src_bytes, hipMemcpyHostToDevice, nullptr));
          break;
      }
    }
  }

  void finish() {
    for (int i = 0; i < nops; ++i) {
      Operand &o = ops[i];
      if (o.finish == Operand::COPY_BACK) {
        const DevMat dst = view(*o.pin, o.M);
        HIPDIE(gf2_launch_copy_masked(nullptr, dst.p, dst.stride, o.d.p, o.d.stride, o.M->nrows, o.M->ncols));
      }
      if (o.finish == Operand::COPY_BACK || o.finish == Operand::NEWER) set_newer(*o.pin, true);  // the host copy is stale until m4ri_amd_sync / m4ri_amd_unpin
      if (o.finish == Operand::DOWNLOAD) download(o.d, const_cast<mzd_t *>(o.M));
    }
    HIPDIE(hipDeviceSynchronize());
    if (kind == COUNTED) { std::lock_guard<std::mutex> sl(g_stats_mu); g_api_stats.calls += 1; }
  }
};

int norm_cutoff(int cutoff, const char *who) {  // strassen.c:348-354
  if (cutoff < 0) die("%s: cutoff must be >= 0.\n", who);
  return cutoff;  // 0 = engine default; >0 normalised inside m4ri_amd_mul_dev
}

// m * l * n at or below which a product from host memory is computed on the host (m4ri_amd_set_small_product_threshold; the measured
// crossover against the GPU path on the GPU box, with the small leaf in the engine: 512^3 31 us on the host, 40 through the GPU;
// 576^3 49 against 47 -- profiles/r06_small_products_host_routine.log).  M4RI_AMD_SMALL_THRESHOLD overrides the default.
std::atomic<int64_t> g_small_threshold{getenv("M4RI_AMD_SMALL_THRESHOLD") ? atoll(getenv("M4RI_AMD_SMALL_THRESHOLD")) : ((int64_t)1 << 27)};
std::atomic<int64_t> g_small_count{0};  // products that took the host path

// Does a product of these dimensions go to the host routine?  m * l * n at most the threshold AND the routine's own cost
// (gf2_small_host_cost of small_host.cpp: word operations of ITS algorithm) at most threshold / 240 -- 2^27 / 240 = 559240, 39 us at the
// 0.07 ns per word operation it runs at: below the 25 ... 60 us a call through the GPU costs whatever its size.  The second bound is
// what keeps degenerate shapes -- 1 x 1 x 2^26, 2^26 x 1 x 1 -- away from a single-threaded loop.
bool small_product_wanted(int64_t m, int64_t l, int64_t n, int64_t threshold) {
  if (threshold <= 0 || m <= 0 || n <= 0) return false;
  if ((double)m * (double)l * (double)n > (double)threshold) return false;
  return gf2_small_host_cost(m, l, n) <= (double)threshold / 240.0;
}

// C (+)= A * B on the device: the Strassen-Winograd engine, or a single leaf
void product_dev(bool strassen, const DevMat &c, const DevMat &a, const DevMat &b, int64_t m, int64_t l, int64_t n, bool add, int cutoff, hipStream_t st) {
  if (strassen) HIPDIE(m4ri_amd_mul_dev(c.p, c.stride, a.p, a.stride, b.p, b.stride, m, l, n, add ? 1 : 0, cutoff, st));
  else HIPDIE(m4ri_amd_m4rm_dev(c.p, c.stride, a.p, a.stride, b.p, b.stride, m, l, n, add ? 1 : 0, 0, st));
}

// ---- large products from host memory, pipelined over blocks -------------------------------------------------------------------------
// C_ij (+)= A_ik * B_kj  on the gi x gj x gk grid of gf2_plan_host_pipeline (host_pipeline_plan.cpp: 2 x 2 x 1 when both m and n allow it,
// 2 x 2 x 2 from 65536^3 on, four row slabs of A and C for narrow products).  The uploads are blocking calls of this thread, the
// downloads of a second one (PCIe is full duplex), the products run on a non-blocking stream:
//   upload A_00, B_00 | P || upload A_01, B_10 | P -> C_00 complete: download || upload B_01 | P || ...
// so of the 1.5 GiB over PCIe at 65536^3 only the first pair of blocks (256 MiB) and the last block of C (128 MiB) stay exposed.  Same
// bits as the one-shot schedule (every step is an ordinary product or addmul).
std::atomic<size_t> g_pipeline_min_bytes{(size_t)64 << 20};  // A + B + C bytes from which blocks are used (16384^3: 2.62 -> 2.42 ms, 24576^3: 6.3 -> 5.3 ms); 0 disables (m4ri_amd_set_host_pipeline)
hipStream_t g_compute_stream[GF2_MAX_DEVICES];

// One block of A, B or C on the device.  ready: recorded on the null stream behind the block's upload and tail mask (a block of C that
// is not uploaded: behind its place in the arena); done (blocks of C only): recorded on the compute stream behind its last product
struct PipeBlock {
  DevMat d;
  hipEvent_t ready = nullptr, done = nullptr;
  bool issued = false;  // uploaded (or placed), `ready` recorded
};
struct PipeBlocks {  // all blocks of one call; their events exist from the start and go with this object
  std::vector<PipeBlock> A, B, C;
  PipeBlocks(int gi, int gj, int gk) : A((size_t)gi * gk), B((size_t)gk * gj), C((size_t)gi * gj) {
    for (auto *v : {&A, &B, &C})
      for (PipeBlock &b : *v) HIPDIE(hipEventCreateWithFlags(&b.ready, hipEventDisableTiming));
    for (PipeBlock &c : C) HIPDIE(hipEventCreateWithFlags(&c.done, hipEventDisableTiming));
  }
  ~PipeBlocks() {
    for (auto *v : {&A, &B, &C})
      for (PipeBlock &b : *v)
        for (hipEvent_t e : {b.ready, b.done})
          if (e) (void)hipEventDestroy(e);
  }
};

// M4RI_AMD_PIPE_TRACE=1: the timeline of a pipelined call on stderr (host clock for the copies, HIP events for the products; read by
// tools/host_pipeline_trace.py).  Unset, every member returns at once.
struct PipeTrace {
  struct Mark { char what; int a, b; double t0, t1; };
  struct Product { int t, k; hipEvent_t e0, e1; };
  const bool on;
  const hipStream_t cs;
  timespec origin;
  std::mutex mu;  // the downloader marks its copies too
  std::vector<Mark> marks;
  std::vector<Product> products;
  hipEvent_t base = nullptr;  // the compute stream's clock ...
  double base_ms  = 0;        // ... on the host's

  explicit PipeTrace(hipStream_t compute) : on(enabled()), cs(compute) { clock_gettime(CLOCK_MONOTONIC, &origin); }
  static bool enabled() { static const bool e = getenv("M4RI_AMD_PIPE_TRACE") != nullptr; return e; }
  double now() const {
    if (!on) return 0;
    timespec t;
    clock_gettime(CLOCK_MONOTONIC, &t);
    return 1e3 * (double)(t.tv_sec - origin.tv_sec) + 1e-6 * (double)(t.tv_nsec - origin.tv_nsec);
  }
  void copied(char what, int a, int b, double t0) {  // a copy that began at t0 = now() has returned
    if (!on) return;
    std::lock_guard<std::mutex> g(mu);
    marks.push_back({what, a, b, t0, now()});
  }
  hipEvent_t stamp() const {  // a timing event on the compute stream, here
    hipEvent_t e;
    HIPDIE(hipEventCreate(&e));
    HIPDIE(hipEventRecord(e, cs));
    return e;
  }
  void tie_clocks() { if (on) { base = stamp(); HIPDIE(hipEventSynchronize(base)); base_ms = now(); } }
  void product_begins(int t, int k) { if (on) products.push_back({t, k, stamp(), nullptr}); }
  void product_issued() { if (on) products.back().e1 = stamp(); }
  void print(int64_t m, int64_t l, int64_t n, const HostPipelinePlan &plan) {  // after the device has been synchronised
    if (!on) return;
    const double t_end = now();
    for (const Product &p : products) {
      float a = 0, b = 0;
      HIPDIE(hipEventElapsedTime(&a, base, p.e0));
      HIPDIE(hipEventElapsedTime(&b, base, p.e1));
      marks.push_back({'P', p.t, p.k, base_ms + a, base_ms + b});
      (void)hipEventDestroy(p.e0);
      (void)hipEventDestroy(p.e1);
    }
    (void)hipEventDestroy(base);
    std::sort(marks.begin(), marks.end(), [](const Mark &x, const Mark &y) { return x.t0 < y.t0; });
    fprintf(stderr, "m4ri_amd pipeline %lld x %lld x %lld, grid %d x %d x %d: %.2f ms (A/B = upload of block (i,k)/(k,j), P = product (block of C, slice), D = download)\n",
            (long long)m, (long long)l, (long long)n, plan.gi(), plan.gj(), plan.gk(), t_end);
    for (const Mark &k : marks) fprintf(stderr, "  %c(%d,%d) %8.2f .. %8.2f  (%6.2f ms)\n", k.what, k.a, k.b, k.t0, k.t1, k.t1 - k.t0);
  }
};

mzd_t block_of(const mzd_t *M, int64_t r0, int64_t r1, int64_t c0, int64_t c1) {  // mzd_init_window, mzd.c:159-177
  mzd_t S = *M;
  S.data  = M->data + r0 * M->rowstride + c0 / 64;
  S.nrows = (rci_t)(r1 - r0);
  S.ncols = (rci_t)(c1 - c0);
  S.width = (S.ncols + 63) / 64;
  S.high_bitmask = (~(word)0) >> ((64 - S.ncols % 64) % 64);
  // the block is a window unless it reaches M's own last column of a non-window M (then whole last words may be written)
  if ((M->flags & FLAG_WINDOW) || c1 != M->ncols) S.flags |= FLAG_WINDOW;
  return S;
}

// Executes the plan; returns false when the plan is not to pipeline (the product is too small to pay for it).  Step s = (block t of C in
// row-major order, inner slice k) is one product on the compute stream; a block of A, B or C goes up (C for C += A * B only) the first
// time a step needs it, and the blocks take their places in the arena in that order.
bool run_pipelined(mzd_t *C, const mzd_t *A, const mzd_t *B, bool add, int cutoff, LateC *late) {
  const int64_t m = A->nrows, l = A->ncols, n = B->ncols;
  static const char *grid_env = getenv("M4RI_AMD_PIPE_GRID");  // "gi,gj[,gk]": developer request for a block grid
  int egi = 0, egj = 0, egk = 1;
  if (!grid_env || sscanf(grid_env, "%d,%d,%d", &egi, &egj, &egk) < 2) egi = 0;
  const HostPipelinePlan plan = gf2_plan_host_pipeline(m, l, n, g_pipeline_min_bytes, egi, egj, egk);
  if (!plan.pipelined) return false;
  const std::vector<int64_t> &rcut = plan.rcut, &ccut = plan.ccut, &kcut = plan.kcut;
  const int gj = plan.gj(), gk = plan.gk(), nt = plan.gi() * gj, steps = nt * gk;
  int dev = 0;
  HIPDIE(hipGetDevice(&dev));
  hipStream_t &cs = g_compute_stream[dev];
  if (!cs) HIPDIE(hipStreamCreateWithFlags(&cs, hipStreamNonBlocking));
  arena_reserve(plan.arena_words);
  PipeTrace trace(cs);
  PipeBlocks blk(plan.gi(), gj, gk);
  auto c_block = [&](int t) {  // of a result still being allocated: first needed by the first download
    return block_of(late ? late->get() : C, rcut[(size_t)(t / gj)], rcut[(size_t)(t / gj) + 1], ccut[(size_t)(t % gj)], ccut[(size_t)(t % gj) + 1]);
  };
  auto ready = [](PipeBlock &b) { HIPDIE(hipEventRecord(b.ready, nullptr)); b.issued = true; };
  auto send = [&](PipeBlock &b, const mzd_t &S, char what, int x, int y) {  // host rows -> device (blocking), tail masks on the null stream
    const double t0 = trace.now();
    upload(b.d, &S);
    trace.copied(what, x, y, t0);
    ready(b);
  };
  auto need_for = [&](int s) {
    const int t = s / gk, k = s % gk, i = t / gj, j = t % gj;
    PipeBlock &a = blk.A[(size_t)i * gk + k], &b = blk.B[(size_t)k * gj + j], &c = blk.C[(size_t)t];
    if (!a.issued) send(a, block_of(A, rcut[(size_t)i], rcut[(size_t)i + 1], kcut[(size_t)k], kcut[(size_t)k + 1]), 'A', i, k);
    if (!b.issued) send(b, block_of(B, kcut[(size_t)k], kcut[(size_t)k + 1], ccut[(size_t)j], ccut[(size_t)j + 1]), 'B', k, j);
    if (!c.issued) {
      if (add) { const mzd_t S = c_block(t); upload(c.d, &S); }
      else dev_alloc(c.d, plan.rows(i), plan.cols(j));
      ready(c);
    }
  };
  auto product = [&](int s) {  // on the compute stream, behind the three blocks' events
    const int t = s / gk, k = s % gk, i = t / gj, j = t % gj;
    const PipeBlock &a = blk.A[(size_t)i * gk + k], &b = blk.B[(size_t)k * gj + j], &c = blk.C[(size_t)t];
    for (const PipeBlock *x : {&a, &b, &c}) HIPDIE(hipStreamWaitEvent(cs, x->ready, 0));
    trace.product_begins(t, k);
    product_dev(true, c.d, a.d, b.d, plan.rows(i), plan.inner(k), plan.cols(j), add || k > 0, cutoff, cs);
    trace.product_issued();
  };
  // The downloads run on a second host thread: a blocking copy holds its thread, and the blocks of C can travel down
  // while the next operands travel up (PCIe is full duplex: 53 GiB/s each way on this box, tools/pcie_probe_2d.py).
  std::mutex dl_mu;
  std::condition_variable dl_cv;
  int complete = 0;  // blocks of C, in order, whose `done` event has been recorded
  std::thread downloader([&]() {
    HIPDIE(hipSetDevice(dev));
    for (int t = 0; t < nt; ++t) {
      { std::unique_lock<std::mutex> lk(dl_mu); dl_cv.wait(lk, [&] { return complete > t; }); }
      HIPDIE(hipEventSynchronize(blk.C[(size_t)t].done));
      mzd_t S = c_block(t);
      const double t0 = trace.now();
      download(blk.C[(size_t)t].d, &S);
      trace.copied('D', t / gj, t % gj, t0);
    }
  });
  trace.tie_clocks();
  need_for(0);
  for (int s = 0; s < steps; ++s) {
    product(s);
    if (s % gk == gk - 1) {  // the block's last inner slice: complete once everything issued on the compute stream so far has run
      HIPDIE(hipEventRecord(blk.C[(size_t)(s / gk)].done, cs));
      { std::lock_guard<std::mutex> lk(dl_mu); complete += 1; }
      dl_cv.notify_one();
    }
    if (s + 1 < steps) need_for(s + 1);  // overlaps product s
  }
  downloader.join();
  HIPDIE(hipDeviceSynchronize());
  trace.print(m, l, n, plan);
  return true;
}

// the whole product: strassen == true runs the Strassen-Winograd engine, false a single leaf
// `late`: C == nullptr and the result is still being allocated (LateC; never with add, never empty)
mzd_t *run(mzd_t *C, const mzd_t *A, const mzd_t *B, bool add, bool strassen, int cutoff, LateC *late = nullptr) {
  const rci_t cm = A->nrows, cn = B->ncols;
  if (cm == 0 || cn == 0) return late ? late->get() : C;  // strassen.c:44
  HostCall call(HostCall::PRODUCT);
  const bool same = (A == B);
  const bool all_on_host = !find_pin(C) && !find_pin(A) && !find_pin(B);  // (C == nullptr, a late result: not pinned)
  // products the launch / PCIe floor of a call would dominate: this library's own host Four Russians (small_host.cpp), on an
  // initialised device and only for matrices that live in host memory (a pinned operand is already on the GPU)
  if (!late && all_on_host && small_product_wanted(cm, A->ncols, cn, g_small_threshold.load())) {
    call.lk.unlock();  // the routine needs no device state: small products of many threads run side by side
    if (m4ri_amd_small_mul_host(C, A, B, add ? 1 : 0)) die("m4ri_amd: small product failed (internal error)\n");
    g_small_count += 1;
    return C;
  }
  if (strassen && !same && all_on_host && run_pipelined(C, A, B, add, cutoff, late)) return late ? late->get() : C;
  // nothing pinned and a few MiB in all: one asynchronous transfer each way through the device's pinned buffer
  if (!late && all_on_host) {
    const size_t wa = dev_words(A->nrows, A->ncols), wb = same ? 0 : dev_words(B->nrows, B->ncols), wc = dev_words(cm, cn);
    if ((wa + wb + wc) * 8 <= SMALL_STAGE_BYTES) {
      arena_reserve(wa + wb + wc);
      word *hs = host_stage(call.dev, wa + wb + wc);
      DevMat dA, dB, dC;
      dev_alloc(dA, A->nrows, A->ncols);
      if (same) dB = dA; else dev_alloc(dB, B->nrows, B->ncols);
      dev_alloc(dC, cm, cn);
      pack_rows(hs, dA.stride, A);
      if (!same) pack_rows(hs + wa, dB.stride, B);
      if (add) pack_rows(hs + wa + wb, dC.stride, C);
      const size_t up = (wa + wb + (add ? wc : 0)) * 8;
      HIPDIE(hipMemcpyAsync(dA.p, hs, up, hipMemcpyHostToDevice, nullptr));   // dA, dB, dC are consecutive in the arena, like hs
      product_dev(strassen, dC, dA, dB, A->nrows, A->ncols, B->ncols, add, cutoff, nullptr);
      HIPDIE(hipMemcpyAsync(hs + wa + wb, dC.p, wc * 8, hipMemcpyDeviceToHost, nullptr));
      HIPDIE(hipStreamSynchronize(nullptr));
      unpack_rows(C, hs + wa + wb, dC.stride);
      { std::lock_guard<std::mutex> sl(g_stats_mu); g_api_stats.h2d += (double)up; g_api_stats.d2h += (double)wc * 8.0; }
      return C;
    }
  }
  // the general path: every operand by the placement rule; a result still on its way (late) has room in staging and is first
  // dereferenced when it is downloaded
  Operand &a = call.in(A), &b = same ? a : call.in(B);
  Operand &c = late ? call.space(cm, cn) : add ? call.inout(C) : call.out(C);
  call.stage();
  const DevMat dC = c.d;
  product_dev(strassen, dC, a.d, b.d, A->nrows, A->ncols, B->ncols, add, cutoff, nullptr);
  // a B that is a window of a pinned parent carries its neighbours' bits in the last word, and they
  // land in C's excess columns: clear them before the result leaves the staging buffer
  // (an unstaged pinned C spans its parent's full width, so its excess bits must be zero anyway:
  // mzd.h:115-121 -- mask there as well, or sync/unpin would carry the neighbours' bits to the host)
  if (c.staged() || cn % 64 != 0) HIPDIE(m4ri_amd_mask_tail_dev(dC.p, dC.stride, cm, cn, nullptr));
  if (late) HostCall::download_to(c, C = late->get());
  call.finish();
  return C;
}

// B <- T^-1 B (left) or B <- B T^-1 (right) for a unit triangular T (triangular.c:41-514); T's other triangle and
// diagonal are never read
void run_trsm(bool upper, const mzd_t *T, mzd_t *B, int cutoff, bool right = false) {
  if (B->nrows == 0 || B->ncols == 0 || (!right && B->nrows <= 1) || (right && B->ncols <= 1)) return;  // one unknown per system: X = B
  HostCall call;
  // T as the solver wants it: bits beyond its last column clean (trsm.hip: solve()).  A ragged window into a pinned parent
  // carries the parent's neighbouring columns in its last word: such a T is solved from a masked copy, like an in/out matrix
  Operand &t = call.in(T, /*clean_tail=*/true), &b = call.inout(B);
  call.stage();
  typedef int (*trsm_dev_fn)(const word *, int64_t, word *, int64_t, int64_t, int64_t, int, void *);
  static const trsm_dev_fn fn[2][2] = {{m4ri_amd_trsm_lower_left_dev, m4ri_amd_trsm_upper_left_dev},
                                       {m4ri_amd_trsm_lower_right_dev, m4ri_amd_trsm_upper_right_dev}};
  HIPDIE(fn[right][upper](t.d.p, t.d.stride, b.d.p, b.d.stride, B->nrows, B->ncols, cutoff, nullptr));
  call.finish();
}

void pin_download(Pin &p) {
  if (!is_newer(p)) return;
  const int64_t width = words_of(p.ncols);
  if (p.nrows && width)
    HIPDIE(hipMemcpy2D(const_cast<word *>(p.hbase), (size_t)p.rowstride * 8, p.dbase, (size_t)p.rowstride * 8, (size_t)width * 8,
                       (size_t)p.nrows, hipMemcpyDeviceToHost));
  set_newer(p, false);
}

void pin_upload(Pin &p) {
  const int64_t width = words_of(p.ncols);
  if (p.nrows && width) {
    HIPDIE(hipMemcpy(p.dbase, p.hbase, p.words * 8, hipMemcpyHostToDevice));  // padding words included: same layout
    HIPDIE(m4ri_amd_mask_tail_dev(p.dbase, p.rowstride, p.nrows, p.ncols, nullptr));
    HIPDIE(hipDeviceSynchronize());
  }
  set_newer(p, false);
}

}  // namespace

extern "C" {

mzd_t *m4ri_amd_mzd_init(rci_t r, rci_t c) {  // mzd.c:142-157
  mzd_t *A = descriptor(r, c);
  if (!A) die("m4ri_amd_mzd_init: out of memory\n");
  if (r && c) {
    void *p = nullptr;
    const size_t bytes = (size_t)r * (size_t)A->rowstride * 8;
    if (bytes >= BIG_BLOCK) {
      // large blocks: a mapping of their own, 2 MiB-aligned (whole transparent huge pages where the system serves them) -- the kernel
      // hands out zero pages, so nothing is cleared and no page is touched before somebody needs it (a fresh 512 MiB block used to
      // cost 87 ms of page faults under one memset, 33 ms under 32 threads); a parked block of that size is cleared and reused.
      // (No MADV_HUGEPAGE: with the usual defrag = madvise setting it makes every fault compact memory synchronously.)
      const size_t len = big_len(bytes);
      if ((p = g_big_cache.take(len)) != nullptr) zero_with_threads(static_cast<char *>(p), bytes);
      else if ((p = big_map(len)) == nullptr) die("m4ri_amd_mzd_init: out of memory\n");
    } else {
      if (posix_memalign(&p, 64, bytes)) die("m4ri_amd_mzd_init: out of memory\n");
      memset(p, 0, bytes);
    }
    A->data = static_cast<word *>(p);
  }
  return A;
}

void m4ri_amd_mzd_free(mzd_t *A) {  // mzd.c:179-185
  if (!A) return;
  if (!(A->flags & FLAG_WINDOW) && A->data) {
    const size_t bytes = (size_t)A->nrows * (size_t)A->rowstride * 8;
    if (bytes >= BIG_BLOCK) {  // m4ri_amd_mzd_init: large blocks are mappings of their own; the cache may keep this one
      if (!g_big_cache.park(A->data, big_len(bytes))) munmap(A->data, big_len(bytes));
    } else free(A->data);
  }
  free(A);
}

// C == NULL at a product entry point: the product into a fresh matrix -- allocated beside the upload and the first products
// when it is large (LateC), in front of them when it is small or the product is empty (the zero matrix)
static mzd_t *run_fresh(mzd_t const *A, mzd_t const *B, bool strassen, int cutoff) {
  const rci_t r = A->nrows, c = B->ncols;
  const size_t bytes = (size_t)r * (size_t)((c + 63) / 64) * 8;
  if (bytes < BIG_BLOCK || A->ncols == 0) {
    mzd_t *C = result_init(r, c);
    return (r == 0 || c == 0 || A->ncols == 0) ? C : run(C, A, B, false, strassen, cutoff);
  }
  LateC late;
  late_begin(late, r, c);
  run(nullptr, A, B, false, strassen, cutoff, &late);
  return late.finish();
}

mzd_t *mzd_mul(mzd_t *C, mzd_t const *A, mzd_t const *B, int cutoff) {  // strassen.c:345-365
  if (A->ncols != B->nrows) die("mzd_mul: A ncols (%d) need to match B nrows (%d).\n", A->ncols, B->nrows);
  cutoff = norm_cutoff(cutoff, "mzd_mul");
  if (C == NULL) return run_fresh(A, B, true, cutoff);
  else if (C->nrows != A->nrows || C->ncols != B->ncols)
    die("mzd_mul: C (%d x %d) has wrong dimensions, expected (%d x %d)\n", C->nrows, C->ncols, A->nrows, B->ncols);
  return run(C, A, B, false, true, cutoff);
}

mzd_t *mzd_addmul(mzd_t *C, mzd_t const *A, mzd_t const *B, int cutoff) {  // strassen.c:675-700
  if (A->ncols != B->nrows) die("mzd_addmul: A ncols (%d) need to match B nrows (%d).\n", A->ncols, B->nrows);
  cutoff = norm_cutoff(cutoff, "mzd_addmul");
  if (C == NULL) return run_fresh(A, B, true, cutoff);  // 0 + A*B
  else if (C->nrows != A->nrows || C->ncols != B->ncols)
    die("mzd_addmul: C (%d x %d) has wrong dimensions, expected (%d x %d)\n", C->nrows, C->ncols, A->nrows, B->ncols);
  if (A->nrows == 0 || A->ncols == 0 || B->ncols == 0) return C;
  return run(C, A, B, true, true, cutoff);
}

mzd_t *_mzd_mul_even(mzd_t *C, mzd_t const *A, mzd_t const *B, int cutoff) { return run(C, A, B, false, true, cutoff); }
mzd_t *_mzd_addmul_even(mzd_t *C, mzd_t const *A, mzd_t const *B, int cutoff) { return run(C, A, B, true, true, cutoff); }
mzd_t *_mzd_addmul(mzd_t *C, mzd_t const *A, mzd_t const *B, int cutoff) { return run(C, A, B, true, true, cutoff); }
mzd_t *_mzd_sqr_even(mzd_t *C, mzd_t const *A, int cutoff) { return run(C, A, A, false, true, cutoff); }
mzd_t *_mzd_addsqr_even(mzd_t *C, mzd_t const *A, int cutoff) { return run(C, A, A, true, true, cutoff); }

mzd_t *mzd_mul_m4rm(mzd_t *C, mzd_t const *A, mzd_t const *B, int k) {  // brilliantrussian.c:999-1012
  (void)k;
  if (A->ncols != B->nrows) die("mzd_mul_m4rm: A ncols (%d) need to match B nrows (%d).\n", A->ncols, B->nrows);
  if (C == NULL) return run_fresh(A, B, false, 0);
  else if (C->nrows != A->nrows || C->ncols != B->ncols)
    die("mzd_mul_m4rm: C (%d x %d) has wrong dimensions.\n", C->nrows, C->ncols);
  return run(C, A, B, false, false, 0);
}

mzd_t *mzd_addmul_m4rm(mzd_t *C, mzd_t const *A, mzd_t const *B, int k) {  // brilliantrussian.c:1014-1028
  (void)k;
  if (C == NULL) die("mzd_addmul_m4rm: C must not be NULL.\n");  // the reference dereferences C first (:1018)
  if (C->ncols == 0 || C->nrows == 0) return C;
  if (A->ncols != B->nrows) die("mzd_mul_m4rm A ncols (%d) need to match B nrows (%d) .\n", A->ncols, B->nrows);
  if (C->nrows != A->nrows || C->ncols != B->ncols) die("mzd_mul_m4rm: C has wrong dimensions.\n");
  return run(C, A, B, true, false, 0);
}

mzd_t *_mzd_mul_m4rm(mzd_t *C, mzd_t const *A, mzd_t const *B, int k, int clear) {  // brilliantrussian.c:1032
  (void)k;
  return run(C, A, B, clear == 0, false, 0);
}

int64_t m4ri_amd_set_small_product_threshold(int64_t ops) {
  const int64_t old = g_small_threshold;
  if (ops >= 0) g_small_threshold = ops;
  return old;
}

int64_t m4ri_amd_small_product_count(void) { return g_small_count; }

int m4ri_amd_small_product_wanted(int64_t m, int64_t l, int64_t n) { return small_product_wanted(m, l, n, g_small_threshold.load()) ? 1 : 0; }

// A + B + C bytes from which the host entry points pipeline a product over row slabs (0: never); returns the previous value
int64_t m4ri_amd_set_host_pipeline(int64_t min_bytes) {
  const std::unique_lock<std::mutex> lk = lock_current_device();
  const int64_t old = (int64_t)g_pipeline_min_bytes;
  if (min_bytes >= 0) g_pipeline_min_bytes = (size_t)min_bytes;
  return old;
}

// ---- triangular solves: the reference's names, host mzd_t in / out -------------
void mzd_trsm_lower_left(mzd_t const *L, mzd_t *B, const int cutoff) {  // triangular.c:396-404
  if (L->ncols != B->nrows) die("mzd_trsm_lower_left: L ncols (%d) need to match B nrows (%d).\n", L->ncols, B->nrows);
  if (L->nrows != L->ncols) die("mzd_trsm_lower_left: L must be square and is found to be (%d) x (%d).\n", L->nrows, L->ncols);
  run_trsm(false, L, B, cutoff < 0 ? 0 : cutoff);
}
void _mzd_trsm_lower_left(mzd_t const *L, mzd_t *B, const int cutoff) { run_trsm(false, L, B, cutoff < 0 ? 0 : cutoff); }  // triangular.c:406
void _mzd_trsm_lower_left_russian(mzd_t const *L, mzd_t *B, int k) { (void)k; run_trsm(false, L, B, 0); }  // triangular_russian.c:206

void mzd_trsm_upper_left(mzd_t const *U, mzd_t *B, const int cutoff) {  // triangular.c:457-465
  if (U->ncols != B->nrows) die("mzd_trsm_upper_left: U ncols (%d) need to match B nrows (%d).\n", U->ncols, B->nrows);
  if (U->nrows != U->ncols) die("mzd_trsm_upper_left: U must be square and is found to be (%d) x (%d).\n", U->nrows, U->ncols);
  run_trsm(true, U, B, cutoff < 0 ? 0 : cutoff);
}
void _mzd_trsm_upper_left(mzd_t const *U, mzd_t *B, const int cutoff) { run_trsm(true, U, B, cutoff < 0 ? 0 : cutoff); }  // triangular.c:467
void _mzd_trsm_upper_left_russian(mzd_t const *U, mzd_t *B, int k) { (void)k; run_trsm(true, U, B, 0); }  // triangular_russian.c:50

void mzd_trsm_upper_right(mzd_t const *U, mzd_t *B, const int cutoff) {  // triangular.c:41-50
  if (U->nrows != B->ncols) die("mzd_trsm_upper_right: U nrows (%d) need to match B ncols (%d).\n", U->nrows, B->ncols);
  if (U->nrows != U->ncols) die("mzd_trsm_upper_right: U must be square and is found to be (%d) x (%d).\n", U->nrows, U->ncols);
  run_trsm(true, U, B, cutoff < 0 ? 0 : cutoff, true);
}
void _mzd_trsm_upper_right(mzd_t const *U, mzd_t *B, const int cutoff) { run_trsm(true, U, B, cutoff < 0 ? 0 : cutoff, true); }  // triangular.c:61
void mzd_trsm_lower_right(mzd_t const *L, mzd_t *B, const int cutoff) {  // triangular.c:301-310
  if (L->nrows != B->ncols) die("mzd_trsm_lower_right: L nrows (%d) need to match B ncols (%d).\n", L->nrows, B->ncols);
  if (L->nrows != L->ncols) die("mzd_trsm_lower_right: L must be square and is found to be (%d) x (%d).\n", L->nrows, L->ncols);
  run_trsm(false, L, B, cutoff < 0 ? 0 : cutoff, true);
}
void _mzd_trsm_lower_right(mzd_t const *L, mzd_t *B, const int cutoff) { run_trsm(false, L, B, cutoff < 0 ? 0 : cutoff, true); }  // triangular.c:312

// ---- PLE decomposition: the reference's names, host mzd_t / mzp_t in and out ---------
static rci_t run_ple(mzd_t *A, mzp_t *P, mzp_t *Q, bool pluq, bool russian) {
  if (A->nrows == 0 || A->ncols == 0) {
    for (rci_t i = 0; i < A->nrows; ++i) P->values[i] = i;
    for (rci_t j = 0; j < A->ncols; ++j) Q->values[j] = j;
    return 0;
  }
  HostCall call;
  Operand &a = call.inout(A);
  call.stage();
  int32_t rank = 0;
  HIPDIE((pluq ? m4ri_amd_pluq_dev : m4ri_amd_ple_dev)(a.d.p, a.d.stride, A->nrows, A->ncols, P->values, Q->values, &rank,
                                                       russian ? 0 : M4RI_AMD_PLE_CUTOFF, nullptr));
  call.finish();
  return rank;
}

rci_t mzd_ple(mzd_t *A, mzp_t *P, mzp_t *Q, const int cutoff) {  // ple.c:33-39
  (void)cutoff;
  if (P->length != A->nrows) die("mzd_ple: Permutation P length (%d) must match A nrows (%d)\n", P->length, A->nrows);
  if (Q->length != A->ncols) die("mzd_ple: Permutation Q length (%d) must match A ncols (%d)\n", Q->length, A->ncols);
  return run_ple(A, P, Q, false, false);
}
rci_t _mzd_ple(mzd_t *A, mzp_t *P, mzp_t *Q, const int cutoff) { (void)cutoff; return run_ple(A, P, Q, false, false); }  // ple.c:62-171
rci_t _mzd_ple_russian(mzd_t *A, mzp_t *P, mzp_t *Q, int k) { (void)k; return run_ple(A, P, Q, false, true); }           // ple_russian.c:380-617

rci_t mzd_pluq(mzd_t *A, mzp_t *P, mzp_t *Q, const int cutoff) {  // ple.c:41-48
  (void)cutoff;
  if (P->length != A->nrows) die("mzd_pluq: Permutation P length (%d) must match A nrows (%d)\n", P->length, A->nrows);
  if (Q->length != A->ncols) die("mzd_pluq: Permutation Q length (%d) must match A ncols (%d)\n", Q->length, A->ncols);
  return run_ple(A, P, Q, true, false);
}
rci_t _mzd_pluq(mzd_t *A, mzp_t *P, mzp_t *Q, const int cutoff) { (void)cutoff; return run_ple(A, P, Q, true, false); }  // ple.c:50-60
rci_t _mzd_pluq_russian(mzd_t *A, mzp_t *P, mzp_t *Q, int k) { (void)k; return run_ple(A, P, Q, true, true); }         // ple_russian.c:625-629

void mzd_apply_p_right_trans_tri(mzd_t *A, mzp_t const *Q) {  // mzp.c:279-293
  if (Q->length != A->ncols) die("mzd_apply_p_right_trans_tri: Permutation length (%d) must match A ncols (%d)\n", Q->length, A->ncols);
  if (A->nrows == 0 || A->ncols == 0) return;
  HostCall call;
  Operand &a = call.inout(A);
  call.stage();
  HIPDIE(m4ri_amd_apply_p_right_trans_tri_dev(a.d.p, a.d.stride, A->nrows, A->ncols, Q->values, nullptr));
  call.finish();
}

// ---- echelon forms and the column permutations (echelon.hip) -----------------------------------------------------
static rci_t run_echelonize(mzd_t *A, int full) {
  if (A->nrows == 0 || A->ncols == 0) return 0;
  HostCall call;
  Operand &a = call.inout(A);
  call.stage();
  int32_t rank = 0;
  HIPDIE(m4ri_amd_echelonize_dev(a.d.p, a.d.stride, A->nrows, A->ncols, full, &rank, nullptr));
  call.finish();
  return rank;
}
rci_t mzd_echelonize(mzd_t *A, int full) { return run_echelonize(A, full); }                  // echelonform.c:29-31
rci_t mzd_echelonize_m4ri(mzd_t *A, int full, int k) { (void)k; return run_echelonize(A, full); }  // echelonform.c:33-35
rci_t mzd_echelonize_pluq(mzd_t *A, int full) { return run_echelonize(A, full); }             // echelonform.c:37-139
rci_t mzd_echelonize_naive(mzd_t *A, int full) { return run_echelonize(A, full); }            // mzd.c:208-233: plain Gauss(-Jordan), the same pivoting rule, the same matrix
rci_t _mzd_echelonize_m4ri(mzd_t *A, const int full, int k, int heuristic, const double threshold) {  // brilliantrussian.c:603-841
  (void)k; (void)heuristic; (void)threshold;
  return run_echelonize(A, full);
}

static void run_apply_p_right(mzd_t *A, mzp_t const *P, int trans) {  // mzp.c:193-260
  if (A->nrows == 0 || A->ncols == 0) return;
  HostCall call;
  Operand &a = call.inout(A);
  call.stage();
  HIPDIE(m4ri_amd_apply_p_right_dev(a.d.p, a.d.stride, A->nrows, A->ncols, P->values, P->length, trans, nullptr));
  call.finish();
}
void mzd_apply_p_right(mzd_t *A, mzp_t const *P) { run_apply_p_right(A, P, 0); }
void mzd_apply_p_right_trans(mzd_t *A, mzp_t const *P) { run_apply_p_right(A, P, 1); }

// ---- the drivers over PLUQ: systems, kernels, inverses, row permutations (solve.hip) ---------------------------------
static void run_apply_p_left(mzd_t *A, mzp_t const *P, int trans) {  // mzp.c:65-81
  if (A->nrows == 0 || A->ncols == 0) return;
  HostCall call;
  Operand &a = call.inout(A);
  call.stage();
  HIPDIE(m4ri_amd_apply_p_left_dev(a.d.p, a.d.stride, A->nrows, A->ncols, P->values, P->length, trans, nullptr));
  call.finish();
}
void mzd_apply_p_left(mzd_t *A, mzp_t const *P) { run_apply_p_left(A, P, 0); }
void mzd_apply_p_left_trans(mzd_t *A, mzp_t const *P) { run_apply_p_left(A, P, 1); }

// A == nullptr-decomposition variant: rank/P/Q given (mzd_pluq_solve_left); otherwise A is decomposed in place
static int run_solve_left(mzd_t *A, mzd_t const *Adec, rci_t rank, mzp_t const *P, mzp_t const *Q, mzd_t *B, int cutoff, int check) {
  HostCall call;
  int retval = 0;
  if (cutoff < 0) cutoff = 0;
  Operand &a = A ? call.inout(A) : call.in(Adec), &b = call.inout(B);
  call.stage();
  if (A)
    HIPDIE(m4ri_amd_solve_left_dev(a.d.p, a.d.stride, A->nrows, A->ncols, b.d.p, b.d.stride, B->nrows, B->ncols, cutoff, check, &retval, nullptr));
  else
    HIPDIE(m4ri_amd_pluq_solve_left_dev(a.d.p, a.d.stride, Adec->nrows, Adec->ncols, rank, P->values, Q->values, b.d.p, b.d.stride, B->nrows, B->ncols,
                                        cutoff, check, &retval, nullptr));
  call.finish();
  return retval;
}

int mzd_solve_left(mzd_t *A, mzd_t *B, int const cutoff, int const inconsistency_check) {  // solve.c:30-40
  if (A->ncols > B->nrows) die("mzd_solve_left: A ncols (%d) must be smaller than B nrows (%d).\n", A->ncols, B->nrows);
  if (B->nrows != (A->ncols > A->nrows ? A->ncols : A->nrows))
    die("mzd_solve_left: B nrows (%d) must be equal to max of A nrows (%d) and A ncols (%d).\n", B->nrows, A->nrows, A->ncols);
  return run_solve_left(A, nullptr, 0, nullptr, nullptr, B, cutoff, inconsistency_check);
}
int _mzd_solve_left(mzd_t *A, mzd_t *B, int const cutoff, int const inconsistency_check) {  // solve.c:123-152
  return run_solve_left(A, nullptr, 0, nullptr, nullptr, B, cutoff, inconsistency_check);
}
int mzd_pluq_solve_left(mzd_t const *A, rci_t rank, mzp_t const *P, mzp_t const *Q, mzd_t *B, int const cutoff, int const inconsistency_check) {  // solve.c:42-55
  if (A->ncols > B->nrows) die("mzd_pluq_solve_left: A ncols (%d) need to be lower than B nrows (%d).\n", A->ncols, B->nrows);
  if (P->length != A->nrows) die("mzd_pluq_solve_left: A nrows (%d) need to match P size (%d).\n", A->nrows, P->length);
  if (Q->length != A->ncols) die("mzd_pluq_solve_left: A ncols (%d) need to match Q size (%d).\n", A->ncols, P->length);
  return run_solve_left(nullptr, A, rank, P, Q, B, cutoff, inconsistency_check);
}
int _mzd_pluq_solve_left(mzd_t const *A, rci_t rank, mzp_t const *P, mzp_t const *Q, mzd_t *B, int const cutoff, int const inconsistency_check) {  // solve.c:57-121
  return run_solve_left(nullptr, A, rank, P, Q, B, cutoff, inconsistency_check);
}

mzd_t *mzd_kernel_left_pluq(mzd_t *A, int const cutoff) {  // solve.c:154-191
  HostCall call;
  if (A->ncols == 0) return nullptr;  // rank 0 == ncols
  if (A->nrows == 0) {                // rank 0: every vector is in the kernel (solve.c:168-180 leaves the identity)
    mzd_t *I = result_init(A->ncols, A->ncols);
    for (rci_t i = 0; i < A->ncols; ++i) I->data[(int64_t)i * I->rowstride + i / 64] |= (word)1 << (i % 64);
    return I;
  }
  Operand &a = call.inout(A), &r = call.space(A->ncols, A->ncols);  // the kernel has at most ncols columns; its real width is known after the PLUQ
  call.stage();
  const DevMat dR = r.d;
  HIPDIE(hipMemsetAsync(dR.p, 0, (size_t)A->ncols * dR.stride * 8, nullptr));
  int32_t rank = 0;
  HIPDIE(m4ri_amd_kernel_left_pluq_dev(a.d.p, a.d.stride, A->nrows, A->ncols, dR.p, dR.stride, cutoff < 0 ? 0 : cutoff, &rank, nullptr));
  mzd_t *R = nullptr;
  if (rank < A->ncols) HostCall::download_to(r, R = result_init(A->ncols, A->ncols - rank));
  call.finish();
  return R;
}

mzd_t *mzd_inv_m4ri(mzd_t *B, mzd_t const *A, int k) {  // brilliantrussian.c:971-997
  (void)k;
  if (A->nrows != A->ncols) die("mzd_inv_m4ri: A must be square and is found to be (%d) x (%d).\n", A->nrows, A->ncols);
  if (B == nullptr) B = result_init(A->nrows, A->ncols);
  else if (B->nrows != A->nrows || B->ncols != A->ncols) die("mzd_inv_m4ri: B (%d x %d) has wrong dimensions.\n", B->nrows, B->ncols);
  if (A->nrows == 0) return B;
  HostCall call;
  // m4ri_amd_inv_dev wants the bits beyond A's last column zero (its elimination of [A | I] reads whole words of A): a ragged
  // window of a pinned parent is inverted from a masked copy, like the T of a triangular solve
  Operand &a = call.in(A, /*clean_tail=*/true), &b = call.inout(B);
  call.stage();
  HIPDIE(m4ri_amd_inv_dev(b.d.p, b.d.stride, a.d.p, a.d.stride, A->nrows, nullptr));
  call.finish();
  return B;
}

// ---- transposes and triangular inverses (transpose.hip, trsm.hip) ----------------------------------------------------
mzd_t *mzd_transpose(mzd_t *DST, mzd_t const *A) {  // mzd.c:1118-1139
  if (DST == nullptr) DST = result_init(A->ncols, A->nrows);
  else if (DST->nrows != A->ncols || DST->ncols != A->nrows) die("mzd_transpose: Wrong size for return matrix.\n");
  if (A->nrows == 0 || A->ncols == 0) return DST;
  HostCall call;
  // the result is always built in staging: DST may be A itself, a window with neighbours in its last word, or pinned
  Operand &a = call.in(A), &d = call.out(DST, /*always_staged=*/true);
  call.stage();
  HIPDIE(m4ri_amd_transpose_dev(d.d.p, d.d.stride, a.d.p, a.d.stride, A->nrows, A->ncols, nullptr));
  call.finish();
  return DST;
}

static mzd_t *run_trtri_upper(mzd_t *A, const char *who) {  // triangular.c:518-547, triangular_russian.c:384-470
  if (A->nrows != A->ncols) die("%s: matrix must be square and is found to be (%d) x (%d).\n", who, A->nrows, A->ncols);
  if (A->nrows <= 1) return A;
  HostCall call;
  Operand &a = call.inout(A);
  call.stage();
  HIPDIE(m4ri_amd_trtri_upper_dev(a.d.p, a.d.stride, A->nrows, nullptr));
  call.finish();
  return A;
}
mzd_t *mzd_trtri_upper(mzd_t *A) { return run_trtri_upper(A, "mzd_trtri_upper"); }
mzd_t *mzd_trtri_upper_russian(mzd_t *A, int k) { (void)k; return run_trtri_upper(A, "mzd_trtri_upper_russian"); }

// ---- the table primitives of the elimination routines (elim.hip) -------------------------
// how mzd_process_rowsN cuts the k-bit strip into N groups, lowest bits first (brilliantrussian.c:357-361,
// :394-398, :440-445, :490-494, :546-552)
static void split_k(int k, int n, int32_t *kb) {
  if (n == 1) { kb[0] = k; return; }
  if (n == 2) { kb[0] = k / 2; kb[1] = k - k / 2; return; }
  const int rem = k % n;
  for (int i = 0; i < n; ++i) kb[i] = k / n + ((i < n - 1 && rem >= n - 1 - i) ? 1 : 0);
}

static void run_process_rows(mzd_t *M, rci_t startrow, rci_t stoprow, rci_t startcol, int k, int nt, mzd_t const *const *T,
                             rci_t const *const *L) {
  if (stoprow <= startrow || M->ncols == 0) return;
  HostCall call;
  int32_t kb[6] = {0, 0, 0, 0, 0, 0};
  split_k(k, nt, kb);
  mzd_t W = *M;  // the rows that are touched, as a window of M
  W.data  = M->data + (int64_t)startrow * M->rowstride;
  W.nrows = stoprow - startrow;
  W.flags |= FLAG_WINDOW;
  Operand &w = call.inout(&W);
  Operand *tab[6], *lst[6];
  for (int t = 0; t < nt; ++t) {  // each table, then its list of 2^kb int32 indices
    const size_t n = (size_t)1 << kb[t];
    tab[t] = &call.in(T[t]);
    lst[t] = &call.words(n / 2 + 1, L[t], n * 4);
  }
  Operand &idx = call.words((size_t)3 * (size_t)W.nrows);  // the kernels' own: three words per row
  call.stage();
  const word *dT[6];
  int64_t ts[6];
  const int32_t *dL[6];
  for (int t = 0; t < nt; ++t) {
    dT[t] = tab[t]->d.p; ts[t] = tab[t]->d.stride;
    dL[t] = reinterpret_cast<const int32_t *>(lst[t]->d.p);
  }
  HIPDIE(m4ri_amd_process_rows_dev(w.d.p, w.d.stride, M->width, 0, W.nrows, startcol, nt, kb, dT, ts, dL, reinterpret_cast<int32_t *>(idx.d.p), nullptr));
  call.finish();
}

void mzd_process_rows(mzd_t *M, rci_t startrow, rci_t endrow, rci_t startcol, int k, mzd_t const *T, rci_t const *L) {  // brilliantrussian.c:213
  run_process_rows(M, startrow, endrow, startcol, k, 1, &T, &L);
}
void mzd_process_rows2(mzd_t *M, rci_t startrow, rci_t endrow, rci_t startcol, int k, mzd_t const *T0, rci_t const *L0, mzd_t const *T1,
                       rci_t const *L1) {  // :350
  mzd_t const *T[2] = {T0, T1}; rci_t const *L[2] = {L0, L1};
  run_process_rows(M, startrow, endrow, startcol, k, 2, T, L);
}
void mzd_process_rows3(mzd_t *M, rci_t startrow, rci_t endrow, rci_t startcol, int k, mzd_t const *T0, rci_t const *L0, mzd_t const *T1,
                       rci_t const *L1, mzd_t const *T2, rci_t const *L2) {  // :386
  mzd_t const *T[3] = {T0, T1, T2}; rci_t const *L[3] = {L0, L1, L2};
  run_process_rows(M, startrow, endrow, startcol, k, 3, T, L);
}
void mzd_process_rows4(mzd_t *M, rci_t startrow, rci_t endrow, rci_t startcol, int k, mzd_t const *T0, rci_t const *L0, mzd_t const *T1,
                       rci_t const *L1, mzd_t const *T2, rci_t const *L2, mzd_t const *T3, rci_t const *L3) {  // :431
  mzd_t const *T[4] = {T0, T1, T2, T3}; rci_t const *L[4] = {L0, L1, L2, L3};
  run_process_rows(M, startrow, endrow, startcol, k, 4, T, L);
}
void mzd_process_rows5(mzd_t *M, rci_t startrow, rci_t endrow, rci_t startcol, int k, mzd_t const *T0, rci_t const *L0, mzd_t const *T1,
                       rci_t const *L1, mzd_t const *T2, rci_t const *L2, mzd_t const *T3, rci_t const *L3, mzd_t const *T4,
                       rci_t const *L4) {  // :481
  mzd_t const *T[5] = {T0, T1, T2, T3, T4}; rci_t const *L[5] = {L0, L1, L2, L3, L4};
  run_process_rows(M, startrow, endrow, startcol, k, 5, T, L);
}
void mzd_process_rows6(mzd_t *M, rci_t startrow, rci_t endrow, rci_t startcol, int k, mzd_t const *T0, rci_t const *L0, mzd_t const *T1,
                       rci_t const *L1, mzd_t const *T2, rci_t const *L2, mzd_t const *T3, rci_t const *L3, mzd_t const *T4,
                       rci_t const *L4, mzd_t const *T5, rci_t const *L5) {  // :537
  mzd_t const *T[6] = {T0, T1, T2, T3, T4, T5}; rci_t const *L[6] = {L0, L1, L2, L3, L4, L5};
  run_process_rows(M, startrow, endrow, startcol, k, 6, T, L);
}

void mzd_make_table(mzd_t const *M, rci_t r, rci_t c, int k, mzd_t *T, rci_t *L) {  // brilliantrussian.c:163-211
  const int twokay = 1 << k;
  std::vector<int32_t> jstar((size_t)twokay, 0);
  L[0] = 0;
  int js = 0;
  for (int i = 1; i < twokay; ++i) {
    L[i ^ (i >> 1)] = i;                                  // ord[i] = the reflected Gray code (graycode.c:31-62)
    if (r + __builtin_ctz((unsigned)i) >= M->nrows) js = i;  // inc[i-1] = the bit that flips: that row does not exist (:181)
    jstar[(size_t)i] = js;
  }
  if (M->ncols == 0 || c / 64 >= M->width) return;
  HostCall call(HostCall::UNCOUNTED);  // the statistics have never counted the tables, only the calls that use them
  mzd_t W = *M;  // the k source rows
  W.data  = M->data + (int64_t)r * M->rowstride;
  W.nrows = (r + k <= M->nrows) ? k : (M->nrows > r ? M->nrows - r : 0);
  W.flags |= FLAG_WINDOW;
  // T is outside the placement rule: a pinned T IS its device copy, whatever its shape, and the table is built there (the host copy
  // goes stale like any pinned result); any other T gets room in staging and partial, unmasked copies of its own, below
  Pin *pinT      = find_pin(T);
  Operand *rows  = W.nrows > 0 ? &call.in(&W) : nullptr;
  Operand *room  = pinT ? nullptr : &call.space(T->nrows, T->ncols);
  Operand &dj    = call.words((size_t)twokay / 2 + 1);
  call.stage();
  const DevMat dM = rows ? rows->d : DevMat{}, dT = pinT ? call.view(*pinT, T) : room->d;
  const int64_t home = c / 64, wide = M->width - home;
  if (!pinT)  // the table's present content, unmasked (rows whose source row is missing keep it, and T[0] seeds the chain)
    HIPDIE(hipMemcpy2D(dT.p + home, (size_t)dT.stride * 8, T->data + home, (size_t)T->rowstride * 8, (size_t)wide * 8, (size_t)twokay, hipMemcpyHostToDevice));
  HIPDIE(hipMemcpyAsync(dj.d.p, jstar.data(), (size_t)twokay * 4, hipMemcpyHostToDevice, nullptr));
  HIPDIE(m4ri_amd_make_table_dev(dM.p, dM.stride, W.nrows, M->ncols, 0, c, k, dT.p, dT.p, dT.stride, reinterpret_cast<int32_t *>(dj.d.p), nullptr));
  if (pinT) set_newer(*pinT, true);
  else
    HIPDIE(hipMemcpy2D(T->data + (int64_t)T->rowstride + home, (size_t)T->rowstride * 8, dT.p + dT.stride + home, (size_t)dT.stride * 8, (size_t)wide * 8,
                       (size_t)(twokay - 1), hipMemcpyDeviceToHost));
  call.finish();
}

void gf2_release_staging(void) {  // called by m4ri_amd_release_workspace: the current device's arena, the parked result blocks
  g_big_cache.drop();
  const std::unique_lock<std::mutex> lk = lock_current_device();
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= GF2_MAX_DEVICES) return;
  if (g_host_stage[dev].p) {
    (void)hipDeviceSynchronize();
    (void)hipHostFree(g_host_stage[dev].p);
    g_host_stage[dev] = HostStage{};
  }
  Arena &a = g_arenas[dev];
  if (!a.base) return;
  (void)hipDeviceSynchronize();
  (void)hipFree(a.base);
  a = Arena{};
}

// Free a result the entry points allocated for C == NULL with the allocator it came from: the host
// program's mzd_free when result_init used its mzd_init (libm4ri's blocks come from its own caches,
// free() on them corrupts the heap), m4ri_amd_mzd_free otherwise.
void m4ri_amd_result_free(mzd_t *A) {
  typedef void (*free_fn)(mzd_t *);
  static free_fn host_free = dlsym(RTLD_DEFAULT, "mzd_init") ? reinterpret_cast<free_fn>(dlsym(RTLD_DEFAULT, "mzd_free")) : nullptr;
  if (host_free) host_free(A);
  else m4ri_amd_mzd_free(A);
}

// ---- part 3: residency ----------------------------------------------------------------------------
int m4ri_amd_pin(mzd_t *M) {
  if (!M || (M->flags & FLAG_WINDOW)) return -1;  // pin the owner of the block; windows into it follow
  {
    PinLock old(M);  // (the lock of the device the OLD entry is on, which need not be this thread's)
    if (old.p) {
      if (old.p->owner == M && old.p->hbase == M->data && old.p->nrows == M->nrows && old.p->ncols == M->ncols) return 0;
      // a matrix freed without unpin left this entry behind and the allocator reused its address: the
      // device copy belongs to a dead matrix -- drop it (without a download) and pin M afresh
      (void)hipFree(old.p->dbase);
      erase_pin(old.p);
    }
  }
  const std::unique_lock<std::mutex> lk = lock_current_device();
  if (M->nrows == 0 || M->ncols == 0 || !M->data) return -1;
  int dev = 0;
  HIPDIE(hipGetDevice(&dev));
  HIPDIE(m4ri_amd_init(dev));
  Pin p{};
  p.device = dev;
  p.hbase = M->data; p.words = (size_t)M->nrows * (size_t)M->rowstride; p.rowstride = M->rowstride;
  p.nrows = M->nrows; p.ncols = M->ncols; p.owner = M;
  HIPDIE(hipMalloc(reinterpret_cast<void **>(&p.dbase), p.words * 8));
  pin_upload(p);
  {
    std::lock_guard<std::mutex> pl(g_pin_mu);
    if (pin_of(M)) { (void)hipFree(p.dbase); return 0; }  // another thread pinned the same block in the meantime: keep theirs
    g_pins.push_back(p);
  }
  return 0;
}

int m4ri_amd_sync(mzd_t *M) {
  PinLock pl(M);
  if (!pl.p) return -1;
  pin_download(*pl.p);
  return 0;
}

int m4ri_amd_host_modified(mzd_t *M) {
  PinLock pl(M);
  if (!pl.p) return -1;
  pin_upload(*pl.p);
  return 0;
}

int m4ri_amd_unpin(mzd_t *M) {
  PinLock pl(M);  // the lock of the pin's device: no product that reads or writes the copy is in flight
  if (!pl.p) return -1;
  pin_download(*pl.p);
  HIPDIE(hipFree(pl.p->dbase));
  erase_pin(pl.p);
  return 0;
}

// A status query: the list's short lock only, never the device lock -- it does not wait for a product running on the pin's device
// (the flag it reads is the one the LAST completed call left; a product in flight sets it before it returns)
int m4ri_amd_is_pinned(const mzd_t *M) {
  std::lock_guard<std::mutex> pl(g_pin_mu);
  const Pin *p = pin_of(M);
  return !p ? 0 : is_newer(*p) ? 2 : 1;
}

// mp.c:277-297 / :299-324.  Several devices + a product large enough: the top Strassen-Winograd
// sub-products go over the devices (multi.hip); else the single-GPU schedule.
static mzd_t *mul_mp(mzd_t *C, mzd_t const *A, mzd_t const *B, int cutoff, bool add, const char *who) {
  if (A->ncols != B->nrows) die("%s: A ncols (%d) need to match B nrows (%d).\n", who, A->ncols, B->nrows);
  cutoff = norm_cutoff(cutoff, who);
  if (C == NULL) C = result_init(A->nrows, B->ncols);
  else if (C->nrows != A->nrows || C->ncols != B->ncols)
    die("%s: C (%d x %d) has wrong dimensions, expected (%d x %d)\n", who, C->nrows, C->ncols, A->nrows, B->ncols);
  if (add && (A->nrows == 0 || A->ncols == 0 || B->ncols == 0)) return C;
  bool pinned;
  pinned = find_pin(A) || find_pin(B) || find_pin(C);
  if (!pinned && gf2_multi_wanted(A->nrows, A->ncols, B->ncols)) {
    const int rc = m4ri_amd_mul_multi(C, A, B, add ? 1 : 0, cutoff, 0);
    if (rc) die("m4ri_amd: multi-device product failed (hipError_t %d: %s)\n", rc, hipGetErrorString((hipError_t)rc));
    return C;
  }
  return run(C, A, B, add, true, cutoff);
}
mzd_t *mzd_mul_mp(mzd_t *C, mzd_t const *A, mzd_t const *B, int cutoff) { return mul_mp(C, A, B, cutoff, false, "mzd_mul_mp"); }
mzd_t *mzd_addmul_mp(mzd_t *C, mzd_t const *A, mzd_t const *B, int cutoff) { return mul_mp(C, A, B, cutoff, true, "mzd_addmul_mp"); }

}  // extern "C"
