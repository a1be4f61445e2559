// dev_scratch.h -- how the host-side drivers hold device memory, written once: the current device's slot in a per-device table,
// the grow-only buffer such a table keeps, the turn that calls on different streams take on it, and the temporaries of one call.
// Internal to the file that includes it (an unnamed namespace, as in batch_common.h, which brings it to the batched files).
#pragma once
#include <hip/hip_runtime.h>
#include <vector>
#include "gf2_internal.h"

namespace {

// the current device's index into a table of GF2_MAX_DEVICES entries
inline int device_slot(int *slot) {
  HIPTRY(hipGetDevice(slot));
  return (*slot < 0 || *slot >= GF2_MAX_DEVICES) ? (int)hipErrorInvalidDevice : 0;
}

// A grow-only device buffer of n elements.  The one that must grow may still be in use by a call queued earlier, on whatever
// stream, and must not be freed under it: the device is synchronised first.  n counts what was really allocated.
template <typename T>
struct GrowBuf {
  T *p     = nullptr;
  size_t n = 0;
  int reserve(size_t need) {
    if (need <= n) return 0;
    if (p) { HIPTRY(hipDeviceSynchronize()); HIPTRY(hipFree(p)); }
    p = nullptr; n = 0;
    HIPTRY(hipMalloc(reinterpret_cast<void **>(&p), need * sizeof(T)));
    n = need;
    return 0;
  }
};

// The turn on a scratch that asynchronous calls on different streams share (the caller's mutex serialises only their
// enqueueing).  `last` is the end of the previous call's work; take() makes the stream wait for it, and the guard's end records
// the new one on every way out of the function, so that whatever an abandoned call did queue is waited for as well.  Declare the
// guard after the lock: it then ends under it.  A record that fails at the guard's end is not reported to the caller: a
// destructor has nobody to return it to, and the next call on another stream is then not ordered behind this one.
struct ScratchTurn {
  hipEvent_t last = nullptr;

  class Guard {
   public:
    Guard()                         = default;
    Guard(const Guard &)            = delete;
    Guard &operator=(const Guard &) = delete;
    ~Guard() {
      if (last_) (void)hipEventRecord(last_, st_);
    }
    int take(ScratchTurn &t, hipStream_t st) {
      if (!t.last) HIPTRY(hipEventCreateWithFlags(&t.last, hipEventDisableTiming));
      else HIPTRY(hipStreamWaitEvent(st, t.last, 0));
      last_ = t.last;
      st_   = st;
      return 0;
    }

   private:
    hipEvent_t last_ = nullptr;
    hipStream_t st_  = nullptr;
  };
};

// The device temporaries of one call.  Work queued on the stream may still use a buffer when the function leaves early, so
// unless done() was reached the stream is synchronised first; then the buffers are freed, in the order they were allocated.
class Scratch {
 public:
  explicit Scratch(hipStream_t st) : st_(st) {}
  Scratch(const Scratch &)            = delete;
  Scratch &operator=(const Scratch &) = delete;
  ~Scratch() {
    if (!done_) (void)hipStreamSynchronize(st_);
    for (void *p : bufs_) (void)hipFree(p);
  }
  template <typename T>
  int alloc(T **p, size_t n) {  // n elements
    HIPTRY(hipMalloc(reinterpret_cast<void **>(p), n * sizeof(T)));
    bufs_.push_back(*p);
    return 0;
  }
  int words(word **p, int64_t n) { return alloc(p, (size_t)n); }
  int done() {  // the function's successful end, after its last synchronisation
    done_ = true;
    return 0;
  }

 private:
  hipStream_t st_;
  bool done_ = false;
  std::vector<void *> bufs_;
};

}  // namespace
