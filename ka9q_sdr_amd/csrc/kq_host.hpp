// kq_host.hpp -- the host half that every handle shares (kq_bank; the satellite banks kq_afsk, kq_decim, kq_mod, kq_spec,
// kq_mon and the slot banks; the compat surface's context, masters, slaves and FFTW plans, kq_compat.hpp): error
// reporting, the handle's streams, and whatever the handle owns on the device or for it -- device memory, pinned host
// memory, events.  Each is named once, where it is made; close() lets go of all of it.  Host only; a handle's struct
// derives from kq::HostSide.  Every member function wants the handle's device current (the entry point's
// kq::DeviceScope).  kq::lazy_device() is for the handles that touch no device before their first set.  What the slot
// banks (kq_wfm, kq_rds, kq_fsk, kq_pag, kq_tone, kq_cw, kq_rtty, kq_rsmp) share beyond this is kq_slots.hpp, on top of
// this file; it lists what each kind of them takes.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <vector>

void kq_internal_set_error(const char *fmt, ...);  // kq_bank.cpp: the text kq_last_error() returns

#define KQ_TRY(expr)                                                                                  \
  do {                                                                                                \
    hipError_t e_ = (expr);                                                                           \
    if (e_ != hipSuccess) {                                                                           \
      kq_internal_set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
      return -1;                                                                                      \
    }                                                                                                 \
  } while (0)

namespace kq {

struct HostSide {
  hipStream_t stream = nullptr;      // the handle's main stream: the caller's, or one of `streams`
  std::vector<void *> held;          // every device allocation the handle holds, in the order it was made
  std::vector<void *> pinned;        // pinned host memory
  std::vector<hipEvent_t> events;
  std::vector<hipStream_t> streams;  // the streams the handle made itself (a stream the caller handed in is never here)

  // the caller's stream (kq_*_config::stream), or a non-blocking one of the handle's own
  int open_stream(void *given) {
    if (given) {
      stream = (hipStream_t)given;
      return 0;
    }
    return new_stream(&stream);
  }

  // a further non-blocking stream of the handle's own
  int new_stream(hipStream_t *s) {
    KQ_TRY(hipStreamCreateWithFlags(s, hipStreamNonBlocking));
    streams.push_back(*s);
    return 0;
  }

  // an event, destroyed by close(); flags as for hipEventCreateWithFlags (hipEventDefault: one that can be timed)
  int new_event(hipEvent_t *e, unsigned flags) {
    KQ_TRY(hipEventCreateWithFlags(e, flags));
    events.push_back(*e);
    return 0;
  }

  // `count` elements of pinned host memory, freed by close(); flags as for hipHostMalloc.  Not cleared
  template <class T>
  int alloc_pinned(T **p, size_t count, unsigned flags = hipHostMallocDefault) {
    KQ_TRY(hipHostMalloc((void **)p, count * sizeof(T), flags));
    pinned.push_back(*p);
    return 0;
  }

  // `count` elements of device memory, freed by release() or close(); zero: cleared on the handle's stream (not waited for)
  template <class T>
  int alloc(T **p, size_t count, bool zero = false) {
    KQ_TRY(hipMalloc((void **)p, count * sizeof(T)));
    held.push_back(*p);
    if (zero) KQ_TRY(hipMemsetAsync(*p, 0, count * sizeof(T), stream));
    return 0;
  }

  // memory that goes away before the handle does; the pointers are left null.  Work queued on the stream may still read it:
  // the caller waits first
  template <class... T>
  void release(T **...p) {
    auto one = [this](void *q) {
      auto it = std::find(held.begin(), held.end(), q);
      if (!q || it == held.end()) return;
      held.erase(it);
      (void)hipFree(q);
    };
    (one(*p), ...);
    ((*p = nullptr), ...);
  }

  // a buffer that only grows (staging of host-memory calls): at least `need` elements, contents not kept.  Waits for the
  // stream before the old buffer goes
  template <class T>
  int grow(T **buf, size_t *capacity, size_t need) {
    if (need <= *capacity) return 0;
    KQ_TRY(hipStreamSynchronize(stream));
    release(buf);
    *capacity = 0;
    if (alloc(buf, need)) return -1;
    *capacity = need;
    return 0;
  }

  // at destroy: waits for every stream before anything goes (a copy in flight on one may read or write a buffer that work
  // on another made), then frees device memory, pinned memory, events and, last, the streams of the handle's own
  void close() {
    if (stream) (void)hipStreamSynchronize(stream);
    for (hipStream_t s : streams) (void)hipStreamSynchronize(s);
    for (void *q : held) (void)hipFree(q);
    for (void *q : pinned) (void)hipHostFree(q);
    for (hipEvent_t e : events) (void)hipEventDestroy(e);
    for (hipStream_t s : streams) (void)hipStreamDestroy(s);
    held.clear();
    pinned.clear();
    events.clear();
    streams.clear();
    stream = nullptr;
  }
};

// The device half of a handle that has none until it is first needed (so that create and the argument checks touch no
// device): the handle keeps `bool dev_ready` and groups every device pointer it holds, with whatever else names device
// memory, in one member `d` whose default initialisers are the state without a device.  make(b) opens the stream and
// allocates; when it fails half way everything made so far goes and `d` is as it was before, so the next call starts
// over and a handle that is not ready holds nothing.
template <class Handle, class Make>
int lazy_device(Handle *b, Make make) {
  if (b->dev_ready) return 0;
  if (make(b) == 0) {
    b->dev_ready = true;
    return 0;
  }
  b->close();
  b->d = {};
  return -1;
}

}  // namespace kq
