// kq_host.hpp -- the host half that the satellite banks share (kq_afsk, kq_decim, kq_mod, kq_spec, kq_wfm): error
// reporting, the handle's stream and the device memory the handle owns.  Host only; a handle's struct derives from
// kq::HostSide.  Every member function wants the handle's device current (the entry point's kq::DeviceScope).
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
  hipStream_t stream = nullptr;
  bool own_stream = false;
  std::vector<void *> held;  // every device allocation the handle holds, in the order it was made

  // the caller's stream (kq_*_config::stream), or a non-blocking one of the handle's own
  int open_stream(void *given) {
    if (given) {
      stream = (hipStream_t)given;
      return 0;
    }
    KQ_TRY(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
    own_stream = true;
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

  // at destroy: waits for the stream, frees what is still held, destroys the stream if it is the handle's own
  void close() {
    if (stream) (void)hipStreamSynchronize(stream);
    for (void *q : held) (void)hipFree(q);
    held.clear();
    if (own_stream) (void)hipStreamDestroy(stream);
    stream = nullptr;
    own_stream = false;
  }
};

}  // namespace kq
