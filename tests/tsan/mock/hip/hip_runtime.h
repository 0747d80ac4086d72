// Device-less stand-in for <hip/hip_runtime.h>, for the ThreadSanitizer build of the library's OWN host protocol code
// (tests/tsan/Makefile): the kq_compat*.cpp units and kq_radio.cpp compile against it unchanged, kq_host.hpp with them.  Test infrastructure only.
//
// What it models of the device: memory is host memory, and a stream is an in-order queue -- every operation that would
// go through a stream runs to completion under one mutex (mock_stream_mutex), which is the ordering the real stream
// gives the kernels and copies that the compat surface queues on its single stream.  Nothing else of HIP is here.
//
// For the tests of set-up paths (slots_harness.cpp): mock_hip().fail_in = k makes the k-th hipMalloc or
// hipStreamCreateWithFlags from then on fail, once; mock_hip() also counts the allocations and the copies.
#pragma once
#include <atomic>
#include <cstddef>
#include <cstdlib>
#include <cstring>
#include <mutex>

struct float2 {
  float x, y;
};
static inline float2 make_float2(float x, float y) { return float2{x, y}; }

typedef int hipError_t;
enum { hipSuccess = 0, hipErrorOutOfMemory = 2 };
typedef struct mock_stream_t *hipStream_t;
enum hipMemcpyKind { hipMemcpyHostToHost, hipMemcpyHostToDevice, hipMemcpyDeviceToHost, hipMemcpyDeviceToDevice, hipMemcpyDefault };
typedef struct mock_event_t *hipEvent_t;
enum { hipStreamNonBlocking = 1, hipHostMallocDefault = 0, hipEventDefault = 0, hipEventDisableTiming = 2 };

inline std::mutex &mock_stream_mutex() {
  static std::mutex m;
  return m;
}
struct mock_hip_state {
  std::atomic<int> fail_in{0}, mallocs{0}, copies{0}, copies2d{0};
};
inline mock_hip_state &mock_hip() {
  static mock_hip_state m;
  return m;
}
inline bool mock_object_fails() { return mock_hip().fail_in.load() > 0 && mock_hip().fail_in.fetch_sub(1) == 1; }
inline const char *hipGetErrorString(hipError_t e) { return e == hipSuccess ? "no error" : "mock error"; }
inline hipError_t hipGetLastError() { return hipSuccess; }
inline hipError_t hipGetDeviceCount(int *n) {
  *n = 1;
  return hipSuccess;
}
inline hipError_t hipGetDevice(int *d) {
  *d = 0;
  return hipSuccess;
}
inline hipError_t hipSetDevice(int) { return hipSuccess; }
inline hipError_t hipStreamCreateWithFlags(hipStream_t *s, unsigned) {
  if (mock_object_fails()) return hipErrorOutOfMemory;
  *s = reinterpret_cast<hipStream_t>(new char);
  return hipSuccess;
}
inline hipError_t hipStreamDestroy(hipStream_t s) {
  delete reinterpret_cast<char *>(s);
  return hipSuccess;
}
inline hipError_t hipEventCreateWithFlags(hipEvent_t *e, unsigned) {
  *e = reinterpret_cast<hipEvent_t>(new char);
  return hipSuccess;
}
inline hipError_t hipEventDestroy(hipEvent_t e) {
  delete reinterpret_cast<char *>(e);
  return hipSuccess;
}
inline hipError_t hipStreamSynchronize(hipStream_t) {
  std::lock_guard<std::mutex> lk(mock_stream_mutex());  // everything queued so far has run
  return hipSuccess;
}
inline hipError_t hipMalloc(void **p, size_t n) {
  if (mock_object_fails()) return hipErrorOutOfMemory;
  mock_hip().mallocs++;
  *p = calloc(1, n ? n : 1);
  return *p ? hipSuccess : hipErrorOutOfMemory;
}
inline hipError_t hipFree(void *p) {
  std::lock_guard<std::mutex> lk(mock_stream_mutex());  // hipFree waits for the device
  free(p);
  return hipSuccess;
}
inline hipError_t hipHostMalloc(void **p, size_t n, unsigned) {
  *p = calloc(1, n ? n : 1);
  return *p ? hipSuccess : hipErrorOutOfMemory;
}
inline hipError_t hipHostFree(void *p) {
  free(p);
  return hipSuccess;
}
inline hipError_t hipMemsetAsync(void *p, int v, size_t n, hipStream_t) {
  std::lock_guard<std::mutex> lk(mock_stream_mutex());
  memset(p, v, n);
  return hipSuccess;
}
inline hipError_t hipMemset(void *p, int v, size_t n) {
  std::lock_guard<std::mutex> lk(mock_stream_mutex());
  memset(p, v, n);
  return hipSuccess;
}
inline hipError_t hipMemcpy(void *d, const void *s, size_t n, hipMemcpyKind) {
  std::lock_guard<std::mutex> lk(mock_stream_mutex());
  memcpy(d, s, n);
  return hipSuccess;
}
inline hipError_t hipMemcpyAsync(void *d, const void *s, size_t n, hipMemcpyKind, hipStream_t) {
  std::lock_guard<std::mutex> lk(mock_stream_mutex());
  mock_hip().copies++;
  memcpy(d, s, n);
  return hipSuccess;
}
inline hipError_t hipMemcpy2DAsync(void *d, size_t dpitch, const void *s, size_t spitch, size_t width, size_t height, hipMemcpyKind,
                                   hipStream_t) {
  std::lock_guard<std::mutex> lk(mock_stream_mutex());
  mock_hip().copies2d++;
  for (size_t r = 0; r < height; r++) memcpy(static_cast<char *>(d) + r * dpitch, static_cast<const char *>(s) + r * spitch, width);
  return hipSuccess;
}
