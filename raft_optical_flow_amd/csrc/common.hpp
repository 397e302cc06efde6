// Shared helpers for the RAFT HIP kernels (gfx950 / CDNA4, wave64).
#pragma once

#include <hip/hip_runtime.h>

#include <atomic>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "raft_hip.h"

namespace raft {

// Last-error message, per host thread (raft_hip_last_error()).
char* last_error_buf();

inline int set_error(int code, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(last_error_buf(), 512, fmt, ap);
  va_end(ap);
  return code;
}

inline int check_launch(const char* what) {
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return set_error((int)e, "%s: launch failed: %s", what, hipGetErrorString(e));
  last_error_buf()[0] = 0;
  return 0;
}

#define RAFT_REQUIRE(cond, ...)                              \
  do {                                                       \
    if (!(cond)) return ::raft::set_error(RAFT_E_INVALID, __VA_ARGS__); \
  } while (0)

inline hipStream_t as_stream(raft_stream_t s) { return reinterpret_cast<hipStream_t>(s); }

__host__ __device__ inline int cdiv(int a, int b) { return (a + b - 1) / b; }
__host__ __device__ inline int round_up(int a, int b) { return cdiv(a, b) * b; }
__host__ __device__ inline long cdiv_l(long a, long b) { return (a + b - 1) / b; }

// Tuning knobs from the environment (DESIGN.md lists them).  How often a knob is read shows where it is read:
//   static const bool off = env_off("RAFT_X");   once, for the life of the process
//   if (env_off("RAFT_X")) ...                   on every call (a test can switch it between launches)
// env_off: the value starts with '0' (a default-on knob turned off); env_on: with '1' (an opt-in knob turned on).
inline bool env_off(const char* name) {
  const char* e = getenv(name);
  return e && e[0] == '0';
}
inline bool env_on(const char* name) {
  const char* e = getenv(name);
  return e && e[0] == '1';
}
inline long env_long(const char* name, long dflt) {
  const char* e = getenv(name);
  return e ? atol(e) : dflt;
}
inline double env_double(const char* name, double dflt) {
  const char* e = getenv(name);
  return e ? atof(e) : dflt;
}

// a [B, H, W] pixel grid the per-pixel entries take: not empty, fewer than 2^30 pixels
inline bool size_ok(int B, int H, int W) { return B > 0 && H > 0 && W > 0 && (long)B * H * W < (1L << 30); }

// work-groups of 256 threads for a grid-stride loop over n elements
inline int grid_for(long n) {
  const long g = (n + 255) / 256;
  return (int)(g > 65536 ? 65536 : g < 1 ? 1 : g);
}

// The CU count of the current device, cached per device (a process may drive several GPUs); 256, MI355X's,
// where there is none to ask.
inline long device_cus() {
  constexpr int MAXDEV = 64;
  static std::atomic<int> cache[MAXDEV];  // 0 = not queried yet
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return 256L;
  if (dev >= 0 && dev < MAXDEV) {
    const int c = cache[dev].load(std::memory_order_relaxed);
    if (c > 0) return (long)c;
  }
  int cus = 0;
  if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0) cus = 256;
  if (dev >= 0 && dev < MAXDEV) cache[dev].store(cus, std::memory_order_relaxed);
  return (long)cus;
}

// XCD-aware tile order.  The dispatcher deals work-groups round-robin over the
// 8 XCDs (work-group L -> XCD L % 8), each with its own L2; hand XCD c a
// contiguous run of the logical tile order so tiles that share operand rows
// (and neighbouring pixels under a conv's taps) hit the same L2.
__device__ inline int xcd_tile(int L, int T) {
  const int c = L & 7, slot = L >> 3;
  const int per = T >> 3, rem = T & 7;
  return c * per + (c < rem ? c : rem) + slot;
}

using f32x4 = __attribute__((ext_vector_type(4))) float;
using f32x2 = __attribute__((ext_vector_type(2))) float;
using f32x16 = __attribute__((ext_vector_type(16))) float;

}  // namespace raft
