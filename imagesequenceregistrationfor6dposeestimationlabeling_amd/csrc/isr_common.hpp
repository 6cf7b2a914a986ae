// isr_common.hpp — shared host-side plumbing for libisr_hip.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <thread>
#include <vector>

#include "../../include/isr_hip.h"

namespace isr {

// Thread-local text behind isr_last_error().
char* last_error_buf();
void set_error(const char* fmt, ...);

// Value of a tuning knob (ISR_TUNE_*): a relaxed atomic load, no environment access.
int tuning(int knob);

inline hipStream_t as_stream(isr_stream_t s) { return reinterpret_cast<hipStream_t>(s); }

// Launch check: hipGetLastError after a kernel launch, no synchronisation.
#define ISR_CHECK_LAUNCH(what)                                                  \
  do {                                                                          \
    hipError_t e__ = hipGetLastError();                                         \
    if (e__ != hipSuccess) {                                                    \
      ::isr::set_error("%s: %s", what, hipGetErrorString(e__));                 \
      return ISR_ERR_HIP;                                                       \
    }                                                                           \
  } while (0)

#define ISR_CHECK_HIP(expr)                                                     \
  do {                                                                          \
    hipError_t e__ = (expr);                                                    \
    if (e__ != hipSuccess) {                                                    \
      ::isr::set_error("%s: %s", #expr, hipGetErrorString(e__));                \
      return ISR_ERR_HIP;                                                       \
    }                                                                           \
  } while (0)

#define ISR_REQUIRE(cond, ...)                                                  \
  do {                                                                          \
    if (!(cond)) {                                                              \
      ::isr::set_error(__VA_ARGS__);                                            \
      return ISR_ERR_ARG;                                                       \
    }                                                                           \
  } while (0)

// Argument checks the packed-field entries share (csrc/field_mlp.hip, csrc/field_density.hip); who: the entry's name.
inline int check_pack_pointers(const char* who, const void* pack, const void* widths) {
  ISR_REQUIRE(pack && widths, "%s: null pointer", who);
  return ISR_OK;
}
inline int check_pack_bytes(const char* who, size_t pack_bytes, int total_words) {
  ISR_REQUIRE(pack_bytes == (size_t)total_words * 4, "%s: pack_bytes %zu, this field packs to %zu", who, pack_bytes,
              (size_t)total_words * 4);
  return ISR_OK;
}
// N rows in, N rows out: the arrays may be null only when there are none
inline int check_rows(const char* who, int N, bool pointers) {
  ISR_REQUIRE(N >= 0, "%s: N = %d", who, N);
  ISR_REQUIRE(N == 0 || pointers, "%s: null pointer", who);
  return ISR_OK;
}

// Host builds of the kernels: fn(i) for i in [0, n), over 8 threads from 8 * per_thread_min rows on
template <class F>
void parallel_rows(long n, long per_thread_min, F fn) {
  const int nthreads = n >= 8 * per_thread_min ? 8 : 1;
  if (nthreads == 1) {
    for (long i = 0; i < n; ++i) fn(i);
    return;
  }
  std::vector<std::thread> pool;
  for (int t = 0; t < nthreads; ++t) {
    const long n0 = n * t / nthreads, n1 = n * (t + 1) / nthreads;
    pool.emplace_back([=] {
      for (long i = n0; i < n1; ++i) fn(i);
    });
  }
  for (auto& th : pool) th.join();
}

inline size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

// Bump allocator over the caller's workspace; every carve is 256-byte aligned.
struct Workspace {
  char* base;
  size_t size;
  size_t off = 0;
  Workspace(void* p, size_t n) : base(static_cast<char*>(p)), size(n) {}
  template <typename T>
  T* take(size_t count) {
    off = align_up(off, 256);
    T* p = reinterpret_cast<T*>(base + off);
    off += count * sizeof(T);
    return p;
  }
  bool ok() const { return off <= size; }
};

constexpr int kWave = 64;  // gfx950 wavefront

// EPnP over the masked correspondences of B images (csrc/epnp.hip), enqueued on `stream`: mask (B, mask_words) words, K_dev
// the images' 3x3 cameras (row-major, K_stride doubles apart), ws epnp_ws_bytes(B) bytes.  status_dev (nullable): images
// with status 0 are skipped, a non-finite pose sets it to 0; pose_dev (nullable): the pose of every finite result.
// Rt_out (B, 12), err_out (B, 3), chosen_out (B): nullable.
size_t epnp_ws_bytes(int B);
int epnp_enqueue(const float* p3d, const float* p2d, const int32_t* M_dev, int M_cap, int B, const uint32_t* mask,
                 int mask_words, const double* K_dev, int K_stride, int32_t* status_dev, double* pose_dev, double* Rt_out,
                 double* err_out, int32_t* chosen_out, void* ws, hipStream_t stream);

// The order-preserving unsigned image of a float (radix select of the top-80 % cut, csrc/select_top.hip; its leading
// 11-bit digit is what K1's epilogue counts for isr_corr_argmax_digits): u(a) < u(b)  <=>  a < b for non-NaN a, b.
__host__ __device__ __forceinline__ uint32_t ordered_bits(float f) {
  union { float f; uint32_t u; } c;
  c.f = f;
  return c.u ^ ((c.u >> 31) ? 0xFFFFFFFFu : 0x80000000u);
}
constexpr int kDigitBins = 2048;    // bins of the leading digit (bits 21 .. 31 of ordered_bits)
constexpr int kDigitShift = 21;

}  // namespace isr
