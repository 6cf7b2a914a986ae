// resample.hip — the fine pass's depths on the device (resample.hpp states the arithmetic): the entries of
// include/isr_resample.h.  One fused launch per call, no workspace, no atomics, no host read.
//
// resample_kernel: a workgroup of kThreads owns R consecutive rays and keeps, per ray, in LDS
//     c    (nb + 1 words, row stride odd)   the weights, then the cdf's knots in place
//     bins (nb + 1 words, row stride odd)   the mid-points of the lengths (or the caller's bins)
//     keys (Kpad words; sorted mode only)   the lengths' bits while the mid-points are made, then the sort keys
//     sum  (1 word)                         S, between the two scans
//   1. the R rows of lengths and weights are one contiguous run of global memory each: a flat, coalesced copy into LDS;
//   2. every thread makes mid-points; lane r of wave 0 runs ray r's two serial scans (weight_sum and pdf_scan, the host's
//      code) — rows an odd number of words apart, so the R lanes of a step hit R different banks — and between the two
//      scans all threads make the quotients pdf_j, which keeps the division out of the serial chain;
//   3. the n searches and interpolations of every ray run across all threads, (ray, sample) flattened; in sorted mode
//      the samples (and with add_input the lengths, in place) become sort keys, the tail up to Kpad the largest key;
//   4. a bitonic sort of each ray's Kpad keys (the network of knn.hip), all rays at once, one barrier per stage;
//   5. the R rows of the output are again one contiguous run: a flat, coalesced store.  Every byte of `out` is written.
// R follows the shape alone: as many rays as fit kLdsBudget (32 KiB, so that five workgroups — 20 waves, 5 per SIMD —
// share a CU's 160 KiB at P = n = 256 with add_input, 4 KiB a ray), at most 64 (one wave's lanes scan); the largest
// ray (P = n = 1024 with add_input: 16 KiB) still leaves 2.  A ray's row depends on its own inputs and ray id only, so
// neither R nor the grid shows in the result.
#include "resample.hpp"
#include "isr_common.hpp"

#include "../../include/isr_resample.h"

#include <vector>

namespace {

using namespace isr::resample;

constexpr int kThreads = 256;
constexpr int kLdsBudget = 32 * 1024;
constexpr int kMaxRaysPerGroup = 64;

struct Plan {
  int R;          // rays per workgroup
  int P_in;       // floats per input row of `a` (lengths: P; bins: nb + 1)
  int W_in;       // floats per input row of `w` (ray_weights: P; weights: nb)
  int w_off;      // w[k] goes to c[k + w_off] when 1 <= k + w_off <= nb
  int stride;     // words between rows of c and of bins: nb + 1 made odd
  int sorted;     // 0: isr_sample_pdf, 1: isr_resample_lengths
  int add_input;
  int P_out;      // floats per output row
  int Kpad;       // keys per ray: P_out padded to a power of two, and at least P_in (the lengths are staged there)
  int ksort;      // the power of two that is sorted
  int half_log2;  // log2(ksort / 2)
};

Plan make_plan(const Spec& sp, int sorted, int add_input) {
  Plan pl{};
  pl.sorted = sorted;
  pl.add_input = sorted && add_input;
  pl.P_in = sorted ? sp.nb + 2 : sp.nb + 1;
  pl.W_in = sorted ? sp.nb + 2 : sp.nb;
  pl.w_off = sorted ? 0 : 1;
  pl.stride = (sp.nb + 1) | 1;
  pl.P_out = sp.n + (pl.add_input ? pl.P_in : 0);
  pl.ksort = sorted ? isr::pad_pow2(pl.P_out) : 0;
  pl.Kpad = sorted ? (pl.ksort > pl.P_in ? pl.ksort : pl.P_in) : 0;
  while ((2 << pl.half_log2) < pl.ksort) ++pl.half_log2;
  const int per_ray = 4 * (2 * pl.stride + pl.Kpad + 1);
  int R = kLdsBudget / per_ray;
  pl.R = R < 1 ? 1 : (R > kMaxRaysPerGroup ? kMaxRaysPerGroup : R);
  return pl;
}

size_t lds_bytes(const Plan& pl) { return (size_t)pl.R * 4 * (2 * pl.stride + pl.Kpad + 1); }

__global__ __launch_bounds__(kThreads) void resample_kernel(Spec sp, Plan pl, const float* __restrict__ a,
                                                            const float* __restrict__ w, long long N,
                                                            const int32_t* __restrict__ ray_ids, float* __restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
  float* c = reinterpret_cast<float*>(lds);
  float* bins = c + (size_t)pl.R * pl.stride;
  uint32_t* keys = reinterpret_cast<uint32_t*>(bins + (size_t)pl.R * pl.stride);
  const int tid = threadIdx.x, nb = sp.nb;
  const long long ray0 = (long long)blockIdx.x * pl.R;
  const int live = (int)(N - ray0 < pl.R ? N - ray0 : pl.R);        // rays of this workgroup, >= 1

  // ---- 1. rows in: `a` to the keys (sorted: the lengths' bits) or straight to bins, `w` to c[1 .. nb]
  const float* a0 = a + (size_t)ray0 * pl.P_in;
  for (int i = tid; i < live * pl.P_in; i += kThreads) {
    const int r = i / pl.P_in, k = i - r * pl.P_in;
    if (pl.sorted)
      keys[r * pl.Kpad + k] = float_bits(a0[i]);
    else
      bins[r * pl.stride + k] = a0[i];
  }
  const float* w0 = w + (size_t)ray0 * pl.W_in;
  for (int i = tid; i < live * pl.W_in; i += kThreads) {
    const int r = i / pl.W_in, k = i - r * pl.W_in + pl.w_off;
    if (k >= 1 && k <= nb) c[r * pl.stride + k] = w0[i];
  }
  __syncthreads();

  // ---- 2. mid-points across the threads, then the two serial scans: one lane per ray
  if (pl.sorted)
    for (int i = tid; i < live * (nb + 1); i += kThreads) {
      const int r = i / (nb + 1), j = i - r * (nb + 1);
      const uint32_t* l = keys + r * pl.Kpad + j;
      bins[r * pl.stride + j] = mid_point(isr::bits_float(l[0]), isr::bits_float(l[1]));
    }
  float* sums = reinterpret_cast<float*>(keys + (size_t)pl.R * pl.Kpad);      // R words behind the keys
  if (tid < live) sums[tid] = weight_sum(c + tid * pl.stride, nb, sp.eps);
  __syncthreads();
  for (int i = tid; i < live * nb; i += kThreads) {
    const int r = i / nb, j = i - r * nb;
    float* slot = c + r * pl.stride + j + 1;
    *slot = pdf_value(*slot, sp.eps, sums[r]);
  }
  __syncthreads();
  if (tid < live) pdf_scan(c + tid * pl.stride, nb);
  __syncthreads();

  // ---- 3. the samples, (ray, sample) flattened over the threads
  const int base = pl.add_input ? pl.P_in : 0;
  if (pl.add_input)
    for (int i = tid; i < live * pl.P_in; i += kThreads) {
      const int r = i / pl.P_in, k = i - r * pl.P_in;
      uint32_t* slot = keys + r * pl.Kpad + k;
      *slot = sort_key(isr::bits_float(*slot));
    }
  float* o0 = out + (size_t)ray0 * pl.P_out;
  for (int i = tid; i < live * sp.n; i += kThreads) {
    const int r = i / sp.n, s = i - r * sp.n;
    const long long ray = ray0 + r;
    const uint32_t id = ray_ids ? (uint32_t)ray_ids[ray] : (uint32_t)ray;
    const float z = sample_at(bins + r * pl.stride, c + r * pl.stride, nb, sp.eps, unit_at(sp, id, s));
    if (pl.sorted)
      keys[r * pl.Kpad + base + s] = sort_key(z);
    else
      o0[i] = z;                                     // P_out = n: the flat index is the output's
  }
  if (!pl.sorted) return;                            // uniform: no barrier is skipped by part of a workgroup
  const int tail = pl.ksort - pl.P_out;
  for (int i = tid; i < live * tail; i += kThreads) {
    const int r = i / tail, k = i - r * tail;
    keys[r * pl.Kpad + pl.P_out + k] = kNanKey;
  }
  __syncthreads();

  // ---- 4. bitonic sort of every ray's ksort keys, ascending: thread i takes the pair (lower index, lower ^ j)
  const int half = pl.ksort >> 1;
  for (int k = 2; k <= pl.ksort; k <<= 1)
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int i = tid; i < live * half; i += kThreads) {
        const int r = i >> pl.half_log2, q = i & (half - 1);
        const int lo = ((q & ~(j - 1)) << 1) | (q & (j - 1)), hi = lo | j;
        uint32_t* row = keys + r * pl.Kpad;
        const uint32_t x = row[lo], y = row[hi];
        if ((x > y) == ((lo & k) == 0)) {
          row[lo] = y;
          row[hi] = x;
        }
      }
      __syncthreads();
    }

  // ---- 5. rows out
  for (int i = tid; i < live * pl.P_out; i += kThreads) {
    const int r = i / pl.P_out, k = i - r * pl.P_out;
    o0[i] = key_value(keys[r * pl.Kpad + k]);
  }
}

int check_call(const char* who, long long N, int nb, int n, int det, float eps, uint64_t seed, const void* a, const void* w,
               const void* out, Spec& sp) {
  const char* wrong = make_spec(N, nb, n, det, eps, seed, sp);
  ISR_REQUIRE(!wrong, "%s: %s (N %lld, P %d, n %d, eps %g)", who, wrong, N, nb + 2, n, (double)eps);
  ISR_REQUIRE(N == 0 || (a && w && out), "%s: null pointer", who);
  return ISR_OK;
}

int launch(const Spec& sp, const Plan& pl, const float* a, const float* w, long long N, const int32_t* ray_ids, float* out,
           isr_stream_t stream) {
  if (N == 0) return ISR_OK;
  const unsigned blocks = (unsigned)((N + pl.R - 1) / pl.R);
  resample_kernel<<<blocks, kThreads, lds_bytes(pl), isr::as_stream(stream)>>>(sp, pl, a, w, N, ray_ids, out);
  ISR_CHECK_LAUNCH("resample_kernel");
  return ISR_OK;
}

}  // namespace

extern "C" int isr_sample_pdf(const float* bins, const float* weights, int64_t N, int nb, int n, int det, float eps,
                              uint64_t seed, const int32_t* ray_ids, float* samples, isr_stream_t stream) {
  Spec sp;
  if (int rc = check_call("isr_sample_pdf", N, nb, n, det, eps, seed, bins, weights, samples, sp)) return rc;
  return launch(sp, make_plan(sp, 0, 0), bins, weights, N, ray_ids, samples, stream);
}

extern "C" int isr_sample_pdf_host(const float* bins, const float* weights, int64_t N, int nb, int n, int det, float eps,
                                   uint64_t seed, const int32_t* ray_ids, float* samples) {
  Spec sp;
  if (int rc = check_call("isr_sample_pdf_host", N, nb, n, det, eps, seed, bins, weights, samples, sp)) return rc;
  isr::parallel_rows((long)N, 64, [=](long i) {
    std::vector<float> cdf((size_t)nb + 1);
    sample_pdf_row(sp, bins + (size_t)i * (nb + 1), weights + (size_t)i * nb, ray_ids ? (uint32_t)ray_ids[i] : (uint32_t)i,
                   cdf.data(), samples + (size_t)i * n);
  });
  return ISR_OK;
}

extern "C" int isr_resample_lengths(const float* lengths, const float* ray_weights, int64_t N, int P, int n, int add_input,
                                    int det, float eps, uint64_t seed, const int32_t* ray_ids, float* out, isr_stream_t stream) {
  Spec sp;
  if (int rc = check_call("isr_resample_lengths", N, P - 2, n, det, eps, seed, lengths, ray_weights, out, sp)) return rc;
  return launch(sp, make_plan(sp, 1, add_input), lengths, ray_weights, N, ray_ids, out, stream);
}

extern "C" int isr_resample_lengths_host(const float* lengths, const float* ray_weights, int64_t N, int P, int n, int add_input,
                                         int det, float eps, uint64_t seed, const int32_t* ray_ids, float* out) {
  Spec sp;
  if (int rc = check_call("isr_resample_lengths_host", N, P - 2, n, det, eps, seed, lengths, ray_weights, out, sp)) return rc;
  const int P_out = n + (add_input ? P : 0);
  isr::parallel_rows((long)N, 64, [=](long i) {
    std::vector<float> scratch(2 * (size_t)(P - 1));
    std::vector<uint32_t> keys((size_t)P_out);
    resample_row(sp, lengths + (size_t)i * P, ray_weights + (size_t)i * P, add_input, ray_ids ? (uint32_t)ray_ids[i] : (uint32_t)i,
                 scratch.data(), scratch.data() + (P - 1), keys.data(), out + (size_t)i * P_out);
  });
  return ISR_OK;
}

/* the rays a workgroup owns for this shape (tests cover its boundaries; tools report it) */
extern "C" int isr_resample_rays_per_group(int P, int n, int add_input, int sorted) {
  Spec sp;
  const int nb = sorted ? P - 2 : P - 1;      // unsorted: P counts the knots of `bins`
  if (make_spec(0, nb, n, 1, 1.f, 0, sp)) {
    isr::set_error("isr_resample_rays_per_group: P = %d, n = %d", P, n);
    return 0;
  }
  return make_plan(sp, sorted, add_input).R;
}
