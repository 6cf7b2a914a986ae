// sample_grad.hip — the backward of isr_sample_nearest on the device (sample_grad.hpp states the rule): the entries of
// include/isr_sample_grad.h.  No float atomics, no call synchronises, and the seams between the steps are kernel boundaries.
//
// The rays of an image are put in the order of the unique key (pixel << 32) | r, rays that belong to no pixel last (pixel =
// H W); then every run of equal pixels is one f32 chain per channel.  The keys are unique, so every correct sort gives the
// same list: nothing depends on how a sort orders equal keys.
//   n <= kLdsRays:  sort_lds_kernel, one workgroup per image: the keys in LDS, a bitonic network, the sorted (pixel, r) list
//                   to the workspace.  trainPose.py's call (16 x 1 024 rays) is one launch of 16 workgroups.
//   above:          keys_kernel writes (pixel, r) in r order; then an LSD radix sort over the pixel's digits only, 8 bits a
//                   pass, ceil(bits(H W) / 8) passes (two at 224 x 224), each pass stable: digit_count_kernel (a block of
//                   kBlockKeys keys counts its digits: integer LDS atomics, whose order cannot show in a count),
//                   digit_scan_kernel (one workgroup per image, thread d owns digit d's row of the (digit, block) table and
//                   turns it into exclusive offsets in (digit, block) order) and digit_scatter_kernel (a key's rank among
//                   its block's keys of the same digit comes from ballots inside its wave and a prefix over the waves' counts
//                   in LDS, never from an atomic's arrival order).
//   fill_kernel:    +0 to every element of dimages, 16 bytes a lane.  A fill and a scatter by segment heads, not a gather in
//                   which every pixel searches the list: the list has B n entries and the image B H W pixels, 49 times as
//                   many in trainPose.py's call, and a search per pixel would read the list that many times over.
//   sum_kernel:     one thread per (list position, channel), the channels of a position consecutive lanes as in the forward.
//                   The threads of a segment's head walk the segment in list order, acc = acc + dout, and store once.
#include "sample_grad.hpp"
#include "isr_common.hpp"

#include "../../include/isr_sample_grad.h"

#include <algorithm>

namespace {

using namespace isr::sample_grad;

constexpr int kThreads = 256;
constexpr int kSortThreads = 1024;
constexpr int kRounds = kBlockKeys / kThreads;      // keys per thread of a radix block
constexpr int kSlots = kBlockKeys / isr::kWave;     // waves' worth of keys in a radix block
static_assert(kDigits == kThreads, "a thread per digit");

struct Plan {
  uint32_t* pix[2];      // (B, n) each; [1] only above kLdsRays
  uint32_t* ray[2];
  uint32_t* table;       // (B, kDigits, nblk): a block's digit counts, then their exclusive offsets inside the image
  int nblk;
};

__global__ __launch_bounds__(kSortThreads) void sort_lds_kernel(const float* __restrict__ xys, int H, int W, int n, int npad,
                                                                uint32_t* __restrict__ pix, uint32_t* __restrict__ ray) {
  __shared__ uint64_t keys[kLdsRays];
  const size_t base = (size_t)blockIdx.x * n;
  for (int r = threadIdx.x; r < npad; r += kSortThreads)
    keys[r] = r < n ? ((uint64_t)ray_pixel(xys, base + r, H, W) << 32) | (uint32_t)r : ~0ull;      // padding sorts last
  __syncthreads();
  for (int k = 2; k <= npad; k <<= 1)
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int t = threadIdx.x; t < npad / 2; t += kSortThreads) {
        const int lo = ((t & ~(j - 1)) << 1) | (t & (j - 1)), hi = lo | j;
        const uint64_t a = keys[lo], c = keys[hi];
        if ((a > c) == ((lo & k) == 0)) {
          keys[lo] = c;
          keys[hi] = a;
        }
      }
      __syncthreads();
    }
  for (int r = threadIdx.x; r < n; r += kSortThreads) {
    pix[base + r] = (uint32_t)(keys[r] >> 32);
    ray[base + r] = (uint32_t)keys[r];
  }
}

__global__ __launch_bounds__(kThreads) void keys_kernel(const float* __restrict__ xys, int H, int W, int n, long long total,
                                                        uint32_t* __restrict__ pix, uint32_t* __restrict__ ray) {
  const long long i = (long long)blockIdx.x * kThreads + threadIdx.x;
  if (i >= total) return;
  pix[i] = ray_pixel(xys, (size_t)i, H, W);
  ray[i] = (uint32_t)(i % n);
}

__global__ __launch_bounds__(kThreads) void digit_count_kernel(const uint32_t* __restrict__ pix, int n, int nblk, int shift,
                                                               uint32_t* __restrict__ table) {
  __shared__ uint32_t count[kDigits];
  count[threadIdx.x] = 0;
  __syncthreads();
  const int b = blockIdx.x / nblk, kb = blockIdx.x % nblk;
  const uint32_t* p = pix + (size_t)b * n;
  const int end = min(n, (kb + 1) * kBlockKeys);
  for (int k = kb * kBlockKeys + threadIdx.x; k < end; k += kThreads) atomicAdd(&count[(p[k] >> shift) & (kDigits - 1)], 1u);
  __syncthreads();
  table[((size_t)b * kDigits + threadIdx.x) * nblk + kb] = count[threadIdx.x];
}

__global__ __launch_bounds__(kThreads) void digit_scan_kernel(uint32_t* __restrict__ table, int nblk) {
  __shared__ uint32_t part[kDigits];
  uint32_t* row = table + ((size_t)blockIdx.x * kDigits + threadIdx.x) * nblk;
  uint32_t sum = 0;
  for (int k = 0; k < nblk; ++k) sum += row[k];
  part[threadIdx.x] = sum;
  __syncthreads();
  for (int off = 1; off < kDigits; off <<= 1) {        // inclusive scan over the digits' totals
    const uint32_t below = threadIdx.x >= off ? part[threadIdx.x - off] : 0u;
    __syncthreads();
    part[threadIdx.x] += below;
    __syncthreads();
  }
  uint32_t run = part[threadIdx.x] - sum;
  for (int k = 0; k < nblk; ++k) {
    const uint32_t v = row[k];
    row[k] = run;
    run += v;
  }
}

__global__ __launch_bounds__(kThreads) void digit_scatter_kernel(const uint32_t* __restrict__ pix_in, const uint32_t* __restrict__ ray_in,
                                                                 int n, int nblk, int shift, const uint32_t* __restrict__ table,
                                                                 uint32_t* __restrict__ pix_out, uint32_t* __restrict__ ray_out) {
  __shared__ uint32_t count[kSlots][kDigits];          // per wave's worth of keys: its digit counts, then their offsets
  for (int i = threadIdx.x; i < kSlots * kDigits; i += kThreads) (&count[0][0])[i] = 0;
  __syncthreads();
  const int b = blockIdx.x / nblk, kb = blockIdx.x % nblk;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const size_t base = (size_t)b * n;
  uint32_t p[kRounds], rank[kRounds];
#pragma unroll
  for (int round = 0; round < kRounds; ++round) {      // every wave makes every trip: the ballots see all 64 lanes
    const int k = kb * kBlockKeys + round * kThreads + (int)threadIdx.x;
    const bool valid = k < n;
    p[round] = valid ? pix_in[base + k] : 0u;
    const uint32_t digit = (p[round] >> shift) & (kDigits - 1);
    unsigned long long same = __ballot(valid);         // lanes of this wave that hold a key with my digit
    for (int bit = 0; bit < kDigitBits; ++bit) {
      const bool one = (digit >> bit) & 1u;
      const unsigned long long ones = __ballot(one);
      same &= one ? ones : ~ones;
    }
    rank[round] = (uint32_t)__popcll(same & ((1ull << lane) - 1ull));
    if (valid && rank[round] == 0) count[round * (kThreads / isr::kWave) + wave][digit] = (uint32_t)__popcll(same);
  }
  __syncthreads();
  uint32_t run = table[((size_t)b * kDigits + threadIdx.x) * nblk + kb];      // thread d: digit d's offsets, slot after slot
  for (int s = 0; s < kSlots; ++s) {
    const uint32_t v = count[s][threadIdx.x];
    count[s][threadIdx.x] = run;
    run += v;
  }
  __syncthreads();
#pragma unroll
  for (int round = 0; round < kRounds; ++round) {
    const int k = kb * kBlockKeys + round * kThreads + (int)threadIdx.x;
    if (k >= n) continue;
    const uint32_t digit = (p[round] >> shift) & (kDigits - 1);
    const uint32_t dst = count[round * (kThreads / isr::kWave) + wave][digit] + rank[round];
    if (dst >= (uint32_t)n) continue;                  // cannot happen with the table of this call; never write outside
    pix_out[base + dst] = p[round];
    ray_out[base + dst] = ray_in[base + k];
  }
}

__global__ __launch_bounds__(kThreads) void fill_kernel(float* __restrict__ out, size_t total) {
  const size_t head = min(total, (size_t)((16 - ((uintptr_t)out & 15)) & 15) / 4);      // floats before a 16-byte boundary
  const size_t quads = (total - head) / 4, tid = (size_t)blockIdx.x * kThreads + threadIdx.x, stride = (size_t)gridDim.x * kThreads;
  float4* body = reinterpret_cast<float4*>(out + head);
  for (size_t q = tid; q < quads; q += stride) body[q] = make_float4(0.f, 0.f, 0.f, 0.f);
  if (tid < head) out[tid] = 0.f;
  for (size_t i = head + 4 * quads + tid; i < total; i += stride) out[i] = 0.f;
}

__global__ __launch_bounds__(kThreads) void sum_kernel(const float* __restrict__ dout, const uint32_t* __restrict__ pix,
                                                       const uint32_t* __restrict__ ray, int n, int C, uint32_t none,
                                                       long long total, float* __restrict__ dimages) {
  const long long t = (long long)blockIdx.x * kThreads + threadIdx.x;
  if (t >= total) return;
  const long long i = t / C;
  const int c = (int)(t % C), b = (int)(i / n), k = (int)(i % n);
  const uint32_t p = pix[i];
  if (p >= none || (k > 0 && pix[i - 1] == p)) return;      // no pixel, or not the head of its segment
  const size_t base = (size_t)b * n;
  float acc = 0.f;
  int j = k;
  do {
    const uint32_t r = ray[base + j];
    if (r < (uint32_t)n) acc = acc + dout[(base + r) * C + c];      // always, with the list of this call; never read outside
    ++j;
  } while (j < n && pix[base + j] == p);
  dimages[((size_t)b * none + p) * C + c] = acc;
}

int check(const char* who, int B, int H, int W, int C, int n, bool pointers) {
  const char* wrong = check_shape(B, H, W, C, n);
  ISR_REQUIRE(!wrong, "%s: %s (B %d, H %d, W %d, C %d, n %d)", who, wrong, B, H, W, C, n);
  ISR_REQUIRE(pointers, "%s: null pointer", who);
  return ISR_OK;
}

size_t carve(isr::Workspace& ws, int B, int n, Plan& pl) {
  const size_t N = (size_t)B * n;
  const bool radix = n > kLdsRays;
  pl.nblk = radix ? (n + kBlockKeys - 1) / kBlockKeys : 0;
  pl.pix[0] = ws.take<uint32_t>(N);
  pl.ray[0] = ws.take<uint32_t>(N);
  pl.pix[1] = radix ? ws.take<uint32_t>(N) : nullptr;
  pl.ray[1] = radix ? ws.take<uint32_t>(N) : nullptr;
  pl.table = radix ? ws.take<uint32_t>((size_t)B * kDigits * pl.nblk) : nullptr;
  return ws.off;
}

}  // namespace

extern "C" size_t isr_sample_grad_workspace_bytes(int B, int H, int W, int n) {
  if (const char* wrong = check_shape(B, H, W, 1, n)) {
    isr::set_error("isr_sample_grad_workspace_bytes: %s (B %d, H %d, W %d, n %d)", wrong, B, H, W, n);
    return 0;
  }
  isr::Workspace ws(nullptr, 0);
  Plan pl;
  return carve(ws, B, n, pl);
}

extern "C" int isr_sample_nearest_backward(const float* dout, int B, int H, int W, int C, const float* xys, int n, float* dimages,
                                           void* ws_ptr, size_t ws_bytes, isr_stream_t stream) {
  if (int rc = check("isr_sample_nearest_backward", B, H, W, C, n, dout && xys && dimages && ws_ptr)) return rc;
  isr::Workspace ws(ws_ptr, ws_bytes);
  Plan pl;
  carve(ws, B, n, pl);
  ISR_REQUIRE(ws.ok(), "isr_sample_nearest_backward: workspace %zu bytes, needs %zu", ws_bytes, ws.off);
  hipStream_t st = isr::as_stream(stream);
  const long long N = (long long)B * n;
  const size_t pixels = (size_t)B * H * W * C;
  fill_kernel<<<(unsigned)std::min<size_t>((pixels / 4 + kThreads) / kThreads, 4096), kThreads, 0, st>>>(dimages, pixels);
  ISR_CHECK_LAUNCH("fill_kernel");
  int sorted = 0;
  if (n <= kLdsRays) {
    int npad = 1;
    while (npad < n) npad <<= 1;
    sort_lds_kernel<<<B, kSortThreads, 0, st>>>(xys, H, W, n, npad, pl.pix[0], pl.ray[0]);
    ISR_CHECK_LAUNCH("sort_lds_kernel");
  } else {
    keys_kernel<<<(unsigned)((N + kThreads - 1) / kThreads), kThreads, 0, st>>>(xys, H, W, n, N, pl.pix[0], pl.ray[0]);
    ISR_CHECK_LAUNCH("keys_kernel");
    const unsigned blocks = (unsigned)((long long)B * pl.nblk);
    for (int pass = 0; pass < radix_passes(H, W); ++pass, sorted ^= 1) {
      const int shift = pass * kDigitBits;
      digit_count_kernel<<<blocks, kThreads, 0, st>>>(pl.pix[sorted], n, pl.nblk, shift, pl.table);
      ISR_CHECK_LAUNCH("digit_count_kernel");
      digit_scan_kernel<<<B, kThreads, 0, st>>>(pl.table, pl.nblk);
      ISR_CHECK_LAUNCH("digit_scan_kernel");
      digit_scatter_kernel<<<blocks, kThreads, 0, st>>>(pl.pix[sorted], pl.ray[sorted], n, pl.nblk, shift, pl.table,
                                                        pl.pix[sorted ^ 1], pl.ray[sorted ^ 1]);
      ISR_CHECK_LAUNCH("digit_scatter_kernel");
    }
  }
  const long long total = N * C;
  sum_kernel<<<(unsigned)((total + kThreads - 1) / kThreads), kThreads, 0, st>>>(dout, pl.pix[sorted], pl.ray[sorted], n, C,
                                                                               (uint32_t)H * (uint32_t)W, total, dimages);
  ISR_CHECK_LAUNCH("sum_kernel");
  return ISR_OK;
}

extern "C" int isr_sample_nearest_backward_host(const float* dout, int B, int H, int W, int C, const float* xys, int n,
                                                float* dimages) {
  if (int rc = check("isr_sample_nearest_backward_host", B, H, W, C, n, dout && xys && dimages)) return rc;
  backward_host(dout, B, H, W, C, xys, n, dimages);
  return ISR_OK;
}

extern "C" int isr_sample_grad_geometry(int which) {
  return which == 0 ? kLdsRays : which == 1 ? kBlockKeys : which == 2 ? kDigitBits : -1;
}
