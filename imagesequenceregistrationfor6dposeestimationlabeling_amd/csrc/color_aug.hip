// color_aug.hip — the colour augmentation pass on the device (include/isr_color_aug.h states every rule, csrc/color_aug.hpp
// the arithmetic).  A pass is a short chain of launches over 16 images at once; a launch is skipped when no image's program
// asks for its stage.  The image's bytes sit in a per-image u8 workspace (150 KB at 224 x 224: L2-resident) between launches:
//   bytes    per pixel: to u8, then the jitter steps that come before the contrast step
//   gray     one workgroup per image: the exact integer sum of gray, for the contrast's mean
//   jitter   per pixel: the contrast step and the steps after it, then RandomBrightnessContrast
//   blur     per pixel: [1 2 1] x [1 2 1] from one buffer into the other
//   noise    one workgroup per image: the exact sums of li and li^2, then one lane builds the Poisson cdf (a chain)
//   iso      per pixel: the Poisson and Irwin-Hall draws and the HLS round trip
//   tables   one workgroup per (tile, image): the histogram in LDS, clipped, spread, scanned into the look-up table
//   finish   per pixel: the four look-ups of CLAHE, back to f32, select / under, the border blanking, normalize
// Per-pixel launches use a workgroup per 256 pixels, so an image spreads over the chip; what one launch writes the next one
// reads, and nothing else orders them: no hand-off between workgroups, no fence.  Histogram counts are integer LDS atomics;
// nothing else is atomic, and the sums are exact integers.  One workgroup per image for the whole pass was measured first:
// 0.81 ms for a 16 x 224 x 224 pass with every gate on, bound by the f64 work of 16 compute units (profiles/color_aug.json
// keeps the figure); this chain spreads the same arithmetic over the chip.
// The programs are made on the host and travel as kernel arguments: no copy, no synchronisation.
#include "block_prims.hpp"
#include "isr_common.hpp"

#include "color_aug.hpp"

namespace {

using namespace isr::color_aug;

constexpr int kPixThreads = 256;               // per-pixel launches: a pixel per thread
constexpr int kSumThreads = 1024;              // per-image sums
constexpr int kSumWaves = kSumThreads / isr::kWave;
constexpr int kMaxLaunches = 8;                // per 16 images, every stage asked for
static_assert(kPixThreads == kBins, "the table kernel gives every bin a thread");

struct Images {
  const float* in;
  const float* select;
  const float* under;
  const float* border_mask;
  float* out;
  uint8_t* ws;
  size_t ws_stride;      // bytes per image
  size_t buf_bytes;      // bytes per u8 buffer
};

struct Work {            // image j's part of the workspace
  uint8_t *a, *b, *luts;
  double* cdf;
  uint64_t* gray_sum;
};

__device__ __forceinline__ Work work_of(const Images& im, int j) {
  uint8_t* base = im.ws + (size_t)j * im.ws_stride;
  Work w;
  w.a = base;
  w.b = base + im.buf_bytes;
  w.luts = base + 2 * im.buf_bytes;
  w.cdf = (double*)(w.luts + kLutBytes);
  w.gray_sum = (uint64_t*)(w.luts + kLutBytes + kCdfBytes);
  return w;
}

// the buffer that holds the image after the blur stage
__device__ __forceinline__ uint8_t* current(const Work& w, const Program& pr) { return pr.ksize == 3 ? w.b : w.a; }

// the sums of a and b over a kSumThreads workgroup, to every thread
__device__ __forceinline__ void block_sum2(uint64_t& a, uint64_t& b, uint64_t (*red)[kSumWaves]) {
  a = isr::wave_reduce((unsigned long long)a, isr::Plus{});
  b = isr::wave_reduce((unsigned long long)b, isr::Plus{});
  if ((threadIdx.x & 63) == 0) {
    red[0][threadIdx.x >> 6] = a;
    red[1][threadIdx.x >> 6] = b;
  }
  __syncthreads();
  a = 0;
  b = 0;
#pragma unroll
  for (int w = 0; w < kSumWaves; ++w) {
    a += red[0][w];
    b += red[1][w];
  }
  __syncthreads();
}

__global__ __launch_bounds__(kPixThreads) void color_bytes_kernel(Images im, Frame f, Batch bt) {
  const int j = blockIdx.y;
  const Program& pr = bt.p[j];
  const size_t npix = (size_t)f.H * f.W, q = (size_t)blockIdx.x * kPixThreads + threadIdx.x;
  if (!pr.pass || q >= npix) return;
  const float* __restrict__ in = im.in + ((size_t)j * npix + q) * 3;
  uint8_t p[3] = {to_u8(in[0]), to_u8(in[1]), to_u8(in[2])};
  if (pr.jitter)
    for (int st = 0; st < 4 && pr.order[st] != 1; ++st) jitter_pixel(p, pr, pr.order[st], 0.0);
  uint8_t* a = work_of(im, j).a + 3 * q;
  a[0] = p[0];
  a[1] = p[1];
  a[2] = p[2];
}

__global__ __launch_bounds__(kSumThreads) void color_gray_kernel(Images im, Frame f, Batch bt) {
  __shared__ uint64_t red[2][kSumWaves];
  const int j = blockIdx.x;
  const Program& pr = bt.p[j];
  if (!pr.pass || !pr.jitter) return;
  const size_t npix = (size_t)f.H * f.W;
  const Work w = work_of(im, j);
  uint64_t sum = 0, unused = 0;
  for (size_t q = threadIdx.x; q < npix; q += kSumThreads) sum += (uint64_t)gray8(w.a + 3 * q);
  block_sum2(sum, unused, red);
  if (threadIdx.x == 0) *w.gray_sum = sum;
}

__global__ __launch_bounds__(kPixThreads) void color_jitter_kernel(Images im, Frame f, Batch bt) {
  const int j = blockIdx.y;
  const Program& pr = bt.p[j];
  const size_t npix = (size_t)f.H * f.W, q = (size_t)blockIdx.x * kPixThreads + threadIdx.x;
  if (!pr.pass || !(pr.jitter || pr.rbc) || q >= npix) return;
  const Work w = work_of(im, j);
  uint8_t* a = w.a + 3 * q;
  uint8_t p[3] = {a[0], a[1], a[2]};
  if (pr.jitter) {
    const double m = mean_gray(*w.gray_sum, npix);
    for (int st = contrast_step(pr); st < 4; ++st) jitter_pixel(p, pr, pr.order[st], m);
  }
  if (pr.rbc)
    for (int c = 0; c < 3; ++c) p[c] = rbc8(p[c], pr.alpha, pr.beta);
  a[0] = p[0];
  a[1] = p[1];
  a[2] = p[2];
}

__global__ __launch_bounds__(kPixThreads) void color_blur_kernel(Images im, Frame f, Batch bt) {
  const int j = blockIdx.y;
  const Program& pr = bt.p[j];
  const size_t npix = (size_t)f.H * f.W, q = (size_t)blockIdx.x * kPixThreads + threadIdx.x;
  if (!pr.pass || pr.ksize != 3 || q >= npix) return;
  const Work w = work_of(im, j);
  const int y = (int)(q / f.W), x = (int)(q - (size_t)y * f.W);
  for (int c = 0; c < 3; ++c) w.b[3 * q + c] = blur_at(w.a, f, x, y, c);
}

__global__ __launch_bounds__(kSumThreads) void color_noise_kernel(Images im, Frame f, Batch bt) {
  __shared__ uint64_t red[2][kSumWaves];
  const int j = blockIdx.x;
  const Program& pr = bt.p[j];
  if (!pr.pass || !pr.iso) return;
  const size_t npix = (size_t)f.H * f.W;
  const Work w = work_of(im, j);
  const uint8_t* cur = current(w, pr);
  uint64_t s1 = 0, s2 = 0;
  for (size_t q = threadIdx.x; q < npix; q += kSumThreads) {
    const uint64_t li = (uint64_t)luma_sum(cur + 3 * q);
    s1 += li;
    s2 += li * li;
  }
  block_sum2(s1, s2, red);
  if (threadIdx.x == 0) poisson_cdf(iso_lambda(pr, sigma_l(s1, s2, npix)), w.cdf);      // a chain: one lane
}

__global__ __launch_bounds__(kPixThreads) void color_iso_kernel(Images im, Frame f, Batch bt) {
  __shared__ double cdf[kBins];
  const int j = blockIdx.y;
  const Program& pr = bt.p[j];
  if (!pr.pass || !pr.iso) return;
  const Work w = work_of(im, j);
  cdf[threadIdx.x] = w.cdf[threadIdx.x];
  __syncthreads();
  const size_t npix = (size_t)f.H * f.W, q = (size_t)blockIdx.x * kPixThreads + threadIdx.x;
  if (q >= npix) return;
  uint8_t* a = current(w, pr) + 3 * q;
  uint8_t p[3] = {a[0], a[1], a[2]};
  iso_pixel(p, (uint32_t)q, cdf, sigma_hue(pr), (uint32_t)pr.noise_key, (uint32_t)(pr.noise_key >> 32));
  a[0] = p[0];
  a[1] = p[1];
  a[2] = p[2];
}

// one workgroup per (tile, image), a thread per bin: clahe_lut's table, its sums as a block sum and a scan
__global__ __launch_bounds__(kPixThreads) void color_tables_kernel(Images im, Frame f, Batch bt) {
  __shared__ uint32_t hist[kBins];
  __shared__ uint32_t scan[2][kBins];
  const int tile = blockIdx.x, j = blockIdx.y, i = threadIdx.x;
  const Program& pr = bt.p[j];
  if (!pr.pass || !pr.clahe) return;
  const Work w = work_of(im, j);
  const uint8_t* cur = current(w, pr);
  const int th = f.H / kGrid, tw = f.W / kGrid, area = th * tw;
  const int y0 = (tile / kGrid) * th, x0 = (tile % kGrid) * tw;
  hist[i] = 0u;
  __syncthreads();
  for (int k = i; k < area; k += kPixThreads) {
    const int y = y0 + k / tw, x = x0 + k % tw;
    atomicAdd(&hist[gray8(cur + ((size_t)y * f.W + x) * 3)], 1u);      // counts only: the order cannot matter
  }
  __syncthreads();
  const uint32_t clip = (uint32_t)clahe_clip(pr.clip_limit, area), h = hist[i];
  scan[0][i] = h > clip ? h - clip : 0u;
  __syncthreads();
  int src = 0;
  for (int o = 1; o < kBins; o <<= 1) {          // inclusive scan: the last entry is the excess
    scan[src ^ 1][i] = scan[src][i] + (i >= o ? scan[src][i - o] : 0u);
    src ^= 1;
    __syncthreads();
  }
  const uint32_t excess = scan[src][kBins - 1];
  __syncthreads();
  scan[0][i] = clahe_bin(h, clip, excess, (uint32_t)i);
  __syncthreads();
  src = 0;
  for (int o = 1; o < kBins; o <<= 1) {
    scan[src ^ 1][i] = scan[src][i] + (i >= o ? scan[src][i - o] : 0u);
    src ^= 1;
    __syncthreads();
  }
  w.luts[tile * kBins + i] = clahe_lut_value(scan[src][i], area);
}

__global__ __launch_bounds__(kPixThreads) void color_finish_kernel(Images im, Frame f, Batch bt) {
  const int j = blockIdx.y;
  const Program& pr = bt.p[j];
  const size_t npix = (size_t)f.H * f.W, q = (size_t)blockIdx.x * kPixThreads + threadIdx.x;
  if (q >= npix) return;
  const int y = (int)(q / f.W), x = (int)(q - (size_t)y * f.W);
  float v3[3], o3[3];
  if (pr.pass) {
    const Work w = work_of(im, j);
    const uint8_t* a = current(w, pr) + 3 * q;
    uint8_t p[3] = {a[0], a[1], a[2]};
    if (pr.clahe) clahe_pixel(p, f, x, y, w.luts);
    for (int c = 0; c < 3; ++c) v3[c] = from_u8(p[c]);
  } else {
    const float* in = im.in + ((size_t)j * npix + q) * 3;
    for (int c = 0; c < 3; ++c) v3[c] = in[c];
  }
  finish_pixel(v3, im.select ? im.select + j * npix : nullptr, im.under ? im.under + j * npix * 3 : nullptr,
               im.border_mask ? im.border_mask + j * npix : nullptr, f, bt.kh[j], bt.kw[j], bt, x, y, o3);
  float* out = im.out + ((size_t)j * npix + q) * 3;
  out[0] = o3[0];
  out[1] = o3[1];
  out[2] = o3[2];
}

bool overlaps(const void* a, size_t na, const void* b, size_t nb) {
  if (!a || !b) return false;
  const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
  return a0 < b0 + nb && b0 < a0 + na;
}

// the checks both builds share; bt: the batches, made before anything runs
int check_call(const char* who, const float* in, int B, int H, int W, const Program* programs, const float* select,
               const float* under, const int32_t* border, const float* border_mask, const float* mean3, const float* std3,
               const float* out, const void* ws, size_t ws_bytes, std::vector<Batch>& batches) {
  ISR_REQUIRE(in && programs && out, "%s: null pointer", who);
  ISR_REQUIRE(shape_ok(B, H, W), "%s: B=%d H=%d W=%d (B >= 1; H, W multiples of 8, >= 8; H W <= 2^20)", who, B, H, W);
  ISR_REQUIRE(!under || select, "%s: under needs select", who);
  ISR_REQUIRE(!border == !border_mask, "%s: border and border_mask go together", who);
  ISR_REQUIRE(!mean3 == !std3, "%s: mean3 and std3 go together", who);
  const size_t npix = (size_t)B * H * W, n_rgb = npix * 3 * sizeof(float), n_one = npix * sizeof(float);
  const void* ins[4] = {in, select, under, border_mask};
  const size_t sizes[4] = {n_rgb, n_one, n_rgb, n_one};
  for (int i = 0; i < 4; ++i) {
    ISR_REQUIRE(!overlaps(out, n_rgb, ins[i], sizes[i]), "%s: out overlaps an input", who);
    ISR_REQUIRE(!overlaps(ws, ws_bytes, ins[i], sizes[i]), "%s: the workspace overlaps an input", who);
  }
  ISR_REQUIRE(!overlaps(ws, ws_bytes, out, n_rgb), "%s: the workspace overlaps out", who);
  batches.resize((B + kMaxBatch - 1) / kMaxBatch);
  for (int b0 = 0; b0 < B; b0 += kMaxBatch) {
    const int nb = B - b0 < kMaxBatch ? B - b0 : kMaxBatch;
    const char* bad = make_batch(b0, nb, programs, border, mean3, std3, batches[b0 / kMaxBatch]);
    ISR_REQUIRE(!bad, "%s: %s (images %d..%d)", who, bad, b0, b0 + nb - 1);
  }
  return ISR_OK;
}

}  // namespace

extern "C" size_t isr_color_aug_workspace_bytes(int B, int H, int W) {
  return shape_ok(B, H, W) ? (size_t)B * image_ws_bytes(H, W) : 0;
}

extern "C" int isr_augment_color(const float* in, int B, int H, int W, const isr_color_program* programs_host, const float* select,
                                 const float* under, const int32_t* border_host, const float* border_mask, const float* mean3,
                                 const float* std3, float* out, void* ws, size_t workspace_bytes, isr_stream_t stream) {
  const char* who = "isr_augment_color";
  std::vector<Batch> batches;
  ISR_REQUIRE(ws && ((uintptr_t)ws & 7) == 0, "%s: the workspace is null or not 8-byte aligned", who);
  // every batch is checked before the first launch: a refused call writes nothing
  if (int rc = check_call(who, in, B, H, W, programs_host, select, under, border_host, border_mask, mean3, std3, out, ws,
                          workspace_bytes, batches))
    return rc;
  ISR_REQUIRE(workspace_bytes >= isr_color_aug_workspace_bytes(B, H, W), "%s: workspace of %zu bytes, %zu needed", who,
              workspace_bytes, isr_color_aug_workspace_bytes(B, H, W));
  const Frame f{H, W};
  const size_t npix = (size_t)H * W, stride = image_ws_bytes(H, W);
  const unsigned gx = (unsigned)((npix + kPixThreads - 1) / kPixThreads);
  hipStream_t st = isr::as_stream(stream);
  for (int b0 = 0; b0 < B; b0 += kMaxBatch) {
    const int nb = B - b0 < kMaxBatch ? B - b0 : kMaxBatch;
    const Batch& bt = batches[b0 / kMaxBatch];
    const Images im{in + b0 * npix * 3,
                    select ? select + b0 * npix : nullptr,
                    under ? under + b0 * npix * 3 : nullptr,
                    border_mask ? border_mask + b0 * npix : nullptr,
                    out + b0 * npix * 3,
                    (uint8_t*)ws + b0 * stride,
                    stride,
                    image_buffer_bytes(H, W)};
    bool pass = false, jitter = false, rbc = false, blur = false, iso = false, clahe = false;      // does any image ask for the stage
    for (int j = 0; j < nb; ++j) {
      const Program& p = bt.p[j];
      if (!p.pass) continue;
      pass = true;
      jitter |= p.jitter != 0;
      rbc |= p.rbc != 0;
      blur |= p.ksize == 3;
      iso |= p.iso != 0;
      clahe |= p.clahe != 0;
    }
    const dim3 pixels(gx, nb);
    if (pass) {
      color_bytes_kernel<<<pixels, kPixThreads, 0, st>>>(im, f, bt);
      ISR_CHECK_LAUNCH("color_bytes_kernel");
    }
    if (jitter) {
      color_gray_kernel<<<nb, kSumThreads, 0, st>>>(im, f, bt);
      ISR_CHECK_LAUNCH("color_gray_kernel");
    }
    if (jitter || rbc) {
      color_jitter_kernel<<<pixels, kPixThreads, 0, st>>>(im, f, bt);
      ISR_CHECK_LAUNCH("color_jitter_kernel");
    }
    if (blur) {
      color_blur_kernel<<<pixels, kPixThreads, 0, st>>>(im, f, bt);
      ISR_CHECK_LAUNCH("color_blur_kernel");
    }
    if (iso) {
      color_noise_kernel<<<nb, kSumThreads, 0, st>>>(im, f, bt);
      ISR_CHECK_LAUNCH("color_noise_kernel");
      color_iso_kernel<<<pixels, kPixThreads, 0, st>>>(im, f, bt);
      ISR_CHECK_LAUNCH("color_iso_kernel");
    }
    if (clahe) {
      color_tables_kernel<<<dim3(kTiles, nb), kPixThreads, 0, st>>>(im, f, bt);
      ISR_CHECK_LAUNCH("color_tables_kernel");
    }
    color_finish_kernel<<<pixels, kPixThreads, 0, st>>>(im, f, bt);
    ISR_CHECK_LAUNCH("color_finish_kernel");
  }
  return ISR_OK;
}

extern "C" int isr_augment_color_host(const float* in, int B, int H, int W, const isr_color_program* programs_host,
                                      const float* select, const float* under, const int32_t* border_host,
                                      const float* border_mask, const float* mean3, const float* std3, float* out) {
  const char* who = "isr_augment_color_host";
  std::vector<Batch> batches;
  if (int rc = check_call(who, in, B, H, W, programs_host, select, under, border_host, border_mask, mean3, std3, out, nullptr, 0,
                          batches))
    return rc;
  const Frame f{H, W};
  const size_t npix = (size_t)H * W;
  isr::parallel_rows(B, 1, [&](long b) {
    image_host(in + b * npix * 3, select ? select + b * npix : nullptr, under ? under + b * npix * 3 : nullptr,
               border_mask ? border_mask + b * npix : nullptr, f, batches[b / kMaxBatch], (int)(b % kMaxBatch), out + b * npix * 3);
  });
  return ISR_OK;
}

extern "C" int isr_color_aug_draws_host(uint64_t noise_key, int n, double lambda, int32_t* k_out, double* z_out) {
  ISR_REQUIRE(k_out && z_out && n >= 1, "isr_color_aug_draws_host: null pointer or n=%d < 1", n);
  ISR_REQUIRE(std::isfinite(lambda) && lambda >= 0, "isr_color_aug_draws_host: lambda must be finite and >= 0");
  double cdf[kBins];
  poisson_cdf(lambda, cdf);
  const uint32_t k0 = (uint32_t)noise_key, k1 = (uint32_t)(noise_key >> 32);
  for (int i = 0; i < n; ++i) {
    k_out[i] = poisson_k(cdf, poisson_word((uint32_t)i, k0, k1));
    z_out[i] = irwin_hall((uint32_t)i, k0, k1);
  }
  return ISR_OK;
}

extern "C" int isr_color_aug_geometry(int which) {
  switch (which) {
    case 0: return kPixThreads;
    case 1: return kMaxBatch;
    case 2: return kMaxLaunches;
    case 3: return (int)sizeof(isr_color_program);
    default: return -1;
  }
}
