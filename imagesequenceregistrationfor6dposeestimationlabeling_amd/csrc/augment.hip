// augment.hip — training batches on the device (include/isr_augment.h states every rule, csrc/augment.hpp the arithmetic):
//   isr_augment_images: augment.py:284-432's warps, paste and borderADD blanking with dataGen.py:16-20's normalize, one image
//     per blockIdx.z in two launches (the masks; then the colours, which read mask_out for the paste and the dilation).
//     HBM-bound byte work: per pixel four neighbours of a u8 mask twice and of the f32 image three times, 5 f32 written.
//   isr_augment_rays: augment.py:639-685's remap, inside filter and sample for B views and both sets in one launch, one
//     1024-thread workgroup per (image, set): count, radix select of the cut on the Philox word (as csrc/select_top.hip and
//     csrc/knn.hip do), an ordered gather and a bitonic sort in LDS (as csrc/sample_grad.hip does).
// The per-image parameters are made on the host and travel as kernel arguments: no copy, no synchronisation, no workspace.
#include "block_prims.hpp"
#include "isr_common.hpp"

#include "../../include/isr_augment.h"
#include "augment.hpp"

namespace {

using namespace isr::augment;

constexpr int kPixThreads = 256;
constexpr int kRayThreads = 1024;
constexpr int kRayWaves = kRayThreads / isr::kWave;

__global__ __launch_bounds__(kPixThreads) void augment_masks_kernel(const uint8_t* __restrict__ mask,
                                                                    const uint8_t* __restrict__ orig_mask, Frame f, ImageBatch ib,
                                                                    float* __restrict__ mask_orig_out,
                                                                    float* __restrict__ mask_out) {
  const int b = blockIdx.z;
  const size_t npix = (size_t)f.H * f.W;
  const size_t pix = (size_t)blockIdx.x * kPixThreads + threadIdx.x;
  if (pix >= npix) return;
  const int y = (int)(pix / f.W), x = (int)(pix - (size_t)y * f.W);
  const ImageParams& p = ib.p[b];
  mask_out[b * npix + pix] = mask_out_at(mask + b * npix, f, p, x, y);
  mask_orig_out[b * npix + pix] = mask_orig_at(orig_mask + b * npix, f, p, x, y);
}

__global__ __launch_bounds__(kPixThreads) void augment_colours_kernel(const float* __restrict__ rgb,
                                                                      const float* __restrict__ canvas,
                                                                      const float* __restrict__ mask_out, Frame f, ImageBatch ib,
                                                                      float* __restrict__ rgb_out) {
  const int b = blockIdx.z;
  const size_t npix = (size_t)f.H * f.W;
  const size_t pix = (size_t)blockIdx.x * kPixThreads + threadIdx.x;
  if (pix >= npix) return;
  const int y = (int)(pix / f.W), x = (int)(pix - (size_t)y * f.W);
  float out3[3];
  rgb_out_at(rgb + b * npix * 3, canvas ? canvas + b * npix * 3 : nullptr, mask_out + b * npix, f, ib.p[b], ib.mu, ib.sd, x, y,
             out3);
  float* o = rgb_out + (b * npix + pix) * 3;
  o[0] = out3[0];
  o[1] = out3[1];
  o[2] = out3[2];
}

// the sum of v over the workgroup, to every thread; red: kRayWaves words of LDS
__device__ __forceinline__ int block_sum(int v, int* red) {
  v = isr::wave_reduce(v, isr::Plus{});
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  int s = 0;
#pragma unroll
  for (int w = 0; w < kRayWaves; ++w) s += red[w];
  __syncthreads();
  return s;
}

__global__ __launch_bounds__(kRayThreads) void augment_rays_kernel(RaySet in0, RaySet in1, RayBatch rb, int S, uint32_t k0,
                                                                   uint32_t k1, RayOut out0, RayOut out1) {
  __shared__ uint64_t keys[kMaxSample];
  __shared__ uint32_t hist[256];
  __shared__ int red[kRayWaves];
  __shared__ uint32_t wave_tot[kRayWaves];

  const int set = blockIdx.x, j = blockIdx.y, tid = threadIdx.x;
  const RaySet in = set ? in1 : in0;
  const RayOut out = set ? out1 : out0;
  const int n = rb.n[set][j];
  const uint32_t view = (uint32_t)rb.view[j];
  const float* __restrict__ xy = in.xys + 2 * rb.start[set][j];
  const float* __restrict__ pos = in.pos + 3 * rb.start[set][j];
  const float m[4] = {rb.m[j][0], rb.m[j][1], rb.m[j][2], rb.m[j][3]};
  const float t[2] = {rb.t[j][0], rb.t[j][1]};

  // 1: does any coordinate touch or leave (-1, 1), and how many rows lie strictly inside
  int n_out = 0, n_in = 0;
  for (int i = tid; i < n; i += kRayThreads) {
    float sx, sy;
    remap(m, t, xy[2 * i], xy[2 * i + 1], sx, sy);
    n_out += touches_outside(sx, sy) ? 1 : 0;
    n_in += strictly_inside(sx, sy) ? 1 : 0;
  }
  const bool filter = block_sum(n_out, red) > 0;
  const int m_cand = filter ? block_sum(n_in, red) : n;
  const int K = m_cand < S ? m_cand : S;

  auto candidate = [&](int i) -> bool {
    if (!filter) return true;
    float sx, sy;
    remap(m, t, xy[2 * i], xy[2 * i + 1], sx, sy);
    return strictly_inside(sx, sy);
  };

  // 2: the cut.  T: the K-th smallest word; `need` of the candidates whose word equals T are taken, in row order.
  const bool take_all = m_cand <= S;
  uint32_t T = 0, known = 0;
  int need = K;
  if (!take_all) {
    for (int shift = 24; shift >= 0; shift -= 8) {
      if (tid < 256) hist[tid] = 0;
      __syncthreads();
      for (int i = tid; i < n; i += kRayThreads) {
        if (!candidate(i)) continue;
        const uint32_t w = key_word((uint32_t)i, view, (uint32_t)set, k0, k1);
        if ((w & known) == T) atomicAdd(&hist[(w >> shift) & 255u], 1u);      // counts only: the order cannot matter
      }
      __syncthreads();
      int cum = 0, digit = 255;
      for (int d = 0; d < 256; ++d) {          // every thread reads the same words: the result is uniform
        const int h = (int)hist[d];
        if (cum + h >= need) {
          digit = d;
          break;
        }
        cum += h;
      }
      need -= cum;
      T |= (uint32_t)digit << shift;
      known |= 255u << shift;
      __syncthreads();
    }
  }
  const int n_less = take_all ? K : K - need;   // candidates whose word is below T

  // 3: the ordered gather.  Ranks come from ballots and a scan over the waves: no atomics.
  const int lane = tid & 63, wave = tid >> 6;
  int base_less = 0, base_tie = 0;
  for (int i0 = 0; i0 < n; i0 += kRayThreads) {
    const int i = i0 + tid;
    bool less = false, tie = false;
    uint32_t w = 0;
    if (i < n && candidate(i)) {
      w = key_word((uint32_t)i, view, (uint32_t)set, k0, k1);
      less = take_all || w < T;
      tie = !take_all && w == T;
    }
    const unsigned long long bl = __ballot(less), bt = __ballot(tie);
    const unsigned long long below = (1ull << lane) - 1ull;
    if (lane == 0) wave_tot[wave] = (uint32_t)__popcll(bl) | ((uint32_t)__popcll(bt) << 16);
    __syncthreads();
    uint32_t before = 0, total = 0;
#pragma unroll
    for (int v = 0; v < kRayWaves; ++v) {
      const uint32_t c = wave_tot[v];
      total += c;
      if (v < wave) before += c;
    }
    if (less) {
      const int slot = base_less + (int)(before & 0xFFFFu) + __popcll(bl & below);
      if (slot < K) keys[slot] = ((uint64_t)w << 32) | (uint32_t)i;
    }
    if (tie) {
      const int r = base_tie + (int)(before >> 16) + __popcll(bt & below);
      if (r < need && n_less + r < K) keys[n_less + r] = ((uint64_t)w << 32) | (uint32_t)i;
    }
    base_less += (int)(total & 0xFFFFu);
    base_tie += (int)(total >> 16);
    __syncthreads();
  }

  // 4: bitonic sort of the K keys, padded to a power of two with keys above every real one
  int Ns = 2;
  while (Ns < K) Ns <<= 1;
  for (int r = K + tid; r < Ns; r += kRayThreads) keys[r] = ~0ull;
  __syncthreads();
  for (int k = 2; k <= Ns; k <<= 1)
    for (int s = k >> 1; s > 0; s >>= 1) {
      for (int a = tid; a < Ns; a += kRayThreads) {
        const int c = a ^ s;
        if (c > a) {
          const uint64_t ka = keys[a], kc = keys[c];
          if ((ka > kc) == ((a & k) == 0)) {
            keys[a] = kc;
            keys[c] = ka;
          }
        }
      }
      __syncthreads();
    }

  // 5: the rows
  for (int r = tid; r < S; r += kRayThreads) {
    const size_t row = (size_t)j * S + r;
    float sx = 0.f, sy = 0.f, p0 = 0.f, p1 = 0.f, p2 = 0.f;
    int32_t idx = -1;
    if (r < K) {
      const uint32_t i = (uint32_t)keys[r];
      remap(m, t, xy[2 * i], xy[2 * i + 1], sx, sy);
      p0 = pos[3 * (size_t)i];
      p1 = pos[3 * (size_t)i + 1];
      p2 = pos[3 * (size_t)i + 2];
      idx = (int32_t)i;
    }
    out.xys[2 * row] = sx;
    out.xys[2 * row + 1] = sy;
    out.pos[3 * row] = p0;
    out.pos[3 * row + 1] = p1;
    out.pos[3 * row + 2] = p2;
    out.index[row] = idx;
  }
  if (tid == 0) out.count[j] = K;
}

int check_images(const char* who, const void* rgb, const void* mask, const void* orig_mask, int B, int H, int W, const void* M,
                 const void* mean3, const void* std3, const void* rgb_out, const void* mask_orig_out, const void* mask_out) {
  ISR_REQUIRE(rgb && mask && orig_mask && M && mean3 && std3 && rgb_out && mask_orig_out && mask_out, "%s: null pointer", who);
  ISR_REQUIRE(B >= 1 && H >= 1 && W >= 1 && (long long)H * W <= kMaxPixels, "%s: B=%d H=%d W=%d (B, H, W >= 1, H W <= 2^28)", who,
              B, H, W);
  return ISR_OK;
}

int check_rays(const char* who, const void* xys_f, const void* pos_f, const void* off_f, const void* xys_b, const void* pos_b,
               const void* off_b, int V, const void* view_ids, const void* rot, const void* t, int B, int S, const void* xo_f,
               const void* po_f, const void* io_f, const void* c_f, const void* xo_b, const void* po_b, const void* io_b,
               const void* c_b) {
  ISR_REQUIRE(xys_f && pos_f && off_f && view_ids && rot && t && xo_f && po_f && io_f && c_f, "%s: null pointer", who);
  const bool back = xys_b || pos_b || off_b || xo_b || po_b || io_b || c_b;
  ISR_REQUIRE(!back || (xys_b && pos_b && off_b && xo_b && po_b && io_b && c_b),
              "%s: the back set needs all of its pointers, or none", who);
  ISR_REQUIRE(B >= 1 && V >= 1, "%s: B=%d V=%d (both >= 1)", who, B, V);
  ISR_REQUIRE(S >= 1 && S <= kMaxSample, "%s: S=%d outside 1..4096", who, S);
  return ISR_OK;
}

}  // namespace

extern "C" int isr_augment_images(const float* rgb, const uint8_t* mask, const uint8_t* orig_mask, const float* canvas, int B,
                                  int H, int W, const int32_t* rect_host, const double* M_host, const int32_t* tra_host,
                                  const int32_t* tra1_host, const int32_t* border_host, const float* mean3, const float* std3,
                                  float* rgb_out, float* mask_orig_out, float* mask_out, isr_stream_t stream) {
  const char* who = "isr_augment_images";
  if (int rc = check_images(who, rgb, mask, orig_mask, B, H, W, M_host, mean3, std3, rgb_out, mask_orig_out, mask_out)) return rc;
  const Frame f{H, W};
  const size_t npix = (size_t)H * W;
  // every batch is checked before the first launch: a refused call writes nothing
  std::vector<ImageBatch> batches((B + kMaxBatch - 1) / kMaxBatch);
  for (int b0 = 0; b0 < B; b0 += kMaxBatch) {
    const int nb = B - b0 < kMaxBatch ? B - b0 : kMaxBatch;
    const char* bad = make_image_batch(b0, nb, rect_host, M_host, tra_host, tra1_host, border_host, mean3, std3,
                                       batches[b0 / kMaxBatch]);
    ISR_REQUIRE(!bad, "%s: %s (images %d..%d)", who, bad, b0, b0 + nb - 1);
  }
  const unsigned gx = (unsigned)((npix + kPixThreads - 1) / kPixThreads);
  for (int b0 = 0; b0 < B; b0 += kMaxBatch) {
    const int nb = B - b0 < kMaxBatch ? B - b0 : kMaxBatch;
    const ImageBatch& ib = batches[b0 / kMaxBatch];
    augment_masks_kernel<<<dim3(gx, 1, nb), kPixThreads, 0, isr::as_stream(stream)>>>(
        mask + b0 * npix, orig_mask + b0 * npix, f, ib, mask_orig_out + b0 * npix, mask_out + b0 * npix);
    ISR_CHECK_LAUNCH("augment_masks_kernel");
    augment_colours_kernel<<<dim3(gx, 1, nb), kPixThreads, 0, isr::as_stream(stream)>>>(
        rgb + b0 * npix * 3, canvas ? canvas + b0 * npix * 3 : nullptr, mask_out + b0 * npix, f, ib, rgb_out + b0 * npix * 3);
    ISR_CHECK_LAUNCH("augment_colours_kernel");
  }
  return ISR_OK;
}

extern "C" int isr_augment_images_host(const float* rgb, const uint8_t* mask, const uint8_t* orig_mask, const float* canvas, int B,
                                       int H, int W, const int32_t* rect_host, const double* M_host, const int32_t* tra_host,
                                       const int32_t* tra1_host, const int32_t* border_host, const float* mean3,
                                       const float* std3, float* rgb_out, float* mask_orig_out, float* mask_out) {
  const char* who = "isr_augment_images_host";
  if (int rc = check_images(who, rgb, mask, orig_mask, B, H, W, M_host, mean3, std3, rgb_out, mask_orig_out, mask_out)) return rc;
  const Frame f{H, W};
  const size_t npix = (size_t)H * W;
  std::vector<ImageBatch> batches((B + kMaxBatch - 1) / kMaxBatch);
  for (int b0 = 0; b0 < B; b0 += kMaxBatch) {
    const int nb = B - b0 < kMaxBatch ? B - b0 : kMaxBatch;
    const char* bad = make_image_batch(b0, nb, rect_host, M_host, tra_host, tra1_host, border_host, mean3, std3,
                                       batches[b0 / kMaxBatch]);
    ISR_REQUIRE(!bad, "%s: %s (images %d..%d)", who, bad, b0, b0 + nb - 1);
  }
  isr::parallel_rows(B, 1, [&](long b) {
    const ImageBatch& ib = batches[b / kMaxBatch];
    images_host_one(rgb + b * npix * 3, mask + b * npix, orig_mask + b * npix, canvas ? canvas + b * npix * 3 : nullptr, f,
                    ib.p[b % kMaxBatch], ib.mu, ib.sd, rgb_out + b * npix * 3, mask_orig_out + b * npix, mask_out + b * npix);
  });
  return ISR_OK;
}

extern "C" int isr_augment_rays(const float* xys_front, const float* pos_front, const int64_t* offsets_front_host,
                                const float* xys_back, const float* pos_back, const int64_t* offsets_back_host, int V,
                                const int32_t* view_ids_host, const float* rot_host, const float* t_host, int B, int S,
                                uint64_t seed, float* xys_out_front, float* pos_out_front, int32_t* index_out_front,
                                int32_t* count_front, float* xys_out_back, float* pos_out_back, int32_t* index_out_back,
                                int32_t* count_back, isr_stream_t stream) {
  const char* who = "isr_augment_rays";
  if (int rc = check_rays(who, xys_front, pos_front, offsets_front_host, xys_back, pos_back, offsets_back_host, V, view_ids_host,
                          rot_host, t_host, B, S, xys_out_front, pos_out_front, index_out_front, count_front, xys_out_back,
                          pos_out_back, index_out_back, count_back))
    return rc;
  const int sets = xys_back ? 2 : 1;
  const int64_t* offsets[2] = {offsets_front_host, offsets_back_host};
  std::vector<RayBatch> batches((B + kMaxBatch - 1) / kMaxBatch);
  for (int b0 = 0; b0 < B; b0 += kMaxBatch) {
    const int nb = B - b0 < kMaxBatch ? B - b0 : kMaxBatch;
    const char* bad = make_ray_batch(b0, nb, offsets, V, view_ids_host, rot_host, t_host, batches[b0 / kMaxBatch]);
    ISR_REQUIRE(!bad, "%s: %s (images %d..%d)", who, bad, b0, b0 + nb - 1);
  }
  const RaySet in0{xys_front, pos_front}, in1{xys_back, pos_back};
  for (int b0 = 0; b0 < B; b0 += kMaxBatch) {
    const int nb = B - b0 < kMaxBatch ? B - b0 : kMaxBatch;
    const size_t r0 = (size_t)b0 * S;
    const RayOut out0{xys_out_front + 2 * r0, pos_out_front + 3 * r0, index_out_front + r0, count_front + b0};
    const RayOut out1 = sets == 2 ? RayOut{xys_out_back + 2 * r0, pos_out_back + 3 * r0, index_out_back + r0, count_back + b0}
                                  : RayOut{nullptr, nullptr, nullptr, nullptr};
    augment_rays_kernel<<<dim3(sets, nb), kRayThreads, 0, isr::as_stream(stream)>>>(
        in0, in1, batches[b0 / kMaxBatch], S, (uint32_t)seed, (uint32_t)(seed >> 32), out0, out1);
    ISR_CHECK_LAUNCH("augment_rays_kernel");
  }
  return ISR_OK;
}

extern "C" int isr_augment_rays_host(const float* xys_front, const float* pos_front, const int64_t* offsets_front_host,
                                     const float* xys_back, const float* pos_back, const int64_t* offsets_back_host, int V,
                                     const int32_t* view_ids_host, const float* rot_host, const float* t_host, int B, int S,
                                     uint64_t seed, float* xys_out_front, float* pos_out_front, int32_t* index_out_front,
                                     int32_t* count_front, float* xys_out_back, float* pos_out_back, int32_t* index_out_back,
                                     int32_t* count_back) {
  const char* who = "isr_augment_rays_host";
  if (int rc = check_rays(who, xys_front, pos_front, offsets_front_host, xys_back, pos_back, offsets_back_host, V, view_ids_host,
                          rot_host, t_host, B, S, xys_out_front, pos_out_front, index_out_front, count_front, xys_out_back,
                          pos_out_back, index_out_back, count_back))
    return rc;
  const int sets = xys_back ? 2 : 1;
  const int64_t* offsets[2] = {offsets_front_host, offsets_back_host};
  std::vector<RayBatch> batches((B + kMaxBatch - 1) / kMaxBatch);
  for (int b0 = 0; b0 < B; b0 += kMaxBatch) {
    const int nb = B - b0 < kMaxBatch ? B - b0 : kMaxBatch;
    const char* bad = make_ray_batch(b0, nb, offsets, V, view_ids_host, rot_host, t_host, batches[b0 / kMaxBatch]);
    ISR_REQUIRE(!bad, "%s: %s (images %d..%d)", who, bad, b0, b0 + nb - 1);
  }
  const RaySet in[2] = {{xys_front, pos_front}, {xys_back, pos_back}};
  const RayOut out[2] = {{xys_out_front, pos_out_front, index_out_front, count_front},
                         {xys_out_back, pos_out_back, index_out_back, count_back}};
  for (int b = 0; b < B; ++b)
    for (int s = 0; s < sets; ++s)
      rays_host_one(in[s], batches[b / kMaxBatch], b % kMaxBatch, s, S, (uint32_t)seed, (uint32_t)(seed >> 32), out[s], (size_t)b);
  return ISR_OK;
}
