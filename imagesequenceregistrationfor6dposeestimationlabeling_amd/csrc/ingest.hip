// ingest.hip — sequence ingest on the device (include/isr_ingest.h states every rule, csrc/ingest.hpp the arithmetic):
// cowrendersynth.py:667-736 for n frames in three launches, whatever n is.
//   box pass       frames on blockIdx.z (groups of 64 on blockIdx.y), strips of rows on blockIdx.x.  A strip is a contiguous byte
//                  range of the mask: head bytes up to the first 16-aligned address, 16-byte loads, tail bytes.  Min / max over
//                  64 lanes with cross-lane moves, the four waves meet in LDS, one partial box per workgroup to the workspace.
//   geometry pass  one thread per frame folds the strips in strip order: geom, status, K_out.
//   resize pass    one lane per output pixel: three colours and the silhouette from the same four neighbour addresses.
// HBM-bound byte work: the mask once for the box, then the boxes' footprint of rgb and mask, 4 f32 written per output pixel.
// No atomics, no host synchronisation; the box never visits the host.
#include "block_prims.hpp"
#include "isr_common.hpp"

#include "../../include/isr_ingest.h"
#include "ingest.hpp"

namespace {

using namespace isr::ingest;

static_assert(kFrameGroup == ISR_INGEST_FRAME_GROUP && kMaxB == ISR_INGEST_MAX_B && kMaxOffset == ISR_INGEST_MAX_OFFSET &&
                  kSilLinear == ISR_INGEST_SIL_LINEAR && kSilNearest == ISR_INGEST_SIL_NEAREST,
              "csrc/ingest.hpp and include/isr_ingest.h disagree");

__device__ __forceinline__ int frame_index() { return (int)(blockIdx.y * kFrameGroup + blockIdx.z); }

__global__ __launch_bounds__(kThreads) void ingest_box_kernel(const uint8_t* __restrict__ mask, int n, int H, int W, int Cm,
                                                              int rows, int strips, int32_t* __restrict__ partial) {
  __shared__ int32_t red[kThreads / isr::kWave][4];
  const int frame = frame_index();
  if (frame >= n) return;
  const int strip = blockIdx.x;
  const uint32_t row_bytes = (uint32_t)W * (uint32_t)Cm;
  const uint8_t* __restrict__ m = mask + (size_t)frame * H * row_bytes;
  const int r0 = strip * rows, r1 = min(r0 + rows, H);
  const uint32_t beg = (uint32_t)r0 * row_bytes, end = (uint32_t)r1 * row_bytes;      // < 3 * 2^28
  uint32_t head = (16u - (uint32_t)((uintptr_t)(m + beg) & 15u)) & 15u;
  head = min(head, end - beg);
  const uint32_t chunks = (end - beg - head) / kChunk;
  const uint32_t tail0 = beg + head + chunks * kChunk;

  Box b = empty_box(H, W);
  if (threadIdx.x < head) box_byte(b, beg + threadIdx.x, m[beg + threadIdx.x], row_bytes, Cm);
  const uint4* __restrict__ body = reinterpret_cast<const uint4*>(m + beg + head);
  for (uint32_t k = threadIdx.x; k < chunks; k += kThreads) {
    const uint4 v = body[k];
    box_chunk(b, beg + head + k * kChunk, v.x, v.y, v.z, v.w, row_bytes, Cm);
  }
  if (tail0 + threadIdx.x < end) box_byte(b, tail0 + threadIdx.x, m[tail0 + threadIdx.x], row_bytes, Cm);      // < 16 bytes

  b.x0 = isr::wave_reduce(b.x0, isr::Min{});
  b.y0 = isr::wave_reduce(b.y0, isr::Min{});
  b.x1 = isr::wave_reduce(b.x1, isr::Max{});
  b.y1 = isr::wave_reduce(b.y1, isr::Max{});
  if ((threadIdx.x & 63) == 0) {
    const int w = threadIdx.x >> 6;
    red[w][0] = b.x0; red[w][1] = b.y0; red[w][2] = b.x1; red[w][3] = b.y1;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < kThreads / isr::kWave; ++w) box_merge(b, Box{red[w][0], red[w][1], red[w][2], red[w][3]});
    int32_t* p = partial + ((size_t)frame * strips + strip) * 4;
    p[0] = b.x0; p[1] = b.y0; p[2] = b.x1; p[3] = b.y1;
  }
}

__global__ __launch_bounds__(kThreads) void ingest_geometry_kernel(const int32_t* __restrict__ partial, const double* __restrict__ K_in,
                                                                   int n, int H, int W, int strips, int maxB, int offset,
                                                                   int make_ndc, double* __restrict__ K_out,
                                                                   int32_t* __restrict__ geom, int32_t* __restrict__ status) {
  const int frame = blockIdx.x * kThreads + threadIdx.x;
  if (frame >= n) return;
  Box b = empty_box(H, W);
  const int32_t* p = partial + (size_t)frame * strips * 4;
  for (int s = 0; s < strips; ++s) box_merge(b, Box{p[4 * s], p[4 * s + 1], p[4 * s + 2], p[4 * s + 3]});
  const Geom g = make_geom(b, offset);
  int32_t* go = geom + (size_t)frame * 8;
  go[0] = g.x2; go[1] = g.y2; go[2] = g.w2; go[3] = g.h2; go[4] = g.hw; go[5] = g.hh; go[6] = g.side; go[7] = g.hs1;
  status[frame] = g.side == 0 ? 1 : 0;
  double Kin[9], Ko[16];
#pragma unroll
  for (int i = 0; i < 9; ++i) Kin[i] = K_in[(size_t)frame * 9 + i];
  camera(Kin, g, maxB, make_ndc, Ko);
#pragma unroll
  for (int i = 0; i < 16; ++i) K_out[(size_t)frame * 16 + i] = Ko[i];
}

__global__ __launch_bounds__(kThreads) void ingest_resize_kernel(const uint8_t* __restrict__ rgb, const uint8_t* __restrict__ mask,
                                                                 int n, int H, int W, int Cm, const int32_t* __restrict__ geom,
                                                                 int maxB, int sil_mode, float* __restrict__ images,
                                                                 float* __restrict__ silhouettes) {
  const int frame = frame_index();
  if (frame >= n) return;
  const int pix = blockIdx.x * kThreads + threadIdx.x;      // maxB^2 <= 2^24
  if (pix >= maxB * maxB) return;
  const int dy = pix / maxB, dx = pix - dy * maxB;
  const int32_t* gi = geom + (size_t)frame * 8;
  const Geom g{gi[0], gi[1], gi[2], gi[3], gi[4], gi[5], gi[6], gi[7]};
  const size_t npix = (size_t)H * W;
  const Frame f{rgb + (size_t)frame * npix * 3, mask + (size_t)frame * npix * Cm, H, W, Cm};
  float c3[3] = {0.f, 0.f, 0.f}, s = 0.f;
  if (g.side != 0) view_pixel(f, g, maxB, sil_mode, dy, dx, c3, s);
  const size_t o = (size_t)frame * maxB * maxB + pix;
  images[3 * o] = c3[0];
  images[3 * o + 1] = c3[1];
  images[3 * o + 2] = c3[2];
  silhouettes[o] = s;
}

__global__ __launch_bounds__(kThreads) void ingest_empty_kernel() {}

int check_call(const char* who, const void* rgb, const void* mask, const void* K_in, int n, int H, int W, int Cm, int maxB,
               int offset, int sil_mode, const void* images, const void* silhouettes, const void* K_out, const void* geom,
               const void* status) {
  ISR_REQUIRE(rgb && mask && K_in && images && silhouettes && K_out && geom && status, "%s: null pointer", who);
  const char* bad = check_shape(n, H, W, Cm, maxB, offset, sil_mode);
  ISR_REQUIRE(!bad, "%s: %s (n=%d H=%d W=%d Cm=%d maxB=%d offset=%d sil_mode=%d)", who, bad, n, H, W, Cm, maxB, offset, sil_mode);
  return ISR_OK;
}

dim3 frame_grid(unsigned x, int n) {
  return dim3(x, (unsigned)((n + kFrameGroup - 1) / kFrameGroup), (unsigned)(n < kFrameGroup ? n : kFrameGroup));
}

}  // namespace

extern "C" size_t isr_ingest_workspace_bytes(int n, int H, int W, int Cm) {
  if (check_shape(n, H, W, Cm, 1, 0, kSilLinear)) return 0;
  return isr::align_up((size_t)n * strips_of(H, W, Cm) * 4 * sizeof(int32_t), 256);
}

extern "C" int isr_ingest_geometry(int which) {
  switch (which) {
    case 0: return kThreads;
    case 1: return kFrameGroup;
    case 2: return 3;
    default: return -1;
  }
}

extern "C" int isr_ingest_strip_rows(int H, int W, int Cm) {
  return check_shape(1, H, W, Cm, 1, 0, kSilLinear) ? 0 : strip_rows(H, W, Cm);
}

extern "C" int isr_ingest_strips(int H, int W, int Cm) {
  return check_shape(1, H, W, Cm, 1, 0, kSilLinear) ? 0 : strips_of(H, W, Cm);
}

extern "C" int isr_ingest_views(const uint8_t* rgb, const uint8_t* mask, const double* K_in, int n, int H, int W, int Cm, int maxB,
                                int offset, int make_ndc, int sil_mode, float* images, float* silhouettes, double* K_out,
                                int32_t* geom, int32_t* status, void* ws, size_t workspace_bytes, isr_stream_t stream) {
  const char* who = "isr_ingest_views";
  if (int rc = check_call(who, rgb, mask, K_in, n, H, W, Cm, maxB, offset, sil_mode, images, silhouettes, K_out, geom, status))
    return rc;
  const size_t need = isr_ingest_workspace_bytes(n, H, W, Cm);
  ISR_REQUIRE(ws && ((uintptr_t)ws & 15u) == 0 && workspace_bytes >= need, "%s: workspace of %zu bytes, 16-byte aligned, needed (got %zu)",
              who, need, workspace_bytes);
  const int rows = strip_rows(H, W, Cm), strips = strips_of(H, W, Cm);
  int32_t* partial = static_cast<int32_t*>(ws);
  hipStream_t st = isr::as_stream(stream);
  ingest_box_kernel<<<frame_grid((unsigned)strips, n), kThreads, 0, st>>>(mask, n, H, W, Cm, rows, strips, partial);
  ISR_CHECK_LAUNCH("ingest_box_kernel");
  ingest_geometry_kernel<<<dim3((unsigned)((n + kThreads - 1) / kThreads)), kThreads, 0, st>>>(partial, K_in, n, H, W, strips, maxB,
                                                                                             offset, make_ndc, K_out, geom, status);
  ISR_CHECK_LAUNCH("ingest_geometry_kernel");
  ingest_resize_kernel<<<frame_grid((unsigned)((maxB * maxB + kThreads - 1) / kThreads), n), kThreads, 0, st>>>(
      rgb, mask, n, H, W, Cm, geom, maxB, sil_mode, images, silhouettes);
  ISR_CHECK_LAUNCH("ingest_resize_kernel");
  return ISR_OK;
}

extern "C" int isr_ingest_views_host(const uint8_t* rgb, const uint8_t* mask, const double* K_in, int n, int H, int W, int Cm,
                                     int maxB, int offset, int make_ndc, int sil_mode, float* images, float* silhouettes,
                                     double* K_out, int32_t* geom, int32_t* status) {
  const char* who = "isr_ingest_views_host";
  if (int rc = check_call(who, rgb, mask, K_in, n, H, W, Cm, maxB, offset, sil_mode, images, silhouettes, K_out, geom, status))
    return rc;
  const size_t npix = (size_t)H * W, nout = (size_t)maxB * maxB;
  isr::parallel_rows(n, 1, [&](long i) {
    const Frame f{rgb + i * npix * 3, mask + i * npix * Cm, H, W, Cm};
    frame_host(f, K_in + i * 9, maxB, offset, make_ndc, sil_mode, images + i * nout * 3, silhouettes + i * nout, K_out + i * 16,
               geom + i * 8, status + i);
  });
  return ISR_OK;
}

extern "C" int isr_ingest_launch_floor(int n, int H, int W, int Cm, int maxB, isr_stream_t stream) {
  const char* bad = check_shape(n, H, W, Cm, maxB, 0, kSilLinear);
  ISR_REQUIRE(!bad, "isr_ingest_launch_floor: %s", bad);
  hipStream_t st = isr::as_stream(stream);
  ingest_empty_kernel<<<frame_grid((unsigned)strips_of(H, W, Cm), n), kThreads, 0, st>>>();
  ingest_empty_kernel<<<dim3((unsigned)((n + kThreads - 1) / kThreads)), kThreads, 0, st>>>();
  ingest_empty_kernel<<<frame_grid((unsigned)((maxB * maxB + kThreads - 1) / kThreads), n), kThreads, 0, st>>>();
  ISR_CHECK_LAUNCH("ingest_empty_kernel");
  return ISR_OK;
}
