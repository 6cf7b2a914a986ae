// render_coords.hip — object-coordinate rasteriser (the reference's ObjCoordRenderer, renderer.py:37-117, without GL):
// one triangle mesh drawn at B poses with B cameras into B frame buffers.  The arithmetic and its rules are stated in
// csrc/raster.hpp; isr_render_coords_host runs the same header as host code, so the two agree bit for bit.
//
// Three launches per call, blockIdx.y the pose:
//   init     per pixel: the z-buffer key the draw starts from (empty, or what the frame buffer holds when clear = 0);
//            the item's counters.
//   raster   per face (one wave = 64 faces): transform, project, snap, box.  A lane walks its own box when it holds at
//            most kLaneBox pixel centres; larger boxes are walked by the whole wave, one face after the other, from the
//            setups the lanes left in LDS.  Every surviving fragment does a 64-bit atomicMin of
//            (f32 depth bits << 32 | face + 1) on the pose's key image (positive floats order as their bits), behind a
//            plain load that skips fragments already hidden.  Integer min only: the result does not depend on the order.
//   resolve  per pixel: decode the face, recompute its setup and barycentrics, interpolate, write colour and depth, count.
// The key image is the whole workspace (8 bytes per pixel and pose: 400 KB at 224 x 224, L2-resident); nothing per face
// is stored.
#include "isr_common.hpp"
#include "raster.hpp"

#include <cmath>
#include <vector>

namespace {

namespace rs = isr::raster;

constexpr int kPixBlock = 256;
constexpr int kLaneBox = 64;       // boxes with more pixel centres than this are walked by the whole wave

__device__ __forceinline__ rs::Camera load_camera(const double* K, const double* Rt, int b) {
  rs::Camera cam;
#pragma unroll
  for (int i = 0; i < 9; ++i) cam.K[i] = K[(size_t)b * 9 + i];
#pragma unroll
  for (int i = 0; i < 12; ++i) cam.Rt[i] = Rt[(size_t)b * 12 + i];
  return cam;
}

__device__ __forceinline__ size_t item_floats(int h, int w) { return (size_t)5 * h * w + 4; }

__global__ __launch_bounds__(kPixBlock) void render_init_kernel(unsigned long long* __restrict__ keys, float* __restrict__ state,
                                                               int h, int w, int clear) {
  const int b = blockIdx.y;
  const size_t npix = (size_t)h * w;
  float* item = state + (size_t)b * item_floats(h, w);
  const size_t p = (size_t)blockIdx.x * kPixBlock + threadIdx.x;
  if (p < npix) {
    unsigned long long key = rs::kEmptyKey;
    if (!clear) key = rs::initial_key(0, item[4 * p + 3], item[4 * npix + p]);
    keys[(size_t)b * npix + p] = key;
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    int32_t* cnt = reinterpret_cast<int32_t*>(item + 5 * npix);
    if (clear) cnt[0] = cnt[1] = 0;
    cnt[2] = 0;
    cnt[3] = 0;
  }
}

__device__ __forceinline__ void try_fragment(const rs::Face& F, int f, int r, int c, double near_, double far_,
                                             unsigned long long* keys, int w) {
  unsigned long long key;
  if (!rs::fragment_key(F, f, r, c, near_, far_, &key)) return;
  unsigned long long* p = keys + (size_t)r * w + c;
  if (key < *p) atomicMin(p, key);      // keys only fall: a stale read can only let a hidden fragment through to the atomic
}

__global__ __launch_bounds__(isr::kWave) void render_raster_kernel(const float* __restrict__ verts, int n_vert,
                                                                   const int32_t* __restrict__ faces, int n_face,
                                                                   const double* __restrict__ K, const double* __restrict__ Rt,
                                                                   int h, int w, double near_, double far_,
                                                                   unsigned long long* keys_all, float* state) {
  __shared__ rs::Face sh[isr::kWave];
  const int b = blockIdx.y;
  const int lane = threadIdx.x;
  const int f0 = blockIdx.x * isr::kWave;
  const int f = f0 + lane;
  const rs::Camera cam = load_camera(K, Rt, b);
  unsigned long long* keys = keys_all + (size_t)b * h * w;
  rs::Face F;
  F.status = rs::kFaceDropped;
  F.c0 = F.r0 = 0;
  F.c1 = F.r1 = -1;
  const bool live = f < n_face;
  if (live) rs::setup_face(verts, n_vert, faces, f, cam, near_, h, w, &F);
  const unsigned long long dropped = __ballot(live && F.status == rs::kFaceDropped);
  const unsigned long long drawn = __ballot(live && F.status != rs::kFaceDropped);
  if (lane == 0) {
    int32_t* cnt = reinterpret_cast<int32_t*>(state + (size_t)b * item_floats(h, w) + (size_t)5 * h * w);
    if (drawn) atomicAdd(&cnt[0], __popcll(drawn));
    if (dropped) atomicAdd(&cnt[1], __popcll(dropped));
  }
  const int bw = F.c1 - F.c0 + 1, bh = F.r1 - F.r0 + 1;
  const bool has_box = F.status == rs::kFaceOk && bw > 0 && bh > 0;
  const bool big = has_box && (long long)bw * bh > kLaneBox;
  if (has_box && !big) {
    for (int r = F.r0; r <= F.r1; ++r)
      for (int c = F.c0; c <= F.c1; ++c) try_fragment(F, f, r, c, near_, far_, keys, w);
  }
  unsigned long long todo = __ballot(big);
  if (todo == 0) return;          // wave-uniform
  sh[lane] = F;
  __syncthreads();
  while (todo) {
    const int l = __ffsll((long long)todo) - 1;
    todo &= todo - 1;
    const rs::Face& G = sh[l];
    const int gw = G.c1 - G.c0 + 1;
    const long long n = (long long)gw * (G.r1 - G.r0 + 1);
    for (long long i = lane; i < n; i += isr::kWave)
      try_fragment(G, f0 + l, G.r0 + (int)(i / gw), G.c0 + (int)(i % gw), near_, far_, keys, w);
  }
}

__global__ __launch_bounds__(kPixBlock) void render_resolve_kernel(const float* __restrict__ verts, int n_vert,
                                                                  const int32_t* __restrict__ faces,
                                                                  const double* __restrict__ K, const double* __restrict__ Rt,
                                                                  int h, int w, const float* __restrict__ offset3, float scale,
                                                                  double near_, int clear,
                                                                  const unsigned long long* __restrict__ keys, float* state) {
  const int b = blockIdx.y;
  const size_t npix = (size_t)h * w;
  float* item = state + (size_t)b * item_floats(h, w);
  const size_t p = (size_t)blockIdx.x * kPixBlock + threadIdx.x;
  int covered = 0;
  if (p < npix) {
    const rs::Camera cam = load_camera(K, Rt, b);
    const int r = (int)(p / w), c = (int)(p % w);
    covered = rs::resolve_pixel(keys[(size_t)b * npix + p], clear, verts, n_vert, faces, cam, near_, h, w, offset3, scale, r, c,
                                item + 4 * p, item + 4 * npix + p);
  }
  const unsigned long long m = __ballot(covered != 0);
  if ((threadIdx.x & (isr::kWave - 1)) == 0 && m)
    atomicAdd(reinterpret_cast<int32_t*>(item + 5 * npix) + 2, __popcll(m));
}

int check_args(const char* who, const void* verts, int n_vert, const void* faces, int n_face, const void* K, const void* Rt,
               int h, int w, const void* offset3, float scale, double near_, double far_, const void* state) {
  ISR_REQUIRE(verts && faces && K && Rt && offset3 && state, "%s: null pointer", who);
  ISR_REQUIRE(n_vert > 0 && n_face > 0 && n_face < 0x7FFFFFFF, "%s: n_vert=%d n_face=%d must be positive", who, n_vert, n_face);
  ISR_REQUIRE(h > 0 && w > 0 && h <= rs::kMaxSide && w <= rs::kMaxSide, "%s: h=%d w=%d must be in [1, %d]", who, h, w,
              rs::kMaxSide);
  ISR_REQUIRE(std::isfinite(scale) && scale != 0.0f, "%s: scale=%g must be finite and non-zero", who, (double)scale);
  ISR_REQUIRE(near_ > 0.0 && far_ >= near_ && far_ <= 3.0e38, "%s: need 0 < near=%g <= far=%g <= 3e38", who, near_, far_);
  return ISR_OK;
}

}  // namespace

extern "C" size_t isr_render_coords_batch_workspace_bytes(int n_vert, int n_face, int h, int w, int B) {
  if (n_vert <= 0 || n_face <= 0 || h <= 0 || w <= 0 || B <= 0) return 0;
  return isr::align_up((size_t)B * h * w * sizeof(unsigned long long), 256);
}

extern "C" int isr_render_coords_batch(const float* verts, int n_vert, const int32_t* faces, int n_face, const double* K,
                                       const double* Rt, int B, int h, int w, const float* offset3, float scale, double near_,
                                       double far_, int clear, void* state, void* ws, size_t ws_bytes, isr_stream_t stream) {
  const char* who = "isr_render_coords_batch";
  if (int rc = check_args(who, verts, n_vert, faces, n_face, K, Rt, h, w, offset3, scale, near_, far_, state)) return rc;
  ISR_REQUIRE(B >= 0 && B <= 65535, "%s: B=%d must be in [0, 65535]", who, B);
  if (B == 0) return ISR_OK;
  const size_t need = isr_render_coords_batch_workspace_bytes(n_vert, n_face, h, w, B);
  if (!ws || ws_bytes < need) {
    isr::set_error("%s: workspace %zu < %zu", who, ws_bytes, need);
    return ISR_ERR_WORKSPACE;
  }
  hipStream_t s = isr::as_stream(stream);
  unsigned long long* keys = static_cast<unsigned long long*>(ws);
  float* st = static_cast<float*>(state);
  const unsigned pix_blocks = (unsigned)(((size_t)h * w + kPixBlock - 1) / kPixBlock);
  const unsigned face_blocks = (unsigned)(((size_t)n_face + isr::kWave - 1) / isr::kWave);
  render_init_kernel<<<dim3(pix_blocks, B), kPixBlock, 0, s>>>(keys, st, h, w, clear ? 1 : 0);
  ISR_CHECK_LAUNCH("render_init_kernel");
  render_raster_kernel<<<dim3(face_blocks, B), isr::kWave, 0, s>>>(verts, n_vert, faces, n_face, K, Rt, h, w, near_, far_, keys,
                                                                    st);
  ISR_CHECK_LAUNCH("render_raster_kernel");
  render_resolve_kernel<<<dim3(pix_blocks, B), kPixBlock, 0, s>>>(verts, n_vert, faces, K, Rt, h, w, offset3, scale, near_,
                                                                   clear ? 1 : 0, keys, st);
  ISR_CHECK_LAUNCH("render_resolve_kernel");
  return ISR_OK;
}

extern "C" int isr_render_coords_host(const float* verts, int n_vert, const int32_t* faces, int n_face, const double* K,
                                      const double* Rt, int h, int w, const float* offset3, float scale, double near_,
                                      double far_, int clear, void* state) {
  const char* who = "isr_render_coords_host";
  if (int rc = check_args(who, verts, n_vert, faces, n_face, K, Rt, h, w, offset3, scale, near_, far_, state)) return rc;
  const size_t npix = (size_t)h * w;
  float* item = static_cast<float*>(state);
  int32_t* cnt = reinterpret_cast<int32_t*>(item + 5 * npix);
  rs::Camera cam;
  for (int i = 0; i < 9; ++i) cam.K[i] = K[i];
  for (int i = 0; i < 12; ++i) cam.Rt[i] = Rt[i];
  std::vector<unsigned long long> keys(npix);
  for (size_t p = 0; p < npix; ++p)
    keys[p] = clear ? rs::kEmptyKey : rs::initial_key(0, item[4 * p + 3], item[4 * npix + p]);
  if (clear) cnt[0] = cnt[1] = 0;
  cnt[2] = cnt[3] = 0;
  for (int f = 0; f < n_face; ++f) {
    rs::Face F;
    rs::setup_face(verts, n_vert, faces, f, cam, near_, h, w, &F);
    if (F.status == rs::kFaceDropped) {
      ++cnt[1];
      continue;
    }
    ++cnt[0];
    if (F.status != rs::kFaceOk) continue;
    for (int r = F.r0; r <= F.r1; ++r)
      for (int c = F.c0; c <= F.c1; ++c) {
        unsigned long long key;
        if (rs::fragment_key(F, f, r, c, near_, far_, &key) && key < keys[(size_t)r * w + c]) keys[(size_t)r * w + c] = key;
      }
  }
  int covered = 0;
  for (size_t p = 0; p < npix; ++p)
    covered += rs::resolve_pixel(keys[p], clear ? 1 : 0, verts, n_vert, faces, cam, near_, h, w, offset3, scale, (int)(p / w),
                                 (int)(p % w), item + 4 * p, item + 4 * npix + p);
  cnt[2] = covered;
  return ISR_OK;
}
