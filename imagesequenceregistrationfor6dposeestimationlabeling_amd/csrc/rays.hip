// rays.hip — ray bundles from cameras on the device (rays.hpp states the arithmetic): the entries of include/isr_rays.h.
//
// Everything here is bandwidth- and launch-bound; a ray costs a handful of fmaf (and, for Monte-Carlo rays, Philox rounds).
//   bundle:  one wave per ray.  Every lane computes the ray (the same values in every lane), lanes 0..2 store the origin and
//            the direction, lanes 0..1 the xy, and all 64 lanes store the ray's P lengths, k = lane, lane + 64, ...: a row of
//            lengths is one contiguous run of stores.
//   select:  one thread per candidate ray, workgroups of kThreads consecutive candidates in (camera, ray) order, so that a
//            scan over the threads is a scan in output order (the pattern of mc_extract.hip).
//     count: the candidate's xy, the mask's nearest pixel, a ballot and a popcount per wave, the workgroup's sum to the
//            workspace.
//     scan:  ONE workgroup turns the sums into exclusive offsets, kThreads per pass with a running carry, and writes the
//            count.  The seams between count, scan and emit are kernel boundaries: no workgroup waits for another inside a
//            launch, no atomic, no fence, and the order depends on nothing but the mask.
//     emit:  the flags again (cheaper than storing them), the ballot's prefix gives a kept ray's row; then the wave walks the
//            set bits of its ballot and writes each kept ray as the bundle kernel does, all lanes on one row at a time.
//            Rows from count to cap are written as zeros by the whole grid.
//   sample:  one thread per output value; the channels of a pixel are consecutive lanes.
#include "rays.hpp"
#include "block_prims.hpp"
#include "isr_common.hpp"

#include "../../include/isr_rays.h"

namespace {

using namespace isr::rays;

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / isr::kWave;

struct Out {
  float* origins;
  float* directions;
  float* lengths;
  float* xys;
  int32_t* src;      // null for a bundle
};

struct Plan {
  int32_t* totals;   // {count}
  uint32_t* boff;    // per workgroup: its sum after count, its exclusive offset after scan
  int nb;
};

// One wave writes candidate ray r of camera b to row `row`: every lane must call this with the same (b, r, row).
__device__ __forceinline__ void wave_write_row(const Spec& s, const Cameras& c, int b, int r, long long row, int src, int lane,
                                               const Out& out) {
  float x, y, o[3], d[3];
  candidate_xy(s, c, b, r, x, y);
  ndc_ray(c.R + 9 * (size_t)b, c.T + 3 * (size_t)b, c.intr + 4 * (size_t)b, x, y, o, d);
  if (lane < 3) {
    out.origins[3 * row + lane] = lane == 0 ? o[0] : lane == 1 ? o[1] : o[2];
    out.directions[3 * row + lane] = lane == 0 ? d[0] : lane == 1 ? d[1] : d[2];
  }
  if (lane < 2) out.xys[2 * row + lane] = lane == 0 ? x : y;
  if (out.src && lane == 0) out.src[row] = src;
  float* lrow = out.lengths + row * s.P;
  for (int k = lane; k < s.P; k += isr::kWave) lrow[k] = length_at(s, c, b, r, k);
}

__global__ __launch_bounds__(kThreads) void rays_bundle_kernel(Spec s, Cameras c, Out out) {
  const int lane = threadIdx.x & 63;
  const long long ray = (long long)blockIdx.x * kWaves + (threadIdx.x >> 6);
  if (ray >= (long long)s.B * s.n) return;          // whole waves leave: no barrier follows
  wave_write_row(s, c, (int)(ray / s.n), (int)(ray % s.n), ray, 0, lane, out);
}

// this thread's candidate: is it kept?  (false past the last candidate)
__device__ __forceinline__ bool thread_keeps(const Spec& s, const Cameras& c, const float* __restrict__ mask, int mh, int mw) {
  const long long e = (long long)blockIdx.x * kThreads + threadIdx.x;
  if (e >= (long long)s.B * s.n) return false;
  return candidate_kept(s, c, mask, mh, mw, (int)(e / s.n), (int)(e % s.n));
}

__global__ __launch_bounds__(kThreads) void rays_count_kernel(Spec s, Cameras c, const float* __restrict__ mask, int mh, int mw,
                                                              Plan pl) {
  __shared__ uint32_t sw[kWaves];
  // a flag per thread: a ballot and a popcount per wave stand in for block_prims' scan (rays_emit_kernel needs the ballot itself)
  const unsigned long long m = __ballot(thread_keeps(s, c, mask, mh, mw));
  if ((threadIdx.x & 63) == 0) sw[threadIdx.x >> 6] = (uint32_t)__popcll(m);
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t total = 0;
    for (int w = 0; w < kWaves; ++w) total += sw[w];
    pl.boff[blockIdx.x] = total;
  }
}

__global__ __launch_bounds__(kThreads) void rays_scan_kernel(Plan pl, int32_t* __restrict__ count_dev) {
  __shared__ uint32_t sw[kWaves];
  uint32_t carry = 0;                                // at most 2^28 in all
  for (int base = 0; base < pl.nb; base += kThreads) {
    const int b = base + threadIdx.x;
    const uint32_t x = b < pl.nb ? pl.boff[b] : 0u;
    uint32_t total;
    const uint32_t ex = isr::block_exclusive_scan<kThreads>(x, sw, total);
    __syncthreads();                                 // sw is free for the next pass
    if (b < pl.nb) pl.boff[b] = carry + ex;
    carry += total;
  }
  if (threadIdx.x == 0) pl.totals[0] = count_dev[0] = (int32_t)carry;
}

__global__ __launch_bounds__(kThreads) void rays_emit_kernel(Spec s, Cameras c, const float* __restrict__ mask, int mh, int mw,
                                                             Plan pl, long long cap, Out out) {
  __shared__ uint32_t sw[kWaves];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const unsigned long long m = __ballot(thread_keeps(s, c, mask, mh, mw));
  if (lane == 0) sw[w] = (uint32_t)__popcll(m);
  __syncthreads();
  long long row = pl.boff[blockIdx.x];
  for (int v = 0; v < w; ++v) row += sw[v];
  // the wave's kept rays in lane order: rows row, row + 1, ...; a cap short of the count loses rows, never a write outside
  const long long first = (long long)blockIdx.x * kThreads + w * 64;
  for (unsigned long long rest = m; rest != 0 && row < cap; rest &= rest - 1, ++row) {
    const long long e = first + (__ffsll((long long)rest) - 1);
    wave_write_row(s, c, (int)(e / s.n), (int)(e % s.n), row, (int)e, lane, out);
  }
  // rows from the count to cap (max: a workspace no count has filled cannot make it negative)
  const long long count = max(pl.totals[0], 0);
  const long long tid = (long long)blockIdx.x * kThreads + threadIdx.x, stride = (long long)gridDim.x * kThreads;
  for (long long r = count + tid; r < cap; r += stride) {
    out.origins[3 * r] = out.origins[3 * r + 1] = out.origins[3 * r + 2] = 0.f;
    out.directions[3 * r] = out.directions[3 * r + 1] = out.directions[3 * r + 2] = 0.f;
    out.xys[2 * r] = out.xys[2 * r + 1] = 0.f;
    out.src[r] = 0;
  }
  for (long long i = count * s.P + tid; i < cap * s.P; i += stride) out.lengths[i] = 0.f;
}

__global__ __launch_bounds__(kThreads) void sample_nearest_kernel(const float* __restrict__ images, int H, int W, int C,
                                                                  const float* __restrict__ xys, int n, long long total,
                                                                  float* __restrict__ out) {
  const long long i = (long long)blockIdx.x * kThreads + threadIdx.x;
  if (i >= total) return;
  const long long row = i / C;
  const int ch = (int)(i % C), b = (int)(row / n);
  const int ix = nearest_pixel(xys[2 * row], W), iy = nearest_pixel(xys[2 * row + 1], H);
  out[i] = ix < 0 || iy < 0 ? 0.f : images[(((size_t)b * H + iy) * W + ix) * C + ch];
}

// the arguments every entry shares
#define ISR_RAYS_SPEC_PARAMS                                                                                                  \
  int mode, const float *R, const float *T, const float *intr, const int32_t *camera_ids, int B, int W, int H, int n, int P,  \
      float min_x, float max_x, float min_y, float max_y, float min_depth, float max_depth, int stratified, uint64_t seed
#define ISR_RAYS_SPEC_ARGS mode, R, T, intr, camera_ids, B, W, H, n, P, min_x, max_x, min_y, max_y, min_depth, max_depth, stratified, seed

int check_spec(const char* who, ISR_RAYS_SPEC_PARAMS, Spec& s, Cameras& c) {
  const char* wrong = make_spec(mode, B, W, H, n, P, min_x, max_x, min_y, max_y, min_depth, max_depth, stratified, seed, s);
  ISR_REQUIRE(!wrong, "%s: %s (mode %d, B %d, W %d, H %d, n %d, P %d)", who, wrong, mode, B, W, H, n, P);
  ISR_REQUIRE(R && T && intr, "%s: null camera pointer", who);
  c.R = R;
  c.T = T;
  c.intr = intr;
  c.ids = mode == kMonteCarlo ? camera_ids : nullptr;
  return ISR_OK;
}

int check_mask(const char* who, const float* mask, int mh, int mw) {
  ISR_REQUIRE(mask, "%s: null mask", who);
  ISR_REQUIRE(mh >= 1 && mw >= 1 && (long long)mh * mw <= kMaxRays, "%s: mask %d x %d (each at least 1, at most 2^28 pixels)", who,
              mh, mw);
  return ISR_OK;
}

int check_out(const char* who, int64_t cap, const Out& o) {
  ISR_REQUIRE(cap >= 0 && cap <= kMaxRays, "%s: cap = %lld (0..2^28)", who, (long long)cap);
  ISR_REQUIRE(cap == 0 || (o.origins && o.directions && o.lengths && o.xys && o.src), "%s: null output pointer", who);
  return ISR_OK;
}

int check_sample(const char* who, const float* images, int B, int H, int W, int C, const float* xys, int n, const float* out) {
  ISR_REQUIRE(B >= 1 && H >= 1 && W >= 1 && n >= 1, "%s: B = %d, H = %d, W = %d, n = %d (each at least 1)", who, B, H, W, n);
  ISR_REQUIRE(C >= 1 && C <= kMaxChannels, "%s: C = %d (1..%d)", who, C, kMaxChannels);
  ISR_REQUIRE((long long)B * n <= kMaxRays && (long long)B * n * C < (1ll << 31), "%s: B * n = %lld > 2^28 or B * n * C >= 2^31", who,
              (long long)B * n);
  ISR_REQUIRE((long long)H * W <= kMaxRays, "%s: image %d x %d has more than 2^28 pixels", who, H, W);
  ISR_REQUIRE(images && xys && out, "%s: null pointer", who);
  return ISR_OK;
}

size_t carve(isr::Workspace& ws, long long N, Plan& pl) {
  pl.nb = (int)((N + kThreads - 1) / kThreads);
  pl.totals = ws.take<int32_t>(2);
  pl.boff = ws.take<uint32_t>((size_t)pl.nb);
  return ws.off;
}

}  // namespace

extern "C" size_t isr_rays_workspace_bytes(int B, int n) {
  if (B < 1 || n < 1 || (long long)B * n > kMaxRays) {
    isr::set_error("isr_rays_workspace_bytes: B = %d, n = %d (each at least 1, B * n at most 2^28)", B, n);
    return 0;
  }
  isr::Workspace ws(nullptr, 0);
  Plan pl;
  return carve(ws, (long long)B * n, pl);
}

extern "C" int isr_rays_bundle(ISR_RAYS_SPEC_PARAMS, float* origins, float* directions, float* lengths, float* xys,
                               isr_stream_t stream) {
  Spec s;
  Cameras c;
  if (int rc = check_spec("isr_rays_bundle", ISR_RAYS_SPEC_ARGS, s, c)) return rc;
  ISR_REQUIRE(origins && directions && lengths && xys, "isr_rays_bundle: null output pointer");
  const Out out{origins, directions, lengths, xys, nullptr};
  const long long N = (long long)s.B * s.n;
  rays_bundle_kernel<<<(unsigned)((N + kWaves - 1) / kWaves), kThreads, 0, isr::as_stream(stream)>>>(s, c, out);
  ISR_CHECK_LAUNCH("rays_bundle_kernel");
  return ISR_OK;
}

extern "C" int isr_rays_bundle_host(ISR_RAYS_SPEC_PARAMS, float* origins, float* directions, float* lengths, float* xys) {
  Spec s;
  Cameras c;
  if (int rc = check_spec("isr_rays_bundle_host", ISR_RAYS_SPEC_ARGS, s, c)) return rc;
  ISR_REQUIRE(origins && directions && lengths && xys, "isr_rays_bundle_host: null output pointer");
  bundle_host(s, c, origins, directions, lengths, xys);
  return ISR_OK;
}

extern "C" int isr_rays_select_count(ISR_RAYS_SPEC_PARAMS, const float* mask, int mh, int mw, int32_t* count_dev, void* ws_ptr,
                                     size_t ws_bytes, isr_stream_t stream) {
  Spec s;
  Cameras c;
  if (int rc = check_spec("isr_rays_select_count", ISR_RAYS_SPEC_ARGS, s, c)) return rc;
  if (int rc = check_mask("isr_rays_select_count", mask, mh, mw)) return rc;
  ISR_REQUIRE(count_dev && ws_ptr, "isr_rays_select_count: null count_dev or workspace");
  isr::Workspace ws(ws_ptr, ws_bytes);
  Plan pl;
  carve(ws, (long long)s.B * s.n, pl);
  ISR_REQUIRE(ws.ok(), "isr_rays_select_count: workspace %zu bytes, needs %zu", ws_bytes, ws.off);
  hipStream_t st = isr::as_stream(stream);
  rays_count_kernel<<<pl.nb, kThreads, 0, st>>>(s, c, mask, mh, mw, pl);
  ISR_CHECK_LAUNCH("rays_count_kernel");
  rays_scan_kernel<<<1, kThreads, 0, st>>>(pl, count_dev);
  ISR_CHECK_LAUNCH("rays_scan_kernel");
  return ISR_OK;
}

extern "C" int isr_rays_select_emit(ISR_RAYS_SPEC_PARAMS, const float* mask, int mh, int mw, const void* ws_ptr, size_t ws_bytes,
                                    int64_t cap, float* origins, float* directions, float* lengths, float* xys, int32_t* src,
                                    isr_stream_t stream) {
  Spec s;
  Cameras c;
  if (int rc = check_spec("isr_rays_select_emit", ISR_RAYS_SPEC_ARGS, s, c)) return rc;
  if (int rc = check_mask("isr_rays_select_emit", mask, mh, mw)) return rc;
  const Out out{origins, directions, lengths, xys, src};
  if (int rc = check_out("isr_rays_select_emit", cap, out)) return rc;
  ISR_REQUIRE(ws_ptr, "isr_rays_select_emit: null workspace");
  isr::Workspace ws(const_cast<void*>(ws_ptr), ws_bytes);
  Plan pl;
  carve(ws, (long long)s.B * s.n, pl);
  ISR_REQUIRE(ws.ok(), "isr_rays_select_emit: workspace %zu bytes, needs %zu", ws_bytes, ws.off);
  if (cap == 0) return ISR_OK;
  rays_emit_kernel<<<pl.nb, kThreads, 0, isr::as_stream(stream)>>>(s, c, mask, mh, mw, pl, (long long)cap, out);
  ISR_CHECK_LAUNCH("rays_emit_kernel");
  return ISR_OK;
}

extern "C" int isr_rays_select_count_host(ISR_RAYS_SPEC_PARAMS, const float* mask, int mh, int mw, int32_t* count) {
  Spec s;
  Cameras c;
  if (int rc = check_spec("isr_rays_select_count_host", ISR_RAYS_SPEC_ARGS, s, c)) return rc;
  if (int rc = check_mask("isr_rays_select_count_host", mask, mh, mw)) return rc;
  ISR_REQUIRE(count, "isr_rays_select_count_host: null count");
  count[0] = (int32_t)select_count_host(s, c, mask, mh, mw);
  return ISR_OK;
}

extern "C" int isr_rays_select_emit_host(ISR_RAYS_SPEC_PARAMS, const float* mask, int mh, int mw, int64_t cap, float* origins,
                                         float* directions, float* lengths, float* xys, int32_t* src) {
  Spec s;
  Cameras c;
  if (int rc = check_spec("isr_rays_select_emit_host", ISR_RAYS_SPEC_ARGS, s, c)) return rc;
  if (int rc = check_mask("isr_rays_select_emit_host", mask, mh, mw)) return rc;
  const Out out{origins, directions, lengths, xys, src};
  if (int rc = check_out("isr_rays_select_emit_host", cap, out)) return rc;
  select_emit_host(s, c, mask, mh, mw, cap, origins, directions, lengths, xys, src);
  return ISR_OK;
}

extern "C" int isr_sample_nearest(const float* images, int B, int H, int W, int C, const float* xys, int n, float* out,
                                  isr_stream_t stream) {
  if (int rc = check_sample("isr_sample_nearest", images, B, H, W, C, xys, n, out)) return rc;
  const long long total = (long long)B * n * C;
  sample_nearest_kernel<<<(unsigned)((total + kThreads - 1) / kThreads), kThreads, 0, isr::as_stream(stream)>>>(images, H, W, C, xys,
                                                                                                              n, total, out);
  ISR_CHECK_LAUNCH("sample_nearest_kernel");
  return ISR_OK;
}

extern "C" int isr_sample_nearest_host(const float* images, int B, int H, int W, int C, const float* xys, int n, float* out) {
  if (int rc = check_sample("isr_sample_nearest_host", images, B, H, W, C, xys, n, out)) return rc;
  sample_nearest_host(images, B, H, W, C, xys, n, out);
  return ISR_OK;
}

extern "C" int isr_rays_philox_host(const uint32_t* counter, const uint32_t* key, uint32_t* words, float* units) {
  ISR_REQUIRE(counter && key && words, "isr_rays_philox_host: null pointer");
  isr::philox4x32_10(counter[0], counter[1], counter[2], counter[3], key[0], key[1], words);
  if (units)
    for (int i = 0; i < 4; ++i) units[i] = isr::unit_float(words[i]);
  return ISR_OK;
}
