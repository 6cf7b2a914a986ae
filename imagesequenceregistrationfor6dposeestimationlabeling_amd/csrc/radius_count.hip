// radius_count.hip — the fixed-radius neighbour count (radius_count.hpp states the rule and the grid): the entries of
// include/isr_radius.h.
//
// Six launches on the caller's stream, no host synchronise, nothing read back:
//   bounds_init, bounds:  the cloud's bounding box, integer atomicMin / atomicMax on the order-preserving image of the floats;
//   grid:                 every workgroup makes the Grid from the box (the same f64 arithmetic, so the same Grid), workgroup 0
//                         stores it, and all of them zero the histogram of the cells this Grid has;
//   histogram:            a point's cell, kept per point, and an integer atomicAdd on the cell's counter;
//   scan:                 one workgroup: the exclusive scan of the histogram -> start, and end = start;
//   scatter:              sorted[atomicAdd(end[cell])] = point, after which end[c] is where cell c ends;
//   count:                one lane per point, radius::count_point over its 27 cells.
// The order inside a cell depends on the atomics; the counts do not (radius_count.hpp).  No float atomics.
#include "radius_count.hpp"
#include "block_prims.hpp"
#include "isr_common.hpp"

#include "../../include/isr_radius.h"

#include <cfloat>
#include <cmath>
#include <vector>

namespace {

using namespace isr::radius;

constexpr int kThreads = 256;
constexpr int kScanThreads = 1024;
constexpr int kBoundsBlocks = 1024;

struct Plan {
  uint32_t* box;       // 6: ordered bits of the minimum x, y, z and of the maximum
  Grid* grid;
  int32_t* start;      // kMaxCells
  int32_t* end;        // kMaxCells
  int32_t* cell;       // N
  float* sorted;       // 3 N
};

__device__ __forceinline__ float from_ordered(uint32_t u) {
  const uint32_t b = (u & 0x80000000u) ? u ^ 0x80000000u : ~u;
  return __uint_as_float(b);
}

__global__ void radius_bounds_init_kernel(Plan p) {
  if (threadIdx.x < 6) p.box[threadIdx.x] = threadIdx.x < 3 ? 0xFFFFFFFFu : 0u;
}

__global__ __launch_bounds__(kThreads) void radius_bounds_kernel(Plan p, const float* __restrict__ pts, int N) {
  float mn[3] = {INFINITY, INFINITY, INFINITY}, mx[3] = {-INFINITY, -INFINITY, -INFINITY};
  for (long i = (long)blockIdx.x * kThreads + threadIdx.x; i < N; i += (long)gridDim.x * kThreads)
    for (int d = 0; d < 3; ++d) {
      const float v = pts[3 * i + d];
      mn[d] = fminf(mn[d], v);
      mx[d] = fmaxf(mx[d], v);
    }
  for (int d = 0; d < 3; ++d) {
    mn[d] = isr::wave_reduce(mn[d], isr::Min{});
    mx[d] = isr::wave_reduce(mx[d], isr::Max{});
    if ((threadIdx.x & 63) == 0) {
      atomicMin(&p.box[d], isr::ordered_bits(mn[d]));
      atomicMax(&p.box[3 + d], isr::ordered_bits(mx[d]));
    }
  }
}

__global__ __launch_bounds__(kThreads) void radius_grid_kernel(Plan p, float r) {
  __shared__ Grid g;
  if (threadIdx.x == 0) {
    float mn[3], mx[3];
    for (int d = 0; d < 3; ++d) {
      mn[d] = from_ordered(p.box[d]);
      mx[d] = from_ordered(p.box[3 + d]);
    }
    make_grid(mn, mx, r, g);
    if (blockIdx.x == 0) *p.grid = g;
  }
  __syncthreads();
  const int c = blockIdx.x * kThreads + threadIdx.x;      // the launch covers kMaxCells
  if (c < g.cells) p.end[c] = 0;
}

__global__ __launch_bounds__(kThreads) void radius_histogram_kernel(Plan p, const float* __restrict__ pts, int N) {
  const long i = (long)blockIdx.x * kThreads + threadIdx.x;
  if (i >= N) return;
  const Grid g = *p.grid;
  const int c = cell_of(g, pts[3 * i], pts[3 * i + 1], pts[3 * i + 2]);
  p.cell[i] = c;
  atomicAdd(&p.end[c], 1);
}

__global__ __launch_bounds__(kScanThreads) void radius_scan_kernel(Plan p) {
  __shared__ int sums[kScanThreads];
  const int cells = p.grid->cells;
  const int chunk = (cells + kScanThreads - 1) / kScanThreads;
  const int c0 = min(threadIdx.x * chunk, cells), c1 = min(c0 + chunk, cells);
  int s = 0;
  for (int c = c0; c < c1; ++c) s += p.end[c];
  sums[threadIdx.x] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    int run = 0;
    for (int t = 0; t < kScanThreads; ++t) {
      const int v = sums[t];
      sums[t] = run;
      run += v;
    }
  }
  __syncthreads();
  int run = sums[threadIdx.x];
  for (int c = c0; c < c1; ++c) {
    const int v = p.end[c];
    p.start[c] = run;
    p.end[c] = run;
    run += v;
  }
}

__global__ __launch_bounds__(kThreads) void radius_scatter_kernel(Plan p, const float* __restrict__ pts, int N) {
  const long i = (long)blockIdx.x * kThreads + threadIdx.x;
  if (i >= N) return;
  const long j = atomicAdd(&p.end[p.cell[i]], 1);
  for (int d = 0; d < 3; ++d) p.sorted[3 * j + d] = pts[3 * i + d];
}

__global__ __launch_bounds__(kThreads) void radius_count_kernel(Plan p, const float* __restrict__ pts, int N, float r2, int cap,
                                                                int32_t* __restrict__ counts) {
  const long i = (long)blockIdx.x * kThreads + threadIdx.x;
  if (i >= N) return;
  const Grid g = *p.grid;
  counts[i] = count_point(g, p.sorted, p.start, p.end, pts[3 * i], pts[3 * i + 1], pts[3 * i + 2], r2, cap);
}

size_t carve(isr::Workspace& ws, int N, Plan& p) {
  p.box = ws.take<uint32_t>(6);
  p.grid = ws.take<Grid>(1);
  p.start = ws.take<int32_t>(kMaxCells);
  p.end = ws.take<int32_t>(kMaxCells);
  p.cell = ws.take<int32_t>((size_t)N);
  p.sorted = ws.take<float>(3 * (size_t)N);
  return ws.off;
}

int check_count(const char* who, const float* pts, int N, double radius, const int32_t* counts, float& r) {
  ISR_REQUIRE(N >= 1 && N <= kMaxPoints, "%s: N = %d (1..%d)", who, N, kMaxPoints);
  ISR_REQUIRE(pts && counts, "%s: null pointer", who);
  r = (float)radius;
  ISR_REQUIRE(std::isfinite(radius) && std::isfinite(r) && r > 0.f && r * r >= FLT_MIN,
              "%s: radius = %g must be finite and positive, its f32 square a normal number", who, radius);
  return ISR_OK;
}

}  // namespace

extern "C" size_t isr_radius_workspace_bytes(int N) {
  if (N < 1 || N > kMaxPoints) {
    isr::set_error("isr_radius_workspace_bytes: N = %d (1..%d)", N, kMaxPoints);
    return 0;
  }
  isr::Workspace ws(nullptr, 0);
  Plan p;
  return carve(ws, N, p);
}

extern "C" int isr_radius_count(const float* pts, int N, double radius, int cap, int32_t* counts, void* ws_ptr, size_t ws_bytes,
                                isr_stream_t stream) {
  float r;
  if (int rc = check_count("isr_radius_count", pts, N, radius, counts, r)) return rc;
  ISR_REQUIRE(ws_ptr, "isr_radius_count: null workspace");
  isr::Workspace ws(ws_ptr, ws_bytes);
  Plan p;
  carve(ws, N, p);
  ISR_REQUIRE(ws.ok(), "isr_radius_count: workspace %zu bytes, needs %zu", ws_bytes, ws.off);
  hipStream_t st = isr::as_stream(stream);
  const unsigned rows = (unsigned)(((long)N + kThreads - 1) / kThreads);
  radius_bounds_init_kernel<<<1, 64, 0, st>>>(p);
  radius_bounds_kernel<<<rows < (unsigned)kBoundsBlocks ? rows : (unsigned)kBoundsBlocks, kThreads, 0, st>>>(p, pts, N);
  radius_grid_kernel<<<kMaxCells / kThreads, kThreads, 0, st>>>(p, r);
  radius_histogram_kernel<<<rows, kThreads, 0, st>>>(p, pts, N);
  radius_scan_kernel<<<1, kScanThreads, 0, st>>>(p);
  radius_scatter_kernel<<<rows, kThreads, 0, st>>>(p, pts, N);
  radius_count_kernel<<<rows, kThreads, 0, st>>>(p, pts, N, r * r, cap, counts);
  ISR_CHECK_LAUNCH("radius_count kernels");
  return ISR_OK;
}

extern "C" int isr_radius_count_host(const float* pts, int N, double radius, int cap, int32_t* counts) {
  float r;
  if (int rc = check_count("isr_radius_count_host", pts, N, radius, counts, r)) return rc;
  std::vector<float> sorted(3 * (size_t)N);
  std::vector<int32_t> start(kMaxCells), end(kMaxCells);
  count_host(pts, N, r, cap, counts, sorted.data(), start.data(), end.data());
  return ISR_OK;
}
