// mc_extract.hip — iso-surface extraction on the device (mc_extract.hpp states the arithmetic and the order): the entries of
// include/isr_mc.h.
//
// One thread per grid point, workgroups of kThreads consecutive points in linear order, so that a scan over the threads is
// a scan in output order.  A cell is tallied by the thread of its grid point: the cells' linear order over
// (nx-1, ny-1, nz-1) is the order of their points.
//   tally:  a thread loads the four k-rows its cell touches at its own k — vol[p], vol[p + ny nz], vol[p + nz] and
//           vol[p + ny nz + nz], each contiguous over the lanes of a wave — into LDS and takes the k + 1 values from its
//           neighbour's slots (the last thread loads the one column past the workgroup): eight corners from four coalesced
//           loads.  From them the point's crossing flags and the cell's case.
//   count:  tally, then an exclusive scan of (vertices, triangles) over the workgroup (block_prims.hpp: lanes by shuffle, waves through
//           LDS); every point's slot word — its first vertex within the workgroup and the flags of axes 0 and 1, which is
//           all a triangle corner needs to find a vertex id — and the workgroup's sums go to the workspace.
//   scan:   ONE workgroup turns the sums into exclusive offsets, kThreads of them per pass with a running carry, and writes
//           the totals.  The seams between count, scan and emit are kernel boundaries: no workgroup waits for another
//           inside a launch, no atomic, no fence, and nothing depends on how many workgroups are resident.
//   emit:   tally and the same workgroup scan again (8 bytes of volume per point are cheaper than keeping every point's two
//           offsets), + the workgroup's offsets: vertices to their slots, and every triangle corner resolved through the
//           slot word of the edge's owner and the offset of the owner's workgroup.
#include "mc_extract.hpp"
#include "block_prims.hpp"
#include "isr_common.hpp"

#include "../../include/isr_mc.h"

#include <vector>

namespace {

using namespace isr::mc;

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / isr::kWave;
// a workgroup's sums fit the halves of one 32-bit word, a point's first vertex and two flags fit 16 bits
static_assert(3 * kThreads < (1 << 14) && kMaxTris * kThreads < (1 << 16), "packed counts");

struct Grid {
  int nx, ny, nz, N;
  float iso;
};

struct Plan {
  uint16_t* slot;    // N: (the point's first vertex within its workgroup) << 2 | flags of axes 0 and 1
  uint64_t* boff;    // per workgroup: its sums after count, its exclusive offsets after scan; vertices low, triangles high
  int32_t* totals;   // {V, F}
  int nb;
};

struct Tally {
  float c[8];        // the cell's corners; c[0] the point's own value, c[1] / c[2] / c[4] its +x / +y / +z neighbours
  int p, i, j, k;
  int flags, cs, ntri;
  bool in;
};

// s: 4 rows of kThreads + 1 floats.  Every thread of the workgroup must call this.
__device__ __forceinline__ void tally(const float* __restrict__ vol, const Grid& g, float (*s)[kThreads + 1], Tally& t) {
  const int tid = threadIdx.x;
  const int p = blockIdx.x * kThreads + tid;
  const int sj = g.nz, si = g.ny * g.nz;
  t.p = p;
  t.in = p < g.N;
  t.k = p % g.nz;
  const int r = p / g.nz;
  t.j = r % g.ny;
  t.i = r / g.ny;
  const bool hx = t.in && t.i + 1 < g.nx, hy = t.in && t.j + 1 < g.ny, hz = t.in && t.k + 1 < g.nz;
  // row di + 2 dj; a row that does not exist holds 0 and is not used (hx, hy and hz gate every use)
  s[0][tid] = t.in ? vol[p] : 0.f;
  s[1][tid] = hx ? vol[p + si] : 0.f;
  s[2][tid] = hy ? vol[p + sj] : 0.f;
  s[3][tid] = hx && hy ? vol[p + si + sj] : 0.f;
  if (tid == kThreads - 1) {      // hz: p + 1 is (i, j, k + 1), inside the volume, and its rows exist where this thread's do
    s[0][kThreads] = hz ? vol[p + 1] : 0.f;
    s[1][kThreads] = hz && hx ? vol[p + si + 1] : 0.f;
    s[2][kThreads] = hz && hy ? vol[p + sj + 1] : 0.f;
    s[3][kThreads] = hz && hx && hy ? vol[p + si + sj + 1] : 0.f;
  }
  __syncthreads();
#pragma unroll
  for (int b = 0; b < 8; ++b) t.c[b] = s[b & 3][tid + (b >> 2)];
  t.flags = point_flags(t.c[0], t.c[1], t.c[2], t.c[4], hx, hy, hz, g.iso);
  t.cs = hx && hy && hz ? case_index(t.c, g.iso) : 0;
  t.ntri = tri_count(t.cs);
}

__device__ __forceinline__ uint32_t packed_counts(const Tally& t) { return (uint32_t)flag_count(t.flags) | (uint32_t)t.ntri << 16; }

__global__ __launch_bounds__(kThreads) void mc_count_kernel(const float* __restrict__ vol, Grid g, Plan pl) {
  __shared__ float s[4][kThreads + 1];
  __shared__ uint32_t sw[kWaves];
  Tally t;
  tally(vol, g, s, t);
  uint32_t total;
  const uint32_t ex = isr::block_exclusive_scan<kThreads>(packed_counts(t), sw, total);
  if (t.in) pl.slot[t.p] = (uint16_t)((ex & 0xffffu) << 2 | (uint32_t)(t.flags & 3));
  if (threadIdx.x == 0) pl.boff[blockIdx.x] = (uint64_t)(total & 0xffffu) | (uint64_t)(total >> 16) << 32;
}

__global__ __launch_bounds__(kThreads) void mc_scan_kernel(Plan pl, int32_t* __restrict__ counts_dev) {
  __shared__ unsigned long long sw[kWaves];
  unsigned long long carry = 0;   // vertices < 2^30 in the low half never carry into the triangles
  for (int base = 0; base < pl.nb; base += kThreads) {
    const int b = base + threadIdx.x;
    const unsigned long long x = b < pl.nb ? pl.boff[b] : 0ull;
    unsigned long long total;
    const unsigned long long ex = isr::block_exclusive_scan<kThreads>(x, sw, total);
    __syncthreads();              // sw is free for the next pass
    if (b < pl.nb) pl.boff[b] = carry + ex;
    carry += total;
  }
  if (threadIdx.x == 0) {
    pl.totals[0] = counts_dev[0] = (int32_t)(uint32_t)carry;
    pl.totals[1] = counts_dev[1] = (int32_t)(carry >> 32);
  }
}

__global__ __launch_bounds__(kThreads) void mc_emit_kernel(const float* __restrict__ vol, Grid g, Plan pl, double* __restrict__ verts,
                                                           long long V, int32_t* __restrict__ tris, long long F) {
  __shared__ float s[4][kThreads + 1];
  __shared__ uint32_t sw[kWaves];
  Tally t;
  tally(vol, g, s, t);
  uint32_t total;
  const uint32_t ex = isr::block_exclusive_scan<kThreads>(packed_counts(t), sw, total);
  const uint64_t bo = pl.boff[blockIdx.x];
  const long long v0 = (long long)(uint32_t)bo + (ex & 0xffffu);
  const long long f0 = (long long)(bo >> 32) + (ex >> 16);
  const int sj = g.nz, si = g.ny * g.nz;

  // slots below V and F only: a caller's V or F short of the totals loses rows, it never gets a write past its buffers
#pragma unroll
  for (int a = 0; a < 3; ++a)
    if (t.flags >> a & 1) {
      const long long slot = v0 + axis_rank(t.flags, a);
      if (slot < V) {
        const double along = interp(t.c[0], t.c[1 << a], g.iso);
        double* o = verts + 3 * slot;
        o[0] = a == 0 ? t.i + along : (double)t.i;
        o[1] = a == 1 ? t.j + along : (double)t.j;
        o[2] = a == 2 ? t.k + along : (double)t.k;
      }
    }
  for (int n = 0; n < t.ntri && f0 + n < F; ++n) {     // ntri > 0: the cell exists, so every owner below is inside the volume
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const int e = kTriEdges[t.cs][3 * n + c];
      int di, dj, dk;
      edge_owner(e, di, dj, dk);
      const int q = t.p + di * si + dj * sj + dk;
      const uint32_t w = pl.slot[q];
      tris[3 * (f0 + n) + c] = (int32_t)((uint32_t)pl.boff[q / kThreads] + (w >> 2) + (uint32_t)axis_rank((int)(w & 3), edge_axis(e)));
    }
  }
  // rows past the totals, where the caller's buffers are longer (max: a workspace no count has filled cannot make r negative)
  const long long stride = (long long)gridDim.x * kThreads;
  for (long long r = max(pl.totals[0], 0) + (long long)t.p; r < V; r += stride) verts[3 * r] = verts[3 * r + 1] = verts[3 * r + 2] = 0.0;
  for (long long r = max(pl.totals[1], 0) + (long long)t.p; r < F; r += stride) tris[3 * r] = tris[3 * r + 1] = tris[3 * r + 2] = -1;
}

int check_volume(const char* who, const float* vol, int nx, int ny, int nz, float iso) {
  ISR_REQUIRE(vol, "%s: null vol", who);
  ISR_REQUIRE(nx >= kMinDim && nx <= kMaxDim && ny >= kMinDim && ny <= kMaxDim && nz >= kMinDim && nz <= kMaxDim,
              "%s: volume %d x %d x %d (every dimension %d..%d)", who, nx, ny, nz, kMinDim, kMaxDim);
  ISR_REQUIRE((long long)nx * ny * nz <= kMaxPoints, "%s: volume %d x %d x %d has more than 2^28 points", who, nx, ny, nz);
  ISR_REQUIRE(iso == iso, "%s: iso is NaN", who);
  return ISR_OK;
}

int check_outputs(const char* who, const double* verts, int64_t V, const int32_t* tris, int64_t F) {
  ISR_REQUIRE(V >= 0 && F >= 0, "%s: V = %lld, F = %lld", who, (long long)V, (long long)F);
  ISR_REQUIRE((verts || V == 0) && (tris || F == 0), "%s: null verts or tris", who);
  return ISR_OK;
}

size_t carve(isr::Workspace& ws, int nx, int ny, int nz, Grid& g, Plan& pl) {
  g.nx = nx, g.ny = ny, g.nz = nz, g.N = nx * ny * nz;
  pl.nb = (g.N + kThreads - 1) / kThreads;
  pl.totals = ws.take<int32_t>(2);
  pl.boff = ws.take<uint64_t>((size_t)pl.nb);
  pl.slot = ws.take<uint16_t>((size_t)g.N);
  return ws.off;
}

void fill_tail(double* verts, int64_t V, int64_t nv, int32_t* tris, int64_t F, int64_t nf) {
  for (int64_t r = 3 * nv; r < 3 * V; ++r) verts[r] = 0.0;
  for (int64_t r = 3 * nf; r < 3 * F; ++r) tris[r] = -1;
}

}  // namespace

extern "C" size_t isr_mc_workspace_bytes(int nx, int ny, int nz) {
  const float dummy = 0.f;
  if (check_volume("isr_mc_workspace_bytes", &dummy, nx, ny, nz, 0.f)) return 0;
  isr::Workspace ws(nullptr, 0);
  Grid g;
  Plan pl;
  return carve(ws, nx, ny, nz, g, pl);
}

extern "C" int isr_mc_count(const float* vol, int nx, int ny, int nz, float iso, int32_t* counts_dev, void* ws_ptr,
                            size_t ws_bytes, isr_stream_t stream) {
  if (int rc = check_volume("isr_mc_count", vol, nx, ny, nz, iso)) return rc;
  ISR_REQUIRE(counts_dev && ws_ptr, "isr_mc_count: null counts_dev or workspace");
  isr::Workspace ws(ws_ptr, ws_bytes);
  Grid g;
  Plan pl;
  carve(ws, nx, ny, nz, g, pl);
  ISR_REQUIRE(ws.ok(), "isr_mc_count: workspace %zu bytes, needs %zu", ws_bytes, ws.off);
  g.iso = iso;
  hipStream_t st = isr::as_stream(stream);
  mc_count_kernel<<<pl.nb, kThreads, 0, st>>>(vol, g, pl);
  ISR_CHECK_LAUNCH("mc_count_kernel");
  mc_scan_kernel<<<1, kThreads, 0, st>>>(pl, counts_dev);
  ISR_CHECK_LAUNCH("mc_scan_kernel");
  return ISR_OK;
}

extern "C" int isr_mc_emit(const float* vol, int nx, int ny, int nz, float iso, const void* ws_ptr, size_t ws_bytes,
                           double* verts, int64_t V, int32_t* tris, int64_t F, isr_stream_t stream) {
  if (int rc = check_volume("isr_mc_emit", vol, nx, ny, nz, iso)) return rc;
  if (int rc = check_outputs("isr_mc_emit", verts, V, tris, F)) return rc;
  ISR_REQUIRE(ws_ptr, "isr_mc_emit: null workspace");
  isr::Workspace ws(const_cast<void*>(ws_ptr), ws_bytes);
  Grid g;
  Plan pl;
  carve(ws, nx, ny, nz, g, pl);
  ISR_REQUIRE(ws.ok(), "isr_mc_emit: workspace %zu bytes, needs %zu", ws_bytes, ws.off);
  g.iso = iso;
  mc_emit_kernel<<<pl.nb, kThreads, 0, isr::as_stream(stream)>>>(vol, g, pl, verts, (long long)V, tris, (long long)F);
  ISR_CHECK_LAUNCH("mc_emit_kernel");
  return ISR_OK;
}

extern "C" int isr_mc_count_host(const float* vol, int nx, int ny, int nz, float iso, int32_t* counts) {
  if (int rc = check_volume("isr_mc_count_host", vol, nx, ny, nz, iso)) return rc;
  ISR_REQUIRE(counts, "isr_mc_count_host: null counts");
  int64_t nv, nf;
  count_host(vol, nx, ny, nz, iso, nullptr, nv, nf);
  counts[0] = (int32_t)nv;
  counts[1] = (int32_t)nf;
  return ISR_OK;
}

extern "C" int isr_mc_emit_host(const float* vol, int nx, int ny, int nz, float iso, double* verts, int64_t V, int32_t* tris,
                                int64_t F) {
  if (int rc = check_volume("isr_mc_emit_host", vol, nx, ny, nz, iso)) return rc;
  if (int rc = check_outputs("isr_mc_emit_host", verts, V, tris, F)) return rc;
  std::vector<int32_t> first((size_t)nx * ny * nz);
  int64_t nv, nf;
  count_host(vol, nx, ny, nz, iso, first.data(), nv, nf);
  ISR_REQUIRE(V >= nv && F >= nf, "isr_mc_emit_host: V = %lld, F = %lld, the volume gives %lld and %lld", (long long)V,
              (long long)F, (long long)nv, (long long)nf);
  emit_host(vol, nx, ny, nz, iso, first.data(), verts, tris);
  fill_tail(verts, V, nv, tris, F, nf);
  return ISR_OK;
}
