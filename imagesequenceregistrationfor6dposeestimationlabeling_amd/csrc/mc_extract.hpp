// mc_extract.hpp — iso-surface extraction (marching cubes), its arithmetic and its order stated once and compiled for host and
// device.  csrc/mc_extract.hip holds the kernels and the C entries (include/isr_mc.h); a plain C++ compiler can include this
// header too (tools/mc_host_check.cpp).  The case table is csrc/mc_table.hpp, written by tools/gen_mc_table.py.
//
// vol (nx, ny, nz) f32 in C order, iso f32.  A corner is BELOW when v < iso and above otherwise (a NaN is above).
//   vertices:  grid point p = (i, j, k) owns its +x, +y and +z edges where those exist.  An owned edge carries one vertex when
//              exactly one of its ends is below, at  owner coordinate + (f64(iso) - f64(va)) / (f64(vb) - f64(va))  along the
//              edge's axis (va: the owner's value; two f64 subtractions, one division), the other two coordinates the integers:
//              index space, f64.  Ordered by the owner's linear index (i * ny + j) * nz + k, then by axis 0, 1, 2.
//   triangles: per cell, in the order of the cell's linear index over (nx-1, ny-1, nz-1), the rows of the case table in table
//              order; a corner is the id of the vertex on that cube edge = first id of the edge's owner + the rank of the
//              edge's axis among the owner's crossing edges.
// The result is a function of (vol, iso) only.  Finite values are a precondition for a meaningful surface; whatever the
// values are, counting and emitting use the same predicate (`below`).
#pragma once
#include <cstddef>
#include <cstdint>

#include "mc_table.hpp"

#include "hd.hpp"

namespace isr {
namespace mc {

constexpr int kMinDim = 2, kMaxDim = 1024;
constexpr long long kMaxPoints = 1ll << 28;
constexpr int kMaxTris = ISR_MC_MAX_TRIS;                  // of one cell
// ids and counts stay inside int32: at most 3 vertices per point and kMaxTris triangles per cell
static_assert(3 * kMaxPoints < (1ll << 30) && kMaxTris * kMaxPoints < (1ll << 31), "int32 ids");

constexpr uint8_t kTriCount[256] = {ISR_MC_TRI_COUNTS};
constexpr int8_t kTriEdges[256][3 * kMaxTris] = {ISR_MC_TRI_EDGES};

ISR_HD bool below(float v, float iso) { return v < iso; }

// the case of a cell from its eight corner values, c[b] at offset (b & 1, (b >> 1) & 1, (b >> 2) & 1)
ISR_HD int case_index(const float* c, float iso) {
  int m = 0;
  for (int b = 0; b < 8; ++b) m |= (int)below(c[b], iso) << b;
  return m;
}

// triangles of a case; the two uniform cases are answered without the table (most cells of a volume)
ISR_HD int tri_count(int cs) { return (cs == 0 || cs == 255) ? 0 : kTriCount[cs]; }

// bit a: the point's +axis-a edge exists (has[a]) and carries a vertex.  va: the point's value, vx / vy / vz: its +x / +y / +z
// neighbours' (not read where the edge does not exist)
ISR_HD int point_flags(float va, float vx, float vy, float vz, bool hasx, bool hasy, bool hasz, float iso) {
  const bool b = below(va, iso);
  return (int)(hasx && below(vx, iso) != b) | (int)(hasy && below(vy, iso) != b) << 1 | (int)(hasz && below(vz, iso) != b) << 2;
}
ISR_HD int flag_count(int flags) { return (flags & 1) + (flags >> 1 & 1) + (flags >> 2 & 1); }
// rank of axis a among the crossing edges of a point with these flags (only bits below a are read)
ISR_HD int axis_rank(int flags, int axis) { return (axis >= 1 ? flags & 1 : 0) + (axis == 2 ? flags >> 1 & 1 : 0); }

// where on an edge the vertex sits, from the owner's end
ISR_HD double interp(float va, float vb, float iso) { return ((double)iso - (double)va) / ((double)vb - (double)va); }

// cube edge e = 4 * axis + idx: its axis, and its owner's offset from the cell's grid point
ISR_HD int edge_axis(int e) { return e >> 2; }
ISR_HD void edge_owner(int e, int& di, int& dj, int& dk) {
  const int a = e >> 2, u = e & 1, v = e >> 1 & 1;
  di = a == 0 ? 0 : u;
  dj = a == 0 ? u : (a == 1 ? 0 : v);
  dk = a == 2 ? 0 : v;
}

// The definition as plain loops.  first (N) receives every point's first vertex id; -> the vertex and triangle totals.
inline void count_host(const float* vol, int nx, int ny, int nz, float iso, int32_t* first, int64_t& V, int64_t& F) {
  V = F = 0;
  const size_t sj = (size_t)nz, si = (size_t)ny * nz;
  for (int i = 0; i < nx; ++i)
    for (int j = 0; j < ny; ++j)
      for (int k = 0; k < nz; ++k) {
        const size_t p = i * si + j * sj + k;
        const bool hx = i + 1 < nx, hy = j + 1 < ny, hz = k + 1 < nz;
        if (first) first[p] = (int32_t)V;
        V += flag_count(point_flags(vol[p], hx ? vol[p + si] : 0.f, hy ? vol[p + sj] : 0.f, hz ? vol[p + 1] : 0.f, hx, hy, hz, iso));
        if (hx && hy && hz) {
          float c[8];
          for (int b = 0; b < 8; ++b) c[b] = vol[p + (b & 1) * si + (b >> 1 & 1) * sj + (b >> 2 & 1)];
          F += tri_count(case_index(c, iso));
        }
      }
}

// verts (V, 3) f64 and tris (F, 3) i32 for the totals count_host gave and the `first` it filled.
inline void emit_host(const float* vol, int nx, int ny, int nz, float iso, const int32_t* first, double* verts, int32_t* tris) {
  const size_t sj = (size_t)nz, si = (size_t)ny * nz;
  size_t f = 0;
  for (int i = 0; i < nx; ++i)
    for (int j = 0; j < ny; ++j)
      for (int k = 0; k < nz; ++k) {
        const size_t p = i * si + j * sj + k;
        const bool hx = i + 1 < nx, hy = j + 1 < ny, hz = k + 1 < nz;
        const float va = vol[p];
        const float nb[3] = {hx ? vol[p + si] : 0.f, hy ? vol[p + sj] : 0.f, hz ? vol[p + 1] : 0.f};
        const int flags = point_flags(va, nb[0], nb[1], nb[2], hx, hy, hz, iso);
        for (int a = 0; a < 3; ++a)
          if (flags >> a & 1) {
            double* o = verts + 3 * ((size_t)first[p] + axis_rank(flags, a));
            o[0] = i, o[1] = j, o[2] = k;
            o[a] += interp(va, nb[a], iso);
          }
        if (!(hx && hy && hz)) continue;
        float c[8];
        for (int b = 0; b < 8; ++b) c[b] = vol[p + (b & 1) * si + (b >> 1 & 1) * sj + (b >> 2 & 1)];
        const int cs = case_index(c, iso);
        for (int t = 0; t < tri_count(cs); ++t, ++f)
          for (int n = 0; n < 3; ++n) {
            const int e = kTriEdges[cs][3 * t + n];
            int di, dj, dk;
            edge_owner(e, di, dj, dk);
            const size_t q = p + di * si + dj * sj + dk;
            const bool qx = i + di + 1 < nx, qy = j + dj + 1 < ny, qz = k + dk + 1 < nz;
            const int qf = point_flags(vol[q], qx ? vol[q + si] : 0.f, qy ? vol[q + sj] : 0.f, qz ? vol[q + 1] : 0.f, qx, qy, qz, iso);
            tris[3 * f + n] = first[q] + axis_rank(qf, edge_axis(e));
          }
      }
}

}  // namespace mc
}  // namespace isr
