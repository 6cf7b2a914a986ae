// radius_count.hpp — how many points of a cloud lie within a radius of each of its points, stated once and compiled for host
// and device.  csrc/radius_count.hip holds the kernels and the C entries (include/isr_radius.h); a plain C++ compiler can
// include this header too (tools/radius_host_check.cpp).
//
// counts[i] = #{ j : d2(i, j) <= r2 }, i itself included, with, in f32,
//     dx = x[j]-x[i]; dy = y[j]-y[i]; dz = z[j]-z[i];  d2 = fmaf(dz, dz, fmaf(dy, dy, dx*dx));  r2 = r * r (r = (float)radius)
// (written out: everything is built with -ffp-contract=off), clamped to cap when cap > 0.  Integers, a function of the
// points, the radius and cap only.
//
// The search: a uniform grid of cells over the cloud's bounding box, edge h >= 1.001 r, points ordered by cell with a
// counting sort (histogram, exclusive scan, scatter); point i scans the 27 cells around its own.  Why 27 are enough: a
// counted pair has |x[j]-x[i]| <= r (1 + 2^-22) on every axis (d2 <= r2 with a handful of f32 roundings), so the f64 values
// (x - min) * inv_h of the two differ by less than 1 / 1.001 * (1 + 2^-20) < 1 and their floors by at most one; clamping is
// monotonic.  A box of more than kMaxCells cells of edge 1.001 r gets a larger h (doubled until it fits): still exact, more
// candidates per cell.  The order of the points inside a cell is whatever the scatter made it: a count does not see it, and
// a scan that stops at cap has counted cap whichever candidates came first.
// PRECONDITION: finite coordinates (a NaN has no cell).
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>

#include "hd.hpp"

namespace isr {
namespace radius {

constexpr int kMaxPoints = 1 << 30;
constexpr int kMaxCells = 1 << 21;
constexpr double kSlack = 1.001;

struct Grid {
  double mn[3];
  double inv_h;
  int n[3];
  int cells;
};

// the cell coordinate of x on an axis that starts at mn and has n cells
ISR_HD int cell_coord(double x, double mn, double inv_h, int n) {
  const double c = floor((x - mn) * inv_h);
  if (!(c > 0.0)) return 0;
  return c < (double)(n - 1) ? (int)c : n - 1;
}

ISR_HD int cell_of(const Grid& g, float x, float y, float z) {
  const int cx = cell_coord((double)x, g.mn[0], g.inv_h, g.n[0]);
  const int cy = cell_coord((double)y, g.mn[1], g.inv_h, g.n[1]);
  const int cz = cell_coord((double)z, g.mn[2], g.inv_h, g.n[2]);
  return (cx * g.n[1] + cy) * g.n[2] + cz;
}

// the grid of a box [mn, mx] (finite, mn <= mx) for radius r > 0
ISR_HD void make_grid(const float* mn, const float* mx, float r, Grid& g) {
  double h = kSlack * (double)r;
  double ext[3];
  bool sane = true;
  for (int d = 0; d < 3; ++d) {
    g.mn[d] = (double)mn[d];
    ext[d] = (double)mx[d] - (double)mn[d];
    sane = sane && ext[d] >= 0.0 && ext[d] <= 1.0e39;
  }
  // a box that is no box (the precondition is broken): one cell, so that every index stays inside the arrays
  g.n[0] = g.n[1] = g.n[2] = 1;
  while (sane) {
    const double nx = floor(ext[0] / h) + 1.0, ny = floor(ext[1] / h) + 1.0, nz = floor(ext[2] / h) + 1.0;
    if (nx * ny * nz <= (double)kMaxCells) {
      g.n[0] = (int)nx;
      g.n[1] = (int)ny;
      g.n[2] = (int)nz;
      break;
    }
    h = h * 2.0;
  }
  g.inv_h = 1.0 / h;
  g.cells = g.n[0] * g.n[1] * g.n[2];
}

ISR_HD float dist2(float x, float y, float z, float sx, float sy, float sz) {
  const float dx = x - sx, dy = y - sy, dz = z - sz;
  return fmaf(dz, dz, fmaf(dy, dy, dx * dx));
}

// The count of one point (x, y, z): sorted (N, 3) the points in cell order, cell c's in [start[c], end[c]).
ISR_HD int count_point(const Grid& g, const float* sorted, const int32_t* start, const int32_t* end, float x, float y,
                              float z, float r2, int cap) {
  const int cx = cell_coord((double)x, g.mn[0], g.inv_h, g.n[0]);
  const int cy = cell_coord((double)y, g.mn[1], g.inv_h, g.n[1]);
  const int cz = cell_coord((double)z, g.mn[2], g.inv_h, g.n[2]);
  const int x0 = cx > 0 ? cx - 1 : 0, x1 = cx + 1 < g.n[0] ? cx + 1 : g.n[0] - 1;
  const int y0 = cy > 0 ? cy - 1 : 0, y1 = cy + 1 < g.n[1] ? cy + 1 : g.n[1] - 1;
  const int z0 = cz > 0 ? cz - 1 : 0, z1 = cz + 1 < g.n[2] ? cz + 1 : g.n[2] - 1;
  int cnt = 0;
  for (int ix = x0; ix <= x1; ++ix)
    for (int iy = y0; iy <= y1; ++iy) {
      // the cells (ix, iy, z0 .. z1) are consecutive, and so are their points
      const int c0 = (ix * g.n[1] + iy) * g.n[2];
      const int j1 = end[c0 + z1];
      for (int j = start[c0 + z0]; j < j1; ++j) {
        if (dist2(sorted[3 * (size_t)j], sorted[3 * (size_t)j + 1], sorted[3 * (size_t)j + 2], x, y, z) <= r2) ++cnt;
        if (cap > 0 && cnt >= cap) return cap;
      }
    }
  return cnt;
}

// The definition as host code: pts (N, 3) finite, N >= 1, r > 0 finite.  scratch: sorted (3 N floats), start and end
// (kMaxCells ints each, only g.cells used).
inline void count_host(const float* pts, int N, float r, int cap, int32_t* counts, float* sorted, int32_t* start, int32_t* end) {
  float mn[3], mx[3];
  for (int d = 0; d < 3; ++d) mn[d] = mx[d] = pts[d];
  for (int i = 1; i < N; ++i)
    for (int d = 0; d < 3; ++d) {
      const float v = pts[3 * (size_t)i + d];
      if (v < mn[d]) mn[d] = v;
      if (v > mx[d]) mx[d] = v;
    }
  Grid g;
  make_grid(mn, mx, r, g);
  for (int c = 0; c < g.cells; ++c) end[c] = 0;
  for (int i = 0; i < N; ++i) ++end[cell_of(g, pts[3 * (size_t)i], pts[3 * (size_t)i + 1], pts[3 * (size_t)i + 2])];
  int run = 0;
  for (int c = 0; c < g.cells; ++c) {
    start[c] = run;
    run += end[c];
    end[c] = start[c];
  }
  for (int i = 0; i < N; ++i) {
    const float* p = pts + 3 * (size_t)i;
    const int j = end[cell_of(g, p[0], p[1], p[2])]++;
    sorted[3 * (size_t)j] = p[0];
    sorted[3 * (size_t)j + 1] = p[1];
    sorted[3 * (size_t)j + 2] = p[2];
  }
  const float r2 = r * r;
  for (int i = 0; i < N; ++i) {
    const float* p = pts + 3 * (size_t)i;
    counts[i] = count_point(g, sorted, start, end, p[0], p[1], p[2], r2, cap);
  }
}

}  // namespace radius
}  // namespace isr
