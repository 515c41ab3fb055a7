// A uniform grid over a point cloud, built by a counting sort into cells: the search structure of the exact 3-NN of sknn_dist2
// (sgr_aux.hip) and of the exact nearest neighbour of sgr_nn_query (sgr_mesh_eval.hip).  Bounding box -> cell size for ~8 points per
// cell if the box were filled (a surface-like cloud ends up with a few dozen per occupied cell), degenerate sides lifted to 1/1024 of
// the longest one, at most max_cells(n) cells -> count, scan, fill.  The order of the points inside a cell is arbitrary (atomics): a
// query must not depend on it, and neither of the two does (both are exact searches, so neither depends on the cell size either).
// The two query kernels stay with their callers; they only read the struct and the arrays.
//
// Non-finite points.  The bounds ignore a NaN coordinate (fminf / fmaxf) and keep an infinite one.  An axis without any finite
// coordinate, or a box whose cell count cannot be brought below max_cells(n) (infinite extents), collapses to one cell; an infinite
// box gives eps = inf, with which a query never stops early and walks the whole grid.  A point with a NaN coordinate lands in a
// clamped cell, is farther than everything from every query (its distances compare false), and as a 3-NN query finds no neighbour
// (mean 0).  Before the two grids were merged the 3-NN path had none of these guards: it clamped a negative extent to 0, kept
// lo = +inf on an axis of NaNs, and with an infinite extent could leave more cells than its count array holds (writes past the
// array).  Where that path stayed inside its arrays, the results are the same as now, since both forms search exactly.
#pragma once

#include "sgr_common.h"

namespace sgr {

struct PointGrid { float lo[3], hi[3]; float h, inv_h, eps; int g[3]; int gmax; int cells; int n; };
struct PointXform { float m[12]; int on; };     // rows of [R | t] applied to every point; on == 0: identity
constexpr float kCellSlack = 8e-6f;             // fp32 rounding of a cell coordinate, relative to |coords|

__device__ __forceinline__ F3 apply(const PointXform& T, F3 p) {
  if (!T.on) return p;
  return {T.m[0] * p.x + T.m[1] * p.y + T.m[2] * p.z + T.m[3], T.m[4] * p.x + T.m[5] * p.y + T.m[6] * p.z + T.m[7],
          T.m[8] * p.x + T.m[9] * p.y + T.m[10] * p.z + T.m[11]};
}
inline PointXform point_xform(const float* m) {
  PointXform T{};
  if (m) { for (int k = 0; k < 12; ++k) T.m[k] = m[k]; T.on = 1; }
  return T;
}
__device__ __forceinline__ int cell_coord(float v, float lo, float inv_h, int g) { return min(g - 1, max(0, (int)floorf((v - lo) * inv_h))); }

// The caller's buffer: the struct, then count / start [cell] (the points of cell c are start[c] .. start[c] + count[c], and the
// cells of one row are consecutive), then the points in cell order (sxyz) with their original indices (sidx).
inline size_t max_cells(int n) { return (size_t)n / 2 + 1024; }
struct GridBlob { PointGrid* grid; uint32_t *mm, *count, *start, *cursor, *cell_of, *sidx; float* sxyz; };
inline GridBlob carve_grid(void* blob, int n) {
  char* p = (char*)blob;
  const size_t mc = max_cells(n);
  GridBlob b;
  b.grid = (PointGrid*)p; p += 256;
  b.mm = (uint32_t*)p; p += 256;
  b.count = (uint32_t*)p; p += align_up(mc * 4);
  b.start = (uint32_t*)p; p += align_up(mc * 4);
  b.cursor = (uint32_t*)p; p += align_up(mc * 4);
  b.cell_of = (uint32_t*)p; p += align_up((size_t)n * 4);
  b.sidx = (uint32_t*)p; p += align_up((size_t)n * 4);
  b.sxyz = (float*)p;
  return b;
}
inline size_t point_grid_bytes(int n) { const size_t mc = max_cells(n); return 512 + 3 * align_up(mc * 4) + 2 * align_up((size_t)n * 4) + align_up((size_t)n * 12); }

// bounds, setup, count, scan, fill of the n > 0 points (under `transform`, 12 floats, or as they are when it is null) into `blob`
// (point_grid_bytes(n)), on `stream`.  False: a memset or a launch failed.
bool build_point_grid(int n, const float* points, const float* transform, void* blob, hipStream_t stream);

}  // namespace sgr
