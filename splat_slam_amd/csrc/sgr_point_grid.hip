// The build of sgr_point_grid.h: five launches.
#include <algorithm>
#include <cmath>

#include "sgr_point_grid.h"
#include "sgr_scan.h"

namespace sgr {
namespace {

constexpr int kThreads = 256;

// floats as unsigned keys of the same order: integer atomicMin / atomicMax on them
__device__ __forceinline__ uint32_t ordered(float f) { const uint32_t u = __float_as_uint(f); return (u & 0x80000000u) ? ~u : (u | 0x80000000u); }
__device__ __forceinline__ float unordered(uint32_t u) { return __uint_as_float((u & 0x80000000u) ? (u & 0x7fffffffu) : ~u); }

// bounding box of the points: per-lane running min / max -> wave (xor shuffles) -> workgroup through LDS -> ONE set of six atomics
// per workgroup and at most 256 workgroups.  (The first version sent six atomics per WAVE of 1024 workgroups to the same six words:
// 24 576 serialised returning atomics = 282 us for 300 k points, a quarter of the whole distCUDA2.)
__global__ void __launch_bounds__(kThreads) grid_bounds_kernel(int n, const float* __restrict__ xyz, PointXform T,
                                                               uint32_t* __restrict__ mm /* min3, max3 (ordered) */) {
  __shared__ float red[4][6];
  float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
  for (int i = blockIdx.x * kThreads + threadIdx.x; i < n; i += gridDim.x * kThreads) {
    const F3 p = apply(T, ld3(xyz + 3 * (size_t)i));
    lo[0] = fminf(lo[0], p.x); hi[0] = fmaxf(hi[0], p.x);
    lo[1] = fminf(lo[1], p.y); hi[1] = fmaxf(hi[1], p.y);
    lo[2] = fminf(lo[2], p.z); hi[2] = fmaxf(hi[2], p.z);
  }
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    for (int off = 32; off > 0; off >>= 1) { lo[k] = fminf(lo[k], __shfl_xor(lo[k], off)); hi[k] = fmaxf(hi[k], __shfl_xor(hi[k], off)); }
    if ((threadIdx.x & 63) == 0) { red[threadIdx.x >> 6][k] = lo[k]; red[threadIdx.x >> 6][3 + k] = hi[k]; }
  }
  __syncthreads();
  if (threadIdx.x < 6) {
    const int k = threadIdx.x;
    if (k < 3) atomicMin(&mm[k], ordered(fminf(fminf(red[0][k], red[1][k]), fminf(red[2][k], red[3][k]))));
    else atomicMax(&mm[k], ordered(fmaxf(fmaxf(red[0][k], red[1][k]), fmaxf(red[2][k], red[3][k]))));
  }
}

__global__ void grid_setup_kernel(int n, int mcells, const uint32_t* __restrict__ mm, PointGrid* __restrict__ out) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  PointGrid G;
  float ext[3], amax = 0.f;
  for (int k = 0; k < 3; ++k) {
    float lo = unordered(mm[k]), hi = unordered(mm[3 + k]);
    if (!(lo <= hi)) lo = hi = 0.f;          // only non-finite points: one cell at the origin
    G.lo[k] = lo; G.hi[k] = hi;
    ext[k] = hi - lo;
    amax = fmaxf(amax, fmaxf(fabsf(lo), fabsf(hi)));
  }
  const float emax = fmaxf(ext[0], fmaxf(ext[1], ext[2]));
  float vol = 1.f;                           // degenerate sides lifted to 1/1024 of the longest one (planar / linear clouds)
  for (int k = 0; k < 3; ++k) vol *= fmaxf(ext[k], emax * (1.f / 1024.f));
  float h = emax > 0.f ? cbrtf(vol * 8.f / (float)n) : 1.f;
  h = fmaxf(h, emax * (1.f / 1024.f));
  if (!(h > 0.f) || !isfinite(h)) h = 1.f;
  for (int iter = 0; iter < 32; ++iter) {
    long long cells = 1;
    for (int k = 0; k < 3; ++k) { G.g[k] = min(1024, max(1, (int)floorf(ext[k] / h) + 1)); cells *= G.g[k]; }
    if (cells <= (long long)mcells) break;
    h *= 1.26f;                              // (cells shrink by ~2 per step)
  }
  if ((long long)G.g[0] * G.g[1] * G.g[2] > (long long)mcells) G.g[0] = G.g[1] = G.g[2] = 1;   // non-finite extents: one cell
  G.cells = G.g[0] * G.g[1] * G.g[2];
  G.gmax = max(G.g[0], max(G.g[1], G.g[2]));
  G.h = h; G.inv_h = 1.f / h;
  G.eps = kCellSlack * (amax + emax) + 1e-30f;   // what fp32 rounding can move a cell coordinate by, in length units
  G.n = n;
  *out = G;
}

__global__ void __launch_bounds__(kThreads) grid_count_kernel(int n, const float* __restrict__ xyz, PointXform T, const PointGrid* __restrict__ Gp,
                                                              uint32_t* __restrict__ count, uint32_t* __restrict__ cell_of) {
  const int i = blockIdx.x * kThreads + threadIdx.x;
  if (i >= n) return;
  const PointGrid G = *Gp;
  const F3 p = apply(T, ld3(xyz + 3 * (size_t)i));
  const int cx = cell_coord(p.x, G.lo[0], G.inv_h, G.g[0]), cy = cell_coord(p.y, G.lo[1], G.inv_h, G.g[1]),
            cz = cell_coord(p.z, G.lo[2], G.inv_h, G.g[2]);
  const uint32_t c = (uint32_t)((cz * G.g[1] + cy) * G.g[0] + cx);
  cell_of[i] = c;
  atomicAdd(&count[c], 1u);
}

__global__ void __launch_bounds__(kThreads) grid_fill_kernel(int n, const float* __restrict__ xyz, PointXform T, const uint32_t* __restrict__ cell_of,
                                                             uint32_t* __restrict__ cursor, float* __restrict__ sxyz, uint32_t* __restrict__ sidx) {
  const int i = blockIdx.x * kThreads + threadIdx.x;
  if (i >= n) return;
  const F3 p = apply(T, ld3(xyz + 3 * (size_t)i));
  const uint32_t pos = atomicAdd(&cursor[cell_of[i]], 1u);      // order inside a cell is arbitrary: the queries do not depend on it
  sxyz[3 * pos] = p.x; sxyz[3 * pos + 1] = p.y; sxyz[3 * pos + 2] = p.z;
  sidx[pos] = (uint32_t)i;
}

}  // namespace

bool build_point_grid(int n, const float* points, const float* transform, void* blob, hipStream_t st) {
  const GridBlob b = carve_grid(blob, n);
  const PointXform T = point_xform(transform);
  const size_t mc = max_cells(n);
  if (hipMemsetAsync(b.mm, 0xff, 12, st) != hipSuccess || hipMemsetAsync(b.mm + 3, 0, 12, st) != hipSuccess ||
      hipMemsetAsync(b.count, 0, mc * 4, st) != hipSuccess)
    return false;
  const int nb = blocks_for(n);
  hipLaunchKernelGGL(grid_bounds_kernel, dim3(std::min(256, nb)), dim3(kThreads), 0, st, n, points, T, b.mm);
  hipLaunchKernelGGL(grid_setup_kernel, dim3(1), dim3(64), 0, st, n, (int)mc, b.mm, b.grid);
  hipLaunchKernelGGL(grid_count_kernel, dim3(nb), dim3(kThreads), 0, st, n, points, T, b.grid, b.count, b.cell_of);
  // cells <= n / 2 + 1024: ~150 chunks at 300 k points
  launch_chunked_scan(b.count, 0, &b.grid->cells, b.start, b.cursor, nullptr, nullptr, st);
  hipLaunchKernelGGL(grid_fill_kernel, dim3(nb), dim3(kThreads), 0, st, n, points, T, b.cell_of, b.cursor, b.sxyz, b.sidx);
  return hipGetLastError() == hipSuccess;
}

}  // namespace sgr
