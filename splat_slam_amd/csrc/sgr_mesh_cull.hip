// Culling a mesh to what a set of cameras saw ("Mesh culling"; the cull_mesh of the NICE-SLAM family of
// evaluations: a frustum test, an occlusion test against depth rendered from the mesh itself, unseen faces dropped).
//   sgr_cull_project      one thread per (vertex, frame), fp64: pixel coordinates snapped to 1/256 pixel as int32, camera z as fp32
//   sgr_cull_raster       z-buffer of the mesh from the snapped coordinates: exact int64 coverage (inclusive edges, both windings),
//                         perspective-correct fp32 depth, integer atomicMin on the bit pattern of the (positive) depth
//   sgr_cull_visibility   one thread per vertex: the number of frames that see it (frustum, far, depth map within eps)
//   sgr_cull_select       faces whose vertices were seen often enough, vertices they still reference: two exclusive scans
//   sgr_cull_compact      vertices, colours and faces in their original order, reindexed (scans and compaction: sgr_scan.h)
// Everything after the projection is integer or single-operation fp32 arithmetic: tests/mesh_cull_ref.py restates it bit for bit.
// No float atomics: the z-buffer does not depend on the order of the triangles.
#include <algorithm>
#include <cmath>
#include <cstdint>

#include "sgr_common.h"
#include "sgr_scan.h"

namespace sgr {
int set_error(int code, const char* fmt, ...);

namespace {

constexpr int kThreads = 256;
constexpr int kSub = 1 << SGR_CULL_SUBPIXEL_BITS;                   // snapped units per pixel
constexpr int kGuardSub = SGR_CULL_GUARD_PIXELS * kSub;             // |snapped coordinate| of a valid vertex is at most this
constexpr int kSmallBox = 8;                                        // a bounding box of at most 8 x 8 pixels is its thread's own loop
constexpr int kLargeBlocks = 1024;                                  // grid of the wave-per-triangle pass (strides over the list)
constexpr uint32_t kInfBits = 0x7f800000u;

struct FrameTab { SgrCullFrame f[SGR_CULL_MAX_FRAMES]; };

// ---- projection: the one place where a vertex meets a camera
struct Snapped { int32_t x, y; float z; };
__device__ __forceinline__ Snapped project_vertex(const SgrCullFrame& c, double X, double Y, double Z, double near) {
#pragma clang fp contract(off)
  const double px = c.w2c[0] * X + c.w2c[1] * Y + c.w2c[2] * Z + c.w2c[3];
  const double py = c.w2c[4] * X + c.w2c[5] * Y + c.w2c[6] * Z + c.w2c[7];
  const double pz = c.w2c[8] * X + c.w2c[9] * Y + c.w2c[10] * Z + c.w2c[11];
  const double u = c.fx * px / pz + c.cx, v = c.fy * py / pz + c.cy;
  const double guard = (double)SGR_CULL_GUARD_PIXELS;
  const float zf = (float)pz;
  // (every comparison is false for NaN; zf > 0 and finite: a z that fp32 cannot hold is no depth)
  const bool ok = pz >= near && fabs(u) <= guard && fabs(v) <= guard && zf > 0.f && zf < INFINITY;
  if (!ok) return {0, 0, 0.f};
  return {(int32_t)llrint(u * (double)kSub), (int32_t)llrint(v * (double)kSub), zf};
}

__global__ void __launch_bounds__(kThreads) cull_project_kernel(int V, const float* __restrict__ xyz, FrameTab tab, double near,
                                                                int32_t* __restrict__ xy, float* __restrict__ z) {
  const int v = blockIdx.x * kThreads + threadIdx.x;
  if (v >= V) return;
  const int f = blockIdx.y;
  const F3 p = ld3(xyz + 3 * (size_t)v);
  const Snapped s = project_vertex(tab.f[f], (double)p.x, (double)p.y, (double)p.z, near);
  const size_t o = (size_t)f * V + v;
  xy[2 * o] = s.x;
  xy[2 * o + 1] = s.y;
  z[o] = s.z;
}

// ---- z-buffer
// A triangle of one frame, oriented to positive doubled area A.  Edge function k (opposite vertex k) at the snapped point (px, py)
// is a[k] px + b[k] py + c[k]: it is A at vertex k, 0 on the opposite edge, and the three sum to A everywhere.
struct Tri {
  int64_t a[3], b[3], c[3], area;
  float rz[3];                     // 1 / z of vertex k
  int j0, j1, i0, i1;              // clamped pixel box (empty when j0 > j1 or i0 > i1)
};
enum { kTriNone = 0, kTriInvalid = 1, kTriDraw = 2 };

__device__ __forceinline__ int tri_setup(int V, const int32_t* __restrict__ tris, size_t t, const int32_t* __restrict__ xy,
                                         const float* __restrict__ z, int H, int W, Tri& T) {
  const int i0 = tris[3 * t], i1 = tris[3 * t + 1], i2 = tris[3 * t + 2];
  if (i0 < 0 || i0 >= V || i1 < 0 || i1 >= V || i2 < 0 || i2 >= V) return kTriInvalid;
  const float z0 = z[i0];
  float z1 = z[i1], z2 = z[i2];
  if (!(z0 > 0.f && z1 > 0.f && z2 > 0.f) || !(z0 < INFINITY && z1 < INFINITY && z2 < INFINITY)) return kTriInvalid;
  const int64_t x0 = xy[2 * (size_t)i0], y0 = xy[2 * (size_t)i0 + 1];
  int64_t x1 = xy[2 * (size_t)i1], y1 = xy[2 * (size_t)i1 + 1], x2 = xy[2 * (size_t)i2], y2 = xy[2 * (size_t)i2 + 1];
  const int64_t g = kGuardSub;
  if (x0 < -g || x0 > g || y0 < -g || y0 > g || x1 < -g || x1 > g || y1 < -g || y1 > g || x2 < -g || x2 > g || y2 < -g || y2 > g)
    return kTriInvalid;            // (coordinates that sgr_cull_project never writes: the int64 products below stay below 2^48)
  int64_t area = (x1 - x0) * (y2 - y0) - (x2 - x0) * (y1 - y0);
  if (area == 0) return kTriNone;
  if (area < 0) {                  // the other winding: swap vertices 1 and 2
    int64_t s = x1; x1 = x2; x2 = s;
    s = y1; y1 = y2; y2 = s;
    const float zs = z1; z1 = z2; z2 = zs;
    area = -area;
  }
  const int64_t xmin = min(x0, min(x1, x2)), xmax = max(x0, max(x1, x2)), ymin = min(y0, min(y1, y2)), ymax = max(y0, max(y1, y2));
  // pixel centres kSub j inside [xmin, xmax]: ceil(xmin / kSub) .. floor(xmax / kSub) (>> floors)
  T.j0 = (int)max((int64_t)0, (xmin + kSub - 1) >> SGR_CULL_SUBPIXEL_BITS);
  T.j1 = (int)min((int64_t)W - 1, xmax >> SGR_CULL_SUBPIXEL_BITS);
  T.i0 = (int)max((int64_t)0, (ymin + kSub - 1) >> SGR_CULL_SUBPIXEL_BITS);
  T.i1 = (int)min((int64_t)H - 1, ymax >> SGR_CULL_SUBPIXEL_BITS);
  if (T.j0 > T.j1 || T.i0 > T.i1) return kTriNone;
  // edge from vertex p to vertex q at (px, py): (xq - xp)(py - yp) - (yq - yp)(px - xp)
  const int64_t xs[3] = {x0, x1, x2}, ys[3] = {y0, y1, y2};
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const int p = (k + 1) % 3, q = (k + 2) % 3;
    T.a[k] = -(ys[q] - ys[p]);
    T.b[k] = xs[q] - xs[p];
    T.c[k] = -(T.b[k] * ys[p]) - T.a[k] * xs[p];
  }
  T.area = area;
  T.rz[0] = 1.f / z0; T.rz[1] = 1.f / z1; T.rz[2] = 1.f / z2;
  return kTriDraw;
}

// pixel (i, j) of the frame's depth image: covered when the three edge functions are >= 0 (inclusive: shared edges are drawn by
// both neighbours, never by neither); depth A / (E0/z0 + E1/z1 + E2/z2) in fp32, every operation rounded once
__device__ __forceinline__ void tri_pixel(const Tri& T, int i, int j, uint32_t* __restrict__ row) {
#pragma clang fp contract(off)
  const int64_t px = (int64_t)j * kSub, py = (int64_t)i * kSub;
  const int64_t e0 = T.a[0] * px + T.b[0] * py + T.c[0], e1 = T.a[1] * px + T.b[1] * py + T.c[1], e2 = T.a[2] * px + T.b[2] * py + T.c[2];
  if ((e0 | e1 | e2) < 0) return;
  const float den = ((float)e0 * T.rz[0] + (float)e1 * T.rz[1]) + (float)e2 * T.rz[2];
  const uint32_t bits = __float_as_uint((float)T.area / den);
  if (bits < row[j]) atomicMin(&row[j], bits);      // values only fall: a stale read costs a redundant atomic, never a lost one
}

__global__ void __launch_bounds__(kThreads) cull_raster_small_kernel(int V, int F, const int32_t* __restrict__ tris,
                                                                     const int32_t* __restrict__ xy, const float* __restrict__ z, int H,
                                                                     int W, uint32_t* __restrict__ depth, int32_t* __restrict__ skipped,
                                                                     uint32_t* __restrict__ large_count, uint64_t* __restrict__ large) {
  const int t = blockIdx.x * kThreads + threadIdx.x;
  if (t >= F) return;
  const int f = blockIdx.y;
  Tri T;
  const int kind = tri_setup(V, tris, (size_t)t, xy + 2 * (size_t)f * V, z + (size_t)f * V, H, W, T);
  if (kind == kTriInvalid) {
    if (skipped) atomicAdd(&skipped[f], 1);
    return;
  }
  if (kind != kTriDraw) return;
  if (T.j1 - T.j0 >= kSmallBox || T.i1 - T.i0 >= kSmallBox) {
    large[atomicAdd(large_count, 1u)] = ((uint64_t)f << 32) | (uint32_t)t;     // at most F * n entries: one per (triangle, frame)
    return;
  }
  uint32_t* img = depth + (size_t)f * H * W;
  for (int i = T.i0; i <= T.i1; ++i)
    for (int j = T.j0; j <= T.j1; ++j) tri_pixel(T, i, j, img + (size_t)i * W);
}

// one wave per listed triangle, lanes over the pixels of its box, the waves striding over the list
__global__ void __launch_bounds__(kThreads) cull_raster_large_kernel(int V, const int32_t* __restrict__ tris, const int32_t* __restrict__ xy,
                                                                     const float* __restrict__ z, int H, int W, uint32_t* __restrict__ depth,
                                                                     const uint32_t* __restrict__ large_count,
                                                                     const uint64_t* __restrict__ large) {
  const uint32_t count = *large_count;
  const int lane = threadIdx.x & 63;
  const uint32_t waves = gridDim.x * (kThreads / 64);
  for (uint32_t e = blockIdx.x * (kThreads / 64) + (threadIdx.x >> 6); e < count; e += waves) {
    const uint64_t rec = large[e];
    const int f = (int)(rec >> 32);
    Tri T;
    if (tri_setup(V, tris, (size_t)(uint32_t)rec, xy + 2 * (size_t)f * V, z + (size_t)f * V, H, W, T) != kTriDraw) continue;
    uint32_t* img = depth + (size_t)f * H * W;
    const int w = T.j1 - T.j0 + 1;
    const int total = w * (T.i1 - T.i0 + 1);         // H, W <= 16384: below 2^28
    for (int k = lane; k < total; k += 64) {
      const int i = T.i0 + k / w, j = T.j0 + k % w;
      tri_pixel(T, i, j, img + (size_t)i * W);
    }
  }
}

// ---- visibility
__global__ void __launch_bounds__(kThreads) cull_visibility_kernel(int V, int n, const int32_t* __restrict__ xy, const float* __restrict__ z,
                                                                   const float* __restrict__ depth, int H, int W, int edge, float far,
                                                                   float eps, int32_t* __restrict__ seen) {
  const int v = blockIdx.x * kThreads + threadIdx.x;
  if (v >= V) return;
  int count = 0;
  for (int f = 0; f < n; ++f) {
    const size_t o = (size_t)f * V + v;
    const float zv = z[o];
    if (!(zv > 0.f && zv <= far)) continue;
    const int j = (xy[2 * o] + kSub / 2) >> SGR_CULL_SUBPIXEL_BITS, i = (xy[2 * o + 1] + kSub / 2) >> SGR_CULL_SUBPIXEL_BITS;
    if (j < edge || j >= W - edge || i < edge || i >= H - edge) continue;
    if (depth) {
      const float d = depth[((size_t)f * H + i) * W + j];
      if (d > 0.f && !(__fsub_rn(zv, d) <= eps)) continue;       // zero, negative, NaN: a hole that constrains nothing; +inf passes
    }
    ++count;
  }
  seen[v] += count;                // one owner per vertex: chunks of frames accumulate without atomics
}

// ---- selection
struct Select { int32_t *vnew, *tnew, *sums; };      // vnew [V + 1], tnew [F + 1]: flags, then exclusive prefixes with the total last
inline size_t select_bytes(int V, int F) {
  return align_up(((size_t)V + 1) * 4) + align_up(((size_t)F + 1) * 4) + align_up(((size_t)scan_blocks(V > F ? V : F) + 1) * 4);
}
inline Select carve_select(void* scratch, int V, int F) {
  char* p = (char*)scratch;
  Select s;
  s.vnew = (int32_t*)p; p += align_up(((size_t)V + 1) * 4);
  s.tnew = (int32_t*)p; p += align_up(((size_t)F + 1) * 4);
  s.sums = (int32_t*)p;
  return s;
}

__global__ void __launch_bounds__(kThreads) cull_face_keep_kernel(int V, int F, const int32_t* __restrict__ tris, const int32_t* __restrict__ seen,
                                                                  int min_views, int any, Select s) {
  const int t = blockIdx.x * kThreads + threadIdx.x;
  if (t >= F) return;
  const int a = tris[3 * (size_t)t], b = tris[3 * (size_t)t + 1], c = tris[3 * (size_t)t + 2];
  bool keep = false;
  if (a >= 0 && a < V && b >= 0 && b < V && c >= 0 && c < V) {
    const bool sa = seen[a] >= min_views, sb = seen[b] >= min_views, sc = seen[c] >= min_views;
    keep = any ? (sa || sb || sc) : (sa && sb && sc);
  }
  s.tnew[t] = keep ? 1 : 0;
  if (keep) { s.vnew[a] = 1; s.vnew[b] = 1; s.vnew[c] = 1; }      // (vnew was zeroed; every writer writes 1)
}

inline size_t raster_bytes(int F, int n) { return 256 + align_up((size_t)F * (size_t)n * 8); }

}  // namespace
}  // namespace sgr

using namespace sgr;

extern "C" {

int sgr_cull_project(int32_t V, const float* vertices, int32_t n, const SgrCullFrame* frames, double near, int32_t* xy, float* z,
                     void* stream) {
  if (V <= 0 || n < 1 || n > SGR_CULL_MAX_FRAMES || !vertices || !frames || !xy || !z || !(near > 0.0))
    return set_error(SGR_ERR_INVALID, "cull_project: bad arguments (V=%d n=%d near=%g)", V, n, near);
  FrameTab tab{};
  for (int f = 0; f < n; ++f) tab.f[f] = frames[f];
  hipLaunchKernelGGL(cull_project_kernel, dim3(blocks_for(V), n), dim3(kThreads), 0, (hipStream_t)stream, V, vertices, tab, near, xy, z);
  return hipGetLastError() == hipSuccess ? SGR_OK : set_error(SGR_ERR_HIP, "cull_project launch failed");
}

size_t sgr_cull_raster_bytes(int32_t F, int32_t n) {
  if (F < 0 || n < 1 || n > SGR_CULL_MAX_FRAMES) return 0;
  return raster_bytes(F, n);
}

int sgr_cull_raster(int32_t V, int32_t F, const int32_t* triangles, int32_t n, const int32_t* xy, const float* z, int32_t H, int32_t W,
                    float* depth, int32_t* skipped, void* scratch, size_t scratch_bytes, void* stream) {
  if (V <= 0 || F < 0 || n < 1 || n > SGR_CULL_MAX_FRAMES || H < 1 || W < 1 || H > SGR_CULL_GUARD_PIXELS || W > SGR_CULL_GUARD_PIXELS ||
      (F > 0 && !triangles) || !xy || !z || !depth)
    return set_error(SGR_ERR_INVALID, "cull_raster: bad arguments (V=%d F=%d n=%d H=%d W=%d)", V, F, n, H, W);
  if (!scratch || scratch_bytes < raster_bytes(F, n)) return set_error(SGR_ERR_WORKSPACE, "cull_raster: scratch too small");
  hipStream_t st = (hipStream_t)stream;
  uint32_t* count = (uint32_t*)scratch;
  uint64_t* large = (uint64_t*)((char*)scratch + 256);
  if (hipMemsetD32Async((hipDeviceptr_t)depth, (int)kInfBits, (size_t)n * H * W, st) != hipSuccess ||
      hipMemsetAsync(count, 0, 256, st) != hipSuccess || (skipped && hipMemsetAsync(skipped, 0, (size_t)n * 4, st) != hipSuccess))
    return set_error(SGR_ERR_HIP, "cull_raster: memset");
  if (F > 0) {
    hipLaunchKernelGGL(cull_raster_small_kernel, dim3(blocks_for(F), n), dim3(kThreads), 0, st, V, F, triangles, xy, z, H, W, (uint32_t*)depth,
                       skipped, count, large);
    const long long pairs = (long long)F * n;
    const int grid = (int)std::min<long long>(kLargeBlocks, (pairs + kThreads / 64 - 1) / (kThreads / 64));
    hipLaunchKernelGGL(cull_raster_large_kernel, dim3(grid), dim3(kThreads), 0, st, V, triangles, xy, z, H, W, (uint32_t*)depth,
                       (const uint32_t*)count, (const uint64_t*)large);
  }
  return hipGetLastError() == hipSuccess ? SGR_OK : set_error(SGR_ERR_HIP, "cull_raster launch failed");
}

int sgr_cull_visibility(int32_t V, int32_t n, const int32_t* xy, const float* z, const float* depth, int32_t H, int32_t W, int32_t edge,
                        float far, float eps, int32_t* seen, void* stream) {
  if (V <= 0 || n < 1 || n > SGR_CULL_MAX_FRAMES || H < 1 || W < 1 || edge < 0 || !xy || !z || !seen || !(far > 0.f) || std::isnan(eps))
    return set_error(SGR_ERR_INVALID, "cull_visibility: bad arguments (V=%d n=%d H=%d W=%d edge=%d)", V, n, H, W, edge);
  hipLaunchKernelGGL(cull_visibility_kernel, dim3(blocks_for(V)), dim3(kThreads), 0, (hipStream_t)stream, V, n, xy, z, depth, H, W, edge, far,
                     eps, seen);
  return hipGetLastError() == hipSuccess ? SGR_OK : set_error(SGR_ERR_HIP, "cull_visibility launch failed");
}

size_t sgr_cull_select_bytes(int32_t V, int32_t F) {
  if (V < 0 || F < 0) return 0;
  return select_bytes(V, F);
}

int sgr_cull_select(int32_t V, int32_t F, const int32_t* triangles, const int32_t* seen, int32_t min_views, int32_t rule, void* scratch,
                    size_t scratch_bytes, int32_t* totals, void* stream) {
  if (V < 0 || F < 0 || min_views < 1 || (rule != SGR_CULL_RULE_ALL && rule != SGR_CULL_RULE_ANY) || !totals || (V > 0 && !seen) ||
      (F > 0 && !triangles))
    return set_error(SGR_ERR_INVALID, "cull_select: bad arguments (V=%d F=%d min_views=%d rule=%d)", V, F, min_views, rule);
  if (!scratch || scratch_bytes < select_bytes(V, F)) return set_error(SGR_ERR_WORKSPACE, "cull_select: scratch too small");
  hipStream_t st = (hipStream_t)stream;
  Select s = carve_select(scratch, V, F);
  if (hipMemsetAsync(s.vnew, 0, ((size_t)V + 1) * 4, st) != hipSuccess) return set_error(SGR_ERR_HIP, "cull_select: memset");
  if (F > 0 && V > 0)
    hipLaunchKernelGGL(cull_face_keep_kernel, dim3(blocks_for(F)), dim3(kThreads), 0, st, V, F, triangles, seen, min_views,
                       rule == SGR_CULL_RULE_ANY ? 1 : 0, s);
  else if (hipMemsetAsync(s.tnew, 0, ((size_t)F + 1) * 4, st) != hipSuccess)
    return set_error(SGR_ERR_HIP, "cull_select: memset");
  scan_exclusive(s.vnew, V, s.sums, st);
  scan_exclusive(s.tnew, F, s.sums, st);
  if (hipMemcpyAsync(totals, s.vnew + V, 4, hipMemcpyDeviceToDevice, st) != hipSuccess ||
      hipMemcpyAsync(totals + 1, s.tnew + F, 4, hipMemcpyDeviceToDevice, st) != hipSuccess)
    return set_error(SGR_ERR_HIP, "cull_select: copy");
  return hipGetLastError() == hipSuccess ? SGR_OK : set_error(SGR_ERR_HIP, "cull_select launch failed");
}

int sgr_cull_compact(int32_t V, int32_t F, const float* vertices, const float* colors, const int32_t* triangles, void* scratch,
                     size_t scratch_bytes, float* out_vertices, float* out_colors, int32_t* out_triangles, int32_t* vertex_map,
                     void* stream) {
  if (V < 0 || F < 0 || (V > 0 && (!vertices || !colors)) || (F > 0 && !triangles))
    return set_error(SGR_ERR_INVALID, "cull_compact: bad arguments (V=%d F=%d)", V, F);
  if (!scratch || scratch_bytes < select_bytes(V, F)) return set_error(SGR_ERR_WORKSPACE, "cull_compact: scratch too small");
  const Select s = carve_select(scratch, V, F);
  launch_mesh_compact(V, F, vertices, colors, triangles, s.vnew, s.tnew, out_vertices, out_colors, out_triangles, vertex_map, (hipStream_t)stream);
  return hipGetLastError() == hipSuccess ? SGR_OK : set_error(SGR_ERR_HIP, "cull_compact launch failed");
}

}  // extern "C"
