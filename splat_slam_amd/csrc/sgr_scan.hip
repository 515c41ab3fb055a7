// The kernels behind sgr_scan.h.
#include "sgr_scan.h"

namespace sgr {
namespace {

constexpr int kThreads = 256;
constexpr int kScanItems = kScanBlock / kThreads;

__global__ void __launch_bounds__(kChunkScanThreads) chunked_scan_kernel(const uint32_t* in, int n, const int32_t* __restrict__ n_dev,
                                                                         uint32_t* out, uint32_t* out2, int32_t* __restrict__ total32,
                                                                         int64_t* __restrict__ total64) {
  __shared__ uint32_t red[kChunkScanThreads / 64];
  const uint32_t total = chunked_exclusive_scan(in, n_dev ? *n_dev : n, out, out2, red);
  if (threadIdx.x == 0) {
    if (total32) *total32 = (int32_t)total;
    if (total64) *total64 = (int64_t)total;
  }
}

// a workgroup's kScanBlock items, 16 consecutive ones per thread: scanned in place, the workgroup's total into sums
__global__ void __launch_bounds__(kThreads) scan_local_kernel(int32_t* __restrict__ data, int n, int32_t* __restrict__ sums) {
  __shared__ uint32_t red[kThreads / 64];
  const int base = blockIdx.x * kScanBlock + threadIdx.x * kScanItems;
  uint32_t s = 0;
  for (int k = 0; k < kScanItems; ++k) s += base + k < n ? (uint32_t)data[base + k] : 0u;
  uint32_t total;
  uint32_t run = block_exclusive_scan<kThreads / 64>(s, red, total);
  for (int k = 0; k < kScanItems; ++k)
    if (base + k < n) {
      const uint32_t v = (uint32_t)data[base + k];
      data[base + k] = (int32_t)run;
      run += v;
    }
  if (threadIdx.x == 0) sums[blockIdx.x] = (int32_t)total;
}

__global__ void __launch_bounds__(kThreads) scan_add_kernel(int32_t* __restrict__ data, int n, const int32_t* __restrict__ sums) {
  const int i = blockIdx.x * kThreads + threadIdx.x;
  if (i < n) data[i] += sums[i / kScanBlock];
}

__global__ void __launch_bounds__(kThreads) compact_vertices_kernel(int V, const float* __restrict__ verts, const float* __restrict__ colors,
                                                                    const int32_t* __restrict__ vnew, float* __restrict__ out_v,
                                                                    float* __restrict__ out_c, int32_t* __restrict__ vmap) {
  const int v = blockIdx.x * kThreads + threadIdx.x;
  if (v >= V) return;
  const int n = vnew[v];
  const bool keep = vnew[v + 1] != n;
  if (vmap) vmap[v] = keep ? n : -1;
  if (!keep) return;
  st3(out_v + 3 * (size_t)n, ld3(verts + 3 * (size_t)v));
  st3(out_c + 3 * (size_t)n, ld3(colors + 3 * (size_t)v));
}

__global__ void __launch_bounds__(kThreads) compact_triangles_kernel(int F, const int32_t* __restrict__ tris, const int32_t* __restrict__ vnew,
                                                                     const int32_t* __restrict__ tnew, int32_t* __restrict__ out_t) {
  const int t = blockIdx.x * kThreads + threadIdx.x;
  if (t >= F) return;
  const int n = tnew[t];
  if (tnew[t + 1] == n) return;
  for (int k = 0; k < 3; ++k) out_t[3 * (size_t)n + k] = vnew[tris[3 * (size_t)t + k]];
}

}  // namespace

void launch_chunked_scan(const uint32_t* in, int n, const int32_t* n_dev, uint32_t* out, uint32_t* out2, int32_t* total32,
                         int64_t* total64, hipStream_t st) {
  hipLaunchKernelGGL(chunked_scan_kernel, dim3(1), dim3(kChunkScanThreads), 0, st, in, n, n_dev, out, out2, total32, total64);
}

void scan_exclusive(int32_t* data, int n, int32_t* sums, hipStream_t st) {
  const int nb = scan_blocks(n);
  hipLaunchKernelGGL(scan_local_kernel, dim3(nb), dim3(kThreads), 0, st, data, n, sums);
  launch_chunked_scan((const uint32_t*)sums, nb, nullptr, (uint32_t*)sums, nullptr, data + n, nullptr, st);
  if (n > 0) hipLaunchKernelGGL(scan_add_kernel, dim3(blocks_for(n)), dim3(kThreads), 0, st, data, n, (const int32_t*)sums);
}

void launch_mesh_compact(int V, int F, const float* verts, const float* colors, const int32_t* tris, const int32_t* vnew,
                         const int32_t* tnew, float* out_v, float* out_c, int32_t* out_t, int32_t* vmap, hipStream_t st) {
  if (V > 0) hipLaunchKernelGGL(compact_vertices_kernel, dim3(blocks_for(V)), dim3(kThreads), 0, st, V, verts, colors, vnew, out_v, out_c, vmap);
  if (F > 0) hipLaunchKernelGGL(compact_triangles_kernel, dim3(blocks_for(F)), dim3(kThreads), 0, st, F, tris, vnew, tnew, out_t);
}

}  // namespace sgr
