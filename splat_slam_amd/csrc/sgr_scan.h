// Integer prefix sums, once: the workgroup primitive, the single-workgroup scan of an array in memory, the device-wide scan, and the
// stable compaction of a mesh by scanned keep flags.  Every kernel lives in sgr_scan.hip behind a host launcher (the library is
// linked without relocatable device code); the device primitives are inlined into their callers.
// Not here, on purpose: the fp64 CDF scan of sgr_mesh_eval.hip (its order of additions is part of its contract), dba::scan_1024,
// the ballot scan of sgr_fuse.hip and the selection scan of sgr_video.hip (different algorithms for different data).
#pragma once

#include "sgr_common.h"

namespace sgr {

// exclusive prefix of `v` inside a workgroup of WAVES waves + the workgroup's total (in every thread); red: WAVES uints of LDS,
// free again on return.  Every thread of the workgroup calls it.
template <int WAVES>
__device__ __forceinline__ uint32_t block_exclusive_scan(uint32_t v, uint32_t* red, uint32_t& total) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const uint32_t inc = wave_scan_add_u32(v);
  if (lane == 63) red[wv] = inc;
  __syncthreads();
  uint32_t w[WAVES];
#pragma unroll
  for (int k = 0; k < WAVES; ++k) w[k] = red[k];
  __syncthreads();
  uint32_t sum = w[0];
#pragma unroll
  for (int k = 1; k < WAVES; ++k) sum += w[k];
  total = sum;
  uint32_t base = wv > 0 ? w[0] : 0u;
#pragma unroll
  for (int k = 1; k < WAVES - 1; ++k) base += wv > k ? w[k] : 0u;
  return base + inc - v;
}
// the 256-thread case under the name the rasteriser kernels know it by
__device__ __forceinline__ uint32_t block256_exclusive_scan(uint32_t v, uint32_t* red, uint32_t& total) {
  return block_exclusive_scan<4>(v, red, total);
}

// One workgroup of 1024 threads scans in[0..n) in chunks of 1024 with a running carry: the exclusive prefix of element i goes to
// out[i] and, when given, to out2[i] (a counting sort's start and cursor); in may be out.  Returns the total in every thread.
// red: 16 uints of LDS.
constexpr int kChunkScanThreads = 1024;
__device__ __forceinline__ uint32_t chunked_exclusive_scan(const uint32_t* in, int n, uint32_t* out, uint32_t* out2, uint32_t* red) {
  uint32_t carry = 0u;
  for (int base = 0; base < n; base += kChunkScanThreads) {
    const int i = base + (int)threadIdx.x;
    const uint32_t v = i < n ? in[i] : 0u;
    uint32_t total;
    const uint32_t ex = carry + block_exclusive_scan<kChunkScanThreads / 64>(v, red, total);
    if (i < n) { out[i] = ex; if (out2) out2[i] = ex; }
    carry += total;
  }
  return carry;
}
// ... as one launch.  The length is n, or *n_dev where n_dev is given (a length only the device knows: the cells of a point grid);
// the total goes to *total32 and / or *total64 where given.
void launch_chunked_scan(const uint32_t* in, int n, const int32_t* n_dev, uint32_t* out, uint32_t* out2, int32_t* total32,
                         int64_t* total64, hipStream_t st);

// Device-wide exclusive scan of data[0..n) in place, the total into data[n]: workgroups of kScanBlock items, their totals scanned by
// one workgroup, then the add.  sums: scan_blocks(n) + 1 ints.  n == 0 writes data[0] = 0 (one idle workgroup, no empty grid).
constexpr int kScanBlock = 4096;
inline int scan_blocks(int n) { const int b = (n + kScanBlock - 1) / kScanBlock; return b > 0 ? b : 1; }
void scan_exclusive(int32_t* data, int n, int32_t* sums, hipStream_t st);

// Stable compaction of a mesh by scanned keep flags: vnew [V + 1] and tnew [F + 1] hold exclusive prefixes with the total last, so
// element i stays iff prefix[i + 1] != prefix[i].  Kept vertices and colours move to their prefix, kept triangles are reindexed
// through vnew; vmap (optional) gets the new index of every vertex or -1.  V == 0 / F == 0 launch nothing.
void launch_mesh_compact(int V, int F, const float* verts, const float* colors, const int32_t* tris, const int32_t* vnew,
                         const int32_t* tnew, float* out_v, float* out_c, int32_t* out_t, int32_t* vmap, hipStream_t st);

}  // namespace sgr
