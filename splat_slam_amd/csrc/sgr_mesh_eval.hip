// Mesh evaluation of eval_rendering's eval_mesh branch (/root/reference/src/utils/eval_utils.py:174-187: run_evaluation of
// evaluate_3d_reconstruction_lib with distance_thresh 0.05 and icp_align=True).  That library's source is not available, so the
// conventions are the ones listed in DESIGN.md section 3, "Mesh evaluation":
//   sgr_surface_sample                       area-weighted surface samples: fp64 areas, fp64 inclusive scan, one thread per sample
//                                            (counter-based hash -> binary search over the CDF -> sqrt-barycentric point)
//   sgr_nn_grid_build / sgr_nn_query         exact nearest neighbours through a uniform grid over the target cloud (sgr_point_grid.h);
//                                            the query walks rings of cells until the best distance is proven
//   sgr_icp_accumulate                       fp64 correspondence sums of one point-to-point ICP step (the SVD runs on the host)
//   sgr_cloud_metrics                        sums and threshold counts of the two distance arrays
// Reductions are per-workgroup partials followed by one fixed-order pass: no float atomics, bitwise reproducible.
#include <cmath>
#include <cstdint>

#include "sgr_common.h"
#include "sgr_point_grid.h"

namespace sgr {
int set_error(int code, const char* fmt, ...);

namespace {

constexpr int kThreads = 256;
constexpr int kScanItems = 16, kScanBlock = kThreads * kScanItems;   // fp64 CDF scan: 4096 faces per workgroup
constexpr int kRedBlocks = 256;                                      // partial workgroups of every reduction (fixed: fixed order)
constexpr int kIcpSums = 17;                                         // count, sum d^2, sum p (3), sum q (3), sum p q^T (9)


// ---- counter-based uniforms: splitmix64 finaliser over (seed, sample, stream); independent of the launch shape
__device__ __forceinline__ uint64_t mix64(uint64_t z) {
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
__device__ __forceinline__ uint64_t hash3(uint64_t seed, uint64_t i, uint32_t stream) {
  return mix64(mix64(seed ^ 0x9E3779B97F4A7C15ull) + 4ull * i + stream);
}
__device__ __forceinline__ double u53(uint64_t h) { return (double)(h >> 11) * 0x1.0p-53; }     // [0, 1)
__device__ __forceinline__ float u24(uint64_t h) { return (float)(h >> 40) * 0x1.0p-24f; }      // [0, 1)

// ---- sampling
__global__ void __launch_bounds__(kThreads) area_kernel(int V, int F, const float* __restrict__ xyz, const int32_t* __restrict__ tri,
                                                        double* __restrict__ area, double* __restrict__ cdf) {
  const int f = blockIdx.x * kThreads + threadIdx.x;
  if (f >= F) return;
  const int a = tri[3 * f], b = tri[3 * f + 1], c = tri[3 * f + 2];
  double s = 0.0;
  if (a >= 0 && a < V && b >= 0 && b < V && c >= 0 && c < V) {
    const double ux = (double)xyz[3 * b] - xyz[3 * a], uy = (double)xyz[3 * b + 1] - xyz[3 * a + 1], uz = (double)xyz[3 * b + 2] - xyz[3 * a + 2];
    const double vx = (double)xyz[3 * c] - xyz[3 * a], vy = (double)xyz[3 * c + 1] - xyz[3 * a + 1], vz = (double)xyz[3 * c + 2] - xyz[3 * a + 2];
    const double cx = uy * vz - uz * vy, cy = uz * vx - ux * vz, cz = ux * vy - uy * vx;
    s = 0.5 * sqrt(cx * cx + cy * cy + cz * cz);
  }
  area[f] = s;                      // out-of-range faces get area 0 (the host refuses them first)
  cdf[f] = s;
}

// inclusive fp64 scan, in place: per workgroup (16 faces per lane, lanes scanned in LDS), then the workgroup totals, then the add
__global__ void __launch_bounds__(kThreads) cdf_local_kernel(int F, double* __restrict__ cdf, double* __restrict__ sums) {
  __shared__ double s[kThreads];
  const int base = blockIdx.x * kScanBlock + threadIdx.x * kScanItems;
  double t = 0.0;
  for (int k = 0; k < kScanItems; ++k) t += base + k < F ? cdf[base + k] : 0.0;
  s[threadIdx.x] = t;
  __syncthreads();
  for (int off = 1; off < kThreads; off <<= 1) {          // Hillis-Steele: fixed order for every lane
    const double v = threadIdx.x >= (unsigned)off ? s[threadIdx.x - off] : 0.0;
    __syncthreads();
    s[threadIdx.x] += v;
    __syncthreads();
  }
  double run = threadIdx.x ? s[threadIdx.x - 1] : 0.0;
  for (int k = 0; k < kScanItems; ++k)
    if (base + k < F) { run += cdf[base + k]; cdf[base + k] = run; }
  if (threadIdx.x == kThreads - 1) sums[blockIdx.x] = s[kThreads - 1];
}

// one workgroup: exclusive scan of the workgroup totals in place, running carry in chunk order
__global__ void __launch_bounds__(kThreads) cdf_sums_kernel(int nb, double* __restrict__ sums) {
  __shared__ double s[kThreads];
  double carry = 0.0;
  for (int c0 = 0; c0 < nb; c0 += kThreads) {
    const int i = c0 + threadIdx.x;
    const double v = i < nb ? sums[i] : 0.0;
    s[threadIdx.x] = v;
    __syncthreads();
    for (int off = 1; off < kThreads; off <<= 1) {
      const double w = threadIdx.x >= (unsigned)off ? s[threadIdx.x - off] : 0.0;
      __syncthreads();
      s[threadIdx.x] += w;
      __syncthreads();
    }
    if (i < nb) sums[i] = carry + (threadIdx.x ? s[threadIdx.x - 1] : 0.0);
    carry += s[kThreads - 1];
    __syncthreads();
  }
  if (threadIdx.x == 0) sums[nb] = carry;
}

__global__ void __launch_bounds__(kThreads) cdf_add_kernel(int F, double* __restrict__ cdf, const double* __restrict__ sums) {
  const int i = blockIdx.x * kThreads + threadIdx.x;
  if (i >= F) return;
  const int b = i / kScanBlock;
  if (b > 0) cdf[i] += sums[b];
}

__global__ void __launch_bounds__(kThreads) sample_kernel(int n, int V, int F, const float* __restrict__ xyz, const int32_t* __restrict__ tri,
                                                          const double* __restrict__ area, const double* __restrict__ cdf, uint64_t seed,
                                                          float* __restrict__ out,
                                                          int32_t* __restrict__ out_tri) {
  const int i = blockIdx.x * kThreads + threadIdx.x;
  if (i >= n) return;
  const double total = cdf[F - 1];
  if (!(total > 0.0)) {                     // refused on the host; keep the output defined
    out[3 * i] = out[3 * i + 1] = out[3 * i + 2] = NAN;
    out_tri[i] = -1;
    return;
  }
  double target = u53(hash3(seed, (uint64_t)i, 0)) * total;
  if (target >= total) target = nextafter(total, 0.0);
  // first f with cdf[f] > target: cdf[f - 1] <= target < cdf[f], so a face of zero area (cdf[f] == cdf[f - 1]) is not picked.
  // Where two scan segments meet, the CDF may step back or forward by an ulp (the segments' offsets are rounded on their own):
  // a zero-area face hit there moves to the next face of positive area (total > 0: one exists), within F steps.
  int lo = 0, hi = F - 1;
  while (lo < hi) {                         // <= 31 steps
    const int mid = (lo + hi) >> 1;
    if (cdf[mid] > target) hi = mid; else lo = mid + 1;
  }
  int f = lo;
  for (int s = 0; s < F && !(area[f] > 0.0); ++s) f = f + 1 < F ? f + 1 : 0;
  const int a = tri[3 * f], b = tri[3 * f + 1], c = tri[3 * f + 2];
  if (a < 0 || a >= V || b < 0 || b >= V || c < 0 || c >= V) {   // (a face of positive area has valid indices: area_kernel)
    out[3 * i] = out[3 * i + 1] = out[3 * i + 2] = NAN;
    out_tri[i] = -1;
    return;
  }
  const float r1 = u24(hash3(seed, (uint64_t)i, 1)), r2 = u24(hash3(seed, (uint64_t)i, 2));
  const float s = sqrtf(r1), wa = 1.f - s, wb = s * (1.f - r2), wc = s * r2;
#pragma unroll
  for (int k = 0; k < 3; ++k) out[3 * i + k] = wa * xyz[3 * a + k] + wb * xyz[3 * b + k] + wc * xyz[3 * c + k];
  out_tri[i] = f;
}

// ---- nearest-neighbour query over a point grid: outside queries, max_dist and index ties
// squared distance from q to the box [a, b] (per axis)
__device__ __forceinline__ float box_d2(const float q[3], const float a[3], const float b[3]) {
  float s = 0.f;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const float d = fmaxf(0.f, fmaxf(a[k] - q[k], q[k] - b[k]));
    s += d * d;
  }
  return s;
}

// one thread per query.  Ring r searches the cells of the box c +- r (clamped to the grid) that ring r - 1 did not; the walk ends
// when every point outside the searched box is provably farther than the best (the distance from q to the part of the target's
// bounding box beyond each open face, every box widened by eps for the rounding of cell coordinates), or, with max_dist, when
// they are all beyond max_dist.  r <= gmax covers the whole grid.  Ties (equal fp32 squared distance) go to the smaller index.
__global__ void __launch_bounds__(kThreads) nn_query_kernel(int nq, const float* __restrict__ query, PointXform T, float max_d2,
                                                            const PointGrid* __restrict__ Gp, const uint32_t* __restrict__ start,
                                                            const uint32_t* __restrict__ count, const float* __restrict__ sxyz,
                                                            const uint32_t* __restrict__ sidx, float* __restrict__ dist,
                                                            int32_t* __restrict__ idx) {
  const int t = blockIdx.x * kThreads + threadIdx.x;
  if (t >= nq) return;
  const PointGrid G = *Gp;
  const F3 p = apply(T, ld3(query + 3 * (size_t)t));
  const float q[3] = {p.x, p.y, p.z};
  const float eps = G.eps + kCellSlack * fmaxf(fabsf(q[0]), fmaxf(fabsf(q[1]), fabsf(q[2])));
  int c[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) c[k] = cell_coord(q[k], G.lo[k], G.inv_h, G.g[k]);
  float best = INFINITY;
  uint32_t bi = 0xffffffffu;
  int p0[3] = {1, 1, 1}, p1[3] = {0, 0, 0};       // previous box (empty)
  for (int r = 0; r <= G.gmax; ++r) {
    int b0[3], b1[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) { b0[k] = max(0, c[k] - r); b1[k] = min(G.g[k] - 1, c[k] + r); }
    for (int cz = b0[2]; cz <= b1[2]; ++cz)
      for (int cy = b0[1]; cy <= b1[1]; ++cy) {
        const int row = (cz * G.g[1] + cy) * G.g[0];
        const bool seen = cz >= p0[2] && cz <= p1[2] && cy >= p0[1] && cy <= p1[1];
        // x-ranges of this row not searched before: the whole row, or the parts left and right of the previous box
        for (int part = 0; part < 2; ++part) {
          int xa, xb;
          if (!seen) { if (part) break; xa = b0[0]; xb = b1[0]; }
          else if (part == 0) { xa = b0[0]; xb = p0[0] - 1; }
          else { xa = p1[0] + 1; xb = b1[0]; }
          if (xa > xb) continue;
          const uint32_t j0 = start[row + xa], j1 = start[row + xb] + count[row + xb];     // cells of one row are consecutive
          for (uint32_t j = j0; j < j1; ++j) {
            const float dx = sxyz[3 * j] - q[0], dy = sxyz[3 * j + 1] - q[1], dz = sxyz[3 * j + 2] - q[2];
            const float d = dx * dx + dy * dy + dz * dz;
            const uint32_t id = sidx[j];
            if (d < best || (d == best && id < bi)) { best = d; bi = id; }
          }
        }
      }
#pragma unroll
    for (int k = 0; k < 3; ++k) { p0[k] = b0[k]; p1[k] = b1[k]; }
    // lower bound on the squared distance to any point outside the searched box
    float bound = INFINITY;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      float a[3], b[3];
#pragma unroll
      for (int m = 0; m < 3; ++m) { a[m] = G.lo[m] - eps; b[m] = G.hi[m] + eps; }
      if (b0[k] > 0) {
        b[k] = G.lo[k] + (float)b0[k] * G.h + eps;
        bound = fminf(bound, box_d2(q, a, b));
        b[k] = G.hi[k] + eps;
      }
      if (b1[k] < G.g[k] - 1) {
        a[k] = G.lo[k] + (float)(b1[k] + 1) * G.h - eps;
        bound = fminf(bound, box_d2(q, a, b));
      }
    }
    if (bound == INFINITY) break;              // the whole grid has been searched
    if (best < bound || bound > max_d2) break;  // proven nearest, or everything unvisited is beyond max_dist
  }
  if (bi == 0xffffffffu || !(best <= max_d2)) { dist[t] = INFINITY; idx[t] = -1; }
  else { dist[t] = sqrtf(best); idx[t] = (int32_t)bi; }
}

// ---- fixed-order reductions (wave_sum_f64, block_partials: sgr_common.h)
__global__ void __launch_bounds__(kThreads) icp_partial_kernel(int n, const float* __restrict__ src, PointXform T, const int32_t* __restrict__ idx,
                                                               int nt, const float* __restrict__ tgt, double* __restrict__ parts) {
  double acc[kIcpSums];
#pragma unroll
  for (int k = 0; k < kIcpSums; ++k) acc[k] = 0.0;
  for (int i = blockIdx.x * kThreads + threadIdx.x; i < n; i += kRedBlocks * kThreads) {
    const int j = idx[i];
    if (j < 0 || j >= nt) continue;
    const F3 pf = apply(T, ld3(src + 3 * (size_t)i));
    const double p[3] = {pf.x, pf.y, pf.z}, q[3] = {tgt[3 * (size_t)j], tgt[3 * (size_t)j + 1], tgt[3 * (size_t)j + 2]};
    acc[0] += 1.0;
    acc[1] += (p[0] - q[0]) * (p[0] - q[0]) + (p[1] - q[1]) * (p[1] - q[1]) + (p[2] - q[2]) * (p[2] - q[2]);
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      acc[2 + a] += p[a];
      acc[5 + a] += q[a];
#pragma unroll
      for (int b = 0; b < 3; ++b) acc[8 + 3 * a + b] += p[a] * q[b];
    }
  }
  block_partials<kIcpSums>(acc, parts + (size_t)blockIdx.x * kIcpSums);
}

__global__ void __launch_bounds__(kThreads) metrics_partial_kernel(int na, const float* __restrict__ da, int nb, const float* __restrict__ db,
                                                                   float tau, double* __restrict__ parts) {
  const bool second = blockIdx.x >= kRedBlocks;
  const int n = second ? nb : na;
  const float* __restrict__ d = second ? db : da;
  double acc[2] = {0.0, 0.0};
  for (int i = (blockIdx.x % kRedBlocks) * kThreads + threadIdx.x; i < n; i += kRedBlocks * kThreads) {
    const float v = d[i];
    acc[0] += (double)v;
    acc[1] += v < tau ? 1.0 : 0.0;
  }
  block_partials<2>(acc, parts + (size_t)blockIdx.x * 2);
}

// one workgroup: out[k] = sum over the partial rows b = 0, 1, ... in order (rows of `width` doubles; `groups` runs of kRedBlocks rows)
__global__ void __launch_bounds__(kThreads) reduce_final_kernel(int width, int groups, const double* __restrict__ parts, double* __restrict__ out) {
  const int k = threadIdx.x;
  if (k >= width * groups) return;
  const int g = k / width, w = k % width;
  double s = 0.0;
  for (int b = 0; b < kRedBlocks; ++b) s += parts[((size_t)g * kRedBlocks + b) * width + w];
  out[k] = s;
}

inline size_t sample_bytes(int F) { const size_t nb = (size_t)(F + kScanBlock - 1) / kScanBlock; return 2 * align_up((size_t)F * 8) + align_up((nb + 1) * 8); }

inline bool finite12(const float* m) {
  if (!m) return true;
  for (int k = 0; k < 12; ++k) if (!std::isfinite(m[k])) return false;
  return true;
}

}  // namespace
}  // namespace sgr

using namespace sgr;

extern "C" {

size_t sgr_surface_sample_bytes(int32_t F) {
  if (F < 0) return 0;
  return sample_bytes(F);
}

int sgr_surface_sample(int32_t V, int32_t F, const float* vertices, const int32_t* triangles, int32_t n, uint64_t seed, void* scratch,
                       size_t scratch_bytes, float* points, int32_t* tri_idx, double* total_area, void* stream) {
  if (V <= 0 || F <= 0 || n < 0 || !vertices || !triangles || (n > 0 && (!points || !tri_idx)))
    return set_error(SGR_ERR_INVALID, "surface_sample: bad arguments (V=%d F=%d n=%d)", V, F, n);
  if (!scratch || scratch_bytes < sample_bytes(F)) return set_error(SGR_ERR_WORKSPACE, "surface_sample: scratch too small");
  hipStream_t st = (hipStream_t)stream;
  double* area = (double*)scratch;
  double* cdf = (double*)((char*)scratch + align_up((size_t)F * 8));
  double* sums = (double*)((char*)scratch + 2 * align_up((size_t)F * 8));
  const int nb = (F + kScanBlock - 1) / kScanBlock;
  hipLaunchKernelGGL(area_kernel, dim3(blocks_for(F)), dim3(kThreads), 0, st, V, F, vertices, triangles, area, cdf);
  hipLaunchKernelGGL(cdf_local_kernel, dim3(nb), dim3(kThreads), 0, st, F, cdf, sums);
  hipLaunchKernelGGL(cdf_sums_kernel, dim3(1), dim3(kThreads), 0, st, nb, sums);
  hipLaunchKernelGGL(cdf_add_kernel, dim3(blocks_for(F)), dim3(kThreads), 0, st, F, cdf, sums);
  if (n > 0)
    hipLaunchKernelGGL(sample_kernel, dim3(blocks_for(n)), dim3(kThreads), 0, st, n, V, F, vertices, triangles, area, cdf, seed, points,
                       tri_idx);
  if (total_area && hipMemcpyAsync(total_area, cdf + (F - 1), 8, hipMemcpyDeviceToDevice, st) != hipSuccess)
    return set_error(SGR_ERR_HIP, "surface_sample: copy");
  return hipGetLastError() == hipSuccess ? SGR_OK : set_error(SGR_ERR_HIP, "surface_sample launch failed");
}

size_t sgr_nn_grid_bytes(int32_t n) {
  if (n <= 0) return 0;
  return point_grid_bytes(n);
}

int sgr_nn_grid_build(int32_t n, const float* points, const float* transform, void* grid, size_t grid_bytes, void* stream) {
  if (n <= 0 || !points) return set_error(SGR_ERR_INVALID, "nn_grid_build: bad arguments (n=%d)", n);
  if (!grid || grid_bytes < point_grid_bytes(n)) return set_error(SGR_ERR_WORKSPACE, "nn_grid_build: grid buffer too small");
  if (!finite12(transform)) return set_error(SGR_ERR_INVALID, "nn_grid_build: transform is not finite");
  if (!build_point_grid(n, points, transform, grid, (hipStream_t)stream)) return set_error(SGR_ERR_HIP, "nn_grid_build: grid build failed");
  return SGR_OK;
}

int sgr_nn_query(int32_t n, const void* grid, size_t grid_bytes, int32_t nq, const float* query, const float* transform, float max_dist,
                 float* dist, int32_t* idx, void* stream) {
  if (n <= 0 || nq < 0 || (nq > 0 && (!query || !dist || !idx)) || !(max_dist >= 0.f))
    return set_error(SGR_ERR_INVALID, "nn_query: bad arguments (n=%d nq=%d)", n, nq);
  if (!grid || grid_bytes < point_grid_bytes(n)) return set_error(SGR_ERR_WORKSPACE, "nn_query: grid buffer too small");
  if (!finite12(transform)) return set_error(SGR_ERR_INVALID, "nn_query: transform is not finite");
  if (nq == 0) return SGR_OK;
  const GridBlob b = carve_grid((void*)grid, n);
  const float max_d2 = std::isinf(max_dist) ? INFINITY : max_dist * max_dist;
  hipLaunchKernelGGL(nn_query_kernel, dim3(blocks_for(nq)), dim3(kThreads), 0, (hipStream_t)stream, nq, query, point_xform(transform), max_d2,
                     b.grid, b.start, b.count, b.sxyz, b.sidx, dist, idx);
  return hipGetLastError() == hipSuccess ? SGR_OK : set_error(SGR_ERR_HIP, "nn_query launch failed");
}

size_t sgr_eval_reduce_bytes(void) { return align_up((size_t)kRedBlocks * kIcpSums * 8); }

int sgr_icp_accumulate(int32_t n, const float* source, const float* transform, const int32_t* idx, int32_t n_target, const float* target,
                       double* sums, void* scratch, size_t scratch_bytes, void* stream) {
  if (n < 0 || n_target <= 0 || !target || !sums || (n > 0 && (!source || !idx)))
    return set_error(SGR_ERR_INVALID, "icp_accumulate: bad arguments (n=%d n_target=%d)", n, n_target);
  if (!scratch || scratch_bytes < sgr_eval_reduce_bytes()) return set_error(SGR_ERR_WORKSPACE, "icp_accumulate: scratch too small");
  if (!finite12(transform)) return set_error(SGR_ERR_INVALID, "icp_accumulate: transform is not finite");
  hipStream_t st = (hipStream_t)stream;
  double* parts = (double*)scratch;
  hipLaunchKernelGGL(icp_partial_kernel, dim3(kRedBlocks), dim3(kThreads), 0, st, n, source, point_xform(transform), idx, n_target, target, parts);
  hipLaunchKernelGGL(reduce_final_kernel, dim3(1), dim3(kThreads), 0, st, kIcpSums, 1, parts, sums);
  return hipGetLastError() == hipSuccess ? SGR_OK : set_error(SGR_ERR_HIP, "icp_accumulate launch failed");
}

int sgr_cloud_metrics(int32_t na, const float* dist_a, int32_t nb, const float* dist_b, float thresh, double* out, void* scratch,
                      size_t scratch_bytes, void* stream) {
  if (na < 0 || nb < 0 || !out || (na > 0 && !dist_a) || (nb > 0 && !dist_b) || !(thresh > 0.f))
    return set_error(SGR_ERR_INVALID, "cloud_metrics: bad arguments (na=%d nb=%d)", na, nb);
  if (!scratch || scratch_bytes < sgr_eval_reduce_bytes()) return set_error(SGR_ERR_WORKSPACE, "cloud_metrics: scratch too small");
  hipStream_t st = (hipStream_t)stream;
  double* parts = (double*)scratch;
  hipLaunchKernelGGL(metrics_partial_kernel, dim3(2 * kRedBlocks), dim3(kThreads), 0, st, na, dist_a, nb, dist_b, thresh, parts);
  hipLaunchKernelGGL(reduce_final_kernel, dim3(1), dim3(kThreads), 0, st, 2, 2, parts, out);   // sum d_a, #(d_a < tau), sum d_b, #(d_b < tau)
  return hipGetLastError() == hipSuccess ? SGR_OK : set_error(SGR_ERR_HIP, "cloud_metrics launch failed");
}

}  // extern "C"
