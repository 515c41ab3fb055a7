// Trajectory scoring of the reference's terminate() (/root/reference/src/utils/eval_traj.py: align_kf_traj, align_full_traj,
// traj_eval_and_plot; evo's umeyama_alignment and APE of the translation part), DESIGN.md section 3, "Trajectory scoring":
//   sgr_traj_accumulate    camera centres of the estimate and the reference, the skip rule, and the 17 fp64 sums of the scaled Umeyama
//                          fit (the 3 x 3 SVD runs on the host): 2 launches
//   sgr_traj_errors        e_i = |s R x_i + t - y_i|, their sums, extrema, the two middle order statistics and the centred sum: 2 launches
// n is a few thousand at most (2 000 frames, 512 keyframes), so both are laid out for latency: launch 1 is one pair per thread (a wave
// stages its 64 rows through LDS with coalesced loads) and leaves per-workgroup partials; launch 2 is ONE workgroup of 1024 threads that
// merges the partials in workgroup order, makes the centred pass over all pairs and the exact selection.  No float atomics, one fixed
// order of additions: bitwise reproducible.  The order statistics are selected on the fp64 bit patterns (non-negative doubles order as
// unsigned integers) with 8-bit digits: 65 535 doubles do not fit the LDS, so a sort there would need a second path for large n.
#include <cmath>
#include <cstdint>

#include "sgr_common.h"
#include "sgr_se3_device.h"

namespace sgr {
int set_error(int code, const char* fmt, ...);

namespace {

constexpr int kThreads = 256, kWaves = kThreads / 64;      // launch 1: one pair per thread
constexpr int kWide = 1024, kWideWaves = kWide / 64;       // launch 2: one workgroup
constexpr int kPartRow = 8;                                // doubles per workgroup partial (7 of accumulate, 5 of errors)
constexpr int kFitSums = 7, kCentredSums = 10, kErrSums = 3;

inline int blocks(int n) { return (n + kThreads - 1) / kThreads; }
inline size_t parts_bytes(int n) { return align_up((size_t)blocks(n) * kPartRow * 8); }
inline size_t total_bytes(int n) { return parts_bytes(n) + align_up((size_t)n * 8); }

struct Sim3 { double s, r[9], t[3]; };

// The wave's `cnt` rows base .. base + cnt - 1 (through rows[] when given) of m [., 16]: four 16-byte loads per lane, a row's four
// quarters on four neighbouring lanes.  t[r] = (m[3], m[7], m[11], .) of row r, fin[4 r + q] = quarter q of row r is finite.
__device__ __forceinline__ void stage_mat4(const float* __restrict__ m, const int64_t* __restrict__ rows, int base, int cnt, int lane,
                                           float (*t)[4], uint8_t* fin) {
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int q = lane + 64 * k, r = q >> 2, part = q & 3;
    if (r < cnt) {
      const int64_t row = rows ? rows[base + r] : (int64_t)(base + r);
      const float4 v = ((const float4*)m)[row * 4 + part];
      t[r][part] = v.w;
      fin[q] = isfinite(v.x) && isfinite(v.y) && isfinite(v.z) && isfinite(v.w);
    }
  }
}

// launch 1 of sgr_traj_accumulate: pos, valid and the workgroup's partial of (count, sum x, sum y) over the valid pairs
template <int KIND>
__global__ void __launch_bounds__(kThreads) traj_centres_kernel(int n, const float* __restrict__ est, const int64_t* __restrict__ rows,
                                                                const float* __restrict__ ref, double* __restrict__ pos,
                                                                uint8_t* __restrict__ valid, double* __restrict__ parts) {
  __shared__ float s_pose[kWaves][64 * 7];
  __shared__ float s_t[2][kWaves][64][4];
  __shared__ uint8_t s_fin[2][kWaves][256];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int base = blockIdx.x * kThreads + wv * 64, cnt = min(64, n - base);
  const int i = base + lane;
  if (KIND == SGR_TRAJ_POSE7_W2C) {
#pragma unroll
    for (int k = 0; k < 7; ++k) {             // 448 consecutive floats of 64 consecutive rows
      const int e = lane + 64 * k, r = e / 7, c = e - 7 * r;
      if (r < cnt) s_pose[wv][e] = est[(rows ? rows[base + r] : (int64_t)(base + r)) * 7 + c];
    }
  } else {
    stage_mat4(est, rows, base, cnt, lane, s_t[1][wv], s_fin[1][wv]);
  }
  stage_mat4(ref, nullptr, base, cnt, lane, s_t[0][wv], s_fin[0][wv]);
  __syncthreads();
  double acc[kFitSums];
#pragma unroll
  for (int k = 0; k < kFitSums; ++k) acc[k] = 0.0;
  if (i < n) {
    float x[3];
    if (KIND == SGR_TRAJ_POSE7_W2C) {
      const Pose c2w = pose_inv(load_pose(&s_pose[wv][7 * lane]));      // the arithmetic of se3_inv: the same bits
      x[0] = c2w.t[0]; x[1] = c2w.t[1]; x[2] = c2w.t[2];
    } else {
      x[0] = s_t[1][wv][lane][0]; x[1] = s_t[1][wv][lane][1]; x[2] = s_t[1][wv][lane][2];
    }
    const uint8_t* f = &s_fin[0][wv][4 * lane];
    const bool ok = f[0] && f[1] && f[2] && f[3];
    valid[i] = ok ? 1 : 0;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const double xk = (double)x[k], yk = (double)s_t[0][wv][lane][k];
      pos[6 * (size_t)i + k] = xk;
      pos[6 * (size_t)i + 3 + k] = yk;
      if (ok) { acc[1 + k] = xk; acc[4 + k] = yk; }
    }
    if (ok) acc[0] = 1.0;
  }
  block_partials<kFitSums, kWaves>(acc, parts + (size_t)blockIdx.x * kPartRow);
}

// launch 2 of sgr_traj_accumulate, one workgroup: the partials in workgroup order, the means, then the centred sums
__global__ void __launch_bounds__(kWide) traj_centred_kernel(int n, int nb, const double* __restrict__ pos, const uint8_t* __restrict__ valid,
                                                             const double* __restrict__ parts, double* __restrict__ sums) {
  __shared__ double s_fit[kFitSums], s_cen[kCentredSums];
  if (threadIdx.x < kFitSums) {
    double s = 0.0;
    for (int b = 0; b < nb; ++b) s += parts[(size_t)b * kPartRow + threadIdx.x];
    s_fit[threadIdx.x] = s;
  }
  __syncthreads();
  const double cnt = s_fit[0];
  double mx[3], my[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) { mx[k] = s_fit[1 + k] / cnt; my[k] = s_fit[4 + k] / cnt; }      // (count 0: no pair reads them)
  double acc[kCentredSums];
#pragma unroll
  for (int k = 0; k < kCentredSums; ++k) acc[k] = 0.0;
  for (int i = threadIdx.x; i < n; i += kWide) {
    if (!valid[i]) continue;
    double dx[3], dy[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) { dx[k] = pos[6 * (size_t)i + k] - mx[k]; dy[k] = pos[6 * (size_t)i + 3 + k] - my[k]; }
    acc[0] += dx[0] * dx[0] + dx[1] * dx[1] + dx[2] * dx[2];
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
      for (int b = 0; b < 3; ++b) acc[1 + 3 * a + b] += dy[a] * dx[b];
  }
  block_partials<kCentredSums, kWideWaves>(acc, s_cen);
  __syncthreads();
  if (threadIdx.x < kFitSums) sums[threadIdx.x] = s_fit[threadIdx.x];
  else if (threadIdx.x < kFitSums + kCentredSums) sums[threadIdx.x] = s_cen[threadIdx.x - kFitSums];
}

__device__ __forceinline__ double wave_min_f64(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = fmin(v, __shfl_xor(v, off));
  return v;
}
__device__ __forceinline__ double wave_max_f64(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = fmax(v, __shfl_xor(v, off));
  return v;
}

// launch 1 of sgr_traj_errors: err and the workgroup's partial of (count, sum e, sum e^2, min, max) over the valid pairs
__global__ void __launch_bounds__(kThreads) traj_errors_kernel(int n, const double* __restrict__ pos, const uint8_t* __restrict__ valid, Sim3 T,
                                                               double* __restrict__ err, double* __restrict__ parts) {
  __shared__ double s_mm[2][kWaves];
  const int i = blockIdx.x * kThreads + threadIdx.x, lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  double acc[kErrSums] = {0.0, 0.0, 0.0}, lo = INFINITY, hi = -INFINITY;
  if (i < n) {
    double e = NAN;
    if (valid[i]) {
      const double* p = pos + 6 * (size_t)i;
      double q = 0.0;
#pragma unroll
      for (int a = 0; a < 3; ++a) {
        const double z = T.s * (T.r[3 * a] * p[0] + T.r[3 * a + 1] * p[1] + T.r[3 * a + 2] * p[2]) + T.t[a] - p[3 + a];
        q += z * z;
      }
      e = sqrt(q);
      acc[0] = 1.0; acc[1] = e; acc[2] = e * e;
      lo = hi = e;
    }
    err[i] = e;
  }
  lo = wave_min_f64(lo); hi = wave_max_f64(hi);
  if (lane == 0) { s_mm[0][wv] = lo; s_mm[1][wv] = hi; }
  double* out = parts + (size_t)blockIdx.x * kPartRow;
  block_partials<kErrSums, kWaves>(acc, out);                 // (its barrier also covers s_mm)
  if (threadIdx.x == 0) {
    out[3] = fmin(fmin(s_mm[0][0], s_mm[0][1]), fmin(s_mm[0][2], s_mm[0][3]));
    out[4] = fmax(fmax(s_mm[1][0], s_mm[1][1]), fmax(s_mm[1][2], s_mm[1][3]));
  }
}

// launch 2 of sgr_traj_errors, one workgroup: the partials in workgroup order, the centred sum, and the order statistics of rank
// (m - 1) / 2 and m / 2 among the m valid errors: a radix select over the bit patterns, most significant byte first (a histogram of
// the keys that share the bytes chosen so far, by integer LDS atomics; wave 0 scans it for the bin that holds the rank), then one
// pass for the upper one: the same value when more than m / 2 keys are <= it, the smallest larger key otherwise.
__global__ void __launch_bounds__(kWide) traj_stats_kernel(int n, int nb, const double* __restrict__ err, const uint8_t* __restrict__ valid,
                                                           const double* __restrict__ parts, double* __restrict__ stats) {
  __shared__ double s_sum[kErrSums + 2], s_cen[1];
  __shared__ uint32_t s_hist[256], s_bin, s_rank, s_le;
  __shared__ unsigned long long s_gt;
  const int tid = threadIdx.x;
  if (tid < kErrSums + 2) {
    double s = tid == 3 ? INFINITY : (tid == 4 ? -INFINITY : 0.0);
    for (int b = 0; b < nb; ++b) {
      const double v = parts[(size_t)b * kPartRow + tid];
      s = tid == 3 ? fmin(s, v) : (tid == 4 ? fmax(s, v) : s + v);
    }
    s_sum[tid] = s;
  }
  if (tid == 0) { s_le = 0u; s_gt = ~0ull; }
  __syncthreads();
  const uint32_t m = (uint32_t)s_sum[0];
  const double mean = s_sum[1] / s_sum[0];
  double acc[1] = {0.0};
  for (int i = tid; i < n; i += kWide)
    if (valid[i]) { const double d = err[i] - mean; acc[0] += d * d; }
  block_partials<1, kWideWaves>(acc, s_cen);
  uint64_t prefix = 0;
  uint32_t rank = m ? (m - 1) / 2 : 0u;
  if (m) {                                            // (m is the same in every thread)
    for (int shift = 56; shift >= 0; shift -= 8) {
      if (tid < 256) s_hist[tid] = 0u;
      __syncthreads();
      for (int i = tid; i < n; i += kWide) {
        if (!valid[i]) continue;
        const uint64_t key = (uint64_t)__double_as_longlong(err[i]);
        if (shift == 56 || (key >> (shift + 8)) == prefix) atomicAdd(&s_hist[(key >> shift) & 255u], 1u);
      }
      __syncthreads();
      if (tid < 64) {
        uint32_t c[4], s = 0u;
#pragma unroll
        for (int j = 0; j < 4; ++j) { c[j] = s_hist[4 * tid + j]; s += c[j]; }
        const uint32_t inc = wave_scan_add_u32(s), exc = inc - s;
        if (exc <= rank && rank < inc) {              // one lane: the counts of a pass add up to more than the rank
          uint32_t r = rank - exc;
          int b = 0;
          while (b < 3 && r >= c[b]) { r -= c[b]; ++b; }
          s_bin = 4u * tid + b;
          s_rank = r;
        }
      }
      __syncthreads();
      prefix = (prefix << 8) | s_bin;
      rank = s_rank;
    }
    uint32_t le = 0u;
    uint64_t gt = ~0ull;
    for (int i = tid; i < n; i += kWide) {
      if (!valid[i]) continue;
      const uint64_t key = (uint64_t)__double_as_longlong(err[i]);
      if (key <= prefix) ++le; else gt = key < gt ? key : gt;
    }
    atomicAdd(&s_le, le);
    atomicMin(&s_gt, (unsigned long long)gt);
  }
  __syncthreads();
  if (tid == 0) {
    const double nan = NAN;
    stats[0] = s_sum[0]; stats[1] = s_sum[1]; stats[2] = s_sum[2];
    stats[3] = m ? s_sum[3] : nan;
    stats[4] = m ? s_sum[4] : nan;
    stats[5] = m ? __longlong_as_double((long long)prefix) : nan;
    stats[6] = m ? __longlong_as_double((long long)(s_le > m / 2 ? prefix : (uint64_t)s_gt)) : nan;
    stats[7] = s_cen[0];
  }
}

inline bool supported(int n) { return n >= 1 && n <= SGR_TRAJ_MAX_POSES; }

}  // namespace
}  // namespace sgr

using namespace sgr;

extern "C" {

size_t sgr_traj_scratch_bytes(int32_t n) { return supported(n) ? total_bytes(n) : 0; }

int sgr_traj_accumulate(int32_t kind, const float* est, int32_t est_rows, const int64_t* inds, int32_t n, const float* ref, double* pos,
                        uint8_t* valid, double* sums, void* scratch, size_t scratch_bytes, void* stream) {
  if (!supported(n) || (kind != SGR_TRAJ_POSE7_W2C && kind != SGR_TRAJ_MAT4_C2W) || !est || est_rows < 1 || !ref || !pos || !valid || !sums)
    return set_error(SGR_ERR_INVALID, "traj_accumulate: bad arguments (kind=%d n=%d est_rows=%d)", kind, n, est_rows);
  if (((uintptr_t)ref & 15) || (kind == SGR_TRAJ_MAT4_C2W && ((uintptr_t)est & 15)))
    return set_error(SGR_ERR_INVALID, "traj_accumulate: 4 x 4 rows must be 16-byte aligned");
  if (!scratch || scratch_bytes < total_bytes(n)) return set_error(SGR_ERR_WORKSPACE, "traj_accumulate: scratch too small");
  if (!inds && n > est_rows) return set_error(SGR_ERR_INVALID, "traj_accumulate: n=%d rows of an estimate of %d", n, est_rows);
  for (int i = 0; inds && i < n; ++i)
    if (inds[i] < 0 || inds[i] >= est_rows)
      return set_error(SGR_ERR_INVALID, "traj_accumulate: inds[%d]=%lld outside [0, %d)", i, (long long)inds[i], est_rows);
  hipStream_t st = (hipStream_t)stream;
  double* parts = (double*)scratch;
  int64_t* rows = nullptr;
  if (inds) {
    rows = (int64_t*)((char*)scratch + parts_bytes(n));
    if (hipMemcpyAsync(rows, inds, (size_t)n * 8, hipMemcpyHostToDevice, st) != hipSuccess)
      return set_error(SGR_ERR_HIP, "traj_accumulate: copy of inds");
  }
  const int nb = blocks(n);
  if (kind == SGR_TRAJ_POSE7_W2C)
    hipLaunchKernelGGL(traj_centres_kernel<SGR_TRAJ_POSE7_W2C>, dim3(nb), dim3(kThreads), 0, st, n, est, rows, ref, pos, valid, parts);
  else
    hipLaunchKernelGGL(traj_centres_kernel<SGR_TRAJ_MAT4_C2W>, dim3(nb), dim3(kThreads), 0, st, n, est, rows, ref, pos, valid, parts);
  hipLaunchKernelGGL(traj_centred_kernel, dim3(1), dim3(kWide), 0, st, n, nb, pos, valid, parts, sums);
  return hipGetLastError() == hipSuccess ? SGR_OK : set_error(SGR_ERR_HIP, "traj_accumulate launch failed");
}

int sgr_traj_errors(int32_t n, const double* pos, const uint8_t* valid, const double* sim3, double* err, double* stats, void* scratch,
                    size_t scratch_bytes, void* stream) {
  if (!supported(n) || !pos || !valid || !sim3 || !err || !stats) return set_error(SGR_ERR_INVALID, "traj_errors: bad arguments (n=%d)", n);
  if (!scratch || scratch_bytes < total_bytes(n)) return set_error(SGR_ERR_WORKSPACE, "traj_errors: scratch too small");
  Sim3 T;
  T.s = sim3[0];
  for (int k = 0; k < 9; ++k) T.r[k] = sim3[1 + k];
  for (int k = 0; k < 3; ++k) T.t[k] = sim3[10 + k];
  hipStream_t st = (hipStream_t)stream;
  double* parts = (double*)scratch;
  const int nb = blocks(n);
  hipLaunchKernelGGL(traj_errors_kernel, dim3(nb), dim3(kThreads), 0, st, n, pos, valid, T, err, parts);
  hipLaunchKernelGGL(traj_stats_kernel, dim3(1), dim3(kWide), 0, st, n, nb, err, valid, parts, stats);
  return hipGetLastError() == hipSuccess ? SGR_OK : set_error(SGR_ERR_HIP, "traj_errors launch failed");
}

}  // extern "C"
