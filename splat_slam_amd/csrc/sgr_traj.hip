// Trajectory scoring of the reference's terminate() (/root/reference/src/utils/eval_traj.py: align_kf_traj, align_full_traj,
// traj_eval_and_plot; evo's umeyama_alignment and APE of the translation part), DESIGN.md section 3, "Trajectory scoring":
//   sgr_traj_accumulate    camera centres of the estimate and the reference, the skip rule, and the 17 fp64 sums of the scaled Umeyama
//                          fit (the 3 x 3 SVD runs on the host): 2 launches
//   sgr_traj_errors        e_i = |s R x_i + t - y_i|, their sums, extrema, the two middle order statistics and the centred sum: 2 launches
//   sgr_traj_associate     the nearest stamp of b for every stamp of a (evo's matching_time_indices), the order check of b and the
//                          matched pairs compacted in order: 2 launches
//   sgr_traj_pose_errors   pose-to-pose errors E = Q^-1 P or (Q_i^-1 Q_j)^-1 (P_i^-1 P_j) in fp64 under every pose relation, over the
//                          used poses ranked by an exclusive scan, and the statistics of sgr_traj_errors (the same code): 4 launches
// n is a few thousand at most (2 000 frames, 512 keyframes), so both are laid out for latency: launch 1 is one pair per thread (a wave
// stages its 64 rows through LDS with coalesced loads) and leaves per-workgroup partials; launch 2 is ONE workgroup of 1024 threads that
// merges the partials in workgroup order, makes the centred pass over all pairs and the exact selection.  No float atomics, one fixed
// order of additions: bitwise reproducible.  The order statistics are selected on the fp64 bit patterns (non-negative doubles order as
// unsigned integers) with 8-bit digits: 65 535 doubles do not fit the LDS, so a sort there would need a second path for large n.
#include <cmath>
#include <cstdint>

#include "sgr_common.h"
#include "sgr_scan.h"
#include "sgr_se3_device.h"

namespace sgr {
int set_error(int code, const char* fmt, ...);

namespace {

constexpr int kThreads = 256, kWaves = kThreads / 64;      // launch 1: one pair per thread
constexpr int kWide = 1024, kWideWaves = kWide / 64;       // launch 2: one workgroup
constexpr int kPartRow = 8;                                // doubles per workgroup partial (7 of accumulate, 5 of errors)
constexpr int kFitSums = 7, kCentredSums = 10, kErrSums = 3;

inline size_t parts_bytes(int n) { return align_up((size_t)blocks_for(n) * kPartRow * 8); }
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
// This is the body of the statistics launch of sgr_traj_errors and of sgr_traj_pose_errors: valid(i) says whether err[i] counts.
struct ValidFlags {
  const uint8_t* __restrict__ v;
  __device__ __forceinline__ bool operator()(int i) const { return v[i] != 0; }
};
struct ValidFirst {                      // the first m of n: the items of sgr_traj_pose_errors
  int m;
  __device__ __forceinline__ bool operator()(int i) const { return i < m; }
};

template <typename Valid>
__device__ __forceinline__ void traj_stats_body(int n, int nb, const double* __restrict__ err, const Valid valid,
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
    if (valid(i)) { const double d = err[i] - mean; acc[0] += d * d; }
  block_partials<1, kWideWaves>(acc, s_cen);
  uint64_t prefix = 0;
  uint32_t rank = m ? (m - 1) / 2 : 0u;
  if (m) {                                            // (m is the same in every thread)
    for (int shift = 56; shift >= 0; shift -= 8) {
      if (tid < 256) s_hist[tid] = 0u;
      __syncthreads();
      for (int i = tid; i < n; i += kWide) {
        if (!valid(i)) continue;
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
      if (!valid(i)) continue;
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

__global__ void __launch_bounds__(kWide) traj_stats_kernel(int n, int nb, const double* __restrict__ err, const uint8_t* __restrict__ valid,
                                                           const double* __restrict__ parts, double* __restrict__ stats) {
  traj_stats_body(n, nb, err, ValidFlags{valid}, parts, stats);
}

// launch 4 of sgr_traj_pose_errors: the same statistics over the first header[0] entries of err
__global__ void __launch_bounds__(kWide) traj_item_stats_kernel(int n, int nb, const double* __restrict__ err, const int32_t* __restrict__ header,
                                                                const double* __restrict__ parts, double* __restrict__ stats) {
  traj_stats_body(n, nb, err, ValidFirst{header[0]}, parts, stats);
}

// ---- sgr_traj_associate ------------------------------------------------------------------------------------------------------------
constexpr int kOrderBlocksMax = 1024;      // launch 1 has at least blocks_for(na) workgroups and up to this many for the order check of b
inline int assoc_blocks(int na, int nb) {
  const int order = blocks_for(nb) < kOrderBlocksMax ? blocks_for(nb) : kOrderBlocksMax;
  return blocks_for(na) > order ? blocks_for(na) : order;
}

// launch 1: thread i < na searches a[i]; ALL threads of the grid stride over j < nb - 1 for the order check.  flags[block] = 1 iff the
// workgroup met a pair out of order.  The search stays inside [0, nb) whatever the order of b is.
__global__ void __launch_bounds__(kThreads) traj_associate_kernel(int na, const double* __restrict__ a, int nb, const double* __restrict__ b,
                                                                  double off, double max_diff, int32_t* __restrict__ match,
                                                                  int32_t* __restrict__ flags) {
  __shared__ int s_bad[kWaves];
  const int i = blockIdx.x * kThreads + threadIdx.x, lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  int bad = 0;
  for (int64_t j = i; j < (int64_t)nb - 1; j += (int64_t)gridDim.x * kThreads) bad |= !(b[j + 1] >= b[j]);
  if (nb == 1 && i == 0) bad |= !(b[0] == b[0]);
  if (i < na) {
    const double t = a[i];
    int lo = 0, hi = nb;                                   // the first j with b[j] + off >= t (nb: none)
    while (lo < hi) {
      const int mid = lo + ((hi - lo) >> 1);
      if (b[mid] + off >= t) hi = mid; else lo = mid + 1;
    }
    int j = lo < nb ? lo : nb - 1;
    double d = fabs(b[j] + off - t);
    if (lo > 0 && lo < nb) {                               // the neighbour below wins a tie: the lower index
      const double dl = fabs(b[lo - 1] + off - t);
      if (dl <= d) { d = dl; j = lo - 1; }
    }
    while (j > 0 && fabs(b[j - 1] + off - t) == d) --j;     // equal distances below: duplicates in b
    match[i] = d <= max_diff ? j : -1;
  }
  bad = __any(bad) ? 1 : 0;
  if (lane == 0) s_bad[wv] = bad;
  __syncthreads();
  if (threadIdx.x == 0) flags[blockIdx.x] = s_bad[0] | s_bad[1] | s_bad[2] | s_bad[3];
}

// launch 2, one workgroup: the flags of the workgroups, the compacted lists in the order of i, the header
__global__ void __launch_bounds__(kWide) traj_compact_kernel(int na, int nflags, const int32_t* __restrict__ match, const int32_t* __restrict__ flags,
                                                             int32_t* __restrict__ a_inds, int32_t* __restrict__ b_inds,
                                                             int32_t* __restrict__ header) {
  __shared__ uint32_t s_red[kWideWaves];
  __shared__ int s_bad;
  const int tid = threadIdx.x;
  if (tid == 0) s_bad = 0;
  __syncthreads();
  int bad = 0;
  for (int k = tid; k < nflags; k += kWide) bad |= flags[k];
  if (bad) atomicOr(&s_bad, 1);
  uint32_t base = 0u;
  for (int i0 = 0; i0 < na; i0 += kWide) {
    const int i = i0 + tid;
    const int j = i < na ? match[i] : -1;
    uint32_t total;
    const uint32_t r = base + block_exclusive_scan<kWideWaves>(j >= 0 ? 1u : 0u, s_red, total);
    if (j >= 0) { a_inds[r] = i; b_inds[r] = j; }
    base += total;
  }
  for (int k = (int)base + tid; k < na; k += kWide) { a_inds[k] = -1; b_inds[k] = -1; }
  __syncthreads();
  if (tid < SGR_TRAJ_HEADER_WORDS) header[tid] = tid == 0 ? (int32_t)base : (tid == 1 ? s_bad : 0);
}

// ---- sgr_traj_pose_errors ----------------------------------------------------------------------------------------------------------
struct Rt { double r[9], t[3]; };          // a rigid pose [R | t], R row-major
constexpr int kMatDoubles = 24;            // per pair in scratch: P (12) then Q (12)

// a^-1 b = [Ra^T Rb | Ra^T (tb - ta)]
__device__ __forceinline__ Rt rt_inv_mul(const Rt& a, const Rt& b) {
  Rt o;
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) o.r[3 * i + j] = a.r[i] * b.r[j] + a.r[3 + i] * b.r[3 + j] + a.r[6 + i] * b.r[6 + j];
  const double d[3] = {b.t[0] - a.t[0], b.t[1] - a.t[1], b.t[2] - a.t[2]};
#pragma unroll
  for (int i = 0; i < 3; ++i) o.t[i] = a.r[i] * d[0] + a.r[3 + i] * d[1] + a.r[6 + i] * d[2];
  return o;
}
__device__ __forceinline__ Rt load_rt(const double* __restrict__ p) {
  Rt o;
#pragma unroll
  for (int k = 0; k < 9; ++k) o.r[k] = p[k];
#pragma unroll
  for (int k = 0; k < 3; ++k) o.t[k] = p[9 + k];
  return o;
}
__device__ __forceinline__ bool finite4(const float4 v) { return isfinite(v.x) && isfinite(v.y) && isfinite(v.z) && isfinite(v.w); }
// rows 0 .. 2 of a row-major 4 x 4 as [R | t], widened; false where one of the 16 entries is not finite
__device__ __forceinline__ bool load_mat4(const float* __restrict__ m, int64_t row, Rt& o) {
  const float4* p = (const float4*)m + row * 4;
  const float4 r0 = p[0], r1 = p[1], r2 = p[2], r3 = p[3];
  o.r[0] = r0.x; o.r[1] = r0.y; o.r[2] = r0.z; o.t[0] = r0.w;
  o.r[3] = r1.x; o.r[4] = r1.y; o.r[5] = r1.z; o.t[1] = r1.w;
  o.r[6] = r2.x; o.r[7] = r2.y; o.r[8] = r2.z; o.t[2] = r2.w;
  return finite4(r0) && finite4(r1) && finite4(r2) && finite4(r3);
}

// launch 1: P and Q of every pair, its used flag, and the workgroup's count of used pairs
template <int KIND>
__global__ void __launch_bounds__(kThreads) traj_poses_kernel(int n, const float* __restrict__ est, int est_rows, const float* __restrict__ ref,
                                                              int ref_rows, const int32_t* __restrict__ est_inds,
                                                              const int32_t* __restrict__ ref_inds, Sim3 T, double* __restrict__ mats,
                                                              uint8_t* __restrict__ used, uint32_t* __restrict__ counts) {
  __shared__ uint32_t s_red[kWaves];
  const int i = blockIdx.x * kThreads + threadIdx.x;
  bool ok = false;
  if (i < n) {
    const int e = est_inds ? est_inds[i] : i, q = ref_inds ? ref_inds[i] : i;
    ok = e >= 0 && e < est_rows && q >= 0 && q < ref_rows;
    if (ok) {
      Rt Q, C;                                             // C: the estimate camera -> world
      ok = load_mat4(ref, q, Q);
      if (KIND == SGR_TRAJ_POSE7_W2C) {
        const float* p = est + (int64_t)e * 7;
        double v[7];
#pragma unroll
        for (int k = 0; k < 7; ++k) { v[k] = (double)p[k]; ok = ok && isfinite(p[k]); }
        const double nrm = sqrt(v[3] * v[3] + v[4] * v[4] + v[5] * v[5] + v[6] * v[6]);
        const double x = v[3] / nrm, y = v[4] / nrm, z = v[5] / nrm, w = v[6] / nrm;
        // R(q) of world -> camera, written transposed: the rotation of camera -> world
        C.r[0] = 1.0 - 2.0 * (y * y + z * z); C.r[3] = 2.0 * (x * y - z * w);       C.r[6] = 2.0 * (x * z + y * w);
        C.r[1] = 2.0 * (x * y + z * w);       C.r[4] = 1.0 - 2.0 * (x * x + z * z); C.r[7] = 2.0 * (y * z - x * w);
        C.r[2] = 2.0 * (x * z - y * w);       C.r[5] = 2.0 * (y * z + x * w);       C.r[8] = 1.0 - 2.0 * (x * x + y * y);
#pragma unroll
        for (int a = 0; a < 3; ++a) C.t[a] = -(C.r[3 * a] * v[0] + C.r[3 * a + 1] * v[1] + C.r[3 * a + 2] * v[2]);
      } else {
        ok = load_mat4(est, e, C) && ok;
      }
      double* out = mats + (size_t)i * kMatDoubles;
#pragma unroll
      for (int a = 0; a < 3; ++a) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          const double v = T.r[3 * a] * C.r[c] + T.r[3 * a + 1] * C.r[3 + c] + T.r[3 * a + 2] * C.r[6 + c];
          ok = ok && isfinite(v);
          out[3 * a + c] = v;
        }
        const double v = T.s * (T.r[3 * a] * C.t[0] + T.r[3 * a + 1] * C.t[1] + T.r[3 * a + 2] * C.t[2]) + T.t[a];
        ok = ok && isfinite(v);
        out[9 + a] = v;
      }
#pragma unroll
      for (int k = 0; k < 9; ++k) out[12 + k] = Q.r[k];
#pragma unroll
      for (int k = 0; k < 3; ++k) out[21 + k] = Q.t[k];
    }
    used[i] = ok ? 1 : 0;
  }
  uint32_t total;
  block256_exclusive_scan(ok ? 1u : 0u, s_red, total);
  if (threadIdx.x == 0) counts[blockIdx.x] = total;
}

// the number of items of c used pairs
__device__ __forceinline__ int item_count(int c, int mode, int delta, int all_pairs) {
  if (mode == SGR_TRAJ_ABSOLUTE) return c;
  if (all_pairs) return c > delta ? c - delta : 0;
  return c >= 1 ? (c - 1) / delta : 0;
}

// launch 2: rank_row[rank of pair i among the used] = i (the workgroup's base from the counts before it), the header by workgroup 0
__global__ void __launch_bounds__(kThreads) traj_ranks_kernel(int n, const uint8_t* __restrict__ used, const uint32_t* __restrict__ counts,
                                                              int mode, int delta, int all_pairs, int32_t* __restrict__ rank_row,
                                                              int32_t* __restrict__ header) {
  __shared__ uint32_t s_red[kWaves];
  const int i = blockIdx.x * kThreads + threadIdx.x, nb = gridDim.x;          // nb <= 256: one count per thread
  const uint32_t mine = (int)threadIdx.x < nb ? counts[threadIdx.x] : 0u;
  uint32_t base, all;                                       // the used pairs of the workgroups before this one, and of all
  block256_exclusive_scan(threadIdx.x < blockIdx.x ? mine : 0u, s_red, base);
  block256_exclusive_scan(mine, s_red, all);
  const bool ok = i < n && used[i];
  uint32_t here;
  const uint32_t r = block256_exclusive_scan(ok ? 1u : 0u, s_red, here);
  if (ok) rank_row[base + r] = i;
  if (blockIdx.x == 0 && threadIdx.x < SGR_TRAJ_HEADER_WORDS) {
    const int t = threadIdx.x;
    header[t] = t == 0 ? item_count((int)all, mode, delta, all_pairs) : (t == 1 ? (int)all : (t == 2 ? n - (int)all : 0));
  }
}

// launch 3: thread k < m forms item k's E and its error; the workgroup's partial of (count, sum e, sum e^2, min, max)
__global__ void __launch_bounds__(kThreads) traj_item_errors_kernel(int n, const double* __restrict__ mats, const int32_t* __restrict__ rank_row,
                                                                    const int32_t* __restrict__ header, int mode, int delta, int all_pairs,
                                                                    int relation, double* __restrict__ err, int32_t* __restrict__ pair_rows,
                                                                    double* __restrict__ parts) {
  __shared__ double s_mm[2][kWaves];
  const int k = blockIdx.x * kThreads + threadIdx.x, lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int m = header[0];
  double acc[kErrSums] = {0.0, 0.0, 0.0}, lo = INFINITY, hi = -INFINITY;
  if (k < n) {
    double e = NAN;
    int row_i = -1, row_j = -1;
    if (k < m) {
      Rt E;
      if (mode == SGR_TRAJ_ABSOLUTE) {
        row_i = rank_row[k];
        const double* p = mats + (size_t)row_i * kMatDoubles;
        E = rt_inv_mul(load_rt(p + 12), load_rt(p));
      } else {
        const int ri = all_pairs ? k : k * delta;
        row_i = rank_row[ri]; row_j = rank_row[ri + delta];
        const double *pi = mats + (size_t)row_i * kMatDoubles, *pj = mats + (size_t)row_j * kMatDoubles;
        const Rt A = rt_inv_mul(load_rt(pi + 12), load_rt(pj + 12)), B = rt_inv_mul(load_rt(pi), load_rt(pj));
        E = rt_inv_mul(A, B);
      }
      if (relation == SGR_TRAJ_TRANSLATION_PART) {
        e = sqrt(E.t[0] * E.t[0] + E.t[1] * E.t[1] + E.t[2] * E.t[2]);
      } else if (relation == SGR_TRAJ_ROTATION_ANGLE_RAD || relation == SGR_TRAJ_ROTATION_ANGLE_DEG) {
        const double a0 = E.r[7] - E.r[5], a1 = E.r[2] - E.r[6], a2 = E.r[3] - E.r[1];
        e = atan2(sqrt(a0 * a0 + a1 * a1 + a2 * a2), E.r[0] + E.r[4] + E.r[8] - 1.0);
        if (relation == SGR_TRAJ_ROTATION_ANGLE_DEG) e *= 57.29577951308232;          // 180 / pi
      } else {
        double q = 0.0;
#pragma unroll
        for (int c = 0; c < 9; ++c) { const double d = E.r[c] - ((c & 3) == 0 ? 1.0 : 0.0); q += d * d; }
        if (relation == SGR_TRAJ_FULL_TRANSFORMATION) q += E.t[0] * E.t[0] + E.t[1] * E.t[1] + E.t[2] * E.t[2];
        e = sqrt(q);
      }
      acc[0] = 1.0; acc[1] = e; acc[2] = e * e;
      lo = hi = e;
    }
    err[k] = e;
    pair_rows[2 * k] = row_i; pair_rows[2 * k + 1] = row_j;
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

inline bool supported(int n) { return n >= 1 && n <= SGR_TRAJ_MAX_POSES; }
inline size_t assoc_bytes(int na, int nb) { return align_up((size_t)assoc_blocks(na, nb) * 4); }
// parts | counts | used | rank_row | mats
inline size_t pe_counts_off(int n) { return parts_bytes(n); }
inline size_t pe_used_off(int n) { return pe_counts_off(n) + align_up((size_t)blocks_for(n) * 4); }
inline size_t pe_rank_off(int n) { return pe_used_off(n) + align_up((size_t)n); }
inline size_t pe_mats_off(int n) { return pe_rank_off(n) + align_up((size_t)n * 4); }
inline size_t pe_bytes(int n) { return pe_mats_off(n) + align_up((size_t)n * kMatDoubles * 8); }

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
  const int nb = blocks_for(n);
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
  const int nb = blocks_for(n);
  hipLaunchKernelGGL(traj_errors_kernel, dim3(nb), dim3(kThreads), 0, st, n, pos, valid, T, err, parts);
  hipLaunchKernelGGL(traj_stats_kernel, dim3(1), dim3(kWide), 0, st, n, nb, err, valid, parts, stats);
  return hipGetLastError() == hipSuccess ? SGR_OK : set_error(SGR_ERR_HIP, "traj_errors launch failed");
}

size_t sgr_traj_associate_scratch_bytes(int32_t na, int32_t nb) {
  return supported(na) && nb >= 1 && nb <= SGR_TRAJ_MAX_STAMPS ? assoc_bytes(na, nb) : 0;
}

int sgr_traj_associate(const double* stamps_a, int32_t na, const double* stamps_b, int32_t nb, double offset_b, double max_diff,
                       int32_t* match, int32_t* a_inds, int32_t* b_inds, int32_t* header, void* scratch, size_t scratch_bytes,
                       void* stream) {
  if (!supported(na) || nb < 1 || nb > SGR_TRAJ_MAX_STAMPS || !stamps_a || !stamps_b || !match || !a_inds || !b_inds || !header)
    return set_error(SGR_ERR_INVALID, "traj_associate: bad arguments (na=%d nb=%d)", na, nb);
  if (!scratch || scratch_bytes < assoc_bytes(na, nb)) return set_error(SGR_ERR_WORKSPACE, "traj_associate: scratch too small");
  hipStream_t st = (hipStream_t)stream;
  int32_t* flags = (int32_t*)scratch;
  const int nblk = assoc_blocks(na, nb);
  hipLaunchKernelGGL(traj_associate_kernel, dim3(nblk), dim3(kThreads), 0, st, na, stamps_a, nb, stamps_b, offset_b, max_diff, match, flags);
  hipLaunchKernelGGL(traj_compact_kernel, dim3(1), dim3(kWide), 0, st, na, nblk, match, flags, a_inds, b_inds, header);
  return hipGetLastError() == hipSuccess ? SGR_OK : set_error(SGR_ERR_HIP, "traj_associate launch failed");
}

size_t sgr_traj_pose_errors_scratch_bytes(int32_t n) { return supported(n) ? pe_bytes(n) : 0; }

int sgr_traj_pose_errors(int32_t kind, const float* est, int32_t est_rows, const float* ref, int32_t ref_rows, const int32_t* est_inds,
                         const int32_t* ref_inds, int32_t n, const double* sim3, int32_t mode, int32_t delta, int32_t all_pairs,
                         int32_t relation, double* err, int32_t* pair_rows, double* stats, int32_t* header, void* scratch,
                         size_t scratch_bytes, void* stream) {
  if (!supported(n) || (kind != SGR_TRAJ_POSE7_W2C && kind != SGR_TRAJ_MAT4_C2W) || !est || est_rows < 1 || !ref || ref_rows < 1 || !sim3 ||
      !err || !pair_rows || !stats || !header)
    return set_error(SGR_ERR_INVALID, "traj_pose_errors: bad arguments (kind=%d n=%d est_rows=%d ref_rows=%d)", kind, n, est_rows, ref_rows);
  if ((mode != SGR_TRAJ_ABSOLUTE && mode != SGR_TRAJ_RELATIVE) || relation < SGR_TRAJ_TRANSLATION_PART ||
      relation > SGR_TRAJ_FULL_TRANSFORMATION || (mode == SGR_TRAJ_RELATIVE && delta < 1))
    return set_error(SGR_ERR_INVALID, "traj_pose_errors: bad mode=%d, relation=%d or delta=%d", mode, relation, delta);
  if (((uintptr_t)ref & 15) || (kind == SGR_TRAJ_MAT4_C2W && ((uintptr_t)est & 15)))
    return set_error(SGR_ERR_INVALID, "traj_pose_errors: 4 x 4 rows must be 16-byte aligned");
  if (!scratch || scratch_bytes < pe_bytes(n)) return set_error(SGR_ERR_WORKSPACE, "traj_pose_errors: scratch too small");
  Sim3 T;
  T.s = sim3[0];
  for (int k = 0; k < 9; ++k) T.r[k] = sim3[1 + k];
  for (int k = 0; k < 3; ++k) T.t[k] = sim3[10 + k];
  hipStream_t st = (hipStream_t)stream;
  char* base = (char*)scratch;
  double* parts = (double*)base;
  uint32_t* counts = (uint32_t*)(base + pe_counts_off(n));
  uint8_t* used = (uint8_t*)(base + pe_used_off(n));
  int32_t* rank_row = (int32_t*)(base + pe_rank_off(n));
  double* mats = (double*)(base + pe_mats_off(n));
  const int nb = blocks_for(n);
  if (kind == SGR_TRAJ_POSE7_W2C)
    hipLaunchKernelGGL(traj_poses_kernel<SGR_TRAJ_POSE7_W2C>, dim3(nb), dim3(kThreads), 0, st, n, est, est_rows, ref, ref_rows, est_inds,
                       ref_inds, T, mats, used, counts);
  else
    hipLaunchKernelGGL(traj_poses_kernel<SGR_TRAJ_MAT4_C2W>, dim3(nb), dim3(kThreads), 0, st, n, est, est_rows, ref, ref_rows, est_inds,
                       ref_inds, T, mats, used, counts);
  hipLaunchKernelGGL(traj_ranks_kernel, dim3(nb), dim3(kThreads), 0, st, n, used, counts, mode, delta, all_pairs ? 1 : 0, rank_row, header);
  hipLaunchKernelGGL(traj_item_errors_kernel, dim3(nb), dim3(kThreads), 0, st, n, mats, rank_row, header, mode, delta, all_pairs ? 1 : 0,
                     relation, err, pair_rows, parts);
  hipLaunchKernelGGL(traj_item_stats_kernel, dim3(1), dim3(kWide), 0, st, n, nb, err, header, parts, stats);
  return hipGetLastError() == hipSuccess ? SGR_OK : set_error(SGR_ERR_HIP, "traj_pose_errors launch failed");
}

}  // extern "C"
