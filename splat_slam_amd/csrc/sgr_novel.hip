// Exposure fit of the novel-view evaluation ("Novel-view evaluation"): a held-out frame has no optimised
// exposure, so sgr_exposure_fit finds, per frame of an SgrMetricFrame table, the gain g and bias b that minimise
//   sum over gt > 0 of (g render + b - gt)^2          (the mask of sgr_render_metrics' PSNR)
// and stores a = log g and b where the table's exposure pointers look for them.
//   launch 1  exposure_sums_kernel    grid (blocks, frames): every workgroup's six fp64 sums of kBlockElems consecutive elements
//   launch 2  exposure_solve_kernel   one wave per frame: the partials in workgroup order, the 2 x 2 solve, the degeneracy rule
// Every term is formed in fp64 from the fp32 inputs (a product of two fp32 values is exact there); the order of every addition is
// fixed by the element's index alone -- per lane, butterfly across the wave, the waves left to right, the workgroups in order -- so a
// frame gives the same bits alone and in any batch, on any stream.  No float atomics, no LDS beyond block_partials' merge.
#include <cmath>
#include <cstdint>

#include "sgr_common.h"

namespace sgr {
int set_error(int code, const char* fmt, ...);

namespace {

constexpr int kFitFrames = SGR_EXPOSURE_FIT_MAX_FRAMES;                     // frames per call: the table travels as a kernel argument
constexpr int kThreads = 256, kWaves = kThreads / 64;
constexpr int kVec = 4, kIters = 4;                    // a lane takes kIters groups of four consecutive elements
constexpr int kBlockElems = kThreads * kVec * kIters;  // 4096 elements of each image per workgroup
constexpr int kSums = 6, kPartRow = 8;                 // m, sum r, sum t, sum r^2, sum r t, sum t^2; a partial is one 64-byte row
constexpr int64_t kMaxElems = (int64_t)1 << 30;

struct FitTab {
  const float* render[kFitFrames];
  const float* gt[kFitFrames];
};

inline int blocks_of(int64_t total) { return (int)((total + kBlockElems - 1) / kBlockElems); }
inline bool supported(int n, int C, int H, int W) {
  return n >= 1 && n <= kFitFrames && C >= 1 && H >= 1 && W >= 1 && (int64_t)C * H * W <= kMaxElems;
}

// ---- launch 1.  Group q = 4 consecutive elements from 4 q; lane l of workgroup w takes groups (w kIters + j) kThreads + l, j < kIters.
// A workgroup whose kBlockElems elements all exist, of two 16-byte aligned images, issues its eight 16-byte loads per lane back to back
// (a branch the whole workgroup takes alike); the last workgroup of a frame and unaligned images go element by element, an element
// past the end counting as gt = 0, which the mask drops.  The same elements in the same order either way.  A dropped element adds
// +0.0 to every sum, which changes no bit of it: the additions need no branch.
__global__ void __launch_bounds__(kThreads) exposure_sums_kernel(FitTab tab, int64_t total, double* __restrict__ parts) {
  const float* __restrict__ r = tab.render[blockIdx.y];
  const float* __restrict__ g = tab.gt[blockIdx.y];
  const int64_t base = (int64_t)blockIdx.x * kBlockElems;
  const bool whole = ((((uintptr_t)r) | ((uintptr_t)g)) & 15) == 0 && base + kBlockElems <= total;
  float rv[kIters][kVec], tv[kIters][kVec];
  if (whole) {
    float4 a[kIters], b[kIters];
#pragma unroll
    for (int j = 0; j < kIters; ++j) {
      const int64_t e = base + (int64_t)(j * kThreads + threadIdx.x) * kVec;
      a[j] = *(const float4*)(r + e);
      b[j] = *(const float4*)(g + e);
    }
#pragma unroll
    for (int j = 0; j < kIters; ++j) {
      rv[j][0] = a[j].x; rv[j][1] = a[j].y; rv[j][2] = a[j].z; rv[j][3] = a[j].w;
      tv[j][0] = b[j].x; tv[j][1] = b[j].y; tv[j][2] = b[j].z; tv[j][3] = b[j].w;
    }
  } else {
#pragma unroll
    for (int j = 0; j < kIters; ++j)
#pragma unroll
      for (int k = 0; k < kVec; ++k) {
        const int64_t e = base + (int64_t)(j * kThreads + threadIdx.x) * kVec + k;
        const bool in = e < total;
        rv[j][k] = in ? r[e] : 0.f;
        tv[j][k] = in ? g[e] : 0.f;
      }
  }
  double acc[kSums];
#pragma unroll
  for (int k = 0; k < kSums; ++k) acc[k] = 0.0;
#pragma unroll
  for (int j = 0; j < kIters; ++j)
#pragma unroll
    for (int k = 0; k < kVec; ++k) {
      const bool in = tv[j][k] > 0.f;                   // the mask of the PSNR: gt > 0 (a NaN is outside it)
      const double x = in ? (double)rv[j][k] : 0.0, y = in ? (double)tv[j][k] : 0.0;
      acc[0] += in ? 1.0 : 0.0; acc[1] += x; acc[2] += y; acc[3] += x * x; acc[4] += x * y; acc[5] += y * y;
    }
  block_partials<kSums, kWaves>(acc, parts + ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * kPartRow);
}

// ---- launch 2: grid (frames), one wave.  Lane k < kSums adds the frame's partials of sum k in workgroup order; lane 0 solves.
__global__ void __launch_bounds__(64) exposure_solve_kernel(int nblk, const double* __restrict__ parts, float* __restrict__ ab,
                                                            int32_t* __restrict__ flags) {
  const int f = blockIdx.x, k = threadIdx.x;
  double s = 0.0;
  if (k < kSums) {
    const double* p = parts + (size_t)f * nblk * kPartRow + k;
#pragma unroll 8
    for (int b = 0; b < nblk; ++b) s += p[(size_t)b * kPartRow];
  }
  const double m = __shfl(s, 0), sr = __shfl(s, 1), st = __shfl(s, 2), srr = __shfl(s, 3), srt = __shfl(s, 4);
  if (k != 0) return;
  // minimise sum (g r + b - t)^2:  g = (m S_rt - S_r S_t) / det,  b = (S_t - g S_r) / m,  det = m S_rr - S_r^2 = m^2 var(r)
  const double det = m * srr - sr * sr;
  const double floor_ = m * m * 0x1p-40 * fmax(srr / m, 1.0);       // a render that is constant on the mask: var(r) is rounding
  float a = 0.f, b = 0.f;
  int flag = 1;
  if (m >= 2.0 && det > 0.0 && det > floor_) {                      // (written so that a NaN fails every test)
    const double gain = (m * srt - sr * st) / det;
    if (gain > 0.0 && isfinite(gain)) {
      const float fa = (float)log(gain), fb = (float)((st - gain * sr) / m);
      if (isfinite(fa) && isfinite(fb)) { a = fa; b = fb; flag = 0; }
    }
  }
  ab[2 * f] = a;
  ab[2 * f + 1] = b;
  flags[f] = flag;
}

}  // namespace
}  // namespace sgr

using namespace sgr;

extern "C" {

size_t sgr_exposure_fit_bytes(int32_t n, int32_t C, int32_t H, int32_t W) {
  return supported(n, C, H, W) ? align_up((size_t)n * blocks_of((int64_t)C * H * W) * kPartRow * sizeof(double)) : 0;
}

int sgr_exposure_fit(int32_t n, const SgrMetricFrame* frames, int32_t C, int32_t H, int32_t W, float* ab, int32_t* flags, void* scratch,
                     size_t scratch_bytes, void* stream) {
  if (!supported(n, C, H, W)) return set_error(SGR_ERR_INVALID, "exposure_fit: n=%d outside 1..%d or bad size %dx%dx%d", n, kFitFrames, C, H, W);
  if (!frames || !ab || !flags) return set_error(SGR_ERR_INVALID, "exposure_fit: null table or output");
  FitTab tab = {};
  for (int i = 0; i < n; ++i) {
    if (!frames[i].render || !frames[i].gt_image) return set_error(SGR_ERR_INVALID, "exposure_fit: frame %d has no image", i);
    if ((((uintptr_t)frames[i].render) | ((uintptr_t)frames[i].gt_image)) & 3)
      return set_error(SGR_ERR_INVALID, "exposure_fit: frame %d is not 4-byte aligned", i);
    tab.render[i] = frames[i].render;
    tab.gt[i] = frames[i].gt_image;
  }
  if (!scratch || scratch_bytes < sgr_exposure_fit_bytes(n, C, H, W))
    return set_error(SGR_ERR_WORKSPACE, "exposure_fit: scratch too small (need %zu)", sgr_exposure_fit_bytes(n, C, H, W));
  const int64_t total = (int64_t)C * H * W;
  const int nblk = blocks_of(total);
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(exposure_sums_kernel, dim3(nblk, n), dim3(kThreads), 0, st, tab, total, (double*)scratch);
  hipLaunchKernelGGL(exposure_solve_kernel, dim3(n), dim3(64), 0, st, nblk, (const double*)scratch, ab, flags);
  return hipGetLastError() == hipSuccess ? SGR_OK : set_error(SGR_ERR_HIP, "exposure_fit launch failed");
}

}  // extern "C"
