// The two per-update passes of the tracker's keyframe store (DepthVideo, thirdparty/glorie_slam/depth_video.py) that are GPU work of
// their own: the convex upsampling of the 1/8-resolution disparity maps (DepthVideo.upsample -> cvx_upsample,
// modules/droid_net/droid_net.py:23-37) and the two-view consistency mask (update_valid_depth_mask, depth_video.py:340-375).
//   sgr_video_cvx_upsample       softmax-weighted 3x3 combination, 64 outputs per coarse pixel, the mask read once
//   sgr_video_depth_thresh       rel * mean(1 / disp) per frame
//   sgr_video_mask_from_counts   lower median of the depths that enough views agree on (exact radix select), depth < 3 * median
//   sgr_video_valid_mask         thresholds -> sgr_dba_depth_filter -> mask, chained on the stream
// The algorithm, the kernel shapes and their traffic floors are described in DESIGN.md section 3, "Depth video".  Floating-point sums
// are fixed-order register / wave-butterfly / LDS reductions; the only atomics are integer counters of histograms, whose result does
// not depend on arrival order: every output is bitwise reproducible.  No host synchronisation, no allocation.
#include <cmath>
#include <cstdint>

#include <hip/hip_fp16.h>

#include "sgr_common.h"
#include "sgr_dba_device.h"

namespace sgr {
int set_error(int code, const char* fmt, ...);

namespace {

using dba::frame_ok;

constexpr int kThreads = 256;
constexpr int kSub = 8;                     // upsampling factor: 8 x 8 outputs per coarse pixel
constexpr int kMaskChannels = 9 * kSub * kSub;
constexpr int kMaxNum = SGR_VIDEO_MAX_FRAMES;      // frames per call (a grid dimension, and the limit of sgr_dba_depth_filter)


// ================================================================================================================================
// convex upsampling.  One thread per (coarse pixel p, sub-row dy): its 9 x 8 logits are 72 independent loads, each of them one
// coalesced run over the 64 consecutive pixels of the wave (for a fixed channel the mask is contiguous in p), and its 8 outputs are
// 32 contiguous bytes of the output row that the neighbouring lanes continue.  The four waves of a workgroup take four dy of the
// same 64 pixels; blockIdx.y picks the upper or the lower four.
// ================================================================================================================================

__device__ __forceinline__ float widen(float v) { return v; }
__device__ __forceinline__ float widen(__half v) { return __half2float(v); }

template <typename T>
__global__ void __launch_bounds__(kThreads) cvx_upsample_kernel(int nf, int ht, int wd, const float* __restrict__ disps,
                                                                const int64_t* __restrict__ inds, const T* __restrict__ mask,
                                                                float* __restrict__ out) {
  const int P = ht * wd, b = blockIdx.z;
  const int64_t f = inds[b];
  if (!frame_ok(f, nf)) return;
  const int p = blockIdx.x * 64 + (threadIdx.x & 63), dy = blockIdx.y * 4 + (threadIdx.x >> 6);
  if (p >= P) return;
  const int y = p / wd, x = p - (p / wd) * wd;
  const T* m = mask + ((size_t)b * kMaskChannels + dy * kSub) * P + p;
  float v[9][kSub];
#pragma unroll
  for (int k = 0; k < 9; ++k)
#pragma unroll
    for (int dx = 0; dx < kSub; ++dx) v[k][dx] = widen(m[(size_t)(k * kSub * kSub + dx) * P]);
  const float* d = disps + (size_t)f * P;
  float nb[9];                                  // the 3 x 3 neighbourhood, row-major; 0 outside the map (the zero padding of the unfold)
#pragma unroll
  for (int k = 0; k < 9; ++k) {
    const int yy = y + k / 3 - 1, xx = x + k % 3 - 1;
    nb[k] = (yy >= 0 && yy < ht && xx >= 0 && xx < wd) ? d[yy * wd + xx] : 0.f;
  }
  float o[kSub];
#pragma unroll
  for (int dx = 0; dx < kSub; ++dx) {
    float mx = v[0][dx];
#pragma unroll
    for (int k = 1; k < 9; ++k) mx = fmaxf(mx, v[k][dx]);
    float s = 0.f, a = 0.f;
#pragma unroll
    for (int k = 0; k < 9; ++k) {
      const float e = expf(v[k][dx] - mx);
      s += e;
      a += e * nb[k];
    }
    o[dx] = a / s;
  }
  float4* dst = (float4*)(out + (size_t)f * (kSub * kSub) * P + (size_t)(kSub * y + dy) * (kSub * wd) + kSub * x);
  dst[0] = make_float4(o[0], o[1], o[2], o[3]);
  dst[1] = make_float4(o[4], o[5], o[6], o[7]);
}

// ================================================================================================================================
// depth_thresh: one 1024-thread workgroup per frame.  Element i belongs to chunk i / 4, chunk c to thread c % 1024, taken in
// increasing c: the order of the sum does not depend on whether the chunk was loaded as one float4.
// ================================================================================================================================

constexpr int kThreshThreads = 1024;

__global__ void __launch_bounds__(kThreshThreads) depth_thresh_kernel(int nf, int P, const float* __restrict__ disps,
                                                                      const int64_t* __restrict__ inds, float rel,
                                                                      float* __restrict__ thresh) {
  __shared__ double red[kThreshThreads / 64];
  const int b = blockIdx.x, t = threadIdx.x;
  const int64_t f = inds[b];
  if (!frame_ok(f, nf)) {
    if (t == 0) thresh[b] = NAN;
    return;
  }
  const float* d = disps + (size_t)f * P;
  const bool vec = (P & 3) == 0 && ((uintptr_t)d & 15) == 0;
  const int chunks = (P + 3) >> 2;
  double s = 0.0;
#pragma unroll 4
  for (int c = t; c < chunks; c += kThreshThreads) {
    if (vec) {
      const float4 q = ((const float4*)d)[c];
      s += (double)(1.0f / q.x);
      s += (double)(1.0f / q.y);
      s += (double)(1.0f / q.z);
      s += (double)(1.0f / q.w);
    } else {
      for (int i = 4 * c; i < min(P, 4 * c + 4); ++i) s += (double)(1.0f / d[i]);
    }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off);
  if ((t & 63) == 0) red[t >> 6] = s;
  __syncthreads();
  if (t == 0) {
    double tot = red[0];
    for (int k = 1; k < kThreshThreads / 64; ++k) tot += red[k];
    thresh[b] = rel * (float)(tot / (double)P);
  }
}

// ================================================================================================================================
// mask_from_counts: exact selection of the lower median by a radix select over the order-preserving integer image of the depth,
// most significant digit first (11 + 11 + 10 bits).  Per digit: hist_kernel counts the candidates that match the digits chosen so
// far (LDS histogram per workgroup of kHistPixels pixels, non-zero bins added to the frame's histogram with integer atomics),
// select_kernel (one workgroup per frame) finds the bin that holds the wanted rank.  A full-size frame is 75 workgroups per pass,
// a 60 x 80 one two; the grid's y is the frame.
// ================================================================================================================================

constexpr int kBins = 2048;
constexpr int kPasses = 3;
constexpr int kHistPerThread = 16;
constexpr int kHistPixels = kThreads * kHistPerThread;

struct __attribute__((aligned(16))) SelState {
  uint32_t prefix;      // the digits chosen so far, in place; after the last pass the key of the median
  int rank;             // rank wanted among the candidates that match prefix
  int m;                // number of candidates of the frame
  int pad;
};

__device__ __forceinline__ uint32_t key_of(float v) {        // v1 < v2  <=>  key_of(v1) < key_of(v2), for every non-NaN v (-0 < +0)
  const uint32_t u = __float_as_uint(v);
  return (u >> 31) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float value_of(uint32_t k) { return __uint_as_float((k >> 31) ? (k & 0x7fffffffu) : ~k); }

__device__ __forceinline__ bool candidate(float disp, float count, float visible, float* depth) {
  *depth = 1.0f / disp;
  return count >= visible && *depth == *depth;
}

template <int PASS>
__device__ __forceinline__ uint32_t digit_of(uint32_t key) {
  return PASS == 0 ? key >> 21 : PASS == 1 ? (key >> 10) & 0x7ffu : key & 0x3ffu;
}
template <int PASS>
__device__ __forceinline__ bool matches(uint32_t key, uint32_t prefix) {
  return PASS == 0 ? true : PASS == 1 ? (key >> 21) == (prefix >> 21) : (key >> 10) == (prefix >> 10);
}

__global__ void __launch_bounds__(kThreads) zero_kernel(uint32_t* __restrict__ p, size_t n) {
  const size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x;
  if (i < n) p[i] = 0u;
}

template <int PASS>
__global__ void __launch_bounds__(kThreads) hist_kernel(int nf, int P, const float* __restrict__ disps, const int64_t* __restrict__ inds,
                                                        const float* __restrict__ counts, float visible,
                                                        const SelState* __restrict__ state, uint32_t* __restrict__ hist) {
  __shared__ uint32_t lh[kBins];
  const int b = blockIdx.y;
  const int64_t f = inds[b];
  if (!frame_ok(f, nf)) return;
  uint32_t prefix = 0u;
  if (PASS > 0) {
    if (state[b].m == 0) return;
    prefix = state[b].prefix;
  }
  for (int i = threadIdx.x; i < kBins; i += kThreads) lh[i] = 0u;
  __syncthreads();
  const float* d = disps + (size_t)f * P;
  const float* c = counts + (size_t)b * P;
  const int p0 = blockIdx.x * kHistPixels + threadIdx.x;
#pragma unroll 4
  for (int n = 0; n < kHistPerThread; ++n) {
    const int p = p0 + n * kThreads;
    if (p >= P) break;
    float depth;
    if (!candidate(d[p], c[p], visible, &depth)) continue;
    const uint32_t key = key_of(depth);
    if (matches<PASS>(key, prefix)) atomicAdd(&lh[digit_of<PASS>(key)], 1u);
  }
  __syncthreads();
  uint32_t* gh = hist + ((size_t)b * kPasses + PASS) * kBins;
  for (int i = threadIdx.x; i < kBins; i += kThreads) {
    const uint32_t v = lh[i];
    if (v) atomicAdd(&gh[i], v);
  }
}

// Thread t owns the bins [8t, 8t + 8).  An inclusive scan of the 256 thread sums finds the thread, and that thread the bin, in
// which the cumulative count passes the wanted rank.
template <int PASS>
__global__ void __launch_bounds__(kThreads) select_kernel(int nf, const int64_t* __restrict__ inds, const uint32_t* __restrict__ hist,
                                                          SelState* __restrict__ state) {
  __shared__ int lds[kThreads];
  constexpr int kPer = kBins / kThreads;
  const int b = blockIdx.x, t = threadIdx.x;
  if (!frame_ok(inds[b], nf)) return;
  const SelState st = PASS > 0 ? state[b] : SelState{0u, 0, 0, 0};      // every thread reads it before the scan's barriers, one writes it after them
  if (PASS > 0 && st.m == 0) return;
  const uint32_t* gh = hist + ((size_t)b * kPasses + PASS) * kBins + t * kPer;
  int c[kPer], s = 0;
#pragma unroll
  for (int i = 0; i < kPer; ++i) {
    c[i] = (int)gh[i];
    s += c[i];
  }
  lds[t] = s;
  __syncthreads();
  for (int off = 1; off < kThreads; off <<= 1) {
    const int v = t >= off ? lds[t - off] : 0;
    __syncthreads();
    lds[t] += v;
    __syncthreads();
  }
  const int total = lds[kThreads - 1], before = lds[t] - s;
  int rank;
  if (PASS == 0) {
    if (total == 0) {
      if (t == 0) state[b] = SelState{0u, 0, 0, 0};
      return;
    }
    rank = (total - 1) / 2;
  } else {
    rank = st.rank;
  }
  if (!(before <= rank && rank < before + s)) return;         // exactly one thread goes on: 0 <= rank < total
  int run = before;
#pragma unroll
  for (int i = 0; i < kPer; ++i) {
    if (rank < run + c[i]) {
      const uint32_t bin = (uint32_t)(t * kPer + i);
      const uint32_t prefix = PASS == 0 ? bin << 21 : PASS == 1 ? st.prefix | (bin << 10) : st.prefix | bin;
      state[b] = SelState{prefix, rank - run, PASS == 0 ? total : st.m, 0};
      return;
    }
    run += c[i];
  }
}

__global__ void __launch_bounds__(kThreads) mask_kernel(int nf, int P, const float* __restrict__ disps, const int64_t* __restrict__ inds,
                                                        const float* __restrict__ counts, float visible,
                                                        const SelState* __restrict__ state, uint8_t* __restrict__ mask_out) {
  const int b = blockIdx.y, p = blockIdx.x * kThreads + threadIdx.x;
  const int64_t f = inds[b];
  if (!frame_ok(f, nf) || p >= P) return;
  const SelState st = state[b];
  const float median = st.m == 0 ? NAN : value_of(st.prefix);
  float depth;
  const bool cand = candidate(disps[(size_t)f * P + p], counts[(size_t)b * P + p], visible, &depth);
  mask_out[(size_t)f * P + p] = (cand && depth < 3.0f * median) ? 1 : 0;
}

// ---- scratch layout
struct VideoScratch {
  uint32_t* hist;       // [num][kPasses][kBins]
  SelState* state;      // [num]
  float* thresh;        // [num]
  float* counts;        // [num][P]
};

size_t carve(int num, int P, char* base, VideoScratch* s) {
  size_t off = 0;
  auto take = [&](size_t bytes) {
    char* p = base ? base + off : nullptr;
    off += align_up(bytes);
    return p;
  };
  VideoScratch d;
  d.hist = (uint32_t*)take((size_t)num * kPasses * kBins * sizeof(uint32_t));
  d.state = (SelState*)take((size_t)num * sizeof(SelState));
  d.thresh = (float*)take((size_t)num * sizeof(float));
  d.counts = (float*)take((size_t)num * P * sizeof(float));
  if (s) *s = d;
  return off;
}

bool sizes_ok(int num, int ht, int wd) {
  return num > 0 && num <= kMaxNum && ht > 0 && wd > 0 && (long long)ht * wd < (1LL << 26);
}

int launch_thresh(const float* disps, int nf, int P, const int64_t* inds, int num, float rel, float* thresh, hipStream_t st) {
  hipLaunchKernelGGL(depth_thresh_kernel, dim3(num), dim3(kThreshThreads), 0, st, nf, P, disps, inds, rel, thresh);
  return hipGetLastError() == hipSuccess ? SGR_OK : set_error(SGR_ERR_HIP, "video_depth_thresh launch failed");
}

int launch_mask(const float* disps, int nf, int P, const int64_t* inds, int num, const float* counts, int visible_num, uint8_t* mask_out,
                const VideoScratch& s, hipStream_t st) {
  const float vis = (float)visible_num;
  const size_t words = (size_t)num * kPasses * kBins;
  const dim3 hg(blocks_for(P, kHistPixels), num);
  hipLaunchKernelGGL(zero_kernel, dim3(blocks_for((long long)words)), dim3(kThreads), 0, st, s.hist, words);
  hipLaunchKernelGGL(hist_kernel<0>, hg, dim3(kThreads), 0, st, nf, P, disps, inds, counts, vis, s.state, s.hist);
  hipLaunchKernelGGL(select_kernel<0>, dim3(num), dim3(kThreads), 0, st, nf, inds, s.hist, s.state);
  hipLaunchKernelGGL(hist_kernel<1>, hg, dim3(kThreads), 0, st, nf, P, disps, inds, counts, vis, s.state, s.hist);
  hipLaunchKernelGGL(select_kernel<1>, dim3(num), dim3(kThreads), 0, st, nf, inds, s.hist, s.state);
  hipLaunchKernelGGL(hist_kernel<2>, hg, dim3(kThreads), 0, st, nf, P, disps, inds, counts, vis, s.state, s.hist);
  hipLaunchKernelGGL(select_kernel<2>, dim3(num), dim3(kThreads), 0, st, nf, inds, s.hist, s.state);
  hipLaunchKernelGGL(mask_kernel, dim3(blocks_for(P), num), dim3(kThreads), 0, st, nf, P, disps, inds, counts, vis, s.state, mask_out);
  return hipGetLastError() == hipSuccess ? SGR_OK : set_error(SGR_ERR_HIP, "video_mask_from_counts launch failed");
}

}  // namespace
}  // namespace sgr

using namespace sgr;

extern "C" {

int sgr_video_cvx_upsample(const float* disps, int32_t num_frames, int32_t ht, int32_t wd, const int64_t* inds, int32_t num,
                           const void* mask, int32_t mask_kind, float* disps_up, void* stream) {
  if (!disps || !inds || !mask || !disps_up || num < 0 || num > kMaxNum || num_frames < 0 || ht <= 0 || wd <= 0 ||
      (long long)ht * wd >= (1LL << 24) || (mask_kind != SGR_VIDEO_MASK_F32 && mask_kind != SGR_VIDEO_MASK_F16) ||
      ((uintptr_t)disps_up & 15) != 0)
    return set_error(SGR_ERR_INVALID, "video_cvx_upsample: bad arguments (disps_up must be 16-byte aligned, num <= %d)", kMaxNum);
  if (num == 0) return SGR_OK;
  const dim3 grid(blocks_for((long long)ht * wd, 64), 2, num);
  if (mask_kind == SGR_VIDEO_MASK_F32)
    hipLaunchKernelGGL(cvx_upsample_kernel<float>, grid, dim3(kThreads), 0, (hipStream_t)stream, num_frames, ht, wd, disps, inds,
                       (const float*)mask, disps_up);
  else
    hipLaunchKernelGGL(cvx_upsample_kernel<__half>, grid, dim3(kThreads), 0, (hipStream_t)stream, num_frames, ht, wd, disps, inds,
                       (const __half*)mask, disps_up);
  return hipGetLastError() == hipSuccess ? SGR_OK : set_error(SGR_ERR_HIP, "video_cvx_upsample launch failed");
}

int sgr_video_depth_thresh(const float* disps, int32_t num_frames, int32_t ht, int32_t wd, const int64_t* inds, int32_t num, float rel,
                           float* thresh, void* stream) {
  if (!disps || !inds || !thresh || num < 0 || num_frames < 0 || (num > 0 && !sizes_ok(num, ht, wd)))
    return set_error(SGR_ERR_INVALID, "video_depth_thresh: bad arguments");
  if (num == 0) return SGR_OK;
  return launch_thresh(disps, num_frames, ht * wd, inds, num, rel, thresh, (hipStream_t)stream);
}

size_t sgr_video_scratch_bytes(int32_t num, int32_t ht, int32_t wd) {
  if (!sizes_ok(num, ht, wd)) return 0;
  return carve(num, ht * wd, nullptr, nullptr);
}

int sgr_video_mask_from_counts(const float* disps, int32_t num_frames, int32_t ht, int32_t wd, const int64_t* inds, int32_t num,
                               const float* counts, int32_t visible_num, uint8_t* mask_out, void* scratch, size_t scratch_bytes,
                               void* stream) {
  if (!disps || !inds || !counts || !mask_out || num < 0 || num_frames < 0 || (num > 0 && !sizes_ok(num, ht, wd)))
    return set_error(SGR_ERR_INVALID, "video_mask_from_counts: bad arguments");
  if (num == 0) return SGR_OK;
  if (!scratch || ((uintptr_t)scratch & 15) != 0 || scratch_bytes < carve(num, ht * wd, nullptr, nullptr))
    return set_error(SGR_ERR_WORKSPACE, "video_mask_from_counts: scratch too small or not 16-byte aligned");
  VideoScratch s;
  carve(num, ht * wd, (char*)scratch, &s);
  return launch_mask(disps, num_frames, ht * wd, inds, num, counts, visible_num, mask_out, s, (hipStream_t)stream);
}

int sgr_video_valid_mask(const float* poses, const float* disps, int32_t num_frames, int32_t ht, int32_t wd, const float* intrinsics,
                         const int64_t* inds, int32_t num, float rel, int32_t visible_num, uint8_t* mask_out, void* scratch,
                         size_t scratch_bytes, void* stream) {
  if (!poses || !disps || !intrinsics || !inds || !mask_out || num < 0 || num_frames < 0 || (num > 0 && !sizes_ok(num, ht, wd)))
    return set_error(SGR_ERR_INVALID, "video_valid_mask: bad arguments");
  if (num == 0) return SGR_OK;
  if (!scratch || ((uintptr_t)scratch & 15) != 0 || scratch_bytes < carve(num, ht * wd, nullptr, nullptr))
    return set_error(SGR_ERR_WORKSPACE, "video_valid_mask: scratch too small or not 16-byte aligned");
  VideoScratch s;
  carve(num, ht * wd, (char*)scratch, &s);
  hipStream_t st = (hipStream_t)stream;
  int rc = launch_thresh(disps, num_frames, ht * wd, inds, num, rel, s.thresh, st);
  if (rc != SGR_OK) return rc;
  rc = sgr_dba_depth_filter(poses, disps, num_frames, ht, wd, intrinsics, inds, num, s.thresh, s.counts, stream);
  if (rc != SGR_OK) return rc;
  return launch_mask(disps, num_frames, ht * wd, inds, num, s.counts, visible_num, mask_out, s, st);
}

}  // extern "C"
