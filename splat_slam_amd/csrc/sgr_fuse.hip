// Keyframe depth fusion: what the mapper seeds and supervises with (Mapper.get_w2c_and_depth of the reference's src/mapper.py:258-301),
// split into the part that depends on the mono-depth map alone and the part that depends on the video's current state.
//   sgr_fuse_prepare   once per keyframe: outlier removal (> 4 mean), 11 x 11 erosion, fill of what that removed
//   sgr_fuse_depth     per request and frame: valid count, weighted scale-and-shift fit of the prepared mono map against the tracker's
//                      depth, depth = valid ? 1 / disp : s mono + q; the frames are read in place through their indices
// The equations, the kernels and the precision of every sum are described in DESIGN.md section 3, "Keyframe depth fusion".  Every
// floating-point sum is a fixed-order register / wave-butterfly / LDS reduction whose partition depends on H x W alone: no atomics,
// bitwise reproducible, a frame gives the same bits alone and in any batch.  One call is stream-ordered from its first launch to its
// last, with no host synchronisation and no allocation.
#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdint>

#include "sgr_common.h"
#include "sgr_dba_device.h"

namespace sgr {
int set_error(int code, const char* fmt, ...);

namespace {

using dba::frame_ok;

constexpr int kMaxNum = SGR_FUSE_MAX_FRAMES;       // frames per call (a grid dimension)
constexpr long long kMaxPixels = 1LL << 28;


__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
  return v;
}

// ================================================================================================================================
// prepare 1/3, mean: one 1024-thread workgroup per map.  Element i belongs to chunk i / 4, chunk c to thread c % 1024, taken in
// increasing c (the order of sgr_video_depth_thresh): the sum does not depend on whether a chunk was loaded as one float4.
// ================================================================================================================================

constexpr int kMeanThreads = 1024;

__global__ void __launch_bounds__(kMeanThreads) mean_kernel(int P, const float* __restrict__ mono, float* __restrict__ mean) {
  __shared__ double red[kMeanThreads / 64];
  const int t = threadIdx.x;
  const float* d = mono + (size_t)blockIdx.x * P;
  const bool vec = (P & 3) == 0 && ((uintptr_t)d & 15) == 0;
  const int chunks = (P + 3) >> 2;
  double s = 0.0;
#pragma unroll 4
  for (int c = t; c < chunks; c += kMeanThreads) {
    if (vec) {
      const float4 q = ((const float4*)d)[c];
      s += (double)q.x;
      s += (double)q.y;
      s += (double)q.z;
      s += (double)q.w;
    } else {
      for (int i = 4 * c; i < min(P, 4 * c + 4); ++i) s += (double)d[i];
    }
  }
  s = wave_sum_f64(s);
  if ((t & 63) == 0) red[t >> 6] = s;
  __syncthreads();
  if (t == 0) {
    double tot = red[0];
    for (int k = 1; k < kMeanThreads / 64; ++k) tot += red[k];
    mean[blockIdx.x] = (float)(tot / (double)P);
  }
}

// ================================================================================================================================
// prepare 2/3, threshold and erosion: a 32 x 32 tile per workgroup.  The tile's positive flags with a halo of 5 (1 outside the image:
// the reference pads with ones) go to LDS, a row pass takes the minimum over 11 columns, a column pass over 11 rows.
// ================================================================================================================================

constexpr int kErodeTile = 32, kErodeR = 5, kErodeSpan = kErodeTile + 2 * kErodeR, kErodeThreads = 256;

__global__ void __launch_bounds__(kErodeThreads) erode_kernel(int H, int W, const float* __restrict__ mono, const float* __restrict__ mean,
                                                              float* __restrict__ filled, uint8_t* __restrict__ eroded) {
  __shared__ uint8_t pos[kErodeSpan][kErodeSpan + 2];
  __shared__ uint8_t row[kErodeSpan][kErodeTile];
  const size_t fo = (size_t)blockIdx.z * H * W;
  const float limit = 4.0f * mean[blockIdx.z];
  const int x0 = blockIdx.x * kErodeTile, y0 = blockIdx.y * kErodeTile, t = threadIdx.x;
  for (int i = t; i < kErodeSpan * kErodeSpan; i += kErodeThreads) {
    const int ly = i / kErodeSpan, lx = i - ly * kErodeSpan, y = y0 + ly - kErodeR, x = x0 + lx - kErodeR;
    uint8_t p = 1;
    if (y >= 0 && y < H && x >= 0 && x < W) {
      const float v = mono[fo + (size_t)y * W + x];
      p = (v > 0.f && !(v > limit)) ? 1 : 0;
    }
    pos[ly][lx] = p;
  }
  __syncthreads();
  for (int i = t; i < kErodeSpan * kErodeTile; i += kErodeThreads) {
    const int ly = i / kErodeTile, lx = i - ly * kErodeTile;
    uint8_t m = 1;
#pragma unroll
    for (int k = 0; k <= 2 * kErodeR; ++k) m &= pos[ly][lx + k];
    row[ly][lx] = m;
  }
  __syncthreads();
  for (int i = t; i < kErodeTile * kErodeTile; i += kErodeThreads) {
    const int ly = i / kErodeTile, lx = i - ly * kErodeTile, y = y0 + ly, x = x0 + lx;
    if (y >= H || x >= W) continue;
    uint8_t m = 1;
#pragma unroll
    for (int k = 0; k <= 2 * kErodeR; ++k) m &= row[ly + k][lx];
    const size_t o = fo + (size_t)y * W + x;
    eroded[o] = m;
    filled[o] = m ? mono[o] : 0.f;
  }
}

// ================================================================================================================================
// prepare 3/3, fill: one 1024-thread workgroup per map.  stamp[p] is the pass in which p became known (0: eroded == 1).  The holes
// are compacted into a list once; pass k sweeps the list, fills every hole that has an 8-neighbour with stamp < k from the window's
// pixels with stamp < k, stamps it k and compacts the list in place to what is left.  A value or a stamp written in pass k is never
// read as known in pass k (its stamp is not below k), so the passes need no second buffer; a workgroup barrier separates them.
// ================================================================================================================================

constexpr int kFillThreads = 1024, kFillWaves = kFillThreads / 64, kFillR = 3;
constexpr int kUnknown = INT_MAX;

// rank of the thread among the workgroup's threads with flag set, in thread order, and their number (to every thread).  One flag per
// thread held in a register: a ballot and sixteen wave counts, two barriers.  (dba::scan_1024 scans an array in memory, with a
// serial chunk per thread and a log-step LDS scan of 1024 entries; the fill calls this once per 1024 list entries and pass.)
__device__ __forceinline__ int block_rank(bool flag, int* cnt, int& total) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const unsigned long long bal = __ballot(flag);
  if (lane == 0) cnt[w] = __popcll(bal);
  __syncthreads();
  int before = 0, all = 0;
#pragma unroll
  for (int k = 0; k < kFillWaves; ++k) {
    const int c = cnt[k];
    before += k < w ? c : 0;
    all += c;
  }
  __syncthreads();
  total = all;
  return before + __popcll(bal & ((1ull << lane) - 1ull));
}

__global__ void __launch_bounds__(kFillThreads) fill_kernel(int H, int W, const uint8_t* __restrict__ eroded, float* filled, int* stamp,
                                                            int* list) {
  __shared__ int cnt[kFillWaves];
  const int P = H * W, t = threadIdx.x;
  const size_t fo = (size_t)blockIdx.x * P;
  eroded += fo;
  filled += fo;
  stamp += fo;
  list += fo;
  int holes = 0;
  for (int base = 0; base < P; base += kFillThreads) {
    const int p = base + t;
    const bool hole = p < P && eroded[p] == 0;
    if (p < P) stamp[p] = hole ? kUnknown : 0;
    if (__syncthreads_count(hole) == 0) continue;
    int total;
    const int r = block_rank(hole, cnt, total);
    if (hole) list[holes + r] = p;
    holes += total;
  }
  __threadfence_block();
  __syncthreads();
  for (int pass = 1; holes > 0; ++pass) {
    int left = 0, done = 0;
    for (int base = 0; base < holes; base += kFillThreads) {
      const int i = base + t;
      const bool active = i < holes;
      const int p = active ? list[i] : 0;
      bool fill = false;
      if (active) {
        const int y = p / W, x = p - y * W;
#pragma unroll
        for (int k = 0; k < 9; ++k) {
          const int yy = y + k / 3 - 1, xx = x + k % 3 - 1;
          if (k != 4 && yy >= 0 && yy < H && xx >= 0 && xx < W) fill |= stamp[yy * W + xx] < pass;
        }
        if (fill) {
          float num = 0.f, den = 0.f;
#pragma unroll
          for (int dy = -kFillR; dy <= kFillR; ++dy) {
#pragma unroll
            for (int dx = -kFillR; dx <= kFillR; ++dx) {
              const int yy = y + dy, xx = x + dx;
              if ((dy != 0 || dx != 0) && yy >= 0 && yy < H && xx >= 0 && xx < W && stamp[yy * W + xx] < pass) {
                const float w = 1.0f / (float)(dx * dx + dy * dy);
                num += w * filled[yy * W + xx];
                den += w;
              }
            }
          }
          filled[p] = num / den;
          stamp[p] = pass;
        }
      }
      int total;
      const int r = block_rank(active && !fill, cnt, total);     // (its barrier: every thread has read list[base ..) by now)
      if (active && !fill) list[left + r] = p;
      left += total;
      done += min(kFillThreads, holes - base) - total;
    }
    holes = left;
    __threadfence_block();
    __syncthreads();
    if (done == 0) break;                                         // nothing known anywhere: the map stays zero
  }
}

// ================================================================================================================================
// depth 1/2, sums: workgroup (j, b) owns the pixels [j * 4096, (j + 1) * 4096) of frame inds[b].  Chunk c = 4 pixels belongs to thread
// c % 256, taken in increasing c; per thread, wave butterfly, waves in order.  The partition depends on H x W alone.
// ================================================================================================================================

constexpr int kThreads = 256, kWaves = kThreads / 64, kPer = 16, kSpan = kThreads * kPer;
constexpr int kSums = 6;                    // valid count, a00, a01, a11, b0, b1 (the count is exact in fp64)

inline int spans(long long P) { return (int)((P + kSpan - 1) / kSpan); }

__device__ __forceinline__ void accumulate(double (&a)[kSums], float disp, uint8_t valid, float mono, uint8_t er) {
  if (valid) a[0] += 1.0;
  if (valid && er) {
    const double x = (double)mono, y = (double)(1.0f / disp);
    a[1] += x * x;
    a[2] += x;
    a[3] += 1.0;
    a[4] += x * y;
    a[5] += y;
  }
}

__global__ void __launch_bounds__(kThreads) sums_kernel(int nf, int P, const float* __restrict__ disps, const uint8_t* __restrict__ valid,
                                                        const float* __restrict__ mono, const uint8_t* __restrict__ eroded,
                                                        const int64_t* __restrict__ inds, double* __restrict__ partial) {
  __shared__ double red[kWaves * kSums];
  const int b = blockIdx.y, j = blockIdx.x, t = threadIdx.x;
  const int64_t f = inds[b];
  if (!frame_ok(f, nf)) return;
  const size_t fo = (size_t)f * P;
  const float *d = disps + fo, *m = mono + fo;
  const uint8_t *v = valid + fo, *e = eroded + fo;
  const bool vec = (P & 3) == 0 && (((uintptr_t)d | (uintptr_t)m) & 15) == 0 && (((uintptr_t)v | (uintptr_t)e) & 3) == 0;
  const int chunks = (P + 3) >> 2, c0 = j * (kSpan / 4);
  double a[kSums] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
  for (int k = 0; k < kPer / 4; ++k) {
    const int c = c0 + k * kThreads + t;
    if (c >= chunks) break;
    if (vec) {
      const float4 dq = ((const float4*)d)[c], mq = ((const float4*)m)[c];
      const uchar4 vq = ((const uchar4*)v)[c], eq = ((const uchar4*)e)[c];
      accumulate(a, dq.x, vq.x, mq.x, eq.x);
      accumulate(a, dq.y, vq.y, mq.y, eq.y);
      accumulate(a, dq.z, vq.z, mq.z, eq.z);
      accumulate(a, dq.w, vq.w, mq.w, eq.w);
    } else {
      for (int i = 4 * c; i < min(P, 4 * c + 4); ++i) accumulate(a, d[i], v[i], m[i], e[i]);
    }
  }
  const int lane = t & 63, w = t >> 6;
#pragma unroll
  for (int i = 0; i < kSums; ++i) {
    const double s = wave_sum_f64(a[i]);
    if (lane == 0) red[w * kSums + i] = s;
  }
  __syncthreads();
  if (t < kSums) {
    double tot = red[t];
    for (int k = 1; k < kWaves; ++k) tot += red[k * kSums + t];
    partial[((size_t)b * gridDim.x + j) * kSums + t] = tot;
  }
}

// ================================================================================================================================
// depth 2/2, solve and map: every workgroup of a frame adds the frame's partials in the same order (lane l takes the spans l, l + 64,
// ... in increasing order, then the butterfly), solves the 2 x 2 system in fp64 as sgr_dspo_align does and writes its 4096 pixels.
// ================================================================================================================================

__device__ __forceinline__ float fuse_one(float disp, uint8_t valid, float mono, bool fit, float s, float q) {
#pragma clang fp contract(off)                                 // a multiply and an add, not an fma: the bits of torch's mono * s + q
  if (valid) return 1.0f / disp;
  const float scaled = s * mono;
  return fit ? scaled + q : 0.f;
}

__global__ void __launch_bounds__(kThreads) map_kernel(int nf, int P, int min_valid, const float* __restrict__ disps,
                                                       const uint8_t* __restrict__ valid, const float* __restrict__ mono,
                                                       const int64_t* __restrict__ inds, const double* __restrict__ partial,
                                                       float* __restrict__ depth, float* __restrict__ scale, float* __restrict__ shift,
                                                       uint8_t* __restrict__ invalid) {
  __shared__ double tot[kSums];
  const int b = blockIdx.y, j = blockIdx.x, t = threadIdx.x, nb = gridDim.x;
  const int64_t f = inds[b];
  if (!frame_ok(f, nf)) {                     // no such frame: flagged, and a depth of zeros rather than whatever the buffer held
    if (j == 0 && t == 0) invalid[b] = 1;
    float* o = depth + (size_t)b * P;
    for (int i = j * kSpan + t; i < min(P, (j + 1) * kSpan); i += kThreads) o[i] = 0.f;
    return;
  }
  if (t < 64) {
    double a[kSums] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int k = t; k < nb; k += 64) {
      const double* p = partial + ((size_t)b * nb + k) * kSums;
#pragma unroll
      for (int i = 0; i < kSums; ++i) a[i] += p[i];
    }
#pragma unroll
    for (int i = 0; i < kSums; ++i) {
      const double s = wave_sum_f64(a[i]);
      if (t == 0) tot[i] = s;
    }
  }
  __syncthreads();
  const bool fit = !(tot[0] < (double)min_valid);
  const double a00 = tot[1], a01 = tot[2], a11 = tot[3], b0 = tot[4], b1 = tot[5];
  const double det = a00 * a11 - a01 * a01;
  const float s = (float)((a11 * b0 - a01 * b1) / det), q = (float)((-a01 * b0 + a00 * b1) / det);
  if (j == 0 && t == 0) {
    invalid[b] = fit ? 0 : 1;
    if (fit) {
      scale[b] = s;
      shift[b] = q;
    }
  }
  const size_t fo = (size_t)f * P, oo = (size_t)b * P;
  const float *d = disps + fo, *m = mono + fo;
  const uint8_t* v = valid + fo;
  float* o = depth + oo;
  const bool vec = (P & 3) == 0 && (((uintptr_t)d | (uintptr_t)m | (uintptr_t)o) & 15) == 0 && ((uintptr_t)v & 3) == 0;
  const int chunks = (P + 3) >> 2, c0 = j * (kSpan / 4);
#pragma unroll
  for (int k = 0; k < kPer / 4; ++k) {
    const int c = c0 + k * kThreads + t;
    if (c >= chunks) break;
    if (vec) {
      const float4 dq = ((const float4*)d)[c], mq = ((const float4*)m)[c];
      const uchar4 vq = ((const uchar4*)v)[c];
      ((float4*)o)[c] = make_float4(fuse_one(dq.x, vq.x, mq.x, fit, s, q), fuse_one(dq.y, vq.y, mq.y, fit, s, q),
                                    fuse_one(dq.z, vq.z, mq.z, fit, s, q), fuse_one(dq.w, vq.w, mq.w, fit, s, q));
    } else {
      for (int i = 4 * c; i < min(P, 4 * c + 4); ++i) o[i] = fuse_one(d[i], v[i], m[i], fit, s, q);
    }
  }
}

// ================================================================================================================================
// host
// ================================================================================================================================

struct FuseScratch {
  float* mean;                              // prepare: [num]
  int* stamp;                               // prepare: [num, P]
  int* list;                                // prepare: [num, P]
  double* partial;                          // depth: [num, spans(P), kSums]
};

bool sizes_ok(int num, int ht, int wd) { return num > 0 && num <= kMaxNum && ht > 0 && wd > 0 && (long long)ht * wd < kMaxPixels; }

// prepare and depth never run at the same time on one scratch buffer: the two layouts share it
size_t carve(int num, long long P, bool prepare, char* base, FuseScratch* s) {
  size_t off = 0;
  auto take = [&](size_t bytes) {
    char* p = base ? base + off : nullptr;
    off += align_up(bytes);
    return p;
  };
  FuseScratch d = {};
  if (prepare) {
    d.mean = (float*)take((size_t)num * sizeof(float));
    d.stamp = (int*)take((size_t)num * P * sizeof(int));
    d.list = (int*)take((size_t)num * P * sizeof(int));
  } else {
    d.partial = (double*)take((size_t)num * spans(P) * kSums * sizeof(double));
  }
  if (s) *s = d;
  return off;
}

}  // namespace
}  // namespace sgr

using namespace sgr;

extern "C" {

size_t sgr_fuse_scratch_bytes(int32_t num, int32_t ht, int32_t wd) {
  if (!sizes_ok(num, ht, wd)) return 0;
  const long long P = (long long)ht * wd;
  return std::max(carve(num, P, true, nullptr, nullptr), carve(num, P, false, nullptr, nullptr));
}

int sgr_fuse_prepare(const float* mono, int32_t num, int32_t ht, int32_t wd, float* mono_filled, uint8_t* eroded, void* scratch,
                     size_t scratch_bytes, void* stream) {
  if (!mono || !mono_filled || !eroded || num < 0) return set_error(SGR_ERR_INVALID, "fuse_prepare: bad arguments");
  if (num == 0) return SGR_OK;
  if (!sizes_ok(num, ht, wd)) return set_error(SGR_ERR_INVALID, "fuse_prepare: bad sizes (num=%d ht=%d wd=%d)", num, ht, wd);
  const int P = ht * wd;
  if (!scratch || ((uintptr_t)scratch & 15) || scratch_bytes < carve(num, P, true, nullptr, nullptr))
    return set_error(SGR_ERR_WORKSPACE, "fuse_prepare: scratch too small or misaligned");
  FuseScratch s;
  carve(num, P, true, (char*)scratch, &s);
  hipStream_t st = (hipStream_t)stream;
  const dim3 tiles((wd + kErodeTile - 1) / kErodeTile, (ht + kErodeTile - 1) / kErodeTile, num);
  if (tiles.y > 65535u) return set_error(SGR_ERR_CAPACITY, "fuse_prepare: ht=%d exceeds the supported %d", ht, 65535 * kErodeTile);
  hipLaunchKernelGGL(mean_kernel, dim3(num), dim3(kMeanThreads), 0, st, P, mono, s.mean);
  hipLaunchKernelGGL(erode_kernel, tiles, dim3(kErodeThreads), 0, st, ht, wd, mono, s.mean, mono_filled, eroded);
  hipLaunchKernelGGL(fill_kernel, dim3(num), dim3(kFillThreads), 0, st, ht, wd, eroded, mono_filled, s.stamp, s.list);
  return hipGetLastError() == hipSuccess ? SGR_OK : set_error(SGR_ERR_HIP, "fuse_prepare launch failed");
}

int sgr_fuse_depth(const float* disps_up, const uint8_t* valid_depth_mask, const float* mono_filled, const uint8_t* eroded,
                   int32_t num_frames, int32_t ht, int32_t wd, const int64_t* inds, int32_t num, int32_t min_valid, float* depth,
                   float* scale, float* shift, uint8_t* invalid, void* scratch, size_t scratch_bytes, void* stream) {
  if (!disps_up || !valid_depth_mask || !mono_filled || !eroded || !inds || !depth || !scale || !shift || !invalid || num < 0 ||
      num_frames < 1)
    return set_error(SGR_ERR_INVALID, "fuse_depth: bad arguments");
  if (num == 0) return SGR_OK;
  if (!sizes_ok(num, ht, wd)) return set_error(SGR_ERR_INVALID, "fuse_depth: bad sizes (num=%d ht=%d wd=%d)", num, ht, wd);
  const int P = ht * wd;
  if (!scratch || ((uintptr_t)scratch & 15) || scratch_bytes < carve(num, P, false, nullptr, nullptr))
    return set_error(SGR_ERR_WORKSPACE, "fuse_depth: scratch too small or misaligned");
  FuseScratch s;
  carve(num, P, false, (char*)scratch, &s);
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid(spans(P), num);
  hipLaunchKernelGGL(sums_kernel, grid, dim3(kThreads), 0, st, num_frames, P, disps_up, valid_depth_mask, mono_filled, eroded, inds,
                     s.partial);
  hipLaunchKernelGGL(map_kernel, grid, dim3(kThreads), 0, st, num_frames, P, min_valid, disps_up, valid_depth_mask, mono_filled, inds,
                     s.partial, depth, scale, shift, invalid);
  return hipGetLastError() == hipSuccess ? SGR_OK : set_error(SGR_ERR_HIP, "fuse_depth launch failed");
}

}  // extern "C"
