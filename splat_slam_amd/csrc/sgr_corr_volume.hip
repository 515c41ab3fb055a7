// The all-pairs correlation volume of the frontend's factor graph (CorrBlock of modules/droid_net/corr.py), built for a batch of
// edges straight into the slots of a store that the lookup reads in place (splat_slam_amd.corr.FusedCorrBlock).
//   sgr_corr_volume_pyramid   V0[e,p1,p2] = (1/16) sum_c maps[src[e],c,p1] maps[dst[e],c,p2] on mfma_f32_16x16x32_f16 and its 2 x 2
//                             block means of levels 1..3, every level reduced from the fp32 accumulators and rounded to fp16 once
// Stated in DESIGN.md section 3, "Fused correlation volume".
//
// Tile.  One workgroup of 256 threads owns kP1 = 64 consecutive pixels p1 of map 1 and a patch of 8 rows x 64 columns of map 2 (rows
// 8 b .., columns 64 t ..; at w = 64 a patch is 512 consecutive p2, one 1 KB run of level 0 per p1).  The patch is the footprint of one
// row of level 3, two of level 2 and four of level 1, so the workgroup writes all four levels and level 0 is never read back.  The
// pixels of map 2 are the A operand and those of map 1 the B operand: a lane of an accumulator holds four consecutive p2 of one p1.
// Wave v owns the patch rows 2 v and 2 v + 1 (8 A tiles of 16 columns) against all four B tiles: 32 accumulator tiles, 128 registers.
// The maps are channels first, so the k loop stages 32 channels at a time through LDS: a thread loads 8 consecutive pixels of two
// channels (16 bytes each where the run is aligned), and writes them transposed, a packed pair of channels per pixel.
// Epilogue, one B tile (16 p1) at a time: the accumulators times 1/16 go to LDS as fp32 [16][512]; level 0 leaves as 16-byte stores
// of 8 consecutive p2; level 1 is 0.25 ((a + b) + (c + d)) over rows (2 y, 2 y + 1) and columns (2 x, 2 x + 1), kept in LDS as
// fp32 for level 2, and so on.  Positions outside the map are staged as zeros and never stored.  Every sum has a fixed order that
// depends on the pixel's place in its patch alone: an edge gives the same bits alone, in any batch and in any slot.
#include <cstdint>

#include "sgr_common.h"

namespace sgr {
int set_error(int code, const char* fmt, ...);

namespace {

typedef _Float16 half_t;
typedef __attribute__((ext_vector_type(4))) _Float16 half4;
typedef __attribute__((ext_vector_type(8))) _Float16 half8;
typedef __attribute__((ext_vector_type(4))) float floatx4;

constexpr int kThreads = 256;
constexpr int kP1 = 64;                     // pixels of map 1 per workgroup: four B tiles
constexpr int kPatchRows = 8, kPatchCols = 64, kPos = kPatchRows * kPatchCols;      // the patch of map 2: 32 A tiles
constexpr int kBK = SGR_CORR_VOLUME_CHANNEL_STEP;     // one MFMA k step
constexpr int kRow = kBK + 8;               // halfs per LDS row of the staged operands (80 bytes: fragment reads spread over the banks)
constexpr int kMaxLevels = SGR_CORR_PYRAMID_MAX_LEVELS;
constexpr int kMaxChannels = SGR_CORR_VOLUME_MAX_CHANNELS;
constexpr int kMaxEdges = SGR_CORR_VOLUME_MAX_EDGES;       // a grid dimension
constexpr int kStride0 = kPos + 4, kStride1 = kPos / 4 + 4, kStride2 = kPos / 16 + 1;   // floats per p1 of the epilogue's level images
constexpr int kStageBytes = (kPos + kP1) * kRow * 2;
constexpr int kEpiBytes = 16 * (kStride0 + kStride1 + kStride2) * 4;
constexpr int kLdsBytes = kStageBytes > kEpiBytes ? kStageBytes : kEpiBytes;

struct VolumeLevels {
  half_t* v[kMaxLevels];
};

// 8 consecutive pixels, from element `off` of its plane on, of channel ch (a) and ch + 1 (b) of one map; pixels from nvalid on are zero
__device__ __forceinline__ void load_pair(const half_t* __restrict__ maps, int64_t chan, int HW, int off, int nvalid, bool vec, half8& a,
                                          half8& b) {
  const int64_t e0 = chan * HW + off;
  if (vec && nvalid == 8 && ((e0 | HW) & 7) == 0) {
    a = *(const half8*)(maps + e0);
    b = *(const half8*)(maps + e0 + HW);
  } else {
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      a[i] = i < nvalid ? maps[e0 + i] : (half_t)0.f;
      b[i] = i < nvalid ? maps[e0 + HW + i] : (half_t)0.f;
    }
  }
}
// ... transposed into rows [row0, row0 + 8) of a staged operand, at the channel pair cp of the k step
__device__ __forceinline__ void stage_pair(half_t* rows, int row0, int cp, const half8& a, const half8& b) {
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    typedef __attribute__((ext_vector_type(2))) _Float16 half2v;
    *(half2v*)&rows[(row0 + i) * kRow + 2 * cp] = half2v{a[i], b[i]};
  }
}

__global__ void __launch_bounds__(kThreads) corr_volume_pyramid_kernel(const half_t* __restrict__ maps, const int64_t* __restrict__ src,
                                                                       const int64_t* __restrict__ dst, const int64_t* __restrict__ slots,
                                                                       VolumeLevels lv, int planes, int capacity, int C, int h, int w, int L,
                                                                       int groups, int col_tiles, bool vec) {
  __shared__ __attribute__((aligned(16))) char lds[kLdsBytes];
  half_t* As = (half_t*)lds;                            // [kPos][kRow]: the patch of map 2, one k step
  half_t* Bs = As + kPos * kRow;                        // [kP1][kRow]: the pixels of map 1
  float* img0 = (float*)lds;                            // the epilogue's images, over the staged operands
  float* img1 = img0 + 16 * kStride0;
  float* img2 = img1 + 16 * kStride1;

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int e = blockIdx.y;
  const int64_t slot = slots[e];
  if (slot < 0 || slot >= capacity) return;             // the same in every thread of the workgroup
  const int64_t fs = src[e], fd = dst[e];
  const bool edge_in = fs >= 0 && fs < planes && fd >= 0 && fd < planes;
  const int g = blockIdx.x % groups, patch = blockIdx.x / groups;
  const int band = patch / col_tiles, y0 = band * kPatchRows, x0 = (patch - band * col_tiles) * kPatchCols;
  const int HW = h * w, p10 = g * kP1;

  // this thread's share of a k step: four (channel pair, 8 columns of a patch row) of map 2 and, for tid < 128, one of map 1
  const int cp = tid & 15;
  half8 ra0[4], ra1[4], rb0, rb1;
  auto gload = [&](int kt) {
    const int ch = kt * kBK + 2 * cp;
#pragma unroll
    for (int it = 0; it < 4; ++it) {
      const int s = it * 16 + (tid >> 4), y = y0 + (s >> 3), x = x0 + (s & 7) * 8;
      const int nvalid = (edge_in && y < h) ? min(max(w - x, 0), 8) : 0;
      load_pair(maps, (edge_in ? fd : 0) * C + ch, HW, y * w + x, nvalid, vec, ra0[it], ra1[it]);
    }
    if (tid < 128) {
      const int p = p10 + (tid >> 4) * 8;
      load_pair(maps, (edge_in ? fs : 0) * C + ch, HW, p, edge_in ? min(max(HW - p, 0), 8) : 0, vec, rb0, rb1);
    }
  };

  floatx4 acc[8][4];
#pragma unroll
  for (int a = 0; a < 8; ++a)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[a][j] = floatx4{0.f, 0.f, 0.f, 0.f};

  const int nk = C / kBK;
  gload(0);
  for (int kt = 0; kt < nk; ++kt) {
#pragma unroll
    for (int it = 0; it < 4; ++it) stage_pair(As, (it * 16 + (tid >> 4)) * 8, cp, ra0[it], ra1[it]);
    if (tid < 128) stage_pair(Bs, (tid >> 4) * 8, cp, rb0, rb1);
    __syncthreads();
    if (kt + 1 < nk) gload(kt + 1);
    half8 bf[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) bf[j] = *(const half8*)&Bs[(j * 16 + (lane & 15)) * kRow + (lane >> 4) * 8];
#pragma unroll
    for (int a = 0; a < 8; ++a) {
      const half8 af = *(const half8*)&As[((wave * 8 + a) * 16 + (lane & 15)) * kRow + (lane >> 4) * 8];
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[a][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(af, bf[j], acc[a][j], 0, 0, 0);
    }
    __syncthreads();
  }

  // acc[a][j][r] is position (wave * 8 + a) * 16 + 4 (lane >> 4) + r of the patch (row = position / 64) against p1 = p10 + 16 j + (lane & 15)
  const int64_t plane0 = slot * HW;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
#pragma unroll
    for (int a = 0; a < 8; ++a)
      *(floatx4*)&img0[(lane & 15) * kStride0 + (wave * 8 + a) * 16 + 4 * (lane >> 4)] = acc[a][j] * 0.0625f;
    __syncthreads();
    const int pj = p10 + 16 * j;
    // level 0: 8 consecutive columns per thread, a wave covers the patch of one p1
#pragma unroll
    for (int it = 0; it < 4; ++it) {
      const int idx = it * kThreads + tid, pl = idx >> 6, s = idx & 63, y = y0 + (s >> 3), x = x0 + (s & 7) * 8, p1 = pj + pl;
      if (p1 < HW && y < h && x < w) {
        const floatx4 v0 = *(const floatx4*)&img0[pl * kStride0 + s * 8], v1 = *(const floatx4*)&img0[pl * kStride0 + s * 8 + 4];
        half8 o;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          o[i] = (half_t)v0[i];
          o[4 + i] = (half_t)v1[i];
        }
        const int64_t at = (plane0 + p1) * HW + (int64_t)y * w + x;
        const int n = min(w - x, 8);
        if (vec && n == 8 && (at & 7) == 0) {
          *(half8*)(lv.v[0] + at) = o;
        } else {
#pragma unroll
          for (int i = 0; i < 8; ++i)
            if (i < n) lv.v[0][at + i] = o[i];
        }
      }
    }
    // level 1: four consecutive columns per thread
    if (L > 1) {
      const int h1 = h >> 1, w1 = w >> 1;
#pragma unroll
      for (int it = 0; it < 2; ++it) {
        const int idx = it * kThreads + tid, pl = idx >> 5, q = idx & 31, r1 = q >> 3, c1 = (q & 7) * 4, p1 = pj + pl;
        const float* top = &img0[pl * kStride0 + (2 * r1) * kPatchCols + 2 * c1];
        const floatx4 t0 = *(const floatx4*)top, t1 = *(const floatx4*)(top + 4);
        const floatx4 b0 = *(const floatx4*)(top + kPatchCols), b1 = *(const floatx4*)(top + kPatchCols + 4);
        floatx4 v;
        v[0] = 0.25f * ((t0[0] + t0[1]) + (b0[0] + b0[1]));
        v[1] = 0.25f * ((t0[2] + t0[3]) + (b0[2] + b0[3]));
        v[2] = 0.25f * ((t1[0] + t1[1]) + (b1[0] + b1[1]));
        v[3] = 0.25f * ((t1[2] + t1[3]) + (b1[2] + b1[3]));
        *(floatx4*)&img1[pl * kStride1 + r1 * (kPatchCols / 2) + c1] = v;
        const int y = y0 / 2 + r1, x = x0 / 2 + c1;
        if (p1 < HW && y < h1 && x < w1) {
          half4 o;
#pragma unroll
          for (int i = 0; i < 4; ++i) o[i] = (half_t)v[i];
          const int64_t at = (plane0 + p1) * ((int64_t)h1 * w1) + (int64_t)y * w1 + x;
          const int n = min(w1 - x, 4);
          if (vec && n == 4 && (at & 3) == 0) {
            *(half4*)(lv.v[1] + at) = o;
          } else {
#pragma unroll
            for (int i = 0; i < 4; ++i)
              if (i < n) lv.v[1][at + i] = o[i];
          }
        }
      }
    }
    __syncthreads();
    if (L > 2) {
      const int h2 = h >> 2, w2 = w >> 2;
#pragma unroll
      for (int it = 0; it < 2; ++it) {
        const int idx = it * kThreads + tid, pl = idx >> 5, q = idx & 31, r2 = q >> 4, c2 = q & 15, p1 = pj + pl;
        const float* top = &img1[pl * kStride1 + (2 * r2) * (kPatchCols / 2) + 2 * c2];
        const float v = 0.25f * ((top[0] + top[1]) + (top[kPatchCols / 2] + top[kPatchCols / 2 + 1]));
        img2[pl * kStride2 + r2 * (kPatchCols / 4) + c2] = v;
        const int y = y0 / 4 + r2, x = x0 / 4 + c2;
        if (p1 < HW && y < h2 && x < w2) lv.v[2][(plane0 + p1) * ((int64_t)h2 * w2) + (int64_t)y * w2 + x] = (half_t)v;
      }
    }
    __syncthreads();
    if (L > 3 && tid < 128) {
      const int h3 = h >> 3, w3 = w >> 3;
      const int pl = tid >> 3, c3 = tid & 7, p1 = pj + pl;
      const float* top = &img2[pl * kStride2 + 2 * c3];
      const float v = 0.25f * ((top[0] + top[1]) + (top[kPatchCols / 4] + top[kPatchCols / 4 + 1]));
      const int y = y0 / 8, x = x0 / 8 + c3;
      if (p1 < HW && y < h3 && x < w3) lv.v[3][(plane0 + p1) * ((int64_t)h3 * w3) + (int64_t)y * w3 + x] = (half_t)v;
    }
  }
}

inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace
}  // namespace sgr

using namespace sgr;

extern "C" {

int sgr_corr_volume_pyramid(const void* maps, const int64_t* src, const int64_t* dst, const int64_t* slots, void* level0, void* level1,
                            void* level2, void* level3, int32_t planes, int32_t edges, int32_t capacity, int32_t channels, int32_t h,
                            int32_t w, int32_t num_levels, void* stream) {
  const char* what = "corr_volume_pyramid";
  if (!maps || !src || !dst || !slots) return set_error(SGR_ERR_INVALID, "%s: null argument", what);
  if (num_levels < 1 || num_levels > kMaxLevels)
    return set_error(SGR_ERR_INVALID, "%s: num_levels (%d) must lie in [1, %d]", what, num_levels, kMaxLevels);
  if (planes < 1 || capacity < 1 || edges < 0 || h < 1 || w < 1)
    return set_error(SGR_ERR_INVALID, "%s: bad sizes (planes=%d edges=%d capacity=%d h=%d w=%d)", what, planes, edges, capacity, h, w);
  if (channels < kBK || channels % kBK || channels > kMaxChannels)
    return set_error(SGR_ERR_CAPACITY, "%s: channels (%d) must be a positive multiple of %d up to %d", what, channels, kBK, kMaxChannels);
  if ((int64_t)h * w > INT32_MAX - kPos || edges > kMaxEdges)
    return set_error(SGR_ERR_CAPACITY, "%s: h*w must fit in int32 and edges (%d) must not exceed %d", what, edges, kMaxEdges);
  VolumeLevels lv = {{(half_t*)level0, (half_t*)level1, (half_t*)level2, (half_t*)level3}};
  bool vec = aligned16(maps);
  for (int l = 0; l < kMaxLevels; ++l) {
    if (l >= num_levels) lv.v[l] = nullptr;
    else if (!lv.v[l] && (h >> l) > 0 && (w >> l) > 0) return set_error(SGR_ERR_INVALID, "%s: level %d is null", what, l);
    vec = vec && aligned16(lv.v[l]);
  }
  if (edges == 0) return SGR_OK;
  const int HW = h * w, groups = (HW + kP1 - 1) / kP1, col_tiles = (w + kPatchCols - 1) / kPatchCols;
  const int64_t nblocks = (int64_t)groups * ((h + kPatchRows - 1) / kPatchRows) * col_tiles;
  if (nblocks > INT32_MAX) return set_error(SGR_ERR_CAPACITY, "%s: maps of %d x %d are too large", what, h, w);
  hipLaunchKernelGGL(corr_volume_pyramid_kernel, dim3((unsigned)nblocks, (unsigned)edges), dim3(kThreads), 0, (hipStream_t)stream,
                     (const half_t*)maps, src, dst, slots, lv, planes, capacity, channels, h, w, num_levels, groups, col_tiles, vec);
  return hipGetLastError() == hipSuccess ? SGR_OK : set_error(SGR_ERR_HIP, "%s launch failed", what);
}

}  // extern "C"
