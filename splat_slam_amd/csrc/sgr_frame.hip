// Frame preparation of the dataset streams (splat_slam_amd/datasets.py; DESIGN.md section 3, "Datasets and frame preparation"): what
// the reference's BaseDataset.__getitem__ does on the CPU per read (src/utils/datasets.py:170-216: cv2.undistort, cv2.resize, / 255, the
// nearest resize of the depth, the crop of the edge), as ONE launch over the cropped output.
//   sgr_frame_prepare      n frames of one camera: u8 colour (3 or 4 bytes a pixel) and u16 depth in, fp32 CHW colour and fp32 depth out
// The arithmetic is integer throughout (5-bit map fractions, 11-bit resize weights) so that this kernel, the numpy host path and the
// plain-Python oracle of the tests agree bit for bit; the two fp32 divisions at the end are correctly rounded.  One thread per output
// pixel, all three channels: it reads the 2 x 2 resize taps, each of them (with a map) the 2 x 2 undistortion taps behind it -- at most
// 16 source pixels, one 32-bit load each with 4 bytes a pixel -- and never writes the full-size undistorted image.  Threads of a wave
// are neighbours in x: the three colour stores and the depth store are each one coalesced row segment.  No LDS, no atomics.
#include <cstdint>

#include "sgr_common.h"

namespace sgr {
int set_error(int code, const char* fmt, ...);

namespace {

constexpr int kTx = 64, kTy = 4;            // a workgroup is 4 waves: 64 output pixels of 4 output rows
constexpr int kMaxSide = 16384;             // (2 j + 1) S and 4096 (2 D) stay far inside int32

struct FrameArgs {
  const uint8_t* color;      // [n, H, W, PS]
  const uint16_t* depth;     // [n, H, W] or null
  const int32_t* map;        // [H, W, 2] (qx, qy) in 1/32 pixel, or null
  float* out_color;          // [n, 3, H_out, W_out]
  float* out_depth;          // [n, H_out, W_out] or null
  int H, W, H_oe, W_oe, H_edge, W_edge, H_out, W_out;
  float depth_scale, sh, sw;
};

struct Tap { int s0, s1; uint32_t w0, w1; };

// the two taps and 11-bit weights of output index j of a D-sized axis over an S-sized one (pixel centres aligned, borders replicated)
__device__ __forceinline__ Tap resize_tap(int j, int S, int D) {
  const int n = (2 * j + 1) * S - D, d = 2 * D;
  int s = n >= 0 ? n / d : -((-n + d - 1) / d);       // floor
  int b = (4096 * (n - s * d) + d) / (2 * d);
  if (s < 0) { s = 0; b = 0; }
  if (s >= S - 1) { s = S - 1; b = 0; }
  Tap t;
  t.s0 = s;
  t.s1 = min(s + 1, S - 1);
  t.w0 = (uint32_t)(2048 - b);
  t.w1 = (uint32_t)b;
  return t;
}

struct Rgb { uint32_t r, g, b; };

template <int PS>
__device__ __forceinline__ Rgb load_rgb(const uint8_t* __restrict__ img, int W, int y, int x) {
  const size_t o = (size_t)y * W + x;
  Rgb p;
  if (PS == 4) {
    const uint32_t v = ((const uint32_t*)img)[o];
    p.r = v & 255u; p.g = (v >> 8) & 255u; p.b = (v >> 16) & 255u;
  } else {
    const uint8_t* q = img + o * 3;
    p.r = q[0]; p.g = q[1]; p.b = q[2];
  }
  return p;
}

// the undistorted level U of source pixel (v, u): bilinear in 1/32 pixel, a tap outside the image counts as 0
template <int PS, bool MAP>
__device__ __forceinline__ Rgb undistorted(const uint8_t* __restrict__ img, const int32_t* __restrict__ map, int H, int W, int v, int u) {
  if (!MAP) return load_rgb<PS>(img, W, v, u);
  const int2 q = ((const int2*)map)[(size_t)v * W + u];
  const int ix = q.x >> 5, iy = q.y >> 5;
  const uint32_t ax = (uint32_t)(q.x & 31), ay = (uint32_t)(q.y & 31);
  const uint32_t wx[2] = {32u - ax, ax}, wy[2] = {32u - ay, ay};
  Rgb acc = {0u, 0u, 0u};
#pragma unroll
  for (int dy = 0; dy < 2; ++dy) {
#pragma unroll
    for (int dx = 0; dx < 2; ++dx) {
      const int yy = iy + dy, xx = ix + dx;
      if (yy >= 0 && yy < H && xx >= 0 && xx < W) {
        const Rgb p = load_rgb<PS>(img, W, yy, xx);
        const uint32_t w = wx[dx] * wy[dy];
        acc.r += w * p.r; acc.g += w * p.g; acc.b += w * p.b;
      }
    }
  }
  acc.r = (acc.r + 512u) >> 10; acc.g = (acc.g + 512u) >> 10; acc.b = (acc.b + 512u) >> 10;
  return acc;
}

template <int PS, bool MAP>
__global__ void __launch_bounds__(kTx * kTy) frame_prepare_kernel(FrameArgs a) {
  const int x = blockIdx.x * kTx + threadIdx.x, y = blockIdx.y * kTy + threadIdx.y;
  if (x >= a.W_out || y >= a.H_out) return;
  const size_t f = blockIdx.z, plane = (size_t)a.H_out * a.W_out, src_px = (size_t)a.H * a.W;
  const int oy = y + a.H_edge, ox = x + a.W_edge;
  const uint8_t* img = a.color + f * src_px * PS;
  const Tap ty = resize_tap(oy, a.H, a.H_oe), tx = resize_tap(ox, a.W, a.W_oe);
  const int vs[2] = {ty.s0, ty.s1}, us[2] = {tx.s0, tx.s1};
  const uint32_t wy[2] = {ty.w0, ty.w1}, wx[2] = {tx.w0, tx.w1};
  uint32_t r = 0u, g = 0u, b = 0u;          // <= 255 * 2^22: 32 unsigned bits
#pragma unroll
  for (int j = 0; j < 2; ++j) {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const uint32_t w = wy[j] * wx[i];
      if (w == 0u) continue;                  // (weight 0 contributes 0: the second tap of a 1:1 or clamped axis is not loaded)
      const Rgb p = undistorted<PS, MAP>(img, a.map, a.H, a.W, vs[j], us[i]);
      r += w * p.r; g += w * p.g; b += w * p.b;
    }
  }
  const size_t o = f * 3 * plane + (size_t)y * a.W_out + x;
  a.out_color[o] = __fdiv_rn((float)((r + (1u << 21)) >> 22), 255.0f);
  a.out_color[o + plane] = __fdiv_rn((float)((g + (1u << 21)) >> 22), 255.0f);
  a.out_color[o + 2 * plane] = __fdiv_rn((float)((b + (1u << 21)) >> 22), 255.0f);
  if (a.depth) {
    // torch's nearest: min((int)floorf(dst * (float)in / (float)out), in - 1); one fp32 product, nothing to contract
    const int sy = min((int)floorf(__fmul_rn((float)oy, a.sh)), a.H - 1);
    const int sx = min((int)floorf(__fmul_rn((float)ox, a.sw)), a.W - 1);
    a.out_depth[f * plane + (size_t)y * a.W_out + x] = __fdiv_rn((float)a.depth[f * src_px + (size_t)sy * a.W + sx], a.depth_scale);
  }
}

template <int PS, bool MAP>
void launch(const FrameArgs& a, int n, hipStream_t st) {
  const dim3 grid((a.W_out + kTx - 1) / kTx, (a.H_out + kTy - 1) / kTy, n);
  hipLaunchKernelGGL((frame_prepare_kernel<PS, MAP>), grid, dim3(kTx, kTy), 0, st, a);
}

}  // namespace
}  // namespace sgr

using namespace sgr;

extern "C" {

int sgr_frame_prepare(int32_t n, const uint8_t* color_u8, int32_t ps, const uint16_t* depth_u16, int32_t H, int32_t W, const int32_t* map_q,
                      int32_t H_oe, int32_t W_oe, int32_t H_edge, int32_t W_edge, float depth_scale, float* out_color, float* out_depth,
                      void* stream) {
  if (n < 1 || n > 65535 || !color_u8 || !out_color || (ps != 3 && ps != 4))
    return set_error(SGR_ERR_INVALID, "frame_prepare: bad arguments (n=%d ps=%d)", n, ps);
  if (H < 1 || W < 1 || H > kMaxSide || W > kMaxSide || H_oe < 1 || W_oe < 1 || H_oe > kMaxSide || W_oe > kMaxSide)
    return set_error(SGR_ERR_INVALID, "frame_prepare: sizes %d x %d -> %d x %d outside [1, %d]", H, W, H_oe, W_oe, kMaxSide);
  if (H_edge < 0 || W_edge < 0 || 2 * (int64_t)H_edge >= H_oe || 2 * (int64_t)W_edge >= W_oe)
    return set_error(SGR_ERR_INVALID, "frame_prepare: edges (%d, %d) leave nothing of %d x %d", H_edge, W_edge, H_oe, W_oe);
  if ((depth_u16 == nullptr) != (out_depth == nullptr))
    return set_error(SGR_ERR_INVALID, "frame_prepare: depth_u16 and out_depth go together");
  if (depth_u16 && !(depth_scale > 0.0f && depth_scale <= 3.0e38f))
    return set_error(SGR_ERR_INVALID, "frame_prepare: depth_scale must be positive and finite");
  if ((ps == 4 && ((uintptr_t)color_u8 & 3)) || ((uintptr_t)map_q & 7) || ((uintptr_t)depth_u16 & 1) || ((uintptr_t)out_color & 3) ||
      ((uintptr_t)out_depth & 3))
    return set_error(SGR_ERR_INVALID, "frame_prepare: a pointer is not aligned to its element (4-byte pixels: 4, map: 8)");
  FrameArgs a;
  a.color = color_u8; a.depth = depth_u16; a.map = map_q; a.out_color = out_color; a.out_depth = out_depth;
  a.H = H; a.W = W; a.H_oe = H_oe; a.W_oe = W_oe; a.H_edge = H_edge; a.W_edge = W_edge;
  a.H_out = H_oe - 2 * H_edge; a.W_out = W_oe - 2 * W_edge;
  a.depth_scale = depth_scale;
  a.sh = (float)H / (float)H_oe;
  a.sw = (float)W / (float)W_oe;
  hipStream_t st = (hipStream_t)stream;
  if (ps == 4) {
    if (map_q) launch<4, true>(a, n, st); else launch<4, false>(a, n, st);
  } else {
    if (map_q) launch<3, true>(a, n, st); else launch<3, false>(a, n, st);
  }
  return hipGetLastError() == hipSuccess ? SGR_OK : set_error(SGR_ERR_HIP, "frame_prepare launch failed");
}

}  // extern "C"
