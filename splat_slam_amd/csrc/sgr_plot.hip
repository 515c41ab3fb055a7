// The per-keyframe figure of the rendering evaluation (the reference's src/utils/eval_utils.py:131-135, plot_rgbd_silhouette), DESIGN.md
// section 3, "Plots": sgr_plot_panels turns up to 16 frames per launch pair into one RGB panel each, 2 x 3 cells reduced by an integer
// factor, with a heading and a title per cell.
//   launch 1  plot_maxima_kernel    per frame the maximum of the colour difference (an integer sum of levels) and of the depth difference
//                                   (the bits of a non-negative float): integer atomicMax, order-independent, hence reproducible
//   launch 2  plot_compose_kernel   four consecutive panel pixels per thread, 12 bytes in three aligned words; every byte written once
// Both launches see the frames through the copy of the caller's table in scratch (a table with its text is 7.9 KB: no kernel argument).
// Every float expression that decides a colour is one correctly rounded operation (__fmul_rn, __fsub_rn, __fdiv_rn), so numpy's fp32
// restates it bit for bit; the rest is integer arithmetic.
#include <algorithm>
#include <cmath>
#include <cstdint>

#include "sgr_common.h"
#include "sgr_plot_tables.h"

namespace sgr {
int set_error(int code, const char* fmt, ...);

namespace {

constexpr int kThreads = 256;
constexpr int kMaxBlocks = 64;            // launch 1: workgroups per frame (each strides over the frame)
constexpr int kGroup = 4;                 // launch 2: panel pixels per thread
constexpr int kM = SGR_PLOT_MARGIN, kCW = SGR_PLOT_CHAR_W, kCH = SGR_PLOT_CHAR_H, kGap = SGR_PLOT_TITLE_GAP, kText = SGR_PLOT_TEXT;
constexpr int kFontScale = 2;
constexpr int kMaxSide = 16384;
constexpr uint32_t kWhite = 0xffffffu;    // a pixel is r | g << 8 | b << 16
static_assert(kCW >= kFontScale * plot::kGlyphW && kCH >= kFontScale * plot::kGlyphH, "a glyph fits its character cell");
static_assert(sizeof(SgrPlotFrame) == 6 * 8 + 7 * kText && sizeof(SgrPlotFrame) % 8 == 0, "the table is copied as it is");

struct Geometry { int H, W, s, ch, cw, PH, PW; };

inline bool geometry(int H, int W, int s, Geometry* g) {
  if (H < 1 || W < 1 || H > kMaxSide || W > kMaxSide || s < 1) return false;
  g->H = H; g->W = W; g->s = s;
  g->ch = (H + s - 1) / s;
  g->cw = (W + s - 1) / s;
  g->PW = kM + 3 * (g->cw + kM);
  g->PH = 2 * kM + kCH + 2 * (kCH + kGap + g->ch + kM);
  return true;
}

inline size_t table_bytes(int n) { return align_up((size_t)n * sizeof(SgrPlotFrame)); }

struct Maxima { uint32_t rgb, depth_bits; };

__device__ __forceinline__ uint32_t jet(int idx) {
  const unsigned char* e = plot::kJet[idx];
  return (uint32_t)e[0] | (uint32_t)e[1] << 8 | (uint32_t)e[2] << 16;
}
// jet(t): entry clamp(floor(256 t), 0, 255); t is finite here
__device__ __forceinline__ uint32_t jet_of(float t) {
  const float v = __fmul_rn(256.f, t);
  return jet(v >= 255.f ? 255 : (v > 0.f ? (int)v : 0));
}
__device__ __forceinline__ int gt_level(float g) { return color_level(fminf(fmaxf(g, 0.f), 1.f)); }

struct FrameView {
  const float *render, *gt, *depth, *gt_depth;
  float ea, eb;
};
__device__ __forceinline__ FrameView view_of(const SgrPlotFrame& f) {
  return {f.render, f.gt_image, f.depth, f.gt_depth, f.exposure_a ? expf(f.exposure_a[0]) : 1.f, f.exposure_b ? f.exposure_b[0] : 0.f};
}
// e of cell (0,2): the sum over the channels of |ground-truth level - render level|, 0 .. 765
__device__ __forceinline__ int rgb_difference(const FrameView& v, size_t HW, size_t o) {
  int e = 0;
#pragma unroll
  for (int c = 0; c < 3; ++c) e += abs(gt_level(v.gt[c * HW + o]) - color_level(exposed_image(v.ea, v.render[c * HW + o], v.eb)));
  return e;
}
// e of cell (1,2): |global_scale d - gd| where both depths are > 0 (eval_utils.py:116-119), else 0; may be inf or NaN
__device__ __forceinline__ float depth_difference(const FrameView& v, size_t o, float global_scale) {
  const float d = v.depth[o], gd = v.gt_depth[o];
  return (d > 0.f && gd > 0.f) ? fabsf(__fsub_rn(__fmul_rn(global_scale, d), gd)) : 0.f;
}

// ---- launch 1: grid (blocks, frames)
__global__ void __launch_bounds__(kThreads) plot_maxima_kernel(const SgrPlotFrame* __restrict__ tab, int HW, float global_scale,
                                                               Maxima* __restrict__ maxima) {
  const FrameView v = view_of(tab[blockIdx.y]);
  uint32_t m_rgb = 0, m_dep = 0;
  for (int o = blockIdx.x * kThreads + threadIdx.x; o < HW; o += gridDim.x * kThreads) {
    m_rgb = max(m_rgb, (uint32_t)rgb_difference(v, (size_t)HW, (size_t)o));
    const float e = depth_difference(v, (size_t)o, global_scale);
    if (isfinite(e)) m_dep = max(m_dep, __float_as_uint(e));          // e >= 0: its bits order as the value
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    m_rgb = max(m_rgb, (uint32_t)__shfl_xor((int)m_rgb, off));
    m_dep = max(m_dep, (uint32_t)__shfl_xor((int)m_dep, off));
  }
  if ((threadIdx.x & 63) == 0) {
    if (m_rgb) atomicMax(&maxima[blockIdx.y].rgb, m_rgb);
    if (m_dep) atomicMax(&maxima[blockIdx.y].depth_bits, m_dep);
  }
}

// ---- launch 2
struct ComposeArgs {
  Geometry g;
  float global_scale, depth_max;
  size_t pixels;                          // k * PH * PW
};

// the byte triple a full-size plot shows at source pixel o of cell (row, col)
__device__ __forceinline__ uint32_t source_pixel(const FrameView& v, int row, int col, size_t HW, size_t o, const ComposeArgs& a,
                                                 Maxima mx) {
  if (col == 0) {
    uint32_t p = 0;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const int level = row == 0 ? gt_level(v.gt[c * HW + o]) : color_level(exposed_image(v.ea, v.render[c * HW + o], v.eb));
      p |= (uint32_t)level << (8 * c);
    }
    return p;
  }
  if (col == 1) {
    const float x = row == 0 ? v.gt_depth[o] : __fmul_rn(a.global_scale, v.depth[o]);
    return isfinite(x) ? jet_of(__fdiv_rn(x, a.depth_max)) : kWhite;
  }
  if (row == 0) {
    const int e = rgb_difference(v, HW, o);
    return jet(mx.rgb ? min(255, 256 * e / (int)mx.rgb) : 0);
  }
  const float e = depth_difference(v, o, a.global_scale);
  if (!isfinite(e)) return kWhite;
  return jet_of(mx.depth_bits ? __fdiv_rn(e, __uint_as_float(mx.depth_bits)) : 0.f);
}

// pixel (ty, tx) of a text drawn from its top left: black where the glyph has a dot
__device__ __forceinline__ uint32_t text_pixel(const char* text, int ty, int tx) {
  const int ci = tx / kCW, gx = (tx % kCW) / kFontScale, gy = ty / kFontScale;
  if (ci >= kText - 1 || gx >= plot::kGlyphW || gy >= plot::kGlyphH) return kWhite;
  for (int k = 0; k < ci; ++k)
    if (text[k] == 0) return kWhite;
  int code = (unsigned char)text[ci];
  if (code == 0) return kWhite;
  if (code < plot::kGlyphFirst || code > plot::kGlyphLast) code = '?';
  return (plot::kGlyph[code - plot::kGlyphFirst][gy] >> (plot::kGlyphW - 1 - gx)) & 1 ? 0u : kWhite;
}

__device__ uint32_t panel_pixel(const SgrPlotFrame& f, Maxima mx, int py, int px, const ComposeArgs& a) {
  const Geometry& g = a.g;
  if (px < kM || py < kM) return kWhite;
  if (py < kM + kCH) return px < g.PW - kM ? text_pixel(f.heading, py - kM, px - kM) : kWhite;
  const int col = (px - kM) / (g.cw + kM), x = (px - kM) % (g.cw + kM);
  const int band = kCH + kGap + g.ch + kM, yy = py - (2 * kM + kCH);
  if (yy < 0 || x >= g.cw) return kWhite;
  const int row = yy / band, y = yy % band;
  if (row > 1 || col > 2) return kWhite;
  if (y < kCH) return text_pixel(f.titles + (3 * row + col) * kText, y, x);
  const int iy = y - (kCH + kGap);
  if (iy < 0 || iy >= g.ch) return kWhite;
  const FrameView v = view_of(f);
  const size_t HW = (size_t)g.H * g.W;
  const int y0 = iy * g.s, y1 = min(y0 + g.s, g.H), x0 = x * g.s, x1 = min(x0 + g.s, g.W);
  uint32_t sum[3] = {0, 0, 0};
  for (int sy = y0; sy < y1; ++sy)
    for (int sx = x0; sx < x1; ++sx) {
      const uint32_t p = source_pixel(v, row, col, HW, (size_t)sy * g.W + sx, a, mx);
      sum[0] += p & 0xffu; sum[1] += (p >> 8) & 0xffu; sum[2] += p >> 16;
    }
  const uint32_t cnt = (uint32_t)((y1 - y0) * (x1 - x0));
  return (sum[0] + cnt / 2) / cnt | ((sum[1] + cnt / 2) / cnt) << 8 | ((sum[2] + cnt / 2) / cnt) << 16;
}

__global__ void __launch_bounds__(kThreads) plot_compose_kernel(const SgrPlotFrame* __restrict__ tab, const Maxima* __restrict__ maxima,
                                                                ComposeArgs a, uint8_t* __restrict__ panels) {
  const size_t p0 = ((size_t)blockIdx.x * kThreads + threadIdx.x) * kGroup;
  if (p0 >= a.pixels) return;
  const size_t per = (size_t)a.g.PH * a.g.PW;
  uint32_t rgb[kGroup];
  const int cnt = (int)min((size_t)kGroup, a.pixels - p0);
#pragma unroll
  for (int k = 0; k < kGroup; ++k) {
    rgb[k] = 0;
    if (k < cnt) {
      const size_t p = p0 + k;
      const int f = (int)(p / per), q = (int)(p % per);
      rgb[k] = panel_pixel(tab[f], maxima[f], q / a.g.PW, q % a.g.PW, a);
    }
  }
  if (cnt == kGroup) {                    // 12 bytes at a multiple of 12: three aligned words (panels is 4-byte aligned)
    uint32_t* w = (uint32_t*)(panels + 3 * p0);
    w[0] = rgb[0] | rgb[1] << 24;
    w[1] = rgb[1] >> 8 | rgb[2] << 16;
    w[2] = rgb[2] >> 16 | rgb[3] << 8;
  } else {
    for (int k = 0; k < cnt; ++k) {
      uint8_t* b = panels + 3 * (p0 + k);
      b[0] = (uint8_t)rgb[k]; b[1] = (uint8_t)(rgb[k] >> 8); b[2] = (uint8_t)(rgb[k] >> 16);
    }
  }
}

}  // namespace
}  // namespace sgr

using namespace sgr;

extern "C" {

void sgr_plot_panel_size(int32_t H, int32_t W, int32_t s, int32_t* PH, int32_t* PW) {
  Geometry g = {};
  geometry(H, W, s, &g);
  if (PH) *PH = g.PH;
  if (PW) *PW = g.PW;
}

size_t sgr_plot_scratch_bytes(int32_t n) {
  return n > 0 ? table_bytes(n) + align_up((size_t)n * sizeof(Maxima)) : 0;
}

int sgr_plot_panels(int32_t n, const SgrPlotFrame* frames, int32_t H, int32_t W, int32_t s, float global_scale, float depth_max,
                    uint8_t* panels, void* scratch, size_t scratch_bytes, void* stream) {
  ComposeArgs a = {};
  if (n <= 0 || !frames || !panels || !geometry(H, W, s, &a.g)) return set_error(SGR_ERR_INVALID, "plot_panels: null/size");
  if (!std::isfinite(global_scale) || !(depth_max > 0.f) || !std::isfinite(depth_max))
    return set_error(SGR_ERR_INVALID, "plot_panels: global_scale must be finite and depth_max positive and finite");
  if (((uintptr_t)panels & 3) != 0) return set_error(SGR_ERR_INVALID, "plot_panels: panels must be 4-byte aligned");
  for (int i = 0; i < n; ++i)
    if (!frames[i].render || !frames[i].gt_image || !frames[i].depth || !frames[i].gt_depth)
      return set_error(SGR_ERR_INVALID, "plot_panels: frame %d has no image or no depth", i);
  if (!scratch || scratch_bytes < sgr_plot_scratch_bytes(n))
    return set_error(SGR_ERR_WORKSPACE, "plot_panels scratch too small (need %zu)", sgr_plot_scratch_bytes(n));
  hipStream_t st = (hipStream_t)stream;
  SgrPlotFrame* tab = (SgrPlotFrame*)scratch;
  Maxima* maxima = (Maxima*)((char*)scratch + table_bytes(n));
  if (hipMemcpyAsync(tab, frames, (size_t)n * sizeof(SgrPlotFrame), hipMemcpyHostToDevice, st) != hipSuccess ||
      hipMemsetAsync(maxima, 0, (size_t)n * sizeof(Maxima), st) != hipSuccess)
    return set_error(SGR_ERR_HIP, "plot_panels: copy of the frame table failed");
  a.global_scale = global_scale;
  a.depth_max = depth_max;
  const int HW = H * W;
  const size_t per = (size_t)a.g.PH * a.g.PW;
  const int blocks = std::min(kMaxBlocks, (HW + kThreads - 1) / kThreads);
  for (int f0 = 0; f0 < n; f0 += SGR_PLOT_MAX_FRAMES) {
    const int k = std::min(n - f0, (int)SGR_PLOT_MAX_FRAMES);
    a.pixels = (size_t)k * per;
    hipLaunchKernelGGL(plot_maxima_kernel, dim3(blocks, k), dim3(kThreads), 0, st, tab + f0, HW, global_scale, maxima + f0);
    const size_t groups = (a.pixels + kGroup - 1) / kGroup;
    hipLaunchKernelGGL(plot_compose_kernel, dim3((unsigned)((groups + kThreads - 1) / kThreads)), dim3(kThreads), 0, st, tab + f0,
                       maxima + f0, a, panels + (size_t)f0 * per * 3);
  }
  return hipGetLastError() == hipSuccess ? SGR_OK : set_error(SGR_ERR_HIP, "plot_panels launch failed");
}

}  // extern "C"
