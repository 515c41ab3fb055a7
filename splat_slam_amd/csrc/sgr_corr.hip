// Correlation lookups of the tracker's update operator: the other half of the droid_backends extension of the reference
// (thirdparty/glorie_slam/lib/correlation_kernels.cu, altcorr_kernel.cu), reached from modules/droid_net/corr.py.
//   sgr_corr_index_forward   corr_index_forward: bilinear (2r+1)^2 window out of each pixel's plane of an all-pairs volume
//   sgr_corr_index_backward  corr_index_backward: its transpose, every element of volume_grad written once
//   sgr_corr_alt_forward     altcorr_forward: the same window with the correlations computed on the fly from two feature maps
//   sgr_corr_alt_backward    altcorr_backward: gradients of that with respect to both feature maps
//   sgr_corr_index_pyramid_forward  corr_index_forward at every level of a volume pyramid kept in slots (sgr_corr_volume.hip), one launch
//   sgr_corr_alt_pyramid_forward  altcorr_forward at every level of a feature pyramid in one launch, the frames of each edge read
//                            through their indices out of an fp16 or fp32 store (the low-memory lookup of FactorGraph.update_lowmem)
// Layout and measured times: DESIGN.md section 3, "Correlation lookups".  Outputs are indexed x offset first, then y offset.  Sums
// are kept in fp32 registers and rounded once on the store; every output element is written exactly once.  Only fmap2_grad is a
// scatter with collisions (fp32 global atomic adds, one 256-byte channel segment per wave instruction): everything else is owned
// by one thread or wave and bitwise reproducible.
#include <cstdint>

#include "sgr_common.h"

namespace sgr {
int set_error(int code, const char* fmt, ...);

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kMaxRadius = SGR_CORR_MAX_RADIUS;    // keeps floor(x0) - radius + i far inside int32 behind the guard below
constexpr int kMaxRegRadius = SGR_CORR_PYRAMID_MAX_RADIUS;   // corr_index_forward keeps a window row in registers up to here (the network's is 3)
constexpr int kAltTile = 64;                // altcorr_forward: pixels of one workgroup = one coalesced 256-byte store per output plane
constexpr size_t kAltLdsLimit = 60 * 1024;

// The integer window of one pixel.  Decided in float BEFORE any conversion to int: a pixel whose floor(x0) or floor(y0) is not
// finite (NaN compares false) or lies outside [-(r+2), w2+r+1] resp. [-(r+2), h2+r+1] has no corner inside the map (a corner
// needs floor(x0) in [-(r+1), w2+r-1]) and is dead: it reads nothing, its outputs and gradient contributions are 0.
struct Window {
  int fx, fy;
  float dx, dy;
  bool live;
};
__device__ __forceinline__ Window make_window(float x0, float y0, int r, int h2, int w2) {
  const float flx = floorf(x0), fly = floorf(y0);
  Window w;
  w.live = flx >= -(float)(r + 2) && flx <= (float)(w2 + r + 1) && fly >= -(float)(r + 2) && fly <= (float)(h2 + r + 1);
  w.fx = w.live ? (int)flx : 0;
  w.fy = w.live ? (int)fly : 0;
  w.dx = w.live ? x0 - flx : 0.f;
  w.dy = w.live ? y0 - fly : 0.f;
  return w;
}

// ---- corr_index: volume [B,h1,w1,h2,w2] (pixel p = (n,y,x) owns the plane p), coords [B,2,h1,w1], corr [B,rd,rd,h1,w1]
// One thread per pixel, lanes along x: the stores to each of the rd*rd output planes are coalesced.  The window is walked row
// by row: each of its (rd+1)^2 elements is loaded once, interpolated along x against its left neighbour, and two consecutive
// rows give one row of outputs.
// The window walk of one pixel, shared by corr_index_fwd_kernel and corr_index_pyramid_fwd_kernel: plane [h2,w2] is the pixel's own,
// out its first output, the rd*rd outputs HW1 elements apart.
template <typename T, int R>
__device__ __forceinline__ void index_window(const T* __restrict__ plane, const Window& w, int h2, int w2, T* __restrict__ out, int HW1) {
  constexpr int RD = 2 * R + 1;
  const float wx0 = 1.f - w.dx, wy0 = 1.f - w.dy;
  float hprev[RD];
#pragma unroll
  for (int j = 0; j <= RD; ++j) {
    const int y1 = w.fy - R + j;
    const bool row_in = w.live && y1 >= 0 && y1 < h2;
    const T* row = plane + (row_in ? y1 * w2 : 0);
    float h[RD], vprev = 0.f;
#pragma unroll
    for (int i = 0; i <= RD; ++i) {
      const int x1 = w.fx - R + i;
      const float v = (row_in && x1 >= 0 && x1 < w2) ? (float)row[x1] : 0.f;
      if (i > 0) h[i - 1] = wx0 * vprev + w.dx * v;
      vprev = v;
    }
#pragma unroll
    for (int a = 0; a < RD; ++a) {
      if (j > 0) out[(int64_t)(a * RD + (j - 1)) * HW1] = (T)(wy0 * hprev[a] + w.dy * h[a]);
      hprev[a] = h[a];
    }
  }
}

template <typename T, int R>
__global__ void __launch_bounds__(kThreads) corr_index_fwd_kernel(const T* __restrict__ volume, const float* __restrict__ coords,
                                                                  T* __restrict__ corr, int P, int HW1, int h2, int w2) {
  constexpr int RD = 2 * R + 1;
  const int p = blockIdx.x * kThreads + threadIdx.x;
  if (p >= P) return;
  const int n = p / HW1, yx = p - n * HW1;
  const float* cp = coords + (int64_t)n * 2 * HW1 + yx;
  const Window w = make_window(cp[0], cp[HW1], R, h2, w2);
  index_window<T, R>(volume + (int64_t)p * (h2 * w2), w, h2, w2, corr + (int64_t)n * (RD * RD) * HW1 + yx, HW1);
}

// ---- corr_index over the slots of a volume pyramid: level_l [capacity,h,w,h>>l,w>>l] fp16, slots [E], coords [E,h,w,2] (x, y),
// corr [E, L*rd*rd, h, w].  blockIdx.y is the level; one thread per (edge, pixel) walks the window of corr_index_fwd_kernel in the
// plane of slot slots[e] at coords * 2^-l (an exact scaling).  An empty level and a slot outside the store are dead windows: zeros.
struct SlotLevels {
  const _Float16* v[4];
};
template <int R>
__global__ void __launch_bounds__(kThreads) corr_index_pyramid_fwd_kernel(SlotLevels lv, const int64_t* __restrict__ slots,
                                                                          const float* __restrict__ coords, _Float16* __restrict__ corr,
                                                                          int P, int HW, int h, int w, int capacity, int L) {
  constexpr int RD = 2 * R + 1;
  const int p = blockIdx.x * kThreads + threadIdx.x;
  if (p >= P) return;
  const int l = blockIdx.y, h2 = h >> l, w2 = w >> l;
  const int e = p / HW, yx = p - e * HW;
  const float2 c = *(const float2*)(coords + (int64_t)p * 2);
  const float scale = 1.f / (float)(1 << l);           // a power of two: coords * scale == coords / 2^l exactly
  const int64_t slot = slots[e];
  const bool on = slot >= 0 && slot < capacity && h2 > 0 && w2 > 0;
  Window win = make_window(c.x * scale, c.y * scale, R, h2, w2);
  if (!on) win = Window{0, 0, 0.f, 0.f, false};
  const _Float16* base = l == 0 ? lv.v[0] : l == 1 ? lv.v[1] : l == 2 ? lv.v[2] : lv.v[3];
  const _Float16* plane = base + (on ? (slot * HW + yx) * ((int64_t)h2 * w2) : 0);
  index_window<_Float16, R>(plane, win, h2, w2, corr + ((int64_t)e * L + l) * (RD * RD) * HW + yx, HW);
}

// any radius: every output gathers its own four corners (no per-thread arrays whose size depends on the radius)
template <typename T>
__global__ void __launch_bounds__(kThreads) corr_index_fwd_any_kernel(const T* __restrict__ volume, const float* __restrict__ coords,
                                                                      T* __restrict__ corr, int P, int HW1, int h2, int w2, int r) {
  const int rd = 2 * r + 1;
  const int p = blockIdx.x * kThreads + threadIdx.x;
  if (p >= P) return;
  const int n = p / HW1, yx = p - n * HW1;
  const float* cp = coords + (int64_t)n * 2 * HW1 + yx;
  const Window w = make_window(cp[0], cp[HW1], r, h2, w2);
  const float wx0 = 1.f - w.dx, wy0 = 1.f - w.dy;
  const T* plane = volume + (int64_t)p * (h2 * w2);
  T* out = corr + (int64_t)n * rd * rd * HW1 + yx;
  auto at = [&](int y1, int x1) { return (w.live && y1 >= 0 && y1 < h2 && x1 >= 0 && x1 < w2) ? (float)plane[y1 * w2 + x1] : 0.f; };
  for (int a = 0; a < rd; ++a)
    for (int b = 0; b < rd; ++b) {
      const int x1 = w.fx - r + a, y1 = w.fy - r + b;
      const float top = wx0 * at(y1, x1) + w.dx * at(y1, x1 + 1), bot = wx0 * at(y1 + 1, x1) + w.dx * at(y1 + 1, x1 + 1);
      out[((int64_t)a * rd + b) * HW1] = (T)(wy0 * top + w.dy * bot);
    }
}

// One thread per element of volume_grad (lanes along w2: coalesced stores): inside the (rd+1)^2 window of its plane it gathers
// the up to four outputs it fed, outside it writes the zero.
template <typename T>
__global__ void __launch_bounds__(kThreads) corr_index_bwd_kernel(const float* __restrict__ coords, const T* __restrict__ corr_grad,
                                                                  T* __restrict__ volume_grad, int64_t total, int HW1, int HW2, int h2,
                                                                  int w2, int r) {
  const int64_t idx = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (idx >= total) return;
  const int rd = 2 * r + 1;
  const int p = (int)(idx / HW2), rem = (int)(idx - (int64_t)p * HW2);
  const int y1 = rem / w2, x1 = rem - y1 * w2;
  const int n = p / HW1, yx = p - n * HW1;
  const float* cp = coords + (int64_t)n * 2 * HW1 + yx;
  const Window w = make_window(cp[0], cp[HW1], r, h2, w2);
  float g = 0.f;
  const int i = x1 - (w.fx - r), j = y1 - (w.fy - r);
  if (w.live && i >= 0 && i <= rd && j >= 0 && j <= rd) {
    const T* cg = corr_grad + (int64_t)n * rd * rd * HW1 + yx;
    const float wx0 = 1.f - w.dx, wy0 = 1.f - w.dy;
    auto at = [&](int a, int b) { return (float)cg[((int64_t)a * rd + b) * HW1]; };
    if (i > 0 && j > 0) g += at(i - 1, j - 1) * (w.dx * w.dy);
    if (i > 0 && j < rd) g += at(i - 1, j) * (w.dx * wy0);
    if (i < rd && j > 0) g += at(i, j - 1) * (wx0 * w.dy);
    if (i < rd && j < rd) g += at(i, j) * (wx0 * wy0);
  }
  volume_grad[idx] = (T)g;
}

// ---- altcorr: fmap1 [B,H1,W1,C], fmap2 [B,H2,W2,C], coords [B,N,H1,W1,2], corr [B,N,rd*rd,H1,W1]
__device__ __forceinline__ float dot4(float4 a, float4 b) { return a.x * b.x + a.y * b.y + a.z * b.z + a.w * b.w; }

// A workgroup owns `tile` consecutive pixels of one (b, n); its four waves take them in turn.  For one pixel, half a wave reads
// one channel row of fmap2 as float4 (512 contiguous bytes at C = 128) against the pixel's fmap1 row held in registers, so a wave
// computes two of the (rd+1)^2 dot products per step and each product exactly once; a fixed butterfly sums the 32 lanes.  The
// dots go to LDS, the rd*rd outputs are spread from them, and the tile's outputs leave through LDS so that the store to each
// output plane is one run of `tile` consecutive pixels.
__global__ void __launch_bounds__(kThreads) altcorr_fwd_kernel(const float* __restrict__ fmap1, const float* __restrict__ fmap2,
                                                               const float* __restrict__ coords, float* __restrict__ corr, int N,
                                                               int HW1, int H2, int W2, int C4, int r, int tile, int tiles_per) {
  extern __shared__ float lds[];
  const int rd = 2 * r + 1, rc = rd + 1, nc = rc * rc, no = rd * rd, stride = tile + 1;
  float* outt = lds;                                   // [no][tile + 1]
  float* dots = lds + (size_t)no * stride;             // [kWaves][nc]
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, half = lane >> 5, l32 = lane & 31;
  const int bn = blockIdx.x / tiles_per, t0 = (blockIdx.x - bn * tiles_per) * tile;
  const int b = bn / N;
  const int npx = min(tile, HW1 - t0);
  const float4* f2 = (const float4*)fmap2 + (int64_t)b * H2 * W2 * C4;
  float* mydots = dots + wave * nc;
  for (int px0 = 0; px0 < npx; px0 += kWaves) {        // uniform trip count: the barriers below are taken by every wave
    const int px = px0 + wave;
    const bool active = px < npx;
    Window w = {0, 0, 0.f, 0.f, false};
    const float4* f1 = nullptr;
    float4 f1a = {0.f, 0.f, 0.f, 0.f};
    if (active) {
      const int yx = t0 + px;
      const float* cp = coords + ((int64_t)bn * HW1 + yx) * 2;
      w = make_window(cp[0], cp[1], r, H2, W2);
      f1 = (const float4*)fmap1 + ((int64_t)b * HW1 + yx) * C4;
      if (w.live && l32 < C4) f1a = f1[l32];
    }
    if (w.live) {                                      // the same in every lane of the wave
      for (int k0 = 0; k0 < nc; k0 += 2) {
        const int k = k0 + half;
        const int ix = k / rc, iy = k - ix * rc;
        const int x2 = w.fx - r + ix, y2 = w.fy - r + iy;
        float s = 0.f;
        if (k < nc && x2 >= 0 && x2 < W2 && y2 >= 0 && y2 < H2) {
          const float4* row = f2 + (int64_t)(y2 * W2 + x2) * C4;
          if (l32 < C4) s = dot4(f1a, row[l32]);
          for (int c = l32 + 32; c < C4; c += 32) s += dot4(f1[c], row[c]);
        }
#pragma unroll
        for (int off = 16; off > 0; off >>= 1) s += __shfl_xor(s, off);
        if (l32 == 0 && k < nc) mydots[k] = s;
      }
    }
    __syncthreads();
    if (active) {
      const float wx0 = 1.f - w.dx, wy0 = 1.f - w.dy;
      for (int o = lane; o < no; o += 64) {
        const int ax = o / rd, ay = o - ax * rd;
        const float* d = mydots + ax * rc + ay;          // corner (ix, iy) sits at ix * rc + iy
        outt[o * stride + px] = w.live ? wy0 * (wx0 * d[0] + w.dx * d[rc]) + w.dy * (wx0 * d[1] + w.dx * d[rc + 1]) : 0.f;
      }
    }
    __syncthreads();
  }
  float* out = corr + (int64_t)bn * no * HW1 + t0;
  for (int e = threadIdx.x; e < no * tile; e += kThreads) {
    const int o = e / tile, px = e - o * tile;
    if (px < npx) out[(int64_t)o * HW1 + px] = outt[o * stride + px];
  }
}

// One wave per pixel (b, h, w), lanes along the channels.  fmap1_grad[b,h,w,:] sums over every n and corner in registers and is
// stored once.  fmap2_grad (zero on entry) takes one atomic add of a whole channel segment (64 consecutive floats) per corner.
__global__ void __launch_bounds__(kThreads) altcorr_bwd_kernel(const float* __restrict__ fmap1, const float* __restrict__ fmap2,
                                                               const float* __restrict__ coords, const float* __restrict__ corr_grad,
                                                               float* __restrict__ fmap1_grad, float* __restrict__ fmap2_grad, int BHW,
                                                               int N, int HW1, int H2, int W2, int C, int r) {
  const int rd = 2 * r + 1, no = rd * rd;
  const int lane = threadIdx.x & 63;
  const int p = blockIdx.x * kWaves + (threadIdx.x >> 6);
  if (p >= BHW) return;
  const int b = p / HW1, yx = p - b * HW1;
  const float* f1 = fmap1 + (int64_t)p * C;
  const float* f2 = fmap2 + (int64_t)b * H2 * W2 * C;
  float* g2 = fmap2_grad + (int64_t)b * H2 * W2 * C;
  for (int c = lane; c < C; c += 64) {
    const float f1c = f1[c];
    float acc = 0.f;
    for (int n = 0; n < N; ++n) {
      const int64_t bn = (int64_t)b * N + n;
      const float* cp = coords + (bn * HW1 + yx) * 2;
      const Window w = make_window(cp[0], cp[1], r, H2, W2);
      if (!w.live) continue;
      const float wx0 = 1.f - w.dx, wy0 = 1.f - w.dy;
      const float* cg = corr_grad + bn * no * HW1 + yx;
      for (int ix = 0; ix <= rd; ++ix) {
        const int x2 = w.fx - r + ix;
        if (x2 < 0 || x2 >= W2) continue;
        for (int iy = 0; iy <= rd; ++iy) {
          const int y2 = w.fy - r + iy;
          if (y2 < 0 || y2 >= H2) continue;
          auto at = [&](int ax, int ay) { return cg[((int64_t)ax * rd + ay) * HW1]; };
          float g = 0.f;
          if (ix > 0 && iy > 0) g += at(ix - 1, iy - 1) * (w.dx * w.dy);
          if (ix > 0 && iy < rd) g += at(ix - 1, iy) * (w.dx * wy0);
          if (ix < rd && iy > 0) g += at(ix, iy - 1) * (wx0 * w.dy);
          if (ix < rd && iy < rd) g += at(ix, iy) * (wx0 * wy0);
          const int64_t row = (int64_t)(y2 * W2 + x2) * C + c;
          acc += g * f2[row];
          atomicAdd(g2 + row, g * f1c);
        }
      }
    }
    fmap1_grad[(int64_t)p * C + c] = acc;
  }
}

// ---- altcorr over a pyramid: levels[l] [F,H>>l,W>>l,C] (fp16 or fp32), src, dst [E], coords [E,H,W,2], corr [E,L*rd*rd,H,W]
constexpr int kMaxPyramidLevels = SGR_CORR_PYRAMID_MAX_LEVELS;
constexpr size_t kPyramidLdsTarget = 32 * 1024;     // the output tile is halved until a workgroup needs no more than this

struct PyramidLevels {
  const void* map[kMaxPyramidLevels];
};

typedef _Float16 half4_t __attribute__((ext_vector_type(4)));
typedef _Float16 half8_t __attribute__((ext_vector_type(8)));

// sum over the C channels of two rows as one chain of fused multiply-adds in channel order (fp16 widened in the instruction:
// v_fma_mix_f32); a is the same address in every lane
__device__ __forceinline__ float dot_rows(const float* __restrict__ a, const float* __restrict__ b, int C) {
  float s = 0.f;
#pragma unroll 4
  for (int c = 0; c < C; c += 4) {
    const float4 x = *(const float4*)(a + c), y = *(const float4*)(b + c);
    s = fmaf(x.w, y.w, fmaf(x.z, y.z, fmaf(x.y, y.y, fmaf(x.x, y.x, s))));
  }
  return s;
}
__device__ __forceinline__ float dot_rows(const _Float16* __restrict__ a, const _Float16* __restrict__ b, int C) {
  float s = 0.f;
  if ((C & 7) == 0) {                                // rows are 16-byte aligned: one 16-byte load per lane and step
#pragma unroll 4
    for (int c = 0; c < C; c += 8) {
      const half8_t x = *(const half8_t*)(a + c), y = *(const half8_t*)(b + c);
#pragma unroll
      for (int i = 0; i < 8; ++i) s = fmaf((float)x[i], (float)y[i], s);
    }
  } else {
    for (int c = 0; c < C; c += 4) {
      const half4_t x = *(const half4_t*)(a + c), y = *(const half4_t*)(b + c);
#pragma unroll
      for (int i = 0; i < 4; ++i) s = fmaf((float)x[i], (float)y[i], s);
    }
  }
  return s;
}

// A workgroup owns `tile` consecutive pixels of one edge; its four waves take them in turn.  For one pixel the (level, corner)
// pairs are dealt to the lanes, x-adjacent corners (contiguous rows of the level's map) to adjacent lanes: at r = 3 every level is
// exactly one wave.  A lane walks the channels of its own row against the pixel's fmap1 row, whose address is the same in every lane
// (scalar loads), so a dot product is one chain of fused multiply-adds in one lane: no reduction across lanes, and bits that depend
// on the edge and the pixel alone.  The dots go to LDS, the L*rd*rd outputs are spread from them, and the tile's outputs leave
// through LDS so that the store to each output plane is one run of `tile` consecutive pixels.
template <typename T>
__global__ void __launch_bounds__(kThreads) altcorr_pyramid_fwd_kernel(PyramidLevels lv, const int64_t* __restrict__ src,
                                                                       const int64_t* __restrict__ dst,
                                                                       const float* __restrict__ coords, float* __restrict__ corr,
                                                                       int F, int H, int W, int C, int r, int L, int tile,
                                                                       int tiles_per) {
  extern __shared__ float lds[];
  const int rd = 2 * r + 1, rc = rd + 1, nc = rc * rc, no = rd * rd, items = L * nc, outs = L * no, stride = tile + 1, HW = H * W;
  float* outt = lds;                                   // [outs][tile + 1]
  float* dots = lds + (size_t)outs * stride;           // [kWaves][items], corner (ix, iy) of level l at l * nc + iy * rc + ix
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int e = blockIdx.x / tiles_per, t0 = (blockIdx.x - e * tiles_per) * tile;
  const int64_t fs = src[e], fd = dst[e];
  const bool edge_in = fs >= 0 && fs < F && fd >= 0 && fd < F;       // as sgr_graph_reproject: zeros, and nothing is read
  const int npx = min(tile, HW - t0);
  float* mydots = dots + wave * items;
  for (int px0 = 0; px0 < npx; px0 += kWaves) {        // uniform trip count: the barriers below are taken by every wave
    const int px = px0 + wave;
    const bool active = px < npx;
    float x0 = 0.f, y0 = 0.f;
    if (active) {
      const int yx = t0 + px;
      const float* cp = coords + ((int64_t)e * HW + yx) * 2;
      x0 = cp[0];
      y0 = cp[1];
      const T* f1 = (const T*)lv.map[0] + (edge_in ? ((int64_t)fs * HW + yx) * C : 0);
      for (int item = lane; item < items; item += 64) {
        const int l = item / nc, k = item - l * nc, iy = k / rc, ix = k - iy * rc;
        const int Hl = H >> l, Wl = W >> l;
        const float scale = 1.f / (float)(1 << l);     // a power of two: coords * scale == coords / 2^l exactly
        const Window w = make_window(x0 * scale, y0 * scale, r, Hl, Wl);
        const int x2 = w.fx - r + ix, y2 = w.fy - r + iy;
        float s = 0.f;
        if (edge_in && w.live && x2 >= 0 && x2 < Wl && y2 >= 0 && y2 < Hl) {
          const void* base = l == 0 ? lv.map[0] : l == 1 ? lv.map[1] : l == 2 ? lv.map[2] : lv.map[3];
          s = dot_rows(f1, (const T*)base + (((int64_t)fd * Hl + y2) * Wl + x2) * C, C);
        }
        mydots[item] = s;
      }
    }
    __syncthreads();
    if (active) {
      for (int o = lane; o < outs; o += 64) {
        const int l = o / no, q = o - l * no, ax = q / rd, ay = q - ax * rd;
        const int Hl = H >> l, Wl = W >> l;
        const float scale = 1.f / (float)(1 << l);
        const Window w = make_window(x0 * scale, y0 * scale, r, Hl, Wl);
        const float wx0 = 1.f - w.dx, wy0 = 1.f - w.dy;
        const float* d = mydots + l * nc + ay * rc + ax;
        const bool on = edge_in && w.live && Hl > 0 && Wl > 0;
        outt[o * stride + px] = on ? wy0 * (wx0 * d[0] + w.dx * d[1]) + w.dy * (wx0 * d[rc] + w.dx * d[rc + 1]) : 0.f;
      }
    }
    __syncthreads();
  }
  float* out = corr + (int64_t)e * outs * HW + t0;
  for (int i = threadIdx.x; i < outs * tile; i += kThreads) {
    const int o = i / tile, px = i - o * tile;
    if (px < npx) out[(int64_t)o * HW + px] = outt[o * stride + px];
  }
}

inline bool fits_i32(int64_t v) { return v >= 0 && v <= INT32_MAX; }

template <typename T>
void launch_index_fwd(const void* volume, const float* coords, void* corr, int P, int HW1, int h2, int w2, int r, hipStream_t st) {
  const dim3 grid((P + kThreads - 1) / kThreads), block(kThreads);
  const T* v = (const T*)volume;
  T* o = (T*)corr;
  switch (r) {
    case 0: hipLaunchKernelGGL((corr_index_fwd_kernel<T, 0>), grid, block, 0, st, v, coords, o, P, HW1, h2, w2); break;
    case 1: hipLaunchKernelGGL((corr_index_fwd_kernel<T, 1>), grid, block, 0, st, v, coords, o, P, HW1, h2, w2); break;
    case 2: hipLaunchKernelGGL((corr_index_fwd_kernel<T, 2>), grid, block, 0, st, v, coords, o, P, HW1, h2, w2); break;
    case 3: hipLaunchKernelGGL((corr_index_fwd_kernel<T, 3>), grid, block, 0, st, v, coords, o, P, HW1, h2, w2); break;
    case 4: hipLaunchKernelGGL((corr_index_fwd_kernel<T, 4>), grid, block, 0, st, v, coords, o, P, HW1, h2, w2); break;
    default: hipLaunchKernelGGL((corr_index_fwd_any_kernel<T>), grid, block, 0, st, v, coords, o, P, HW1, h2, w2, r); break;
  }
  static_assert(kMaxRegRadius == 4, "one case per register radius");
}

// shapes shared by the two corr_index entry points: B*h1*w1 and h2*w2 each fit int32, everything beyond is indexed in 64 bits
int index_sizes(const char* what, int32_t dtype, int32_t batch, int32_t h1, int32_t w1, int32_t h2, int32_t w2, int32_t radius) {
  if (dtype != SGR_CORR_F32 && dtype != SGR_CORR_F16) return set_error(SGR_ERR_INVALID, "%s: dtype must be SGR_CORR_F32 or SGR_CORR_F16", what);
  if (batch < 1 || h1 < 1 || w1 < 1 || h2 < 1 || w2 < 1 || radius < 0 || radius > kMaxRadius)
    return set_error(SGR_ERR_INVALID, "%s: bad sizes (batch=%d h1=%d w1=%d h2=%d w2=%d radius=%d)", what, batch, h1, w1, h2, w2, radius);
  if (!fits_i32((int64_t)batch * h1 * w1) || !fits_i32((int64_t)h2 * w2))
    return set_error(SGR_ERR_CAPACITY, "%s: batch*h1*w1 and h2*w2 must each fit in int32", what);
  return SGR_OK;
}

}  // namespace
}  // namespace sgr

using namespace sgr;

extern "C" {

int sgr_corr_index_forward(const void* volume, const float* coords, void* corr, int32_t dtype, int32_t batch, int32_t h1, int32_t w1,
                           int32_t h2, int32_t w2, int32_t radius, void* stream) {
  if (!volume || !coords || !corr) return set_error(SGR_ERR_INVALID, "corr_index_forward: null argument");
  if (int rc = index_sizes("corr_index_forward", dtype, batch, h1, w1, h2, w2, radius)) return rc;
  const int P = batch * h1 * w1;
  if (dtype == SGR_CORR_F16)
    launch_index_fwd<_Float16>(volume, coords, corr, P, h1 * w1, h2, w2, radius, (hipStream_t)stream);
  else
    launch_index_fwd<float>(volume, coords, corr, P, h1 * w1, h2, w2, radius, (hipStream_t)stream);
  return hipGetLastError() == hipSuccess ? SGR_OK : set_error(SGR_ERR_HIP, "corr_index_forward launch failed");
}

int sgr_corr_index_backward(const float* coords, const void* corr_grad, void* volume_grad, int32_t dtype, int32_t batch, int32_t h1,
                            int32_t w1, int32_t h2, int32_t w2, int32_t radius, void* stream) {
  if (!coords || !corr_grad || !volume_grad) return set_error(SGR_ERR_INVALID, "corr_index_backward: null argument");
  if (int rc = index_sizes("corr_index_backward", dtype, batch, h1, w1, h2, w2, radius)) return rc;
  const int64_t total = (int64_t)batch * h1 * w1 * h2 * w2, nblocks = (total + kThreads - 1) / kThreads;
  if (!fits_i32(nblocks)) return set_error(SGR_ERR_CAPACITY, "corr_index_backward: volume of %lld elements is too large", (long long)total);
  const dim3 grid((unsigned)nblocks), block(kThreads);
  if (dtype == SGR_CORR_F16)
    hipLaunchKernelGGL((corr_index_bwd_kernel<_Float16>), grid, block, 0, (hipStream_t)stream, coords, (const _Float16*)corr_grad,
                       (_Float16*)volume_grad, total, h1 * w1, h2 * w2, h2, w2, radius);
  else
    hipLaunchKernelGGL((corr_index_bwd_kernel<float>), grid, block, 0, (hipStream_t)stream, coords, (const float*)corr_grad,
                       (float*)volume_grad, total, h1 * w1, h2 * w2, h2, w2, radius);
  return hipGetLastError() == hipSuccess ? SGR_OK : set_error(SGR_ERR_HIP, "corr_index_backward launch failed");
}

static int alt_sizes(const char* what, int32_t batch, int32_t num, int32_t h1, int32_t w1, int32_t h2, int32_t w2, int32_t channels,
                     int32_t radius) {
  if (batch < 1 || num < 1 || h1 < 1 || w1 < 1 || h2 < 1 || w2 < 1 || radius < 0 || radius > kMaxRadius)
    return set_error(SGR_ERR_INVALID, "%s: bad sizes (batch=%d num=%d h1=%d w1=%d h2=%d w2=%d radius=%d)", what, batch, num, h1, w1, h2, w2,
                     radius);
  if (channels < 4 || channels % 4) return set_error(SGR_ERR_INVALID, "%s: channels (%d) must be a positive multiple of 4", what, channels);
  if (!fits_i32((int64_t)batch * num * h1 * w1) || !fits_i32((int64_t)h2 * w2))
    return set_error(SGR_ERR_CAPACITY, "%s: batch*num*h1*w1 and h2*w2 must each fit in int32", what);
  return SGR_OK;
}

int sgr_corr_alt_forward(const float* fmap1, const float* fmap2, const float* coords, float* corr, int32_t batch, int32_t num, int32_t h1,
                         int32_t w1, int32_t h2, int32_t w2, int32_t channels, int32_t radius, void* stream) {
  if (!fmap1 || !fmap2 || !coords || !corr) return set_error(SGR_ERR_INVALID, "corr_alt_forward: null argument");
  if (int rc = alt_sizes("corr_alt_forward", batch, num, h1, w1, h2, w2, channels, radius)) return rc;
  const int rd = 2 * radius + 1, HW1 = h1 * w1;
  auto lds_bytes = [&](int tile) { return ((size_t)rd * rd * (tile + 1) + (size_t)kWaves * (rd + 1) * (rd + 1)) * sizeof(float); };
  int tile = kAltTile;
  while (tile > 1 && lds_bytes(tile) > kAltLdsLimit) tile >>= 1;
  if (lds_bytes(tile) > kAltLdsLimit)
    return set_error(SGR_ERR_CAPACITY, "corr_alt_forward: radius %d needs more than %zu bytes of LDS per pixel", radius, kAltLdsLimit);
  const int tiles_per = (HW1 + tile - 1) / tile;
  const int64_t nblocks = (int64_t)batch * num * tiles_per;
  if (!fits_i32(nblocks)) return set_error(SGR_ERR_CAPACITY, "corr_alt_forward: too many pixels");
  hipLaunchKernelGGL(altcorr_fwd_kernel, dim3((unsigned)nblocks), dim3(kThreads), lds_bytes(tile), (hipStream_t)stream, fmap1, fmap2, coords,
                     corr, num, HW1, h2, w2, channels / 4, radius, tile, tiles_per);
  return hipGetLastError() == hipSuccess ? SGR_OK : set_error(SGR_ERR_HIP, "corr_alt_forward launch failed");
}

int sgr_corr_alt_pyramid_forward(const void* level0, const void* level1, const void* level2, const void* level3, const int64_t* src,
                                 const int64_t* dst, const float* coords, float* corr, int32_t dtype, int32_t frames, int32_t edges,
                                 int32_t h, int32_t w, int32_t channels, int32_t radius, int32_t num_levels, void* stream) {
  const char* what = "corr_alt_pyramid_forward";
  if (!src || !dst || !coords || !corr) return set_error(SGR_ERR_INVALID, "%s: null argument", what);
  if (dtype != SGR_CORR_F32 && dtype != SGR_CORR_F16) return set_error(SGR_ERR_INVALID, "%s: dtype must be SGR_CORR_F32 or SGR_CORR_F16", what);
  if (num_levels < 1 || num_levels > kMaxPyramidLevels)
    return set_error(SGR_ERR_INVALID, "%s: num_levels (%d) must lie in [1, %d]", what, num_levels, kMaxPyramidLevels);
  if (frames < 1) return set_error(SGR_ERR_INVALID, "%s: frames (%d) must be positive", what, frames);
  if (int rc = alt_sizes(what, 1, edges, h, w, h, w, channels, radius)) return rc;
  if (radius > kMaxRegRadius) return set_error(SGR_ERR_CAPACITY, "%s: radius %d exceeds the supported %d", what, radius, kMaxRegRadius);
  PyramidLevels lv = {{level0, level1, level2, level3}};
  for (int l = 0; l < kMaxPyramidLevels; ++l) {
    if (l >= num_levels) lv.map[l] = nullptr;
    else if (!lv.map[l] && (h >> l) > 0 && (w >> l) > 0) return set_error(SGR_ERR_INVALID, "%s: level %d is null", what, l);
  }
  const int rd = 2 * radius + 1, HW = h * w, outs = num_levels * rd * rd, items = num_levels * (rd + 1) * (rd + 1);
  auto lds_bytes = [&](int tile) { return ((size_t)outs * (tile + 1) + (size_t)kWaves * items) * sizeof(float); };
  int tile = kAltTile;
  while (tile > 1 && lds_bytes(tile) > kPyramidLdsTarget) tile >>= 1;
  const int tiles_per = (HW + tile - 1) / tile;
  const int64_t nblocks = (int64_t)edges * tiles_per;
  if (!fits_i32(nblocks)) return set_error(SGR_ERR_CAPACITY, "%s: too many pixels", what);
  const dim3 grid((unsigned)nblocks), block(kThreads);
  if (dtype == SGR_CORR_F16)
    hipLaunchKernelGGL((altcorr_pyramid_fwd_kernel<_Float16>), grid, block, lds_bytes(tile), (hipStream_t)stream, lv, src, dst, coords, corr,
                       frames, h, w, channels, radius, num_levels, tile, tiles_per);
  else
    hipLaunchKernelGGL((altcorr_pyramid_fwd_kernel<float>), grid, block, lds_bytes(tile), (hipStream_t)stream, lv, src, dst, coords, corr,
                       frames, h, w, channels, radius, num_levels, tile, tiles_per);
  return hipGetLastError() == hipSuccess ? SGR_OK : set_error(SGR_ERR_HIP, "%s launch failed", what);
}

int sgr_corr_index_pyramid_forward(const void* level0, const void* level1, const void* level2, const void* level3, const int64_t* slots,
                                   const float* coords, void* corr, int32_t capacity, int32_t edges, int32_t h, int32_t w, int32_t radius,
                                   int32_t num_levels, void* stream) {
  const char* what = "corr_index_pyramid_forward";
  if (!slots || !coords || !corr) return set_error(SGR_ERR_INVALID, "%s: null argument", what);
  if (num_levels < 1 || num_levels > kMaxPyramidLevels)
    return set_error(SGR_ERR_INVALID, "%s: num_levels (%d) must lie in [1, %d]", what, num_levels, kMaxPyramidLevels);
  if (capacity < 1 || edges < 1 || h < 1 || w < 1 || radius < 0)
    return set_error(SGR_ERR_INVALID, "%s: bad sizes (capacity=%d edges=%d h=%d w=%d radius=%d)", what, capacity, edges, h, w, radius);
  if (radius > kMaxRegRadius) return set_error(SGR_ERR_CAPACITY, "%s: radius %d exceeds the supported %d", what, radius, kMaxRegRadius);
  if (!fits_i32((int64_t)edges * h * w)) return set_error(SGR_ERR_CAPACITY, "%s: edges*h*w must fit in int32", what);
  SlotLevels lv = {{(const _Float16*)level0, (const _Float16*)level1, (const _Float16*)level2, (const _Float16*)level3}};
  for (int l = 0; l < kMaxPyramidLevels; ++l) {
    if (l >= num_levels) lv.v[l] = nullptr;
    else if (!lv.v[l] && (h >> l) > 0 && (w >> l) > 0) return set_error(SGR_ERR_INVALID, "%s: level %d is null", what, l);
  }
  const int HW = h * w, P = edges * HW;
  const dim3 grid((P + kThreads - 1) / kThreads, num_levels), block(kThreads);
  _Float16* o = (_Float16*)corr;
  hipStream_t st = (hipStream_t)stream;
  switch (radius) {
    case 0: hipLaunchKernelGGL((corr_index_pyramid_fwd_kernel<0>), grid, block, 0, st, lv, slots, coords, o, P, HW, h, w, capacity, num_levels); break;
    case 1: hipLaunchKernelGGL((corr_index_pyramid_fwd_kernel<1>), grid, block, 0, st, lv, slots, coords, o, P, HW, h, w, capacity, num_levels); break;
    case 2: hipLaunchKernelGGL((corr_index_pyramid_fwd_kernel<2>), grid, block, 0, st, lv, slots, coords, o, P, HW, h, w, capacity, num_levels); break;
    case 3: hipLaunchKernelGGL((corr_index_pyramid_fwd_kernel<3>), grid, block, 0, st, lv, slots, coords, o, P, HW, h, w, capacity, num_levels); break;
    default: hipLaunchKernelGGL((corr_index_pyramid_fwd_kernel<4>), grid, block, 0, st, lv, slots, coords, o, P, HW, h, w, capacity, num_levels); break;
  }
  static_assert(kMaxRegRadius == 4, "one case per register radius");
  return hipGetLastError() == hipSuccess ? SGR_OK : set_error(SGR_ERR_HIP, "%s launch failed", what);
}

int sgr_corr_alt_backward(const float* fmap1, const float* fmap2, const float* coords, const float* corr_grad, float* fmap1_grad,
                          float* fmap2_grad, int32_t batch, int32_t num, int32_t h1, int32_t w1, int32_t h2, int32_t w2, int32_t channels,
                          int32_t radius, void* stream) {
  if (!fmap1 || !fmap2 || !coords || !corr_grad || !fmap1_grad || !fmap2_grad)
    return set_error(SGR_ERR_INVALID, "corr_alt_backward: null argument");
  if (int rc = alt_sizes("corr_alt_backward", batch, num, h1, w1, h2, w2, channels, radius)) return rc;
  const int BHW = batch * h1 * w1;
  hipLaunchKernelGGL(altcorr_bwd_kernel, dim3((BHW + kWaves - 1) / kWaves), dim3(kThreads), 0, (hipStream_t)stream, fmap1, fmap2, coords,
                     corr_grad, fmap1_grad, fmap2_grad, BHW, num, h1 * w1, h2, w2, channels, radius);
  return hipGetLastError() == hipSuccess ? SGR_OK : set_error(SGR_ERR_HIP, "corr_alt_backward launch failed");
}

}  // extern "C"
