// SSIM (forward + backward) and the rendering metrics of the evaluation (include/splat_hip.h):
//   sgr_ssim, sgr_ssim_backward  loss_utils.ssim                /root/reference/thirdparty/gaussian_splatting/utils/loss_utils.py:36-101
//   sgr_render_metrics           per-frame PSNR / SSIM / depth L1 /root/reference/src/utils/eval_utils.py:90-128
// One workgroup owns a 32x16 output tile of one (image, channel).  The tile and a halo of 5 go to LDS, the 11-tap Gaussian runs
// as a horizontal pass into LDS and a vertical pass per pixel (the 2-D window is the outer product of the 1-D one).  Every sum is a
// per-workgroup partial followed by one fixed-order pass per image: no float atomics, bitwise reproducible.
#include <cmath>

#include <cstdint>

#include "sgr_common.h"

namespace sgr {
int set_error(int code, const char* fmt, ...);

namespace {

constexpr int kSsimR = 5;                       // window 11 = 2 * 5 + 1, zero padding of 5 (loss_utils.py:83)
constexpr int kSsimTW = 32, kSsimTH = 16;       // output tile
constexpr int kSsimIW = kSsimTW + 2 * kSsimR;   // 42: tile + halo
constexpr int kSsimIH = kSsimTH + 2 * kSsimR;   // 26
constexpr int kSsimThreads = 256;
constexpr float kC1 = 0.01f * 0.01f, kC2 = 0.03f * 0.03f;
// gaussian(11, 1.5) of loss_utils.py:36-43 as the reference computes it in fp32 (exp in double, normalised in fp32)
__device__ constexpr float kGauss[11] = {1.028380124e-03f, 7.598758209e-03f, 3.600077331e-02f, 1.093606874e-01f, 2.130055279e-01f,
                                         2.660117149e-01f, 2.130055279e-01f, 1.093606874e-01f, 3.600077331e-02f, 7.598758209e-03f,
                                         1.028380124e-03f};

// ---- the tile code shared by every kernel of this file

// in[NI][kSsimIH][kSsimIW] <- load(offset, v[NI]) over the tile and its halo; zero outside the image
template <int NI, class Load>
__device__ __forceinline__ void tile_load(float* in, int ty0, int tx0, int H, int W, Load load) {
  for (int i = threadIdx.x; i < kSsimIH * kSsimIW; i += kSsimThreads) {
    const int r = i / kSsimIW, c = i - r * kSsimIW;
    const int gy = ty0 - kSsimR + r, gx = tx0 - kSsimR + c;
    float v[NI];
    if (gy >= 0 && gy < H && gx >= 0 && gx < W) {
      load(gy * W + gx, v);
    } else {
#pragma unroll
      for (int n = 0; n < NI; ++n) v[n] = 0.f;
    }
#pragma unroll
    for (int n = 0; n < NI; ++n) in[n * kSsimIH * kSsimIW + i] = v[n];
  }
}

// hor[NM][kSsimIH][kSsimTW] <- horizontal 11-tap pass over prod(in[.][r][c + k]) (NM moments of NI inputs)
template <int NI, int NM, class Prod>
__device__ __forceinline__ void tile_hblur(const float* in, float* hor, Prod prod) {
  for (int j = threadIdx.x; j < kSsimIH * kSsimTW; j += kSsimThreads) {
    const int r = j / kSsimTW, c = j % kSsimTW;
    float acc[NM];
#pragma unroll
    for (int m = 0; m < NM; ++m) acc[m] = 0.f;
#pragma unroll
    for (int k = 0; k < 11; ++k) {
      float v[NI], p[NM];
#pragma unroll
      for (int n = 0; n < NI; ++n) v[n] = in[n * kSsimIH * kSsimIW + r * kSsimIW + c + k];
      prod(v, p);
#pragma unroll
      for (int m = 0; m < NM; ++m) acc[m] += kGauss[k] * p[m];
    }
#pragma unroll
    for (int m = 0; m < NM; ++m) hor[m * kSsimIH * kSsimTW + j] = acc[m];
  }
}

// vertical 11-tap pass at output pixel (ty, tx) of the tile
template <int NM>
__device__ __forceinline__ void tile_vblur(const float* hor, int ty, int tx, float* out) {
#pragma unroll
  for (int m = 0; m < NM; ++m) out[m] = 0.f;
#pragma unroll
  for (int k = 0; k < 11; ++k) {
#pragma unroll
    for (int m = 0; m < NM; ++m) out[m] += kGauss[k] * hor[m * kSsimIH * kSsimTW + (ty + k) * kSsimTW + tx];
  }
}

struct Moments5 {   // (x, y) -> (x, y, x^2, y^2, xy)
  __device__ __forceinline__ void operator()(const float* v, float* p) const {
    p[0] = v[0]; p[1] = v[1]; p[2] = v[0] * v[0]; p[3] = v[1] * v[1]; p[4] = v[0] * v[1];
  }
};
struct Identity3 {
  __device__ __forceinline__ void operator()(const float* v, float* p) const { p[0] = v[0]; p[1] = v[1]; p[2] = v[2]; }
};

// SSIM of one pixel from its five moments (loss_utils.py:84-101); with `dmap`, the three per-pixel derivatives of the map's mean
// (scale = 1 / (C H W)): dS/dmu1 through the sigmas, dS/dE[x^2], dS/dE[xy].  With A1 = 2 mu1 mu2 + C1, A2 = 2 s12 + C2,
// B1 = mu1^2 + mu2^2 + C1, B2 = s11 + s22 + C2 and S = A1 A2 / (B1 B2):
//   dm  = 2 mu2 (A2 - A1) / (B1 B2) - 2 mu1 S (1/B1 - 1/B2),   d11 = -S / B2,   d12 = 2 A1 / (B1 B2).
// The B's are formed as A + (B - A), with B1 - A1 = (mu1 - mu2)^2 and B2 - A2 = E[(x-y)^2] - (mu1 - mu2)^2, and dm is regrouped
// around the factors (mu1 - mu2), (1 - S) and (B2 - A2) - (B1 - A1): every one of them is an exact zero when x == y, so x == y
// gives S = 1, dm = 0 and d12 = -2 d11 bit for bit whichever products the compiler fuses into FMAs (-ffp-contract=fast).
__device__ __forceinline__ float ssim_pixel(const float* m, float scale, float* dmap /* [3] or nullptr */) {
  const float mu1 = m[0], mu2 = m[1], dmu = mu1 - mu2;
  const float mu12 = mu1 * mu2;
  const float A1 = 2.f * mu12 + kC1, A2 = 2.f * (m[4] - mu12) + kC2;
  const float D1 = dmu * dmu;                                   // B1 - A1
  const float D2 = ((m[2] + m[3]) - 2.f * m[4]) - D1;           // B2 - A2
  const float B1 = A1 + D1, B2 = A2 + D2;
  const float r1 = A1 / B1, S = r1 * (A2 / B2);
  if (dmap) {
    // mu2 (A2 - A1) - mu1 S (B2 - B1) = mu2 (A2 - A1)(1 - S) - mu2 S (D2 - D1) - (mu1 - mu2) S (B2 - B1)
    const float t = (mu2 * (A2 - A1) * (1.f - S) - mu2 * S * (D2 - D1)) - dmu * S * (B2 - B1);
    dmap[0] = scale * (2.f * t / (B1 * B2));
    dmap[1] = scale * (-S / B2);
    dmap[2] = scale * (2.f * r1 / B2);
  }
  return S;
}

// dL/dx at one pixel from the blurred maps g = (G*dm, G*d11, G*d12): g0 + 2 x g1 + y g2, grouped as g0 + y (g2 + 2 g1) + 2 g1 (x - y)
// so that x == y (g0 = 0, g2 = -2 g1 exactly) gives an exact zero under any FMA fusion
__device__ __forceinline__ float ssim_grad_pixel(const float* g, float x, float y, float u) {
  return u * (g[0] + (y * (g[2] + 2.f * g[1]) + 2.f * g[1] * (x - y)));
}

// block sum of NP floats in a fixed order (DPP wave sums, then the four waves in order); thread 0 writes out[0..NP)
template <int NP>
__device__ __forceinline__ void block_partial(float (&v)[NP], float* red /* LDS [4 * NP] */, float* out) {
#pragma unroll
  for (int k = 0; k < NP; ++k) v[k] = wave_sum(v[k]);
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < NP; ++k) red[wv * NP + k] = v[k];
  }
  __syncthreads();
  if (threadIdx.x < NP) {
    const int k = threadIdx.x;
    out[k] = ((red[k] + red[NP + k]) + red[2 * NP + k]) + red[3 * NP + k];
  }
}

// fixed-order block sum in double over 256 threads (LDS tree); the total is valid in thread 0
__device__ __forceinline__ double block_sum_f64(double v, double* red /* LDS [256] */) {
  red[threadIdx.x] = v;
  __syncthreads();
  for (int s = kSsimThreads / 2; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
    __syncthreads();
  }
  const double t = red[0];
  __syncthreads();
  return t;
}

int ssim_tiles(int H, int W) { return ((W + kSsimTW - 1) / kSsimTW) * ((H + kSsimTH - 1) / kSsimTH); }

constexpr int kMetricFrames = 16;
constexpr int kMetricParts = 5;                 // ssim sum, squared error, its count, depth L1, its count

}  // namespace

// ---- SSIM forward: grid (tiles, C, B); parts[(b C + c) tiles + tile] = sum of the tile's SSIM map
__global__ void __launch_bounds__(kSsimThreads) ssim_fwd_kernel(int C, int H, int W, const float* __restrict__ img1,
                                                                const float* __restrict__ img2, float* __restrict__ maps,
                                                                float* __restrict__ parts) {
  __shared__ float in[2 * kSsimIH * kSsimIW];
  __shared__ float hor[5 * kSsimIH * kSsimTW];
  __shared__ float red[4];
  const int tiles_x = (W + kSsimTW - 1) / kSsimTW;
  const int tx0 = (blockIdx.x % tiles_x) * kSsimTW, ty0 = (blockIdx.x / tiles_x) * kSsimTH;
  const size_t HW = (size_t)H * W;
  const size_t plane = ((size_t)blockIdx.z * C + blockIdx.y) * HW;
  const float* x = img1 + plane;
  const float* y = img2 + plane;
  tile_load<2>(in, ty0, tx0, H, W, [&](int o, float* v) { v[0] = x[o]; v[1] = y[o]; });
  __syncthreads();
  tile_hblur<2, 5>(in, hor, Moments5());
  __syncthreads();
  const size_t N = (size_t)gridDim.z * C * HW;
  const float scale = 1.f / (float)((size_t)C * HW);
  float acc[1] = {0.f};
  for (int p = threadIdx.x; p < kSsimTH * kSsimTW; p += kSsimThreads) {
    const int ty = p / kSsimTW, tx = p % kSsimTW, gy = ty0 + ty, gx = tx0 + tx;
    if (gy >= H || gx >= W) continue;
    float m[5], d[3];
    tile_vblur<5>(hor, ty, tx, m);
    acc[0] += ssim_pixel(m, scale, maps ? d : nullptr);
    if (maps) {
      const size_t o = plane + (size_t)gy * W + gx;
      maps[o] = d[0];
      maps[N + o] = d[1];
      maps[2 * N + o] = d[2];
    }
  }
  block_partial<1>(acc, red, parts + ((size_t)blockIdx.z * C + blockIdx.y) * gridDim.x + blockIdx.x);
}

// one block per image: the C * tiles partials in a fixed order -> mean SSIM of the image
__global__ void __launch_bounds__(kSsimThreads) ssim_final_kernel(int nparts, float inv_n, const float* __restrict__ parts,
                                                                  float* __restrict__ out) {
  __shared__ double red[kSsimThreads];
  const float* p = parts + (size_t)blockIdx.x * nparts;
  double t = 0.0;
  for (int i = threadIdx.x; i < nparts; i += kSsimThreads) t += (double)p[i];
  t = block_sum_f64(t, red);
  if (threadIdx.x == 0) out[blockIdx.x] = (float)(t * (double)inv_n);
}

// ---- SSIM backward: dL/dx = u_b (G*dm + 2 x (G*d11) + y (G*d12)); the window is symmetric and the padding zero, so the blur is
// its own adjoint
__global__ void __launch_bounds__(kSsimThreads) ssim_bwd_kernel(int C, int H, int W, const float* __restrict__ img1,
                                                                const float* __restrict__ img2, const float* __restrict__ maps,
                                                                const float* __restrict__ upstream, int upstream_stride,
                                                                float upstream_scale, float* __restrict__ dx) {
  __shared__ float in[3 * kSsimIH * kSsimIW];
  __shared__ float hor[3 * kSsimIH * kSsimTW];
  const int tiles_x = (W + kSsimTW - 1) / kSsimTW;
  const int tx0 = (blockIdx.x % tiles_x) * kSsimTW, ty0 = (blockIdx.x / tiles_x) * kSsimTH;
  const size_t HW = (size_t)H * W;
  const size_t plane = ((size_t)blockIdx.z * C + blockIdx.y) * HW;
  const size_t N = (size_t)gridDim.z * C * HW;
  const float* dm = maps + plane;
  tile_load<3>(in, ty0, tx0, H, W, [&](int o, float* v) { v[0] = dm[o]; v[1] = dm[N + o]; v[2] = dm[2 * N + o]; });
  __syncthreads();
  tile_hblur<3, 3>(in, hor, Identity3());
  __syncthreads();
  const float u = upstream[(size_t)blockIdx.z * upstream_stride] * upstream_scale;
  for (int p = threadIdx.x; p < kSsimTH * kSsimTW; p += kSsimThreads) {
    const int ty = p / kSsimTW, tx = p % kSsimTW, gy = ty0 + ty, gx = tx0 + tx;
    if (gy >= H || gx >= W) continue;
    float g[3];
    tile_vblur<3>(hor, ty, tx, g);
    const size_t o = plane + (size_t)gy * W + gx;
    dx[o] = ssim_grad_pixel(g, img1[o], img2[o], u);
  }
}

// ---- rendering metrics (eval_utils.py:90-128) of up to kMetricFrames frames per launch: grid (tiles, C, frames)
struct MetricTab { SgrMetricFrame f[kMetricFrames]; };

__global__ void __launch_bounds__(kSsimThreads) metrics_kernel(MetricTab tab, int C, int H, int W, float global_scale,
                                                               float* __restrict__ parts) {
  __shared__ float in[2 * kSsimIH * kSsimIW];
  __shared__ float hor[5 * kSsimIH * kSsimTW];
  __shared__ float red[4 * kMetricParts];
  const SgrMetricFrame& f = tab.f[blockIdx.z];
  const int tiles_x = (W + kSsimTW - 1) / kSsimTW;
  const int tx0 = (blockIdx.x % tiles_x) * kSsimTW, ty0 = (blockIdx.x / tiles_x) * kSsimTH;
  const size_t HW = (size_t)H * W;
  const float* r = f.render + blockIdx.y * HW;
  const float* gt = f.gt_image + blockIdx.y * HW;
  // image = clamp(exp(a) r + b, 0, 1) (:96-100), built while loading; no exposure = the first frame's identity
  const float ea = f.exposure_a ? expf(f.exposure_a[0]) : 1.f;
  const float eb = f.exposure_b ? f.exposure_b[0] : 0.f;
  tile_load<2>(in, ty0, tx0, H, W, [&](int o, float* v) { v[0] = fminf(fmaxf(ea * r[o] + eb, 0.f), 1.f); v[1] = gt[o]; });
  __syncthreads();
  tile_hblur<2, 5>(in, hor, Moments5());
  __syncthreads();
  const bool with_depth = blockIdx.y == 0 && f.depth && f.gt_depth;
  float acc[kMetricParts] = {0.f, 0.f, 0.f, 0.f, 0.f};
  for (int p = threadIdx.x; p < kSsimTH * kSsimTW; p += kSsimThreads) {
    const int ty = p / kSsimTW, tx = p % kSsimTW, gy = ty0 + ty, gx = tx0 + tx;
    if (gy >= H || gx >= W) continue;
    float m[5];
    tile_vblur<5>(hor, ty, tx, m);
    acc[0] += ssim_pixel(m, 0.f, nullptr);
    const int c = (ty + kSsimR) * kSsimIW + tx + kSsimR;
    const float img = in[c], g = in[kSsimIH * kSsimIW + c];
    if (g > 0.f) {                                          // mask = gt > 0 (:109), PSNR over the masked elements (:123)
      const float e = img - g;
      acc[1] += e * e;
      acc[2] += 1.f;
    }
    if (with_depth) {                                       // |s d - gd| where d > 0 and gd > 0 (:116-120)
      const int o = gy * W + gx;
      const float d = f.depth[o], gd = f.gt_depth[o];
      if (d > 0.f && gd > 0.f) {
        acc[3] += fabsf(global_scale * d - gd);
        acc[4] += 1.f;
      }
    }
  }
  block_partial<kMetricParts>(acc, red, parts + (((size_t)blockIdx.z * C + blockIdx.y) * gridDim.x + blockIdx.x) * kMetricParts);
}

// one block per frame: out[3 f + 0..2] = PSNR, SSIM, depth L1 (0/0 -> NaN as in the reference; a perfect frame -> PSNR inf)
__global__ void __launch_bounds__(kSsimThreads) metrics_final_kernel(int nparts, double inv_n, const float* __restrict__ parts,
                                                                     float* __restrict__ out) {
  __shared__ double red[kSsimThreads];
  const float* p = parts + (size_t)blockIdx.x * nparts * kMetricParts;
  double t[kMetricParts] = {0.0, 0.0, 0.0, 0.0, 0.0};
  for (int i = threadIdx.x; i < nparts; i += kSsimThreads) {
#pragma unroll
    for (int k = 0; k < kMetricParts; ++k) t[k] += (double)p[(size_t)i * kMetricParts + k];
  }
#pragma unroll
  for (int k = 0; k < kMetricParts; ++k) t[k] = block_sum_f64(t[k], red);
  if (threadIdx.x == 0) {
    const double mse = t[1] / t[2];
    out[3 * blockIdx.x + 0] = (float)(20.0 * log10(1.0 / sqrt(mse)));
    out[3 * blockIdx.x + 1] = (float)(t[0] * inv_n);
    out[3 * blockIdx.x + 2] = (float)(t[3] / t[4]);
  }
}

// ---- the mapping loss with the SSIM term (slam_utils.py:89-105, ssim_loss: True) of a group of views: grid (tiles, 3, views)
//   L = alpha mean_{c,p} [(1 - lam) |m r| + lam (1 - ssim(x, gt))] + (1 - alpha) mean_p |md (d - gd)|,   x = exp(a) I + b
// Pass A writes the three derivative maps of the SSIM mean and LossPart.rgb of its (tile, channel); pass B blurs the maps, forms
// dL/dx, and writes dL/dimage, dL/ddepth and LossPart.{dep, da, db}.  parts[v][c tiles + tile] is one LossPart: launch_mapping_loss_final
// (or the fused Adam tail) adds them up exactly as it does for the L1 epilogue's per-8x8-tile records.
namespace {
__device__ __forceinline__ float exposed(float ea, float I, float eb) { return __builtin_fmaf(ea, I, eb); }   // same bits in A and B
__device__ __forceinline__ bool rgb_mask(const float* gt, size_t HW, int o, float thr) { return (gt[o] + gt[HW + o]) + gt[2 * HW + o] > thr; }
__device__ __forceinline__ float sign_of(float r) { return r > 0.f ? 1.f : (r < 0.f ? -1.f : 0.f); }
}  // namespace

__global__ void __launch_bounds__(kSsimThreads) ssimloss_moments_kernel(LossTab lt, int v0, int H, int W, float lam, float thr,
                                                                        float scale, float* __restrict__ maps, size_t map_stride) {
  __shared__ float in[2 * kSsimIH * kSsimIW];
  __shared__ float hor[5 * kSsimIH * kSsimTW];
  __shared__ float red[4];
  const int vw = v0 + blockIdx.z, c = blockIdx.y;
  const int tiles_x = (W + kSsimTW - 1) / kSsimTW;
  const int tx0 = (blockIdx.x % tiles_x) * kSsimTW, ty0 = (blockIdx.x / tiles_x) * kSsimTH;
  const size_t HW = (size_t)H * W;
  const float* I = lt.image[vw] + c * HW;
  const float* gt = lt.gt_image[vw];
  const float* y = gt + c * HW;
  const float ea = lt.exp_a[vw] ? __expf(lt.exp_a[vw][0]) : 1.f;
  const float eb = lt.exp_b[vw] ? lt.exp_b[vw][0] : 0.f;
  tile_load<2>(in, ty0, tx0, H, W, [&](int o, float* v) { v[0] = exposed(ea, I[o], eb); v[1] = y[o]; });
  __syncthreads();
  tile_hblur<2, 5>(in, hor, Moments5());
  __syncthreads();
  float* mp = maps + (size_t)blockIdx.z * map_stride + c * HW;     // [3 maps][3 channels][H W] per view
  float acc[1] = {0.f};
  for (int p = threadIdx.x; p < kSsimTH * kSsimTW; p += kSsimThreads) {
    const int ty = p / kSsimTW, tx = p % kSsimTW, gy = ty0 + ty, gx = tx0 + tx;
    if (gy >= H || gx >= W) continue;
    float m[5], d[3];
    tile_vblur<5>(hor, ty, tx, m);
    const float S = ssim_pixel(m, scale, d);
    const int o = gy * W + gx;
    mp[o] = d[0];
    mp[3 * HW + o] = d[1];
    mp[6 * HW + o] = d[2];
    const int ci = (ty + kSsimR) * kSsimIW + tx + kSsimR;
    const float r = rgb_mask(gt, HW, o, thr) ? in[ci] - in[kSsimIH * kSsimIW + ci] : 0.f;
    acc[0] += (1.f - lam) * fabsf(r) + lam * (1.f - S);
  }
  block_partial<1>(acc, red, (float*)((LossPart*)lt.parts[vw] + (size_t)c * gridDim.x + blockIdx.x));
}

// dL/dx = w_l1 sign(m r) + u (G*dm + 2 x G*d11 + y G*d12), w_l1 = upstream alpha (1 - lam) / (3 H W), u = -upstream alpha lam
__global__ void __launch_bounds__(kSsimThreads) ssimloss_grad_kernel(LossTab lt, int v0, int H, int W, float w_l1, float w_dep,
                                                                     float u, float thr, const float* __restrict__ maps,
                                                                     size_t map_stride) {
  __shared__ float in[3 * kSsimIH * kSsimIW];
  __shared__ float hor[3 * kSsimIH * kSsimTW];
  __shared__ float red[4 * 3];
  const int vw = v0 + blockIdx.z, c = blockIdx.y;
  const int tiles_x = (W + kSsimTW - 1) / kSsimTW;
  const int tx0 = (blockIdx.x % tiles_x) * kSsimTW, ty0 = (blockIdx.x / tiles_x) * kSsimTH;
  const size_t HW = (size_t)H * W;
  const float* mp = maps + (size_t)blockIdx.z * map_stride + c * HW;
  tile_load<3>(in, ty0, tx0, H, W, [&](int o, float* v) { v[0] = mp[o]; v[1] = mp[3 * HW + o]; v[2] = mp[6 * HW + o]; });
  __syncthreads();
  tile_hblur<3, 3>(in, hor, Identity3());
  __syncthreads();
  const float* I = lt.image[vw] + c * HW;
  const float* gt = lt.gt_image[vw];
  float* __restrict__ dimage = lt.dimage[vw];
  float* __restrict__ ddepth = lt.ddepth[vw];
  const float ea = lt.exp_a[vw] ? __expf(lt.exp_a[vw][0]) : 1.f;
  const float eb = lt.exp_b[vw] ? lt.exp_b[vw][0] : 0.f;
  const bool with_depth = c == 0;                 // the depth term rides in the channel-0 workgroups
  float acc[3] = {0.f, 0.f, 0.f};                 // dep, da, db
  for (int p = threadIdx.x; p < kSsimTH * kSsimTW; p += kSsimThreads) {
    const int ty = p / kSsimTW, tx = p % kSsimTW, gy = ty0 + ty, gx = tx0 + tx;
    if (gy >= H || gx >= W) continue;
    float g[3];
    tile_vblur<3>(hor, ty, tx, g);
    const int o = gy * W + gx;
    const float Iv = I[o], x = exposed(ea, Iv, eb), yv = gt[c * HW + o];
    const float r = rgb_mask(gt, HW, o, thr) ? x - yv : 0.f;
    const float dab = w_l1 * sign_of(r) + ssim_grad_pixel(g, x, yv, u);   // dL/d(image_ab)
    if (dimage) dimage[c * HW + o] = dab * ea;
    acc[1] += dab * ea * Iv;
    acc[2] += dab;
    if (with_depth) {
      const float gd = lt.gt_depth[vw][o];
      const float rd = gd > 0.01f ? lt.depth[vw][o] - gd : 0.f;
      acc[0] += fabsf(rd);
      if (ddepth) ddepth[o] = w_dep * sign_of(rd);
    }
  }
  block_partial<3>(acc, red, (float*)((LossPart*)lt.parts[vw] + (size_t)c * gridDim.x + blockIdx.x) + 1);
}

size_t ssim_term_view_maps(int H, int W) { return ((size_t)9 * H * W * sizeof(float) + 255) & ~(size_t)255; }
int ssim_loss_nparts(int H, int W) { return 3 * ssim_tiles(H, W); }

// views v0 .. v0 + nv of `lt` (nv <= the arena's view slots); parts[v] needs ssim_loss_nparts(H, W) LossParts
void launch_ssim_mapping_loss(const LossTab& lt, int v0, int nv, int H, int W, float alpha, float lam, float thr, float upstream,
                              float* maps, hipStream_t st) {
  const int tiles = ssim_tiles(H, W);
  const float inv_rgb = 1.f / (3.f * (float)H * (float)W), inv_dep = 1.f / ((float)H * (float)W);
  const size_t stride = ssim_term_view_maps(H, W) / sizeof(float);
  hipLaunchKernelGGL(ssimloss_moments_kernel, dim3(tiles, 3, nv), dim3(kSsimThreads), 0, st, lt, v0, H, W, lam, thr, inv_rgb, maps,
                     stride);
  hipLaunchKernelGGL(ssimloss_grad_kernel, dim3(tiles, 3, nv), dim3(kSsimThreads), 0, st, lt, v0, H, W,
                     upstream * alpha * (1.f - lam) * inv_rgb, upstream * (1.f - alpha) * inv_dep, -upstream * alpha * lam, thr,
                     (const float*)maps, stride);
}

}  // namespace sgr

using namespace sgr;

extern "C" {

size_t sgr_ssim_scratch_bytes(int32_t B, int32_t C, int32_t H, int32_t W) {
  if (B <= 0 || C <= 0 || H <= 0 || W <= 0) return 0;
  return (size_t)B * C * ssim_tiles(H, W) * kMetricParts * sizeof(float);
}

size_t sgr_ssim_term_bytes(int32_t max_views, int32_t H, int32_t W) {
  if (max_views <= 0 || H <= 0 || W <= 0) return 0;
  const size_t parts = ((size_t)ssim_loss_nparts(H, W) * sizeof(LossPart) + 255) & ~(size_t)255;
  return (size_t)max_views * ssim_term_view_maps(H, W) + parts;
}

int sgr_mapping_loss_ssim(int32_t H, int32_t W, const float* image, const float* depth, const float* gt_image,
                          const float* gt_depth, const float* exposure_a, const float* exposure_b, float alpha,
                          float rgb_boundary_threshold, float upstream, const SgrSsimTerm* term, float* loss,
                          float* dL_dimage, float* dL_ddepth, float* dL_dexp_a, float* dL_dexp_b, void* stream) {
  if (H <= 0 || W <= 0 || H > 65535 * kSsimTH || !image || !depth || !gt_image || !gt_depth || !term)
    return set_error(SGR_ERR_INVALID, "mapping_loss_ssim: null/size");
  if (!term->arena || term->max_views <= 0 || term->arena_bytes < sgr_ssim_term_bytes(term->max_views, H, W))
    return set_error(SGR_ERR_WORKSPACE, "mapping_loss_ssim: SSIM arena too small (need %zu for %d views)",
                     sgr_ssim_term_bytes(term->max_views > 0 ? term->max_views : 1, H, W), term->max_views);
  // arena: max_views map slots, then the partial records of ONE view (the batched entry points keep theirs in loss_scratch)
  float* maps = (float*)term->arena;
  LossTab tab = {};
  tab.image[0] = image; tab.depth[0] = depth; tab.gt_image[0] = gt_image; tab.gt_depth[0] = gt_depth;
  tab.exp_a[0] = exposure_a; tab.exp_b[0] = exposure_b; tab.loss[0] = loss; tab.dimage[0] = dL_dimage;
  tab.ddepth[0] = dL_ddepth; tab.da[0] = dL_dexp_a; tab.db[0] = dL_dexp_b;
  tab.parts[0] = (char*)term->arena + (size_t)term->max_views * ssim_term_view_maps(H, W);
  hipStream_t st = (hipStream_t)stream;
  launch_ssim_mapping_loss(tab, 0, 1, H, W, alpha, term->lambda_dssim, rgb_boundary_threshold, upstream, maps, st);
  launch_mapping_loss_final(tab, 1, H * W, ssim_loss_nparts(H, W), alpha, st);
  return hipGetLastError() == hipSuccess ? SGR_OK : set_error(SGR_ERR_HIP, "mapping_loss_ssim launch failed");
}

int sgr_ssim(int32_t B, int32_t C, int32_t H, int32_t W, const float* img1, const float* img2, float* ssim_out, float* maps,
             void* scratch, size_t scratch_bytes, void* stream) {
  if (B <= 0 || C <= 0 || H <= 0 || W <= 0 || B > 65535 || C > 65535 || !img1 || !img2 || !ssim_out)
    return set_error(SGR_ERR_INVALID, "ssim: null/size");
  if (!scratch || scratch_bytes < sgr_ssim_scratch_bytes(B, C, H, W))
    return set_error(SGR_ERR_WORKSPACE, "ssim scratch too small (need %zu)", sgr_ssim_scratch_bytes(B, C, H, W));
  const int tiles = ssim_tiles(H, W);
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(ssim_fwd_kernel, dim3(tiles, C, B), dim3(kSsimThreads), 0, st, C, H, W, img1, img2, maps, (float*)scratch);
  hipLaunchKernelGGL(ssim_final_kernel, dim3(B), dim3(kSsimThreads), 0, st, C * tiles, (float)(1.0 / ((double)C * H * W)),
                     (const float*)scratch, ssim_out);
  return hipGetLastError() == hipSuccess ? SGR_OK : set_error(SGR_ERR_HIP, "ssim launch failed");
}

int sgr_ssim_backward(int32_t B, int32_t C, int32_t H, int32_t W, const float* img1, const float* img2, const float* maps,
                      const float* upstream, int32_t upstream_stride, float upstream_scale, float* dL_dimg1, void* stream) {
  if (B <= 0 || C <= 0 || H <= 0 || W <= 0 || B > 65535 || C > 65535 || upstream_stride < 0 || !img1 || !img2 || !maps ||
      !upstream || !dL_dimg1)
    return set_error(SGR_ERR_INVALID, "ssim_backward: null/size");
  hipLaunchKernelGGL(ssim_bwd_kernel, dim3(ssim_tiles(H, W), C, B), dim3(kSsimThreads), 0, (hipStream_t)stream, C, H, W, img1, img2,
                     maps, upstream, upstream_stride, upstream_scale, dL_dimg1);
  return hipGetLastError() == hipSuccess ? SGR_OK : set_error(SGR_ERR_HIP, "ssim_backward launch failed");
}

int sgr_render_metrics(int32_t n, const SgrMetricFrame* frames, int32_t C, int32_t H, int32_t W, float global_scale, float* out,
                       void* scratch, size_t scratch_bytes, void* stream) {
  if (n <= 0 || C <= 0 || H <= 0 || W <= 0 || C > 65535 || !frames || !out) return set_error(SGR_ERR_INVALID, "render_metrics: null/size");
  for (int i = 0; i < n; ++i)
    if (!frames[i].render || !frames[i].gt_image) return set_error(SGR_ERR_INVALID, "render_metrics: frame %d has no image", i);
  if (!scratch || scratch_bytes < sgr_ssim_scratch_bytes(n, C, H, W))
    return set_error(SGR_ERR_WORKSPACE, "render_metrics scratch too small (need %zu)", sgr_ssim_scratch_bytes(n, C, H, W));
  const int tiles = ssim_tiles(H, W);
  hipStream_t st = (hipStream_t)stream;
  float* parts = (float*)scratch;
  for (int f0 = 0; f0 < n; f0 += kMetricFrames) {
    const int k = n - f0 < kMetricFrames ? n - f0 : kMetricFrames;
    MetricTab tab = {};
    for (int i = 0; i < k; ++i) tab.f[i] = frames[f0 + i];
    hipLaunchKernelGGL(metrics_kernel, dim3(tiles, C, k), dim3(kSsimThreads), 0, st, tab, C, H, W, global_scale,
                       parts + (size_t)f0 * C * tiles * kMetricParts);
  }
  hipLaunchKernelGGL(metrics_final_kernel, dim3(n), dim3(kSsimThreads), 0, st, C * tiles, 1.0 / ((double)C * H * W),
                     (const float*)parts, out);
  return hipGetLastError() == hipSuccess ? SGR_OK : set_error(SGR_ERR_HIP, "render_metrics launch failed");
}

}  // extern "C"
