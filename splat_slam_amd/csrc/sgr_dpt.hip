// The decoder of the mono-depth prior (reassemble, layerN_rn, the four fusion blocks and the head of the DPT network; the equations
// are DESIGN.md section 3, "Mono-depth prior") and the two resizes of predict, inference only.  DESIGN.md section 3, "DPT decoder".
//   sgr_dpt_conv         one stride-1 convolution (1x1, 3x3, zero padding) on the shared tile of sgr_conv_mma.h: channels-last fp16 in,
//                        optional ReLU on the gathered input, epilogue relu?(sum + bias) + res0 + res1 in fp32, one rounding, stored
//                        channels-last fp16 (8-byte stores) or fp32; cout 1..1024, the tail of a channel tile masked
//   sgr_dpt_up2          bilinear 2x, align_corners=True, channels-last fp16, positions in integers
//   sgr_dpt_resize_in    fp32 planes -> antialiased bilinear resize, (x - 0.5) / 0.5, fp16 planes, both axes in one launch
//   sgr_dpt_resize_out   fp32 plane -> clamp, bicubic (A = -0.75) resize, clamp, fp32 plane
//   sgr_dpt_forward      the whole decoder: 35 stream-ordered launches, no host synchronisation
// Tiles of the convolution span images (pixel m runs over the whole batch), yet every output sums its k = tap * cin + channel in the
// MFMA's order whatever tile it falls into: no atomics, bitwise reproducible, and image i of a batch gives the bits of that image alone.
#include <cstdint>

#include "sgr_conv_mma.h"

namespace sgr {
namespace {

constexpr int kMaxChannels = 1024;
constexpr int kHeadMid = 32;                // output_conv.2 -> 32 channels, output_conv.4 -> 1

struct ConvArgs {
  SgrDptConv c;
  int HW, M, k_pad;                         // M = n * h * w
};

template <int KS, int BN>
__global__ void __launch_bounds__(kThreads) dpt_conv_kernel(const ConvArgs a) {
  constexpr int NT = BN / 16, P = (KS - 1) / 2;
  __shared__ __attribute__((aligned(16))) half_t Xs[kBM * kRow];
  __shared__ __attribute__((aligned(16))) half_t Ws[BN * kRow];
  const SgrDptConv& c = a.c;
  const int tid = threadIdx.x, m0 = blockIdx.x * kBM, n0 = blockIdx.y * BN;
  const half_t* src = (const half_t*)c.src;

  // This kernel keeps its own gather, not ConvWindow's: it addresses a tap as (first pixel of the image + y w + x) * stride, one
  // 64-bit product, where the shared one adds the image to the product; the compiler's code for the two differs.
  int py[2], px[2];
  int64_t base[2];                                           // first pixel of the row's image
  bool pv[2];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int m = m0 + (tid >> 2) + 64 * i;
    pv[i] = m < a.M;
    const int mm = pv[i] ? m : 0, img = mm / a.HW, p = mm - img * a.HW;
    py[i] = p / c.w;
    px[i] = p - py[i] * c.w;
    base[i] = (int64_t)img * a.HW;
  }
  const bool relu_in = c.relu_in != 0;
  auto gather = [&](int i, bool tv, int ty, int tx, int ch) {
    const int yy = py[i] + ty - P, xx = px[i] + tx - P;
    half8 v = {0, 0, 0, 0, 0, 0, 0, 0};
    if (pv[i] && tv && (unsigned)yy < (unsigned)c.h && (unsigned)xx < (unsigned)c.w)
      v = *(const half8*)(src + (base[i] + (int64_t)yy * c.w + xx) * c.src_stride + ch);
    return v;
  };
  // the ReLU in front of an RCU's conv1, four packed maxima per chunk on its way to LDS (the padding's zeros stay zeros)
  auto pre = [&](half8 v) { return relu_in ? __builtin_elementwise_max(v, half8{0, 0, 0, 0, 0, 0, 0, 0}) : v; };
  floatx4 acc[NT][2];
  conv_mma_mainloop<KS, BN>(Xs, Ws, (const half_t*)c.weight, n0, a.k_pad, c.cin, gather, pre, acc);

  // acc[t][j] holds channels acc_channel(n0, t) .. + 3 of pixel acc_pixel(j) of the batch
  const half_t* res0 = (const half_t*)c.res0;
  const half_t* res1 = (const half_t*)c.res1;
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int64_t m = acc_pixel(j);
    if (m >= a.M) continue;
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      const int nb = acc_channel(n0, t);
      if (nb >= c.cout) continue;
      const bool full = nb + 4 <= c.cout;
      floatx4 v = acc[t][j];
      if (c.bias) v += *(const floatx4*)&c.bias[nb];           // padded to whole tiles of 64
      if (c.relu)
#pragma unroll
        for (int r = 0; r < 4; ++r) v[r] = fmaxf(v[r], 0.f);
      if (res0) {
        if (full) {
          const half4 x = *(const half4*)&res0[m * c.res0_stride + nb];
#pragma unroll
          for (int r = 0; r < 4; ++r) v[r] += (float)x[r];
        } else {
          for (int r = 0; nb + r < c.cout; ++r) v[r] += (float)res0[m * c.res0_stride + nb + r];
        }
      }
      if (res1) {
        if (full) {
          const half4 x = *(const half4*)&res1[m * c.res1_stride + nb];
#pragma unroll
          for (int r = 0; r < 4; ++r) v[r] += (float)x[r];
        } else {
          for (int r = 0; nb + r < c.cout; ++r) v[r] += (float)res1[m * c.res1_stride + nb + r];
        }
      }
      if (c.out_kind == SGR_UPDATE_OUT_CL_F16) {
        half_t* o = (half_t*)c.out + m * c.out_stride + nb;
        if (full) {
          half4 h;
#pragma unroll
          for (int r = 0; r < 4; ++r) h[r] = (half_t)v[r];
          *(half4*)o = h;
        } else {
          for (int r = 0; nb + r < c.cout; ++r) o[r] = (half_t)v[r];
        }
      } else {
        float* o = (float*)c.out + m * c.out_stride + nb;
        for (int r = 0; r < 4 && nb + r < c.cout; ++r) o[r] = v[r];
      }
    }
  }
}

struct Up2Args {
  const half_t* src;
  half_t* dst;
  int h, w, chunks, src_stride, dst_stride;
  int64_t total;                             // n * 2h * 2w * chunks
};

// One thread per (output pixel, 8 channels).  Source row of output row o: o (h - 1) / (2h - 1) = i0 + r / den in integers; the four
// weights are (den_y - ry | ry) (den_x - rx | rx) / (den_y den_x), one fp32 division each.
__global__ void __launch_bounds__(kThreads) dpt_up2_kernel(const Up2Args a) {
  const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i >= a.total) return;
  const int j = (int)(i % a.chunks);
  const int64_t q = i / a.chunks;
  const int wo = 2 * a.w, ho = 2 * a.h;
  const int ox = (int)(q % wo), oy = (int)((q / wo) % ho);
  const int64_t img = q / ((int64_t)wo * ho);
  const int deny = 2 * a.h - 1, denx = 2 * a.w - 1;
  const int64_t numy = (int64_t)oy * (a.h - 1), numx = (int64_t)ox * (a.w - 1);
  const int y0 = (int)(numy / deny), x0 = (int)(numx / denx);
  const int ry = (int)(numy - (int64_t)y0 * deny), rx = (int)(numx - (int64_t)x0 * denx);
  const int y1 = min(y0 + 1, a.h - 1), x1 = min(x0 + 1, a.w - 1);
  const float dd = (float)((int64_t)deny * denx);
  const float w00 = (float)((int64_t)(deny - ry) * (denx - rx)) / dd, w01 = (float)((int64_t)(deny - ry) * rx) / dd;
  const float w10 = (float)((int64_t)ry * (denx - rx)) / dd, w11 = (float)((int64_t)ry * rx) / dd;
  const half_t* s = a.src + img * a.h * a.w * a.src_stride + j * 8;
  const half8 v00 = *(const half8*)&s[((int64_t)y0 * a.w + x0) * a.src_stride], v01 = *(const half8*)&s[((int64_t)y0 * a.w + x1) * a.src_stride];
  const half8 v10 = *(const half8*)&s[((int64_t)y1 * a.w + x0) * a.src_stride], v11 = *(const half8*)&s[((int64_t)y1 * a.w + x1) * a.src_stride];
  half8 o;
#pragma unroll
  for (int k = 0; k < 8; ++k)
    o[k] = (half_t)fmaf(w11, (float)v11[k], fmaf(w10, (float)v10[k], fmaf(w01, (float)v01[k], w00 * (float)v00[k])));
  *(half8*)&a.dst[q * a.dst_stride + j * 8] = o;
}

struct ResizeArgs {
  const float* src;
  void* dst;
  int H, W, h, w;                            // source H x W, destination h x w
  int64_t total;                             // planes * h * w
};

// The taps of output o on an axis of `in` samples resized to `out` with the antialiased triangle filter: with S = max(in, out) the
// support is S / out around the centre (2o + 1) in / (2 out), tap x has the weight max(0, 2S - |(2x + 1) out - (2o + 1) in|) / 2S,
// and the weights are divided by their sum: all integers up to that division.
struct Taps {
  int lo, hi;                                // taps lo .. hi - 1
  int64_t c, S2, sum;                        // (2o + 1) in, 2S, the sum of the integer weights
};
__device__ __forceinline__ int64_t tri_weight(const Taps& t, int x, int out) {
  int64_t d = (int64_t)(2 * x + 1) * out - t.c;
  d = d < 0 ? -d : d;
  return d < t.S2 ? t.S2 - d : 0;
}
__device__ __forceinline__ Taps aa_taps(int o, int in, int out) {
  Taps t;
  const int64_t S = in > out ? in : out;
  t.c = (int64_t)(2 * o + 1) * in;
  t.S2 = 2 * S;
  const int64_t lo = t.c - 2 * S + out, hi = t.c + 2 * S + out;       // (centre -+ support + 0.5) * 2 out
  t.lo = lo <= 0 ? 0 : (int)(lo / (2 * out));
  t.hi = hi / (2 * out) < in ? (int)(hi / (2 * out)) : in;
  t.sum = 0;
  for (int x = t.lo; x < t.hi; ++x) t.sum += tri_weight(t, x, out);
  return t;
}

// One thread per output element of a plane; rows are summed first, in ascending x, then the rows in ascending y, all in fp32.
__global__ void __launch_bounds__(kThreads) dpt_resize_in_kernel(const ResizeArgs a) {
  const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i >= a.total) return;
  const int ox = (int)(i % a.w), oy = (int)((i / a.w) % a.h);
  const int64_t plane = i / ((int64_t)a.w * a.h);
  const Taps ty = aa_taps(oy, a.H, a.h), tx = aa_taps(ox, a.W, a.w);
  const float* s = a.src + plane * a.H * a.W;
  const float sy = (float)ty.sum, sx = (float)tx.sum;
  float v = 0.f;
  for (int y = ty.lo; y < ty.hi; ++y) {
    float row = 0.f;
    for (int x = tx.lo; x < tx.hi; ++x) row = fmaf((float)tri_weight(tx, x, a.w) / sx, s[(int64_t)y * a.W + x], row);
    v = fmaf((float)tri_weight(ty, y, a.h) / sy, row, v);
  }
  ((half_t*)a.dst)[i] = (half_t)((v - 0.5f) / 0.5f);
}

// The four cubic-convolution weights (A = -0.75) of the fraction t, evaluated in fp64 and rounded once
__device__ __forceinline__ void cubic_weights(double t, float (&w)[4]) {
  const double A = -0.75;
  auto inner = [&](double x) { return ((A + 2.0) * x - (A + 3.0)) * x * x + 1.0; };
  auto outer = [&](double x) { return ((A * x - 5.0 * A) * x + 8.0 * A) * x - 4.0 * A; };
  w[0] = (float)outer(t + 1.0), w[1] = (float)inner(t), w[2] = (float)inner(1.0 - t), w[3] = (float)outer(2.0 - t);
}

// One thread per output pixel.  Source position of output o: ((2o + 1) in - out) / (2 out) = i0 + r / (2 out), floor division.
__global__ void __launch_bounds__(kThreads) dpt_resize_out_kernel(const ResizeArgs a) {
  const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i >= a.total) return;
  const int ox = (int)(i % a.w), oy = (int)((i / a.w) % a.h);
  const int64_t plane = i / ((int64_t)a.w * a.h);
  auto pos = [](int o, int in, int out, int& i0, double& t) {
    const int64_t num = (int64_t)(2 * o + 1) * in - out, den = 2 * (int64_t)out;
    int64_t q = num / den;
    if (num - q * den < 0) --q;
    i0 = (int)q;
    t = (double)(num - q * den) / (double)den;
  };
  int y0, x0;
  double fy, fx;
  pos(oy, a.H, a.h, y0, fy);
  pos(ox, a.W, a.w, x0, fx);
  float wy[4], wx[4];
  cubic_weights(fy, wy);
  cubic_weights(fx, wx);
  const float* s = a.src + plane * a.H * a.W;
  float v = 0.f;
#pragma unroll
  for (int dy = 0; dy < 4; ++dy) {
    const int y = min(max(y0 - 1 + dy, 0), a.H - 1);
    float row = 0.f;
#pragma unroll
    for (int dx = 0; dx < 4; ++dx) {
      const int x = min(max(x0 - 1 + dx, 0), a.W - 1);
      row = fmaf(wx[dx], fminf(fmaxf(s[(int64_t)y * a.W + x], 0.f), 1.f), row);
    }
    v = fmaf(wy[dy], row, v);
  }
  ((float*)a.dst)[i] = fminf(fmaxf(v, 0.f), 1.f);
}

int launch_conv(const SgrDptConv& c, hipStream_t stream) {
  if (!c.src || !c.weight || !c.out) return set_error(SGR_ERR_INVALID, "dpt_conv: null argument");
  if (!map_ok(c.n, c.h, c.w) || (int64_t)c.n * c.h * c.w > 0x7fffffff - kBM || c.cin < 8 || c.cin % 8 || c.cin > kMaxChannels)
    return set_error(SGR_ERR_INVALID, "dpt_conv: bad sizes (n=%d h=%d w=%d cin=%d); n * h * w must fit int32, cin a multiple of 8 up to 1024", c.n,
                     c.h, c.w, c.cin);
  if (c.cout < 1 || c.cout > kMaxChannels) return set_error(SGR_ERR_INVALID, "dpt_conv: cout %d outside 1..1024", c.cout);
  if (c.ksize != 1 && c.ksize != 3) return set_error(SGR_ERR_INVALID, "dpt_conv: kernel size %d is not 1 or 3", c.ksize);
  int k_pad;                                                 // (the rows are padded to whole tiles of 64)
  if (int rc = check_conv_operands("dpt_conv", c.src, c.src_stride, c.cin, c.ksize, c.weight, c.weight_elems, round_up(c.cout, 64), c.bias, k_pad))
    return rc;
  if (c.out_kind != SGR_UPDATE_OUT_CL_F16 && c.out_kind != SGR_UPDATE_OUT_CL_F32)
    return set_error(SGR_ERR_INVALID, "dpt_conv: the output is channels-last fp16 or fp32, got kind %d", c.out_kind);
  if (c.out_stride < c.cout || !aligned16(c.out) || (c.out_kind == SGR_UPDATE_OUT_CL_F16 && c.out_stride % 8))
    return set_error(SGR_ERR_INVALID, "dpt_conv: out needs a 16-byte aligned base and a stride (%d) >= cout %d, for fp16 a multiple of 8", c.out_stride,
                     c.cout);
  if ((c.res0 && (c.res0_stride < c.cout || c.res0_stride % 8 || !aligned16(c.res0))) ||
      (c.res1 && (c.res1_stride < c.cout || c.res1_stride % 8 || !aligned16(c.res1))))
    return set_error(SGR_ERR_INVALID, "dpt_conv: a residual needs a 16-byte aligned base and a stride that is a multiple of 8 and >= cout %d", c.cout);
  ConvArgs a;
  a.c = c;
  a.HW = c.h * c.w;
  a.M = c.n * a.HW;
  a.k_pad = k_pad;
  // the channel tile of sgr_resnet_conv: the widest of 64, 32, 16 that divides cout; any other cout takes 16 and masks the tail
  const int bn = c.cout % 64 == 0 ? 64 : c.cout % 32 == 0 ? 32 : 16;
  const dim3 grid((unsigned)tiles_of(a.M), (unsigned)((c.cout + bn - 1) / bn)), block(kThreads);
  if (c.ksize == 1)
    dispatch_conv<16, 32, 64>(1, bn, [&](auto ks, auto bnc) {
      hipLaunchKernelGGL((dpt_conv_kernel<1, decltype(bnc)::value>), grid, block, 0, stream, a);
    });
  else
    dispatch_conv<16, 32, 64>(3, bn, [&](auto ks, auto bnc) {
      hipLaunchKernelGGL((dpt_conv_kernel<3, decltype(bnc)::value>), grid, block, 0, stream, a);
    });
  return launched("dpt_conv");
}

int launch_up2(const half_t* src, int n, int h, int w, int C, int src_stride, half_t* dst, int dst_stride, hipStream_t stream) {
  if (!src || !dst || !aligned16(src) || !aligned16(dst)) return set_error(SGR_ERR_INVALID, "dpt_up2: null or unaligned argument");
  if (!map_ok(n, h, w) || (int64_t)n * h * w * 4 > 0x7fffffff || C < 8 || C % 8 || C > kMaxChannels || src_stride < C || src_stride % 8 ||
      dst_stride < C || dst_stride % 8)
    return set_error(SGR_ERR_INVALID,
                     "dpt_up2: bad sizes (n=%d h=%d w=%d channels=%d strides %d, %d); channels and strides multiples of 8, the output pixels "
                     "must fit int32", n, h, w, C, src_stride, dst_stride);
  Up2Args a;
  a.src = src, a.dst = dst, a.h = h, a.w = w, a.chunks = C / 8, a.src_stride = src_stride, a.dst_stride = dst_stride;
  a.total = (int64_t)n * h * w * 4 * a.chunks;
  const int64_t blocks = (a.total + kThreads - 1) / kThreads;
  if (blocks > 0x7fffffff) return set_error(SGR_ERR_INVALID, "dpt_up2: the map is too large for one launch");
  hipLaunchKernelGGL(dpt_up2_kernel, dim3((unsigned)blocks), dim3(kThreads), 0, stream, a);
  return launched("dpt_up2");
}

template <class Kernel>
int launch_resize(const char* what, Kernel kernel, const float* src, int planes, int H, int W, void* dst, int h, int w, hipStream_t stream) {
  if (!src || !dst) return set_error(SGR_ERR_INVALID, "%s: null argument", what);
  if (planes < 1 || planes > 65535 || H < 1 || W < 1 || h < 1 || w < 1 || H > 32768 || W > 32768 || h > 32768 || w > 32768)
    return set_error(SGR_ERR_INVALID, "%s: bad sizes (planes=%d %d x %d -> %d x %d); sides of 1..32768, at most 65535 planes", what, planes, H, W, h,
                     w);
  ResizeArgs a;
  a.src = src, a.dst = dst, a.H = H, a.W = W, a.h = h, a.w = w, a.total = (int64_t)planes * h * w;
  const int64_t blocks = (a.total + kThreads - 1) / kThreads;
  if (blocks > 0x7fffffff) return set_error(SGR_ERR_INVALID, "%s: the output is too large for one launch", what);
  hipLaunchKernelGGL(kernel, dim3((unsigned)blocks), dim3(kThreads), 0, stream, a);
  return launched(what);
}

bool sizes_ok(int n, int H, int W, int dim, int features) {
  return map_ok(n, H, W) && H % 32 == 0 && W % 32 == 0 && (int64_t)n * H * W <= 0x7fffffff - kBM && dim >= 16 && dim % 16 == 0 &&
         dim <= kMaxChannels && features >= 16 && features % 16 == 0 && features <= kMaxChannels;
}

// The maps of a call, all channels-last fp16: the packed taps and the reassembled maps, the four layerN_rn outputs, four rotating
// buffers of the largest fusion map (1/2 resolution, `features` channels) and the two full-resolution maps of the head.
struct Plan {
  half_t *t3, *r3, *t4, *u4, *r4, *s[4], *work[4], *hu, *h2;
  size_t bytes;
};
Plan carve(void* base, int n, int H, int W, int dim, int f) {
  Plan p;
  Carver cv{base};
  const size_t hw = (size_t)n * H * W, g = hw / 256;          // pixels at full and at 1/16 resolution
  p.t3 = (half_t*)cv.take(g * dim * 2);
  p.r3 = (half_t*)cv.take(g * dim * 2);
  p.t4 = (half_t*)cv.take(g * dim * 2);
  p.u4 = (half_t*)cv.take(g * dim * 2);
  p.r4 = (half_t*)cv.take(g / 4 * dim * 2);
  for (int i = 0; i < 4; ++i) p.s[i] = (half_t*)cv.take((hw >> (4 + 2 * i)) * f * 2);
  for (int i = 0; i < 4; ++i) p.work[i] = (half_t*)cv.take(hw / 4 * f * 2);
  p.hu = (half_t*)cv.take(hw * (f / 2) * 2);
  p.h2 = (half_t*)cv.take(hw * kHeadMid * 2);
  p.bytes = cv.off;
  return p;
}

}  // namespace
}  // namespace sgr

using namespace sgr;

extern "C" {

size_t sgr_dpt_scratch_bytes(int32_t n, int32_t H, int32_t W, int32_t dim, int32_t features) {
  if (!sizes_ok(n, H, W, dim, features)) return 0;
  return carve(nullptr, n, H, W, dim, features).bytes;
}

int sgr_dpt_conv(const SgrDptConv* conv, void* stream) {
  if (!conv) return set_error(SGR_ERR_INVALID, "dpt_conv: null argument");
  return launch_conv(*conv, (hipStream_t)stream);
}

int sgr_dpt_up2(const void* src, int32_t n, int32_t h, int32_t w, int32_t channels, int32_t src_stride, void* dst, int32_t dst_stride,
                void* stream) {
  return launch_up2((const half_t*)src, n, h, w, channels, src_stride, (half_t*)dst, dst_stride, (hipStream_t)stream);
}

int sgr_dpt_resize_in(const float* src, int32_t planes, int32_t H, int32_t W, void* dst, int32_t h, int32_t w, void* stream) {
  return launch_resize("dpt_resize_in", dpt_resize_in_kernel, src, planes, H, W, dst, h, w, (hipStream_t)stream);
}

int sgr_dpt_resize_out(const float* src, int32_t planes, int32_t h, int32_t w, float* dst, int32_t H, int32_t W, void* stream) {
  return launch_resize("dpt_resize_out", dpt_resize_out_kernel, src, planes, h, w, dst, H, W, (hipStream_t)stream);
}

int sgr_dpt_forward(const SgrDptWeights* wt, const SgrDptCall* call, void* scratch, size_t scratch_bytes, void* stream_) {
  if (!wt || !call || !scratch) return set_error(SGR_ERR_INVALID, "dpt_forward: null argument");
  const int n = call->n, H = call->H, W = call->W, D = wt->dim, f = wt->features;
  if (!sizes_ok(n, H, W, D, f) || wt->chs0 < 8 || wt->chs0 % 8 || wt->chs0 > kMaxChannels || wt->chs1 < 8 || wt->chs1 % 8 ||
      wt->chs1 > kMaxChannels)
    return set_error(SGR_ERR_INVALID,
                     "dpt_forward: unsupported sizes (n=%d H=%d W=%d dim=%d features=%d stages=%d,%d); H and W multiples of 32, dim and features "
                     "multiples of 16, stage widths multiples of 8, all up to 1024", n, H, W, D, f, wt->chs0, wt->chs1);
  for (int i = 0; i < SGR_DPT_LAYERS; ++i)
    if (!wt->layer[i].weight) return set_error(SGR_ERR_INVALID, "dpt_forward: null weights");
  if (!call->tap3.data || !call->tap4.data || !call->l1 || !call->l2 || !call->depth || !aligned16(call->l1) || !aligned16(call->l2) ||
      !aligned16(call->depth))
    return set_error(SGR_ERR_INVALID, "dpt_forward: null or unaligned tensor");
  const Plan s = carve(scratch, n, H, W, D, f);
  if (scratch_bytes < s.bytes || !aligned16(scratch))
    return set_error(SGR_ERR_WORKSPACE, "dpt_forward: scratch of %zu bytes, need %zu (16-byte aligned)", scratch_bytes, s.bytes);
  hipStream_t stream = (hipStream_t)stream_;
  int rc = SGR_OK, layer = 0;
  LaunchRange on{call->first_launch, call->last_launch};
  // the next layer as one launch on an h x w map: out = relu?(conv(relu_in?(src)) + bias) + res0 + res1
  auto conv = [&](const half_t* src, int cin, int h, int w, int ks, int cout, int relu_in, int relu, const half_t* res0, const half_t* res1,
                  void* out, int out_kind = SGR_UPDATE_OUT_CL_F16) -> int {
    const SgrUpdateLayer& L = wt->layer[layer++];
    if (!on()) return SGR_OK;
    SgrDptConv c = {};
    c.src = src, c.src_stride = cin, c.cin = cin, c.ksize = ks, c.n = n, c.h = h, c.w = w;
    c.weight = L.weight, c.weight_elems = L.weight_elems, c.bias = L.bias, c.cout = cout, c.relu_in = relu_in, c.relu = relu;
    c.res0 = res0, c.res0_stride = cout, c.res1 = res1, c.res1_stride = cout, c.out = out, c.out_kind = out_kind, c.out_stride = cout;
    return launch_conv(c, stream);
  };
  auto up2 = [&](const half_t* src, int h, int w, int C, half_t* dst) -> int {
    return on() ? launch_up2(src, n, h, w, C, C, dst, C, stream) : SGR_OK;
  };
  const int gh = H / 16, gw = W / 16;
  // reassemble: the transformer's taps arrive NCHW
  if (on() && (rc = sgr_update_pack(&call->tap3, n, D, gh, gw, s.t3, D, D, stream_))) return rc;
  if ((rc = conv(s.t3, D, gh, gw, 1, D, 0, 0, nullptr, nullptr, s.r3))) return rc;
  if (on() && (rc = sgr_update_pack(&call->tap4, n, D, gh, gw, s.t4, D, D, stream_))) return rc;
  if ((rc = conv(s.t4, D, gh, gw, 1, D, 0, 0, nullptr, nullptr, s.u4))) return rc;
  {
    const SgrUpdateLayer& L = wt->layer[layer++];               // 3x3, stride 2, padding 1: weight [dim][k_pad], bias [dim]
    SgrResnetConv c = {};
    c.src = s.u4, c.src_stride = D, c.cin = D, c.ksize = 3, c.stride = 2, c.n = n, c.h = gh, c.w = gw, c.pad_top = 1, c.pad_left = 1;
    c.ho = gh / 2, c.wo = gw / 2, c.weight = L.weight, c.weight_elems = L.weight_elems, c.bias = L.bias, c.cout = D;
    c.out = s.r4, c.out_kind = SGR_UPDATE_OUT_CL_F16, c.out_stride = D;
    if (on() && (rc = sgr_resnet_conv(&c, stream_))) return rc;
  }
  if ((rc = conv((const half_t*)call->l1, wt->chs0, H / 4, W / 4, 3, f, 0, 0, nullptr, nullptr, s.s[0]))) return rc;
  if ((rc = conv((const half_t*)call->l2, wt->chs1, H / 8, W / 8, 3, f, 0, 0, nullptr, nullptr, s.s[1]))) return rc;
  if ((rc = conv(s.r3, D, gh, gw, 3, f, 0, 0, nullptr, nullptr, s.s[2]))) return rc;
  if ((rc = conv(s.r4, D, gh / 2, gw / 2, 3, f, 0, 0, nullptr, nullptr, s.s[3]))) return rc;
  // refinenet4: no skip, so only resConfUnit2
  int h = gh / 2, w = gw / 2;
  if ((rc = conv(s.s[3], f, h, w, 3, f, 1, 1, nullptr, nullptr, s.work[0]))) return rc;
  if ((rc = conv(s.work[0], f, h, w, 3, f, 0, 0, s.s[3], nullptr, s.work[1]))) return rc;
  if ((rc = up2(s.work[1], h, w, f, s.work[2]))) return rc;
  h *= 2, w *= 2;
  if ((rc = conv(s.work[2], f, h, w, 1, f, 0, 0, nullptr, nullptr, s.work[3]))) return rc;
  half_t* path = s.work[3];
  for (int i = 2; i >= 0; --i) {
    half_t* fr[3];
    for (int k = 0, j = 0; k < 4 && j < 3; ++k)
      if (s.work[k] != path) fr[j++] = s.work[k];
    const half_t* skip = s.s[i];
    if ((rc = conv(skip, f, h, w, 3, f, 1, 1, nullptr, nullptr, fr[0]))) return rc;           // resConfUnit1.conv1
    if ((rc = conv(fr[0], f, h, w, 3, f, 0, 0, skip, path, fr[1]))) return rc;                // resConfUnit1.conv2 + skip + path
    if ((rc = conv(fr[1], f, h, w, 3, f, 1, 1, nullptr, nullptr, fr[0]))) return rc;          // resConfUnit2.conv1
    if ((rc = conv(fr[0], f, h, w, 3, f, 0, 0, fr[1], nullptr, path))) return rc;             // resConfUnit2.conv2 + its input
    if ((rc = up2(path, h, w, f, fr[0]))) return rc;
    h *= 2, w *= 2;
    if ((rc = conv(fr[0], f, h, w, 1, f, 0, 0, nullptr, nullptr, fr[1]))) return rc;          // out_conv
    path = fr[1];
  }
  // the head, from the 1/2 map to the depth plane
  half_t* h0 = path == s.work[0] ? s.work[1] : s.work[0];
  if ((rc = conv(path, f, h, w, 3, f / 2, 0, 0, nullptr, nullptr, h0))) return rc;
  if ((rc = up2(h0, h, w, f / 2, s.hu))) return rc;
  if ((rc = conv(s.hu, f / 2, H, W, 3, kHeadMid, 0, 1, nullptr, nullptr, s.h2))) return rc;
  if ((rc = conv(s.h2, kHeadMid, H, W, 1, 1, 0, 1, nullptr, nullptr, call->depth, SGR_UPDATE_OUT_CL_F32))) return rc;
  return SGR_OK;
}

}  // extern "C"
