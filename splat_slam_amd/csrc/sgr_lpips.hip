// LPIPS v0.1 on the AlexNet trunk (the third image figure of eval_rendering; the definition is DESIGN.md section 3, "LPIPS"), inference
// only.  A call on n pairs works on 2n images: image i is the first, image n + i the second member of pair i.
//   sgr_lpips_pack, _pack_pairs   the scaled input, channels-last fp16 [2n][H][W][8] (channels 3..7 zero), from the frame table of
//                                 sgr_render_metrics (exposure and clamp applied to the render) or from two fp32 tensors
//   sgr_lpips_conv                relu(conv + bias), 11x11 stride 4, 5x5 or 3x3, symmetric zero padding, on the shared MFMA tile
//   sgr_lpips_maxpool             3x3 stride 2 without padding
//   sgr_lpips_distance            one tap: per-(pair, workgroup) sums of d_p = sum_c w_c (u_c - v_c)^2 over unit-normalised features
//   sgr_lpips_forward             the whole metric: 14 stream-ordered launches, no host synchronisation
// The GEMM is the tile of sgr_conv_mma.h; a workgroup's 128 output pixels are consecutive pixels of the batch (a tile may span images,
// no pixel's sum depends on its tile) and output channels come in tiles of 64.  Every sum has a fixed order: no atomics, bitwise
// reproducible, and a pair gives the bits it has alone in any batch.
#include <cstdint>

#include "sgr_conv_mma.h"

namespace sgr {
namespace {

constexpr int kInPad = 8;                                    // the 3 image channels padded to one 16-byte chunk
constexpr int kBN = 64;                                      // output channels of one workgroup
constexpr int kTaps = 5;
constexpr int kChannels[kTaps] = {64, 192, 384, 256, 256};
constexpr int kKsize[kTaps] = {11, 5, 3, 3, 3};
constexpr int kDistPixels = SGR_LPIPS_DIST_PIXELS;           // pixels of one workgroup of the distance: 4 rounds of 32 groups of 8 lanes
constexpr float kNormEps = 1e-8f;                            // inside the square root of the unit normalisation

// ---- pack
struct PackTab {
  const float* first[SGR_LPIPS_MAX_PAIRS];                   // [3][H][W] each
  const float* second[SGR_LPIPS_MAX_PAIRS];
  const float* exp_a[SGR_LPIPS_MAX_PAIRS];                   // device scalars or NULL, of the first image
  const float* exp_b[SGR_LPIPS_MAX_PAIRS];
  float shift[3], scale[3];
  int n, HW, clamp_first, normalize;
};

// One thread per pixel of image blockIdx.y: three planar fp32 loads, one 16-byte store.  The exposure is a product and a sum rounded
// on their own, the bits of torch's exp(a) * r + b (sgr_render_metrics leaves the two to the compiler, which may fuse them: up to one fp32
// ulp apart before the clamp, far below the fp16 value written here).
__global__ void __launch_bounds__(kThreads) lpips_pack_kernel(const PackTab t, half_t* __restrict__ dst) {
#pragma clang fp contract(off)
  const int img = blockIdx.y, o = blockIdx.x * kThreads + threadIdx.x;
  if (o >= t.HW) return;
  const bool second = img >= t.n;
  const int i = second ? img - t.n : img;
  const float* src = second ? t.second[i] : t.first[i];
  const bool expose = !second && t.clamp_first;
  const float ea = expose && t.exp_a[i] ? expf(t.exp_a[i][0]) : 1.f, eb = expose && t.exp_b[i] ? t.exp_b[i][0] : 0.f;
  half8 v = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    float x = src[(int64_t)c * t.HW + o];
    if (expose) x = exposed_image(ea, x, eb);
    if (t.normalize) x = 2.f * x - 1.f;
    v[c] = (half_t)((x - t.shift[c]) / t.scale[c]);
  }
  *(half8*)&dst[((int64_t)img * t.HW + o) * kInPad] = v;
}

// ---- convolution
struct ConvArgs {
  SgrLpipsConv c;
  int ho, wo, HWo, M, k_pad;                 // M = n * HWo output pixels in the batch
};

// The shared tile on the kBM output pixels m0 .. of the batch (a tile may span images): stride c.stride, c.pad rows and columns of
// zeros all round.
template <int KS>
__global__ void __launch_bounds__(kThreads) lpips_conv_kernel(const ConvArgs a) {
  constexpr int NT = kBN / 16;
  __shared__ __attribute__((aligned(16))) half_t Xs[kBM * kRow];
  __shared__ __attribute__((aligned(16))) half_t Ws[kBN * kRow];
  const SgrLpipsConv& c = a.c;
  const int tid = threadIdx.x, m0 = blockIdx.x * kBM, n0 = blockIdx.y * kBN;

  ConvWindow win;
  const half_t* src[2];                                      // the image of each of this thread's two pixel rows
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int m = m0 + (tid >> 2) + 64 * i;
    const bool pv = m < a.M;
    const int mm = pv ? m : 0, img = mm / a.HWo, p = mm - img * a.HWo, oy = p / a.wo;
    src[i] = (const half_t*)c.src + (int64_t)img * c.h * c.w * c.cin;
    win.row(i, pv, p, oy, a.wo, c.stride, c.pad, c.pad);
  }
  auto gather = [&](int i, bool tv, int ty, int tx, int ch) { return win.chunk(src[i], c.h, c.w, c.cin, i, tv, ty, tx, ch); };
  floatx4 acc[NT][2];
  conv_mma_mainloop<KS, kBN>(Xs, Ws, (const half_t*)c.weight, n0, a.k_pad, c.cin, gather, acc);

  // acc[t][j] holds channels nb .. nb + 3 of pixel gm of the batch
  half_t* out = (half_t*)c.out;
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int64_t gm = acc_pixel(j);
    if (gm >= a.M) continue;
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      const int nb = acc_channel(n0, t);
      const floatx4 v = acc[t][j] + *(const floatx4*)&c.bias[nb];
      half4 o;
#pragma unroll
      for (int r = 0; r < 4; ++r) o[r] = (half_t)fmaxf(v[r], 0.f);
      *(half4*)&out[gm * c.cout + nb] = o;
    }
  }
}

// ---- pool
struct PoolArgs {
  const half_t* src;
  half_t* dst;
  int h, w, ho, wo, chunks;
  int64_t total;                             // n * ho * wo * chunks
};

// One thread per (output pixel, 8 channels): nine 16-byte loads, all inside the map, one 16-byte store.
__global__ void __launch_bounds__(kThreads) lpips_pool_kernel(const PoolArgs a) {
  const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i >= a.total) return;
  const int j = (int)(i % a.chunks);
  const int64_t q = i / a.chunks;
  const int ox = (int)(q % a.wo), oy = (int)((q / a.wo) % a.ho);
  const int64_t img = q / ((int64_t)a.wo * a.ho);
  const int64_t C = (int64_t)a.chunks * 8;
  half8 best = *(const half8*)&a.src[((img * a.h + oy * 2) * a.w + ox * 2) * C + j * 8];
#pragma unroll
  for (int t = 1; t < 9; ++t) {
    const int yy = oy * 2 + t / 3, xx = ox * 2 + t % 3;
    const half8 v = *(const half8*)&a.src[((img * a.h + yy) * a.w + xx) * C + j * 8];
#pragma unroll
    for (int k = 0; k < 8; ++k) best[k] = v[k] > best[k] ? v[k] : best[k];
  }
  *(half8*)&a.dst[q * C + j * 8] = best;
}

// ---- distance
struct DistArgs {
  const half_t* maps;                        // [2n][P][C]
  const float* weight;                       // [C]
  float* partials;                           // [n][blocks]
  float* per_pixel;                          // [n][P] or NULL
  int n, P;
};

// One tap of pair blockIdx.y on the kDistPixels pixels from blockIdx.x * kDistPixels: eight lanes per pixel, lane l holds the 16-byte
// chunks l, l + 8, ... of both feature vectors (NCH = C / 64 chunks each, read once) from the norm to the difference.  Per pixel:
// s = sum f^2 (the lane's values in ascending order, then a butterfly over the eight lanes, so every lane holds the same bits),
// u = f * (1 / sqrt(1e-8 + s)) rounded, likewise v, t = u - v rounded, d = sum w t^2 in the same order.  Nothing here may be fused:
// u - v must see the rounded u and v, so that equal maps give exactly 0 and swapped maps the same bits.  A group adds its four
// pixels in ascending order, thread 0 the 32 groups in ascending order.
template <int NCH>
__global__ void __launch_bounds__(kThreads) lpips_dist_kernel(const DistArgs a) {
#pragma clang fp contract(off)
  constexpr int C = 64 * NCH;
  __shared__ float red[kThreads / 8];
  const int tid = threadIdx.x, g = tid >> 3, l = tid & 7;
  const int pair = blockIdx.y, p0 = blockIdx.x * kDistPixels;
  const half_t* f0 = a.maps + (int64_t)pair * a.P * C;
  const half_t* f1 = a.maps + (int64_t)(a.n + pair) * a.P * C;
  float w[NCH][8];
#pragma unroll
  for (int j = 0; j < NCH; ++j) {
    const floatx4 lo = *(const floatx4*)&a.weight[(j * 8 + l) * 8], hi = *(const floatx4*)&a.weight[(j * 8 + l) * 8 + 4];
#pragma unroll
    for (int k = 0; k < 4; ++k) w[j][k] = lo[k], w[j][k + 4] = hi[k];
  }
  float acc = 0.f;
  for (int it = 0; it < kDistPixels / (kThreads / 8); ++it) {
    const int p = p0 + it * (kThreads / 8) + g;
    const bool valid = p < a.P;
    const int64_t row = (int64_t)(valid ? p : a.P - 1) * C;
    half8 x[NCH], y[NCH];
#pragma unroll
    for (int j = 0; j < NCH; ++j) {
      x[j] = *(const half8*)&f0[row + (j * 8 + l) * 8];
      y[j] = *(const half8*)&f1[row + (j * 8 + l) * 8];
    }
    float s0 = 0.f, s1 = 0.f;
#pragma unroll
    for (int j = 0; j < NCH; ++j)
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        const float xf = (float)x[j][k], yf = (float)y[j][k];
        s0 += xf * xf;
        s1 += yf * yf;
      }
#pragma unroll
    for (int d = 1; d < 8; d <<= 1) {
      s0 += __shfl_xor(s0, d);
      s1 += __shfl_xor(s1, d);
    }
    const float r0 = 1.f / sqrtf(kNormEps + s0), r1 = 1.f / sqrtf(kNormEps + s1);
    float dp = 0.f;
#pragma unroll
    for (int j = 0; j < NCH; ++j)
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        const float u = (float)x[j][k] * r0, v = (float)y[j][k] * r1;
        const float t = u - v;
        dp += w[j][k] * (t * t);
      }
#pragma unroll
    for (int d = 1; d < 8; d <<= 1) dp += __shfl_xor(dp, d);
    if (valid) {
      acc += dp;
      if (a.per_pixel && l == 0) a.per_pixel[(int64_t)pair * a.P + p] = dp;
    }
  }
  if (l == 0) red[g] = acc;
  __syncthreads();
  if (tid == 0) {
    float s = red[0];
    for (int i = 1; i < kThreads / 8; ++i) s += red[i];
    a.partials[(int64_t)pair * gridDim.x + blockIdx.x] = s;
  }
}

// ---- final
struct FinalArgs {
  const float* partials[kTaps];              // [n][blocks[t]]
  int blocks[kTaps], pixels[kTaps];
  float* out;                                // [n]
  float* levels;                             // [n][5] or NULL
};

// One workgroup per pair: thread t < 5 adds the partial sums of tap t in ascending order in fp64 and divides by the tap's pixels,
// thread 0 adds the five means in ascending order; one rounding to fp32 each.
__global__ void __launch_bounds__(64) lpips_final_kernel(const FinalArgs a) {
  __shared__ double lv[kTaps];
  const int t = threadIdx.x, pair = blockIdx.x;
  if (t < kTaps) {
    const float* p = a.partials[t] + (int64_t)pair * a.blocks[t];
    double s = 0.0;
    for (int i = 0; i < a.blocks[t]; ++i) s += (double)p[i];
    lv[t] = s / (double)a.pixels[t];
    if (a.levels) a.levels[pair * kTaps + t] = (float)lv[t];
  }
  __syncthreads();
  if (t == 0) a.out[pair] = (float)((((lv[0] + lv[1]) + lv[2]) + lv[3]) + lv[4]);
}

// ---- host
inline int conv_out(int i, int k, int s, int pad) { return i + 2 * pad < k ? 0 : (i + 2 * pad - k) / s + 1; }
inline int pool_out(int i) { return i < 3 ? 0 : (i - 3) / 2 + 1; }
inline int dist_blocks(int P) { return (P + kDistPixels - 1) / kDistPixels; }

int launch_pack(const PackTab& t, int H, int W, half_t* dst, hipStream_t stream) {
  const dim3 grid((unsigned)((t.HW + kThreads - 1) / kThreads), (unsigned)(2 * t.n));
  hipLaunchKernelGGL(lpips_pack_kernel, grid, dim3(kThreads), 0, stream, t, dst);
  return launched("lpips_pack");
}

bool pack_sizes_ok(int n, int H, int W) { return n >= 1 && n <= SGR_LPIPS_MAX_PAIRS && map_ok(2 * n, H, W); }

int fill_norm(PackTab& t, const float* shift, const float* scale) {
  if (!shift || !scale) return set_error(SGR_ERR_INVALID, "lpips_pack: null shift or scale");
  for (int c = 0; c < 3; ++c) {
    if (!(scale[c] > 0.f)) return set_error(SGR_ERR_INVALID, "lpips_pack: scale[%d] = %g is not positive", c, (double)scale[c]);
    t.shift[c] = shift[c], t.scale[c] = scale[c];
  }
  return SGR_OK;
}

int pack_frames(int n, const SgrMetricFrame* frames, int H, int W, const float* shift, const float* scale, half_t* dst, hipStream_t stream) {
  if (!frames || !dst || !aligned16(dst)) return set_error(SGR_ERR_INVALID, "lpips_pack: null or unaligned argument");
  if (!pack_sizes_ok(n, H, W)) return set_error(SGR_ERR_INVALID, "lpips_pack: bad sizes (n=%d H=%d W=%d); 1 <= n <= %d", n, H, W, SGR_LPIPS_MAX_PAIRS);
  PackTab t = {};
  if (int rc = fill_norm(t, shift, scale)) return rc;
  for (int i = 0; i < n; ++i) {
    if (!frames[i].render || !frames[i].gt_image) return set_error(SGR_ERR_INVALID, "lpips_pack: frame %d has no image", i);
    t.first[i] = frames[i].render, t.second[i] = frames[i].gt_image, t.exp_a[i] = frames[i].exposure_a, t.exp_b[i] = frames[i].exposure_b;
  }
  t.n = n, t.HW = H * W, t.clamp_first = 1, t.normalize = 1;
  return launch_pack(t, H, W, dst, stream);
}

int pack_pairs(const float* img0, const float* img1, int n, int H, int W, int normalize, const float* shift, const float* scale, half_t* dst,
               hipStream_t stream) {
  if (!img0 || !img1 || !dst || !aligned16(dst)) return set_error(SGR_ERR_INVALID, "lpips_pack_pairs: null or unaligned argument");
  if (!pack_sizes_ok(n, H, W))
    return set_error(SGR_ERR_INVALID, "lpips_pack_pairs: bad sizes (n=%d H=%d W=%d); 1 <= n <= %d", n, H, W, SGR_LPIPS_MAX_PAIRS);
  PackTab t = {};
  if (int rc = fill_norm(t, shift, scale)) return rc;
  for (int i = 0; i < n; ++i) t.first[i] = img0 + (int64_t)i * 3 * H * W, t.second[i] = img1 + (int64_t)i * 3 * H * W;
  t.n = n, t.HW = H * W, t.clamp_first = 0, t.normalize = normalize != 0;
  return launch_pack(t, H, W, dst, stream);
}

// launch(integral_constant<KS>) for the kernel size 11, 5 or 3
template <class Launch>
inline void dispatch_lpips_conv(int ksize, Launch&& launch) {
  if (ksize == 11)
    launch(std::integral_constant<int, 11>{});
  else if (ksize == 5)
    launch(std::integral_constant<int, 5>{});
  else
    launch(std::integral_constant<int, 3>{});
}

int launch_conv(const SgrLpipsConv& c, hipStream_t stream) {
  if (!c.src || !c.weight || !c.bias || !c.out) return set_error(SGR_ERR_INVALID, "lpips_conv: null argument");
  if (!map_ok(c.n, c.h, c.w) || c.cin < 8 || c.cin % 8 || c.cin > 1024)
    return set_error(SGR_ERR_INVALID, "lpips_conv: bad sizes (n=%d h=%d w=%d cin=%d); n <= 65535, cin a multiple of 8 up to 1024", c.n, c.h, c.w, c.cin);
  if (c.cout < kBN || c.cout % kBN || c.cout > 1024) return set_error(SGR_ERR_INVALID, "lpips_conv: cout %d is not a multiple of 64 in 64..1024", c.cout);
  if (c.ksize != 11 && c.ksize != 5 && c.ksize != 3) return set_error(SGR_ERR_INVALID, "lpips_conv: kernel size %d is not 11, 5 or 3", c.ksize);
  // (the trunk has strides 1 and 4; 2 is what the kernel shares with the encoder's and the ResNet's, and the tests hold the three to each other)
  if (c.stride != 1 && c.stride != 2 && c.stride != 4) return set_error(SGR_ERR_INVALID, "lpips_conv: stride %d is not 1, 2 or 4", c.stride);
  if (c.pad < 0 || c.pad >= c.ksize) return set_error(SGR_ERR_INVALID, "lpips_conv: padding %d outside 0..ksize-1", c.pad);
  ConvArgs a;
  a.c = c;
  a.ho = conv_out(c.h, c.ksize, c.stride, c.pad), a.wo = conv_out(c.w, c.ksize, c.stride, c.pad);
  if (a.ho < 1 || a.wo < 1)
    return set_error(SGR_ERR_INVALID, "lpips_conv: a %d x %d map has no output under kernel %d, padding %d", c.h, c.w, c.ksize, c.pad);
  a.HWo = a.ho * a.wo;
  if ((int64_t)c.n * a.HWo > 0x7fffffff - kBM) return set_error(SGR_ERR_INVALID, "lpips_conv: %d x %d x %d output pixels do not fit int32", c.n, a.ho, a.wo);
  a.M = c.n * a.HWo;
  a.k_pad = round_up(c.ksize * c.ksize * c.cin, kBK);
  if (c.weight_elems < (int64_t)c.cout * a.k_pad || !aligned16(c.weight) || !aligned16(c.bias) || !aligned16(c.src) || !aligned16(c.out))
    return set_error(SGR_ERR_INVALID, "lpips_conv: 16-byte aligned bases and packed weights [%d][%d] fp16, got %lld elements", c.cout, a.k_pad,
                     (long long)c.weight_elems);
  const dim3 grid((unsigned)tiles_of(a.M), (unsigned)(c.cout / kBN)), block(kThreads);
  dispatch_lpips_conv(c.ksize, [&](auto ks) { hipLaunchKernelGGL((lpips_conv_kernel<decltype(ks)::value>), grid, block, 0, stream, a); });
  return launched("lpips_conv");
}

int launch_pool(const half_t* src, int n, int h, int w, int C, half_t* dst, hipStream_t stream) {
  PoolArgs a;
  a.src = src, a.dst = dst, a.h = h, a.w = w, a.ho = pool_out(h), a.wo = pool_out(w), a.chunks = C / 8;
  a.total = (int64_t)n * a.ho * a.wo * a.chunks;
  const int64_t blocks = (a.total + kThreads - 1) / kThreads;
  if (blocks > 0x7fffffff) return set_error(SGR_ERR_INVALID, "lpips_maxpool: the map is too large for one launch");
  hipLaunchKernelGGL(lpips_pool_kernel, dim3((unsigned)blocks), dim3(kThreads), 0, stream, a);
  return launched("lpips_maxpool");
}

int launch_dist(const half_t* maps, int n, int P, int C, const float* weight, float* partials, float* per_pixel, hipStream_t stream) {
  DistArgs a;
  a.maps = maps, a.weight = weight, a.partials = partials, a.per_pixel = per_pixel, a.n = n, a.P = P;
  const dim3 grid((unsigned)dist_blocks(P), (unsigned)n), block(kThreads);
  switch (C) {
    case 64: hipLaunchKernelGGL(lpips_dist_kernel<1>, grid, block, 0, stream, a); break;
    case 192: hipLaunchKernelGGL(lpips_dist_kernel<3>, grid, block, 0, stream, a); break;
    case 256: hipLaunchKernelGGL(lpips_dist_kernel<4>, grid, block, 0, stream, a); break;
    case 384: hipLaunchKernelGGL(lpips_dist_kernel<6>, grid, block, 0, stream, a); break;
    default: return set_error(SGR_ERR_INVALID, "lpips_distance: %d channels; the taps have 64, 192, 256 or 384", C);
  }
  return launched("lpips_distance");
}

// The sizes of a call and its maps.  Every launch reads one of two buffers and writes the other: the packed images, the pooled maps
// and tap 4 live in the first, taps 1, 2, 3 and 5 in the second (a tap is dead once its distance and its pool have read it), each
// buffer as large as its largest map; then the partial sums of every tap.
struct Plan {
  int h[kTaps], w[kTaps];                    // the taps
  int hp[2], wp[2];                          // the pooled maps behind taps 1 and 2
  bool ok;
  half_t *xin, *tap[kTaps], *pool[2];
  float* parts[kTaps];
  size_t bytes;
};
Plan carve(void* base, int n, int H, int W) {
  Plan s = {};
  s.ok = false;
  if (!pack_sizes_ok(n, H, W)) return s;
  s.h[0] = conv_out(H, 11, 4, 2), s.w[0] = conv_out(W, 11, 4, 2);
  s.hp[0] = pool_out(s.h[0]), s.wp[0] = pool_out(s.w[0]);
  s.h[1] = s.hp[0], s.w[1] = s.wp[0];
  s.hp[1] = pool_out(s.h[1]), s.wp[1] = pool_out(s.w[1]);
  for (int t = 2; t < kTaps; ++t) s.h[t] = s.hp[1], s.w[t] = s.wp[1];
  if (s.hp[1] < 1 || s.wp[1] < 1) return s;
  s.ok = true;
  Carver cv{base};
  const size_t m = 2 * (size_t)n;
  auto tap_bytes = [&](int t) { return m * s.h[t] * s.w[t] * kChannels[t] * 2; };
  auto pool_bytes = [&](int t) { return m * s.hp[t] * s.wp[t] * kChannels[t] * 2; };
  auto mx = [](size_t a, size_t b) { return a > b ? a : b; };
  half_t* const first = (half_t*)cv.take(mx(mx(m * H * W * kInPad * 2, pool_bytes(0)), mx(pool_bytes(1), tap_bytes(3))));
  half_t* const second = (half_t*)cv.take(mx(mx(tap_bytes(0), tap_bytes(1)), mx(tap_bytes(2), tap_bytes(4))));
  s.xin = s.pool[0] = s.pool[1] = s.tap[3] = first;
  s.tap[0] = s.tap[1] = s.tap[2] = s.tap[4] = second;
  for (int t = 0; t < kTaps; ++t) s.parts[t] = (float*)cv.take((size_t)n * dist_blocks(s.h[t] * s.w[t]) * 4);
  s.bytes = cv.off;
  return s;
}

}  // namespace
}  // namespace sgr

using namespace sgr;

extern "C" {

size_t sgr_lpips_scratch_bytes(int32_t n, int32_t H, int32_t W) {
  const Plan s = carve(nullptr, n, H, W);
  return s.ok ? s.bytes : 0;
}

int sgr_lpips_pack(int32_t n, const SgrMetricFrame* frames, int32_t H, int32_t W, const float* shift, const float* scale, void* dst,
                   void* stream) {
  return pack_frames(n, frames, H, W, shift, scale, (half_t*)dst, (hipStream_t)stream);
}

int sgr_lpips_pack_pairs(const float* img0, const float* img1, int32_t n, int32_t H, int32_t W, int32_t normalize, const float* shift,
                         const float* scale, void* dst, void* stream) {
  return pack_pairs(img0, img1, n, H, W, normalize, shift, scale, (half_t*)dst, (hipStream_t)stream);
}

int sgr_lpips_conv(const SgrLpipsConv* conv, void* stream) {
  if (!conv) return set_error(SGR_ERR_INVALID, "lpips_conv: null argument");
  return launch_conv(*conv, (hipStream_t)stream);
}

int sgr_lpips_maxpool(const void* src, int32_t n, int32_t h, int32_t w, int32_t channels, void* dst, void* stream) {
  if (!src || !dst || !aligned16(src) || !aligned16(dst)) return set_error(SGR_ERR_INVALID, "lpips_maxpool: null or unaligned argument");
  if (!map_ok(n, h, w) || h < 3 || w < 3 || channels < 8 || channels % 8 || channels > 1024)
    return set_error(SGR_ERR_INVALID, "lpips_maxpool: bad sizes (n=%d h=%d w=%d channels=%d); h and w >= 3, channels a multiple of 8 up to 1024", n,
                     h, w, channels);
  return launch_pool((const half_t*)src, n, h, w, channels, (half_t*)dst, (hipStream_t)stream);
}

int sgr_lpips_distance(const void* maps, int32_t n, int32_t P, int32_t C, const float* weight, float* partials, float* per_pixel,
                       void* stream) {
  if (!maps || !weight || !partials || !aligned16(maps) || !aligned16(weight))
    return set_error(SGR_ERR_INVALID, "lpips_distance: null or unaligned argument");
  if (n < 1 || n > 32767 || P < 1 || P > 0x7fffffff - kDistPixels)
    return set_error(SGR_ERR_INVALID, "lpips_distance: bad sizes (n=%d P=%d); n <= 32767", n, P);
  return launch_dist((const half_t*)maps, n, P, C, weight, partials, per_pixel, (hipStream_t)stream);
}

int sgr_lpips_forward(const SgrLpipsWeights* wt, const SgrLpipsCall* call, void* scratch, size_t scratch_bytes, void* stream_) {
  if (!wt || !call || !scratch || !call->out) return set_error(SGR_ERR_INVALID, "lpips_forward: null argument");
  const int n = call->n, H = call->H, W = call->W;
  const Plan s = carve(scratch, n, H, W);
  if (!s.ok)
    return set_error(SGR_ERR_INVALID, "lpips_forward: unsupported sizes (n=%d H=%d W=%d); 1 <= n <= %d, H and W >= 31", n, H, W, SGR_LPIPS_MAX_PAIRS);
  if (scratch_bytes < s.bytes || !aligned16(scratch))
    return set_error(SGR_ERR_WORKSPACE, "lpips_forward: scratch of %zu bytes, need %zu (16-byte aligned)", scratch_bytes, s.bytes);
  for (int t = 0; t < kTaps; ++t)
    if (!wt->conv[t].weight || !wt->conv[t].bias || !wt->lin[t] || !aligned16(wt->lin[t])) return set_error(SGR_ERR_INVALID, "lpips_forward: null or unaligned weights");
  if (!call->frames && (!call->img0 || !call->img1)) return set_error(SGR_ERR_INVALID, "lpips_forward: neither a frame table nor two images");
  hipStream_t stream = (hipStream_t)stream_;
  int rc = SGR_OK;
  LaunchRange on{call->first_launch, call->last_launch};
  if (on()) {
    rc = call->frames ? pack_frames(n, call->frames, H, W, wt->shift, wt->scale, s.xin, stream)
                      : pack_pairs(call->img0, call->img1, n, H, W, call->normalize, wt->shift, wt->scale, s.xin, stream);
    if (rc) return rc;
  }
  const half_t* cur = s.xin;
  int cin = kInPad, h = H, w = W;
  for (int t = 0; t < kTaps; ++t) {
    SgrLpipsConv c = {};
    c.src = cur, c.n = 2 * n, c.h = h, c.w = w, c.cin = cin, c.ksize = kKsize[t], c.stride = t == 0 ? 4 : 1, c.pad = t == 0 ? 2 : kKsize[t] / 2;
    c.weight = wt->conv[t].weight, c.weight_elems = wt->conv[t].weight_elems, c.bias = wt->conv[t].bias, c.cout = kChannels[t], c.out = s.tap[t];
    if (on() && (rc = launch_conv(c, stream))) return rc;
    if (on() && (rc = launch_dist(s.tap[t], n, s.h[t] * s.w[t], kChannels[t], wt->lin[t], s.parts[t], nullptr, stream))) return rc;
    cur = s.tap[t], cin = kChannels[t], h = s.h[t], w = s.w[t];
    if (t < 2) {
      if (on() && (rc = launch_pool(s.tap[t], 2 * n, h, w, cin, s.pool[t], stream))) return rc;
      cur = s.pool[t], h = s.hp[t], w = s.wp[t];
    }
  }
  if (on()) {
    FinalArgs f;
    for (int t = 0; t < kTaps; ++t) f.partials[t] = s.parts[t], f.pixels[t] = s.h[t] * s.w[t], f.blocks[t] = dist_blocks(f.pixels[t]);
    f.out = call->out, f.levels = call->levels;
    hipLaunchKernelGGL(lpips_final_kernel, dim3((unsigned)n), dim3(64), 0, stream, f);
    if ((rc = launched("lpips_forward: final"))) return rc;
  }
  return SGR_OK;
}

}  // extern "C"
