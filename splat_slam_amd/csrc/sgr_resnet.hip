// The ResNet-V2 backbone of the mono-depth prior (weight-standardised convolutions without bias, group norms, bottleneck blocks; the
// equations are DESIGN.md section 3, "Mono-depth prior"), inference only.
//   sgr_resnet_conv        one implicit-GEMM convolution (1x1, 3x3, 7x7; stride 1 or 2; explicit top / left padding and output size, taps
//                          outside the map read zero) on mfma_f32_16x16x32_f16, with a fused epilogue or, with a group norm, the raw fp32
//                          sums and per-tile, per-group shifted statistics
//   sgr_resnet_stats       the same statistics of a given fp32 map (what a caller without a convolution in front of the norm needs)
//   sgr_resnet_groupnorm   the second launch of a norm: merges the statistics in fp64, writes relu?(residual + affine(normalised))
//   sgr_resnet_maxpool     3x3 stride 2, TF "same" padding filled with -inf
//   sgr_resnet_forward     a whole backbone: 4 + sum over stages (6 blocks + 2) stream-ordered launches, no host synchronisation
// Layouts, the launch list and the statistics scheme are described in DESIGN.md section 3, "ResNet-V2 backbone".  The GEMM is the shared
// tile of sgr_conv_mma.h; here a workgroup's 128 output pixels belong to one image (blockIdx.z), the padding is explicit and output
// channels come in tiles of 16, 32 or 64.  Every sum has a fixed order: no atomics, bitwise reproducible, and image i of a batch gives
// the bits of that image alone.
#include <cstdint>

#include "sgr_conv_mma.h"

namespace sgr {
namespace {

constexpr int kInPad = 8;                   // the 3 image channels padded to one 16-byte chunk
constexpr int kMaxGroups = 256;             // one merge thread per group
constexpr int kMaxChannels = 1024;

struct ConvArgs {
  SgrResnetConv c;
  int HWo, k_pad, tiles, cshift;            // cshift = log2(channels per group)
};

// The shared tile on the kBM output pixels m0 .. of image blockIdx.z: stride c.stride, c.pad_top rows and c.pad_left columns of zeros
// in front, whatever the output size needs behind.
template <int KS, int BN>
__global__ void __launch_bounds__(kThreads) resnet_conv_kernel(const ConvArgs a) {
  constexpr int NT = BN / 16;
  __shared__ __attribute__((aligned(16))) half_t Xs[kBM * kRow];
  __shared__ __attribute__((aligned(16))) half_t Ws[BN * kRow];
  __shared__ float red[2][4][BN];
  __shared__ float shift[BN];
  const SgrResnetConv& c = a.c;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int img = blockIdx.z, m0 = blockIdx.x * kBM, n0 = blockIdx.y * BN;
  const half_t* src = (const half_t*)c.src + (int64_t)img * c.h * c.w * c.src_stride;

  ConvWindow win;
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int m = m0 + (tid >> 2) + 64 * i;
    const bool pv = m < a.HWo;
    const int mm = pv ? m : 0;
    win.row(i, pv, mm, mm / c.wo, c.wo, c.stride, c.pad_top, c.pad_left);
  }
  auto gather = [&](int i, bool tv, int ty, int tx, int ch) { return win.chunk(src, c.h, c.w, c.src_stride, i, tv, ty, tx, ch); };
  floatx4 acc[NT][2];
  conv_mma_mainloop<KS, BN>(Xs, Ws, (const half_t*)c.weight, n0, a.k_pad, c.cin, gather, acc);

  // acc[t][j] holds channels acc_channel(n0, t) .. + 3 of pixel acc_pixel(j) of this image
  bool valid[2];
  int64_t gm[2];                                             // pixel index over the whole batch
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int m = acc_pixel(j);
    valid[j] = m < a.HWo;
    gm[j] = (int64_t)img * a.HWo + m;
  }

  if (c.norm) {
    // Per (tile, group): the count, a reference value s = the sum of the group's first channel at the tile's first pixel, S1 = sum (v - s)
    // and S2 = sum (v - s)^2 over the tile's pixels and the group's channels.  The 16 pixel lanes are summed by a butterfly, then one
    // thread per group adds the channels in ascending order and, inside a channel, the waves in ascending order.
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      if (!valid[j]) continue;
#pragma unroll
      for (int t = 0; t < NT; ++t) *(floatx4*)&c.raw[acc_channel(gm[j] * c.cout + n0, t)] = acc[t][j];
    }
    const int cmask = (1 << a.cshift) - 1;
    if (wave == 0 && (lane & 15) == 0) {
#pragma unroll
      for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int n = acc_channel(0, t) + r;
          if ((n & cmask) == 0) shift[n >> a.cshift] = acc[t][0][r];
        }
    }
    __syncthreads();
    tile_shifted_sums<BN>(acc, valid, [&](int n) { return shift[n >> a.cshift]; }, red);
    __syncthreads();
    if (tid < (BN >> a.cshift)) {
      const int cpg = 1 << a.cshift;
      float s1 = 0.f, s2 = 0.f;
      for (int n = tid * cpg; n < (tid + 1) * cpg; ++n) {
        s1 += ((red[0][0][n] + red[0][1][n]) + red[0][2][n]) + red[0][3][n];
        s2 += ((red[1][0][n] + red[1][1][n]) + red[1][2][n]) + red[1][3][n];
      }
      const float cnt = (float)(min(kBM, a.HWo - m0) * cpg);
      *(floatx4*)&c.stats[(((int64_t)img * a.tiles + blockIdx.x) * c.groups + (n0 >> a.cshift) + tid) * 4] = floatx4{cnt, shift[tid], s1, s2};
    }
    return;
  }

#pragma unroll
  for (int j = 0; j < 2; ++j) {
    if (!valid[j]) continue;
    const int p = (int)(gm[j] - (int64_t)img * a.HWo);
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      const int nb = acc_channel(n0, t);
      floatx4 v = acc[t][j];
      if (c.bias) v += *(const floatx4*)&c.bias[nb];
      if (c.act == SGR_RESNET_ACT_RELU)
#pragma unroll
        for (int r = 0; r < 4; ++r) v[r] = fmaxf(v[r], 0.f);
      store_out4(c.out, c.out_kind, c.out_stride, v, gm[j], img, p, nb, c.cout, a.HWo);
    }
  }
}

struct StatsArgs {
  const float* raw;
  float* stats;
  int HW, tiles, C, G, cshift;
};

// The statistics of the convolution's epilogue for a map that is already there, grid (tiles, images): one thread per group walks the
// tile's pixels and the group's channels in ascending order.  Not on the backbone's path.
__global__ void __launch_bounds__(kThreads) resnet_stats_kernel(const StatsArgs a) {
  const int img = blockIdx.y, m0 = blockIdx.x * kBM, cpg = 1 << a.cshift, np = min(kBM, a.HW - m0);
  const float* base = a.raw + ((int64_t)img * a.HW + m0) * a.C;
  for (int g = threadIdx.x; g < a.G; g += kThreads) {
    const float sh = base[g * cpg];
    float s1 = 0.f, s2 = 0.f;
    for (int p = 0; p < np; ++p)
      for (int k = 0; k < cpg; ++k) {
        const float d = base[(int64_t)p * a.C + g * cpg + k] - sh;
        s1 += d;
        s2 += d * d;
      }
    *(floatx4*)&a.stats[(((int64_t)img * a.tiles + blockIdx.x) * a.G + g) * 4] = floatx4{(float)(np * cpg), sh, s1, s2};
  }
}

struct NormArgs {
  const float* raw;
  const float* stats;
  const float* gamma;
  const float* beta;
  const half_t* res;
  half_t* out;
  int HW, tiles, C, G, cshift, relu, res_stride, out_stride, pixels;
};

// The second launch of a norm, grid (pixel blocks, images).  Every workgroup first merges the per-tile statistics of its image, one
// statistic per group (merge_tile_stats, sgr_conv_mma.h); then y = (v - mean) * rstd * gamma + beta, + residual, ReLU in fp32, one
// rounding to fp16.  One thread per (pixel, 8 channels).
__global__ void __launch_bounds__(kThreads) resnet_norm_kernel(const NormArgs a) {
  __shared__ double pa[kThreads], pb[kThreads];
  __shared__ float mu[kMaxGroups], rs[kMaxGroups];
  const int tid = threadIdx.x, img = blockIdx.y, C = a.C, G = a.G;
  merge_tile_stats((const floatx4*)a.stats + (int64_t)img * a.tiles * G, a.tiles, G, (double)a.HW * (double)(1 << a.cshift), pa, pb, mu, rs);
  const int chunks = C / 8, p0 = blockIdx.x * a.pixels;
  for (int i = tid; i < a.pixels * chunks; i += kThreads) {
    const int p = p0 + i / chunks, j = i % chunks;
    if (p >= a.HW) break;
    const int64_t m = (int64_t)img * a.HW + p;
    const floatx4 lo = *(const floatx4*)&a.raw[m * C + j * 8], hi = *(const floatx4*)&a.raw[m * C + j * 8 + 4];
    const floatx4 g0 = *(const floatx4*)&a.gamma[j * 8], g1 = *(const floatx4*)&a.gamma[j * 8 + 4];
    const floatx4 b0 = *(const floatx4*)&a.beta[j * 8], b1 = *(const floatx4*)&a.beta[j * 8 + 4];
    float v[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const int g = (j * 8 + k) >> a.cshift;
      v[k] = ((k < 4 ? lo[k] : hi[k - 4]) - mu[g]) * rs[g] * (k < 4 ? g0[k] : g1[k - 4]) + (k < 4 ? b0[k] : b1[k - 4]);
    }
    if (a.res) {
      const half8 x = *(const half8*)&a.res[m * a.res_stride + j * 8];
#pragma unroll
      for (int k = 0; k < 8; ++k) v[k] += (float)x[k];
    }
    half8 o;
#pragma unroll
    for (int k = 0; k < 8; ++k) o[k] = (half_t)(a.relu ? fmaxf(v[k], 0.f) : v[k]);
    *(half8*)&a.out[m * a.out_stride + j * 8] = o;
  }
}

struct PoolArgs {
  const half_t* src;
  half_t* dst;
  int h, w, ho, wo, chunks, pad_top, pad_left;
  int64_t total;                             // n * ho * wo * chunks
};

// One thread per (output pixel, 8 channels): up to 9 16-byte loads, one 16-byte store; taps outside the map count as -inf.
__global__ void __launch_bounds__(kThreads) resnet_pool_kernel(const PoolArgs a) {
  const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i >= a.total) return;
  const int j = (int)(i % a.chunks);
  const int64_t q = i / a.chunks;
  const int ox = (int)(q % a.wo), oy = (int)((q / a.wo) % a.ho);
  const int64_t img = q / ((int64_t)a.wo * a.ho);
  const half_t ninf = (half_t)(-__builtin_inff());
  half8 best = {ninf, ninf, ninf, ninf, ninf, ninf, ninf, ninf};
  for (int dy = 0; dy < 3; ++dy) {
    const int yy = oy * 2 - a.pad_top + dy;
    if ((unsigned)yy >= (unsigned)a.h) continue;
    for (int dx = 0; dx < 3; ++dx) {
      const int xx = ox * 2 - a.pad_left + dx;
      if ((unsigned)xx >= (unsigned)a.w) continue;
      const half8 v = *(const half8*)&a.src[((img * a.h + yy) * a.w + xx) * ((int64_t)a.chunks * 8) + j * 8];
#pragma unroll
      for (int k = 0; k < 8; ++k) best[k] = v[k] > best[k] ? v[k] : best[k];
    }
  }
  *(half8*)&a.dst[q * ((int64_t)a.chunks * 8) + j * 8] = best;
}

inline int pad_before(int i, int k, int s) {            // TF "same": the smaller half of the total goes in front
  const int total = ((i + s - 1) / s - 1) * s + k - i;
  return total > 0 ? total / 2 : 0;
}

// log2 of the channels per group, or -1: groups must divide C into a power of two of at most 64 channels, with at most 256 groups
int group_shift(int C, int groups) {
  if (groups < 1 || groups > kMaxGroups || C % groups) return -1;
  const int cpg = C / groups;
  for (int s = 0; s <= 6; ++s)
    if (cpg == 1 << s) return s;
  return -1;
}

int launch_conv(const SgrResnetConv& c, hipStream_t stream) {
  if (!c.src || !c.weight) return set_error(SGR_ERR_INVALID, "resnet_conv: null argument");
  if (!map_ok(c.n, c.h, c.w) || c.cin < 8 || c.cin % 8 || c.cin > kMaxChannels)
    return set_error(SGR_ERR_INVALID, "resnet_conv: bad sizes (n=%d h=%d w=%d cin=%d); n <= 65535, cin a multiple of 8 up to 1024", c.n, c.h, c.w,
                     c.cin);
  if (c.cout < 16 || c.cout % 16 || c.cout > kMaxChannels)
    return set_error(SGR_ERR_INVALID, "resnet_conv: cout %d is not a multiple of 16 in 16..1024", c.cout);
  if (c.ksize != 1 && c.ksize != 3 && c.ksize != 7) return set_error(SGR_ERR_INVALID, "resnet_conv: kernel size %d is not 1, 3 or 7", c.ksize);
  if (c.stride != 1 && c.stride != 2) return set_error(SGR_ERR_INVALID, "resnet_conv: stride %d is not 1 or 2", c.stride);
  if (c.pad_top < 0 || c.pad_top >= c.ksize || c.pad_left < 0 || c.pad_left >= c.ksize)
    return set_error(SGR_ERR_INVALID, "resnet_conv: padding (%d, %d) outside 0..ksize-1", c.pad_top, c.pad_left);
  // ho is consistent when some padding 0 <= after < ksize gives it: ho = (h + pad_top + after - ksize) / stride + 1
  auto out_ok = [&](int i, int before, int o) {
    if (o < 1) return false;
    const int64_t need = (int64_t)(o - 1) * c.stride + c.ksize - i - before, after = need > 0 ? need : 0;
    return after < c.ksize && -need < c.stride;
  };
  if (!out_ok(c.h, c.pad_top, c.ho) || !out_ok(c.w, c.pad_left, c.wo) || !map_ok(c.n, c.ho, c.wo))
    return set_error(SGR_ERR_INVALID, "resnet_conv: output %d x %d does not follow from a %d x %d map, kernel %d, stride %d, padding (%d, %d)",
                     c.ho, c.wo, c.h, c.w, c.ksize, c.stride, c.pad_top, c.pad_left);
  int k_pad;
  if (int rc = check_conv_operands("resnet_conv", c.src, c.src_stride, c.cin, c.ksize, c.weight, c.weight_elems, c.cout, c.bias, k_pad)) return rc;
  ConvArgs a;
  a.c = c;
  a.HWo = c.ho * c.wo;
  a.k_pad = k_pad;
  a.tiles = tiles_of(a.HWo);
  a.cshift = 0;
  if (c.norm) {
    const int64_t M = (int64_t)c.n * a.HWo;
    if (c.norm != SGR_RESNET_NORM_GROUP) return set_error(SGR_ERR_INVALID, "resnet_conv: unknown norm %d", c.norm);
    a.cshift = group_shift(c.cout, c.groups);
    if (a.cshift < 0 || ((int64_t)a.HWo << a.cshift) < 2)
      return set_error(SGR_ERR_INVALID,
                       "resnet_conv: unsupported groups (%d of %d channels on %d pixels): a power of two of at most 64 channels per group, at "
                       "most 256 groups, at least 2 elements per group", c.groups, c.cout, a.HWo);
    if (!c.raw || !c.stats || !aligned16(c.raw) || !aligned16(c.stats) || c.raw_elems < M * c.cout ||
        c.stats_elems < (int64_t)c.n * a.tiles * c.groups * 4)
      return set_error(SGR_ERR_WORKSPACE, "resnet_conv: a normalised convolution needs raw fp32 [%lld][%d] and stats fp32 [%d][%d][%d][4]",
                       (long long)M, c.cout, c.n, a.tiles, c.groups);
  } else {
    if (c.act != SGR_RESNET_ACT_NONE && c.act != SGR_RESNET_ACT_RELU) return set_error(SGR_ERR_INVALID, "resnet_conv: unknown epilogue %d", c.act);
    if (!c.out || !aligned16(c.out)) return set_error(SGR_ERR_INVALID, "resnet_conv: out must be 16-byte aligned");
    if (c.out_kind < SGR_UPDATE_OUT_CL_F16 || c.out_kind > SGR_UPDATE_OUT_NCHW_F32)
      return set_error(SGR_ERR_INVALID, "resnet_conv: unknown output kind %d", c.out_kind);
    if (c.out_kind <= SGR_UPDATE_OUT_CL_F32 && (c.out_stride < c.cout || c.out_stride % 8))
      return set_error(SGR_ERR_INVALID, "resnet_conv: out_stride %d must be a multiple of 8 and >= cout %d", c.out_stride, c.cout);
  }
  // the widest channel tile that divides cout; a group (a power of two <= 64 that divides cout) then never spans two tiles
  const int bn = c.cout % 64 == 0 ? 64 : c.cout % 32 == 0 ? 32 : 16;
  const dim3 grid((unsigned)a.tiles, (unsigned)(c.cout / bn), (unsigned)c.n), block(kThreads);
  dispatch_conv<16, 32, 64>(c.ksize, bn, [&](auto ks, auto bnc) {
    hipLaunchKernelGGL((resnet_conv_kernel<decltype(ks)::value, decltype(bnc)::value>), grid, block, 0, stream, a);
  });
  return launched("resnet_conv");
}

// pixels of one workgroup of the norm launch: about 16384 elements, and at least as many pixels as the image has tiles, so that the
// merge every workgroup repeats stays below the map it normalises
inline int norm_pixels(int hw, int C) {
  const int by_size = 16384 / C, tiles = tiles_of(hw);
  return by_size > tiles ? by_size : tiles;
}

int launch_norm(const SgrResnetNorm& g, hipStream_t stream) {
  if (!g.raw || !g.stats || !g.gamma || !g.beta || !g.out) return set_error(SGR_ERR_INVALID, "resnet_groupnorm: null argument");
  if (g.n < 1 || g.n > 65535 || g.hw < 1 || g.hw > 0x7fffffff - kBM || g.cout < 8 || g.cout % 8 || g.cout > kMaxChannels)
    return set_error(SGR_ERR_INVALID, "resnet_groupnorm: bad sizes (n=%d hw=%d cout=%d)", g.n, g.hw, g.cout);
  const int cshift = group_shift(g.cout, g.groups);
  if (cshift < 0 || ((int64_t)g.hw << cshift) < 2)
    return set_error(SGR_ERR_INVALID,
                     "resnet_groupnorm: unsupported groups (%d of %d channels on %d pixels): a power of two of at most 64 channels per group, at "
                     "most 256 groups, at least 2 elements per group", g.groups, g.cout, g.hw);
  if (!aligned16(g.raw) || !aligned16(g.stats) || !aligned16(g.gamma) || !aligned16(g.beta) || !aligned16(g.out) || g.out_stride < g.cout ||
      g.out_stride % 8)
    return set_error(SGR_ERR_INVALID, "resnet_groupnorm: 16-byte aligned bases and an out_stride (%d) that is a multiple of 8 and >= %d",
                     g.out_stride, g.cout);
  if (g.residual && (g.residual_stride < g.cout || g.residual_stride % 8 || !aligned16(g.residual)))
    return set_error(SGR_ERR_INVALID, "resnet_groupnorm: residual needs a 16-byte aligned base and a stride (%d) that is a multiple of 8 and >= %d",
                     g.residual_stride, g.cout);
  NormArgs a;
  a.raw = g.raw, a.stats = g.stats, a.gamma = g.gamma, a.beta = g.beta, a.res = (const half_t*)g.residual, a.out = (half_t*)g.out;
  a.HW = g.hw, a.tiles = tiles_of(g.hw), a.C = g.cout, a.G = g.groups, a.cshift = cshift, a.relu = g.relu != 0;
  a.res_stride = g.residual_stride, a.out_stride = g.out_stride, a.pixels = norm_pixels(g.hw, g.cout);
  const dim3 grid((unsigned)((g.hw + a.pixels - 1) / a.pixels), (unsigned)g.n);
  hipLaunchKernelGGL(resnet_norm_kernel, grid, dim3(kThreads), 0, stream, a);
  return launched("resnet_groupnorm");
}

int launch_pool(const half_t* src, int n, int h, int w, int C, half_t* dst, hipStream_t stream) {
  PoolArgs a;
  a.src = src, a.dst = dst, a.h = h, a.w = w, a.ho = (h + 1) / 2, a.wo = (w + 1) / 2, a.chunks = C / 8;
  a.pad_top = pad_before(h, 3, 2), a.pad_left = pad_before(w, 3, 2);
  a.total = (int64_t)n * a.ho * a.wo * a.chunks;
  const int64_t blocks = (a.total + kThreads - 1) / kThreads;
  if (blocks > 0x7fffffff) return set_error(SGR_ERR_INVALID, "resnet_maxpool: the map is too large for one launch");
  hipLaunchKernelGGL(resnet_pool_kernel, dim3((unsigned)blocks), dim3(kThreads), 0, stream, a);
  return launched("resnet_maxpool");
}

bool widths_ok(int stem, const int* chs) {
  if (stem < 16 || stem % 16 || stem > kMaxChannels) return false;
  for (int s = 0; s < 3; ++s)
    if (chs[s] < 64 || chs[s] % 64 || chs[s] > kMaxChannels) return false;
  return true;
}
bool sizes_ok(int n, int H, int W, int stem, const int* chs) {
  return map_ok(n, H, W) && H % 32 == 0 && W % 32 == 0 && (int64_t)n * H * W <= ((int64_t)1 << 40) && widths_ok(stem, chs);
}

// The maps of a call: the packed image, four rotating activation buffers of the largest map, the raw sums and the statistics.
struct Plan {
  half_t *xin, *act[4];
  float *raw, *stats;
  int64_t raw_elems, stats_elems;
  size_t bytes;
};
Plan carve(void* base, int n, int H, int W, int stem, const int* chs) {
  Plan s;
  Carver cv{base};
  // (pixels, widest map) per level: the stem at 1/2; the pool, stage 0 and the first convolution of stage 1 at 1/4; and so on
  const int64_t hw[4] = {(int64_t)(H / 2) * (W / 2), (int64_t)(H / 4) * (W / 4), (int64_t)(H / 8) * (W / 8), (int64_t)(H / 16) * (W / 16)};
  auto mx = [](int64_t x, int64_t y) { return x > y ? x : y; };
  const int64_t wide[4] = {stem, mx(mx(stem, chs[0]), chs[1] / 4), mx(chs[1], chs[2] / 4), chs[2]};
  int64_t act_elems = 0;
  s.stats_elems = 0;
  for (int l = 0; l < 4; ++l) {
    act_elems = act_elems > n * hw[l] * wide[l] ? act_elems : n * hw[l] * wide[l];
    const int64_t st = (int64_t)n * tiles_of(hw[l]) * kMaxGroups * 4;
    s.stats_elems = s.stats_elems > st ? s.stats_elems : st;
  }
  s.raw_elems = act_elems;
  s.xin = (half_t*)cv.take((size_t)n * H * W * kInPad * 2);
  for (int i = 0; i < 4; ++i) s.act[i] = (half_t*)cv.take((size_t)act_elems * 2);
  s.raw = (float*)cv.take((size_t)s.raw_elems * 4);
  s.stats = (float*)cv.take((size_t)s.stats_elems * 4);
  s.bytes = cv.off;
  return s;
}

}  // namespace
}  // namespace sgr

using namespace sgr;

extern "C" {

size_t sgr_resnet_scratch_bytes(int32_t n, int32_t H, int32_t W, int32_t stem_chs, int32_t chs0, int32_t chs1, int32_t chs2) {
  const int chs[3] = {chs0, chs1, chs2};
  if (!sizes_ok(n, H, W, stem_chs, chs)) return 0;
  return carve(nullptr, n, H, W, stem_chs, chs).bytes;
}

int sgr_resnet_conv(const SgrResnetConv* conv, void* stream) {
  if (!conv) return set_error(SGR_ERR_INVALID, "resnet_conv: null argument");
  return launch_conv(*conv, (hipStream_t)stream);
}

int sgr_resnet_stats(const float* raw, int32_t n, int32_t hw, int32_t cout, int32_t groups, float* stats, void* stream) {
  if (!raw || !stats || !aligned16(raw) || !aligned16(stats)) return set_error(SGR_ERR_INVALID, "resnet_stats: null or unaligned argument");
  if (n < 1 || n > 65535 || hw < 1 || hw > 0x7fffffff - kBM || cout < 1 || cout > kMaxChannels)
    return set_error(SGR_ERR_INVALID, "resnet_stats: bad sizes (n=%d hw=%d cout=%d)", n, hw, cout);
  const int cshift = group_shift(cout, groups);
  if (cshift < 0 || ((int64_t)hw << cshift) < 2)
    return set_error(SGR_ERR_INVALID,
                     "resnet_stats: unsupported groups (%d of %d channels on %d pixels): a power of two of at most 64 channels per group, at most "
                     "256 groups, at least 2 elements per group", groups, cout, hw);
  StatsArgs a;
  a.raw = raw, a.stats = stats, a.HW = hw, a.tiles = tiles_of(hw), a.C = cout, a.G = groups, a.cshift = cshift;
  hipLaunchKernelGGL(resnet_stats_kernel, dim3((unsigned)a.tiles, (unsigned)n), dim3(kThreads), 0, (hipStream_t)stream, a);
  return launched("resnet_stats");
}

int sgr_resnet_groupnorm(const SgrResnetNorm* norm, void* stream) {
  if (!norm) return set_error(SGR_ERR_INVALID, "resnet_groupnorm: null argument");
  return launch_norm(*norm, (hipStream_t)stream);
}

int sgr_resnet_maxpool(const void* src, int32_t n, int32_t h, int32_t w, int32_t channels, void* dst, void* stream) {
  if (!src || !dst || !aligned16(src) || !aligned16(dst)) return set_error(SGR_ERR_INVALID, "resnet_maxpool: null or unaligned argument");
  if (!map_ok(n, h, w) || channels < 8 || channels % 8 || channels > kMaxChannels)
    return set_error(SGR_ERR_INVALID, "resnet_maxpool: bad sizes (n=%d h=%d w=%d channels=%d); channels a multiple of 8 up to 1024", n, h, w, channels);
  return launch_pool((const half_t*)src, n, h, w, channels, (half_t*)dst, (hipStream_t)stream);
}

int sgr_resnet_forward(const SgrResnetWeights* wt, const SgrResnetCall* call, void* scratch, size_t scratch_bytes, void* stream_) {
  if (!wt || !call || !scratch || !wt->layers) return set_error(SGR_ERR_INVALID, "resnet_forward: null argument");
  const int n = call->n, H = call->H, W = call->W, stem = wt->stem_chs, G = wt->groups;
  if (!sizes_ok(n, H, W, stem, wt->stage_chs))
    return set_error(SGR_ERR_INVALID, "resnet_forward: unsupported sizes (n=%d H=%d W=%d stem=%d stages=%d,%d,%d); H and W multiples of 32", n, H, W,
                     stem, wt->stage_chs[0], wt->stage_chs[1], wt->stage_chs[2]);
  int layers = 1;
  for (int s = 0; s < 3; ++s) {
    if (wt->stage_blocks[s] < 1 || wt->stage_blocks[s] > 1024) return set_error(SGR_ERR_INVALID, "resnet_forward: a stage has 1..1024 blocks");
    layers += 3 * wt->stage_blocks[s] + 1;
    if (group_shift(wt->stage_chs[s], G) < 0 || group_shift(wt->stage_chs[s] / 4, G) < 0)
      return set_error(SGR_ERR_INVALID, "resnet_forward: %d groups do not split %d or %d channels", G, wt->stage_chs[s], wt->stage_chs[s] / 4);
  }
  if (group_shift(stem, G) < 0) return set_error(SGR_ERR_INVALID, "resnet_forward: %d groups do not split the stem's %d channels", G, stem);
  if (wt->num_layers != layers) return set_error(SGR_ERR_INVALID, "resnet_forward: %d layers given, the network has %d", wt->num_layers, layers);
  for (int i = 0; i < layers; ++i)
    if (!wt->layers[i].weight || !wt->layers[i].gamma || !wt->layers[i].beta) return set_error(SGR_ERR_INVALID, "resnet_forward: null weights");
  if (!call->images.data || !call->l1 || !call->l2 || !call->l3 || !aligned16(call->l1) || !aligned16(call->l2) || !aligned16(call->l3))
    return set_error(SGR_ERR_INVALID, "resnet_forward: null or unaligned tensor");
  const Plan s = carve(scratch, n, H, W, stem, wt->stage_chs);
  if (scratch_bytes < s.bytes || !aligned16(scratch))
    return set_error(SGR_ERR_WORKSPACE, "resnet_forward: scratch of %zu bytes, need %zu (16-byte aligned)", scratch_bytes, s.bytes);
  hipStream_t stream = (hipStream_t)stream_;
  int rc = SGR_OK;
  LaunchRange on{call->first_launch, call->last_launch};
  // one convolution with TF "same" padding and its norm: two launches
  auto conv = [&](int layer, const half_t* src, int cin, int h, int w, int ks, int stride, int cout, int relu, const half_t* res,
                  half_t* out) -> int {
    const SgrResnetLayer& L = wt->layers[layer];
    SgrResnetConv c = {};
    c.src = src, c.src_stride = cin, c.cin = cin, c.ksize = ks, c.stride = stride, c.n = n, c.h = h, c.w = w;
    c.pad_top = pad_before(h, ks, stride), c.pad_left = pad_before(w, ks, stride), c.ho = (h + stride - 1) / stride, c.wo = (w + stride - 1) / stride;
    c.weight = L.weight, c.weight_elems = L.weight_elems, c.cout = cout, c.norm = SGR_RESNET_NORM_GROUP, c.groups = G;
    c.raw = s.raw, c.raw_elems = s.raw_elems, c.stats = s.stats, c.stats_elems = s.stats_elems;
    if (on() && (rc = launch_conv(c, stream))) return rc;
    SgrResnetNorm g = {};
    g.raw = s.raw, g.stats = s.stats, g.n = n, g.hw = c.ho * c.wo, g.cout = cout, g.groups = G, g.relu = relu, g.gamma = L.gamma, g.beta = L.beta;
    g.residual = res, g.residual_stride = cout, g.out = out, g.out_stride = cout;
    if (on() && (rc = launch_norm(g, stream))) return rc;
    return SGR_OK;
  };
  if (on() && (rc = sgr_encoder_pack(&call->images, n, H, W, call->normalize ? call->mean : nullptr, call->normalize ? call->std_ : nullptr, s.xin,
                                     stream_)))
    return rc;
  if ((rc = conv(0, s.xin, kInPad, H, W, 7, 2, stem, 1, nullptr, s.act[0]))) return rc;
  if (on() && (rc = launch_pool(s.act[0], n, H / 2, W / 2, stem, s.act[1], stream))) return rc;
  const half_t* cur = s.act[1];
  half_t* const outs[3] = {(half_t*)call->l1, (half_t*)call->l2, (half_t*)call->l3};
  int layer = 1, cin = stem, h = H / 4, w = W / 4;
  for (int st = 0; st < 3; ++st) {
    const int cout = wt->stage_chs[st], mid = cout / 4;
    for (int b = 0; b < wt->stage_blocks[st]; ++b) {
      // y = relu(gn(conv1(x))), y = relu(gn(conv2(y))) in place of the first, out = relu(gn(conv3(y)) + x'), x' = x or gn(downsample(x))
      half_t* free_[3];
      for (int i = 0, k = 0; i < 4 && k < 3; ++i)
        if (s.act[i] != cur) free_[k++] = s.act[i];
      half_t *y = free_[0], *xd = free_[1];
      half_t* o = b == wt->stage_blocks[st] - 1 ? outs[st] : free_[2];
      const int stride = st > 0 && b == 0 ? 2 : 1, ho = h / stride, wo = w / stride;
      if ((rc = conv(layer, cur, cin, h, w, 1, 1, mid, 1, nullptr, y))) return rc;
      const half_t* skip = cur;
      if (b == 0) {
        if ((rc = conv(layer + 3, cur, cin, h, w, 1, stride, cout, 0, nullptr, xd))) return rc;
        skip = xd;
      }
      if ((rc = conv(layer + 1, y, mid, h, w, 3, stride, mid, 1, nullptr, y))) return rc;
      if ((rc = conv(layer + 2, y, mid, ho, wo, 1, 1, cout, 1, skip, o))) return rc;
      layer += b == 0 ? 4 : 3;
      cur = o, cin = cout, h = ho, w = wo;
    }
  }
  return SGR_OK;
}

}  // extern "C"
