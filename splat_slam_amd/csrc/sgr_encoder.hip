// The tracker's feature and context encoders (BasicEncoder of the reference's thirdparty/glorie_slam/modules/droid_net/extractor.py: fnet with
// InstanceNorm2d, cnet without a norm), inference only.
//   sgr_encoder_pack      [n,3,H,W] (fp16 or fp32, any strides), optionally (x - mean[c]) / std[c] -> channels-last fp16, 8 channels per pixel
//   sgr_encoder_conv      one implicit-GEMM convolution (1x1, 3x3, 7x7; zero padding (k-1)/2; stride 1 or 2) on mfma_f32_16x16x32_f16 with a
//                         fused epilogue, or, with an instance norm, the raw fp32 sums with per-tile statistics followed by one apply launch
//   sgr_encoder_forward   a whole encoder: 32 (fnet) or 17 (cnet) stream-ordered launches, no host synchronisation
// Layouts, the launch list, the rounding points and the statistics scheme are described in DESIGN.md section 3, "Encoders".  The GEMM is
// the shared tile of sgr_conv_mma.h; here a workgroup's 128 output pixels belong to one image (blockIdx.z), the gather takes a stride, and
// output channels come in tiles of 32 or 64.  Every sum has a fixed order: no atomics, bitwise reproducible, and image i of a batch gives
// the bits of that image alone.
#include <cstdint>

#include "sgr_conv_mma.h"

namespace sgr {
namespace {

constexpr int kInPad = 8;                   // the 3 image channels padded to one 16-byte chunk
constexpr int kApplyPixels = 512;           // pixels of one workgroup of the apply launch
constexpr int kLayers = SGR_ENCODER_LAYERS;

struct ConvArgs {
  SgrEncoderConv c;
  int ho, wo, HWo, k_pad, tiles;
};

// The shared tile on the kBM output pixels m0 .. of image blockIdx.z: zero padding KS / 2, stride c.stride.
template <int KS, int BN>
__global__ void __launch_bounds__(kThreads) enc_conv_kernel(const ConvArgs a) {
  constexpr int NT = BN / 16;
  __shared__ __attribute__((aligned(16))) half_t Xs[kBM * kRow];
  __shared__ __attribute__((aligned(16))) half_t Ws[BN * kRow];
  __shared__ float red[2][4][BN];
  __shared__ float shift[BN];
  const SgrEncoderConv& c = a.c;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int img = blockIdx.z, m0 = blockIdx.x * kBM, n0 = blockIdx.y * BN;
  const half_t* src = (const half_t*)c.src + (int64_t)img * c.h * c.w * c.src_stride;

  ConvWindow win;
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int m = m0 + (tid >> 2) + 64 * i;
    const bool pv = m < a.HWo;
    const int mm = pv ? m : 0;
    win.row(i, pv, mm, mm / a.wo, a.wo, c.stride, 0, 0);
  }
  // the padding is a constant here and comes off the tap, not off the origin: the order of the sum this kernel was compiled with
  auto gather = [&](int i, bool tv, int ty, int tx, int ch) {
    return win.chunk(src, c.h, c.w, c.src_stride, i, tv, ty - KS / 2, tx - KS / 2, ch);
  };
  floatx4 acc[NT][2];
  conv_mma_mainloop<KS, BN>(Xs, Ws, (const half_t*)c.weight, n0, a.k_pad, c.cin, gather, acc);

  // acc[t][j] holds channels acc_channel(n0, t) .. + 3 of pixel acc_pixel(j) of this image
  bool valid[2];
  int64_t gm[2];                                             // pixel index over the whole batch
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    // acc_pixel(j), spelled out: this kernel also indexes red by wave, and through the function the compiler folds that shared shift
    // another way
    const int m = m0 + wave * 32 + j * 16 + (lane & 15);
    valid[j] = m < a.HWo;
    gm[j] = (int64_t)img * a.HWo + m;
  }

  if (c.norm) {
    // The bias of a normalised convolution cancels: the statistics and the stored sums are those of the bias-free accumulator.  Per
    // (tile, channel): the count, a shift s = the tile mean rounded to fp32, S1 = sum (v - s) and S2 = sum (v - s)^2.  The 16 pixel
    // lanes are summed by a butterfly, the 2 x 4 partials of a channel in the order (j, wave).
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      if (!valid[j]) continue;
#pragma unroll
      for (int t = 0; t < NT; ++t) *(floatx4*)&c.raw[acc_channel(gm[j] * c.cout + n0, t)] = acc[t][j];
    }
    const float cnt = (float)min(kBM, a.HWo - m0);
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        float s = (valid[0] ? acc[t][0][r] : 0.f) + (valid[1] ? acc[t][1][r] : 0.f);
#pragma unroll
        for (int d = 1; d < 16; d <<= 1) s += __shfl_xor(s, d);
        if ((lane & 15) == 0) red[0][wave][acc_channel(0, t) + r] = s;
      }
    __syncthreads();
    if (tid < BN) shift[tid] = (((red[0][0][tid] + red[0][1][tid]) + red[0][2][tid]) + red[0][3][tid]) / cnt;
    __syncthreads();
    tile_shifted_sums<BN>(acc, valid, [&](int n) { return shift[n]; }, red);
    __syncthreads();
    if (tid < BN) {
      const float s1 = ((red[0][0][tid] + red[0][1][tid]) + red[0][2][tid]) + red[0][3][tid];
      const float s2 = ((red[1][0][tid] + red[1][1][tid]) + red[1][2][tid]) + red[1][3][tid];
      *(floatx4*)&c.stats[(((int64_t)img * a.tiles + blockIdx.x) * c.cout + n0 + tid) * 4] = floatx4{cnt, shift[tid], s1, s2};
    }
    return;
  }

  const half_t* res = (const half_t*)c.residual;
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    if (!valid[j]) continue;
    const int p = (int)(gm[j] - (int64_t)img * a.HWo);
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      const int nb = acc_channel(n0, t);
      floatx4 v = acc[t][j] + *(const floatx4*)&c.bias[nb];
      if (c.act == SGR_ENCODER_ACT_SPLIT) {                  // cout = 256: tanh(net) | relu(inp), two NCHW fp16 tensors
        const bool lo = nb < 128;
        half_t* dst = (half_t*)(lo ? c.out : c.out2) + ((int64_t)img * 128 + (lo ? nb : nb - 128)) * a.HWo + p;
#pragma unroll
        for (int r = 0; r < 4; ++r) dst[(int64_t)r * a.HWo] = (half_t)(lo ? tanhf(v[r]) : fmaxf(v[r], 0.f));
        continue;
      }
      if (c.act == SGR_ENCODER_ACT_RELU)
#pragma unroll
        for (int r = 0; r < 4; ++r) v[r] = fmaxf(v[r], 0.f);
      if (res) {
        const half4 x = *(const half4*)&res[gm[j] * c.residual_stride + nb];
#pragma unroll
        for (int r = 0; r < 4; ++r) v[r] = fmaxf((float)x[r] + v[r], 0.f);
      }
      store_out4(c.out, c.out_kind, c.out_stride, v, gm[j], img, p, nb, c.cout, a.HWo);
    }
  }
}

struct ApplyArgs {
  const float* raw;
  const float* stats;
  const half_t* res;
  void* out;
  int HWo, tiles, C, relu, res_stride, out_f32, out_stride;
};

// The second launch of a normalised convolution, grid (pixel blocks, images).  Every workgroup first merges the per-tile statistics of
// its image, one statistic per channel (merge_tile_stats, sgr_conv_mma.h); then y = (v - mean) * rstd, ReLU, + residual, ReLU in fp32,
// one rounding to the output.  One thread per (pixel, 8 channels).
__global__ void __launch_bounds__(kThreads) enc_apply_kernel(const ApplyArgs a) {
  __shared__ double pa[kThreads], pb[kThreads];
  __shared__ float mu[128], rs[128];
  const int tid = threadIdx.x, img = blockIdx.y, C = a.C;
  merge_tile_stats((const floatx4*)a.stats + (int64_t)img * a.tiles * C, a.tiles, C, (double)a.HWo, pa, pb, mu, rs);
  const int chunks = C / 8, p0 = blockIdx.x * kApplyPixels;
  for (int i = tid; i < kApplyPixels * chunks; i += kThreads) {
    const int p = p0 + i / chunks, j = i % chunks;
    if (p >= a.HWo) break;
    const int64_t m = (int64_t)img * a.HWo + p;
    const floatx4 lo = *(const floatx4*)&a.raw[m * C + j * 8], hi = *(const floatx4*)&a.raw[m * C + j * 8 + 4];
    float v[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      v[k] = ((k < 4 ? lo[k] : hi[k - 4]) - mu[j * 8 + k]) * rs[j * 8 + k];
      if (a.relu) v[k] = fmaxf(v[k], 0.f);
    }
    if (a.res) {
      const half8 x = *(const half8*)&a.res[m * a.res_stride + j * 8];
#pragma unroll
      for (int k = 0; k < 8; ++k) v[k] = fmaxf((float)x[k] + v[k], 0.f);
    }
    if (a.out_f32) {
      float* o = (float*)a.out + m * a.out_stride + j * 8;
      *(floatx4*)o = floatx4{v[0], v[1], v[2], v[3]};
      *(floatx4*)(o + 4) = floatx4{v[4], v[5], v[6], v[7]};
    } else {
      half8 o;
#pragma unroll
      for (int k = 0; k < 8; ++k) o[k] = (half_t)v[k];
      *(half8*)&((half_t*)a.out)[m * a.out_stride + j * 8] = o;
    }
  }
}

struct PackArgs {
  SgrUpdateTensor src;
  float mean[3], inv_on, std_[3];
  int HW, w;
};

// One thread per pixel: three strided reads, one 16-byte store (channels 3..7 zero).  (x - mean) / std is the fp32 expression torch
// evaluates for sub then div, so normalising here or beforehand gives the same fp16 values.
__global__ void __launch_bounds__(kThreads) enc_pack_kernel(const PackArgs a, half_t* __restrict__ dst) {
  const int p = blockIdx.x * kThreads + threadIdx.x, img = blockIdx.y;
  if (p >= a.HW) return;
  const int y = p / a.w, x = p - y * a.w;
  const int64_t base = img * a.src.stride[0] + y * a.src.stride[2] + x * a.src.stride[3];
  half8 v = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
  for (int ch = 0; ch < 3; ++ch) {
    const int64_t o = base + ch * a.src.stride[1];
    float f = a.src.dtype == SGR_UPDATE_F16 ? (float)((const half_t*)a.src.data)[o] : ((const float*)a.src.data)[o];
    if (a.inv_on != 0.f) f = (f - a.mean[ch]) / a.std_[ch];
    v[ch] = (half_t)f;
  }
  *(half8*)&dst[((int64_t)img * a.HW + p) * kInPad] = v;
}

inline int out_size(int v, int stride) { return (v - 1) / stride + 1; }

int launch_conv(const SgrEncoderConv& c, hipStream_t stream) {
  if (!c.src || !c.weight || !c.bias) return set_error(SGR_ERR_INVALID, "encoder_conv: null argument");
  if (!map_ok(c.n, c.h, c.w) || c.cin < 8 || c.cin % 8)
    return set_error(SGR_ERR_INVALID, "encoder_conv: bad sizes (n=%d h=%d w=%d cin=%d); n <= 65535, cin a positive multiple of 8", c.n, c.h, c.w,
                     c.cin);
  if (c.cout != 32 && c.cout != 64 && c.cout != 128 && c.cout != 256)
    return set_error(SGR_ERR_INVALID, "encoder_conv: cout %d is not 32, 64, 128 or 256", c.cout);
  if (c.ksize != 1 && c.ksize != 3 && c.ksize != 7) return set_error(SGR_ERR_INVALID, "encoder_conv: kernel size %d is not 1, 3 or 7", c.ksize);
  if (c.stride != 1 && c.stride != 2) return set_error(SGR_ERR_INVALID, "encoder_conv: stride %d is not 1 or 2", c.stride);
  int k_pad;
  if (int rc = check_conv_operands("encoder_conv", c.src, c.src_stride, c.cin, c.ksize, c.weight, c.weight_elems, c.cout, c.bias, k_pad)) return rc;
  if (c.act < SGR_ENCODER_ACT_NONE || c.act > SGR_ENCODER_ACT_SPLIT) return set_error(SGR_ERR_INVALID, "encoder_conv: unknown epilogue %d", c.act);
  if (c.residual && (c.residual_stride < c.cout || c.residual_stride % 8 || !aligned16(c.residual)))
    return set_error(SGR_ERR_INVALID, "encoder_conv: residual needs a 16-byte aligned base and a stride (%d) that is a multiple of 8 and >= %d",
                     c.residual_stride, c.cout);
  if (!c.out || !aligned16(c.out)) return set_error(SGR_ERR_INVALID, "encoder_conv: out must be 16-byte aligned");
  ConvArgs a;
  a.c = c;
  a.ho = out_size(c.h, c.stride), a.wo = out_size(c.w, c.stride);
  a.HWo = a.ho * a.wo;
  a.k_pad = k_pad;
  a.tiles = tiles_of(a.HWo);
  if (c.act == SGR_ENCODER_ACT_SPLIT) {
    if (c.cout != 256 || c.norm || c.residual || !c.out2)
      return set_error(SGR_ERR_INVALID, "encoder_conv: the tanh | relu split needs cout = 256, out2, no norm and no residual");
  } else {
    if (c.out_kind < SGR_UPDATE_OUT_CL_F16 || c.out_kind > SGR_UPDATE_OUT_NCHW_F32)
      return set_error(SGR_ERR_INVALID, "encoder_conv: unknown output kind %d", c.out_kind);
    if (c.out_kind <= SGR_UPDATE_OUT_CL_F32 && (c.out_stride < c.cout || c.out_stride % 8))
      return set_error(SGR_ERR_INVALID, "encoder_conv: out_stride %d must be a multiple of 8 and >= cout %d", c.out_stride, c.cout);
  }
  if (c.norm) {
    const int64_t M = (int64_t)c.n * a.HWo;
    if (c.norm != SGR_ENCODER_NORM_INSTANCE || c.cout > 128 || c.out_kind > SGR_UPDATE_OUT_CL_F32)
      return set_error(SGR_ERR_INVALID, "encoder_conv: a normalised convolution has cout <= 128 and a channels-last output");
    if (!c.raw || !c.stats || !aligned16(c.raw) || !aligned16(c.stats) || c.raw_elems < M * c.cout ||
        c.stats_elems < (int64_t)c.n * a.tiles * c.cout * 4)
      return set_error(SGR_ERR_WORKSPACE, "encoder_conv: a normalised convolution needs raw fp32 [%lld][%d] and stats fp32 [%d][%d][%d][4]",
                       (long long)M, c.cout, c.n, a.tiles, c.cout);
  }
  const int bn = c.cout == 32 ? 32 : 64;
  const dim3 grid((unsigned)a.tiles, (unsigned)(c.cout / bn), (unsigned)c.n), block(kThreads);
  dispatch_conv<32, 64>(c.ksize, bn, [&](auto ks, auto bnc) {
    hipLaunchKernelGGL((enc_conv_kernel<decltype(ks)::value, decltype(bnc)::value>), grid, block, 0, stream, a);
  });
  return launched("encoder_conv");
}

// (the arguments were validated by launch_conv of the same record)
int launch_apply(const SgrEncoderConv& c, hipStream_t stream) {
  ApplyArgs a;
  a.raw = c.raw, a.stats = c.stats, a.res = (const half_t*)c.residual, a.out = c.out;
  a.HWo = out_size(c.h, c.stride) * out_size(c.w, c.stride);
  a.tiles = tiles_of(a.HWo);
  a.C = c.cout, a.relu = c.act == SGR_ENCODER_ACT_RELU, a.res_stride = c.residual_stride;
  a.out_f32 = c.out_kind == SGR_UPDATE_OUT_CL_F32, a.out_stride = c.out_stride;
  const dim3 grid((unsigned)((a.HWo + kApplyPixels - 1) / kApplyPixels), (unsigned)c.n);
  hipLaunchKernelGGL(enc_apply_kernel, grid, dim3(kThreads), 0, stream, a);
  return launched("encoder_conv: apply");
}

int launch_pack(const SgrUpdateTensor& src, int n, int H, int W, const float* mean, const float* std_, half_t* dst, hipStream_t stream) {
  PackArgs a;
  a.src = src;
  a.inv_on = mean ? 1.f : 0.f;
  for (int i = 0; i < 3; ++i) a.mean[i] = mean ? mean[i] : 0.f, a.std_[i] = mean ? std_[i] : 1.f;
  a.HW = H * W, a.w = W;
  hipLaunchKernelGGL(enc_pack_kernel, dim3((unsigned)((a.HW + kThreads - 1) / kThreads), (unsigned)n), dim3(kThreads), 0, stream, a, dst);
  return launched("encoder_pack");
}

// The maps of a call: level 0 the image, level 1 after the stem (32 channels), 2 after layer2 (64), 3 after layer3 (128).
struct Plan {
  int h[4], w[4];
  half_t *xin, *act[4];
  float *raw, *stats;
  int64_t raw_elems, stats_elems;
  size_t bytes;
};
Plan carve(void* base, int n, int H, int W, bool norm) {
  Plan s;
  s.h[0] = H, s.w[0] = W;
  for (int l = 1; l < 4; ++l) s.h[l] = out_size(s.h[l - 1], 2), s.w[l] = out_size(s.w[l - 1], 2);
  Carver cv{base};
  int64_t act_elems = 0;
  s.raw_elems = s.stats_elems = 0;
  for (int l = 1; l < 4; ++l) {
    const int64_t hw = (int64_t)s.h[l] * s.w[l], ch = 16 << l;
    act_elems = act_elems > n * hw * ch ? act_elems : n * hw * ch;
    const int64_t st = (int64_t)n * tiles_of(hw) * ch * 4;
    s.stats_elems = s.stats_elems > st ? s.stats_elems : st;
  }
  s.raw_elems = act_elems;
  s.xin = (half_t*)cv.take((size_t)n * H * W * kInPad * 2);
  for (int i = 0; i < 4; ++i) s.act[i] = (half_t*)cv.take((size_t)act_elems * 2);
  s.raw = (float*)cv.take(norm ? (size_t)s.raw_elems * 4 : 0);
  s.stats = (float*)cv.take(norm ? (size_t)s.stats_elems * 4 : 0);
  s.bytes = cv.off;
  return s;
}

bool sizes_ok(int n, int H, int W, int out_dim, int norm) {
  if (!map_ok(n, H, W) || (out_dim != 128 && out_dim != 256) || (norm != SGR_ENCODER_NORM_NONE && norm != SGR_ENCODER_NORM_INSTANCE)) return false;
  if ((int64_t)n * H * W > ((int64_t)1 << 40)) return false;
  const int h3 = out_size(out_size(out_size(H, 2), 2), 2), w3 = out_size(out_size(out_size(W, 2), 2), 2);
  return !norm || (int64_t)h3 * w3 > 1;             // an instance norm over one element is undefined (torch raises as well)
}

}  // namespace
}  // namespace sgr

using namespace sgr;

extern "C" {

size_t sgr_encoder_scratch_bytes(int32_t n, int32_t H, int32_t W, int32_t out_dim, int32_t norm) {
  if (!sizes_ok(n, H, W, out_dim, norm)) return 0;
  return carve(nullptr, n, H, W, norm != 0).bytes;
}

int sgr_encoder_pack(const SgrUpdateTensor* src, int32_t n, int32_t H, int32_t W, const float* mean, const float* std_, void* dst, void* stream) {
  if (!src || !src->data || !dst || !aligned16(dst)) return set_error(SGR_ERR_INVALID, "encoder_pack: null or unaligned argument");
  if (!map_ok(n, H, W)) return set_error(SGR_ERR_INVALID, "encoder_pack: bad sizes (n=%d H=%d W=%d)", n, H, W);
  if (src->dtype != SGR_UPDATE_F16 && src->dtype != SGR_UPDATE_F32) return set_error(SGR_ERR_INVALID, "encoder_pack: unknown dtype");
  if ((mean != nullptr) != (std_ != nullptr)) return set_error(SGR_ERR_INVALID, "encoder_pack: mean and std come together");
  return launch_pack(*src, n, H, W, mean, std_, (half_t*)dst, (hipStream_t)stream);
}

int sgr_encoder_conv(const SgrEncoderConv* conv, void* stream) {
  if (!conv) return set_error(SGR_ERR_INVALID, "encoder_conv: null argument");
  const int rc = launch_conv(*conv, (hipStream_t)stream);
  if (rc != SGR_OK || !conv->norm) return rc;
  return launch_apply(*conv, (hipStream_t)stream);
}

int sgr_encoder_forward(const SgrEncoderWeights* wt, const SgrEncoderCall* call, void* scratch, size_t scratch_bytes, void* stream_) {
  if (!wt || !call || !scratch) return set_error(SGR_ERR_INVALID, "encoder_forward: null argument");
  const int n = call->n, H = call->H, W = call->W, norm = wt->norm, out_dim = wt->out_dim;
  if (!sizes_ok(n, H, W, out_dim, norm))
    return set_error(SGR_ERR_INVALID, "encoder_forward: unsupported sizes (n=%d H=%d W=%d out_dim=%d norm=%d)", n, H, W, out_dim, norm);
  if (!call->images.data || !call->out) return set_error(SGR_ERR_INVALID, "encoder_forward: null tensor");
  if (call->images.dtype != SGR_UPDATE_F16 && call->images.dtype != SGR_UPDATE_F32) return set_error(SGR_ERR_INVALID, "encoder_forward: unknown dtype");
  if (call->split && (out_dim != 256 || !call->out2)) return set_error(SGR_ERR_INVALID, "encoder_forward: the split output needs out_dim = 256 and out2");
  for (int i = 0; i < kLayers; ++i)
    if (!wt->layer[i].weight || !wt->layer[i].bias) return set_error(SGR_ERR_INVALID, "encoder_forward: null weights");
  const Plan s = carve(scratch, n, H, W, norm != 0);
  if (scratch_bytes < s.bytes || !aligned16(scratch))
    return set_error(SGR_ERR_WORKSPACE, "encoder_forward: scratch of %zu bytes, need %zu (16-byte aligned)", scratch_bytes, s.bytes);
  hipStream_t stream = (hipStream_t)stream_;
  int rc = SGR_OK;
  LaunchRange on{call->first_launch, call->last_launch};
  // one convolution of the list: with a norm two launches (sums + statistics, apply), otherwise one
  auto conv = [&](int layer, const half_t* src, int cin, int lvl_in, int ks, int stride, int cout, int act, const half_t* res, void* out,
                  int out_kind, void* out2) -> int {
    SgrEncoderConv c = {};
    c.src = src, c.src_stride = cin, c.cin = cin, c.ksize = ks, c.stride = stride, c.n = n, c.h = s.h[lvl_in], c.w = s.w[lvl_in];
    c.weight = wt->layer[layer].weight, c.weight_elems = wt->layer[layer].weight_elems, c.bias = wt->layer[layer].bias;
    c.cout = cout, c.act = act, c.residual = res, c.residual_stride = cout;
    c.out = out, c.out2 = out2, c.out_kind = out_kind, c.out_stride = cout;
    const bool normed = norm && layer != kLayers - 1;
    c.norm = normed ? norm : SGR_ENCODER_NORM_NONE;
    c.raw = normed ? s.raw : nullptr, c.raw_elems = s.raw_elems, c.stats = normed ? s.stats : nullptr, c.stats_elems = s.stats_elems;
    if (on() && (rc = launch_conv(c, stream))) return rc;
    if (normed && on() && (rc = launch_apply(c, stream))) return rc;
    return SGR_OK;
  };
  const int CL = SGR_UPDATE_OUT_CL_F16, NONE = SGR_ENCODER_ACT_NONE, RELU = SGR_ENCODER_ACT_RELU;
  if (on() && (rc = launch_pack(call->images, n, H, W, call->normalize ? call->mean : nullptr, call->normalize ? call->std_ : nullptr, s.xin, stream)))
    return rc;
  if ((rc = conv(0, s.xin, kInPad, 0, 7, 2, 32, RELU, nullptr, s.act[0], CL, nullptr))) return rc;
  int cur = 0, layer = 1;
  // a residual block: y = relu(n(conv1(x))), out = relu(x' + relu(n(conv2(y)))), x' = x or n(downsample(x)); x, y, x', out in four buffers
  auto block = [&](int lvl_in, int cin, int cout, int stride) -> int {
    const int y = (cur + 1) & 3, xd = (cur + 2) & 3, o = (cur + 3) & 3, lvl = lvl_in + (stride == 2);
    if ((rc = conv(layer, s.act[cur], cin, lvl_in, 3, stride, cout, RELU, nullptr, s.act[y], CL, nullptr))) return rc;
    const half_t* skip = s.act[cur];
    if (stride == 2) {
      if ((rc = conv(layer + 2, s.act[cur], cin, lvl_in, 1, 2, cout, NONE, nullptr, s.act[xd], CL, nullptr))) return rc;
      skip = s.act[xd];
    }
    if ((rc = conv(layer + 1, s.act[y], cout, lvl, 3, 1, cout, RELU, skip, s.act[o], CL, nullptr))) return rc;
    layer += stride == 2 ? 3 : 2;
    cur = o;
    return SGR_OK;
  };
  if ((rc = block(1, 32, 32, 1)) || (rc = block(1, 32, 32, 1))) return rc;
  if ((rc = block(1, 32, 64, 2)) || (rc = block(2, 64, 64, 1))) return rc;
  if ((rc = block(2, 64, 128, 2)) || (rc = block(3, 128, 128, 1))) return rc;
  return conv(kLayers - 1, s.act[cur], 128, 3, 1, 1, out_dim, call->split ? SGR_ENCODER_ACT_SPLIT : NONE, nullptr, call->out,
              SGR_UPDATE_OUT_NCHW_F16, call->out2);
}

}  // extern "C"
