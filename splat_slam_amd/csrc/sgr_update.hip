// The tracker's update operator (UpdateModule of the reference's thirdparty/glorie_slam/modules/droid_net/droid_net.py:83-153 with the
// ConvGRU of gru.py and GraphAgg of droid_net.py:48-80), inference only.
//   sgr_update_pack      NCHW (fp16 or fp32, any strides) -> channels-last fp16 [pixel][channel], channels zero-padded to a multiple of 8
//   sgr_update_conv      one implicit-GEMM convolution (1x1, 3x3, 7x7; zero padding, stride 1) on mfma_f32_16x16x32_f16 with a fused epilogue
//   sgr_update_forward   the whole operator: 17 stream-ordered launches, no host synchronisation
// Layouts, the launch list and the rounding points are described in DESIGN.md section 3, "Update operator".  The GEMM, its
// operand roles and the accumulator's lane map are those of sgr_conv_mma.h, shared with the encoders and the ResNet; here a pixel is
// m = (edge, y, x).  Every sum has a fixed order (the MFMA k order, serial loops elsewhere): no atomics, bitwise reproducible.
#include <cstdint>

#include "sgr_conv_mma.h"

namespace sgr {
namespace {

constexpr int kNPad = 64;                   // packed weights have their rows padded to a multiple of this
constexpr int kHidden = 128;
constexpr int kCat = 448;                   // [net | inp | corr_enc | flow_enc]
constexpr int kCorrPad = 200;               // 196 correlation channels padded to a multiple of 8
constexpr int kFlowPad = 8;
constexpr int kGlo = 3 * kHidden;

struct ConvArgs {
  SgrUpdateConv c;
  int M, HW, k_pad;
};

__device__ __forceinline__ float sigmoidf(float v) { return 1.f / (1.f + expf(-v)); }

// The shared tile (sgr_conv_mma.h) on pixels m = (edge, y, x) over all edges: a workgroup's 128 pixels may belong to several edges, the
// halo test is on (y, x) of each pixel's own map, and the channels come from two sources split at c.split.
template <int KS, int BN>
__global__ void __launch_bounds__(kThreads) conv_kernel(const ConvArgs a) {
  constexpr int NT = BN / 16;
  __shared__ __attribute__((aligned(16))) half_t Xs[kBM * kRow];
  __shared__ __attribute__((aligned(16))) half_t Ws[BN * kRow];
  const SgrUpdateConv& c = a.c;
  const int tid = threadIdx.x, m0 = blockIdx.x * kBM, n0 = blockIdx.y * BN;
  const half_t* src0 = (const half_t*)c.src0;
  const half_t* src1 = (const half_t*)c.src1;

  int py[2], px[2], pm[2];
  bool pv[2];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int m = m0 + (tid >> 2) + 64 * i;
    pv[i] = m < a.M;
    pm[i] = pv[i] ? m : 0;
    const int rem = pm[i] % a.HW;
    py[i] = rem / c.w;
    px[i] = rem - py[i] * c.w;
  }
  auto gather = [&](int i, bool tv, int ty, int tx, int ch) {
    const int dy = ty - KS / 2, dx = tx - KS / 2, yy = py[i] + dy, xx = px[i] + dx;
    half8 v = {0, 0, 0, 0, 0, 0, 0, 0};
    if (pv[i] && tv && (unsigned)yy < (unsigned)c.h && (unsigned)xx < (unsigned)c.w) {   // the halo test is on (y, x) of this pixel
      const int64_t pix = (int64_t)pm[i] + dy * c.w + dx;                                 // same edge: yy, xx are inside its map
      const half_t* s = ch < c.split ? src0 + pix * c.stride0 + ch : src1 + pix * c.stride1 + (ch - c.split);
      v = *(const half8*)s;
    }
    return v;
  };
  floatx4 acc[NT][2];
  conv_mma_mainloop<KS, BN>(Xs, Ws, (const half_t*)c.weight, n0, a.k_pad, c.cin, gather, acc);

  // epilogue: acc[t][j][r] is channel acc_channel(n0, t) + r of pixel acc_pixel(j)
  const half_t* aux0 = (const half_t*)c.aux0;
  const half_t* aux1 = (const half_t*)c.aux1;
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int m = acc_pixel(j);
    if (m >= a.M) continue;
    const int e = m / a.HW, p = m - e * a.HW;
#pragma unroll
    for (int t = 0; t < NT; ++t) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int n = acc_channel(n0, t) + r;
        if (n >= c.cout) continue;
        float v = acc[t][j][r] + c.bias[n];
        if (c.eadd) v += c.eadd[(int64_t)e * c.eadd_stride + n];
        switch (c.act) {
          case SGR_UPDATE_ACT_RELU: v = fmaxf(v, 0.f); break;
          case SGR_UPDATE_ACT_SIGMOID: v = sigmoidf(v); break;
          case SGR_UPDATE_ACT_TANH: v = tanhf(v); break;
          case SGR_UPDATE_ACT_ETA: v = 0.01f * (v > 20.f ? v : log1pf(expf(v))); break;
          case SGR_UPDATE_ACT_GATE: v = sigmoidf(v) * (float)aux0[(int64_t)m * c.aux0_stride + n]; break;
          case SGR_UPDATE_ACT_ZR: {
            v = sigmoidf(v);
            if (n >= kHidden) {
              v *= (float)aux0[(int64_t)m * c.aux0_stride + (n - kHidden)];
              ((half_t*)c.out2)[(int64_t)m * c.out2_stride + (n - kHidden)] = (half_t)v;
              continue;
            }
            break;
          }
          case SGR_UPDATE_ACT_BLEND: {
            const float q = tanhf(v), z = (float)aux1[(int64_t)m * c.aux1_stride + n], h0 = (float)aux0[(int64_t)m * c.aux0_stride + n];
            v = (1.f - z) * h0 + z * q;
            ((half_t*)c.out2)[((int64_t)e * c.cout + n) * a.HW + p] = (half_t)v;
            break;
          }
          default: break;
        }
        switch (c.out_kind) {
          case SGR_UPDATE_OUT_CL_F16: ((half_t*)c.out)[(int64_t)m * c.out_stride + n] = (half_t)v; break;
          case SGR_UPDATE_OUT_CL_F32: ((float*)c.out)[(int64_t)m * c.out_stride + n] = v; break;
          case SGR_UPDATE_OUT_NCHW_F16: ((half_t*)c.out)[((int64_t)e * c.cout + n) * a.HW + p] = (half_t)v; break;
          default: ((float*)c.out)[((int64_t)e * c.cout + n) * a.HW + p] = v; break;
        }
      }
    }
  }
}

// One thread per (pixel, 8 channels), pixels fastest: the reads of a plane are coalesced, each store is one 16-byte chunk.
__global__ void __launch_bounds__(kThreads) pack_kernel(const SgrUpdateTensor src, int M, int HW, int w, int C, half_t* __restrict__ dst,
                                                        int dst_stride, int chunks) {
  const int64_t idx = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (idx >= (int64_t)M * chunks) return;
  const int j = (int)(idx / M), m = (int)(idx - (int64_t)j * M);
  half8 v = {0, 0, 0, 0, 0, 0, 0, 0};
  if (src.data) {
    const int e = m / HW, rem = m - e * HW, y = rem / w, x = rem - y * w;
    const int64_t base = e * src.stride[0] + y * src.stride[2] + x * src.stride[3];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int ch = j * 8 + i;
      if (ch < C) {
        const int64_t o = base + ch * src.stride[1];
        v[i] = src.dtype == SGR_UPDATE_F16 ? ((const half_t*)src.data)[o] : (half_t)((const float*)src.data)[o];
      }
    }
  }
  *(half8*)&dst[(int64_t)m * dst_stride + j * 8] = v;
}

// glo[e][c] = mean over the pixels of edge e of gated [M][128] (fp16), rounded to fp16 as the operand of the three 1x1 maps, then
// out[e][o] = bias[o] + sum_c weight[o][c] glo[c] for the 384 outputs (z, r, q).  One workgroup per edge: 16 pixel lanes x 16 channel
// chunks, each lane summing its pixels in ascending order, then the 16 partials in lane order.
__global__ void __launch_bounds__(kThreads) glo_kernel(const half_t* __restrict__ gated, int HW, const float* __restrict__ weight,
                                                       const float* __restrict__ bias, float* __restrict__ out) {
  __shared__ float part[16][kHidden];
  __shared__ float glo[kHidden];
  const int e = blockIdx.x, cc = threadIdx.x & 15, pl = threadIdx.x >> 4;
  float s[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  for (int p = pl; p < HW; p += 16) {
    const half8 v = *(const half8*)&gated[((int64_t)e * HW + p) * kHidden + cc * 8];
#pragma unroll
    for (int i = 0; i < 8; ++i) s[i] += (float)v[i];
  }
#pragma unroll
  for (int i = 0; i < 8; ++i) part[pl][cc * 8 + i] = s[i];
  __syncthreads();
  if (threadIdx.x < kHidden) {
    float t = 0.f;
    for (int k = 0; k < 16; ++k) t += part[k][threadIdx.x];
    glo[threadIdx.x] = (float)(half_t)(t / (float)HW);
  }
  __syncthreads();
  for (int o = threadIdx.x; o < kGlo; o += kThreads) {
    float t = 0.f;
    for (int k = 0; k < kHidden; ++k) t += weight[o * kHidden + k] * glo[k];
    out[(int64_t)e * kGlo + o] = t + bias[o];
  }
}

// out[k][p][c] = mean over the edges e with ix[e] == k, in ascending e, of x[e][p][c]; one thread per (k, p, 8 channels)
__global__ void __launch_bounds__(kThreads) segmean_kernel(const half_t* __restrict__ x, const int64_t* __restrict__ ix, int E, int K,
                                                           int HW, half_t* __restrict__ out) {
  const int64_t idx = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (idx >= (int64_t)K * HW * 16) return;
  const int cc = (int)(idx & 15);
  const int64_t kp = idx >> 4;
  const int k = (int)(kp / HW), p = (int)(kp - (int64_t)k * HW);
  float s[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  int cnt = 0;
  for (int e = 0; e < E; ++e) {
    if (ix[e] != k) continue;
    const half8 v = *(const half8*)&x[((int64_t)e * HW + p) * kHidden + cc * 8];
#pragma unroll
    for (int i = 0; i < 8; ++i) s[i] += (float)v[i];
    ++cnt;
  }
  const float inv = cnt ? 1.f / (float)cnt : 0.f;
  half8 v;
#pragma unroll
  for (int i = 0; i < 8; ++i) v[i] = (half_t)(s[i] * inv);
  *(half8*)&out[kp * kHidden + cc * 8] = v;
}

int launch_conv(const SgrUpdateConv& c, hipStream_t stream) {
  if (!c.src0 || !c.weight || !c.bias || !c.out) return set_error(SGR_ERR_INVALID, "update_conv: null argument");
  if (c.E < 1 || c.h < 1 || c.w < 1 || c.cout < 1 || c.cin < 8 || c.cin % 8)
    return set_error(SGR_ERR_INVALID, "update_conv: bad sizes (E=%d h=%d w=%d cin=%d cout=%d); cin is a positive multiple of 8", c.E, c.h, c.w,
                     c.cin, c.cout);
  if (c.ksize != 1 && c.ksize != 3 && c.ksize != 7) return set_error(SGR_ERR_INVALID, "update_conv: kernel size %d is not 1, 3 or 7", c.ksize);
  const int64_t M = (int64_t)c.E * c.h * c.w;
  if (M > 0x7fffffff - kBM) return set_error(SGR_ERR_CAPACITY, "update_conv: E*h*w = %lld does not fit int32", (long long)M);
  const int split = c.src1 ? c.split : c.cin;
  if (split < 0 || split > c.cin || split % 8 || c.stride0 < split || c.stride0 % 8 || !aligned16(c.src0))
    return set_error(SGR_ERR_INVALID, "update_conv: src0 needs a 16-byte aligned base and a stride (%d) that is a multiple of 8 and >= %d",
                     c.stride0, split);
  if (c.src1 && (c.stride1 < c.cin - split || c.stride1 % 8 || !aligned16(c.src1)))
    return set_error(SGR_ERR_INVALID, "update_conv: src1 needs a 16-byte aligned base and a stride (%d) that is a multiple of 8 and >= %d",
                     c.stride1, c.cin - split);
  const int k_pad = round_up(c.ksize * c.ksize * c.cin, kBK), n_pad = round_up(c.cout, kNPad);
  if (c.weight_elems < (int64_t)n_pad * k_pad || !aligned16(c.weight))
    return set_error(SGR_ERR_INVALID, "update_conv: packed weights must be 16-byte aligned [%d][%d] fp16, got %lld elements", n_pad, k_pad,
                     (long long)c.weight_elems);
  if (c.act < SGR_UPDATE_ACT_NONE || c.act > SGR_UPDATE_ACT_BLEND) return set_error(SGR_ERR_INVALID, "update_conv: unknown epilogue %d", c.act);
  if (c.out_kind < SGR_UPDATE_OUT_CL_F16 || c.out_kind > SGR_UPDATE_OUT_NCHW_F32)
    return set_error(SGR_ERR_INVALID, "update_conv: unknown output kind %d", c.out_kind);
  if (c.out_kind <= SGR_UPDATE_OUT_CL_F32 && c.out_stride < (c.act == SGR_UPDATE_ACT_ZR ? kHidden : c.cout))
    return set_error(SGR_ERR_INVALID, "update_conv: out_stride %d is below the number of channels written", c.out_stride);
  if (c.eadd && c.eadd_stride < c.cout) return set_error(SGR_ERR_INVALID, "update_conv: eadd_stride %d < cout %d", c.eadd_stride, c.cout);
  if (c.act >= SGR_UPDATE_ACT_GATE) {
    const int ch = c.act == SGR_UPDATE_ACT_ZR ? kHidden : c.cout;
    if (!c.aux0 || c.aux0_stride < ch) return set_error(SGR_ERR_INVALID, "update_conv: the gated epilogues need aux0 with stride >= %d", ch);
    if (c.act == SGR_UPDATE_ACT_ZR && (c.cout != 2 * kHidden || !c.out2 || c.out2_stride < kHidden || c.out_kind != SGR_UPDATE_OUT_CL_F16))
      return set_error(SGR_ERR_INVALID, "update_conv: the z|r epilogue needs cout = 256, channels-last fp16 out and out2");
    if (c.act == SGR_UPDATE_ACT_BLEND && (!c.aux1 || c.aux1_stride < c.cout || !c.out2))
      return set_error(SGR_ERR_INVALID, "update_conv: the blend epilogue needs aux1 (z) and out2 (NCHW fp16)");
  }
  ConvArgs a;
  a.c = c;
  a.c.split = split;
  a.M = (int)M;
  a.HW = c.h * c.w;
  a.k_pad = k_pad;
  const bool narrow = c.cout <= 16;
  const dim3 grid((unsigned)((M + kBM - 1) / kBM), (unsigned)((c.cout + (narrow ? 16 : 64) - 1) / (narrow ? 16 : 64))), block(kThreads);
  dispatch_conv<16, 64>(c.ksize, narrow ? 16 : 64, [&](auto ks, auto bn) {
    hipLaunchKernelGGL((conv_kernel<decltype(ks)::value, decltype(bn)::value>), grid, block, 0, stream, a);
  });
  return launched("update_conv");
}

int launch_pack(const SgrUpdateTensor& src, int E, int C, int h, int w, half_t* dst, int dst_stride, int c_pad, hipStream_t stream) {
  const int64_t M = (int64_t)E * h * w, total = M * (c_pad / 8), nblocks = (total + kThreads - 1) / kThreads;
  if (nblocks > 0x7fffffff) return set_error(SGR_ERR_CAPACITY, "update_pack: too many elements");
  hipLaunchKernelGGL(pack_kernel, dim3((unsigned)nblocks), dim3(kThreads), 0, stream, src, (int)M, h * w, w, C, dst, dst_stride, c_pad / 8);
  return launched("update_pack");
}

// Scratch of one call, in halfs per pixel of the E edges unless noted.  hid2 holds z | r*net during the GRU and the two hidden maps
// of the heads afterwards; tmp holds the first layer of an encoder, then the gated map, then GraphAgg's conv1.
struct Scratch {
  half_t *cat, *corr, *flow, *tmp, *hid2, *netn, *agg, *agg2;
  float* glo;
  size_t bytes;
};
Scratch carve(void* base, int64_t M, int64_t MK, int E) {
  Scratch s;
  Carver cv{base};
  s.cat = (half_t*)cv.take((size_t)M * kCat * 2);
  s.corr = (half_t*)cv.take((size_t)M * kCorrPad * 2);
  s.flow = (half_t*)cv.take((size_t)M * kFlowPad * 2);
  s.tmp = (half_t*)cv.take((size_t)M * kHidden * 2);
  s.hid2 = (half_t*)cv.take((size_t)M * 2 * kHidden * 2);
  s.netn = (half_t*)cv.take((size_t)M * kHidden * 2);
  s.agg = (half_t*)cv.take((size_t)MK * kHidden * 2);
  s.agg2 = (half_t*)cv.take((size_t)MK * kHidden * 2);
  s.glo = (float*)cv.take((size_t)E * kGlo * 4);
  s.bytes = cv.off;
  return s;
}

bool sizes_ok(int E, int K, int h, int w) {
  if (E < 1 || K < 0 || K > E || h < 1 || w < 1) return false;
  return (int64_t)E * h * w <= 0x7fffffff - kBM;
}

}  // namespace
}  // namespace sgr

using namespace sgr;

extern "C" {

size_t sgr_update_scratch_bytes(int32_t E, int32_t K, int32_t h, int32_t w) {
  if (!sizes_ok(E, K, h, w)) return 0;
  return carve(nullptr, (int64_t)E * h * w, (int64_t)K * h * w, E).bytes;
}

int sgr_update_pack(const SgrUpdateTensor* src, int32_t E, int32_t C, int32_t h, int32_t w, void* dst, int32_t dst_stride, int32_t c_pad,
                    void* stream) {
  if (!src || !dst) return set_error(SGR_ERR_INVALID, "update_pack: null argument");
  if (!sizes_ok(E, 0, h, w) || C < 1 || c_pad < C || c_pad % 8 || dst_stride < c_pad || dst_stride % 8 || !aligned16(dst))
    return set_error(SGR_ERR_INVALID, "update_pack: bad sizes (E=%d C=%d h=%d w=%d c_pad=%d dst_stride=%d) or unaligned dst", E, C, h, w, c_pad,
                     dst_stride);
  if (src->data && src->dtype != SGR_UPDATE_F16 && src->dtype != SGR_UPDATE_F32) return set_error(SGR_ERR_INVALID, "update_pack: unknown dtype");
  return launch_pack(*src, E, C, h, w, (half_t*)dst, dst_stride, c_pad, (hipStream_t)stream);
}

int sgr_update_conv(const SgrUpdateConv* conv, void* stream) {
  if (!conv) return set_error(SGR_ERR_INVALID, "update_conv: null argument");
  return launch_conv(*conv, (hipStream_t)stream);
}

int sgr_update_forward(const SgrUpdateWeights* wt, const SgrUpdateCall* call, void* scratch, size_t scratch_bytes, void* stream_) {
  if (!wt || !call || !scratch) return set_error(SGR_ERR_INVALID, "update_forward: null argument");
  const int E = call->E, K = call->K, h = call->h, w = call->w;
  if (!sizes_ok(E, K, h, w)) return set_error(SGR_ERR_INVALID, "update_forward: bad sizes (E=%d K=%d h=%d w=%d)", E, K, h, w);
  if (!call->net.data || !call->inp.data || !call->corr.data || !call->net_out || !call->delta || !call->weight)
    return set_error(SGR_ERR_INVALID, "update_forward: null tensor");
  if (K > 0 && (!call->ix || !call->eta || !call->upmask)) return set_error(SGR_ERR_INVALID, "update_forward: K > 0 needs ix, eta and upmask");
  for (const SgrUpdateTensor* t : {&call->net, &call->inp, &call->corr, &call->flow})
    if (t->data && t->dtype != SGR_UPDATE_F16 && t->dtype != SGR_UPDATE_F32) return set_error(SGR_ERR_INVALID, "update_forward: unknown dtype");
  if (!wt->glo_weight || !wt->glo_bias) return set_error(SGR_ERR_INVALID, "update_forward: null weights");
  const int64_t M = (int64_t)E * h * w, MK = (int64_t)K * h * w;
  const Scratch s = carve(scratch, M, MK, E);
  if (scratch_bytes < s.bytes || !aligned16(scratch))
    return set_error(SGR_ERR_WORKSPACE, "update_forward: scratch of %zu bytes, need %zu (16-byte aligned)", scratch_bytes, s.bytes);
  hipStream_t stream = (hipStream_t)stream_;
  LaunchRange on{call->first_launch, call->last_launch};
  auto conv = [&](int layer, const half_t* src0, int stride0, const half_t* src1, int stride1, int split, int cin, int ks, int edges, int cout,
                  int act, const float* eadd, const half_t* aux0, int aux0_stride, const half_t* aux1, void* out, int out_kind, int out_stride,
                  void* out2, int out2_stride) {
    SgrUpdateConv c = {};
    c.src0 = src0, c.stride0 = stride0, c.src1 = src1, c.stride1 = stride1, c.split = split, c.cin = cin, c.ksize = ks;
    c.E = edges, c.h = h, c.w = w;
    c.weight = wt->layer[layer].weight, c.weight_elems = wt->layer[layer].weight_elems, c.bias = wt->layer[layer].bias;
    c.cout = cout, c.act = act, c.eadd = eadd, c.eadd_stride = kGlo;
    c.aux0 = aux0, c.aux0_stride = aux0_stride, c.aux1 = aux1, c.aux1_stride = kHidden;
    c.out = out, c.out_kind = out_kind, c.out_stride = out_stride, c.out2 = out2, c.out2_stride = out2_stride;
    return launch_conv(c, stream);
  };
  const int CL = SGR_UPDATE_OUT_CL_F16;
  const int NONE = SGR_UPDATE_ACT_NONE, RELU = SGR_UPDATE_ACT_RELU;
  half_t* z = s.hid2;                    // [M][128]
  half_t* rnet = s.hid2 + M * kHidden;   // [M][128]
  int rc = SGR_OK;
  if (on()) {
    if ((rc = launch_pack(call->net, E, kHidden, h, w, s.cat, kCat, kHidden, stream))) return rc;
    if ((rc = launch_pack(call->inp, E, kHidden, h, w, s.cat + kHidden, kCat, kHidden, stream))) return rc;
    if ((rc = launch_pack(call->corr, E, 196, h, w, s.corr, kCorrPad, kCorrPad, stream))) return rc;
    if ((rc = launch_pack(call->flow, E, 4, h, w, s.flow, kFlowPad, kFlowPad, stream))) return rc;
  }
  // encoders
  if (on() && (rc = conv(0, s.corr, kCorrPad, nullptr, 0, 0, kCorrPad, 1, E, kHidden, RELU, nullptr, nullptr, 0, nullptr, s.tmp, CL, kHidden, nullptr, 0)))
    return rc;
  if (on() && (rc = conv(1, s.tmp, kHidden, nullptr, 0, 0, kHidden, 3, E, kHidden, RELU, nullptr, nullptr, 0, nullptr, s.cat + 256, CL, kCat, nullptr, 0)))
    return rc;
  if (on() && (rc = conv(2, s.flow, kFlowPad, nullptr, 0, 0, kFlowPad, 7, E, kHidden, RELU, nullptr, nullptr, 0, nullptr, s.tmp, CL, kHidden, nullptr, 0)))
    return rc;
  if (on() && (rc = conv(3, s.tmp, kHidden, nullptr, 0, 0, kHidden, 3, E, 64, RELU, nullptr, nullptr, 0, nullptr, s.cat + 384, CL, kCat, nullptr, 0)))
    return rc;
  // ConvGRU
  if (on() && (rc = conv(4, s.cat, kCat, nullptr, 0, 0, kHidden, 1, E, kHidden, SGR_UPDATE_ACT_GATE, nullptr, s.cat, kCat, nullptr, s.tmp, CL, kHidden,
                         nullptr, 0)))
    return rc;
  if (on()) {
    hipLaunchKernelGGL(glo_kernel, dim3(E), dim3(kThreads), 0, stream, (const half_t*)s.tmp, h * w, wt->glo_weight, wt->glo_bias, s.glo);
    if ((rc = launched("update_forward: glo"))) return rc;
  }
  if (on() && (rc = conv(5, s.cat, kCat, nullptr, 0, 0, kCat, 3, E, 2 * kHidden, SGR_UPDATE_ACT_ZR, s.glo, s.cat, kCat, nullptr, z, CL, kHidden, rnet,
                         kHidden)))
    return rc;
  if (on() && (rc = conv(6, rnet, kHidden, s.cat + kHidden, kCat, kHidden, kCat, 3, E, kHidden, SGR_UPDATE_ACT_BLEND, s.glo + 2 * kHidden, s.cat, kCat, z,
                         s.netn, CL, kHidden, call->net_out, 0)))
    return rc;
  // heads: the two hidden maps side by side, then 128 -> 2 each
  if (on() && (rc = conv(7, s.netn, kHidden, nullptr, 0, 0, kHidden, 3, E, 2 * kHidden, RELU, nullptr, nullptr, 0, nullptr, s.hid2, CL, 2 * kHidden,
                         nullptr, 0)))
    return rc;
  if (on() && (rc = conv(8, s.hid2, 2 * kHidden, nullptr, 0, 0, kHidden, 3, E, 2, NONE, nullptr, nullptr, 0, nullptr, call->delta, CL, 2, nullptr, 0)))
    return rc;
  if (on() && (rc = conv(9, s.hid2 + kHidden, 2 * kHidden, nullptr, 0, 0, kHidden, 3, E, 2, SGR_UPDATE_ACT_SIGMOID, nullptr, nullptr, 0, nullptr,
                         call->weight, CL, 2, nullptr, 0)))
    return rc;
  if (K == 0) return SGR_OK;
  // GraphAgg
  if (on() && (rc = conv(10, s.netn, kHidden, nullptr, 0, 0, kHidden, 3, E, kHidden, RELU, nullptr, nullptr, 0, nullptr, s.tmp, CL, kHidden, nullptr, 0)))
    return rc;
  if (on()) {
    const int64_t nblocks = (MK * 16 + kThreads - 1) / kThreads;
    hipLaunchKernelGGL(segmean_kernel, dim3((unsigned)nblocks), dim3(kThreads), 0, stream, (const half_t*)s.tmp, call->ix, E, K, h * w, s.agg);
    if ((rc = launched("update_forward: segmented mean"))) return rc;
  }
  if (on() && (rc = conv(11, s.agg, kHidden, nullptr, 0, 0, kHidden, 3, K, kHidden, RELU, nullptr, nullptr, 0, nullptr, s.agg2, CL, kHidden, nullptr, 0)))
    return rc;
  if (on() && (rc = conv(12, s.agg2, kHidden, nullptr, 0, 0, kHidden, 3, K, 1, SGR_UPDATE_ACT_ETA, nullptr, nullptr, 0, nullptr, call->eta,
                         SGR_UPDATE_OUT_CL_F32, 1, nullptr, 0)))
    return rc;
  if (on() && (rc = conv(13, s.agg2, kHidden, nullptr, 0, 0, kHidden, 1, K, 576, NONE, nullptr, nullptr, 0, nullptr, call->upmask,
                         SGR_UPDATE_OUT_NCHW_F16, 0, nullptr, 0)))
    return rc;
  return SGR_OK;
}

}  // extern "C"
