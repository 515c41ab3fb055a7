// The vision transformer of the mono-depth prior (timm's ViT blocks as the DPT of the reference's
// thirdparty/mono_priors/omnidata/modules/midas/vit.py reads them), inference only.
//   sgr_vit_layernorm    fp32 row -> fp16 row, one wave per row
//   sgr_vit_gemm         out[M][N] = epi(A[M][K] W[N][K]^T + bias) on mfma_f32_16x16x32_f16, six epilogues
//   sgr_vit_attention    softmax(q k^T / 8) v per (image, head), flash style, no T x T buffer
//   sgr_vit_forward      the whole stack: 5 + 7 depth stream-ordered launches, no host synchronisation
// Layouts, the launch list and the rounding points are described in DESIGN.md section 3, "Vision transformer".  As in sgr_update.hip
// the weights are the A operand of the MFMA and the tokens the B operand, so that a lane of the accumulator holds four consecutive
// output channels of one token.  Every sum has a fixed order that follows from the shape alone: no atomics, bitwise reproducible, and
// a row never sees another row.
#include <cstdint>

#include "sgr_conv_mma.h"                   // the vector types and the host helpers; the GEMM here has its own tile

namespace sgr {
namespace {

typedef short short4v __attribute__((__vector_size__(8)));

constexpr int kHead = 64;                   // head dimension
constexpr int kMaxHeads = 16;
constexpr int kBN = 64;                     // output channels of one GEMM workgroup
constexpr int kBK = 64;                     // k of one staging step: two MFMA k steps (this file's, not the convolution tile's 32)
constexpr int kRow = kBK + 8;               // halfs per LDS row: 144 bytes, so that the 16 rows of a fragment read spread over the banks

// exact GELU, 0.5 v (1 + erf(v / sqrt 2)), written with erfc so that the left tail keeps its relative accuracy
__device__ __forceinline__ float gelu(float v) { return 0.5f * v * erfcf(-0.70710678118654752f * v); }

// ---- layer norm: one wave per row, lane l holds elements l, l + 64, ... ----------------------------------------------------------------
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) v += __shfl_xor(v, o);
  return v;
}

__global__ void __launch_bounds__(kThreads) layernorm_kernel(const float* __restrict__ x, const float* __restrict__ gamma,
                                                             const float* __restrict__ beta, int64_t M, int D, half_t* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const int64_t m = (int64_t)blockIdx.x * (kThreads / 64) + (threadIdx.x >> 6);
  if (m >= M) return;                       // whole waves leave
  const float* row = x + m * D;
  const int n = D / 64;
  const float x0 = row[0];                  // the shift: differences of nearby values are exact, a constant row becomes zeros
  float d[kMaxHeads];
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < kMaxHeads; ++i) {
    d[i] = i < n ? row[i * 64 + lane] - x0 : 0.f;
    s += d[i];
  }
  const float mean = wave_sum(s) / (float)D;
  float q = 0.f;
#pragma unroll
  for (int i = 0; i < kMaxHeads; ++i) {
    d[i] = i < n ? d[i] - mean : 0.f;
    q += d[i] * d[i];
  }
  const float rstd = 1.f / sqrtf(wave_sum(q) / (float)D + 1e-6f);
#pragma unroll
  for (int i = 0; i < kMaxHeads; ++i)
    if (i < n) out[m * D + i * 64 + lane] = (half_t)(d[i] * rstd * gamma[i * 64 + lane] + beta[i * 64 + lane]);
}

// ---- GEMM -------------------------------------------------------------------------------------------------------------------------------
// One workgroup: BM = 32 MT tokens x 64 output channels.  The four waves sit 2 x 2: wave (wm, wn) owns tokens [16 MT wm, 16 MT (wm + 1))
// as MT B tiles and channels [32 wn, 32 wn + 32) as two A tiles.  Staging: thread t loads the 16-byte chunk k = 8 (t & 7) of rows
// t >> 3 + 32 i into registers one step ahead of the MFMAs that consume the previous step out of LDS.
template <int MT>
__global__ void __launch_bounds__(kThreads) gemm_kernel(const SgrVitGemm g) {
  constexpr int BM = 32 * MT, XR = BM / 32;
  __shared__ __attribute__((aligned(16))) half_t Xs[BM * kRow];
  __shared__ __attribute__((aligned(16))) half_t Ws[kBN * kRow];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wm = wave >> 1, wn = wave & 1;
  const int m0 = blockIdx.x * BM, n0 = blockIdx.y * kBN;
  const int kc = tid & 7, srow = tid >> 3;
  const half_t* ap[XR];
  bool av[XR];
#pragma unroll
  for (int i = 0; i < XR; ++i) {
    const int m = m0 + srow + 32 * i;
    av[i] = m < g.M;
    ap[i] = (const half_t*)g.a + (int64_t)(av[i] ? m : 0) * g.lda + kc * 8;
  }
  const half_t* wp[2];
#pragma unroll
  for (int i = 0; i < 2; ++i) wp[i] = (const half_t*)g.w + (int64_t)(n0 + srow + 32 * i) * g.ldw + kc * 8;

  half8 xr[XR], wr[2];
  auto gload = [&](int kt) {
#pragma unroll
    for (int i = 0; i < XR; ++i) {
      half8 v = {0, 0, 0, 0, 0, 0, 0, 0};
      if (av[i]) v = *(const half8*)(ap[i] + (int64_t)kt * kBK);
      xr[i] = v;
    }
#pragma unroll
    for (int i = 0; i < 2; ++i) wr[i] = *(const half8*)(wp[i] + (int64_t)kt * kBK);
  };

  floatx4 acc[2][MT];
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int j = 0; j < MT; ++j) acc[t][j] = floatx4{0.f, 0.f, 0.f, 0.f};

  const int nk = g.K / kBK;
  gload(0);
  for (int kt = 0; kt < nk; ++kt) {
#pragma unroll
    for (int i = 0; i < XR; ++i) *(half8*)&Xs[(srow + 32 * i) * kRow + kc * 8] = xr[i];
#pragma unroll
    for (int i = 0; i < 2; ++i) *(half8*)&Ws[(srow + 32 * i) * kRow + kc * 8] = wr[i];
    __syncthreads();
    if (kt + 1 < nk) gload(kt + 1);
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      half8 bf[MT], af[2];
#pragma unroll
      for (int j = 0; j < MT; ++j) bf[j] = *(const half8*)&Xs[(wm * 16 * MT + j * 16 + (lane & 15)) * kRow + s * 32 + (lane >> 4) * 8];
#pragma unroll
      for (int t = 0; t < 2; ++t) af[t] = *(const half8*)&Ws[(wn * 32 + t * 16 + (lane & 15)) * kRow + s * 32 + (lane >> 4) * 8];
#pragma unroll
      for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int j = 0; j < MT; ++j) acc[t][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(af[t], bf[j], acc[t][j], 0, 0, 0);
    }
    __syncthreads();
  }

  // epilogue: acc[t][j][r] is channel n0 + 32 wn + 16 t + 4 (lane >> 4) + r of token m0 + 16 MT wm + 16 j + (lane & 15)
#pragma unroll
  for (int j = 0; j < MT; ++j) {
    const int m = m0 + wm * 16 * MT + j * 16 + (lane & 15);
    if (m >= g.M) continue;
    int b = 0, tok = 0;
    if (g.epi == SGR_VIT_EPI_READOUT) {
      b = m / g.T, tok = m - b * g.T;
      if (tok == 0) continue;
    } else if (g.epi == SGR_VIT_EPI_EMBED) {
      b = m / (g.T - 1), tok = m - b * (g.T - 1) + 1;
    }
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      const int n = n0 + wn * 32 + t * 16 + (lane >> 4) * 4;
      floatx4 v = acc[t][j];
      if (g.bias) v += *(const floatx4*)&g.bias[n];
      switch (g.epi) {
        case SGR_VIT_EPI_STORE_F16:
          *(half4*)&((half_t*)g.out)[(int64_t)m * g.ldo + n] = half4{(half_t)v[0], (half_t)v[1], (half_t)v[2], (half_t)v[3]};
          break;
        case SGR_VIT_EPI_STORE_F32: *(floatx4*)&((float*)g.out)[(int64_t)m * g.ldo + n] = v; break;
        case SGR_VIT_EPI_GELU_F16:
          *(half4*)&((half_t*)g.out)[(int64_t)m * g.ldo + n] = half4{(half_t)gelu(v[0]), (half_t)gelu(v[1]), (half_t)gelu(v[2]), (half_t)gelu(v[3])};
          break;
        case SGR_VIT_EPI_RESIDUAL: {
          float* o = &((float*)g.out)[(int64_t)m * g.ldo + n];
          v += *(const floatx4*)o;
          *(floatx4*)o = v;
          if (g.tap) *(half4*)&((half_t*)g.tap)[(int64_t)m * g.ldo + n] = half4{(half_t)v[0], (half_t)v[1], (half_t)v[2], (half_t)v[3]};
          break;
        }
        case SGR_VIT_EPI_READOUT: {
          v += *(const floatx4*)&g.aux[(int64_t)b * g.N + n];
#pragma unroll
          for (int r = 0; r < 4; ++r) ((half_t*)g.out)[((int64_t)b * g.N + n + r) * (g.T - 1) + tok - 1] = (half_t)gelu(v[r]);
          break;
        }
        default: {  // SGR_VIT_EPI_EMBED
          v += *(const floatx4*)&g.aux[(int64_t)tok * g.N + n];
          *(floatx4*)&((float*)g.out)[((int64_t)b * g.T + tok) * g.ldo + n] = v;
          break;
        }
      }
    }
  }
}

// stream[b * T][:] = pos[0][:], the class token with its position row
__global__ void __launch_bounds__(kThreads) cls_kernel(const float* __restrict__ pos, int B, int T, int D, float* __restrict__ stream) {
  const int idx = blockIdx.x * kThreads + threadIdx.x;
  if (idx >= B * D) return;
  const int b = idx / D, c = idx - b * D;
  stream[(int64_t)b * T * D + c] = pos[c];
}

// ---- attention ----------------------------------------------------------------------------------------------------------------------------
// One workgroup: 64 queries of one (image, head), wave v the 16 queries 16 v .. 16 v + 15; K and V go through LDS in tiles of 64 keys.
// S^T = K Q^T (K the A operand, Q the B operand): a lane holds, for its query lane & 15, the keys 16 c + 4 (lane >> 4) + r of key tile
// c in register r, so a row's maximum and sum are 16 in-lane steps and two shuffles.  O^T = V^T P^T takes those registers as the B
// operand without moving them: k slot (g = lane >> 4, j) of the 32-key step s stands for key 32 s + 16 (j >> 2) + 4 g + (j & 3), and
// the A operand reads V^T in the same order with two transposed LDS reads (ds_read_b64_tr_b16: the 16 lanes of group g give the
// addresses of rows 4 g .. 4 g + 3 of a 4 x 16 block and lane i of the group receives column i).
constexpr int kQB = 64, kKB = 64;

__global__ void __launch_bounds__(kThreads) attention_kernel(const half_t* __restrict__ qkv, int T, int heads, half_t* __restrict__ out) {
  __shared__ __attribute__((aligned(16))) half_t Ks[kKB * kRow];
  __shared__ __attribute__((aligned(16))) half_t Vs[kKB * kRow];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, g = lane >> 4, li = lane & 15;
  const int head = blockIdx.y, D = heads * kHead;
  const int64_t row = 3 * (int64_t)D;                                     // halfs between two tokens of qkv
  const half_t* base = qkv + (int64_t)blockIdx.z * T * row + head * kHead;
  const int q = blockIdx.x * kQB + wave * 16 + li;

  half8 qf[2];
#pragma unroll
  for (int s = 0; s < 2; ++s) {
    half8 v = {0, 0, 0, 0, 0, 0, 0, 0};
    if (q < T) v = *(const half8*)(base + q * row + s * 32 + g * 8);
    qf[s] = v;
  }

  const int kc = tid & 7, srow = tid >> 3;
  half8 kr[2], vr[2];
  auto gload = [&](int kt) {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int key = kt * kKB + srow + 32 * i;
      half8 a = {0, 0, 0, 0, 0, 0, 0, 0}, b = a;                          // keys past T: zeros, so that 0 * v stays 0
      if (key < T) {
        const half_t* p = base + key * row + kc * 8;
        a = *(const half8*)(p + D);
        b = *(const half8*)(p + 2 * D);
      }
      kr[i] = a, vr[i] = b;
    }
  };

  floatx4 o[4];
#pragma unroll
  for (int dt = 0; dt < 4; ++dt) o[dt] = floatx4{0.f, 0.f, 0.f, 0.f};
  float mx = -INFINITY, sum = 0.f;                                        // sum: this lane's share of the row sum

  const int nt = (T + kKB - 1) / kKB;
  gload(0);
  for (int kt = 0; kt < nt; ++kt) {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      *(half8*)&Ks[(srow + 32 * i) * kRow + kc * 8] = kr[i];
      *(half8*)&Vs[(srow + 32 * i) * kRow + kc * 8] = vr[i];
    }
    __syncthreads();
    if (kt + 1 < nt) gload(kt + 1);

    floatx4 sc[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      sc[c] = floatx4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        const half8 kf = *(const half8*)&Ks[(c * 16 + li) * kRow + s * 32 + g * 8];
        sc[c] = __builtin_amdgcn_mfma_f32_16x16x32_f16(kf, qf[s], sc[c], 0, 0, 0);
      }
    }
    float tmax = -INFINITY;
#pragma unroll
    for (int c = 0; c < 4; ++c)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int key = kt * kKB + c * 16 + g * 4 + r;
        sc[c][r] = key < T ? sc[c][r] * 0.125f : -INFINITY;
        tmax = fmaxf(tmax, sc[c][r]);
      }
    tmax = fmaxf(tmax, __shfl_xor(tmax, 16));
    tmax = fmaxf(tmax, __shfl_xor(tmax, 32));
    const float mnew = fmaxf(mx, tmax);                                   // finite: key kt * 64 of every tile is below T
    const float alpha = expf(mx - mnew);                                  // 0 on the first tile
    mx = mnew;
    half8 pf[2];
    float psum = 0.f;
#pragma unroll
    for (int c = 0; c < 4; ++c)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const half_t p = (half_t)expf(sc[c][r] - mnew);
        pf[c >> 1][(c & 1) * 4 + r] = p;
        psum += (float)p;
      }
    sum = sum * alpha + psum;
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) {
      o[dt] *= alpha;
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        // rows 32 s + 4 g + (li >> 2) and 16 below, columns 16 dt + 4 (li & 3) .. + 3
        const half_t* p = &Vs[(s * 32 + g * 4 + (li >> 2)) * kRow + dt * 16 + (li & 3) * 4];
        const half4 lo = __builtin_bit_cast(half4, __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) short4v*)p));
        const half4 hi =
            __builtin_bit_cast(half4, __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) short4v*)(p + 16 * kRow)));
        const half8 vf = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
        o[dt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(vf, pf[s], o[dt], 0, 0, 0);
      }
    }
    __syncthreads();
  }

  sum += __shfl_xor(sum, 16);
  sum += __shfl_xor(sum, 32);
  if (q >= T) return;
  const float inv = 1.f / sum;
  half_t* dst = out + ((int64_t)blockIdx.z * T + q) * D + head * kHead;
#pragma unroll
  for (int dt = 0; dt < 4; ++dt)    // o[dt][r] is channel 16 dt + 4 g + r of query q
    *(half4*)&dst[dt * 16 + g * 4] = half4{(half_t)(o[dt][0] * inv), (half_t)(o[dt][1] * inv), (half_t)(o[dt][2] * inv), (half_t)(o[dt][3] * inv)};
}

// ---- host side --------------------------------------------------------------------------------------------------------------------------
constexpr int64_t kMaxRows = 0x7fffffff - 128;

bool geometry_ok(int64_t B, int64_t T, int heads, int depth) {
  return B >= 1 && T >= 2 && heads >= 1 && heads <= kMaxHeads && depth >= 1 && B * T <= kMaxRows;
}

int launch_layernorm(const float* x, const float* gamma, const float* beta, int64_t M, int D, half_t* out, hipStream_t stream) {
  if (!x || !gamma || !beta || !out) return set_error(SGR_ERR_INVALID, "vit_layernorm: null argument");
  if (M < 1 || M > kMaxRows || D < 64 || D % 64 || D > 64 * kMaxHeads)
    return set_error(SGR_ERR_INVALID, "vit_layernorm: bad sizes (M=%lld D=%d); D is a multiple of 64 up to %d", (long long)M, D, 64 * kMaxHeads);
  if (!aligned16(out)) return set_error(SGR_ERR_INVALID, "vit_layernorm: out must be 16-byte aligned");
  hipLaunchKernelGGL(layernorm_kernel, dim3((unsigned)((M + 3) / 4)), dim3(kThreads), 0, stream, x, gamma, beta, M, D, out);
  return launched("vit_layernorm");
}

int launch_gemm(const SgrVitGemm& g, hipStream_t stream) {
  if (!g.a || !g.w || !g.out) return set_error(SGR_ERR_INVALID, "vit_gemm: null argument");
  if (g.M < 1 || g.M > kMaxRows || g.N < 64 || g.N % 64 || g.K < 64 || g.K % 64)
    return set_error(SGR_ERR_INVALID, "vit_gemm: bad sizes (M=%d N=%d K=%d); N and K are positive multiples of 64", g.M, g.N, g.K);
  if (g.epi < SGR_VIT_EPI_STORE_F16 || g.epi > SGR_VIT_EPI_STORE_F32) return set_error(SGR_ERR_INVALID, "vit_gemm: unknown epilogue %d", g.epi);
  if (g.lda < g.K || g.lda % 8 || g.ldw < g.K || g.ldw % 8 || !aligned16(g.a) || !aligned16(g.w))
    return set_error(SGR_ERR_INVALID, "vit_gemm: a and w need 16-byte aligned bases and row strides (%lld, %lld) that are multiples of 8 and >= K",
                     (long long)g.lda, (long long)g.ldw);
  const bool mapped = g.epi == SGR_VIT_EPI_READOUT || g.epi == SGR_VIT_EPI_EMBED;
  if (!aligned16(g.out) || (g.bias && !aligned16(g.bias)) || (g.epi != SGR_VIT_EPI_READOUT && (g.ldo < g.N || g.ldo % 8)))
    return set_error(SGR_ERR_INVALID, "vit_gemm: out and bias must be 16-byte aligned, ldo (%lld) a multiple of 8 and >= N", (long long)g.ldo);
  if (g.tap && (g.epi != SGR_VIT_EPI_RESIDUAL || !aligned16(g.tap))) return set_error(SGR_ERR_INVALID, "vit_gemm: tap goes with the residual epilogue");
  if (mapped) {
    const int per = g.epi == SGR_VIT_EPI_READOUT ? g.T : g.T - 1;
    if (!g.aux || !aligned16(g.aux) || g.T < 2 || g.M % per)
      return set_error(SGR_ERR_INVALID, "vit_gemm: the readout and embedding epilogues need aux, T >= 2 and whole images (M=%d T=%d)", g.M, g.T);
    if ((int64_t)(g.M / per) * g.T > kMaxRows) return set_error(SGR_ERR_CAPACITY, "vit_gemm: B * T does not fit int32");
  }
  const bool wide = g.N >= 1536 && g.M > 64;          // the wide layers have enough column tiles to fill the chip with 128-token tiles
  const int bm = wide ? 128 : 64;
  const dim3 grid((unsigned)((g.M + bm - 1) / bm), (unsigned)(g.N / kBN)), block(kThreads);
  if (wide)
    hipLaunchKernelGGL(gemm_kernel<4>, grid, block, 0, stream, g);
  else
    hipLaunchKernelGGL(gemm_kernel<2>, grid, block, 0, stream, g);
  return launched("vit_gemm");
}

int launch_attention(const half_t* qkv, int B, int T, int heads, half_t* out, hipStream_t stream) {
  if (!qkv || !out) return set_error(SGR_ERR_INVALID, "vit_attention: null argument");
  if (!geometry_ok(B, T, heads, 1) || B > 65535)
    return set_error(SGR_ERR_INVALID, "vit_attention: bad sizes (B=%d T=%d heads=%d); heads 1..%d, T >= 2, B <= 65535", B, T, heads, kMaxHeads);
  if (!aligned16(qkv) || !aligned16(out)) return set_error(SGR_ERR_INVALID, "vit_attention: qkv and out must be 16-byte aligned");
  hipLaunchKernelGGL(attention_kernel, dim3((unsigned)((T + kQB - 1) / kQB), (unsigned)heads, (unsigned)B), dim3(kThreads), 0, stream, qkv, T,
                     heads, out);
  return launched("vit_attention");
}

// Scratch of one call.  xn: a normalised row; hid: the MLP's hidden rows; rv: the class-token half of the two readouts.
struct Scratch {
  float *stream, *rv;
  half_t *xn, *qkv, *att, *hid, *tap[2];
  size_t bytes;
};
Scratch carve(void* base, int64_t B, int64_t M, int64_t D) {
  Scratch s;
  Carver cv{base};
  s.stream = (float*)cv.take((size_t)M * D * 4);
  s.xn = (half_t*)cv.take((size_t)M * D * 2);
  s.qkv = (half_t*)cv.take((size_t)M * 3 * D * 2);
  s.att = (half_t*)cv.take((size_t)M * D * 2);
  s.hid = (half_t*)cv.take((size_t)M * 4 * D * 2);
  s.tap[0] = (half_t*)cv.take((size_t)M * D * 2);
  s.tap[1] = (half_t*)cv.take((size_t)M * D * 2);
  s.rv = (float*)cv.take((size_t)2 * B * D * 4);
  s.bytes = cv.off;
  return s;
}

}  // namespace
}  // namespace sgr

using namespace sgr;

extern "C" {

size_t sgr_vit_scratch_bytes(int32_t B, int32_t T, int32_t heads, int32_t depth) {
  if (!geometry_ok(B, T, heads, depth) || B > 65535) return 0;
  return carve(nullptr, B, (int64_t)B * T, (int64_t)heads * kHead).bytes;
}

int sgr_vit_layernorm(const float* x, const float* gamma, const float* beta, int64_t M, int32_t D, void* out, void* stream) {
  return launch_layernorm(x, gamma, beta, M, D, (half_t*)out, (hipStream_t)stream);
}

int sgr_vit_gemm(const SgrVitGemm* gemm, void* stream) {
  if (!gemm) return set_error(SGR_ERR_INVALID, "vit_gemm: null argument");
  return launch_gemm(*gemm, (hipStream_t)stream);
}

int sgr_vit_attention(const void* qkv, int32_t B, int32_t T, int32_t heads, void* out, void* stream) {
  return launch_attention((const half_t*)qkv, B, T, heads, (half_t*)out, (hipStream_t)stream);
}

int sgr_vit_forward(const SgrVitWeights* wt, const SgrVitCall* call, void* scratch, size_t scratch_bytes, void* stream_) {
  if (!wt || !call || !scratch) return set_error(SGR_ERR_INVALID, "vit_forward: null argument");
  const int B = call->B, D = wt->dim, heads = wt->heads, depth = wt->depth;
  if (call->gh < 1 || call->gw < 1 || (int64_t)call->gh * call->gw > kMaxRows)
    return set_error(SGR_ERR_INVALID, "vit_forward: bad grid %d x %d", call->gh, call->gw);
  const int T = 1 + call->gh * call->gw;
  if (!geometry_ok(B, T, heads, depth) || B > 65535 || D != heads * kHead || wt->cin < 64 || wt->cin % 64)
    return set_error(SGR_ERR_INVALID, "vit_forward: bad sizes (B=%d T=%d dim=%d heads=%d depth=%d cin=%d)", B, T, D, heads, depth, wt->cin);
  if (wt->tap[0] < 0 || wt->tap[0] >= depth || wt->tap[1] < 0 || wt->tap[1] >= depth || wt->tap[0] == wt->tap[1])
    return set_error(SGR_ERR_INVALID, "vit_forward: the taps (%d, %d) must be two distinct blocks below %d", wt->tap[0], wt->tap[1], depth);
  if (!call->patches || !call->pos || !call->out[0] || !call->out[1] || !wt->embed_w || !wt->blocks || !wt->readout_w[0] || !wt->readout_w[1] ||
      !wt->readout_b[0] || !wt->readout_b[1])
    return set_error(SGR_ERR_INVALID, "vit_forward: null tensor");
  const int64_t M = (int64_t)B * T;
  const Scratch s = carve(scratch, B, M, D);
  if (scratch_bytes < s.bytes || !aligned16(scratch))
    return set_error(SGR_ERR_WORKSPACE, "vit_forward: scratch of %zu bytes, need %zu (16-byte aligned)", scratch_bytes, s.bytes);
  hipStream_t stream = (hipStream_t)stream_;
  LaunchRange on{call->first_launch, call->last_launch};
  auto gemm = [&](const void* a, int64_t lda, const void* w, int64_t ldw, const float* bias, int m, int n, int k, int epi, void* out, int64_t ldo,
                  void* tap, const float* aux) {
    SgrVitGemm g = {};
    g.a = a, g.lda = lda, g.w = w, g.ldw = ldw, g.bias = bias, g.M = m, g.N = n, g.K = k, g.epi = epi, g.out = out, g.ldo = ldo, g.tap = tap;
    g.aux = aux, g.T = T;
    return launch_gemm(g, stream);
  };
  int rc = SGR_OK;
  if (on()) {
    hipLaunchKernelGGL(cls_kernel, dim3((unsigned)((B * D + kThreads - 1) / kThreads)), dim3(kThreads), 0, stream, call->pos, B, T, D, s.stream);
    if ((rc = launched("vit_forward: class-token"))) return rc;
    if ((rc = gemm(call->patches, wt->cin, wt->embed_w, wt->cin, wt->embed_b, B * (T - 1), D, wt->cin, SGR_VIT_EPI_EMBED, s.stream, D, nullptr,
                   call->pos)))
      return rc;
  }
  for (int i = 0; i < depth; ++i) {
    const SgrVitBlock& b = wt->blocks[i];
    half_t* tap = i == wt->tap[0] ? s.tap[0] : i == wt->tap[1] ? s.tap[1] : nullptr;
    if (on() && (rc = launch_layernorm(s.stream, b.ln1_g, b.ln1_b, M, D, s.xn, stream))) return rc;
    if (on() && (rc = gemm(s.xn, D, b.qkv_w, D, b.qkv_b, (int)M, 3 * D, D, SGR_VIT_EPI_STORE_F16, s.qkv, 3 * D, nullptr, nullptr))) return rc;
    if (on() && (rc = launch_attention(s.qkv, B, T, heads, s.att, stream))) return rc;
    if (on() && (rc = gemm(s.att, D, b.proj_w, D, b.proj_b, (int)M, D, D, SGR_VIT_EPI_RESIDUAL, s.stream, D, nullptr, nullptr))) return rc;
    if (on() && (rc = launch_layernorm(s.stream, b.ln2_g, b.ln2_b, M, D, s.xn, stream))) return rc;
    if (on() && (rc = gemm(s.xn, D, b.fc1_w, D, b.fc1_b, (int)M, 4 * D, D, SGR_VIT_EPI_GELU_F16, s.hid, 4 * D, nullptr, nullptr))) return rc;
    if (on() && (rc = gemm(s.hid, 4 * D, b.fc2_w, 4 * D, b.fc2_b, (int)M, D, 4 * D, SGR_VIT_EPI_RESIDUAL, s.stream, D, tap, nullptr))) return rc;
  }
  for (int j = 0; j < 2; ++j) {
    float* rv = s.rv + (int64_t)j * B * D;
    // the class-token rows of the tap are T * D apart
    if (on() && (rc = gemm(s.tap[j], (int64_t)T * D, (const half_t*)wt->readout_w[j] + D, 2 * D, wt->readout_b[j], B, D, D, SGR_VIT_EPI_STORE_F32, rv, D,
                           nullptr, nullptr)))
      return rc;
    if (on() && (rc = gemm(s.tap[j], D, wt->readout_w[j], 2 * D, nullptr, (int)M, D, D, SGR_VIT_EPI_READOUT, call->out[j], 0, nullptr, rv))) return rc;
  }
  return SGR_OK;
}

}  // extern "C"
