// The convolution tile shared by the update operator (sgr_update.hip), the encoders (sgr_encoder.hip), the ResNet-V2 backbone
// (sgr_resnet.hip), the DPT decoder (sgr_dpt.hip) and LPIPS (sgr_lpips.hip): the k loop, the window gather of the four that read one
// channels-last map and the accumulator's layout; the pieces of the two norms that are the same in both; and the host helpers of
// these files and of sgr_vit.hip.  DESIGN.md section 3, "Update operator", describes the tile.
//
// The GEMM is D[n][m] = sum_k W[n][k] X[m][k] with m a pixel, n an output channel and k = tap * cin + channel: the weights are the A
// operand of mfma_f32_16x16x32_f16 and the pixels the B operand, so that a lane of the accumulator holds four consecutive output channels
// of one pixel.  One workgroup of kThreads: kBM pixels x BN output channels.  Wave v owns pixels [32v, 32v + 32) as two 16-wide B tiles
// and all BN / 16 A tiles, and acc[t][j][r] is output channel n0 + 16 t + 4 (lane >> 4) + r of pixel m0 + 32 v + 16 j + (lane & 15).
// Every sum has a fixed order (the MFMA k order, serial loops elsewhere): no atomics, bitwise reproducible.
#pragma once

#include <type_traits>

#include "sgr_common.h"

namespace sgr {
int set_error(int code, const char* fmt, ...);

typedef _Float16 half_t;
typedef __attribute__((ext_vector_type(4))) _Float16 half4;
typedef __attribute__((ext_vector_type(8))) _Float16 half8;
typedef __attribute__((ext_vector_type(4))) float floatx4;

constexpr int kThreads = 256;
constexpr int kBM = 128;                    // pixels of one workgroup: 4 waves x 2 tiles of 16
constexpr int kBK = 32;                     // one MFMA k step
constexpr int kRow = kBK + 8;               // halfs per LDS row: 80 bytes, so that the 16 rows of a fragment read spread over the banks
constexpr float kEps = 1e-5f;               // of the instance and the group norm

// The accumulator's layout, stated once: acc[t][j][r] is output channel acc_channel(n0, t) + r of pixel acc_pixel(j), n0 the first
// channel of the workgroup's tile.  The pixel counts from the workgroup's first, blockIdx.x * kBM: taken here and not as an argument,
// because the compiler folds the sum with its low bits in sight, as it did where every kernel spelled the sum out.
__device__ __forceinline__ int acc_pixel(int j) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, m0 = blockIdx.x * kBM;
  return m0 + wave * 32 + j * 16 + (lane & 15);
}
template <class T>                                          // T: int, or the int64_t of an element index that ends in the channel
__device__ __forceinline__ T acc_channel(T n0, int t) {
  const int tid = threadIdx.x, lane = tid & 63;
  return n0 + t * 16 + (lane >> 4) * 4;
}

// The KS x KS windows of the two pixel rows a thread stages (t >> 2 and 64 + (t >> 2) of the workgroup's kBM, see the k loop below) on
// channels-last maps of h x w pixels, src_stride halfs apart.  row(i, ...) places row i: output pixel p = oy * wo + ox of an image
// with output width wo, under a stride and pad_top rows and pad_left columns of zeros in front (oy is the caller's division, so that
// it stands where the caller has its other arithmetic on the pixel).  Which image a row belongs to is the caller's business alone
// (blockIdx.z, or m / HWo where a tile spans images): chunk takes the image's first pixel, and the map's geometry as the caller
// reads it out of its argument record at every call (a copy kept here lets the compiler hoist the 1x1 kernels' column test).
struct ConvWindow {
  int iy[2], ix[2];                                          // the window's origin in the image, may lie in the halo
  bool pv[2];                                                // false: a row past the end of the map
  __device__ __forceinline__ void row(int i, bool valid, int p, int oy, int wo, int stride, int pad_top, int pad_left) {
    pv[i] = valid;
    iy[i] = oy * stride - pad_top;
    ix[i] = (p - oy * wo) * stride - pad_left;
  }
  // the gather of conv_mma_mainloop: channels ch .. ch + 7 at tap (ty, tx) of row i, zeros for a halo; the halo test is on (y, x) of
  // the pixel's own map, so that a tile that spans images never reads a neighbour's pixels
  __device__ __forceinline__ half8 chunk(const half_t* image, int h, int w, int src_stride, int i, bool tv, int ty, int tx, int ch) const {
    const int yy = iy[i] + ty, xx = ix[i] + tx;
    half8 v = {0, 0, 0, 0, 0, 0, 0, 0};
    if (pv[i] && tv && (unsigned)yy < (unsigned)h && (unsigned)xx < (unsigned)w)
      v = *(const half8*)(image + ((int64_t)yy * w + xx) * src_stride + ch);
    return v;
  }
};

// The k loop of one workgroup: Xs [kBM][kRow], Ws [BN][kRow] in LDS, weight the packed [.][k_pad] rows, acc zeroed here.  Staging: thread
// t loads the 16-byte chunk k = 8 (t & 3) of pixel rows t >> 2 and 64 + (t >> 2) and of weight row n0 + (t >> 2) into registers one k step
// ahead of the MFMAs that consume the previous step out of LDS.  gather(i, tv, ty, tx, ch) returns the chunk of pixel row t >> 2 + 64 i at
// tap (ty, tx) of the KS x KS window, channels ch .. ch + 7, or zeros for a halo, a pixel past the end or, with tv false, the zero tail
// of a k_pad that is no multiple of the taps: which image, which stride and which padding is the caller's business alone.
// pre is a map over the gathered chunks, applied where they go to LDS: pre(chunk) runs one k step after the load that fetched the
// chunk, behind the MFMAs of the step before, so that the loads stay in flight (a map inside gather would wait for its load at once).
template <int KS, int BN, class Gather, class Pre>
__device__ __forceinline__ void conv_mma_mainloop(half_t* Xs, half_t* Ws, const half_t* weight, int n0, int k_pad, int cin, Gather&& gather,
                                                  Pre&& pre, floatx4 (&acc)[BN / 16][2]) {
  constexpr int NT = BN / 16;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int kc = tid & 3, srow = tid >> 2;
  const bool wv = tid < BN * 4;
  const half_t* wp = weight + (size_t)(n0 + (wv ? srow : 0)) * k_pad + kc * 8;

  int tap = (kc * 8) / cin, ch = (kc * 8) % cin;             // this thread's chunk of the current k step
  half8 xr[2], wr;
  auto gload = [&](int kt) {
    const int ty = tap / KS, tx = tap % KS;
    const bool tv = tap < KS * KS;
#pragma unroll
    for (int i = 0; i < 2; ++i) xr[i] = gather(i, tv, ty, tx, ch);
    if (wv) wr = *(const half8*)(wp + (size_t)kt * kBK);
  };

#pragma unroll
  for (int t = 0; t < NT; ++t)
#pragma unroll
    for (int j = 0; j < 2; ++j) acc[t][j] = floatx4{0.f, 0.f, 0.f, 0.f};

  const int nk = k_pad / kBK;
  gload(0);
  for (int kt = 0; kt < nk; ++kt) {
    *(half8*)&Xs[srow * kRow + kc * 8] = pre(xr[0]);
    *(half8*)&Xs[(srow + 64) * kRow + kc * 8] = pre(xr[1]);
    if (wv) *(half8*)&Ws[srow * kRow + kc * 8] = wr;
    __syncthreads();
    if (kt + 1 < nk) {
      ch += kBK;
      while (ch >= cin) {
        ch -= cin;
        ++tap;
      }
      gload(kt + 1);
    }
    half8 bf[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) bf[j] = *(const half8*)&Xs[(wave * 32 + j * 16 + (lane & 15)) * kRow + (lane >> 4) * 8];
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      const half8 af = *(const half8*)&Ws[(t * 16 + (lane & 15)) * kRow + (lane >> 4) * 8];
#pragma unroll
      for (int j = 0; j < 2; ++j) acc[t][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(af, bf[j], acc[t][j], 0, 0, 0);
    }
    __syncthreads();
  }
}

// the k loop without a map
template <int KS, int BN, class Gather>
__device__ __forceinline__ void conv_mma_mainloop(half_t* Xs, half_t* Ws, const half_t* weight, int n0, int k_pad, int cin, Gather&& gather,
                                                  floatx4 (&acc)[BN / 16][2]) {
  conv_mma_mainloop<KS, BN>(Xs, Ws, weight, n0, k_pad, cin, gather, [](half8 v) { return v; }, acc);
}

// The shifted sums of a tile for a norm: with d = acc - shift_of(n) over the valid pixels, red[0][wave][n] = S1 = sum d and
// red[1][wave][n] = S2 = sum d^2 of channel n of the tile (n in 0 .. BN - 1) over the wave's 32 pixels, the 16 pixel lanes summed by a
// butterfly.  The caller chooses the shift, puts a barrier behind this and folds the four waves of red.
template <int BN, class Shift>
__device__ __forceinline__ void tile_shifted_sums(const floatx4 (&acc)[BN / 16][2], const bool (&valid)[2], Shift&& shift_of,
                                                  float (&red)[2][4][BN]) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int t = 0; t < BN / 16; ++t)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int n = acc_channel(0, t) + r;
      const float sh = shift_of(n);
      const float d0 = valid[0] ? acc[t][0][r] - sh : 0.f, d1 = valid[1] ? acc[t][1][r] - sh : 0.f;
      float s1 = d0 + d1, s2 = d0 * d0 + d1 * d1;
#pragma unroll
      for (int d = 1; d < 16; d <<= 1) {
        s1 += __shfl_xor(s1, d);
        s2 += __shfl_xor(s2, d);
      }
      if ((lane & 15) == 0) {
        red[0][wave][n] = s1;
        red[1][wave][n] = s2;
      }
    }
}

// The merge of the per-tile statistics {count, shift, S1, S2} of one image, st [tiles][G], by a whole workgroup in fp64 about s0, the
// shift of tile 0: with d = s_i - s0, A = sum (n_i d + S1_i) and B = sum (S2_i + 2 d S1_i + n_i d^2) are the sums of (v - s0) and
// (v - s0)^2 over the N elements of a statistic, so mean = s0 + A / N and M2 = B - A^2 / N.  Thread (slot, g) takes the tiles slot,
// slot + S, ... (S = kThreads / G) in ascending order, the slots are then added in ascending order: the result depends on the map
// alone.  mu[g] = mean and rs[g] = 1 / sqrt(M2 / N + eps) are rounded once to fp32; a barrier follows.  pa, pb: kThreads doubles of LDS.
__device__ __forceinline__ void merge_tile_stats(const floatx4* st, int tiles, int G, double N, double* pa, double* pb, float* mu, float* rs) {
  const int tid = threadIdx.x, g = tid % G, slot = tid / G, S = kThreads / G;
  const double s0 = (double)st[g][1];
  double A = 0.0, B = 0.0;
  if (slot < S)
    for (int t = slot; t < tiles; t += S) {
      const floatx4 q = st[(int64_t)t * G + g];
      const double n = q[0], d = (double)q[1] - s0, s1 = q[2], s2 = q[3];
      A += n * d + s1;
      B += s2 + 2.0 * d * s1 + n * d * d;
    }
  pa[tid] = A;
  pb[tid] = B;
  __syncthreads();
  if (tid < G) {
    for (int s = 1; s < S; ++s) {
      A += pa[s * G + tid];
      B += pb[s * G + tid];
    }
    const double mean = s0 + A / N, var = fmax((B - A * A / N) / N, 0.0);
    mu[tid] = (float)mean;
    rs[tid] = (float)(1.0 / sqrt(var + (double)kEps));
  }
  __syncthreads();
}

// v = output channels nb .. nb + 3 of pixel p of image img (gm = img * HW + p) under the four SGR_UPDATE_OUT_* kinds
__device__ __forceinline__ void store_out4(void* out, int out_kind, int out_stride, const floatx4& v, int64_t gm, int img, int p, int nb, int cout,
                                           int HW) {
  switch (out_kind) {
    case SGR_UPDATE_OUT_CL_F16: {
      half4 o;
#pragma unroll
      for (int r = 0; r < 4; ++r) o[r] = (half_t)v[r];
      *(half4*)&((half_t*)out)[gm * out_stride + nb] = o;
      break;
    }
    case SGR_UPDATE_OUT_CL_F32: *(floatx4*)&((float*)out)[gm * out_stride + nb] = v; break;
    case SGR_UPDATE_OUT_NCHW_F16:
#pragma unroll
      for (int r = 0; r < 4; ++r) ((half_t*)out)[((int64_t)img * cout + nb + r) * HW + p] = (half_t)v[r];
      break;
    default:
#pragma unroll
      for (int r = 0; r < 4; ++r) ((float*)out)[((int64_t)img * cout + nb + r) * HW + p] = v[r];
      break;
  }
}

// ---- host helpers
inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }
inline int round_up(int v, int m) { return (v + m - 1) / m * m; }
inline int tiles_of(int64_t hw) { return (int)((hw + kBM - 1) / kBM); }
inline bool map_ok(int n, int h, int w) { return n >= 1 && n <= 65535 && h >= 1 && w >= 1 && (int64_t)h * w <= 0x7fffffff - kBM; }

// behind a kernel launch: SGR_OK, or the error "<what> launch failed"
inline int launched(const char* what) { return hipGetLastError() == hipSuccess ? SGR_OK : set_error(SGR_ERR_HIP, "%s launch failed", what); }

// The launches of a forward are numbered in the order of its list; on() counts one and says whether it lies in first..last of the call.
struct LaunchRange {
  int first, last, launch = -1;
  bool operator()() {
    ++launch;
    return launch >= first && launch <= last;
  }
};

// What every convolution record says of its operands, under the caller's name `who`: src channels-last with cin channels of a pixel
// src_stride halfs apart, weight the packed fp16 [rows][k_pad] with k_pad = ksize^2 cin rounded up to the k step, bias (may be null)
// read four floats at a time.  Sets k_pad.
inline int check_conv_operands(const char* who, const void* src, int src_stride, int cin, int ksize, const void* weight, int64_t weight_elems,
                               int rows, const void* bias, int& k_pad) {
  if (src_stride < cin || src_stride % 8 || !aligned16(src))
    return set_error(SGR_ERR_INVALID, "%s: src needs a 16-byte aligned base and a stride (%d) that is a multiple of 8 and >= %d", who, src_stride,
                     cin);
  k_pad = round_up(ksize * ksize * cin, kBK);
  if (weight_elems < (int64_t)rows * k_pad || !aligned16(weight) || !aligned16(bias))
    return set_error(SGR_ERR_INVALID, "%s: packed weights must be 16-byte aligned [%d][%d] fp16, got %lld elements", who, rows, k_pad,
                     (long long)weight_elems);
  return SGR_OK;
}

// Carves a scratch buffer into 256-byte aligned pieces; with a null base only the size is counted.
struct Carver {
  void* base;
  size_t off = 0;
  void* take(size_t nbytes) {
    void* p = base ? (char*)base + off : nullptr;
    off += align_up(nbytes);
    return p;
  }
};

// launch(integral_constant<KS>, integral_constant<BN>) for the kernel size (1, 3, else 7) and the one of BNs that equals bn
template <int... BNs, class Launch>
inline void dispatch_conv(int ksize, int bn, Launch&& launch) {
  auto by_bn = [&](auto ks) { (void)((bn == BNs && (launch(ks, std::integral_constant<int, BNs>{}), true)) || ...); };
  if (ksize == 1)
    by_bn(std::integral_constant<int, 1>{});
  else if (ksize == 3)
    by_bn(std::integral_constant<int, 3>{});
  else
    by_bn(std::integral_constant<int, 7>{});
}

}  // namespace sgr
