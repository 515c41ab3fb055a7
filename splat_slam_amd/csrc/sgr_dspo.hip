// Stage 2 ("depth_scale") of the tracker's DSPO bundle adjustment: the disparities of every frame an edge starts from and one
// scale and shift per frame that tie the mono-depth prior to them, poses fixed (BA_with_scale_shift of the reference's
// thirdparty/glorie_slam/geom/ba.py, reached from DepthVideo.dspo, thirdparty/glorie_slam/depth_video.py:236-299), and the weighted
// least-squares alignment that initialises the scales and shifts (align_scale_and_shift, src/utils/common.py:68-104).
//   sgr_dspo_align   per frame: scale, shift and mean absolute error of scale * prediction + shift against target
//   sgr_dspo_ba      Gauss-Newton over disparities, scales and shifts
// The algorithm, the kernels and the precision of every sum are described in DESIGN.md section 3, "DSPO stage 2".  Every sum is a
// fixed-order register / wave-butterfly / LDS reduction: no atomics, bitwise reproducible.  One call is stream-ordered from its first
// launch to its last, with no host synchronisation.
#include <algorithm>
#include <cmath>
#include <cstdint>

#include "sgr_common.h"
#include "sgr_dba_device.h"

namespace sgr {
int set_error(int code, const char* fmt, ...);

namespace {

using namespace dba;

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr float kMinDepth = 0.2f;           // MIN_DEPTH of the reference's Python projection (geom/projective_ops.py); sgr_dba uses 0.25
constexpr float kWeightScale = 0.001f;
constexpr float kMonoMin = 1e-6f;           // a mono disparity below this carries no prior
constexpr float kValidGain = 10.f;          // weight of the prior on pixels of the two-view consistency mask
constexpr int kSums = 7;                    // per-frame sums of the reduced 2 x 2 system (see system_kernel)
constexpr int kStatusBadM = 1;              // number of distinct depth frames differs from eta.shape[0]


__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
  return v;
}

// Sums v[0..NV) over the workgroup in fp64: butterfly per wave, then the kWaves partials in wave order.  The result is valid in
// red[0..NV) for every thread after the call.  red holds kWaves * NV doubles.
template <int NV>
__device__ __forceinline__ void block_sum_f64(double (&v)[NV], double* red) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const double s = wave_sum_f64(v[i]);
    if (lane == 0) red[w * NV + i] = s;
  }
  __syncthreads();
  double tot = 0.0;
  if ((int)threadIdx.x < NV) {
    tot = red[threadIdx.x];
    for (int k = 1; k < kWaves; ++k) tot += red[k * NV + threadIdx.x];
  }
  __syncthreads();
  if ((int)threadIdx.x < NV) red[threadIdx.x] = tot;
  __syncthreads();
}

// ================================================================================================================================
// align: one workgroup per frame, every sum in fp64
// ================================================================================================================================

__device__ __forceinline__ float weight_at(const void* w, int kind, size_t i) {
  if (kind == SGR_DSPO_WEIGHTS_F32) return ((const float*)w)[i];
  if (kind == SGR_DSPO_WEIGHTS_U8) return ((const uint8_t*)w)[i] ? 1.f : 0.f;
  return 1.f;
}

__global__ void __launch_bounds__(kThreads) align_kernel(int P, const float* __restrict__ pred, const float* __restrict__ target,
                                                         const void* __restrict__ weights, int kind, float* __restrict__ out) {
  __shared__ double red[kWaves * 5];
  const size_t fo = (size_t)blockIdx.x * P;
  double a[5] = {0.0, 0.0, 0.0, 0.0, 0.0};      // a00, a01, a11, b0, b1
  for (int p = threadIdx.x; p < P; p += kThreads) {
    const double w = (double)weight_at(weights, kind, fo + p), x = (double)pred[fo + p], y = (double)target[fo + p];
    a[0] += w * x * x;
    a[1] += w * x;
    a[2] += w;
    a[3] += w * x * y;
    a[4] += w * y;
  }
  block_sum_f64<5>(a, red);
  const double a00 = red[0], a01 = red[1], a11 = red[2], b0 = red[3], b1 = red[4];
  __syncthreads();
  const double det = a00 * a11 - a01 * a01;
  const double s = (a11 * b0 - a01 * b1) / det, q = (-a01 * b0 + a00 * b1) / det;
  double e[1] = {0.0};
  for (int p = threadIdx.x; p < P; p += kThreads) {
    const double w = (double)weight_at(weights, kind, fo + p), x = (double)pred[fo + p], y = (double)target[fo + p];
    e[0] += w * fabs(s * x + q - y);
  }
  block_sum_f64<1>(e, red);
  if (threadIdx.x == 0) {
    out[3 * blockIdx.x] = (float)s;
    out[3 * blockIdx.x + 1] = (float)q;
    out[3 * blockIdx.x + 2] = (float)(red[0] / a11);
  }
}

// ================================================================================================================================
// ba: graph structure and relative poses (once per call).  nv = frames that exist in both poses and disps; edges whose ii or jj
// lies outside [0, nv) take part in nothing.
// ================================================================================================================================

struct __attribute__((aligned(32))) EdgePose {
  float t[3];
  float q[4];
  int e;
};

// One int per edge: 2 * ii[e] + kept, or -1 for an edge with a frame outside [0, nv).  Both passes over the edge list below stage
// these codes in LDS a tile at a time and let every thread walk the tile (a broadcast read), instead of a serial walk of global memory.
__device__ __forceinline__ int edge_code(int nv, int E, const int64_t* __restrict__ ii, const int64_t* __restrict__ jj,
                                         const uint8_t* __restrict__ keep, int e) {
  if (e >= E) return -1;
  const int64_t a = ii[e], b = jj[e];
  if (!(frame_ok(a, nv) && frame_ok(b, nv))) return -1;
  return 2 * (int)a + ((!keep || keep[e]) ? 1 : 0);
}

// flag[f]: some edge starts from f (f is a depth frame);  cnt[f]: the kept edges that start from f
__global__ void __launch_bounds__(kThreads) mark_kernel(int nv, int E, const int64_t* __restrict__ ii, const int64_t* __restrict__ jj,
                                                        const uint8_t* __restrict__ keep, int* __restrict__ flag,
                                                        int* __restrict__ cnt) {
  __shared__ int code[kThreads];
  const int f = blockIdx.x * kThreads + threadIdx.x;
  int all = 0, kept = 0;
  for (int e0 = 0; e0 < E; e0 += kThreads) {
    code[threadIdx.x] = edge_code(nv, E, ii, jj, keep, e0 + threadIdx.x);
    __syncthreads();
    const int m = min(kThreads, E - e0);
    for (int n = 0; n < m; ++n) {
      const int c = code[n];
      all += (c >> 1) == f;                    // (-1 >> 1 = -1: never a frame)
      kept += c == 2 * f + 1;
    }
    __syncthreads();
  }
  if (f >= nv) return;
  flag[f] = all > 0;
  cnt[f] = kept;
}

// kx[row] = f for the depth frames in ascending order;  CSR offsets of the kept edges by ii;  status
__global__ void __launch_bounds__(1024) scan_kernel(int nv, int M, int* __restrict__ flag, int* __restrict__ rank, int* __restrict__ kx,
                                                    int* __restrict__ cnt, int* __restrict__ ptr, int* __restrict__ status) {
  __shared__ int lds[1024];
  const int nk = scan_1024(nv, flag, rank, lds);
  __syncthreads();
  for (int f = threadIdx.x; f < nv; f += 1024) {
    const int r = rank[f];
    if (flag[f] && r < M) kx[r] = f;
  }
  __syncthreads();
  scan_1024(nv, cnt, ptr, lds);
  if (threadIdx.x == 0) status[0] = nk != M ? kStatusBadM : 0;
}

// the kept edges of every frame in edge order, each with its relative pose Gij = Gj Gi^-1 (poses do not change during the call):
// one thread per edge, whose place in its frame's run is the number of kept edges of that frame before it
__global__ void __launch_bounds__(kThreads) fill_kernel(int nv, int E, const int64_t* __restrict__ ii, const int64_t* __restrict__ jj,
                                                        const uint8_t* __restrict__ keep, const float* __restrict__ poses,
                                                        const int* __restrict__ ptr, EdgePose* __restrict__ edges) {
  __shared__ int code[kThreads];
  const int e = blockIdx.x * kThreads + threadIdx.x;
  const int mine = edge_code(nv, E, ii, jj, keep, e);
  const int last = min(E, (int)(blockIdx.x + 1) * kThreads);        // edges at or beyond it come after every edge of this workgroup
  int before = 0;
  for (int e0 = 0; e0 < last; e0 += kThreads) {
    code[threadIdx.x] = edge_code(nv, E, ii, jj, keep, e0 + threadIdx.x);
    __syncthreads();
    const int m = min(kThreads, last - e0);
    for (int n = 0; n < m; ++n) before += (code[n] == mine) && (e0 + n < e);
    __syncthreads();
  }
  if (mine < 0 || !(mine & 1)) return;
  const int64_t a = ii[e], b = jj[e];
  EdgePose g = {{kStereoBaseline, 0.f, 0.f}, {0.f, 0.f, 0.f, 1.f}, e};
  if (a != b) rel_se3(poses + 7 * a, poses + 7 * b, g.t, g.q);
  edges[ptr[a] + before] = g;
}

// ================================================================================================================================
// ba: one Gauss-Newton iteration = system_kernel + update_kernel
// ================================================================================================================================

// Per (depth row k, pixel): the edge terms of every kept edge from frame kx[k] in edge order, the mono-prior terms, the per-pixel
// system, and this workgroup's share of the frame's sums.  With cpe = C_proj + eta, C = cpe + Jd^2 and Q = 1 / C, the reduced
// system of the frame is formed per pixel BEFORE it is summed, so that no sum cancels against another:
//   S = H~ - sum Q E E^T = sum [Js Jq]^T [Js Jq] (Q cpe) + diag(ep + lm H_diag)          (1 - Q Jd^2 = Q cpe)
//   g = u  - sum Q E b   = -sum [Js Jq] Q (rd cpe + Jd b_proj)
// which leaves seven sums: H00, H11 (for the damping), the three of S and the two of g.  Stored per pixel: Q b, Q E0, Q E1.
__global__ void __launch_bounds__(kThreads) system_kernel(int P, int wd, int nb, const float2* __restrict__ targets,
                                                          const float2* __restrict__ weights, const float* __restrict__ disps,
                                                          const float* __restrict__ intr, const float* __restrict__ mono,
                                                          const uint8_t* __restrict__ vmask, const float* __restrict__ scales,
                                                          const float* __restrict__ shifts, const float* __restrict__ eta,
                                                          const int* __restrict__ kx, const int* __restrict__ ptr,
                                                          const EdgePose* __restrict__ edges, const int* __restrict__ status,
                                                          int ignore_frames, float sqrt_alpha, float* __restrict__ QB,
                                                          double* __restrict__ partial) {
  __shared__ double red[kWaves * kSums];
  if (status[0]) return;
  const int k = blockIdx.y, f = kx[k];
  const int lo = ptr[f], hi = ptr[f + 1];
  if (lo == hi) return;                       // inactive: every edge from f was masked out
  const int p = blockIdx.x * kThreads + threadIdx.x;
  double v[kSums];
#pragma unroll
  for (int l = 0; l < kSums; ++l) v[l] = 0.0;
  if (p < P) {
    const Intr K = load_intr(intr);
    const size_t fo = (size_t)f * P + p, ko = (size_t)k * P + p;
    const int i = p / wd, j = p - (p / wd) * wd;
    const float h = disps[fo];
    const float Xi[4] = {((float)j - K.cx) / K.fx, ((float)i - K.cy) / K.fy, 1.f, h};
    float c = 0.f, b = 0.f;
#pragma unroll 2
    for (int n = lo; n < hi; ++n) {
      const EdgePose g = edges[n];
      const float2 tg = targets[(size_t)g.e * P + p], wt = weights[(size_t)g.e * P + p];
      float X[4];
      act_se3(g.t, g.q, Xi, X);
      const bool front = X[2] > kMinDepth;
      const float d = front ? 1.f / X[2] : 0.f, d2 = d * d;
      const float wx = front ? kWeightScale * wt.x : 0.f, wy = front ? kWeightScale * wt.y : 0.f;
      const float rx = tg.x - (K.fx * d * X[0] + K.cx), ry = tg.y - (K.fy * d * X[1] + K.cy);
      const float jx = K.fx * (g.t[0] * d - g.t[2] * (X[0] * d2)), jy = K.fy * (g.t[1] * d - g.t[2] * (X[1] * d2));
      c += wx * jx * jx;
      b += wx * rx * jx;
      c += wy * jy * jy;
      b += wy * ry * jy;
    }
    const float m = mono[fo];
    const bool vd = vmask[fo] != 0, invalid = (m < kMonoMin) || (f < ignore_frames);
    const float a = sqrt_alpha * (vd ? kValidGain : 1.f);
    const float Jd = (invalid && vd) ? 0.f : a;
    const float Js = invalid ? 0.f : -m * a, Jq = invalid ? 0.f : -a;
    const float rd = sqrt_alpha * (h - (scales[f] * m + shifts[f]));
    const float cpe = c + eta[ko];
    const float Q = 1.f / (cpe + Jd * Jd);
    const float bb = b - Jd * rd;
    const size_t qo = (size_t)k * 3 * P + p;
    QB[qo] = Q * bb;
    QB[qo + P] = Q * (Js * Jd);
    QB[qo + 2 * (size_t)P] = Q * (Jq * Jd);
    const double js = (double)Js, jq = (double)Jq, q = (double)Q;
    const double qc = q * (double)cpe;
    const double gr = q * ((double)rd * (double)cpe + (double)Jd * (double)b);
    v[0] = js * js;
    v[1] = jq * jq;
    v[2] = js * js * qc;
    v[3] = js * jq * qc;
    v[4] = jq * jq * qc;
    v[5] = -js * gr;
    v[6] = -jq * gr;
  }
  block_sum_f64<kSums>(v, red);
  if (threadIdx.x < kSums) partial[((size_t)k * nb + blockIdx.x) * kSums + threadIdx.x] = red[threadIdx.x];
}

// Per depth row: the frame's sums from the workgroup partials in block order, the damped 2 x 2 system solved by Cholesky in fp64
// (not positive definite: dwq = 0 for THIS frame), dz = Q (b - E^T dwq), disps = max(disps + dz, 0), scales += dwq0, shifts += dwq1.
// Every workgroup of a row repeats the row's solve; the first one writes dwq and moves the scale and the shift.
__global__ void __launch_bounds__(kThreads) update_kernel(int P, int nb, float lm, float ep, const int* __restrict__ kx,
                                                          const int* __restrict__ ptr, const float* __restrict__ QB,
                                                          const double* __restrict__ partial, const int* __restrict__ status,
                                                          float* __restrict__ disps, float* __restrict__ scales,
                                                          float* __restrict__ shifts, float* __restrict__ dwq, float* __restrict__ dz) {
  __shared__ double sums[kSums];
  __shared__ float step[2];
  const int k = blockIdx.y, p = blockIdx.x * kThreads + threadIdx.x;
  const size_t ko = (size_t)k * P + p;
  const bool first = blockIdx.x == 0 && threadIdx.x == 0;
  if (status[0]) {
    if (p < P) dz[ko] = NAN;
    if (first) dwq[2 * k] = dwq[2 * k + 1] = NAN;
    return;
  }
  const int f = kx[k];
  if (ptr[f] == ptr[f + 1]) {
    if (p < P) dz[ko] = 0.f;
    if (first) dwq[2 * k] = dwq[2 * k + 1] = 0.f;
    return;
  }
  if (threadIdx.x < kSums) {
    const double* src = partial + (size_t)k * nb * kSums + threadIdx.x;
    double s = src[0];
    for (int n = 1; n < nb; ++n) s += src[(size_t)n * kSums];
    sums[threadIdx.x] = s;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    const double s00 = sums[2] + (double)ep + (double)lm * sums[0], s01 = sums[3], s11 = sums[4] + (double)ep + (double)lm * sums[1];
    double x0 = 0.0, x1 = 0.0;
    if (s00 > 0.0) {
      const double l00 = sqrt(s00), l10 = s01 / l00, dd = s11 - l10 * l10;
      if (dd > 0.0) {
        const double l11 = sqrt(dd);
        const double y0 = sums[5] / l00, y1 = (sums[6] - l10 * y0) / l11;
        x1 = y1 / l11;
        x0 = (y0 - l10 * x1) / l00;
      }
    }
    step[0] = (float)x0;
    step[1] = (float)x1;
  }
  __syncthreads();
  const float d0 = step[0], d1 = step[1];
  if (p < P) {
    const size_t qo = (size_t)k * 3 * P + p, fo = (size_t)f * P + p;
    const float d = QB[qo] - (QB[qo + P] * d0 + QB[qo + 2 * (size_t)P] * d1);
    dz[ko] = d;
    disps[fo] = fmaxf(disps[fo] + d, 0.f);
  }
  if (first) {
    dwq[2 * k] = d0;
    dwq[2 * k + 1] = d1;
    scales[f] += d0;
    shifts[f] += d1;
  }
}

// ---- scratch layout of ba
struct DspoScratch {
  int *flag, *rank, *kx, *cnt, *ptr, *status;
  EdgePose* edges;
  float* QB;
  double* partial;
};

size_t carve(int nv, int E, int M, int P, char* base, DspoScratch* s) {
  size_t off = 0;
  auto take = [&](size_t bytes) {
    char* p = base ? base + off : nullptr;
    off += align_up(bytes);
    return p;
  };
  const size_t i4 = sizeof(int);
  DspoScratch d;
  d.flag = (int*)take((size_t)nv * i4);
  d.rank = (int*)take((size_t)(nv + 1) * i4);
  d.kx = (int*)take((size_t)M * i4);
  d.cnt = (int*)take((size_t)nv * i4);
  d.ptr = (int*)take((size_t)(nv + 1) * i4);
  d.status = (int*)take(i4);
  d.edges = (EdgePose*)take((size_t)E * sizeof(EdgePose));
  d.QB = (float*)take((size_t)M * 3 * P * sizeof(float));
  d.partial = (double*)take((size_t)M * blocks_for(P) * kSums * sizeof(double));
  if (s) *s = d;
  return off;
}

bool sizes_ok(int nv, int E, int M, int ht, int wd) {
  return nv > 0 && nv < (1 << 30) && E > 0 && M > 0 && M <= 65535 && ht > 0 && wd > 0 && (long long)ht * wd < (1LL << 26) &&
         (long long)E * ht * wd < (1LL << 40);
}

}  // namespace
}  // namespace sgr

using namespace sgr;

extern "C" {

int sgr_dspo_align(const float* prediction, const float* target, const void* weights, int32_t weights_kind, int32_t num, int32_t pixels,
                   float* out, void* stream) {
  if (!prediction || !target || !out || num < 0 || pixels <= 0 || weights_kind < SGR_DSPO_WEIGHTS_NONE ||
      weights_kind > SGR_DSPO_WEIGHTS_U8 || (weights_kind != SGR_DSPO_WEIGHTS_NONE && !weights))
    return set_error(SGR_ERR_INVALID, "dspo_align: bad arguments");
  if (num == 0) return SGR_OK;
  hipLaunchKernelGGL(align_kernel, dim3(num), dim3(kThreads), 0, (hipStream_t)stream, pixels, prediction, target, weights, weights_kind,
                     out);
  return hipGetLastError() == hipSuccess ? SGR_OK : set_error(SGR_ERR_HIP, "dspo_align launch failed");
}

size_t sgr_dspo_scratch_bytes(int32_t num_frames, int32_t num_edges, int32_t num_depth, int32_t ht, int32_t wd) {
  if (!sizes_ok(num_frames, num_edges, num_depth, ht, wd)) return 0;
  return carve(num_frames, num_edges, num_depth, ht * wd, nullptr, nullptr);
}

int sgr_dspo_ba(const SgrDspoProblem* pr, void* scratch, size_t scratch_bytes, void* stream) {
  if (!pr || !pr->poses || !pr->disps || !pr->intrinsics || !pr->mono_disps || !pr->valid_depth_mask || !pr->scales || !pr->shifts ||
      !pr->targets || !pr->weights || !pr->eta || !pr->ii || !pr->jj || !pr->dwq || !pr->dz)
    return set_error(SGR_ERR_INVALID, "dspo_ba: null argument");
  const int nv = std::min(pr->num_poses, pr->num_frames), E = pr->num_edges, M = pr->num_depth, ht = pr->ht, wd = pr->wd, P = ht * wd;
  if (!sizes_ok(nv, E, M, ht, wd) || pr->iterations < 0 || !(pr->alpha >= 0.f))
    return set_error(SGR_ERR_INVALID, "dspo_ba: bad sizes (frames=%d edges=%d M=%d ht=%d wd=%d iterations=%d alpha=%g)", nv, E, M, ht, wd,
                     pr->iterations, (double)pr->alpha);
  if (!scratch || scratch_bytes < carve(nv, E, M, P, nullptr, nullptr)) return set_error(SGR_ERR_WORKSPACE, "dspo_ba: scratch too small");
  DspoScratch s;
  carve(nv, E, M, P, (char*)scratch, &s);
  hipStream_t st = (hipStream_t)stream;
  const float sqrt_alpha = (float)std::sqrt((double)pr->alpha);
  const int nb = blocks_for(P);

  hipLaunchKernelGGL(mark_kernel, dim3(blocks_for(nv)), dim3(kThreads), 0, st, nv, E, pr->ii, pr->jj, pr->edge_keep, s.flag, s.cnt);
  hipLaunchKernelGGL(scan_kernel, dim3(1), dim3(1024), 0, st, nv, M, s.flag, s.rank, s.kx, s.cnt, s.ptr, s.status);
  hipLaunchKernelGGL(fill_kernel, dim3(blocks_for(E)), dim3(kThreads), 0, st, nv, E, pr->ii, pr->jj, pr->edge_keep, pr->poses, s.ptr,
                     s.edges);
  for (int it = 0; it < pr->iterations; ++it) {
    hipLaunchKernelGGL(system_kernel, dim3(nb, M), dim3(kThreads), 0, st, P, wd, nb, (const float2*)pr->targets,
                       (const float2*)pr->weights, pr->disps, pr->intrinsics, pr->mono_disps, pr->valid_depth_mask, pr->scales,
                       pr->shifts, pr->eta, s.kx, s.ptr, s.edges, s.status, pr->ignore_frames, sqrt_alpha, s.QB, s.partial);
    hipLaunchKernelGGL(update_kernel, dim3(nb, M), dim3(kThreads), 0, st, P, nb, pr->lm, pr->ep, s.kx, s.ptr, s.QB, s.partial, s.status,
                       pr->disps, pr->scales, pr->shifts, pr->dwq, pr->dz);
  }
  return hipGetLastError() == hipSuccess ? SGR_OK : set_error(SGR_ERR_HIP, "dspo_ba launch failed");
}

}  // extern "C"
