// Dense bundle adjustment and frame geometry of the tracker: the droid_backends extension of the reference
// (thirdparty/glorie_slam/lib/droid_kernels.cu), reached from DepthVideo (thirdparty/glorie_slam/depth_video.py).
//   sgr_dba_ba              ba: Gauss-Newton over poses [t0, t1) and the disparities of every frame an edge starts from
//   sgr_dba_frame_distance  frame_distance: mean optical flow of an edge, 1000 when too few points stay in front
//   sgr_dba_projmap         projmap: reprojected pixel coordinates and the MIN_DEPTH validity of every edge
//   sgr_dba_iproj           iproj: back-projection of every disparity map to world points
//   sgr_dba_depth_filter    depth_filter: per pixel, how many of the six neighbouring frames agree with its depth
// Layout, reductions, the solve and its size limit are described in DESIGN.md section 3, "Dense bundle adjustment".  Every sum is
// a fixed-order register / wave-butterfly / LDS reduction and every scatter is a gather: no atomics, bitwise reproducible.  One ba
// call is stream-ordered from its first launch to its last, with no host synchronisation.
#include <algorithm>
#include <cmath>
#include <cstdint>

#include "sgr_common.h"
#include "sgr_dba_device.h"

namespace sgr {
int set_error(int code, const char* fmt, ...);

namespace {

using namespace dba;      // SE3 on (t, q xyzw), intrinsics, scan_1024: shared with sgr_dspo.hip

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr float kMinDepth = 0.25f;          // MIN_DEPTH of the reference
constexpr float kSensorAlpha = 0.05f;       // weight of the depth-sensor prior where disps_sens > 0
constexpr int kMaxWindow = SGR_DBA_MAX_WINDOW;     // t1 - t0: reduced system of at most 3072 x 3072 (fp64)
constexpr int kMaxEdges = 65535 - kMaxWindow;   // the slot launch spans T + E workgroup rows
constexpr int kNb = 64;                     // Cholesky block
constexpr int kHs = 4 * 36 + 12;            // per edge: Hii, Hij, Hji, Hjj (6x6 each), vi, vj
constexpr int kStatusBadK = 1;              // number of distinct depth frames differs from eta.shape[0]


// ---- SE3 on (t, q xyzw), fp32 as in the reference (act_so3, act_se3, rel_se3: sgr_dba_device.h)
// Y = Adj(T)^T X for a 6-vector (translation part first)
__device__ __forceinline__ void adjT_se3(const float* t, const float* q, const float* X, float* Y) {
  const float qinv[4] = {-q[0], -q[1], -q[2], q[3]};
  act_so3(qinv, X, Y);
  act_so3(qinv, X + 3, Y + 3);
  const float u[3] = {t[2] * X[1] - t[1] * X[2], t[0] * X[2] - t[2] * X[0], t[1] * X[0] - t[0] * X[1]};
  float v[3];
  act_so3(qinv, u, v);
  Y[3] += v[0];
  Y[4] += v[1];
  Y[5] += v[2];
}

__device__ __forceinline__ void cross_inplace(const float* a, float* b) {
  const float x0 = a[1] * b[2] - a[2] * b[1], x1 = a[2] * b[0] - a[0] * b[2], x2 = a[0] * b[1] - a[1] * b[0];
  b[0] = x0;
  b[1] = x1;
  b[2] = x2;
}

__device__ __forceinline__ void exp_se3(const float* xi, float* t, float* q) {
  const float* phi = xi + 3;
  const float th2 = phi[0] * phi[0] + phi[1] * phi[1] + phi[2] * phi[2];
  const float th = sqrtf(th2);
  float imag, real;
  if (th2 < 1e-8f) {
    const float th4 = th2 * th2;
    imag = 0.5f - (1.f / 48.f) * th2 + (1.f / 3840.f) * th4;
    real = 1.f - (1.f / 8.f) * th2 + (1.f / 384.f) * th4;
  } else {
    imag = sinf(0.5f * th) / th;
    real = cosf(0.5f * th);
  }
  q[0] = imag * phi[0];
  q[1] = imag * phi[1];
  q[2] = imag * phi[2];
  q[3] = real;
  float tau[3] = {xi[0], xi[1], xi[2]};
  t[0] = tau[0];
  t[1] = tau[1];
  t[2] = tau[2];
  if (th > 1e-4f) {
    const float a = (1.f - cosf(th)) / th2;
    cross_inplace(phi, tau);
    t[0] += a * tau[0];
    t[1] += a * tau[1];
    t[2] += a * tau[2];
    const float b = (th - sinf(th)) / (th * th2);
    cross_inplace(phi, tau);
    t[0] += b * tau[0];
    t[1] += b * tau[1];
    t[2] += b * tau[2];
  }
}

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
  return v;
}

// Sums v[0..NV) over the workgroup: butterfly per wave, then the kWaves partials in wave order.  The result is valid in red[0..NV)
// for every thread after the call.  red holds kWaves * NV floats.
template <int NV>
__device__ __forceinline__ void block_sum(float (&v)[NV], float* red) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const float s = wave_sum(v[i]);
    if (lane == 0) red[w * NV + i] = s;
  }
  __syncthreads();
  float tot = 0.f;
  if ((int)threadIdx.x < NV) {
    tot = red[threadIdx.x];
    for (int k = 1; k < kWaves; ++k) tot += red[k * NV + threadIdx.x];
  }
  __syncthreads();
  if ((int)threadIdx.x < NV) red[threadIdx.x] = tot;
  __syncthreads();
}

// ================================================================================================================================
// ba: graph structure (once per call).  nv = frames that exist in both poses and disps; edges whose ii or jj lies outside [0, nv)
// take part in nothing.
// ================================================================================================================================

// flag[f]: frame f has a disparity row (f in [t0, t1) or f = some ii);  cnt_ii / cnt_jj: edges leaving / entering f
__global__ void __launch_bounds__(kThreads) mark_kernel(int nv, int E, const int64_t* __restrict__ ii, const int64_t* __restrict__ jj,
                                                        int t0, int t1, int* __restrict__ flag, int* __restrict__ cnt_ii,
                                                        int* __restrict__ cnt_jj) {
  const int f = blockIdx.x * kThreads + threadIdx.x;
  if (f >= nv) return;
  int fl = (f >= t0 && f < t1), ci = 0, cj = 0;
  for (int e = 0; e < E; ++e) {
    const int64_t a = ii[e], b = jj[e];
    const bool ok = frame_ok(a, nv) && frame_ok(b, nv);
    ci += (ok && a == f);
    cj += (ok && b == f);
  }
  flag[f] = fl | (ci > 0);
  cnt_ii[f] = ci;
  cnt_jj[f] = cj;
}

// rank[f] = row of frame f in the depth arrays (-1: none), kx[rank] = f;  CSR offsets of the edges by ii and by jj;  status
__global__ void __launch_bounds__(1024) scan_kernel(int nv, int K, int check_k, int* __restrict__ flag, int* __restrict__ rank,
                                                    int* __restrict__ kx, int* __restrict__ cnt_ii, int* __restrict__ ptr_ii,
                                                    int* __restrict__ cnt_jj, int* __restrict__ ptr_jj, int* __restrict__ status) {
  __shared__ int lds[1024];
  const int nk = scan_1024(nv, flag, rank, lds);
  __syncthreads();
  for (int f = threadIdx.x; f < nv; f += 1024) {
    const int r = rank[f];
    if (flag[f]) {
      if (r < K) kx[r] = f;
    } else {
      rank[f] = -1;
    }
  }
  __syncthreads();
  scan_1024(nv, cnt_ii, ptr_ii, lds);
  __syncthreads();
  scan_1024(nv, cnt_jj, ptr_jj, lds);
  if (threadIdx.x == 0) status[0] = (check_k && nk != K) ? kStatusBadK : 0;
}

// the edges of every frame, in edge order: by ii (idx_ii) and by jj (idx_jj)
__global__ void __launch_bounds__(kThreads) fill_kernel(int nv, int E, const int64_t* __restrict__ ii, const int64_t* __restrict__ jj,
                                                        const int* __restrict__ ptr_ii, int* __restrict__ idx_ii,
                                                        const int* __restrict__ ptr_jj, int* __restrict__ idx_jj) {
  const int f = blockIdx.x * kThreads + threadIdx.x;
  if (f >= nv) return;
  int ci = ptr_ii[f], cj = ptr_jj[f];
  for (int e = 0; e < E; ++e) {
    const int64_t a = ii[e], b = jj[e];
    if (!(frame_ok(a, nv) && frame_ok(b, nv))) continue;
    if (a == f) idx_ii[ci++] = e;
    if (b == f) idx_jj[cj++] = e;
  }
}

// Slots of the Schur complement.  A slot is one (depth row k, window pose a) pair with a nonzero 6 x P block F_{k,a} = the sum of
// the depth Jacobian rows of every term that couples the two.  slot[k][a]:
//   a            frame kx[k] is pose t0 + a: its own Jii rows (summed over its edges) plus those of edges kx[k] -> kx[k];
//   T + e        the first edge e (edge order) from kx[k] to t0 + a: the Jij rows of every such edge, summed into Eij[e];
//   -1           no term.
__global__ void __launch_bounds__(kThreads) slot_kernel(int K, int T, int t0, const int64_t* __restrict__ jj, const int* __restrict__ kx,
                                                        const int* __restrict__ ptr_ii, const int* __restrict__ idx_ii,
                                                        const int* __restrict__ status, int* __restrict__ slot) {
  const long long id = (long long)blockIdx.x * kThreads + threadIdx.x;
  if (id >= (long long)K * T || status[0]) return;
  const int k = (int)(id / T), a = (int)(id % T), f = kx[k], p = t0 + a;
  int s = -1;
  if (f == p) {
    s = a;
  } else {
    for (int i = ptr_ii[f]; i < ptr_ii[f + 1]; ++i) {
      const int e = idx_ii[i];
      if (jj[e] == p) {
        s = T + e;
        break;
      }
    }
  }
  slot[id] = s;
}

// per depth row: the slots in pose order, compacted
__global__ void __launch_bounds__(kThreads) klist_kernel(int K, int T, const int* __restrict__ slot, const int* __restrict__ status,
                                                         int* __restrict__ kcnt, int* __restrict__ kpose, int* __restrict__ kslot) {
  const int k = blockIdx.x * kThreads + threadIdx.x;
  if (k >= K || status[0]) return;
  int c = 0;
  for (int a = 0; a < T; ++a) {
    const int s = slot[(size_t)k * T + a];
    if (s >= 0) {
      kpose[(size_t)k * T + c] = a;
      kslot[(size_t)k * T + c] = s;
      ++c;
    }
  }
  kcnt[k] = c;
}

// ================================================================================================================================
// ba: one Gauss-Newton iteration
// ================================================================================================================================

// Linearisation of edge e over the P pixels of frame ii[e]: per pixel Eii, Eij (6 rows each, [E][6][P]), Cii and bz ([E][P]); per
// edge the 6x6 blocks and 6-vectors of the pose system (fp32, reduced in a fixed order).
__global__ void __launch_bounds__(kThreads) linearize_kernel(int nv, int P, int wd, const float* __restrict__ targets,
                                                             const float* __restrict__ weights, const float* __restrict__ poses,
                                                             const float* __restrict__ disps, const float* __restrict__ intr,
                                                             const int64_t* __restrict__ ii, const int64_t* __restrict__ jj,
                                                             const int* __restrict__ status, float* __restrict__ Hs,
                                                             float* __restrict__ Eii, float* __restrict__ Eij, float* __restrict__ Cii,
                                                             float* __restrict__ bz) {
  __shared__ float red[kWaves * 90];
  if (status[0]) return;
  const int e = blockIdx.x;
  const int64_t ix = ii[e], jx = jj[e];
  const bool ok = frame_ok(ix, nv) && frame_ok(jx, nv);
  const Intr K = load_intr(intr);
  float tij[3] = {kStereoBaseline, 0.f, 0.f}, qij[4] = {0.f, 0.f, 0.f, 1.f};
  if (ok && ix != jx) rel_se3(poses + 7 * ix, poses + 7 * jx, tij, qij);
  const bool stereo = ix == jx;
  float acc[90];    // 78 = lower triangle of the 12x12 [Ji; Jj] normal matrix, then vi (6), vj (6)
#pragma unroll
  for (int l = 0; l < 90; ++l) acc[l] = 0.f;
  const size_t eo = (size_t)e * P;
  const float* dsp = disps + (ok ? ix : 0) * (size_t)P;
  for (int k = threadIdx.x; k < P; k += kThreads) {
    float ei[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, ej[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, c = 0.f, b = 0.f;
    if (ok) {
      const int i = k / wd, j = k - (k / wd) * wd;
      const float Xi[4] = {((float)j - K.cx) / K.fx, ((float)i - K.cy) / K.fy, 1.f, dsp[k]};
      float Xj[4];
      act_se3(tij, qij, Xi, Xj);
      const float x = Xj[0], y = Xj[1], h = Xj[3];
      const bool front = !(Xj[2] < kMinDepth);
      const float d = front ? 1.f / Xj[2] : 0.f, d2 = d * d;
      const float* tg = targets + 2 * eo;
      const float* wt = weights + 2 * eo;
      float w2[2] = {front ? 0.001f * wt[k] : 0.f, front ? 0.001f * wt[P + k] : 0.f};
      const float r2[2] = {tg[k] - (K.fx * d * x + K.cx), tg[P + k] - (K.fy * d * y + K.cy)};
#pragma unroll
      for (int c2 = 0; c2 < 2; ++c2) {
        float Jx[12];
        float* Ji = Jx;
        float* Jj = Jx + 6;
        float Jz;
        if (c2 == 0) {
          Jj[0] = K.fx * (h * d);
          Jj[1] = 0.f;
          Jj[2] = K.fx * (-x * h * d2);
          Jj[3] = K.fx * (-x * y * d2);
          Jj[4] = K.fx * (1.f + x * x * d2);
          Jj[5] = K.fx * (-y * d);
          Jz = K.fx * (tij[0] * d - tij[2] * (x * d2));
        } else {
          Jj[0] = 0.f;
          Jj[1] = K.fy * (h * d);
          Jj[2] = K.fy * (-y * h * d2);
          Jj[3] = K.fy * (-1.f - y * y * d2);
          Jj[4] = K.fy * (x * y * d2);
          Jj[5] = K.fy * (x * d);
          Jz = K.fy * (tij[1] * d - tij[2] * (y * d2));
        }
        float w = w2[c2];
        const float r = r2[c2];
        c += w * Jz * Jz;          // the disparity terms keep stereo edges ...
        b += w * r * Jz;
        if (stereo) w = 0.f;       // ... the pose terms do not
        adjT_se3(tij, qij, Jj, Ji);
#pragma unroll
        for (int n = 0; n < 6; ++n) Ji[n] = -Ji[n];
        int l = 0;
#pragma unroll
        for (int n = 0; n < 12; ++n) {
#pragma unroll
          for (int m = 0; m <= n; ++m) acc[l++] += w * Jx[n] * Jx[m];
        }
#pragma unroll
        for (int n = 0; n < 6; ++n) {
          acc[78 + n] += w * r * Ji[n];
          acc[84 + n] += w * r * Jj[n];
          ei[n] += w * Jz * Ji[n];
          ej[n] += w * Jz * Jj[n];
        }
      }
    }
#pragma unroll
    for (int n = 0; n < 6; ++n) {
      Eii[(eo * 6) + (size_t)n * P + k] = ei[n];
      Eij[(eo * 6) + (size_t)n * P + k] = ej[n];
    }
    Cii[eo + k] = c;
    bz[eo + k] = b;
  }
  block_sum<90>(acc, red);
  float* H = Hs + (size_t)e * kHs;
  const int t = threadIdx.x;
  if (t < 78) {
    int n = 0;
    while ((n + 1) * (n + 2) / 2 <= t) ++n;
    const int m = t - n * (n + 1) / 2;
    const float s = red[t];
    if (n < 6) {                       // Hii (both triangles)
      H[n * 6 + m] = s;
      H[m * 6 + n] = s;
    } else if (m < 6) {                // Hij[m][n-6], Hji[n-6][m]
      H[36 + m * 6 + (n - 6)] = s;
      H[72 + (n - 6) * 6 + m] = s;
    } else {                           // Hjj
      H[108 + (n - 6) * 6 + (m - 6)] = s;
      H[108 + (m - 6) * 6 + (n - 6)] = s;
    }
  } else if (t < 90) {
    H[144 + (t - 78)] = red[t];        // vi, vj
  }
}

// per depth row k (frame f = kx[k]) and pixel: C = sum of Cii over the edges from f + prior, w = sum of bz - prior residual, Q = 1/C
__global__ void __launch_bounds__(kThreads) depth_rows_kernel(int P, const float* __restrict__ disps, const float* __restrict__ sens,
                                                              const float* __restrict__ eta, const int* __restrict__ kx,
                                                              const int* __restrict__ ptr_ii, const int* __restrict__ idx_ii,
                                                              const float* __restrict__ Cii, const float* __restrict__ bz,
                                                              const int* __restrict__ status, float* __restrict__ Qo,
                                                              float* __restrict__ Wo, float* __restrict__ QWo) {
  const int p = blockIdx.x * kThreads + threadIdx.x, k = blockIdx.y;
  if (p >= P || status[0]) return;
  const int f = kx[k];
  float c = 0.f, w = 0.f;
  for (int i = ptr_ii[f]; i < ptr_ii[f + 1]; ++i) {
    const size_t o = (size_t)idx_ii[i] * P + p;
    c += Cii[o];
    w += bz[o];
  }
  const size_t fo = (size_t)f * P + p, ko = (size_t)k * P + p;
  const float s = sens[fo];
  if (s > 0.f) {
    c += kSensorAlpha;
    w -= kSensorAlpha * (disps[fo] - s);
  } else {
    c += eta[ko];
  }
  const float q = 1.f / c;
  Qo[ko] = q;
  Wo[ko] = w;
  QWo[ko] = q * w;
}

__device__ __forceinline__ const float* slot_rows(int s, int T, int P, const float* Ei, const float* Eij) {
  return s < T ? Ei + (size_t)s * 6 * P : Eij + (size_t)(s - T) * 6 * P;
}

// builds the slot blocks: Ei[a] for the window frames, and in place into Eij[e] for the first edge of each (ii, jj) group
__global__ void __launch_bounds__(kThreads) merge_kernel(int nv, int P, int T, int t0, const int64_t* __restrict__ ii,
                                                         const int64_t* __restrict__ jj, const int* __restrict__ rank,
                                                         const int* __restrict__ ptr_ii, const int* __restrict__ idx_ii,
                                                         const int* __restrict__ slot, const float* __restrict__ Eii,
                                                         float* __restrict__ Eij, float* __restrict__ Ei, const int* __restrict__ status) {
  const int p = blockIdx.x * kThreads + threadIdx.x, s = blockIdx.y;
  if (p >= P || status[0]) return;
  float v[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  if (s < T) {
    const int f = t0 + s;
    for (int i = ptr_ii[f]; i < ptr_ii[f + 1]; ++i) {
      const int e = idx_ii[i];
      const size_t o = (size_t)e * 6 * P + p;
#pragma unroll
      for (int n = 0; n < 6; ++n) v[n] += Eii[o + (size_t)n * P];
      if (jj[e] == f) {
#pragma unroll
        for (int n = 0; n < 6; ++n) v[n] += Eij[o + (size_t)n * P];
      }
    }
#pragma unroll
    for (int n = 0; n < 6; ++n) Ei[((size_t)s * 6 + n) * P + p] = v[n];
    return;
  }
  const int e = s - T;
  const int64_t a = ii[e], b = jj[e];
  if (!(frame_ok(a, nv) && frame_ok(b, nv)) || b < t0 || b >= t0 + T || a == b) return;
  if (slot[(size_t)rank[a] * T + (b - t0)] != s) return;      // not the first edge of its group
  int members = 0;
  for (int i = ptr_ii[a]; i < ptr_ii[a + 1]; ++i) {
    const int e2 = idx_ii[i];
    if (jj[e2] != b) continue;
    const size_t o = (size_t)e2 * 6 * P + p;
#pragma unroll
    for (int n = 0; n < 6; ++n) v[n] += Eij[o + (size_t)n * P];
    ++members;
  }
  if (members > 1) {
#pragma unroll
    for (int n = 0; n < 6; ++n) Eij[((size_t)e * 6 + n) * P + p] = v[n];
  }
}

// Block (a, b), b <= a, of the damped reduced system in fp64: the pose blocks of every edge between t0 + a and t0 + b, minus (when
// the depths are free) sum_k F_{k,a} diag(Q_k) F_{k,b}^T.  The diagonal blocks also write the right-hand side.
__global__ void __launch_bounds__(kThreads) assemble_kernel(int P, int T, int t0, int K, int schur, float lm, float ep,
                                                            const int64_t* __restrict__ ii, const int64_t* __restrict__ jj,
                                                            const int* __restrict__ ptr_ii, const int* __restrict__ idx_ii,
                                                            const int* __restrict__ ptr_jj, const int* __restrict__ idx_jj,
                                                            const float* __restrict__ Hs, const int* __restrict__ slot,
                                                            const float* __restrict__ Ei, const float* __restrict__ Eij,
                                                            const float* __restrict__ Q, const float* __restrict__ QW,
                                                            const int* __restrict__ status, double* __restrict__ H,
                                                            double* __restrict__ g, int* __restrict__ fail) {
  __shared__ float red[kWaves * 42];
  const int a = blockIdx.y, b = blockIdx.x;
  if (b > a || status[0]) return;
  if (a == 0 && threadIdx.x == 0) fail[0] = 0;
  const bool diag = a == b;
  float acc[42];
#pragma unroll
  for (int l = 0; l < 42; ++l) acc[l] = 0.f;
  if (schur) {
    for (int k = 0; k < K; ++k) {
      const int sa = slot[(size_t)k * T + a], sb = slot[(size_t)k * T + b];
      if (sa < 0 || sb < 0) continue;
      const float* Fa = slot_rows(sa, T, P, Ei, Eij);
      const float* Fb = slot_rows(sb, T, P, Ei, Eij);
      const float* q = Q + (size_t)k * P;
      const float* qw = QW + (size_t)k * P;
      for (int p = threadIdx.x; p < P; p += kThreads) {
        float fa[6], fb[6];
        const float qp = q[p];
#pragma unroll
        for (int n = 0; n < 6; ++n) {
          fa[n] = Fa[(size_t)n * P + p];
          fb[n] = Fb[(size_t)n * P + p];
        }
#pragma unroll
        for (int n = 0; n < 6; ++n) {
          const float an = fa[n] * qp;
#pragma unroll
          for (int m = 0; m < 6; ++m) acc[n * 6 + m] += an * fb[m];
        }
        if (diag) {
          const float r = qw[p];
#pragma unroll
          for (int n = 0; n < 6; ++n) acc[36 + n] += fa[n] * r;
        }
      }
    }
  }
  block_sum<42>(acc, red);
  const int t = threadIdx.x;
  const int n6 = 6 * T;
  const int pa = t0 + a, pb = t0 + b;
  if (t < 36) {
    const int n = t / 6, m = t % 6;
    double s = 0.0;
    for (int i = ptr_ii[pa]; i < ptr_ii[pa + 1]; ++i) {          // edges leaving pose a: Hii, Hij
      const int e = idx_ii[i];
      const float* h = Hs + (size_t)e * kHs;
      if (diag) s += (double)h[n * 6 + m];
      if (jj[e] == pb) s += (double)h[36 + n * 6 + m];
    }
    for (int i = ptr_jj[pa]; i < ptr_jj[pa + 1]; ++i) {          // edges entering pose a: Hji, Hjj
      const int e = idx_jj[i];
      const float* h = Hs + (size_t)e * kHs;
      if (ii[e] == pb) s += (double)h[72 + n * 6 + m];
      if (diag) s += (double)h[108 + n * 6 + m];
    }
    s -= (double)red[t];
    if (diag && n == m) s += (double)ep + (double)lm * s;
    H[(size_t)(6 * a + n) * n6 + 6 * b + m] = s;
  } else if (diag && t < 42) {
    const int n = t - 36;
    double s = 0.0;
    for (int i = ptr_ii[pa]; i < ptr_ii[pa + 1]; ++i) s += (double)Hs[(size_t)idx_ii[i] * kHs + 144 + n];
    for (int i = ptr_jj[pa]; i < ptr_jj[pa + 1]; ++i) s += (double)Hs[(size_t)idx_jj[i] * kHs + 150 + n];
    g[6 * a + n] = s - (double)red[t];
  }
}

// ---- fp64 Cholesky of the lower triangle, blocked by kNb: potrf of the diagonal block, trsm of the panel below, update of the
// trailing lower triangle.  A pivot that is not > 0 sets fail[0]; from then on every step returns and the solve writes dx = 0.
__global__ void __launch_bounds__(kThreads) potrf_kernel(int n, int kb, double* __restrict__ H, int* __restrict__ fail) {
  __shared__ double L[kNb][kNb + 1];
  __shared__ int bad;
  if (fail[0]) return;
  const int k0 = kb * kNb, bs = min(kNb, n - k0);
  for (int id = threadIdx.x; id < bs * bs; id += kThreads) {
    const int r = id / bs, c = id % bs;
    L[r][c] = c <= r ? H[(size_t)(k0 + r) * n + k0 + c] : 0.0;
  }
  if (threadIdx.x == 0) bad = 0;
  __syncthreads();
  for (int j = 0; j < bs; ++j) {
    if (threadIdx.x == 0) {
      const double d = L[j][j];
      if (!(d > 0.0)) bad = 1;
      L[j][j] = d > 0.0 ? sqrt(d) : 1.0;
    }
    __syncthreads();
    const double ljj = L[j][j];
    for (int i = j + 1 + threadIdx.x; i < bs; i += kThreads) L[i][j] /= ljj;
    __syncthreads();
    const int m = bs - j - 1;
    for (int id = threadIdx.x; id < m * m; id += kThreads) {
      const int i = j + 1 + id / m, c = j + 1 + id % m;
      if (c <= i) L[i][c] -= L[i][j] * L[c][j];
    }
    __syncthreads();
  }
  for (int id = threadIdx.x; id < bs * bs; id += kThreads) {
    const int r = id / bs, c = id % bs;
    if (c <= r) H[(size_t)(k0 + r) * n + k0 + c] = L[r][c];
  }
  if (threadIdx.x == 0 && bad) fail[0] = 1;
}

// rows of block row kb + 1 + blockIdx.x: X = A * L_kk^-T, one thread per row
__global__ void __launch_bounds__(kNb) trsm_kernel(int n, int kb, double* __restrict__ H, const int* __restrict__ fail) {
  __shared__ double L[kNb][kNb + 1];
  if (fail[0]) return;
  const int k0 = kb * kNb, bs = min(kNb, n - k0);
  for (int id = threadIdx.x; id < bs * bs; id += kNb) {
    const int r = id / bs, c = id % bs;
    L[r][c] = c <= r ? H[(size_t)(k0 + r) * n + k0 + c] : 0.0;
  }
  __syncthreads();
  const int r = (kb + 1 + blockIdx.x) * kNb + threadIdx.x;
  if (r >= n) return;
  double* row = H + (size_t)r * n + k0;
  for (int c = 0; c < bs; ++c) {
    double s = row[c];
    for (int j = 0; j < c; ++j) s -= row[j] * L[c][j];
    row[c] = s / L[c][c];
  }
}

// A[ib][jb] -= L[ib][kb] L[jb][kb]^T for the lower tiles jb <= ib of the trailing matrix; 64x64 tile, 4x4 per thread
__global__ void __launch_bounds__(kThreads) syrk_kernel(int n, int kb, double* __restrict__ H, const int* __restrict__ fail) {
  constexpr int kc = 16;
  __shared__ double As[kNb][kc + 1], Bs[kNb][kc + 1];
  if (fail[0]) return;
  const int ib = kb + 1 + blockIdx.y, jb = kb + 1 + blockIdx.x;
  if (jb > ib) return;
  const int r0 = ib * kNb, c0 = jb * kNb, k0 = kb * kNb, kw = min(kNb, n - k0);
  const int tx = threadIdx.x % 16, ty = threadIdx.x / 16;
  double acc[4][4] = {};
  for (int kk = 0; kk < kw; kk += kc) {
    for (int id = threadIdx.x; id < kNb * kc; id += kThreads) {
      const int r = id / kc, c = id % kc, col = k0 + kk + c;
      const bool cok = kk + c < kw;
      As[r][c] = (cok && r0 + r < n) ? H[(size_t)(r0 + r) * n + col] : 0.0;
      Bs[r][c] = (cok && c0 + r < n) ? H[(size_t)(c0 + r) * n + col] : 0.0;
    }
    __syncthreads();
#pragma unroll
    for (int c = 0; c < kc; ++c) {
#pragma unroll
      for (int u = 0; u < 4; ++u) {
#pragma unroll
        for (int v = 0; v < 4; ++v) acc[u][v] += As[ty * 4 + u][c] * Bs[tx * 4 + v][c];
      }
    }
    __syncthreads();
  }
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int r = r0 + ty * 4 + u;
#pragma unroll
    for (int v = 0; v < 4; ++v) {
      const int c = c0 + tx * 4 + v;
      if (r < n && c < n && c <= r) H[(size_t)r * n + c] -= acc[u][v];
    }
  }
}

// L L^T x = g by blocked forward and backward substitution in one workgroup; dx = x (fp32), 0 after a failed factorisation, NaN
// when the call was refused on the device (status)
__global__ void __launch_bounds__(1024) solve_kernel(int n, const double* __restrict__ H, const double* __restrict__ g,
                                                     const int* __restrict__ fail, const int* __restrict__ status,
                                                     float* __restrict__ dx) {
  __shared__ double y[kMaxWindow * 6];
  const int t = threadIdx.x;
  if (status[0] || fail[0]) {
    for (int i = t; i < n; i += 1024) dx[i] = status[0] ? NAN : 0.f;
    return;
  }
  for (int i = t; i < n; i += 1024) y[i] = g[i];
  __syncthreads();
  const int nbk = (n + kNb - 1) / kNb;
  for (int kb = 0; kb < nbk; ++kb) {                 // L y = g
    const int k0 = kb * kNb, k1 = min(n, k0 + kNb);
    if (t == 0) {
      for (int c = k0; c < k1; ++c) {
        double s = y[c];
        for (int j = k0; j < c; ++j) s -= H[(size_t)c * n + j] * y[j];
        y[c] = s / H[(size_t)c * n + c];
      }
    }
    __syncthreads();
    for (int r = k1 + t; r < n; r += 1024) {
      double s = 0.0;
      for (int j = k0; j < k1; ++j) s += H[(size_t)r * n + j] * y[j];
      y[r] -= s;
    }
    __syncthreads();
  }
  for (int kb = nbk - 1; kb >= 0; --kb) {            // L^T x = y
    const int k0 = kb * kNb, k1 = min(n, k0 + kNb);
    if (t == 0) {
      for (int c = k1 - 1; c >= k0; --c) {
        double s = y[c];
        for (int j = c + 1; j < k1; ++j) s -= H[(size_t)j * n + c] * y[j];
        y[c] = s / H[(size_t)c * n + c];
      }
    }
    __syncthreads();
    for (int r = t; r < k0; r += 1024) {
      double s = 0.0;
      for (int j = k0; j < k1; ++j) s += H[(size_t)j * n + r] * y[j];
      y[r] -= s;
    }
    __syncthreads();
  }
  for (int i = t; i < n; i += 1024) dx[i] = (float)y[i];
}

// poses[t0 + a] = exp(dx[a]) * poses[t0 + a]
__global__ void __launch_bounds__(kThreads) pose_retr_kernel(int T, int t0, float* __restrict__ poses, const float* __restrict__ dx,
                                                             const int* __restrict__ status) {
  if (status[0]) return;
  for (int a = threadIdx.x; a < T; a += kThreads) {
    float* P = poses + 7 * (size_t)(t0 + a);
    const float t[3] = {P[0], P[1], P[2]}, q[4] = {P[3], P[4], P[5], P[6]};
    float dt[3], dq[4];
    exp_se3(dx + 6 * a, dt, dq);
    const float q1[4] = {dq[3] * q[0] + dq[0] * q[3] + dq[1] * q[2] - dq[2] * q[1],
                         dq[3] * q[1] + dq[1] * q[3] + dq[2] * q[0] - dq[0] * q[2],
                         dq[3] * q[2] + dq[2] * q[3] + dq[0] * q[1] - dq[1] * q[0],
                         dq[3] * q[3] - dq[0] * q[0] - dq[1] * q[1] - dq[2] * q[2]};
    float t1[3];
    act_so3(dq, t, t1);
    P[0] = t1[0] + dt[0];
    P[1] = t1[1] + dt[1];
    P[2] = t1[2] + dt[2];
    P[3] = q1[0];
    P[4] = q1[1];
    P[5] = q1[2];
    P[6] = q1[3];
  }
}

// dz = Q (w - sum_a F_{k,a} dx[a]) over the slots of row k whose pose is not t0 (as the reference's back-substitution, which
// skips the first window pose); disps[kx[k]] += dz
__global__ void __launch_bounds__(kThreads) dz_kernel(int P, int T, const int* __restrict__ kx, const int* __restrict__ kcnt,
                                                      const int* __restrict__ kpose, const int* __restrict__ kslot,
                                                      const float* __restrict__ Ei, const float* __restrict__ Eij,
                                                      const float* __restrict__ Q, const float* __restrict__ W,
                                                      const float* __restrict__ dx, const int* __restrict__ status,
                                                      float* __restrict__ dz, float* __restrict__ disps) {
  const int p = blockIdx.x * kThreads + threadIdx.x, k = blockIdx.y;
  if (p >= P) return;
  const size_t ko = (size_t)k * P + p;
  if (status[0]) {
    dz[ko] = NAN;
    return;
  }
  float s = 0.f;
  for (int c = 0; c < kcnt[k]; ++c) {
    const int a = kpose[(size_t)k * T + c];
    if (a < 1) continue;
    const float* F = slot_rows(kslot[(size_t)k * T + c], T, P, Ei, Eij);
    float dw = 0.f;
#pragma unroll
    for (int n = 0; n < 6; ++n) dw += F[(size_t)n * P + p] * dx[6 * a + n];
    s += dw;
  }
  // the step is rounded once, and that rounded step is what moves the disparity: contracted into an FMA the map would move by the
  // unrounded product and disps_after != disps_before + dz in the last bit
  {
#pragma clang fp contract(off)
    const float d = Q[ko] * (W[ko] - s);
    dz[ko] = d;
    disps[(size_t)kx[k] * P + p] += d;
  }
}

// ================================================================================================================================
// frame geometry
// ================================================================================================================================

__global__ void __launch_bounds__(kThreads) frame_distance_kernel(int nv, int P, int wd, const float* __restrict__ poses,
                                                                  const float* __restrict__ disps, const float* __restrict__ intr,
                                                                  const int64_t* __restrict__ ii, const int64_t* __restrict__ jj,
                                                                  float beta, float* __restrict__ dist) {
  __shared__ float red[kWaves * 3];
  const int e = blockIdx.x;
  const int64_t ix = ii[e], jx = jj[e];
  if (!(frame_ok(ix, nv) && frame_ok(jx, nv))) {
    if (threadIdx.x == 0) dist[e] = NAN;
    return;
  }
  const Intr K = load_intr(intr);
  float tij[3], qij[4];
  rel_se3(poses + 7 * ix, poses + 7 * jx, tij, qij);
  const float* dsp = disps + ix * (size_t)P;
  float v[3] = {0.f, 0.f, 0.f};    // accum, valid, total
  for (int k = threadIdx.x; k < P; k += kThreads) {
    const int i = k / wd, j = k - (k / wd) * wd;
    const float u = (float)j, vv = (float)i;
    const float Xi[4] = {(u - K.cx) / K.fx, (vv - K.cy) / K.fy, 1.f, dsp[k]};
    float Xj[4];
    act_se3(tij, qij, Xi, Xj);                       // full motion, weight beta
    float du = K.fx * (Xj[0] / Xj[2]) + K.cx - u, dv = K.fy * (Xj[1] / Xj[2]) + K.cy - vv;
    float d = sqrtf(du * du + dv * dv);
    v[2] += beta;
    if (Xj[2] > kMinDepth) {
      v[0] += beta * d;
      v[1] += beta;
    }
    const float X2[3] = {Xi[0] + Xi[3] * tij[0], Xi[1] + Xi[3] * tij[1], Xi[2] + Xi[3] * tij[2]};   // translation only, 1 - beta
    du = K.fx * (X2[0] / X2[2]) + K.cx - u;
    dv = K.fy * (X2[1] / X2[2]) + K.cy - vv;
    d = sqrtf(du * du + dv * dv);
    v[2] += 1.f - beta;
    if (X2[2] > kMinDepth) {
      v[0] += (1.f - beta) * d;
      v[1] += 1.f - beta;
    }
  }
  block_sum<3>(v, red);
  if (threadIdx.x == 0) dist[e] = ((double)red[1] / ((double)red[2] + 1e-8) < 0.75) ? 1000.f : red[0] / red[1];
}

__global__ void __launch_bounds__(kThreads) projmap_kernel(int nv, int P, int wd, const float* __restrict__ poses,
                                                           const float* __restrict__ disps, const float* __restrict__ intr,
                                                           const int64_t* __restrict__ ii, const int64_t* __restrict__ jj,
                                                           float* __restrict__ coords, float* __restrict__ valid) {
  const int k = blockIdx.x * kThreads + threadIdx.x, e = blockIdx.y;
  if (k >= P) return;
  const size_t o = (size_t)e * P + k;
  const int64_t ix = ii[e], jx = jj[e];
  if (!(frame_ok(ix, nv) && frame_ok(jx, nv))) {
    coords[3 * o] = coords[3 * o + 1] = coords[3 * o + 2] = NAN;
    valid[o] = 0.f;
    return;
  }
  const Intr K = load_intr(intr);
  float tij[3], qij[4];
  rel_se3(poses + 7 * ix, poses + 7 * jx, tij, qij);
  const int i = k / wd, j = k - (k / wd) * wd;
  const float u = (float)j, v = (float)i;
  const float Xi[4] = {(u - K.cx) / K.fx, (v - K.cy) / K.fy, 1.f, disps[ix * (size_t)P + k]};
  float Xj[4];
  act_se3(tij, qij, Xi, Xj);
  const bool in_front = (double)Xj[2] > 0.01;
  coords[3 * o] = in_front ? K.fx * (Xj[0] / Xj[2]) + K.cx : u;
  coords[3 * o + 1] = in_front ? K.fy * (Xj[1] / Xj[2]) + K.cy : v;
  coords[3 * o + 2] = 0.f;
  valid[o] = Xj[2] > kMinDepth ? 1.f : 0.f;
}

__global__ void __launch_bounds__(kThreads) iproj_kernel(int P, int wd, const float* __restrict__ poses, const float* __restrict__ disps,
                                                         const float* __restrict__ intr, float* __restrict__ points) {
  const int k = blockIdx.x * kThreads + threadIdx.x, f = blockIdx.y;
  if (k >= P) return;
  const Intr K = load_intr(intr);
  const float* pose = poses + 7 * (size_t)f;
  const int i = k / wd, j = k - (k / wd) * wd;
  const float Xi[4] = {((float)j - K.cx) / K.fx, ((float)i - K.cy) / K.fy, 1.f, disps[(size_t)f * P + k]};
  float Xj[4];
  act_se3(pose, pose + 3, Xi, Xj);
  const size_t o = 3 * ((size_t)f * P + k);
  points[o] = Xj[0] / Xj[3];
  points[o + 1] = Xj[1] / Xj[3];
  points[o + 2] = Xj[2] / Xj[3];
}

// neighbours of frame ix: ix-1, ix-2, ix-3, ix+3, ix+4, ix+5 (the reference's choice); a pixel counts a neighbour when one of the
// four disparities around its reprojection gives a depth within thresh of its own (compared in fp64, as the reference does)
__global__ void __launch_bounds__(kThreads) depth_filter_kernel(int nf, int ht, int wd, const float* __restrict__ poses,
                                                                const float* __restrict__ disps, const float* __restrict__ intr,
                                                                const int64_t* __restrict__ inds, const float* __restrict__ thresh,
                                                                float* __restrict__ counter) {
  const int P = ht * wd;
  const int k = blockIdx.x * kThreads + threadIdx.x, b = blockIdx.y;
  if (k >= P) return;
  const int64_t ix = inds[b];
  float count = 0.f;
  if (frame_ok(ix, nf)) {
    const Intr K = load_intr(intr);
    const float t = thresh[b];
    const int i = k / wd, j = k - (k / wd) * wd;
    const float Xi[4] = {((float)j - K.cx) / K.fx, ((float)i - K.cy) / K.fy, 1.f, disps[ix * (size_t)P + k]};
    for (int nb = 0; nb < 6; ++nb) {
      const int64_t jx = nb < 3 ? ix - nb - 1 : ix + nb;
      if (jx < 0 || jx >= nf) continue;
      float tij[3], qij[4], Xj[4];
      rel_se3(poses + 7 * ix, poses + 7 * jx, tij, qij);
      act_se3(tij, qij, Xi, Xj);
      const float uj = K.fx * (Xj[0] / Xj[2]) + K.cx, vj = K.fy * (Xj[1] / Xj[2]) + K.cy, dj = Xj[3] / Xj[2];
      const float fu = floorf(uj), fv = floorf(vj);
      if (!(fu >= 0.f && fv >= 0.f && fu < (float)(wd - 1) && fv < (float)(ht - 1))) continue;
      const int u0 = (int)fu, v0 = (int)fv;
      const float* dn = disps + jx * (size_t)P;
      const double rj = 1.0 / (double)dj;
      const float d00 = dn[v0 * wd + u0], d01 = dn[v0 * wd + u0 + 1], d10 = dn[(v0 + 1) * wd + u0], d11 = dn[(v0 + 1) * wd + u0 + 1];
      if (fabs(rj - 1.0 / (double)d00) < t || fabs(rj - 1.0 / (double)d01) < t || fabs(rj - 1.0 / (double)d10) < t ||
          fabs(rj - 1.0 / (double)d11) < t)
        count += 1.f;
    }
  }
  counter[(size_t)b * P + k] = count;
}

// ---- scratch layout of ba
struct DbaScratch {
  float *Hs, *Eii, *Eij, *Cii, *bz, *Ei, *Q, *W, *QW;
  int *flag, *rank, *kx, *cnt_ii, *ptr_ii, *idx_ii, *cnt_jj, *ptr_jj, *idx_jj, *slot, *kcnt, *kpose, *kslot, *status, *fail;
  double *H, *g;
};

size_t carve(int nv, int E, int K, int T, int P, char* base, DbaScratch* s) {
  size_t off = 0;
  auto take = [&](size_t bytes) {
    char* p = base ? base + off : nullptr;
    off += align_up(bytes);
    return p;
  };
  const size_t f4 = sizeof(float), i4 = sizeof(int), n6 = 6 * (size_t)T;
  DbaScratch d;
  d.Hs = (float*)take((size_t)E * kHs * f4);
  d.Eii = (float*)take((size_t)E * 6 * P * f4);
  d.Eij = (float*)take((size_t)E * 6 * P * f4);
  d.Cii = (float*)take((size_t)E * P * f4);
  d.bz = (float*)take((size_t)E * P * f4);
  d.Ei = (float*)take(n6 * P * f4);
  d.Q = (float*)take((size_t)K * P * f4);
  d.W = (float*)take((size_t)K * P * f4);
  d.QW = (float*)take((size_t)K * P * f4);
  d.flag = (int*)take((size_t)nv * i4);
  d.rank = (int*)take((size_t)(nv + 1) * i4);
  d.kx = (int*)take((size_t)K * i4);
  d.cnt_ii = (int*)take((size_t)nv * i4);
  d.ptr_ii = (int*)take((size_t)(nv + 1) * i4);
  d.idx_ii = (int*)take((size_t)E * i4);
  d.cnt_jj = (int*)take((size_t)nv * i4);
  d.ptr_jj = (int*)take((size_t)(nv + 1) * i4);
  d.idx_jj = (int*)take((size_t)E * i4);
  d.slot = (int*)take((size_t)K * T * i4);
  d.kcnt = (int*)take((size_t)K * i4);
  d.kpose = (int*)take((size_t)K * T * i4);
  d.kslot = (int*)take((size_t)K * T * i4);
  d.status = (int*)take(i4);
  d.fail = (int*)take(i4);
  d.H = (double*)take(n6 * n6 * sizeof(double));
  d.g = (double*)take(n6 * sizeof(double));
  if (s) *s = d;
  return off;
}

bool sizes_ok(int nv, int E, int K, int T, int ht, int wd) {
  return nv > 0 && E > 0 && E <= kMaxEdges && K > 0 && K <= 65535 && T > 0 && T <= kMaxWindow && ht > 0 && wd > 0 &&
         (long long)ht * wd < (1LL << 26) &&
         (long long)E * 6 * ht * wd < (1LL << 40);
}

}  // namespace
}  // namespace sgr

using namespace sgr;

extern "C" {

size_t sgr_dba_scratch_bytes(int32_t num_frames, int32_t num_edges, int32_t num_depth, int32_t window, int32_t ht, int32_t wd) {
  if (!sizes_ok(num_frames, num_edges, num_depth, window, ht, wd)) return 0;
  return carve(num_frames, num_edges, num_depth, window, ht * wd, nullptr, nullptr);
}

int sgr_dba_ba(const SgrDbaProblem* pr, void* scratch, size_t scratch_bytes, void* stream) {
  if (!pr || !pr->poses || !pr->disps || !pr->intrinsics || !pr->disps_sens || !pr->targets || !pr->weights || !pr->eta || !pr->ii ||
      !pr->jj || !pr->dx)
    return set_error(SGR_ERR_INVALID, "dba_ba: null argument");
  const int nv = std::min(pr->num_poses, pr->num_frames), E = pr->num_edges, K = pr->num_depth, t0 = pr->t0, t1 = pr->t1;
  const int T = t1 - t0, ht = pr->ht, wd = pr->wd, P = ht * wd;
  if (t0 < 0 || t1 > nv || T < 1)
    return set_error(SGR_ERR_INVALID, "dba_ba: window [%d, %d) must be non-empty and inside the %d frames", t0, t1, nv);
  if (T > kMaxWindow) return set_error(SGR_ERR_CAPACITY, "dba_ba: window of %d frames exceeds the supported %d", T, kMaxWindow);
  if (!sizes_ok(nv, E, K, T, ht, wd) || pr->iterations < 0)
    return set_error(SGR_ERR_INVALID, "dba_ba: bad sizes (frames=%d edges=%d K=%d ht=%d wd=%d iterations=%d)", nv, E, K, ht, wd,
                     pr->iterations);
  const bool motion_only = pr->motion_only != 0, depth_only = pr->depth_only != 0;
  if (!motion_only && !pr->dz) return set_error(SGR_ERR_INVALID, "dba_ba: dz is required unless motion_only");
  if (!scratch || scratch_bytes < carve(nv, E, K, T, P, nullptr, nullptr)) return set_error(SGR_ERR_WORKSPACE, "dba_ba: scratch too small");
  DbaScratch s;
  carve(nv, E, K, T, P, (char*)scratch, &s);
  hipStream_t st = (hipStream_t)stream;
  const int n = 6 * T, nbk = (n + kNb - 1) / kNb;

  hipLaunchKernelGGL(mark_kernel, dim3(blocks_for(nv)), dim3(kThreads), 0, st, nv, E, pr->ii, pr->jj, t0, t1, s.flag, s.cnt_ii, s.cnt_jj);
  hipLaunchKernelGGL(scan_kernel, dim3(1), dim3(1024), 0, st, nv, K, motion_only ? 0 : 1, s.flag, s.rank, s.kx, s.cnt_ii, s.ptr_ii,
                     s.cnt_jj, s.ptr_jj, s.status);
  hipLaunchKernelGGL(fill_kernel, dim3(blocks_for(nv)), dim3(kThreads), 0, st, nv, E, pr->ii, pr->jj, s.ptr_ii, s.idx_ii, s.ptr_jj, s.idx_jj);
  if (!motion_only) {
    hipLaunchKernelGGL(slot_kernel, dim3(blocks_for((long long)K * T)), dim3(kThreads), 0, st, K, T, t0, pr->jj, s.kx, s.ptr_ii, s.idx_ii,
                       s.status, s.slot);
    hipLaunchKernelGGL(klist_kernel, dim3(blocks_for(K)), dim3(kThreads), 0, st, K, T, s.slot, s.status, s.kcnt, s.kpose, s.kslot);
  }
  const dim3 pix(blocks_for(P));
  for (int it = 0; it < pr->iterations; ++it) {
    hipLaunchKernelGGL(linearize_kernel, dim3(E), dim3(kThreads), 0, st, nv, P, wd, pr->targets, pr->weights, pr->poses, pr->disps,
                       pr->intrinsics, pr->ii, pr->jj, s.status, s.Hs, s.Eii, s.Eij, s.Cii, s.bz);
    if (!motion_only) {
      hipLaunchKernelGGL(depth_rows_kernel, dim3(pix.x, K), dim3(kThreads), 0, st, P, pr->disps, pr->disps_sens, pr->eta, s.kx, s.ptr_ii,
                         s.idx_ii, s.Cii, s.bz, s.status, s.Q, s.W, s.QW);
      hipLaunchKernelGGL(merge_kernel, dim3(pix.x, T + E), dim3(kThreads), 0, st, nv, P, T, t0, pr->ii, pr->jj, s.rank, s.ptr_ii,
                         s.idx_ii, s.slot, s.Eii, s.Eij, s.Ei, s.status);
    }
    hipLaunchKernelGGL(assemble_kernel, dim3(T, T), dim3(kThreads), 0, st, P, T, t0, K, motion_only ? 0 : 1, pr->lm, pr->ep, pr->ii,
                       pr->jj, s.ptr_ii, s.idx_ii, s.ptr_jj, s.idx_jj, s.Hs, s.slot, s.Ei, s.Eij, s.Q, s.QW, s.status, s.H, s.g,
                       s.fail);
    for (int kb = 0; kb < nbk; ++kb) {
      hipLaunchKernelGGL(potrf_kernel, dim3(1), dim3(kThreads), 0, st, n, kb, s.H, s.fail);
      const int rest = nbk - kb - 1;
      if (rest > 0) {
        hipLaunchKernelGGL(trsm_kernel, dim3(rest), dim3(kNb), 0, st, n, kb, s.H, s.fail);
        hipLaunchKernelGGL(syrk_kernel, dim3(rest, rest), dim3(kThreads), 0, st, n, kb, s.H, s.fail);
      }
    }
    hipLaunchKernelGGL(solve_kernel, dim3(1), dim3(1024), 0, st, n, s.H, s.g, s.fail, s.status, pr->dx);
    if (motion_only || !depth_only)
      hipLaunchKernelGGL(pose_retr_kernel, dim3(1), dim3(kThreads), 0, st, T, t0, pr->poses, pr->dx, s.status);
    if (!motion_only)
      hipLaunchKernelGGL(dz_kernel, dim3(pix.x, K), dim3(kThreads), 0, st, P, T, s.kx, s.kcnt, s.kpose, s.kslot, s.Ei, s.Eij, s.Q, s.W,
                         pr->dx, s.status, pr->dz, pr->disps);
  }
  return hipGetLastError() == hipSuccess ? SGR_OK : set_error(SGR_ERR_HIP, "dba_ba launch failed");
}

int sgr_dba_frame_distance(const float* poses, int32_t num_poses, const float* disps, int32_t num_frames, int32_t ht, int32_t wd,
                           const float* intrinsics, const int64_t* ii, const int64_t* jj, int32_t num_edges, float beta, float* dist,
                           void* stream) {
  if (!poses || !disps || !intrinsics || !ii || !jj || !dist || num_edges < 0 || ht <= 0 || wd <= 0)
    return set_error(SGR_ERR_INVALID, "dba_frame_distance: bad arguments");
  if (num_edges == 0) return SGR_OK;
  hipLaunchKernelGGL(frame_distance_kernel, dim3(num_edges), dim3(kThreads), 0, (hipStream_t)stream, std::min(num_poses, num_frames),
                     ht * wd, wd, poses, disps, intrinsics, ii, jj, beta, dist);
  return hipGetLastError() == hipSuccess ? SGR_OK : set_error(SGR_ERR_HIP, "dba_frame_distance launch failed");
}

int sgr_dba_projmap(const float* poses, int32_t num_poses, const float* disps, int32_t num_frames, int32_t ht, int32_t wd,
                    const float* intrinsics, const int64_t* ii, const int64_t* jj, int32_t num_edges, float* coords, float* valid,
                    void* stream) {
  if (!poses || !disps || !intrinsics || !ii || !jj || !coords || !valid || num_edges < 0 || num_edges > 65535 || ht <= 0 || wd <= 0)
    return set_error(SGR_ERR_INVALID, "dba_projmap: bad arguments");
  if (num_edges == 0) return SGR_OK;
  hipLaunchKernelGGL(projmap_kernel, dim3(blocks_for(ht * wd), num_edges), dim3(kThreads), 0, (hipStream_t)stream,
                     std::min(num_poses, num_frames), ht * wd, wd, poses, disps, intrinsics, ii, jj, coords, valid);
  return hipGetLastError() == hipSuccess ? SGR_OK : set_error(SGR_ERR_HIP, "dba_projmap launch failed");
}

int sgr_dba_iproj(const float* poses, const float* disps, int32_t num_frames, int32_t ht, int32_t wd, const float* intrinsics,
                  float* points, void* stream) {
  if (!poses || !disps || !intrinsics || !points || num_frames < 0 || num_frames > 65535 || ht <= 0 || wd <= 0)
    return set_error(SGR_ERR_INVALID, "dba_iproj: bad arguments");
  if (num_frames == 0) return SGR_OK;
  hipLaunchKernelGGL(iproj_kernel, dim3(blocks_for(ht * wd), num_frames), dim3(kThreads), 0, (hipStream_t)stream, ht * wd, wd, poses, disps,
                     intrinsics, points);
  return hipGetLastError() == hipSuccess ? SGR_OK : set_error(SGR_ERR_HIP, "dba_iproj launch failed");
}

int sgr_dba_depth_filter(const float* poses, const float* disps, int32_t num_frames, int32_t ht, int32_t wd, const float* intrinsics,
                         const int64_t* inds, int32_t num, const float* thresh, float* counter, void* stream) {
  if (!poses || !disps || !intrinsics || !inds || !thresh || !counter || num < 0 || num > 65535 || ht <= 0 || wd <= 0)
    return set_error(SGR_ERR_INVALID, "dba_depth_filter: bad arguments");
  if (num == 0) return SGR_OK;
  hipLaunchKernelGGL(depth_filter_kernel, dim3(blocks_for(ht * wd), num), dim3(kThreads), 0, (hipStream_t)stream, num_frames, ht, wd, poses,
                     disps, intrinsics, inds, thresh, counter);
  return hipGetLastError() == hipSuccess ? SGR_OK : set_error(SGR_ERR_HIP, "dba_depth_filter launch failed");
}

}  // extern "C"
