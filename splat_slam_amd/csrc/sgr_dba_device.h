// Device helpers shared by the tracker's bundle adjustment kernels (sgr_dba.hip, sgr_dspo.hip): SE3 on (t, q xyzw) in fp32 as in the
// reference, pinhole intrinsics, and the one-workgroup scan the edge grouping uses.
#pragma once

#include <cstdint>

#include "sgr_common.h"

namespace sgr {
namespace dba {

constexpr float kStereoBaseline = -0.1f;    // ii == jj edges: fixed relative pose (t = (-0.1, 0, 0), q = identity)

__device__ __forceinline__ void act_so3(const float* q, const float* X, float* Y) {
  const float uv0 = 2.f * (q[1] * X[2] - q[2] * X[1]);
  const float uv1 = 2.f * (q[2] * X[0] - q[0] * X[2]);
  const float uv2 = 2.f * (q[0] * X[1] - q[1] * X[0]);
  Y[0] = X[0] + q[3] * uv0 + (q[1] * uv2 - q[2] * uv1);
  Y[1] = X[1] + q[3] * uv1 + (q[2] * uv0 - q[0] * uv2);
  Y[2] = X[2] + q[3] * uv2 + (q[0] * uv1 - q[1] * uv0);
}

// homogeneous point (x, y, z, h): rotate the xyz part, add h * t
__device__ __forceinline__ void act_se3(const float* t, const float* q, const float* X, float* Y) {
  act_so3(q, X, Y);
  Y[3] = X[3];
  Y[0] += X[3] * t[0];
  Y[1] += X[3] * t[1];
  Y[2] += X[3] * t[2];
}

// Gij = Gj * Gi^-1 (poses map world to camera)
__device__ __forceinline__ void rel_se3(const float* pi, const float* pj, float* tij, float* qij) {
  const float *ti = pi, *qi = pi + 3, *tj = pj, *qj = pj + 3;
  qij[0] = -qj[3] * qi[0] + qj[0] * qi[3] - qj[1] * qi[2] + qj[2] * qi[1];
  qij[1] = -qj[3] * qi[1] + qj[1] * qi[3] - qj[2] * qi[0] + qj[0] * qi[2];
  qij[2] = -qj[3] * qi[2] + qj[2] * qi[3] - qj[0] * qi[1] + qj[1] * qi[0];
  qij[3] = qj[3] * qi[3] + qj[0] * qi[0] + qj[1] * qi[1] + qj[2] * qi[2];
  act_so3(qij, ti, tij);
  tij[0] = tj[0] - tij[0];
  tij[1] = tj[1] - tij[1];
  tij[2] = tj[2] - tij[2];
}

struct Intr {
  float fx, fy, cx, cy;
};
__device__ __forceinline__ Intr load_intr(const float* k) { return {k[0], k[1], k[2], k[3]}; }

__device__ __forceinline__ bool frame_ok(int64_t f, int nv) { return f >= 0 && f < nv; }

// exclusive scan of n ints by one 1024-thread workgroup (out[n] = total; out may be data); returns the total to every thread
__device__ inline int scan_1024(int n, int* __restrict__ data, int* __restrict__ out, int* lds) {
  const int t = threadIdx.x, chunk = (n + 1023) / 1024;
  const int lo = min(n, t * chunk), hi = min(n, lo + chunk);
  int s = 0;
  for (int i = lo; i < hi; ++i) s += data[i];
  lds[t] = s;
  __syncthreads();
  for (int off = 1; off < 1024; off <<= 1) {
    const int v = t >= off ? lds[t - off] : 0;
    __syncthreads();
    lds[t] += v;
    __syncthreads();
  }
  const int total = lds[1023];
  int run = lds[t] - s;
  for (int i = lo; i < hi; ++i) {
    const int d = data[i];
    out[i] = run;
    run += d;
  }
  __syncthreads();
  if (t == 0) out[n] = total;
  return total;
}

}  // namespace dba
}  // namespace sgr
