// SE3 on (t, q xyzw) in fp32, as lietorch has it: the device functions behind the se3_* entry points (sgr_aux.hip), shared with the
// kernels that must give the same bits as those entry points (sgr_traj.hip: the camera centre is the translation of SE3(p).inv()).
#pragma once

#include "sgr_common.h"

namespace sgr {

struct Pose { float t[3]; float q[4]; };   // q = (x, y, z, w)
__device__ __forceinline__ Pose load_pose(const float* p) { return {{p[0], p[1], p[2]}, {p[3], p[4], p[5], p[6]}}; }
__device__ __forceinline__ void store_pose(float* p, const Pose& a) {
  p[0] = a.t[0]; p[1] = a.t[1]; p[2] = a.t[2]; p[3] = a.q[0]; p[4] = a.q[1]; p[5] = a.q[2]; p[6] = a.q[3];
}
__device__ __forceinline__ void quat_rotate(const float q[4], const float v[3], float out[3]) {
  // v + 2w (u x v) + 2 u x (u x v),  u = (x,y,z)
  float ux = q[0], uy = q[1], uz = q[2], w = q[3];
  float cx = uy * v[2] - uz * v[1], cy = uz * v[0] - ux * v[2], cz = ux * v[1] - uy * v[0];
  float dx = uy * cz - uz * cy, dy = uz * cx - ux * cz, dz = ux * cy - uy * cx;
  out[0] = v[0] + 2.f * (w * cx + dx);
  out[1] = v[1] + 2.f * (w * cy + dy);
  out[2] = v[2] + 2.f * (w * cz + dz);
}
__device__ __forceinline__ void quat_mul(const float a[4], const float b[4], float o[4]) {
  o[0] = a[3] * b[0] + a[0] * b[3] + a[1] * b[2] - a[2] * b[1];
  o[1] = a[3] * b[1] - a[0] * b[2] + a[1] * b[3] + a[2] * b[0];
  o[2] = a[3] * b[2] + a[0] * b[1] - a[1] * b[0] + a[2] * b[3];
  o[3] = a[3] * b[3] - a[0] * b[0] - a[1] * b[1] - a[2] * b[2];
}
// (q, t)^-1 = (q*, -(q* t)): quat_rotate(q*, t) with every rounding written out, so that each kernel this is inlined into gives
// the same bits.  Left to the compiler, which products of quat_rotate are fused depends on the code around it; the roundings
// below are the ones se3_inv has always had (c = -q x t and d = -q x c as a product and a fused multiply-add each; w c + d fused
// in x and y, w c_z rounded on its own).
__device__ __forceinline__ Pose pose_inv(const Pose& p) {
#pragma clang fp contract(off)
  const float qx = p.q[0], qy = p.q[1], qz = p.q[2], w = p.q[3], t0 = p.t[0], t1 = p.t[1], t2 = p.t[2];
  const float cx = __builtin_fmaf(t1, qz, -(t2 * qy)), cy = __builtin_fmaf(t2, qx, -(t0 * qz)), cz = __builtin_fmaf(t0, qy, -(t1 * qx));
  const float dx = __builtin_fmaf(qz, cy, -(qy * cz)), dy = __builtin_fmaf(qx, cz, -(qz * cx)), dz = __builtin_fmaf(-qx, cy, qy * cx);
  Pose r;
  r.q[0] = -qx; r.q[1] = -qy; r.q[2] = -qz; r.q[3] = w;
  r.t[0] = -__builtin_fmaf(2.f, __builtin_fmaf(w, cx, dx), t0);
  r.t[1] = -__builtin_fmaf(2.f, __builtin_fmaf(w, cy, dy), t1);
  r.t[2] = -__builtin_fmaf(2.f, w * cz + dz, t2);
  return r;
}

}  // namespace sgr
