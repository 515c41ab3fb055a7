// Device code of the optimiser tail of a mapping iteration, shared by the two launches that run it: gather_adam_kernel
// (sgr_aux.hip) and the K1 instantiation whose blocks begin with the previous iteration's step for their own segment
// (preprocess_fwd_kernel<true>, sgr_preprocess.hip).  ONE definition: the two must agree bit for bit.
#pragma once

#include "sgr_common.h"

namespace sgr {

// second stage of the mapping loss: one 256-thread block adds a view's partials in a fixed order (thread-strided, then DPP + LDS)
__device__ __forceinline__ void loss_final_view(const LossPart* __restrict__ parts, int nparts, float inv_rgb, float inv_dep,
                                                float alpha, float* loss, float* da, float* db, LossPart* red /*LDS[4]*/) {
#pragma clang fp contract(off)
  LossPart t = {0.f, 0.f, 0.f, 0.f};
  for (int i = threadIdx.x; i < nparts; i += 256) {
    LossPart p = parts[i];
    t.rgb += p.rgb; t.dep += p.dep; t.da += p.da; t.db += p.db;
  }
  float v[4] = {t.rgb, t.dep, t.da, t.db};
#pragma unroll
  for (int k = 0; k < 4; ++k) v[k] = wave_sum(v[k]);
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  if (lane == 0) red[wv] = {v[0], v[1], v[2], v[3]};
  __syncthreads();
  if (threadIdx.x == 0) {
    LossPart s = red[0];
    for (int w = 1; w < 4; ++w) { s.rgb += red[w].rgb; s.dep += red[w].dep; s.da += red[w].da; s.db += red[w].db; }
    if (loss) loss[0] = alpha * (s.rgb * inv_rgb) + (1.f - alpha) * (s.dep * inv_dep);
    if (da) da[0] = s.da;
    if (db) db[0] = s.db;
  }
  __syncthreads();
}

__device__ __forceinline__ void masked_adam_row(int r, int width, float* __restrict__ p, const float* __restrict__ g,
                                                float* __restrict__ m, float* __restrict__ v, int32_t* __restrict__ step,
                                                float lr, float b1, float b2, float eps) {
#pragma clang fp contract(off)
  int st = step[r] + 1;
  step[r] = st;
  float bc1 = 1.f - powf(b1, (float)st), bc2 = 1.f - powf(b2, (float)st);
  float step_size = lr / bc1, bc2s = sqrtf(bc2);
  for (int k = 0; k < width; ++k) {
    int i = r * width + k;
    float gi = g[i], mi = m[i], vi = v[i];
    mi = mi + (gi - mi) * (1.f - b1);
    vi = vi * b2 + (1.f - b2) * gi * gi;
    p[i] = p[i] - step_size * (mi / (sqrtf(vi) / bc2s + eps));
    m[i] = mi;
    v[i] = vi;
  }
}

#define adam_update(p, g, m, v, GRP, c)                      \
  do {                                                       \
    m = m + (g - m) * (1.f - c.b1);                          \
    v = v * c.b2 + (1.f - c.b2) * g * g;                     \
    float denom_ = sqrtf(v) / c.bc2_sqrt[GRP] + c.eps;       \
    p = p - c.step_size[GRP] * (m / denom_);                 \
  } while (0)

// MODE 0: gradient = sink (read, then zeroed)            -- sgr_gaussian_adam_step
// MODE 1: gradient = sink + gathered (sink zeroed)        -- fused tail, sinks may hold earlier contributions
// MODE 2: gradient = gathered (sinks known to be zero)    -- fused tail, steady state: the sinks are never touched
template <int MODE>
__device__ __forceinline__ float take_grad(float* __restrict__ sink, int64_t j, float gathered) {
  if (MODE == 2) return gathered;
  float g = sink[j];
  sink[j] = 0.f;
  return MODE == 1 ? g + gathered : g;
}

template <int MODE>
__device__ __forceinline__ void gaussian_adam_one(int64_t i, const AdamGroups& G, const AdamConst& c, float iso_coef,
                                                  const float* e /*[14] gathered or zeros*/, float* __restrict__ s_out,
                                                  float* __restrict__ r_out, float* __restrict__ o_out, float* keep = nullptr) {
  // keep (optional, registers of the caller): [0..2] the xyz row as stored, [3..5] the s_out row, [6..9] the r_out row -- the very
  // values a load of those rows would return afterwards (K1 with the carried step takes its phase-A inputs from here)
  // every product and sum below is rounded on its own: the instantiations (and the separate activate_kernel)
  // must agree bit for bit, which fused multiply-adds chosen per instantiation would not guarantee
#pragma clang fp contract(off)
  // xyz and f_dc: identity activations.  (3-float rows move as one 12-byte access per array: three dword accesses with a
  // 12-byte lane stride use a third of every cache line they touch)
#pragma unroll
  for (int grp = 0; grp < 2; ++grp) {
    const SgrAdamGroup& A = G.g[grp];
    if (i < G.r0[grp] || i >= G.r1[grp]) continue;
    float g[3];
    if (MODE == 2) {
      g[0] = e[3 * grp]; g[1] = e[3 * grp + 1]; g[2] = e[3 * grp + 2];
    } else {
      F3 gs = ld3(A.grad + 3 * i);
      st3(A.grad + 3 * i, F3{0.f, 0.f, 0.f});
      g[0] = gs.x; g[1] = gs.y; g[2] = gs.z;
      if (MODE == 1) { g[0] = g[0] + e[3 * grp]; g[1] = g[1] + e[3 * grp + 1]; g[2] = g[2] + e[3 * grp + 2]; }
    }
    if (A.skip) continue;
    F3 p3 = ld3(A.param + 3 * i), m3 = ld3(A.exp_avg + 3 * i), v3 = ld3(A.exp_avg_sq + 3 * i);
    float p[3] = {p3.x, p3.y, p3.z}, m[3] = {m3.x, m3.y, m3.z}, v[3] = {v3.x, v3.y, v3.z};
#pragma unroll
    for (int k = 0; k < 3; ++k) adam_update(p[k], g[k], m[k], v[k], grp, c);
    st3(A.param + 3 * i, F3{p[0], p[1], p[2]});
    st3(A.exp_avg + 3 * i, F3{m[0], m[1], m[2]});
    st3(A.exp_avg_sq + 3 * i, F3{v[0], v[1], v[2]});
    if (keep && grp == 0) { keep[0] = p[0]; keep[1] = p[1]; keep[2] = p[2]; }
  }
  if (i >= G.r0[2] && i < G.r1[2]) {   // opacity: sigmoid
    const SgrAdamGroup& A = G.g[2];
    float p = A.param[i];
    float sg = 1.f / (1.f + expf(-p));
    float g = take_grad<MODE>(A.grad, i, e[6]) * sg * (1.f - sg);
    if (!A.skip) {
      float m = A.exp_avg[i], v = A.exp_avg_sq[i];
      adam_update(p, g, m, v, 2, c);
      A.param[i] = p; A.exp_avg[i] = m; A.exp_avg_sq[i] = v;
    }
    if (o_out) o_out[i] = 1.f / (1.f + expf(-p));
  }
  if (i >= G.r0[3] && i < G.r1[3]) {   // scaling: exp, plus d/ds of iso_weight * mean_{N,3} |s - mean_3(s)|
    const SgrAdamGroup& A = G.g[3];
    const F3 p3 = ld3(A.param + 3 * i);
    float p[3] = {p3.x, p3.y, p3.z}, s[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) s[k] = expf(p[k]);
    float mean = (s[0] + s[1] + s[2]) / 3.f;
    float sg[3], ssum = 0.f;
#pragma unroll
    for (int k = 0; k < 3; ++k) { float d = s[k] - mean; sg[k] = d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f); ssum += sg[k]; }
    float gin[3];
    if (MODE == 2) {
      gin[0] = e[7]; gin[1] = e[8]; gin[2] = e[9];
    } else {
      F3 gs = ld3(A.grad + 3 * i);
      st3(A.grad + 3 * i, F3{0.f, 0.f, 0.f});
      gin[0] = gs.x; gin[1] = gs.y; gin[2] = gs.z;
      if (MODE == 1) { gin[0] = gin[0] + e[7]; gin[1] = gin[1] + e[8]; gin[2] = gin[2] + e[9]; }
    }
    if (!A.skip) {
      F3 m3 = ld3(A.exp_avg + 3 * i), v3 = ld3(A.exp_avg_sq + 3 * i);
      float m[3] = {m3.x, m3.y, m3.z}, v[3] = {v3.x, v3.y, v3.z};
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        float gs = gin[k] + iso_coef * (sg[k] - ssum / 3.f);
        float g = gs * s[k];
        adam_update(p[k], g, m[k], v[k], 3, c);
      }
      st3(A.param + 3 * i, F3{p[0], p[1], p[2]});
      st3(A.exp_avg + 3 * i, F3{m[0], m[1], m[2]});
      st3(A.exp_avg_sq + 3 * i, F3{v[0], v[1], v[2]});
    }
    if (s_out) {
      const F3 so = F3{expf(p[0]), expf(p[1]), expf(p[2])};
      st3(s_out + 3 * i, so);
      if (keep) { keep[3] = so.x; keep[4] = so.y; keep[5] = so.z; }
    }
  }
  if (i >= G.r0[4] && i < G.r1[4]) {   // rotation: x / max(|x|, 1e-12)
    const SgrAdamGroup& A = G.g[4];
    float4 x = *(const float4*)(A.param + 4 * i);
    float4 gy;
    if (MODE == 2) {
      gy = make_float4(e[10], e[11], e[12], e[13]);
    } else {
      gy = *(const float4*)(A.grad + 4 * i);
      *(float4*)(A.grad + 4 * i) = make_float4(0.f, 0.f, 0.f, 0.f);
      if (MODE == 1) { gy.x += e[10]; gy.y += e[11]; gy.z += e[12]; gy.w += e[13]; }
    }
    float nrm = sqrtf(x.x * x.x + x.y * x.y + x.z * x.z + x.w * x.w);
    float gx[4];
    if (nrm > 1e-12f) {
      float inv = 1.f / nrm;
      float y[4] = {x.x * inv, x.y * inv, x.z * inv, x.w * inv};
      float dot = y[0] * gy.x + y[1] * gy.y + y[2] * gy.z + y[3] * gy.w;
      gx[0] = (gy.x - y[0] * dot) * inv; gx[1] = (gy.y - y[1] * dot) * inv;
      gx[2] = (gy.z - y[2] * dot) * inv; gx[3] = (gy.w - y[3] * dot) * inv;
    } else {
      gx[0] = gy.x * 1e12f; gx[1] = gy.y * 1e12f; gx[2] = gy.z * 1e12f; gx[3] = gy.w * 1e12f;
    }
    float pp[4] = {x.x, x.y, x.z, x.w};
    if (!A.skip) {
      float4 m = *(const float4*)(A.exp_avg + 4 * i), v = *(const float4*)(A.exp_avg_sq + 4 * i);
      float mm[4] = {m.x, m.y, m.z, m.w}, vv[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
      for (int k = 0; k < 4; ++k) adam_update(pp[k], gx[k], mm[k], vv[k], 4, c);
      *(float4*)(A.param + 4 * i) = make_float4(pp[0], pp[1], pp[2], pp[3]);
      *(float4*)(A.exp_avg + 4 * i) = make_float4(mm[0], mm[1], mm[2], mm[3]);
      *(float4*)(A.exp_avg_sq + 4 * i) = make_float4(vv[0], vv[1], vv[2], vv[3]);
    }
    if (r_out) {      // same expression as activate_kernel
      float nn = fmaxf(sqrtf(pp[0] * pp[0] + pp[1] * pp[1] + pp[2] * pp[2] + pp[3] * pp[3]), 1e-12f);
      const float4 ro = make_float4(pp[0] / nn, pp[1] / nn, pp[2] / nn, pp[3] / nn);
      *(float4*)(r_out + 4 * i) = ro;
      if (keep) { keep[6] = ro.x; keep[7] = ro.y; keep[8] = ro.z; keep[9] = ro.w; }
    }
  }
}

// LDS of the optimiser pass: per-view pointers (the gather indexes them per LANE; a by-value kernarg table cannot be) and the
// riders' reduction slots
struct AdamShared {
  const char* scratch[kMaxViews];
  const int32_t* radii[kMaxViews];
  uint32_t over[kMaxViews];
  LossPart red[4];
};

// Rider block of view v (one per view, independent of every other block): fixed-order sum of the view's per-tile loss parts,
// then the exposure (keyframe) Adam step of the ONE slab row this view's exposure gradient lives in (every active row belongs
// to a window keyframe, and those are rendered every iteration: mapper.py:426-447, 1096-1111)
__device__ __forceinline__ void adam_rider_view(const FusedAdam& fa, const char* saved_v, int v, AdamShared& sh) {
  loss_final_view((const LossPart*)fa.tail_parts[v], fa.tail_nparts, fa.tail_inv_rgb, fa.tail_inv_dep, fa.tail_alpha,
                  fa.tail_loss[v], fa.tail_da[v], fa.tail_db[v], sh.red);
  // (a view whose forward ran out of pair capacity rendered truncated lists: it takes no part in this step, see below)
  if (threadIdx.x == 0 && fa.exp_rows > 0 && fa.tail_da[v] && ((const SavedHeader*)saved_v)->overflow == 0u) {
    const ptrdiff_t d = fa.tail_da[v] - fa.exp_grad;
    if (d >= 0 && d < (ptrdiff_t)fa.exp_rows * fa.exp_width && d % fa.exp_width == 0) {
      const int r = (int)(d / fa.exp_width);
      if (fa.exp_active[r])
        masked_adam_row(r, fa.exp_width, fa.exp_param, fa.exp_grad, fa.exp_avg, fa.exp_avg_sq, fa.exp_step, fa.exp_lr,
                        fa.exp_b1, fa.exp_b2, fa.exp_eps);
    }
  }
}

// The pass itself for the 256 Gaussians seg * 256 + threadIdx.x (every thread of the block calls it: one barrier inside).
// thread = Gaussian: adds up its gradient records over the views of the batch in view order (exactly grad_gather_kernel's
// sum), then the Adam step of all five groups, then the activations the next forward renders with.  MODE 3 (multi-GPU) stops
// after the sum: it is added to the gradient buffers (what grad_gather_kernel does with accumulate = 1); MODE 4 stores it
// instead (for every Gaussian), so that the flat buffer the ranks exchange is never zeroed in between.
template <int MODE>
__device__ __forceinline__ void gather_adam_segment(const FusedAdam& fa, const AdamViews& av, const LOff& L, int seg, AdamShared& sh,
                                                    float* keep = nullptr) {
  const int nviews = av.nviews;
#pragma unroll
  for (int u = 0; u < kMaxViews; ++u)
    if ((int)threadIdx.x == u && u < nviews) {
      sh.scratch[u] = av.scratch[u];
      sh.radii[u] = av.radii[u];
      sh.over[u] = ((const SavedHeader*)av.saved[u])->overflow;
    }
  __syncthreads();
  // Capacity overflow (R > cap): the view's lists were truncated and some of its partial slots were never written.  Such a
  // view contributes NOTHING to this step -- no gradient, no densification statistics, no exposure update -- instead of
  // feeding uninitialised sums into the Adam moments; the host sees header.overflow at its next check and grows the capacity.
  uint32_t truncated = 0u;
  for (int u = 0; u < nviews; ++u) truncated |= (sh.over[u] != 0u ? 1u : 0u) << u;
  const int i = seg * 256 + (int)threadIdx.x;
  if (i >= L.N) return;
  float a[14];
#pragma unroll
  for (int k = 0; k < 14; ++k) a[k] = 0.f;
  float st_norm = 0.f, st_cnt = 0.f, st_maxr = 0.f;
  // K1 left one word per Gaussian with the views of the batch that see it.  Every lane walks ITS OWN set bits in
  // ascending view order (the fixed summation order of grad_gather_kernel): a wave makes max-over-lanes(popcount) record
  // round trips -- about 3 for a SLAM batch -- instead of one per view of the batch.
  uint32_t seen = 0u;
  for (int p = 0; p < min(av.k1_parts, nviews); ++p) seen |= ((const uint32_t*)(av.saved[0] + L.o_vismask))[(size_t)p * L.N + i];
  seen &= ~truncated;
  const bool any = seen != 0u;
  while (seen) {
    const int v = __builtin_ctz(seen);
    seen &= seen - 1u;
    const float4* rec = (const float4*)(sh.scratch[v] + L.o_gradrec) + (size_t)i * 4;
    const int r = sh.radii[v][i];
    float4 r0 = rec[0], r1 = rec[1], r2 = rec[2], r3 = rec[3];
    a[0] += r0.x; a[1] += r0.y; a[2] += r0.z; a[3] += r0.w; a[4] += r1.x; a[5] += r1.y; a[6] += r1.z; a[7] += r1.w;
    a[8] += r2.x; a[9] += r2.y; a[10] += r2.z; a[11] += r2.w; a[12] += r3.x; a[13] += r3.y;
    st_norm += sqrtf(r3.z * r3.z + r3.w * r3.w);
    st_cnt += 1.f;
    st_maxr = fmaxf(st_maxr, (float)r);
  }
  if (any && fa.stat_accum) {
    fa.stat_accum[i] += st_norm;
    fa.stat_denom[i] += st_cnt;
    fa.stat_maxr[i] = fmaxf(fa.stat_maxr[i], st_maxr);
  }
  if (MODE == 3) {          // multi-GPU iteration: the sums go into the flat gradient buffer the ranks all-reduce
    if (!any) return;
    float* g0 = fa.G.g[0].grad + 3 * (size_t)i; float* g1 = fa.G.g[1].grad + 3 * (size_t)i; float* g3 = fa.G.g[3].grad + 3 * (size_t)i;
    float* g4 = fa.G.g[4].grad + 4 * (size_t)i;
    g0[0] += a[0]; g0[1] += a[1]; g0[2] += a[2];
    g1[0] += a[3]; g1[1] += a[4]; g1[2] += a[5];
    fa.G.g[2].grad[i] += a[6];
    g3[0] += a[7]; g3[1] += a[8]; g3[2] += a[9];
    g4[0] += a[10]; g4[1] += a[11]; g4[2] += a[12]; g4[3] += a[13];
    return;
  }
  if (MODE == 4) {          // ... STORED, for every Gaussian (zeros where no view sees it): nobody has to zero the buffer in between
    st3(fa.G.g[0].grad + 3 * (size_t)i, F3{a[0], a[1], a[2]});
    st3(fa.G.g[1].grad + 3 * (size_t)i, F3{a[3], a[4], a[5]});
    fa.G.g[2].grad[i] = a[6];
    st3(fa.G.g[3].grad + 3 * (size_t)i, F3{a[7], a[8], a[9]});
    *(float4*)(fa.G.g[4].grad + 4 * (size_t)i) = make_float4(a[10], a[11], a[12], a[13]);
    return;
  }
  gaussian_adam_one<MODE >= 3 ? 1 : MODE>(i, fa.G, fa.c, fa.iso_coef, a, fa.s_out, fa.r_out, fa.o_out, keep);
}

}  // namespace sgr
