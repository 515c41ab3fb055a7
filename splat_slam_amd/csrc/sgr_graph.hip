// The two device passes of the tracker's factor graph (FactorGraph, thirdparty/glorie_slam/factor_graph.py):
//   sgr_graph_reproject          projective_transform with per-frame intrinsics (geom/projective_ops.py:110-139) and, with a target,
//                                the motion features of FactorGraph.update (:233-235), one launch
//   sgr_graph_select_proximity   the greedy edge selection of add_proximity_factors (:337-397)
//   sgr_graph_select_backend     the one of add_backend_proximity_factors (:400-477)
// Semantics, the tie rule and the way the selection is parallelised are stated in DESIGN.md section 3, "Factor graph".  The selection
// is one workgroup: the visit is a sequential dependency, and at most 512 x 512 entries are one workgroup's worth of work; there is
// no waiting of one workgroup on another, and every loop has a trip bound that follows from the sizes.  No host synchronisation, no
// allocation; every output is bitwise reproducible.
#include <cmath>
#include <cstdint>

#include "sgr_common.h"
#include "sgr_dba_device.h"

namespace sgr {
int set_error(int code, const char* fmt, ...);

namespace {

using dba::frame_ok;

constexpr int kThreads = 256;
constexpr float kMinDepth = 0.2f;           // MIN_DEPTH of projective_ops.py; the projection replaces z below half of it by 1
constexpr float kMotionClamp = 64.f;
constexpr int kMaxEdges = SGR_GRAPH_MAX_EDGES;      // a grid dimension


// ================================================================================================================================
// reprojection.  One thread per pixel, blockIdx.y is the edge.  Thread 0 does the pose algebra of the edge once and leaves
// (t, q, K_i, K_j) in LDS.  Consecutive lanes are consecutive pixels: disps is read and valid written 4 bytes per lane, coords
// (channel-last) and target are one 8-byte access per lane, and each of motn's four planes (channel-first) is 4 bytes per lane,
// so every access of a wave is one contiguous run.
// ================================================================================================================================

__device__ __forceinline__ float clamp_motion(float v) {     // (comparisons, not fminf / fmaxf: a NaN stays a NaN, as torch.clamp has it)
  return v < -kMotionClamp ? -kMotionClamp : (v > kMotionClamp ? kMotionClamp : v);
}

template <bool MOTION>
__global__ void __launch_bounds__(kThreads) reproject_kernel(int nv, int P, int wd, const float* __restrict__ poses,
                                                             const float* __restrict__ disps, const float* __restrict__ intr,
                                                             const int64_t* __restrict__ ii, const int64_t* __restrict__ jj,
                                                             const float* __restrict__ target, float* __restrict__ coords,
                                                             float* __restrict__ valid, float* __restrict__ motn) {
  __shared__ float sh[16];                    // t [3], q [4], K_i [4], K_j [4], in range
  const int e = blockIdx.y;
  const int64_t ix = ii[e], jx = jj[e];
  if (threadIdx.x == 0) {
    const bool ok = frame_ok(ix, nv) && frame_ok(jx, nv);
    sh[15] = ok ? 1.f : 0.f;
    if (ok) {
      if (ix == jx) {
        sh[0] = dba::kStereoBaseline;
        sh[1] = sh[2] = sh[3] = sh[4] = sh[5] = 0.f;
        sh[6] = 1.f;
      } else {
        dba::rel_se3(poses + 7 * ix, poses + 7 * jx, sh, sh + 3);
      }
      for (int k = 0; k < 4; ++k) {
        sh[7 + k] = intr[4 * ix + k];
        sh[11 + k] = intr[4 * jx + k];
      }
    }
  }
  __syncthreads();
  const int k = blockIdx.x * kThreads + threadIdx.x;
  if (k >= P) return;
  const size_t o = (size_t)e * P + k;
  if (sh[15] == 0.f) {
    ((float2*)coords)[o] = make_float2(0.f, 0.f);
    valid[o] = 0.f;
    if (MOTION) {
      float* m = motn + (size_t)e * 4 * P + k;
      m[0] = m[P] = m[2 * (size_t)P] = m[3 * (size_t)P] = 0.f;
    }
    return;
  }
  const int y = k / wd, x = k - (k / wd) * wd;
  const float gx = (float)x, gy = (float)y;
  const float d = disps[(size_t)ix * P + k];
  const float X0[3] = {(gx - sh[9]) / sh[7], (gy - sh[10]) / sh[8], 1.f};
  float X1[3];
  dba::act_so3(sh + 3, X0, X1);
  X1[0] += d * sh[0];
  X1[1] += d * sh[1];
  X1[2] += d * sh[2];
  const float Z = X1[2] < 0.5f * kMinDepth ? 1.f : X1[2];
  const float cx = sh[11] * (X1[0] / Z) + sh[13], cy = sh[12] * (X1[1] / Z) + sh[14];
  ((float2*)coords)[o] = make_float2(cx, cy);
  valid[o] = X1[2] > kMinDepth ? 1.f : 0.f;
  if (MOTION) {
    const float2 tg = ((const float2*)target)[o];
    float* m = motn + (size_t)e * 4 * P + k;
    m[0] = clamp_motion(cx - gx);
    m[P] = clamp_motion(cy - gy);
    m[2 * (size_t)P] = clamp_motion(tg.x - cx);
    m[3 * (size_t)P] = clamp_motion(tg.y - cy);
  }
}

// ================================================================================================================================
// edge selection: one 1024-thread workgroup.
//   1  mask       w = d, or inf where rule 1 says so (NaN -> inf, -0 -> +0); the diamonds around the existing edges (frontend)
//   2  window     the local-window pairs go to es at positions known in closed form; their entries become inf
//   3  compact    the entries with w <= thresh, in flat-index order (exclusive scan)
//   4  sort       stable LSD radix sort of the order-preserving integer image of w, 4 digits of 8 bits: equal distances stay in
//                 flat-index order, which is the tie rule.  Thread t owns a contiguous chunk and a column of digit counters.
//   5  visit      wave 0 takes 64 sorted candidates at a time against a suppression bitmap in LDS; the first live lane is the
//                 next pick, its region goes into the bitmap, and the lanes of the batch that lie in it are dropped in registers.
// ================================================================================================================================

constexpr int kSelThreads = 1024;
constexpr int kMaxSide = SGR_GRAPH_MAX_SIDE;
constexpr int kDigits = 256;
constexpr int kLoopGap = 20;                // a loop edge joins frames more than this apart
enum { kFrontend = 0, kBackend = 1, kBackendLoop = 2 };

struct SelArgs {
  const float* d;
  int rows, cols, row0, col0;               // entry (r, c) is the frame pair (row0 + r, col0 + c); row0 + rows == col0 + cols
  const int64_t *ii_old, *jj_old;
  int num_old;
  int rad, nms;
  float thresh;
  int max_factors;
  int64_t* es;
  int cap;                                  // pairs es has room for
  int32_t* counts;                          // [0] pairs emitted, [1] loop pairs among them
  float* w;                                 // scratch, see carve_select
  int* pos;
  uint32_t *key_a, *key_b;
  int *idx_a, *idx_b;
  int* digit_counts;
};

__device__ __forceinline__ uint32_t key_of(float v) {        // v1 < v2  <=>  key_of(v1) < key_of(v2), for every non-NaN v
  const uint32_t u = __float_as_uint(v);
  return (u >> 31) ? ~u : (u | 0x80000000u);
}

__device__ __forceinline__ int diamond_radius(int i, int j, int nms) { return max(min(abs(i - j) - 2, nms), 0); }

// pairs of the local windows of the rows before frame i:  sum over k in [0, i) of min(r1, k)
__device__ __forceinline__ int window_pairs_before(int i, int r1) {
  if (i <= 0 || r1 <= 0) return 0;
  return i <= r1 ? i * (i - 1) / 2 : r1 * (r1 - 1) / 2 + (i - r1) * r1;
}

template <int MODE>
__global__ void __launch_bounds__(kSelThreads) select_kernel(SelArgs a) {
  __shared__ int lds[kSelThreads];
  __shared__ uint32_t bitmap[kMaxSide * kMaxSide / 32];
  const int t = threadIdx.x, n = a.rows * a.cols, r1 = max(a.rad + 1, 0);
  const int nms = a.nms;

  // ---- 1: mask
  for (int k = t; k < n; k += kSelThreads) {
    const int i = a.row0 + k / a.cols, j = a.col0 + k % a.cols;
    float v = a.d[k];
    const float cut = MODE == kFrontend ? 100.f : a.thresh;
    if (!(v <= cut) || i - a.rad < j) v = INFINITY;
    a.w[k] = v + 0.f;
  }
  for (int k = t; k < kMaxSide * kMaxSide / 32; k += kSelThreads) bitmap[k] = 0u;
  __syncthreads();
  if (MODE == kFrontend) {
    const int side = 2 * nms + 1;
    for (int k = t; k < a.num_old; k += kSelThreads) {
      const int64_t i = a.ii_old[k], j = a.jj_old[k];
      // (an edge further than nms outside the matrix reaches no entry; the test also keeps the int arithmetic below in range)
      if (i < (int64_t)a.row0 - nms || i >= (int64_t)a.row0 + a.rows + nms || j < (int64_t)a.col0 - nms ||
          j >= (int64_t)a.col0 + a.cols + nms)
        continue;
      const int r = diamond_radius((int)i, (int)j, nms);
      for (int c = 0; c < side * side; ++c) {
        const int di = c / side - nms, dj = c % side - nms;
        if (abs(di) + abs(dj) > r) continue;
        const int rr = (int)i + di - a.row0, cc = (int)j + dj - a.col0;
        if (rr >= 0 && rr < a.rows && cc >= 0 && cc < a.cols) a.w[rr * a.cols + cc] = INFINITY;     // (every writer writes inf)
      }
    }
    __syncthreads();
  }

  // ---- 2: local windows
  const int base = window_pairs_before(a.row0, r1);
  const int local_pairs = 2 * (window_pairs_before(a.row0 + a.rows, r1) - base);
  for (int r = t; r < a.rows; r += kSelThreads) {
    const int i = a.row0 + r, jlo = max(i - r1, 0);
    int o = 2 * (window_pairs_before(i, r1) - base);
    for (int j = jlo; j < i; ++j, o += 2) {
      if (o + 2 <= a.cap) {
        a.es[2 * o] = i;
        a.es[2 * o + 1] = j;
        a.es[2 * o + 2] = j;
        a.es[2 * o + 3] = i;
      }
      const int cc = j - a.col0;
      if (cc >= 0 && cc < a.cols) a.w[r * a.cols + cc] = INFINITY;
    }
  }
  __syncthreads();

  // ---- 3: compact the candidates
  for (int k = t; k < n; k += kSelThreads) a.pos[k] = a.w[k] <= a.thresh ? 1 : 0;
  __syncthreads();
  const int m = dba::scan_1024(n, a.pos, a.pos, lds);
  __syncthreads();
  for (int k = t; k < n; k += kSelThreads) {
    const float v = a.w[k];
    if (v <= a.thresh) {
      const int p = a.pos[k];
      a.key_a[p] = key_of(v);
      a.idx_a[p] = k;
    }
  }
  __syncthreads();

  // ---- 4: sort
  const int cols_used = min(kSelThreads, max(1, (m + 15) / 16)), chunk = (m + cols_used - 1) / cols_used;
  const int lo = min(m, t * chunk), hi = t < cols_used ? min(m, lo + chunk) : lo;
  uint32_t *ka = a.key_a, *kb = a.key_b;
  int *ia = a.idx_a, *ib = a.idx_b;
  for (int pass = 0; pass < 4 && m > 1; ++pass) {
    const int shift = 8 * pass;
    if (t < cols_used)
      for (int dg = 0; dg < kDigits; ++dg) a.digit_counts[dg * cols_used + t] = 0;
    for (int k = lo; k < hi; ++k) a.digit_counts[((ka[k] >> shift) & 0xffu) * cols_used + t] += 1;
    __syncthreads();
    dba::scan_1024(kDigits * cols_used, a.digit_counts, a.digit_counts, lds);
    __syncthreads();
    for (int k = lo; k < hi; ++k) {
      const uint32_t key = ka[k];
      const int p = a.digit_counts[((key >> shift) & 0xffu) * cols_used + t]++;
      kb[p] = key;
      ib[p] = ia[k];
    }
    __syncthreads();
    uint32_t* ks = ka;
    ka = kb;
    kb = ks;
    int* is = ia;
    ia = ib;
    ib = is;
  }

  // ---- 5: visit
  if (t >= 64) return;
  int len = min(local_pairs, a.cap), loops = 0;
  bool stop = false;
  for (int b0 = 0; b0 < m && !stop; b0 += 64) {
    const int k = b0 + t < m ? ia[b0 + t] : -1;
    const int r = k >= 0 ? k / a.cols : 0, c = k >= 0 ? k % a.cols : 0;
    bool alive = k >= 0 && !((bitmap[k >> 5] >> (k & 31)) & 1u);
    for (int step = 0; step < 64; ++step) {
      const unsigned long long live = __ballot(alive);
      if (live == 0ull) break;
      if (len > a.max_factors) {
        stop = true;
        break;
      }
      const int first = __ffsll((long long)live) - 1;
      const int pr = __shfl(r, first), pc = __shfl(c, first);
      const int pi = a.row0 + pr, pj = a.col0 + pc;
      // the pick's pairs, written by its own lane in the order of the sequential rule
      int emitted = 0;
      if (t == first) {
        if (MODE == kBackendLoop) {
          const int t_end = a.row0 + a.rows;
          for (int si = max(pi - 1, a.row0); si < min(pi + 2, t_end); ++si)
            for (int sj = max(pj - 1, a.col0); sj < min(pj + 2, t_end); ++sj)
              if (a.d[(si - a.row0) * a.cols + (sj - a.col0)] <= a.thresh && si - sj > kLoopGap && len + emitted < a.cap) {
                a.es[2 * (len + emitted)] = si;
                a.es[2 * (len + emitted) + 1] = sj;
                ++emitted;
              }
        } else if (len + 2 <= a.cap) {
          a.es[2 * len] = pi;
          a.es[2 * len + 1] = pj;
          a.es[2 * len + 2] = pj;
          a.es[2 * len + 3] = pi;
          emitted = 2;
        }
      }
      emitted = __shfl(emitted, first);
      len += emitted;
      if (MODE == kBackendLoop) loops += emitted;
      // suppression: the pick's region into the bitmap for the batches to come, and out of this batch in registers
      const int rad_p = MODE == kFrontend ? diamond_radius(pi, pj, nms) : nms, side = 2 * rad_p + 1;
      for (int q = t; q < side * side; q += 64) {
        const int di = q / side - rad_p, dj = q % side - rad_p;
        if (MODE == kFrontend && abs(di) + abs(dj) > rad_p) continue;
        const int rr = pr + di, cc = pc + dj;
        if (rr >= 0 && rr < a.rows && cc >= 0 && cc < a.cols) {
          const int cell = rr * a.cols + cc;
          atomicOr(&bitmap[cell >> 5], 1u << (cell & 31));
        }
      }
      __threadfence_block();
      const int di = abs(r - pr), dj = abs(c - pc);
      if (t == first || (MODE == kFrontend ? di + dj <= rad_p : (di <= rad_p && dj <= rad_p))) alive = false;
    }
  }
  if (t == 0) {
    a.counts[0] = len;
    a.counts[1] = loops;
  }
}

size_t carve_select(int n, char* base, SelArgs* a) {
  size_t off = 0;
  auto take = [&](size_t bytes) {
    char* p = base ? base + off : nullptr;
    off += align_up(bytes);
    return p;
  };
  float* w = (float*)take((size_t)n * sizeof(float));
  int* pos = (int*)take((size_t)(n + 1) * sizeof(int));
  uint32_t* key_a = (uint32_t*)take((size_t)n * sizeof(uint32_t));
  uint32_t* key_b = (uint32_t*)take((size_t)n * sizeof(uint32_t));
  int* idx_a = (int*)take((size_t)n * sizeof(int));
  int* idx_b = (int*)take((size_t)n * sizeof(int));
  // (at most max(16, n / 16 + 1) <= 1024 columns of 256 counters, and the scan's total)
  int* digit_counts = (int*)take(((size_t)kDigits * kSelThreads + 1) * sizeof(int));
  if (a) {
    a->w = w;
    a->pos = pos;
    a->key_a = key_a;
    a->key_b = key_b;
    a->idx_a = idx_a;
    a->idx_b = idx_b;
    a->digit_counts = digit_counts;
  }
  return off;
}

bool select_sizes_ok(int rows, int cols) { return rows >= 1 && cols >= 1 && rows <= kMaxSide && cols <= kMaxSide; }

int select(int mode, const char* what, const float* d, int rows, int cols, int row0, int col0, const int64_t* ii_old,
           const int64_t* jj_old, int num_old, int rad, int nms, float thresh, int max_factors, int64_t* es, int cap, int32_t* counts,
           void* scratch, size_t scratch_bytes, void* stream) {
  if (!d || !es || !counts || !select_sizes_ok(rows, cols) || row0 < 0 || col0 < 0 || row0 > (1 << 14) || col0 > (1 << 14) ||
      row0 + rows != col0 + cols || num_old < 0 || (num_old > 0 && (!ii_old || !jj_old)) || rad < 0 || rad > (1 << 14) || nms < 0 || nms > kMaxSide ||
      !std::isfinite(thresh) || cap < 0)
    return set_error(SGR_ERR_INVALID, "%s: bad arguments (1 <= rows, cols <= %d, row0 + rows == col0 + cols, finite thresh, nms <= rows limit)", what,
                     kMaxSide);
  if (!scratch || ((uintptr_t)scratch & 15) != 0 || scratch_bytes < carve_select(rows * cols, nullptr, nullptr))
    return set_error(SGR_ERR_WORKSPACE, "%s: scratch too small or not 16-byte aligned", what);
  SelArgs a;
  a.d = d;
  a.rows = rows, a.cols = cols, a.row0 = row0, a.col0 = col0;
  a.ii_old = ii_old, a.jj_old = jj_old, a.num_old = num_old;
  a.rad = rad, a.nms = nms, a.thresh = thresh, a.max_factors = max_factors;
  a.es = es, a.cap = cap, a.counts = counts;
  carve_select(rows * cols, (char*)scratch, &a);
  hipStream_t st = (hipStream_t)stream;
  if (mode == kFrontend)
    hipLaunchKernelGGL(select_kernel<kFrontend>, dim3(1), dim3(kSelThreads), 0, st, a);
  else if (mode == kBackend)
    hipLaunchKernelGGL(select_kernel<kBackend>, dim3(1), dim3(kSelThreads), 0, st, a);
  else
    hipLaunchKernelGGL(select_kernel<kBackendLoop>, dim3(1), dim3(kSelThreads), 0, st, a);
  return hipGetLastError() == hipSuccess ? SGR_OK : set_error(SGR_ERR_HIP, "%s launch failed", what);
}

}  // namespace
}  // namespace sgr

using namespace sgr;

extern "C" {

int sgr_graph_reproject(const float* poses, int32_t num_poses, const float* disps, int32_t num_frames, int32_t ht, int32_t wd,
                        const float* intrinsics, const int64_t* ii, const int64_t* jj, int32_t num_edges, const float* target,
                        float* coords, float* valid, float* motn, void* stream) {
  if (!poses || !disps || !intrinsics || !ii || !jj || !coords || !valid || (target != nullptr) != (motn != nullptr) || num_poses < 0 ||
      num_frames < 0 || num_edges < 0 || ht <= 0 || wd <= 0 || (long long)ht * wd >= (1LL << 24) || ((uintptr_t)coords & 7) != 0 ||
      ((uintptr_t)target & 7) != 0)
    return set_error(SGR_ERR_INVALID, "graph_reproject: bad arguments (target and motn come together; coords, target 8-byte aligned)");
  if (num_edges > kMaxEdges) return set_error(SGR_ERR_CAPACITY, "graph_reproject: %d edges exceed the supported %d", num_edges, kMaxEdges);
  if (num_edges == 0) return SGR_OK;
  const int P = ht * wd, nv = num_poses < num_frames ? num_poses : num_frames;
  const dim3 grid(blocks_for(P), num_edges);
  if (motn)
    hipLaunchKernelGGL(reproject_kernel<true>, grid, dim3(kThreads), 0, (hipStream_t)stream, nv, P, wd, poses, disps, intrinsics, ii, jj,
                       target, coords, valid, motn);
  else
    hipLaunchKernelGGL(reproject_kernel<false>, grid, dim3(kThreads), 0, (hipStream_t)stream, nv, P, wd, poses, disps, intrinsics, ii, jj,
                       target, coords, valid, motn);
  return hipGetLastError() == hipSuccess ? SGR_OK : set_error(SGR_ERR_HIP, "graph_reproject launch failed");
}

size_t sgr_graph_select_scratch_bytes(int32_t rows, int32_t cols) {
  if (!select_sizes_ok(rows, cols)) return 0;
  return carve_select(rows * cols, nullptr, nullptr);
}

int sgr_graph_select_proximity(const float* d, int32_t t0, int32_t t1, int32_t t, const int64_t* ii_old, const int64_t* jj_old,
                               int32_t num_old, int32_t rad, int32_t nms, float thresh, int32_t max_factors, int64_t* es, int32_t cap,
                               int32_t* counts, void* scratch, size_t scratch_bytes, void* stream) {
  return select(kFrontend, "graph_select_proximity", d, t - t0, t - t1, t0, t1, ii_old, jj_old, num_old, rad, nms, thresh, max_factors,
                es, cap, counts, scratch, scratch_bytes, stream);
}

int sgr_graph_select_backend(const float* d, int32_t t_start, int32_t t_end, int32_t t_start_loop, int32_t loop, int32_t nms,
                             int32_t radius, float thresh, int32_t max_factors, int64_t* es, int32_t cap, int32_t* counts,
                             void* scratch, size_t scratch_bytes, void* stream) {
  return select(loop ? kBackendLoop : kBackend, "graph_select_backend", d, t_end - t_start_loop, t_end - t_start, t_start_loop, t_start,
                nullptr, nullptr, 0, radius, nms, thresh, max_factors, es, cap, counts, scratch, scratch_bytes, stream);
}

}  // extern "C"
