// TSDF fusion, marching cubes and mesh cleaning of eval_rendering's mesh branch (/root/reference/src/utils/eval_utils.py:70-74,
// 142-179, clean_mesh :331-379), after Open3D's ScalableTSDFVolume (RGB8) and trimesh:
//   sgr_tsdf_touch / sgr_tsdf_integrate        one chunk of <= 16 frames: allocate the units a frame's depth touches, then update
//                                              each touched unit with one workgroup per unit, frames in order (no float atomics)
//   sgr_tsdf_extract_count / sgr_tsdf_extract  marching cubes: units sorted by key, count pass, scan, emit pass
//   sgr_mesh_components / sgr_mesh_compact     union-find labels (minimum vertex id), component sizes, stable compaction
// (the scans and the compaction kernels: sgr_scan.h)
// Every assumption about Open3D's semantics is one named constant below (DESIGN.md section 3 lists them): none has been checked
// against Open3D itself.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>

#include "sgr_common.h"
#include "sgr_mc_table.h"
#include "sgr_scan.h"

namespace sgr {
int set_error(int code, const char* fmt, ...);

namespace {

// ---- Open3D ScalableTSDFVolume conventions (assumed)
constexpr int kUnitRes = 16;                    // (1) a unit is 16^3 voxels; key = floor(p / (16 voxel_length))
constexpr int kUnitVox = kUnitRes * kUnitRes * kUnitRes;
constexpr float kVoxelCentre = 0.5f;            // (1) voxel i of a unit has its centre at origin + (i + 0.5) voxel_length
constexpr int kTouchStride = 4;                 // (2) units touched by the stride-4 point cloud of the depth, +- sdf_trunc
constexpr float kPixelShift = 0.5f;             // (3) u_f = x fx / z + cx + 0.5, u = (int)u_f
constexpr float kPixelMin = 0.0001f;            // (3) 0.0001 <= u_f < W
constexpr float kColorScale = 255.f;            // (3) colour (image * 255) truncated to uint8, averaged on the 0..255 scale
// (3) sdf = (d - z) * |ray(u, v)|, updated where sdf > -sdf_trunc, tsdf = min(1, sdf / sdf_trunc), running means over w
// (4) a cube is voxel p and its seven +1 neighbours, skipped if any corner has weight 0 or no unit; bit i set where T_i < 0

constexpr int kThreads = 256;
constexpr uint64_t kEmpty = ~0ull;              // bit 63 is never set in a key
constexpr int kKeyBits = 21, kKeyBias = 1 << (kKeyBits - 1);
constexpr int kNb = 27;                         // the 3x3x3 units around a unit
constexpr int kStateCounters = 8;

__host__ __device__ inline uint64_t pack_key(int x, int y, int z) {
  return ((uint64_t)(uint32_t)(x + kKeyBias) << (2 * kKeyBits)) | ((uint64_t)(uint32_t)(y + kKeyBias) << kKeyBits) |
         (uint64_t)(uint32_t)(z + kKeyBias);
}
__device__ inline void unpack_key(uint64_t k, int& x, int& y, int& z) {
  const uint64_t m = (1ull << kKeyBits) - 1;
  x = (int)((k >> (2 * kKeyBits)) & m) - kKeyBias;
  y = (int)((k >> kKeyBits) & m) - kKeyBias;
  z = (int)(k & m) - kKeyBias;
}
__device__ inline bool key_in_range(int x, int y, int z) {
  return x >= -kKeyBias && x < kKeyBias && y >= -kKeyBias && y < kKeyBias && z >= -kKeyBias && z < kKeyBias;
}
__device__ inline uint32_t hash_key(uint64_t k) {
  k ^= k >> 33;
  k *= 0xff51afd7ed558ccdull;
  k ^= k >> 33;
  return (uint32_t)k;
}

struct State {            // carved from SgrTsdfVolume::state
  uint64_t* keys;         // [cap]
  int32_t* slot_unit;     // [cap] pool index of the slot's unit
  uint32_t* marks;        // [cap] bit f: frame f of the chunk touches the slot's unit
  int32_t* list;          // [cap] touched slots of the chunk
  int32_t* counters;      // [kStateCounters]
};
inline State carve_state(const SgrTsdfVolume* v) {
  const size_t cap = (size_t)v->hash_capacity;
  char* p = (char*)v->state;
  State s;
  s.keys = (uint64_t*)p;
  p += align_up(cap * 8);
  s.slot_unit = (int32_t*)p;
  p += align_up(cap * 4);
  s.marks = (uint32_t*)p;
  p += align_up(cap * 4);
  s.list = (int32_t*)p;
  p += align_up(cap * 4);
  s.counters = (int32_t*)p;
  return s;
}

__device__ inline int hash_find(const uint64_t* keys, uint32_t mask, uint64_t key) {
  uint32_t h = hash_key(key) & mask;
  for (uint32_t probe = 0; probe <= mask; ++probe) {
    const uint64_t k = keys[h];
    if (k == key) return (int)h;
    if (k == kEmpty) return -1;
    h = (h + 1) & mask;
  }
  return -1;
}

// find or insert; the inserting thread hands out the pool index.  -1: the table is full (counters[1] raised)
__device__ inline int hash_insert(uint64_t* keys, int32_t* slot_unit, int32_t* counters, uint32_t mask, uint64_t key, int unit) {
  uint32_t h = hash_key(key) & mask;
  for (uint32_t probe = 0; probe <= mask; ++probe) {
    uint64_t k = __hip_atomic_load(&keys[h], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (k == kEmpty) {
      k = atomicCAS((unsigned long long*)&keys[h], (unsigned long long)kEmpty, (unsigned long long)key);
      if (k == kEmpty) {
        slot_unit[h] = unit >= 0 ? unit : atomicAdd(&counters[0], 1);
        return (int)h;
      }
    }
    if (k == key) return (int)h;
    h = (h + 1) & mask;
  }
  atomicOr(&counters[1], 1);
  return -1;
}

struct FrameDev {
  const float* render;
  const float* depth;
  const float* gt_depth;
  const float* ea;
  const float* eb;
  float fx, fy, cx, cy, scale;
  float w2c[12];          // rows 0..2 of world -> camera
  float c2w[12];          // rows 0..2 of its inverse
};
struct FrameTab { FrameDev f[SGR_TSDF_MAX_FRAMES]; };

// depth as create_from_color_and_depth sees it: global_scale * rendered, 0 where the ground truth is 0, 0 beyond depth_trunc
__device__ inline float frame_depth(const FrameDev& f, int o, float depth_trunc) {
  float d = f.scale * f.depth[o];
  if (f.gt_depth && f.gt_depth[o] == 0.f) d = 0.f;
  return d > depth_trunc ? 0.f : d;
}

// colour byte of channel c: (clamp(exp(a) r + b, 0, 1) * 255) truncated (exposed_image, color_level of sgr_common.h)
__device__ inline float frame_color(const FrameDev& f, float ea, float eb, int c, size_t HW, int o) {
  return (float)color_level(exposed_image(ea, f.render[c * HW + o], eb));
}

// ---- touch: thread = sampled pixel of one frame (grid.y)
__global__ void __launch_bounds__(kThreads) tsdf_touch_kernel(FrameTab tab, int H, int W, float unit_len, float trunc,
                                                              float depth_trunc, uint64_t* keys, int32_t* slot_unit,
                                                              uint32_t* marks, int32_t* counters, uint32_t mask) {
  const FrameDev& f = tab.f[blockIdx.y];
  const int ws = (W + kTouchStride - 1) / kTouchStride, hs = (H + kTouchStride - 1) / kTouchStride;
  const int s = blockIdx.x * kThreads + threadIdx.x;
  if (s >= ws * hs) return;
  const int u = (s % ws) * kTouchStride, v = (s / ws) * kTouchStride;
  const float d = frame_depth(f, v * W + u, depth_trunc);
  if (!(d > 0.f)) return;
  const float xc = (u - f.cx) * d / f.fx, yc = (v - f.cy) * d / f.fy, zc = d;
  float p[3];
#pragma unroll
  for (int r = 0; r < 3; ++r) p[r] = f.c2w[4 * r] * xc + f.c2w[4 * r + 1] * yc + f.c2w[4 * r + 2] * zc + f.c2w[4 * r + 3];
  int lo[3], hi[3];
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    lo[r] = (int)floorf((p[r] - trunc) / unit_len);
    hi[r] = (int)floorf((p[r] + trunc) / unit_len);
  }
  if (!key_in_range(lo[0], lo[1], lo[2]) || !key_in_range(hi[0], hi[1], hi[2])) return;
  const uint32_t bit = 1u << blockIdx.y;
  for (int x = lo[0]; x <= hi[0]; ++x)
    for (int y = lo[1]; y <= hi[1]; ++y)
      for (int z = lo[2]; z <= hi[2]; ++z) {
        const int h = hash_insert(keys, slot_unit, counters, mask, pack_key(x, y, z), -1);
        if (h >= 0 && !(__hip_atomic_load(&marks[h], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & bit)) atomicOr(&marks[h], bit);
      }
}

// the chunk's touched slots (any order: every unit is then updated by its own workgroup)
__global__ void __launch_bounds__(kThreads) tsdf_list_kernel(const uint32_t* marks, int cap, int32_t* list, int32_t* counters) {
  const int s = blockIdx.x * kThreads + threadIdx.x;
  if (s < cap && marks[s]) list[atomicAdd(&counters[2], 1)] = s;
}

__global__ void __launch_bounds__(kThreads) tsdf_rehash_kernel(const uint64_t* src_keys, const int32_t* src_unit, int src_cap,
                                                               uint64_t* keys, int32_t* slot_unit, int32_t* counters, uint32_t mask) {
  const int s = blockIdx.x * kThreads + threadIdx.x;
  if (s < src_cap && src_keys[s] != kEmpty) hash_insert(keys, slot_unit, counters, mask, src_keys[s], src_unit[s]);
}

// ---- integrate: workgroup = touched unit, thread = 16 voxels; the unit's frames in chunk order, every voxel by one lane
__global__ void __launch_bounds__(kThreads) tsdf_integrate_kernel(FrameTab tab, int n, int H, int W, float voxel_len, float trunc,
                                                                  float depth_trunc, const uint64_t* keys,
                                                                  const int32_t* slot_unit, uint32_t* marks,
                                                                  const int32_t* list, int32_t* counters, float* pool,
                                                                  int pool_capacity) {
  const int slot = list[blockIdx.x];
  const uint32_t fmask = marks[slot];
  const int unit = slot_unit[slot];
  __syncthreads();
  if (threadIdx.x == 0) marks[slot] = 0u;
  if (unit < 0 || unit >= pool_capacity) {
    if (threadIdx.x == 0) atomicOr(&counters[3], 1);
    return;
  }
  int kx, ky, kz;
  unpack_key(keys[slot], kx, ky, kz);
  float* U = pool + (size_t)unit * SGR_TSDF_UNIT_FLOATS;
  const size_t HW = (size_t)H * W;
  for (int j = 0; j < kUnitVox / kThreads; ++j) {
    const int vi = j * kThreads + threadIdx.x;
    const int ix = vi & 15, iy = (vi >> 4) & 15, iz = vi >> 8;
    const float xw = ((float)(kx * kUnitRes + ix) + kVoxelCentre) * voxel_len;
    const float yw = ((float)(ky * kUnitRes + iy) + kVoxelCentre) * voxel_len;
    const float zw = ((float)(kz * kUnitRes + iz) + kVoxelCentre) * voxel_len;
    float T = U[vi], Wt = U[kUnitVox + vi], R = U[2 * kUnitVox + vi], G = U[3 * kUnitVox + vi], B = U[4 * kUnitVox + vi];
    bool dirty = false;
    for (int fi = 0; fi < n; ++fi) {
      if (!((fmask >> fi) & 1u)) continue;
      const FrameDev& f = tab.f[fi];
      const float x = f.w2c[0] * xw + f.w2c[1] * yw + f.w2c[2] * zw + f.w2c[3];
      const float y = f.w2c[4] * xw + f.w2c[5] * yw + f.w2c[6] * zw + f.w2c[7];
      const float z = f.w2c[8] * xw + f.w2c[9] * yw + f.w2c[10] * zw + f.w2c[11];
      if (!(z > 0.f)) continue;
      const float uf = x * f.fx / z + f.cx + kPixelShift, vf = y * f.fy / z + f.cy + kPixelShift;
      if (!(uf >= kPixelMin && uf < (float)W && vf >= kPixelMin && vf < (float)H)) continue;
      const int u = (int)uf, v = (int)vf, o = v * W + u;
      const float d = frame_depth(f, o, depth_trunc);
      if (!(d > 0.f)) continue;
      const float rx = (u - f.cx) / f.fx, ry = (v - f.cy) / f.fy;
      const float sdf = (d - z) * sqrtf(rx * rx + ry * ry + 1.f);
      if (!(sdf > -trunc)) continue;
      const float tsdf = fminf(1.f, sdf / trunc);
      const float ea = f.ea ? expf(f.ea[0]) : 1.f, eb = f.eb ? f.eb[0] : 0.f;
      const float w1 = Wt + 1.f;
      T = (T * Wt + tsdf) / w1;
      R = (R * Wt + frame_color(f, ea, eb, 0, HW, o)) / w1;
      G = (G * Wt + frame_color(f, ea, eb, 1, HW, o)) / w1;
      B = (B * Wt + frame_color(f, ea, eb, 2, HW, o)) / w1;
      Wt = w1;
      dirty = true;
    }
    if (dirty) {
      U[vi] = T;
      U[kUnitVox + vi] = Wt;
      U[2 * kUnitVox + vi] = R;
      U[3 * kUnitVox + vi] = G;
      U[4 * kUnitVox + vi] = B;
    }
  }
}

// ---- extraction
__global__ void __launch_bounds__(kThreads) gather_units_kernel(const uint64_t* keys, const int32_t* slot_unit, int cap,
                                                                uint64_t* skeys, int32_t* sunit, int32_t* cursor) {
  const int s = blockIdx.x * kThreads + threadIdx.x;
  if (s < cap && keys[s] != kEmpty) {
    const int i = atomicAdd(cursor, 1);
    skeys[i] = keys[s];
    sunit[i] = slot_unit[s];
  }
}

// one compare-exchange step (k, j) of a bitonic sort of (key, unit) pairs, ascending
__global__ void __launch_bounds__(kThreads) bitonic_step_kernel(uint64_t* skeys, int32_t* sunit, int n, int k, int j) {
  const int i = blockIdx.x * kThreads + threadIdx.x;
  const int l = i ^ j;
  if (i >= n || l <= i) return;
  const uint64_t a = skeys[i], b = skeys[l];
  const bool asc = (i & k) == 0;
  if (asc ? a > b : a < b) {
    skeys[i] = b;
    skeys[l] = a;
    const int t = sunit[i];
    sunit[i] = sunit[l];
    sunit[l] = t;
  }
}

struct Extract {          // carved from the extraction scratch
  uint64_t* skeys;        // [sortn] unit keys, ascending after the sort
  int32_t* sunit;         // [sortn] their pool indices
  int32_t* rank;          // [pool_capacity] sorted rank of a pool unit
  int32_t* nb;            // [cap * 27] pool index of the 3x3x3 neighbours of rank i (-1: none)
  int32_t* cnt_v;         // [cap + 1] vertices per rank, then their exclusive scan
  int32_t* cnt_t;         // [cap + 1] triangles per rank, likewise
  int32_t* sums;          // [scan_blocks(cap) + 1]
  int32_t* cursor;        // [1]
  uint32_t* vinfo;        // [pool_capacity * 4096] (vertex offset in the unit << 3) | mask of active x/y/z edges
};
inline int sort_len(int cap) { int n = 1; while (n < cap) n <<= 1; return n; }
inline Extract carve_extract(void* scratch, int cap, int pool_capacity) {
  char* p = (char*)scratch;
  Extract e;
  const size_t sn = (size_t)sort_len(cap);
  e.skeys = (uint64_t*)p; p += align_up(sn * 8);
  e.sunit = (int32_t*)p; p += align_up(sn * 4);
  e.rank = (int32_t*)p; p += align_up((size_t)pool_capacity * 4);
  e.nb = (int32_t*)p; p += align_up((size_t)cap * kNb * 4);
  e.cnt_v = (int32_t*)p; p += align_up(((size_t)cap + 1) * 4);
  e.cnt_t = (int32_t*)p; p += align_up(((size_t)cap + 1) * 4);
  e.sums = (int32_t*)p; p += align_up(((size_t)scan_blocks(cap) + 1) * 4);
  e.cursor = (int32_t*)p; p += 256;
  e.vinfo = (uint32_t*)p; p += align_up((size_t)pool_capacity * kUnitVox * 4);
  return e;
}
inline size_t extract_bytes(int cap, int pool_capacity) {
  Extract e = carve_extract(nullptr, cap, pool_capacity);
  return (size_t)((char*)e.vinfo - (char*)nullptr) + align_up((size_t)pool_capacity * kUnitVox * 4);
}

// voxel (x, y, z) in [-1, 17) of the unit whose neighbours are nb: pool unit (-1: none) and voxel index
__device__ inline int locate(const int* nb, int x, int y, int z, int& vi) {
  const int ox = x < 0 ? -1 : (x >= kUnitRes ? 1 : 0), oy = y < 0 ? -1 : (y >= kUnitRes ? 1 : 0),
            oz = z < 0 ? -1 : (z >= kUnitRes ? 1 : 0);
  vi = (x - ox * kUnitRes) + kUnitRes * ((y - oy * kUnitRes) + kUnitRes * (z - oz * kUnitRes));
  return nb[(ox + 1) + 3 * (oy + 1) + 9 * (oz + 1)];
}
__device__ inline float weight_at(const float* pool, const int* nb, int x, int y, int z) {
  int vi;
  const int u = locate(nb, x, y, z, vi);
  return u < 0 ? 0.f : pool[(size_t)u * SGR_TSDF_UNIT_FLOATS + kUnitVox + vi];
}
__device__ inline float tsdf_at(const float* pool, const int* nb, int x, int y, int z) {
  int vi;
  const int u = locate(nb, x, y, z, vi);
  return u < 0 ? 0.f : pool[(size_t)u * SGR_TSDF_UNIT_FLOATS + vi];
}
// the case index of the cube at (x, y, z), or -1 where a corner has weight 0 / no unit
__device__ inline int cube_case(const float* pool, const int* nb, int x, int y, int z) {
  int ci = 0;
  for (int c = 0; c < 8; ++c) {
    const int cx = x + mc::kCorner[c][0], cy = y + mc::kCorner[c][1], cz = z + mc::kCorner[c][2];
    if (!(weight_at(pool, nb, cx, cy, cz) > 0.f)) return -1;
    if (tsdf_at(pool, nb, cx, cy, cz) < 0.f) ci |= 1 << c;
  }
  return ci;
}
// active edges of voxel (x, y, z): bit d = its +d edge changes sign and a cube next to it is valid
__device__ inline int edge_mask(const float* pool, const int* nb, int x, int y, int z) {
  if (!(weight_at(pool, nb, x, y, z) > 0.f)) return 0;
  const bool in0 = tsdf_at(pool, nb, x, y, z) < 0.f;
  int m = 0;
  for (int d = 0; d < 3; ++d) {
    const int qx = x + (d == 0), qy = y + (d == 1), qz = z + (d == 2);
    if (!(weight_at(pool, nb, qx, qy, qz) > 0.f) || (tsdf_at(pool, nb, qx, qy, qz) < 0.f) == in0) continue;
    const int a = d == 0 ? 1 : 0, b = d == 2 ? 1 : 2;      // the two axes across the edge
    bool any = false;
    for (int c = 0; c < 4 && !any; ++c) {
      int o[3] = {0, 0, 0};
      o[a] = -(c & 1);
      o[b] = -(c >> 1);
      any = cube_case(pool, nb, x + o[0], y + o[1], z + o[2]) >= 0;
    }
    if (any) m |= 1 << d;
  }
  return m;
}

__device__ inline void load_neighbours(const uint64_t* keys, const int32_t* slot_unit, uint32_t mask, uint64_t key, int* nb) {
  if (threadIdx.x < kNb) {
    int x, y, z;
    unpack_key(key, x, y, z);
    const int t = threadIdx.x;
    const int nx = x + t % 3 - 1, ny = y + (t / 3) % 3 - 1, nz = z + t / 9 - 1;
    int u = -1;
    if (key_in_range(nx, ny, nz)) {
      const int h = hash_find(keys, mask, pack_key(nx, ny, nz));
      u = h >= 0 ? slot_unit[h] : -1;
    }
    nb[t] = u;
  }
}

// count pass: workgroup = unit (rank i), thread = one x-row of 16 voxels (y = t % 16, z = t / 16)
__global__ void __launch_bounds__(kThreads) mc_count_kernel(const uint64_t* keys, const int32_t* slot_unit, uint32_t mask,
                                                            const float* pool, Extract e) {
  __shared__ int nb[kNb];
  __shared__ uint32_t red[kThreads / 64];
  const int i = blockIdx.x;
  load_neighbours(keys, slot_unit, mask, e.skeys[i], nb);
  __syncthreads();
  if (threadIdx.x < kNb) e.nb[(size_t)i * kNb + threadIdx.x] = nb[threadIdx.x];
  if (threadIdx.x == 0) e.rank[nb[13]] = i;
  const int y = threadIdx.x & 15, z = threadIdx.x >> 4;
  int masks[kUnitRes];
  int nv = 0, nt = 0;
  for (int x = 0; x < kUnitRes; ++x) {
    masks[x] = edge_mask(pool, nb, x, y, z);
    nv += __popc(masks[x]);
    const int ci = cube_case(pool, nb, x, y, z);
    nt += ci < 0 ? 0 : mc::kNumTris[ci];
  }
  uint32_t tv, tt;
  int off = (int)block_exclusive_scan<kThreads / 64>((uint32_t)nv, red, tv);
  block_exclusive_scan<kThreads / 64>((uint32_t)nt, red, tt);
  uint32_t* vinfo = e.vinfo + (size_t)nb[13] * kUnitVox + kUnitRes * threadIdx.x;
  for (int x = 0; x < kUnitRes; ++x) {
    vinfo[x] = ((uint32_t)off << 3) | (uint32_t)masks[x];
    off += __popc(masks[x]);
  }
  if (threadIdx.x == 0) {
    e.cnt_v[i] = (int32_t)tv;
    e.cnt_t[i] = (int32_t)tt;
  }
}

// emit pass: the same walk; vertices at (unit base + offset in the unit + rank of the edge), triangles likewise
__global__ void __launch_bounds__(kThreads) mc_emit_kernel(const float* pool, float voxel_len, Extract e, float* __restrict__ verts,
                                                           float* __restrict__ colors, int32_t* __restrict__ tris) {
  __shared__ int nb[kNb];
  __shared__ uint32_t red[kThreads / 64];
  const int i = blockIdx.x;
  if (threadIdx.x < kNb) nb[threadIdx.x] = e.nb[(size_t)i * kNb + threadIdx.x];
  __syncthreads();
  int kx, ky, kz;
  unpack_key(e.skeys[i], kx, ky, kz);
  const int y = threadIdx.x & 15, z = threadIdx.x >> 4;
  const uint32_t* vinfo = e.vinfo + (size_t)nb[13] * kUnitVox + kUnitRes * threadIdx.x;
  const int vbase = e.cnt_v[i];
  // vertices
  for (int x = 0; x < kUnitRes; ++x) {
    const uint32_t info = vinfo[x];
    if (!(info & 7u)) continue;
    int vi;
    const int u0 = locate(nb, x, y, z, vi);
    const float* U0 = pool + (size_t)u0 * SGR_TSDF_UNIT_FLOATS;
    const float f0 = U0[vi];
    int id = vbase + (int)(info >> 3);
    for (int d = 0; d < 3; ++d) {
      if (!((info >> d) & 1u)) continue;
      int vj;
      const int u1 = locate(nb, x + (d == 0), y + (d == 1), z + (d == 2), vj);
      const float* U1 = pool + (size_t)u1 * SGR_TSDF_UNIT_FLOATS;
      const float f1 = U1[vj];
      const float t = fabsf(f0) / (fabsf(f0) + fabsf(f1));
      float p[3] = {((float)(kx * kUnitRes + x) + kVoxelCentre) * voxel_len, ((float)(ky * kUnitRes + y) + kVoxelCentre) * voxel_len,
                    ((float)(kz * kUnitRes + z) + kVoxelCentre) * voxel_len};
      p[d] = p[d] + t * voxel_len;
      for (int c = 0; c < 3; ++c) {
        const float c0 = U0[(2 + c) * kUnitVox + vi], c1 = U1[(2 + c) * kUnitVox + vj];
        colors[(size_t)id * 3 + c] = (c0 + t * (c1 - c0)) / kColorScale;
        verts[(size_t)id * 3 + c] = p[c];
      }
      ++id;
    }
  }
  // triangles
  int cases[kUnitRes];
  int nt = 0;
  for (int x = 0; x < kUnitRes; ++x) {
    cases[x] = cube_case(pool, nb, x, y, z);
    nt += cases[x] < 0 ? 0 : mc::kNumTris[cases[x]];
  }
  uint32_t tt;
  int tid = e.cnt_t[i] + (int)block_exclusive_scan<kThreads / 64>((uint32_t)nt, red, tt);
  for (int x = 0; x < kUnitRes; ++x) {
    const int ci = cases[x];
    if (ci < 0) continue;
    for (int k = 0; k < 3 * mc::kNumTris[ci]; ++k) {
      const int ed = mc::kTris[ci][k];
      const int a = mc::kEdge[ed][0], b = mc::kEdge[ed][1];
      int d = 0;
      while (mc::kCorner[a][d] == mc::kCorner[b][d]) ++d;
      const int lo = mc::kCorner[a][d] < mc::kCorner[b][d] ? a : b;      // the edge's owner: its lower corner
      int vj;
      const int u = locate(nb, x + mc::kCorner[lo][0], y + mc::kCorner[lo][1], z + mc::kCorner[lo][2], vj);
      const uint32_t info = e.vinfo[(size_t)u * kUnitVox + vj];
      tris[(size_t)tid * 3 + k] = e.cnt_v[e.rank[u]] + (int)(info >> 3) + __popc(info & ((1u << d) - 1u));
    }
    tid += mc::kNumTris[ci];
  }
}

// ---- cleaning
struct Clean {            // carved from the cleaning scratch
  int32_t* label;         // [V]
  int32_t* csize;         // [V] component sizes (at the label)
  int32_t* vnew;          // [V + 1] keep flags, then their exclusive scan
  int32_t* tnew;          // [F + 1] likewise for triangles
  int32_t* bcount;        // [V + 1] kept triangles per smallest vertex, then bucket starts
  int32_t* bfill;         // [V]
  int32_t* bucket;        // [F]
  int32_t* sums;          // [scan_blocks(max(V, F)) + 1]
};
inline Clean carve_clean(void* scratch, int V, int F) {
  char* p = (char*)scratch;
  Clean c;
  c.label = (int32_t*)p; p += align_up((size_t)V * 4);
  c.csize = (int32_t*)p; p += align_up((size_t)V * 4);
  c.vnew = (int32_t*)p; p += align_up(((size_t)V + 1) * 4);
  c.tnew = (int32_t*)p; p += align_up(((size_t)F + 1) * 4);
  c.bcount = (int32_t*)p; p += align_up(((size_t)V + 1) * 4);
  c.bfill = (int32_t*)p; p += align_up((size_t)V * 4);
  c.bucket = (int32_t*)p; p += align_up((size_t)F * 4);
  c.sums = (int32_t*)p;
  return c;
}
inline size_t clean_bytes(int V, int F) {
  Clean c = carve_clean(nullptr, V, F);
  return (size_t)((char*)c.sums - (char*)nullptr) + align_up(((size_t)scan_blocks(V > F ? V : F) + 1) * 4);
}

__device__ inline int find_root(int32_t* label, int x) {
  int p = __hip_atomic_load(&label[x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  while (p != x) {
    x = p;
    p = __hip_atomic_load(&label[x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  return x;
}

__global__ void __launch_bounds__(kThreads) cc_init_kernel(int V, Clean c) {
  const int v = blockIdx.x * kThreads + threadIdx.x;
  if (v < V) {
    c.label[v] = v;
    c.csize[v] = 0;
    c.bcount[v] = 0;
    c.bfill[v] = 0;
  }
}

// union over the three edges of a triangle: the larger root is hooked below the smaller one (CAS), so a root is always the
// smallest id of its tree and the final labels do not depend on the order of the races
__global__ void __launch_bounds__(kThreads) cc_union_kernel(int F, const int32_t* tris, Clean c) {
  const int t = blockIdx.x * kThreads + threadIdx.x;
  if (t >= F) return;
  for (int k = 0; k < 3; ++k) {
    int a = tris[(size_t)t * 3 + k], b = tris[(size_t)t * 3 + (k + 1) % 3];
    while (true) {
      a = find_root(c.label, a);
      b = find_root(c.label, b);
      if (a == b) break;
      if (a < b) { const int s = a; a = b; b = s; }
      const int old = atomicCAS(&c.label[a], a, b);
      if (old == a) break;
      a = old;
    }
  }
}

__global__ void __launch_bounds__(kThreads) cc_flatten_kernel(int V, Clean c) {
  const int v = blockIdx.x * kThreads + threadIdx.x;
  if (v < V) {
    const int r = find_root(c.label, v);
    c.label[v] = r;
    atomicAdd(&c.csize[r], 1);
  }
}

__global__ void __launch_bounds__(kThreads) cc_keep_vertices_kernel(int V, int min_len, Clean c) {
  const int v = blockIdx.x * kThreads + threadIdx.x;
  if (v < V) c.vnew[v] = c.csize[c.label[v]] >= min_len ? 1 : 0;
}

// a triangle stays if its component does and it is not degenerate (repeated index, zero area); kept ones go to the bucket of their
// smallest vertex for the duplicate test
__global__ void __launch_bounds__(kThreads) tri_keep_kernel(int F, const int32_t* tris, const float* verts, int min_len, Clean c) {
  const int t = blockIdx.x * kThreads + threadIdx.x;
  if (t >= F) return;
  const int a = tris[(size_t)t * 3], b = tris[(size_t)t * 3 + 1], d = tris[(size_t)t * 3 + 2];
  bool keep = c.csize[c.label[a]] >= min_len && a != b && b != d && a != d;
  if (keep) {
    // every product is rounded on its own: with e1 == e2, or e2 a power of two times e1, the two products of a component are then
    // the same float and the face is dropped, where an fma would leave the rounding residual of one product
#pragma clang fp contract(off)
    float e1[3], e2[3];
    for (int k = 0; k < 3; ++k) {
      e1[k] = verts[(size_t)b * 3 + k] - verts[(size_t)a * 3 + k];
      e2[k] = verts[(size_t)d * 3 + k] - verts[(size_t)a * 3 + k];
    }
    const float nx = e1[1] * e2[2] - e1[2] * e2[1], ny = e1[2] * e2[0] - e1[0] * e2[2], nz = e1[0] * e2[1] - e1[1] * e2[0];
    keep = nx != 0.f || ny != 0.f || nz != 0.f;
  }
  c.tnew[t] = keep ? 1 : 0;
  if (keep) atomicAdd(&c.bcount[min(a, min(b, d))], 1);
}

__device__ inline void sort3(int& a, int& b, int& c) {
  if (a > b) { const int s = a; a = b; b = s; }
  if (b > c) { const int s = b; b = c; c = s; }
  if (a > b) { const int s = a; a = b; b = s; }
}

__global__ void __launch_bounds__(kThreads) tri_bucket_kernel(int F, const int32_t* tris, Clean c) {
  const int t = blockIdx.x * kThreads + threadIdx.x;
  if (t >= F || !c.tnew[t]) return;
  int a = tris[(size_t)t * 3], b = tris[(size_t)t * 3 + 1], d = tris[(size_t)t * 3 + 2];
  sort3(a, b, d);
  c.bucket[c.bcount[a] + atomicAdd(&c.bfill[a], 1)] = t;
}

// a kept triangle with the vertex set of a kept triangle of smaller index is dropped (the bucket's order does not matter)
__global__ void __launch_bounds__(kThreads) tri_dedup_kernel(int F, const int32_t* tris, Clean c) {
  const int t = blockIdx.x * kThreads + threadIdx.x;
  if (t >= F || !c.tnew[t]) return;
  int a = tris[(size_t)t * 3], b = tris[(size_t)t * 3 + 1], d = tris[(size_t)t * 3 + 2];
  sort3(a, b, d);
  const int s0 = c.bcount[a], s1 = c.bcount[a + 1];
  for (int s = s0; s < s1; ++s) {
    const int o = c.bucket[s];
    if (o >= t) continue;
    int oa = tris[(size_t)o * 3], ob = tris[(size_t)o * 3 + 1], od = tris[(size_t)o * 3 + 2];
    sort3(oa, ob, od);
    if (oa == a && ob == b && od == d) {
      c.tnew[t] = 0;      // read by nobody else in this launch: the buckets hold the kept set
      return;
    }
  }
}

bool volume_ok(const SgrTsdfVolume* v) {
  return v && v->state && v->pool && v->hash_capacity >= 64 && (v->hash_capacity & (v->hash_capacity - 1)) == 0 &&
         v->pool_capacity > 0 && v->voxel_length > 0.f && v->sdf_trunc > 0.f && v->depth_trunc > 0.f;
}

// rows 0..2 of w2c and of its inverse (any invertible 4x4 whose last row is 0 0 0 1), inverted in double
bool frame_tab(int n, const SgrTsdfFrame* frames, FrameTab& tab) {
  tab = {};
  for (int i = 0; i < n; ++i) {
    const SgrTsdfFrame& s = frames[i];
    if (!s.render || !s.depth || !(s.fx != 0.f) || !(s.fy != 0.f)) return false;
    FrameDev& f = tab.f[i];
    f.render = s.render;
    f.depth = s.depth;
    f.gt_depth = s.gt_depth;
    f.ea = s.exposure_a;
    f.eb = s.exposure_b;
    f.fx = s.fx; f.fy = s.fy; f.cx = s.cx; f.cy = s.cy; f.scale = s.global_scale;
    double m[3][3], t[3];
    for (int r = 0; r < 3; ++r) {
      for (int c = 0; c < 3; ++c) m[r][c] = s.w2c[4 * r + c];
      t[r] = s.w2c[4 * r + 3];
    }
    const double det = m[0][0] * (m[1][1] * m[2][2] - m[1][2] * m[2][1]) - m[0][1] * (m[1][0] * m[2][2] - m[1][2] * m[2][0]) +
                       m[0][2] * (m[1][0] * m[2][1] - m[1][1] * m[2][0]);
    if (!(det != 0.0) || !std::isfinite(det)) return false;
    double inv[3][3];
    for (int r = 0; r < 3; ++r)
      for (int c = 0; c < 3; ++c) {
        const int r1 = (c + 1) % 3, r2 = (c + 2) % 3, c1 = (r + 1) % 3, c2 = (r + 2) % 3;
        inv[r][c] = (m[r1][c1] * m[r2][c2] - m[r1][c2] * m[r2][c1]) / det;
      }
    for (int r = 0; r < 3; ++r) {
      for (int c = 0; c < 4; ++c) f.w2c[4 * r + c] = s.w2c[4 * r + c];
      double tt = 0.0;
      for (int c = 0; c < 3; ++c) {
        f.c2w[4 * r + c] = (float)inv[r][c];
        tt -= inv[r][c] * t[c];
      }
      f.c2w[4 * r + 3] = (float)tt;
    }
  }
  return true;
}

}  // namespace
}  // namespace sgr

using namespace sgr;

extern "C" {

size_t sgr_tsdf_bytes(int32_t hash_capacity) {
  if (hash_capacity <= 0) return 0;
  const size_t cap = (size_t)hash_capacity;
  return align_up(cap * 8) + 3 * align_up(cap * 4) + align_up(kStateCounters * 4);
}

int sgr_tsdf_reset(const SgrTsdfVolume* vol, void* stream) {
  if (!volume_ok(vol)) return set_error(SGR_ERR_INVALID, "tsdf_reset: bad volume");
  hipStream_t st = (hipStream_t)stream;
  State s = carve_state(vol);
  const size_t cap = (size_t)vol->hash_capacity;
  if (hipMemsetAsync(s.keys, 0xff, cap * 8, st) != hipSuccess ||
      hipMemsetAsync(s.marks, 0, cap * 4, st) != hipSuccess ||
      hipMemsetAsync(s.counters, 0, kStateCounters * 4, st) != hipSuccess ||
      hipMemsetAsync(vol->pool, 0, (size_t)vol->pool_capacity * SGR_TSDF_UNIT_FLOATS * 4, st) != hipSuccess)
    return set_error(SGR_ERR_HIP, "tsdf_reset: memset failed");
  return SGR_OK;
}

int sgr_tsdf_rehash(const SgrTsdfVolume* src, const SgrTsdfVolume* dst, void* stream) {
  if (!volume_ok(src) || !volume_ok(dst) || dst->hash_capacity < src->hash_capacity)
    return set_error(SGR_ERR_INVALID, "tsdf_rehash: bad volumes");
  hipStream_t st = (hipStream_t)stream;
  State a = carve_state(src), b = carve_state(dst);
  if (hipMemcpyAsync(b.counters, a.counters, sizeof(int32_t), hipMemcpyDeviceToDevice, st) != hipSuccess)
    return set_error(SGR_ERR_HIP, "tsdf_rehash: copy failed");
  hipLaunchKernelGGL(tsdf_rehash_kernel, dim3(blocks_for(src->hash_capacity)), dim3(kThreads), 0, st, (const uint64_t*)a.keys,
                     (const int32_t*)a.slot_unit, src->hash_capacity, b.keys, b.slot_unit, b.counters,
                     (uint32_t)dst->hash_capacity - 1u);
  return hipGetLastError() == hipSuccess ? SGR_OK : set_error(SGR_ERR_HIP, "tsdf_rehash launch failed");
}

int sgr_tsdf_touch(const SgrTsdfVolume* vol, int32_t n, const SgrTsdfFrame* frames, int32_t H, int32_t W, void* stream) {
  if (!volume_ok(vol) || n <= 0 || n > SGR_TSDF_MAX_FRAMES || !frames || H <= 0 || W <= 0)
    return set_error(SGR_ERR_INVALID, "tsdf_touch: bad arguments");
  FrameTab tab;
  if (!frame_tab(n, frames, tab)) return set_error(SGR_ERR_INVALID, "tsdf_touch: a frame has no image / bad intrinsics or pose");
  hipStream_t st = (hipStream_t)stream;
  State s = carve_state(vol);
  if (hipMemsetAsync(s.counters + 2, 0, sizeof(int32_t), st) != hipSuccess) return set_error(SGR_ERR_HIP, "tsdf_touch: memset");
  const long long pts = (long long)((W + kTouchStride - 1) / kTouchStride) * ((H + kTouchStride - 1) / kTouchStride);
  hipLaunchKernelGGL(tsdf_touch_kernel, dim3(blocks_for(pts), n), dim3(kThreads), 0, st, tab, H, W, vol->voxel_length * kUnitRes,
                     vol->sdf_trunc, vol->depth_trunc, s.keys, s.slot_unit, s.marks, s.counters, (uint32_t)vol->hash_capacity - 1u);
  hipLaunchKernelGGL(tsdf_list_kernel, dim3(blocks_for(vol->hash_capacity)), dim3(kThreads), 0, st, (const uint32_t*)s.marks,
                     vol->hash_capacity, s.list, s.counters);
  return hipGetLastError() == hipSuccess ? SGR_OK : set_error(SGR_ERR_HIP, "tsdf_touch launch failed");
}

int sgr_tsdf_integrate(const SgrTsdfVolume* vol, int32_t n, const SgrTsdfFrame* frames, int32_t H, int32_t W, int32_t n_touched,
                       void* stream) {
  if (!volume_ok(vol) || n <= 0 || n > SGR_TSDF_MAX_FRAMES || !frames || H <= 0 || W <= 0 || n_touched < 0 ||
      n_touched > vol->hash_capacity)
    return set_error(SGR_ERR_INVALID, "tsdf_integrate: bad arguments");
  FrameTab tab;
  if (!frame_tab(n, frames, tab)) return set_error(SGR_ERR_INVALID, "tsdf_integrate: a frame has no image / bad intrinsics or pose");
  if (n_touched == 0) return SGR_OK;
  State s = carve_state(vol);
  hipLaunchKernelGGL(tsdf_integrate_kernel, dim3(n_touched), dim3(kThreads), 0, (hipStream_t)stream, tab, n, H, W,
                     vol->voxel_length, vol->sdf_trunc, vol->depth_trunc, (const uint64_t*)s.keys, (const int32_t*)s.slot_unit,
                     s.marks, (const int32_t*)s.list, s.counters, vol->pool, vol->pool_capacity);
  return hipGetLastError() == hipSuccess ? SGR_OK : set_error(SGR_ERR_HIP, "tsdf_integrate launch failed");
}

size_t sgr_tsdf_extract_bytes(int32_t hash_capacity, int32_t pool_capacity) {
  if (hash_capacity <= 0 || pool_capacity <= 0) return 0;
  return extract_bytes(hash_capacity, pool_capacity);
}

int sgr_tsdf_extract_count(const SgrTsdfVolume* vol, int32_t n_units, void* scratch, size_t scratch_bytes, int32_t* totals,
                           void* stream) {
  if (!volume_ok(vol) || n_units < 0 || n_units > vol->pool_capacity || n_units > vol->hash_capacity || !totals)
    return set_error(SGR_ERR_INVALID, "tsdf_extract_count: bad arguments");
  if (!scratch || scratch_bytes < extract_bytes(vol->hash_capacity, vol->pool_capacity))
    return set_error(SGR_ERR_WORKSPACE, "tsdf_extract_count: scratch too small (need %zu)",
                     extract_bytes(vol->hash_capacity, vol->pool_capacity));
  hipStream_t st = (hipStream_t)stream;
  if (n_units == 0) return hipMemsetAsync(totals, 0, 2 * sizeof(int32_t), st) == hipSuccess ? SGR_OK : set_error(SGR_ERR_HIP, "memset");
  State s = carve_state(vol);
  Extract e = carve_extract(scratch, vol->hash_capacity, vol->pool_capacity);
  const int sn = sort_len(n_units < 2 ? 2 : n_units);
  if (hipMemsetAsync(e.skeys, 0xff, (size_t)sn * 8, st) != hipSuccess || hipMemsetAsync(e.cursor, 0, 4, st) != hipSuccess)
    return set_error(SGR_ERR_HIP, "tsdf_extract_count: memset");
  hipLaunchKernelGGL(gather_units_kernel, dim3(blocks_for(vol->hash_capacity)), dim3(kThreads), 0, st, (const uint64_t*)s.keys,
                     (const int32_t*)s.slot_unit, vol->hash_capacity, e.skeys, e.sunit, e.cursor);
  for (int k = 2; k <= sn; k <<= 1)
    for (int j = k >> 1; j > 0; j >>= 1)
      hipLaunchKernelGGL(bitonic_step_kernel, dim3(blocks_for(sn)), dim3(kThreads), 0, st, e.skeys, e.sunit, sn, k, j);
  hipLaunchKernelGGL(mc_count_kernel, dim3(n_units), dim3(kThreads), 0, st, (const uint64_t*)s.keys, (const int32_t*)s.slot_unit,
                     (uint32_t)vol->hash_capacity - 1u, (const float*)vol->pool, e);
  scan_exclusive(e.cnt_v, n_units, e.sums, st);
  scan_exclusive(e.cnt_t, n_units, e.sums, st);
  if (hipMemcpyAsync(totals, e.cnt_v + n_units, 4, hipMemcpyDeviceToDevice, st) != hipSuccess ||
      hipMemcpyAsync(totals + 1, e.cnt_t + n_units, 4, hipMemcpyDeviceToDevice, st) != hipSuccess)
    return set_error(SGR_ERR_HIP, "tsdf_extract_count: copy");
  return hipGetLastError() == hipSuccess ? SGR_OK : set_error(SGR_ERR_HIP, "tsdf_extract_count launch failed");
}

int sgr_tsdf_extract(const SgrTsdfVolume* vol, int32_t n_units, void* scratch, size_t scratch_bytes, float* vertices,
                     float* colors, int32_t* triangles, void* stream) {
  if (!volume_ok(vol) || n_units < 0 || n_units > vol->pool_capacity || n_units > vol->hash_capacity)
    return set_error(SGR_ERR_INVALID, "tsdf_extract: bad arguments");
  if (!scratch || scratch_bytes < extract_bytes(vol->hash_capacity, vol->pool_capacity))
    return set_error(SGR_ERR_WORKSPACE, "tsdf_extract: scratch too small");
  if (n_units == 0) return SGR_OK;
  if (!vertices || !colors || !triangles) return set_error(SGR_ERR_INVALID, "tsdf_extract: null output");
  Extract e = carve_extract(scratch, vol->hash_capacity, vol->pool_capacity);
  hipLaunchKernelGGL(mc_emit_kernel, dim3(n_units), dim3(kThreads), 0, (hipStream_t)stream, (const float*)vol->pool,
                     vol->voxel_length, e, vertices, colors, triangles);
  return hipGetLastError() == hipSuccess ? SGR_OK : set_error(SGR_ERR_HIP, "tsdf_extract launch failed");
}

size_t sgr_mesh_bytes(int32_t V, int32_t F) {
  if (V < 0 || F < 0) return 0;
  return clean_bytes(V, F);
}

int sgr_mesh_components(int32_t V, int32_t F, const float* vertices, const int32_t* triangles, int32_t min_len, void* scratch,
                        size_t scratch_bytes, int32_t* totals, void* stream) {
  if (V < 0 || F < 0 || min_len < 1 || !totals || (V > 0 && !vertices) || (F > 0 && !triangles))
    return set_error(SGR_ERR_INVALID, "mesh_components: bad arguments");
  if (!scratch || scratch_bytes < clean_bytes(V, F)) return set_error(SGR_ERR_WORKSPACE, "mesh_components: scratch too small");
  hipStream_t st = (hipStream_t)stream;
  Clean c = carve_clean(scratch, V, F);
  const int vb = std::max(1, blocks_for(V));      // V == 0: one idle workgroup, not an empty grid
  hipLaunchKernelGGL(cc_init_kernel, dim3(vb), dim3(kThreads), 0, st, V, c);
  if (F > 0) hipLaunchKernelGGL(cc_union_kernel, dim3(blocks_for(F)), dim3(kThreads), 0, st, F, triangles, c);
  hipLaunchKernelGGL(cc_flatten_kernel, dim3(vb), dim3(kThreads), 0, st, V, c);
  hipLaunchKernelGGL(cc_keep_vertices_kernel, dim3(vb), dim3(kThreads), 0, st, V, min_len, c);
  scan_exclusive(c.vnew, V, c.sums, st);
  if (F > 0) {
    hipLaunchKernelGGL(tri_keep_kernel, dim3(blocks_for(F)), dim3(kThreads), 0, st, F, triangles, vertices, min_len, c);
    scan_exclusive(c.bcount, V, c.sums, st);
    hipLaunchKernelGGL(tri_bucket_kernel, dim3(blocks_for(F)), dim3(kThreads), 0, st, F, triangles, c);
    hipLaunchKernelGGL(tri_dedup_kernel, dim3(blocks_for(F)), dim3(kThreads), 0, st, F, triangles, c);
  }
  scan_exclusive(c.tnew, F, c.sums, st);
  if (hipMemcpyAsync(totals, c.vnew + V, 4, hipMemcpyDeviceToDevice, st) != hipSuccess ||
      hipMemcpyAsync(totals + 1, c.tnew + F, 4, hipMemcpyDeviceToDevice, st) != hipSuccess)
    return set_error(SGR_ERR_HIP, "mesh_components: copy");
  return hipGetLastError() == hipSuccess ? SGR_OK : set_error(SGR_ERR_HIP, "mesh_components launch failed");
}

int sgr_mesh_compact(int32_t V, int32_t F, const float* vertices, const float* colors, const int32_t* triangles, void* scratch,
                     size_t scratch_bytes, float* out_vertices, float* out_colors, int32_t* out_triangles, int32_t* vertex_map,
                     void* stream) {
  if (V < 0 || F < 0 || (V > 0 && (!vertices || !colors)) || (F > 0 && !triangles))
    return set_error(SGR_ERR_INVALID, "mesh_compact: bad arguments");
  if (!scratch || scratch_bytes < clean_bytes(V, F)) return set_error(SGR_ERR_WORKSPACE, "mesh_compact: scratch too small");
  const Clean c = carve_clean(scratch, V, F);
  launch_mesh_compact(V, F, vertices, colors, triangles, c.vnew, c.tnew, out_vertices, out_colors, out_triangles, vertex_map, (hipStream_t)stream);
  return hipGetLastError() == hipSuccess ? SGR_OK : set_error(SGR_ERR_HIP, "mesh_compact launch failed");
}

}  // extern "C"
