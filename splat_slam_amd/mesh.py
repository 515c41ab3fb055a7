"""TSDF fusion and mesh extraction of eval_rendering's `mesh` branch (/root/reference/src/utils/eval_utils.py:70-74, 142-179) and
its clean_mesh (:331-379), on the HIP kernels of csrc/sgr_mesh.hip.  The reference uses Open3D's ScalableTSDFVolume (RGB8) and
trimesh; the conventions reproduced here are assumptions about those libraries, listed in DESIGN.md section 3.

GPU tensors only: there is no CPU path."""
import numpy as np
import torch

from splat_slam_amd import _native as nat


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _need_gpu(*tensors):
    for t in tensors:
        if t is not None and (not torch.is_tensor(t) or t.device.type != "cuda"):
            raise RuntimeError("splat_slam_amd.mesh needs GPU tensors (HIP only, no CPU fallback)")


class TriangleMesh:
    """vertices f32 [V,3], triangles i32 [F,3], vertex_colors f32 [V,3] in 0..1 (float; not quantised to k/255)."""

    def __init__(self, vertices, triangles, vertex_colors):
        self.vertices, self.triangles, self.vertex_colors = vertices, triangles, vertex_colors

    def __len__(self):
        return int(self.vertices.shape[0])

    def write_ply(self, path):
        """binary little-endian PLY: float x, y, z, uchar red, green, blue; faces as uchar-counted int lists"""
        v = self.vertices.detach().cpu().numpy().astype("<f4").reshape(-1, 3)
        c = np.clip(np.round(self.vertex_colors.detach().cpu().numpy().astype(np.float64) * 255.0), 0, 255).astype(np.uint8).reshape(-1, 3)
        f = self.triangles.detach().cpu().numpy().astype("<i4").reshape(-1, 3)
        head = ("ply\nformat binary_little_endian 1.0\nelement vertex %d\nproperty float x\nproperty float y\nproperty float z\n"
                "property uchar red\nproperty uchar green\nproperty uchar blue\nelement face %d\n"
                "property list uchar int vertex_indices\nend_header\n") % (len(v), len(f))
        vrec = np.zeros(len(v), dtype=[("p", "<f4", 3), ("c", "u1", 3)])
        vrec["p"], vrec["c"] = v, c
        frec = np.zeros(len(f), dtype=[("n", "u1"), ("i", "<i4", 3)])
        frec["n"], frec["i"] = 3, f
        with open(path, "wb") as fh:
            fh.write(head.encode("ascii"))
            fh.write(vrec.tobytes())
            fh.write(frec.tobytes())

    @staticmethod
    def read_ply(path):
        """reads what write_ply writes (CPU tensors; colours as uchar / 255)"""
        with open(path, "rb") as fh:
            data = fh.read()
        end = data.index(b"end_header\n") + len(b"end_header\n")
        head = data[:end].decode("ascii").split("\n")
        if "format binary_little_endian 1.0" not in head:
            raise ValueError(f"{path}: not a binary little-endian PLY")
        nv = nf = 0
        for line in head:
            if line.startswith("element vertex"):
                nv = int(line.split()[2])
            elif line.startswith("element face"):
                nf = int(line.split()[2])
        vrec = np.frombuffer(data, dtype=[("p", "<f4", 3), ("c", "u1", 3)], count=nv, offset=end)
        frec = np.frombuffer(data, dtype=[("n", "u1"), ("i", "<i4", 3)], count=nf, offset=end + vrec.nbytes)
        if nf and not (frec["n"] == 3).all():
            raise ValueError(f"{path}: faces that are not triangles")
        return TriangleMesh(torch.from_numpy(vrec["p"].copy()), torch.from_numpy(frec["i"].copy()),
                            torch.from_numpy(vrec["c"].astype(np.float32) / 255.0))


def _w2c_rows(w2c):
    m = torch.as_tensor(w2c).detach().double().cpu().reshape(4, 4)
    return (nat.C.c_float * 16)(*[float(x) for x in m.reshape(-1)])


class TSDFVolume:
    """ScalableTSDFVolume(voxel_length, sdf_trunc, RGB8) on the device: units of 16^3 voxels in a hash, a pool that grows."""

    def __init__(self, voxel_length=5.0 / 512.0, sdf_trunc=0.04, depth_trunc=30.0, device="cuda", hash_capacity=1 << 16,
                 pool_capacity=256):
        if not str(device).startswith("cuda"):
            raise RuntimeError("TSDFVolume needs a GPU device (HIP only, no CPU fallback)")
        if not (voxel_length > 0 and sdf_trunc > 0 and depth_trunc > 0):
            raise ValueError("TSDFVolume: voxel_length, sdf_trunc and depth_trunc must be > 0")
        self.voxel_length, self.sdf_trunc, self.depth_trunc = float(voxel_length), float(sdf_trunc), float(depth_trunc)
        self.device = torch.device(device)
        self._lib = nat.lib()
        cap = 64
        while cap < hash_capacity:
            cap *= 2
        self._alloc(cap, max(1, int(pool_capacity)))
        self.reset()

    @classmethod
    def from_voxels(cls, vox, voxel_length, sdf_trunc, depth_trunc=30.0, device="cuda", hash_capacity=None, pool_capacity=None):
        """the inverse of voxels(): a volume that holds exactly the units of vox (keys int64 [n,3], tsdf / weight [n,4096], color
        [n,4096,3] on 0..255; numpy or torch, any device), in a hash of at least 2 n slots and a pool of at least n units.  The keys
        go into the first n slots of a source state and sgr_tsdf_rehash inserts them: no kernel of its own."""
        get = lambda name: torch.as_tensor(vox[name]).detach()
        keys, tsdf, weight, color = get("keys").cpu(), get("tsdf"), get("weight"), get("color")
        if keys.dim() != 2 or keys.shape[1] != 3 or keys.dtype != torch.int64:
            raise ValueError(f"TSDFVolume.from_voxels: keys must be int64 [n,3], got {tuple(keys.shape)} {keys.dtype}")
        n = keys.shape[0]
        if tuple(tsdf.shape) != (n, 4096) or tuple(weight.shape) != (n, 4096) or tuple(color.shape) != (n, 4096, 3):
            raise ValueError(f"TSDFVolume.from_voxels: tsdf / weight must be [{n},4096] and color [{n},4096,3], got "
                             f"{tuple(tsdf.shape)}, {tuple(weight.shape)}, {tuple(color.shape)}")
        bias = 1 << 20
        if n and (int(keys.min()) < -bias or int(keys.max()) >= bias):
            raise ValueError("TSDFVolume.from_voxels: unit keys outside [-2^20, 2^20)")
        packed = ((keys[:, 0] + bias) << 42) | ((keys[:, 1] + bias) << 21) | (keys[:, 2] + bias)
        if torch.unique(packed).numel() != n:
            raise ValueError("TSDFVolume.from_voxels: duplicate unit keys")
        vol = cls(voxel_length, sdf_trunc, depth_trunc, device, max(int(hash_capacity or 0), 2 * n),
                  max(int(pool_capacity or 0), n, 1))
        if n == 0:
            return vol
        src_cap = 64
        while src_cap < n:
            src_cap *= 2
        src = torch.zeros(vol._lib.sgr_tsdf_bytes(src_cap), dtype=torch.uint8, device=vol.device)
        src[:src_cap * 8].fill_(0xFF)
        src[:n * 8].view(torch.int64).copy_(packed)
        src[src_cap * 8:src_cap * 8 + n * 4].view(torch.int32).copy_(torch.arange(n, dtype=torch.int32))
        src[20 * src_cap:20 * src_cap + 4].view(torch.int32).fill_(n)
        pool = vol._pool.view(-1, 5, 4096)
        pool[:n, 0].copy_(tsdf.float())
        pool[:n, 1].copy_(weight.float())
        pool[:n, 2:5].copy_(color.float().permute(0, 2, 1))
        nat.check(vol._lib.sgr_tsdf_rehash(vol._vol(state=src, cap=src_cap), vol._vol(), _stream()), "sgr_tsdf_rehash")
        vol.num_units = n
        return vol

    # ---- state
    def _alloc(self, cap, pool_cap):
        self.hash_capacity, self.pool_capacity = cap, pool_cap
        self._state = torch.empty(self._lib.sgr_tsdf_bytes(cap), dtype=torch.uint8, device=self.device)
        self._pool = torch.empty(pool_cap * nat.SGR_TSDF_UNIT_FLOATS, dtype=torch.float32, device=self.device)

    def _vol(self, state=None, pool=None, cap=None, pool_cap=None):
        state = self._state if state is None else state
        pool = self._pool if pool is None else pool
        return nat.SgrTsdfVolume(self.voxel_length, self.sdf_trunc, self.depth_trunc, cap or self.hash_capacity,
                                 pool_cap or self.pool_capacity, state.data_ptr(), pool.data_ptr())

    # the state's layout (csrc/sgr_mesh.hip carve_state; hash_capacity >= 64 keeps every part 256-byte aligned):
    # keys u64 [cap], slot units i32 [cap], marks u32 [cap], touched list i32 [cap], counters i32 [8]
    def _counters(self):
        return self._state[20 * self.hash_capacity:20 * self.hash_capacity + 32].view(torch.int32)

    def reset(self):
        v = self._vol()
        nat.check(self._lib.sgr_tsdf_reset(v, _stream()), "sgr_tsdf_reset")
        self.num_units = 0

    def _rehash(self, cap):
        state = torch.empty(self._lib.sgr_tsdf_bytes(cap), dtype=torch.uint8, device=self.device)
        dst = self._vol(state=state, cap=cap)
        src = self._vol()
        state.fill_(0)                                      # a fresh hash: empty keys, zero marks and counters (the pool stays)
        state[:cap * 8].fill_(0xFF)
        nat.check(self._lib.sgr_tsdf_rehash(src, dst, _stream()), "sgr_tsdf_rehash")
        self._state, self.hash_capacity = state, cap

    def _grow_pool(self, need):
        cap = max(need + need // 4, 2 * self.pool_capacity)
        pool = torch.zeros(cap * nat.SGR_TSDF_UNIT_FLOATS, dtype=torch.float32, device=self.device)
        pool[:self._pool.numel()].copy_(self._pool)
        self._pool, self.pool_capacity = pool, cap

    # ---- integration
    def _frame(self, render, depth, w2c, fx, fy, cx, cy, gt_depth, exposure_a, exposure_b, global_scale, keep):
        _need_gpu(render, depth, gt_depth, exposure_a, exposure_b)
        if render.dtype != torch.float32 or render.dim() != 3 or render.shape[0] != 3:
            raise ValueError(f"TSDFVolume: render must be fp32 [3,H,W], got {tuple(render.shape)} {render.dtype}")
        H, W = render.shape[1:]
        r = render.detach().contiguous()
        d = depth.detach().float().reshape(-1).contiguous()
        if d.numel() != H * W:
            raise ValueError(f"TSDFVolume: depth has {d.numel()} values for a {H}x{W} image")
        g = None
        if gt_depth is not None:
            g = gt_depth.detach().float().reshape(-1).contiguous()
            if g.numel() != H * W:
                raise ValueError(f"TSDFVolume: gt_depth has {g.numel()} values for a {H}x{W} image")
        a = None if exposure_a is None else exposure_a.detach().float().reshape(-1)[:1].contiguous()
        b = None if exposure_b is None else exposure_b.detach().float().reshape(-1)[:1].contiguous()
        keep += [r, d, g, a, b]
        return (H, W), nat.SgrTsdfFrame(r.data_ptr(), d.data_ptr(), nat.ptr(g), nat.ptr(a), nat.ptr(b), float(fx), float(fy),
                                        float(cx), float(cy), _w2c_rows(w2c), float(global_scale))

    def integrate(self, render, depth, w2c, fx, fy, cx, cy, gt_depth=None, exposure_a=None, exposure_b=None, global_scale=1.0):
        """one frame: render [3,H,W] (colour = clamp(exp(a) render + b, 0, 1), truncated to 0..255), depth [H,W] or [1,H,W]
        (times global_scale, dropped where gt_depth == 0 and beyond depth_trunc), w2c [4,4] world -> camera"""
        self.integrate_frames([dict(render=render, depth=depth, w2c=w2c, fx=fx, fy=fy, cx=cx, cy=cy, gt_depth=gt_depth,
                                    exposure_a=exposure_a, exposure_b=exposure_b, global_scale=global_scale)])

    def integrate_frames(self, frames):
        """frames in order: dicts with the arguments of integrate.  One host synchronisation per 16 frames."""
        for c0 in range(0, len(frames), nat.SGR_TSDF_MAX_FRAMES):
            keep, table, size = [], [], None
            for fr in frames[c0:c0 + nat.SGR_TSDF_MAX_FRAMES]:
                hw, f = self._frame(fr["render"], fr["depth"], fr["w2c"], fr["fx"], fr["fy"], fr["cx"], fr["cy"], fr.get("gt_depth"),
                                    fr.get("exposure_a"), fr.get("exposure_b"), fr.get("global_scale", 1.0), keep)
                if size is not None and hw != size:
                    raise ValueError("TSDFVolume.integrate_frames: frames of one call must share their size")
                size = hw
                table.append(f)
            self._integrate_table((nat.SgrTsdfFrame * len(table))(*table), size[0], size[1])

    def _integrate_table(self, table, H, W):
        """one chunk (<= 16 frames) of raw SgrTsdfFrame records whose device buffers the caller keeps alive"""
        n = len(table)
        nat.check(self._lib.sgr_tsdf_touch(self._vol(), n, table, H, W, _stream()), "sgr_tsdf_touch")
        cnt = self._counters().cpu()                                     # the one synchronisation of the chunk
        while int(cnt[1]) or 2 * int(cnt[0]) > self.hash_capacity:      # full or over half: larger hash, touch again (idempotent)
            self._rehash(2 * self.hash_capacity)
            nat.check(self._lib.sgr_tsdf_touch(self._vol(), n, table, H, W, _stream()), "sgr_tsdf_touch")
            cnt = self._counters().cpu()
        if int(cnt[3]):
            raise RuntimeError("TSDFVolume: integration met a unit beyond the pool")
        if int(cnt[0]) > self.pool_capacity:
            self._grow_pool(int(cnt[0]))
        nat.check(self._lib.sgr_tsdf_integrate(self._vol(), n, table, H, W, int(cnt[2]), _stream()), "sgr_tsdf_integrate")
        self.num_units = int(cnt[0])

    # ---- read-back and extraction
    def voxels(self):
        """the allocated units in ascending key order: keys int64 [n,3] (unit coordinates), tsdf / weight float32 [n,4096] and
        color float32 [n,4096,3] on 0..255, voxel v = x + 16 y + 256 z"""
        cap = self.hash_capacity
        keys = self._state[:cap * 8].view(torch.int64)
        slot_unit = self._state[cap * 8:cap * 12].view(torch.int32)
        used = keys != -1
        k, u = keys[used], slot_unit[used].long()
        order = torch.argsort(k)
        k, u = k[order], u[order]
        bias, m = 1 << 20, (1 << 21) - 1
        coords = torch.stack([((k >> 42) & m) - bias, ((k >> 21) & m) - bias, (k & m) - bias], 1)
        pool = self._pool.view(-1, 5, 4096)[u]
        return {"keys": coords, "tsdf": pool[:, 0].contiguous(), "weight": pool[:, 1].contiguous(),
                "color": pool[:, 2:5].permute(0, 2, 1).contiguous()}

    def extract_triangle_mesh(self):
        """marching cubes: vertices in (unit key, voxel, edge) order, colours 0..1"""
        n = self.num_units
        scratch_bytes = self._lib.sgr_tsdf_extract_bytes(self.hash_capacity, self.pool_capacity)
        scratch = torch.empty(scratch_bytes, dtype=torch.uint8, device=self.device)
        totals = torch.zeros(2, dtype=torch.int32, device=self.device)
        v = self._vol()
        nat.check(self._lib.sgr_tsdf_extract_count(v, n, scratch.data_ptr(), scratch_bytes, totals.data_ptr(), _stream()),
                  "sgr_tsdf_extract_count")
        nv, nt = (int(x) for x in totals.cpu())
        verts = torch.empty(nv, 3, dtype=torch.float32, device=self.device)
        cols = torch.empty(nv, 3, dtype=torch.float32, device=self.device)
        tris = torch.empty(nt, 3, dtype=torch.int32, device=self.device)
        if n:
            nat.check(self._lib.sgr_tsdf_extract(v, n, scratch.data_ptr(), scratch_bytes, verts.data_ptr(), cols.data_ptr(),
                                                 tris.data_ptr(), _stream()), "sgr_tsdf_extract")
        return TriangleMesh(verts, tris, cols)


def clean_mesh(mesh, min_len=100, return_vertex_map=False):
    """clean_mesh of eval_utils.py:331-379: keep the connected components of at least min_len vertices, then drop faces with a
    repeated index or zero area and repeated faces.  Vertices and faces keep their original order; colours stay float.  With
    return_vertex_map, also the new index of every input vertex (-1: dropped)."""
    if int(min_len) < 1:
        raise ValueError(f"clean_mesh: min_len must be >= 1, got {min_len}")
    v, t, c = mesh.vertices, mesh.triangles, mesh.vertex_colors
    _need_gpu(v, t, c)
    if v.dim() != 2 or v.shape[1] != 3 or c.shape != v.shape or t.dim() != 2 or t.shape[1] != 3:
        raise ValueError(f"clean_mesh: vertices / colours must be [V,3] and triangles [F,3], got {tuple(v.shape)}, "
                         f"{tuple(c.shape)}, {tuple(t.shape)}")
    if v.dtype != torch.float32 or c.dtype != torch.float32 or t.dtype != torch.int32:
        raise TypeError("clean_mesh: vertices and colours must be fp32, triangles int32")
    lib = nat.lib()
    v, t, c = v.contiguous(), t.contiguous(), c.contiguous()
    V, F = v.shape[0], t.shape[0]
    if F and (int(t.min()) < 0 or int(t.max()) >= V):
        raise ValueError(f"clean_mesh: triangle indices outside [0, {V})")
    nbytes = lib.sgr_mesh_bytes(V, F)
    scratch = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=v.device)
    totals = torch.zeros(2, dtype=torch.int32, device=v.device)
    st = _stream()
    nat.check(lib.sgr_mesh_components(V, F, v.data_ptr(), t.data_ptr(), int(min_len), scratch.data_ptr(), nbytes, totals.data_ptr(),
                                      st), "sgr_mesh_components")
    kv, kt = (int(x) for x in totals.cpu())
    ov = torch.empty(kv, 3, dtype=torch.float32, device=v.device)
    oc = torch.empty(kv, 3, dtype=torch.float32, device=v.device)
    ot = torch.empty(kt, 3, dtype=torch.int32, device=v.device)
    vmap = torch.empty(V, dtype=torch.int32, device=v.device) if return_vertex_map else None
    nat.check(lib.sgr_mesh_compact(V, F, v.data_ptr(), c.data_ptr(), t.data_ptr(), scratch.data_ptr(), nbytes, ov.data_ptr(),
                                   oc.data_ptr(), ot.data_ptr(), nat.ptr(vmap), st), "sgr_mesh_compact")
    out = TriangleMesh(ov, ot, oc)
    return (out, vmap) if return_vertex_map else out


__all__ = ["TSDFVolume", "TriangleMesh", "clean_mesh"]
