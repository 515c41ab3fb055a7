"""Culling a mesh to what a set of cameras saw, before it is scored ("Mesh culling"), on the HIP kernels of
csrc/sgr_mesh_cull.hip: the cull_mesh of the NICE-SLAM family of evaluations -- a frustum test, an occlusion test against depth
rendered from the mesh itself, faces of unseen vertices dropped.  The reference does not need it (its configs point at ground-truth
meshes that were culled beforehand); a whole-scene ground truth does.

Conventions: pixel centres sit at integer (u, v) with u = fx x / z + cx; poses are camera -> world 4x4 and are inverted in fp64 on
the host; any number of poses, worked through in chunks of 16.  `occlusion_eps` = 0.03 m and `edge` = 0 are this project's choices,
not a reference's.  There is no near-plane clipping: a triangle with a vertex behind `near` (or outside the guard band of 16384
pixels) is not rasterised, and counted.  That is harmless while triangles are shorter than the camera's clearance to the surface
(TSDF and scanned meshes), and wrong for a wall made of two triangles.

GPU tensors only: there is no CPU path."""
import math

import numpy as np
import torch

from splat_slam_amd import _native as nat
from splat_slam_amd.mesh import TriangleMesh

OCCLUSION_EPS = 0.03            # metres a vertex may lie behind the rendered depth and still count as seen
NEAR = 0.01
CHUNK = nat.SGR_CULL_MAX_FRAMES
RULES = {"all": nat.SGR_CULL_RULE_ALL, "any": nat.SGR_CULL_RULE_ANY}


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _need_gpu(*tensors):
    for t in tensors:
        if t is not None and (not torch.is_tensor(t) or t.device.type != "cuda"):
            raise RuntimeError("splat_slam_amd.mesh_cull needs GPU tensors (HIP only, no CPU fallback)")


def _check_mesh(mesh, what, colors=False):
    v, t, c = mesh.vertices, mesh.triangles, mesh.vertex_colors
    _need_gpu(v, t, c if colors else None)
    if v.dim() != 2 or v.shape[1] != 3 or t.dim() != 2 or t.shape[1] != 3 or (colors and c.shape != v.shape):
        raise ValueError(f"{what}: vertices / colours must be [V,3] and triangles [F,3], got {tuple(v.shape)}, {tuple(t.shape)}")
    if v.dtype != torch.float32 or t.dtype != torch.int32 or (colors and c.dtype != torch.float32):
        raise TypeError(f"{what}: vertices and colours must be fp32, triangles int32")
    V, F = int(v.shape[0]), int(t.shape[0])
    if V == 0:
        raise ValueError(f"{what}: the mesh has no vertices")
    if F and (int(t.min()) < 0 or int(t.max()) >= V):
        raise ValueError(f"{what}: triangle indices outside [0, {V})")
    return v.detach().contiguous(), t.contiguous(), (c.detach().contiguous() if colors else None)


def invert_poses(c2w):
    """world -> camera rows, fp64 numpy [n,3,4], of camera -> world poses (a [n,4,4] tensor / array or a sequence of 4x4)"""
    if torch.is_tensor(c2w) or isinstance(c2w, np.ndarray):
        m = np.asarray(torch.as_tensor(c2w).detach().double().cpu())
    else:
        m = np.stack([np.asarray(torch.as_tensor(p).detach().double().cpu()) for p in c2w]) if len(c2w) else np.zeros((0, 4, 4))
    if m.ndim == 2:
        m = m[None]
    if m.ndim != 3 or m.shape[1:] != (4, 4) or m.shape[0] == 0:
        raise ValueError(f"mesh_cull: poses must be [n,4,4] camera -> world with n >= 1, got {m.shape}")
    if not np.isfinite(m).all():
        raise ValueError("mesh_cull: a pose is not finite")
    return np.stack([np.linalg.inv(p)[:3] for p in m])


def _intrinsics(n, fx, fy, cx, cy):
    """fp64 [n,4]: each of fx, fy, cx, cy one number for every frame or n of them"""
    cols = []
    for name, a in (("fx", fx), ("fy", fy), ("cx", cx), ("cy", cy)):
        a = np.asarray(torch.as_tensor(a).detach().double().cpu()).reshape(-1)
        if a.size not in (1, n):
            raise ValueError(f"mesh_cull: {name} must be one value or one per pose ({n}), got {a.size}")
        cols.append(np.broadcast_to(a, (n,)))
    k = np.stack(cols, 1)
    if not np.isfinite(k).all() or (k[:, :2] <= 0).any():
        raise ValueError("mesh_cull: intrinsics must be finite with fx, fy > 0")
    return k


def _size(H, W):
    H, W = int(H), int(W)
    if not (1 <= H <= nat.SGR_CULL_GUARD_PIXELS and 1 <= W <= nat.SGR_CULL_GUARD_PIXELS):
        raise ValueError(f"mesh_cull: the image must be 1..{nat.SGR_CULL_GUARD_PIXELS} pixels a side, got {H}x{W}")
    return H, W


def _table(w2c, intr):
    tab = (nat.SgrCullFrame * len(w2c))()
    for f, (m, k) in enumerate(zip(w2c, intr)):
        tab[f].w2c[:] = [float(x) for x in m.reshape(-1)]
        tab[f].fx, tab[f].fy, tab[f].cx, tab[f].cy = (float(x) for x in k)
    return tab


# ---- one chunk of at most 16 frames: the entry points as they are
def project(vertices, w2c, intr, near=NEAR):
    """sgr_cull_project: (xy int32 [n,V,2], z fp32 [n,V]) of vertices fp32 [V,3] for n <= 16 world -> camera rows [n,3,4] and
    intrinsics [n,4] (host, fp64)"""
    n, V = len(w2c), int(vertices.shape[0])
    xy = torch.empty(n, V, 2, dtype=torch.int32, device=vertices.device)
    z = torch.empty(n, V, dtype=torch.float32, device=vertices.device)
    nat.check(nat.lib().sgr_cull_project(V, vertices.data_ptr(), n, _table(w2c, intr), float(near), xy.data_ptr(), z.data_ptr(),
                                         _stream()), "sgr_cull_project")
    return xy, z


def rasterize(xy, z, triangles, H, W):
    """sgr_cull_raster: (depth fp32 [n,H,W] with +inf where nothing is hit, skipped int32 [n]) from snapped coordinates"""
    n, V = int(z.shape[0]), int(z.shape[1])
    F = int(triangles.shape[0])
    lib = nat.lib()
    nbytes = lib.sgr_cull_raster_bytes(F, n)
    scratch = torch.empty(nbytes, dtype=torch.uint8, device=z.device)
    depth = torch.empty(n, H, W, dtype=torch.float32, device=z.device)
    skipped = torch.empty(n, dtype=torch.int32, device=z.device)
    nat.check(lib.sgr_cull_raster(V, F, triangles.data_ptr(), n, xy.data_ptr(), z.data_ptr(), H, W, depth.data_ptr(), skipped.data_ptr(),
                                  scratch.data_ptr(), nbytes, _stream()), "sgr_cull_raster")
    return depth, skipped


def count_visible(xy, z, depth, H, W, seen, edge=0, far=math.inf, eps=OCCLUSION_EPS):
    """sgr_cull_visibility: seen int32 [V] += the number of the chunk's frames that see each vertex (depth None: frustum only)"""
    n, V = int(z.shape[0]), int(z.shape[1])
    nat.check(nat.lib().sgr_cull_visibility(V, n, xy.data_ptr(), z.data_ptr(), nat.ptr(depth), H, W, int(edge), float(far), float(eps),
                                            seen.data_ptr(), _stream()), "sgr_cull_visibility")
    return seen


def select(mesh, seen, min_views=1, rule="all"):
    """sgr_cull_select + sgr_cull_compact: (the mesh of the faces whose vertices -- all of them, or any -- have seen >= min_views, in
    the original order and reindexed; vertex_map int32 [V], the new index of every input vertex or -1)"""
    if rule not in RULES:
        raise ValueError(f"mesh_cull: rule must be 'all' or 'any', got {rule!r}")
    if int(min_views) < 1:
        raise ValueError(f"mesh_cull: min_views must be >= 1, got {min_views}")
    v, t, c = _check_mesh(mesh, "mesh_cull.select", colors=True)
    _need_gpu(seen)
    V, F = int(v.shape[0]), int(t.shape[0])
    if seen.dtype != torch.int32 or tuple(seen.shape) != (V,):
        raise ValueError(f"mesh_cull.select: seen must be int32 [{V}], got {seen.dtype} {tuple(seen.shape)}")
    lib = nat.lib()
    nbytes = lib.sgr_cull_select_bytes(V, F)
    scratch = torch.empty(nbytes, dtype=torch.uint8, device=v.device)
    totals = torch.zeros(2, dtype=torch.int32, device=v.device)
    st = _stream()
    nat.check(lib.sgr_cull_select(V, F, t.data_ptr(), seen.contiguous().data_ptr(), int(min_views), RULES[rule], scratch.data_ptr(), nbytes,
                                  totals.data_ptr(), st), "sgr_cull_select")
    kv, kt = (int(x) for x in totals.cpu())
    ov = torch.empty(kv, 3, dtype=torch.float32, device=v.device)
    oc = torch.empty(kv, 3, dtype=torch.float32, device=v.device)
    ot = torch.empty(kt, 3, dtype=torch.int32, device=v.device)
    vmap = torch.empty(V, dtype=torch.int32, device=v.device)
    nat.check(lib.sgr_cull_compact(V, F, v.data_ptr(), c.data_ptr(), t.data_ptr(), scratch.data_ptr(), nbytes, ov.data_ptr(),
                                   oc.data_ptr(), ot.data_ptr(), vmap.data_ptr(), st), "sgr_cull_compact")
    return TriangleMesh(ov, ot, oc), vmap


# ---- any number of poses
def _chunks(c2w, fx, fy, cx, cy):
    w2c = invert_poses(c2w)
    intr = _intrinsics(len(w2c), fx, fy, cx, cy)
    return [(c0, w2c[c0:c0 + CHUNK], intr[c0:c0 + CHUNK]) for c0 in range(0, len(w2c), CHUNK)]


def _near(near):
    if not float(near) > 0.0:
        raise ValueError(f"mesh_cull: near must be > 0, got {near}")
    return float(near)


def render_mesh_depth(mesh, c2w, fx, fy, cx, cy, H, W, near=NEAR):
    """The mesh's depth from every pose: (depth fp32 [n,H,W], +inf where nothing is hit; int32 [n], the triangles of each frame
    that were not rasterised because a vertex lies behind `near` or outside the guard band)."""
    v, t, _ = _check_mesh(mesh, "render_mesh_depth")
    H, W = _size(H, W)
    near = _near(near)
    depths, skipped = [], []
    for _, w2c, intr in _chunks(c2w, fx, fy, cx, cy):
        xy, z = project(v, w2c, intr, near)
        d, s = rasterize(xy, z, t, H, W)
        depths.append(d)
        skipped.append(s)
    return torch.cat(depths), torch.cat(skipped)


def _visibility(mesh, c2w, intrinsics, H, W, occlusion, edge, near, far, occlusion_eps, what):
    v, t, _ = _check_mesh(mesh, what)
    H, W = _size(H, W)
    near = _near(near)
    if int(edge) < 0 or not float(far) > 0.0 or not math.isfinite(float(occlusion_eps)):
        raise ValueError(f"{what}: edge must be >= 0, far > 0 and occlusion_eps finite, got {edge}, {far}, {occlusion_eps}")
    k = np.asarray(torch.as_tensor(intrinsics).detach().double().cpu())
    if k.ndim not in (1, 2) or k.shape[-1] != 4:
        raise ValueError(f"{what}: intrinsics must be (fx, fy, cx, cy) or one such row per pose, got {k.shape}")
    k = k.reshape(-1, 4)
    chunks = _chunks(c2w, k[:, 0], k[:, 1], k[:, 2], k[:, 3])
    n = sum(len(w) for _, w, _ in chunks)
    supplied = None
    if torch.is_tensor(occlusion):
        _need_gpu(occlusion)
        if occlusion.dtype != torch.float32 or tuple(occlusion.shape) != (n, H, W):
            raise ValueError(f"{what}: occlusion depths must be fp32 [{n},{H},{W}], got {occlusion.dtype} {tuple(occlusion.shape)}")
        supplied = occlusion.detach().contiguous()
    elif occlusion is not None and not (isinstance(occlusion, str) and occlusion == "mesh"):
        raise ValueError(f"{what}: occlusion must be 'mesh', None or a depth tensor, got {occlusion!r}")
    seen = torch.zeros(v.shape[0], dtype=torch.int32, device=v.device)
    unrasterized = 0
    for c0, w2c, intr in chunks:
        xy, z = project(v, w2c, intr, near)
        depth = None
        if supplied is not None:
            depth = supplied[c0:c0 + len(w2c)]
        elif occlusion == "mesh":
            depth, skipped = rasterize(xy, z, t, H, W)
            unrasterized = max(unrasterized, int(skipped.max()))
        count_visible(xy, z, depth, H, W, seen, edge, far, occlusion_eps)
    return seen, unrasterized


def vertex_visibility(mesh, c2w, intrinsics, H, W, occlusion="mesh", edge=0, near=NEAR, far=math.inf, occlusion_eps=OCCLUSION_EPS):
    """seen int32 [V]: the number of poses (camera -> world [n,4,4]) that see each vertex of the mesh.  intrinsics: (fx, fy, cx, cy)
    for every pose or [n,4].  A pose sees a vertex whose camera z is in [near, far], whose nearest pixel lies at least `edge` pixels
    inside the H x W image and which is not occluded: occlusion="mesh" renders the mesh's own depth and asks z - depth <=
    occlusion_eps; a tensor fp32 [n,H,W] supplies the depth maps (zero, negative and NaN depth constrain nothing, like sensor
    holes); None tests the frustum only.  occlusion_eps = 0.03 m and edge = 0 are this project's choices."""
    return _visibility(mesh, c2w, intrinsics, H, W, occlusion, edge, near, far, occlusion_eps, "vertex_visibility")[0]


def cull_mesh(mesh, c2w, intrinsics, H, W, occlusion="mesh", edge=0, near=NEAR, far=math.inf, occlusion_eps=OCCLUSION_EPS, min_views=1,
              rule="all", return_info=False):
    """The mesh without what the poses did not see: vertex_visibility's count per vertex, then the faces whose vertices -- all of
    them (rule="all") or any (rule="any") -- were seen by at least min_views poses, and the vertices those faces reference, in
    their original order.  With return_info also a dict: seen, vertex_map (new index or -1), vertices_before / _after, faces_before /
    _after and unrasterized_triangles (the largest number, over the poses, of triangles left out of the occlusion depth because a
    vertex lies behind `near`: there is no near-plane clipping)."""
    if rule not in RULES:
        raise ValueError(f"cull_mesh: rule must be 'all' or 'any', got {rule!r}")
    if int(min_views) < 1:
        raise ValueError(f"cull_mesh: min_views must be >= 1, got {min_views}")
    _check_mesh(mesh, "cull_mesh", colors=True)
    seen, unrasterized = _visibility(mesh, c2w, intrinsics, H, W, occlusion, edge, near, far, occlusion_eps, "cull_mesh")
    out, vmap = select(mesh, seen, min_views, rule)
    if not return_info:
        return out
    return out, {"seen": seen, "vertex_map": vmap, "vertices_before": len(mesh), "vertices_after": len(out),
                 "faces_before": int(mesh.triangles.shape[0]), "faces_after": int(out.triangles.shape[0]),
                 "unrasterized_triangles": unrasterized}


__all__ = ["render_mesh_depth", "vertex_visibility", "cull_mesh"]
