"""Mesh culling without a GPU: csrc/sgr_mesh_cull.hip (with the shared csrc/sgr_scan.hip) compiles for gfx950 without scratch, spills or float atomics, its entry points
are declared, exported and bound and refuse bad arguments before any launch, splat_slam_amd.mesh_cull refuses what it does not
implement, the restatement of tests/mesh_cull_ref.py gets simple cases right, and the inputs of the GPU tests are well conditioned:
no projected coordinate sits on a rounding tie."""
import ctypes
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

import mesh_cull_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
KERNELS = ("cull_project_kernel", "cull_raster_small_kernel", "cull_raster_large_kernel", "cull_visibility_kernel",
           "cull_face_keep_kernel", "scan_local_kernel", "chunked_scan_kernel", "scan_add_kernel",
           "compact_vertices_kernel", "compact_triangles_kernel")
SOURCES = ("sgr_mesh_cull", "sgr_scan")          # the file and what it launches through sgr_scan.h (the scans, the compaction)
ENTRY_POINTS = ("sgr_cull_project", "sgr_cull_raster_bytes", "sgr_cull_raster", "sgr_cull_visibility", "sgr_cull_select_bytes",
                "sgr_cull_select", "sgr_cull_compact")


# ---- ISA budget and ABI
@pytest.fixture(scope="module")
def cull_isa(tmp_path_factory):
    if not (os.path.exists(HIPCC) or shutil.which(HIPCC)):
        pytest.skip("hipcc not available")
    text, meta = "", {}
    for src in SOURCES:
        out = str(tmp_path_factory.mktemp("isa") / (src + ".s"))
        subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-S", "--cuda-device-only", "-o", out,
                        os.path.join(ROOT, "splat_slam_amd", "csrc", src + ".hip")], check=True, capture_output=True)
        one = open(out).read()
        text += one
        for block in one.split("\n  - ")[1:]:
            m = re.search(r"\.name:\s+(\S+)", block)
            if m and ".private_segment_fixed_size" in block:
                assert m.group(1) not in meta, m.group(1)
                meta[m.group(1)] = block
    return text, meta


def test_every_mesh_cull_kernel_has_no_scratch_no_spills_and_no_float_atomics(cull_isa):
    text, meta = cull_isa
    for k in KERNELS:
        names = [n for n in meta if re.search(r"\d%s" % k, n)]
        assert len(names) == 1, (k, sorted(meta))
        block = meta[names[0]]
        scratch = int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", block).group(1))
        spill = int(re.search(r"\.vgpr_spill_count:\s+(\d+)", block).group(1))
        sspill = int(re.search(r"\.sgpr_spill_count:\s+(\d+)", block).group(1))
        assert scratch == 0 and spill == 0 and sspill == 0, (k, scratch, spill, sspill)
    assert len(meta) == len(KERNELS), sorted(meta)
    assert not re.search(r"(global|flat|buffer|ds)_atomic_\w*(f32|f64|pk_add)", text)
    assert re.search(r"(global|flat)_atomic_umin\b", text)          # the z-buffer: an integer minimum on the depth's bits


def test_mesh_cull_entry_points_are_declared_exported_and_bound():
    from splat_slam_amd.build import build_native
    from splat_slam_amd import _native as nat
    path = build_native(verbose=False)
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "splat_hip.h")).read(), flags=re.S)
    h = ctypes.CDLL(path)
    for name in ENTRY_POINTS:
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert hasattr(h, name), name
        assert name in nat.SIGNATURES, name
    lib = nat.lib()
    assert lib.sgr_abi_version() == 10
    assert (nat.SGR_CULL_MAX_FRAMES, nat.SGR_CULL_SUBPIXEL_BITS, nat.SGR_CULL_GUARD_PIXELS) == (16, 8, 16384)
    assert ctypes.sizeof(nat.SgrCullFrame) == 16 * 8
    # host-only size functions
    assert lib.sgr_cull_raster_bytes(1000, 16) >= 1000 * 16 * 8 and lib.sgr_cull_raster_bytes(1000, 17) == 0
    assert lib.sgr_cull_raster_bytes(0, 1) > 0
    assert lib.sgr_cull_select_bytes(1000, 2000) >= (1000 + 2000 + 2) * 4 and lib.sgr_cull_select_bytes(-1, 0) == 0


def test_entry_points_refuse_bad_arguments_before_any_launch():
    from splat_slam_amd import _native as nat
    lib = nat.lib()
    buf = ctypes.create_string_buffer(4096)
    p = ctypes.addressof(buf)                       # a host address: nothing may be launched on it
    frames = (nat.SgrCullFrame * 16)()
    INV, WS = nat.SGR_ERR_INVALID, nat.SGR_ERR_WORKSPACE
    # project
    assert lib.sgr_cull_project(0, p, 1, frames, 0.01, p, p, None) == INV and "cull_project" in nat.last_error()
    for n in (0, 17, -1):
        assert lib.sgr_cull_project(4, p, n, frames, 0.01, p, p, None) == INV
    assert lib.sgr_cull_project(4, None, 1, frames, 0.01, p, p, None) == INV
    assert lib.sgr_cull_project(4, p, 1, None, 0.01, p, p, None) == INV
    assert lib.sgr_cull_project(4, p, 1, frames, 0.01, None, p, None) == INV
    assert lib.sgr_cull_project(4, p, 1, frames, 0.01, p, None, None) == INV
    assert lib.sgr_cull_project(4, p, 1, frames, 0.0, p, p, None) == INV
    assert lib.sgr_cull_project(4, p, 1, frames, math.nan, p, p, None) == INV
    # raster
    need = lib.sgr_cull_raster_bytes(8, 2)
    assert lib.sgr_cull_raster(4, 8, p, 2, p, p, 0, 8, p, None, p, need, None) == INV and "cull_raster" in nat.last_error()
    assert lib.sgr_cull_raster(4, 8, p, 2, p, p, 8, 0, p, None, p, need, None) == INV
    assert lib.sgr_cull_raster(4, 8, p, 2, p, p, 8, 16385, p, None, p, need, None) == INV
    assert lib.sgr_cull_raster(4, 8, p, 0, p, p, 8, 8, p, None, p, need, None) == INV
    assert lib.sgr_cull_raster(4, 8, p, 17, p, p, 8, 8, p, None, p, need, None) == INV
    assert lib.sgr_cull_raster(0, 8, p, 2, p, p, 8, 8, p, None, p, need, None) == INV
    assert lib.sgr_cull_raster(4, 8, None, 2, p, p, 8, 8, p, None, p, need, None) == INV
    assert lib.sgr_cull_raster(4, 8, p, 2, None, p, 8, 8, p, None, p, need, None) == INV
    assert lib.sgr_cull_raster(4, 8, p, 2, p, None, 8, 8, p, None, p, need, None) == INV
    assert lib.sgr_cull_raster(4, 8, p, 2, p, p, 8, 8, None, None, p, need, None) == INV
    assert lib.sgr_cull_raster(4, 8, p, 2, p, p, 8, 8, p, None, p, need - 1, None) == WS and "scratch" in nat.last_error()
    assert lib.sgr_cull_raster(4, 8, p, 2, p, p, 8, 8, p, None, None, need, None) == WS
    # visibility
    assert lib.sgr_cull_visibility(0, 1, p, p, None, 8, 8, 0, math.inf, 0.03, p, None) == INV and "cull_visibility" in nat.last_error()
    for n in (0, 17):
        assert lib.sgr_cull_visibility(4, n, p, p, None, 8, 8, 0, math.inf, 0.03, p, None) == INV
    assert lib.sgr_cull_visibility(4, 1, p, p, None, 0, 8, 0, math.inf, 0.03, p, None) == INV
    assert lib.sgr_cull_visibility(4, 1, p, p, None, 8, 0, 0, math.inf, 0.03, p, None) == INV
    assert lib.sgr_cull_visibility(4, 1, p, p, None, 8, 8, -1, math.inf, 0.03, p, None) == INV
    assert lib.sgr_cull_visibility(4, 1, None, p, None, 8, 8, 0, math.inf, 0.03, p, None) == INV
    assert lib.sgr_cull_visibility(4, 1, p, None, None, 8, 8, 0, math.inf, 0.03, p, None) == INV
    assert lib.sgr_cull_visibility(4, 1, p, p, None, 8, 8, 0, math.inf, 0.03, None, None) == INV
    assert lib.sgr_cull_visibility(4, 1, p, p, None, 8, 8, 0, math.nan, 0.03, p, None) == INV
    assert lib.sgr_cull_visibility(4, 1, p, p, None, 8, 8, 0, math.inf, math.nan, p, None) == INV
    # select / compact
    need = lib.sgr_cull_select_bytes(4, 8)
    assert lib.sgr_cull_select(-1, 8, p, p, 1, 0, p, need, p, None) == INV and "cull_select" in nat.last_error()
    assert lib.sgr_cull_select(4, 8, None, p, 1, 0, p, need, p, None) == INV
    assert lib.sgr_cull_select(4, 8, p, None, 1, 0, p, need, p, None) == INV
    assert lib.sgr_cull_select(4, 8, p, p, 0, 0, p, need, p, None) == INV
    assert lib.sgr_cull_select(4, 8, p, p, 1, 2, p, need, p, None) == INV
    assert lib.sgr_cull_select(4, 8, p, p, 1, 0, p, need, None, None) == INV
    assert lib.sgr_cull_select(4, 8, p, p, 1, 0, p, need - 1, p, None) == WS
    assert lib.sgr_cull_select(4, 8, p, p, 1, 0, None, need, p, None) == WS
    assert lib.sgr_cull_compact(4, 8, None, p, p, p, need, p, p, p, None, None) == INV and "cull_compact" in nat.last_error()
    assert lib.sgr_cull_compact(4, 8, p, None, p, p, need, p, p, p, None, None) == INV
    assert lib.sgr_cull_compact(4, 8, p, p, None, p, need, p, p, p, None, None) == INV
    assert lib.sgr_cull_compact(4, 8, p, p, p, p, need - 1, p, p, p, None, None) == WS


# ---- argument checks of the Python layer
def _host_mesh():
    from splat_slam_amd.mesh import TriangleMesh
    v = torch.rand(4, 3)
    return TriangleMesh(v, torch.tensor([[0, 1, 2], [1, 2, 3]], dtype=torch.int32), v.clone())


def test_mesh_cull_refuses_cpu_tensors():
    from splat_slam_amd import mesh_cull as mc
    m, pose = _host_mesh(), np.eye(4)[None]
    with pytest.raises(RuntimeError, match="GPU"):
        mc.render_mesh_depth(m, pose, 50.0, 50.0, 16.0, 12.0, 24, 32)
    with pytest.raises(RuntimeError, match="GPU"):
        mc.vertex_visibility(m, pose, (50.0, 50.0, 16.0, 12.0), 24, 32)
    with pytest.raises(RuntimeError, match="GPU"):
        mc.cull_mesh(m, pose, (50.0, 50.0, 16.0, 12.0), 24, 32)
    with pytest.raises(RuntimeError, match="GPU"):
        mc.select(m, torch.zeros(4, dtype=torch.int32))


def test_mesh_cull_refuses_bad_arguments_before_the_device(monkeypatch):
    """the host-side checks, on host tensors with the GPU check lifted: each raises before anything reaches the library"""
    from splat_slam_amd import mesh_cull as mc
    from splat_slam_amd.mesh import TriangleMesh
    monkeypatch.setattr(mc, "_need_gpu", lambda *a: None)
    m, pose, k = _host_mesh(), np.eye(4)[None], (50.0, 50.0, 16.0, 12.0)
    v = m.vertices
    with pytest.raises(ValueError, match="outside"):
        mc.cull_mesh(TriangleMesh(v, torch.tensor([[0, 1, 4]], dtype=torch.int32), v), pose, k, 24, 32)
    with pytest.raises(ValueError, match="outside"):
        mc.vertex_visibility(TriangleMesh(v, torch.tensor([[0, -1, 2]], dtype=torch.int32), v), pose, k, 24, 32)
    with pytest.raises(TypeError, match="int32"):
        mc.render_mesh_depth(TriangleMesh(v, m.triangles.long(), v), pose, *k, 24, 32)
    with pytest.raises(TypeError, match="fp32"):
        mc.vertex_visibility(TriangleMesh(v.double(), m.triangles, v), pose, k, 24, 32)
    with pytest.raises(ValueError, match=r"\[V,3\]"):
        mc.vertex_visibility(TriangleMesh(v[:, :2], m.triangles, v), pose, k, 24, 32)
    with pytest.raises(ValueError, match="no vertices"):
        mc.vertex_visibility(TriangleMesh(v[:0], m.triangles[:0], v[:0]), pose, k, 24, 32)
    with pytest.raises(ValueError, match="poses"):
        mc.vertex_visibility(m, np.eye(3)[None], k, 24, 32)
    with pytest.raises(ValueError, match="poses"):
        mc.vertex_visibility(m, [], k, 24, 32)
    with pytest.raises(ValueError, match="not finite"):
        mc.vertex_visibility(m, np.full((1, 4, 4), np.nan), k, 24, 32)
    with pytest.raises(ValueError, match="intrinsics"):
        mc.vertex_visibility(m, pose, (50.0, 50.0, 16.0), 24, 32)
    with pytest.raises(ValueError, match="one per pose"):
        mc.vertex_visibility(m, pose, np.tile(k, (3, 1)), 24, 32)
    with pytest.raises(ValueError, match="fx, fy > 0"):
        mc.vertex_visibility(m, pose, (0.0, 50.0, 16.0, 12.0), 24, 32)
    with pytest.raises(ValueError, match="image"):
        mc.vertex_visibility(m, pose, k, 0, 32)
    with pytest.raises(ValueError, match="image"):
        mc.render_mesh_depth(m, pose, *k, 24, 16385)
    with pytest.raises(ValueError, match="near"):
        mc.render_mesh_depth(m, pose, *k, 24, 32, near=0.0)
    with pytest.raises(ValueError, match="edge"):
        mc.vertex_visibility(m, pose, k, 24, 32, edge=-1)
    with pytest.raises(ValueError, match="far"):
        mc.vertex_visibility(m, pose, k, 24, 32, far=0.0)
    with pytest.raises(ValueError, match="occlusion"):
        mc.vertex_visibility(m, pose, k, 24, 32, occlusion="depth")
    with pytest.raises(ValueError, match="occlusion depths"):
        mc.vertex_visibility(m, pose, k, 24, 32, occlusion=torch.zeros(2, 24, 32))
    with pytest.raises(ValueError, match="rule"):
        mc.cull_mesh(m, pose, k, 24, 32, rule="most")
    with pytest.raises(ValueError, match="min_views"):
        mc.cull_mesh(m, pose, k, 24, 32, min_views=0)
    with pytest.raises(ValueError, match="seen"):
        mc.select(m, torch.zeros(5, dtype=torch.int32))
    with pytest.raises(ValueError, match="seen"):
        mc.select(m, torch.zeros(4, dtype=torch.int64))


def test_poses_are_inverted_in_fp64_and_intrinsics_broadcast():
    from splat_slam_amd import mesh_cull as mc
    c2w = ref.room_cameras(3)
    w = mc.invert_poses(torch.from_numpy(c2w).float().double())
    assert w.dtype == np.float64 and w.shape == (3, 3, 4)
    assert np.array_equal(mc.invert_poses([torch.from_numpy(p) for p in c2w]), ref.invert(c2w))
    assert np.array_equal(mc.invert_poses(c2w[0]), ref.invert(c2w[:1]))
    k = mc._intrinsics(3, 50.0, [51.0, 52.0, 53.0], torch.tensor(16.0), 12)
    assert k.dtype == np.float64 and k.tolist() == [[50.0, 51.0, 16.0, 12.0], [50.0, 52.0, 16.0, 12.0], [50.0, 53.0, 16.0, 12.0]]
    tab = mc._table(ref.invert(c2w), k)
    assert np.array_equal(np.array(tab[2].w2c[:]).reshape(3, 4), ref.invert(c2w)[2]) and tab[1].fy == 52.0


def test_eval_rendering_refuses_as_before_with_the_culling_arguments():
    import types
    from splat_slam_amd.eval import eval_rendering
    frame = types.SimpleNamespace(original_image=torch.zeros(3, 4, 4))
    with pytest.raises(RuntimeError, match="GPU tensors"):
        eval_rendering([frame], None, None, None, mesh=True, cull_mesh=True, cull_poses=[np.eye(4)])
    with pytest.raises(ValueError, match="no frames"):
        eval_rendering([], None, None, None, mesh=True, cull_mesh=True)


# ---- the restatement
def _quad(z00, z10, z01, z11, H, W):
    """two triangles over the whole image and more, corner depths given: (xy, z, triangles)"""
    xy = np.array([(-3, -2), (W + 2, -2), (-3, H + 1), (W + 2, H + 1)], np.int64) * ref.SUB
    return xy, np.array([z00, z10, z01, z11], np.float32), np.array([(0, 1, 2), (1, 3, 2)])


def test_restated_raster_of_a_fronto_parallel_plane_is_its_constant_depth():
    H, W = 11, 17
    d, skipped = ref.raster(*_quad(2.5, 2.5, 2.5, 2.5, H, W), H, W)
    assert skipped == 0 and np.all(np.abs(d - 2.5) < 1e-15)


def test_restated_raster_of_a_tilted_plane_is_affine_in_inverse_depth():
    H, W = 11, 17
    d, _ = ref.raster(*_quad(1.0, 4.0, 1.0, 4.0, H, W), H, W)       # tilted about the vertical axis: 1/z affine in j, constant in i
    assert np.all(np.isfinite(d))
    inv = 1.0 / d
    want = 1.0 + (np.arange(W) + 3) / (W + 5) * (0.25 - 1.0)
    assert np.abs(inv - want[None, :]).max() < 1e-14
    assert np.abs(np.diff(inv, 2, axis=1)).max() < 1e-14 and np.abs(np.diff(inv, axis=0)).max() < 1e-14


def test_restated_raster_edges_are_inclusive_for_both_windings_and_skip_what_it_must():
    S = ref.SUB
    xy = np.array([(2, 2), (6, 2), (2, 6)], np.int64) * S
    z = np.ones(3, np.float32)
    for tri in ((0, 1, 2), (0, 2, 1)):
        d, _ = ref.raster(xy, z, [tri], 8, 8)
        hit = np.isfinite(d)
        assert hit[2, 2] and hit[2, 6] and hit[6, 2] and hit[4, 4] and not hit[5, 4] and not hit[1, 2] and hit.sum() == 15
    d, s = ref.raster(xy, np.array([1, 0, 1], np.float32), [(0, 1, 2)], 8, 8)
    assert s == 1 and not np.isfinite(d).any()
    d, s = ref.raster(np.array([(1, 1), (3, 3), (6, 6)], np.int64) * S, z, [(0, 1, 2)], 8, 8)
    assert s == 0 and not np.isfinite(d).any()
    # the plane of raster_cases leaves no hole inside
    for H, W in ((37, 53), (48, 64)):
        d, _ = ref.raster(*ref.raster_cases(H, W)["tessellated_plane"], H, W)
        (i0, i1), (j0, j1) = ref.plane_interior(H, W)
        assert np.isfinite(d[i0:i1 + 1, j0:j1 + 1]).all() and np.isfinite(d).sum() == (i1 - i0 + 1) * (j1 - j0 + 1)


def test_restated_projection_and_visibility_classify_the_border_cases():
    w2c, k = np.eye(4)[None, :3], np.array([[50.0, 50.0, 16.0, 12.0]])
    H, W, near = 24, 32, 0.25                                   # (near and every coordinate below are exact in fp32)
    at = lambda u, v, z: ((u - 16.0) * z / 50.0, (v - 12.0) * z / 50.0, z)
    pts = np.array([at(7.0, 5.0, 2.0),                          # exactly a pixel centre
                    at(7.5, 5.0, 2.0),                          # half way: 7.5 * 256 + 128 = 2048 -> pixel 8
                    at(-0.5, 0.0, 2.0), at(-0.5 - 1 / 256, 0.0, 2.0),       # the left border: pixel 0, then outside
                    at(31.0 + 127 / 256, 23.0, 2.0), at(31.5, 23.0, 2.0),   # the right border: pixel 31, then 32: outside
                    (0.0, 0.0, near), (0.0, 0.0, np.nextafter(np.float32(near), np.float32(0)))], np.float64)
    xy, z = ref.project(pts, w2c, k, near)
    assert xy[0, 0].tolist() == [7 * 256, 5 * 256] and z[0, 0] == 2.0
    assert xy[0, 1, 0] == 7 * 256 + 128
    assert z[0, 6] == np.float32(near) and z[0, 7] == 0 and xy[0, 7].tolist() == [0, 0]
    per_vertex = lambda **kw: [int(ref.visibility(xy[:, i:i + 1], z[:, i:i + 1], None, H, W, **kw)[0]) for i in range(len(pts))]
    assert per_vertex() == [1, 1, 1, 0, 1, 0, 1, 0]
    assert per_vertex(edge=5) == [1, 1, 0, 0, 0, 0, 1, 0]
    assert per_vertex(far=1.0) == [0, 0, 0, 0, 0, 0, 1, 0]
    # depth maps: a hole (0, NaN, negative) constrains nothing, +inf passes, and z - d <= eps is one fp32 subtraction
    one = lambda d, eps: int(ref.visibility(xy[:, :1], z[:, :1], np.full((1, H, W), d, np.float32), H, W, eps=eps)[0])
    assert [one(d, 0.03) for d in (0.0, np.nan, -1.0, np.inf, 2.0, 1.98, 1.96)] == [1, 1, 1, 1, 1, 1, 0]
    d = np.float32(2.0) - np.float32(0.03)
    assert one(d, np.float32(2.0) - d) == 1 and one(np.nextafter(d, np.float32(0)), np.float32(2.0) - d) == 0


def test_restated_selection_keeps_order_and_reindexes():
    tris = np.array([(0, 1, 2), (2, 3, 4), (4, 5, 0), (1, 3, 5)])
    seen = np.array([2, 1, 1, 0, 2, 2])
    kv, kf, faces, vmap = ref.select(6, tris, seen, 1, "all")
    assert kv.tolist() == [0, 1, 2, 4, 5] and kf.tolist() == [0, 2] and faces.tolist() == [[0, 1, 2], [3, 4, 0]]
    assert vmap.tolist() == [0, 1, 2, -1, 3, 4]
    kv, kf, faces, vmap = ref.select(6, tris, seen, 2, "any")
    assert kf.tolist() == [0, 1, 2, 3] and kv.tolist() == [0, 1, 2, 3, 4, 5]
    kv, kf, faces, vmap = ref.select(6, tris, seen, 3, "any")
    assert len(kv) == 0 and len(kf) == 0 and (vmap == -1).all()


# ---- conditioning of the GPU tests' inputs
def _margins(vertices, c2w, intr, near=0.01):
    """(distance of 256 u and 256 v from a rounding tie, relative distance of p.z from an fp32 rounding boundary and from near,
    distance of |u|, |v| from the guard), over the finite vertices in front of the camera: minima"""
    us, vs, pz = ref.project_raw(vertices, ref.invert(c2w), intr)
    with np.errstate(all="ignore"):
        fin = np.isfinite(us) & np.isfinite(vs) & np.isfinite(pz)
        near_rel = np.abs(pz[np.isfinite(pz)] - near) / near
        front = fin & (pz >= near)
        inside = front & (np.abs(us) <= ref.GUARD * ref.SUB) & (np.abs(vs) <= ref.GUARD * ref.SUB)
        tie = np.minimum(np.abs(np.abs(us[inside] - np.floor(us[inside])) - 0.5), np.abs(np.abs(vs[inside] - np.floor(vs[inside])) - 0.5))
        guard = np.minimum(np.abs(np.abs(us[front]) / ref.SUB - ref.GUARD), np.abs(np.abs(vs[front]) / ref.SUB - ref.GUARD))
        z = pz[front]
        zf = z.astype(np.float32)
        lo, hi = np.nextafter(zf, np.float32(-np.inf)).astype(np.float64), np.nextafter(zf, np.float32(np.inf)).astype(np.float64)
        zf = zf.astype(np.float64)
        bound = np.minimum(np.abs(z - 0.5 * (zf + lo)), np.abs(z - 0.5 * (zf + hi))) / np.abs(z)
    return tie.min(), bound.min(), near_rel.min(), guard.min()


def _scenes():
    """the inputs whose projection the GPU tests compare with the restatement (the other GPU tests start from the kernel's own
    coordinates)"""
    return ref.project_inputs()


@pytest.mark.parametrize("name", sorted(_scenes()))
def test_gpu_test_inputs_are_away_from_every_rounding_tie(name):
    """the GPU tests compare integers and bits with no vertex excluded: that holds when no fp64 256 u or 256 v lies within 1e-9 of a
    tie, and no p.z within 1e-9 (relative) of an fp32 rounding boundary, of near or |u|, |v| of the guard.  Verified here; an input
    that violates it gets another pose, not an allowance."""
    v, c2w, intr = _scenes()[name]
    tie, bound, near_rel, guard = _margins(v, c2w, intr)
    assert tie > 1e-9, tie
    assert bound > 1e-9, bound
    assert near_rel > 1e-9, near_rel
    assert guard > 1e-9 * ref.GUARD, guard


# ---- Slam.evaluate
def test_slam_evaluate_hands_the_culling_keywords_only_when_asked(monkeypatch):
    """Slam.evaluate on a stand-in for a finished run: what reaches eval_rendering without cull_mesh is what reached it before; with
    it, cull_mesh=True and the ground-truth poses of the keyframes (by video timestamp), or None without ground truth"""
    import types
    from splat_slam_amd import eval as eval_mod
    from splat_slam_amd import traj_eval, trajectory_filler
    from splat_slam_amd.slam import Slam
    calls = []
    monkeypatch.setattr(eval_mod, "eval_rendering", lambda *a, **kw: calls.append(kw) or {"psnr": []})

    def degenerate(*a, **kw):
        raise traj_eval.TrajectoryDegenerate("stand-in")

    monkeypatch.setattr(traj_eval, "kf_traj_eval", degenerate)
    monkeypatch.setattr(traj_eval, "full_traj_eval", degenerate)
    monkeypatch.setattr(trajectory_filler, "PoseTrajectoryFiller", lambda *a, **kw: None)
    loop = types.SimpleNamespace(viewpoints={4: "d", 0: "a", 2: "c"}, gaussians=None, background=None)
    video = types.SimpleNamespace(timestamp=torch.tensor([0.0, 3.0, 5.0, 6.0, 9.0, 0.0]), counter=types.SimpleNamespace(value=0),
                                  device="cpu")
    slam = types.SimpleNamespace(stream=types.SimpleNamespace(), video=video, net=None,
                                 session=types.SimpleNamespace(init=False, loop=loop))
    gt = [np.eye(4) * (i + 1) for i in range(10)]
    before = {"gt_depths", "global_scale", "mesh", "mesh_path", "c2w", "gt_mesh_path", "lpips"}
    Slam.evaluate(slam, gt_poses=gt, mesh=True, gt_mesh_path="gt.ply")
    Slam.evaluate(slam, gt_poses=gt, mesh=True, gt_mesh_path="gt.ply", cull_mesh=False)
    assert set(calls[0]) == before and set(calls[1]) == before
    Slam.evaluate(slam, gt_poses=gt, mesh=True, gt_mesh_path="gt.ply", cull_mesh=True)
    assert set(calls[2]) == before | {"cull_mesh", "cull_poses"} and calls[2]["cull_mesh"] is True
    assert [float(p[0, 0]) for p in calls[2]["cull_poses"]] == [1.0, 6.0, 10.0]          # timestamps 0, 5, 9 of keyframes 0, 2, 4
    Slam.evaluate(slam, mesh=True, gt_mesh_path="gt.ply", cull_mesh=True)
    assert calls[3]["cull_mesh"] is True and calls[3]["cull_poses"] is None and calls[3]["c2w"] is None
