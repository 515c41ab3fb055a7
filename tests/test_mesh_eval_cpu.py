"""Mesh evaluation without a GPU: csrc/sgr_mesh_eval.hip (with the shared csrc/sgr_point_grid.hip and csrc/sgr_scan.hip) compiles for gfx950 without scratch, spills or float atomics, its entry
points are declared, exported and bound, read_mesh_ply reads the PLY variants ground-truth meshes come in, splat_slam_amd.mesh_eval
refuses what it does not implement, and the fp64 restatement of tests/mesh_eval_ref.py gets simple cases right."""
import ctypes
import os
import re
import shutil
import struct
import subprocess
import types

import numpy as np
import pytest
import torch

import mesh_eval_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
# the file, the grid build it launches through sgr_point_grid.h, and that build's scan (sgr_scan.hip, with its other kernels)
SOURCES = ("sgr_mesh_eval", "sgr_point_grid", "sgr_scan")
KERNELS = ("area_kernel", "cdf_local_kernel", "cdf_sums_kernel", "cdf_add_kernel", "sample_kernel", "grid_bounds_kernel",
           "grid_setup_kernel", "grid_count_kernel", "chunked_scan_kernel", "grid_fill_kernel", "nn_query_kernel", "icp_partial_kernel",
           "metrics_partial_kernel", "reduce_final_kernel", "scan_local_kernel", "scan_add_kernel", "compact_vertices_kernel",
           "compact_triangles_kernel")
ENTRY_POINTS = ("sgr_surface_sample_bytes", "sgr_surface_sample", "sgr_nn_grid_bytes", "sgr_nn_grid_build", "sgr_nn_query",
                "sgr_eval_reduce_bytes", "sgr_icp_accumulate", "sgr_cloud_metrics")


# ---- ISA budget and ABI
@pytest.fixture(scope="module")
def eval_isa(tmp_path_factory):
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


def test_every_mesh_eval_kernel_has_no_scratch_no_spills_and_no_float_atomics(eval_isa):
    text, meta = eval_isa
    for k in KERNELS:
        names = [n for n in meta if re.search(r"\d%s" % k, n)]
        assert len(names) == 1, (k, sorted(meta))
        block = meta[names[0]]
        scratch = int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", block).group(1))
        spill = int(re.search(r"\.vgpr_spill_count:\s+(\d+)", block).group(1))
        assert scratch == 0 and spill == 0, (k, scratch, spill)
    assert len(meta) == len(KERNELS), sorted(meta)
    assert not re.search(r"(global|flat|buffer|ds)_atomic_\w*(f32|f64|pk_add)", text)
    assert not re.search(r"(global|flat|buffer)_atomic_pk_add", text)


def test_mesh_eval_entry_points_are_declared_exported_and_bound():
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
    # host-only size functions
    assert lib.sgr_nn_grid_bytes(0) == 0 and lib.sgr_nn_grid_bytes(1000) >= 1000 * 20
    assert lib.sgr_nn_grid_bytes(2000) > lib.sgr_nn_grid_bytes(1000)
    assert lib.sgr_surface_sample_bytes(5000) >= 2 * 5000 * 8
    assert lib.sgr_eval_reduce_bytes() >= 17 * 8


def test_entry_points_refuse_bad_arguments_before_any_launch():
    from splat_slam_amd import _native as nat
    lib = nat.lib()
    assert lib.sgr_nn_grid_build(0, None, None, None, 0, None) == nat.SGR_ERR_INVALID
    assert "nn_grid_build" in nat.last_error()
    assert lib.sgr_nn_query(10, None, 0, 5, None, None, 1.0, None, None, None) == nat.SGR_ERR_INVALID
    assert lib.sgr_surface_sample(0, 1, None, None, 1, 0, None, 0, None, None, None, None) == nat.SGR_ERR_INVALID
    assert lib.sgr_cloud_metrics(1, None, 1, None, 0.05, None, None, 0, None) == nat.SGR_ERR_INVALID
    buf = ctypes.create_string_buffer(16)
    assert lib.sgr_icp_accumulate(0, None, None, None, 5, ctypes.addressof(buf), ctypes.addressof(buf), ctypes.addressof(buf), 16,
                                  None) == nat.SGR_ERR_WORKSPACE


# ---- PLY input
def _header(fmt, nv, nf, vprops, flist="property list uchar int vertex_indices", extra=""):
    return ("ply\nformat %s 1.0\ncomment test\nelement vertex %d\n%s\nelement face %d\n%s\n%send_header\n"
            % (fmt, nv, "\n".join(vprops), nf, flist, extra)).encode("ascii")


V4 = np.array([[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0], [0.5, 1.5, 0.25]], np.float32)
POLYS = [[0, 1, 2], [0, 2, 3], [0, 1, 2, 3], [0, 1, 2, 4, 3]]
WANT = [[0, 1, 2], [0, 2, 3], [0, 1, 2], [0, 2, 3], [0, 1, 2], [0, 2, 4], [0, 4, 3]]


def _binary(bo, path, idx_type=("uchar", "B", "int", "i"), polys=POLYS, trailing=False):
    props = ["property float x", "property double nx", "property float y", "property float z", "property uchar red",
             "property uchar green", "property uchar blue", "property uchar alpha"]
    ct, cf, it, fi = idx_type
    extra = "element edge 1\nproperty int vertex1\nproperty int vertex2\n" if trailing else ""
    data = _header("binary_%s_endian" % ("little" if bo == "<" else "big"), len(V4), len(polys), props,
                   "property list %s %s vertex_indices" % (ct, it), extra)
    for k, p in enumerate(V4):
        data += struct.pack(bo + "fdffBBBB", p[0], 0.5, p[1], p[2], 10 * k, 20, 255, 7)
    for poly in polys:
        data += struct.pack(bo + cf + fi * len(poly), len(poly), *poly)
    if trailing:
        data += struct.pack(bo + "ii", 0, 1)
    open(path, "wb").write(data)


@pytest.mark.parametrize("bo", ["<", ">"])
@pytest.mark.parametrize("idx_type", [("uchar", "B", "int", "i"), ("uint", "I", "uint", "I"), ("ushort", "H", "short", "h")])
def test_read_binary_ply_with_extra_properties_and_polygons(tmp_path, bo, idx_type):
    from splat_slam_amd.mesh_eval import read_mesh_ply
    path = str(tmp_path / "m.ply")
    _binary(bo, path, idx_type, trailing=True)
    m = read_mesh_ply(path)
    assert m.vertices.dtype == torch.float32 and m.triangles.dtype == torch.int32
    assert np.array_equal(m.vertices.numpy(), V4)
    assert m.triangles.tolist() == WANT
    assert np.allclose(m.vertex_colors.numpy()[:, 0], 10 * np.arange(5) / 255.0) and np.allclose(m.vertex_colors.numpy()[:, 2], 1.0)


@pytest.mark.parametrize("bo", ["<", ">"])
def test_read_binary_ply_triangles_only_takes_the_vectorised_path(tmp_path, bo):
    from splat_slam_amd.mesh_eval import read_mesh_ply
    path = str(tmp_path / "t.ply")
    rng = np.random.default_rng(0)
    tris = rng.integers(0, 5, size=(50, 3)).tolist()
    _binary(bo, path, polys=tris, trailing=True)
    assert read_mesh_ply(path).triangles.tolist() == tris


def test_read_ascii_ply(tmp_path):
    from splat_slam_amd.mesh_eval import read_mesh_ply
    lines = ["ply", "format ascii 1.0", "element vertex 5", "property float x", "property float y", "property float z",
             "property float nx", "property float red", "property float green", "property float blue", "element face 4",
             "property list uchar int vertex_index", "element material 1", "property float k", "end_header"]
    for k, p in enumerate(V4):
        lines.append("%r %r %r 0.0 %r 0.5 0.25" % (float(p[0]), float(p[1]), float(p[2]), 0.1 * k))
    for poly in POLYS:
        lines.append(" ".join(map(str, [len(poly)] + poly)))
    lines.append("3.5")
    path = str(tmp_path / "a.ply")
    open(path, "w").write("\n".join(lines) + "\n")
    m = read_mesh_ply(path)
    assert np.array_equal(m.vertices.numpy(), V4)
    assert m.triangles.tolist() == WANT
    assert np.allclose(m.vertex_colors.numpy()[:, 0], 0.1 * np.arange(5)) and np.allclose(m.vertex_colors.numpy()[:, 1], 0.5)


def test_read_mesh_ply_matches_read_ply_on_what_write_ply_writes(tmp_path):
    from splat_slam_amd.mesh import TriangleMesh
    from splat_slam_amd.mesh_eval import read_mesh_ply
    g = torch.Generator().manual_seed(1)
    m = TriangleMesh(torch.rand(40, 3, generator=g), torch.randint(0, 40, (60, 3), generator=g, dtype=torch.int32),
                     torch.rand(40, 3, generator=g))
    path = str(tmp_path / "w.ply")
    m.write_ply(path)
    a, b = TriangleMesh.read_ply(path), read_mesh_ply(path)
    assert torch.equal(a.vertices, b.vertices) and torch.equal(a.triangles, b.triangles)
    assert torch.allclose(a.vertex_colors, b.vertex_colors, atol=1e-7)


def test_read_mesh_ply_refuses_broken_files(tmp_path):
    from splat_slam_amd.mesh_eval import read_mesh_ply
    path = str(tmp_path / "bad.ply")
    open(path, "wb").write(b"not a ply")
    with pytest.raises(ValueError):
        read_mesh_ply(path)
    _binary("<", path, polys=[[0, 1, 9]])
    with pytest.raises(ValueError, match="outside"):
        read_mesh_ply(path)


# ---- argument checks
def test_mesh_eval_refuses_cpu_tensors_and_bad_arguments():
    from splat_slam_amd.mesh import TriangleMesh
    from splat_slam_amd.mesh_eval import PointGrid, evaluate_mesh, sample_surface
    v = torch.rand(4, 3)
    t = torch.tensor([[0, 1, 2], [1, 2, 3]], dtype=torch.int32)
    m = TriangleMesh(v, t, v.clone())
    with pytest.raises(RuntimeError, match="GPU"):
        sample_surface(m, 10)
    with pytest.raises(RuntimeError, match="GPU"):
        PointGrid(v)
    with pytest.raises(RuntimeError, match="GPU"):
        evaluate_mesh(m, m)
    with pytest.raises(ValueError, match="samples"):
        evaluate_mesh(m, m, samples=0)
    with pytest.raises(ValueError, match="samples"):
        evaluate_mesh(m, m, samples=-5)
    with pytest.raises(ValueError, match="distance_thresh"):
        evaluate_mesh(m, m, distance_thresh=0.0)
    with pytest.raises(ValueError, match="distance_thresh"):
        evaluate_mesh(m, m, distance_thresh=-1.0)
    with pytest.raises(ValueError, match="n must be"):
        sample_surface(m, 0)


def test_mesh_checks_refuse_empty_meshes_and_bad_indices_before_the_device(monkeypatch):
    """_check_mesh's host-side checks, on host tensors with the GPU check lifted"""
    from splat_slam_amd import mesh_eval as me
    from splat_slam_amd.mesh import TriangleMesh
    monkeypatch.setattr(me, "_need_gpu", lambda *a: None)
    v = torch.rand(4, 3)
    with pytest.raises(ValueError, match="empty"):
        me._check_mesh(TriangleMesh(v, torch.zeros(0, 3, dtype=torch.int32), v), "x")
    with pytest.raises(ValueError, match="empty"):
        me._check_mesh(TriangleMesh(torch.zeros(0, 3), torch.zeros(0, 3, dtype=torch.int32), torch.zeros(0, 3)), "x")
    with pytest.raises(ValueError, match="outside"):
        me._check_mesh(TriangleMesh(v, torch.tensor([[0, 1, 4]], dtype=torch.int32), v), "x")
    with pytest.raises(ValueError, match="outside"):
        me._check_mesh(TriangleMesh(v, torch.tensor([[0, -1, 2]], dtype=torch.int32), v), "x")


def test_eval_rendering_without_a_ground_truth_mesh_raises_nothing_new():
    """what eval_rendering refuses is unchanged: the new arguments add nothing before the GPU check"""
    from splat_slam_amd.eval import eval_rendering
    frame = types.SimpleNamespace(original_image=torch.zeros(3, 4, 4))
    with pytest.raises(RuntimeError, match="GPU tensors"):
        eval_rendering([frame], None, None, None, mesh=True)
    with pytest.raises(ValueError, match="no frames"):
        eval_rendering([], None, None, None, mesh=True)


# ---- the restatement
def _plane(z, n=21, step=0.05):
    i, j = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    return np.stack([i.ravel() * step, j.ravel() * step, np.full(n * n, z)], 1)


def test_restated_metrics_of_two_parallel_planes():
    a, b = _plane(0.0), _plane(0.03)
    d_ab, _ = ref.nearest(a, b)
    d_ba, _ = ref.nearest(b, a)
    m = ref.metrics(d_ab, d_ba, 0.05)
    assert abs(m["accuracy"] - 0.03) < 1e-12 and abs(m["completion"] - 0.03) < 1e-12
    assert m["completion_ratio"] == 1.0 and m["precision"] == 1.0 and m["fscore"] == 1.0
    m = ref.metrics(d_ab, d_ba, 0.02)
    assert m["completion_ratio"] == 0.0 and m["precision"] == 0.0 and m["fscore"] == 0.0
    assert abs(m["chamfer_l1"] - 0.03) < 1e-12


def test_restated_nearest_breaks_ties_by_the_smallest_index():
    t = np.array([[1.0, 0, 0], [0, 0, 0], [1.0, 0, 0], [0, 0, 0]])
    d, i = ref.nearest(np.array([[0.9, 0, 0], [0.1, 0, 0]]), t)
    assert i.tolist() == [0, 1] and np.allclose(d, [0.1, 0.1])
    big = ref.nearest_large(np.random.default_rng(0).random((500, 3)), np.random.default_rng(1).random((800, 3)))
    if big is not None:
        d0, _ = ref.nearest(np.random.default_rng(0).random((500, 3)), np.random.default_rng(1).random((800, 3)))
        assert np.allclose(big[0], d0, rtol=0, atol=1e-12)


def test_restated_kabsch_recovers_a_transform_and_guards_reflections():
    rng = np.random.default_rng(2)
    p = rng.normal(size=(200, 3))
    R = ref.rotation((0.3, -0.5, 0.8), 17.0)
    t = np.array([0.1, -0.2, 0.3])
    R1, t1 = ref.kabsch(p, p @ R.T + t)
    assert np.abs(R1 - R).max() < 1e-12 and np.abs(t1 - t).max() < 1e-12
    # a mirrored target: the best proper rotation, never a reflection
    M = np.diag([1.0, 1.0, -1.0])
    R2, _ = ref.kabsch(p, p @ M.T)
    assert abs(np.linalg.det(R2) - 1.0) < 1e-12
    # a planar cloud mirrored across its own plane is fitted exactly by a rotation
    pl = p.copy()
    pl[:, 2] = 0.0
    R3, t3 = ref.kabsch(pl, pl @ M.T)
    assert abs(np.linalg.det(R3) - 1.0) < 1e-12 and np.abs(pl @ R3.T + t3 - pl @ M.T).max() < 1e-12


def test_restated_icp_recovers_a_small_motion():
    rng = np.random.default_rng(3)
    v, t = ref.room_mesh(8)
    pts = v[t].mean(1)
    pts = np.concatenate([pts, v])
    R = ref.rotation((1.0, 2.0, -0.5), 1.5)
    moved = (pts @ R.T + np.array([0.02, -0.01, 0.015])).astype(np.float32)
    res = ref.icp(moved, pts + rng.normal(scale=1e-4, size=pts.shape), max_dist=0.2)
    back = ref.transform(res["transformation"], moved)
    assert np.abs(back - pts).max() < 5e-3, np.abs(back - pts).max()
    assert res["fitness"] == 1.0 and 1 <= res["iterations"] <= 30
