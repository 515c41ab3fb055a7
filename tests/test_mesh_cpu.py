"""The TSDF mesh without a GPU: the generated marching-cubes table (csrc/sgr_mc_table.h) is what scripts/gen_mc_table.py writes
and cannot crack, the fp64 restatement (tests/mesh_ref.py) fuses an analytic sphere into one closed genus-0 surface,
csrc/sgr_mesh.hip compiles for gfx950 without scratch, spills or float atomics, and splat_slam_amd.mesh refuses what it does not
implement."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

import mesh_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
KERNELS = ("tsdf_touch_kernel", "tsdf_list_kernel", "tsdf_rehash_kernel", "tsdf_integrate_kernel", "scan_blocks_kernel",
           "scan_sums_kernel", "scan_add_kernel", "gather_units_kernel", "bitonic_step_kernel", "mc_count_kernel", "mc_emit_kernel",
           "cc_init_kernel", "cc_union_kernel", "cc_flatten_kernel", "cc_keep_vertices_kernel", "tri_keep_kernel",
           "tri_bucket_kernel", "tri_dedup_kernel", "compact_vertices_kernel", "compact_triangles_kernel")


# ---- the table
def test_regenerating_the_table_reproduces_the_header():
    gen = ref.load_generator()
    assert open(gen.OUT).read() == gen.render()


def _sign_edges(case):
    return {e for e, (a, b) in enumerate(ref.EDGES) if ((case >> a) & 1) != ((case >> b) & 1)}


def test_every_triangle_vertex_is_on_a_sign_change_and_every_sign_change_is_used():
    for case in range(256):
        used = {e for tri in ref.TABLE[case] for e in tri}
        assert used == _sign_edges(case), case
        for tri in ref.TABLE[case]:
            assert len(set(tri)) == 3, (case, tri)


def _face_of_edge_pair(a, b):
    """the cube face holding both edges, as (axis, side), or None"""
    ca = {c for c in ref.EDGES[a]}
    cb = {c for c in ref.EDGES[b]}
    corners = ca | cb
    for axis in range(3):
        for side in (0, 1):
            if all(ref.CORNERS[c][axis] == side for c in corners):
                return axis, side
    return None


def _boundary(case):
    """directed edges used once by the case's triangles (an undirected pair used twice is interior)"""
    cnt = {}
    for a, b, c in ref.TABLE[case]:
        for e in ((a, b), (b, c), (c, a)):
            cnt[e] = cnt.get(e, 0) + 1
    return [e for e in cnt if (e[1], e[0]) not in cnt]


def _face_signs(case, axis, side):
    return tuple(sorted((ref.CORNERS[c], (case >> c) & 1) for c in range(8) if ref.CORNERS[c][axis] == side))


def _edge_corners(e):
    return tuple(sorted(ref.CORNERS[c] for c in ref.EDGES[e]))


def test_triangle_boundaries_lie_on_faces_and_match_across_shared_faces():
    # per case, boundary segments grouped by face, as geometric edges (pairs of corner positions)
    seg = {}
    for case in range(256):
        faces = {}
        for a, b in _boundary(case):
            f = _face_of_edge_pair(a, b)
            assert f is not None, (case, a, b)            # a boundary edge runs across one cube face
            faces.setdefault(f, []).append((_edge_corners(a), _edge_corners(b)))
        seg[case] = faces
    # the segments on a face depend only on that face's four corner signs
    by_signs = {}
    for case in range(256):
        for axis in range(3):
            for side in (0, 1):
                key = (axis, side, _face_signs(case, axis, side))
                got = sorted(seg[case].get((axis, side), []))
                assert by_signs.setdefault(key, got) == got, (case, axis, side)
    # the neighbour across face (axis, 1) sees it as its face (axis, 0), shifted by one along axis: same segments, reversed
    for case in range(256):
        for axis in range(3):
            mine = seg[case].get((axis, 1), [])
            face_signs = {c: (case >> c) & 1 for c in range(8) if ref.CORNERS[c][axis] == 1}
            for other in range(256):
                o_signs = {c: (other >> c) & 1 for c in range(8) if ref.CORNERS[c][axis] == 0}
                match = all(face_signs[c] == o_signs[d] for c in face_signs for d in o_signs
                            if all(ref.CORNERS[c][k] == ref.CORNERS[d][k] for k in range(3) if k != axis))
                if not match:
                    continue
                shift = lambda p: tuple(p[k] + (1 if k == axis else 0) for k in range(3))
                theirs = sorted((tuple(sorted(map(shift, b))), tuple(sorted(map(shift, a)))) for a, b in seg[other].get((axis, 0), []))
                assert sorted(mine) == theirs, (case, other, axis)
                break


# ---- the restatement on an analytic sphere
def test_restated_fusion_of_a_sphere_is_one_closed_genus_zero_surface():
    # sdf_trunc of three voxels: at two, cubes seen only at grazing angles keep an unobserved corner (sdf along the ray < -trunc)
    # and leave the surface open there, as the fusion would
    r, vl = 0.3, 0.02
    frames = ref.sphere_views(14, r, 160, 120, 200.0, 1.0, centre=(0.013, -0.021, 0.007))
    vol = ref.RefVolume(vl, 0.06)
    for fr in frames:
        vol.integrate(fr)
    v, t, c = ref.extract(vol.arrays(), vl)
    v, t, c, _ = ref.clean(v, t, c, 100)
    assert len(v) > 1000 and len(t) > 2000
    lab = ref.components(len(v), t)
    assert len(np.unique(lab)) == 1
    assert ref.closed_and_oriented(t)
    assert ref.euler(len(v), t) == 2
    dist = np.abs(np.linalg.norm(v - np.array([0.013, -0.021, 0.007]), axis=1) - r)
    assert dist.max() <= 0.5 * vl, dist.max()
    # triangles face from T < 0 (inside) toward T > 0: normals point away from the centre
    n = np.cross(v[t[:, 1]] - v[t[:, 0]], v[t[:, 2]] - v[t[:, 0]])
    out = v[t].mean(1) - np.array([0.013, -0.021, 0.007])
    assert ((n * out).sum(1) > 0).mean() > 0.99


def test_restated_cleaning_drops_small_components():
    verts = np.random.default_rng(0).normal(size=(9, 3))
    tris = np.array([[0, 1, 2], [1, 2, 3], [4, 5, 6], [1, 2, 3], [0, 0, 1]])
    v, t, c, vmap = ref.clean(verts, tris, verts, min_len=4)
    assert (vmap[:4] == np.arange(4)).all() and (vmap[4:] == -1).all()
    assert t.tolist() == [[0, 1, 2], [1, 2, 3]]


# ---- ISA budget
@pytest.fixture(scope="module")
def mesh_isa(tmp_path_factory):
    if not (os.path.exists(HIPCC) or shutil.which(HIPCC)):
        pytest.skip("hipcc not available")
    out = str(tmp_path_factory.mktemp("isa") / "mesh.s")
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-S", "--cuda-device-only", "-o", out,
                    os.path.join(ROOT, "splat_slam_amd", "csrc", "sgr_mesh.hip")], check=True, capture_output=True)
    text = open(out).read()
    meta = {}
    for block in text.split("\n  - ")[1:]:
        m = re.search(r"\.name:\s+(\S+)", block)
        if m and ".private_segment_fixed_size" in block:
            meta[m.group(1)] = block
    return text, meta


def test_every_mesh_kernel_has_no_scratch_no_spills_and_no_float_atomics(mesh_isa):
    text, meta = mesh_isa
    for k in KERNELS:
        names = [n for n in meta if re.search(r"\d%s" % k, n)]
        assert len(names) == 1, (k, sorted(meta))
        block = meta[names[0]]
        scratch = int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", block).group(1))
        spill = int(re.search(r"\.vgpr_spill_count:\s+(\d+)", block).group(1))
        assert scratch == 0 and spill == 0, (k, scratch, spill)
    assert len(meta) == len(KERNELS), sorted(meta)
    # float atomics of any width or packing (v_pk_add_f32 is a plain VALU add, not an atomic)
    assert not re.search(r"(global|flat|buffer|ds)_atomic_\w*(f32|f64|pk_add)", text)
    assert not re.search(r"(global|flat|buffer)_atomic_pk_add", text)


# ---- argument checks
def test_mesh_api_refuses_cpu_tensors_wrong_shapes_and_min_len():
    from splat_slam_amd.mesh import TriangleMesh, TSDFVolume, clean_mesh
    v = torch.zeros(4, 3)
    t = torch.tensor([[0, 1, 2], [1, 2, 3]], dtype=torch.int32)
    with pytest.raises(RuntimeError, match="GPU"):
        clean_mesh(TriangleMesh(v, t, v.clone()))
    with pytest.raises(ValueError, match="min_len"):
        clean_mesh(TriangleMesh(v, t, v.clone()), min_len=0)
    with pytest.raises(RuntimeError, match="GPU"):
        TSDFVolume(device="cpu")
    with pytest.raises(RuntimeError, match="GPU"):
        clean_mesh(TriangleMesh(v[:, :2], t, v.clone()))
    from splat_slam_amd.eval import eval_rendering
    with pytest.raises(RuntimeError, match="GPU tensors"):
        import types
        eval_rendering([types.SimpleNamespace(original_image=torch.zeros(3, 4, 4))], None, None, None, mesh=True)


def test_ply_round_trip_on_the_host(tmp_path):
    from splat_slam_amd.mesh import TriangleMesh
    g = torch.Generator().manual_seed(0)
    v = torch.rand(10, 3, generator=g)
    c = torch.rand(10, 3, generator=g)
    t = torch.randint(0, 10, (7, 3), generator=g, dtype=torch.int32)
    m = TriangleMesh(v, t, c)
    m.write_ply(str(tmp_path / "m.ply"))
    r = TriangleMesh.read_ply(str(tmp_path / "m.ply"))
    assert torch.equal(r.vertices, v) and torch.equal(r.triangles, t)
    assert (r.vertex_colors - c).abs().max() <= 0.5 / 255 + 1e-7
