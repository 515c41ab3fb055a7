"""-m gpu: mesh culling on the HIP kernels (splat_slam_amd.mesh_cull, csrc/sgr_mesh_cull.hip) against the restatement of
tests/mesh_cull_ref.py: the projection in every integer and bit, the z-buffer in its exact coverage and to a few ulp in depth, the
visibility count and the selection exactly, and cull_mesh / eval_rendering end to end."""
import numpy as np
import pytest
import torch

import mesh_cull_ref as ref
import mesh_eval_ref as eref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
H0, W0 = 48, 64                 # the image of ref.INTR


def _mesh(v, t):
    from splat_slam_amd.mesh import TriangleMesh
    v = torch.from_numpy(np.ascontiguousarray(v, dtype=np.float32)).to(DEV)
    c = (v - v.min()) / (v.max() - v.min())                     # colours that tell the vertices apart
    return TriangleMesh(v, torch.from_numpy(np.ascontiguousarray(t, dtype=np.int32)).to(DEV), c.contiguous())


def _np(t):
    return t.cpu().numpy()


# ---- projection
@pytest.mark.parametrize("name", sorted(ref.project_inputs()))
def test_projection_equals_the_restatement_in_every_integer_and_bit(name):
    """the room with vertices behind the camera, either side of near and of the guard, NaN and inf; 1, 16 and 17 frames (the last
    through the chunking of vertex_visibility's layer); own and shared intrinsics.  tests/test_mesh_cull_cpu.py verifies that none
    of these inputs sits within 1e-9 of a rounding tie: nothing is excluded."""
    from splat_slam_amd import mesh_cull as mc
    v, c2w, intr = ref.project_inputs()[name]
    vt = torch.from_numpy(v).to(DEV)
    xs, zs = [], []
    for _, w2c, k in mc._chunks(c2w, intr[:, 0], intr[:, 1], intr[:, 2], intr[:, 3]):
        assert len(w2c) <= 16
        xy, z = mc.project(vt, w2c, k, 0.01)
        xs.append(_np(xy))
        zs.append(_np(z))
    xy, z = np.concatenate(xs), np.concatenate(zs)
    want_xy, want_z = ref.project(v, ref.invert(c2w), intr, 0.01)
    assert xy.shape == want_xy.shape == (len(c2w), len(v), 2)
    assert np.array_equal(xy, want_xy)
    assert np.array_equal(z.view(np.uint32), want_z.view(np.uint32))
    valid = want_z > 0
    assert valid.any() and not valid.all() and not xy[~valid].any()
    if name.startswith("n"):        # the hand-placed vertices, for camera 0: behind, under / over near, inside / outside the guard
        assert valid[0, -11:].tolist() == [False, False, True, True, False, True, False, False, False, False, False]


# ---- z-buffer
def _raster(xy, z, tris, H, W):
    from splat_slam_amd import mesh_cull as mc
    V = np.asarray(z).shape[-1]
    xy = torch.from_numpy(np.ascontiguousarray(xy, dtype=np.int32)).to(DEV).reshape(-1, V, 2)
    zt = torch.from_numpy(np.ascontiguousarray(z, dtype=np.float32)).to(DEV).reshape(-1, V)
    depth, skipped = mc.rasterize(xy, zt, torch.from_numpy(np.ascontiguousarray(tris, dtype=np.int32)).to(DEV), H, W)
    return _np(depth), _np(skipped)


def _assert_depth(got, want):
    """The finite mask is exact: coverage is integer arithmetic on both sides.  The depth: with u = 2^-24, the kernel rounds each
    edge function to fp32 (1 + u), multiplies by the rounded reciprocal of z (two more), adds the three non-negative terms (two
    more: a sum of non-negative terms inherits the largest relative error of a term, nothing cancels), rounds A and divides (two
    more): (1 + u)^7 - 1 < 2^-21.1.  A reciprocal or division good to 2.5 ulp instead of 0.5 adds 6 u.  The restatement's fp64 error
    is 2^-50.  The minimum over triangles keeps the bound.  2^-19 = 32 u holds all of it; no pixel is excluded."""
    mask = np.isfinite(want)
    assert np.array_equal(np.isfinite(got), mask)
    assert np.all(got[~mask] == np.inf)
    g, w = got[mask].astype(np.float64), want[mask]
    assert np.all(np.abs(g - w) <= 2.0 ** -19 * w), np.max(np.abs(g - w) / w) * 2 ** 24


@pytest.mark.parametrize("size", [(37, 53), (48, 64)])
def test_raster_of_hand_written_coordinates(size):
    H, W = size
    rng = np.random.default_rng(7)
    for name, (xy, z, tris) in ref.raster_cases(H, W).items():
        want, want_skipped = ref.raster(xy, z, tris, H, W)
        got, skipped = _raster(xy, z, tris, H, W)
        assert got.shape == (1, H, W) and got.dtype == np.float32, name
        _assert_depth(got[0], want)
        assert skipped.tolist() == [want_skipped], name
        # twice, and with the triangles permuted: the same bits
        again, _ = _raster(xy, z, tris, H, W)
        perm, _ = _raster(xy, z, tris[rng.permutation(len(tris))], H, W)
        assert np.array_equal(got.view(np.uint32), again.view(np.uint32)), name
        assert np.array_equal(got.view(np.uint32), perm.view(np.uint32)), name
        if name == "tessellated_plane":
            (i0, i1), (j0, j1) = ref.plane_interior(H, W)
            assert np.isfinite(got[0, i0:i1 + 1, j0:j1 + 1]).all()
        if name == "zero_area":
            assert not np.isfinite(got).any()
        if name == "whole_image":
            assert np.isfinite(got).all()


def test_raster_keeps_its_frames_apart():
    """three frames of one call: the plane shifted by a different amount in each, one of them with an invalid vertex"""
    H, W = 37, 53
    xy, z, tris = ref.raster_cases(H, W)["tessellated_plane"]
    shifts = [(0, 0), (5 * ref.SUB + 37, -3 * ref.SUB - 11), (-7 * ref.SUB + 101, 4 * ref.SUB + 3)]
    xys = np.stack([xy + np.asarray(s) for s in shifts])
    zs = np.stack([z, z * 2, z + 1])
    zs[2, 5] = 0.0
    got, skipped = _raster(xys, zs, tris, H, W)
    for f in range(3):
        want, s = ref.raster(xys[f], zs[f], tris, H, W)
        _assert_depth(got[f], want)
        assert skipped[f] == s
    assert skipped.tolist()[:2] == [0, 0] and skipped[2] > 0


# ---- visibility
@pytest.fixture(scope="module")
def room32():
    """room_mesh(32) under 17 cameras inside the room: per chunk of 16, the kernel's own coordinates and depth"""
    from splat_slam_amd import mesh_cull as mc
    v, t = eref.room_mesh(32)
    mesh = _mesh(v, t)
    c2w, intr = ref.room_cameras(17), ref.room_intrinsics(17)
    chunks = []
    for _, w2c, k in mc._chunks(c2w, intr[:, 0], intr[:, 1], intr[:, 2], intr[:, 3]):
        xy, z = mc.project(mesh.vertices, w2c, k, 0.01)
        depth, skipped = mc.rasterize(xy, z, mesh.triangles, H0, W0)
        chunks.append((xy, z, depth, skipped))
    return mesh, c2w, intr, chunks


def _ref_seen(chunks, frames, use_depth, depths=None, **kw):
    """the restatement's count over the first `frames` frames of the chunks, from the kernel's coordinates"""
    total, f0 = 0, 0
    for xy, z, depth, _ in chunks:
        n = min(len(z), frames - f0)
        if n <= 0:
            break
        d = None
        if depths is not None:
            d = depths[f0:f0 + n]
        elif use_depth:
            d = _np(depth)[:n]
        total = total + ref.visibility(_np(xy)[:n], _np(z)[:n], d, H0, W0, **kw)
        f0 += n
    return total


@pytest.mark.parametrize("frames", [6, 17])
@pytest.mark.parametrize("occlusion", [None, "mesh"])
def test_visibility_equals_the_restatement(room32, frames, occlusion):
    """six cameras, and 17: one more than a chunk, so the second chunk adds to the first one's counts"""
    from splat_slam_amd import mesh_cull as mc
    mesh, c2w, intr, chunks = room32
    for kw in (dict(), dict(edge=5), dict(far=2.2), dict(edge=5, far=1.7, occlusion_eps=0.002)):
        seen = _np(mc.vertex_visibility(mesh, c2w[:frames], intr[:frames], H0, W0, occlusion=occlusion, **kw))
        rkw = {("eps" if k == "occlusion_eps" else k): v for k, v in kw.items()}
        want = _ref_seen(chunks, frames, occlusion == "mesh", **rkw)
        assert seen.dtype == np.int32 and np.array_equal(seen, want), kw
        assert 0 < (seen > 0).sum() < len(seen) and seen.max() <= frames
    if occlusion == "mesh":         # occlusion removes something the frustum keeps
        frustum = _np(mc.vertex_visibility(mesh, c2w[:frames], intr[:frames], H0, W0, occlusion=None))
        assert np.all(seen <= frustum) and (_np(mc.vertex_visibility(mesh, c2w[:frames], intr[:frames], H0, W0)) < frustum).any()


def test_visibility_with_supplied_depth_maps_and_their_holes(room32):
    from splat_slam_amd import mesh_cull as mc
    mesh, c2w, intr, chunks = room32
    depths = np.concatenate([_np(c[2]) for c in chunks])
    depths[:, :, :9] = 0.0                                      # sensor holes
    depths[:, 10:20, 20:30] = np.nan
    depths[:, 30:40, 40:50] = -1.0
    depths[:, 25:35, 10:18] = np.inf
    depths[:, 5:15, 50:60] *= 0.5                               # something in front of the mesh: those vertices are occluded
    d = torch.from_numpy(depths).to(DEV)
    seen = _np(mc.vertex_visibility(mesh, c2w, intr, H0, W0, occlusion=d))
    want = _ref_seen(chunks, 17, True, depths=depths)
    assert np.array_equal(seen, want)
    plain = _ref_seen(chunks, 17, True)
    frustum = _ref_seen(chunks, 17, False)
    assert (seen > plain).any() and (seen < plain).any() and np.all(seen <= frustum)


def test_render_mesh_depth_is_the_chunks_depth(room32):
    from splat_slam_amd import mesh_cull as mc
    mesh, c2w, intr, chunks = room32
    depth, skipped = mc.render_mesh_depth(mesh, c2w, intr[:, 0], intr[:, 1], intr[:, 2], intr[:, 3], H0, W0)
    assert tuple(depth.shape) == (17, H0, W0) and tuple(skipped.shape) == (17,)
    assert torch.equal(depth.view(torch.int32), torch.cat([c[2] for c in chunks]).view(torch.int32))
    assert torch.equal(skipped, torch.cat([c[3] for c in chunks]))
    assert bool(torch.isfinite(depth).all())                    # cameras inside a closed room: every pixel hits something
    # against the restatement's rasteriser, one frame
    xy, z = _np(chunks[0][0])[3], _np(chunks[0][1])[3]
    want, s = ref.raster(xy, z, _np(mesh.triangles), H0, W0)
    _assert_depth(_np(depth)[3], want)
    assert int(skipped[3]) == s and s > 0                       # the walls behind the camera


# ---- selection
@pytest.mark.parametrize("rule", ["all", "any"])
@pytest.mark.parametrize("min_views", [1, 2])
def test_selection_equals_the_restatement(rule, min_views):
    from splat_slam_amd import mesh_cull as mc
    v, t = eref.room_mesh(24)                                   # 5 618 vertices, 10 368 faces: more than one scan block
    mesh = _mesh(v, t)
    rng = np.random.default_rng(11)
    seen = rng.integers(0, 4, len(v)).astype(np.int32)
    seen[1000:3000] = 0                                         # a dropped stretch
    seen[4000:5000] = 3
    out, vmap = mc.select(mesh, torch.from_numpy(seen).to(DEV), min_views, rule)
    kv, kf, faces, want_map = ref.select(len(v), t, seen, min_views, rule)
    assert 0 < len(kf) < len(t) and 0 < len(kv) < len(v)
    assert np.array_equal(_np(vmap), want_map)
    assert np.array_equal(_np(out.triangles), faces)
    assert np.array_equal(_np(out.vertices), _np(mesh.vertices)[kv])
    assert np.array_equal(_np(out.vertex_colors), _np(mesh.vertex_colors)[kv])


def test_selection_that_keeps_everything_and_nothing():
    from splat_slam_amd import mesh_cull as mc
    v, t = eref.room_mesh(8)
    mesh = _mesh(v, t)
    out, vmap = mc.select(mesh, torch.ones(len(v), dtype=torch.int32, device=DEV))
    assert torch.equal(out.vertices, mesh.vertices) and torch.equal(out.triangles, mesh.triangles)
    assert torch.equal(out.vertex_colors, mesh.vertex_colors) and vmap.tolist() == list(range(len(v)))
    out, vmap = mc.select(mesh, torch.ones(len(v), dtype=torch.int32, device=DEV), min_views=2)
    assert tuple(out.vertices.shape) == (0, 3) and tuple(out.triangles.shape) == (0, 3) and bool((vmap == -1).all())
    from splat_slam_amd.mesh import TriangleMesh                # a mesh without faces
    out, vmap = mc.select(TriangleMesh(mesh.vertices, mesh.triangles[:0], mesh.vertex_colors),
                          torch.ones(len(v), dtype=torch.int32, device=DEV))
    assert len(out) == 0 and out.triangles.shape[0] == 0 and bool((vmap == -1).all())


@pytest.mark.parametrize("V,F", [(0, 0), (1, 1), (4096, 4095), (4097, 4097)])
def test_selection_of_every_second_face_at_the_scan_block_edges(V, F):
    """sgr_cull_select + sgr_cull_compact straight on the C ABI (mesh_cull.select refuses a mesh without vertices) around the 4096-item
    block of the device-wide scan that the culling shares with the mesh cleaning: an empty mesh, one face, one item short of a block
    and one past it.  Face f joins vertices of its own parity (f, f - 2, f - 4; no wrap), and only even vertices were seen, so under
    either rule exactly the faces 0, 2, 4, ... stay, with the even vertices."""
    from splat_slam_amd import _native as nat
    from splat_slam_amd.mesh_cull import RULES
    lib = nat.lib()
    f = np.arange(F, dtype=np.int64)
    t = np.stack([f, np.where(f >= 2, f - 2, f), np.where(f >= 4, f - 4, f)], 1).astype(np.int32).reshape(F, 3)
    seen = (np.arange(V) % 2 == 0).astype(np.int32)
    rng = np.random.default_rng(V + 1)
    v, c = rng.standard_normal((V, 3)).astype(np.float32), rng.random((V, 3)).astype(np.float32)
    kv, kf, faces, want_map = ref.select(V, t, seen, 1, "all")
    assert np.array_equal(kf, np.arange(0, F, 2)) and np.array_equal(kv, np.arange(0, V, 2))
    dv, dc, dt, ds = (torch.from_numpy(a).to(DEV) for a in (v, c, t, seen))
    st = torch.cuda.current_stream().cuda_stream
    for rule in ("all", "any"):
        nbytes = lib.sgr_cull_select_bytes(V, F)
        scratch = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
        totals = torch.full((2,), -1, dtype=torch.int32, device=DEV)
        nat.check(lib.sgr_cull_select(V, F, dt.data_ptr(), ds.data_ptr(), 1, RULES[rule], scratch.data_ptr(), nbytes, totals.data_ptr(), st),
                  "sgr_cull_select")
        assert totals.tolist() == [len(kv), len(kf)], rule
        ov = torch.empty(len(kv), 3, dtype=torch.float32, device=DEV)
        oc = torch.empty(len(kv), 3, dtype=torch.float32, device=DEV)
        ot = torch.empty(len(kf), 3, dtype=torch.int32, device=DEV)
        vmap = torch.full((V,), -5, dtype=torch.int32, device=DEV)
        nat.check(lib.sgr_cull_compact(V, F, dv.data_ptr(), dc.data_ptr(), dt.data_ptr(), scratch.data_ptr(), nbytes, ov.data_ptr(),
                                       oc.data_ptr(), ot.data_ptr(), vmap.data_ptr(), st), "sgr_cull_compact")
        assert np.array_equal(_np(vmap), want_map), rule
        assert np.array_equal(_np(ot), faces.reshape(-1, 3)), rule
        assert np.array_equal(_np(ov), v[kv]) and np.array_equal(_np(oc), c[kv]), rule


# ---- end to end
SCALE = 5                      # 240 x 320 images


@pytest.fixture(scope="module")
def culled_room():
    from splat_slam_amd import mesh_cull as mc
    v, t = eref.room_mesh(32)
    mesh = _mesh(v, t)
    c2w, intr = ref.room_cameras(6), ref.scaled_intrinsics(6, SCALE)
    out, info = mc.cull_mesh(mesh, c2w, intr, H0 * SCALE, W0 * SCALE, return_info=True)
    return v, t, mesh, c2w, intr, out, info


def test_cull_mesh_drops_what_no_camera_saw(culled_room):
    from splat_slam_amd import mesh_cull as mc
    v, t, mesh, c2w, intr, out, info = culled_room
    H, W = H0 * SCALE, W0 * SCALE
    assert info["vertices_before"] == len(v) and info["faces_before"] == len(t)
    assert info["vertices_after"] == len(out) < len(v) and info["faces_after"] == out.triangles.shape[0] < len(t)
    assert info["unrasterized_triangles"] > 0                   # the walls behind each camera
    seen, vmap = _np(info["seen"]), _np(info["vertex_map"])
    # every kept face has all three vertices seen by the restatement (from the kernel's own coordinates and depth)
    w2c = mc.invert_poses(c2w)
    xy, z = mc.project(mesh.vertices, w2c, intr, 0.01)
    depth, skipped = mc.rasterize(xy, z, mesh.triangles, H, W)
    assert int(skipped.max()) == info["unrasterized_triangles"]
    want_seen = ref.visibility(_np(xy), _np(z), _np(depth), H, W)
    assert np.array_equal(seen, want_seen)
    kv, kf, faces, want_map = ref.select(len(v), t, want_seen, 1, "all")
    assert np.array_equal(vmap, want_map) and np.array_equal(_np(out.triangles), faces)
    assert np.all(want_seen[t[kf]] >= 1)
    # the sides of the inner boxes that face away from every camera are gone.  (Each side has its own vertices; those on its rim
    # coincide with the neighbouring side's and are seen with them, so a face is judged by its vertices inside the rim.)
    checked = ref.assert_hidden_box_sides_are_gone(v, t, kf, c2w[:, :3, 3], 32)
    assert checked >= 4                                         # both bottoms and at least one upright side of each box


def test_scores_against_the_culled_ground_truth_are_complete(culled_room):
    """pred = the culled room.  Against the whole room the completion ratio is below 1: the unseen sides have no prediction near
    them.  Against the room culled by the same cameras it is >= 0.999: the whole room has 68.9 m^2, so 200 000 samples are at least
    2 900 per m^2, a disc of 5 cm radius around a ground-truth sample holds at least 22 predicted samples on average and is empty
    with probability below e^-22."""
    from splat_slam_amd import mesh_cull as mc
    from splat_slam_amd.mesh_eval import evaluate_mesh
    v, t, mesh, c2w, intr, pred, info = culled_room
    whole = evaluate_mesh(pred, mesh, icp_align=False, samples=200_000)
    gt_culled = mc.cull_mesh(mesh, c2w, intr, H0 * SCALE, W0 * SCALE)
    assert torch.equal(gt_culled.triangles, pred.triangles)
    culled = evaluate_mesh(pred, gt_culled, icp_align=False, samples=200_000)
    print("completion ratio: whole room %.4f, culled room %.4f" % (whole["completion_ratio"], culled["completion_ratio"]))
    assert whole["completion_ratio"] < 1.0
    assert culled["completion_ratio"] >= 0.999
    assert culled["completion"] < whole["completion"]


def test_eval_rendering_culls_only_when_asked(tmp_path):
    from splat_slam_amd import synthetic as syn
    from splat_slam_amd.eval import eval_rendering
    from splat_slam_amd.mapper import PipelineParams
    from test_gpu_mesh_eval import _room_session
    sess = _room_session()
    frames = [sess.loop.viewpoints[k] for k in sorted(sess.loop.viewpoints)]
    args = (frames, sess.loop.gaussians, PipelineParams(), sess.loop.background)
    half = np.array(syn.ROOM) / 2
    v, t = eref.box_mesh(-half, half, 24)
    walls = _mesh(v, t)
    today = eval_rendering(*args, mesh=True, gt_mesh_path=walls)
    off = eval_rendering(*args, mesh=True, gt_mesh_path=walls, cull_mesh=False, cull_poses=None)
    assert set(off) == set(today) and "mesh_cull" not in off and "gt_mesh_culled" not in off
    for k in today:
        if k == "mesh":
            assert torch.equal(off[k].vertices, today[k].vertices) and torch.equal(off[k].triangles, today[k].triangles)
        elif k == "mesh_metrics":
            assert {a: b for a, b in off[k].items() if a != "icp"} == {a: b for a, b in today[k].items() if a != "icp"}
            assert np.array_equal(off[k]["icp"]["transformation"], today[k]["icp"]["transformation"])
        else:
            assert off[k] == today[k], k
    path = str(tmp_path / "mesh.ply")
    on = eval_rendering(*args, mesh=True, gt_mesh_path=walls, cull_mesh=True, mesh_path=path)
    assert set(on) == set(today) | {"mesh_cull", "gt_mesh_culled"}
    assert torch.equal(on["mesh"].vertices, today["mesh"].vertices) and torch.equal(on["mesh"].triangles, today["mesh"].triangles)
    from splat_slam_amd.mesh import TriangleMesh
    assert TriangleMesh.read_ply(path).triangles.shape == today["mesh"].triangles.shape      # the PLY is the unculled mesh
    info = on["mesh_cull"]
    assert set(info) == {"pred", "gt"}
    for part in info.values():
        assert set(part) == {"vertices_before", "vertices_after", "faces_before", "faces_after", "unrasterized_triangles"}
        assert all(isinstance(x, int) for x in part.values())
    assert info["gt"]["faces_before"] == len(t) and 0 < info["gt"]["faces_after"] < len(t)
    assert info["pred"]["faces_before"] == today["mesh"].triangles.shape[0] and 0 < info["pred"]["faces_after"] <= info["pred"]["faces_before"]
    assert on["gt_mesh_culled"].triangles.shape[0] == info["gt"]["faces_after"]
    print("completion ratio vs walls: %.4f unculled, %.4f culled" % (today["mesh_metrics"]["completion_ratio"],
                                                                    on["mesh_metrics"]["completion_ratio"]))
    assert on["mesh_metrics"]["completion_ratio"] >= today["mesh_metrics"]["completion_ratio"]
    # explicit poses; and a culled mesh without faces is reported, not raised
    away = torch.eye(4, dtype=torch.float64)
    away[:3, 3] = torch.tensor([100.0, 0.0, 0.0])               # a camera far outside, looking away
    none = eval_rendering(*args, mesh=True, gt_mesh_path=walls, cull_mesh=True, cull_poses=[away])
    assert "mesh_metrics" not in none and "empty" in none["mesh_metrics_error"] and none["mesh_cull"]["gt"]["faces_after"] == 0
