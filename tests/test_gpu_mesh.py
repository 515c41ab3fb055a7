"""-m gpu: TSDF fusion, marching cubes and cleaning on the HIP kernels (splat_slam_amd.mesh, csrc/sgr_mesh.hip) against the fp64
restatement of tests/mesh_ref.py, and the mesh branch of eval_rendering / MappingSession.evaluate."""
import types

import numpy as np
import pytest
import torch

import mesh_ref as ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _dev_frames(frames, exposure=True):
    out = []
    for k, fr in enumerate(frames):
        g = dict(fr)
        g["render"] = torch.from_numpy(fr["render"]).to(DEV)
        g["depth"] = torch.from_numpy(fr["depth"]).to(DEV)
        g["w2c"] = torch.from_numpy(np.asarray(fr["w2c"], dtype=np.float64))
        if "gt_depth" in fr:
            g["gt_depth"] = torch.from_numpy(fr["gt_depth"]).to(DEV)
        if exposure and k > 0:
            g["exposure_a"] = torch.tensor([0.05 * ((k % 5) - 2)], device=DEV)
            g["exposure_b"] = torch.tensor([0.02 * ((k % 3) - 1)], device=DEV)
        out.append(g)
    return out


def _host(fr):
    return {k: (v.cpu().numpy() if torch.is_tensor(v) else v) for k, v in fr.items()}


def _plane_frames(n, W=96, H=72, seed=0):
    """random planes in front of cameras on a small orbit, with a ground-truth depth hole and a random colour image"""
    rng = np.random.default_rng(seed)
    frames = []
    f, cx, cy = 80.0, (W - 1) / 2.0, (H - 1) / 2.0
    for k in range(n):
        ang = 0.2 * k
        Rm = np.array([[np.cos(ang), 0, -np.sin(ang)], [0, 1, 0], [np.sin(ang), 0, np.cos(ang)]])
        w2c = np.eye(4)
        w2c[:3, :3] = Rm
        w2c[:3, 3] = rng.normal(scale=0.05, size=3)
        nrm = np.array([rng.normal(scale=0.3), rng.normal(scale=0.3), 1.0])
        d0 = rng.uniform(0.8, 1.4)
        v, u = np.mgrid[0:H, 0:W].astype(np.float64)
        ray = np.stack([(u - cx) / f, (v - cy) / f, np.ones_like(u)], -1)
        depth = (d0 / (ray @ nrm)).astype(np.float32)
        gt = np.ones((H, W), np.float32)
        gt[H // 3:H // 2, W // 4:W // 2] = 0.0
        render = rng.uniform(0, 1, size=(3, H, W)).astype(np.float32)
        frames.append(dict(render=render, depth=depth, gt_depth=gt, w2c=w2c, fx=f, fy=f, cx=cx, cy=cy, global_scale=1.03))
    return frames


def _sphere_frames(n, W, H, f, r=0.3, centre=(0.013, -0.021, 0.007)):
    return ref.sphere_views(n, r, W, H, f, 1.0, centre=centre)


def _volume(vl, trunc, frames):
    from splat_slam_amd.mesh import TSDFVolume
    vol = TSDFVolume(voxel_length=vl, sdf_trunc=trunc, device=DEV, hash_capacity=256, pool_capacity=8)   # small: both grow
    vol.integrate_frames(frames)
    return vol


def _hip_units(vol):
    return set(map(tuple, vol.voxels()["keys"].cpu().tolist()))


# ---- touched units and integration
@pytest.mark.parametrize("scene", ["planes", "sphere"])
def test_touched_units_equal_the_restatement(scene):
    vl, trunc = (0.02, 0.04) if scene == "planes" else (0.02, 0.06)
    frames = _dev_frames(_plane_frames(6) if scene == "planes" else _sphere_frames(6, 160, 120, 200.0))
    want, margin = set(), np.inf
    for fr in frames:
        k, m = ref.touched_units(_host(fr), vl, trunc)
        want |= k
        margin = min(margin, m)
    assert margin > 1e-5, margin
    vol = _volume(vl, trunc, frames)
    assert _hip_units(vol) == want
    assert vol.num_units == len(want)


def _compare_volumes(vol, rv):
    got = vol.voxels()
    want = rv.arrays()
    gk = {tuple(k): i for i, k in enumerate(got["keys"].cpu().tolist())}
    gt, gw, gc = (got[n].cpu().numpy().astype(np.float64) for n in ("tsdf", "weight", "color"))
    rows = [gk[tuple(k)] for k in want["keys"].tolist()]
    assert len(rows) == len(gk)
    gt, gw, gc = gt[rows], gw[rows], gc[rows]
    updated = (want["weight"] > 0) | (gw > 0)
    ok = (gw == want["weight"]) & (np.abs(gt - want["tsdf"]) <= 1e-5) & (np.abs(gc - want["color"]).max(-1) <= 1e-3)
    bad = updated & ~ok
    return int(updated.sum()), int(bad.sum()), int((bad & ~want["ambiguous"]).sum())


@pytest.mark.parametrize("scene", ["planes", "sphere"])
def test_integration_matches_the_restatement(scene):
    vl, trunc = (0.02, 0.04) if scene == "planes" else (0.02, 0.06)
    frames = _dev_frames(_plane_frames(6) if scene == "planes" else _sphere_frames(8, 160, 120, 200.0))
    vol = _volume(vl, trunc, frames)
    rv = ref.RefVolume(vl, trunc)
    for fr in frames:
        rv.integrate(_host(fr))
    n, bad, bad_clear = _compare_volumes(vol, rv)
    print(f"{scene}: {bad} of {n} updated voxels differ from the fp64 restatement ({bad_clear} away from a knife edge)")
    assert n > 10000
    assert bad <= 1e-3 * n, (bad, n)
    assert bad_clear == 0, bad_clear


# ---- extraction, determinism
def _sphere_volume(n=10, vl=0.02, trunc=0.06):
    return _volume(vl, trunc, _dev_frames(_sphere_frames(n, 160, 120, 200.0)))


def test_extraction_matches_the_restatement_on_the_hip_volume():
    vol = _sphere_volume()
    m = vol.extract_triangle_mesh()
    vox = {k: v.cpu().numpy() for k, v in vol.voxels().items()}
    v, t, c = ref.extract(vox, vol.voxel_length)
    assert len(t) > 2000
    assert np.array_equal(m.triangles.cpu().numpy().astype(np.int64), t)
    assert np.abs(m.vertices.cpu().numpy() - v).max() <= 1e-6
    assert np.abs(m.vertex_colors.cpu().numpy() - c).max() <= 1e-5


def test_two_runs_are_bitwise_equal():
    from splat_slam_amd.mesh import clean_mesh
    a = clean_mesh(_sphere_volume().extract_triangle_mesh())
    b = clean_mesh(_sphere_volume().extract_triangle_mesh())
    for x, y in ((a.vertices, b.vertices), (a.triangles, b.triangles), (a.vertex_colors, b.vertex_colors)):
        assert x.shape == y.shape and torch.equal(x, y)


# ---- cleaning
def test_cleaning_drops_the_floating_blob_and_keeps_the_surface():
    sp = pytest.importorskip("scipy.sparse")
    csgraph = pytest.importorskip("scipy.sparse.csgraph")
    from splat_slam_amd.mesh import TriangleMesh, clean_mesh
    big = _sphere_volume().extract_triangle_mesh()
    # a floating blob: a triangle strip of 40 vertices, away from the sphere
    g = torch.Generator().manual_seed(3)
    nb = 40
    bv = torch.rand(nb, 3, generator=g) * 0.05 + 2.0
    bt = torch.stack([torch.arange(nb - 2), torch.arange(1, nb - 1), torch.arange(2, nb)], 1).int()
    V = big.vertices.shape[0]
    verts = torch.cat([big.vertices, bv.to(DEV)])
    tris = torch.cat([bt.to(DEV) + V, big.triangles])          # the blob first: order must not matter
    cols = torch.cat([big.vertex_colors, torch.rand(nb, 3, generator=g).to(DEV)])
    m, vmap = clean_mesh(TriangleMesh(verts, tris, cols), min_len=100, return_vertex_map=True)
    t = tris.cpu().numpy()
    n = verts.shape[0]
    adj = sp.coo_matrix((np.ones(3 * len(t)), (np.concatenate([t[:, 0], t[:, 1], t[:, 2]]), np.concatenate([t[:, 1], t[:, 2], t[:, 0]]))),
                        shape=(n, n))
    _, lab = csgraph.connected_components(adj, directed=False)
    size = np.bincount(lab)
    keep = size[lab] >= 100
    vm = vmap.cpu().numpy()
    assert np.array_equal(vm >= 0, keep)
    assert not keep[V:].any() and keep[:V].sum() > 1000
    assert np.array_equal(vm[keep], np.arange(keep.sum()))
    assert torch.equal(m.vertices, verts[torch.from_numpy(keep).to(DEV)])
    want_v, want_t, _, _ = ref.clean(verts.cpu().numpy().astype(np.float64), t.astype(np.int64), cols.cpu().numpy(), 100)
    assert np.array_equal(m.triangles.cpu().numpy(), want_t)


# ---- analytic sphere at 640x480
def test_sphere_at_640x480_and_1cm_is_closed_and_on_the_surface():
    from splat_slam_amd.mesh import clean_mesh
    r, vl, centre = 0.3, 0.01, np.array([0.013, -0.021, 0.007])
    frames = _dev_frames(_sphere_frames(14, 640, 480, 700.0, r=r, centre=tuple(centre)), exposure=False)
    vol = _volume(vl, 0.03, frames)
    m = clean_mesh(vol.extract_triangle_mesh())
    v, t = m.vertices.cpu().numpy().astype(np.float64), m.triangles.cpu().numpy().astype(np.int64)
    assert len(v) > 10000
    assert ref.closed_and_oriented(t)
    assert ref.euler(len(v), t) == 2
    dist = np.abs(np.linalg.norm(v - centre, axis=1) - r)
    print(f"sphere 640x480, 1 cm: {len(v)} vertices, |r - 0.3| max {dist.max():.5f} m, 99th pct {np.percentile(dist, 99):.5f} m")
    assert dist.max() <= 0.5 * vl


# ---- end to end
def test_session_evaluate_with_mesh(tmp_path):
    from splat_slam_amd import synthetic as syn
    from splat_slam_amd.mesh import TriangleMesh
    from splat_slam_amd.session import MappingSession
    intr = syn.INTRINSICS["metric"]
    world = syn.room_parameters(60000, seed=43, device=DEV)
    world["scaling"] = world["scaling"] * 0 + world["scaling"].mean(dim=1, keepdim=True) + 1.6    # opaque surface splats
    world["opacity"] = torch.full_like(world["opacity"], 4.0)
    gm = syn.model_from_parameters(world, device=DEV, knn_fn=lambda p: torch.ones(p.shape[0], device=p.device))
    cams = syn.make_views(world, 6, intr, DEV, seed=5, perturb=False)
    bg = torch.zeros(3, device=DEV)
    loop = types.SimpleNamespace(config=syn.DEFAULT_CONFIG, device=DEV, viewpoints={2 * k: c for k, c in enumerate(cams)},
                                 gaussians=gm, background=bg)
    sess = MappingSession(loop, intr)
    plain = sess.evaluate()
    path = str(tmp_path / "mesh.ply")
    got = sess.evaluate(mesh=True, mesh_path=path)
    mesh = got.pop("mesh")
    assert got == plain
    v = mesh.vertices.cpu().numpy().astype(np.float64)
    assert len(v) > 1000
    half = np.array(syn.ROOM) / 2
    assert (np.abs(v) <= half + 0.04).all()
    wall = lambda p: np.min(np.abs(np.abs(p) - half), axis=1)
    # the fused geometry: every frame's rendered depth back-projected (alpha-weighted, so it sits in front of the box's walls)
    from splat_slam_amd.camera import getWorld2View2
    from splat_slam_amd.mapper import PipelineParams
    from splat_slam_amd.renderer import render
    given = []
    with torch.no_grad():
        for cam in cams:
            d = render(cam, gm, PipelineParams(), bg)["depth"][0].cpu().numpy().astype(np.float64)
            vv, uu = np.nonzero((d > 0) & (cam.depth.cpu().numpy() > 0))
            z = d[vv, uu]
            pc = np.stack([(uu - cam.cx) * z / cam.fx, (vv - cam.cy) * z / cam.fy, z, np.ones_like(z)])
            given.append((np.linalg.inv(getWorld2View2(cam.R, cam.T).double().cpu().numpy()) @ pc)[:3].T)
    dg = wall(np.concatenate(given))
    dist = wall(v)
    med, p95 = float(np.median(dist)), float(np.percentile(dist, 95))
    gmed, gp95 = float(np.median(dg)), float(np.percentile(dg, 95))
    print(f"room mesh: {len(v)} vertices, distance to the nearest wall median {med:.4f} m, 95th pct {p95:.4f} m; "
          f"rendered depth points: median {gmed:.4f} m, 95th pct {gp95:.4f} m")
    # the fusion adds at most 1.5 cm (median) / 5 cm (95th percentile) to where the rendered depth already puts the walls
    assert med <= gmed + 0.015 and p95 <= gp95 + 0.05
    back = TriangleMesh.read_ply(path)
    assert torch.equal(back.vertices, mesh.vertices.cpu()) and torch.equal(back.triangles, mesh.triangles.cpu())
    assert (back.vertex_colors - mesh.vertex_colors.cpu()).abs().max() <= 0.5 / 255 + 1e-6


def test_against_open3d_where_it_exists():
    o3d = pytest.importorskip("open3d")
    vl, trunc = 0.02, 0.06
    frames = _sphere_frames(6, 160, 120, 200.0)
    vol = o3d.pipelines.integration.ScalableTSDFVolume(voxel_length=vl, sdf_trunc=trunc,
                                                      color_type=o3d.pipelines.integration.TSDFVolumeColorType.RGB8)
    for fr in frames:
        color = o3d.geometry.Image(np.ascontiguousarray((fr["render"].transpose(1, 2, 0) * 255).astype(np.uint8)))
        depth = o3d.geometry.Image(np.ascontiguousarray(fr["depth"]))
        rgbd = o3d.geometry.RGBDImage.create_from_color_and_depth(color, depth, depth_scale=1.0, depth_trunc=30,
                                                                  convert_rgb_to_intensity=False)
        intr = o3d.camera.PinholeCameraIntrinsic(160, 120, fr["fx"], fr["fy"], fr["cx"], fr["cy"])
        vol.integrate(rgbd, intr, fr["w2c"])
    o = vol.extract_triangle_mesh()
    ours = _volume(vl, trunc, _dev_frames(frames, exposure=False)).extract_triangle_mesh()
    a = np.unique(np.round(np.asarray(o.vertices) / 1e-5).astype(np.int64), axis=0)
    b = np.unique(np.round(ours.vertices.cpu().numpy() / 1e-5).astype(np.int64), axis=0)
    assert len(a) == len(b) and np.array_equal(a, b)
