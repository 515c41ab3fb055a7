"""-m gpu: mesh evaluation on the HIP kernels (splat_slam_amd.mesh_eval, csrc/sgr_mesh_eval.hip) against the fp64 restatement of
tests/mesh_eval_ref.py: exact nearest neighbours, area-weighted sampling, the metric reductions, ICP, determinism, and the
eval_mesh branch of eval_rendering / MappingSession.evaluate."""
import math
import types

import numpy as np
import pytest
import torch

import mesh_eval_ref as ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
REL, ABS = 4e-7, 1e-8


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(DEV)


def _mesh(v, t):
    from splat_slam_amd.mesh import TriangleMesh
    v = _dev(v)
    return TriangleMesh(v, torch.from_numpy(np.asarray(t, np.int32)).to(DEV), torch.full_like(v, 0.5))


def _query(target, query, **kw):
    from splat_slam_amd.mesh_eval import PointGrid
    d, i = PointGrid(_dev(target)).query(_dev(query), **kw)
    return d.cpu().numpy().astype(np.float64), i.cpu().numpy().astype(np.int64)


def _assert_exact(target, query, d, i):
    """d is the fp64 minimum over the fp32 inputs, and the returned index attains it"""
    t64 = np.asarray(target, np.float32).astype(np.float64)
    q64 = np.asarray(query, np.float32).astype(np.float64)
    want, _ = ref.nearest(q64, t64)
    assert (i >= 0).all() and (i < len(t64)).all()
    tol = REL * want + ABS
    assert np.all(np.abs(d - want) <= tol), np.max(np.abs(d - want) - tol)
    got = np.linalg.norm(q64 - t64[i], axis=1)
    assert np.all(np.abs(got - want) <= tol), np.max(np.abs(got - want) - tol)


def _room_samples(n, rng):
    v, t = ref.room_mesh(8)
    a = 0.5 * np.linalg.norm(np.cross(v[t[:, 1]] - v[t[:, 0]], v[t[:, 2]] - v[t[:, 0]]), axis=1)
    f = rng.choice(len(t), n, p=a / a.sum())
    r1, r2 = rng.random(n), rng.random(n)
    s = np.sqrt(r1)
    return ((1 - s)[:, None] * v[t[f, 0]] + (s * (1 - r2))[:, None] * v[t[f, 1]] + (s * r2)[:, None] * v[t[f, 2]]).astype(np.float32)


# ---- nearest neighbours
@pytest.mark.parametrize("case", ["volume", "sphere", "room", "plane", "line"])
def test_nearest_neighbours_are_exact(case):
    rng = np.random.default_rng({"volume": 0, "sphere": 1, "room": 2, "plane": 3, "line": 4}[case])
    if case == "volume":
        t = rng.uniform(-2, 3, size=(20000, 3))
        q = rng.uniform(-2.5, 3.5, size=(4000, 3))
    elif case == "sphere":
        t = rng.normal(size=(20000, 3))
        t = 1.3 * t / np.linalg.norm(t, axis=1, keepdims=True) + 0.2
        q = rng.normal(size=(4000, 3))
        q = (1.3 + rng.normal(scale=0.05, size=(4000, 1))) * q / np.linalg.norm(q, axis=1, keepdims=True) + 0.2
        q[:200] = rng.normal(scale=0.05, size=(200, 3)) + 0.2              # the empty centre: long walks
    elif case == "room":
        t = _room_samples(20000, rng)
        q = _room_samples(4000, rng) + rng.normal(scale=0.01, size=(4000, 3))
    elif case == "plane":
        t = np.concatenate([rng.uniform(-1, 1, size=(20000, 2)), np.full((20000, 1), 0.7)], 1)
        q = rng.uniform(-1.5, 1.5, size=(4000, 3))
    else:
        s = rng.uniform(-3, 3, size=(20000, 1))
        t = np.array([0.5, -0.2, 0.1]) + s * np.array([0.6, 0.0, 0.8])
        q = rng.uniform(-3, 3, size=(4000, 3))
    t, q = t.astype(np.float32), q.astype(np.float32)
    d, i = _query(t, q)
    _assert_exact(t, q, d, i)


def test_duplicated_points_return_the_smallest_index():
    rng = np.random.default_rng(5)
    u = rng.uniform(-1, 1, size=(3000, 3)).astype(np.float32)
    group = rng.permutation(np.repeat(np.arange(3000), 3))             # every point three times, at shuffled indices
    t = u[group]
    smallest = np.full(3000, 1 << 30)
    np.minimum.at(smallest, group, np.arange(len(group)))
    q = np.concatenate([u, rng.uniform(-1.2, 1.2, size=(3000, 3)).astype(np.float32)])
    d, i = _query(t, q)
    _assert_exact(t, q, d, i)
    assert np.array_equal(i, smallest[group[i]])
    assert (d[:3000] == 0).all()


def test_queries_far_outside_the_target_box_terminate_and_are_exact():
    rng = np.random.default_rng(6)
    t = _room_samples(20000, rng)
    centre = np.array([0.0, 0.0, 1.25])
    dirs = rng.normal(size=(3000, 3))
    dirs /= np.linalg.norm(dirs, axis=1, keepdims=True)
    q = (centre + dirs * (2.5 + rng.uniform(1, 10, size=(3000, 1)))).astype(np.float32)     # 1-10 m beyond the box's reach
    d, i = _query(t, q)
    _assert_exact(t, q, d, i)
    assert d.min() > 0.5


def test_tiny_targets_and_an_empty_query():
    rng = np.random.default_rng(7)
    q = rng.uniform(-3, 3, size=(500, 3)).astype(np.float32)
    for n in (1, 2):
        t = rng.uniform(-1, 1, size=(n, 3)).astype(np.float32)
        d, i = _query(t, q)
        _assert_exact(t, q, d, i)
    from splat_slam_amd.mesh_eval import PointGrid
    d, i = PointGrid(_dev(q)).query(torch.zeros(0, 3, device=DEV))
    assert d.shape == (0,) and i.shape == (0,)


def test_max_dist_cuts_off_exactly_beyond_it():
    rng = np.random.default_rng(8)
    t = rng.uniform(-1, 1, size=(20000, 3)).astype(np.float32)
    q = rng.uniform(-1.3, 1.3, size=(4000, 3)).astype(np.float32)
    want, _ = ref.nearest(q.astype(np.float64), t.astype(np.float64))
    for md in (0.02, 0.05, 0.2):
        d, i = _query(t, q, max_dist=md)
        near = np.abs(want - md) <= 1e-6 * md                           # the rounding may decide these either way
        cut = i == -1
        assert np.array_equal(cut[~near], want[~near] > md), md
        assert np.isinf(d[cut]).all()
        keep = ~cut
        tol = REL * want[keep] + ABS
        assert np.all(np.abs(d[keep] - want[keep]) <= tol)
        assert 0 < cut.sum() < len(q)


def test_a_transformed_query_matches_the_query_of_transformed_points():
    rng = np.random.default_rng(9)
    t = _room_samples(20000, rng)
    q = _room_samples(4000, rng)
    T = np.eye(4)
    T[:3, :3] = ref.rotation((0.2, 1.0, -0.4), 7.0)
    T[:3, 3] = (0.05, -0.03, 0.08)
    from splat_slam_amd.mesh_eval import PointGrid
    grid = PointGrid(_dev(t))
    d1, i1 = (x.cpu().numpy() for x in grid.query(_dev(q), transform=torch.from_numpy(T)))
    pre = ref.transform_f32(T, q)
    d2, i2 = (x.cpu().numpy() for x in grid.query(_dev(pre)))
    assert np.allclose(d1, d2, rtol=2e-6, atol=2e-6)
    diff = i1 != i2
    t64 = t.astype(np.float64)
    pre64 = pre.astype(np.float64)
    assert np.all(np.abs(np.linalg.norm(pre64[diff] - t64[i1[diff]], axis=1) - np.linalg.norm(pre64[diff] - t64[i2[diff]], axis=1)) <= 1e-5)
    assert diff.mean() < 1e-3
    # the grid can be built of transformed points as well
    d3, _ = PointGrid(_dev(q), transform=torch.from_numpy(T)).query(_dev(t))
    d4, _ = PointGrid(_dev(pre)).query(_dev(t))
    assert np.allclose(d3.cpu().numpy(), d4.cpu().numpy(), rtol=2e-6, atol=2e-6)


def test_a_million_targets_against_ckdtree():
    pytest.importorskip("scipy")
    rng = np.random.default_rng(10)
    t = np.concatenate([_room_samples(900000, rng), rng.uniform(-2, 2, size=(100000, 3)).astype(np.float32)])
    q = _room_samples(20000, rng) + rng.normal(scale=0.02, size=(20000, 3)).astype(np.float32)
    q = q.astype(np.float32)
    d, i = _query(t, q)
    want, _ = ref.nearest_large(q.astype(np.float64), t.astype(np.float64))
    tol = REL * want + ABS
    assert np.all(np.abs(d - want) <= tol)
    got = np.linalg.norm(q.astype(np.float64) - t.astype(np.float64)[i], axis=1)
    assert np.all(np.abs(got - want) <= tol)


# ---- sampling
def _spread_mesh(rng):
    """60 triangles whose areas span 10^4, plus faces of zero area (a repeated vertex, three collinear vertices)"""
    v, t = [], []
    for k in range(60):
        s = 10 ** (-2 * k / 59)                            # edge scale 1 .. 0.01: areas 1 .. 1e-4
        o = rng.uniform(-2, 2, size=3)
        e = rng.normal(size=(2, 3))
        v += [o, o + s * e[0], o + s * e[1]]
        t.append((3 * k, 3 * k + 1, 3 * k + 2))
    base = len(v)
    v += [np.zeros(3), np.array([1.0, 1, 1]), np.array([2.0, 2, 2])]
    zero = [(base, base + 1, base + 2), (0, 0, 1), (5, 4, 5)]
    t += zero
    return np.array(v), np.array(t), list(range(60, 63))


def test_samples_lie_on_their_triangles_in_proportion_to_area_and_never_on_zero_area_faces():
    from splat_slam_amd.mesh_eval import sample_surface
    rng = np.random.default_rng(11)
    v, t, zero = _spread_mesh(rng)
    n = 400000
    pts, tri = sample_surface(_mesh(v, t), n, seed=3)
    pts, tri = pts.cpu().numpy().astype(np.float64), tri.cpu().numpy()
    assert not np.isin(tri, zero).any() and (tri >= 0).all()
    v32 = v.astype(np.float32).astype(np.float64)
    a, b, c = v32[t[tri, 0]], v32[t[tri, 1]], v32[t[tri, 2]]
    e1, e2, r = b - a, c - a, pts - a
    # barycentrics by least squares (exact for a point in the plane)
    g11, g12, g22 = (e1 * e1).sum(1), (e1 * e2).sum(1), (e2 * e2).sum(1)
    r1, r2 = (r * e1).sum(1), (r * e2).sum(1)
    det = g11 * g22 - g12 * g12
    u, w = (g22 * r1 - g12 * r2) / det, (g11 * r2 - g12 * r1) / det
    scale = np.maximum(np.linalg.norm(e1, axis=1), np.linalg.norm(e2, axis=1))
    resid = np.linalg.norm(r - u[:, None] * e1 - w[:, None] * e2, axis=1)
    assert (resid <= 4e-6 * (1 + np.abs(a).max(1))).all()
    tol = 4e-6 * (1 + np.abs(a).max(1)) / scale
    assert (u >= -tol).all() and (w >= -tol).all() and (u + w <= 1 + tol).all()
    faces_area = 0.5 * np.linalg.norm(np.cross(v32[t[:, 1]] - v32[t[:, 0]], v32[t[:, 2]] - v32[t[:, 0]]), axis=1)
    expect = n * faces_area / faces_area.sum()
    counts = np.bincount(tri, minlength=len(t)).astype(np.float64)
    big = expect >= 5
    obs = np.append(counts[big], counts[~big].sum())
    exp = np.append(expect[big], expect[~big].sum())
    chi2 = ((obs - exp) ** 2 / exp).sum()
    dof = len(obs) - 1
    assert chi2 < dof + 6 * math.sqrt(2 * dof), (chi2, dof)


def test_sampling_is_bitwise_reproducible_seeded_and_independent_of_n():
    from splat_slam_amd.mesh_eval import sample_surface
    v, t, _ = _spread_mesh(np.random.default_rng(12))
    m = _mesh(v, t)
    a, ta = sample_surface(m, 10001, seed=7)
    b, tb = sample_surface(m, 10001, seed=7)
    c, _ = sample_surface(m, 10001, seed=8)
    d, td = sample_surface(m, 10002, seed=7)
    assert torch.equal(a, b) and torch.equal(ta, tb)
    assert not torch.equal(a, c)
    assert torch.equal(a, d[:10001]) and torch.equal(ta, td[:10001])


def test_empty_and_zero_area_meshes_are_refused():
    from splat_slam_amd.mesh_eval import evaluate_mesh, sample_surface
    flat = _mesh(np.array([[0, 0, 0], [1, 1, 1], [2, 2, 2], [0, 0, 0]]), [[0, 1, 2], [0, 3, 1]])
    with pytest.raises(ValueError, match="positive area"):
        sample_surface(flat, 10)
    good = _mesh(np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]]), [[0, 1, 2]])
    with pytest.raises(ValueError, match="positive area"):
        evaluate_mesh(flat, good, samples=100)
    with pytest.raises(ValueError, match="positive area"):
        evaluate_mesh(good, flat, samples=None)
    with pytest.raises(ValueError, match="empty"):
        evaluate_mesh(_mesh(np.zeros((3, 3)), np.zeros((0, 3))), good)
    with pytest.raises(ValueError, match="outside"):
        evaluate_mesh(_mesh(np.eye(3), [[0, 1, 3]]), good)


# ---- metrics
def _moved_room(noise=0.002, seed=13, move=True):
    rng = np.random.default_rng(seed)
    v, t = ref.room_mesh(16)
    noisy = v + rng.normal(scale=noise, size=v.shape)
    Tt = np.eye(4)
    if move:
        Tt[:3, :3] = ref.rotation((0.3, -0.7, 0.5), 2.0)
        Tt[:3, 3] = (0.02, -0.01, 0.015)
    return v, t, ref.transform(Tt, noisy), noisy, Tt


def test_metrics_equal_the_restatement_on_the_gpus_own_samples():
    from splat_slam_amd.mesh_eval import GT_SEED_OFFSET, evaluate_mesh, sample_surface
    v, t, moved, _, _ = _moved_room()
    pred, gt = _mesh(moved, t), _mesh(v, t)
    n, tau = 8000, 0.05
    got = evaluate_mesh(pred, gt, distance_thresh=tau, icp_align=False, samples=n, seed=4)
    P = sample_surface(pred, n, seed=4)[0].cpu().numpy().astype(np.float64)
    G = sample_surface(gt, n, seed=4 + GT_SEED_OFFSET)[0].cpu().numpy().astype(np.float64)
    d_pg, _ = ref.nearest(P, G)
    d_gp, _ = ref.nearest(G, P)
    want = ref.metrics(d_pg, d_gp, tau)
    for k in ("accuracy", "completion", "chamfer_l1"):
        assert abs(got[k] - want[k]) <= 1e-6 * want[k], (k, got[k], want[k])
    amb_p = int((np.abs(d_pg - tau) <= 1e-6).sum())
    amb_g = int((np.abs(d_gp - tau) <= 1e-6).sum())
    assert abs(got["precision"] * n - want["precision"] * n) <= amb_p + 1e-9
    assert abs(got["completion_ratio"] * n - want["completion_ratio"] * n) <= amb_g + 1e-9
    assert got["recall"] == got["completion_ratio"]
    p, r = got["precision"], got["recall"]
    assert abs(got["fscore"] - 2 * p * r / (p + r)) <= 1e-15
    assert got["icp"] is None and got["samples"] == n and got["distance_thresh"] == tau


# ---- ICP
def _angle_deg(R):
    return math.degrees(math.acos(max(-1.0, min(1.0, (np.trace(R) - 1) / 2))))


def test_icp_recovers_the_motion_and_matches_the_restatement():
    from splat_slam_amd.mesh_eval import GT_SEED_OFFSET, ICP_THRESHOLD, PointGrid, evaluate_mesh, icp, sample_surface
    v, t, moved, noisy, Tt = _moved_room()
    pred, gt = _mesh(moved, t), _mesh(v, t)
    n = 50000
    got = evaluate_mesh(pred, gt, samples=n, seed=0)
    T = got["icp"]["transformation"]
    E = T @ Tt                                             # the identity where the motion is undone
    assert _angle_deg(E[:3, :3]) < 0.1, _angle_deg(E[:3, :3])
    assert np.linalg.norm(E[:3, 3]) < 0.002, np.linalg.norm(E[:3, 3])
    assert 1 <= got["icp"]["iterations"] <= 30 and got["icp"]["fitness"] > 0.99
    # the restatement on the same samples
    P = sample_surface(pred, n, seed=0)[0]
    G = sample_surface(gt, n, seed=GT_SEED_OFFSET)[0]
    mine = icp(P, PointGrid(G), max_correspondence_distance=ICP_THRESHOLD)
    assert np.array_equal(mine["transformation"], T)
    G64 = G.cpu().numpy().astype(np.float64)
    tree = None
    try:
        from scipy.spatial import cKDTree
        tree = cKDTree(G64)
    except ImportError:
        pass
    nn = (lambda q, _t: tree.query(q, k=1)) if tree is not None else None
    want = ref.icp(P.cpu().numpy(), G64, max_dist=ICP_THRESHOLD, nn=nn)
    assert np.abs(want["transformation"] - T).max() <= 1e-5, np.abs(want["transformation"] - T).max()
    assert abs(want["iterations"] - got["icp"]["iterations"]) <= 1
    # post-ICP accuracy is that of the unmoved noisy mesh; without ICP it is clearly worse
    still = evaluate_mesh(_mesh(noisy, t), gt, icp_align=False, samples=n, seed=0)
    assert abs(got["accuracy"] - still["accuracy"]) <= 1e-3, (got["accuracy"], still["accuracy"])
    raw = evaluate_mesh(pred, gt, icp_align=False, samples=n, seed=0)
    # (with 50 k independent samples per mesh, ~1.8 cm of the aligned accuracy is the samples' own spacing)
    assert raw["accuracy"] > got["accuracy"] + 0.01 and raw["accuracy"] > 1.5 * got["accuracy"]
    assert raw["fscore"] < got["fscore"] and raw["chamfer_l1"] > got["chamfer_l1"]
    print(f"room ICP: {got['icp']['iterations']} iterations, angle error {_angle_deg(E[:3, :3]):.4f} deg, "
          f"translation error {1e3 * np.linalg.norm(E[:3, 3]):.3f} mm; accuracy {got['accuracy']:.5f} (unmoved {still['accuracy']:.5f},"
          f" without ICP {raw['accuracy']:.5f})")


def test_two_evaluations_are_bitwise_equal():
    from splat_slam_amd.mesh_eval import evaluate_mesh
    v, t, moved, _, _ = _moved_room(seed=14)
    pred, gt = _mesh(moved, t), _mesh(v, t)
    a = evaluate_mesh(pred, gt, samples=30000)
    b = evaluate_mesh(pred, gt, samples=30000)
    assert set(a) == set(b)
    for k in a:
        if k == "icp":
            assert np.array_equal(a[k]["transformation"], b[k]["transformation"])
            assert {x: y for x, y in a[k].items() if x != "transformation"} == {x: y for x, y in b[k].items() if x != "transformation"}
        else:
            assert a[k] == b[k], k


# ---- end to end
def _room_session():
    from splat_slam_amd import synthetic as syn
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
    return MappingSession(loop, intr)


def test_eval_rendering_scores_its_own_mesh_perfectly_and_keeps_its_keys(tmp_path):
    from splat_slam_amd.eval import eval_rendering
    from splat_slam_amd.mapper import PipelineParams
    sess = _room_session()
    frames = [sess.loop.viewpoints[k] for k in sorted(sess.loop.viewpoints)]
    args = (frames, sess.loop.gaussians, PipelineParams(), sess.loop.background)
    path = str(tmp_path / "own.ply")
    plain = eval_rendering(*args, mesh=True, mesh_path=path)
    assert set(plain) == {"psnr", "ssim", "depth_l1", "mean_psnr", "mean_ssim", "mean_depthl1", "mesh"}
    got = eval_rendering(*args, mesh=True, gt_mesh_path=path, icp_align=False, mesh_samples=None)
    m = got.pop("mesh_metrics")
    assert m["accuracy"] == 0.0 and m["completion"] == 0.0 and m["completion_ratio"] == 1.0 and m["fscore"] == 1.0
    assert m["samples"] is None and m["icp"] is None
    assert set(got) == set(plain)
    assert got["psnr"] == plain["psnr"] and got["ssim"] == plain["ssim"]
    # a ground truth without area: the error is reported, the rendering metrics stay
    from splat_slam_amd.mesh import TriangleMesh
    flat = TriangleMesh(torch.zeros(3, 3, device=DEV), torch.tensor([[0, 1, 2]], dtype=torch.int32, device=DEV),
                        torch.zeros(3, 3, device=DEV))
    bad = eval_rendering(*args, mesh=True, gt_mesh_path=flat)
    assert "positive area" in bad["mesh_metrics_error"] and "mesh_metrics" not in bad and bad["psnr"] == plain["psnr"]


def test_session_evaluate_against_the_box_walls(tmp_path):
    from splat_slam_amd import synthetic as syn
    from splat_slam_amd.mesh import TriangleMesh
    half = np.array(syn.ROOM) / 2
    v, t = ref.box_mesh(-half, half, 24)
    path = str(tmp_path / "walls.ply")
    TriangleMesh(torch.from_numpy(v.astype(np.float32)), torch.from_numpy(t.astype(np.int32)),
                 torch.full((len(v), 3), 0.5)).write_ply(path)
    got = _room_session().evaluate(mesh=True, gt_mesh_path=path)
    m = got["mesh_metrics"]
    print("room session vs walls: " + ", ".join(f"{k} {m[k]:.4f}" for k in ("accuracy", "completion", "precision",
                                                                           "completion_ratio", "fscore", "chamfer_l1")))
    # the mesh sits a median 3.5 cm in front of the walls and covers what 6 views see
    assert 0.005 < m["accuracy"] < 0.08
    assert m["precision"] > 0.4
    assert 0.02 < m["completion_ratio"] <= 1.0 and m["completion"] > 0.0
    assert m["icp"] is not None and m["icp"]["fitness"] > 0.5
