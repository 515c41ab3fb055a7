"""droid_backends.ba on the MI355X at its graph and size edges, every element held to its own derived bound (tests/dba_cases.py:
criteria A, B, C against the fp64 oracle with magnitudes of tests/dba_ref.py), and the frame geometry functions at small odd
shapes with out-of-range edges.  tests/test_dba_cpu.py proves the same criteria on the CPU: the fp32 restatement passes them and
every planted fault fails one."""
import numpy as np
import pytest
import torch

import dba_cases as DC
import dba_ref as R

pytestmark = pytest.mark.gpu


def f32(a):
    return torch.tensor(np.asarray(a), dtype=torch.float32, device="cuda").contiguous()


def i64(a):
    return torch.tensor([int(v) for v in a], dtype=torch.int64, device="cuda")


def to_gpu(c, edges=None):
    e = list(range(len(c["ii"]))) if edges is None else edges
    return dict(poses=f32(c["poses"]), disps=f32(c["disps"]), intr=f32(c["intr"]), sens=f32(c["sens"]), tgt=f32(c["tgt"][e]),
                wgt=f32(c["wgt"][e]), eta=f32(c["eta"]), ii=i64([c["ii"][k] for k in e]), jj=i64([c["jj"][k] for k in e]))


def run(c, g, iterations=1):
    import droid_backends
    dx, dz = droid_backends.ba(g["poses"], g["disps"], g["intr"], g["sens"], g["tgt"], g["wgt"], g["eta"], g["ii"], g["jj"], c["t0"], c["t1"],
                               iterations, c["lm"], c["ep"], c["mode"] == "motion_only", c["mode"] == "depth_only")
    torch.cuda.synchronize()
    return dx, dz


def outputs(g, dx, dz):
    return g["poses"].cpu().numpy(), g["disps"].cpu().numpy(), dx.cpu().numpy(), None if dz is None else dz.cpu().numpy()


def same_bits(a, b):
    for x, y in zip(a, b):
        if x is None or y is None:
            assert x is None and y is None
        else:
            assert torch.equal(x, y)


@pytest.mark.parametrize("name", DC.CASES)
def test_one_iteration_is_inside_every_bound(name):
    DC.check_scene(name, want_behind=not name.startswith(("chol", "big")))
    c = DC.case(name)
    g = to_gpu(c)
    dx, dz = run(c, g)
    ratios, broken = DC.criteria(name, *outputs(g, dx, dz))
    print(f"\n{name}: err / bound " + " ".join(f"{k}={v:.4f}" for k, v in sorted(ratios.items())), broken)
    assert not broken, broken
    for k, r in ratios.items():
        assert r <= 1.0, (name, k, r)
    if name == "win:no_edge_singular":
        assert torch.equal(dx, torch.zeros_like(dx))


@pytest.mark.parametrize("name", ["oob", "oob:long_poses"])
def test_out_of_range_edges_take_part_in_nothing(name):
    c = DC.case(name)
    keep = R.kept_edges(c["ii"], c["jj"], min(len(c["poses"]), len(c["disps"])))
    assert 0 < len(keep) < len(c["ii"])
    assert 8 not in DC.oracle(name)["kx"]               # frame 8 occurs only as the ii of a dropped edge: no depth row
    g_all, g_kept = to_gpu(c), to_gpu(c, keep)
    dx1, dz1 = run(c, g_all)
    dx2, dz2 = run(c, g_kept)
    same_bits((dx1, dz1, g_all["poses"], g_all["disps"]), (dx2, dz2, g_kept["poses"], g_kept["disps"]))


def test_two_iterations_equal_two_calls_of_one():
    c = DC.case("iter")
    g2, g11 = to_gpu(c), to_gpu(c)
    dx2, dz2 = run(c, g2, iterations=2)
    run(c, g11)
    dx11, dz11 = run(c, g11)
    same_bits((dx2, dz2, g2["poses"], g2["disps"]), (dx11, dz11, g11["poses"], g11["disps"]))


def test_a_side_stream_gives_the_bits_of_the_default_stream():
    c = DC.case("iter")
    g0, g1 = to_gpu(c), to_gpu(c)
    dx0, dz0 = run(c, g0, iterations=2)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        dx1, dz1 = run(c, g1, iterations=2)
    torch.cuda.synchronize()
    same_bits((dx0, dz0, g0["poses"], g0["disps"]), (dx1, dz1, g1["poses"], g1["disps"]))


# ---- frame geometry
GEOM_SHAPES = ((7, 9), (5, 13), (3, 5))
GEOM_II = [0, 1, 2, 3, 4, 5, 8, 1]
GEOM_JJ = [1, 0, 4, 3, 7, 2, 0, 8]


def edge_depths(poses, disps, intr, i, j):
    """z of every pixel of frame i in frame j, and under the translation alone (frame_distance's second term)"""
    _, _, xr, yr = R.pixel_rays(*disps.shape[1:], intr)
    t, q = R.relative(poses[i], poses[j])
    h = disps[i].reshape(-1)
    return (np.stack([xr, yr, np.ones_like(xr)], 1) @ R.rotmat(q).T)[:, 2] + h * t[2], 1.0 + h * t[2]


def geometry_scene(ht, wd, n=9):
    """the ba scene (three pixels per frame far behind the camera on forward edges) with one pixel of frame 0 placed at z = 0.12 in
    frame 1, between projmap's two thresholds"""
    _, poses, disps = DC.scene(ht, wd, n, seed=70 + wd)
    intr = DC.intrinsics(ht, wd)
    poses, disps, intr = DC.r32(poses), DC.r32(disps), DC.r32(intr)
    _, _, xr, yr = R.pixel_rays(ht, wd, intr)
    t, q = R.relative(poses[0], poses[1])
    p = ht * wd - 1
    disps[0].reshape(-1)[p] = (0.12 - (R.rotmat(q) @ np.array([xr[p], yr[p], 1.0]))[2]) / t[2]
    return poses, DC.r32(disps), intr


@pytest.mark.parametrize("shape", GEOM_SHAPES)
def test_frame_distance_projmap_iproj_match_the_oracle_with_out_of_range_edges(shape):
    import droid_backends
    poses, disps, intr = geometry_scene(*shape)
    nv = len(disps)
    z = np.concatenate([np.concatenate(edge_depths(poses, disps, intr, i, j)) for i, j in zip(GEOM_II, GEOM_JJ)])
    zfull = np.concatenate([edge_depths(poses, disps, intr, i, j)[0] for i, j in zip(GEOM_II, GEOM_JJ)])
    assert np.abs(z - R.MIN_DEPTH).min() > 1e-3 and np.abs(zfull - 0.01).min() > 1e-3      # no decision on a knife edge
    assert (zfull <= 0.01).any() and ((zfull > 0.01) & (zfull <= R.MIN_DEPTH)).any() and (zfull > R.MIN_DEPTH).any()
    bad = [DC.resolve_oob(v, nv) for v in DC.OOB]
    ii = [bad[0]] + GEOM_II[:3] + [2, bad[2]] + GEOM_II[3:6] + [bad[4]] + GEOM_II[6:] + [3]
    jj = [1] + GEOM_JJ[:3] + [bad[1], bad[3]] + GEOM_JJ[3:6] + [bad[0]] + GEOM_JJ[6:] + [bad[3]]
    good = R.kept_edges(ii, jj, nv)
    assert [ii[e] for e in good] == GEOM_II and [jj[e] for e in good] == GEOM_JJ
    out = [e for e in range(len(ii)) if e not in good]
    P, D, I = f32(poses), f32(disps), f32(intr)
    dist = droid_backends.frame_distance(P, D, I, i64(ii), i64(jj), 0.3)
    dist0 = droid_backends.frame_distance(P, D, I, i64(GEOM_II), i64(GEOM_JJ), 0.3)
    assert torch.isnan(dist[out]).all()
    assert torch.equal(dist[good], dist0)
    np.testing.assert_allclose(dist0.cpu().numpy(), R.frame_distance(poses, disps, intr, GEOM_II, GEOM_JJ, 0.3), rtol=1e-4, atol=1e-4)
    coords, valid = droid_backends.projmap(P, D, I, i64(ii), i64(jj))
    coords0, valid0 = droid_backends.projmap(P, D, I, i64(GEOM_II), i64(GEOM_JJ))
    assert torch.isnan(coords[out]).all() and torch.equal(valid[out], torch.zeros_like(valid[out]))
    assert torch.equal(coords[good], coords0) and torch.equal(valid[good], valid0)
    c_ref, v_ref = R.projmap(poses, disps, intr, ii, jj)
    assert np.isnan(c_ref[out]).all() and not v_ref[out].any()
    np.testing.assert_array_equal(valid0.cpu().numpy(), v_ref[good])
    np.testing.assert_allclose(coords0.cpu().numpy(), c_ref[good], rtol=1e-4, atol=2e-3)
    pts = droid_backends.iproj(P, D, I).cpu().numpy()
    np.testing.assert_allclose(pts, R.iproj(poses, disps, intr), rtol=1e-4, atol=1e-5)


def depth_filter_scene(ht, wd, n=10):
    rng, poses, _ = DC.scene(ht, wd, n, seed=80 + wd)
    disps = rng.uniform(0.45, 0.55, (n, ht, wd))          # a nearly planar scene, so neighbours agree often
    inds = [0, 2, n - 4, n - 1]                           # ix - 3 .. ix + 5 falls partly outside [0, n) for all but the second
    thresh = 0.05 * (1.0 / disps)[inds].mean(axis=(1, 2))
    return DC.r32(poses), DC.r32(disps), DC.r32(DC.intrinsics(ht, wd)), inds, DC.r32(thresh)


@pytest.mark.parametrize("shape", GEOM_SHAPES)
def test_depth_filter_counts_match_away_from_the_knife_edge(shape):
    import droid_backends
    poses, disps, intr, inds, thresh = depth_filter_scene(*shape)
    assert [len(R.depth_filter_neighbours(ix, len(disps))) for ix in inds] == [3, 5, 4, 3]
    ref, marg = R.depth_filter(poses, disps, intr, inds, thresh, margins=True)
    cnt = droid_backends.depth_filter(f32(poses), f32(disps), f32(intr), i64(inds), f32(thresh)).cpu().numpy()
    safe = marg > 1e-3
    assert safe.mean() > 0.5
    assert 0 < ref[safe].mean() < 6
    np.testing.assert_array_equal(cnt[safe], ref[safe])
