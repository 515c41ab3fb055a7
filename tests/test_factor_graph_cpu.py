"""The restatements of tests/factor_graph_ref.py checked against independent formulations, without a GPU: the two selections against a
brute-force repeated arg-min on small matrices (ties included), the reprojection against a pixel computed by hand and against the
identity G_i = G_j => coords = grid, the GPU test's scene against its own 1 % exclusion budget, and the bookkeeping on a short script."""
import numpy as np
import pytest
import torch

import factor_graph_ref as R


# ---- selection: brute force.  State is a matrix of live distances; every step takes the first minimum (np.argmin: lowest flat index).
def _brute(d, row0, col0, rows, cols, window, old, cut, thresh, max_factors, region, emit):
    d = np.array(d, np.float32).reshape(rows, cols).astype(np.float64)
    end = row0 + rows
    d[~(d <= np.float32(cut))] = np.inf
    for r in range(rows):
        for c in range(cols):
            if row0 + r - window < col0 + c:
                d[r, c] = np.inf
    dead = np.zeros((rows, cols), bool)
    for i, j in old:
        for rr, cc in region(i, j):
            if 0 <= rr - row0 < rows and 0 <= cc - col0 < cols:
                dead[rr - row0, cc - col0] = True
    es = []
    for i in range(row0, end):
        for j in range(max(i - window - 1, 0), i):
            es += [(i, j), (j, i)]
            if 0 <= j - col0 < cols:
                dead[i - row0, j - col0] = True
    loops = 0
    while True:
        live = np.where(dead, np.inf, d)
        k = int(np.argmin(live))
        if not live.reshape(-1)[k] <= np.float32(thresh) or len(es) > max_factors:
            break
        i, j = row0 + k // cols, col0 + k % cols
        new = emit(i, j)
        es += new
        loops += len(new)
        for rr, cc in region(i, j):
            if 0 <= rr - row0 < rows and 0 <= cc - col0 < cols:
                dead[rr - row0, cc - col0] = True
    return es, loops


def _brute_front(d, t0, t1, t, ii_old, jj_old, rad, nms, thresh, max_factors):
    def region(i, j):
        r = max(min(abs(i - j) - 2, nms), 0)
        return [(i + a, j + b) for a in range(-r, r + 1) for b in range(-r, r + 1) if abs(a) + abs(b) <= r]
    return _brute(d, t0, t1, t - t0, t - t1, rad, list(zip(ii_old, jj_old)), 100.0, thresh, max_factors, region,
                  lambda i, j: [(i, j), (j, i)])[0]


def _brute_back(d, t_start, t_end, tsl, loop, nms, radius, thresh, max_factors):
    tsl = tsl if loop else t_start
    raw = np.array(d, np.float32).reshape(t_end - tsl, t_end - t_start)

    def region(i, j):
        return [(i + a, j + b) for a in range(-nms, nms + 1) for b in range(-nms, nms + 1)]

    def emit(i, j):
        if not loop:
            return [(i, j), (j, i)]
        return [(si, sj) for si in range(i - 1, i + 2) for sj in range(j - 1, j + 2)
                if tsl <= si < t_end and t_start <= sj < t_end and raw[si - tsl, sj - t_start] <= np.float32(thresh) and si - sj > 20]
    return _brute(d, tsl, t_start, t_end - tsl, t_end - t_start, radius, [], thresh, thresh, max_factors, region, emit)


def _matrix(rng, rows, cols, levels=None):
    d = rng.uniform(0.0, 30.0, size=rows * cols).astype(np.float32)
    if levels:
        d = (np.floor(d / 30.0 * levels) * (30.0 / levels)).astype(np.float32)
    return d


@pytest.mark.parametrize("levels", [None, 8, 2])
def test_proximity_reference_equals_the_brute_force(levels):
    rng = np.random.default_rng(3)
    for t0, t1, t, rad, nms, thresh, mf in [(0, 0, 1, 2, 2, 16.0, 10), (2, 0, 9, 2, 2, 16.0, 40), (3, 1, 12, 1, 1, 25.0, 30),
                                            (0, 0, 14, 2, 3, 20.0, 48), (4, 2, 15, 3, 2, 12.0, 1000), (0, 0, 10, 2, 2, 16.0, -1),
                                            (1, 1, 11, 0, 0, 29.0, 60)]:
        d = _matrix(rng, t - t0, t - t1, levels)
        d[rng.integers(0, d.size, size=d.size // 10)] = np.nan
        d[rng.integers(0, d.size, size=d.size // 10)] = np.inf
        old = rng.integers(-2, t + 2, size=(5, 2))
        got = R.proximity_edges(d, t0, t1, t, old[:, 0], old[:, 1], rad, nms, thresh, mf)
        assert got == _brute_front(d, t0, t1, t, old[:, 0], old[:, 1], rad, nms, thresh, mf), (t0, t1, t, rad, nms, thresh, mf)


@pytest.mark.parametrize("levels", [None, 8, 2])
@pytest.mark.parametrize("loop", [False, True])
def test_backend_reference_equals_the_brute_force(levels, loop):
    rng = np.random.default_rng(4)
    for t_start, t_end, tsl, nms, radius, thresh, mf in [(0, 1, 0, 1, 1, 10.0, 10), (0, 30, 22, 2, 1, 18.0, 60), (2, 34, 25, 1, 2, 25.0, 1000),
                                                         (0, 28, 24, 0, 1, 29.0, 70), (1, 33, 27, 3, 1, 15.0, 20)]:
        rows = t_end - (tsl if loop else t_start)
        d = _matrix(rng, rows, t_end - t_start, levels)
        d[rng.integers(0, d.size, size=d.size // 10)] = np.nan
        got = R.backend_edges(d, t_start, t_end, tsl, loop, nms, radius, thresh, mf)
        want = _brute_back(d, t_start, t_end, tsl, loop, nms, radius, thresh, mf)
        assert got[0] == want[0], (t_start, t_end, tsl, nms, radius, thresh, mf)
        assert got[1] == (want[1] if loop else 0)
        if loop:
            assert all(i - j > 20 for i, j in got[0][-got[1]:]) or got[1] == 0


def test_selection_edge_cases_of_the_reference():
    assert R.proximity_edges([1.0], 0, 0, 1, [], [], 2, 2, 16.0, 10) == []                          # 1 x 1: i - rad < j
    d = np.full(36, 5.0, np.float32)
    es = R.proximity_edges(d, 0, 0, 6, [], [], 1, 0, 16.0, 1000)                                    # all ties: flat-index order
    local = [p for i in range(6) for j in range(max(i - 2, 0), i) for p in ((i, j), (j, i))]
    assert es[:len(local)] == local
    assert es[len(local):] == [p for i in range(6) for j in range(0, i - 2) for p in ((i, j), (j, i))]
    assert R.proximity_edges(d, 0, 0, 6, [], [], 1, 0, 4.0, 1000) == local                          # thresh below every entry
    assert R.proximity_edges(np.full(36, np.nan), 0, 0, 6, [], [], 1, 0, 16.0, 1000) == local
    stopped = R.proximity_edges(d, 0, 0, 6, [], [], 1, 0, 16.0, len(local) + 1)                     # stops once len > max_factors
    assert stopped == es[:len(local) + 2]


# ---- reprojection
def test_reprojection_of_one_pixel_by_hand():
    """Frame 0 at the origin, frame 1 shifted by t = (0.5, 0, 0.25) without rotation.  Pixel (x, y) = (3, 1), disparity 0.5, intrinsics
    0: (4, 4, 1, 1), 1: (8, 2, 2, 3).  X0 = ((3-1)/4, (1-1)/4, 1) = (0.5, 0, 1); X1 = X0 + 0.5 t = (0.75, 0, 1.125);
    coords = (8 * 0.75 / 1.125 + 2, 2 * 0 / 1.125 + 3) = (22/3, 3).  Every input is a dyadic number, so fp64 is exact up to the division."""
    poses = np.array([[0, 0, 0, 0, 0, 0, 1], [0.5, 0, 0.25, 0, 0, 0, 1]], np.float32)
    disps = np.full((2, 2, 4), 0.5, np.float32)
    intr = np.array([[4, 4, 1, 1], [8, 2, 2, 3]], np.float32)
    out = R.reproject(poses, disps, intr, [0, 0, 0], [1, 0, 5])
    assert abs(out["coords"][0, 1, 3, 0] - 22.0 / 3.0) < 1e-14 and out["coords"][0, 1, 3, 1] == 3.0
    assert out["z"][0, 1, 3] == 1.125 and out["valid"][0, 1, 3, 0] == 1.0
    # the stereo edge: X1 = X0 + 0.5 * (-0.1f, 0, 0), projected with frame 0's own intrinsics
    assert abs(out["coords"][1, 1, 3, 0] - (4 * (0.5 + 0.5 * float(np.float32(-0.1))) + 1)) < 1e-14
    assert not out["coords"][2].any() and not out["valid"][2].any() and not out["bound"][2].any()   # out of range
    # magnitude of the x coordinate: |fx_j| (M(X1.x) / Z + |X1.x| M(Z) / Z^2) + |cx_j| with M(X1.x) = (3+1)/4 + 0.25, M(Z) = 1.125
    M = 8 * (1.25 / 1.125 + 0.75 * 1.125 / 1.125 ** 2) + 2
    assert abs(out["bound"][0, 1, 3, 0] - R.C_COORDS * R.U32 * M) < 1e-18


def test_equal_poses_reproject_onto_the_grid_and_points_behind_take_z_one():
    rng = np.random.default_rng(0)
    pose = np.array([0.3, -0.2, 0.1, 0.1, -0.3, 0.2, 0.0], np.float32)
    pose[6] = np.sqrt(1 - (pose[3:6] ** 2).sum())
    poses = np.stack([pose, pose])
    disps = rng.uniform(0.2, 2.0, size=(2, 5, 7)).astype(np.float32)
    intr = np.tile(np.array([6.0, 5.0, 3.5, 2.5], np.float32), (2, 1))
    out = R.reproject(poses, disps, intr, [0], [1])
    gy, gx = np.meshgrid(np.arange(5.0), np.arange(7.0), indexing="ij")
    assert np.abs(out["coords"][0, ..., 0] - gx).max() < 1e-6 and np.abs(out["coords"][0, ..., 1] - gy).max() < 1e-6
    assert (out["bound"][0] > 0).all() and out["bound"][0].max() < 1e-4
    # identity -> (t = (0.2, 0, 0.3), half a turn about y): X1 = (-X, Y, -1) + t d, behind the camera, so Z = 1 and nothing is divided
    poses = np.array([[0, 0, 0, 0, 0, 0, 1], [0.2, 0, 0.3, 0, 1, 0, 0]], np.float32)
    back = R.reproject(poses, disps, intr, [0], [1])
    d = disps[0].astype(np.float64)
    t = poses[1, :3].astype(np.float64)
    assert np.abs(back["z"][0] - (-1 + t[2] * d)).max() < 1e-15 and (back["z"] < 0.1).all() and not back["valid"].any()
    assert np.abs(back["coords"][0, ..., 0] - (6.0 * (-(gx - 3.5) / 6.0 + t[0] * d) + 3.5)).max() < 1e-14
    assert np.abs(back["coords"][0, ..., 1] - (5.0 * ((gy - 2.5) / 5.0) + 2.5)).max() < 1e-14


@pytest.mark.parametrize("h,w", [(6, 8), (11, 13)])
def test_the_gpu_scene_keeps_its_exclusions_under_one_percent(h, w):
    poses, disps, intr, ii, jj, target = R.reproject_case(h, w, 5)
    out = R.reproject(poses, disps, intr, ii, jj)
    assert out["near_valid"].mean() <= 0.01 and out["near_branch"].mean() <= 0.01
    assert (out["z"][3] < 0.1).all() and (out["z"][:3] > 0.2).all()                         # (1,4) is behind; the others in front
    assert not out["coords"][4].any()
    assert (np.abs(target - out["coords"]) > 64).any() and (np.abs(target - out["coords"]) < 64).any()
    assert len(set(map(tuple, intr))) == 5 and (ii[0], jj[0]) == (ii[2], jj[2]) and ii[1] == jj[1]
    assert out["bound"][:4].max() < 0.05                                                    # a bound that holds something


# ---- bookkeeping
def test_book_follows_a_short_script():
    b = R.Book(max_factors=8)
    b.add_neighborhood_factors(0, 4, r=2)
    assert list(zip(b.ii, b.jj)) == [(0, 1), (0, 2), (1, 0), (1, 2), (1, 3), (2, 0), (2, 1), (2, 3), (3, 1), (3, 2)]
    b.add_factors([0, 0, 3], [1, 3, 0])                                                     # (0,1) is a duplicate
    assert len(b.ii) == 12 and b.age == [0] * 12
    b.tick()
    b.filter_edges([1.0] * 10 + [0.0, 0.0])                                                 # (0,3) and (3,0) are distant and weak
    assert (b.ii_bad, b.jj_bad) == ([0, 3], [3, 0]) and len(b.ii) == 10
    b.add_factors([4, 4], [3, 2], remove=True)                                              # 12 > 8: rank[k] >= 6 by position
    assert list(zip(b.ii_inac, b.jj_inac)) == [(2, 1), (2, 3), (3, 1), (3, 2)]
    assert b.age == [1] * 6 + [0, 0]
    b.add_factors([2], [1])                                                                 # inactive edges are duplicates too
    assert len(b.ii) == 8
    b.rm_keyframe(1)
    assert list(zip(b.ii, b.jj)) == [(0, 1), (1, 0), (3, 2), (3, 1)] and list(zip(b.ii_inac, b.jj_inac)) == [(1, 2), (2, 1)]


def test_module_refuses_cpu_tensors_and_oversized_matrices_before_any_launch():
    from splat_slam_amd import factor_graph as fg
    poses, disps, intr = torch.zeros(2, 7), torch.ones(2, 3, 4), torch.ones(2, 4)
    e = torch.zeros(1, dtype=torch.long)
    with pytest.raises(RuntimeError, match="GPU tensor"):
        fg.reproject(poses, disps, intr, e, e)
    with pytest.raises(ValueError, match="per frame"):
        fg.reproject(poses, disps, torch.ones(3, 4), e, e)
    with pytest.raises(TypeError, match="int64"):
        fg.reproject(poses, disps, intr, e.int(), e)
    with pytest.raises(ValueError, match="target must be"):
        fg.reproject(poses, disps, intr, e, e, torch.zeros(1, 3, 4, 3))
    with pytest.raises(ValueError, match="exceeds the supported 512 x 512"):
        fg.select_proximity_edges(torch.zeros(513 * 4), 0, 509, 513, e, e, 2, 2, 16.0, 10)
    with pytest.raises(ValueError, match="exceeds the supported 512 x 512"):
        fg.select_backend_edges(torch.zeros(513 * 513), 0, 513, None, False, 2, 1, 16.0, 10)
    with pytest.raises(ValueError, match="entries"):
        fg.select_proximity_edges(torch.zeros(10), 0, 0, 4, e, e, 2, 2, 16.0, 10)
    with pytest.raises(ValueError, match="finite"):
        fg.select_proximity_edges(torch.zeros(16), 0, 0, 4, e, e, 2, 2, float("inf"), 10)
    with pytest.raises(RuntimeError, match="GPU tensor"):
        fg.select_proximity_edges(torch.zeros(16), 0, 0, 4, e, e, 2, 2, 16.0, 10)
    with pytest.raises(RuntimeError, match="GPU tensor"):
        fg.select_backend_edges(torch.zeros(16), 0, 4, None, False, 2, 1, 16.0, 10)
