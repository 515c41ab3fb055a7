"""bench.py --dump-outputs: what the timed path leaves its caller, written as float32 / float64 .npy files within 64 MB (a seeded
sample of the per-Gaussian rows when the whole map would not fit), the same files for the same state."""
import os
import types

import numpy as np
import torch

import bench


def _loop(n, window=3, views=5):
    g = torch.Generator().manual_seed(1)
    r = lambda *s: torch.nn.Parameter(torch.randn(*s, generator=g))
    gm = types.SimpleNamespace(_xyz=r(n, 3), _features_dc=r(n, 1, 3), _features_rest=r(n, 0, 3), _opacity=r(n, 1), _scaling=r(n, 3),
                               _rotation=r(n, 4))
    cams = {}
    for uid in range(views):
        cams[uid] = types.SimpleNamespace(uid=uid, exposure_a=r(1), exposure_b=r(1), cam_rot_delta=r(3), cam_trans_delta=r(3))
    vis = {kf: (torch.rand(n, generator=g) > 0.5).long() for kf in range(window)}
    return types.SimpleNamespace(gaussians=gm, current_window=list(range(window)), occ_aware_visibility=vis, viewpoints=cams)


def _read(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def test_whole_map_when_it_fits(tmp_path):
    loop = _loop(1000)
    bench.dump_outputs(loop, str(tmp_path))
    a = _read(str(tmp_path))
    assert "gaussian_rows" not in a and "gaussians_f_rest" not in a          # (an empty tensor has nothing to compare)
    assert all(v.dtype in (np.float32, np.float64) for v in a.values())
    assert np.array_equal(a["gaussians_xyz"], loop.gaussians._xyz.detach().numpy())
    assert np.array_equal(a["gaussians_rotation"], loop.gaussians._rotation.detach().numpy())
    assert a["occ_aware_visibility"].shape == (1000, 3)
    assert np.array_equal(a["occ_aware_visibility"][:, 2], loop.occ_aware_visibility[2].float().numpy())
    assert a["keyframe_exposure_ab"].shape == (5, 2) and a["keyframe_pose_deltas"].shape == (5, 6)
    assert np.array_equal(a["keyframe_pose_deltas"][4, 3:], loop.viewpoints[4].cam_trans_delta.detach().numpy())


def test_seeded_sample_within_the_budget(tmp_path):
    loop = _loop(20000)
    budget = 1 << 20
    for d in ("a", "b"):
        bench.dump_outputs(loop, str(tmp_path / d), budget=budget)
    a, b = _read(str(tmp_path / "a")), _read(str(tmp_path / "b"))
    assert sum(os.path.getsize(str(tmp_path / "a" / f)) for f in os.listdir(str(tmp_path / "a"))) <= budget
    assert a.keys() == b.keys() and all(np.array_equal(a[k], b[k]) for k in a)
    rows = a["gaussian_rows"]
    assert rows.dtype == np.float64 and 0 < len(rows) < 20000 and np.all(np.diff(rows) > 0)
    idx = rows.astype(np.int64)
    assert np.array_equal(a["gaussians_scaling"], loop.gaussians._scaling.detach().numpy()[idx])
    assert np.array_equal(a["occ_aware_visibility"][:, 0], loop.occ_aware_visibility[0].float().numpy()[idx])
