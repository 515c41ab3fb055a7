"""What of the fused correlation volume can be checked without a GPU: the block-mean oracle of tests/corr_volume_ref.py against
successive avg_pool2d of its own fp64 level 0, and the argument checks of droid_backends.corr_volume_pyramid,
droid_backends.corr_index_pyramid_forward and splat_slam_amd.corr.FusedCorrBlock, which all raise before any launch."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import corr_volume_ref as V


@pytest.mark.parametrize("h,w", [(12, 16), (7, 9), (6, 8), (1, 1), (17, 24)])
def test_block_mean_oracle_equals_successive_avg_pool(h, w):
    rng = np.random.default_rng(h * 100 + w)
    maps = rng.normal(size=(4, 32, h, w))
    src, dst = [0, 1, 3, 7, -1], [1, 1, 2, 0, 0]
    pyr = V.volume_pyramid(maps, src, dst, 4)
    for kind in (0, 1):
        cur = torch.tensor(pyr[0][kind]).reshape(-1, 1, h, w)
        for l in range(4):
            got = pyr[l][kind]
            assert got.shape == (5, h, w, h >> l, w >> l)
            np.testing.assert_allclose(got.reshape(5 * h * w, h >> l, w >> l), cur[:, 0].numpy(), rtol=1e-13, atol=1e-13)
            if l < 3:
                cur = F.avg_pool2d(cur, 2, 2) if min(cur.shape[-2:]) >= 2 else cur.new_zeros(cur.shape[0], 1, cur.shape[2] // 2, cur.shape[3] // 2)
    assert not pyr[0][0][3].any() and not pyr[0][0][4].any() and pyr[0][0][0].any()      # planes outside [0, planes): zeros
    if (h, w) == (6, 8):
        assert pyr[3][0].size == 0
    if (h, w) == (7, 9):
        assert pyr[1][0].shape[-2:] == (3, 4)                                            # the odd row and column are dropped
    # level 0 from the definition, one element
    e, p1, p2 = 2, (h - 1, w - 1), (0, w // 2)
    want = (maps[3, :, p1[0], p1[1]] * maps[2, :, p2[0], p2[1]]).sum() / 16.0
    assert abs(pyr[0][0][e, p1[0], p1[1], p2[0], p2[1]] - want) <= 1e-12
    assert (pyr[0][1] >= np.abs(pyr[0][0]) - 1e-12).all()


def _levels(cap=3, h=6, w=8, n=4, dtype=torch.float16):
    return [torch.zeros((cap, h, w, h >> l, w >> l), dtype=dtype) for l in range(n)]


def test_wrappers_check_their_arguments_before_any_launch():
    import droid_backends as db
    maps = torch.zeros((4, 32, 6, 8), dtype=torch.float16)
    idx = torch.zeros(2, dtype=torch.int64)
    coords = torch.zeros((2, 6, 8, 2))
    with pytest.raises(RuntimeError, match="GPU tensor"):
        db.corr_volume_pyramid(maps, idx, idx, _levels(), idx)
    with pytest.raises(RuntimeError, match="GPU tensor"):
        db.corr_index_pyramid_forward(_levels(), idx, coords, 3)
    with pytest.raises(TypeError):
        db.corr_volume_pyramid(maps.float(), idx, idx, _levels(), idx)
    with pytest.raises(TypeError):
        db.corr_volume_pyramid(maps, idx, idx, _levels(dtype=torch.float32), idx)
    with pytest.raises(TypeError):
        db.corr_volume_pyramid(maps, idx.int(), idx, _levels(), idx)
    with pytest.raises(TypeError):
        db.corr_volume_pyramid(maps, idx, idx, _levels(), idx.int())
    with pytest.raises(ValueError, match="levels"):
        db.corr_volume_pyramid(maps, idx, idx, [], idx)
    with pytest.raises(ValueError, match="levels"):
        db.corr_volume_pyramid(maps, idx, idx, _levels(n=4) + _levels(n=1), idx)
    bad = _levels()
    bad[2] = torch.zeros((3, 6, 8, 2, 2), dtype=torch.float16)
    with pytest.raises(ValueError, match=r"levels\[2\]"):
        db.corr_volume_pyramid(maps, idx, idx, bad, idx)
    with pytest.raises(ValueError, match=r"levels\[2\]"):
        db.corr_index_pyramid_forward(bad, idx, coords, 3)
    with pytest.raises(ValueError, match="maps"):
        db.corr_volume_pyramid(maps[:, :, :5], idx, idx, _levels(), idx)             # not contiguous, and not 6 x 8
    with pytest.raises(ValueError, match="maps"):
        db.corr_volume_pyramid(torch.zeros((4, 32, 6, 9), dtype=torch.float16), idx, idx, _levels(), idx)
    with pytest.raises(ValueError, match="multiple of 32"):
        db.corr_volume_pyramid(torch.zeros((4, 48, 6, 8), dtype=torch.float16), idx, idx, _levels(), idx)
    with pytest.raises(ValueError, match="multiple of 32"):
        db.corr_volume_pyramid(torch.zeros((4, 2048, 6, 8), dtype=torch.float16), idx, idx, _levels(), idx)
    with pytest.raises(ValueError, match="same length"):
        db.corr_volume_pyramid(maps, idx, idx[:1], _levels(), idx)
    with pytest.raises(ValueError, match="slots"):
        db.corr_volume_pyramid(maps, idx, idx, _levels(), idx[:1])
    with pytest.raises(ValueError, match="coords"):
        db.corr_index_pyramid_forward(_levels(), idx, coords[:1], 3)
    with pytest.raises(ValueError, match="coords"):
        db.corr_index_pyramid_forward(_levels(), idx, coords.permute(0, 3, 1, 2).contiguous(), 3)
    with pytest.raises(TypeError):
        db.corr_index_pyramid_forward(_levels(), idx, coords.double(), 3)
    with pytest.raises(ValueError, match="radius"):
        db.corr_index_pyramid_forward(_levels(), idx, coords, 5)
    with pytest.raises(ValueError, match="radius"):
        db.corr_index_pyramid_forward(_levels(), idx, coords, -1)


def test_fused_block_checks_its_maps():
    from splat_slam_amd.corr import FusedCorrBlock
    with pytest.raises(TypeError, match="float16"):
        FusedCorrBlock(torch.zeros((3, 1, 32, 6, 8)))
    with pytest.raises(ValueError, match="frames,cams,C,h,w"):
        FusedCorrBlock(torch.zeros((3, 32, 6, 8), dtype=torch.float16))
    with pytest.raises(ValueError, match="num_levels"):
        FusedCorrBlock(torch.zeros((3, 1, 32, 6, 8), dtype=torch.float16), num_levels=5)
    with pytest.raises(ValueError, match="capacity"):
        FusedCorrBlock(torch.zeros((3, 1, 32, 6, 8), dtype=torch.float16), capacity=0)


def test_the_keyword_reaches_the_graph_and_its_default_is_volume():
    import inspect
    from splat_slam_amd.factor_graph import FactorGraph
    from splat_slam_amd.frontend import Frontend
    from splat_slam_amd.tracker import Tracker
    from splat_slam_amd.trajectory_filler import PoseTrajectoryFiller
    assert inspect.signature(FactorGraph.__init__).parameters["corr_impl"].default == "volume"
    assert inspect.signature(Frontend.__init__).parameters["corr_impl"].default == "volume"
    assert inspect.signature(PoseTrajectoryFiller.__init__).parameters["corr_impl"].default == "volume"
    assert inspect.signature(Tracker.__init__).parameters["frontend_corr_impl"].default == "volume"
