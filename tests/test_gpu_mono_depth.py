"""splat_slam_amd.mono_depth on the MI355X: a reduced network against the fp64 statement tests/mono_depth_ref.py, its error measured
against that of the torch autocast composition of the same weights (the criterion of tests/test_gpu_update_op.py), predict against
forward composed by hand, and the prior as Slam's mono_depth callable."""
import pytest
import torch

import mono_depth_ref as R
import vit_ref as VR

pytestmark = pytest.mark.gpu

DEV = "cuda"
SEED = 5


def reduced_cfg():
    from splat_slam_amd.mono_depth import MonoDepthConfig
    return MonoDepthConfig(stem_chs=32, stage_chs=(64, 128, 256), stage_layers=(1, 1, 2), gn_groups=8, dim=128, heads=2, depth=4, taps=(2, 3),
                           pos_grid=4, features=32, net_size=(64, 96))


@pytest.fixture(scope="module")
def models():
    from splat_slam_amd import mono_depth as M
    cfg = reduced_cfg()
    sd = M.synthetic_state_dict(SEED, cfg)
    prepared = R.prepare(sd)
    return cfg, M.MonoDepth.from_state_dict(sd, cfg, DEV), R.TorchMonoDepth(prepared, cfg, DEV), prepared


def make_image(B, H, W, seed):
    return (2 * torch.rand(B, 3, H, W, generator=torch.Generator().manual_seed(seed)) - 1).half().float().to(DEV)


@pytest.mark.parametrize("H,W", [(32, 32), (64, 96)])
def test_forward_is_as_close_to_the_fp64_oracle_as_the_autocast_composition(models, H, W):
    """at 32 x 32 the deepest map is one pixel, and the first fusion block upsamples it with align_corners=True"""
    cfg, model, torch_model, prepared = models
    x = make_image(2, H, W, H + W)
    got = model.forward(x)
    assert got.dtype == torch.float32 and tuple(got.shape) == (2, H, W) and torch.isfinite(got).all() and (got >= 0).all()
    oracle = R.mono_depth_ref(prepared, cfg, x)
    assert float(oracle.max()) > 0                                         # the head's ReLU leaves something to compare
    VR.check_against_oracle(f"mono-{H}x{W}", ("depth",), (got,), (torch_model(x),), (oracle,))
    assert torch.equal(model.forward(x), got)


def test_sizes_that_are_no_multiple_of_32_raise(models):
    model = models[1]
    with pytest.raises(ValueError, match="multiples of 32"):
        model.forward(make_image(1, 40, 64, 1))
    with pytest.raises(RuntimeError, match="GPU tensor"):
        model.forward(torch.zeros(1, 3, 32, 32))


def test_predict_is_forward_between_the_stated_resizes(models):
    model = models[1]
    image = torch.rand(1, 3, 48, 80, generator=torch.Generator().manual_seed(9)).to(DEV)
    got = model.predict(image)
    assert got.dtype == torch.float32 and tuple(got.shape) == (48, 80) and float(got.min()) >= 0 and float(got.max()) <= 1
    assert torch.equal(got, R.predict_by_hand(model, image)) and torch.equal(got, model(3.0, image))


def test_the_prior_is_slams_mono_depth_callable(models):
    """Slam constructs around it, and what Slam._mono returns for a frame of the stream is a map KeyframeDepth.put_mono accepts"""
    import numpy as np
    import test_gpu_slam as S
    import tracker_cases as T
    from splat_slam_amd.droid_net import DroidNet
    from splat_slam_amd.fused import FusedMappingLoop
    from splat_slam_amd.mono_depth import MonoDepth
    from splat_slam_amd.slam import Slam
    cfg = S.make_cfg()
    torch.manual_seed(43)
    np.random.seed(43)
    prior = MonoDepth.synthetic(SEED, reduced_cfg(), DEV)
    slam = Slam(cfg, DroidNet.synthetic(7, device=DEV), T.SyntheticStream(2), FusedMappingLoop(cfg, device=DEV), prior)
    timestamp, image, _, _ = slam.stream[0]
    mono = slam._mono(timestamp, image)
    assert tuple(mono.shape) == (T.HT, T.WD) and mono.dtype == torch.float32 and torch.isfinite(mono).all()
    assert float(mono.min()) >= 0 and float(mono.max()) <= 1
    assert torch.equal(mono, models[1].predict(image))                      # the same weights, the same bits
    slam.depth.put_mono(0, mono.contiguous())
    assert 0 in slam.depth.has_mono and torch.isfinite(slam.depth.mono_filled[0]).all()
