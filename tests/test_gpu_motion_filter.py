"""splat_slam_amd.motion_filter on the MI355X: what the first frame leaves in the video, and the keyframe decision of later frames
against the same quantity computed by hand from the encoders, CorrBlock and the update operator."""
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
H, W = 40, 56
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


@pytest.fixture(scope="module")
def net():
    from splat_slam_amd.droid_net import DroidNet
    return DroidNet.synthetic(7, DEV)


def image(seed):
    return torch.rand(1, 3, H, W, generator=torch.Generator().manual_seed(seed)).to(DEV)


def make_filter(net, thresh=2.5, mono_depth=None):
    from splat_slam_amd.depth_video import DepthVideo
    from splat_slam_amd.motion_filter import MotionFilter
    video = DepthVideo(H, W, buffer=4, device=DEV)
    return MotionFilter(net, video, thresh=thresh, mono_depth=mono_depth, device=DEV), video


INTR = [50.0, 52.0, 28.0, 20.0]


def test_first_frame_is_always_appended(net):
    filt, video = make_filter(net, thresh=1e9)
    img = image(1)
    keep = img.clone()
    filt.track(3.0, img, torch.tensor(INTR, device=DEV))
    assert video.counter.value == 1 and filt.count == 0 and torch.equal(img, keep)
    fmap = net.fnet(img[None], MEAN, STD)
    ctx_net, ctx_inp = net.cnet.context(img[None], MEAN, STD)
    assert tuple(video.fmaps[0].shape) == (1, 128, 5, 7) and torch.equal(video.fmaps[0], fmap[0])
    assert torch.equal(video.nets[0], ctx_net[0, 0]) and torch.equal(video.inps[0], ctx_inp[0, 0])
    assert float(video.nets[0].float().std()) > 0.05 and float(video.inps[0].float().max()) > 0.05       # (not a comparison of zeros)
    assert video.poses[0].tolist() == [0, 0, 0, 0, 0, 0, 1] and bool((video.disps[0] == 1).all())
    assert float(video.timestamp[0]) == 3.0 and torch.equal(video.intrinsics[0], torch.tensor(INTR, device=DEV) / 8)
    assert not video.mono_disps.any()                                                               # no prior without a mono_depth


def decision_value(net, first, second):
    """mean flow magnitude of one update step between the maps of two frames, from the parts"""
    from splat_slam_amd.corr import CorrBlock
    fmap0, fmap1 = net.fnet(first[None], MEAN, STD), net.fnet(second[None], MEAN, STD)
    ctx_net, ctx_inp = net.cnet.context(first[None], MEAN, STD)
    y, x = torch.meshgrid(torch.arange(H // 8, device=DEV).float(), torch.arange(W // 8, device=DEV).float(), indexing="ij")
    corr = CorrBlock(fmap0, fmap1)(torch.stack([x, y], dim=-1)[None, None])
    _, delta, _ = net.update(ctx_net, ctx_inp, corr)
    return float(delta.float().norm(dim=-1).mean())


def test_second_frame_is_kept_or_dropped_at_the_threshold(net):
    a, b = image(1), image(2)
    value = decision_value(net, a, b)
    print("decision value:", value, " identical frame:", decision_value(net, a, a))
    assert value > 1e-3
    # just below: appended, count reset
    filt, video = make_filter(net, thresh=value * (1 - 1e-3))
    filt.count = 5
    filt.track(0.0, a, torch.tensor(INTR, device=DEV))
    filt.track(1.0, b, torch.tensor(INTR, device=DEV))
    assert video.counter.value == 2 and filt.count == 0
    assert torch.equal(video.fmaps[1], net.fnet(b[None], MEAN, STD)[0])
    ctx_net, ctx_inp = net.cnet.context(b[None], MEAN, STD)
    assert torch.equal(video.nets[1], ctx_net[0, 0]) and torch.equal(video.inps[1], ctx_inp[0, 0])
    assert float(video.timestamp[1]) == 1.0 and video.poses[1].tolist() == [0, 0, 0, 0, 0, 0, 1]     # pose and disparity left as they were
    assert torch.equal(filt.fmap, video.fmaps[1])                                                   # the new keyframe is compared next
    # just above: dropped, count up
    filt, video = make_filter(net, thresh=value * (1 + 1e-3))
    filt.track(0.0, a, torch.tensor(INTR, device=DEV))
    filt.track(1.0, b, torch.tensor(INTR, device=DEV))
    assert video.counter.value == 1 and filt.count == 1 and not video.fmaps[1].any()
    filt.track(2.0, b, torch.tensor(INTR, device=DEV))
    assert video.counter.value == 1 and filt.count == 2


def test_an_identical_second_frame_is_dropped(net):
    filt, video = make_filter(net)
    a = image(1)
    filt.track(0.0, a, torch.tensor(INTR, device=DEV))
    filt.track(1.0, a.clone(), torch.tensor(INTR, device=DEV))
    assert video.counter.value == 1 and filt.count == 1


def test_mono_depth_callable_fills_the_prior(net):
    depth = 1.0 + torch.rand(H, W, generator=torch.Generator().manual_seed(3)).to(DEV)
    depth[3, 3] = 0.0                                             # an invalid depth gives disparity 0
    seen = []

    def mono(tstamp, img):
        seen.append((tstamp, tuple(img.shape)))
        return depth

    filt, video = make_filter(net, mono_depth=mono)
    filt.track(7.0, image(1), torch.tensor(INTR, device=DEV))
    assert seen == [(7.0, (1, 3, H, W))]
    want = depth[3::8, 3::8]
    want = torch.where(want > 0, 1.0 / want, torch.zeros_like(want))
    assert torch.equal(video.mono_disps[0], want) and float(video.mono_disps[0, 0, 0]) == 0.0 and float(video.mono_disps[0].max()) > 0.5
    assert not video.mono_disps[1:].any()


def test_bad_image_raises(net):
    filt, _ = make_filter(net)
    with pytest.raises(RuntimeError, match=r"\[1,3,H,W\]"):
        filt.track(0.0, torch.zeros(3, H, W, device=DEV))
