"""splat_slam_amd.slam.Slam on the MI355X: the tracker, the keyframe depth fusion and the mapping session joined in one process, over a
synthetic stream at 48 x 64 with a synthetic-weight DroidNet and a closed-form mono-depth callable.  What Slam hands to the mapper is
held bit for bit to a by-hand run (a Tracker with a recording callback over an identical video, KeyframeDepth.get at the same points):
the tracker is bit-deterministic and the mapper does not feed back into it."""
import copy

import numpy as np
import pytest
import torch

import tracker_cases as T

pytestmark = pytest.mark.gpu

DEV = "cuda"
N_STREAM = 10


def mono_depth(timestamp, image):
    """a smooth surface that drifts with the timestamp, a 4 x 4 patch of outliers and one pixel without a prior"""
    y, x = torch.meshgrid(torch.arange(T.HT, dtype=torch.float32, device=DEV), torch.arange(T.WD, dtype=torch.float32, device=DEV),
                          indexing="ij")
    m = 2.0 + 0.3 * torch.sin(0.2 * x + 0.1 * float(timestamp)) * torch.cos(0.15 * y)
    m[20:24, 40:44] *= 25.0
    m[35, 12] = 0.0
    return m


def make_cfg(final_ba=False):
    """the tracker configuration of tests/test_gpu_tracker.py's Tracker.run (every frame a keyframe, initialised after four) with a
    multi-view filter that accepts what an untrained network produces, and synthetic.DEFAULT_CONFIG's mapping part cut down"""
    from splat_slam_amd import synthetic as syn
    cfg = T.make_cfg(**{"tracking.warmup": 4, "tracking.motion_filter.thresh": 0.0, "tracking.frontend.keyframe_thresh": -1.0,
                        "tracking.frontend.enable_online_ba": True, "tracking.backend.ba_freq": 3, "mapping.every_keyframe": 1,
                        "tracking.multiview_filter.thresh": 1e6, "tracking.multiview_filter.visible_num": 1})
    cfg["cam"] = {"H_out": T.HT, "W_out": T.WD}
    cfg["tracking"]["backend"]["final_ba"] = final_ba
    mapping = copy.deepcopy(syn.DEFAULT_CONFIG["mapping"])
    tr = mapping["Training"]
    tr["init_itr_num"], tr["mapping_itr_num"], tr["window_size"] = 30, 4, 4
    tr["init_gaussian_update"], tr["init_gaussian_reset"] = 10, 10 ** 9
    mapping["opt_params"]["densify_from_iter"] = 10 ** 9
    mapping["final_refine_iters"] = 8
    cfg["mapping"].update(mapping)
    return cfg


def make_slam(final_ba=False):
    from splat_slam_amd.droid_net import DroidNet
    from splat_slam_amd.fused import FusedMappingLoop
    from splat_slam_amd.slam import Slam
    cfg = make_cfg(final_ba)
    torch.manual_seed(43)
    np.random.seed(43)
    return Slam(cfg, DroidNet.synthetic(7, device=DEV), T.SyntheticStream(N_STREAM), FusedMappingLoop(cfg, device=DEV), mono_depth)


def video_w2c(video, i):
    import lietorch
    return lietorch.SE3(video.poses[i:i + 1]).matrix()[0]


@pytest.fixture(scope="module")
def run():
    """one Slam run with final_ba on, everything the tests look at recorded on the way"""
    slam = make_slam(final_ba=True)
    rec = dict(process=[], prefetch=[], poses_agree=[], deform=[])
    process, source = slam.session.process, slam.session.pose_source
    prefetch = source.prefetch

    def process_(video_idx, idx, color, depth, w2c):
        rec["process"].append((video_idx, idx, color.clone(), depth.clone(), w2c.clone()))
        status = process(video_idx, idx, color, depth, w2c)
        if status == "mapped":
            earlier = [i for i in slam.session.video_idxs[:-1]]
            rec["poses_agree"].append((video_idx, [bool(torch.equal(slam.session.cameras[i].R, video_w2c(slam.video, i)[:3, :3])
                                                        and torch.equal(slam.session.cameras[i].T, video_w2c(slam.video, i)[:3, 3]))
                                                   for i in earlier]))
        return status

    def prefetch_(video_idxs):
        rec["prefetch"].append(list(video_idxs))
        return prefetch(video_idxs)

    slam.session.process, source.prefetch = process_, prefetch_
    slam.run()
    rec["log"] = list(slam.log)
    rec["prefetch_before_terminate"] = len(rec["prefetch"])
    rec["psnr"] = slam.terminate()
    return slam, rec


def test_slam_hands_the_mapper_what_a_by_hand_run_computes(run):
    from splat_slam_amd.depth_fusion import KeyframeDepth
    from splat_slam_amd.depth_video import DepthVideo
    from splat_slam_amd.droid_net import DroidNet
    from splat_slam_amd.tracker import Tracker
    slam, rec = run
    print("slam log:", rec["log"])
    status = [s for _, s in rec["log"]]
    assert status[0] == "init" and "mapped" in status and "invalid" not in status
    assert [i for i, _ in rec["log"]] == list(range(3, N_STREAM))
    # by hand: the tracker alone over an identical video, the fusion called where Slam calls it
    cfg = make_cfg(True)
    video = DepthVideo.from_config(cfg)
    kd, frames, by_hand = KeyframeDepth(video), {}, []

    def mono(timestamp, image):
        frames[float(timestamp)] = (image[0], mono_depth(timestamp, image))
        return frames[float(timestamp)][1]

    def on_keyframe(video_idx, timestamp):
        if video_idx is None:
            return
        color, m = frames[float(timestamp)]
        kd.put_mono(video_idx, m)
        depth, w2c, invalid = kd.get([video_idx])
        assert invalid == [False]
        by_hand.append((video_idx, timestamp, color, depth[0].clone(), w2c[0].clone()))

    Tracker(cfg, DroidNet.synthetic(7, device=DEV), video, on_keyframe=on_keyframe, mono_depth=mono).run(T.SyntheticStream(N_STREAM))
    assert len(by_hand) == len(rec["process"]) == len(rec["log"])
    for got, want in zip(rec["process"], by_hand):
        assert got[0] == want[0] and got[1] == want[1]
        for a, b in zip(got[2:], want[2:]):
            assert a.dtype == b.dtype and torch.equal(a, b), got[0]
    depth = rec["process"][-1][3]
    assert torch.isfinite(depth).all() and (depth > 0).all()             # the zero and the outliers of the mono map were filled


def test_a_mapped_keyframe_refreshes_every_earlier_camera_with_one_batched_fusion(run):
    slam, rec = run
    mapped = [i for i, s in rec["log"] if s == "mapped"]
    assert mapped and [i for i, _ in rec["poses_agree"]] == mapped
    for video_idx, agree in rec["poses_agree"]:
        assert agree and all(agree), (video_idx, agree)
    # one prefetch per mapped keyframe, over every keyframe registered so far (the newest included)
    assert rec["prefetch_before_terminate"] == len(mapped)
    seen = [i for i, _ in rec["log"]]
    for video_idx, asked in zip(mapped, rec["prefetch"]):
        assert asked == seen[:seen.index(video_idx) + 1]
    # ... and the video carries the fit of every keyframe that was fused
    assert (slam.video.depth_scale[seen] != 0).all()


def test_terminate_with_final_ba_returns_one_finite_psnr_per_viewpoint(run):
    slam, rec = run
    assert len(rec["prefetch"]) == rec["prefetch_before_terminate"] + 1   # the final update: one more batched fusion
    assert rec["prefetch"][-1] == [i for i, _ in rec["log"]]
    assert len(rec["psnr"]) == len(slam.session.loop.viewpoints) >= 2
    assert all(np.isfinite(rec["psnr"])), rec["psnr"]
    for i, cam in slam.session.cameras.items():                           # after the final bundle adjustment and the final update
        assert torch.equal(cam.R, video_w2c(slam.video, i)[:3, :3]) and torch.equal(cam.T, video_w2c(slam.video, i)[:3, 3])


def test_an_invalid_keyframe_is_registered_but_never_mapped_or_rescaled():
    from splat_slam_amd import session as session_mod
    slam = make_slam()
    on_keyframe, forced = slam.tracker.on_keyframe, 6
    deforms = []
    real = session_mod.update_mapping_points

    def on_keyframe_(video_idx, timestamp):
        if video_idx == forced:
            slam.video.valid_depth_mask[forced] = False                   # fewer than 100 valid pixels
        on_keyframe(video_idx, timestamp)

    def update_(gaussians, frame_idx, *args, method=None):
        deforms.append((frame_idx, method))
        return real(gaussians, frame_idx, *args, method=method)

    slam.tracker.on_keyframe = on_keyframe_
    session_mod.update_mapping_points = update_
    try:
        slam.run()
    finally:
        session_mod.update_mapping_points = real
    print("slam log with keyframe 6 forced invalid:", slam.log)
    assert dict(slam.log)[forced] == "invalid" and slam.session.is_kf[forced] is False
    assert forced in slam.session.cameras and forced not in slam.session.loop.viewpoints and forced not in slam.session.depth_dict
    after = [s for i, s in slam.log if i > forced]
    assert len(after) == N_STREAM - 1 - forced and "mapped" in after     # the run went on
    assert deforms and all(i != forced for i, _ in deforms)
    assert not (slam.session.loop.gaussians.unique_kfIDs == forced).any()


def test_a_session_with_a_two_tuple_pose_source_behaves_as_before():
    from splat_slam_amd import synthetic as syn
    from splat_slam_amd.fused import FusedMappingLoop
    from splat_slam_amd.session import MappingSession
    cfg = {"mapping": make_cfg()["mapping"]}
    intr = syn.INTRINSICS["tiny"]
    frames = syn.keyframe_stream(5, intr, DEV, n_world=20000, seed=5, sweep_deg=70.0)
    asked = []

    def run_session(pose_source):
        torch.manual_seed(43)
        np.random.seed(43)
        sess = MappingSession(FusedMappingLoop(cfg, device=DEV), intr, pose_source=pose_source)
        status = [sess.process(*f) for f in frames]
        return sess, status

    def two_tuple(video_idx):
        asked.append(video_idx)
        return frames[video_idx][4], frames[video_idx][3]               # (w2c, depth): the unchanged estimate

    class ThreeTuple:
        """the same estimate through the additive interface: announced once per mapped keyframe, flagged valid"""
        announced = []

        def prefetch(self, video_idxs):
            self.announced.append(list(video_idxs))

        def __call__(self, video_idx):
            return frames[video_idx][4], frames[video_idx][3], False

    a, status_a = run_session(two_tuple)
    mapped = [i for i, s in enumerate(status_a) if s == "mapped"]
    assert status_a[0] == "init" and mapped
    # asked for every keyframe registered so far at every mapped keyframe, one at a time
    assert asked == [k for i in mapped for k in range(i + 1)]
    assert sorted(a.depth_dict) == [i for i, s in enumerate(status_a) if s != "skipped"]
    for i, cam in a.cameras.items():
        assert torch.equal(cam.R, frames[i][4][:3, :3].to(DEV)) and torch.equal(cam.T, frames[i][4][:3, 3].to(DEV))
    source = ThreeTuple()
    b, status_b = run_session(source)
    assert status_b == status_a and source.announced == [list(range(i + 1)) for i in mapped]
    assert b.loop.gaussians.get_xyz.shape == a.loop.gaussians.get_xyz.shape and sorted(b.depth_dict) == sorted(a.depth_dict)
    c, status_c = run_session(None)
    assert status_c[0] == "init" and len(c.cameras) == 5
    # a mapped keyframe that later reports invalid: moved rigidly (no depth rescaling), and its reference depth is left alone
    from splat_slam_amd import session as session_mod
    moved = frames[0][4].clone()
    moved[:3, 3] += torch.tensor([0.01, -0.005, 0.008])
    other_depth = frames[0][3] * 1.1

    def invalid_first(video_idx):
        if video_idx == 0:
            return moved, other_depth, True
        return frames[video_idx][4], frames[video_idx][3] * 1.05, False

    deforms, real = [], session_mod.update_mapping_points

    def update_(gaussians, frame_idx, *args, method=None):
        deforms.append((frame_idx, method))
        return real(gaussians, frame_idx, *args, method=method)

    session_mod.update_mapping_points = update_
    try:
        d, status_d = run_session(invalid_first)
    finally:
        session_mod.update_mapping_points = real
    print("deformations with keyframe 0 reported invalid:", deforms, status_d)
    of_first = [m for i, m in deforms if i == 0]
    assert of_first and all(m == "rigid" for m in of_first)
    assert [m for i, m in deforms if i != 0] and all(m is None for i, m in deforms if i != 0)
    assert torch.equal(d.depth_dict[0], frames[0][3].to(DEV))                       # not replaced by the invalid frame's depth
    assert torch.equal(d.cameras[0].T, moved[:3, 3].to(DEV)) and torch.equal(d.cameras[0].depth, other_depth.to(DEV))
    later = [i for i in d.depth_dict if i != 0 and (i, None) in deforms]
    assert later and all(torch.equal(d.depth_dict[i], (frames[i][3] * 1.05).to(DEV)) for i in later)
