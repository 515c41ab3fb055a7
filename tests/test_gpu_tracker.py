"""The tracker loop on the MI355X: FactorGraph.update_lowmem with corr_impl "alt_fused" and "alt", Backend, Frontend, PoseTrajectoryFiller
and Tracker, on the twelve-keyframe 48 x 64 video of tests/test_gpu_factor_graph.py (tracker_cases.make_video).  The classes are held,
bit for bit, to the same FactorGraph / DepthVideo calls made by hand on a second, identical video: what they add is the order of the
calls, so that is what is compared.  Where the lookup matters (6, 7) the update operator is tracker_cases.stub_corr, whose flow is a
function of the correlation features; elsewhere it is the stub of test_gpu_factor_graph.py."""
import types

import numpy as np
import pytest
import torch

import se3_ref as R
from tracker_cases import DEV, N_FRAMES, SyntheticStream, make_cfg, make_video, net_of, stub, stub_corr

pytestmark = pytest.mark.gpu


def same_video(v, u, masks=True):
    assert torch.equal(v.poses, u.poses) and torch.equal(v.disps, u.disps) and torch.equal(v.disps_up, u.disps_up)
    assert torch.isfinite(v.poses).all() and torch.isfinite(v.disps).all()
    if masks:
        assert torch.equal(v.valid_depth_mask, u.valid_depth_mask) and torch.equal(v.dirty, u.dirty)
        assert torch.equal(v.npc_dirty, u.npc_dirty) and v.counter.value == u.counter.value


def same_graph(g, h):
    for name in ("ii", "jj", "age", "target", "weight", "net", "ii_inac", "jj_inac", "target_inac", "weight_inac", "ii_bad", "jj_bad"):
        assert torch.equal(getattr(g, name), getattr(h, name)), name


# ---- 6. the low-memory update
def by_hand_lowmem(u, block, op, net, target, weight, ii, jj, t0, t1, steps):
    """the stages of FactorGraph.update_lowmem on the video u: reproject, per chunk of 8 source frames the lookup, the operator and the
    upsampling, then bundle adjustment"""
    from splat_slam_amd import factor_graph as fg
    num, rig, ch, ht, wd = u.fmaps.shape
    corr_op = block(u.fmaps.view(1, num * rig, ch, ht, wd))
    damp = 1e-6 * torch.ones_like(u.disps)
    for step in range(steps):
        coords, _, motn = fg.reproject(u.poses, u.disps, u.intrinsics, ii, jj, target[0].contiguous())
        for first in range(0, int(jj.max()) + 1, 8):
            c = (ii >= first) & (ii < first + 8)
            if int(c.sum()) < 1:
                continue
            corr = corr_op(coords[None][:, c], ii[c], jj[c])
            assert tuple(corr.shape) == (1, int(c.sum()), 4 * 49, ht, wd) and corr.any()
            with torch.autocast("cuda", enabled=True):
                n, delta, w, damping, upmask = op(net[:, c], u.inps[None, ii[c]], corr, motn[None][:, c], ii[c], jj[c])
                u.upsample(torch.unique(ii[c]), upmask)
            net[:, c], target[:, c], weight[:, c] = n, coords[None][:, c] + delta.float(), w.float()
            damp[torch.unique(ii[c])] = damping
        eta = .2 * damp[torch.unique(ii)].contiguous() + 1e-7
        u.ba(target, weight, eta, ii, jj, t0, t1, iters=2, lm=1e-5, ep=1e-2, motion_only=False,
             opt_type="pose_depth" if step % 2 == 0 else "depth_scale")
    return net, target, weight


@pytest.mark.parametrize("impl", ["alt_fused", "alt"])
def test_update_lowmem_equals_its_stages_called_by_hand(impl):
    from splat_slam_amd import factor_graph as fg
    from splat_slam_amd.corr import AltCorrBlock, FusedAltCorrBlock
    v, u = make_video(), make_video()
    g = fg.FactorGraph(v, stub_corr, device=DEV, corr_impl=impl, max_factors=-1)
    g.add_neighborhood_factors(0, 12, r=2)                                     # source frames 0..11: the chunks [0, 8) and [8, 16)
    ii, jj = g.ii.clone(), g.jj.clone()
    assert g.corr is None and g.inp is None
    net, target, weight = g.net.clone(), g.target.clone(), g.weight.clone()
    g.update_lowmem(t0=1, t1=12, itrs=2, steps=2)
    block = FusedAltCorrBlock if impl == "alt_fused" else AltCorrBlock
    net, target, weight = by_hand_lowmem(u, block, stub_corr, net, target, weight, ii, jj, 1, 12, 2)
    assert torch.equal(g.target, target) and torch.equal(g.weight, weight) and torch.equal(g.net, net)
    same_video(v, u)
    assert not torch.equal(v.poses[1:12], make_video().poses[1:12]) and g.age.tolist() == [0] * len(ii)
    # the operator's flow really is a function of the lookup: without it the targets differ
    w = make_video()
    plain = fg.FactorGraph(w, stub, device=DEV, corr_impl=impl, max_factors=-1)
    plain.add_neighborhood_factors(0, 12, r=2)
    plain.update_lowmem(t0=1, t1=12, itrs=2, steps=2)
    assert not torch.equal(plain.target, g.target)


# ---- 7. the backend
def test_dense_ba_equals_the_hand_called_sequence():
    from splat_slam_amd.backend import Backend
    from splat_slam_amd.factor_graph import FactorGraph
    cfg = make_cfg()
    be_cfg = cfg["tracking"]["backend"]
    v, u = make_video(), make_video()
    be = Backend(net_of(stub_corr), v, cfg)
    assert be.corr_impl == "alt_fused"
    graphs, make = [], be._graph
    be._graph = lambda mf: (graphs.append(make(mf)), graphs[-1])[1]
    n, n_edges = be.dense_ba(2)
    mf = ((be_cfg["radius"] + 2) * 2) * 12
    assert (n, len(graphs)) == (12, 1) and n_edges >= 3
    g = graphs[0]
    assert g.ii is None and g.target is None and g.net is None and g.max_factors == mf and g.corr_impl == "alt_fused"      # released
    assert not v.dirty[:12].any() and v.npc_dirty[:12].all() and not v.npc_dirty[12:].any()
    u.normalize()
    h = FactorGraph(u, stub_corr, device=DEV, corr_impl="alt_fused", max_factors=mf)
    num = h.add_backend_proximity_factors(0, 12, be_cfg["nms"], be_cfg["radius"], be_cfg["thresh"], mf, cfg["tracking"]["beta"], 0, False)
    assert num == n_edges == h.ii.shape[0]
    h.update_lowmem(t0=1, t1=12, itrs=2, use_inactive=False, steps=2, enable_wq=True)
    h.clear_edges()
    u.set_dirty(0, 12)
    u.update_valid_depth_mask()
    same_video(v, u)
    fresh = make_video()
    assert not torch.equal(v.poses[1:12], fresh.poses[1:12])
    with pytest.raises(ValueError, match="corr_impl"):
        Backend(net_of(stub), v, cfg, corr_impl="volume")


def test_loop_ba_without_a_loop_edge_leaves_the_video_untouched():
    from splat_slam_amd.backend import Backend
    from splat_slam_amd.factor_graph import FactorGraph
    cfg = make_cfg(**{"tracking.backend.loop_thresh": -1.0, "tracking.backend.loop_window": 5})
    v, fresh = make_video(), make_video()
    be = Backend(net_of(stub_corr), v, cfg)
    assert be.loop_ba(0, 12, steps=2) == (5, 0)
    same_video(v, fresh)
    local = FactorGraph(v, stub, device=DEV, max_factors=30)
    local.add_neighborhood_factors(0, 6, r=1)
    kept = {k: getattr(local, k).clone() for k in ("ii", "jj", "age", "net", "target", "weight")}
    graphs, make = [], be._graph
    be._graph = lambda mf: (graphs.append(make(mf)), graphs[-1])[1]
    assert be.loop_ba(0, 12, steps=2, local_graph=local) == (5, 0)
    assert graphs[0].max_factors == 8 * 5 and graphs[0].ii is None
    for k, t in kept.items():
        assert torch.equal(getattr(local, k), t), k
    same_video(v, fresh)


# ---- 8. the frontend
def hand_initialize(u, cfg):
    from splat_slam_amd.factor_graph import FactorGraph
    fe, warmup = cfg["tracking"]["frontend"], cfg["tracking"]["warmup"]
    g = FactorGraph(u, stub, device=DEV, corr_impl="volume", max_factors=fe["max_factors"])
    t1 = u.counter.value
    g.add_neighborhood_factors(0, t1, r=3)
    for _ in range(8):
        g.update(1, use_inactive=True, opt_type="pose_depth")
    g.add_proximity_factors(0, 0, rad=2, nms=2, thresh=fe["thresh"], remove=False)
    for _ in range(8):
        g.update(1, use_inactive=True, opt_type="pose_depth")
    u.poses[t1] = u.poses[t1 - 1].clone()
    u.disps[t1] = u.disps[t1 - 4:t1].mean()
    u.set_dirty(0, t1)
    g.rm_factors(g.ii < warmup - 4, store=True)
    u.update_valid_depth_mask()
    return g, t1


def hand_update(u, g, t1, cfg):
    tr, fe = cfg["tracking"], cfg["tracking"]["frontend"]
    t1 += 1
    g.rm_factors(g.age > tr["max_age"], store=True)
    g.add_proximity_factors(t1 - 5, max(t1 - fe["window"], 0), rad=fe["radius"], nms=fe["nms"], thresh=fe["thresh"], beta=tr["beta"],
                            remove=True)
    for itr in range(8):
        g.update(None, None, use_inactive=True, opt_type="pose_depth" if itr % 2 == 0 else "depth_scale")
    d = u.distance([t1 - 2], [t1 - 1], beta=tr["beta"], bidirectional=True).item()
    if d < fe["keyframe_thresh"]:
        g.rm_keyframe(t1 - 1)
        u.counter.value -= 1
        t1 -= 1
    else:
        for itr in range(4):
            g.update(None, None, use_inactive=True, opt_type="pose_depth" if itr % 2 == 0 else "depth_scale")
    u.poses[t1] = u.poses[t1 - 1]
    u.disps[t1] = u.disps[t1 - 1].mean()
    u.set_dirty(g.ii.min(), t1)
    u.update_valid_depth_mask()
    return t1, d


def initialized_pair(cfg):
    from splat_slam_amd.frontend import Frontend
    v, u = make_video(), make_video()
    v.counter.value = u.counter.value = 8                                       # the frames 8..11 wait in the buffer
    fr = Frontend(net_of(stub), v, cfg)
    assert (fr.t1, fr.is_initialized, fr.iters1, fr.iters2, fr.max_age, fr.warmup) == (0, False, 8, 4, 50, 8)
    assert fr.graph.corr_impl == "volume" and fr.graph.max_factors == 75 and fr.loop_closing.corr_impl == "alt_fused"
    before = v.poses.clone()
    v.counter.value = 7
    fr()                                                                        # not yet: nothing happens
    assert not fr.is_initialized and torch.equal(v.poses, before) and fr.graph.ii.shape[0] == 0
    v.counter.value = 8
    fr()
    h, t1 = hand_initialize(u, cfg)
    return fr, v, u, h, t1


def test_frontend_initialises_at_warmup():
    cfg = make_cfg()
    fr, v, u, h, t1 = initialized_pair(cfg)
    assert fr.is_initialized and fr.t1 == 8 == t1 and v.counter.value == 8
    assert torch.equal(v.poses[8], v.poses[7]) and torch.equal(v.disps[8], v.disps[4:8].mean().expand(6, 8))
    assert int(fr.graph.ii.min()) >= 4 and fr.graph.ii_inac.shape[0] > 0 and int(fr.graph.ii_inac.max()) < 4
    assert torch.equal(fr.last_pose, v.poses[7]) and torch.equal(fr.last_disp, v.disps[7]) and float(fr.last_time) == 7.0
    assert not v.dirty.any() and v.npc_dirty[:8].all()
    same_graph(fr.graph, h)
    same_video(v, u)
    fr()                                                                        # t1 == counter: nothing to do
    same_graph(fr.graph, h)
    same_video(v, u)


@pytest.mark.parametrize("keep", [False, True])
def test_frontend_update_drops_or_keeps_the_new_keyframe(keep):
    cfg = make_cfg(**{"tracking.frontend.keyframe_thresh": -1.0 if keep else 1e9})
    fr, v, u, h, t1 = initialized_pair(cfg)
    v.counter.value = u.counter.value = 9
    fr()
    t1, d = hand_update(u, h, t1, cfg)
    assert np.isfinite(d) and d > 0
    if keep:
        assert fr.t1 == 9 == t1 and v.counter.value == 9
        assert torch.equal(v.poses[9], v.poses[8]) and torch.equal(v.disps[9], v.disps[8].mean().expand(6, 8))
        assert int(fr.graph.ii.max()) == 8 and fr.graph.age.min() >= 12        # 8 + 4 updates since the newest edges came
    else:
        assert fr.t1 == 8 == t1 and v.counter.value == 8
        for name in ("ii", "jj", "ii_inac", "jj_inac"):
            assert int(getattr(fr.graph, name).max()) < 8, name
        assert torch.equal(v.poses[8], v.poses[7]) and torch.equal(v.disps[8], v.disps[7].mean().expand(6, 8))
    same_graph(fr.graph, h)
    same_video(v, u)


# ---- 9. the trajectory filler
def host(t):
    return t.detach().cpu().numpy()


def held(name, got, ref):
    val, mag, units = ref
    r = float((np.abs(host(got).astype(np.float64) - val) / R.bound(mag, units)).max())
    print(f"filler stage {name}: worst |err| / bound {r:.3f}")
    assert r <= 1.0, name


def test_interpolation_stage_by_stage_and_at_the_keyframes():
    """interpolate is lietorch's inv, mul, log, exp and mul with two scalings between: it must equal those calls bit for bit, and every
    one of them is held to the per-element bound units * 2^-24 * magnitude of tests/se3_ref.py (C_INV_T, C_MUL_*, C_LOG_*, C_EXP_*), the
    tolerance tests/test_gpu_se3.py holds exp, log and mul to, each against the fp64 oracle fed the fp32 output of the stage before.
    The scaling w = v / dt * (t - ts[t0]), with t the fp32 timestamp, is held to 6 roundings of |w|: dt = ts[t1] - ts[t0] + 1e-3 has two
    (the difference is exact for these timestamps; the constant in fp32, the sum), the division and the product one each,
    t - ts[t0] one."""
    from lietorch import SE3
    from splat_slam_amd.trajectory_filler import PoseTrajectoryFiller, bracket
    v = make_video()
    filler = PoseTrajectoryFiller(types.SimpleNamespace(fnet=None, update=None), v, device=DEV)
    times = [0.0, 0.25, 3.5, 7.0, 10.999, 11.0, 12.5, 5.001, 1.75, 9.125, 3.0]
    got = filler.interpolate(times)
    assert tuple(got.shape) == (len(times), 7) and got.dtype == torch.float32
    ts, tt = v.timestamp[:N_FRAMES], torch.tensor(times, device=DEV)
    t0, t1 = bracket(ts, tt)
    assert t0.tolist() == [0, 0, 3, 7, 10, 11, 11, 5, 1, 9, 3] and t1.tolist() == [1, 1, 4, 8, 11, 11, 11, 6, 2, 10, 4]
    P = v.poses[:N_FRAMES]
    P0, P1 = P[t0].contiguous(), P[t1].contiguous()
    P0i = SE3(P0).inv().data
    held("inv", P0i, R.inv(host(P0)))
    rel = (SE3(P1) * SE3(P0i)).data
    held("mul", rel, R.mul(host(P1), host(P0i)))
    lg = SE3(rel).log()
    held("log", lg, R.log(host(rel)))
    dt = ts[t1] - ts[t0] + 1e-3
    w = lg / dt[:, None] * (tt - ts[t0])[:, None]
    dt64 = host(ts[t1]).astype(np.float64) - host(ts[t0]).astype(np.float64) + 1e-3
    w64 = host(lg).astype(np.float64) / dt64[:, None] * (host(tt).astype(np.float64) - host(ts[t0]))[:, None]
    assert (np.abs(host(w) - w64) <= 6 * 2.0 ** -24 * np.abs(w64) + 2.0 ** -149).all()
    E = SE3.exp(w).data
    held("exp", E, R.exp(host(w)))
    G = (SE3(E) * SE3(P0)).data
    held("mul 2", G, R.mul(host(E), host(P0)))
    assert torch.equal(got, G)
    # at a keyframe's timestamp exactly the keyframe's pose
    for k in (0, 3, 7, 11):
        assert torch.equal(got[times.index(float(k))], P[k]), k
    # behind the last keyframe t0 = t1: the step is log(P P^-1), zero up to the rounding of that product, over dt = 1e-3
    assert (got[6] - P[11]).abs().max() <= 1500 * 7 * 2.0 ** -24
    # 2^-10 before keyframe 4 the share of the step from keyframe 3 still to go is 1 - (1 - 2^-10) / 1.001 = 1.97e-3 (the 1e-3 in dt),
    # up to the curvature of the path (a rotation of 0.01 rad between the two: a relative 1e-2)
    near = filler.interpolate([4.0 - 2.0 ** -10])[0]
    share = float((near[:3] - P[4, :3]).norm() / (P[4, :3] - P[3, :3]).norm())
    print(f"filler: share of the step left 2^-10 before the keyframe {share:.3e}")
    assert 1.5e-3 < share < 2.5e-3


def test_filler_fills_a_stream_and_restores_the_video():
    from splat_slam_amd.droid_net import DroidNet
    from splat_slam_amd.trajectory_filler import PoseTrajectoryFiller
    net = DroidNet.synthetic(7, device=DEV)
    v, fresh = make_video(buffer=32), make_video(buffer=32)
    filler = PoseTrajectoryFiller(net, v, device=DEV)
    poses = filler(SyntheticStream(19, step=0.5))
    assert tuple(poses.shape) == (19, 7) and poses.dtype == torch.float32 and torch.isfinite(poses).all()
    assert (poses[:, 3:].norm(dim=1) - 1).abs().max() < 1e-3
    assert v.counter.value == 12 and filler.count == 19
    assert torch.equal(v.poses[:12], fresh.poses[:12]) and torch.equal(v.disps[:12], fresh.disps[:12])
    start = filler.interpolate([0.5 * i for i in range(19)])
    assert not torch.equal(poses, start)                                        # the twelve updates moved them
    with pytest.raises(ValueError, match="exceed the video buffer"):
        PoseTrajectoryFiller(net, make_video(buffer=16), device=DEV)(SyntheticStream(3))


# ---- 10. the tracker
def run_tracker(only_tracking):
    from splat_slam_amd.depth_video import DepthVideo
    from splat_slam_amd.droid_net import DroidNet
    from splat_slam_amd.tracker import Tracker
    cfg = make_cfg(**{"tracking.warmup": 4, "tracking.motion_filter.thresh": 0.0, "tracking.frontend.keyframe_thresh": -1.0,
                      "tracking.frontend.enable_online_ba": True, "tracking.backend.ba_freq": 3, "mapping.every_keyframe": 1})
    video = DepthVideo(48, 64, buffer=16, device=DEV)
    calls, bas = [], []
    tracker = Tracker(cfg, DroidNet.synthetic(7, device=DEV), video, on_keyframe=lambda i, t: calls.append((i, t, tracker.frontend.is_initialized)),
                      only_tracking=only_tracking)
    dense = tracker.online_ba.dense_ba
    tracker.online_ba.dense_ba = lambda steps: (bas.append((steps, video.counter.value)), dense(steps))[1]
    tracker.run(SyntheticStream(10))
    return tracker, video, calls, bas


def test_tracker_reports_keyframes_after_initialisation():
    tracker, video, calls, bas = run_tracker(False)
    assert tracker.frontend.is_initialized and video.counter.value == 10 and tracker.frontend.t1 == 10
    assert calls[-1][:2] == (None, None) and all(c[2] for c in calls)
    idx = [c[0] for c in calls[:-1]]
    assert idx == list(range(3, 10)) and [c[1] for c in calls[:-1]] == [float(i) for i in idx]
    assert bas == [(2, 4), (2, 7), (2, 10)]                                     # keyframe indices 3, 6 and 9
    assert torch.isfinite(video.poses).all() and torch.isfinite(video.disps).all()


def test_tracker_with_only_tracking_calls_nothing():
    tracker, video, calls, bas = run_tracker(True)
    assert calls == [] and video.counter.value == 10 and len(bas) == 3
