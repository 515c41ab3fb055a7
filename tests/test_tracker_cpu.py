"""The order in which Frontend, Backend, PoseTrajectoryFiller and Tracker call the factor graph and the video, without a GPU: a fake
video and a FactorGraph that records every call stand in for the real ones, and the recorded traces are compared with the sequence of
the reference's frontend.py, backend.py and tracker.py written out by hand.  The same classes run on the real graph in
tests/test_gpu_tracker.py."""
import contextlib
import types

import pytest
import torch

from tracker_cases import make_cfg

LOG = []


class FakeVideo:
    def __init__(self, counter, distance=10.0, buffer=32):
        self.counter = types.SimpleNamespace(value=counter)
        self.d, self.down_scale = distance, 8
        self.poses = torch.arange(buffer * 7, dtype=torch.float32).reshape(buffer, 7)
        self.disps = torch.arange(buffer * 4, dtype=torch.float32).reshape(buffer, 2, 2) + 1.0
        self.timestamp = torch.arange(buffer, dtype=torch.float32)

    def get_lock(self):
        return contextlib.nullcontext()

    def distance(self, ii, jj, beta=0.3, bidirectional=True):
        LOG.append(("distance", list(ii), list(jj), beta, bidirectional))
        return torch.tensor([self.d])

    def set_dirty(self, a, b):
        LOG.append(("set_dirty", int(a), int(b)))

    def update_valid_depth_mask(self):
        LOG.append(("update_valid_depth_mask",))

    def normalize(self):
        LOG.append(("normalize",))


class FakeGraph:
    """records (name of the graph, method, arguments); edge lists as the tests set them"""
    edge_num = 0                                    # what add_backend_proximity_factors reports

    def __init__(self, video, update_op, device="cuda", corr_impl="volume", max_factors=-1):
        self.name = "front" if corr_impl == "volume" else "back"
        self.video, self.corr_impl, self.max_factors = video, corr_impl, max_factors
        LOG.append((self.name, "FactorGraph", update_op, device, corr_impl, max_factors))
        self.ii = torch.zeros(0, dtype=torch.long)
        self.jj, self.age = self.ii.clone(), self.ii.clone()
        self.corr = self.net = None
        self.target = self.weight = torch.zeros(1, 0, 2, 2, 2)

    def _set_edges(self, ii, ages):
        self.ii = torch.tensor(ii)
        self.jj = self.ii + 1
        self.age = torch.tensor(ages)
        self.corr, self.net = object(), torch.zeros(1, len(ii), 1, 2, 2)
        self.target = self.weight = torch.zeros(1, len(ii), 2, 2, 2)

    def add_neighborhood_factors(self, t0, t1, r=3):
        LOG.append((self.name, "add_neighborhood_factors", t0, t1, r))
        self._set_edges(list(range(t0, t1 - 1)), [0] * (t1 - 1 - t0))

    def add_proximity_factors(self, t0=0, t1=0, rad=2, nms=2, beta=0.25, thresh=16.0, remove=False):
        LOG.append((self.name, "add_proximity_factors", t0, t1, rad, nms, beta, thresh, remove))

    def add_backend_proximity_factors(self, t_start, t_end, nms, radius, thresh, max_factors, beta, t_start_loop=None, loop=False):
        LOG.append((self.name, "add_backend_proximity_factors", t_start, t_end, nms, radius, thresh, max_factors, beta, t_start_loop, loop))
        return FakeGraph.edge_num

    def update(self, t0=None, t1=None, itrs=2, use_inactive=False, EP=1e-7, motion_only=False, opt_type="pose_depth"):
        LOG.append((self.name, "update", t0, t1, itrs, use_inactive, motion_only, opt_type))
        self.age = self.age + 1

    def update_lowmem(self, t0=None, t1=None, itrs=2, use_inactive=False, EP=1e-7, steps=8, enable_wq=True):
        LOG.append((self.name, "update_lowmem", t0, t1, itrs, use_inactive, steps, enable_wq))

    def rm_factors(self, mask, store=False):
        LOG.append((self.name, "rm_factors", mask.tolist(), store))
        keep = ~mask
        self.ii, self.jj, self.age = self.ii[keep], self.jj[keep], self.age[keep]

    def rm_keyframe(self, ix):
        LOG.append((self.name, "rm_keyframe", ix))

    def clear_edges(self):
        LOG.append((self.name, "clear_edges"))
        self.ii = None


UPDATE_OP = "the update operator"
NET = types.SimpleNamespace(update=UPDATE_OP)


@pytest.fixture
def fake(monkeypatch):
    from splat_slam_amd import backend, frontend
    monkeypatch.setattr(backend, "FactorGraph", FakeGraph)
    monkeypatch.setattr(frontend, "FactorGraph", FakeGraph)
    monkeypatch.setattr(FakeGraph, "edge_num", 0)
    LOG.clear()
    return LOG


def upd(t0, opt, t1=None):
    return ("front", "update", t0, t1, 2, True, False, opt)


ALTERNATING8 = [upd(None, "pose_depth" if i % 2 == 0 else "depth_scale") for i in range(8)]
ALTERNATING4 = ALTERNATING8[:4]


# ---- Frontend
def test_frontend_initialisation_trace(fake):
    from splat_slam_amd.frontend import Frontend
    cfg = make_cfg(device="cpu")
    video = FakeVideo(7)
    fr = Frontend(NET, video, cfg)
    assert fake == [("front", "FactorGraph", UPDATE_OP, "cpu", "volume", 75)]
    assert (fr.t1, fr.is_initialized, fr.max_age, fr.iters1, fr.iters2, fr.warmup, fr.beta) == (0, False, 50, 8, 4, 8, 0.75)
    assert (fr.frontend_nms, fr.keyframe_thresh, fr.frontend_window, fr.frontend_thresh, fr.frontend_radius, fr.frontend_max_factors,
            fr.enable_loop) == (1, 4.0, 25, 16.0, 2, 75, False)
    assert fr.update_op is UPDATE_OP and fr.video is video and fr.loop_closing.video is video and fr.graph.name == "front"
    fake.clear()
    fr()                                                                        # counter 7 != warmup 8
    assert fake == [] and not fr.is_initialized
    video.counter.value = 8
    pose7, disp47 = video.poses[7].clone(), video.disps[4:8].mean()
    fr()
    assert fake == ([("front", "add_neighborhood_factors", 0, 8, 3)] + [upd(1, "pose_depth")] * 8 +
                    [("front", "add_proximity_factors", 0, 0, 2, 2, 0.25, 16.0, False)] + [upd(1, "pose_depth")] * 8 +
                    [("set_dirty", 0, 8), ("front", "rm_factors", [True] * 4 + [False] * 3, True), ("update_valid_depth_mask",)])
    assert fr.is_initialized and fr.t1 == 8
    assert torch.equal(video.poses[8], pose7) and torch.equal(video.disps[8], disp47.expand(2, 2))
    assert torch.equal(fr.last_pose, pose7) and float(fr.last_time) == 7.0 and torch.equal(fr.last_disp, video.disps[7])
    fake.clear()
    fr()                                                                        # initialised, t1 == counter: nothing
    assert fake == []


def initialised(cfg, distance):
    from splat_slam_amd.frontend import Frontend
    video = FakeVideo(8, distance)
    fr = Frontend(NET, video, cfg)
    fr()
    assert fr.is_initialized and fr.graph.ii.tolist() == [4, 5, 6] and fr.graph.age.tolist() == [16, 16, 16]
    video.counter.value = 9
    LOG.clear()
    return fr, video


def head(window=25, old=(False, False, False)):
    return [("front", "rm_factors", list(old), True), ("front", "add_proximity_factors", 4, max(9 - window, 0), 2, 1, 0.75, 16.0, True)] + \
        ALTERNATING8 + [("distance", [7], [8], 0.75, True)]


def test_frontend_keeps_a_distant_keyframe(fake):
    fr, video = initialised(make_cfg(device="cpu"), distance=4.0)               # not below keyframe_thresh 4.0
    pose8, disp8 = video.poses[8].clone(), video.disps[8].mean()
    fr()
    assert fake == head() + ALTERNATING4 + [("set_dirty", 4, 9), ("update_valid_depth_mask",)]
    assert fr.t1 == 9 and video.counter.value == 9
    assert torch.equal(video.poses[9], pose8) and torch.equal(video.disps[9], disp8.expand(2, 2))


def test_frontend_drops_a_close_keyframe(fake):
    fr, video = initialised(make_cfg(device="cpu"), distance=3.9)
    pose7, disp7 = video.poses[7].clone(), video.disps[7].mean()
    fr()
    assert fake == head() + [("front", "rm_keyframe", 8), ("set_dirty", 4, 8), ("update_valid_depth_mask",)]
    assert fr.t1 == 8 and video.counter.value == 8
    assert torch.equal(video.poses[8], pose7) and torch.equal(video.disps[8], disp7.expand(2, 2))


def test_frontend_ages_out_old_edges(fake):
    fr, video = initialised(make_cfg(device="cpu", **{"tracking.max_age": 15}), distance=10.0)
    fr.graph.age = torch.tensor([16, 3, 16])
    fr()
    assert fake[0] == ("front", "rm_factors", [True, False, True], True) and fr.graph.ii.tolist() == [5]
    assert fake[-2] == ("set_dirty", 5, 9)


@pytest.mark.parametrize("edges", [0, 31])
def test_frontend_loop_closure_trace(fake, edges):
    cfg = make_cfg(device="cpu", **{"tracking.frontend.enable_loop": True, "tracking.frontend.window": 8,
                                    "tracking.backend.loop_window": 6})
    fr, video = initialised(cfg, distance=10.0)                                 # counter 9 > window 8
    FakeGraph.edge_num = edges
    fr()
    back = [("back", "FactorGraph", UPDATE_OP, "cpu", "alt_fused", 48),
            ("back", "add_backend_proximity_factors", 0, 9, 12, 1, 25.0, 48 - 3, 0.75, 3, True)]
    back += [("back", "update_lowmem", 4, 9, 2, False, 4, True)] if edges else []
    back += [("back", "clear_edges")]
    tail = [("set_dirty", 4, 9), ("update_valid_depth_mask",)]
    assert fake == head(window=8) + back + ([] if edges else ALTERNATING4) + tail
    assert fr.last_loop_t == 9 and fr.graph.ii.tolist() == [4, 5, 6]           # the local graph keeps its edges: the copy was released
    # below the window no loop closure is tried
    video.counter.value = 10
    fr.frontend_window = 25
    fake.clear()
    fr()
    assert not [c for c in fake if c[0] == "back"] and fake[-6:-2] == ALTERNATING4


# ---- Backend
def test_backend_ba_traces_and_max_factors(fake):
    from splat_slam_amd.backend import Backend
    cfg = make_cfg(device="cpu")
    video = FakeVideo(12)
    be = Backend(NET, video, cfg)
    assert (be.beta, be.backend_thresh, be.backend_radius, be.backend_nms, be.backend_normalize) == (0.75, 22.0, 2, 3, True)
    assert (be.backend_loop_window, be.backend_loop_thresh, be.backend_loop_radius, be.backend_loop_nms) == (25, 25.0, 1, 12)
    assert be.update_op is UPDATE_OP and be.device == "cpu" and (be.t0, be.t1) == (0, 0) and fake == []
    mf = ((2 + 2) * 2) * 12
    for edges in (0, 40):
        FakeGraph.edge_num = edges
        fake.clear()
        assert be.dense_ba(steps=3, enable_wq=False) == (12, edges)
        want = [("normalize",), ("back", "FactorGraph", UPDATE_OP, "cpu", "alt_fused", mf),
                ("back", "add_backend_proximity_factors", 0, 12, 3, 2, 22.0, mf, 0.75, 0, False)]
        want += [("back", "update_lowmem", 1, 12, 2, False, 3, False)] if edges else []
        assert fake == want + [("back", "clear_edges"), ("set_dirty", 0, 12), ("update_valid_depth_mask",)]
    # defaults, no normalisation, the reference's lookup
    cfg["tracking"]["backend"]["normalize"] = False
    be = Backend(NET, video, cfg, corr_impl="alt")
    fake.clear()
    be.dense_ba()
    assert fake[0] == ("back", "FactorGraph", UPDATE_OP, "cpu", "alt", mf) and fake[2] == ("back", "update_lowmem", 1, 12, 2, False, 6, True)
    # loop_ba: the window's first frame is fixed, max_factors 8 * window less the edges taken over from the local graph
    local = FakeGraph(video, UPDATE_OP)
    local._set_edges([3, 4, 5, 6, 7], [1, 2, 3, 4, 5])
    for lg, left in ((None, 200), (local, 195)):
        fake.clear()
        assert be.loop_ba(2, 40, steps=5, local_graph=lg, enable_wq=False) == (25, 40)
        assert fake == [("back", "FactorGraph", UPDATE_OP, "cpu", "alt", 200),
                        ("back", "add_backend_proximity_factors", 2, 40, 12, 1, 25.0, left, 0.75, 15, True),
                        ("back", "update_lowmem", 16, 40, 2, False, 5, False), ("back", "clear_edges")]
    assert be.loop_ba(0, 10) == (10, 40) and fake[-3][1:5] == ("add_backend_proximity_factors", 0, 10, 12) and fake[-3][9] == 0
    with pytest.raises(ValueError, match="must not precede"):
        be.ba(5, 10, 2, FakeGraph(video, UPDATE_OP, corr_impl="alt"), 1, 1, 1.0, 10, t_start_loop=3, loop=True)


def test_loop_ba_copies_the_local_graph_with_clone(fake):
    from splat_slam_amd.backend import Backend
    video = FakeVideo(12)
    be = Backend(NET, video, make_cfg(device="cpu"))
    local = FakeGraph(video, UPDATE_OP)
    local._set_edges([3, 4], [7, 9])
    made, plain = [], be._graph
    be._graph = lambda mf: (made.append(plain(mf)), made[-1])[1]
    seen = {}
    made_ba = be.ba
    be.ba = lambda t_start, t_end, steps, graph, *a, **k: (seen.update({n: getattr(graph, n) for n in ("ii", "jj", "age", "net", "target",
                                                                                                     "weight")}),
                                                           made_ba(t_start, t_end, steps, graph, *a, **k))[1]
    be.loop_ba(0, 12, local_graph=local)
    for name, t in seen.items():
        src = getattr(local, name)
        assert torch.equal(t, src) and t.data_ptr() != src.data_ptr(), name
    assert made[0].corr is None and local.ii.tolist() == [3, 4]


# ---- Tracker
def test_tracker_schedules_online_ba_and_keyframe_reports(monkeypatch):
    from splat_slam_amd import tracker as T
    log = []
    accept = [1, 1, 1, 1, 0, 1, 1, 1]
    drop = {6}

    class Filter:
        def __init__(self, net, video, thresh=2.5, device="cuda"):
            self.video, self.i = video, 0
            log.append(("MotionFilter", thresh, device))

        def track(self, tstamp, image, intrinsics=None):
            assert not torch.is_grad_enabled() and intrinsics == "K"
            log.append(("track", tstamp, image))
            self.video.counter.value += accept[self.i]
            self.i += 1

    class Front:
        def __init__(self, net, video, cfg):
            self.video, self.is_initialized, self.i = video, False, 0

        def __call__(self):
            assert not torch.is_grad_enabled()
            log.append(("frontend",))
            if self.video.counter.value == 3:
                self.is_initialized = True
            if self.i in drop:
                self.video.counter.value -= 1
            self.i += 1

    class Back:
        def __init__(self, net, video, cfg):
            pass

        def dense_ba(self, steps=6, enable_wq=True):
            log.append(("dense_ba", steps))

    monkeypatch.setattr(T, "MotionFilter", Filter)
    monkeypatch.setattr(T, "Frontend", Front)
    monkeypatch.setattr(T, "Backend", Back)
    cfg = make_cfg(device="cpu", **{"tracking.frontend.enable_online_ba": True, "tracking.backend.ba_freq": 2, "mapping.every_keyframe": 2,
                                    "tracking.motion_filter.thresh": 3.5})

    class Stream:
        def __len__(self):
            return len(accept)

        def __getitem__(self, i):
            return 10.0 * i, f"image {i}", None, None

        def get_intrinsic(self):
            return "K"

    def run(**kw):
        log.clear()
        video = FakeVideo(0)
        T.Tracker(cfg, NET, video, **kw).run(Stream())
        assert log[0] == ("MotionFilter", 3.5, "cpu")
        frames = [c for c in log if c[0] in ("track", "frontend")]
        assert frames == [c for i in range(8) for c in (("track", 10.0 * i, f"image {i}"), ("frontend",))]
        return [(log[:k].count(("frontend",)) - 1, c) for k, c in enumerate(log) if c[0] in ("dense_ba", "kf")]

    kf = lambda i, t: log.append(("kf", i, t))
    # keyframe index after each frame: 0 1 2 3 3 4 4 5 (frame 4 is no keyframe, frame 6's is dropped); initialised from frame 2 on
    assert run(on_keyframe=kf) == [(2, ("dense_ba", 2)), (3, ("kf", 3, 30.0)), (5, ("dense_ba", 2)), (7, ("kf", 5, 70.0)),
                                   (7, ("kf", None, None))]
    assert run(on_keyframe=kf, only_tracking=True) == [(2, ("dense_ba", 2)), (5, ("dense_ba", 2))]
    assert run() == [(2, ("dense_ba", 2)), (5, ("dense_ba", 2))]
    cfg["tracking"]["frontend"]["enable_online_ba"] = False
    cfg["mapping"]["every_keyframe"] = 1
    assert run(on_keyframe=kf) == [(2, ("kf", 2, 20.0)), (3, ("kf", 3, 30.0)), (5, ("kf", 4, 50.0)), (7, ("kf", 5, 70.0)),
                                   (7, ("kf", None, None))]


# ---- the filler's brackets
def test_filler_brackets():
    from splat_slam_amd.trajectory_filler import BLOCK, PoseTrajectoryFiller, bracket
    ts = torch.tensor([2.0, 5.0, 5.5, 9.0])
    tt = torch.tensor([1.0, 2.0, 3.0, 5.0, 5.25, 5.5, 8.999, 9.0, 100.0])
    t0, t1 = bracket(ts, tt)
    assert t0.tolist() == [-1, 0, 0, 1, 1, 2, 2, 3, 3] and t1.tolist() == [0, 1, 1, 2, 2, 3, 3, 3, 3]
    assert t0.dtype == torch.int64 and t1.dtype == torch.int64
    one = bracket(ts[:1], tt)
    assert one[0].tolist() == [-1] + [0] * 8 and one[1].tolist() == [0] * 9     # a single keyframe: t1 = t0 wherever t0 = N - 1 = 0
    video = FakeVideo(4)
    video.timestamp[:4] = ts
    filler = PoseTrajectoryFiller(types.SimpleNamespace(fnet=None, update=None), video, device="cpu")
    _, k0, k1 = filler._bracket(tt)
    assert k0.tolist() == [3, 0, 0, 1, 1, 2, 2, 3, 3] and k1.tolist() == t1.tolist()           # -1 wraps to the last keyframe
    assert BLOCK == 16
    video.counter.value = 17                                                    # 17 + 16 > 32
    with pytest.raises(ValueError, match="exceed the video buffer of 32"):
        filler(None)
    video.counter.value = 0
    with pytest.raises(ValueError, match="no keyframe"):
        filler.interpolate([1.0])


def test_module_docstrings_state_the_call_order_and_the_differences():
    from splat_slam_amd import backend, corr, frontend, tracker, trajectory_filler
    import droid_backends
    for mod, words in ((backend, ("Backend(net, video, cfg, corr_impl=\"alt_fused\")", "dense_ba", "loop_ba", "clone()", "8 * loop_window",
                                  "((radius + 2) * 2) * frames", "DESIGN.md section 3")),
                       (frontend, ("Frontend(net, video, cfg)", "iters1 = 8", "iters2 = 4", "keyframe_thresh", "rm_keyframe", "loop_ba",
                                   "update_valid_depth_mask", "DESIGN.md section 3")),
                       (trajectory_filler, ("PoseTrajectoryFiller(net, video, device=\"cuda\")", "#{ts <= t} - 1", "1e-3", "16 at a time",
                                            "motion_only=True", "ValueError", "DESIGN.md section 3")),
                       (tracker, ("Tracker(cfg, net, video, on_keyframe=None, only_tracking=False)", "dense_ba(2)", "every_keyframe",
                                  "on_keyframe(None, None)", "DESIGN.md section 3")),
                       (corr, ("FusedAltCorrBlock(fmaps [1,N,C,H,W], num_levels=4, radius=3)", "altcorr_pyramid_forward")),
                       (droid_backends, ("altcorr_pyramid_forward(levels, src [E], dst [E], coords [E,H,W,2], radius)",))):
        for w in words:
            assert w in mod.__doc__, (mod.__name__, w)
    assert "altcorr_pyramid_forward" in droid_backends.__all__ and "FusedAltCorrBlock" in corr.__all__
