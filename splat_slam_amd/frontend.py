"""The tracker's local optimisation (Frontend of the reference's thirdparty/glorie_slam/frontend.py): called once per frame after the
motion filter, it bootstraps the map from the first `warmup` keyframes and afterwards optimises a sliding window of keyframes with
FactorGraph.update, dropping the newest keyframe again when it is too close to the one before.  Stated in DESIGN.md section 3, "Tracker".

    Frontend(net, video, cfg)
        net: a DroidNet (net.update); video: a DepthVideo; cfg: the reference's dict, read at cfg["device"], cfg["tracking"][max_age,
        warmup, beta] and cfg["tracking"]["frontend"][nms, keyframe_thresh, window, thresh, radius, max_factors, enable_loop]
        (and what Backend reads).  One more keyword, corr_impl="volume": the graph's correlation operator, "volume" (a CorrBlock
        per batch of edges) or "volume_fused" (one FusedCorrBlock over video.fmaps).  Attributes as in the reference: video, update_op, t1, is_initialized, max_age, iters1 = 8,
        iters2 = 4, warmup, beta, frontend_*, enable_loop, loop_closing (a Backend), graph, and after the
        initialisation last_pose, last_disp, last_time.
    frontend()
        counter == warmup and not initialised: neighbourhood edges (r = 3), 8 updates, proximity edges (rad 2, nms 2, remove=False),
            8 updates, frame t1 seeded with the pose of t1 - 1 and the mean disparity of the last four, the edges with ii < warmup - 4
            stored as inactive.
        initialised and t1 < counter: edges older than max_age stored as inactive, proximity edges over (t1 - 5, max(t1 - window, 0)),
            iters1 updates alternating "pose_depth" / "depth_scale", then the bidirectional distance of frames t1 - 2 and t1 - 1: below
            keyframe_thresh the keyframe is removed (rm_keyframe, counter and t1 go down by one); otherwise iters2 more updates, or,
            with enable_loop and counter > window, Backend.loop_ba on a copy of the graph and the iters2 updates only when it added no
            edge.  Frame t1 is seeded from t1 - 1, and the frames from the oldest active edge on are marked dirty.
        Both branches end with video.update_valid_depth_mask(); any other call does nothing.

Kept from the reference: the initialisation's proximity edges use FactorGraph's default beta (0.25), not cfg's.  Difference, deliberate:
the allocator's cache is not emptied after a step.
"""
import torch

from splat_slam_amd.backend import Backend
from splat_slam_amd.factor_graph import FactorGraph

__all__ = ["Frontend"]


class Frontend:
    def __init__(self, net, video, cfg, corr_impl="volume"):
        if corr_impl not in ("volume", "volume_fused"):
            raise ValueError(f"Frontend: corr_impl must be 'volume' or 'volume_fused', got {corr_impl!r}")
        self.video, self.update_op = video, net.update
        self.t1 = 0                                     # end of the local optimisation window
        self.is_initialized = False
        tr, fe = cfg["tracking"], cfg["tracking"]["frontend"]
        self.max_age = tr["max_age"]
        self.iters1, self.iters2 = 4 * 2, 2 * 2
        self.warmup, self.beta = tr["warmup"], tr["beta"]
        self.frontend_nms, self.keyframe_thresh, self.frontend_window = fe["nms"], fe["keyframe_thresh"], fe["window"]
        self.frontend_thresh, self.frontend_radius, self.frontend_max_factors = fe["thresh"], fe["radius"], fe["max_factors"]
        self.enable_loop = fe["enable_loop"]
        self.loop_closing = Backend(net, video, cfg)
        self.graph = FactorGraph(video, net.update, device=cfg["device"], corr_impl=corr_impl, max_factors=self.frontend_max_factors)

    def _refine(self):
        for itr in range(self.iters2):
            self.graph.update(t0=None, t1=None, use_inactive=True, opt_type="pose_depth" if itr % 2 == 0 else "depth_scale")

    def _update(self):
        """add edges, perform update"""
        self.t1 += 1
        if self.graph.corr is not None:
            self.graph.rm_factors(self.graph.age > self.max_age, store=True)
        self.graph.add_proximity_factors(self.t1 - 5, max(self.t1 - self.frontend_window, 0), rad=self.frontend_radius,
                                         nms=self.frontend_nms, thresh=self.frontend_thresh, beta=self.beta, remove=True)
        for itr in range(self.iters1):
            self.graph.update(None, None, use_inactive=True, opt_type="pose_depth" if itr % 2 == 0 else "depth_scale")
        d = self.video.distance([self.t1 - 2], [self.t1 - 1], beta=self.beta, bidirectional=True)
        if d.item() < self.keyframe_thresh:
            self.graph.rm_keyframe(self.t1 - 1)
            with self.video.get_lock():
                self.video.counter.value -= 1
                self.t1 -= 1
        else:
            cur_t = self.video.counter.value
            if self.enable_loop and cur_t > self.frontend_window:
                _, n_edge = self.loop_closing.loop_ba(t_start=0, t_end=cur_t, steps=self.iters2, motion_only=False,
                                                      local_graph=self.graph, enable_wq=True)
                if n_edge == 0:
                    self._refine()
                self.last_loop_t = cur_t
            else:
                self._refine()
        # the next frame starts from this one
        self.video.poses[self.t1] = self.video.poses[self.t1 - 1]
        self.video.disps[self.t1] = self.video.disps[self.t1 - 1].mean()
        self.video.set_dirty(self.graph.ii.min(), self.t1)

    def _initialize(self):
        """bootstrapping from the first `warmup` keyframes"""
        self.t1 = self.video.counter.value
        self.graph.add_neighborhood_factors(0, self.t1, r=3)
        for _ in range(8):
            self.graph.update(1, use_inactive=True, opt_type="pose_depth")
        self.graph.add_proximity_factors(0, 0, rad=2, nms=2, thresh=self.frontend_thresh, remove=False)
        for _ in range(8):
            self.graph.update(1, use_inactive=True, opt_type="pose_depth")
        self.video.poses[self.t1] = self.video.poses[self.t1 - 1].clone()
        self.video.disps[self.t1] = self.video.disps[self.t1 - 4:self.t1].mean()
        self.is_initialized = True
        self.last_pose = self.video.poses[self.t1 - 1].clone()
        self.last_disp = self.video.disps[self.t1 - 1].clone()
        self.last_time = self.video.timestamp[self.t1 - 1].clone()
        with self.video.get_lock():
            self.video.set_dirty(0, self.t1)
        self.graph.rm_factors(self.graph.ii < self.warmup - 4, store=True)

    @torch.no_grad()
    def __call__(self):
        """main update"""
        if not self.is_initialized and self.video.counter.value == self.warmup:
            self._initialize()
            self.video.update_valid_depth_mask()
        elif self.is_initialized and self.t1 < self.video.counter.value:
            self._update()
            self.video.update_valid_depth_mask()
