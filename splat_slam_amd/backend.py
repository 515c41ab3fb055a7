"""The tracker's global optimisation (Backend of the reference's thirdparty/glorie_slam/backend.py): bundle adjustment over every
keyframe, and loop closure over the frontend's graph plus the loop edges of the last `loop_window` keyframes, both through
FactorGraph.update_lowmem.  Stated in DESIGN.md section 3, "Tracker".

    Backend(net, video, cfg, corr_impl="alt_fused")
        net: a DroidNet (only net.update is used); video: a DepthVideo; cfg: the reference's dict, read at cfg["device"],
        cfg["tracking"]["beta"] and cfg["tracking"]["backend"][thresh, radius, nms, normalize, loop_window, loop_thresh, loop_radius,
        loop_nms]; corr_impl: "alt_fused" (one lookup launch per chunk) or "alt" (the reference's four launches per chunk)
    ba(t_start, t_end, steps, graph, nms, radius, thresh, max_factors, t_start_loop=None, loop=False, motion_only=False, enable_wq=True)
        -> number of edges; adds the backend's edges to `graph`, runs `steps` low-memory updates with the first frame t_start_loop fixed
        and releases the graph (clear_edges).  No edge added: 0, and the video is not touched.
    dense_ba(steps=6, enable_wq=True) -> (frames, edges): all frames [0, counter), max_factors = ((radius + 2) * 2) * frames; normalises
        the video first when configured; afterwards every frame is dirty and the valid-depth mask is recomputed.
    loop_ba(t_start, t_end, steps=6, motion_only=False, local_graph=None, enable_wq=True) -> (t_end - t_start_loop, edges):
        t_start_loop = max(0, t_end - loop_window), max_factors = 8 * loop_window less the edges taken over; ii, jj, age, net, target
        and weight of local_graph are cloned into the new graph.

Kept from the reference: `motion_only` is accepted and not used (update_lowmem always optimises poses and depths).  Differences, both
deliberate: tensors are copied with clone() instead of deepcopy, and the allocator's cache is not emptied after a pass.
"""
import torch

from splat_slam_amd.factor_graph import FactorGraph

__all__ = ["Backend"]

COPIED = ("ii", "jj", "age", "net", "target", "weight")


class Backend:
    def __init__(self, net, video, cfg, corr_impl="alt_fused"):
        if corr_impl not in ("alt", "alt_fused"):
            raise ValueError(f"Backend: corr_impl must be 'alt' or 'alt_fused', got {corr_impl!r}")
        self.video, self.update_op, self.device, self.corr_impl = video, net.update, cfg["device"], corr_impl
        self.t0 = self.t1 = 0
        tr, be = cfg["tracking"], cfg["tracking"]["backend"]
        self.beta = tr["beta"]
        self.backend_thresh, self.backend_radius, self.backend_nms = be["thresh"], be["radius"], be["nms"]
        self.backend_normalize = be["normalize"]
        self.backend_loop_window, self.backend_loop_thresh = be["loop_window"], be["loop_thresh"]
        self.backend_loop_radius, self.backend_loop_nms = be["loop_radius"], be["loop_nms"]

    def _graph(self, max_factors):
        return FactorGraph(self.video, self.update_op, device=self.device, corr_impl=self.corr_impl, max_factors=max_factors)

    @torch.no_grad()
    def ba(self, t_start, t_end, steps, graph, nms, radius, thresh, max_factors, t_start_loop=None, loop=False, motion_only=False,
           enable_wq=True):
        if t_start_loop is None or not loop:
            t_start_loop = t_start
        if t_start_loop < t_start:
            raise ValueError(f"Backend.ba: t_start_loop ({t_start_loop}) must not precede t_start ({t_start})")
        edge_num = graph.add_backend_proximity_factors(t_start, t_end, nms, radius, thresh, max_factors, self.beta, t_start_loop, loop)
        if edge_num == 0:
            graph.clear_edges()
            return 0
        # the first frame of the loop window stays fixed, against drift: t_start_loop, not t_start
        graph.update_lowmem(t0=t_start_loop + 1, t1=t_end, itrs=2, use_inactive=False, steps=steps, enable_wq=enable_wq)
        graph.clear_edges()
        return edge_num

    @torch.no_grad()
    def dense_ba(self, steps=6, enable_wq=True):
        t_start, t_end = 0, self.video.counter.value
        n = t_end - t_start
        max_factors = ((self.backend_radius + 2) * 2) * n
        if self.backend_normalize:
            self.video.normalize()
        n_edges = self.ba(t_start, t_end, steps, self._graph(max_factors), self.backend_nms, self.backend_radius, self.backend_thresh,
                          max_factors, motion_only=False, enable_wq=enable_wq)
        self.video.set_dirty(t_start, t_end)
        self.video.update_valid_depth_mask()
        return n, n_edges

    @torch.no_grad()
    def loop_ba(self, t_start, t_end, steps=6, motion_only=False, local_graph=None, enable_wq=True):
        window = self.backend_loop_window
        max_factors = 8 * window
        t_start_loop = max(0, t_end - window)
        graph = self._graph(max_factors)
        if local_graph is not None:
            for key in COPIED:
                val = getattr(local_graph, key)
                if val is not None:
                    setattr(graph, key, val.clone())
        left_factors = max_factors - len(graph.ii)
        n_edges = self.ba(t_start, t_end, steps, graph, self.backend_loop_nms, self.backend_loop_radius, self.backend_loop_thresh,
                          left_factors, t_start_loop=t_start_loop, loop=True, motion_only=motion_only, enable_wq=enable_wq)
        return t_end - t_start_loop, n_edges
