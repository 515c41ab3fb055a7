"""The tracker's factor graph (FactorGraph, thirdparty/glorie_slam/factor_graph.py) on the gfx950 kernels `sgr_graph_*`
(include/splat_hip.h, csrc/sgr_graph.hip): it owns the edge lists, the targets and weights and the GRU state, builds the correlation
operator, calls the update operator and writes its output into DepthVideo.ba and DepthVideo.upsample.  Stated in DESIGN.md
section 3, "Factor graph".

    reproject(poses [N,7], disps [N,h,w], intrinsics [N,4], ii [E], jj [E], target=None)
        -> coords [E,h,w,2], valid [E,h,w,1]; with target [E,h,w,2] also motn [E,4,h,w] = clamp((coords - grid, target - coords), +-64).
        Intrinsics are per frame.  ii == jj is the fixed stereo baseline.  An edge with an index outside [0, N) gives zeros.
    select_proximity_edges(d, t0, t1, t, ii_old, jj_old, rad, nms, thresh, max_factors) -> (ii, jj)
        the frontend's greedy selection over d [(t-t0)*(t-t1)] (row i - t0, column j - t1); ii_old, jj_old are the existing edges.
    select_backend_edges(d, t_start, t_end, t_start_loop, loop, nms, radius, thresh, max_factors) -> (ii, jj, num_loop)
        the backend's, over d [(t_end-t_start_loop)*(t_end-t_start)].
    FactorGraph(video, update_op, device="cuda", corr_impl="volume", max_factors=-1): the reference's class, see its docstring.

Both selections visit the entries in ascending distance and equal distances in ascending flat index (the reference leaves ties to
argsort), treat NaN as inf, and ignore what rules 2 and 3 would touch outside the matrix (the reference's flat index would wrap for
j < t1; no call of its frontend has such a j).  A selection costs one host read, of the two counters; everything before it is
stream-ordered.  The matrix is at most 512 x 512 (the DepthVideo buffer limit).  Every tensor lives on the GPU; there is no CPU path.
"""
import torch

from splat_slam_amd import _native as nat
from splat_slam_amd.corr import AltCorrBlock, CorrBlock, FusedAltCorrBlock, FusedCorrBlock

__all__ = ["reproject", "select_proximity_edges", "select_backend_edges", "FactorGraph"]

_I32 = 2 ** 31 - 1


def _gpu(name, t, dtype, ndim=None):
    """dtype, rank and layout of one argument; the device is checked by _same_device once every shape is known to be right."""
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"factor_graph: {name} must be a torch.Tensor")
    if t.dtype != dtype:
        raise TypeError(f"factor_graph: {name} must be {dtype}, got {t.dtype}")
    if ndim is not None and t.dim() != ndim:
        raise ValueError(f"factor_graph: {name} must have {ndim} dimensions, got shape {tuple(t.shape)}")
    if not t.is_contiguous():
        raise ValueError(f"factor_graph: {name} must be contiguous")
    return t


def _same_device(*ts):
    dev = ts[0].device
    for t in ts:
        if not t.is_cuda:
            raise RuntimeError("factor_graph (MI355X build): every tensor must be a GPU tensor; there is no CPU path")
    for t in ts[1:]:
        if t.device != dev:
            raise RuntimeError(f"factor_graph: every tensor must be on {dev}, found one on {t.device}")
    return dev


def _stream(dev):
    return torch.cuda.current_stream(dev).cuda_stream


def reproject(poses, disps, intrinsics, ii, jj, target=None):
    _gpu("poses", poses, torch.float32, 2)
    _gpu("disps", disps, torch.float32, 3)
    _gpu("intrinsics", intrinsics, torch.float32, 2)
    _gpu("ii", ii, torch.int64, 1)
    _gpu("jj", jj, torch.int64, 1)
    if poses.shape[1] != 7:
        raise ValueError(f"factor_graph: poses must be [N,7] (t, q xyzw), got {tuple(poses.shape)}")
    n, h, w = disps.shape
    if h <= 0 or w <= 0:
        raise ValueError(f"factor_graph: disps must be [N,h,w] with h, w > 0, got {tuple(disps.shape)}")
    if tuple(intrinsics.shape) != (n, 4):
        raise ValueError(f"factor_graph: intrinsics must be one (fx, fy, cx, cy) per frame, [{n},4], got {tuple(intrinsics.shape)}")
    if ii.shape != jj.shape:
        raise ValueError(f"factor_graph: ii and jj must have the same length, got {ii.shape[0]} and {jj.shape[0]}")
    E = ii.shape[0]
    if E > nat.SGR_GRAPH_MAX_EDGES:
        raise ValueError(f"factor_graph.reproject: {E} edges in one call exceed the supported {nat.SGR_GRAPH_MAX_EDGES}")
    ts = (poses, disps, intrinsics, ii, jj)
    if target is not None:
        _gpu("target", target, torch.float32, 4)
        if tuple(target.shape) != (E, h, w, 2):
            raise ValueError(f"factor_graph.reproject: target must be [E,h,w,2] = {(E, h, w, 2)}, got {tuple(target.shape)}")
        ts += (target,)
    dev = _same_device(*ts)
    coords = torch.empty((E, h, w, 2), dtype=torch.float32, device=dev)
    valid = torch.empty((E, h, w, 1), dtype=torch.float32, device=dev)
    motn = None if target is None else torch.empty((E, 4, h, w), dtype=torch.float32, device=dev)
    if E:
        with torch.cuda.device(dev):
            nat.check(nat.lib().sgr_graph_reproject(poses.data_ptr(), poses.shape[0], disps.data_ptr(), n, h, w, intrinsics.data_ptr(),
                                                    ii.data_ptr(), jj.data_ptr(), E, nat.ptr(target), coords.data_ptr(),
                                                    valid.data_ptr(), nat.ptr(motn), _stream(dev)), "sgr_graph_reproject")
    return (coords, valid) if target is None else (coords, valid, motn)


# ---- edge selection
def _window_pairs(first, rows, rad):
    """pairs (i, j), j in [max(i - rad - 1, 0), i), over the rows i in [first, first + rows)"""
    return sum(min(rad + 1, i) for i in range(first, first + rows))


def _select_args(fn, d, rows, cols, row0, col0, rad, nms, thresh, max_factors):
    _gpu("d", d, torch.float32, 1)
    if rows < 1 or cols < 1:
        raise ValueError(f"factor_graph.{fn}: the distance matrix must have at least one row and one column, got {rows} x {cols}")
    if rows > nat.SGR_GRAPH_MAX_SIDE or cols > nat.SGR_GRAPH_MAX_SIDE:
        raise ValueError(f"factor_graph.{fn}: a {rows} x {cols} distance matrix exceeds the supported "
                         f"{nat.SGR_GRAPH_MAX_SIDE} x {nat.SGR_GRAPH_MAX_SIDE}")
    if d.shape[0] != rows * cols:
        raise ValueError(f"factor_graph.{fn}: d must have {rows} * {cols} = {rows * cols} entries, got {d.shape[0]}")
    if row0 < 0 or col0 < 0 or row0 + rows > (1 << 14):
        raise ValueError(f"factor_graph.{fn}: frame indices must lie in [0, {1 << 14}]")
    if not 0 <= rad <= (1 << 14) or not 0 <= nms <= nat.SGR_GRAPH_MAX_SIDE:
        raise ValueError(f"factor_graph.{fn}: need 0 <= rad <= {1 << 14} and 0 <= nms <= {nat.SGR_GRAPH_MAX_SIDE}, got {rad} and {nms}")
    if thresh != thresh or thresh in (float("inf"), float("-inf")):
        raise ValueError(f"factor_graph.{fn}: thresh must be finite, got {thresh}")
    return max(min(max_factors, _I32 - 16), -1)


def _select_buffers(rows, cols, cap, dev):
    lib = nat.lib()
    nbytes = lib.sgr_graph_select_scratch_bytes(rows, cols)
    es = torch.empty((max(cap, 1), 2), dtype=torch.int64, device=dev)
    counts = torch.empty((2,), dtype=torch.int32, device=dev)
    return lib, es, counts, torch.empty(nbytes, dtype=torch.uint8, device=dev), nbytes


def proximity_edges_on_device(d, t0, t1, t, ii_old, jj_old, rad, nms, thresh, max_factors):
    """The device part of select_proximity_edges: es [cap,2] int64 and counts [2] int32 (pairs, 0), with no host synchronisation."""
    t0, t1, t, rad, nms, thresh, max_factors = int(t0), int(t1), int(t), int(rad), int(nms), float(thresh), int(max_factors)
    rows, cols = t - t0, t - t1
    max_factors = _select_args("select_proximity_edges", d, rows, cols, t0, t1, rad, nms, thresh, max_factors)
    _gpu("ii_old", ii_old, torch.int64, 1)
    _gpu("jj_old", jj_old, torch.int64, 1)
    if ii_old.shape != jj_old.shape:
        raise ValueError(f"factor_graph: ii_old and jj_old must have the same length, got {ii_old.shape[0]} and {jj_old.shape[0]}")
    if ii_old.shape[0] > _I32:
        raise ValueError("factor_graph.select_proximity_edges: too many existing edges")
    dev = _same_device(d, ii_old, jj_old)
    local = 2 * _window_pairs(t0, rows, rad)
    cap = max(local, min(max_factors + 2, local + 2 * rows * cols))
    lib, es, counts, scratch, nbytes = _select_buffers(rows, cols, cap, dev)
    with torch.cuda.device(dev):
        nat.check(lib.sgr_graph_select_proximity(d.data_ptr(), t0, t1, t, ii_old.data_ptr(), jj_old.data_ptr(), ii_old.shape[0], rad, nms,
                                                 thresh, max_factors, es.data_ptr(), es.shape[0], counts.data_ptr(), scratch.data_ptr(),
                                                 nbytes, _stream(dev)), "sgr_graph_select_proximity")
    return es, counts


def backend_edges_on_device(d, t_start, t_end, t_start_loop, loop, nms, radius, thresh, max_factors):
    """The device part of select_backend_edges: es [cap,2] int64 and counts [2] int32 (pairs, loop pairs), no host synchronisation."""
    t_start, t_end, nms, radius, thresh, max_factors = int(t_start), int(t_end), int(nms), int(radius), float(thresh), int(max_factors)
    loop = bool(loop)
    t_start_loop = t_start if (t_start_loop is None or not loop) else int(t_start_loop)
    if t_start_loop < t_start:
        raise ValueError(f"factor_graph.select_backend_edges: t_start_loop ({t_start_loop}) must not precede t_start ({t_start})")
    rows, cols = t_end - t_start_loop, t_end - t_start
    max_factors = _select_args("select_backend_edges", d, rows, cols, t_start_loop, t_start, radius, nms, thresh, max_factors)
    dev = _same_device(d)
    local, per_pick = 2 * _window_pairs(t_start_loop, rows, radius), 9 if loop else 2
    cap = max(local, min(max_factors + per_pick, local + per_pick * rows * cols))
    lib, es, counts, scratch, nbytes = _select_buffers(rows, cols, cap, dev)
    with torch.cuda.device(dev):
        nat.check(lib.sgr_graph_select_backend(d.data_ptr(), t_start, t_end, t_start_loop, int(loop), nms, radius, thresh, max_factors,
                                               es.data_ptr(), es.shape[0], counts.data_ptr(), scratch.data_ptr(), nbytes, _stream(dev)),
                  "sgr_graph_select_backend")
    return es, counts


def select_proximity_edges(d, t0, t1, t, ii_old, jj_old, rad, nms, thresh, max_factors):
    es, counts = proximity_edges_on_device(d, t0, t1, t, ii_old, jj_old, rad, nms, thresh, max_factors)
    num = counts.tolist()[0]                    # the one host read
    return es[:num, 0].contiguous(), es[:num, 1].contiguous()


def select_backend_edges(d, t_start, t_end, t_start_loop, loop, nms, radius, thresh, max_factors):
    es, counts = backend_edges_on_device(d, t_start, t_end, t_start_loop, loop, nms, radius, thresh, max_factors)
    num, num_loop = counts.tolist()             # the one host read
    return es[:num, 0].contiguous(), es[:num, 1].contiguous(), num_loop


class FactorGraph:
    """The reference's graph: attributes `ii, jj, age, net, inp, corr, damping, target, weight, ii_inac, jj_inac, ii_bad, jj_bad,
    target_inac, weight_inac, coords0` with its shapes and dtypes (target, weight [1,E,h,w,2] fp32, net [1,E,128,h,w]), and methods
    `add_factors, rm_factors, rm_keyframe, filter_edges, clear_edges, update, update_lowmem, add_neighborhood_factors,
    add_proximity_factors, add_backend_proximity_factors`.  `update_op(net, inp, corr, motn, ii, jj) -> (net, delta, weight, damping,
    upmask)` is any callable with the signature of the reference's update operator; the graph does not contain the network.
    `corr_impl`: "volume" keeps a CorrBlock per edge (the frontend); "volume_fused" keeps one FusedCorrBlock over `video.fmaps`
    (max_factors + 16 slots, 64 when max_factors is unbounded; it grows when it must), adds edges into free slots, drops them from
    its slot list and looks every level up in one launch; "alt" and "alt_fused" keep none and differ only in the operator
    `update_lowmem` builds (AltCorrBlock, FusedAltCorrBlock).

    New edges that are already active or inactive are dropped, on the device (keys i * 2^31 + j, torch.isin).

    Kept quirk: when `add_factors(remove=True)` would exceed `max_factors`, the reference argsorts the ages and removes the edge at
    POSITION k when the k-th entry of that permutation is >= max_factors - (number of new edges): the mask is indexed by rank, not by
    edge.  It is kept as written, with a stable argsort.  A stereo edge (ii == jj) takes the second feature map of its frame when the
    video has one (`fmaps.shape[1] > 1`), the first otherwise.

    Host synchronisations, all of which the reference has too: boolean-mask indexing, `t0=None` in `update` (reads ii.min()), the
    chunk loop of `update_lowmem`, and one read of the edge count per selection (the reference: one read per candidate).
    """

    def __init__(self, video, update_op, device="cuda", corr_impl="volume", max_factors=-1):
        self.video, self.update_op, self.device = video, update_op, device
        self.max_factors, self.corr_impl = max_factors, corr_impl
        self.ht = ht = video.ht // video.down_scale
        self.wd = wd = video.wd // video.down_scale
        y, x = torch.meshgrid(torch.arange(ht, device=device).float(), torch.arange(wd, device=device).float(), indexing="ij")
        self.coords0 = torch.stack([x, y], dim=-1)
        self.corr, self.net, self.inp = None, None, None
        self.damping = 1e-6 * torch.ones_like(video.disps)
        for name in ("ii", "jj", "age", "ii_inac", "jj_inac", "ii_bad", "jj_bad"):
            setattr(self, name, torch.zeros(0, dtype=torch.long, device=device))
        for name in ("target", "weight", "target_inac", "weight_inac"):
            setattr(self, name, torch.zeros(1, 0, ht, wd, 2, dtype=torch.float, device=device))

    def _new_edges(self, ii, jj):
        """the edges of (ii, jj) that are neither active nor inactive"""
        key = lambda i, j: (i << 31) + j
        seen = torch.cat([key(self.ii, self.jj), key(self.ii_inac, self.jj_inac)])
        keep = ~torch.isin(key(ii, jj), seen)
        return ii[keep], jj[keep]

    def filter_edges(self):
        """moves the distant edges (|i - j| > 2) whose mean weight is below 0.001 to the bad list"""
        conf = torch.mean(self.weight, dim=[0, 2, 3, 4])
        mask = ((self.ii - self.jj).abs() > 2) & (conf < 0.001)
        self.ii_bad = torch.cat([self.ii_bad, self.ii[mask]])
        self.jj_bad = torch.cat([self.jj_bad, self.jj[mask]])
        self.rm_factors(mask, store=False)

    def clear_edges(self):
        for name in ("ii", "jj", "age", "corr", "damping", "net", "inp", "target", "weight", "ii_inac", "jj_inac", "ii_bad", "jj_bad",
                     "target_inac", "weight_inac"):
            setattr(self, name, None)

    @torch.no_grad()
    def add_factors(self, ii, jj, remove=False):
        ii, jj = self.video.format_indicies(ii, jj, self.device)
        ii, jj = self._new_edges(ii, jj)
        if ii.shape[0] == 0:
            return
        if self.max_factors > 0 and self.ii.shape[0] + ii.shape[0] > self.max_factors and self.corr is not None and remove:
            rank = torch.argsort(self.age, stable=True)
            self.rm_factors(rank >= self.max_factors - ii.shape[0], store=True)          # (the kept quirk of the class docstring)
        net = self.video.nets[ii].to(self.device).unsqueeze(0)
        if self.corr_impl == "volume":
            second = (ii == jj).long().clamp(max=self.video.fmaps.shape[1] - 1)
            with torch.autocast("cuda", enabled=True):
                corr = CorrBlock(self.video.fmaps[ii, 0].to(self.device).unsqueeze(0),
                                 self.video.fmaps[jj, second].to(self.device).unsqueeze(0))
            self.corr = corr if self.corr is None else self.corr.cat(corr)
        elif self.corr_impl == "volume_fused":
            if self.corr is None:
                self.corr = FusedCorrBlock(self.video.fmaps, capacity=self.max_factors + 16 if self.max_factors > 0 else 64)
            self.corr.add(ii, jj)
        if self.corr_impl in ("volume", "volume_fused"):
            inp = self.video.inps[ii].to(self.device).unsqueeze(0)
            self.inp = inp if self.inp is None else torch.cat([self.inp, inp], 1)
        target = reproject(self.video.poses, self.video.disps, self.video.intrinsics, ii.contiguous(), jj.contiguous())[0][None]
        self.ii = torch.cat([self.ii, ii])
        self.jj = torch.cat([self.jj, jj])
        self.age = torch.cat([self.age, torch.zeros_like(ii)])
        self.net = net if self.net is None else torch.cat([self.net, net], 1)
        self.target = torch.cat([self.target, target], 1)
        self.weight = torch.cat([self.weight, torch.zeros_like(target)], 1)

    def rm_factors(self, mask, store=False):
        """drops the masked edges; store=True keeps their targets and weights as inactive factors"""
        if store:
            self.ii_inac = torch.cat([self.ii_inac, self.ii[mask]])
            self.jj_inac = torch.cat([self.jj_inac, self.jj[mask]])
            self.target_inac = torch.cat([self.target_inac, self.target[:, mask]], 1)
            self.weight_inac = torch.cat([self.weight_inac, self.weight[:, mask]], 1)
        keep = ~mask
        self.ii, self.jj, self.age = self.ii[keep], self.jj[keep], self.age[keep]
        if self.corr_impl == "volume" and self.corr is not None:
            self.corr = self.corr[keep]
        elif self.corr_impl == "volume_fused" and self.corr is not None:
            self.corr = self.corr[keep, self.ii.shape[0]]
        if self.net is not None:
            self.net = self.net[:, keep]
        if self.inp is not None:
            self.inp = self.inp[:, keep]
        self.target, self.weight = self.target[:, keep], self.weight[:, keep]

    def rm_keyframe(self, ix):
        """frame ix + 1 takes the place of frame ix in the video; the edges of ix go, the indices above it move down by one"""
        v = self.video
        with v.get_lock():
            for buf in (v.timestamp, v.images, v.dirty, v.npc_dirty, v.poses, v.disps, v.disps_up, v.intrinsics, v.depth_scale,
                        v.depth_shift, v.mono_disps, v.valid_depth_mask, v.valid_depth_mask_small, v.nets, v.inps, v.fmaps):
                buf[ix] = buf[ix + 1]
        gone = (self.ii_inac == ix) | (self.jj_inac == ix)
        self.ii_inac = (self.ii_inac - (self.ii_inac >= ix).long())[~gone]
        self.jj_inac = (self.jj_inac - (self.jj_inac >= ix).long())[~gone]
        self.target_inac, self.weight_inac = self.target_inac[:, ~gone], self.weight_inac[:, ~gone]
        gone = (self.ii == ix) | (self.jj == ix)
        self.ii = self.ii - (self.ii >= ix).long()
        self.jj = self.jj - (self.jj >= ix).long()
        self.rm_factors(gone, store=False)

    def _motion(self):
        """coords [1,E,h,w,2] and the motion features [1,E,4,h,w] of the active edges, one launch"""
        v = self.video
        coords, _, motn = reproject(v.poses, v.disps, v.intrinsics, self.ii.contiguous(), self.jj.contiguous(),
                                    self.target[0].contiguous())
        return coords[None], motn[None]

    @torch.no_grad()
    def update(self, t0=None, t1=None, itrs=2, use_inactive=False, EP=1e-7, motion_only=False, opt_type="pose_depth"):
        """one pass of the update operator over the active edges, then bundle adjustment and upsampling"""
        coords1, motn = self._motion()
        with torch.autocast("cuda", enabled=True):
            corr = self.corr(coords1)
            self.net, delta, weight, damping, upmask = self.update_op(self.net, self.inp, corr, motn, self.ii, self.jj)
        if t0 is None:
            t0 = max(1, self.ii.min().item() + 1)
        self.target = coords1 + delta.float()
        self.weight = weight.float()
        self.damping[torch.unique(self.ii)] = damping
        if use_inactive:
            m = (self.ii_inac >= t0 - 3) & (self.jj_inac >= t0 - 3)
            ii = torch.cat([self.ii_inac[m], self.ii])
            jj = torch.cat([self.jj_inac[m], self.jj])
            target = torch.cat([self.target_inac[:, m], self.target], 1)
            weight = torch.cat([self.weight_inac[:, m], self.weight], 1)
        else:
            ii, jj, target, weight = self.ii, self.jj, self.target, self.weight
        eta = .2 * self.damping[torch.unique(ii)].contiguous() + EP
        self.video.ba(target, weight, eta, ii, jj, t0, t1, iters=itrs, lm=1e-4, ep=0.1, motion_only=motion_only, opt_type=opt_type)
        self.video.upsample(torch.unique(self.ii), upmask)
        self.age += 1

    @torch.no_grad()
    def update_lowmem(self, t0=None, t1=None, itrs=2, use_inactive=False, EP=1e-7, steps=8, enable_wq=True):
        """`steps` passes with the low-memory correlation operator (corr_impl "alt_fused": FusedAltCorrBlock, one launch per chunk;
        otherwise AltCorrBlock), the edges taken in chunks of 8 source frames"""
        num, rig, ch, ht, wd = self.video.fmaps.shape
        block = FusedAltCorrBlock if self.corr_impl == "alt_fused" else AltCorrBlock
        corr_op = block(self.video.fmaps.view(1, num * rig, ch, ht, wd))
        for step in range(steps):
            coords1, motn = self._motion()
            for first in range(0, int(self.jj.max()) + 1, 8):
                v = (self.ii >= first) & (self.ii < first + 8)
                if int(v.sum()) < 1:
                    continue
                iis, jjs = self.ii[v], self.jj[v]
                corr1 = corr_op(coords1[:, v], rig * iis, rig * jjs + (iis == jjs).long())
                with torch.autocast("cuda", enabled=True):
                    net, delta, weight, damping, upmask = self.update_op(self.net[:, v], self.video.inps[None, iis], corr1, motn[:, v],
                                                                         iis, jjs)
                    self.video.upsample(torch.unique(iis), upmask)
                self.net[:, v] = net
                self.target[:, v] = coords1[:, v] + delta.float()
                self.weight[:, v] = weight.float()
                self.damping[torch.unique(iis)] = damping
            eta = .2 * self.damping[torch.unique(self.ii)].contiguous() + EP
            opt_type = "depth_scale" if (enable_wq and step % 2 == 1) else "pose_depth"
            self.video.ba(self.target, self.weight, eta, self.ii, self.jj, t0, t1, iters=itrs, lm=1e-5, ep=1e-2, motion_only=False,
                          opt_type=opt_type)

    def add_neighborhood_factors(self, t0, t1, r=3):
        """edges between the frames of [t0, t1) that are at most r apart"""
        ii, jj = torch.meshgrid(torch.arange(t0, t1, device=self.device), torch.arange(t0, t1, device=self.device), indexing="ij")
        ii, jj = ii.reshape(-1), jj.reshape(-1)
        gap = (ii - jj).abs()
        keep = (gap > 0) & (gap <= r)
        self.add_factors(ii[keep], jj[keep])

    def _distance_matrix(self, first_row, first_col, end, beta):
        ii, jj = torch.meshgrid(torch.arange(first_row, end), torch.arange(first_col, end), indexing="ij")
        return self.video.distance(ii.reshape(-1), jj.reshape(-1), beta=beta).contiguous()

    def add_proximity_factors(self, t0=0, t1=0, rad=2, nms=2, beta=0.25, thresh=16.0, remove=False):
        """the frontend's edges: the local windows, then the closest frame pairs under non-maximum suppression"""
        t = self.video.counter.value
        if max(t - t0, t - t1) > nat.SGR_GRAPH_MAX_SIDE:
            raise ValueError(f"FactorGraph.add_proximity_factors: a {t - t0} x {t - t1} distance matrix exceeds the supported "
                             f"{nat.SGR_GRAPH_MAX_SIDE} x {nat.SGR_GRAPH_MAX_SIDE}")
        d = self._distance_matrix(t0, t1, t, beta)
        ii, jj = select_proximity_edges(d, t0, t1, t, torch.cat([self.ii, self.ii_bad, self.ii_inac]),
                                        torch.cat([self.jj, self.jj_bad, self.jj_inac]), rad, nms, thresh, self.max_factors)
        self.add_factors(ii, jj, remove)

    def add_backend_proximity_factors(self, t_start, t_end, nms, radius, thresh, max_factors, beta, t_start_loop=None, loop=False):
        """the backend's edges; returns the number of active edges afterwards, or 0 when nothing was added"""
        if t_start_loop is None or not loop:
            t_start_loop = t_start
        if t_start_loop < t_start:
            raise ValueError(f"FactorGraph.add_backend_proximity_factors: t_start_loop ({t_start_loop}) precedes t_start ({t_start})")
        if t_end - t_start > nat.SGR_GRAPH_MAX_SIDE:
            raise ValueError(f"FactorGraph.add_backend_proximity_factors: a {t_end - t_start_loop} x {t_end - t_start} distance matrix "
                             f"exceeds the supported {nat.SGR_GRAPH_MAX_SIDE} x {nat.SGR_GRAPH_MAX_SIDE}")
        d = self._distance_matrix(t_start_loop, t_start, t_end, beta)
        ii, jj, num_loop = select_backend_edges(d, t_start, t_end, t_start_loop, loop, nms, radius, thresh, max_factors)
        if ii.shape[0] < 3 or (loop and num_loop == 0):
            return 0
        self.add_factors(ii, jj, remove=True)
        return self.ii.shape[0]
