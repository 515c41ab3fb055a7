"""Novel-view evaluation ("Novel-view evaluation"): the rendering metrics of eval_rendering at frames of the
stream that the mapper never saw.  The reference's eval_rendering (src/utils/eval_utils.py:64-197) scores the mapped keyframes only,
the views the map was optimised on; it has no counterpart of this module, so the conventions here are the project's own.

    select_frames(num_frames, keyframe_timestamps, every=5, first=0) -> list[int]
        first, first + every, ... below num_frames, without every timestamp of keyframe_timestamps (every registered keyframe,
        mapped or not: a frame the tracker kept is no held-out frame).
    interpolate_exposure(kf_timestamps, kf_a, kf_b, timestamps) -> (a [M], b [M])
        host, fp64: the exposure of the mapped keyframes, linear in time between the two that bracket a stamp, constant outside them.
        The first mapped keyframe counts as (0, 0) whatever it stores: eval_rendering never applies its exposure.
    eval_novel_views(loop_or_session, stream, c2w, frame_ids, exposure="fit", global_scale=1.0, lpips=None, kf_timestamps=None) -> dict
        c2w [T,4,4]: camera -> world of every frame of the stream in the map's frame (traj_est of traj_eval.full_traj_eval);
        frame_ids: the frames to score, stream[i] -> (timestamp, colour [3,H,W] or [1,3,H,W], depth [H,W] or None, ...).
        exposure: "fit": per frame the gain and bias that fit the render to the ground truth in the least-squares sense over gt > 0
        (sgr_exposure_fit, on the device between the renders and the metrics); "keyframes": interpolate_exposure of the mapped
        keyframes' (kf_timestamps: their stamps in the order of sorted(loop.viewpoints); default the session's, or the keys
        themselves for a bare loop); "none": the render as it is.
        Returns frame_ids, psnr, ssim, depth_l1, mean_psnr, mean_ssim, mean_depthl1 (eval_rendering's names), exposure_a, exposure_b,
        exposure_flags (1: the fit was degenerate and the identity was used), and lpips / mean_lpips with an LPIPS object.
        The ground truth of the whole selection is read before anything is rendered (a frame of another shape is a ValueError) and
        stays on the device for the call; renders live for a chunk of 16 frames.  One copy to the host per call, one more for LPIPS.

HIP only: frames on the CPU are a RuntimeError, as in eval_rendering."""
import numpy as np
import torch

from splat_slam_amd import _native as nat

__all__ = ["select_frames", "interpolate_exposure", "eval_novel_views", "EXPOSURE_MODES"]

EXPOSURE_MODES = ("fit", "keyframes", "none")
_CHUNK = 16                 # frames rendered, fitted and measured per launch chain (SGR_EXPOSURE_FIT_MAX_FRAMES)


def select_frames(num_frames, keyframe_timestamps, every=5, first=0):
    every, first = int(every), int(first)
    if every < 1 or first < 0:
        raise ValueError(f"select_frames: every={every} must be >= 1 and first={first} >= 0")
    taken = {int(round(float(t))) for t in keyframe_timestamps}
    return [i for i in range(first, int(num_frames), every) if i not in taken]


def interpolate_exposure(kf_timestamps, kf_a, kf_b, timestamps):
    ts = np.asarray(kf_timestamps, dtype=np.float64).reshape(-1)
    a = np.array(kf_a, dtype=np.float64).reshape(-1)
    b = np.array(kf_b, dtype=np.float64).reshape(-1)
    if len(ts) < 1 or len(a) != len(ts) or len(b) != len(ts):
        raise ValueError(f"interpolate_exposure: {len(ts)} stamps, {len(a)} and {len(b)} exposure values")
    if np.any(np.diff(ts) <= 0):
        raise ValueError("interpolate_exposure: the keyframes' stamps must increase")
    a[0] = b[0] = 0.0                               # the first mapped keyframe is rendered without its exposure
    t = np.asarray(timestamps, dtype=np.float64).reshape(-1)
    if len(ts) == 1:
        return np.full(len(t), a[0]), np.full(len(t), b[0])
    hi = np.clip(np.searchsorted(ts, t, side="right"), 1, len(ts) - 1)              # ts[hi - 1] <= t < ts[hi] inside the range
    lo = hi - 1
    w = (t - ts[lo]) / (ts[hi] - ts[lo])
    before, after = t <= ts[0], t >= ts[-1]                                         # constant outside, the end values as they are
    pick = lambda v: np.where(after, v[-1], np.where(before, v[0], v[lo] + w * (v[hi] - v[lo])))
    return pick(a), pick(b)


def _setup(obj):
    """(loop, intrinsics dict, projection matrix, stamps of the mapped keyframes) of a MappingSession or of a bare loop"""
    if hasattr(obj, "loop"):
        loop = obj.loop
        stamp = dict(zip(obj.video_idxs, obj.keyframe_idxs))
        return loop, obj.intr, obj.projection_matrix, [float(stamp.get(k, k)) for k in sorted(loop.viewpoints)]
    if not obj.viewpoints:
        raise ValueError("eval_novel_views: the loop has no mapped viewpoint")
    keys = sorted(obj.viewpoints)
    v = obj.viewpoints[keys[0]]
    intr = dict(W=int(v.image_width), H=int(v.image_height), fx=v.fx, fy=v.fy, cx=v.cx, cy=v.cy)
    return obj, intr, v.projection_matrix, [float(k) for k in keys]


def _w2c_of(c2w, ids):
    """the selected camera -> world rows in one copy to the host, inverted as rigid transforms in fp64: [R | t]^-1 = [R^T | -R^T t]"""
    if torch.is_tensor(c2w):
        rows = c2w.detach().index_select(0, torch.as_tensor(ids, dtype=torch.long, device=c2w.device)).double().cpu().numpy()
    else:
        rows = np.stack([np.asarray(c2w[i], dtype=np.float64) for i in ids])
    if rows.shape[1:] != (4, 4):
        raise ValueError(f"eval_novel_views: c2w rows are {rows.shape[1:]}, not 4 x 4")
    out = np.tile(np.eye(4), (len(ids), 1, 1))
    rt = rows[:, :3, :3].transpose(0, 2, 1)
    out[:, :3, :3] = rt
    out[:, :3, 3] = -np.einsum("nij,nj->ni", rt, rows[:, :3, 3])
    return out


@torch.no_grad()
def eval_novel_views(loop_or_session, stream, c2w, frame_ids, exposure="fit", global_scale=1.0, lpips=None, kf_timestamps=None):
    from splat_slam_amd.camera import Camera, focal2fov
    from splat_slam_amd.eval import _device_depth
    from splat_slam_amd.mapper import PipelineParams
    from splat_slam_amd.renderer import render
    if exposure not in EXPOSURE_MODES:
        raise ValueError(f"eval_novel_views: exposure={exposure!r}, one of {EXPOSURE_MODES}")
    ids = [int(i) for i in frame_ids]
    if not ids:
        raise ValueError("eval_novel_views: no frames")
    loop, intr, proj, stamps = _setup(loop_or_session)
    if kf_timestamps is not None:
        stamps = [float(t) for t in kf_timestamps]
    n_poses = len(c2w)
    if min(ids) < 0 or max(ids) >= n_poses:
        raise ValueError(f"eval_novel_views: frames {min(ids)} .. {max(ids)} of a trajectory of {n_poses} poses")
    C, H, W = 3, int(intr["H"]), int(intr["W"])
    # ---- the ground truth of every selected frame, checked before anything is rendered
    colors, depths, dev = [], [], None
    for i in ids:
        item = stream[i]
        color, depth = item[1], item[2]
        if not torch.is_tensor(color) or color.device.type != "cuda":
            raise RuntimeError("eval_novel_views needs GPU tensors (HIP only, no CPU fallback)")
        if color.dim() == 4 and color.shape[0] == 1:
            color = color[0]
        if tuple(color.shape) != (C, H, W):
            raise ValueError(f"eval_novel_views: frame {i} is {tuple(color.shape)}, the map's frames are {(C, H, W)}")
        if depth is not None and tuple(depth.shape[-2:]) != (H, W):
            raise ValueError(f"eval_novel_views: the depth of frame {i} is {tuple(depth.shape)}, the map's frames are {(H, W)}")
        dev = color.device if dev is None else dev
        colors.append(color.detach().to(dtype=torch.float32, device=dev).contiguous())
        depths.append(None if depth is None else _device_depth(depth, dev))
    lib = nat.lib()
    n = len(ids)
    lp_out = None
    if lpips is not None:
        from splat_slam_amd.lpips import tap_sizes
        tap_sizes(H, W)
        if lpips.device != (dev if dev.index is not None else torch.device("cuda", torch.cuda.current_device())):
            raise RuntimeError(f"eval_novel_views(lpips=...): the frames are on {dev}, the metric on {lpips.device}")
        lp_out = torch.empty(n, dtype=torch.float32, device=dev)
    w2c = torch.from_numpy(_w2c_of(c2w, ids).astype(np.float32)).to(dev)            # one upload; the cameras hold views of it
    host_ab = None
    if exposure == "keyframes":
        if len(stamps) != len(loop.viewpoints):
            raise ValueError(f"eval_novel_views: {len(stamps)} keyframe stamps for {len(loop.viewpoints)} mapped viewpoints")
        views = [loop.viewpoints[k] for k in sorted(loop.viewpoints)]
        kf = torch.cat([torch.cat([v.exposure_a.detach().reshape(1), v.exposure_b.detach().reshape(1)]) for v in views]).double().cpu()
        kf = kf.view(len(views), 2).numpy()
        host_ab = np.stack(interpolate_exposure(stamps, kf[:, 0], kf[:, 1], [float(i) for i in ids]), axis=1)
    # ---- one arena: metrics [n,3], exposure [n,2], flags [n] (int32 bits), then the two scratch areas
    metric_bytes = lib.sgr_ssim_scratch_bytes(_CHUNK, C, H, W)
    fit_bytes = lib.sgr_exposure_fit_bytes(min(n, _CHUNK), C, H, W) if exposure == "fit" else 0
    if exposure == "fit" and fit_bytes == 0:
        raise ValueError(f"eval_novel_views: sgr_exposure_fit does not take frames of {(C, H, W)}")
    arena = torch.empty(6 * n + 64 + (metric_bytes + fit_bytes) // 4 + 128, dtype=torch.float32, device=dev)
    arena[:6 * n].zero_()
    out, ab, flags = arena[:3 * n], arena[3 * n:5 * n], arena[5 * n:6 * n].view(torch.int32)
    pad = lambda t: t[(-t.data_ptr() // 4) % 64:]                                  # scratch starts on a 256-byte boundary
    metric_scratch = pad(arena[6 * n:])
    fit_scratch = pad(metric_scratch[metric_bytes // 4:])
    if host_ab is not None:
        ab.copy_(torch.from_numpy(host_ab.astype(np.float32).reshape(-1)))          # one upload, [n,2]
    stream_ptr = torch.cuda.current_stream().cuda_stream
    bg, pipe = loop.background, PipelineParams()
    fovx, fovy = focal2fov(intr["fx"], W), focal2fov(intr["fy"], H)
    for c0 in range(0, n, _CHUNK):
        keep, table = [], (nat.SgrMetricFrame * min(_CHUNK, n - c0))()
        for i, k in enumerate(range(c0, c0 + len(table))):
            # a Camera as MappingSession._camera builds one: the session's intrinsics and projection, then update_RT
            cam = Camera(ids[k], colors[k], depths[k], w2c[k], proj, intr["fx"], intr["fy"], intr["cx"], intr["cy"], fovx, fovy, H, W,
                         device=loop.device)
            cam.update_RT(cam.R_gt, cam.T_gt)
            pkg = render(cam, loop.gaussians, pipe, bg)
            r, d = pkg["render"].detach().contiguous(), pkg["depth"].detach().contiguous()
            if tuple(r.shape) != (C, H, W):
                raise ValueError(f"eval_novel_views: the render of frame {ids[k]} is {tuple(r.shape)}, not {(C, H, W)}")
            keep += [r, d]
            pa, pb = (None, None) if exposure == "none" else (ab[2 * k:].data_ptr(), ab[2 * k + 1:].data_ptr())
            table[i] = nat.SgrMetricFrame(r.data_ptr(), colors[k].data_ptr(), d.data_ptr(), nat.ptr(depths[k]), pa, pb)
        if exposure == "fit":
            nat.check(lib.sgr_exposure_fit(len(table), table, C, H, W, ab[2 * c0:].data_ptr(), flags[c0:].data_ptr(),
                                           fit_scratch.data_ptr(), fit_bytes, stream_ptr), "sgr_exposure_fit")
        nat.check(lib.sgr_render_metrics(len(table), table, C, H, W, float(global_scale), out[3 * c0:].data_ptr(),
                                         metric_scratch.data_ptr(), metric_bytes, stream_ptr), "sgr_render_metrics")
        if lpips is not None:
            lpips.frames(table, H, W, lp_out[c0:])
    host = arena[:6 * n].cpu()                                                      # the one copy to the host
    vals = host[:3 * n].view(n, 3).double()
    psnr_l, ssim_l, depth_l = (vals[:, j].tolist() for j in range(3))
    hab = host[3 * n:5 * n].view(n, 2).double()
    result = {"frame_ids": ids, "psnr": psnr_l, "ssim": ssim_l, "depth_l1": depth_l, "mean_psnr": float(np.mean(psnr_l)),
              "mean_ssim": float(np.mean(ssim_l)), "mean_depthl1": float(np.mean(depth_l)), "exposure_a": hab[:, 0].tolist(),
              "exposure_b": hab[:, 1].tolist(), "exposure_flags": host[5 * n:6 * n].view(torch.int32).tolist()}
    if lpips is not None:
        result["lpips"] = lp_out.cpu().double().tolist()                            # one more copy to the host
        result["mean_lpips"] = float(np.mean(result["lpips"]))
    return result
