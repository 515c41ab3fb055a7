"""Rendering metrics of eval_rendering, /root/reference/src/utils/eval_utils.py:64-197: PSNR (psnr() of
/root/reference/thirdparty/gaussian_splatting/utils/image_utils.py:19-21), SSIM (the reference's own in-tree
loss_utils.ssim, thirdparty/gaussian_splatting/utils/loss_utils.py:61-101) and the rendered depth's L1 error.
`eval_rendering` computes all three on the HIP kernels (sgr_render_metrics); `eval_rendering_psnr` is the PSNR-only
torch formulation.  With mesh=True, eval_rendering also fuses every frame into a TSDF volume and returns the cleaned
mesh (:70-74, 142-179, clean_mesh :331-379) from the HIP kernels of splat_slam_amd.mesh; given a ground-truth mesh it also
scores that mesh (:174-187: accuracy, completion, completion ratio, precision, F-score and chamfer-L1 after ICP alignment) on the
HIP kernels of splat_slam_amd.mesh_eval.  Given an `splat_slam_amd.lpips.LPIPS` object, eval_rendering also reports LPIPS (:66-68, 125,
192) from the HIP kernels of splat_slam_amd.lpips; the project ships no trained AlexNet weights, the object loads the caller's."""
import functools
import inspect

import numpy as np
import torch

from splat_slam_amd import _native as nat
from splat_slam_amd.renderer import render


def psnr(img1, img2):
    mse = ((img1 - img2) ** 2).view(img1.shape[0], -1).mean(1, keepdim=True)
    return 20 * torch.log10(1.0 / torch.sqrt(mse))


@torch.no_grad()
def eval_rendering_psnr(frames, gaussians, pipe, background):
    """frames: list of Camera in keyframe order; exposure compensation is applied to every frame but the first
    (eval_utils.py:96-99); PSNR over pixels where the ground truth is > 0 (:109,123)."""
    scores = []
    for k, frame in enumerate(frames):
        rendering = render(frame, gaussians, pipe, background)["render"].detach()
        image = torch.exp(frame.exposure_a.detach()) * rendering + frame.exposure_b.detach() if k > 0 else rendering
        image = torch.clamp(image, 0.0, 1.0)
        gt = frame.original_image
        mask = gt > 0
        scores.append(psnr(image[mask].unsqueeze(0), gt[mask].unsqueeze(0)).item())
    return scores


_METRIC_CHUNK = 16          # frames rendered, then measured in one launch (renders of a chunk stay alive until it is measured)


def _device_depth(d, device):
    if not torch.is_tensor(d):
        d = torch.from_numpy(d)
    return d.to(dtype=torch.float32, device=device).reshape(d.shape[-2:]).contiguous()


def _with_mesh_culling(fn):
    """eval_rendering plus two opt-in keywords, as a stage around the function: cull_mesh=True scores the meshes after culling them.
    The function itself, its parameter list and its defaults stay what tests/test_lpips_cpu.py pins."""
    @functools.wraps(fn)
    def eval_rendering(*args, cull_mesh=False, cull_poses=None, **kwargs):
        a = inspect.signature(fn).bind(*args, **kwargs)
        a.apply_defaults()
        a = a.arguments
        if not (cull_mesh and a["mesh"] and a["eval_mesh"] and a["gt_mesh_path"] is not None):
            return fn(*args, **kwargs)
        result = fn(**{**a, "eval_mesh": False})
        from splat_slam_amd.mesh_eval import evaluate_mesh
        frames = a["frames"]
        poses = cull_poses if cull_poses is not None else a["c2w"]
        if poses is None:
            poses = [torch.linalg.inv(p) for p in _w2c(frames)]
        try:
            pred, gt = _culled(result, result["mesh"], a["gt_mesh_path"], frames, poses)
            result["mesh_metrics"] = evaluate_mesh(pred, gt, distance_thresh=a["distance_thresh"], icp_align=a["icp_align"],
                                                   samples=a["mesh_samples"])
        except ValueError as e:
            result["mesh_metrics_error"] = str(e)
        return result
    return eval_rendering


@_with_mesh_culling
@torch.no_grad()
def eval_rendering(frames, gaussians, pipe, background, gt_depths=None, global_scale=1.0, mesh=False, mesh_path=None, c2w=None,
                   voxel_length=5.0 / 512.0, sdf_trunc=0.04, eval_mesh=True, gt_mesh_path=None, distance_thresh=0.05, icp_align=True,
                   mesh_samples=200_000, lpips=None):
    """eval_rendering's per-frame metrics (eval_utils.py:90-128, means as :190-194) on the HIP kernels: frames is a list of Camera
    in keyframe order; every frame but the first gets its exposure compensation (:96-99), the image is clamped to [0, 1];
    PSNR over the elements where the ground truth is > 0 (:109,123), SSIM of the whole image (:124), depth L1 of
    global_scale * rendered depth over pixels where both depths are > 0 (:116-120).  gt_depths: one [H,W] per frame (default:
    each frame's `depth`).  One copy to the host per call.  A frame without a valid depth pixel gives NaN (the reference's 0/0), a
    perfect frame PSNR inf.
    lpips: an splat_slam_amd.lpips.LPIPS object (:66-68, 125): the result gains "lpips", LPIPS(image, ground truth) per frame on the
    same clamped, exposure-compensated image, and "mean_lpips" (:192); each chunk of 16 frames is measured from the table of
    sgr_render_metrics while its renders are alive, and the values come back in one more copy to the host.  Frames must be 3 x H x W
    with H and W at least 31 (ValueError before anything is rendered).  With None the result is what it is without the argument.
    mesh=True (:70-74, 142-179): each frame's render of the metrics chunk is also fused into a TSDF volume (voxel_length, sdf_trunc,
    depth_trunc 30) with the exposure-compensated colour and global_scale * rendered depth, dropped where the ground-truth depth is
    0, at the pose c2w[k] (camera -> world 4x4, the reference's traj_est_aligned; default each frame's own pose).  The result gains
    "mesh", the cleaned TriangleMesh, written as PLY to mesh_path when given.
    eval_mesh with a ground-truth mesh gt_mesh_path (a PLY path or a TriangleMesh; :174-187): the result also gains "mesh_metrics",
    splat_slam_amd.mesh_eval.evaluate_mesh(mesh, gt, distance_thresh, icp_align, samples=mesh_samples), or, where that raises
    ValueError (e.g. a mesh without a triangle of positive area), "mesh_metrics_error" with its message, as the reference's
    try/except does.  Without a ground-truth mesh the result is what it is without these arguments.
    Two more keywords, cull_mesh=False and cull_poses=None (_with_mesh_culling; nothing is culled by default): with cull_mesh=True and
    a ground-truth mesh, the cleaned mesh and the ground truth are both culled, before they are scored, to what the poses cull_poses
    (camera -> world 4x4 each; default the fusion poses) see, by splat_slam_amd.mesh_cull.cull_mesh with the frames' intrinsics and
    size (frame k's for pose k when there is one pose per frame, else the first frame's) and occlusion from each mesh's own depth.
    The result gains "mesh_cull" ({"pred", "gt"}: the counts of cull_mesh's info) and "gt_mesh_culled"; "mesh" and the written PLY
    stay the unculled mesh.  A culled mesh without faces ends in "mesh_metrics_error"."""
    if not frames:
        raise ValueError("eval_rendering: no frames")
    if gt_depths is not None and len(gt_depths) != len(frames):
        raise ValueError(f"eval_rendering: {len(gt_depths)} ground-truth depths for {len(frames)} frames")
    if c2w is not None and len(c2w) != len(frames):
        raise ValueError(f"eval_rendering: {len(c2w)} poses for {len(frames)} frames")
    lib = nat.lib()
    dev = frames[0].original_image.device
    if dev.type != "cuda":
        raise RuntimeError("eval_rendering needs GPU tensors (HIP only, no CPU fallback)")
    C, H, W = frames[0].original_image.shape
    n = len(frames)
    lp_out = None
    if lpips is not None:
        from splat_slam_amd.lpips import tap_sizes
        if C != 3:
            raise ValueError(f"eval_rendering(lpips=...): colour frames must have 3 channels, not {C}")
        tap_sizes(H, W)
        if lpips.device != (dev if dev.index is not None else torch.device("cuda", torch.cuda.current_device())):
            raise RuntimeError(f"eval_rendering(lpips=...): the frames are on {dev}, the metric on {lpips.device}")
        lp_out = torch.empty(n, dtype=torch.float32, device=dev)
    scratch_bytes = lib.sgr_ssim_scratch_bytes(_METRIC_CHUNK, C, H, W)
    arena = torch.empty(3 * n + scratch_bytes // 4, dtype=torch.float32, device=dev)
    out, scratch = arena[:3 * n], arena[3 * n:]
    stream = torch.cuda.current_stream().cuda_stream
    volume = poses = None
    if mesh:
        from splat_slam_amd.mesh import TSDFVolume
        volume = TSDFVolume(voxel_length=voxel_length, sdf_trunc=sdf_trunc, depth_trunc=30.0, device=dev)
        poses = _w2c(frames) if c2w is None else [torch.linalg.inv(torch.as_tensor(p).detach().double().cpu()) for p in c2w]
    for c0 in range(0, n, _METRIC_CHUNK):
        keep, table = [], (nat.SgrMetricFrame * min(_METRIC_CHUNK, n - c0))()
        fuse = (nat.SgrTsdfFrame * len(table))() if mesh else None
        for i, k in enumerate(range(c0, c0 + len(table))):
            frame = frames[k]
            pkg = render(frame, gaussians, pipe, background)
            r, d = pkg["render"].contiguous(), pkg["depth"].contiguous()
            gt = frame.original_image.contiguous()
            gd = _device_depth(frame.depth if gt_depths is None else gt_depths[k], dev)
            if tuple(gt.shape) != (C, H, W) or tuple(r.shape) != (C, H, W) or gt.dtype != torch.float32:
                raise ValueError(f"eval_rendering: frame {k} is {tuple(gt.shape)} {gt.dtype}, not fp32 {(C, H, W)}")
            a, b = (frame.exposure_a, frame.exposure_b) if k > 0 else (None, None)
            a = None if a is None else a.detach().float().contiguous()
            b = None if b is None else b.detach().float().contiguous()
            keep += [r, d, gt, gd, a, b]
            table[i] = nat.SgrMetricFrame(r.data_ptr(), gt.data_ptr(), d.data_ptr(), gd.data_ptr(), nat.ptr(a), nat.ptr(b))
            if mesh:
                pose = poses[k]
                fuse[i] = nat.SgrTsdfFrame(r.data_ptr(), d.data_ptr(), gd.data_ptr(), nat.ptr(a), nat.ptr(b), float(frame.fx),
                                           float(frame.fy), float(frame.cx), float(frame.cy),
                                           (nat.C.c_float * 16)(*[float(x) for x in pose.reshape(-1)]), float(global_scale))
        nat.check(lib.sgr_render_metrics(len(table), table, C, H, W, float(global_scale), out[3 * c0:].data_ptr(), scratch.data_ptr(),
                                         scratch_bytes, stream), "sgr_render_metrics")
        if lpips is not None:
            lpips.frames(table, H, W, lp_out[c0:])
        if mesh:
            if C != 3:
                raise ValueError(f"eval_rendering(mesh=True): colour frames must have 3 channels, not {C}")
            volume._integrate_table(fuse, H, W)
    vals = out.view(n, 3).cpu().double()            # the one copy to the host
    psnr_l, ssim_l, depth_l = (vals[:, j].tolist() for j in range(3))
    result = {"psnr": psnr_l, "ssim": ssim_l, "depth_l1": depth_l, "mean_psnr": float(np.mean(psnr_l)),
              "mean_ssim": float(np.mean(ssim_l)), "mean_depthl1": float(np.mean(depth_l))}
    if lpips is not None:
        result["lpips"] = lp_out.cpu().double().tolist()            # one more copy to the host
        result["mean_lpips"] = float(np.mean(result["lpips"]))
    if mesh:
        from splat_slam_amd.mesh import clean_mesh
        result["mesh"] = clean_mesh(volume.extract_triangle_mesh(), min_len=100)
        if mesh_path is not None:
            result["mesh"].write_ply(mesh_path)
        if eval_mesh and gt_mesh_path is not None:
            from splat_slam_amd.mesh_eval import evaluate_mesh
            try:
                result["mesh_metrics"] = evaluate_mesh(result["mesh"], gt_mesh_path, distance_thresh=distance_thresh,
                                                       icp_align=icp_align, samples=mesh_samples)
            except ValueError as e:
                result["mesh_metrics_error"] = str(e)
    return result


def _culled(result, pred, gt, frames, c2w):
    """both meshes culled to the poses c2w; fills result["mesh_cull"] and result["gt_mesh_culled"]"""
    from splat_slam_amd.mesh_cull import cull_mesh
    from splat_slam_amd.mesh_eval import _as_mesh
    H, W = frames[0].original_image.shape[1:]
    use = frames if len(c2w) == len(frames) else frames[:1]
    intr = [[float(f.fx), float(f.fy), float(f.cx), float(f.cy)] for f in use]
    gt = _as_mesh(gt, frames[0].original_image.device)
    counts = ("vertices_before", "vertices_after", "faces_before", "faces_after", "unrasterized_triangles")
    out, result["mesh_cull"] = [], {}
    for name, m in (("pred", pred), ("gt", gt)):
        culled, info = cull_mesh(m, c2w, intr, H, W, return_info=True)
        result["mesh_cull"][name] = {k: info[k] for k in counts}
        out.append(culled)
    result["gt_mesh_culled"] = out[1]
    return out


def _w2c(frames):
    """every frame's own world -> camera pose, host fp64, in one copy"""
    from splat_slam_amd.camera import getWorld2View2
    return torch.stack([getWorld2View2(f.R, f.T).detach() for f in frames]).double().cpu()
