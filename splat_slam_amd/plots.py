"""The pictures of the reference's evaluation ("Plots"): the 2 x 3 figure per mapped keyframe
(the reference's src/utils/eval_utils.py:131-135, plot_rgbd_silhouette), the GIF of those figures (create_gif_from_directory) and the
trajectory plot (src/utils/eval_traj.py, traj_eval_and_plot).  The per-keyframe figure is composed on the device by sgr_plot_panels
(csrc/sgr_plot.hip): no matplotlib, one copy to the host per 16 frames, the PNG encoder of Pillow on the calling thread.

    compose_panels(renders, gt_images, depths, gt_depths, headings, titles, s=1, exposures=None, global_scale=1.0, depth_max=5.0)
        -> uint8 [n, PH, PW, 3] on the device; panel_size(H, W, s) -> (PH, PW).  renders, gt_images: n fp32 [3,H,W]; depths, gt_depths:
        n fp32 [H,W]; headings: n strings; titles: n lists of six strings, cell (r, c) at 3 r + c; exposures: n pairs (a, b) of device
        scalars or None.
    plot_rendering(frames, gaussians, pipe, background, metrics, out_dir, names, gt_depths=None, global_scale=1.0, depth_max=5.0,
                   gif=True) -> {"files", "gif", "s", "panel_size", "compose_s", "copy_s", "encode_s", "gif_s"}
        out_dir is the reference's plots_<iteration> directory.  The frames are rendered again, 16 at a time (eval_rendering's renders do
        not outlive its chunk and its parameter list is pinned): the price of the figures is a second forward per keyframe.
    plot_trajectory(alignment, path, title) -> (width, height)
        the 2D xy plot on the host with Pillow's ImageDraw: one figure per run, a few thousand segments, no hot path.
"""
import functools
import os
import re
import time

import numpy as np
import torch

from splat_slam_amd import _native as nat

__all__ = ["compose_panels", "panel_size", "reduction_factor", "plot_rendering", "plot_trajectory", "jet_table", "TITLES", "MAX_CELL_WIDTH",
           "TRAJ_SIZE", "TRAJ_GRAY", "trajectory_projection", "segment_colors"]

CHUNK = nat.SGR_PLOT_MAX_FRAMES
MAX_CELL_WIDTH = 640            # the reference's figure is about half size at 1200 wide
TITLES = ("Ground Truth RGB", "Input Depth", "Diff RGB L1", "Rasterized RGB, PSNR: {:.2f}", "Rasterized Depth, L1: {:.2f}", "Diff Depth L1")
_pending = []                   # (event, table): sgr_plot_panels copies the table on the stream, so it lives until the stream has passed


def panel_size(H, W, s):
    ph, pw = nat.C.c_int32(), nat.C.c_int32()
    nat.lib().sgr_plot_panel_size(int(H), int(W), int(s), nat.C.byref(ph), nat.C.byref(pw))
    if ph.value == 0:
        raise ValueError(f"panel_size: H, W must lie in 1 .. 16384 and s be at least 1, got {(H, W, s)}")
    return ph.value, pw.value


def reduction_factor(W, limit=MAX_CELL_WIDTH):
    """the smallest integer s with ceil(W / s) <= limit"""
    return max(1, -(-int(W) // limit))


def _text(s, what):
    raw = s.encode("latin-1", "replace") if isinstance(s, str) else bytes(s)
    if len(raw) > nat.SGR_PLOT_TEXT - 1:
        raise ValueError(f"{what}: {len(raw)} bytes, at most {nat.SGR_PLOT_TEXT - 1} fit")
    return raw


def _f32(t, shape, what):
    if not torch.is_tensor(t) or t.device.type != "cuda":
        raise RuntimeError("splat_slam_amd.plots needs GPU tensors (HIP only, no CPU fallback)")
    if tuple(t.shape) != shape or t.dtype != torch.float32:
        raise ValueError(f"{what} must be fp32 {shape}, got {t.dtype} {tuple(t.shape)}")
    return t.detach().contiguous()


@torch.no_grad()
def compose_panels(renders, gt_images, depths, gt_depths, headings, titles, s=1, exposures=None, global_scale=1.0, depth_max=5.0):
    n = len(renders)
    if n == 0 or not (len(gt_images) == len(depths) == len(gt_depths) == len(headings) == len(titles) == n):
        raise ValueError("compose_panels: one render, ground truth, depth pair, heading and title list per frame, at least one frame")
    if exposures is not None and len(exposures) != n:
        raise ValueError(f"compose_panels: {len(exposures)} exposures for {n} frames")
    H, W = (int(v) for v in depths[0].shape[-2:])
    PH, PW = panel_size(H, W, s)
    lib = nat.lib()
    keep, table = [], (nat.SgrPlotFrame * n)()
    for i in range(n):
        r, g = _f32(renders[i], (3, H, W), "render"), _f32(gt_images[i], (3, H, W), "gt_image")
        d, gd = _f32(depths[i].reshape(depths[i].shape[-2:]), (H, W), "depth"), _f32(gt_depths[i].reshape(gt_depths[i].shape[-2:]), (H, W), "gt_depth")
        a, b = (None, None) if exposures is None or exposures[i] is None else exposures[i]
        a = None if a is None else a.detach().float().contiguous()
        b = None if b is None else b.detach().float().contiguous()
        if len(titles[i]) != 6:
            raise ValueError(f"compose_panels: frame {i} has {len(titles[i])} titles, not 6")
        keep += [r, g, d, gd, a, b]
        f = table[i]
        f.render, f.gt_image, f.depth, f.gt_depth, f.exposure_a, f.exposure_b = (r.data_ptr(), g.data_ptr(), d.data_ptr(), gd.data_ptr(),
                                                                                nat.ptr(a), nat.ptr(b))
        text = bytearray(7 * nat.SGR_PLOT_TEXT)          # the heading, then the six titles: the struct's two char arrays are adjacent
        for k, t in enumerate([headings[i], *titles[i]]):
            raw = _text(t, "heading" if k == 0 else "title")
            text[k * nat.SGR_PLOT_TEXT:k * nat.SGR_PLOT_TEXT + len(raw)] = raw
        nat.C.memmove(nat.C.addressof(f) + nat.SgrPlotFrame.heading.offset, bytes(text), len(text))
    dev = keep[0].device
    nbytes = lib.sgr_plot_scratch_bytes(n)
    with torch.cuda.device(dev):
        panels = torch.empty((n, PH, PW, 3), dtype=torch.uint8, device=dev)
        scratch = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        nat.check(lib.sgr_plot_panels(n, table, H, W, int(s), float(global_scale), float(depth_max), panels.data_ptr(), scratch.data_ptr(),
                                      nbytes, torch.cuda.current_stream().cuda_stream), "sgr_plot_panels")
        done = torch.cuda.Event()
        done.record()
    _pending[:] = [p for p in _pending if not p[0].query()] + [(done, table)]
    return panels


def frame_titles(psnr, depth_l1):
    return [t.format(psnr) if "PSNR" in t else (t.format(depth_l1) if "L1: " in t else t) for t in TITLES]


@torch.no_grad()
def plot_rendering(frames, gaussians, pipe, background, metrics, out_dir, names, gt_depths=None, global_scale=1.0, depth_max=5.0, gif=True):
    """One PNG per frame in out_dir (<name>.png, heading "frame: <name>") and, with gif, output.gif of all panels in order, 100 ms per
    frame, looping.  metrics: eval_rendering's result for the same frames (the titles carry psnr[k] and depth_l1[k] to two decimals);
    every frame but the first gets its exposure, as there.  s = reduction_factor(W).  Encoding runs on the calling thread; the returned
    dict says what the device work, the copies and the encoding cost (seconds, host clock around synchronised sections)."""
    from PIL import Image
    from splat_slam_amd.eval import _device_depth
    from splat_slam_amd.renderer import render
    n = len(frames)
    if n == 0:
        raise ValueError("plot_rendering: no frames")
    if len(names) != n or len(metrics["psnr"]) != n or (gt_depths is not None and len(gt_depths) != n):
        raise ValueError(f"plot_rendering: {n} frames need as many names, metrics and ground-truth depths")
    dev = frames[0].original_image.device
    if dev.type != "cuda":
        raise RuntimeError("plot_rendering needs GPU tensors (HIP only, no CPU fallback)")
    os.makedirs(out_dir, exist_ok=True)
    H, W = frames[0].original_image.shape[-2:]
    s = reduction_factor(W)
    cost = {"compose_s": 0.0, "copy_s": 0.0, "encode_s": 0.0, "gif_s": 0.0}
    files, reel = [], []
    for c0 in range(0, n, CHUNK):
        ks = range(c0, min(n, c0 + CHUNK))
        t0 = time.perf_counter()
        pk = [render(frames[k], gaussians, pipe, background) for k in ks]
        panels = compose_panels(
            [p["render"] for p in pk], [frames[k].original_image for k in ks], [p["depth"] for p in pk],
            [_device_depth(frames[k].depth if gt_depths is None else gt_depths[k], dev) for k in ks],
            ["frame: " + names[k] for k in ks], [frame_titles(metrics["psnr"][k], metrics["depth_l1"][k]) for k in ks], s=s,
            exposures=[(frames[k].exposure_a, frames[k].exposure_b) if k > 0 else None for k in ks], global_scale=global_scale,
            depth_max=depth_max)
        torch.cuda.synchronize(dev)
        t1 = time.perf_counter()
        host = panels.cpu().numpy()                 # the chunk's one copy to the host
        t2 = time.perf_counter()
        for i, k in enumerate(ks):
            img = Image.fromarray(host[i])
            path = os.path.join(out_dir, names[k] + ".png")
            img.save(path)
            files.append(path)
            if gif:
                reel.append(img.quantize(256))
        cost["compose_s"] += t1 - t0
        cost["copy_s"] += t2 - t1
        cost["encode_s"] += time.perf_counter() - t2
    out = {"files": files, "gif": None, "s": s, "panel_size": panel_size(H, W, s)}
    if gif:
        t0 = time.perf_counter()
        out["gif"] = os.path.join(out_dir, "output.gif")
        reel[0].save(out["gif"], save_all=True, append_images=reel[1:], duration=100, loop=0)
        cost["gif_s"] = time.perf_counter() - t0
    out.update(cost)
    return out


# ---- the trajectory plot
TRAJ_SIZE = (800, 640)                  # width, height
TRAJ_AREA = (60, 50, 640, 580)          # the plot area: left, top, right, bottom
TRAJ_BAR = (690, 162, 710, 418)         # the colour bar: 256 rows, the maximum on top
TRAJ_GRAY = (128, 128, 128)
_DASH_ON, _DASH_OFF = 6, 4


@functools.lru_cache(maxsize=None)
def jet_table():
    """the 256 x 3 uint8 jet table of the composer, read from csrc/sgr_plot_tables.h (what scripts/gen_plot_tables.py wrote)"""
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "csrc", "sgr_plot_tables.h")) as f:
        text = f.read()
    body = text[text.index("kJet[256][3]"):]
    body = body[body.index("{") + 1:body.index("};")]
    return np.array([int(v) for v in re.findall(r"\d+", body)], dtype=np.uint8).reshape(256, 3)


def _host(x):
    return np.asarray(x.detach().cpu() if torch.is_tensor(x) else x)


def trajectory_projection(points):
    """points [m,2] -> (scale, to_pixel): one scale for both axes, the larger extent with a 5 % margin on either side filling the plot
    area's smaller side, the bounding box centred, y up; an extent of 0 (or no point) falls back to scale 1"""
    x0, y0, x1, y1 = TRAJ_AREA
    lo, hi = (points.min(0), points.max(0)) if len(points) else (np.zeros(2), np.zeros(2))
    extent = float((hi - lo).max())
    scale = min(x1 - x0, y1 - y0) / (1.1 * extent) if extent > 0 else 1.0
    mid = 0.5 * (lo + hi)

    def to_pixel(p):
        return (int(round(0.5 * (x0 + x1) + (p[0] - mid[0]) * scale)), int(round(0.5 * (y0 + y1) - (p[1] - mid[1]) * scale)))
    return scale, to_pixel


def segment_colors(err):
    """jet entries of the segments between consecutive vertices: the mean error of a segment's two ends between the minimum and the maximum
    vertex error, idx = clamp(floor(256 t), 0, 255); a single vertex gets its own"""
    err = np.asarray(err, dtype=np.float64)
    lo, hi = (float(err.min()), float(err.max())) if len(err) else (0.0, 0.0)
    e = 0.5 * (err[:-1] + err[1:]) if len(err) > 1 else err
    t = (e - lo) / (hi - lo) if hi > lo else np.zeros_like(e)
    return np.clip(np.floor(256.0 * t), 0, 255).astype(np.int64), lo, hi


def _dashed(draw, p, q, fill):
    length = float(np.hypot(q[0] - p[0], q[1] - p[1]))
    at = 0.0
    while at < length or at == 0.0:
        end = min(at + _DASH_ON, length)
        a = (p[0] + (q[0] - p[0]) * at / max(length, 1e-12), p[1] + (q[1] - p[1]) * at / max(length, 1e-12))
        b = (p[0] + (q[0] - p[0]) * end / max(length, 1e-12), p[1] + (q[1] - p[1]) * end / max(length, 1e-12))
        draw.line([a, b], fill=fill, width=1)
        at += _DASH_ON + _DASH_OFF
    draw.point([p, q], fill=fill)


def plot_trajectory(alignment, path, title):
    """The reference's xy plot: the reference positions as a gray dashed polyline, then the aligned estimate's segments coloured by their
    APE through the jet table between the minimum and the maximum error, a colour bar with the two as text.  Positions, validity and
    errors come from alignment.pairs (pairs.errors(r_a, t_a, s)); skipped pairs are left out.  Writes a PNG of TRAJ_SIZE."""
    from PIL import Image, ImageDraw
    pairs = alignment.pairs
    if pairs is None:
        raise ValueError("plot_trajectory: the alignment carries no pairs (use traj_eval.align)")
    pos = _host(pairs.pos).astype(np.float64).reshape(-1, 2, 3)
    valid = _host(pairs.valid).astype(bool).reshape(-1)
    err = _host(pairs.errors(alignment.r_a, alignment.t_a, alignment.s)[0]).astype(np.float64).reshape(-1)[valid]
    est = alignment.s * (pos[valid, 0] @ np.asarray(alignment.r_a, dtype=np.float64).T) + np.asarray(alignment.t_a, dtype=np.float64)
    ref = pos[valid, 1]
    _, to_pixel = trajectory_projection(np.concatenate([ref[:, :2], est[:, :2]]))
    jet = jet_table()
    img = Image.new("RGB", TRAJ_SIZE, (255, 255, 255))
    draw = ImageDraw.Draw(img)
    x0, y0, x1, y1 = TRAJ_AREA
    draw.rectangle([x0, y0, x1, y1], outline=(0, 0, 0))
    draw.text((x0, 20), str(title), fill=(0, 0, 0))
    draw.text((0.5 * (x0 + x1) - 15, y1 + 12), "x (m)", fill=(0, 0, 0))
    draw.text((10, 0.5 * (y0 + y1)), "y (m)", fill=(0, 0, 0))
    rp = [to_pixel(p) for p in ref]
    for p, q in zip(rp[:-1], rp[1:]):
        _dashed(draw, p, q, TRAJ_GRAY)
    if rp:
        draw.point(rp, fill=TRAJ_GRAY)
    ep = [to_pixel(p) for p in est]
    idx, lo, hi = segment_colors(err)
    if len(ep) == 1:
        draw.ellipse([ep[0][0] - 1, ep[0][1] - 1, ep[0][0] + 1, ep[0][1] + 1], fill=tuple(int(v) for v in jet[idx[0]]))
    for k, (p, q) in enumerate(zip(ep[:-1], ep[1:])):
        c = tuple(int(v) for v in jet[idx[k]])
        draw.line([p, q], fill=c, width=3)
        for v in (p, q):
            draw.ellipse([v[0] - 1, v[1] - 1, v[0] + 1, v[1] + 1], fill=c)
    bx0, by0, bx1, by1 = TRAJ_BAR
    for r in range(256):
        draw.line([(bx0, by0 + r), (bx1, by0 + r)], fill=tuple(int(v) for v in jet[255 - r]))
    draw.text((bx1 + 6, by0 - 5), f"{hi:.4f}", fill=(0, 0, 0))
    draw.text((bx1 + 6, by1 - 5), f"{lo:.4f}", fill=(0, 0, 0))
    draw.text((bx0 - 10, by0 - 24), "APE (m)", fill=(0, 0, 0))
    os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
    img.save(path)
    return TRAJ_SIZE
