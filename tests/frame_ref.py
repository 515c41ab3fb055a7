"""The oracle of the frame preparation (include/splat_hip.h, sgr_frame_prepare; DESIGN.md section 3, "Datasets and frame preparation"):
its equations restated per pixel in plain Python integers -- loops, nothing vectorised, nothing shared with splat_slam_amd.datasets --
plus the cases and the tiny on-disk sequences that tests/test_datasets_cpu.py and tests/test_gpu_datasets.py share."""
import math
import os

import numpy as np

TUM_DISTORTION = [0.2624, -0.9531, -0.0054, 0.0026, 1.1633]       # configs/TUM_RGBD/freiburg1_desk.yaml


# ---- the oracle -------------------------------------------------------------------------------------------------------------------------
def ref_map(H, W, fx, fy, cx, cy, distortion):
    k1, k2, p1, p2 = (float(v) for v in distortion[:4])
    k3 = float(distortion[4]) if len(distortion) > 4 else 0.0
    out = np.zeros((H, W, 2), dtype=np.int32)
    for v in range(H):
        for u in range(W):
            x = (float(u) - cx) / fx
            y = (float(v) - cy) / fy
            r2 = x * x + y * y
            kr = 1.0 + k1 * r2 + k2 * (r2 * r2) + k3 * (r2 * r2 * r2)
            xd = x * kr + 2.0 * p1 * x * y + p2 * (r2 + 2.0 * x * x)
            yd = y * kr + p1 * (r2 + 2.0 * y * y) + 2.0 * p2 * x * y
            qx = float(np.rint(np.float64(32.0 * (fx * xd + cx))))
            qy = float(np.rint(np.float64(32.0 * (fy * yd + cy))))
            out[v, u, 0] = int(min(max(qx, -float(1 << 20)), float(1 << 20)))
            out[v, u, 1] = int(min(max(qy, -float(1 << 20)), float(1 << 20)))
    return out


def ref_tap(j, S, D):
    n, d = (2 * j + 1) * S - D, 2 * D
    s = n // d                                      # Python's // is floor
    b = (4096 * (n - s * d) + d) // (2 * d)
    if s < 0:
        s, b = 0, 0
    if s >= S - 1:
        s, b = S - 1, 0
    return s, min(s + 1, S - 1), b


def ref_undistorted(img, map_q, v, u, c):
    """(U, whether every tap lay inside the image)"""
    if map_q is None:
        return int(img[v, u, c]), True
    H, W = img.shape[:2]
    qx, qy = int(map_q[v, u, 0]), int(map_q[v, u, 1])
    ix, ax, iy, ay = qx >> 5, qx & 31, qy >> 5, qy & 31       # Python's >> is arithmetic
    acc, inside = 0, True
    for yy, xx, w in ((iy, ix, (32 - ax) * (32 - ay)), (iy, ix + 1, ax * (32 - ay)), (iy + 1, ix, (32 - ax) * ay), (iy + 1, ix + 1, ax * ay)):
        if 0 <= yy < H and 0 <= xx < W:
            acc += w * int(img[yy, xx, c])
        else:
            inside = False
    return (acc + 512) >> 10, inside


def ref_color(img, map_q, H_oe, W_oe, H_edge, W_edge):
    """img [H,W,>=3] uint8 -> (color [3,H_out,W_out] fp32, inside [H_out,W_out] bool: all 16 taps of the pixel lay inside the image)"""
    H, W = img.shape[:2]
    H_out, W_out = H_oe - 2 * H_edge, W_oe - 2 * W_edge
    out = np.zeros((3, H_out, W_out), dtype=np.float32)
    inside = np.ones((H_out, W_out), dtype=bool)
    for y in range(H_out):
        v0, v1, by = ref_tap(y + H_edge, H, H_oe)
        for x in range(W_out):
            u0, u1, bx = ref_tap(x + W_edge, W, W_oe)
            for c in range(3):
                acc = 0
                for v, wy in ((v0, 2048 - by), (v1, by)):
                    for u, wx in ((u0, 2048 - bx), (u1, bx)):
                        level, ok = ref_undistorted(img, map_q, v, u, c)
                        acc += wy * wx * level
                        inside[y, x] &= ok
                assert acc + (1 << 21) < (1 << 32)
                out[c, y, x] = np.float32((acc + (1 << 21)) >> 22) / np.float32(255.0)
    return out, inside


# ---- the colour cases of the issue: name -> (H, W, H_oe, W_oe, H_edge, W_edge, distortion scale or None) ------------------------------------
COLOR_CASES = {
    "down": (17, 23, 13, 17, 1, 2, None),                 # 17 x 23 -> 11 x 13 with edges (1, 2)
    "down_map": (17, 23, 13, 17, 1, 2, 8.0),              # ... with the TUM distortion x 8: samples outside, negative map coordinates
    "identity": (9, 9, 9, 9, 0, 0, None),
    "up": (7, 5, 15, 12, 0, 0, None),                     # both border clamps
    "half": (16, 64, 8, 32, 0, 0, None),                  # exactly 2 : 1
}
DEPTH_CASES = {"down": (17, 23, 13, 17, 1, 2), "tum": (480, 640, 400, 528, 0, 0), "up": (7, 5, 15, 12, 0, 0)}
DEPTH_SCALES = (5000.0, 6553.5)
_CACHE = {}


def case_map(name):
    H, W, _, _, _, _, k = COLOR_CASES[name]
    if k is None:
        return None
    key = ("map", name)
    if key not in _CACHE:
        # a camera of the case's own size: focal length about the width, the principal point off the centre
        _CACHE[key] = ref_map(H, W, 0.9 * W, 0.85 * W, 0.48 * W, 0.53 * H, [k * v for v in TUM_DISTORTION])
    return _CACHE[key]


def case_map_args(name):
    H, W, _, _, _, _, k = COLOR_CASES[name]
    return (H, W, 0.9 * W, 0.85 * W, 0.48 * W, 0.53 * H, [k * v for v in TUM_DISTORTION])


def case_images(name):
    """[2,H,W,4] uint8: a seeded random image and a constant 255 one (the fourth byte is random: it must not matter)"""
    H, W = COLOR_CASES[name][:2]
    key = ("img", name)
    if key not in _CACHE:
        rng = np.random.default_rng(sum(map(ord, name)))
        img = rng.integers(0, 256, (2, H, W, 4), dtype=np.uint8)
        img[1, :, :, :3] = 255
        _CACHE[key] = img
    return _CACHE[key]


def case_reference(name):
    """(color [2,3,H_out,W_out] fp32, inside [H_out,W_out]) of the oracle, computed once"""
    key = ("ref", name)
    if key not in _CACHE:
        _, _, H_oe, W_oe, H_edge, W_edge, _ = COLOR_CASES[name]
        res = [ref_color(img, case_map(name), H_oe, W_oe, H_edge, W_edge) for img in case_images(name)]
        _CACHE[key] = (np.stack([r[0] for r in res]), res[0][1])
    return _CACHE[key]


def case_depth(name):
    H, W = DEPTH_CASES[name][:2]
    key = ("depth", name)
    if key not in _CACHE:
        d = np.random.default_rng(7 + H).integers(0, 65536, (1, H, W), dtype=np.uint16)
        d[0, 0, 0], d[0, -1, -1], d[0, 0, -1], d[0, -1, 0] = 0, 65535, 65535, 0
        _CACHE[key] = d
    return _CACHE[key]


def torch_depth(depth_u16, H_oe, W_oe, H_edge, W_edge, scale):
    """the reference's depth path: astype(float32) / scale, F.interpolate(nearest) on the CPU, the crop"""
    import torch
    import torch.nn.functional as F
    full = torch.from_numpy(depth_u16.astype(np.float32) / scale).float()
    out = F.interpolate(full[:, None], (H_oe, W_oe), mode="nearest")[:, 0]
    return out[:, H_edge:H_oe - H_edge, W_edge:W_oe - W_edge].contiguous().numpy()


# ---- tiny sequences on disk -----------------------------------------------------------------------------------------------------------------
SEQ_H, SEQ_W, SEQ_N = 24, 32, 12


def seq_cfg(dataset, root, folder, distortion=None, **over):
    cam = {"H": SEQ_H, "W": SEQ_W, "fx": 30.0, "fy": 29.0, "cx": 15.3, "cy": 12.1, "png_depth_scale": 5000.0,
           "H_out": 16, "W_out": 20, "H_edge": 2, "W_edge": 2}
    if distortion is not None:
        cam["distortion"] = list(distortion)
    cfg = {"dataset": dataset, "stride": 1, "max_frames": -1, "cam": cam, "data": {"dataset_root": str(root), "input_folder": folder}}
    cfg.update(over)
    return cfg


def seq_frame(k):
    """(rgb [H,W,3] uint8 smooth enough for JPEG, depth [H,W] uint16) of frame k"""
    yy, xx = np.mgrid[0:SEQ_H, 0:SEQ_W]
    rgb = np.stack([(8 * xx + 5 * k) % 256, (9 * yy + 11 * k) % 256, (3 * xx + 4 * yy + 17 * k) % 256], -1).astype(np.uint8)
    depth = ((1000 * k + 37 * yy + 91 * xx) % 65536).astype(np.uint16)
    depth[0, 0], depth[-1, -1] = 0, 65535
    return rgb, depth


def seq_pose(k):
    c, s = math.cos(0.1 * k), math.sin(0.1 * k)
    return np.array([[c, 0.0, s, 0.1 * k], [0.0, 1.0, 0.0, -0.05 * k], [-s, 0.0, c, 0.02 * k * k], [0.0, 0.0, 0.0, 1.0]])


def _save(rgb, depth, color_path, depth_path):
    from PIL import Image
    Image.fromarray(rgb).save(color_path, quality=95)
    Image.fromarray(depth).save(depth_path)


def write_replica(root, folder="room"):
    d = os.path.join(str(root), folder, "results")
    os.makedirs(d)
    with open(os.path.join(str(root), folder, "traj.txt"), "w") as f:
        for k in range(SEQ_N):
            _save(*seq_frame(k), os.path.join(d, f"frame{k:06d}.jpg"), os.path.join(d, f"depth{k:06d}.png"))
            f.write(" ".join(repr(float(v)) for v in seq_pose(k).reshape(-1)) + "\n")
        f.write(" ".join(["9.0"] * 16) + "\n")          # a line more than there are images: n_img lines are read
    return seq_cfg("replica", root, folder)


def write_scannet(root, folder="scene"):
    base = os.path.join(str(root), folder)
    for sub in ("color", "depth", "pose"):
        os.makedirs(os.path.join(base, sub))
    for k in range(SEQ_N):
        _save(*seq_frame(k), os.path.join(base, "color", f"{k}.jpg"), os.path.join(base, "depth", f"{k}.png"))
        with open(os.path.join(base, "pose", f"{k}.txt"), "w") as f:
            for row in seq_pose(k):
                f.write(" ".join(repr(float(v)) for v in row) + "\n")
    return seq_cfg("scannet", root, folder)


# colour timestamps: jittered 10 Hz; frame 4 has no depth within 0.08 s (its depth frame is missing and the neighbours are 0.1 s away);
# frame 8 follows frame 7 by 0.02 s < 1/32 s
TUM_T_COLOR = [10.000, 10.103, 10.198, 10.305, 10.400, 10.497, 10.602, 10.700, 10.720, 10.801, 10.905, 11.000]
TUM_T_DEPTH = [10.010, 10.110, 10.190, 10.300, 10.500, 10.610, 10.690, 10.730, 10.810, 10.900, 11.010]      # none near 10.400
TUM_KEPT = [0, 1, 2, 3, 5, 6, 7, 9, 10, 11]           # by hand: 4 has no depth; 8 is 0.02 s after 7
TUM_DEPTH_OF = {0: 0, 1: 1, 2: 2, 3: 3, 5: 4, 6: 5, 7: 6, 9: 8, 10: 9, 11: 10}     # nearest depth stamp of each kept colour frame


def tum_quaternion(k):
    """(x, y, z, w), deliberately not of unit length"""
    q = np.array([0.1 * k - 0.3, 0.2, -0.05 * k, 1.0])
    return q * (1.0 + 0.1 * k)


def tum_translation(k):
    return np.array([0.1 * k, -0.2 + 0.03 * k, 0.01 * k * k])


def write_tum(root, folder="desk", distortion=TUM_DISTORTION):
    base = os.path.join(str(root), folder)
    os.makedirs(os.path.join(base, "rgb"))
    os.makedirs(os.path.join(base, "depth"))
    with open(os.path.join(base, "rgb.txt"), "w") as f:
        f.write("# color images\n# file: 'test'\n# timestamp filename\n")
        for k, t in enumerate(TUM_T_COLOR):
            f.write(f"{t:.6f} rgb/{t:.6f}.jpg\n")
    with open(os.path.join(base, "depth.txt"), "w") as f:
        f.write("# depth maps\n# file: 'test'\n# timestamp filename\n")
        for t in TUM_T_DEPTH:
            f.write(f"{t:.6f} depth/{t:.6f}.png\n")
    for k, t in enumerate(TUM_T_COLOR):
        from PIL import Image
        Image.fromarray(seq_frame(k)[0]).save(os.path.join(base, "rgb", f"{t:.6f}.jpg"), quality=95)
    for m, t in enumerate(TUM_T_DEPTH):
        from PIL import Image
        Image.fromarray(seq_frame(100 + m)[1]).save(os.path.join(base, "depth", f"{t:.6f}.png"))
    with open(os.path.join(base, "groundtruth.txt"), "w") as f:
        f.write("# ground truth trajectory\n# file: 'test'\n# timestamp tx ty tz qx qy qz qw\n")
        for k, t in enumerate(TUM_T_COLOR):             # one pose 3 ms after every colour frame
            f.write(f"{t + 0.003:.6f} " + " ".join(repr(float(v)) for v in np.concatenate([tum_translation(k), tum_quaternion(k)])) + "\n")
    return seq_cfg("tumrgbd", root, folder, distortion=distortion)
