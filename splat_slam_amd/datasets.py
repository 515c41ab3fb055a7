"""Dataset streams of the reference (src/utils/datasets.py: Replica, ScanNet, TUM RGB-D) with the per-frame work -- undistortion, resize,
crop, normalisation -- on the device, in one launch of csrc/sgr_frame.hip.  Stated in DESIGN.md section 3, "Datasets and frame
preparation".

    get_dataset(cfg, device="cuda:0", prepare="hip", prefetch=1) -> dataset_dict[cfg["dataset"]](cfg, ...)
        cfg: the reference's dict (splat_slam_amd.config.load_config): cfg["dataset"], ["stride"], ["max_frames"], cfg["cam"] (H, W, fx,
        fy, cx, cy, H_out, W_out, H_edge, W_edge, png_depth_scale, optional distortion [k1, k2, p1, p2(, k3)]) and cfg["data"]
        (dataset_root, input_folder).
    len(stream); stream[i] -> (i, color [1,3,H_out,W_out] fp32 in [0,1] RGB, depth [H_out,W_out] fp32 or None, pose [4,4] fp32 camera ->
        world (CPU) or None); stream.get_color(i) -> the colour alone; stream.get_intrinsic() -> [4] fp32 (fx, fy, cx, cy) of the output
        image; stream.poses: list of fp64 4x4; stream.close().  This is what Tracker.run, Slam, full_traj_eval and
        DepthVideo.eval_depth_l1 read.  Attributes carry the reference's names (H, W, fx, fy, cx, cy: of the OUTPUT image; fx_orig ...:
        of the files; H_out, W_out, H_edge, W_edge, H_out_with_edge, W_out_with_edge, fovx, fovy, distortion, png_depth_scale,
        input_folder, color_paths, depth_paths, n_img, w2c_first_pose).

    prepare="hip": the frame goes to the device as bytes (RGBX u8, u16 depth) and sgr_frame_prepare writes the fp32 outputs; needs a GPU
        device.  prepare="host": the same integer arithmetic in numpy (frame_prepare_host), then one copy; works with device="cpu".  Both
        give the same bits.
    prefetch=k > 0: one daemon thread decodes up to k frames ahead of the last index asked for into a ring of k + 1 (pinned, on a GPU
        device) host buffers; it makes no GPU call.  The calling thread copies to the device and launches, records an event per buffer
        after the copy and waits for it before the buffer is handed out again.  Any index may be asked for at any time (what is not in
        the ring is decoded on demand).  prefetch=0: no thread.  One consumer thread per stream.

    frame_prepare(color_u8, depth_u16, map_q, H_oe, W_oe, H_edge, W_edge, depth_scale) -> (color, depth): device tensors, n frames, one launch
    frame_prepare_host(...)                                                             -> the same on numpy arrays
    undistortion_map(H, W, fx, fy, cx, cy, distortion) -> [H,W,2] int32 (numpy), resize_taps(S, D) -> (s0, s1, b)

Decoding is Pillow's (Image.open(path).convert("RGB"), 16-bit PNG depth as uint16): its JPEG decoder is not guaranteed to give the bytes
OpenCV's gives.  EXR depth is not supported: a depth path that is no .png, or that Pillow cannot read as one, raises TypeError as the
reference's depthloader does for an unknown extension.
"""
import collections
import glob
import math
import os
import threading

import numpy as np
import torch
from PIL import Image

from splat_slam_amd.camera import focal2fov

__all__ = ["BaseDataset", "Replica", "ScanNet", "TUM_RGBD", "dataset_dict", "get_dataset", "frame_prepare", "frame_prepare_host",
           "undistortion_map", "resize_taps"]

MAP_SHIFT = 5                   # map coordinates are in 1/32 pixel
MAP_LIMIT = 1 << 20
MAX_SIDE = 16384


def undistortion_map(H, W, fx, fy, cx, cy, distortion):
    """(qx, qy) [H,W,2] int32: where pixel (u, v) of the undistorted image lies in the file's image, in 1/32 pixel (numpy fp64, rint)"""
    d = [float(v) for v in np.asarray(distortion, dtype=np.float64).reshape(-1)]
    if len(d) not in (4, 5):
        raise ValueError(f"distortion has {len(d)} entries: [k1, k2, p1, p2] or [k1, k2, p1, p2, k3]")
    k1, k2, p1, p2 = d[:4]
    k3 = d[4] if len(d) == 5 else 0.0
    fx, fy, cx, cy = float(fx), float(fy), float(cx), float(cy)
    u = np.arange(W, dtype=np.float64)[None, :]
    v = np.arange(H, dtype=np.float64)[:, None]
    x = np.broadcast_to((u - cx) / fx, (H, W))
    y = np.broadcast_to((v - cy) / fy, (H, W))
    r2 = x * x + y * y
    kr = 1.0 + k1 * r2 + k2 * (r2 * r2) + k3 * (r2 * r2 * r2)
    xd = x * kr + 2.0 * p1 * x * y + p2 * (r2 + 2.0 * x * x)
    yd = y * kr + p1 * (r2 + 2.0 * y * y) + 2.0 * p2 * x * y
    qx = np.clip(np.rint(32.0 * (fx * xd + cx)), -MAP_LIMIT, MAP_LIMIT)
    qy = np.clip(np.rint(32.0 * (fy * yd + cy)), -MAP_LIMIT, MAP_LIMIT)
    return np.ascontiguousarray(np.stack([qx, qy], axis=-1).astype(np.int32))


def resize_taps(S, D):
    """per output index of a D-sized axis over an S-sized one: first tap, second tap, weight b of the second in 1/2048 (int64 [D] each)"""
    j = np.arange(D, dtype=np.int64)
    n, d = (2 * j + 1) * S - D, 2 * D
    s = n // d
    b = (4096 * (n - s * d) + d) // (2 * d)
    low, high = s < 0, s >= S - 1
    s = np.where(low, 0, np.where(high, S - 1, s))
    b = np.where(low | high, 0, b)
    return s, np.minimum(s + 1, S - 1), b


def _check_sizes(n, H, W, ps, H_oe, W_oe, H_edge, W_edge):
    if n < 1 or ps not in (3, 4):
        raise ValueError(f"colour must be [n >= 1, H, W, 3 or 4] uint8 (n={n}, last={ps})")
    if not (1 <= H <= MAX_SIDE and 1 <= W <= MAX_SIDE and 1 <= H_oe <= MAX_SIDE and 1 <= W_oe <= MAX_SIDE):
        raise ValueError(f"sizes {H} x {W} -> {H_oe} x {W_oe} outside [1, {MAX_SIDE}]")
    if H_edge < 0 or W_edge < 0 or 2 * H_edge >= H_oe or 2 * W_edge >= W_oe:
        raise ValueError(f"edges ({H_edge}, {W_edge}) leave nothing of {H_oe} x {W_oe}")


def _undistorted_host(img, map_q, rows, cols):
    """U [n, len(rows), len(cols), 3] int64 at the source pixels rows x cols"""
    H, W = img.shape[1:3]
    if map_q is None:
        return img[:, rows[:, None], cols[None, :], :3].astype(np.int64)
    q = map_q[rows[:, None], cols[None, :]].astype(np.int64)
    ix, iy = q[..., 0] >> MAP_SHIFT, q[..., 1] >> MAP_SHIFT
    ax, ay = q[..., 0] & 31, q[..., 1] & 31
    acc = np.zeros((img.shape[0],) + ix.shape + (3,), dtype=np.int64)
    for dy, wy in ((0, 32 - ay), (1, ay)):
        for dx, wx in ((0, 32 - ax), (1, ax)):
            yy, xx = iy + dy, ix + dx
            inside = (yy >= 0) & (yy < H) & (xx >= 0) & (xx < W)
            p = img[:, np.clip(yy, 0, H - 1), np.clip(xx, 0, W - 1), :3].astype(np.int64)
            acc += ((wy * wx) * inside)[None, :, :, None] * p
    return (acc + 512) >> 10


def frame_prepare_host(color_u8, depth_u16, map_q, H_oe, W_oe, H_edge, W_edge, depth_scale=1.0):
    """sgr_frame_prepare's arithmetic in numpy.  color_u8 [n,H,W,3|4] uint8, depth_u16 [n,H,W] uint16 or None, map_q [H,W,2] int32 or None
    -> (color [n,3,H_out,W_out] fp32, depth [n,H_out,W_out] fp32 or None)"""
    color_u8 = np.asarray(color_u8)
    if color_u8.dtype != np.uint8 or color_u8.ndim != 4:
        raise ValueError("colour must be [n, H, W, 3 or 4] uint8")
    n, H, W, ps = color_u8.shape
    _check_sizes(n, H, W, ps, H_oe, W_oe, H_edge, W_edge)
    if map_q is not None and (map_q.shape != (H, W, 2) or map_q.dtype != np.int32):
        raise ValueError("map_q must be [H, W, 2] int32")
    H_out, W_out = H_oe - 2 * H_edge, W_oe - 2 * W_edge
    ys0, ys1, by = (t[H_edge:H_edge + H_out] for t in resize_taps(H, H_oe))
    xs0, xs1, bx = (t[W_edge:W_edge + W_out] for t in resize_taps(W, W_oe))
    acc = np.zeros((n, H_out, W_out, 3), dtype=np.int64)
    for rows, wy in ((ys0, 2048 - by), (ys1, by)):
        for cols, wx in ((xs0, 2048 - bx), (xs1, bx)):
            acc += (wy[:, None] * wx[None, :])[None, :, :, None] * _undistorted_host(color_u8, map_q, rows, cols)
    level = ((acc + (1 << 21)) >> 22).astype(np.float32)
    color = np.ascontiguousarray(np.transpose(level / np.float32(255.0), (0, 3, 1, 2)))
    if depth_u16 is None:
        return color, None
    depth_u16 = np.asarray(depth_u16)
    if depth_u16.dtype != np.uint16 or depth_u16.shape != (n, H, W):
        raise ValueError("depth must be [n, H, W] uint16")
    if not (depth_scale > 0 and math.isfinite(depth_scale)):
        raise ValueError("depth_scale must be positive and finite")
    sh, sw = np.float32(H) / np.float32(H_oe), np.float32(W) / np.float32(W_oe)
    sy = np.minimum(np.floor((np.arange(H_out) + H_edge).astype(np.float32) * sh).astype(np.int64), H - 1)
    sx = np.minimum(np.floor((np.arange(W_out) + W_edge).astype(np.float32) * sw).astype(np.int64), W - 1)
    depth = depth_u16[:, sy[:, None], sx[None, :]].astype(np.float32) / np.float32(depth_scale)
    return color, np.ascontiguousarray(depth)


def frame_prepare(color_u8, depth_u16, map_q, H_oe, W_oe, H_edge, W_edge, depth_scale=1.0):
    """One sgr_frame_prepare launch on the current stream.  color_u8 [n,H,W,3|4] torch.uint8, depth_u16 [n,H,W] torch.int16 or uint16
    (the bits of the uint16 values) or None, map_q [H,W,2] torch.int32 or None, all contiguous on one GPU
    -> (color [n,3,H_out,W_out] fp32, depth [n,H_out,W_out] fp32 or None)"""
    from splat_slam_amd import _native as nat
    if not color_u8.is_cuda or color_u8.dtype != torch.uint8 or color_u8.dim() != 4 or not color_u8.is_contiguous():
        raise ValueError("colour must be a contiguous [n, H, W, 3 or 4] uint8 tensor on the GPU")
    n, H, W, ps = color_u8.shape
    _check_sizes(n, H, W, ps, H_oe, W_oe, H_edge, W_edge)
    dev = color_u8.device
    if depth_u16 is not None and (depth_u16.device != dev or depth_u16.element_size() != 2 or depth_u16.is_floating_point()
                                  or tuple(depth_u16.shape) != (n, H, W) or not depth_u16.is_contiguous()):
        raise ValueError("depth must be a contiguous [n, H, W] 16-bit integer tensor on the colour's device")
    if map_q is not None and (map_q.device != dev or map_q.dtype != torch.int32 or tuple(map_q.shape) != (H, W, 2)
                              or not map_q.is_contiguous()):
        raise ValueError("map_q must be a contiguous [H, W, 2] int32 tensor on the colour's device")
    H_out, W_out = H_oe - 2 * H_edge, W_oe - 2 * W_edge
    color = torch.empty((n, 3, H_out, W_out), dtype=torch.float32, device=dev)
    depth = torch.empty((n, H_out, W_out), dtype=torch.float32, device=dev) if depth_u16 is not None else None
    with torch.cuda.device(dev):
        nat.check(nat.lib().sgr_frame_prepare(n, color_u8.data_ptr(), ps, nat.ptr(depth_u16), H, W, nat.ptr(map_q), H_oe, W_oe, H_edge,
                                              W_edge, float(depth_scale), color.data_ptr(), nat.ptr(depth),
                                              torch.cuda.current_stream().cuda_stream), "sgr_frame_prepare")
    return color, depth


class _Slot:
    """one decoded frame on the host: RGBX bytes and the u16 depth (stored as int16 bits), pinned when the stream's device is a GPU"""
    IDLE, QUEUED, BUSY, READY = range(4)

    def __init__(self, H, W, with_depth, pinned):
        self.color = torch.zeros((1, H, W, 4), dtype=torch.uint8, pin_memory=pinned)
        self.depth = torch.zeros((1, H, W), dtype=torch.int16, pin_memory=pinned) if with_depth else None
        self.color_np = self.color.numpy()
        self.depth_np = self.depth.numpy().view(np.uint16) if with_depth else None
        self.index, self.state, self.error, self.event, self.in_flight = None, _Slot.IDLE, None, None, False

    def record_copy(self):
        """(calling thread) a copy out of this buffer was just enqueued on the current stream"""
        if self.event is None:
            self.event = torch.cuda.Event()
        self.event.record()
        self.in_flight = True

    def wait_copied(self):
        """(calling thread) the last copy out of this buffer has finished: it may be written again"""
        if self.in_flight:
            self.event.synchronize()
            self.in_flight = False


class _Ring:
    """k + 1 slots and one worker that decodes what the calling thread queued; the worker touches host memory only"""

    def __init__(self, decode, n_items, ahead, make_slot):
        self.decode, self.n_items, self.ahead = decode, n_items, ahead
        self.slots = [make_slot() for _ in range(ahead + 1)]
        self.cond = threading.Condition()
        self.queue = collections.deque()
        self.stop = False
        self.thread = threading.Thread(target=self._work, name="splat_slam_amd.datasets.prefetch", daemon=True)
        self.thread.start()

    def _work(self):
        while True:
            with self.cond:
                while not self.queue and not self.stop:
                    self.cond.wait()
                if self.stop:
                    return
                slot = self.queue.popleft()
                slot.state, index = _Slot.BUSY, slot.index
            error = None
            try:
                self.decode(index, slot)
            except BaseException as e:      # noqa: BLE001  (handed to the caller of get)
                error = e
            with self.cond:
                slot.error, slot.state = error, _Slot.READY
                self.cond.notify_all()

    def get(self, index):
        want = range(index, min(index + self.ahead + 1, self.n_items))
        with self.cond:
            if self.stop:
                raise RuntimeError("the stream is closed")
            while True:
                held = {s.index: s for s in self.slots if s.state != _Slot.IDLE}
                free = [s for s in self.slots if s.state != _Slot.BUSY and (s.state == _Slot.IDLE or s.index not in want)]
                for j in want:
                    if j in held or not free:
                        continue
                    slot = free.pop()
                    if slot.state == _Slot.QUEUED:
                        self.queue.remove(slot)
                    slot.wait_copied()
                    slot.index, slot.state, slot.error = j, _Slot.QUEUED, None
                    self.queue.append(slot)
                    held[j] = slot
                    self.cond.notify_all()
                if index in held:
                    break
                self.cond.wait()            # the only slot left is being decoded for an index nobody wants any more
            slot = held[index]
            while slot.state != _Slot.READY:
                self.cond.wait()
            if slot.error is not None:
                error, slot.state, slot.index = slot.error, _Slot.IDLE, None
                raise error
            return slot

    def close(self, join=True):
        with self.cond:
            self.stop = True
            self.cond.notify_all()
        if join:
            self.thread.join()


class BaseDataset:
    def __init__(self, cfg, device="cuda:0", prepare="hip", prefetch=1):
        if prepare not in ("hip", "host"):
            raise ValueError(f"prepare={prepare!r}: 'hip' or 'host'")
        self.name = cfg["dataset"]
        self.device = torch.device(device)
        self.prepare, self.prefetch = prepare, int(prefetch)
        if self.prefetch < 0:
            raise ValueError("prefetch must be >= 0")
        if prepare == "hip" and self.device.type != "cuda":
            raise ValueError("prepare='hip' runs on a GPU device; use prepare='host' with device='cpu'")
        cam = cfg["cam"]
        self.png_depth_scale = cam["png_depth_scale"]
        self.n_img = -1
        self.depth_paths, self.color_paths, self.poses, self.image_timestamps = None, None, None, None
        self.w2c_first_pose = None
        self.H, self.W = int(cam["H"]), int(cam["W"])
        self.fx_orig, self.fy_orig, self.cx_orig, self.cy_orig = cam["fx"], cam["fy"], cam["cx"], cam["cy"]
        self.H_out, self.W_out = int(cam["H_out"]), int(cam["W_out"])
        self.H_edge, self.W_edge = int(cam["H_edge"]), int(cam["W_edge"])
        self.H_out_with_edge, self.W_out_with_edge = self.H_out + self.H_edge * 2, self.W_out + self.W_edge * 2
        _check_sizes(1, self.H, self.W, 4, self.H_out_with_edge, self.W_out_with_edge, self.H_edge, self.W_edge)
        self.fx, self.fy, self.cx, self.cy = (float(v) for v in self.get_intrinsic().tolist())
        self.fovx = focal2fov(self.fx, self.W_out)
        self.fovy = focal2fov(self.fy, self.H_out)
        self.distortion = np.array(cam["distortion"]) if "distortion" in cam else None
        self.input_folder = os.path.join(cfg["data"]["dataset_root"], cfg["data"]["input_folder"])
        self._map_host = None if self.distortion is None else undistortion_map(
            self.H, self.W, self.fx_orig, self.fy_orig, self.cx_orig, self.cy_orig, self.distortion)
        self._map_dev = None
        self._ring, self._slot = None, None

    # ---- the stream's contract ---------------------------------------------------------------------------------------------------
    def __len__(self):
        return self.n_img

    def get_intrinsic(self):
        """(fx, fy, cx, cy) of the output image in the reference's fp32 tensor arithmetic: scale by out_with_edge / in, subtract the edge"""
        intrinsic = torch.as_tensor([self.fx_orig, self.fy_orig, self.cx_orig, self.cy_orig]).float()
        intrinsic[0] *= self.W_out_with_edge / self.W
        intrinsic[1] *= self.H_out_with_edge / self.H
        intrinsic[2] *= self.W_out_with_edge / self.W
        intrinsic[3] *= self.H_out_with_edge / self.H
        intrinsic[2] -= self.W_edge
        intrinsic[3] -= self.H_edge
        return intrinsic

    def get_color(self, index):
        return self._item(index, False)[0]

    def __getitem__(self, index):
        index = self._index(index)
        color, depth = self._item(index, True)
        pose = torch.from_numpy(np.asarray(self.poses[index])).float() if self.poses is not None else None
        return index, color, depth, pose

    def close(self):
        """stops the prefetch thread (joined) and drops the host buffers; the stream can still be read, without prefetch"""
        ring, self._ring = self._ring, None
        if ring is not None:
            ring.close()
            for slot in ring.slots:
                slot.wait_copied()
        self.prefetch = 0

    def __del__(self):
        ring = getattr(self, "_ring", None)
        if ring is not None:
            ring.close(join=False)      # (a daemon thread: never waited for from a finaliser, which may run at interpreter exit)

    # ---- decoding (host memory only: this is what the prefetch thread runs) ----------------------------------------------------------
    def _index(self, index):
        index = int(index)
        if index < 0:
            index += self.n_img
        if not 0 <= index < self.n_img:
            raise IndexError(f"frame {index} of {self.n_img}")
        return index

    def _read_depth(self, path):
        if ".png" not in path:
            raise TypeError(path)               # (.exr included: EXR depth is not supported)
        try:
            with Image.open(path) as im:
                depth = np.asarray(im)
        except (OSError, ValueError) as e:
            raise TypeError(f"{path}: {e}") from e
        if depth.ndim != 2 or depth.dtype.kind not in "iu" or depth.min() < 0 or depth.max() > 65535:
            raise TypeError(f"{path}: not a single-channel 16-bit depth image ({depth.dtype}, {depth.shape})")
        return depth.astype(np.uint16)

    def _decode(self, index, slot):
        with Image.open(self.color_paths[index]) as im:
            rgb = np.asarray(im.convert("RGB"))
        if rgb.shape != (self.H, self.W, 3):
            raise ValueError(f"{self.color_paths[index]} is {rgb.shape[0]} x {rgb.shape[1]}, the config says {self.H} x {self.W}")
        slot.color_np[0, :, :, :3] = rgb
        if slot.depth_np is not None:
            depth = self._read_depth(self.depth_paths[index])
            if depth.shape != (self.H, self.W):
                raise ValueError(f"{self.depth_paths[index]} is {depth.shape[0]} x {depth.shape[1]}, the config says {self.H} x {self.W}")
            slot.depth_np[0] = depth

    def _make_slot(self):
        return _Slot(self.H, self.W, self.depth_paths is not None, self.device.type == "cuda")

    def _fetch(self, index):
        if self.prefetch > 0:
            if self._ring is None:
                self._ring = _Ring(self._decode, self.n_img, self.prefetch, self._make_slot)
            return self._ring.get(index)
        if self._slot is None:
            self._slot = self._make_slot()
        slot = self._slot
        if slot.index != index:
            slot.wait_copied()
            slot.index = None
            self._decode(index, slot)
            slot.index = index
        return slot

    # ---- preparation (calling thread) ----------------------------------------------------------------------------------------------
    def _item(self, index, with_depth):
        slot = self._fetch(self._index(index))
        with_depth = with_depth and slot.depth is not None
        args = (self.H_out_with_edge, self.W_out_with_edge, self.H_edge, self.W_edge, float(self.png_depth_scale))
        if self.prepare == "host":
            color, depth = frame_prepare_host(slot.color_np, slot.depth_np if with_depth else None, self._map_host, *args)
            color = torch.from_numpy(color).to(self.device)
            return color, (torch.from_numpy(depth[0]).to(self.device) if with_depth else None)
        with torch.cuda.device(self.device):
            if self._map_host is not None and self._map_dev is None:
                self._map_dev = torch.from_numpy(self._map_host).to(self.device)
            color_u8 = slot.color.to(self.device, non_blocking=True)
            depth_u16 = slot.depth.to(self.device, non_blocking=True) if with_depth else None
            slot.record_copy()
            color, depth = frame_prepare(color_u8, depth_u16, self._map_dev, *args)
        return color, (depth[0] if with_depth else None)


def _cut(items, stride, max_frames):
    return items[:int(1e5) if max_frames < 0 else max_frames][::stride]


class Replica(BaseDataset):
    """<input_folder>/results/frame*.jpg, depth*.png and traj.txt (one camera -> world matrix of 16 numbers a line)"""

    def __init__(self, cfg, device="cuda:0", prepare="hip", prefetch=1):
        super().__init__(cfg, device, prepare, prefetch)
        stride, max_frames = cfg["stride"], cfg["max_frames"]
        color_paths = sorted(glob.glob(f"{self.input_folder}/results/frame*.jpg"))
        depth_paths = sorted(glob.glob(f"{self.input_folder}/results/depth*.png"))
        self.n_img = len(color_paths)
        self.load_poses(f"{self.input_folder}/traj.txt")
        self.color_paths = _cut(color_paths, stride, max_frames)
        self.depth_paths = _cut(depth_paths, stride, max_frames)
        self.poses = _cut(self.poses, stride, max_frames)
        self.w2c_first_pose = np.linalg.inv(self.poses[0])
        self.n_img = len(self.color_paths)

    def load_poses(self, path):
        with open(path, "r") as f:
            lines = f.readlines()
        self.poses = [np.array([float(v) for v in lines[i].split()], dtype=np.float64).reshape(4, 4) for i in range(self.n_img)]


def _by_number(paths):
    return sorted(paths, key=lambda p: int(os.path.splitext(os.path.basename(p))[0]))


class ScanNet(BaseDataset):
    """<input_folder>/color/<k>.jpg, depth/<k>.png, pose/<k>.txt (4 lines of 4 numbers), each list in the order of the integer k.  As in
    the reference, paths and poses are cut and strided as separately built lists."""

    def __init__(self, cfg, device="cuda:0", prepare="hip", prefetch=1):
        super().__init__(cfg, device, prepare, prefetch)
        stride, max_frames = cfg["stride"], cfg["max_frames"]
        self.color_paths = _cut(_by_number(glob.glob(os.path.join(self.input_folder, "color", "*.jpg"))), stride, max_frames)
        self.depth_paths = _cut(_by_number(glob.glob(os.path.join(self.input_folder, "depth", "*.png"))), stride, max_frames)
        self.load_poses(os.path.join(self.input_folder, "pose"))
        self.poses = _cut(self.poses, stride, max_frames)
        self.n_img = len(self.color_paths)

    def load_poses(self, path):
        self.poses = []
        for pose_path in _by_number(glob.glob(os.path.join(path, "*.txt"))):
            with open(pose_path, "r") as f:
                self.poses.append(np.array([float(v) for v in f.read().split()], dtype=np.float64).reshape(4, 4))


class TUM_RGBD(BaseDataset):
    """<input_folder>/rgb.txt, depth.txt and groundtruth.txt (or pose.txt): `timestamp path` and `timestamp tx ty tz qx qy qz qw` lines,
    `#` starts a comment.  Frames are associated by nearest timestamp (max_dt 0.08 s against depth and pose), thinned to 32 a second, and
    the poses are expressed in the first kept camera's frame (that pose is exactly the identity)."""

    def __init__(self, cfg, device="cuda:0", prepare="hip", prefetch=1):
        super().__init__(cfg, device, prepare, prefetch)
        color_paths, depth_paths, poses = self.loadtum(self.input_folder, frame_rate=32)
        stride, max_frames = cfg["stride"], cfg["max_frames"]
        self.color_paths = _cut(color_paths, stride, max_frames)
        self.depth_paths = _cut(depth_paths, stride, max_frames)
        self.poses = _cut(poses, stride, max_frames)
        self.w2c_first_pose = np.linalg.inv(self.poses[0])
        self.n_img = len(self.color_paths)

    @staticmethod
    def parse_list(filepath):
        """the whitespace-separated fields of every line that is neither empty nor a comment"""
        rows = []
        with open(filepath, "r") as f:
            for line in f:
                line = line.strip()
                if line and not line.startswith("#"):
                    rows.append(line.split())
        return rows

    @staticmethod
    def associate_frames(tstamp_image, tstamp_depth, tstamp_pose, max_dt=0.08):
        associations = []
        for i, t in enumerate(tstamp_image):
            j = int(np.argmin(np.abs(tstamp_depth - t)))
            if not np.abs(tstamp_depth[j] - t) < max_dt:
                continue
            if tstamp_pose is None:
                associations.append((i, j))
                continue
            k = int(np.argmin(np.abs(tstamp_pose - t)))
            if np.abs(tstamp_pose[k] - t) < max_dt:
                associations.append((i, j, k))
        return associations

    @staticmethod
    def pose_matrix_from_quaternion(pvec):
        """(tx, ty, tz, qx, qy, qz, qw) -> 4x4 fp64; the quaternion is normalised first"""
        pvec = np.asarray(pvec, dtype=np.float64)
        q = pvec[3:7]
        norm = np.sqrt(np.dot(q, q))
        if not norm > 0.0:
            raise ValueError("a pose with a zero quaternion")
        x, y, z, w = q / norm
        pose = np.eye(4)
        pose[:3, :3] = [[1.0 - 2.0 * (y * y + z * z), 2.0 * (x * y - z * w), 2.0 * (x * z + y * w)],
                        [2.0 * (x * y + z * w), 1.0 - 2.0 * (x * x + z * z), 2.0 * (y * z - x * w)],
                        [2.0 * (x * z - y * w), 2.0 * (y * z + x * w), 1.0 - 2.0 * (x * x + y * y)]]
        pose[:3, 3] = pvec[:3]
        return pose

    def loadtum(self, datapath, frame_rate=-1):
        pose_list = os.path.join(datapath, "groundtruth.txt")
        if not os.path.isfile(pose_list):
            pose_list = os.path.join(datapath, "pose.txt")
        image_data = self.parse_list(os.path.join(datapath, "rgb.txt"))
        depth_data = self.parse_list(os.path.join(datapath, "depth.txt"))
        pose_data = self.parse_list(pose_list)
        tstamp_image = np.array([float(r[0]) for r in image_data], dtype=np.float64)
        tstamp_depth = np.array([float(r[0]) for r in depth_data], dtype=np.float64)
        tstamp_pose = np.array([float(r[0]) for r in pose_data], dtype=np.float64)
        pose_vecs = np.array([[float(v) for v in r[1:8]] for r in pose_data], dtype=np.float64)
        associations = self.associate_frames(tstamp_image, tstamp_depth, tstamp_pose)
        if not associations:
            raise ValueError(f"{datapath}: no colour frame has a depth frame and a pose within 0.08 s")
        kept = [0]
        for i in range(1, len(associations)):
            if tstamp_image[associations[i][0]] - tstamp_image[associations[kept[-1]][0]] > 1.0 / frame_rate:
                kept.append(i)
        images, depths, poses, inv_pose = [], [], [], None
        for ix in kept:
            i, j, k = associations[ix]
            images.append(os.path.join(datapath, image_data[i][1]))
            depths.append(os.path.join(datapath, depth_data[j][1]))
            c2w = self.pose_matrix_from_quaternion(pose_vecs[k])
            if inv_pose is None:
                inv_pose, c2w = np.linalg.inv(c2w), np.eye(4)
            else:
                c2w = inv_pose @ c2w
            poses.append(c2w)
        self.image_timestamps = [float(tstamp_image[associations[ix][0]]) for ix in kept]
        return images, depths, poses


dataset_dict = {"replica": Replica, "scannet": ScanNet, "tumrgbd": TUM_RGBD}


def get_dataset(cfg, device="cuda:0", prepare="hip", prefetch=1):
    return dataset_dict[cfg["dataset"]](cfg, device=device, prepare=prepare, prefetch=prefetch)
