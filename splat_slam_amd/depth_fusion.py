"""Keyframe depth fusion (Mapper.get_w2c_and_depth of the reference's src/mapper.py:258-301): what turns a tracker keyframe into the
depth map and pose the mapper seeds and supervises with, on the gfx950 kernels `sgr_fuse_*` (include/splat_hip.h, csrc/sgr_fuse.hip).
Stated in DESIGN.md section 3, "Keyframe depth fusion".

    prepare_mono(mono) -> (mono_filled, eroded)
        mono [H,W] or [n,H,W] fp32: pixels above 4 x the map's mean removed, the 11 x 11 erosion of what is left (eroded, uint8), and
        the removed pixels filled from the known ones in passes (mono_filled).  Depends on the mono map alone: once per keyframe.
    fuse_depth(disps_up, valid_depth_mask, mono_filled, eroded, inds, min_valid=100) -> (depth [m,H,W], scale [m], shift [m], invalid [m])
        disps_up [N,H,W] fp32, valid_depth_mask [N,H,W] bool|uint8, mono_filled [N,H,W] fp32 and eroded [N,H,W] uint8 hold one slot per
        video index and are read in place; inds names the m frames (any order, repeats allowed).  Per frame: invalid = fewer than
        min_valid valid pixels; (scale, shift) = the least-squares fit of mono_filled to 1 / disps_up over eroded & valid; depth =
        valid ? 1 / disps_up : mono_filled * scale + shift (bit for bit torch's expression).  An invalid frame gets 0 outside the mask
        and its scale and shift are left as torch.empty made them.  inds is a sequence of ints or a CPU int64 tensor, which is
        range-checked here, or a GPU int64 tensor, which the host does not read: an entry outside [0, N) gives a slot flagged
        invalid with a depth of zeros.
    KeyframeDepth(video)
        put_mono(video_idx, mono)       prepares the keyframe's mono map once and keeps it
        get(video_idxs) -> (depth [m,H,W], w2c [m,4,4], invalid list[bool])
            one fuse_depth call over the video's buffers, the poses in one batched lietorch call, video.depth_scale / depth_shift
            updated for the valid frames (the reference's side effect), and exactly one host read, for the invalid flags
        get_w2c_and_depth(video_idx) -> (depth [H,W], w2c [4,4], invalid)      the reference's single-frame form

Every tensor lives on the GPU; there is no CPU path.  All work goes on the current torch stream; prepare_mono and fuse_depth never
synchronise with the host.  Differences from the reference, both deliberate: the holes are filled by the distance-weighted passes stated
in DESIGN.md, not by cv2's Navier-Stokes in-painting (a serial fast-marching method on the host); and what depends on the mono map alone
is computed once per keyframe and cached, where the reference redoes it on the host for every past keyframe at every mapped keyframe.
"""
import torch

from splat_slam_amd import _native as nat

__all__ = ["prepare_mono", "fuse_depth", "KeyframeDepth"]

_MASK = (torch.bool, torch.uint8)


def _gpu(name, t, dtype, ndim=None):
    """dtype, rank and layout of one argument; the device is checked by _same_device once every shape is known to be right."""
    dtypes = dtype if isinstance(dtype, tuple) else (dtype,)
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"depth_fusion: {name} must be a torch.Tensor")
    if t.dtype not in dtypes:
        raise TypeError(f"depth_fusion: {name} must be {' or '.join(str(d) for d in dtypes)}, got {t.dtype}")
    if ndim is not None and t.dim() != ndim:
        raise ValueError(f"depth_fusion: {name} must have {ndim} dimensions, got shape {tuple(t.shape)}")
    if not t.is_contiguous():
        raise ValueError(f"depth_fusion: {name} must be contiguous")
    return t


def _same_device(*ts):
    dev = ts[0].device
    for t in ts:
        if not t.is_cuda:
            raise RuntimeError("depth_fusion (MI355X build): every tensor must be a GPU tensor; there is no CPU path")
    for t in ts[1:]:
        if t.device != dev:
            raise RuntimeError(f"depth_fusion: every tensor must be on {dev}, found one on {t.device}")
    return dev


def _stream(dev):
    return torch.cuda.current_stream(dev).cuda_stream


def _scratch(fn, lib, num, h, w, dev):
    nbytes = lib.sgr_fuse_scratch_bytes(num, h, w)
    if nbytes == 0:
        raise ValueError(f"depth_fusion.{fn}: unsupported sizes (frames={num} h={h} w={w})")
    return torch.empty(nbytes, dtype=torch.uint8, device=dev), nbytes


def _prepare_into(mono, mono_filled, eroded):
    """mono, mono_filled [n,H,W] fp32 and eroded [n,H,W] uint8, checked by the callers"""
    n, h, w = mono.shape
    dev = mono.device
    lib = nat.lib()
    scratch, nbytes = _scratch("prepare_mono", lib, n, h, w, dev)
    with torch.cuda.device(dev):
        nat.check(lib.sgr_fuse_prepare(mono.data_ptr(), n, h, w, mono_filled.data_ptr(), eroded.data_ptr(), scratch.data_ptr(), nbytes,
                                       _stream(dev)), "sgr_fuse_prepare")


def prepare_mono(mono):
    single = isinstance(mono, torch.Tensor) and mono.dim() == 2
    if single:
        mono = mono.unsqueeze(0)
    _gpu("mono", mono, torch.float32, 3)
    n, h, w = mono.shape
    if h < 1 or w < 1:
        raise ValueError(f"depth_fusion.prepare_mono: mono must be [H,W] or [n,H,W] with H, W > 0, got {tuple(mono.shape)}")
    if n > nat.SGR_FUSE_MAX_FRAMES:
        raise ValueError(f"depth_fusion.prepare_mono: {n} maps in one call exceed the supported {nat.SGR_FUSE_MAX_FRAMES}")
    dev = _same_device(mono)
    mono_filled = torch.empty_like(mono)
    eroded = torch.empty((n, h, w), dtype=torch.uint8, device=dev)
    if n:
        _prepare_into(mono, mono_filled, eroded)
    return (mono_filled[0], eroded[0]) if single else (mono_filled, eroded)


def _inds(inds, n, dev):
    """int64 on the device; what the host knows is range-checked before anything is launched"""
    if isinstance(inds, torch.Tensor):
        _gpu("inds", inds, torch.int64, 1)
        if inds.is_cuda:
            return inds
        host = inds.tolist()
    else:
        try:
            host = [int(i) for i in inds]
        except TypeError:
            raise TypeError("depth_fusion: inds must be a sequence of ints or an int64 tensor") from None
    for i in host:
        if not 0 <= i < n:
            raise IndexError(f"depth_fusion: frame index {i} lies outside [0, {n})")
    return torch.tensor(host, dtype=torch.int64).reshape(-1).to(dev, non_blocking=True)


def fuse_depth(disps_up, valid_depth_mask, mono_filled, eroded, inds, min_valid=100):
    _gpu("disps_up", disps_up, torch.float32, 3)
    _gpu("valid_depth_mask", valid_depth_mask, _MASK, 3)
    _gpu("mono_filled", mono_filled, torch.float32, 3)
    _gpu("eroded", eroded, torch.uint8, 3)
    n, h, w = disps_up.shape
    if n < 1 or h < 1 or w < 1:
        raise ValueError(f"depth_fusion.fuse_depth: disps_up must be [N,H,W] with N, H, W > 0, got {tuple(disps_up.shape)}")
    for name, t in (("valid_depth_mask", valid_depth_mask), ("mono_filled", mono_filled), ("eroded", eroded)):
        if t.shape != disps_up.shape:
            raise ValueError(f"depth_fusion.fuse_depth: {name} must have the shape of disps_up {tuple(disps_up.shape)}, "
                             f"got {tuple(t.shape)}")
    dev = _same_device(disps_up, valid_depth_mask, mono_filled, eroded)
    min_valid = int(min_valid)
    inds = _inds(inds, n, dev)
    _same_device(disps_up, inds)
    m = inds.shape[0]
    if m > nat.SGR_FUSE_MAX_FRAMES:
        raise ValueError(f"depth_fusion.fuse_depth: {m} frames in one call exceed the supported {nat.SGR_FUSE_MAX_FRAMES}")
    depth = torch.empty((m, h, w), dtype=torch.float32, device=dev)
    scale = torch.empty((m,), dtype=torch.float32, device=dev)
    shift = torch.empty((m,), dtype=torch.float32, device=dev)
    invalid = torch.empty((m,), dtype=torch.uint8, device=dev)
    if m:
        lib = nat.lib()
        scratch, nbytes = _scratch("fuse_depth", lib, m, h, w, dev)
        with torch.cuda.device(dev):
            nat.check(lib.sgr_fuse_depth(disps_up.data_ptr(), valid_depth_mask.data_ptr(), mono_filled.data_ptr(), eroded.data_ptr(), n, h,
                                         w, inds.data_ptr(), m, min_valid, depth.data_ptr(), scale.data_ptr(), shift.data_ptr(),
                                         invalid.data_ptr(), scratch.data_ptr(), nbytes, _stream(dev)), "sgr_fuse_depth")
    return depth, scale, shift, invalid


class KeyframeDepth:
    """The mapper's view of a DepthVideo: fused depth and world-to-camera pose of its keyframes.  Holds one prepared mono map per
    video index (the buffers are allocated at the first put_mono)."""

    def __init__(self, video, min_valid=100):
        self.video, self.min_valid = video, int(min_valid)
        self.mono_filled = self.eroded = None
        self.has_mono = set()

    def put_mono(self, video_idx, mono):
        v = self.video
        video_idx = int(video_idx)
        n, h, w = v.disps_up.shape
        if not 0 <= video_idx < n:
            raise IndexError(f"KeyframeDepth.put_mono: video index {video_idx} lies outside [0, {n})")
        _gpu("mono", mono, torch.float32, 2)
        if tuple(mono.shape) != (h, w):
            raise ValueError(f"KeyframeDepth.put_mono: mono must be [H,W] = {(h, w)}, got {tuple(mono.shape)}")
        _same_device(v.disps_up, mono)
        if self.mono_filled is None:
            self.mono_filled = torch.zeros_like(v.disps_up)
            self.eroded = torch.zeros(v.disps_up.shape, dtype=torch.uint8, device=v.disps_up.device)
        _prepare_into(mono.unsqueeze(0), self.mono_filled[video_idx:video_idx + 1], self.eroded[video_idx:video_idx + 1])
        self.has_mono.add(video_idx)

    def get(self, video_idxs):
        import lietorch
        v = self.video
        idxs = [int(i) for i in video_idxs]
        for i in idxs:
            if i not in self.has_mono:
                raise KeyError(f"KeyframeDepth.get: no mono map was put for video index {i}")
        ix = torch.tensor(idxs, dtype=torch.int64).to(v.poses.device, non_blocking=True)      # (in range: each has a mono map)
        depth, scale, shift, invalid = fuse_depth(v.disps_up, v.valid_depth_mask, self.mono_filled, self.eroded, ix, self.min_valid)
        w2c = lietorch.SE3(v.poses[ix]).matrix()            # the video's poses map world to camera
        # the reference's side effect (get_depth_scale_and_shift): the fit of every valid frame goes into the video; of a frame named
        # twice both entries carry the same bits
        ok = invalid == 0
        v.depth_scale[ix] = torch.where(ok, scale, v.depth_scale[ix])
        v.depth_shift[ix] = torch.where(ok, shift, v.depth_shift[ix])
        return depth, w2c, [bool(b) for b in invalid.tolist()]          # the one host read

    def get_w2c_and_depth(self, video_idx):
        depth, w2c, invalid = self.get([video_idx])
        return depth[0], w2c[0], invalid[0]
