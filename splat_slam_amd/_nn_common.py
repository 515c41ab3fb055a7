"""What the networks on the MFMA convolution kernels share on the Python side (update_op, encoder, resnetv2, vit, dpt_decoder, lpips,
mono_depth): the packing of weights and biases, the tensor record, the tensor and device checks, the current stream, the closed-form
synthetic weights, the scratch cache and the scaffold of a forward call."""
import ctypes as C

import numpy as np
import torch

from splat_slam_amd import _native as nat


def round_up(v, m):
    return (v + m - 1) // m * m


def pack_weight(w, cin_pad, row_pad=1):
    """[cout, cin, k, k] -> fp16 [round_up(cout, row_pad)][round_up(k*k*cin_pad, 32)], column tap * cin_pad + channel, zero padding; the
    update operator's kernel reads whole 64-row tiles (row_pad 64), the others have cout a multiple of their tile"""
    cout, cin, k, _ = w.shape
    p = torch.zeros((cout, k * k, cin_pad), dtype=torch.float16, device=w.device)
    p[:, :, :cin] = w.permute(0, 2, 3, 1).reshape(cout, k * k, cin).to(torch.float16)
    out = torch.zeros((round_up(cout, row_pad), round_up(k * k * cin_pad, 32)), dtype=torch.float16, device=w.device)
    out[:cout, :k * k * cin_pad] = p.reshape(cout, -1)
    return out.contiguous()


def pack_bias(b, cout, device, row_pad=1):
    """[cout] (None: zeros) rounded to fp16 -> fp32 [round_up(cout, row_pad)]"""
    out = torch.zeros(round_up(cout, row_pad), dtype=torch.float32, device=device)
    if b is not None:
        out[:cout] = b.to(torch.float16).to(torch.float32)
    return out


def stream(dev):
    return torch.cuda.current_stream(dev).cuda_stream


F16_F32 = (torch.float16, torch.float32)


def gpu_tensor(what, name, t, dtypes, dtype_text=None):
    """t if it is a GPU tensor of one of dtypes, else RuntimeError under the caller's name `what`; dtype_text: how the caller's message
    names the dtypes ("fp16 or fp32"), by default the tuple itself"""
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise RuntimeError(f"{what} (MI355X build): {name} must be a GPU tensor; there is no CPU path")
    if t.dtype not in dtypes:
        raise RuntimeError(f"{what}: {name} must be {dtype_text or f'one of {dtypes}'}, got {t.dtype}")
    return t


def network_device(device, what, noun):
    """the device a network lives on: cuda only, the index filled in; noun: what the module calls its network in the message"""
    device = torch.device(device)
    if device.type != "cuda":
        raise RuntimeError(f"{what} (MI355X build): the {noun} lives on a GPU; there is no CPU path")
    return torch.device("cuda", torch.cuda.current_device()) if device.index is None else device


def tensor_desc(t):
    """SgrUpdateTensor of a [E,C,h,w] view (None: zeros)"""
    d = nat.SgrUpdateTensor()
    if t is None:
        d.data, d.dtype = None, nat.SGR_UPDATE_F32
        return d
    d.data = t.data_ptr()
    d.stride = (C.c_int64 * 4)(*t.stride())
    d.dtype = nat.SGR_UPDATE_F16 if t.dtype == torch.float16 else nat.SGR_UPDATE_F32
    return d


def name_hash(name):
    h = 2166136261                        # FNV-1a, 32 bit
    for b in name.encode():
        h = ((h ^ b) * 16777619) & 0xFFFFFFFF
    return h


def hash_uniform(name, n, seed):
    """n values of U[-1, 1) as float64: the murmur3 finaliser of (flat index * 0x9E3779B1 + FNV-1a(name) + seed * 0x85EBCA77) mod 2^32."""
    m = np.uint64(0xFFFFFFFF)
    x = (np.arange(n, dtype=np.uint64) * np.uint64(0x9E3779B1) + np.uint64(name_hash(name))
         + np.uint64((int(seed) * 0x85EBCA77) & 0xFFFFFFFF)) & m
    x ^= x >> np.uint64(16)
    x = (x * np.uint64(0x85EBCA6B)) & m
    x ^= x >> np.uint64(13)
    x = (x * np.uint64(0xC2B2AE35)) & m
    x ^= x >> np.uint64(16)
    return x.astype(np.float64) / 2.0 ** 31 - 1.0


class ScratchCache:
    """one uint8 buffer per key (a shape and a stream), the four most recent kept"""

    def __init__(self):
        self._bufs = {}

    def get(self, key, device, nbytes_of, unsupported, grow=False):
        """nbytes_of() sizes a missing buffer; 0 raises RuntimeError(unsupported).  grow, for a key that leaves the batch out: nbytes_of()
        is asked on every call and a held buffer that is smaller is replaced, so that a buffer ends up as large as the largest batch"""
        nbytes = nbytes_of() if grow or key not in self._bufs else None
        if nbytes == 0:
            raise RuntimeError(unsupported)
        buf = self._bufs.pop(key, None)
        if buf is None or (grow and buf.numel() < nbytes):
            buf = torch.empty(nbytes, dtype=torch.uint8, device=device)
        while len(self._bufs) >= 4:
            self._bufs.pop(next(iter(self._bufs)))
        self._bufs[key] = buf
        return buf


def run_forward(net, call, key, nbytes_of, unsupported, forward, grow=False):
    """Enqueues the launches first_launch..last_launch of the record `call` on the current stream of net.device: the scratch buffer of
    (key, stream) out of net._scratch (sized by nbytes_of(), see ScratchCache.get), then the C entry point named `forward` on
    net._weights and the record."""
    with torch.cuda.device(net.device):
        st = stream(net.device)
        scratch = net._scratch.get(key + (st,), net.device, nbytes_of, unsupported, grow)
        nat.check(getattr(nat.lib(), forward)(C.byref(net._weights), C.byref(call), scratch.data_ptr(), scratch.numel(), st), forward)
