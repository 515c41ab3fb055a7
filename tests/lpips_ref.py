"""The fp64 restatement of LPIPS v0.1 on the AlexNet trunk as splat_slam_amd.lpips defines it ("LPIPS"), the oracle
of tests/test_lpips_cpu.py and tests/test_gpu_lpips.py, and the torch composition (fp16 convolutions and pools, the distance in fp32)
that the project's criterion compares the kernels with.  P is lpips.prepare(canon): conv1..5.weight / .bias (already rounded to fp16),
lin0..4 [1,C,1,1], shift, scale [3]."""
import torch
import torch.nn.functional as F

GEOMETRY = ((4, 2), (1, 2), (1, 1), (1, 1), (1, 1))          # (stride, padding) of conv1 .. conv5
EPS = 1e-8


def scale_input(x, shift, scale, normalize=True):
    """(2 x - 1 - shift) / scale per channel in fp64 (x - shift without normalize); x [N,3,H,W]"""
    x = x.double()
    if normalize:
        x = 2.0 * x - 1.0
    return (x - shift.double().to(x.device).reshape(1, 3, 1, 1)) / scale.double().to(x.device).reshape(1, 3, 1, 1)


def exposed(render, a=None, b=None):
    """clamp(exp(a) render + b, 0, 1) in fp64 from the fp32 values; a, b scalars or None (identity)"""
    r = render.double()
    if a is not None:
        r = torch.exp(a.double()) * r
    if b is not None:
        r = r + b.double()
    return r.clamp(0.0, 1.0)


def conv_ref(x, w, b, stride, pad):
    """relu(conv2d) in fp64 on the values given"""
    return torch.relu(F.conv2d(x.double(), w.double(), b.double(), stride=stride, padding=pad))


def conv_unfold(x, w, b, stride, pad):
    """the same convolution from its sum: every output pixel's window as a row (F.unfold), one matrix product with [cout, cin k k]"""
    x, w = x.double(), w.double()
    N, _, h, wd = x.shape
    cout, _, k, _ = w.shape
    ho, wo = (h + 2 * pad - k) // stride + 1, (wd + 2 * pad - k) // stride + 1
    cols = F.unfold(x, k, padding=pad, stride=stride)                           # [N, cin k k, ho wo]
    y = torch.einsum("ok,nkp->nop", w.reshape(cout, -1), cols) + b.double().reshape(1, cout, 1)
    return torch.relu(y).reshape(N, cout, ho, wo)


def pool_ref(x):
    return F.max_pool2d(x, 3, 2)


def unit(f):
    """f / sqrt(1e-8 + sum_c f^2), f [N,C,...]"""
    return f / torch.sqrt(EPS + (f * f).sum(1, keepdim=True))


def pixel_distance(f0, f1, w):
    """d_p = sum_c w_c (u_c - v_c)^2 in fp64: f0, f1 [N,C,...], w [C] or [1,C,1,1] -> [N,...]"""
    u, v = unit(f0.double()), unit(f1.double())
    shape = (1, -1) + (1,) * (f0.dim() - 2)
    return (w.double().reshape(shape) * (u - v) ** 2).sum(1)


def pixel_bound_sum(f0, f1, w):
    """sum_c w_c (|u_c| + |v_c|)^2 per pixel, what the distance kernel's rounding errors are proportional to"""
    u, v = unit(f0.double()), unit(f1.double())
    shape = (1, -1) + (1,) * (f0.dim() - 2)
    return (w.double().reshape(shape) * (u.abs() + v.abs()) ** 2).sum(1)


def trunk(P, x, cast=lambda t: t):
    """the five taps of the scaled input x; cast is applied to every map a layer hands on"""
    taps = []
    for i, (stride, pad) in enumerate(GEOMETRY):
        w, b = P[f"conv{i + 1}.weight"].to(x.device, x.dtype), P[f"conv{i + 1}.bias"].to(x.device, x.dtype)
        x = cast(torch.relu(F.conv2d(x, w, b, stride=stride, padding=pad)))
        taps.append(x)
        if i < 2:
            x = F.max_pool2d(x, 3, 2)
    return taps


def _levels(P, t0, t1):
    lv = [pixel_distance(a, b, P[f"lin{i}"].to(a.device)).flatten(1).mean(1) for i, (a, b) in enumerate(zip(t0, t1))]
    return torch.stack(lv, 1)


def lpips_ref(P, x0, x1, normalize=True):
    """(total [N], levels [N,5]) in fp64 with the prepared parameters; x0, x1 [N,3,H,W] taken as they are"""
    s0, s1 = (scale_input(x, P["shift"], P["scale"], normalize) for x in (x0, x1))
    levels = _levels(P, trunk(P, s0), trunk(P, s1))
    return levels.sum(1), levels


def lpips_torch(P, x0, x1, normalize=True):
    """the torch composition of the same weights: the input scaled in fp32 and rounded to fp16, F.conv2d / F.max_pool2d in fp16, the
    distance in fp32; (total [N], levels [N,5]) fp32"""
    taps = []
    for x in (x0, x1):
        x = x.float()
        if normalize:
            x = 2.0 * x - 1.0
        s = (x - P["shift"].float().to(x.device).reshape(1, 3, 1, 1)) / P["scale"].float().to(x.device).reshape(1, 3, 1, 1)
        taps.append(trunk(P, s.to(torch.float16)))
    lv = []
    for i, (a, b) in enumerate(zip(*taps)):
        a, b = a.float(), b.float()
        u, v = a / torch.sqrt(EPS + (a * a).sum(1, keepdim=True)), b / torch.sqrt(EPS + (b * b).sum(1, keepdim=True))
        lv.append(F.conv2d((u - v) ** 2, P[f"lin{i}"].float().to(a.device)).flatten(1).mean(1))
    levels = torch.stack(lv, 1)
    return levels.sum(1), levels
