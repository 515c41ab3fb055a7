"""fp64 statement of the tracker's encoders (splat_slam_amd.encoder), written from their equations, and the torch composition of the same
weights under autocast that the GPU tests and scripts/encoder_times.py take as the scale of fp16 arithmetic.

    n(v)   = (v - mean_hw(v)) / sqrt(var_hw(v) + 1e-5) per (image, channel), biased variance (fnet), or v (cnet)
    x      = relu(n(conv7x7/2(image)))                                         3 -> 32
    block  : y = relu(n(conv3x3/s(x)));  y = relu(n(conv3x3(y)));  x = relu(x' + y),  x' = x (s = 1) or n(conv1x1/2(x)) (s = 2)
    layer1 = block(32, s=1), block(32);  layer2 = block(64, s=2), block(64);  layer3 = block(128, s=2), block(128)
    out    = conv1x1(x)                                                      128 -> out_dim
"""
import torch
import torch.nn.functional as F

EPS = 1e-5
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


def round_fp16(sd):
    """the values the encoder holds: every tensor rounded to fp16"""
    return {k: v.to(torch.float16).to(torch.float32) for k, v in sd.items()}


def instance_stats(y):
    """mean and biased standard deviation sqrt(var + eps) per (image, channel) of [B,C,h,w]"""
    mu = y.mean(dim=(2, 3), keepdim=True)
    return mu, ((y - mu) ** 2).mean(dim=(2, 3), keepdim=True).add(EPS).sqrt()


def conv2d_ref(x, w, b=None, stride=1, norm=None, act="none", residual=None, return_stats=False):
    """fp64 convolution with zero padding (k - 1) / 2 on [B,cin,h,w], then the norm, the activation (none, relu, split = tanh of the
    first 128 channels | relu of the rest) and relu(residual + .)"""
    x, w = x.double().cpu(), w.double().cpu()
    y = F.conv2d(x, w, None if b is None else b.double().cpu(), stride=stride, padding=w.shape[-1] // 2)
    stats = None
    if norm == "instance":
        stats = instance_stats(y)
        y = (y - stats[0]) / stats[1]
    if act == "relu":
        y = torch.relu(y)
    elif act == "split":
        return torch.tanh(y[:, :128]), torch.relu(y[:, 128:])
    if residual is not None:
        y = torch.relu(residual.double().cpu() + y)
    return (y, stats) if return_stats else y


def encoder_ref(sd, norm, images):
    """the encoder in fp64 on the weights sd (keys of encoder.LAYER_SHAPES) exactly as given; images [b,n,3,H,W] -> [b,n,out_dim,h,w]"""
    P = {k: v.double().cpu() for k, v in sd.items()}
    b, n = images.shape[:2]

    def conv(name, x, stride=1, act="none", residual=None, normed=True):
        return conv2d_ref(x, P[name + ".weight"], P[name + ".bias"], stride, norm if normed else None, act, residual)

    x = conv("conv1", images.double().cpu().flatten(0, 1), 2, "relu")
    for layer, stride in (("layer1", 1), ("layer2", 2), ("layer3", 2)):
        for blk, s in ((".0", stride), (".1", 1)):
            y = conv(layer + blk + ".conv1", x, s, "relu")
            skip = x if s == 1 else conv(layer + blk + ".downsample.0", x, s)
            x = conv(layer + blk + ".conv2", y, 1, "relu", skip)
    x = conv("conv2", x, normed=False)
    return x.reshape((b, n) + tuple(x.shape[1:]))


class TorchEncoder:
    """The same encoder as a composition of torch ops with the reference's signature: F.conv2d on fp32 parameters and F.instance_norm
    under torch.autocast, so every convolution runs in fp16 through the vendor library and every other step follows autocast's rules."""

    def __init__(self, sd, norm, device):
        self.p = {k: v.to(device=device, dtype=torch.float32) for k, v in sd.items()}
        self.norm = norm

    def conv(self, name, x, stride=1, normed=True):
        w = self.p[name + ".weight"]
        y = F.conv2d(x, w, self.p[name + ".bias"], stride=stride, padding=w.shape[-1] // 2)
        return F.instance_norm(y, eps=EPS) if normed and self.norm == "instance" else y

    def __call__(self, images, mean=None, std=None):
        b, n = images.shape[:2]
        with torch.autocast("cuda", enabled=True):
            x = images.flatten(0, 1)
            if mean is not None:
                x = (x.float() - torch.tensor(mean, device=x.device)[:, None, None]) / torch.tensor(std, device=x.device)[:, None, None]
            x = torch.relu(self.conv("conv1", x, 2))
            for layer, stride in (("layer1", 1), ("layer2", 2), ("layer3", 2)):
                for blk, s in ((".0", stride), (".1", 1)):
                    y = torch.relu(self.conv(layer + blk + ".conv1", x, s))
                    y = torch.relu(self.conv(layer + blk + ".conv2", y))
                    if s != 1:
                        x = self.conv(layer + blk + ".downsample.0", x, s)
                    x = torch.relu(x + y)
            x = self.conv("conv2", x, normed=False)
        return x.reshape((b, n) + tuple(x.shape[1:]))

    def context(self, images, mean=None, std=None):
        with torch.autocast("cuda", enabled=True):
            net, inp = self(images, mean, std).split([128, 128], dim=2)
            return net.tanh(), inp.relu()


def make_images(b, n, H, W, seed, device="cpu", dtype=torch.float32):
    """N(0, 1) images, every value fp16-representable"""
    g = torch.Generator().manual_seed(seed)
    return torch.randn(b, n, 3, H, W, generator=g).to(torch.float16).to(dtype).to(device)
