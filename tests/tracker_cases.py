"""Shared inputs of tests/test_gpu_alt_pyramid.py, tests/test_gpu_tracker.py and tests/test_tracker_cpu.py: the coordinate recipe of
tests/test_gpu_corr.py, the twelve-keyframe video and the stub update operator of tests/test_gpu_factor_graph.py (restated, so that
no test module imports another), a stub whose output depends on the correlation features, the tracker's configuration dict and a
synthetic image stream.  Nothing here touches a GPU at import."""
import types

import numpy as np
import torch

DEV = "cuda"
N_FRAMES, HT, WD = 12, 48, 64


def f32(a, device=DEV):
    return torch.tensor(np.asarray(a), dtype=torch.float32, device=device).contiguous()


def li(a, device=DEV):
    return torch.tensor(np.asarray(a), dtype=torch.int64, device=device).reshape(-1)


def np_(t):
    return t.detach().cpu().numpy()


def axis_set(rng, n, size, r):
    """interior fractional points, exact integers, points within r+1 of both borders on both sides, points wholly outside, -1e-7"""
    k = rng.integers(0, 7, n)
    v = rng.uniform(0, size - 1, n)
    v = np.where(k == 1, np.round(rng.uniform(-(r + 2), size + r + 1, n)), v)
    v = np.where(k == 2, rng.uniform(-(r + 1), r + 1, n), v)
    v = np.where(k == 3, rng.uniform(size - 1 - (r + 1), size - 1 + (r + 1), n), v)
    v = np.where(k == 4, np.where(rng.random(n) < 0.5, -(r + 1.5) - rng.uniform(0, 40, n), size + r + 0.5 + rng.uniform(0, 4000, n)), v)
    v = np.where(k == 5, -1e-7, v)
    return v                                            # k == 0 and 6: interior


def edge_coords(rng, E, H, W, r):
    """[E,H,W,2] fp32 (x, y) at the scale of level 0"""
    n = E * H * W
    return torch.tensor(np.stack([axis_set(rng, n, W, r), axis_set(rng, n, H, r)], -1).reshape(E, H, W, 2), dtype=torch.float32)


def make_video(**kw):
    """twelve keyframes on a smooth path in front of a gently varying surface, DepthVideo(48, 64, buffer=16)"""
    from splat_slam_amd.depth_video import DepthVideo
    rng = np.random.default_rng(40)
    v = DepthVideo(HT, WD, buffer=kw.pop("buffer", 16), device=DEV, **kw)
    h, w = HT // 8, WD // 8
    yy, xx = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    for f in range(N_FRAMES):
        ang = 0.01 * f
        pose = np.array([0.03 * f, 0.01 * np.sin(f), 0.015 * f, 0.0, np.sin(ang / 2), 0.0, np.cos(ang / 2)])
        disp = 0.5 + 0.05 * np.sin(0.7 * xx + 0.3 * f) * np.cos(0.5 * yy) + rng.uniform(-0.005, 0.005, (h, w))
        v.append(float(f), torch.zeros(3, HT, WD, dtype=torch.uint8, device=DEV), f32(pose), f32(disp), None, f32([7.0, 7.5, 4.0, 3.0]))
    v.mono_disps[:N_FRAMES] = 1.7 * v.disps[:N_FRAMES] + 0.05
    v.fmaps[:N_FRAMES] = torch.tensor(rng.integers(-8, 9, size=(N_FRAMES, 1, 128, h, w)) / 8.0, dtype=torch.half, device=DEV)
    v.nets[:N_FRAMES] = torch.tensor(rng.normal(size=(N_FRAMES, 128, h, w)), dtype=torch.half, device=DEV)
    v.inps[:N_FRAMES] = torch.tensor(rng.normal(size=(N_FRAMES, 128, h, w)), dtype=torch.half, device=DEV)
    return v


def stub(net, inp, corr, motn, ii, jj):
    """a deterministic stand-in for the update operator, with the shapes of the reference's (GraphAgg: one eta and one mask per
    distinct source frame)"""
    E, h, w = motn.shape[1], motn.shape[3], motn.shape[4]
    K = torch.unique(ii).shape[0]
    g = torch.Generator(device="cpu").manual_seed(1234 + E)
    delta = (0.1 * motn[:, :, :2]).permute(0, 1, 3, 4, 2).contiguous()
    weight = torch.full((1, E, h, w, 2), 0.5, device=motn.device)
    damping = (0.01 * torch.rand((1, K, h, w), generator=g)).to(motn.device)
    upmask = (4.0 * torch.rand((1, K, 576, h, w), generator=g) - 2.0).to(motn.device)
    return net, delta, weight, damping, upmask


def stub_corr(net, inp, corr, motn, ii, jj):
    """the stub with a flow correction that is a function of two correlation channels (one of level 0, one of level 2), so that what the
    graph does with it depends on every bit of the lookup"""
    net, delta, weight, damping, upmask = stub(net, inp, corr, motn, ii, jj)
    delta = delta + 0.01 * torch.tanh(corr[:, :, [24, 2 * 49 + 24]].float()).permute(0, 1, 3, 4, 2)
    return net, delta.contiguous(), weight, damping, upmask


def make_cfg(device=DEV, **over):
    """the keys the tracker reads, with the values of the reference's configuration where the tests do not need others;
    over: 'a.b.c'=value"""
    cfg = {"device": device,
           "mapping": {"every_keyframe": 1},
           "tracking": {"beta": 0.75, "warmup": 8, "max_age": 50, "mono_thres": 0.1, "buffer": 16,
                        "motion_filter": {"thresh": 4.0},
                        "multiview_filter": {"thresh": 0.01, "visible_num": 2},
                        "frontend": {"enable_loop": False, "enable_online_ba": False, "keyframe_thresh": 4.0, "thresh": 16.0, "window": 25,
                                     "radius": 2, "nms": 1, "max_factors": 75},
                        "backend": {"thresh": 22.0, "radius": 2, "nms": 3, "normalize": True, "loop_window": 25, "loop_thresh": 25.0,
                                    "loop_radius": 1, "loop_nms": 12, "BA_type": "DSPO", "ba_freq": 20}}}
    for key, val in over.items():
        d = cfg
        *path, last = key.split(".")
        for p in path:
            d = d[p]
        assert last in d, key
        d[last] = val
    return cfg


def net_of(update_op):
    """what Frontend and Backend need of a DroidNet: its update operator"""
    return types.SimpleNamespace(update=update_op)


class SyntheticStream:
    """n frames of a smooth moving pattern, [1,3,H,W] in [0, 1]: (timestamp, image, None, None), as the reference's datasets yield"""

    def __init__(self, n, ht=HT, wd=WD, device=DEV, step=1.0):
        self.n, self.ht, self.wd, self.device, self.step = n, ht, wd, device, step

    def __len__(self):
        return self.n

    def __getitem__(self, i):
        if not 0 <= i < self.n:
            raise IndexError(i)
        y, x = torch.meshgrid(torch.arange(self.ht, dtype=torch.float32), torch.arange(self.wd, dtype=torch.float32), indexing="ij")
        s = 3.0 * i
        img = torch.stack([0.5 + 0.5 * torch.sin(0.31 * (x + s) + 0.11 * y), 0.5 + 0.5 * torch.cos(0.23 * (y - s) + 0.07 * x),
                           0.5 + 0.5 * torch.sin(0.17 * (x + y + s))])
        return self.step * i, img[None].to(self.device), None, None

    def __iter__(self):
        return (self[i] for i in range(self.n))

    def get_intrinsic(self):
        return torch.tensor([56.0, 60.0, 32.0, 24.0], device=self.device)
