"""Scenes with EXACT per-8x8-tile list lengths, knife-free by construction (CPU; no GPU needed to build or check them).

The tile kernels pick one of about a dozen programs from two inputs: the caller's list hint (SgrWorkspace.max_list_hint) and the
actual length of each tile's list.  These scenes pin the second input exactly, so that a test can walk the first through every class:

* blanket_scene(L, W, H): L isotropic Gaussians centred on the optical axis, each with a 2D standard deviation of ten image
  diagonals.  Every pixel sees alpha = opacity * G with G >= 0.998, the alpha = 1/255 contour lies far outside the image, and every
  8x8 bin holds exactly L pairs.  View depths are distinct (spacing >= 1.4e-3 at depths 2..8) and permuted against the index.
* mixed_scene(W, H): eight blanket Gaussians plus "stacks" of point-like Gaussians (2D variance = the 0.3 dilation) centred
  between the four middle pixels of one bin each: a stack member reaches those four pixels with alpha = 1.4/255 and no other
  pixel (next ring: alpha = 0.05/255), and its level-set box lies inside its bin, so it adds exactly one pair to exactly one bin.
  One view then has bins of 8 (only the blanket), 65..128, 257..512 and > 1024 entries.

Knife-freeness (oracle/raster_oracle.py: knife_edge_gaussians) is designed in, not searched for:
* alpha vs 1/255: blanket opacities are >= 0.006 (alpha >= 1.5/255), stack alphas are 1.4/255 inside and 0.05/255 outside;
* the transmittance thresholds T' = 1e-4 (termination) and 0.5 (n_touched): opacities are assigned in depth order, tracking T at
  every pixel in fp64; a splat whose step would bring T at some pixel within JUMP_MARGIN (2 %) of a threshold gets the opacity
  that takes every pixel at least that far BELOW it in one step (G varies by < 0.2 % over the image, so all pixels cross on the
  same splat).  The mixed scene's nearest Gaussian is a blanket of opacity 0.6 (T = 0.4 behind it) and its lists never reach
  T = 1e-4 (T >= 6e-4 behind the longest stack);
* the radius ceil(3 sqrt(lambda)): each blanket scale is solved so that 3 sqrt(lambda) lies half-way between two integers;
  stack radii are 3 sqrt(0.616) = 2.35;
* the 16-pixel tile rectangle: blanket rectangles are clamped far outside the image, stack centres sit at 8k + 3.5.
tests/test_list_scenes_cpu.py checks all of it with the fp64 oracle.
"""
import functools
import math

import torch

from oracle import raster_oracle as O

BLANKET_LENGTHS = (1, 2, 16, 17, 32, 33, 64, 65, 128, 129, 256, 257, 512, 513, 768, 769, 1024, 1025, 2048, 4096, 4097)
IMAGES = ((44, 20), (72, 40))          # partial 8x8 bins / partial 16x16 super tiles, 6 and 15 super tiles
MIXED_IMAGE = (72, 40)
MIXED_BLANKET = 8
# (bin x, bin y, members): bins of 8 + members entries; every other bin holds the blanket's 8
MIXED_STACKS = ((1, 1, 100), (6, 1, 120), (3, 2, 300), (7, 3, 480), (2, 3, 1030), (5, 3, 1200))
MIXED_REGIMES = ((1, 16), (65, 128), (257, 512), (1025, 1 << 30))
JUMP_MARGIN = 0.02
THRESHOLDS = (O.N_TOUCHED_T, O.T_EPS)


def _camera(W, H):
    f = 1.1 * W
    w2c = torch.eye(4, dtype=torch.float64)
    return O.make_settings(w2c, f, f, W / 2.0 + 0.25, H / 2.0 + 0.25, W, H, bg=torch.tensor([0.2, 0.1, 0.3], dtype=torch.float64)), f


def _fp32(t):
    return t.float().double()


def _settings32(s):
    return s._replace(bg=s.bg.float(), viewmatrix=s.viewmatrix.float(), projmatrix=s.projmatrix.float(),
                      projmatrix_raw=s.projmatrix_raw.float(), campos=s.campos.float(),
                      tanfovx=float(torch.tensor(s.tanfovx, dtype=torch.float32)),
                      tanfovy=float(torch.tensor(s.tanfovy, dtype=torch.float32)))


def _blanket_scales(z, f, W, H):
    """Scale per depth: 2D sigma >= 10 image diagonals with 3 sqrt(lambda) = (integer + 0.5) (lambda = sigma^2 + 0.3 + sqrt(0.1))."""
    sig = 10.0 * math.hypot(W, H)
    ext = math.floor(3.0 * math.sqrt(sig * sig + 0.3 + math.sqrt(0.1))) + 0.5
    s2d = math.sqrt((ext / 3.0) ** 2 - 0.3 - math.sqrt(0.1))
    return s2d * z / f


def _pixel_power(pp, ids, W, H):
    """power(pixel, splat) of the oracle's blend for the given splats: [H*W, len(ids)], fp64."""
    py, px = torch.meshgrid(torch.arange(H, dtype=torch.float64), torch.arange(W, dtype=torch.float64), indexing="ij")
    px, py = px.reshape(-1, 1), py.reshape(-1, 1)
    dx = pp.xy[ids, 0].detach()[None, :] - px
    dy = pp.xy[ids, 1].detach()[None, :] - py
    con = pp.conic[ids].detach()
    return -0.5 * (con[:, 0] * dx * dx + con[:, 2] * dy * dy) - con[:, 1] * dx * dy


def _preprocess(inp, s):
    return O.preprocess(inp["means3D"], None, inp["opacities"], inp["shs"], None, inp["scales"], inp["rotations"], None, None, None, s)


def _assign_opacities(inp, s, draw, fixed=None):
    """Opacities in depth order (draw[i] unless a threshold is near, see the module docstring); fixed: {index: opacity}."""
    W, H = int(s.image_width), int(s.image_height)
    pp = _preprocess(inp, s)
    order = torch.argsort(pp.depth.detach().float(), stable=True)
    G = torch.exp(_pixel_power(pp, order, W, H).clamp_max(0.0))          # [P, N] in depth order
    T = torch.ones(H * W, dtype=torch.float64)
    op = draw.clone()
    for j, i in enumerate(order.tolist()):
        o = fixed.get(i, float(draw[i])) if fixed else float(draw[i])
        g = G[:, j]
        live = T >= O.T_EPS
        Tn = T * (1.0 - (o * g).clamp_max(O.ALPHA_MAX))
        for thr in THRESHOLDS:
            near = live & (Tn > thr * (1.0 - JUMP_MARGIN)) & (Tn < thr * (1.0 + JUMP_MARGIN))
            if bool(near.any()):
                assert not (fixed and i in fixed), "a fixed opacity lands next to a threshold"
                need = ((1.0 - thr * (1.0 - JUMP_MARGIN) / T[live]) / g[live]).max().item()
                o = min(0.9, max(o, need) * 1.002)
                Tn = T * (1.0 - (o * g).clamp_max(O.ALPHA_MAX))
                assert not bool((live & (Tn > thr * (1.0 - JUMP_MARGIN)) & (Tn < thr * (1.0 + JUMP_MARGIN))).any())
        op[i] = o
        T = torch.where(T >= O.T_EPS, Tn, T)
    return _fp32(op)


def _rgb_to_sh(rgb):
    return ((rgb - 0.5) / O.SH_C0)[:, None, :]


@functools.lru_cache(maxsize=None)
def blanket_scene(L, W, H):
    """(inputs, settings): fp32-exact fp64 tensors, like gpu_utils.to_fp32_inputs; every 8x8 bin holds exactly L pairs."""
    g = torch.Generator().manual_seed(1000 * L + W)
    s, f = _camera(W, H)
    s = _settings32(s)
    z = 2.0 + 6.0 * (torch.arange(L, dtype=torch.float64) + 0.5) / L
    z = z[torch.randperm(L, generator=g)]
    means = torch.zeros(L, 3, dtype=torch.float64)
    means[:, 2] = z
    sc = torch.tensor([_blanket_scales(float(zz), f, W, H) for zz in z], dtype=torch.float64)
    rgb = 0.1 + 0.8 * torch.rand(L, 3, generator=g, dtype=torch.float64)
    inp = dict(means3D=_fp32(means), means2D=torch.zeros(L, 3, dtype=torch.float64),
               opacities=torch.zeros(L, 1, dtype=torch.float64), shs=_fp32(_rgb_to_sh(rgb)),
               scales=_fp32(sc[:, None].expand(L, 3).contiguous()),
               rotations=_fp32(torch.tensor([1.0, 0.0, 0.0, 0.0], dtype=torch.float64).expand(L, 4).contiguous()),
               theta=torch.zeros(3, dtype=torch.float64), rho=torch.zeros(3, dtype=torch.float64))
    draw = 0.006 + 0.024 * torch.rand(L, generator=g, dtype=torch.float64)
    inp["opacities"] = _assign_opacities(inp, s, draw)[:, None].contiguous()
    return inp, s


@functools.lru_cache(maxsize=None)
def mixed_scene(W=MIXED_IMAGE[0], H=MIXED_IMAGE[1]):
    """(inputs, settings, expected [gy, gx] list lengths): blanket + local stacks, bins in four length regimes."""
    g = torch.Generator().manual_seed(4242)
    s, f = _camera(W, H)
    s = _settings32(s)
    gx, gy = (W + 7) // 8, (H + 7) // 8
    expect = torch.full((gy, gx), MIXED_BLANKET, dtype=torch.int64)
    nb = MIXED_BLANKET
    ns = sum(m for _, _, m in MIXED_STACKS)
    n = nb + ns
    z = 2.0 + 6.0 * (torch.arange(n, dtype=torch.float64) + 0.5) / n
    z = z[torch.randperm(n, generator=g)]
    near = int(torch.argmin(z))
    z[[0, near]] = z[[near, 0]]             # Gaussian 0 (a blanket, opacity 0.6) is the nearest of all
    means = torch.zeros(n, 3, dtype=torch.float64)
    means[:, 2] = z
    sc = torch.zeros(n, dtype=torch.float64)
    for i in range(nb):
        sc[i] = _blanket_scales(float(z[i]), f, W, H)
    cx, cy = W / 2.0 + 0.25, H / 2.0 + 0.25
    k = nb
    for bx, by, m in MIXED_STACKS:
        px, py = 8 * bx + 3.5, 8 * by + 3.5
        zz = z[k:k + m]
        means[k:k + m, 0] = (px - cx + 0.5) * zz / f          # px = f x / z + cx - 0.5
        means[k:k + m, 1] = (py - cy + 0.5) * zz / f
        sc[k:k + m] = 1e-3 * zz / f                           # 2D variance 1e-6 + the 0.3 dilation
        expect[by, bx] += m
        k += m
    rgb = 0.1 + 0.8 * torch.rand(n, 3, generator=g, dtype=torch.float64)
    inp = dict(means3D=_fp32(means), means2D=torch.zeros(n, 3, dtype=torch.float64),
               opacities=torch.zeros(n, 1, dtype=torch.float64), shs=_fp32(_rgb_to_sh(rgb)),
               scales=_fp32(sc[:, None].expand(n, 3).contiguous()),
               rotations=_fp32(torch.tensor([1.0, 0.0, 0.0, 0.0], dtype=torch.float64).expand(n, 4).contiguous()),
               theta=torch.zeros(3, dtype=torch.float64), rho=torch.zeros(3, dtype=torch.float64))
    draw = torch.empty(n, dtype=torch.float64)
    draw[:nb] = 0.006 + 0.024 * torch.rand(nb, generator=g, dtype=torch.float64)
    draw[nb:] = 0.01265                                       # alpha = 1.4 / 255 at the four middle pixels of the bin
    inp["opacities"] = _assign_opacities(inp, s, draw, fixed={0: 0.6})[:, None].contiguous()
    assert bool((inp["opacities"][nb:, 0] == _fp32(torch.tensor(0.01265, dtype=torch.float64))).all()), \
        "a stack member needed a jump: its footprint would no longer be what the docstring says"
    return inp, s, expect


def all_scenes():
    """[(name, inputs, settings, expected [gy, gx] list lengths)] of every blanket scene and the mixed scene."""
    out = []
    for W, H in IMAGES:
        for L in BLANKET_LENGTHS:
            inp, s = blanket_scene(L, W, H)
            out.append(("blanket_L%d_%dx%d" % (L, W, H), inp, s, torch.full(((H + 7) // 8, (W + 7) // 8), L, dtype=torch.int64)))
    inp, s, e = mixed_scene()
    out.append(("mixed_%dx%d" % MIXED_IMAGE, inp, s, e))
    return out


@torch.no_grad()
def bin_list_lengths(inp, s):
    """[gy, gx] per-8x8-bin list lengths from the fp64 oracle's preprocess: the Gaussians whose alpha >= 1/255 (power <= 0) at some
    pixel of the bin that its 16x16 tile rectangle lets it reach."""
    W, H = int(s.image_width), int(s.image_height)
    gx, gy = (W + 7) // 8, (H + 7) // 8
    pp = _preprocess(inp, s)
    vis = torch.nonzero(pp.visible).flatten()
    counts = torch.zeros(gy, gx, dtype=torch.int64)
    py, px = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    px, py = px.reshape(-1), py.reshape(-1)
    binid = (py // 8) * gx + px // 8
    for c0 in range(0, vis.numel(), 512):
        ids = vis[c0:c0 + 512]
        power = _pixel_power(pp, ids, W, H)
        raw = pp.opacity[ids].detach()[None, :] * torch.exp(power.clamp_max(0.0))
        r = pp.rect[ids]
        tx, ty = (px // O.TILE)[:, None], (py // O.TILE)[:, None]
        inrect = (tx >= r[None, :, 0]) & (tx < r[None, :, 2]) & (ty >= r[None, :, 1]) & (ty < r[None, :, 3])
        hit = (power <= 0) & (raw >= O.ALPHA_MIN) & inrect                       # [P, n]
        per_bin = torch.zeros(gy * gx, ids.numel(), dtype=torch.int64).index_add_(0, binid, hit.long()) > 0
        counts += per_bin.sum(dim=1).reshape(gy, gx)
    return counts


def depths_distinct_fp32(inp, s):
    pp = _preprocess(inp, s)
    d = pp.depth.detach().float()[pp.visible]
    return int(torch.unique(d).numel()) == int(d.numel())
