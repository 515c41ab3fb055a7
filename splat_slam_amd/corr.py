"""The two correlation operators of the tracker's factor graph (modules/droid_net/corr.py), forward only, over the lookups that
droid_backends already has (`sgr_corr_*`, csrc/sgr_corr.hip).  No kernel of its own.

    CorrBlock(fmap1 [B,E,C,h,w], fmap2 [B,E,C,h,w], num_levels=4, radius=3)
        all-pairs correlation of the maps divided by 4 (torch.matmul), averaged down num_levels - 1 times (F.avg_pool2d);
        block(coords [B,E,h,w,2]) -> [B,E,num_levels*(2r+1)^2,h,w]: corr_index_forward at coords / 2^level, levels along the channels.
        block.cat(other) appends other's edges, block[index] keeps the indexed edges; both change the block and return it.
    AltCorrBlock(fmaps [B,N,C,H,W], num_levels=4, radius=3)
        keeps a pyramid of the maps instead of the volumes; block(coords [B,E,H,W,2], ii, jj) -> [B,E,num_levels*(2r+1)^2,H,W]
        correlates frame ii[e] at full resolution with frame jj[e] at every level (altcorr_forward, fp32).
        coords [B,E,H,W,S,2] gives [B,E,num_levels*(2r+1)^2,H,W,S].
    FusedAltCorrBlock(fmaps [1,N,C,H,W], num_levels=4, radius=3)
        the same pyramid, values and dtype, and the same call for coords [1,E,H,W,2]: one altcorr_pyramid_forward launch over every
        level, reading frames ii[e] and jj[e] out of the pyramid through their indices (no gathered copies, no concatenation).  Both
        classes define the same real-valued function; the fp32 sums differ in their order.  At most 4 levels, radius <= 4.

A level whose map would have no pixel left (maps smaller than 2^level) is empty and its
lookups are zeros.  Every tensor lives on the GPU.  Not provided: autograd through any block, a fused multi-level lookup of CorrBlock,
the S dimension in FusedAltCorrBlock.
"""
import torch
import torch.nn.functional as F

import droid_backends

__all__ = ["CorrBlock", "AltCorrBlock", "FusedAltCorrBlock"]


def _halve(maps):
    """2 x 2 average of [n,c,h,w]; a map with a side below 2 leaves an empty one, in which every lookup finds zeros"""
    n, c, h, w = maps.shape
    if h < 2 or w < 2:
        return maps.new_zeros((n, c, h // 2, w // 2))
    return F.avg_pool2d(maps, kernel_size=2, stride=2)


class CorrBlock:
    def __init__(self, fmap1, fmap2, num_levels=4, radius=3):
        if fmap1.dim() != 5 or fmap1.shape != fmap2.shape:
            raise ValueError(f"CorrBlock: fmap1 and fmap2 must both be [B,E,C,h,w], got {tuple(fmap1.shape)} and {tuple(fmap2.shape)}")
        self.num_levels, self.radius = int(num_levels), int(radius)
        B, E, C, h, w = fmap1.shape
        a = fmap1.reshape(B * E, C, h * w) / 4.0
        b = fmap2.reshape(B * E, C, h * w) / 4.0
        corr = torch.matmul(a.transpose(1, 2), b).reshape(B * E * h * w, 1, h, w)
        self.corr_pyramid = []
        for lvl in range(self.num_levels):
            self.corr_pyramid.append(corr.view(B * E, h, w, h // 2 ** lvl, w // 2 ** lvl))
            if lvl + 1 < self.num_levels:
                corr = _halve(corr)

    def __call__(self, coords):
        B, E, h, w, _ = coords.shape
        coords = coords.permute(0, 1, 4, 2, 3).reshape(B * E, 2, h, w)
        out = []
        for lvl, volume in enumerate(self.corr_pyramid):
            corr, = droid_backends.corr_index_forward(volume.contiguous(), (coords / 2 ** lvl).float().contiguous(), self.radius)
            out.append(corr.view(B, E, -1, h, w))
        return torch.cat(out, dim=2)

    def cat(self, other):
        self.corr_pyramid = [torch.cat([a, b], dim=0) for a, b in zip(self.corr_pyramid, other.corr_pyramid)]
        return self

    def __getitem__(self, index):
        self.corr_pyramid = [volume[index] for volume in self.corr_pyramid]
        return self


class AltCorrBlock:
    def __init__(self, fmaps, num_levels=4, radius=3):
        if fmaps.dim() != 5:
            raise ValueError(f"AltCorrBlock: fmaps must be [B,N,C,H,W], got {tuple(fmaps.shape)}")
        self.num_levels, self.radius = int(num_levels), int(radius)
        B, N, C, H, W = fmaps.shape
        fmaps = fmaps.reshape(B * N, C, H, W) / 4.0
        self.pyramid = []
        for lvl in range(self.num_levels):
            self.pyramid.append(fmaps.permute(0, 2, 3, 1).contiguous().view(B, N, H // 2 ** lvl, W // 2 ** lvl, C))
            if lvl + 1 < self.num_levels:
                fmaps = _halve(fmaps)

    def __call__(self, coords, ii, jj):
        squeeze = coords.dim() == 5
        if squeeze:
            coords = coords.unsqueeze(-2)
        B, E, H, W, S, _ = coords.shape
        coords = coords.permute(0, 1, 4, 2, 3, 5)                   # [B,E,S,H,W,2]
        fmap1 = self.pyramid[0][:, ii].reshape(B * E, H, W, -1).float().contiguous()
        out = []
        for lvl, maps in enumerate(self.pyramid):
            fmap2 = maps[:, jj].reshape((B * E,) + tuple(maps.shape[2:])).float().contiguous()
            at = (coords / 2 ** lvl).reshape(B * E, S, H, W, 2).float().contiguous()
            corr, = droid_backends.altcorr_forward(fmap1, fmap2, at, self.radius)
            out.append(corr.view(B, E, S, -1, H, W).permute(0, 1, 3, 4, 5, 2))
        corr = torch.cat(out, dim=2)                                # [B,E,levels*(2r+1)^2,H,W,S]
        if squeeze:
            corr = corr.squeeze(-1)
        return corr.contiguous()


class FusedAltCorrBlock:
    def __init__(self, fmaps, num_levels=4, radius=3):
        if fmaps.dim() != 5:
            raise ValueError(f"FusedAltCorrBlock: fmaps must be [B,N,C,H,W], got {tuple(fmaps.shape)}")
        if fmaps.shape[0] != 1:
            raise ValueError(f"FusedAltCorrBlock: B must be 1, got fmaps {tuple(fmaps.shape)}")
        self.num_levels, self.radius = int(num_levels), int(radius)
        B, N, C, H, W = fmaps.shape
        fmaps = fmaps.reshape(B * N, C, H, W) / 4.0
        self.pyramid = []
        for lvl in range(self.num_levels):
            self.pyramid.append(fmaps.permute(0, 2, 3, 1).contiguous().view(B, N, H // 2 ** lvl, W // 2 ** lvl, C))
            if lvl + 1 < self.num_levels:
                fmaps = _halve(fmaps)

    def __call__(self, coords, ii, jj):
        if coords.dim() != 5:
            raise ValueError(f"FusedAltCorrBlock: coords must be [1,E,H,W,2], got {tuple(coords.shape)}; AltCorrBlock takes [B,E,H,W,S,2]")
        if coords.shape[0] != 1:
            raise ValueError(f"FusedAltCorrBlock: B must be 1, got coords {tuple(coords.shape)}")
        corr, = droid_backends.altcorr_pyramid_forward([maps[0] for maps in self.pyramid], ii.long().contiguous(), jj.long().contiguous(),
                                                       coords[0].float().contiguous(), self.radius)
        return corr[None]
