"""The correlation operators of the tracker's factor graph (modules/droid_net/corr.py), forward only, over the kernels of
droid_backends (`sgr_corr_*`, csrc/sgr_corr.hip and csrc/sgr_corr_volume.hip).

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
    FusedCorrBlock(maps [frames,cams,C,h,w] fp16, num_levels=4, radius=3, capacity=64)
        CorrBlock's operator for edges between the frames of one store of maps (DepthVideo.fmaps, kept by reference and read when an
        edge is added; fp32 maps raise TypeError).  One tensor [capacity,h,w,h >> l,w >> l] fp16 per level holds the volumes in slots.
        block.add(ii, jj) computes the new edges' pyramids into free slots with one corr_volume_pyramid launch: source plane
        ii * cams, destination plane jj * cams + (1 if ii == jj and cams > 1 else 0), the stereo rule of FactorGraph.add_factors.
        block[index] keeps the indexed edges (long index, bool mask, or (bool mask, number kept)) and changes the slot list alone.
        Both return the block.  block(coords [1,E,h,w,2]) -> [1,E,num_levels*(2r+1)^2,h,w] fp16 in one corr_index_pyramid_forward
        launch, CorrBlock's layout.  len(block), block.slots (device int64), block.volumes(l) (gathered, for tests).  B = 1.
        The volumes are the same real-valued function as CorrBlock's with fewer roundings: level 0 is one fp32 MFMA sum scaled by
        1/16 and every level is averaged from the fp32 level 0 and rounded to fp16 once, where CorrBlock rounds the maps / 4, the
        matmul result and every pooled level in turn.  At most 4 levels, radius <= 4, C a multiple of 32 up to 1024.

A level whose map would have no pixel left (maps smaller than 2^level) is empty and its
lookups are zeros.  Every tensor lives on the GPU.  Not provided: autograd through any block, a fused multi-level lookup of CorrBlock
itself (FusedCorrBlock has one over its own store), B > 1 in the fused blocks, the S dimension in FusedAltCorrBlock.
"""
import torch
import torch.nn.functional as F

import droid_backends

__all__ = ["CorrBlock", "AltCorrBlock", "FusedAltCorrBlock", "FusedCorrBlock"]


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


class FusedCorrBlock:
    """CorrBlock's volumes in the slots of one store per level.  `add` writes the new edges' pyramids straight into free slots
    (one corr_volume_pyramid launch, no gathered copies of the maps), `block[index]` only shortens the slot list, the call is one
    corr_index_pyramid_forward launch that reads the slots in place.  No volume moves because another edge came or went.

    Free slots are found on the device (the used ones are marked, the first n free are taken in ascending order), so `add` and
    `block[index]` with a long index read nothing back.  A bool mask says how many edges it keeps only on the device: give the count
    along, `block[mask, count]`, as FactorGraph does (it has the count from its own masked lists); a bare `block[mask]` costs one
    host read.  When an `add` does not fit, every level is reallocated to max(2 * capacity, edges needed) slots and the old store
    is copied over once: at the tracker's size (48 x 64 maps, four levels) that is 25.07 MB read and written per slot of the old
    capacity, 1.6 GB each way at 64 slots.  Size the capacity so that it does not happen.
    """

    def __init__(self, maps, num_levels=4, radius=3, capacity=64):
        if not isinstance(maps, torch.Tensor) or maps.dim() != 5:
            raise ValueError(f"FusedCorrBlock: maps must be [frames,cams,C,h,w], got {tuple(getattr(maps, 'shape', ()))}")
        if maps.dtype != torch.float16:
            raise TypeError(f"FusedCorrBlock: maps must be torch.float16, got {maps.dtype}")
        if not 1 <= int(num_levels) <= 4:
            raise ValueError(f"FusedCorrBlock: num_levels must lie in [1, 4], got {num_levels}")
        if int(capacity) < 1:
            raise ValueError(f"FusedCorrBlock: capacity must be positive, got {capacity}")
        self.maps, self.num_levels, self.radius, self.capacity = maps, int(num_levels), int(radius), int(capacity)
        h, w = maps.shape[3:]
        self.levels = [torch.empty((self.capacity, h, w, h >> l, w >> l), dtype=torch.float16, device=maps.device)
                       for l in range(self.num_levels)]
        self.slots = torch.zeros(0, dtype=torch.long, device=maps.device)

    def __len__(self):
        return self.slots.shape[0]

    def _grow(self, need):
        capacity = max(2 * self.capacity, need)
        levels = []
        for old in self.levels:
            new = torch.empty((capacity,) + tuple(old.shape[1:]), dtype=old.dtype, device=old.device)
            new[:self.capacity].copy_(old)
            levels.append(new)
        self.levels, self.capacity = levels, capacity

    def add(self, ii, jj):
        frames, cams, C, h, w = self.maps.shape
        ii, jj = ii.long().reshape(-1), jj.long().reshape(-1)
        n = ii.shape[0]
        if jj.shape[0] != n:
            raise ValueError(f"FusedCorrBlock.add: ii and jj must have the same length, got {n} and {jj.shape[0]}")
        if n == 0:
            return self
        if len(self) + n > self.capacity:
            self._grow(len(self) + n)
        used = torch.zeros(self.capacity, dtype=torch.uint8, device=self.slots.device)
        used.index_fill_(0, self.slots, 1)
        new = torch.sort(used, stable=True).indices[:n].contiguous()          # the free slots come first, in ascending order
        src = ii * cams
        dst = jj * cams + ((ii == jj).long() if cams > 1 else 0)
        droid_backends.corr_volume_pyramid(self.maps.view(frames * cams, C, h, w), src.contiguous(), dst.contiguous(), self.levels, new)
        self.slots = torch.cat([self.slots, new])
        return self

    def __getitem__(self, index):
        count = None
        if isinstance(index, tuple):
            index, count = index
        if index.dtype == torch.bool:
            if count is None:
                self.slots = self.slots[index]
            else:                                                             # the kept positions first, in their order: no host read
                order = torch.sort((~index).to(torch.uint8), stable=True).indices[:int(count)]
                self.slots = self.slots[order]
        else:
            self.slots = self.slots[index.long()]
        return self

    def volumes(self, level):
        """the edges' volumes of one level gathered in edge order, [E, h, w, h >> level, w >> level] (a copy; for tests)"""
        return self.levels[level][self.slots]

    def __call__(self, coords):
        if coords.dim() != 5 or coords.shape[0] != 1:
            raise ValueError(f"FusedCorrBlock: coords must be [1,E,h,w,2], got {tuple(coords.shape)}")
        corr, = droid_backends.corr_index_pyramid_forward(self.levels, self.slots.contiguous(), coords[0].float().contiguous(), self.radius)
        return corr[None]
