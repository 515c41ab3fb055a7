"""fp64 numpy restatement of the four correlation functions of droid_backends, written from their definition (bilinear sample with
zero padding of a (2r+1)^2 window, output index x offset first, then y offset) by gathering the corners of every pixel; never a
loop over the volume.  Every function returns (value, magnitude, terms) per output element:

    value      the result in fp64
    magnitude  the same sum with every product replaced by its absolute value and every corner weight taken as 1
    terms      the number of products summed

A pixel whose floor(x0) or floor(y0) is not finite, or lies outside [-(r+2), w2+r+1] resp. [-(r+2), h2+r+1], is dead: it has no
corner inside the map, so for finite coordinates this is the plain definition, and for NaN / inf it is the defined behaviour."""
import numpy as np

CORNERS = ((0, 0), (1, 0), (0, 1), (1, 1))      # (cx, cy)


def window(x0, y0, r, h2, w2):
    """floor, fractional part and liveness of every pixel (flat arrays)"""
    x0, y0 = np.asarray(x0, np.float64), np.asarray(y0, np.float64)
    with np.errstate(invalid="ignore"):
        fx, fy = np.floor(x0), np.floor(y0)
        live = np.isfinite(fx) & np.isfinite(fy) & (fx >= -(r + 2)) & (fx <= w2 + r + 1) & (fy >= -(r + 2)) & (fy <= h2 + r + 1)
        dx, dy = np.where(live, x0 - fx, 0.0), np.where(live, y0 - fy, 0.0)
    fx, fy = np.where(live, fx, 0.0).astype(np.int64), np.where(live, fy, 0.0).astype(np.int64)
    return fx, fy, dx, dy, live


def weight(dx, dy, cx, cy):
    return (dx if cx else 1.0 - dx) * (dy if cy else 1.0 - dy)


def corr_index_forward(volume, coords, r):
    """volume [B,h1,w1,h2,w2] (any float dtype: elements are widened after the gather), coords [B,2,h1,w1] -> three [B,rd,rd,h1,w1]"""
    B, h1, w1, h2, w2 = volume.shape
    rd, P = 2 * r + 1, B * h1 * w1
    vol = volume.reshape(P, h2 * w2)
    rows = np.arange(P)
    fx, fy, dx, dy, live = window(coords[:, 0].reshape(P), coords[:, 1].reshape(P), r, h2, w2)
    val, mag, cnt = (np.zeros((B, rd, rd, h1, w1)) for _ in range(3))
    for a in range(rd):
        for b in range(rd):
            v, m, c = np.zeros(P), np.zeros(P), np.zeros(P)
            for cx, cy in CORNERS:
                x1, y1 = fx - r + a + cx, fy - r + b + cy
                inb = live & (x1 >= 0) & (x1 < w2) & (y1 >= 0) & (y1 < h2)
                s = np.where(inb, vol[rows, np.where(inb, y1 * w2 + x1, 0)].astype(np.float64), 0.0)
                v += weight(dx, dy, cx, cy) * s
                m += np.abs(s)
                c += inb
            val[:, a, b], mag[:, a, b], cnt[:, a, b] = v.reshape(B, h1, w1), m.reshape(B, h1, w1), c.reshape(B, h1, w1)
    return val, mag, cnt


def corr_index_backward(shape, coords, corr_grad, r):
    """shape of the volume, coords [B,2,h1,w1], corr_grad [B,rd,rd,h1,w1] -> three [B,h1,w1,h2,w2]"""
    B, h1, w1, h2, w2 = shape
    rd, P = 2 * r + 1, B * h1 * w1
    rows = np.arange(P)
    fx, fy, dx, dy, live = window(coords[:, 0].reshape(P), coords[:, 1].reshape(P), r, h2, w2)
    val, mag, cnt = (np.zeros((P, h2 * w2)) for _ in range(3))
    for a in range(rd):
        for b in range(rd):
            g = corr_grad[:, a, b].reshape(P).astype(np.float64)
            for cx, cy in CORNERS:
                x1, y1 = fx - r + a + cx, fy - r + b + cy
                inb = live & (x1 >= 0) & (x1 < w2) & (y1 >= 0) & (y1 < h2)
                p, lin = rows[inb], (y1 * w2 + x1)[inb]         # one element per plane: the pairs (p, lin) are distinct
                val[p, lin] += weight(dx, dy, cx, cy)[inb] * g[inb]
                mag[p, lin] += np.abs(g[inb])
                cnt[p, lin] += 1
    return tuple(t.reshape(shape) for t in (val, mag, cnt))


def _alt_corners(fmap2_b, coords_bn, r):
    """per corner (ix, iy) of the (rd+1)^2 window: flat row index into fmap2[b] and the in-bounds mask, both [rd+1, rd+1, H1*W1]"""
    H2, W2 = fmap2_b.shape[:2]
    fx, fy, dx, dy, live = window(coords_bn[..., 0].reshape(-1), coords_bn[..., 1].reshape(-1), r, H2, W2)
    rc = 2 * r + 2
    lin, inb = np.zeros((rc, rc, fx.size), np.int64), np.zeros((rc, rc, fx.size), bool)
    for ix in range(rc):
        for iy in range(rc):
            x2, y2 = fx - r + ix, fy - r + iy
            inb[ix, iy] = live & (x2 >= 0) & (x2 < W2) & (y2 >= 0) & (y2 < H2)
            lin[ix, iy] = np.where(inb[ix, iy], y2 * W2 + x2, 0)
    return lin, inb, dx, dy


def altcorr_forward(fmap1, fmap2, coords, r):
    """fmap1 [B,H1,W1,C], fmap2 [B,H2,W2,C], coords [B,N,H1,W1,2] -> three [B,N,rd*rd,H1,W1]"""
    B, H1, W1, C = fmap1.shape
    N, rd = coords.shape[1], 2 * r + 1
    f1, f2 = fmap1.astype(np.float64), fmap2.astype(np.float64)
    val, mag, cnt = (np.zeros((B, N, rd * rd, H1 * W1)) for _ in range(3))
    for b in range(B):
        a1, a2 = f1[b].reshape(-1, C), f2[b].reshape(-1, C)
        for n in range(N):
            lin, inb, dx, dy = _alt_corners(f2[b], coords[b, n], r)
            dot, adot = np.zeros(lin.shape), np.zeros(lin.shape)
            for ix in range(rd + 1):
                for iy in range(rd + 1):
                    rows = a2[lin[ix, iy]]
                    dot[ix, iy] = np.where(inb[ix, iy], (a1 * rows).sum(1), 0.0)
                    adot[ix, iy] = np.where(inb[ix, iy], np.abs(a1 * rows).sum(1), 0.0)
            for ax in range(rd):
                for ay in range(rd):
                    for cx, cy in CORNERS:
                        val[b, n, ax * rd + ay] += weight(dx, dy, cx, cy) * dot[ax + cx, ay + cy]
                        mag[b, n, ax * rd + ay] += adot[ax + cx, ay + cy]
                        cnt[b, n, ax * rd + ay] += C * inb[ax + cx, ay + cy]
    return tuple(t.reshape(B, N, rd * rd, H1, W1) for t in (val, mag, cnt))


def altcorr_backward(fmap1, fmap2, coords, corr_grad, r):
    """-> (fmap1_grad, fmap2_grad), each a (value, magnitude, terms) triple in the shape of its feature map"""
    B, H1, W1, C = fmap1.shape
    H2, W2 = fmap2.shape[1:3]
    N, rd = coords.shape[1], 2 * r + 1
    f1, f2 = fmap1.astype(np.float64), fmap2.astype(np.float64)
    cg = corr_grad.astype(np.float64).reshape(B, N, rd * rd, H1 * W1)
    g1 = [np.zeros((B, H1 * W1, C)) for _ in range(3)]
    g2 = [np.zeros((B, H2 * W2, C)) for _ in range(3)]
    for b in range(B):
        a1, a2 = f1[b].reshape(-1, C), f2[b].reshape(-1, C)
        for n in range(N):
            lin, inb, dx, dy = _alt_corners(f2[b], coords[b, n], r)
            for ix in range(rd + 1):
                for iy in range(rd + 1):
                    g, gabs, k = np.zeros(H1 * W1), np.zeros(H1 * W1), np.zeros(H1 * W1)
                    for cx, cy in CORNERS:
                        ax, ay = ix - cx, iy - cy
                        if 0 <= ax < rd and 0 <= ay < rd:
                            g += weight(dx, dy, cx, cy) * cg[b, n, ax * rd + ay]
                            gabs += np.abs(cg[b, n, ax * rd + ay])
                            k += 1
                    m = inb[ix, iy]
                    g, gabs, k = g * m, gabs * m, k * m
                    rows = a2[lin[ix, iy]]
                    g1[0][b] += g[:, None] * rows
                    g1[1][b] += gabs[:, None] * np.abs(rows)
                    g1[2][b] += k[:, None]
                    idx = lin[ix, iy][m]
                    np.add.at(g2[0][b], idx, g[m, None] * a1[m])
                    np.add.at(g2[1][b], idx, gabs[m, None] * np.abs(a1[m]))
                    np.add.at(g2[2][b], idx, np.broadcast_to(k[m, None], (idx.size, C)))
    return tuple(t.reshape(fmap1.shape) for t in g1), tuple(t.reshape(fmap2.shape) for t in g2)


U32 = 2.0 ** -24


def bound(ref, mag, units, half=False):
    """per element: units * 2^-24 * magnitude for an fp32 sum in any order; a half output adds its one final rounding"""
    e = units * U32 * mag
    if half:
        e = e * (1 + 2.0 ** -11) + 2.0 ** -11 * np.abs(ref) + 2.0 ** -25
    return e
