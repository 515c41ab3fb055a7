"""fp64 numpy restatement of the keyframe depth fusion ("Keyframe depth fusion"): what sgr_fuse_prepare and
sgr_fuse_depth compute, stated by its equations.  Inputs are taken as given (the tests hand in what the GPU sees: fp32 values)."""
import numpy as np

ERODE_R = 5                 # chessboard radius of the erosion: five 3 x 3 erosions
FILL_R = 3                  # radius of the fill's window (the reference's inpaintRadius)
OUTLIER = 4.0               # mono > OUTLIER * mean is removed


def mean32(mono):
    """the mean as the kernel rounds it: an fp64 sum, rounded once to fp32"""
    return float(np.float32(np.asarray(mono, float).sum() / mono.size))


def erode(positive):
    """eroded(p) = 1 iff every pixel within chessboard distance ERODE_R of p inside the image is positive"""
    pos = np.asarray(positive, bool)
    H, W = pos.shape
    pad = np.ones((H + 2 * ERODE_R, W + 2 * ERODE_R), bool)
    pad[ERODE_R:-ERODE_R, ERODE_R:-ERODE_R] = pos
    out = np.ones((H, W), bool)
    for dy in range(2 * ERODE_R + 1):
        for dx in range(2 * ERODE_R + 1):
            out &= pad[dy:dy + H, dx:dx + W]
    return out


def _shift(a, dy, dx, fill):
    """b[y, x] = a[y + dy, x + dx], `fill` outside the image"""
    H, W = a.shape
    b = np.full_like(a, fill)
    ys, xs = slice(max(0, -dy), min(H, H - dy)), slice(max(0, -dx), min(W, W - dx))
    yt, xt = slice(max(0, dy), min(H, H + dy)), slice(max(0, dx), min(W, W + dx))
    b[ys, xs] = a[yt, xt]
    return b


def fill(values, known):
    """The passes of the fill.  Returns (values, number of passes, the pass in which each pixel became known; -1: never)."""
    v = np.where(known, np.asarray(values, float), 0.0)
    K = np.asarray(known, bool).copy()
    stamp = np.where(K, 0, -1)
    passes = 0
    while not K.all():
        near = np.zeros_like(K)
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                if dy or dx:
                    near |= _shift(K, dy, dx, False)
        todo = near & ~K
        if not todo.any():
            break
        passes += 1
        num, den = np.zeros_like(v), np.zeros_like(v)
        for dy in range(-FILL_R, FILL_R + 1):               # row-major window order
            for dx in range(-FILL_R, FILL_R + 1):
                if dy or dx:
                    w = 1.0 / (dx * dx + dy * dy)
                    k = _shift(K, dy, dx, False)
                    num += np.where(k, w * _shift(v, dy, dx, 0.0), 0.0)
                    den += np.where(k, w, 0.0)
        v[todo] = num[todo] / den[todo]
        K |= todo
        stamp[todo] = passes
    return v, passes, stamp


def prepare(mono):
    """mono [H,W] -> (mono_filled [H,W] fp64, eroded [H,W] bool, passes P)"""
    m = np.asarray(mono, float).copy()
    m[m > OUTLIER * mean32(mono)] = 0.0
    er = erode(m > 0)
    m[~er] = 0.0
    filled, passes, _ = fill(m, er)
    return filled, er, passes


def fit(mono_filled, disp, valid, eroded):
    """(s, q) minimising sum w (s mono + q - target)^2, w = eroded & valid, target = 1.0f / disp; a zero determinant gives inf / NaN"""
    w = np.asarray(eroded, bool) & np.asarray(valid, bool)
    x = np.asarray(mono_filled, float)[w]
    with np.errstate(divide="ignore", invalid="ignore"):
        y = (np.float32(1.0) / np.asarray(disp, np.float32)[w]).astype(float)
        a00, a01, a11, b0, b1 = (x * x).sum(), x.sum(), float(w.sum()), (x * y).sum(), y.sum()
        det = np.float64(a00 * a11 - a01 * a01)
        return (a11 * b0 - a01 * b1) / det, (-a01 * b0 + a00 * b1) / det


def fuse(mono_filled, disp, valid, eroded, min_valid=100):
    """one frame -> (depth [H,W] fp64, s, q, invalid); s and q are None for an invalid frame"""
    valid = np.asarray(valid, bool)
    with np.errstate(divide="ignore", invalid="ignore"):
        tracker = (np.float32(1.0) / np.asarray(disp, np.float32)).astype(float)
    if valid.sum() < min_valid:
        return np.where(valid, tracker, 0.0), None, None, True
    s, q = fit(mono_filled, disp, valid, eroded)
    with np.errstate(invalid="ignore"):
        return np.where(valid, tracker, s * np.asarray(mono_filled, float) + q), s, q, False
