"""numpy restatement of the per-keyframe panel of csrc/sgr_plot.hip ("Plots"), pixel by pixel, for the tests only.
Integer parts are in integers; the three float expressions (depth / depth_max, global_scale * depth, their difference and its quotient by
the maximum) are fp32 with numpy's separately rounded operations, which restates the kernel's correctly rounded intrinsics bit for bit;
the exposure image clamp(exp(a) render + b, 0, 1) is fp64, and panel() returns how far 255 image stays from an integer so that a test can
hold its inputs to a margin.  The jet and glyph tables come from scripts/gen_plot_tables.py."""
import importlib.util
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MARGIN, CHAR_W, CHAR_H, TITLE_GAP, FONT_SCALE, TEXT = 8, 12, 16, 4, 2, 64
TITLES = ("Ground Truth RGB", "Input Depth", "Diff RGB L1", "Rasterized RGB, PSNR: {:.2f}", "Rasterized Depth, L1: {:.2f}", "Diff Depth L1")
F32 = np.float32


def load_generator():
    spec = importlib.util.spec_from_file_location("gen_plot_tables", os.path.join(ROOT, "scripts", "gen_plot_tables.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


GEN = load_generator()
JET = GEN.jet_table().astype(np.int64)


def panel_size(H, W, s):
    ch, cw = -(-H // s), -(-W // s)
    return 2 * MARGIN + CHAR_H + 2 * (CHAR_H + TITLE_GAP + ch + MARGIN), MARGIN + 3 * (cw + MARGIN)


def smallest_factor(W, limit=640):
    s = 1
    while -(-W // s) > limit:
        s += 1
    return s


def _jet_index(t):
    with np.errstate(all="ignore"):
        v = F32(256) * t.astype(F32)
        return np.where(v >= 255, 255, np.where(v > 0, np.trunc(v), 0)).astype(np.int64)


def _level32(x):
    """(int)(255 clamp(x, 0, 1)) in fp32; fmax / fmin as the device's fmaxf / fminf"""
    return np.trunc(F32(255) * np.fmin(np.fmax(x.astype(F32), F32(0)), F32(1))).astype(np.int64)


def render_levels(render, a, b):
    """levels of clamp(exp(a) render + b, 0, 1) and the distance of 255 image from the nearest integer (of the clamp's bound where the
    clamp acts).  Without exposure the image is the render itself and the level is fp32, as the ground truth's: distance None."""
    if a is None and b is None:
        return _level32(render), None
    raw = np.exp(np.float64(0.0 if a is None else F32(a))) * render.astype(np.float64) + np.float64(0.0 if b is None else F32(b))
    q = 255.0 * raw
    dist = np.where((raw > 0) & (raw < 1), np.abs(q - np.round(q)), np.minimum(np.abs(q), np.abs(q - 255.0)))
    return np.trunc(255.0 * np.clip(raw, 0.0, 1.0)).astype(np.int64), float(dist.min())


def depth_difference(depth, gt_depth, global_scale):
    with np.errstate(all="ignore"):
        e = np.abs(F32(global_scale) * depth.astype(F32) - gt_depth.astype(F32))
    return np.where((depth > 0) & (gt_depth > 0), e, F32(0)).astype(F32)


def source_cells(frame, global_scale, depth_max):
    """the six full-size images [H,W,3] int64 as {(row, col): image}, the two maxima and the conditioning distance"""
    gt, render = np.asarray(frame["gt"], F32), np.asarray(frame["render"], F32)
    d, gd = np.asarray(frame["depth"], F32), np.asarray(frame["gt_depth"], F32)
    white = np.array([255, 255, 255], np.int64)
    lg = _level32(gt)
    lp, dist = render_levels(render, frame.get("a"), frame.get("b"))
    cells = {(0, 0): lg.transpose(1, 2, 0), (1, 0): lp.transpose(1, 2, 0)}
    with np.errstate(all="ignore"):
        for row, x in ((0, gd), (1, (F32(global_scale) * d).astype(F32))):
            fin = np.isfinite(x)
            t = (np.where(fin, x, F32(0)) / F32(depth_max)).astype(F32)
            cells[(row, 1)] = np.where(fin[..., None], JET[_jet_index(t)], white)
    e = np.abs(lg - lp).sum(0)
    m_rgb = int(e.max())
    cells[(0, 2)] = JET[np.minimum(255, 256 * e // m_rgb) if m_rgb else np.zeros_like(e)]
    ed = depth_difference(d, gd, global_scale)
    fin = np.isfinite(ed)
    m_dep = F32(ed[fin].max()) if fin.any() else F32(0)
    with np.errstate(all="ignore"):
        t = (np.where(fin, ed, F32(0)) / m_dep).astype(F32) if m_dep > 0 else np.zeros_like(ed)
    cells[(1, 2)] = np.where(fin[..., None], JET[_jet_index(t)], white)
    return cells, (m_rgb, float(m_dep)), dist


def reduce_cell(img, s):
    """[H,W,3] -> [ceil(H/s), ceil(W/s), 3]: (sum + cnt // 2) // cnt over each s x s block, cnt the pixels that exist"""
    H, W = img.shape[:2]
    rows, cols = np.arange(0, H, s), np.arange(0, W, s)
    total = np.add.reduceat(np.add.reduceat(img, rows, axis=0), cols, axis=1)
    cnt = np.add.reduceat(np.add.reduceat(np.ones((H, W, 1), np.int64), rows, axis=0), cols, axis=1)
    return (total + cnt // 2) // cnt


def clean_text(text):
    """the bytes the panel draws: up to the first NUL, at most TEXT - 1, anything outside 32 .. 126 as '?'"""
    raw = text.encode("latin-1") if isinstance(text, str) else bytes(text)
    raw = raw.split(b"\0")[0][:TEXT - 1]
    return bytes(c if 32 <= c <= 126 else ord("?") for c in raw)


def draw_text(panel, text, y0, x0, x_end):
    for k, code in enumerate(clean_text(text)):
        rows = GEN.glyph_rows(code)
        for gy in range(GEN.GLYPH_H):
            for gx in range(GEN.GLYPH_W):
                if (rows[gy] >> (GEN.GLYPH_W - 1 - gx)) & 1:
                    for dy in range(FONT_SCALE):
                        for dx in range(FONT_SCALE):
                            x = x0 + k * CHAR_W + gx * FONT_SCALE + dx
                            if x < x_end:
                                panel[y0 + gy * FONT_SCALE + dy, x] = 0


def panel(frame, s, global_scale=1.0, depth_max=5.0):
    """frame: dict(render [3,H,W], gt [3,H,W], depth [H,W], gt_depth [H,W], a, b (floats or None), heading, titles (6, cell (r, c) at
    3 r + c)) -> (panel [PH,PW,3] uint8, info: dict(maxima=(rgb, depth), image_margin=distance or None))"""
    H, W = np.asarray(frame["depth"]).shape
    PH, PW = panel_size(H, W, s)
    ch, cw = -(-H // s), -(-W // s)
    out = np.full((PH, PW, 3), 255, np.int64)
    draw_text(out, frame["heading"], MARGIN, MARGIN, PW - MARGIN)
    cells, maxima, dist = source_cells(frame, global_scale, depth_max)
    for r in range(2):
        for c in range(3):
            x0 = MARGIN + c * (cw + MARGIN)
            y0 = 2 * MARGIN + CHAR_H + r * (CHAR_H + TITLE_GAP + ch + MARGIN)
            draw_text(out, frame["titles"][3 * r + c], y0, x0, x0 + cw)
            out[y0 + CHAR_H + TITLE_GAP:y0 + CHAR_H + TITLE_GAP + ch, x0:x0 + cw] = reduce_cell(cells[(r, c)], s)
    assert out.min() >= 0 and out.max() <= 255
    return out.astype(np.uint8), {"maxima": maxima, "image_margin": dist}


# ---- the inputs of the GPU tests' panel cases (tests/test_gpu_plots.py; their conditioning is asserted in tests/test_plots_cpu.py)
# (H, W, s, variant, global_scale): "edges" puts the depth edge values and an empty title into frame 0; "identical" makes frame 0 a
# render equal to its ground truth with equal depths (global_scale 1).  1.25 is exact in fp32.
PANEL_CASES = ((5, 7, 1, "edges", 1.25), (5, 7, 2, "identical", 1.0), (48, 64, 1, "identical", 1.0), (48, 64, 3, "edges", 1.25))
DEPTH_MAX = 5.0
EXPOSURES = ((None, None), (0.3, -0.05), (-0.2, 0.04))
LONG_TITLE = ("a title of the maximum length \xe9 " + "x" * TEXT)[:TEXT - 1]


def lattice_render(rng, shape, a, b):
    """a render whose exposure image sits near (k + 1/2) / 255: the lattice pushed through the inverse exposure, rounded to fp32.  Some
    levels lie outside 0 .. 255 so that the clamp acts, half a level away from its bounds at least."""
    k = rng.integers(-20, 276, size=shape)
    image = (k + 0.5) / 255.0
    return ((image - np.float64(F32(b))) / np.exp(np.float64(F32(a)))).astype(F32)


def case_frames(H, W, variant="edges", global_scale=1.25, seed=0):
    """three frames: the first without exposure, the others with a != 0 and b != 0.  Frame 0 is, by variant, "edges": depths below 0,
    above and exactly depth_max, one NaN and one +inf pixel in either depth, an infinite difference, and an empty title; "identical": the
    render equals the ground truth and the depths agree, so both maxima are 0.  Frame 2 has no pixel where both depths are > 0 and a
    title of the maximum length with a byte >= 128."""
    rng = np.random.default_rng(1000 * H + W + seed)
    frames = []
    for i, (a, b) in enumerate(EXPOSURES):
        gt = rng.random((3, H, W)).astype(F32)
        gt.flat[::7] = 0.0
        gt.flat[3::11] = 1.0
        render = rng.random((3, H, W)).astype(F32) if a is None else lattice_render(rng, (3, H, W), a, b)
        depth = (0.2 + 5.5 * rng.random((H, W))).astype(F32)
        gt_depth = (0.2 + 5.5 * rng.random((H, W))).astype(F32)
        gt_depth.flat[::5] = 0.0
        titles = [t.format(12.3456 + i) for t in TITLES]
        if i == 0 and variant == "edges":
            depth.flat[0], depth.flat[1], depth.flat[2] = -1.0, 7.0, DEPTH_MAX / global_scale      # below 0, above, exactly depth_max
            gt_depth.flat[1], gt_depth.flat[2], gt_depth.flat[3] = -0.5, DEPTH_MAX, 6.5
            depth.flat[4], depth.flat[6] = np.nan, np.inf
            gt_depth.flat[8], gt_depth.flat[9] = np.nan, np.inf
            gt_depth.flat[6] = 1.0                                                                 # inf - 1: an infinite difference
            titles[1] = ""
        if i == 0 and variant == "identical":
            assert global_scale == 1.0
            render, gt_depth = gt.copy(), depth.copy()
        if i == 2:
            depth.flat[::2] = 0.0
            gt_depth.flat[1::2] = 0.0                                                              # never both > 0
            titles[4] = LONG_TITLE
        frames.append(dict(render=render, gt=gt, depth=depth, gt_depth=gt_depth, a=a, b=b, heading=f"frame: video_idx_{i}_kf_idx_{10 * i}",
                           titles=titles))
    return frames
