"""The evaluation's plots and the run entry point without a GPU: csrc/sgr_plot.hip compiles for gfx950 without scratch, spills or float
atomics, its entry points are declared, exported and bound and refuse bad arguments before any launch, the generated tables are up to
date and are the jet map and a usable font, the inputs of the GPU panel cases are well conditioned, plot_trajectory draws what it says
on host stand-ins, and splat_slam_amd.run parses its command line and refuses what it does not implement."""
import ctypes
import os
import re
import shutil
import subprocess
import sys
import types

import numpy as np
import pytest

import plots_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
KERNELS = ("plot_maxima_kernel", "plot_compose_kernel")
ENTRY_POINTS = ("sgr_plot_panel_size", "sgr_plot_scratch_bytes", "sgr_plot_panels")


# ---- ISA budget and ABI
@pytest.fixture(scope="module")
def plot_isa(tmp_path_factory):
    if not (os.path.exists(HIPCC) or shutil.which(HIPCC)):
        pytest.skip("hipcc not available")
    out = str(tmp_path_factory.mktemp("isa") / "plot.s")
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-S", "--cuda-device-only", "-o", out,
                    os.path.join(ROOT, "splat_slam_amd", "csrc", "sgr_plot.hip")], check=True, capture_output=True)
    text = open(out).read()
    meta = {}
    for block in text.split("\n  - ")[1:]:
        m = re.search(r"\.name:\s+(\S+)", block)
        if m and ".private_segment_fixed_size" in block:
            meta[m.group(1)] = block
    return text, meta


def test_every_plot_kernel_has_no_scratch_and_no_spills(plot_isa):
    _, meta = plot_isa
    for k in KERNELS:
        names = [n for n in meta if re.search(r"\d%s" % k, n)]
        assert len(names) == 1, (k, sorted(meta))
        block = meta[names[0]]
        scratch = int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", block).group(1))
        spill = int(re.search(r"\.vgpr_spill_count:\s+(\d+)", block).group(1))
        sspill = int(re.search(r"\.sgpr_spill_count:\s+(\d+)", block).group(1))
        assert scratch == 0 and spill == 0 and sspill == 0, (k, scratch, spill, sspill)
    assert len(meta) == len(KERNELS), sorted(meta)


def test_the_maxima_are_integer_atomics_and_there_is_no_float_atomic(plot_isa):
    text, _ = plot_isa
    assert not re.search(r"(global|flat|buffer|ds)_atomic_\w*(f32|f64|pk_add)", text)
    assert len(re.findall(r"(?:global|flat)_atomic_umax\b", text)) == 2          # the colour sum and the depth difference's bits


def test_plot_entry_points_are_declared_exported_and_bound():
    from splat_slam_amd.build import build_native
    from splat_slam_amd import _native as nat
    path = build_native(verbose=False)
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "splat_hip.h")).read(), flags=re.S)
    h = ctypes.CDLL(path)
    for name in ENTRY_POINTS:
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert hasattr(h, name), name
        assert name in nat.SIGNATURES, name
    lib = nat.lib()
    assert lib.sgr_abi_version() == 10 and nat.SGR_ABI_VERSION == 10
    assert (nat.SGR_PLOT_MAX_FRAMES, nat.SGR_PLOT_LAUNCHES, nat.SGR_PLOT_TEXT) == (16, 2, ref.TEXT)
    assert (nat.SGR_PLOT_MARGIN, nat.SGR_PLOT_CHAR_W, nat.SGR_PLOT_CHAR_H, nat.SGR_PLOT_TITLE_GAP) == (ref.MARGIN, ref.CHAR_W, ref.CHAR_H,
                                                                                                      ref.TITLE_GAP)
    # the six pointers of SgrMetricFrame, then the text: one heading and six titles
    assert [f for f, _ in nat.SgrPlotFrame._fields_][:6] == [f for f, _ in nat.SgrMetricFrame._fields_]
    assert ctypes.sizeof(nat.SgrPlotFrame) == 6 * 8 + 7 * ref.TEXT
    assert nat.SgrPlotFrame.heading.offset == 48 and nat.SgrPlotFrame.titles.offset == 48 + ref.TEXT
    assert lib.sgr_plot_scratch_bytes(0) == 0 and lib.sgr_plot_scratch_bytes(-3) == 0
    assert lib.sgr_plot_scratch_bytes(17) >= 17 * (ctypes.sizeof(nat.SgrPlotFrame) + 8)


def test_the_generated_tables_are_up_to_date():
    script = os.path.join(ROOT, "scripts", "gen_plot_tables.py")
    r = subprocess.run([sys.executable, script, "--check"], capture_output=True, text=True)
    assert r.returncode == 0 and "up to date" in r.stdout, (r.stdout, r.stderr)
    assert open(ref.GEN.OUT).read() == ref.GEN.render()


@pytest.mark.parametrize("H,W,s", [(5, 7, 1), (5, 7, 2), (48, 64, 3), (680, 1200, 2), (480, 640, 1), (1, 1, 9), (16384, 16384, 1)])
def test_panel_size_is_the_restatements(H, W, s):
    from splat_slam_amd import plots
    assert plots.panel_size(H, W, s) == ref.panel_size(H, W, s)


def test_panel_size_refuses_and_the_reduction_factor_is_the_smallest():
    from splat_slam_amd import _native as nat
    from splat_slam_amd import plots
    for H, W, s in ((0, 7, 1), (5, 0, 1), (5, 7, 0), (16385, 7, 1), (5, 7, -2)):
        ph, pw = ctypes.c_int32(-1), ctypes.c_int32(-1)
        nat.lib().sgr_plot_panel_size(H, W, s, ctypes.byref(ph), ctypes.byref(pw))
        assert (ph.value, pw.value) == (0, 0)
        with pytest.raises(ValueError):
            plots.panel_size(H, W, s)
    for W in (1, 64, 639, 640, 641, 1200, 1280, 1281, 16384):
        s = plots.reduction_factor(W)
        assert s == ref.smallest_factor(W) and -(-W // s) <= 640 and (s == 1 or -(-W // (s - 1)) > 640)
    assert plots.reduction_factor(1200) == 2


# ---- tables
JET_13 = {0: (0, 0, 127), 1: (0, 0, 132), 31: (0, 0, 255), 32: (0, 0, 255), 95: (18, 252, 228), 96: (21, 255, 225), 127: (121, 255, 125),
          128: (124, 255, 121), 159: (224, 255, 21), 160: (228, 255, 18), 223: (255, 33, 0), 224: (255, 29, 0), 255: (127, 0, 0)}


def test_the_jet_table_is_jet():
    from splat_slam_amd import plots
    jet = ref.GEN.jet_table()
    assert jet.shape == (256, 3) and jet.dtype == np.uint8
    for i, rgb in JET_13.items():
        assert tuple(int(v) for v in jet[i]) == rgb, i
    assert np.array_equal(plots.jet_table(), jet)                # what plot_trajectory reads out of the generated header
    try:
        from matplotlib import colormaps
    except ImportError:
        return
    assert np.array_equal(jet, colormaps["jet"](np.arange(256), bytes=True)[:, :3])


def test_every_printable_glyph_is_drawn_and_no_two_are_alike():
    g = ref.GEN.glyph_table()
    assert g.shape == (95, ref.GEN.GLYPH_H) and int(g.max()) < 1 << ref.GEN.GLYPH_W
    assert not g[0].any() and all(g[i].any() for i in range(1, 95))
    assert len({tuple(int(v) for v in row) for row in g}) == 95
    assert ref.GEN.glyph_rows(200) == ref.GEN.glyph_rows(ord("?")) == ref.GEN.glyph_rows(7)
    assert ref.CHAR_W >= ref.FONT_SCALE * ref.GEN.GLYPH_W and ref.CHAR_H >= ref.FONT_SCALE * ref.GEN.GLYPH_H


# ---- bad arguments: refused with no device
def test_plot_panels_refuses_bad_arguments_before_any_launch():
    from splat_slam_amd import _native as nat
    lib = nat.lib()
    buf = ctypes.create_string_buffer(4096)
    p = ctypes.addressof(buf)                       # a host address: nothing may be launched on it
    frames = (nat.SgrPlotFrame * 2)()
    for f in frames:
        f.render = f.gt_image = f.depth = f.gt_depth = p
    need = lib.sgr_plot_scratch_bytes(2)
    INV, WS = nat.SGR_ERR_INVALID, nat.SGR_ERR_WORKSPACE
    call = lambda n=2, fr=frames, H=5, W=7, s=1, gs=1.0, dm=5.0, out=p, sc=p, nb=need: lib.sgr_plot_panels(n, fr, H, W, s, gs, dm, out, sc, nb, None)
    assert call(n=0) == INV and "plot_panels" in nat.last_error()
    assert call(n=-1) == INV and call(s=0) == INV and call(s=-1) == INV
    assert call(H=0) == INV and call(W=0) == INV and call(H=16385) == INV and call(fr=None) == INV and call(out=None) == INV
    assert call(dm=0.0) == INV and call(dm=float("nan")) == INV and call(dm=float("inf")) == INV and call(gs=float("inf")) == INV
    assert call(out=p + 1) == INV
    for field in ("render", "gt_image", "depth", "gt_depth"):
        setattr(frames[1], field, None)
        assert call() == INV and "frame 1" in nat.last_error(), field
        setattr(frames[1], field, p)
    assert call(nb=need - 1) == WS and "scratch" in nat.last_error()
    assert call(sc=None) == WS


def test_compose_panels_refuses_host_tensors_and_bad_lists():
    import torch
    from splat_slam_amd import plots
    img, d = torch.zeros(3, 5, 7), torch.zeros(5, 7)
    with pytest.raises(RuntimeError, match="GPU"):
        plots.compose_panels([img], [img], [d], [d], ["h"], [list(ref.TITLES)])
    with pytest.raises(ValueError, match="per frame"):
        plots.compose_panels([img], [img], [d], [d], ["h", "i"], [list(ref.TITLES)])
    with pytest.raises(ValueError, match="per frame"):
        plots.compose_panels([], [], [], [], [], [])


# ---- conditioning of the GPU tests' inputs
@pytest.mark.parametrize("case", ref.PANEL_CASES, ids=lambda c: "%dx%d_s%d_%s" % c[:4])
def test_gpu_panel_inputs_keep_the_exposure_image_away_from_every_level_boundary(case):
    """the fp64 oracle truncates 255 clamp(exp(a) r + b, 0, 1); the kernel's fp32 expf, product and sum are worth under 1e-4 of a level
    there, so inputs that stay 1e-3 from an integer (and from the clamp's two bounds) give the same level.  Every other quantity is
    restated bit for bit and needs no margin."""
    H, W, s, variant, gs = case
    frames = ref.case_frames(H, W, variant, gs)
    assert [f["a"] is None for f in frames] == [True, False, False]
    for f in frames[1:]:
        assert f["a"] != 0 and f["b"] != 0
        _, info = ref.panel(f, s, gs, ref.DEPTH_MAX)
        assert info["image_margin"] >= 1e-3, info
        raw = np.exp(np.float64(np.float32(f["a"]))) * f["render"].astype(np.float64) + np.float64(np.float32(f["b"]))
        assert (raw < 0).any() and (raw > 1).any()                # the clamp acts on both sides
    # what the cases are said to carry
    _, info = ref.panel(frames[0], s, gs, ref.DEPTH_MAX)
    d, gd = frames[0]["depth"], frames[0]["gt_depth"]
    if variant == "identical":
        assert info["maxima"] == (0, 0.0)
    else:
        scaled = np.float32(gs) * d
        assert (scaled[np.isfinite(scaled)] < 0).any() and (scaled[np.isfinite(scaled)] > ref.DEPTH_MAX).any() and (scaled == ref.DEPTH_MAX).any()
        assert (gd == ref.DEPTH_MAX).any() and np.isnan(d).sum() == 1 and np.isposinf(d).sum() == 1
        assert np.isinf(ref.depth_difference(d, gd, gs)).any() and frames[0]["titles"][1] == ""
    assert not ((frames[2]["depth"] > 0) & (frames[2]["gt_depth"] > 0)).any()
    assert ref.panel(frames[2], s, gs, ref.DEPTH_MAX)[1]["maxima"][1] == 0.0
    assert len(ref.LONG_TITLE) == ref.TEXT - 1 and any(ord(c) >= 128 for c in ref.LONG_TITLE) and ref.LONG_TITLE in frames[2]["titles"]
    assert ref.CHAR_W * len(frames[0]["titles"][0]) > -(-W // s) or W > 7          # 5 x 7: the titles are wider than a cell


def test_the_restated_reduction_and_text_are_right_on_cases_done_by_hand():
    img = np.arange(5 * 7 * 3, dtype=np.int64).reshape(5, 7, 3)
    out = ref.reduce_cell(img, 2)
    assert out.shape == (3, 4, 3)
    assert out[0, 0, 0] == (img[0:2, 0:2, 0].sum() + 2) // 4 and out[2, 3, 1] == img[4, 6, 1]         # a full block, the ragged corner
    assert out[2, 0, 2] == (img[4, 0:2, 2].sum() + 1) // 2 and out[0, 3, 0] == (img[0:2, 6, 0].sum() + 1) // 2
    assert np.array_equal(ref.reduce_cell(img, 1), img)
    assert ref.clean_text("ab\0cd") == b"ab" and ref.clean_text("\xe9\x01~") == b"??~" and len(ref.clean_text("x" * 200)) == ref.TEXT - 1
    panel = np.full((20, 40, 3), 255, np.int64)
    ref.draw_text(panel, "I", 2, 3, 40)
    rows = ref.GEN.glyph_rows(ord("I"))
    for gy in range(7):
        for gx in range(5):
            want = 0 if (rows[gy] >> (4 - gx)) & 1 else 255
            assert (panel[2 + 2 * gy:4 + 2 * gy, 3 + 2 * gx:5 + 2 * gx] == want).all()
    clipped = np.full((20, 40, 3), 255, np.int64)
    ref.draw_text(clipped, "MM", 0, 0, 15)
    assert (clipped[:, 15:] == 255).all() and (clipped[:, 12:15] == 0).any()


# ---- plot_trajectory on host stand-ins
class HostPairs:
    """host arrays behind the attributes plot_trajectory reads"""

    def __init__(self, est, ref_pos, valid):
        self.pos = np.stack([np.asarray(est, np.float64), np.asarray(ref_pos, np.float64)], 1)
        self.valid = np.asarray(valid, np.uint8)
        self.n = len(self.valid)

    def errors(self, r=None, t=None, s=1.0):
        x = s * (self.pos[:, 0] @ np.asarray(r).T) + np.asarray(t)
        err = np.linalg.norm(x - self.pos[:, 1], axis=1)
        err[self.valid == 0] = np.nan
        return err, None


def _alignment(est, ref_pos, valid, s=2.0):
    from splat_slam_amd.traj_eval import Alignment
    r = np.array([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])
    return Alignment(r, np.array([0.5, -0.25, 0.0]), s, int(np.sum(valid)), int(len(valid) - np.sum(valid)), HostPairs(est, ref_pos, valid))


def _decode(path):
    from PIL import Image
    with Image.open(path) as im:
        return np.asarray(im.convert("RGB"))


def test_plot_trajectory_draws_the_coloured_estimate_over_the_gray_reference(tmp_path):
    from splat_slam_amd import plots
    est = [(0.0, 0.0, 0.0), (0.5, 0.1, 0.0), (1.0, 0.3, 0.1), (1.5, 0.2, 0.0), (9.0, 9.0, 9.0), (2.0, 0.6, 0.0), (2.5, 0.5, 0.0)]
    valid = np.array([1, 1, 1, 1, 0, 1, 1])                      # six poses count, the fifth is skipped
    al = _alignment(est, np.zeros((7, 3)), valid)
    aligned = al.s * (np.asarray(est) @ al.r_a.T) + al.t_a
    refp = aligned + np.array([(0.9, 0.0, 0), (0.8, 0.1, 0), (0.9, -0.1, 0), (1.0, 0.0, 0), (0, 0, 0), (0.7, 0.1, 0), (0.9, 0.0, 0)])
    al.pairs.pos[:, 1] = refp
    path = str(tmp_path / "kf_traj.png")
    assert plots.plot_trajectory(al, path, "Keyframes traj") == plots.TRAJ_SIZE
    img = _decode(path)
    assert img.shape == (plots.TRAJ_SIZE[1], plots.TRAJ_SIZE[0], 3)
    keep = valid.astype(bool)
    err = np.linalg.norm(aligned - refp, axis=1)[keep]
    idx, lo, hi = plots.segment_colors(err)
    assert len(idx) == 5 and lo == err.min() and hi == err.max() and idx.max() > idx.min()
    _, to_pixel = plots.trajectory_projection(np.concatenate([refp[keep, :2], aligned[keep, :2]]))
    jet = plots.jet_table()
    for k, v in enumerate(aligned[keep]):
        x, y = to_pixel(v)
        adjacent = [tuple(int(c) for c in jet[idx[j]]) for j in (k - 1, k) if 0 <= j < len(idx)]
        assert tuple(int(c) for c in img[y, x]) in adjacent, (k, img[y, x], adjacent)
    for v in refp[keep]:
        x, y = to_pixel(v)
        assert tuple(int(c) for c in img[y, x]) == plots.TRAJ_GRAY
    # the skipped pose is not drawn: its pixel would lie far outside the others' box
    x0, y0, x1, y1 = plots.TRAJ_AREA
    body = img[y0 + 1:y1, x0 + 1:x1]
    assert (body != 255).any(axis=2).sum() < 0.2 * body.shape[0] * body.shape[1]


def test_plot_trajectory_of_one_pose_and_of_no_extent_still_draws(tmp_path):
    from splat_slam_amd import plots
    al = _alignment([(0.3, 0.2, 0.0), (5.0, 5.0, 5.0)], [(1.0, 1.0, 0.0), (0.0, 0.0, 0.0)], np.array([1, 0]))
    path = str(tmp_path / "one.png")
    plots.plot_trajectory(al, path, "one pose")
    img = _decode(path)
    assert img.shape == (plots.TRAJ_SIZE[1], plots.TRAJ_SIZE[0], 3)
    est = al.s * (np.array([0.3, 0.2, 0.0]) @ al.r_a.T) + al.t_a
    scale, to_pixel = plots.trajectory_projection(np.array([[1.0, 1.0], est[:2]]))
    x, y = to_pixel(est)
    assert tuple(int(c) for c in img[y, x]) == tuple(int(c) for c in plots.jet_table()[0])      # minimum = maximum: t = 0
    x, y = to_pixel((1.0, 1.0))
    assert tuple(int(c) for c in img[y, x]) == plots.TRAJ_GRAY
    # an xy extent of 0: every position in one point (the estimate moves along z only); the scale falls back to 1
    n = 4
    al = _alignment([(0.0, 0.0, 0.1 * i) for i in range(n)], [(0.5, -0.25, 0.0)] * n, np.ones(n), s=1.0)
    scale, to_pixel = plots.trajectory_projection(np.tile([[0.5, -0.25]], (2 * n, 1)))
    assert scale == 1.0
    path = str(tmp_path / "flat.png")
    plots.plot_trajectory(al, path, "no extent")
    img = _decode(path)
    x0, y0, x1, y1 = plots.TRAJ_AREA
    assert to_pixel((0.5, -0.25)) == ((x0 + x1) // 2, (y0 + y1) // 2)
    x, y = to_pixel((0.5, -0.25))
    assert tuple(int(c) for c in img[y, x]) in {tuple(int(c) for c in row) for row in plots.jet_table()}


def test_the_trajectory_evaluations_take_plot_and_default_to_none():
    import inspect
    from splat_slam_amd import traj_eval
    from splat_slam_amd.slam import Slam
    for fn in (traj_eval.kf_traj_eval, traj_eval.full_traj_eval):
        assert inspect.signature(fn).parameters["plot"].default is False
    assert inspect.signature(Slam.evaluate).parameters["plots"].default is False
    with pytest.raises(ValueError, match="out_dir"):
        Slam.evaluate(types.SimpleNamespace(stream=types.SimpleNamespace()), plots=True)


# ---- run
def test_main_help_exits_0_and_unsupported_modes_are_refused_before_anything_is_loaded(monkeypatch, capsys):
    from splat_slam_amd import run
    with pytest.raises(SystemExit) as e:
        run.main(["--help"])
    assert e.value.code == 0 and "--lpips-weights" in capsys.readouterr().out

    def never(*a, **kw):
        raise AssertionError("nothing may be loaded or written")

    monkeypatch.setattr(run, "load_droid_net", never)
    monkeypatch.setattr(run, "load_mono_depth", never)
    monkeypatch.setattr(run.config_mod, "save_config", never)
    base = {"setup_seed": 43, "scene": "room", "data": {"output": "/nonexistent/output"}}
    for cfg, name in (({"only_tracking": True}, "only_tracking"), ({"mapping": {"eval_before_final_ba": True}}, "eval_before_final_ba"),
                      ({"mono_prior": {"predict_online": False}}, "predict_online")):
        with pytest.raises(NotImplementedError, match=name):
            run.run({**base, **cfg})
    assert len(run.DEPTH_STATS_LABELS) == 9


def test_setup_seed_seeds_torch_numpy_and_random():
    import random
    import torch
    from splat_slam_amd import run
    run.setup_seed(7)
    a = (torch.rand(1).item(), np.random.rand(), random.random())
    run.setup_seed(7)
    assert a == (torch.rand(1).item(), np.random.rand(), random.random())
