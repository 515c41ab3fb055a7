"""The novel-view evaluation without a GPU: select_frames and interpolate_exposure against their restatements (tests/novel_view_ref.py),
the two entry points of csrc/sgr_novel.hip in the header, the binding and the built library with the ABI version unchanged, their
kernels' code objects (no scratch, no spills, no float atomics, 16-byte loads), the public keywords, and the condition under which
tests/test_gpu_novel_view.py may hold the kernel to one fp32 ulp: fit_bound is under a quarter of that ulp for every case."""
import ctypes
import inspect
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import novel_view_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
KERNELS = ("exposure_sums_kernel", "exposure_solve_kernel")


# ---- select_frames
@pytest.mark.parametrize("num,kf,every,first", [
    (10, list(range(10)), 1, 0),            # every frame a keyframe: nothing is left
    (11, [0, 10], 5, 0),                    # a keyframe at index 0 and one at the last index
    (23, [4, 7.0, 12], 3, 4),               # first > 0, a keyframe on the first candidate, one off the grid
    (6, [2], 50, 1),                        # every larger than the stream
    (6, [1], 50, 1),                        # ... and its only candidate a keyframe
    (0, [], 5, 0),
])
def test_select_frames_is_the_restatement(num, kf, every, first):
    from splat_slam_amd.novel_view import select_frames
    got = select_frames(num, kf, every=every, first=first)
    assert got == R.select_ref(num, kf, every, first)
    assert all(isinstance(i, int) for i in got) and not set(got) & {int(t) for t in kf}


def test_select_frames_known_answers_and_refusals():
    from splat_slam_amd.novel_view import select_frames
    assert select_frames(10, range(10), every=1) == []
    assert select_frames(11, [0, 10]) == [5]
    assert select_frames(23, [4, 7, 12], every=3, first=4) == [10, 13, 16, 19, 22]
    assert select_frames(6, [2], every=50, first=1) == [1]
    assert select_frames(12, []) == [0, 5, 10]
    for bad in (dict(every=0), dict(first=-1)):
        with pytest.raises(ValueError):
            select_frames(5, [], **bad)


# ---- interpolate_exposure
KF_T = [3.0, 10.0, 14.0, 30.0]
KF_A = [0.7, 0.11, -0.2, 0.05]              # the first keyframe's stored values are not zero, and count as zero
KF_B = [-0.3, 0.02, 0.04, -0.01]


@pytest.mark.parametrize("stamps", [
    [10.0, 14.0, 3.0, 30.0],                # equal to a keyframe's stamp
    [0.0, 2.999, 30.001, 1e6],              # before the first and after the last keyframe
    [3.5, 9.0, 11.0, 13.9, 29.0, 6.5],      # inside every interval
])
def test_interpolate_exposure_is_the_restatement(stamps):
    from splat_slam_amd.novel_view import interpolate_exposure
    a, b = interpolate_exposure(KF_T, KF_A, KF_B, stamps)
    ra, rb = R.interpolate_ref(KF_T, KF_A, KF_B, stamps)
    assert a.dtype == np.float64 and b.dtype == np.float64 and a.shape == (len(stamps),)
    assert np.array_equal(a, ra) and np.array_equal(b, rb)


def test_interpolate_exposure_known_answers():
    from splat_slam_amd.novel_view import interpolate_exposure
    a, b = interpolate_exposure(KF_T, KF_A, KF_B, [3.0, 10.0, 14.0, 30.0, 0.0, 99.0, 6.5, 12.0])
    assert a.tolist()[:6] == [0.0, 0.11, -0.2, 0.05, 0.0, 0.05] and b.tolist()[:6] == [0.0, 0.02, 0.04, -0.01, 0.0, -0.01]
    assert a[6] == 0.0 + 0.5 * 0.11 and b[6] == 0.5 * 0.02                        # the first keyframe as (0, 0), not (0.7, -0.3)
    assert a[7] == 0.11 + 0.5 * (-0.2 - 0.11) and b[7] == 0.02 + 0.5 * (0.04 - 0.02)
    # one mapped keyframe only: the identity everywhere, whatever it stores
    a, b = interpolate_exposure([5.0], [0.4], [0.1], [0.0, 5.0, 9.0])
    assert a.tolist() == [0.0] * 3 and b.tolist() == [0.0] * 3
    ra, rb = R.interpolate_ref([5.0], [0.4], [0.1], [0.0, 5.0, 9.0])
    assert ra.tolist() == [0.0] * 3 and rb.tolist() == [0.0] * 3
    # the caller's arrays are left alone
    ka = np.array(KF_A)
    interpolate_exposure(KF_T, ka, KF_B, [4.0])
    assert ka[0] == 0.7
    for bad in (([], [], []), ([1.0, 1.0], [0, 0], [0, 0]), ([1.0, 2.0], [0.0], [0, 0])):
        with pytest.raises(ValueError):
            interpolate_exposure(*bad, [1.0])


# ---- the ABI
def test_the_header_declares_both_entry_points_and_the_abi_version_stays_10():
    from splat_slam_amd import _native as nat
    text = open(nat.HEADER_PATH).read()
    assert "size_t sgr_exposure_fit_bytes(int32_t n, int32_t C, int32_t H, int32_t W);" in text
    assert re.search(r"int sgr_exposure_fit\(int32_t n, const SgrMetricFrame\* frames, int32_t C, int32_t H, int32_t W, float\* ab, "
                     r"int32_t\* flags, void\* scratch,\s+size_t scratch_bytes, void\* stream\);", text)
    assert nat.SGR_ABI_VERSION == 10
    assert nat.SGR_EXPOSURE_FIT_MAX_FRAMES == 16 and nat.SGR_EXPOSURE_FIT_LAUNCHES == 2
    res, args = nat.SIGNATURES["sgr_exposure_fit"]
    assert res is ctypes.c_int and len(args) == 10 and args[1] == ctypes.POINTER(nat.SgrMetricFrame)
    assert args[5] is ctypes.c_void_p and args[6] is ctypes.c_void_p          # ab and flags are device memory
    res, args = nat.SIGNATURES["sgr_exposure_fit_bytes"]
    assert res is ctypes.c_size_t and args == [ctypes.c_int32] * 4


def test_the_built_library_exports_both_functions_and_sizes_its_scratch():
    from splat_slam_amd import _native as nat
    h = ctypes.CDLL(nat.LIB_PATH)
    assert hasattr(h, "sgr_exposure_fit") and hasattr(h, "sgr_exposure_fit_bytes")
    lib = nat.lib()
    assert lib.sgr_abi_version() == 10
    f = lib.sgr_exposure_fit_bytes                 # (no device: a pure host computation)
    assert f(0, 3, 8, 8) == 0 and f(17, 3, 8, 8) == 0 and f(1, 0, 8, 8) == 0 and f(1, 3, 1 << 15, 1 << 15) == 0
    # one 64-byte row of fp64 partials per workgroup of 4096 elements and frame, rounded up to 256 bytes
    assert f(1, 1, 1, 2) == 256 and f(16, 3, 64, 65) == 16 * 4 * 64 and f(16, 3, 480, 640) == 16 * 225 * 64
    # the argument checks come before any launch: they need no device either
    table = (nat.SgrMetricFrame * 1)()
    for n in (0, 17, -1):
        assert lib.sgr_exposure_fit(n, table, 3, 8, 8, 256, 256, 256, 1 << 20, None) == nat.SGR_ERR_INVALID
        assert "exposure_fit" in nat.last_error()
    assert lib.sgr_exposure_fit(1, table, 3, 8, 8, 256, 256, 256, 1 << 20, None) == nat.SGR_ERR_INVALID      # a row without images
    table[0] = nat.SgrMetricFrame(256, 512, None, None, None, None)
    assert lib.sgr_exposure_fit(1, table, 3, 8, 8, 256, 256, 256, 255, None) == nat.SGR_ERR_WORKSPACE
    assert lib.sgr_exposure_fit(1, table, 3, 8, 8, 256, 256, None, 1 << 20, None) == nat.SGR_ERR_WORKSPACE
    assert lib.sgr_exposure_fit(1, table, 3, 8, 8, None, 256, 256, 1 << 20, None) == nat.SGR_ERR_INVALID


# ---- ISA budget
@pytest.fixture(scope="module")
def novel_isa(tmp_path_factory):
    if not (os.path.exists(HIPCC) or shutil.which(HIPCC)):
        pytest.skip("hipcc not available")
    out = str(tmp_path_factory.mktemp("isa") / "novel.s")
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-S", "--cuda-device-only", "-o", out,
                    os.path.join(ROOT, "splat_slam_amd", "csrc", "sgr_novel.hip")], check=True, capture_output=True)
    text = open(out).read()
    meta = {}
    for block in text.split("\n  - ")[1:]:
        m = re.search(r"\.name:\s+(\S+)", block)
        if m and ".private_segment_fixed_size" in block:
            meta[m.group(1)] = block
    return text, meta


def test_both_kernels_have_no_scratch_no_spills_and_no_float_atomics(novel_isa):
    text, meta = novel_isa
    for k in KERNELS:
        names = [n for n in meta if re.search(r"\d%s" % k, n)]
        assert len(names) == 1, (k, sorted(meta))
        block = meta[names[0]]
        scratch = int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", block).group(1))
        spill = int(re.search(r"\.vgpr_spill_count:\s+(\d+)", block).group(1))
        sspill = int(re.search(r"\.sgpr_spill_count:\s+(\d+)", block).group(1))
        assert scratch == 0 and spill == 0 and sspill == 0, (k, scratch, spill, sspill)
    assert len(meta) == len(KERNELS), sorted(meta)
    assert not re.search(r"(global|flat|buffer|ds)_atomic", text)                  # the sums are fixed-order: no atomics at all
    # the images are read 16 bytes a lane, the sums are fp64, and the only LDS is the cross-wave merge (4 waves x 6 sums x 8 bytes)
    assert "global_load_dwordx4" in text and re.search(r"v_(add|fma)_f64", text)
    sums = meta[[n for n in meta if "exposure_sums_kernel" in n][0]]
    assert int(re.search(r"\.group_segment_fixed_size:\s+(\d+)", sums).group(1)) == 4 * 6 * 8


# ---- the public surface
def test_the_public_keywords_and_their_defaults():
    from splat_slam_amd import novel_view, run, traj_eval
    from splat_slam_amd.session import MappingSession
    from splat_slam_amd.slam import Slam
    p = inspect.signature(Slam.evaluate).parameters
    assert p["novel_views"].default is None and p["novel_exposure"].default == "fit"
    assert list(p)[-2:] == ["novel_views", "novel_exposure"]                       # behind the keywords there were
    p = inspect.signature(novel_view.eval_novel_views).parameters
    assert list(p) == ["loop_or_session", "stream", "c2w", "frame_ids", "exposure", "global_scale", "lpips", "kf_timestamps"]
    assert p["exposure"].default == "fit" and p["global_scale"].default == 1.0 and p["lpips"].default is None
    assert novel_view.EXPOSURE_MODES == ("fit", "keyframes", "none")
    p = inspect.signature(novel_view.select_frames).parameters
    assert p["every"].default == 5 and p["first"].default == 0
    assert list(inspect.signature(MappingSession.evaluate_novel_views).parameters)[:4] == ["self", "stream", "c2w", "frame_ids"]
    assert inspect.signature(traj_eval.full_traj_eval).parameters["traj"].default is None and callable(traj_eval.filled_trajectory)
    assert inspect.signature(run.run).parameters["novel_views"].default is None
    with pytest.raises(SystemExit):
        run.main(["--help"])
    with pytest.raises(ValueError):
        novel_view.eval_novel_views(None, None, None, [1], exposure="auto")
    with pytest.raises(ValueError):
        novel_view.eval_novel_views(None, None, None, [])


def test_the_run_flag_is_parsed_and_a_bad_value_is_refused_before_anything_is_loaded(monkeypatch, capsys):
    from splat_slam_amd import run
    with pytest.raises(SystemExit):
        run.main(["--help"])
    assert "--novel_views N" in capsys.readouterr().out
    with pytest.raises(ValueError):
        run.run({}, novel_views=0)


# ---- what the GPU test's tolerance rests on
@pytest.mark.parametrize("case", R.CASES, ids=R.case_id)
def test_fit_bound_is_under_a_quarter_of_an_fp32_ulp_of_the_reference(case):
    render, gt = R.make_case(case)
    (C, H, W), n, _ = case
    assert render.shape == gt.shape == (n, C, H, W) and render.dtype == gt.dtype == np.float32
    assert render.min() >= 0.1 and render.max() <= 0.9 and gt.min() >= 0 and gt.max() <= 1
    for f in range(n):
        assert int((gt[f] == 0).sum()) >= (C * H * W) // 5                        # the mask matters (from 5 elements up)
        a, b, flag = R.fit_ref(render[f], gt[f])
        assert flag == 0
        da, db = R.fit_bound(render[f], gt[f])
        assert da < 0.25 * R.ulp32(a) and db < 0.25 * R.ulp32(b), (f, a, b, da, db)


def test_the_case_list_covers_the_shapes_and_counts_of_the_issue():
    assert {c[0] for c in R.CASES} == set(R.SHAPES) and {c[1] for c in R.CASES} == {1, 16} and len(R.CASES) == 36
    assert all(sum(1 for c in R.CASES if c[0] == s and c[1] == n) == 3 for s in R.SHAPES for n in R.COUNTS)
    # the oracle's degeneracy rule on the four degenerate frames of the GPU test
    r = np.linspace(0.1, 0.9, 24, dtype=np.float32).reshape(3, 2, 4)
    assert R.fit_ref(r, np.zeros_like(r)) == (0.0, 0.0, 1)
    one = np.zeros_like(r)
    one[1, 0, 2] = 0.5
    assert R.fit_ref(r, one) == (0.0, 0.0, 1)
    assert R.fit_ref(np.full_like(r, 0.37), r) == (0.0, 0.0, 1)
    assert R.fit_ref(r, (1.0 - r).astype(np.float32)) == (0.0, 0.0, 1)
    a, b, flag = R.fit_ref(r, (np.float32(0.5) * r + np.float32(0.25)).astype(np.float32))
    assert flag == 0 and abs(a - np.log(0.5)) < 1e-6 and abs(b - 0.25) < 1e-6
