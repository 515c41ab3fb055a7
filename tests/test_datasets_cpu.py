"""splat_slam_amd.config and splat_slam_amd.datasets without a GPU: the config loader on the reference's YAML fixtures, the numpy host path
of the frame preparation bit for bit against the per-pixel oracle of tests/frame_ref.py and against CPU torch's nearest resize, the three
loaders on tiny sequences written with Pillow, and the prefetch thread."""
import os

import numpy as np
import pytest
import torch

import frame_ref as R
from splat_slam_amd import datasets as D
from splat_slam_amd.config import load_config, save_config, update_recursive

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CONFIGS = os.path.join(GOLDEN, "configs")
DEFAULT = os.path.join(CONFIGS, "splat_slam.yaml")


# ---- config loader ------------------------------------------------------------------------------------------------------------------------
def test_load_config_tum_chain():
    cfg = load_config(os.path.join(CONFIGS, "TUM_RGBD", "freiburg1_desk.yaml"), DEFAULT, root=GOLDEN)
    assert cfg["cam"]["H_out"] == 384 and cfg["cam"]["H_edge"] == 8 and cfg["cam"]["W_out"] == 512
    assert cfg["cam"]["distortion"] == [0.2624, -0.9531, -0.0054, 0.0026, 1.1633] == R.TUM_DISTORTION
    assert cfg["dataset"] == "tumrgbd" and cfg["scene"] == "freiburg1_desk"
    assert cfg["data"]["input_folder"] == "rgbd_dataset_freiburg1_desk" and cfg["data"]["dataset_root"] == "datasets/TUM_RGBD"
    # only in splat_slam.yaml: survives the chain
    assert cfg["mapping"]["Training"]["kf_overlap"] == 0.95 and cfg["mapping"]["opt_params"]["feature_lr"] == 0.0025
    # tum.yaml overrides one leaf of tracking.frontend and one of mapping.Calibration; their siblings stay
    import yaml
    with open(DEFAULT) as f:
        base = yaml.safe_load(f)
    assert cfg["tracking"]["frontend"]["keyframe_thresh"] == 3.0 != base["tracking"]["frontend"]["keyframe_thresh"]
    for key, value in base["tracking"]["frontend"].items():
        if key not in ("keyframe_thresh", "radius"):
            assert cfg["tracking"]["frontend"][key] == value, key
    assert cfg["mapping"]["Calibration"]["depth_scale"] == 5000.0


def test_load_config_root_and_cwd(tmp_path, monkeypatch):
    path = os.path.join(CONFIGS, "Replica", "office0.yaml")
    cfg = load_config(path, DEFAULT, root=GOLDEN)
    assert cfg["dataset"] == "replica" and cfg["cam"]["H"] == 680 and cfg["cam"]["W_out"] == 640 and cfg["cam"]["png_depth_scale"] == 6553.5
    assert "distortion" not in cfg["cam"]
    scan = load_config(os.path.join(CONFIGS, "Scannet", "scene0000.yaml"), DEFAULT, root=GOLDEN)
    assert scan["dataset"] == "scannet"
    monkeypatch.chdir(tmp_path)                 # without root the path is relative to the current directory, as in the reference
    with pytest.raises(OSError):
        load_config(path, DEFAULT)
    monkeypatch.chdir(GOLDEN)
    assert load_config(path, DEFAULT) == cfg


def test_update_recursive_and_round_trip(tmp_path):
    dst = {"a": {"b": 1, "c": [1, 2, 3], "d": {"e": 5}}, "k": 1}
    out = update_recursive(dst, {"a": {"c": [9], "d": {"f": 6}}, "k": {"n": 2}, "z": None})
    assert out is dst and dst == {"a": {"b": 1, "c": [9], "d": {"e": 5, "f": 6}}, "k": {"n": 2}, "z": None}
    cfg = load_config(os.path.join(CONFIGS, "TUM_RGBD", "freiburg1_desk.yaml"), DEFAULT, root=GOLDEN)
    save_config(cfg, tmp_path / "saved.yaml")
    # (the merged dict keeps its inherit_from key, as in the reference: the saved file inherits again, and says the same)
    assert load_config(str(tmp_path / "saved.yaml"), root=GOLDEN) == cfg
    plain = {k: v for k, v in cfg.items() if k != "inherit_from"}
    save_config(plain, str(tmp_path / "plain.yaml"))
    assert load_config(str(tmp_path / "plain.yaml")) == plain
    child = tmp_path / "child.yaml"
    child.write_text("inherit_from: plain.yaml\ncam:\n  H_edge: 3\n")
    again = load_config(str(child), root=str(tmp_path))
    assert again["cam"]["H_edge"] == 3 and again["cam"]["W_edge"] == 8 and again["inherit_from"] == "plain.yaml"
    assert {k: v for k, v in again.items() if k not in ("cam", "inherit_from")} == {k: v for k, v in plain.items() if k != "cam"}


# ---- host path against the oracle ---------------------------------------------------------------------------------------------------------------
def host_map(name):
    return None if R.COLOR_CASES[name][6] is None else D.undistortion_map(*R.case_map_args(name))


@pytest.mark.parametrize("name", list(R.COLOR_CASES))
def test_host_color_matches_oracle(name):
    H, W, H_oe, W_oe, H_edge, W_edge, k = R.COLOR_CASES[name]
    ref, inside = R.case_reference(name)
    map_q = host_map(name)
    if k is not None:
        oracle_map = R.case_map(name)
        assert map_q.dtype == np.int32 and np.array_equal(map_q, oracle_map)
        ix, iy = oracle_map[..., 0] >> 5, oracle_map[..., 1] >> 5
        assert oracle_map.min() < 0, "the case must send map coordinates negative"
        assert (ix + 1 >= W).any() and (iy + 1 >= H).any() and (ix < 0).any() and (iy < 0).any(), "the case must sample outside the image"
        assert inside.any() and not inside.all()
    else:
        assert inside.all()
    img = R.case_images(name)
    got4, none = D.frame_prepare_host(img, None, map_q, H_oe, W_oe, H_edge, W_edge)
    got3, _ = D.frame_prepare_host(np.ascontiguousarray(img[..., :3]), None, map_q, H_oe, W_oe, H_edge, W_edge)
    assert none is None and got4.dtype == np.float32 and got4.shape == (2, 3, H_oe - 2 * H_edge, W_oe - 2 * W_edge)
    assert np.array_equal(got4, ref) and np.array_equal(got3, ref)
    assert (got4[1][:, inside] == 1.0).all(), "a constant 255 image stays exactly 1.0 where all taps are inside"
    assert got4.min() >= 0.0 and got4.max() <= 1.0
    if name == "identity":
        assert np.array_equal(got4, np.transpose(img[..., :3], (0, 3, 1, 2)).astype(np.float32) / np.float32(255.0))
    if name == "up":
        for S, Dn in ((H, H_oe), (W, W_oe)):
            taps = [R.ref_tap(j, S, Dn) for j in range(Dn)]
            assert taps[0] == (0, 1, 0) and taps[-1] == (S - 1, S - 1, 0), "both border clamps are hit"
            s0, s1, b = D.resize_taps(S, Dn)
            assert [tuple(int(v) for v in t) for t in zip(s0, s1, b)] == taps
    if name == "half":
        assert all(R.ref_tap(j, H, H_oe) == (2 * j, 2 * j + 1, 1024) for j in range(H_oe))


def test_map_with_four_coefficients_has_no_k3():
    args = R.case_map_args("down_map")
    four = D.undistortion_map(*args[:6], args[6][:4])
    assert np.array_equal(four, D.undistortion_map(*args[:6], args[6][:4] + [0.0]))
    assert np.array_equal(four, R.ref_map(*args[:6], args[6][:4])) and not np.array_equal(four, R.case_map("down_map"))
    with pytest.raises(ValueError):
        D.undistortion_map(*args[:6], [0.1, 0.2, 0.3])


@pytest.mark.parametrize("scale", R.DEPTH_SCALES)
@pytest.mark.parametrize("name", list(R.DEPTH_CASES))
def test_host_depth_matches_torch_nearest(name, scale):
    H, W, H_oe, W_oe, H_edge, W_edge = R.DEPTH_CASES[name]
    depth = R.case_depth(name)
    assert depth.min() == 0 and depth.max() == 65535
    color = np.zeros((1, H, W, 3), dtype=np.uint8)
    _, got = D.frame_prepare_host(color, depth, None, H_oe, W_oe, H_edge, W_edge, scale)
    ref = R.torch_depth(depth, H_oe, W_oe, H_edge, W_edge, scale)
    assert got.dtype == np.float32 and got.shape == ref.shape and np.array_equal(got, ref)


def test_host_path_refuses_bad_sizes():
    img = np.zeros((1, 4, 4, 3), dtype=np.uint8)
    for bad in ((4, 4, 2, 0), (4, 4, 0, 2), (0, 4, 0, 0), (4, 4, -1, 0)):
        with pytest.raises(ValueError):
            D.frame_prepare_host(img, None, None, *bad)
    with pytest.raises(ValueError):
        D.frame_prepare_host(np.zeros((1, 4, 4, 2), dtype=np.uint8), None, None, 4, 4, 0, 0)
    with pytest.raises(ValueError):
        D.frame_prepare_host(img, np.zeros((1, 4, 4), dtype=np.uint16), None, 4, 4, 0, 0, 0.0)


# ---- loaders ------------------------------------------------------------------------------------------------------------------------------------
def expected_item(ds, color_path, depth_path):
    """what stream[i] must hold for these two files: Pillow's decode through the oracle-checked host path"""
    from PIL import Image
    rgb = np.asarray(Image.open(color_path).convert("RGB"))[None]
    depth = np.asarray(Image.open(depth_path)).astype(np.uint16)[None]
    map_q = None if ds.distortion is None else D.undistortion_map(ds.H, ds.W, ds.fx_orig, ds.fy_orig, ds.cx_orig, ds.cy_orig, ds.distortion)
    color, depth = D.frame_prepare_host(rgb, depth, map_q, ds.H_out_with_edge, ds.W_out_with_edge, ds.H_edge, ds.W_edge, ds.png_depth_scale)
    return color, depth[0]


def check_item(ds, i, color_path, depth_path, pose):
    idx, color, depth, got_pose = ds[i]
    assert idx == i
    assert color.dtype == torch.float32 and tuple(color.shape) == (1, 3, ds.H_out, ds.W_out)
    assert depth.dtype == torch.float32 and tuple(depth.shape) == (ds.H_out, ds.W_out)
    assert got_pose.dtype == torch.float32 and tuple(got_pose.shape) == (4, 4)
    assert float(color.min()) >= 0.0 and float(color.max()) <= 1.0
    ref_color, ref_depth = expected_item(ds, color_path, depth_path)
    assert np.array_equal(color.numpy(), ref_color) and np.array_equal(depth.numpy(), ref_depth)
    assert np.array_equal(got_pose.numpy(), pose.astype(np.float32))
    assert torch.equal(ds.get_color(i), color)


def check_intrinsic(ds, cam):
    f32 = np.float32
    sx, sy = f32((cam["W_out"] + 2 * cam["W_edge"]) / cam["W"]), f32((cam["H_out"] + 2 * cam["H_edge"]) / cam["H"])
    want = np.array([f32(cam["fx"]) * sx, f32(cam["fy"]) * sy, f32(cam["cx"]) * sx - f32(cam["W_edge"]), f32(cam["cy"]) * sy - f32(cam["H_edge"])],
                    dtype=np.float32)
    got = ds.get_intrinsic()
    assert got.dtype == torch.float32 and tuple(got.shape) == (4,) and np.array_equal(got.numpy(), want)
    assert [ds.fx, ds.fy, ds.cx, ds.cy] == [float(v) for v in want]
    assert (ds.fx_orig, ds.fy_orig, ds.cx_orig, ds.cy_orig) == (cam["fx"], cam["fy"], cam["cx"], cam["cy"])
    assert ds.H_out_with_edge == cam["H_out"] + 2 * cam["H_edge"] and ds.W_out_with_edge == cam["W_out"] + 2 * cam["W_edge"]
    assert ds.fovx == pytest.approx(2 * np.arctan(ds.W_out / (2 * ds.fx))) and ds.fovy == pytest.approx(2 * np.arctan(ds.H_out / (2 * ds.fy)))


def test_replica_stride_and_max_frames(tmp_path):
    cfg = R.write_replica(tmp_path)
    cfg.update(stride=2, max_frames=9)
    ds = D.get_dataset(cfg, device="cpu", prepare="host", prefetch=0)
    frames = [0, 2, 4, 6, 8]
    assert isinstance(ds, D.Replica) and len(ds) == ds.n_img == 5 and len(ds.poses) == 5 and ds.distortion is None
    assert [os.path.basename(p) for p in ds.color_paths] == [f"frame{k:06d}.jpg" for k in frames]
    assert [os.path.basename(p) for p in ds.depth_paths] == [f"depth{k:06d}.png" for k in frames]
    assert ds.input_folder == os.path.join(str(tmp_path), "room") and ds.png_depth_scale == 5000.0
    for i, k in enumerate(frames):
        assert ds.poses[i].dtype == np.float64 and np.array_equal(ds.poses[i], R.seq_pose(k))
        check_item(ds, i, ds.color_paths[i], ds.depth_paths[i], R.seq_pose(k))
    assert np.allclose(ds.w2c_first_pose @ ds.poses[0], np.eye(4))
    check_intrinsic(ds, cfg["cam"])
    assert len(list(ds)) == 5                       # the sequence protocol ends with IndexError
    with pytest.raises(IndexError):
        ds[5]
    cfg.update(stride=1, max_frames=-1)
    assert len(D.get_dataset(cfg, device="cpu", prepare="host", prefetch=0)) == R.SEQ_N


def test_scannet_numeric_order(tmp_path):
    cfg = R.write_scannet(tmp_path)
    ds = D.get_dataset(cfg, device="cpu", prepare="host", prefetch=0)
    assert isinstance(ds, D.ScanNet) and len(ds) == R.SEQ_N
    assert [os.path.basename(p) for p in ds.color_paths] == [f"{k}.jpg" for k in range(R.SEQ_N)]        # 10 follows 9, not 1
    assert [os.path.basename(p) for p in ds.depth_paths] == [f"{k}.png" for k in range(R.SEQ_N)]
    for k in (0, 1, 2, 9, 10, 11):
        check_item(ds, k, ds.color_paths[k], ds.depth_paths[k], R.seq_pose(k))
    # paths and poses are cut from separately built lists: a missing colour file shifts the paths, not the poses
    os.remove(os.path.join(ds.input_folder, "color", "3.jpg"))
    cfg.update(stride=3)
    ds = D.get_dataset(cfg, device="cpu", prepare="host", prefetch=0)
    assert [os.path.basename(p) for p in ds.color_paths] == ["0.jpg", "4.jpg", "7.jpg", "10.jpg"]
    assert [os.path.basename(p) for p in ds.depth_paths] == ["0.png", "3.png", "6.png", "9.png"]
    assert all(np.array_equal(p, R.seq_pose(k)) for p, k in zip(ds.poses, (0, 3, 6, 9)))


def test_tum_association_thinning_and_poses(tmp_path):
    from scipy.spatial.transform import Rotation
    cfg = R.write_tum(tmp_path)
    ds = D.get_dataset(cfg, device="cpu", prepare="host", prefetch=0)
    assert isinstance(ds, D.TUM_RGBD) and len(ds) == len(R.TUM_KEPT) == 10
    assert [os.path.basename(p) for p in ds.color_paths] == [f"{R.TUM_T_COLOR[k]:.6f}.jpg" for k in R.TUM_KEPT]
    assert [os.path.basename(p) for p in ds.depth_paths] == [f"{R.TUM_T_DEPTH[R.TUM_DEPTH_OF[k]]:.6f}.png" for k in R.TUM_KEPT]
    assert np.array_equal(ds.distortion, np.array(R.TUM_DISTORTION))

    def c2w(k):
        m = np.eye(4)
        m[:3, :3] = Rotation.from_quat(R.tum_quaternion(k)).as_matrix()         # scipy normalises
        m[:3, 3] = R.tum_translation(k)
        return m

    for k in (0, 3, 11):
        assert np.allclose(D.TUM_RGBD.pose_matrix_from_quaternion(np.concatenate([R.tum_translation(k), R.tum_quaternion(k)])), c2w(k),
                           rtol=0, atol=1e-14)
    assert np.array_equal(ds.poses[0], np.eye(4)), "the first pose is exactly the identity"
    first_inv = np.linalg.inv(c2w(R.TUM_KEPT[0]))
    for i, k in enumerate(R.TUM_KEPT):
        assert ds.poses[i].dtype == np.float64 and np.allclose(ds.poses[i], first_inv @ c2w(k), rtol=0, atol=1e-12)
    assert np.array_equal(ds.w2c_first_pose, np.eye(4))
    for i in (0, 4, 7, 9):
        check_item(ds, i, ds.color_paths[i], ds.depth_paths[i], ds.poses[i])
    check_intrinsic(ds, cfg["cam"])
    cfg.update(stride=3, max_frames=8)
    ds = D.get_dataset(cfg, device="cpu", prepare="host", prefetch=0)
    assert [os.path.basename(p) for p in ds.color_paths] == [f"{R.TUM_T_COLOR[k]:.6f}.jpg" for k in R.TUM_KEPT[:8][::3]]


def test_tum_reads_pose_txt_when_there_is_no_groundtruth(tmp_path):
    cfg = R.write_tum(tmp_path)
    folder = os.path.join(str(tmp_path), "desk")
    os.rename(os.path.join(folder, "groundtruth.txt"), os.path.join(folder, "pose.txt"))
    assert len(D.get_dataset(cfg, device="cpu", prepare="host", prefetch=0)) == 10


def test_depth_without_png_extension_raises_type_error(tmp_path):
    cfg = R.write_replica(tmp_path)
    ds = D.get_dataset(cfg, device="cpu", prepare="host", prefetch=0)
    ds.depth_paths[1] = ds.depth_paths[1][:-4] + ".exr"
    with pytest.raises(TypeError):
        ds[1]
    ds.depth_paths[2] = ds.depth_paths[2][:-4]
    with pytest.raises(TypeError):
        ds[2]
    ds.depth_paths[3] = ds.color_paths[3][:-4] + ".png"        # a .png that is not there
    with pytest.raises(TypeError):
        ds[3]
    assert ds[0][2] is not None                 # the stream still reads
    with pytest.raises(ValueError):
        D.get_dataset(cfg, device="cpu", prepare="hip")
    with pytest.raises(ValueError):
        D.get_dataset(cfg, device="cpu", prepare="torch")


# ---- prefetch -----------------------------------------------------------------------------------------------------------------------------------
def test_prefetch_gives_the_same_tensors(tmp_path):
    import threading
    cfg = R.write_tum(tmp_path)
    plain = D.get_dataset(cfg, device="cpu", prepare="host", prefetch=0)
    ahead = D.get_dataset(cfg, device="cpu", prepare="host", prefetch=2)
    n = len(plain)
    order = list(range(n)) + [int(i) for i in np.random.default_rng(3).permutation(n)] + [n - 1, 0, 0, -1, 5, 4, 3]
    before = threading.active_count()
    for i in order:
        a, b = plain[i], ahead[i]
        assert a[0] == b[0] == i % n
        assert torch.equal(a[1], b[1]) and torch.equal(a[2], b[2]) and torch.equal(a[3], b[3])
    assert threading.active_count() == before + 1, "one worker thread, started on first use"
    ahead.depth_paths[6] = ahead.depth_paths[6] + ".bin"       # a decode error in the worker surfaces in the caller, and only there
    with pytest.raises(TypeError):
        ahead[6]
    assert torch.equal(ahead[7][1], plain[7][1])
    ahead.close()
    assert threading.active_count() == before, "close() joins the worker"
    ahead.close()                                   # twice is fine
    assert torch.equal(ahead[2][1], plain[2][1])    # and the stream still reads, without a thread
    assert threading.active_count() == before
    plain.close()
