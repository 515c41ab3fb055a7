"""sgr_frame_prepare and the dataset streams on the MI355X: the kernel bit for bit against the numpy host path (itself held to the
per-pixel oracle in tests/test_datasets_cpu.py) on every case of tests/frame_ref.py, colour and depth; several frames in one launch;
refused sizes; and TUM_RGBD / Replica streams with prepare="hip" against prepare="host", with and without the prefetch thread."""
import numpy as np
import pytest
import torch

import frame_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda"


def dev(a):
    if a is None:
        return None
    if a.dtype == np.uint16:
        a = a.view(np.int16)
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def host_map(name):
    from splat_slam_amd import datasets as D
    return None if R.COLOR_CASES[name][6] is None else D.undistortion_map(*R.case_map_args(name))


@pytest.mark.parametrize("ps", [3, 4])
@pytest.mark.parametrize("name", list(R.COLOR_CASES))
def test_kernel_color_matches_host_path(name, ps):
    from splat_slam_amd import datasets as D
    _, _, H_oe, W_oe, H_edge, W_edge, _ = R.COLOR_CASES[name]
    img = np.ascontiguousarray(R.case_images(name)[..., :ps])
    map_q = host_map(name)
    want, _ = D.frame_prepare_host(img, None, map_q, H_oe, W_oe, H_edge, W_edge)
    got, none = D.frame_prepare(dev(img), None, dev(map_q), H_oe, W_oe, H_edge, W_edge)
    assert none is None and got.dtype == torch.float32 and tuple(got.shape) == want.shape
    assert np.array_equal(got.cpu().numpy(), want)
    assert np.array_equal(want, R.case_reference(name)[0])            # and both are the oracle's bits


@pytest.mark.parametrize("scale", R.DEPTH_SCALES)
@pytest.mark.parametrize("name", list(R.DEPTH_CASES))
def test_kernel_depth_matches_host_path_and_torch(name, scale):
    from splat_slam_amd import datasets as D
    H, W, H_oe, W_oe, H_edge, W_edge = R.DEPTH_CASES[name]
    depth = R.case_depth(name)
    img = np.random.default_rng(H).integers(0, 256, (1, H, W, 4), dtype=np.uint8)
    want_c, want_d = D.frame_prepare_host(img, depth, None, H_oe, W_oe, H_edge, W_edge, scale)
    got_c, got_d = D.frame_prepare(dev(img), dev(depth), None, H_oe, W_oe, H_edge, W_edge, scale)
    assert np.array_equal(got_d.cpu().numpy(), want_d) and np.array_equal(got_c.cpu().numpy(), want_c)
    assert np.array_equal(want_d, R.torch_depth(depth, H_oe, W_oe, H_edge, W_edge, scale))


def test_three_frames_in_one_call_equal_three_calls():
    from splat_slam_amd import datasets as D
    name = "down_map"
    H, W, H_oe, W_oe, H_edge, W_edge, _ = R.COLOR_CASES[name]
    rng = np.random.default_rng(11)
    img = rng.integers(0, 256, (3, H, W, 4), dtype=np.uint8)
    depth = rng.integers(0, 65536, (3, H, W), dtype=np.uint16)
    map_q = dev(host_map(name))
    img_d, depth_d = dev(img), dev(depth)
    color, dep = D.frame_prepare(img_d, depth_d, map_q, H_oe, W_oe, H_edge, W_edge, 5000.0)
    for k in range(3):
        c1, d1 = D.frame_prepare(img_d[k:k + 1].contiguous(), depth_d[k:k + 1].contiguous(), map_q, H_oe, W_oe, H_edge, W_edge, 5000.0)
        assert torch.equal(color[k:k + 1], c1) and torch.equal(dep[k:k + 1], d1)
    want_c, want_d = D.frame_prepare_host(img, depth, host_map(name), H_oe, W_oe, H_edge, W_edge, 5000.0)
    assert np.array_equal(color.cpu().numpy(), want_c) and np.array_equal(dep.cpu().numpy(), want_d)


def test_invalid_sizes_are_refused_without_a_launch():
    from splat_slam_amd import _native as nat
    assert nat.SGR_FRAME_PREPARE_LAUNCHES == 1
    lib = nat.lib()
    H, W = 8, 8
    img = torch.zeros((1, H, W, 4), dtype=torch.uint8, device=DEV)
    depth = torch.zeros((1, H, W), dtype=torch.int16, device=DEV)
    sentinel = 7.0
    out_c = torch.full((1, 3, 8, 8), sentinel, device=DEV)
    out_d = torch.full((1, 8, 8), sentinel, device=DEV)
    st = torch.cuda.current_stream().cuda_stream

    def call(n=1, color=img.data_ptr(), ps=4, dep=depth.data_ptr(), H=H, W=W, map_q=None, H_oe=8, W_oe=8, H_edge=0, W_edge=0, scale=1.0,
             oc=out_c.data_ptr(), od=out_d.data_ptr()):
        return lib.sgr_frame_prepare(n, color, ps, dep, H, W, map_q, H_oe, W_oe, H_edge, W_edge, scale, oc, od, st)

    bad = [dict(n=0), dict(n=65536), dict(ps=2), dict(ps=5), dict(H=0), dict(W=0), dict(H=16385), dict(W_oe=16385), dict(H_oe=0),
           dict(H_edge=-1), dict(W_edge=4), dict(H_edge=4), dict(color=None), dict(oc=None), dict(dep=None), dict(od=None),
           dict(scale=0.0), dict(scale=-1.0), dict(scale=float("inf")), dict(scale=float("nan")),
           dict(color=img.data_ptr() + 1), dict(map_q=img.data_ptr() + 4), dict(dep=depth.data_ptr() + 1)]
    for kw in bad:
        assert call(**kw) == nat.SGR_ERR_INVALID, kw
        assert nat.last_error().startswith("frame_prepare"), kw
    torch.cuda.synchronize()
    assert bool((out_c == sentinel).all()) and bool((out_d == sentinel).all()), "nothing was launched"
    assert call() == 0 and call(dep=None, od=None) == 0
    torch.cuda.synchronize()
    assert bool((out_c == 0).all()) and bool((out_d == 0).all())


@pytest.fixture(scope="module")
def sequences(tmp_path_factory):
    root = tmp_path_factory.mktemp("frames")
    return {"tum": R.write_tum(root), "replica": R.write_replica(root)}


@pytest.mark.parametrize("prefetch", [0, 2])
@pytest.mark.parametrize("which", ["tum", "replica"])
def test_stream_hip_equals_host(sequences, which, prefetch):
    from splat_slam_amd import datasets as D
    cfg = sequences[which]
    host = D.get_dataset(cfg, device="cpu", prepare="host", prefetch=0)
    hip = D.get_dataset(cfg, device="cuda:0", prepare="hip", prefetch=prefetch)
    assert len(hip) == len(host) == (10 if which == "tum" else R.SEQ_N)
    assert (hip.distortion is not None) == (which == "tum")
    n = len(hip)
    for i in list(range(n)) + [int(v) for v in np.random.default_rng(5).permutation(n)]:
        a, b = host[i], hip[i]
        # Tracker.run's contract: (timestamp, image [1,3,H,W] fp32 in [0,1] on the device, ...)
        assert b[0] == i and b[1].is_cuda and b[1].dtype == torch.float32 and tuple(b[1].shape) == (1, 3, hip.H_out, hip.W_out)
        assert float(b[1].min()) >= 0.0 and float(b[1].max()) <= 1.0
        assert b[2].is_cuda and b[2].dtype == torch.float32 and tuple(b[2].shape) == (hip.H_out, hip.W_out)
        assert torch.equal(b[1].cpu(), a[1]) and torch.equal(b[2].cpu(), a[2]) and torch.equal(b[3], a[3])
    assert torch.equal(hip.get_color(3).cpu(), host[3][1])
    assert torch.equal(hip.get_intrinsic(), host.get_intrinsic()) and tuple(hip.get_intrinsic().shape) == (4,)
    hip.close()
    host.close()


def test_host_preparation_on_a_gpu_device(sequences):
    from splat_slam_amd import datasets as D
    cfg = sequences["tum"]
    a = D.get_dataset(cfg, device="cuda:0", prepare="host", prefetch=1)
    b = D.get_dataset(cfg, device="cuda:0", prepare="hip", prefetch=1)
    for i in (0, 5, 9):
        assert a[i][1].is_cuda and torch.equal(a[i][1], b[i][1]) and torch.equal(a[i][2], b[i][2])
    a.close()
    b.close()
