"""The novel-view evaluation on the MI355X (splat_slam_amd/novel_view.py, csrc/sgr_novel.hip): sgr_exposure_fit against the exactly
summed oracle of tests/novel_view_ref.py within fit_bound plus one fp32 ulp (tests/test_novel_view_cpu.py shows the bound to be under a
quarter of that ulp for every case), the degenerate frames, determinism and batch independence, the argument errors, the recovery of a
known exposure end to end on the synthetic room, and Slam.evaluate(novel_views=2) on the tiny tracker run."""
import math
import types

import numpy as np
import pytest
import torch

import novel_view_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda"
PSNR_TOL = 1e-4                     # dB: what tests/test_gpu_ssim.py holds sgr_render_metrics' PSNR to


def _nat():
    from splat_slam_amd import _native as nat
    return nat, nat.lib()


def hip_fit(render, gt, stream=None):
    """sgr_exposure_fit over [n,C,H,W] device tensors: (ab [n,2] fp32, flags [n] int32), prefilled so that a missing write shows"""
    nat, lib = _nat()
    n, C, H, W = render.shape
    ab = torch.full((n, 2), float("nan"), dtype=torch.float32, device=DEV)
    flags = torch.full((n,), -1, dtype=torch.int32, device=DEV)
    table = (nat.SgrMetricFrame * n)()
    for f in range(n):
        table[f] = nat.SgrMetricFrame(render[f].data_ptr(), gt[f].data_ptr(), None, None, ab[f, 0:].data_ptr(), ab[f, 1:].data_ptr())
    nbytes = lib.sgr_exposure_fit_bytes(n, C, H, W)
    assert nbytes > 0
    scratch = torch.empty(nbytes // 8, dtype=torch.float64, device=DEV)
    ptr = torch.cuda.current_stream().cuda_stream if stream is None else stream.cuda_stream
    nat.check(lib.sgr_exposure_fit(n, table, C, H, W, ab.data_ptr(), flags.data_ptr(), scratch.data_ptr(), nbytes, ptr), "sgr_exposure_fit")
    return ab, flags


def direct_metrics(render, gt, depth=None, gt_depth=None, ab=None, global_scale=1.0):
    """sgr_render_metrics over lists of device tensors: [n,3] fp32; ab [n,2] device fp32 or None (NULL exposure)"""
    nat, lib = _nat()
    n = len(render)
    C, H, W = render[0].shape
    table = (nat.SgrMetricFrame * n)()
    for f in range(n):
        table[f] = nat.SgrMetricFrame(render[f].data_ptr(), gt[f].data_ptr(), nat.ptr(depth[f]) if depth else None,
                                      nat.ptr(gt_depth[f]) if gt_depth else None, None if ab is None else ab[f, 0:].data_ptr(),
                                      None if ab is None else ab[f, 1:].data_ptr())
    nbytes = lib.sgr_ssim_scratch_bytes(n, C, H, W)
    scratch = torch.empty(nbytes // 4 + 1, dtype=torch.float32, device=DEV)
    out = torch.empty((n, 3), dtype=torch.float32, device=DEV)
    nat.check(lib.sgr_render_metrics(n, table, C, H, W, float(global_scale), out.data_ptr(), scratch.data_ptr(), nbytes,
                                     torch.cuda.current_stream().cuda_stream), "sgr_render_metrics")
    return out


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def within_the_bound(a, b, render, gt, what):
    """|a - a_ref| and |b - b_ref| within fit_bound plus one fp32 ulp of the reference value (ab is stored as fp32)"""
    a_ref, b_ref, flag = R.fit_ref(render, gt)
    da, db = R.fit_bound(render, gt)
    err_a, err_b = abs(a - a_ref), abs(b - b_ref)
    print(f"{what}: a {a!r} ref {a_ref!r} err {err_a:.3e} bound {da + R.ulp32(a_ref):.3e}; b {b!r} ref {b_ref!r} err {err_b:.3e} "
          f"bound {db + R.ulp32(b_ref):.3e}")
    assert flag == 0
    assert err_a <= da + R.ulp32(a_ref) and err_b <= db + R.ulp32(b_ref), (what, a, a_ref, b, b_ref)


# ---- 1. the fit against the oracle
@pytest.mark.parametrize("case", R.CASES, ids=R.case_id)
def test_fit_matches_the_oracle_within_its_bound(case):
    render, gt = R.make_case(case)
    ab, flags = hip_fit(dev(render), dev(gt))
    ab, flags = ab.cpu().double().numpy(), flags.cpu().tolist()
    assert flags == [0] * case[1]
    for f in range(case[1]):
        within_the_bound(float(ab[f, 0]), float(ab[f, 1]), render[f], gt[f], f"{R.case_id(case)} frame {f}")


# ---- 2. degenerate frames
def degenerate_frames(C=3, H=16, W=20):
    rng = np.random.default_rng(7)
    r = rng.uniform(0.1, 0.9, size=(C, H, W)).astype(np.float32)
    one = np.zeros_like(r)
    one[1, 5, 7] = 0.5
    const, half = r.copy(), rng.uniform(0.1, 0.9, size=(C, H, W)).astype(np.float32)
    half[:, :, W // 2:] = 0                          # the mask is the left half: the render is constant there and varies outside
    const[:, :, :W // 2] = np.float32(0.37)
    frames = [("m = 0", r, np.zeros_like(r)), ("m = 1", r, one), ("constant on the mask", const, half),
              ("anti-correlated", r, (np.float32(1.0) - r).astype(np.float32))]
    return frames


def test_degenerate_frames_give_the_identity_and_flag_1():
    frames = degenerate_frames()
    for name, r, g in frames:
        assert R.fit_ref(r, g) == (0.0, 0.0, 1), name                            # the oracle's rule agrees
    render, gt = dev(np.stack([f[1] for f in frames])), dev(np.stack([f[2] for f in frames]))
    ab, flags = hip_fit(render, gt)
    assert flags.cpu().tolist() == [1] * len(frames)
    assert bits(ab).tolist() == [[0, 0]] * len(frames)                            # +0.0 exactly, nothing that is not finite
    # a good frame among them keeps its fit
    good = (np.float32(0.5) * frames[0][1] + np.float32(0.25)).astype(np.float32)
    ab2, flags2 = hip_fit(torch.cat([render[:2], render[:1], render[2:]]), torch.cat([gt[:2], dev(good[None]), gt[2:]]))
    assert flags2.cpu().tolist() == [1, 1, 0, 1, 1]
    within_the_bound(float(ab2[2, 0]), float(ab2[2, 1]), frames[0][1], good, "the good frame among degenerate ones")
    # the metrics with these rows' exposure are the metrics without exposure, bit for bit
    lists = [list(render), list(gt)]
    with_ab = direct_metrics(*lists, ab=ab)
    without = direct_metrics(*lists, ab=None)
    assert torch.equal(bits(with_ab), bits(without))
    assert math.isnan(float(without[0, 0])) and all(math.isfinite(float(v)) for v in without[1:, 0])      # m = 0: the reference's 0/0


# ---- 3. determinism and batch independence
@pytest.mark.parametrize("shape", [(3, 31, 33), (3, 64, 65)])
def test_two_calls_any_row_and_a_side_stream_give_the_same_bits(shape):
    render, gt = R.make_case((shape, 16, (1.3, -0.05)))
    other_r, other_g = R.make_case((shape, 16, (0.6, 0.2)), seed=1)
    render, gt, other_r, other_g = dev(render), dev(gt), dev(other_r), dev(other_g)
    ab, flags = hip_fit(render, gt)
    ab_again, flags_again = hip_fit(render, gt)
    assert torch.equal(bits(ab), bits(ab_again)) and torch.equal(flags, flags_again)
    # frame 3 alone (16-byte aligned: its own allocation), and at rows 0, 7 and 15 among other neighbours (an odd frame size leaves
    # the odd rows of a stacked tensor unaligned: the element-by-element path)
    alone, _ = hip_fit(render[3:4].clone(), gt[3:4].clone())
    assert torch.equal(bits(alone[0]), bits(ab[3]))
    mixed_r, mixed_g = other_r.clone(), other_g.clone()
    for row in (0, 7, 15):
        mixed_r[row], mixed_g[row] = render[3], gt[3]
    mixed, mflags = hip_fit(mixed_r, mixed_g)
    assert mflags.cpu().tolist() == [0] * 16
    for row in (0, 7, 15):
        assert torch.equal(bits(mixed[row]), bits(ab[3])), row
    if (shape[0] * shape[1] * shape[2]) % 4:
        assert render[7].data_ptr() % 16 != 0 and render[3:4].clone().data_ptr() % 16 == 0
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ab_side, flags_side = hip_fit(render, gt, stream=side)
    side.synchronize()
    assert torch.equal(bits(ab_side), bits(ab)) and torch.equal(flags_side, flags)


# ---- the map of the end-to-end tests: the synthetic room and the few-view session of tests/test_gpu_mesh.py, at the tiny image size
class ListStream:
    """frame i -> (timestamp, colour, depth, None), as the dataset streams yield"""

    def __init__(self, frames):
        self.frames = frames

    def __len__(self):
        return len(self.frames)

    def __getitem__(self, i):
        color, depth = self.frames[i]
        return float(i), color, depth, None


def rigid_inverse(m):
    out = np.eye(4)
    out[:3, :3] = m[:3, :3].T
    out[:3, 3] = -m[:3, :3].T @ m[:3, 3]
    return out


@pytest.fixture(scope="module")
def room():
    """six mapped orbit views (viewpoints 0, 2, .. 10, their stamps) and three poses between them (frames 1, 3, 5 of a 12-frame
    trajectory), each with its own detached render and depth"""
    from splat_slam_amd import synthetic as syn
    from splat_slam_amd.mapper import PipelineParams
    from splat_slam_amd.renderer import render
    from splat_slam_amd.session import MappingSession
    intr = syn.INTRINSICS["tiny"]
    world = syn.room_parameters(60000, seed=43, device=DEV)
    world["scaling"] = world["scaling"] * 0 + world["scaling"].mean(dim=1, keepdim=True) + 1.6    # opaque surface splats
    world["opacity"] = torch.full_like(world["opacity"], 4.0)
    gm = syn.model_from_parameters(world, device=DEV, knn_fn=lambda p: torch.ones(p.shape[0], device=p.device))
    cams = syn.make_views(world, 6, intr, DEV, seed=5, perturb=False)
    for k, cam in enumerate(cams):                   # exposures as a mapped session leaves them: not zero, the first one included
        cam.exposure_a.data.fill_(0.03 * (k + 1))
        cam.exposure_b.data.fill_(-0.01 * (k + 1))
    bg = torch.zeros(3, device=DEV)
    loop = types.SimpleNamespace(config=syn.DEFAULT_CONFIG, device=DEV, viewpoints={2 * k: c for k, c in enumerate(cams)},
                                 gaussians=gm, background=bg)
    sess = MappingSession(loop, intr)
    H, W = intr["H"], intr["W"]
    c2w = np.tile(np.eye(4), (12, 1, 1))
    renders, rdepths = {}, {}
    for k in range(12):
        w2c = syn.orbit_w2c(k / 2.0, 6).double().numpy()
        c2w[k] = rigid_inverse(w2c)
    c2w = c2w.astype(np.float32).astype(np.float64)  # the trajectory is fp32 (traj_est); the same values go in as a tensor and as fp64
    with torch.no_grad():
        for k in (1, 3, 5):                          # the camera eval_novel_views builds: the fp32 rigid inverse of the fp64 pose
            w2c = torch.from_numpy(rigid_inverse(c2w[k]).astype(np.float32))
            cam = syn.make_camera(k, w2c, intr, torch.zeros(3, H, W, device=DEV), torch.zeros(H, W, device=DEV), DEV)
            pkg = render(cam, gm, PipelineParams(), bg)
            renders[k], rdepths[k] = pkg["render"].detach().contiguous().clone(), pkg["depth"][0].detach().contiguous().clone()
    return types.SimpleNamespace(sess=sess, loop=loop, c2w=torch.from_numpy(c2w.astype(np.float32)).to(DEV), c2w64=c2w, renders=renders,
                                 depths=rdepths, ids=[1, 3, 5], H=H, W=W, kf_stamps=[2.0 * k for k in range(6)])


def stream_of(room, gts):
    frames = [(None, None)] * 12
    for k in room.ids:
        frames[k] = (gts[k], room.depths[k])
    return ListStream(frames)


# ---- 4. argument errors
def test_argument_errors():
    nat, lib = _nat()
    t = torch.zeros(3 * 8 * 8 + 4096, dtype=torch.float32, device=DEV)
    table = (nat.SgrMetricFrame * 17)()
    for f in range(17):
        table[f] = nat.SgrMetricFrame(t.data_ptr(), t.data_ptr(), None, None, None, None)
    for n in (0, 17):
        rc = lib.sgr_exposure_fit(n, table, 3, 8, 8, t[192:].data_ptr(), t[300:].data_ptr(), t[512:].data_ptr(), 4 * (t.numel() - 512), None)
        assert rc == nat.SGR_ERR_INVALID and "exposure_fit" in nat.last_error()
        assert lib.sgr_exposure_fit_bytes(n, 3, 8, 8) == 0
    torch.cuda.synchronize()
    assert float(t.abs().max()) == 0.0               # nothing was launched


def test_eval_novel_views_refuses_an_empty_selection_a_wrong_shape_and_cpu_frames(room):
    from splat_slam_amd.novel_view import eval_novel_views
    gts = {k: room.renders[k] for k in room.ids}
    stream = stream_of(room, gts)
    with pytest.raises(ValueError, match="no frames"):
        eval_novel_views(room.sess, stream, room.c2w, [])
    bad = dict(gts)
    bad[5] = torch.zeros(3, room.H, room.W + 1, device=DEV)
    with pytest.raises(ValueError, match="frame 5"):
        eval_novel_views(room.sess, stream_of(room, bad), room.c2w, room.ids)
    cpu = dict(gts)
    cpu[3] = gts[3].cpu()
    with pytest.raises(RuntimeError, match="GPU tensors"):
        eval_novel_views(room.sess, stream_of(room, cpu), room.c2w, room.ids)
    with pytest.raises(ValueError):
        eval_novel_views(room.sess, stream, room.c2w, [12])


# ---- 5. recovery end to end
G0, B0 = 0.7, 0.1


def test_a_known_exposure_is_recovered_end_to_end(room):
    from splat_slam_amd.novel_view import eval_novel_views
    gts = {k: (G0 * room.renders[k] + B0).contiguous() for k in room.ids}
    clean = all(float(room.renders[k].min()) >= 0.0 and float(room.renders[k].max()) <= 1.0 and float(gts[k].min()) > 0.0
                and float(gts[k].max()) <= 1.0 for k in room.ids)
    if not clean:
        pytest.skip("an element of the render or of the ground truth clamps: the recovery claim does not apply")
    stream = stream_of(room, gts)
    got = eval_novel_views(room.sess, stream, room.c2w, room.ids, exposure="fit")
    assert got["frame_ids"] == room.ids and got["exposure_flags"] == [0, 0, 0]
    for key in ("psnr", "ssim", "depth_l1", "exposure_a", "exposure_b"):
        assert len(got[key]) == 3
    for i, k in enumerate(room.ids):
        r, g = room.renders[k].cpu().numpy(), gts[k].cpu().numpy()
        a, b = got["exposure_a"][i], got["exposure_b"][i]
        within_the_bound(a, b, r, g, f"frame {k}")
        da, db = R.fit_bound(r, g)
        a_ref, b_ref, _ = R.fit_ref(r, g)
        assert da < 0.25 * R.ulp32(a_ref) and db < 0.25 * R.ulp32(b_ref)
        # ... and (log g0, b0) itself: gt = fl(fl(g0 r) + b0) is off the affine map by at most 2^-24 an element (two roundings below 1),
        # which moves the least-squares gain by at most 2^-24 / std(r) (Cauchy-Schwarz) and the bias by 2^-24 + mean(r) times that
        std, mean = float(r.astype(np.float64).std()), float(r.astype(np.float64).mean())
        dg = 2.0 ** -24 / std
        g32, b32 = float(np.float32(G0)), float(np.float32(B0))
        print(f"frame {k}: a - log g0 = {a - math.log(g32):.3e} (bound {dg / g32 + da + R.ulp32(a_ref):.3e}), b - b0 = {b - b32:.3e}")
        assert abs(a - math.log(g32)) <= dg / g32 * 1.01 + da + R.ulp32(a_ref)
        assert abs(b - b32) <= 2.0 ** -24 + mean * dg * 1.01 + db + R.ulp32(b_ref)
        # recovery to about 2^-22 leaves |image - gt| < 1e-5: PSNR inf or >= 100 dB
        assert got["psnr"][i] == math.inf or got["psnr"][i] >= 100.0, got["psnr"]
        assert got["depth_l1"][i] == 0.0                         # the ground-truth depth is the pose's own rendered depth
    assert got["mean_psnr"] == float(np.mean(got["psnr"])) and got["mean_ssim"] == float(np.mean(got["ssim"]))
    # the session's thin wrapper is the same call
    assert room.sess.evaluate_novel_views(stream, room.c2w, room.ids) == got
    # "none": the render as it is, PSNR = 20 log10(1 / rms(gt - render)) over gt > 0 (every element here)
    none = eval_novel_views(room.sess, stream, room.c2w, room.ids, exposure="none")
    assert none["exposure_a"] == [0.0] * 3 and none["exposure_b"] == [0.0] * 3 and none["exposure_flags"] == [0] * 3
    for i, k in enumerate(room.ids):
        r, g = room.renders[k].cpu().numpy().astype(np.float64), gts[k].cpu().numpy().astype(np.float64)
        want = 20.0 * math.log10(1.0 / math.sqrt(float(((np.clip(r, 0, 1) - g) ** 2)[g > 0].mean())))
        print(f"frame {k}: PSNR without exposure {none['psnr'][i]!r}, numpy {want!r}")
        assert abs(none["psnr"][i] - want) <= PSNR_TOL
    direct = direct_metrics([room.renders[k] for k in room.ids], [gts[k] for k in room.ids], [room.depths[k][None] for k in room.ids],
                            [room.depths[k] for k in room.ids])
    assert np.array_equal(np.array([none["psnr"], none["ssim"], none["depth_l1"]]).T, direct.cpu().double().numpy())
    # "keyframes": the interpolated exposure of the mapped keyframes, the first one counting as (0, 0): a direct call, bit for bit
    kf = eval_novel_views(room.loop, stream, room.c2w64, room.ids, exposure="keyframes", global_scale=1.25)
    views = [room.loop.viewpoints[k] for k in sorted(room.loop.viewpoints)]
    ra, rb = R.interpolate_ref(room.kf_stamps, [v.exposure_a.item() for v in views], [v.exposure_b.item() for v in views], room.ids)
    assert ra[0] == 0.5 * views[1].exposure_a.item() and ra[1] != 0.0
    ab = dev(np.stack([ra, rb], axis=1).astype(np.float32))
    direct = direct_metrics([room.renders[k] for k in room.ids], [gts[k] for k in room.ids], [room.depths[k][None] for k in room.ids],
                            [room.depths[k] for k in room.ids], ab=ab, global_scale=1.25)
    assert np.array_equal(np.array([kf["psnr"], kf["ssim"], kf["depth_l1"]]).T, direct.cpu().double().numpy())
    assert np.array_equal(np.array([kf["exposure_a"], kf["exposure_b"]]).T, ab.cpu().double().numpy())
    assert kf == room.sess.evaluate_novel_views(stream, room.c2w, room.ids, exposure="keyframes", global_scale=1.25,
                                                kf_timestamps=room.kf_stamps)
    assert all(d > 0.0 for d in kf["depth_l1"])              # the scale reached the depth error


# ---- 6. Slam.evaluate(novel_views=2)
class HeldOutStream:
    """tests/tracker_cases.SyntheticStream's pattern at half its step a frame, 18 frames.  While `dense` is False the stream shows only
    the frames 0, 1, 3, 5, .. 17, as ten consecutive items with their own stamps: what a tracker is left with after a motion filter
    dropped the others.  Every frame it is shown becomes a keyframe; the even frames from 2 on are the held-out ones."""

    def __init__(self, n_seen, poses, device=DEV):
        import tracker_cases as T
        self.n_seen, self.poses, self.device, self.dense = n_seen, poses, device, False
        self.ht, self.wd = T.HT, T.WD

    def frame_of(self, i):
        return i if self.dense or i == 0 else 2 * i - 1

    def __len__(self):
        return 2 * self.n_seen - 2 if self.dense else self.n_seen

    def __getitem__(self, i):
        if not 0 <= i < len(self):
            raise IndexError(i)
        j = self.frame_of(i)
        y, x = torch.meshgrid(torch.arange(self.ht, dtype=torch.float32), torch.arange(self.wd, dtype=torch.float32), indexing="ij")
        s = 1.5 * j
        img = torch.stack([0.5 + 0.5 * torch.sin(0.31 * (x + s) + 0.11 * y), 0.5 + 0.5 * torch.cos(0.23 * (y - s) + 0.07 * x),
                           0.5 + 0.5 * torch.sin(0.17 * (x + y + s))])
        return float(j), img[None].to(self.device), None, None

    def __iter__(self):
        return (self[i] for i in range(len(self)))

    def get_intrinsic(self):
        return torch.tensor([56.0, 60.0, 32.0, 24.0], device=self.device)


def same(a, b):
    if torch.is_tensor(a):
        return torch.is_tensor(b) and torch.equal(a, b)
    if isinstance(a, np.ndarray):
        return isinstance(b, np.ndarray) and np.array_equal(a, b, equal_nan=True)
    if isinstance(a, dict):
        return isinstance(b, dict) and a.keys() == b.keys() and all(same(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return type(a) is type(b) and len(a) == len(b) and all(same(x, y) for x, y in zip(a, b))
    if isinstance(a, float) and isinstance(b, float) and math.isnan(a) and math.isnan(b):
        return True
    if hasattr(a, "__dict__") and type(a) is type(b):          # an Alignment and its Pairs; a private workspace (_scratch) is no result
        public = lambda o: {k: v for k, v in vars(o).items() if not k.startswith("_")}
        return same(public(a), public(b))
    return a == b


def test_slam_evaluate_scores_every_second_frame_that_is_no_keyframe():
    import test_gpu_slam_evaluate as E
    from splat_slam_amd.droid_net import DroidNet
    from splat_slam_amd.fused import FusedMappingLoop
    from splat_slam_amd.slam import Slam
    cfg = E.make_cfg()
    torch.manual_seed(43)
    np.random.seed(43)
    stream = HeldOutStream(E.N_STREAM, E.smooth_path(2 * E.N_STREAM - 2))
    slam = Slam(cfg, DroidNet.synthetic(7, device=DEV), stream, FusedMappingLoop(cfg, device=DEV), E.mono_depth)
    slam.run()
    slam.terminate()
    n = slam.video.counter.value
    kf_stamps = slam.video.timestamp[:n].tolist()
    assert kf_stamps == [0.0] + [float(2 * i - 1) for i in range(1, E.N_STREAM)] and not slam.session.init
    registered = [float(t) for t in slam.session.keyframe_idxs]                  # the warm-up keyframes never reach the session
    assert registered and set(registered) <= set(kf_stamps) and len(slam.session.loop.viewpoints) >= 2
    stream.dense = True
    plain = slam.evaluate()
    got = slam.evaluate(novel_views=2)
    assert "novel_views" not in plain and "novel_views" in got
    novel = got.pop("novel_views")
    assert got.keys() == plain.keys()
    for k in plain:
        assert same(got[k], plain[k]), k
    want = R.select_ref(len(stream), kf_stamps, every=2)
    assert want == list(range(2, 18, 2)) and novel["frame_ids"] == want
    for key in ("psnr", "ssim", "depth_l1", "exposure_a", "exposure_b", "exposure_flags"):
        assert len(novel[key]) == len(want), key
    assert not {float(i) for i in novel["frame_ids"]} & set(kf_stamps)
    assert all(math.isnan(d) for d in novel["depth_l1"])         # the stream yields no depth: the reference's 0/0
    assert all(f in (0, 1) for f in novel["exposure_flags"]) and all(math.isfinite(v) for v in novel["exposure_a"] + novel["exposure_b"])
    print("novel views:", {k: novel[k] for k in ("frame_ids", "psnr", "ssim", "exposure_a", "exposure_b", "exposure_flags")})
    # the poses are the filled trajectory's, the scale the keyframe alignment's: the same call by hand
    from splat_slam_amd.novel_view import eval_novel_views
    by_hand = eval_novel_views(slam.session, stream, plain["traj_est"], want, exposure="fit", global_scale=plain["global_scale"])
    assert same(by_hand, novel)
    # the other two modes, and without ground-truth poses (the filled trajectory is then computed for this alone)
    assert slam.evaluate(novel_views=2, novel_exposure="none")["novel_views"]["exposure_a"] == [0.0] * len(want)
    loop = slam.session.loop
    views = [loop.viewpoints[k] for k in sorted(loop.viewpoints)]
    stamps = [kf_stamps[k] for k in sorted(loop.viewpoints)]
    ra, rb = R.interpolate_ref(stamps, [v.exposure_a.item() for v in views], [v.exposure_b.item() for v in views], want)
    keyed = slam.evaluate(novel_views=2, novel_exposure="keyframes")["novel_views"]
    assert keyed["exposure_a"] == ra.astype(np.float32).astype(np.float64).tolist()
    assert keyed["exposure_b"] == rb.astype(np.float32).astype(np.float64).tolist() and keyed["exposure_flags"] == [0] * len(want)
    with pytest.raises(ValueError):
        slam.evaluate(novel_views=2, novel_exposure="auto")
    poses, stream.poses = stream.poses, None
    try:
        blind = slam.evaluate(novel_views=2)
    finally:
        stream.poses = poses
    assert blind["traj_est"] is None and blind["novel_views"]["frame_ids"] == want
    assert same(blind["novel_views"], eval_novel_views(slam.session, stream, plain["traj_est"], want, exposure="fit", global_scale=1.0))
    # every candidate a keyframe: nothing to score
    assert slam.evaluate(novel_views=1000)["novel_views"] is None
