"""splat_slam_amd.depth_video without a GPU: the numpy restatement (tests/depth_video_ref.py) against the torch composition of the same
formula and against hand-made cases of the lower median, every argument check of the new functions and of DepthVideo (raised on CPU
tensors or wrong shapes before any launch), the item-setter and counter rules, and the properties of the scenes the GPU tests of the
chain rely on."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import depth_video_ref as V


def torch_cvx_upsample(d, mask):
    """the composition the kernel replaces (softmax, unfold, broadcast multiply, sum, permute), in fp64"""
    h, w = d.shape
    m = torch.softmax(mask.view(1, 1, 9, 8, 8, h, w), dim=2)
    up = F.unfold(d.view(1, 1, h, w), kernel_size=(3, 3), padding=(1, 1)).view(1, 1, 9, 1, 1, h, w)
    return torch.sum(m * up, dim=2).permute(0, 4, 2, 5, 3, 1).reshape(8 * h, 8 * w)


# ---- the restatement
@pytest.mark.parametrize("shape", [(5, 7), (3, 3), (6, 4)])
def test_ref_upsampling_equals_the_torch_composition(shape):
    rng = np.random.default_rng(1)
    d = rng.uniform(0.2, 2.0, shape)
    mask = rng.uniform(-8, 8, (576,) + shape)
    ref = V.cvx_upsample(d, mask)
    tor = torch_cvx_upsample(torch.tensor(d), torch.tensor(mask)).numpy()
    assert ref.shape == (8 * shape[0], 8 * shape[1])
    h, w = shape
    for y, x in ((h // 2, w // 2), (0, w // 2), (h - 1, w // 2), (h // 2, 0), (h // 2, w - 1), (0, 0), (h - 1, w - 1)):
        blk = np.s_[8 * y:8 * y + 8, 8 * x:8 * x + 8]
        assert np.abs(ref[blk] - tor[blk]).max() < 1e-12
    assert np.abs(ref - tor).max() < 1e-12


def test_equal_logits_give_the_zero_padded_mean():
    rng = np.random.default_rng(2)
    d = rng.uniform(0.2, 2.0, (4, 6))
    out = V.cvx_upsample(d, np.full((576, 4, 6), 1.5))
    pad = np.zeros((6, 8))
    pad[1:-1, 1:-1] = d
    mean = sum(pad[i:i + 4, j:j + 6] for i in range(3) for j in range(3)) / 9
    np.testing.assert_allclose(out, np.repeat(np.repeat(mean, 8, 0), 8, 1), rtol=0, atol=1e-14)
    assert abs(out[0, 0] - (d[0, 0] + d[0, 1] + d[1, 0] + d[1, 1]) / 9) < 1e-14           # a corner sees five zeros


def _one_frame(depths, counts):
    d = (1.0 / np.asarray(depths, np.float64)).astype(np.float32).reshape(1, 1, -1)
    return d, np.asarray(counts, np.float32).reshape(1, 1, -1)


def test_lower_median_even_odd_empty_ties_and_inf():
    # depths chosen as powers of two and their reciprocals, so 1 / (1 / x) is exact in fp32
    d, c = _one_frame([1, 2, 4, 8, 64], [2, 2, 2, 2, 2])                                 # odd: the median is 4, 3 * 4 = 12
    mask, med = V.mask_from_counts(d, [0], c, 2)
    assert med[0] == 4 and mask.reshape(-1).tolist() == [True, True, True, True, False]
    d, c = _one_frame([1, 2, 4, 8], [2, 3, 2, 6])                                        # even: the LOWER of 2 and 4
    mask, med = V.mask_from_counts(d, [0], c, 2)
    assert med[0] == 2 and mask.reshape(-1).tolist() == [True, True, True, False]
    t = torch.tensor([1.0, 2.0, 4.0, 8.0])
    assert t.nanmedian().item() == 2.0                                                   # ... which is what torch.nanmedian returns
    d, c = _one_frame([1, 2, 4, 8], [1, 0, 1, 1])                                        # no candidate: NaN median, all-zero mask
    mask, med = V.mask_from_counts(d, [0], c, 2)
    assert np.isnan(med[0]) and not mask.any()
    d, c = _one_frame([2, 2, 2, 1, 16, 0.5], [2, 2, 2, 2, 2, 0])                         # ties at the median; a non-candidate below it
    mask, med = V.mask_from_counts(d, [0], c, 2)
    assert med[0] == 2 and mask.reshape(-1).tolist() == [True, True, True, True, False, False]
    d = np.array([[[1.0, 0.5, 0.0, 0.0, 0.0]]], np.float32)                              # depth inf (disparity 0): ordered last
    mask, med = V.mask_from_counts(d, [0], np.full((1, 1, 5), 2, np.float32), 2)
    assert np.isinf(med[0]) and mask.reshape(-1).tolist() == [True, True, False, False, False]
    d = np.array([[[1.0, 0.5, 0.25, 0.0, np.nan]]], np.float32)                          # a NaN depth is no candidate
    mask, med = V.mask_from_counts(d, [0], np.full((1, 1, 5), 2, np.float32), 2)
    assert med[0] == 2 and mask.reshape(-1).tolist() == [True, True, True, False, False]
    d = np.array([[[-1.0, -0.5, 1.0, 0.5, 0.25]]], np.float32)                           # negative depths order below the positive ones
    mask, med = V.mask_from_counts(d, [0], np.full((1, 1, 5), 2, np.float32), 2)
    assert med[0] == 1 and mask.reshape(-1).tolist() == [True, True, True, True, False]


def test_ref_threshold_is_rel_times_the_mean_depth():
    d = np.array([[[0.5, 0.25], [1.0, 2.0]], [[4.0, 4.0], [4.0, 4.0]]], np.float32)
    np.testing.assert_allclose(V.depth_thresh(d, [1, 0], 0.5), [0.5 * 0.25, 0.5 * (2 + 4 + 1 + 0.5) / 4], rtol=1e-7)


# ---- the scenes of the GPU tests of the chain
@pytest.mark.parametrize("shape", list(V.SHAPES))
def test_chain_scenes_have_every_kind_of_pixel_away_from_the_knife_edge(shape):
    import dba_ref as R
    poses, disps, intr = V.chain_scene(shape)
    inds = list(range(len(disps)))
    mask, lo, hi, safe = V.valid_depth_mask(poses, disps, intr, inds, V.REL, V.VISIBLE)
    p, d, K = (np.asarray(a, np.float32).astype(float) for a in (poses, disps, intr))
    counts = R.depth_filter(p, d, K, inds, V.depth_thresh(d, inds, V.REL).astype(np.float32).astype(float))
    dep = V.depths32(d)
    for b in inds:
        assert np.isfinite(lo[b]) and np.isfinite(hi[b]) and lo[b] <= hi[b]               # no empty bracket
        assert safe[b].mean() >= 0.9, (b, safe[b].mean())
        s = safe[b]
        assert (s & mask[b]).sum() > 100
        assert (s & ~mask[b] & (counts[b] < V.VISIBLE)).sum() > 20                         # too few views agree
        far = s & ~mask[b] & (counts[b] >= V.VISIBLE)
        assert far.sum() > 20 and (dep[b][far] > 3 * hi[b]).all()                          # beyond 3 x the median
        assert (dep[b][s & mask[b]] < 3 * lo[b]).all()


# ---- argument checks: everything is raised before a device is touched
def _args(n=4, h=6, w=8, num=2):
    return dict(poses=torch.zeros(n, 7), disps=torch.ones(n, h, w), intr=torch.ones(4), inds=torch.arange(num),
                mask=torch.zeros(num, 576, h, w), counts=torch.zeros(num, h, w), out=torch.zeros(n, h, w, dtype=torch.bool))


def test_functions_refuse_cpu_tensors():
    from splat_slam_amd import depth_video as dv
    a = _args()
    for call in (lambda: dv.cvx_upsample(a["disps"], a["inds"], a["mask"]),
                 lambda: dv.cvx_upsample(a["disps"], a["inds"], a["mask"].half(), out=torch.zeros(4, 48, 64)),
                 lambda: dv.depth_thresh(a["disps"], a["inds"], 0.05),
                 lambda: dv.mask_from_counts(a["disps"], a["inds"], a["counts"], 2, a["out"]),
                 lambda: dv.valid_depth_mask(a["poses"], a["disps"], a["intr"], a["inds"], 0.05, 2, a["out"])):
        with pytest.raises(RuntimeError, match="GPU tensor"):
            call()


def test_functions_check_types_and_shapes():
    from splat_slam_amd import depth_video as dv
    a = _args()
    d, i, m, c, o, p, k = a["disps"], a["inds"], a["mask"], a["counts"], a["out"], a["poses"], a["intr"]
    with pytest.raises(TypeError, match="disps must be a torch.Tensor"):
        dv.cvx_upsample(d.numpy(), i, m)
    with pytest.raises(TypeError, match="disps must be torch.float32"):
        dv.cvx_upsample(d.double(), i, m)
    with pytest.raises(TypeError, match="inds must be torch.int64"):
        dv.cvx_upsample(d, i.int(), m)
    with pytest.raises(TypeError, match="mask must be torch.float16 or torch.float32"):
        dv.cvx_upsample(d, i, m.double())
    with pytest.raises(ValueError, match="disps must have 3 dimensions"):
        dv.depth_thresh(d[0], i, 0.05)
    with pytest.raises(ValueError, match="inds must have 1 dimensions"):
        dv.depth_thresh(d, i[None], 0.05)
    with pytest.raises(ValueError, match="disps must be contiguous"):
        dv.depth_thresh(d.transpose(1, 2), i, 0.05)
    with pytest.raises(ValueError, match=r"mask must be \[len\(inds\),576,h,w\]"):
        dv.cvx_upsample(d, i, m[:1])
    with pytest.raises(ValueError, match=r"mask must be \[len\(inds\),576,h,w\]"):
        dv.cvx_upsample(d, i, torch.zeros(2, 64, 6, 8))
    with pytest.raises(ValueError, match=r"out must be \[N,8h,8w\]"):
        dv.cvx_upsample(d, i, m, out=torch.zeros(4, 6, 8))
    with pytest.raises(TypeError, match="out must be torch.float32"):
        dv.cvx_upsample(d, i, m, out=torch.zeros(4, 48, 64, dtype=torch.float64))
    with pytest.raises(ValueError, match=r"counts must be \[len\(inds\),h,w\]"):
        dv.mask_from_counts(d, i, c[:1], 2, o)
    with pytest.raises(TypeError, match="counts must be torch.float32"):
        dv.mask_from_counts(d, i, c.int(), 2, o)
    with pytest.raises(TypeError, match="out must be torch.bool or torch.uint8"):
        dv.mask_from_counts(d, i, c, 2, o.float())
    with pytest.raises(ValueError, match="out must have the shape of disps"):
        dv.mask_from_counts(d, i, c, 2, o[:2])
    with pytest.raises(ValueError, match=r"poses must be \[N,7\]"):
        dv.valid_depth_mask(torch.zeros(4, 6), d, k, i, 0.05, 2, o)
    with pytest.raises(ValueError, match="must cover the 4 disparity maps"):
        dv.valid_depth_mask(p[:3], d, k, i, 0.05, 2, o)
    with pytest.raises(ValueError, match=r"intrinsics must be \[4\]"):
        dv.valid_depth_mask(p, d, torch.ones(3), i, 0.05, 2, o)
    with pytest.raises(ValueError, match="out must have the shape of disps"):
        dv.valid_depth_mask(p, d, k, i, 0.05, 2, torch.zeros(4, 6, 9, dtype=torch.bool))
    with pytest.raises(ValueError, match="exceed the supported 65535"):
        dv.depth_thresh(d, torch.zeros(65536, dtype=torch.int64), 0.05)


# ---- DepthVideo: state, items, counter
def _video(**kw):
    from splat_slam_amd.depth_video import DepthVideo
    return DepthVideo(16, 24, buffer=6, device="cpu", **kw)


def _item(v, t, with_features=False):
    mono = torch.full((v.ht, v.wd), 2.0)
    mono[3, 3] = 0.0                                    # sampled at [3::8, 3::8]: a hole at coarse pixel (0, 0)
    mono[11, 19] = 4.0
    item = (float(t), torch.full((3, v.ht, v.wd), t, dtype=torch.uint8), torch.tensor([t, 0, 0, 0, 0, 0, 1.0]),
            torch.full((2, 3), 0.5), mono, torch.tensor([10.0, 11.0, 12.0, 8.0]))
    if with_features:
        item += (torch.ones(1, 128, 2, 3).half(), 2 * torch.ones(128, 2, 3).half(), 3 * torch.ones(128, 2, 3).half())
    return item


def test_state_tensors_have_the_reference_shapes_and_dtypes():
    v = _video()
    want = dict(timestamp=((6,), torch.float32), images=((6, 3, 16, 24), torch.uint8), dirty=((6,), torch.bool),
                npc_dirty=((6,), torch.bool), poses=((6, 7), torch.float32), disps=((6, 2, 3), torch.float32),
                zeros=((6, 2, 3), torch.float32), disps_up=((6, 16, 24), torch.float32), intrinsics=((6, 4), torch.float32),
                mono_disps=((6, 2, 3), torch.float32), depth_scale=((6,), torch.float32), depth_shift=((6,), torch.float32),
                valid_depth_mask=((6, 16, 24), torch.bool), valid_depth_mask_small=((6, 2, 3), torch.bool),
                fmaps=((6, 1, 128, 2, 3), torch.float16), nets=((6, 128, 2, 3), torch.float16), inps=((6, 128, 2, 3), torch.float16))
    for name, (shape, dtype) in want.items():
        t = getattr(v, name)
        assert tuple(t.shape) == shape and t.dtype == dtype, name
    assert torch.equal(v.poses, torch.tensor([0, 0, 0, 0, 0, 0, 1.0]).expand(6, 7)) and (v.disps == 1).all()
    assert v.down_scale == 8 and v.counter.value == 0 and not v.dirty.any()
    with v.get_lock():
        pass


def test_constructor_checks():
    from splat_slam_amd.depth_video import DepthVideo
    for ht, wd in ((20, 24), (16, 30), (0, 8)):
        with pytest.raises(ValueError, match="multiples of 8"):
            DepthVideo(ht, wd, device="cpu")
    with pytest.raises(ValueError, match="buffer"):
        DepthVideo(16, 24, buffer=0, device="cpu")
    with pytest.raises(NotImplementedError, match="BA_type"):
        DepthVideo(16, 24, device="cpu", BA_type="MoBA")


def test_from_config_reads_the_reference_keys():
    from splat_slam_amd.depth_video import DepthVideo
    cfg = {"cam": {"H_out": 16, "W_out": 32}, "device": "cpu",
           "tracking": {"buffer": 5, "mono_thres": 0.2, "backend": {"BA_type": "DBA"}, "multiview_filter": {"thresh": 0.03, "visible_num": 3}}}
    v = DepthVideo.from_config(cfg)
    assert (v.ht, v.wd, v.BA_type, v.mono_thres, v.filter_thresh, v.filter_visible_num) == (16, 32, "DBA", 0.2, 0.03, 3)
    assert v.disps.shape == (5, 2, 4) and v.device == torch.device("cpu")


def test_item_setter_counter_rules_and_negative_indexing():
    v = _video()
    v.append(*_item(v, 1))
    assert v.counter.value == 1
    v[1] = _item(v, 2, with_features=True)
    assert v.counter.value == 2
    v[0] = _item(v, 3)                                   # below the counter: it stays
    assert v.counter.value == 2 and v.timestamp[0] == 3 and v.images[0, 0, 0, 0] == 3 and v.poses[0, 0] == 3
    assert (v.disps[1] == 0.5).all() and torch.equal(v.intrinsics[1], torch.tensor([10.0, 11.0, 12.0, 8.0]))
    want = torch.full((2, 3), 0.5)
    want[0, 0], want[1, 2] = 0.0, 0.25                  # 1 / d where d > 0, else 0; sampled at [3::8, 3::8]
    assert torch.equal(v.mono_disps[1], want)
    assert (v.fmaps[1] == 1).all() and (v.nets[1] == 2).all() and (v.inps[1] == 3).all() and not v.fmaps[0].any()
    pose, disp, intr, fmap, net, inp = v[-1]             # negative: counted from the counter
    assert pose[0] == 2 and fmap.shape == (1, 128, 2, 3) and (net == 2).all() and (inp == 3).all() and intr[3] == 8
    assert v[-2][0][0] == 3 and v[1][0][0] == 2
    v[5] = (9.0, torch.zeros(3, 16, 24, dtype=torch.uint8), None, None, None, None)      # None leaves pose, disparity, prior, intrinsics
    assert v.counter.value == 6 and v.poses[5, 6] == 1 and (v.disps[5] == 1).all() and v.timestamp[5] == 9
    # the kept quirk: a tensor index moves the counter only when its maximum EXCEEDS the counter
    w = _video()
    w.counter.value = 2
    idx = torch.tensor([1, 2])
    w[idx] = (torch.tensor([5.0, 6.0]), torch.zeros(2, 3, 16, 24, dtype=torch.uint8), None, None, None, None)
    assert w.counter.value == 2 and w.timestamp[2] == 6
    idx = torch.tensor([1, 3])
    w[idx] = (torch.tensor([5.0, 7.0]), torch.zeros(2, 3, 16, 24, dtype=torch.uint8), None, None, None, None)
    assert w.counter.value == 4


def test_set_dirty_normalize_and_format_indicies():
    from splat_slam_amd.depth_video import DepthVideo
    v = _video()
    for t in range(3):
        v.append(*_item(v, t + 1))
    v.disps[:3] = torch.tensor([1.0, 2.0, 3.0])[:, None, None]
    v.normalize()
    assert torch.allclose(v.disps[:3].mean(), torch.tensor(1.0)) and torch.allclose(v.poses[:3, 0], torch.tensor([2.0, 4.0, 6.0]))
    assert (v.disps[3:] == 1).all()
    assert v.dirty.tolist() == [True] * 3 + [False] * 3 and torch.equal(v.dirty, v.npc_dirty)
    v.set_dirty(4, 6)
    assert v.dirty.tolist() == [True, True, True, False, True, True]
    ii, jj = DepthVideo.format_indicies([[0, 1], [2, 3]], np.array([1, 2, 3, 4], np.int32), device="cpu")
    assert ii.dtype == jj.dtype == torch.int64 and ii.tolist() == [0, 1, 2, 3] and jj.tolist() == [1, 2, 3, 4]


def test_methods_refuse_cpu_state_and_bad_arguments_before_any_launch():
    v = _video()
    for t in range(3):
        v.append(*_item(v, t + 1))
    with pytest.raises(ValueError, match="mask must view to"):
        v.upsample(torch.tensor([0, 1]), torch.zeros(2, 576, 2, 2))
    with pytest.raises(TypeError, match="mask must be a torch.Tensor"):
        v.upsample(torch.tensor([0, 1]), None)
    with pytest.raises(RuntimeError, match="GPU tensor"):
        v.upsample(torch.tensor([0, 1]), torch.zeros(1, 2, 576, 2, 3))
    v.set_dirty(0, 2)
    for up in (True, False):
        with pytest.raises(RuntimeError, match="GPU tensor"):
            v.update_valid_depth_mask(up=up)
    assert v.dirty[:2].all()                             # nothing was cleared
    v.dirty[:] = False
    v.update_valid_depth_mask(up=True)                   # nothing dirty: nothing to do
    ii, jj = torch.tensor([0, 1]), torch.tensor([1, 0])
    tw, eta = torch.zeros(2, 2, 3, 2), torch.zeros(2, 2, 3)
    with pytest.raises(RuntimeError, match="GPU tensor"):
        v.distance(ii, jj)
    with pytest.raises(RuntimeError, match="GPU tensor"):
        v.ba(tw, tw, eta, ii, jj, t0=1, t1=2)
    with pytest.raises(RuntimeError, match="GPU tensor"):
        v.ba(tw, tw, eta, ii, jj, t0=1, t1=2, opt_type="depth_scale")
    with pytest.raises(NotImplementedError, match="opt_type"):
        v.dspo(tw, tw, eta, ii, jj, t1=2, opt_type="scale_only")
    v.BA_type = "MoBA"
    with pytest.raises(NotImplementedError, match="BA_type"):
        v.ba(tw, tw, eta, ii, jj, t1=2)
    with pytest.raises(RuntimeError, match="GPU"):
        v.get_depth_and_pose(0, "cpu")
    assert not hasattr(v, "reproject")


def test_save_video_writes_the_reference_keys(tmp_path, monkeypatch):
    v = _video()
    for t in range(3):
        v.append(*_item(v, t + 1))
    v.disps_up[:3] = 0.5
    v.valid_depth_mask[1] = True
    monkeypatch.setattr(v, "get_pose", lambda index, device: torch.eye(4) * (index + 1))          # the pose matrix is GPU work
    path = str(tmp_path / "video.npz")
    v.save_video(path)
    z = dict(np.load(path))
    assert sorted(z) == ["depths", "poses", "timestamps", "valid_depth_masks"]
    assert z["poses"].shape == (3, 4, 4) and z["depths"].shape == (3, 16, 24) and z["valid_depth_masks"].dtype == bool
    assert (z["depths"] == 2).all() and z["timestamps"].tolist() == [1, 2, 3] and z["valid_depth_masks"][1].all()
    assert not z["valid_depth_masks"][0].any() and z["poses"][2, 0, 0] == 3
