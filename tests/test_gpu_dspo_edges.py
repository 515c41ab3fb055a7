"""splat_slam_amd.dspo on the MI355X at its graph and size edges, every element held to its own derived bound (tests/dspo_cases.py:
criteria A and B and the exact conditions, against the fp64 oracle with magnitudes of tests/dspo_ref.py), depth_scale_step with edges
whose frames do not exist, and the alignment at small odd frames and at its degenerate ones.  tests/test_dspo_cpu.py proves the same
criteria on the CPU: the fp32 restatement passes them and the planted faults fail one."""
import numpy as np
import pytest
import torch

import dba_ref as R
import dspo_cases as DC
import dspo_ref as D

pytestmark = pytest.mark.gpu


def f32(a):
    return torch.tensor(np.asarray(a), dtype=torch.float32, device="cuda").contiguous()


def i64(a):
    return torch.tensor([int(v) for v in a], dtype=torch.int64, device="cuda")


def to_gpu(c, edges=None):
    e = list(range(len(c["ii"]))) if edges is None else edges
    keep = None if c["keep"] is None else torch.tensor(c["keep"][e], device="cuda")
    return dict(poses=f32(c["poses"]), disps=f32(c["disps"]), intr=f32(c["intr"]), tgt=f32(c["tgt"][e]), wgt=f32(c["wgt"][e]),
                eta=f32(c["eta"]), ii=i64([c["ii"][k] for k in e]), jj=i64([c["jj"][k] for k in e]), mono=f32(c["mono"]),
                vmask=torch.tensor(c["vmask"], dtype=torch.bool, device="cuda"), scales=f32(c["scales"]), shifts=f32(c["shifts"]),
                keep=keep)


def run(c, g, iterations=1):
    from splat_slam_amd import dspo
    dwq, dz = dspo.ba_with_scale_shift(g["tgt"], g["wgt"], g["eta"], g["poses"], g["disps"], g["intr"], g["ii"], g["jj"], g["mono"],
                                       g["scales"], g["shifts"], g["vmask"], c["ignore_frames"], c["lm"], c["ep"], c["alpha"], iterations,
                                       g["keep"])
    torch.cuda.synchronize()
    return dwq, dz


def outputs(g, dwq, dz):
    return tuple(t.cpu().numpy() for t in (g["disps"], g["scales"], g["shifts"], dwq, dz))


def same_bits(a, b):
    for x, y in zip(a, b):
        assert torch.equal(x, y)


def state(g, dwq, dz):
    return dwq, dz, g["disps"], g["scales"], g["shifts"]


@pytest.mark.parametrize("name", DC.CASES)
def test_one_iteration_is_inside_every_bound(name):
    DC.check_scene(name, want_between=name.startswith("pix"))
    c = DC.case(name)
    g = to_gpu(c)
    if name == "mask:u8":
        assert g["keep"].dtype == torch.uint8 and sorted(set(g["keep"].tolist())) == [0, 1, 2, 255]
    g_in = {k: (None if v is None else v.clone()) for k, v in g.items()}
    dwq, dz = run(c, g)
    ratios, broken = DC.criteria(name, *outputs(g, dwq, dz))
    print(f"\n{name}: err / bound " + " ".join(f"{k}={v:.4f}" for k, v in sorted(ratios.items())), broken)
    assert not broken, broken
    for k, r in ratios.items():
        assert r <= 1.0, (name, k, r)
    for k in ("poses", "intr", "tgt", "wgt", "eta", "ii", "jj", "mono", "vmask"):
        assert torch.equal(g[k], g_in[k]), k
    o = DC.oracle(name)
    if name == "singular":                              # the frame without a prior: no step in s and q, and dz = Q b all the same
        k = o["kx"].index(DC.SINGULAR_FRAME[name])
        assert not dwq[k].any() and dz[k].abs().max() > 1e-4
        rest = [r for r in range(o["M"]) if r != k]
        assert (dwq[rest].abs() > 0).all()
    if name.startswith("mask"):                         # frames 4 and 7 lose every edge: zero rows, the bits that came in
        for f in (4, 7):
            k = o["kx"].index(f)
            assert not dwq[k].any() and not dz[k].any()
            for key in ("disps", "scales", "shifts"):
                assert torch.equal(g[key][f], g_in[key][f])


def test_uint8_mask_with_values_above_one_gives_the_bits_of_the_bool_mask():
    cb, cu = DC.case("mask:bool"), DC.case("mask:u8")
    gb, gu = to_gpu(cb), to_gpu(cu)
    same_bits(state(gb, *run(cb, gb)), state(gu, *run(cu, gu)))


@pytest.mark.parametrize("name", ["oob", "oob:long_poses", "oob:short_poses"])
def test_out_of_range_edges_take_part_in_nothing(name):
    c = DC.case(name)
    keep = R.kept_edges(c["ii"], c["jj"], min(len(c["poses"]), len(c["disps"])))
    assert 0 < len(keep) < len(c["ii"])
    assert 8 not in DC.oracle(name)["kx"]               # frame 8 occurs only as the ii of a dropped edge: no depth row
    g_all, g_kept = to_gpu(c), to_gpu(c, keep)
    a, b = state(g_all, *run(c, g_all)), state(g_kept, *run(c, g_kept))
    same_bits(a, b)
    assert a[0].abs().max() > 0 and a[1].abs().max() > 0


def test_two_iterations_equal_two_calls_of_one_and_a_side_stream_gives_the_same_bits():
    c = DC.case("iter")                                 # the relative poses do not change between iterations, so this must hold
    g2, g11, gs = to_gpu(c), to_gpu(c), to_gpu(c)
    two = state(g2, *run(c, g2, iterations=2))
    first = [t.clone() for t in run(c, g11)]
    both = state(g11, *run(c, g11))
    same_bits(two, both)
    assert not torch.equal(first[1], both[1])           # the second step is a step of its own
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        dwq, dz = run(c, gs, iterations=2)
    torch.cuda.synchronize()
    same_bits(two, state(gs, dwq, dz))


# ---- depth_scale_step with edges whose frames do not exist
def test_depth_scale_step_ignores_out_of_range_edges():
    """Frames 0, 1 and 8 are the ii of no in-range edge; their maps hold negative and zero disparities, which only the final clamp of
    a MOVED frame would change.  Edges -1 -> 3, n + 5 -> 4 and 1 -> n are kept by the bad-frame rule (no frame is bad) and dropped by
    the kernels; they must not mark frames 0, 8 and 1 as moved."""
    from splat_slam_amd import dspo
    n = 9
    ii = [-1] + DC.GRAPH_II[:5] + [n + 5] + DC.GRAPH_II[5:] + [1]
    jj = [3] + DC.GRAPH_JJ[:5] + [4] + DC.GRAPH_JJ[5:] + [n]
    c = dict(DC.make("step_oob", 7, 9, ii, jj, n=n, seed=181, alpha=0.01, plant=False))
    for f in (0, 1, 8):
        c["disps"][f, 1, :2] = (0.0, -0.5)
        assert (c["disps"][f] < 0).any() and (c["disps"][f] == 0).any() and f not in D.depth_frames(ii, jj, n)
    inr = R.kept_edges(ii, jj, n)
    assert len(inr) == len(ii) - 3
    d_ref, s_ref, q_ref, keep_ref, any_ref = D.depth_scale_step(c["poses"], c["disps"], c["intr"], c["mono"], c["vmask"], c["scales"],
                                                                c["shifts"], n, c["tgt"], c["wgt"], c["eta"], ii, jj, itrs=1)
    assert any_ref and keep_ref[inr].all()              # no frame is bad: every in-range edge is kept
    g = to_gpu(c)
    g_in = {k: (None if v is None else v.clone()) for k, v in g.items()}
    # the pieces of the step on their own: the fit and the mask, then one iteration from the fit
    p = to_gpu(c)
    keep = dspo.align_and_mask(p["disps"], p["mono"], p["vmask"], p["scales"], p["shifts"], n, p["ii"], p["jj"])
    assert np.array_equal(keep.cpu().numpy()[inr], keep_ref[inr])
    fit = dict(c, scales=p["scales"].cpu().numpy().astype(np.float64), shifts=p["shifts"].cpu().numpy().astype(np.float64),
               keep=keep.cpu().numpy())
    np.testing.assert_allclose(fit["scales"], D.bad_frames(c["mono"], c["disps"], c["vmask"], n, 0.1)[0], rtol=1e-5, atol=0)
    np.testing.assert_allclose(fit["shifts"], D.bad_frames(c["mono"], c["disps"], c["vmask"], n, 0.1)[1], rtol=1e-5, atol=0)
    dwq, dz = dspo.ba_with_scale_shift(p["tgt"], p["wgt"], p["eta"], p["poses"], p["disps"], p["intr"], p["ii"], p["jj"], p["mono"],
                                       p["scales"], p["shifts"], p["vmask"], 0, 1e-4, 0.1, 0.01, 1, keep)
    o = D.linearize_mag(fit)
    ratios, broken = DC.criteria_for(fit, o, *outputs(p, dwq, dz))
    print("\nstep_oob: err / bound " + " ".join(f"{k}={v:.4f}" for k, v in sorted(ratios.items())), broken)
    assert not broken and all(r <= 1.0 for r in ratios.values()), (ratios, broken)
    # the whole step
    any_kept = dspo.depth_scale_step(g["poses"], g["disps"], g["intr"], g["mono"], g["vmask"], g["scales"], g["shifts"], n, g["tgt"],
                                     g["wgt"], g["eta"], g["ii"], g["jj"], itrs=1, alpha=0.01)
    torch.cuda.synchronize()
    assert bool(any_kept) is any_ref
    for f in (0, 1, 8):                                 # not moved: the bits that came in, negative and zero disparities included
        assert torch.equal(g["disps"][f], g_in["disps"][f]), f
    moved = sorted(set(ii[e] for e in inr))
    assert moved == [2, 3, 4, 5, 6, 7]
    # moved frames: the iteration's own bits, clamped; and criterion B's bound around the oracle's dz at the device's dwq, clamped alike
    assert torch.equal(g["disps"][moved], p["disps"][moved].clamp(min=1e-5))
    assert torch.equal(g["scales"], p["scales"]) and torch.equal(g["shifts"], p["shifts"])
    ref = D.back_substitute(o, dwq.cpu().numpy())
    for k, f in enumerate(o["kx"]):
        before = c["disps"][f].reshape(-1) + ref.v[k]
        want = np.maximum(np.maximum(before, 0.0), 1e-5)
        bnd = ref.bound()[k] + R.U32 * np.abs(before) + R.U32 * 1e-5      # dz, one rounding of the sum, the fp32 1e-5 (max is 1-Lipschitz)
        err = np.abs(g["disps"][f].cpu().numpy().reshape(-1).astype(np.float64) - want)
        assert np.all(err <= bnd), (f, float((err / bnd).max()))
    # and the fp64 step as a whole: the same frames moved, by steps that agree to the backward error A allows
    untouched = [f for f in range(n) if f not in moved]
    assert np.array_equal(d_ref[untouched], c["disps"][untouched])
    assert (d_ref[moved] >= 1e-5).all() and (g["disps"][moved] >= 1e-5).all()
    for got, want in ((g["scales"], s_ref), (g["shifts"], q_ref)):        # no depth frame: the fit alone
        np.testing.assert_allclose(got.cpu().numpy()[untouched], want[untouched], rtol=1e-5, atol=0)


# ---- the alignment at its edges
ALIGN_SHAPES = ((3, 5), (1, 257), (16, 16))


def align_frames(ht, wd, n=4, seed=0):
    rng = np.random.default_rng(190 + wd + seed)
    est = rng.uniform(0.3, 1.0, (n, ht, wd))
    mono = 1.7 * est + 0.05 + rng.normal(0, 0.02, est.shape)
    return rng, DC.r32(mono), DC.r32(est)


@pytest.mark.parametrize("shape", ALIGN_SHAPES)
@pytest.mark.parametrize("kind", ["bool", "uint8", "float"])
def test_alignment_matches_the_oracle_at_small_and_odd_frames(shape, kind):
    from splat_slam_amd import dspo
    rng, mono, est = align_frames(*shape)
    if kind == "float":
        w = DC.r32(rng.uniform(0.0, 1.0, est.shape))
        wt, w_ref = f32(w), w
    elif kind == "uint8":
        w = rng.choice(np.array([0, 1, 2, 255], np.uint8), est.shape)
        wt, w_ref = torch.tensor(w, device="cuda"), (w != 0).astype(float)
    else:
        w = rng.uniform(size=est.shape) < 0.6
        wt, w_ref = torch.tensor(w, device="cuda"), w.astype(float)
    got = np.stack([t.cpu().numpy() for t in dspo.align_scale_and_shift(f32(mono), f32(est), wt)])
    want = np.stack(D.align_scale_and_shift(mono, est, w_ref))
    print("\nalign", shape, kind, np.abs(got / want - 1).max())
    np.testing.assert_allclose(got, want, rtol=1e-5, atol=0)


def test_alignment_of_a_frame_without_weights_is_nan_and_its_edges_are_dropped():
    from splat_slam_amd import dspo
    n, (ht, wd) = 6, (7, 9)
    rng, mono, est = align_frames(ht, wd, n)
    valid = rng.uniform(size=est.shape) < 0.7
    valid[1] = False                                    # no weight at all: 0 / 0 in all three outputs
    valid[3] = rng.uniform(size=(ht, wd)) < 0.3         # fewer than half the pixels valid
    mono[4] = -mono[4]                                  # opposite sign: the fitted scale is negative
    counts = valid.sum((1, 2))
    assert counts[1] == 0 and counts[3] < 31 and all(counts[f] > 32 for f in (0, 2, 4, 5))
    s, q, e = (t.cpu().numpy() for t in dspo.align_scale_and_shift(f32(mono), f32(est), torch.tensor(valid, device="cuda")))
    assert np.isnan([s[1], q[1], e[1]]).all() and np.isfinite(np.delete(np.stack([s, q, e]), 1, 1)).all()
    s_ref, q_ref, bad_ref = D.bad_frames(mono, est, valid, 5, 0.1)
    assert s_ref[4] < 0 and list(np.nonzero(bad_ref)[0]) == [1, 3, 4]
    ii, jj = [0, 1, 2, 0, 3, 2, 4, 5, 2, 5], [1, 0, 0, 2, 2, 3, 0, 4, 5, 5]
    keep_ref = np.array([not ((i < 5 and bad_ref[i]) or (j < 5 and bad_ref[j])) for i, j in zip(ii, jj)])
    assert keep_ref.tolist() == [False, False, True, True, False, False, False, False, True, True]
    scales, shifts = f32(np.full(n, 7.0)), f32(np.full(n, -3.0))
    keep = dspo.align_and_mask(f32(est), f32(mono), torch.tensor(valid, device="cuda"), scales, shifts, 5, i64(ii), i64(jj))
    assert keep.dtype == torch.bool and np.array_equal(keep.cpu().numpy(), keep_ref)
    # n_frames < N: the rows beyond it keep their bits, the rows below it hold the fit
    assert scales[5].item() == 7.0 and shifts[5].item() == -3.0
    ok = [0, 2, 3, 4]
    np.testing.assert_allclose(scales.cpu().numpy()[ok], s_ref[ok], rtol=1e-5, atol=0)
    np.testing.assert_allclose(shifts.cpu().numpy()[ok], q_ref[ok], rtol=1e-5, atol=0)
    assert torch.isnan(scales[1]) and torch.isnan(shifts[1])


def test_alignment_of_no_frames_returns_empty_outputs():
    from splat_slam_amd import dspo
    e = torch.empty((0, 3, 5), dtype=torch.float32, device="cuda")
    out = dspo.align_scale_and_shift(e, e, torch.empty((0, 3, 5), dtype=torch.bool, device="cuda"))
    assert all(t.shape == (0,) and t.dtype == torch.float32 and t.is_cuda for t in out)
