"""splat_slam_amd.dspo on the MI355X against the fp64 restatement (tests/dspo_ref.py): one and two iterations, the edge mask, ignored
frames, the refused call, reproducibility, the absence of host synchronisation, the alignment, convergence, the bad-frame rule of
depth_scale_step and a backend-sized graph.  Bounds are those tests/test_gpu_dba.py uses for the same arithmetic; one iteration is
also held element by element to the derived bounds of tests/dspo_cases.py, as tests/test_gpu_dspo_edges.py holds the small shapes."""
import numpy as np
import pytest
import torch

import dba_ref as R
import dspo_cases as DC
import dspo_ref as D

pytestmark = pytest.mark.gpu

SHAPES = {(48, 64): np.array([50.0, 52.0, 31.5, 23.5]), (40, 80): np.array([60.0, 58.0, 39.5, 19.5])}
II = [2, 3, 3, 4, 4, 5, 5, 2, 3, 6, 7, 4, 3]          # depth frames 2..7; frames 0, 1 only receive edges, frame 8 has none
JJ = [3, 2, 4, 3, 5, 4, 2, 5, 3, 5, 4, 6, 0]          # (3, 3) is a stereo edge


def r32(a):
    return np.asarray(a, np.float32).astype(float)


def rel(a, b):
    a, b = np.asarray(a, float), np.asarray(b, float)
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30)


def make_scene(ht, wd, n=9, seed=0, near_block=True):
    rng = np.random.default_rng(seed)
    poses = []
    for f in range(n):
        t, q = R.exp_se3(np.concatenate([[0.03 * f, 0.01 * np.sin(f), 0.02 * f], rng.normal(0, 0.02, 3)]))
        poses.append(np.concatenate([t, q]))
    disps = rng.uniform(0.3, 1.0, (n, ht, wd))
    if near_block:
        disps[:, :6, :10] = -60.0                   # z = 1 + h tz: where tz < 0 these pixels land far nearer than MIN_DEPTH
    return rng, np.stack(poses), disps


def problem(ht, wd, seed=0, noise=0.5, near_block=True, mono_noise=0.01, mono_holes=0.1, ii=II, jj=JJ, n=9):
    """Flow targets of the true scene (+ noise) in the [E,ht,wd,2] layout, perturbed disparities, a mono prior m = 1.7 h + 0.05 (+ noise)
    with holes (exactly 0), a valid-depth mask on ~60 % of the pixels that overlaps the holes, scales and shifts near the truth."""
    rng, poses, disps = make_scene(ht, wd, n=n, seed=seed, near_block=near_block)
    intr = SHAPES[(ht, wd)]
    tgt = np.stack([D.project(poses[i], poses[j], disps[i], intr, i == j).reshape(ht, wd, 2) for i, j in zip(ii, jj)])
    tgt += rng.normal(0, noise, tgt.shape) if noise else 0.0
    wgt = rng.uniform(0.2, 1.0, tgt.shape)
    d0 = np.where(disps < 0, disps, disps * rng.uniform(0.95, 1.05, disps.shape))
    mono = 1.7 * disps + 0.05 + (rng.normal(0, mono_noise, disps.shape) if mono_noise else 0.0)
    mono[rng.uniform(size=mono.shape) < mono_holes] = 0.0
    vmask = rng.uniform(size=mono.shape) < 0.6
    scales = 1 / 1.7 + rng.normal(0, 0.02, n)
    shifts = -0.05 / 1.7 + rng.normal(0, 0.01, n)
    eta = rng.uniform(1e-3, 1e-2, (len(set(ii)), ht, wd))
    return dict(poses=poses, disps=d0, truth=disps, intr=intr, tgt=tgt, wgt=wgt, mono=mono, vmask=vmask, scales=scales, shifts=shifts,
                eta=eta, ii=list(ii), jj=list(jj))


def to_gpu(pr):
    f = lambda a: torch.tensor(np.asarray(a), dtype=torch.float32, device="cuda").contiguous()
    li = lambda a: torch.tensor(a, dtype=torch.int64, device="cuda")
    return dict(poses=f(pr["poses"]), disps=f(pr["disps"]), intr=f(pr["intr"]), tgt=f(pr["tgt"]), wgt=f(pr["wgt"]), mono=f(pr["mono"]),
                vmask=torch.tensor(pr["vmask"], dtype=torch.bool, device="cuda"), scales=f(pr["scales"]), shifts=f(pr["shifts"]),
                eta=f(pr["eta"]), ii=li(pr["ii"]), jj=li(pr["jj"]))


def run_gpu(g, iters=1, lm=1e-4, ep=0.1, alpha=1.0, ignore_frames=0, keep=None):
    from splat_slam_amd import dspo
    dwq, dz = dspo.ba_with_scale_shift(g["tgt"], g["wgt"], g["eta"], g["poses"], g["disps"], g["intr"], g["ii"], g["jj"], g["mono"],
                                       g["scales"], g["shifts"], g["vmask"], ignore_frames, lm, ep, alpha, iters, keep)
    torch.cuda.synchronize()
    return dwq, dz


def run_ref(pr, iters=1, lm=1e-4, ep=0.1, alpha=1.0, ignore_frames=0, keep=None, margins=False):
    # the oracle sees the fp32-rounded inputs the GPU sees
    return D.ba_with_scale_shift(r32(pr["tgt"]), r32(pr["wgt"]), r32(pr["eta"]), r32(pr["poses"]), r32(pr["disps"]), r32(pr["intr"]),
                                 pr["ii"], pr["jj"], r32(pr["mono"]), r32(pr["scales"]), r32(pr["shifts"]), pr["vmask"], ignore_frames,
                                 lm, ep, alpha, iters, keep, margins)


def check_scene(pr, marg, counted):
    """No pixel, counted or not, near the depth threshold; no mono value near its threshold; every (invalid, valid-depth) case."""
    assert marg.min() > 1e-3, marg.min()
    assert counted.any() and (~counted).any()
    m = r32(pr["mono"])
    assert not ((m > 0) & (m < 0.1)).any()
    kx = D.depth_frames(pr["ii"])
    hole, vd = m[kx] < 1e-6, pr["vmask"][kx]
    assert all((hole[vd == b] == a).any() for a in (False, True) for b in (False, True))
    assert 0.05 < (m[kx] == 0).mean() < 0.15 and 0.5 < vd.mean() < 0.7


def check_against_oracle(g, pr, g_in, dwq, dz, ref):
    d_ref, s_ref, q_ref, dwq_ref, dz_ref = ref
    dwq, dz = dwq.cpu().numpy(), dz.cpu().numpy()
    assert np.all(np.isfinite(dwq)) and np.all(np.isfinite(dz))
    print("dwq rel", rel(dwq, dwq_ref), "dz err", np.abs(dz - dz_ref).max(), "of", np.abs(dz_ref).max(),
          "disps err", np.abs(g["disps"].cpu().numpy() - d_ref).max(), "dwq max", np.abs(dwq_ref).max())
    tol = 2e-3
    assert rel(dwq, dwq_ref) < tol, rel(dwq, dwq_ref)
    assert np.abs(dz - dz_ref).max() < tol * np.abs(dz_ref).max() + 1e-6
    assert np.abs(g["disps"].cpu().numpy() - d_ref).max() < tol * np.abs(dz_ref).max() + 1e-5
    assert np.abs(g["scales"].cpu().numpy() - s_ref).max() < tol * np.abs(dwq_ref).max() + 1e-6
    assert np.abs(g["shifts"].cpu().numpy() - q_ref).max() < tol * np.abs(dwq_ref).max() + 1e-6
    assert torch.equal(g["poses"], g_in["poses"])                      # poses: the bits that came in
    for f in set(range(len(pr["poses"]))) - set(pr["ii"]):              # frames that are no depth frames: untouched bits
        assert torch.equal(g["disps"][f], g_in["disps"][f])
        assert torch.equal(g["scales"][f], g_in["scales"][f]) and torch.equal(g["shifts"][f], g_in["shifts"][f])


def clone(g):
    return {k: v.clone() for k, v in g.items()}


@pytest.mark.parametrize("shape", list(SHAPES))
@pytest.mark.parametrize("alpha", [1.0, 0.01])
def test_one_iteration_matches_the_fp64_oracle(shape, alpha):
    pr = problem(*shape, seed=3)
    g = to_gpu(pr)
    g_in = clone(g)
    dwq, dz = run_gpu(g, 1, alpha=alpha)
    *ref, marg, counted = run_ref(pr, 1, alpha=alpha, margins=True)
    check_scene(pr, marg, counted)
    assert dwq.shape == (6, 2) and dz.shape == (6, shape[0] * shape[1])
    check_against_oracle(g, pr, g_in, dwq, dz, ref)
    # ... and element by element: criteria A and B and the exact conditions of tests/dspo_cases.py at the tracker's sizes
    c = DC.from_problem(pr, alpha=alpha)
    o = D.linearize_mag(c)
    assert o["zmargin"] > 1e-3 and not o["fail"].any() and o["pivots"].min() >= 1e-6
    ratios, broken = DC.criteria_for(c, o, *(t.cpu().numpy() for t in (g["disps"], g["scales"], g["shifts"], dwq, dz)))
    print(f"{shape} alpha={alpha}: err / bound " + " ".join(f"{k}={v:.4f}" for k, v in sorted(ratios.items())), broken)
    assert not broken, broken
    assert set(ratios) == {"A", "B"} and all(r <= 1.0 for r in ratios.values()), ratios


@pytest.mark.parametrize("shape", list(SHAPES))
@pytest.mark.parametrize("alpha", [1.0, 0.01])
def test_two_iterations_match_the_fp64_oracle(shape, alpha):
    pr = problem(*shape, seed=4)
    g = to_gpu(pr)
    g_in = clone(g)
    dwq, dz = run_gpu(g, 2, alpha=alpha)
    *ref, marg, counted = run_ref(pr, 2, alpha=alpha, margins=True)
    check_scene(pr, marg, counted)
    check_against_oracle(g, pr, g_in, dwq, dz, ref)


def test_masked_edges_equal_a_host_filtered_edge_list_bit_for_bit():
    pr = problem(48, 64, seed=5)
    keep = np.array([i != 4 and j != 4 for i, j in zip(pr["ii"], pr["jj"])])        # frame 7 loses its only edge as well
    g = to_gpu(pr)
    g_in = clone(g)
    dwq, dz = run_gpu(g, 2, keep=torch.tensor(keep, device="cuda"))
    kx = D.depth_frames(pr["ii"])
    ii2, jj2 = [i for i, k in zip(pr["ii"], keep) if k], [j for j, k in zip(pr["jj"], keep) if k]
    kx2 = D.depth_frames(ii2)
    rows = [kx.index(f) for f in kx2]
    assert kx2 == [2, 3, 5, 6]
    h = clone(g_in)
    sel = torch.tensor(np.nonzero(keep)[0], device="cuda")
    h.update(tgt=g_in["tgt"][sel].contiguous(), wgt=g_in["wgt"][sel].contiguous(), eta=g_in["eta"][rows].contiguous(),
             ii=torch.tensor(ii2, device="cuda"), jj=torch.tensor(jj2, device="cuda"))
    dwq2, dz2 = run_gpu(h, 2)
    assert torch.equal(dwq[rows], dwq2) and torch.equal(dz[rows], dz2)
    assert dwq2.abs().max() > 0 and dz2.abs().max() > 0
    for k in ("disps", "scales", "shifts", "poses"):
        assert torch.equal(g[k], h[k]), k
    for f in (4, 7):                                                    # masked out: untouched, zero rows
        assert torch.equal(g["disps"][f], g_in["disps"][f]) and torch.equal(g["scales"][f], g_in["scales"][f])
        assert torch.equal(g["shifts"][f], g_in["shifts"][f])
        assert not dwq[kx.index(f)].any() and not dz[kx.index(f)].any()
    ref = run_ref(pr, 2, keep=keep)
    check_against_oracle(g, pr, g_in, dwq, dz, ref)


def test_an_all_zero_edge_mask_changes_nothing():
    pr = problem(40, 80, seed=6)
    g = to_gpu(pr)
    g_in = clone(g)
    dwq, dz = run_gpu(g, 2, keep=torch.zeros(len(pr["ii"]), dtype=torch.uint8, device="cuda"))
    assert not dwq.any() and not dz.any()
    for k in g:
        assert torch.equal(g[k], g_in[k]), k


@pytest.mark.parametrize("shape", list(SHAPES))
def test_ignored_frames_match_the_oracle(shape):
    pr = problem(*shape, seed=7)
    g = to_gpu(pr)
    g_in = clone(g)
    dwq, dz = run_gpu(g, 1, ignore_frames=3)
    ref = run_ref(pr, 1, ignore_frames=3)
    assert np.all(ref[3][0] == 0)                        # frame 2 < ignore_frames: no prior, so no scale or shift step
    check_against_oracle(g, pr, g_in, dwq, dz, ref)


def test_wrong_number_of_depth_frames_is_reported_as_nan_and_updates_nothing():
    pr = problem(48, 64, seed=8)
    pr["eta"] = pr["eta"][:-1]
    g = to_gpu(pr)
    g_in = clone(g)
    dwq, dz = run_gpu(g, 2)
    assert torch.isnan(dwq).all() and torch.isnan(dz).all()
    for k in g:
        assert torch.equal(g[k], g_in[k]), k


def test_two_identical_calls_give_identical_bits():
    from splat_slam_amd import dspo
    pr = problem(40, 80, seed=9)
    outs = []
    for _ in range(2):
        g = to_gpu(pr)
        dwq, dz = run_gpu(g, 3)
        fit = dspo.align_scale_and_shift(g["mono"], g["disps"], g["vmask"])
        outs.append((dwq, dz, g["disps"], g["scales"], g["shifts"]) + tuple(fit))
    for a, b in zip(*outs):
        assert torch.equal(a, b)


def test_no_entry_point_synchronises_with_the_host():
    from splat_slam_amd import dspo
    pr = problem(48, 64, seed=10)
    g = to_gpu(pr)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        dspo.ba_with_scale_shift(g["tgt"], g["wgt"], g["eta"], g["poses"], g["disps"], g["intr"], g["ii"], g["jj"], g["mono"], g["scales"],
                                 g["shifts"], g["vmask"], 0, 1e-4, 0.1, 1.0, 2)
        any_kept = dspo.depth_scale_step(g["poses"], g["disps"], g["intr"], g["mono"], g["vmask"], g["scales"], g["shifts"], 9, g["tgt"],
                                         g["wgt"], g["eta"], g["ii"], g["jj"])
    finally:
        torch.cuda.set_sync_debug_mode(0)
    torch.cuda.synchronize()
    assert any_kept.dim() == 0 and any_kept.dtype == torch.bool and any_kept.is_cuda
    assert torch.isfinite(g["disps"]).all() and torch.isfinite(g["scales"]).all()


# ---- alignment
@pytest.mark.parametrize("shape", list(SHAPES))
def test_alignment_matches_the_oracle(shape):
    from splat_slam_amd import dspo
    pr = problem(*shape, seed=11)
    g = to_gpu(pr)
    s, q, e = (t.cpu().numpy() for t in dspo.align_scale_and_shift(g["mono"], g["disps"], g["vmask"]))
    s_ref, q_ref, e_ref = D.align_scale_and_shift(r32(pr["mono"]), r32(pr["disps"]), pr["vmask"].astype(float))
    print("align", np.abs(s / s_ref - 1).max(), np.abs(q / q_ref - 1).max(), np.abs(e / e_ref - 1).max())
    assert s.shape == (9,)
    np.testing.assert_allclose(s, s_ref, rtol=1e-5, atol=0)
    np.testing.assert_allclose(q, q_ref, rtol=1e-5, atol=0)
    np.testing.assert_allclose(e, e_ref, rtol=1e-5, atol=0)
    s0, q0, e0 = (t.cpu().numpy() for t in dspo.align_scale_and_shift(g["mono"], g["disps"]))           # no weights: all ones
    s0_ref, q0_ref, e0_ref = D.align_scale_and_shift(r32(pr["mono"]), r32(pr["disps"]))
    np.testing.assert_allclose(np.stack([s0, q0, e0]), np.stack([s0_ref, q0_ref, e0_ref]), rtol=1e-5, atol=0)


def test_alignment_takes_one_map_and_bool_weights_equal_float_weights():
    from splat_slam_amd import dspo
    pr = problem(48, 64, seed=12)
    g = to_gpu(pr)
    a = dspo.align_scale_and_shift(g["mono"], g["disps"], g["vmask"])
    b = dspo.align_scale_and_shift(g["mono"], g["disps"], g["vmask"].to(torch.float32))
    c = dspo.align_scale_and_shift(g["mono"], g["disps"], g["vmask"].to(torch.uint8))
    for x, y, z in zip(a, b, c):
        assert torch.equal(x, y) and torch.equal(x, z)
    one = dspo.align_scale_and_shift(g["mono"][2], g["disps"][2], g["vmask"][2])
    for x, y in zip(one, a):
        assert x.shape == (1,) and torch.equal(x[0], y[2])


def test_alignment_recovers_an_exact_scale_and_shift():
    from splat_slam_amd import dspo
    gen = torch.Generator(device="cuda").manual_seed(13)
    pred = torch.rand(5, 48, 64, device="cuda", generator=gen) * 1.8 + 0.2
    mask = torch.rand(5, 48, 64, device="cuda", generator=gen) < 0.5
    s, q, e = dspo.align_scale_and_shift(pred, 1.7 * pred + 0.05, mask)
    print("exact", s.tolist(), q.tolist(), e.tolist())
    assert (s - 1.7).abs().max() < 1e-5 and (q - 0.05).abs().max() < 1e-5
    assert e.max() < 1e-6


# ---- the whole stage
def step_gpu(g, n_frames, **kw):
    from splat_slam_amd import dspo
    return dspo.depth_scale_step(g["poses"], g["disps"], g["intr"], g["mono"], g["vmask"], g["scales"], g["shifts"], n_frames, g["tgt"],
                                 g["wgt"], g["eta"], g["ii"], g["jj"], **kw)


@pytest.mark.parametrize("shape", list(SHAPES))
def test_converges_on_noise_free_data(shape):
    pr = problem(*shape, seed=14, noise=0.0, near_block=False, mono_noise=0.0, mono_holes=0.0)
    pr["wgt"] = np.ones_like(pr["wgt"])
    g = to_gpu(pr)
    state = (r32(pr["disps"]), r32(pr["scales"]), r32(pr["shifts"]))
    fixed = dict(poses=r32(pr["poses"]), intr=r32(pr["intr"]), tgt=r32(pr["tgt"]), wgt=r32(pr["wgt"]), eta=r32(pr["eta"]),
                 mono=r32(pr["mono"]))
    for _ in range(8):
        assert bool(step_gpu(g, 9))
        d, s, q, _, kept = D.depth_scale_step(fixed["poses"], state[0], fixed["intr"], fixed["mono"], pr["vmask"], state[1], state[2], 9,
                                              fixed["tgt"], fixed["wgt"], fixed["eta"], pr["ii"], pr["jj"])
        assert kept
        state = (d, s, q)

    def cost(d, s, q):
        return D.cost(fixed["tgt"], fixed["wgt"], fixed["poses"], d, fixed["intr"], pr["ii"], pr["jj"], fixed["mono"], s, q, pr["vmask"], 0,
                      0.01, fixed["eta"], r32(pr["disps"]))

    s0, q0, _ = D.align_scale_and_shift(fixed["mono"], r32(pr["disps"]), pr["vmask"].astype(float))
    c0 = cost(r32(pr["disps"]), s0, q0)
    c_ref = cost(*state)
    c_gpu = cost(*(g[k].cpu().numpy().astype(float) for k in ("disps", "scales", "shifts")))
    print("cost", c0, c_ref, c_gpu)
    assert c_ref < 0.5 * c0                              # the oracle itself converges ...
    assert c_gpu < 1.5 * c_ref + 1e-4 * c0, (c0, c_ref, c_gpu)       # ... and the GPU as far
    kx = D.depth_frames(pr["ii"])
    err = lambda d: np.abs(np.asarray(d, float)[kx] - pr["truth"][kx]).mean()
    assert err(g["disps"].cpu().numpy()) < err(pr["disps"])


def test_depth_scale_step_drops_the_edges_of_badly_fitting_frames():
    from splat_slam_amd import dspo
    pr = problem(48, 64, seed=15)
    pr["mono"][4] = -pr["mono"][4]                       # opposite sign: the fitted scale is negative
    pr["vmask"][6] = np.random.default_rng(0).uniform(size=pr["vmask"][6].shape) < 0.3          # fewer than half the pixels valid
    g = to_gpu(pr)
    g_in = clone(g)
    d_ref, s_ref, q_ref, keep_ref, kept_ref = D.depth_scale_step(r32(pr["poses"]), r32(pr["disps"]), r32(pr["intr"]), r32(pr["mono"]),
                                                                 pr["vmask"], r32(pr["scales"]), r32(pr["shifts"]), 9, r32(pr["tgt"]),
                                                                 r32(pr["wgt"]), r32(pr["eta"]), pr["ii"], pr["jj"])
    s_fit, _, bad_ref = D.bad_frames(r32(pr["mono"]), r32(pr["disps"]), pr["vmask"], 9, 0.1)
    assert s_fit[4] < 0 and list(np.nonzero(bad_ref)[0]) == [4, 6] and kept_ref
    probe = clone(g_in)
    keep = dspo.align_and_mask(probe["disps"], probe["mono"], probe["vmask"], probe["scales"], probe["shifts"], 9, probe["ii"], probe["jj"])
    assert keep.dtype == torch.bool and np.array_equal(keep.cpu().numpy(), keep_ref)
    any_kept = step_gpu(g, 9)
    torch.cuda.synchronize()
    assert bool(any_kept) is True
    for f in (4, 6):
        assert torch.equal(g["disps"][f], g_in["disps"][f])
    assert torch.equal(g["disps"][8], g_in["disps"][8]) and torch.equal(g["poses"], g_in["poses"])
    dz_scale = np.abs(d_ref - r32(pr["disps"]))[D.depth_frames(pr["ii"])]
    dz_scale = dz_scale[dz_scale < 1.0].max()            # (not the near block, which the step moves from -60 to the floor)
    assert np.abs(g["disps"].cpu().numpy() - d_ref).max() < 2e-3 * dz_scale + 1e-5
    np.testing.assert_allclose(g["scales"].cpu().numpy(), s_ref, rtol=2e-3, atol=1e-6)
    np.testing.assert_allclose(g["shifts"].cpu().numpy(), q_ref, rtol=2e-3, atol=1e-6)
    moved = sorted(set(i for i, k in zip(pr["ii"], keep_ref) if k))
    assert (g["disps"][moved] >= 1e-5).all() and (g["disps"][4] < 0).any()

    # every frame bad (too few valid pixels everywhere): no edge is kept, and only the scales and shifts change -- to the alignment result
    pr["vmask"] = np.random.default_rng(1).uniform(size=pr["vmask"].shape) < 0.3
    g = to_gpu(pr)
    g_in = clone(g)
    assert D.bad_frames(r32(pr["mono"]), r32(pr["disps"]), pr["vmask"], 9, 0.1)[2].all()
    any_kept = step_gpu(g, 9)
    torch.cuda.synchronize()
    assert bool(any_kept) is False
    fit = dspo.align_scale_and_shift(g_in["mono"], g_in["disps"], g_in["vmask"])
    assert torch.isfinite(fit[0]).all() and torch.equal(g["scales"], fit[0]) and torch.equal(g["shifts"], fit[1])
    for k in g:
        if k not in ("scales", "shifts"):
            assert torch.equal(g[k], g_in[k]), k


def test_backend_sized_graph_matches_the_oracle():
    """Held to the norm-wise bounds of check_against_oracle only: the linearisation with magnitudes of 970 edges at 48 x 64 would
    take too long for this suite.  The element-wise criteria see the same code paths at the small shapes of test_gpu_dspo_edges.py
    (several edge tiles: tile:513; more than 1024 frames: big)."""
    ht, wd, n = 48, 64, 100
    ii, jj = [], []
    for i in range(n):
        for j in range(max(0, i - 5), min(n, i + 6)):
            if i != j:
                ii.append(i)
                jj.append(j)
    assert 900 <= len(ii) <= 1100
    pr = problem(ht, wd, seed=16, near_block=False, ii=ii, jj=jj, n=n)
    g = to_gpu(pr)
    g_in = clone(g)
    dwq, dz = run_gpu(g, 1)
    ref = run_ref(pr, 1)
    check_against_oracle(g, pr, g_in, dwq, dz, ref)
