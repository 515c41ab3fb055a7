"""-m gpu, round 5: the store-mode gradient exchange on the paths that cannot take the fused gather pass, the multi-rank
iteration with pose optimisation (mapping.BA) on, and the fused loop's never-drop capacity behaviour."""
import copy
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _scene(n=3000, views=6, seed=7):
    from splat_slam_amd import synthetic as syn
    intr = syn.INTRINSICS["tiny"]
    params = syn.room_parameters(n, seed=seed, device=DEV)
    params["scaling"] = params["scaling"] + 1.2          # make the splats a few pixels wide at 96x64
    cams = syn.make_views(params, views, intr, DEV, seed=seed)
    return syn, params, cams


def _config(syn, ba=False):
    cfg = copy.deepcopy(syn.DEFAULT_CONFIG)
    cfg["mapping"]["BA"] = bool(ba)
    return cfg


def _loop(cls, syn, params, cams, window, ba=False, **kw):
    loop = cls(_config(syn, ba), device=DEV, **kw)
    loop.gaussians = syn.model_from_parameters(params, device=DEV)
    loop.viewpoints = {c.uid: c for c in cams}
    loop.current_window = list(window)
    loop.build_keyframe_optimizers()
    return loop


@pytest.mark.parametrize("ba", [True, False])
def test_store_mode_holds_this_calls_sums_on_every_path(ba):
    """SgrMapStep.grads_clean = -3 promises that the sinks need not be zero on entry.  With pose gradients asked for (mapping.BA) the
    batch cannot take the fused gather pass, the accumulating passes run -- and used to ADD to whatever the sinks held (ADVICE r4:
    a ZeRO-1 run with BA on reduce-scattered g_t + g_(t-1) + ...).  Sinks filled with garbage + store mode must equal zeroed sinks +
    add mode bit for bit, on the fallback (BA) and on the fused path."""
    from splat_slam_amd import _native as nat
    from splat_slam_amd.fused import FusedMappingLoop
    syn, params, cams = _scene(n=3000, views=4)
    f = _loop(FusedMappingLoop, syn, params, cams, [0, 1, 2, 3], ba=ba)
    assert (f.keyframe_optimizers is not None) == ba
    f._ensure_state()
    f._activate()
    pl = f._plan()
    arr = f._views_array(cams[1:4], False)
    assert bool(arr[0].dL_dtau) == ba

    def run(mode, prefill):
        f._acc["flat"].fill_(prefill)
        st = f._setup(pl, 10.0, False, (), False, False, "none")
        st.num_views, st.views = 3, arr
        st.adam_groups, st.exp_rows, st.grads_clean = None, 0, mode
        sc, st.scaling = st.scaling, None            # (activations were written by _activate)
        ro, st.rotation = st.rotation, None
        op, st.opacity = st.opacity, None
        nat.check(f.lib.sgr_map_step(C.byref(st), f._stream()), "sgr_map_step")
        st.scaling, st.rotation, st.opacity = sc, ro, op
        torch.cuda.synchronize()
        return f._acc["flat"].clone()

    added = run(-2, 0.0)
    stored = run(-3, 7.0)
    assert added.abs().max().item() > 0
    assert torch.equal(added, stored)


def _mg_state(f, cams):
    gm = f.gaussians
    st = {g["name"]: gm.optimizer.state[g["params"][0]] for g in gm.optimizer.param_groups}
    out = {k: getattr(gm, k).detach().cpu().clone() for k in ["_xyz", "_features_dc", "_opacity", "_scaling", "_rotation"]}
    out.update({"m_" + k: st[k]["exp_avg"].detach().cpu().clone() for k in ["xyz", "f_dc", "opacity", "scaling", "rotation"]})
    out["exposure"] = f._exp.param[:8].detach().cpu().clone()
    out["R"] = torch.stack([torch.as_tensor(c.R).detach().cpu().float() for c in cams])
    out["T"] = torch.stack([torch.as_tensor(c.T).detach().cpu().float() for c in cams])
    return out


def _ba_worker(rank, world, port, out, sync):
    import os
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from splat_slam_amd.fused import FusedMappingLoop
    from splat_slam_amd.parallel import Comm
    syn, params, cams = _scene(n=2000, views=6, seed=21)
    f = _loop(FusedMappingLoop, syn, params, cams, [0, 1, 2, 3], ba=True)
    f.set_parallel(world, rank, split_views=True, sync=sync, comm=Comm(staged=True))
    f.iteration_count = 50
    torch.manual_seed(3)
    f.map(f.current_window, iters=4)
    torch.cuda.synchronize()
    out[rank] = _mg_state(f, cams)
    dist.destroy_process_group()


def _spawn2(fn, *args):
    import socket
    import torch.multiprocessing as mp
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    out = mp.Manager().dict()
    mp.spawn(fn, args=(2, port, out) + args, nprocs=2, join=True)
    return out[0], out[1]


def test_two_ranks_with_pose_optimisation_agree_bitwise_and_match_single_process():
    """mapping.BA on (pose deltas stepped every iteration: /root/reference/src/mapper.py:1076-1109, 561-567) over two ranks: the
    iteration never takes the fused gather pass, the sinks are exchanged every iteration (ZeRO-1 and all-reduce), the pose gradients
    of the views meet in their own small all-reduce.  Replicas must not drift (parameters, moments, exposures, camera poses), the two
    exchange variants must agree bit for bit, and four iterations must land where the single-process loop lands up to summation
    order -- a gradient buffer that accumulates across iterations (the defect) is off by whole Adam steps after the second one."""
    from splat_slam_amd.fused import FusedMappingLoop
    z0, z1 = _spawn2(_ba_worker, "zero1")
    for k in z0:
        assert torch.equal(z0[k], z1[k]), ("ranks differ", k)
    a0, _ = _spawn2(_ba_worker, "allreduce")
    for k in z0:
        assert torch.equal(z0[k], a0[k]), ("zero1 != allreduce", k)
    syn, params, cams = _scene(n=2000, views=6, seed=21)
    f = _loop(FusedMappingLoop, syn, params, cams, [0, 1, 2, 3], ba=True)
    f.iteration_count = 50
    torch.manual_seed(3)
    f.map(f.current_window, iters=4)
    torch.cuda.synchronize()
    single = _mg_state(f, cams)
    lr = {"_xyz": 9.6e-4, "_features_dc": 2.5e-3, "_opacity": 0.05, "_scaling": 6e-3, "_rotation": 1e-3}
    for k, step in lr.items():
        d = (z0[k] - single[k]).abs()
        assert (d > 0.02 * step).float().mean().item() < 0.01, (k, (d > 0.02 * step).float().mean().item())
    assert (z0["exposure"] - single["exposure"]).abs().max().item() < 2e-3
    assert (z0["R"] - single["R"]).abs().max().item() < 1e-4 and (z0["T"] - single["T"]).abs().max().item() < 1e-4
    assert (single["T"] - torch.stack([torch.as_tensor(c.T).cpu().float() for c in _scene(n=2000, views=6, seed=21)[2]])).abs().max().item() > 0, \
        "the poses did not move: BA was not exercised"


# ------------------------------------------------------------------------------------------------ never drop
def _dense_scene():
    from splat_slam_amd import synthetic as syn
    intr = syn.INTRINSICS["metric"]
    params = syn.room_parameters(60000, seed=5, device=DEV)
    params["scaling"] = params["scaling"] + 2.0          # > 65 536 (tile, Gaussian) pairs per view: more than the floor capacity
    cams = syn.make_views(params, 5, intr, DEV, seed=5)
    return syn, params, cams


def _full_state(f):
    gm = f.gaussians
    out = {k: getattr(gm, k).detach().clone() for k in ["_xyz", "_features_dc", "_opacity", "_scaling", "_rotation"]}
    for g in gm.optimizer.param_groups:
        st = gm.optimizer.state.get(g["params"][0])
        if st and g["params"][0].numel():
            out["m_" + g["name"]], out["v_" + g["name"]] = st["exp_avg"].detach().clone(), st["exp_avg_sq"].detach().clone()
            out["step_" + g["name"]] = torch.tensor(float(st["step"]))
    out["accum"], out["denom"], out["maxr"] = gm.xyz_gradient_accum.clone(), gm.denom.clone(), gm.max_radii2D.clone()
    out["exp_param"], out["exp_m"], out["exp_step"] = f._exp.param[:8].clone(), f._exp.m[:8].clone(), f._exp.step[:8].clone()
    out["occ"] = torch.stack([v for _, v in sorted(f.occ_aware_visibility.items())]).clone()
    out["flat"] = f._acc["flat"].clone()
    return out


def _sabotage(f, estimated):
    for vb in f._views.values():          # pretend every count had been measured on a nearly empty map
        vb.pairs, vb.estimated = 1, estimated
    f._cap = 1 << 16
    f._views_dirty()


def _drive(kind, sabotage, estimated=False, fresh_plan=False):
    import numpy as np
    from splat_slam_amd.fused import FusedMappingLoop
    syn, params, cams = _dense_scene()
    f = _loop(FusedMappingLoop, syn, params, cams, [0, 1, 2])
    f.iteration_count = 50
    torch.manual_seed(3)
    np.random.seed(3)
    f.map(f.current_window, iters=2)
    torch.cuda.synchronize()
    assert max(h[0] for h in f._pair_hint.values()) > (1 << 16)
    ev0 = f.overflow_events
    if sabotage:
        _sabotage(f, estimated)
    if fresh_plan:                 # the launch structs of the parameter set are made inside the transaction's first launch (what
        f._plan_key = None         # happens after every keyframe's new Gaussians): their step counters must follow a restore too
    if kind == "map":
        f.map(f.current_window, iters=4)
    elif kind == "map_three_spans":            # a keyframe's 60 iterations go out as 2 + 6 + 52: one transaction, three launches
        f.map(f.current_window, iters=20)
    elif kind == "prune_then_refine":          # single-step paths: a prune pass (gradients stay in the sinks), then final_refine
        f.map(f.current_window, prune=True, iters=1)
        if sabotage:
            _sabotage(f, estimated)
        f.final_refine(iters=5)
    elif kind == "per_iteration":              # no span calls: one sgr_map_step per iteration
        f.span_calls = False
        f.map(f.current_window, iters=3)
    torch.cuda.synchronize()
    return _full_state(f), f.overflow_events - ev0, f.replayed_transactions, f


@pytest.mark.parametrize("kind,estimated,fresh_plan", [("map", False, False), ("map", True, False), ("map", True, True), ("map_three_spans", False, True),
                                                       ("prune_then_refine", False, False), ("per_iteration", False, True)])
def test_fused_loop_with_a_tiny_capacity_ends_bitwise_where_the_ample_run_ends(kind, estimated, fresh_plan):
    """VERDICT r4 item 5 / SURVEY 8b ownership row: upstream's rasterizer never drops a view (it sizes its buffers inside the call).
    FusedMappingLoop learns of a truncated forward at its next check -- and then puts parameters, Adam moments, step counters,
    densification statistics and exposure rows back to where the transaction began, grows the workspace and issues the same
    iterations again.  Same seeds, one run with the capacity sabotaged down to the floor right before the iterations: every tensor
    of the optimisation must come out bit-identical to the ample-capacity run, with the overflow counted and nothing warned."""
    import warnings
    ample, ev_a, rp_a, _ = _drive(kind, False, fresh_plan=fresh_plan)
    assert ev_a == 0 and rp_a == 0
    with warnings.catch_warnings(record=True) as caught:      # (recorded, not turned into errors: an exception raised from inside
        warnings.simplefilter("always")                        #  a torch C++ call that holds no GIL terminates the process)
        tiny, ev_t, rp_t, f = _drive(kind, True, estimated, fresh_plan)
    assert not [w for w in caught if "capacity" in str(w.message)], [str(w.message) for w in caught]
    assert ev_t > 0 and rp_t > 0, (ev_t, rp_t)
    for k in ample:
        assert torch.equal(ample[k], tiny[k]), k
    assert f._cap > (1 << 16) and f.check_overflow() == []


def test_session_with_a_replayed_transaction_ends_bitwise_where_an_overflow_free_session_ends():
    """The same check one level up: 24 tracker frames through MappingSession (seeding, keyframe management, 60 + 1 iterations per
    keyframe, densification).  With the default capacity rule one view's estimate falls short once in this stretch: the transaction
    is replayed.  With a capacity floor no view reaches nothing overflows.  Map size and every parameter must agree bit for bit (this
    is the run that found the launch structs' step counters missing from the restore when the parameter set's structs are made inside
    the transaction -- which is the case after every keyframe's new Gaussians)."""
    import numpy as np
    from splat_slam_amd import synthetic as syn
    from splat_slam_amd.fused import FusedMappingLoop
    from splat_slam_amd.session import MappingSession
    intr = syn.INTRINSICS["metric"]
    NF = 24

    def run(floor):
        torch.manual_seed(43)
        np.random.seed(43)
        frames = syn.keyframe_stream(NF, intr, DEV, n_world=400000, seed=43, sweep_deg=360.0 * (NF - 1) / 160)
        torch.manual_seed(43)
        np.random.seed(43)
        loop = FusedMappingLoop(syn.DEFAULT_CONFIG, device=DEV)
        loop.capacity_floor = floor
        sess = MappingSession(loop, intr)
        status = [sess.process(*f) for f in frames]
        torch.cuda.synchronize()
        gm = loop.gaussians
        return ({k: getattr(gm, k).detach().clone() for k in ("_xyz", "_features_dc", "_opacity", "_scaling", "_rotation")},
                loop.overflow_events, loop.replayed_transactions, status)

    ample, ev_a, rp_a, st_a = run(1 << 22)
    tight, ev_t, rp_t, st_t = run(1 << 16)
    assert ev_a == 0 and rp_a == 0
    assert ev_t >= 1 and rp_t >= 1, "no overflow in this stretch any more: pick a stretch / floor that has one"
    assert st_a == st_t and st_a.count("mapped") >= 15
    for k in ample:
        assert ample[k].shape == tight[k].shape, (k, ample[k].shape, tight[k].shape)
        assert torch.equal(ample[k], tight[k]), k


# ------------------------------------------------------------------------------------------------ no depth-key hand-over, batched path
def test_batched_mapping_path_matches_an_oracle_that_sorts_by_its_own_depths():
    """the no-hand-over case of round 4 (tests/test_gpu_round4.py) runs the drop-in autograd API; this is the same
    discipline on the path bench.py times -- one sgr_map_views batch: fused tile kernel (forward + loss epilogue + backward in one
    wave), dense backward, gather with densification statistics.  The scene (configs[0] shape, one view) is first moved off every
    knife edge and every overlapping near tie in depth; the oracle then sorts by its OWN depths, radii must be equal, and every
    Gaussian's accumulated gradient and statistic is held to 1e-4 with no knife-edge list to hide behind."""
    from gpu_utils import move_off_knife_edges_and_depth_ties
    from oracle import raster_oracle as O
    from test_gpu_fullsize import _activated_inputs, _oracle_settings, _run_batched_case

    def prepare(syn, intr, params, cams):
        for attempt in range(4):
            gm = syn.model_from_parameters(params, device=DEV)
            inp = _activated_inputs(gm)
            s = _oracle_settings(cams[0], intr)
            if attempt:
                d = O.knife_edge_gaussians(inp["means3D"], inp["opacities"], shs=inp["shs"], scales=inp["scales"], rotations=inp["rotations"],
                                           settings=s, detail=True)
                if d["alpha"].numel() == 0 and d["geometric"].numel() == 0:
                    return                      # what the GPU activates from the raw parameters is off every edge
            move_off_knife_edges_and_depth_ties(inp, s)
            # back to raw parameters (fp32): xyz as is, logit / log of the activated values
            o = inp["opacities"].clamp(1e-6, 1 - 1e-6)
            params["xyz"] = inp["means3D"].float().to(DEV)
            params["opacity"] = torch.log(o / (1 - o)).float().to(DEV)
            params["scaling"] = torch.log(inp["scales"]).float().to(DEV)
        raise AssertionError("the raw parameters still activate onto a knife edge")

    _run_batched_case(20000, "replica", 1, prepare=prepare, own_depth_sort=True)


# ------------------------------------------------------------------------------------------------ never drop, several ranks
def _mg_overflow_worker(rank, world, port, out, sabotage_rank):
    import os
    import numpy as np
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from splat_slam_amd.fused import FusedMappingLoop
    from splat_slam_amd.parallel import Comm
    syn, params, cams = _dense_scene()
    f = _loop(FusedMappingLoop, syn, params, cams, [0, 1, 2, 3])
    f.set_parallel(world, rank, split_views=True, sync="zero1", comm=Comm(staged=True))
    f.iteration_count = 50
    torch.manual_seed(3)
    np.random.seed(3)
    f.map(f.current_window, iters=2)
    torch.cuda.synchronize()
    if rank == sabotage_rank:                  # ONE rank's capacity falls short: every rank must replay (the collectives are journaled)
        _sabotage(f, False)
    f.map(f.current_window, iters=3)
    torch.cuda.synchronize()
    st = _full_state(f)
    st["events"], st["replays"] = torch.tensor(float(f.overflow_events)), torch.tensor(float(f.replayed_transactions))
    out[rank] = {k: v.cpu() for k, v in st.items() if k != "flat"}
    dist.destroy_process_group()


def test_two_ranks_replay_together_when_one_rank_overflows():
    """ZeRO-1 over two ranks (views dealt round-robin).  Rank 1's capacity is sabotaged before three iterations: its check finds the
    truncated forwards, the flag is all-reduced, BOTH ranks put their state back and issue the span (with its reduce-scatter /
    all-gather) again.  Replicas stay bitwise equal, and equal to the run in which nobody overflowed."""
    a0, a1 = _spawn2(_mg_overflow_worker, -1)
    t0, t1 = _spawn2(_mg_overflow_worker, 1)
    assert a0["replays"].item() == 0 and a1["replays"].item() == 0
    assert t1["events"].item() > 0 and t0["events"].item() == 0
    assert t0["replays"].item() >= 1 and t1["replays"].item() >= 1, "both ranks replay"
    skip = ("events", "replays", "accum", "denom", "maxr")       # (densification statistics are per rank until a densification)
    for k in a0:
        if k in skip:
            continue
        assert torch.equal(t0[k], t1[k]), ("ranks differ", k)
        assert torch.equal(t0[k], a0[k]), ("replayed != overflow-free", k)
    for k in ("accum", "denom", "maxr"):
        assert torch.equal(t0[k], a0[k]) and torch.equal(t1[k], a1[k]), k


def test_session_with_systematically_short_estimates_replays_often_and_still_ends_bitwise_equal(monkeypatch):
    """Stress: every carried-over pair-count estimate is cut to a fifth (so that twice the estimate is still short), which makes
    the first transaction after most keyframes overflow -- across seeding, densification / pruning and an opacity reset.  30 tracker
    frames; the map must come out bit-identical to the session with a capacity floor that nothing reaches."""
    import numpy as np
    from splat_slam_amd import fused as fused_mod
    from splat_slam_amd import synthetic as syn
    from splat_slam_amd.session import MappingSession
    intr = syn.INTRINSICS["metric"]
    NF = 30
    real = fused_mod.estimate_pairs

    def run(floor, short):
        monkeypatch.setattr(fused_mod, "estimate_pairs", (lambda h, u, n: (None if real(h, u, n) is None else max(1, real(h, u, n) // 5))) if short else real)
        torch.manual_seed(43)
        np.random.seed(43)
        frames = syn.keyframe_stream(NF, intr, DEV, n_world=400000, seed=43, sweep_deg=360.0 * (NF - 1) / 160)
        torch.manual_seed(43)
        np.random.seed(43)
        loop = fused_mod.FusedMappingLoop(syn.DEFAULT_CONFIG, device=DEV)
        loop.capacity_floor = floor
        sess = MappingSession(loop, intr)
        status = []
        for f in frames:
            if short:              # the capacity only ever grows: forget it before every frame, so that the short estimates decide
                loop._cap = loop.capacity_floor
                loop._views_dirty()
            status.append(sess.process(*f))
        torch.cuda.synchronize()
        gm = loop.gaussians
        return ({k: getattr(gm, k).detach().clone() for k in ("_xyz", "_features_dc", "_opacity", "_scaling", "_rotation")},
                loop.overflow_events, loop.replayed_transactions, status)

    ample, ev_a, rp_a, st_a = run(1 << 22, False)
    short, ev_s, rp_s, st_s = run(1 << 12, True)
    print("replayed transactions with short estimates:", rp_s, "overflow events:", ev_s)
    assert ev_a == 0 and rp_a == 0 and rp_s >= 5, (rp_s, ev_s)
    assert st_a == st_s
    for k in ample:
        assert ample[k].shape == short[k].shape, (k, ample[k].shape, short[k].shape)
        assert torch.equal(ample[k], short[k]), k
