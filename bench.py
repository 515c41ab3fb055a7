#!/usr/bin/env python3
"""bench.py -- the reference's headline metric on MI355X: mapping frames/sec (+ render ms) at 640x480 / 300k Gaussians.

One STEP = one iteration of the keyframe mapping loop (/root/reference/src/mapper.py:414-568) on the synthetic room
(SURVEY.md 8d): 10 window views + 2 random views rendered forward AND backward through the HIP rasterizer, the
mapping loss per view, the isotropy regulariser, one Adam step on all Gaussian parameters (6 groups), the xyz lr
update, and the exposure (keyframe) Adam step.  A mapped keyframe costs 60 such iterations + 1 prune pass (forward +
backward, no optimiser step: configs/splat_slam.yaml:44, mapper.py:1113-1114), so  mapping frames/sec = steps/sec / 61.

`python bench.py --gpus N` with no WORLD_SIZE in the environment starts the N ranks itself (re-executes under
torch.distributed.run on 127.0.0.1); under the driver's own torch.distributed.run launch it is one of the ranks.  With
fewer GPUs than ranks (tests on a 1-GPU box) the ranks share the GPUs and exchange through host-staged gloo.

N > 1, --scaling strong (default): the 12 views of ONE iteration are split round-robin over the ranks -- the reference's
iteration, parallelised; gradients meet in one RCCL reduce-scatter, Adam runs on each rank's 1/N slice of the Gaussians,
an all-gather returns the parameters (ZeRO-1).  value = steps/sec / 61, no factor N.
--scaling weak: every rank renders its own 12 views (a 12*N-view batch per step); value = N * steps/sec / 61.

A plain run sets up, runs the event-timed kernel legs below (they are the iterations before the --warmup steps, so every run's
timed steps start from the same state), warms up, times the steps, writes --dump-outputs and prints the line.  Besides the headline
it carries (measured outside the headline's timed region):
  roofline            the fused tile kernel (forward + loss + backward of a tile in one wave): the dominant kernel of the timed loop
  roofline_unfused_blend_bwd   blend_bwd_kernel<true> -- the north-star kernel -- event-timed with the tile kernels UN-fused
  work_per_view       visible Gaussians, (tile, Gaussian) pairs and walked-list lengths per view
With --full the run then measures everything else (each trimmed by its own --no-* / --refine-iters option):
  roofline.traffic    HBM bytes and VALU issue of the two tile kernels from rocprofv3 --pmc child passes of this command
  render_ms, refine_iterations_per_s   single-view render timings and the final_refine rate (N > 1: `refine`, over the ranks)
  extra.session       40 tracker frames of the configs[1] session (MappingSession, default hyper-parameters): ms per keyframe, PSNR
  extra.session_full  the WHOLE configs[1] session (160 tracker frames once around the room): final map size, wall
                      ms per mapped keyframe / keyframes per s, PSNR over all keyframes, HIP- vs oracle-rendered PSNR of the final map
  dropin_keyframes_per_s   the same map() iteration through the drop-in autograd API (GaussianRasterizer per view, reference
                      loop structure intact, torch.optim.Adam)
  extra.opaque_scene  the same N with log-scale + 1.6: a converged, surface-covering map (long per-tile lists); roofline_opaque
  cpu_baseline        the oracle on the host cores, one view of the same scene

Prints ONE JSON line (rank 0).
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

T_START = time.perf_counter()          # (SPLAT_BENCH_TRACE times its messages from here: torch's import included)
ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

KINDS = ["preprocess_fwd", "tile_scan", "scatter", "blend_fused_fwd_loss_bwd", "blend_fwd_incl_tile_sort", "blend_bwd",
         "preprocess_bwd_incl_optimiser_pass"]
PK_FUSED, PK_FWD, PK_BWD = 3, 4, 5
HBM_PEAK_GBS = 8000.0          # MI355X_MICROARCH.md: 8 TB/s spec
FP32_PEAK_TFLOPS = 157.3
HIST_BINS = ["0", "1-4", "5-8", "9-16", "17-32", "33-64", "65-256", ">256"]


def trace(msg):
    if os.environ.get("SPLAT_BENCH_TRACE"):
        print("[trace] %.2f s" % (time.perf_counter() - T_START), msg, file=sys.stderr, flush=True)


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--gaussians", type=int, default=300000)
    ap.add_argument("--camera", default="metric", choices=["metric", "replica", "tiny"])
    ap.add_argument("--views", type=int, default=16, help="keyframes in the map (10 window + pool of random views)")
    ap.add_argument("--loop", default="fused", choices=["fused", "autograd"],
                    help="fused: autograd-free C-ABI sequence (product path); autograd: the drop-in autograd API per view")
    ap.add_argument("--scaling", default="strong", choices=["strong", "weak"], help="multi-GPU mode (see the module docstring)")
    ap.add_argument("--sync", default="zero1", choices=["zero1", "allreduce"],
                    help="multi-GPU gradient exchange: reduce-scatter + sliced Adam + all-gather, or one all-reduce + replicated Adam")
    ap.add_argument("--scale-add", type=float, default=0.0, help="added to every log-scale of the room (1.6 = opaque surfaces)")
    ap.add_argument("--order", default="random", choices=["random", "keyframe"],
                    help="order of the Gaussians in memory: random (worst case for the forward's per-segment view test) or the "
                         "order a SLAM session produces (keyframe after keyframe)")
    ap.add_argument("--full", action="store_true",
                    help="after the headline, also measure everything else the module docstring lists (PMC child passes, render and "
                         "refine timings, CPU baseline, drop-in / session / scene legs); --no-pmc, --refine-iters 0, --no-cpu-baseline "
                         "and --no-extras leave out their part")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-extras", action="store_true", help="skip the drop-in and opaque-scene legs")
    ap.add_argument("--refine-iters", type=int, default=200, help="final_refine iterations timed for refine it/s (0 = skip)")
    ap.add_argument("--profile-all", action="store_true", help="event-time every kernel kind inside the timed region (adds overhead)")
    ap.add_argument("--refine-views", default="world", help="views per optimiser step of the timed final_refine leg on N > 1 GPUs: "
                    "'world' (one random view per rank and step: configs[4]) or 1 (the reference's step, replicated)")
    ap.add_argument("--settle", type=int, default=0, help="extra untimed iterations right after the scene is built, BEFORE the --warmup steps "
                    "(rounds 3-5: 150, so that capacities, list hints, allocator pools and the GPU's clocks were settled; round 6: the "
                    "event-timed roofline legs run before the headline instead and this is 0 -- the line's `warmup` is all the warm-up "
                    "the headline gets beyond work the line reports anyway, see `iterations_before_timed_region`)")
    ap.add_argument("--no-pmc", action="store_true", help="do not start the rocprofv3 --pmc child passes that measure `roofline.traffic` "
                    "(HBM bytes of the dominant kernel, FETCH_SIZE / WRITE_SIZE)")
    ap.add_argument("--dry-run", action="store_true", help="launch / rendezvous / timing protocol only, no GPU work (CPU test of --gpus N)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the last timed step left a caller of map() (raw Gaussian parameters, "
                         "window visibility, exposure and pose deltas of every keyframe) as DIR/<name>.npy, at most 64 MB in all")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be at least 1")
    return args


def relaunch(args):
    """`python bench.py --gpus N` outside a launcher: become the launcher (one process per GPU, RCCL over xGMI inside)."""
    import socket
    import subprocess
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=%d" % args.gpus, "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    env.setdefault("OMP_NUM_THREADS", "4")
    return subprocess.call(cmd, env=env)


def dry_run(args):
    """The launch path without a GPU: rendezvous (gloo), the barrier-bracketed timed region, max over ranks, one line."""
    import torch.distributed as dist
    world, rank = int(os.environ.get("WORLD_SIZE", "1")), int(os.environ.get("RANK", "0"))
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        dist.init_process_group("gloo", rank=rank, world_size=world)
        dist.barrier()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        pass
    if world > 1:
        dist.barrier()
    t = torch.tensor([time.perf_counter() - t0], dtype=torch.float64)
    seen = torch.ones(1)
    if world > 1:
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        dist.all_reduce(seen)
    if rank == 0:
        print(json.dumps({"metric": "mapping frames/sec + render ms @640x480, 300k Gaussians; PSNR vs ref", "value": None, "dry_run": True,
                          "n_gpus": world, "ranks_seen": int(seen.item()), "steps": args.steps, "warmup": args.warmup,
                          "ms_per_step": round(1e3 * float(t.item()) / max(1, args.steps), 6),
                          "scaling": args.scaling if world > 1 else "none", "scaling_when_sharded": args.scaling, "full": args.full}))
    if world > 1:
        dist.destroy_process_group()


_PMC_BROKEN = []          # (a failed pass is not tried again in this run: a box whose profiler hangs must not cost the line minutes)


VALU_PEAK_GINST = 256 * 4 * 2.4 / 4.0          # G wave-instructions/s: 256 CUs x 4 SIMDs, one VALU instruction per 4 cycles at 2.4 GHz (the
                                                # clock at which 16 lanes x 2 flop x 2 (packed) give the guide's 157.3 TFLOP/s fp32 vector peak)
PMC_PASSES = (("FETCH_SIZE",), ("WRITE_SIZE",), ("SQ_WAVES", "SQ_INSTS_VALU", "SQ_ACTIVE_INST_VALU", "SQ_BUSY_CYCLES"))


def measure_counters(extra_args, kernels, timeout=90, passes=PMC_PASSES):
    """Counters of `kernels`, measured NOW: short rocprofv3 child passes of this same script (counters in their own runs, --pmc +
    --kernel-trace only, from /tmp: MI355X_MICROARCH.md), averaged over the batched (largest-grid) launches.
      hbm_bytes = (2 * FETCH_SIZE + WRITE_SIZE) * 1024 (gfx950 counts a 128-byte request as 64 in FETCH_SIZE; both are in KiB);
      valu_insts_per_wave = SQ_INSTS_VALU / SQ_WAVES, waves = the launch's grid in waves, valu_busy = SQ_ACTIVE_INST_VALU x 4 /
      (SQ_BUSY_CYCLES x 32 SIMDs per shader engine) -- the share of the launch during which a SIMD's VALU is issuing.
    Returns ({kernel: {...}}, how) -- ({}, reason) when rocprofv3 is not on this box or a pass fails."""
    import collections
    import csv
    import glob
    import shutil
    import subprocess
    import tempfile
    if shutil.which("rocprofv3") is None:
        return {}, "rocprofv3 not found on this box"
    if _PMC_BROKEN:
        return {}, _PMC_BROKEN[0]
    # never nest profilers: when this very process is being traced (somebody runs `rocprofv3 ... -- python bench.py`) its tool
    # environment would be inherited by the child passes -- a --pmc pass inside a --stats / trace pass is the combination the
    # GPU pool's launcher refuses
    if any(k.startswith(("ROCPROF", "ROCP_TOOL", "ROCPROFILER")) for k in os.environ) or "rocprof" in os.environ.get("LD_PRELOAD", ""):
        return {}, "this process runs under a profiler itself: no nested rocprofv3 passes"
    child = [sys.executable, os.path.abspath(__file__), "--steps", "12", "--warmup", "2", "--no-cpu-baseline", "--no-extras",
             "--refine-iters", "0", "--no-pmc"] + list(extra_args)
    env = dict(os.environ, TMPDIR="/tmp")
    vals = {}
    for counters in passes:
        d = tempfile.mkdtemp(prefix="bench_pmc_", dir="/tmp")
        try:
            r = subprocess.run(["rocprofv3", "--pmc"] + list(counters) + ["--kernel-trace", "--output-format", "csv", "-d", d, "-o", "p", "--"] + child,
                               cwd="/tmp", env=env, capture_output=True, text=True, timeout=timeout)
            files = glob.glob(os.path.join(d, "**", "*counter_collection.csv"), recursive=True)
            if r.returncode != 0 or not files:
                _PMC_BROKEN.append("rocprofv3 --pmc %s pass failed (rc %d)" % (" ".join(counters), r.returncode))
                return {}, _PMC_BROKEN[0]
            agg = collections.defaultdict(lambda: collections.defaultdict(list))
            for row in csv.DictReader(open(files[0])):
                if row["Counter_Name"] in counters:
                    agg[row["Kernel_Name"].split("(")[0].replace("void ", "")][row["Counter_Name"]].append((int(row["Grid_Size"]), float(row["Counter_Value"])))
            for k, cs in agg.items():
                for cn, v in cs.items():
                    g = max(x[0] for x in v)
                    sel = [x[1] for x in v if x[0] == g]
                    vals.setdefault(k, {})[cn] = sum(sel) / len(sel)
                    vals[k]["grid_threads"] = g
        except Exception as e:      # noqa: BLE001
            _PMC_BROKEN.append("rocprofv3 --pmc %s pass: %r" % (" ".join(counters), e))
            return {}, _PMC_BROKEN[0]
        finally:
            shutil.rmtree(d, ignore_errors=True)
    out = {}
    for want in kernels:
        for k, c in vals.items():
            if not k.endswith(want):
                continue
            o = {}
            if "FETCH_SIZE" in c and "WRITE_SIZE" in c:
                o["hbm_bytes"] = int((2.0 * c["FETCH_SIZE"] + c["WRITE_SIZE"]) * 1024)
            if c.get("SQ_WAVES") and "SQ_INSTS_VALU" in c:
                o["valu_insts_per_wave"] = round(c["SQ_INSTS_VALU"] / c["SQ_WAVES"], 1)
                o["waves"] = int(c["grid_threads"] // 64)
                if c.get("SQ_BUSY_CYCLES") and "SQ_ACTIVE_INST_VALU" in c:
                    o["valu_busy"] = round(c["SQ_ACTIVE_INST_VALU"] * 4.0 / (c["SQ_BUSY_CYCLES"] * 32.0), 4)
            if o:
                out[want] = o
    return out, ("measured by this run: rocprofv3 --pmc child passes (%s) of `bench.py %s` (batched launches; "
                 "bytes = (2 x FETCH_SIZE + WRITE_SIZE) x 1024, MI355X_MICROARCH.md)" % (" | ".join(" ".join(c) for c in passes), " ".join(child[2:])))


def apply_counters(roof, c, how):
    """Folds one kernel's measured counters into its roofline object.  With an instruction count the object states the bound the
    counters show -- VALU issue -- and keeps the SURVEY.md 8d byte formula and the measured traffic as HBM fractions of their own."""
    ms = roof["avg_launch_ms"]
    if "hbm_bytes" in c:
        roof["traffic"], roof["traffic_source"] = c["hbm_bytes"], how
        roof["traffic_over_algorithmic"] = round(c["hbm_bytes"] / roof["algorithmic_bytes"], 4)
        roof["hbm_frac_measured_traffic"] = round(c["hbm_bytes"] / (ms * 1e-3) / 1e9 / HBM_PEAK_GBS, 5) if ms > 0 else None
    if "valu_insts_per_wave" in c and ms > 0:
        ginst = c["valu_insts_per_wave"] * c["waves"] / (ms * 1e-3) / 1e9
        roof.update({"bound": "valu", "achieved": round(ginst, 2), "peak": round(VALU_PEAK_GINST, 1), "unit": "G wave-instructions/s",
                     "frac": round(ginst / VALU_PEAK_GINST, 5), "valu_instructions_per_wave": c["valu_insts_per_wave"],
                     "waves_per_launch": c["waves"], "valu_busy_share_of_launch": c.get("valu_busy"),
                     "bound_note": "SQ_INSTS_VALU x waves / launch time against 256 CUs x 4 SIMDs x 2.4 GHz / 4 cycles: the share of the chip's "
                                   "VALU issue slots this kernel fills (SQ_ACTIVE_INST_VALU says how long the VALUs are busy: transcendental "
                                   "and 64-bit instructions hold theirs longer than one slot).  hbm_frac_survey_formula = SURVEY.md 8d bytes / "
                                   "time / 8 TB/s (rounds 1-5 printed it as `frac`); hbm_frac_measured_traffic = the PMC traffic / time / 8 TB/s"})


class Bench:
    def __init__(self, args):
        self.args = args
        self.world = int(os.environ.get("WORLD_SIZE", "1"))
        self.rank = int(os.environ.get("RANK", "0"))
        local_rank = int(os.environ.get("LOCAL_RANK", "0"))
        assert torch.cuda.is_available(), "bench.py needs an MI355X (no CPU fallback in the product path)"
        ngpu = torch.cuda.device_count()
        local_world = int(os.environ.get("LOCAL_WORLD_SIZE", str(self.world)))
        # fewer GPUs than ranks (2 ranks on a 1-GPU box: tests): the ranks share GPUs, messages go through host memory (gloo)
        self.staged = local_world > ngpu
        local_rank = local_rank % ngpu
        torch.cuda.set_device(local_rank)
        self.dev = torch.device("cuda", local_rank)
        self.dist = None
        self.transport = "none"
        if self.world > 1:
            import torch.distributed as dist
            os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
            dist.init_process_group("gloo" if self.staged else "nccl", rank=self.rank, world_size=self.world)
            self.dist = dist
            self.transport = ("gloo, host-staged: %d ranks share %d GPU(s)" % (local_world, ngpu)) if self.staged else "RCCL (nccl backend)"
        from splat_slam_amd import _native as nat
        from splat_slam_amd import synthetic as syn
        self.nat, self.syn, self.lib = nat, syn, nat.lib()
        self.intr = syn.INTRINSICS[args.camera]

    # ------------------------------------------------------------------------------------------------ scene + loop
    def build(self, loop_kind, scale_add, seed_shift=0, order=None):
        """The room at `scale_add`, `views` keyframes around it, and a mapping loop in the state right after a densification
        point (149 iterations without map surgery follow: the metric is quoted AT 300k Gaussians)."""
        import numpy as np
        from splat_slam_amd.fused import FusedMappingLoop
        from splat_slam_amd.mapper import MappingLoop
        args, syn, dev = self.args, self.syn, self.dev
        torch.manual_seed(43)
        np.random.seed(43)
        params = syn.room_parameters(args.gaussians, seed=43, device=dev)
        if scale_add:
            params["scaling"] = params["scaling"] + scale_add
        if (order or args.order) == "keyframe":
            perm = syn.keyframe_order(params["xyz"]).to(dev)
            params = {k: v[perm].contiguous() for k, v in params.items()}
        # strong scaling: every rank holds the SAME views (it renders its share of them); weak: its own set
        seed = 43 + (self.rank if (self.world > 1 and args.scaling == "weak") else 0) + seed_shift
        cams = syn.make_views(params, args.views, self.intr, dev, seed=seed)
        loop = (FusedMappingLoop if loop_kind == "fused" else MappingLoop)(syn.DEFAULT_CONFIG, device=dev)
        loop.gaussians = syn.model_from_parameters(params, device=dev)
        loop.viewpoints = {c.uid: c for c in cams}
        loop.current_window = list(range(min(10, args.views)))
        loop.build_keyframe_optimizers()
        loop.iteration_count = 50
        if self.world > 1:
            if loop_kind == "fused":
                from splat_slam_amd.parallel import Comm
                loop.set_parallel(self.world, self.rank, split_views=(args.scaling == "strong"), sync=args.sync,
                                  comm=Comm(staged=self.staged))
            else:
                from splat_slam_amd.parallel import GradientSync
                loop.grad_sync = GradientSync(loop.gaussians, self.world)
        return loop, cams

    @staticmethod
    def run_steps(loop, k):
        """Exactly k iterations, driven the way the reference drives them: map(window, iters=...) calls (mapper.py:1113 uses
        iters=60; here up to 90 per call so that any k stays clear of the densification points)."""
        while k > 0:
            n = min(k, 90)
            loop.iteration_count = 50
            loop.map(loop.current_window, iters=n)
            k -= n

    def barrier(self):
        torch.cuda.synchronize()
        if self.dist is not None:
            self.dist.barrier()
        torch.cuda.synchronize()

    def timed(self, loop, steps):
        """(elapsed seconds MAX over ranks, seconds the host needed to enqueue)."""
        self.barrier()
        t0 = time.perf_counter()
        self.run_steps(loop, steps)
        host_issue = time.perf_counter() - t0
        self.barrier()
        elapsed = time.perf_counter() - t0
        if self.dist is not None:
            t = torch.tensor([elapsed], device="cpu" if self.staged else self.dev, dtype=torch.float64)
            self.dist.all_reduce(t, op=self.dist.ReduceOp.MAX)
            elapsed = float(t.item())
        return elapsed, host_issue

    def profiled(self, loop, steps, mask, fused_blend):
        """HIP-event times (on the launch stream) of the kernel kinds in `mask` over `steps` iterations."""
        lib, nat = self.lib, self.nat
        lib.sgr_set_option(nat.SGR_OPT_FUSED_BLEND, int(fused_blend))
        try:
            self.run_steps(loop, 3)
            torch.cuda.synchronize()
            lib.sgr_profile_enable(mask)
            self.run_steps(loop, steps)
            torch.cuda.synchronize()
            ms = (C.c_float * len(KINDS))()
            cnt = (C.c_int64 * len(KINDS))()
            lib.sgr_profile_read(ms, cnt)
        finally:
            lib.sgr_profile_enable(0)
            lib.sgr_set_option(nat.SGR_OPT_FUSED_BLEND, 1)
        return {i: (float(ms[i]) / max(1, int(cnt[i])), int(cnt[i])) for i in range(len(KINDS))}

    def work_counters(self, loop):
        """(V, R, R_eff, non-empty tiles) of every view of the last iteration + walked-list histogram of the last one."""
        nat, lib, intr = self.nat, self.lib, self.intr
        N = loop.gaussians.get_xyz.shape[0]
        stats, per_view = (C.c_int64 * 4)(), []
        stream = torch.cuda.current_stream(self.dev).cuda_stream
        for cam in loop.last_used:
            vb = loop.workspace_of(cam)            # (the random picks of a span render in shared workspace slots)
            ws = nat.SgrWorkspace(vb.saved.data_ptr(), vb.saved.numel(), vb.scratch.data_ptr(), vb.scratch.numel(), loop._cap)
            nat.check(lib.sgr_query_stats(C.byref(ws), N, intr["H"], intr["W"], loop._views[cam.uid].radii.data_ptr(), stats, stream), "sgr_query_stats")
            per_view.append([int(x) for x in stats])
        hist = (C.c_int64 * 8)()
        nat.check(lib.sgr_query_list_histogram(C.byref(ws), N, intr["H"], intr["W"], hist, stream), "sgr_query_list_histogram")
        return per_view, dict(zip(HIST_BINS, [int(x) for x in hist]))

    def rooflines(self, loop, per_view, steps):
        """blend_bwd (un-fused leg) and the fused tile kernel, each against its SURVEY.md 8d algorithmic bytes."""
        intr, N = self.intr, loop.gaussians.get_xyz.shape[0]
        HW, nv = intr["H"] * intr["W"], len(per_view)
        r_eff = sum(p[2] for p in per_view)
        unf = self.profiled(loop, steps, (1 << PK_FWD) | (1 << PK_BWD), fused_blend=False)
        fus = self.profiled(loop, steps, 1 << PK_FUSED, fused_blend=True)
        bwd_ms, bwd_n = unf[PK_BWD]
        fwd_ms, _ = unf[PK_FWD]
        fus_ms, fus_n = fus[PK_FUSED]
        bytes_bwd = 84 * r_eff + (24 * HW + 40 * N) * nv
        bytes_fwd = 48 * r_eff + 28 * HW * nv
        bytes_fused = bytes_bwd + bytes_fwd
        own_bytes = 92 * r_eff + 9 * HW * nv          # what the un-fused backward of this design moves
        pair_evals = r_eff * 64
        gbs = lambda b, ms: b / (ms * 1e-3) / 1e9 if ms > 0 else 0.0
        # PMC traffic comes from a separate rocprofv3 pass of this same command (committed under profiles/): it is only quoted when
        # that pass ran THIS workload and its kernel took the time it takes in this run (within 10 %); otherwise null
        def committed_traffic(kernel, ms_now):
            try:
                pm = json.load(open(os.path.join(ROOT, "profiles", "latest_pmc_hbm_bytes.json")))
                kt = json.load(open(os.path.join(ROOT, "profiles", "latest_kernel_batched_avg.json")))
                if pm.get("workload") != [N, intr["W"], intr["H"], nv]:
                    return None
                us = kt["kernels"][kernel]["avg_us"]
                if ms_now <= 0 or abs(us - 1e3 * ms_now) / (1e3 * ms_now) > 0.10:
                    return None
                return pm["kernels"][kernel]["hbm_bytes_per_launch_corrected"]
            except Exception:
                return None
        traffic = committed_traffic("sgr::blend_bwd_kernel<true>", bwd_ms)
        a = gbs(bytes_bwd, bwd_ms)
        # `traffic` is filled in by main() from rocprofv3 --pmc child passes of THIS run (measure_traffic); the committed profile's
        # figure is kept beside it under its own name
        roof = {"kernel": "blend_bwd_kernel<true>", "bound": "hbm", "achieved": round(a, 2), "peak": HBM_PEAK_GBS, "unit": "GB/s",
                "frac": round(a / HBM_PEAK_GBS, 5), "hbm_frac_survey_formula": round(a / HBM_PEAK_GBS, 5), "hbm_frac_measured_traffic": None,
                "traffic": None, "traffic_from_committed_profile": traffic, "in_timed_region": False,
                "traffic_source": "not measured (see main(): --no-pmc, or rocprofv3 missing); traffic_from_committed_profile = "
                                  "profiles/latest_pmc_hbm_bytes.json (scripts/collect_profiles.py on the builder's box), null unless "
                                  "that pass ran this workload and its kernel duration agrees with this run's within 10 %",
                "avg_launch_ms": round(bwd_ms, 5), "launches": bwd_n,
                "views_per_launch": nv, "algorithmic_bytes": bytes_bwd, "own_formula_bytes": own_bytes,
                "pixel_splat_pairs_per_launch": pair_evals,
                "valu_frac_at_60flop_per_pair": round(pair_evals * 60 / (bwd_ms * 1e-3) / 1e12 / FP32_PEAK_TFLOPS, 4) if bwd_ms > 0 else 0.0,
                "blend_fwd_avg_launch_ms": round(fwd_ms, 5),
                "note": "measured with SGR_OPT_FUSED_BLEND=0 (the two tile kernels launched separately) in this run; the headline "
                        "runs them fused (roofline_fused). Splat-list blending is VALU-issue bound (DESIGN.md 3): the HBM "
                        "fraction is small by construction"}
        af = gbs(bytes_fused, fus_ms)
        roof_f = {"kernel": "blend_fwd_kernel<*, FUSED=true> (forward + loss + backward of a tile in one wave)", "bound": "hbm",
                  "achieved": round(af, 2), "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": round(af / HBM_PEAK_GBS, 5),
                  "hbm_frac_survey_formula": round(af / HBM_PEAK_GBS, 5), "hbm_frac_measured_traffic": None, "traffic": None, "traffic_from_committed_profile": committed_traffic("sgr::blend_fwd_kernel<512, true>", fus_ms),
                  "in_timed_region": True, "traffic_source": roof["traffic_source"],
                  "avg_launch_ms": round(fus_ms, 5), "launches": fus_n, "views_per_launch": nv, "algorithmic_bytes": bytes_fused,
                  "algorithmic_bytes_formula": "SURVEY 8d: blend-bwd 84 R_eff + 24 HW + 40 N  +  blend-fwd 48 R_eff + 28 HW, per view",
                  "pixel_splat_pairs_per_launch": pair_evals,
                  "valu_frac_at_85flop_per_pair": round(pair_evals * 85 / (fus_ms * 1e-3) / 1e12 / FP32_PEAK_TFLOPS, 4) if fus_ms > 0 else 0.0,
                  "unfused_pair_avg_launch_ms": round(fwd_ms + bwd_ms, 5),
                  "note": "event-timed (HIP events on the launch stream, sgr_profile_enable) over this run's own iterations; the kernel is "
                          "VALU-issue bound (DESIGN.md 3): the HBM fraction is small by construction"}
        return roof, roof_f

    # ------------------------------------------------------------------------------------------------ legs
    def dropin_leg(self, steps=6, share_activations=True):
        """The same map() iteration through the drop-in autograd API: splat_slam_amd.mapper.MappingLoop keeps the reference's
        loop structure (render() per view -> GaussianRasterizer, loss, backward, torch.optim.Adam).
        share_activations=False: the scene model computes its activations anew on every getter call, like the reference's own
        GaussianModel (scene/gaussian_model.py:76-101) -- every render hands the rasterizer different tensor objects."""
        loop, cams = self.build("autograd", self.args.scale_add)
        loop.gaussians.share_activations = bool(share_activations)
        self.run_steps(loop, 6)
        # host-bound: one-off stalls of the first iterations (lazy kernel loads, allocator growth: tens of ms once) would swamp a
        # 6-iteration average -- the better of two timed blocks is the steady state
        blocks = [self.timed(loop, steps) for _ in range(2)]
        el = sum(b[0] for b in blocks) / len(blocks)            # the MEAN of the timed blocks (both are printed)
        host = sum(b[1] for b in blocks) / len(blocks)
        views = len(loop.current_window) + min(2, self.args.views - len(loop.current_window))
        ms_it = 1e3 * el / steps
        return {"dropin_keyframes_per_s": round((steps / el) / 61.0, 3), "ms_per_iteration": round(ms_it, 3),
                "timing": "mean of %d timed blocks of %d iterations after 6 warm-up iterations" % (len(blocks), steps),
                "ms_per_iteration_blocks": [round(1e3 * b[0] / steps, 3) for b in blocks],
                "ms_per_view_fwd_loss_bwd_incl_adam_share": round(ms_it / views, 4),
                "host_enqueue_ms_per_iteration": round(1e3 * host / steps, 3), "views_per_iteration": views}, loop, cams

    def order_leg(self, steps=30):
        """preprocess_fwd (K1) on the SAME room stored in keyframe order, with and without the per-segment view test."""
        loop, cams = self.build("fused", self.args.scale_add, order="keyframe")
        self.run_steps(loop, 10)
        el, _ = self.timed(loop, steps)
        res = {"ms_per_step": round(1e3 * el / steps, 4)}
        for name, on in (("preprocess_fwd_ms_with_segment_test", 1), ("preprocess_fwd_ms_without_segment_test", 0)):
            self.lib.sgr_set_option(self.nat.SGR_OPT_SEGMENT_TEST, on)
            try:
                res[name] = round(self.profiled(loop, 20, 1 << 0, fused_blend=True)[0][0], 5)
            finally:
                self.lib.sgr_set_option(self.nat.SGR_OPT_SEGMENT_TEST, 0)
        return res

    def scene_leg(self, scale_add, steps=40, order=None):
        loop, cams = self.build("fused", scale_add, order=order)
        self.run_steps(loop, 10)
        el, _ = self.timed(loop, steps)
        per_view, hist = self.work_counters(loop)
        roof, roof_f = self.rooflines(loop, per_view, 20)
        allk = self.profiled(loop, 20, (1 << len(KINDS)) - 1, fused_blend=True)      # (HIP events around every kernel: serialises them)
        nv = len(per_view)
        return {"scale_add": scale_add, "kernel_ms": {KINDS[i]: round(ms, 5) for i, (ms, n) in allk.items() if n}, "ms_per_step": round(1e3 * el / steps, 4), "keyframes_per_s": round((steps / el) / 61.0, 3),
                "visible_gaussians": sum(p[0] for p in per_view) // nv, "tile_pairs_R": sum(p[1] for p in per_view) // nv,
                "tile_pairs_walked_R_eff": sum(p[2] for p in per_view) // nv, "tiles_by_walked_list_length_last_view": hist,
                "blend_bwd_frac": roof["frac"], "blend_bwd_avg_launch_ms": roof["avg_launch_ms"],
                "blend_fwd_avg_launch_ms": roof["blend_fwd_avg_launch_ms"], "fused_tile_kernel_avg_launch_ms": roof_f["avg_launch_ms"],
                "fused_tile_kernel_frac": roof_f["frac"], "_roofline_fused": roof_f}


    def session_leg(self, frames_n=40, refine_iters=200, step_of=160, warm_frames=12):
        """The converged-map number under the driver's clock: the first `frames_n` tracker frames of the configs[1] session
        (scripts/run_session_config1.py: `step_of` frames around the room, default splat_slam.yaml hyper-parameters -- 1050
        initialisation iterations, 60 + 1 iterations per keyframe, densification, opacity resets, seeding of 1/32 of the
        pixels per keyframe, keyframe selection on n_touched) through MappingSession + FusedMappingLoop; then a short
        final_refine, the per-keyframe PSNR (eval_utils.py:90-123 protocol) and ONE view of the final map rendered by the HIP
        rasterizer and by the oracle (HIP-vs-oracle PSNR, SURVEY.md 8d item iv)."""
        import math
        import numpy as np
        from splat_slam_amd.fused import FusedMappingLoop
        from splat_slam_amd.session import MappingSession
        syn, dev, intr = self.syn, self.dev, self.intr
        torch.manual_seed(43)
        np.random.seed(43)
        t0 = time.perf_counter()
        frames = syn.keyframe_stream(frames_n, intr, dev, n_world=400000, seed=43, sweep_deg=360.0 * (frames_n - 1) / step_of)
        torch.cuda.synchronize()
        t_feed = time.perf_counter() - t0
        # an untimed throw-away session over the first frames first, like scripts/run_session_config1.py: a session's first keyframes
        # in a process pay allocator growth (hipMalloc of every workspace size once) and lazy code loading -- 227 vs 64 ms per
        # keyframe measured for the first and second half of a cold 40-frame session
        wl = FusedMappingLoop(syn.DEFAULT_CONFIG, device=dev)
        ws = MappingSession(wl, intr)
        for f in frames[:warm_frames]:
            ws.process(*f)
        torch.cuda.synchronize()
        del wl, ws
        torch.manual_seed(43)
        np.random.seed(43)
        loop = FusedMappingLoop(syn.DEFAULT_CONFIG, device=dev)
        sess = MappingSession(loop, intr)
        status, t_kf = [], []
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for f in frames:
            t1 = time.perf_counter()
            status.append(sess.process(*f))
            torch.cuda.synchronize()
            t_kf.append(time.perf_counter() - t1)
        t_map = time.perf_counter() - t0
        mapped = status.count("mapped")
        n_mapped = int(loop.gaussians.get_xyz.shape[0])
        t1 = time.perf_counter()
        scores = sess.finish(refine_iters=refine_iters)
        torch.cuda.synchronize()
        t_refine = time.perf_counter() - t1
        res = {"frames": frames_n, "keyframes_mapped": mapped, "skipped": status.count("skipped"),
               "ms_per_keyframe": round(1e3 * (t_map - t_kf[0]) / max(1, mapped), 3),
               "ms_per_mapped_keyframe": round(1e3 * (t_map - t_kf[0]) / max(1, mapped), 3),
               "keyframes_per_s": round(mapped / max(1e-9, t_map - t_kf[0]), 3),
               "ms_init_keyframe_1050_iterations": round(1e3 * t_kf[0], 1),
               "ms_per_keyframe_second_half": round(1e3 * sum(t for t, st in list(zip(t_kf, status))[frames_n // 2:] if st == "mapped")
                                                    / max(1, status[frames_n // 2:].count("mapped")), 3),
               "gaussians_final": int(loop.gaussians.get_xyz.shape[0]), "gaussians_after_mapping": n_mapped,
               "final_refine": {"iters": refine_iters, "it_per_s": round(refine_iters / t_refine, 1) if refine_iters else None},
               "psnr_all_keyframes_mean": round(float(np.mean(scores)), 3), "psnr_min": round(float(np.min(scores)), 3),
               "overflow_events": loop.overflow_events, "feed_s_rendering_ground_truth_untimed": round(t_feed, 2),
               "warmup_frames_untimed_throwaway_session": warm_frames,
               "ms_by_frame": [round(1e3 * t, 1) for t in t_kf] if frames_n <= 48 else None,
               "ms_per_keyframe_by_quarter": [round(1e3 * sum(t for t, st in list(zip(t_kf, status))[max(1, q * frames_n // 4):(q + 1) * frames_n // 4] if st == "mapped")
                                                    / max(1, status[max(1, q * frames_n // 4):(q + 1) * frames_n // 4].count("mapped")), 2) for q in range(4)],
               "note": ("the WHOLE configs[1] session as SURVEY.md 8d C1 states it: %d tracker frames once around the room, default "
                        "splat_slam.yaml hyper-parameters (mapper.py:834-1116), wall clock incl. seeding, densify / prune, keyframe management"
                        % frames_n) if frames_n >= step_of else
                       ("the first %d of the %d tracker frames of the configs[1] session (same angular step); includes seeding, "
                        "densify / prune, keyframe management; the whole session is extra.session_full" % (frames_n, step_of))}
        # ---- one view of the final map: HIP render vs oracle render (the oracle is the checker, never the product path)
        from oracle import raster_oracle as O
        from splat_slam_amd.mapper import PipelineParams
        from splat_slam_amd.renderer import render
        gm = loop.gaussians
        torch.set_num_threads(usable_cores())
        k = sorted(loop.viewpoints)[len(loop.viewpoints) // 2]
        cam = loop.viewpoints[k]

        def psnr(img, gt):
            mask = gt > 0                                             # eval_utils.py:109,123
            return float(20 * torch.log10(1.0 / torch.sqrt(((img[mask] - gt[mask]) ** 2).mean())))
        with torch.no_grad():
            inp = dict(means3D=gm.get_xyz.cpu(), opacities=gm.get_opacity.cpu(), shs=gm.get_features.cpu(), scales=gm.get_scaling.cpu(),
                       rotations=gm.get_rotation.cpu())
            img_h = render(cam, gm, PipelineParams(), loop.background)["render"].cpu()
            s = O.OracleSettings(intr["H"], intr["W"], math.tan(cam.FoVx * 0.5), math.tan(cam.FoVy * 0.5), torch.zeros(3), 1.0,
                                 cam.world_view_transform.cpu(), cam.full_proj_transform.cpu(), cam.projection_matrix.cpu(), 0,
                                 cam.camera_center.cpu(), False, False)
            img_o = O.rasterize(inp["means3D"], None, inp["opacities"], shs=inp["shs"], scales=inp["scales"],
                                rotations=inp["rotations"], settings=s)[0]
            ea, eb = (torch.exp(cam.exposure_a).item(), cam.exposure_b.item()) if k > 0 else (1.0, 0.0)      # eval_utils.py:96-99
            gt = cam.original_image.cpu()
            res["hip_vs_oracle_one_view"] = {
                "keyframe": int(k), "psnr_hip_render": round(psnr(torch.clamp(ea * img_h + eb, 0.0, 1.0), gt), 3),
                "psnr_oracle_render": round(psnr(torch.clamp(ea * img_o + eb, 0.0, 1.0), gt), 3),
                "image_max_abs_diff": round(float((img_h - img_o).abs().max()), 6)}
        return res


def main():
    args = parse()
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        sys.exit(relaunch(args))
    if args.dry_run:
        return dry_run(args)
    B = Bench(args)
    if B.world != args.gpus and B.rank == 0:
        print("[bench] --gpus %d but the launcher started %d rank(s): reporting n_gpus = %d" % (args.gpus, B.world, B.world), file=sys.stderr)
    world, rank, dev, intr, lib = B.world, B.rank, B.dev, B.intr, B.lib
    N = args.gaussians
    loop, cams = B.build(args.loop, args.scale_add)
    untimed = 0
    if args.settle:
        B.run_steps(loop, args.settle)
        untimed += args.settle
    trace("setup done")
    # The kernel-level legs of the line (event-timed rooflines of the fused tile kernel and of the un-fused pair) run BEFORE the
    # headline: they are part of what this script reports anyway, and after them workspace capacities, list hints, allocator pools and
    # the GPU's clocks are where a session has them from its second keyframe on -- rounds 3-5 reached that state with 150 extra untimed
    # iterations (--settle, now 0 by default) on top of the --warmup the caller asked for.  Then exactly --warmup untimed steps, then
    # exactly --steps timed ones.  `iterations_before_timed_region` counts everything this process ran before the clock started.
    per_view = hist = roof_bwd = roof_f = None
    if args.loop == "fused" and world == 1:
        B.run_steps(loop, 2)
        per_view, hist = B.work_counters(loop)
        roof_bwd, roof_f = B.rooflines(loop, per_view, 30)
        untimed += 2 + 2 * 33
        trace("rooflines done")
    if args.warmup:
        B.run_steps(loop, args.warmup)
        untimed += args.warmup
    trace("warmup done")
    if args.profile_all:
        lib.sgr_profile_enable((1 << len(KINDS)) - 1)
    elapsed, host_issue = B.timed(loop, args.steps)
    trace("timed loop done")
    if args.dump_outputs and rank == 0:
        dump_outputs(loop, args.dump_outputs)
    kernel_ms = None
    if args.profile_all:
        ms, cnt = (C.c_float * len(KINDS))(), (C.c_int64 * len(KINDS))()
        lib.sgr_profile_read(ms, cnt)
        lib.sgr_profile_enable(0)
        kernel_ms = {k: round(float(ms[i]) / max(1, int(cnt[i])), 5) for i, k in enumerate(KINDS) if int(cnt[i])}

    ms_per_step = 1e3 * elapsed / args.steps
    views_per_step = len(loop.current_window) + min(2, args.views - len(loop.current_window))
    weak = world > 1 and args.scaling == "weak"
    value = (world if weak else 1) * (args.steps / elapsed) / 61.0
    assert loop.gaussians.get_xyz.shape[0] == N, "N changed during the benchmark"

    out = {
        "metric": "mapping frames/sec + render ms @640x480, 300k Gaussians; PSNR vs ref",
        "value": round(value, 4), "unit": "mapped keyframes/s (61 map() iterations each)",
        "n_gpus": world, "steps": args.steps, "warmup": args.warmup, "ms_per_step": round(ms_per_step, 4),
        "higher_is_better": True, "scaling": args.scaling if world > 1 else "none", "scaling_when_sharded": args.scaling,
        "vs_baseline": None, "dtype": "f32",
        "data": "synthetic",
        "config": {"workload": "configs[1]-shaped: synthetic room (SURVEY 8d), %d Gaussians, %dx%d, %d views/step "
                               "(10 window + 2 random) fwd+bwd + loss + isotropy + Adam%s"
                               % (N, intr["W"], intr["H"], views_per_step * (world if weak else 1),
                                  "" if world == 1 else ("; views split over %d ranks" % world if not weak else "; %d views per rank" % views_per_step)),
                   "gaussians": N, "width": intr["W"], "height": intr["H"], "views_per_step": views_per_step * (world if weak else 1),
                   "loop": args.loop, "scale_add": args.scale_add,
                   "parallelism": "single GPU" if world == 1 else
                   ("view-parallel x%d, %s" % (world, "RCCL reduce-scatter + Adam on 1/%d of the Gaussians + all-gather (ZeRO-1)" % world
                                                 if args.sync == "zero1" else "one RCCL all-reduce of the flat gradient buffer"))},
        "host_enqueue_ms_per_step": round(1e3 * host_issue / args.steps, 4), "settle_iterations_untimed": args.settle,
        "iterations_before_timed_region": untimed,
        "map_iterations_per_s": round(args.steps / elapsed, 2),
        "world_size_seen": (B.dist.get_world_size() if B.dist is not None else 1), "transport": B.transport, "full": args.full,
    }
    if args.full and world > 1 and args.loop == "fused" and args.refine_iters > 0:
        # configs[4]: global map refinement over the ranks (mapper.py:656-708 with one random view per RANK and optimiser step,
        # ZeRO-1 exchange) -- renders/s of the whole job; --refine-views 1 times the reference's single-view step, replicated
        g = world if args.refine_views == "world" else int(args.refine_views)
        loop.final_refine(iters=5 * g, views_per_step=g)
        B.barrier()
        a = time.perf_counter()
        loop.final_refine(iters=args.refine_iters, views_per_step=g)
        B.barrier()
        dt = time.perf_counter() - a
        out["refine"] = {"views_per_step": g, "renders_per_s": round(args.refine_iters / dt, 1),
                         "optimiser_steps_per_s": round(args.refine_iters / g / dt, 1)}
    if kernel_ms is not None:
        out["kernel_ms"] = kernel_ms

    if args.loop == "fused":
        if per_view is None:
            per_view, hist = B.work_counters(loop)
        nv = len(per_view)
        out["work_per_view"] = {"visible_gaussians": sum(p[0] for p in per_view) // nv, "tile_pairs_R": sum(p[1] for p in per_view) // nv,
                                "tile_pairs_walked_R_eff": sum(p[2] for p in per_view) // nv,
                                "nonempty_tiles": sum(p[3] for p in per_view) // nv, "views_in_last_launch": nv,
                                "tiles_by_walked_list_length_last_view": hist}
    if args.loop == "fused" and world == 1:
        # `roofline` (the contract key) = the dominant kernel of the headline's timed region: the fused tile kernel;
        # `roofline_unfused_blend_bwd` = the north-star's kernel as a stand-alone launch (SGR_OPT_FUSED_BLEND = 0 leg of this run);
        # `roofline_fused` stays as an alias of `roofline` so that earlier rounds' readers find it
        out["roofline"], out["roofline_unfused_blend_bwd"], out["roofline_fused"] = roof_f, roof_bwd, roof_f
        if not args.full:
            for roof in (roof_f, roof_bwd):
                roof["traffic_source"] = "not measured: the PMC child passes run with --full; " + roof["traffic_source"]
    # ---- --full: everything besides the headline line's own keys (a plain run ends here)
    if args.full and args.loop == "fused" and world == 1:
        if not args.no_pmc:
            pass_args = ["--gaussians", str(N), "--camera", args.camera, "--views", str(args.views), "--scale-add", str(args.scale_add),
                         "--order", args.order]
            tr, how = measure_counters(pass_args, ["blend_fwd_kernel<512, true>", "blend_bwd_kernel<true>"])
            for roof, k in ((roof_f, "blend_fwd_kernel<512, true>"), (roof_bwd, "blend_bwd_kernel<true>")):
                if k in tr:
                    apply_counters(roof, tr[k], how)
                else:
                    roof["traffic_source"] = "not measured: %s; " % how + roof["traffic_source"]
        trace("rooflines done")
        # ---- single-render timings through the drop-in autograd API + the loop's own forward-only render
        from splat_slam_amd.mapper import PipelineParams
        from splat_slam_amd.renderer import render
        cam0, bg = cams[0], loop.background

        def rep(fn, reps=20):
            for _ in range(3):          # (first uses load kernels lazily: the second backward is the first to ACCUMULATE pose gradients)
                fn()
            torch.cuda.synchronize()
            a = time.perf_counter()
            for _ in range(reps):
                fn()
            torch.cuda.synchronize()
            return 1e3 * (time.perf_counter() - a) / reps

        def fwd_only():
            with torch.no_grad():
                render(cam0, loop.gaussians, PipelineParams(), bg)

        def fwd_bwd():
            pkg = render(cam0, loop.gaussians, PipelineParams(), bg)
            loop.loss_fn(loop.config["mapping"], pkg["render"], pkg["depth"], cam0, pkg["opacity"]).backward()
            loop.gaussians.optimizer.zero_grad(set_to_none=True)

        out["render_ms"] = {"forward": round(rep(fwd_only), 4), "forward_backward_loss": round(rep(fwd_bwd), 4),
                            "forward_fused_loop": round(rep(lambda: loop.render_forward(cam0), 50), 4),
                            "note": "forward / forward_backward_loss: ONE view through the drop-in autograd API (no host "
                                    "synchronisation, pooled workspaces); forward_fused_loop: FusedMappingLoop.render_forward"}
        if args.refine_iters > 0:     # mapper.py:656-708: ONE random view fwd+bwd + Adam on all N per iteration
            loop.final_refine(iters=5)
            torch.cuda.synchronize()
            a = time.perf_counter()
            loop.final_refine(iters=args.refine_iters)
            torch.cuda.synchronize()
            out["refine_iterations_per_s"] = round(args.refine_iters / (time.perf_counter() - a), 1)
        trace("render/refine done")
        if not args.no_cpu_baseline:
            out["cpu_baseline"] = cpu_baseline(loop, cams[0], intr, views_per_step)
        if not args.no_extras:          # (a failing extra must never cost the headline line)
            del loop
            torch.cuda.empty_cache()
            try:
                drop, dloop, dcams = B.dropin_leg()
                out["dropin_keyframes_per_s"] = drop.pop("dropin_keyframes_per_s")
                out["dropin"] = drop
                del dloop, dcams
                torch.cuda.empty_cache()
                # the same iteration under the reference's OWN scene model (activations recomputed per getter call): the renders of
                # an iteration join one batch by autograd provenance (dgr_native.cpp Batch::matches) instead of twelve batches of one
                ref, dloop, dcams = B.dropin_leg(share_activations=False)
                drop["reference_getters_ms_per_iteration"] = ref["ms_per_iteration"]
                drop["reference_getters_ms_per_iteration_blocks"] = ref["ms_per_iteration_blocks"]
                drop["reference_getters_keyframes_per_s"] = ref["dropin_keyframes_per_s"]
                del dloop, dcams
            except Exception as e:      # noqa: BLE001
                out.setdefault("dropin", {})["error"] = repr(e)
            trace("dropin done")
            torch.cuda.empty_cache()
            out["extra"] = {}
            for name, leg in (("session", B.session_leg), ("session_full", lambda: B.session_leg(frames_n=160, step_of=160, warm_frames=0)),
                              ("opaque_scene", lambda: B.scene_leg(args.scale_add + 1.6)), ("keyframe_ordered_map", B.order_leg),
                              ("opaque_scene_keyframe_ordered", lambda: B.scene_leg(args.scale_add + 1.6, order="keyframe"))):
                try:
                    out["extra"][name] = leg()
                except Exception as e:      # noqa: BLE001
                    out["extra"][name] = {"error": repr(e)}
                torch.cuda.empty_cache()
                trace(name + " done")

    ex = out.get("extra") or {}
    for leg in ex.values():
        if isinstance(leg, dict) and "_roofline_fused" in leg and leg is not ex.get("opaque_scene"):
            leg.pop("_roofline_fused")
    if isinstance(ex.get("opaque_scene"), dict) and "_roofline_fused" in ex["opaque_scene"]:
        # the converged-map fraction as a contract key of its own: the SAME kernel and formula as `roofline`, on the same N with
        # surface-covering splats (lists of 33-256 per tile: what a SLAM map is after a few hundred keyframes)
        ro = dict(ex["opaque_scene"].pop("_roofline_fused"))
        ro["workload"] = "same N, every log-scale + 1.6 (extra.opaque_scene): %d walked (tile, Gaussian) pairs per view" % ex["opaque_scene"]["tile_pairs_walked_R_eff"]
        if not args.no_pmc:
            tr, how = measure_counters(["--gaussians", str(N), "--camera", args.camera, "--views", str(args.views), "--scale-add",
                                        str(args.scale_add + 1.6), "--order", args.order], ["blend_fwd_kernel<512, true>"])
            if tr:
                apply_counters(ro, tr["blend_fwd_kernel<512, true>"], how)
        out["roofline_opaque"] = ro
    if ex:        # the headline scene is a FRESH map (mean list 11); what a converged map costs belongs next to the number
        out["value_context"] = {
            "headline_scene": "fresh map: ~18 k of 300 k Gaussians visible, ~54 k (tile, Gaussian) pairs per view, lists <= 32",
            "same_N_surface_covering_map_keyframes_per_s": (ex.get("opaque_scene") or {}).get("keyframes_per_s"),
            "same_N_surface_covering_map_ms_per_step": (ex.get("opaque_scene") or {}).get("ms_per_step"),
            "session_ms_per_keyframe_incl_seeding_densify_prune": (ex.get("session") or {}).get("ms_per_keyframe"),
            "session_keyframes_per_s": (round(1e3 / ex["session"]["ms_per_keyframe"], 2) if (ex.get("session") or {}).get("ms_per_keyframe") else None),
            "full_160_frame_session_keyframes_per_s": (ex.get("session_full") or {}).get("keyframes_per_s"),
            "full_160_frame_session_gaussians_final": (ex.get("session_full") or {}).get("gaussians_final")}
    if rank == 0:
        print(json.dumps(out))
    if B.dist is not None:
        B.dist.destroy_process_group()


DUMP_BUDGET_BYTES = 64 << 20


def dump_outputs(loop, out_dir, budget=DUMP_BUDGET_BYTES, seed=0):
    """What the timed path hands its caller after the last timed step, as float32 .npy files under `out_dir`: the raw Gaussian
    parameters (the optimiser's tensors), occ_aware_visibility of the window (one row per window keyframe, 0 / 1), and per keyframe
    (uid order) exposure a, b and the pose deltas.  Per-Gaussian arrays share one row set: all rows when they fit in `budget`,
    otherwise a fixed seeded sample whose row indices are written as gaussian_rows.npy (float64)."""
    import numpy as np
    gm = loop.gaussians
    n = gm._xyz.shape[0]
    per_gaussian = {"xyz": gm._xyz, "f_dc": gm._features_dc, "f_rest": gm._features_rest, "opacity": gm._opacity,
                    "scaling": gm._scaling, "rotation": gm._rotation}
    per_gaussian = {"gaussians_" + k: v.detach().reshape(n, -1) for k, v in per_gaussian.items() if v.numel() > 0}
    window = [kf for kf in loop.current_window if kf in loop.occ_aware_visibility]
    if window:
        per_gaussian["occ_aware_visibility"] = torch.stack([loop.occ_aware_visibility[kf].reshape(n) for kf in window], 1)
    cams = [loop.viewpoints[uid] for uid in sorted(loop.viewpoints)]

    def vec(t, k):
        return torch.zeros(k) if t is None else t.detach().reshape(k).float().cpu()

    small = {"keyframe_uids": torch.tensor([float(c.uid) for c in cams], dtype=torch.float64),
             "keyframe_exposure_ab": torch.stack([torch.cat([vec(c.exposure_a, 1), vec(c.exposure_b, 1)]) for c in cams]),
             "keyframe_pose_deltas": torch.stack([torch.cat([vec(c.cam_rot_delta, 3), vec(c.cam_trans_delta, 3)]) for c in cams])}
    row_bytes = 4 * sum(v.shape[1] for v in per_gaussian.values())
    room = budget - 4096 - sum(v.numel() * 8 for v in small.values())        # (4096: the .npy headers)
    if n * row_bytes > room:
        k = room // (row_bytes + 8)           # (+ 8: the float64 row index written beside the sample)
        rows = torch.randperm(n, generator=torch.Generator().manual_seed(seed))[:k].sort().values
        small["gaussian_rows"] = rows.double()
        per_gaussian = {name: v[rows.to(v.device)] for name, v in per_gaussian.items()}
    os.makedirs(out_dir, exist_ok=True)
    for name, v in per_gaussian.items():
        np.save(os.path.join(out_dir, name + ".npy"), v.float().cpu().numpy())
    for name, v in small.items():
        np.save(os.path.join(out_dir, name + ".npy"), v.cpu().numpy().astype(np.float64 if v.dtype == torch.float64 else np.float32))


def usable_cores():
    """Host threads we may really use: affinity mask clipped by the cgroup CPU quota (the GPU box exposes 256 cores
    behind a 16-CPU quota; asking torch for 256 threads there makes the oracle crawl)."""
    n = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    try:
        quota, period = open("/sys/fs/cgroup/cpu.max").read().split()
        if quota != "max":
            n = min(n, max(1, int(int(quota) / int(period))))
    except Exception:
        pass
    return max(1, n)


def cpu_baseline(loop, cam, intr, views_per_step):
    """Times oracle/raster_oracle.py (PyTorch CPU, fp32) forward+backward of ONE view of the same scene."""
    from oracle import raster_oracle as O
    import math
    ncores = usable_cores()
    torch.set_num_threads(ncores)
    gm = loop.gaussians
    with torch.no_grad():
        inp = dict(means3D=gm.get_xyz.detach().cpu(), opacities=gm.get_opacity.detach().cpu(),
                   shs=gm.get_features.detach().cpu(), scales=gm.get_scaling.detach().cpu(),
                   rotations=gm.get_rotation.detach().cpu())
        gt_img = cam.original_image.cpu()
        gt_dep = cam.depth.cpu()[None]
    s = O.OracleSettings(intr["H"], intr["W"], math.tan(cam.FoVx * 0.5), math.tan(cam.FoVy * 0.5), torch.zeros(3), 1.0,
                         cam.world_view_transform.cpu(), cam.full_proj_transform.cpu(), cam.projection_matrix.cpu(), 0,
                         cam.camera_center.cpu(), False, False)
    def once():
        x = {k: v.clone().requires_grad_(True) for k, v in inp.items()}
        m2d = torch.zeros_like(x["means3D"], requires_grad=True)
        t0 = time.perf_counter()
        col, radii, dep, opa, nt = O.rasterize(x["means3D"], m2d, x["opacities"], shs=x["shs"], scales=x["scales"],
                                               rotations=x["rotations"], theta=torch.zeros(3, requires_grad=True),
                                               rho=torch.zeros(3, requires_grad=True), settings=s)
        t1 = time.perf_counter()
        loss = 0.8 * (col - gt_img).abs().mean() + 0.2 * (dep - gt_dep).abs().mean()
        loss.backward()
        return t1 - t0, time.perf_counter() - t1

    once()                                              # warm-up (thread pool, allocator)
    runs = sorted((once() for _ in range(3)), key=lambda r: r[0] + r[1])
    t_fwd, t_bwd = runs[1]                              # the median run
    sec_view = t_fwd + t_bwd
    t0, t1, t2 = 0.0, t_fwd, sec_view
    return {"value": round(1.0 / (sec_view * views_per_step * 61.0), 6), "unit": "mapped keyframes/s (61 map() iterations each)",
            "cores": ncores, "kind": "port",
            "sample": "1 view (of the %d per step) forward+backward of the same %d-Gaussian scene through "
                      "oracle/raster_oracle.py (PyTorch CPU fp32, %d threads), 1 warm-up + median of 3; Adam excluded"
                      % (views_per_step, inp["means3D"].shape[0], ncores),
            "forward_s": round(t1 - t0, 3), "backward_s": round(t2 - t1, 3)}


if __name__ == "__main__":
    main()
