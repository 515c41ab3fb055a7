"""GPU box: HIP-event times of the mesh evaluation (csrc/sgr_mesh_eval.hip, splat_slam_amd.mesh_eval): area-weighted sampling, grid
build and nearest-neighbour queries at 200 k x 200 k and 200 k x 1 M points, a "misaligned" query set with 10 % of its points 1 m
outside the target's box, and a whole evaluate_mesh with ICP of the synthetic room's TSDF mesh against its box walls; for context,
scipy's cKDTree on the host for the same queries where scipy is installed.  Writes one JSON file.

    python scripts/mesh_eval_times.py [--out profiles/mesh_eval_times.json] [--reps 5]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
DEV = "cuda:0"


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), out


def median_ms(fn, reps):
    fn()                                            # warm-up
    return float(np.median([event_ms(fn)[0] for _ in range(reps)]))


def room_mesh_gpu(n=64):
    import mesh_eval_ref as ref
    from splat_slam_amd.mesh import TriangleMesh
    v, t = ref.room_mesh(n)
    v = torch.from_numpy(v.astype(np.float32)).to(DEV)
    return TriangleMesh(v, torch.from_numpy(t.astype(np.int32)).to(DEV), torch.full_like(v, 0.5))


def host_kdtree_ms(target, query):
    try:
        from scipy.spatial import cKDTree
    except ImportError:
        return None
    t, q = target.cpu().numpy().astype(np.float64), query.cpu().numpy().astype(np.float64)
    t0 = time.perf_counter()
    tree = cKDTree(t)
    t1 = time.perf_counter()
    tree.query(q, k=1, workers=int(os.environ.get("OMP_NUM_THREADS", "1")))
    t2 = time.perf_counter()
    return {"build_ms": (t1 - t0) * 1e3, "query_ms": (t2 - t1) * 1e3}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mesh_eval_times.json"))
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    from splat_slam_amd.mesh_eval import PointGrid, evaluate_mesh, sample_surface
    mesh = room_mesh_gpu()
    out = dict(device=torch.cuda.get_device_name(0), mesh_triangles=int(mesh.triangles.shape[0]))
    out["sample_200k_ms"] = median_ms(lambda: sample_surface(mesh, 200_000, seed=0), args.reps)
    out["sample_1M_ms"] = median_ms(lambda: sample_surface(mesh, 1_000_000, seed=1), args.reps)
    q200 = sample_surface(mesh, 200_000, seed=2)[0]
    rows = {}
    for name, n in (("200k", 200_000), ("1M", 1_000_000)):
        tgt = sample_surface(mesh, n, seed=3)[0]
        grid = PointGrid(tgt)
        r = {"build_ms": median_ms(lambda: PointGrid(tgt), args.reps),
             "query_ms": median_ms(lambda: grid.query(q200), args.reps),
             "query_max_dist_0.1_ms": median_ms(lambda: grid.query(q200, max_dist=0.1), args.reps)}
        mis = q200.clone()
        k = mis.shape[0] // 10
        mis[:k, 0] = 2.0 + 1.0                      # 10 %: 1 m beyond the room's +x wall (x = 2)
        r["query_misaligned_ms"] = median_ms(lambda: grid.query(mis), args.reps)
        r["host_ckdtree"] = host_kdtree_ms(tgt, q200)
        rows[f"200k_x_{name}"] = r
    out["nn"] = rows
    # the synthetic room session's TSDF mesh against its box walls (tests/test_gpu_mesh_eval.py)
    import mesh_eval_ref as ref
    from splat_slam_amd import synthetic as syn
    from splat_slam_amd.mesh import TriangleMesh
    from test_gpu_mesh_eval import _room_session
    sess = _room_session()
    pred = sess.evaluate(mesh=True)["mesh"]
    half = np.array(syn.ROOM) / 2
    v, t = ref.box_mesh(-half, half, 64)
    vv = torch.from_numpy(v.astype(np.float32)).to(DEV)
    walls = TriangleMesh(vv, torch.from_numpy(t.astype(np.int32)).to(DEV), torch.full_like(vv, 0.5))
    res = {}
    ms = median_ms(lambda: res.update(evaluate_mesh(pred, walls)), args.reps)
    # its parts: the two sample sets, ICP alone, and each direction's query after alignment
    from splat_slam_amd.mesh_eval import GT_SEED_OFFSET, SAMPLES, icp
    P = sample_surface(pred, SAMPLES, seed=0)[0]
    G = sample_surface(walls, SAMPLES, seed=GT_SEED_OFFSET)[0]
    grid_g = PointGrid(G)
    T = res["icp"]["transformation"]
    parts = {"icp_ms": median_ms(lambda: icp(P, grid_g), args.reps),
             "query_pred_to_gt_ms": median_ms(lambda: grid_g.query(P, transform=T), args.reps)}
    grid_p = PointGrid(P, transform=T)
    parts["query_gt_to_pred_ms"] = median_ms(lambda: grid_p.query(G), args.reps)
    out["evaluate_mesh_room"] = dict(ms=ms, pred_vertices=len(pred), pred_triangles=int(pred.triangles.shape[0]),
                                     icp_iterations=res["icp"]["iterations"], parts=parts,
                                     metrics={k: res[k] for k in ("accuracy", "completion", "precision", "completion_ratio",
                                                                   "fscore", "chamfer_l1")})
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
