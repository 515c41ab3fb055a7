"""Mesh accuracy, completion and ICP alignment of eval_rendering's eval_mesh branch (/root/reference/src/utils/eval_utils.py:174-187:
run_evaluation(pred_ply, ..., "mesh", distance_thresh=0.05, full_path_to_gt_ply=gt_mesh, icp_align=True) of
evaluate_3d_reconstruction_lib), on the HIP kernels of csrc/sgr_mesh_eval.hip.  That library's source is not available: the metric
definitions below are assumptions, listed in DESIGN.md section 3 ("Mesh evaluation") and kept as the named constants and default
arguments of this module.

GPU tensors only: there is no CPU path (read_mesh_ply reads on the host and returns host tensors, like TriangleMesh.read_ply)."""
import math

import numpy as np
import torch

from splat_slam_amd import _native as nat
from splat_slam_amd.mesh import TriangleMesh

DISTANCE_THRESH = 0.05          # (A3) tau of precision / recall, metres (the reference's distance_thresh)
SAMPLES = 200_000               # (A1) points drawn from each mesh
ICP_THRESHOLD = 0.10            # (A2) ICP max_correspondence_distance, metres
ICP_MAX_ITERATION = 30          # (A2) Open3D's ICPConvergenceCriteria defaults
ICP_RELATIVE_FITNESS = 1e-6
ICP_RELATIVE_RMSE = 1e-6
GT_SEED_OFFSET = 1              # (A1) the ground truth is sampled with seed + 1, so a mesh compared with itself is not sampled twice alike


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _need_gpu(*tensors):
    for t in tensors:
        if t is not None and (not torch.is_tensor(t) or t.device.type != "cuda"):
            raise RuntimeError("splat_slam_amd.mesh_eval needs GPU tensors (HIP only, no CPU fallback)")


def _rows12(transform):
    """host 3x4 row-major float[12] of a 4x4 / 3x4 transform (None -> NULL: identity)"""
    if transform is None:
        return None
    m = torch.as_tensor(transform).detach().double().cpu()
    if tuple(m.shape) not in ((4, 4), (3, 4)):
        raise ValueError(f"transform must be 4x4 or 3x4, got {tuple(m.shape)}")
    if not bool(torch.isfinite(m).all()):
        raise ValueError("transform is not finite")
    return (nat.C.c_float * 12)(*[float(x) for x in m[:3].reshape(-1)])


def _points(p, what):
    _need_gpu(p)
    if p.dim() != 2 or p.shape[1] != 3:
        raise ValueError(f"{what}: points must be [n,3], got {tuple(p.shape)}")
    return p.detach().float().contiguous()


# ---- PLY input
_PLY_TYPES = {"char": "i1", "int8": "i1", "uchar": "u1", "uint8": "u1", "short": "i2", "int16": "i2", "ushort": "u2", "uint16": "u2",
              "int": "i4", "int32": "i4", "uint": "u4", "uint32": "u4", "float": "f4", "float32": "f4", "double": "f8",
              "float64": "f8"}


def _parse_header(data, path):
    if not data.startswith(b"ply"):
        raise ValueError(f"{path}: not a PLY file")
    end = data.find(b"end_header")
    if end < 0:
        raise ValueError(f"{path}: no end_header")
    nl = data.index(b"\n", end) + 1
    fmt, elements = None, []
    for line in data[:nl].decode("ascii", "replace").splitlines():
        w = line.split()
        if not w or w[0] in ("comment", "obj_info", "ply", "end_header"):
            continue
        if w[0] == "format":
            fmt = w[1]
        elif w[0] == "element":
            elements.append({"name": w[1], "count": int(w[2]), "props": []})
        elif w[0] == "property":
            if not elements:
                raise ValueError(f"{path}: property before any element")
            if w[1] == "list":
                elements[-1]["props"].append((w[4], ("list", _PLY_TYPES[w[2]], _PLY_TYPES[w[3]])))
            else:
                elements[-1]["props"].append((w[2], _PLY_TYPES[w[1]]))
    if fmt not in ("ascii", "binary_little_endian", "binary_big_endian"):
        raise ValueError(f"{path}: unsupported PLY format {fmt!r}")
    return fmt, elements, nl


def _fan(polys):
    """fan triangulation of index lists (polygons of fewer than 3 vertices dropped)"""
    out = [(p[0], p[i], p[i + 1]) for p in polys for i in range(1, len(p) - 1)]
    return np.asarray(out, dtype=np.int64).reshape(-1, 3)


def _read_binary_element(data, off, el, bo):
    """one element from `off`: (dict of scalar columns, list of per-record index lists or None, new offset)"""
    props, n = el["props"], el["count"]
    if all(not isinstance(t, tuple) for _, t in props):
        dt = np.dtype([(name, bo + t) for name, t in props])
        rec = np.frombuffer(data, dtype=dt, count=n, offset=off)
        return {name: rec[name] for name, _ in props}, None, off + n * dt.itemsize
    # a list property: the vectorised path when every list has the length of the first record's
    if n == 0:
        return {}, [], off
    first = []
    o = off
    for name, t in props:
        if isinstance(t, tuple):
            cnt = int(np.frombuffer(data, dtype=bo + t[1], count=1, offset=o)[0])
            first.append((name, t, cnt))
            o += np.dtype(t[1]).itemsize + cnt * np.dtype(t[2]).itemsize
        else:
            first.append((name, t, None))
            o += np.dtype(t).itemsize
    fields = []
    for name, t, cnt in first:
        if cnt is None:
            fields.append((name, bo + t))
        else:
            fields.append((name + "#n", bo + t[1]))
            if cnt:
                fields.append((name, bo + t[2], (cnt,)))
    dt = np.dtype(fields)
    if off + n * dt.itemsize <= len(data):
        rec = np.frombuffer(data, dtype=dt, count=n, offset=off)
        if all(cnt is None or (rec[name + "#n"] == cnt).all() for name, _, cnt in first):
            cols, lists = {}, None
            for name, t, cnt in first:
                if cnt is None:
                    cols[name] = rec[name]
                elif name in ("vertex_indices", "vertex_index"):
                    lists = rec[name].reshape(n, cnt) if cnt else np.zeros((n, 0), np.int64)
            return cols, lists, off + n * dt.itemsize
    # mixed polygon sizes: record by record
    cols = {name: [] for name, t in props if not isinstance(t, tuple)}
    lists = []
    o = off
    for _ in range(n):
        for name, t in props:
            if isinstance(t, tuple):
                cnt = int(np.frombuffer(data, dtype=bo + t[1], count=1, offset=o)[0])
                o += np.dtype(t[1]).itemsize
                idx = np.frombuffer(data, dtype=bo + t[2], count=cnt, offset=o)
                o += cnt * np.dtype(t[2]).itemsize
                if name in ("vertex_indices", "vertex_index"):
                    lists.append(idx.astype(np.int64).tolist())
            else:
                cols[name].append(np.frombuffer(data, dtype=bo + t, count=1, offset=o)[0])
                o += np.dtype(t).itemsize
    return {k: np.asarray(v) for k, v in cols.items()}, lists, o


def _read_ascii_element(tokens, pos, el):
    props, n = el["props"], el["count"]
    if all(not isinstance(t, tuple) for _, t in props):
        k = len(props)
        arr = np.asarray(tokens[pos:pos + n * k], dtype=np.float64).reshape(n, k)
        return {name: arr[:, j] for j, (name, _) in enumerate(props)}, None, pos + n * k
    cols = {name: [] for name, t in props if not isinstance(t, tuple)}
    lists = []
    for _ in range(n):
        for name, t in props:
            if isinstance(t, tuple):
                cnt = int(float(tokens[pos]))
                idx = [int(float(x)) for x in tokens[pos + 1:pos + 1 + cnt]]
                pos += 1 + cnt
                if name in ("vertex_indices", "vertex_index"):
                    lists.append(idx)
            else:
                cols[name].append(float(tokens[pos]))
                pos += 1
    return {k: np.asarray(v) for k, v in cols.items()}, lists, pos


def read_mesh_ply(path):
    """A triangle mesh from a PLY file in any of the three formats, as host tensors: x y z by name (other vertex properties
    ignored), red green blue when present (integers / 255, floats as they are; grey 0.5 otherwise), faces from a vertex_indices
    or vertex_index list of any count and index type, polygons fan-triangulated; elements other than vertex and face are skipped."""
    with open(path, "rb") as fh:
        data = fh.read()
    fmt, elements, off = _parse_header(data, path)
    verts = faces = None
    if fmt == "ascii":
        tokens = data[off:].split()
        pos = 0
    bo = "<" if fmt == "binary_little_endian" else ">"
    for el in elements:
        if fmt == "ascii":
            cols, lists, pos = _read_ascii_element(tokens, pos, el)
        else:
            cols, lists, off = _read_binary_element(data, off, el, bo)
        if el["name"] == "vertex":
            verts = (cols, dict(el["props"]))
        elif el["name"] == "face":
            if lists is None:
                raise ValueError(f"{path}: the face element has no vertex_indices / vertex_index list")
            faces = lists
        if verts is not None and faces is not None:
            break                                            # later elements are not read
    if verts is None:
        raise ValueError(f"{path}: no vertex element")
    cols, types = verts
    for k in "xyz":
        if k not in cols:
            raise ValueError(f"{path}: vertex property {k} missing")
    v = np.stack([np.asarray(cols[k], dtype=np.float64) for k in "xyz"], 1).astype(np.float32).reshape(-1, 3)
    if all(k in cols for k in ("red", "green", "blue")):
        c = np.stack([np.asarray(cols[k], dtype=np.float64) for k in ("red", "green", "blue")], 1)
        if not str(types["red"]).startswith("f"):
            c = c / 255.0
        c = c.astype(np.float32)
    else:
        c = np.full_like(v, 0.5)
    if faces is None:
        t = np.zeros((0, 3), np.int64)
    elif isinstance(faces, np.ndarray):
        t = faces.astype(np.int64)
        if t.shape[1] != 3:
            t = _fan(t.tolist()) if t.shape[1] > 3 else np.zeros((0, 3), np.int64)
    else:
        t = _fan(faces)
    if len(t) and (t.min() < 0 or t.max() >= len(v)):
        raise ValueError(f"{path}: face indices outside [0, {len(v)})")
    return TriangleMesh(torch.from_numpy(np.ascontiguousarray(v)), torch.from_numpy(t.astype(np.int32)), torch.from_numpy(c))


# ---- sampling
def _check_mesh(mesh, what):
    v, t = mesh.vertices, mesh.triangles
    _need_gpu(v, t)
    if v.dim() != 2 or v.shape[1] != 3 or t.dim() != 2 or t.shape[1] != 3:
        raise ValueError(f"{what}: vertices must be [V,3] and triangles [F,3], got {tuple(v.shape)}, {tuple(t.shape)}")
    V, F = int(v.shape[0]), int(t.shape[0])
    if V == 0 or F == 0:
        raise ValueError(f"{what}: empty mesh ({V} vertices, {F} triangles)")
    t = t.to(torch.int32).contiguous()
    if int(t.min()) < 0 or int(t.max()) >= V:
        raise ValueError(f"{what}: triangle indices outside [0, {V})")
    return v.detach().float().contiguous(), t


def _sample(mesh, n, seed, what):
    v, t = _check_mesh(mesh, what)
    lib = nat.lib()
    F = int(t.shape[0])
    nbytes = lib.sgr_surface_sample_bytes(F)
    scratch = torch.empty(nbytes, dtype=torch.uint8, device=v.device)
    total = torch.empty(1, dtype=torch.float64, device=v.device)
    pts = torch.empty(n, 3, dtype=torch.float32, device=v.device)
    tri = torch.empty(n, dtype=torch.int32, device=v.device)
    nat.check(lib.sgr_surface_sample(int(v.shape[0]), F, v.data_ptr(), t.data_ptr(), int(n), int(seed) & (2 ** 64 - 1),
                                     scratch.data_ptr(), nbytes, nat.ptr(pts) if n else None, nat.ptr(tri) if n else None,
                                     total.data_ptr(), _stream()), "sgr_surface_sample")
    area = float(total.cpu())
    if not area > 0.0:
        raise ValueError(f"{what}: the mesh has no triangle of positive area")
    return pts, tri, area


def sample_surface(mesh, n, seed=0):
    """n points drawn uniformly by area from the mesh's surface (fixed seed; the same seed gives the same points, bitwise, and
    sample i does not depend on n): (points f32 [n,3], face index i32 [n])"""
    if int(n) <= 0:
        raise ValueError(f"sample_surface: n must be > 0, got {n}")
    pts, tri, _ = _sample(mesh, int(n), seed, "sample_surface")
    return pts, tri


# ---- nearest neighbours
class PointGrid:
    """Exact nearest neighbours among `points` (f32 [n,3] on the GPU, n >= 1) through a uniform grid built once on the device;
    `transform` (4x4 or 3x4, host) moves the points before they are sorted in."""

    def __init__(self, points, transform=None):
        p = _points(points, "PointGrid")
        if p.shape[0] == 0:
            raise ValueError("PointGrid: no points")
        self.points, self.n = p, int(p.shape[0])
        self._lib = nat.lib()
        self._bytes = self._lib.sgr_nn_grid_bytes(self.n)
        self._grid = torch.empty(self._bytes, dtype=torch.uint8, device=p.device)
        nat.check(self._lib.sgr_nn_grid_build(self.n, p.data_ptr(), _rows12(transform), self._grid.data_ptr(), self._bytes, _stream()),
                  "sgr_nn_grid_build")

    def query(self, q, max_dist=math.inf, transform=None):
        """(dist f32 [m], idx i32 [m]) of the nearest point to each row of q (moved by `transform` first); ties go to the smaller
        index; where the distance exceeds max_dist, dist = inf and idx = -1"""
        q = _points(q, "PointGrid.query")
        if not float(max_dist) >= 0.0:
            raise ValueError(f"PointGrid.query: max_dist must be >= 0, got {max_dist}")
        m = int(q.shape[0])
        dist = torch.empty(m, dtype=torch.float32, device=q.device)
        idx = torch.empty(m, dtype=torch.int32, device=q.device)
        nat.check(self._lib.sgr_nn_query(self.n, self._grid.data_ptr(), self._bytes, m, q.data_ptr(), _rows12(transform),
                                         float(max_dist), dist.data_ptr(), idx.data_ptr(), _stream()), "sgr_nn_query")
        return dist, idx


# ---- ICP
def _kabsch(sums):
    """the rigid fit (Umeyama without scale) q ~ R p + t from sgr_icp_accumulate's 17 sums, fp64 4x4"""
    n = sums[0]
    mp, mq = sums[2:5] / n, sums[5:8] / n
    sigma = sums[8:17].reshape(3, 3).T / n - np.outer(mq, mp)          # cov(q, p)
    U, _, Vt = np.linalg.svd(sigma)
    S = np.eye(3)
    if np.linalg.det(U) * np.linalg.det(Vt) < 0:
        S[2, 2] = -1.0
    R = U @ S @ Vt
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = R, mq - R @ mp
    return T


def icp(source, target_grid, max_correspondence_distance=ICP_THRESHOLD, init=None, max_iteration=ICP_MAX_ITERATION,
        relative_fitness=ICP_RELATIVE_FITNESS, relative_rmse=ICP_RELATIVE_RMSE):
    """Point-to-point ICP of source (f32 [n,3], GPU) onto the points of target_grid (a PointGrid), as Open3D's registration_icp
    with TransformationEstimationPointToPoint: correspondences are nearest neighbours within max_correspondence_distance; each
    update is the Kabsch fit (reflection guarded) composed on the left in fp64; stops after max_iteration updates or when fitness
    and inlier RMSE both change by less than the relative criteria.  The source is never rewritten: every query moves it on the
    fly.  Returns {transformation (4x4 fp64 numpy), fitness, inlier_rmse, iterations}."""
    src = _points(source, "icp")
    if not isinstance(target_grid, PointGrid):
        raise TypeError("icp: target_grid must be a PointGrid")
    if not float(max_correspondence_distance) > 0.0:
        raise ValueError("icp: max_correspondence_distance must be > 0")
    lib = nat.lib()
    n = int(src.shape[0])
    T = np.eye(4) if init is None else np.asarray(torch.as_tensor(init).double().cpu(), dtype=np.float64).reshape(4, 4).copy()
    scratch = torch.empty(lib.sgr_eval_reduce_bytes(), dtype=torch.uint8, device=src.device)
    sums = torch.empty(17, dtype=torch.float64, device=src.device)

    def evaluate(T):
        rows = _rows12(T)
        _, idx = target_grid.query(src, max_dist=max_correspondence_distance, transform=T)
        nat.check(lib.sgr_icp_accumulate(n, src.data_ptr(), rows, idx.data_ptr(), target_grid.n, target_grid.points.data_ptr(),
                                         sums.data_ptr(), scratch.data_ptr(), scratch.numel(), _stream()), "sgr_icp_accumulate")
        s = sums.cpu().numpy()                    # the one read per iteration
        cnt = s[0]
        fit = cnt / n if n else 0.0
        rmse = math.sqrt(s[1] / cnt) if cnt > 0 else 0.0
        return s, fit, rmse

    s, fit, rmse = evaluate(T)
    it = 0
    for _ in range(int(max_iteration)):
        if s[0] < 3:                              # no rigid fit from fewer than three correspondences
            break
        T = _kabsch(s) @ T
        it += 1
        prev_fit, prev_rmse = fit, rmse
        s, fit, rmse = evaluate(T)
        if abs(prev_fit - fit) < relative_fitness and abs(prev_rmse - rmse) < relative_rmse:
            break
    return {"transformation": T, "fitness": float(fit), "inlier_rmse": float(rmse), "iterations": it}


# ---- metrics
def _as_mesh(m, device):
    if isinstance(m, TriangleMesh):
        return m
    mesh = read_mesh_ply(str(m))
    if device is not None:
        mesh = TriangleMesh(mesh.vertices.to(device), mesh.triangles.to(device), mesh.vertex_colors.to(device))
    return mesh


def _cloud(mesh, samples, seed, what):
    if samples is None:
        _sample(mesh, 0, seed, what)              # validation and the area check only
        return mesh.vertices.detach().float().contiguous()
    return _sample(mesh, samples, seed, what)[0]


def evaluate_mesh(pred, gt, distance_thresh=DISTANCE_THRESH, icp_align=True, samples=SAMPLES, seed=0, icp_threshold=ICP_THRESHOLD):
    """Accuracy, completion, completion ratio (recall), precision, F-score and chamfer-L1 of the predicted mesh against the
    ground-truth mesh (each a TriangleMesh on the GPU or a PLY path), in metres; DESIGN.md section 3 lists the definitions.
    `samples` points are drawn by area from each mesh (None: their vertices); with icp_align the predicted points are first
    aligned to the ground truth by point-to-point ICP (icp_threshold).  Returns a dict of the metrics, "icp" (icp()'s result or
    None), "distance_thresh" and "samples"."""
    if not float(distance_thresh) > 0.0:
        raise ValueError(f"evaluate_mesh: distance_thresh must be > 0, got {distance_thresh}")
    if samples is not None and int(samples) <= 0:
        raise ValueError(f"evaluate_mesh: samples must be > 0 or None, got {samples}")
    dev_of = lambda m: m.vertices.device if isinstance(m, TriangleMesh) else None
    dp, dg = dev_of(pred), dev_of(gt)
    fallback = torch.device("cuda", torch.cuda.current_device()) if (dp is None and dg is None and torch.cuda.is_available()) else None
    pred = _as_mesh(pred, dg or fallback)
    gt = _as_mesh(gt, dp or dg or fallback)
    if samples is not None:
        samples = int(samples)
    P = _cloud(pred, samples, seed, "evaluate_mesh (prediction)")
    G = _cloud(gt, samples, seed + GT_SEED_OFFSET, "evaluate_mesh (ground truth)")
    if P.device != G.device:
        raise ValueError("evaluate_mesh: the two meshes are on different devices")
    grid_g = PointGrid(G)
    reg, T = None, None
    if icp_align:
        reg = icp(P, grid_g, max_correspondence_distance=icp_threshold)
        T = reg["transformation"]
    d_pg, _ = grid_g.query(P, transform=T)
    d_gp, _ = PointGrid(P, transform=T).query(G)
    lib = nat.lib()
    scratch = torch.empty(lib.sgr_eval_reduce_bytes(), dtype=torch.uint8, device=P.device)
    out = torch.empty(4, dtype=torch.float64, device=P.device)
    nat.check(lib.sgr_cloud_metrics(int(d_pg.numel()), d_pg.data_ptr(), int(d_gp.numel()), d_gp.data_ptr(), float(distance_thresh),
                                    out.data_ptr(), scratch.data_ptr(), scratch.numel(), _stream()), "sgr_cloud_metrics")
    s_pg, c_pg, s_gp, c_gp = out.cpu().tolist()
    n_p, n_g = int(d_pg.numel()), int(d_gp.numel())
    acc, comp = s_pg / n_p, s_gp / n_g
    prec, rec = c_pg / n_p, c_gp / n_g
    fscore = 2.0 * prec * rec / (prec + rec) if (prec + rec) > 0 else 0.0
    return {"accuracy": acc, "completion": comp, "completion_ratio": rec, "precision": prec, "recall": rec, "fscore": fscore,
            "chamfer_l1": 0.5 * (acc + comp), "icp": reg, "distance_thresh": float(distance_thresh), "samples": samples}


__all__ = ["read_mesh_ply", "sample_surface", "PointGrid", "icp", "evaluate_mesh"]
