"""fp64 numpy restatement of the mesh evaluation of splat_slam_amd.mesh_eval ("Mesh evaluation"): exact
nearest neighbours (brute force in row chunks; scipy's cKDTree for large clouds where scipy is installed), the Kabsch / Umeyama
rigid fit, point-to-point ICP as Open3D's registration_icp, and the accuracy / completion metrics.  Tests only."""
import math

import numpy as np


def nearest(query, target):
    """(fp64 distance, smallest index among the nearest) of every query row against the target rows, brute force in row chunks
    of about 50 MB"""
    q = np.asarray(query, np.float64).reshape(-1, 3)
    t = np.asarray(target, np.float64).reshape(-1, 3)
    chunk = max(1, 2_000_000 // max(1, len(t)))
    dist = np.empty(len(q))
    idx = np.empty(len(q), np.int64)
    for a in range(0, len(q), chunk):
        d2 = ((q[a:a + chunk, None, :] - t[None, :, :]) ** 2).sum(-1)
        j = np.argmin(d2, 1)                       # argmin: the first (smallest) index of the minimum
        idx[a:a + chunk] = j
        dist[a:a + chunk] = np.sqrt(d2[np.arange(len(j)), j])
    return dist, idx


def nearest_large(query, target):
    """fp64 nearest distances through scipy's cKDTree (None where scipy is not installed)"""
    try:
        from scipy.spatial import cKDTree
    except ImportError:
        return None
    d, i = cKDTree(np.asarray(target, np.float64)).query(np.asarray(query, np.float64), k=1)
    return d, i


def kabsch(p, q):
    """R, t minimising sum |R p + t - q|^2 (no scale; det < 0 flips the last singular vector), fp64"""
    p = np.asarray(p, np.float64)
    q = np.asarray(q, np.float64)
    mp, mq = p.mean(0), q.mean(0)
    sigma = (q - mq).T @ (p - mp) / len(p)
    U, _, Vt = np.linalg.svd(sigma)
    S = np.eye(3)
    if np.linalg.det(U) * np.linalg.det(Vt) < 0:
        S[2, 2] = -1.0
    R = U @ S @ Vt
    return R, mq - R @ mp


def transform(T, p):
    return np.asarray(p, np.float64) @ T[:3, :3].T + T[:3, 3]


def transform_f32(T, p):
    """what the kernels form: fp32 rows of [R | t] applied in fp32"""
    m = np.asarray(T, np.float64)[:3].astype(np.float32)
    p = np.asarray(p, np.float32)
    return (m[:, 0] * p[:, :1] + m[:, 1] * p[:, 1:2] + m[:, 2] * p[:, 2:3] + m[:, 3]).astype(np.float32)


def icp(source, target, max_dist=0.1, max_iteration=30, relative_fitness=1e-6, relative_rmse=1e-6, nn=None):
    """point-to-point ICP of source onto target from the identity, Open3D's loop: evaluate, then per iteration fit, compose on the
    left, re-evaluate, stop when fitness and inlier RMSE both change by less than the criteria.  nn(query, target) -> (dist, idx)"""
    nn = nn or nearest
    src = np.asarray(source, np.float32)
    tgt = np.asarray(target, np.float64)
    T = np.eye(4)

    def evaluate(T):
        p = transform_f32(T, src).astype(np.float64)
        d, j = nn(p, tgt)
        ok = d <= max_dist
        cnt = int(ok.sum())
        fit = cnt / len(src)
        rmse = math.sqrt((d[ok] ** 2).sum() / cnt) if cnt else 0.0
        return p[ok], tgt[j[ok]], fit, rmse

    p, q, fit, rmse = evaluate(T)
    it = 0
    for _ in range(max_iteration):
        if len(p) < 3:
            break
        R, t = kabsch(p, q)
        U = np.eye(4)
        U[:3, :3], U[:3, 3] = R, t
        T = U @ T
        it += 1
        pf, pr = fit, rmse
        p, q, fit, rmse = evaluate(T)
        if abs(pf - fit) < relative_fitness and abs(pr - rmse) < relative_rmse:
            break
    return {"transformation": T, "fitness": fit, "inlier_rmse": rmse, "iterations": it}


def metrics(d_pg, d_gp, tau):
    """accuracy, completion, ratios, F-score and chamfer-L1 from the two distance arrays"""
    d_pg = np.asarray(d_pg, np.float64)
    d_gp = np.asarray(d_gp, np.float64)
    prec, rec = float((d_pg < tau).mean()), float((d_gp < tau).mean())
    acc, comp = float(d_pg.mean()), float(d_gp.mean())
    return {"accuracy": acc, "completion": comp, "completion_ratio": rec, "precision": prec, "recall": rec,
            "fscore": 2 * prec * rec / (prec + rec) if prec + rec > 0 else 0.0, "chamfer_l1": 0.5 * (acc + comp)}


def rotation(axis, deg):
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    th = math.radians(deg)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + math.sin(th) * K + (1 - math.cos(th)) * K @ K


def box_mesh(lo, hi, n=8):
    """the closed surface of the box [lo, hi] as a grid of n x n quads per face (two triangles each): vertices, triangles"""
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    verts, tris = [], []
    for axis in range(3):
        u, v = [k for k in range(3) if k != axis]
        for side in (0, 1):
            base = len(verts)
            for i in range(n + 1):
                for j in range(n + 1):
                    p = np.empty(3)
                    p[axis] = hi[axis] if side else lo[axis]
                    p[u] = lo[u] + (hi[u] - lo[u]) * i / n
                    p[v] = lo[v] + (hi[v] - lo[v]) * j / n
                    verts.append(p)
            for i in range(n):
                for j in range(n):
                    a, b, c, d = base + i * (n + 1) + j, base + (i + 1) * (n + 1) + j, base + (i + 1) * (n + 1) + j + 1, base + i * (n + 1) + j + 1
                    tris += [(a, b, c), (a, c, d)]
    return np.array(verts), np.array(tris, np.int64)


def room_mesh(n=16):
    """a non-symmetric room: a 4 x 3 x 2.5 m box with two inner boxes of different sizes"""
    parts = [box_mesh((-2.0, -1.5, 0.0), (2.0, 1.5, 2.5), n), box_mesh((0.6, -1.2, 0.0), (1.5, -0.4, 0.9), n // 2),
             box_mesh((-1.6, 0.3, 0.0), (-1.1, 1.2, 1.6), n // 2)]
    v, t, off = [], [], 0
    for pv, pt in parts:
        v.append(pv)
        t.append(pt + off)
        off += len(pv)
    return np.concatenate(v), np.concatenate(t)
