"""-m gpu: the kernels of csrc/sgr_mesh.hip at their edges, on the cases of tests/mesh_cases.py (tests/test_mesh_cpu.py proves, without
a GPU, that each case is what it claims to be, so nothing is excluded here): marching cubes on noise, holes, missing units and exact
zeros; the scans across their 4096-item blocks and their 256-sum carry round; integration across its 16-frame chunks and across the
growth of the hash and the pool, bit for bit; the colour byte's separate roundings; clean_mesh on faces it has to drop."""
import numpy as np
import pytest
import torch

import mesh_cases as MC
import mesh_ref as ref
import test_gpu_mesh as base                     # its frames, its volumes and its criterion _compare_volumes

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
VL, TRUNC = 0.02, 0.06
VL32 = float(np.float32(VL))                     # the voxel length the kernels compute with


def _vol(vox, vl=VL, **kw):
    from splat_slam_amd.mesh import TSDFVolume
    return TSDFVolume.from_voxels(vox, vl, TRUNC, device=DEV, **kw)


def _bits(t):
    return t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t


def _same_bits(a, b):
    """tensors, TriangleMeshes or voxels() dicts: same shapes and the same bits (so -0.0 is not 0.0)"""
    if isinstance(a, dict):
        return a.keys() == b.keys() and all(_same_bits(a[k], b[k]) for k in a)
    if not torch.is_tensor(a):
        return all(_same_bits(getattr(a, n), getattr(b, n)) for n in ("vertices", "triangles", "vertex_colors"))
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(_bits(a), _bits(b))


def _dev(vox):
    return {k: torch.as_tensor(v).to(DEV) for k, v in vox.items()}


def _mesh_np(m):
    return m.vertices.cpu().numpy(), m.triangles.cpu().numpy().astype(np.int64), m.vertex_colors.cpu().numpy()


def _no_boundary(tris):
    """every directed edge a -> b (a != b) is used as often as b -> a"""
    e = np.concatenate([tris[:, [0, 1]], tris[:, [1, 2]], tris[:, [2, 0]]]).astype(np.int64)
    e = e[e[:, 0] != e[:, 1]]
    n = int(e.max()) + 1
    return np.array_equal(np.sort(e[:, 0] * n + e[:, 1]), np.sort(e[:, 1] * n + e[:, 0]))


@pytest.fixture(scope="module")
def noise():
    vox, block = MC.noise_block()
    return dict(vox=vox, block=block, mesh=_mesh_np(_vol(vox).extract_triangle_mesh()))


# ---- from_voxels
@pytest.mark.parametrize("case", ["noise", "holes5", "empty"])
def test_from_voxels_is_the_inverse_of_voxels(case):
    vox = MC.noise_block()[0] if case == "noise" else MC.holes(5)
    if case == "empty":
        vox = {k: v[:0] for k, v in vox.items()}
    vol = _vol(vox)
    assert vol.num_units == len(vox["keys"]) and vol.hash_capacity >= 2 * len(vox["keys"])
    assert _same_bits(vol.voxels(), _dev(vox))


def test_a_from_voxels_copy_of_an_integrated_volume_extracts_the_same_bits():
    vol = base._sphere_volume(6)
    copy = _vol(vol.voxels(), vol.voxel_length)
    assert copy.num_units == vol.num_units > 20
    a, b = vol.extract_triangle_mesh(), copy.extract_triangle_mesh()
    assert len(a.triangles) > 2000 and _same_bits(a, b)


# ---- extraction
def _case_volume(case):
    return MC.noise_block()[0] if case == "noise" else MC.holes(int(case))


@pytest.mark.parametrize("case", ["noise", "1", "3", "5", "7", "9"])
def test_extraction_of_noise_and_holes_equals_the_restatement(case, noise):
    """Triangles as integers, colours to the 1e-5 of tests/test_gpu_mesh.py, and every vertex component to MC.vertex_bound, which
    follows from the operations of mc_emit_kernel with u = 2^-24 (fp32 round to nearest), L = voxel_length as the fp32 the kernel
    holds (the restatement is given the same value), K the voxel's integer coordinate:
      p0 = fl((K + 0.5) L): K + 0.5 is exact (|K| < 2^23), one rounding                      |p0 - exact| <= u |p0| <= u (|p| + L)
      t  = fl(|f0| / fl(|f0| + |f1|)): two roundings of a value in [0, 1]                     |t - exact|  <= 2 u
      p  = fl(p0 + fl(t L)), or fl(fma(t, L, p0)) if the compiler contracts: at most          u L + u |p|
    in all 2 u |p| + 4 u L (the components off the edge's axis have the first term alone).  The fp64 restatement's own error is
    2^-29 of that.  No vertex is excluded."""
    vox = _case_volume(case)
    gv, gt, gc = noise["mesh"] if case == "noise" else _mesh_np(_vol(vox).extract_triangle_mesh())
    v, t, c = ref.extract(vox, VL32)
    assert len(t) > 1000 and gt.shape == t.shape and gv.shape == v.shape
    assert np.array_equal(gt, t)
    assert np.abs(gc - c).max() <= 1e-5
    ratio = np.abs(gv.astype(np.float64) - v) / MC.vertex_bound(v, VL32)
    print(f"{case}: {len(v)} vertices, {len(t)} triangles, max vertex error / bound {ratio.max():.3f}")
    assert ratio.max() <= 1.0


TABLE_MEMBRANES = ("the triangle table fans polygons from their lowest edge: where the cubes on both sides of an ambiguous face each "
                   "put a triangle through three crossings of that face, the two triangles coincide with opposite orientation (64 such "
                   "pairs among the 87 996 triangles of noise_block, 128 edges with four triangles, in the restatement alike).  The "
                   "surface has no boundary, but it is no 2-manifold there, and clean_mesh takes one of each pair for a repeated "
                   "face.  scripts/gen_mc_table.py would have to choose its fans differently")


@pytest.mark.xfail(strict=True, reason=TABLE_MEMBRANES)
def test_noise_block_mesh_is_closed_and_oriented(noise):
    assert ref.closed_and_oriented(noise["mesh"][1])


def test_noise_block_mesh_by_the_volume_alone(noise):
    """without the restatement: no boundary, every vertex used, one vertex per sign-changing voxel edge and on that edge, and the
    vertices of the edges at an exact zero (or a subnormal) on the voxel itself, bit for bit"""
    gv, gt, _ = noise["mesh"]
    T = noise["block"]["T"].astype(np.float64)
    assert _no_boundary(gt)
    assert np.array_equal(np.unique(gt), np.arange(len(gv)))
    inside = T < 0
    crossings = sum(int((np.take(inside, range(0, 31), ax) != np.take(inside, range(1, 32), ax)).sum()) for ax in range(3))
    assert len(gv) == crossings
    g = gv.astype(np.float64) / VL32 - 0.5 + 16                               # in voxels of the block
    near = np.abs(g - np.round(g)) < 1e-4
    assert (near.sum(1) >= 2).all()
    on_voxel = near.all(1)                                                    # t = 0 or 1: only next to a marked voxel
    q = np.round(g[on_voxel]).astype(np.int64)
    assert (np.abs(T[q[:, 2], q[:, 1], q[:, 0]]) < 1e-30).all()
    assert on_voxel.sum() >= 3 * len(MC.MARKS)
    e = g[~on_voxel]
    d = np.argmin(near[~on_voxel], 1)
    b0 = np.round(e).astype(np.int64)
    b0[np.arange(len(e)), d] = np.floor(e[np.arange(len(e)), d]).astype(np.int64)
    b1 = b0.copy()
    b1[np.arange(len(e)), d] += 1
    f0, f1 = T[b0[:, 2], b0[:, 1], b0[:, 0]], T[b1[:, 2], b1[:, 1], b1[:, 0]]
    assert ((f0 < 0) != (f1 < 0)).all()
    assert np.abs(e[np.arange(len(e)), d] - b0[np.arange(len(e)), d] - np.abs(f0) / (np.abs(f0) + np.abs(f1))).max() < 1e-4
    for (x, y, z), _ in MC.MARKS:                                             # the three edges toward +x, +y, +z start on the voxel
        p = (np.array([x, y, z], np.float32) - np.float32(16) + np.float32(0.5)) * np.float32(VL)
        assert (gv.view(np.int32) == p.view(np.int32)).all(1).sum() >= 3, (x, y, z)


def test_a_strip_of_4100_units_is_one_sheet_across_the_scan_block():
    vox, t = MC.strip_of_units()
    n = MC.STRIP_UNITS
    m = _vol(vox).extract_triangle_mesh()
    v, f = m.vertices, m.triangles.long()
    V, F = 16 * 16 * n, 2 * 15 * (16 * n - 1)
    assert tuple(v.shape) == (V, 3) and tuple(f.shape) == (F, 3)
    assert int(f.min()) == 0 and int(f.max()) == V - 1
    z = (7.5 + t) * VL32
    ratio = float((v[:, 2].double() - z).abs().max()) / float(MC.vertex_bound(np.float64(z), VL32))
    print(f"strip: plane height error / bound {ratio:.3f}")
    assert ratio <= 1.0
    p = v.double()
    nz = torch.linalg.cross(p[f[:, 1]] - p[f[:, 0]], p[f[:, 2]] - p[f[:, 0]])[:, 2]
    assert bool((nz > 0).all()) or bool((nz < 0).all())
    e = torch.cat([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
    und = torch.minimum(e[:, 0], e[:, 1]) * V + torch.maximum(e[:, 0], e[:, 1])
    _, count = torch.unique(und, return_counts=True)
    assert int(count.min()) == 1 and int(count.max()) == 2
    assert V - count.numel() + F == 1
    # the first four units on their own: the same vertices, and the same triangles up to the cubes that reach the fifth unit
    head = _vol({k: a[:4] for k, a in vox.items()}).extract_triangle_mesh()
    assert tuple(head.vertices.shape) == (16 * 16 * 4, 3) and tuple(head.triangles.shape) == (2 * 15 * 63, 3)
    assert _same_bits(head.vertices, m.vertices[:16 * 16 * 4]) and _same_bits(head.vertex_colors, m.vertex_colors[:16 * 16 * 4])
    assert torch.equal(head.triangles[:2 * 15 * 16 * 3], m.triangles[:2 * 15 * 16 * 3])


def test_empty_volumes_and_empty_meshes():
    from splat_slam_amd.mesh import TriangleMesh, TSDFVolume, clean_mesh
    empty = {k: v[:0] for k, v in MC.holes(1).items()}
    for vol in (TSDFVolume(VL, TRUNC, device=DEV, hash_capacity=64, pool_capacity=1), _vol(empty)):
        m = vol.extract_triangle_mesh()
        assert tuple(m.vertices.shape) == (0, 3) and tuple(m.triangles.shape) == (0, 3) and tuple(m.vertex_colors.shape) == (0, 3)
        assert m.vertices.dtype == torch.float32 and m.triangles.dtype == torch.int32 and m.vertex_colors.dtype == torch.float32
        assert vol.voxels()["keys"].shape == (0, 3)
    pts = torch.rand(5, 3, device=DEV)
    for mesh, min_len, kept in ((m, 100, 0), (TriangleMesh(pts, m.triangles, pts.clone()), 100, 0),
                                (TriangleMesh(pts, m.triangles, pts.clone()), 1, 5)):
        out, vmap = clean_mesh(mesh, min_len=min_len, return_vertex_map=True)
        shapes = [tuple(x.shape) for x in (out.vertices, out.triangles, out.vertex_colors)]
        assert shapes == [(kept, 3), (0, 3), (kept, 3)]
        assert out.vertices.dtype == torch.float32 and out.triangles.dtype == torch.int32 and vmap.dtype == torch.int32
        assert vmap.tolist() == ([-1] * len(mesh) if kept == 0 else list(range(kept)))
        if kept:
            assert _same_bits(out.vertices, pts)


def test_neither_the_pool_order_nor_the_table_size_reaches_the_mesh(noise):
    vox = noise["vox"]
    perm = np.random.default_rng(0).permutation(len(vox["keys"]))
    a = _vol(vox).extract_triangle_mesh()
    b = _vol({k: v[perm] for k, v in vox.items()}, hash_capacity=4096, pool_capacity=37).extract_triangle_mesh()
    assert np.array_equal(a.triangles.cpu().numpy(), noise["mesh"][1])
    assert _same_bits(a, b)


# ---- integration
def _new_volume(hash_capacity=256, pool_capacity=8):
    from splat_slam_amd.mesh import TSDFVolume
    return TSDFVolume(voxel_length=VL, sdf_trunc=TRUNC, device=DEV, hash_capacity=hash_capacity, pool_capacity=pool_capacity)


def _host_frames33():
    """33 of the sphere views at 64x48 with a ground-truth hole: 16 of a sphere, 16 of a second one two units further along x and
    one of a third, so that the second and the third chunk of 16 add units next to those that exist (32, 56 and 66 units)"""
    a = np.array([0.013, -0.021, 0.007])
    views = lambda n, shift: base._sphere_frames(n, 64, 48, 80.0, centre=tuple(a + shift))
    host = views(16, (0, 0, 0)) + views(16, (0.64, 0, 0)) + views(33, (1.5, 0.3, 0.2))[32:]
    for fr in host:
        fr["gt_depth"] = np.ones((48, 64), np.float32)
        fr["gt_depth"][20:30, 24:40] = 0.0
    return host


@pytest.fixture(scope="module")
def frames33():
    return base._dev_frames(_host_frames33())                                # exposure on all but the first


@pytest.fixture(scope="module")
def fused33(frames33):
    vol = _new_volume()
    vol.integrate_frames(frames33)
    return vol.voxels()


def test_33_frames_in_one_call_against_the_restatement(frames33, fused33):
    vol = _new_volume()
    vol.integrate_frames(frames33)
    assert _same_bits(vol.voxels(), fused33)
    rv = ref.RefVolume(VL, TRUNC)
    for fr in frames33:
        rv.integrate(base._host(fr))
    n, bad, bad_clear = base._compare_volumes(vol, rv)
    print(f"33 frames: {bad} of {n} updated voxels differ from the fp64 restatement ({bad_clear} away from a knife edge)")
    assert n > 10000
    assert bad <= 1e-3 * n, (bad, n)
    assert bad_clear == 0, bad_clear


@pytest.mark.parametrize("split", ["one by one", "15 + 1 + 17"])
def test_33_frames_give_the_same_bits_however_the_calls_are_split(frames33, fused33, split):
    vol = _new_volume()
    if split == "one by one":
        for fr in frames33:
            vol.integrate(**fr)
    else:
        for part in (frames33[:15], frames33[15:16], frames33[16:]):
            vol.integrate_frames(part)
    assert _same_bits(vol.voxels(), fused33)


def test_growing_the_hash_and_the_pool_between_chunks_changes_no_bit(frames33, fused33):
    small, large = _new_volume(64, 1), _new_volume(1 << 14, 2048)
    seen = []
    for part in (frames33[:16], frames33[16:32], frames33[32:]):              # the chunks of one call
        small.integrate_frames(part)
        seen.append((small.num_units, small.hash_capacity, small.pool_capacity))
    large.integrate_frames(frames33)
    print("units, hash and pool capacity after each chunk:", seen)
    assert seen[0][0] < seen[1][0] < seen[2][0]                                # every chunk adds units to those that exist,
    assert 64 <= seen[0][1] < seen[1][1] < seen[2][1]                          # the second and the third rehash them
    assert 1 < seen[0][2] < seen[1][2]                                         # and the second moves them to a larger pool
    assert (large.hash_capacity, large.pool_capacity) == (1 << 14, 2048) and large.num_units == small.num_units
    assert _same_bits(small.voxels(), fused33) and _same_bits(large.voxels(), fused33)


def test_a_from_voxels_copy_of_a_half_built_volume_continues_bit_for_bit(frames33, fused33):
    vol = _new_volume()
    vol.integrate_frames(frames33[:16])
    copy = _vol(vol.voxels())
    assert copy.num_units == vol.num_units
    copy.integrate_frames(frames33[16:])
    assert _same_bits(copy.voxels(), fused33)


def test_the_colour_byte_is_rounded_at_every_step():
    """one frame: every voxel of weight 1 that is clear of a pixel border holds (int)(fl(clamp(fl(fl(ea r) + eb), 0, 1) 255)) of its
    pixel, for one of the three fp32 neighbours of exp(a), the same for all.  tests/test_mesh_cpu.py shows that a fused multiply-add
    changes several hundred of these bytes for each of the three."""
    fr = MC.color_frame()
    dev = dict(fr, **{k: torch.from_numpy(fr[k]).to(DEV) for k in ("render", "depth", "exposure_a", "exposure_b")})
    dev["w2c"] = torch.from_numpy(fr["w2c"])
    vol = _new_volume()
    vol.integrate(**dev)
    vox = {k: v.cpu().numpy() for k, v in vol.voxels().items()}
    ui, vi, clear = MC.voxel_pixels(fr, vox["keys"], VL, TRUNC)
    use = clear & (vox["weight"] == 1)
    assert use.sum() > 5000 and not (vox["weight"] > 1).any()
    got = vox["color"][use]
    wrong = [int((MC.color_bytes(fr, e)[:, vi[use], ui[use]].T != got).sum()) for e in MC.exposure_candidates(fr)]
    fused = [int((MC.color_bytes(fr, e, fused=True)[:, vi[use], ui[use]].T != got).sum()) for e in MC.exposure_candidates(fr)]
    print(f"{int(use.sum())} voxels: bytes off per candidate of exp(a), rounded separately {wrong}, fused {fused}")
    assert sorted(wrong)[0] == 0 and sorted(wrong)[1] > 0


# ---- cleaning
def _clean(verts, faces, cols, min_len=100):
    from splat_slam_amd.mesh import TriangleMesh, clean_mesh
    mesh = TriangleMesh(torch.as_tensor(verts).to(DEV), torch.as_tensor(faces).int().to(DEV), torch.as_tensor(cols).to(DEV))
    return clean_mesh(mesh, min_len=min_len, return_vertex_map=True)


def _assert_clean_equals(out, vmap, want):
    wv, wt, wc, wmap = want
    assert np.array_equal(vmap.cpu().numpy(), wmap)
    assert np.array_equal(out.triangles.cpu().numpy(), wt)
    assert np.array_equal(out.vertices.cpu().numpy().view(np.int32), wv.astype(np.float32).view(np.int32))
    assert np.array_equal(out.vertex_colors.cpu().numpy().view(np.int32), wc.astype(np.float32).view(np.int32))


def test_cleaning_small_equals_the_restatement_in_any_face_order_and_on_a_side_stream():
    verts, faces, cols = MC.cleaning_small()
    want = ref.clean(verts.astype(np.float64), faces, cols)
    out, vmap = _clean(verts, faces, cols)
    assert 0 < len(want[1]) < len(faces) and 0 < len(want[0]) < len(verts)
    _assert_clean_equals(out, vmap, want)
    # the faces shuffled: the labels do not depend on the races, and of two copies the one with the lower index stays
    perm = np.random.default_rng(1).permutation(len(faces))
    want_p = ref.clean(verts.astype(np.float64), faces[perm], cols)
    out_p, vmap_p = _clean(verts, faces[perm], cols)
    _assert_clean_equals(out_p, vmap_p, want_p)
    assert _same_bits(out_p.vertices, out.vertices) and torch.equal(vmap_p, vmap)
    sets = lambda t: np.unique(np.sort(t.cpu().numpy(), 1), axis=0)
    assert np.array_equal(sets(out_p.triangles), sets(out.triangles))
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        out_s, vmap_s = _clean(verts, faces, cols)
    side.synchronize()
    assert _same_bits(out_s, out) and torch.equal(vmap_s, vmap)


@pytest.fixture(scope="module")
def cleaned_noise():
    """the marching-cubes mesh of noise_block through clean_mesh(min_len=1), and which of its faces have exactly no area"""
    from splat_slam_amd.mesh import clean_mesh
    mesh = _vol(MC.noise_block()[0]).extract_triangle_mesh()
    out, vmap = clean_mesh(mesh, min_len=1, return_vertex_map=True)
    v, t, _ = _mesh_np(mesh)
    v64 = v.astype(np.float64)
    e1, e2 = v64[t[:, 1]] - v64[t[:, 0]], v64[t[:, 2]] - v64[t[:, 0]]
    sin = np.linalg.norm(np.cross(e1, e2), axis=1) / np.maximum(np.linalg.norm(e1, axis=1) * np.linalg.norm(e2, axis=1), 1e-300)
    flat = np.nonzero(sin < 1e-6)[0]                                          # all others have an area by fp64's margin
    area = np.ones(len(t), bool)
    area[[i for i in flat if not any(MC.exact_cross(v, t[i]))]] = False
    _, ident = np.unique(v, axis=0, return_inverse=True)
    return dict(mesh=mesh, out=out, vmap=vmap, v=v, t=t, area=area, ident=ident.reshape(-1))


def test_cleaning_the_noise_block_mesh_drops_every_face_of_no_area_and_no_other_but_a_copy(cleaned_noise):
    """The vertices of the edges that start at an exact zero coincide, so faces between them have no area.  A face stays if and
    only if its exact area is not zero and no earlier face with an area has its three vertices.  About half of the faces without
    area have two equal edge vectors that are not zero: a fused cross product keeps those."""
    c = cleaned_noise
    v, t, area = c["v"], c["t"], c["area"]
    zero = np.nonzero(~area)[0]
    telling = sum(not MC.fused_cross_is_zero(v, t[i]) for i in zero)
    print(f"noise block: {len(zero)} of {len(t)} faces have no area; a fused cross product would keep {telling} of them")
    assert len(zero) >= 20 and telling >= 3
    assert c["ident"].max() + 1 <= len(v) - 2 * len(MC.MARKS)                 # the zeros did put vertices on one point
    assert _same_bits(c["out"].vertices, c["mesh"].vertices)
    assert torch.equal(c["vmap"].cpu(), torch.arange(len(v), dtype=torch.int32))
    _, first = np.unique(np.sort(t[area], 1), axis=0, return_index=True)
    keep = np.nonzero(area)[0][np.sort(first)]
    print(f"{int(area.sum()) - len(keep)} faces with an area repeat the vertices of an earlier one")
    assert np.array_equal(c["out"].triangles.cpu().numpy(), t[keep])
    assert _no_boundary(c["ident"][t[area]])                                  # taking the faces of no area away opens nothing


@pytest.mark.xfail(strict=True, reason=TABLE_MEMBRANES)
def test_cleaning_the_noise_block_mesh_loses_no_face_with_an_area_and_stays_closed(cleaned_noise):
    c = cleaned_noise
    kept = c["out"].triangles.cpu().numpy().astype(np.int64)
    assert len(kept) == int(c["area"].sum())
    assert _no_boundary(c["ident"][kept])


def test_cleaning_large_equals_its_closed_form_and_itself():
    m = MC.cleaning_large()
    V, F = m["vertices"].shape[0], m["faces"].shape[0]
    assert V > 2 ** 20 + 4096 and F > 2 ** 21
    dev = {k: v.to(DEV) for k, v in m.items()}
    out, vmap = _clean(dev["vertices"], dev["faces"], dev["colors"])
    assert torch.equal(vmap, dev["vertex_map"])
    assert _same_bits(out.vertices, dev["vertices"][dev["keep_vertex"]])
    assert _same_bits(out.vertex_colors, dev["colors"][dev["keep_vertex"]])
    assert torch.equal(out.triangles, dev["vertex_map"][dev["faces"][dev["keep_face"]].long()])
    again, vmap2 = _clean(dev["vertices"], dev["faces"], dev["colors"])
    assert _same_bits(again, out) and torch.equal(vmap2, vmap)
