"""The TSDF mesh without a GPU: the generated marching-cubes table (csrc/sgr_mc_table.h) is what scripts/gen_mc_table.py writes
and cannot crack, the fp64 restatement (tests/mesh_ref.py) fuses an analytic sphere into one closed genus-0 surface,
csrc/sgr_mesh.hip (with the shared csrc/sgr_scan.hip) compiles for gfx950 without scratch, spills or float atomics, splat_slam_amd.mesh refuses what it does not
implement, and the cases of tests/mesh_cases.py meet, on the restatement alone, the conditions that make them worth running on
the kernels (tests/test_gpu_mesh_edges.py)."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

import mesh_cases as MC
import mesh_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
# the file and what it launches through sgr_scan.h (the scans, the compaction)
SOURCES = ("sgr_mesh", "sgr_scan")
KERNELS = ("tsdf_touch_kernel", "tsdf_list_kernel", "tsdf_rehash_kernel", "tsdf_integrate_kernel", "scan_local_kernel",
           "chunked_scan_kernel", "scan_add_kernel", "gather_units_kernel", "bitonic_step_kernel", "mc_count_kernel", "mc_emit_kernel",
           "cc_init_kernel", "cc_union_kernel", "cc_flatten_kernel", "cc_keep_vertices_kernel", "tri_keep_kernel",
           "tri_bucket_kernel", "tri_dedup_kernel", "compact_vertices_kernel", "compact_triangles_kernel")


# ---- the table
def test_regenerating_the_table_reproduces_the_header():
    gen = ref.load_generator()
    assert open(gen.OUT).read() == gen.render()


def _sign_edges(case):
    return {e for e, (a, b) in enumerate(ref.EDGES) if ((case >> a) & 1) != ((case >> b) & 1)}


def test_every_triangle_vertex_is_on_a_sign_change_and_every_sign_change_is_used():
    for case in range(256):
        used = {e for tri in ref.TABLE[case] for e in tri}
        assert used == _sign_edges(case), case
        for tri in ref.TABLE[case]:
            assert len(set(tri)) == 3, (case, tri)


def _face_of_edge_pair(a, b):
    """the cube face holding both edges, as (axis, side), or None"""
    ca = {c for c in ref.EDGES[a]}
    cb = {c for c in ref.EDGES[b]}
    corners = ca | cb
    for axis in range(3):
        for side in (0, 1):
            if all(ref.CORNERS[c][axis] == side for c in corners):
                return axis, side
    return None


def _boundary(case):
    """directed edges used once by the case's triangles (an undirected pair used twice is interior)"""
    cnt = {}
    for a, b, c in ref.TABLE[case]:
        for e in ((a, b), (b, c), (c, a)):
            cnt[e] = cnt.get(e, 0) + 1
    return [e for e in cnt if (e[1], e[0]) not in cnt]


def _face_signs(case, axis, side):
    return tuple(sorted((ref.CORNERS[c], (case >> c) & 1) for c in range(8) if ref.CORNERS[c][axis] == side))


def _edge_corners(e):
    return tuple(sorted(ref.CORNERS[c] for c in ref.EDGES[e]))


def test_triangle_boundaries_lie_on_faces_and_match_across_shared_faces():
    # per case, boundary segments grouped by face, as geometric edges (pairs of corner positions)
    seg = {}
    for case in range(256):
        faces = {}
        for a, b in _boundary(case):
            f = _face_of_edge_pair(a, b)
            assert f is not None, (case, a, b)            # a boundary edge runs across one cube face
            faces.setdefault(f, []).append((_edge_corners(a), _edge_corners(b)))
        seg[case] = faces
    # the segments on a face depend only on that face's four corner signs
    by_signs = {}
    for case in range(256):
        for axis in range(3):
            for side in (0, 1):
                key = (axis, side, _face_signs(case, axis, side))
                got = sorted(seg[case].get((axis, side), []))
                assert by_signs.setdefault(key, got) == got, (case, axis, side)
    # the neighbour across face (axis, 1) sees it as its face (axis, 0), shifted by one along axis: same segments, reversed
    for case in range(256):
        for axis in range(3):
            mine = seg[case].get((axis, 1), [])
            face_signs = {c: (case >> c) & 1 for c in range(8) if ref.CORNERS[c][axis] == 1}
            for other in range(256):
                o_signs = {c: (other >> c) & 1 for c in range(8) if ref.CORNERS[c][axis] == 0}
                match = all(face_signs[c] == o_signs[d] for c in face_signs for d in o_signs
                            if all(ref.CORNERS[c][k] == ref.CORNERS[d][k] for k in range(3) if k != axis))
                if not match:
                    continue
                shift = lambda p: tuple(p[k] + (1 if k == axis else 0) for k in range(3))
                theirs = sorted((tuple(sorted(map(shift, b))), tuple(sorted(map(shift, a)))) for a, b in seg[other].get((axis, 0), []))
                assert sorted(mine) == theirs, (case, other, axis)
                break


# ---- the restatement on an analytic sphere
def test_restated_fusion_of_a_sphere_is_one_closed_genus_zero_surface():
    # sdf_trunc of three voxels: at two, cubes seen only at grazing angles keep an unobserved corner (sdf along the ray < -trunc)
    # and leave the surface open there, as the fusion would
    r, vl = 0.3, 0.02
    frames = ref.sphere_views(14, r, 160, 120, 200.0, 1.0, centre=(0.013, -0.021, 0.007))
    vol = ref.RefVolume(vl, 0.06)
    for fr in frames:
        vol.integrate(fr)
    v, t, c = ref.extract(vol.arrays(), vl)
    v, t, c, _ = ref.clean(v, t, c, 100)
    assert len(v) > 1000 and len(t) > 2000
    lab = ref.components(len(v), t)
    assert len(np.unique(lab)) == 1
    assert ref.closed_and_oriented(t)
    assert ref.euler(len(v), t) == 2
    dist = np.abs(np.linalg.norm(v - np.array([0.013, -0.021, 0.007]), axis=1) - r)
    assert dist.max() <= 0.5 * vl, dist.max()
    # triangles face from T < 0 (inside) toward T > 0: normals point away from the centre
    n = np.cross(v[t[:, 1]] - v[t[:, 0]], v[t[:, 2]] - v[t[:, 0]])
    out = v[t].mean(1) - np.array([0.013, -0.021, 0.007])
    assert ((n * out).sum(1) > 0).mean() > 0.99


def test_restated_cleaning_drops_small_components():
    verts = np.random.default_rng(0).normal(size=(9, 3))
    tris = np.array([[0, 1, 2], [1, 2, 3], [4, 5, 6], [1, 2, 3], [0, 0, 1]])
    v, t, c, vmap = ref.clean(verts, tris, verts, min_len=4)
    assert (vmap[:4] == np.arange(4)).all() and (vmap[4:] == -1).all()
    assert t.tolist() == [[0, 1, 2], [1, 2, 3]]


# ---- ISA budget
@pytest.fixture(scope="module")
def mesh_isa(tmp_path_factory):
    if not (os.path.exists(HIPCC) or shutil.which(HIPCC)):
        pytest.skip("hipcc not available")
    text, meta = "", {}
    for src in SOURCES:
        out = str(tmp_path_factory.mktemp("isa") / (src + ".s"))
        subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-S", "--cuda-device-only", "-o", out,
                        os.path.join(ROOT, "splat_slam_amd", "csrc", src + ".hip")], check=True, capture_output=True)
        one = open(out).read()
        text += one
        for block in one.split("\n  - ")[1:]:
            m = re.search(r"\.name:\s+(\S+)", block)
            if m and ".private_segment_fixed_size" in block:
                assert m.group(1) not in meta, m.group(1)
                meta[m.group(1)] = block
    return text, meta


def test_every_mesh_kernel_has_no_scratch_no_spills_and_no_float_atomics(mesh_isa):
    text, meta = mesh_isa
    for k in KERNELS:
        names = [n for n in meta if re.search(r"\d%s" % k, n)]
        assert len(names) == 1, (k, sorted(meta))
        block = meta[names[0]]
        scratch = int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", block).group(1))
        spill = int(re.search(r"\.vgpr_spill_count:\s+(\d+)", block).group(1))
        assert scratch == 0 and spill == 0, (k, scratch, spill)
    assert len(meta) == len(KERNELS), sorted(meta)
    # float atomics of any width or packing (v_pk_add_f32 is a plain VALU add, not an atomic)
    assert not re.search(r"(global|flat|buffer|ds)_atomic_\w*(f32|f64|pk_add)", text)
    assert not re.search(r"(global|flat|buffer)_atomic_pk_add", text)


# ---- argument checks
def test_mesh_api_refuses_cpu_tensors_wrong_shapes_and_min_len():
    from splat_slam_amd.mesh import TriangleMesh, TSDFVolume, clean_mesh
    v = torch.zeros(4, 3)
    t = torch.tensor([[0, 1, 2], [1, 2, 3]], dtype=torch.int32)
    with pytest.raises(RuntimeError, match="GPU"):
        clean_mesh(TriangleMesh(v, t, v.clone()))
    with pytest.raises(ValueError, match="min_len"):
        clean_mesh(TriangleMesh(v, t, v.clone()), min_len=0)
    with pytest.raises(RuntimeError, match="GPU"):
        TSDFVolume(device="cpu")
    with pytest.raises(RuntimeError, match="GPU"):
        clean_mesh(TriangleMesh(v[:, :2], t, v.clone()))
    from splat_slam_amd.eval import eval_rendering
    with pytest.raises(RuntimeError, match="GPU tensors"):
        import types
        eval_rendering([types.SimpleNamespace(original_image=torch.zeros(3, 4, 4))], None, None, None, mesh=True)


def test_ply_round_trip_on_the_host(tmp_path):
    from splat_slam_amd.mesh import TriangleMesh
    g = torch.Generator().manual_seed(0)
    v = torch.rand(10, 3, generator=g)
    c = torch.rand(10, 3, generator=g)
    t = torch.randint(0, 10, (7, 3), generator=g, dtype=torch.int32)
    m = TriangleMesh(v, t, c)
    m.write_ply(str(tmp_path / "m.ply"))
    r = TriangleMesh.read_ply(str(tmp_path / "m.ply"))
    assert torch.equal(r.vertices, v) and torch.equal(r.triangles, t)
    assert (r.vertex_colors - c).abs().max() <= 0.5 / 255 + 1e-7


# ---- the cases of tests/mesh_cases.py are what tests/test_gpu_mesh_edges.py needs them to be
def test_noise_block_reaches_every_case_in_cubes_across_1_2_4_and_8_units():
    vox, block = MC.noise_block()
    t = MC.cube_tables(vox)
    assert int(t["valid"].sum()) == 31 ** 3 and not t["hole"].any()
    for span in (1, 2, 4, 8):
        assert (t["valid"] & (t["span"] == span)).any(), span
    assert (t["valid"] & (t["span"] == 8)).sum() == 1
    count = np.bincount(t["case"][t["valid"]], minlength=256)
    print("cubes per case: min %d, median %d" % (count.min(), np.median(count)))
    assert count.min() >= 20
    # the 3 x 30 x 30 cubes across one unit border reach nearly every case on their own, the 3 x 30 across two a good many
    assert len(np.unique(t["case"][t["valid"] & (t["span"] == 2)])) >= 250
    assert len(np.unique(t["case"][t["valid"] & (t["span"] == 4)])) >= 50
    T = block["T"]
    assert (np.abs(T) >= 2.0 ** -10).sum() == T.size - len(MC.MARKS)
    assert (T[[0, -1]] == 1).all() and (T[:, [0, -1]] == 1).all() and (T[:, :, [0, -1]] == 1).all()
    kinds = set()
    for (x, y, z), val in MC.MARKS:
        got = T[z, y, x]
        assert got == np.float32(val) and np.signbit(got) == np.signbit(np.float32(val)) and abs(got) < 1.2e-38
        kinds.add((float(got) == 0.0, bool(np.signbit(got))))
        inside = got < 0
        assert all((T[z + dz, y + dy, x + dx] < 0) != inside for dx, dy, dz in ((1, 0, 0), (0, 1, 0), (0, 0, 1)))
    assert kinds == {(True, False), (True, True), (False, False), (False, True)}
    # the restatement closes it, and the zeros put several vertices on one point
    v, tri, _ = ref.extract(vox, 2.0 ** -6)
    assert len(np.unique(tri)) == len(v)
    (de, dc), (ue, uc) = ref.edge_use(tri)
    back = {(a, b): c for (a, b), c in zip(map(tuple, de.tolist()), dc.tolist())}
    assert all(back.get((b, a)) == c for (a, b), c in back.items())                  # no boundary: every directed edge has its reverse
    # ... but not closed_and_oriented: where the cubes on both sides of an ambiguous face each put a triangle through three crossings
    # of that face, the two coincide with opposite orientation, and their edges carry four triangles (test_gpu_mesh_edges has the
    # strict xfail)
    sets, count = np.unique(np.sort(tri, 1), axis=0, return_counts=True)
    assert (count == 2).sum() == 64 and count.max() == 2
    print("edges by number of triangles:", np.bincount(uc).tolist())
    assert set(uc.tolist()) == {2, 4} and (uc == 4).sum() < 1e-3 * len(uc)
    assert len(np.unique(v, axis=0)) <= len(v) - 2 * len(MC.MARKS)


@pytest.mark.parametrize("n_units", sorted(MC.HOLE_KEYS))
def test_holes_skip_cubes_for_every_reason_and_have_active_edges_without_a_cube(n_units):
    vox = MC.holes(n_units)
    assert len(vox["keys"]) == n_units and (n_units == 1 or n_units & (n_units - 1))      # one unit, or no power of two
    t = MC.cube_tables(vox)
    frac = 1 - vox["weight"].mean()
    assert 0.04 < frac < 0.06
    assert t["valid"].sum() > 1000 and not (t["valid"] & (t["hole"] | t["face"] | t["diagonal"])).any()
    assert (~t["valid"] == (t["hole"] | t["face"] | t["diagonal"])).all()
    only = lambda name: t[name] & ~np.logical_or.reduce([t[o] for o in ("hole", "face", "diagonal") if o != name])
    assert only("hole").sum() > 100 and only("face").sum() > 100
    # a cube can lack a diagonal unit alone only where the units across its faces exist: in the block with one unit taken out
    assert t["diagonal"].any() and (only("diagonal").sum() >= 1) == (n_units >= 7)
    dead = MC.dead_active_edges(vox)
    print(f"holes({n_units}): {int(t['valid'].sum())} valid cubes, {dead} active edges without a valid cube")
    assert dead >= 10
    v, tri, _ = ref.extract(vox, 0.02)
    assert len(v) > 1000 and len(np.unique(tri)) == len(v)             # every vertex of the restatement is used by a face


def test_holes_have_a_far_unit_and_units_that_meet_only_diagonally():
    for n, keys in MC.HOLE_KEYS.items():
        assert len(set(keys)) == n
        assert (MC.FAR in keys) == (n != 7)
    touch = lambda a, b: sorted(abs(a[k] - b[k]) for k in range(3))
    for n in (3, 5):
        ks = [k for k in MC.HOLE_KEYS[n] if k != MC.FAR]
        kinds = [touch(a, b) for i, a in enumerate(ks) for b in ks[i + 1:] if max(touch(a, b)) <= 1]
        assert kinds and all(sum(k) >= 2 for k in kinds), kinds            # neighbours, none across a face
    assert touch((1, 1, 1), (0, 0, 0)) == [1, 1, 1]


def test_strip_of_units_is_one_sheet_across_the_scan_block():
    vox, t = MC.strip_of_units(6, -3)
    assert MC.STRIP_UNITS > 4096 and MC.STRIP_FIRST < 0 < MC.STRIP_FIRST + MC.STRIP_UNITS
    assert abs(t - 0.3) < 1e-6
    v, tri, _ = ref.extract(vox, 0.02)
    assert len(v) == 16 * 16 * 6 and len(tri) == 2 * 15 * (16 * 6 - 1)
    assert np.abs(v[:, 2] - (7.5 + t) * 0.02).max() < 1e-12
    assert ref.euler(len(v), tri) == 1


def test_cleaning_small_meets_every_drop_reason_with_no_face_near_the_decision():
    verts, faces, cols = MC.cleaning_small()
    v64 = verts.astype(np.float64)
    reason, keepv = MC.drop_reasons(verts, faces)
    for r in (MC.KEPT, MC.SMALL, MC.REPEATED, MC.ZERO_AREA, MC.DUPLICATE):
        assert (reason == r).sum() >= 4, r
    wv, wt, wc, vmap = ref.clean(v64, faces, cols)
    assert np.array_equal(vmap >= 0, keepv) and np.array_equal(wt, vmap[faces[reason == MC.KEPT]])
    # components: 99 goes, 100 and 101 stay, single vertices go, and the small ones come first
    size = np.bincount(ref.components(len(verts), faces))
    size = size[size > 0]
    assert {1, 99, 100, 101} <= set(size.tolist()) and size[0] == 1 and list(size[3:6]) == [99, 100, 101]
    assert (size == 100).sum() == 2                                      # one of them through a face with a repeated index alone
    # kept faces are far from degenerate: the kernel's fp32 rule and the exact one cannot differ on them
    e1, e2 = v64[faces[:, 1]] - v64[faces[:, 0]], v64[faces[:, 2]] - v64[faces[:, 0]]
    sin = np.linalg.norm(np.cross(e1, e2), axis=1) / np.maximum(np.linalg.norm(e1, axis=1) * np.linalg.norm(e2, axis=1), 1e-300)
    live = (reason == MC.KEPT) | (reason == MC.DUPLICATE)
    print("smallest |cross| / (|e1| |e2|) of a non-degenerate face: %.4f" % sin[live].min())
    assert sin[live].min() >= 1e-3
    # the zero-area faces: exactly zero, of both kinds, and a fused cross product would keep some of each
    zero = np.nonzero(reason == MC.ZERO_AREA)[0]
    equal = [i for i in zero if any((verts[faces[i, a]] == verts[faces[i, b]]).all() for a, b in ((0, 1), (1, 2), (0, 2)))]
    line = [i for i in zero if i not in equal]
    assert len(equal) >= 6 and len(line) >= 6
    for group in (equal, line):
        assert all(len(set(faces[i].tolist())) == 3 for i in group)
        assert sum(not MC.fused_cross_is_zero(verts, faces[i]) for i in group) >= 2
    # copies: of kept faces in all six orders on either side of the original, and of dropped faces
    kept_sets = {tuple(sorted(f)): i for i, f in enumerate(faces.tolist()) if reason[i] == MC.KEPT}
    perms = {"before": set(), "after": set()}
    for i in np.nonzero(reason == MC.DUPLICATE)[0]:
        f, k = faces[i].tolist(), kept_sets[tuple(sorted(faces[i].tolist()))]
        assert k < i
        perms["before" if k < MC.SMALL_FRONT else "after"].add(tuple(faces[k].tolist().index(x) for x in f))
    assert len(perms["before"]) == 6 and len(perms["after"]) == 6, perms
    dropped = {tuple(f) for i, f in enumerate(faces.tolist()) if reason[i] in (MC.REPEATED, MC.ZERO_AREA)}
    assert sum(faces.tolist().count(list(f)) >= 2 for f in dropped) >= 4


def test_cleaning_large_in_closed_form_is_what_the_restatement_gives():
    m = MC.cleaning_large(strips=30)
    v, f, c = m["vertices"].numpy().astype(np.float64), m["faces"].numpy().astype(np.int64), m["colors"].numpy()
    assert len(v) == 100 * 30 and len(f) == 197 * 30
    wv, wt, wc, vmap = ref.clean(v, f, c)
    assert np.array_equal(vmap, m["vertex_map"].numpy())
    assert np.array_equal(wt, m["vertex_map"].numpy()[f[m["keep_face"].numpy()]])
    assert np.array_equal(wv, v[m["keep_vertex"].numpy()])
    reason, _ = MC.drop_reasons(m["vertices"].numpy(), f)
    assert (reason == MC.DUPLICATE).sum() == 20 and (reason == MC.ZERO_AREA).sum() == 10 and (reason == MC.REPEATED).sum() == 10
    zero = np.nonzero(reason == MC.ZERO_AREA)[0]
    assert sum(not MC.fused_cross_is_zero(m["vertices"].numpy(), f[i]) for i in zero) >= 5
    e1, e2 = v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]]
    sin = np.linalg.norm(np.cross(e1, e2), axis=1) / np.maximum(np.linalg.norm(e1, axis=1) * np.linalg.norm(e2, axis=1), 1e-300)
    assert sin[m["keep_face"].numpy()].min() >= 1e-3
    assert 100 * MC.LARGE_STRIPS > 2 ** 20 + 4096 and 197 * MC.LARGE_STRIPS > 2 ** 21 and MC.LARGE_STRIPS % 6 == 3


def test_color_frame_tells_separate_rounding_from_a_fused_multiply_add():
    fr = MC.color_frame()
    vl, trunc = 0.02, 0.06
    keys, _ = ref.touched_units(fr, vl, trunc)
    ui, vi, clear = MC.voxel_pixels(fr, np.array(sorted(keys)), vl, trunc)
    used = np.zeros(fr["depth"].shape, bool)
    used[vi[clear], ui[clear]] = True
    assert clear.sum() > 5000 and used.sum() > 500
    cands = MC.exposure_candidates(fr)
    assert len({float(e) for e in cands}) == 3
    images = [MC.color_bytes(fr, e) for e in cands]
    for e, img in zip(cands, images):
        differ = (MC.color_bytes(fr, e, fused=True) != img)[:, used].sum()
        print("exp(a) = %.9g: a fused multiply-add changes %d of %d bytes" % (e, differ, 3 * used.sum()))
        assert differ >= 5
        assert 0 < (img[:, used] == 0).sum() and 0 < (img[:, used] == 255).sum()       # both clamps are met
    for a in range(3):                                                   # and the three candidates can be told apart
        for b in range(a + 1, 3):
            assert (images[a] != images[b])[:, used].sum() >= 5


def test_from_voxels_refuses_bad_units_before_any_launch():
    from splat_slam_amd.mesh import TSDFVolume
    good = MC.holes(3)
    bad = lambda **kw: dict(good, **kw)
    twice = good["keys"].copy()
    twice[2] = twice[0]
    far = good["keys"].copy()
    far[1, 2] = 1 << 20
    low = good["keys"].copy()
    low[1, 0] = -(1 << 20) - 1
    for vox, what in ((bad(keys=twice), "duplicate"), (bad(keys=far), "outside"), (bad(keys=low), "outside"),
                      (bad(keys=good["keys"].astype(np.int32)), "int64"), (bad(keys=good["keys"][:, :2]), "int64"),
                      (bad(tsdf=good["tsdf"][:2]), "4096"), (bad(weight=good["weight"][:, :100]), "4096"),
                      (bad(color=good["color"][..., :2]), "4096")):
        with pytest.raises(ValueError, match=what):
            TSDFVolume.from_voxels(vox, 0.02, 0.06)
    with pytest.raises(RuntimeError, match="GPU"):
        TSDFVolume.from_voxels(good, 0.02, 0.06, device="cpu")
