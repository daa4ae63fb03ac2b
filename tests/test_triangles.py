"""Triangles and triangle meshes (rtw_quad.shape = RTW_QUAD_TRIANGLE; Triangle, Mesh, load_obj, worlds.icosphere) on
the host backend (RTW_DEVICE_CPU, the GPU's per-sample code compiled for the host): quad_t against float64 and against
the parallelogram it shares its plane with, boxes, a quad split into two triangles, an instance tree against the list
on a closed mesh whose every edge is shared, the triangle light's analytic form factor, the OBJ loader and the
refusals.  Every seed is fixed: every figure below is deterministic."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import instance_tree_scenes as T
import lights_scenes as S
import mesh_scenes as M

CPU = M.CPU


# ---------------------------------------------------------------- 1. quad_t
N_PAIRS = 1_000_000


@functools.lru_cache(maxsize=None)
def pairs():
    p = M.random_pairs(N_PAIRS, 0)
    for a in p.values():
        a.setflags(write=False)
    return p


def test_quad_t_against_float64(rtw):
    """10^6 random (triangle, ray, interval) pairs through rtw_debug_quad_hit -- Quad.init's derivation and the
    kernels' quad_t on the host -- against t, alpha, beta in float64.  Wherever float64 keeps min(alpha, beta,
    1 - alpha - beta) 1e-4 away from zero, t - tmin and tmax - t (as distances along the ray) 1e-4 L away from zero
    (L: the triangle's longest edge) and |n.d| >= 1e-6 |n| |d|, the hit flag agrees and t is within
    1e-5 max(1, |t|).  The excluded pairs are at most 2 % (numpy alone decides that: mesh_scenes.random_pairs).
    Measured: 1.26 % excluded, 12.3 % of the rest hit, no flag differs, worst |t - t64| / max(1, |t|) = 2.1e-6,
    worst |alpha - alpha64| = 2.7e-5 (the distribution's analysis predicts ~2e-5)."""
    p = pairs()
    t, alpha, beta, cos = M.reference_f64(p)
    for k in ("q", "o"):
        assert np.abs(p[k]).max() <= 1000.0
    assert max(np.abs(p["q"] + p["u"]).max(), np.abs(p["q"] + p["v"]).max()) <= 1000.0 * (1 + 1e-6)
    assert max(np.abs(p[k]).max() for k in "qo") >= 900.0          # coordinates up to 1e3 do occur
    assert p["sliver"].mean() > 0.15 and (cos < 0.05).mean() > 0.05 and cos.min() < 0.025
    dlen = np.linalg.norm(p["d"].astype(np.float64), axis=1)
    tmin, tmax, L = p["tmin"].astype(np.float64), p["tmax"].astype(np.float64), p["L"]
    edge = np.minimum(np.minimum(alpha, beta), 1.0 - alpha - beta)
    near_t = (np.abs(t - tmin) * dlen < 1e-4 * L) | (np.abs(tmax - t) * dlen < 1e-4 * L)
    excluded = (np.abs(edge) < 1e-4) | near_t | (cos < 1e-6)
    print(f"excluded {excluded.mean():.4%} (edge {(np.abs(edge) < 1e-4).mean():.4%}, interval {near_t.mean():.4%})")
    assert excluded.mean() <= 0.02
    assert near_t.mean() > 0.005                                   # intervals that end near the hit do occur
    # the library's |denom| < 1e-8 reject is out of play: n.d is the unit normal's product with d
    assert (cos * dlen)[~excluded].min() > 1e-7
    expect = (edge > 0) & (t >= tmin) & (t <= tmax)
    rec = M.quad_records(rtw, p["q"], p["u"], p["v"], rtw._abi.RTW_QUAD_TRIANGLE)
    hit, tt, ab = M.quad_hit(rtw, rec, p["o"], p["d"], p["tmin"], p["tmax"])
    inc = ~excluded
    print(f"hits among the included: {expect[inc].mean():.3%}; flags that differ: {(hit != expect)[inc].sum()}")
    assert 0.05 < expect[inc].mean() < 0.5
    assert np.array_equal(hit[inc], expect[inc])
    both = inc & hit
    err = np.abs(tt[both].astype(np.float64) - t[both]) / np.maximum(1.0, np.abs(t[both]))
    print(f"worst |t - t64| / max(1, |t|) = {err.max():.3e}; worst |alpha - alpha64| = "
          f"{np.abs(ab[both, 0] - alpha[both]).max():.3e}, |beta - beta64| = {np.abs(ab[both, 1] - beta[both]).max():.3e}")
    assert (err <= 1e-5).all()


def test_triangle_is_the_parallelogram_cut_at_the_diagonal(rtw):
    """Same (q, u, v) and rays: the triangle accepts exactly the rays the parallelogram accepts with
    fl(alpha + beta) <= 1, with the same t and (alpha, beta) bits -- the parallelogram path is the library's
    behaviour before there were triangles."""
    p = pairs()
    A = rtw._abi
    args = (p["o"], p["d"], p["tmin"], p["tmax"])
    hq, tq, abq = M.quad_hit(rtw, M.quad_records(rtw, p["q"], p["u"], p["v"], A.RTW_QUAD_PARALLELOGRAM), *args)
    ht, tt, abt = M.quad_hit(rtw, M.quad_records(rtw, p["q"], p["u"], p["v"], A.RTW_QUAD_TRIANGLE), *args)
    with np.errstate(invalid="ignore"):
        s = abq[:, 0] + abq[:, 1]                        # float32 + float32, as the library adds them
    assert s.dtype == np.float32
    assert np.array_equal(ht, hq & (s <= np.float32(1.0)))
    assert 0.3 < ht.sum() / hq.sum() < 0.7
    assert np.array_equal(tt[ht].view(np.uint32), tq[ht].view(np.uint32))
    assert np.array_equal(abt[ht].view(np.uint32), abq[ht].view(np.uint32))
    # the diagonal itself is inside: alpha + beta == 1 exactly (dyadic coordinates: every product is exact)
    one = M.quad_records(rtw, [[0, 0, 0]] * 3, [[4, 0, 0]] * 3, [[0, 4, 0]] * 3, A.RTW_QUAD_TRIANGLE)
    o = np.array([[2, 2, 1], [3, 1, 1], [2.5, 2, 1]], np.float32)
    d = np.array([[0, 0, -1]] * 3, np.float32)
    h, _, ab = M.quad_hit(rtw, one, o, d, np.full(3, 0.001, np.float32), np.full(3, np.inf, np.float32))
    assert h.tolist() == [True, True, False] and ab[:2].sum(1).tolist() == [1.0, 1.0]


# ---------------------------------------------------------------- 2. boxes
def _vertices(arr, i):
    q, u, v = (arr.quads[i][k].astype(np.float32) for k in "quv")
    return np.stack([q, q + u, q + v])


def _pad(lo, hi):
    """Aabb.pad (aabb.zig:36-43) in float32."""
    lo, hi = lo.astype(np.float32).copy(), hi.astype(np.float32).copy()
    delta = np.float32(0.0001)
    thin = ~(hi - lo >= delta)
    lo[thin] -= delta / np.float32(2)
    hi[thin] += delta / np.float32(2)
    return lo, hi


def _ancestor_boxes(nodes):
    """For every leaf of a pre-order / skip-link node array: the indices of the inner nodes above it."""
    w = nodes["a"][:, 3].view(np.uint32)
    leaf = (w & 0x80000000) != 0
    skip = (w & 0x7FFFFFFF).astype(np.int64)
    out, stack = {}, []
    for i in range(len(nodes)):
        while stack and skip[stack[-1]] <= i:
            stack.pop()
        if leaf[i]:
            out[i] = list(stack)
        else:
            stack.append(i)
    return out


@pytest.mark.parametrize("mode", ["sah", "reference"])
def test_vertices_inside_every_ancestor_box(rtw, mode):
    """cornell_mesh(): triangles at the top level, in a list instance (12) and in a tree instance (320).  Every
    vertex lies in every box above its leaf -- the world tree's in world space (through the instance's transforms),
    the instance tree's in object space."""
    A = rtw._abi
    arr = rtw.flatten(M.mixed_objects(rtw), bvh_mode=T.mode_of(rtw, mode))
    shape = A.quad_shape(arr.quads)
    assert (shape == A.RTW_QUAD_TRIANGLE).sum() == 2 + 320 + 12 + 1 and (shape == 0).sum() == 5
    world = rtw.World(arr, device=CPU)
    nodes = world.nodes()
    inst_nodes = [world.instance_nodes(i) for i in range(len(arr.instances))]
    world.close()
    assert [len(n) for n in inst_nodes] == [2 * 320 - 1, 0]
    bw = nodes["b"][:, 3].view(np.uint32)
    idx = nodes["b"][:, 2].view(np.uint32)
    seen = 0
    for leaf, above in _ancestor_boxes(nodes).items():
        kind = (bw[leaf] >> 8) & 0xFF
        if kind == A.RTW_OBJ_QUAD and shape[idx[leaf]] == A.RTW_QUAD_TRIANGLE:
            pts = _vertices(arr, idx[leaf]).astype(np.float64)
        elif kind == A.RTW_OBJ_INSTANCE:
            inst = arr.instances[idx[leaf]]
            members = arr.members[inst["first"]:inst["first"] + inst["count"]]
            pts = np.concatenate([_vertices(arr, m["index"]) for m in members]).astype(np.float64)
            for x in inst["xf"][:inst["n_xf"]]:               # innermost first
                if x["kind"] == A.RTW_XF_TRANSLATE:
                    pts = pts + x["v"].astype(np.float64)
                else:
                    r = np.radians(np.float64(x["v"][0]))
                    px, pz = pts[:, 0].copy(), pts[:, 2].copy()
                    pts[:, 0] = np.cos(r) * px + np.sin(r) * pz
                    pts[:, 2] = -np.sin(r) * px + np.cos(r) * pz
        else:
            continue
        seen += len(pts)
        for i in above:
            lo, hi = nodes["a"][i, :3].astype(np.float64), nodes["b"][i, :3].astype(np.float64)
            # (the rotation above is float64 where the library's is float32: 1e-3 of slack on coordinates of ~500)
            assert (pts >= lo - 1e-3).all() and (pts <= hi + 1e-3).all(), (leaf, i)
    assert seen == 3 * (2 + 1 + 320 + 12)
    # the tree instance's own tree, in object space: exact
    tn = inst_nodes[0]
    tb = tn["b"][:, 2].view(np.uint32)
    above = _ancestor_boxes(tn)
    assert len(above) == 320
    for leaf, anc in above.items():
        pts = _vertices(arr, tb[leaf])
        for i in anc:
            assert (pts >= tn["a"][i, :3]).all() and (pts <= tn["b"][i, :3]).all(), (leaf, i)


@pytest.mark.parametrize("mode", ["sah", "reference"])
def test_single_triangle_root_box(rtw, mode):
    """One triangle's box is the padded (Aabb.pad) box of its three vertices.  A world of one object is one leaf,
    which carries no box, so the triangle shares the world with a far sphere that extends the root on one side
    only: the root's other side is the triangle's.  SAH trees push every inner box out by the scene's box_pad
    (rtw_scene_stats), the reference tree by nothing."""
    a, b, c = [1.0, 2.0, 3.0], [4.0, 2.0, 3.5], [2.0, 2.0, 7.0]       # flat in y: padded there
    mat = rtw.Lambertian.fromColor([0.5] * 3)
    tri = rtw.Triangle.init(a, b, c, mat)
    v = np.array([a, b, c], np.float32)
    lo, hi = _pad(v.min(0), v.max(0))
    # the four-corner box would reach (5, 2, 7.5): the triangle's does not
    assert hi[0] == 4.0 and hi[2] == 7.0 and lo[1] == np.float32(2.0) - np.float32(0.00005)
    for centre, side, mine in (([100, 100, 100], "a", lo), ([-100, -100, -100], "b", hi)):
        arr = rtw.flatten([tri, rtw.Sphere.init(centre, 1, mat)], bvh_mode=T.mode_of(rtw, mode))
        world = rtw.World(arr, device=CPU)
        nodes, pad = world.nodes(), np.float32(world.stats()["box_pad"])
        world.close()
        assert len(nodes) == 3 and not (nodes["a"][0, 3].view(np.uint32) & 0x80000000)
        assert (pad > 0) == (mode == "sah")
        assert np.array_equal(nodes[side][0, :3], mine - pad if side == "a" else mine + pad), (mode, side)


# ---------------------------------------------------------------- 3. split quad
QW, QDEPTH, QSPP = 32, 10, 256
QSEEDS = tuple(range(60, 68))


@functools.lru_cache(maxsize=None)
def quads_images(split):
    rtw = M.pkg()
    arr = rtw.flatten(M.quads_objects(rtw, split))
    cam = M.sky_camera(rtw, QW, QSPP, QDEPTH)
    world = rtw.World(arr, device=CPU)
    out = np.stack([M.render(rtw, arr, cam, QSPP, s, world=world)[:, :3] / QSPP for s in QSEEDS]).astype(np.float64)
    world.close()
    out.setflags(write=False)
    return out


def test_split_quads_render_the_quads(rtw):
    """quads_world under its sky, each quad as the triangles (q, u, v) and (q + u + v, -u, -v): every 4 x 4 block
    and channel, and the image mean, within 5 sqrt(seA^2 + seB^2) of the quads' render over 8 seeds x 256 spp
    (the quad description is the reference).  Measured: no difference at all -- these quads are axis-aligned, so
    both triangles' planes give the quad's t to the bit, and a solid Lambertian does not read the hit's (u, v)."""
    a, b = quads_images(True), quads_images(False)
    # (two whole parallelograms per quad would pass the comparison below as well: each triangle is a half)
    cam = M.sky_camera(rtw, QW, 4, QDEPTH)
    halves = rtw.flatten(M.quads_objects(rtw, True)[::2])
    assert not np.array_equal(M.render(rtw, halves, cam, 4, QSEEDS[0]),
                              M.render(rtw, rtw.flatten(M.quads_objects(rtw, False)), cam, 4, QSEEDS[0]))
    n = np.sqrt(len(QSEEDS))

    def blocks(img):
        s = img.shape[0]
        return img.reshape(s, QW // 4, 4, QW // 4, 4, 3).mean(axis=(2, 4)).reshape(s, -1, 3)

    for what, x, y in (("blocks", blocks(a), blocks(b)), ("image", a.mean(1), b.mean(1))):
        se = np.sqrt((x.std(0, ddof=1) / n) ** 2 + (y.std(0, ddof=1) / n) ** 2)
        diff = np.abs(x.mean(0) - y.mean(0))
        print(f"split quads {what}: worst |difference| - 5 se = {(diff - 5 * se).max():.3e}, worst |difference| = "
              f"{diff.max():.3e}")
        assert (diff <= 5 * se).all(), (what, (diff - 5 * se).max())       # (se = 0 where the sky saturates a channel)


# ---------------------------------------------------------------- 4. tree equals list
@pytest.mark.parametrize("medium", [False, True], ids=["solid", "medium_boundary"])
@pytest.mark.parametrize("mode", ["sah", "reference"])
def test_tree_equals_list(rtw, mode, medium):
    """The 80-triangle icosphere under RotateY + Translate, as a private tree and as a list: 48 x 48 x 8 spp, depth
    50, bit-identical (every edge is shared by two triangles: exact ties go to the later member either way)."""
    cam = rtw.Camera(image_width=48, samples_per_pixel=8, max_depth=50, **T.CAM_KW).init()
    imgs = []
    for bvh in (True, False):
        arr = rtw.flatten(M.ico_objects(rtw, bvh, medium), bvh_mode=T.mode_of(rtw, mode))
        assert arr.instances["flags"][0] == rtw._abi.RTW_INST_LIST | (rtw._abi.RTW_INST_BVH if bvh else 0)
        imgs.append(M.render(rtw, arr, cam, 8, 11))
    assert np.isfinite(imgs[0]).all()
    assert np.array_equal(imgs[0], imgs[1])
    # the mesh is in the picture: without it the render differs
    arr = rtw.flatten(M.ico_objects(rtw, None, medium)[:2], bvh_mode=T.mode_of(rtw, mode))
    assert not np.array_equal(M.render(rtw, arr, cam, 8, 11), imgs[0])


# ---------------------------------------------------------------- 5. triangle light
def expected_tri_floor(cam):
    xz = S.floor_hits(cam)
    sel = np.nonzero(np.hypot(xz[:, 0], xz[:, 1]) <= 3.0)[0]      # lights_scenes.expected_floor's selection
    return sel, S.ALBEDO / np.pi * M.TRI_LIGHT[3] * M.triangle_form_factor(xz[sel], M.TRI_LIGHT)


def test_triangle_quadrature_helper():
    """The two triangles of the 1 x 1 light sum to lights_scenes.form_factor of the quad."""
    pts = np.array([[0.0, 0.0], [1.5, -0.7], [-2.0, 2.0]])
    q, u, v, le = (np.array(a, np.float64) for a in S.LIGHT1)
    other = (q + u + v, -u, -v, le)
    both = M.triangle_form_factor(pts, M.TRI_LIGHT) + M.triangle_form_factor(pts, other)
    assert np.allclose(both, S.form_factor(pts, S.LIGHT1), rtol=1e-9)


def test_triangle_light_analytic(rtw):
    """The analytic scene of tests/lights_scenes.py with its 1 x 1 light replaced by the right triangle (q, q + u,
    q + v) of the same plane: seed-mean of 16 x 256 spp against albedo / pi * Le * integral cos cos' / r^2 dA over
    the triangle, within 5 se + 0.5 %, with the light registered (a wrong area, fold or interior test in light_pdf
    shows here) and without.  Measured: worst |mean - expected| / bound = 0.813 registered, 0.815 not."""
    cam = S.analytic_camera(rtw, S.SPP)
    sel, expected = expected_tri_floor(cam)
    assert len(sel) > 1000
    for lights in (True, False):
        img = M.tri_light_seed_images(lights)[:, sel]
        mean, se = img.mean(0), img.std(0, ddof=1) / np.sqrt(len(S.SEEDS))
        z = np.abs(mean - expected) / (5 * se + 0.005 * expected)
        print(f"triangle light, registered={lights}: worst |mean - expected| / bound = {z.max():.3f}")
        assert (z <= 1).all(), (lights, int(sel[z.argmax()]), z.max())


def test_triangle_light_variance_reduction(rtw):
    """Summed across-seed variance with the triangle registered / without: <= 0.25, the bound of
    test_lights.test_variance_reduction.  Measured: 0.0222."""
    cam = S.analytic_camera(rtw, S.SPP)
    sel, _ = expected_tri_floor(cam)
    on = M.tri_light_seed_images(True)[:, sel].var(0, ddof=1).sum()
    off = M.tri_light_seed_images(False)[:, sel].var(0, ddof=1).sum()
    print(f"triangle light variance ratio on / off = {on / off:.4f}")
    assert on / off <= 0.25


def test_triangle_light_round_trip_and_hash(rtw):
    A = rtw._abi
    objs = M.tri_light_objects(rtw)
    arr_on, arr_off = rtw.flatten(objs, lights="emissive"), rtw.flatten(objs)
    assert arr_on.lights.tolist() == [(A.RTW_OBJ_QUAD, 1)] and A.quad_shape(arr_on.quads).tolist() == [0, 1]
    w_on, w_off = rtw.World(arr_on, device=CPU), rtw.World(arr_off, device=CPU)
    assert w_on.lights().tolist() == [(A.RTW_OBJ_QUAD, 1)] and len(w_off.lights()) == 0

    def scene_hash(world):
        h = C.c_uint64()
        A.check(rtw.lib().rtw_scene_hash(world.handle, C.byref(h)), "rtw_scene_hash")
        return h.value

    h_on, h_off = scene_hash(w_on), scene_hash(w_off)
    assert h_on != h_off
    w_on.set_lights(None)
    assert scene_hash(w_on) == h_off
    # the shape is part of the scene image: the same (q, u, v) as a parallelogram hashes differently
    arr_quad = rtw.flatten(objs)
    A.quad_shape(arr_quad.quads)[1] = A.RTW_QUAD_PARALLELOGRAM
    w_quad = rtw.World(arr_quad, device=CPU)
    assert scene_hash(w_quad) != h_off
    for w in (w_on, w_off, w_quad):
        w.close()


# ---------------------------------------------------------------- 6. loader
def _same_mesh(a, b):
    return (np.array_equal(a.vertices, b.vertices) and np.array_equal(a.faces, b.faces) and
            len(a.objects) == len(b.objects) and
            all(np.array_equal(getattr(x, k), getattr(y, k)) for x, y in zip(a.objects, b.objects) for k in "quv"))


def test_obj_fixtures_load_the_same_mesh(rtw):
    mat = rtw.Lambertian.fromColor([0.5] * 3)
    ref = rtw.worlds.icosphere(1, [0, 0, 0], 1, mat)
    assert len(ref.objects) == 80 and len(ref.vertices) == 42
    for name in ("v", "vt", "vtn", "vn"):
        path = os.path.join(M.MESHES, f"ico1_{name}.obj")
        assert os.path.getsize(path) < 8192
        mesh = rtw.load_obj(path, mat)
        assert isinstance(mesh, rtw.Mesh) and isinstance(mesh, rtw.HittableList)
        assert _same_mesh(mesh, ref), name
        assert all(t.shape == rtw._abi.RTW_QUAD_TRIANGLE and t.mat is mat for t in mesh.objects)
    assert _same_mesh(rtw.load_obj(open(os.path.join(M.MESHES, "ico1_v.obj")).read(), mat), ref)   # text


def test_icosphere_is_closed_and_outward(rtw):
    for level, n in ((0, 20), (1, 80), (2, 320)):
        m = rtw.worlds.icosphere(level, [1, 2, 3], 5, rtw.Lambertian.fromColor([0.5] * 3))
        assert len(m.objects) == n == 20 * 4 ** level
        edges = {}
        for f in m.faces:
            for i, j in ((f[0], f[1]), (f[1], f[2]), (f[2], f[0])):
                edges[(i, j)] = edges.get((i, j), 0) + 1
        assert all(c == 1 and (j, i) in edges for (i, j), c in edges.items())    # every edge once each way
        assert np.allclose(np.linalg.norm(m.vertices - np.float32([1, 2, 3]), axis=1), 5, rtol=1e-6)
        for t in m.objects:
            assert np.dot(np.cross(t.u, t.v), t.q + (t.u + t.v) / 3 - np.float32([1, 2, 3])) > 0


def test_obj_fans_negative_indices_and_errors(rtw):
    mat = rtw.Lambertian.fromColor([0.5] * 3)
    text = """# a pentagon as one face, then a triangle by negative indices
mtllib ignored.mtl
v 0 0 0
v 2 0 0
v 3 2 0
v 1 3 0
v -1 2 0
vn 0 0 1
usemtl ignored
f 1/1/1 2/1/1 3/1/1 4/1/1 5/1/1
v 0 0 1
f -1 -6 -5
"""
    m = rtw.load_obj(text, mat)
    assert m.faces.tolist() == [[0, 1, 2], [0, 2, 3], [0, 3, 4], [5, 0, 1]]
    assert len(m.vertices) == 6 and len(m.objects) == 4
    assert np.array_equal(m.objects[3].q, np.float32([0, 0, 1])) and np.array_equal(m.objects[3].u, np.float32([0, 0, -1]))
    for bad in ("v 0 0 0\nv 1 0 0\nv 0 1 0\nf 1 2 4\n", "v 0 0 0\nv 1 0 0\nv 0 1 0\nf 0 1 2\n",
                "v 0 0 0\nv 1 0 0\nv 0 1 0\nf -4 1 2\n", "v 0 0 0\nv 1 0 0\nf 1 2 3\nv 0 1 0\n"):
        with pytest.raises(ValueError):
            rtw.load_obj(bad, mat)
    with pytest.raises(ValueError):
        rtw.Mesh.init([[0, 0, 0], [1, 0, 0], [0, 1, 0]], [[0, 1, 3]], mat)


def test_mesh_is_a_list(rtw):
    """Mesh: bvh = None keeps the list's rule (a tree above 127 members); bare, it is an instance without
    transforms."""
    A = rtw._abi
    mat = rtw.Lambertian.fromColor([0.5] * 3)
    ground = rtw.Sphere.init([0, -1000, 0], 990, mat)
    for level, tree in ((1, False), (2, True)):
        arr = rtw.flatten([ground, rtw.worlds.icosphere(level, [0, 0, 0], 5, mat)])
        assert arr.instances["n_xf"][0] == 0 and arr.instances["count"][0] == 20 * 4 ** level
        assert bool(arr.instances["flags"][0] & A.RTW_INST_BVH) == tree
        w = rtw.World(arr, device=CPU)
        assert (len(w.instance_nodes(0)) > 0) == tree
        w.close()
    assert rtw.flatten([ground, rtw.worlds.icosphere(1, [0, 0, 0], 5, mat, bvh=True)]).instances["flags"][0] & A.RTW_INST_BVH


# ---------------------------------------------------------------- 7. refusals
def test_unknown_shape_is_refused_by_name(rtw):
    A = rtw._abi
    arr = rtw.flatten(rtw.worlds.cornell_box())
    A.quad_shape(arr.quads)[7] = 2
    d = arr.desc()
    h = C.c_void_p()
    for create in (lambda: rtw.lib().rtw_scene_create(C.byref(d), CPU, C.byref(h)),
                   lambda: rtw.lib().rtw_scene_create_ex(C.byref(d), CPU, None, C.byref(h))):
        assert create() == A.RTW_E_INVALID
        msg = rtw.lib().rtw_last_error()
        assert b"quad 7" in msg and b"shape 2" in msg, msg
    n, depth = C.c_uint32(), C.c_uint32()
    assert rtw.lib().rtw_scene_flatten(C.byref(d), None, 0, C.byref(n), C.byref(depth)) == A.RTW_E_INVALID
    rec = M.quad_records(rtw, [[0, 0, 0]], [[1, 0, 0]], [[0, 1, 0]], 2)
    z = np.zeros(3, np.float32)
    one = np.ones(1, np.float32)
    out = np.zeros(4, np.float32)
    rc = rtw.lib().rtw_debug_quad_hit(1, rec.ctypes.data, z.ctypes.data, z.ctypes.data, one.ctypes.data, one.ctypes.data,
                                      out.ctypes.data, out.ctypes.data, out.ctypes.data)
    assert rc == A.RTW_E_INVALID and b"quad 0" in rtw.lib().rtw_last_error()


def test_emissive_triangle_in_an_instance_is_refused(rtw):
    """As test_lights.test_validation_and_get refuses an instance member quad: lights inside a mesh stay out of
    scope."""
    A = rtw._abi
    glow = rtw.DiffuseLight.fromColor([4, 4, 4])
    mesh = rtw.worlds.icosphere(0, [0, 3, 0], 1, glow)
    objs = S.analytic_objects(rtw) + [rtw.Translate.init(mesh, [0, 1, 0])]
    arr = rtw.flatten(objs, lights="emissive")
    assert arr.lights.tolist() == [(A.RTW_OBJ_QUAD, 1)]           # "emissive": top-level records only
    world = rtw.World(arr, device=CPU)
    member = tuple(int(x) for x in arr.members[0])
    assert member[0] == A.RTW_OBJ_QUAD and A.quad_shape(arr.quads)[member[1]] == A.RTW_QUAD_TRIANGLE
    recs = np.array([member], A.OBJECT_DT)
    assert rtw.lib().rtw_scene_set_lights(world.handle, A.ptr(recs), 1) == A.RTW_E_INVALID
    assert b"is an instance member" in rtw.lib().rtw_last_error()
    assert world.lights().tolist() == [(A.RTW_OBJ_QUAD, 1)]
    world.close()
    with pytest.raises(rtw.RtwError):
        rtw.World(rtw.flatten(objs, lights=[mesh.objects[0]]), device=CPU)
