"""Per-vertex normals and uvs on triangles (rtw_scene_set_vertex_attrs), without a GPU: the host-only hook
rtw_debug_quad_shade -- quad_prep and quad_attr, the code every kernel runs -- against float64 and against exact
identities, the radial identity of a smooth icosphere, images on the host backend against the analytic Sphere,
registration, and the Python layer (Triangle / Mesh / load_obj / icosphere / flatten)."""
import ctypes as C
import dataclasses
import os

import numpy as np
import pytest

import mesh_scenes as M
import smooth_scenes as S

CPU = S.CPU


@pytest.fixture(scope="module")
def hits(rtw):
    """mesh_scenes.random_pairs(200_000): the pairs that hit, with the library's own t and (alpha, beta)."""
    p = M.random_pairs(200_000)
    rec = M.quad_records(rtw, p["q"], p["u"], p["v"], rtw._abi.RTW_QUAD_TRIANGLE)
    hit, t, ab = M.quad_hit(rtw, rec, p["o"], p["d"], p["tmin"], p["tmax"])
    assert hit.sum() > 10_000
    sel = {k: v[hit] for k, v in p.items()}
    return dict(p=sel, rec=rec[hit], t=t[hit], ab=ab[hit])


def test_hook_against_float64(rtw, hits):
    """Random unit vertex normals within 60 degrees of the face normal, uvs in [0, 1]^2: |m| >= 0.5, three products
    and two sums per component -> a few 2^-24 / |m|.  Bounds: 4e-6 per normal component, 1e-6 per uv."""
    p, rec, t, ab = hits["p"], hits["rec"], hits["t"], hits["ab"]
    n = len(rec)
    rng = np.random.default_rng(5)
    g64 = np.cross(p["u"].astype(np.float64), p["v"].astype(np.float64))
    g64 /= np.linalg.norm(g64, axis=1, keepdims=True)
    normals = S.normals_near(g64, 60.0, rng).astype(np.float32)
    uvs = rng.random((n, 3, 2)).astype(np.float32)
    got_n, got_uv, front = S.quad_shade(rtw, rec, S.attr_records(rtw, n, normals, uvs), p["o"], p["d"], t)
    ns, uv, lm = S.shade_reference_f64(p, ab[:, 0], ab[:, 1], normals, uvs)
    assert lm.min() >= 0.5 - 1e-6
    # front: the sign test on the fp32 geometric normal, exactly
    g32 = S.geometric_normal_f32(p["u"], p["v"])
    want_front = S.dot_f32(p["d"], g32) < 0
    assert np.array_equal(front, want_front)
    want_n = np.where(want_front[:, None], ns, -ns)
    en = np.abs(got_n.astype(np.float64) - want_n).max()
    eu = np.abs(got_uv.astype(np.float64) - uv).max()
    print(f"hook vs float64 over {n} hits: worst normal component {en:.3g}, worst uv {eu:.3g}")
    assert en <= 4e-6
    assert eu <= 1e-6


def test_exact_identities(rtw, hits):
    p, rec, t, ab = hits["p"], hits["rec"], hits["t"], hits["ab"]
    n = len(rec)
    A = rtw._abi
    g32 = S.geometric_normal_f32(p["u"], p["v"])
    front = S.dot_f32(p["d"], g32) < 0
    plain_n = np.where(front[:, None], g32, -g32).astype(np.float32)
    bits = lambda a: np.ascontiguousarray(a, np.float32).view(np.uint32)                      # noqa: E731
    # flags = 0: quad_prep's record
    zero = np.zeros(n, A.VERTEX_ATTR_DT)
    zero["normal"], zero["uv"] = 7.0, 9.0          # ignored without their flags
    got_n, got_uv, got_f = S.quad_shade(rtw, rec, zero, p["o"], p["d"], t)
    assert np.array_equal(got_f, front)
    assert np.array_equal(bits(got_n), bits(plain_n))
    assert np.array_equal(bits(got_uv), bits(ab))
    # uvs (0,0), (1,0), (0,1): (alpha, beta) exactly; the normal untouched
    unit_uv = np.broadcast_to(np.array([[0, 0], [1, 0], [0, 1]], np.float32), (n, 3, 2))
    got_n, got_uv, _ = S.quad_shade(rtw, rec, S.attr_records(rtw, n, None, unit_uv), p["o"], p["d"], t)
    assert np.array_equal(bits(got_uv), bits(ab))
    assert np.array_equal(bits(got_n), bits(plain_n))
    # n0 = n1 = n2 = -n: flipped to n's side, +n on the front side; the uv untouched
    flipped = np.broadcast_to((-g32)[:, None, :], (n, 3, 3))
    got_n, got_uv, _ = S.quad_shade(rtw, rec, S.attr_records(rtw, n, flipped), p["o"], p["d"], t)
    assert np.abs(got_n[front] - g32[front]).max() <= 1e-6
    assert np.abs(got_n[~front] + g32[~front]).max() <= 1e-6
    assert np.array_equal(bits(got_uv), bits(ab))
    # m vanishes (n1 = -n0, alpha = w0 = 0.5, beta = 0): the geometric normal.  Axis-aligned records at
    # power-of-two scales, the ray along the normal through the middle of the edge q .. q + u: t, the hit point and
    # (alpha, beta) are exact, the hook normalises n0 and -n0 to exact negatives, and the sum is exactly 0.
    eye = np.eye(3, dtype=np.float32)
    qs, us, vs, gs = [], [], [], []
    for j in range(-3, 4):
        for ax in range(3):
            s = np.float32(2.0 ** j)
            eu, ev, en = eye[ax], eye[(ax + 1) % 3], eye[(ax + 2) % 3]
            qs.append(-s * eu), us.append(2 * s * eu), vs.append(2 * s * ev), gs.append(en)
    qs, us, vs, gs = (np.stack(x) for x in (qs, us, vs, gs))
    k = len(qs)
    rk = M.quad_records(rtw, qs, us, vs, A.RTW_QUAD_TRIANGLE)
    o, d = 2 * gs, -gs
    hit, tk, abk = M.quad_hit(rtw, rk, o, d, np.full(k, 1e-3, np.float32), np.full(k, np.inf, np.float32))
    assert hit.all() and (tk == 2).all() and (abk[:, 0] == 0.5).all() and (abk[:, 1] == 0).all()
    n0 = S.normals_near(gs.astype(np.float64), 40.0, np.random.default_rng(2), 1)[:, 0].astype(np.float32)
    nv = np.stack([n0, -n0, gs], axis=1)
    nn, _, ff = S.quad_shade(rtw, rk, S.attr_records(rtw, k, nv), o, d, tk)
    assert ff.all()
    assert np.array_equal(bits(nn), bits(gs))


def _ico_faces(rtw, level, c, R, **kw):
    mesh = rtw.worlds.icosphere(level, c, R, rtw.Lambertian.fromColor([0.5] * 3), **kw)
    return mesh


def test_radial_identity(rtw):
    """icosphere(2, c, R, smooth=True): the shading normal at a point p of a face is unit(p - c) -- vertex normals
    are the vertex directions and p is the same combination of the vertices.  1e-5 rad: fp32 vertex rounding at
    R = 5, |c| <= 10.  The flat normal on the same hits is off by more than 0.05 rad on average."""
    A = rtw._abi
    c, R = np.array([4.0, -7.0, 5.5]), 5.0
    mesh = _ico_faces(rtw, 2, c, R, smooth=True)
    tris = mesh.objects
    assert len(tris) == 320 and all(t.normals is not None and t.uvs is None for t in tris)
    rng = np.random.default_rng(9)
    n = 10_000
    f = rng.integers(0, len(tris), n)
    a, b = rng.random(n), rng.random(n)
    fold = a + b > 1
    a, b = np.where(fold, 1 - a, a), np.where(fold, 1 - b, b)
    a, b = 0.02 + 0.94 * a, 0.02 + 0.94 * b * (1 - 0.02)          # away from the edges: every ray hits
    q = np.stack([tris[i].q for i in f]).astype(np.float32)
    u = np.stack([tris[i].u for i in f]).astype(np.float32)
    v = np.stack([tris[i].v for i in f]).astype(np.float32)
    nrm = np.stack([tris[i].normals for i in f]).astype(np.float32)
    target = q.astype(np.float64) + a[:, None] * u + b[:, None] * v
    out = target - c
    out /= np.linalg.norm(out, axis=1, keepdims=True)
    noise = rng.normal(size=(n, 3))
    skew = out + 0.5 * noise / np.linalg.norm(noise, axis=1, keepdims=True)    # within 30 degrees of radial
    skew /= np.linalg.norm(skew, axis=1, keepdims=True)
    o = (target + 3.0 * skew).astype(np.float32)
    d = (target - o.astype(np.float64)).astype(np.float32)
    rec = M.quad_records(rtw, q, u, v, A.RTW_QUAD_TRIANGLE)
    hit, t, ab = M.quad_hit(rtw, rec, o, d, np.full(n, 1e-3, np.float32), np.full(n, np.inf, np.float32))
    assert hit.all()
    got, _, front = S.quad_shade(rtw, rec, S.attr_records(rtw, n, nrm), o, d, t)
    assert front.all()
    # the point the library's own (alpha, beta) names, in float64 over the fp32 vertices
    p64 = q.astype(np.float64) + ab[:, :1].astype(np.float64) * u + ab[:, 1:].astype(np.float64) * v
    want = p64 - c
    want /= np.linalg.norm(want, axis=1, keepdims=True)
    angle = lambda x, y: np.arctan2(np.linalg.norm(np.cross(x, y), axis=1), (x * y).sum(1))   # noqa: E731
    worst = angle(got.astype(np.float64), want).max()
    flat, _, _ = S.quad_shade(rtw, rec, np.zeros(n, A.VERTEX_ATTR_DT), o, d, t)
    flat_mean = angle(flat.astype(np.float64), want).mean()
    print(f"radial identity: worst angle {worst:.3g} rad; flat normal off by {flat_mean:.3g} rad on average")
    assert worst <= 1e-5
    assert flat_mean > 0.05


# ---------------------------------------------------------------- images on the host backend
IW, ISPP, ISEED, IR = 96, 4, 33, 3.0


def _centre_hits(cam, R, frac):
    """Pixels whose centre ray meets the sphere of radius R at the origin within frac * R of the camera's axis (z):
    (pixel indices, hit points on the sphere, ray origins, directions), float64."""
    cd = cam.derived
    W, H = cd.image_width, cd.image_height
    f3 = lambda x: np.array(list(x), np.float64)                                              # noqa: E731
    o = f3(cd.center)
    jj, ii = np.mgrid[0:H, 0:W]
    d = f3(cd.pixel00_loc) + ii[..., None] * f3(cd.pixel_delta_u) + jj[..., None] * f3(cd.pixel_delta_v) - o
    d = d.reshape(-1, 3)
    a, hb, cc = (d * d).sum(1), (d * o).sum(1), (o * o).sum() - R * R
    disc = hb * hb - a * cc
    ok = disc > 0
    t = (-hb - np.sqrt(np.where(ok, disc, 0))) / a
    p = o + t[:, None] * d
    ok &= np.hypot(p[:, 0], p[:, 1]) <= frac * R
    idx = np.flatnonzero(ok)
    return idx, p[idx], o, d[idx]


def _mesh_uv_f64(mesh, o, d):
    """Closest hit of each ray (o, d[i]) with the mesh in float64 and the interpolated per-corner uv there."""
    q = np.stack([t.q for t in mesh.objects]).astype(np.float64)
    u = np.stack([t.u for t in mesh.objects]).astype(np.float64)
    v = np.stack([t.v for t in mesh.objects]).astype(np.float64)
    uv = np.stack([t.uvs for t in mesh.objects]).astype(np.float64)
    nrm = np.cross(u, v)
    w = nrm / (nrm * nrm).sum(1, keepdims=True)
    out = np.full((len(d), 2), np.nan)
    for i, di in enumerate(d):
        den = nrm @ di
        with np.errstate(divide="ignore", invalid="ignore"):
            t = ((q - o) * nrm).sum(1) / den
        pl = o + t[:, None] * di - q
        al = (w * np.cross(pl, v)).sum(1)
        be = (w * np.cross(u, pl)).sum(1)
        ok = (t > 1e-3) & (al >= 0) & (be >= 0) & (al + be <= 1)
        k = np.flatnonzero(ok)
        k = k[np.argmin(t[k])]
        out[i] = (1 - al[k] - be[k]) * uv[k, 0] + al[k] * uv[k, 1] + be[k] * uv[k, 2]
    return out


def _texel(uv, w, h):
    nu, nv = np.clip(uv[:, 0], 0, 1), 1.0 - np.clip(uv[:, 1], 0, 1)
    return np.minimum((nu * w).astype(int), w - 1), np.minimum((nv * h).astype(int), h - 1)


def test_mirror_sphere_images(rtw):
    """A level-3 icosphere of radius 3 as a mirror under the gradient sky, flat, smooth and as the analytic Sphere,
    96 x 96 x 4 spp, depth 2, one seed (the same camera rays).  The flat normal is off by 0.041 rad on average at
    level 3, the smooth one only by the chord's depth error (about 0.006 rad at 0.8 R): a ratio near 0.15, required
    <= 0.25 over the pixels whose centre ray meets the sphere within 0.8 R of the axis."""
    metal = rtw.Metal.fromColor([0.9, 0.9, 0.9], 0.0)
    cam = M.sky_camera(rtw, IW, ISPP, 2)
    img = {}
    for name, objs in (("flat", [rtw.worlds.icosphere(3, [0, 0, 0], IR, metal)]),
                       ("smooth", [rtw.worlds.icosphere(3, [0, 0, 0], IR, metal, smooth=True)]),
                       ("analytic", [rtw.Sphere.init([0, 0, 0], IR, metal)])):
        arr = rtw.flatten(objs)
        assert (arr.vertex_attrs is not None) == (name == "smooth")
        img[name] = M.render(rtw, arr, cam, ISPP, ISEED)[:, :3].astype(np.float64)
    idx, _, _, _ = _centre_hits(cam, IR, 0.8)
    assert len(idx) > 300
    e_smooth = np.abs(img["smooth"][idx] - img["analytic"][idx]).mean()
    e_flat = np.abs(img["flat"][idx] - img["analytic"][idx]).mean()
    print(f"mirror icosphere level 3 over {len(idx)} pixels: mean |smooth - analytic| {e_smooth:.4g}, "
          f"mean |flat - analytic| {e_flat:.4g}, ratio {e_smooth / e_flat:.3f}")
    assert e_flat > 0
    assert e_smooth <= 0.25 * e_flat


def test_texture_on_uv_mapped_icosphere(rtw):
    """An 8 x 4 image of distinct texels as a DiffuseLight on the smooth, uv-mapped level-3 icosphere and on the
    analytic Sphere, depth 1: at least 95 % of the selected pixels are the same texels in both (seams and texel
    borders may differ) -- as the float64 uv of the centre rays' hits already is."""
    tex = rtw.ImageTexture.init([S.texel_image(rtw)], 0)
    light = rtw.DiffuseLight.init(tex)
    cam = M.sky_camera(rtw, IW, ISPP, 1)
    mesh = rtw.worlds.icosphere(3, [0, 0, 0], IR, light, smooth=True, uv=True)
    idx, p, o, d = _centre_hits(cam, IR, 0.8)
    # float64: the mesh's interpolated uv against the sphere's own at the same centre rays
    out = p / IR
    sph_uv = np.stack([(np.arctan2(-out[:, 2], out[:, 0]) + np.pi) / (2 * np.pi), np.arccos(-out[:, 1]) / np.pi], 1)
    mesh_uv = _mesh_uv_f64(mesh, o, d)
    tx, ty = _texel(mesh_uv, 8, 4)
    sx, sy = _texel(sph_uv, 8, 4)
    same64 = ((tx == sx) & (ty == sy)).mean()
    a_mesh, a_sph = rtw.flatten([mesh]), rtw.flatten([rtw.Sphere.init([0, 0, 0], IR, light)])
    assert a_mesh.vertex_attrs is not None
    got = M.render(rtw, a_mesh, cam, ISPP, ISEED)[:, :3]
    ref = M.render(rtw, a_sph, cam, ISPP, ISEED)[:, :3]
    same = (got[idx] == ref[idx]).all(1).mean()
    print(f"texels over {len(idx)} pixels: float64 centre rays {same64:.4f} the same, rendered pixels {same:.4f}")
    assert same64 >= 0.95
    assert same >= 0.95
    # and more than one texel is in view
    assert len({(int(x), int(y)) for x, y in zip(sx, sy)}) >= 4


# ---------------------------------------------------------------- registration
def _plain(rtw):
    """Two triangles and a parallelogram at the top level, one triangle in an instance: quads 0..3."""
    lam = rtw.Lambertian.fromColor([0.6, 0.5, 0.4])
    objs = [rtw.Triangle.init([-3, -2, 0], [3, -2, 0], [0, 3, 0], lam),
            rtw.Quad.init([-4, -4, -2], [8, 0, 0], [0, 8, 0], lam),
            rtw.Triangle.init([-3, -2, 1], [0, -2, 2], [-2, 2, 1], rtw.Metal.fromColor([0.8] * 3, 0.0)),
            rtw.Translate.init(rtw.RotateY.init(rtw.Triangle.init([0, 0, 0], [2, 0, 0], [0, 2, 0], lam), 30), [1, 0, 3])]
    return objs


def _some_attrs(rtw, n):
    rng = np.random.default_rng(1)
    nrm = np.array([0, 0, 1.0]) + 0.4 * rng.normal(size=(n, 3, 3))
    return S.attr_records(rtw, n, (2.5 * nrm).astype(np.float32), rng.random((n, 3, 2)).astype(np.float32))


def test_registration(rtw):
    A = rtw._abi
    lib = rtw.lib()
    arr = rtw.flatten(_plain(rtw))
    assert arr.vertex_attrs is None and len(arr.quads) == 4
    cam = M.sky_camera(rtw, 32, 4, 8)
    never = M.render(rtw, arr, cam, 4, 3)
    world = rtw.World(arr, device=CPU)
    h0 = C.c_uint64()
    A.check(lib.rtw_scene_hash(world.handle, C.byref(h0)), "rtw_scene_hash")
    q0, a0 = world.vertex_attrs()
    assert len(q0) == 0 and len(a0) == 0
    idx = np.array([3, 0, 2], np.uint32)
    att = _some_attrs(rtw, 3)
    att["flags"][1] = A.RTW_ATTR_UVS
    world.set_vertex_attrs(idx, att)
    q1, a1 = world.vertex_attrs()
    assert q1.tolist() == [3, 0, 2]
    assert a1["flags"].tolist() == att["flags"].tolist()
    n64 = att["normal"].astype(np.float64)
    n64 /= np.linalg.norm(n64, axis=2, keepdims=True)
    assert np.abs(a1["normal"][[0, 2]] - n64[[0, 2]]).max() <= 3e-7           # stored normalised
    assert np.array_equal(a1["normal"][1], np.zeros((3, 3), np.float32))       # no flag: not stored
    assert np.array_equal(a1["uv"], att["uv"])
    h1 = C.c_uint64()
    A.check(lib.rtw_scene_hash(world.handle, C.byref(h1)), "rtw_scene_hash")
    assert h1.value != h0.value
    with_attrs = M.render(rtw, arr, cam, 4, 3, world=world)
    assert not np.array_equal(with_attrs, never)
    # every refusal names the entry and changes nothing
    bad = []
    def case(what, quads, recs):                                                                # noqa: E306
        bad.append((what, np.array(quads, np.uint32), recs))
    ok2 = _some_attrs(rtw, 2)
    case("out of range", [0, 4], ok2)
    case("parallelogram", [0, 1], ok2)
    case("listed twice", [2, 2], ok2)
    r = ok2.copy(); r["flags"][1] = 4 | A.RTW_ATTR_NORMALS; case("unknown flag", [0, 2], r)    # noqa: E702
    r = ok2.copy(); r["normal"][1, 2] = 0; case("zero normal", [0, 2], r)                      # noqa: E702
    r = ok2.copy(); r["normal"][1, 0, 1] = np.inf; case("non-finite normal", [0, 2], r)        # noqa: E702
    r = ok2.copy(); r["normal"][1, 1, 0] = np.nan; case("NaN normal", [0, 2], r)               # noqa: E702
    r = ok2.copy(); r["uv"][1, 2, 1] = np.nan; case("non-finite uv", [0, 2], r)                # noqa: E702
    for what, quads, recs in bad:
        rc = lib.rtw_scene_set_vertex_attrs(world.handle, quads.ctypes.data, recs.ctypes.data, len(quads))
        assert rc == A.RTW_E_INVALID, what
        msg = lib.rtw_last_error()
        assert b"rtw_scene_set_vertex_attrs" in msg and b"entry 1" in msg, (what, msg)
        q2, a2 = world.vertex_attrs()
        assert np.array_equal(q2, q1) and a2.tobytes() == a1.tobytes(), what
    # a non-finite value under a flag that is not set is ignored
    r = ok2.copy()
    r["flags"] = A.RTW_ATTR_UVS
    r["normal"][0] = np.nan
    world.set_vertex_attrs([0, 2], r)
    assert lib.rtw_scene_set_vertex_attrs(world.handle, None, None, 1) == A.RTW_E_INVALID
    # clear: the hash and the image of a context that never had attributes
    world.set_vertex_attrs(None)
    assert len(world.vertex_attrs()[0]) == 0
    h2 = C.c_uint64()
    A.check(lib.rtw_scene_hash(world.handle, C.byref(h2)), "rtw_scene_hash")
    assert h2.value == h0.value
    assert np.array_equal(M.render(rtw, arr, cam, 4, 3, world=world), never)
    # flags = 0 records: the attribute instantiations, the plain image
    world.set_vertex_attrs([0, 2, 3], np.zeros(3, A.VERTEX_ATTR_DT))
    assert np.array_equal(M.render(rtw, arr, cam, 4, 3, world=world), never)
    world.close()


def test_flatten_and_world_refuse_bad_attributes(rtw):
    """World registers what flatten collected; a parallelogram with attributes is refused by flatten itself."""
    lam = rtw.Lambertian.fromColor([0.5] * 3)
    q = rtw.Quad.init([0, 0, 0], [1, 0, 0], [0, 1, 0], lam)
    q.uvs = np.zeros((3, 2), np.float32)
    with pytest.raises(ValueError):
        rtw.flatten([q])
    tri = rtw.Triangle.init([0, 0, 0], [1, 0, 0], [0, 1, 0], lam, normals=np.zeros((3, 3)))
    with pytest.raises(rtw.RtwError):   # World applies the set; the library refuses the zero normal
        rtw.World(rtw.flatten([tri]), device=CPU)


# ---------------------------------------------------------------- Python
@pytest.mark.parametrize("name", ["ico1_v", "ico1_vn", "ico1_vt", "ico1_vtn"])
def test_load_obj_attributes(rtw, name):
    lam = rtw.Lambertian.fromColor([0.5] * 3)
    path = os.path.join(M.MESHES, name + ".obj")
    ref = rtw.worlds.icosphere(1, [0, 0, 0], 1.0, lam)
    plain = rtw.load_obj(path, lam)
    mesh = rtw.load_obj(path, lam, attributes=True)
    assert rtw.flatten([plain]).vertex_attrs is None
    assert all(t.normals is None and t.uvs is None for t in plain.objects)
    assert len(mesh.objects) == len(ref.objects) == 80
    for a, b, c in zip(mesh.objects, ref.objects, plain.objects):
        for f in "quv":
            assert np.array_equal(getattr(a, f), getattr(c, f))
            assert np.abs(getattr(a, f) - getattr(b, f)).max() <= 1e-6
    has_n, has_t = "n" in name.split("_")[1], "t" in name.split("_")[1]
    vts = []
    with open(path) as fh:
        for line in fh:
            tok = line.split()
            if tok and tok[0] == "vt":
                vts.append([float(x) for x in tok[1:3]])
    vts = np.array(vts, np.float32).reshape(-1, 2)
    for t in mesh.objects:
        assert (t.normals is not None) == has_n and (t.uvs is not None) == has_t
        if has_n:   # the unit sphere at the origin: a vertex's normal is its position (6 decimals in the file)
            corners = np.stack([t.q, t.q + t.u, t.q + t.v])
            assert np.abs(t.normals - corners).max() <= 1e-6
        if has_t:
            for c in t.uvs:
                assert (np.abs(vts - c).max(1) == 0).any()
    arr = rtw.flatten([mesh])
    if has_n or has_t:
        quads, recs = arr.vertex_attrs
        assert quads.tolist() == list(range(80))
        want = (rtw._abi.RTW_ATTR_NORMALS if has_n else 0) | (rtw._abi.RTW_ATTR_UVS if has_t else 0)
        assert (recs["flags"] == want).all()
    else:
        assert arr.vertex_attrs is None


def test_load_obj_text_forms(rtw):
    lam = rtw.Lambertian.fromColor([0.5] * 3)
    text = ("v 0 0 0\nv 1 0 0\nv 1 1 0\nv 0 1 0\nvn 0 0 1\nvn 0 1 1\nvt 0 0\nvt 1 0\nvt 1 1\nvt 0 1\n"
            "f 1/1/1 2/2/1 3/3/2 4/4/2\n"        # a fan of two, i/j/k
            "f 1//1 2//-1 3//2\n"                # i//k, a negative index
            "f -4/1 -3/2 -2/3\n"                 # i/j
            "f 1 2 3\n"                          # bare
            "f 1/1/1 2/2 3/3/1\n")               # one corner without a normal: uvs only
    m = rtw.load_obj(text, lam, attributes=True)
    t = m.objects
    assert len(t) == 6
    assert np.array_equal(t[0].normals, [[0, 0, 1], [0, 0, 1], [0, 1, 1]])
    assert np.array_equal(t[1].normals, [[0, 0, 1], [0, 1, 1], [0, 1, 1]])
    assert np.array_equal(t[1].uvs, [[0, 0], [1, 1], [0, 1]])
    assert np.array_equal(t[2].normals, [[0, 0, 1], [0, 1, 1], [0, 1, 1]]) and t[2].uvs is None
    assert t[3].normals is None and np.array_equal(t[3].uvs, [[0, 0], [1, 0], [1, 1]])
    assert t[4].normals is None and t[4].uvs is None
    assert t[5].normals is None and np.array_equal(t[5].uvs, [[0, 0], [1, 0], [1, 1]])
    for bad, line in (("v 0 0 0\nv 1 0 0\nv 0 1 0\nvn 0 0 1\nf 1//1 2//1 3//2\n", "line 5"),
                      ("v 0 0 0\nv 1 0 0\nv 0 1 0\nvt 0 0\n\nf 1/1 2/1 3/-2\n", "line 6")):
        with pytest.raises(ValueError, match=line):
            rtw.load_obj(bad, lam, attributes=True)
        assert len(rtw.load_obj(bad, lam).objects) == 1     # the default ignores them, as before


def test_flatten_places_records(rtw):
    """A smooth, uv-mapped mesh inside Translate(RotateY(...)) beside plain quads: the records sit on the mesh's quad
    indices, in corner order, object space."""
    A = rtw._abi
    lam = rtw.Lambertian.fromColor([0.5] * 3)
    mesh = rtw.worlds.icosphere(0, [1, 2, 3], 2.0, lam, smooth=True, uv=True)
    lone = rtw.Triangle.init([0, 0, 0], [1, 0, 0], [0, 1, 0], lam, uvs=[[0, 0], [0.5, 0], [0, 0.25]])
    objs = [rtw.Quad.init([0, 0, 0], [1, 0, 0], [0, 1, 0], lam), rtw.Triangle.init([0, 0, 1], [1, 0, 1], [0, 1, 1], lam),
            rtw.Translate.init(rtw.RotateY.init(mesh, 20), [5, 0, 0]), lone,
            rtw.Quad.init([0, 0, 5], [1, 0, 0], [0, 1, 0], lam)]
    arr = rtw.flatten(objs)
    quads, recs = arr.vertex_attrs
    assert recs.dtype == A.VERTEX_ATTR_DT and quads.dtype == np.uint32
    assert quads.tolist() == list(range(2, 22)) + [22]
    assert (recs["flags"][:20] == (A.RTW_ATTR_NORMALS | A.RTW_ATTR_UVS)).all() and recs["flags"][20] == A.RTW_ATTR_UVS
    for k, tri in enumerate(mesh.objects):
        assert np.array_equal(arr.quads[2 + k]["q"], tri.q)
        corners = np.stack([tri.q, tri.q + tri.u, tri.q + tri.v]).astype(np.float64) - [1, 2, 3]
        assert np.abs(recs["normal"][k] - corners / 2.0).max() <= 1e-6
        assert np.array_equal(recs["uv"][k], tri.uvs)
    assert np.array_equal(recs["uv"][20], np.array([[0, 0], [0.5, 0], [0, 0.25]], np.float32))
    # the defaults are unchanged
    assert rtw.flatten([rtw.worlds.icosphere(1, [0, 0, 0], 1.0, lam)]).vertex_attrs is None
    assert rtw.flatten(rtw.worlds.cornell_mesh()).vertex_attrs is None
    smooth = rtw.flatten(rtw.worlds.cornell_mesh(smooth=True))
    assert len(smooth.vertex_attrs[0]) == 320
    assert np.array_equal(smooth.quads, rtw.flatten(rtw.worlds.cornell_mesh()).quads)
    w = rtw.World(dataclasses.replace(smooth), device=CPU)
    assert len(w.vertex_attrs()[0]) == 320
    w.close()
