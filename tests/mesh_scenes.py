"""Scenes, inputs and renders shared by tests/test_triangles.py (host backend) and tests/test_gpu_triangles.py (GPU):
triangles (rtw_quad.shape = RTW_QUAD_TRIANGLE) at the top level, in list instances, in tree instances, as medium
boundaries and as lights.

Not a test module.  References are rendered once per process and returned read-only."""
import ctypes as C
import functools
import os

import numpy as np

import lights_scenes as S

CPU = S.CPU
MESHES = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "meshes")


def pkg():
    return S.pkg()


# ---------------------------------------------------------------- rtw_debug_quad_hit
def quad_records(rtw, q, u, v, shape):
    rec = np.zeros(len(q), rtw._abi.QUAD_DT)
    rec["q"], rec["u"], rec["v"] = q, u, v
    rtw._abi.quad_shape(rec)[...] = shape
    return rec


def quad_hit(rtw, rec, o, d, tmin, tmax):
    """rtw_debug_quad_hit over n pairs -> (hit, t, alpha_beta); t and alpha_beta are NaN where there is no hit."""
    n = len(rec)
    o, d = (np.ascontiguousarray(a, np.float32) for a in (o, d))
    tmin, tmax = (np.ascontiguousarray(a, np.float32) for a in (tmin, tmax))
    hit = np.zeros(n, np.uint8)
    t = np.full(n, np.nan, np.float32)
    ab = np.full((n, 2), np.nan, np.float32)
    rc = rtw.lib().rtw_debug_quad_hit(n, rec.ctypes.data, o.ctypes.data, d.ctypes.data, tmin.ctypes.data,
                                      tmax.ctypes.data, hit.ctypes.data, t.ctypes.data, ab.ctypes.data)
    rtw._abi.check(rc, "rtw_debug_quad_hit")
    return hit.astype(bool), t, ab


def _unit(x):
    return x / np.linalg.norm(x, axis=1, keepdims=True)


def random_pairs(n, seed=0):
    """n (triangle, ray, interval) pairs as float32 inputs, with some of the float64 construction's figures.

    The distribution is built from fp32's own error so that the parity bound can hold wherever the test demands it.
    With eps = 2^-24, Quad.hit's t = (D - n.o) / (n.d) sums products as large as the coordinates of q and o, so its
    numerator is off by about 3 eps X, X = |q| + |o| <~ S + lat + dist (S: the offset of the whole pair from the
    world origin, lat: the hit point's offset from the corner q, dist: origin to hit point).  That moves the hit
    point by 3 eps X / cos along the ray (cos = |n.d| / |d|), and alpha and beta by that over the triangle's
    least altitude h.  The test excludes pairs within 1e-4 of an edge, so every pair keeps
        X <= 100 cos h         (alpha, beta within ~2e-5: a fifth of the margin)
    which is a lower bound on cos for a given triangle and hit point: cos >= lat / (80 h), the rest of the budget
    going to S and dist.  Rays as grazing as that allows are drawn on purpose (below).  The populations:
      * longest edge L log-uniform in [0.05, 1000], coordinates up to 1e3; fat triangles (the sine of the angle
        between u and v in [0.3, 1]) and slivers (20 %: sine log-uniform in [0.05, 0.2], altitude down to L / 40);
      * hit points at (alpha, beta) uniform in [-0.5, 1.5]^2 -- about 1 in 8 inside the triangle, 0.1 % within 1e-4
        of an edge -- pulled towards the corner q where the bound above would ask for cos > 0.9 (slivers);
      * cos uniform in [cmin, 1], cmin = max(0.02, lat / (80 h)), and for a quarter of the pairs log-uniform in
        [cmin, min(1, 4 cmin)]: the most grazing rays fp32 resolves at that hit point;
      * t = 0.1 (dist / h) U[0.3, 1] within [1e-4, 10] (the direction's length is free): t's absolute error,
        t 3 eps X / (dist cos) <= 2e-5 t h / dist, then stays below 1e-5 max(1, |t|);
      * 5 % of the intervals end near the hit: tmin or tmax at a distance L 10^U[-5, -1] before or behind it along
        the ray (a quarter of them within the excluded 1e-4 L), the rest are (0.001 t, inf)."""
    rng = np.random.default_rng(seed)
    L = 10.0 ** rng.uniform(np.log10(0.05), 3.0, n)
    sliver = rng.random(n) < 0.2
    sin_uv = np.where(sliver, 10.0 ** rng.uniform(np.log10(0.05), np.log10(0.2), n), rng.uniform(0.3, 1.0, n))
    ang = np.arcsin(sin_uv)
    ang = np.where(rng.random(n) < 0.5, ang, np.pi - ang)      # acute and obtuse corners
    # an orthonormal frame (e1, e2, nrm); u along e1, v at the angle `ang` from it
    e1 = _unit(rng.normal(size=(n, 3)))
    e2 = _unit(np.cross(e1, rng.normal(size=(n, 3))))
    nrm = np.cross(e1, e2)
    lu = L * rng.uniform(0.5, 1.0, n)
    lv = L * rng.uniform(0.5, 1.0, n)
    u = lu[:, None] * e1
    v = lv[:, None] * (np.cos(ang)[:, None] * e1 + np.sin(ang)[:, None] * e2)
    h = np.minimum(lu, lv) * sin_uv
    a, b = rng.uniform(-0.5, 1.5, n), rng.uniform(-0.5, 1.5, n)
    lat = np.linalg.norm(a[:, None] * u + b[:, None] * v, axis=1)
    pull = np.minimum(1.0, 0.9 * 80.0 * h / np.maximum(lat, 1e-300))
    a, b, lat = a * pull, b * pull, lat * pull
    cmin = np.maximum(0.02, lat / (80.0 * h))
    graze = rng.random(n) < 0.25
    cos = np.where(graze, cmin * np.minimum(4.0, 1.0 / cmin) ** rng.random(n), rng.uniform(cmin, 1.0, n))
    rem = 100.0 * cos * h - lat
    S_mag = np.minimum(0.5 * rem, 1000.0)
    shift = rng.uniform(-1.0, 1.0, (n, 3)) * (S_mag / np.sqrt(3.0))[:, None]
    dist = np.minimum(0.5 * rem, 10.0 * L) * rng.uniform(0.01, 1.0, n)
    # the corner q: the hit point sits at `shift` from the world origin
    q = shift - (a[:, None] * u + b[:, None] * v)
    target = q + a[:, None] * u + b[:, None] * v
    # a unit direction at cosine `cos` to the normal, either side
    phi = rng.uniform(0, 2 * np.pi, n)
    side = np.where(rng.random(n) < 0.5, 1.0, -1.0)
    sn = np.sqrt(1.0 - cos * cos)
    dhat = (sn * np.cos(phi))[:, None] * e1 + (sn * np.sin(phi))[:, None] * e2 + (side * cos)[:, None] * nrm
    o = target - dist[:, None] * dhat
    t0 = np.clip(0.1 * (dist / h) * rng.uniform(0.3, 1.0, n), 1e-4, 10.0)
    d = dhat * (dist / t0)[:, None]
    tmin = 0.001 * t0
    tmax = np.full(n, np.inf)
    near = rng.integers(0, 80, n)         # 0..3: tmin just before / behind the hit, tmax just behind / before
    e = L * 10.0 ** rng.uniform(-5.0, -1.0, n) / (dist / t0)
    tmin = np.where(near == 0, t0 - e, np.where(near == 1, t0 + e, tmin))
    tmax = np.where(near == 2, t0 + e, np.where(near == 3, t0 - e, tmax))
    # every coordinate within 1e3: pairs that reach further are scaled down as a whole (every ratio above stays)
    reach = np.max([np.abs(x).max(1) for x in (q, q + u, q + v, o)], axis=0)
    k = np.minimum(1.0, 1000.0 / reach)
    q, u, v, o, d, L = q * k[:, None], u * k[:, None], v * k[:, None], o * k[:, None], d * k[:, None], L * k
    f = np.float32
    return dict(q=q.astype(f), u=u.astype(f), v=v.astype(f), o=o.astype(f), d=d.astype(f), tmin=tmin.astype(f),
                tmax=tmax.astype(f), L=L, sliver=sliver, graze=graze, cos=cos)


def reference_f64(p):
    """Quad.hit's t, alpha, beta of the float32 inputs in float64, and cos = |n.d| / (|n| |d|)."""
    q, u, v, o, d = (p[k].astype(np.float64) for k in "quvod")
    n = np.cross(u, v)
    nn = (n * n).sum(1)
    nd = (n * d).sum(1)
    with np.errstate(divide="ignore", invalid="ignore"):
        t = (n * (q - o)).sum(1) / nd
        planar = o + t[:, None] * d - q
        w = n / nn[:, None]
        alpha = (w * np.cross(planar, v)).sum(1)
        beta = (w * np.cross(u, planar)).sum(1)
        cos = np.abs(nd) / np.sqrt(nn * (d * d).sum(1))
    return t, alpha, beta, cos


# ---------------------------------------------------------------- scenes
def sky_camera(rtw, W, spp, depth, **kw):
    base = dict(aspect_ratio=1.0, vfov=80.0, lookfrom=(0.0, 0.0, 9.0), lookat=(0.0, 0.0, 0.0), vup=(0.0, 1.0, 0.0),
                defocus_angle=0.0, background_mode=rtw._abi.RTW_BG_GRADIENT)
    base.update(kw)
    return rtw.Camera(image_width=W, samples_per_pixel=spp, max_depth=depth, **base).init()


def quads_objects(rtw, split):
    """quads_world (five Lambertian quads), or each quad as its two triangles."""
    objs = rtw.worlds.quads_world()
    if not split:
        return objs
    return [t for q in objs for t in rtw.quad_triangles(q)]


def ico_objects(rtw, bvh, medium=False):
    """A level-1 icosphere (80 triangles, every edge shared by two) under RotateY + Translate, between the light and
    the ground of the instance-tree scenes; as a tree or a list; solid or the boundary of a ConstantMedium."""
    import instance_tree_scenes as T
    ico = rtw.worlds.icosphere(1, [0, 0, 0], 120, rtw.Lambertian.fromColor([0.73, 0.6, 0.5]), bvh=bvh)
    inst = rtw.Translate.init(rtw.RotateY.init(ico, 25), [278, 250, 200])
    objs = T._light_and_ground(rtw)
    return objs + [rtw.ConstantMedium.initFromColor(inst, 0.01, [0.9, 0.9, 0.9]) if medium else inst]


def ico_smoke_objects(rtw, bvh):
    """Cornell smoke's walls and light with the icosphere as the one medium's boundary: media beside quads under an
    instance tree."""
    walls, _ = rtw.worlds._cornell_walls([113, 554, 127], [330, 0, 0], [0, 0, 305], [7, 7, 7])
    ico = rtw.worlds.icosphere(1, [0, 0, 0], 120, rtw.Lambertian.fromColor([0.73, 0.73, 0.73]), bvh=bvh)
    inst = rtw.Translate.init(rtw.RotateY.init(ico, 25), [278, 200, 278])
    return walls + [rtw.ConstantMedium.initFromColor(inst, 0.01, [1, 1, 1])]


def mixed_objects(rtw):
    """Triangles in every place: cornell_mesh() -- two emissive and one free-standing triangle at the top level, 12
    in a list instance, 320 in a tree instance."""
    return rtw.worlds.cornell_mesh()


def render(rtw, arr, cam, spp, seed, device=CPU, tuning=None, world=None):
    return S.render(rtw, arr, cam, spp, seed, device=device, tuning=tuning, world=world)


# GPU tests: 64 x 64 x 6 spp (several waves per tile row; no multiple of the 16-sample run), depth 50
GW, GSPP, GDEPTH, GSEED = 64, 6, 50, 21


def cornell_mesh_camera(rtw):
    return rtw.cornell_camera(image_width=GW, spp=GSPP, max_depth=GDEPTH).init()


@functools.lru_cache(maxsize=None)
def cornell_mesh_host(lights):
    """cornell_mesh() on the host backend at the GPU tests' shape, with or without its two triangle lights."""
    rtw = pkg()
    arr = rtw.flatten(mixed_objects(rtw), lights="emissive" if lights else None)
    out = render(rtw, arr, cornell_mesh_camera(rtw), GSPP, GSEED)
    out.setflags(write=False)
    return out


# ---------------------------------------------------------------- the analytic triangle light
# the right triangle (q, q + u, q + v) in the plane of lights_scenes.LIGHT1, same corner and radiance: half of it
TRI_LIGHT = (S.LIGHT1[0], S.LIGHT1[1], S.LIGHT1[2], S.LIGHT1[3])


def tri_light_objects(rtw):
    floor = S.analytic_objects(rtw)[0]
    q, u, v, le = (np.array(a, np.float32) for a in TRI_LIGHT)
    return [floor, rtw.Triangle.init(q, q + u, q + v, rtw.DiffuseLight.fromColor([float(le)] * 3))]


def triangle_form_factor(points_xz, light, order=24):
    """integral over the triangle (q, q + u, q + v) of cos(theta) cos(theta') / r^2 dA for floor points (x, 0, z),
    normal +y: Gauss-Legendre in float64 on the unit square folded onto the triangle by the Duffy map
    (a, b) -> (a, (1 - a) b), Jacobian (1 - a)."""
    q, u, v, _ = (np.array(a, np.float64) for a in light)
    g, wg = np.polynomial.legendre.leggauss(order)
    g, wg = 0.5 * (g + 1), 0.5 * wg
    n = np.cross(u, v)
    par = np.linalg.norm(n)
    n = n / par
    p = np.stack([points_xz[:, 0], np.zeros(len(points_xz)), points_xz[:, 1]], axis=1)
    out = np.zeros(len(p))
    for a, wa in zip(g, wg):
        for b, wb in zip(g, wg):
            y = q + a * u + (1 - a) * b * v
            w = y - p
            r2 = (w * w).sum(1)
            r = np.sqrt(r2)
            cos_s = np.maximum(0.0, w[:, 1] / r)
            cos_l = np.abs(w @ n) / r
            out += wa * wb * (1 - a) * par * cos_s * cos_l / r2
    return out


@functools.lru_cache(maxsize=None)
def tri_light_seed_images(lights):
    """16 seeds x 256 spp of the triangle-light scene on the host backend: (16, pixels), as
    lights_scenes.analytic_seed_images."""
    rtw = pkg()
    arr = rtw.flatten(tri_light_objects(rtw), lights="emissive" if lights else None)
    cam = S.analytic_camera(rtw, S.SPP)
    world = rtw.World(arr, device=CPU)
    out = np.stack([S.render(rtw, arr, cam, S.SPP, s, world=world)[:, 0] / S.SPP for s in S.SEEDS]).astype(np.float64)
    world.close()
    out.setflags(write=False)
    return out
