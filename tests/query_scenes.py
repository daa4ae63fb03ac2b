"""Scenes, seeded ray sets and cached references shared by tests/test_query.py (host backend) and
tests/test_gpu_query.py (GPU): closest-hit and occlusion queries for caller-supplied rays (rtw_trace_rays,
rtw_occluded).

Not a test module.  A *case* is a named (scene arrays, tuning, rays) triple; CASES lists every case a host test uses,
and the GPU tests run each of them against the host context's records.  Ray sets are seeded and hold at most 4096
rays.  References are computed once per process and returned read-only."""
import functools
import math

import numpy as np

import denoise_scenes as D
import instance_tree_scenes as T

CPU = -1
N = 4096
F = np.float32


def pkgs():
    import importlib
    import oracle as O
    O.lib()
    return importlib.import_module("zig-raytracing-weekend_amd"), O


def frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays if len(arrays) > 1 else arrays[0]


# ---------------------------------------------------------------- scenes
def book1_64(rtw):
    """Book-1 capped at 64 spheres: the ground, every 8th of the small spheres up to 60, and the three large ones."""
    objs = rtw.worlds.generate_world(0, "book1")
    small = objs[1:-3][::8][:60]
    return [objs[0]] + small + objs[-3:]


def moving_world(rtw):
    """A ground sphere and 63 spheres over it, every second one moving (centre2 = centre1 + U[0, 0.5)^3)."""
    rng = np.random.default_rng(5)
    objs = [rtw.Sphere.init([0, -1000, 0], 1000, rtw.Lambertian.fromColor([0.5, 0.5, 0.5]))]
    for i in range(63):
        c = np.array([rng.uniform(-8, 8), rng.uniform(0.3, 1.5), rng.uniform(-8, 8)], F)
        r = F(rng.uniform(0.3, 0.8))
        mat = rtw.Lambertian.fromColor([0.3, 0.5, 0.7])
        if i % 2:
            objs.append(rtw.Sphere.initMoving(c, c + rng.uniform(0, 0.5, 3).astype(F), r, mat))
        else:
            objs.append(rtw.Sphere.init(c, r, mat))
    return objs


def mesh320(rtw):
    return rtw.worlds.icosphere(2, [0, 0, 0], 10, rtw.Lambertian.fromColor([0.7, 0.7, 0.7]))


@functools.lru_cache(maxsize=None)
def arrays(name):
    """(SceneArrays, tuning or None) of a named scene."""
    rtw, _ = pkgs()
    A, W = rtw._abi, rtw.worlds
    if name == "book1_64":
        return rtw.flatten(book1_64(rtw)), None
    if name == "book1_64_hoist0":      # the ground sphere under the tree's boxes
        return rtw.flatten(book1_64(rtw)), {"hoist": 0}
    if name == "quads":
        return rtw.flatten(W.quads_world()), None
    if name == "moving":
        return rtw.flatten(moving_world(rtw)), None
    if name == "book1":
        return rtw.flatten(W.generate_world(0, "book1")), None
    if name == "book1_orders8":
        return rtw.flatten(W.generate_world(0, "book1")), {"bvh_orders": 8}
    if name == "book1_hoist0":
        return rtw.flatten(W.generate_world(0, "book1")), {"hoist": 0}
    if name == "book1_reference":
        return rtw.flatten(W.generate_world(0, "book1"), bvh_mode=A.RTW_BVH_REFERENCE), None
    if name == "cornell":
        return rtw.flatten(W.cornell_box()), None
    if name == "cornell_list":
        return T.cornell_arrays(rtw, False), None
    if name == "cornell_tree":
        return T.cornell_arrays(rtw, True), None
    if name == "mesh_inst":      # 320 triangles as one instance without transforms: a private tree
        return rtw.flatten([mesh320(rtw)]), None
    if name == "mesh_top":       # the same triangles as 320 world objects
        return rtw.flatten(list(mesh320(rtw).objects)), None
    if name == "cornell_mesh":
        return rtw.flatten(W.cornell_mesh(smooth=True)), None
    if name.startswith("guide_"):
        arr, tuning, _ = D.scene(rtw, name[6:])
        return arr, tuning
    raise KeyError(name)


def world(name, device=CPU):
    rtw, _ = pkgs()
    arr, tuning = arrays(name)
    return rtw.World(arr, device=device, tuning=tuning)


# ---------------------------------------------------------------- ray sets
def pixel_centre_rays(cam):
    """The guide rays of a camera in guide_pixel's fp32 association: (pixel00 + du (x + off)) + dv (y + off), minus
    the centre; from the centre, time 0, unbounded."""
    rtw, _ = pkgs()
    d = cam.derived
    c, p00, du, dv = (np.array(v[:], F) for v in (d.center, d.pixel00_loc, d.pixel_delta_u, d.pixel_delta_v))
    ys, xs = np.mgrid[0:d.image_height, 0:d.image_width]
    fx = (xs.reshape(-1, 1) + d.pixel_offset).astype(F)
    fy = (ys.reshape(-1, 1) + d.pixel_offset).astype(F)
    pc = (p00 + du * fx) + dv * fy
    assert pc.dtype == F
    return rtw._abi.rays(np.broadcast_to(c, pc.shape), pc - c)


def prim_centres(arr):
    """A point inside every top-level sphere and quad (a triangle: its centroid) and every instance member, in world
    space for members of untransformed instances only."""
    pts = [arr.spheres["center1"][i] for i in range(len(arr.spheres))]
    rtw, _ = pkgs()
    for q in arr.quads:
        k = 3.0 if q[rtw._abi.QUAD_SHAPE] == rtw._abi.RTW_QUAD_TRIANGLE else 2.0
        pts.append(q["q"] + (q["u"] + q["v"]) / F(k))
    return np.array(pts, F)


def ray_set(seed, targets, box_lo, box_hi, shell_centre, shell_radius, n=N, time=0.0, upper=False, up=False):
    """n seeded rays: the first half start on a sphere around the scene and aim at one of `targets` (t = 1 there), the
    second half start inside the box [box_lo, box_hi] and point anywhere (|dir| in [0.5, 2)).  Every fourth ray is
    bounded: tmax in [0.2, 1.5) x the distance scale of its half.  upper: the shell's upper hemisphere only; up: the
    second half points upwards (dir.y >= 0)."""
    rtw, _ = pkgs()
    rng = np.random.default_rng(seed)
    h = n // 2
    v = rng.normal(size=(h, 3))
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    if upper:
        v[:, 1] = np.abs(v[:, 1])
    o1 = (np.asarray(shell_centre, np.float64) + shell_radius * v).astype(F)
    d1 = targets[rng.integers(0, len(targets), h)] - o1
    lo, hi = np.asarray(box_lo, np.float64), np.asarray(box_hi, np.float64)
    o2 = (lo + rng.random((n - h, 3)) * (hi - lo)).astype(F)
    w = rng.normal(size=(n - h, 3))
    w *= (rng.uniform(0.5, 2.0, (n - h, 1)) / np.linalg.norm(w, axis=1, keepdims=True))
    if up:
        w[:, 1] = np.abs(w[:, 1])
    d2 = w.astype(F)
    tmax = np.full(n, np.inf, F)
    scale = np.concatenate([np.ones(h), shell_radius / np.linalg.norm(d2, axis=1)])
    bounded = np.arange(n) % 4 == 3
    tmax[bounded] = (rng.uniform(0.2, 1.5, n) * scale)[bounded].astype(F)
    return rtw._abi.rays(np.concatenate([o1, o2]), np.concatenate([d1.astype(F), d2]), tmax, time)


def far_rays(seed, targets, extent, n=1024, upper=False):
    """Rays from 100 x extent away, each aimed at one of `targets` (t = 1 there), unbounded.  upper: from y > 0."""
    rtw, _ = pkgs()
    rng = np.random.default_rng(seed)
    v = rng.normal(size=(n, 3))
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    if upper:
        v[:, 1] = np.abs(v[:, 1])
    o = (100.0 * extent * v).astype(F)
    return rtw._abi.rays(o, targets[rng.integers(0, len(targets), n)] - o)


def advanced(rays, t0):
    """The same rays started at origin + t0 dir (fp32), direction unchanged."""
    r = rays.copy()
    r["origin"] = rays["origin"] + rays["dir"] * np.asarray(t0, F).reshape(-1, 1)
    return r


def cornell_targets(seed, n=512):
    """Points well inside the faces of the Cornell box's walls and of its two boxes' bounding region."""
    rng = np.random.default_rng(seed)
    return (55.0 + rng.random((n, 3)) * 445.0).astype(F)


def degenerate(rays):
    """`rays` with every 16th ray replaced in turn by a zero direction, a NaN origin, a NaN direction and an infinite
    direction component; returns (rays, mask of the replaced ones)."""
    r = rays.copy()
    bad = np.arange(len(r)) % 16 == 5
    k = np.nonzero(bad)[0]
    r["dir"][k[0::4]] = 0
    r["origin"][k[1::4], 1] = np.nan
    r["dir"][k[2::4], 0] = np.nan
    r["dir"][k[3::4], 2] = np.inf
    return r, bad


BRUTE = ("book1_64", "quads", "moving_t0", "moving_t05", "moving_t1")
GUIDES = D.SCENES + ("cornell_smoke_no_media",)
TREE_BOOK1 = ("book1", "book1_orders8", "book1_hoist0", "book1_reference")


@functools.lru_cache(maxsize=None)
def case(name):
    """(scene name, rays) of a named case; the rays are read-only."""
    rtw, _ = pkgs()
    if name.startswith("guide_"):
        return name, frozen(pixel_centre_rays(D.scene(rtw, name[6:])[2]))
    if name == "book1_64":
        arr, _ = arrays(name)
        return name, frozen(ray_set(101, prim_centres(arr), [-12, 0.05, -12], [12, 3, 12], [0, 0, 0], 30.0, upper=True))
    if name == "quads":
        # quadsWorld's last two quads coincide (the reference puts "upper_orange" and "lower_teal" both in the plane
        # y = -3): every hit there is a tie by construction.  So the set goes there seldom: one aimed ray in 199, from
        # above, and the second half starts above the plane and points upwards.
        arr, _ = arrays(name)
        c = prim_centres(arr)
        targets = np.concatenate([np.repeat(c[:3], 66, axis=0), c[3:4]])
        return name, frozen(ray_set(102, targets, [-4, -2.9, -1], [4, 4, 6], [0, 0, 3], 12.0, upper=True, up=True))
    if name.startswith("moving_t"):
        arr, _ = arrays("moving")
        time = {"moving_t0": 0.0, "moving_t05": 0.5, "moving_t1": 1.0}[name]
        return "moving", frozen(ray_set(103, prim_centres(arr), [-9, 0.05, -9], [9, 3, 9], [0, 0, 0], 25.0, time=time,
                                        upper=True))
    if name in TREE_BOOK1:
        arr, _ = arrays("book1")
        return name, frozen(ray_set(104, prim_centres(arr), [-12, 0.05, -12], [12, 3, 12], [0, 0, 0], 30.0, upper=True))
    if name in ("cornell_list", "cornell_tree"):
        return name, frozen(ray_set(105, cornell_targets(1), [1, 1, 1], [554, 554, 554], [278, 278, 278], 1200.0))
    if name in ("mesh_inst", "mesh_top"):
        arr, _ = arrays("mesh_top")
        return name, frozen(ray_set(106, prim_centres(arr), [-15, -15, -15], [15, 15, 15], [0, 0, 0], 40.0))
    if name == "far_book1":
        # 1024 rays from 100 x extent that Sphere.hit's fp32 arithmetic resolves (resolved(), below), of 8192 candidates
        # aimed at the primitive centres, at points of the ground sphere 150 .. 1000 from its top, and past its horizon
        arr, _ = arrays("book1_64")
        rng = np.random.default_rng(7)
        ang, rho = rng.uniform(0, 2 * np.pi, 8192), rng.uniform(150.0, 1400.0, 8192)
        y = np.where(rho < 1000.0, np.sqrt(np.maximum(1e6 - rho * rho, 0.0)) - 1000.0, 0.0)
        ground = np.stack([rho * np.cos(ang), y, rho * np.sin(ang)], 1).astype(F)
        cand = far_rays(107, np.concatenate([prim_centres(arr), ground]), extent_of("book1_64"), n=8192, upper=True)
        return "book1_64", frozen(cand[resolved(cand, arr)][:1024])
    if name == "far_book1_hoist0":
        return "book1_64_hoist0", case("far_book1")[1]
    if name in ("far_aimed_book1", "far_aimed_book1_hoist0"):
        # every far ray aimed at a primitive centre, resolved or not: fp32 cannot tell which small sphere such a ray
        # hits, so there is no oracle for it, but a GPU context (FMA slab test, switched off per ray) and a host
        # context (aabb.zig's arithmetic throughout) must still give the same records
        arr, _ = arrays("book1_64")
        rays = frozen(far_rays(107, prim_centres(arr), extent_of("book1_64")))
        return ("book1_64" if name == "far_aimed_book1" else "book1_64_hoist0"), rays
    if name in ("far_grazing_book1", "far_grazing_book1_hoist0"):
        # horizontal rays from 100 x extent through a point just under the top (or over the bottom) of a small sphere:
        # they graze the sphere where it touches its leaf's box, so a box test that is not conservative from there
        # (the FMA slab test: its pad covers origins within 7 x extent) culls what the exact one keeps
        arr, _ = arrays("book1_64")
        rng = np.random.default_rng(11)
        k = rng.integers(1, len(arr.spheres), 1024)
        c, r = arr.spheres["center1"][k].astype(np.float64), arr.spheres["radius"][k].astype(np.float64)
        side = np.where(rng.random(1024) < 0.5, 1.0, -1.0)
        point = c + np.stack([np.zeros(1024), side * r * (1.0 - rng.uniform(0.0, 1e-2, 1024)), np.zeros(1024)], 1)
        az = rng.uniform(0, 2 * np.pi, 1024)
        o = (point - 100.0 * extent_of("book1_64") * np.stack([np.cos(az), np.zeros(1024), np.sin(az)], 1)).astype(F)
        rays = frozen(rtw._abi.rays(o, point.astype(F) - o))
        return ("book1_64" if name == "far_grazing_book1" else "book1_64_hoist0"), rays
    if name == "flat_cornell_mesh":
        return "guide_cornell_mesh_flat", case("attr_cornell_mesh")[1]
    if name == "permuted_cornell_tree":
        _, rays = case("cornell_tree")
        return "cornell_tree", frozen(rays[np.random.default_rng(3).permutation(len(rays))])
    if name == "far_cornell":
        # from above only: the two boxes stand on the floor, so from below a box's bottom face and the floor are hit
        # at the same point -- a tie by construction, which rounding decides differently from far and from near
        return "cornell", frozen(far_rays(108, cornell_targets(2), extent_of("cornell"), upper=True))
    if name == "near_cornell":
        # the far rays advanced to 1000 units before their targets: outside the 555-unit box, inside 7 x extent
        _, far = case("far_cornell")
        len_d = np.linalg.norm(far["dir"].astype(np.float64), axis=1)
        return "cornell", frozen(advanced(far, 1.0 - 1000.0 / len_d))
    if name == "attr_cornell_mesh":
        # aimed at the icosphere (radius 90, centre (82.5, 100, 82.5) under RotateY 15 + Translate (265, 0, 295): in
        # the world (366, 100, 353)) from inside the room, and anywhere
        rng = np.random.default_rng(9)
        ball = (np.array([366.0, 100.0, 353.0]) + rng.normal(size=(256, 3)) * 40.0).astype(F)
        return "cornell_mesh", frozen(ray_set(109, ball, [1, 1, 1], [554, 554, 554], [278, 278, 100], 150.0, n=2048))
    if name == "degenerate":
        _, rays = case("book1_64")
        return "book1_64", frozen(degenerate(rays[:1024])[0])
    if name == "tmax_bad":
        _, rays = case("book1_64")
        r = rays[:768].copy()
        r["tmax"] = np.repeat(np.array([np.nan, 0.0, 0.001], F), 256)
        return "book1_64", frozen(r)
    if name.startswith("tmax_eq_") or name.startswith("tmax_next_"):
        base = name.split("_", 2)[2]
        scene, rays = case(base)
        hits, _ = host(base)
        r = rays[hits["kind"] != 0xFFFFFFFF].copy()
        t = hits["t"][hits["kind"] != 0xFFFFFFFF]
        r["tmax"] = t if name.startswith("tmax_eq_") else np.nextafter(t, F(np.inf))
        return scene, frozen(r)
    raise KeyError(name)


TMAX_BASES = ("book1_64", "quads", "moving_t05", "cornell_tree")
CASES = tuple("guide_" + s for s in GUIDES) + BRUTE + TREE_BOOK1 + (
    "cornell_list", "cornell_tree", "mesh_inst", "mesh_top", "far_book1", "far_book1_hoist0", "far_aimed_book1",
    "far_aimed_book1_hoist0", "far_grazing_book1", "far_grazing_book1_hoist0", "flat_cornell_mesh", "permuted_cornell_tree", "far_cornell", "near_cornell",
    "attr_cornell_mesh", "degenerate", "tmax_bad") + tuple(
    p + b for b in TMAX_BASES for p in ("tmax_eq_", "tmax_next_"))


@functools.lru_cache(maxsize=None)
def extent_of(scene):
    w = world(scene)
    e = w.stats()["extent"]
    w.close()
    return e


@functools.lru_cache(maxsize=None)
def host(name):
    """(hits, occluded) of a case on the host backend, read-only."""
    scene, rays = case(name)
    w = world(scene)
    hits, occ = w.trace(rays), w.occluded(rays)
    w.close()
    return frozen(hits, occ)


# ---------------------------------------------------------------- the oracle's brute force
def resolved(rays, arr):
    """Rays for which fp32 Sphere.hit decides hit or miss of every sphere of `arr` as exact arithmetic does: the
    discriminant hb^2 - a c, evaluated in float64, exceeds in size 8 x 2^-24 x (hb^2 + a (|oc|^2 + r^2)) -- the
    roundings of the fp32 evaluation (three-term dot products, two products, two differences: at most six half-ulp
    steps on terms of that size).  Computed from the geometry alone: no library and no oracle call.  From 2e5 units
    out a ray must pass some 140 units clear of a sphere of radius 0.2 to be told from one that hits it; where it
    is not, a brute force over all spheres "hits" whatever rounding offers, and is no reference for any walk."""
    o, d, time = (rays[k].astype(np.float64) for k in ("origin", "dir", "time"))
    ok = np.ones(len(rays), bool)
    for s in arr.spheres:
        c = s["center1"].astype(np.float64)
        if s["is_moving"]:
            c = c + time[:, None] * (s["center2"].astype(np.float64) - c)
        oc = o - c
        a, hb, oo = (d * d).sum(1), (oc * d).sum(1), (oc * oc).sum(1)
        r2 = float(s["radius"]) ** 2
        ok &= np.abs(hb * hb - a * (oo - r2)) > 8 * 2.0 ** -24 * (hb * hb + a * (oo + r2))
    return ok


@functools.lru_cache(maxsize=None)
def brute_force(name):
    """The closest hit of every ray of a case over the scene's top-level spheres and quads by oracle_sphere_hit /
    oracle_quad_hit on (0.001, tmax): (t -- inf on a miss --, kind, index, how many primitives attain t, the front
    flag, p), read-only.
    Spheres are tested only where a float64 discriminant, widened by 1e-4 of its terms, is not negative: the fp32
    discriminant of a pair left out is far below zero, and Sphere.hit rejects it."""
    _, O = pkgs()
    scene, rays = case(name)
    arr, _ = arrays(scene)
    assert len(arr.instances) == 0 and len(arr.media) == 0
    L = O.lib()
    n = len(rays)
    best = np.full(n, np.inf, F)
    kind = np.full(n, 0xFFFFFFFF, np.uint32)
    index = np.full(n, 0xFFFFFFFF, np.uint32)
    count = np.zeros(n, np.int64)
    front = np.zeros(n, np.uint32)
    point = np.zeros((n, 3), F)
    o64, d64 = rays["origin"].astype(np.float64), rays["dir"].astype(np.float64)
    out = np.zeros(10, F)
    orig, dirs, tmax, time = (np.ascontiguousarray(rays[k]) for k in ("origin", "dir", "tmax", "time"))

    def take(i, t, k, j):
        if not (t < tmax[i]):      # Quad.hit's interval is closed; the query's is open at tmax
            return
        if t < best[i]:
            best[i], kind[i], index[i], count[i] = t, k, j, 1
            front[i], point[i] = out[7] != 0, out[1:4]
        elif t == best[i]:
            count[i] += 1

    for j, s in enumerate(arr.spheres):
        c = s["center1"].astype(np.float64)
        if s["is_moving"]:
            c = c + time.astype(np.float64)[:, None] * (s["center2"].astype(np.float64) - c)
        oc = o64 - c
        a, hb, oo = (d64 * d64).sum(1), (oc * d64).sum(1), (oc * oc).sum(1)
        r2 = float(s["radius"]) ** 2
        disc = hb * hb - a * (oo - r2)
        rec = arr.spheres[j:j + 1]
        for i in np.nonzero(disc >= -1e-4 * (hb * hb + a * (oo + r2)))[0]:
            if L.oracle_sphere_hit(rec.ctypes.data, orig[i].ctypes.data, dirs[i].ctypes.data, float(time[i]), 0.001,
                                   float(tmax[i]), out.ctypes.data):
                take(i, out[0], 0, j)
    for j in range(len(arr.quads)):
        rec = arr.quads[j:j + 1]
        for i in range(n):
            if L.oracle_quad_hit(rec.ctypes.data, orig[i].ctypes.data, dirs[i].ctypes.data, 0.001, float(tmax[i]),
                                 out.ctypes.data):
                take(i, out[0], 1, j)
    return frozen(best, kind, index, count, front, point)


# ---------------------------------------------------------------- attributes: the object space of cornell_mesh's ball
def ball_object_space(rays):
    """World rays in the object space of cornell_mesh's icosphere instance (Translate(RotateY(ball, 15), (265, 0,
    295))) by inst_to_object's fp32 operations, and the function taking object-space normals back to the world
    (inst_to_world).  sin / cos as RotateY.init computes them: fp32 sin / cos of 15 pi / 180 in fp32."""
    radians = F(F(15.0) * F(3.1415926535897932385)) / F(180.0)
    sn, cs = F(math.sin(float(radians))), F(math.cos(float(radians)))
    o = rays["origin"] - np.array([265, 0, 295], F)
    d = rays["dir"]

    def rot(v):
        out = v.copy()
        out[:, 0] = cs * v[:, 0] - sn * v[:, 2]
        out[:, 2] = sn * v[:, 0] + cs * v[:, 2]
        return out

    def normal_to_world(nrm):
        out = nrm.copy()
        out[:, 0] = cs * nrm[:, 0] + sn * nrm[:, 2]
        out[:, 2] = -sn * nrm[:, 0] + cs * nrm[:, 2]
        return out

    return rot(o), rot(d), normal_to_world
