"""Scenes, cameras and the float64 reference shared by tests/test_tile_lists.py (no GPU) and
tests/test_gpu_tile_lists.py (GPU): the camera-ray candidate lists of static sphere scenes (rtw_tuning.tile_lists;
csrc/rtw_wavefront.hip: tile_frustum, tile_reach, wf_tile_lists, wf_tile_lists_walk).

Not a test module.  The reference is plain numpy float64 and takes nothing from the code under test but the camera
struct (rtw_camera, rtw_debug_camera_ray) and the tree's leaves (rtw_scene_nodes).  References are computed once per
process and returned read-only.

Per 8x8 tile of a rendered pixel range:
  T     the spheres some ray of the tile hits at a ray parameter Sphere.hit accepts (t > 0.001, either root) -- the
        real rays of samples 0..7 of every rendered pixel, and extreme rays built from the camera's fields (the tile's
        corner pixels with jitter +-0.5, origins on the rim and at the centre of the defocus disk) -- with the smallest
        such parameter, t_min
  R0    the documented bound (the comment above TileFrustum and tile_reach) restated with every margin at zero: what
        any implementation of the bound must keep
  R2    the same with each of the code's margins doubled (2e-3 relative and 2e-5 absolute slack, sec x 1.002,
        tlow x 0.9998): fp32 rounding of these expressions is of the order 1e-6 relative, three orders below the
        margins, so fp32 code that implements the bound lies between R0 and R2
"""
import ctypes as C
import functools

import numpy as np

CPU = -1
f32, f64 = np.float32, np.float64
LEAF_BIT = 0x80000000
TL_WALK = 0xFFFFFFFF
TL_MAX = 128
T_MIN = 0.001  # Sphere.hit's lower end (objects.zig:127-136)

MARGINS_R0 = dict(slack_rel=0.0, slack_abs=0.0, sec_factor=1.0, tlow_factor=1.0)
MARGINS_R2 = dict(slack_rel=2e-3, slack_abs=2e-5, sec_factor=1.002, tlow_factor=0.9998)
# the code's own margins: R1 is no bound for a test, only the record of how far the fp32 lists are from their float64 twin
MARGINS_R1 = dict(slack_rel=1e-3, slack_abs=1e-5, sec_factor=1.001, tlow_factor=0.9999)


def pkg():
    import importlib
    return importlib.import_module("zig-raytracing-weekend_amd")


# ---------------------------------------------------------------- scenes and cameras
@functools.lru_cache(maxsize=None)
def arrays(scene):
    rtw = pkg()
    if scene == "book1":
        return rtw.flatten(rtw.worlds.generate_world(0, "book1"))
    assert scene == "stress"
    return rtw.flatten(rtw.worlds.stress_world(3000, 5))


# name -> (Camera fields, strata, (pix_begin, pix_end) in units of (rows, pixels) or None)
_BASE = dict(samples_per_pixel=4, max_depth=8, lookat=(0.0, 0.0, 0.0), pixel_offset=0)
_CAM_I = dict(_BASE, lookfrom=(13.0, 2.0, 3.0), vfov=60.0, defocus_angle=0.6, focus_dist=10.0)
_CAM_II = dict(_BASE, lookfrom=(20.0, 6.0, 5.0), vfov=30.0, defocus_angle=0.6, focus_dist=10.0)
CAMERAS = {
    "i": (dict(_CAM_I, image_width=40, image_height=24), 0, None),
    "ii": (dict(_CAM_II, image_width=43, image_height=21), 0, None),
    "iii": (dict(_BASE, lookfrom=(0.0, 30.0, 0.1), vfov=50.0, defocus_angle=0.0, focus_dist=10.0, image_width=40,
                 image_height=24), 0, None),
    "iv": (dict(_BASE, lookfrom=(2.0, 0.5, 1.0), lookat=(0.0, 0.5, 0.0), vfov=90.0, defocus_angle=12.0, focus_dist=0.5,
                image_width=43, image_height=21), 0, None),
    "v": (dict(_CAM_I, image_width=72, image_height=64), 0, None),
    "vi": (dict(_CAM_II, image_width=43, image_height=21, pixel_offset=1), 3, None),
    # rows 5 (from x = 3) .. 13 (up to x = 8): the second row of tiles holds row 13 alone, so its tiles right of x = 15
    # have no rendered pixel, and the tiles of the first and last pixels are partly rendered
    "vii": (dict(_CAM_II, image_width=43, image_height=21), 0, ((5, 3), (13, 9))),
}


@functools.lru_cache(maxsize=None)
def camera(name):
    """(initialised Camera, pix_begin, pix_end) of a case."""
    rtw = pkg()
    fields, strata, rng = CAMERAS[name]
    cam = rtw.Camera(aspect_ratio=fields["image_width"] / fields["image_height"],
                     background_mode=rtw._abi.RTW_BG_GRADIENT, strata=strata, **fields).init()
    w = cam.derived.image_width
    assert (w, cam.derived.image_height) == (fields["image_width"], fields["image_height"])
    if rng is None:
        return cam, 0, cam.size
    (r0, p0), (r1, p1) = rng
    return cam, r0 * w + p0, r1 * w + p1


def universe(nodes):
    """The spheres of a tree: (ids, centres (N, 3) float32, radii (N,) float32) of every ordering-0 node with the leaf
    bit (hoisted leaves included); id = node index."""
    a = np.ascontiguousarray(nodes["a"])
    ids = np.flatnonzero(a.view(np.uint32)[:, 3] & LEAF_BIT).astype(np.uint32)
    return ids, a[ids, :3].copy(), np.abs(nodes["b"][ids, 0]).astype(f32)


@functools.lru_cache(maxsize=None)
def scene_universe(scene, device=CPU):
    """universe() of the scene's tree as a context on `device` builds it by default."""
    rtw = pkg()
    world = rtw.World(arrays(scene), device=device)
    out = universe(world.nodes())
    world.close()
    for v in out:
        v.setflags(write=False)
    return out


# ---------------------------------------------------------------- tiles of a rendered range (wf_pixel)
def tile_grid(cam, pix_begin, pix_end):
    """(n_tx, row0, n_tiles) of the range, as run_wavefront lays the batch out."""
    w = cam.image_width
    row0 = pix_begin // w
    n_rows = (pix_end - 1) // w - row0 + 1
    n_tx = (w + 7) // 8
    return n_tx, row0, n_tx * ((n_rows + 7) // 8)


def tile_pixels(cam, pix_begin, pix_end, n_tx, row0, t):
    """(xs, ys) of the rendered pixels of tile t: x in 8 (t % n_tx) .. +7, rows row0 + 8 (t // n_tx) .. +7, clipped to
    the image and to [pix_begin, pix_end)."""
    w, h = cam.image_width, cam.image_height
    last_row = (pix_end - 1) // w
    xs, ys = np.meshgrid(8 * (t % n_tx) + np.arange(8), row0 + 8 * (t // n_tx) + np.arange(8))
    xs, ys = xs.ravel(), ys.ravel()
    pix = ys * w + xs
    ok = (xs < w) & (ys < h) & (ys <= last_row) & (pix >= pix_begin) & (pix < pix_end)
    return xs[ok], ys[ok]


# ---------------------------------------------------------------- the bound, restated in float64
def _v(x):
    return np.array(list(x), f64)


def frustum(cam, x0, x1, y0, y1, sec_factor=1.0):
    """The tile's ray set (the comment above TileFrustum): every ray starts within rd of the camera centre in the
    plane through it, and passes through the rectangle [ru0, ru1] x [rv0, rv1] of the pixel plane (pixel centres
    widened by the +-0.5 jitter) at depth h along fz; sec bounds 1 / cos of a ray's angle to fz."""
    du, dv, ctr = _v(cam.pixel_delta_u), _v(cam.pixel_delta_v), _v(cam.center)
    fw = np.cross(du, dv)
    fl, ul, vl = np.linalg.norm(fw), np.linalg.norm(du), np.linalg.norm(dv)
    with np.errstate(all="ignore"):
        fz, uh, vh = fw / fl, du / ul, dv / vl
    p0 = _v(cam.pixel00_loc) - ctr
    h, pu, pv = p0 @ fz, p0 @ uh, p0 @ vh
    off = float(cam.pixel_offset)
    F = dict(ctr=ctr, fz=fz, uh=uh, vh=vh, h=h,
             ok=bool(h > 0 and fl > 0 and abs(du @ dv) <= 1e-4 * ul * vl),
             ru0=pu + (x0 + off - 0.5) * ul, ru1=pu + (x1 + off + 0.5) * ul,
             rv0=pv + (y0 + off - 0.5) * vl, rv1=pv + (y1 + off + 0.5) * vl,
             rd=max(np.linalg.norm(_v(cam.defocus_disk_u)), np.linalg.norm(_v(cam.defocus_disk_v)))
             if cam.defocus_angle > 0 else 0.0)
    mu, mv = max(abs(F["ru0"]), abs(F["ru1"])), max(abs(F["rv0"]), abs(F["rv1"]))
    with np.errstate(all="ignore"):  # (h = 0: no frame)
        tphi = (np.hypot(mu, mv) + F["rd"]) / h
    F["sec"] = np.sqrt(1.0 + tphi * tphi) * sec_factor
    return F


def reach(F, centres, radii, slack_rel=0.0, slack_abs=0.0, tlow_factor=1.0, **_):
    """Can a ray of the tile pass within rho of c?  -> (keep (N,) bool, tlow (N,) float64).  With z the depth of c
    along fz: rays only go forward, so a sphere wholly behind the camera plane (z < -rho) is out; all rays reach
    depth z at t = z / h, where they lie in the rectangle scaled by t widened by |1 - t| rd, and a ray passes within
    rho of c only if that cross-section comes within rho sec of c; such a hit has t >= (z - rho) / h.  A sphere that
    reaches the camera plane (z <= rho) is hit at depth <= z + rho, so t <= t1 = (z + rho) / h, within
    max(1, t1) rd + t1 |T|max of the axis (T: a target in the rectangle): it is kept when its centre is within rho
    of that, with tlow 0."""
    with np.errstate(all="ignore"):
        cc = np.asarray(centres, f64) - F["ctr"]
        rho = np.asarray(radii, f64)
        z, cu, cv = cc @ F["fz"], cc @ F["uh"], cc @ F["vh"]
        slack = slack_rel * (np.abs(z) + np.abs(cu) + np.abs(cv) + rho) + slack_abs
        behind = z < -(rho + slack)
        front = z > rho + slack
        t1 = np.maximum(0.0, (z + rho + slack) / F["h"])
        tmax = np.sqrt(max(F["ru0"] ** 2, F["ru1"] ** 2) + max(F["rv0"] ** 2, F["rv1"] ** 2))
        lat = np.hypot(cu, cv)
        keep_s = ~(lat > rho + np.maximum(1.0, t1) * F["rd"] + t1 * tmax + slack)
        t = z / F["h"]
        dx = np.maximum(0.0, np.maximum(t * F["ru0"] - cu, cu - t * F["ru1"]))
        dy = np.maximum(0.0, np.maximum(t * F["rv0"] - cv, cv - t * F["rv1"]))
        gap = np.hypot(dx, dy) - np.abs(1.0 - t) * F["rd"]
        keep_f = ~(gap > rho * F["sec"] + slack)
        tlow_f = np.maximum(0.0, (z - rho - slack) / F["h"] * tlow_factor)
    keep = np.where(behind, False, np.where(front, keep_f, keep_s))
    return keep, np.where(front, tlow_f, 0.0)


def reach_with(cam, bounds, centres, radii, margins):
    return reach(frustum(cam, *bounds, sec_factor=margins["sec_factor"]), centres, radii, **margins)


# ---------------------------------------------------------------- rays and exact intersection
def extreme_rays(cam, bounds):
    """Rays (b): targets at the four corner pixels of `bounds` with jitter +-0.5, origins at 8 points of the rim of
    the defocus disk and at its centre (the centre alone without defocus).  -> (origins, dirs), float64; dir =
    target - origin, so the focus plane is at t = 1."""
    x0, x1, y0, y1 = bounds
    p00, du, dv, ctr = _v(cam.pixel00_loc), _v(cam.pixel_delta_u), _v(cam.pixel_delta_v), _v(cam.center)
    off = float(cam.pixel_offset)
    targets = [p00 + (x + off + px) * du + (y + off + py) * dv
               for x in (x0, x1) for y in (y0, y1) for px in (-0.5, 0.5) for py in (-0.5, 0.5)]
    origins = [ctr]
    if cam.defocus_angle > 0:
        ku, kv = _v(cam.defocus_disk_u), _v(cam.defocus_disk_v)
        origins += [ctr + np.cos(p) * ku + np.sin(p) * kv for p in np.arange(8) * (np.pi / 4)]
    o = np.array([o for o in origins for _ in targets])
    return o, np.array([t for _ in origins for t in targets]) - o


def real_rays(rtw, cam, xs, ys, n_samples=8, seed=0):
    """Rays (a): rtw_debug_camera_ray of samples 0 .. n_samples - 1 of the pixels (xs, ys)."""
    pix = np.repeat((ys * cam.image_width + xs).astype(np.uint32), n_samples)
    smp = np.tile(np.arange(n_samples, dtype=np.uint32), len(xs))
    o, d = np.full((len(pix), 3), np.nan, f32), np.full((len(pix), 3), np.nan, f32)
    rc = rtw.lib().rtw_debug_camera_ray(C.byref(cam), seed, len(pix), pix.ctypes.data, smp.ctypes.data, o.ctypes.data,
                                        d.ctypes.data, None, None)
    rtw._abi.check(rc, "rtw_debug_camera_ray")
    return o.astype(f64), d.astype(f64)


def first_hits(o, d, centres, radii):
    """Per sphere the smallest root t > 0.001 of |o + t d - c| = r over the rays (inf: none hits it)."""
    c, r = np.asarray(centres, f64), np.asarray(radii, f64)
    best = np.full(len(c), np.inf)
    a = np.einsum("ij,ij->i", d, d)[:, None]
    for s in range(0, len(c), 1024):  # (rays x spheres blocks)
        oc = o[:, None, :] - c[None, s:s + 1024, :]
        hb = np.einsum("rsj,rj->rs", oc, d)
        disc = hb * hb - a * (np.einsum("rsj,rsj->rs", oc, oc) - r[None, s:s + 1024] ** 2)
        with np.errstate(invalid="ignore"):
            sq = np.sqrt(disc)
            for root in ((-hb - sq) / a, (-hb + sq) / a):
                best[s:s + 1024] = np.minimum(best[s:s + 1024], np.where(root > T_MIN, root, np.inf).min(axis=0))
    return best


# ---------------------------------------------------------------- the reference of a case
@functools.lru_cache(maxsize=None)
def reference(scene, cam_name, device=CPU):
    """The case's tiles against the scene's spheres: a dict of n_tx, row0, n_tiles, ids / centres / radii (the
    universe, N spheres), and per tile: bounds (n_tiles, 4) = x0, x1, y0, y1 of its rendered pixels (NaN: none),
    t_min (n_tiles, N; inf = not in T), R0, R2 (n_tiles, N) bool, tlow0, tlow2 (n_tiles, N); R1 (n_tiles, N) bool,
    the restatement at the code's own margins, for the record only."""
    rtw = pkg()
    camobj, pix_begin, pix_end = camera(cam_name)
    cam = camobj.derived
    ids, centres, radii = scene_universe(scene, device)
    n_tx, row0, n_tiles = tile_grid(cam, pix_begin, pix_end)
    n = len(ids)
    ref = dict(n_tx=n_tx, row0=row0, n_tiles=n_tiles, ids=ids, centres=centres, radii=radii,
               bounds=np.full((n_tiles, 4), np.nan), t_min=np.full((n_tiles, n), np.inf),
               R0=np.zeros((n_tiles, n), bool), R2=np.zeros((n_tiles, n), bool), R1=np.zeros((n_tiles, n), bool),
               tlow0=np.zeros((n_tiles, n)), tlow2=np.zeros((n_tiles, n)))
    for t in range(n_tiles):
        xs, ys = tile_pixels(cam, pix_begin, pix_end, n_tx, row0, t)
        if not len(xs):
            continue
        b = (float(xs.min()), float(xs.max()), float(ys.min()), float(ys.max()))
        ref["bounds"][t] = b
        oa, da = real_rays(rtw, cam, xs, ys)
        ob, db = extreme_rays(cam, b)
        ref["t_min"][t] = first_hits(np.concatenate([oa, ob]), np.concatenate([da, db]), centres, radii)
        ref["R0"][t], ref["tlow0"][t] = reach_with(cam, b, centres, radii, MARGINS_R0)
        ref["R2"][t], ref["tlow2"][t] = reach_with(cam, b, centres, radii, MARGINS_R2)
        ref["R1"][t] = reach_with(cam, b, centres, radii, MARGINS_R1)[0]
    for v in ref.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return ref


def bands(ref):
    """Tiles by |R0|: (empty, 1..32, 33..64, 65..128, > 128)."""
    k = ref["R0"].sum(axis=1)
    return (int((k == 0).sum()), int(((k >= 1) & (k <= 32)).sum()), int(((k >= 33) & (k <= 64)).sum()),
            int(((k >= 65) & (k <= 128)).sum()), int((k > 128).sum()))


def tile_reach_fp32(rtw, cam, bounds, centres, radii):
    """rtw_debug_tile_reach: the builders' fp32 geometry on the host -> (reach bool, tlow float32, frame_ok)."""
    c = np.ascontiguousarray(centres, f32).reshape(-1, 3)
    r = np.ascontiguousarray(radii, f32).reshape(-1)
    keep, tlow, ok = np.full(len(r), 255, np.uint8), np.full(len(r), np.nan, f32), C.c_uint8(255)
    rc = rtw.lib().rtw_debug_tile_reach(C.byref(cam), *[float(v) for v in bounds], len(r), c.ctypes.data,
                                        r.ctypes.data, keep.ctypes.data, tlow.ctypes.data, C.byref(ok))
    rtw._abi.check(rc, "rtw_debug_tile_reach")
    assert set(np.unique(keep)) <= {0, 1} and ok.value in (0, 1)
    return keep.astype(bool), tlow, bool(ok.value)
