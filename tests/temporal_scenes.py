"""Scenes, cameras and references shared by tests/test_temporal.py (host backend) and tests/test_gpu_temporal.py
(GPU): the temporal reprojection (rtw_temporal_accumulate, include/rtw_gpu.h "Temporal reprojection").  The
projection step restated in numpy float64, the scenes of the tests and a float64 restatement of a whole call for
single-tap (snapped) frames.

Not a test module.  Nothing here reads the library's results."""
import ctypes as C
import dataclasses
import functools
import math

import numpy as np

import denoise_scenes as D

CPU = -1
F = np.float32


def pkg():
    return D.pkg()


# ---------------------------------------------------------------- cameras
def with_(cam, **kw):
    """A fresh, initialised copy of a Camera with fields replaced."""
    return dataclasses.replace(cam, derived=None, strata=cam.strata, **kw).init()


def projection_cameras(rtw):
    """The projection test's five: Book-1's and Cornell's at their own size and 4096 wide, one with pixel_offset 0."""
    return [("book1", rtw.book1_camera(spp=1).init()), ("book1_4096", rtw.book1_camera(image_width=4096, spp=1).init()),
            ("cornell", rtw.cornell_camera(spp=1).init()), ("cornell_4096", rtw.cornell_camera(image_width=4096, spp=1).init()),
            ("book1_off0", with_(rtw.book1_camera(image_width=400, spp=1), pixel_offset=0))]


def fields64(d):
    """(centre, pixel00, du, dv, offset) of an RtwCamera: its float32 fields as float64."""
    v = [np.array(x[:], np.float64) for x in (d.center, d.pixel00_loc, d.pixel_delta_u, d.pixel_delta_v)]
    return v[0], v[1], v[2], v[3], float(d.pixel_offset)


def centre_points(cam, max_rows=64):
    """The pixel centres of a camera as float32 points and unit directions, with their (x, y): every column of at
    most max_rows evenly spaced rows (the first and the last included)."""
    d = cam.derived
    c, p00, du, dv, off = fields64(d)
    H, W = d.image_height, d.image_width
    rows = np.unique(np.linspace(0, H - 1, min(H, max_rows)).round().astype(np.int64))
    ys, xs = np.meshgrid(rows, np.arange(W), indexing="ij")
    xs, ys = xs.ravel(), ys.ravel()
    pts = p00 + (xs[:, None] + off) * du + (ys[:, None] + off) * dv
    dirs = pts - c
    dirs /= np.linalg.norm(dirs, axis=1, keepdims=True)
    return np.ascontiguousarray(pts, F), np.ascontiguousarray(dirs, F), xs, ys


def project64(d, e):
    """The header's projection step in float64: e (N, 3) = point - centre, or a direction -> (fx, fy, ok)."""
    c, p00, du, dv, off = fields64(d)
    n = np.cross(du, dv)
    a = p00 - c
    with np.errstate(all="ignore"):
        lam = (n @ a) / (e @ n)
        r = e * lam[:, None] - a
        fx = (r @ du) / (du @ du) - off
        fy = (r @ dv) / (dv @ dv) - off
    ok = (lam > 0) & np.isfinite(lam)
    return fx, fy, ok


def reproject(rtw, cam, points=None, dirs=None):
    """rtw_debug_reproject: (xy (N, 2), ok (N,) bool)."""
    src = points if points is not None else dirs
    src = np.ascontiguousarray(src, F)
    n = len(src)
    xy, ok = np.zeros((n, 2), F), np.zeros(n, np.uint8)
    rc = rtw.lib().rtw_debug_reproject(C.byref(cam.derived), n, src.ctypes.data if points is not None else None,
                                       src.ctypes.data if points is None else None, xy.ctypes.data, ok.ctypes.data)
    rtw._abi.check(rc, "rtw_debug_reproject")
    return xy, ok.astype(bool)


def first_hits64(cam, nd):
    """The world-space first-hit point of every pixel from the guides, float64 (H * W, 3); rows of misses are the
    unit directions.  Also (unit directions, hit mask)."""
    dirs, c = D.centre_dirs(cam)
    u = dirs / np.linalg.norm(dirs, axis=1, keepdims=True)
    hit = nd[:, 3] > 0
    return np.where(hit[:, None], c + u * nd[:, 3:4].astype(np.float64), u), u, hit


# ---------------------------------------------------------------- scenes
def frame_camera(rtw, lookfrom, lookat, W=64, H=48, vfov=40.0, focus_dist=1.0, sky=False, background=(0, 0, 0)):
    return rtw.Camera(aspect_ratio=W / H, image_width=W, image_height=H, samples_per_pixel=1, max_depth=8,
                      background=background,
                      background_mode=rtw._abi.RTW_BG_GRADIENT if sky else rtw._abi.RTW_BG_CONSTANT, vfov=vfov,
                      lookfrom=tuple(lookfrom), lookat=tuple(lookat), vup=(0.0, 1.0, 0.0), defocus_angle=0.0,
                      focus_dist=focus_dist).init()


def shift_scene(rtw):
    """A checker-textured DiffuseLight quad in the plane z = -1 that fills the view of a camera at the origin looking
    down -z with focus distance 1, and the same camera translated along u by exactly 3 pixels of its own
    (3 pixel_delta_u: the quad lies in the focus plane, so the image moves by 3 columns)."""
    S = rtw.scene
    tex = S.CheckerTexture.init(0.11, S.SolidColor.init((4.0, 1.0, 0.25)), S.SolidColor.init((0.25, 1.0, 4.0)))
    quad = S.Quad.init((-8.0, -8.0, -1.0), (16.0, 0.0, 0.0), (0.0, 16.0, 0.0), S.DiffuseLight.init(tex))
    prev = frame_camera(rtw, (0.0, 0.0, 0.0), (0.0, 0.0, -1.0))
    step = 3.0 * np.array(prev.derived.pixel_delta_u[:], np.float64)
    cur = frame_camera(rtw, step, step + np.array([0.0, 0.0, -1.0]))
    return rtw.flatten([quad]), prev, cur


def disocclusion_scene(rtw):
    """A sphere of radius 0.3 at z = -3 in front of a wall in z = -5, both Lambertian, under a constant sky; the
    camera at the origin and translated sideways by 0.3."""
    S = rtw.scene
    wall = S.Quad.init((-20.0, -20.0, -5.0), (40.0, 0.0, 0.0), (0.0, 40.0, 0.0), S.Lambertian.fromColor((0.7, 0.6, 0.5)))
    ball = S.Sphere.init((0.0, 0.0, -3.0), 0.3, S.Lambertian.fromColor((0.2, 0.4, 0.8)))
    kw = dict(background=(0.8, 0.9, 1.0), focus_dist=3.0)
    prev = frame_camera(rtw, (0.0, 0.0, 0.0), (0.0, 0.0, -3.0), **kw)
    cur = frame_camera(rtw, (0.3, 0.0, 0.0), (0.3, 0.0, -3.0), **kw)
    return rtw.flatten([wall, ball]), prev, cur


def sky_scene(rtw):
    """Two spheres (a ground and a ball) under the gradient sky; the camera panned by 5 degrees about its centre."""
    S = rtw.scene
    objs = [S.Sphere.init((0.0, -100.5, -3.0), 100.0, S.Lambertian.fromColor((0.5, 0.6, 0.3))),
            S.Sphere.init((0.0, 0.0, -3.0), 0.5, S.Lambertian.fromColor((0.7, 0.3, 0.3)))]
    a = math.radians(5.0)
    prev = frame_camera(rtw, (0.0, 0.0, 0.0), (0.0, 0.0, -3.0), sky=True, focus_dist=3.0)
    cur = frame_camera(rtw, (0.0, 0.0, 0.0), (3.0 * math.sin(a), 0.0, -3.0 * math.cos(a)), sky=True, focus_dist=3.0)
    return rtw.flatten(objs), prev, cur


def orbit(rtw, frames, W, step_deg=1.0):
    """Cornell's camera at W x W and `frames` - 1 further ones, each turned by step_deg about the box's centre."""
    base = rtw.cornell_camera(image_width=W, spp=1, max_depth=20)
    centre = np.array([278.0, 278.0, 278.0])
    r = np.array(base.lookfrom) - centre
    cams = []
    for k in range(frames):
        a = math.radians(step_deg * k)
        rot = np.array([r[0] * math.cos(a) + r[2] * math.sin(a), r[1], -r[0] * math.sin(a) + r[2] * math.cos(a)])
        cams.append(with_(base, lookfrom=tuple(float(x) for x in centre + rot), lookat=tuple(centre)))
    return cams


@functools.lru_cache(maxsize=None)
def host_world(name):
    """A host context of a named scene with its two cameras: (world, prev_cam, cur_cam); "cornell": cameras None."""
    rtw = pkg()
    if name == "cornell":
        return rtw.World(rtw.flatten(rtw.worlds.cornell_box()), device=CPU), None, None
    arr, prev, cur = {"shift": shift_scene, "disocclusion": disocclusion_scene, "sky": sky_scene}[name](rtw)
    return rtw.World(arr, device=CPU), prev, cur


def render(world, cam, spp, seed):
    return D.render(pkg(), world, cam, spp, seed)


def rmse(acc, ref):
    """Root mean square error of the mean radiance of two accumulator-form frames (pixels with w > 0 in both)."""
    with np.errstate(all="ignore"):
        a = acc[:, :3].astype(np.float64) / acc[:, 3:4]
        b = ref[:, :3].astype(np.float64) / ref[:, 3:4]
    ok = np.isfinite(a).all(1) & np.isfinite(b).all(1)
    return float(np.sqrt(np.mean((a[ok] - b[ok]) ** 2)))


# ---------------------------------------------------------------- synthetic frames (no scene is read)
def synthetic_frames(rtw, W, H, kind, seed=0):
    """(cur_cam, prev_cam, cur_accum, cur_nd, prev_accum, prev_nd, prev_moments) for a frame W x H whose guides are
    those of a wall in z = -4 facing the cameras with a nearer strip (z = -3) across its middle rows and a band of
    misses in its top rows -- written from the geometry in float64, so no scene is traced -- and seeded accumulators
    and moments, with a NaN pixel, a w = 0 pixel and an n = 0 pixel in the history where the frame holds them.
    kind: "still" (the same camera), "translated" (0.21 sideways, 0.05 up) or "panned" (2 degrees)."""
    prev = frame_camera(rtw, (0.0, 0.0, 0.0), (0.0, 0.0, -3.0), W=W, H=H, focus_dist=3.0)
    if kind == "still":
        cur = frame_camera(rtw, (0.0, 0.0, 0.0), (0.0, 0.0, -3.0), W=W, H=H, focus_dist=3.0)
    elif kind == "translated":
        cur = frame_camera(rtw, (0.21, 0.05, 0.0), (0.21, 0.05, -3.0), W=W, H=H, focus_dist=3.0)
    else:
        a = math.radians(2.0)
        cur = frame_camera(rtw, (0.0, 0.0, 0.0), (3.0 * math.sin(a), 0.0, -3.0 * math.cos(a)), W=W, H=H, focus_dist=3.0)
    rng = np.random.default_rng(seed + 17 * W + H)

    def guides(cam):
        dirs, c = D.centre_dirs(cam)
        u = dirs / np.linalg.norm(dirs, axis=1, keepdims=True)
        ys = np.repeat(np.arange(H), W)
        z = np.where((ys >= H // 3) & (ys < H // 3 + max(1, H // 4)), -3.0, -4.0)
        t = (z - c[2]) / u[:, 2]
        nd = np.concatenate([np.tile([0.0, 0.0, 1.0], (W * H, 1)), t[:, None]], 1)
        nd[ys < H // 8] = 0
        return nd.astype(F)

    def accum():
        w = rng.integers(1, 9, W * H).astype(F)
        return np.concatenate([(rng.random((W * H, 3)) * 4).astype(F) * w[:, None], w[:, None]], 1).astype(F)
    cur_acc, prev_acc = accum(), accum()
    n = W * H
    mom = np.zeros((2, n, 4), F)
    mom[0] = prev_acc
    cnt = rng.integers(1, 6, n).astype(F)
    mom[1] = np.stack([rng.random(n).astype(F), (rng.random(n) * cnt).astype(F), cnt, prev_acc[:, 3]], 1)
    if n >= 12:
        prev_acc[D.nan_pixel(W, H), 1] = np.nan
        prev_acc[D.zero_w_pixel(W, H)] = (1.0, 2.0, 3.0, 0.0)
        mom[1, (n // 2 + 3) % n] = 0
        cur_acc[(n // 3) % n, 0] = np.inf
        cur_acc[(n // 5) % n] = (0.5, 0.5, 0.5, 0.0)
    return cur, prev, cur_acc, guides(cur), prev_acc, guides(prev), mom
