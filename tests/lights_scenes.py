"""Scenes, cameras and renders shared by tests/test_lights.py (host backend) and tests/test_gpu_lights.py (GPU):
light importance sampling (rtw_scene_set_lights).

Not a test module.  The analytic scene: a Lambertian floor (albedo 0.5) in y = 0 under a 1 x 1 light of radiance 4
at height 2, black background, max_depth 2 -- a floor pixel is albedo / pi * Le * the light's form-factor integral
at its hit point, which the tests compute by quadrature.  The camera looks down at the point under the light from
(0, 4, -8) through a narrow lens: seen from there either light covers floor only beyond 5 units of that point, and a
pixel's footprint on the floor is about 0.07 x 0.15 units."""
import ctypes as C
import functools

import numpy as np

CPU = -1
ALBEDO = 0.5
FLOOR_HALF = 40.0
# (q, u, v, radiance): the light of the analytic scene, and the second light of the two-light scene
LIGHT1 = ((-0.5, 2.0, -0.5), (1.0, 0.0, 0.0), (0.0, 0.0, 1.0), 4.0)
LIGHT2 = ((1.0, 1.5, 0.5), (0.5, 0.0, 0.0), (0.0, 0.0, 1.5), 9.0)
CAM_KW = dict(aspect_ratio=1.0, vfov=20.0, lookfrom=(0.0, 4.0, -8.0), lookat=(0.0, 0.0, 0.0), vup=(0.0, 1.0, 0.0),
              defocus_angle=0.0, background=(0.0, 0.0, 0.0))
W = 48


def pkg():
    import importlib
    return importlib.import_module("zig-raytracing-weekend_amd")


def analytic_objects(rtw, two=False):
    floor = rtw.Quad.init([-FLOOR_HALF, 0, -FLOOR_HALF], [2 * FLOOR_HALF, 0, 0], [0, 0, 2 * FLOOR_HALF],
                          rtw.Lambertian.fromColor([ALBEDO] * 3))
    objs = [floor]
    for q, u, v, le in (LIGHT1, LIGHT2)[:2 if two else 1]:
        objs.append(rtw.Quad.init(q, u, v, rtw.DiffuseLight.fromColor([le] * 3)))
    return objs


def analytic_arrays(rtw, two=False, lights=True):
    return rtw.flatten(analytic_objects(rtw, two), lights="emissive" if lights else None)


def analytic_camera(rtw, spp, depth=2):
    return rtw.Camera(image_width=W, samples_per_pixel=spp, max_depth=depth, **CAM_KW).init()


def floor_hits(cam):
    """Where each pixel's centre ray meets the floor (y = 0): (x, z) per pixel in float64, NaN where it does not."""
    d = cam.derived
    off = d.pixel_offset
    c = np.array(d.center[:], np.float64)
    p00, du, dv = (np.array(v[:], np.float64) for v in (d.pixel00_loc, d.pixel_delta_u, d.pixel_delta_v))
    ys, xs = np.mgrid[0:d.image_height, 0:d.image_width]
    pc = p00 + (xs[..., None] + off) * du + (ys[..., None] + off) * dv
    dirs = (pc - c).reshape(-1, 3)
    with np.errstate(divide="ignore", invalid="ignore"):
        t = np.where(dirs[:, 1] < 0, -c[1] / dirs[:, 1], np.nan)
    hit = c + t[:, None] * dirs
    return hit[:, [0, 2]]


def form_factor(points_xz, light, order=24):
    """integral over the light of cos(theta) cos(theta') / r^2 dA for floor points (x, 0, z), normal +y, by
    Gauss-Legendre quadrature in float64."""
    q, u, v, _ = (np.array(a, np.float64) for a in light)
    g, wg = np.polynomial.legendre.leggauss(order)
    g, wg = 0.5 * (g + 1), 0.5 * wg
    n = np.cross(u, v)
    area = np.linalg.norm(n)
    n = n / area
    p = np.stack([points_xz[:, 0], np.zeros(len(points_xz)), points_xz[:, 1]], axis=1)
    out = np.zeros(len(p))
    for a, wa in zip(g, wg):
        for b, wb in zip(g, wg):
            y = q + a * u + b * v
            w = y - p
            r2 = (w * w).sum(1)
            r = np.sqrt(r2)
            cos_s = np.maximum(0.0, w[:, 1] / r)
            cos_l = np.abs(w @ n) / r
            out += wa * wb * area * cos_s * cos_l / r2
    return out


def expected_floor(cam, two=False):
    """(selected pixel indices, expected radiance there): pixels whose centre ray meets the floor within 3 units of
    the point below the first light."""
    xz = floor_hits(cam)
    sel = np.nonzero(np.hypot(xz[:, 0], xz[:, 1]) <= 3.0)[0]
    e = np.zeros(len(sel))
    for light in (LIGHT1, LIGHT2)[:2 if two else 1]:
        e += ALBEDO / np.pi * light[3] * form_factor(xz[sel], light)
    return sel, e


def render(rtw, arr, cam, spp, seed, device=CPU, tuning=None, s0=0, world=None):
    """Samples [s0, spp) of the whole frame as a fresh float4 accumulator."""
    w = world if world is not None else rtw.World(arr, device=device, tuning=tuning)
    buf = np.zeros((cam.size, 4), np.float32)
    rc = rtw.lib().rtw_render(w.handle, C.byref(cam.derived), 0, cam.size, s0, spp, seed, buf.ctypes.data, None,
                              rtw._abi.PROGRESS_FN(0), None)
    rtw._abi.check(rc, "rtw_render")
    if world is None:
        w.close()
    return buf


SEEDS = tuple(range(100, 116))
SPP = 256


@functools.lru_cache(maxsize=None)
def analytic_seed_images(two, lights):
    """16 seeds x 256 spp of the analytic scene on the host backend: (16, pixels) mean radiance (the scene is
    grey: channel 0).  Rendered once per process, read-only."""
    rtw = pkg()
    arr = analytic_arrays(rtw, two, lights)
    cam = analytic_camera(rtw, SPP)
    world = rtw.World(arr, device=CPU)
    out = np.stack([render(rtw, arr, cam, SPP, s, world=world)[:, 0] / SPP for s in SEEDS]).astype(np.float64)
    world.close()
    out.setflags(write=False)
    return out


def cornell(rtw, name, lights, mode=None):
    objs = rtw.worlds.cornell_box() if name == "cornell" else rtw.worlds.cornell_smoke()
    return rtw.flatten(objs, bvh_mode=mode, lights="emissive" if lights else None)
