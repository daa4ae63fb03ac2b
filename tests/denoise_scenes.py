"""Scenes, inputs and references shared by tests/test_denoise.py (host backend) and tests/test_gpu_denoise.py (GPU):
the first-hit guide buffers (rtw_render_guides) and the a-trous filter (rtw_denoise).

Not a test module.  Host references are computed once per process and returned read-only."""
import ctypes as C
import functools

import numpy as np

CPU = -1
GW, GH = 40, 24           # the GPU tests' frame: partial 32 x 8 blocks in x, three block rows
H5 = np.array([1 / 16, 1 / 4, 3 / 8, 1 / 4, 1 / 16], np.float64)
FLOOR = 2.0 ** -8


def pkg():
    import importlib
    return importlib.import_module("zig-raytracing-weekend_amd")


# ---------------------------------------------------------------- scenes of the guide tests
def small(cam, width=GW, height=GH):
    """The scene's camera at the GPU tests' frame, pixel_offset 1."""
    cam.image_width, cam.image_height, cam.pixel_offset = width, height, 1
    cam.aspect_ratio = width / height
    return cam.init()


SCENES = ("book1", "earth_perlin", "cornell", "cornell_smoke", "simple_light", "cornell_mesh")


def scene(rtw, name):
    """(SceneArrays, tuning or None, initialised camera) of a guide-test scene."""
    W = rtw.worlds
    if name == "book1":
        return rtw.flatten(W.generate_world(0, "book1")), None, small(rtw.book1_camera(spp=1))
    if name == "book1_orders8":
        return rtw.flatten(W.generate_world(0, "book1")), {"bvh_orders": 8}, small(rtw.book1_camera(spp=1))
    if name == "book1_hoist0":
        return rtw.flatten(W.generate_world(0, "book1")), {"hoist": 0}, small(rtw.book1_camera(spp=1))
    if name == "earth_perlin":
        return rtw.flatten(W.earth_perlin_world(0)), None, small(rtw.earth_perlin_camera(spp=1))
    if name == "cornell":
        return rtw.flatten(W.cornell_box()), None, small(rtw.cornell_camera(spp=1))
    if name == "cornell_smoke":
        return rtw.flatten(W.cornell_smoke()), None, small(rtw.cornell_smoke_camera(spp=1))
    if name == "cornell_smoke_no_media":
        objs = [o for o in W.cornell_smoke() if not isinstance(o, rtw.ConstantMedium)]
        return rtw.flatten(objs), None, small(rtw.cornell_smoke_camera(spp=1))
    if name == "simple_light":
        return rtw.flatten(W.simple_light_world(0), lights="emissive+spheres"), None, small(rtw.simple_light_camera(spp=1))
    if name == "cornell_mesh":
        return rtw.flatten(W.cornell_mesh(smooth=True)), None, small(rtw.cornell_camera(spp=1))
    if name == "cornell_mesh_flat":
        return rtw.flatten(W.cornell_mesh(smooth=False)), None, small(rtw.cornell_camera(spp=1))
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def host_guides(name):
    """(albedo, normal_depth) of a scene on the host backend, read-only."""
    rtw = pkg()
    arr, tuning, cam = scene(rtw, name)
    w = rtw.World(arr, device=CPU, tuning=tuning)
    a, n = w.render_guides(cam)
    w.close()
    a.setflags(write=False)
    n.setflags(write=False)
    return a, n


def centre_dirs(cam):
    """The ray direction through every pixel centre in float64, (H * W, 3), and the camera centre."""
    d = cam.derived
    c = np.array(d.center[:], np.float64)
    p00, du, dv = (np.array(v[:], np.float64) for v in (d.pixel00_loc, d.pixel_delta_u, d.pixel_delta_v))
    ys, xs = np.mgrid[0:d.image_height, 0:d.image_width]
    pc = p00 + (xs[..., None] + d.pixel_offset) * du + (ys[..., None] + d.pixel_offset) * dv
    return (pc - c).reshape(-1, 3), c


# ---------------------------------------------------------------- inputs of the filter tests
def random_inputs(W, H, seed=0, bad=True):
    """A seeded frame for the filter: (accum, albedo, normal_depth) as float32 (W * H, 4).

    Means in [0, 4) over w in 1 .. 8; albedo in [0.25, 1) (within a factor 4 of each other: demodulation then
    inflates a neighbour's rounding error by at most that); unit normals within ~0.3 of one of two directions (left
    and right half) and depths 5 .. 6, so that every pixel has taps of non-negligible weight at the sigmas the tests
    use; the top-right corner block misses (normal_depth = 0, albedo.w = 0).  bad: one NaN pixel and one pixel with
    w = 0, both away from the border and the miss block where the frame allows it."""
    rng = np.random.default_rng(seed)
    n = W * H
    w = rng.integers(1, 9, n).astype(np.float32)
    mean = (rng.random((n, 3)) * 4).astype(np.float32)
    accum = np.concatenate([mean * w[:, None], w[:, None]], 1).astype(np.float32)
    albedo = np.concatenate([0.25 + 0.75 * rng.random((n, 3)), np.ones((n, 1))], 1).astype(np.float32)
    xs = np.tile(np.arange(W), H)
    ys = np.repeat(np.arange(H), W)
    base = np.where((xs < W // 2)[:, None], np.array([0.0, 0.0, -1.0]), np.array([0.6, 0.0, -0.8]))
    nrm = base + 0.15 * rng.normal(size=(n, 3))
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    depth = 5.0 + rng.random(n)
    nd = np.concatenate([nrm, depth[:, None]], 1).astype(np.float32)
    miss = (xs >= W - max(1, W // 4)) & (ys < max(1, H // 3)) if W * H > 1 else np.zeros(n, bool)
    nd[miss] = 0
    albedo[miss, 3] = 0
    if bad and n >= 12:
        accum[nan_pixel(W, H), 1] = np.nan
        accum[zero_w_pixel(W, H)] = (1.0, 2.0, 3.0, 0.0)
    return accum, albedo, nd


def nan_pixel(W, H):
    return (H // 2) * W + W // 4


def zero_w_pixel(W, H):
    return (2 * H // 3) * W + W // 2 + 1


def largest_mean(accum):
    with np.errstate(divide="ignore", invalid="ignore"):
        m = accum[:, :3].astype(np.float64) / accum[:, 3:4].astype(np.float64)
    return float(np.max(m[np.isfinite(m).all(1)]))


def reference_filter(accum, albedo, nd, W, H, passes, demodulate, sigma_color, sigma_normal, sigma_depth):
    """The header's arithmetic restated in float64: returns the accumulator-form result (H * W, 4)."""
    a = accum.astype(np.float64).reshape(H, W, 4)
    g = nd.astype(np.float64).reshape(H, W, 4)
    w = a[..., 3]
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        c = a[..., :3] * (1.0 / w)[..., None]
        if demodulate:
            al = np.maximum(albedo.astype(np.float64).reshape(H, W, 4)[..., :3], FLOOR)
            c = c / al
        hit = g[..., 3] > 0
        kn = 1.0 / sigma_normal ** 2 if sigma_normal > 0 else 0.0
        kz = np.where(hit, 1.0 / (sigma_depth ** 2 * g[..., 3] ** 2), 0.0) if sigma_depth > 0 else np.zeros((H, W))
        ys, xs = np.mgrid[0:H, 0:W]
        for i in range(passes):
            s = 1 << i
            sc = sigma_color * 2.0 ** -i
            fin_p = np.isfinite(c).all(-1)
            kc = np.where(fin_p, 1.0 / sc ** 2, 0.0) if sigma_color > 0 else np.zeros((H, W))
            cp = np.where(fin_p[..., None], c, 0.0)
            acc = np.zeros((H, W, 3))
            wsum = np.zeros((H, W))
            for dy in range(-2, 3):
                for dx in range(-2, 3):
                    qy, qx = ys + s * dy, xs + s * dx
                    inside = (qy >= 0) & (qy < H) & (qx >= 0) & (qx < W)
                    qy, qx = np.clip(qy, 0, H - 1), np.clip(qx, 0, W - 1)
                    cq, gq = c[qy, qx], g[qy, qx]
                    ok = inside & np.isfinite(cq).all(-1) & ((gq[..., 3] > 0) == hit)
                    cq = np.where(ok[..., None], cq, 0.0)
                    x = (((cq - cp) ** 2).sum(-1) * kc + ((gq[..., :3] - g[..., :3]) ** 2).sum(-1) * kn) + \
                        (gq[..., 3] - g[..., 3]) ** 2 * kz
                    e = np.where(x <= 87.0, np.exp(-np.minimum(x, 87.0)), 0.0)
                    wgt = np.where(ok, H5[dx + 2] * H5[dy + 2] * e, 0.0)
                    acc += wgt[..., None] * cq
                    wsum += wgt
            c = np.where((wsum > 0)[..., None], acc / np.where(wsum > 0, wsum, 1.0)[..., None], c)
        if demodulate:
            c = c * al
        out = np.concatenate([c * w[..., None], w[..., None]], -1)
    return out.reshape(-1, 4)


def denoise(rtw, world, accum, albedo, nd, W, H, **params):
    return world.denoise(accum, (albedo, nd), W, H, **params)


@functools.lru_cache(maxsize=None)
def host_world():
    """A host context to filter on (the filter reads no scene): two spheres."""
    rtw = pkg()
    return rtw.World(rtw.flatten(rtw.worlds.two_spheres_world()), device=CPU)


def render(rtw, world, cam, spp, seed):
    buf = np.zeros((cam.size, 4), np.float32)
    rc = rtw.lib().rtw_render(world.handle, C.byref(cam.derived), 0, cam.size, 0, spp, seed, buf.ctypes.data, None,
                              rtw._abi.PROGRESS_FN(0), None)
    rtw._abi.check(rc, "rtw_render")
    return buf
