"""Denoised previews on the host backend (no GPU): the first-hit guide buffers (rtw_render_guides) against known
answers, rtw_expneg against float64 exp, the a-trous filter (rtw_denoise) against a float64 restatement of the
header's arithmetic and its properties, and the quality of the shipped defaults on an 8-spp Cornell box."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import denoise_scenes as D
from conftest import REPO

CPU = D.CPU


def one_sphere(rtw, mat, width=33, height=17, **cam_kw):
    """A unit sphere at the origin seen from (0, 0, 5), gradient sky; pixel_offset 0 and odd sizes put the centre
    pixel's ray on the axis."""
    arr = rtw.flatten([rtw.Sphere.init([0, 0, 0], 1.0, mat)])
    kw = dict(aspect_ratio=width / height, image_width=width, image_height=height, samples_per_pixel=1, max_depth=5,
              background_mode=rtw._abi.RTW_BG_GRADIENT, vfov=40.0, lookfrom=(0.0, 0.0, 5.0), lookat=(0.0, 0.0, 0.0),
              defocus_angle=0.0, pixel_offset=0)
    kw.update(cam_kw)
    cam = rtw.Camera(**kw).init()
    w = rtw.World(arr, device=CPU)
    a, n = w.render_guides(cam)
    w.close()
    return cam, a, n


# ---------------------------------------------------------------- guides: known answers
def test_sphere_centre_and_sky_corner(rtw):
    cam, a, n = one_sphere(rtw, rtw.Lambertian.fromColor([0.3, 0.6, 0.9]))
    W, H = 33, 17
    c = (H // 2) * W + W // 2
    assert np.allclose(n[c, :3], [0, 0, 1], atol=2e-6)                    # the unit vector towards the camera
    assert abs(n[c, 3] - 4.0) <= 8 * np.spacing(np.float32(4.0))          # distance - radius, a few ulp
    assert np.array_equal(a[c], np.array([0.3, 0.6, 0.9, 1.0], np.float32))
    dirs, _ = D.centre_dirs(cam)
    for corner in (0, W - 1, (H - 1) * W, H * W - 1):
        assert np.array_equal(n[corner], np.zeros(4, np.float32)) and a[corner, 3] == 0
        t = 0.5 * (dirs[corner, 1] / np.linalg.norm(dirs[corner]) + 1.0)
        assert np.allclose(a[corner, :3], (1 - t) * np.ones(3) + t * np.array([0.5, 0.7, 1.0]), atol=1e-6)
    hit = n[:, 3] > 0
    assert hit.any() and (~hit).any() and np.array_equal(hit, a[:, 3] == 1)
    assert np.allclose(np.linalg.norm(n[hit, :3], axis=1), 1, atol=1e-5)
    assert ((n[hit, :3] * dirs[hit]).sum(1) < 0).all()


def test_pixel_offset_is_applied_as_a_render_applies_it(rtw):
    """pixel_offset 1 (camera.zig:100-101): pixel (x, y) looks through the centre of grid cell (x + 1, y + 1), so the
    axis ray belongs to the pixel one up and one left of the frame's centre, the whole frame equals the offset-0
    frame shifted by one pixel, and the sky corners follow the gradient of the shifted directions."""
    mat = rtw.Lambertian.fromColor([0.3, 0.6, 0.9])
    W, H = 33, 17
    _, a0, n0 = one_sphere(rtw, mat)
    cam, a1, n1 = one_sphere(rtw, mat, pixel_offset=1)
    assert cam.derived.pixel_offset == 1
    c = (H // 2 - 1) * W + W // 2 - 1
    assert np.allclose(n1[c, :3], [0, 0, 1], atol=2e-6) and abs(n1[c, 3] - 4.0) <= 8 * np.spacing(np.float32(4.0))
    assert not np.allclose(n1[(H // 2) * W + W // 2, :3], [0, 0, 1], atol=1e-3)
    img0, img1 = n0.reshape(H, W, 4), n1.reshape(H, W, 4)
    assert np.array_equal(img1[:-1, :-1], img0[1:, 1:])
    assert np.array_equal(a1.reshape(H, W, 4)[:-1, :-1], a0.reshape(H, W, 4)[1:, 1:])
    d = cam.derived
    p00, du, dv, centre = (np.array(v[:], np.float64) for v in (d.pixel00_loc, d.pixel_delta_u, d.pixel_delta_v, d.center))
    for x, y in ((0, 0), (W - 1, 0), (0, H - 1), (W - 1, H - 1)):
        v = p00 + (x + 1) * du + (y + 1) * dv - centre
        t = 0.5 * (v[1] / np.linalg.norm(v) + 1.0)
        p = y * W + x
        assert a1[p, 3] == 0 and np.array_equal(n1[p], np.zeros(4, np.float32))
        assert np.allclose(a1[p, :3], (1 - t) * np.ones(3) + t * np.array([0.5, 0.7, 1.0]), atol=1e-6)
        # an offset of 0 or 2 would miss by far more than the tolerance
        v_off = p00 + x * du + y * dv - centre
        t_off = 0.5 * (v_off[1] / np.linalg.norm(v_off) + 1.0)
        assert abs(t - t_off) * 0.3 > 1e-4


def test_no_jitter_no_defocus_no_seed(rtw):
    """The guides ignore the camera's defocus disk and its strata, and two calls give the same bits."""
    mat = rtw.Lambertian.fromColor([0.3, 0.6, 0.9])
    _, a0, n0 = one_sphere(rtw, mat)
    _, a1, n1 = one_sphere(rtw, mat, defocus_angle=2.0, focus_dist=5.0, strata=4)
    _, a2, n2 = one_sphere(rtw, mat)
    assert np.array_equal(a0, a1) and np.array_equal(n0, n1)
    assert np.array_equal(a0, a2) and np.array_equal(n0, n2)


def test_albedo_by_material(rtw):
    """Metal gives its albedo, Dielectric 1, DiffuseLight its emit value (one sphere each, the centre pixel)."""
    c = (17 // 2) * 33 + 33 // 2
    _, a, _ = one_sphere(rtw, rtw.Metal.fromColor([0.7, 0.6, 0.5], 0.1))
    assert np.array_equal(a[c], np.array([0.7, 0.6, 0.5, 1], np.float32))
    _, a, _ = one_sphere(rtw, rtw.Dielectric.init(1.5))
    assert np.array_equal(a[c], np.array([1, 1, 1, 1], np.float32))
    _, a, _ = one_sphere(rtw, rtw.DiffuseLight.fromColor([4, 5, 6]))
    assert np.array_equal(a[c], np.array([4, 5, 6, 1], np.float32))


def pixel_towards(cam, point):
    dirs, c = D.centre_dirs(cam)
    v = np.asarray(point, np.float64) - c
    cos = dirs @ v / np.linalg.norm(dirs, axis=1) / np.linalg.norm(v)
    return int(np.argmax(cos))


def test_light_pixels_of_cornell_and_simple_light(rtw):
    """The pixel looking at the Cornell ceiling light sees its emit value (15), the wall pixels their colours; the
    pixels looking at simple_light's quad and sphere lights see 4."""
    _, _, cam = D.scene(rtw, "cornell")
    a, n = D.host_guides("cornell")
    p = pixel_towards(cam, (278.0, 554.0, 279.5))
    assert np.array_equal(a[p], np.array([15, 15, 15, 1], np.float32))
    assert np.allclose(n[p, :3], [0, -1, 0], atol=1e-6)                    # the light faces down, towards the ray
    row = D.GH // 2 * D.GW
    hit = n[row:row + D.GW, 3] > 0
    cols = np.nonzero(hit)[0]
    left, right = a[row + cols[0]], a[row + cols[-1]]                      # the image's left is the green wall (x = 555)
    assert np.allclose(left[:3], [0.12, 0.45, 0.15]) and np.allclose(right[:3], [0.65, 0.05, 0.05])
    _, _, cam = D.scene(rtw, "simple_light")
    a, n = D.host_guides("simple_light")
    for light in ((4.0, 2.0, -2.0), (0.0, 7.0, 0.0)):
        p = pixel_towards(cam, light)
        assert np.array_equal(a[p], np.array([4, 4, 4, 1], np.float32)), light


def test_media_are_transparent(rtw):
    """cornell_smoke's guides equal, bit for bit, those of the same object list without the two media: a medium leaf
    gives a guide ray no hit, and the closest hit does not depend on the tree's topology."""
    a1, n1 = D.host_guides("cornell_smoke")
    a2, n2 = D.host_guides("cornell_smoke_no_media")
    assert np.array_equal(a1, a2) and np.array_equal(n1, n2)
    assert (n1[:, 3] > 0).sum() > 400
    # and nothing of the smoke's boundary boxes shows: every hit is a wall or the light
    colours = {tuple(round(float(x), 2) for x in c) for c in a1[n1[:, 3] > 0, :3]}
    assert colours <= {(0.73, 0.73, 0.73), (0.65, 0.05, 0.05), (0.12, 0.45, 0.15), (7.0, 7.0, 7.0)}, colours


def test_topology_independent_on_book1(rtw):
    a, n = D.host_guides("book1")
    for other in ("book1_orders8", "book1_hoist0"):
        a2, n2 = D.host_guides(other)
        assert np.array_equal(a, a2) and np.array_equal(n, n2), other


def test_smooth_mesh_normals(rtw):
    """cornell_mesh(smooth=True): the shading normal where attributes are registered -- it differs from the flat
    mesh's on the icosphere, nowhere else, and stays on the ray's side."""
    _, _, cam = D.scene(rtw, "cornell_mesh")
    a, n = D.host_guides("cornell_mesh")
    af, nf = D.host_guides("cornell_mesh_flat")
    assert np.array_equal(a, af) and np.array_equal(n[:, 3], nf[:, 3])     # same hits, same depths
    diff = (n[:, :3] != nf[:, :3]).any(1)
    assert 10 <= diff.sum() < (n[:, 3] > 0).sum()
    dirs, _ = D.centre_dirs(cam)
    hit = n[:, 3] > 0
    assert ((n[hit, :3] * dirs[hit]).sum(1) < 0).all()
    assert np.allclose(np.linalg.norm(n[hit, :3], axis=1), 1, atol=1e-5)


# ---------------------------------------------------------------- rtw_expneg
def test_expneg_against_float64(rtw):
    x = np.linspace(0.0, 87.0, 1_000_000).astype(np.float32)
    out = np.empty_like(x)
    rtw._abi.check(rtw.lib().rtw_debug_expneg(len(x), x.ctypes.data, out.ctypes.data), "rtw_debug_expneg")
    ref = np.exp(-x.astype(np.float64))
    rel = np.abs(out.astype(np.float64) - ref) / ref
    print(f"rtw_expneg: max relative error {rel.max():.3e} = 2^{np.log2(rel.max()):.2f} at x = {x[rel.argmax()]}")
    assert rel.max() <= 2.0 ** -20
    edge = np.array([0.0, 87.0, np.nextafter(np.float32(87), np.float32(100)), 88.0, 1e30, np.inf], np.float32)
    got = np.empty_like(edge)
    rtw._abi.check(rtw.lib().rtw_debug_expneg(len(edge), edge.ctypes.data, got.ctypes.data), "rtw_debug_expneg")
    assert got[0] == 1.0 and got[1] > 0 and (got[2:] == 0).all()


# ---------------------------------------------------------------- the filter against float64
SIGMAS = [(1.0, 0.5, 0.2), (0.0, 0.5, 0.2), (1.0, 0.0, 0.2), (1.0, 0.5, 0.0)]


@pytest.mark.parametrize("demodulate", [False, True])
@pytest.mark.parametrize("W,H,passes", [(32, 24, 5), (33, 17, 8)])
def test_filter_against_float64(rtw, W, H, passes, demodulate):
    """Tolerance passes x 4e-6 x M (M: the largest finite input mean): per pass twice the exp error bound
    (2 x 2^-20) plus about 30 ulp for a 25-term fp32 weighted mean.  Measured worst case over these cases:
    4.9e-7 x M (DESIGN.md §Denoised previews)."""
    acc, alb, nd = D.random_inputs(W, H)
    M = D.largest_mean(acc)
    tol = passes * 4e-6 * M
    wgt = acc[:, 3:4].astype(np.float64)
    ok = wgt[:, 0] > 0
    world = D.host_world()
    for sig in SIGMAS:
        got = D.denoise(rtw, world, acc, alb, nd, W, H, passes=passes, demodulate=demodulate, sigma_color=sig[0],
                        sigma_normal=sig[1], sigma_depth=sig[2])
        ref = D.reference_filter(acc, alb, nd, W, H, passes, demodulate, *sig)
        err = np.abs(got[ok, :3] / wgt[ok] - ref[ok, :3] / wgt[ok]).max()
        print(f"{W} x {H}, {passes} passes, demodulate {demodulate}, sigmas {sig}: {err / M:.2e} x M (bound {tol / M:.1e})")
        assert np.isfinite(got).all()
        assert err <= tol, (sig, err, tol)
        assert np.array_equal(got[:, 3], acc[:, 3])
        assert np.isfinite(got[D.nan_pixel(W, H)]).all()                   # the NaN pixel is filled from its neighbours
        assert np.array_equal(got[D.zero_w_pixel(W, H)], np.zeros(4, np.float32))


# ---------------------------------------------------------------- filter properties
def two_regions(W=32, H=24):
    """Left half: normal -z, colour 1 +- noise; right half: normal +x, colour 3 +- noise.  One depth, w = 4."""
    rng = np.random.default_rng(5)
    n = W * H
    left = np.tile(np.arange(W) < W // 2, H)
    mean = np.where(left[:, None], 1.0, 3.0) + 0.2 * (rng.random((n, 3)) - 0.5)
    acc = np.concatenate([mean * 4, np.full((n, 1), 4.0)], 1).astype(np.float32)
    nd = np.zeros((n, 4), np.float32)
    nd[left, :3], nd[~left, :3] = (0, 0, -1), (1, 0, 0)
    nd[:, 3] = 5.0
    return acc, nd, left


def test_nothing_leaks_across_a_normal_edge(rtw):
    """|dn|^2 = 2 across the edge, sigma_normal 0.1: the weight there is e(200) = 0, so each region is filtered on
    its own and five passes with the colour term off bring it to a near-constant -- its own, far from the other's."""
    W, H = 32, 24
    acc, nd, left = two_regions(W, H)
    out = D.denoise(rtw, D.host_world(), acc, None, nd, W, H, passes=5, demodulate=False, sigma_color=0.0,
                    sigma_normal=0.1, sigma_depth=0.0)
    m = out[:, :3] / 4
    for region, centre in ((left, 1.0), (~left, 3.0)):
        assert np.abs(m[region] - centre).max() < 0.06, centre            # noise of +-0.1 averaged over >= 100 taps
        assert m[region].max() - m[region].min() < 0.06
    # the region means are kept: what a leak would move
    before = acc[:, :3] / 4
    assert abs(m[left].mean() - before[left].mean()) < 0.01 and abs(m[~left].mean() - before[~left].mean()) < 0.01


def test_hit_and_miss_never_mix(rtw):
    """Every sigma 0: all weights are the kernel's, yet a miss pixel averages misses only."""
    W, H = 32, 24
    acc, nd, left = two_regions(W, H)
    acc[left, :3], acc[~left, :3] = 4.0, 12.0                              # means 1 and 3, exactly
    nd[left] = 0                                                           # the left half misses
    out = D.denoise(rtw, D.host_world(), acc, None, nd, W, H, passes=5, demodulate=False, sigma_color=0.0,
                    sigma_normal=0.0, sigma_depth=0.0)
    tol = 5 * 4e-6 * 3.0
    assert np.abs(out[left, :3] / 4 - 1.0).max() <= tol and np.abs(out[~left, :3] / 4 - 3.0).max() <= tol


def test_in_place_and_w_kept(rtw):
    W, H = 33, 17
    acc, alb, nd = D.random_inputs(W, H)
    world = D.host_world()
    sep = D.denoise(rtw, world, acc, alb, nd, W, H)
    buf = acc.copy()
    same = world.denoise(buf, (alb, nd), W, H, out=buf)
    assert same is buf and np.array_equal(buf, sep, equal_nan=True)
    assert np.array_equal(sep[:, 3], acc[:, 3])
    for wrong in (np.zeros((W * H, 3), np.float32), np.zeros((W * H, 4), np.float64), np.zeros((W * H, 8), np.float32)[:, ::2]):
        with pytest.raises(ValueError):
            world.denoise(acc, (alb, nd), W, H, out=wrong)
    # without demodulation the albedo may be absent
    a = D.denoise(rtw, world, acc, None, nd, W, H, demodulate=False)
    b = D.denoise(rtw, world, acc, alb, nd, W, H, demodulate=False)
    assert np.array_equal(a, b)


def test_defaults_cite_the_search(rtw):
    A = rtw._abi
    p = A.denoise_params()
    assert C.sizeof(A.RtwDenoiseParams) == 32
    rep = json.load(open(os.path.join(REPO, "profiles", "denoise", "defaults.json")))
    w = rep["winner"]
    assert (p.passes, bool(p.flags & A.RTW_DENOISE_DEMODULATE)) == (w["passes"], w["demodulate"])
    assert (p.sigma_color, p.sigma_normal, p.sigma_depth) == tuple(
        np.float32(w[k]) for k in ("sigma_color", "sigma_normal", "sigma_depth"))
    assert 1 <= p.passes <= A.RTW_DENOISE_MAX_PASSES and p.flags & ~A.RTW_DENOISE_DEMODULATE == 0


def test_refusals_leave_out_untouched(rtw):
    A = rtw._abi
    L = rtw.lib()
    W, H = 8, 6
    acc, alb, nd = D.random_inputs(W, H, bad=False)
    world = D.host_world()
    out = np.full((W * H, 4), 7.0, np.float32)

    def call(p, w=W, h=H, accum=acc, albedo=alb, guide=nd, o=out, handle=None):
        return L.rtw_denoise(world.handle if handle is None else handle, w, h, A.ptr(accum), A.ptr(albedo),
                             A.ptr(guide), C.byref(p) if p is not None else None, A.ptr(o))
    good = A.denoise_params(passes=2)
    bad = [dict(passes=0), dict(passes=9), dict(sigma_color=-1.0), dict(sigma_normal=float("nan")),
           dict(sigma_depth=float("inf")), dict(sigma_depth=-0.5), dict(flags=2), dict(flags=1 | 4)]
    for kw in bad:
        assert call(A.denoise_params(**kw)) == A.RTW_E_INVALID, kw
        assert L.rtw_last_error()
    assert call(good, w=0) == A.RTW_E_INVALID and call(good, h=0) == A.RTW_E_INVALID
    assert call(good, accum=None) == A.RTW_E_INVALID and call(good, guide=None) == A.RTW_E_INVALID
    assert call(None) == A.RTW_E_INVALID and call(good, handle=C.c_void_p()) == A.RTW_E_INVALID
    assert call(A.denoise_params(passes=2, demodulate=True), albedo=None) == A.RTW_E_INVALID
    assert L.rtw_denoise(world.handle, W, H, A.ptr(acc), A.ptr(alb), A.ptr(nd), C.byref(good), None) == A.RTW_E_INVALID
    # the device entry points refuse a host context
    assert L.rtw_denoise_device(world.handle, W, H, A.ptr(acc), A.ptr(alb), A.ptr(nd), C.byref(good), A.ptr(out), None,
                                0) == A.RTW_E_INVALID
    cam = rtw.Camera(image_width=W, image_height=H, aspect_ratio=W / H).init()
    assert L.rtw_render_guides_device(world.handle, C.byref(cam.derived), A.ptr(out), A.ptr(out), None,
                                      0) == A.RTW_E_INVALID
    assert L.rtw_render_guides(world.handle, C.byref(cam.derived), None, A.ptr(out)) == A.RTW_E_INVALID
    assert L.rtw_render_guides(world.handle, None, A.ptr(out), A.ptr(out)) == A.RTW_E_INVALID
    assert (out == 7.0).all()
    assert call(good) == A.RTW_OK and not (out == 7.0).all()
    assert call(A.denoise_params(passes=2, demodulate=False), albedo=None) == A.RTW_OK


# ---------------------------------------------------------------- Python layer and quality
def test_state_denoised_and_quality(rtw):
    """Cornell 48 x 48 on the host backend: the 8-spp image denoised with the shipped defaults is closer (RMSE of
    the mean radiance) to a 2048-spp render than the 8-spp image itself.  RayTraceState.denoised returns a new
    buffer in the accumulator's form and leaves the state's accumulator alone."""
    arr = rtw.flatten(rtw.worlds.cornell_box())
    cam = rtw.cornell_camera(image_width=48, spp=8).init()
    world = rtw.World(arr, device=CPU)
    target = D.render(rtw, world, cam, 2048, 1000)
    state = rtw.RayTraceState(cam, rtw.SharedStateImageWriter(48, 48), world, seed=7)
    cam.render_range(state, 0, cam.size, 0, 8)
    noisy = state.writer.buffer.copy()
    out = state.denoised()
    world.close()
    assert out is not state.writer.buffer and np.array_equal(state.writer.buffer, noisy)
    assert out.shape == (cam.size, 4) and np.array_equal(out[:, 3], noisy[:, 3]) and np.isfinite(out).all()

    def rmse(a):
        return np.sqrt(np.mean((a[:, :3].astype(np.float64) / a[:, 3:4] - target[:, :3].astype(np.float64) / 2048) ** 2))
    print(f"RMSE 8 spp {rmse(noisy):.4f}, denoised {rmse(out):.4f}, ratio {rmse(out) / rmse(noisy):.3f}")
    assert rmse(out) < rmse(noisy)
    # the texel update takes the result as it takes the accumulator
    tex = np.zeros((cam.size, 4), np.uint8)
    rtw._abi.check(rtw.lib().rtw_texture_from_accum(out.ctypes.data, cam.size, tex.ctypes.data), "rtw_texture_from_accum")
    assert (tex[:, 3] == 255).all() and tex[:, :3].max() > 0
