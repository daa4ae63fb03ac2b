"""Environment maps (rtw_scene_set_environment: image-based lighting, importance-sampled as one more light of the
mixture density) on the host backend (RTW_DEVICE_CPU, the GPU's per-sample code compiled for the host): validation,
the getter, clearing and the scene hash; the lookup, the density and the sampler through rtw_debug_environment;
analytic renders under a constant map and a sky with a small sun; the variance sampling buys; schedule invariance;
the guides; the Radiance reader.  Every seed is fixed: every figure below is deterministic."""
import ctypes as C

import numpy as np
import pytest

import environment_scenes as E
import lights_scenes as S

CPU = E.CPU


def set_env_rc(rtw, world, rgb, width=None, height=None, scale=(1, 1, 1), rotate_y=0.0, flags=1):
    A = rtw._abi
    r = A.RtwEnvironment()
    a = None if rgb is None else np.ascontiguousarray(rgb, np.float32)
    r.rgb = None if a is None else a.ctypes.data
    r.width = (a.shape[1] if a is not None else 4) if width is None else width
    r.height = (a.shape[0] if a is not None else 2) if height is None else height
    r.scale[:] = [float(np.float32(x)) for x in scale]
    r.rotate_y = rotate_y
    r.flags = flags
    return rtw.lib().rtw_scene_set_environment(world.handle, C.byref(r))


def floor_world(rtw, env=None):
    return rtw.World(rtw.flatten(S.analytic_objects(rtw)[:1], environment=env), device=CPU)


# ---------------------------------------------------------------- 1. validation, get, clear, hash
def test_validation_get_clear_hash(rtw):
    A = rtw._abi
    base = E.random_map(6, 3, 1)
    never = floor_world(rtw)
    h_never = E.scene_hash(rtw, never)
    assert never.environment() is None
    world = floor_world(rtw)
    given = rtw.Environment(base, scale=(0.5, 2.0, 1.5), rotate_y=30.0, sample=True)
    world.set_environment(given)
    h_set = E.scene_hash(rtw, world)

    def unchanged(what):
        got = world.environment()
        assert got is not None and np.array_equal(got.rgb, base), what
        assert got.scale == (0.5, 2.0, 1.5) and got.rotate_y == 30.0 and got.sample is True, what
        assert E.scene_hash(rtw, world) == h_set, what

    unchanged("after the set")
    nan, inf = float("nan"), float("inf")

    def with_texel(v):
        m = base.copy()
        m[1, 2, 1] = v
        return m

    bad = {"a null rgb": dict(rgb=None), "a zero width": dict(rgb=base, width=0), "a zero height": dict(rgb=base, height=0),
           "a width over the maximum": dict(rgb=base, width=A.RTW_ENV_MAX_WIDTH + 1),
           "a height over the maximum": dict(rgb=base, height=A.RTW_ENV_MAX_HEIGHT + 1),
           "a negative texel": dict(rgb=with_texel(-1.0)), "a NaN texel": dict(rgb=with_texel(nan)),
           "an infinite texel": dict(rgb=with_texel(inf)), "a negative scale": dict(rgb=base, scale=(1, -1, 1)),
           "a NaN scale": dict(rgb=base, scale=(nan, 1, 1)), "an infinite scale": dict(rgb=base, scale=(1, 1, inf)),
           "a NaN rotation": dict(rgb=base, rotate_y=nan), "an infinite rotation": dict(rgb=base, rotate_y=inf),
           "unknown flag bits": dict(rgb=base, flags=3)}
    for what, kw in bad.items():
        assert set_env_rc(rtw, world, **kw) == A.RTW_E_INVALID, what
        assert b"rtw_scene_set_environment" in rtw.lib().rtw_last_error(), what
        unchanged(what)
    # the hash covers the map, the scale, the rotation and the flag
    hashes = {"set": h_set, "never": h_never}
    variants = {"map": rtw.Environment(with_texel(7.0), (0.5, 2.0, 1.5), 30.0, True),
                "scale": rtw.Environment(base, (0.5, 2.0, 1.25), 30.0, True),
                "rotation": rtw.Environment(base, (0.5, 2.0, 1.5), 31.0, True),
                "flag": rtw.Environment(base, (0.5, 2.0, 1.5), 30.0, False)}
    for name, env in variants.items():
        world.set_environment(env)
        hashes[name] = E.scene_hash(rtw, world)
    assert len(set(hashes.values())) == len(hashes), hashes
    world.set_environment(given)
    assert E.scene_hash(rtw, world) == h_set
    world.set_environment(None)
    assert world.environment() is None
    assert E.scene_hash(rtw, world) == h_never
    assert rtw.lib().rtw_debug_environment(world.handle, 0, None, None, None, None, None, None) == A.RTW_E_INVALID
    world.close()
    never.close()


def test_flatten_carries_the_environment(rtw):
    env = rtw.Environment(E.random_map(5, 4, 2), rotate_y=-12.5, sample=False)
    arr = rtw.flatten(S.analytic_objects(rtw)[:1], environment=env)
    assert arr.environment is env
    world = rtw.World(arr, device=CPU)
    got = world.environment()
    assert np.array_equal(got.rgb, env.rgb) and got.rotate_y == -12.5 and got.sample is False
    world.close()


# ---------------------------------------------------------------- 2. lookup
@pytest.mark.parametrize("shape", [(1, 1), (2, 1), (37, 19), (64, 32)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_lookup_at_texel_centres(rtw, shape):
    """Directions built in float64 at the texel centres look up their texel, and its radiance is exactly
    fp32(scale) * texel."""
    w, h = shape
    m = E.random_map(w, h, 3)
    scale = np.array([0.5, 2.0, 1.3], np.float32)
    world = floor_world(rtw, rtw.Environment(m, scale=scale))
    out = world.debug_environment(dirs=E.centre_dirs(rtw, w, h))
    assert np.array_equal(out["texel"], np.arange(w * h))
    assert np.array_equal(out["radiance"], (m * scale).reshape(-1, 3))
    assert np.isfinite(out["pdf"]).all()
    # the poles: the top and the bottom row, finite
    poles = world.debug_environment(dirs=[[0, 1, 0], [0, -1, 0]])
    assert poles["texel"][0] < w and poles["texel"][1] >= (h - 1) * w
    assert np.isfinite(poles["radiance"]).all() and np.isfinite(poles["pdf"]).all()
    world.close()


def test_lookup_rotated(rtw):
    w, h = 64, 32
    m = E.random_map(w, h, 4)
    world = floor_world(rtw, rtw.Environment(m, rotate_y=90.0))
    # the world directions of the turned map's texel centres find their texels ...
    out = world.debug_environment(dirs=E.centre_dirs(rtw, w, h, 90.0))
    assert np.array_equal(out["texel"], np.arange(w * h))
    # ... and the unturned centres land a quarter of the width away, in their own rows
    plain = world.debug_environment(dirs=E.centre_dirs(rtw, w, h))["texel"]
    idx = np.arange(w * h)
    assert np.array_equal(plain // w, idx // w)
    shift = (plain % w - idx % w) % w
    assert (shift == shift[0]).all() and shift[0] in (w // 4, w - w // 4), shift[0]
    world.close()


# ---------------------------------------------------------------- 3. density
def lit_texel_map():
    m = np.zeros((8, 16, 3), np.float32)
    m[2, 5] = (3.0, 100.0, 0.5)
    return m


DENSITY_MAPS = {"37x19": lambda: E.random_map(37, 19, 5), "64x32": lambda: E.random_map(64, 32, 6),
                "black_rows": lambda: E.random_map(32, 16, 7, black_rows=(0, 5, 6, 15)), "one_texel": lit_texel_map}


@pytest.mark.parametrize("name", sorted(DENSITY_MAPS))
def test_density_integrates_to_one(rtw, name):
    """sum_ij pdf(centre_ij) sin(theta_ij) 2 pi^2 / (W H) = 1 within 1e-4 (at most 2048 fp32 terms of relative
    error about 1e-6 each); 0 exactly on texels of no weight, finite everywhere."""
    m = DENSITY_MAPS[name]()
    h, w = m.shape[:2]
    scale = np.array([1.0, 0.5, 2.0], np.float32)
    world = floor_world(rtw, rtw.Environment(m, scale=scale))
    pdf = world.debug_environment(dirs=E.centre_dirs(rtw, w, h))["pdf"].astype(np.float64).reshape(h, w)
    world.close()
    assert np.isfinite(pdf).all() and (pdf >= 0).all()
    sin_t = np.sin(np.pi * (np.arange(h) + 0.5) / h)[:, None]
    total = (pdf * sin_t).sum() * 2 * np.pi ** 2 / (w * h)
    print(f"{name}: integral of the density = {total:.7f}")
    assert abs(total - 1.0) <= 1e-4
    dark = (m * scale).sum(axis=2) == 0
    assert (pdf[dark] == 0).all() and (pdf[~dark] > 0).all()


def test_unsampled_and_black_maps_have_no_density(rtw):
    dirs = E.centre_dirs(rtw, 8, 4)
    for env in (rtw.Environment(E.random_map(8, 4, 8), sample=False), rtw.Environment(np.zeros((4, 8, 3), np.float32))):
        world = floor_world(rtw, env)
        assert (world.debug_environment(dirs=dirs)["pdf"] == 0).all()
        world.close()


# ---------------------------------------------------------------- 4. sampling
def grid_map():
    """16 x 8, grey texels of small integer radiance, every row's sum 64 (so the conditional distributions' cell
    edges are multiples of 1 / 64, exact in fp32 and half a grid step from every draw), zero texels in every row
    and one black row."""
    g = np.random.default_rng(9)
    m = np.zeros((8, 16), np.float64)
    for j in range(8):
        if j == 3:
            continue
        cells = g.permutation(16)[:10]
        v = np.ones(10)
        for _ in range(54):
            v[g.integers(10)] += 1
        m[j, cells] = v
    assert (m.sum(1)[[0, 1, 2, 4, 5, 6, 7]] == 64).all()
    return np.repeat(m[..., None], 3, axis=2).astype(np.float32)


def test_sampling_grid(rtw):
    """A K x K regular grid of draws (a, b), K = 256, on grid_map(): every sampled direction looks up a texel of
    positive weight with a positive density, the draw counts follow the masses within the grid's own granularity
    (2 K: one line of draws at each edge of a cell's interval), and the direction looks up the texel the draws
    chose.  No draw lies within 1e-3 of a cell of the cell's edge: a's grid (k + 1/2) / K sits half a step from the
    multiples of 1 / 64, and b's offset is the first of a fixed list that keeps that distance from the marginal
    distribution's edges (computed here in float64)."""
    K = 256
    m = grid_map()
    h, w = m.shape[:2]
    wgt = m[..., 0].astype(np.float64) * np.sin(np.pi * (np.arange(h) + 0.5) / h)[:, None]
    row_mass = wgt.sum(1) / wgt.sum()
    marg = np.cumsum(row_mass)
    marg[-1] = 1.0
    cond = np.cumsum(m[..., 0].astype(np.float64), axis=1) / 64.0
    edges = np.concatenate([[0.0], marg])
    for off in (0.5, 0.25, 0.75, 0.125, 0.375, 0.625, 0.875):
        b = (np.arange(K) + off) / K
        rows = np.searchsorted(marg, b, side="right")
        lo, hi = edges[rows], edges[rows + 1]
        if (np.minimum(b - lo, hi - b) >= 1e-3 * (hi - lo)).all():
            break
    else:
        raise AssertionError("no offset keeps the b grid off the marginal edges")
    a = (np.arange(K) + 0.5) / K
    aa, bb = np.meshgrid(a, b)              # bb varies along axis 0
    draws = np.stack([aa.ravel(), bb.ravel()], axis=1).astype(np.float32)
    assert np.array_equal(draws[:, 0].astype(np.float64), aa.ravel())   # the grids are exact in fp32
    rows = np.repeat(np.searchsorted(marg, b.astype(np.float32).astype(np.float64), side="right"), K)
    cols = np.array([np.searchsorted(cond[r], a, side="right") for r in rows[::K]]).ravel()
    world = floor_world(rtw, rtw.Environment(m))
    sampled = world.debug_environment(draws=draws)["sampled_dir"]
    assert np.isfinite(sampled).all() and np.allclose(np.linalg.norm(sampled.astype(np.float64), axis=1), 1, atol=1e-5)
    back = world.debug_environment(dirs=sampled)
    world.close()
    tex = back["texel"].astype(np.int64)
    assert (wgt.ravel()[tex] > 0).all() and (back["pdf"] > 0).all()
    assert np.array_equal(tex, rows * w + cols)
    row_count = np.bincount(tex // w, minlength=h)
    assert (np.abs(row_count - K * K * row_mass) <= 2 * K).all(), (row_count, K * K * row_mass)
    tex_mass = (wgt / wgt.sum()).ravel()
    tex_count = np.bincount(tex, minlength=w * h)
    worst = np.abs(tex_count - K * K * tex_mass).max()
    print(f"sampling grid: worst texel count error {worst:.1f} of an allowance of {2 * K}")
    assert worst <= 2 * K
    assert (tex_count[tex_mass == 0] == 0).all()


# ---------------------------------------------------------------- 5. analytic renders
def pixel_ratio(img, expected):
    mean, se = img.mean(0), img.std(0, ddof=1) / np.sqrt(img.shape[0])
    return np.abs(mean - expected) / (5 * se + 0.005 * expected), se


@pytest.mark.parametrize("sample", [True, False], ids=["sample", "no_sample"])
def test_analytic_constant_map(rtw, sample):
    """A constant map of radiance 1 over the floor: albedo * Le at every selected pixel, seed-mean of 16 x 256 spp
    within 5 se + 0.5 %.  Measured: worst |mean - expected| / bound = 0.793 (sample), 0.080 (no_sample)."""
    cam = S.analytic_camera(rtw, S.SPP)
    sel, expected = E.expected(rtw, cam, "constant")
    assert len(sel) > 1000 and np.allclose(expected, S.ALBEDO, rtol=1e-3)
    z, se = pixel_ratio(E.seed_images("constant", sample)[:, sel], expected)
    print(f"constant map sample={sample}: {len(sel)} pixels, worst |mean - expected| / bound = {z.max():.3f}")
    assert (z <= 1).all(), (int(sel[z.argmax()]), z.max())


def test_analytic_sun_sampled(rtw):
    """sky_sun with a 2-degree sun of radiance 5000 over a dim sky, sample on: albedo / pi * sum L cos(theta) dOmega
    (float64, 8 x 8 sub-samples per texel) at every selected pixel within 5 se + 0.5 %.  Measured: worst
    |mean - expected| / bound = 0.687 (expected 1.4456, mean se / expected 0.016)."""
    cam = S.analytic_camera(rtw, S.SPP)
    sel, expected = E.expected(rtw, cam, "sun")
    z, se = pixel_ratio(E.seed_images("sun", True)[:, sel], expected)
    print(f"sun sample=True: expected {expected[0]:.4f}, worst |mean - expected| / bound = {z.max():.3f}, "
          f"mean se / expected = {(se / expected).mean():.4f}")
    assert (z <= 1).all(), (int(sel[z.argmax()]), z.max())


def test_analytic_sun_unsampled(rtw):
    """The same scene with sample off.  A pixel's 16 x 256 samples meet the sun's texels under 4 times on average
    (a sample's chance is their cosine-weighted share of the hemisphere, about 9e-4) and 2.5 % of the pixels never do:
    a handful of hits of radiance up to 5000 is no Gaussian mean and a pixel's standard error over the seeds
    estimates nothing -- measured per pixel, 3.8 % of the 1908 pixels lie over 5 se + 0.5 %, the worst at 170 times
    it, exactly the pixels with no hit.  So the bound is applied where it means something: to the mean over the
    selected pixels, which all expect the same value (about 7000 hits), with se the standard error of that mean
    over the 16 seeds.  Measured: mean 1.4227 for 1.4456, se 0.0211,
    |mean - expected| / bound = 0.203."""
    cam = S.analytic_camera(rtw, S.SPP)
    sel, expected = E.expected(rtw, cam, "sun")
    assert np.ptp(expected) == 0
    per_seed = E.seed_images("sun", False)[:, sel].mean(1)
    mean, se = per_seed.mean(), per_seed.std(ddof=1) / np.sqrt(len(per_seed))
    z = abs(mean - expected[0]) / (5 * se + 0.005 * expected[0])
    print(f"sun sample=False: pooled mean {mean:.4f}, expected {expected[0]:.4f}, se {se:.4f}, "
          f"|mean - expected| / bound = {z:.3f}")
    assert z <= 1


def test_analytic_sun_and_quad_light(rtw):
    """The sun map and the registered quad LIGHT1: the hemisphere sum, minus the part of the sky the quad hides,
    plus the quad's own form factor -- a wrong 1 / (n + 1) or a wrong pick of k shows here.  Measured: worst
    |mean - expected| / bound = 0.767 (seeds 200..215: environment_scenes.SEEDS says why)."""
    cam = S.analytic_camera(rtw, S.SPP)
    sel, expected = E.expected(rtw, cam, "sun_light")
    z, se = pixel_ratio(E.seed_images("sun_light", True)[:, sel], expected)
    print(f"sun + LIGHT1: worst |mean - expected| / bound = {z.max():.3f}, mean se / expected = "
          f"{(se / expected).mean():.4f}")
    assert (z <= 1).all(), (int(sel[z.argmax()]), z.max())


# ---------------------------------------------------------------- 6. variance
def test_variance_reduction(rtw):
    """Summed across-seed variance on the sun scene, sample on over sample off, equal spp: <= 3 F / (1 - F), F the
    cosine-weighted fraction of the hemisphere's energy outside the sun's support (computed from the map here).
    Brute force leaves the variance of meeting the sun or not, which belongs to the share 1 - F of the energy; a
    sampler that follows the map removes that part and leaves what the map's density does not follow -- the cosine
    over the share F --, so the ratio is at most of order F / (1 - F); 3 x margin as test_lights.py takes.
    Measured: F = 0.0518, bound 0.164, ratio 0.00090."""
    cam = S.analytic_camera(rtw, S.SPP)
    sel, _ = E.expected(rtw, cam, "sun")
    f = E.sun_support_fraction(rtw, E.analytic_map("sun"))
    assert 0 < f < 0.5
    bound = 3 * f / (1 - f)
    on = E.seed_images("sun", True)[:, sel].var(0, ddof=1).sum()
    off = E.seed_images("sun", False)[:, sel].var(0, ddof=1).sum()
    print(f"variance: F = {f:.4f}, bound {bound:.4f}, ratio on / off = {on / off:.5f}")
    assert on / off <= bound


# ---------------------------------------------------------------- 7. schedule invariance, off is off
def schedule_scene(rtw, strata=0):
    arr = rtw.flatten(rtw.worlds.cornell_mesh(smooth=True), lights="emissive", environment=E.small_env(rtw))
    cam = rtw.cornell_camera(image_width=40, spp=6, max_depth=50)
    cam.strata = strata
    return arr, cam.init()


def render_into(rtw, world, cam, buf, s0, s1, seed=21):
    rc = rtw.lib().rtw_render(world.handle, C.byref(cam.derived), 0, cam.size, s0, s1, seed, buf.ctypes.data, None,
                              rtw._abi.PROGRESS_FN(0), None)
    rtw._abi.check(rc, "rtw_render")


@pytest.mark.parametrize("strata", [0, 2])
def test_schedule_invariance(rtw, strata):
    arr, cam = schedule_scene(rtw, strata)
    world = rtw.World(arr, device=CPU)
    one = np.zeros((cam.size, 4), np.float32)
    render_into(rtw, world, cam, one, 0, 6)
    two = np.zeros((cam.size, 4), np.float32)
    render_into(rtw, world, cam, two, 0, 3)
    render_into(rtw, world, cam, two, 3, 6)
    assert np.array_equal(one, two)
    for threads in (1, 4):
        assert np.array_equal(E.render(rtw, arr, cam, tuning={"cpu_threads": threads}), one), threads
    # row shards reassemble the frame
    d = rtw.distributed
    H, W = cam.derived.image_height, cam.derived.image_width
    img = np.zeros((H, W, 4), np.float32)
    for s in range(2):
        tr = d.shard_tile_rows(H, 8, 2, s)
        tile = np.zeros((tr * W, 4), np.float32)
        rtw._abi.check(rtw.lib().rtw_render_rows(world.handle, C.byref(cam.derived), 8, 2, s, 0, 6, 21,
                                                 tile.ctypes.data, None), "rtw_render_rows")
        for r in range(tr):
            y = d.shard_row(H, 8, 2, s, r)
            if y < H:
                img[y] = tile.reshape(-1, W, 4)[r]
    assert np.array_equal(img.reshape(-1, 4), one)
    world.close()
    if strata:
        plain_arr, plain_cam = schedule_scene(rtw, 0)
        assert not np.array_equal(E.render(rtw, plain_arr, plain_cam), one)


def test_off_is_off(rtw):
    arr, cam = schedule_scene(rtw)
    arr.environment = None
    never = E.render(rtw, arr, cam)
    world = rtw.World(arr, device=CPU)
    world.set_environment(E.small_env(rtw))
    on = E.render(rtw, arr, cam, world=world)
    world.set_environment(E.small_env(rtw, sample=False))
    unsampled = E.render(rtw, arr, cam, world=world)
    world.set_environment(None)
    cleared = E.render(rtw, arr, cam, world=world)
    world.close()
    assert np.array_equal(cleared, never)
    assert not np.array_equal(on, never) and not np.array_equal(unsampled, never) and not np.array_equal(on, unsampled)


def test_sphere_scene_renders_with_an_environment(rtw):
    """A scene of spheres alone takes an environment: every miss carries the map's radiance (no pixel of the sky
    is the camera's background), and it is the same image at 1 and 4 threads."""
    env = E.small_env(rtw)
    arr, cam = E.parity_scene(rtw, "book1", env)
    got = E.render(rtw, arr, cam, tuning={"cpu_threads": 4})
    assert np.array_equal(got, E.render(rtw, arr, cam, tuning={"cpu_threads": 1}))
    arr.environment = None
    assert not np.array_equal(got, E.render(rtw, arr, cam))
    assert np.isfinite(got).all()


# ---------------------------------------------------------------- 8. guides
def test_guides_report_the_environment(rtw):
    env = E.small_env(rtw, rotate_y=25.0)
    arr, cam = E.parity_scene(rtw, "book1", env)
    world = rtw.World(arr, device=CPU)
    albedo, nd = world.render_guides(cam)
    miss = albedo[:, 3] == 0
    assert 50 < miss.sum() < cam.size
    # the pixel-centre ray as guide_pixel builds it, in fp32: (pixel00 + du i) + dv j - center
    d = cam.derived
    f = np.float32
    p00, du, dv, c = (np.array(v[:], f) for v in (d.pixel00_loc, d.pixel_delta_u, d.pixel_delta_v, d.center))
    ys, xs = np.divmod(np.arange(cam.size), d.image_width)
    i, j = (xs + d.pixel_offset).astype(f)[:, None], (ys + d.pixel_offset).astype(f)[:, None]
    dirs = ((p00 + du * i) + dv * j) - c
    assert dirs.dtype == np.float32
    rad = world.debug_environment(dirs=dirs[miss])["radiance"]
    world.close()
    assert np.array_equal(albedo[miss, :3], rad)
    assert (nd[miss] == 0).all()


# ---------------------------------------------------------------- 9. load_hdr
def to_rgbe(rgb):
    """Radiance's float -> RGBE (truncating mantissas), uint8 (h, w, 4)."""
    v = rgb.max(axis=2).astype(np.float64)
    m, e = np.frexp(v)
    out = np.zeros(rgb.shape[:2] + (4,), np.uint8)
    ok = v >= 1e-32
    k = np.where(ok, m * 256.0 / np.where(ok, v, 1.0), 0.0)
    out[..., :3] = np.floor(rgb.astype(np.float64) * k[..., None]).astype(np.uint8)
    out[..., 3] = np.where(ok, e + 128, 0).astype(np.uint8)
    return out


def rle_scanline(px):
    """A new-style run-length-encoded scanline of uint8 (w, 4) pixels."""
    w = len(px)
    out = bytearray([2, 2, w >> 8, w & 255])
    for c in range(4):
        ch, x = px[:, c], 0
        while x < w:
            run = 1
            while x + run < w and run < 127 and ch[x + run] == ch[x]:
                run += 1
            if run >= 3:
                out += bytes([128 + run, int(ch[x])])
                x += run
                continue
            lit = x
            while lit < w and lit - x < 128 and not (lit + 2 < w and ch[lit] == ch[lit + 1] == ch[lit + 2]):
                lit += 1
            out += bytes([lit - x]) + bytes(int(b) for b in ch[x:lit])
            x = lit
    return bytes(out)


@pytest.mark.parametrize("encoding", ["flat", "rle"])
def test_load_hdr_round_trip(rtw, tmp_path, encoding):
    m = E.random_map(16, 5, 11)
    m[1, 3:12] = (2.5, 0.25, 8.0)      # runs in every channel
    m[4] = 0                            # a black row: e = 0
    q = to_rgbe(m)
    header = b"#?RADIANCE\n# written by the test\nFORMAT=32-bit_rle_rgbe\n\n-Y 5 +X 16\n"
    body = q.tobytes() if encoding == "flat" else b"".join(rle_scanline(row) for row in q)
    path = tmp_path / f"{encoding}.hdr"
    path.write_bytes(header + body)
    env = rtw.Environment.load_hdr(str(path), rotate_y=10.0)
    assert env.rgb.shape == (5, 16, 3) and env.rotate_y == 10.0
    # exactly the quantised values ...
    expect = q[..., :3].astype(np.float64) * np.where(q[..., 3:] > 0, 2.0 ** (q[..., 3:].astype(np.float64) - 136), 0.0)
    assert np.array_equal(env.rgb.astype(np.float64), expect)
    # ... which differ from the floats by the quantisation alone: below one step of the shared exponent
    step = np.where(q[..., 3:] > 0, 2.0 ** (q[..., 3:].astype(np.float64) - 136), 1e-32)
    assert (np.abs(expect - m) <= step).all()
    with pytest.raises(ValueError):
        bad = tmp_path / "bad.hdr"
        bad.write_bytes(header.replace(b"-Y 5 +X 16", b"+Y 5 +X 16") + body)
        rtw.Environment.load_hdr(str(bad))
