"""Light importance sampling (rtw_scene_set_lights: the mixture density of "The Rest of Your Life") on the host
backend (RTW_DEVICE_CPU, the GPU's per-sample code compiled for the host): validation, clearing, the scene hash,
the analytic form factor of a quad light over a Lambertian floor, the variance it buys, agreement with the oracle
(which knows nothing of lights: the estimator is unbiased, only its variance changes) and schedule invariance.
Every seed is fixed: every figure below is deterministic."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import lights_scenes as S

CPU = S.CPU


def set_lights_rc(rtw, world, recs):
    a = np.array(recs, rtw._abi.OBJECT_DT).reshape(-1)
    return rtw.lib().rtw_scene_set_lights(world.handle, rtw._abi.ptr(a), len(a))


def scene_hash(rtw, world):
    h = C.c_uint64()
    rtw._abi.check(rtw.lib().rtw_scene_hash(world.handle, C.byref(h)), "rtw_scene_hash")
    return h.value


def test_validation_and_get(rtw):
    A = rtw._abi
    arr = rtw.flatten(rtw.worlds.cornell_box())
    # cornell_box(): quads 0..5 are the walls (2: the light), then the boxes' sides, members of two instances
    assert arr.materials[arr.quads[2]["material"]]["kind"] == A.RTW_MAT_DIFFUSE_LIGHT
    member = tuple(int(x) for x in arr.members[0])
    assert member[0] == A.RTW_OBJ_QUAD
    world = rtw.World(arr, device=CPU)
    assert len(world.lights()) == 0
    assert set_lights_rc(rtw, world, [(A.RTW_OBJ_QUAD, 2)]) == A.RTW_OK
    bad = {"a sphere": [(A.RTW_OBJ_SPHERE, 0)], "an instance": [(A.RTW_OBJ_INSTANCE, 0)],
           "an instance member": [member], "a non-emissive quad": [(A.RTW_OBJ_QUAD, 0)],
           "an index out of range": [(A.RTW_OBJ_QUAD, len(arr.quads))], "the same quad twice": [(A.RTW_OBJ_QUAD, 2)] * 2,
           "17 lights": [(A.RTW_OBJ_QUAD, 2)] * 17}
    for what, recs in bad.items():
        assert set_lights_rc(rtw, world, recs) == A.RTW_E_INVALID, what
        assert b"rtw_scene_set_lights" in rtw.lib().rtw_last_error(), what
        assert world.lights().tolist() == [(A.RTW_OBJ_QUAD, 2)], what     # a refused call changes nothing
    assert rtw.lib().rtw_scene_set_lights(world.handle, None, 1) == A.RTW_E_INVALID
    world.set_lights(None)
    assert len(world.lights()) == 0
    world.close()
    # a sphere scene has no quad to register
    sw = rtw.World(rtw.flatten(rtw.worlds.generate_world(0, "book1")), device=CPU)
    assert set_lights_rc(rtw, sw, [(A.RTW_OBJ_SPHERE, 0)]) == A.RTW_E_INVALID
    assert set_lights_rc(rtw, sw, [(A.RTW_OBJ_QUAD, 0)]) == A.RTW_E_INVALID
    sw.close()
    # a medium's boundary quad
    glass = rtw.Quad.init([0, 0, 0], [1, 0, 0], [0, 1, 0], rtw.DiffuseLight.fromColor([1, 1, 1]))
    objs = S.analytic_objects(rtw) + [rtw.ConstantMedium.initFromColor(glass, 0.1, [1, 1, 1])]
    marr = rtw.flatten(objs)
    mw = rtw.World(marr, device=CPU)
    boundary = tuple(int(x) for x in marr.media[0]["boundary"])
    assert set_lights_rc(rtw, mw, [boundary]) == A.RTW_E_INVALID
    mw.close()


def test_flatten_lights_argument(rtw):
    A = rtw._abi
    objs = S.analytic_objects(rtw, two=True)
    assert rtw.flatten(objs).lights is None
    assert rtw.flatten(objs, lights="emissive").lights.tolist() == [(A.RTW_OBJ_QUAD, 1), (A.RTW_OBJ_QUAD, 2)]
    arr = rtw.flatten(objs, lights=[objs[2]])
    assert arr.lights.tolist() == [(A.RTW_OBJ_QUAD, 2)]
    world = rtw.World(arr, device=CPU)
    assert world.lights().tolist() == [(A.RTW_OBJ_QUAD, 2)]
    world.close()
    with pytest.raises(ValueError):
        rtw.flatten(objs, lights=[rtw.Quad.init([0, 0, 0], [1, 0, 0], [0, 1, 0], objs[1].mat)])
    with pytest.raises(rtw.RtwError):   # World applies the list; the library refuses the floor
        rtw.World(rtw.flatten(objs, lights=[objs[0]]), device=CPU)
    # the box sides of the Cornell box are instance members: "emissive" takes top-level quads only
    assert rtw.flatten(rtw.worlds.cornell_box(), lights="emissive").lights.tolist() == [(A.RTW_OBJ_QUAD, 2)]


def test_off_is_off(rtw):
    arr = rtw.flatten(rtw.worlds.cornell_box())
    cam = rtw.cornell_camera(image_width=32, spp=4, max_depth=50).init()
    never = S.render(rtw, arr, cam, 4, 3)
    world = rtw.World(arr, device=CPU)
    world.set_lights([(rtw._abi.RTW_OBJ_QUAD, 2)])
    on = S.render(rtw, arr, cam, 4, 3, world=world)
    world.set_lights(None)
    cleared = S.render(rtw, arr, cam, 4, 3, world=world)
    world.close()
    assert np.array_equal(cleared, never)
    assert not np.array_equal(on, never)


def test_hash_covers_lights_and_checkpoint_refuses(rtw, tmp_path):
    arr_off = rtw.flatten(rtw.worlds.cornell_box())
    arr_on = rtw.flatten(rtw.worlds.cornell_box(), lights="emissive")
    w_off, w_on = rtw.World(arr_off, device=CPU), rtw.World(arr_on, device=CPU)
    h_off, h_on = scene_hash(rtw, w_off), scene_hash(rtw, w_on)
    assert h_off != h_on
    w_on.set_lights(None)
    assert scene_hash(rtw, w_on) == h_off
    w_on.set_lights(arr_on.lights)
    assert scene_hash(rtw, w_on) == h_on

    def state(world):
        cam = rtw.cornell_camera(image_width=16, spp=4, max_depth=10)
        cam.init()
        return rtw.RayTraceState(cam, rtw.SharedStateImageWriter(16, 16), world, seed=9)

    for src, dst, same in ((w_on, w_off, w_on), (w_off, w_on, w_off)):
        path = str(tmp_path / f"ck_{src is w_on}.bin")
        st = state(src)
        st.camera.render_range(st, 0, st.camera.size, 0, 2)
        st.checkpoint(path, 2)
        with pytest.raises(rtw.RtwError):
            state(dst).resume(path)
        assert state(same).resume(path) == 2
    w_off.close()
    w_on.close()


@pytest.mark.parametrize("two", [False, True], ids=["one_light", "two_lights"])
def test_analytic_form_factor(rtw, two):
    """Seed-mean of 16 x 256 spp against albedo / pi * Le * integral cos cos' / r^2 dA at the pixel-centre hit point,
    within 5 se + 0.5 % (the pixel footprint).  Two lights of different size and radiance: the sum of both terms
    (a wrong 1 / n or a wrong pick of k shows here).  Measured: worst |mean - expected| / bound = 0.94 (one
    light), 0.74 (two)."""
    cam = S.analytic_camera(rtw, S.SPP)
    sel, expected = S.expected_floor(cam, two)
    assert len(sel) > 1000
    img = S.analytic_seed_images(two, True)[:, sel]
    mean, se = img.mean(0), img.std(0, ddof=1) / np.sqrt(len(S.SEEDS))
    z = np.abs(mean - expected) / (5 * se + 0.005 * expected)
    print(f"analytic two={two}: {len(sel)} pixels, worst |mean - expected| / bound = {z.max():.3f}, "
          f"mean se / expected = {(se / expected).mean():.4f}")
    assert (z <= 1).all(), (int(sel[z.argmax()]), z.max())


def test_variance_reduction(rtw):
    """Summed across-seed variance with lights / without, same pixels, equal spp: <= 0.25 (brute force F(1 - F)
    against the ideal mixture's F^2 (1 - F) / (1 + F): F / (1 + F) ~ 0.07 under the light, with a 3 x margin for
    area sampling).  Measured: 0.043."""
    cam = S.analytic_camera(rtw, S.SPP)
    sel, _ = S.expected_floor(cam, False)
    on = S.analytic_seed_images(False, True)[:, sel].var(0, ddof=1).sum()
    off = S.analytic_seed_images(False, False)[:, sel].var(0, ddof=1).sum()
    print(f"variance ratio lights on / off = {on / off:.4f}")
    assert on / off <= 0.25


# ---- against the oracle: Cornell and Cornell smoke, 32 x 32, depth 10, reference BVH mode
CW, CDEPTH, CSPP, OSPP = 32, 10, 256, 512
CSEEDS = tuple(range(40, 48))


@functools.lru_cache(maxsize=None)
def cornell_images(name):
    """(lights on, lights off, oracle): (8, pixels, 3) mean radiance per seed -- the library at 256 spp on the host
    backend, the oracle at 512 spp."""
    import oracle as O
    rtw = S.pkg()
    mode = rtw._abi.RTW_BVH_REFERENCE
    cam = rtw.cornell_camera(image_width=CW, spp=CSPP, max_depth=CDEPTH).init()
    out = []
    for lights in (True, False):
        arr = S.cornell(rtw, name, lights, mode)
        world = rtw.World(arr, device=CPU)
        out.append(np.stack([S.render(rtw, arr, cam, CSPP, s, world=world)[:, :3] / CSPP for s in CSEEDS]))
        world.close()
    ocam = O.camera(aspect_ratio=1.0, image_width=CW, samples_per_pixel=OSPP, max_depth=CDEPTH, vfov=40.0,
                    lookfrom=(278.0, 278.0, -800.0), lookat=(278.0, 278.0, 0.0), defocus_angle=0.0,
                    pixel_offset=cam.derived.pixel_offset)
    assert ocam.image_height == cam.derived.image_height
    ow = O.World.from_arrays(S.cornell(rtw, name, False, mode))
    pix = np.arange(cam.size, dtype=np.uint32)
    thr = min(os.cpu_count() or 1, 16)
    out.append(np.stack([ow.render_pixels(ocam, s, pix, 0, OSPP, threads=thr)[:, :3] / OSPP for s in CSEEDS]))
    out = [o.astype(np.float64) for o in out]
    for o in out:
        o.setflags(write=False)
    return tuple(out)


def blocks(img):
    """(seeds, 32 * 32, 3) -> (seeds, 8 * 8, 3): means over 4 x 4 pixel blocks."""
    s = img.shape[0]
    return img.reshape(s, CW // 4, 4, CW // 4, 4, 3).mean(axis=(2, 4)).reshape(s, -1, 3)


@pytest.mark.parametrize("name", ["cornell", "cornell_smoke"])
def test_unbiased_against_oracle(rtw, oracle, name):
    """Every 4 x 4 block and channel, and the whole-image mean per channel, within 5 sqrt(seA^2 + seB^2) of the
    oracle's (se: the standard error over the 8 seeds)."""
    on, _, ref = cornell_images(name)
    n = np.sqrt(len(CSEEDS))
    for what, a, b in (("blocks", blocks(on), blocks(ref)), ("image", on.mean(1), ref.mean(1))):
        da = a.mean(0) - b.mean(0)
        se = np.sqrt((a.std(0, ddof=1) / n) ** 2 + (b.std(0, ddof=1) / n) ** 2)
        z = np.abs(da) / (5 * se)
        print(f"{name} {what}: worst |difference| / (5 se) = {z.max():.3f}")
        assert (z <= 1).all(), (name, what, z.max())


# MSE(256 spp, lights on) / MSE(256 spp, lights off) against the pooled oracle image, mean over the 8 seeds,
# measured on the host backend
MEASURED_MSE_RATIO = {"cornell": 0.5705, "cornell_smoke": 0.4046}


@pytest.mark.parametrize("name", ["cornell", "cornell_smoke"])
def test_noise_against_oracle(rtw, oracle, name):
    on, off, ref = cornell_images(name)
    pooled = ref.mean(0)
    ratio = ((on - pooled) ** 2).mean() / ((off - pooled) ** 2).mean()
    print(f"{name}: MSE lights on / off at {CSPP} spp = {ratio:.4f}")
    assert MEASURED_MSE_RATIO[name] < 1
    assert ratio <= 1.25 * MEASURED_MSE_RATIO[name]


def test_schedule_invariance(rtw):
    """Lights on, Cornell 40 x 40 x 6 spp on the host: [0, 3) + [3, 6) == [0, 6); rtw_render_rows shards reassemble
    to the frame; cpu_threads 1 == 4."""
    arr = S.cornell(rtw, "cornell", True)
    cam = rtw.cornell_camera(image_width=40, spp=6, max_depth=50).init()
    W = H = 40
    full = S.render(rtw, arr, cam, 6, 7, tuning={"cpu_threads": 4})
    assert np.array_equal(S.render(rtw, arr, cam, 6, 7, tuning={"cpu_threads": 1}), full)
    world = rtw.World(arr, device=CPU)
    buf = np.zeros((cam.size, 4), np.float32)
    for a, b in ((0, 3), (3, 6)):
        rtw._abi.check(rtw.lib().rtw_render(world.handle, C.byref(cam.derived), 0, cam.size, a, b, 7, buf.ctypes.data,
                                            None, rtw._abi.PROGRESS_FN(0), None), "rtw_render")
    assert np.array_equal(buf, full)
    image = np.zeros((H, W, 4), np.float32)
    for k in range(3):
        rows = rtw.distributed.shard_rows(H, 8, 3, k)
        tile = np.zeros((len(rows) * W, 4), np.float32)
        rtw.distributed.render_rows_host(world, cam, 8, 3, k, 0, 6, tile, seed=7)
        image[rows] = tile.reshape(len(rows), W, 4)
    world.close()
    assert np.array_equal(image.reshape(-1, 4), full)
