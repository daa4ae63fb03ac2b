"""The coherent queues on per-wave LDS cursors (csrc/rtw_wavefront.hip wf_push_bucketed, wf_close_blocks) in
every kernel that pushes: the compact-LDS fused steps of both block shapes, the node-LDS fused step of object
scenes and the split shade.

Where a survivor lands never changes an image, so every render must equal the render of the same build
without bucketing (sort_iters 0: plain appends) bit for bit, and the host backend's.  After every render the
stripe counters must be within the stripe capacity (the queues are not bound-checked on the device).

The frames are small, so deal bit 128 (RTW_DEAL_SMALL_SORT) forces the bucketed queues on; at 64x48 a wave gets
at most one chunk (every bucket's first push opens a block), so one larger frame gives each wave several chunks
and fills open blocks across pushes."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SPP, SEED = 8, 6


def render(rtw, world, cam, spp=SPP):
    buf = np.zeros((cam.size, 4), np.float32)
    rc = rtw.lib().rtw_render(world.handle, C.byref(cam.derived), 0, cam.size, 0, spp, SEED, buf.ctypes.data, None,
                              rtw._abi.PROGRESS_FN(0), None)
    rtw._abi.check(rc, "rtw_render")
    return buf


def stripes_fit(rtw, world):
    cap = C.c_uint32()
    counters = np.zeros(768, np.uint32)
    rtw._abi.check(rtw.lib().rtw_debug_stripe_counters(world.handle, C.byref(cap), counters.ctypes.data),
                   "rtw_debug_stripe_counters")
    assert cap.value > 0 and counters.max() <= cap.value, (int(counters.max()), cap.value)
    return counters


def render_with(rtw, arr, cam, tuning, spp=SPP):
    world = rtw.World(arr, tuning=tuning)
    try:
        out = render(rtw, world, cam, spp)
        counters = stripes_fit(rtw, world)
    finally:
        world.close()
    return out, counters


@pytest.fixture(scope="module")
def book1_small(rtw):
    """The Book-1 scene at 64x48, 8 spp, depth 50: the unbucketed GPU render and the host backend's."""
    arr = rtw.flatten(rtw.worlds.generate_world(0, "book1"))
    cam = rtw.book1_camera(image_width=64, aspect_ratio=64 / 48, spp=SPP, max_depth=50).init()
    plain, _ = render_with(rtw, arr, cam, {"sort_iters": 0, "sort_iters_split": 0})
    host = rtw.World(arr, device=rtw._abi.RTW_DEVICE_CPU)
    ref = render(rtw, host, cam)
    host.close()
    return arr, cam, plain, ref


BUCKETED = [{"deal": 128, "sort_iters": 100}, {"deal": 187}]
KNOBS = [{}, {"sort_bits": 0}, {"sort_bits": 2}, {"sort_bits": 4}, {"clds_shape": 1},
         {"fuse": 0, "sort_iters_split": 100}]


@pytest.mark.parametrize("knob", KNOBS, ids=lambda k: ",".join(f"{a}={b}" for a, b in k.items()) or "default")
@pytest.mark.parametrize("base", BUCKETED, ids=["static100", "deal187"])
def test_book1_bucketed_is_unbucketed(rtw, book1_small, base, knob):
    arr, cam, plain, host = book1_small
    got, _ = render_with(rtw, arr, cam, {**base, **knob})
    assert np.array_equal(got, plain)
    assert np.array_equal(got, host)


def test_unbucketed_is_host(rtw, book1_small):
    _, _, plain, host = book1_small
    assert np.array_equal(plain, host)


@pytest.mark.parametrize("base", BUCKETED, ids=["static100", "deal187"])
def test_blocks_fill_across_pushes(rtw, base):
    """400x240 at 16 spp: 24,000 chunks, several per wave, so buckets meet open blocks with room."""
    arr = rtw.flatten(rtw.worlds.generate_world(0, "book1"))
    cam = rtw.book1_camera(image_width=400, aspect_ratio=400 / 240, spp=16, max_depth=50).init()
    plain, _ = render_with(rtw, arr, cam, {"sort_iters": 0}, 16)
    for knob in ({}, {"clds_shape": 1}):
        got, _ = render_with(rtw, arr, cam, {**base, **knob}, 16)
        assert np.array_equal(got, plain), knob


def test_object_scene_node_lds_step(rtw):
    """The Cornell box through wf_step<FEAT, true> (the 32-B nodes in LDS), every iteration bucketed."""
    W = rtw.worlds
    arr = rtw.flatten(W.cornell_box())
    cam = rtw.Camera(image_width=64, samples_per_pixel=SPP, max_depth=50, aspect_ratio=1.0, vfov=40.0,
                     lookfrom=(278.0, 278.0, -800.0), lookat=(278.0, 278.0, 0.0), defocus_angle=0.0).init()
    plain, _ = render_with(rtw, arr, cam, {"sort_iters": 0, "sort_iters_split": 0})
    host = rtw.World(arr, device=rtw._abi.RTW_DEVICE_CPU)
    ref = render(rtw, host, cam)
    host.close()
    assert np.array_equal(plain, ref)
    for tu in ({"deal": 187, "sort_iters": 100}, {"deal": 128, "sort_iters": 100},
               {"deal": 187, "fuse": 0, "sort_iters_split": 100}):
        got, _ = render_with(rtw, arr, cam, tu)
        assert np.array_equal(got, plain), tu


def test_whole_wave_in_one_bucket(rtw):
    """A camera facing one large mirror sphere (Metal, fuzz 0) through a 1-degree lens: every camera ray hits it
    and reflects back within ~0.02 rad of (1, 1, 1), one direction bucket (x, z >= 0, the top elevation level), so
    the 64 lanes of a chunk push with one key and every push overflows a block."""
    from importlib import import_module
    S = import_module(rtw.__name__ + ".scene")
    objs = [S.Sphere.init([0, 0, 0], 1000, S.Metal.fromColor([0.8, 0.8, 0.8], 0.0)),
            S.Sphere.init([-5000, 0, 0], 1, S.Lambertian.fromColor([0.5, 0.5, 0.5]))]
    arr = rtw.flatten(objs)
    cam = rtw.Camera(image_width=64, samples_per_pixel=SPP, max_depth=50, aspect_ratio=64 / 48, vfov=1.0,
                     lookfrom=(1200.0, 1200.0, 1200.0), lookat=(0.0, 0.0, 0.0), defocus_angle=0.0,
                     background=(0.7, 0.8, 1.0)).init()
    # (one wavefront iteration, then the tail: the counters of iteration 0's pushes are still there after the render)
    plain, plain_counters = render_with(rtw, arr, cam, {"sort_iters": 0, "sort_iters_split": 0, "wf_iters": 1})
    host = rtw.World(arr, device=rtw._abi.RTW_DEVICE_CPU)
    ref = render(rtw, host, cam)
    host.close()
    assert np.array_equal(plain, ref)
    assert plain_counters.sum() == cam.size * SPP  # every camera ray survives its first bounce
    for tu in ({"deal": 128, "sort_iters": 100}, {"deal": 187}, {"deal": 187, "clds_shape": 1},
               {"deal": 128, "fuse": 0, "sort_iters_split": 100}):
        got, counters = render_with(rtw, arr, cam, {**tu, "wf_iters": 1})
        assert np.array_equal(got, plain), tu
        # whole blocks only: 64 lanes, one key -- as many slots as survivors, no partly filled block
        assert counters.sum() == cam.size * SPP, tu
