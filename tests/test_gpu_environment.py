"""Environment maps (rtw_scene_set_environment) on the GPU: every kernel family's RTW_F_ENV instantiation renders the
host backend's image bit for bit (the lookup, the two searches and the density are plain fp32 in one association) --
on object scenes and on a scene of spheres alone, whose octant copies, compact nodes and hoisted spheres the general
kernels then walk or leave aside --, clearing restores the kernels without it, and the guides and the debug sample
agree.  Images are 64 x 48 x 8 spp, maps 37 x 19 and 64 x 32."""
import ctypes as C
import functools

import numpy as np
import pytest

import environment_scenes as E

pytestmark = pytest.mark.gpu

SCENES = ("mesh_lights", "mesh", "smoke", "book1", "tree")
SEED = 21


def env_of(rtw, name):
    # the odd map (no power of two) under the sphere scene and the smoke, turned; the other under the meshes
    if name in ("book1", "smoke"):
        return E.small_env(rtw, 37, 19, rotate_y=40.0, scale=(1.0, 0.9, 0.8))
    return E.small_env(rtw, 64, 32)


@functools.lru_cache(maxsize=None)
def host_image(name):
    rtw = E.pkg()
    arr, cam = E.parity_scene(rtw, name, env_of(rtw, name))
    out = E.render(rtw, arr, cam, SEED)
    out.setflags(write=False)
    return out


def knobs(rtw):
    A = rtw._abi
    return {"default": None,
            "kernel_persistent": {"kernel": A.RTW_KERNEL_PERSISTENT}, "kernel_simple": {"kernel": A.RTW_KERNEL_SIMPLE},
            "fuse_0": {"fuse": 0},                  # split trace / shade
            "deal_all": {"deal": A.RTW_DEAL_ALL},   # the bucketed queues on a small image
            "wf_iters_1": {"wf_iters": 1},          # the tail does nearly every bounce
            "wf_iters_100": {"wf_iters": 100}}      # no tail


KNOBS = ("default", "kernel_persistent", "kernel_simple", "fuse_0", "deal_all", "wf_iters_1", "wf_iters_100")


@pytest.mark.parametrize("knob", KNOBS)
@pytest.mark.parametrize("name", SCENES)
def test_gpu_equals_host_every_family(rtw, name, knob):
    """GPU == host backend bit for bit under the knobs that change which kernel walks and shades a bounce (so the
    families agree with each other too)."""
    arr, cam = E.parity_scene(rtw, name, env_of(rtw, name))
    got = E.render(rtw, arr, cam, SEED, device=0, tuning=knobs(rtw)[knob])
    assert np.array_equal(got, host_image(name)), (name, knob)


def test_sphere_scene_carries_its_structures(rtw):
    """The sphere scene of the parity test is one with octant copies and a hoisted sphere under the default tuning
    (what the environment classes must walk or leave aside), and its image is not the one without the map."""
    arr, cam = E.parity_scene(rtw, "book1", None)
    world = rtw.World(arr, device=0)
    st = world.stats()
    plain = E.render(rtw, arr, cam, SEED, world=world)
    world.close()
    assert st["n_hoisted"] >= 1
    assert not np.array_equal(plain, host_image("book1"))


@pytest.mark.parametrize("name", ["mesh_lights", "book1"])
def test_debug_sample_equals_render(rtw, name):
    """rtw_debug_sample (one lane of the per-sample kernel) sums to the rendered pixel."""
    arr, cam = E.parity_scene(rtw, name, env_of(rtw, name))
    world = rtw.World(arr, device=0)
    out = np.zeros(32, np.float32)
    ref = host_image(name)
    spp = cam.derived.samples_per_pixel
    for pixel in (0, 777, cam.size - 1, cam.size // 2 + 13):
        acc = np.zeros(3, np.float32)
        for s in range(spp):
            rtw._abi.check(rtw.lib().rtw_debug_sample(world.handle, C.byref(cam.derived), SEED, pixel, s,
                                                      out.ctypes.data), "rtw_debug_sample")
            acc += out[:3]
        assert np.array_equal(acc, ref[pixel, :3]), (name, pixel)
    world.close()


@pytest.mark.parametrize("name", ["mesh", "book1"])
def test_guides_equal_host(rtw, name):
    import torch
    arr, cam = E.parity_scene(rtw, name, env_of(rtw, name))
    host = rtw.World(arr, device=E.CPU)
    ha, hn = host.render_guides(cam)
    host.close()
    assert (ha[:, 3] == 0).any()
    world = rtw.World(arr, device=0)
    a = torch.zeros((cam.size, 4), dtype=torch.float32, device="cuda")
    n = torch.zeros((cam.size, 4), dtype=torch.float32, device="cuda")
    rtw._abi.check(rtw.lib().rtw_render_guides_device(world.handle, C.byref(cam.derived), a.data_ptr(), n.data_ptr(),
                                                      None, 0), "rtw_render_guides_device")
    world.close()
    assert np.array_equal(a.cpu().numpy(), ha) and np.array_equal(n.cpu().numpy(), hn)


@pytest.mark.parametrize("name", ["mesh_lights", "book1"])
def test_clearing_restores_the_parent_kernels(rtw, name):
    arr, cam = E.parity_scene(rtw, name, None)
    never = E.render(rtw, arr, cam, SEED, device=0)
    world = rtw.World(arr, device=0)
    world.set_environment(env_of(rtw, name))
    on = E.render(rtw, arr, cam, SEED, world=world)
    world.set_environment(None)
    cleared = E.render(rtw, arr, cam, SEED, world=world)
    world.close()
    assert np.array_equal(on, host_image(name))
    assert np.array_equal(cleared, never)
    assert not np.array_equal(on, never)


def test_two_devices(rtw):
    import torch
    if torch.cuda.device_count() < 2:
        pytest.skip("needs two devices")
    A = rtw._abi
    arr, cam = E.parity_scene(rtw, "mesh_lights", env_of(rtw, "mesh_lights"))
    w0, w1 = rtw.World(arr, device=0), rtw.World(arr, device=1)
    ctxs = (C.c_void_p * 2)(w0.handle, w1.handle)
    m = C.c_void_p()
    w1.set_environment(E.small_env(rtw, 64, 32, rotate_y=1.0))
    assert rtw.lib().rtw_multi_create(ctxs, 2, C.byref(m)) == A.RTW_E_INVALID
    w1.set_environment(env_of(rtw, "mesh_lights"))
    A.check(rtw.lib().rtw_multi_create(ctxs, 2, C.byref(m)), "rtw_multi_create")
    buf = np.zeros((cam.size, 4), np.float32)
    A.check(rtw.lib().rtw_render_multi_ex(m, C.byref(cam.derived), 8, 0, cam.derived.samples_per_pixel, SEED,
                                          buf.ctypes.data, None), "rtw_render_multi_ex")
    rtw.lib().rtw_multi_destroy(m)
    w0.close()
    w1.close()
    assert np.array_equal(buf, host_image("mesh_lights"))
