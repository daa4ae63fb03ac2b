"""Sphere lights (rtw_scene_set_lights with RTW_OBJ_SPHERE records) on the GPU: every kernel family's RTW_F_PDF
instantiation renders the host backend's image bit for bit with a quad and a sphere registered (the cone's draws,
its cosine and sine and the densities are plain fp32 / fp64 in one association), also from inside a sphere light
and beside an instance tree; clearing restores the kernels without lights, and row shards reassemble."""
import ctypes as C
import functools

import numpy as np
import pytest

import instance_tree_scenes as T
import lights_scenes as S
import sphere_lights_scenes as P
from test_gpu_lights import KNOBS, knobs

pytestmark = pytest.mark.gpu

# 64 x 36: several waves per tile row; 6 spp: no multiple of the 16-sample run; noise textures: the Perlin LDS stage
W, SPP, SEED = 64, 6, 21


def camera(rtw):
    return rtw.simple_light_camera(image_width=W, spp=SPP).init()   # depth 50


@functools.lru_cache(maxsize=None)
def host_image():
    rtw = S.pkg()
    out = S.render(rtw, P.simple_light(rtw), camera(rtw), SPP, SEED)
    out.setflags(write=False)
    return out


@pytest.mark.parametrize("knob", KNOBS)
def test_gpu_equals_host_every_family(rtw, knob):
    """simple_light, quad + sphere registered: GPU == host backend bit for bit under the knobs that change which
    kernel shades a bounce (so the families agree with each other too)."""
    arr = P.simple_light(rtw)
    assert arr.lights.tolist() == [(rtw._abi.RTW_OBJ_QUAD, 0), (rtw._abi.RTW_OBJ_SPHERE, 2)]
    got = S.render(rtw, arr, camera(rtw), SPP, SEED, device=0, tuning=knobs(rtw)[knob])
    assert np.isfinite(got).all()
    assert np.array_equal(got, host_image()), knob


def test_with_instance_tree(rtw):
    """The RTW_F_ALL | RTW_F_TREE | RTW_F_PDF instantiations: the 300-sphere tree instance scene with one more
    emissive quad and a top-level emissive sphere, every light registered, 48 x 48 x 4 spp."""
    A = rtw._abi
    objs = P.tree_objects(rtw)
    arr = rtw.flatten(objs, lights="emissive+spheres")
    assert [k for k, _ in arr.lights.tolist()] == [A.RTW_OBJ_QUAD, A.RTW_OBJ_QUAD, A.RTW_OBJ_SPHERE]
    cam, _ = T.cameras(48, 50)
    host = T.render(rtw, arr, cam)
    for tuning in (None, {"kernel": A.RTW_KERNEL_PERSISTENT}, {"kernel": A.RTW_KERNEL_SIMPLE}, {"fuse": 0}):
        assert np.array_equal(T.render(rtw, arr, cam, device=0, tuning=tuning), host), tuning
    assert not np.array_equal(host, T.render(rtw, rtw.flatten(objs, lights="emissive"), cam))


def test_inside_a_dome(rtw):
    """The q >= 1 branch on the device: floor and camera inside the only light, 48 x 48 x 8 spp."""
    arr = P.arrays(rtw, "dome")
    cam = S.analytic_camera(rtw, 8, depth=2)
    got = S.render(rtw, arr, cam, 8, 5, device=0)
    assert np.isfinite(got).all()
    assert np.array_equal(got, S.render(rtw, arr, cam, 8, 5))


def test_clearing(rtw):
    arr = P.simple_light(rtw, lights=None)
    cam = camera(rtw)
    never = S.render(rtw, arr, cam, 4, 3, device=0)
    world = rtw.World(arr, device=0)
    world.set_lights([(rtw._abi.RTW_OBJ_QUAD, 0), (rtw._abi.RTW_OBJ_SPHERE, 2)])
    on = S.render(rtw, arr, cam, 4, 3, world=world)
    world.set_lights(None)
    cleared = S.render(rtw, arr, cam, 4, 3, world=world)
    world.close()
    assert np.array_equal(cleared, never)
    assert not np.array_equal(on, never)


def test_row_shards_reassemble(rtw):
    import torch
    arr = P.simple_light(rtw)
    cam = camera(rtw)
    H = cam.derived.image_height
    world = rtw.World(arr, device=0)
    full = torch.zeros((cam.size, 4), dtype=torch.float32, device="cuda")
    rtw._abi.check(rtw.lib().rtw_render_device(world.handle, C.byref(cam.derived), 0, cam.size, 0, SPP, SEED,
                                               full.data_ptr(), None, None), "rtw_render_device")
    img = np.zeros((H, W, 4), np.float32)
    d = rtw.distributed
    for s in range(2):
        tr = d.shard_tile_rows(H, 8, 2, s)
        tile = torch.zeros((tr * W, 4), dtype=torch.float32, device="cuda")
        rtw._abi.check(rtw.lib().rtw_render_rows_device(world.handle, C.byref(cam.derived), 8, 2, s, 0, SPP, SEED,
                                                        tile.data_ptr(), None, None), "rtw_render_rows_device")
        t = tile.cpu().numpy().reshape(-1, W, 4)
        for r in range(tr):
            y = d.shard_row(H, 8, 2, s, r)
            if y < H:
                img[y] = t[r]
    world.close()
    got = full.cpu().numpy()
    assert np.array_equal(img.reshape(-1, 4), got)
    assert np.array_equal(got, host_image())
