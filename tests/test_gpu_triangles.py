"""Triangles (rtw_quad.shape = RTW_QUAD_TRIANGLE) on the GPU: cornell_mesh() -- a top-level triangle, 12 in a list
instance, 320 in a tree instance, two emissive ones -- renders the host backend's image bit for bit in every kernel
family, without lights and with the two triangle lights registered (the fold of the two draws, the halved area and
the shape test in light_pdf are plain fp32); an instance tree over a closed mesh equals the list, also as a medium
boundary beside quads; row shards reassemble.  64 x 64 x 6 spp, depth 50."""
import ctypes as C

import numpy as np
import pytest

import instance_tree_scenes as T
import mesh_scenes as M
from test_gpu_lights import KNOBS, knobs

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("knob", KNOBS)
def test_gpu_equals_host_every_family(rtw, knob):
    """No lights registered: the RTW_F_ALL | RTW_F_TREE kernels of every family."""
    arr = rtw.flatten(M.mixed_objects(rtw))
    assert arr.lights is None
    got = M.render(rtw, arr, M.cornell_mesh_camera(rtw), M.GSPP, M.GSEED, device=0, tuning=knobs(rtw)[knob])
    assert np.isfinite(got).all()
    assert np.array_equal(got, M.cornell_mesh_host(False)), knob


def test_triangle_lights_registered(rtw):
    """The two emissive triangles registered: the RTW_F_PDF instantiations; another image than without; clearing
    restores the render without lights."""
    A = rtw._abi
    arr = rtw.flatten(M.mixed_objects(rtw), lights="emissive")
    assert arr.lights.tolist() == [(A.RTW_OBJ_QUAD, 2), (A.RTW_OBJ_QUAD, 3)]
    assert A.quad_shape(arr.quads)[[2, 3]].tolist() == [A.RTW_QUAD_TRIANGLE] * 2
    cam = M.cornell_mesh_camera(rtw)
    host = M.cornell_mesh_host(True)
    assert not np.array_equal(host, M.cornell_mesh_host(False))
    for tuning in (None, {"kernel": A.RTW_KERNEL_PERSISTENT}, {"kernel": A.RTW_KERNEL_SIMPLE}, {"fuse": 0}):
        got = M.render(rtw, arr, cam, M.GSPP, M.GSEED, device=0, tuning=tuning)
        assert np.isfinite(got).all()
        assert np.array_equal(got, host), tuning
    world = rtw.World(arr, device=0)
    world.set_lights(None)
    cleared = M.render(rtw, arr, cam, M.GSPP, M.GSEED, world=world)
    world.close()
    assert np.array_equal(cleared, M.cornell_mesh_host(False))


@pytest.mark.parametrize("scene", ["solid", "medium", "smoke_walls"])
def test_tree_equals_list(rtw, scene):
    """The 80-triangle icosphere (every edge shared) under RotateY + Translate as a tree and as a list, on the
    device, against the host's list render: solid, as a medium boundary, and as a medium boundary beside Cornell
    smoke's walls (media and quads under RTW_F_ALL | RTW_F_TREE)."""
    if scene == "smoke_walls":
        build = lambda bvh: M.ico_smoke_objects(rtw, bvh)                                   # noqa: E731
        cam = rtw.cornell_smoke_camera(image_width=48, spp=8, max_depth=50).init()
    else:
        build = lambda bvh: M.ico_objects(rtw, bvh, scene == "medium")                      # noqa: E731
        cam = rtw.Camera(image_width=48, samples_per_pixel=8, max_depth=50, **T.CAM_KW).init()
    host = M.render(rtw, rtw.flatten(build(False)), cam, 8, 11)
    for bvh in (True, False):
        got = M.render(rtw, rtw.flatten(build(bvh)), cam, 8, 11, device=0)
        assert np.isfinite(got).all()
        assert np.array_equal(got, host), (scene, bvh)


def test_row_shards_reassemble(rtw):
    import torch
    arr = rtw.flatten(M.mixed_objects(rtw), lights="emissive")
    cam = M.cornell_mesh_camera(rtw)
    H, W = cam.derived.image_height, M.GW
    world = rtw.World(arr, device=0)
    full = torch.zeros((cam.size, 4), dtype=torch.float32, device="cuda")
    rtw._abi.check(rtw.lib().rtw_render_device(world.handle, C.byref(cam.derived), 0, cam.size, 0, M.GSPP, M.GSEED,
                                               full.data_ptr(), None, None), "rtw_render_device")
    img = np.zeros((H, W, 4), np.float32)
    d = rtw.distributed
    for s in range(2):
        tr = d.shard_tile_rows(H, 8, 2, s)
        tile = torch.zeros((tr * W, 4), dtype=torch.float32, device="cuda")
        rtw._abi.check(rtw.lib().rtw_render_rows_device(world.handle, C.byref(cam.derived), 8, 2, s, 0, M.GSPP,
                                                        M.GSEED, tile.data_ptr(), None, None), "rtw_render_rows_device")
        t = tile.cpu().numpy().reshape(-1, W, 4)
        for r in range(tr):
            y = d.shard_row(H, 8, 2, s, r)
            if y < H:
                img[y] = t[r]
    world.close()
    got = full.cpu().numpy()
    assert np.array_equal(img.reshape(-1, 4), got)
    assert np.array_equal(got, M.cornell_mesh_host(True))
