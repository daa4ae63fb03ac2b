"""Per-vertex normals and uvs on triangles (rtw_scene_set_vertex_attrs) on the GPU: the RTW_F_ALL | RTW_F_TREE |
RTW_F_ATTR [| RTW_F_PDF] kernels of every family render the host backend's image bit for bit -- attributes on a
top-level triangle, in a list instance and in a tree instance, with and without registered lights, and in a scene
without any instance tree; records with flags = 0 and a cleared context render the plain image; row shards
reassemble.  64 x 64 x 6 spp, depth 50."""
import ctypes as C

import numpy as np
import pytest

import mesh_scenes as M
import smooth_scenes as S
from test_gpu_lights import KNOBS, knobs

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("knob", KNOBS)
def test_mixed_equals_host_every_family(rtw, knob):
    """smooth_mixed without lights: the RTW_F_ALL | RTW_F_TREE | RTW_F_ATTR kernels of every family."""
    arr = S.mixed_arrays(False)
    assert arr.lights is None and arr.vertex_attrs is not None
    got = M.render(rtw, arr, M.cornell_mesh_camera(rtw), M.GSPP, M.GSEED, device=0, tuning=knobs(rtw)[knob])
    assert np.isfinite(got).all()
    assert np.array_equal(got, S.mixed_host(False)), knob


def test_mixed_differs_from_flat(rtw):
    A = rtw._abi
    quads, recs = S.mixed_arrays(False).vertex_attrs
    both = A.RTW_ATTR_NORMALS | A.RTW_ATTR_UVS
    # the icosphere's 320 (a tree instance), the box's 12 (a list instance), the free-standing triangle
    assert sorted(recs["flags"].tolist()) == [A.RTW_ATTR_NORMALS] + [A.RTW_ATTR_UVS] * 12 + [both] * 320
    assert not np.array_equal(S.mixed_host(False), S.mixed_host(False, False))
    assert not np.array_equal(S.mixed_host(True), S.mixed_host(True, False))


def test_mixed_with_lights_registered(rtw):
    """The two triangle lights registered as well: the RTW_F_ALL | RTW_F_TREE | RTW_F_PDF | RTW_F_ATTR kernels."""
    A = rtw._abi
    arr = S.mixed_arrays(True)
    assert len(arr.lights) == 2
    cam = M.cornell_mesh_camera(rtw)
    host = S.mixed_host(True)
    assert not np.array_equal(host, S.mixed_host(False))
    for tuning in (None, {"kernel": A.RTW_KERNEL_PERSISTENT}, {"kernel": A.RTW_KERNEL_SIMPLE}, {"fuse": 0}):
        got = M.render(rtw, arr, cam, M.GSPP, M.GSEED, device=0, tuning=tuning)
        assert np.isfinite(got).all()
        assert np.array_equal(got, host), tuning


def test_treeless_equals_host(rtw):
    """No instance tree (hit ids split 24 | 7, rtw_dev_instance.tree = 0) under the RTW_F_TREE instantiation the
    attribute kernels are built on: the default path, the split kernels and the persistent kernel."""
    A = rtw._abi
    arr = S.treeless_arrays()
    assert arr.vertex_attrs is not None and len(arr.vertex_attrs[0]) == 32
    assert not (arr.instances["flags"] & A.RTW_INST_BVH).any() and len(arr.instances) == 1
    cam = M.cornell_mesh_camera(rtw)
    host = S.treeless_host()
    for tuning in (None, {"fuse": 0}, {"kernel": A.RTW_KERNEL_PERSISTENT}):
        got = M.render(rtw, arr, cam, M.GSPP, M.GSEED, device=0, tuning=tuning)
        assert np.isfinite(got).all()
        assert np.array_equal(got, host), tuning


def test_plain_image_from_attribute_kernels(rtw):
    """flags = 0 records on every triangle of cornell_mesh(): the new kernels, the old answer; and clearing on a
    live world restores the plain image."""
    cam = M.cornell_mesh_camera(rtw)
    arr = S.plain_with_empty_records(rtw)
    world = rtw.World(arr, device=0)
    assert len(world.vertex_attrs()[0]) == len(arr.vertex_attrs[0]) > 300
    got = M.render(rtw, arr, cam, M.GSPP, M.GSEED, world=world)
    world.close()
    assert np.array_equal(got, M.cornell_mesh_host(False))
    mixed = S.mixed_arrays(False)
    world = rtw.World(mixed, device=0)
    smooth = M.render(rtw, mixed, cam, M.GSPP, M.GSEED, world=world)
    world.set_vertex_attrs(None)
    cleared = M.render(rtw, mixed, cam, M.GSPP, M.GSEED, world=world)
    world.close()
    assert np.array_equal(smooth, S.mixed_host(False))
    assert np.array_equal(cleared, S.mixed_host(False, False))


def test_row_shards_reassemble(rtw):
    import torch
    arr = S.mixed_arrays(True)
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
    assert np.array_equal(got, S.mixed_host(True))
