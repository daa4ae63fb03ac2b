"""Light importance sampling (rtw_scene_set_lights) on the GPU: every kernel family's RTW_F_PDF instantiation
renders the host backend's image bit for bit (the mixture's draws and densities are plain fp32 in one
association), clearing the lights restores the kernels without them, and row shards reassemble."""
import ctypes as C
import functools

import numpy as np
import pytest

import instance_tree_scenes as T
import lights_scenes as S

pytestmark = pytest.mark.gpu

SCENES = ("cornell", "cornell_smoke")
W, SPP, DEPTH, SEED = 64, 6, 50, 21   # 64 tiles, several waves per tile row; 6 spp: no multiple of the 16-sample run


def camera(rtw):
    return rtw.cornell_camera(image_width=W, spp=SPP, max_depth=DEPTH).init()


@functools.lru_cache(maxsize=None)
def host_image(name):
    rtw = S.pkg()
    out = S.render(rtw, S.cornell(rtw, name, True), camera(rtw), SPP, SEED)
    out.setflags(write=False)
    return out


def knobs(rtw):
    A = rtw._abi
    return {"default": None,                                    # test 9: the product path
            "kernel_persistent": {"kernel": A.RTW_KERNEL_PERSISTENT}, "kernel_simple": {"kernel": A.RTW_KERNEL_SIMPLE},
            "wf_iters_1": {"wf_iters": 1},                      # the tail does nearly every bounce
            "wf_iters_100": {"wf_iters": 100},                  # no tail
            "lds_0": {"lds": 0},                                # everything through L1/L2
            "fuse_0": {"fuse": 0},                              # split trace / shade
            "fuse_7": {"fuse": 7},
            "fuse_0_lds_0": {"fuse": 0, "lds": 0},              # split kernels and the global tail
            "sort_iters_0": {"sort_iters": 0},
            "deal_0": {"deal": 0}, "deal_all": {"deal": A.RTW_DEAL_ALL}}


KNOBS = ("default", "kernel_persistent", "kernel_simple", "wf_iters_1", "wf_iters_100", "lds_0", "fuse_0", "fuse_7",
         "fuse_0_lds_0", "sort_iters_0", "deal_0", "deal_all")


@pytest.mark.parametrize("knob", KNOBS)
@pytest.mark.parametrize("name", SCENES)
def test_gpu_equals_host_every_family(rtw, name, knob):
    """GPU == host backend bit for bit, lights on, under the knobs that change which kernel shades a bounce
    (so the families agree with each other too)."""
    got = S.render(rtw, S.cornell(rtw, name, True), camera(rtw), SPP, SEED, device=0, tuning=knobs(rtw)[knob])
    assert np.array_equal(got, host_image(name)), (name, knob)


def test_with_instance_tree(rtw):
    """The RTW_F_ALL | RTW_F_TREE | RTW_F_PDF instantiations: the 300-sphere tree instance scene with one more
    emissive quad, both lights registered, 48 x 48 x 4 spp."""
    objs = T.cluster_objects(rtw) + [rtw.Quad.init([400, 300, 100], [0, 120, 0], [0, 0, 150],
                                                    rtw.DiffuseLight.fromColor([5, 4, 3]))]
    arr = rtw.flatten(objs, lights="emissive")
    assert len(arr.lights) == 2
    cam, _ = T.cameras(48, 50)
    host = T.render(rtw, arr, cam)
    for tuning in (None, {"kernel": rtw._abi.RTW_KERNEL_PERSISTENT}, {"kernel": rtw._abi.RTW_KERNEL_SIMPLE},
                   {"fuse": 0}):
        assert np.array_equal(T.render(rtw, arr, cam, device=0, tuning=tuning), host), tuning
    assert not np.array_equal(host, T.render(rtw, rtw.flatten(objs), cam))


def test_two_lights(rtw):
    arr = S.analytic_arrays(rtw, two=True)
    cam = S.analytic_camera(rtw, 8, depth=2)
    assert np.array_equal(S.render(rtw, arr, cam, 8, 5, device=0), S.render(rtw, arr, cam, 8, 5))


def test_clearing(rtw):
    arr = rtw.flatten(rtw.worlds.cornell_box())
    cam = rtw.cornell_camera(image_width=64, spp=4, max_depth=50).init()
    never = S.render(rtw, arr, cam, 4, 3, device=0)
    world = rtw.World(arr, device=0)
    world.set_lights([(rtw._abi.RTW_OBJ_QUAD, 2)])
    on = S.render(rtw, arr, cam, 4, 3, world=world)
    world.set_lights(None)
    cleared = S.render(rtw, arr, cam, 4, 3, world=world)
    world.close()
    assert np.array_equal(cleared, never)
    assert not np.array_equal(on, never)


def test_row_shards_reassemble(rtw):
    import torch
    arr = S.cornell(rtw, "cornell", True)
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
    assert np.array_equal(got, host_image("cornell"))
