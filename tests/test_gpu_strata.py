"""Stratified pixel samples (rtw_camera.strata) on the GPU: every kernel family draws the jitter of the host
backend, bit for bit.  Each case renders strata 3, samples [0, 7) + [7, 20) -- two full passes of 9 cells and a
prefix of 2, cut inside the first pass -- of a 40 x 24 frame (partial 8 x 8 tiles) with pixel_offset 1 and compares
with the host backend's one-call image (tests/strata_scenes.py, rendered once per scene)."""
import ctypes as C

import numpy as np
import pytest

import strata_scenes as S

pytestmark = pytest.mark.gpu

W, H = S.GW, S.GH


def gpu_split(rtw, arr, cam, tuning=None):
    world = rtw.World(arr, device=0, tuning=tuning)
    buf = S.render(rtw, world, cam, S.GS0, S.GSPLIT, S.GSEED)
    S.render(rtw, world, cam, S.GSPLIT, S.GS1, S.GSEED, buf=buf)
    world.close()
    return buf


BOOK1_TUNINGS = [{}, {"tile_lists": 0}, {"tile_lists": 128}, {"bvh_orders": 8}, {"fuse": 0},
                 {"lds": 127 & ~2, "fuse": 5}, {"deal": 187}, {"deal": 0}, {"wf_paths": 4096},
                 {"kernel": 1}, {"kernel": 2}]


@pytest.mark.parametrize("tuning", BOOK1_TUNINGS, ids=lambda t: ",".join(f"{k}={v}" for k, v in t.items()) or "default")
def test_book1_defocus(rtw, tuning):
    """Book-1 with its defocus disk: the compact-LDS fused step with and without the tile lists, the split trace /
    shade (CAM instantiations), the fused step through L1/L2, both deals, many batches, and the persistent
    (kernel 1) and simple (kernel 2) kernels."""
    A = rtw._abi
    assert (A.RTW_KERNEL_PERSISTENT, A.RTW_KERNEL_SIMPLE) == (1, 2)
    arr, cam = S.scene("book1")
    assert cam.derived.strata == 3 and cam.derived.pixel_offset == 1 and cam.derived.defocus_angle > 0
    got = gpu_split(rtw, arr, cam, tuning)
    assert (got[:, 3] == S.GS1).all()
    assert np.array_equal(got, S.host_image("book1"))


@pytest.mark.parametrize("cam_seed", range(6))
def test_tile_lists_random_cameras_strata(rtw, cam_seed):
    """The cameras of test_gpu_parity.py::test_tile_lists_random_cameras with strata 5: a cell is closed on both
    sides (px reaches +0.5 exactly), which the lists' pixel rectangle -- closed, widened by 10^-3 relative -- covers:
    tile lists on and off render the same bits."""
    arr = S.book1_arrays()
    g = np.random.default_rng(100 + cam_seed)
    lookfrom = tuple(float(v) for v in g.uniform([-14, 0.3, -14], [14, 6, 14]))
    lookat = tuple(float(v) for v in g.uniform([-4, 0, -4], [4, 1.5, 4]))
    cam = rtw.Camera(aspect_ratio=float(g.uniform(0.6, 2.0)), image_width=int(g.integers(96, 200)),
                     samples_per_pixel=3, max_depth=8, background_mode=rtw._abi.RTW_BG_GRADIENT,
                     vfov=float(g.uniform(8, 100)), lookfrom=lookfrom, lookat=lookat,
                     defocus_angle=float(g.choice([0.0, 0.6, 4.0, 12.0])),
                     focus_dist=float(g.uniform(0.5, 20)), strata=5).init()
    outs = []
    for tl in (0, 1):
        w = rtw.World(arr, tuning={"tile_lists": tl})
        outs.append(S.render(rtw, w, cam, 0, 3, cam_seed))
        w.close()
    assert np.isfinite(outs[1]).all()
    assert np.array_equal(outs[0], outs[1])


@pytest.mark.parametrize("name", ["earth_perlin", "cornell", "cornell_smoke", "simple_light", "cornell_mesh_smooth"])
def test_scene_classes(rtw, name):
    """The node-LDS steps and the other translation units: textured spheres, objects, media, registered quad and
    sphere lights (the mixture density), a smooth mesh (vertex attributes, instance trees)."""
    arr, cam = S.scene(name)
    assert np.array_equal(gpu_split(rtw, arr, cam), S.host_image(name))


def test_row_shards_reassemble(rtw):
    import torch
    arr, cam = S.scene("book1")
    world = rtw.World(arr, device=0)
    img = np.zeros((H, W, 4), np.float32)
    d = rtw.distributed
    for s in range(3):
        tr = d.shard_tile_rows(H, 5, 3, s)
        tile = torch.zeros((tr * W, 4), dtype=torch.float32, device="cuda")
        for a, b in ((S.GS0, S.GSPLIT), (S.GSPLIT, S.GS1)):
            rtw._abi.check(rtw.lib().rtw_render_rows_device(world.handle, C.byref(cam.derived), 5, 3, s, a, b, S.GSEED,
                                                            tile.data_ptr(), None, None), "rtw_render_rows_device")
        t = tile.cpu().numpy().reshape(-1, W, 4)
        for r in range(tr):
            y = d.shard_row(H, 5, 3, s, r)
            if y < H:
                img[y] = t[r]
    world.close()
    assert np.array_equal(img.reshape(-1, 4), S.host_image("book1"))


def test_multi_gpu(rtw):
    import torch
    n = min(8, torch.cuda.device_count())
    if n < 2:
        pytest.skip("needs at least 2 devices")
    arr, cam = S.scene("book1")
    worlds = [rtw.World(arr, device=k) for k in range(n)]
    m = rtw.distributed.MultiDeviceRender(worlds, rows_per_block=8)
    got = np.zeros((cam.size, 4), np.float32)
    m.render_host(cam, S.GS0, S.GSPLIT, got, seed=S.GSEED)
    m.render_host(cam, S.GSPLIT, S.GS1, got, seed=S.GSEED)
    m.close()
    for w in worlds:
        w.close()
    assert np.array_equal(got, S.host_image("book1"))


def test_refusal(rtw):
    """rtw_render_device refuses a camera poked past RTW_MAX_STRATA and launches nothing."""
    import torch
    arr, _ = S.scene("book1")
    cam = S.book1_camera(rtw)
    cam.derived.strata = 257
    world = rtw.World(arr, device=0)
    buf = torch.zeros((cam.size, 4), dtype=torch.float32, device="cuda")
    rc = rtw.lib().rtw_render_device(world.handle, C.byref(cam.derived), 0, cam.size, 0, 4, S.GSEED, buf.data_ptr(),
                                     None, None)
    assert rc == rtw._abi.RTW_E_INVALID and b"strata" in rtw.lib().rtw_last_error()
    out = np.zeros(3, np.float32)
    assert rtw.lib().rtw_debug_sample(world.handle, C.byref(cam.derived), 0, 0, 0,
                                      out.ctypes.data) == rtw._abi.RTW_E_INVALID
    torch.cuda.synchronize()
    assert not buf.any().item()
    world.close()
