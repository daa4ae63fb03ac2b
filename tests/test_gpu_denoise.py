"""Denoised previews on the GPU: the guide kernels and the a-trous filter kernels give the host backend's bits --
the guides of six scenes (sphere scenes under three tunings, textures, quads and instances, media, registered
lights, vertex attributes and instance trees) through the host-buffer and the device entry points; the filter on
seeded inputs at four frame sizes (partial blocks, one pixel, several blocks), 1 / 5 / 8 passes, demodulation on and
off, each sigma 0, in place and on a caller's stream; and render + guides + filter end to end.  Frames are 40 x 24
with pixel_offset 1 unless a case says otherwise."""
import ctypes as C

import numpy as np
import pytest

import denoise_scenes as D

pytestmark = pytest.mark.gpu


def gpu_tensor(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.mark.parametrize("name", ["book1", "book1_orders8", "book1_hoist0", "earth_perlin", "cornell",
                                  "cornell_smoke", "simple_light", "cornell_mesh"])
def test_guides_equal_host(rtw, name):
    import torch
    arr, tuning, cam = D.scene(rtw, name)
    assert (cam.derived.image_width, cam.derived.image_height, cam.derived.pixel_offset) == (D.GW, D.GH, 1)
    ha, hn = D.host_guides(name)
    world = rtw.World(arr, device=0, tuning=tuning)
    if name == "simple_light":
        assert len(world.lights()) == 2
    if name == "cornell_mesh":
        assert len(world.vertex_attrs()[0]) == 320
    a, n = world.render_guides(cam)                                         # the host-buffer entry point
    da = torch.full((cam.size, 4), -1.0, dtype=torch.float32, device="cuda")
    dn = torch.full((cam.size, 4), -1.0, dtype=torch.float32, device="cuda")
    rc = rtw.lib().rtw_render_guides_device(world.handle, C.byref(cam.derived), da.data_ptr(), dn.data_ptr(), None, 0)
    rtw._abi.check(rc, "rtw_render_guides_device")
    world.close()
    assert np.array_equal(a, ha) and np.array_equal(n, hn)
    assert np.array_equal(da.cpu().numpy(), ha) and np.array_equal(dn.cpu().numpy(), hn)
    assert (hn[:, 3] > 0).sum() > 100 and (hn[:, 3] == 0).sum() > 50


@pytest.fixture(scope="module")
def gpu_world(rtw):
    w = rtw.World(rtw.flatten(rtw.worlds.two_spheres_world()), device=0)
    yield w
    w.close()


S0 = (1.0, 0.5, 0.2)
# (passes, demodulate, (sigma_color, sigma_normal, sigma_depth))
CONFIGS = [(1, True, S0), (5, True, S0), (8, True, S0), (5, False, S0), (5, True, (0.0, 0.5, 0.2)),
           (5, True, (1.0, 0.0, 0.2)), (5, True, (1.0, 0.5, 0.0)), (8, False, (0.0, 0.0, 0.0))]


def params(rtw, cfg):
    passes, demod, sig = cfg
    return rtw._abi.denoise_params(passes=passes, demodulate=demod, sigma_color=sig[0], sigma_normal=sig[1],
                                   sigma_depth=sig[2])


def host_filter(rtw, acc, alb, nd, W, H, cfg):
    passes, demod, sig = cfg
    return D.denoise(rtw, D.host_world(), acc, alb, nd, W, H, passes=passes, demodulate=demod, sigma_color=sig[0],
                     sigma_normal=sig[1], sigma_depth=sig[2])


@pytest.mark.parametrize("W,H", [(40, 24), (33, 17), (1, 1), (130, 70)])
def test_filter_equals_host(rtw, gpu_world, W, H):
    """At 8 passes the taps are up to 256 px away: nearly all of them are off these frames."""
    import torch
    acc, alb, nd = D.random_inputs(W, H, seed=W)
    d_acc, d_alb, d_nd = gpu_tensor(acc), gpu_tensor(alb), gpu_tensor(nd)
    L = rtw.lib()
    for cfg in CONFIGS:
        p = params(rtw, cfg)
        want = host_filter(rtw, acc, alb, nd, W, H, cfg)
        d_out = torch.full((W * H, 4), -1.0, dtype=torch.float32, device="cuda")
        rc = L.rtw_denoise_device(gpu_world.handle, W, H, d_acc.data_ptr(), d_alb.data_ptr() if cfg[1] else None,
                                  d_nd.data_ptr(), C.byref(p), d_out.data_ptr(), None, 0)
        rtw._abi.check(rc, "rtw_denoise_device")
        assert np.array_equal(d_out.cpu().numpy(), want, equal_nan=True), cfg
        if W * H >= 12:
            assert np.isfinite(want).all() and (want[D.zero_w_pixel(W, H)] == 0).all()
    # in place, and through the host-buffer entry point of the GPU context
    cfg = CONFIGS[1]
    want = host_filter(rtw, acc, alb, nd, W, H, cfg)
    buf = d_acc.clone()
    rc = L.rtw_denoise_device(gpu_world.handle, W, H, buf.data_ptr(), d_alb.data_ptr(), d_nd.data_ptr(),
                              C.byref(params(rtw, cfg)), buf.data_ptr(), None, 0)
    rtw._abi.check(rc, "rtw_denoise_device")
    assert np.array_equal(buf.cpu().numpy(), want, equal_nan=True)
    got = gpu_world.denoise(acc, (alb, nd), W, H, passes=cfg[0], demodulate=cfg[1], sigma_color=cfg[2][0],
                            sigma_normal=cfg[2][1], sigma_depth=cfg[2][2])
    assert np.array_equal(got, want, equal_nan=True)


def test_filter_on_a_callers_stream(rtw, gpu_world):
    import torch
    W, H = D.GW, D.GH
    acc, alb, nd = D.random_inputs(W, H, seed=3)
    cfg = CONFIGS[1]
    want = host_filter(rtw, acc, alb, nd, W, H, cfg)
    d_acc, d_alb, d_nd = gpu_tensor(acc), gpu_tensor(alb), gpu_tensor(nd)
    d_out = torch.full((W * H, 4), -1.0, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    rc = rtw.lib().rtw_denoise_device(gpu_world.handle, W, H, d_acc.data_ptr(), d_alb.data_ptr(), d_nd.data_ptr(),
                                      C.byref(params(rtw, cfg)), d_out.data_ptr(), C.c_void_p(stream.cuda_stream),
                                      rtw._abi.RTW_RENDER_NO_SYNC)
    rtw._abi.check(rc, "rtw_denoise_device")
    stream.synchronize()
    assert np.array_equal(d_out.cpu().numpy(), want, equal_nan=True)
    # a second call on the context's own stream is ordered after it (other sizes: the planes are reused)
    again = gpu_world.denoise(acc, (alb, nd), W, H, passes=cfg[0], demodulate=cfg[1], sigma_color=cfg[2][0],
                              sigma_normal=cfg[2][1], sigma_depth=cfg[2][2])
    assert np.array_equal(again, want, equal_nan=True)


def test_refusals_on_a_gpu_context(rtw, gpu_world):
    import torch
    A = rtw._abi
    W, H = 8, 6
    acc, alb, nd = D.random_inputs(W, H, bad=False)
    d_acc, d_alb, d_nd = gpu_tensor(acc), gpu_tensor(alb), gpu_tensor(nd)
    d_out = torch.full((W * H, 4), 7.0, dtype=torch.float32, device="cuda")
    L = rtw.lib()
    for kw, flags in ((dict(passes=0), 0), (dict(passes=9), 0), (dict(sigma_color=-1.0), 0), (dict(flags=2), 0),
                      (dict(passes=2), 2)):
        rc = L.rtw_denoise_device(gpu_world.handle, W, H, d_acc.data_ptr(), d_alb.data_ptr(), d_nd.data_ptr(),
                                  C.byref(A.denoise_params(**kw)), d_out.data_ptr(), None, flags)
        assert rc == A.RTW_E_INVALID, (kw, flags)
    rc = L.rtw_denoise_device(gpu_world.handle, W, H, d_acc.data_ptr(), None, d_nd.data_ptr(),
                              C.byref(A.denoise_params(demodulate=True)), d_out.data_ptr(), None, 0)
    assert rc == A.RTW_E_INVALID
    torch.cuda.synchronize()
    assert (d_out.cpu().numpy() == 7.0).all()


def test_render_guides_denoise_end_to_end(rtw):
    """4 spp of Cornell, its guides and the filter with the shipped defaults: the GPU context's three calls give the
    host context's bits."""
    arr, _, cam = D.scene(rtw, "cornell")
    outs = []
    for device in (0, D.CPU):
        world = rtw.World(arr, device=device)
        acc = D.render(rtw, world, cam, 4, 11)
        guides = world.render_guides(cam)
        outs.append((acc, world.denoise(acc, guides, D.GW, D.GH)))
        world.close()
    assert np.array_equal(outs[0][0], outs[1][0])
    assert np.array_equal(outs[0][1], outs[1][1], equal_nan=True)
    assert np.isfinite(outs[0][1]).all() and not np.array_equal(outs[0][1], outs[0][0])
