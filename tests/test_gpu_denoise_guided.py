"""The variance-guided filter on the GPU: rtw_denoise_guided gives the host backend's bits -- at 1 x 1, 33 x 17
(partial blocks), 40 x 24 and 130 x 70 (halos that cross block borders at spacing 1 and 2, wide passes that reach past
them), 1 / 5 / 8 passes, demodulation on and off, with and without variance_out, in place, on a caller's stream,
through the device and the host-buffer entry points, with the words past the arrays' ends untouched; refusals; and
render + moments + estimate + filter end to end."""
import ctypes as C

import numpy as np
import pytest

import denoise_scenes as D
import guided_scenes as G

pytestmark = pytest.mark.gpu
PAD = 64
S0 = (1.0, 0.5, 0.2)
# (passes, demodulate, (sigma_color, sigma_normal, sigma_depth))
CONFIGS = [(1, True, S0), (5, True, S0), (8, True, S0), (5, False, S0), (1, False, S0), (8, False, (0.0, 0.0, 0.0)),
           (5, True, (0.0, 0.5, 0.2))]


@pytest.fixture(scope="module")
def gpu_world(rtw):
    w = rtw.World(rtw.flatten(rtw.worlds.two_spheres_world()), device=0)
    yield w
    w.close()


def upload(a, fill=-3.0):
    import torch
    t = torch.full((a.size + PAD,), fill, dtype=torch.float32, device="cuda")
    t[:a.size] = torch.from_numpy(np.ascontiguousarray(a).reshape(-1)).cuda()
    return t


def body(t, shape):
    n = int(np.prod(shape))
    host = t.cpu().numpy()
    assert (host[n:] == -3.0).all(), "words past the array's end were written"
    return host[:n].reshape(shape)


def keywords(cfg):
    passes, demod, sig = cfg
    return dict(passes=passes, demodulate=demod, sigma_color=sig[0], sigma_normal=sig[1], sigma_depth=sig[2])


def same(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


@pytest.mark.parametrize("W,H", [(1, 1), (33, 17), (40, 24), (130, 70)])
def test_guided_equals_host(rtw, gpu_world, W, H):
    import torch
    A, L = rtw._abi, rtw.lib()
    n = W * H
    acc, mom, alb, nd = G.filter_inputs(W, H, seed=W)
    d_acc, d_mom, d_alb, d_nd = upload(acc), upload(mom), upload(alb), upload(nd)
    host = D.host_world()
    blank = np.full((n, 4), -1.0, np.float32)
    for cfg in CONFIGS:
        p = A.denoise_guided_params(**keywords(cfg))
        want, wvar = G.guided(host, acc, mom, alb, nd, W, H, **keywords(cfg))
        d_out, d_var = upload(blank), upload(blank[:, 0])
        A.check(L.rtw_denoise_guided_device(gpu_world.handle, W, H, d_acc.data_ptr(), d_mom.data_ptr(),
                                            d_alb.data_ptr() if cfg[1] else None, d_nd.data_ptr(), C.byref(p),
                                            d_out.data_ptr(), d_var.data_ptr(), None, 0), "rtw_denoise_guided_device")
        assert same(body(d_out, (n, 4)), want) and same(body(d_var, (n,)), wvar), cfg
        # without variance_out: the same colour
        d_out2 = upload(blank)
        A.check(L.rtw_denoise_guided_device(gpu_world.handle, W, H, d_acc.data_ptr(), d_mom.data_ptr(),
                                            d_alb.data_ptr() if cfg[1] else None, d_nd.data_ptr(), C.byref(p),
                                            d_out2.data_ptr(), None, None, 0), "rtw_denoise_guided_device")
        assert same(body(d_out2, (n, 4)), want), cfg
    for t, a in ((d_acc, acc), (d_mom, mom), (d_alb, alb), (d_nd, nd)):
        assert same(body(t, a.shape), a)                                    # the inputs and their guard words
    # in place on a caller's stream without a sync, then the host-buffer entry point of the GPU context
    cfg = CONFIGS[1]
    want, wvar = G.guided(host, acc, mom, alb, nd, W, H, **keywords(cfg))
    buf, d_var = upload(acc), upload(blank[:, 0])
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    A.check(L.rtw_denoise_guided_device(gpu_world.handle, W, H, buf.data_ptr(), d_mom.data_ptr(), d_alb.data_ptr(),
                                        d_nd.data_ptr(), C.byref(A.denoise_guided_params(**keywords(cfg))), buf.data_ptr(),
                                        d_var.data_ptr(), C.c_void_p(stream.cuda_stream), A.RTW_RENDER_NO_SYNC),
            "rtw_denoise_guided_device")
    stream.synchronize()
    assert same(body(buf, (n, 4)), want) and same(body(d_var, (n,)), wvar)
    got, gvar = G.guided(gpu_world, acc, mom, alb, nd, W, H, **keywords(cfg))
    assert same(got, want) and same(gvar, wvar)
    assert same(G.guided(gpu_world, acc, mom, None, nd, W, H, variance=False, **keywords(CONFIGS[3])),
                G.guided(host, acc, mom, None, nd, W, H, variance=False, **keywords(CONFIGS[3])))
    # rtw_denoise on the same context afterwards: the shared planes serve it unchanged
    assert same(gpu_world.denoise(acc, (alb, nd), W, H, passes=5, demodulate=True),
                host.denoise(acc, (alb, nd), W, H, passes=5, demodulate=True))


def test_refusals_on_a_gpu_context(rtw, gpu_world):
    import torch
    A, L = rtw._abi, rtw.lib()
    W, H = 8, 6
    acc, mom, alb, nd = G.filter_inputs(W, H)
    d_acc, d_mom, d_alb, d_nd = upload(acc), upload(mom), upload(alb), upload(nd)
    d_out = upload(np.full((W * H, 4), 7.0, np.float32))
    d_var = upload(np.full(W * H, 7.0, np.float32))

    def call(p, moments=d_mom.data_ptr(), albedo=d_alb.data_ptr(), flags=0):
        return L.rtw_denoise_guided_device(gpu_world.handle, W, H, d_acc.data_ptr(), moments, albedo, d_nd.data_ptr(),
                                           C.byref(p), d_out.data_ptr(), d_var.data_ptr(), None, flags)
    for kw in (dict(passes=0), dict(passes=9), dict(sigma_color=-1.0), dict(flags=2)):
        assert call(A.denoise_guided_params(**kw)) == A.RTW_E_INVALID, kw
    good = A.denoise_guided_params(passes=2)
    assert call(good, flags=2) == A.RTW_E_INVALID
    assert call(good, moments=None) == A.RTW_E_INVALID
    assert call(A.denoise_guided_params(demodulate=True), albedo=None) == A.RTW_E_INVALID
    torch.cuda.synchronize()
    assert (body(d_out, (W * H, 4)) == 7.0).all() and (body(d_var, (W * H,)) == 7.0).all()


def test_render_moments_estimate_filter_end_to_end(rtw):
    """Cornell 48 x 48: four 2-spp renders with the moments updated after each, the estimate and the guided filter with
    the shipped defaults -- the GPU context's calls give the host context's bits."""
    arr = rtw.flatten(rtw.worlds.cornell_box())
    cam = rtw.cornell_camera(image_width=48, spp=8).init()
    outs = []
    for device in (0, D.CPU):
        world = rtw.World(arr, device=device)
        accs = G.render_batches(rtw, world, cam, (2, 2, 2, 2), 11)
        mom = G.fold(world, accs, 48, 48)
        err, tiles, s = world.noise_estimate(mom, 48, 48, threshold=0.1, floor=0.01)
        out, var = world.denoise_guided(accs[-1], mom, world.render_guides(cam), 48, 48, variance=True)
        outs.append((accs[-1], mom, err, tiles, bytes(s), out, var))
        world.close()
    for g, h in zip(*outs):
        assert same(g, h) if isinstance(g, np.ndarray) else g == h
    acc, mom, err, tiles, _, out, var = outs[0]
    assert (mom[1, :, 2] == 4).all() and np.isfinite(err).all() and tiles.shape == (6, 6)
    assert np.isfinite(out).all() and not np.array_equal(out, acc) and (var >= 0).all()
