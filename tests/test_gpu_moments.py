"""Noise estimates on the GPU: rtw_moments_update and rtw_noise_estimate give the host backend's bits -- three
updates with unequal batches and the estimate's err, tile_max and summary, at 1 x 1, 33 x 17 (partial blocks and
partial 8 x 8 tiles), 40 x 24 and 130 x 70 (several blocks in both directions), through the device and the host-buffer
entry points, on a caller's stream, with the words past the arrays' ends untouched; refusals on a GPU context."""
import ctypes as C

import numpy as np
import pytest

import denoise_scenes as D
import guided_scenes as G

pytestmark = pytest.mark.gpu
PAD = 64                      # guard words behind every device array
SIZES = [(1, 1), (33, 17), (40, 24), (130, 70)]


@pytest.fixture(scope="module")
def gpu_world(rtw):
    w = rtw.World(rtw.flatten(rtw.worlds.two_spheres_world()), device=0)
    yield w
    w.close()


def padded(words, fill=-3.0):
    import torch
    return torch.full((words + PAD,), fill, dtype=torch.float32, device="cuda")


def upload(a):
    """A device copy of `a` followed by PAD guard words."""
    import torch
    t = padded(a.size)
    t[:a.size] = torch.from_numpy(np.ascontiguousarray(a).reshape(-1)).cuda()
    return t


def body(t, shape):
    n = int(np.prod(shape))
    host = t.cpu().numpy()
    assert (host[n:] == -3.0).all(), "words past the array's end were written"
    return host[:n].reshape(shape)


@pytest.mark.parametrize("W,H", SIZES)
def test_moments_and_estimate_equal_host(rtw, gpu_world, W, H):
    import torch
    A, L = rtw._abi, rtw.lib()
    n = W * H
    seq = G.accumulator_sequence(W, H, seed=W, batches=(1, 3, 2))
    host = D.host_world()
    want = np.zeros((2, n, 4), np.float32)
    d_mom = upload(want)
    via_host_buffers = want.copy()
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    for j, acc in enumerate(seq):
        host.moments_update(acc, want, W, H)
        d_acc = upload(acc)
        torch.cuda.synchronize()
        # the second update on a caller's stream without a sync, the others on the context's
        s, flags = (C.c_void_p(stream.cuda_stream), A.RTW_RENDER_NO_SYNC) if j == 1 else (None, 0)
        A.check(L.rtw_moments_update_device(gpu_world.handle, W, H, d_acc.data_ptr(), d_mom.data_ptr(), s, flags),
                "rtw_moments_update_device")
        stream.synchronize()
        assert np.array_equal(body(d_mom, (2, n, 4)).view(np.uint32), want.view(np.uint32)), j
        body(d_acc, (n, 4))
        gpu_world.moments_update(acc, via_host_buffers, W, H)
        assert np.array_equal(via_host_buffers.view(np.uint32), want.view(np.uint32)), j
    th, tw = (H + 7) // 8, (W + 7) // 8
    for floor, thr in ((0.01, 0.05), (0.0, 0.3)):
        err, tiles, summ = host.noise_estimate(want, W, H, threshold=thr, floor=floor)
        d_err, d_tiles, d_sum = padded(n), padded(th * tw), padded(6)
        A.check(L.rtw_noise_estimate_device(gpu_world.handle, W, H, d_mom.data_ptr(), floor, thr, d_err.data_ptr(),
                                            d_tiles.data_ptr(), d_sum.data_ptr(), None, 0), "rtw_noise_estimate_device")
        assert np.array_equal(body(d_err, (n,)).view(np.uint32), err.view(np.uint32))
        assert np.array_equal(body(d_tiles, (th, tw)).view(np.uint32), tiles.view(np.uint32))
        got = A.RtwNoiseSummary.from_buffer_copy(body(d_sum, (6,)).tobytes())
        assert (got.over, got.known, got.max_err) == (summ.over, summ.known, summ.max_err)
        # without the optional outputs, on a caller's stream
        d_sum2 = padded(6)
        torch.cuda.synchronize()
        A.check(L.rtw_noise_estimate_device(gpu_world.handle, W, H, d_mom.data_ptr(), floor, thr, None, None,
                                            d_sum2.data_ptr(), C.c_void_p(stream.cuda_stream), A.RTW_RENDER_NO_SYNC),
                "rtw_noise_estimate_device")
        stream.synchronize()
        assert body(d_sum2, (6,)).tobytes() == body(d_sum, (6,)).tobytes()
        e2, t2, s2 = gpu_world.noise_estimate(want, W, H, threshold=thr, floor=floor)
        assert np.array_equal(e2.view(np.uint32), err.view(np.uint32)) and np.array_equal(t2, tiles)
        assert bytes(s2) == bytes(summ)
    if n > 4:
        assert 0 < summ.known < n and np.isinf(tiles).any() and summ.max_err > 0


def test_refusals_on_a_gpu_context(rtw, gpu_world):
    import torch
    A, L = rtw._abi, rtw.lib()
    W, H = 8, 6
    seq = G.accumulator_sequence(W, H, batches=(1, 2))
    d_acc = upload(seq[0])
    d_mom = padded(8 * W * H, 0.0)
    d_err, d_sum = padded(W * H, 7.0), padded(6, 7.0)
    h = gpu_world.handle
    assert L.rtw_moments_update_device(h, W, H, None, d_mom.data_ptr(), None, 0) == A.RTW_E_INVALID
    assert L.rtw_moments_update_device(h, W, H, d_acc.data_ptr(), None, None, 0) == A.RTW_E_INVALID
    assert L.rtw_moments_update_device(h, 0, H, d_acc.data_ptr(), d_mom.data_ptr(), None, 0) == A.RTW_E_INVALID
    assert L.rtw_moments_update_device(h, W, H, d_acc.data_ptr(), d_mom.data_ptr(), None, 2) == A.RTW_E_INVALID
    for floor, thr, flags in ((-1.0, 0.05, 0), (0.01, float("nan"), 0), (float("inf"), 0.05, 0), (0.01, 0.05, 4)):
        assert L.rtw_noise_estimate_device(h, W, H, d_mom.data_ptr(), floor, thr, d_err.data_ptr(), None,
                                           d_sum.data_ptr(), None, flags) == A.RTW_E_INVALID
    assert L.rtw_noise_estimate_device(h, W, H, None, 0.01, 0.05, d_err.data_ptr(), None, d_sum.data_ptr(), None,
                                       0) == A.RTW_E_INVALID
    assert L.rtw_noise_estimate_device(h, W, H, d_mom.data_ptr(), 0.01, 0.05, d_err.data_ptr(), None, None, None,
                                       0) == A.RTW_E_INVALID
    torch.cuda.synchronize()
    assert not d_mom.cpu().numpy()[:8 * W * H].any()
    assert (d_err.cpu().numpy()[:W * H] == 7.0).all() and (d_sum.cpu().numpy()[:6] == 7.0).all()
