"""Temporal reprojection on the GPU: rtw_temporal_accumulate_device gives the host backend's bits for the
accumulator, the moments and the history -- a still, a translated and a panned camera at 1 x 1, 33 x 17 (partial
blocks) and 130 x 70, with and without moments and history_out, in place, on a caller's stream, with the words past
every array's end untouched, and through the host-buffer entry point of the GPU context; refusals on a GPU context;
RayTraceState.move_camera on device 0 against the host context."""
import ctypes as C

import numpy as np
import pytest

import temporal_scenes as T

pytestmark = pytest.mark.gpu
PAD = 64                      # guard words behind every device array
SIZES = [(1, 1), (33, 17), (130, 70)]
KINDS = ["still", "translated", "panned"]


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


def body(t, shape, fill=-3.0):
    n = int(np.prod(shape))
    host = t.cpu().numpy()
    assert (host[n:] == fill).all(), "words past the array's end were written"
    return host[:n].reshape(shape)


def same(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("W,H", SIZES)
def test_device_equals_host(rtw, gpu_world, W, H, kind):
    import torch
    A, L = rtw._abi, rtw.lib()
    n = W * H
    cc, pc, cur, cnd, prev, pnd, mom = T.synthetic_frames(rtw, W, H, kind)
    host = T.D.host_world()
    p = A.temporal_params(max_history=6.0)
    want, want_m, want_h = host.temporal_accumulate(cc, pc, cur, cnd, prev, pnd, mom, max_history=6.0)
    plain, none, plain_h = host.temporal_accumulate(cc, pc, cur, cnd, prev, pnd, max_history=6.0)
    assert none is None and same(plain, want) and same(plain_h, want_h)
    if n > 4:
        assert (want_h > 0).any()
    d = {k: upload(v) for k, v in (("cur", cur), ("cnd", cnd), ("prev", prev), ("pnd", pnd), ("mom", mom))}
    d_out, d_om, d_h = padded(4 * n), padded(8 * n), padded(n)
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()

    def run(out, om, hist, s=None, flags=0, pm=True):
        A.check(L.rtw_temporal_accumulate_device(
            gpu_world.handle, C.byref(cc.derived), C.byref(pc.derived), d["cur"].data_ptr(), d["cnd"].data_ptr(),
            d["prev"].data_ptr(), d["pnd"].data_ptr(), d["mom"].data_ptr() if pm else None, C.byref(p), out.data_ptr(),
            om.data_ptr() if om is not None else None, hist.data_ptr() if hist is not None else None, s, flags),
            "rtw_temporal_accumulate_device")
    # with moments and history, on the context's stream
    run(d_out, d_om, d_h)
    assert same(body(d_out, (n, 4)), want) and same(body(d_om, (2, n, 4)), want_m) and same(body(d_h, (n,)), want_h)
    # without either, on a caller's stream without a sync
    d_out2 = padded(4 * n)
    torch.cuda.synchronize()
    run(d_out2, None, None, C.c_void_p(stream.cuda_stream), A.RTW_RENDER_NO_SYNC, pm=False)
    stream.synchronize()
    assert same(body(d_out2, (n, 4)), want)
    # in place on cur_accum, the same way
    d_om2 = padded(8 * n)
    torch.cuda.synchronize()
    run(d["cur"], d_om2, None, C.c_void_p(stream.cuda_stream), A.RTW_RENDER_NO_SYNC)
    stream.synchronize()
    assert same(body(d["cur"], (n, 4)), want) and same(body(d_om2, (2, n, 4)), want_m)
    for k in ("cnd", "prev", "pnd"):
        assert same(body(d[k], (n, 4)), {"cnd": cnd, "prev": prev, "pnd": pnd}[k])
    assert same(body(d["mom"], (2, n, 4)), mom)
    # the host-buffer entry point of the GPU context, out of place and in place
    got, got_m, got_h = gpu_world.temporal_accumulate(cc, pc, cur, cnd, prev, pnd, mom, max_history=6.0)
    assert same(got, want) and same(got_m, want_m) and same(got_h, want_h)
    cur2 = cur.copy()
    got2, none2, got_h2 = gpu_world.temporal_accumulate(cc, pc, cur2, cnd, prev, pnd, out=cur2, max_history=6.0)
    assert got2 is cur2 and none2 is None and same(cur2, want) and same(got_h2, want_h)


def test_torch_entry_point(rtw, gpu_world):
    import torch
    W, H = 33, 17
    cc, pc, cur, cnd, prev, pnd, mom = T.synthetic_frames(rtw, W, H, "translated")
    want, want_m, want_h = T.D.host_world().temporal_accumulate(cc, pc, cur, cnd, prev, pnd, mom)
    t = [torch.from_numpy(x).cuda() for x in (cur, cnd, prev, pnd, mom)]
    out, m, h = gpu_world.temporal_accumulate_device(cc, pc, *t)
    assert same(out.cpu().numpy(), want) and same(m.cpu().numpy(), want_m) and same(h.cpu().numpy(), want_h)
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    out2, none, h2 = gpu_world.temporal_accumulate_device(cc, pc, *t[:4], stream=s)
    s.synchronize()
    assert none is None and same(out2.cpu().numpy(), want) and same(h2.cpu().numpy(), want_h)
    with pytest.raises(ValueError):
        gpu_world.temporal_accumulate_device(cc, pc, t[0].cpu(), *t[1:4])


def test_refusals_on_a_gpu_context(rtw, gpu_world):
    import torch
    A, L = rtw._abi, rtw.lib()
    W, H = 9, 5
    n = W * H
    cc, pc, cur, cnd, prev, pnd, mom = T.synthetic_frames(rtw, W, H, "translated")
    other = T.frame_camera(rtw, (0, 0, 0), (0, 0, -3), W=W + 1, H=H)
    d = {k: upload(v) for k, v in (("cur", cur), ("cnd", cnd), ("prev", prev), ("pnd", pnd), ("mom", mom))}
    d_out, d_om, d_h = padded(4 * n, 7.0), padded(8 * n, 7.0), padded(n, 7.0)
    good = A.temporal_params()
    bad = A.temporal_params()
    bad.max_history = float("nan")
    flagged = A.temporal_params()
    flagged.flags = 2
    base = dict(cc=cc, pc=pc, cur=d["cur"], cnd=d["cnd"], prev=d["prev"], pnd=d["pnd"], pm=d["mom"], p=good, out=d_out,
                om=d_om, hist=d_h, flags=0)
    cases = {"sizes": dict(pc=other), "null cur": dict(cur=None), "null prev_nd": dict(pnd=None), "null out": dict(out=None),
             "null params": dict(p=None), "one moments pointer": dict(om=None), "the other": dict(pm=None),
             "nan": dict(p=bad), "params flags": dict(p=flagged), "call flags": dict(flags=4),
             "out is prev": dict(out=d["prev"]), "moments onto prev_nd": dict(om=d["pnd"]), "null camera": dict(cc=None)}
    for name, kw in cases.items():
        a = {**base, **kw}
        ptr = (lambda t: t.data_ptr() if t is not None else None)
        cam = (lambda c: C.byref(c.derived) if c is not None else None)
        rc = L.rtw_temporal_accumulate_device(gpu_world.handle, cam(a["cc"]), cam(a["pc"]), ptr(a["cur"]), ptr(a["cnd"]),
                                              ptr(a["prev"]), ptr(a["pnd"]), ptr(a["pm"]),
                                              C.byref(a["p"]) if a["p"] is not None else None, ptr(a["out"]), ptr(a["om"]),
                                              ptr(a["hist"]), None, a["flags"])
        assert rc == A.RTW_E_INVALID, name
    torch.cuda.synchronize()
    for t, words in ((d_out, 4 * n), (d_om, 8 * n), (d_h, n)):
        assert (t.cpu().numpy() == 7.0).all()
    assert same(body(d["prev"], (n, 4)), prev) and same(body(d["pnd"], (n, 4)), pnd)
    # and the host-buffer form of the GPU context
    out = np.full((n, 4), 7, np.float32)
    rc = L.rtw_temporal_accumulate(gpu_world.handle, C.byref(cc.derived), C.byref(other.derived), cur.ctypes.data,
                                   cnd.ctypes.data, prev.ctypes.data, pnd.ctypes.data, None, C.byref(good),
                                   out.ctypes.data, None, None)
    assert rc == A.RTW_E_INVALID and (out == 7).all()


def test_move_camera_equals_host(rtw):
    W = H = 40
    cams = T.orbit(rtw, 4, W, step_deg=2.0)
    arr = rtw.flatten(rtw.worlds.cornell_box())
    results = []
    for device in (0, T.CPU):
        world = rtw.World(arr, device=device)
        state = rtw.RayTraceState(camera=cams[0], writer=rtw.SharedStateImageWriter(W, H), world=world, seed=3)
        cams[0].render_range(state, 0, cams[0].size, 0, 2)
        state.update_moments()
        hists = [state.move_camera(cam, 2) for cam in cams[1:]]
        results.append((state.writer.buffer.copy(), state.moments.copy(), hists))
        world.close()
    (b0, m0, h0), (b1, m1, h1) = results
    assert same(b0, b1) and same(m0, m1) and all(same(x, y) for x, y in zip(h0, h1))
    assert (h0[-1] > 0).sum() > 0.8 * W * H
