"""Ray queries on the GPU: query_closest_kernel / query_any_kernel give the host backend's records bit for bit, for
every case of tests/test_query.py (tests/query_scenes.py CASES), through the host-buffer and the device entry points;
on a caller's stream; for ray counts around a wave and a block, with the words past the last ray untouched; and
through the torch wrappers."""
import ctypes as C

import numpy as np
import pytest

import query_scenes as Q

pytestmark = pytest.mark.gpu
NONE = 0xFFFFFFFF


def words(a):
    """A record array as its 4-byte words (bit for bit comparisons: NaNs, signed zeros)."""
    return np.ascontiguousarray(a).view(np.uint32).reshape(len(a), -1)


def ray_tensor(rays):
    import torch
    return torch.from_numpy(np.ascontiguousarray(rays).view(np.float32).reshape(-1, 8).copy()).cuda()


def hit_array(t):
    return np.ascontiguousarray(t.cpu().numpy()).view(Q.pkgs()[0]._abi.HIT_DTYPE).reshape(-1)


@pytest.mark.parametrize("name", Q.CASES)
def test_records_equal_host(rtw, name):
    """Both query kinds, the host-buffer entry points of the GPU context and the device entry points.  Degenerate
    rays give unspecified records: there the other rays are compared."""
    import torch
    scene, rays = Q.case(name)
    want, want_occ = Q.host(name)
    keep = ~Q.degenerate(rays)[1] if name == "degenerate" else np.ones(len(rays), bool)
    w = Q.world(scene, device=0)
    got, got_occ = w.trace(rays), w.occluded(rays)
    d_rays = ray_tensor(rays)
    d_hits = torch.full((len(rays), 16), 0x55555555, dtype=torch.int32, device="cuda")
    d_occ = torch.full((len(rays),), 7, dtype=torch.uint8, device="cuda")
    L = rtw.lib()
    rtw._abi.check(L.rtw_trace_rays_device(w.handle, len(rays), d_rays.data_ptr(), d_hits.data_ptr(), None, 0),
                   "rtw_trace_rays_device")
    rtw._abi.check(L.rtw_occluded_device(w.handle, len(rays), d_rays.data_ptr(), d_occ.data_ptr(), None, 0),
                   "rtw_occluded_device")
    w.close()
    assert np.array_equal(words(got)[keep], words(want)[keep]) and np.array_equal(got_occ[keep], want_occ[keep])
    assert np.array_equal(words(hit_array(d_hits))[keep], words(want)[keep])
    assert np.array_equal(d_occ.cpu().numpy()[keep] == 1, want_occ[keep])
    assert set(np.unique(d_occ.cpu().numpy())) <= {0, 1}


@pytest.fixture(scope="module")
def cornell(rtw):
    w = Q.world("cornell_tree", device=0)
    yield w
    w.close()


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, 4096])
def test_partial_waves_and_blocks_write_nothing_past_n(rtw, cornell, n):
    """One record and one byte past n are pre-filled and come back untouched."""
    import torch
    _, rays = Q.case("cornell_tree")
    want, want_occ = Q.host("cornell_tree")
    d_rays = ray_tensor(rays)                       # all 4096 rays are readable; only n are traced
    d_hits = torch.full((n + 1, 16), 0x55555555, dtype=torch.int32, device="cuda")
    d_occ = torch.full((n + 1,), 7, dtype=torch.uint8, device="cuda")
    L = rtw.lib()
    rtw._abi.check(L.rtw_trace_rays_device(cornell.handle, n, d_rays.data_ptr(), d_hits.data_ptr(), None, 0),
                   "rtw_trace_rays_device")
    rtw._abi.check(L.rtw_occluded_device(cornell.handle, n, d_rays.data_ptr(), d_occ.data_ptr(), None, 0),
                   "rtw_occluded_device")
    hits, occ = d_hits.cpu().numpy(), d_occ.cpu().numpy()
    assert np.array_equal(words(hit_array(d_hits[:n])), words(want[:n])) and np.array_equal(occ[:n] == 1, want_occ[:n])
    assert (hits[n] == 0x55555555).all() and occ[n] == 7


def test_on_a_callers_stream(rtw, cornell):
    import torch
    _, rays = Q.case("cornell_tree")
    want, want_occ = Q.host("cornell_tree")
    d_rays = ray_tensor(rays)
    d_hits = torch.full((len(rays), 16), 0x55555555, dtype=torch.int32, device="cuda")
    d_occ = torch.full((len(rays),), 7, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    L, A = rtw.lib(), rtw._abi
    sp = C.c_void_p(stream.cuda_stream)
    A.check(L.rtw_trace_rays_device(cornell.handle, len(rays), d_rays.data_ptr(), d_hits.data_ptr(), sp,
                                    A.RTW_RENDER_NO_SYNC), "rtw_trace_rays_device")
    A.check(L.rtw_occluded_device(cornell.handle, len(rays), d_rays.data_ptr(), d_occ.data_ptr(), sp,
                                  A.RTW_RENDER_NO_SYNC), "rtw_occluded_device")
    stream.synchronize()
    assert np.array_equal(words(hit_array(d_hits)), words(want)) and np.array_equal(d_occ.cpu().numpy() == 1, want_occ)
    # a call on the context's own stream is ordered after them
    assert np.array_equal(words(cornell.trace(rays)), words(want))


def test_torch_wrappers(rtw, cornell):
    import torch
    A = rtw._abi
    _, rays = Q.case("cornell_tree")
    want, want_occ = Q.host("cornell_tree")
    o = torch.from_numpy(rays["origin"].copy()).cuda()
    d = torch.from_numpy(rays["dir"].copy()).cuda()
    rows = rtw.ray_rows(o, d, tmax=torch.from_numpy(rays["tmax"].copy()).cuda(), time=0.0)
    assert np.array_equal(rows.cpu().numpy().view(np.uint32), words(rays))
    hits = cornell.trace_device(rows)
    occ = cornell.occluded_device(rows)
    assert hits.shape == (len(rays), 16) and hits.dtype == torch.int32 and occ.dtype == torch.uint8
    assert np.array_equal(words(hit_array(hits)), words(want)) and np.array_equal(occ.cpu().numpy() == 1, want_occ)
    cols = rtw.hit_columns(hits)
    assert np.array_equal(cols["hit"].cpu().numpy(), want["kind"] != NONE)
    for f in ("t", "p", "normal", "uv"):
        assert cols[f].dtype == torch.float32
        assert np.array_equal(cols[f].cpu().numpy().view(np.uint32), np.ascontiguousarray(want[f]).view(np.uint32)), f
    for f in ("kind", "index", "member", "material", "front", "prim_kind", "prim_index"):
        assert np.array_equal(cols[f].cpu().numpy().view(np.uint32), want[f]), f
    # into the caller's tensors, on the caller's stream
    out_h = torch.zeros((len(rays), 16), dtype=torch.int32, device="cuda")
    out_o = torch.zeros((len(rays),), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    assert cornell.trace_device(rows, out_h, stream=stream) is out_h
    assert cornell.occluded_device(rows, out_o, stream=stream) is out_o
    stream.synchronize()
    assert torch.equal(out_h, hits) and torch.equal(out_o, occ)
    # nothing to do; and what the wrappers refuse
    assert cornell.trace_device(rows[:0]).shape == (0, 16) and cornell.occluded_device(rows[:0]).shape == (0,)
    with pytest.raises(ValueError):
        cornell.trace_device(rows.cpu())
    with pytest.raises(ValueError):
        cornell.trace_device(rows[:, :7])
    with pytest.raises(ValueError):
        cornell.trace_device(rows, torch.zeros((len(rays), 16), dtype=torch.float32, device="cuda"))


def test_refusals_on_a_gpu_context(rtw, cornell):
    import torch
    A, L = rtw._abi, rtw.lib()
    _, rays = Q.case("cornell_tree")
    d_rays = ray_tensor(rays[:8])
    d_hits = torch.full((8, 16), 0x55555555, dtype=torch.int32, device="cuda")
    d_occ = torch.full((8,), 7, dtype=torch.uint8, device="cuda")
    assert L.rtw_trace_rays_device(cornell.handle, 0, None, None, None, 0) == A.RTW_OK
    assert L.rtw_occluded_device(cornell.handle, 0, d_rays.data_ptr(), d_occ.data_ptr(), None, 0) == A.RTW_OK
    for rc in (L.rtw_trace_rays_device(cornell.handle, 8, None, d_hits.data_ptr(), None, 0),
               L.rtw_trace_rays_device(cornell.handle, 8, d_rays.data_ptr(), None, None, 0),
               L.rtw_trace_rays_device(cornell.handle, 8, d_rays.data_ptr(), d_hits.data_ptr(), None, 2),
               L.rtw_trace_rays_device(cornell.handle, 1 << 32, d_rays.data_ptr(), d_hits.data_ptr(), None, 0),
               L.rtw_trace_rays_device(None, 8, d_rays.data_ptr(), d_hits.data_ptr(), None, 0),
               L.rtw_trace_rays_device(cornell.handle, 7, d_rays.data_ptr() + 4, d_hits.data_ptr(), None, 0),   # not
               L.rtw_trace_rays_device(cornell.handle, 7, d_rays.data_ptr(), d_hits.data_ptr() + 8, None, 0),   # 16-byte
               L.rtw_occluded_device(cornell.handle, 7, d_rays.data_ptr() + 4, d_occ.data_ptr(), None, 0),      # aligned
               L.rtw_occluded_device(cornell.handle, 8, None, d_occ.data_ptr(), None, 0),
               L.rtw_occluded_device(cornell.handle, 8, d_rays.data_ptr(), None, None, 0),
               L.rtw_occluded_device(cornell.handle, 8, d_rays.data_ptr(), d_occ.data_ptr(), None, 4)):
        assert rc == A.RTW_E_INVALID
    torch.cuda.synchronize()
    assert (d_hits.cpu().numpy() == 0x55555555).all() and (d_occ.cpu().numpy() == 7).all()
