"""Temporal reprojection (rtw_temporal_accumulate, rtw_debug_reproject; include/rtw_gpu.h "Temporal reprojection") on
the host backend: the projection against a float64 restatement, and what a caller relies on -- a still camera adds
exactly, an integer shift copies, a hidden point takes no history, the sky reprojects by direction, the cap, the
moments, degenerate inputs, every refusal, and that it is worth having.  No GPU."""
import ctypes as C

import numpy as np
import pytest

import guided_scenes as G
import temporal_scenes as T

F = np.float32
SNAP = 2.0 ** -6
# The largest deviation of rtw_debug_reproject from the float64 restatement over the five cameras, points and
# directions, as test_projection prints it: 1.25e-3 pixel (Book-1's camera 4096 wide; DESIGN.md §Temporal
# reprojection).  The projection's tolerance is 4 x that -- and below the snap radius, which must be >= 4 x it too.
MEASURED_ROUND_OFF = 1.26e-3
PARITY = 1e-5   # the project's parity tolerance: |got - ref| / max(1, |ref|)


def rel(got, ref):
    return np.abs(got.astype(np.float64) - ref) / np.maximum(1.0, np.abs(ref))


def call(rtw, world, cc, pc, cur, cnd, prev, pnd, pm, params, out, om, hist):
    """rtw_temporal_accumulate with raw arguments (None: a null pointer); returns the code."""
    def p(a):
        return a.ctypes.data if a is not None else None
    cam = (lambda c: C.byref(c.derived) if hasattr(c, "derived") else (C.byref(c) if c is not None else None))
    return rtw.lib().rtw_temporal_accumulate(world.handle if world is not None else None, cam(cc), cam(pc), p(cur), p(cnd),
                                             p(prev), p(pnd), p(pm), C.byref(params) if params is not None else None,
                                             p(out), p(om), p(hist))


def reference_still(cur, prev, m1, max_history):
    """A whole call in float32 for a still camera whose every pixel reprojects onto itself with valid geometry: per
    pixel, the header's blend and moments with the one tap of weight 1.  -> (out, plane 1)."""
    with np.errstate(all="ignore"):
        pv = np.isfinite(prev).all(1) & (prev[:, 3] > 0)
        inv = F(1) / prev[:, 3]
        mean = np.where(pv[:, None], prev[:, :3] * inv[:, None], F(0)).astype(F)
        hi = np.where(pv, prev[:, 3], F(0)).astype(F)
        h = np.minimum(hi, F(max_history))
        ck = np.isfinite(cur).all(1) & (cur[:, 3] > 0)
        both = np.concatenate([mean * h[:, None] + cur[:, :3], (h + cur[:, 3])[:, None]], 1)
        only = np.concatenate([mean * h[:, None], h[:, None]], 1)
        out = np.where((h > 0)[:, None], np.where(ck[:, None], both, only), np.where(ck[:, None], cur, F(0))).astype(F)
        m = np.where((pv & (m1[:, 2] >= 1))[:, None], m1, F(0)).astype(F)
        m[:, 3] = np.where(hi > F(max_history), m[:, 3] * (h / hi), m[:, 3])
        a = np.where(ck[:, None], cur, F(0)).astype(F)       # a batch that does not advance changes nothing
        west = G.moments_update(a, np.stack([np.zeros_like(a), m]), F)[1]
    return out, west


# ---------------------------------------------------------------- projection
@pytest.mark.parametrize("k", range(5))
def test_projection(rtw, k):
    name, cam = T.projection_cameras(rtw)[k]
    pts, dirs, xs, ys = T.centre_points(cam)
    c = np.array(cam.derived.center[:], np.float64)
    assert 4 * MEASURED_ROUND_OFF <= SNAP == rtw._abi.RTW_TEMPORAL_SNAP <= 2.0 ** -4
    for form, src, e in (("points", pts, pts.astype(np.float64) - c), ("dirs", dirs, dirs.astype(np.float64))):
        xy, ok = T.reproject(rtw, cam, **{form: src})
        fx, fy, ok64 = T.project64(cam.derived, e)
        dev = max(np.abs(xy[:, 0] - fx).max(), np.abs(xy[:, 1] - fy).max())
        own = max(np.abs(xy[:, 0] - xs).max(), np.abs(xy[:, 1] - ys).max())
        print(f"{name} {form}: largest deviation from float64 {dev:.3g} pixel, from the own centre {own:.3g}")
        assert ok.all() and ok64.all()
        assert dev <= 4 * MEASURED_ROUND_OFF
        assert own <= SNAP       # a camera reprojected onto itself
    # behind the camera: the mirrored points and directions
    for form, src in (("points", (2 * c - pts.astype(np.float64)).astype(F)), ("dirs", -dirs)):
        xy, ok = T.reproject(rtw, cam, **{form: src[::97]})
        assert not ok.any() and not xy.any()


def test_reproject_refusals(rtw):
    cam = rtw.cornell_camera(image_width=8).init()
    p = np.zeros((1, 3), F)
    xy, ok = np.zeros(2, F), np.zeros(1, np.uint8)
    L = rtw.lib()
    assert L.rtw_debug_reproject(C.byref(cam.derived), 1, p.ctypes.data, p.ctypes.data, xy.ctypes.data, ok.ctypes.data) == -1
    assert L.rtw_debug_reproject(C.byref(cam.derived), 1, None, None, xy.ctypes.data, ok.ctypes.data) == -1
    assert L.rtw_debug_reproject(None, 1, p.ctypes.data, None, xy.ctypes.data, ok.ctypes.data) == -1


# ---------------------------------------------------------------- still camera
@pytest.mark.parametrize("scene", ["sky", "disocclusion"])
def test_still_camera_adds_exactly(rtw, scene):
    world, cam, _ = T.host_world(scene)
    nd = world.render_guides(cam)[1]
    A, B = T.render(world, cam, 4, 1), T.render(world, cam, 2, 2)
    out, mom, hist = world.temporal_accumulate(cam, cam, B, nd, A, nd, max_history=64.0)
    assert mom is None
    assert (hist == 4).all() and (out[:, 3] == 6).all()
    assert rel(out[:, :3], A[:, :3].astype(np.float64) + B[:, :3]).max() <= PARITY


def test_still_camera_4096_wide_snaps(rtw):
    """Every pixel of a 4096-wide frame lands within the snap radius of itself: the history is copied, not spread."""
    world = T.D.host_world()
    cam = rtw.Camera(aspect_ratio=4096 / 6, image_width=4096, image_height=6, vfov=2.0, lookfrom=(13.0, 2.0, 3.0),
                     lookat=(0.0, 0.0, 0.0), defocus_angle=0.0, focus_dist=10.0).init()
    n = cam.size
    rng = np.random.default_rng(3)
    nd = np.concatenate([np.tile([0.0, 1.0, 0.0], (n, 1)), 5 + 10 * rng.random((n, 1))], 1).astype(F)
    w = rng.integers(1, 30, n).astype(F)
    A = np.concatenate([rng.random((n, 3)).astype(F) * w[:, None], w[:, None]], 1).astype(F)
    B = np.zeros((n, 4), F)
    out, _, hist = world.temporal_accumulate(cam, cam, B, nd, A, nd, max_history=64.0)
    assert np.array_equal(hist, w)
    assert rel(out[:, :3], A[:, :3].astype(np.float64)).max() <= PARITY


# ---------------------------------------------------------------- integer shift
def test_integer_shift_copies(rtw):
    world, prev, cur = T.host_world("shift")
    W, H = 64, 48
    pnd, cnd = world.render_guides(prev)[1], world.render_guides(cur)[1]
    assert (pnd[:, 3] > 0).all() and (cnd[:, 3] > 0).all()
    A, B = T.render(world, prev, 4, 1), T.render(world, cur, 2, 2)
    # where the float64 restatement sends the current pixels: 3 columns over, to within the snap radius
    p, _, _ = T.first_hits64(cur, cnd)
    fx, fy, ok = T.project64(prev.derived, p - np.array(prev.derived.center[:], np.float64))
    xs, ys = np.tile(np.arange(W), H), np.repeat(np.arange(H), W)
    assert ok.all() and np.abs(fx - (xs + 3)).max() < SNAP / 4 and np.abs(fy - ys).max() < SNAP / 4
    zero = np.zeros_like(B)
    only, _, hist = world.temporal_accumulate(cur, prev, zero, cnd, A, pnd, max_history=64.0)
    out, _, hist2 = world.temporal_accumulate(cur, prev, B, cnd, A, pnd, max_history=64.0)
    assert np.array_equal(hist, hist2)
    A2, h2, only2 = A.reshape(H, W, 4), hist.reshape(H, W), only.reshape(H, W, 4)
    assert np.array_equal(h2[:, :W - 3], A2[:, 3:, 3])
    # the history's mean is the previous mean 3 columns over: (rgb (1 / w)) w against rgb, the still camera's
    # difference, so the still camera's tolerance
    assert rel(only2[:, :W - 3, :3], A2[:, 3:, :3].astype(np.float64)).max() <= PARITY
    assert (h2[:, W - 3:] == 0).all()
    assert np.array_equal(out.reshape(H, W, 4)[:, W - 3:].view(np.uint32), B.reshape(H, W, 4)[:, W - 3:].view(np.uint32))
    assert rel(out.reshape(H, W, 4)[:, :W - 3, :3], A2[:, 3:, :3].astype(np.float64) + B.reshape(H, W, 4)[:, :W - 3, :3]).max() <= PARITY


# ---------------------------------------------------------------- disocclusion
def edge_band(pnd, W, H, fx, fy, tol):
    """True where the 2 x 2 footprint at (fx, fy), grown by one pixel, touches a pixel of the previous frame that
    differs from one of its 8 neighbours in hit state or, relatively, in depth by more than tol."""
    d = pnd[:, 3].reshape(H, W).astype(np.float64)
    pad = np.pad(d, 1, mode="edge")
    edge = np.zeros((H, W), bool)
    for dy in range(3):
        for dx in range(3):
            q = pad[dy:dy + H, dx:dx + W]
            edge |= ((q > 0) != (d > 0)) | (np.abs(q - d) > tol * np.maximum(q, d))
    x0, y0 = np.floor(fx).astype(int), np.floor(fy).astype(int)
    band = np.zeros(len(fx), bool)
    for dy in range(-1, 3):
        for dx in range(-1, 3):
            band |= edge[np.clip(y0 + dy, 0, H - 1), np.clip(x0 + dx, 0, W - 1)]
    return band


def test_disocclusion(rtw):
    world, prev, cur = T.host_world("disocclusion")
    W, H, tol = 64, 48, 0.05
    pnd, cnd = world.render_guides(prev)[1], world.render_guides(cur)[1]
    A, B = T.render(world, prev, 4, 1), T.render(world, cur, 2, 2)
    _, _, hist = world.temporal_accumulate(cur, prev, B, cnd, A, pnd, depth_tolerance=tol)
    p, _, hit = T.first_hits64(cur, cnd)
    assert hit.all()
    cp = np.array(prev.derived.center[:], np.float64)
    e = p - cp
    t = world.trace(np.tile(cp, (len(e), 1)), e)["t"].astype(np.float64)     # in units of |e|: 1 reaches p
    occluded = t < 1 - tol
    assert occluded.sum() >= 8, "the scene hides nothing"
    assert (hist[occluded] == 0).all()
    fx, fy, ok = T.project64(prev.derived, e)
    inside = ok & (fx >= 0) & (fx <= W - 1) & (fy >= 0) & (fy <= H - 1)
    visible = np.abs(t - 1) <= 1e-3
    band = edge_band(pnd, W, H, fx, fy, tol)
    print(f"occluded {occluded.sum()}, visible and inside {(visible & inside).sum()}, of them in the edge band "
          f"{(visible & inside & band).sum()} of {W * H} pixels")
    assert (visible & inside & band).sum() <= 0.10 * W * H
    keep = visible & inside & ~band
    assert keep.sum() >= 0.7 * W * H
    assert (hist[keep] > 0).all()


# ---------------------------------------------------------------- sky
def test_sky_reprojects_by_direction(rtw):
    world, prev, cur = T.host_world("sky")
    W, H = 64, 48
    pnd, cnd = world.render_guides(prev)[1], world.render_guides(cur)[1]
    A, B = T.render(world, prev, 4, 1), T.render(world, cur, 2, 2)
    A = A.copy()
    prev_hit = pnd[:, 3] > 0
    A[prev_hit, :3] = 4e6                                   # a hit tap would show
    out, _, hist = world.temporal_accumulate(cur, prev, B, cnd, A, pnd)
    _, u, hit = T.first_hits64(cur, cnd)
    miss = ~hit
    assert miss.sum() > W * H // 4 and hit.sum() > W * H // 8
    fx, fy, ok = T.project64(prev.derived, u)
    x0, y0 = np.floor(fx).astype(int), np.floor(fy).astype(int)
    ph = prev_hit.reshape(H, W)
    n_on, n_sky = np.zeros(W * H, int), np.zeros(W * H, int)
    for dy in (0, 1):
        for dx in (0, 1):
            on = ok & (x0 + dx >= 0) & (x0 + dx < W) & (y0 + dy >= 0) & (y0 + dy < H)
            sky = on & ~ph[np.clip(y0 + dy, 0, H - 1), np.clip(x0 + dx, 0, W - 1)]
            n_on += on
            n_sky += sky
    saw_sky, no_sky = miss & (n_sky == 4), miss & (n_sky == 0)
    assert saw_sky.sum() > W * H // 8 and no_sky.sum() >= 32
    assert (hist[saw_sky] > 0).all()
    assert (hist[no_sky] == 0).all()
    mean = out[miss, :3] / out[miss, 3:4]
    assert mean.max() <= 1.0 + 1e-5                         # the gradient sky is at most 1: no hit tap came through
    assert (hist[miss] <= 4 * (1 + 1e-6)).all()            # renormalised weights: never more than a tap holds


# ---------------------------------------------------------------- cap
def test_cap(rtw):
    W, H = 33, 17
    cur_cam, prev_cam, B, cnd, A, pnd, mom = T.synthetic_frames(rtw, W, H, "still")
    world = T.D.host_world()
    A = np.ascontiguousarray(np.abs(np.nan_to_num(A, nan=1.0)) / np.maximum(A[:, 3:4], 1) * 100)    # w = 100
    A[:, 3] = 100
    B = np.ascontiguousarray(np.abs(np.nan_to_num(B, posinf=1.0)) / np.maximum(B[:, 3:4], 1) * 2)   # 2 spp
    B[:, 3] = 2
    mom[1, :, 2] = np.maximum(mom[1, :, 2], 1)
    out, m, hist = world.temporal_accumulate(cur_cam, prev_cam, B, cnd, A.astype(F), pnd, mom, max_history=8.0)
    assert (hist == 8).all() and (out[:, 3] == 10).all()
    want = (8 * (A[:, :3].astype(np.float64) / 100) + 2 * (B[:, :3].astype(np.float64) / 2)) / 10
    assert rel(out[:, :3] / out[:, 3:4], want).max() <= PARITY
    # the moments: sw scaled by 8 / 100 with M2 and n kept, then West's update by the 2 current samples -- the
    # header's operations in float32, so bit for bit
    ref_out, ref_m = reference_still(B.astype(F), A.astype(F), mom[1], 8.0)
    assert np.array_equal(out.view(np.uint32), ref_out.view(np.uint32))
    assert np.array_equal(m[1].view(np.uint32), ref_m.view(np.uint32))
    assert np.array_equal(m[0].view(np.uint32), out.view(np.uint32))
    scaled = mom[1, :, 3] * (F(8) / F(100))
    assert np.array_equal(m[1][:, 3], scaled + F(2)) and np.array_equal(m[1][:, 2], mom[1, :, 2] + 1)
    zero = np.zeros_like(B)                                  # no current samples: the interpolated history itself
    _, m0, _ = world.temporal_accumulate(cur_cam, prev_cam, zero, cnd, A.astype(F), pnd, mom, max_history=8.0)
    assert np.array_equal(m0[1][:, 3], scaled)
    assert np.array_equal(m0[1][:, 1:3], mom[1][:, 1:3]) and np.array_equal(m0[1][:, 0], mom[1][:, 0])


# ---------------------------------------------------------------- moments downstream
def test_moments_downstream(rtw):
    world, _, _ = T.host_world("cornell")
    cams = T.orbit(rtw, 4, 48, step_deg=2.0)
    W = H = 48
    state = rtw.RayTraceState(camera=cams[0], writer=rtw.SharedStateImageWriter(W, H), world=world, seed=5)
    cams[0].render_range(state, 0, cams[0].size, 0, 2)
    state.update_moments()
    n0 = state.moments[1][:, 2].copy()
    assert (n0 == 1).all()
    for cam in cams[1:]:
        n_before = state.moments[1][:, 2].copy()
        hist = state.move_camera(cam, 2)
        assert state.camera is cam
        n = state.moments[1][:, 2]
        kept = hist > 0
        assert kept.sum() > 0.8 * W * H and (~kept).any()
        assert (n[kept] > 1).all() and (n[~kept] == 1).all()
        assert n[kept].mean() > n_before.mean()
        assert np.array_equal(state.moments[0], state.writer.buffer)
        assert (state.writer.buffer[:, 3] == hist + 2).all()
    err, tiles, summary = world.noise_estimate(state.moments, W, H)
    assert np.isfinite(err[state.moments[1][:, 2] >= 2]).all() and summary.known > 0.8 * W * H
    out, var = world.denoise_guided(state.writer.buffer, state.moments, state._guides[1], W, H, variance=True)
    assert np.isfinite(out).all() and np.isfinite(var).all()


# ---------------------------------------------------------------- degenerate inputs
@pytest.mark.parametrize("kind", ["still", "translated", "panned"])
def test_degenerate_history_and_current(rtw, kind):
    W, H = 33, 17
    cur_cam, prev_cam, B, cnd, A, pnd, mom = T.synthetic_frames(rtw, W, H, kind)
    world = T.D.host_world()
    out, m, hist = world.temporal_accumulate(cur_cam, prev_cam, B, cnd, A, pnd, mom, max_history=6.0)
    assert np.isfinite(out).all() and np.isfinite(m).all() and np.isfinite(hist).all()
    assert (hist >= 0).all() and (hist <= 6).all() and (hist > 0).sum() > W * H // 2
    bad_cur = ~(np.isfinite(B).all(1) & (B[:, 3] > 0))
    assert bad_cur.sum() == 2
    assert np.array_equal(out[bad_cur, 3], hist[bad_cur])            # a current pixel that contributes nothing
    assert np.array_equal(out[~bad_cur, 3], hist[~bad_cur] + B[~bad_cur, 3])
    assert np.array_equal(m[0], out)
    if kind == "still":
        ref_out, ref_m = reference_still(B, A, mom[1], 6.0)
        assert np.array_equal(out.view(np.uint32), ref_out.view(np.uint32))
        assert np.array_equal(m[1].view(np.uint32), ref_m.view(np.uint32))
        bad = ~(np.isfinite(A).all(1) & (A[:, 3] > 0))
        assert bad.sum() == 2 and (hist[bad] == 0).all()
    else:
        # the bad taps are skipped and the rest renormalised: the history's mean stays inside the valid taps' range
        good = np.isfinite(A).all(1) & (A[:, 3] > 0)
        means = A[good, :3] / A[good, 3:4]
        only, _, h = world.temporal_accumulate(cur_cam, prev_cam, np.zeros_like(B), cnd, A, pnd, max_history=64.0)
        k = h > 0
        got = only[k, :3] / only[k, 3:4]
        assert got.min() >= means.min() - 1e-4 and got.max() <= means.max() + 1e-4
        assert h[k].min() >= 1 - 1e-5 and h.max() <= 8 + 1e-5
    # in place on cur_accum
    B2 = B.copy()
    out2, m2, hist2 = world.temporal_accumulate(cur_cam, prev_cam, B2, cnd, A, pnd, mom, out=B2, max_history=6.0)
    assert out2 is B2
    for a, b in ((out, out2), (m, m2), (hist, hist2)):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


def test_refusals_leave_outputs_untouched(rtw):
    W, H = 9, 5
    cc, pc, B, cnd, A, pnd, mom = T.synthetic_frames(rtw, W, H, "translated")
    world = T.D.host_world()
    A_ = rtw._abi
    n = W * H
    out, om, hist = np.full((n, 4), 7, F), np.full((2, n, 4), 7, F), np.full(n, 7, F)
    good = A_.temporal_params()
    other = T.frame_camera(rtw, (0, 0, 0), (0, 0, -3), W=W + 1, H=H)
    empty = A_.RtwCamera.from_buffer_copy(bytes(cc.derived))
    empty.image_width = 0

    def params(**kw):
        p = A_.temporal_params()
        for k, v in kw.items():
            setattr(p, k, v)
        return p
    base = dict(world=world, cc=cc, pc=pc, cur=B, cnd=cnd, prev=A, pnd=pnd, pm=mom, params=good, out=out, om=om, hist=hist)
    cases = {
        "sizes differ": dict(pc=other), "sizes differ (current)": dict(cc=other),
        "zero-sized current": dict(cc=empty), "zero-sized previous": dict(pc=empty),
        "null ctx": dict(world=None), "null cur_cam": dict(cc=None), "null prev_cam": dict(pc=None),
        "null cur_accum": dict(cur=None), "null cur_nd": dict(cnd=None), "null prev_accum": dict(prev=None),
        "null prev_nd": dict(pnd=None), "null params": dict(params=None), "null out": dict(out=None),
        "prev_moments alone": dict(om=None), "out_moments alone": dict(pm=None),
        "max_history 0": dict(params=params(max_history=0.0)), "max_history < 0": dict(params=params(max_history=-1.0)),
        "max_history inf": dict(params=params(max_history=np.inf)), "max_history nan": dict(params=params(max_history=np.nan)),
        "tolerance 0": dict(params=params(depth_tolerance=0.0)), "tolerance inf": dict(params=params(depth_tolerance=np.inf)),
        "tolerance nan": dict(params=params(depth_tolerance=np.nan)), "cos > 1": dict(params=params(normal_cos=1.5)),
        "cos < -1": dict(params=params(normal_cos=-1.5)), "cos nan": dict(params=params(normal_cos=np.nan)),
        "flags": dict(params=params(flags=1)),
        "out is prev_accum": dict(out=A), "out is prev_nd": dict(out=pnd), "out_moments is prev_moments": dict(om=mom),
        "history in prev_accum": dict(hist=A.reshape(-1)[:n]),
    }
    keep = [x.copy() for x in (A, pnd, mom)]
    for name, kw in cases.items():
        rc = call(rtw, **{**base, **kw})
        assert rc == A_.RTW_E_INVALID, name
        assert rtw.lib().rtw_last_error(), name
        assert (out == 7).all() and (om == 7).all() and (hist == 7).all(), name
        for x, y in zip((A, pnd, mom), keep):
            assert np.array_equal(x, y, equal_nan=True), name
    assert call(rtw, **base) == A_.RTW_OK
    assert not (out == 7).all() and not (hist == 7).all()
    with pytest.raises(KeyError):
        A_.temporal_params(sigma=1.0)
    # the device form refuses a host context
    rc = rtw.lib().rtw_temporal_accumulate_device(world.handle, C.byref(cc.derived), C.byref(pc.derived), B.ctypes.data,
                                                  cnd.ctypes.data, A.ctypes.data, pnd.ctypes.data, None, C.byref(good),
                                                  out.ctypes.data, None, None, None, 0)
    assert rc == A_.RTW_E_INVALID and b"host context" in rtw.lib().rtw_last_error()


def test_defaults_are_the_grid_winner(rtw):
    import json
    import os
    from conftest import REPO
    rec = json.load(open(os.path.join(REPO, "profiles", "temporal", "defaults.json")))
    p = rtw._abi.temporal_params()
    assert C.sizeof(p) == 32 and p.flags == 0
    w = rec["winner"]
    assert (p.max_history, p.depth_tolerance, p.normal_cos) == (F(w["max_history"]), F(w["depth_tolerance"]), F(w["normal_cos"]))


# ---------------------------------------------------------------- worth having
def test_worth_having(rtw):
    """An 8-frame Cornell orbit at 2 spp per frame against 256 spp of the last camera: carrying the history beats
    starting over, raw and under the guided filter.  Only the sign is claimed; the ratios measured on the host
    backend are in profiles/temporal/README.md."""
    world, _, _ = T.host_world("cornell")
    W = H = 64
    cams = T.orbit(rtw, 8, W, step_deg=1.0)
    state = rtw.RayTraceState(camera=cams[0], writer=rtw.SharedStateImageWriter(W, H), world=world, seed=11)
    cams[0].render_range(state, 0, cams[0].size, 0, 2)
    state.update_moments()
    for cam in cams[1:]:
        state.move_camera(cam, 2)
    last = cams[-1]
    ref = T.render(world, last, 256, 999)
    guides = world.render_guides(last)
    alone = G.render_batches(rtw, world, last, (1, 1), 77)
    alone_guided = world.denoise_guided(alone[-1], G.fold(world, alone, W, H), guides, W, H)
    temporal = state.writer.buffer
    temporal_guided = world.denoise_guided(temporal, state.moments, guides, W, H)
    e = {k: T.rmse(v, ref) for k, v in (("alone", alone[-1]), ("temporal", temporal), ("guided alone", alone_guided),
                                        ("temporal + guided", temporal_guided))}
    print({k: round(v, 5) for k, v in e.items()}, "ratios", round(e["temporal"] / e["alone"], 3),
          round(e["temporal + guided"] / e["guided alone"], 3))
    assert e["temporal"] < e["alone"]
    assert e["temporal + guided"] < e["guided alone"]
