"""The geometry of the camera-ray candidate lists (rtw_tuning.tile_lists) without a GPU: tile_frustum and tile_reach
of csrc/rtw_wavefront.hip are host + device functions, and rtw_debug_tile_reach runs them on the host.

tests/tile_scenes.py holds the float64 reference: T (what brute-force rays of a tile hit), R0 (the documented bound
with every margin at zero) and R2 (with the code's margins doubled).  The documented bound must be conservative
(T within R0, tlow_R0 <= t_min), and the fp32 code must lie between R0 and R2."""
import ctypes as C

import numpy as np
import pytest

import tile_scenes as TS

f32, f64 = np.float32, np.float64


@pytest.mark.parametrize("cam_name", sorted(TS.CAMERAS))
def test_documented_bound_is_conservative_and_fp32_lies_between(rtw, cam_name):
    """Book-1's spheres under every camera of the GPU cases, tile by tile:
    T within R0 and tlow_R0 <= t_min on T (the bound as documented is conservative against real and extreme rays);
    R0 within reach_fp32 within R2 and tlow_R2 <= tlow_fp32 <= tlow_R0 wherever the fp32 code keeps a sphere (the code
    implements that bound, with margins between zero and twice its own); the frame is usable."""
    ref = TS.reference("book1", cam_name)
    cam = TS.camera(cam_name)[0].derived
    rendered = 0
    for t in range(ref["n_tiles"]):
        b = ref["bounds"][t]
        hit = np.isfinite(ref["t_min"][t])
        if np.isnan(b[0]):
            assert not hit.any() and not ref["R0"][t].any()
            continue
        rendered += 1
        assert not (hit & ~ref["R0"][t]).any(), (t, ref["ids"][hit & ~ref["R0"][t]])
        assert (ref["tlow0"][t][hit] <= ref["t_min"][t][hit]).all(), t
        keep, tlow, ok = TS.tile_reach_fp32(rtw, cam, b, ref["centres"], ref["radii"])
        assert ok
        assert not (ref["R0"][t] & ~keep).any(), (t, ref["ids"][ref["R0"][t] & ~keep])
        assert not (keep & ~ref["R2"][t]).any(), (t, ref["ids"][keep & ~ref["R2"][t]])
        assert (ref["tlow2"][t][keep] <= tlow[keep]).all() and (tlow[keep] <= ref["tlow0"][t][keep]).all(), t
    assert rendered and ref["R0"].any() and np.isfinite(ref["t_min"]).any()


def test_frame_ok_exactly_for_an_orthogonal_plane_in_front(rtw):
    """frame_ok is false exactly when pixel_delta_u . pixel_delta_v is not zero to 1e-4 |du| |dv| or the pixel plane is
    not in front of the centre along du x dv (h <= 0): camera structs built by hand."""
    def cam_of(du, dv, p00):
        c = rtw._abi.RtwCamera()
        c.image_width, c.image_height, c.size, c.max_depth = 16, 16, 256, 8
        c.pixel_delta_u[:], c.pixel_delta_v[:], c.pixel00_loc[:] = du, dv, p00
        return c

    def ok(c):
        return TS.tile_reach_fp32(rtw, c, (0.0, 7.0, 0.0, 7.0), np.zeros((1, 3)), np.ones(1))[2]

    du, dv = (0.01, 0.0, 0.0), (0.0, -0.01, 0.0)  # du x dv = -z: the plane z = -1 is in front
    for c, want in ((cam_of(du, dv, (-0.08, 0.08, -1.0)), True),
                    (cam_of(du, dv, (-0.08, 0.08, 1.0)), False),   # behind: h < 0
                    (cam_of(du, dv, (-0.08, 0.08, 0.0)), False),   # through the centre: h = 0
                    (cam_of(du, (0.5e-6, -0.01, 0.0), (-0.08, 0.08, -1.0)), True),    # cos 0.5e-4
                    (cam_of(du, (2e-6, -0.01, 0.0), (-0.08, 0.08, -1.0)), False),     # cos 2e-4
                    (cam_of(du, (0.0, 0.0, 0.0), (-0.08, 0.08, -1.0)), False)):       # no plane at all
        assert ok(c) == want
        assert TS.frustum(c, 0.0, 7.0, 0.0, 7.0)["ok"] == want


# ---------------------------------------------------------------- edges of tile_reach
def _axis_camera(rtw, defocus):
    """At the origin looking down -z with vup +y: fz = -z, uh = +x, vh = -y exactly, so a sphere at frame coordinates
    (cu, cv, z) has the centre (cu, -cv, -z) with no rounding.  64 x 48, focus distance 2."""
    return rtw.Camera(aspect_ratio=64 / 48, image_width=64, image_height=48, vfov=40.0, lookfrom=(0.0, 0.0, 0.0),
                      lookat=(0.0, 0.0, -1.0), defocus_angle=defocus, focus_dist=2.0, pixel_offset=0).init().derived


BOUNDS = (40.0, 47.0, 8.0, 15.0)  # an off-axis tile: right of and above the axis


def _check(rtw, cam, frame_xyz, radii):
    """The spheres at frame coordinates (cu, cv, z) through the hook against R0, R2 and the extreme rays."""
    frame_xyz = np.asarray(frame_xyz, f64).reshape(-1, 3)
    F = TS.frustum(cam, *BOUNDS)
    assert np.array_equal(F["fz"], [0, 0, -1]) and np.array_equal(F["uh"], [1, 0, 0]) and np.array_equal(F["vh"], [0, -1, 0])
    centres = (frame_xyz * [1, -1, -1]).astype(f32)
    radii = np.broadcast_to(np.asarray(radii, f32), len(centres)).copy()
    keep, tlow, ok = TS.tile_reach_fp32(rtw, cam, BOUNDS, centres, radii)
    assert ok
    k0, t0 = TS.reach_with(cam, BOUNDS, centres, radii, TS.MARGINS_R0)
    k2, t2 = TS.reach_with(cam, BOUNDS, centres, radii, TS.MARGINS_R2)
    t_min = TS.first_hits(*TS.extreme_rays(cam, BOUNDS), centres, radii)
    hit = np.isfinite(t_min)
    assert not (hit & ~k0).any() and (t0[hit] <= t_min[hit]).all()
    assert not (k0 & ~keep).any(), np.flatnonzero(k0 & ~keep)
    assert not (keep & ~k2).any(), np.flatnonzero(keep & ~k2)
    assert (t2[keep] <= tlow[keep]).all() and (tlow[keep] <= t0[keep]).all()
    return keep, tlow, k0, k2, hit


@pytest.mark.parametrize("defocus", [0.0, 12.0])
def test_tile_reach_at_the_camera_plane(rtw, defocus):
    """Spheres that touch, straddle, contain or lie behind the camera plane z = 0.
    Centre exactly on the plane; z = +-rho and its float32 neighbours (the branch thresholds, which the slack moves:
    whichever branch takes them, the result lies between R0 and R2); a sphere that contains the camera (Book-1's
    r = 1000 ground does) is kept with tlow 0; a sphere wholly behind the camera is rejected."""
    cam = _axis_camera(rtw, defocus)
    rho = f32(0.75)
    zs = [0.0, rho, np.nextafter(rho, f32(0)), np.nextafter(rho, f32(2)), -rho, np.nextafter(-rho, f32(0)),
          np.nextafter(-rho, f32(-2))]
    # on the axis, off it inside the straddle bound, and far off it
    pts = [(cu, cv, float(z)) for z in zs for cu, cv in ((0.0, 0.0), (0.5, -0.4), (30.0, 0.0))]
    keep, tlow, k0, k2, _ = _check(rtw, cam, pts, rho)
    assert keep[0::3].all() and not keep[2::3].any() and (tlow[keep] == 0).all()
    # containing the camera; wholly behind it (near the axis: only the sign of z rejects it)
    keep, tlow, *_ = _check(rtw, cam, [(0.0, 999.0, 3.0), (0.1, 0.1, -5.0), (0.0, 0.0, -1.01)], [1000.0, 1.0, 1.0])
    assert keep.tolist() == [True, False, False] and tlow[0] == 0


@pytest.mark.parametrize("defocus", [0.0, 12.0])
@pytest.mark.parametrize("t", [0.25, 1.0, 40.0, 5000.0])
def test_tile_reach_at_the_frustum_edge(rtw, defocus, t):
    """Spheres approaching the tile's frustum from outside, at depth t h: before the focus plane (t < 1, where the
    cross-section is the rectangle widened by (1 - t) rd), on it, far behind it ((t - 1) rd: the other side of the
    disk), and at a distance of 10^4, where the slack must scale with the coordinates.  Sweeps of the gap across
    rho sec from three edges and the far corner: R0 within fp32 within R2 and the extreme rays' hits are kept
    (_check); R0 ends exactly at rho sec; the fp32 code keeps everything up to there and nothing from 1.2 rho sec on
    (its slack, 1e-3 of the coordinates, is worth about 0.03 rho sec here; R2's twice that)."""
    cam = _axis_camera(rtw, defocus)
    F = TS.frustum(cam, *BOUNDS)
    z = t * F["h"]
    rho = 0.05 * z
    grow = abs(1.0 - t) * F["rd"]
    gaps = rho * F["sec"] * np.concatenate([np.linspace(0.5, 0.99, 8), [1 - 1e-4, 1 + 1e-4], np.linspace(1.01, 1.1, 4),
                                            [1.2, 1.35, 1.5]])
    mid_u, mid_v = 0.5 * t * (F["ru0"] + F["ru1"]), 0.5 * t * (F["rv0"] + F["rv1"])
    pts = [(t * F["ru1"] + grow + g, mid_v, z) for g in gaps]                 # right of the right edge
    pts += [(t * F["ru0"] - grow - g, mid_v, z) for g in gaps]                # left of the left edge
    pts += [(mid_u, t * F["rv0"] - grow - g, z) for g in gaps]                # past the edge farther from the axis
    assert F["ru1"] > F["ru0"] > 0 > F["rv1"] > F["rv0"]
    d = np.array([F["ru1"], F["rv0"]]) / np.hypot(F["ru1"], F["rv0"])
    pts += [(t * F["ru1"] + (grow + g) * d[0], t * F["rv0"] + (grow + g) * d[1], z) for g in gaps]  # the far corner
    keep, tlow, k0, k2, hit = _check(rtw, cam, pts, rho)
    for s in range(4):
        sl = slice(s * len(gaps), (s + 1) * len(gaps))
        assert k0[sl][:9].all() and not k0[sl][9:].any(), (s, k0[sl])
        assert keep[sl][:9].all() and not keep[sl][-3:].any(), (s, keep[sl])
        assert not k2[sl][-3:].any(), (s, k2[sl])
    assert hit.any() and (tlow[keep] > 0).all()


def test_tile_reach_nan_centre(rtw):
    """A NaN in any coordinate of the centre makes z, cu, cv and the slack NaN: `z < -(rho + slack)` is false (not
    behind) and `z > rho + slack` is false, so the straddle branch takes it, where t1 = fmaxf(0, NaN) = 0 and
    `!(lat > ...)` with lat NaN is true: the sphere is kept with tlow 0 -- on every tile, so it can only cost time,
    never a hit.  The front branch cannot see a NaN centre.  The float64 restatement does the same."""
    cam = _axis_camera(rtw, 0.6)
    nan = float("nan")
    centres = np.array([(nan, 0, -3), (0, nan, -3), (0, 0, nan), (nan, nan, nan), (50, 50, nan)], f32)
    keep, tlow, ok = TS.tile_reach_fp32(rtw, cam, BOUNDS, centres, np.full(5, 0.5, f32))
    assert ok and keep.all() and (tlow == 0).all()
    k0, t0 = TS.reach_with(cam, BOUNDS, centres, np.full(5, 0.5), TS.MARGINS_R0)
    assert k0.all() and (t0 == 0).all()
