"""Noise estimates on the host backend: rtw_moments_update and rtw_noise_estimate against the header's arithmetic
restated in numpy float32 (bit for bit) and float64 (within a derived bound), on real renders against numpy's
weighted statistics, and progressive_render's stop criterion."""
import ctypes as C

import numpy as np
import pytest

import denoise_scenes as D
import guided_scenes as G

W, H = 33, 17
EPS = 2.0 ** -24


@pytest.fixture(scope="module")
def sequence():
    seq = G.accumulator_sequence(W, H)
    for a in seq:
        a.setflags(write=False)
    return seq


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def test_moments_bit_for_bit(rtw, sequence):
    """Six updates (batches 1, 1, 2, 5, 1, 3): both planes equal the float32 restatement's bits after each; the
    pixels that do not advance, and the pixel whose w falls, are untouched in both planes; the NaN pixel keeps its
    moments and follows the accumulator in plane 0."""
    world = D.host_world()
    mom = np.zeros((2, W * H, 4), np.float32)
    want = mom.copy()
    still, nanp, fall = G.still_pixels(W, H), G.nan_pixel(W, H), G.falling_pixel(W, H)
    for j, acc in enumerate(sequence):
        before = mom.copy()
        assert world.moments_update(acc, mom, W, H) is mom
        want = G.moments_update(acc, want)
        assert np.array_equal(bits(mom), bits(want)), j
        if j == 2:
            assert np.array_equal(bits(mom[:, still]), bits(before[:, still]))
            assert not np.array_equal(mom[1, :still.start], before[1, :still.start])
        if j == 3:
            assert np.array_equal(bits(mom[:, fall]), bits(before[:, fall]))
        if j >= 1:
            assert np.array_equal(bits(mom[1, nanp]), bits(before[1, nanp]))
            assert np.array_equal(bits(mom[0, nanp]), bits(acc[nanp])) and np.isnan(mom[0, nanp, 1])
    n = mom[1, :, 2]
    assert n[nanp] == 1 and n[still.start] == 5 and n.max() == 6
    # an update with nothing new changes nothing
    again = mom.copy()
    world.moments_update(sequence[-1], again, W, H)
    assert np.array_equal(bits(again), bits(mom))


def test_moments_against_float64(rtw, sequence):
    """The bound, from the update's operation count.  With Y the largest |y| of the sequence, U the number of updates
    and K the samples folded, in units of eps = 2^-24:
      y       1 / k, the subtraction, the product, three products and two sums of the luminance: <= 8 eps Y
      mean    a convex combination of the old mean and y -- their errors do not add -- plus four roundings (e, k / sw,
              the product, the sum) on values <= 2 Y: <= 8 eps Y more per update, so <= (8 + 8 U) eps Y =: dm
      M2      each update adds (k e)(y - mean'), both factors <= 2 Y and each off by <= 2 dm, and rounds three times
              on a term <= 4 k Y^2: <= k (8 Y dm + 12 eps Y^2) per update; over the sequence
              <= K Y^2 (8 (8 + 8 U) + 12 + U) eps  (the last U: the running sum's own roundings)
    U = 6, K = 13: 3.3e-6 Y for the mean, 3.6e-4 Y^2 for M2.  Measured worst case: DESIGN.md §Noise estimates and the
    guided filter."""
    world = D.host_world()
    mom = np.zeros((2, W * H, 4), np.float32)
    ref = np.zeros((2, W * H, 4), np.float64)
    ymax = 0.0
    prev = np.zeros((W * H, 4))
    for acc in sequence:
        world.moments_update(acc, mom, W, H)
        ref = G.moments_update(acc, ref, np.float64)
        with np.errstate(all="ignore"):
            y = G.luma((acc[:, :3].astype(np.float64) - prev[:, :3]) / (acc[:, 3:4] - prev[:, 3:4]))
        ok = np.isfinite(y) & (acc[:, 3] > prev[:, 3])
        ymax = max(ymax, np.abs(y[ok & (np.arange(W * H) != G.falling_pixel(W, H))]).max())
        prev = ref[0]
    U, K = len(sequence), sum(G.BATCHES)
    tol_mean = (8 + 8 * U) * EPS * ymax
    tol_m2 = K * ymax ** 2 * (8 * (8 + 8 * U) + 12 + U) * EPS
    keep = np.arange(W * H) != G.falling_pixel(W, H)          # (its last batch is measured from a stale plane 0)
    em = np.abs(mom[1, keep, 0] - ref[1, keep, 0]).max()
    e2 = np.abs(mom[1, keep, 1] - ref[1, keep, 1]).max()
    print(f"mean: {em / ymax:.2e} Y (bound {tol_mean / ymax:.1e});  M2: {e2 / ymax ** 2:.2e} Y^2 (bound {tol_m2 / ymax ** 2:.1e})")
    assert em <= tol_mean and e2 <= tol_m2
    assert np.array_equal(mom[1, :, 2:], ref[1, :, 2:])       # n and sw are small integers: exact


@pytest.mark.parametrize("floor,threshold", [(0.01, 0.05), (0.0, 0.5), (1.0, 0.0)])
def test_noise_estimate_exact(rtw, sequence, floor, threshold):
    """err equals the float32 restatement's bits; tile_max, over, known and max_err are exact."""
    world = D.host_world()
    mom = G.fold(world, sequence, W, H)
    mom[1, 5] = (0.0, 0.0, 3.0, 3.0)                           # a black pixel without variance: err = 0, floor 0 too
    err, tiles, s = world.noise_estimate(mom, W, H, threshold=threshold, floor=floor)
    want = G.noise_error(mom[1], floor)
    assert np.array_equal(bits(err), bits(want))
    wt, over, known, mx = G.noise_outputs(want, mom[1], W, H, threshold)
    assert tiles.shape == (3, 5) and np.array_equal(bits(tiles), bits(wt))
    assert (s.over, s.known, s.max_err) == (over, known, mx)
    assert err[5] == 0 and np.isinf(err[G.nan_pixel(W, H)]) and s.known == W * H - 1 and 0 < s.over < W * H
    # the optional outputs may be absent
    s2 = rtw._abi.RtwNoiseSummary()
    rc = rtw.lib().rtw_noise_estimate(world.handle, W, H, mom.ctypes.data, floor, threshold, None, None, C.byref(s2))
    assert rc == 0 and bytes(s2) == bytes(s)
    # against float64: one division, one square root and one division more on top of the moments' own error
    ref = G.noise_error(mom[1].astype(np.float64), floor, np.float64)
    fin = np.isfinite(ref)
    assert np.array_equal(fin, np.isfinite(err))
    assert np.abs(err[fin] - ref[fin]).max() <= 8 * EPS * ref[fin].max()


def test_noise_refusals(rtw):
    A, L = rtw._abi, rtw.lib()
    world = D.host_world()
    mom = np.zeros((2, 6, 4), np.float32)
    acc = np.ones((6, 4), np.float32)
    err = np.full(6, 7.0, np.float32)
    s = A.RtwNoiseSummary(over=9, known=9, max_err=9.0)

    def est(floor=0.01, thr=0.05, w=3, h=2, m=mom, out=s, handle=world.handle):
        return L.rtw_noise_estimate(handle, w, h, A.ptr(m), floor, thr, A.ptr(err), None,
                                    C.byref(out) if out is not None else None)
    for kw in (dict(floor=-1.0), dict(floor=float("nan")), dict(thr=float("inf")), dict(thr=-0.5), dict(w=0), dict(h=0),
               dict(m=None), dict(out=None), dict(handle=None)):
        assert est(**kw) == A.RTW_E_INVALID, kw
    assert L.rtw_moments_update(world.handle, 3, 2, None, A.ptr(mom)) == A.RTW_E_INVALID
    assert L.rtw_moments_update(world.handle, 3, 2, A.ptr(acc), None) == A.RTW_E_INVALID
    assert L.rtw_moments_update(world.handle, 0, 2, A.ptr(acc), A.ptr(mom)) == A.RTW_E_INVALID
    assert L.rtw_moments_update(None, 3, 2, A.ptr(acc), A.ptr(mom)) == A.RTW_E_INVALID
    # the device forms refuse a host context
    assert L.rtw_moments_update_device(world.handle, 3, 2, A.ptr(acc), A.ptr(mom), None, 0) == A.RTW_E_INVALID
    assert L.rtw_noise_estimate_device(world.handle, 3, 2, A.ptr(mom), 0.01, 0.05, A.ptr(err), None,
                                       C.addressof(s), None, 0) == A.RTW_E_INVALID
    assert (err == 7.0).all() and not mom.any() and (s.over, s.known, s.max_err) == (9, 9, 9.0)
    assert C.sizeof(A.RtwNoiseSummary) == 24
    assert est() == A.RTW_OK and np.isinf(err).all() and (s.over, s.known, s.max_err) == (6, 0, 0.0)


# ---------------------------------------------------------------- real renders
@pytest.fixture(scope="module")
def cornell(rtw):
    """Cornell 24 x 24 on the host backend: the accumulators of eight 1-spp batches and of the same samples as four
    2-spp batches."""
    arr = rtw.flatten(rtw.worlds.cornell_box())
    cam = rtw.cornell_camera(image_width=24, spp=8).init()
    world = rtw.World(arr, device=D.CPU)
    ones = G.render_batches(rtw, world, cam, (1,) * 8, 5)
    twos = G.render_batches(rtw, world, cam, (2,) * 4, 5)
    yield world, ones, twos
    world.close()


def batch_luma(accs):
    """(batches, pixels) mean luminance of each batch and its size, in float64."""
    prev = np.zeros_like(accs[0], np.float64)
    ys, ks = [], []
    for a in accs:
        a = a.astype(np.float64)
        k = a[:, 3] - prev[:, 3]
        ys.append(G.luma((a[:, :3] - prev[:, :3]) / k[:, None]))
        ks.append(k)
        prev = a
    return np.array(ys), np.array(ks)


def weighted_stats(accs):
    y, k = batch_luma(accs)
    mean = (k * y).sum(0) / k.sum(0)
    s2 = (k * (y - mean) ** 2).sum(0) / (len(y) - 1)
    return mean, s2, s2 / k.sum(0), np.abs(y).max()


def test_moments_of_real_renders(rtw, cornell):
    """mean and s2 after eight 1-spp updates against numpy's weighted statistics of the eight batch differences,
    within test_moments_against_float64's bound (U = 8, K = 8; s2 = M2 / 7).
    The same samples as four 2-spp batches give another estimate of the same v: both are unbiased, so their
    difference d has mean zero in every pixel, and the pixels are independent -- the mean of d over the N pixels
    has standard deviation std(d) / sqrt(N).  std(d) is taken from numpy's statistics of the batch differences, not
    from the library; the margin is four such standard deviations (6e-5 of being exceeded by chance)."""
    world, ones, twos = cornell
    assert np.array_equal(ones[-1], twos[-1])                              # the same samples
    m8 = G.fold(world, ones, 24, 24)
    m4 = G.fold(world, twos, 24, 24)
    mean, s2, v8, Y = weighted_stats(ones)
    U = K = 8
    tol_mean = (8 + 8 * U) * EPS * Y
    tol_m2 = K * Y ** 2 * (8 * (8 + 8 * U) + 12 + U) * EPS
    assert (m8[1, :, 2] == 8).all() and (m8[1, :, 3] == 8).all() and (m4[1, :, 2] == 4).all()
    em = np.abs(m8[1, :, 0] - mean).max()
    e2 = np.abs(m8[1, :, 1] / 7.0 - s2).max()
    print(f"cornell 24 x 24: mean {em / Y:.2e} Y (bound {tol_mean / Y:.1e}), s2 {e2 / Y ** 2:.2e} Y^2 (bound {tol_m2 / 7 / Y ** 2:.1e})")
    assert em <= tol_mean and e2 <= tol_m2 / 7 + EPS * s2.max()
    assert s2.max() > 0
    _, _, v4, _ = weighted_stats(twos)
    margin = 4 * np.std(v8 - v4) / np.sqrt(v8.size)
    got8, got4 = G.variance(m8[1]), G.variance(m4[1])
    assert not np.array_equal(got8, got4)                                  # another state
    diff = float(np.mean(got8.astype(np.float64) - got4))
    print(f"mean v: 1-spp batches {got8.mean():.4e}, 2-spp batches {got4.mean():.4e}, difference {diff:.2e}, margin {margin:.2e}")
    assert abs(diff) <= margin


def test_progressive_render_stops_on_noise(rtw):
    """Two spheres under the gradient sky: a threshold the frame reaches long before `spp` stops the render early,
    never before two batches; the default leaves the moments alone and renders every sample."""
    arr = rtw.flatten(rtw.worlds.two_spheres_world())
    world = rtw.World(arr, device=D.CPU)
    cam = rtw.Camera(image_width=16, image_height=12, aspect_ratio=16 / 12, samples_per_pixel=64, max_depth=8,
                     background_mode=rtw._abi.RTW_BG_GRADIENT, defocus_angle=0.0).init()
    state = rtw.RayTraceState(cam, rtw.SharedStateImageWriter(16, 12), world, seed=3)
    done = rtw.progressive_render(state, batch=2, until_noise=1.0, noise_floor=0.05)
    assert 4 <= done < 64 and done == state.samples_done()
    n = state.moments[1, :, 2]
    assert (n == done // 2).all()
    _, _, s = world.noise_estimate(state.moments, 16, 12, threshold=1.0, floor=0.05)
    assert s.over == 0 and s.known == 16 * 12
    # an unreachable threshold: every sample; scrub() resets the moments
    state.writer.scrub()
    assert not state.moments.any()
    cam.samples_per_pixel = 6
    assert rtw.progressive_render(state, batch=2, until_noise=0.0) == 6 and (state.moments[1, :, 2] == 3).all()
    other = rtw.RayTraceState(cam, rtw.SharedStateImageWriter(16, 12), world, seed=3)
    assert rtw.progressive_render(other, batch=2) == 6 and other.writer.moments is None
    assert np.array_equal(other.writer.buffer, state.writer.buffer)
    world.close()
