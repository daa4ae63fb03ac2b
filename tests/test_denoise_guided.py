"""The variance-guided filter (rtw_denoise_guided) on the host backend: against the header's arithmetic in float64,
what the variance does to the colour term and how it is propagated, the quality on host renders with the shipped
defaults, refusals, and that a guided call leaves rtw_denoise's results alone."""
import ctypes as C
import json
import os

import numpy as np
import pytest

from conftest import REPO

import denoise_scenes as D
import guided_scenes as G

CPU = -1
SIGMAS = [(1.0, 0.5, 0.2), (0.0, 0.5, 0.2), (1.0, 0.0, 0.2), (1.0, 0.5, 0.0)]


# ---------------------------------------------------------------- against float64
@pytest.mark.parametrize("demodulate", [False, True])
@pytest.mark.parametrize("W,H,passes", [(32, 24, 5), (33, 17, 8)])
def test_guided_against_float64(rtw, W, H, passes, demodulate):
    """Tolerances per pass, as test_filter_against_float64 derives its own (M: the largest finite input mean, V: the
    largest input variance -- the propagated variance is a mean of the taps' with weights <= 1, it never grows):
      a weight h e(x) is off by e's 2^-20, and by x's relative rounding error times x e(x) <= 1 / e.  x = tl + ... with
      tl = |Y_q - Y_p| kl: five roundings in each luminance and one in the difference; in kl the 9-term weighted mean
      vbar (about 12 ulp), the square root (half of vbar's, plus its own), the product, the sum and the reciprocal
      -- about 24 ulp in all, 24 x 2^-24 / e = 5.3e-7.  So a weight is off by 1.5e-6, relatively.
      colour    the weights enter the sum and wsum: 2 x 1.5e-6, plus about 30 ulp for the 25-term weighted mean:
                4.8e-6, rounded up to 5e-6 x M per pass
      variance  the weights enter squared, above and below: 4 x 1.5e-6, plus 30 ulp for the sum and 2 ulp for
                wsum wsum and the division: 7.9e-6, rounded up to 1e-5 x V per pass
    Measured worst case over these cases: DESIGN.md §Noise estimates and the guided filter."""
    acc, mom, alb, nd = G.filter_inputs(W, H)
    M = D.largest_mean(acc)
    V = float(G.variance(mom[1].astype(np.float64), np.float64).max())
    if demodulate:
        V = V / (0.25 ** 2)                                   # albedo >= 0.25 in these inputs: la >= 0.25
    tol_c, tol_v = passes * 5e-6 * M, passes * 1e-5 * V
    wgt = acc[:, 3:4].astype(np.float64)
    ok = wgt[:, 0] > 0
    world = D.host_world()
    for sig in SIGMAS:
        got, var = G.guided(world, acc, mom, alb, nd, W, H, passes=passes, demodulate=demodulate, sigma_color=sig[0],
                            sigma_normal=sig[1], sigma_depth=sig[2])
        ref, rvar = G.reference_guided(acc, mom, alb, nd, W, H, passes, demodulate, *sig)
        err = np.abs(got[ok, :3] / wgt[ok] - ref[ok, :3] / wgt[ok]).max()
        known = rvar >= 0
        verr = np.abs(var[known] - rvar[known]).max()
        print(f"{W} x {H}, {passes} passes, demodulate {demodulate}, sigmas {sig}: colour {err / M:.2e} x M "
              f"(bound {tol_c / M:.1e}), variance {verr / V:.2e} x V (bound {tol_v / V:.1e})")
        assert np.isfinite(got).all() and np.isfinite(var).all()
        assert err <= tol_c, (sig, err, tol_c)
        assert verr <= tol_v, (sig, verr, tol_v)
        assert np.array_equal(var < 0, ~known) and (var[~known] == -1).all()
        assert not known[G.unknown_pixel(W, H)] and known.sum() == W * H - 1
        assert np.array_equal(got[:, 3], acc[:, 3])
        assert np.isfinite(got[D.nan_pixel(W, H)]).all()                   # the NaN pixel is filled from its neighbours
        assert np.array_equal(got[D.zero_w_pixel(W, H)], np.zeros(4, np.float32))
        # without variance_out the colour is the same
        assert np.array_equal(G.guided(world, acc, mom, alb, nd, W, H, variance=False, passes=passes,
                                       demodulate=demodulate, sigma_color=sig[0], sigma_normal=sig[1],
                                       sigma_depth=sig[2]), got)


# ---------------------------------------------------------------- what the variance does
def flat_guides(n):
    nd = np.zeros((n, 4), np.float32)
    nd[:, 2], nd[:, 3] = -1.0, 5.0
    return nd


def known_moments(acc, v):
    """Moments that say: variance of the mean v everywhere (n = 4, sw = w)."""
    n = len(acc)
    mom = np.zeros((2, n, 4), np.float32)
    mom[0] = acc
    mean = G.luma(acc[:, :3].astype(np.float64) / acc[:, 3:4])
    mom[1] = np.stack([mean, np.float64(v) * acc[:, 3] * 3, np.full(n, 4.0), acc[:, 3]], 1)
    return mom


def test_zero_variance_keeps_a_step(rtw):
    """Zero variance everywhere, flat guides, a luminance step of 0.1: kl = 2^20, a tap across the step has weight
    e(0.1 x 2^20) = 0, so every pixel is a mean of equal values: within 4 ulp of its input.  The plain filter with its
    defaults (a wide colour term) moves the pixels at the step by more than 0.01."""
    W, H = 32, 24
    n = W * H
    left = np.tile(np.arange(W) < W // 2, H)
    mean = np.where(left, np.float32(0.5), np.float32(0.6))
    acc = np.stack([mean * 4, mean * 4, mean * 4, np.full(n, 4.0)], 1).astype(np.float32)
    nd = flat_guides(n)
    world = D.host_world()
    out, var = G.guided(world, acc, known_moments(acc, 0.0), None, nd, W, H)
    ulp = np.spacing(mean.astype(np.float32))
    assert (np.abs(out[:, :3] / 4 - mean[:, None]) <= 4 * ulp[:, None]).all()
    assert (var == 0).all()
    plain = D.denoise(rtw, world, acc, None, nd, W, H)
    at_step = np.tile((np.arange(W) == W // 2 - 1) | (np.arange(W) == W // 2), H)
    assert (np.abs(plain[at_step, :3] / 4 - mean[at_step, None]) > 0.01).all()


@pytest.mark.parametrize("passes", [1, 2, 3])
def test_variance_shrinks_as_the_kernel_says(rtw, passes):
    """sl = 0, flat guides, constant variance v0: every weight is the kernel's, wsum = 1, and a pass multiplies the
    variance by sum (h[dx] h[dy])^2 = (70 / 256)^2 wherever all 25 taps are on the image -- after p passes, at
    pixels farther than 2 (2^p - 1) from the border, v0 (70 / 256)^(2 p), to the float64 test's bound."""
    W, H = 40, 32
    acc, _, _ = D.random_inputs(W, H, seed=2, bad=False)
    v0 = 0.37
    mom = known_moments(acc, v0)
    v_in = float(G.variance(mom[1].astype(np.float64), np.float64).max())
    _, var = G.guided(D.host_world(), acc, mom, None, flat_guides(W * H), W, H, passes=passes, sigma_color=0.0,
                      sigma_normal=0.5, sigma_depth=0.2)
    r = 2 * (2 ** passes - 1)
    inner = var.reshape(H, W)[r:H - r, r:W - r]
    assert inner.size > 0
    want = v_in * (70 / 256) ** (2 * passes)
    assert np.abs(inner - want).max() <= passes * 1e-5 * v_in
    assert var.reshape(H, W)[0, 0] > want * 1.5                             # fewer taps at the corner: less averaging


# ---------------------------------------------------------------- quality, defaults, Python layer
def test_guided_defaults_cite_the_search(rtw):
    A = rtw._abi
    p = A.denoise_guided_params()
    rep = json.load(open(os.path.join(REPO, "profiles", "denoise_guided", "defaults.json")))
    w = rep["winner"]
    assert (p.passes, bool(p.flags & A.RTW_DENOISE_DEMODULATE)) == (w["passes"], w["demodulate"])
    assert (p.sigma_color, p.sigma_normal, p.sigma_depth) == tuple(
        np.float32(w[k]) for k in ("sigma_color", "sigma_normal", "sigma_depth"))
    assert rep["winner_beats_plain"] == (w["score"] < rep["plain_defaults"]["score"])


def rmse(a, target, spp):
    return np.sqrt(np.mean((a[:, :3].astype(np.float64) / a[:, 3:4] - target[:, :3].astype(np.float64) / spp) ** 2))


def preview(rtw, arr, cam, seed):
    """(8 spp in 1-spp batches, the guided and the plain filter's results with the shipped defaults, the 2048-spp
    target) on the host backend, through RayTraceState."""
    world = rtw.World(arr, device=CPU)
    target = D.render(rtw, world, cam, 2048, 1000)
    w, h = cam.derived.image_width, cam.derived.image_height
    state = rtw.RayTraceState(cam, rtw.SharedStateImageWriter(w, h), world, seed=seed)
    for s in range(8):
        cam.render_range(state, 0, cam.size, s, s + 1)
        state.update_moments()
    noisy = state.writer.buffer.copy()
    guided = state.denoised(guided=True)
    plain = state.denoised()
    assert (state.moments[1, :, 2] == 8).all() and np.array_equal(state.writer.buffer, noisy)
    world.close()
    return noisy, guided, plain, target


def square(cam, size):
    cam.image_width, cam.image_height, cam.aspect_ratio = size, size, 1.0
    return cam.init()


def test_quality_earth_perlin(rtw):
    """Earth + Perlin 64 x 64, seed 1: the guided filter's result is closer to the 2048-spp target than the 8-spp
    input, which the plain filter's is not (1.14 recorded in profiles/denoise/defaults.json)."""
    arr = rtw.flatten(rtw.worlds.earth_perlin_world(0))
    noisy, guided, plain, target = preview(rtw, arr, square(rtw.earth_perlin_camera(spp=8), 64), 1)
    r = [rmse(a, target, 2048) for a in (noisy, guided, plain)]
    print(f"earth + Perlin: RMSE 8 spp {r[0]:.4f}, guided {r[1]:.4f} ({r[1] / r[0]:.3f}), plain {r[2]:.4f} ({r[2] / r[0]:.3f})")
    assert r[1] < r[0]


def test_quality_book1(rtw):
    """Book-1 64 x 64, seed 1: the guided filter beats the plain filter's shipped defaults."""
    arr = rtw.flatten(rtw.worlds.generate_world(0, "book1"))
    noisy, guided, plain, target = preview(rtw, arr, square(rtw.book1_camera(spp=8), 64), 1)
    r = [rmse(a, target, 2048) for a in (noisy, guided, plain)]
    print(f"Book-1: RMSE 8 spp {r[0]:.4f}, guided {r[1]:.4f} ({r[1] / r[0]:.3f}), plain {r[2]:.4f} ({r[2] / r[0]:.3f})")
    assert r[1] < r[2]


def test_quality_cornell_and_the_accumulator_form(rtw):
    """Cornell 48 x 48, seed 7: closer to the target than the input.  The result has the accumulator's form: w is
    kept, and the texel update and the encoders take it."""
    arr = rtw.flatten(rtw.worlds.cornell_box())
    noisy, guided, plain, target = preview(rtw, arr, rtw.cornell_camera(image_width=48, spp=8).init(), 7)
    r = [rmse(a, target, 2048) for a in (noisy, guided, plain)]
    print(f"Cornell: RMSE 8 spp {r[0]:.4f}, guided {r[1]:.4f} ({r[1] / r[0]:.3f}), plain {r[2]:.4f} ({r[2] / r[0]:.3f})")
    assert r[1] < r[0]
    assert guided.shape == noisy.shape and np.array_equal(guided[:, 3], noisy[:, 3]) and np.isfinite(guided).all()
    n = len(guided)
    tex = np.zeros((n, 4), np.uint8)
    rtw._abi.check(rtw.lib().rtw_texture_from_accum(guided.ctypes.data, n, tex.ctypes.data), "rtw_texture_from_accum")
    assert (tex[:, 3] == 255).all() and tex[:, :3].max() > 0
    size = C.c_size_t()
    buf = np.zeros(64 + 12 * n, np.uint8)
    rtw._abi.check(rtw.lib().rtw_encode_ppm(guided.ctypes.data, 48, 48, rtw._abi.RTW_PPM_WRITECOLOR, buf.ctypes.data,
                                            buf.size, C.byref(size)), "rtw_encode_ppm")
    assert bytes(buf[:2]) == b"P3" and size.value > n


# ---------------------------------------------------------------- refusals, shared planes
def test_guided_refusals_leave_outputs_untouched(rtw):
    A, L = rtw._abi, rtw.lib()
    W, H = 8, 6
    acc, mom, alb, nd = G.filter_inputs(W, H)
    world = D.host_world()
    out = np.full((W * H, 4), 7.0, np.float32)
    var = np.full(W * H, 7.0, np.float32)

    def call(p, w=W, h=H, accum=acc, moments=mom, albedo=alb, guide=nd, o=out, handle=None):
        return L.rtw_denoise_guided(world.handle if handle is None else handle, w, h, A.ptr(accum), A.ptr(moments),
                                    A.ptr(albedo), A.ptr(guide), C.byref(p) if p is not None else None, A.ptr(o),
                                    A.ptr(var))
    good = A.denoise_guided_params(passes=2)
    for kw in (dict(passes=0), dict(passes=9), dict(sigma_color=-1.0), dict(sigma_normal=float("nan")),
               dict(sigma_depth=float("inf")), dict(flags=2), dict(flags=1 | 4)):
        assert call(A.denoise_guided_params(**kw)) == A.RTW_E_INVALID, kw
        assert L.rtw_last_error().startswith(b"rtw_denoise_guided: ")      # the message names the call refused
    assert call(good, w=0) == A.RTW_E_INVALID and call(good, h=0) == A.RTW_E_INVALID
    assert call(good, accum=None) == A.RTW_E_INVALID and call(good, guide=None) == A.RTW_E_INVALID
    assert call(good, moments=None) == A.RTW_E_INVALID and b"moments" in L.rtw_last_error()
    assert call(good, o=None) == A.RTW_E_INVALID
    assert call(None) == A.RTW_E_INVALID and call(good, handle=C.c_void_p()) == A.RTW_E_INVALID
    assert call(A.denoise_guided_params(passes=2, demodulate=True), albedo=None) == A.RTW_E_INVALID
    assert L.rtw_denoise_guided_device(world.handle, W, H, A.ptr(acc), A.ptr(mom), A.ptr(alb), A.ptr(nd), C.byref(good),
                                       A.ptr(out), A.ptr(var), None, 0) == A.RTW_E_INVALID
    assert (out == 7.0).all() and (var == 7.0).all()
    assert call(good) == A.RTW_OK and not (out[:, :3] == 7.0).any() and not (var == 7.0).any()
    assert call(A.denoise_guided_params(passes=2, demodulate=False), albedo=None) == A.RTW_OK
    with pytest.raises(KeyError):
        A.denoise_guided_params(sigma_luma=1.0)


def test_plain_filter_unchanged_by_a_guided_call(rtw):
    """The colour planes are shared by the two filters: rtw_denoise's results on random_inputs are the same bits
    before and after guided calls (another size, then the same size) on the same context; and in place."""
    W, H = 33, 17
    acc, alb, nd = D.random_inputs(W, H)
    world = rtw.World(rtw.flatten(rtw.worlds.two_spheres_world()), device=CPU)
    before = [D.denoise(rtw, world, acc, alb, nd, W, H, **kw) for kw in ({}, dict(passes=5, demodulate=True))]
    a2, m2, l2, n2 = G.filter_inputs(40, 24)
    G.guided(world, a2, m2, l2, n2, 40, 24, passes=4, demodulate=True)
    a1, m1, l1, n1 = G.filter_inputs(W, H)
    sep, _ = G.guided(world, a1, m1, l1, n1, W, H, passes=5)
    after = [D.denoise(rtw, world, acc, alb, nd, W, H, **kw) for kw in ({}, dict(passes=5, demodulate=True))]
    for b, a in zip(before, after):
        assert np.array_equal(b, a, equal_nan=True)
    buf = a1.copy()
    same = world.denoise_guided(buf, m1, (l1, n1), W, H, out=buf, passes=5)
    assert same is buf and np.array_equal(buf, sep, equal_nan=True)
    world.close()
