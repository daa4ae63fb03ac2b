"""Inputs and references shared by the tests of the noise estimates and the variance-guided filter:
tests/test_moments.py and tests/test_denoise_guided.py (host backend), tests/test_gpu_moments.py and
tests/test_gpu_denoise_guided.py (GPU).  The header's arithmetic (include/rtw_gpu.h, "Noise estimates and the
variance-guided filter") restated in numpy: in float32, every step one correctly rounded operation, for the moments
and the estimate; in float64 for both and for the filter.

Not a test module.  Nothing here reads the library's results."""
import numpy as np

import denoise_scenes as D

F = np.float32
LR, LG, LB = 0.2126, 0.7152, 0.0722
G3 = np.array([0.25, 0.5, 0.25])
BATCHES = (1, 1, 2, 5, 1, 3)     # the batch sizes of the moment tests' six updates


def luma(c, t=np.float64):
    return (t(LR) * c[..., 0] + t(LG) * c[..., 1]) + t(LB) * c[..., 2]


# ---------------------------------------------------------------- accumulator sequences
def still_pixels(W, H):
    """A pixel sub-range that does not advance in the third update of accumulator_sequence."""
    n = W * H
    return slice(n // 3, n // 3 + max(1, n // 5))


def nan_pixel(W, H):
    return (W * H) // 2 + 1 if W * H > 2 else None


def falling_pixel(W, H):
    return (W * H) // 4 if W * H > 4 else None


def accumulator_sequence(W, H, seed=0, batches=BATCHES):
    """The accumulator after each of len(batches) render calls, float32 (W * H, 4) each: every call adds `k` samples
    of a per-pixel distribution (mean in [0, 2), spread up to the mean) in fp32, as a render does.  In the third
    call the pixels of still_pixels() do not advance; from the second on nan_pixel() carries a NaN; in the fourth
    falling_pixel()'s w falls (a scrubbed and restarted pixel) and rises again afterwards."""
    rng = np.random.default_rng(seed)
    n = W * H
    mean = rng.random((n, 3)) * 2
    acc = np.zeros((n, 4), F)
    out = []
    for j, k in enumerate(batches):
        nxt = acc.copy()
        nxt[:, :3] += (k * mean * (1 + (rng.random((n, 3)) - 0.5) * 2 / np.sqrt(k))).astype(F)
        nxt[:, 3] += F(k)
        if j == 2:
            nxt[still_pixels(W, H)] = acc[still_pixels(W, H)]
        if j >= 1 and nan_pixel(W, H) is not None:
            nxt[nan_pixel(W, H), 1] = np.nan
        if j == 3 and falling_pixel(W, H) is not None:
            nxt[falling_pixel(W, H)] = (0.5, 0.25, 0.125, 1.0)
        acc = nxt
        out.append(acc)
    return out


# ---------------------------------------------------------------- moments and the estimate, restated
def moments_update(accum, mom, t=F):
    """One rtw_moments_update on (2, n, 4) moments of type t; returns the new moments."""
    a = accum.astype(t)
    p, m = mom[0], mom[1]
    with np.errstate(all="ignore"):
        k = a[:, 3] - p[:, 3]
        adv = k > 0
        inv = t(1) / k
        d = (a[:, :3] - p[:, :3]) * inv[:, None]
        y = luma(d, t)
        upd = adv & np.isfinite(y)
        sw = m[:, 3] + k
        e = y - m[:, 0]
        mean = m[:, 0] + e * (k / sw)
        m2 = m[:, 1] + (k * e) * (y - mean)
        new = np.stack([mean, m2, m[:, 2] + t(1), sw], 1)
    out = np.empty_like(mom)
    out[0] = np.where(adv[:, None], a, p)
    out[1] = np.where(upd[:, None], new, m)
    assert out.dtype == t
    return out


def variance(m1, t=F):
    """v of plane 1 (n, 4) of type t; -1 where unknown."""
    with np.errstate(all="ignore"):
        v = (m1[:, 1] / (m1[:, 2] - t(1))) / m1[:, 3]
    v = np.where(v > 0, v, t(0))
    return np.where(m1[:, 2] >= 2, v, t(-1)).astype(t)


def noise_error(m1, floor, t=F):
    v = variance(m1, t)
    with np.errstate(all="ignore"):
        sv = np.sqrt(np.maximum(v, t(0)))
        e = np.where(sv > 0, sv / (np.abs(m1[:, 0]) + t(floor)), t(0))
    e = np.where(e >= 0, e, t(np.inf))
    return np.where(v < 0, t(np.inf), e).astype(t)


def noise_outputs(err, m1, W, H, threshold):
    """(tile_max (th, tw), over, known, max_err) of an error image."""
    th, tw = (H + 7) // 8, (W + 7) // 8
    pad = np.zeros((th * 8, tw * 8), err.dtype)
    pad[:H, :W] = err.reshape(H, W)
    tiles = pad.reshape(th, 8, tw, 8).max((1, 3))
    fin = err[np.isfinite(err)]
    return tiles, int((err > err.dtype.type(threshold)).sum()), int((m1[:, 2] >= 2).sum()), \
        (fin.max() if fin.size else err.dtype.type(0))


# ---------------------------------------------------------------- inputs of the filter tests
def unknown_pixel(W, H):
    return (H // 3) * W + W // 3


def zero_region(W, H):
    """The pixel indices of a block of zero variance (away from the miss block of random_inputs)."""
    ys, xs = np.mgrid[H // 2:min(H, H // 2 + 5), 1:min(W, 7)]
    return (ys * W + xs).ravel()


def filter_inputs(W, H, seed=0):
    """D.random_inputs plus moments (2, W * H, 4): plane 1 = (the luminance of the mean, M2, n, sw) with n in
    2 .. 8, sw = max(w, 1) and a variance of the mean v = s^2, s in [0.5, 1.5) -- the scale of the luminance
    differences between neighbours, so the colour term neither vanishes nor shuts every tap out.  One pixel of
    unknown variance (n = 1) and, on frames that hold it, a block of zero variance whose means step by 0.05 from pixel
    to pixel (there kl = 2^20: every tap but the centre has weight e(> 5e4) = 0, in either precision)."""
    acc, alb, nd = D.random_inputs(W, H, seed)
    rng = np.random.default_rng(seed + 1000)
    n = W * H
    zr = zero_region(W, H) if n >= 12 else np.zeros(0, int)
    w = acc[:, 3].copy()
    for j, q in enumerate(zr):
        if np.isfinite(acc[q]).all() and w[q] > 0:
            acc[q, :3] = F(1 + 0.05 * j) * w[q]
    sw = np.maximum(w, 1).astype(F)
    cnt = rng.integers(2, 9, n).astype(F)
    v = ((0.5 + rng.random(n)) ** 2).astype(F)
    if n >= 12:
        cnt[unknown_pixel(W, H)] = 1
        v[zr] = 0
    with np.errstate(all="ignore"):
        mean = luma(acc[:, :3].astype(np.float64) / np.where(w > 0, w, 1)[:, None])
    mean = np.where(np.isfinite(mean), mean, 0.0)
    mom = np.zeros((2, n, 4), F)
    mom[0] = acc
    mom[1] = np.stack([mean.astype(F), (v * sw) * (cnt - 1), cnt, sw], 1)
    return acc, mom, alb, nd


def reference_guided(accum, mom, albedo, nd, W, H, passes, demodulate, sl, sn, sd):
    """The header's guided filter in float64: (accumulator-form result (H * W, 4), variance_out (H * W,))."""
    a = accum.astype(np.float64).reshape(H, W, 4)
    g = nd.astype(np.float64).reshape(H, W, 4)
    w = a[..., 3]
    with np.errstate(all="ignore"):
        c = a[..., :3] * (1.0 / w)[..., None]
        v = variance(mom[1].astype(np.float64), np.float64).reshape(H, W)
        if demodulate:
            al = np.maximum(albedo.astype(np.float64).reshape(H, W, 4)[..., :3], D.FLOOR)
            c = c / al
            la = luma(al)
            v = np.where(v >= 0, v / (la * la), v)
        hit = g[..., 3] > 0
        kn = 1.0 / sn ** 2 if sn > 0 else 0.0
        kz = np.where(hit, 1.0 / (sd ** 2 * g[..., 3] ** 2), 0.0) if sd > 0 else np.zeros((H, W))
        ys, xs = np.mgrid[0:H, 0:W]

        def tap(dy, dx):
            qy, qx = ys + dy, xs + dx
            inside = (qy >= 0) & (qy < H) & (qx >= 0) & (qx < W)
            qy, qx = np.clip(qy, 0, H - 1), np.clip(qx, 0, W - 1)
            cq, gq, vq = c[qy, qx], g[qy, qx], v[qy, qx]
            return cq, gq, vq, inside & np.isfinite(cq).all(-1) & ((gq[..., 3] > 0) == hit)
        for i in range(passes):
            s = 1 << i
            fin_p = np.isfinite(c).all(-1)
            vs, gs = np.zeros((H, W)), np.zeros((H, W))
            for dy in range(-1, 2):
                for dx in range(-1, 2):
                    _, _, vq, ok = tap(dy, dx)
                    ok = ok & (vq >= 0)
                    vs += np.where(ok, G3[dx + 1] * G3[dy + 1] * vq, 0.0)
                    gs += np.where(ok, G3[dx + 1] * G3[dy + 1], 0.0)
            on = fin_p & (gs > 0) & (sl > 0)
            kl = np.where(on, 1.0 / (sl * np.sqrt(vs / np.where(gs > 0, gs, 1.0)) + 2.0 ** -20), 0.0)
            yp = luma(np.where(fin_p[..., None], c, 0.0))
            acc, wsum, vsum = np.zeros((H, W, 3)), np.zeros((H, W)), np.zeros((H, W))
            for dy in range(-2, 3):
                for dx in range(-2, 3):
                    cq, gq, vq, ok = tap(s * dy, s * dx)
                    cq = np.where(ok[..., None], cq, 0.0)
                    x = (np.abs(luma(cq) - yp) * kl + ((gq[..., :3] - g[..., :3]) ** 2).sum(-1) * kn) + \
                        (gq[..., 3] - g[..., 3]) ** 2 * kz
                    e = np.where(x <= 87.0, np.exp(-np.minimum(x, 87.0)), 0.0)
                    wgt = np.where(ok, D.H5[dx + 2] * D.H5[dy + 2] * e, 0.0)
                    acc += wgt[..., None] * cq
                    wsum += wgt
                    vsum += wgt * wgt * np.maximum(vq, 0.0)
            some = wsum > 0
            safe = np.where(some, wsum, 1.0)
            c = np.where(some[..., None], acc / safe[..., None], c)
            v = np.where(v >= 0, np.where(some, vsum / (safe * safe), v), -1.0)
        if demodulate:
            c = c * al
            v = np.where(v >= 0, v * (la * la), v)
        out = np.concatenate([c * w[..., None], w[..., None]], -1)
    return out.reshape(-1, 4), v.reshape(-1)


GUIDED_KEYS = ("passes", "demodulate", "sigma_color", "sigma_normal", "sigma_depth")


def guided(world, acc, mom, alb, nd, W, H, variance=True, **params):
    return world.denoise_guided(acc, mom, (alb, nd), W, H, variance=variance, **params)


def render_batches(rtw, world, cam, batches, seed):
    """The accumulator after each batch of a render of sum(batches) samples per pixel, split into those batches."""
    import ctypes as C
    buf = np.zeros((cam.size, 4), np.float32)
    out, s = [], 0
    for k in batches:
        rc = rtw.lib().rtw_render(world.handle, C.byref(cam.derived), 0, cam.size, s, s + k, seed, buf.ctypes.data, None,
                                  rtw._abi.PROGRESS_FN(0), None)
        rtw._abi.check(rc, "rtw_render")
        s += k
        out.append(buf.copy())
    return out


def fold(world, accs, W, H):
    """Zeroed moments updated after each accumulator of accs."""
    mom = np.zeros((2, W * H, 4), np.float32)
    for a in accs:
        world.moments_update(a, mom, W, H)
    return mom
