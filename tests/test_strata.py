"""Stratified pixel samples (rtw_camera.strata, rtw_camera_set_strata: the sqrt_spp jittering of "The Rest of Your
Life") on the host backend (RTW_DEVICE_CPU, the GPU's per-sample code compiled for the host) and through the
host-only hook rtw_debug_camera_ray: the ABI, the jitter bit for bit against its numpy restatement, strata off,
the variance bound at an edge, agreement with the oracle (which knows no strata: the estimator stays unbiased) and
schedule invariance.  Every seed is fixed: every figure below is deterministic."""
import ctypes as C
import re
import os

import numpy as np
import pytest

import strata_scenes as S

CPU = S.CPU
f32 = np.float32
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------- 1. ABI
def test_abi(rtw):
    A = rtw._abi
    lib = rtw.lib()
    assert hasattr(lib, "rtw_camera_set_strata") and hasattr(lib, "rtw_debug_camera_ray")
    cam = rtw.book1_camera(image_width=32, aspect_ratio=1.6, spp=5, max_depth=4).init()
    assert cam.derived.strata == 0
    for n in (0, 1, 2, 256):
        assert lib.rtw_camera_set_strata(C.byref(cam.derived), n) == A.RTW_OK
        assert cam.derived.strata == n
    before = bytes(cam.derived)
    assert lib.rtw_camera_set_strata(C.byref(cam.derived), 257) == A.RTW_E_INVALID
    assert b"strata" in lib.rtw_last_error()
    assert bytes(cam.derived) == before and cam.derived.strata == 256
    assert lib.rtw_camera_set_strata(None, 2) == A.RTW_E_INVALID
    assert A.RTW_MAX_STRATA == 256
    # the Camera field goes through the same call
    assert rtw.Camera(image_width=16, strata=5).init().derived.strata == 5
    with pytest.raises(rtw.RtwError):
        rtw.Camera(image_width=16, strata=257).init()
    # a camera poked past the maximum is refused by the render and by the hook
    world = rtw.World(S.book1_arrays(), device=CPU)
    cam.derived.strata = 257
    buf = np.zeros((cam.size, 4), f32)
    rc = lib.rtw_render(world.handle, C.byref(cam.derived), 0, cam.size, 0, 1, 0, buf.ctypes.data, None,
                        A.PROGRESS_FN(0), None)
    assert rc == A.RTW_E_INVALID and b"strata" in lib.rtw_last_error()
    assert not buf.any()
    with pytest.raises(rtw.RtwError):
        S.camera_rays(rtw, cam, 0, [0], [0])
    world.close()
    # the struct is the one of ABI 8: 8 words, 9 vectors + background, one float
    assert C.sizeof(A.RtwCamera) == 4 * (8 + 3 * 9 + 1 + 3) == 156
    assert A.RtwCamera.strata.offset == 28 and A.RtwCamera.center.offset == 32
    # ... and the header's: its fields, counted
    text = open(os.path.join(REPO, "include", "rtw_gpu.h")).read()
    body = re.sub(r"/\*.*?\*/", "", re.search(r"typedef struct rtw_camera \{(.*?)\} rtw_camera;", text, re.S).group(1),
                  flags=re.S)
    words = 0
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        ty, names = decl.split(None, 1)
        assert ty in ("uint32_t", "float")
        for name in names.split(","):
            m = re.fullmatch(r"\s*(\w+)(?:\[(\d+)\])?\s*", name)
            words += int(m.group(2) or 1)
    assert 4 * words == C.sizeof(A.RtwCamera)
    assert "uint32_t strata;" in body and "_pad" not in body
    assert lib.rtw_version() == 8


# ---------------------------------------------------------------- 2. exact jitter
PIXELS = (0, 7, 333, 639)          # of the 32 x 20 frame


def sample_set(n):
    s = set()
    if n <= 16:
        s.update(range(3 * n * n))
    m = np.arange(0, 1 << 17, n * n, dtype=np.int64)
    for d in (-1, 0, 1):
        s.update((m + d)[(m + d) >= 0].tolist())
    s.update(range((1 << 24) - 3, (1 << 24) + 2))
    s.update((2 ** 32 - 2, 2 ** 32 - 1))
    return np.array(sorted(s), np.uint32)


def test_numpy_stream_is_rng_py(rtw):
    """The vectorised restatement this file checks against is rng.py's path stream."""
    pix = np.array([0, 7, 333, 639, 5], np.uint32)
    smp = np.array([0, 1, 99, (1 << 24) - 1, 2 ** 32 - 1], np.uint32)
    st = S.path_states(77, pix, smp)
    st, a = S.path_float(st)
    st, b = S.path_float(st)
    for k in range(len(pix)):
        r = rtw.rng.Stream(77, rtw.rng.DOMAIN_RENDER, int(pix[k]), int(smp[k]))
        assert (r.path_float(), r.path_float()) == (a[k], b[k])


@pytest.mark.parametrize("defocus", [0.0, 0.6], ids=["pinhole", "defocus"])
@pytest.mark.parametrize("n", [1, 2, 3, 4, 7, 16, 256])
def test_exact_jitter(rtw, n, defocus):
    seed = 5
    base = dict(image_width=32, image_height=20, aspect_ratio=1.6, spp=5, max_depth=4)
    cam = rtw.book1_camera(**base)
    cam.defocus_angle = defocus
    cam = S.with_strata(cam, n, 1)
    off = rtw.book1_camera(**base)
    off.defocus_angle = defocus
    off = S.with_strata(off, 0, 1)
    smp = sample_set(n)
    pixels = np.repeat(np.array(PIXELS, np.uint32), len(smp))
    samples = np.tile(smp, len(PIXELS))
    o, d, t, j = S.camera_rays(rtw, cam, seed, pixels, samples)
    o0, d0, t0, j0 = S.camera_rays(rtw, off, seed, pixels, samples)
    px, py = S.jitter_reference(seed, pixels, samples, n)
    assert np.array_equal(j[:, 0].view(np.uint32), px.view(np.uint32))
    assert np.array_equal(j[:, 1].view(np.uint32), py.view(np.uint32))
    # the closed cell
    si, sj = S.cells(n, samples)
    m = max(n, 1)
    for jit, c in ((j[:, 0], si), (j[:, 1], sj)):
        assert (jit.astype(np.float64) >= c / m - 0.5).all() and (jit.astype(np.float64) <= (c + 1) / m - 0.5).all()
    # every aligned pass visits every cell once
    if n <= 16:
        k = (sj * m + si)[:3 * m * m].reshape(3, m * m)
        assert (np.sort(k, axis=1) == np.arange(m * m)).all()
    # the disk and time draws keep their places: origin and time do not know about strata
    assert np.array_equal(o.view(np.uint32), o0.view(np.uint32))
    assert np.array_equal(t.view(np.uint32), t0.view(np.uint32))
    if n == 1:
        assert np.array_equal(d.view(np.uint32), d0.view(np.uint32))
        assert np.array_equal(j.view(np.uint32), j0.view(np.uint32))
    # dir = pixel_sample - origin (camera.zig:169-180), in float32
    dv = cam.derived
    p00, du, dvv = (np.array(v[:], f32) for v in (dv.pixel00_loc, dv.pixel_delta_u, dv.pixel_delta_v))
    fi = (pixels % dv.image_width + dv.pixel_offset).astype(f32)[:, None]
    fj = (pixels // dv.image_width + dv.pixel_offset).astype(f32)[:, None]
    centre = (p00 + du * fi) + dvv * fj
    sample = centre + (j[:, :1] * du + j[:, 1:] * dvv)
    assert np.array_equal((sample - o).view(np.uint32), d.view(np.uint32))


# ---------------------------------------------------------------- 3. off is off
def test_off_is_off(rtw):
    A = rtw._abi
    arr = S.book1_arrays()
    base = dict(image_width=32, image_height=20, aspect_ratio=1.6, spp=5, max_depth=8)
    cams = {n: S.with_strata(rtw.book1_camera(**base), n) for n in (0, 1, 3)}
    ref = None
    for kernel in (A.RTW_KERNEL_WAVEFRONT, A.RTW_KERNEL_PERSISTENT, A.RTW_KERNEL_SIMPLE):
        world = rtw.World(arr, device=CPU, tuning={"kernel": kernel})
        img = {n: S.render(rtw, world, cam, 0, 5, 3) for n, cam in cams.items()}
        world.close()
        assert np.array_equal(img[0], img[1])
        assert not np.array_equal(img[3], img[0])
        assert (img[3][:, 3] == 5).all()
        if ref is None:
            ref = img
        assert np.array_equal(img[0], ref[0]) and np.array_equal(img[3], ref[3])


# ---------------------------------------------------------------- 4. edge variance
EDGE_SEEDS = tuple(range(200, 264))
EDGE_BOUND = 0.584     # (2n - 1) / (4 n^4) over f (1 - f) / n^2 at n = 4, f (1 - f) >= 3 / 16


def test_edge_variance(rtw):
    """One emissive quad (radiance 1), a long strip whose two parallel edges, 8 pixels apart (no pixel sees both),
    cross a 32 x 32 frame at 29 degrees through no pixel corner; black background, max_depth 1: a pixel's value is
    its coverage f.  strata 4 against strata 0 at 16 spp, 64 seeds each, on the
    pixels with f in [0.25, 0.75]: n^2 plain samples have variance f (1 - f) / n^2 >= 3 / (16 n^2); a stratified
    pass has at most 2n - 1 cells the line crosses, each of variance <= 1/4, so its variance is at most
    (2n - 1) / (4 n^4): the ratio of the summed variances is <= 0.584 at n = 4.  Measured: 0.2152 over 33 pixels;
    worst |difference of the seed-means| / (5 se) = 0.404."""
    th = np.radians(29.0)
    e, nrm = np.array([np.cos(th), np.sin(th), 0.0]), np.array([-np.sin(th), np.cos(th), 0.0])
    p = np.array([0.13, 0.07, 0.0])            # a point of one edge; a pixel is 0.11 wide at the quad
    quad = rtw.Quad.init(list(p - 20 * e), list(40 * e), list(0.9 * nrm), rtw.DiffuseLight.fromColor([1, 1, 1]))
    world = rtw.World(rtw.flatten([quad]), device=CPU)
    kw = dict(aspect_ratio=1.0, image_width=32, samples_per_pixel=16, max_depth=1, vfov=20.0,
              lookfrom=(0.0, 0.0, -10.0), lookat=(0.0, 0.0, 0.0), defocus_angle=0.0, background=(0.0, 0.0, 0.0),
              pixel_offset=0)
    img = {}
    for n in (0, 4):
        cam = rtw.Camera(strata=n, **kw).init()
        img[n] = np.stack([S.render(rtw, world, cam, 0, 16, s)[:, 0] / 16 for s in EDGE_SEEDS]).astype(np.float64)
    world.close()
    f = img[0].mean(0)
    sel = np.flatnonzero((f >= 0.25) & (f <= 0.75))
    assert len(sel) >= 20, len(sel)
    on, off = img[4][:, sel], img[0][:, sel]
    ratio = on.var(0, ddof=1).sum() / off.var(0, ddof=1).sum()
    se = np.sqrt(on.var(0, ddof=1) / len(EDGE_SEEDS) + off.var(0, ddof=1) / len(EDGE_SEEDS))
    z = np.abs(on.mean(0) - off.mean(0)) / (5 * se)
    print(f"edge: {len(sel)} pixels, variance ratio strata 4 / off = {ratio:.4f}, "
          f"worst |difference| / (5 se) = {z.max():.3f}")
    assert ratio <= EDGE_BOUND
    assert (z <= 1).all(), (int(sel[z.argmax()]), z.max())


# ---------------------------------------------------------------- 5. unbiased against the oracle
def test_unbiased_against_oracle(rtw, oracle):
    """Cornell 32 x 32, depth 10, reference BVH mode, 8 seeds: strata 4 at 256 spp on the host against the oracle
    at 512 spp (tests/test_lights.py's, rendered once per session): every 4 x 4 block and channel, and the image
    mean per channel, within 5 sqrt(seA^2 + seB^2).  Measured: worst 0.518 (blocks), 0.160 (image)."""
    import lights_scenes as LS
    import test_lights as TL
    ref = TL.cornell_images("cornell")[2]
    cam = S.with_strata(rtw.cornell_camera(image_width=TL.CW, spp=TL.CSPP, max_depth=TL.CDEPTH), 4)
    world = rtw.World(LS.cornell(rtw, "cornell", False, rtw._abi.RTW_BVH_REFERENCE), device=CPU)
    on = np.stack([S.render(rtw, world, cam, 0, TL.CSPP, s)[:, :3] / TL.CSPP for s in TL.CSEEDS]).astype(np.float64)
    world.close()
    n = np.sqrt(len(TL.CSEEDS))
    for what, a, b in (("blocks", TL.blocks(on), TL.blocks(ref)), ("image", on.mean(1), ref.mean(1))):
        da = a.mean(0) - b.mean(0)
        se = np.sqrt((a.std(0, ddof=1) / n) ** 2 + (b.std(0, ddof=1) / n) ** 2)
        z = np.abs(da) / (5 * se)
        print(f"cornell strata 4 {what}: worst |difference| / (5 se) = {z.max():.3f}")
        assert (z <= 1).all(), (what, z.max())


# ---------------------------------------------------------------- 6. schedule invariance
W, H, S0, SPLIT, S1, SEED = S.GW, S.GH, S.GS0, S.GSPLIT, S.GS1, S.GSEED   # 40 x 24, [0, 7) + [7, 20), strata 3


def split_render(rtw, world, cam):
    buf = S.render(rtw, world, cam, S0, SPLIT, SEED)
    return S.render(rtw, world, cam, SPLIT, S1, SEED, buf=buf)


def test_schedule_invariance(rtw, tmp_path):
    """Book-1, strata 3, samples [0, 20) = two full passes of 9 and a prefix of 2: the stratum is a function of the
    absolute sample index, so every way of cutting the work renders the same bits."""
    arr, cam = S.scene("book1")
    full = S.host_image("book1")
    assert (full[:, 3] == S1).all()
    world = rtw.World(arr, device=CPU, tuning={"cpu_threads": 4})
    assert np.array_equal(S.render(rtw, world, cam, S0, S1, SEED), full)
    assert np.array_equal(split_render(rtw, world, cam), full)
    assert np.array_equal(S.render(rtw, world, cam, S0, S1, SEED, spp_batch=3), full)
    one = rtw.World(arr, device=CPU, tuning={"cpu_threads": 1})
    assert np.array_equal(S.render(rtw, one, cam, S0, S1, SEED), full)
    one.close()
    for flag in (0, rtw._abi.RTW_ROWS_BALANCED):
        image = np.zeros((H, W, 4), f32)
        for k in range(3):
            rows = rtw.distributed.shard_rows(H, 5 | flag, 3, k)
            tile = np.zeros((len(rows) * W, 4), f32)
            rtw.distributed.render_rows_host(world, cam, 5 | flag, 3, k, S0, S1, tile, seed=SEED)
            image[rows] = tile.reshape(len(rows), W, 4)
        assert np.array_equal(image.reshape(-1, 4), full), flag
    part = S.render(rtw, world, cam, S0, S1, SEED, pix=(137, 611))
    assert np.array_equal(part[137:611], full[137:611]) and not part[:137].any() and not part[611:].any()
    # a checkpoint at 7 resumes to the same image; another strata is another camera
    path = str(tmp_path / "strata.ck")
    st = rtw.RayTraceState(cam, rtw.SharedStateImageWriter(W, H), world, seed=SEED)
    cam.render_range(st, 0, cam.size, S0, SPLIT)
    st.checkpoint(path, SPLIT)
    st2 = rtw.RayTraceState(cam, rtw.SharedStateImageWriter(W, H), world, seed=SEED)
    assert st2.resume(path) == SPLIT
    cam.render_range(st2, 0, cam.size, SPLIT, S1)
    assert np.array_equal(st2.writer.buffer, full)
    other = rtw.RayTraceState(S.book1_camera(rtw, strata=4), rtw.SharedStateImageWriter(W, H), world, seed=SEED)
    with pytest.raises(rtw.RtwError):
        other.resume(path)
    world.close()


@pytest.mark.parametrize("name", ["cornell_lights", "cornell_mesh_smooth"])
def test_schedule_invariance_registered(rtw, name):
    """The split-call identity with registered lights (the RTW_F_PDF kernels' class) and with a smooth mesh (vertex
    attributes: RTW_F_ATTR)."""
    arr, cam = S.scene(name)
    assert (arr.lights is not None) == (name == "cornell_lights")
    assert (arr.vertex_attrs is not None) == (name == "cornell_mesh_smooth")
    world = rtw.World(arr, device=CPU)
    assert np.array_equal(split_render(rtw, world, cam), S.host_image(name))
    world.close()
    assert cam.derived.strata == 3
