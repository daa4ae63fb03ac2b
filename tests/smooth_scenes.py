"""Scenes, inputs and renders shared by tests/test_smooth_mesh.py (host backend) and tests/test_gpu_smooth_mesh.py
(GPU): triangles with per-vertex normals and uvs (rtw_scene_set_vertex_attrs) at the top level, in list instances
and in tree instances.

Not a test module.  References are rendered once per process and returned read-only."""
import dataclasses
import functools

import numpy as np

import mesh_scenes as M

CPU = M.CPU


def pkg():
    return M.pkg()


# ---------------------------------------------------------------- rtw_debug_quad_shade
def attr_records(rtw, n, normals=None, uvs=None):
    rec = np.zeros(n, rtw._abi.VERTEX_ATTR_DT)
    if normals is not None:
        rec["normal"] = normals
        rec["flags"] |= rtw._abi.RTW_ATTR_NORMALS
    if uvs is not None:
        rec["uv"] = uvs
        rec["flags"] |= rtw._abi.RTW_ATTR_UVS
    return rec


def quad_shade(rtw, rec, attrs, o, d, t):
    """rtw_debug_quad_shade over n tuples -> (normal (n, 3), uv (n, 2), front (n,) bool)."""
    n = len(rec)
    o, d, t = (np.ascontiguousarray(a, np.float32) for a in (o, d, t))
    rec, attrs = np.ascontiguousarray(rec), np.ascontiguousarray(attrs)
    assert len(attrs) == n and len(o) == n and len(d) == n and len(t) == n
    normal = np.full((n, 3), np.nan, np.float32)
    uv = np.full((n, 2), np.nan, np.float32)
    front = np.full(n, 7, np.uint8)
    rc = rtw.lib().rtw_debug_quad_shade(n, rec.ctypes.data, attrs.ctypes.data, o.ctypes.data, d.ctypes.data,
                                        t.ctypes.data, normal.ctypes.data, uv.ctypes.data, front.ctypes.data)
    rtw._abi.check(rc, "rtw_debug_quad_shade")
    assert set(np.unique(front)) <= {0, 1}
    return normal, uv, front.astype(bool)


def geometric_normal_f32(q_u, q_v):
    """Quad.init's unit normal as the library derives it (rtw_quad_init): every operation rounded to fp32."""
    u, v = q_u.astype(np.float32), q_v.astype(np.float32)
    n = np.stack([u[:, 1] * v[:, 2] - u[:, 2] * v[:, 1], u[:, 2] * v[:, 0] - u[:, 0] * v[:, 2],
                  u[:, 0] * v[:, 1] - u[:, 1] * v[:, 0]], axis=1)
    ln = np.sqrt(n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1] + n[:, 2] * n[:, 2])
    return n / ln[:, None]


def dot_f32(a, b):
    a, b = a.astype(np.float32), b.astype(np.float32)
    return a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1] + a[:, 2] * b[:, 2]


def shade_reference_f64(p, alpha, beta, normals, uvs):
    """The semantics in float64 at the library's fp32 (alpha, beta): the shading normal on the geometric normal's
    side (before it is turned towards the ray) and the interpolated uv."""
    a, b = alpha.astype(np.float64), beta.astype(np.float64)
    w0 = (1.0 - a) - b
    nv = normals.astype(np.float64)
    nv = nv / np.linalg.norm(nv, axis=2, keepdims=True)
    m = w0[:, None] * nv[:, 0] + a[:, None] * nv[:, 1] + b[:, None] * nv[:, 2]
    lm = np.linalg.norm(m, axis=1)
    ns = m / lm[:, None]
    n = np.cross(p["u"].astype(np.float64), p["v"].astype(np.float64))
    n = n / np.linalg.norm(n, axis=1, keepdims=True)
    ns = np.where(((ns * n).sum(1) < 0)[:, None], -ns, ns)
    t = uvs.astype(np.float64)
    uv = w0[:, None] * t[:, 0] + a[:, None] * t[:, 1] + b[:, None] * t[:, 2]
    return ns, uv, lm


def normals_near(n, max_deg, rng, count=3):
    """`count` random unit vectors per row of n (unit), each within max_deg degrees of it."""
    out = np.empty((len(n), count, 3))
    for k in range(count):
        r = rng.normal(size=n.shape)
        perp = r - (r * n).sum(1, keepdims=True) * n
        perp /= np.linalg.norm(perp, axis=1, keepdims=True)
        ang = np.radians(rng.uniform(0.0, max_deg, len(n)))
        out[:, k] = np.cos(ang)[:, None] * n + np.sin(ang)[:, None] * perp
    return out


# ---------------------------------------------------------------- scenes
def texel_image(rtw):
    """8 x 4 RGBA, every texel another colour."""
    px = np.zeros((4, 8, 4), np.uint8)
    for y in range(4):
        for x in range(8):
            px[y, x] = (20 + 30 * x, 40 + 60 * y, 255 - 25 * x - 10 * y, 255)
    return rtw.Image(px)


def without_attrs(arr):
    return dataclasses.replace(arr, vertex_attrs=None)


def smooth_mixed_objects(rtw):
    """cornell_mesh(smooth=True) with attributes in every place: the icosphere (320 triangles, a tree instance)
    smooth, uv-mapped and image-textured; the box's 12 triangles (a list instance) with uvs only, under the same
    image; the free-standing top-level triangle, a mirror, with normals only."""
    w = rtw.worlds
    objs = w.cornell_mesh(smooth=True)
    tex = rtw.ImageTexture.init([texel_image(rtw)], 0)
    ball = w.icosphere(2, [82.5, 100, 82.5], 90, rtw.Lambertian.init(tex), smooth=True, uv=True)
    assert isinstance(objs[-3], rtw.Translate) and isinstance(objs[-3].object.object, rtw.Mesh)
    objs[-3] = rtw.Translate.init(rtw.RotateY.init(ball, 15), [265, 0, 295])
    box = objs[-2].object.object
    assert len(box.objects) == 12
    img = rtw.Lambertian.init(tex)
    for k, tri in enumerate(box.objects):
        tri.mat = img
        tri.uvs = np.array([[0.1 * (k % 4), 0.2], [0.9, 0.1 + 0.05 * k], [0.3, 0.95]], np.float32)
    tri = objs[-1]
    tri.mat = rtw.Metal.fromColor([0.8, 0.8, 0.9], 0.0)
    tri.normals = np.array([[-0.5, 0.2, -1.0], [0.5, 0.2, -1.0], [0.0, 0.9, -1.0]], np.float32)
    return objs


def smooth_treeless_objects(rtw):
    """No instance tree: Cornell's walls, the 20 triangles of a level-0 icosphere at the top level (metal, smooth)
    and the box's 12 triangles as one list instance (smooth by hand: every corner's normal tilted)."""
    w = rtw.worlds
    objs, white = w._cornell_walls([343, 554, 332], [-130, 0, 0], [0, 0, -105], [15, 15, 15])
    objs += w.icosphere(0, [370, 120, 300], 110, rtw.Metal.fromColor([0.9, 0.8, 0.7], 0.0), smooth=True).objects
    box = rtw.HittableList.init()
    for side in rtw.createBox([0, 0, 0], [165, 165, 165], white).objects:
        for tri in rtw.quad_triangles(side):
            n = np.cross(tri.u, tri.v)
            n = n / np.linalg.norm(n)
            tri.normals = (n[None, :] + 0.3 * np.array([[1, 0, 0], [0, 1, 0], [0, 0, 1]])).astype(np.float32)
            box.add(tri)
    objs.append(rtw.Translate.init(rtw.RotateY.init(box, -18), [130, 0, 65]))
    return objs


@functools.lru_cache(maxsize=None)
def mixed_arrays(lights):
    rtw = pkg()
    return rtw.flatten(smooth_mixed_objects(rtw), lights="emissive" if lights else None)


@functools.lru_cache(maxsize=None)
def mixed_host(lights, attrs=True):
    """smooth_mixed on the host backend at the GPU tests' shape; attrs = False: the same scene, flat."""
    rtw = pkg()
    arr = mixed_arrays(lights)
    out = M.render(rtw, arr if attrs else without_attrs(arr), M.cornell_mesh_camera(rtw), M.GSPP, M.GSEED)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def treeless_arrays():
    rtw = pkg()
    return rtw.flatten(smooth_treeless_objects(rtw))


@functools.lru_cache(maxsize=None)
def treeless_host():
    rtw = pkg()
    out = M.render(rtw, treeless_arrays(), M.cornell_mesh_camera(rtw), M.GSPP, M.GSEED)
    out.setflags(write=False)
    return out


def plain_with_empty_records(rtw):
    """cornell_mesh() with a flags = 0 record registered on every triangle: the attribute kernels, the plain image."""
    arr = rtw.flatten(M.mixed_objects(rtw))
    tri = np.flatnonzero(rtw._abi.quad_shape(arr.quads) == rtw._abi.RTW_QUAD_TRIANGLE).astype(np.uint32)
    return dataclasses.replace(arr, vertex_attrs=(tri, np.zeros(len(tri), rtw._abi.VERTEX_ATTR_DT)))
