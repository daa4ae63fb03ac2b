"""Host-side scene API mirroring the reference's object model.

Reference types (all by value in Zig) and their mirrors here:

* ``Texture`` union  (src/textures.zig:10-27): ``SolidColor``, ``CheckerTexture``,
  ``ImageTexture``, ``NoiseTexture`` (+ ``Perlin``, src/perlin.zig:76-101)
* ``Material`` union (src/material.zig:11-30): ``Lambertian``, ``Metal``,
  ``Dielectric``, ``DiffuseLight``, ``Isotropic``
* ``Sphere`` (src/objects.zig:68-149): ``Sphere.init`` / ``Sphere.initMoving``
* ``Quad`` (src/objects.zig:193-262; ``Triangle``, ``Mesh`` and ``load_obj``: the same record with the
  triangle's interior test), ``HittableList`` (:264-290), ``Translate``
  (:292-331), ``RotateY`` (:333-443), ``ConstantMedium`` (:445-508) and
  ``createBox`` (:510-532)
* ``BVHTree`` (src/bvh.zig:17-104): ``BVHTree.init(objects, start, end)`` --
  flattens the objects to the C-ABI records (include/rtw_gpu.h) and hands them
  to ``rtw_scene_create``, which builds the reference-topology BVH natively
  and uploads it to the GPU.

Flattening order (one material per sphere, one texture per textured material,
Perlin tables and images de-duplicated by identity) is part of the fixture
contract checked in tests/test_scenes.py.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass, field
from typing import List, Optional, Sequence

import numpy as np

from . import _abi
from .rng import DOMAIN_PERLIN, Stream, f32


def _v3(x) -> np.ndarray:
    a = np.asarray(x, dtype=np.float32).reshape(3)
    return a.copy()


# ---------------------------------------------------------------- textures
@dataclass(eq=False)
class Texture:
    kind: int


@dataclass(eq=False)
class SolidColor(Texture):
    color_value: np.ndarray = field(default_factory=lambda: np.zeros(3, np.float32))

    @staticmethod
    def init(color) -> "SolidColor":
        return SolidColor(_abi.RTW_TEX_SOLID, _v3(color))


@dataclass(eq=False)
class CheckerTexture(Texture):
    inv_scale: np.float32 = f32(1)
    even: SolidColor = None
    odd: SolidColor = None

    @staticmethod
    def init(scale, even: SolidColor, odd: SolidColor) -> "CheckerTexture":
        """textures.zig:53-56: inv_scale = 1.0 / scale (f32)."""
        return CheckerTexture(_abi.RTW_TEX_CHECKER, f32(f32(1.0) / f32(scale)), even, odd)


@dataclass(eq=False)
class Image:
    """A decoded zstbi.Image: RGBA8 rows (src/rtw_image.zig, forced 4 components)."""
    rgba: np.ndarray  # (H, W, 4) uint8

    @property
    def width(self) -> int:
        return int(self.rgba.shape[1])

    @property
    def height(self) -> int:
        return int(self.rgba.shape[0])

    @staticmethod
    def load_npz(path: str, key: str = "rgba") -> "Image":
        with np.load(path, allow_pickle=False) as z:
            return Image(np.ascontiguousarray(z[key], dtype=np.uint8))


@dataclass(eq=False)
class ImageTexture(Texture):
    image: Image = None

    @staticmethod
    def init(images: Sequence[Image], image_index: int) -> "ImageTexture":
        return ImageTexture(_abi.RTW_TEX_IMAGE, images[image_index])


@dataclass(eq=False)
class Perlin:
    ranvec: np.ndarray  # (256, 3) f32
    perm_x: np.ndarray  # (256,) u16
    perm_y: np.ndarray
    perm_z: np.ndarray

    @staticmethod
    def init(seed: int = 0, table_id: int = 0) -> "Perlin":
        """perlin.zig:83-101 on the seeded stream (domain 3, a = table id).

        ``permute``'s randomIntRange(0, i) can return i + 1; at i = 255 the
        reference indexes p[256] (UB) -- clamped to 255 here."""
        s = Stream(seed, DOMAIN_PERLIN, table_id, 0)
        ranvec = np.zeros((256, 3), np.float32)
        for i in range(256):
            p = s.vec_range(-1, 1)
            ls = f32(f32(f32(p[0] * p[0]) + f32(p[1] * p[1])) + f32(p[2] * p[2]))
            ranvec[i] = p / np.sqrt(ls, dtype=np.float32)
        perms = []
        for _ in range(3):
            p = np.arange(256, dtype=np.uint16)
            for i in range(255, 0, -1):
                t = min(s.int_range(0, i), 255)
                p[i], p[t] = p[t], p[i]
            perms.append(p)
        return Perlin(ranvec, *perms)


@dataclass(eq=False)
class NoiseTexture(Texture):
    noise: Perlin = None
    scale: np.float32 = f32(1)

    @staticmethod
    def init(scale, perlin: Optional[Perlin] = None, seed: int = 0) -> "NoiseTexture":
        return NoiseTexture(_abi.RTW_TEX_NOISE, perlin if perlin is not None else Perlin.init(seed), f32(scale))


# ---------------------------------------------------------------- materials
@dataclass(eq=False)
class Material:
    kind: int
    texture: Optional[Texture] = None
    albedo: np.ndarray = field(default_factory=lambda: np.zeros(3, np.float32))
    fuzz: np.float32 = f32(0)
    ir: np.float32 = f32(0)


class Lambertian:
    @staticmethod
    def init(texture: Texture) -> Material:
        return Material(_abi.RTW_MAT_LAMBERTIAN, texture)

    @staticmethod
    def fromColor(color) -> Material:
        return Material(_abi.RTW_MAT_LAMBERTIAN, SolidColor.init(color))


class Metal:
    @staticmethod
    def fromColor(color, f) -> Material:
        """material.zig:61-63: fuzz clamped to <= 1."""
        f = f32(f)
        return Material(_abi.RTW_MAT_METAL, None, _v3(color), f if f < f32(1) else f32(1))


class Dielectric:
    @staticmethod
    def init(ir) -> Material:
        return Material(_abi.RTW_MAT_DIELECTRIC, None, ir=f32(ir))


class DiffuseLight:
    @staticmethod
    def init(texture: Texture) -> Material:
        return Material(_abi.RTW_MAT_DIFFUSE_LIGHT, texture)

    @staticmethod
    def fromColor(color) -> Material:
        return Material(_abi.RTW_MAT_DIFFUSE_LIGHT, SolidColor.init(color))


class Isotropic:
    @staticmethod
    def init(texture: Texture) -> Material:
        return Material(_abi.RTW_MAT_ISOTROPIC, texture)

    @staticmethod
    def fromColor(color) -> Material:
        return Material(_abi.RTW_MAT_ISOTROPIC, SolidColor.init(color))


# ---------------------------------------------------------------- objects
@dataclass(eq=False)
class Sphere:
    center1: np.ndarray
    radius: np.float32
    mat: Material
    is_moving: bool = False
    center2: Optional[np.ndarray] = None

    @staticmethod
    def init(center1, radius, mat: Material) -> "Sphere":
        return Sphere(_v3(center1), f32(radius), mat)

    @staticmethod
    def initMoving(center1, center2, radius, mat: Material) -> "Sphere":
        return Sphere(_v3(center1), f32(radius), mat, True, _v3(center2))


@dataclass(eq=False)
class Quad:
    """Quad.init (objects.zig:201-210); the library derives normal, d, w and the box.

    shape: RTW_QUAD_PARALLELOGRAM, or RTW_QUAD_TRIANGLE -- the triangle q, q + u, q + v (``Triangle.init``).
    normals / uvs (triangles only): per-corner shading normals (3, 3) and texture coordinates (3, 2), corners in
    the order q, q + u, q + v; None = the geometric normal / (alpha, beta)."""
    q: np.ndarray
    u: np.ndarray
    v: np.ndarray
    mat: Material
    shape: int = _abi.RTW_QUAD_PARALLELOGRAM
    normals: Optional[np.ndarray] = None
    uvs: Optional[np.ndarray] = None

    @staticmethod
    def init(q, u, v, mat: Material) -> "Quad":
        return Quad(_v3(q), _v3(u), _v3(v), mat)


class Triangle:
    """The book's first "additional 2D primitive": a Quad record with another interior test (alpha + beta <= 1,
    inclusive like the quad's edges).  Plane, normal (cross(b - a, c - a)), front face and (u, v) = (alpha, beta)
    are the quad's; the box is that of the three vertices.

    normals (3, 3) / uvs (3, 2): per-vertex shading normals (any length but zero) and texture coordinates of a, b,
    c, interpolated over the face (smooth shading; ``World`` registers them, rtw_scene_set_vertex_attrs)."""

    @staticmethod
    def init(a, b, c, mat: Material, normals=None, uvs=None) -> Quad:
        a = _v3(a)
        if normals is not None:
            normals = np.array(normals, dtype=np.float32).reshape(3, 3)
        if uvs is not None:
            uvs = np.array(uvs, dtype=np.float32).reshape(3, 2)
        return Quad(a, _v3(b) - a, _v3(c) - a, mat, _abi.RTW_QUAD_TRIANGLE, normals, uvs)


def quad_triangles(quad: Quad) -> List[Quad]:
    """The two triangles (q, u, v) and (q + u + v, -u, -v) that tile a parallelogram (same plane and normal)."""
    if quad.shape != _abi.RTW_QUAD_PARALLELOGRAM:
        raise ValueError("not a parallelogram")
    far = (quad.q + quad.u) + quad.v
    return [Quad(quad.q.copy(), quad.u.copy(), quad.v.copy(), quad.mat, _abi.RTW_QUAD_TRIANGLE),
            Quad(far, -quad.u, -quad.v, quad.mat, _abi.RTW_QUAD_TRIANGLE)]


@dataclass(eq=False)
class HittableList:
    """objects.zig:264-290 (members: Spheres / Quads / Triangles).

    bvh: under a transform the library walks a private BVH over the members (``Hittable{.tree}`` in the
    reference) instead of testing them in turn -- True / False, or None = when there are more than 127."""
    objects: list = field(default_factory=list)
    bvh: Optional[bool] = None

    @staticmethod
    def init(bvh: Optional[bool] = None) -> "HittableList":
        return HittableList([], bvh)

    def add(self, obj) -> None:
        self.objects.append(obj)


@dataclass(eq=False)
class Mesh(HittableList):
    """A triangle mesh: a HittableList of ``Triangle``s over shared vertices -- bare or under Translate / RotateY
    it is an instance (more than 127 triangles: with a private BVH, as any list; ``bvh`` as HittableList's), and
    as such a ConstantMedium boundary.

    normals (n, 3) / uvs (n, 2): per-vertex shading normals and texture coordinates, interpolated over each face;
    face_normals / face_uvs (m, 3): the corners' indices into them, where they differ from ``faces`` (an OBJ file's
    ``i/j/k``); a face with a negative index there gets no attribute of that kind."""
    vertices: np.ndarray = None   # (n, 3) f32
    faces: np.ndarray = None      # (m, 3) vertex indices

    @staticmethod
    def init(vertices, faces, mat: Material, bvh: Optional[bool] = None, normals=None, uvs=None, face_normals=None,
             face_uvs=None) -> "Mesh":
        v = np.ascontiguousarray(vertices, dtype=np.float32).reshape(-1, 3)
        f = np.ascontiguousarray(faces, dtype=np.int64).reshape(-1, 3)
        if len(f) and (f.min() < 0 or f.max() >= len(v)):
            raise ValueError("face index out of range")

        def corner_values(values, index, width, what):
            if values is None:
                if index is not None:
                    raise ValueError(f"face_{what} without {what}")
                return None, None
            a = np.ascontiguousarray(values, dtype=np.float32).reshape(-1, width)
            ix = f if index is None else np.ascontiguousarray(index, dtype=np.int64).reshape(-1, 3)
            if ix.shape != f.shape:
                raise ValueError(f"face_{what}: one index triple per face")
            if len(ix) and ix.max() >= len(a):
                raise ValueError(f"{what} index out of range")
            return a, ix

        vn, fn = corner_values(normals, face_normals, 3, "normals")
        vt, ft = corner_values(uvs, face_uvs, 2, "uvs")
        tris = []
        for m, (i, j, k) in enumerate(f):
            tn = vn[fn[m]] if vn is not None and fn[m].min() >= 0 else None
            tt = vt[ft[m]] if vt is not None and ft[m].min() >= 0 else None
            tris.append(Triangle.init(v[i], v[j], v[k], mat, tn, tt))
        return Mesh(tris, bvh, v, f)


def load_obj(path_or_text: str, mat: Material, bvh: Optional[bool] = None, attributes: bool = False) -> Mesh:
    """A Wavefront OBJ file (or its text, if the argument has a line break) as a Mesh: ``v`` and ``f`` lines
    -- face corners ``i``, ``i/j``, ``i/j/k`` or ``i//k``, 1-based or negative (relative to the vertices read so
    far), polygons as fans about their first corner.  Everything else is ignored; an index out of range raises
    ValueError.

    attributes: False = the vertex index of a corner alone is used (flat shading, ``vn`` / ``vt`` lines ignored);
    True = ``vn`` and ``vt`` lines are read too and a face whose corners all carry a ``k`` (``j``) gets per-vertex
    normals (uvs); a ``vn`` / ``vt`` index out of range raises ValueError naming the line."""
    if "\n" in path_or_text:
        text = path_or_text
    else:
        with open(path_or_text) as fh:
            text = fh.read()
    verts, faces, vns, vts, fns, fts = [], [], [], [], [], []

    def index(ln, text, have, what):
        i = int(text)
        k = i - 1 if i > 0 else len(have) + i
        if i == 0 or not 0 <= k < len(have):
            raise ValueError(f"line {ln}: {what} index {i} out of range ({len(have)} so far)")
        return k

    for ln, line in enumerate(text.splitlines(), 1):
        tok = line.split("#", 1)[0].split()
        if not tok:
            continue
        if tok[0] == "v":
            if len(tok) < 4:
                raise ValueError(f"line {ln}: a vertex needs three coordinates")
            verts.append([float(x) for x in tok[1:4]])
        elif tok[0] == "vn" and attributes:
            if len(tok) < 4:
                raise ValueError(f"line {ln}: a normal needs three coordinates")
            vns.append([float(x) for x in tok[1:4]])
        elif tok[0] == "vt" and attributes:
            if len(tok) < 3:
                raise ValueError(f"line {ln}: a texture coordinate needs two values")
            vts.append([float(x) for x in tok[1:3]])
        elif tok[0] == "f":
            corners, cn, ct = [], [], []
            for c in tok[1:]:
                part = c.split("/")
                i = int(part[0])
                k = i - 1 if i > 0 else len(verts) + i
                if i == 0 or not 0 <= k < len(verts):
                    raise ValueError(f"line {ln}: vertex index {i} out of range ({len(verts)} vertices so far)")
                corners.append(k)
                if attributes:   # -1: the corner has none
                    ct.append(index(ln, part[1], vts, "vt") if len(part) > 1 and part[1] else -1)
                    cn.append(index(ln, part[2], vns, "vn") if len(part) > 2 and part[2] else -1)
            if len(corners) < 3:
                raise ValueError(f"line {ln}: a face needs three corners")
            fan = range(1, len(corners) - 1)
            faces += [(corners[0], corners[j], corners[j + 1]) for j in fan]
            if attributes:
                fns += [(cn[0], cn[j], cn[j + 1]) for j in fan]
                fts += [(ct[0], ct[j], ct[j + 1]) for j in fan]
    v, f = np.array(verts, np.float32).reshape(-1, 3), np.array(faces, np.int64).reshape(-1, 3)
    if not attributes:
        return Mesh.init(v, f, mat, bvh)
    return Mesh.init(v, f, mat, bvh, normals=np.array(vns, np.float32).reshape(-1, 3) if vns else None,
                     uvs=np.array(vts, np.float32).reshape(-1, 2) if vts else None,
                     face_normals=np.array(fns, np.int64).reshape(-1, 3) if vns else None,
                     face_uvs=np.array(fts, np.int64).reshape(-1, 3) if vts else None)


@dataclass(eq=False)
class Translate:
    """objects.zig:292-331."""
    object: object
    offset: np.ndarray

    @staticmethod
    def init(obj, offset) -> "Translate":
        return Translate(obj, _v3(offset))


@dataclass(eq=False)
class RotateY:
    """objects.zig:333-443 (sin/cos of degreesToRadians(angle), computed by the library)."""
    object: object
    angle: np.float32

    @staticmethod
    def init(obj, angle) -> "RotateY":
        return RotateY(obj, f32(angle))


@dataclass(eq=False)
class ConstantMedium:
    """objects.zig:445-508: boundary + density + Isotropic phase function."""
    boundary: object
    density: np.float32
    phase: Material

    @staticmethod
    def initFromColor(boundary, density, color) -> "ConstantMedium":
        return ConstantMedium(boundary, f32(density), Isotropic.init(SolidColor.init(color)))

    @staticmethod
    def initFromTexture(boundary, density, texture: Texture) -> "ConstantMedium":
        return ConstantMedium(boundary, f32(density), Isotropic.init(texture))


def createBox(a, b, mat: Material) -> HittableList:
    """objects.zig:510-532: the six sides of the box with opposite vertices a, b."""
    a, b = _v3(a), _v3(b)
    mn = np.minimum(a, b)
    mx = np.maximum(a, b)
    z = np.float32(0)
    dx = np.array([mx[0] - mn[0], z, z], np.float32)
    dy = np.array([z, mx[1] - mn[1], z], np.float32)
    dz = np.array([z, z, mx[2] - mn[2]], np.float32)
    sides = HittableList.init()
    sides.add(Quad.init([mn[0], mn[1], mn[2]], dx, dy, mat))
    sides.add(Quad.init([mx[0], mn[1], mx[2]], -dz, dy, mat))
    sides.add(Quad.init([mx[0], mn[1], mn[2]], -dx, dy, mat))
    sides.add(Quad.init([mn[0], mn[1], mn[2]], dz, dy, mat))
    sides.add(Quad.init([mn[0], mx[1], mx[2]], dx, -dz, mat))
    sides.add(Quad.init([mn[0], mn[1], mn[2]], dx, dz, mat))
    return sides


class Environment:
    """An environment map (rtw_environment): an equirectangular image of linear radiance, float32 (H, W, 3), row 0
    at +y, looked up by the direction of a ray that leaves the scene (sphere_uv's mapping, nearest texel).
    radiance = scale * texel; rotate_y turns the map about y (degrees); sample=True makes the map one more light
    of the mixture density diffuse scatter draws from (RTW_ENV_SAMPLE), so a small bright sun converges."""

    def __init__(self, rgb, scale=(1.0, 1.0, 1.0), rotate_y: float = 0.0, sample: bool = True):
        a = np.ascontiguousarray(rgb, dtype=np.float32)
        if a.ndim != 3 or a.shape[2] != 3:
            raise ValueError("Environment: rgb is not (height, width, 3)")
        self.rgb = a
        self.scale = tuple(float(x) for x in np.asarray(scale, np.float32).reshape(3))
        self.rotate_y = float(rotate_y)
        self.sample = bool(sample)

    @property
    def width(self) -> int:
        return self.rgb.shape[1]

    @property
    def height(self) -> int:
        return self.rgb.shape[0]

    def record(self) -> "_abi.RtwEnvironment":
        """The rtw_environment of this map (it addresses self.rgb: keep self alive across the call)."""
        r = _abi.RtwEnvironment()
        r.rgb = self.rgb.ctypes.data
        r.width, r.height = self.width, self.height
        r.scale[:] = list(self.scale)
        r.rotate_y = self.rotate_y
        r.flags = _abi.RTW_ENV_SAMPLE if self.sample else 0
        return r

    @staticmethod
    def load_hdr(path, **kw) -> "Environment":
        """A Radiance RGBE (.hdr) file as an Environment: flat or new-style run-length-encoded scanlines,
        orientation "-Y h +X w" only.  A pixel (r, g, b, e) is (r, g, b) * 2^(e - 136), and 0 where e = 0."""
        with open(path, "rb") as f:
            data = f.read()
        if not (data.startswith(b"#?RADIANCE") or data.startswith(b"#?RGBE")):
            raise ValueError(f"{path}: not a Radiance RGBE file")
        end = data.find(b"\n\n")
        if end < 0:
            raise ValueError(f"{path}: no end of header")
        header = data[:end].split(b"\n")
        if not any(ln.strip() == b"FORMAT=32-bit_rle_rgbe" for ln in header):
            raise ValueError(f"{path}: FORMAT is not 32-bit_rle_rgbe")
        eol = data.find(b"\n", end + 2)
        res = data[end + 2:eol].split()
        if len(res) != 4 or res[0] != b"-Y" or res[2] != b"+X":
            raise ValueError(f"{path}: orientation {data[end + 2:eol]!r} (only '-Y h +X w' is read)")
        h, w = int(res[1]), int(res[3])
        raw = np.frombuffer(data, np.uint8, offset=eol + 1)
        px = np.zeros((h, w, 4), np.uint8)
        pos = 0
        for y in range(h):
            rle = 8 <= w < 32768 and pos + 4 <= len(raw) and raw[pos] == 2 and raw[pos + 1] == 2 and \
                (int(raw[pos + 2]) << 8 | int(raw[pos + 3])) == w
            if not rle:   # a flat scanline
                if pos + 4 * w > len(raw):
                    raise ValueError(f"{path}: truncated at scanline {y}")
                px[y] = raw[pos:pos + 4 * w].reshape(w, 4)
                pos += 4 * w
                continue
            pos += 4
            for c in range(4):
                x = 0
                while x < w:
                    if pos >= len(raw):
                        raise ValueError(f"{path}: truncated at scanline {y}")
                    n = int(raw[pos])
                    pos += 1
                    if n > 128:   # a run
                        n -= 128
                        if n == 0 or x + n > w or pos >= len(raw):
                            raise ValueError(f"{path}: bad run at scanline {y}")
                        px[y, x:x + n, c] = raw[pos]
                        pos += 1
                    else:         # literals
                        if n == 0 or x + n > w or pos + n > len(raw):
                            raise ValueError(f"{path}: bad literal count at scanline {y}")
                        px[y, x:x + n, c] = raw[pos:pos + n]
                        pos += n
                    x += n
        e = px[..., 3].astype(np.int32)
        f = np.where(e > 0, np.ldexp(np.float32(1.0), e - 136), np.float32(0.0)).astype(np.float32)
        return Environment(px[..., :3].astype(np.float32) * f[..., None], **kw)


@dataclass
class SceneArrays:
    """The neutral scene description handed across the C ABI."""
    spheres: np.ndarray
    materials: np.ndarray
    textures: np.ndarray
    perlins: np.ndarray
    images: List[Image]
    bvh_seed: int = 0
    bvh_mode: int = _abi.RTW_BVH_SAH   # or _abi.RTW_BVH_REFERENCE (bvh.zig topology, same closest hits)
    order_dir: tuple = (0.0, 0.0, 0.0)
    quads: np.ndarray = field(default_factory=lambda: np.zeros(0, _abi.QUAD_DT))
    members: np.ndarray = field(default_factory=lambda: np.zeros(0, _abi.OBJECT_DT))
    instances: np.ndarray = field(default_factory=lambda: np.zeros(0, _abi.INSTANCE_DT))
    media: np.ndarray = field(default_factory=lambda: np.zeros(0, _abi.MEDIUM_DT))
    objects: Optional[np.ndarray] = None   # world_objects order; None = every sphere in order
    lights: Optional[np.ndarray] = None    # rtw_object records World registers (rtw_scene_set_lights); None = none
    # (quad indices u4, VERTEX_ATTR_DT records) of the triangles with per-vertex normals / uvs, which World
    # registers (rtw_scene_set_vertex_attrs); None = none
    vertex_attrs: Optional[tuple] = None
    environment: Optional["Environment"] = None   # World registers it (rtw_scene_set_environment); None = none

    def desc(self):
        """Build an RtwSceneDesc (keeps the ctypes image array alive on self)."""
        imgs = (_abi.RtwImage * max(1, len(self.images)))()
        for i, im in enumerate(self.images):
            imgs[i].data = im.rgba.ctypes.data
            imgs[i].width = im.width
            imgs[i].height = im.height
            imgs[i].bytes_per_row = im.width * 4
        self._imgs = imgs
        d = _abi.RtwSceneDesc()
        d.spheres, d.n_spheres = _abi.ptr(self.spheres), len(self.spheres)
        d.materials, d.n_materials = _abi.ptr(self.materials), len(self.materials)
        d.textures, d.n_textures = _abi.ptr(self.textures), len(self.textures)
        d.images, d.n_images = (C.addressof(imgs) if self.images else 0), len(self.images)
        d.perlins, d.n_perlins = _abi.ptr(self.perlins), len(self.perlins)
        d.bvh_seed = self.bvh_seed
        d.bvh_mode = self.bvh_mode
        d.order_dir[:] = list(self.order_dir)
        d.quads, d.n_quads = _abi.ptr(self.quads), len(self.quads)
        d.members, d.n_members = _abi.ptr(self.members), len(self.members)
        d.instances, d.n_instances = _abi.ptr(self.instances), len(self.instances)
        d.media, d.n_media = _abi.ptr(self.media), len(self.media)
        if self.objects is not None:
            d.objects, d.n_objects = _abi.ptr(self.objects), len(self.objects)
        return d


def flatten(objects: Sequence, bvh_seed: int = 0, bvh_mode: Optional[int] = None, lights=None,
            environment: Optional["Environment"] = None) -> SceneArrays:
    """world_objects -> C-ABI records.  bvh_mode: RTW_BVH_SAH (default, fastest) or
    RTW_BVH_REFERENCE (the reference's random-axis median tree, seeded by bvh_seed).

    environment: an Environment the World registers (rtw_scene_set_environment), carried on the arrays as given.

    lights: the quads and spheres diffuse scatter samples towards (rtw_scene_set_lights) -- None = none,
    "emissive" = every top-level Quad whose material is a DiffuseLight, "emissive+spheres" = those, then
    every top-level static Sphere whose material is a DiffuseLight, or a list of Quad / Sphere objects
    (found by identity among everything flattened; the library validates them).

    Every primitive gets its own material record (and textured materials their own
    texture record), in object order; Perlin tables and images are shared by identity.
    Translate/RotateY chains over a HittableList (or one primitive) become an
    instance; a ConstantMedium's boundary is a sphere, quad or instance record that
    is not itself a world object."""
    spheres, quads, members, instances, media, objs = [], [], [], [], [], []
    mats, texs, perlins, images = [], [], [], []

    def tex_index(t: Texture) -> int:
        rec = np.zeros((), _abi.TEXTURE_DT)
        rec["kind"] = t.kind
        if isinstance(t, SolidColor):
            rec["even"] = t.color_value
        elif isinstance(t, CheckerTexture):
            rec["scale"] = t.inv_scale
            rec["even"] = t.even.color_value
            rec["odd"] = t.odd.color_value
        elif isinstance(t, ImageTexture):
            idx = next((i for i, im in enumerate(images) if im is t.image), None)
            if idx is None:
                images.append(t.image)
                idx = len(images) - 1
            rec["image"] = idx
        elif isinstance(t, NoiseTexture):
            idx = next((i for i, p in enumerate(perlins) if p is t.noise), None)
            if idx is None:
                perlins.append(t.noise)
                idx = len(perlins) - 1
            rec["perlin"] = idx
            rec["scale"] = t.scale
        texs.append(rec)
        return len(texs) - 1

    def mat_index(m: Material) -> int:
        rec = np.zeros((), _abi.MATERIAL_DT)
        rec["kind"] = m.kind
        if m.texture is not None:
            rec["texture"] = tex_index(m.texture)
        rec["albedo"] = m.albedo
        rec["fuzz"] = m.fuzz
        rec["ir"] = m.ir
        mats.append(rec)
        return len(mats) - 1

    where = {}   # id(primitive) -> its (kind, index) record, for `lights`
    attr_quads, attr_recs = [], []   # the triangles with normals / uvs: quad index, VERTEX_ATTR_DT record

    def prim(o) -> tuple:
        where[id(o)] = ref = new_prim(o)
        return ref

    def new_prim(o) -> tuple:
        if isinstance(o, Sphere):
            rec = np.zeros((), _abi.SPHERE_DT)
            rec["center1"] = o.center1
            rec["radius"] = o.radius
            if o.is_moving:
                rec["center2"] = o.center2
                rec["is_moving"] = 1
            rec["material"] = mat_index(o.mat)
            spheres.append(rec)
            return (_abi.RTW_OBJ_SPHERE, len(spheres) - 1)
        if isinstance(o, Quad):
            rec = np.zeros((), _abi.QUAD_DT)
            rec["q"], rec["u"], rec["v"] = o.q, o.u, o.v
            _abi.quad_shape(rec)[...] = o.shape
            rec["material"] = mat_index(o.mat)
            quads.append(rec)
            if o.normals is not None or o.uvs is not None:
                if o.shape != _abi.RTW_QUAD_TRIANGLE:
                    raise ValueError("normals / uvs on a parallelogram (only triangles take vertex attributes)")
                a = np.zeros((), _abi.VERTEX_ATTR_DT)
                if o.normals is not None:
                    a["normal"], a["flags"] = o.normals, a["flags"] | _abi.RTW_ATTR_NORMALS
                if o.uvs is not None:
                    a["uv"], a["flags"] = o.uvs, a["flags"] | _abi.RTW_ATTR_UVS
                attr_quads.append(len(quads) - 1)
                attr_recs.append(a)
            return (_abi.RTW_OBJ_QUAD, len(quads) - 1)
        raise TypeError(f"not a primitive: {type(o).__name__}")

    def hittable(o) -> tuple:
        if isinstance(o, (Sphere, Quad)):
            return prim(o)
        if isinstance(o, (Translate, RotateY, HittableList)):
            xfs = []
            while isinstance(o, (Translate, RotateY)):   # outermost first
                if isinstance(o, Translate):
                    xfs.append((_abi.RTW_XF_TRANSLATE, o.offset))
                else:
                    xfs.append((_abi.RTW_XF_ROTATE_Y, np.array([o.angle, 0, 0], np.float32)))
                o = o.object
            if len(xfs) > _abi.RTW_MAX_XF:
                raise ValueError(f"at most {_abi.RTW_MAX_XF} transforms per instance")
            inner = o.objects if isinstance(o, HittableList) else [o]
            rec = np.zeros((), _abi.INSTANCE_DT)
            rec["first"] = len(members)
            refs = [prim(m) for m in inner]
            for k, i in refs:
                members.append(np.array((k, i), _abi.OBJECT_DT))
            rec["count"] = len(refs)
            rec["n_xf"] = len(xfs)
            rec["flags"] = _abi.RTW_INST_LIST if isinstance(o, HittableList) else 0
            if isinstance(o, HittableList) and (o.bvh or (o.bvh is None and len(refs) > _abi.RTW_INST_LIST_MAX)):
                rec["flags"] |= _abi.RTW_INST_BVH
            for j, (k, v) in enumerate(reversed(xfs)):    # xf[0] = innermost
                rec["xf"][j]["kind"] = k
                rec["xf"][j]["v"] = v
            instances.append(rec)
            return (_abi.RTW_OBJ_INSTANCE, len(instances) - 1)
        if isinstance(o, ConstantMedium):
            rec = np.zeros((), _abi.MEDIUM_DT)
            k, i = hittable(o.boundary)
            rec["boundary"]["kind"], rec["boundary"]["index"] = k, i
            rec["density"] = o.density
            rec["material"] = mat_index(o.phase)
            media.append(rec)
            return (_abi.RTW_OBJ_MEDIUM, len(media) - 1)
        raise TypeError(f"unsupported hittable: {type(o).__name__}")

    for o in objects:
        objs.append(hittable(o))
    light_refs = None
    if isinstance(lights, str):
        if lights not in ("emissive", "emissive+spheres"):
            raise ValueError(f"lights: None, 'emissive', 'emissive+spheres' or a list of objects, not {lights!r}")
        light_refs = [ref for o, ref in zip(objects, objs)
                      if isinstance(o, Quad) and o.mat.kind == _abi.RTW_MAT_DIFFUSE_LIGHT]
        if lights == "emissive+spheres":
            light_refs += [ref for o, ref in zip(objects, objs)
                           if isinstance(o, Sphere) and not o.is_moving and o.mat.kind == _abi.RTW_MAT_DIFFUSE_LIGHT]
    elif lights is not None:
        light_refs = []
        for o in lights:
            if id(o) not in where:
                raise ValueError("lights: an object that is not in the scene")
            light_refs.append(where[id(o)])
    pl = np.zeros(len(perlins), _abi.PERLIN_DT)
    for i, p in enumerate(perlins):
        pl[i]["ranvec"] = p.ranvec
        pl[i]["perm_x"], pl[i]["perm_y"], pl[i]["perm_z"] = p.perm_x, p.perm_y, p.perm_z

    def arr(lst, dt):
        return np.array(lst, dt).reshape(-1) if lst else np.zeros(0, dt)

    only_spheres = all(k == _abi.RTW_OBJ_SPHERE and i == n for n, (k, i) in enumerate(objs)) and \
        len(objs) == len(spheres)
    return SceneArrays(arr(spheres, _abi.SPHERE_DT), arr(mats, _abi.MATERIAL_DT), arr(texs, _abi.TEXTURE_DT), pl,
                       images, bvh_seed, _abi.RTW_BVH_SAH if bvh_mode is None else bvh_mode,
                       quads=arr(quads, _abi.QUAD_DT), members=arr(members, _abi.OBJECT_DT),
                       instances=arr(instances, _abi.INSTANCE_DT), media=arr(media, _abi.MEDIUM_DT),
                       objects=None if only_spheres else arr(objs, _abi.OBJECT_DT),
                       lights=None if light_refs is None else arr(light_refs, _abi.OBJECT_DT),
                       vertex_attrs=(np.array(attr_quads, np.uint32), arr(attr_recs, _abi.VERTEX_ATTR_DT))
                       if attr_quads else None, environment=environment)


def flatten_bvh(arrays: SceneArrays) -> np.ndarray:
    """Host-only BVH build + pre-order flatten (rtw_scene_flatten): the node array
    rtw_scene_create would upload."""
    L = _abi.lib()
    d = arrays.desc()
    n, depth = C.c_uint32(), C.c_uint32()
    _abi.check(L.rtw_scene_flatten(C.byref(d), None, 0, C.byref(n), C.byref(depth)), "rtw_scene_flatten")
    out = np.zeros(n.value, _abi.NODE_DT)
    _abi.check(L.rtw_scene_flatten(C.byref(d), out.ctypes.data, n.value, C.byref(n), C.byref(depth)),
               "rtw_scene_flatten")
    return out


class World:
    """A device-resident world: the result of ``BVHTree.init`` over the objects.

    Owns an ``rtw_ctx`` (one GPU).  ``Hittable{.tree = ...}`` in the reference."""

    def __init__(self, arrays: SceneArrays, device: int = 0, tuning: Optional[dict] = None):
        """tuning: rtw_tuning fields to override (A/B measurement; every setting renders the same image)."""
        L = _abi.lib()
        self.arrays = arrays
        self.device = device
        self._desc = arrays.desc()
        h = C.c_void_p()
        self._tile_lists = int(_abi.tuning(**(tuning or {})).tile_lists)
        if tuning:
            t = _abi.tuning(**tuning)
            _abi.check(L.rtw_scene_create_ex(C.byref(self._desc), device, C.byref(t), C.byref(h)), "rtw_scene_create_ex")
        else:
            _abi.check(L.rtw_scene_create(C.byref(self._desc), device, C.byref(h)), "rtw_scene_create")
        self.handle = h
        try:
            if arrays.lights is not None and len(arrays.lights):
                self.set_lights(arrays.lights)
            if arrays.vertex_attrs is not None and len(arrays.vertex_attrs[0]):
                self.set_vertex_attrs(*arrays.vertex_attrs)
            if arrays.environment is not None:
                self.set_environment(arrays.environment)
        except Exception:
            self.close()
            raise

    def set_lights(self, lights) -> None:
        """rtw_scene_set_lights: the quads and spheres diffuse scatter samples towards -- an OBJECT_DT array,
        (kind, index) pairs, or None / empty to clear (the world then renders exactly as one never given lights).  Must not
        race a render on this world."""
        recs = np.zeros(0, _abi.OBJECT_DT) if lights is None else np.ascontiguousarray(
            lights if isinstance(lights, np.ndarray) and lights.dtype == _abi.OBJECT_DT
            else np.array([tuple(int(x) for x in o) for o in lights], _abi.OBJECT_DT).reshape(-1))
        _abi.check(_abi.lib().rtw_scene_set_lights(self.handle, _abi.ptr(recs), len(recs)), "rtw_scene_set_lights")

    def lights(self) -> np.ndarray:
        """The registered lights (rtw_scene_lights_get) as OBJECT_DT records."""
        n = C.c_uint32()
        f = _abi.lib().rtw_scene_lights_get
        _abi.check(f(self.handle, None, 0, C.byref(n)), "rtw_scene_lights_get")
        out = np.zeros(n.value, _abi.OBJECT_DT)
        if n.value:
            _abi.check(f(self.handle, out.ctypes.data, n.value, C.byref(n)), "rtw_scene_lights_get")
        return out

    def set_vertex_attrs(self, quads, attrs=None) -> None:
        """rtw_scene_set_vertex_attrs: per-vertex normals / uvs of triangles -- quad indices and as many
        VERTEX_ATTR_DT records, or None / empty to clear (the world then renders exactly as one never given any).
        Replaces the registered set.  Must not race a render on this world."""
        q = np.zeros(0, np.uint32) if quads is None else np.ascontiguousarray(quads, dtype=np.uint32).reshape(-1)
        a = np.zeros(0, _abi.VERTEX_ATTR_DT) if attrs is None else np.ascontiguousarray(attrs, dtype=_abi.VERTEX_ATTR_DT).reshape(-1)
        if len(q) != len(a):
            raise ValueError("set_vertex_attrs: one record per quad index")
        _abi.check(_abi.lib().rtw_scene_set_vertex_attrs(self.handle, _abi.ptr(q), _abi.ptr(a), len(q)),
                   "rtw_scene_set_vertex_attrs")

    def vertex_attrs(self) -> tuple:
        """The registered vertex attributes (rtw_scene_vertex_attrs_get): (quad indices, VERTEX_ATTR_DT records),
        the normals as stored (unit vectors)."""
        n = C.c_uint32()
        f = _abi.lib().rtw_scene_vertex_attrs_get
        _abi.check(f(self.handle, None, None, 0, C.byref(n)), "rtw_scene_vertex_attrs_get")
        q, a = np.zeros(n.value, np.uint32), np.zeros(n.value, _abi.VERTEX_ATTR_DT)
        if n.value:
            _abi.check(f(self.handle, q.ctypes.data, a.ctypes.data, n.value, C.byref(n)), "rtw_scene_vertex_attrs_get")
        return q, a

    def set_environment(self, env: Optional["Environment"]) -> None:
        """rtw_scene_set_environment: the radiance a ray that leaves the scene collects -- an Environment, or None
        to clear (the world then renders exactly as one never given any).  The map is copied at the call.  Must not
        race a render on this world."""
        f = _abi.lib().rtw_scene_set_environment
        if env is None:
            _abi.check(f(self.handle, None), "rtw_scene_set_environment")
            return
        rec = env.record()
        _abi.check(f(self.handle, C.byref(rec)), "rtw_scene_set_environment")

    def environment(self) -> Optional["Environment"]:
        """The registered environment (rtw_scene_environment_get) as given, or None."""
        f = _abi.lib().rtw_scene_environment_get
        rec = _abi.RtwEnvironment()
        _abi.check(f(self.handle, C.byref(rec), None, 0), "rtw_scene_environment_get")
        if rec.width == 0:
            return None
        rgb = np.zeros((rec.height, rec.width, 3), np.float32)
        _abi.check(f(self.handle, C.byref(rec), rgb.ctypes.data, rgb.size), "rtw_scene_environment_get")
        return Environment(rgb, tuple(rec.scale), rec.rotate_y, bool(rec.flags & _abi.RTW_ENV_SAMPLE))

    def debug_environment(self, dirs=None, draws=None) -> dict:
        """rtw_debug_environment: the device's environment functions on the host.  dirs (N, 3) gives `radiance`
        (N, 3), `pdf` (N,) -- the density of the map's own sampler, D / sin(theta), 0 with sampling off -- and
        `texel` (N,), row * width + column; draws (N, 2) = (a, b) gives `sampled_dir` (N, 3)."""
        d = None if dirs is None else np.ascontiguousarray(dirs, np.float32).reshape(-1, 3)
        u = None if draws is None else np.ascontiguousarray(draws, np.float32).reshape(-1, 2)
        if d is not None and u is not None and len(d) != len(u):
            raise ValueError("debug_environment: as many draws as directions")
        n = len(d) if d is not None else len(u) if u is not None else 0
        out = {}
        if d is not None:
            out = {"radiance": np.zeros((n, 3), np.float32), "pdf": np.zeros(n, np.float32),
                   "texel": np.zeros(n, np.uint32)}
        if u is not None:
            out["sampled_dir"] = np.zeros((n, 3), np.float32)
        p = _abi.ptr
        _abi.check(_abi.lib().rtw_debug_environment(self.handle, n, p(d), p(u), p(out.get("radiance")),
                                                    p(out.get("pdf")), p(out.get("sampled_dir")), p(out.get("texel"))),
                   "rtw_debug_environment")
        return out

    def debug_tile_lists(self, cam, pix_begin: int = 0, pix_end: Optional[int] = None, builder: int = 0,
                         cap: int = 0) -> tuple:
        """rtw_debug_tile_lists: the camera-ray candidate lists a render of pixels [pix_begin, pix_end) with `cam`
        (a Camera, initialised on demand, or an RtwCamera) would build, by builder 0 (the one a render picks), 1
        (the flat scan) or 2 (the frustum walk) at cap 0 (the world's) or 2..128.  Returns (counts, ids, tlow,
        centres, rr, n_tx, row0): counts (T,) uint32, 0xFFFFFFFF for a tile that walks the tree; per tile and slot
        k < cap the leaf index ids (T, cap) uint32 (0xFFFFFFFF: never written), the bound tlow (T, cap) float32, the
        stored centres (T, cap, 3) and squared radii rr (T, cap) float32; tile t covers x in 8 (t % n_tx) .. +7 and
        rows row0 + 8 (t // n_tx) .. +7.  GPU worlds of static spheres only."""
        c = cam
        if not isinstance(cam, _abi.RtwCamera):
            if cam.derived is None:
                cam.init()
            c = cam.derived
        end = int(c.size) if pix_end is None else int(pix_end)
        if not 0 <= pix_begin < end <= c.size:
            raise ValueError("debug_tile_lists: empty pixel range or out of the image")
        w = int(c.image_width)
        tiles = ((w + 7) // 8) * (((end - 1) // w - pix_begin // w + 1 + 7) // 8)
        width = int(cap) if cap else 128
        counts = np.zeros(tiles, np.uint32)
        raw = np.zeros((tiles, width, 8), np.uint32)
        n, n_tx, row0 = C.c_uint32(), C.c_uint32(), C.c_uint32()
        _abi.check(_abi.lib().rtw_debug_tile_lists(self.handle, C.byref(c), pix_begin, end, builder, cap, C.byref(n),
                                                   C.byref(n_tx), C.byref(row0), counts.ctypes.data, raw.ctypes.data,
                                                   tiles), "rtw_debug_tile_lists")
        assert n.value == tiles
        if not cap:  # the world's cap (rtw_tuning.tile_lists): what the call wrote is (tiles, that cap, 8), packed
            width = min(self._tile_lists, 128) if self._tile_lists != 1 else 32 if self.stats()["n_nodes"] <= 4096 else 128
            raw = raw.reshape(-1)[:tiles * width * 8].reshape(tiles, width, 8)
        f = raw.view(np.float32)
        return counts, raw[:, :, 4].copy(), f[:, :, 5].copy(), f[:, :, 0:3].copy(), f[:, :, 3].copy(), n_tx.value, row0.value

    def render_guides(self, cam) -> tuple:
        """rtw_render_guides: the first-hit guide buffers of the camera's frame, (albedo, normal_depth), each a
        float32 (W * H, 4) array in image order.  One deterministic ray per pixel through its centre (no jitter, no
        defocus, time 0, no seed); media are transparent.  albedo.w = 1 on a hit, 0 on a miss (rgb = the
        background); normal_depth = (normal towards the ray, depth > 0) on a hit, 0 on a miss.  cam: a Camera (initialised on
        demand) or an RtwCamera."""
        c = cam
        if not isinstance(cam, _abi.RtwCamera):
            if cam.derived is None:
                cam.init()
            c = cam.derived
        albedo = np.zeros((c.size, 4), np.float32)
        nd = np.zeros((c.size, 4), np.float32)
        _abi.check(_abi.lib().rtw_render_guides(self.handle, C.byref(c), albedo.ctypes.data, nd.ctypes.data),
                   "rtw_render_guides")
        return albedo, nd

    def denoise(self, accum: np.ndarray, guides, width: int, height: int, out: Optional[np.ndarray] = None,
                **params) -> np.ndarray:
        """rtw_denoise: the edge-avoiding a-trous filter over the float4 accumulator `accum` (W * H, 4), guided by
        guides = (albedo, normal_depth) of render_guides (albedo may be None without demodulation).  params:
        rtw_denoise_params fields over rtw_denoise_defaults() -- passes, sigma_color, sigma_normal, sigma_depth,
        flags, or demodulate=True / False.  Returns a new accumulator-form array (rgb = mean * w, w), or fills
        `out`, which may be `accum` itself."""
        albedo, nd = guides
        p = _abi.denoise_params(**params)
        n = int(width) * int(height)

        def plane(a, name):
            if a is None:
                return None
            a = np.ascontiguousarray(a, dtype=np.float32)
            if a.size != 4 * n:
                raise ValueError(f"denoise: {name} is not float4[{width} * {height}]")
            return a
        acc, albedo, nd = plane(accum, "accum"), plane(albedo, "albedo"), plane(nd, "normal_depth")
        if out is None:
            out = np.empty((n, 4), np.float32)
        if not (isinstance(out, np.ndarray) and out.flags["C_CONTIGUOUS"] and out.flags["WRITEABLE"]
                and out.dtype == np.float32 and out.size == 4 * n):
            raise ValueError(f"denoise: out is not a writable contiguous float32 float4[{width} * {height}]")
        _abi.check(_abi.lib().rtw_denoise(self.handle, width, height, _abi.ptr(acc), _abi.ptr(albedo), _abi.ptr(nd),
                                          C.byref(p), out.ctypes.data), "rtw_denoise")
        return out

    # ---- noise estimates and the guided filter (DESIGN.md §Noise estimates and the guided filter)
    @staticmethod
    def _frame(a, words: int, name: str, writable: bool = False) -> np.ndarray:
        if not (isinstance(a, np.ndarray) and a.flags["C_CONTIGUOUS"] and a.dtype == np.float32 and a.size == words
                and (a.flags["WRITEABLE"] or not writable)):
            raise ValueError(f"{name} is not a contiguous float32 array of {words} words")
        return a

    def moments_update(self, accum: np.ndarray, moments: np.ndarray, width: int, height: int) -> np.ndarray:
        """rtw_moments_update: fold what `accum` (W * H, 4) gained since the last update into `moments`
        (2, W * H, 4) -- plane 0 the accumulator then, plane 1 (mean, M2, n, sw) of the per-batch mean luminance; all
        zeros is the reset state -- in place.  Returns `moments`."""
        n = int(width) * int(height)
        self._frame(accum, 4 * n, "moments_update: accum")
        self._frame(moments, 8 * n, "moments_update: moments", writable=True)
        _abi.check(_abi.lib().rtw_moments_update(self.handle, width, height, accum.ctypes.data, moments.ctypes.data),
                   "rtw_moments_update")
        return moments

    def noise_estimate(self, moments: np.ndarray, width: int, height: int, threshold: float = 0.05,
                       floor: float = 0.01) -> tuple:
        """rtw_noise_estimate: (err, tile_max, summary) -- err (W * H,) = sqrt(v) / (|mean| + floor), +inf where the
        variance is unknown (fewer than two batches); tile_max (ceil(H / 8), ceil(W / 8)) its maximum over each
        8 x 8 tile; summary an RtwNoiseSummary: over (pixels with err > threshold), known, max_err."""
        n = int(width) * int(height)
        self._frame(moments, 8 * n, "noise_estimate: moments")
        err = np.empty(n, np.float32)
        tiles = np.empty(((height + 7) // 8, (width + 7) // 8), np.float32)
        s = _abi.RtwNoiseSummary()
        _abi.check(_abi.lib().rtw_noise_estimate(self.handle, width, height, moments.ctypes.data, floor, threshold,
                                                 err.ctypes.data, tiles.ctypes.data, C.byref(s)), "rtw_noise_estimate")
        return err, tiles, s

    def denoise_guided(self, accum: np.ndarray, moments: np.ndarray, guides, width: int, height: int,
                       variance: bool = False, out: Optional[np.ndarray] = None, **params):
        """rtw_denoise_guided: the variance-guided a-trous filter over `accum` with the moments of moments_update;
        guides and `out` as denoise().  params: rtw_denoise_params fields over rtw_denoise_guided_defaults()
        (sigma_color in standard deviations).  Returns the accumulator-form result, or with variance=True
        (result, variance_out): the variance of the filtered mean luminance, -1 where unknown."""
        albedo, nd = guides
        p = _abi.denoise_guided_params(**params)
        n = int(width) * int(height)
        acc = self._frame(np.ascontiguousarray(accum, np.float32), 4 * n, "denoise_guided: accum")
        nd = self._frame(np.ascontiguousarray(nd, np.float32), 4 * n, "denoise_guided: normal_depth")
        if albedo is not None:
            albedo = self._frame(np.ascontiguousarray(albedo, np.float32), 4 * n, "denoise_guided: albedo")
        self._frame(moments, 8 * n, "denoise_guided: moments")
        if out is None:
            out = np.empty((n, 4), np.float32)
        self._frame(out, 4 * n, "denoise_guided: out", writable=True)
        var = np.empty(n, np.float32) if variance else None
        _abi.check(_abi.lib().rtw_denoise_guided(self.handle, width, height, _abi.ptr(acc), moments.ctypes.data,
                                                 _abi.ptr(albedo), _abi.ptr(nd), C.byref(p), out.ctypes.data,
                                                 _abi.ptr(var)), "rtw_denoise_guided")
        return (out, var) if variance else out

    # ---- temporal reprojection (rtw_temporal_accumulate; DESIGN.md §Temporal reprojection)
    @staticmethod
    def _derived(cam) -> "_abi.RtwCamera":
        if isinstance(cam, _abi.RtwCamera):
            return cam
        if cam.derived is None:
            cam.init()
        return cam.derived

    def temporal_accumulate(self, cur_cam, prev_cam, cur_accum: np.ndarray, cur_normal_depth: np.ndarray,
                            prev_accum: np.ndarray, prev_normal_depth: np.ndarray,
                            prev_moments: Optional[np.ndarray] = None, out: Optional[np.ndarray] = None,
                            **params) -> tuple:
        """rtw_temporal_accumulate: carry the previous camera's accumulator (and moments) onto the current camera's
        frame and add the current frame's samples.  cur_* / prev_*: float32 (W * H, 4) accumulators and the
        normal_depth guides of render_guides for the two cameras (Camera or RtwCamera); prev_moments: (2, W * H, 4)
        or None.  params: rtw_temporal_params fields over rtw_temporal_defaults().  Returns (accum, moments | None,
        history): history (W * H,) is the weight in samples each pixel took over.  out: where to put accum; it may be
        cur_accum itself."""
        cc, pc = self._derived(cur_cam), self._derived(prev_cam)
        n = int(cc.size)
        p = _abi.temporal_params(**params)
        for a, name in ((cur_accum, "cur_accum"), (cur_normal_depth, "cur_normal_depth"), (prev_accum, "prev_accum"),
                        (prev_normal_depth, "prev_normal_depth")):
            self._frame(a, 4 * n, f"temporal_accumulate: {name}")
        mom = None
        if prev_moments is not None:
            self._frame(prev_moments, 8 * n, "temporal_accumulate: prev_moments")
            mom = np.empty((2, n, 4), np.float32)
        if out is None:
            out = np.empty((n, 4), np.float32)
        self._frame(out, 4 * n, "temporal_accumulate: out", writable=True)
        hist = np.empty(n, np.float32)
        _abi.check(_abi.lib().rtw_temporal_accumulate(
            self.handle, C.byref(cc), C.byref(pc), cur_accum.ctypes.data, cur_normal_depth.ctypes.data,
            prev_accum.ctypes.data, prev_normal_depth.ctypes.data, _abi.ptr(prev_moments), C.byref(p), out.ctypes.data,
            _abi.ptr(mom), hist.ctypes.data), "rtw_temporal_accumulate")
        return out, mom, hist

    def temporal_accumulate_device(self, cur_cam, prev_cam, cur_accum, cur_normal_depth, prev_accum,
                                   prev_normal_depth, prev_moments=None, out=None, stream=None, **params) -> tuple:
        """rtw_temporal_accumulate_device on torch CUDA tensors, shaped as temporal_accumulate's arrays.  Returns
        (accum, moments | None, history) tensors.  stream=None: on torch's current stream, finished on return; a
        torch.cuda.Stream: enqueued there, not synchronised."""
        import torch
        cc, pc = self._derived(cur_cam), self._derived(prev_cam)
        n = int(cc.size)
        p = _abi.temporal_params(**params)

        def frame(t, words, name):
            if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()
                    and t.numel() == words and t.device.index == self.device):
                raise ValueError(f"temporal_accumulate_device: {name} is not a contiguous float32 tensor of {words} "
                                 f"words on device {self.device}")
            return t
        for t, name in ((cur_accum, "cur_accum"), (cur_normal_depth, "cur_normal_depth"), (prev_accum, "prev_accum"),
                        (prev_normal_depth, "prev_normal_depth")):
            frame(t, 4 * n, name)
        dev = cur_accum.device
        mom = None
        if prev_moments is not None:
            frame(prev_moments, 8 * n, "prev_moments")
            mom = torch.empty((2, n, 4), dtype=torch.float32, device=dev)
        if out is None:
            out = torch.empty((n, 4), dtype=torch.float32, device=dev)
        frame(out, 4 * n, "out")
        hist = torch.empty(n, dtype=torch.float32, device=dev)
        if stream is None:
            handle, flags = torch.cuda.current_stream(dev).cuda_stream, 0
        else:
            handle, flags = stream.cuda_stream, _abi.RTW_RENDER_NO_SYNC
        _abi.check(_abi.lib().rtw_temporal_accumulate_device(
            self.handle, C.byref(cc), C.byref(pc), cur_accum.data_ptr(), cur_normal_depth.data_ptr(),
            prev_accum.data_ptr(), prev_normal_depth.data_ptr(),
            prev_moments.data_ptr() if prev_moments is not None else None, C.byref(p), out.data_ptr(),
            mom.data_ptr() if mom is not None else None, hist.data_ptr(), C.c_void_p(handle), flags),
            "rtw_temporal_accumulate_device")
        return out, mom, hist

    # ---- ray queries (rtw_trace_rays / rtw_occluded; DESIGN.md §Ray queries)
    @staticmethod
    def _rays(origins, dirs, tmax, time) -> np.ndarray:
        if isinstance(origins, np.ndarray) and origins.dtype == _abi.RAY_DTYPE:
            if dirs is not None or tmax is not None or time is not None:
                raise ValueError("ray records carry their own dir, tmax and time")
            return np.ascontiguousarray(origins).reshape(-1)
        return _abi.rays(origins, dirs, tmax, time)

    def trace(self, origins, dirs=None, tmax=None, time=None) -> np.ndarray:
        """rtw_trace_rays: the closest hit of every ray on (0.001, tmax), as HIT_DTYPE records (a miss: t = inf,
        kind = RTW_HIT_NONE).  origins, dirs: (N, 3); tmax (default inf) and time (default 0): scalars or one per
        ray -- or `origins` alone as RAY_DTYPE records.  The walk and the hit record of a render's first bounce;
        media are transparent."""
        r = self._rays(origins, dirs, tmax, time)
        hits = np.zeros(len(r), _abi.HIT_DTYPE)
        _abi.check(_abi.lib().rtw_trace_rays(self.handle, len(r), _abi.ptr(r), _abi.ptr(hits)), "rtw_trace_rays")
        return hits

    def occluded(self, origins, dirs=None, tmax=None, time=None) -> np.ndarray:
        """rtw_occluded: a bool per ray, True if any surface is hit on (0.001, tmax).  Arguments as trace()."""
        r = self._rays(origins, dirs, tmax, time)
        out = np.zeros(len(r), np.uint8)
        _abi.check(_abi.lib().rtw_occluded(self.handle, len(r), _abi.ptr(r), _abi.ptr(out)), "rtw_occluded")
        return out.astype(bool)

    def _query_device(self, name, rays, out, words, dtype, stream):
        import torch
        if not (isinstance(rays, torch.Tensor) and rays.is_cuda and rays.dtype == torch.float32 and rays.dim() == 2
                and rays.shape[1] == 8 and rays.is_contiguous()):
            raise ValueError(f"{name}: rays is not a contiguous (N, 8) float32 CUDA tensor")
        if rays.device.index != self.device:
            raise ValueError(f"{name}: rays live on {rays.device}, the world on device {self.device}")
        n = rays.shape[0]
        shape = (n, words) if words > 1 else (n,)
        if out is None:
            out = torch.empty(shape, dtype=dtype, device=rays.device)
        if not (isinstance(out, torch.Tensor) and out.device == rays.device and out.dtype == dtype
                and tuple(out.shape) == shape and out.is_contiguous()):
            raise ValueError(f"{name}: the output is not a contiguous {shape} {dtype} tensor on {rays.device}")
        if stream is None:
            handle, flags = torch.cuda.current_stream(rays.device).cuda_stream, 0
        else:
            handle, flags = stream.cuda_stream, _abi.RTW_RENDER_NO_SYNC
        fn = getattr(_abi.lib(), name)
        _abi.check(fn(self.handle, n, rays.data_ptr() if n else None, out.data_ptr() if n else None,
                      C.c_void_p(handle), flags), name)
        return out

    def trace_device(self, rays, hits=None, stream=None):
        """rtw_trace_rays_device on torch CUDA tensors: rays (N, 8) float32 -- origin, tmax, dir, time, the words of
        RAY_DTYPE -- gives hits (N, 16) int32, the words of HIT_DTYPE (hit_columns() names them).  stream=None: on
        torch's current stream, finished on return; a torch.cuda.Stream: enqueued there, not synchronised."""
        import torch
        return self._query_device("rtw_trace_rays_device", rays, hits, 16, torch.int32, stream)

    def occluded_device(self, rays, out=None, stream=None):
        """rtw_occluded_device on torch CUDA tensors: rays as trace_device(), out (N,) uint8, 1 = occluded."""
        import torch
        return self._query_device("rtw_occluded_device", rays, out, 1, torch.uint8, stream)

    def close(self):
        if getattr(self, "handle", None) and self.handle.value:
            _abi.lib().rtw_scene_destroy(self.handle)
            self.handle = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def stats(self) -> dict:
        s = _abi.RtwSceneStats()
        _abi.check(_abi.lib().rtw_scene_stats_get(self.handle, C.byref(s)), "rtw_scene_stats_get")
        return {k: getattr(s, k) for k, _ in s._fields_ if not k.startswith("_")}

    def nodes(self) -> np.ndarray:
        n = C.c_uint32()
        _abi.check(_abi.lib().rtw_scene_nodes(self.handle, None, 0, C.byref(n)), "rtw_scene_nodes")
        out = np.zeros(n.value, _abi.NODE_DT)
        _abi.check(_abi.lib().rtw_scene_nodes(self.handle, out.ctypes.data, n.value, C.byref(n)), "rtw_scene_nodes")
        return out


    def instance_nodes(self, i: int) -> np.ndarray:
        """The private BVH of instance i in its object space (rtw_scene_instance_nodes); empty without one."""
        n = C.c_uint32()
        f = _abi.lib().rtw_scene_instance_nodes
        _abi.check(f(self.handle, i, None, 0, C.byref(n)), "rtw_scene_instance_nodes")
        out = np.zeros(n.value, _abi.NODE_DT)
        if n.value:
            _abi.check(f(self.handle, i, out.ctypes.data, n.value, C.byref(n)), "rtw_scene_instance_nodes")
        return out


def ray_rows(origins, dirs, tmax=None, time=None):
    """The (N, 8) float32 tensor World.trace_device() takes, from (N, 3) origin and direction tensors; tmax
    (default inf) and time (default 0): scalars or (N,) tensors."""
    import torch
    n = origins.shape[0]
    r = torch.empty((n, 8), dtype=torch.float32, device=origins.device)
    r[:, 0:3], r[:, 4:7] = origins, dirs
    r[:, 3] = float("inf") if tmax is None else tmax
    r[:, 7] = 0.0 if time is None else time
    return r


def hit_columns(hits) -> dict:
    """The named columns of World.trace_device()'s (N, 16) int32 tensor, as views of it: the fields of HIT_DTYPE --
    t, p, normal, uv as float32, kind, index, member, material, front, prim_kind, prim_index as int32 (RTW_HIT_NONE
    reads -1) --, and `hit`, a bool tensor, True where the ray hit."""
    import torch
    cols = {}
    for name, (first, words, is_float) in _abi.HIT_WORDS.items():
        c = hits[:, first:first + words] if words > 1 else hits[:, first]
        cols[name] = c.view(torch.float32) if is_float else c
    cols["hit"] = cols["kind"] != -1
    return cols


class BVHTree:
    """bvh.zig:17-41 -- ``BVHTree.init(objects, start, end)`` returns a World."""

    @staticmethod
    def init(objects: Sequence, start: int = 0, end: Optional[int] = None, seed: int = 0,
             device: int = 0, bvh_mode: Optional[int] = None) -> World:
        end = len(objects) if end is None else end
        return World(flatten(list(objects[start:end]), bvh_seed=seed, bvh_mode=bvh_mode), device)
