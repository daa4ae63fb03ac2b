"""Scene builders (src/main.zig:88-312) restated on the seeded scene stream,
plus the benchmark configurations of BASELINE.json.

Every builder returns the object list; ``BVHTree.init`` turns it into a GPU
world.  Draw order follows the Zig source exactly (struct-literal fields are
evaluated left to right), so a given seed always yields the same scene.
"""
from __future__ import annotations

import os
from typing import List, Optional, Sequence

import numpy as np

from . import _abi
from .rng import DOMAIN_SCENE, Stream, f32
from .scene import (CheckerTexture, ConstantMedium, Dielectric, DiffuseLight, HittableList, Image, ImageTexture,
                    Lambertian, Mesh, Metal, NoiseTexture, Perlin, Quad, RotateY, SolidColor, Sphere, Translate,
                    Triangle, createBox, quad_triangles)

_HERE = os.path.dirname(os.path.abspath(__file__))


def _length(v: np.ndarray) -> np.float32:
    ls = f32(f32(f32(v[0] * v[0]) + f32(v[1] * v[1])) + f32(v[2] * v[2]))
    return np.sqrt(ls, dtype=np.float32)


def generate_world(seed: int = 0, variant: str = "book1", images: Optional[Sequence[Image]] = None) -> List[Sphere]:
    """generateWorld (src/main.zig:253-312).

    variant "book1": static spheres, solid grey ground, brown (-4,1,0) sphere
    (the Book-1 cover, image.ppm / image2.ppm).  variant "ref_head": exactly
    HEAD -- checker ground (scale 0.32), moving diffuse spheres
    (initMoving, +U[0,0.5)^3), earth image texture on the (-4,1,0) sphere.
    """
    if variant not in ("book1", "ref_head"):
        raise ValueError(variant)
    head = variant == "ref_head"
    s = Stream(seed, DOMAIN_SCENE)
    objs: List[Sphere] = []
    if head:
        checker = CheckerTexture.init(0.32, SolidColor.init([0.2, 0.3, 0.1]), SolidColor.init([0.9, 0.9, 0.9]))
        ground = Lambertian.init(checker)
    else:
        ground = Lambertian.fromColor([0.5, 0.5, 0.5])
    objs.append(Sphere.init([0, -1000, 0], 1000, ground))
    ref = np.array([4, 0.2, 0], np.float32)
    for ai in range(-11, 11):
        for bi in range(-11, 11):
            a, b = f32(ai), f32(bi)
            choose_mat = s.float()
            cx = f32(a + f32(f32(0.9) * s.float()))
            cz = f32(b + f32(f32(0.9) * s.float()))
            center = np.array([cx, f32(f32(0.4) * choose_mat), cz], np.float32)
            if _length(center - ref) > f32(0.9):
                if choose_mat < f32(0.8):
                    albedo = s.vec() * s.vec()
                    mat = Lambertian.fromColor(albedo)
                    if head:
                        d = np.array([s.range(0, 0.5), s.range(0, 0.5), s.range(0, 0.5)], np.float32)
                        objs.append(Sphere.initMoving(center, center + d, f32(f32(0.4) * choose_mat), mat))
                    else:
                        objs.append(Sphere.init(center, f32(f32(0.4) * choose_mat), mat))
                elif choose_mat < f32(0.95):
                    albedo = s.vec_range(0.5, 1)
                    fuzz = s.range(0, 0.5)
                    objs.append(Sphere.init(center, f32(f32(0.5) * choose_mat), Metal.fromColor(albedo, fuzz)))
                else:
                    ir = s.range(1, 2)
                    objs.append(Sphere.init(center, f32(f32(0.3) * choose_mat), Dielectric.init(ir)))
    objs.append(Sphere.init([0, 1, 0], 1.0, Dielectric.init(1.5)))
    if head:
        if not images:
            images = [earth_image()]
        objs.append(Sphere.init([-4, 1, 0], 1.0, Lambertian.init(ImageTexture.init(images, 0))))
    else:
        objs.append(Sphere.init([-4, 1, 0], 1.0, Lambertian.fromColor([0.4, 0.2, 0.1])))
    objs.append(Sphere.init([4, 1, 0], 1.0, Metal.fromColor([0.7, 0.6, 0.5], 0.1)))
    return objs


def stress_world(n: int = 100_000, seed: int = 0) -> List[Sphere]:
    """BASELINE config 4: n random spheres on the Book-1 ground.

    Per sphere, in draw order: choose_mat, x = -50 + 100u, z = -50 + 100u,
    radius = 0.05 + 0.25u, y = radius; then the Book-1 material draws."""
    s = Stream(seed, DOMAIN_SCENE, 4, 0)
    objs: List[Sphere] = [Sphere.init([0, -1000, 0], 1000, Lambertian.fromColor([0.5, 0.5, 0.5]))]
    for _ in range(n):
        choose_mat = s.float()
        x = s.range(-50, 50)
        z = s.range(-50, 50)
        r = s.range(0.05, 0.3)
        center = np.array([x, r, z], np.float32)
        if choose_mat < f32(0.8):
            albedo = s.vec() * s.vec()
            objs.append(Sphere.init(center, r, Lambertian.fromColor(albedo)))
        elif choose_mat < f32(0.95):
            albedo = s.vec_range(0.5, 1)
            fuzz = s.range(0, 0.5)
            objs.append(Sphere.init(center, r, Metal.fromColor(albedo, fuzz)))
        else:
            objs.append(Sphere.init(center, r, Dielectric.init(s.range(1, 2))))
    objs.append(Sphere.init([0, 1, 0], 1.0, Dielectric.init(1.5)))
    objs.append(Sphere.init([-4, 1, 0], 1.0, Lambertian.fromColor([0.4, 0.2, 0.1])))
    objs.append(Sphere.init([4, 1, 0], 1.0, Metal.fromColor([0.7, 0.6, 0.5], 0.1)))
    return objs


def earth_image() -> Image:
    """content/earthmap.jpg decoded by the reference's stb_image v2.28 (forced RGBA),
    committed as tests/golden/earthmap_rgba.npz (sha256 pinned in the tests)."""
    path = os.path.join(os.path.dirname(_HERE), "tests", "golden", "earthmap_rgba.npz")
    return Image.load_npz(path)


def earth_world(images: Optional[Sequence[Image]] = None) -> List[Sphere]:
    """earthWorld (src/main.zig:88-99)."""
    images = images or [earth_image()]
    return [Sphere.init([0, 0, 0], 2, Lambertian.init(ImageTexture.init(images, 0)))]


def two_spheres_world() -> List[Sphere]:
    """twoSpheresWorld (src/main.zig:101-113)."""
    checker = CheckerTexture.init(0.8, SolidColor.init([0.2, 0.3, 0.1]), SolidColor.init([0.9, 0.9, 0.9]))
    mat = Lambertian.init(checker)
    return [Sphere.init([0, -10, 0], 10, mat), Sphere.init([0, 10, 0], 10, mat)]


def two_perlin_world(seed: int = 0) -> List[Sphere]:
    """twoPerlinWorld (src/main.zig:115-125): one NoiseTexture(scale 4) shared by both spheres."""
    mat = Lambertian.init(NoiseTexture.init(4, Perlin.init(seed, 0)))
    return [Sphere.init([0, -1000, 0], 1000, mat), Sphere.init([0, 2, 0], 2, mat)]


def earth_perlin_world(seed: int = 0, images: Optional[Sequence[Image]] = None) -> List[Sphere]:
    """BASELINE config 5: earthmap image-textured sphere + Perlin-noise spheres
    (earthWorld + twoPerlinWorld, src/main.zig:88-125), placed side by side."""
    images = images or [earth_image()]
    noise = Lambertian.init(NoiseTexture.init(4, Perlin.init(seed, 0)))
    return [
        Sphere.init([0, -1000, 0], 1000, noise),
        Sphere.init([0, 2, 2.5], 2, noise),
        Sphere.init([0, 2, -2.5], 2, Lambertian.init(ImageTexture.init(images, 0))),
    ]


def quads_world() -> list:
    """quadsWorld (src/main.zig:127-144): five coloured quads."""
    left_red = Lambertian.init(SolidColor.init([1, 0.2, 0.2]))
    back_green = Lambertian.init(SolidColor.init([0.2, 1.0, 0.2]))
    right_blue = Lambertian.init(SolidColor.init([0.2, 0.2, 1.0]))
    upper_orange = Lambertian.init(SolidColor.init([1.0, 0.5, 0]))
    lower_teal = Lambertian.init(SolidColor.init([0.2, 0.8, 0.8]))
    return [
        Quad.init([-3, -2, 5], [0, 0, -4], [0, 4, 0], left_red),
        Quad.init([-2, -2, 0], [4, 0, 0], [0, 4, 0], back_green),
        Quad.init([3, -2, 1], [0, 0, 4], [0, 4, 0], right_blue),
        Quad.init([-2, -3, 1], [4, 0, 0], [0, 0, 4], upper_orange),
        Quad.init([-2, -3, 5], [4, 0, 0], [0, 0, -4], lower_teal),
    ]


def simple_light_world(seed: int = 0) -> list:
    """simpleLightWorld (src/main.zig:146-166): Perlin spheres lit by a quad and a sphere light
    (camera: camera.simple_light_camera)."""
    mat = Lambertian.init(NoiseTexture.init(4, Perlin.init(seed, 0)))
    difflight = DiffuseLight.init(SolidColor.init([4, 4, 4]))
    return [
        Sphere.init([0, -1000, 0], 1000, mat),
        Sphere.init([0, 2, 0], 2, mat),
        Quad.init([3, 1, -2], [2, 0, 0], [0, 2, 0], difflight),
        Sphere.init([0, 7, 0], 2, difflight),
    ]


def _cornell_walls(light_q, light_u, light_v, light_color):
    red = Lambertian.init(SolidColor.init([0.65, 0.05, 0.05]))
    white = Lambertian.init(SolidColor.init([0.73, 0.73, 0.73]))
    green = Lambertian.init(SolidColor.init([0.12, 0.45, 0.15]))
    light = DiffuseLight.init(SolidColor.init(light_color))
    walls = [
        Quad.init([555, 0, 0], [0, 555, 0], [0, 0, 555], green),
        Quad.init([0, 0, 0], [0, 555, 0], [0, 0, 555], red),
        Quad.init(light_q, light_u, light_v, light),
        Quad.init([0, 0, 0], [555, 0, 0], [0, 0, 555], white),
        Quad.init([555, 555, 555], [-555, 0, 0], [0, 0, -555], white),
        Quad.init([0, 0, 555], [555, 0, 0], [0, 555, 0], white),
    ]
    return walls, white


def cornell_box() -> list:
    """cornellBox (src/main.zig:168-205), HEAD's default scene (camera: camera.cornell_camera)."""
    objs, white = _cornell_walls([343, 554, 332], [-130, 0, 0], [0, 0, -105], [15, 15, 15])
    box1 = createBox([0, 0, 0], [165, 330, 165], white)
    box1 = RotateY.init(box1, 15)
    box1 = Translate.init(box1, [265, 0, 295])
    objs.append(box1)
    box2 = createBox([0, 0, 0], [165, 165, 165], white)
    box2 = RotateY.init(box2, -18)
    box2 = Translate.init(box2, [130, 0, 65])
    objs.append(box2)
    return objs


def cornell_smoke() -> list:
    """cornellBoxSmoke (src/main.zig:207-251): the two boxes as ConstantMedium (density 0.01),
    black and white smoke (camera: camera.cornell_smoke_camera)."""
    objs, white = _cornell_walls([113, 554, 127], [330, 0, 0], [0, 0, 305], [7, 7, 7])
    box1 = Translate.init(RotateY.init(createBox([0, 0, 0], [165, 330, 165], white), 15), [265, 0, 295])
    objs.append(ConstantMedium.initFromColor(box1, 0.01, [0, 0, 0]))
    box2 = Translate.init(RotateY.init(createBox([0, 0, 0], [165, 165, 165], white), -18), [130, 0, 65])
    objs.append(ConstantMedium.initFromColor(box2, 0.01, [1, 1, 1]))
    return objs


def icosphere(level: int, centre, radius, mat, bvh: Optional[bool] = None, smooth: bool = False,
              uv: bool = False) -> Mesh:
    """A sphere of 20 * 4^level triangles (generated, not loaded): the icosahedron, every triangle split in four
    `level` times, the new vertices pushed out to the sphere.  Closed, every edge shared by two triangles, normals
    (cross(b - a, c - a)) outward.  Vertices are computed in float64 and rounded once.

    smooth: per-vertex normals, the vertex directions (the shading normal of a point of a face is then the
    sphere's at the point's direction).  uv: per-corner texture coordinates, the Sphere's own (u, v) of the vertex
    direction (getSphereUV); a face across the u = 1 | 0 seam continues past 1 (an image texture clamps there), and
    a pole vertex, whose u is arbitrary, takes the mean u of its face's other corners."""
    t = (1.0 + 5.0 ** 0.5) / 2.0
    verts = [(-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t), (0, -1, -t), (0, 1, -t),
             (t, 0, -1), (t, 0, 1), (-t, 0, -1), (-t, 0, 1)]
    verts = [np.array(v, np.float64) / np.linalg.norm(v) for v in verts]
    faces = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2),
             (10, 7, 6), (7, 1, 8), (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11),
             (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    for _ in range(level):
        mid = {}

        def midpoint(i, j):
            key = (min(i, j), max(i, j))
            if key not in mid:
                m = verts[i] + verts[j]
                verts.append(m / np.linalg.norm(m))
                mid[key] = len(verts) - 1
            return mid[key]

        split = []
        for a, b, c in faces:
            ab, bc, ca = midpoint(a, b), midpoint(b, c), midpoint(c, a)
            split += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        faces = split
    dirs = np.array(verts)
    faces = np.array(faces, np.int64)
    v = np.asarray(centre, np.float64).reshape(3) + float(radius) * dirs
    uvs = face_uvs = None
    if uv:
        u = (np.arctan2(-dirs[:, 2], dirs[:, 0]) + np.pi) / (2 * np.pi)
        uvs = np.stack([u, np.arccos(np.clip(-dirs[:, 1], -1, 1)) / np.pi], 1)[faces]   # (m, 3, 2) per corner
        pole = np.abs(dirs[:, 1])[faces] > 1 - 1e-12
        for tri, pl in zip(uvs, pole):
            rest = tri[~pl, 0]
            if rest.max() - rest.min() > 0.5:
                rest[rest < 0.5] += 1.0
            tri[~pl, 0] = rest
            tri[pl, 0] = rest.mean()
        uvs = uvs.reshape(-1, 2)
        face_uvs = np.arange(len(uvs)).reshape(-1, 3)
    return Mesh.init(v.astype(np.float32), faces, mat, bvh, normals=dirs if smooth else None, uvs=uvs,
                     face_uvs=face_uvs)


def cornell_mesh(level: int = 2, analytic: bool = False, smooth: bool = False) -> list:
    """The Cornell box (camera: camera.cornell_camera) with triangles in every place a scene can hold them: the
    ceiling light as two emissive triangles, the tall box replaced by an icosphere of 20 * 4^level triangles under
    RotateY + Translate (level 2: 320, an instance with a private BVH), the short box by its 12 triangles (an
    instance tested as a list), and one free-standing top-level triangle.  analytic: the icosphere's place taken by
    the Sphere it approximates (the price of the mesh, for measurements).  smooth: the icosphere with per-vertex
    normals (icosphere(smooth=True))."""
    walls, white = _cornell_walls([343, 554, 332], [-130, 0, 0], [0, 0, -105], [15, 15, 15])
    objs = []
    for q in walls:
        objs += quad_triangles(q) if q.mat.kind == _abi.RTW_MAT_DIFFUSE_LIGHT else [q]
    if analytic:
        ball = HittableList.init()
        ball.add(Sphere.init([82.5, 100, 82.5], 90, white))
    else:
        ball = icosphere(level, [82.5, 100, 82.5], 90, white, smooth=smooth)
    objs.append(Translate.init(RotateY.init(ball, 15), [265, 0, 295]))
    box = HittableList.init()
    for side in createBox([0, 0, 0], [165, 165, 165], white).objects:
        for tri in quad_triangles(side):
            box.add(tri)
    objs.append(Translate.init(RotateY.init(box, -18), [130, 0, 65]))
    objs.append(Triangle.init([300, 10, 60], [420, 10, 90], [350, 150, 120],
                              Lambertian.init(SolidColor.init([0.2, 0.4, 0.8]))))
    return objs


def env_directions(width: int, height: int, sub: int = 1) -> np.ndarray:
    """Unit directions (float64, (height * sub, width * sub, 3)) of an equirectangular map's texels, `sub` x `sub`
    regular sub-samples per texel: row 0 at +y, (u, v) = sphere_uv's, i.e. the inverse of the library's lookup --
    theta = pi (1 - (j + .5) / H), phi = 2 pi (i + .5) / W, d = (-sin(theta) cos(phi), -cos(theta), sin(theta) sin(phi))."""
    hh, ww = height * sub, width * sub
    theta = np.pi * (1.0 - (np.arange(hh) + 0.5) / hh)[:, None]
    phi = 2.0 * np.pi * ((np.arange(ww) + 0.5) / ww)[None, :]
    st = np.sin(theta)
    return np.stack([-st * np.cos(phi), np.broadcast_to(-np.cos(theta), (hh, ww)), st * np.sin(phi)], axis=-1)


def sky_sun(width: int = 512, height: int = 256, sun_dir=(0.3, 0.8, 0.5), sun_radiance=5000.0,
            sun_half_angle: float = 2.0, zenith=(0.25, 0.45, 0.9), horizon=(0.8, 0.85, 0.9)) -> np.ndarray:
    """A procedural HDR sky for Environment: float32 (height, width, 3) linear radiance, row 0 at +y.  The sky
    blends horizon -> zenith by the direction's height (the horizon colour below it); a sun of angular radius
    sun_half_angle (degrees) about sun_dir adds sun_radiance (a scalar or rgb) times the fraction of the texel it
    covers (4 x 4 sub-samples), so a sun smaller than a texel keeps its energy."""
    sub = 4
    d = env_directions(width, height, sub)
    s = np.asarray(sun_dir, np.float64)
    s = s / np.linalg.norm(s)
    inside = (d @ s >= np.cos(np.radians(sun_half_angle))).astype(np.float64)
    cover = inside.reshape(height, sub, width, sub).mean(axis=(1, 3))
    up = np.clip(env_directions(width, height)[..., 1], 0.0, 1.0)[..., None]
    sky = (1.0 - up) * np.asarray(horizon, np.float64) + up * np.asarray(zenith, np.float64)
    sun = np.broadcast_to(np.asarray(sun_radiance, np.float64), (3,))
    return (sky + cover[..., None] * sun).astype(np.float32)


def next_week_world(seed: int = 0, boxes_per_side: int = 20, cluster: int = 1000,
                    images: Optional[Sequence[Image]] = None) -> list:
    """The final scene of *Ray Tracing: The Next Week* (not in the reference's main.zig: "Part 2" is an open
    item of its README), written from the book's description with the reference's objects:

    * boxes_per_side^2 ground boxes of random height (createBox lists at top level);
    * the quad light, a moving sphere, a glass and a metal sphere;
    * a glass ball with a blue medium inside it, and the thin white fog around the whole scene;
    * the earth sphere and a Perlin sphere;
    * ``cluster`` small white spheres as ONE instance, Translate(RotateY(list, 15), (-100, 270, 395)) --
      above 127 members the library walks it through a private BVH (RTW_INST_BVH).

    Draws come from the seeded scene stream (a = 6): box heights first, then the cluster's centres."""
    s = Stream(seed, DOMAIN_SCENE, 6, 0)
    objs: list = []
    ground = Lambertian.fromColor([0.48, 0.83, 0.53])
    w = f32(100.0)
    for i in range(boxes_per_side):
        for j in range(boxes_per_side):
            x0 = f32(f32(-1000.0) + f32(f32(i) * w))
            z0 = f32(f32(-1000.0) + f32(f32(j) * w))
            y1 = s.range(1, 101)
            objs.append(createBox([x0, 0.0, z0], [f32(x0 + w), y1, f32(z0 + w)], ground))
    light = DiffuseLight.fromColor([7, 7, 7])
    objs.append(Quad.init([123, 554, 147], [300, 0, 0], [0, 0, 265], light))
    center1 = np.array([400, 400, 200], np.float32)
    objs.append(Sphere.initMoving(center1, center1 + np.array([30, 0, 0], np.float32), 50,
                                  Lambertian.fromColor([0.7, 0.3, 0.1])))
    objs.append(Sphere.init([260, 150, 45], 50, Dielectric.init(1.5)))
    objs.append(Sphere.init([0, 150, 145], 50, Metal.fromColor([0.8, 0.8, 0.9], 1.0)))
    objs.append(Sphere.init([360, 150, 145], 70, Dielectric.init(1.5)))
    objs.append(ConstantMedium.initFromColor(Sphere.init([360, 150, 145], 70, Dielectric.init(1.5)), 0.2,
                                             [0.2, 0.4, 0.9]))
    objs.append(ConstantMedium.initFromColor(Sphere.init([0, 0, 0], 5000, Dielectric.init(1.5)), 0.0001, [1, 1, 1]))
    if not images:
        images = [earth_image()]
    objs.append(Sphere.init([400, 200, 400], 100, Lambertian.init(ImageTexture.init(images, 0))))
    objs.append(Sphere.init([220, 280, 300], 80, Lambertian.init(NoiseTexture.init(0.2, Perlin.init(seed, 0)))))
    white = Lambertian.fromColor([0.73, 0.73, 0.73])
    balls = HittableList.init()
    for _ in range(cluster):
        balls.add(Sphere.init(s.vec_range(0, 165), 10, white))
    objs.append(Translate.init(RotateY.init(balls, 15), [-100, 270, 395]))
    return objs
