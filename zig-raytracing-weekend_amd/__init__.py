"""zig-raytracing-weekend_amd -- MI355X-native drop-in for the per-pixel sample
loop of dariooddenino/zig-raytracing-weekend (src/camera.zig:93-208).

Host API (mirrors the reference's Zig API names):
  scene:   SolidColor, CheckerTexture, ImageTexture, NoiseTexture, Perlin,
           Lambertian, Metal, Dielectric, DiffuseLight, Isotropic,
           Sphere.init / Sphere.initMoving, Quad.init, Triangle.init, Mesh.init, load_obj,
           BVHTree.init -> World;
           flatten(objs, lights="emissive" | "emissive+spheres") / World.set_lights: light importance sampling
           Triangle.init(..., normals=, uvs=), Mesh.init(..., normals=, uvs=), load_obj(..., attributes=True) /
           World.set_vertex_attrs: smooth shading and mesh UVs
           Environment(rgb, scale, rotate_y, sample) / Environment.load_hdr, flatten(objs, environment=) /
           World.set_environment: image-based lighting, importance-sampled (worlds.sky_sun: a procedural sky)
           World.trace / World.occluded (numpy), World.trace_device / World.occluded_device (torch; ray_rows,
           hit_columns): closest-hit and occlusion queries for the caller's own rays
  camera:  Camera (+ init, render(state, task)), SharedStateImageWriter, Task,
           RayTraceState, start_render
  worlds:  generate_world, earth_world, two_spheres_world, two_perlin_world,
           stress_world, earth_perlin_world, cornell_box, cornell_smoke, icosphere, cornell_mesh
The hot path runs in librtw_gpu.so (include/rtw_gpu.h) on gfx950.
"""
from . import _abi, configs, distributed, output, rng, worlds  # noqa: F401
from ._abi import RtwError, lib  # noqa: F401
from .camera import (Camera, RayTraceState, SharedStateImageWriter, Task, book1_camera,  # noqa: F401
                     cornell_camera, cornell_smoke_camera, earth_perlin_camera, next_week_camera, progressive_render,
                     simple_light_camera, start_render)
from .scene import (BVHTree, CheckerTexture, ConstantMedium, Dielectric, DiffuseLight, Environment,  # noqa: F401
                    HittableList, Image, ImageTexture, Isotropic, Lambertian, Mesh, Metal, NoiseTexture, Perlin, Quad,
                    RotateY, SceneArrays, SolidColor, Sphere, Translate, Triangle, World, createBox, flatten,
                    hit_columns, load_obj, quad_triangles, ray_rows)
