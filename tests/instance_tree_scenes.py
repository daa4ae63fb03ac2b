"""Scenes, cameras and cached oracle references shared by tests/test_instance_tree.py (host backend) and
tests/test_gpu_instance_tree.py (GPU): instances walked through their own BVH (RTW_INST_BVH).

Not a test module.  Every camera here has the constant background (0.7, 0.8, 1.0), so every path carries
radiance (with a black background most pixels of these 4-spp renders would be zero and hide a wrong hit).
References are rendered once per process and never modified (arrays are returned read-only)."""
import ctypes as C
import functools
import os

import numpy as np

CPU = -1
SPP = 4
SEED = 11
CAM_KW = dict(aspect_ratio=1.0, vfov=40.0, lookfrom=(478.0, 278.0, -600.0), lookat=(278.0, 278.0, 0.0),
              defocus_angle=0.0, background=(0.7, 0.8, 1.0))


def pkgs():
    import importlib
    import oracle as O
    O.lib()
    return importlib.import_module("zig-raytracing-weekend_amd"), O


def cameras(W, depth):
    rtw, O = pkgs()
    cam = rtw.Camera(image_width=W, samples_per_pixel=SPP, max_depth=depth, **CAM_KW).init()
    ocam = O.camera(image_width=W, samples_per_pixel=SPP, max_depth=depth, **CAM_KW)
    assert cam.derived.image_height == ocam.image_height
    return cam, ocam


def mode_of(rtw, name):
    return {"sah": rtw._abi.RTW_BVH_SAH, "reference": rtw._abi.RTW_BVH_REFERENCE}[name]


def _light_and_ground(rtw):
    return [rtw.Quad.init([123, 554, 147], [300, 0, 0], [0, 0, 265], rtw.DiffuseLight.fromColor([7, 7, 7])),
            rtw.Sphere.init([278, -1000, 278], 1000, rtw.Lambertian.fromColor([0.48, 0.83, 0.53]))]


def cluster_spheres(rtw, n=300):
    """n spheres of radius 10, centres default_rng(1).random((n, 3)) * 165; every 7th metal or dielectric in turn."""
    centres = (np.random.default_rng(1).random((n, 3)) * 165).astype(np.float32)
    out = []
    for i, c in enumerate(centres):
        if i % 7 == 0:
            mat = rtw.Metal.fromColor([0.8, 0.8, 0.9], 0.1) if (i // 7) % 2 == 0 else rtw.Dielectric.init(1.5)
        else:
            mat = rtw.Lambertian.fromColor([0.73, 0.73, 0.73])
        out.append(rtw.Sphere.init(c, 10, mat))
    return out


def cluster_objects(rtw, chunks=1, bvh=None):
    """The cluster scene: light, ground, and the 300 spheres under Translate(RotateY(list, 15), (-100, 270, 395)):
    one instance (a tree: more than 127 members), or `chunks` list instances of 300 / chunks under the same
    transforms -- the form every version of the library accepts."""
    objs = _light_and_ground(rtw)
    spheres = cluster_spheres(rtw)
    per = len(spheres) // chunks
    for k in range(chunks):
        lst = rtw.HittableList.init(bvh)
        for s in spheres[k * per:(k + 1) * per]:
            lst.add(s)
        objs.append(rtw.Translate.init(rtw.RotateY.init(lst, 15), [-100, 270, 395]))
    return objs


def medium_objects(rtw):
    """A ConstantMedium bounded by a 150-sphere tree instance (boundary queries on (-inf, inf) and (t1 + 1e-4, inf))."""
    centres = (np.random.default_rng(2).random((150, 3)) * np.array([120, 60, 120])).astype(np.float32)
    lst = rtw.HittableList.init()
    white = rtw.Lambertian.fromColor([0.73, 0.73, 0.73])
    for c in centres:
        lst.add(rtw.Sphere.init(c, 25, white))
    return _light_and_ground(rtw) + [
        rtw.ConstantMedium.initFromColor(rtw.Translate.init(lst, [100, 380, 100]), 0.02, [1, 1, 1])]


def rotated12_objects(rtw, bvh):
    """A 12-sphere rotated instance (one moving member), flagged or not."""
    centres = (np.random.default_rng(3).random((12, 3)) * 150).astype(np.float32)
    lst = rtw.HittableList.init(bvh)
    for i, c in enumerate(centres):
        mat = rtw.Lambertian.fromColor([0.2 + 0.06 * i, 0.5, 0.9 - 0.06 * i])
        if i == 5:
            lst.add(rtw.Sphere.initMoving(c, c + np.array([20, 5, 0], np.float32), 30, mat))
        else:
            lst.add(rtw.Sphere.init(c, 30, mat))
    return _light_and_ground(rtw) + [rtw.Translate.init(rtw.RotateY.init(lst, 30), [150, 200, 250])]


def cornell_arrays(rtw, bvh, mode="sah"):
    """cornell_box() with RTW_INST_BVH set on both boxes or not (box sides share edges: exact quad ties)."""
    arr = rtw.flatten(rtw.worlds.cornell_box(), bvh_mode=mode_of(rtw, mode))
    if bvh:
        arr.instances["flags"] |= rtw._abi.RTW_INST_BVH
    return arr


def final_objects(rtw):
    """The reduced Next Week final scene: 6 x 6 ground boxes, a 200-sphere cluster."""
    return rtw.worlds.next_week_world(0, boxes_per_side=6, cluster=200)


def arrays(rtw, name, mode="sah"):
    build = {"cluster": lambda: cluster_objects(rtw), "cluster3": lambda: cluster_objects(rtw, 3),
             "medium": lambda: medium_objects(rtw), "rot12_tree": lambda: rotated12_objects(rtw, True),
             "rot12_list": lambda: rotated12_objects(rtw, False), "final": lambda: final_objects(rtw)}
    if name == "cornell_tree":
        return cornell_arrays(rtw, True, mode)
    if name == "cornell_list":
        return cornell_arrays(rtw, False, mode)
    return rtw.flatten(build[name](), bvh_mode=mode_of(rtw, mode))


# name -> (image width, max depth)
SHAPES = {"cluster": (64, 50), "cluster3": (64, 50), "medium": (64, 50), "rot12_tree": (64, 50), "rot12_list": (64, 50),
          "cornell_tree": (64, 50), "cornell_list": (64, 50), "final": (96, 40)}


def render(rtw, arr, cam, device=CPU, tuning=None):
    world = rtw.World(arr, device=device, tuning=tuning)
    buf = np.zeros((cam.size, 4), np.float32)
    rc = rtw.lib().rtw_render(world.handle, C.byref(cam.derived), 0, cam.size, 0, SPP, SEED, buf.ctypes.data, None,
                              rtw._abi.PROGRESS_FN(0), None)
    rtw._abi.check(rc, "rtw_render")
    world.close()
    return buf


@functools.lru_cache(maxsize=None)
def oracle_image(name, mode="reference"):
    """The oracle's render of scene `name` (the reference's own tree: the topology only decides exact ties)."""
    rtw, O = pkgs()
    arr = arrays(rtw, name, mode)
    cam, ocam = cameras(*SHAPES[name])
    ref = O.World.from_arrays(arr).render_pixels(ocam, SEED, np.arange(cam.size, dtype=np.uint32), 0, SPP,
                                                 threads=min(os.cpu_count() or 1, 16))
    ref.setflags(write=False)
    return ref


@functools.lru_cache(maxsize=None)
def host_image(name, mode="sah"):
    """The host backend's render of scene `name`."""
    rtw, _ = pkgs()
    cam, _ = cameras(*SHAPES[name])
    out = render(rtw, arrays(rtw, name, mode), cam)
    out.setflags(write=False)
    return out


def close(got, ref, rel):
    return np.abs(got - ref) <= rel * np.maximum(1.0, np.abs(ref))
