"""The scene image a host context builds (rtw_scene_create_ex on RTW_DEVICE_CPU) against recorded values.

Scene creation lays the scene out as one blob, section by section; its hash, its size and the world tree's node
count must not move when the host runtime is restructured.  tests/golden/host_scene_image.json holds, per scene,
`hash` (rtw_scene_hash after the scene's lights / vertex attributes are registered), `device_bytes` and `n_nodes`
(rtw_scene_stats) as commit 617f84d ("Wavefront dispatch: one grid cache, launch helper, plan and class table")
built them.  To re-record (only when a change means to alter the image), build the library at the commit whose
values are wanted and run

    RTW_LIB=<that librtw_gpu.so> python tests/test_host_scene_image.py record > tests/golden/host_scene_image.json

`python tests/test_host_scene_image.py dump` prints the full comparison record of the library in RTW_LIB (every
stats field, digests of rtw_scene_nodes / rtw_scene_instance_nodes, the registered lights and vertex attributes
read back, the digest of a 32 x 32, 4 spp host render) for an A/B of two builds: diff the two outputs.
"""
import ctypes as C
import hashlib
import json
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "host_scene_image.json")
CPU = -1  # RTW_DEVICE_CPU


def _earth(rtw):
    with np.load(os.path.join(HERE, "golden", "earthmap_rgba.npz"), allow_pickle=False) as z:
        return [rtw.Image(np.ascontiguousarray(z["rgba"]))]


def _cluster(rtw):
    """Light, ground and one rotated, translated instance of 300 spheres (more than 127 members: its own tree)."""
    objs = [rtw.Quad.init([123, 554, 147], [300, 0, 0], [0, 0, 265], rtw.DiffuseLight.fromColor([7, 7, 7])),
            rtw.Sphere.init([278, -1000, 278], 1000, rtw.Lambertian.fromColor([0.48, 0.83, 0.53]))]
    lst = rtw.HittableList.init(None)
    for c in (np.random.default_rng(1).random((300, 3)) * 165).astype(np.float32):
        lst.add(rtw.Sphere.init(c, 10, rtw.Lambertian.fromColor([0.73, 0.73, 0.73])))
    return objs + [rtw.Translate.init(rtw.RotateY.init(lst, 15), [-100, 270, 395])]


def _book1_cam(rtw):
    return rtw.book1_camera(image_width=32, aspect_ratio=1.0, spp=4, max_depth=50)


def _cornell_cam(rtw):
    return rtw.cornell_camera(image_width=32, spp=4, max_depth=50)


# name -> (SceneArrays builder, camera builder)
SCENES = {
    "book1_sah": (lambda r: r.flatten(r.worlds.generate_world(0, "book1")), _book1_cam),
    "book1_reference": (lambda r: r.flatten(r.worlds.generate_world(0, "book1"), bvh_seed=3,
                                            bvh_mode=r._abi.RTW_BVH_REFERENCE), _book1_cam),
    "moving_head": (lambda r: r.flatten(r.worlds.generate_world(0, "ref_head", _earth(r))), _book1_cam),
    "earth_perlin": (lambda r: r.flatten(r.worlds.earth_perlin_world(0, _earth(r))),
                     lambda r: r.earth_perlin_camera(image_width=32, spp=4)),
    "cornell": (lambda r: r.flatten(r.worlds.cornell_box(), lights="emissive"), _cornell_cam),
    "cornell_smoke": (lambda r: r.flatten(r.worlds.cornell_smoke()), _cornell_cam),
    "cornell_mesh2_flat": (lambda r: r.flatten(r.worlds.cornell_mesh(2), lights="emissive"), _cornell_cam),
    "cornell_mesh2_smooth": (lambda r: r.flatten(r.worlds.cornell_mesh(2, smooth=True), lights="emissive"),
                             _cornell_cam),
    "cluster300": (lambda r: r.flatten(_cluster(r)), _cornell_cam),
}


def _hash(rtw, world):
    h = C.c_uint64()
    rtw._abi.check(rtw.lib().rtw_scene_hash(world.handle, C.byref(h)), "rtw_scene_hash")
    return f"{h.value:016x}"


def image_record(rtw, name):
    world = rtw.World(SCENES[name][0](rtw), device=CPU)
    try:
        st = world.stats()
        return {"hash": _hash(rtw, world), "device_bytes": int(st["device_bytes"]), "n_nodes": int(st["n_nodes"])}
    finally:
        world.close()


def full_record(rtw, name):
    def sha(a):
        return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()[:16]

    arr = SCENES[name][0](rtw)
    world = rtw.World(arr, device=CPU)
    try:
        rec = {"hash": _hash(rtw, world), "stats": {k: (float(v) if isinstance(v, float) else int(v))
                                                    for k, v in world.stats().items()}}
        rec["nodes"] = sha(world.nodes())
        rec["instance_nodes"] = [sha(world.instance_nodes(i)) for i in range(len(arr.instances))]
        rec["lights"] = [[int(o["kind"]), int(o["index"])] for o in world.lights()]
        q, a = world.vertex_attrs()
        rec["vertex_attrs"] = [len(q), sha(q), sha(a)]
        cam = SCENES[name][1](rtw).init()
        buf = np.zeros((cam.size, 4), np.float32)
        rtw._abi.check(rtw.lib().rtw_render(world.handle, C.byref(cam.derived), 0, cam.size, 0, 4, 7, buf.ctypes.data,
                                            None, rtw._abi.PROGRESS_FN(0), None), "rtw_render")
        rec["render_32x32x4"] = sha(buf)
        return rec
    finally:
        world.close()


@pytest.mark.parametrize("name", sorted(SCENES))
def test_host_scene_image_is_the_recorded_one(rtw, name):
    with open(GOLDEN) as f:
        want = json.load(f)[name]
    assert image_record(rtw, name) == want


if __name__ == "__main__":
    import importlib
    sys.path.insert(0, os.path.dirname(HERE))
    pkg = importlib.import_module("zig-raytracing-weekend_amd")
    make = {"record": image_record, "dump": full_record}[sys.argv[1]]
    print(json.dumps({n: make(pkg, n) for n in sorted(SCENES)}, indent=1, sort_keys=True))
