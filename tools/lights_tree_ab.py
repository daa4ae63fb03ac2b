"""Lights on an instance-tree scene (the RTW_F_ALL | RTW_F_TREE | RTW_F_PDF kernels) on the GPU: the 300-sphere tree
instance scene of tests/instance_tree_scenes.py with one more emissive quad and a top-level emissive sphere, 600 x 600
x 64 spp, depth 50, with the quads registered and -- the in-tree library only -- the quads and the sphere.  Warm-up,
5 HIP-event timed repeats, median, and the per-kernel times of one more pass; one JSON line.  With RTW_LIB set (an
A/B build that may predate sphere lights) only the quads arm runs: alternate the two libraries from a shell loop
(profiles/lights/sphere_lights_vs_parent.json, profiles/AB_RECIPES.md).
Usage: [RTW_LIB=build/rtw_parent.so] python tools/lights_tree_ab.py"""
import ctypes as C, importlib, json, os, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")]
import numpy as np, torch
rtw = importlib.import_module("zig-raytracing-weekend_amd")
import instance_tree_scenes as T
W, SPP = 600, 64
objs = T.cluster_objects(rtw) + [rtw.Quad.init([400, 300, 100], [0, 120, 0], [0, 0, 150], rtw.DiffuseLight.fromColor([5, 4, 3])),
                                  rtw.Sphere.init([150, 330, 120], 40, rtw.DiffuseLight.fromColor([3, 4, 5]))]
cam = rtw.Camera(image_width=W, samples_per_pixel=SPP, max_depth=50, **T.CAM_KW).init()
out = {"lib": os.environ.get("RTW_LIB", "in-tree"), "build_id": rtw.lib().rtw_build_id().decode()}
modes = ["emissive"] + (["emissive+spheres"] if "RTW_LIB" not in os.environ else [])
for mode in modes:
    w = rtw.World(rtw.flatten(objs, lights=mode))
    ms = []
    for rep in range(6):
        acc = torch.zeros((cam.size, 4), dtype=torch.float32, device="cuda")
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        rtw._abi.check(rtw.lib().rtw_render_device(w.handle, C.byref(cam.derived), 0, cam.size, 0, SPP, 0, acc.data_ptr(), None, None), "render")
        b.record(); torch.cuda.synchronize()
        if rep: ms.append(a.elapsed_time(b))
    tm = rtw._abi.RtwKernelTiming()
    opts = rtw._abi.render_opts(timing=tm)
    acc = torch.zeros((cam.size, 4), dtype=torch.float32, device="cuda")
    rtw._abi.check(rtw.lib().rtw_render_device(w.handle, C.byref(cam.derived), 0, cam.size, 0, SPP, 0, acc.data_ptr(), None, C.byref(opts)), "render")
    torch.cuda.synchronize()
    out[mode] = {"median_ms": statistics.median(ms), "ms": ms, "finite": bool(torch.isfinite(acc).all()),
                 "kernel_ms": {n: tm.ms[i] for i, n in enumerate(rtw._abi.RTW_K_NAMES) if tm.launches[i]}}
    w.close()
print(json.dumps(out))
