#!/usr/bin/env python3
"""The README's environment-map picture: the smooth icosphere on a floor under worlds.sky_sun, 64 spp, rendered
with the map sampled (left) and not (right), side by side in one PPM.

    python tools/environment_demo.py out.ppm [--device -1] [--width 400] [--spp 64]

--device -1 renders on the host backend (the same bits as a GPU context)."""
import argparse
import ctypes as C
import importlib
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
rtw = importlib.import_module("zig-raytracing-weekend_amd")


def scene(sample):
    white = rtw.Lambertian.fromColor([0.73, 0.73, 0.73])
    floor = rtw.Quad.init([-40, 0, -40], [80, 0, 0], [0, 0, 80], rtw.Lambertian.fromColor([0.5, 0.5, 0.5]))
    ball = rtw.worlds.icosphere(3, [0, 1, 0], 1.0, white, smooth=True)
    env = rtw.Environment(rtw.worlds.sky_sun(1024, 512, (0.5, 0.6, -0.6), 5000.0, 2.0), sample=sample)
    return rtw.flatten([floor, ball], environment=env)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("out")
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--width", type=int, default=400)
    ap.add_argument("--spp", type=int, default=64)
    a = ap.parse_args()
    cam = rtw.Camera(aspect_ratio=1.0, image_width=a.width, samples_per_pixel=a.spp, max_depth=16, vfov=30.0,
                     lookfrom=(0.0, 2.0, -7.0), lookat=(0.0, 0.8, 0.0), defocus_angle=0.0).init()
    halves = []
    for sample in (True, False):
        world = rtw.World(scene(sample), device=a.device)
        buf = np.zeros((cam.size, 4), np.float32)
        rtw._abi.check(rtw.lib().rtw_render(world.handle, C.byref(cam.derived), 0, cam.size, 0, a.spp, 1,
                                            buf.ctypes.data, None, rtw._abi.PROGRESS_FN(0), None), "rtw_render")
        world.close()
        halves.append(buf.reshape(cam.derived.image_height, a.width, 4))
    both = np.concatenate(halves, axis=1)
    rtw.output.write_ppm(a.out, both.reshape(-1, 4), 2 * a.width, cam.derived.image_height)
    print(f"{a.out}: {2 * a.width} x {cam.derived.image_height}, {a.spp} spp, sampled | not sampled")


if __name__ == "__main__":
    main()
