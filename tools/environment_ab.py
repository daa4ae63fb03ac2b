#!/usr/bin/env python3
"""Cost of an environment map at a user's size (profiles/environment/): Cornell-mesh at 600 x 600 x 200 spp and
Book-1 at 1200 x 800 x 100 spp, each with its camera's constant background (what the parent renders: run this side
with RTW_LIB=build/rtw_parent.so too) and, where the library has the feature, under a 2048 x 1024 worlds.sky_sun
with sampling on and off.

    python tools/environment_ab.py <out.jsonl> [rounds]

One JSON line per (scene, mode, round): seconds of the timed render (after a warm-up render of 4 spp), Msamples/s."""
import ctypes as C
import importlib
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
rtw = importlib.import_module("zig-raytracing-weekend_amd")


def scenes():
    yield ("cornell_mesh", lambda: rtw.worlds.cornell_mesh(smooth=True),
           rtw.cornell_camera(image_width=600, spp=200, max_depth=50).init(), "emissive")
    yield ("book1", lambda: rtw.worlds.generate_world(0, "book1"),
           rtw.book1_camera(image_width=1200, aspect_ratio=1.5, spp=100, max_depth=50).init(), None)


def timed(world, cam, spp):
    acc = torch.zeros((cam.size, 4), dtype=torch.float32, device="cuda:0")
    f = rtw.lib().rtw_render_device
    rtw._abi.check(f(world.handle, C.byref(cam.derived), 0, cam.size, 0, 4, 1, acc.data_ptr(), None, None), "warm-up")
    torch.cuda.synchronize()
    acc.zero_()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    rtw._abi.check(f(world.handle, C.byref(cam.derived), 0, cam.size, 0, spp, 1, acc.data_ptr(), None, None), "render")
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    got = acc.cpu().numpy()
    assert np.isfinite(got).all() and (got[:, 3] == spp).all()
    return dt


def main():
    out, rounds = sys.argv[1], int(sys.argv[2]) if len(sys.argv) > 2 else 3
    has_env = hasattr(rtw.lib(), "rtw_scene_set_environment")
    side = "parent" if os.environ.get("RTW_LIB") else "this"
    sky = rtw.worlds.sky_sun(2048, 1024) if has_env else None
    with open(out, "a") as fh:
        for name, objs, cam, lights in scenes():
            spp = cam.derived.samples_per_pixel
            modes = [("background", None)]
            if has_env:
                modes += [("env_sample", rtw.Environment(sky, sample=True)), ("env_no_sample", rtw.Environment(sky, sample=False))]
            for mode, env in modes:
                world = rtw.World(rtw.flatten(objs(), lights=lights), device=0)
                if env is not None:
                    world.set_environment(env)
                for r in range(rounds):
                    dt = timed(world, cam, spp)
                    rec = {"side": side, "scene": name, "mode": mode, "round": r, "seconds": round(dt, 4),
                           "msamples_per_s": round(cam.size * spp / dt / 1e6, 1),
                           "build": rtw.lib().rtw_build_id().decode()}
                    fh.write(json.dumps(rec) + "\n")
                    fh.flush()
                    print(rec)
                world.close()


if __name__ == "__main__":
    main()
