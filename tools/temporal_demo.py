#!/usr/bin/env python3
"""What carrying the history across a camera move buys: a short Cornell orbit as a strip.  One column per frame; top
to bottom the frame's own samples alone, those under the guided filter, and the temporal accumulation
(RayTraceState.move_camera) under the guided filter.

    python tools/temporal_demo.py out.png [--device -1] [--width 160] [--frames 6] [--spp 2] [--step 2.0]

--device -1 renders on the host backend (the same bits as a GPU context)."""
import argparse
import ctypes as C
import importlib
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
rtw = importlib.import_module("zig-raytracing-weekend_amd")


def orbit(frames, width, step_deg):
    centre = np.array([278.0, 278.0, 278.0])
    r = np.array(rtw.cornell_camera().lookfrom) - centre
    cams = []
    for k in range(frames):
        a = math.radians(step_deg * k)
        at = centre + np.array([r[0] * math.cos(a) + r[2] * math.sin(a), r[1], -r[0] * math.sin(a) + r[2] * math.cos(a)])
        cam = rtw.cornell_camera(image_width=width, spp=1, max_depth=20)
        cam.lookfrom, cam.lookat = tuple(float(x) for x in at), tuple(float(x) for x in centre)
        cams.append(cam.init())
    return cams


def texels(accum, w, h):
    out = np.zeros((w * h, 4), np.uint8)
    rtw._abi.check(rtw.lib().rtw_texture_from_accum(np.ascontiguousarray(accum).ctypes.data, w * h, out.ctypes.data),
                   "rtw_texture_from_accum")
    return out.reshape(h, w, 4)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("out")
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--width", type=int, default=160)
    ap.add_argument("--frames", type=int, default=6)
    ap.add_argument("--spp", type=int, default=2)
    ap.add_argument("--step", type=float, default=2.0, help="degrees between frames")
    a = ap.parse_args()
    world = rtw.World(rtw.flatten(rtw.worlds.cornell_box()), device=a.device)
    cams = orbit(a.frames, a.width, a.step)
    W = H = a.width
    state = rtw.RayTraceState(camera=cams[0], writer=rtw.SharedStateImageWriter(W, H), world=world, seed=1)
    columns = []
    for k, cam in enumerate(cams):
        if k == 0:
            cam.render_range(state, 0, cam.size, 0, a.spp)
            state.update_moments()
        else:
            state.move_camera(cam, a.spp)
        guides = world.render_guides(cam)
        # the frame's own samples, in two batches so that they carry a variance
        alone = np.zeros((cam.size, 4), np.float32)
        mom = np.zeros((2, cam.size, 4), np.float32)
        for s0, s1 in ((0, max(1, a.spp // 2)), (max(1, a.spp // 2), max(2, a.spp))):
            rtw._abi.check(rtw.lib().rtw_render(world.handle, C.byref(cam.derived), 0, cam.size, s0, s1, 1000 + k,
                                                alone.ctypes.data, None, rtw._abi.PROGRESS_FN(0), None), "rtw_render")
            world.moments_update(alone, mom, W, H)
        rows = [alone, world.denoise_guided(alone, mom, guides, W, H),
                world.denoise_guided(state.writer.buffer, state.moments, guides, W, H)]
        columns.append(np.concatenate([texels(r, W, H) for r in rows], axis=0))
    strip = np.ascontiguousarray(np.concatenate(columns, axis=1))
    rtw.output.write_png(a.out, strip.reshape(-1, 4), strip.shape[1], strip.shape[0])
    world.close()
    print(f"{a.out}: {strip.shape[1]} x {strip.shape[0]}; {a.frames} frames of {a.spp} spp, {a.step} degrees apart; rows: "
          "raw | guided filter | temporal + guided filter")


if __name__ == "__main__":
    main()
