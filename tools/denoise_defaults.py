#!/usr/bin/env python3
"""The grid search behind rtw_denoise_defaults (host backend, no GPU): writes profiles/denoise/defaults.json.

Scenes: Cornell, Book-1 and earth + Perlin at 64 x 64.  For each, a 2048-spp host render is the target and 8-spp
renders (three seeds) the input; a parameter set's score is the mean over scenes and seeds of
RMSE(denoised) / RMSE(8 spp), both on the mean radiance against the target.  The grid: passes 3 .. 6, sigma_color,
sigma_normal, sigma_depth as listed below, demodulation on and off.  The winner goes into rtw_denoise_defaults
(csrc/rtw_denoise.hip) by hand; the file also records the quality test's figure (Cornell 48 x 48, tests/test_denoise.py).

    python tools/denoise_defaults.py [--out profiles/denoise/defaults.json]
"""
import argparse
import ctypes as C
import importlib
import itertools
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
rtw = importlib.import_module("zig-raytracing-weekend_amd")
CPU = rtw._abi.RTW_DEVICE_CPU

GRID = {
    "passes": [3, 4, 5, 6],
    "sigma_color": [0.3, 0.6, 1.0, 2.0, 4.0, 8.0, 16.0, 32.0, 64.0],
    "sigma_normal": [0.05, 0.1, 0.25, 0.5, 1.0],
    "sigma_depth": [0.005, 0.01, 0.02, 0.05, 0.1, 0.3],
    "demodulate": [False, True],
}
SPP, REF_SPP, SIZE, SEEDS, REF_SEED = 8, 2048, 64, (1, 2, 3), 1000


def scenes(size):
    W = rtw.worlds

    def cam(c):
        c.image_width, c.image_height, c.aspect_ratio = size, size, 1.0
        return c.init()
    return {
        "cornell": (rtw.flatten(W.cornell_box()), cam(rtw.cornell_camera(spp=SPP))),
        "book1": (rtw.flatten(W.generate_world(0, "book1")), cam(rtw.book1_camera(spp=SPP))),
        "earth_perlin": (rtw.flatten(W.earth_perlin_world(0)), cam(rtw.earth_perlin_camera(spp=SPP))),
    }


def render(world, cam, spp, seed):
    buf = np.zeros((cam.size, 4), np.float32)
    rc = rtw.lib().rtw_render(world.handle, C.byref(cam.derived), 0, cam.size, 0, spp, seed, buf.ctypes.data, None,
                              rtw._abi.PROGRESS_FN(0), None)
    rtw._abi.check(rc, "rtw_render")
    return buf


def rmse(acc, target):
    """RMSE of the mean radiance of an accumulator against the target's."""
    a = acc[:, :3].astype(np.float64) / acc[:, 3:4]
    t = target[:, :3].astype(np.float64) / target[:, 3:4]
    return float(np.sqrt(np.mean((a - t) ** 2)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "denoise", "defaults.json"))
    ap.add_argument("--ref-spp", type=int, default=REF_SPP)
    args = ap.parse_args()
    cases = []
    t0 = time.time()
    for name, (arr, cam) in scenes(SIZE).items():
        world = rtw.World(arr, device=CPU)
        target = render(world, cam, args.ref_spp, REF_SEED)
        guides = world.render_guides(cam)
        for seed in SEEDS:
            noisy = render(world, cam, SPP, seed)
            cases.append((name, world, cam, guides, noisy, target, rmse(noisy, target)))
        print(f"{name}: rendered ({time.time() - t0:.0f} s), 8-spp RMSE {cases[-1][-1]:.4f}", flush=True)
    keys = list(GRID)
    rows = []
    for combo in itertools.product(*(GRID[k] for k in keys)):
        p = dict(zip(keys, combo))
        ratios = {}
        for name, world, cam, guides, noisy, target, base in cases:
            out = world.denoise(noisy, guides, SIZE, SIZE, **p)
            ratios.setdefault(name, []).append(rmse(out, target) / base)
        per_scene = {k: float(np.mean(v)) for k, v in ratios.items()}
        rows.append({**p, "score": float(np.mean(list(per_scene.values()))), **per_scene})
    rows.sort(key=lambda r: r["score"])
    best = rows[0]
    # the quality test's case: Cornell 48 x 48, seed 7, the winner's parameters
    arr = rtw.flatten(rtw.worlds.cornell_box())
    cam = rtw.cornell_camera(image_width=48, spp=SPP).init()
    world = rtw.World(arr, device=CPU)
    target = render(world, cam, args.ref_spp, REF_SEED)
    noisy = render(world, cam, SPP, 7)
    out = world.denoise(noisy, world.render_guides(cam), 48, 48, **{k: best[k] for k in keys})
    quality = {"scene": "cornell 48 x 48, 8 spp, seed 7, against 2048 spp (seed 1000)", "rmse_8spp": rmse(noisy, target),
               "rmse_denoised": rmse(out, target)}
    quality["ratio"] = quality["rmse_denoised"] / quality["rmse_8spp"]
    rep = {
        "what": "grid search for rtw_denoise_defaults on the host backend (tools/denoise_defaults.py)",
        "metric": "mean over scenes and seeds of RMSE(denoised) / RMSE(8 spp), mean radiance against the target",
        "scenes": list(scenes(8)), "size": SIZE, "spp": SPP, "target_spp": args.ref_spp, "seeds": list(SEEDS),
        "grid": GRID, "combinations": len(rows), "winner": best, "top10": rows[:10],
        "worst": rows[-1], "quality_test": quality,
        "by_sigma_color": {str(sc): min(r["score"] for r in rows if r["sigma_color"] == sc) for sc in GRID["sigma_color"]},
        "by_passes": {str(n): min(r["score"] for r in rows if r["passes"] == n) for n in GRID["passes"]},
        "by_demodulate": {str(d): min(r["score"] for r in rows if r["demodulate"] == d) for d in GRID["demodulate"]},
    }
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rep, f, indent=1)
        f.write("\n")
    print(json.dumps({"winner": best, "quality_test": quality}, indent=1))


if __name__ == "__main__":
    main()
