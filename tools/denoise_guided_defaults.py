#!/usr/bin/env python3
"""The grid search behind rtw_denoise_guided_defaults (host backend, no GPU): writes
profiles/denoise_guided/defaults.json.

The setting of tools/denoise_defaults.py -- its scenes, size, seeds, target and metric -- with each 8-spp input
rendered as eight 1-spp batches and the moments updated after each (rtw_moments_update).  The grid: passes, sigma_color
(sl, in standard deviations), sigma_normal, sigma_depth, demodulation on and off.  The plain filter's shipped defaults
(rtw_denoise_defaults) are scored on the same inputs in the same run, and the inputs of two 4-batch splits (2-spp
batches) are scored with the winner.  The winner goes into rtw_denoise_guided_defaults (csrc/rtw_denoise.hip) by hand.

    python tools/denoise_guided_defaults.py [--out profiles/denoise_guided/defaults.json]
"""
import argparse
import ctypes as C
import itertools
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import denoise_defaults as P  # noqa: E402  (the plain search: scenes, render, rmse, the sizes and seeds)

rtw, CPU, REPO = P.rtw, P.CPU, P.REPO
GRID = {
    "passes": [3, 4, 5, 6],
    "sigma_color": [1.0, 2.0, 4.0, 8.0, 16.0],
    "sigma_normal": [0.1, 0.25, 0.5],
    "sigma_depth": [0.005, 0.02, 0.1],
    "demodulate": [False, True],
}
SPP, SIZE, SEEDS, REF_SEED = P.SPP, P.SIZE, P.SEEDS, P.REF_SEED


def render_with_moments(world, cam, spp, seed, batch=1):
    """(accumulator, moments) of `spp` samples rendered in batches of `batch`, the moments updated after each."""
    buf = np.zeros((cam.size, 4), np.float32)
    mom = np.zeros((2, cam.size, 4), np.float32)
    w, h = cam.derived.image_width, cam.derived.image_height
    for s in range(0, spp, batch):
        rc = rtw.lib().rtw_render(world.handle, C.byref(cam.derived), 0, cam.size, s, min(spp, s + batch), seed,
                                  buf.ctypes.data, None, rtw._abi.PROGRESS_FN(0), None)
        rtw._abi.check(rc, "rtw_render")
        world.moments_update(buf, mom, w, h)
    return buf, mom


def score(rows_of_ratios):
    per_scene = {k: float(np.mean(v)) for k, v in rows_of_ratios.items()}
    return float(np.mean(list(per_scene.values()))), per_scene


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "denoise_guided", "defaults.json"))
    ap.add_argument("--ref-spp", type=int, default=P.REF_SPP)
    args = ap.parse_args()
    cases = []
    t0 = time.time()
    for name, (arr, cam) in P.scenes(SIZE).items():
        world = rtw.World(arr, device=CPU)
        target = P.render(world, cam, args.ref_spp, REF_SEED)
        guides = world.render_guides(cam)
        for seed in SEEDS:
            noisy, mom = render_with_moments(world, cam, SPP, seed)
            assert np.array_equal(noisy, P.render(world, cam, SPP, seed))   # the plain search's inputs, to the bit
            _, mom2 = render_with_moments(world, cam, SPP, seed, batch=2)
            cases.append((name, world, guides, noisy, mom, mom2, target, P.rmse(noisy, target)))
        print(f"{name}: rendered ({time.time() - t0:.0f} s), 8-spp RMSE {cases[-1][-1]:.4f}", flush=True)

    def run(filt):
        ratios, per_seed = {}, {}
        for name, world, guides, noisy, mom, mom2, target, base in cases:
            r = P.rmse(filt(world, guides, noisy, mom, mom2), target) / base
            ratios.setdefault(name, []).append(r)
            per_seed.setdefault(name, []).append(round(r, 4))
        s, per_scene = score(ratios)
        return s, per_scene, per_seed
    plain_score, plain_scene, plain_seed = run(lambda w, g, a, m, m2: w.denoise(a, g, SIZE, SIZE))
    keys = list(GRID)
    rows = []
    for combo in itertools.product(*(GRID[k] for k in keys)):
        p = dict(zip(keys, combo))
        s, per_scene, _ = run(lambda w, g, a, m, m2: w.denoise_guided(a, m, g, SIZE, SIZE, **p))
        rows.append({**p, "score": s, **per_scene})
    rows.sort(key=lambda r: r["score"])
    best = rows[0]
    # below the grid (the plain search starts at 3 passes too): the winner's sigmas with 2 passes, for the record
    two_passes = dict(best, passes=2)
    two_passes["score"], per_scene, _ = run(
        lambda w, g, a, m, m2: w.denoise_guided(a, m, g, SIZE, SIZE, **{k: two_passes[k] for k in keys}))
    two_passes.update(per_scene)
    bp = {k: best[k] for k in keys}
    _, _, best_seed = run(lambda w, g, a, m, m2: w.denoise_guided(a, m, g, SIZE, SIZE, **bp))
    two_score, two_scene, _ = run(lambda w, g, a, m, m2: w.denoise_guided(a, m2, g, SIZE, SIZE, **bp))
    # the quality test's case: Cornell 48 x 48, seed 7, the winner's parameters and the plain defaults
    arr = rtw.flatten(rtw.worlds.cornell_box())
    cam = rtw.cornell_camera(image_width=48, spp=SPP).init()
    world = rtw.World(arr, device=CPU)
    target = P.render(world, cam, args.ref_spp, REF_SEED)
    noisy, mom = render_with_moments(world, cam, SPP, 7)
    guides = world.render_guides(cam)
    quality = {"scene": "cornell 48 x 48, 8 spp in 1-spp batches, seed 7, against 2048 spp (seed 1000)",
               "rmse_8spp": P.rmse(noisy, target),
               "rmse_guided": P.rmse(world.denoise_guided(noisy, mom, guides, 48, 48, **bp), target),
               "rmse_plain_defaults": P.rmse(world.denoise(noisy, guides, 48, 48), target)}
    quality["ratio_guided"] = quality["rmse_guided"] / quality["rmse_8spp"]
    quality["ratio_plain"] = quality["rmse_plain_defaults"] / quality["rmse_8spp"]
    rep = {
        "what": "grid search for rtw_denoise_guided_defaults on the host backend (tools/denoise_guided_defaults.py)",
        "metric": "mean over scenes and seeds of RMSE(denoised) / RMSE(8 spp), mean radiance against the target",
        "scenes": list(P.scenes(8)), "size": SIZE, "spp": SPP, "moments": "eight 1-spp batches",
        "target_spp": args.ref_spp, "seeds": list(SEEDS), "grid": GRID, "combinations": len(rows),
        "plain_defaults": {"score": plain_score, **plain_scene, "per_seed": plain_seed},
        "winner": best, "winner_per_seed": best_seed,
        "winner_beats_plain": bool(best["score"] < plain_score),
        "winner_with_2spp_batches": {"score": two_score, **two_scene},
        "winner_sigmas_with_2_passes": two_passes, "top10": rows[:10], "worst": rows[-1], "quality_test": quality,
        "by_sigma_color": {str(v): min(r["score"] for r in rows if r["sigma_color"] == v) for v in GRID["sigma_color"]},
        "by_passes": {str(v): min(r["score"] for r in rows if r["passes"] == v) for v in GRID["passes"]},
        "by_demodulate": {str(v): min(r["score"] for r in rows if r["demodulate"] == v) for v in GRID["demodulate"]},
        "best_demodulated": next(r for r in rows if r["demodulate"]),
    }
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rep, f, indent=1)
        f.write("\n")
    print(json.dumps({"plain_defaults": rep["plain_defaults"], "winner": best, "two_spp": rep["winner_with_2spp_batches"],
                      "two_passes": two_passes,
                      "best_demodulated": rep["best_demodulated"], "quality_test": quality}, indent=1))


if __name__ == "__main__":
    main()
