#!/usr/bin/env python3
"""The grid search behind rtw_temporal_defaults (host backend, no GPU): writes profiles/temporal/defaults.json.

The orbit of tests/test_temporal.py's quality test: Cornell at 64 x 64, 8 cameras each turned by 1 degree about the
box's centre -- and, as further cases, 8 cameras 3 degrees apart and 24 cameras half a degree apart, without which no
cap above 16 samples would ever bite --, 2 spp per frame, the moments updated per frame; the target is the last camera
at --ref-spp.  Every frame and guide is rendered once per seed and shared by the whole grid.  Scored per
combination: RMSE(temporal) / RMSE(the last frame's 2 spp alone) and RMSE(temporal + guided filter) / RMSE(guided
filter alone, its moments from two 1-spp batches), the mean of the two over cases and seeds.  The winner goes into
rtw_temporal_defaults (csrc/rtw_temporal.hip) by hand.

    python tools/temporal_defaults.py [--out profiles/temporal/defaults.json]
"""
import argparse
import ctypes as C
import itertools
import json
import math
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import importlib  # noqa: E402

rtw = importlib.import_module("zig-raytracing-weekend_amd")
CPU = rtw._abi.RTW_DEVICE_CPU
GRID = {
    "max_history": [8.0, 16.0, 32.0, 64.0],
    # 0.2 is as loose as the search may go: an occluder that stands off its background by less than the tolerance is
    # not noticed, and this orbit -- a convex box, almost nothing hidden -- cannot show what that costs (0.4 scores
    # 0.403 here, profiles/temporal/README.md)
    "depth_tolerance": [0.01, 0.05, 0.1, 0.2],
    "normal_cos": [0.5, 0.9, 0.98],
}
SIZE, SPP, SEEDS, REF_SEED = 64, 2, (1, 2, 3), 1000
ORBITS = ((1.0, 8), (3.0, 8), (0.5, 24))     # (degrees per frame, frames): the last one long enough for the cap to bite


def orbit(frames, size, step_deg):
    base = rtw.cornell_camera(image_width=size, spp=1, max_depth=20)
    centre = np.array([278.0, 278.0, 278.0])
    r = np.array(base.lookfrom) - centre
    cams = []
    for k in range(frames):
        a = math.radians(step_deg * k)
        at = centre + np.array([r[0] * math.cos(a) + r[2] * math.sin(a), r[1], -r[0] * math.sin(a) + r[2] * math.cos(a)])
        cams.append(rtw.cornell_camera(image_width=size, spp=1, max_depth=20))
        cams[-1].lookfrom, cams[-1].lookat = tuple(float(x) for x in at), tuple(float(x) for x in centre)
        cams[-1].init()
    return cams


def render(world, cam, s0, s1, seed, buf=None):
    buf = np.zeros((cam.size, 4), np.float32) if buf is None else buf
    rc = rtw.lib().rtw_render(world.handle, C.byref(cam.derived), 0, cam.size, s0, s1, seed, buf.ctypes.data, None,
                              rtw._abi.PROGRESS_FN(0), None)
    rtw._abi.check(rc, "rtw_render")
    return buf


def rmse(acc, ref):
    with np.errstate(all="ignore"):
        a = acc[:, :3].astype(np.float64) / acc[:, 3:4]
        b = ref[:, :3].astype(np.float64) / ref[:, 3:4]
    ok = np.isfinite(a).all(1) & np.isfinite(b).all(1)
    return float(np.sqrt(np.mean((a[ok] - b[ok]) ** 2)))


def run_orbit(world, case, params):
    """The accumulator and the moments after the orbit's last frame."""
    cams, frames, guides = case["cams"], case["frames"], case["guides"]
    acc = frames[0]
    mom = world.moments_update(acc, np.zeros((2, acc.shape[0], 4), np.float32), SIZE, SIZE)
    for k in range(1, len(cams)):
        acc, mom, _ = world.temporal_accumulate(cams[k], cams[k - 1], frames[k], guides[k][1], acc, guides[k - 1][1], mom,
                                                **params)
    return acc, mom


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "temporal", "defaults.json"))
    ap.add_argument("--ref-spp", type=int, default=1024)
    args = ap.parse_args()
    world = rtw.World(rtw.flatten(rtw.worlds.cornell_box()), device=CPU)
    t0 = time.time()
    cases = []
    for step, FRAMES in ORBITS:
        cams = orbit(FRAMES, SIZE, step)
        guides = [world.render_guides(c) for c in cams]
        target = render(world, cams[-1], 0, args.ref_spp, REF_SEED)
        for seed in SEEDS:
            frames = [render(world, c, 0, SPP, 100 * seed + k) for k, c in enumerate(cams)]
            one = render(world, cams[-1], 0, 1, 100 * seed + FRAMES - 1)
            m = world.moments_update(one, np.zeros((2, one.shape[0], 4), np.float32), SIZE, SIZE)
            two = render(world, cams[-1], 1, 2, 100 * seed + FRAMES - 1, one.copy())
            m = world.moments_update(two, m, SIZE, SIZE)
            assert np.array_equal(two, frames[-1])
            alone_guided = world.denoise_guided(two, m, guides[-1], SIZE, SIZE)
            cases.append({"step_deg": step, "n_frames": FRAMES, "seed": seed, "cams": cams, "guides": guides, "frames": frames,
                          "target": target, "rmse_alone": rmse(two, target), "rmse_guided_alone": rmse(alone_guided, target)})
        print(f"step {step}: rendered ({time.time() - t0:.0f} s)", flush=True)

    def score(params):
        raw, filt = [], []
        for c in cases:
            acc, mom = run_orbit(world, c, params)
            raw.append(rmse(acc, c["target"]) / c["rmse_alone"])
            filt.append(rmse(world.denoise_guided(acc, mom, c["guides"][-1], SIZE, SIZE), c["target"]) / c["rmse_guided_alone"])
        return {"score": float(np.mean(raw + filt)), "temporal_over_alone": float(np.mean(raw)),
                "temporal_guided_over_guided": float(np.mean(filt)),
                "per_case": [[c["step_deg"], c["seed"], round(r, 4), round(f, 4)] for c, r, f in zip(cases, raw, filt)]}
    keys = list(GRID)
    rows = []
    for combo in itertools.product(*(GRID[k] for k in keys)):
        p = dict(zip(keys, combo))
        rows.append({**p, **score(p)})
    rows.sort(key=lambda r: r["score"])
    best = rows[0]
    shipped = rtw._abi.temporal_params()
    rep = {
        "what": "grid search for rtw_temporal_defaults on the host backend (tools/temporal_defaults.py)",
        "metric": "mean over cases and seeds of RMSE(temporal) / RMSE(2 spp alone) and RMSE(temporal + guided) / "
                  "RMSE(guided alone), mean radiance against the target; per_case rows are [step, seed, the two ratios]",
        "scene": "cornell", "size": SIZE, "orbits_deg_frames": [list(o) for o in ORBITS], "spp_per_frame": SPP,
        "target_spp": args.ref_spp, "seeds": list(SEEDS), "grid": GRID, "combinations": len(rows),
        "winner": best, "top10": [{k: v for k, v in r.items() if k != "per_case"} for r in rows[:10]],
        "worst": {k: v for k, v in rows[-1].items() if k != "per_case"},
        "by_max_history": {str(v): min(r["score"] for r in rows if r["max_history"] == v) for v in GRID["max_history"]},
        "by_depth_tolerance": {str(v): min(r["score"] for r in rows if r["depth_tolerance"] == v)
                               for v in GRID["depth_tolerance"]},
        "by_normal_cos": {str(v): min(r["score"] for r in rows if r["normal_cos"] == v) for v in GRID["normal_cos"]},
        "shipped": {"max_history": shipped.max_history, "depth_tolerance": shipped.depth_tolerance,
                    "normal_cos": shipped.normal_cos},
    }
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rep, f, indent=1)
        f.write("\n")
    print(json.dumps({k: rep[k] for k in ("winner", "top10", "worst", "by_max_history", "by_depth_tolerance",
                                          "by_normal_cos", "shipped")}, indent=1))


if __name__ == "__main__":
    main()
