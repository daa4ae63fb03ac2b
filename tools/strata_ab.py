"""Stratified pixel samples (rtw_camera.strata) A/B: what they cost and what they buy.

  python tools/strata_ab.py cost  [out.json] [repeats]      one library (RTW_LIB names another build, e.g. the parent's:
        tools/build_at.sh <commit> parent): C2, C5 and Cornell at bench geometry and spp, strata off and -- where the
        library has rtw_camera_set_strata -- strata = floor(sqrt(spp)), the arms alternated: warm-up, then HIP-event
        timed repeats of rtw_render_device (the way bench.py times a step), median, min, max, Msamples/s and on / off.
  python tools/strata_ab.py merge <out.json> <parent.json>... -- <this.json>...
        the strata-off arms of alternated `cost` runs of two libraries on one box: per scene both sides' medians and
        this build's median against the parent's own min-max spread.
  python tools/strata_ab.py gain  [out.json] [gpu | host] [ref_spp] [seeds]
        Cornell and Book-1 (its checker ground) at 64 spp, strata 8 against off: MSE against a ref_spp (4096) render
        of the same build with strata off and another seed, mean over the seeds (8); the reference's own noise
        MSE_off * 64 / ref_spp is taken out of both.  gpu: bench geometry; host: the host backend at a reduced size.

Every file is stamped with rtw_build_id.  Default outputs: profiles/strata/{cost,off_vs_parent,gain_<where>}.json"""
import ctypes as C, importlib, json, math, os, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "profiles", "strata")
MODE = sys.argv[1] if len(sys.argv) > 1 else "cost"


def write(path, result):
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    json.dump(result, open(path, "w"), indent=1)
    print("wrote", path)


if MODE == "merge":
    sep = sys.argv.index("--")
    sides = {"parent": [json.load(open(p)) for p in sys.argv[3:sep]],
             "this": [json.load(open(p)) for p in sys.argv[sep + 1:]]}
    result = {"what": "strata off: the parent commit's library against this build, processes alternated on one box",
              "device": sides["this"][0]["device"], "scenes": {},
              **{f"{k}_build_id": sorted({r["build_id"] for r in v}) for k, v in sides.items()}}
    for name in sides["this"][0]["scenes"]:
        ms = {k: [t for r in v for t in r["scenes"][name]["off"]["ms"]] for k, v in sides.items()}
        med = {k: statistics.median(v) for k, v in ms.items()}
        lo, hi = min(ms["parent"]), max(ms["parent"])
        result["scenes"][name] = {"parent_ms": ms["parent"], "this_ms": ms["this"], "parent_median_ms": med["parent"],
                                  "this_median_ms": med["this"], "this_over_parent": med["this"] / med["parent"],
                                  "parent_spread_ms": [lo, hi], "parent_spread_rel": (hi - lo) / med["parent"],
                                  "this_median_inside_parent_spread": lo <= med["this"] <= hi}
        print(name, json.dumps({k: v for k, v in result["scenes"][name].items() if not k.endswith("_ms")}))
    write(sys.argv[2], result)
    sys.exit(0)

import numpy as np
rtw = importlib.import_module("zig-raytracing-weekend_amd")
HAS = hasattr(rtw.lib(), "rtw_camera_set_strata")
build_id = rtw.lib().rtw_build_id().decode()


def camera(cfg, strata, **over):
    cam = rtw.configs.CONFIGS[cfg].camera()
    for k, v in over.items():
        setattr(cam, k, v)
    cam.strata = strata
    return cam.init()


if MODE == "cost":
    import torch
    out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(OUT, "cost.json")
    reps = int(sys.argv[3]) if len(sys.argv) > 3 else 5

    def render(world, cam):
        acc = torch.zeros((cam.size, 4), dtype=torch.float32, device="cuda")
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        rc = rtw.lib().rtw_render_device(world.handle, C.byref(cam.derived), 0, cam.size, 0, cam.samples_per_pixel, 0,
                                         acc.data_ptr(), None, None)
        rtw._abi.check(rc, "rtw_render_device")
        b.record()
        torch.cuda.synchronize()
        assert bool(torch.isfinite(acc).all())
        return a.elapsed_time(b)

    result = {"lib": os.environ.get("RTW_LIB", "in-tree"), "build_id": build_id, "repeats": reps,
              "device": torch.cuda.get_device_name(0), "scenes": {}}
    for cfg in ("c2", "c5", "cornell"):
        spp = rtw.configs.CONFIGS[cfg].camera().samples_per_pixel
        arms = {"off": camera(cfg, 0)}
        if HAS:
            arms["on"] = camera(cfg, math.isqrt(spp))
        world = rtw.World(rtw.flatten(rtw.configs.CONFIGS[cfg].objects()))
        ms = {k: [] for k in arms}
        for rep in range(reps + 1):          # rep 0: warm-up
            for k, cam in arms.items():
                t = render(world, cam)
                if rep:
                    ms[k].append(t)
        world.close()
        n = arms["off"].size * spp
        rec = {k: {"strata": int(arms[k].derived.strata) if HAS else 0, "ms": v, "median_ms": statistics.median(v),
                   "min_ms": min(v), "max_ms": max(v), "msamples_per_s": n / statistics.median(v) / 1e3}
               for k, v in ms.items()}
        if HAS:
            rec["msamples_on_over_off"] = rec["on"]["msamples_per_s"] / rec["off"]["msamples_per_s"]
        result["scenes"][cfg] = rec
        print(cfg, json.dumps({k: (round(v["median_ms"], 2), round(v["msamples_per_s"], 1)) if isinstance(v, dict) else
                               round(v, 4) for k, v in rec.items()}), flush=True)
    write(out_path, result)
elif MODE == "gain":
    where = sys.argv[3] if len(sys.argv) > 3 else "gpu"
    out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(OUT, f"gain_{where}.json")
    REF_SPP = int(sys.argv[4]) if len(sys.argv) > 4 else 4096
    seeds = list(range(int(sys.argv[5]) if len(sys.argv) > 5 else 8))
    SPP, STRATA, REF_SEED = 64, 8, 977
    device = 0 if where == "gpu" else rtw._abi.RTW_DEVICE_CPU
    small = {} if where == "gpu" else {"image_width": 150}

    def render(world, cam, spp, seed):
        buf = np.zeros((cam.size, 4), np.float32)
        rc = rtw.lib().rtw_render(world.handle, C.byref(cam.derived), 0, cam.size, 0, spp, seed, buf.ctypes.data, None,
                                  rtw._abi.PROGRESS_FN(0), None)
        rtw._abi.check(rc, "rtw_render")
        return buf[:, :3].astype(np.float64) / spp

    result = {"where": where, "build_id": build_id, "spp": SPP, "strata": STRATA, "ref_spp": REF_SPP,
              "seeds": len(seeds), "scenes": {}}
    for cfg in ("cornell", "c2"):
        off, on = camera(cfg, 0, samples_per_pixel=SPP, **small), camera(cfg, STRATA, samples_per_pixel=SPP, **small)
        world = rtw.World(rtw.flatten(rtw.configs.CONFIGS[cfg].objects()), device=device)
        ref = render(world, off, REF_SPP, REF_SEED)
        mse = {k: [float(((render(world, cam, SPP, s) - ref) ** 2).mean()) for s in seeds]
               for k, cam in (("off", off), ("on", on))}
        world.close()
        m = {k: statistics.mean(v) for k, v in mse.items()}
        ref_mse = m["off"] * SPP / (REF_SPP + SPP)   # MSE_off = own + ref's, ref's = own * SPP / REF_SPP
        result["scenes"][cfg] = {"size": [off.derived.image_width, off.derived.image_height], "mse_off": mse["off"],
                                 "mse_on": mse["on"], "mse_ratio_on_off_raw": m["on"] / m["off"],
                                 "mse_ratio_on_off": (m["on"] - ref_mse) / (m["off"] - ref_mse)}
        print(cfg, json.dumps({k: v for k, v in result["scenes"][cfg].items() if not k.startswith("mse_o")}), flush=True)
    write(out_path, result)
else:
    sys.exit(__doc__)
