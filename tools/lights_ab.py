"""Light importance sampling A/B on the GPU: Cornell and Cornell smoke at 600 x 600 x 200 spp, depth 50, with and
without the light registered (rtw_scene_set_lights), alternated -- or, with `simple_light` as the fourth argument,
simple_light at 800 x 450 x 100 spp, depth 50, with nothing, the quad alone ("quad") and the quad and the sphere
("quad_sphere") registered.  Per scene and arm: Msamples/s (warm-up, then
HIP-event timed repeats, median -- the way bench.py times a step; a second timed pass per arm takes the per-kernel
times, rtw_kernel_timing, outside the timed region), the image's RMSE against a lights-off render of REF_SPP
samples per pixel of the same scene (another seed), and the spp a lights-off render needs for the lights-on RMSE
(from the 1 / sqrt(N) law; the reference's own noise, RMSE_off^2 * spp / REF_SPP, is taken out of both first).
Every lit arm is compared with "off" (<arm>_vs_off: mse_ratio, base_spp_for_rmse, time_ratio_equal_rmse);
simple_light also compares "quad_sphere" with "quad" the same way.
Usage: python tools/lights_ab.py [out.json] [repeats] [ref_spp] [cornell | simple_light]
       (default profiles/lights/cornell_ab.json 5 4096 cornell; simple_light: profiles/lights/simple_light_ab.json)"""
import ctypes as C, importlib, json, os, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np, torch
rtw = importlib.import_module("zig-raytracing-weekend_amd")
WHICH = sys.argv[4] if len(sys.argv) > 4 else "cornell"
out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "lights", f"{WHICH}_ab.json")
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
REF_SPP = int(sys.argv[3]) if len(sys.argv) > 3 else 4096
SEED, REF_SEED, DEPTH = 0, 977, 50
if WHICH == "simple_light":
    W, H, SPP = 800, 450, 100
    SCENES = (("simple_light", rtw.worlds.simple_light_world(), rtw.simple_light_camera(W, SPP),
               {"off": None, "quad": "emissive", "quad_sphere": "emissive+spheres"}),)
else:
    W, H, SPP = 600, 600, 200
    SCENES = tuple((name, objs, rtw.cornell_camera(W, SPP, DEPTH), {"off": None, "on": "emissive"})
                   for name, objs in (("cornell", rtw.worlds.cornell_box()), ("cornell_smoke", rtw.worlds.cornell_smoke())))


def render(world, cam, spp, seed, timing=None):
    acc = torch.zeros((cam.size, 4), dtype=torch.float32, device="cuda")
    opts = rtw._abi.render_opts(timing=timing) if timing is not None else None
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    rc = rtw.lib().rtw_render_device(world.handle, C.byref(cam.derived), 0, cam.size, 0, spp, seed, acc.data_ptr(), None,
                                     C.byref(opts) if opts is not None else None)
    rtw._abi.check(rc, "rtw_render_device")
    b.record()
    torch.cuda.synchronize()
    return acc, a.elapsed_time(b)


result = {"config": f"{W}x{H} x {SPP} spp, depth {DEPTH}", "ref_spp": REF_SPP, "repeats": reps,
          "build_id": rtw.lib().rtw_build_id().decode(), "device": torch.cuda.get_device_name(0), "scenes": {}}
for name, objs, cam, lit in SCENES:
    cam = cam.init()
    assert cam.derived.max_depth == DEPTH and cam.derived.image_height == H
    arms = {k: rtw.World(rtw.flatten(objs, lights=v)) for k, v in lit.items()}
    ref, _ = render(arms["off"], cam, REF_SPP, REF_SEED)
    ref = (ref[:, :3] / REF_SPP).double()
    ms = {k: [] for k in arms}
    img = {}
    for rep in range(reps + 1):      # rep 0: warm-up
        for k, w in arms.items():
            acc, t = render(w, cam, SPP, SEED)
            if rep:
                ms[k].append(t)
            img[k] = acc
    rec = {}
    for k, w in arms.items():
        tm = rtw._abi.RtwKernelTiming()
        render(w, cam, SPP, SEED, timing=tm)
        med = statistics.median(ms[k])
        mse = float((((img[k][:, :3] / SPP).double() - ref) ** 2).mean())
        rec[k] = {"ms": ms[k], "median_ms": med, "msamples_per_s": cam.size * SPP / med / 1e3, "rmse": mse ** 0.5,
                  "finite": bool(torch.isfinite(img[k]).all()), "lights": w.lights().tolist(),
                  "kernel_ms": {n: tm.ms[i] for i, n in enumerate(rtw._abi.RTW_K_NAMES) if tm.launches[i]}}
        w.close()
    # the reference carries the lights-off estimator's noise at REF_SPP: take it out of every MSE
    ref_mse = rec["off"]["rmse"] ** 2 * SPP / (REF_SPP + SPP)
    own = {k: max(rec[k]["rmse"] ** 2 - ref_mse, 1e-30) for k in arms}
    pairs = [(k, "off") for k in arms if k != "off"] + ([("quad_sphere", "quad")] if "quad_sphere" in arms else [])
    for k, base in pairs:
        tag = f"{k}_vs_{base}"
        rec[tag] = {"mse_ratio": own[k] / own[base], "base_spp_for_rmse": SPP * own[base] / own[k]}
        # wall time of a `base` render reaching arm k's RMSE / arm k's render's
        rec[tag]["time_ratio_equal_rmse"] = (rec[tag]["base_spp_for_rmse"] / SPP) * rec[base]["median_ms"] / rec[k]["median_ms"]
    if "on" in arms:   # the Cornell table's field names (profiles/lights/cornell_ab.json)
        rec["mse_ratio_on_off"] = rec["on_vs_off"]["mse_ratio"]
        rec["off_spp_for_on_rmse"] = rec["on_vs_off"]["base_spp_for_rmse"]
        rec["time_ratio_equal_rmse_off_over_on"] = rec["on_vs_off"]["time_ratio_equal_rmse"]
    result["scenes"][name] = rec
    print(name, json.dumps({k: v for k, v in rec.items() if k not in arms}),
          {k: (round(rec[k]["median_ms"], 2), round(rec[k]["msamples_per_s"], 1), round(rec[k]["rmse"], 5)) for k in arms},
          flush=True)
os.makedirs(os.path.dirname(out_path), exist_ok=True)
json.dump(result, open(out_path, "w"), indent=1)
print("wrote", out_path)
