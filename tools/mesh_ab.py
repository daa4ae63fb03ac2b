"""Triangle-mesh measurements on the GPU (DESIGN.md §Triangles and meshes; JSON under profiles/meshes/).

    python tools/mesh_ab.py quads out.json [repeats]   Cornell and Cornell smoke at bench geometry (600 x 600 x 200 spp,
                                                       depth 50), lights off and on: what the shape test costs the
                                                       quad path.  Uses no triangle, so RTW_LIB may name the parent
                                                       commit's library: alternate the two in one session.
    python tools/mesh_ab.py mesh out.json [repeats]    worlds.cornell_mesh(level 5) -- a 20 480-triangle icosphere as a
                                                       tree instance -- against the same scene with the analytic
                                                       Sphere in its place, lights off and on, with per-kernel times.
    python tools/mesh_ab.py smooth out.json [repeats]  the price of per-vertex normals (DESIGN.md §Smooth shading and mesh
                                                       UVs): worlds.cornell_mesh(5, smooth=True) -- the attribute
                                                       kernels -- against cornell_mesh(5), lights off and on.
    python tools/mesh_ab.py leaks out.json [--host-only]  the camera inside a closed emissive level-2 icosphere, depth 1,
                                                       64 x 64 x 64 spp: samples that escape (device 0 and the host).

Timing: one warm-up, then HIP-event timed repeats (default 5), median -- the way bench.py times a step; a further
pass per arm takes the per-kernel times (rtw_kernel_timing) outside the timed region."""
import ctypes as C, importlib, json, os, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
rtw = importlib.import_module("zig-raytracing-weekend_amd")
MODE, out_path = sys.argv[1], sys.argv[2]
reps = int(sys.argv[3]) if len(sys.argv) > 3 and sys.argv[3].isdigit() else 5
W, SPP, DEPTH, SEED = 600, 200, 50, 0


def render_timed(world, cam, spp, timing=None):
    import torch
    acc = torch.zeros((cam.size, 4), dtype=torch.float32, device="cuda")
    opts = rtw._abi.render_opts(timing=timing) if timing is not None else None
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    rc = rtw.lib().rtw_render_device(world.handle, C.byref(cam.derived), 0, cam.size, 0, spp, SEED, acc.data_ptr(), None,
                                     C.byref(opts) if opts is not None else None)
    rtw._abi.check(rc, "rtw_render_device")
    b.record()
    torch.cuda.synchronize()
    return acc, a.elapsed_time(b)


def time_arms(arms, cam):
    """arms: name -> World.  -> name -> {ms, median_ms, msamples_per_s, kernel_ms, finite, mean}"""
    import torch
    ms = {k: [] for k in arms}
    img = {}
    for rep in range(reps + 1):      # rep 0: warm-up
        for k, w in arms.items():
            img[k], t = render_timed(w, cam, SPP)
            if rep:
                ms[k].append(t)
    rec = {}
    for k, w in arms.items():
        tm = rtw._abi.RtwKernelTiming()
        render_timed(w, cam, SPP, timing=tm)
        med = statistics.median(ms[k])
        rec[k] = {"ms": ms[k], "median_ms": med, "msamples_per_s": cam.size * SPP / med / 1e3,
                  "finite": bool(torch.isfinite(img[k]).all()), "mean_rgb": (img[k][:, :3].mean(0) / SPP).tolist(),
                  "lights": w.lights().tolist(), "stats": w.stats(),
                  "vertex_attrs": 0 if w.arrays.vertex_attrs is None else int(len(w.arrays.vertex_attrs[0])),
                  "kernel_ms": {n: tm.ms[i] for i, n in enumerate(rtw._abi.RTW_K_NAMES) if tm.launches[i]}}
        w.close()
    return rec


def leaks(device):
    """Samples that see the background from inside a closed emissive icosphere (radiance 1, black background)."""
    glow = rtw.DiffuseLight.fromColor([1, 1, 1])
    ico = rtw.worlds.icosphere(2, [0, 0, 0], 10, glow)
    cam = rtw.Camera(image_width=64, aspect_ratio=1.0, samples_per_pixel=64, max_depth=1, vfov=140.0,
                     lookfrom=(0.3, 0.2, 0.1), lookat=(1.0, 0.5, -2.0), vup=(0, 1, 0), defocus_angle=0.0,
                     background=(0.0, 0.0, 0.0)).init()
    out = {}
    for what, objs in (("instance", [ico]), ("top_level", ico.objects)):
        world = rtw.World(rtw.flatten(objs), device=device)
        buf = np.zeros((cam.size, 4), np.float32)
        rc = rtw.lib().rtw_render(world.handle, C.byref(cam.derived), 0, cam.size, 0, 64, SEED, buf.ctypes.data, None,
                                  rtw._abi.PROGRESS_FN(0), None)
        rtw._abi.check(rc, "rtw_render")
        world.close()
        assert np.array_equal(buf[:, 0], np.round(buf[:, 0])) and buf[:, 0].max() <= 64
        out[what] = {"samples": int(cam.size * 64), "escaped": int(cam.size * 64 - buf[:, 0].astype(np.int64).sum())}
    return out


result = {"mode": MODE, "build_id": rtw.lib().rtw_build_id().decode(), "lib": os.environ.get("RTW_LIB", "in-tree")}
if MODE == "leaks":
    result["what"] = "camera inside a closed emissive level-2 icosphere (320 triangles), depth 1, 64 x 64 x 64 spp"
    result["host"] = leaks(rtw._abi.RTW_DEVICE_CPU)
    if "--host-only" not in sys.argv:
        result["gpu"] = leaks(0)
else:
    import torch
    result.update(config=f"{W}x{W} x {SPP} spp, depth {DEPTH}", repeats=reps, device=torch.cuda.get_device_name(0),
                  scenes={})
    cam = rtw.cornell_camera(W, SPP, DEPTH).init()
    if MODE == "quads":
        scenes = {"cornell": rtw.worlds.cornell_box(), "cornell_smoke": rtw.worlds.cornell_smoke()}
    elif MODE == "smooth":
        scenes = {"mesh_level5_smooth": rtw.worlds.cornell_mesh(5, smooth=True), "mesh_level5_flat": rtw.worlds.cornell_mesh(5)}
    else:
        scenes = {"mesh_level5": rtw.worlds.cornell_mesh(5), "analytic_sphere": rtw.worlds.cornell_mesh(5, analytic=True)}
    for name, objs in scenes.items():
        arms = {k: rtw.World(rtw.flatten(objs, lights=v)) for k, v in (("off", None), ("on", "emissive"))}
        result["scenes"][name] = time_arms(arms, cam)
        print(name, {k: (round(v["median_ms"], 3), v["kernel_ms"]) for k, v in result["scenes"][name].items()}, flush=True)
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
json.dump(result, open(out_path, "w"), indent=1)
print("wrote", out_path, json.dumps({k: v for k, v in result.items() if k in ("host", "gpu")}))
