"""next_week at 800x800: the cluster as one tree instance vs eight 125-member list instances, alternated
(profiles/next_week/).  Usage: python tools/next_week_ab.py <out.json> <spp> <repeats>"""
import ctypes as C, importlib, json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
rtw = importlib.import_module("zig-raytracing-weekend_amd")
out_path, spp, reps = sys.argv[1], int(sys.argv[2]), int(sys.argv[3])

def objects(chunks):
    objs = rtw.worlds.next_week_world(0)
    inst = objs.pop()
    balls = inst.object.object.objects
    per = len(balls) // chunks
    for k in range(chunks):
        lst = rtw.HittableList.init()
        for s in balls[k * per:(k + 1) * per]:
            lst.add(s)
        objs.append(rtw.Translate.init(rtw.RotateY.init(lst, 15), [-100, 270, 395]))
    return objs

cam = rtw.next_week_camera(800, spp, 40).init()
worlds = {"tree": rtw.World(rtw.flatten(objects(1))), "lists8": rtw.World(rtw.flatten(objects(8)))}
print({k: (w.stats()["n_nodes"], len(w.instance_nodes(len(w.arrays.instances) - 1))) for k, w in worlds.items()}, flush=True)
res = {k: [] for k in worlds}
imgs = {}
for rep in range(reps + 1):       # rep 0: warm-up
    for k, w in worlds.items():
        acc = torch.zeros((cam.size, 4), dtype=torch.float32, device="cuda")
        tm = rtw._abi.RtwKernelTiming()
        opts = rtw._abi.render_opts(timing=tm)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        rc = rtw.lib().rtw_render_device(w.handle, C.byref(cam.derived), 0, cam.size, 0, spp, 0, acc.data_ptr(), None,
                                         C.byref(opts))
        rtw._abi.check(rc, "rtw_render_device")
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        if rep:
            res[k].append({"seconds": dt, "msamples_per_s": cam.size * spp / dt / 1e6,
                           "kernel_ms": {n: tm.ms[i] for i, n in enumerate(rtw._abi.RTW_K_NAMES)},
                           "launches": {n: tm.launches[i] for i, n in enumerate(rtw._abi.RTW_K_NAMES)}})
            print(k, rep, f"{dt:.3f} s", f"{cam.size * spp / dt / 1e6:.1f} Msamples/s", flush=True)
        imgs[k] = acc.cpu().numpy()
same = bool(np.array_equal(imgs["tree"], imgs["lists8"]))
print("images identical:", same, "finite:", bool(np.isfinite(imgs["tree"]).all()))
json.dump({"config": "next_week 800x800", "spp": spp, "max_depth": 40, "build_id": rtw.lib().rtw_build_id().decode(),
           "images_identical": same, "runs": res}, open(out_path, "w"), indent=1)
for w in worlds.values():
    w.close()
