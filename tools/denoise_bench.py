#!/usr/bin/env python3
"""What the denoiser costs on the GPU (needs an MI355X; there is no fallback): for 1200 x 800 and 3840 x 2160 frames

  * the time of one rtw_denoise_device call (HIP events on the caller's stream, after warm-up), with the shipped
    defaults and with 5 demodulated passes;
  * the time of one 1-spp rtw_render_device batch of Book-1 at the same frame in the same run -- the filter's cost
    is stated as a number of samples per pixel -- and of one rtw_render_guides_device call;
  * the per-pass kernel times from a separate `rocprofv3 --kernel-trace --stats` run of this script (--trace-child),
    as 48 B x pixels over the time -- the two 16-B planes a pass must read and the one it must write -- against the
    6.29 TB/s copy rate measured on this part.  A share of that copy rate, not of a bound: the planes of a frame
    are cache-resident and the 25 taps re-read them through L1 / L2.

    python tools/denoise_bench.py --out profiles/denoise        # writes README.md and denoise_bench.json there
    RTW_LIB=build/rtw_x.so python tools/denoise_bench.py --ab-child   # one A/B sample: a JSON line, no trace
"""
import argparse
import ctypes as C
import csv
import glob
import importlib
import json
import os
import signal
import statistics
import subprocess
import sys
import tempfile

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
FRAMES = [(1200, 800), (3840, 2160)]
COPY_TBS = 6.29           # the measured HBM copy rate of the part, TB/s
PASS_BYTES = 48           # per pixel: two 16-B planes read, one written
CONFIGS = {"defaults": {}, "5 passes, demodulated": dict(passes=5, demodulate=True)}


def setup(rtw, W, H, spp=4):
    """Book-1 on device 0 at W x H: (world, camera, accumulator after `spp` samples, albedo, normal_depth)."""
    import torch
    world = rtw.World(rtw.flatten(rtw.worlds.generate_world(0, "book1")), device=0)
    cam = rtw.book1_camera(image_width=W, aspect_ratio=W / H, image_height=H, spp=spp).init()
    acc = torch.zeros((cam.size, 4), dtype=torch.float32, device="cuda")
    alb, nd = torch.empty_like(acc), torch.empty_like(acc)
    L = rtw.lib()
    rtw._abi.check(L.rtw_render_device(world.handle, C.byref(cam.derived), 0, cam.size, 0, spp, 0, acc.data_ptr(), None,
                                       None), "rtw_render_device")
    rtw._abi.check(L.rtw_render_guides_device(world.handle, C.byref(cam.derived), alb.data_ptr(), nd.data_ptr(), None, 0),
                   "rtw_render_guides_device")
    return world, cam, acc, alb, nd


def timed(fn, stream, warmup, reps):
    """Milliseconds of each of `reps` calls of fn() (which enqueues on `stream`), by HIP events."""
    import torch
    out = []
    with torch.cuda.stream(stream):
        for k in range(warmup + reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            if k >= warmup:
                out.append(a.elapsed_time(b))
    return out


def summary(ms):
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "n": len(ms)}


def denoise_call(rtw, world, W, H, acc, alb, nd, out, stream, params):
    L = rtw.lib()
    sp = C.c_void_p(stream.cuda_stream)

    def fn():
        rtw._abi.check(L.rtw_denoise_device(world.handle, W, H, acc.data_ptr(), alb.data_ptr(), nd.data_ptr(),
                                            C.byref(params), out.data_ptr(), sp, rtw._abi.RTW_RENDER_NO_SYNC),
                       "rtw_denoise_device")
    return fn


def measure(rtw, W, H, warmup, reps):
    import torch
    world, cam, acc, alb, nd = setup(rtw, W, H)
    out = torch.empty_like(acc)
    stream = torch.cuda.Stream()
    L = rtw.lib()
    sp = C.c_void_p(stream.cuda_stream)
    opts = rtw._abi.render_opts(flags=rtw._abi.RTW_RENDER_NO_SYNC)
    s = [4]

    def render_1spp():
        rtw._abi.check(L.rtw_render_device(world.handle, C.byref(cam.derived), 0, cam.size, s[0], s[0] + 1, 0,
                                           acc.data_ptr(), sp, C.byref(opts)), "rtw_render_device")
        s[0] += 1

    def guides():
        rtw._abi.check(L.rtw_render_guides_device(world.handle, C.byref(cam.derived), alb.data_ptr(), nd.data_ptr(), sp,
                                                  rtw._abi.RTW_RENDER_NO_SYNC), "rtw_render_guides_device")
    torch.cuda.synchronize()
    res = {"frame": [W, H], "render_1spp": summary(timed(render_1spp, stream, warmup, reps)),
           "guides": summary(timed(guides, stream, warmup, reps)), "denoise": {}}
    for name, kw in CONFIGS.items():
        p = rtw._abi.denoise_params(**kw)
        r = summary(timed(denoise_call(rtw, world, W, H, acc, alb, nd, out, stream, p), stream, warmup, reps))
        r["passes"] = p.passes
        r["cost_spp"] = r["median_ms"] / res["render_1spp"]["median_ms"]
        res["denoise"][name] = r
    torch.cuda.synchronize()
    world.close()
    return res


def trace_child(rtw, reps):
    """Under rocprofv3: `reps` denoise calls per frame and configuration (the first half of them is the
    configuration's warm-up, per_pass reads the second half), nothing else worth tracing after setup."""
    import torch
    for W, H in FRAMES:
        world, cam, acc, alb, nd = setup(rtw, W, H, spp=1)
        out = torch.empty_like(acc)
        stream = torch.cuda.Stream()
        for kw in CONFIGS.values():
            fn = denoise_call(rtw, world, W, H, acc, alb, nd, out, stream, rtw._abi.denoise_params(**kw))
            for _ in range(reps):
                fn()
            stream.synchronize()
        world.close()


def per_pass(trace_csv, rtw, reps):
    """Per-pass kernel microseconds from the trace: the calls come in the order of trace_child."""
    rows = []
    for r in csv.DictReader(open(trace_csv)):
        if "denoise_" in r["Kernel_Name"]:
            rows.append((int(r["Start_Timestamp"]), (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3,
                         "prepass" if "prepass" in r["Kernel_Name"] else "pass"))
    rows.sort()
    out, k = [], 0
    for W, H in FRAMES:
        for name, kw in CONFIGS.items():
            n = rtw._abi.denoise_params(**kw).passes
            calls = [rows[k + c * (n + 1): k + (c + 1) * (n + 1)] for c in range(reps)]
            k += reps * (n + 1)
            assert all(len(c) == n + 1 and c[0][2] == "prepass" and all(x[2] == "pass" for x in c[1:]) for c in calls), \
                "trace does not match the calls made"
            warm = calls[reps // 2:]                                         # the first half is the warm-up
            med = [statistics.median(c[j][1] for c in warm) for j in range(n + 1)]
            passes = []
            for i, us in enumerate(med[1:]):
                tbs = PASS_BYTES * W * H / (us * 1e-6) / 1e12
                passes.append({"pass": i, "spacing": 1 << i, "us": us, "tb_per_s": tbs, "share_of_copy_rate": tbs / COPY_TBS})
            out.append({"frame": [W, H], "config": name, "prepass_us": med[0], "passes": passes,
                        "kernels_us": sum(med), "calls_read": len(warm)})
    assert k == len(rows), (k, len(rows))
    return out


def readme(rep):
    lines = ["# Denoised previews: what the filter costs on the GPU", "",
             "`python tools/denoise_bench.py --out profiles/denoise` on one MI355X; the figures are in",
             "`denoise_bench.json` beside this file.  Times are HIP events on the caller's stream around one",
             f"call, median of {rep['reps']} after {rep['warmup']} warm-up calls; Book-1 at the same frame gives the price of a sample.", "",
             "| frame | configuration | passes | denoise ms (min .. max) | 1 spp ms | cost in spp | guides ms |",
             "|---|---|---|---|---|---|---|"]
    for f in rep["frames"]:
        for name, d in f["denoise"].items():
            lines.append(f"| {f['frame'][0]} x {f['frame'][1]} | {name} | {d['passes']} | {d['median_ms']:.3f} "
                         f"({d['min_ms']:.3f} .. {d['max_ms']:.3f}) | {f['render_1spp']['median_ms']:.3f} | "
                         f"{d['cost_spp']:.2f} | {f['guides']['median_ms']:.3f} |")
    if rep.get("per_pass"):
        lines += ["", "Per-pass kernel times (a separate `rocprofv3 --kernel-trace --stats` run; the median of the last "
                  f"{rep['trace_reps'] - rep['trace_reps'] // 2} of {rep['trace_reps']} calls per configuration), as {PASS_BYTES} B x pixels over the time, against the {COPY_TBS} TB/s copy rate "
                  "measured on this part.  A share of that copy rate, not of a bound: the planes are cache-resident.", "",
                  "| frame | configuration | pass | spacing | us | TB/s | share of the copy rate |", "|---|---|---|---|---|---|---|"]
        for c in rep["per_pass"]:
            lines.append(f"| {c['frame'][0]} x {c['frame'][1]} | {c['config']} | pre-pass | | {c['prepass_us']:.1f} | | |")
            for p in c["passes"]:
                lines.append(f"| | | {p['pass']} | {p['spacing']} | {p['us']:.1f} | {p['tb_per_s']:.2f} | "
                             f"{100 * p['share_of_copy_rate']:.0f} % |")
        ev = {(tuple(f["frame"]), k): v["median_ms"] for f in rep["frames"] for k, v in f["denoise"].items()}
        lines += ["", "The traced kernels of a call, summed, against the same call by HIP events in the other run (separate "
                  "processes; the per-pass shares above are of the traced times):", ""]
        for c in rep["per_pass"]:
            lines.append(f"- {c['frame'][0]} x {c['frame'][1]}, {c['config']}: {c['kernels_us'] / 1e3:.3f} ms traced, "
                         f"{ev[(tuple(c['frame']), c['config'])]:.3f} ms by events")
    if rep.get("notes"):
        lines += [""] + rep["notes"]
    return "\n".join(lines) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "denoise"))
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--trace-reps", type=int, default=20)
    ap.add_argument("--no-trace", action="store_true")
    ap.add_argument("--trace-child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--ab-child", action="store_true", help="one JSON line of denoise times (an A/B sample)")
    args = ap.parse_args()
    per = None
    if not (args.trace_child or args.ab_child or args.no_trace):
        # the trace first, in a child of its own, before this process opens the GPU
        with tempfile.TemporaryDirectory() as d:
            cmd = ["rocprofv3", "--kernel-trace", "--stats", "-d", d, "-o", "dn", "--output-format", "csv", "--",
                   sys.executable, os.path.abspath(__file__), "--trace-child", "--trace-reps", str(args.trace_reps)]
            # a process group of its own: on a timeout the traced grandchild goes with rocprofv3
            child = subprocess.Popen(cmd, stdout=subprocess.DEVNULL, start_new_session=True)
            try:
                rc = child.wait(timeout=300)
            except subprocess.TimeoutExpired:
                os.killpg(child.pid, signal.SIGKILL)
                child.wait()
                raise SystemExit("the rocprofv3 run did not finish in 300 s: killed with its process group")
            if rc != 0:
                raise SystemExit(f"the rocprofv3 run failed ({rc})")
            found = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)
            if len(found) != 1:
                raise SystemExit(f"rocprofv3 left {len(found)} kernel traces")
            rtw = importlib.import_module("zig-raytracing-weekend_amd")
            per = per_pass(found[0], rtw, args.trace_reps)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("denoise_bench needs a GPU (there is no fallback)")
    rtw = importlib.import_module("zig-raytracing-weekend_amd")
    if args.trace_child:
        trace_child(rtw, args.trace_reps)
        return
    frames = [measure(rtw, W, H, args.warmup, args.reps) for W, H in FRAMES]
    rep = {"device": torch.cuda.get_device_name(0), "build_id": rtw.lib().rtw_build_id().decode(),
           "lib": os.environ.get("RTW_LIB") or "in-tree", "warmup": args.warmup, "reps": args.reps,
           "trace_reps": args.trace_reps, "copy_rate_tb_per_s": COPY_TBS, "pass_bytes_per_pixel": PASS_BYTES,
           "frames": frames, "per_pass": per}
    if args.ab_child:
        print(json.dumps({"lib": rep["lib"], "denoise_ms": {f"{f['frame'][0]}x{f['frame'][1]} {k}": v["median_ms"]
                                                             for f in frames for k, v in f["denoise"].items()}}))
        return
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, "denoise_bench.json"), "w") as f:
        json.dump(rep, f, indent=1)
        f.write("\n")
    with open(os.path.join(args.out, "README.md"), "w") as f:
        f.write(readme(rep))
    print(readme(rep))


if __name__ == "__main__":
    main()
