#!/usr/bin/env python3
"""What the temporal reprojection costs on the GPU (needs an MI355X; there is no fallback): writes
profiles/temporal/temporal_bench.json and prints the table that profiles/temporal/README.md quotes.  For 1200 x 800
and 3840 x 2160 frames of Book-1

  * rtw_temporal_accumulate_device per call -- a still camera (every pixel snaps to one tap), a camera moved sideways
    and one panned (four taps), each with and without the moments -- as bytes over the copy rate and in units of one
    1-spp render batch at the same frame;
  * with --variant-lib: the block-shape A/B, alternating pairs of fresh processes (A: the in-tree library, blocks of
    32 x 8 pixels; B: the build with -DRTW_TEMPORAL_BLOCK_W=64, 64 x 4);
  * with --parent-lib: bench.py (C2) alternating between the parent's library and the in-tree one, three rounds.

Times are HIP events on the caller's stream around one call, median of 30 after 5 warm-up calls, with the fastest and
the slowest beside it.

    python tools/temporal_bench.py [--variant-lib build/rtw_temporal_w64.so] [--parent-lib build/rtw_parent.so]
    RTW_LIB=build/rtw_x.so python tools/temporal_bench.py --ab-child    # one A/B sample: a JSON line
"""
import argparse
import ctypes as C
import dataclasses
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import denoise_bench as B  # noqa: E402  (setup, timed, summary, the frames and the copy rate)
import denoise_guided_bench as GB  # noqa: E402  (bench_ab: bench.py on two libraries, alternating)

REPO, FRAMES, COPY_TBS = B.REPO, B.FRAMES, B.COPY_TBS
# what a call must move per pixel: the two current frames and out_accum, one tap's worth of the two previous frames,
# the history; with the moments also plane 1 of the previous ones and both planes written
BYTES = {False: 16 + 16 + 16 + 16 + 16 + 4, True: 16 + 16 + 16 + 16 + 16 + 4 + 16 + 32}
MOVES = {"still": (0.0, 0.0), "sideways": (0.05, 0.0), "panned": (0.0, 0.05)}   # lookfrom.x / lookat.x, world units


def moved(rtw, cam, dfrom, dat):
    f, a = list(cam.lookfrom), list(cam.lookat)
    f[0] += dfrom
    a[0] += dat + dfrom
    return dataclasses.replace(cam, derived=None, strata=0, lookfrom=tuple(f), lookat=tuple(a)).init()


def measure(rtw, W, H, warmup, reps):
    import torch
    A, L = rtw._abi, rtw.lib()
    world, prev_cam, prev_acc, _, prev_nd = B.setup(rtw, W, H, spp=4)
    n = prev_cam.size
    stream = torch.cuda.Stream()
    sp = C.c_void_p(stream.cuda_stream)
    NS = A.RTW_RENDER_NO_SYNC
    opts = A.render_opts(flags=NS)
    mom = torch.zeros((2, n, 4), dtype=torch.float32, device="cuda")
    A.check(L.rtw_moments_update_device(world.handle, W, H, prev_acc.data_ptr(), mom.data_ptr(), None, 0), "moments")
    cur = torch.zeros((n, 4), dtype=torch.float32, device="cuda")
    alb, nd = torch.empty_like(cur), torch.empty_like(cur)
    out, om = torch.empty_like(cur), torch.empty_like(mom)
    hist = torch.empty(n, dtype=torch.float32, device="cuda")
    p = A.temporal_params()
    s = [0]

    def render_1spp():
        A.check(L.rtw_render_device(world.handle, C.byref(prev_cam.derived), 0, n, s[0], s[0] + 1, 1, cur.data_ptr(), sp,
                                    C.byref(opts)), "rtw_render_device")
        s[0] += 1
    torch.cuda.synchronize()
    res = {"frame": [W, H], "render_1spp": B.summary(B.timed(render_1spp, stream, warmup, reps)), "calls": {}}
    for name, (dfrom, dat) in MOVES.items():
        cam = moved(rtw, prev_cam, dfrom, dat)
        cur.zero_()
        torch.cuda.synchronize()
        A.check(L.rtw_render_device(world.handle, C.byref(cam.derived), 0, n, 0, 2, 2, cur.data_ptr(), None, None), "render")
        A.check(L.rtw_render_guides_device(world.handle, C.byref(cam.derived), alb.data_ptr(), nd.data_ptr(), None, 0), "guides")
        torch.cuda.synchronize()
        for with_m in (False, True):
            def call():
                A.check(L.rtw_temporal_accumulate_device(
                    world.handle, C.byref(cam.derived), C.byref(prev_cam.derived), cur.data_ptr(), nd.data_ptr(),
                    prev_acc.data_ptr(), prev_nd.data_ptr(), mom.data_ptr() if with_m else None, C.byref(p),
                    out.data_ptr(), om.data_ptr() if with_m else None, hist.data_ptr(), sp, NS), "rtw_temporal_accumulate_device")
            r = B.summary(B.timed(call, stream, warmup, reps))
            r["bytes_per_pixel"] = BYTES[with_m]
            r["share_of_copy_rate"] = BYTES[with_m] * n / (r["median_ms"] * 1e-3) / 1e12 / COPY_TBS
            r["cost_spp"] = r["median_ms"] / res["render_1spp"]["median_ms"]
            r["pixels_with_history"] = float((hist > 0).float().mean().item())
            res["calls"][f"{name}, {'with' if with_m else 'without'} moments"] = r
    torch.cuda.synchronize()
    world.close()
    return res


def shape_ab(variant_lib, pairs):
    me = [sys.executable, os.path.abspath(__file__), "--ab-child"]
    rows = []
    for _ in range(pairs):
        rows.append({"side": "A", **GB.child(None, me)})
        rows.append({"side": "B", **GB.child(variant_lib, me)})
    return rows


def table(rep):
    L = ["| frame | camera | 1 spp ms | call ms | in spp | B / pixel | share of the copy rate | pixels with history |",
         "|---|---|---|---|---|---|---|---|"]
    for f in rep["frames"]:
        for name, r in f["calls"].items():
            L.append(f"| {f['frame'][0]} x {f['frame'][1]} | {name} | {f['render_1spp']['median_ms']:.3f} | {r['median_ms']:.4f} "
                     f"({r['min_ms']:.4f} .. {r['max_ms']:.4f}) | {r['cost_spp']:.3f} | {r['bytes_per_pixel']} | "
                     f"{100 * r['share_of_copy_rate']:.0f} % | {100 * r['pixels_with_history']:.0f} % |")
    if rep.get("shape_ab"):
        L += ["", "| frame, camera | A: 32 x 8 | B: 64 x 4 | B / A (medians) |", "|---|---|---|---|"]
        for k in rep["shape_ab"][0]["ms"]:
            a = [r["ms"][k] for r in rep["shape_ab"] if r["side"] == "A"]
            b = [r["ms"][k] for r in rep["shape_ab"] if r["side"] == "B"]
            L.append(f"| {k} | {GB.span(a)} | {GB.span(b)} | {GB.statistics.median(b) / GB.statistics.median(a):.3f} |")
    if rep.get("bench_ab"):
        pa = [r["value"] for r in rep["bench_ab"] if r["side"] == "parent"]
        th = [r["value"] for r in rep["bench_ab"] if r["side"] == "this"]
        L += ["", f"bench.py --gpus 1 --steps {rep['bench_steps']} --warmup {rep['bench_warmup']}, alternating "
                  f"({rep['bench_ab'][0].get('unit') or ''}): parent {', '.join(f'{v:.2f}' for v in pa)}; this tree "
                  f"{', '.join(f'{v:.2f}' for v in th)}"]
    return "\n".join(L) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "temporal"))
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--variant-lib", help="the -DRTW_TEMPORAL_BLOCK_W=64 build: runs the block-shape A/B")
    ap.add_argument("--pairs", type=int, default=3)
    ap.add_argument("--ab-child", action="store_true", help="one JSON line of call times (an A/B sample)")
    ap.add_argument("--parent-lib", help="the parent commit's library: runs bench.py on both, alternating")
    ap.add_argument("--bench-steps", type=int, default=5)
    ap.add_argument("--bench-warmup", type=int, default=1)
    args = ap.parse_args()
    # the children first, each a fresh process, before this one opens the GPU
    sab = shape_ab(args.variant_lib, args.pairs) if args.variant_lib and not args.ab_child else None
    bab = GB.bench_ab(args.parent_lib, 3, args.bench_steps, args.bench_warmup) if args.parent_lib and not args.ab_child else None
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("temporal_bench needs a GPU (there is no fallback)")
    rtw = B.importlib.import_module("zig-raytracing-weekend_amd")
    frames = [measure(rtw, W, H, args.warmup, args.reps) for W, H in FRAMES]
    if args.ab_child:
        print(json.dumps({"lib": GB.lib_name(os.environ.get("RTW_LIB")),
                          "ms": {f"{f['frame'][0]} x {f['frame'][1]}, {k}": r["median_ms"]
                                 for f in frames for k, r in f["calls"].items()}}))
        return
    rep = {"device": torch.cuda.get_device_name(0), "build_id": rtw.lib().rtw_build_id().decode(), "warmup": args.warmup,
           "reps": args.reps, "copy_rate_tb_per_s": COPY_TBS, "frames": frames, "shape_ab": sab, "bench_ab": bab,
           "bench_steps": args.bench_steps, "bench_warmup": args.bench_warmup}
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, "temporal_bench.json"), "w") as f:
        json.dump(rep, f, indent=1)
        f.write("\n")
    print(table(rep))


if __name__ == "__main__":
    main()
