#!/usr/bin/env python3
"""What ray queries deliver on the GPU (needs an MI355X; there is no fallback): Mrays/s of rtw_trace_rays_device and
rtw_occluded_device on

  * Book-1 at 1200 x 800, the C4 100 k-sphere scene at 1200 x 800 and Cornell at 1000 x 1000: the pixel-centre rays in
    image order, the same rays shuffled, and bounce rays (the first hits turned into one hemisphere direction each);
  * Cornell: bounded occlusion rays from the first hits to the centre of the light, tmax = the distance to it;

and, the only in-tree yardstick of a trace-only kernel, rtw_render_guides_device on the Book-1 frame in the same
session.  Times are HIP events on the caller's stream around one call (RTW_RENDER_NO_SYNC), the median of --reps
after --warmup calls, with the minimum and maximum beside it.

    python tools/query_bench.py --out profiles/queries      # writes query_bench.json and README.md there
    python tools/query_bench.py --resources                 # no GPU: the kernels' registers from the compiler,
                                                            # into profiles/queries/resources.json
"""
import argparse
import ctypes as C
import importlib
import json
import os
import re
import statistics
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
CSRC = os.path.join(REPO, "zig-raytracing-weekend_amd", "csrc")
RAY_BYTES, HIT_BYTES, GUIDE_BYTES = 32, 64, 32


# ---------------------------------------------------------------- the compiler's view (no GPU)
def resources(out_dir):
    """VGPRs, SGPRs, scratch and waves per SIMD of the query kernels and of guides_kernel, from
    -Rpass-analysis=kernel-resource-usage with the library's flags."""
    mk = open(os.path.join(CSRC, "Makefile")).read()
    flags = re.search(r"^HIPFLAGS = (.*\\\n.*)$", mk, re.M).group(1).replace("\\\n", " ")
    flags = flags.replace("$(ARCH)", "gfx950").replace("$(EXTRA_DEFS)", "").split()
    rows = []
    for src in ("rtw_query.hip", "rtw_denoise.hip"):
        p = subprocess.run(["/opt/rocm/bin/hipcc"] + flags + ["--cuda-device-only", "-c", src, "-o", os.devnull,
                                                              "-Rpass-analysis=kernel-resource-usage"],
                           cwd=CSRC, capture_output=True, text=True, check=True)
        cur = None
        for line in p.stderr.splitlines():
            m = re.search(r"remark: (?:\s*)([A-Za-z ]+?)(?: \[[^\]]*\])?: (\S+)", line)
            if not m:
                continue
            key, val = m.group(1).strip(), m.group(2)
            if key == "Function Name":
                name = subprocess.run(["c++filt", val], capture_output=True, text=True).stdout.strip()
                short = re.sub(r"^void \(anonymous namespace\)::", "", name).split("(")[0]
                cur = {"kernel": short} if re.match(r"(query_|guides_)", short) else None
                if cur:
                    rows.append(cur)
            elif cur is not None and key in ("VGPRs", "TotalSGPRs", "ScratchSize", "Occupancy"):
                cur[{"VGPRs": "vgpr", "TotalSGPRs": "sgpr", "ScratchSize": "scratch", "Occupancy": "waves_per_simd"}[key]] = int(val)
    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, "resources.json"), "w") as f:
        json.dump({"flags": " ".join(flags), "kernels": rows}, f, indent=1)
        f.write("\n")
    return rows


# ---------------------------------------------------------------- ray sets (torch, on the device)
def pixel_rays(rtw, cam):
    """(N, 8) pixel-centre rays of the camera in image order: from the centre, unbounded, time 0."""
    import torch
    d = cam.derived
    f = lambda v: torch.tensor(list(v), dtype=torch.float32, device="cuda")
    ys, xs = torch.meshgrid(torch.arange(d.image_height, device="cuda"), torch.arange(d.image_width, device="cuda"),
                            indexing="ij")
    fx = (xs.reshape(-1, 1) + d.pixel_offset).float()
    fy = (ys.reshape(-1, 1) + d.pixel_offset).float()
    pc = (f(d.pixel00_loc) + f(d.pixel_delta_u) * fx) + f(d.pixel_delta_v) * fy
    c = f(d.center)
    return rtw.ray_rows(c.expand_as(pc), pc - c)


def bounce_rays(rtw, hits, gen):
    """The first hits turned into one direction each, uniform over the hemisphere about the record's normal."""
    import torch
    h = rtw.hit_columns(hits)
    keep = h["hit"]
    p, n = h["p"][keep], h["normal"][keep]
    v = torch.randn(p.shape, generator=gen, device="cuda")
    v = v / v.norm(dim=1, keepdim=True)
    v = torch.where((v * n).sum(1, keepdim=True) < 0, -v, v)
    return rtw.ray_rows(p.contiguous(), v)


def light_rays(rtw, hits, light):
    """From the first hits to the point `light`: unit directions, tmax = the distance."""
    import torch
    h = rtw.hit_columns(hits)
    p = h["p"][h["hit"]].contiguous()
    d = torch.tensor(light, dtype=torch.float32, device="cuda") - p
    dist = d.norm(dim=1)
    ok = dist > 1e-3
    return rtw.ray_rows(p[ok], d[ok] / dist[ok, None], tmax=dist[ok])


# ---------------------------------------------------------------- timing
def timed(fn, stream, warmup, reps):
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


def summary(ms, n):
    med = statistics.median(ms)
    return {"rays": n, "median_ms": med, "min_ms": min(ms), "max_ms": max(ms), "reps": len(ms),
            "mrays_per_s": n / med / 1e3, "mrays_per_s_worst": n / max(ms) / 1e3, "mrays_per_s_best": n / min(ms) / 1e3}


def measure_set(world, rays, stream, warmup, reps):
    import torch
    n = rays.shape[0]
    hits = torch.empty((n, 16), dtype=torch.int32, device="cuda")
    occ = torch.empty((n,), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    res = {"closest": summary(timed(lambda: world.trace_device(rays, hits, stream=stream), stream, warmup, reps), n),
           "any": summary(timed(lambda: world.occluded_device(rays, occ, stream=stream), stream, warmup, reps), n)}
    stream.synchronize()
    res["hit_fraction"] = float(occ.float().mean())
    assert int(occ.sum()) == int((hits[:, 1] != -1).sum()), "occluded disagrees with trace"
    return res


SCENES = {
    "book1": ("Book-1, 1200 x 800", lambda rtw: rtw.worlds.generate_world(0, "book1"),
              lambda rtw: rtw.book1_camera(image_width=1200, aspect_ratio=1.5, spp=1)),
    "c4": ("C4: 100 k spheres, 1200 x 800", lambda rtw: rtw.worlds.stress_world(100_000, 0),
           lambda rtw: rtw.book1_camera(image_width=1200, aspect_ratio=1.5, spp=1)),
    "cornell": ("Cornell, 1000 x 1000", lambda rtw: rtw.worlds.cornell_box(), lambda rtw: rtw.cornell_camera(1000, 1)),
}
CORNELL_LIGHT = (278.0, 554.0, 279.5)      # the centre of the ceiling light


def measure(rtw, warmup, reps, seed=0):
    import torch
    out = {}
    stream = torch.cuda.Stream()
    for key, (title, objs, camera) in SCENES.items():
        world = rtw.World(rtw.flatten(objs(rtw)), device=0)
        cam = camera(rtw).init()
        gen = torch.Generator(device="cuda")
        gen.manual_seed(seed)
        ordered = pixel_rays(rtw, cam)
        first = world.trace_device(ordered)
        sets = {"ordered": ordered,
                "shuffled": ordered[torch.randperm(ordered.shape[0], generator=gen, device="cuda")].contiguous(),
                "bounce": bounce_rays(rtw, first, gen)}
        if key == "cornell":
            sets["to the light (bounded)"] = light_rays(rtw, first, CORNELL_LIGHT)
        res = {"title": title, "sets": {k: measure_set(world, v, stream, warmup, reps) for k, v in sets.items()}}
        for kind in ("closest", "any"):
            res["shuffled_over_ordered_" + kind] = (res["sets"]["shuffled"][kind]["median_ms"] /
                                                    res["sets"]["ordered"][kind]["median_ms"])
        if key == "book1":
            alb = torch.empty((cam.size, 4), dtype=torch.float32, device="cuda")
            nd = torch.empty_like(alb)
            sp = C.c_void_p(stream.cuda_stream)

            def guides():
                rtw._abi.check(rtw.lib().rtw_render_guides_device(world.handle, C.byref(cam.derived), alb.data_ptr(),
                                                                  nd.data_ptr(), sp, rtw._abi.RTW_RENDER_NO_SYNC),
                               "rtw_render_guides_device")
            res["guides"] = summary(timed(guides, stream, warmup, reps), cam.size)
            res["closest_ordered_over_guides"] = res["sets"]["ordered"]["closest"]["median_ms"] / res["guides"]["median_ms"]
        torch.cuda.synchronize()
        world.close()
        out[key] = res
    return out


def readme(rep, res):
    L = ["# Ray queries: what the trace-only kernels deliver", "",
         "`python tools/query_bench.py --out profiles/queries` on one MI355X; the figures are in `query_bench.json`",
         "beside this file.  One call of `rtw_trace_rays_device` (closest hit: 32 B read and 64 B written per ray) or",
         "`rtw_occluded_device` (any hit: 32 B read, 1 B written) per measurement, timed by HIP events on the caller's",
         f"stream; the median of {rep['reps']} calls after {rep['warmup']} warm-up calls, the slowest and the fastest call in brackets.",
         "Pixel-centre rays of the scene's camera in image order, the same rays shuffled, and bounce rays: every",
         "first hit turned into one direction of the hemisphere about its normal (the misses dropped).", "",
         "| scene | rays | count | hit | closest Mrays/s | any-hit Mrays/s |", "|---|---|---|---|---|---|"]
    cell = lambda s: f"{s['mrays_per_s']:.0f} ({s['mrays_per_s_worst']:.0f} .. {s['mrays_per_s_best']:.0f})"
    for sc in rep["scenes"].values():
        for name, s in sc["sets"].items():
            L.append(f"| {sc['title']} | {name} | {s['closest']['rays']} | {100 * s['hit_fraction']:.0f} % | "
                     f"{cell(s['closest'])} | {cell(s['any'])} |")
    L += ["", "Shuffled over ordered, as a ratio of times (1 = no loss; the walk's coherence, with no shading in the kernel):", ""]
    for sc in rep["scenes"].values():
        L.append(f"- {sc['title']}: closest {sc['shuffled_over_ordered_closest']:.2f} x, any-hit "
                 f"{sc['shuffled_over_ordered_any']:.2f} x")
    b = rep["scenes"]["book1"]
    g = b["guides"]
    L += ["", "## Against `guides_kernel`", "",
          f"`rtw_render_guides_device` on the Book-1 frame in the same session: {g['median_ms']:.4f} ms "
          f"({g['min_ms']:.4f} .. {g['max_ms']:.4f}).  The closest-hit query on the image-order rays takes "
          f"{b['sets']['ordered']['closest']['median_ms']:.4f} ms: **{b['closest_ordered_over_guides']:.2f} x** the guides.",
          f"The query moves {RAY_BYTES + HIT_BYTES} B per ray against the guides' {GUIDE_BYTES} B (two float4 stores, the ray",
          "computed from kernel arguments)."]
    if res:
        L += ["", "## Registers (the compiler's view)", "",
              "`python tools/query_bench.py --resources`: `-Rpass-analysis=kernel-resource-usage` with the library's flags;",
              "the template argument is the feature class (63: every feature but the media, 191: with instance trees,",
              "703: with vertex attributes).", "",
              "| kernel | VGPRs | SGPRs | scratch B/lane | waves / SIMD |", "|---|---|---|---|---|"]
        for k in res["kernels"]:
            L.append(f"| `{k['kernel']}` | {k['vgpr']} | {k['sgpr']} | {k['scratch']} | {k['waves_per_simd']} |")
    L += ["", "This file is written by the tool.  What the figures say is in `FINDINGS.md` beside it, written by hand."]
    return "\n".join(L) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "queries"))
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--resources", action="store_true", help="only the compiler's register report (no GPU)")
    ap.add_argument("--readme", action="store_true", help="only rewrite README.md from the JSON files (no GPU)")
    args = ap.parse_args()
    res_path = os.path.join(args.out, "resources.json")
    bench_path = os.path.join(args.out, "query_bench.json")
    if args.resources:
        for k in resources(args.out):
            print(k)
    elif not args.readme:
        import torch
        if not torch.cuda.is_available():
            raise SystemExit("query_bench needs a GPU (there is no fallback)")
        rtw = importlib.import_module("zig-raytracing-weekend_amd")
        rep = {"device": torch.cuda.get_device_name(0), "build_id": rtw.lib().rtw_build_id().decode(),
               "warmup": args.warmup, "reps": args.reps, "scenes": measure(rtw, args.warmup, args.reps)}
        os.makedirs(args.out, exist_ok=True)
        with open(bench_path, "w") as f:
            json.dump(rep, f, indent=1)
            f.write("\n")
    if os.path.exists(bench_path):
        rep = json.load(open(bench_path))
        text = readme(rep, json.load(open(res_path)) if os.path.exists(res_path) else None)
        with open(os.path.join(args.out, "README.md"), "w") as f:
            f.write(text)
        print(text)


if __name__ == "__main__":
    main()
