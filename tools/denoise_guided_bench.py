#!/usr/bin/env python3
"""What the noise estimates and the guided filter cost on the GPU (needs an MI355X; there is no fallback): writes
profiles/denoise_guided/README.md and guided_bench.json.  For 1200 x 800 and 3840 x 2160 frames of Book-1

  * rtw_denoise_guided_device against rtw_denoise_device on the same frames, the shipped defaults of each and 5 passes,
    alternating in one session;
  * rtw_moments_update_device and rtw_noise_estimate_device per call, in units of one 1-spp render batch at the same
    frame and as bytes over the copy rate;
  * with --nolds-lib: the LDS A/B of the guided passes, five alternating pairs of fresh processes (A: the build with
    -DRTW_GUIDED_NO_LDS, B: the in-tree library);
  * with --parent-lib: bench.py (C2) alternating between the parent's library and the in-tree one, three rounds.

Times are HIP events on the caller's stream around one call, median of 30 after 5 warm-up calls, with the fastest and
the slowest beside it.

    python tools/denoise_guided_bench.py [--nolds-lib build/rtw_guided_nolds.so] [--parent-lib build/rtw_parent.so]
    RTW_LIB=build/rtw_x.so python tools/denoise_guided_bench.py --ab-child    # one A/B sample: a JSON line
"""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import denoise_bench as B  # noqa: E402  (setup, timed, summary, the frames and the copy rate)

REPO, FRAMES, COPY_TBS = B.REPO, B.FRAMES, B.COPY_TBS
CONFIGS = {"defaults": {}, "5 passes": dict(passes=5)}
# what one pass must move per pixel: two 16-B planes read and one written; the guided pass also reads and writes a
# 4-B variance plane
PLAIN_BYTES, GUIDED_BYTES = 48, 56
MOMENTS_BYTES = 16 + 32 + 32      # the accumulator read, both planes read and written
NOISE_BYTES = 16 + 4              # plane 1 read, err written (tile_max and the summary are noise beside them)


def measure(rtw, W, H, warmup, reps, rounds, filters_only=False):
    import torch
    A, L = rtw._abi, rtw.lib()
    world, cam, acc, alb, nd = B.setup(rtw, W, H, spp=1)
    n = cam.size
    out, var = torch.empty_like(acc), torch.empty(n, dtype=torch.float32, device="cuda")
    mom = torch.zeros((2, n, 4), dtype=torch.float32, device="cuda")
    err = torch.empty(n, dtype=torch.float32, device="cuda")
    tiles = torch.empty(((H + 7) // 8) * ((W + 7) // 8), dtype=torch.float32, device="cuda")
    summ = torch.zeros(6, dtype=torch.float32, device="cuda")
    stream = torch.cuda.Stream()
    sp = C.c_void_p(stream.cuda_stream)
    NS = A.RTW_RENDER_NO_SYNC
    opts = A.render_opts(flags=NS)
    s = [1]

    def render_1spp():
        A.check(L.rtw_render_device(world.handle, C.byref(cam.derived), 0, n, s[0], s[0] + 1, 0, acc.data_ptr(), sp,
                                    C.byref(opts)), "rtw_render_device")
        s[0] += 1

    def moments():
        # every timed call folds a new batch: a call that finds nothing new writes nothing and would flatter the figure
        render_1spp()
        stream.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        A.check(L.rtw_moments_update_device(world.handle, W, H, acc.data_ptr(), mom.data_ptr(), sp, NS),
                "rtw_moments_update_device")
        b.record()
        b.synchronize()
        return a.elapsed_time(b)

    def noise():
        A.check(L.rtw_noise_estimate_device(world.handle, W, H, mom.data_ptr(), 0.01, 0.05, err.data_ptr(),
                                            tiles.data_ptr(), summ.data_ptr(), sp, NS), "rtw_noise_estimate_device")

    def plain(p):
        return lambda: A.check(L.rtw_denoise_device(world.handle, W, H, acc.data_ptr(), alb.data_ptr(), nd.data_ptr(),
                                                    C.byref(p), out.data_ptr(), sp, NS), "rtw_denoise_device")

    def guided(p):
        return lambda: A.check(L.rtw_denoise_guided_device(world.handle, W, H, acc.data_ptr(), mom.data_ptr(),
                                                           alb.data_ptr(), nd.data_ptr(), C.byref(p), out.data_ptr(),
                                                           var.data_ptr(), sp, NS), "rtw_denoise_guided_device")
    torch.cuda.synchronize()
    res = {"frame": [W, H], "render_1spp": B.summary(B.timed(render_1spp, stream, warmup, reps))}
    with torch.cuda.stream(stream):
        ms = [moments() for _ in range(2 if filters_only else warmup + reps)][0 if filters_only else warmup:]
    res["moments_update"] = B.summary(ms)
    res["noise_estimate"] = B.summary(B.timed(noise, stream, warmup, 1 if filters_only else reps))
    for key, nbytes in (("moments_update", MOMENTS_BYTES), ("noise_estimate", NOISE_BYTES)):
        r = res[key]
        r["cost_spp"] = r["median_ms"] / res["render_1spp"]["median_ms"]
        r["bytes_per_pixel"] = nbytes
        r["share_of_copy_rate"] = nbytes * n / (r["median_ms"] * 1e-3) / 1e12 / COPY_TBS
    res["filters"] = {}
    for name, kw in CONFIGS.items():
        pp, pg = A.denoise_params(**kw), A.denoise_guided_params(**kw)
        tp, tg = [], []
        for _ in range(rounds):                                              # alternating in one session
            tp += B.timed(plain(pp), stream, warmup, reps)
            tg += B.timed(guided(pg), stream, warmup, reps)
        rp, rg = B.summary(tp), B.summary(tg)
        for r, p, nbytes in ((rp, pp, PLAIN_BYTES), (rg, pg, GUIDED_BYTES)):
            r["passes"] = p.passes
            r["share_of_copy_rate"] = nbytes * p.passes * n / (r["median_ms"] * 1e-3) / 1e12 / COPY_TBS
        res["filters"][name] = {"plain": rp, "guided": rg, "ratio": rg["median_ms"] / rp["median_ms"],
                                "guided_cost_spp": rg["median_ms"] / res["render_1spp"]["median_ms"]}
    torch.cuda.synchronize()
    world.close()
    return res


def lib_name(path):
    """How a record names a library: its path inside the repository, or its file name; "in-tree" for the product."""
    if not path:
        return "in-tree"
    rel = os.path.relpath(os.path.abspath(path), REPO)
    return os.path.basename(path) if rel.startswith("..") else rel


def child(env_lib, args, timeout=300):
    env = dict(os.environ)
    env.pop("RTW_LIB", None)
    if env_lib:
        env["RTW_LIB"] = os.path.abspath(env_lib)
    out = subprocess.run(args, env=env, cwd=REPO, stdout=subprocess.PIPE, timeout=timeout, check=True, text=True).stdout
    return json.loads(out.strip().splitlines()[-1])


def lds_ab(nolds_lib, pairs):
    me = [sys.executable, os.path.abspath(__file__), "--ab-child"]
    rows = []
    for _ in range(pairs):
        rows.append({"side": "A", **child(nolds_lib, me)})
        rows.append({"side": "B", **child(None, me)})
    return rows


def bench_ab(parent_lib, rounds, steps, warmup):
    cmd = [sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup)]
    rows = []
    for _ in range(rounds):
        for side, lib in (("parent", parent_lib), ("this", None)):
            r = child(lib, cmd, timeout=600)
            rows.append({"side": side, "value": r["value"], "unit": r.get("unit")})
    return rows


def span(v):
    return f"{statistics.median(v):.4f} ({min(v):.4f} .. {max(v):.4f})"


def readme(rep):
    L = ["# Noise estimates and the guided filter: what they cost on the GPU", "",
         "`python tools/denoise_guided_bench.py --nolds-lib ... --parent-lib ...` on one MI355X; the figures are in",
         "`guided_bench.json` beside this file.  Times are HIP events on the caller's stream around one call, median of",
         f"{rep['reps']} after {rep['warmup']} warm-up calls (fastest .. slowest beside it); Book-1 at the same frame gives the",
         "price of a sample.", "",
         "## The guided filter against `rtw_denoise`", "",
         f"The same frames, alternating in one session ({rep['rounds']} rounds of {rep['reps']} calls each side).  The share is",
         f"{PLAIN_BYTES} B (plain) or {GUIDED_BYTES} B (guided: the variance plane read and written too) x pixels x passes over the",
         f"time, against the {COPY_TBS} TB/s copy rate measured on this part: a share of that rate, not of a bound -- the",
         "planes are cache-resident, the taps re-read them through LDS / L1 / L2, and the pre-pass is left out of the bytes.", "",
         "| frame | configuration | passes | plain ms | share | guided ms | share | guided / plain | guided in spp |",
         "|---|---|---|---|---|---|---|---|---|"]
    for f in rep["frames"]:
        for name, d in f["filters"].items():
            p, g = d["plain"], d["guided"]
            L.append(f"| {f['frame'][0]} x {f['frame'][1]} | {name} | {p['passes']} / {g['passes']} | {p['median_ms']:.4f} "
                     f"({p['min_ms']:.4f} .. {p['max_ms']:.4f}) | {100 * p['share_of_copy_rate']:.0f} % | {g['median_ms']:.4f} "
                     f"({g['min_ms']:.4f} .. {g['max_ms']:.4f}) | {100 * g['share_of_copy_rate']:.0f} % | {d['ratio']:.2f} | "
                     f"{d['guided_cost_spp']:.2f} |")
    L += ["", "## Moments and the estimate: what a viewer pays per refresh", "",
          f"Each a single streaming pass: {MOMENTS_BYTES} B per pixel for the update (the accumulator read, both planes read and",
          f"written; every timed update folds a fresh 1-spp batch), {NOISE_BYTES} B for the estimate (plane 1 read, err written).", "",
          "| frame | 1 spp ms | update ms | in spp | share of the copy rate | estimate ms | in spp | share of the copy rate |",
          "|---|---|---|---|---|---|---|---|"]
    for f in rep["frames"]:
        m, e = f["moments_update"], f["noise_estimate"]
        L.append(f"| {f['frame'][0]} x {f['frame'][1]} | {f['render_1spp']['median_ms']:.3f} | {m['median_ms']:.4f} "
                 f"({m['min_ms']:.4f} .. {m['max_ms']:.4f}) | {m['cost_spp']:.3f} | {100 * m['share_of_copy_rate']:.0f} % | "
                 f"{e['median_ms']:.4f} ({e['min_ms']:.4f} .. {e['max_ms']:.4f}) | {e['cost_spp']:.3f} | "
                 f"{100 * e['share_of_copy_rate']:.0f} % |")
    if rep.get("lds_ab"):
        L += ["", "## LDS tiling of the guided filter's first two passes: A/B", "",
              "A: every pass takes its taps (25 + 9 of three planes) through L1 / L2 (`-DRTW_GUIDED_NO_LDS`).  B: the passes with",
              "spacing 1 and 2 stage colour, guide and variance tiles with their halo in LDS, as `rtw_denoise`'s do.  Fresh",
              "processes alternating A, B, A, B, ...; each sample the median of a process's calls, ms (median, min .. max of the",
              "samples).", "", "| frame, configuration | A | B | B / A (medians) |", "|---|---|---|---|"]
        keys = list(rep["lds_ab"][0]["guided_ms"])
        for k in keys:
            a = [r["guided_ms"][k] for r in rep["lds_ab"] if r["side"] == "A"]
            b = [r["guided_ms"][k] for r in rep["lds_ab"] if r["side"] == "B"]
            L.append(f"| {k} | {span(a)} | {span(b)} | {statistics.median(b) / statistics.median(a):.2f} |")
    if rep.get("bench_ab"):
        pa = [r["value"] for r in rep["bench_ab"] if r["side"] == "parent"]
        th = [r["value"] for r in rep["bench_ab"] if r["side"] == "this"]
        unit = rep["bench_ab"][0].get("unit") or ""
        L += ["", "## `bench.py` (C2) against the parent's library", "",
              f"`python bench.py --gpus 1 --steps {rep['bench_steps']} --warmup {rep['bench_warmup']}`, the parent's library and this tree's",
              f"alternating, {len(pa)} rounds ({unit}): parent {', '.join(f'{v:.2f}' for v in pa)}; this tree",
              f"{', '.join(f'{v:.2f}' for v in th)}.  No render kernel changed (`profiles/isa_resources.json`)."]
    L += ["", "What the figures led to, and what they leave open, is in `NOTES.md` beside this file (kept by hand: this tool does",
          "not write it)."]
    return "\n".join(L) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "denoise_guided"))
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--nolds-lib", help="the -DRTW_GUIDED_NO_LDS build: runs the LDS A/B")
    ap.add_argument("--pairs", type=int, default=5)
    ap.add_argument("--parent-lib", help="the parent commit's library: runs bench.py on both, alternating")
    ap.add_argument("--bench-steps", type=int, default=5)
    ap.add_argument("--bench-warmup", type=int, default=1)
    ap.add_argument("--ab-child", action="store_true", help="one JSON line of guided filter times (an A/B sample)")
    args = ap.parse_args()
    # the children first, each a fresh process, before this one opens the GPU
    ab = lds_ab(args.nolds_lib, args.pairs) if args.nolds_lib and not args.ab_child else None
    bab = bench_ab(args.parent_lib, 3, args.bench_steps, args.bench_warmup) if args.parent_lib and not args.ab_child else None
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("denoise_guided_bench needs a GPU (there is no fallback)")
    rtw = B.importlib.import_module("zig-raytracing-weekend_amd")
    frames = [measure(rtw, W, H, args.warmup, args.reps, 1 if args.ab_child else args.rounds, args.ab_child)
              for W, H in FRAMES]
    if args.ab_child:
        print(json.dumps({"lib": lib_name(os.environ.get("RTW_LIB")),
                          "guided_ms": {f"{f['frame'][0]} x {f['frame'][1]}, {k}": v["guided"]["median_ms"]
                                        for f in frames for k, v in f["filters"].items()}}))
        return
    rep = {"device": torch.cuda.get_device_name(0), "build_id": rtw.lib().rtw_build_id().decode(), "warmup": args.warmup,
           "reps": args.reps, "rounds": args.rounds, "copy_rate_tb_per_s": COPY_TBS, "frames": frames, "lds_ab": ab,
           "bench_ab": bab, "bench_steps": args.bench_steps, "bench_warmup": args.bench_warmup}
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, "guided_bench.json"), "w") as f:
        json.dump(rep, f, indent=1)
        f.write("\n")
    with open(os.path.join(args.out, "README.md"), "w") as f:
        f.write(readme(rep))
    print(readme(rep))


if __name__ == "__main__":
    main()
