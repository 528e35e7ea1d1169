"""Resampled light picks (rtr_pick_slots_ris) on sponza_class at 1920x1080, 1 spp — the bench frame's 2 073 600 camera hits — beside the
calls whose place they take: one JSON object, printed and written to profiles/ris/ris_rate_1080p.json.

  kernels      rtr_pick_slots_ris at M = 1, 2, 4, 8 and 16, plain and with RTR_RIS_MIS, beside rtr_pick_slots_power and
               rtr_mis_pick_weights_power (what one call of it replaces), and rtr_shade_hits_picked at P = 1 for scale, on the same hits
  loops        api.path_trace_ris (M = 4) against api.path_trace_power, 1 and 2 bounces, wall time of a frame; with --parent-root (a
               checkout of the parent commit with its library built) api.path_trace_power as the PARENT builds it, in a child process of
               its own before this process opens the device, run twice around this tree's so that its own spread stands beside the
               difference
  variance     the same scene at 640x360, 1 bounce, pick_from=0, frames 0 ... N - 1: the per-pixel variance of radiance — mean, median,
               99.9th percentile, maximum — for resampled picks (path_trace_ris, M = 4 and 16, sky_samples=0) against power picks
               (path_trace_power), and the image sums with their standard errors

The kernels are enqueued through the Python wrappers in their asynchronous forms, HIP events on the context's stream, which is torch's
current stream; three warm-up calls, then at least 0.2 s of timed calls per repeat.  The five repeats of the cases are interleaved, and
the minimum is reported beside the median and all five.  No time is asserted anywhere.

    python profiles/ris_rate.py [--parent-root DIR] [--width 1920 --height 1080] [--frames 32] [--out profiles/ris/ris_rate_1080p.json]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CANDIDATES = (1, 2, 4, 8, 16)


def five_each(fns):
    """the repeats of several loops interleaved, so that a drift of the clock is in all of them alike"""
    ms = {k: [] for k in fns}
    for _ in range(5):
        for k, fn in fns.items():
            ms[k].append(fn())
    return {k: {"ms_min": min(v), "ms_median": statistics.median(v), "ms_all": v} for k, v in ms.items()}


def kernels(api, A, torch, ctx, scene, s, W, H):
    from query_rate import timed
    lp = api.make_light_params(s.num_lights, 3, 0, W, 1, A.LIGHT_SHADOWED)
    rays = api.camera_rays(ctx, s.camera, W, H, 1)
    hits = api.trace_rays(scene, rays).hits
    n = W * H
    scene.prepare_light_power()
    pick, mis = api.make_pick_params(1, 0), api.make_mis_params(1, s.num_lights, 3)
    sl, w = api.pick_slots_power(scene, n, lp, pick)
    occ = torch.zeros(2 * n, dtype=torch.uint8, device=rays.device)
    stages = {"pick_slots_power_P1": lambda: api.pick_slots_power(scene, n, lp, pick, asynchronous=True),
              "mis_pick_weights_power_P1": lambda: api.mis_pick_weights_power(scene, rays, hits, lp, pick, mis, sl, asynchronous=True),
              "shade_hits_picked_P1": lambda: api.shade_hits_picked(scene, rays, hits, lp, pick, sl, occ, weights=w, asynchronous=True)}
    for m in CANDIDATES:
        plain, weighted = api.make_ris_params(m), api.make_ris_params(m, True, mis.lobes)
        stages[f"pick_slots_ris_M{m}"] = lambda r=plain: api.pick_slots_ris(scene, rays, hits, lp, pick, r, asynchronous=True)
        stages[f"pick_slots_ris_mis_M{m}"] = lambda r=weighted: api.pick_slots_ris(scene, rays, hits, lp, pick, r, asynchronous=True)
    torch.cuda.synchronize()
    return {"kernels": five_each({k: (lambda fn=fn: timed(fn)[0]) for k, fn in stages.items()})}


def loop_walls(root, which, W, H):
    """the path-trace cases of one side, five interleaved repeats -> dict; which: "parent" (path_trace_power of the package under root
    alone) or "this" (path_trace_power and path_trace_ris)"""
    sys.path.insert(0, root)             # the package of that checkout, and nothing of this one
    import torch
    from realtimeraytracer_amd import _abi as A
    from realtimeraytracer_amd import api, scenes
    torch.cuda.init()
    ctx = api.Context(0)
    s = scenes.sponza_class(W, H)
    scene = api.Scene(ctx, s.desc)
    rays = api.camera_rays(ctx, s.camera, W, H, 1)
    lp = api.make_light_params(s.num_lights, 3, 0, W, 1, A.LIGHT_SHADOWED)

    def wall(fn):
        def run():
            torch.cuda.synchronize()
            t = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            return (time.perf_counter() - t) * 1e3
        return run
    cases = {}
    for bounces in (1, 2):
        cases[f"path_trace_power_{bounces}"] = wall(lambda bounces=bounces: api.path_trace_power(scene, rays, lp, bounces, sky_samples=0, light_picks=1))
        if which == "this":
            cases[f"path_trace_ris_M4_{bounces}"] = wall(lambda bounces=bounces: api.path_trace_ris(scene, rays, lp, bounces, sky_samples=0, light_picks=1))
    for fn in cases.values():
        fn()                             # warm-up: every shape once
    out = {"wall_ms": five_each(cases), "package_is_under_root": os.path.abspath(api.__file__).startswith(os.path.abspath(root) + os.sep)}
    scene.close()
    ctx.close()
    return out


def child(root, which, W, H):
    cmd = [sys.executable, os.path.abspath(__file__), "--role", which, "--root", root, "--width", str(W), "--height", str(H)]
    text = subprocess.run(cmd, check=True, stdout=subprocess.PIPE, timeout=300).stdout.decode()
    return json.loads(text.strip().splitlines()[-1])


def variance(api, A, torch, scenes, ctx, frames):
    """mean, median, 99.9th percentile and maximum of the per-pixel variance (the mean is a few pixels': profiles/light_power_rate.py)"""
    W, H = 640, 360
    s = scenes.sponza_class(W, H)
    scene = api.Scene(ctx, s.desc)
    rays = api.camera_rays(ctx, s.camera, W, H, 1)
    n = W * H
    runs = {"power": lambda lp: api.path_trace_power(scene, rays, lp, 1, sky_samples=0, light_picks=1, pick_from=0),
            "ris_M4": lambda lp: api.path_trace_ris(scene, rays, lp, 1, sky_samples=0, light_picks=1, pick_from=0, ris_candidates=4),
            "ris_M16": lambda lp: api.path_trace_ris(scene, rays, lp, 1, sky_samples=0, light_picks=1, pick_from=0, ris_candidates=16)}
    acc = {k: [torch.zeros(n, dtype=torch.float64, device=rays.device) for _ in range(2)] for k in runs}
    sums = {k: [] for k in runs}
    for f in range(frames):
        lp = api.make_light_params(s.num_lights, 3, f, W, 1, A.LIGHT_SHADOWED)
        for k, fn in runs.items():
            x = fn(lp).radiance.double().sum(1)
            acc[k][0] += x
            acc[k][1] += x * x
            sums[k].append(float(x.sum()))
    var = {k: ((acc[k][1] - acc[k][0] ** 2 / frames) / (frames - 1)).float() for k in runs}
    stats = {k: {"mean": float(v.double().mean()), "median": float(v.median()), "p99_9": float(torch.quantile(v[::3], 0.999)), "max": float(v.max())}
             for k, v in var.items()}
    t = {k: torch.tensor(v, dtype=torch.float64) for k, v in sums.items()}
    out = {"scene": "sponza_class", "width": W, "height": H, "bounces": 1, "pick_from": 0, "frames": frames,
           "table_weights": [int(w) for w in scene.export_light_power()[0]], "pixel_variance_radiance": stats,
           "ris_over_power": {k: {q: stats[k][q] / stats["power"][q] for q in ("mean", "median", "p99_9")} for k in ("ris_M4", "ris_M16")},
           "image_sum_mean": {k: float(v.mean()) for k, v in t.items()}, "image_sum_se": {k: float(v.std() / frames ** 0.5) for k, v in t.items()}}
    scene.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--frames", type=int, default=32)
    ap.add_argument("--parent-root", default=None, help="a checkout of the parent commit with its library built; without it the parent's side is left out")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ris", "ris_rate_1080p.json"))
    ap.add_argument("--role", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--root", default=ROOT, help=argparse.SUPPRESS)
    args = ap.parse_args()
    W, H = args.width, args.height
    if args.role:                        # a child: one side's loops, JSON on the last line
        print(json.dumps(loop_walls(args.root, args.role, W, H)))
        return
    loops = {}
    if args.parent_root:                 # before this process opens the device: one process on the GPU at a time
        loops["parent_first"] = child(args.parent_root, "parent", W, H)
    loops["this"] = child(ROOT, "this", W, H)
    if args.parent_root:
        loops["parent_second"] = child(args.parent_root, "parent", W, H)
    assert all(side["package_is_under_root"] for side in loops.values()), "a child imported another checkout's package"
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "profiles"))
    import torch
    from realtimeraytracer_amd import _abi as A
    from realtimeraytracer_amd import api, scenes
    torch.cuda.init()
    ctx = api.Context(0)
    stream = torch.cuda.Stream()          # a stream of its own: the default stream's handle (0) would give the context a new stream
    torch.cuda.set_stream(stream)
    ctx.set_stream(stream.cuda_stream)
    s = scenes.sponza_class(W, H)
    out = {"what": "resampled light picks at a path vertex", "scene": "sponza_class", "width": W, "height": H, "spp": 1, "hits": W * H,
           "device": ctx.device_name(), "kernel_revision": A.hip_lib().rtr_kernel_revision().decode(), "loops": loops}
    scene = api.Scene(ctx, s.desc)
    out.update(kernels(api, A, torch, ctx, scene, s, W, H))
    scene.close()
    torch.cuda.empty_cache()
    out["variance_at_1_bounce"] = variance(api, A, torch, scenes, ctx, args.frames)
    ctx.set_stream(None)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(json.dumps(out, indent=1) + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
