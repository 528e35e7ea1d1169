"""Power-proportional light picks (rtr_pick_slots_power and the power forms of the MIS kernels) on sponza_class at 1920x1080, 1 spp —
the bench frame's 2 073 600 camera hits — against their uniform neighbours: one JSON object, printed and written to
profiles/light_power/light_power_rate_1080p.json.

  table        the wall time of rtr_scene_prepare_light_power (a fresh scene each: allocation, two launches, one join), and the two
               launches of the build alone, enqueued behind an rtr_scene_update_lights (the wall time of that call with and without a
               table)
  kernels      rtr_pick_slots_power at P = 1 and 2 against rtr_light_rays_picked drawing its own slots and taking them handed in (the
               difference of those two is the uniform draw's share of that kernel), rtr_mis_pick_weights_power against
               rtr_mis_pick_weights and rtr_emitter_hits_power against rtr_emitter_hits on the same hits
  loops        api.path_trace_power against api.path_trace_mis, 1 and 2 bounces, wall time of a frame
  variance     the same scene at 640x360, 1 bounce, pick_from=0, frames 0 ... N - 1, with its own lights (8.4 : 1 in power as they stand)
               and with their intensities spread further (light l times 10^(1 - l mod 3): rtr_scene_update_lights): the per-pixel
               variance of radiance — mean, median, 99.9th percentile, maximum — for power picks (path_trace_power, sky_samples=0)
               against uniform picks (path_trace_mis), and the image sums with their standard errors

The kernels are enqueued through the Python wrappers in their asynchronous forms, HIP events on the context's stream, which is torch's
current stream; three warm-up calls, then at least 0.2 s of timed calls per repeat.  The five repeats of the cases are interleaved, and
the minimum is reported beside the median and all five.

    python profiles/light_power_rate.py [--width 1920 --height 1080] [--frames 32] [--out profiles/light_power/light_power_rate_1080p.json]
"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "profiles"))
from bounce_rate import five_each  # noqa: E402
from query_rate import timed  # noqa: E402
from realtimeraytracer_amd import _abi as A  # noqa: E402


def wall_ms(fn, repeats=5):
    ms = []
    for _ in range(repeats):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t) * 1e3)
    return {"ms_min": min(ms), "ms_all": ms}


def table(api, ctx, s):
    lights = [s.desc.lights[i] for i in range(s.num_lights)]
    prepare = []
    for _ in range(3):
        sc = api.Scene(ctx, s.desc)
        torch.cuda.synchronize()
        t = time.perf_counter()
        sc.prepare_light_power()
        prepare.append((time.perf_counter() - t) * 1e3)
        sc.close()
    plain, tabled = api.Scene(ctx, s.desc), api.Scene(ctx, s.desc)
    tabled.prepare_light_power()
    out = {"light_triangles": int(tabled.export_light_power()[0].size), "prepare_wall": {"ms_min": min(prepare), "ms_all": prepare},
           "update_lights_wall_without_a_table": wall_ms(lambda: plain.update_lights(lights)),
           "update_lights_wall_with_a_table": wall_ms(lambda: tabled.update_lights(lights))}
    plain.close()
    tabled.close()
    return out


def kernels(api, ctx, scene, s, W, H):
    n = W * H
    lp = api.make_light_params(s.num_lights, 3, 0, W, 1, A.LIGHT_SHADOWED)
    rays = api.camera_rays(ctx, s.camera, W, H, 1)
    hits = api.trace_rays(scene, rays).hits
    surf = api.hit_surfaces(scene, rays, hits)
    b = api.bounce_rays(ctx, rays, surf, api.make_bounce_params(frame=0, depth=0, width=W, spp=1))
    bhits = api.trace_rays(scene, b.rays).hits
    scene.prepare_light_power()
    stages = {}
    for P in (1, 2):
        pick, mis = api.make_pick_params(P, 0), api.make_mis_params(P, s.num_lights, 3)
        sl, _ = api.pick_slots_power(scene, n, lp, pick)
        stages.update({
            f"pick_slots_power_P{P}": lambda pick=pick: api.pick_slots_power(scene, n, lp, pick, asynchronous=True),
            f"light_rays_picked_P{P}_own_draw": lambda pick=pick: api.light_rays_picked(scene, rays, hits, lp, pick, asynchronous=True),
            f"light_rays_picked_P{P}_slots_handed_in": lambda pick=pick, sl=sl: api.light_rays_picked(scene, rays, hits, lp, pick, slots=sl, asynchronous=True),
            f"mis_pick_weights_P{P}": lambda pick=pick, mis=mis, sl=sl: api.mis_pick_weights(scene, rays, hits, lp, pick, mis, sl, asynchronous=True),
            f"mis_pick_weights_power_P{P}": lambda pick=pick, mis=mis, sl=sl: api.mis_pick_weights_power(scene, rays, hits, lp, pick, mis, sl, asynchronous=True),
            f"emitter_hits_P{P}": lambda mis=mis: api.emitter_hits(scene, b.rays, bhits, surf, b, mis, asynchronous=True),
            f"emitter_hits_power_P{P}": lambda mis=mis: api.emitter_hits_power(scene, b.rays, bhits, surf, b, mis, asynchronous=True)})
    torch.cuda.synchronize()
    return {"bounce_rays_on_a_light_share": float((bhits[:, 3] >= 0).logical_and(bhits[:, 3] < s.num_lights).float().mean()),
            "kernels": five_each({k: (lambda fn=fn: timed(fn)[0]) for k, fn in stages.items()})}


def loops(api, ctx, scene, s, W, H):
    rays = api.camera_rays(ctx, s.camera, W, H, 1)
    lp = api.make_light_params(s.num_lights, 3, 0, W, 1, A.LIGHT_SHADOWED)
    runs = {}
    for bounces in (1, 2):
        runs[f"path_trace_mis_{bounces}"] = lambda bounces=bounces: api.path_trace_mis(scene, rays, lp, bounces, light_picks=1)
        runs[f"path_trace_power_{bounces}"] = lambda bounces=bounces: api.path_trace_power(scene, rays, lp, bounces, sky_samples=0, light_picks=1)

    def wall(fn):
        def run():
            torch.cuda.synchronize()
            t = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            return (time.perf_counter() - t) * 1e3
        return run
    return {"wall_ms": five_each({k: wall(fn) for k, fn in runs.items()})}


def variance(api, scenes, ctx, frames):
    """own lights (sponza_class's two lights are 8.4 : 1 in power as they stand) and the variant; mean, median, 99.9th percentile and
    maximum of the per-pixel variance: the last vertex of a path has no bounce behind it and keeps plain next-event estimation, whose
    1 / d^2 near a light gives the per-pixel variance a heavy tail, so the mean is a few pixels' and the percentiles are the body's"""
    W, H = 640, 360
    s = scenes.sponza_class(W, H)
    scene = api.Scene(ctx, s.desc)
    rays = api.camera_rays(ctx, s.camera, W, H, 1)
    n = W * H
    runs = {"uniform": lambda lp: api.path_trace_mis(scene, rays, lp, 1, light_picks=1, pick_from=0),
            "power": lambda lp: api.path_trace_power(scene, rays, lp, 1, sky_samples=0, light_picks=1, pick_from=0)}
    out = {"scene": "sponza_class", "width": W, "height": H, "bounces": 1, "pick_from": 0, "frames": frames, "lights": {}}
    for name in ("own", "light l's intensity times 10^(1 - l mod 3)"):
        lights = [A.RtrAreaLightInfo.from_buffer_copy(s.desc.lights[i]) for i in range(s.num_lights)]
        if name != "own":
            for l, li in enumerate(lights):
                li.intensity = float(li.intensity) * 10.0 ** (1 - l % 3)
            scene.update_lights(lights)
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
        out["lights"][name] = {"table_weights": [int(w) for w in scene.export_light_power()[0]], "pixel_variance_radiance": stats,
                               "power_over_uniform": {q: stats["power"][q] / stats["uniform"][q] for q in ("mean", "median", "p99_9")},
                               "image_sum_mean": {k: float(v.mean()) for k, v in t.items()},
                               "image_sum_se": {k: float(v.std() / frames ** 0.5) for k, v in t.items()}}
    scene.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--frames", type=int, default=32)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "light_power", "light_power_rate_1080p.json"))
    args = ap.parse_args()
    from realtimeraytracer_amd import api, scenes
    W, H = args.width, args.height
    torch.cuda.init()
    ctx = api.Context(0)
    stream = torch.cuda.Stream()          # a stream of its own: the default stream's handle (0) would give the context a new stream
    torch.cuda.set_stream(stream)
    ctx.set_stream(stream.cuda_stream)
    s = scenes.sponza_class(W, H)
    out = {"what": "power-proportional light picks at a path vertex", "scene": "sponza_class", "width": W, "height": H, "spp": 1, "hits": W * H,
           "device": ctx.device_name(), "kernel_revision": A.hip_lib().rtr_kernel_revision().decode(), "cdf": "global memory"}
    out["table"] = table(api, ctx, s)
    scene = api.Scene(ctx, s.desc)
    out.update(kernels(api, ctx, scene, s, W, H))
    out["loops"] = loops(api, ctx, scene, s, W, H)
    scene.close()
    torch.cuda.empty_cache()
    out["variance_at_1_bounce"] = variance(api, scenes, ctx, args.frames)
    ctx.set_stream(None)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(json.dumps(out, indent=1) + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
