"""Continuation-ray rates (rtr_bounce_rays) on sponza_class at 1920x1080, 1 spp — the bench frame's 2 073 600 camera hits — and the
cost of api.path_trace: one JSON object, printed and written to profiles/bounce/bounce_rate_1080p.json.

  bounce_rays    k_bounce_rays on the frame's hits: 176 B per hit (32-B ray + 80-B surface in, 32-B ray + 32-B RtrBounce out)
  hit_surfaces   rtr_hit_surfaces on the same hits, and
  light_rays     rtr_light_rays on the same hits (Q rays of 32 B out per hit), for scale
  path_trace     api.path_trace at 0, 1 and 2 bounces: wall time of the whole composed call, joined

The three kernels are enqueued through the C ABI directly on preallocated outputs (the timing is of the kernel, not of Python), HIP
events on the context's stream, which is torch's current stream; three warm-up launches, then at least 0.2 s of timed launches per
repeat.  The five repeats of the cases are interleaved, so that a drift of the clock is in all of them alike, and the minimum is reported
beside the median and all five.  path_trace is timed with a host clock around the call and a device join, five interleaved repeats.

    python profiles/bounce_rate.py [--width 1920 --height 1080] [--out profiles/bounce/bounce_rate_1080p.json]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "profiles"))
from query_rate import timed  # noqa: E402
from realtimeraytracer_amd import _abi as A  # noqa: E402
from realtimeraytracer_amd import api, scenes  # noqa: E402

BOUNCE_BYTES = 32 + 80 + 32 + 32


def five_each(fns):
    """the repeats of several loops interleaved, so that a drift of the clock is in all of them alike"""
    ms = {k: [] for k in fns}
    for _ in range(5):
        for k, fn in fns.items():
            ms[k].append(fn())
    return {k: {"ms_min": min(v), "ms_median": statistics.median(v), "ms_all": v} for k, v in ms.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bounce", "bounce_rate_1080p.json"))
    args = ap.parse_args()
    W, H = args.width, args.height
    torch.cuda.init()
    ctx = api.Context(0)
    stream = torch.cuda.Stream()          # a stream of its own: the default stream's handle (0) would give the context a new stream
    torch.cuda.set_stream(stream)
    ctx.set_stream(stream.cuda_stream)
    s = scenes.sponza_class(W, H)
    scene = api.Scene(ctx, s.desc)
    lib, n = ctx.lib, W * H
    out = {"what": "continuation-ray rates", "scene": "sponza_class", "width": W, "height": H, "spp": 1, "hits": n,
           "device": ctx.device_name(), "kernel_revision": A.hip_lib().rtr_kernel_revision().decode(), "bounce_bytes_per_hit": BOUNCE_BYTES}

    rays = api.camera_rays(ctx, s.camera, W, H, 1)
    hits = api.trace_rays(scene, rays).hits
    surf = api.hit_surfaces(scene, rays, hits).raw
    lp = api.make_light_params(s.num_lights, 3, 0, W, 1, A.LIGHT_SHADOWED)
    bp = api.make_bounce_params(frame=0, depth=0, width=W, spp=1)
    Q = api.light_slots(scene, lp)
    out_rays = torch.empty((n, 8), dtype=torch.float32, device=rays.device)
    out_b = torch.empty((n, 8), dtype=torch.float32, device=rays.device)
    out_surf = torch.empty((n, 20), dtype=torch.float32, device=rays.device)
    out_light = torch.empty((n * Q, 8), dtype=torch.float32, device=rays.device)
    torch.cuda.synchronize()
    rp, hp, sp = A.VP(rays.data_ptr()), A.VP(hits.data_ptr()), A.VP(surf.data_ptr())

    def bounce():
        return lib.rtr_bounce_rays_async(ctx.h, rp, sp, n, C.byref(bp), None, A.VP(out_rays.data_ptr()), A.VP(out_b.data_ptr()))

    def surfaces():
        return lib.rtr_hit_surfaces_async(ctx.h, scene.h, rp, hp, n, A.VP(out_surf.data_ptr()))

    def light():
        return lib.rtr_light_rays_async(ctx.h, scene.h, rp, hp, n, C.byref(lp), None, A.VP(out_light.data_ptr()))

    for fn in (bounce, surfaces, light):
        assert fn() == 0, lib.rtr_last_error()
    torch.cuda.synchronize()
    lobe = out_b.view(torch.int32)[:, 4]
    out["records"] = {"dead": int((lobe == 0).sum()), "diffuse": int((lobe == A.BOUNCE_DIFFUSE).sum()), "specular": int((lobe == A.BOUNCE_SPECULAR).sum())}
    out["light_slots_per_hit"] = Q

    k = five_each({"bounce_rays": lambda: timed(bounce)[0], "hit_surfaces": lambda: timed(surfaces)[0], "light_rays": lambda: timed(light)[0]})
    for name, v in k.items():
        v["mhits_s"] = n / v["ms_min"] / 1e3
    k["bounce_rays"]["gb_s"] = n * BOUNCE_BYTES / k["bounce_rays"]["ms_min"] / 1e6
    k["hit_surfaces"]["stream_gb_s"] = n * (32 + 32 + 80) / k["hit_surfaces"]["ms_min"] / 1e6
    k["light_rays"]["stream_gb_s"] = n * (32 + 32 + 32 * Q) / k["light_rays"]["ms_min"] / 1e6
    out["kernels"] = k
    out["bounce_over_hit_surfaces"] = k["bounce_rays"]["ms_min"] / k["hit_surfaces"]["ms_min"]
    out["bounce_over_light_rays"] = k["bounce_rays"]["ms_min"] / k["light_rays"]["ms_min"]

    def path(bounces):
        def run():
            torch.cuda.synchronize()
            t = time.perf_counter()
            api.path_trace(scene, rays, lp, bounces)
            torch.cuda.synchronize()
            return (time.perf_counter() - t) * 1e3
        return run

    for b in (0, 1, 2):
        path(b)()                                                                 # warm-up: every shape once
    out["path_trace_wall"] = five_each({f"bounces_{b}": path(b) for b in (0, 1, 2)})
    ctx.set_stream(None)
    text = json.dumps(out, indent=1)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
