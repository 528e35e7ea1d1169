"""Path-compaction rates (rtr_compact_paths) on sponza_class at 1920x1080, 1 spp — the bench frame's 2 073 600 camera hits — and what
compaction and Russian roulette do to api.path_trace: one JSON object, printed and written to profiles/compact/compact_rate_1080p.json.

  compact_paths  the three kernels on the depth-0 bounce output of the frame: the continuation rays and the RtrBounce records as they
                 are (throughput stride 32), seeds and ids; about 150 B per path
  bounce_rays    k_bounce_rays on the same hits, for scale
  path_trace     api.path_trace at 1 and 2 bounces with compact=False — the parent's loop unchanged, the baseline — against
                 compact=True, and with roulette_from=1; wall time of the whole composed call, joined; the live counts per depth

The kernels are enqueued through the C ABI directly on preallocated outputs (the timing is of the kernels, not of Python), HIP events on
the context's stream, which is torch's current stream; three warm-up launches, then at least 0.2 s of timed launches per repeat.  The
five repeats of the cases are interleaved, so that a drift of the clock is in all of them alike, and the minimum is reported beside the
median and all five.  path_trace is timed with a host clock around the call and a device join, five interleaved repeats.

    python profiles/compact_rate.py [--width 1920 --height 1080] [--out profiles/compact/compact_rate_1080p.json]
"""
import argparse
import ctypes as C
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
from realtimeraytracer_amd import api, scenes  # noqa: E402

COMPACT_BYTES_IN = 32 + 12 + 4 + 4           # read by k_compact_count (ray, throughput, seed) and again by a survivor, plus its id
COMPACT_BYTES_OUT = 32 + 12 + 4 + 4          # every output slot is written once


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "compact", "compact_rate_1080p.json"))
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
    out = {"what": "path-compaction rates", "scene": "sponza_class", "width": W, "height": H, "spp": 1, "paths": n,
           "device": ctx.device_name(), "kernel_revision": A.hip_lib().rtr_kernel_revision().decode()}

    rays = api.camera_rays(ctx, s.camera, W, H, 1)
    hits = api.trace_rays(scene, rays).hits
    surf = api.hit_surfaces(scene, rays, hits).raw
    lp = api.make_light_params(s.num_lights, 3, 0, W, 1, A.LIGHT_SHADOWED)
    bp = api.make_bounce_params(frame=0, depth=0, width=W, spp=1)
    b = api.bounce_rays(ctx, rays, surf, bp)
    k = torch.arange(n, device=rays.device, dtype=torch.int64)
    seeds = api._wrap32((k % W) * 733 + (k // W) * 1933)
    ids = torch.arange(n, device=rays.device, dtype=torch.int32)
    nbytes = api.compact_scratch_bytes(lib, n)
    scratch = torch.empty(nbytes, dtype=torch.uint8, device=rays.device)
    o_rays = torch.empty((n, 8), dtype=torch.float32, device=rays.device)
    o_t = torch.empty((n, 3), dtype=torch.float32, device=rays.device)
    o_seeds, o_ids = torch.empty_like(seeds), torch.empty_like(ids)
    count = torch.zeros(1, dtype=torch.int32, device=rays.device)
    out_rays2, out_b2 = torch.empty_like(b.rays), torch.empty_like(b.raw)
    torch.cuda.synchronize()

    def compact(roulette):
        p = api.make_compact_params(frame=0, depth=0, roulette=roulette, survival_floor=0.05, throughput_stride=32)

        def run():
            return lib.rtr_compact_paths_async(ctx.h, A.VP(b.rays.data_ptr()), A.VP(b.raw.data_ptr()), A.VP(seeds.data_ptr()), A.VP(ids.data_ptr()), n, C.byref(p),
                                               A.VP(scratch.data_ptr()), nbytes, A.VP(o_rays.data_ptr()), A.VP(o_t.data_ptr()), A.VP(o_seeds.data_ptr()),
                                               A.VP(o_ids.data_ptr()), A.VP(count.data_ptr()))
        return run

    def bounce():
        return lib.rtr_bounce_rays_async(ctx.h, A.VP(rays.data_ptr()), A.VP(surf.data_ptr()), n, C.byref(bp), None, A.VP(out_rays2.data_ptr()), A.VP(out_b2.data_ptr()))

    survivors = {}
    for name, fn in (("plain", compact(False)), ("roulette", compact(True))):
        assert fn() == 0, lib.rtr_last_error()
        torch.cuda.synchronize()
        survivors[name] = int(count.item())
    assert bounce() == 0, lib.rtr_last_error()
    out["survivors_of_the_depth_0_bounce"] = survivors
    out["scratch_bytes"] = nbytes

    kern = five_each({"compact_paths": lambda: timed(compact(False))[0], "compact_paths_roulette": lambda: timed(compact(True))[0],
                      "bounce_rays": lambda: timed(bounce)[0]})
    for name, v in kern.items():
        v["mpaths_s"] = n / v["ms_min"] / 1e3
    for name, live in (("compact_paths", survivors["plain"]), ("compact_paths_roulette", survivors["roulette"])):
        moved = n * (COMPACT_BYTES_IN + COMPACT_BYTES_OUT) + live * COMPACT_BYTES_IN
        kern[name]["bytes_per_path"] = moved / n
        kern[name]["gb_s"] = moved / kern[name]["ms_min"] / 1e6
    out["kernels"] = kern
    out["compact_over_bounce_rays"] = kern["compact_paths"]["ms_min"] / kern["bounce_rays"]["ms_min"]

    live_counts = {}

    def path(bounces, **kw):
        def run():
            torch.cuda.synchronize()
            t = time.perf_counter()
            res = api.path_trace(scene, rays, lp, bounces, **kw)
            torch.cuda.synchronize()
            if res.live is not None:
                live_counts[f"bounces_{bounces}" + ("_roulette" if kw.get("roulette_from") is not None else "")] = res.live
            return (time.perf_counter() - t) * 1e3
        return run

    cases = {}
    for bounces in (1, 2):
        cases[f"bounces_{bounces}_plain"] = path(bounces)
        cases[f"bounces_{bounces}_compact"] = path(bounces, compact=True)
        cases[f"bounces_{bounces}_compact_roulette_from_1"] = path(bounces, compact=True, roulette_from=1)
    cases["bounces_4_plain"] = path(4)
    cases["bounces_4_compact"] = path(4, compact=True)
    cases["bounces_4_compact_roulette_from_1"] = path(4, compact=True, roulette_from=1)
    for fn in cases.values():
        fn()                                                                      # warm-up: every shape once
    out["path_trace_wall"] = five_each(cases)
    out["path_trace_live"] = live_counts
    w = out["path_trace_wall"]
    out["compact_over_plain"] = {f"bounces_{bn}": w[f"bounces_{bn}_compact"]["ms_min"] / w[f"bounces_{bn}_plain"]["ms_min"] for bn in (1, 2, 4)}
    out["roulette_over_plain"] = {f"bounces_{bn}": w[f"bounces_{bn}_compact_roulette_from_1"]["ms_min"] / w[f"bounces_{bn}_plain"]["ms_min"] for bn in (1, 2, 4)}
    ctx.set_stream(None)
    text = json.dumps(out, indent=1)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
