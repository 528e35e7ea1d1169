"""Sky importance sampling (rtr_sky_rays, rtr_shade_sky, rtr_sky_hits) on sponza_class at 1920x1080, 1 spp — the bench frame's 2 073 600
camera hits — against its neighbours: one JSON object, printed and written to profiles/sky/sky_rate_1080p.json.

  kernels      rtr_sky_rays at S = 1 and 2, rtr_shade_sky (S = 1) and rtr_sky_hits (on the camera hits' bounce rays) against
               rtr_light_rays_picked (P = 1) and rtr_bounce_rays on the same hits, and the bytes each moves per hit; once with the
               scene's own sky (constant: the 32 x 16 table) and once with a synthetic 2048 x 1024 HDRI that has a small bright patch, so
               that the row and the column search are real
  table        the wall time of rtr_scene_prepare_sky for both skies (a fresh scene each; the build runs once per scene)
  variance     the textured room (its HDRI has a bright patch) at 640x360, 2 bounces, frames 0 ... N - 1: the mean per-pixel variance
               of radiance for api.path_trace_mis and api.path_trace_sky (S = 1, with and without the heuristic), and their wall time

  --lib PATH --label KEY: load another build of librtr_hip.so (`make -C realtimeraytracer_amd/csrc sky_global_variant`: k_sky_rays
  searching the marginal sums in global memory instead of LDS) and merge this run's kernel figures into the JSON under variants[KEY]; the
  rest of the file is kept.  DESIGN.md section 3 compares the two.

The kernels are enqueued through the Python wrappers in their asynchronous forms (outputs from torch's caching allocator, no join), HIP
events on the context's stream, which is torch's current stream; three warm-up calls, then at least 0.2 s of timed calls per repeat.  The
five repeats of the cases are interleaved, so that a drift of the clock is in all of them alike, and the minimum is reported beside the
median and all five.

    python profiles/sky_rate.py [--width 1920 --height 1080] [--frames 32] [--out profiles/sky/sky_rate_1080p.json] [--lib PATH --label KEY]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "profiles"))
from bounce_rate import five_each  # noqa: E402
from query_rate import timed  # noqa: E402
from realtimeraytracer_amd import _abi as A  # noqa: E402


def synthetic_hdri(width=2048, height=1024):
    """RGBA8: a dim gradient with a 24 x 16 texel patch at full brightness in the upper hemisphere"""
    yy, xx = np.mgrid[0:height, 0:width]
    px = np.zeros((height, width, 4), np.uint8)
    px[..., 0], px[..., 1], px[..., 2], px[..., 3] = 20 + (xx * 40) // width, 30 + (yy * 40) // height, 60, 255
    px[700:716, 500:524, 0:3] = 255
    return px


def kernels(api, ctx, scene, s, W, H):
    n = W * H
    lp = api.make_light_params(s.num_lights, 3, 0, W, 1, A.LIGHT_SHADOWED)
    rays = api.camera_rays(ctx, s.camera, W, H, 1)
    hits = api.trace_rays(scene, rays).hits
    surf = api.hit_surfaces(scene, rays, hits)
    pick = api.make_pick_params(1, 0)
    bp = api.make_bounce_params(frame=0, depth=0, width=W, spp=1)
    b = api.bounce_rays(ctx, rays, surf, bp)
    bhits = api.trace_rays(scene, b.rays).hits
    sky1, sky2 = api.make_sky_params(samples=1, width=W, spp=1), api.make_sky_params(samples=2, width=W, spp=1)
    scene.prepare_sky()
    k1 = api.sky_rays(scene, rays, surf, sky1)
    occ = api.trace_rays(scene, k1.rays.reshape(-1, 8), any_hit=True).occluded
    esc = api.sky_hits(scene, b.rays, bhits, surf, b, sky1)
    torch.cuda.synchronize()
    out = {"live_sample_share": float((k1.rays[:, 0, 7] != 0).float().mean()), "unoccluded_share_of_live": float(((occ == 0) & (k1.rays[:, 0, 7] != 0)).float().sum() / max(float((k1.rays[:, 0, 7] != 0).sum()), 1.0)),
           "bounce_rays_that_miss_share": float((bhits[:, 3] == -1).float().mean()), "mean_w_bounce_at_a_miss": float(esc.w_bounce[bhits[:, 3] == -1].mean()) if bool((bhits[:, 3] == -1).any()) else None}
    stages = {"sky_rays_S1": lambda: api.sky_rays(scene, rays, surf, sky1, asynchronous=True),
              "sky_rays_S2": lambda: api.sky_rays(scene, rays, surf, sky2, asynchronous=True),
              "shade_sky_S1": lambda: api.shade_sky(ctx, k1.raw, occ, asynchronous=True),
              "sky_hits": lambda: api.sky_hits(scene, b.rays, bhits, surf, b, sky1, asynchronous=True),
              "light_rays_picked_P1": lambda: api.light_rays_picked(scene, rays, hits, lp, pick, asynchronous=True),
              "bounce_rays": lambda: api.bounce_rays(ctx, rays, surf, bp, asynchronous=True)}
    # bytes of the per-hit records a lane moves (the tables, gathered, are beside them): origin 16 + surface 64 in, 64 S out; 32 S + S in,
    # 16 out; hit 16 (+ direction 16 + surface 16 + bounce 16 at a miss) in, 32 out; ray 32 + hit 32 in, 64 + 8 out (P = 1 and the
    # directional light); 112 in + 64 out
    out["bytes_per_hit"] = {"sky_rays_S1": 144, "sky_rays_S2": 208, "shade_sky_S1": 49, "sky_hits": 96, "light_rays_picked_P1": 200, "bounce_rays": 176}
    st = out["kernels"] = five_each({k: (lambda fn=fn: timed(fn)[0]) for k, fn in stages.items()})
    out["kernel_tb_per_s"] = {k: out["bytes_per_hit"][k] * n / (st[k]["ms_min"] * 1e-3) / 1e12 for k in stages}
    return out


def with_hdri(desc, px):
    tex = A.rtr_texture(px.ctypes.data_as(C.POINTER(C.c_uint8)), px.shape[1], px.shape[0], 4, 0)
    d = A.rtr_scene_desc.from_buffer_copy(desc)
    d.hdri = C.pointer(tex)
    d._keep = (tex, px)
    return d


def prepare_ms(api, ctx, desc):
    ms = []
    for _ in range(3):
        sc = api.Scene(ctx, desc)
        torch.cuda.synchronize()
        t = time.perf_counter()
        sc.prepare_sky()
        ms.append((time.perf_counter() - t) * 1e3)
        sc.close()
    return {"ms_min": min(ms), "ms_all": ms}


def variance(api, scenes, ctx, frames):
    W, H = 640, 360
    s = scenes.textured_room(W, H)
    scene = api.Scene(ctx, s.desc)
    rays = api.camera_rays(ctx, s.camera, W, H, 1)
    n = W * H
    loops = {"mis": lambda lp: api.path_trace_mis(scene, rays, lp, 2, light_picks=1),
             "sky_S1": lambda lp: api.path_trace_sky(scene, rays, lp, 2, sky_samples=1, light_picks=1),
             "sky_S1_without_the_heuristic": lambda lp: api.path_trace_sky(scene, rays, lp, 2, sky_samples=1, sky_mis=False, light_picks=1)}
    acc = {k: [torch.zeros(n, dtype=torch.float64, device=rays.device) for _ in range(2)] for k in loops}
    sums = {k: [] for k in loops}
    for f in range(frames):
        lp = api.make_light_params(s.num_lights, 3, f, W, 1, A.LIGHT_SHADOWED)
        for k, fn in loops.items():
            x = fn(lp).radiance.double().sum(1)
            acc[k][0] += x
            acc[k][1] += x * x
            sums[k].append(float(x.sum()))
    var = {k: float(((acc[k][1] - acc[k][0] ** 2 / frames) / (frames - 1)).mean()) for k in loops}
    lp = api.make_light_params(s.num_lights, 3, 0, W, 1, A.LIGHT_SHADOWED)

    def wall(fn):
        def run():
            torch.cuda.synchronize()
            t = time.perf_counter()
            fn(lp)
            torch.cuda.synchronize()
            return (time.perf_counter() - t) * 1e3
        return run

    t = {k: torch.tensor(v, dtype=torch.float64) for k, v in sums.items()}
    out = {"scene": "textured_room", "width": W, "height": H, "bounces": 2, "frames": frames, "mean_pixel_variance_radiance": var,
           "sky_S1_over_mis": var["sky_S1"] / var["mis"], "image_sum_mean": {k: float(v.mean()) for k, v in t.items()},
           "image_sum_se": {k: float(v.std() / frames ** 0.5) for k, v in t.items()}, "wall_ms": five_each({k: wall(fn) for k, fn in loops.items()})}
    scene.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--frames", type=int, default=32)
    ap.add_argument("--lib", default=None, help="another build of librtr_hip.so to measure the kernels of")
    ap.add_argument("--label", default=None, help="with --lib: the key of this run under variants")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sky", "sky_rate_1080p.json"))
    args = ap.parse_args()
    if args.lib:
        A.LIB_HIP_PATH = os.path.abspath(args.lib)
    from realtimeraytracer_amd import api, scenes
    W, H = args.width, args.height
    torch.cuda.init()
    ctx = api.Context(0)
    stream = torch.cuda.Stream()          # a stream of its own: the default stream's handle (0) would give the context a new stream
    torch.cuda.set_stream(stream)
    ctx.set_stream(stream.cuda_stream)
    s = scenes.sponza_class(W, H)
    out = {"what": "sky importance sampling at a path vertex", "scene": "sponza_class", "width": W, "height": H, "spp": 1, "hits": W * H,
           "device": ctx.device_name(), "kernel_revision": A.hip_lib().rtr_kernel_revision().decode()}
    skies = {"own_sky_constant_32x16": s.desc, "synthetic_hdri_2048x1024": with_hdri(s.desc, synthetic_hdri())}
    runs = {}
    for name, desc in skies.items():
        scene = api.Scene(ctx, desc)
        runs[name] = kernels(api, ctx, scene, s, W, H)
        scene.close()
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    if args.lib:
        merged = json.load(open(args.out)) if os.path.exists(args.out) else out
        merged.setdefault("variants", {})[args.label or os.path.basename(args.lib)] = {"lib": os.path.basename(args.lib), "skies": runs}
        out = merged
    else:
        out["marginal_sums"] = "LDS up to 4096 rows"
        out["skies"] = runs
        out["prepare_sky_wall"] = {name: prepare_ms(api, ctx, desc) for name, desc in skies.items()}
        out["variance_at_2_bounces"] = variance(api, scenes, ctx, args.frames)
    ctx.set_stream(None)
    with open(args.out, "w") as f:
        f.write(json.dumps(out, indent=1) + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
