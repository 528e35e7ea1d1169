"""Picked light samples (rtr_light_rays_picked, rtr_shade_hits_picked) on sponza_class at 1920x1080, 1 spp — the bench frame's 2 073 600
camera hits, Q = 13 — against the full light loops: one JSON object, printed and written to profiles/light_pick/light_pick_rate_1080p.json.

  vertex       light rays, occlusion and shade of one path vertex: the full loops (Q rays per hit) against P = 1 and P = 2 picks (P + 1
               rays per hit), the occlusion through the dense route (trace_rays, any hit) and the queued route (trace_occlusion)
  path_trace   api.path_trace at 1, 2 and 4 bounces against api.path_trace_picked with light_picks=1, and with compact=True, roulette_from=1 too; wall
               time of the whole composed call, joined
  variance     the per-pixel variance of per_depth[1] (the sum of its channels) over frames 0 ... 63 at 1 bounce, one pick over the full
               loops: the mean over the pixels of each, and their ratio; and the image sums' means, as tests/test_gpu_light_pick.py has them

The stages are enqueued through the Python wrappers in their asynchronous forms (outputs from torch's caching allocator, no join), HIP
events on the context's stream, which is torch's current stream; three warm-up calls, then at least 0.2 s of timed calls per repeat.
The five repeats of the cases are interleaved, so that a drift of the clock is in all of them alike, and the minimum is reported beside
the median and all five.  path_trace is timed with a host clock around the call and a device join, five interleaved repeats.

    python profiles/light_pick_rate.py [--width 1920 --height 1080] [--frames 64] [--out profiles/light_pick/light_pick_rate_1080p.json]
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
from realtimeraytracer_amd import api, scenes  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "light_pick", "light_pick_rate_1080p.json"))
    args = ap.parse_args()
    W, H = args.width, args.height
    torch.cuda.init()
    ctx = api.Context(0)
    stream = torch.cuda.Stream()          # a stream of its own: the default stream's handle (0) would give the context a new stream
    torch.cuda.set_stream(stream)
    ctx.set_stream(stream.cuda_stream)
    s = scenes.sponza_class(W, H)
    scene = api.Scene(ctx, s.desc)
    n = W * H
    lp = api.make_light_params(s.num_lights, 3, 0, W, 1, A.LIGHT_SHADOWED)
    Q = api.light_slots(scene, lp)
    out = {"what": "picked light samples against the full light loops", "scene": "sponza_class", "width": W, "height": H, "spp": 1, "hits": n,
           "slots_per_hit_full": Q, "device": ctx.device_name(), "kernel_revision": A.hip_lib().rtr_kernel_revision().decode()}

    rays = api.camera_rays(ctx, s.camera, W, H, 1)
    hits = api.trace_rays(scene, rays).hits
    torch.cuda.synchronize()

    # ---- one vertex, stage by stage ----
    full_rays = api.light_rays(scene, rays, hits, lp)
    full_occ = api.trace_rays(scene, full_rays, any_hit=True).occluded
    stages = {"full_light_rays": lambda: api.light_rays(scene, rays, hits, lp, asynchronous=True),
              "full_occlusion_dense": lambda: api.trace_rays(scene, full_rays, any_hit=True, asynchronous=True),
              "full_occlusion_queued": lambda: api.trace_occlusion(scene, full_rays, asynchronous=True),
              "full_shade": lambda: api.shade_hits(scene, rays, hits, lp, full_occ, asynchronous=True)}
    keep = []
    for P in (1, 2):
        pick = api.make_pick_params(P, 1)
        prays, slots = api.light_rays_picked(scene, rays, hits, lp, pick)
        pocc = api.trace_rays(scene, prays, any_hit=True).occluded
        keep.append((pick, prays, slots, pocc))
        stages[f"picks_{P}_light_rays"] = lambda pick=pick: api.light_rays_picked(scene, rays, hits, lp, pick, asynchronous=True)
        stages[f"picks_{P}_occlusion_dense"] = lambda prays=prays: api.trace_rays(scene, prays, any_hit=True, asynchronous=True)
        stages[f"picks_{P}_occlusion_queued"] = lambda prays=prays: api.trace_occlusion(scene, prays, asynchronous=True)
        stages[f"picks_{P}_shade"] = lambda pick=pick, slots=slots, pocc=pocc: api.shade_hits_picked(scene, rays, hits, lp, pick, slots, pocc, asynchronous=True)
        out[f"picks_{P}_rays_sent_share"] = float((prays != 0).any(1).float().mean())
    out["full_rays_sent_share"] = float((full_rays != 0).any(1).float().mean())
    torch.cuda.synchronize()
    st = five_each({k: (lambda fn=fn: timed(fn)[0]) for k, fn in stages.items()})
    out["vertex_stages"] = st
    out["vertex_ms_min"] = {f"{who}_{route}": st[f"{who}_light_rays"]["ms_min"] + st[f"{who}_occlusion_{route}"]["ms_min"] + st[f"{who}_shade"]["ms_min"]
                            for who in ("full", "picks_1", "picks_2") for route in ("dense", "queued")}
    v = out["vertex_ms_min"]
    out["picked_vertex_over_full"] = {f"picks_{P}_{route}": v[f"picks_{P}_{route}"] / v[f"full_{route}"] for P in (1, 2) for route in ("dense", "queued")}
    del full_rays, full_occ, keep, stages
    torch.cuda.empty_cache()

    # ---- path_trace ----
    def path(bounces, **kw):
        def run():
            torch.cuda.synchronize()
            t = time.perf_counter()
            (api.path_trace_picked if "light_picks" in kw else api.path_trace)(scene, rays, lp, bounces, **kw)
            torch.cuda.synchronize()
            return (time.perf_counter() - t) * 1e3
        return run

    cases = {}
    for bounces in (1, 2, 4):
        cases[f"bounces_{bounces}_plain"] = path(bounces)
        cases[f"bounces_{bounces}_light_picks_1"] = path(bounces, light_picks=1)
        cases[f"bounces_{bounces}_light_picks_1_compact_roulette_from_1"] = path(bounces, light_picks=1, compact=True, roulette_from=1)
    for fn in cases.values():
        fn()                                                                      # warm-up: every shape once
    w = out["path_trace_wall"] = five_each(cases)
    out["light_picks_over_plain"] = {f"bounces_{b}": w[f"bounces_{b}_light_picks_1"]["ms_min"] / w[f"bounces_{b}_plain"]["ms_min"] for b in (1, 2, 4)}
    out["light_picks_compact_roulette_over_plain"] = {f"bounces_{b}": w[f"bounces_{b}_light_picks_1_compact_roulette_from_1"]["ms_min"] / w[f"bounces_{b}_plain"]["ms_min"]
                                                      for b in (1, 2, 4)}

    # ---- the variance the picks add to the bounce vertex ----
    acc = {k: [torch.zeros(n, dtype=torch.float64, device=rays.device), torch.zeros(n, dtype=torch.float64, device=rays.device), []] for k in ("full", "picked")}
    for f in range(args.frames):
        lpf = api.make_light_params(s.num_lights, 3, f, W, 1, A.LIGHT_SHADOWED)
        for k, kw in (("full", {}), ("picked", {"light_picks": 1})):
            x = (api.path_trace_picked if kw else api.path_trace)(scene, rays, lpf, 1, **kw).per_depth[1].double().sum(1)
            acc[k][0] += x
            acc[k][1] += x * x
            acc[k][2].append(float(x.sum()))
    F = args.frames
    var = {k: float(((a[1] - a[0] * a[0] / F) / (F - 1)).mean()) for k, a in acc.items()}
    sums = {k: torch.tensor(a[2], dtype=torch.float64) for k, a in acc.items()}
    out["bounce_vertex_variance"] = {"frames": F, "mean_pixel_variance_full": var["full"], "mean_pixel_variance_picked": var["picked"],
                                     "picked_over_full": var["picked"] / var["full"],
                                     "image_sum_mean_full": float(sums["full"].mean()), "image_sum_mean_picked": float(sums["picked"].mean()),
                                     "image_sum_se_full": float(sums["full"].std() / F ** 0.5), "image_sum_se_picked": float(sums["picked"].std() / F ** 0.5)}
    ctx.set_stream(None)
    text = json.dumps(out, indent=1)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
