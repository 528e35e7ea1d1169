"""MIS at a path vertex (rtr_mis_pick_weights, rtr_emitter_hits) on sponza_class at 1920x1080, 1 spp — the bench frame's 2 073 600 camera
hits — against their neighbours: one JSON object, printed and written to profiles/mis/mis_rate_1080p.json.

  kernels      rtr_mis_pick_weights (P = 1, without and with the RtrMisSample records) and rtr_emitter_hits (on the camera hits' bounce
               rays) against rtr_shade_hits_picked (P = 1) and rtr_bounce_rays on the same hits, and the bytes each moves per hit
  path_trace   api.path_trace_picked(light_picks=1) against api.path_trace_mis(light_picks=1) at 1, 2 and 4 bounces, and both with
               pick_from=0; wall time of the whole composed call, joined
  variance     over frames 0 ... 63 at 2 bounces: the mean per-pixel variance of per_depth[1] and of radiance (the sums of their
               channels) for both loops.  Under MIS the lights of vertex 1 are shared between per_depth[1] (its picks, weighted) and
               per_depth[2] (its bounce ray's emitter hit), so radiance is the like-for-like figure.

The kernels are enqueued through the Python wrappers in their asynchronous forms (outputs from torch's caching allocator, no join), HIP
events on the context's stream, which is torch's current stream; three warm-up calls, then at least 0.2 s of timed calls per repeat.  The
five repeats of the cases are interleaved, so that a drift of the clock is in all of them alike, and the minimum is reported beside the
median and all five.  path_trace is timed with a host clock around the call and a device join, five interleaved repeats.

  back_seen    (--back-seen [--label KEY]: this section alone) the share of the hits of vertex 0 and of vertex 1 that are objects seen
               from behind their shading normal (dot(N, V) < 0), the per-frame differences of the image sums picked - full and MIS -
               full (full: api.path_trace) over frames 0 ... 63 at 2 bounces with their standard errors, and the wall time of
               path_trace_mis at 2 bounces.  Merged into the JSON at --out under back_seen[KEY]; the rest of the file is kept.  The
               committed file holds two builds of one session, which DESIGN.md section 3 compares: the one before the rule for views
               from behind the shading normal (--label build_before_the_rule, run against that build's libraries) and the one with it.

    python profiles/mis_rate.py [--width 1920 --height 1080] [--frames 64] [--out profiles/mis/mis_rate_1080p.json] [--back-seen [--label KEY]]
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


def back_seen(ctx, scene, s, rays, W, H, frames):
    def share(r, surf):
        nov = ((r[:, 0:3] - surf.position) * surf.normal).sum(1)
        obj = surf.kind == A.SURFACE_OBJECT
        return float((obj & (nov < 0)).sum()) / max(int(obj.sum()), 1), int(obj.sum())

    hits = api.trace_rays(scene, rays).hits
    surf = api.hit_surfaces(scene, rays, hits)
    b = api.bounce_rays(ctx, rays, surf, api.make_bounce_params(frame=0, depth=0, width=W, spp=1))
    live = (b.rays != 0).any(1)
    r1 = b.rays[live]
    surf1 = api.hit_surfaces(scene, r1, api.trace_rays(scene, r1).hits)
    s0, n0 = share(rays, surf)
    s1, n1 = share(r1, surf1)
    out = {"frames": frames, "vertex_0": {"object_hits": n0, "seen_from_behind_share": s0}, "vertex_1": {"object_hits": n1, "seen_from_behind_share": s1}}
    sums = {"full": [], "picked": [], "mis": []}
    for f in range(frames):
        lpf = api.make_light_params(s.num_lights, 3, f, W, 1, A.LIGHT_SHADOWED)
        sums["full"].append(float(api.path_trace(scene, rays, lpf, 2).radiance.double().sum()))
        sums["picked"].append(float(api.path_trace_picked(scene, rays, lpf, 2, light_picks=1).radiance.double().sum()))
        sums["mis"].append(float(api.path_trace_mis(scene, rays, lpf, 2, light_picks=1).radiance.double().sum()))
    t = {k: torch.tensor(v, dtype=torch.float64) for k, v in sums.items()}
    out["image_sum_mean"] = {k: float(v.mean()) for k, v in t.items()}
    for k in ("picked", "mis"):
        d = t[k] - t["full"]
        out[f"{k}_minus_full"] = {"mean": float(d.mean()), "se": float(d.std() / frames ** 0.5), "relative": float(d.mean() / t["full"].mean())}
    lp = api.make_light_params(s.num_lights, 3, 0, W, 1, A.LIGHT_SHADOWED)

    def run():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        api.path_trace_mis(scene, rays, lp, 2, light_picks=1)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    run()
    out["path_trace_mis_2_bounces_ms"] = five_each({"mis": run})["mis"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--back-seen", action="store_true")
    ap.add_argument("--label", default="build_with_the_rule", help="with --back-seen: the key of this build's figures under back_seen")
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mis", "mis_rate_1080p.json"))
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
    out = {"what": "MIS between picked light samples and the bounce ray", "scene": "sponza_class", "width": W, "height": H, "spp": 1, "hits": n,
           "device": ctx.device_name(), "kernel_revision": A.hip_lib().rtr_kernel_revision().decode()}

    rays = api.camera_rays(ctx, s.camera, W, H, 1)
    if args.back_seen:
        # merged into the file that is there under the build's label: the other sections and the other build's figures stay
        merged = json.load(open(args.out)) if os.path.exists(args.out) else out
        merged.setdefault("back_seen", {})[args.label] = dict(back_seen(ctx, scene, s, rays, W, H, args.frames), kernel_revision=out["kernel_revision"])
        ctx.set_stream(None)
        with open(args.out, "w") as f:
            f.write(json.dumps(merged, indent=1) + "\n")
        print(json.dumps({"back_seen": {args.label: merged["back_seen"][args.label]}}))
        return
    hits = api.trace_rays(scene, rays).hits
    surf = api.hit_surfaces(scene, rays, hits)
    pick, mis = api.make_pick_params(1, 0), api.make_mis_params(1, s.num_lights, 3)
    prays, slots = api.light_rays_picked(scene, rays, hits, lp, pick)
    pocc = api.trace_rays(scene, prays, any_hit=True).occluded
    bp = api.make_bounce_params(frame=0, depth=0, width=W, spp=1)
    b = api.bounce_rays(ctx, rays, surf, bp)
    bhits = api.trace_rays(scene, b.rays).hits
    em = api.emitter_hits(scene, b.rays, bhits, surf, b, mis)
    torch.cuda.synchronize()
    out["bounce_rays_on_a_light_share"] = float((em.kind == A.SURFACE_LIGHT).float().mean())

    # ---- the kernels and their neighbours ----
    stages = {"mis_pick_weights": lambda: api.mis_pick_weights(scene, rays, hits, lp, pick, mis, slots, asynchronous=True),
              "mis_pick_weights_with_samples": lambda: api.mis_pick_weights(scene, rays, hits, lp, pick, mis, slots, samples=True, asynchronous=True),
              "emitter_hits": lambda: api.emitter_hits(scene, b.rays, bhits, surf, b, mis, asynchronous=True),
              "shade_hits_picked": lambda: api.shade_hits_picked(scene, rays, hits, lp, pick, slots, pocc, asynchronous=True),
              "bounce_rays": lambda: api.bounce_rays(ctx, rays, surf, bp, asynchronous=True)}
    # bytes of the per-hit records a lane moves (the scene's tables, gathered, are beside them): ray 32 + hit 32 + slot 4 + weight 4 (+ 32
    # of samples); ray 32 + hit 32 + 32 of the surface + 16 of the bounce + 32 out; ray 32 + hit 32 + slot 4 + 2 bytes + 48 out; 112 in + 64 out
    out["bytes_per_hit"] = {"mis_pick_weights": 72, "mis_pick_weights_with_samples": 104, "emitter_hits": 144, "shade_hits_picked": 118, "bounce_rays": 176}
    st = out["kernels"] = five_each({k: (lambda fn=fn: timed(fn)[0]) for k, fn in stages.items()})
    out["kernel_tb_per_s"] = {k: out["bytes_per_hit"][k] * n / (st[k]["ms_min"] * 1e-3) / 1e12 for k in stages}
    del stages
    torch.cuda.empty_cache()

    # ---- path_trace ----
    def path(fn, bounces, **kw):
        def run():
            torch.cuda.synchronize()
            t = time.perf_counter()
            fn(scene, rays, lp, bounces, light_picks=1, **kw)
            torch.cuda.synchronize()
            return (time.perf_counter() - t) * 1e3
        return run

    cases = {}
    for bounces in (1, 2, 4):
        cases[f"bounces_{bounces}_picked"] = path(api.path_trace_picked, bounces)
        cases[f"bounces_{bounces}_mis"] = path(api.path_trace_mis, bounces)
        cases[f"bounces_{bounces}_picked_pick_from_0"] = path(api.path_trace_picked, bounces, pick_from=0)
        cases[f"bounces_{bounces}_mis_pick_from_0"] = path(api.path_trace_mis, bounces, pick_from=0)
    for fn in cases.values():
        fn()                                                                      # warm-up: every shape once
    w = out["path_trace_wall"] = five_each(cases)
    out["mis_over_picked"] = {f"bounces_{bb}{sfx}": w[f"bounces_{bb}_mis{sfx}"]["ms_min"] / w[f"bounces_{bb}_picked{sfx}"]["ms_min"]
                              for bb in (1, 2, 4) for sfx in ("", "_pick_from_0")}

    # ---- the variance ----
    names = ("picked", "mis")
    acc = {k: {"d1": [torch.zeros(n, dtype=torch.float64, device=rays.device) for _ in range(2)],
               "radiance": [torch.zeros(n, dtype=torch.float64, device=rays.device) for _ in range(2)], "sums": []} for k in names}
    for f in range(args.frames):
        lpf = api.make_light_params(s.num_lights, 3, f, W, 1, A.LIGHT_SHADOWED)
        for k, fn in zip(names, (api.path_trace_picked, api.path_trace_mis)):
            res = fn(scene, rays, lpf, 2, light_picks=1)
            for key, x in (("d1", res.per_depth[1].double().sum(1)), ("radiance", res.radiance.double().sum(1))):
                acc[k][key][0] += x
                acc[k][key][1] += x * x
            acc[k]["sums"].append(float(res.radiance.double().sum()))
    F = args.frames
    var = {k: {key: float(((acc[k][key][1] - acc[k][key][0] ** 2 / F) / (F - 1)).mean()) for key in ("d1", "radiance")} for k in names}
    sums = {k: torch.tensor(acc[k]["sums"], dtype=torch.float64) for k in names}
    out["variance_at_2_bounces"] = {"frames": F, "mean_pixel_variance_per_depth_1": {k: var[k]["d1"] for k in names},
                                    "mean_pixel_variance_radiance": {k: var[k]["radiance"] for k in names},
                                    "mis_over_picked_radiance": var["mis"]["radiance"] / var["picked"]["radiance"],
                                    "image_sum_mean": {k: float(sums[k].mean()) for k in names},
                                    "image_sum_se": {k: float(sums[k].std() / F ** 0.5) for k in names}}
    ctx.set_stream(None)
    text = json.dumps(out, indent=1)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
