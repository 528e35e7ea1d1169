"""Ray-query rates (rtr_trace_rays) on sponza_class at 1920x1080, 1 spp: one JSON line.

  closest_camera   closest hit of the frame's camera rays (rtr_camera_rays_async), next to the render's primaryMs for the same camera with
                   the tunable primary_persist = 0 (k_primary + k_primary_tail: the kernel the query mirrors)
  closest_shuffled the same rays in a seeded random permutation (incoherent waves)
  occlusion        any-hit rays from the camera rays' hit points towards seeded points on the area lights

HIP events on the query's stream (the context is put on torch's current stream and the queries are enqueued asynchronously), three
warm-up launches, then at least 0.2 s of timed launches per case.

    python profiles/query_rate.py [--width 1920 --height 1080]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from realtimeraytracer_amd import _abi as A  # noqa: E402
from realtimeraytracer_amd import api, scenes  # noqa: E402


def timed(fn, min_s=0.2, warmup=3):
    """ms per call of fn (enqueued on torch's current stream), over at least min_s seconds of calls"""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    n = 4
    while True:
        a.record()
        for _ in range(n):
            fn()
        b.record()
        b.synchronize()
        ms = a.elapsed_time(b)
        if ms >= min_s * 1000.0:
            return ms / n, n
        n = max(n * 2, int(n * min_s * 1000.0 / max(ms, 1e-3) * 1.2) + 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--seed", type=int, default=1)
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
    out = {"what": "ray-query rates", "scene": "sponza_class", "width": W, "height": H, "spp": 1, "rays": n,
           "device": ctx.device_name(), "kernel_revision": A.hip_lib().rtr_kernel_revision().decode()}

    # the render's camera-ray kernel for the same camera: k_primary (+ tail), primaryMs by the render's own events
    ctx.set_tunable("primary_persist", 0)
    frame = api.Frame(ctx, W, H)
    p = api.make_params(W, H, spp=1, pipeline=2)
    pms = []
    for i in range(23):
        api.render(scene, s.camera, s.scene_info(0), p, frame)
        if i >= 3:
            pms.append(frame.stats().primaryMs)
    out["render_primary_ms_median"] = float(np.median(pms))

    rays = api.camera_rays(ctx, s.camera, W, H, 1)
    torch.cuda.synchronize()
    ms, reps = timed(lambda: api.trace_rays(scene, rays, asynchronous=True))
    out["closest_camera"] = {"ms": ms, "mrays_s": n / ms / 1e3, "launches": reps}
    out["closest_camera_over_primary_ms"] = ms / out["render_primary_ms_median"]
    out["closest_camera_within_1_25x"] = bool(ms <= 1.25 * out["render_primary_ms_median"])

    g = torch.Generator(device="cpu").manual_seed(args.seed)
    shuffled = rays[torch.randperm(n, generator=g).cuda()].contiguous()
    ms, reps = timed(lambda: api.trace_rays(scene, shuffled, asynchronous=True))
    out["closest_shuffled"] = {"ms": ms, "mrays_s": n / ms / 1e3, "launches": reps}

    # occlusion rays: from each camera ray's hit point (objects only) to a seeded point on a seeded light triangle; the direction is the
    # unnormalised segment, so t in (0.001, 0.999) stays short of both ends
    r = api.trace_rays(scene, rays)
    tris = np.frombuffer(scene.export_bvh()[1], dtype=np.uint32).reshape(-1, 12)
    lt = tris[tris[:, 3] < s.num_lights].view(np.float32)
    ci = r.custom_index.cpu().numpy()
    keep = np.nonzero(ci >= s.num_lights)[0]
    rn = rays.cpu().numpy()[keep]
    hp = rn[:, 0:3] + rn[:, 4:7] * r.t.cpu().numpy()[keep, None]
    rng = np.random.default_rng(args.seed)
    pick = rng.integers(0, len(lt), len(keep))
    b1, b2 = rng.uniform(0, 1, len(keep)), rng.uniform(0, 1, len(keep))
    flip = b1 + b2 > 1
    b1, b2 = np.where(flip, 1 - b1, b1), np.where(flip, 1 - b2, b2)
    lp = lt[pick, 0:3] + lt[pick, 4:7] * b1[:, None] + lt[pick, 8:11] * b2[:, None]
    occ_rays = np.zeros((len(keep), 8), np.float32)
    occ_rays[:, 0:3], occ_rays[:, 3], occ_rays[:, 4:7], occ_rays[:, 7] = hp, 0.001, lp - hp, 0.999
    occ_t = torch.from_numpy(occ_rays).cuda()
    ms, reps = timed(lambda: api.trace_rays(scene, occ_t, any_hit=True, asynchronous=True))
    occluded = api.trace_rays(scene, occ_t, any_hit=True).occluded
    out["occlusion"] = {"ms": ms, "mrays_s": len(keep) / ms / 1e3, "launches": reps, "rays": int(len(keep)),
                        "occluded_fraction": float(occluded.float().mean())}
    st = api.trace_rays(scene, rays, collect_stats=True).stats
    out["closest_camera_counters"] = {"node_visits_per_ray": st.numNodeVisits / n, "tri_tests_per_ray": st.numTriTests / n, "tail_rays": int(st.tailRays)}
    ctx.set_stream(None)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
