"""What a cull mask costs (rtr_trace_rays_masked, rtr_trace_occlusion_masked) on sponza_class at 1920x1080, 1 spp: one JSON line, also
written to profiles/cull_mask/cull_mask_rate_<height>p.json.  One process:

  (a) unmasked against masked with cullMask 0xff (default instance masks, rayMasks NULL: the same answers and counters), their five
      repeats interleaved, for
        closest_camera      closest hit of the frame's camera rays
        closest_shuffled    the same rays in a seeded random permutation
        light_dense         the frame's light rays (rtr_light_rays_hinted of the camera hits, null slots included), RTR_QUERY_ANY
        light_queued_hinted the same rays and their hints through the queued query
  (b) the same light rays traced as a CLOSEST-hit bounce set with the light instances masked out (bit 0 cleared on the emitters,
      cullMask 0x01), against the same rays unmasked;
  (c) record visits and triangle tests per ray of (b), both ways, and how many rays came back with a light's customIndex.

HIP events on the query's stream, as profiles/query_rate.py times (its `timed`): three warm-up launches, then at least 0.2 s of launches.

    python profiles/cull_mask_rate.py [--width 1920 --height 1080]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "profiles"))
from query_rate import timed  # noqa: E402
from realtimeraytracer_amd import _abi as A  # noqa: E402
from realtimeraytracer_amd import api, scenes  # noqa: E402


def five_each(fns):
    """the repeats of several loops interleaved, so that a drift of the clock is in all of them alike"""
    ms = {k: [] for k in fns}
    for _ in range(5):
        for k, fn in fns.items():
            ms[k].append(timed(fn)[0])
    return {k: {"ms_min": min(v), "ms_median": statistics.median(v), "ms_all": v} for k, v in ms.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--out", default=None, help="where the JSON goes (default profiles/cull_mask/cull_mask_rate_<height>p.json)")
    args = ap.parse_args()
    W, H = args.width, args.height
    torch.cuda.init()
    ctx = api.Context(0)
    stream = torch.cuda.Stream()          # a stream of its own: the default stream's handle (0) would give the context a new stream
    torch.cuda.set_stream(stream)
    ctx.set_stream(stream.cuda_stream)
    s = scenes.sponza_class(W, H)
    scene = api.Scene(ctx, s.desc)
    lib, n, VP = ctx.lib, W * H, A.VP
    out = {"what": "cost of the cull mask in the ray queries", "scene": "sponza_class", "width": W, "height": H, "spp": 1,
           "device": ctx.device_name(), "kernel_revision": A.hip_lib().rtr_kernel_revision().decode()}

    lp = api.make_light_params(s.num_lights, 3, 0, W, 1, A.LIGHT_SHADOWED)
    Q = api.light_slots(scene, lp)
    rays = api.camera_rays(ctx, s.camera, W, H, 1)
    g = torch.Generator(device="cpu").manual_seed(args.seed)
    shuffled = rays[torch.randperm(n, generator=g).cuda()].contiguous()
    hits = torch.empty((n, 8), dtype=torch.int32, device=rays.device)
    lrays = torch.empty((n * Q, 8), dtype=torch.float32, device=rays.device)
    leaves = torch.empty(n * Q, dtype=torch.int32, device=rays.device)
    lhits = torch.empty((n * Q, 8), dtype=torch.int32, device=rays.device)
    occ = torch.empty(n * Q, dtype=torch.uint8, device=rays.device)
    need = api.occlusion_scratch_bytes(lib, n * Q)
    scratch = torch.empty(need, dtype=torch.uint8, device=rays.device)
    assert lib.rtr_trace_rays(ctx.h, scene.h, VP(rays.data_ptr()), n, A.QUERY_CLOSEST, VP(hits.data_ptr()), None, None) == 0
    assert lib.rtr_light_rays_hinted(ctx.h, scene.h, VP(rays.data_ptr()), VP(hits.data_ptr()), n, C.byref(lp), None, VP(lrays.data_ptr()),
                                     VP(leaves.data_ptr())) == 0
    out.update({"camera_rays": n, "slots_per_hit": Q, "light_rays": n * Q, "null_share_of_light_rays": 1.0 - float(lrays.any(1).sum()) / (n * Q)})

    def closest(r, m, masked, cull=0xff):
        if masked:
            assert lib.rtr_trace_rays_masked_async(ctx.h, scene.h, VP(r.data_ptr()), None, m, A.QUERY_CLOSEST, cull, VP(lhits.data_ptr()), None) == 0
        else:
            assert lib.rtr_trace_rays_async(ctx.h, scene.h, VP(r.data_ptr()), m, A.QUERY_CLOSEST, VP(lhits.data_ptr()), None) == 0

    def dense(masked):
        if masked:
            assert lib.rtr_trace_rays_masked_async(ctx.h, scene.h, VP(lrays.data_ptr()), None, n * Q, A.QUERY_ANY, 0xff, None, VP(occ.data_ptr())) == 0
        else:
            assert lib.rtr_trace_rays_async(ctx.h, scene.h, VP(lrays.data_ptr()), n * Q, A.QUERY_ANY, None, VP(occ.data_ptr())) == 0

    def hinted(masked):
        if masked:
            assert lib.rtr_trace_occlusion_masked_async(ctx.h, scene.h, VP(lrays.data_ptr()), VP(leaves.data_ptr()), None, n * Q, 0, 0xff,
                                                        VP(scratch.data_ptr()), need, VP(occ.data_ptr())) == 0
        else:
            assert lib.rtr_trace_occlusion_hinted_async(ctx.h, scene.h, VP(lrays.data_ptr()), VP(leaves.data_ptr()), n * Q, 0, VP(scratch.data_ptr()),
                                                        need, VP(occ.data_ptr())) == 0

    # (a) unmasked against masked with 0xff
    a = {}
    cases = {"closest_camera": (lambda mk: closest(rays, n, mk), n), "closest_shuffled": (lambda mk: closest(shuffled, n, mk), n),
             "light_dense": (dense, n * Q), "light_queued_hinted": (hinted, n * Q)}
    for name, (fn, m) in cases.items():
        r = five_each({"unmasked": lambda fn=fn: fn(False), "masked_ff": lambda fn=fn: fn(True)})
        r["rays"] = m
        r["masked_over_unmasked_min"] = r["masked_ff"]["ms_min"] / r["unmasked"]["ms_min"]
        r["masked_over_unmasked_median"] = r["masked_ff"]["ms_median"] / r["unmasked"]["ms_median"]
        a[name] = r
    out["masked_ff_against_unmasked"] = a

    # (b), (c) the light rays as a closest-hit bounce set, the emitters masked out
    masks = np.array([0xfe if s.desc.instances[i].customIndex < s.num_lights else 0xff for i in range(s.desc.numInstances)], np.uint8)
    scene.set_instance_masks(masks)
    b = five_each({"unmasked": lambda: closest(lrays, n * Q, False), "lights_masked_out": lambda: closest(lrays, n * Q, True, 0x01)})
    b["rays"] = n * Q
    b["masked_over_unmasked_min"] = b["lights_masked_out"]["ms_min"] / b["unmasked"]["ms_min"]
    st = A.rtr_query_stats()
    for key, masked in (("unmasked", False), ("lights_masked_out", True)):
        if masked:
            assert lib.rtr_trace_rays_masked(ctx.h, scene.h, VP(lrays.data_ptr()), None, n * Q, A.QUERY_CLOSEST, 0x01, VP(lhits.data_ptr()), None, C.byref(st)) == 0
        else:
            assert lib.rtr_trace_rays(ctx.h, scene.h, VP(lrays.data_ptr()), n * Q, A.QUERY_CLOSEST, VP(lhits.data_ptr()), None, C.byref(st)) == 0
        ci = lhits[:, 3]
        b[key]["counters"] = {"rays_counted": st.numRays, "node_visits": st.numNodeVisits, "tri_tests": st.numTriTests, "tail_rays": st.tailRays,
                              "visits_per_ray": st.numNodeVisits / max(st.numRays, 1), "tri_tests_per_ray": st.numTriTests / max(st.numRays, 1),
                              "light_hits": int(((ci >= 0) & (ci < s.num_lights)).sum()), "hits": int((ci >= 0).sum())}
    out["bounce_off_the_emitters"] = b
    ctx.set_stream(None)
    path = args.out or os.path.join(ROOT, "profiles", "cull_mask", f"cull_mask_rate_{H}p.json")
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
