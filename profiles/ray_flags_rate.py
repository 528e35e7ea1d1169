"""What the culling ray flags of the ray queries cost (RTR_QUERY_CULL_BACK_FACING / FRONT_FACING / OPAQUE / NO_OPAQUE) on the bench
frame — sponza_class and sponza_mixed at 1920x1080, 1 spp: one JSON line, also written to profiles/ray_flags/ray_flags_rate_<height>p.json.
One process per scene list; per scene, per route

    closest_camera       closest hit of the frame's camera rays            (k_query + k_query_tail over the BVH2)
    closest_shuffled     the same rays in a seeded random permutation
    any_light_dense      the frame's light rays (rtr_light_rays_hinted of the camera hits, null slots included), RTR_QUERY_ANY
    any_light_queued_hinted   the same rays and their hints through the queued query (k_occlusion_gen, k_shadow_trace4, k_query_tail)

the unflagged call (which launches the unfiltered kernels) and the same call with each of the four flags (which launch the filtered,
cull-mask forms with mask 0xff), their five repeats interleaved, the minimum reported; then one counting-form call of each for the
node visits, triangle tests and opacity tests per ray.  A flag changes the answers, so it changes the work: the rows say what a call
with the flag costs on this frame, not what the filter's instructions cost (profiles/cull_mask_rate.py prices those: the same forms
with nothing culled).

HIP events on the query's stream, as profiles/query_rate.py times (its `timed`): three warm-up launches, then at least 0.2 s of launches.

    python profiles/ray_flags_rate.py [--width 1920 --height 1080] [--scenes sponza_class,sponza_mixed]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "profiles"))
from query_rate import timed  # noqa: E402
from realtimeraytracer_amd import _abi as A  # noqa: E402
from realtimeraytracer_amd import api, scenes  # noqa: E402

FLAGS = {"none": 0, "cull_back_facing": A.QUERY_CULL_BACK_FACING, "cull_front_facing": A.QUERY_CULL_FRONT_FACING,
         "cull_opaque": A.QUERY_CULL_OPAQUE, "cull_no_opaque": A.QUERY_CULL_NO_OPAQUE}


def five_each(fns):
    """the repeats of several loops interleaved, so that a drift of the clock is in all of them alike"""
    ms = {k: [] for k in fns}
    for _ in range(5):
        for k, fn in fns.items():
            ms[k].append(timed(fn)[0])
    return {k: {"ms_min": min(v), "ms_median": statistics.median(v), "ms_all": v} for k, v in ms.items()}


def one_scene(ctx, name, W, H, seed):
    s = getattr(scenes, name)(W, H)
    scene = api.Scene(ctx, s.desc)
    lib, n, VP = ctx.lib, W * H, A.VP
    lp = api.make_light_params(s.num_lights, 3, 0, W, 1, A.LIGHT_SHADOWED)
    Q = api.light_slots(scene, lp)
    rays = api.camera_rays(ctx, s.camera, W, H, 1)
    g = torch.Generator(device="cpu").manual_seed(seed)
    shuffled = rays[torch.randperm(n, generator=g).cuda()].contiguous()
    hits = torch.empty((n, 8), dtype=torch.int32, device=rays.device)
    lrays = torch.empty((n * Q, 8), dtype=torch.float32, device=rays.device)
    leaves = torch.empty(n * Q, dtype=torch.int32, device=rays.device)
    occ = torch.empty(n * Q, dtype=torch.uint8, device=rays.device)
    need = api.occlusion_scratch_bytes(lib, n * Q)
    scratch = torch.empty(need, dtype=torch.uint8, device=rays.device)
    assert lib.rtr_trace_rays(ctx.h, scene.h, VP(rays.data_ptr()), n, A.QUERY_CLOSEST, VP(hits.data_ptr()), None, None) == 0
    assert lib.rtr_light_rays_hinted(ctx.h, scene.h, VP(rays.data_ptr()), VP(hits.data_ptr()), n, C.byref(lp), None, VP(lrays.data_ptr()),
                                     VP(leaves.data_ptr())) == 0
    out = {"camera_rays": n, "slots_per_hit": Q, "light_rays": n * Q, "null_share_of_light_rays": 1.0 - float(lrays.any(1).sum()) / (n * Q)}
    hp, op, sp = VP(hits.data_ptr()), VP(occ.data_ptr()), VP(scratch.data_ptr())

    def closest(r, f, st=None):
        if st is None:
            assert lib.rtr_trace_rays_async(ctx.h, scene.h, VP(r.data_ptr()), n, A.QUERY_CLOSEST | f, hp, None) == 0
        else:
            assert lib.rtr_trace_rays(ctx.h, scene.h, VP(r.data_ptr()), n, A.QUERY_CLOSEST | f, hp, None, C.byref(st)) == 0

    def dense(f, st=None):
        if st is None:
            assert lib.rtr_trace_rays_async(ctx.h, scene.h, VP(lrays.data_ptr()), n * Q, A.QUERY_ANY | f, None, op) == 0
        else:
            assert lib.rtr_trace_rays(ctx.h, scene.h, VP(lrays.data_ptr()), n * Q, A.QUERY_ANY | f, None, op, C.byref(st)) == 0

    def hinted(f, st=None):
        if st is None:
            assert lib.rtr_trace_occlusion_hinted_async(ctx.h, scene.h, VP(lrays.data_ptr()), VP(leaves.data_ptr()), n * Q, f, sp, need, op) == 0
        else:
            assert lib.rtr_trace_occlusion_hinted(ctx.h, scene.h, VP(lrays.data_ptr()), VP(leaves.data_ptr()), n * Q, f, sp, need, op, C.byref(st)) == 0

    routes = {"closest_camera": (lambda f, st=None: closest(rays, f, st), n), "closest_shuffled": (lambda f, st=None: closest(shuffled, f, st), n),
              "any_light_dense": (dense, n * Q), "any_light_queued_hinted": (hinted, n * Q)}
    for rname, (fn, m) in routes.items():
        r = five_each({k: (lambda fn=fn, f=f: fn(f)) for k, f in FLAGS.items()})
        for k, f in FLAGS.items():
            st = A.rtr_query_stats()
            fn(f, st)
            rays_counted = max(st.numRays, 1)
            r[k]["over_unflagged_min"] = r[k]["ms_min"] / r["none"]["ms_min"]
            r[k]["counters"] = {"rays_counted": st.numRays, "visits_per_ray": st.numNodeVisits / rays_counted, "tri_tests_per_ray": st.numTriTests / rays_counted,
                                "alpha_tests": st.numAlphaTests, "tail_rays": st.tailRays,
                                "answers": int(occ[:m].sum()) if rname.startswith("any") else int((hits[:, 3] >= 0).sum())}
        r["rays"] = m
        out[rname] = r
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--scenes", default="sponza_class,sponza_mixed")
    ap.add_argument("--out", default=None, help="where the JSON goes (default profiles/ray_flags/ray_flags_rate_<height>p.json)")
    args = ap.parse_args()
    W, H = args.width, args.height
    torch.cuda.init()
    ctx = api.Context(0)
    stream = torch.cuda.Stream()          # a stream of its own: the default stream's handle (0) would give the context a new stream
    torch.cuda.set_stream(stream)
    ctx.set_stream(stream.cuda_stream)
    out = {"what": "cost of the culling ray flags in the ray queries", "width": W, "height": H, "spp": 1,
           "device": ctx.device_name(), "kernel_revision": A.hip_lib().rtr_kernel_revision().decode(), "scenes": {}}
    for name in args.scenes.split(","):
        out["scenes"][name] = one_scene(ctx, name, W, H, args.seed)
    ctx.set_stream(None)
    path = args.out or os.path.join(ROOT, "profiles", "ray_flags", f"ray_flags_rate_{H}p.json")
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
