"""What the multi-hit query costs (rtr_trace_rays_multi) on sponza_class at 1920x1080, 1 spp: one JSON line, also written to
profiles/multihit/multihit_rate_<height>p.json.  One process:

  (a) K = 1, 2, 4, 8 against rtr_trace_rays_masked(RTR_QUERY_CLOSEST, cullMask 0xff) on the same rays, their five repeats interleaved, for
        camera      the frame's camera rays
        shuffled    the same rays in a seeded random permutation
  (b) a K = 2 chain run to exhaustion (every link resumed from a device-side gather of the previous link's last slots, no host join inside
      a link; the host reads the counts between links to know when to stop) against K = 8 once, on the camera rays: the wall time of the
      whole chain, its links, and how many hits each found;
  (c) the counters of every K of (a): record visits and triangle tests per ray, tail rays, and how the hit counts are distributed.

HIP events on the query's stream, as profiles/query_rate.py times (its `timed`): three warm-up launches, then at least 0.2 s of launches.

    python profiles/multihit_rate.py [--width 1920 --height 1080]
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
from cull_mask_rate import five_each  # noqa: E402
from realtimeraytracer_amd import _abi as A  # noqa: E402
from realtimeraytracer_amd import api, scenes  # noqa: E402

KS = (1, 2, 4, 8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--out", default=None, help="where the JSON goes (default profiles/multihit/multihit_rate_<height>p.json)")
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
    out = {"what": "cost of the multi-hit ray query against the closest-hit query", "scene": "sponza_class", "width": W, "height": H, "spp": 1,
           "device": ctx.device_name(), "kernel_revision": A.hip_lib().rtr_kernel_revision().decode(), "rays": n}

    rays = api.camera_rays(ctx, s.camera, W, H, 1)
    g = torch.Generator(device="cpu").manual_seed(args.seed)
    shuffled = rays[torch.randperm(n, generator=g).cuda()].contiguous()
    hits = torch.empty((n, max(KS), 8), dtype=torch.int32, device=rays.device)
    counts = torch.empty(n, dtype=torch.int32, device=rays.device)

    def closest(r):
        assert lib.rtr_trace_rays_masked_async(ctx.h, scene.h, VP(r.data_ptr()), None, n, A.QUERY_CLOSEST, 0xff, VP(hits.data_ptr()), None) == 0

    def multi(r, k):
        assert lib.rtr_trace_rays_multi_async(ctx.h, scene.h, VP(r.data_ptr()), None, n, k, 0, 0xff, None, VP(hits.data_ptr()), VP(counts.data_ptr())) == 0

    # (a) every K against the closest-hit query
    a = {}
    for name, r in (("camera", rays), ("shuffled", shuffled)):
        fns = {"closest_masked_ff": lambda r=r: closest(r)}
        fns.update({f"multi_k{k}": (lambda r=r, k=k: multi(r, k)) for k in KS})
        res = five_each(fns)
        for k in KS:
            res[f"multi_k{k}"]["over_closest_min"] = res[f"multi_k{k}"]["ms_min"] / res["closest_masked_ff"]["ms_min"]
            res[f"multi_k{k}"]["mrays_per_s_min"] = n / res[f"multi_k{k}"]["ms_min"] / 1e3
        res["closest_masked_ff"]["mrays_per_s_min"] = n / res["closest_masked_ff"]["ms_min"] / 1e3
        a[name] = res
    out["k_against_closest"] = a

    # (c) counters and the distribution of the hit counts
    c = {}
    st = A.rtr_query_stats()
    assert lib.rtr_trace_rays_masked(ctx.h, scene.h, VP(rays.data_ptr()), None, n, A.QUERY_CLOSEST, 0xff, VP(hits.data_ptr()), None, C.byref(st)) == 0
    c["closest_masked_ff"] = {"visits_per_ray": st.numNodeVisits / n, "tri_tests_per_ray": st.numTriTests / n, "alpha_tests": st.numAlphaTests, "tail_rays": st.tailRays}
    for k in KS:
        assert lib.rtr_trace_rays_multi(ctx.h, scene.h, VP(rays.data_ptr()), None, n, k, 0, 0xff, None, VP(hits.data_ptr()), VP(counts.data_ptr()), C.byref(st)) == 0
        c[f"multi_k{k}"] = {"visits_per_ray": st.numNodeVisits / n, "tri_tests_per_ray": st.numTriTests / n, "alpha_tests": st.numAlphaTests, "tail_rays": st.tailRays,
                            "hits_per_ray": float(counts.sum()) / n, "rays_by_count": torch.bincount(counts, minlength=k + 1).tolist()}
    out["counters_camera"] = c

    # (b) a K = 2 chain to exhaustion against K = 8 once
    def chain(k, limit=64):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        found, links = [], 0
        res = api.trace_rays_multi(scene, rays, k, asynchronous=True)
        while links < limit:
            links += 1
            m = int(res.counts.sum())            # the host join between links: it decides whether to go on
            if m == 0:
                break
            found.append(m)
            res = api.trace_rays_multi(scene, rays, k, after=res, asynchronous=True)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, found

    chain(2)                                     # warm-up
    runs = [chain(2) for _ in range(5)]
    once = five_each({"multi_k8": lambda: multi(rays, 8)})["multi_k8"]
    multi(rays, 8)
    torch.cuda.synchronize()
    out["chain_k2_to_exhaustion"] = {"wall_ms_min": min(r[0] for r in runs), "wall_ms_all": [r[0] for r in runs], "links_with_hits": len(runs[0][1]),
                                     "hits_per_link": runs[0][1], "hits_total": sum(runs[0][1]), "k8_once_ms_min": once["ms_min"],
                                     "k8_once_hits": int(counts.sum()), "rays_with_8_or_more_hits": int((counts == 8).sum()),
                                     "note": "wall_ms includes the Python layer, the gathers of the last slots and one host join per link; k8_once is HIP events"}
    ctx.set_stream(None)
    path = args.out or os.path.join(ROOT, "profiles", "multihit", f"multihit_rate_{H}p.json")
    os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
