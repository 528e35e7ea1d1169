"""Hit-surface rates (rtr_hit_surfaces) on sponza_class at 1920x1080, 1 spp: one JSON line.

  camera    the surfaces of the frame's camera-ray hits (rtr_camera_rays_async + a closest-hit query), in ray order
  shuffled  the same rays and hits in a seeded random permutation (incoherent gathers)
  query     the closest-hit query that made the hits, timed the same way, for scale

Bytes per hit, against the issue's model: reads 64 (ray + hit) + 12 (3 indices) + 144 (3 x 48-B vertices) + 80 (ObjectInfo) + 96 (xform +
nmat), write 80: ~476 B touched per hit before texels; of these only the streams (ray 32, hit 32, surface 80 = 144 B) need to come from
HBM when the gathers hit in L2.  The achieved rate is reported over those 144 B.

HIP events on the context's stream, which is torch's current stream; the surfaces are enqueued through the C ABI directly
(rtr_hit_surfaces_async, output preallocated) so that the timing is of the kernel, not of Python.  Three warm-up launches, then at least
0.2 s of timed launches per case.

    python profiles/surface_rate.py [--width 1920 --height 1080]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "profiles"))
from query_rate import timed  # noqa: E402
from realtimeraytracer_amd import _abi as A  # noqa: E402
from realtimeraytracer_amd import api, scenes  # noqa: E402

TOUCHED_BYTES = 64 + 12 + 144 + 80 + 96 + 80
STREAM_BYTES = 32 + 32 + 80


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
    out = {"what": "hit-surface rates", "scene": "sponza_class", "width": W, "height": H, "spp": 1, "hits": n,
           "device": ctx.device_name(), "kernel_revision": A.hip_lib().rtr_kernel_revision().decode(),
           "model_touched_bytes_per_hit": TOUCHED_BYTES, "model_hbm_bytes_per_hit": STREAM_BYTES}
    lib = ctx.lib

    rays = api.camera_rays(ctx, s.camera, W, H, 1)
    hits = api.trace_rays(scene, rays).hits
    surf = torch.empty((n, 20), dtype=torch.float32, device=rays.device)
    torch.cuda.synchronize()

    def case(r, h):
        rp, hp, op = A.VP(r.data_ptr()), A.VP(h.data_ptr()), A.VP(surf.data_ptr())
        ms, reps = timed(lambda: lib.rtr_hit_surfaces_async(ctx.h, scene.h, rp, hp, n, op))
        return {"ms": ms, "mhits_s": n / ms / 1e3, "launches": reps, "hbm_gb_s": n * STREAM_BYTES / ms / 1e6,
                "touched_gb_s": n * TOUCHED_BYTES / ms / 1e6}

    assert lib.rtr_hit_surfaces_async(ctx.h, scene.h, A.VP(rays.data_ptr()), A.VP(hits.data_ptr()), n, A.VP(surf.data_ptr())) == 0
    torch.cuda.synchronize()
    kind = surf.view(torch.int32)[:, 3].cpu().numpy()
    out["kinds"] = {name: int((kind == k).sum()) for name, k in (("miss", A.SURFACE_MISS), ("object", A.SURFACE_OBJECT),
                                                                  ("light", A.SURFACE_LIGHT), ("invalid", A.SURFACE_INVALID))}
    ois = [s.desc.objects[i] for i in range(s.desc.numObjects)]
    out["objects_with_maps"] = int(sum(1 for o in ois if o.usesColorMap or o.usesSpecularMap or o.usesMetallicMap))
    out["camera"] = case(rays, hits)

    g = torch.Generator(device="cpu").manual_seed(args.seed)
    perm = torch.randperm(n, generator=g).cuda()
    rays_s, hits_s = rays[perm].contiguous(), hits[perm].contiguous()
    torch.cuda.synchronize()
    out["shuffled"] = case(rays_s, hits_s)

    ms, reps = timed(lambda: api.trace_rays(scene, rays, asynchronous=True))
    out["query_closest_camera"] = {"ms": ms, "launches": reps}
    out["camera_over_query"] = out["camera"]["ms"] / ms
    out["camera_within_0_10_ms"] = bool(out["camera"]["ms"] <= 0.10)
    ctx.set_stream(None)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
