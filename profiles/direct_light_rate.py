"""Direct-lighting rates for ray-query hits on sponza_class at 1920x1080, 1 spp (the bench frame's camera rays): one JSON line.

  composed   closest hit -> rtr_light_rays -> RTR_QUERY_ANY of those rays -> rtr_shade_hits (framebuffer output only) ->
             rtr_tonemap_pack, in chunks of hits whose light rays fit --ray-mb; hits/s of the whole and the share of each launch
  direct     rtr_light_rays alone in the unstaged form of its kernel (every lane storing its rays at its own 32 Q-byte stride), which
             only the library's test build can select: what the staged form (rays made in LDS, stored as one block per wave) is worth
  render     rtr_render_async of the same frame, AS A REFERENCE POINT ONLY: the composed route traces dense, unbinned rays (null slots
             included) over the BVH2 where the staged pipeline walks a compacted, octant-binned queue over the 4-wide tree.  No
             ratio is promised.

Every step is a process of its own under its own time limit (this file re-runs itself with --step), so a step that hangs or faults
ends there and nothing is started after it.  HIP events on the context's stream, which is torch's current stream; the launches go
through the C ABI directly with preallocated outputs, so that the timing is of the kernels, not of Python.

    python profiles/direct_light_rate.py [--width 1920 --height 1080 --ray-mb 256]
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEPS = (("composed", 240), ("render", 120), ("direct", 120))


def step(args):
    import ctypes as C

    import torch

    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "profiles"))
    from query_rate import timed
    from realtimeraytracer_amd import _abi as A
    from realtimeraytracer_amd import api, scenes

    W, H = args.width, args.height
    torch.cuda.init()
    if args.step == "direct":
        os.environ["RTR_LIGHT_RAYS_DIRECT"] = "1"
    ctx = api.Context(0, test_hooks=args.step == "direct")
    stream = torch.cuda.Stream()          # a stream of its own: the default stream's handle (0) would give the context a new stream
    torch.cuda.set_stream(stream)
    ctx.set_stream(stream.cuda_stream)
    s = scenes.sponza_class(W, H)
    scene = api.Scene(ctx, s.desc)
    lib, n = ctx.lib, W * H
    out = {"device": ctx.device_name(), "kernel_revision": A.hip_lib().rtr_kernel_revision().decode()}
    if args.step == "render":
        frame = api.Frame(ctx, W, H)
        p = api.make_params(W, H, spp=1, shadow_rays=3)
        ms, reps = timed(lambda: api.render(scene, s.camera, s.scene_info(0), p, frame, asynchronous=True))
        out.update({"ms": ms, "launches": reps})
    else:
        lp = api.make_light_params(s.num_lights, 3, 0, W, 1, A.LIGHT_SHADOWED)
        Q = api.light_slots(scene, lp)
        chunk = min(n, max(1, (args.ray_mb << 20) // (32 * Q)))
        rays = api.camera_rays(ctx, s.camera, W, H, 1)
        hits = torch.empty((n, 8), dtype=torch.int32, device=rays.device)
        lrays = torch.empty((chunk * Q, 8), dtype=torch.float32, device=rays.device)
        occ = torch.empty(chunk * Q, dtype=torch.uint8, device=rays.device)
        rad = torch.empty((n, 12), dtype=torch.float32, device=rays.device)
        px = torch.empty(n, dtype=torch.int32, device=rays.device)
        k = torch.arange(n, device=rays.device, dtype=torch.int64)
        seeds = ((k % W) * 733 + (k // W) * 1933).to(torch.int32)          # explicit, so that a chunk may start anywhere
        VP = A.VP
        chunks = [(a, min(n, a + chunk)) for a in range(0, n, chunk)]

        def closest():
            assert lib.rtr_trace_rays_async(ctx.h, scene.h, VP(rays.data_ptr()), n, A.QUERY_CLOSEST, VP(hits.data_ptr()), None) == 0

        def light(a, b):
            assert lib.rtr_light_rays_async(ctx.h, scene.h, VP(rays.data_ptr() + 32 * a), VP(hits.data_ptr() + 32 * a), b - a, C.byref(lp),
                                            VP(seeds.data_ptr() + 4 * a), VP(lrays.data_ptr())) == 0

        def anyhit(a, b):
            assert lib.rtr_trace_rays_async(ctx.h, scene.h, VP(lrays.data_ptr()), (b - a) * Q, A.QUERY_ANY, None, VP(occ.data_ptr())) == 0

        def shade(a, b):
            assert lib.rtr_shade_hits_async(ctx.h, scene.h, VP(rays.data_ptr() + 32 * a), VP(hits.data_ptr() + 32 * a), b - a, C.byref(lp),
                                            VP(seeds.data_ptr() + 4 * a), VP(occ.data_ptr()), VP(rad.data_ptr() + 48 * a)) == 0

        def tonemap():
            assert lib.rtr_tonemap_pack_async(ctx.h, VP(rad.data_ptr()), 48, n, VP(px.data_ptr())) == 0

        def whole():
            closest()
            for a, b in chunks:
                light(a, b); anyhit(a, b); shade(a, b)
            tonemap()

        if args.step == "direct":
            closest()
            ms = timed(lambda: [light(a, b) for a, b in chunks])[0]
            out.update({"light_rays_ms": ms, "light_rays_gb_s_written": n * Q * 32 / ms / 1e6})
            ctx.set_stream(None)
            print("STEP " + json.dumps(out))
            return
        whole()
        torch.cuda.synchronize()
        sent = int(lrays[:(chunks[-1][1] - chunks[-1][0]) * Q].any(1).sum())
        ms, reps = timed(whole)
        out.update({"hits": n, "slots_per_hit": Q, "chunks": len(chunks), "chunk_hits": chunk, "ray_mb": args.ray_mb,
                    "rays_sent_share_last_chunk": sent / ((chunks[-1][1] - chunks[-1][0]) * Q),
                    "ms": ms, "launches": reps, "mhits_s": n / ms / 1e3, "mslots_s": n * Q / ms / 1e3})
        parts = {"closest_hit": timed(closest)[0], "tonemap_pack": timed(tonemap)[0]}
        for name, fn in (("light_rays", light), ("any_hit", anyhit), ("shade_hits", shade)):       # in this order: each reads what the one before left
            parts[name] = timed(lambda: [fn(a, b) for a, b in chunks])[0]
        out["launch_ms"] = parts
        out["launch_share"] = {k2: v / sum(parts.values()) for k2, v in parts.items()}
        out["light_rays_gb_s_written"] = n * Q * 32 / parts["light_rays"] / 1e6
    ctx.set_stream(None)
    print("STEP " + json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--ray-mb", type=int, default=256)
    ap.add_argument("--step", choices=[n for n, _ in STEPS])
    args = ap.parse_args()
    if args.step:
        return step(args)
    out = {"what": "direct-lighting rates for ray-query hits", "scene": "sponza_class", "width": args.width, "height": args.height, "spp": 1}
    for name, limit in STEPS:
        cmd = [sys.executable, os.path.abspath(__file__), "--step", name, "--width", str(args.width), "--height", str(args.height),
               "--ray-mb", str(args.ray_mb)]
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=limit)
        except subprocess.TimeoutExpired:
            out[name] = {"error": f"no result within {limit} s"}
            break                                           # nothing more is started on the device after a step that did not end
        line = [ln for ln in r.stdout.splitlines() if ln.startswith("STEP ")]
        if r.returncode != 0 or not line:
            out[name] = {"error": f"exit status {r.returncode}", "stderr": r.stderr[-2000:]}
            break
        out[name] = json.loads(line[-1][5:])
    if "light_rays_ms" in out.get("direct", {}) and "launch_ms" in out.get("composed", {}):
        out["light_rays_direct_over_staged"] = out["direct"]["light_rays_ms"] / out["composed"]["launch_ms"]["light_rays"]
    if "ms" in out.get("composed", {}) and "ms" in out.get("render", {}):
        out["composed_over_render"] = out["composed"]["ms"] / out["render"]["ms"]
    print(json.dumps(out))
    return 0 if "composed_over_render" in out else 1


if __name__ == "__main__":
    sys.exit(main())
