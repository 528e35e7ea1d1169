"""Occlusion-query rates on the bench frame's light rays (sponza_class, 1920x1080, 1 spp: the light rays rtr_light_rays makes of the
camera hits, null slots included), one JSON line, also written to profiles/occlusion/occlusion_rate_<height>p.json:

  dense      rtr_trace_rays(RTR_QUERY_ANY) on the ray buffer                                   (k_query + k_query_tail over the BVH2)
  queued     rtr_trace_occlusion on the same buffer, queue build, walk and tail together       (kernels/rtr_occlusion.hip), and its
             counting form once: rays, record visits, triangle tests per ray, tail rays
  composed_dense / composed_queued   closest hit -> light rays -> occlusion -> shade -> tone map, the occlusion either way
  render     rtr_render of the same frame with the tunable trace_own_leaf = 0: shadowGenMs + shadowTraceMs are the floor — the
             renderer's own queue build and walk without the one rule an RtrRay cannot carry

Every timed loop is repeated five times (min and median reported).  Every step is a process of its own under its own time limit (this
file re-runs itself with --step): a step that hangs or faults ends there and nothing is started after it.

    python profiles/occlusion_rate.py [--width 1920 --height 1080]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEPS = (("dense", 240), ("queued", 240), ("composed_dense", 240), ("composed_queued", 240), ("render", 120))


def step(args):
    import ctypes as C

    import torch

    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "profiles"))
    from query_rate import timed
    from realtimeraytracer_amd import _abi as A
    from realtimeraytracer_amd import api, scenes

    def five(fn):
        ms = [timed(fn)[0] for _ in range(5)]
        return {"ms_min": min(ms), "ms_median": statistics.median(ms), "ms_all": ms}

    W, H = args.width, args.height
    torch.cuda.init()
    ctx = api.Context(0)
    stream = torch.cuda.Stream()          # a stream of its own: the default stream's handle (0) would give the context a new stream
    torch.cuda.set_stream(stream)
    ctx.set_stream(stream.cuda_stream)
    s = scenes.sponza_class(W, H)
    scene = api.Scene(ctx, s.desc)
    lib, n, VP = ctx.lib, W * H, A.VP
    out = {"device": ctx.device_name(), "kernel_revision": A.hip_lib().rtr_kernel_revision().decode()}
    if args.step == "render":
        ctx.set_tunable("trace_own_leaf", 0)
        frame = api.Frame(ctx, W, H)
        p = api.make_params(W, H, spp=1, shadow_rays=3)
        gen, trace, total = [], [], []
        for _ in range(5):
            for _ in range(20):
                api.render(scene, s.camera, s.scene_info(0), p, frame)
            g = frame.stats()
            gen.append(g.shadowGenMs); trace.append(g.shadowTraceMs); total.append(g.totalMs)
        out.update({"trace_own_leaf": 0, "shadow_gen_ms_min": min(gen), "shadow_gen_ms_median": statistics.median(gen),
                    "shadow_trace_ms_min": min(trace), "shadow_trace_ms_median": statistics.median(trace),
                    "total_ms_min": min(total), "total_ms_median": statistics.median(total)})
    else:
        lp = api.make_light_params(s.num_lights, 3, 0, W, 1, A.LIGHT_SHADOWED)
        Q = api.light_slots(scene, lp)
        rays = api.camera_rays(ctx, s.camera, W, H, 1)
        hits = torch.empty((n, 8), dtype=torch.int32, device=rays.device)
        lrays = torch.empty((n * Q, 8), dtype=torch.float32, device=rays.device)
        occ = torch.empty(n * Q, dtype=torch.uint8, device=rays.device)
        rad = torch.empty((n, 12), dtype=torch.float32, device=rays.device)
        px = torch.empty(n, dtype=torch.int32, device=rays.device)
        need = api.occlusion_scratch_bytes(lib, n * Q)
        scratch = torch.empty(need, dtype=torch.uint8, device=rays.device)

        def closest():
            assert lib.rtr_trace_rays_async(ctx.h, scene.h, VP(rays.data_ptr()), n, A.QUERY_CLOSEST, VP(hits.data_ptr()), None) == 0

        def light():
            assert lib.rtr_light_rays_async(ctx.h, scene.h, VP(rays.data_ptr()), VP(hits.data_ptr()), n, C.byref(lp), None, VP(lrays.data_ptr())) == 0

        def dense():
            assert lib.rtr_trace_rays_async(ctx.h, scene.h, VP(lrays.data_ptr()), n * Q, A.QUERY_ANY, None, VP(occ.data_ptr())) == 0

        def queued():
            assert lib.rtr_trace_occlusion_async(ctx.h, scene.h, VP(lrays.data_ptr()), n * Q, 0, VP(scratch.data_ptr()), need, VP(occ.data_ptr())) == 0

        def shade():
            assert lib.rtr_shade_hits_async(ctx.h, scene.h, VP(rays.data_ptr()), VP(hits.data_ptr()), n, C.byref(lp), None, VP(occ.data_ptr()),
                                            VP(rad.data_ptr())) == 0

        def tonemap():
            assert lib.rtr_tonemap_pack_async(ctx.h, VP(rad.data_ptr()), 48, n, VP(px.data_ptr())) == 0

        closest(); light()
        torch.cuda.synchronize()
        out.update({"hits": n, "slots_per_hit": Q, "rays": n * Q, "ray_bytes": n * Q * 32, "scratch_bytes": need})
        occlusion = queued if args.step in ("queued", "composed_queued") else dense
        if args.step in ("dense", "queued"):
            out["null_share"] = 1.0 - float(lrays.any(1).sum()) / (n * Q)
            out.update(five(occlusion))
            out["mrays_s"] = n * Q / out["ms_min"] / 1e3
            out["occluded"] = int(occ.to(torch.int64).sum())
            st = A.rtr_query_stats()
            if args.step == "queued":
                assert lib.rtr_trace_occlusion(ctx.h, scene.h, VP(lrays.data_ptr()), n * Q, 0, VP(scratch.data_ptr()), need, VP(occ.data_ptr()), C.byref(st)) == 0
            else:
                assert lib.rtr_trace_rays(ctx.h, scene.h, VP(lrays.data_ptr()), n * Q, A.QUERY_ANY, None, VP(occ.data_ptr()), C.byref(st)) == 0
            out["counters"] = {"rays_counted": st.numRays, "node_visits": st.numNodeVisits, "tri_tests": st.numTriTests, "alpha_tests": st.numAlphaTests,
                               "tail_rays": st.tailRays, "visits_per_counted_ray": st.numNodeVisits / max(st.numRays, 1),
                               "tri_tests_per_counted_ray": st.numTriTests / max(st.numRays, 1)}
        else:
            def whole():
                closest(); light(); occlusion(); shade(); tonemap()
            out.update(five(whole))
            out["mhits_s"] = n / out["ms_min"] / 1e3
    ctx.set_stream(None)
    print("STEP " + json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--step", choices=[n for n, _ in STEPS])
    args = ap.parse_args()
    if args.step:
        return step(args)
    out = {"what": "occlusion-query rates on the light rays of a frame's camera hits", "scene": "sponza_class", "width": args.width,
           "height": args.height, "spp": 1}
    ok = True
    for name, limit in STEPS:
        cmd = [sys.executable, os.path.abspath(__file__), "--step", name, "--width", str(args.width), "--height", str(args.height)]
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=limit)
        except subprocess.TimeoutExpired:
            out[name] = {"error": f"no result within {limit} s"}
            ok = False
            break                                           # nothing more is started on the device after a step that did not end
        line = [ln for ln in r.stdout.splitlines() if ln.startswith("STEP ")]
        if r.returncode != 0 or not line:
            out[name] = {"error": f"exit status {r.returncode}", "stderr": r.stderr[-2000:]}
            ok = False
            break
        out[name] = json.loads(line[-1][5:])
    if ok:
        out["device"], out["rtr_kernel_revision"] = out["dense"]["device"], out["dense"]["kernel_revision"]
        out["same_answers"] = out["dense"]["occluded"] == out["queued"]["occluded"]
        out["queued_over_dense_min"] = out["queued"]["ms_min"] / out["dense"]["ms_min"]
        out["queued_over_dense_median"] = out["queued"]["ms_median"] / out["dense"]["ms_median"]
        out["composed_queued_over_dense_min"] = out["composed_queued"]["ms_min"] / out["composed_dense"]["ms_min"]
        out["queued_over_render_floor_min"] = out["queued"]["ms_min"] / (out["render"]["shadow_gen_ms_min"] + out["render"]["shadow_trace_ms_min"])
        path = os.path.join(ROOT, "profiles", "occlusion", f"occlusion_rate_{args.height}p.json")
        os.makedirs(os.path.dirname(path), exist_ok=True)
        with open(path, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")
    print(json.dumps(out))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
