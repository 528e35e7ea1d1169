"""Occlusion-query rates on the bench frame's light rays (sponza_class, 1920x1080, 1 spp: the light rays rtr_light_rays makes of the
camera hits, null slots included), one JSON line, also written to profiles/occlusion/occlusion_rate_<height>p.json:

  dense      rtr_trace_rays(RTR_QUERY_ANY) on the ray buffer                                   (k_query + k_query_tail over the BVH2)
  queued     rtr_trace_occlusion on the same buffer, queue build, walk and tail together       (kernels/rtr_occlusion.hip), and its
             counting form once: rays, record visits, triangle tests per ray, tail rays
  composed_dense / composed_queued   closest hit -> light rays -> occlusion -> shade -> tone map, the occlusion either way
  render     rtr_render of the same frame with the tunable trace_own_leaf = 0: shadowGenMs + shadowTraceMs are the floor — the
             renderer's own queue build and walk without the one rule an RtrRay cannot carry

With --own-leaf the start hints of the queued query are measured instead, on the same rays, into profiles/occlusion/own_leaf_rate_<height>p.json:

  own_leaf            rtr_trace_occlusion and rtr_trace_occlusion_hinted (rtr_light_rays_hinted's hints) on the same ray buffer in the
                      same process, their five repeats interleaved; both counting forms once; rtr_light_rays against
                      rtr_light_rays_hinted, interleaved likewise
  composed_own_leaf   closest hit -> hinted light rays -> hinted occlusion -> shade -> tone map
  render_default      rtr_render at the default tunables (trace_own_leaf = 1): shadowGenMs + shadowTraceMs, the renderer's own queue build
                      and walk with the rule

Every timed loop is repeated five times (min and median reported).  Every step is a process of its own under its own time limit (this
file re-runs itself with --step): a step that hangs or faults ends there and nothing is started after it.

    python profiles/occlusion_rate.py [--width 1920 --height 1080] [--own-leaf]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEPS = (("dense", 240), ("queued", 240), ("composed_dense", 240), ("composed_queued", 240), ("render", 120))
OWN_LEAF_STEPS = (("own_leaf", 300), ("composed_own_leaf", 240), ("render_default", 120))


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
    if args.step in ("render", "render_default"):
        own = 0 if args.step == "render" else ctx.get_tunable("trace_own_leaf")
        ctx.set_tunable("trace_own_leaf", own)
        frame = api.Frame(ctx, W, H)
        p = api.make_params(W, H, spp=1, shadow_rays=3)
        gen, trace, total = [], [], []
        for _ in range(5):
            for _ in range(20):
                api.render(scene, s.camera, s.scene_info(0), p, frame)
            g = frame.stats()
            gen.append(g.shadowGenMs); trace.append(g.shadowTraceMs); total.append(g.totalMs)
        out.update({"trace_own_leaf": own, "shadow_gen_ms_min": min(gen), "shadow_gen_ms_median": statistics.median(gen),
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

        leaves = torch.empty(n * Q, dtype=torch.int32, device=rays.device)

        def light_hinted():
            assert lib.rtr_light_rays_hinted_async(ctx.h, scene.h, VP(rays.data_ptr()), VP(hits.data_ptr()), n, C.byref(lp), None, VP(lrays.data_ptr()),
                                                   VP(leaves.data_ptr())) == 0

        def hinted():
            assert lib.rtr_trace_occlusion_hinted_async(ctx.h, scene.h, VP(lrays.data_ptr()), VP(leaves.data_ptr()), n * Q, 0, VP(scratch.data_ptr()), need,
                                                        VP(occ.data_ptr())) == 0

        def five_each(fns):
            """the repeats of several loops interleaved, so that a drift of the clock is in all of them alike"""
            ms = {k: [] for k in fns}
            for _ in range(5):
                for k, fn in fns.items():
                    ms[k].append(timed(fn)[0])
            return {k: {"ms_min": min(v), "ms_median": statistics.median(v), "ms_all": v} for k, v in ms.items()}

        closest(); light()
        if args.step in ("own_leaf", "composed_own_leaf"):
            light_hinted()                 # the scene's first hinted call builds its leaf table, outside every timed loop
        torch.cuda.synchronize()
        out.update({"hits": n, "slots_per_hit": Q, "rays": n * Q, "ray_bytes": n * Q * 32, "scratch_bytes": need})
        occlusion = queued if args.step in ("queued", "composed_queued") else dense
        if args.step == "own_leaf":
            def counters(stq):
                return {"rays_counted": stq.numRays, "node_visits": stq.numNodeVisits, "tri_tests": stq.numTriTests, "alpha_tests": stq.numAlphaTests,
                        "tail_rays": stq.tailRays, "visits_per_counted_ray": stq.numNodeVisits / max(stq.numRays, 1),
                        "tri_tests_per_counted_ray": stq.numTriTests / max(stq.numRays, 1)}
            out["hinted_rays"] = int((leaves != 0).sum())
            out["hinted_share_of_sent_rays"] = out["hinted_rays"] / max(int(lrays.any(1).sum()), 1)
            out.update(five_each({"queued": queued, "hinted": hinted}))
            out["occluded"] = {}
            for k, fn in (("queued", queued), ("hinted", hinted)):
                fn(); torch.cuda.synchronize()
                out["occluded"][k] = int(occ.to(torch.int64).sum())
            out["light_rays"] = five_each({"plain": light, "hinted": light_hinted})
            st = A.rtr_query_stats()
            assert lib.rtr_trace_occlusion(ctx.h, scene.h, VP(lrays.data_ptr()), n * Q, 0, VP(scratch.data_ptr()), need, VP(occ.data_ptr()), C.byref(st)) == 0
            out["queued"]["counters"] = counters(st)
            assert lib.rtr_trace_occlusion_hinted(ctx.h, scene.h, VP(lrays.data_ptr()), VP(leaves.data_ptr()), n * Q, 0, VP(scratch.data_ptr()), need,
                                                  VP(occ.data_ptr()), C.byref(st)) == 0
            out["hinted"]["counters"] = counters(st)
        elif args.step == "composed_own_leaf":
            def whole_own_leaf():
                closest(); light_hinted(); hinted(); shade(); tonemap()
            out.update(five(whole_own_leaf))
            out["mhits_s"] = n / out["ms_min"] / 1e3
        elif args.step in ("dense", "queued"):
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
    ap.add_argument("--step", choices=[n for n, _ in STEPS + OWN_LEAF_STEPS])
    ap.add_argument("--own-leaf", action="store_true", help="measure the start hints of the queued query instead (own_leaf_rate_<height>p.json)")
    args = ap.parse_args()
    if args.step:
        return step(args)
    if args.own_leaf:
        return main_own_leaf(args)
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


def run_steps(args, steps, out):
    """every step as a process of its own under its time limit; False: a step failed and nothing was started after it"""
    for name, limit in steps:
        cmd = [sys.executable, os.path.abspath(__file__), "--step", name, "--width", str(args.width), "--height", str(args.height)]
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=limit)
        except subprocess.TimeoutExpired:
            out[name] = {"error": f"no result within {limit} s"}
            return False
        line = [ln for ln in r.stdout.splitlines() if ln.startswith("STEP ")]
        if r.returncode != 0 or not line:
            out[name] = {"error": f"exit status {r.returncode}", "stderr": r.stderr[-2000:]}
            return False
        out[name] = json.loads(line[-1][5:])
    return True


def main_own_leaf(args):
    out = {"what": "start hints of the queued occlusion query on the light rays of a frame's camera hits", "scene": "sponza_class", "width": args.width,
           "height": args.height, "spp": 1}
    ok = run_steps(args, OWN_LEAF_STEPS, out)
    if ok:
        o, r = out["own_leaf"], out["render_default"]
        out["device"], out["rtr_kernel_revision"] = o["device"], o["kernel_revision"]
        out["same_answers"] = o["occluded"]["queued"] == o["occluded"]["hinted"]
        out["hinted_over_queued_min"] = o["hinted"]["ms_min"] / o["queued"]["ms_min"]
        out["hinted_over_queued_median"] = o["hinted"]["ms_median"] / o["queued"]["ms_median"]
        out["hinted_over_render_default_min"] = o["hinted"]["ms_min"] / (r["shadow_gen_ms_min"] + r["shadow_trace_ms_min"])
        out["light_rays_hinted_over_plain_min"] = o["light_rays"]["hinted"]["ms_min"] / o["light_rays"]["plain"]["ms_min"]
        path = os.path.join(ROOT, "profiles", "occlusion", f"own_leaf_rate_{args.height}p.json")
        os.makedirs(os.path.dirname(path), exist_ok=True)
        with open(path, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")
    print(json.dumps(out))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
