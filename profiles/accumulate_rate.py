"""Path-accumulation rates (rtr_accumulate_paths, rtr_gather_records) on sponza_class at 1920x1080, 1 spp — the bench frame's 2 073 600
camera hits — and what the library route does to the composed path tracer: one JSON object, printed and written to
profiles/accumulate/accumulate_rate_1080p.json.

  accumulate_paths  k_accumulate_paths on the frame's depth-0 records with EVERY optional array: the RtrRadiance of direct_light, a packed
                    throughput, ids (a random permutation: the worst scatter; the identity; and the ids of a compaction, in order with
                    RTR_PATH_NONE behind the survivors), RtrEmitter and RtrSkyEscape records, the 16-B sky sums, the RtrBounce records, outTerm and
                    outThroughput, both flags set; and with no optional array
  gather_records    k_gather_records on the RtrSurface records (80 B) by the ids of a compaction of the depth-0 bounce
  compact_paths, bounce_rays   on the same paths, the streaming kernels to compare against
  path_trace        the wall time of api.path_trace_power as the PARENT commit builds it (--parent-root: a checkout of the parent with
                    its library built; run twice, so that its own spread is known) against api.path_trace_library(loop="power") of
                    this tree, at 1, 2 and 4 bounces, plain and with compact=True, roulette_from=1.  Each side runs in a process of
                    its own (a fresh child: parent, this tree, parent again), five interleaved repeats of the six cases in each.

The kernels are enqueued through the C ABI directly on preallocated outputs (the timing is of the kernels, not of Python), HIP events
on the context's stream, which is torch's current stream; three warm-up launches, then at least 0.2 s of timed launches per repeat; the
five repeats of the cases are interleaved and the minimum is reported beside the median and all five.

    python profiles/accumulate_rate.py [--parent-root DIR] [--width 1920 --height 1080] [--out profiles/accumulate/accumulate_rate_1080p.json]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

BYTES_ALL = 16 + 12 + 4 + 16 + 16 + 32 + 12 + 12 + 12 + 12       # radiance, T, id, sky sum, bounce, emitter or escape (at most), accum in and out, outTerm, outThroughput
BYTES_NONE = 16 + 12 + 12 + 12                                     # radiance, T, accum in and out


def five_each(fns):
    """the repeats of several loops interleaved, so that a drift of the clock is in all of them alike"""
    ms = {k: [] for k in fns}
    for _ in range(5):
        for k, fn in fns.items():
            ms[k].append(fn())
    return {k: {"ms_min": min(v), "ms_median": statistics.median(v), "ms_all": v} for k, v in ms.items()}


def wall(root, which, W, H):
    """role of a child process: the six path-trace cases of one side, five interleaved repeats -> JSON on the last line"""
    sys.path.insert(0, root)             # the package of that checkout, and nothing of this one
    import torch
    from realtimeraytracer_amd import _abi as A
    from realtimeraytracer_amd import api, scenes
    torch.cuda.init()
    ctx = api.Context(0)
    s = scenes.sponza_class(W, H)
    scene = api.Scene(ctx, s.desc)
    rays = api.camera_rays(ctx, s.camera, W, H, 1)
    lp = api.make_light_params(s.num_lights, 3, 0, W, 1, A.LIGHT_SHADOWED)
    live = {}

    def path(bounces, **kw):
        def run():
            torch.cuda.synchronize()
            t = time.perf_counter()
            res = api.path_trace_library(scene, rays, lp, bounces, loop="power", **kw) if which == "library" else api.path_trace_power(scene, rays, lp, bounces, **kw)
            torch.cuda.synchronize()
            if res.live is not None:
                live[f"bounces_{bounces}"] = res.live
            return (time.perf_counter() - t) * 1e3
        return run
    cases = {}
    for bounces in (1, 2, 4):
        cases[f"bounces_{bounces}_plain"] = path(bounces)
        cases[f"bounces_{bounces}_compact_roulette_from_1"] = path(bounces, compact=True, roulette_from=1)
    for fn in cases.values():
        fn()                                                                      # warm-up: every shape once
    out = {"wall": five_each(cases), "live": live, "package": os.path.dirname(os.path.abspath(api.__file__))}
    scene.close()
    ctx.close()
    print(json.dumps(out))


def child(root, which, W, H):
    cmd = [sys.executable, os.path.abspath(__file__), "--role", which, "--root", root, "--width", str(W), "--height", str(H)]
    text = subprocess.run(cmd, check=True, stdout=subprocess.PIPE, timeout=300).stdout.decode()
    return json.loads(text.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "accumulate", "accumulate_rate_1080p.json"))
    ap.add_argument("--parent-root", default=None, help="a checkout of the parent commit with its library built; without it the path-trace comparison is left out")
    ap.add_argument("--role", default=None, choices=["power", "library"])
    ap.add_argument("--root", default=ROOT)
    args = ap.parse_args()
    W, H = args.width, args.height
    if args.role:
        return wall(args.root, args.role, W, H)

    out = {"what": "path-accumulation rates", "scene": "sponza_class", "width": W, "height": H, "spp": 1, "paths": W * H}
    if args.parent_root:                 # before this process opens the device: one process on the GPU at a time
        sides = {"parent_first": child(args.parent_root, "power", W, H), "library": child(ROOT, "library", W, H), "parent_second": child(args.parent_root, "power", W, H)}
        assert os.path.abspath(sides["parent_first"]["package"]).startswith(os.path.abspath(args.parent_root)), sides["parent_first"]["package"]
        out["path_trace_wall"] = {k: v["wall"] for k, v in sides.items()}
        out["path_trace_live"] = {k: v["live"] for k, v in sides.items()}
        cmp = {}
        for case in sides["library"]["wall"]:
            a, b, l = (sides[k]["wall"][case]["ms_min"] for k in ("parent_first", "parent_second", "library"))
            cmp[case] = {"parent_ms_min": min(a, b), "parent_spread_ms": abs(a - b), "library_ms_min": l, "library_over_parent": l / min(a, b),
                         "faster_by_more_than_the_parents_spread": bool(min(a, b) - l > abs(a - b))}
        out["library_against_parent"] = cmp

    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "profiles"))
    import torch
    from realtimeraytracer_amd import _abi as A
    from realtimeraytracer_amd import api, scenes
    from query_rate import timed
    torch.cuda.init()
    ctx = api.Context(0)
    stream = torch.cuda.Stream()          # a stream of its own: the default stream's handle (0) would give the context a new stream
    torch.cuda.set_stream(stream)
    ctx.set_stream(stream.cuda_stream)
    s = scenes.sponza_class(W, H)
    scene = api.Scene(ctx, s.desc)
    lib, n = ctx.lib, W * H
    out.update({"device": ctx.device_name(), "kernel_revision": A.hip_lib().rtr_kernel_revision().decode()})

    rays = api.camera_rays(ctx, s.camera, W, H, 1)
    hits = api.trace_rays(scene, rays)
    surf = api.hit_surfaces(scene, rays, hits).raw
    lp = api.make_light_params(s.num_lights, 3, 0, W, 1, A.LIGHT_SHADOWED)
    bp = api.make_bounce_params(frame=0, depth=0, width=W, spp=1)
    lit = api.direct_light(scene, rays, hits, lp, ctx=ctx).raw
    b = api.bounce_rays(ctx, rays, surf, bp)
    dev = rays.device
    k = torch.arange(n, device=dev, dtype=torch.int64)
    seeds = api._wrap32((k % W) * 733 + (k // W) * 1933)
    ids = torch.randperm(n, device=dev).to(torch.int32)                # the scatter of a frame after compactions: every slot once, in no order
    ident = torch.arange(n, device=dev, dtype=torch.int32)
    T = torch.rand((n, 3), device=dev)
    emit, esc = torch.rand((n, 8), device=dev), torch.rand((n, 8), device=dev)
    sums = torch.rand((n, 4), device=dev)
    accum, term, out_t = torch.zeros((n, 3), device=dev), torch.zeros((n, 3), device=dev), torch.empty((n, 3), device=dev)
    kinds = lit.view(torch.int32)[:, 3]
    out["kinds"] = {name: int((kinds == v).sum()) for name, v in (("miss", A.SURFACE_MISS), ("object", A.SURFACE_OBJECT), ("light", A.SURFACE_LIGHT))}
    nbytes = api.compact_scratch_bytes(lib, n)
    scratch = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    o_rays, o_t = torch.empty((n, 8), device=dev), torch.empty((n, 3), device=dev)
    o_seeds, o_ids = torch.empty_like(seeds), torch.empty_like(ident)
    count = torch.zeros(1, dtype=torch.int32, device=dev)
    out_rays2, out_b2 = torch.empty_like(b.rays), torch.empty_like(b.raw)
    gathered = torch.empty_like(surf)
    cp = api.make_compact_params(frame=0, depth=0, throughput_stride=32)
    p_all, p_none = api.make_accum_params(n, True, True), api.make_accum_params(n)
    torch.cuda.synchronize()

    def vp(x):
        return A.VP(x.data_ptr()) if x is not None else None

    def accumulate(full, path_ids):
        def run():
            if full:
                return lib.rtr_accumulate_paths_async(ctx.h, vp(lit), vp(T), vp(path_ids), vp(emit), vp(esc), vp(sums), vp(b.raw), n, C.byref(p_all), vp(accum), vp(term),
                                                      vp(out_t))
            return lib.rtr_accumulate_paths_async(ctx.h, vp(lit), vp(T), None, None, None, None, None, n, C.byref(p_none), vp(accum), None, None)
        return run

    def compact():
        return lib.rtr_compact_paths_async(ctx.h, vp(b.rays), vp(b.raw), vp(seeds), vp(ident), n, C.byref(cp), vp(scratch), nbytes, vp(o_rays), vp(o_t), vp(o_seeds),
                                           vp(o_ids), vp(count))

    def bounce():
        return lib.rtr_bounce_rays_async(ctx.h, vp(rays), vp(surf), n, C.byref(bp), None, vp(out_rays2), vp(out_b2))

    def gather():
        return lib.rtr_gather_records_async(ctx.h, vp(surf), 80, n, vp(o_ids), n, vp(gathered))

    assert compact() == 0, lib.rtr_last_error()                        # o_ids: the survivors' ids in order, RTR_PATH_NONE behind them
    fns = {"accumulate_paths_all_arrays": accumulate(True, ids), "accumulate_paths_all_arrays_identity_ids": accumulate(True, ident),
           "accumulate_paths_all_arrays_compacted_ids": accumulate(True, o_ids),
           "accumulate_paths_no_optional_array": accumulate(False, None), "compact_paths": compact, "gather_records_80": gather, "bounce_rays": bounce}
    for name, fn in fns.items():
        assert fn() == 0, (name, lib.rtr_last_error())
    torch.cuda.synchronize()
    live = int(count.item())
    out["survivors_of_the_depth_0_bounce"] = live
    kern = five_each({name: (lambda f=fn: timed(f)[0]) for name, fn in fns.items()})
    moved = {"accumulate_paths_all_arrays": n * BYTES_ALL, "accumulate_paths_all_arrays_identity_ids": n * BYTES_ALL, "accumulate_paths_no_optional_array": n * BYTES_NONE,
             "accumulate_paths_all_arrays_compacted_ids": n * (BYTES_ALL - 36) + live * 36, "gather_records_80": n * (4 + 80) + live * 80}
    for name, v in kern.items():
        v["mpaths_s"] = n / v["ms_min"] / 1e3
        if name in moved:
            v["bytes_per_path"] = moved[name] / n
            v["gb_s"] = moved[name] / v["ms_min"] / 1e6
    out["kernels"] = kern
    out["accumulate_over_compact_paths"] = kern["accumulate_paths_all_arrays"]["ms_min"] / kern["compact_paths"]["ms_min"]
    ctx.set_stream(None)
    text = json.dumps(out, indent=1)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
