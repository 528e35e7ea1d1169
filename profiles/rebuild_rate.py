"""What a rebuild costs and what it wins (rtr_scene_rebuild, rtr_scene_tree_cost) on sponza_class: one JSON line, also written to
profiles/rebuild/rebuild_rate.json.  One process, a sweep of deformation strengths — the deformation of profiles/vertex_update_rate.py
(every object vertex along its normal by strength x the scene's diagonal x a sine of its position), at 0.01 (that script's), and around it.

For every strength, on a scene created with the device builder and deformed by one rtr_scene_update_vertices:
  tree_cost        rtr_scene_tree_cost after the refit, after a device rebuild, after a host rebuild (sah and the integer sums)
  frame_ms         the frame bench.py renders (1 spp, 3 shadow rays, timed kernels: rtr_frame_stats.totalMs) on each of the three trees
  rebuild_ms       wall clock around rtr_scene_rebuild, device and host (synchronous calls), and around the parent commit's way to the
                   same tree: rtr_scene_destroy + rtr_scene_create of the same vertices with the device builder
  tree_cost_ms     wall clock around rtr_scene_tree_cost (kernel + the join of the scene's stream)
Repeats are interleaved and the minimum of five is taken (the three trees cannot live in one scene, so the frame times come from three
scenes that hold the refitted, the device-rebuilt and the host-rebuilt tree of the same vertices; a rebuild is timed by rebuilding those
again: the same work every time).  Whether sah tracks the frame time of the 4-wide walk is what the file is for: sah_vs_frame lists the
pairs, normalised to the device-rebuilt tree of each strength.

    python profiles/rebuild_rate.py [--width 1920 --height 1080 --strengths 0.0025,0.01,0.04,0.16]
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from realtimeraytracer_amd import _abi as A  # noqa: E402
from realtimeraytracer_amd import api, scenes  # noqa: E402
from vertex_update_rate import deformed, wall_ms  # noqa: E402


def interleaved(fns, repeats=5):
    """one warm-up each, then the repeats of all of them in turn; the minimum and every value"""
    for fn in fns.values():
        fn()
    vals = {k: [] for k in fns}
    for _ in range(repeats):
        for k, fn in fns.items():
            vals[k].append(fn())
    return {k: {"ms_min": min(v), "ms_all": v} for k, v in vals.items()}


def cost_dict(c):
    return {"sah": c.sah, "inner_area": list(c.inner_area), "leaf_area": list(c.leaf_area), "root_area": list(c.root_area),
            "num_inner": c.num_inner, "num_leaf_refs": c.num_leaf_refs}


def with_vertices(d, v12, flags):
    d2 = A.rtr_scene_desc.from_buffer_copy(bytes(d))
    arr = (A.RtrVertex * len(v12)).from_buffer_copy(np.ascontiguousarray(v12, np.float32).tobytes())
    d2.vertices = C.cast(arr, C.POINTER(A.RtrVertex))
    d2.buildFlags = flags
    d2._keep = arr
    return d2


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--strengths", default="0.0025,0.01,0.04,0.16")
    ap.add_argument("--out", default=None, help="where the JSON goes (default profiles/rebuild/rebuild_rate.json)")
    args = ap.parse_args()
    W, H = args.width, args.height
    torch.cuda.init()
    ctx = api.Context(0)
    s = scenes.sponza_class(W, H)
    d = s.desc
    p = api.make_params(W, H, spp=1, shadow_rays=3)
    out = {"what": "cost of rtr_scene_rebuild / rtr_scene_tree_cost and of the trees they leave", "scene": "sponza_class", "width": W, "height": H,
           "device": ctx.device_name(), "kernel_revision": A.hip_lib().rtr_kernel_revision().decode(),
           "num_vertices": int(d.numVertices), "deformation": "object vertices along their normals, strength x scene diagonal x sin(position)",
           "timing": "min of 5 interleaved repeats; calls: wall clock around the synchronous call; frames: rtr_frame_stats.totalMs", "steps": []}
    frame = api.Frame(ctx, W, H)

    def frame_of(scene):
        def run():
            api.render(scene, s.camera, s.scene_info(3), p, frame)
            return float(frame.stats().totalMs)
        return run

    dev_flags = with_vertices(d, deformed(d, 0.01)[0], A.BUILD_DEVICE_LBVH)      # the undeformed vertices, device builder
    for strength in [float(x) for x in args.strengths.split(",")]:
        old, new, _ = deformed(d, strength)
        pos = np.ascontiguousarray(new[:, 0:3])
        trees = {}
        for k in ("refit", "device_rebuild", "host_rebuild"):
            trees[k] = api.Scene(ctx, dev_flags)
            trees[k].update_vertices([(0, pos)])
        trees["device_rebuild"].rebuild("device")
        trees["host_rebuild"].rebuild("host")
        step = {"strength": strength, "num_triangles": int(trees["refit"].stats().numTriangles),
                "tree_cost": {k: cost_dict(sc.tree_cost()) for k, sc in trees.items()}}
        step["frame_ms"] = interleaved({k: frame_of(sc) for k, sc in trees.items()})
        fresh_desc = with_vertices(d, new, A.BUILD_DEVICE_LBVH)
        holder = {"scene": api.Scene(ctx, fresh_desc)}

        def destroy_and_create():
            holder["scene"].close()
            holder["scene"] = api.Scene(ctx, fresh_desc)

        step["rebuild_ms"] = interleaved({"device": lambda: wall_ms(lambda: trees["device_rebuild"].rebuild("device")),
                                          "host": lambda: wall_ms(lambda: trees["host_rebuild"].rebuild("host")),
                                          "destroy_and_create_device": lambda: wall_ms(destroy_and_create)})
        step["tree_cost_ms"] = interleaved({"tree_cost": lambda: wall_ms(trees["refit"].tree_cost)})["tree_cost"]
        base_sah, base_ms = step["tree_cost"]["device_rebuild"]["sah"], step["frame_ms"]["device_rebuild"]["ms_min"]
        step["sah_vs_frame"] = {k: {"sah_ratio": step["tree_cost"][k]["sah"] / base_sah, "frame_ratio": step["frame_ms"][k]["ms_min"] / base_ms} for k in trees}
        out["steps"].append(step)
        holder["scene"].close()
        for sc in trees.values():
            sc.close()

    line = json.dumps(out)
    print(line)
    path = args.out or os.path.join(ROOT, "profiles", "rebuild", "rebuild_rate.json")
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
