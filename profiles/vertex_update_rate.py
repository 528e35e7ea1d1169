"""What a vertex update costs (rtr_scene_update_vertices) on sponza_class: one JSON line, also written to
profiles/vertex_update/vertex_update_rate.json.  One process:

  (a) the call itself, wall clock (it is synchronous: it returns when the new state is complete), for
        one_mesh_host / one_mesh_device   the positions of the mesh with the most vertices, from numpy / from a torch device tensor
        all_host / all_device             the positions of every vertex
        update_instances                  rtr_scene_update_instances with unchanged transforms: the refit the calls share
      five repeats, interleaved, the minimum taken; every repeat writes the same deformed positions, so the work is the same.
      The split: shared refit = update_instances; staging + check + write kernels (+ the light-triangle table, which a vertex update
      always remakes) = the call minus that.
  (b) the frame bench.py renders (1920x1080, 1 spp, 3 shadow rays, timed kernels): rtr_frame_stats.totalMs, minimum of five, on the
      scene before the deformation, after it (the refitted tree), and on a scene freshly built from the deformed vertices — what the
      refit costs in tree quality.

The deformation: every object vertex moved along its normal by 1 % of the scene's diagonal times a sine of its position.

    python profiles/vertex_update_rate.py [--width 1920 --height 1080]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from realtimeraytracer_amd import _abi as A  # noqa: E402
from realtimeraytracer_amd import api, scenes  # noqa: E402


def wall_ms(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


def five_each(fns):
    """the repeats of several calls interleaved, so that a drift of the clocks is in all of them alike"""
    for fn in fns.values():
        fn()                               # warm-up: first-use allocations (staging buffer, refit arrays) are not part of the rate
    ms = {k: [] for k in fns}
    for _ in range(5):
        for k, fn in fns.items():
            ms[k].append(wall_ms(fn))
    return {k: {"ms_min": min(v), "ms_all": v} for k, v in ms.items()}


def frame_ms(ctx, scene, s, p):
    frame = api.Frame(ctx, p.width, p.height)
    ms = []
    for k in range(7):
        api.render(scene, s.camera, s.scene_info(k), p, frame)
        ms.append(frame.stats().totalMs)
    frame.close()
    return {"ms_min": min(ms[2:]), "ms_all": ms[2:]}


def deformed(d, strength):
    """(the description's vertices as (n, 12) float32, the same with every object vertex moved along its normal by `strength` x the
    scene's diagonal x a sine of its position, [(first vertex, count) of the object meshes]); profiles/rebuild_rate.py sweeps strength"""
    n = d.numVertices
    old = np.ctypeslib.as_array(C.cast(d.vertices, C.POINTER(C.c_float)), (n, 12)).copy()
    light_meshes = {d.instances[i].meshIndex for i in range(d.numInstances) if d.instances[i].customIndex < d.numLights}
    diag = float(np.linalg.norm(old[:, 0:3].max(0).astype(np.float64) - old[:, 0:3].min(0)))
    new = old.copy()
    meshes = [(int(d.meshes[m].vertexOffset), int(d.meshes[m].vertexCount)) for m in range(d.numMeshes) if m not in light_meshes]
    for first, count in meshes:
        p, nrm = old[first:first + count, 0:3].astype(np.float64), old[first:first + count, 4:7].astype(np.float64)
        phase = p @ np.array([1.0, 1.7, 0.6]) * (2 * np.pi * 4 / diag)
        new[first:first + count, 0:3] = (p + strength * diag * np.sin(phase)[:, None] * nrm).astype(np.float32)
    assert (new[:, 0:3] != old[:, 0:3]).any(), "the scene stores no normals to deform along"
    return old, new, meshes


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--out", default=None, help="where the JSON goes (default profiles/vertex_update/vertex_update_rate.json)")
    args = ap.parse_args()
    W, H = args.width, args.height
    torch.cuda.init()
    ctx = api.Context(0)
    s = scenes.sponza_class(W, H)
    d = s.desc
    n = d.numVertices
    old, new, meshes = deformed(d, 0.01)
    big_first, big_count = max(meshes, key=lambda m: m[1])

    scene = api.Scene(ctx, d)
    st = scene.stats()
    out = {"what": "cost of rtr_scene_update_vertices and of the refitted tree", "scene": "sponza_class", "width": W, "height": H,
           "device": ctx.device_name(), "kernel_revision": A.hip_lib().rtr_kernel_revision().decode(),
           "num_vertices": int(n), "num_triangles": int(st.numTriangles), "one_mesh_vertices": big_count,
           "deformation": "object vertices along their normals, 0.01 x scene diagonal x sin(position)", "timing": "wall clock around the synchronous call, min of 5 interleaved repeats"}
    p = api.make_params(W, H, spp=1, shadow_rays=3)
    out["frame_before"] = frame_ms(ctx, scene, s, p)

    one_h = np.ascontiguousarray(new[big_first:big_first + big_count, 0:3])
    all_h = np.ascontiguousarray(new[:, 0:3])
    one_d, all_d = torch.from_numpy(one_h).cuda(), torch.from_numpy(all_h).cuda()
    torch.cuda.synchronize()
    inst = [A.RtrInstance.from_buffer_copy(bytes(i)) for i in s.host.instances()]
    calls = {
        "one_mesh_host": lambda: scene.update_vertices([(big_first, one_h)]),
        "one_mesh_device": lambda: scene.update_vertices([(big_first, one_d)]),
        "all_host": lambda: scene.update_vertices([(0, all_h)]),
        "all_device": lambda: scene.update_vertices([(0, all_d)]),
        "update_instances": lambda: scene.update_instances(inst),
    }
    out["calls"] = five_each(calls)
    refit = out["calls"]["update_instances"]["ms_min"]
    out["split_ms"] = {k: {"shared_refit": refit, "staging_check_write_and_light_table": out["calls"][k]["ms_min"] - refit}
                      for k in calls if k != "update_instances"}
    out["vertices_per_second_all_device"] = n / (out["calls"]["all_device"]["ms_min"] * 1e-3)

    assert np.array_equal(scene.export_vertices(raw=True)[:, 0:3], new[:, 0:3])
    out["frame_after_refit"] = frame_ms(ctx, scene, s, p)
    d2 = A.rtr_scene_desc.from_buffer_copy(bytes(d))
    arr = (A.RtrVertex * n).from_buffer_copy(new.tobytes())
    d2.vertices = C.cast(arr, C.POINTER(A.RtrVertex))
    fresh = api.Scene(ctx, d2)
    out["frame_fresh_build"] = frame_ms(ctx, fresh, s, p)
    out["fresh_build_ms"] = float(fresh.stats().buildMs)
    out["refit_over_fresh_frame"] = out["frame_after_refit"]["ms_min"] / out["frame_fresh_build"]["ms_min"]

    line = json.dumps(out)
    print(line)
    path = args.out or os.path.join(ROOT, "profiles", "vertex_update", "vertex_update_rate.json")
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
