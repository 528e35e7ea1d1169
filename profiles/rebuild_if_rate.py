"""What the rebuild policy on the device costs on the bench scene (sponza_class, built with RTR_BUILD_DEVICE_LBVH): one JSON line, also
written to profiles/rebuild/rebuild_if_rate.json.  One process, one stream (torch's, set as the context's), ONE scene, so the yardstick —
rtr_scene_rebuild_async's chain — is measured in the same run at the same commit:

  if_host_ms          host time of one rtr_scene_rebuild_if_async (the call returns with everything enqueued); skipped and built apart
  skipped_gpu_ms      GPU time of a SKIPPED chain (rebuild_above = inf): cost kernel, decision, the gated launches that return at once,
                      and what is not gated — the memsets of stage and scratch arrays and the radix sort of the scratch keys
  built_gpu_ms        GPU time of a BUILT chain (rebuild_above = 0): the above plus the build, the commit, the tail and the close
  unconditional_gpu_ms  GPU time of rtr_scene_rebuild_async's chain on the same (policy-prepared) scene
  skipped_over_unconditional   the ratio of the minima: what a frame that does not rebuild pays, in units of a blind rebuild
  skipped_kernels_ms  every kernel and memset of a skipped chain from torch's profiler ("not measured" where it is not available):
                      ungated_share_of_skipped is the share of the sort and the memsets in it

HIP events around the call on the stream; each timing is taken five times, interleaved, and the minimum is reported next to all five.
Between rounds the scene takes a small deformation of one object mesh, so each build has a new tree to build.

    python profiles/rebuild_if_rate.py [--width 1920 --height 1080]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rebuild", "rebuild_if_rate.json"))
    args = ap.parse_args()
    W, H = args.width, args.height
    torch.cuda.init()
    ctx = api.Context(0)
    stream = torch.cuda.Stream()          # a stream of its own: the default stream's handle (0) would give the context a new stream
    torch.cuda.set_stream(stream)
    ctx.set_stream(stream.cuda_stream)
    s = scenes.sponza_class(W, H)
    desc = A.rtr_scene_desc.from_buffer_copy(bytes(s.desc))
    desc.buildFlags = A.BUILD_DEVICE_LBVH
    scene = api.Scene(ctx, desc)
    scene.prepare_async_rebuild_if()
    stream.synchronize()
    st = scene.stats()

    n = desc.numVertices
    base = np.ctypeslib.as_array(C.cast(desc.vertices, C.POINTER(C.c_float)), (n, 12))[:, 0:3].copy()
    me = desc.meshes[desc.instances[desc.numInstances - 1].meshIndex]          # the last object instance's mesh
    first, count = int(me.vertexOffset), int(me.vertexCount)
    diag = float(np.linalg.norm(base.max(0) - base.min(0)))
    phase = [0]

    def deform():
        phase[0] += 1
        p = base[first:first + count].copy()
        p[:, 1] += np.float32(0.01 * diag) * np.sin(p[:, 0] * np.float32(20.0 / diag) + np.float32(0.7 * phase[0])).astype(np.float32)
        scene.update_vertices_async([(first, torch.from_numpy(p).cuda())])
        stream.synchronize()

    def timed(call):
        stream.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        t0 = time.perf_counter()
        call()
        host = (time.perf_counter() - t0) * 1e3
        e1.record(stream)
        e1.synchronize()
        return host, e0.elapsed_time(e1)

    calls = {"skipped": lambda: scene.rebuild_if_async(float("inf")), "built": lambda: scene.rebuild_if_async(0.0), "unconditional": scene.rebuild_async}
    for _ in range(2):
        for call in calls.values():
            deform(); timed(call)
    host_ms, gpu_ms = {k: [] for k in calls}, {k: [] for k in calls}
    before = scene.rebuild_if_status()
    for _ in range(5):
        for k, call in calls.items():
            deform()
            h, g = timed(call)
            host_ms[k].append(h); gpu_ms[k].append(g)
    after = scene.rebuild_if_status()

    kernels, ungated = "not measured", "not measured"
    try:
        from torch.profiler import ProfilerActivity, profile
        stream.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            for _ in range(5):
                scene.rebuild_if_async(float("inf"))
                stream.synchronize()
        by_name = {}
        for e in prof.events():
            t = float(getattr(e, "device_time", 0.0) or getattr(e, "cuda_time", 0.0)) * 1e-3
            if t > 0.0:
                by_name.setdefault(e.name.split("(")[0], []).append(t)
        if by_name:
            kernels = {k: {"min": min(v), "launches_per_call": len(v) / 5.0, "sum_per_call": sum(v) / 5.0} for k, v in sorted(by_name.items())}
            total = sum(v["sum_per_call"] for v in kernels.values())
            ours = sum(v["sum_per_call"] for k, v in kernels.items() if "rtrdev" in k or k.startswith("k_"))
            ungated = {"sum_of_records_ms": total, "project_kernels_ms": ours, "sort_and_memsets_ms": total - ours, "share": (total - ours) / total if total else 0.0}
    except Exception as exc:      # the profiler is optional: the other numbers stand without it
        kernels = f"not measured ({type(exc).__name__})"

    status = scene.update_status()
    skipped, built, uncond = min(gpu_ms["skipped"]), min(gpu_ms["built"]), min(gpu_ms["unconditional"])
    out = {
        "what": "the rebuild policy on the device, bench scene: a skipped chain, a built chain, and rtr_scene_rebuild_async's chain in the same run",
        "scene": "sponza_class (RTR_BUILD_DEVICE_LBVH)", "device": ctx.device_name(), "kernel_revision": A.hip_lib().rtr_kernel_revision().decode(),
        "width": W, "height": H, "triangles": int(st.numTriangles), "nodes": int(st.numNodes),
        "if_host_ms": {"skipped": {"min": min(host_ms["skipped"]), "all": host_ms["skipped"]}, "built": {"min": min(host_ms["built"]), "all": host_ms["built"]}},
        "unconditional_host_ms": {"min": min(host_ms["unconditional"]), "all": host_ms["unconditional"]},
        "skipped_gpu_ms": {"min": skipped, "all": gpu_ms["skipped"]},
        "built_gpu_ms": {"min": built, "all": gpu_ms["built"]},
        "unconditional_gpu_ms": {"min": uncond, "all": gpu_ms["unconditional"]},
        "skipped_over_unconditional": skipped / uncond, "built_over_unconditional": built / uncond,
        "skipped_kernels_ms": kernels, "ungated_share_of_skipped": ungated,
        "decisions_in_the_timed_rounds": {"evaluated": after.evaluated - before.evaluated, "rebuilt": after.rebuilt - before.rebuilt},
        "updates_enqueued": status.enqueued, "updates_refused": status.refused,
    }
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
