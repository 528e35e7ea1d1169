"""What a device rebuild costs on the bench scene (sponza_class, built with RTR_BUILD_DEVICE_LBVH), synchronous against enqueued: one
JSON line, also written to profiles/rebuild/rebuild_async_rate.json.  One process, one stream (torch's, set as the context's):

  sync_wall_ms     wall time of one rtr_scene_rebuild(RTR_BUILD_DEVICE_LBVH), the stream idle before it
  async_host_ms    host time of one rtr_scene_rebuild_async (the call returns with everything enqueued)
  async_gpu_ms     GPU time of the enqueued chain (device build into the stage, commit, 4-wide view, order, permutation, status fold),
                   HIP events around the call on the stream
  commit_gpu_ms    k_commit_tree alone, from the kernel records of torch's profiler around enqueued rebuilds ("not measured" where the
                   profiler is not available); chain_kernels_ms lists every kernel of the chain the same way
  prepare_bytes    device memory rtr_scene_prepare_async_rebuild took (stage + build scratch + the enqueued updates' tables), from the
                   free-memory figure before and after it; per triangle beside it

The timings are taken five times each, interleaved, and the minimum is reported next to all five.  Between rebuilds both scenes take
the same small deformation of one object mesh, so each rebuild has a new tree to build.

    python profiles/rebuild_async_rate.py [--width 1920 --height 1080]
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rebuild", "rebuild_async_rate.json"))
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
    sync_scene, async_scene = api.Scene(ctx, desc), api.Scene(ctx, desc)
    stream.synchronize()
    free0 = torch.cuda.mem_get_info()[0]
    async_scene.prepare_async_rebuild()
    stream.synchronize()
    prepare_bytes = free0 - torch.cuda.mem_get_info()[0]
    st = sync_scene.stats()

    n = desc.numVertices
    base = np.ctypeslib.as_array(C.cast(desc.vertices, C.POINTER(C.c_float)), (n, 12))[:, 0:3].copy()
    me = desc.meshes[desc.instances[desc.numInstances - 1].meshIndex]          # the last object instance's mesh
    first, count = int(me.vertexOffset), int(me.vertexCount)
    diag = float(np.linalg.norm(base.max(0) - base.min(0)))
    phase = [0]

    def next_positions():
        phase[0] += 1
        p = base[first:first + count].copy()
        p[:, 1] += np.float32(0.01 * diag) * np.sin(p[:, 0] * np.float32(20.0 / diag) + np.float32(0.7 * phase[0])).astype(np.float32)
        return p

    def deform():
        p = next_positions()
        sync_scene.update_vertices([(first, p)])
        async_scene.update_vertices_async([(first, torch.from_numpy(p).cuda())])
        stream.synchronize()

    def sync_wall():
        stream.synchronize()
        t0 = time.perf_counter()
        sync_scene.rebuild("device")
        return (time.perf_counter() - t0) * 1e3

    def async_both():
        stream.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        t0 = time.perf_counter()
        async_scene.rebuild_async()
        host = (time.perf_counter() - t0) * 1e3
        e1.record(stream)
        e1.synchronize()
        return host, e0.elapsed_time(e1)

    for _ in range(2):
        deform(); sync_wall(); async_both()
    sync_ms, host_ms, gpu_ms = [], [], []
    for _ in range(5):
        deform()
        sync_ms.append(sync_wall())
        h, g = async_both()
        host_ms.append(h); gpu_ms.append(g)

    commit_ms, kernels = "not measured", "not measured"
    try:
        from torch.profiler import ProfilerActivity, profile
        stream.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            for _ in range(5):
                async_scene.rebuild_async()
                stream.synchronize()
        by_name = {}
        for e in prof.events():
            t = float(getattr(e, "device_time", 0.0) or getattr(e, "cuda_time", 0.0)) * 1e-3
            if t > 0.0:
                by_name.setdefault(e.name.split("(")[0], []).append(t)
        found = [v for k, v in by_name.items() if "k_commit_tree" in k]
        if found:
            commit_ms = min(found[0])
            kernels = {k: {"min": min(v), "launches_per_call": len(v) / 5.0} for k, v in sorted(by_name.items())}
    except Exception as exc:      # the profiler is optional: the other numbers stand without it
        commit_ms = f"not measured ({type(exc).__name__})"

    status = async_scene.update_status()
    same = bytes(async_scene.export_bvh()[0]) == bytes(sync_scene.export_bvh()[0])
    out = {
        "what": "device rebuild of the bench scene, synchronous vs enqueued", "scene": "sponza_class (RTR_BUILD_DEVICE_LBVH)", "device": ctx.device_name(),
        "kernel_revision": A.hip_lib().rtr_kernel_revision().decode(),
        "width": W, "height": H, "triangles": int(st.numTriangles), "nodes": int(st.numNodes), "max_depth": int(async_scene.stats().maxDepth),
        "stack_entries": int(async_scene.stats().stackEntries),
        "sync_wall_ms": {"min": min(sync_ms), "all": sync_ms},
        "async_host_ms": {"min": min(host_ms), "all": host_ms},
        "async_gpu_ms": {"min": min(gpu_ms), "all": gpu_ms},
        "commit_gpu_ms": commit_ms,
        "commit_small_beside_the_chain": (commit_ms < 0.1 * min(gpu_ms)) if isinstance(commit_ms, float) else "not measured",
        "chain_kernels_ms": kernels,
        "prepare_bytes": int(prepare_bytes), "prepare_bytes_per_triangle": prepare_bytes / float(st.numTriangles),
        "updates_enqueued": status.enqueued, "updates_refused": status.refused, "same_nodes_as_the_synchronous_scene": same,
    }
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
