"""What moving ONE object instance costs on the bench scene (sponza_class), synchronous against enqueued: one JSON line, also written to
profiles/instance_update/instance_update_rate.json.  One process, one stream (torch's, set as the context's):

  sync_wall_ms    wall time of one rtr_scene_update_instances (all instances from the host, one of them moved), the stream idle
                  before it
  async_host_ms   host time of one rtr_scene_update_instances_async (one record, the moved instance; the call returns with everything
                  enqueued)
  async_gpu_ms    GPU time of the enqueued chain (check, write, refit, 4-wide view, order, permutation, light triangles, status fold),
                  HIP events around the call on the stream

The three timings are taken five times each, interleaved, and the minimum is reported next to all five.  Every update moves the
scene's last object instance along a small circle, so both forms refit the same tree.

    python profiles/instance_update_rate.py [--width 1920 --height 1080]
"""
import argparse
import json
import math
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "instance_update", "instance_update_rate.json"))
    args = ap.parse_args()
    W, H = args.width, args.height
    torch.cuda.init()
    ctx = api.Context(0)
    stream = torch.cuda.Stream()          # a stream of its own: the default stream's handle (0) would give the context a new stream
    torch.cuda.set_stream(stream)
    ctx.set_stream(stream.cuda_stream)
    s = scenes.sponza_class(W, H)
    sync_scene, async_scene = api.Scene(ctx, s.desc), api.Scene(ctx, s.desc)
    async_scene.prepare_async_updates()
    st = sync_scene.stats()
    base = [A.RtrInstance.from_buffer_copy(bytes(i)) for i in s.host.instances()]
    which = len(base) - 1                 # an object instance: the lights come first
    assert base[which].customIndex >= s.desc.numLights
    m0 = np.array(base[which].transform[:], np.float32).reshape(3, 4)
    radius = 0.002 * float(np.linalg.norm(np.array(st.boundsMax[:]) - np.array(st.boundsMin[:])))
    phase = [0]

    def next_matrix():
        phase[0] += 1
        m = m0.copy()
        m[0, 3] += np.float32(radius * math.cos(0.3 * phase[0]))
        m[2, 3] += np.float32(radius * math.sin(0.3 * phase[0]))
        return m

    def sync_wall():
        inst = [A.RtrInstance.from_buffer_copy(bytes(i)) for i in base]
        for k, v in enumerate(next_matrix().reshape(-1)):
            inst[which].transform[k] = float(v)
        stream.synchronize()
        t0 = time.perf_counter()
        sync_scene.update_instances(inst)
        return (time.perf_counter() - t0) * 1e3

    def async_both():
        t = torch.from_numpy(next_matrix().reshape(1, 3, 4)).cuda()
        stream.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        t0 = time.perf_counter()
        async_scene.update_instances_async(t, first_instance=which)
        host = (time.perf_counter() - t0) * 1e3
        e1.record(stream)
        e1.synchronize()
        return host, e0.elapsed_time(e1)

    for _ in range(2):
        sync_wall(); async_both()
    sync_ms, host_ms, gpu_ms = [], [], []
    for _ in range(5):
        sync_ms.append(sync_wall())
        h, g = async_both()
        host_ms.append(h); gpu_ms.append(g)
    status = async_scene.update_status()
    out = {
        "what": "one object instance moved per update, synchronous vs enqueued", "scene": "sponza_class", "device": ctx.device_name(),
        "kernel_revision": A.hip_lib().rtr_kernel_revision().decode(),
        "width": W, "height": H, "triangles": int(st.numTriangles), "nodes": int(st.numNodes), "instances": len(base), "moved_instance": which,
        "sync_wall_ms": {"min": min(sync_ms), "all": sync_ms},
        "async_host_ms": {"min": min(host_ms), "all": host_ms},
        "async_gpu_ms": {"min": min(gpu_ms), "all": gpu_ms},
        "updates_enqueued": status.enqueued, "updates_refused": status.refused,
    }
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
