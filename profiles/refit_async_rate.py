"""What a vertex update costs between two frames of the bench scene (sponza_class), synchronous against enqueued: one JSON line, also
written to profiles/vertex_update/refit_async_rate.json.  One process, one stream (torch's, set as the context's):

  sync_wall_ms       wall time of one rtr_scene_update_vertices (device tensors), the stream idle before it
  async_host_ms      host time of one rtr_scene_update_vertices_async (the call returns with everything enqueued)
  async_gpu_ms       GPU time of the enqueued chain, HIP events around the call on the stream
  wide_order_gpu_ms  k_wide_order alone, from the kernel records of torch's profiler around one enqueued update ("not measured" where
                     the profiler does not see the library's kernels)
  fps_sync, fps_async  frames per second of the loop "torch deformation -> update -> rtr_render_async" with each form, joined once
                     at the end (the synchronous update joins by itself every frame)

The three timings are taken five times each, interleaved, and the minimum is reported next to all five.  Every update writes every
vertex of the scene (one range), a sine wave whose phase moves from call to call.

    python profiles/refit_async_rate.py [--width 1920 --height 1080 --frames 60]
"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from realtimeraytracer_amd import api, scenes  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--frames", type=int, default=60)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "vertex_update", "refit_async_rate.json"))
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
    base = torch.from_numpy(sync_scene.export_vertices(raw=True)[:, 0:3].copy()).cuda()
    amp = 0.002 * float((base.max(0).values - base.min(0).values).max())

    def deform(k):
        out = base.clone()
        out[:, 1] += amp * torch.sin(base[:, 0] * 0.05 + 0.3 * k)
        return out

    phase = [0]

    def next_positions():
        phase[0] += 1
        return deform(phase[0])

    def sync_wall():
        pos = next_positions()
        stream.synchronize()
        t0 = time.perf_counter()
        sync_scene.update_vertices([(0, pos)])
        return (time.perf_counter() - t0) * 1e3

    def async_both():
        pos = next_positions()
        stream.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        t0 = time.perf_counter()
        async_scene.update_vertices_async([(0, pos)])
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

    order_ms = "not measured"
    try:
        from torch.profiler import ProfilerActivity, profile
        pos = next_positions()
        stream.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            async_scene.update_vertices_async([(0, pos)])
            stream.synchronize()
        found = [e for e in prof.events() if "k_wide_order" in e.name]
        if found:
            order_ms = min(float(getattr(e, "device_time", 0.0) or getattr(e, "cuda_time", 0.0)) for e in found) * 1e-3
    except Exception as exc:      # the profiler is optional: the other numbers stand without it
        order_ms = f"not measured ({type(exc).__name__})"

    p = api.make_params(W, H, spp=1)
    frame = api.Frame(ctx, W, H)

    def loop(scene, update):
        stream.synchronize()
        t0 = time.perf_counter()
        for k in range(args.frames):
            update(scene, [(0, next_positions())])
            api.render(scene, s.camera, s.scene_info(k), p, frame, asynchronous=True)
        frame.wait()
        stream.synchronize()
        return args.frames / (time.perf_counter() - t0)

    fps = {"sync": [], "async": []}
    for _ in range(3):
        fps["sync"].append(loop(sync_scene, lambda sc, r: sc.update_vertices(r)))
        fps["async"].append(loop(async_scene, lambda sc, r: sc.update_vertices_async(r)))
    status = async_scene.update_status()
    out = {
        "what": "vertex update between frames, synchronous vs enqueued", "scene": "sponza_class", "device": ctx.device_name(),
        "width": W, "height": H, "triangles": int(st.numTriangles), "nodes": int(st.numNodes), "vertices": int(base.shape[0]),
        "sync_wall_ms": {"min": min(sync_ms), "all": sync_ms},
        "async_host_ms": {"min": min(host_ms), "all": host_ms},
        "async_gpu_ms": {"min": min(gpu_ms), "all": gpu_ms},
        "wide_order_gpu_ms": order_ms,
        "async_gpu_below_sync_wall": min(gpu_ms) < min(sync_ms),
        "fps_sync": {"max": max(fps["sync"]), "all": fps["sync"]}, "fps_async": {"max": max(fps["async"]), "all": fps["async"]},
        "frames_per_loop": args.frames, "updates_enqueued": status.enqueued, "updates_refused": status.refused,
    }
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
