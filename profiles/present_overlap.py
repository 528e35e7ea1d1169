"""The presented frame (1920x1080 sponza_class, five ray-gen images at 4 spp, 4 a-trous rounds, combine) three ways:
  (a) one frame at a time, synchronous: rtr_render + rtr_denoise_combine (what bench.py's `presented_frame` times);
  (b) two contexts alternating rtr_render_async + rtr_denoise_combine_async, joined only one frame behind;
  (c) librtr_mgpu.so's present mode (RTR_MGPU_PRESENT) with one rank exchanging with itself (test build), one frame at a time and
      with two slots in flight.
(a) and (b) alternate within one process, repeated; every timing is a host clock around a device synchronise after a warm-up.
--mode deint runs k_deinterleave_images (five 1080p images from eight shards) and five k_deinterleave launches back to back, for a
kernel trace of its own (rocprofv3 --kernel-trace --stats).

python profiles/present_overlap.py --mode ab|mgpu|deint"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("--mode", choices=["ab", "mgpu", "deint"], default="ab")
ap.add_argument("--frames", type=int, default=20)
ap.add_argument("--repeats", type=int, default=4)
args = ap.parse_args()
if args.mode == "mgpu":
    os.environ["RTR_MGPU_SELF_EXCHANGE"] = "1"      # the one-rank communicator still sends its shard through RCCL (librtr_mgpu_test.so)

import numpy as np
import torch
from realtimeraytracer_amd import _abi as A
from realtimeraytracer_amd import api, mgpu, scenes

W, H, SPP, IT = 1920, 1080, 4, 4


def sync_frames(scene, s, p, frame, first, n):
    """(a): one frame at a time"""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for j in range(n):
        api.render(scene, s.camera, s.scene_info(first + j), p, frame)
        frame.denoise_combine(IT)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / n


def overlapped_frames(scene, s, p, frames, first, n):
    """(b): two contexts alternate; frame j is joined after frame j + 1 has been enqueued"""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for j in range(n):
        fr = frames[j % 2]
        api.render(scene, s.camera, s.scene_info(first + j), p, fr, asynchronous=True)
        fr.denoise_combine_async(IT)
        if j >= 1:
            frames[(j - 1) % 2].wait()
    frames[(n - 1) % 2].wait()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / n


if args.mode == "ab":
    s = scenes.sponza_class(W, H, ltc=scenes.shipped_ltc())
    ctx = api.Context(0)
    scene = api.Scene(ctx, s.desc)
    p = api.make_params(W, H, spp=SPP, images=A.IMAGES_RAYGEN5)
    one = api.Frame(ctx, W, H, 0xff)
    ctxs = [api.Context(0), api.Context(0)]
    two = [api.Frame(c, W, H, 0xff) for c in ctxs]
    print(f"device: {ctx.device_name()}; {W}x{H} sponza_class, {SPP} spp, five images, {IT} a-trous rounds + combine; {args.frames} frames per timing")
    sync_frames(scene, s, p, one, 0, 4)                   # warm-up of both forms
    overlapped_frames(scene, s, p, two, 0, 4)
    # the two forms must present the same frame
    api.render(scene, s.camera, s.scene_info(100), p, one); one.denoise_combine(IT)
    overlapped_frames(scene, s, p, two, 100, 1)
    same = int((one.download(A.IMAGE_FINAL) != two[0].download(A.IMAGE_FINAL)).sum())
    print(f"FINAL of frame 100, (a) vs (b): {same} pixels differ")
    ra, rb = [], []
    for rep in range(args.repeats):
        ra.append(sync_frames(scene, s, p, one, 10, args.frames))
        rb.append(overlapped_frames(scene, s, p, two, 10, args.frames))
        print(f"repeat {rep}: (a) one at a time {ra[-1]:.3f} ms/frame   (b) two contexts, joined one behind {rb[-1]:.3f} ms/frame")
    # what the post passes cost on their own (the frame's images are already rendered)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.frames):
        one.denoise_combine(IT)
    post = (time.perf_counter() - t0) * 1e3 / args.frames
    print(f"(a) median {np.median(ra):.3f} ms/frame, (b) median {np.median(rb):.3f} ms/frame, (b)/(a) {np.median(rb) / np.median(ra):.3f}; "
          f"denoise + combine alone {post:.3f} ms")
elif args.mode == "mgpu":
    s = scenes.sponza_class(W, H, ltc=scenes.shipped_ltc())
    m = mgpu.MultiGpu(devices=[0], frames_in_flight=2)
    assert m.info.selfExchange == 1
    m.scene_create(s.desc)
    p = api.make_params(W, H, spp=SPP, images=A.IMAGES_RAYGEN5)
    for j in range(4):
        m.render_async(j % 2, s.camera, s.scene_info(j), p, present=True)
        m.wait(j % 2)
    res_one, res_two = [], []
    for rep in range(args.repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for j in range(args.frames):
            m.render_async(0, s.camera, s.scene_info(10 + j), p, present=True)
            m.wait(0)
        torch.cuda.synchronize()
        res_one.append((time.perf_counter() - t0) * 1e3 / args.frames)
        t0 = time.perf_counter()
        for j in range(args.frames):
            m.render_async(j % 2, s.camera, s.scene_info(10 + j), p, present=True)
            if j >= 1:
                m.wait((j - 1) % 2)
        m.wait((args.frames - 1) % 2)
        torch.cuda.synchronize()
        res_two.append((time.perf_counter() - t0) * 1e3 / args.frames)
        print(f"repeat {rep}: (c) one rank, self-exchange, present: one at a time {res_one[-1]:.3f} ms/frame, two slots in flight {res_two[-1]:.3f} ms/frame")
    print(f"(c) median: one at a time {np.median(res_one):.3f} ms/frame, two slots in flight {np.median(res_two):.3f} ms/frame")
    m.close()
else:
    N, band, planes, reps = 8, 8, 5, 50
    ctx = api.Context(0)
    rows = api.shard_rows(H, band, N)
    g = torch.randint(0, 2 ** 31 - 1, (N, planes, rows, W), dtype=torch.int32, device="cuda")
    outs = [torch.empty((H, W), dtype=torch.int32, device="cuda") for _ in range(planes)]
    per_plane = [g[:, k].contiguous() for k in range(planes)]
    one = torch.empty((H, W), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()                      # the library's kernels run on the context's stream, not torch's
    for r in range(reps):
        api.deinterleave_images(ctx, g.data_ptr(), [o.data_ptr() for o in outs], W, H, band, N)
        for k in range(planes):
            api.deinterleave_bands(ctx, per_plane[k].data_ptr(), one.data_ptr(), W, H, band, N)
    torch.cuda.synchronize()
    mb = 2 * planes * W * H * 4 / 1e6
    print(f"{reps} x (k_deinterleave_images of {planes} images + {planes} x k_deinterleave), {W}x{H}, {N} shards: {mb:.1f} MB moved per {planes}-image de-interleave; "
          f"at 6.3 TB/s that is {mb / 6.3e6 * 1e6:.1f} us")
