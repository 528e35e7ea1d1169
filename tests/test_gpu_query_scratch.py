"""The three kinds of ray query (rtr_trace_rays, rtr_trace_rays_multi, rtr_trace_occlusion) share one context's query scratch: the redo
list, its count, the deep stacks, the counters and the two events.  Run back to back on two streams, asynchronous and counting forms
mixed, every call must still give what it gives alone: no stale redo count, no missing wait between the streams."""
import os

import pytest
import torch

from realtimeraytracer_amd import api, host

from deep_scene import _deep_scene

pytestmark = pytest.mark.gpu

COUNTERS = ("numRays", "numNodeVisits", "numTriTests", "numAlphaTests", "tailRays")


def _counters(stats):
    return tuple(int(getattr(stats, k)) for k in COUNTERS)


def test_queries_of_every_kind_share_the_scratch_across_two_streams():
    """16 x 8 camera rays from each of the deep scene's two ends, 256 rays: from the head they outgrow the closest-hit walks' 16-entry
    stack (nearest child first), from the wall end, looking back, the any-hit walks' (farthest child first; tests/test_gpu_occlusion.py),
    so that with a redo list of 4 entries EVERY kind of query abandons more rays than the list holds and its tail finds them by their
    sentinel.  (The head's fan alone, at 2 samples a pixel, leaves both any-hit walks at tailRays 0: they end on the wall at once.)"""
    W, H = 16, 8
    K = 4
    os.environ["RTR_QUERY_REDO_CAP"] = "4"
    try:
        rctx = api.Context(0, test_hooks=True)
        d, keep, rscene, cam = _deep_scene(rctx)
        end = float(1 << 19) * 0.01
        back = host.Camera(0.004, (end + 0.5, -0.995, 0.0), (0.2 * end, -1.0, 0.0), (0.0, 1.0, 0.0), W, H).getGPUData()
        rays = torch.cat([api.camera_rays(rctx, c, W, H, 1) for c in (cam, back)])
        assert rays.shape[0] == W * H * 2 == 256
        ref = {"closest": api.trace_rays(rscene, rays, collect_stats=True),
               "any": api.trace_rays(rscene, rays, any_hit=True, collect_stats=True),
               "multi": api.trace_rays_multi(rscene, rays, K, collect_stats=True),
               "occlusion": api.trace_occlusion(rscene, rays, collect_stats=True)}

        ctx = api.Context(0, test_hooks=True)
        scene = api.Scene(ctx, d)
        a, b = torch.cuda.Stream(), torch.cuda.Stream()
        torch.cuda.synchronize()                      # the rays were made on torch's default stream
        ctx.set_stream(a.cuda_stream)
        with torch.cuda.stream(a):
            multi_a = api.trace_rays_multi(scene, rays, K, asynchronous=True)
        ctx.set_stream(b.cuda_stream)
        with torch.cuda.stream(b):
            occ_b = api.trace_occlusion(scene, rays, asynchronous=True)
        got = {}
        ctx.set_stream(a.cuda_stream)
        got["closest"] = api.trace_rays(scene, rays, collect_stats=True)
        ctx.set_stream(b.cuda_stream)
        got["multi"] = api.trace_rays_multi(scene, rays, K, collect_stats=True)
        ctx.set_stream(a.cuda_stream)
        got["any"] = api.trace_rays(scene, rays, any_hit=True, collect_stats=True)
        ctx.set_stream(b.cuda_stream)
        got["occlusion"] = api.trace_occlusion(scene, rays, collect_stats=True)
        torch.cuda.synchronize()

        for what in ("closest", "any", "multi", "occlusion"):
            print(what, _counters(got[what].stats), "alone:", _counters(ref[what].stats))
        for what, r in (("multi, asynchronous", multi_a), ("multi", got["multi"])):
            assert torch.equal(r.hits, ref["multi"].hits), what
            assert torch.equal(r.counts, ref["multi"].counts), what
        assert torch.equal(got["closest"].hits, ref["closest"].hits)
        assert torch.equal(got["any"].occluded, ref["any"].occluded)
        for what, r in (("occlusion, asynchronous", occ_b), ("occlusion", got["occlusion"])):
            assert torch.equal(r.occluded, ref["occlusion"].occluded), what
        # each ray's walk is its own in these three, so their counters are the lone call's
        for what in ("closest", "any", "multi"):
            assert _counters(got[what].stats) == _counters(ref[what].stats), what
        # the queued query's visit counts depend on how its persistent waves share the queue
        assert got["occlusion"].stats.numRays == ref["occlusion"].stats.numRays == 256
        for what in ("closest", "any", "multi", "occlusion"):
            for where, r in (("alone", ref), ("in the sequence", got)):
                assert r[what].stats.tailRays > 4, f"{what}, {where}: tailRays {r[what].stats.tailRays}"

        ctx.set_stream(None)
        scene.close(); ctx.close()
        rscene.close(); rctx.close()
    finally:
        del os.environ["RTR_QUERY_REDO_CAP"]
