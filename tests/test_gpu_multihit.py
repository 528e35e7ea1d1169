"""The multi-hit ray query on the device (rtr_trace_rays_multi: the first K hits along a ray by (t, customIndex, primitiveId), resumable)
against tests/multihit_witness.py: test_gpu_cull_masks.all_hits' candidates — every record oracle_mt accepts — classed by
tests/ray_flags_witness.py, filtered, sorted, cut behind `after`, sliced and padded with the ray's miss record.  Every slot of every
ray is compared bit for bit, and the counts.  With K = 1 the query is held to the closest-hit query's bytes and counters."""
import os

import numpy as np
import pytest
import torch

from realtimeraytracer_amd import _abi as A
from realtimeraytracer_amd import api, scenes

import multihit_witness as M
import ray_flags_witness as W
from test_gpu_cull_masks import all_hits, by_custom, counters, scene_of, seeded_masks
from test_gpu_occlusion import mixed_rays
from deep_scene import _deep_scene

pytestmark = pytest.mark.gpu

INVALID = -1
BUILDS = pytest.mark.parametrize("build", [A.BUILD_HOST_SAH, A.BUILD_DEVICE_LBVH], ids=["host_sah", "device_lbvh"])
OPQ = A.QUERY_OPAQUE


def _np(x):
    return x.cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)


def _kw(flags):
    return {"opaque": bool(flags & OPQ), "ray_flags": flags & ~OPQ}


def assert_slots(res, exp, what, more=""):
    """every slot of every ray, all 8 words, and the counts"""
    hits, counts = exp
    got = _np(res.hits).view(np.uint32)
    assert got.shape == hits.shape, f"{what}: shape {got.shape}, expected {hits.shape}"
    bad = (got != hits).any(axis=2)
    if bad.any():
        r, j = (x[:5] for x in np.nonzero(bad))
        raise AssertionError(f"{what}: {int(bad.sum())} slots of {int(bad.any(1).sum())} rays differ; first (ray, slot) {list(zip(r.tolist(), j.tolist()))}: "
                             f"gpu {got[r, j].tolist()} expected {hits[r, j].tolist()} {more}")
    gc = _np(res.counts).astype(np.int64)
    assert (gc == counts).all(), f"{what}: counts differ at rays {np.nonzero(gc != counts)[0][:8].tolist()} {more}"


def _layered(gpu_ctx, build):
    desc, keep = M.layered_scene()
    old = desc.buildFlags
    desc.buildFlags = build
    try:
        scene = api.Scene(gpu_ctx, desc)
    finally:
        desc.buildFlags = old
    rays, kinds = M.layered_rays(scene.stats(), mixed_rays)
    return scene, desc, keep, rays, kinds


# ---- 1. K = 1 is the closest-hit query ----------------------------------------------------------------------------------------------
@BUILDS
@pytest.mark.parametrize("case", ["textured_room", "sponza_mixed"])
def test_k1_is_the_closest_hit_query(gpu_ctx, scene_cache, tmp_path, case, build):
    scene, desc, keep, s = scene_of(case, gpu_ctx, tmp_path, build)
    st = scene.stats()
    diag = float(np.linalg.norm(np.array(st.boundsMax[:]) - np.array(st.boundsMin[:])))
    rays = torch.cat([api.camera_rays(gpu_ctx, s.camera, 160, 100, 1), torch.from_numpy(mixed_rays(st, 20000, 3, diag)).cuda()])
    alpha_tests = 0
    for kw in (dict(opaque=False), dict(opaque=True), dict(opaque=False, ray_flags=A.QUERY_CULL_BACK_FACING)):
        a = api.trace_rays(scene, rays, collect_stats=True, cull_mask=0xff, **kw)
        b = api.trace_rays_multi(scene, rays, 1, collect_stats=True, **kw)
        assert b.hits.shape == (rays.shape[0], 1, 8) and b.counts.shape == (rays.shape[0],)
        assert torch.equal(b.hits.view(-1, 8), a.hits), f"{case} {kw}: K = 1 must give the closest-hit records"
        assert counters(b.stats) == counters(a.stats), f"{case} {kw}: counters {counters(b.stats)} against {counters(a.stats)}"
        assert torch.equal(b.counts, (a.custom_index != -1).to(torch.int32))
        assert torch.equal(api.trace_rays_multi(scene, rays, 1, **kw).hits, b.hits), "the timed form"
        alpha_tests += a.stats.numAlphaTests
    assert alpha_tests > 0


# ---- 2. the layered scene against first_k ------------------------------------------------------------------------------------------
@BUILDS
def test_layered_scene_equals_first_k(gpu_ctx, oracle, build):
    scene, desc, keep, rays, kinds = _layered(gpu_ctx, build)
    rt = torch.from_numpy(rays).cuda()
    bvh = scene.export_bvh()
    cands = all_hits(oracle, bvh, rays)
    classes = W.classify(cands, rays, bvh, W.mirrored_by_custom(desc), W.AlphaWitness(desc))
    n = np.array([len(c[0]) for c in cands])
    for kind in (0, 1):                                      # true by construction (tests/test_multihit_abi.py holds the scene to it)
        inside = M.grid_inside(rays[kinds == kind])
        assert inside.sum() >= 100 and (~inside).sum() >= 100
        assert (n[kinds == kind][inside] > 8).all(), "every grid ray inside the quad has more than 8 accepted records: truncation"
        assert (n[kinds == kind][~inside] == 0).all(), "every grid ray outside has none: padding"
    for K in (1, 2, 4, 5, 8):                                # 4 cuts the tie pair of layer 3 (customIndex 3 and 12)
        exp = M.first_k(cands, classes, rays, K, 0)
        assert_slots(api.trace_rays_multi(scene, rt, K), exp, f"layered K = {K}")
        assert_slots(api.trace_rays_multi(scene, rt, K, collect_stats=True), exp, f"layered K = {K}, counting form")
    thru = np.nonzero((kinds == 0) & (n == 16))[0]
    got = _np(api.trace_rays_multi(scene, rt, 4).custom_index)[thru]
    assert (got == [0, 1, 2, 3]).all(), "of the tie (t, 3, .) / (t, 12, .) the lower customIndex comes fourth"
    assert_slots(api.trace_rays_multi(scene, rays, 5), M.first_k(cands, classes, rays, 5, 0), "numpy in, numpy out")
    assert isinstance(api.trace_rays_multi(scene, rays, 5).hits, np.ndarray)


# ---- 3. chained enumeration ----------------------------------------------------------------------------------------------------------
@BUILDS
def test_chained_calls_enumerate_every_hit_exactly_once(gpu_ctx, oracle, build):
    scene, desc, keep, rays, kinds = _layered(gpu_ctx, build)
    rt = torch.from_numpy(rays).cuda()
    bvh = scene.export_bvh()
    cands = all_hits(oracle, bvh, rays)
    full = M.accepted(cands, M.trivial_classes(cands), rays, 0)
    thru = (kinds <= 1) & M.grid_inside(rays) & (rays[:, 0] != rays[:, 1])
    assert thru.sum() > 200 and all(len(full[k]) == 16 for k in np.nonzero(thru)[0])
    once = api.trace_rays_multi(scene, rt, 8)
    for K in (2, 3):
        seen = [[] for _ in rays]
        links = []
        res = api.trace_rays_multi(scene, rt, K)
        for _ in range(40):
            c = _np(res.counts)
            if not c.any():
                break
            links.append(res)
            h = _np(res.hits).view(np.uint32)
            for k in np.nonzero(c)[0]:
                for j in range(int(c[k])):
                    seen[k].append(((h[k, j, 0:1].view(np.float32)[0], int(h[k, j, 3]), int(h[k, j, 4])), h[k, j, 1:3].view(np.float32).copy()))
            res = api.trace_rays_multi(scene, rt, K, after=res)
        else:
            raise AssertionError(f"K = {K}: the chain did not end")
        assert not _np(res.counts).any() and (_np(res.custom_index) == -1).all()
        assert (_np(res.t).view(np.uint32) == rays[:, 7:8].view(np.uint32)).all(), "an exhausted ray reports its own tmax"
        for k, (got, exp) in enumerate(zip(seen, full)):
            assert [g[0] for g in got] == [e[0] for e in exp], f"K = {K} ray {k}: {[g[0] for g in got]} against {[e[0] for e in exp]}"
            assert all((g[1].view(np.uint32) == np.array([e[1], e[2]], np.float32).view(np.uint32)).all() for g, e in zip(got, exp))
        if K == 2:                                           # four links are K = 8 once
            assert len(links) >= 4
            assert torch.equal(torch.cat([x.hits for x in links[:4]], dim=1), once.hits), "four links of K = 2 against K = 8"
        # a link equals the witness's resumed slice, miss padding included
        exp = M.first_k(cands, M.trivial_classes(cands), rays, K, 0, after=_np(links[0].last))
        assert_slots(links[1], exp, f"K = {K}: the second link")
        assert_slots(api.trace_rays_multi(scene, rt, K, after=links[0].last, collect_stats=True), exp, f"K = {K}: the second link, counting form")


# ---- 4. workload scenes against first_k ---------------------------------------------------------------------------------------------
@BUILDS
@pytest.mark.parametrize("case", ["features", "textured_room", "sponza_mixed"])
def test_workload_scenes_equal_first_k(gpu_ctx, oracle, scene_cache, tmp_path, case, build):
    scene, desc, keep, s = scene_of(case, gpu_ctx, tmp_path, build)
    st = scene.stats()
    diag = float(np.linalg.norm(np.array(st.boundsMax[:]) - np.array(st.boundsMin[:])))
    rays = mixed_rays(st, 300 if case == "sponza_mixed" else 1500, 31, diag)
    if case == "sponza_mixed":          # rays that meet more of the scene: camera rays of a coarse frame
        rays = np.concatenate([rays, _np(api.camera_rays(gpu_ctx, s.camera, 16, 9, 1))]).astype(np.float32)
    rt = torch.from_numpy(rays).cuda()
    bvh = scene.export_bvh()
    cands = all_hits(oracle, bvh, rays)
    classes = W.classify(cands, rays, bvh, W.mirrored_by_custom(desc), W.AlphaWitness(desc))
    masks = seeded_masks(desc.numInstances, 101)
    scene.set_instance_masks(masks)
    cm = by_custom(desc, masks)
    rm = seeded_masks(len(rays), 7)
    rmt = torch.from_numpy(rm).cuda()
    runs = [(OPQ, {}, dict(custom_masks=cm, ray_masks=0xff))]      # no mask given is cullMask 0xff: an instance whose mask is 0 stays unseen
    runs += [(f, dict(cull_mask=0xb7, ray_masks=rmt), dict(custom_masks=cm, ray_masks=rm.astype(np.int64) & 0xb7))
             for f in (A.QUERY_CULL_BACK_FACING, A.QUERY_CULL_FRONT_FACING, A.QUERY_CULL_OPAQUE, A.QUERY_CULL_NO_OPAQUE)]
    for flags, kw, wkw in runs:
        sizes = np.array([len(x) for x in M.accepted(cands, classes, rays, flags, **wkw)])
        for K in (2, 8):
            share = f"({(sizes > K).mean():.3f} of the rays have more than {K} accepted records, {(sizes > 0).mean():.3f} have any)"
            res = api.trace_rays_multi(scene, rt, K, **_kw(flags), **kw)
            assert_slots(res, M.first_k(cands, classes, rays, K, flags, **wkw), f"{case} flags {flags:#x} K = {K}", share)
            if flags == OPQ and K == 2:
                assert (sizes > K).any(), f"{case}: truncation must occur {share}"


# ---- 5. deep stacks ------------------------------------------------------------------------------------------------------------------
def test_deep_rays_take_the_tail_kernel(gpu_ctx):
    d, keep, scene, cam = _deep_scene(gpu_ctx)
    rays = api.camera_rays(gpu_ctx, cam, 16, 8, 2)
    n = rays.shape[0]
    r4 = api.trace_rays_multi(scene, rays, 4, collect_stats=True)
    assert r4.stats.tailRays > 0 and r4.stats.numRays == n, "the rays must go through k_multihit_tail"
    assert torch.equal(api.trace_rays_multi(scene, rays, 4).hits, r4.hits), "the timed form"
    closest = api.trace_rays(scene, rays, collect_stats=True, cull_mask=0xff)
    r1 = api.trace_rays_multi(scene, rays, 1, collect_stats=True)
    assert torch.equal(r1.hits.view(-1, 8), closest.hits) and counters(r1.stats) == counters(closest.stats)
    assert torch.equal(r4.hits[:, 0, :], closest.hits), "slot 0 of K = 4 is the closest hit"
    # which rays were abandoned: a group of rays launched alone whose tailRays equals its size holds only such rays (a lone deep ray
    # walks for a tenth of a second, so the groups are halved, not the rays asked one by one)
    def tail_count(idx):
        sub = rays[torch.from_numpy(idx).to(rays.device)].contiguous()
        return api.trace_rays_multi(scene, sub, 4, collect_stats=True).stats.tailRays

    tail = M.tail_rays(tail_count, n)
    assert tail and len(tail) <= r4.stats.tailRays
    sub = _np(rays)[tail]
    cands = M.all_hits32(scene.export_bvh(), sub)
    exp = M.first_k(cands, M.trivial_classes(cands), sub, 4, 0)
    got = api.MultiHitResult()
    got.hits, got.counts = r4.hits[tail], r4.counts[tail]
    assert_slots(got, exp, f"{len(tail)} tail rays, K = 4")
    assert (exp[1] > 0).any(), "some tail ray must hit"
    # resumed behind their second hit, the tail rays go on where they stopped
    link = api.trace_rays_multi(scene, rays, 2)
    nxt = api.trace_rays_multi(scene, rays, 2, after=link, collect_stats=True)
    assert torch.equal(torch.cat([link.hits, nxt.hits], dim=1), r4.hits), "two links of K = 2 against K = 4"
    # a redo list of 4 entries: the tail kernel finds the abandoned rays by their sentinel (RTR_QUERY_REDO_CAP: librtr_hip_test.so only)
    os.environ["RTR_QUERY_REDO_CAP"] = "4"
    try:
        hctx = api.Context(0, test_hooks=True)
        hscene = api.Scene(hctx, d)
        for counts_form in (True, False):
            hr = api.trace_rays_multi(hscene, rays, 4, collect_stats=counts_form)
            assert torch.equal(hr.hits, r4.hits) and torch.equal(hr.counts, r4.counts), "the redo list overflowed"
            assert not counts_form or hr.stats.tailRays > 4
        hscene.close(); hctx.close()
    finally:
        del os.environ["RTR_QUERY_REDO_CAP"]


# ---- 6. degenerate input and refusals -----------------------------------------------------------------------------------------------
def test_degenerate_rays_and_refusals(gpu_ctx, scene_cache):
    s = scenes.cornell_box(64, 64)
    scene = api.Scene(gpu_ctx, s.desc)
    lib, ctx = gpu_ctx.lib, gpu_ctx.h
    good = _np(api.camera_rays(gpu_ctx, s.camera, 8, 8, 1))
    bad = np.repeat(good[:1], 8, axis=0)
    bad[0] = 0.0                                             # the null ray
    bad[1, 4:7] = 0.0                                        # zero direction
    bad[2, 0] = np.nan; bad[3, 5] = np.inf; bad[4, 2] = -np.inf
    bad[5, 7] = np.nan                                       # NaN tmax
    bad[6, 7] = bad[6, 3]                                    # an empty interval
    bad[7, 7] = -1.0
    rays = np.concatenate([good, bad]).astype(np.float32)
    rt = torch.from_numpy(rays).cuda()
    for K in (1, 3, 8):
        r = api.trace_rays_multi(scene, rt, K, collect_stats=True)
        h = _np(r.hits).view(np.uint32)[64:]
        assert not _np(r.counts)[64:].any()
        assert (h[:, :, 0] == bad[:, 7:8].view(np.uint32)).all(), "a miss reports the ray's own tmax bits"
        assert (h[:, :, 3] == M.MISS).all() and (h[:, :, 4] == M.MISS).all() and not h[:, :, [1, 2, 5, 6, 7]].any()
        assert r.stats.numRays == len(rays)
        assert torch.equal(r.hits[:64, 0], api.trace_rays(scene, rt[:64].contiguous()).hits)
    only_bad = api.trace_rays_multi(scene, rt[64:].contiguous(), 4, collect_stats=True)
    assert only_bad.stats.numNodeVisits == 0 and only_bad.stats.numTriTests == 0, "a degenerate ray walks nothing"
    zero = api.trace_rays_multi(scene, rt, 4, cull_mask=0, collect_stats=True)
    assert not _np(zero.counts).any() and zero.stats.numNodeVisits == 0, "an effective mask of 0 walks nothing"
    # refused, and the prefilled outputs are untouched
    n = 64
    hits = torch.full((n * 8 * 8 + 8,), 0x5a5a5a5a, dtype=torch.int32, device="cuda")
    cnts = torch.full((n + 1,), 0x5a5a5a5a, dtype=torch.int32, device="cuda")
    pre_h, pre_c = hits.clone(), cnts.clone()
    rp, hp, cp = A.VP(rt.data_ptr()), A.VP(hits.data_ptr()), A.VP(cnts.data_ptr())
    both = A.QUERY_CULL_BACK_FACING | A.QUERY_CULL_FRONT_FACING

    def call(rays_p=rp, masks_p=None, num=n, k=4, flags=0, cull=0xff, after=None, hits_p=hp, counts_p=cp, c=ctx, sc=scene.h):
        return lib.rtr_trace_rays_multi(c, sc, rays_p, masks_p, num, k, flags, cull, after, hits_p, counts_p, None)

    refusals = [(dict(k=0), b"maxHits"), (dict(k=9), b"maxHits"), (dict(flags=A.QUERY_ANY), b"RTR_QUERY_ANY"), (dict(flags=both), b"exclude"),
                (dict(flags=A.QUERY_OPAQUE | A.QUERY_CULL_OPAQUE), b"exclude"), (dict(flags=4), b"flag"), (dict(flags=8), b"flag"),
                (dict(flags=0x100), b"flag"), (dict(cull=0x100), b"cullMask"), (dict(hits_p=A.VP(hits.data_ptr() + 4)), b"hits is not 16-B aligned"),
                (dict(rays_p=A.VP(rt.data_ptr() + 8)), b"rays is not 16-B aligned"), (dict(after=A.VP(rt.data_ptr() + 4)), b"after is not 16-B aligned"),
                (dict(counts_p=A.VP(cnts.data_ptr() + 2)), b"counts is not 4-B aligned"), (dict(rays_p=None), b"rays is null"),
                (dict(hits_p=None), b"hits is null"), (dict(c=None), b"null context or scene"), (dict(sc=None), b"null context or scene")]
    for kw, msg in refusals:
        assert call(**kw) == INVALID, kw
        err = lib.rtr_last_error()
        assert msg in err and b"rtr_trace_rays_multi" in err, (kw, err)
        assert lib.rtr_trace_rays_multi_async(kw.get("c", ctx), kw.get("sc", scene.h), kw.get("rays_p", rp), None, n, kw.get("k", 4), kw.get("flags", 0),
                                              kw.get("cull", 0xff), kw.get("after"), kw.get("hits_p", hp), kw.get("counts_p", cp)) == INVALID, kw
    torch.cuda.synchronize()
    assert torch.equal(hits, pre_h) and torch.equal(cnts, pre_c), "a refused call writes nothing"
    if torch.cuda.device_count() > 1:
        other = api.Context(1)
        assert call(c=other.h) == INVALID
        other.close()
    # no rays: nothing to do, nothing written; counts = NULL works; ray masks need no alignment
    assert call(rays_p=None, num=0, hits_p=None, counts_p=None) == 0
    assert call(num=0) == 0
    torch.cuda.synchronize()
    assert torch.equal(hits, pre_h) and torch.equal(cnts, pre_c)
    ref = api.trace_rays_multi(scene, rt[:n].contiguous(), 4)
    assert call(counts_p=None) == 0
    assert torch.equal(hits[:n * 32].view(n, 4, 8), ref.hits) and torch.equal(hits[n * 32:], pre_h[n * 32:]) and torch.equal(cnts, pre_c)
    rm = torch.full((n + 1,), 0xff, dtype=torch.uint8, device="cuda")
    hits.fill_(0)
    assert call(masks_p=A.VP(rm.data_ptr() + 1)) == 0
    assert torch.equal(hits[:n * 32].view(n, 4, 8), ref.hits) and torch.equal(cnts[:n], ref.counts)
    # the Python layer refuses before anything is launched
    for kw in (dict(max_hits=0), dict(max_hits=9), dict(max_hits=2, ray_flags=A.QUERY_ANY), dict(max_hits=2, ray_flags=both)):
        with pytest.raises(ValueError):
            api.trace_rays_multi(scene, rt, **kw)
    for after in (ref.last[:10], ref.last.to(torch.float32), ref.last.cpu(), ref.hits):
        with pytest.raises(ValueError):
            api.trace_rays_multi(scene, rt[:n].contiguous(), 2, after=after)
    with pytest.raises(ValueError):
        api.trace_rays_multi(scene, rt, 2, collect_stats=True, asynchronous=True)


# ---- 7. composition with hit_surfaces -----------------------------------------------------------------------------------------------
def test_hit_surfaces_of_the_flattened_result(gpu_ctx, scene_cache, tmp_path):
    scene, desc, keep, s = scene_of("textured_room", gpu_ctx, tmp_path)
    rays = api.camera_rays(gpu_ctx, s.camera, 160, 100, 1)
    K = 4
    r = api.trace_rays_multi(scene, rays, K)
    assert int((r.counts > 1).sum()) > 0
    surf = api.hit_surfaces(scene, rays.repeat_interleave(K, 0), r.hits.view(-1, 8))
    first = api.hit_surfaces(scene, rays, api.trace_rays(scene, rays))
    assert torch.equal(surf.raw.view(-1, K, 20)[:, 0].view(torch.int32), first.raw.view(torch.int32)), "column 0: the surfaces of the closest hits"
    kinds = surf.kind.view(-1, K)
    assert bool((kinds[:, 1:][r.custom_index[:, 1:] == -1] == A.SURFACE_MISS).all()), "a miss record gives the sky"
    assert bool((kinds != A.SURFACE_INVALID).all())


# ---- 8. stream order ----------------------------------------------------------------------------------------------------------------
def test_a_chain_enqueued_without_a_host_join(scene_cache):
    ctx = api.Context(0)
    desc, keep = M.layered_scene()
    scene = api.Scene(ctx, desc)
    rays_np, kinds = M.layered_rays(scene.stats(), mixed_rays)
    rays0 = torch.from_numpy(rays_np).cuda()
    a = api.trace_rays_multi(scene, rays0, 3)
    b = api.trace_rays_multi(scene, rays0, 3, after=a)
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        ctx.set_stream(stream.cuda_stream)
        rays = rays0 * 1.0                                    # torch work on the stream ahead of the calls
        x = api.trace_rays_multi(scene, rays, 3, asynchronous=True)
        y = api.trace_rays_multi(scene, rays, 3, after=x, asynchronous=True)       # x.last: a device-side gather on the same stream
        t = y.t * 1.0                                         # consumed on the same stream, no host join in between
        stream.synchronize()
        assert torch.equal(x.hits, a.hits) and torch.equal(x.counts, a.counts)
        assert torch.equal(y.hits, b.hits) and torch.equal(y.counts, b.counts) and torch.equal(t.view(torch.int32), b.t.view(torch.int32))
        assert int(b.counts.sum()) > 0
        ctx.set_stream(None)
    with pytest.raises(ValueError):
        api.trace_rays_multi(scene, rays, 3, asynchronous=True)          # the context is no longer on torch's current stream
    scene.close(); ctx.close()
