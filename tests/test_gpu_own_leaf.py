"""Start hints for the queued occlusion query on the device (rtr_hit_leaves, rtr_light_rays_hinted, rtr_trace_occlusion_hinted).  Every
comparison is at tolerance 0:
  * the triangle -> leaf table is a numpy restatement's, for host-built and device-built trees, before and after a refit;
  * the hinted light rays are rtr_light_rays' bytes, and the hints are the renderer's marks (the oracle counts them);
  * hints never change a byte — right ones, none, other triangles' leaves, arbitrary int32 words;
  * with the hinted light rays of a frame's camera hits the query's counters are the renderer's any-hit counters at its defaults
    (trace_own_leaf = 1) and the oracle's: it IS the renderer's walk;
  * the composed route through it gives the dense route's and the renderer's bits; stream order, the shared scratch, bad arguments, and
    the renderer is untouched."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from realtimeraytracer_amd import _abi as A
from realtimeraytracer_amd import api, scenes
from test_gpu_occlusion import assert_same_bytes, mixed_rays

pytestmark = pytest.mark.gpu

MISS = 0xffffffff
INVALID = -1
ALL3 = A.LIGHT_SHADOWED | A.LIGHT_UNSHADOWED | A.LIGHT_ANALYTIC
ALL5 = A.IMAGES_RAYGEN5 | A.IMG_BIT(A.IMAGE_HDR)


def _np(x):
    return x.cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)


def _with_flags(desc, flags):
    d = A.rtr_scene_desc.from_buffer_copy(bytes(desc))
    d.buildFlags = flags
    return d


def table_from_export(bvh):
    """The restatement: walk the BVH2 nodes; every leaf child writes its code at (customIndex, primitiveId) of its records.  Returns the
    sorted keys customIndex << 32 | primitiveId and their codes."""
    nodes = np.frombuffer(bvh[0], dtype=np.int32).reshape(-1, 8)
    tris = np.frombuffer(bvh[1], dtype=np.uint32).reshape(-1, 12)
    child = nodes[:, 6:8].reshape(-1)
    leaf = child[child < 0]
    code = (~leaf).astype(np.int64)
    first, cnt = code >> 3, (code & 7) + 1
    assert (first + cnt <= len(tris)).all()
    rec = np.repeat(first, cnt) + (np.arange(cnt.sum()) - np.repeat(np.cumsum(cnt) - cnt, cnt))
    codes = np.repeat(leaf, cnt)
    keys = (tris[rec, 3].astype(np.uint64) << np.uint64(32)) | tris[rec, 7].astype(np.uint64)
    order = np.argsort(keys, kind="stable")
    keys, codes = keys[order], codes[order]
    same = keys[1:] == keys[:-1]                         # a single-leaf scene stores its leaf as both children: the same value twice
    assert (codes[1:][same] == codes[:-1][same]).all()
    assert len(np.unique(keys)) == len(tris), "every record sits in a leaf"
    return keys, codes


def expected_leaves(table, hits):
    keys, codes = table
    hits = _np(hits).view(np.uint32)
    k = (hits[:, 3].astype(np.uint64) << np.uint64(32)) | hits[:, 4].astype(np.uint64)
    at = np.minimum(np.searchsorted(keys, k), len(keys) - 1)
    return np.where(keys[at] == k, codes[at], 0).astype(np.int32)


def camera_hits(ctx, scene, s, w, h):
    rays = api.camera_rays(ctx, s.camera, w, h, 1)
    return rays, api.trace_rays(scene, rays).hits


# ---- 1. the table -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags", [A.BUILD_HOST_SAH, A.BUILD_DEVICE_LBVH])
@pytest.mark.parametrize("case", ["cornell_box", "sponza_mixed"])
def test_hit_leaves_equal_the_exported_tree(gpu_ctx, scene_cache, case, flags):
    w, h = (128, 128) if case == "cornell_box" else (160, 100)
    s = getattr(scenes, case)(w, h)
    scene = api.Scene(gpu_ctx, _with_flags(s.desc, flags))
    rays, hits = camera_hits(gpu_ctx, scene, s, w, h)
    table = table_from_export(scene.export_bvh())
    got = api.hit_leaves(scene, hits)
    assert got.dtype == torch.int32 and got.shape == (w * h,)
    exp = expected_leaves(table, hits)
    hu = _np(hits).view(np.uint32)
    miss = hu[:, 3] == MISS
    assert (exp[~miss] < 0).all() and (exp[miss] == 0).all()
    assert (_np(got) == exp).all(), f"{int((_np(got) != exp).sum())} of {w * h} leaves differ"
    assert (~miss).any()
    # light instances are in the tree, so a light hit gets its leaf; a miss gets 0
    probe = np.zeros((2, 8), np.uint32)
    probe[1, 3] = probe[1, 4] = MISS
    assert s.num_lights > 0
    pl = api.hit_leaves(scene, probe.view(np.int32))
    assert pl[0] < 0 and pl[0] == expected_leaves(table, probe.view(np.int32))[0] and pl[1] == 0
    # a leaf holds the triangle it is the leaf of
    tris = np.frombuffer(scene.export_bvh()[1], dtype=np.uint32).reshape(-1, 12)
    for k in np.nonzero(~miss)[0][:: max(1, int((~miss).sum()) // 200)]:
        code = ~int(exp[k])
        recs = tris[code >> 3: (code >> 3) + (code & 7) + 1]
        assert ((recs[:, 3] == hu[k, 3]) & (recs[:, 7] == hu[k, 4])).any()
    # forged ids: customIndex or primitiveId out of range give 0; numpy in, numpy out
    forged = hu.copy()
    n_inst = s.desc.numInstances
    forged[0::4, 3] = n_inst
    forged[1::4, 3] = 0xfffffffe                         # RTR_STACK_OVERFLOW's neighbourhood
    forged[2::4, 4] = 0x7fffffff
    fx = expected_leaves(table, forged.view(np.int32))
    assert (fx[0::4] == 0).all() and (fx[1::4] == 0).all() and (fx[2::4] == 0).all() and (fx[3::4] == exp[3::4]).all()
    gn = api.hit_leaves(scene, forged.view(np.int32))
    assert isinstance(gn, np.ndarray) and (gn == fx).all()
    # a refit keeps the table: moved instances, same leaves, and they still match a fresh export
    inst = [A.RtrInstance.from_buffer_copy(s.desc.instances[i]) for i in range(s.desc.numInstances)]
    for k, i in enumerate(inst):
        if i.customIndex >= s.num_lights:
            i.transform[3] += 3.0 * (k % 3)
            i.transform[7] -= 2.0 * (k % 2)
    scene.update_instances(inst)
    after = api.hit_leaves(scene, hits)
    assert (_np(after) == exp).all(), "the leaves of the same ids after rtr_scene_update_instances"
    assert (expected_leaves(table_from_export(scene.export_bvh()), hits) == exp).all()
    scene.close()


def test_a_scene_made_like_another_makes_its_own_table(gpu_ctx, scene_cache):
    s = scenes.cornell_box(64, 64)
    built = api.Scene(gpu_ctx, s.desc)
    rays, hits = camera_hits(gpu_ctx, built, s, 64, 64)
    ctx2 = api.Context(0)
    out = A.VP()
    assert ctx2.lib.rtr_scene_create_like(ctx2.h, s.desc, built.h, out) == 0
    leaves = torch.full((64 * 64,), 7, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    assert ctx2.lib.rtr_hit_leaves(ctx2.h, out, A.VP(hits.data_ptr()), 64 * 64, A.VP(leaves.data_ptr())) == 0
    assert (_np(leaves) == expected_leaves(table_from_export(built.export_bvh()), hits)).all()
    assert torch.equal(api.hit_leaves(built, hits), leaves)
    ctx2.lib.rtr_scene_destroy(out)
    ctx2.close(); built.close()


# ---- 2. the rays and the hints ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["cornell_box", "sponza_mixed"])
def test_hinted_light_rays_are_the_light_rays_and_the_renderers_marks(gpu_ctx, oracle, scene_cache, case):
    w, h = (128, 128) if case == "cornell_box" else (160, 100)
    s = getattr(scenes, case)(w, h)
    scene = api.Scene(gpu_ctx, s.desc)
    rays, hits = camera_hits(gpu_ctx, scene, s, w, h)
    own = _np(api.hit_leaves(scene, hits))
    for frame in (0, 3):
        p = api.make_light_params(s.num_lights, 3, frame, w, 1)
        q = api.light_slots(scene, p)
        plain = api.light_rays(scene, rays, hits, p)
        lr, leaves = api.light_rays(scene, rays, hits, p, hints=True)
        assert leaves.dtype == torch.int32 and leaves.shape == (w * h * q,)
        assert torch.equal(lr.view(torch.int32), plain.view(torch.int32)), "the rays are rtr_light_rays' bytes"
        lv = _np(leaves).reshape(w * h, q)
        null = ~_np(lr).view(np.uint32).reshape(w * h, q, 8).any(2)
        assert ((lv == 0) | (lv == own[:, None])).all(), "a hint is 0 or its hit's leaf"
        assert (lv[null] == 0).all(), "null slots carry no hint"
        assert (lv[:, q - 1] == 0).all(), "the directional light's ray is never marked"
        assert null.any() and (lv != 0).any() and ((lv == 0) & ~null).any()
        ref = oracle.render(s.desc, s.camera, s.scene_info(frame), api.make_params(w, h, spp=1, shadow_rays=3), bvh=scene.export_bvh(), threads=16)
        assert int((lv != 0).sum()) == ref.walk.ownLeafRays, f"{case} frame {frame}: {int((lv != 0).sum())} hints, the oracle marks {ref.walk.ownLeafRays} rays"
    # numpy in, numpy out; explicit seeds
    seeds = np.arange(500, dtype=np.int32) * 7
    a = api.light_rays(scene, _np(rays)[:500], _np(hits)[:500], p, seeds=seeds)
    b, bl = api.light_rays(scene, _np(rays)[:500], _np(hits)[:500], p, seeds=seeds, hints=True)
    assert isinstance(bl, np.ndarray) and bl.dtype == np.int32 and (a.view(np.uint32) == b.view(np.uint32)).all()
    scene.close()


def test_both_forms_of_the_hinted_kernel_write_the_same(scene_cache):
    """The staged and the direct form of k_light_rays, which only the test build lets a caller pick (RTR_LIGHT_RAYS_DIRECT): the same rays —
    rtr_light_rays' — and the same hints; n is not a multiple of 64, so the last wave is partial."""
    code = (
        "import os, sys, torch\n"
        "sys.path.insert(0, sys.argv[1])\n"
        "from realtimeraytracer_amd import api, scenes\n"
        "ctx = api.Context(0, test_hooks=True)\n"
        "for s in (scenes.cornell_box(100, 75), scenes.textured_room(100, 75)):\n"
        "    scene = api.Scene(ctx, s.desc)\n"
        "    rays = api.camera_rays(ctx, s.camera, 100, 75, 1)[:7475]\n"
        "    q = api.trace_rays(scene, rays)\n"
        "    for nsr in (1, 3, 4):\n"
        "        p = api.make_light_params(s.num_lights, nsr, 1, 100, 1)\n"
        "        got = []\n"
        "        for direct in ('0', '1'):\n"
        "            os.environ['RTR_LIGHT_RAYS_DIRECT'] = direct\n"
        "            plain = api.light_rays(scene, rays, q.hits[:7475], p).view(torch.int32).clone()\n"
        "            lr, lv = api.light_rays(scene, rays, q.hits[:7475], p, hints=True)\n"
        "            assert torch.equal(lr.view(torch.int32), plain), (s.name, nsr, direct)\n"
        "            got.append((plain, lv.clone()))\n"
        "        assert bool(got[0][1].any()) and torch.equal(got[0][0], got[1][0]) and torch.equal(got[0][1], got[1][1]), (s.name, nsr)\n"
        "print('SAME')\n")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, RTR_SCENE_CACHE=scene_cache)
    r = subprocess.run([sys.executable, "-c", code, root], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0 and "SAME" in r.stdout, r.stdout + r.stderr


# ---- 3. hints never change a byte -----------------------------------------------------------------------------------------------------------
def hint_sets(rng, n, own_pool, ntri):
    """other triangles' leaves, permuted; and arbitrary words: positive, 0x80000000, -1, codes past the triangle count, anything"""
    others = rng.choice(own_pool, n).astype(np.int32)
    adv = rng.integers(-2**31, 2**31, n, dtype=np.int64).astype(np.int32)
    kind = rng.integers(0, 8, n)
    adv[kind == 0] = rng.integers(1, 2**31, n)[kind == 0]
    adv[kind == 1] = np.int32(-2**31)
    adv[kind == 2] = -1
    adv[kind == 3] = (~((np.int64(ntri) << 3) | rng.integers(0, 8, n)))[kind == 3]                      # first = the record count
    adv[kind == 4] = (~(((np.int64(ntri) - rng.integers(1, 8, n)) << 3) | 7))[kind == 4]                 # starts inside, ends outside
    adv[kind == 5] = np.int32(-2**31 + 1)
    return others, adv


def test_hints_never_change_a_byte(gpu_ctx, scene_cache):
    """The adversarial words are a safety property, run once: the refill takes a word as a leaf only when it is negative and its
    first + count lies within the scene's triangle records (k_shadow_trace4, HINTS), so none of them can address a record outside."""
    w, h = 160, 100
    s = scenes.sponza_mixed(w, h)
    scene = api.Scene(gpu_ctx, s.desc)
    st = scene.stats()
    raw = np.frombuffer(scene.export_bvh()[1], dtype=np.uint32).reshape(-1, 12)
    assert (raw[:, 11] & 1).any(), "the scene must hold alpha-tested triangles"
    rays, hits = camera_hits(gpu_ctx, scene, s, w, h)
    p = api.make_light_params(s.num_lights, 3, 0, w, 1)
    lr, leaves = api.light_rays(scene, rays, hits, p, hints=True)
    pool = np.unique(_np(api.hit_leaves(scene, hits)))
    pool = pool[pool != 0]
    diag = float(np.linalg.norm(np.array(st.boundsMax[:]) - np.array(st.boundsMin[:])))
    n = 200003
    rnd = torch.from_numpy(mixed_rays(st, n, 31, diag)).cuda()
    rng = np.random.default_rng(5)
    for name, r, correct in (("light rays", lr, leaves), ("random rays", rnd, None)):
        m = int(r.shape[0])
        others, adv = hint_sets(rng, m, pool, st.numTriangles)
        sets = [("no hints", None), ("other triangles' leaves", torch.from_numpy(others).cuda()), ("arbitrary words", torch.from_numpy(adv).cuda())]
        if correct is not None:
            sets.insert(0, ("the hits' own leaves", correct))
        for opaque in (False, True):
            dense = api.trace_rays(scene, r, any_hit=True, opaque=opaque).occluded
            assert bool(dense.any()) and not bool(dense.all())
            for what, sl in sets:
                q = api.trace_occlusion(scene, r, opaque=opaque, start_leaves=sl)
                assert_same_bytes(q.occluded, dense, f"{name}, opaque={opaque}, {what}")
    # numpy in, numpy out
    qn = api.trace_occlusion(scene, _np(rnd)[:1000], start_leaves=adv[:1000].copy())
    assert isinstance(qn.occluded, np.ndarray)
    assert_same_bytes(qn.occluded, _np(api.trace_rays(scene, rnd[:1000].contiguous(), any_hit=True).occluded), "numpy rays and hints")
    scene.close()


# ---- 4. it is the renderer's walk -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["sponza_class", "sponza_mixed"])
def test_counters_equal_the_renderers_walk_at_its_defaults(oracle, scene_cache, case):
    """A context left at its defaults (trace_own_leaf = 1): the hinted light rays of the frame's camera hits ARE the renderer's shadow rays
    with its marks, so the hinted query's counters are rtr_render's any-hit counters and the oracle's (own_leaf=True).  Checked on the CPU
    on the host-built tree: with the rule on, sponza_class has 1 ray that outgrows the LDS stack at this extent (the tail is in the
    numbers), sponza_mixed none, but 6 460 alpha tests in the frame."""
    W, H = 320, 184
    s = getattr(scenes, case)(W, H)
    ctx = api.Context(0)
    assert ctx.get_tunable("trace_own_leaf") == 1
    scene = api.Scene(ctx, s.desc)
    frame = api.Frame(ctx, W, H)
    try:
        p = api.make_params(W, H, spp=1, shadow_rays=3, collect_stats=1, pipeline=2)
        api.render(scene, s.camera, s.scene_info(0), p, frame)
        g = frame.stats()
        rays, hits = camera_hits(ctx, scene, s, W, H)
        lp = api.make_light_params(s.num_lights, 3, 0, W, 1)
        lr, leaves = api.light_rays(scene, rays, hits, lp, hints=True)
        cam_alpha = api.trace_rays(scene, rays, collect_stats=True).stats.numAlphaTests
        res = api.trace_occlusion(scene, lr, collect_stats=True, start_leaves=leaves)
        q = res.stats
        plain = api.trace_occlusion(scene, lr, collect_stats=True).stats
        ref = oracle.render(s.desc, s.camera, s.scene_info(0), p, bvh=scene.export_bvh(), threads=16, own_leaf=True)
        print(f"{case}: hinted rays {q.numRays} visits {q.numNodeVisits} tests {q.numTriTests} tail {q.tailRays} alpha {q.numAlphaTests}; "
              f"unhinted visits {plain.numNodeVisits} tests {plain.numTriTests}; own-leaf rays {ref.walk.ownLeafRays} stopped {ref.walk.ownLeafStopped}")
        assert int((_np(leaves) != 0).sum()) == ref.walk.ownLeafRays
        for name, o in (("rtr_render", g), ("oracle", ref.stats)):
            assert q.numRays == o.numShadowRays, f"{name}: rays {q.numRays} != {o.numShadowRays}"
            assert q.numNodeVisits == o.numShadowNodeVisits, f"{name}: node visits {q.numNodeVisits} != {o.numShadowNodeVisits}"
            assert q.numTriTests == o.numShadowTriTests, f"{name}: triangle tests {q.numTriTests} != {o.numShadowTriTests}"
            assert q.tailRays == o.shadowTailRays, f"{name}: tail rays {q.tailRays} != {o.shadowTailRays}"
            assert q.numAlphaTests == o.numAlphaTests - cam_alpha, f"{name}: alpha tests {q.numAlphaTests} != {o.numAlphaTests} - {cam_alpha}"
        assert q.numNodeVisits < plain.numNodeVisits, "the rule saves record visits"
        assert q.numRays == plain.numRays
        if case == "sponza_class":
            assert q.tailRays > 0
        if case == "sponza_mixed":
            assert q.numAlphaTests > 0
        assert q.ms > 0.0
        assert_same_bytes(res.occluded, api.trace_rays(scene, lr, any_hit=True).occluded, f"{case}, counting form")
        assert_same_bytes(api.trace_occlusion(scene, lr, start_leaves=leaves).occluded, res.occluded, f"{case}, timed form")
    finally:
        frame.close(); scene.close(); ctx.close()


# ---- 5. the composed route --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["cornell_box", "textured_room"])
def test_composed_route_own_leaf_equals_dense_and_the_renderer(gpu_ctx, scene_cache, case):
    if case == "cornell_box":
        s, w, h = scenes.cornell_box(128, 128, ltc=scenes.shipped_ltc()), 128, 128
    else:
        s, w, h = scenes.textured_room(160, 100, ltc=scenes.shipped_ltc()), 160, 100
    scene = api.Scene(gpu_ctx, s.desc)
    frame = api.Frame(gpu_ctx, w, h, ALL5)
    rays, hits = camera_hits(gpu_ctx, scene, s, w, h)
    for f in (0, 5):
        api.render(scene, s.camera, s.scene_info(f), api.make_params(w, h, spp=1, images=ALL5), frame)
        p = api.make_light_params(s.num_lights, 3, f, w, 1, ALL3)
        dense = api.direct_light(scene, rays, hits, p)
        own = api.direct_light(scene, rays, hits, p, occlusion="queued_own_leaf")
        chunks = api.direct_light(scene, rays, hits, p, occlusion="queued_own_leaf", max_ray_bytes=1 << 20)
        assert (_np(own.raw).view(np.uint32) == _np(dense.raw).view(np.uint32)).all(), f"{case} frame {f}: RtrRadiance bits"
        assert (_np(chunks.raw).view(np.uint32) == _np(dense.raw).view(np.uint32)).all(), f"{case} frame {f}: RtrRadiance bits, in chunks"
        hdr = frame.download(A.IMAGE_HDR).reshape(-1, 4)
        assert (_np(own.shadowed).view(np.uint32) == hdr[:, :3].view(np.uint32)).all(), f"{case} frame {f}: RTR_IMAGE_HDR"
    frame.close(); scene.close()


# ---- 6. housekeeping ----------------------------------------------------------------------------------------------------------------------------
def test_asynchronous_forms_on_torchs_stream(scene_cache):
    w, h = 128, 128
    s = scenes.cornell_box(w, h)
    ctx = api.Context(0)
    scene = api.Scene(ctx, s.desc)
    rays, hits = camera_hits(ctx, scene, s, w, h)
    p = api.make_light_params(s.num_lights, 3, 0, w, 1)
    ref_lr, ref_lv = api.light_rays(scene, rays, hits, p, hints=True)
    ref_own = api.hit_leaves(scene, hits).clone()
    ref = api.trace_rays(scene, ref_lr, any_hit=True).occluded.clone()
    fresh = api.Scene(ctx, s.desc)                             # its table is made by the asynchronous call below
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        ctx.set_stream(stream.cuda_stream)
        r2 = (rays * 0.5) * 2.0                                # the producer: torch work on the stream right before the calls (exact)
        lr, lv = api.light_rays(fresh, r2, hits, p, hints=True, asynchronous=True)
        own = api.hit_leaves(fresh, hits, asynchronous=True)
        q = api.trace_occlusion(fresh, lr, start_leaves=lv, asynchronous=True)
        total = q.occluded.to(torch.int64).sum()               # the consumer, on the same stream, no host join in between
        again = api.trace_occlusion(fresh, lr, start_leaves=own.repeat_interleave(lr.shape[0] // own.shape[0]), asynchronous=True)
        stream.synchronize()
        assert torch.equal(lr.view(torch.int32), ref_lr.view(torch.int32)) and torch.equal(lv, ref_lv) and torch.equal(own, ref_own)
        assert int(total) == int(ref.to(torch.int64).sum())
        assert torch.equal(q.occluded, ref) and torch.equal(again.occluded, ref)
        ctx.set_stream(None)
    with pytest.raises(ValueError):
        api.hit_leaves(scene, hits, asynchronous=True)         # the context is no longer on torch's current stream
    fresh.close(); scene.close(); ctx.close()


def test_repeated_hinted_calls_with_one_scratch_leave_nothing_behind(gpu_ctx, scene_cache):
    s = scenes.cornell_box(64, 64)
    scene = api.Scene(gpu_ctx, s.desc)
    st = scene.stats()
    lib = gpu_ctx.lib
    rng = np.random.default_rng(9)
    big = torch.from_numpy(mixed_rays(st, 150001, 5, 1500.0)).cuda()
    small = torch.from_numpy(mixed_rays(st, 777, 6, 1500.0)).cuda()
    pool = np.unique(_np(api.hit_leaves(scene, camera_hits(gpu_ctx, scene, s, 64, 64)[1])))
    hb = torch.from_numpy(rng.choice(pool, big.shape[0]).astype(np.int32)).cuda()
    hs = torch.from_numpy(rng.choice(pool, small.shape[0]).astype(np.int32)).cuda()
    need = api.occlusion_scratch_bytes(lib, big.shape[0])
    scratch = torch.randint(0, 256, (need,), dtype=torch.uint8, device="cuda")       # garbage in: the query initialises what it reads
    torch.cuda.synchronize()
    exp = {id(big): api.trace_rays(scene, big, any_hit=True).occluded, id(small): api.trace_rays(scene, small, any_hit=True).occluded}
    for rays, hints in ((big, hb), (small, None), (big, None), (big, hb), (small, hs)):
        occ = torch.full((rays.shape[0],), 7, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        assert lib.rtr_trace_occlusion_hinted(gpu_ctx.h, scene.h, A.VP(rays.data_ptr()), A.VP(hints.data_ptr()) if hints is not None else None,
                                              rays.shape[0], 0, A.VP(scratch.data_ptr()), need, A.VP(occ.data_ptr()), None) == 0
        assert_same_bytes(occ, exp[id(rays)], f"{rays.shape[0]} rays, shared scratch, hints {hints is not None}")
    scene.close()


def test_invalid_arguments(gpu_ctx, scene_cache):
    s = scenes.cornell_box(64, 64)
    scene = api.Scene(gpu_ctx, s.desc)
    lib, ctx = gpu_ctx.lib, gpu_ctx.h
    rays, hits = camera_hits(gpu_ctx, scene, s, 8, 8)
    p = api.make_light_params(s.num_lights, 3, 0, 8, 1)
    q = api.light_slots(scene, p)
    lr, lv = api.light_rays(scene, rays, hits, p, hints=True)
    n = 64 * q
    need = api.occlusion_scratch_bytes(lib, n)
    scratch = torch.empty(need, dtype=torch.uint8, device="cuda")
    occ = torch.empty(n, dtype=torch.uint8, device="cuda")
    pad = torch.zeros(n + 4, dtype=torch.int32, device="cuda")
    rp, hp, lp, sp, op = (A.VP(x.data_ptr()) for x in (lr, lv, hits, scratch, occ))
    call = lib.rtr_trace_occlusion_hinted
    assert call(ctx, scene.h, rp, hp, n, 0, sp, need, op, None) == 0
    assert call(ctx, scene.h, rp, None, n, A.QUERY_ANY | A.QUERY_OPAQUE, sp, need, op, None) == 0        # NULL hints: the unhinted call
    assert call(ctx, scene.h, rp, A.VP(pad.data_ptr() + 2), n, 0, sp, need, op, None) == INVALID        # misaligned startLeaves
    assert b"rtr_trace_occlusion_hinted: startLeaves is not 4-B aligned" in lib.rtr_last_error()
    assert call(ctx, scene.h, rp, A.VP(pad.data_ptr() + 4), n, 0, sp, need, op, None) == 0              # 4-B alignment is enough
    assert call(ctx, scene.h, rp, hp, n, 0, sp, need - 1, op, None) == INVALID and b"scratch" in lib.rtr_last_error()
    assert lib.rtr_trace_occlusion_hinted_async(ctx, scene.h, rp, hp, n, 4, sp, need, op) == INVALID     # flag value 4 stays unknown
    assert b"flag" in lib.rtr_last_error()
    assert call(ctx, scene.h, None, None, 0, 0, None, 0, None, None) == 0                               # no rays: nothing to do
    out = torch.empty(64, dtype=torch.int32, device="cuda")
    assert lib.rtr_hit_leaves(ctx, scene.h, lp, 64, None) == INVALID and b"leaves is null" in lib.rtr_last_error()
    assert lib.rtr_hit_leaves(ctx, scene.h, None, 64, A.VP(out.data_ptr())) == INVALID and b"hits is null" in lib.rtr_last_error()
    assert lib.rtr_hit_leaves(ctx, scene.h, A.VP(hits.data_ptr() + 4), 64, A.VP(out.data_ptr())) == INVALID and b"aligned" in lib.rtr_last_error()
    assert lib.rtr_hit_leaves(ctx, scene.h, None, 0, None) == 0
    rr = A.VP(rays.data_ptr())
    fn = lib.rtr_light_rays_hinted
    assert fn(ctx, scene.h, rr, lp, 64, C.byref(p), None, rp, None) == INVALID and b"outLeaves is null" in lib.rtr_last_error()
    assert fn(ctx, scene.h, rr, lp, 64, C.byref(p), None, rp, A.VP(pad.data_ptr() + 1)) == INVALID and b"outLeaves is not 4-B aligned" in lib.rtr_last_error()
    assert fn(ctx, scene.h, rr, lp, 64, C.byref(p), None, None, hp) == INVALID and b"outRays is null" in lib.rtr_last_error()
    assert fn(ctx, scene.h, None, None, 0, C.byref(p), None, None, None) == 0
    assert api.hit_leaves(scene, hits[:0]).shape == (0,)
    for bad in (lv[:-1], lv.to(torch.int64), lv.cpu(), lv.float(), _np(lv)):
        with pytest.raises(ValueError):
            api.trace_occlusion(scene, lr, start_leaves=bad)
    # a scene of another context of the same device is served, table and all
    ctx2 = api.Context(0)
    assert torch.equal(api.hit_leaves(scene, hits, ctx=ctx2), api.hit_leaves(scene, hits))
    assert_same_bytes(api.trace_occlusion(scene, lr, ctx=ctx2, start_leaves=lv).occluded, api.trace_rays(scene, lr, any_hit=True).occluded, "another context")
    ctx2.close(); scene.close()


# ---- 7. the renderer is untouched ---------------------------------------------------------------------------------------------------------------
def test_hinted_queries_change_nothing_in_a_render(scene_cache):
    W, H = 128, 128
    s = scenes.cornell_box(W, H)
    ctx = api.Context(0)
    scene = api.Scene(ctx, s.desc)
    frame = api.Frame(ctx, W, H)
    fields = [f for f, _ in A.rtr_frame_stats._fields_ if f.startswith("num") or f.endswith("TailRays")]
    assert "numShadowNodeVisits" in fields and "numTriTests" in fields

    def render():
        out = []
        for stats in (1, 0):
            api.render(scene, s.camera, s.scene_info(2), api.make_params(W, H, spp=2, shadow_rays=3, collect_stats=stats, pipeline=2), frame)
            out.append(frame.download().copy())
            if stats:
                g = frame.stats()
                out.append([getattr(g, f) for f in fields])
        return out

    before = render()
    rays, hits = camera_hits(ctx, scene, s, W, H)
    lr, lv = api.light_rays(scene, rays, hits, api.make_light_params(s.num_lights, 3, 2, W, 1), hints=True)
    api.trace_occlusion(scene, lr, collect_stats=True, start_leaves=lv)
    api.trace_occlusion(scene, lr, start_leaves=lv)
    api.hit_leaves(scene, hits)
    after = render()
    assert (before[0] == after[0]).all() and (before[2] == after[2]).all()
    assert before[1] == after[1], dict(zip(fields, zip(before[1], after[1])))
    frame.close(); scene.close(); ctx.close()
