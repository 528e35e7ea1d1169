"""The queued occlusion query (rtr_trace_occlusion) on the device.  Every comparison is at tolerance 0:
  * its bytes are the dense query's (rtr_trace_rays, RTR_QUERY_ANY) and brute force's;
  * its work counters are the renderer's any-hit walk's — the CPU oracle's and rtr_render's with trace_own_leaf = 0 — so it IS that walk;
  * the composed direct-light route through it gives the dense route's and the renderer's bits;
  * deep rays take the tail, moved instances are seen, stream order holds, bad arguments are refused, and the renderer is untouched."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from realtimeraytracer_amd import _abi as A
from realtimeraytracer_amd import api, host, scenes

pytestmark = pytest.mark.gpu

MISS = 0xffffffff
F3 = A.f32 * 3
INVALID = -1
ALL3 = A.LIGHT_SHADOWED | A.LIGHT_UNSHADOWED | A.LIGHT_ANALYTIC
ALL5 = A.IMAGES_RAYGEN5 | A.IMG_BIT(A.IMAGE_HDR)


def _np(x):
    return x.cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)


def random_rays(lo, hi, n, seed, tmax_scale):
    """tests/test_gpu_query.py's generator, re-stated: origins in and around the box, unit directions, tmin from {0, 0.001, 0.5}, tmax far,
    infinite, short, below tmin or equal to it"""
    rng = np.random.default_rng(seed)
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    ext = hi - lo
    o = lo + ext * rng.uniform(-0.2, 1.2, (n, 3))
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    tmin = rng.choice(np.array([0.0, 0.001, 0.5], np.float32), n)
    tmax = rng.choice(np.array([10000.0, np.inf], np.float32), n).astype(np.float64)
    part = rng.uniform(0, 1, n)
    tmax = np.where(part < 0.3, rng.uniform(0.0, 1.0, n) * tmax_scale, tmax)         # short rays
    tmax = np.where(part > 0.95, tmin - rng.uniform(0, 1, n), tmax)                   # tmax < tmin
    tmax = np.where((part > 0.9) & (part <= 0.95), tmin, tmax)                         # tmax == tmin
    r = np.zeros((n, 8), np.float32)
    r[:, 0:3], r[:, 3], r[:, 4:7], r[:, 7] = o, tmin, d, tmax
    return r


def mixed_rays(st, n, seed, tmax_scale):
    """random rays with random tmin (up to a good part of the scene: it must matter) and, sprinkled in, null rays and degenerate ones"""
    r = random_rays(st.boundsMin[:], st.boundsMax[:], n, seed, tmax_scale)
    rng = np.random.default_rng(seed + 1000)
    far = rng.uniform(0, 1, n) < 0.3
    r[far, 3] = (rng.uniform(0.0, 0.5, n) * tmax_scale).astype(np.float32)[far]          # tmin well inside the scene
    kind = rng.integers(0, 40, n)
    r[kind == 0] = 0.0                                                                    # the null ray
    r[kind == 1, 4:7] = 0.0                                                               # zero direction
    r[kind == 2, rng.integers(0, 3)] = np.nan                                             # origin not finite
    r[kind == 3, 4 + rng.integers(0, 3)] = np.inf                                         # direction not finite
    r[kind == 4, 7] = np.nan
    r[kind == 5, 3] = np.nan
    return r


def assert_same_bytes(got, exp, what):
    got, exp = _np(got), _np(exp)
    assert got.dtype == np.uint8 and got.shape == exp.shape
    assert set(np.unique(got).tolist()) <= {0, 1}, f"{what}: bytes other than 0 and 1: {np.unique(got).tolist()}"
    bad = got != exp
    if bad.any():
        k = np.nonzero(bad)[0][:8]
        raise AssertionError(f"{what}: {int(bad.sum())} of {len(got)} rays differ; first {k.tolist()}: queued {got[k].tolist()} expected {exp[k].tolist()}")


def camera_light_rays(ctx, scene, s, w, h, frame):
    rays = api.camera_rays(ctx, s.camera, w, h, 1)
    hits = api.trace_rays(scene, rays)
    p = api.make_light_params(s.num_lights, 3, frame, w, 1)
    return rays, hits, p, api.light_rays(scene, rays, hits, p)


# ---- 1. the dense query's bytes -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["cornell_box", "textured_room", "sponza_mixed"])
def test_same_bytes_as_the_dense_query(gpu_ctx, scene_cache, case):
    w, h = (128, 128) if case == "cornell_box" else (160, 100)
    s = getattr(scenes, case)(w, h)
    scene = api.Scene(gpu_ctx, s.desc)
    st = scene.stats()
    if case != "cornell_box":
        raw = np.frombuffer(scene.export_bvh()[1], dtype=np.uint32).reshape(-1, 12)
        assert (raw[:, 11] & 1).any(), "the scene must hold alpha-tested triangles"
    lr = camera_light_rays(gpu_ctx, scene, s, w, h, 0)[3]
    assert (~_np(lr).any(1)).any(), "the light rays hold null slots"
    diag = float(np.linalg.norm(np.array(st.boundsMax[:]) - np.array(st.boundsMin[:])))
    n = 200003                                                  # not a multiple of 64, of the batch or of a workgroup's share
    rnd = torch.from_numpy(mixed_rays(st, n, 31, diag)).cuda()
    differ = 0
    for name, rays in (("light rays", lr), ("random rays", rnd)):
        dense = {}
        for opaque in (False, True):
            dense[opaque] = api.trace_rays(scene, rays, any_hit=True, opaque=opaque).occluded
            q = api.trace_occlusion(scene, rays, opaque=opaque)
            assert q.occluded.dtype == torch.uint8 and q.occluded.shape == (rays.shape[0],)
            assert_same_bytes(q.occluded, dense[opaque], f"{case}, {name}, opaque={opaque}")
            assert bool(dense[opaque].any()) and not bool(dense[opaque].all())
        differ += int((dense[False] != dense[True]).sum())
    if case != "cornell_box":
        assert differ > 0, "skipping the opacity map must change some answers"
    # numpy in, numpy out
    qn = api.trace_occlusion(scene, _np(rnd)[:1000])
    assert isinstance(qn.occluded, np.ndarray)
    assert_same_bytes(qn.occluded, _np(api.trace_rays(scene, rnd[:1000].contiguous(), any_hit=True).occluded), "numpy rays")


# ---- 2. brute force's bytes -------------------------------------------------------------------------------------------------------------
def brute_force_any(oracle, bvh, rays):
    """is there a triangle record with oracle_mt (the kernels' Moeller-Trumbore, t > tmin) and t < tmax?  Opaque scenes only."""
    raw = np.frombuffer(bvh[1], dtype=np.uint32).reshape(-1, 12).copy()
    flt = raw.view(np.float32)
    assert not (raw[:, 11] & 1).any()
    L = oracle.lib()
    tris = [(F3(*flt[j, 0:3]), F3(*flt[j, 4:7]), F3(*flt[j, 8:11])) for j in range(len(raw))]
    out = np.zeros(len(rays), np.uint8)
    tuv = (A.f32 * 3)()
    for k, r in enumerate(rays):
        tmin, tmax = r[3], r[7]
        if not (tmax > tmin) or not np.isfinite(r[[0, 1, 2, 4, 5, 6]]).all() or not r[4:7].any():
            continue
        o, d = F3(*r[0:3]), F3(*r[4:7])
        for v0, e1, e2 in tris:
            if L.oracle_mt(o, d, v0, e1, e2, float(tmin), tuv) and np.float32(tuv[0]) < tmax:
                out[k] = 1
                break
    return out


def test_same_bytes_as_brute_force(gpu_ctx, oracle, scene_cache):
    s = scenes.cornell_box(64, 64)
    scene = api.Scene(gpu_ctx, s.desc)
    st = scene.stats()
    diag = float(np.linalg.norm(np.array(st.boundsMax[:]) - np.array(st.boundsMin[:])))
    rays = mixed_rays(st, 3001, 7, diag)
    exp = brute_force_any(oracle, scene.export_bvh(), rays)
    assert 0.02 < exp.mean() < 0.98
    assert_same_bytes(api.trace_occlusion(scene, rays).occluded, exp, "cornell, brute force")
    # tmin is the ray's own: moved past the first occluder's distance it changes answers, and both sides see that
    moved = rays.copy()
    moved[:, 3] = np.float32(0.25 * diag)
    exp2 = brute_force_any(oracle, scene.export_bvh(), moved)
    assert (exp2 != exp).any()
    assert_same_bytes(api.trace_occlusion(scene, moved).occluded, exp2, "cornell, brute force, tmin moved")


# ---- 3. the renderer's walk ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["sponza_mixed", "sponza_class"])
def test_counters_equal_the_renderers_any_hit_walk(oracle, scene_cache, case):
    """The light rays api.light_rays makes of a frame's camera hits ARE the renderer's shadow rays, so the queued query's counters are the
    any-hit counters of that frame rendered with trace_own_leaf = 0 (the one rule an RtrRay cannot carry).  Cases picked on the CPU: the
    oracle counts 3 (sponza_mixed) and 1 (sponza_class) shadow rays that outgrow the LDS stack at this extent, so the 4-wide walk and the
    BVH2 tail are both in the numbers; sponza_mixed has alpha tests among them."""
    W, H = 320, 184
    s = getattr(scenes, case)(W, H)
    ctx = api.Context(0)
    ctx.set_tunable("trace_own_leaf", 0)
    scene = api.Scene(ctx, s.desc)
    frame = api.Frame(ctx, W, H)
    try:
        p = api.make_params(W, H, spp=1, shadow_rays=3, collect_stats=1, pipeline=2)
        api.render(scene, s.camera, s.scene_info(0), p, frame)
        g = frame.stats()
        rays, hits, lp, lr = camera_light_rays(ctx, scene, s, W, H, 0)
        cam_alpha = api.trace_rays(scene, rays, collect_stats=True).stats.numAlphaTests
        res = api.trace_occlusion(scene, lr, collect_stats=True)
        q = res.stats
        ref = oracle.render(s.desc, s.camera, s.scene_info(0), p, bvh=scene.export_bvh(), threads=16, own_leaf=False).stats
        assert ref.shadowTailRays > 0, "the case must exercise the tail"
        for name, o in (("rtr_render", g), ("oracle", ref)):
            assert q.numRays == o.numShadowRays, f"{name}: rays {q.numRays} != {o.numShadowRays}"
            assert q.numNodeVisits == o.numShadowNodeVisits, f"{name}: node visits {q.numNodeVisits} != {o.numShadowNodeVisits}"
            assert q.numTriTests == o.numShadowTriTests, f"{name}: triangle tests {q.numTriTests} != {o.numShadowTriTests}"
            assert q.tailRays == o.shadowTailRays, f"{name}: tail rays {q.tailRays} != {o.shadowTailRays}"
            assert q.numAlphaTests == o.numAlphaTests - cam_alpha, f"{name}: alpha tests {q.numAlphaTests} != {o.numAlphaTests} - {cam_alpha}"
        if case == "sponza_mixed":
            assert q.numAlphaTests > 0
        assert q.ms > 0.0
        assert_same_bytes(res.occluded, api.trace_rays(scene, lr, any_hit=True).occluded, f"{case}, counting form")
        assert_same_bytes(api.trace_occlusion(scene, lr).occluded, res.occluded, f"{case}, timed form")
    finally:
        frame.close(); scene.close(); ctx.close()


# ---- 4. the composed route ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["cornell_box", "textured_room"])
def test_composed_route_queued_equals_dense_and_the_renderer(gpu_ctx, scene_cache, case):
    if case == "cornell_box":
        s, w, h = scenes.cornell_box(128, 128, ltc=scenes.shipped_ltc()), 128, 128
    else:
        s, w, h = scenes.textured_room(160, 100, ltc=scenes.shipped_ltc()), 160, 100
    scene = api.Scene(gpu_ctx, s.desc)
    frame = api.Frame(gpu_ctx, w, h, ALL5)
    rays = api.camera_rays(gpu_ctx, s.camera, w, h, 1)
    hits = api.trace_rays(scene, rays)
    for f in (0, 5):
        api.render(scene, s.camera, s.scene_info(f), api.make_params(w, h, spp=1, images=ALL5), frame)
        p = api.make_light_params(s.num_lights, 3, f, w, 1, ALL3)
        dense = api.direct_light(scene, rays, hits, p)
        queued = api.direct_light(scene, rays, hits, p, occlusion="queued")
        chunks = api.direct_light(scene, rays, hits, p, occlusion="queued", max_ray_bytes=1 << 20)
        assert (_np(queued.raw).view(np.uint32) == _np(dense.raw).view(np.uint32)).all(), f"{case} frame {f}: RtrRadiance bits"
        assert (_np(chunks.raw).view(np.uint32) == _np(dense.raw).view(np.uint32)).all(), f"{case} frame {f}: RtrRadiance bits, in chunks"
        hdr = frame.download(A.IMAGE_HDR).reshape(-1, 4)
        assert (_np(queued.shadowed).view(np.uint32) == hdr[:, :3].view(np.uint32)).all(), f"{case} frame {f}: RTR_IMAGE_HDR"
        for name, img in (("shadowed", A.IMAGE_SHADOWED), ("unshadowed", A.IMAGE_UNSHADOWED), ("analytic", A.IMAGE_ANALYTIC)):
            got = _np(api.tonemap_pack(gpu_ctx, getattr(queued, name))).view(np.uint32)
            assert (got == _np(api.tonemap_pack(gpu_ctx, getattr(dense, name))).view(np.uint32)).all()
            d = int((got != frame.download(img).reshape(-1)).sum())
            assert d == 0, f"{case} frame {f}: {d} of {w * h} pixels differ in the {name} image"
    with pytest.raises(ValueError):
        api.direct_light(scene, rays, hits, p, occlusion="sparse")


# ---- 5. deep rays ---------------------------------------------------------------------------------------------------------------------------
def _deep_scene(ctx):
    """tests/test_gpu_query.py's construction, re-stated: a squeezed row of 2^19 triangles 0.01 apart whose rays, looking down its length
    from its head, keep one pending far child per level of the ~20-level tree"""
    N = 1 << 19
    x = np.arange(N, dtype=np.float32) * np.float32(0.01)
    tri = np.stack([np.stack([x, np.full(N, -1.0, np.float32), np.full(N, -0.3, np.float32)], 1),
                    np.stack([x + np.float32(0.006), np.full(N, -1.0, np.float32), np.zeros(N, np.float32)], 1),
                    np.stack([x, np.full(N, -1.0, np.float32), np.full(N, 0.3, np.float32)], 1)], 1).reshape(-1, 3)
    wall = np.array([[N * 0.01 + 1.0, -4.0, -4.0], [N * 0.01 + 1.0, 4.0, -4.0], [N * 0.01 + 1.0, 0.0, 4.0]], np.float32)
    verts = np.concatenate([wall, tri])
    V = np.zeros((len(verts), 12), np.float32)
    V[:, :3] = verts
    idx = np.concatenate([np.array([0, 1, 2], np.uint32), np.arange(3 * N, dtype=np.uint32)])
    meshes = (A.RtrMesh * 2)()
    for m, (vo, io, vc, ic) in zip(meshes, [(0, 0, 3, 3), (3, 3, 3 * N, 3 * N)]):
        m.vertexOffset, m.indexOffset, m.vertexCount, m.indexCount, m.isOpaque = vo, io, vc, ic, 1
    inst = (A.RtrInstance * 2)()
    for i, (mi, ci) in zip(inst, [(0, 0), (1, 1)]):
        i.meshIndex, i.customIndex = mi, ci
        for k, val in enumerate((1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0)):
            i.transform[k] = float(val)
    objs = (A.RtrObjectInfo * 2)()
    for o, (vo, io) in zip(objs, [(0, 0), (3, 3)]):
        o.vertexOffset, o.indexOffset = vo, io
        o.color[0] = o.color[1] = o.color[2] = 0.8
    d = A.rtr_scene_desc()
    d.vertices = V.ctypes.data_as(C.POINTER(A.RtrVertex)); d.numVertices = len(V)
    d.indices = idx.ctypes.data_as(C.POINTER(A.u32)); d.numIndices = len(idx)
    d.meshes, d.numMeshes = meshes, 2
    d.instances, d.numInstances = inst, 2
    d.objects, d.numObjects = objs, 2
    d.skyColor[0] = d.skyColor[1] = d.skyColor[2] = 0.5
    keep = (V, idx, meshes, inst, objs)
    scene = api.Scene(ctx, d)
    assert scene.stats().maxDepth > 16
    end = float(N) * 0.01
    cam = host.Camera(0.004, (-30.0, -0.995, 0.0), (0.8 * end, -1.0, 0.0), (0.0, 1.0, 0.0), 16, 8).getGPUData()
    return d, keep, scene, cam


def test_deep_rays_take_the_tail(gpu_ctx, oracle):
    """Two fans of camera rays down the length of the squeezed row, so that brute force (the oracle's primary hits without a tree) knows
    their answers.  From the head: they end on the wall behind the row, which the far-exit-first walk finds at once.  From the wall end,
    looking back: they graze the whole row and leave the scene, every child box of every record on their way — the any-hit walk then holds
    up to three pending children per level of the 4-wide tree and outgrows its 16 entries."""
    d, keep, scene, cam = _deep_scene(gpu_ctx)
    W, H, S = 16, 8, 2
    end = float(1 << 19) * 0.01
    back = host.Camera(0.004, (end + 0.5, -0.995, 0.0), (0.2 * end, -1.0, 0.0), (0.0, 1.0, 0.0), W, H).getGPUData()
    p = api.make_params(W, H, spp=S)
    rays = torch.cat([api.camera_rays(gpu_ctx, c, W, H, S) for c in (cam, back)])
    exp = np.concatenate([(oracle.primary_hits(d, c, p, bvh=None, threads=16)[3] != MISS).astype(np.uint8) for c in (cam, back)])     # brute force
    assert exp.any() and not exp.all()
    r = api.trace_occlusion(scene, rays, collect_stats=True)
    assert r.stats.tailRays > 0 and r.stats.numRays == 2 * W * H * S
    assert_same_bytes(r.occluded, exp, "deep rays, counting form")
    assert_same_bytes(api.trace_occlusion(scene, rays).occluded, exp, "deep rays, timed form")
    # a list of 4 entries: more rays are abandoned than it holds, and the tail finds them by their sentinel (librtr_hip_test.so only)
    os.environ["RTR_QUERY_REDO_CAP"] = "4"
    try:
        hctx = api.Context(0, test_hooks=True)
        hscene = api.Scene(hctx, d)
        hr = api.trace_occlusion(hscene, rays, collect_stats=True)
        assert hr.stats.tailRays > 4
        assert_same_bytes(hr.occluded, exp, "deep rays, list overflowed, counting form")
        assert_same_bytes(api.trace_occlusion(hscene, rays).occluded, exp, "deep rays, list overflowed, timed form")
        hscene.close(); hctx.close()
    finally:
        del os.environ["RTR_QUERY_REDO_CAP"]


# ---- 6. dynamic scenes and plumbing ---------------------------------------------------------------------------------------------------------
def test_moved_instances_are_seen(gpu_ctx, oracle, scene_cache):
    s = scenes.cornell_box(64, 64)
    scene = api.Scene(gpu_ctx, s.desc)
    st = scene.stats()
    rays = random_rays(st.boundsMin[:], st.boundsMax[:], 1500, seed=21, tmax_scale=1500.0)
    before = api.trace_occlusion(scene, rays).occluded
    inst = [A.RtrInstance.from_buffer_copy(s.desc.instances[i]) for i in range(s.desc.numInstances)]
    for k, i in enumerate(inst):
        if i.customIndex >= s.num_lights:
            i.transform[3] += 40.0 * (k % 3)
            i.transform[7] -= 25.0 * (k % 2)
    scene.update_instances(inst)
    after = api.trace_occlusion(scene, rays).occluded
    assert_same_bytes(after, brute_force_any(oracle, scene.export_bvh(), rays), "after update_instances")
    assert (after != before).any()


def test_asynchronous_query_on_torchs_stream(scene_cache):
    s = scenes.cornell_box(128, 128)
    ctx = api.Context(0)
    scene = api.Scene(ctx, s.desc)
    st = scene.stats()
    base = torch.from_numpy(random_rays(st.boundsMin[:], st.boundsMax[:], 1 << 20, seed=3, tmax_scale=1500.0)).cuda()
    ref = api.trace_rays(scene, base, any_hit=True).occluded.clone()
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        ctx.set_stream(stream.cuda_stream)
        rays = (base * 0.5) * 2.0                              # the producer: torch work on the stream right before the query (exact)
        q = api.trace_occlusion(scene, rays, asynchronous=True)
        total = q.occluded.to(torch.int64).sum()               # the consumer, on the same stream, no host join in between
        again = api.trace_occlusion(scene, rays, asynchronous=True)      # the same scratch, the next query
        stream.synchronize()
        assert int(total) == int(ref.to(torch.int64).sum())
        assert torch.equal(q.occluded, ref) and torch.equal(again.occluded, ref)
        with pytest.raises(ValueError):
            api.trace_occlusion(scene, rays, asynchronous=True, collect_stats=True)
        ctx.set_stream(None)
    with pytest.raises(ValueError):
        api.trace_occlusion(scene, rays, asynchronous=True)    # the context is no longer on torch's current stream
    scene.close(); ctx.close()


def test_repeated_calls_with_one_scratch_leave_nothing_behind(gpu_ctx, scene_cache):
    s = scenes.cornell_box(64, 64)
    scene = api.Scene(gpu_ctx, s.desc)
    st = scene.stats()
    lib = gpu_ctx.lib
    big = torch.from_numpy(mixed_rays(st, 150001, 5, 1500.0)).cuda()
    small = torch.from_numpy(mixed_rays(st, 777, 6, 1500.0)).cuda()
    need = api.occlusion_scratch_bytes(lib, big.shape[0])
    scratch = torch.randint(0, 256, (need,), dtype=torch.uint8, device="cuda")       # garbage in: the query initialises what it reads
    torch.cuda.synchronize()
    exp = {id(big): api.trace_rays(scene, big, any_hit=True).occluded, id(small): api.trace_rays(scene, small, any_hit=True).occluded}
    for rays in (big, small, big, big, small):
        occ = torch.full((rays.shape[0],), 7, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        assert lib.rtr_trace_occlusion(gpu_ctx.h, scene.h, A.VP(rays.data_ptr()), rays.shape[0], 0, A.VP(scratch.data_ptr()), need,
                                       A.VP(occ.data_ptr()), None) == 0
        assert_same_bytes(occ, exp[id(rays)], f"{rays.shape[0]} rays, shared scratch")


def test_invalid_arguments(gpu_ctx, scene_cache):
    s = scenes.cornell_box(64, 64)
    scene = api.Scene(gpu_ctx, s.desc)
    lib, ctx = gpu_ctx.lib, gpu_ctx.h
    rays = api.camera_rays(gpu_ctx, s.camera, 8, 8, 1)
    need = api.occlusion_scratch_bytes(lib, 64)
    scratch = torch.empty(need + 16, dtype=torch.uint8, device="cuda")
    occ = torch.empty(64 + 16, dtype=torch.uint8, device="cuda")
    rp, sp, op = A.VP(rays.data_ptr()), A.VP(scratch.data_ptr()), A.VP(occ.data_ptr())
    call = lib.rtr_trace_occlusion
    assert call(ctx, scene.h, rp, 64, 0, sp, need, op, None) == 0
    assert call(ctx, scene.h, rp, 64, A.QUERY_ANY | A.QUERY_OPAQUE, sp, need, op, None) == 0            # RTR_QUERY_ANY is accepted and ignored
    assert call(ctx, scene.h, rp, 64, 0, sp, need - 1, op, None) == INVALID                             # scratch too small
    assert b"scratch" in lib.rtr_last_error() and str(need).encode() in lib.rtr_last_error()
    assert call(ctx, scene.h, rp, 64, 0, A.VP(scratch.data_ptr() + 8), need, op, None) == INVALID       # misaligned
    assert b"aligned" in lib.rtr_last_error()
    assert call(ctx, scene.h, A.VP(rays.data_ptr() + 4), 64, 0, sp, need, op, None) == INVALID
    assert call(ctx, scene.h, rp, 64, 0, sp, need, A.VP(occ.data_ptr() + 1), None) == INVALID
    for args in ((None, 64, 0, sp, need, op), (rp, 64, 0, None, need, op), (rp, 64, 0, sp, need, None)):
        assert call(ctx, scene.h, *args, None) == INVALID
        assert b"null" in lib.rtr_last_error()
    assert lib.rtr_trace_occlusion_async(ctx, scene.h, rp, 64, 4, sp, need, op) == INVALID              # unknown flag bit
    assert b"flag" in lib.rtr_last_error()
    assert lib.rtr_trace_occlusion_async(None, scene.h, rp, 64, 0, sp, need, op) == INVALID
    assert call(ctx, scene.h, None, 0, 0, None, 0, None, None) == 0                                     # no rays: nothing to do
    assert api.trace_occlusion(scene, rays[:0]).occluded.shape == (0,)
    if torch.cuda.device_count() > 1:
        other = api.Context(1)
        assert call(other.h, scene.h, rp, 64, 0, sp, need, op, None) == INVALID                         # scene on another device
        assert b"device" in lib.rtr_last_error()
        other.close()
    for bad in (rays[:, :7].contiguous(), rays.double(), rays.cpu(), rays.t().contiguous().t(), rays[:, 0]):
        with pytest.raises(ValueError):
            api.trace_occlusion(scene, bad)
    # a scene of another context of the same device is served
    ctx2 = api.Context(0)
    assert_same_bytes(api.trace_occlusion(scene, rays, ctx=ctx2).occluded, api.trace_rays(scene, rays, any_hit=True).occluded, "another context")
    ctx2.close()


# ---- 7. the renderer is untouched -------------------------------------------------------------------------------------------------------------
def test_a_queued_query_changes_nothing_in_a_render(scene_cache):
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
    st = scene.stats()
    rays = torch.from_numpy(mixed_rays(st, 100000, 2, 1500.0)).cuda()
    api.trace_occlusion(scene, rays, collect_stats=True)
    api.trace_occlusion(scene, rays)
    after = render()
    assert (before[0] == after[0]).all() and (before[2] == after[2]).all()
    assert before[1] == after[1], dict(zip(fields, zip(before[1], after[1])))
    frame.close(); scene.close(); ctx.close()
