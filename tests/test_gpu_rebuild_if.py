"""rtr_scene_rebuild_if_async on the device: the rebuild policy decided by the stream.  The reference is always a SYNCHRONOUS TWIN driven
by the calls that existed before — update_vertices, tree_cost, rebuild("device"), update_vertices_or_rebuild — never the code under
test: the twin's tree_cost().sah is what the decide kernel must have looked at (as float64 BITS: one function, kernels/rtr_tree_sah.h,
on both sides), its cost after a build is the baseline, and the two scenes must hold the same bytes and answer alike.
`room` has 14 triangles and no device tree (test_gpu_rebuild_async.py): its case holds the prepare refusal."""
import struct
import time

import numpy as np
import pytest
import torch

import test_gpu_rebuild_async as ra
import test_gpu_update_async as ua
import test_gpu_vertex_update as vu
from realtimeraytracer_amd import _abi as A
from realtimeraytracer_amd import api
from test_gpu_bvh import _render, _with_flags
from test_gpu_occlusion import assert_same_bytes
from test_gpu_rebuild_async import L, P, _points_case, _positions, _rays_at, assert_stats, device_scene, prepared, status
from test_gpu_update_async import _filler, _filler_ms, full, on_device
from test_gpu_vertex_update import SIZES, _np, _setup, changed_ranges, far, snapshot, verts_of
from test_rebuild_abi import empty_desc

pytestmark = pytest.mark.gpu

INF = float("inf")
WHO = "rtr_scene_rebuild_if_async"
PREPARE = "rtr_scene_prepare_async_rebuild_if"


@pytest.fixture(scope="module", autouse=True)
def _cleanup():
    yield
    vu._setups.clear(); ua._grid.clear()


def bits(x):
    return struct.pack("<d", float(x))


def policy_scene(ctx, desc):
    b = device_scene(ctx, desc)
    b.prepare_async_rebuild_if()
    return b


def frames_of(s, steps=6):
    """the ranges of step k = 1 .. steps: the vertices `far` moves, a fraction k / steps of the way from the original (the runs are the
    same at every step; the last step is `far` itself)"""
    old = verts_of(s.desc)
    new = far(s.desc, old)
    runs = changed_ranges(old, new)

    def ranges(k):
        f = k / steps
        pos = new[:, 0:3] if k == steps else (old[:, 0:3].astype(np.float64) * (1.0 - f) + new[:, 0:3].astype(np.float64) * f).astype(np.float32)
        return [(a, np.ascontiguousarray(pos[a:a + len(p)]), n) for a, p, n in runs]

    return old, new, ranges


def assert_same_answers(ctx, s, b, a, what):
    st = a.stats()
    lo, hi = np.array(st.boundsMin[:]), np.array(st.boundsMax[:])
    cam = _np(api.camera_rays(ctx, s.camera, 64, 48, 1))
    rays = np.ascontiguousarray(np.concatenate([cam[::3], vu.random_rays(lo, hi, 1500, 7, float(np.linalg.norm(hi - lo)))]))
    ha, hb = api.trace_rays(a, rays), api.trace_rays(b, rays)
    assert hb.hits.view(np.uint32).tolist() == ha.hits.view(np.uint32).tolist(), f"{what}: closest hits"
    assert (np.asarray(hb.custom_index) != 0xffffffff).any(), f"{what}: some rays hit"
    assert_same_bytes(api.trace_rays(b, rays, any_hit=True).occluded, api.trace_rays(a, rays, any_hit=True).occluded, f"{what}: any-hit")
    assert_same_bytes(api.trace_occlusion(b, rays).occluded, api.trace_occlusion(a, rays).occluded, f"{what}: queued occlusion")
    p = api.make_params(64, 48, spp=1)
    fa, fb = _render(ctx, a, s, p, frame_no=1), _render(ctx, b, s, p, frame_no=1)
    assert np.array_equal(fb.download(), fa.download()), f"{what}: image"
    fa.close(); fb.close()


# ---- 1. both decisions, forced, over a run of frames --------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["bunny", "cornell"])
def test_both_decisions_forced_over_a_run_of_frames(gpu_ctx, scene_cache, name):
    """the threshold is put 0.1 % under (odd steps) or over (even steps) the ratio the twin measures — many orders above double
    rounding — so both decisions occur whatever the costs are"""
    s = _setup(name)
    _, _, ranges = frames_of(s)
    a, b = device_scene(gpu_ctx, s.desc), policy_scene(gpu_ctx, s.desc)
    cls = b.stats().stackEntries
    base = a.tree_cost().sah
    st = b.rebuild_if_status()
    assert (st.evaluated, st.rebuilt, st.last_sah, st.last_decision) == (0, 0, 0.0, None)
    assert bits(st.built_sah) == bits(base), "the baseline of prepare is rtr_scene_tree_cost's sah"
    b.prepare_async_rebuild_if()
    assert bits(b.rebuild_if_status().built_sah) == bits(base), "prepare is idempotent"
    rebuilt = 0
    for k in range(1, 7):
        r = ranges(k)
        a.update_vertices(r)
        x = a.tree_cost().sah
        assert x > 0.0 and base > 0.0, f"premise: positive costs ({x}, {base})"
        b.update_vertices_async(on_device(r))
        if k % 2:
            a.rebuild("device")
            assert a.stats().maxDepth <= cls, "premise: the rebuilt tree fits the stack class, so the commit is not refused"
            b.rebuild_if_async(0.999 * x / base)
            base = a.tree_cost().sah
            rebuilt += 1
        else:
            b.rebuild_if_async(1.001 * x / base)
        st = b.rebuild_if_status()
        print(f"{name} step {k}: sah {x!r}, baseline {base!r}, decision {st.last_decision}")
        assert bits(st.last_sah) == bits(x), f"step {k}: the device looked at {st.last_sah!r}, the host computes {x!r}"
        assert st.last_decision is bool(k % 2), f"step {k}"
        assert bits(st.built_sah) == bits(base), f"step {k}: baseline {st.built_sah!r} != the twin's {base!r}"
        assert (st.evaluated, st.rebuilt) == (k, rebuilt)
    assert full(b) == full(a)
    assert_stats(b, a, skip=("stackEntries",))
    us = b.update_status()
    assert (us.enqueued, us.refused) == (12, 0)
    assert_same_answers(gpu_ctx, s, b, a, name)
    a.close(); b.close()


# ---- 2. the Python policies agree ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("above", [0.0, INF, 1.0])
def test_the_python_policies_agree(gpu_ctx, scene_cache, above):
    s = _setup("bunny")
    _, _, ranges = frames_of(s)
    a, b, c = device_scene(gpu_ctx, s.desc), policy_scene(gpu_ctx, s.desc), prepared(gpu_ctx, s.desc)
    cls = b.stats().stackEntries
    decisions = []
    for k in range(1, 7):
        r = ranges(k)
        decisions.append(a.update_vertices_or_rebuild(r, rebuild_above=above, rebuild_build="device"))
        assert a.stats().maxDepth <= cls, "premise: no commit is refused for its depth"
        assert b.update_vertices_or_rebuild_async(on_device(r), above) is None
        if above == INF:
            c.update_vertices(r)                                         # refit only
        elif above == 0.0:
            c.update_vertices_async(on_device(r)); c.rebuild_async()     # the unconditional enqueued rebuild, every frame
        st = b.rebuild_if_status()
        assert (st.evaluated, st.rebuilt, st.last_decision) == (k, sum(decisions), decisions[-1]), f"step {k}: the twin decided {decisions}"
    print(f"rebuild_above {above}: the twin decided {decisions}")
    if above == 0.0:
        assert all(decisions)
    if above == INF:
        assert not any(decisions)
    assert full(b) == full(a)
    if above != 1.0:
        assert full(b) == full(c)
    us = b.update_status()
    assert (us.enqueued, us.refused) == (12, 0)
    a.close(); b.close(); c.close()


# ---- 3. a skip leaves every byte, table and hint ------------------------------------------------------------------------------------
def test_a_skip_leaves_every_byte_table_and_hint(gpu_ctx, scene_cache):
    name = "cornell"
    s, (w, h) = _setup(name), SIZES[name]
    old = verts_of(s.desc)
    r = changed_ranges(old, far(s.desc, old))
    b = policy_scene(gpu_ctx, s.desc)
    b.update_vertices_async(on_device(r))                                # a refitted tree: a rebuild would have something to do
    rays = api.camera_rays(gpu_ctx, s.camera, w, h, 1)
    hits = api.trace_rays(b, rays).hits
    leaves = _np(api.hit_leaves(b, hits))                                # the leaf table exists from here on
    assert (leaves != 0).any()
    ni = s.desc.numInstances
    masks = np.array([(0x01, 0x02, 0x04, 0xff, 0x03)[k % 5] for k in range(ni)], np.uint8)
    b.set_instance_masks(masks)

    def masked():
        return [(api.trace_rays(b, rays, cull_mask=cm).hits.view(torch.int32).tolist(), _np(api.trace_occlusion(b, rays, cull_mask=cm).occluded).tobytes()) for cm in (0x01, 0x06, 0xff)]

    before, answers, sah = full(b), masked(), b.tree_cost().sah
    enq = b.update_status().enqueued
    b.rebuild_if_async(INF)
    assert (_np(api.hit_leaves(b, hits)) == leaves).all(), "hit_leaves right after the skip, from the table that was there"
    us = b.update_status()
    assert (us.enqueued, us.refused, us.first_refused_update, us.first_bad_vertex) == (enq + 1, 0, None, None)
    st = b.rebuild_if_status()
    assert (st.evaluated, st.rebuilt, st.last_decision) == (1, 0, False) and bits(st.last_sah) == bits(sah)
    assert full(b) == before, "a skipped rebuild changed a byte"
    assert masked() == answers
    assert (b.instance_masks() == masks).all()
    assert (_np(api.hit_leaves(b, hits)) == leaves).all()
    lp = api.make_light_params(s.num_lights, 3, 1, w, 1)
    lr, lv = api.light_rays(b, rays, hits, lp, hints=True)
    assert bool((lv < 0).any())
    assert_same_bytes(api.trace_occlusion(b, lr, start_leaves=lv).occluded, api.trace_rays(b, lr, any_hit=True).occluded, "hinted occlusion after the skip")
    # the control: the same call with 0.0 does rebuild this tree
    b.rebuild_if_async(0.0)
    assert b.rebuild_if_status().rebuilt == 1 and snapshot(b)[0] != before[0]
    b.close()


# ---- 4. the depth rule still refuses ------------------------------------------------------------------------------------------------
def test_the_depth_rule_still_refuses(gpu_ctx, scene_cache, tmp_path):
    case = _points_case(tmp_path, "lattice", L)
    to_p, to_l = [(0, _positions(case.desc, P))], [(0, _positions(case.desc, L))]
    a, b = device_scene(gpu_ctx, case.desc), policy_scene(gpu_ctx, case.desc)
    assert a.stats().maxDepth <= 16 and a.stats().stackEntries == 16, f"premise: the lattice's depth is {a.stats().maxDepth}"
    st0 = b.rebuild_if_status()
    assert bits(st0.built_sah) == bits(a.tree_cost().sah) and st0.built_sah > 0.0
    a.update_vertices(to_p)
    refit_only, x = full(a), a.tree_cost().sah
    assert x > 0.0, "premise: the refitted tree has a positive cost, so 0.0 decides to build"
    b.update_vertices_async(on_device(to_p))
    b.rebuild_if_async(0.0)
    st = b.rebuild_if_status()
    assert (st.evaluated, st.rebuilt, st.last_decision) == (1, 0, True), "decided to build, and the commit was refused"
    assert bits(st.last_sah) == bits(x) and bits(st.built_sah) == bits(st0.built_sah), "a refused commit leaves the baseline"
    ra._assert_same_queries_and_image(gpu_ctx, case, b, a, _rays_at(P), "after the refused rebuild")
    assert full(b) == refit_only, "a refused rebuild leaves the refitted tree, byte for byte"
    rebuilt = device_scene(gpu_ctx, case.desc)
    rebuilt.update_vertices(to_p)
    rebuilt.rebuild("device")
    deep = rebuilt.stats().maxDepth
    assert 17 <= deep <= 32 and rebuilt.stats().stackEntries == 32, f"premise: the powers of two build a tree of depth {deep}"
    rebuilt.close()
    assert status(b) == (2, 1, 2, deep)
    # back to the lattice: committed
    a.update_vertices(to_l); a.rebuild("device")
    b.update_vertices_async(on_device(to_l)); b.rebuild_if_async(0.0)
    assert status(b) == (4, 1, None, None)
    st = b.rebuild_if_status()
    assert (st.evaluated, st.rebuilt, st.last_decision) == (2, 1, True) and bits(st.built_sah) == bits(a.tree_cost().sah)
    assert full(b) == full(a)
    assert_stats(b, a)
    a.close(); b.close()


# ---- 5. the baseline follows the other builds ---------------------------------------------------------------------------------------
def test_the_baseline_follows_the_other_builds(gpu_ctx, scene_cache):
    s = _setup("cornell")
    old = verts_of(s.desc)
    new = far(s.desc, old)
    there, back = changed_ranges(old, new), changed_ranges(new, old)
    a, b = device_scene(gpu_ctx, s.desc), policy_scene(gpu_ctx, s.desc)
    first = b.rebuild_if_status().built_sah
    # the unconditional enqueued rebuild
    a.update_vertices(there); a.rebuild("device")
    b.update_vertices_async(on_device(there)); b.rebuild_async()
    st = b.rebuild_if_status()
    assert bits(st.built_sah) == bits(a.tree_cost().sah) and st.built_sah != first, "rebuild_async moves the baseline to the new tree's cost"
    assert (st.evaluated, st.rebuilt, st.last_decision, st.last_sah) == (0, 0, None, 0.0)
    assert full(b) == full(a) and status(b) == (2, 0, None, None)
    # the synchronous policy takes the device's baseline: the policies mix
    assert b.update_vertices_or_rebuild(back, rebuild_above=INF) is False
    assert bits(b._built_sah) == bits(st.built_sah)
    a.update_vertices(back)
    # the synchronous device rebuild, and the scene stays prepared
    a.rebuild("device"); b.rebuild("device")
    st = b.rebuild_if_status()
    assert bits(st.built_sah) == bits(a.tree_cost().sah) and (st.evaluated, st.rebuilt) == (0, 0)
    b.rebuild_if_async(INF)
    st = b.rebuild_if_status()
    assert (st.evaluated, st.rebuilt, st.last_decision) == (1, 0, False) and bits(st.last_sah) == bits(a.tree_cost().sah)
    # a host rebuild drops the readiness
    a.rebuild("host"); b.rebuild("host")
    before, enq = full(b), b.update_status().enqueued
    with pytest.raises(api.RtrError, match=PREPARE) as e:
        b.rebuild_if_async(0.0)
    assert vu.INVALID_NAME in str(e.value) and WHO in str(e.value)
    assert full(b) == before == full(a) and b.update_status().enqueued == enq
    # and a device rebuild brings it back, the counts going on
    a.rebuild("device"); b.rebuild("device")
    assert bits(b.rebuild_if_status().built_sah) == bits(a.tree_cost().sah)
    a.update_vertices(there); a.rebuild("device")
    b.update_vertices_async(on_device(there)); b.rebuild_if_async(0.0)
    st = b.rebuild_if_status()
    assert (st.evaluated, st.rebuilt, st.last_decision) == (2, 1, True) and bits(st.built_sah) == bits(a.tree_cost().sah)
    assert full(b) == full(a)
    # a scene prepared for rebuild_async only: its chain and status as they were, and no policy
    c = prepared(gpu_ctx, s.desc)
    c.update_vertices_async(on_device(there)); c.rebuild_async()
    assert full(c) == full(a) and status(c) == (2, 0, None, None)
    st = c.rebuild_if_status()
    assert (st.evaluated, st.rebuilt, st.built_sah, st.last_sah, st.last_decision) == (0, 0, 0.0, 0.0, None)
    with pytest.raises(api.RtrError, match=PREPARE):
        c.rebuild_if_async(0.0)
    assert status(c) == (2, 0, None, None)
    a.close(); b.close(); c.close()


# ---- 6. stream order, no join -------------------------------------------------------------------------------------------------------
def test_the_policy_is_stream_ordered_and_does_not_join(scene_cache):
    ctx = api.Context(0)
    stream = torch.cuda.Stream()
    ctx.set_stream(stream.cuda_stream)
    s = _setup("bunny")
    old = verts_of(s.desc)
    new = far(s.desc, old)
    a0, a = device_scene(ctx, s.desc), device_scene(ctx, s.desc)
    a.update_vertices(changed_ranges(old, new))
    a.rebuild("device")
    p = api.make_params(64, 48, spp=1)
    ref0, ref1 = _render(ctx, a0, s, p, frame_no=1), _render(ctx, a, s, p, frame_no=1)
    img0, img1 = ref0.download(), ref1.download()
    assert (img0 != img1).any(), "premise: the deformation shows in the image"
    b = policy_scene(ctx, s.desc)
    f0, f1 = _render(ctx, b, s, p, frame_no=1), api.Frame(ctx, 64, 48, A.IMAGES_FRAMEBUFFER)      # a first render: its scratch exists from here on
    assert np.array_equal(f0.download(), img0)
    with torch.cuda.stream(stream):
        x = torch.rand(4096, 4096, device="cuda")
        dev_new = torch.from_numpy(new).cuda()
    stream.synchronize()
    _filler_ms(stream, x, 1)
    rounds, ms = 2, 0.0
    while True:
        ms = _filler_ms(stream, x, rounds)
        if ms >= 100.0:
            break
        rounds = max(rounds + 1, int(rounds * 130.0 / max(ms, 1e-3)) + 1)
        assert rounds < 100000
    done = torch.cuda.Event()
    with torch.cuda.stream(stream):
        _filler(x, rounds)
        pos = dev_new[:, 0:3] * 1.0                   # the positions are MADE on the stream, behind the filler (x * 1 is exact)
        nrm = dev_new[:, 4:7].clone()
        api.render(b, s.camera, s.scene_info(1), p, f0, asynchronous=True)         # enqueued BEFORE: the old tree
        b.update_vertices_async([(0, pos, nrm)])
        t0 = time.perf_counter()
        b.rebuild_if_async(0.0)
        host_ms = (time.perf_counter() - t0) * 1e3
        done.record(stream)
        pending = not done.query()
        api.render(b, s.camera, s.scene_info(1), p, f1, asynchronous=True)         # enqueued AFTER: the new tree
    print(f"filler {ms:.1f} ms in {rounds} rounds; rebuild_if_async returned after {host_ms:.3f} ms on the host; the stream was {'busy' if pending else 'IDLE'}")
    assert pending, "the call waited for the work queued in front of it"
    st = b.rebuild_if_status()
    assert done.query()
    assert (st.evaluated, st.rebuilt, st.last_decision) == (1, 1, True)
    assert status(b) == (2, 0, None, None)
    assert np.array_equal(f0.download(), img0), "the render enqueued before the call saw the old tree"
    assert np.array_equal(f1.download(), img1), "the render enqueued after the call saw the new tree"
    assert full(b) == full(a), "the chain read the positions the stream produced"
    again = _filler_ms(stream, x, rounds)
    assert again >= 50.0, f"inconclusive: the filler that took {ms:.1f} ms now takes {again:.1f} ms"
    for o in (ref0, ref1, f0, f1, a0, a, b):
        o.close()
    ctx.set_stream(None)
    ctx.close()


# ---- 7. refusals enqueue nothing ----------------------------------------------------------------------------------------------------
def test_refusals_enqueue_nothing(gpu_ctx, scene_cache):
    s = _setup("cornell")

    def refused(scene, call, match, who):
        before, enq = full(scene), scene.update_status().enqueued
        with pytest.raises(api.RtrError, match=match) as e:
            call()
        assert vu.INVALID_NAME in str(e.value) and e.value.status == -1 and who in str(e.value), str(e.value)
        assert scene.update_status().enqueued == enq and full(scene) == before

    def raw(scene, flags, above):
        return lambda: api._check(scene.lib.rtr_scene_rebuild_if_async(scene.h, flags, above), WHO)

    scene = device_scene(gpu_ctx, s.desc)
    refused(scene, lambda: scene.rebuild_if_async(1.0), PREPARE, WHO)                                    # unprepared
    scene.prepare_async_rebuild()
    refused(scene, lambda: scene.rebuild_if_async(1.0), PREPARE, WHO)                                    # prepared for rebuild_async only
    st = scene.rebuild_if_status()
    assert (st.evaluated, st.rebuilt, st.built_sah, st.last_sah, st.last_decision) == (0, 0, 0.0, 0.0, None)
    scene.prepare_async_rebuild_if()
    for bad in (0, 2, 3):
        refused(scene, raw(scene, bad, 1.0), "buildFlags", WHO)
    for bad in (float("nan"), -1.0, -INF, -1e-300):
        refused(scene, raw(scene, A.BUILD_DEVICE_LBVH, bad), "rebuildAbove", WHO)
    with pytest.raises(ValueError):
        scene.rebuild_if_async(1.0, build="host")
    assert scene.rebuild_if_status().evaluated == 0
    scene.rebuild_if_async(INF)
    assert status(scene) == (1, 0, None, None) and scene.rebuild_if_status().evaluated == 1
    scene.close()

    host = api.Scene(gpu_ctx, _with_flags(s.desc, A.BUILD_HOST_SAH))
    refused(host, host.prepare_async_rebuild_if, r"rtr_scene_rebuild\(scene, RTR_BUILD_DEVICE_LBVH\)", "rtr_scene_prepare_async_rebuild")
    refused(host, lambda: host.rebuild_if_async(0.0), PREPARE, WHO)
    host.close()

    room = device_scene(gpu_ctx, _setup("room").desc)                    # 14 triangles: the prepare refusal of the enqueued rebuild
    assert room.stats().numTriangles < 16
    refused(room, room.prepare_async_rebuild_if, "16 triangles", "rtr_scene_prepare_async_rebuild")
    refused(room, lambda: room.rebuild_if_async(0.0), PREPARE, WHO)
    room.close()

    e = empty_desc()
    e.buildFlags = A.BUILD_DEVICE_LBVH
    scene = api.Scene(gpu_ctx, e)
    before = snapshot(scene)
    scene.prepare_async_rebuild_if()
    scene.rebuild_if_async(0.0)
    st = scene.rebuild_if_status()
    assert (st.evaluated, st.rebuilt, st.built_sah, st.last_sah, st.last_decision) == (0, 0, 0.0, 0.0, None)
    assert status(scene) == (1, 0, None, None) and snapshot(scene) == before
    scene.close()
