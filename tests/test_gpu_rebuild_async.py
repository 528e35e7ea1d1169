"""rtr_scene_rebuild_async on the device: the device rebuild as stream-ordered work.  The reference is always the SYNCHRONOUS TWIN: a
second scene built from the same description takes update_vertices / update_instances / rebuild("device"), the scene under test the
enqueued calls, and the two must hold the same bytes — tree, records, grid, 4-wide view, vertices, stats, tree cost — and answer
queries and renders bit for bit alike.  The two differ in where the tree is built (a stage that k_commit_tree copies over the live
arrays, against fresh arrays that are swapped in), in who decides (the device, on the staged depth against the scene's stack class),
and in the host mirrors, which the enqueued call leaves stale.
Of the three scenes of test_gpu_vertex_update.py, `room` has 14 triangles: it takes the host builder whatever the flag and so, by
the n >= 16 rule of rtr_scene_prepare_async_rebuild, has no enqueued rebuild; its cases hold that refusal and the synchronous route
(assert_too_small_for_the_device_builder)."""
import os
import re
import time

import numpy as np
import pytest
import torch

import conditioned_scenes as cs
import test_gpu_instance_async as ia
import test_gpu_update_async as ua
import test_gpu_vertex_update as vu
from realtimeraytracer_amd import _abi as A
from realtimeraytracer_amd import api
from test_gpu_bvh import _moved, _render, _with_flags
from test_gpu_occlusion import assert_same_bytes
from test_gpu_rebuild import STATS, rays_for, same_answers
from test_gpu_update_async import _filler, _filler_ms, full, on_device
from test_gpu_vertex_update import SIZES, _np, _setup, changed_ranges, collapsed, far, smooth, snapshot, verts_of, with_vertices
from test_rebuild_abi import empty_desc

pytestmark = pytest.mark.gpu

DEVICE = A.BUILD_DEVICE_LBVH
DEFORM = {"smooth": smooth, "far": far, "collapsed": collapsed}
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_twins = {}


@pytest.fixture(scope="module", autouse=True)
def _cleanup():
    yield
    for m in _twins.values():
        m["a"].close()
    _twins.clear(); vu._setups.clear(); ua._grid.clear()


def device_scene(ctx, desc):
    return api.Scene(ctx, _with_flags(desc, DEVICE))


def prepared(ctx, desc):
    b = device_scene(ctx, desc)
    b.prepare_async_rebuild()
    return b


def status(scene):
    st = scene.update_status()
    return (st.enqueued, st.refused, st.first_refused_update, st.first_bad_vertex)


def assert_stats(b, a, skip=()):
    sb, sa = b.stats(), a.stats()
    for f in STATS:
        if f not in skip:
            assert getattr(sb, f) == getattr(sa, f), f"stats.{f}: {getattr(sb, f)} != the twin's {getattr(sa, f)}"


def twin(ctx, name, deform):
    """the synchronous twin of (name, deform): created on the device, update_vertices, rebuild("device"); built once"""
    key = (name, deform)
    if key not in _twins:
        s = _setup(name)
        old = verts_of(s.desc)
        new = DEFORM[deform](s.desc, old)
        a = device_scene(ctx, s.desc)
        cls = a.stats().stackEntries
        ranges = changed_ranges(old, new)
        a.update_vertices(ranges)
        a.rebuild("device")
        _twins[key] = {"s": s, "old": old, "new": new, "ranges": ranges, "a": a, "cls": cls, "desc": with_vertices(s.desc, new, DEVICE)}
    return _twins[key]


def enqueued_twin(ctx, m):
    b = prepared(ctx, m["s"].desc)
    b.update_vertices_async(on_device(m["ranges"]))
    b.rebuild_async()
    return b


def assert_too_small_for_the_device_builder(b, a):
    """`room` has 14 triangles: fewer than 16 take the host builder whatever the flag (rtr_scene_create, rtr_scene_rebuild), so the scene
    has no device tree and, by the rule of rtr_scene_prepare_async_rebuild (a device tree of n >= 16), no enqueued rebuild.  What holds
    for it: the prepare call and the enqueued call are refused before anything is enqueued, no byte changes, and the synchronous
    rebuild of the scene that took the enqueued updates is the twin's."""
    assert b.stats().numTriangles < 16 and b.stats().sahCost > 0.0
    before, enq = full(b), b.update_status().enqueued
    with pytest.raises(api.RtrError, match="16 triangles") as e:
        b.prepare_async_rebuild()
    assert vu.INVALID_NAME in str(e.value) and "rtr_scene_rebuild(scene, RTR_BUILD_DEVICE_LBVH)" in str(e.value)
    with pytest.raises(api.RtrError, match="not prepared"):
        b.rebuild_async()
    assert full(b) == before and b.update_status().enqueued == enq
    b.rebuild("device")
    assert full(b) == full(a)
    assert_stats(b, a)


def same_bytes_case(ctx, desc, new_positions):
    """case 1's comparison on any description: all positions replaced, then the rebuild, both ways"""
    ranges = [(0, np.ascontiguousarray(new_positions, np.float32))]
    a = device_scene(ctx, desc)
    cls = a.stats().stackEntries
    a.update_vertices(ranges)
    a.rebuild("device")
    assert a.stats().stackEntries == cls, "premise: the stack class does not change in this case"
    b = prepared(ctx, desc)
    b.update_vertices_async(on_device(ranges))
    b.rebuild_async()
    assert full(b) == full(a)
    assert_stats(b, a)
    assert status(b) == (2, 0, None, None)
    return a, b


# ---- 1. the same bytes as the synchronous call --------------------------------------------------------------------------------------
@pytest.mark.parametrize("deform", ["smooth", "far", "collapsed"])
@pytest.mark.parametrize("name", ["cornell", "bunny", "room"])
def test_same_bytes_as_the_synchronous_call(gpu_ctx, scene_cache, name, deform):
    m = twin(gpu_ctx, name, deform)
    a = m["a"]
    assert a.stats().stackEntries == m["cls"], "premise: the stack class does not change in this case"
    if a.stats().numTriangles < 16:
        b = device_scene(gpu_ctx, m["s"].desc)
        b.prepare_async_updates()
        b.update_vertices_async(on_device(m["ranges"]))
        assert_too_small_for_the_device_builder(b, a)
        b.close()
        return
    b = enqueued_twin(gpu_ctx, m)
    assert full(b) == full(a)
    assert_stats(b, a)
    assert status(b) == (2, 0, None, None)
    refit_only = device_scene(gpu_ctx, m["s"].desc)
    refit_only.update_vertices(m["ranges"])
    if deform == "far":
        assert snapshot(refit_only)[0] != snapshot(b)[0], "the rebuilt tree is not the refitted one: the rebuild had something to do"
    refit_only.close(); b.close()


# ---- 2. answers ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,deform", [("cornell", "collapsed"), ("bunny", "far")])
def test_answers_equal_the_synchronous_twin(gpu_ctx, oracle, scene_cache, name, deform):
    m = twin(gpu_ctx, name, deform)
    w, h = SIZES[name]
    b = prepared(gpu_ctx, m["s"].desc)
    frame = api.Frame(gpu_ctx, w, h, A.IMAGES_FRAMEBUFFER)          # made BEFORE the rebuild
    b.update_vertices_async(on_device(m["ranges"]))
    b.rebuild_async()
    cam, shuffled = rays_for(gpu_ctx, m, name)
    # nothing before this line exported or asked for stats: the queries and the render run on stale mirrors
    img = _render(gpu_ctx, b, m["s"], api.make_params(w, h, spp=1), frame_no=2)
    ref = _render(gpu_ctx, m["a"], m["s"], api.make_params(w, h, spp=1), frame_no=2)
    assert np.array_equal(img.download(), ref.download())
    img.close(); ref.close()
    same_answers(gpu_ctx, oracle, b, m["a"], b.export_bvh(), m["s"], name, cam, shuffled, f"{name} {deform}", frames=(frame,))
    frame.close(); b.close()


# ---- 3. stream order, no join -------------------------------------------------------------------------------------------------------
def test_the_rebuild_is_stream_ordered_and_does_not_join(scene_cache):
    """also the check that the hipcub sort, with its temp storage supplied, neither joins nor allocates"""
    ctx = api.Context(0)
    stream = torch.cuda.Stream()
    ctx.set_stream(stream.cuda_stream)
    s = _setup("bunny")
    old = verts_of(s.desc)
    new = far(s.desc, old)
    a = device_scene(ctx, s.desc)
    a.update_vertices(changed_ranges(old, new))
    a.rebuild("device")
    b = prepared(ctx, s.desc)
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
        t0 = time.perf_counter()
        b.update_vertices_async([(0, pos, nrm)])
        t1 = time.perf_counter()
        b.rebuild_async()
        t2 = time.perf_counter()
        done.record(stream)
    pending = not done.query()
    print(f"filler {ms:.1f} ms in {rounds} rounds; update_vertices_async returned after {(t1 - t0) * 1e3:.3f} ms, rebuild_async after {(t2 - t1) * 1e3:.3f} ms "
          f"on the host; the stream was {'busy' if pending else 'IDLE'}")
    assert pending, "a call waited for the work queued in front of it"
    assert status(b) == (2, 0, None, None)
    assert done.query()
    assert full(b) == full(a), "the build read the positions the stream produced"
    again = _filler_ms(stream, x, rounds)
    assert again >= 50.0, f"inconclusive: the filler that took {ms:.1f} ms now takes {again:.1f} ms"
    a.close(); b.close()
    ctx.set_stream(None)
    ctx.close()


# ---- 4. a run of frames -------------------------------------------------------------------------------------------------------------
def test_a_run_of_frames(gpu_ctx, scene_cache):
    s = _setup("bunny")
    old = verts_of(s.desc)
    first, count, _, _ = [me for me in vu.meshes_of(s.desc) if not me[3]][-1]
    p = old[first:first + count, 0:3].astype(np.float64)
    d = vu._diag(old)
    which = s.desc.numInstances - 1

    def phase(k):
        out = p.copy()
        out[:, 1] += 0.08 * d * np.sin(p[:, 0] * (12.0 / d) + k * np.pi / 4)
        return out.astype(np.float32)

    a, b = device_scene(gpu_ctx, s.desc), prepared(gpu_ctx, s.desc)
    for k in range(8):
        if k % 2 == 0:
            a.update_vertices([(first, phase(k))])
            b.update_vertices_async([(first, torch.from_numpy(phase(k)).cuda())])
        else:
            inst, lights = _moved(s, which, (0.05 * d * k, 0.0, -0.02 * d * k), 1.0 + 0.02 * k)
            a.update_instances(inst, lights)
            b.update_instances_async(ia.transforms_of(inst), lights=ia.lights_of(lights) if lights else None)
            a.rebuild("device")
            b.rebuild_async()
    st = b.update_status()
    assert (st.enqueued, st.refused) == (12, 0)
    assert full(b) == full(a)
    assert bytes(b.export_instances()) == bytes(a.export_instances())
    assert_stats(b, a, skip=("stackEntries",))
    a.close(); b.close()


# ---- 5. the device refuses a class that would rise, and only that -------------------------------------------------------------------
CORNERS = np.array([[-0.125, -0.125, -0.125], [0.125, -0.125, 0.125], [0.0, 0.125, 0.0]])          # the box centre is the point, exactly
P = np.array([(0, 0, 0)] + [t for i in range(10) for t in ((2 ** i, 0, 0), (0, 2 ** i, 0), (0, 0, 2 ** i))] + [(1024, 0, 0), (0, 1024, 0), (0, 0, 1024)], np.float64)
L = np.array([(x, y, z) for x in range(4) for y in range(3) for z in range(3)], np.float64)[:34]
assert len(P) == 34 and len(L) == 34


def _points_case(tmp_path, name, points):
    v = (points[:, None, :] + CORNERS[None, :, :]).reshape(-1, 3)
    return cs._soup_case(name, tmp_path, [(v, np.arange(3 * len(points)).reshape(-1, 3))], (1500.0, 1100.0, -1900.0), (300.0, 250.0, 300.0), 64, 48)


def _positions(desc, points):
    """the vertex positions that put triangle f of the description on points[f] (whatever order the loader gave the vertices)"""
    (first, count, faces, _), = vu.meshes_of(desc)
    assert len(faces) == len(points) and len(np.unique(faces)) == 3 * len(points) == count and first == 0
    out = np.zeros((count, 3), np.float32)
    for k in range(3):
        out[faces[:, k]] = (points + CORNERS[k]).astype(np.float32)
    return out


def _rays_at(points):
    """a ray down the z axis onto every triangle, a miss beside it, and random rays through the bounds"""
    n = len(points)
    r = np.zeros((2 * n, 8), np.float32)
    r[:n, 0:3] = points + np.array([0.0, -0.04, -5.0]); r[n:, 0:3] = points + np.array([0.2, 0.3, -5.0])
    r[:, 6] = 1.0; r[:, 7] = 1e4
    lo, hi = points.min(0) - 0.125, points.max(0) + 0.125
    return np.concatenate([r, vu.random_rays(lo, hi, 1500, 3, float(np.linalg.norm(hi - lo)))])


def _assert_same_queries_and_image(ctx, case, b, a, rays, what):
    ha, hb = api.trace_rays(a, rays), api.trace_rays(b, rays)
    assert hb.hits.view(np.uint32).tolist() == ha.hits.view(np.uint32).tolist(), f"{what}: closest hits"
    assert (np.asarray(hb.custom_index)[:34] != 0xffffffff).all(), f"{what}: the aimed rays hit"
    assert_same_bytes(api.trace_rays(b, rays, any_hit=True).occluded, api.trace_rays(a, rays, any_hit=True).occluded, f"{what}: any-hit")
    assert_same_bytes(api.trace_occlusion(b, rays).occluded, api.trace_occlusion(a, rays).occluded, f"{what}: queued occlusion")
    p = api.make_params(64, 48, spp=1)
    fa, fb = _render(ctx, a, case, p, frame_no=1), _render(ctx, b, case, p, frame_no=1)
    assert np.array_equal(fb.download(), fa.download()), f"{what}: image"
    fa.close(); fb.close()


def test_a_class_that_would_rise_is_refused(gpu_ctx, scene_cache, tmp_path):
    """34 independent triangles, created on a 4 x 3 x 3 lattice (depth 4 by a numpy restatement of k_morton, the Karras split and the
    <= 4 collapse: class 16), sent to the powers of two on the three axes (depth 27: class 32).  The premises are asserted on the twin."""
    case = _points_case(tmp_path, "lattice", L)
    to_p, to_l = [(0, _positions(case.desc, P))], [(0, _positions(case.desc, L))]
    a, b = device_scene(gpu_ctx, case.desc), prepared(gpu_ctx, case.desc)
    assert a.stats().maxDepth <= 16 and a.stats().stackEntries == 16, f"premise: the lattice's depth is {a.stats().maxDepth}"
    a.update_vertices(to_p)
    refit_only = full(a)
    rays = _rays_at(P)
    b.update_vertices_async(on_device(to_p))
    b.rebuild_async()
    _assert_same_queries_and_image(gpu_ctx, case, b, a, rays, "after the refused rebuild")
    assert full(b) == refit_only, "a refused rebuild leaves the refitted tree, byte for byte"
    assert b.stats().stackEntries == 16
    rebuilt = device_scene(gpu_ctx, case.desc)
    rebuilt.update_vertices(to_p)
    rebuilt.rebuild("device")
    deep = rebuilt.stats().maxDepth
    print(f"depth of the lattice {a.stats().maxDepth}, of the powers of two {deep}")
    assert 17 <= deep <= 32 and rebuilt.stats().stackEntries == 32, f"premise: the powers of two build a tree of depth {deep}"
    assert status(b) == (2, 1, 2, deep)
    rebuilt.close()
    # back to the lattice: committed
    a.update_vertices(to_l); a.rebuild("device")
    b.update_vertices_async(on_device(to_l)); b.rebuild_async()
    assert status(b) == (4, 1, None, None)
    assert full(b) == full(a)
    assert_stats(b, a)
    a.close(); b.close()


def test_a_class_that_would_fall_is_committed_and_kept(gpu_ctx, scene_cache, tmp_path):
    case = _points_case(tmp_path, "powers", P)
    to_l = [(0, _positions(case.desc, L))]
    a, b = device_scene(gpu_ctx, case.desc), prepared(gpu_ctx, case.desc)
    assert 17 <= a.stats().maxDepth <= 32 and b.stats().stackEntries == 32, f"premise: the powers of two build a tree of depth {a.stats().maxDepth}"
    a.update_vertices(to_l); a.rebuild("device")
    b.update_vertices_async(on_device(to_l)); b.rebuild_async()
    assert status(b) == (2, 0, None, None)
    _assert_same_queries_and_image(gpu_ctx, case, b, a, _rays_at(L), "after the committed rebuild")
    assert full(b) == full(a), "tree, 4-wide view and tree cost are the twin's"
    assert_stats(b, a, skip=("stackEntries",))
    assert a.stats().maxDepth <= 16 and b.stats().maxDepth == a.stats().maxDepth
    assert (b.stats().stackEntries, a.stats().stackEntries) == (32, 16), "an enqueued rebuild never lowers the class"
    a.close(); b.close()


# ---- 6. masks and tables ------------------------------------------------------------------------------------------------------------
def test_masks_and_tables(gpu_ctx, scene_cache):
    m = twin(gpu_ctx, "cornell", "smooth")
    s, desc = m["s"], _with_flags(m["s"].desc, DEVICE)
    ni = desc.numInstances
    masks = np.array([(0x01, 0x02, 0x04, 0xff, 0x03)[k % 5] for k in range(ni)], np.uint8)
    _, rays = vu.query_rays(gpu_ctx, {"s": s, "scene": m["a"]}, "cornell")
    a, b = api.Scene(gpu_ctx, desc), api.Scene(gpu_ctx, desc)
    b.prepare_async_rebuild()
    a.set_instance_masks(masks); b.set_instance_masks(masks)
    a.update_vertices(m["ranges"]); a.rebuild("device")
    b.update_vertices_async(on_device(m["ranges"])); b.rebuild_async()
    for cm in (0x01, 0x06, 0xff):
        ha, hb = api.trace_rays(a, rays, cull_mask=cm), api.trace_rays(b, rays, cull_mask=cm)
        assert hb.hits.view(np.uint32).tolist() == ha.hits.view(np.uint32).tolist(), f"masked closest hits, cullMask {cm:#x}"
        assert_same_bytes(api.trace_occlusion(b, rays, cull_mask=cm).occluded, api.trace_occlusion(a, rays, cull_mask=cm).occluded, f"masked occlusion {cm:#x}")
    assert (api.trace_rays(b, rays, cull_mask=0x01).hits.view(np.uint32) != api.trace_rays(b, rays, cull_mask=0x06).hits.view(np.uint32)).any()
    rec = np.frombuffer(bytes(b.export_bvh()[1]), dtype=np.uint32).reshape(-1, 12)
    want = {int(desc.instances[i].customIndex): (~int(masks[i]) & 0xff) for i in range(ni)}
    assert all(((int(r[11]) >> 8) & 0xff) == want[int(r[3])] for r in rec), "the records of the enqueued rebuild carry the masks"
    assert (b.instance_masks() == masks).all()
    assert full(b) == full(a)
    a.close(); b.close()

    # an enqueued instance update, then the rebuild: the build reads the DEVICE tables (the host mirrors are stale).  `room` has 14
    # triangles and no device tree (see assert_too_small_for_the_device_builder); `bunny` carries the check of the device tables
    for name in ("room", "bunny"):
        s = _setup(name)
        desc = _with_flags(s.desc, DEVICE)
        inst, lights = _moved(s, desc.numInstances - 1, (3.0, -2.0, 5.0), 1.3)
        a, b = api.Scene(gpu_ctx, desc), api.Scene(gpu_ctx, desc)
        before = snapshot(a)[0]
        a.update_instances(inst, lights); a.rebuild("device")
        if name == "room":
            b.prepare_async_updates()
            b.update_instances_async(ia.transforms_of(inst), lights=ia.lights_of(lights) if lights else None)
            assert_too_small_for_the_device_builder(b, a)
        else:
            b.prepare_async_rebuild()
            b.update_instances_async(ia.transforms_of(inst), lights=ia.lights_of(lights) if lights else None); b.rebuild_async()
            assert full(b) == full(a) and snapshot(b)[0] != before
            assert status(b) == (2, 0, None, None)
        assert bytes(b.export_instances()) == bytes(a.export_instances())
        a.close(); b.close()


# ---- 7. the leaf table --------------------------------------------------------------------------------------------------------------
def test_the_leaf_table_stays_ready_and_current(gpu_ctx, scene_cache):
    name = "cornell"
    m = twin(gpu_ctx, name, "far")
    s, (w, h), a = m["s"], SIZES[name], m["a"]
    rays = api.camera_rays(gpu_ctx, s.camera, w, h, 1)
    lp = api.make_light_params(s.num_lights, 3, 1, w, 1)
    b, c = prepared(gpu_ctx, s.desc), prepared(gpu_ctx, s.desc)
    b.update_vertices_async(on_device(m["ranges"])); c.update_vertices_async(on_device(m["ranges"]))
    hits = api.trace_rays(b, rays).hits
    old_leaves = _np(api.hit_leaves(b, hits))                       # b's table exists from here on; c never asks before the rebuild
    _, stale = api.light_rays(b, rays, hits, lp, hints=True)
    assert bool((stale < 0).any())
    b.rebuild_async(); c.rebuild_async()
    assert api.trace_rays(b, rays).hits.view(torch.int32).tolist() == hits.view(torch.int32).tolist()
    la = _np(api.hit_leaves(a, hits))
    assert (_np(api.hit_leaves(b, hits)) == la).all() and (la != 0).any(), "hit_leaves after the enqueued rebuild != the twin's"
    assert (la != old_leaves).any(), "the leaf order changed"
    lr, lv = api.light_rays(b, rays, hits, lp, hints=True)
    lra, lva = api.light_rays(a, rays, hits, lp, hints=True)
    assert (_np(lv) == _np(lva)).all() and (_np(lr).view(np.uint32) == _np(lra).view(np.uint32)).all()
    qa, qb = api.trace_occlusion(a, lra, collect_stats=True, start_leaves=lva), api.trace_occlusion(b, lr, collect_stats=True, start_leaves=lv)
    assert_same_bytes(qb.occluded, qa.occluded, "hinted queued occlusion")
    for f in ("numRays", "numNodeVisits", "numTriTests", "numAlphaTests", "tailRays"):
        assert getattr(qb.stats, f) == getattr(qa.stats, f), f"hinted query, {f}: {getattr(qb.stats, f)} != the twin's {getattr(qa.stats, f)}"
    plain = api.trace_occlusion(b, lr, collect_stats=True)
    print(f"hinted: {qb.stats.numNodeVisits} node visits, unhinted: {plain.stats.numNodeVisits}")
    assert_same_bytes(qb.occluded, plain.occluded, "hinted vs unhinted")
    assert_same_bytes(api.trace_occlusion(b, lr, start_leaves=stale).occluded, plain.occluded, "hints made before the rebuild change no byte")
    assert (_np(api.hit_leaves(c, hits)) == la).all(), "a scene that never asked gets a correct table on first use"
    b.close(); c.close()


# ---- 8. mirrors ---------------------------------------------------------------------------------------------------------------------
def test_the_mirrors_are_current(gpu_ctx, scene_cache):
    name = "bunny"
    m = twin(gpu_ctx, name, "far")
    a, s, (w, h) = m["a"], m["s"], SIZES[name]
    b = enqueued_twin(gpu_ctx, m)
    ea, eb = a.export_bvh(), b.export_bvh()
    assert bytes(eb[0]) == bytes(ea[0]) and bytes(eb[1]) == bytes(ea[1]) and bytes(eb[2]) == bytes(ea[2]) and bytes(eb.wide) == bytes(ea.wide)
    assert_stats(b, a)
    assert bytes(b.stats().grid) == bytes(a.stats().grid)
    assert b.tree_cost() == a.tree_cost() == api.host_tree_cost(eb[0], eb[2])
    like = api.Scene(gpu_ctx, m["desc"], like=b)
    assert snapshot(like) == snapshot(a)
    p = api.make_params(w, h, spp=1)
    f0, f1 = _render(gpu_ctx, a, s, p, frame_no=3), _render(gpu_ctx, like, s, p, frame_no=3)
    assert np.array_equal(f0.download(), f1.download())
    f0.close(); f1.close(); like.close(); b.close()
    # stats asked FIRST after the call (no export in between)
    b = enqueued_twin(gpu_ctx, m)
    assert b.stats().maxDepth == a.stats().maxDepth and b.stats().numWideNodes == a.stats().numWideNodes
    b.close()


# ---- 9. with the synchronous calls --------------------------------------------------------------------------------------------------
def test_with_the_synchronous_calls(gpu_ctx, scene_cache):
    m = twin(gpu_ctx, "cornell", "far")
    s, desc = m["s"], _with_flags(m["s"].desc, DEVICE)
    back = changed_ranges(m["new"], m["old"])
    masks = np.array([0x01 if i % 2 else 0x02 for i in range(desc.numInstances)], np.uint8)
    a, b = api.Scene(gpu_ctx, desc), api.Scene(gpu_ctx, desc)
    b.prepare_async_rebuild()
    a.update_vertices(m["ranges"]); a.rebuild("device")
    b.update_vertices_async(on_device(m["ranges"])); b.rebuild_async()
    a.update_vertices(back); b.update_vertices(back)
    assert full(b) == full(a), "update_vertices after rebuild_async"
    a.set_instance_masks(masks); b.set_instance_masks(masks)
    assert full(b) == full(a), "set_instance_masks after rebuild_async"
    b.rebuild_async(); a.rebuild("device")
    a.rebuild("device"); b.rebuild("device")
    assert full(b) == full(a), "rebuild('device') after rebuild_async"
    b.update_vertices_async(on_device(m["ranges"])); b.rebuild_async()      # still prepared, without a call
    a.update_vertices(m["ranges"]); a.rebuild("device")
    assert full(b) == full(a)
    # a host rebuild: the readiness is gone
    a.rebuild("host"); b.rebuild("host")
    before, enq = full(b), b.update_status().enqueued
    with pytest.raises(api.RtrError, match="not prepared") as e:
        b.rebuild_async()
    assert vu.INVALID_NAME in str(e.value) and "rtr_scene_rebuild_async" in str(e.value)
    with pytest.raises(api.RtrError, match=r"rtr_scene_rebuild\(scene, RTR_BUILD_DEVICE_LBVH\)") as e:
        b.prepare_async_rebuild()
    assert vu.INVALID_NAME in str(e.value)
    assert full(b) == before == full(a) and b.update_status().enqueued == enq
    b.update_vertices_async(on_device(back)); a.update_vertices(back)      # the enqueued updates still work on the host tree
    assert full(b) == full(a)
    # a device rebuild prepares again, without a call
    a.rebuild("device"); b.rebuild("device")
    a.update_vertices(m["ranges"]); a.rebuild("device")
    b.update_vertices_async(on_device(m["ranges"])); b.rebuild_async()
    assert full(b) == full(a)
    assert b.update_status().refused == 0
    a.close(); b.close()


# ---- 10. refusals enqueue nothing ---------------------------------------------------------------------------------------------------
def test_refusals_enqueue_nothing(gpu_ctx, scene_cache, tmp_path):
    s = _setup("cornell")

    def refused(scene, call, match, who):
        before, enq = snapshot(scene), scene.update_status().enqueued
        with pytest.raises(api.RtrError, match=match) as e:
            call()
        assert vu.INVALID_NAME in str(e.value) and e.value.status == -1 and who in str(e.value), str(e.value)
        assert scene.update_status().enqueued == enq and snapshot(scene) == before

    scene = device_scene(gpu_ctx, s.desc)
    refused(scene, scene.rebuild_async, "not prepared", "rtr_scene_rebuild_async")                       # unprepared
    scene.prepare_async_updates()
    refused(scene, scene.rebuild_async, "rtr_scene_prepare_async_rebuild", "rtr_scene_rebuild_async")    # prepared for updates only
    scene.prepare_async_rebuild()
    scene.prepare_async_rebuild()                                                                        # idempotent
    for bad in (0, 2):
        refused(scene, lambda: api._check(scene.lib.rtr_scene_rebuild_async(scene.h, bad), "rtr_scene_rebuild_async"), "buildFlags", "rtr_scene_rebuild_async")
    with pytest.raises(ValueError):
        scene.rebuild_async("host")
    scene.rebuild_async()
    assert status(scene) == (1, 0, None, None)
    scene.close()

    host = api.Scene(gpu_ctx, _with_flags(s.desc, A.BUILD_HOST_SAH))
    refused(host, host.prepare_async_rebuild, r"rtr_scene_rebuild\(scene, RTR_BUILD_DEVICE_LBVH\)", "rtr_scene_prepare_async_rebuild")
    refused(host, host.rebuild_async, "not prepared", "rtr_scene_rebuild_async")
    host.close()

    rng = np.random.default_rng(5)
    v, t = cs._tri_soup(rng, 15, np.zeros(3), 20.0, 6.0)
    tiny = cs._soup_case("fifteen", tmp_path, [(v, t)], (10.0, 5.0, -90.0), (0.0, 0.0, 0.0), 64, 48)
    scene = device_scene(gpu_ctx, tiny.desc)
    assert scene.stats().numTriangles == 15 and scene.stats().sahCost > 0.0           # the host builder, whatever the flag
    refused(scene, scene.prepare_async_rebuild, "16 triangles", "rtr_scene_prepare_async_rebuild")
    scene.close()

    e = empty_desc()
    e.buildFlags = DEVICE
    scene = api.Scene(gpu_ctx, e)
    before = snapshot(scene)
    scene.prepare_async_rebuild()
    scene.rebuild_async()
    assert status(scene) == (1, 0, None, None) and snapshot(scene) == before
    scene.close()


# ---- 11. the copy's edges -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [16, 17, 18, 19])
def test_array_tails(gpu_ctx, scene_cache, tmp_path, n):
    """16 is the device build's minimum; 16 .. 19 cover every residue mod 4 of n and n - 1, so every word-wise tail of the commit copy
    (parent and the live counters are 4 (n - 1) bytes, slotOfPrim 4 n)"""
    rng = np.random.default_rng(100 + n)
    v, t = cs._tri_soup(rng, n, np.zeros(3), 20.0, 6.0)
    case = cs._soup_case(f"soup{n}", tmp_path, [(v, t)], (10.0, 5.0, -90.0), (0.0, 0.0, 0.0), 64, 48)
    old = verts_of(case.desc)[:, 0:3]
    new = (old[::-1] * np.float32(1.5) + np.float32(2.0)).astype(np.float32)          # the triangles trade places: another Morton order
    a, b = same_bytes_case(gpu_ctx, case.desc, new)
    assert a.stats().numTriangles == n and a.stats().numNodes == n - 1 and a.stats().sahCost == 0.0
    a.close(); b.close()


def commit_max_blocks():
    text = open(os.path.join(ROOT, "realtimeraytracer_amd", "csrc", "kernels", "rtr_bvh.h")).read()
    return int(re.search(r"constexpr\s+uint32_t\s+kCommitMaxBlocks\s*=\s*(\d+)\s*;", text).group(1))


def test_a_copy_of_more_than_one_trip(gpu_ctx, scene_cache, tmp_path_factory):
    """the displaced grid mesh of 104 882 triangles: the commit kernel's grid-stride loop takes more than one trip on the largest array
    (the fp32 nodes, 64 B per node slot) under its grid cap"""
    c = ua._grid_case(tmp_path_factory.mktemp("grid"), 230)
    n = c.num_triangles
    cap = commit_max_blocks()
    chunks = 64 * (n - 1) // 16
    trips = -(-chunks // (cap * 256))
    print(f"{n} triangles: the largest staged array has {chunks} 16-byte chunks; a grid of {cap} x 256 lanes copies it in {trips} trips")
    assert n > 100000 and trips > 1
    old = verts_of(c.desc)
    new = old[:, 0:3].copy()
    new[:, 1] = (old[:, 1] + 9.0 * np.sin(old[:, 0] * 0.05 + 1.0) * np.sin(old[:, 2] * 0.09)).astype(np.float32)
    new[:, 0] = (old[:, 0] * np.float32(1.0) + 30.0 * np.sin(old[:, 2] * 0.03)).astype(np.float32)
    a, b = same_bytes_case(gpu_ctx, c.desc, new)
    refit_only = device_scene(gpu_ctx, c.desc)
    refit_only.update_vertices([(0, new)])
    assert snapshot(refit_only)[0] != snapshot(b)[0], "the rebuilt tree is not the refitted one"
    refit_only.close(); a.close(); b.close()
