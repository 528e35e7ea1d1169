"""The resident order of the 4-wide records (kernels/rtr_hot_top.h): the device holds a best-first top towards the area lights — what
k_shadow_trace4 keeps in LDS — and then every other record in breadth-first order; the export stays breadth-first.  Checked here:
the order's invariants and an independent numpy restatement of the growth on a CPU-only box, the host restatement against the device's
bytes, and that nothing a ray does depends on where a record is stored: framebuffer bytes and work counters against the oracle, in the
timed and the counting form, over the plain and the binned queue, with and without the own-leaf start, and after every kind of update."""
import ctypes as C

import numpy as np
import pytest

from realtimeraytracer_amd import _abi as A
from realtimeraytracer_amd import api, scenes

F32 = np.float32
EMPTY = -2 ** 31
COUNTERS = ("numRays", "numShadowRays", "numNodeVisits", "numTriTests", "numShadowNodeVisits", "numShadowTriTests", "shadowTailRays", "numHits")


# ---- helpers --------------------------------------------------------------------------------------------------------------------------
def words(wide):
    return np.frombuffer(bytes(wide), dtype=np.uint32).reshape(-1, 16)


def lights_of(desc):
    return [A.RtrAreaLightInfo.from_buffer_copy(bytes(desc.lights[i])) for i in range(desc.numLights)]


def plane32(h):
    v = np.array([h], np.uint16).view(np.float16).astype(F32)[0]
    return F32(np.sign(v) * 65536.0) if np.isinf(v) else v


def score32(w, grid, centres):
    """rtr_hot_score, operation for operation, in numpy float32"""
    c = [F32(grid.wideCentreXY & 0xffff), F32(grid.wideCentreXY >> 16), F32(grid.wideCentreZ & 0xffff)]
    hlo = [int(w[0]) & 0xffff, int(w[0]) >> 16, int(w[2]) & 0xffff]
    hhi = [int(w[1]) & 0xffff, int(w[1]) >> 16, int(w[2]) >> 16]
    lo = [F32(F32((plane32(hlo[k]) + c[k]) * F32(grid.scale[k])) + F32(grid.origin[k])) for k in range(3)]
    hi = [F32(F32((plane32(hhi[k]) + c[k]) * F32(grid.scale[k])) + F32(grid.origin[k])) for k in range(3)]
    d = [max(F32(hi[k] - lo[k]), F32(0)) for k in range(3)]
    area = F32(F32(2) * F32(F32(F32(d[0] * d[1]) + F32(d[1] * d[2])) + F32(d[2] * d[0])))
    score = F32(0)
    for p in centres:
        d2 = F32(0)
        for k in range(3):
            out = max(max(F32(lo[k] - F32(p[k])), F32(F32(p[k]) - hi[k])), F32(0))
            d2 = F32(d2 + F32(out * out))
        sphere = F32(F32(12.566370614359172) * d2)
        score = F32(score + (F32(area / sphere) if sphere > area else F32(1)))
    return score


def expected_top(bfs, grid, lights, top):
    """the set grown from the root as the issue states it: the highest priority among the inner children of the set, ties to the lower
    breadth-first index -> the breadth-first ids in the order they are taken"""
    w = words(bfs)
    child = w[:, 12:16].view(np.int32)
    centres = [[l.transform[12], l.transform[13], l.transform[14]] for l in lights]
    sel, cand = [0], {}

    def add(i):
        for k in range(4):
            if child[i, k] >= 0:
                cand[int(child[i, k])] = score32(w[i, 3 * k:3 * k + 3], grid, centres)
    add(0)
    while len(sel) < top and cand:
        best = min(cand, key=lambda i: (-float(cand[i]), i))
        del cand[best]
        sel.append(best)
        add(best)
    return sel


def positions(bfs, res):
    """where each record of the breadth-first view sits in the resident one: the two are walked together from the root, level by level,
    and every pair of records met must hold the same boxes, the same leaf codes and inner children in the same slots"""
    a, b = words(bfs), words(res)
    assert a.shape == b.shape
    ca, cb = a[:, 12:16].view(np.int32), b[:, 12:16].view(np.int32)
    pos = np.full(len(a), -1, np.int64)
    pos[0] = 0
    level = np.array([0])
    while level.size:
        here = pos[level]
        assert np.array_equal(a[level, :12], b[here, :12]), "the boxes of a record changed with the order"
        inner = ca[level] >= 0
        assert np.array_equal(inner, cb[here] >= 0) and np.array_equal(ca[level][~inner], cb[here][~inner]), "a leaf code or an empty slot changed"
        assert (pos[ca[level][inner]] < 0).all(), "a record has two parents"
        pos[ca[level][inner]] = cb[here][inner]
        level = ca[level][inner]
    assert np.array_equal(np.sort(pos), np.arange(len(a))), "the resident records are a permutation of the breadth-first ones"
    return pos


def check_order(bfs, res, top, grid=None, lights=None):
    """the invariants of the resident order; with grid and lights, also that its top IS the best-first set"""
    pos = positions(bfs, res)
    cb = words(res)[:, 12:16].view(np.int32)
    n = len(pos)
    own = np.broadcast_to(np.arange(n)[:, None], (n, 4))
    inner = cb >= 0
    assert (cb[inner] > own[inner]).all(), "every inner child index is greater than its parent's"
    parent = np.full(n, -1, np.int64)
    parent[cb[inner]] = own[inner]
    t = min(top, n)
    assert pos[0] == 0 and parent[0] == -1 and ((parent[1:t] >= 0) & (parent[1:t] < t)).all(), "the first records form a connected top rooted at record 0"
    inv = np.argsort(pos)
    assert np.all(np.diff(inv[t:]) > 0), "everything after the top keeps its breadth-first order"
    if grid is not None:
        want = expected_top(bfs, grid, lights, top) if lights else list(range(t))
        assert inv[:t].tolist() == want, "the top is the set grown best-first from the root, in the order it grew"
    return pos


def cpu_setup(name):
    return scenes.cornell_box(64, 64) if name == "cornell_box" else scenes.sponza_class(128, 72)


# ---- CPU: the order's invariants ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["cornell_box", "sponza_class"])
def test_resident_order_invariants(name, scene_cache, monkeypatch):
    s = cpu_setup(name)
    lights = lights_of(s.desc)
    assert lights
    for greedy in ("0", "1"):
        monkeypatch.setenv("RTR_BVH_WIDE_GREEDY", greedy)
        bvh = api.host_build_bvh_wide(s.desc)
        n = len(bvh.wide)
        for top in sorted({api.trace_top_nodes(), 2, 7} | ({n, n + 5} if n + 5 <= 256 else set())):
            res = api.host_wide_resident(bvh.wide, bvh[2], lights, top)
            pos = check_order(bvh.wide, res, top, bvh[2], lights)
            if name == "sponza_class" and top == api.trace_top_nodes():
                assert (pos[:top] != np.arange(top)).any(), "on the atrium the best-first top is not the first breadth-first records"
        # a top of one record, and no lights at all: the breadth-first bytes
        assert bytes(api.host_wide_resident(bvh.wide, bvh[2], lights, 1)) == bytes(bvh.wide)
        assert bytes(api.host_wide_resident(bvh.wide, bvh[2], [], api.trace_top_nodes())) == bytes(bvh.wide)
    assert 0 < api.trace_top_nodes() <= 256


def test_a_tree_of_one_record_and_bad_arguments(scene_cache):
    from test_rebuild_abi import one_triangle_desc
    d = one_triangle_desc()
    bvh = api.host_build_bvh_wide(d)
    assert len(bvh.wide) == 1
    light = lights_of(scenes.cornell_box(16, 16).desc)
    assert bytes(api.host_wide_resident(bvh.wide, bvh[2], light)) == bytes(bvh.wide)
    lib = A.hip_lib()
    out = (A.RtrWideNode * 1)()
    assert lib.rtr_host_wide_resident(bvh.wide, 63, C.byref(bvh[2]), None, 0, 40, out) == -1
    assert lib.rtr_host_wide_resident(bvh.wide, 64, C.byref(bvh[2]), None, 1, 40, out) == -1
    assert lib.rtr_host_wide_resident(None, 64, C.byref(bvh[2]), None, 0, 40, out) == -1


# ---- GPU ----------------------------------------------------------------------------------------------------------------------------------
def _flags(desc, flags):
    d = A.rtr_scene_desc.from_buffer_copy(bytes(desc))
    d.buildFlags = flags
    return d


def check_scene(scene, lights):
    """the device's resident bytes are the host restatement's of its own export, and satisfy the invariants"""
    ex = scene.export_bvh()
    res = scene.export_wide_resident()
    assert bytes(res) == bytes(api.host_wide_resident(ex.wide, ex[2], lights)), "device-made and host-made resident orders differ"
    check_order(ex.wide, res, api.trace_top_nodes(), ex[2], lights)
    return ex


@pytest.mark.gpu
@pytest.mark.parametrize("flags", [A.BUILD_HOST_SAH, A.BUILD_DEVICE_LBVH], ids=["sah", "lbvh"])
@pytest.mark.parametrize("name", ["cornell_box", "sponza_class"])
def test_device_and_host_make_the_same_order(gpu_ctx, scene_cache, name, flags):
    s = cpu_setup(name)
    scene = api.Scene(gpu_ctx, _flags(s.desc, flags))
    ex = check_scene(scene, lights_of(s.desc))
    if flags == A.BUILD_HOST_SAH:      # the whole host route, from the description
        host = api.host_build_bvh_wide(s.desc)
        assert bytes(ex.wide) == bytes(host.wide)
        assert bytes(scene.export_wide_resident()) == bytes(api.host_wide_resident(host.wide, host[2], lights_of(s.desc)))
    if name == "cornell_box":
        assert len(ex.wide) < api.trace_top_nodes(), "the edge this case is for: fewer records than the kernel keeps in LDS"
    scene.close()


@pytest.mark.gpu
def test_one_record_and_no_lights_on_the_device(gpu_ctx, scene_cache):
    from test_rebuild_abi import one_triangle_desc
    scene = api.Scene(gpu_ctx, one_triangle_desc())
    ex = scene.export_bvh()
    assert len(ex.wide) == 1 and bytes(scene.export_wide_resident()) == bytes(ex.wide)
    scene.close()


_ref = {}


def _oracle(oracle, name, s, p, own_leaf):
    key = (name, own_leaf)
    if key not in _ref:
        _ref[key] = oracle.render(s.desc, s.camera, s.scene_info(0), p, bvh=api.host_build_bvh_wide(s.desc), threads=8, own_leaf=own_leaf)
    return _ref[key]


def _render(ctx, scene, s, p):
    frame = api.Frame(ctx, p.width, api.shard_rows(p.height, p.bandRows or 8, p.shardCount or 1), A.IMAGES_FRAMEBUFFER)
    api.render(scene, s.camera, s.scene_info(0), p, frame)
    return frame


def assert_oracle_equal(ctx, oracle, scene, desc, s, w, h, own_leaf=True, ref=None, what=""):
    """the timed and the counting form against the oracle's walk of the exported tree: framebuffer bytes and work counters"""
    pc = api.make_params(w, h, spp=1, shadow_rays=3, collect_stats=1)
    pt = api.make_params(w, h, spp=1, shadow_rays=3)
    if ref is None:
        ref = oracle.render(desc, s.camera, s.scene_info(0), pc, bvh=scene.export_bvh(), threads=8, own_leaf=own_leaf)
    counted = _render(ctx, scene, s, pc)
    assert np.array_equal(counted.download(), ref.images[A.IMAGE_SHADOWED]), f"{what}: counting form, framebuffer"
    g = counted.stats()
    got, want = {f: int(getattr(g, f)) for f in COUNTERS}, {f: int(getattr(ref.stats, f)) for f in COUNTERS}
    print(what, got)
    assert got == want, f"{what}: work counters"
    assert np.array_equal(_render(ctx, scene, s, pt).download(), ref.images[A.IMAGE_SHADOWED]), f"{what}: timed form, framebuffer"


@pytest.mark.gpu
@pytest.mark.parametrize("own_leaf", [1, 0])
@pytest.mark.parametrize("name,w,h", [("cornell_box", 64, 64), ("sponza_class", 128, 72)])
def test_parity_with_the_oracle(gpu_ctx, oracle, scene_cache, queue_mode, name, w, h, own_leaf):
    s = scenes.cornell_box(w, h) if name == "cornell_box" else scenes.sponza_class(w, h)
    pc = api.make_params(w, h, spp=1, shadow_rays=3, collect_stats=1)
    ref = _oracle(oracle, name, s, pc, bool(own_leaf))
    scene = api.Scene(gpu_ctx, s.desc)
    if name == "sponza_class":
        assert bytes(scene.export_wide_resident()) != bytes(scene.export_bvh().wide), "the order under test is not the breadth-first one"
    gpu_ctx.set_tunable("trace_own_leaf", own_leaf)
    try:
        assert_oracle_equal(gpu_ctx, oracle, scene, s.desc, s, w, h, bool(own_leaf), ref, f"{name} {queue_mode} own_leaf={own_leaf}")
    finally:
        gpu_ctx.set_tunable("trace_own_leaf", 1)
    scene.close()


@pytest.mark.gpu
@pytest.mark.parametrize("flags", [A.BUILD_HOST_SAH, A.BUILD_DEVICE_LBVH], ids=["sah", "lbvh"])
def test_updates_keep_the_scene_oracle_equal(gpu_ctx, oracle, scene_cache, flags):
    """update_vertices, update_instances_async moving a light, rebuild and rebuild_async: after each the scene is oracle-equal, the
    resident order is the host restatement's for the boxes and lights the scene has then, and it satisfies the invariants"""
    import test_gpu_vertex_update as vu
    from test_gpu_bvh import _moved
    from test_gpu_instance_async import lights_of as lights_tensor, transforms_of
    w, h = 96, 64
    s = scenes.bunny_class(w, h, subdiv=3)
    scene = api.Scene(gpu_ctx, _flags(s.desc, flags))
    lights = lights_of(s.desc)
    check_scene(scene, lights)
    # a deformation, refitted
    old = vu.verts_of(s.desc)
    new = vu.smooth(s.desc, old)
    scene.update_vertices(vu.changed_ranges(old, new))
    desc = vu.with_vertices(s.desc, new, flags)
    check_scene(scene, lights)
    assert_oracle_equal(gpu_ctx, oracle, scene, desc, s, w, h, what="after update_vertices")
    # the light moves, enqueued: the order follows it
    inst, moved = _moved(s, 0, (35.0, -20.0, 15.0))
    scene.prepare_async_updates()
    scene.update_instances_async(transforms_of(inst), lights=lights_tensor(moved))
    assert scene.update_status().refused == 0
    desc = vu.with_vertices(s.desc, new, flags, instances=inst, lights=moved)
    check_scene(scene, moved)
    assert_oracle_equal(gpu_ctx, oracle, scene, desc, s, w, h, what="after update_instances_async")
    # rebuilt, synchronously and enqueued
    scene.rebuild("device")
    check_scene(scene, moved)
    assert_oracle_equal(gpu_ctx, oracle, scene, desc, s, w, h, what="after rebuild")
    scene.prepare_async_rebuild()
    scene.rebuild_async()
    assert scene.update_status().refused == 0
    check_scene(scene, moved)
    assert_oracle_equal(gpu_ctx, oracle, scene, desc, s, w, h, what="after rebuild_async")
    scene.close()
    vu._setups.clear()
