"""rtr_scene_update_instances_async on the device: the instance update as stream-ordered work.  The yardstick is always the synchronous
twin: a scene that took update_instances_async must hold the bytes — tree, 4-wide view, vertices, stats, tree cost, the exported
instances — of a twin built from the same description that took update_instances, and answer queries and renders bit for bit like
it.  The two differ in where the tables are made: the synchronous call makes the transform, normal-matrix, mirrored-bit and
InstanceRef tables in host loops, the enqueued one in k_write_instances on the device; and in the host mirrors of the instances and
lights, which the enqueued call leaves stale for refresh_mirrors to read back.  Most tests below are aimed at the second: a stale mirror
silently snaps the instances back at the next synchronous call that re-uploads tables from it."""
import time

import numpy as np
import pytest
import torch

import test_gpu_vertex_update as vu
from realtimeraytracer_amd import _abi as A
from realtimeraytracer_amd import api, scenes
from test_gpu_bvh import _moved, _render, _with_flags
from test_gpu_occlusion import assert_same_bytes
from test_gpu_update_async import _filler, _filler_ms, full, on_device
from test_gpu_vertex_update import BUILDERS, changed_ranges, smooth
from test_rebuild_abi import empty_desc, one_triangle_desc

pytestmark = pytest.mark.gpu

BUILDER_IDS = vu.BUILDER_IDS
BACK, FRONT = A.QUERY_CULL_BACK_FACING, A.QUERY_CULL_FRONT_FACING


@pytest.fixture(scope="module", autouse=True)
def _cleanup():
    yield
    vu._setups.clear()


# ---- helpers ------------------------------------------------------------------------------------------------------------------------
def copies(s):
    return ([A.RtrInstance.from_buffer_copy(bytes(i)) for i in s.host.instances()],
            [A.RtrAreaLightInfo.from_buffer_copy(bytes(l)) for l in s.host.lightInfos()])


def matrix(inst, which):
    return np.array(inst[which].transform[:], np.float32).reshape(3, 4)


def set_matrix(inst, lights, which, m):
    """instance `which` gets the row-major 3x4 m; a light instance's info gets the same matrix, column-major (as _moved does)"""
    m = np.asarray(m, np.float32).reshape(3, 4)
    for k, v in enumerate(m.reshape(-1)):
        inst[which].transform[k] = float(v)
    if which < len(lights):
        cm = np.zeros((4, 4), np.float32); cm[:3, :] = m; cm[3, 3] = 1
        for k, v in enumerate(cm.T.reshape(-1)):
            lights[which].transform[k] = float(v)


def transforms_of(inst, form="34"):
    """the transforms as a device tensor: (n, 3, 4) packed, or (n, 4, 4) row-major matrices with the row 0 0 0 1"""
    m = np.array([i.transform[:] for i in inst], np.float32).reshape(-1, 3, 4)
    if form == "44":
        m4 = np.zeros((len(m), 4, 4), np.float32); m4[:, :3, :] = m; m4[:, 3, 3] = 1
        m = m4
    return torch.from_numpy(np.ascontiguousarray(m)).cuda()


def lights_of(lights):
    """the light infos as a uint8 device tensor"""
    raw = bytes((A.RtrAreaLightInfo * len(lights))(*lights))
    return torch.frombuffer(bytearray(raw), dtype=torch.uint8).cuda()


def state(scene):
    """everything the two forms must agree on, as bytes: full() of the vertex tests and the exported instances"""
    return full(scene) + (bytes(scene.export_instances()),)


def sync_twin(ctx, desc, inst, lights):
    a = api.Scene(ctx, desc)
    a.update_instances(inst, lights)
    return a


def async_twin(ctx, desc, inst, lights, form="34"):
    b = api.Scene(ctx, desc)
    b.prepare_async_updates()
    b.update_instances_async(transforms_of(inst, form), lights=lights_of(lights) if lights else None)
    return b


def rays_for(ctx, s, scene, name):
    return vu.query_rays(ctx, {"s": s, "scene": scene}, name)[1]


def hits_of(scene, rays, **kw):
    return api.trace_rays(scene, rays, **kw).hits.view(np.uint32).tolist()


def assert_same_answers(a, b, rays, what):
    assert hits_of(b, rays) == hits_of(a, rays), f"{what}: closest hits"
    assert_same_bytes(api.trace_rays(b, rays, any_hit=True).occluded, api.trace_rays(a, rays, any_hit=True).occluded, f"{what}: any-hit")
    assert_same_bytes(api.trace_occlusion(b, rays).occluded, api.trace_occlusion(a, rays).occluded, f"{what}: queued occlusion")


# ---- 1. the same bytes as the synchronous call --------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags", BUILDERS, ids=BUILDER_IDS)
@pytest.mark.parametrize("form", ["n34", "n44", "sub"])
@pytest.mark.parametrize("name", ["cornell", "bunny", "room"])
def test_same_bytes_as_the_synchronous_call(gpu_ctx, scene_cache, name, form, flags):
    """one object instance translated and scaled by 1.1: all instances as an (n,3,4) tensor with the lights as a device tensor, the
    same as (n,4,4) matrices (stride 64), and the moved instance alone as a sub-range without lights"""
    s = vu._setup(name)
    desc = _with_flags(s.desc, flags)
    which = desc.numInstances - 1
    assert which >= desc.numLights
    inst, lights = _moved(s, which, (3.0, -2.0, 5.0), 1.1)
    a = sync_twin(gpu_ctx, desc, inst, lights)
    b = api.Scene(gpu_ctx, desc)
    b.prepare_async_updates()
    if form == "sub":
        b.update_instances_async(transforms_of(inst[which:which + 1]), first_instance=which, lights=None)
    else:
        b.update_instances_async(transforms_of(inst, form[1:]), lights=lights_of(lights))
    assert full(b) == full(a)
    assert bytes(b.export_instances()) == bytes(a.export_instances())
    assert bytes(b.export_instances()) == bytes((A.RtrInstance * len(inst))(*inst))
    st = b.update_status()
    assert (st.enqueued, st.refused, st.first_refused_update, st.first_bad_vertex) == (1, 0, None, None)
    a.close(); b.close()


def test_strided_views_and_a_staged_light_list(gpu_ctx, scene_cache):
    """an RtrInstance-shaped (n,16) array entered at +16 bytes (a row view of stride 64 that is taken as it is), and the lights as a
    sequence of RtrAreaLightInfo (staged once by the binding); the light instance moves, so the staged infos are read"""
    s = vu._setup("cornell")
    desc = _with_flags(s.desc, A.BUILD_DEVICE_LBVH)
    inst, lights = _moved(s, 0, (10.0, -20.0, 5.0))
    a = sync_twin(gpu_ctx, desc, inst, lights)
    b = api.Scene(gpu_ctx, desc)
    b.prepare_async_updates()
    rec = np.frombuffer(bytes((A.RtrInstance * len(inst))(*inst)), np.float32).reshape(-1, 16)
    view = torch.from_numpy(rec.copy()).cuda()[:, 4:16]
    assert view.stride(0) == 16 and not view.is_contiguous()
    b.update_instances_async(view, lights=lights)
    assert b.update_status().refused == 0
    assert state(b) == state(a)
    # lights alone: the colour changes, nothing else
    lights[0].color[0] = 0.25
    a.update_instances(inst, lights)
    b.update_instances_async(None, lights=lights)
    assert b.update_status() == api.UpdateStatus(2, 0, None, None)
    assert state(b) == state(a)
    view = scenes.cornell_box(64, 48)
    p = api.make_params(64, 48, spp=1)
    assert np.array_equal(_render(gpu_ctx, b, view, p, frame_no=1).download(), _render(gpu_ctx, a, view, p, frame_no=1).download())
    a.close(); b.close()


# ---- 2. a mirrored instance ---------------------------------------------------------------------------------------------------------
def _mesh_centre(desc, inst, which):
    me = desc.meshes[inst[which].meshIndex]
    v = vu.verts_of(desc)[me.vertexOffset: me.vertexOffset + me.vertexCount, 0:3].astype(np.float64)
    m = matrix(inst, which).astype(np.float64)
    return (v @ m[:, :3].T + m[:, 3]).mean(0)


@pytest.mark.parametrize("flags", BUILDERS, ids=BUILDER_IDS)
def test_a_mirrored_instance(gpu_ctx, scene_cache, flags):
    """the tall block reflected about its own centre (row 0 negated: determinant -1) and the short block shrunk to a speck with one
    axis negated (determinant -1e-9: negative, and tiny): the mirrored bits decide the face culling, the normal matrices the surfaces"""
    s = vu._setup("cornell")
    desc = _with_flags(s.desc, flags)
    ni = desc.numInstances
    inst, lights = copies(s)
    tall, short = ni - 1, ni - 2
    c = _mesh_centre(desc, inst, tall)
    m = matrix(inst, tall)
    m[0, :] = -m[0, :]
    m[0, 3] += np.float32(2.0 * c[0])
    set_matrix(inst, lights, tall, m)
    c = _mesh_centre(desc, inst, short)
    m = matrix(inst, short).astype(np.float64)
    sc = np.diag([-1e-3, 1e-3, 1e-3])
    m2 = np.zeros((3, 4)); m2[:, :3] = sc @ m[:, :3]; m2[:, 3] = c - sc @ (c - m[:, 3])
    set_matrix(inst, lights, short, m2)
    speck = _mesh_centre(desc, inst, short)
    for k in (tall, short):
        assert np.linalg.det(matrix(inst, k)[:, :3].astype(np.float64)) < 0
    assert abs(np.linalg.det(matrix(inst, short)[:, :3].astype(np.float64))) < 2e-9

    a = sync_twin(gpu_ctx, desc, inst, lights)
    b = async_twin(gpu_ctx, desc, inst, lights)
    rng = np.random.default_rng(3)
    d = rng.normal(size=(400, 3)); d /= np.linalg.norm(d, axis=1, keepdims=True)
    aimed = np.zeros((400, 8), np.float32)      # rays at the speck from 50 units away
    aimed[:, 0:3] = speck + 50.0 * d; aimed[:, 4:7] = -d; aimed[:, 3] = 1e-3; aimed[:, 7] = 1e4
    rays = np.ascontiguousarray(np.concatenate([rays_for(gpu_ctx, s, a, "cornell"), aimed]))
    per_flag = {}
    for fl in (0, BACK, FRONT):
        ha, hb = api.trace_rays(a, rays, ray_flags=fl), api.trace_rays(b, rays, ray_flags=fl)
        assert hb.hits.view(np.uint32).tolist() == ha.hits.view(np.uint32).tolist(), f"closest hits, flags {fl:#x}"
        per_flag[fl] = hb.hits.view(np.uint32)
        sa, sb = api.hit_surfaces(a, rays, ha), api.hit_surfaces(b, rays, hb)
        assert vu._np(sb.raw).view(np.uint32).tolist() == vu._np(sa.raw).view(np.uint32).tolist(), f"surfaces (normals, geomNormals), flags {fl:#x}"
        assert_same_bytes(api.trace_rays(b, rays, any_hit=True, ray_flags=fl).occluded, api.trace_rays(a, rays, any_hit=True, ray_flags=fl).occluded, f"any-hit, flags {fl:#x}")
        assert_same_bytes(api.trace_occlusion(b, rays, ray_flags=fl).occluded, api.trace_occlusion(a, rays, ray_flags=fl).occluded, f"queued occlusion, flags {fl:#x}")
    assert (per_flag[BACK] != per_flag[FRONT]).any(), "the two face flags must answer differently somewhere"
    custom = api.trace_rays(b, rays).custom_index
    for k in (tall, short):
        assert (vu._np(custom) == desc.instances[k].customIndex).any(), f"no ray hits the mirrored instance {k}"
    assert state(b) == state(a)
    a.close(); b.close()


# ---- 3. queries and a render equal the twin ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags", BUILDERS, ids=BUILDER_IDS)
@pytest.mark.parametrize("name,which", [("cornell", 0), ("bunny", 1), ("room", -1)])
def test_queries_and_a_render_equal_the_synchronous_twin(gpu_ctx, scene_cache, name, which, flags):
    """cornell: the LIGHT instance moves (light infos and the light-triangle table); the others: an object"""
    s = vu._setup(name)
    desc = _with_flags(s.desc, flags)
    which = which % desc.numInstances
    inst, lights = _moved(s, which, (12.0, -9.0, 7.0), 1.1)
    a = sync_twin(gpu_ctx, desc, inst, lights)
    rays = rays_for(gpu_ctx, s, a, name)
    b = async_twin(gpu_ctx, desc, inst, lights)
    # nothing up to the last line exports or asks for stats: B's host mirrors stay stale
    for opaque in (False, True):
        assert hits_of(b, rays, opaque=opaque) == hits_of(a, rays, opaque=opaque), f"closest hits, opaque={opaque}"
        assert_same_bytes(api.trace_rays(b, rays, any_hit=True, opaque=opaque).occluded, api.trace_rays(a, rays, any_hit=True, opaque=opaque).occluded, "any-hit")
        assert_same_bytes(api.trace_occlusion(b, rays, opaque=opaque).occluded, api.trace_occlusion(a, rays, opaque=opaque).occluded, "queued occlusion")
    view = {"cornell": lambda: scenes.cornell_box(64, 48), "bunny": lambda: scenes.bunny_class(64, 48, subdiv=3), "room": lambda: scenes.textured_room(64, 48)}[name]()
    p = api.make_params(64, 48, spp=1)
    img = _render(gpu_ctx, b, view, p, frame_no=2).download()
    assert np.array_equal(img, _render(gpu_ctx, a, view, p, frame_no=2).download()), "64x48 render"
    assert len(np.unique(img)) > 8
    assert state(b) == state(a)
    a.close(); b.close()


# ---- 4. the mirrors are current -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags", BUILDERS, ids=BUILDER_IDS)
@pytest.mark.parametrize("then", ["vertices_sync", "masks", "rebuild_device", "rebuild_host", "vertices_async", "lights_sync", "create_like", "refused"])
def test_the_mirrors_are_current(gpu_ctx, scene_cache, then, flags):
    """an enqueued instance update, then a call that reads the host copies of the instances or lights: with stale copies the
    instances snap back (the tables are re-uploaded from them, or the new tree is built from them)"""
    s = vu._setup("cornell")
    desc = _with_flags(s.desc, flags)
    ni = desc.numInstances
    old = vu.verts_of(s.desc)
    ranges = changed_ranges(old, smooth(s.desc, old))
    inst, lights = _moved(s, ni - 1, (-60.0, 0.0, -40.0), 1.1)
    tmp = type("T", (), {})()
    tmp.host = type("H", (), {"instances": lambda self=None: inst, "lightInfos": lambda self=None: lights})()
    inst, lights = _moved(tmp, 0, (20.0, -15.0, 10.0))                     # the light moves too: hostLights is a mirror as well
    a, b = api.Scene(gpu_ctx, desc), api.Scene(gpu_ctx, desc)
    b.prepare_async_updates()
    extra = None
    if then == "refused":
        bad = transforms_of(inst)
        bad[3, 1, 2] = float("nan")
        b.update_instances_async(bad, lights=lights_of(lights))
        st = b.update_status()
        assert (st.enqueued, st.refused, st.first_bad_vertex) == (1, 1, 3)
        a.update_vertices(ranges); b.update_vertices(ranges)
    else:
        a.update_instances(inst, lights)
        b.update_instances_async(transforms_of(inst), lights=lights_of(lights))
    if then == "vertices_sync":
        a.update_vertices(ranges); b.update_vertices(ranges)              # instances=None: the prim tables come from hostInstances
    elif then == "masks":
        masks = np.array([0x01 if i % 2 else 0x02 for i in range(ni)], np.uint8)
        a.set_instance_masks(masks); b.set_instance_masks(masks)
        rays = rays_for(gpu_ctx, s, a, "cornell")
        for cm in (0x01, 0x02, 0xff):
            assert hits_of(b, rays, cull_mask=cm) == hits_of(a, rays, cull_mask=cm), f"masked closest hits, cullMask {cm:#x}"
            assert_same_bytes(api.trace_occlusion(b, rays, cull_mask=cm).occluded, api.trace_occlusion(a, rays, cull_mask=cm).occluded, f"masked occlusion {cm:#x}")
        assert hits_of(b, rays, cull_mask=0x01) != hits_of(b, rays, cull_mask=0x02)
        assert state(b) == state(a)
        a.update_vertices(ranges); b.update_vertices_async(on_device(ranges))      # the tables set_instance_masks re-uploaded
    elif then in ("rebuild_device", "rebuild_host"):
        a.rebuild(then[8:]); b.rebuild(then[8:])
        assert state(b) == state(a)
        a.update_vertices(ranges); b.update_vertices_async(on_device(ranges))      # the tables the rebuild prepared again
    elif then == "vertices_async":
        a.update_vertices(ranges); b.update_vertices_async(on_device(ranges))
    elif then == "lights_sync":
        lights[0].intensity = 7.5                                          # rtr_scene_update_lights compares the transforms first
        a.lib.rtr_scene_update_lights(a.h, (A.RtrAreaLightInfo * 1)(*lights), 1)
        rc = b.lib.rtr_scene_update_lights(b.h, (A.RtrAreaLightInfo * 1)(*lights), 1)
        assert rc == 0, b.lib.rtr_last_error()
        a.update_vertices(ranges); b.update_vertices(ranges)              # keeps the lights: from hostLights
    elif then == "create_like":
        d2 = vu.with_vertices(s.desc, old, flags, bytes_to_instances(b), lights)
        extra = api.Scene(gpu_ctx, d2, like=b)
        assert vu.snapshot(extra) == vu.snapshot(a)
    rays = rays_for(gpu_ctx, s, a, "cornell")
    assert_same_answers(a, b, rays, then)
    assert state(b) == state(a)
    if then != "refused":
        assert bytes(b.export_instances()) == bytes((A.RtrInstance * ni)(*inst))
    if extra is not None:
        assert_same_answers(a, extra, rays, "the scene created like it")
        extra.close()
    a.close(); b.close()


def bytes_to_instances(scene):
    """the exported instances as a list of RtrInstance copies: what rtr_scene_create_like's description needs after a device-side move"""
    return [A.RtrInstance.from_buffer_copy(bytes(i)) for i in scene.export_instances()]


# ---- 5. back-to-back updates --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags", BUILDERS, ids=BUILDER_IDS)
def test_eight_updates_in_a_row(gpu_ctx, scene_cache, flags):
    s = vu._setup("bunny")
    desc = _with_flags(s.desc, flags)
    which = 1
    assert which >= desc.numLights

    def phase(k):
        t = k * np.pi / 4
        return _moved(s, which, (40.0 * np.sin(t), 6.0 * k, 40.0 * (1.0 - np.cos(t))), 1.0 + 0.02 * k)

    b = api.Scene(gpu_ctx, desc)
    b.prepare_async_updates()
    tensors = [transforms_of(phase(k)[0][which:which + 1]) for k in range(1, 9)]
    torch.cuda.synchronize()
    for t in tensors:
        b.update_instances_async(t, first_instance=which)
    st = b.update_status()
    assert (st.enqueued, st.refused, st.first_refused_update, st.first_bad_vertex) == (8, 0, None, None)
    a = sync_twin(gpu_ctx, desc, *phase(8))
    assert state(b) == state(a)
    a.close(); b.close()


# ---- 6. refused data ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags", BUILDERS, ids=BUILDER_IDS)
def test_refused_data_changes_nothing(gpu_ctx, scene_cache, flags):
    s = vu._setup("cornell")
    desc = _with_flags(s.desc, flags)
    ni = desc.numInstances
    assert ni >= 6
    b = api.Scene(gpu_ctx, desc)
    b.prepare_async_updates()
    before = state(b)
    verts = b.export_vertices(raw=True).tobytes()
    rays = vu.random_rays(b.stats().boundsMin[:], b.stats().boundsMax[:], 2000, 4, 500.0)
    hits_before = hits_of(b, rays)
    occ_before = api.trace_occlusion(b, rays).occluded
    inst, lights = _moved(s, ni - 1, (5.0, 0.0, -5.0), 1.1)

    def unchanged(what):
        assert state(b) == before, what
        assert b.export_vertices(raw=True).tobytes() == verts, what
        assert hits_of(b, rays) == hits_before, what
        assert_same_bytes(api.trace_occlusion(b, rays).occluded, occ_before, what)

    def poisoned():
        t = transforms_of(inst)
        t[2, 0, 3] = float("nan")
        t[5, 2, 1] = float("inf")
        return t

    def wrong_light():
        out = [A.RtrAreaLightInfo.from_buffer_copy(bytes(l)) for l in lights]
        out[0].numTriangles += 1
        return lights_of(out)

    b.update_instances_async(poisoned(), lights=lights_of(lights))
    st = b.update_status()
    assert (st.enqueued, st.refused, st.first_refused_update, st.first_bad_vertex) == (1, 1, 1, 2)
    unchanged("a non-finite transform")
    b.update_instances_async(transforms_of(inst), lights=wrong_light())
    st = b.update_status()
    assert (st.enqueued, st.refused, st.first_refused_update, st.first_bad_vertex) == (2, 2, 2, ni + 0)
    unchanged("a light that changed its mesh")
    b.update_instances_async(poisoned(), lights=wrong_light())
    st = b.update_status()
    assert (st.enqueued, st.refused, st.first_refused_update, st.first_bad_vertex) == (3, 3, 3, 2)      # the smallest element index
    unchanged("both")
    # a good update lands; the count stays, the "first refused since the last status call" starts again
    b.update_instances_async(transforms_of(inst), lights=lights_of(lights))
    st = b.update_status()
    assert (st.enqueued, st.refused, st.first_refused_update, st.first_bad_vertex) == (4, 3, None, None)
    a = sync_twin(gpu_ctx, desc, inst, lights)
    assert state(b) == state(a)
    a.close(); b.close()


# ---- 7. stream order, no join -------------------------------------------------------------------------------------------------------
def test_the_update_is_stream_ordered_and_does_not_join(scene_cache):
    ctx = api.Context(0)
    stream = torch.cuda.Stream()
    ctx.set_stream(stream.cuda_stream)
    s = vu._setup("bunny")
    desc = _with_flags(s.desc, A.BUILD_DEVICE_LBVH)
    inst, lights = _moved(s, desc.numInstances - 1, (30.0, 4.0, -20.0), 1.1)
    a = sync_twin(ctx, desc, inst, lights)
    b = api.Scene(ctx, desc)
    b.prepare_async_updates()
    with torch.cuda.stream(stream):
        x = torch.rand(4096, 4096, device="cuda")
        dev_new = transforms_of(inst)
    stream.synchronize()
    torch.cuda.synchronize()
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
        t = dev_new * 1.0                             # the transforms are MADE on the stream, behind the filler (x * 1 is exact)
        t0 = time.perf_counter()
        b.update_instances_async(t)
        host_ms = (time.perf_counter() - t0) * 1e3
        done.record(stream)
    pending = not done.query()
    print(f"filler {ms:.1f} ms in {rounds} rounds; the enqueued update returned after {host_ms:.3f} ms on the host; the stream was {'busy' if pending else 'IDLE'}")
    assert pending, "the call waited for the work queued in front of it"
    assert b.update_status().refused == 0
    assert done.query()
    assert state(b) == state(a), "the update read the transforms the stream produced"
    again = _filler_ms(stream, x, rounds)
    print(f"the filler once more: {again:.1f} ms")
    assert again >= 50.0, f"inconclusive: the filler that took {ms:.1f} ms now takes {again:.1f} ms"
    a.close(); b.close()
    ctx.set_stream(None)
    ctx.close()


# ---- 8. refusals before anything is enqueued ----------------------------------------------------------------------------------------
def test_refusals_enqueue_nothing(gpu_ctx, scene_cache):
    s = vu._setup("cornell")
    inst, lights = copies(s)
    ni = len(inst)
    t = transforms_of(inst)
    scene = api.Scene(gpu_ctx, s.desc)
    before = state(scene)
    with pytest.raises(api.RtrError, match="rtr_scene_prepare_async_updates") as e:
        scene.update_instances_async(t)
    assert vu.INVALID_NAME in str(e.value) and "rtr_scene_update_instances_async" in str(e.value)
    assert scene.update_status().enqueued == 0
    scene.prepare_async_updates()
    with pytest.raises(ValueError, match="update_instances"):
        scene.update_instances_async(t.cpu().numpy())
    with pytest.raises(ValueError, match="update_instances"):
        scene.update_instances_async(t, lights=np.zeros(96, np.uint8))
    with pytest.raises(api.RtrError, match="leave the scene's") as e:
        scene.update_instances_async(t, first_instance=1)
    assert "rtr_scene_update_instances_async" in str(e.value)
    with pytest.raises(api.RtrError, match="lights given") as e:
        scene.update_instances_async(t, lights=lights_of(lights + lights))
    assert "rtr_scene_update_instances_async" in str(e.value)
    with pytest.raises(ValueError, match="nothing to update"):
        scene.update_instances_async(None, lights=None)
    with pytest.raises(ValueError, match="must be"):
        scene.update_instances_async(t.reshape(ni, 6, 2))
    with pytest.raises(ValueError, match="instances"):
        scene.update_vertices_async([(0, torch.zeros(1, 3, device="cuda"))], instances=inst)       # the vertex call still takes none
    assert scene.update_status().enqueued == 0
    assert state(scene) == before
    scene.update_instances_async(t)
    assert scene.update_status().enqueued == 1
    assert state(scene) == before          # the same transforms
    scene.close()


# ---- 9. scenes whose root is the only level -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags", BUILDERS, ids=BUILDER_IDS)
@pytest.mark.parametrize("which", ["one", "empty"])
def test_scenes_whose_root_is_the_only_level(gpu_ctx, scene_cache, which, flags):
    natural = {"one": one_triangle_desc, "empty": empty_desc}[which]()      # owns the arrays its copy points at
    desc = _with_flags(natural, flags)
    a, b = api.Scene(gpu_ctx, desc), api.Scene(gpu_ctx, desc)
    b.prepare_async_updates()
    before = state(b)
    if which == "one":
        inst = [A.RtrInstance.from_buffer_copy(bytes(desc.instances[0]))]
        m = matrix(inst, 0); m[:, :3] *= np.float32(1.25); m[:, 3] += np.float32(3.0)
        set_matrix(inst, [], 0, m)
        a.update_instances(inst)
        b.update_instances_async(transforms_of(inst))
        assert state(b) != before
    else:
        a.update_instances([])
        b.update_instances_async(None, lights=[])          # no instances to name: a lights-only update of no lights
        assert state(b) == before
    st = b.update_status()
    assert (st.enqueued, st.refused) == (1, 0)
    assert state(b) == state(a)
    a.close(); b.close()
