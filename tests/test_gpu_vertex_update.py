"""rtr_scene_update_vertices on the device: deforming meshes by a refit.  Results of the queries and of the renderer do not depend on the
tree, so an updated scene is checked bit for bit against a scene freshly built from the new vertices, against the CPU oracle on the
exported tree and against its brute-force loop — for the host-SAH and the device-LBVH builder, on small scenes: cornell_box (36
triangles), bunny_class at subdiv 3 (1 280 triangles: both builders are real) and textured_room (uv and alpha-tested records).

Two deformations: SMOOTH — every object vertex displaced along its normal by a sine of its position, normals recomputed — and FAR — a
mesh pulled so that part of it lands several scene diameters outside the old bounds, so the quantisation grid must follow."""
import ctypes as C

import numpy as np
import pytest
import torch

import conditioned_scenes as cs
from realtimeraytracer_amd import _abi as A
from realtimeraytracer_amd import api, scenes
from test_gpu_bvh import _moved, _render, _with_flags
from test_gpu_occlusion import assert_same_bytes, brute_force_any
from test_gpu_own_leaf import expected_leaves, table_from_export
from test_gpu_query import MISS, assert_hits, brute_force, random_rays
from test_gpu_surfaces import Expect, assert_surfaces
from test_oracle_bvh import _check_bvh
from witness import Witness

pytestmark = pytest.mark.gpu

INVALID_NAME = "RTR_ERR_INVALID_ARGUMENT"
BUILDERS = [A.BUILD_HOST_SAH, A.BUILD_DEVICE_LBVH]
BUILDER_IDS = ["sah", "lbvh"]
SIZES = {"cornell": (96, 64), "bunny": (128, 80), "room": (96, 64)}
BRUTE_BUDGET = 250_000          # ray x triangle pairs of one brute-force loop (a ctypes call each)

_setups, _made = {}, {}


@pytest.fixture(scope="module", autouse=True)
def _cleanup():
    yield
    for m in _made.values():
        m["scene"].close(); m["fresh"].close()
    _made.clear(); _setups.clear()


def _np(x):
    return x.cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)


def _setup(name):
    if name not in _setups:
        w, h = SIZES[name]
        _setups[name] = {"cornell": lambda: scenes.cornell_box(w, h), "bunny": lambda: scenes.bunny_class(w, h, subdiv=3),
                         "room": lambda: scenes.textured_room(w, h)}[name]()
    return _setups[name]


# ---- geometry in numpy --------------------------------------------------------------------------------------------------------------
def verts_of(desc):
    """the description's vertex array as (n, 12) float32: position 0..2, normal 4..6, uv 8..9, pads 3, 7, 10, 11"""
    n = desc.numVertices
    return np.ctypeslib.as_array(C.cast(desc.vertices, C.POINTER(C.c_float)), (n, 12)).copy()


def with_vertices(desc, v12, flags=None, instances=None, lights=None):
    """a copy of the description that carries other vertices (and build flags, instances, lights)"""
    d = A.rtr_scene_desc.from_buffer_copy(bytes(desc))
    arr = (A.RtrVertex * len(v12)).from_buffer_copy(np.ascontiguousarray(v12, np.float32).tobytes())
    d.vertices = C.cast(arr, C.POINTER(A.RtrVertex))
    d._keep = [arr]
    if flags is not None:
        d.buildFlags = flags
    if instances is not None:
        ia = (A.RtrInstance * len(instances))(*instances)
        d.instances = C.cast(ia, C.POINTER(A.RtrInstance)); d._keep.append(ia)
    if lights is not None:
        la = (A.RtrAreaLightInfo * len(lights))(*lights)
        d.lights = C.cast(la, C.POINTER(A.RtrAreaLightInfo)); d._keep.append(la)
    return d


def meshes_of(desc):
    """[(vertexOffset, vertexCount, faces as global vertex ids, is a light's mesh)]"""
    idx = np.ctypeslib.as_array(desc.indices, (desc.numIndices,)).astype(np.int64)
    light_meshes = {desc.instances[i].meshIndex for i in range(desc.numInstances) if desc.instances[i].customIndex < desc.numLights}
    out = []
    for m in range(desc.numMeshes):
        me = desc.meshes[m]
        faces = idx[me.indexOffset: me.indexOffset + me.indexCount].reshape(-1, 3) + me.vertexOffset
        out.append((int(me.vertexOffset), int(me.vertexCount), faces, m in light_meshes))
    return out


def recomputed_normals(desc, v12):
    """area-weighted vertex normals of the new positions, float32; a vertex no triangle with area touches keeps its normal"""
    out = v12.copy()
    acc = np.zeros((len(v12), 3), np.float64)
    for _, _, faces, _ in meshes_of(desc):
        p = v12[:, 0:3].astype(np.float64)
        fn = np.cross(p[faces[:, 1]] - p[faces[:, 0]], p[faces[:, 2]] - p[faces[:, 0]])
        for k in range(3):
            np.add.at(acc, faces[:, k], fn)
    ln = np.linalg.norm(acc, axis=1)
    ok = ln > 0
    out[ok, 4:7] = (acc[ok] / ln[ok, None]).astype(np.float32)
    return out


def _diag(v12):
    return float(np.linalg.norm(v12[:, 0:3].max(0).astype(np.float64) - v12[:, 0:3].min(0)))


def smooth(desc, v12):
    """every object vertex moved along its (area-weighted) normal by a sine of its position (3 % of the scene's diagonal), normals
    recomputed; the stored normals are not used for the direction: a scene loaded without normals stores zeros"""
    out = v12.copy()
    d = _diag(v12)
    along = recomputed_normals(desc, v12)
    for first, count, _, is_light in meshes_of(desc):
        if is_light:
            continue
        p, n = v12[first:first + count, 0:3].astype(np.float64), along[first:first + count, 4:7].astype(np.float64)
        phase = p @ np.array([1.0, 1.7, 0.6]) * (2 * np.pi * 2.5 / d)
        out[first:first + count, 0:3] = (p + 0.03 * d * np.sin(phase)[:, None] * n).astype(np.float32)
    return recomputed_normals(desc, out)


def far(desc, v12):
    """The last object mesh pulled out of the scene along its longest axis: a vertex at one end stays, the other end lands
    (4, 5, -6) scene diameters away, the vertices between them in proportion — part of the mesh ends up 8.8 diameters outside the old
    bounds and the quantisation grid must follow.
    Why a pull and not "every second vertex thrown": that makes every triangle of a tessellated mesh a needle whose edges are the throw
    (15 000 units on bunny_class), and on such triangles rtr_mt_intersect's fp32 t is off by more than the builders' box padding
    (2^-18 of the largest coordinate) — measured on the CPU against a float64 Moeller-Trumbore over this file's random rays: |t32 - t64| up
    to 0.23 units at a padding of 0.042.  The slab test is conservative with respect to the fp32 t only inside that padding
    (include/rtr_math.h, rtr_slab), so for such hits "the result does not depend on the tree", the premise of every comparison here, is
    not defined.  The pull stretches a tessellated mesh evenly (longest edge 978 units on bunny_class, |t32 - t64| <= 0.0014); a mesh of
    a few quads still gets triangles as long as the new scene, as the walls of the Cornell box are as long as the old one."""
    out = v12.copy()
    d = _diag(v12)
    first, count, _, _ = [m for m in meshes_of(desc) if not m[3]][-1]
    p = v12[first:first + count, 0:3].astype(np.float64)
    axis = int(np.argmax(p.max(0) - p.min(0)))
    w = (p[:, axis] - p[:, axis].min()) / (p[:, axis].max() - p[:, axis].min())
    out[first:first + count, 0:3] = (p + w[:, None] * np.array([4.0 * d, 5.0 * d, -6.0 * d])).astype(np.float32)
    return recomputed_normals(desc, out)


def collapsed(desc, v12):
    """every vertex of the last object mesh in one point"""
    out = v12.copy()
    first, count, _, _ = [m for m in meshes_of(desc) if not m[3]][-1]
    out[first:first + count, 0:3] = v12[first:first + count, 0:3].mean(0, dtype=np.float64).astype(np.float32)
    return out


DEFORM = {"smooth": smooth, "far": far}


def changed_ranges(old, new):
    """one (first, positions, normals) per run of changed vertices: packed float3 arrays"""
    diff = (old.view(np.uint32) != new.view(np.uint32)).any(1)
    edges = np.flatnonzero(np.diff(np.concatenate([[0], diff.astype(np.int8), [0]])))
    return [(int(a), np.ascontiguousarray(new[a:b, 0:3]), np.ascontiguousarray(new[a:b, 4:7])) for a, b in zip(edges[0::2], edges[1::2])]


def snapshot(scene):
    ex = scene.export_bvh()
    return (bytes(ex[0]), bytes(ex[1]), bytes(ex[2]), bytes(ex.wide) if ex.wide is not None else b"", scene.export_vertices(raw=True).tobytes())


def made(ctx, name, flags, deform):
    """the scene of `name` after update_vertices with the deformation, a scene freshly built from the deformed vertices, and what the
    tests share about them; built once per form"""
    key = (name, flags, deform)
    if key not in _made:
        s = _setup(name)
        old = verts_of(s.desc)
        new = DEFORM[deform](s.desc, old)
        assert (old[:, 0:3] != new[:, 0:3]).any()
        scene = api.Scene(ctx, _with_flags(s.desc, flags))
        scene.update_vertices(changed_ranges(old, new))
        desc = with_vertices(s.desc, new, flags)
        fresh = api.Scene(ctx, desc)
        _made[key] = {"s": s, "old": old, "new": new, "scene": scene, "fresh": fresh, "desc": desc, "ex": scene.export_bvh(), "fresh_ex": fresh.export_bvh()}
    return _made[key]


def records(tris, n):
    """the triangle records sorted by (customIndex, primitiveId)"""
    raw = np.frombuffer(tris, dtype=np.uint32).reshape(-1, 12)[:n]
    return raw[np.lexsort((raw[:, 7], raw[:, 3]))]


def check_wide(ex, num_tris):
    """the 4-wide view reaches every triangle record exactly once, through leaf codes inside the record array"""
    wide = np.frombuffer(ex.wide, dtype=np.int32).reshape(-1, 16)
    seen = np.zeros(num_tris, np.int32)
    visited = np.zeros(len(wide), bool)
    todo = [0]
    while todo:
        i = todo.pop()
        assert not visited[i], "a 4-wide record has two parents"
        visited[i] = True
        for c in wide[i, 12:16].tolist():
            if c == -2**31:
                continue
            if c >= 0:
                assert c < len(wide)
                todo.append(c)
            else:
                code = ~c
                first, cnt = code >> 3, (code & 7) + 1
                assert first + cnt <= num_tris
                seen[first:first + cnt] += 1
    assert visited.all() and (seen == 1).all()


def query_rays(ctx, m, name, seed=5):
    """(camera rays, a shuffled set: camera rays and random rays through and around the NEW bounds, in random order), as numpy"""
    s = m["s"]
    w, h = SIZES[name]
    cam = _np(api.camera_rays(ctx, s.camera, w, h, 1))
    st = m["scene"].stats()
    d = float(np.linalg.norm(np.array(st.boundsMax[:]) - np.array(st.boundsMin[:])))
    rnd = random_rays(st.boundsMin[:], st.boundsMax[:], 3000, seed, d)
    rng = np.random.default_rng(seed)
    both = np.concatenate([cam[rng.permutation(len(cam))[:2000]], rnd])
    return cam, np.ascontiguousarray(both[rng.permutation(len(both))])


def subsample(rays, num_tris, seed):
    n = int(np.clip(BRUTE_BUDGET // max(num_tris, 1), 100, len(rays)))
    return np.sort(np.random.default_rng(seed).permutation(len(rays))[:n])


# ---- 1. bytes landed ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags", BUILDERS, ids=BUILDER_IDS)
@pytest.mark.parametrize("name", ["cornell", "room"])
def test_bytes_landed(gpu_ctx, scene_cache, name, flags):
    s = _setup(name)
    old = verts_of(s.desc)
    n = len(old)
    rng = np.random.default_rng(3)
    old_marked = old.copy()
    scene = api.Scene(gpu_ctx, _with_flags(s.desc, flags))
    assert scene.export_vertices(raw=True).view(np.uint32).tolist() == old.view(np.uint32).tolist()
    st = scene.export_vertices()
    assert st.dtype.itemsize == 48 and (st["position"] == old[:, 0:3]).all() and (st["uv"] == old[:, 8:10]).all()
    if name == "room":
        assert old[:, 8:10].any(), "the room has texture coordinates"
    expect = old_marked.copy()
    a0, a1, b0, b1 = 1, n // 3, n // 2, n - 2             # two disjoint ranges, neither at a mesh boundary
    for stride in (12, 16, 48):
        for with_normals in (False, True):
            new = expect.copy()
            for a, b in ((a0, a1), (b0, b1)):
                new[a:b, 0:3] = (expect[a:b, 0:3] + rng.normal(0, 1.0, (b - a, 3))).astype(np.float32)
                if with_normals:
                    new[a:b, 4:7] = rng.normal(0, 1.0, (b - a, 3)).astype(np.float32)
            ranges = []
            for a, b in ((a0, a1), (b0, b1)):
                if stride == 12:
                    p, q = np.ascontiguousarray(new[a:b, 0:3]), np.ascontiguousarray(new[a:b, 4:7])
                elif stride == 16:
                    p4, q4 = np.full((b - a, 4), 7.0, np.float32), np.full((b - a, 4), 9.0, np.float32)
                    p4[:, 0:3], q4[:, 0:3] = new[a:b, 0:3], new[a:b, 4:7]
                    p, q = p4, q4                         # (n, 4): the first three columns are used
                else:
                    rec = np.full((b - a, 12), 5.0, np.float32)      # RtrVertex records whose uv and pads must NOT land
                    rec[:, 0:3], rec[:, 4:7] = new[a:b, 0:3], new[a:b, 4:7]
                    p, q = rec[:, 0:3], rec[:, 4:7]       # normals = base + 16
                    assert p.strides == (48, 4) and q.ctypes.data == p.ctypes.data + 16
                ranges.append((a, p, q) if with_normals else (a, p))
            scene.update_vertices(ranges)
            if not with_normals:
                new[:, 4:7] = expect[:, 4:7]
            got = scene.export_vertices(raw=True)
            assert got.view(np.uint32).tolist() == new.view(np.uint32).tolist(), (stride, with_normals)
            assert (got[:, [3, 7, 8, 9, 10, 11]].view(np.uint32) == old[:, [3, 7, 8, 9, 10, 11]].view(np.uint32)).all()
            for a, b in ((0, a0), (a1, b0), (b1, n)):
                assert (got[a:b].view(np.uint32) == old[a:b].view(np.uint32)).all(), "vertices outside the ranges"
            expect = new
    # an empty range among the ranges, and a range that spans meshes
    assert s.desc.numMeshes > 1 and s.desc.meshes[0].vertexCount < b1
    scene.update_vertices([(0, np.zeros((0, 3), np.float32)), (a0, np.ascontiguousarray(old[a0:b1, 0:3]), np.ascontiguousarray(old[a0:b1, 4:7]))])
    assert scene.export_vertices(raw=True).view(np.uint32).tolist() == old.view(np.uint32).tolist()
    scene.close()


# ---- 2. records and tree ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags", BUILDERS, ids=BUILDER_IDS)
@pytest.mark.parametrize("deform", ["smooth", "far"])
@pytest.mark.parametrize("name", ["cornell", "bunny", "room"])
def test_records_equal_a_fresh_build_and_the_tree_holds(gpu_ctx, scene_cache, name, deform, flags):
    m = made(gpu_ctx, name, flags, deform)
    scene, st = m["scene"], m["scene"].stats()
    nodes, tris, grid = m["ex"]
    n = st.numTriangles
    assert n == m["fresh"].stats().numTriangles
    assert np.array_equal(records(tris, n), records(m["fresh_ex"][1], n)), "records of the update != records of a fresh build"
    assert scene.export_vertices(raw=True).view(np.uint32).tolist() == m["new"].view(np.uint32).tolist()
    _check_bvh(m["desc"], st, nodes, tris, grid)
    cs.check_padding(nodes, tris, grid, st)
    check_wide(m["ex"], n)
    assert st.numWideNodes == len(m["ex"].wide)
    if deform == "far":                                                # the grid followed the geometry
        old_st = api.host_build_bvh(m["s"].desc)[0]
        assert max(st.grid.scale[:]) > 2 * max(old_st.grid.scale[:]) and st.boxPad > 2 * old_st.boxPad


# ---- 3. queries ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags", BUILDERS, ids=BUILDER_IDS)
@pytest.mark.parametrize("deform", ["smooth", "far"])
@pytest.mark.parametrize("name", ["cornell", "bunny", "room"])
def test_queries_equal_a_fresh_build_and_brute_force(gpu_ctx, oracle, scene_cache, name, deform, flags):
    m = made(gpu_ctx, name, flags, deform)
    scene, fresh, ex = m["scene"], m["fresh"], m["ex"]
    ntri = scene.stats().numTriangles
    alpha = bool((np.frombuffer(ex[1], dtype=np.uint32).reshape(-1, 12)[:, 11] & 1).any())
    assert alpha == (name == "room")
    cam, shuffled = query_rays(gpu_ctx, m, name)
    for what, rays in (("camera rays", cam), ("shuffled set", shuffled)):
        sub = subsample(rays, ntri, 9)
        exp = brute_force(oracle, ex, rays[sub], opaque=True)
        assert (exp[3] != MISS).mean() > 0.05, what
        exp_any = None if alpha else brute_force_any(oracle, ex, rays[sub])
        for opaque in (False, True):
            tag = f"{name} {deform} {what} opaque={opaque}"
            got, ref = api.trace_rays(scene, rays, opaque=opaque), api.trace_rays(fresh, rays, opaque=opaque)
            assert got.hits.view(np.uint32).tolist() == ref.hits.view(np.uint32).tolist(), f"{tag}: closest hits != a fresh build's"
            if opaque or not alpha:
                sel = api.QueryResult()
                sel.t, sel.u, sel.v, sel.custom_index, sel.primitive_id = (getattr(got, k)[sub] for k in ("t", "u", "v", "custom_index", "primitive_id"))
                assert_hits(sel, exp, tag)
            occ = api.trace_rays(scene, rays, any_hit=True, opaque=opaque).occluded
            assert_same_bytes(occ, api.trace_rays(fresh, rays, any_hit=True, opaque=opaque).occluded, f"{tag}: RTR_QUERY_ANY vs fresh")
            queued = api.trace_occlusion(scene, rays, opaque=opaque).occluded
            assert_same_bytes(queued, occ, f"{tag}: rtr_trace_occlusion vs dense")
            assert_same_bytes(queued, api.trace_occlusion(fresh, rays, opaque=opaque).occluded, f"{tag}: rtr_trace_occlusion vs fresh")
            if exp_any is not None:
                assert_same_bytes(occ[sub], exp_any, f"{tag}: RTR_QUERY_ANY vs brute force")
            elif opaque:
                assert_same_bytes(occ[sub], (exp[3] != MISS).astype(np.uint8), f"{tag}: RTR_QUERY_ANY vs brute force")
    # surfaces: normals follow the new vertex normals (the float64 witness of the new description), uv is the old uv
    hits = api.trace_rays(scene, cam)
    surf, fsurf = api.hit_surfaces(scene, cam, hits), api.hit_surfaces(fresh, cam, hits)
    assert surf.raw.view(np.uint32).tolist() == fsurf.raw.view(np.uint32).tolist(), "surfaces != a fresh build's"
    if deform == "smooth":
        assert_surfaces(surf, Expect(Witness(m["desc"]), cam, hits.hits), f"{name} {deform} surfaces")
        keep = with_vertices(m["s"].desc, np.concatenate([m["new"][:, 0:4], m["old"][:, 4:8], m["new"][:, 8:12]], 1))     # old normals
        e_old = Expect(Witness(keep), cam, hits.hits)
        e_new = Expect(Witness(m["desc"]), cam, hits.hits)
        obj = e_new.kind == A.SURFACE_OBJECT
        assert (np.abs(e_new.val["normal"][obj] - e_old.val["normal"][obj]).max(1) > 1e-3).mean() > 0.05, "the deformation turns normals"
        assert np.array_equal(e_new.val["uv"], e_old.val["uv"])


# ---- 4. the renderer ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags", BUILDERS, ids=BUILDER_IDS)
@pytest.mark.parametrize("name,deform", [("cornell", "smooth"), ("cornell", "far"), ("bunny", "smooth"), ("bunny", "far"), ("room", "smooth")])
def test_render_equals_a_fresh_build_and_the_oracle(gpu_ctx, oracle, scene_cache, name, deform, flags):
    m = made(gpu_ctx, name, flags, deform)
    s, (w, h) = m["s"], SIZES[name]
    p = api.make_params(w, h, spp=1, collect_stats=1)
    f = _render(gpu_ctx, m["scene"], s, p, frame_no=2)
    img = f.download()
    assert np.array_equal(img, _render(gpu_ctx, m["fresh"], s, p, frame_no=2).download()), "image != a fresh build's"
    ref = oracle.render(m["desc"], s.camera, s.scene_info(2), p, bvh=m["ex"], threads=16)
    assert np.array_equal(img, ref.images[A.IMAGE_SHADOWED]), "image != the oracle's on the exported tree"
    g = f.stats()
    assert (g.numRays, g.numNodeVisits, g.numTriTests, g.numHits) == (ref.stats.numRays, ref.stats.numNodeVisits, ref.stats.numTriTests, ref.stats.numHits)
    brute = oracle.render(m["desc"], s.camera, s.scene_info(2), p, bvh=None, threads=16)
    assert np.array_equal(img, brute.images[A.IMAGE_SHADOWED]), "image != the oracle's brute force"
    p0 = api.make_params(w, h, spp=1, collect_stats=0)
    assert np.array_equal(_render(gpu_ctx, m["scene"], s, p0, frame_no=2).download(), img), "the timed kernels"
    before = _render(gpu_ctx, api.Scene(gpu_ctx, s.desc), s, p0, frame_no=2).download()
    assert not np.array_equal(before, img), "the deformation is visible"


# ---- 5. a deformed light ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags", BUILDERS, ids=BUILDER_IDS)
def test_a_deformed_light_remakes_the_light_triangle_table(gpu_ctx, scene_cache, flags):
    s, (w, h) = _setup("cornell"), SIZES["cornell"]
    old = verts_of(s.desc)
    first, count, _, _ = [m for m in meshes_of(s.desc) if m[3]][0]
    new = old.copy()
    c = old[first:first + count, 0:3].mean(0)
    new[first:first + count, 0:3] = (c + (old[first:first + count, 0:3] - c) * np.float32(0.5) + np.array([30.0, 0.0, -40.0], np.float32)).astype(np.float32)
    scene = api.Scene(gpu_ctx, _with_flags(s.desc, flags))
    p = api.make_params(w, h, spp=1)
    before = _render(gpu_ctx, scene, s, p).download()
    rays = api.camera_rays(gpu_ctx, s.camera, w, h, 1)
    lp = api.make_light_params(s.num_lights, 3, 0, w, 1, outputs=A.LIGHT_SHADOWED | A.LIGHT_UNSHADOWED)
    rad_before = _np(api.direct_light(scene, rays, params=lp).raw).copy()
    scene.update_vertices([(first, np.ascontiguousarray(new[first:first + count, 0:3]))])
    fresh = api.Scene(gpu_ctx, with_vertices(s.desc, new, flags))
    img = _render(gpu_ctx, scene, s, p).download()
    assert not np.array_equal(img, before)
    assert np.array_equal(img, _render(gpu_ctx, fresh, s, p).download()), "image with the moved light != a fresh build's"
    rad, frad = _np(api.direct_light(scene, rays, params=lp).raw), _np(api.direct_light(fresh, rays, params=lp).raw)
    assert rad.view(np.uint32).tolist() == frad.view(np.uint32).tolist(), "direct_light radiance != a fresh build's"
    assert not np.array_equal(rad, rad_before)
    scene.close(); fresh.close()


# ---- 6. host route = device route ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags", BUILDERS, ids=BUILDER_IDS)
@pytest.mark.parametrize("name,deform", [("cornell", "smooth"), ("bunny", "far")])       # one range of everything; 88 ranges
def test_host_route_equals_device_route(gpu_ctx, scene_cache, name, deform, flags):
    m = made(gpu_ctx, name, flags, deform)
    s, old, new = m["s"], m["old"], m["new"]
    want = snapshot(m["scene"])                                        # the host route, packed float3 ranges
    dev_new = torch.from_numpy(new).cuda()
    n = len(new)
    p4 = torch.full((n, 4), 3.0, device="cuda"); p4[:, 0:3] = dev_new[:, 0:3]
    q4 = torch.full((n, 4), 4.0, device="cuda"); q4[:, 0:3] = dev_new[:, 4:7]
    forms = {
        "packed tensors per range": [(a, torch.from_numpy(p).cuda(), torch.from_numpy(q).cuda()) for a, p, q in changed_ranges(old, new)],
        "a non-contiguous (n, 4)[:, :3] view": [(0, p4[:, :3], q4[:, :3])],
        "rows of the RtrVertex tensor": [(0, dev_new[:, 0:3], dev_new[:, 4:7])],
        "the same rows from numpy": [(0, new[:, 0:3], new[:, 4:7])],
    }
    assert not forms["a non-contiguous (n, 4)[:, :3] view"][0][1].is_contiguous()
    for what, ranges in forms.items():
        scene = api.Scene(gpu_ctx, _with_flags(s.desc, flags))
        scene.update_vertices(ranges)
        assert snapshot(scene) == want, what
        scene.close()
    with pytest.raises(ValueError, match="mixture"):
        m["scene"].update_vertices([(0, new[:, 0:3], dev_new[:, 4:7])])
    # a tensor made on another stream just before the call: the call orders itself behind it
    side = torch.cuda.Stream()
    scene = api.Scene(gpu_ctx, _with_flags(s.desc, flags))
    with torch.cuda.stream(side):
        late = dev_new.clone()
        scene.update_vertices([(0, late[:, 0:3], late[:, 4:7])])
    assert snapshot(scene) == want, "data enqueued on another stream"
    scene.close()


# ---- 7. one refit for both ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags", BUILDERS, ids=BUILDER_IDS)
def test_one_refit_carries_vertices_instances_and_lights(gpu_ctx, scene_cache, flags):
    m = made(gpu_ctx, "cornell", flags, "smooth")
    s, ranges = m["s"], changed_ranges(m["old"], m["new"])
    inst, lights = _moved(s, len(s.host.instances()) - 1, (-60.0, 0.0, -30.0))
    tmp = type("T", (), {})()
    tmp.host = type("H", (), {"instances": lambda self=None: inst, "lightInfos": lambda self=None: lights})()
    inst, lights = _moved(tmp, 0, (20.0, -15.0, 10.0))
    one = api.Scene(gpu_ctx, _with_flags(s.desc, flags))
    one.update_vertices(ranges, instances=inst, lights=lights)
    two = api.Scene(gpu_ctx, _with_flags(s.desc, flags))
    two.update_instances(inst, lights)
    two.update_vertices(ranges)
    assert snapshot(one) == snapshot(two)
    assert snapshot(one) != snapshot(m["scene"]), "the instances moved"
    w, h = SIZES["cornell"]
    p = api.make_params(w, h, spp=1)
    fresh = api.Scene(gpu_ctx, with_vertices(s.desc, m["new"], flags, inst, lights))
    assert np.array_equal(_render(gpu_ctx, one, s, p).download(), _render(gpu_ctx, fresh, s, p).download())
    rays = api.camera_rays(gpu_ctx, s.camera, w, h, 1)
    lp = api.make_light_params(s.num_lights, 3, 0, w, 1)
    assert _np(api.direct_light(one, rays, params=lp).raw).view(np.uint32).tolist() == _np(api.direct_light(fresh, rays, params=lp).raw).view(np.uint32).tolist()
    for x in (one, two, fresh):
        x.close()


# ---- 8. round trip ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags", BUILDERS, ids=BUILDER_IDS)
@pytest.mark.parametrize("name", ["cornell", "bunny"])
def test_round_trip_restores_image_and_tree(gpu_ctx, scene_cache, name, flags):
    s, (w, h) = _setup(name), SIZES[name]
    old = verts_of(s.desc)
    scene = api.Scene(gpu_ctx, _with_flags(s.desc, flags))
    p = api.make_params(w, h, spp=1)
    image, original = _render(gpu_ctx, scene, s, p).download(), snapshot(scene)
    for deform in ("smooth", "far"):
        new = DEFORM[deform](s.desc, old)
        scene.update_vertices(changed_ranges(old, new))
        assert snapshot(scene) != original
        assert not np.array_equal(_render(gpu_ctx, scene, s, p).download(), image)
        scene.update_vertices([(a, q, r) for a, q, r in changed_ranges(new, old)])
        assert np.array_equal(_render(gpu_ctx, scene, s, p).download(), image), f"{deform}: the original image"
        back = snapshot(scene)
        for part, a, b in zip(("nodes", "records", "grid", "4-wide view", "vertices"), back, original):
            assert a == b, f"{deform}: {part} differ from the original export"
    scene.close()


# ---- 9. what survives ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags", BUILDERS, ids=BUILDER_IDS)
def test_masks_leaves_and_hints_survive(gpu_ctx, oracle, scene_cache, flags):
    name = "cornell"
    s, (w, h) = _setup(name), SIZES[name]
    old = verts_of(s.desc)
    new = smooth(s.desc, old)
    scene = api.Scene(gpu_ctx, _with_flags(s.desc, flags))
    ninst = s.desc.numInstances
    masks = np.array([(0x01, 0x02, 0x04, 0xff, 0x03)[k % 5] for k in range(ninst)], np.uint8)
    scene.set_instance_masks(masks)
    rays = api.camera_rays(gpu_ctx, s.camera, w, h, 1)
    hits_before = api.trace_rays(scene, rays).hits
    leaves_before = _np(api.hit_leaves(scene, hits_before))            # the table exists before the update
    scene.update_vertices(changed_ranges(old, new))
    assert (scene.instance_masks() == masks).all()
    ex = scene.export_bvh()
    raw = np.frombuffer(ex[1], dtype=np.uint32).reshape(-1, 12)
    by_custom = np.zeros(ninst, np.uint32)
    for i in range(ninst):
        by_custom[s.desc.instances[i].customIndex] = masks[i]
    assert (((~raw[:, 11]) >> 8) & 0xff == by_custom[raw[:, 3]]).all(), "the records carry the masks after the update"
    rn = _np(rays)
    sub = subsample(rn, len(raw), 4)
    for cull in (0x01, 0x06):
        alive = raw[(by_custom[raw[:, 3]] & cull) != 0]
        assert 0 < len(alive) < len(raw)
        exp = brute_force(oracle, (None, alive.tobytes(), None), rn[sub], opaque=True)
        got = api.trace_rays(scene, rays, cull_mask=cull)
        sel = api.QueryResult()
        sel.t, sel.u, sel.v, sel.custom_index, sel.primitive_id = (_np(getattr(got, k))[sub] for k in ("t", "u", "v", "custom_index", "primitive_id"))
        assert_hits(sel, exp, f"masked query, cull mask {cull:#x}")
        occ = api.trace_occlusion(scene, rays, cull_mask=cull).occluded
        assert_same_bytes(occ[torch.from_numpy(sub).cuda()], (exp[3] != MISS).astype(np.uint8), f"masked occlusion, cull mask {cull:#x}")
    # the triangle -> leaf table: topology and leaf order are kept, so the leaves of the same ids are the same and match the fresh export
    hits = api.trace_rays(scene, rays).hits
    table = table_from_export(ex)
    assert (_np(api.hit_leaves(scene, hits)) == expected_leaves(table, hits)).all()
    assert (_np(api.hit_leaves(scene, hits_before)) == leaves_before).all()
    assert (expected_leaves(table, hits_before) == leaves_before).all()
    # hinted occlusion bytes equal the dense ones
    lp = api.make_light_params(s.num_lights, 3, 1, w, 1)
    lr, lv = api.light_rays(scene, rays, hits, lp, hints=True)
    assert bool((lv < 0).any())
    dense = api.trace_rays(scene, lr, any_hit=True).occluded
    assert_same_bytes(api.trace_occlusion(scene, lr, start_leaves=lv).occluded, dense, "hinted occlusion after the update")
    assert bool(dense.any()) and not bool(dense.all())
    scene.close()


# ---- 10. a degenerate result --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags", BUILDERS, ids=BUILDER_IDS)
@pytest.mark.parametrize("name", ["cornell", "bunny"])
def test_a_mesh_collapsed_to_a_point_is_never_hit(gpu_ctx, oracle, scene_cache, name, flags):
    s, (w, h) = _setup(name), SIZES[name]
    old = verts_of(s.desc)
    new = collapsed(s.desc, old)
    scene = api.Scene(gpu_ctx, _with_flags(s.desc, flags))
    scene.update_vertices(changed_ranges(old, new))                    # succeeds
    ex = scene.export_bvh()
    raw = np.frombuffer(ex[1], dtype=np.uint32).reshape(-1, 12)
    flat = ~raw.view(np.float32)[:, [4, 5, 6, 8, 9, 10]].any(1)
    assert flat.sum() >= 4, "the collapsed mesh's records have zero edges"
    gone = set(np.unique(raw[flat, 3]).tolist())
    m = {"s": s, "scene": scene}
    cam, shuffled = query_rays(gpu_ctx, m, name)
    for what, rays in (("camera rays", cam), ("shuffled set", shuffled)):
        sub = subsample(rays, len(raw), 2)
        exp = brute_force(oracle, ex, rays[sub], opaque=True)
        got = api.trace_rays(scene, rays)
        assert not (set(np.unique(got.custom_index).tolist()) & gone), "a zero-area triangle was hit"
        sel = api.QueryResult()
        sel.t, sel.u, sel.v, sel.custom_index, sel.primitive_id = (getattr(got, k)[sub] for k in ("t", "u", "v", "custom_index", "primitive_id"))
        assert_hits(sel, exp, f"{name} collapsed, {what}")
        occ = api.trace_rays(scene, rays, any_hit=True).occluded
        assert_same_bytes(occ[sub], brute_force_any(oracle, ex, rays[sub]), f"{name} collapsed, {what}, any hit")
        assert_same_bytes(api.trace_occlusion(scene, rays).occluded, occ, f"{name} collapsed, {what}, queued")
    scene.close()


# ---- 11. refusals leave the scene unchanged -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags", BUILDERS, ids=BUILDER_IDS)
def test_refusals_leave_the_scene_unchanged(gpu_ctx, scene_cache, flags):
    s = _setup("cornell")
    old = verts_of(s.desc)
    n = len(old)
    scene = api.Scene(gpu_ctx, _with_flags(s.desc, flags))
    scene.update_vertices([(0, np.ascontiguousarray(old[:, 0:3]))])    # a scene that has been refitted once: the device arrays are live
    before = snapshot(scene)
    lib = scene.lib
    good = np.ascontiguousarray(old[4:20, 0:3] + np.float32(1.0))
    other = np.ascontiguousarray(old[30:40, 0:3] + np.float32(1.0))

    def refused(call, *needles):
        with pytest.raises(api.RtrError) as e:
            call()
        assert e.value.status_name == INVALID_NAME and e.value.status == -1, str(e.value)
        for needle in needles:
            assert needle in str(e.value), str(e.value)
        assert snapshot(scene) == before, f"the scene changed although the call was refused: {e.value}"

    for bad_value in (np.nan, np.inf, -np.inf):
        bad = other.copy(); bad[7, 1] = bad_value
        refused(lambda: scene.update_vertices([(4, good), (30, bad)]), "range 1, vertex 7", "scene vertex 37", "non-finite")
        refused(lambda: scene.update_vertices([(4, torch.from_numpy(good).cuda()), (30, torch.from_numpy(bad).cuda())]),
                "range 1, vertex 7", "scene vertex 37", "non-finite")
    # the FIRST bad vertex in range order is named, whichever lane finds one first
    many = np.ascontiguousarray(old[:, 0:3]).copy(); many[n // 2:, 0] = np.nan
    refused(lambda: scene.update_vertices([(0, torch.from_numpy(many).cuda())]), f"range 0, vertex {n // 2} ")
    # a NaN normal is not an error: normals are shading data
    nrm = np.ascontiguousarray(old[4:20, 4:7]); nrm[0, 0] = np.nan
    probe = api.Scene(gpu_ctx, _with_flags(s.desc, flags))
    probe.update_vertices([(4, np.ascontiguousarray(old[4:20, 0:3]), nrm)])
    assert np.isnan(probe.export_vertices(raw=True)[4, 4])
    probe.close()
    refused(lambda: scene.update_vertices([(4, good), (10, other)]), "overlap")
    refused(lambda: scene.update_vertices([(10, other), (4, good)]), "overlap")
    refused(lambda: scene.update_vertices([(n - 5, other)]), "leaves the scene's")
    refused(lambda: scene.update_vertices([(0xfffffff0, other)]), "leaves the scene's")
    inst = [A.RtrInstance.from_buffer_copy(bytes(i)) for i in s.host.instances()]
    inst[3].meshIndex = 1
    refused(lambda: scene.update_vertices([(4, good)], instances=inst), "rtr_scene_update_vertices", "instance 3 changed mesh")
    inst = [A.RtrInstance.from_buffer_copy(bytes(i)) for i in s.host.instances()]
    refused(lambda: scene.update_vertices([(4, good)], instances=inst[:-1]), "instances given")
    inst[2].transform[3] = float("nan")
    refused(lambda: scene.update_vertices([(4, good)], instances=inst), "non-finite transform")
    lights = [A.RtrAreaLightInfo.from_buffer_copy(bytes(l)) for l in s.host.lightInfos()]
    lights[0].numTriangles += 1
    refused(lambda: scene.update_vertices([(4, good)], lights=lights), "light 0 changed its mesh")

    # what the Python layer cannot express goes through the C ABI
    def raw_call(table, count, pstride, nstride, route):
        def call():
            api._check(lib.rtr_scene_update_vertices(scene.h, table, count, pstride, nstride, route, None, 0, None, 0), "rtr_scene_update_vertices")
        return call

    dev = torch.from_numpy(np.zeros((64, 4), np.float32)).cuda()
    host_tab = (A.rtr_vertex_range * 1)(A.rtr_vertex_range(4, 16, good.ctypes.data, None))
    for stride in (10, 8):
        refused(raw_call(host_tab, 1, stride, 12, A.VERTICES_HOST), "positionStride")
    with_n = (A.rtr_vertex_range * 1)(A.rtr_vertex_range(4, 16, good.ctypes.data, good.ctypes.data))
    for stride in (10, 8):
        refused(raw_call(with_n, 1, 12, stride, A.VERTICES_HOST), "normalStride")
    refused(raw_call((A.rtr_vertex_range * 1)(A.rtr_vertex_range(4, 16, dev.data_ptr() + 2, None)), 1, 16, 16, A.VERTICES_DEVICE), "4-byte aligned")
    refused(raw_call((A.rtr_vertex_range * 1)(A.rtr_vertex_range(4, 16, dev.data_ptr(), dev.data_ptr() + 1)), 1, 16, 16, A.VERTICES_DEVICE), "4-byte aligned")
    refused(raw_call((A.rtr_vertex_range * 1)(A.rtr_vertex_range(4, 16, None, None)), 1, 12, 12, A.VERTICES_HOST), "null positions")
    refused(raw_call(host_tab, 1, 12, 12, 2), "unknown flag bits")
    refused(raw_call(host_tab, 0, 12, 12, A.VERTICES_HOST), "numRanges == 0")
    refused(raw_call(None, 1, 12, 12, A.VERTICES_HOST), "null ranges")
    with pytest.raises(api.RtrError):
        api._check(lib.rtr_scene_export_vertices(scene.h, (C.c_char * 48)(), 48 * (n + 1)), "rtr_scene_export_vertices")
    # and the scene still takes a good update
    scene.update_vertices([(4, good), (30, other)])
    got = scene.export_vertices(raw=True)
    assert (got[4:20, 0:3] == good).all() and (got[30:40, 0:3] == other).all() and snapshot(scene) != before
    scene.close()


def test_an_empty_scene_takes_the_call_and_does_nothing(gpu_ctx):
    d = A.rtr_scene_desc()
    d.skyColor[0] = d.skyColor[1] = d.skyColor[2] = 0.5
    scene = api.Scene(gpu_ctx, d)
    assert scene.export_vertices().shape == (0,)
    scene.update_vertices([(0, np.zeros((0, 3), np.float32))])
    with pytest.raises(api.RtrError):
        scene.update_vertices([(0, np.zeros((1, 3), np.float32))])      # there is no vertex 0
    scene.close()
