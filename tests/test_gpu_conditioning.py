"""Device BVH builds, refits, ray queries and renders on badly conditioned geometry (tests/conditioned_scenes.py): scenes far from the
origin, millimetre-sized, huge, seen from 1000 scene sizes away, and the Morton / Karras edge cases (identical triangles, a flat scene,
20 000 triangles on a line, a 1e4 / 1e-3 size mix, 15 / 16 / 17 / 255 / 256 / 257 / 4097 triangles).  Every case is built by the host
SAH builder and by the device LBVH; the placement cases again by refit (built where the scene naturally sits, then moved into place by
update_instances).  Trees keep their invariants, queries equal the brute force bit for bit, renders equal the oracle's."""
import numpy as np
import pytest

import conditioned_scenes as cs
from realtimeraytracer_amd import _abi as A
from realtimeraytracer_amd import api
from test_gpu_query import MISS, assert_hits, brute_force, oracle_camera_hits
from test_oracle_bvh import _check_bvh

pytestmark = pytest.mark.gpu

W, H, SPP = 96, 54, 2
BUILDERS = {"sah": A.BUILD_HOST_SAH, "lbvh": A.BUILD_DEVICE_LBVH}
FORMS = [(n, b, False) for n in cs.ALL for b in BUILDERS] + [(n, b, True) for n in cs.ALL if n.startswith(cs.PLACED) for b in BUILDERS]
IDS = [f"{n}-{b}{'-refit' if r else ''}" for n, b, r in FORMS]
BRUTE_BUDGET = 600_000           # oracle_mt calls per case (ctypes, one ray and triangle at a time)

_cases, _scenes, _expect, _ref = {}, {}, {}, {}


@pytest.fixture(scope="module")
def made(tmp_path_factory):
    yield tmp_path_factory
    for s, _ in _scenes.values():
        s.close()
    _scenes.clear(); _cases.clear(); _expect.clear(); _ref.clear()


def _flags(desc, flags):
    d = A.rtr_scene_desc.from_buffer_copy(bytes(desc))
    d.buildFlags = flags
    return d


def _case(made, name):
    if name not in _cases:
        _cases[name] = cs.case(name, made.mktemp(name.replace("-", "_")))
    return _cases[name]


def _scene(ctx, made, name, builder, refit):
    """the case's scene and its exported tree, built once per form and shared by the tests"""
    key = (name, builder, refit)
    if key not in _scenes:
        c = _case(made, name)
        if refit:
            s = api.Scene(ctx, _flags(c.natural, BUILDERS[builder]))
            s.update_instances(c.instances, c.lights)
        else:
            s = api.Scene(ctx, _flags(c.desc, BUILDERS[builder]))
        _scenes[key] = (s, s.export_bvh())
    return _scenes[key]


def _records(tris, n):
    """the triangle records sorted by (customIndex, primitiveId): what any builder must produce, in its own order"""
    raw = np.frombuffer(tris, dtype=np.uint32).reshape(-1, 12)[:n]
    return raw[np.lexsort((raw[:, 7], raw[:, 3]))]


# ---- tree invariants --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,builder,refit", FORMS, ids=IDS)
def test_tree_invariants(gpu_ctx, made, scene_cache, name, builder, refit):
    c = _case(made, name)
    scene, ex = _scene(gpu_ctx, made, name, builder, refit)
    st = scene.stats()
    nodes, tris, grid = ex
    _check_bvh(c.desc, st, nodes, tris, grid)
    cs.check_padding(nodes, tris, grid, st)
    assert st.numTriangles == c.num_triangles
    assert st.maxDepth <= 64 and st.stackEntries >= st.maxDepth
    host = api.host_build_bvh_wide(c.desc)
    # k_world_prims (build and refit) writes the records the host packer writes, bit for bit
    assert np.array_equal(_records(tris, st.numTriangles), _records(host[1], st.numTriangles))
    if builder == "lbvh" and st.numTriangles >= 16:
        assert st.numNodes == st.numTriangles - 1
    if name == "graded":                                               # the case that keeps k_query_tail under test
        assert st.maxDepth > 16
    if refit:
        return
    if builder == "sah" or st.numTriangles < 16:                       # below 16 triangles the device build falls back to the host builder
        assert bytes(nodes) == bytes(host[0]) and bytes(tris) == bytes(host[1])
        assert (grid.wideCentreXY, grid.wideCentreZ) == (host.stats.grid.wideCentreXY, host.stats.grid.wideCentreZ)
        assert bytes(ex.wide) == bytes(host.wide)
    else:
        again = api.Scene(gpu_ctx, _flags(c.desc, A.BUILD_DEVICE_LBVH))
        try:
            n2, t2, g2 = ex2 = again.export_bvh()
        finally:
            again.close()
        assert bytes(n2) == bytes(nodes) and bytes(t2) == bytes(tris) and bytes(g2) == bytes(grid) and bytes(ex2.wide) == bytes(ex.wide)


# ---- queries ----------------------------------------------------------------------------------------------------------------------
def _expected(oracle, made, name):
    """the case's rays and their brute-force closest hits (shared by every form: the records are the same), plus the camera rays' hits"""
    if name not in _expect:
        c = _case(made, name)
        st, nodes, tris = api.host_build_bvh(c.desc)
        bvh = (nodes, tris, st.grid)
        n = int(np.clip(BRUTE_BUDGET // c.num_triangles, 64, 2000))
        r = cs.rays(c, n, seed=11)
        exp = brute_force(oracle, bvh, r)
        tr, _ = cs.tight(r, exp[0], exp[3] != MISS, max(8, n // 8), seed=12)
        if len(tr):
            exp = tuple(np.concatenate([a, b]) for a, b in zip(exp, brute_force(oracle, bvh, tr)))
            r = np.concatenate([r, tr])
        _expect[name] = (r, exp, oracle_camera_hits(oracle, _Setup(c), W, H, SPP, None))
    return _expect[name]


class _Setup:
    """desc + camera of a moved case, in the shape oracle_camera_hits reads"""
    def __init__(self, c):
        self.desc, self.camera = c.desc, c.camera


@pytest.mark.parametrize("name,builder,refit", FORMS, ids=IDS)
def test_queries_equal_brute_force(gpu_ctx, oracle, made, scene_cache, name, builder, refit):
    c = _case(made, name)
    scene, ex = _scene(gpu_ctx, made, name, builder, refit)
    rays, exp, cam_exp = _expected(oracle, made, name)
    found = exp[3] != MISS
    assert found.mean() > 0.05
    for opaque in (False, True):                                       # no alpha-tested geometry: both modes give the brute force
        res = api.trace_rays(scene, rays, opaque=opaque, collect_stats=True)
        assert_hits(res, exp, f"{name} {builder} refit={refit} opaque={opaque}")
        occ = api.trace_rays(scene, rays, any_hit=True, opaque=opaque).occluded
        assert (occ == found).all(), f"any hit disagrees with the closest hit on {int((occ != found).sum())} rays"
        timed = api.trace_rays(scene, rays, opaque=opaque)
        assert_hits(timed, exp, f"{name} {builder} refit={refit} opaque={opaque}, timed form")
    cam = api.camera_rays(gpu_ctx, c.camera, W, H, SPP)
    r = api.trace_rays(scene, cam, collect_stats=True)
    assert r.stats.numRays == W * H * SPP
    assert_hits(r, cam_exp, f"{name} {builder} refit={refit} camera rays")
    if scene.stats().maxDepth > 16:
        _check_deep_rays(oracle, c, scene, ex, f"{name} {builder} refit={refit}", required=name == "graded")


# ---- deep rays: k_query_tail -------------------------------------------------------------------------------------------------------
def _overflowing(scene, pool, cap=48):
    """the rows of pool that k_query abandons (more than 16 stacked nodes), found by bisection over the counting form's tailRays"""
    found, todo = [], [(0, len(pool))]
    while todo and len(found) < cap:
        lo, hi = todo.pop()
        if api.trace_rays(scene, pool[lo:hi], collect_stats=True).stats.tailRays == 0:
            continue
        if hi - lo == 1:
            found.append(lo)
        else:
            mid = (lo + hi) // 2
            todo += [(mid, hi), (lo, mid)]
    return np.array(sorted(found), np.int64)


def _check_deep_rays(oracle, c, scene, ex, what, required):
    """A tree deeper than the 16-entry LDS stack: the rays that overflow it are walked again by k_query_tail and must still equal the
    brute force bit for bit, in the counting and the timed forms, closest and any hit.  A ray overflows only when it enters both
    children at 17 nested levels; on trees barely deeper than 16 (bunny's LBVH at 17, count_4097's SAH tree at 19) no candidate of the
    pool does, so only the graded line, whose rays down its length do, is required to find some."""
    pool = cs.deep_pool(c, 30000, seed=21, tree=ex)
    idx = _overflowing(scene, pool)
    assert len(idx) > 0 or not required, f"{what}: depth {scene.stats().maxDepth}, but no ray of the pool needs more than 16 stacked nodes"
    if len(idx) == 0:
        return
    deep = pool[idx]
    exp = brute_force(oracle, ex, deep)
    res = api.trace_rays(scene, deep, collect_stats=True)
    assert res.stats.tailRays == len(deep), (res.stats.tailRays, len(deep))
    assert_hits(res, exp, f"{what} deep rays")
    assert_hits(api.trace_rays(scene, deep), exp, f"{what} deep rays, timed form")
    occ = api.trace_rays(scene, deep, any_hit=True).occluded
    assert (occ == (exp[3] != MISS)).all()
    print(f"\n{what}: depth {scene.stats().maxDepth}, {len(deep)} tail rays, {int((exp[3] != MISS).sum())} of them hit")


# ---- rendering --------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,builder,refit", FORMS, ids=IDS)
def test_render_equals_oracle(gpu_ctx, oracle, made, scene_cache, queue_mode, name, builder, refit):
    c = _case(made, name)
    scene, ex = _scene(gpu_ctx, made, name, builder, refit)
    info = c.scene_info(1)
    for pipeline in (1, 2):
        key = (name, builder, refit, pipeline)
        if key not in _ref:
            p = api.make_params(W, H, spp=SPP, collect_stats=1, pipeline=pipeline)
            tree = oracle.render(c.desc, c.camera, info, p, bvh=ex, threads=16)
            bkey = (name, pipeline)
            if bkey not in _ref:
                _ref[bkey] = oracle.render(c.desc, c.camera, info, p, bvh=None, threads=16).images[A.IMAGE_SHADOWED]
            assert np.array_equal(tree.images[A.IMAGE_SHADOWED], _ref[bkey]), f"oracle over the {builder} tree != brute force"
            _ref[key] = tree
        ref = _ref[key]
        for collect in (0, 1):
            p = api.make_params(W, H, spp=SPP, collect_stats=collect, pipeline=pipeline)
            frame = api.Frame(gpu_ctx, W, api.shard_rows(H, 8, 1))
            try:
                api.render(scene, c.camera, info, p, frame)
                img, g = frame.download(), frame.stats()
            finally:
                frame.close()
            assert np.array_equal(img, ref.images[A.IMAGE_SHADOWED]), (pipeline, collect, int((img != ref.images[A.IMAGE_SHADOWED]).sum()))
            if collect:
                for f in ("numRays", "numPrimaryRays", "numShadowRays", "numHits", "numNodeVisits", "numTriTests",
                          "numShadowNodeVisits", "numShadowTriTests"):
                    assert getattr(g, f) == getattr(ref.stats, f), (pipeline, f, getattr(g, f), getattr(ref.stats, f))
