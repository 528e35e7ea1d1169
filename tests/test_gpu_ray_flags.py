"""The culling ray flags of the ray queries on the device (RTR_QUERY_CULL_BACK_FACING / FRONT_FACING / OPAQUE / NO_OPAQUE) against a
brute force of the test's own: test_gpu_cull_masks.all_hits' candidates (oracle_mt over the exported triangle records), each classed
by tests/ray_flags_witness.py — facing from the float32 restatement of rtr_mt_intersect's determinant XOR the instance's mirrored bit
(float64, from the descriptor), opacity from the record's flags bit 0 and RTR_QUERY_OPAQUE, the opacity-map verdict from the float32
restatement of alpha_pass — and filtered.  Every ray is compared, hits bit for bit, occlusion bytes byte for byte, on every route."""
import ctypes as C
import os
import shutil

import numpy as np
import pytest
import torch

from realtimeraytracer_amd import _abi as A
from realtimeraytracer_amd import api, host, scenes

import ray_flags_witness as W
from test_gpu_cull_masks import all_hits, by_custom, counters, leaves_of, scene_of, seeded_masks
from test_gpu_occlusion import assert_same_bytes, camera_light_rays, mixed_rays
from deep_scene import _deep_scene
from test_gpu_query import GOLD, MISS, assert_hits

pytestmark = pytest.mark.gpu

INVALID = -1
BACK, FRONT, C_OP, C_NOP, OPQ = A.QUERY_CULL_BACK_FACING, A.QUERY_CULL_FRONT_FACING, A.QUERY_CULL_OPAQUE, A.QUERY_CULL_NO_OPAQUE, A.QUERY_OPAQUE
SINGLE = [BACK, FRONT, C_OP, C_NOP]
PAIRS = [f | o for f in (BACK, FRONT) for o in (C_OP, C_NOP, OPQ)]


def _np(x):
    return x.cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)


def _kw(flags):
    """the Python keywords of a flags word"""
    return {"opaque": bool(flags & OPQ), "ray_flags": flags & ~OPQ}


def _features_with_a_real_alpha_layer(tmp_path):
    """test_gpu_query._features_setup with an opacity map that passes some candidates and rejects others (half 255, half 0; the
    constant 200 of that setup rejects every one, which would leave RTR_QUERY_CULL_NO_OPAQUE nothing to change)"""
    for f in ("features.obj", "features.mtl"):
        shutil.copy(os.path.join(GOLD, f), tmp_path / f)
    os.makedirs(tmp_path / "textures", exist_ok=True)
    for n in ("albedo", "spec", "metal"):
        scenes.write_png(str(tmp_path / "textures" / f"{n}.png"), np.full((4, 4, 3), 200, np.uint8))
    halves = np.zeros((4, 4, 3), np.uint8)
    halves[:, :2] = 255                     # two texel columns pass, two reject; the filter blends between them
    scenes.write_png(str(tmp_path / "textures" / "alpha.png"), halves)
    cwd = os.getcwd()
    os.chdir(tmp_path)
    try:
        hs = host.HostScene()
        hs.addObjMtlPair("features.obj", "")
        hs.setSky((0.5, 0.7, 1.0))
        hs.build()
    finally:
        os.chdir(cwd)
    return hs


def _scene(case, gpu_ctx, tmp_path, build=A.BUILD_HOST_SAH):
    if case != "features":
        return scene_of(case, gpu_ctx, tmp_path, build)
    hs = _features_with_a_real_alpha_layer(tmp_path)
    old = hs.desc.buildFlags
    hs.desc.buildFlags = build
    try:
        scene = api.Scene(gpu_ctx, hs.desc)
    finally:
        hs.desc.buildFlags = old
    return scene, hs.desc, hs, None


def _rays_for(case, gpu_ctx, scene, s, seed=31):
    st = scene.stats()
    diag = float(np.linalg.norm(np.array(st.boundsMax[:]) - np.array(st.boundsMin[:])))
    rays = mixed_rays(st, 300 if case == "sponza_mixed" else 1200, seed, diag)
    if s is not None:                   # rays that meet more of the scene: camera rays of a coarse frame
        rays = np.concatenate([rays, _np(api.camera_rays(gpu_ctx, s.camera, 16, 9, 1))]).astype(np.float32)
    return rays


def _routes(scene, rt, hints, **kw):
    return {"dense any": api.trace_rays(scene, rt, any_hit=True, **kw),
            "queued": api.trace_occlusion(scene, rt, **kw),
            "queued hinted": api.trace_occlusion(scene, rt, start_leaves=hints, **kw),
            "queued hinted, counting": api.trace_occlusion(scene, rt, start_leaves=hints, collect_stats=True, **kw)}


# ---- 1. flags 0 change nothing -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["sponza_mixed", "textured_room"])
def test_flags_0_change_nothing(gpu_ctx, scene_cache, tmp_path, case):
    scene, desc, keep, s = scene_of(case, gpu_ctx, tmp_path)
    st = scene.stats()
    rays, hits, lp, lr = camera_light_rays(gpu_ctx, scene, s, 160, 100, 0)
    diag = float(np.linalg.norm(np.array(st.boundsMax[:]) - np.array(st.boundsMin[:])))
    rnd = torch.from_numpy(mixed_rays(st, 50000, 3, diag)).cuda()
    for name, r in (("camera", rays), ("light", lr), ("random", rnd)):
        for opaque in (False, True):
            a = api.trace_rays(scene, r, opaque=opaque, collect_stats=True)
            b = api.trace_rays(scene, r, opaque=opaque, collect_stats=True, ray_flags=0)
            assert torch.equal(a.hits, b.hits) and counters(a.stats) == counters(b.stats), f"{case} {name}: dense closest"
            a = api.trace_rays(scene, r, any_hit=True, opaque=opaque, collect_stats=True)
            b = api.trace_rays(scene, r, any_hit=True, opaque=opaque, collect_stats=True, ray_flags=0)
            assert_same_bytes(b.occluded, a.occluded, f"{case} {name}: dense any")
            assert counters(a.stats) == counters(b.stats), f"{case} {name}: dense any counters"
            a = api.trace_occlusion(scene, r, opaque=opaque, collect_stats=True)
            b = api.trace_occlusion(scene, r, opaque=opaque, collect_stats=True, ray_flags=0)
            assert_same_bytes(b.occluded, a.occluded, f"{case} {name}: queued")
            assert counters(a.stats) == counters(b.stats), f"{case} {name}: queued counters"
            hn = leaves_of(scene, r)
            a = api.trace_occlusion(scene, r, opaque=opaque, collect_stats=True, start_leaves=hn)
            b = api.trace_occlusion(scene, r, opaque=opaque, collect_stats=True, start_leaves=hn, ray_flags=0)
            assert_same_bytes(b.occluded, a.occluded, f"{case} {name}: queued hinted")
            assert counters(a.stats) == counters(b.stats), f"{case} {name}: queued hinted counters"
            # a masked call without flags is the masked call it was
            m = api.trace_rays(scene, r, opaque=opaque, collect_stats=True, cull_mask=0xff, ray_flags=0)
            assert counters(m.stats) == counters(api.trace_rays(scene, r, opaque=opaque, collect_stats=True).stats)


# ---- 2. each flag and each legal pair against the filtered brute force -----------------------------------------------------------
@pytest.mark.parametrize("build", [A.BUILD_HOST_SAH, A.BUILD_DEVICE_LBVH], ids=["host_sah", "device_lbvh"])
@pytest.mark.parametrize("case", ["features", "textured_room", "sponza_mixed"])
def test_each_flag_equals_the_filtered_brute_force(gpu_ctx, oracle, scene_cache, tmp_path, case, build):
    scene, desc, keep, s = _scene(case, gpu_ctx, tmp_path, build)
    rays = _rays_for(case, gpu_ctx, scene, s)
    rt = torch.from_numpy(rays).cuda()
    bvh = scene.export_bvh()
    cands = all_hits(oracle, bvh, rays)
    classes = W.classify(cands, rays, bvh, W.mirrored_by_custom(desc), W.AlphaWitness(desc))
    fronts = {f for c in classes for f in c[0]}
    assert fronts == {True, False}, "both facing classes must occur among the candidates"
    assert {b for c in classes for b in c[1]} == {True, False}, "both opacity classes must occur among the candidates"
    hints = leaves_of(scene, rt)
    assert int((hints != 0).sum()) > 0
    plain, plain_occ = W.filtered(cands, classes, rays, 0)
    assert_hits(api.trace_rays(scene, rt), plain, f"{case}: no flags, opacity maps tested")
    for name, res in _routes(scene, rt, hints).items():
        assert_same_bytes(res.occluded, plain_occ, f"{case}: no flags: {name}")
    for flags in SINGLE + PAIRS:
        what = f"{case} flags {flags:#x}"
        exp, occ = W.filtered(cands, classes, rays, flags)
        if flags in SINGLE:
            assert (exp[3] != plain[3]).any() or (exp[4] != plain[4]).any(), f"{what}: the flag must change some closest hit"
        assert_hits(api.trace_rays(scene, rt, **_kw(flags)), exp, what)
        assert_hits(api.trace_rays(scene, rt, collect_stats=True, **_kw(flags)), exp, what + ", counting form")
        for name, res in _routes(scene, rt, hints, **_kw(flags)).items():
            assert_same_bytes(res.occluded, occ, f"{what}: {name}")


# ---- 3. a mirrored instance ----------------------------------------------------------------------------------------------------------
def test_a_mirrored_instance_keeps_its_object_space_facing(gpu_ctx, oracle, scene_cache, tmp_path):
    s = scenes.cornell_box(96, 64)
    d = s.desc
    n = d.numInstances
    before = W.mirrored_by_custom(d)
    pick = next(i for i in range(n) if d.instances[i].customIndex >= s.num_lights + 2 and not before[d.instances[i].customIndex])
    inst = (A.RtrInstance * n)(*[A.RtrInstance.from_buffer_copy(d.instances[i]) for i in range(n)])
    orig = [A.RtrInstance.from_buffer_copy(x) for x in inst]
    # mirror about the plane x = c through the instance's own origin column: negate the first row of the 3x4 (x' = -x + 2c)
    c = inst[pick].transform[3]
    for k in range(3):
        inst[pick].transform[k] = -inst[pick].transform[k]
    inst[pick].transform[3] = c
    old = C.cast(d.instances, C.POINTER(A.RtrInstance))
    d.instances = inst
    try:
        scene = api.Scene(gpu_ctx, d)
        mirrored = W.mirrored_by_custom(d)
    finally:
        d.instances = old
    assert mirrored.sum() == before.sum() + 1 and mirrored[inst[pick].customIndex]
    st = scene.stats()
    rays = mixed_rays(st, 2500, 13, 1500.0)
    rt = torch.from_numpy(rays).cuda()
    hints = leaves_of(scene, rt)
    alpha = W.AlphaWitness(d)

    def check(sc, mir, what):
        bvh = sc.export_bvh()
        raw = np.frombuffer(bvh[1], dtype=np.uint32).reshape(-1, 12)
        assert not (raw[:, 11] & ~np.uint32(1)).any(), f"{what}: the mirrored bit must not show in the records' flags word"
        cands = all_hits(oracle, bvh, rays)
        classes = W.classify(cands, rays, bvh, mir, alpha)
        on_pick = sum(1 for cd in cands for cu in cd[3] if cu == inst[pick].customIndex)
        assert on_pick > 20, "rays must meet the instance"
        differ = 0
        for flags in (BACK, FRONT):
            exp, occ = W.filtered(cands, classes, rays, flags)
            wrong = W.filtered(cands, W.classify(cands, rays, bvh, before if mir is mirrored else mirrored, alpha), rays, flags)[0]
            differ += int((exp[3] != wrong[3]).sum())
            assert_hits(api.trace_rays(sc, rt, ray_flags=flags), exp, f"{what} flags {flags:#x}")
            for name, res in _routes(sc, rt, hints if sc is scene else leaves_of(sc, rt), ray_flags=flags).items():
                assert_same_bytes(res.occluded, occ, f"{what} flags {flags:#x}: {name}")
        assert differ > 0, "the mirrored bit must matter to some ray"

    check(scene, mirrored, "mirrored")
    flags_word = np.frombuffer(scene.export_bvh()[1], dtype=np.uint32).reshape(-1, 12)[:, 11].copy()
    scene.update_instances(orig)                    # un-mirrored: the table follows the update
    assert np.array_equal(np.frombuffer(scene.export_bvh()[1], dtype=np.uint32).reshape(-1, 12)[:, 11], flags_word)
    check(scene, before, "after rtr_scene_update_instances")
    twin = api.Scene(gpu_ctx, d, like=scene)      # rtr_scene_create_like evaluates the bit from ITS description
    check(twin, before, "rtr_scene_create_like")


# ---- 4. agreement with rtr_hit_surfaces -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["cornell_box", "textured_room", "sponza_mixed"])
def test_facing_agrees_with_the_geometric_normal_of_hit_surfaces(gpu_ctx, scene_cache, case):
    s = getattr(scenes, case)(160, 100)
    scene = api.Scene(gpu_ctx, s.desc)
    st = scene.stats()
    diag = float(np.linalg.norm(np.array(st.boundsMax[:]) - np.array(st.boundsMin[:])))
    cam = api.camera_rays(gpu_ctx, s.camera, 160, 100, 1)
    rnd = torch.from_numpy(mixed_rays(st, 20000, 5, diag)).cuda()
    mirrored = W.mirrored_by_custom(s.desc)
    raw = np.frombuffer(scene.export_bvh()[1], dtype=np.uint32).reshape(-1, 12)
    flt = raw.view(np.float32)
    where = {(int(c), int(p)): j for j, (c, p) in enumerate(zip(raw[:, 3], raw[:, 7]))}
    kinds = set()
    for name, rt in (("camera", cam), ("random", rnd)):
        hits = api.trace_rays(scene, rt)
        surf = api.hit_surfaces(scene, rt, hits)
        r = _np(rt)
        cu, pr = _np(hits.custom_index), _np(hits.primitive_id)
        hit = np.nonzero(cu >= 0)[0]
        js = np.array([where[(int(cu[k]), int(pr[k]))] for k in hit])
        a = W.det32(r[hit, 4:7], flt[js, 4:7], flt[js, 8:11])
        front = (a > 0) != mirrored[cu[hit]]
        gn = _np(surf.geom_normal)[hit].astype(np.float64)
        dirs = r[hit, 4:7].astype(np.float64)
        dot = np.einsum("ij,ij->i", dirs, gn)
        judged = np.abs(dot) > 1e-5 * np.linalg.norm(dirs, axis=1)
        if name == "camera":
            assert 1.0 - judged.mean() < 0.01, f"{case}: {1.0 - judged.mean():.4f} of the camera hits are too close to edge-on to judge"
        assert ((dot < 0) == front)[judged].all(), f"{case} {name}: front-facing means the ray goes against geomNormal"
        kinds |= set(_np(surf.kind)[hit].tolist())
        assert front.any()
    assert {A.SURFACE_OBJECT, A.SURFACE_LIGHT} <= kinds, "objects and lights must both be hit"


# ---- 5. composition with cull masks and per-ray masks -----------------------------------------------------------------------------
def test_flags_compose_with_instance_masks_and_ray_masks(gpu_ctx, oracle, scene_cache, tmp_path):
    scene, desc, keep, s = scene_of("textured_room", gpu_ctx, tmp_path)
    rays = _rays_for("textured_room", gpu_ctx, scene, s, seed=57)
    rt = torch.from_numpy(rays).cuda()
    masks = seeded_masks(desc.numInstances, 303)
    scene.set_instance_masks(masks)
    cm = by_custom(desc, masks)
    bvh = scene.export_bvh()
    cands = all_hits(oracle, bvh, rays)
    classes = W.classify(cands, rays, bvh, W.mirrored_by_custom(desc), W.AlphaWitness(desc))
    hints = leaves_of(scene, rt)
    rm = np.array([0xff, 0x0f, 0xf0, 0x01, 0x00], np.uint8)[np.random.default_rng(2).integers(0, 5, len(rays))]
    rmt = torch.from_numpy(rm).cuda()
    for flags, cull in ((BACK, 0x5a), (FRONT | C_NOP, 0xff), (C_OP, 0x3c)):
        exp, occ = W.filtered(cands, classes, rays, flags, cm, rm.astype(np.int64) & cull)
        only_mask = W.filtered(cands, classes, rays, 0, cm, rm.astype(np.int64) & cull)[0]
        only_flag = W.filtered(cands, classes, rays, flags)[0]
        assert (exp[3] != only_mask[3]).any() and (exp[3] != only_flag[3]).any(), "both filters must matter"
        what = f"flags {flags:#x} cull {cull:#x}"
        assert_hits(api.trace_rays(scene, rt, cull_mask=cull, ray_masks=rmt, **_kw(flags)), exp, what)
        for name, res in _routes(scene, rt, hints, cull_mask=cull, ray_masks=rmt, **_kw(flags)).items():
            assert_same_bytes(res.occluded, occ, f"{what}: {name}")


# ---- 6. deep rays ---------------------------------------------------------------------------------------------------------------------
def test_deep_rays_honour_the_flags_in_both_tails(gpu_ctx, oracle):
    """test_gpu_cull_masks' deep-ray method: the brute force is the oracle's O(N) loop on the scene with the culled instances moved out
    of reach.  All triangles of an instance of this scene share one plane and one winding, so a facing flag culls, for one ray, the
    whole instance or nothing of it: the test restates the determinant per ray and instance and picks, per ray, the run of the oracle
    with exactly that ray's culled instances away."""
    d, keep, scene, cam = _deep_scene(gpu_ctx)
    inst = keep[3]
    W_, H, S = 16, 8, 1
    end = float(1 << 19) * 0.01
    back = host.Camera(0.004, (end + 0.5, -0.995, 0.0), (0.2 * end, -1.0, 0.0), (0.0, 1.0, 0.0), W_, H).getGPUData()
    rays = torch.cat([api.camera_rays(gpu_ctx, c, W_, H, S) for c in (cam, back)])
    r = _np(rays)
    raw = np.frombuffer(scene.export_bvh()[1], dtype=np.uint32).reshape(-1, 12)
    flt = raw.view(np.float32)
    p = api.make_params(W_, H, spp=S)
    front = np.zeros((2, len(r)), bool)
    for ci in range(2):
        rec = flt[raw[:, 3] == ci]
        a0, a1 = W.det32(r[:, 4:7], np.broadcast_to(rec[0, 4:7], (len(r), 3)), np.broadcast_to(rec[0, 8:11], (len(r), 3))), \
            W.det32(r[:, 4:7], np.broadcast_to(rec[-1, 4:7], (len(r), 3)), np.broadcast_to(rec[-1, 8:11], (len(r), 3)))
        assert ((a0 > 0) == (a1 > 0)).all()
        front[ci] = a0 > 0                                          # identity transforms: nothing is mirrored
    runs = {}
    for away in ((False, False), (True, False), (False, True), (True, True)):
        for i in range(2):
            inst[i].transform[7] = 1.0e7 if away[i] else 0.0        # y translation: far beyond tmax = 10000
        try:
            parts = [oracle.primary_hits(d, c, p, bvh=None, threads=16) for c in (cam, back)]
        finally:
            for i in range(2):
                inst[i].transform[7] = 0.0
        runs[away] = tuple(np.concatenate([x[k] for x in parts]) for k in range(5))
    changed = dense_tail = queued_tail = 0
    for flags in (BACK, FRONT):
        culled = ~front if flags == BACK else front                 # (instance, ray)
        sel = [runs[(bool(culled[0, k]), bool(culled[1, k]))] for k in range(len(r))]
        t, u, v, cu, pr = (np.array([sel[k][j][k] for k in range(len(r))]) for j in range(5))
        exp = (np.where(cu == MISS, np.float32(10000.0), t).astype(np.float32), u.astype(np.float32), v.astype(np.float32), cu.astype(np.int64), pr.astype(np.int64))
        occ = (cu != MISS).astype(np.uint8)
        changed += int((cu != runs[(False, False)][3]).sum())
        res = api.trace_rays(scene, rays, collect_stats=True, ray_flags=flags)
        assert res.stats.tailRays > 0, "the rays must go through k_query_tail"
        assert_hits(res, exp, f"deep rays, flags {flags:#x}")
        assert_hits(api.trace_rays(scene, rays, ray_flags=flags), exp, f"deep rays, flags {flags:#x}, timed form")
        a = api.trace_rays(scene, rays, any_hit=True, collect_stats=True, ray_flags=flags)
        assert_same_bytes(a.occluded, occ, f"deep rays, dense any, flags {flags:#x}")
        q = api.trace_occlusion(scene, rays, collect_stats=True, ray_flags=flags)
        assert_same_bytes(q.occluded, occ, f"deep rays, queued, flags {flags:#x}")
        assert_same_bytes(api.trace_occlusion(scene, rays, ray_flags=flags).occluded, occ, f"deep rays, queued, timed, flags {flags:#x}")
        dense_tail += int(a.stats.tailRays)
        queued_tail += int(q.stats.tailRays)
    assert dense_tail > 0, "the dense any-hit walk must have sent rays through k_query_tail under a face flag"
    assert queued_tail > 0, "the queued walk must have sent rays through the occlusion tail under a face flag"
    assert changed > 0, "the flags must change some deep ray's hit"
    # the opacity filter in the tails: every record of this scene is opaque, so RTR_QUERY_CULL_OPAQUE leaves nothing (no walk ends
    # early: every route's deep rays reach its tail) and RTR_QUERY_CULL_NO_OPAQUE leaves everything
    n = len(r)
    t0, u0, v0, cu0, pr0 = runs[(False, False)]
    cases = {C_NOP: ((np.where(cu0 == MISS, np.float32(10000.0), t0).astype(np.float32), u0.astype(np.float32), v0.astype(np.float32),
                      cu0.astype(np.int64), pr0.astype(np.int64)), (cu0 != MISS).astype(np.uint8)),
             C_OP: ((np.full(n, 10000.0, np.float32), np.zeros(n, np.float32), np.zeros(n, np.float32), np.full(n, MISS, np.int64),
                     np.full(n, MISS, np.int64)), np.zeros(n, np.uint8))}
    for flags, (exp, occ) in cases.items():
        res = api.trace_rays(scene, rays, collect_stats=True, ray_flags=flags)
        assert res.stats.tailRays > 0
        assert_hits(res, exp, f"deep rays, flags {flags:#x}")
        assert_hits(api.trace_rays(scene, rays, ray_flags=flags), exp, f"deep rays, flags {flags:#x}, timed form")
        a = api.trace_rays(scene, rays, any_hit=True, collect_stats=True, ray_flags=flags)
        q = api.trace_occlusion(scene, rays, collect_stats=True, ray_flags=flags)
        assert_same_bytes(a.occluded, occ, f"deep rays, dense any, flags {flags:#x}")
        assert_same_bytes(q.occluded, occ, f"deep rays, queued, flags {flags:#x}")
        assert_same_bytes(api.trace_occlusion(scene, rays, ray_flags=flags).occluded, occ, f"deep rays, queued, timed, flags {flags:#x}")
        if flags == C_OP:
            assert a.stats.tailRays > 0, "with every record culled the dense any-hit walk's deep rays reach k_query_tail"
            assert q.stats.tailRays > 0, "with every record culled the queued walk's deep rays reach the occlusion tail"


# ---- 7. counters ---------------------------------------------------------------------------------------------------------------------
def test_culled_records_run_no_opacity_test_and_count_as_fetched(gpu_ctx, scene_cache, tmp_path):
    scene, desc, keep, s = scene_of("sponza_mixed", gpu_ctx, tmp_path)
    rays, hits, lp, lr = camera_light_rays(gpu_ctx, scene, s, 160, 100, 0)
    for r in (rays, lr):
        for route in ("closest", "dense any", "queued"):
            def run(flags):
                if route == "queued":
                    return api.trace_occlusion(scene, r, collect_stats=True, ray_flags=flags).stats
                return api.trace_rays(scene, r, any_hit=route == "dense any", collect_stats=True, ray_flags=flags).stats
            base = run(0)
            assert base.numAlphaTests > 0
            assert run(C_NOP).numAlphaTests == 0, f"{route}: a culled record must not be alpha-tested"
            assert run(C_NOP).numTriTests > 0
            if route != "closest":
                assert run(C_OP).numAlphaTests > 0, f"{route}: the alpha-tested layer alone still runs its opacity tests"
            for flags in SINGLE:
                assert run(flags).numRays == base.numRays


# ---- 8. the use case: emitters seen from behind -------------------------------------------------------------------------------------
def test_bounce_rays_pass_through_one_sided_lights_from_behind(gpu_ctx, scene_cache, tmp_path):
    s = scenes.textured_room(160, 100)
    desc, nl = s.desc, s.num_lights
    # the workload's lights are two-sided: the test's copy of the light table makes them one-sided emitters (isTwoSided = 0), which
    # changes what they emit and nothing about the geometry the rays meet
    lights = (A.RtrAreaLightInfo * nl)(*[A.RtrAreaLightInfo.from_buffer_copy(desc.lights[l]) for l in range(nl)])
    for l in range(nl):
        lights[l].isTwoSided = 0
    old = C.cast(desc.lights, C.POINTER(A.RtrAreaLightInfo))
    desc.lights = lights
    try:
        scene = api.Scene(gpu_ctx, desc)
    finally:
        desc.lights = old
    one_sided = np.array([lights[l].isTwoSided == 0 for l in range(nl)])
    assert nl > 0 and one_sided.all()
    lr = camera_light_rays(gpu_ctx, scene, s, 160, 100, 0)[3]
    # the bounce set: the frame's light rays, sent on past their light (tmax 10000).  The room's lights face into it, so those rays reach
    # them from the front; rays that reach a one-sided light from behind are added: aimed, from seeded distances behind it, at seeded
    # points of its exported triangles (behind = against the side the as-wound object-space normal points to: the world-space
    # cross(e1, e2) of the record, turned over for a mirrored light instance)
    live = lr[lr[:, 4:7].abs().sum(1) > 0]
    fwd = live.clone(); fwd[:, 7] = 10000.0
    raw = np.frombuffer(scene.export_bvh()[1], dtype=np.uint32).reshape(-1, 12)
    flt = raw.view(np.float32)
    mirrored = W.mirrored_by_custom(desc)
    on = raw[:, 3] < nl
    lt, lt_mirrored = flt[on], mirrored[raw[on, 3]]
    assert len(lt)
    rng = np.random.default_rng(8)
    m = 600
    pick = rng.integers(0, len(lt), m)
    b = rng.uniform(0.05, 0.45, (m, 2))
    tgt = lt[pick, 0:3] + lt[pick, 4:7] * b[:, :1] + lt[pick, 8:11] * b[:, 1:]
    nrm = np.cross(lt[pick, 4:7].astype(np.float64), lt[pick, 8:11].astype(np.float64))
    size = np.sqrt(np.linalg.norm(nrm, axis=1))[:, None]
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    nrm[lt_mirrored[pick]] *= -1.0
    h = size * (10.0 ** rng.uniform(-3.0, 0.5, (m, 1)))
    aimed = np.zeros((m, 8), np.float32)
    aimed[:, 0:3], aimed[:, 3], aimed[:, 4:7], aimed[:, 7] = tgt - nrm * h, 0.0, nrm, 10000.0
    bounce = torch.cat([fwd, torch.from_numpy(aimed).cuda()]).contiguous()

    def on_a_one_sided_lights_back(res):
        surf = api.hit_surfaces(scene, bounce, res)
        cu = _np(res.custom_index)
        light = (cu >= 0) & (cu < nl)
        light[light] &= one_sided[cu[light]]
        dot = np.einsum("ij,ij->i", _np(bounce)[:, 4:7].astype(np.float64), _np(surf.geom_normal).astype(np.float64))
        return light & (dot > 0)                                    # the ray runs along the normal: it arrived from behind

    before = api.trace_rays(scene, bounce)
    assert on_a_one_sided_lights_back(before).sum() > 0, "without the flag some bounce rays end on a one-sided light's back"
    after = api.trace_rays(scene, bounce, ray_flags=BACK)
    assert on_a_one_sided_lights_back(after).sum() == 0
    moved = on_a_one_sided_lights_back(before)
    assert (_np(after.t)[moved] > _np(before.t)[moved]).all(), "what lies behind the light"


# ---- 9. invalid arguments ---------------------------------------------------------------------------------------------------------
def test_invalid_arguments(gpu_ctx, scene_cache):
    s = scenes.cornell_box(64, 64)
    scene = api.Scene(gpu_ctx, s.desc)
    lib, ctx = gpu_ctx.lib, gpu_ctx.h
    rays = api.camera_rays(gpu_ctx, s.camera, 8, 8, 1)
    hits = torch.empty((64, 8), dtype=torch.int32, device="cuda")
    occ = torch.empty(64 + 16, dtype=torch.uint8, device="cuda")
    need = api.occlusion_scratch_bytes(lib, 64)
    scratch = torch.empty(need + 16, dtype=torch.uint8, device="cuda")
    rp, hp, op, sp = A.VP(rays.data_ptr()), A.VP(hits.data_ptr()), A.VP(occ.data_ptr()), A.VP(scratch.data_ptr())
    families = {
        "rtr_trace_rays": lambda f: lib.rtr_trace_rays(ctx, scene.h, rp, 64, f, hp, op, None),
        "rtr_trace_rays_async": lambda f: lib.rtr_trace_rays_async(ctx, scene.h, rp, 64, f, hp, op),
        "rtr_trace_rays_masked": lambda f: lib.rtr_trace_rays_masked(ctx, scene.h, rp, None, 64, f, 0xff, hp, op, None),
        "rtr_trace_rays_masked_async": lambda f: lib.rtr_trace_rays_masked_async(ctx, scene.h, rp, None, 64, f, 0xff, hp, op),
        "rtr_trace_occlusion": lambda f: lib.rtr_trace_occlusion(ctx, scene.h, rp, 64, f, sp, need, op, None),
        "rtr_trace_occlusion_async": lambda f: lib.rtr_trace_occlusion_async(ctx, scene.h, rp, 64, f, sp, need, op),
        "rtr_trace_occlusion_hinted": lambda f: lib.rtr_trace_occlusion_hinted(ctx, scene.h, rp, None, 64, f, sp, need, op, None),
        "rtr_trace_occlusion_hinted_async": lambda f: lib.rtr_trace_occlusion_hinted_async(ctx, scene.h, rp, None, 64, f, sp, need, op),
        "rtr_trace_occlusion_masked": lambda f: lib.rtr_trace_occlusion_masked(ctx, scene.h, rp, None, None, 64, f, 0xff, sp, need, op, None),
        "rtr_trace_occlusion_masked_async": lambda f: lib.rtr_trace_occlusion_masked_async(ctx, scene.h, rp, None, None, 64, f, 0xff, sp, need, op),
    }
    for name, call in families.items():
        for f in (4, 8, 0x100, BACK | 4, 0x80000000):
            assert call(f) == INVALID, f"{name} flags {f:#x}"
            err = lib.rtr_last_error()
            assert b"flag" in err and name.encode() in err, (name, f, err)
        assert call(BACK | FRONT) == INVALID
        assert b"RTR_QUERY_CULL_BACK_FACING" in lib.rtr_last_error() and b"RTR_QUERY_CULL_FRONT_FACING" in lib.rtr_last_error()
        for a, b in ((OPQ, C_OP), (OPQ, C_NOP), (C_OP, C_NOP)):
            assert call(a | b) == INVALID, f"{name} flags {a | b:#x}"
            err = lib.rtr_last_error()
            for bit, word in ((OPQ, b"RTR_QUERY_OPAQUE"), (C_OP, b"RTR_QUERY_CULL_OPAQUE"), (C_NOP, b"RTR_QUERY_CULL_NO_OPAQUE")):
                if (a | b) & bit:
                    assert word in err, (name, err)
        assert call(OPQ | C_OP | C_NOP | BACK) == INVALID
        for f in SINGLE + PAIRS:
            assert call(f) == 0, f"{name} flags {f:#x}: {lib.rtr_last_error()}"
    torch.cuda.synchronize()
    with pytest.raises(api.RtrError):
        api.trace_rays(scene, rays, ray_flags=4)
    with pytest.raises(ValueError):
        api.trace_rays(scene, rays, ray_flags=BACK | FRONT)
    with pytest.raises(ValueError):
        api.trace_occlusion(scene, rays, opaque=True, ray_flags=C_NOP)


# ---- 10. the composed stage ----------------------------------------------------------------------------------------------------------
def test_direct_light_passes_the_shadow_ray_flags_to_every_route(gpu_ctx, scene_cache, tmp_path):
    scene, desc, keep, s = scene_of("textured_room", gpu_ctx, tmp_path)
    rays = api.camera_rays(gpu_ctx, s.camera, 96, 64, 1)
    lp = api.make_light_params(s.num_lights, 3, 0, 96, 1)
    base = api.direct_light(scene, rays, params=lp).raw
    changed = 0
    for flags in (FRONT, C_NOP, BACK | C_OP):
        out = {}
        for route in ("dense", "queued", "queued_own_leaf"):
            assert torch.equal(api.direct_light(scene, rays, params=lp, occlusion=route, shadow_ray_flags=0).raw, base), f"{route}: 0 is the call as before"
            out[route] = api.direct_light(scene, rays, params=lp, occlusion=route, shadow_ray_flags=flags).raw
        assert torch.equal(out["dense"], out["queued"]) and torch.equal(out["dense"], out["queued_own_leaf"]), f"flags {flags:#x}"
        assert bool((out["dense"][:, 0:3] >= base[:, 0:3]).all()), "fewer occluders never darken"
        changed += int(not torch.equal(out["dense"], base))
    assert changed > 0, "culled shadow casters must brighten some pixels"
